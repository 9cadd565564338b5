"""CPU tests of vsm.Absorption's host side and of tests/absorption_oracle.py, the reference the GPU tests compare against.

read_hitran: the values of the reference's own read_hitran testset (test/test_Absorption.jl:15-71) on its 16-line test file.
Complex error functions: the oracle's three against scipy.special.wofz on x in [0, 40] x y in [1e-5, 20]; the bounds are the measured
maxima of the relative error of Re w, times 2 -- the approximations' own error.
Limits: Voigt against Lorentz (y large) and Doppler (y small), the normalisation of one line, the spline of qoft, the one deviation
from the reference, and the host bookkeeping of compute_absorption_profile with the device replaced by the oracle."""
import math

import numpy as np
import pytest

import absorption_cases as AC
import absorption_oracle as AO

GOLDEN_PAR = AC.GOLDEN_PAR

# measured maxima of |Re w - Re wofz| / Re wofz on the grid below: 8.37e-5 (at 11.75 + 3.26i, Humlicek region I just above
# |x| + y = 15), 2.28e-6 (at 5.15 + 2.89i, Humlicek region II just above 8), 8.30e-3 (at 2.5 + 0.047i, CPF12 at small y)
CEF_BOUND = {"HumlicekWeidemann32VoigtErrorFunction": 2 * 8.37e-5, "HumlicekWeidemann32SDErrorFunction": 2 * 2.28e-6,
             "CPF12ErrorFunction": 2 * 8.30e-3}


@pytest.fixture(scope="module")
def A():
    import vsmartmom_jl_amd as v
    return v.Absorption


# ---- read_hitran ---------------------------------------------------------------------------------------------------------------------
def test_read_hitran_fields_of_the_four_lines(A):
    ht = A.read_hitran(GOLDEN_PAR, mol=2, iso=1, ν_min=6000, ν_max=6400)
    assert ht.mol.tolist() == [2, 2, 2, 2] and ht.mol.dtype == np.int64
    assert ht.iso.tolist() == [1, 1, 1, 1] and ht.iso.dtype == np.int64
    assert ht.nu.tolist() == [6000.542970, 6286.403343, 6317.417493, 6380.824116] and ht.nu.dtype == np.float64
    assert ht.S.tolist() == [1.098E-28, 9.843E-30, 5.613E-27, 1.809E-30]
    assert ht.A.tolist() == [9.993e-08, 1.179e-08, 1.324e-05, 1.601e-02]
    assert ht.gamma_air.tolist() == [.0880, .0687, .0682, .0671]
    assert ht.gamma_self.tolist() == [0.118, 0.087, 0.081, 0.073]
    assert ht.E_low.tolist() == [7.8043, 464.1717, 639.6004, 3798.2095]
    assert ht.n_air.tolist() == [0.77, 0.76, 0.76, 0.73]
    assert ht.delta_air.tolist() == [-.004342, -.007362, -.007443, -.007669]
    assert ht.global_upper_quanta == ["       4 1 1 03", "       2 2 2 12", "       2 2 2 12", "       4 2 2 12"]
    assert ht.global_lower_quanta == ["       0 0 0 01", "       0 0 0 01", "       0 0 0 01", "       1 2 2 01"]
    assert ht.local_upper_quanta == ["               "] * 4
    assert ht.local_lower_quanta == ["     Q  4e     ", "     Q 34e     ", "     R 40e     ", "     R 51f     "]
    assert ht.ierr == ["367774", "367764", "367764", "367774"]
    assert ht.iref == ["2029 5 4 5 7"] * 4
    assert ht.line_mixing_flag == [" "] * 4
    assert ht.g_upper.tolist() == [9.0, 69.0, 83.0, 105.0]
    assert ht.g_lower.tolist() == [9.0, 69.0, 81.0, 103.0]


def test_read_hitran_filters(A):
    ht = A.read_hitran(GOLDEN_PAR, iso=1, ν_min=6000, ν_max=6400)
    assert ht.mol.tolist() == [1, 2, 2, 2, 2] and ht.iso.tolist() == [1, 1, 1, 1, 1]
    assert ht.nu.tolist() == [6286.403343, 6000.542970, 6286.403343, 6317.417493, 6380.824116]
    assert ht.g_lower.tolist() == [69.0, 9.0, 69.0, 81.0, 103.0]
    ht = A.read_hitran(GOLDEN_PAR, mol=2, ν_min=6000, ν_max=6400)
    assert ht.mol.tolist() == [2, 2, 2, 2, 2] and ht.iso.tolist() == [2, 1, 1, 1, 1]
    assert ht.nu.tolist() == [6000.542970, 6000.542970, 6286.403343, 6317.417493, 6380.824116]
    assert ht.g_lower.tolist() == [9.0, 9.0, 69.0, 81.0, 103.0]
    ht = A.read_hitran(GOLDEN_PAR, ν_min=6000, ν_max=6400)
    assert ht.mol.tolist() == [1, 2, 2, 2, 2, 2] and ht.iso.tolist() == [1, 2, 1, 1, 1, 1]
    assert ht.nu.tolist() == [6286.403343, 6000.542970, 6000.542970, 6286.403343, 6317.417493, 6380.824116]
    assert ht.g_lower.tolist() == [69.0, 9.0, 9.0, 69.0, 81.0, 103.0]
    assert len(A.read_hitran(GOLDEN_PAR, mol=2, iso=1, ν_max=6400)) == 9
    assert len(A.read_hitran(GOLDEN_PAR, mol=2, iso=1, ν_min=6000)) == 7
    assert len(A.read_hitran(GOLDEN_PAR, mol=2, iso=1)) == 12
    with pytest.raises(A.HitranEmptyError):
        A.read_hitran(GOLDEN_PAR, mol=9)


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def test_unbuilt_error_functions_and_missing_isotopologues_raise(A):
    import vsmartmom_jl_amd as vsm
    for name in ("ErfcHumliErrorFunctionVoigt", "ErfcHumliErrorFunctionSD", "ErfcErrorFunction", "HumlicekErrorFunction"):
        with pytest.raises(NotImplementedError):
            getattr(A, name)()
    assert A.absorption_cross_section is A.compute_absorption_cross_section
    t = AC.synthetic_table(3, 5, two_species=True)
    t["mol"][:] = [2, 7, 2, 7, 2]
    iso = AC.isotopologues(A)
    del iso[(7, 1)]
    with pytest.raises(vsm.VSMError, match=r"\(7, 1\)"):
        A.make_hitran_model(AC.hitran_table(A, t), A.Voigt(), isotopologues=iso)
    m = AC.make_model(A, t)
    assert isinstance(m.CEF, A.HumlicekWeidemann32SDErrorFunction) and m.wing_cutoff == 5.0
    assert A.make_hitran_model(AC.hitran_table(A, t), A.Voigt(), isotopologues=AC.isotopologues(A)).wing_cutoff == 40.0
    with pytest.raises(vsm.VSMError, match="between"):          # the reference's assertion Tmin < T < Tmax
        A.qoft(AC.isotopologues(A)[(2, 1)], 99.0)
    with pytest.raises(vsm.VSMError, match="ascending"):
        A.compute_absorption_cross_section(m, [6030.0, 6020.0], 500.0, 250.0)


# ---- complex error functions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cef", AO.CEFS)
def test_oracle_cef_against_wofz(cef):
    wofz = pytest.importorskip("scipy.special").wofz
    X, Y = np.meshgrid(np.linspace(0.0, 40.0, 801), np.geomspace(1e-5, 20.0, 121))
    z = (X + 1j * Y).ravel()
    ref = wofz(z)
    got = AO.w(cef, z)
    err = np.abs(got.real - ref.real) / ref.real
    k = int(np.argmax(err))
    print("%s: max rel err of Re w %.3e at z = %r; of w %.3e" % (cef, err[k], z[k], np.max(np.abs(got - ref) / np.abs(ref))))
    assert err[k] <= CEF_BOUND[cef]
    neg = AO.w(cef, -z.real + 1j * z.imag)                       # Re w is even in x (the sums run in another order there)
    np.testing.assert_allclose(neg.real, got.real, rtol=1e-9, atol=0)


# ---- limits --------------------------------------------------------------------------------------------------------------------------
def _one_line(gamma_air, delta=0.0, E_low=-1.0, S=1e-22, nu=6025.0):
    return dict(mol=np.array([2]), iso=np.array([1]), nu=np.array([nu]), S=np.array([S]), gamma_air=np.array([gamma_air]),
                gamma_self=np.array([gamma_air]), n_air=np.array([0.7]), delta_air=np.array([delta]), E_low=np.array([E_low]))


@pytest.mark.parametrize("cef", AO.CEFS[:2])
def test_voigt_tends_to_lorentz_for_large_y(cef):
    """Re w(x + i y) = y / (sqrt(pi) (x^2 + y^2)) (1 + (3 x^2 - y^2) / (2 (x^2 + y^2)^2) + ...): the Voigt profile deviates from the
    Lorentz profile by at most 3 / (2 y^2) relative, up to the next order of the series (factor 2 below)."""
    t = _one_line(gamma_air=5.0)
    grid = np.linspace(6000.0, 6050.0, 501)
    kw = dict(p=[1013.25], T=[296.0], wing_cutoff=40.0)
    y = float(AO.line_parameters(t, 0, 1013.25, 296.0, 0.0, 1.0, AC.ISOTOPOLOGUES[(2, 1)][0])[3])
    assert y > 500
    v = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, broadening="Voigt", cef=cef, **kw)
    lo = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, broadening="Lorentz", **kw)
    assert np.all(lo > 0) and np.max(np.abs(v - lo) / lo) <= 2 * 1.5 / y ** 2


@pytest.mark.parametrize("cef", AO.CEFS[:2])
def test_voigt_tends_to_doppler_for_small_y(cef):
    """Re w(x + i y) = exp(-x^2) - (2 y / sqrt(pi)) (1 - 2 x F(x)) + O(y^2), F Dawson's integral, |1 - 2 x F(x)| <= 1: within |x| <= 2
    the two profiles differ by at most the prefactor times (2 y / sqrt(pi) + the error function's own error bound)."""
    t = _one_line(gamma_air=0.07)
    p = 0.5
    nu, gl, gd, y, S = (float(v) for v in AO.line_parameters(t, 0, p, 296.0, 0.0, 1.0, AC.ISOTOPOLOGUES[(2, 1)][0]))
    assert 1e-3 < y < 1e-2
    grid = np.linspace(nu - 2 * gd / AO.SQRTLN2, nu + 2 * gd / AO.SQRTLN2, 401)
    kw = dict(p=[p], T=[296.0], wing_cutoff=1.0)
    v = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, broadening="Voigt", cef=cef, **kw)
    d = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, broadening="Doppler", **kw)
    pre = S * AO.SQRTLN2_SQRTPI / gd
    assert np.max(np.abs(v - d)) <= pre * (2 * y / math.sqrt(math.pi) * (1 + 10 * y) + CEF_BOUND[cef])
    assert np.max(np.abs(v - d)) > 0.1 * pre * y                  # (and they are not the same function)


def test_one_line_integrates_to_its_strength():
    """One isolated line on a fine grid with a wide cutoff: the trapezoid sum of sigma is S(T) less the wings beyond the cutoff.
    Wings: a Voigt profile is a Lorentz profile convolved with a unit-area Gaussian of width << cutoff, so the area beyond
    +/- cutoff is at most that of the Lorentz wings beyond (cutoff - 5 gamma_d'): (2 / pi) atan-complement <= 2 gamma_l / (pi c').
    Trapezoid: |error| <= (b - a) h^2 / 12 max |f''|, and max |f''| of the convolution is at most that of the Lorentz profile,
    2 S / (pi gamma_l^3).  The window ends are rounded to the nearest point: at most half a step of Lorentz wing at each end."""
    t = _one_line(gamma_air=0.07, E_low=412.0, delta=-0.006)
    p, T, cutoff, h = 900.0, 260.0, 10.0, 2e-4
    qr = float(AO.qoft(AC.ISOTOPOLOGUES[(2, 1)][1], AC.ISOTOPOLOGUES[(2, 1)][2], [T])[0])
    nu, gl, gd, y, S = (float(v) for v in AO.line_parameters(t, 0, p, T, 0.0, qr, AC.ISOTOPOLOGUES[(2, 1)][0]))
    n = int(round(2 * (cutoff + 1.0) / h)) + 1
    grid = np.linspace(6025.0 - cutoff - 1.0, 6025.0 + cutoff + 1.0, n)
    sig = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, [p], [T], wing_cutoff=cutoff)[0]
    step = grid[1] - grid[0]
    area = float(np.sum(0.5 * (sig[1:] + sig[:-1]) * np.diff(grid)))
    wings = 2 * gl / (math.pi * (cutoff - 5 * gd / AO.SQRTLN2 - step))
    trapezoid = 2 * cutoff * step ** 2 / 12 * 2 / (math.pi * gl ** 3)
    edge = step * gl / (math.pi * (cutoff - step) ** 2)          # each end of the window is rounded to the nearest point
    print("area / S = %.6f; wings <= %.3e, trapezoid <= %.3e, edge <= %.3e" % (area / S, wings, trapezoid, edge))
    assert S > 0 and -(wings + trapezoid + edge + CEF_BOUND[AO.CEFS[1]]) <= area / S - 1 <= trapezoid + edge + CEF_BOUND[AO.CEFS[1]]
    assert np.count_nonzero(sig == 0) > 0                         # the cutoff is applied: points beyond it are exact zeros


def test_qoft_against_scipy_natural_spline(A):
    CubicSpline = pytest.importorskip("scipy.interpolate").CubicSpline
    T = np.array([101.0, 180.0, 223.4, 296.0, 305.5, 399.0])
    for key, (mass, TT, TQ) in AC.ISOTOPOLOGUES.items():
        cs = CubicSpline(TT, TQ, bc_type="natural")
        ref = cs(296.0) / cs(T)
        np.testing.assert_allclose(A.qoft(A.IsotopologueData(mass, TT, TQ), T), ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(AO.qoft(TT, TQ, T), ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(AO.qoft(TT, TQ, T, dtype=np.longdouble).astype(np.float64), ref, rtol=1e-12, atol=0)
        assert isinstance(A.qoft(A.IsotopologueData(mass, TT, TQ), 250.0), float)
        assert A.qoft(A.IsotopologueData(mass, TT, TQ), 296.0) == 1.0


# ---- the deviation and the host bookkeeping, with the device replaced by the oracle ----------------------------------------------------
class OracleDevice:
    """Stands in for absorption._Device: the same five methods on numpy arrays, vsm_absorption_xsec computed by the oracle from
    exactly what the host would hand the library."""
    calls = []

    def __init__(self, architecture):
        pass

    def empty(self, Nz, nSpec):
        return np.full((Nz, nSpec), np.nan)

    def zeros(self, Nz, nSpec):
        return np.zeros((Nz, nSpec))

    def profile(self, job):
        return job

    def xsec(self, job, handle, scale, out, accumulate):
        assert handle is job and np.all(np.diff(job.lines["nu"]) >= 0) and job.delta_max >= np.max(np.abs(job.lines["delta_air"]))
        sig = AO.cross_section_lines(job.grid, job.lines, job.lines["species"], job.molar_mass, job.qratio, job.p, job.T, job.vmr_self,
                                     AO.BROADENINGS[job.broadening], AO.CEFS[job.cef], job.wing_cutoff)
        OracleDevice.calls.append((job.n_lines, int(accumulate)))
        out[...] = (out if accumulate else 0.0) + sig * np.asarray(scale)[:, None]

    def fetch(self, outs):
        return [np.array(o) for o in outs]


@pytest.fixture()
def oracle_device(A, monkeypatch):
    monkeypatch.setattr(A, "_Device", OracleDevice)
    OracleDevice.calls = []
    return OracleDevice


def test_a_line_whose_shifted_window_misses_the_grid_contributes_nothing(A, oracle_device):
    t, grid, cutoff, p, T = AC.deviation_case()
    assert grid[0] - cutoff < t["nu"][0] < grid[0]                                         # inside the unshifted filter
    assert t["nu"][0] + p[0] / AO.P_REF * t["delta_air"][0] + cutoff < grid[0]             # the shifted window misses the grid
    ref = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff)
    assert ref.shape == (1, len(grid)) and np.all(ref == 0)
    got = A.compute_absorption_cross_section(AC.make_model(A, t, wing_cutoff=cutoff), grid, p, T)
    assert oracle_device.calls == [(1, 0)]                                                 # the host filter kept the line
    assert got.shape == (1, len(grid)) and np.all(got == 0)
    # without the shift the same line reaches the first points
    t["delta_air"][:] = 0.0
    assert np.count_nonzero(AO.cross_section(t, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff)) > 0


def test_cross_section_host_side_shapes_sort_filter_and_wavelength_flag(A, oracle_device):
    t = AC.synthetic_table(11, 40, two_species=True, no_E_share=0.2)
    t["nu"][:3] = [5990.0, 6060.1, 5994.9]                                                 # outside (min - cutoff, max + cutoff)
    grid = AC.nonuniform_grid(120, 5)
    m = AC.make_model(A, t, vmr=np.array([0.0, 0.3, 0.1]))
    sig = A.compute_absorption_cross_section(m, grid, AC.P3, AC.T3)
    assert oracle_device.calls == [(37, 0)]
    ref = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, [0.0, 0.3, 0.1], wing_cutoff=5.0)
    assert sig.shape == (3, 120) and np.array_equal(sig, ref)
    one = A.compute_absorption_cross_section(AC.make_model(A, t, vmr=0.3), grid, float(AC.P3[1]), float(AC.T3[1]))
    assert one.shape == (120,) and np.array_equal(one, sig[1])
    wl = np.linspace(1652.9, 1666.6, 90)                                                   # nm, ascending
    wn = (1e7 / wl)[::-1]
    a = A.compute_absorption_cross_section(m, wl, AC.P3, AC.T3, wavelength_flag=True)
    b = A.compute_absorption_cross_section(m, wn, AC.P3, AC.T3)
    assert np.count_nonzero(b) > 0 and np.array_equal(a, b[:, ::-1])
    assert np.array_equal(a, AO.cross_section(t, AC.ISOTOPOLOGUES, wl, AC.P3, AC.T3, [0.0, 0.3, 0.1], wing_cutoff=5.0,
                                              wavelength_flag=True))
    # an empty selection: exact zeros and no launch
    oracle_device.calls.clear()
    z = A.compute_absorption_cross_section(m, np.linspace(7000.0, 7010.0, 7), AC.P3, AC.T3)
    assert z.shape == (3, 7) and np.all(z == 0) and oracle_device.calls == []


def test_absorption_profile_bookkeeping(A, oracle_device):
    ta = AC.synthetic_table(21, 30, no_E_share=0.1)
    tb = AC.synthetic_table(22, 17, two_species=True)
    tc = AC.synthetic_table(23, 4, lo=7000.0, hi=7001.0)                                   # no line near the grid
    grid = AC.nonuniform_grid(64, 9)
    vcd = np.array([3.1e21, 2.2e23, 1.9e24])
    vmr_a, vmr_b = 4.1e-4, np.array([0.21, 0.2, 0.19])
    pairs = [(AC.make_model(A, tc), 1e-6), (AC.make_model(A, ta, vmr=vmr_a), vmr_a), (AC.make_model(A, tb, vmr=vmr_b), vmr_b)]
    tau = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd)
    assert oracle_device.calls == [(30, 0), (17, 1)]               # the empty gas launches nothing; the second adds on the device
    ref, ref_dots = AO.absorption_profile([(tc, AC.ISOTOPOLOGUES, 0.0, 1e-6), (ta, AC.ISOTOPOLOGUES, vmr_a, vmr_a),
                                           (tb, AC.ISOTOPOLOGUES, vmr_b, vmr_b)], grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0)
    assert tau.shape == (64, 3) and tau.flags["C_CONTIGUOUS"]
    np.testing.assert_allclose(tau, ref, rtol=4e-16, atol=0)       # (sigma vcd) vmr against sigma (vcd vmr): one rounding each
    oracle_device.calls.clear()
    tau2, dots = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd, lin=True)
    assert oracle_device.calls == [(30, 0), (30, 0), (17, 1), (17, 0)]
    assert np.array_equal(tau2, tau) and len(dots) == 3 and all(d.shape == (64, 3) for d in dots)
    assert np.all(dots[0] == 0)
    for d, r in zip(dots[1:], ref_dots[1:]):
        assert np.array_equal(d, r)                                # tau_abs_dot[g] = sigma_g vcd_dry
    np.testing.assert_allclose(dots[1] * vmr_a + dots[2] * vmr_b[None, :], tau, rtol=1e-15, atol=0)
    import vsmartmom_jl_amd as vsm
    with pytest.raises(vsm.VSMError, match="uniform"):
        A.compute_absorption_profile([(pairs[1][0], np.ones(2))], grid, AC.P3, AC.T3, vcd)
    z = A.compute_absorption_profile([pairs[0]], grid, AC.P3, AC.T3, vcd)
    assert z.shape == (64, 3) and np.all(z == 0)


def test_entry_refuses_bad_arguments_before_any_launch():
    """vsm_absorption_xsec checks sizes, switches and null pointers before it touches the device: the codes come back on a machine
    without one."""
    import ctypes as C
    import vsmartmom_jl_amd as vsm
    lib = vsm._lib.lib()
    buf = (C.c_double * 64)()
    P = C.cast(buf, C.c_void_p)

    def call(nSpec=4, nLines=2, nSpecies=1, Nz=1, cutoff=5.0, dmax=0.01, broadening=2, cef=1, accumulate=0, null=None):
        ptrs = [None if i == null else P for i in range(15)]
        return lib.vsm_absorption_xsec(nSpec, nLines, nSpecies, Nz, *ptrs, C.c_double(cutoff), C.c_double(dmax), broadening, cef,
                                       accumulate, None if null == 15 else P, None if null == 16 else P, None)

    INVALID = 1
    for kw in (dict(nSpec=0), dict(nLines=0), dict(nSpecies=0), dict(Nz=0), dict(Nz=65536), dict(cutoff=-1.0), dict(cutoff=float("nan")),
               dict(dmax=-1e-3), dict(broadening=3), dict(broadening=-1), dict(cef=3), dict(accumulate=2)):
        assert call(**kw) == INVALID, kw
        assert b"vsm_absorption_xsec" in lib.vsm_last_error()
    for null in range(17):
        assert call(null=null) == INVALID, null
    assert lib.vsm_absorption_work_elems(40, 2000) == 8 * 40 * 2000
    assert lib.vsm_absorption_work_elems(1, 0) == 0 and lib.vsm_absorption_work_elems(-1, 5) == 0
    assert lib.vsm_absorption_chunk() == 256
