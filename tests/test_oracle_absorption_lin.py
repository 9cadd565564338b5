"""CPU tests of the linearized Absorption: tests/absorption_lin_oracle.py against finite differences of the FORWARD oracle, qoft_lin,
and the host bookkeeping of compute_absorption_cross_section_lin / compute_absorption_profile_lin with the device replaced by the
oracle.

The finite-difference check.  The analytic slots (80-bit) are compared with two-level Richardson central differences (relative step
2e-3, error O(h^4)) of the forward oracle's own pieces (AO.line_parameters, AO.window, the AO approximants), windows and error-function
regions frozen at the base state.  Per slot the deviation is divided by A, the absolute term sum
sum_lines (|pre dlnpre F| + |pre F_x x_theta| + |pre F_y y_theta|): a formula error is a share of A, the difference error is not.
The bound 1e-6 is not a measurement of the code under test: the difference error of a smooth function at this step is
(h^4 / 480) f^(5) scale, 1e-8 or less (measured: the maxima printed below), and a wrong or missing factor moves a term by a share of
order one of itself.  That the cases exercise every factor is tested too: each of the six non-zero factors of the table, dropped from
the oracle, must miss the bound by at least 100 x on at least one case."""
import ctypes as C
import functools

import numpy as np
import pytest

import absorption_cases as AC
import absorption_lin_oracle as AL
import absorption_oracle as AO

SD, HW, CPF = AO.CEFS[1], AO.CEFS[0], AO.CEFS[2]
FD_BOUND = 1e-6
VMR3 = np.array([0.0, 0.3, 0.11])

# name: (broadening, cef, cutoff, grid span, line span); all on 257 points x 40 lines x 3 layers, two species, a share of E'' = -1 lines.
# Doppler: exp(-ln 2 u^2), u = dnu / gamma_d, moves by the factor exp(-2 ln 2 u du) under a step du, so the O(h^4) error of the
# differences, relative to the derivative, grows as (2 ln 2 u du)^4: differences at a relative step of 2e-3 resolve the derivative
# only at small |u|.  The cutoff of 0.01 cm^-1 keeps |u| below 2.3 (gamma_d = 4.4e-3 cm^-1 at 180 K), on a grid fine enough to have
# points there.  (The GPU tests, which need no differences, run Doppler at 0.1 cm^-1.)
FD_CASES = {"voigt_sd": ("Voigt", SD, 5.0, (6000.0, 6050.0), (6015.0, 6035.0)),
            "voigt_hw": ("Voigt", HW, 5.0, (6000.0, 6050.0), (6015.0, 6035.0)),
            "doppler": ("Doppler", SD, 0.01, (6024.5, 6025.5), (6024.8, 6025.2)),
            "lorentz": ("Lorentz", SD, 5.0, (6000.0, 6050.0), (6015.0, 6035.0))}


@pytest.fixture(scope="module")
def A():
    import vsmartmom_jl_amd as v
    return v.Absorption


def _fd_inputs(name):
    broadening, cef, cutoff, gspan, lspan = FD_CASES[name]
    table = AC.synthetic_table(1000 + sum(map(ord, name)), 40, lo=lspan[0], hi=lspan[1], two_species=True, no_E_share=0.25)
    assert np.any(table["E_low"] == -1) and len(set(table["mol"])) == 2
    return table, AC.uniform_grid(257, *gspan), dict(broadening=broadening, cef=cef, wing_cutoff=cutoff)


@functools.lru_cache(maxsize=None)
def _fd_reference(name):
    """(Richardson differences, A) in 80-bit: computed once per case, shared, never changed."""
    table, grid, kw = _fd_inputs(name)
    fd = AL.richardson_differences(table, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, VMR3, **kw)
    A80 = AL.cross_section_lin(table, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, VMR3, dtype=np.longdouble, **kw)[1]
    fd.setflags(write=False)
    A80.setflags(write=False)
    return fd, A80


def _fd_deviation(name, drop=None):
    """max over points of |analytic - differences| / A per slot; a slot whose A is zero everywhere (Doppler's vmr_self) must be zero."""
    table, grid, kw = _fd_inputs(name)
    fd, A80 = _fd_reference(name)
    dot = AL.cross_section_lin(table, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, VMR3, dtype=np.longdouble, drop=drop, **kw)[0]
    out = []
    for k in range(3):
        nz = A80[k] > 0
        assert np.all(dot[k][~nz] == 0) and np.all(fd[k][~nz] == 0)
        out.append(float(np.max(np.abs(dot[k][nz] - fd[k][nz]) / A80[k][nz])) if nz.any() else 0.0)
    return out


@pytest.mark.parametrize("name", sorted(FD_CASES))
def test_oracle_slots_against_richardson_differences(name):
    fd, A80 = _fd_reference(name)
    assert 0 < np.count_nonzero(A80[0] == 0) < A80[0].size, "the case should have points no window reaches"
    dev = _fd_deviation(name)
    print("absorption lin %s: max |analytic - differences| / A per slot (T, p, vmr_self): %.2e %.2e %.2e" % (name, *dev))
    assert max(dev) <= FD_BOUND, dev
    if name == "doppler":
        assert np.all(A80[2] == 0) and np.all(fd[2] == 0)                # gamma_l does not enter: the slot is identically zero
    else:
        assert all(np.count_nonzero(A80[k]) > 0 for k in range(3))


@pytest.mark.parametrize("term", AL.TERMS)
def test_each_factor_of_the_table_matters(term):
    """The oracle without one factor misses the bound by at least 100 x on at least one case: the cases exercise that factor."""
    slot = AL.SLOTS.index(term[0])
    worst = {name: _fd_deviation(name, drop=term)[slot] for name in sorted(FD_CASES)}
    print("absorption lin without %r: %s" % (term, {k: "%.2e" % v for k, v in worst.items()}))
    assert max(worst.values()) >= 100 * FD_BOUND, worst


def test_both_regions_of_each_error_function_occur():
    for name in ("voigt_sd", "voigt_hw"):
        table, grid, kw = _fd_inputs(name)
        g, lines, species, mass, qr, dq, p, T, vmr = AL._selection(table, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, VMR3, kw["wing_cutoff"],
                                                                   False, np.float64)
        seen = set()
        for iz in range(3):
            for j in range(len(lines["nu"])):
                r = AL.line_record(lines, j, p[iz], T[iz], vmr[iz], 1.0, 0.0, mass[int(species[j])], "Voigt")
                i0, i1 = AO.window(g, float(r["nu"]), kw["wing_cutoff"])
                seen |= set(np.unique(AL.region(kw["cef"], r["sx"] * (g[i0 - 1:i1] - r["nu"]), r["y"])).tolist())
        assert seen == {True, False}, (name, seen)


def test_w_lin_is_the_forward_w_and_its_derivative():
    z = np.array([0.3 + 0.01j, 3 + 2j, 7.9 + 0.05j, 9 + 1j, 20 + 0.3j, 14.2 + 0.5j, -5 + 4j, -15.5 + 1e-4j])
    for cef in (HW, SD):
        w, dw = AL.w_lin(cef, z, np.longdouble)
        np.testing.assert_allclose(w, AO.w(cef, z, np.longdouble), rtol=1e-17, atol=0)      # z inv against z / den
        h = np.longdouble(1e-5)
        mask = AL.region(cef, z.real, z.imag)
        fd = (AL.w_lin(cef, z + h, np.longdouble, mask)[0] - AL.w_lin(cef, z - h, np.longdouble, mask)[0]) / (2 * h)
        assert np.max(np.abs(dw - fd) / np.abs(fd)) < 1e-8               # h^2 / 6 w''' / w': 1e-10 .. 1e-9 here


def test_qoft_lin_against_scipy_natural_spline(A):
    CubicSpline = pytest.importorskip("scipy.interpolate").CubicSpline
    T = np.array([101.0, 180.0, 223.4, 296.0, 305.5, 399.0])
    for key, (mass, TT, TQ) in AC.ISOTOPOLOGUES.items():
        cs = CubicSpline(TT, TQ, bc_type="natural")
        ref = -cs(296.0) * cs(T, 1) / cs(T) ** 2
        iso = A.IsotopologueData(mass, TT, TQ)
        r, d = A.qoft_lin(iso, T)
        assert np.array_equal(r, A.qoft(iso, T))
        np.testing.assert_allclose(d, ref, rtol=1e-11, atol=0)
        np.testing.assert_allclose(AL.qoft_lin(TT, TQ, T)[1], ref, rtol=1e-11, atol=0)
        np.testing.assert_allclose(AL.qoft_lin(TT, TQ, T, dtype=np.longdouble)[1].astype(np.float64), ref, rtol=1e-11, atol=0)
        r1, d1 = A.qoft_lin(iso, 250.0)
        assert isinstance(r1, float) and isinstance(d1, float) and r1 == A.qoft(iso, 250.0)
    import vsmartmom_jl_amd as vsm
    with pytest.raises(vsm.VSMError, match="between"):
        A.qoft_lin(A.IsotopologueData(*AC.ISOTOPOLOGUES[(2, 1)]), 99.0)


# ---- host bookkeeping, with the device replaced by the oracle ----------------------------------------------------------------------------
class OracleDevice:
    """Stands in for absorption._Device: its methods on numpy arrays, the library calls computed by the oracles from exactly what the
    host would hand the library."""
    calls = []

    def __init__(self, architecture):
        pass

    def empty(self, Nz, nSpec):
        return np.full((Nz, nSpec), np.nan)

    def zeros(self, Nz, nSpec):
        return np.zeros((Nz, nSpec))

    def profile(self, job):
        return job

    profile_lin = profile

    def _sigma(self, job):
        return AO.cross_section_lines(job.grid, job.lines, job.lines["species"], job.molar_mass, job.qratio, job.p, job.T, job.vmr_self,
                                      AO.BROADENINGS[job.broadening], AO.CEFS[job.cef], job.wing_cutoff)

    def xsec(self, job, handle, scale, out, accumulate):
        assert handle is job
        OracleDevice.calls.append(("xsec", job.n_lines, int(accumulate)))
        out[...] = (out if accumulate else 0.0) + self._sigma(job) * np.asarray(scale)[:, None]

    def xsec_lin(self, job, handle, scale, out, out_dT, out_dp, out_dvmr, accumulate):
        assert handle is job and np.all(np.diff(job.lines["nu"]) >= 0) and job.qratio_dlnT.shape == job.qratio.shape
        dot = AL.cross_section_lin_lines(job.grid, job.lines, job.lines["species"], job.molar_mass, job.qratio, job.qratio_dlnT, job.p,
                                         job.T, job.vmr_self, AO.BROADENINGS[job.broadening], AO.CEFS[job.cef], job.wing_cutoff)[0]
        OracleDevice.calls.append(("xsec_lin", job.n_lines, int(accumulate)))
        for o, v in zip((out, out_dT, out_dp, out_dvmr), (self._sigma(job), dot[0], dot[1], dot[2])):
            o[...] = (o if accumulate else 0.0) + v * np.asarray(scale)[:, None]

    def profile_slots(self, dT, dp, T_dot, p_dot):
        OracleDevice.calls.append(("slots", len(T_dot)))
        return dT[None] * np.asarray(T_dot)[:, :, None] + dp[None] * np.asarray(p_dot)[:, :, None]

    def fetch(self, outs):
        return [np.array(o) for o in outs]


@pytest.fixture()
def oracle_device(A, monkeypatch):
    monkeypatch.setattr(A, "_Device", OracleDevice)
    OracleDevice.calls = []
    return OracleDevice


def test_cross_section_lin_shapes_sort_wavelength_flag_and_empty_selection(A, oracle_device):
    assert A.SLOTS == ("T", "p", "vmr_self") == AL.SLOTS
    t = AC.synthetic_table(11, 40, two_species=True, no_E_share=0.2)
    t["nu"][:3] = [5990.0, 6060.1, 5994.9]                                                 # outside (min - cutoff, max + cutoff)
    grid = AC.nonuniform_grid(120, 5)
    m = AC.make_model(A, t, vmr=VMR3)
    sig, dot = A.compute_absorption_cross_section_lin(m, grid, AC.P3, AC.T3)
    assert oracle_device.calls == [("xsec_lin", 37, 0)]                                   # one call; the unsorted table was sorted
    ref = AL.cross_section_lin(t, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, VMR3, wing_cutoff=5.0)[0]
    assert sig.shape == (3, 120) and dot.shape == (3, 3, 120) and np.array_equal(dot, ref) and np.count_nonzero(dot[2]) > 0
    oracle_device.calls.clear()
    assert np.array_equal(sig, A.compute_absorption_cross_section(m, grid, AC.P3, AC.T3))
    s1, d1 = A.compute_absorption_cross_section_lin(AC.make_model(A, t, vmr=0.3), grid, float(AC.P3[1]), float(AC.T3[1]))
    assert s1.shape == (120,) and d1.shape == (3, 120) and np.array_equal(s1, sig[1]) and np.array_equal(d1, dot[:, 1])
    wl = np.linspace(1652.9, 1666.6, 90)                                                   # nm, ascending
    wn = (1e7 / wl)[::-1]
    sa, da = A.compute_absorption_cross_section_lin(m, wl, AC.P3, AC.T3, wavelength_flag=True)
    sb, db = A.compute_absorption_cross_section_lin(m, wn, AC.P3, AC.T3)
    assert np.count_nonzero(db) > 0 and np.array_equal(sa, sb[:, ::-1]) and np.array_equal(da, db[:, :, ::-1])
    oracle_device.calls.clear()
    sz, dz = A.compute_absorption_cross_section_lin(m, np.linspace(7000.0, 7010.0, 7), AC.P3, AC.T3)
    assert sz.shape == (3, 7) and dz.shape == (3, 3, 7) and np.all(sz == 0) and np.all(dz == 0) and oracle_device.calls == []
    sz, dz = A.compute_absorption_cross_section_lin(AC.make_model(A, t, vmr=0.3), np.linspace(7000.0, 7010.0, 7), 500.0, 250.0)
    assert sz.shape == (7,) and dz.shape == (3, 7) and np.all(dz == 0)


def test_absorption_profile_lin_bookkeeping(A, oracle_device):
    ta = AC.synthetic_table(21, 30, no_E_share=0.1)
    tb = AC.synthetic_table(22, 17, two_species=True)
    tc = AC.synthetic_table(23, 4, lo=7000.0, hi=7001.0)                                   # no line near the grid
    grid = AC.nonuniform_grid(64, 9)
    vcd = np.array([3.1e21, 2.2e23, 1.9e24])
    vmr_a, vmr_b = 4.1e-4, np.array([0.21, 0.2, 0.19])
    pairs = [(AC.make_model(A, tc), 1e-6), (AC.make_model(A, ta, vmr=vmr_a), vmr_a), (AC.make_model(A, tb, vmr=vmr_b), vmr_b)]
    gases = [(tc, AC.ISOTOPOLOGUES, 0.0, 1e-6), (ta, AC.ISOTOPOLOGUES, vmr_a, vmr_a), (tb, AC.ISOTOPOLOGUES, vmr_b, vmr_b)]
    tau, dots = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd, lin=True)
    oracle_device.calls.clear()
    T_dot = np.vstack([np.eye(3), np.ones((1, 3)), np.zeros((1, 3))])                     # unit table, a shift, nothing
    p_dot = np.vstack([np.zeros((4, 3)), (AC.P3 / AC.P3[-1])[None]])                      # ... and surface pressure
    r = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd, T_dot=T_dot, p_dot=p_dot)
    # the empty gas launches nothing; the second gas adds on the device; the slots are formed before the one fetch
    assert oracle_device.calls == [("xsec_lin", 30, 0), ("xsec", 30, 0), ("xsec_lin", 17, 1), ("xsec", 17, 0), ("slots", 5)]
    assert np.array_equal(r.tau_abs, tau) and len(r.tau_abs_dot) == 3 and all(np.array_equal(a, b) for a, b in zip(r.tau_abs_dot, dots))
    (dT, dp, dv), _ = AL.absorption_profile_lin(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0)
    for got, want in ((r.dtau_dT, dT), (r.dtau_dp, dp), (r.dtau_dvmr_self[1], dv[1]), (r.dtau_dvmr_self[2], dv[2])):
        assert got.shape == (64, 3) and got.flags["C_CONTIGUOUS"] and np.count_nonzero(want) > 0
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)    # the order of the products and of the sum over gases
    assert np.all(r.dtau_dvmr_self[0] == 0) and np.all(r.tau_abs_dot[0] == 0) and len(r.dtau_dvmr_self) == 3
    assert r.profile_slots.shape == (5, 64, 3)
    for k in range(3):                                               # a unit table: layer k's partial in layer k, zero elsewhere
        want = np.zeros((64, 3))
        want[:, k] = r.dtau_dT[:, k]
        assert np.array_equal(r.profile_slots[k], want)
    assert np.array_equal(r.profile_slots[3], r.dtau_dT)
    assert np.array_equal(r.profile_slots[4], r.dtau_dp * (AC.P3 / AC.P3[-1])[None, :])
    slots = r.lin_model_slots()
    assert len(slots) == 3 + 5 and all(a is b for a, b in zip(slots[:3], r.tau_abs_dot))
    assert all(np.array_equal(a, b) for a, b in zip(slots[3:], r.profile_slots))
    # no tables: no profile slots, no launch for them; T_dot alone: p_dot counts as zeros
    oracle_device.calls.clear()
    r0 = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd)
    assert r0.profile_slots.shape == (0, 64, 3) and len(r0.lin_model_slots()) == 3 and ("slots", 0) not in oracle_device.calls
    assert np.array_equal(r0.dtau_dT, r.dtau_dT)
    r1 = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd, T_dot=np.ones((1, 3)))
    assert np.array_equal(r1.profile_slots[0], r.dtau_dT)
    # an all-empty list: exact zeros without a launch
    oracle_device.calls.clear()
    rz = A.compute_absorption_profile_lin([pairs[0]], grid, AC.P3, AC.T3, vcd, T_dot=np.ones((2, 3)))
    assert oracle_device.calls == [] and rz.profile_slots.shape == (2, 64, 3)
    assert all(np.all(a == 0) for a in (rz.tau_abs, rz.dtau_dT, rz.dtau_dp, rz.profile_slots, rz.tau_abs_dot[0], rz.dtau_dvmr_self[0]))


def test_lin_calls_refuse_what_the_forward_refuses_and_cpf12_before_any_launch(A, oracle_device):
    import vsmartmom_jl_amd as vsm
    t = AC.synthetic_table(3, 5)
    grid = AC.uniform_grid(33)
    m = AC.make_model(A, t)
    vcd = np.ones(3)
    with pytest.raises(NotImplementedError, match="CPF12"):
        A.compute_absorption_cross_section_lin(AC.make_model(A, t, cef=CPF), grid, AC.P3, AC.T3)
    with pytest.raises(NotImplementedError, match="CPF12"):
        A.compute_absorption_profile_lin([(m, 0.1), (AC.make_model(A, t, cef=CPF), 0.1)], grid, AC.P3, AC.T3, vcd)
    A.compute_absorption_cross_section_lin(AC.make_model(A, t, "Doppler", CPF, 0.1), grid, AC.P3, AC.T3)   # the CEF is read under Voigt only
    oracle_device.calls.clear()
    for call, match in (
            (lambda: A.compute_absorption_cross_section_lin(m, [6030.0, 6020.0], 500.0, 250.0), "ascending"),
            (lambda: A.compute_absorption_cross_section_lin(m, grid, AC.P3, AC.T3[:2]), "one length"),
            (lambda: A.compute_absorption_cross_section_lin(AC.make_model(A, t, vmr=np.ones(2)), grid, AC.P3, AC.T3), "model.vmr"),
            (lambda: A.compute_absorption_cross_section_lin(m, grid, AC.P3, np.array([180.0, 99.0, 250.0])), "between"),
            (lambda: A.compute_absorption_cross_section_lin("no model", grid, AC.P3, AC.T3), "HitranModel"),
            (lambda: A.compute_absorption_profile_lin([], grid, AC.P3, AC.T3, vcd), "no \\(model, vmr\\) pair"),
            (lambda: A.compute_absorption_profile_lin([(m, np.ones(2))], grid, AC.P3, AC.T3, vcd), "uniform"),
            (lambda: A.compute_absorption_profile_lin([(m, 0.1)], grid, AC.P3, AC.T3, vcd[:2]), "layers"),
            (lambda: A.compute_absorption_profile_lin([(m, 0.1)], grid, AC.P3, AC.T3, vcd, T_dot=np.ones(3)), r"T_dot .* is not \[K, 3\]"),
            (lambda: A.compute_absorption_profile_lin([(m, 0.1)], grid, AC.P3, AC.T3, vcd, p_dot=np.ones((2, 4))), r"p_dot .* is not \[K, 3\]"),
            (lambda: A.compute_absorption_profile_lin([(m, 0.1)], grid, AC.P3, AC.T3, vcd, T_dot=np.ones((1, 3)), p_dot=np.ones((2, 3))),
             "differ in K")):
        with pytest.raises(vsm.VSMError, match=match):
            call()
    assert oracle_device.calls == []


def test_entry_refuses_bad_arguments_before_any_launch():
    """vsm_absorption_xsec_lin and vsm_absorption_profile_slots check sizes, switches and null pointers before they touch the device:
    the codes come back on a machine without one."""
    import vsmartmom_jl_amd as vsm
    lib = vsm._lib.lib()
    buf = (C.c_double * 64)()
    P = C.cast(buf, C.c_void_p)
    INVALID = 1

    def call(nSpec=4, nLines=2, nSpecies=1, Nz=1, cutoff=5.0, dmax=0.01, broadening=2, cef=1, accumulate=0, null=None):
        ptrs = [None if i == null else P for i in range(21)]
        return lib.vsm_absorption_xsec_lin(nSpec, nLines, nSpecies, Nz, *ptrs[:16], C.c_double(cutoff), C.c_double(dmax), broadening, cef,
                                           accumulate, *ptrs[16:], None)

    for kw in (dict(nSpec=0), dict(nLines=0), dict(nSpecies=0), dict(Nz=0), dict(Nz=65536), dict(cutoff=-1.0), dict(cutoff=float("nan")),
               dict(dmax=-1e-3), dict(broadening=3), dict(broadening=-1), dict(cef=3), dict(cef=-1), dict(accumulate=2),
               dict(broadening=2, cef=2)):
        assert call(**kw) == INVALID, kw
        assert b"vsm_absorption_xsec_lin" in lib.vsm_last_error()
    assert b"CPF12" in lib.vsm_last_error()
    for null in range(21):
        assert call(null=null) == INVALID, null
    assert lib.vsm_absorption_lin_chunk() == 256
    assert lib.vsm_absorption_lin_work_elems(40, 2000) == (8 + 10) * 40 * 2000
    assert lib.vsm_absorption_lin_work_elems(1, 0) == 0 and lib.vsm_absorption_lin_work_elems(-1, 5) == 0
    assert lib.vsm_absorption_chunk() == 256 and lib.vsm_absorption_work_elems(40, 2000) == 8 * 40 * 2000      # the forward's keep theirs
    for args in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (4, 65536, 1), (4, 1, 65536)):
        assert lib.vsm_absorption_profile_slots(*args, P, P, P, P, P, None) == INVALID, args
        assert b"vsm_absorption_profile_slots" in lib.vsm_last_error()
    for null in range(5):
        assert lib.vsm_absorption_profile_slots(4, 1, 1, *[None if i == null else P for i in range(5)], None) == INVALID, null
