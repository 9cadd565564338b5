"""GPU tests of vsm.Absorption (vsm_absorption_xsec, csrc/vsm_absorption.hip) against tests/absorption_oracle.py, through the public
functions, on seeded synthetic tables and the reference's 16-line HITRAN test file.

Acceptance per case:
 (a) the pattern of exact zeros equals the oracle's at every (layer, point): a window off by one point fails here whatever its size;
 (b) the per-point relative deviation from the FP64 oracle is at most 10 x the case's own rounding floor, the floor being
     max |oracle64 - oracle_longdouble| / oracle_longdouble computed here on the CPU (never from the code under test); a floor below
     1e-14 counts as 1e-14, i.e. the bound is never below 1e-13.  The factor 10 covers the device's exp and pow differing from libm by
     a few ulp and FMA contraction; all terms are positive, so the sums are well conditioned.  The floor is large (1e-10) where
     Weideman's 32-term polynomial is evaluated at small y and large |x|: Re w there is the small remainder of cancelling terms, in
     the oracle as on the device.
The measured maxima per broadening and error function are in DESIGN.md 4.25.

Shapes: nSpec = 1 (the N_grid == 1 branch), 255 / 256 / 257 (the edges of the 256-point tile), 1000 on a non-uniform grid (four tiles,
sixteen waves); nLines = 1, chunk - 1, chunk, chunk + 1, 3 chunk + 7 with chunk = vsm_absorption_chunk(); Nz = 1 and 3 with p from
0.1 to 1013 hPa and T from 180 to 320 K (y from 1e-4 to 10: every region of every error function).  The lines sit in the middle of the
grid with a cutoff of a tenth of its span, so each case has points no window reaches.
Doppler cases use a cutoff of 0.1 cm^-1: further out exp(-ln 2 (dnu / gamma_d)^2) falls into the subnormal range and below, where a
relative bound means nothing."""
import functools

import numpy as np
import pytest

import absorption_cases as AC
import absorption_oracle as AO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SD, HW, CPF = AO.CEFS[1], AO.CEFS[0], AO.CEFS[2]
CHUNK = 256      # asserted against the library in test_chunk_is_the_exported_one

# name: (nSpec, non-uniform grid seed or None, nLines, Nz, broadening, cef, self-vmr, cutoff, table options)
CASES = {
    "n1_l1_voigt_sd": (1, None, 1, 1, "Voigt", SD, 0.0, 5.0, dict(lo=6021.0, hi=6029.0)),
    "n1_lc_voigt_hw": (1, None, CHUNK, 3, "Voigt", HW, 0.3, 5.0, dict(lo=6021.0, hi=6029.0)),
    "n255_lcm1_voigt_hw": (255, None, CHUNK - 1, 3, "Voigt", HW, 0.3, 5.0, {}),
    "n256_lc_doppler": (256, None, CHUNK, 1, "Doppler", SD, 0.0, 0.1, {}),
    "n257_lcp1_lorentz": (257, None, CHUNK + 1, 3, "Lorentz", SD, "layers", 5.0, dict(no_E_share=0.3)),
    "n257_l1_voigt_cpf": (257, None, 1, 3, "Voigt", CPF, 0.0, 5.0, {}),
    "n1000_l3c7_voigt_sd": (1000, 31, 3 * CHUNK + 7, 3, "Voigt", SD, "layers", 5.0, dict(two_species=True, no_E_share=0.2)),
    "n1000_l3c7_voigt_cpf": (1000, 32, 3 * CHUNK + 7, 3, "Voigt", CPF, 0.3, 5.0, dict(two_species=True)),
    "n1000_lcp1_voigt_hw": (1000, 33, CHUNK + 1, 1, "Voigt", HW, 0.0, 5.0, dict(no_E_share=0.2)),
    "n1000_lc_doppler": (1000, 34, CHUNK, 3, "Doppler", SD, 0.0, 0.1, dict(two_species=True)),
    "n255_l3c7_lorentz": (255, 35, 3 * CHUNK + 7, 1, "Lorentz", SD, 0.3, 5.0, {}),
}


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU()


def _inputs(name):
    nSpec, gseed, nLines, Nz, broadening, cef, vmr, cutoff, opts = CASES[name]
    grid = AC.uniform_grid(nSpec) if gseed is None else AC.nonuniform_grid(nSpec, gseed)
    table = AC.synthetic_table(sum(map(ord, name)), nLines, **opts)
    p, T = (AC.P3, AC.T3) if Nz == 3 else (AC.P1, AC.T1)
    if isinstance(vmr, str):
        vmr = np.array([0.0, 0.3, 0.11])[:Nz]
    return grid, table, p, T, vmr, broadening, cef, cutoff


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(oracle in float64, oracle in long double) of a case: computed once, shared, never changed."""
    grid, table, p, T, vmr, broadening, cef, cutoff = _inputs(name)
    kw = dict(vmr=vmr, broadening=broadening, cef=cef, wing_cutoff=cutoff)
    r64 = AO.cross_section(table, AC.ISOTOPOLOGUES, grid, p, T, dtype=np.float64, **kw)
    rld = AO.cross_section(table, AC.ISOTOPOLOGUES, grid, p, T, dtype=np.longdouble, **kw)
    r64.setflags(write=False)
    rld.setflags(write=False)
    return r64, rld


def _accept(dev, r64, rld, what):
    assert dev.shape == r64.shape and dev.dtype == np.float64, (what, dev.shape, r64.shape)
    assert np.all(np.isfinite(dev)), what
    zeros_dev, zeros_ref = dev == 0, r64 == 0
    nz = ~zeros_ref
    floor = float(np.max(np.abs(r64[nz].astype(np.longdouble) - rld[nz]) / rld[nz])) if nz.any() else 0.0
    bound = 10 * max(floor, 1e-14)
    d = np.abs(dev[nz].astype(np.longdouble) - r64[nz].astype(np.longdouble)) / rld[nz] if nz.any() else np.zeros(1)
    print("absorption %s: %d of %d points zero; floor %.2e, bound %.2e, max rel dev %.2e"
          % (what, int(zeros_ref.sum()), zeros_ref.size, floor, bound, float(d.max())))
    assert np.array_equal(zeros_dev, zeros_ref), (what, int(zeros_dev.sum()), int(zeros_ref.sum()))          # (a)
    assert float(d.max()) <= bound, (what, float(d.max()), bound)                                             # (b)


def _model(vsm, arch, name):
    grid, table, p, T, vmr, broadening, cef, cutoff = _inputs(name)
    return AC.make_model(vsm.Absorption, table, broadening, cef, cutoff, vmr, arch), grid, p, T


def test_chunk_is_the_exported_one(vsm):
    assert vsm._lib.lib().vsm_absorption_chunk() == CHUNK
    assert vsm._lib.lib().vsm_absorption_work_elems(3, 7) == 8 * 3 * 7 and vsm._lib.lib().vsm_absorption_work_elems(0, 7) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_cross_section_against_oracle(vsm, arch, name):
    model, grid, p, T = _model(vsm, arch, name)
    r64, rld = _reference(name)
    if "doppler" not in name and CASES[name][0] > 1:
        assert 0 < np.count_nonzero(r64 == 0) < r64.size, "the case should have points no window reaches"
    got = vsm.Absorption.compute_absorption_cross_section(model, grid, p, T)
    _accept(got, r64, rld, name)
    again = vsm.Absorption.compute_absorption_cross_section(model, grid, p, T)
    assert np.array_equal(got, again), "two calls are not bit-identical"
    if len(p) == 1:                                                      # the reference's call: scalar p, T -> [nSpec]
        one = vsm.Absorption.compute_absorption_cross_section(model, grid, float(p[0]), float(T[0]))
        assert one.shape == (len(grid),) and np.array_equal(one, got[0])


def test_layers_of_a_profile_equal_single_layer_calls(vsm, arch):
    """One call for the profile against one call per layer: bit for bit (the work of a layer does not depend on its neighbours)."""
    name = "n1000_l3c7_voigt_sd"
    model, grid, p, T = _model(vsm, arch, name)
    A = vsm.Absorption
    whole = A.compute_absorption_cross_section(model, grid, p, T)
    for iz in range(len(p)):
        m1 = AC.make_model(A, _inputs(name)[1], "Voigt", SD, 5.0, float(np.asarray(model.vmr)[iz]), arch)
        assert np.array_equal(A.compute_absorption_cross_section(m1, grid, float(p[iz]), float(T[iz])), whole[iz]), iz


@pytest.mark.parametrize("cef", AO.CEFS)
def test_golden_hitran_file(vsm, arch, cef):
    """The reference's CO2 test lines (mol 2, iso 1 and 2; mol 1) at the default cutoff of 40 cm^-1 on 6250 .. 6400 cm^-1."""
    A = vsm.Absorption
    ht = A.read_hitran(AC.GOLDEN_PAR, ν_min=6000, ν_max=6400)
    iso = dict(AC.ISOTOPOLOGUES)
    iso[(2, 2)] = (44.99318, iso[(2, 1)][1], 2.0 * iso[(2, 1)][2])
    iso[(1, 1)] = (18.01056, iso[(7, 1)][1], 0.8 * iso[(7, 1)][2])
    grid = np.linspace(6250.0, 6400.0, 257)
    model = A.make_hitran_model(ht, A.Voigt(), CEF=getattr(A, cef)(), vmr=4e-4, architecture=arch,
                                isotopologues={k: A.IsotopologueData(*v) for k, v in iso.items()})
    kw = dict(vmr=4e-4, broadening="Voigt", cef=cef, wing_cutoff=40.0)
    r64 = AO.cross_section(AC.table_dict(ht), iso, grid, AC.P3, AC.T3, dtype=np.float64, **kw)
    rld = AO.cross_section(AC.table_dict(ht), iso, grid, AC.P3, AC.T3, dtype=np.longdouble, **kw)
    _accept(A.compute_absorption_cross_section(model, grid, AC.P3, AC.T3), r64, rld, "golden " + cef)


def test_wavelength_flag_is_the_reversed_wavenumber_result(vsm, arch):
    A = vsm.Absorption
    model = AC.make_model(A, AC.synthetic_table(77, 300, two_species=True), vmr=0.3, architecture=arch)
    wl = np.linspace(1652.9, 1666.6, 300)                                # nm, ascending
    wn = (1e7 / wl)[::-1]
    a = A.compute_absorption_cross_section(model, wl, AC.P3, AC.T3, wavelength_flag=True)
    b = A.compute_absorption_cross_section(model, wn, AC.P3, AC.T3)
    assert np.count_nonzero(b) > 0 and np.array_equal(a, b[:, ::-1])


def test_empty_selection_and_deviation_case_are_exact_zeros(vsm, arch):
    A = vsm.Absorption
    model = AC.make_model(A, AC.synthetic_table(5, 20), architecture=arch)
    z = A.compute_absorption_cross_section(model, np.linspace(7000.0, 7010.0, 300), AC.P3, AC.T3)
    assert z.shape == (3, 300) and np.all(z == 0)
    t, grid, cutoff, p, T = AC.deviation_case()
    ref = AO.cross_section(t, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff)
    got = A.compute_absorption_cross_section(AC.make_model(A, t, wing_cutoff=cutoff, architecture=arch), grid, p, T)
    assert np.all(ref == 0) and got.shape == ref.shape and np.all(got == 0)
    # the same line beside one that does reach the grid: only the second contributes
    t2 = {k: np.concatenate([v, v]) for k, v in t.items()}
    t2["nu"][1] = 6000.4
    ref2 = AO.cross_section(t2, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff)
    got2 = A.compute_absorption_cross_section(AC.make_model(A, t2, wing_cutoff=cutoff, architecture=arch), grid, p, T)
    _accept(got2, ref2, AO.cross_section(t2, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff, dtype=np.longdouble), "deviation + 1")


def _profile_case(vsm, arch):
    A = vsm.Absorption
    ta = AC.synthetic_table(41, CHUNK + 9, no_E_share=0.1)
    tb = AC.synthetic_table(42, 60, two_species=True)
    tc = AC.synthetic_table(43, 4, lo=7000.0, hi=7001.0)                 # no line near the grid
    vcd = np.array([3.1e21, 2.2e23, 1.9e24])
    vmr_a, vmr_b = 4.1e-4, np.array([0.21, 0.2, 0.19])
    pairs = [(AC.make_model(A, tc, architecture=arch), 1e-6), (AC.make_model(A, ta, vmr=vmr_a, architecture=arch), vmr_a),
             (AC.make_model(A, tb, vmr=vmr_b, architecture=arch), vmr_b)]
    gases = [(tc, AC.ISOTOPOLOGUES, 0.0, 1e-6), (ta, AC.ISOTOPOLOGUES, vmr_a, vmr_a), (tb, AC.ISOTOPOLOGUES, vmr_b, vmr_b)]
    return pairs, gases, vcd


def test_accumulate_sums_two_gases_on_the_device(vsm, arch):
    A = vsm.Absorption
    pairs, gases, vcd = _profile_case(vsm, arch)
    grid = AC.nonuniform_grid(300, 12)
    both = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd)
    one = A.compute_absorption_profile(pairs[1:2], grid, AC.P3, AC.T3, vcd)
    two = A.compute_absorption_profile(pairs[2:3], grid, AC.P3, AC.T3, vcd)
    assert both.shape == (300, 3) and np.count_nonzero(one) > 0 and np.count_nonzero(two) > 0
    assert np.all(np.abs(both - (one + two)) <= np.spacing(np.maximum(one, two)))
    tau, dots = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd, lin=True)
    assert np.array_equal(tau, both) and len(dots) == 3 and np.all(dots[0] == 0)
    ref64, dots64 = AO.absorption_profile(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0)
    refld, dotsld = AO.absorption_profile(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0, dtype=np.longdouble)
    _accept(tau, ref64, refld, "tau_abs of two gases")
    for g in (1, 2):
        _accept(dots[g], dots64[g], dotsld[g], "tau_abs_dot[%d]" % g)


def test_profile_feeds_rt_run(vsm, arch):
    """compute_absorption_profile -> model_from_arrays -> CoreRT.rt_run at nSpec = 64 equals the run on the oracle's tau_abs within
    the FP64 end-to-end parity bound of test_gpu_parity.py (1e-8 of the largest element)."""
    A = vsm.Absorption
    pairs, gases, vcd = _profile_case(vsm, arch)
    grid = AC.nonuniform_grid(64, 13, lo=6010.0, hi=6040.0)
    vcd = vcd * 0.05                                                     # column tau_abs from below 1e-3 to a few
    tau = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd)
    ref = AO.absorption_profile(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0)[0]
    assert tau.shape == (64, 3) and tau.min() >= 0 and tau.sum(axis=1).min() < 1e-3 and tau.sum(axis=1).max() > 0.5
    tau_rayl = np.tile(0.02 * np.array([0.05, 0.25, 0.7]), (64, 1))
    out = []
    for ta in (tau, ref):
        m = vsm.host_model.model_from_arrays(arch, "IQU", 8, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=ta, depol=0.0279,
                                             albedo=0.15, m_max=2)
        out.append(vsm.CoreRT.rt_run(m))
    for got, want in zip(out[0], out[1]):
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-8
