"""GPU tests of the linearized Absorption (vsm_absorption_xsec_lin, csrc/vsm_absorption.hip) against tests/absorption_lin_oracle.py,
through the public functions, on the seeded synthetic tables of tests/absorption_cases.py.

Acceptance per (case, slot) -- slots T, p, vmr_self:
 (a) the pattern of exact zeros equals the oracle's at every (layer, point), Doppler's identically-zero vmr_self slot included;
 (b) |device - oracle64| / A80 <= 10 x max(floor, 1e-14), with A80 the absolute term sum of the slot in the 80-bit format
     (sum_lines |pre dlnpre F| + |pre F_x x_theta| + |pre F_y y_theta|: a derivative is a sum of terms of both signs, so a relative
     deviation from the sum itself means nothing near its zeros) and floor = max |oracle64 - oracle80| / A80, computed here on the CPU
     and never from the code under test.  The factor 10 is the forward tests', for the same reason: the device's exp, pow and expm1
     differ from libm by a few ulp, and FMA contraction.  A case whose floor exceeds 1e-7 tests nothing and is not admitted.
sigma of the linearized call is held to the forward call bit for bit on every case.

Shapes: nSpec = 1, 255 / 256 / 257 (the edges of the 256-point tile), 1000 on a non-uniform grid; nLines = 1, c - 1, c, c + 1,
3 c + 7 with c = vsm_absorption_lin_chunk(); Nz = 1 and 3 (p 0.1 .. 1013 hPa, T 180 .. 320 K: every region of both error functions);
per-layer vmr, E'' = -1 lines, two species.  The lines sit in the middle of the grid with a cutoff of a tenth of its span, so each case
has points no window reaches; Doppler at a cutoff of 0.1 cm^-1, as the forward tests."""
import functools

import numpy as np
import pytest

import absorption_cases as AC
import absorption_lin_oracle as AL
import absorption_oracle as AO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SD, HW, CPF = AO.CEFS[1], AO.CEFS[0], AO.CEFS[2]
CHUNK = 256      # asserted against the library in test_chunk_is_the_exported_one
FLOOR_LIMIT = 1e-7

# name: (nSpec, non-uniform grid seed or None, nLines, Nz, broadening, cef, self-vmr, cutoff, table options)
CASES = {
    "n1_l1_voigt_sd": (1, None, 1, 1, "Voigt", SD, 0.0, 5.0, dict(lo=6021.0, hi=6029.0)),
    "n1_lc_voigt_hw": (1, None, CHUNK, 3, "Voigt", HW, 0.3, 5.0, dict(lo=6021.0, hi=6029.0)),
    "n255_lcm1_voigt_hw": (255, None, CHUNK - 1, 3, "Voigt", HW, 0.3, 5.0, {}),
    "n256_lc_doppler": (256, None, CHUNK, 1, "Doppler", SD, 0.0, 0.1, {}),
    "n257_lcp1_lorentz": (257, None, CHUNK + 1, 3, "Lorentz", SD, "layers", 5.0, dict(no_E_share=0.3)),
    "n257_l1_voigt_sd": (257, None, 1, 3, "Voigt", SD, 0.0, 5.0, {}),
    "n1000_l3c7_voigt_sd": (1000, 31, 3 * CHUNK + 7, 3, "Voigt", SD, "layers", 5.0, dict(two_species=True, no_E_share=0.2)),
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
    """(oracle64 slots, oracle80 slots, A80) of a case, each [3, Nz, nSpec]: computed once, shared, never changed."""
    grid, table, p, T, vmr, broadening, cef, cutoff = _inputs(name)
    kw = dict(vmr=vmr, broadening=broadening, cef=cef, wing_cutoff=cutoff)
    r64 = AL.cross_section_lin(table, AC.ISOTOPOLOGUES, grid, p, T, dtype=np.float64, **kw)[0]
    rld, Ald = AL.cross_section_lin(table, AC.ISOTOPOLOGUES, grid, p, T, dtype=np.longdouble, **kw)
    for a in (r64, rld, Ald):
        a.setflags(write=False)
    return r64, rld, Ald


def _accept(dev, r64, rld, Ald, what):
    """(a) and (b) of the module docstring for one slot; prints the figures before it asserts."""
    assert dev.shape == r64.shape and dev.dtype == np.float64, (what, dev.shape, r64.shape)
    assert np.all(np.isfinite(dev)), what
    # (b) over the points where the FP64 oracle is not an exact zero, as the forward tests take it: outside every window, and where
    # Doppler's exp(-ln 2 x^2) underflows to zero in FP64 (a window edge rounded outwards to a point 40 gamma_d away) -- (a) holds there
    nz = r64 != 0
    assert np.all(Ald[nz] > 0)
    floor = float(np.max(np.abs(r64[nz].astype(np.longdouble) - rld[nz]) / Ald[nz])) if nz.any() else 0.0
    bound = 10 * max(floor, 1e-14)
    d = float(np.max(np.abs(dev[nz].astype(np.longdouble) - r64[nz].astype(np.longdouble)) / Ald[nz])) if nz.any() else 0.0
    print("absorption lin %s: %d of %d points zero; floor %.2e, bound %.2e, max dev / A %.2e"
          % (what, int((r64 == 0).sum()), r64.size, floor, bound, d))
    assert floor <= FLOOR_LIMIT, (what, floor)
    assert np.array_equal(dev == 0, r64 == 0), (what, int((dev == 0).sum()), int((r64 == 0).sum()))            # (a)
    assert d <= bound, (what, d, bound)                                                                        # (b)


def _model(vsm, arch, name):
    grid, table, p, T, vmr, broadening, cef, cutoff = _inputs(name)
    return AC.make_model(vsm.Absorption, table, broadening, cef, cutoff, vmr, arch), grid, p, T


def test_chunk_is_the_exported_one(vsm):
    lib = vsm._lib.lib()
    assert lib.vsm_absorption_lin_chunk() == CHUNK
    assert lib.vsm_absorption_lin_work_elems(3, 7) == (8 + 10) * 3 * 7 and lib.vsm_absorption_lin_work_elems(0, 7) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_cross_section_lin_against_oracle(vsm, arch, name):
    A = vsm.Absorption
    model, grid, p, T = _model(vsm, arch, name)
    r64, rld, Ald = _reference(name)
    if "doppler" not in name and CASES[name][0] > 1:
        assert 0 < np.count_nonzero(Ald[0] == 0) < Ald[0].size, "the case should have points no window reaches"
    sig, dot = A.compute_absorption_cross_section_lin(model, grid, p, T)
    assert np.array_equal(sig, A.compute_absorption_cross_section(model, grid, p, T)), "sigma is not the forward call's bit for bit"
    assert dot.shape == (3, len(p), len(grid))
    for k, slot in enumerate(AL.SLOTS):
        _accept(dot[k], r64[k], rld[k], Ald[k], "%s d/d%s" % (name, slot))
    if "doppler" in name:
        assert np.all(dot[2] == 0)
    sig2, dot2 = A.compute_absorption_cross_section_lin(model, grid, p, T)
    assert np.array_equal(sig, sig2) and np.array_equal(dot, dot2), "two calls are not bit-identical"
    if len(p) == 1:                                                      # scalar p, T -> [nSpec], [3, nSpec]
        s1, d1 = A.compute_absorption_cross_section_lin(model, grid, float(p[0]), float(T[0]))
        assert s1.shape == (len(grid),) and d1.shape == (3, len(grid)) and np.array_equal(s1, sig[0]) and np.array_equal(d1, dot[:, 0])


def test_layers_of_a_profile_equal_single_layer_calls(vsm, arch):
    name = "n1000_l3c7_voigt_sd"
    model, grid, p, T = _model(vsm, arch, name)
    A = vsm.Absorption
    sig, dot = A.compute_absorption_cross_section_lin(model, grid, p, T)
    for iz in range(len(p)):
        m1 = AC.make_model(A, _inputs(name)[1], "Voigt", SD, 5.0, float(np.asarray(model.vmr)[iz]), arch)
        s1, d1 = A.compute_absorption_cross_section_lin(m1, grid, float(p[iz]), float(T[iz]))
        assert np.array_equal(s1, sig[iz]) and np.array_equal(d1, dot[:, iz]), iz


def test_wavelength_flag_is_the_reversed_wavenumber_result(vsm, arch):
    A = vsm.Absorption
    model = AC.make_model(A, AC.synthetic_table(77, 300, two_species=True), vmr=0.3, architecture=arch)
    wl = np.linspace(1652.9, 1666.6, 300)                                # nm, ascending
    wn = (1e7 / wl)[::-1]
    sa, da = A.compute_absorption_cross_section_lin(model, wl, AC.P3, AC.T3, wavelength_flag=True)
    sb, db = A.compute_absorption_cross_section_lin(model, wn, AC.P3, AC.T3)
    assert all(np.count_nonzero(db[k]) > 0 for k in range(3))
    assert np.array_equal(sa, sb[:, ::-1]) and np.array_equal(da, db[:, :, ::-1])


def test_empty_selection_and_deviation_case_are_exact_zeros(vsm, arch):
    A = vsm.Absorption
    model = AC.make_model(A, AC.synthetic_table(5, 20), architecture=arch)
    s, d = A.compute_absorption_cross_section_lin(model, np.linspace(7000.0, 7010.0, 300), AC.P3, AC.T3)
    assert s.shape == (3, 300) and d.shape == (3, 3, 300) and np.all(s == 0) and np.all(d == 0)
    t, grid, cutoff, p, T = AC.deviation_case()
    ref = AL.cross_section_lin(t, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff)[0]
    s, d = A.compute_absorption_cross_section_lin(AC.make_model(A, t, wing_cutoff=cutoff, architecture=arch), grid, p, T)
    assert np.all(ref == 0) and d.shape == ref.shape and np.all(d == 0) and np.all(s == 0)
    # the same line beside one that does reach the grid: only the second contributes
    t2 = {k: np.concatenate([v, v]) for k, v in t.items()}
    t2["nu"][1] = 6000.4
    r64 = AL.cross_section_lin(t2, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff)[0]
    rld, Ald = AL.cross_section_lin(t2, AC.ISOTOPOLOGUES, grid, p, T, wing_cutoff=cutoff, dtype=np.longdouble)
    s, d = A.compute_absorption_cross_section_lin(AC.make_model(A, t2, wing_cutoff=cutoff, architecture=arch), grid, p, T)
    for k, slot in enumerate(AL.SLOTS):
        _accept(d[k], r64[k], rld[k], Ald[k], "deviation + 1 d/d%s" % slot)


def test_cpf12_is_refused(vsm, arch):
    A = vsm.Absorption
    model = AC.make_model(A, AC.synthetic_table(5, 20), cef=CPF, architecture=arch)
    with pytest.raises(NotImplementedError, match="CPF12"):
        A.compute_absorption_cross_section_lin(model, AC.uniform_grid(64), AC.P3, AC.T3)


def _profile_case(vsm, arch, wing_cutoff=5.0):
    A = vsm.Absorption
    ta = AC.synthetic_table(41, CHUNK + 9, no_E_share=0.1)
    tb = AC.synthetic_table(42, 60, two_species=True)
    tc = AC.synthetic_table(43, 4, lo=7000.0, hi=7001.0)                 # no line near the grid
    vcd = np.array([3.1e21, 2.2e23, 1.9e24])
    vmr_a, vmr_b = 4.1e-4, np.array([0.21, 0.2, 0.19])
    mk = lambda t, **kw: AC.make_model(A, t, wing_cutoff=wing_cutoff, architecture=arch, **kw)
    pairs = [(mk(tc), 1e-6), (mk(ta, vmr=vmr_a), vmr_a), (mk(tb, vmr=vmr_b), vmr_b)]
    gases = [(tc, AC.ISOTOPOLOGUES, 0.0, 1e-6), (ta, AC.ISOTOPOLOGUES, vmr_a, vmr_a), (tb, AC.ISOTOPOLOGUES, vmr_b, vmr_b)]
    return pairs, gases, vcd


def test_profile_lin_of_two_gases(vsm, arch):
    A = vsm.Absorption
    pairs, gases, vcd = _profile_case(vsm, arch)
    grid = AC.nonuniform_grid(300, 12)
    tau, dots = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd, lin=True)
    T_dot = np.vstack([np.eye(3), np.ones((1, 3))])                      # a unit table per layer, and a profile shift
    p_dot = np.vstack([np.zeros((3, 3)), (AC.P3 / AC.P3[-1])[None]])     # ... with the surface-pressure table beside the shift
    r = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd, T_dot=T_dot, p_dot=p_dot)
    assert np.array_equal(r.tau_abs, tau) and len(r.tau_abs_dot) == 3
    assert all(np.array_equal(a, b) for a, b in zip(r.tau_abs_dot, dots))
    (dT, dp, dv), _ = AL.absorption_profile_lin(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0)
    (dTl, dpl, dvl), (AT, Ap, Av) = AL.absorption_profile_lin(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0, dtype=np.longdouble)
    _accept(r.dtau_dT, dT, dTl, AT, "dtau_dT of two gases")
    _accept(r.dtau_dp, dp, dpl, Ap, "dtau_dp of two gases")
    assert np.all(r.dtau_dvmr_self[0] == 0)
    for g in (1, 2):
        _accept(r.dtau_dvmr_self[g], dv[g], dvl[g], Av[g], "dtau_dvmr_self[%d]" % g)
    assert r.profile_slots.shape == (4, 300, 3)
    for k in range(3):
        want = np.zeros((300, 3))
        want[:, k] = r.dtau_dT[:, k]
        assert np.array_equal(r.profile_slots[k], want), k
    shift = r.dtau_dT + r.dtau_dp * (AC.P3 / AC.P3[-1])[None, :]         # one product and one sum per element: FMA or not, 1 ulp
    assert np.all(np.abs(r.profile_slots[3] - shift) <= np.spacing(np.abs(r.dtau_dT) + np.abs(r.dtau_dp)))
    again = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd, T_dot=T_dot, p_dot=p_dot)
    for a, b in zip(r.lin_model_slots() + [r.dtau_dT, r.dtau_dp] + r.dtau_dvmr_self,
                    again.lin_model_slots() + [again.dtau_dT, again.dtau_dp] + again.dtau_dvmr_self):
        assert np.array_equal(a, b)


def test_profile_lin_feeds_rt_run_lin(vsm, arch):
    """nSpec = 64, Nz = 3, Stokes_IQU, Rayleigh and one gas, its column-amount slot and one profile-shift slot in T:
    rt_run_lin on lin_model_slots() against (1) the same run on the oracle's tau_abs and slots, within the 1e-8 of test_gpu_parity.py,
    and (2) central differences, dT = 1 K, of compute_absorption_profile -> rt_run, at the bounds of test_gpu_mie_lin.py's run check
    (err.max() < 1e-3 and err.mean() < 1e-4 of the largest |slot|).  The cutoff is wider than the grid, so no window moves; the
    truncation at dT / T = 4e-3 is about 1e-5, and a point that crosses |x| + y = 8 adds at most the approximants' 2.3e-6 mismatch
    divided by the step, about 3e-4 of one line's term."""
    A, H = vsm.Absorption, vsm.host_model
    table = AC.synthetic_table(41, 120, no_E_share=0.1)
    grid = AC.nonuniform_grid(64, 13, lo=6010.0, hi=6040.0)
    vcd = 2.0 * np.array([3.1e21, 2.2e23, 1.9e24])                      # column tau_abs from 4e-4 to 0.8
    vmr, cutoff = 4.1e-4, 60.0
    pair = lambda: [(AC.make_model(A, table, wing_cutoff=cutoff, vmr=vmr, architecture=arch), vmr)]
    gases = [(table, AC.ISOTOPOLOGUES, vmr, vmr)]
    r = A.compute_absorption_profile_lin(pair(), grid, AC.P3, AC.T3, vcd, T_dot=np.ones((1, 3)))
    slots = r.lin_model_slots()
    assert len(slots) == 2 and r.tau_abs.shape == (64, 3) and r.tau_abs.sum(axis=1).min() < 1e-3 and r.tau_abs.sum(axis=1).max() > 0.5
    tau_o, dots_o = AO.absorption_profile(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=cutoff)
    (dT_o, _, _), _ = AL.absorption_profile_lin(gases, grid, AC.P3, AC.T3, vcd, wing_cutoff=cutoff)
    tau_rayl = np.tile(0.02 * np.array([0.05, 0.25, 0.7]), (64, 1))

    def model(ta):
        return H.model_from_arrays(arch, "IQU", 8, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=ta, depol=0.0279, albedo=0.15, m_max=2)

    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(model(r.tau_abs), H.LinModel(tau_abs_dot=slots), 0, 2, 1)
    Ro, To, Rdo, Tdo = vsm.CoreRTLin.rt_run_lin(model(tau_o), H.LinModel(tau_abs_dot=[dots_o[0], dT_o]), 0, 2, 1)
    for got, want in ((R, Ro), (T, To), (Rd[..., 0], Rdo[..., 0]), (Td[..., 0], Tdo[..., 0]), (Rd[..., 1], Rdo[..., 1]),
                      (Td[..., 1], Tdo[..., 1])):
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-8
    h = 1.0
    (Rp, Tp), (Rm, Tm) = (vsm.CoreRT.rt_run(model(A.compute_absorption_profile(pair(), grid, AC.P3, AC.T3 + s, vcd))) for s in (h, -h))
    for an, fd in ((Rd[..., 1], (Rp - Rm) / (2 * h)), (Td[..., 1], (Tp - Tm) / (2 * h))):
        err = np.abs(fd - an) / np.abs(fd).max()
        print("absorption lin end to end, T shift: err max %.2e mean %.2e" % (err.max(), err.mean()))
        assert err.max() < 1e-3 and err.mean() < 1e-4, (err.max(), err.mean())
