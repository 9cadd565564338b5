"""CPU tests of tests/mie_oracle.py (the numpy restatement of the reference's NAI-2 Mie path) against numbers that are not ours:
published single-sphere efficiencies, the Rayleigh limit, the identities a Greek expansion satisfies -- and of the host part of
vsm.Scattering against the oracle's, bit for bit; and, for the edge cases of tests/mie_cases.py, of the two conditions the GPU edge
tests (tests/test_gpu_mie_edges.py) rest on: a defect of one order, radius or angle moves the outputs by >= 1e-6, and the float64
oracle stays within 1e-10 of its long-double form.  No kernel runs here."""
import math
import os
import re
import types

import numpy as np
import pytest

import mie_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_AEROSOL = dict(r_m=0.3, sigma_g=2.1, n_r=1.3, n_i=0.001, wavelength=0.55)     # the reference's test aerosol (test_mie_gpu.jl)


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


@pytest.fixture(scope="module")
def test_aerosol_optics():
    a = TEST_AEROSOL
    return MO.compute_aerosol_optical_properties(MO.LogNormal(a["r_m"], a["sigma_g"]), a["n_r"], a["n_i"], a["wavelength"], 3.0, 37)


# x, n_r, n_i, Q_ext, Q_sca: Bohren & Huffman app. A (3.10543), Wiscombe 1979 (2.881999; 2.094388; 2.459791 / 1.235144)
SPHERES = [(2 * math.pi * 0.525 / 0.6328, 1.55, 0.0, 3.1054255, 3.1054255),
           (10.0, 1.5, 0.0, 2.8819990, 2.8819990),
           (100.0, 1.5, 0.0, 2.0943878, 2.0943878),
           (10.0, 1.5, 0.1, 2.4597905, 1.2351442)]


@pytest.mark.parametrize("x,n_r,n_i,q_ext,q_sca", SPHERES)
def test_single_sphere_efficiencies(x, n_r, n_i, q_ext, q_sca):
    """nquad = 1: Q = C / (pi r^2) to 1e-6 relative."""
    o = MO.monodisperse(x, n_r, n_i)
    r = float(o.host.r[0])
    assert o.host.x[0] == x
    assert abs(o.C_ext / (math.pi * r * r) - q_ext) <= 1e-6 * q_ext
    assert abs(o.C_sca / (math.pi * r * r) - q_sca) <= 1e-6 * q_sca


def test_rayleigh_limit_fixes_the_sign_conventions():
    """x = 1e-3, m = 1.5: get_greek_rayleigh(0) -- beta = [1, 0, 1/2], alpha_2 = 3, gamma_2 = +sqrt(1.5), delta_1 = 1.5, everything
    else 0 -- to 1e-5 (the deviation is O(x^2) = 1e-6).  n_max_i = 1 here; n_max = 2 is the floor of mie_inputs."""
    o = MO.monodisperse(1e-3, 1.5, 0.0)
    assert (o.host.n_max, o.host.n_mu, int(o.host.nmax_i[0])) == (2, 3, 1)
    want = np.stack(MO.get_greek_rayleigh(0.0))
    assert want[2, 2] == math.sqrt(1.5) and want[3, 1] == 1.5 and want[0, 2] == 3.0
    assert o.greek.shape == (6, 3)
    assert np.max(np.abs(o.greek - want)) <= 1e-5, o.greek - want


def test_identities_on_the_test_aerosol(vsm, test_aerosol_optics):
    o = test_aerosol_optics
    assert (o.host.n_max, o.host.n_mu) == (57, 113)
    assert abs(o.greek[1, 0] - 1.0) <= 1e-12
    assert 0.0 < o.ssa < 1.0
    a = TEST_AEROSOL
    o0 = MO.compute_aerosol_optical_properties(MO.LogNormal(a["r_m"], a["sigma_g"]), a["n_r"], 0.0, a["wavelength"], 3.0, 37)
    assert abs(o0.ssa - 1.0) <= 1e-12
    g = vsm.host_model.GreekCoefs(*o.greek)
    rec = np.array([vsm.StandaloneSS.reconstruct_phase(g, float(m)) for m in o.mu])
    scale = np.max(o.bulk_f[0])
    assert np.max(np.abs(rec[:, 0] - o.bulk_f[0])) <= 1e-10 * scale
    assert np.max(np.abs(rec[:, 1] - o.bulk_f[2])) <= 1e-10 * scale


def test_get_n_max_has_both_branches(vsm):
    S = vsm.Scattering
    assert S.get_n_max(8.0) == round(8.0 + 4.0 * 2.0 + 1) == 17             # x <= 8
    assert S.get_n_max(8.5) == round(8.5 + 4.05 * 8.5 ** (1 / 3) + 10) == 27  # x > 8
    for x in (1e-3, 0.5, 7.999, 8.0, 8.0000001, 8.5, 100.0, 200.0, 500.0):
        assert S.get_n_max(x) == MO.get_n_max(x)
    assert S.get_n_max(500.0) == 542


CASES = [(3.0, 37), (3.0, 7), (0.5, 16), (30.0, 100)]


@pytest.mark.parametrize("r_max,nquad", CASES)
def test_host_part_equals_the_oracle_bit_for_bit(vsm, r_max, nquad):
    S = vsm.Scattering
    a = TEST_AEROSOL
    h = S.mie_host_inputs(S.make_mie_model(S.Aerosol(S.LogNormal(a["r_m"], a["sigma_g"]), a["n_r"], a["n_i"]), a["wavelength"],
                                           r_max, nquad))
    o = MO.mie_inputs(MO.LogNormal(a["r_m"], a["sigma_g"]), a["wavelength"], r_max, nquad)
    assert (h.n_max, h.n_mu, h.k_wave) == (o.n_max, o.n_mu, o.k_wave) and h.n_mu == 2 * h.n_max - 1
    for name in ("r", "wx", "wr", "x", "nmax_i", "mu", "w_mu"):
        assert np.array_equal(getattr(h, name), getattr(o, name)), name
    assert h.nmax_i.dtype == np.int32 and abs(h.wx.sum() - 1.0) <= 1e-14
    # the tabulated input fed the LogNormal nodes and unnormalised weights gives the same arrays
    r, w_r = S.gauleg_log(nquad, max(S.LogNormal(a["r_m"], a["sigma_g"]).quantile(1e-8), 1e-6 * r_max), r_max)
    tab = S.TabulatedSizeDistribution(r, S.LogNormal(a["r_m"], a["sigma_g"]).pdf(r) * w_r)
    ht = S.mie_host_inputs(S.make_mie_model(S.Aerosol(tab, a["n_r"], a["n_i"]), a["wavelength"]))
    for name in ("r", "wx", "wr", "x", "nmax_i", "mu", "w_mu"):
        assert np.array_equal(getattr(h, name), getattr(ht, name)), name


def test_host_refusals_and_the_library_cap(vsm):
    S = vsm.Scattering
    ln = S.LogNormal(0.3, 2.1)
    with pytest.raises(vsm.VSMError):                       # n_i < 0
        S.mie_host_inputs(S.make_mie_model(S.Aerosol(ln, 1.3, -0.001), 0.55, 3.0, 37))
    with pytest.raises(vsm.VSMError):                       # r_max <= r_min = quantile(1e-8) = 4.7e-3
        S.mie_host_inputs(S.make_mie_model(S.Aerosol(ln, 1.3, 0.0), 0.55, 4.0e-3, 37))
    with pytest.raises(vsm.VSMError):                       # nquad_radius < 1
        S.mie_host_inputs(S.make_mie_model(S.Aerosol(ln, 1.3, 0.0), 0.55, 3.0, 0))
    with pytest.raises(vsm.VSMError):                       # n_max above the cap: x_max = 1100
        S.mie_host_inputs(S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution([1100.0], [1.0]), 1.3, 0.0), MO.MONO_WAVELENGTH))
    with pytest.raises(vsm.VSMError):                       # no CPU fallback
        S.compute_aerosol_optical_properties(S.make_mie_model(S.Aerosol(ln, 1.3, 0.0), 0.55, 3.0, 37), vsm.Architectures.CPU())
    header = open(os.path.join(ROOT, "include", "vsmartmom_hip.h")).read()
    cap = re.findall(r"#define\s+VSM_MIE_MAX_NMAX\s+(\d+)", header)
    assert len(cap) == 1 and int(cap[0]) == S.MAX_N_MAX >= 600
    lib = vsm._lib.lib()
    assert lib.vsm_mie_work_elems(37, 57, 113) > 6 * 60 * 64 and lib.vsm_mie_work_elems(37, 57, 112) == 0
    assert lib.vsm_mie_work_elems(1, S.MAX_N_MAX, 2 * S.MAX_N_MAX - 1) > 0 and lib.vsm_mie_work_elems(1, S.MAX_N_MAX + 1, 2 * S.MAX_N_MAX + 1) == 0
    # x = 500 runs: n_max = 542 is inside the cap
    h = S.mie_host_inputs(S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution([500.0], [1.0]), 1.5, 0.1), MO.MONO_WAVELENGTH))
    assert (h.n_max, h.n_mu) == (542, 1083)


def test_fine_mode_aerosol_drops_into_model_from_arrays(vsm):
    """The oracle's optics of the end-to-end case as a host_model.AerosolOptics: the layer optics of the host model equal the
    oracle model's (19 coefficients under l_trunc = 20)."""
    from oracle import vsm_oracle as O
    H = vsm.host_model
    o = MO.compute_aerosol_optical_properties(MO.LogNormal(0.08, 1.6), 1.45, 0.005, 0.76, 0.35, 20)
    assert (o.host.n_max, o.host.n_mu) == (10, 19)
    S, L = 8, 2
    tau_rayl = np.tile(0.02 * np.ones(L), (S, 1))
    tau_abs = np.tile(np.linspace(0.0, 0.5, S)[:, None], (1, L))
    tau_aer = np.array([[0.05, 0.2]])
    pm = H.model_from_arrays(vsm.Architectures.CPU(), "IQU", 20, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs,
                             tau_aer=tau_aer, aerosol_optics=[H.AerosolOptics(H.GreekCoefs(*o.greek), o.ssa, 0.0)], depol=0.03,
                             albedo=0.1, m_max=3)
    om = O.build_model("IQU", 20, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, tau_aer=tau_aer,
                       aerosols=[O.AerosolOptics(O.GreekCoefs(*o.greek), o.ssa, 0.0)], depol=0.03, albedo=0.1, m_max=3)
    for m in (0, 2):
        for a, b in zip(H.constructCoreOpticalProperties(pm, m), O.construct_core_optical_properties(om, m)):
            assert np.allclose(a.tau, b.tau, rtol=1e-15) and np.allclose(a.varpi, b.varpi, rtol=1e-15)
            assert np.allclose(a.Zpp, b.Zpp, rtol=1e-12, atol=1e-13)


# ---- the edge cases of tests/mie_cases.py: recipe, float64 path unchanged, sensitivity, rounding floor ---------------------------------
import mie_cases as MC

GOLDEN_F64, GOLDEN_CASES, SENSITIVITY = MC.GOLDEN_F64, MC.GOLDEN_CASES, MC.SENSITIVITY
perturbations, greek_move = MC.perturbations, MC.greek_move


def test_cases_follow_the_recipe():
    assert [(c.nquad, c.n_max) for c in MC.CASES[:11]] == MC.SHAPES and len(MC.CASES) == 14 and len(set(MC.NAMES)) == 14
    for c in MC.CASES:
        h = MC.inputs(c)
        top = c.n_max if c.cap is None else c.cap
        nm = h.nmax_i
        assert nm.dtype == np.int32 and nm.shape == (c.nquad,) and nm.min() >= 1 and nm.max() == top
        if c.nquad > 1:
            assert nm.min() == 1 and np.any(np.diff(nm) > 0) and np.any(np.diff(nm) < 0), c.name       # at 1; unsorted
        if c.n_max >= 6:
            have = set(nm.tolist())
            assert any({4 * j - 1, 4 * j, 4 * j + 1} <= have for j in range(1, top // 4 + 1)), c.name
        u = h.x / (nm + 1)
        assert np.all(u >= 1.0) and np.all(u <= 1.3) and np.all(h.x > nm)                              # cut-offs below x
        assert np.all(h.wx > 0) and abs(h.wx.sum() - 1) <= 1e-15 and np.all(h.wx * c.nquad < 3) and np.all(h.wx * c.nquad > 1 / 3)
        assert np.array_equal(h.wr, 4 * math.pi * h.x ** 2 * h.wx) and np.array_equal(h.wr_dot, 4 * math.pi * h.x ** 2 * h.wx_dot)
        assert h.k_wave == 1.0 and h.n_mu == 2 * c.n_max - 1 == len(h.mu) == len(h.w_mu)
        assert h.wx_dot.shape == (2, c.nquad) and np.all(np.abs(h.wx_dot.sum(axis=1)) <= 1e-15)
        if c.nquad > 1:
            assert np.any(h.wx_dot > 0) and np.any(h.wx_dot < 0)
        again = MC.inputs(c)
        assert all(np.array_equal(getattr(h, k), getattr(again, k)) for k in ("x", "wx", "wx_dot", "nmax_i"))
    assert MC.inputs(MC.BY_NAME["q33_n32_cap20"]).nmax_i.max() == 20
    assert MC.BY_NAME["q33_n32_real"].m == (1.33, 0.0) and MC.BY_NAME["q33_n32_absorbing"].m == (2.0, 1.0)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_float64_path_is_the_recorded_one_bit_for_bit(name):
    """The default path against what the oracle returned before it took a dtype (tests/golden/mie_oracle_float64.npz)."""
    want = np.load(GOLDEN_F64)
    h = MC.inputs(MC.BY_NAME[name])
    greek, scal, bulk = MO.nai2_reference(*MC.forward_args(h))
    assert greek.dtype == bulk.dtype == np.float64
    assert np.array_equal(greek, want[name + "/greek"]) and np.array_equal(bulk, want[name + "/bulk_f"])
    assert np.array_equal(np.array(scal, dtype=np.float64), want[name + "/scal"])
    for explicit in (MO.nai2_reference(*MC.forward_args(h), dtype=np.float64), MO.nai2_reference(*MC.forward_args(h), scales=True)):
        assert np.array_equal(explicit[0], greek) and explicit[1] == scal and np.array_equal(explicit[2], bulk)
    # stage 3 factored out: the same numbers from the bulk functions alone
    assert np.array_equal(MO.greek_from_bulk(bulk, scal[0], h.mu, h.w_mu), greek)


def test_long_double_path_widens_the_arithmetic_only():
    h = MC.inputs(MC.BY_NAME["q33_n32"])
    g64, s64, b64 = MO.nai2_reference(*MC.forward_args(h))
    gld, sld, bld, S = MO.nai2_reference(*MC.forward_args(h), dtype=np.longdouble, scales=True)
    assert gld.dtype == bld.dtype == np.longdouble and isinstance(sld[0], np.longdouble) and np.finfo(np.longdouble).nmant >= 63
    assert S.bulk_abs.dtype == np.longdouble and np.all(S.bulk_abs > 0) and S.c_abs[0] > 0 and S.c_abs[1] > 0
    for a, b in ((g64, gld), (b64, bld)):
        dev = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        assert 0 < dev < 1e-12, dev                          # not the same numbers, and no further apart than float64 rounding
    for fn, args in ((MO.compute_mie_pi_tau, (h.mu, 5)), (MO.compute_legendre_poly, (h.mu, 5)),
                     (MO.compute_mie_ab, (h.x, complex(1.4, -0.01), h.nmax_i, 32))):
        assert all(a.dtype in (np.longdouble, np.clongdouble) for a in fn(*args, dtype=np.longdouble))
        assert all(a.dtype in (np.float64, np.complex128) for a in fn(*args))
    with pytest.raises(ValueError):
        MO.nai2_reference(*MC.forward_args(h), dtype=np.float32)


@pytest.mark.parametrize("name", MC.NAMES)
def test_a_defect_of_one_order_radius_or_angle_moves_the_coefficients(name):
    """Sensitivity: each perturbation moves at least one Greek vector by >= 1e-6 of max(1, max |vector|) -- three decades above the
    largest bound tests/test_gpu_mie_edges.py may assert (1e-9)."""
    c = MC.BY_NAME[name]
    h = MC.inputs(c)
    base = MO.nai2_reference(*MC.forward_args(h))[0]
    least = (math.inf, None)
    for what, change in perturbations(h, c.n_max):
        d = dict(vars(h))
        d.update(change)
        move = greek_move(MO.nai2_reference(*MC.forward_args(types.SimpleNamespace(**d)))[0], base)
        least = min(least, (move, what))
        assert move >= SENSITIVITY, (name, what, move)
    print("mie sensitivity %s: least move %.2e (%s)" % (name, least[0], least[1]))


@pytest.mark.parametrize("name", MC.NAMES)
def test_rounding_floor_of_the_forward_outputs(name):
    """Floor: float64 against long double on the comparison scales, over the oracle itself and eight runs with every x_i one ulp
    off; no case above 1e-10."""
    ref, floor = MC.case_floors(name)
    print("mie floor %s: %s" % (name, "  ".join("%s %.1e" % (f, floor[f]) for f in MC.FORWARD)))
    for f in MC.FORWARD:
        assert MC.MIN_FLOOR <= floor[f] <= MC.FLOOR_LIMIT, (name, f, floor[f])
    if MC.BY_NAME[name].m[1] == 0.0:                          # no absorption: the albedo is 1
        assert abs(MC.oracle(MC.inputs(MC.BY_NAME[name]))["scal"][2] - 1.0) <= 10 * floor["scal"]
        assert abs(float(ref["scal"][2]) - 1.0) <= 1e-17
