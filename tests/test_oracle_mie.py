"""CPU tests of tests/mie_oracle.py (the numpy restatement of the reference's NAI-2 Mie path) against numbers that are not ours:
published single-sphere efficiencies, the Rayleigh limit, the identities a Greek expansion satisfies -- and of the host part of
vsm.Scattering against the oracle's, bit for bit.  No kernel runs here."""
import math
import os
import re

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
