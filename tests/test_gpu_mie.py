"""GPU tests of vsm.Scattering (vsm_mie_nai2, csrc/vsm_mie.hip) against tests/mie_oracle.py.

Bounds: those of the reference's own GPU-against-CPU test (test_mie_gpu.jl:326-333) -- rtol 1e-6 on the single-scattering albedo and
on k, atol 1e-6 on each of the six coefficient vectors.  Both sides are FP64; the measured maxima are in DESIGN.md 4.21.
Shapes: monodisperse spheres (nquad = 1: a radius tile with 15 dead columns beside a dead tile) at the reference's D_n stress cases,
among them the two sides of the get_n_max branch and n_max = 542; the reference's test aerosol with n_max = 57, n_mu = 113 (no
multiple of 16 or 4) at nquad below, at and above one tile and one group of 32; every x <= 8; n_max = 381."""
import functools
import math

import numpy as np
import pytest

import mie_oracle as MO
from oracle import vsm_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength (test_mie_gpu.jl)
FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)


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


@functools.lru_cache(maxsize=None)
def _oracle_dist(aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    return MO.compute_aerosol_optical_properties(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad)


@functools.lru_cache(maxsize=None)
def _oracle_mono(x, n_r, n_i):
    return MO.monodisperse(x, n_r, n_i)


def _dist_model(S, aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    return S.make_mie_model(S.Aerosol(S.LogNormal(r_m, sigma_g), n_r, n_i), lam, r_max, nquad)


def _mono_model(S, x, n_r, n_i):
    return S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution([x], [1.0]), n_r, n_i), MO.MONO_WAVELENGTH)


def _greek(opt):
    g = opt.greek_coefs
    return np.stack([g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta])


def _compare(opt, ref, what):
    g = _greek(opt)
    assert g.shape == ref.greek.shape, (g.shape, ref.greek.shape)
    dev = [float(np.max(np.abs(g[i] - ref.greek[i]))) for i in range(6)]
    d_ssa, d_k = abs(opt.ssa - ref.ssa) / ref.ssa, abs(opt.k - ref.k) / ref.k
    print("mie %s: n_max %d  max|d greek| %s  rel d ssa %.2e  rel d k %.2e" % (what, ref.host.n_max, " ".join("%.2e" % v for v in dev),
                                                                            d_ssa, d_k))
    assert np.all(np.isfinite(g)) and math.isfinite(opt.ssa) and math.isfinite(opt.k)
    assert d_ssa <= 1e-6 and d_k <= 1e-6, (d_ssa, d_k)
    for i, name in enumerate(("alpha", "beta", "gamma", "delta", "epsilon", "zeta")):
        assert dev[i] <= 1e-6, (name, dev[i])
    assert opt.f_trunc == 0.0 and opt.C_ext == opt.k and abs(opt.C_sca - ref.C_sca) <= 1e-6 * ref.C_sca
    scale = np.max(np.abs(ref.bulk_f))
    assert np.max(np.abs(opt.bulk_f / opt.C_sca - ref.bulk_f)) <= 1e-6 * scale


MONO = [(0.5, 1.5, 0.0), (8.0, 1.33, 0.0), (8.5, 1.33, 0.0), (100.0, 2.0, 1.0), (200.0, 1.33, 0.0), (500.0, 1.5, 0.1)]


@pytest.mark.parametrize("x,n_r,n_i", MONO)
def test_monodisperse_against_the_oracle(vsm, arch, x, n_r, n_i):
    S = vsm.Scattering
    ref = _oracle_mono(x, n_r, n_i)
    if x == 500.0:
        assert (ref.host.n_max, ref.host.n_mu) == (542, 1083)
    if x in (8.0, 8.5):
        assert ref.host.n_max == {8.0: 17, 8.5: 27}[x]
    opt, = S.compute_aerosol_optical_properties(_mono_model(S, x, n_r, n_i), arch)
    _compare(opt, ref, "x = %g, m = %g - %gi" % (x, n_r, n_i))


DIST = [(TEST_AEROSOL, 3.0, 7), (TEST_AEROSOL, 3.0, 16), (TEST_AEROSOL, 3.0, 37), (TEST_AEROSOL, 3.0, 100),
        (TEST_AEROSOL, 0.5, 16), (TEST_AEROSOL, 30.0, 100), (FINE_MODE, 0.35, 20)]


@pytest.mark.parametrize("aer,r_max,nquad", DIST)
def test_size_distribution_against_the_oracle(vsm, arch, aer, r_max, nquad):
    S = vsm.Scattering
    ref = _oracle_dist(aer, r_max, nquad)
    if aer is TEST_AEROSOL and r_max == 3.0:
        # (the largest node lies below r_max: n_max = 52, 56, 57, 57 for nquad = 7, 16, 37, 100)
        assert (ref.host.n_max, ref.host.n_mu) == ({7: 52, 16: 56}.get(nquad, 57), {7: 103, 16: 111}.get(nquad, 113))
        assert np.count_nonzero(ref.host.nmax_i < ref.host.n_max) >= nquad - 4      # the zero padding above n_max_i
    if r_max == 0.5:
        assert np.all(ref.host.x <= 8.0)
    if r_max == 30.0:
        assert ref.host.n_max > 370
    opt, = S.compute_aerosol_optical_properties(_dist_model(S, aer, r_max, nquad), arch)
    _compare(opt, ref, "r_max = %g, nquad = %d" % (r_max, nquad))
    assert abs(opt.greek_coefs.beta[0] - 1.0) <= 1e-9 and 0.0 < opt.ssa < 1.0


def test_tabulated_distribution_equals_the_lognormal_call_bit_for_bit(vsm, arch):
    S = vsm.Scattering
    r_m, sigma_g, n_r, n_i, lam = TEST_AEROSOL
    ln = S.LogNormal(r_m, sigma_g)
    r, w_r = S.gauleg_log(37, max(ln.quantile(1e-8), 1e-6 * 3.0), 3.0)
    tab = S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution(r, ln.pdf(r) * w_r), n_r, n_i), lam)
    a, = S.compute_aerosol_optical_properties(_dist_model(S, TEST_AEROSOL, 3.0, 37), arch)
    b, = S.compute_aerosol_optical_properties(tab, arch)
    assert np.array_equal(_greek(a), _greek(b)) and (a.ssa, a.k, a.C_sca) == (b.ssa, b.k, b.C_sca)
    assert np.array_equal(a.bulk_f, b.bulk_f)


def test_calls_are_bit_identical(vsm, arch, monkeypatch):
    """Two calls, a call with and one without poisoned work buffers, a list of three models against three single calls."""
    S = vsm.Scattering
    models = [_dist_model(S, TEST_AEROSOL, 3.0, 100), _mono_model(S, 8.5, 1.33, 0.0), _dist_model(S, FINE_MODE, 0.35, 20)]
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    first = [S.compute_aerosol_optical_properties(m, arch)[0] for m in models]
    again = [S.compute_aerosol_optical_properties(m, arch)[0] for m in models]
    monkeypatch.delenv("VSM_POISON_WORK")
    plain = [S.compute_aerosol_optical_properties(m, arch)[0] for m in models]
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    listed = S.compute_aerosol_optical_properties(models, arch)
    assert len(listed) == 3
    for other in (again, plain, listed):
        for a, b in zip(first, other):
            assert np.all(np.isfinite(_greek(a)))
            assert np.array_equal(_greek(a), _greek(b)) and np.array_equal(a.bulk_f, b.bulk_f)
            assert (a.ssa, a.k, a.C_sca) == (b.ssa, b.k, b.C_sca)


def test_fine_mode_aerosol_end_to_end_through_rt_run(vsm, arch):
    """LogNormal(0.08, 1.6), 1.45 - 0.005i at 0.76 um, r_max = 0.35: x_max = 2.9, n_max = 10, 19 coefficients.  rt_run (IQU,
    l_trunc = 20, two layers, 8 points) on the device's Mie optics against the oracle's rt_run on the oracle's Mie optics, at the
    tolerance tests/test_gpu_parity.py uses for its aerosol scenes (relative 1e-8)."""
    S, H = vsm.Scattering, vsm.host_model
    ref = _oracle_dist(FINE_MODE, 0.35, 20)
    assert (ref.host.n_max, ref.host.n_mu) == (10, 19) and 2.8 < np.max(ref.host.x) < 3.0
    opt, = S.compute_aerosol_optical_properties(_dist_model(S, FINE_MODE, 0.35, 20), arch)
    assert isinstance(opt, H.AerosolOptics) and len(opt.greek_coefs.beta) == 19
    rng = np.random.default_rng(11)
    Sp, L = 8, 2
    tau_rayl = np.tile(0.02 * np.ones(L), (Sp, 1))
    tau_abs = 10.0 ** rng.uniform(-3, 0, (Sp, L))
    tau_aer = np.array([[0.05, 0.2]])
    geo = ("IQU", 20, 40.0, [30.0, 0.0], [0.0, 75.0])
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, tau_aer=tau_aer, depol=0.03, albedo=0.1, m_max=4)
    pm = H.model_from_arrays(arch, *geo, aerosol_optics=[opt], **kw)
    om = O.build_model(*geo, aerosols=[O.AerosolOptics(O.GreekCoefs(*ref.greek), ref.ssa, 0.0)], **kw)
    Ro, To = O.rt_run(om)
    Rg, Tg = vsm.CoreRT.rt_run(pm)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    print("mie end to end: rel d R %.2e  rel d T %.2e" % (rel(Rg, Ro), rel(Tg, To)))
    assert rel(Rg, Ro) < 1e-8 and rel(Tg, To) < 1e-8


def test_refusals(vsm, arch):
    S = vsm.Scattering
    ln = S.LogNormal(0.3, 2.1)
    run = lambda m, a=arch: S.compute_aerosol_optical_properties(m, a)
    with pytest.raises(vsm.VSMError):                       # n_i < 0
        run(S.make_mie_model(S.Aerosol(ln, 1.3, -0.001), 0.55, 3.0, 37))
    with pytest.raises(vsm.VSMError):                       # r_max <= r_min
        run(S.make_mie_model(S.Aerosol(ln, 1.3, 0.0), 0.55, 4.0e-3, 37))
    with pytest.raises(vsm.VSMError):                       # nquad_radius < 1
        run(S.make_mie_model(S.Aerosol(ln, 1.3, 0.0), 0.55, 3.0, 0))
    with pytest.raises(vsm.VSMError):                       # n_max above the cap
        run(_mono_model(S, 1100.0, 1.3, 0.0))
    with pytest.raises(vsm.VSMError):                       # a CPU architecture
        run(S.make_mie_model(S.Aerosol(ln, 1.3, 0.0), 0.55, 3.0, 37), vsm.Architectures.CPU())
    lib = vsm._lib.lib()                                    # the library refuses what the host layer would
    assert lib.vsm_mie_nai2(1, S.MAX_N_MAX + 1, 2 * S.MAX_N_MAX + 1, 1.3, 0.0, 1.0, *([None] * 11)) == 2    # VSM_ERR_UNSUPPORTED
    assert lib.vsm_mie_nai2(1, 4, 7, 1.3, -0.1, 1.0, *([None] * 11)) == 1                                   # VSM_ERR_INVALID_ARG
