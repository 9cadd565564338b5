"""GPU tests of Scattering.truncate_phase / truncate_phase_lowconf (vsm_truncate_dbge, csrc/vsm_truncate.hip) against
tests/truncation_oracle.py.

Bounds: those tests/test_gpu_mie.py takes from the reference's GPU-against-CPU test -- atol 1e-6 on each coefficient vector, rtol 1e-6
on c0.  For scale: the reference's formulas move by at most 3.3e-9 on these optics when f comes from bulk_f instead of the
reconstruction or carries 1e-13 of relative noise; the normal equations reach a condition number of 7.6e8 at l_max = 112.  The
measured maxima are in DESIGN.md 4.22.
Shapes: the reference's test aerosol with n_mu = 113 (no multiple of 4, 16 or 64; one angle chunk) and a coarse mode with
n_mu = 307 (three angle chunks, the last one partly filled); l_max = 3 (a gamma system of one unknown), 17 and 20 (18 and 21 rows
of [A | b]: one tile pair more), 64 and 112 (the cap region: five and eight tiles of 16 rows)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import mie_oracle as MO
import truncation_oracle as TO
from oracle import vsm_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength (test_mie_gpu.jl)
COARSE_MODE = (1.0, 1.8, 1.53, 0.008, 0.76)
FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)
SETS = {"test": (TEST_AEROSOL, 3.0, 37, 113), "coarse": (COARSE_MODE, 15.0, 200, 307)}
NAMES = ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")


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
def _oracle_mie(aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    o = MO.compute_aerosol_optical_properties(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad)
    o.greek.flags.writeable = False
    return o


@functools.lru_cache(maxsize=None)
def _oracle_set(name):
    aer, r_max, nquad, n_mu = SETS[name]
    o = _oracle_mie(aer, r_max, nquad)
    assert o.host.n_mu == n_mu
    return o


@functools.lru_cache(maxsize=None)
def _oracle_fit(name, l_max):
    return TO.truncate_phase(_oracle_set(name).greek, l_max)


@functools.lru_cache(maxsize=None)
def _oracle_fit_lowconf(name, l_max, delta):
    return TO.truncate_phase_lowconf(_oracle_set(name).greek, l_max, delta)


def _model(S, name):
    (r_m, sigma_g, n_r, n_i, lam), r_max, nquad, _ = SETS[name]
    return S.make_mie_model(S.Aerosol(S.LogNormal(r_m, sigma_g), n_r, n_i), lam, r_max, nquad)


_device_mie = {}


def _device_set(vsm, arch, name):
    """The device's own Mie optics of a set (MieAerosolOptics with bulk_f), computed once per module."""
    if name not in _device_mie:
        _device_mie[name], = vsm.Scattering.compute_aerosol_optical_properties(_model(vsm.Scattering, name), arch)
    return _device_mie[name]


def _plain(vsm, greek, ssa=0.9):
    """A hand-made AerosolOptics: no bulk_f, so the device reconstructs f11, f12, f34 from the coefficients."""
    H = vsm.host_model
    return H.AerosolOptics(H.GreekCoefs(*(np.array(greek[i], dtype=np.float64) for i in range(6))), ssa, 0.0)


def _greek(opt):
    g = opt.greek_coefs
    return np.stack([g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta])


def _compare(opt, want, what, atol=1e-6, rtol=1e-6):
    g_ref, c0_ref, ft_ref = want
    g = _greek(opt)
    assert g.shape == g_ref.shape, (g.shape, g_ref.shape)
    dev = [float(np.max(np.abs(g[i] - g_ref[i]))) for i in range(6)]
    d_c0 = abs(opt.c0 - c0_ref) / abs(c0_ref)
    print("dbge %s: max|d greek| %s  rel d c0 %.2e  d f_trunc %.2e" % (what, " ".join("%.2e" % v for v in dev), d_c0,
                                                                      abs(opt.f_trunc - ft_ref)))
    assert np.all(np.isfinite(g)) and math.isfinite(opt.c0)
    for i, name in enumerate(NAMES):
        assert dev[i] <= atol, (name, dev[i])
    assert d_c0 <= rtol, d_c0
    assert abs(opt.f_trunc - ft_ref) <= atol and opt.f_trunc == 1.0 - opt.c0


# ---- 1. device against oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["reconstruct", "bulk_f"])
@pytest.mark.parametrize("l_max", [3, 17, 20, 64, 112])
@pytest.mark.parametrize("name", ["test", "coarse"])
def test_truncate_phase_against_the_oracle(vsm, arch, name, l_max, path):
    """reconstruct: the oracle's coefficients go in, the device rebuilds f from all n_mu of them.  bulk_f: the device's own Mie
    optics go in with their bulk_f and C_sca, as the truncation= keyword hands them over."""
    S = vsm.Scattering
    ref = _oracle_set(name)
    src = _plain(vsm, ref.greek, ref.ssa) if path == "reconstruct" else _device_set(vsm, arch, name)
    assert (getattr(src, "bulk_f", None) is not None) == (path == "bulk_f")
    opt = S.truncate_phase(S.DeltaBGE(l_max), src, arch)
    assert isinstance(opt, S.TruncatedAerosolOptics) and isinstance(opt, vsm.host_model.AerosolOptics)
    assert opt.untruncated is src and opt.method == S.DeltaBGE(l_max) and opt.ssa == src.ssa and opt.info == (0, 0, 0)
    if path == "bulk_f":
        assert (opt.k, opt.C_ext, opt.C_sca) == (src.k, src.C_ext, src.C_sca)
    _compare(opt, _oracle_fit(name, l_max), "%s n_mu %d l_max %d %s" % (name, ref.host.n_mu, l_max, path))
    assert abs(opt.greek_coefs.beta[0] - 1.0) <= 1e-15 and np.all(opt.greek_coefs.gamma[:2] == 0)


# ---- 2. the low-confidence variant -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [2.0, 5.0])
def test_truncate_phase_lowconf_against_the_oracle(vsm, arch, delta):
    S = vsm.Scattering
    ref = _oracle_set("test")
    opt = S.truncate_phase_lowconf(S.DeltaBGE(20, delta), _plain(vsm, ref.greek, ref.ssa), arch)
    _compare(opt, _oracle_fit_lowconf("test", 20, delta), "lowconf %g deg l_max 20" % delta)
    other = _oracle_fit_lowconf("test", 20, 7.0 - delta)
    assert abs(opt.c0 - other[1]) > 1e-4                    # (the cone is read: the two angles give different fits)


def test_scalar_phase_function_keeps_its_zero_series(vsm, arch):
    """Henyey-Greenstein g = 0.7 with 200 terms: gamma and epsilon are series of exact zeros, their systems are skipped."""
    S, H = vsm.Scattering, vsm.host_model
    hg = H.AerosolOptics(H.henyey_greenstein_greek(0.7, 199), 0.95)
    assert len(hg.greek_coefs.beta) == 200
    want = TO.truncate_phase_lowconf(_greek(hg), 20, 2.0)
    for fit, ref in ((S.truncate_phase_lowconf, want), (S.truncate_phase, TO.truncate_phase(_greek(hg), 20))):
        opt = fit(S.DeltaBGE(20, 2.0), hg, arch)
        assert opt.info == (0, 1, 1)
        assert not np.any(opt.greek_coefs.gamma) and not np.any(opt.greek_coefs.epsilon)
        _compare(opt, ref, "HG 0.7 %s" % fit.__name__)


# ---- 3. exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_max", [19, 24])
def test_a_series_below_l_max_is_returned_unchanged(vsm, arch, l_max):
    S = vsm.Scattering
    fine = _oracle_mie(FINE_MODE, 0.35, 20)
    assert fine.greek.shape == (6, 19)
    padded = np.concatenate([fine.greek, np.zeros((6, 21))], axis=1)
    opt = S.truncate_phase(S.DeltaBGE(l_max), _plain(vsm, padded, fine.ssa), arch)
    g = _greek(opt)
    print("dbge exactness l_max %d: max|d greek| %.2e  |c0 - 1| %.2e" % (l_max, np.max(np.abs(g - padded[:, :l_max])), abs(opt.c0 - 1)))
    assert g.shape == (6, l_max) and abs(opt.c0 - 1.0) <= 1e-10 and abs(opt.f_trunc) <= 1e-10
    for i, name in enumerate(NAMES):
        assert np.max(np.abs(g[i] - padded[i, :l_max])) <= 1e-10, name


# ---- 4. determinism and the keyword ------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(_greek(a), _greek(b)) and (a.c0, a.f_trunc, a.ssa, a.info) == (b.c0, b.f_trunc, b.ssa, b.info)


def test_calls_are_bit_identical(vsm, arch, monkeypatch):
    S = vsm.Scattering
    sets = [_device_set(vsm, arch, "coarse"), _plain(vsm, _oracle_set("coarse").greek), _plain(vsm, _oracle_set("test").greek)]
    method = S.DeltaBGE(64)
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    first = [S.truncate_phase(method, s, arch) for s in sets]
    again = [S.truncate_phase(method, s, arch) for s in sets]
    monkeypatch.delenv("VSM_POISON_WORK")
    plain = [S.truncate_phase(method, s, arch) for s in sets]
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    listed = S.truncate_phase(method, sets, arch)
    assert isinstance(listed, list) and len(listed) == 3
    for other in (again, plain, listed):
        for a, b in zip(first, other):
            assert np.all(np.isfinite(_greek(a))) and _same(a, b)


def test_truncation_keyword(vsm, arch):
    S = vsm.Scattering
    models = [_model(S, "test"), _model(S, "coarse")]
    today = S.compute_aerosol_optical_properties(models, arch)
    none = S.compute_aerosol_optical_properties(models, arch, truncation=None)
    for a, b in zip(today, none):
        assert type(b) is S.MieAerosolOptics and b.f_trunc == 0.0
        assert np.array_equal(_greek(a), _greek(b)) and np.array_equal(a.bulk_f, b.bulk_f)
        assert (a.ssa, a.k, a.C_ext, a.C_sca) == (b.ssa, b.k, b.C_ext, b.C_sca)
    method = S.DeltaBGE(20)
    fitted = S.compute_aerosol_optical_properties(models, arch, truncation=method)
    assert len(fitted) == 2
    for a, t in zip(today, fitted):
        assert isinstance(t, S.TruncatedAerosolOptics) and isinstance(t.untruncated, S.MieAerosolOptics)
        assert np.array_equal(_greek(t.untruncated), _greek(a)) and len(t.greek_coefs.beta) == 20
        assert (t.k, t.C_ext, t.C_sca, t.ssa) == (a.k, a.C_ext, a.C_sca, a.ssa) and 0.0 < t.f_trunc < 1.0
        assert _same(t, S.truncate_phase(method, t.untruncated, arch))
    kept, = S.compute_aerosol_optical_properties(models[:1], arch, truncation=S.DeltaBGE(113))     # n_mu <= l_max: nothing to cut
    assert kept.method == S.NoTruncation() and kept.f_trunc == 0.0 and kept.greek_coefs is kept.untruncated.greek_coefs
    wrapped, = S.compute_aerosol_optical_properties(models[:1], arch, truncation=S.NoTruncation())
    assert wrapped.f_trunc == 0.0 and np.array_equal(_greek(wrapped), _greek(today[0]))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
def test_truncated_coarse_aerosol_end_to_end_through_rt_run(vsm, arch):
    """The test aerosol (113 coefficients) truncated on the device to l_max = 20 behind its Mie call, through rt_run (IQU,
    l_trunc = 20, two layers, 8 points: the scene of test_fine_mode_aerosol_end_to_end_through_rt_run) against the oracle's rt_run on
    the oracle's truncated optics, at that test's relative 1e-8."""
    S, H = vsm.Scattering, vsm.host_model
    ref = _oracle_set("test")
    g_ref, c0_ref, ft_ref = _oracle_fit("test", 20)
    opt, = S.compute_aerosol_optical_properties(_model(S, "test"), arch, truncation=S.DeltaBGE(20))
    assert len(opt.greek_coefs.beta) == 20 and 0.1 < opt.f_trunc < 0.2
    rng = np.random.default_rng(11)
    Sp, L = 8, 2
    tau_rayl = np.tile(0.02 * np.ones(L), (Sp, 1))
    tau_abs = 10.0 ** rng.uniform(-3, 0, (Sp, L))
    tau_aer = np.array([[0.05, 0.2]])
    geo = ("IQU", 20, 40.0, [30.0, 0.0], [0.0, 75.0])
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, tau_aer=tau_aer, depol=0.03, albedo=0.1, m_max=4)
    pm = H.model_from_arrays(arch, *geo, aerosol_optics=[opt], **kw)
    om = O.build_model(*geo, aerosols=[O.AerosolOptics(O.GreekCoefs(*g_ref), ref.ssa, ft_ref)], **kw)
    Ro, To = O.rt_run(om)
    Rg, Tg = vsm.CoreRT.rt_run(pm)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    print("dbge end to end: f_trunc %.6f  rel d R %.2e  rel d T %.2e" % (opt.f_trunc, rel(Rg, Ro), rel(Tg, To)))
    assert rel(Rg, Ro) < 1e-8 and rel(Tg, To) < 1e-8


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(vsm, arch):
    S, H = vsm.Scattering, vsm.host_model
    lib = vsm._lib.lib()
    none = [None] * 10
    assert lib.vsm_truncate_dbge(200, 129, 0, 1.0, *none) == 2          # VSM_ERR_UNSUPPORTED
    assert lib.vsm_truncate_dbge(200, 2, 0, 1.0, *none) == 1            # VSM_ERR_INVALID_ARG
    assert lib.vsm_truncate_dbge(20, 20, 0, 1.0, *none) == 1            # n_mu <= l_max
    assert lib.vsm_truncate_dbge(200, 20, 19, 0.5, *none) == 1          # fewer nodes outside the cone than unknowns
    buf = torch.zeros(6 * 200, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.vsm_truncate_dbge(200, 20, 0, 1.0, p, p, None, p, p, p, p, p, p, None) == 1       # a lone bulk_f
    assert lib.vsm_truncate_dbge(200, 20, 0, 1.0, p, None, p, p, p, p, p, p, p, None) == 1       # a lone scal
    assert lib.vsm_truncate_dbge(200, 20, 0, 1.0, p, None, None, p, p, p, p, None, p, None) == 1     # a null required pointer
    assert lib.vsm_dbge_work_elems(200, 129) == 0 and lib.vsm_dbge_work_elems(20, 20) == 0 and lib.vsm_dbge_work_elems(200, 20) > 0
    hg = H.AerosolOptics(H.henyey_greenstein_greek(0.7, 199), 1.0)
    for bad in (S.DeltaBGE(129), S.DeltaBGE(2)):
        with pytest.raises(vsm.VSMError):
            S.truncate_phase(bad, hg, arch)
    with pytest.raises(vsm.VSMError):                                   # a cone that leaves fewer than l_max nodes
        S.truncate_phase_lowconf(S.DeltaBGE(20, 170.0), hg, arch)
    with pytest.raises(vsm.VSMError):                                   # a CPU architecture
        S.truncate_phase(S.DeltaBGE(20), hg, vsm.Architectures.CPU())
    short = H.AerosolOptics(H.henyey_greenstein_greek(0.7, 19), 1.0)    # len(beta) = 20 <= l_max: the NoTruncation result
    for method in (S.DeltaBGE(20), S.DeltaBGE(64), S.NoTruncation()):
        kept = S.truncate_phase(method, short, arch)
        assert kept.greek_coefs is short.greek_coefs and kept.greek_coefs.beta is short.greek_coefs.beta
        assert kept.f_trunc == 0.0 and kept.c0 == 1.0 and kept.method == S.NoTruncation() and kept.untruncated is short


def test_a_phase_function_through_zero_is_a_status_not_a_fault(vsm, arch):
    """beta = (1, 3, 0, ...): f11 = 1 + 3 mu changes sign inside the node range, the weights w / f11^2 mean nothing there.  The beta
    system reports info = 2, the host raises, and the device goes on working."""
    S = vsm.Scattering
    greek = np.zeros((6, 40))
    greek[1, :2] = (1.0, 3.0)
    with pytest.raises(vsm.VSMError, match="beta"):
        S.truncate_phase(S.DeltaBGE(20), _plain(vsm, greek), arch)
    ref = _oracle_set("test")
    opt = S.truncate_phase(S.DeltaBGE(20), _plain(vsm, ref.greek, ref.ssa), arch)
    _compare(opt, _oracle_fit("test", 20), "after the refused set")
