"""GPU tests of Scattering.truncate_phase_lin / compute_truncated_aerosol_optical_properties_lin (vsm_truncate_dbge_lin,
csrc/vsm_truncate.hip) against tests/truncation_lin_oracle.py, whose literal form is the reference's text and is itself checked
against central differences in tests/test_oracle_truncation_lin.py.

Bounds: those of tests/test_gpu_mie_lin.py -- per slot and coefficient family |dev - ref| <= tol max(1, max |ref|), on f_trunc_dot
tol max(1, |ref|), tol = 1e-6 -- except where the reference's own formula does not hold a fixed number: per system the oracle's
literal and fused forms (algebraically equal) are evaluated and their disagreement d widens that system's rows to
tol = max(1e-6, 10 d); beta's d governs alpha, beta, delta, zeta and f_trunc_dot.  Only the epsilon system of the coarse set needs
it (f34 changes sign, the weights 1 / f34^3 blow up, the condition number reaches 7.6e8).  The factor 10: the device sums in a
third order (angle chunks, MFMA lane groups).  The measured maxima are in DESIGN.md 4.24.
Shapes: those tests/test_gpu_truncation.py pins the forward fit at -- n_mu = 113 (one partly filled angle chunk) and 307 (three);
l_max = 3 (a gamma system of one unknown), 17 and 20 (a partly filled tile of 16 rows, one and two tiles), 64 and 112 (65 rows; the
largest triangle the sets allow)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import mie_lin_oracle as ML
import mie_oracle as MO
import truncation_lin_oracle as TL
import truncation_oracle as TO
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength
COARSE_MODE = (1.0, 1.8, 1.53, 0.008, 0.76)
FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)
SETS = {"test": (TEST_AEROSOL, 3.0, 37, 113), "coarse": (COARSE_MODE, 15.0, 200, 307)}
NAMES = ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")
SYSTEM_OF = (0, 0, 1, 0, 2, 0)                   # the system (beta, gamma, epsilon) whose solution a family comes from


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
def _oracle_mie_lin(aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    o = ML.compute_aerosol_optical_properties_lin(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad)
    o.greek.flags.writeable = False
    o.greek_dot.flags.writeable = False
    return o


def _oracle_set(name):
    aer, r_max, nquad, n_mu = SETS[name]
    o = _oracle_mie_lin(aer, r_max, nquad)
    assert o.host.n_mu == n_mu
    return o


@functools.lru_cache(maxsize=None)
def _oracle_fit(name, l_max):
    """The literal form's (greek_t, c0, f_trunc, greek_t_dot, c0_dot, f_trunc_dot) and the two forms' disagreement d [3]."""
    o = _oracle_set(name)
    return TL.truncate_phase_lin(o.greek, o.greek_dot, l_max), TL.form_disagreement(o.greek, o.greek_dot, l_max)


def _model(S, name):
    (r_m, sigma_g, n_r, n_i, lam), r_max, nquad, _ = SETS[name]
    return S.make_mie_model(S.Aerosol(S.LogNormal(r_m, sigma_g), n_r, n_i), lam, r_max, nquad)


_device_mie = {}


def _device_pair(vsm, arch, name):
    """The device's own linearized Mie optics of a set (with bulk_f, bulk_f_dot), computed once per module."""
    if name not in _device_mie:
        _device_mie[name], = vsm.Scattering.compute_aerosol_optical_properties_lin(_model(vsm.Scattering, name), arch)
    return _device_mie[name]


def _coefs(vsm, g):
    return vsm.host_model.GreekCoefs(*(np.array(g[i], dtype=np.float64) for i in range(6)))


def _plain_pair(vsm, greek, greek_dot, ssa=0.9, ssa_dot=None):
    """A hand-made (AerosolOptics, LinAerosolOptics): no bulk_f, so the device reconstructs f and f' from the coefficients."""
    H = vsm.host_model
    lin = H.LinAerosolOptics([_coefs(vsm, greek_dot[s]) for s in range(4)], np.zeros(4) if ssa_dot is None else np.array(ssa_dot),
                             np.zeros(4))
    return H.AerosolOptics(_coefs(vsm, greek), ssa, 0.0), lin


def _stack(g):
    return np.stack([g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta])


def _greek(opt):
    return _stack(opt.greek_coefs)


def _greek_dot(lin):
    return np.stack([_stack(g) for g in lin.lin_greek_coefs])


def _same_forward(a, b):
    assert np.array_equal(_greek(a), _greek(b)), "greek_t"
    assert (a.c0, a.f_trunc, a.ssa, a.info, a.k, a.C_ext, a.C_sca) == (b.c0, b.f_trunc, b.ssa, b.info, b.k, b.C_ext, b.C_sca)


def _same_lin(a, b):
    assert np.array_equal(_greek_dot(a), _greek_dot(b)), "greek_t_dot"
    for n in ("ssa_dot", "f_trunc_dot", "c0_dot"):
        assert np.array_equal(getattr(a, n), getattr(b, n)), n


def _compare_lin(lin, want, d, what, tol0=1e-6):
    """Test 1's bound: tol = max(tol0, 10 d) per system."""
    gtd_ref, c0_dot_ref, ft_dot_ref = want
    gtd = _greek_dot(lin)
    assert gtd.shape == gtd_ref.shape, (gtd.shape, gtd_ref.shape)
    assert np.all(np.isfinite(gtd)) and np.all(np.isfinite(lin.f_trunc_dot))
    tol = np.maximum(tol0, 10.0 * np.asarray(d))
    worst = np.zeros(3)
    for s in range(4):
        for c, name in enumerate(NAMES):
            k = SYSTEM_OF[c]
            dev = float(np.max(np.abs(gtd[s, c] - gtd_ref[s, c]))) / max(1.0, float(np.max(np.abs(gtd_ref[s, c]))))
            worst[k] = max(worst[k], dev)
        dev = abs(lin.f_trunc_dot[s] - ft_dot_ref[s]) / max(1.0, abs(ft_dot_ref[s]))
        worst[0] = max(worst[0], dev)
    print("dbge lin %s: worst beta-system %.2e gamma %.2e epsilon %.2e   d %s   tol %s"
          % (what, worst[0], worst[1], worst[2], " ".join("%.2e" % v for v in d), " ".join("%.2e" % v for v in tol)))
    for s in range(4):
        for c, name in enumerate(NAMES):
            k = SYSTEM_OF[c]
            dev = float(np.max(np.abs(gtd[s, c] - gtd_ref[s, c]))) / max(1.0, float(np.max(np.abs(gtd_ref[s, c]))))
            assert dev <= tol[k], (what, ML.SLOTS[s], name, dev, tol[k])
        assert abs(lin.f_trunc_dot[s] - ft_dot_ref[s]) <= tol[0] * max(1.0, abs(ft_dot_ref[s])), (what, ML.SLOTS[s])
        assert abs(lin.c0_dot[s] - c0_dot_ref[s]) <= tol[0] * max(1.0, abs(c0_dot_ref[s])), (what, ML.SLOTS[s])
    assert np.array_equal(lin.f_trunc_dot, -lin.c0_dot)
    assert np.all(gtd[:, 2, :2] == 0) and np.all(gtd[:, 4, :2] == 0)


# ---- 1. device against the literal oracle; 2. the forward half ---------------------------------------------------------------
@pytest.mark.parametrize("path", ["reconstruct", "bulk_f_dot"])
@pytest.mark.parametrize("l_max", [3, 17, 20, 64, 112])
@pytest.mark.parametrize("name", ["test", "coarse"])
def test_truncate_phase_lin_against_the_oracle(vsm, arch, name, l_max, path):
    """reconstruct: the oracle's greek and greek_dot go in, the device rebuilds f and f' from all n_mu of them.  bulk_f_dot: the
    device's own linearized Mie optics go in with bulk_f, bulk_f_dot, C_sca and C_sca_dot."""
    S, H = vsm.Scattering, vsm.host_model
    ref = _oracle_set(name)
    if path == "reconstruct":
        src, lin_src = _plain_pair(vsm, ref.greek, ref.greek_dot, ref.ssa, ref.ssa_dot)
    else:
        src, lin_src = _device_pair(vsm, arch, name)
    assert (getattr(lin_src, "bulk_f_dot", None) is not None) == (path == "bulk_f_dot")
    method = S.DeltaBGE(l_max)
    opt, lin = S.truncate_phase_lin(method, src, lin_src, arch)
    assert isinstance(opt, S.TruncatedAerosolOptics) and isinstance(lin, S.TruncatedLinAerosolOptics)
    assert isinstance(lin, H.LinAerosolOptics) and lin.untruncated is lin_src and opt.untruncated is src and lin.method == method
    assert lin.ssa_dot is lin_src.ssa_dot and opt.info == (0, 0, 0)
    if path == "bulk_f_dot":
        assert lin.k_dot is lin_src.k_dot and lin.C_ext_dot is lin_src.C_ext_dot and lin.C_sca_dot is lin_src.C_sca_dot
    _same_forward(opt, S.truncate_phase(method, src, arch))
    fit, d = _oracle_fit(name, l_max)
    _compare_lin(lin, fit[3:], d, "%s n_mu %d l_max %d %s" % (name, ref.host.n_mu, l_max, path))
    for k, system in enumerate(TL.SYSTEMS):                 # (only the coarse set's epsilon system may widen its bound)
        assert (name, system) == ("coarse", "epsilon") or 10.0 * d[k] <= 1e-6, (system, d[k])


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------
def test_calls_are_bit_identical(vsm, arch, monkeypatch):
    """Two calls, poisoned against plain work buffers, a list of three pairs against three single calls."""
    S = vsm.Scattering
    coarse, test = _oracle_set("coarse"), _oracle_set("test")
    pairs = [_device_pair(vsm, arch, "coarse"), _plain_pair(vsm, coarse.greek, coarse.greek_dot),
             _plain_pair(vsm, test.greek, test.greek_dot)]
    method = S.DeltaBGE(64)
    one = lambda p: S.truncate_phase_lin(method, p[0], p[1], arch)
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    first = [one(p) for p in pairs]
    again = [one(p) for p in pairs]
    monkeypatch.delenv("VSM_POISON_WORK")
    plain = [one(p) for p in pairs]
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    listed = S.truncate_phase_lin(method, [p[0] for p in pairs], [p[1] for p in pairs], arch)
    assert isinstance(listed, list) and len(listed) == 3
    for other in (again, plain, listed):
        for (a, la), (b, lb) in zip(first, other):
            assert np.all(np.isfinite(_greek(a))) and np.all(np.isfinite(_greek_dot(la))) and np.all(np.isfinite(la.f_trunc_dot))
            _same_forward(a, b)
            _same_lin(la, lb)


def test_one_pass_call_equals_the_two_calls(vsm, arch):
    """compute_truncated_aerosol_optical_properties_lin against truncate_phase_lin on compute_aerosol_optical_properties_lin's
    pairs, bit for bit; NoTruncation() and n_mu <= l_max hand the very same arrays back."""
    S = vsm.Scattering
    models = [_model(S, "test"), _model(S, "coarse")]
    method = S.DeltaBGE(20)
    pairs = S.compute_aerosol_optical_properties_lin(models, arch)
    fused = S.compute_truncated_aerosol_optical_properties_lin(models, method, arch)
    split = S.truncate_phase_lin(method, [p[0] for p in pairs], [p[1] for p in pairs], arch)
    assert len(fused) == 2 and len(split) == 2
    for (a, la), (b, lb), (u, lu) in zip(fused, split, pairs):
        assert len(a.greek_coefs.beta) == 20 and 0.0 < a.f_trunc < 1.0 and np.any(la.f_trunc_dot)
        _same_forward(a, b)
        _same_lin(la, lb)
        assert isinstance(a.untruncated, S.MieAerosolOptics) and isinstance(la.untruncated, S.MieLinAerosolOptics)
        assert np.array_equal(_greek(a.untruncated), _greek(u)) and np.array_equal(_greek_dot(la.untruncated), _greek_dot(lu))
        assert np.array_equal(la.untruncated.bulk_f_dot, lu.bulk_f_dot) and np.array_equal(la.k_dot, lu.k_dot)
        _same_forward(a, S.compute_aerosol_optical_properties(models[:1] if u is pairs[0][0] else models[1:], arch,
                                                              truncation=method)[0])
    for kept_method in (S.DeltaBGE(113), S.NoTruncation()):
        (kept, lkept), = S.compute_truncated_aerosol_optical_properties_lin(models[:1], kept_method, arch)
        assert kept.method == S.NoTruncation() and kept.f_trunc == 0.0 and kept.greek_coefs is kept.untruncated.greek_coefs
        assert lkept.method == S.NoTruncation() and lkept.lin_greek_coefs is lkept.untruncated.lin_greek_coefs
        assert np.array_equal(lkept.f_trunc_dot, np.zeros(4)) and lkept.ssa_dot is lkept.untruncated.ssa_dot
    src, lin_src = pairs[0]
    kept, lkept = S.truncate_phase_lin(S.DeltaBGE(113), src, lin_src, arch)
    assert kept.greek_coefs is src.greek_coefs and lkept.lin_greek_coefs is lin_src.lin_greek_coefs
    assert kept.f_trunc == 0.0 and np.array_equal(lkept.f_trunc_dot, np.zeros(4)) and lkept.untruncated is lin_src


# ---- 4. a scalar phase function ------------------------------------------------------------------------------------------
def test_scalar_phase_function_keeps_exact_zero_derivatives(vsm, arch):
    """Henyey-Greenstein g = 0.7 with 200 terms and d beta / d g in slot 0, a multiple of it in slot 2: the gamma and epsilon
    systems are skipped, their derivative rows are exact zeros."""
    S = vsm.Scattering
    greek = TO.henyey_greenstein_greek(0.7, 200)
    l = np.arange(200)
    greek_dot = np.zeros((4, 6, 200))
    greek_dot[0, 1] = l * (2 * l + 1) * 0.7 ** np.maximum(l - 1, 0)
    greek_dot[2, 1] = -0.25 * greek_dot[0, 1]
    opt, lin = S.truncate_phase_lin(S.DeltaBGE(20, 2.0), *_plain_pair(vsm, greek, greek_dot, 0.95), arch)
    assert opt.info == (0, 1, 1)
    gtd = _greek_dot(lin)
    assert not np.any(gtd[:, 2]) and not np.any(gtd[:, 4]) and not np.any(opt.greek_coefs.gamma)
    want = TL.truncate_phase_lin(greek, greek_dot, 20)
    _compare_lin(lin, want[3:], TL.form_disagreement(greek, greek_dot, 20), "HG 0.7")
    assert np.any(gtd[0, 1]) and not np.any(gtd[1]) and not np.any(gtd[3]) and lin.f_trunc_dot[1] == 0.0


# ---- 5. fixed point ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_max", [19, 24])
def test_a_series_below_l_max_keeps_its_derivatives(vsm, arch, l_max):
    S = vsm.Scattering
    fine = _oracle_mie_lin(FINE_MODE, 0.35, 20)
    assert fine.greek.shape == (6, 19)
    greek = np.concatenate([fine.greek, np.zeros((6, 21))], axis=1)
    greek_dot = np.concatenate([fine.greek_dot, np.zeros((4, 6, 21))], axis=2)
    opt, lin = S.truncate_phase_lin(S.DeltaBGE(l_max), *_plain_pair(vsm, greek, greek_dot, fine.ssa, fine.ssa_dot), arch)
    gtd = _greek_dot(lin)
    err = float(np.max(np.abs(gtd - greek_dot[:, :, :l_max])))
    print("dbge lin fixed point l_max %d: max|d greek'| %.2e  max|f_trunc'| %.2e" % (l_max, err, np.max(np.abs(lin.f_trunc_dot))))
    assert gtd.shape == (4, 6, l_max) and err <= 1e-9 and np.max(np.abs(lin.f_trunc_dot)) <= 1e-10


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
def _tabulated(S, aer, r_max, nquad, d_mu=0.0, d_sigma=0.0, n_r=None, n_i=None):
    """The LogNormal's own nodes with the weights of LogNormal(mu + d_mu, sigma + d_sigma) on them."""
    r_m, sigma_g, nr0, ni0, lam = aer
    base = S.LogNormal(r_m, sigma_g)
    r, w_r = S.gauleg_log(nquad, max(base.quantile(1e-8), 1e-6 * r_max), r_max)
    ln = base if d_mu == 0.0 and d_sigma == 0.0 else S.LogNormal(math.exp(base.mu + d_mu), math.exp(base.sigma + d_sigma))
    tab = S.TabulatedSizeDistribution(r, ln.pdf(r) * w_r)
    return S.make_mie_model(S.Aerosol(tab, nr0 if n_r is None else n_r, ni0 if n_i is None else n_i), lam)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_truncated_jacobians_end_to_end_through_rt_run_lin(vsm, arch):
    """The test aerosol (113 coefficients) truncated to l_max = 20 behind its linearized Mie call, the device's pair handed to
    model_from_arrays / LinModel as it is, in the scene of tests/test_gpu_mie_lin.py's end-to-end test: rt_run_lin(pm, pl, 1, 1, 1)
    against the oracle's on the oracle's truncated lin optics (1e-9 on R, T, 1e-8 per slot), and slots 1-4 against central
    differences (h = 1e-5) of the device's own forward Mie call with truncation = DeltaBGE(20) plus rt_run, the radius nodes held
    fixed through the tabulated form (err.max() < 1e-3, err.mean() < 1e-4)."""
    S, H = vsm.Scattering, vsm.host_model
    aer, r_max, nquad, _ = SETS["test"]
    ref = _oracle_set("test")
    method = S.DeltaBGE(20)
    (g_t, c0, f_t, gtd, c0_dot, ft_dot), _ = _oracle_fit("test", 20)
    (opt, lin), = S.compute_truncated_aerosol_optical_properties_lin(_model(S, "test"), method, arch)
    assert len(opt.greek_coefs.beta) == 20 and 0.1 < opt.f_trunc < 0.2 and np.all(np.abs(lin.f_trunc_dot) > 0.1)
    rng = np.random.default_rng(11)
    Sp, L = 8, 2
    tau_rayl = np.tile(0.02 * np.ones(L), (Sp, 1))
    tau_abs = 10.0 ** rng.uniform(-3, 0, (Sp, L))
    tau_aer = np.array([[0.05, 0.2]])
    tau_aer_dot = np.zeros((1, 7, L))
    tau_aer_dot[0, 0], tau_aer_dot[0, 5], tau_aer_dot[0, 6] = [0.25, 1.0], [0.5, -0.5], [-0.2, 0.3]
    geo = ("IQU", 20, 40.0, [30.0, 0.0], [0.0, 75.0])
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, tau_aer=tau_aer, depol=0.03, albedo=0.1, m_max=4)
    pm = H.model_from_arrays(arch, *geo, aerosol_optics=[opt], **kw)
    pl = H.LinModel([tau_abs.copy()], tau_aer_dot=tau_aer_dot, lin_aerosol_optics=[lin])
    om = O.build_model(*geo, aerosols=[O.AerosolOptics(O.GreekCoefs(*g_t), ref.ssa, f_t)], **kw)
    ol = OL.LinModel([tau_abs.copy()], tau_aer_dot=tau_aer_dot,
                     lin_aerosol_optics=[OL.LinAerosolOptics([O.GreekCoefs(*gtd[s]) for s in range(4)], ref.ssa_dot, ft_dot)])
    Ro, To, Rdo, Tdo = OL.rt_run_lin(om, ol)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(pm, pl, 1, 1, 1)
    assert Rd.shape == Rdo.shape and Rd.shape[-1] == 9
    print("dbge lin end to end: f_trunc %.6f f_trunc_dot %s  rel d R %.2e  d T %.2e  slots %s"
          % (opt.f_trunc, " ".join("%.4f" % v for v in lin.f_trunc_dot), _rel(R, Ro), _rel(T, To),
             " ".join("%.1e" % max(_rel(Rd[..., p], Rdo[..., p]), _rel(Td[..., p], Tdo[..., p])) for p in range(9))))
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9
    for p in range(9):
        assert _rel(Rd[..., p], Rdo[..., p]) < 1e-8 and _rel(Td[..., p], Tdo[..., p]) < 1e-8, p
    h = 1e-5

    def forward(**kwargs):
        o, = S.compute_aerosol_optical_properties(_tabulated(S, aer, r_max, nquad, **kwargs), arch, truncation=method)
        return vsm.CoreRT.rt_run(H.model_from_arrays(arch, *geo, aerosol_optics=[o], **kw))

    n_r, n_i = aer[2], aer[3]
    steps = [lambda s: dict(n_r=n_r + s), lambda s: dict(n_i=n_i + s), lambda s: dict(d_mu=s), lambda s: dict(d_sigma=s)]
    for k, step in enumerate(steps):
        (Rp, Tp), (Rm, Tm) = forward(**step(h)), forward(**step(-h))
        for an, fd in ((Rd[..., 1 + k], (Rp - Rm) / (2 * h)), (Td[..., 1 + k], (Tp - Tm) / (2 * h))):
            err = np.abs(fd - an) / np.abs(fd).max()
            print("  slot %d (%s): err max %.2e mean %.2e" % (1 + k, ML.SLOTS[k], err.max(), err.mean()))
            assert err.max() < 1e-3 and err.mean() < 1e-4, (k, err.max(), err.mean())


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(vsm, arch):
    S, H = vsm.Scattering, vsm.host_model
    lib = vsm._lib.lib()
    none = [None] * 15
    assert lib.vsm_truncate_dbge_lin(200, 129, 0, 1.0, *none) == 2         # VSM_ERR_UNSUPPORTED
    assert lib.vsm_truncate_dbge_lin(200, 2, 0, 1.0, *none) == 1           # VSM_ERR_INVALID_ARG
    assert lib.vsm_truncate_dbge_lin(20, 20, 0, 1.0, *none) == 1           # n_mu <= l_max
    assert lib.vsm_truncate_dbge_lin(200, 20, 150, 0.5, *none) == 2        # the low-confidence variant is not linearized
    buf = torch.zeros(max(4 * 6 * 200, int(lib.vsm_dbge_lin_work_elems(200, 20))), dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    #                                              greek bulk_f scal greek' bulk_f' scal' mu w_mu ...
    assert lib.vsm_truncate_dbge_lin(200, 20, 0, 1.0, p, None, None, p, p, None, p, p, p, p, p, p, p, p, None) == 1   # a lone bulk_f_dot
    assert lib.vsm_truncate_dbge_lin(200, 20, 0, 1.0, p, p, p, p, None, None, p, p, p, p, p, p, p, p, None) == 1      # bulk_f without it
    assert lib.vsm_truncate_dbge_lin(200, 20, 0, 1.0, p, p, None, p, p, p, p, p, p, p, p, p, p, p, None) == 1         # a lone bulk_f
    assert lib.vsm_truncate_dbge_lin(200, 20, 0, 1.0, p, None, None, None, None, None, p, p, p, p, p, p, p, p, None) == 1   # no greek_dot
    assert lib.vsm_truncate_dbge_lin(200, 20, 0, 1.0, p, None, None, p, None, None, p, p, p, p, None, p, p, p, None) == 1   # no greek_t_dot
    assert lib.vsm_dbge_lin_work_elems(200, 129) == 0 and lib.vsm_dbge_lin_work_elems(20, 20) == 0
    assert lib.vsm_dbge_lin_work_elems(200, 2) == 0
    for n_mu, l_max in ((200, 20), (113, 3), (307, 112), (761, 128)):
        assert lib.vsm_dbge_lin_work_elems(n_mu, l_max) > lib.vsm_dbge_work_elems(n_mu, l_max) > 0
    hg = TO.henyey_greenstein_greek(0.7, 200)
    hg_dot = np.zeros((4, 6, 200))
    hg_dot[0, 1] = hg[1]
    src, lin_src = _plain_pair(vsm, hg, hg_dot, 1.0)
    for bad in (S.DeltaBGE(129), S.DeltaBGE(2)):
        with pytest.raises(vsm.VSMError):
            S.truncate_phase_lin(bad, src, lin_src, arch)
    with pytest.raises(vsm.VSMError):                                   # a CPU architecture
        S.truncate_phase_lin(S.DeltaBGE(20), src, lin_src, vsm.Architectures.CPU())
    with pytest.raises(vsm.VSMError):                                   # lists of different length
        S.truncate_phase_lin(S.DeltaBGE(20), [src, src], [lin_src], arch)
    with pytest.raises(vsm.VSMError):                                   # one set against a list
        S.truncate_phase_lin(S.DeltaBGE(20), src, [lin_src], arch)
    with pytest.raises(vsm.VSMError):                                   # derivative vectors of another length
        S.truncate_phase_lin(S.DeltaBGE(20), src, _plain_pair(vsm, hg[:, :150], hg_dot[:, :, :150])[1], arch)
    for row in (2, 4):                                                  # a skipped system whose derivative series is not zero
        moving = hg_dot.copy()
        moving[3, row, 5] = 1e-3
        with pytest.raises(vsm.VSMError, match=NAMES[row]):
            S.truncate_phase_lin(S.DeltaBGE(20), src, _plain_pair(vsm, hg, moving)[1], arch)
        with pytest.raises(vsm.VSMError, match=NAMES[row]):             # (refused whatever the method: nothing is launched)
            S.truncate_phase_lin(S.NoTruncation(), src, _plain_pair(vsm, hg, moving)[1], arch)
    with pytest.raises(vsm.VSMError):
        S.compute_truncated_aerosol_optical_properties_lin(_model(S, "test"), S.DeltaBGE(129), arch)
    with pytest.raises(vsm.VSMError):
        S.compute_truncated_aerosol_optical_properties_lin(_model(S, "test"), S.DeltaBGE(20), vsm.Architectures.CPU())
    short, lin_short = _plain_pair(vsm, hg[:, :20], hg_dot[:, :, :20], 1.0)      # len(beta) = 20 <= l_max
    for method in (S.DeltaBGE(20), S.DeltaBGE(64), S.NoTruncation()):
        kept, lkept = S.truncate_phase_lin(method, short, lin_short, arch)
        assert kept.greek_coefs is short.greek_coefs and lkept.lin_greek_coefs is lin_short.lin_greek_coefs
        assert kept.f_trunc == 0.0 and kept.c0 == 1.0 and kept.method == S.NoTruncation() and kept.untruncated is short
        assert np.array_equal(lkept.f_trunc_dot, np.zeros(4)) and np.array_equal(lkept.c0_dot, np.zeros(4))
        assert lkept.method == S.NoTruncation() and lkept.untruncated is lin_short and lkept.ssa_dot is lin_short.ssa_dot


# ---- 8. a failed system is a status ----------------------------------------------------------------------------------------
def test_a_phase_function_through_zero_is_a_status_not_a_fault(vsm, arch):
    """beta = (1, 3, 0, ...): f11 = 1 + 3 mu changes sign inside the node range.  The beta system reports info = 2, its
    derivative rows are NaN on the device, the host raises naming the system, and the next call is correct."""
    S = vsm.Scattering
    greek = np.zeros((6, 40))
    greek[1, :2] = (1.0, 3.0)
    greek_dot = np.zeros((4, 6, 40))
    greek_dot[0, 1, 1] = 1.0
    with pytest.raises(vsm.VSMError, match="beta"):
        S.truncate_phase_lin(S.DeltaBGE(20), *_plain_pair(vsm, greek, greek_dot), arch)
    ref = _oracle_set("test")
    opt, lin = S.truncate_phase_lin(S.DeltaBGE(20), *_plain_pair(vsm, ref.greek, ref.greek_dot, ref.ssa, ref.ssa_dot), arch)
    fit, d = _oracle_fit("test", 20)
    _compare_lin(lin, fit[3:], d, "after the refused set")
