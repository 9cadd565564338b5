"""GPU tests of vsm.Scattering.compute_aerosol_optical_properties_lin (vsm_mie_nai2_lin, csrc/vsm_mie.hip) against
tests/mie_lin_oracle.py, which computes the n_r and the n_i derivatives separately (the device computes n_r and uses
d / d n_i = -i d / d n_r) and is itself checked against central differences in tests/test_oracle_mie_lin.py.

Bounds: the forward bounds of tests/test_gpu_mie.py carried to the scale of each derivative -- per slot and coefficient family
|dev - ref| <= 1e-6 max(1, max |ref|); ssa' 1e-6 max(1, |ref|); k', C_sca' 1e-6 max(|ref|, k); bulk_f' as bulk_f there.  The
measured maxima are in DESIGN.md 4.23.  Shapes: those at which the forward kernels are pinned (tests/test_gpu_mie.py)."""
import functools
import math

import numpy as np
import pytest

import mie_lin_oracle as ML
import mie_oracle as MO
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength
FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)
MONO = [(0.5, 1.5, 0.0), (8.0, 1.33, 0.0), (8.5, 1.33, 0.0), (100.0, 2.0, 1.0), (500.0, 1.5, 0.1)]
DIST = [(TEST_AEROSOL, 3.0, 7), (TEST_AEROSOL, 3.0, 16), (TEST_AEROSOL, 3.0, 37), (TEST_AEROSOL, 3.0, 100),
        (TEST_AEROSOL, 0.5, 16), (FINE_MODE, 0.35, 20)]
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
def _oracle_dist(aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    return ML.compute_aerosol_optical_properties_lin(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad)


@functools.lru_cache(maxsize=None)
def _oracle_mono(x, n_r, n_i):
    return ML.monodisperse_lin(x, n_r, n_i)


def _dist_model(S, aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    return S.make_mie_model(S.Aerosol(S.LogNormal(r_m, sigma_g), n_r, n_i), lam, r_max, nquad)


def _mono_model(S, x, n_r, n_i):
    return S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution([x], [1.0]), n_r, n_i), MO.MONO_WAVELENGTH)


def _stack(g):
    return np.stack([g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta])


def _greek(opt):
    return _stack(opt.greek_coefs)


def _greek_dot(lin):
    return np.stack([_stack(g) for g in lin.lin_greek_coefs])


def _same_forward(a, b):
    assert np.array_equal(_greek(a), _greek(b)) and np.array_equal(a.bulk_f, b.bulk_f)
    assert (a.ssa, a.k, a.C_ext, a.C_sca, a.f_trunc) == (b.ssa, b.k, b.C_ext, b.C_sca, b.f_trunc)


def _same_lin(a, b):
    assert np.array_equal(_greek_dot(a), _greek_dot(b)) and np.array_equal(a.bulk_f_dot, b.bulk_f_dot)
    for n in ("ssa_dot", "f_trunc_dot", "k_dot", "C_ext_dot", "C_sca_dot"):
        assert np.array_equal(getattr(a, n), getattr(b, n)), n


def _compare(vsm, arch, model, ref, what):
    """Test 1 (against the oracle) and test 2 (the forward outputs against the forward call, bit for bit) of one case."""
    S, H = vsm.Scattering, vsm.host_model
    (opt, lin), = S.compute_aerosol_optical_properties_lin(model, arch)
    fwd, = S.compute_aerosol_optical_properties(model, arch)
    assert type(opt) is S.MieAerosolOptics and isinstance(lin, S.MieLinAerosolOptics) and isinstance(lin, H.LinAerosolOptics)
    _same_forward(opt, fwd)
    gd = _greek_dot(lin)
    n_mu = ref.host.n_mu
    assert gd.shape == (4, 6, n_mu) and lin.bulk_f_dot.shape == (4, 4, n_mu) and lin.ssa_dot.shape == (4,)
    assert np.all(np.isfinite(gd)) and np.all(np.isfinite(lin.bulk_f_dot)) and np.all(np.isfinite(lin.ssa_dot))
    assert np.array_equal(lin.f_trunc_dot, np.zeros(4)) and np.array_equal(lin.k_dot, lin.C_ext_dot)
    worst = dict(greek=0.0, ssa=0.0, k=0.0, c_sca=0.0, bulk=0.0)
    for s in range(4):
        for c, name in enumerate(NAMES):
            dev = float(np.max(np.abs(gd[s, c] - ref.greek_dot[s, c]))) / max(1.0, float(np.max(np.abs(ref.greek_dot[s, c]))))
            worst["greek"] = max(worst["greek"], dev)
            assert dev <= 1e-6, (what, ML.SLOTS[s], name, dev)
        d_ssa = abs(lin.ssa_dot[s] - ref.ssa_dot[s]) / max(1.0, abs(ref.ssa_dot[s]))
        d_k = abs(lin.k_dot[s] - ref.k_dot[s]) / max(abs(ref.k_dot[s]), ref.k)
        d_c = abs(lin.C_sca_dot[s] - ref.C_sca_dot[s]) / max(abs(ref.C_sca_dot[s]), ref.k)
        worst["ssa"], worst["k"], worst["c_sca"] = max(worst["ssa"], d_ssa), max(worst["k"], d_k), max(worst["c_sca"], d_c)
        assert d_ssa <= 1e-6 and d_k <= 1e-6 and d_c <= 1e-6, (what, ML.SLOTS[s], d_ssa, d_k, d_c)
        scale = float(np.max(np.abs(ref.bulk_f_dot[s])))
        if scale == 0.0:                                   # a distribution without weight derivatives: exact zeros
            assert not np.any(lin.bulk_f_dot[s]) and not np.any(gd[s]) and lin.ssa_dot[s] == 0 and lin.k_dot[s] == 0
            assert lin.C_sca_dot[s] == 0
        else:
            d_b = float(np.max(np.abs(lin.bulk_f_dot[s] - ref.bulk_f_dot[s]))) / scale
            worst["bulk"] = max(worst["bulk"], d_b)
            assert d_b <= 1e-6, (what, ML.SLOTS[s], d_b)
    print("mie lin %s: n_max %d  worst greek' %.2e  ssa' %.2e  k' %.2e  C_sca' %.2e  bulk_f' %.2e"
          % (what, ref.host.n_max, worst["greek"], worst["ssa"], worst["k"], worst["c_sca"], worst["bulk"]))
    return opt, lin


@pytest.mark.parametrize("x,n_r,n_i", MONO)
def test_monodisperse_against_the_oracle(vsm, arch, x, n_r, n_i):
    ref = _oracle_mono(x, n_r, n_i)
    if x == 500.0:
        assert (ref.host.n_max, ref.host.n_mu) == (542, 1083)
    if x in (8.0, 8.5):
        assert ref.host.n_max == {8.0: 17, 8.5: 27}[x]
    _, lin = _compare(vsm, arch, _mono_model(vsm.Scattering, x, n_r, n_i), ref, "x = %g, m = %g - %gi" % (x, n_r, n_i))
    assert not np.any(_greek_dot(lin)[2:]) and np.any(_greek_dot(lin)[0]) and np.any(_greek_dot(lin)[1])


@pytest.mark.parametrize("aer,r_max,nquad", DIST)
def test_size_distribution_against_the_oracle(vsm, arch, aer, r_max, nquad):
    ref = _oracle_dist(aer, r_max, nquad)
    if aer is TEST_AEROSOL and r_max == 3.0:
        assert (ref.host.n_max, ref.host.n_mu) == ({7: 52, 16: 56}.get(nquad, 57), {7: 103, 16: 111}.get(nquad, 113))
    if r_max == 0.5:
        assert np.all(ref.host.x <= 8.0)
    _, lin = _compare(vsm, arch, _dist_model(vsm.Scattering, aer, r_max, nquad), ref, "r_max = %g, nquad = %d" % (r_max, nquad))
    assert np.max(np.abs(_greek_dot(lin)[:, 1, 0])) <= 1e-9       # beta_0 = 1 whatever the parameters


def test_calls_are_bit_identical(vsm, arch, monkeypatch):
    """Two calls, a call with and one without poisoned work buffers, a list of three models against three single calls."""
    S = vsm.Scattering
    models = [_dist_model(S, TEST_AEROSOL, 3.0, 100), _mono_model(S, 8.5, 1.33, 0.0), _dist_model(S, FINE_MODE, 0.35, 20)]
    one = lambda m: S.compute_aerosol_optical_properties_lin(m, arch)[0]
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    first = [one(m) for m in models]
    again = [one(m) for m in models]
    monkeypatch.delenv("VSM_POISON_WORK")
    plain = [one(m) for m in models]
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    listed = S.compute_aerosol_optical_properties_lin(models, arch)
    assert len(listed) == 3
    for other in (again, plain, listed):
        for (a, la), (b, lb) in zip(first, other):
            assert np.all(np.isfinite(_greek(a))) and np.all(np.isfinite(_greek_dot(la))) and np.all(np.isfinite(la.bulk_f_dot))
            assert np.all(np.isfinite(la.ssa_dot)) and np.all(np.isfinite(la.k_dot)) and np.all(np.isfinite(la.C_sca_dot))
            _same_forward(a, b)
            _same_lin(la, lb)


def _tabulated(S, aer, r_max, nquad, d_mu=0.0, d_sigma=0.0, with_dot=True, n_r=None, n_i=None):
    """The LogNormal's own nodes with the weights of LogNormal(mu + d_mu, sigma + d_sigma) on them."""
    r_m, sigma_g, nr0, ni0, lam = aer
    base = S.LogNormal(r_m, sigma_g)
    r, w_r = S.gauleg_log(nquad, max(base.quantile(1e-8), 1e-6 * r_max), r_max)
    ln = base if d_mu == 0.0 and d_sigma == 0.0 else S.LogNormal(math.exp(base.mu + d_mu), math.exp(base.sigma + d_sigma))
    raw = ln.pdf(r) * w_r
    tab = S.TabulatedSizeDistribution(r, raw, weights_dot=S.lognormal_raw_dot(ln, r, raw) if with_dot else None)
    return S.make_mie_model(S.Aerosol(tab, nr0 if n_r is None else n_r, ni0 if n_i is None else n_i), lam)


def test_tabulated_distribution(vsm, arch):
    S = vsm.Scattering
    run = lambda m: S.compute_aerosol_optical_properties_lin(m, arch)[0]
    a, la = run(_dist_model(S, TEST_AEROSOL, 3.0, 37))
    b, lb = run(_tabulated(S, TEST_AEROSOL, 3.0, 37))
    _same_forward(a, b)
    _same_lin(la, lb)
    c, lc = run(_tabulated(S, TEST_AEROSOL, 3.0, 37, with_dot=False))
    _same_forward(a, c)
    gd, gc = _greek_dot(la), _greek_dot(lc)
    assert np.array_equal(gd[:2], gc[:2]) and not np.any(gc[2:]) and np.any(gd[2]) and np.any(gd[3])
    assert np.array_equal(la.bulk_f_dot[:2], lc.bulk_f_dot[:2]) and not np.any(lc.bulk_f_dot[2:])
    for n in ("ssa_dot", "k_dot", "C_sca_dot"):
        assert np.array_equal(getattr(la, n)[:2], getattr(lc, n)[:2]) and not np.any(getattr(lc, n)[2:]), n


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_fine_mode_jacobians_end_to_end_through_rt_run_lin(vsm, arch):
    """A physical aerosol's Jacobian out of the package: the fine mode (19 coefficients) in the scene of
    tests/test_gpu_mie.py::test_fine_mode_aerosol_end_to_end_through_rt_run, the device's lin_optics handed to LinModel as it is.
    tau_aer_dot rows 1-4 are zero (tau_aer held fixed).  rt_run_lin(pm, pl, 1, 1, 1) against the oracle's on the oracle's
    linearized Mie optics at the bounds of tests/test_gpu_lin.py::test_rt_run_lin_aerosol_slots (1e-9 on R, T, 1e-8 per slot), and
    slots 1-4 against central differences (h = 1e-5) of the device's own forward Mie call plus rt_run, the radius nodes held fixed
    through the tabulated form (err.max() < 1e-3, err.mean() < 1e-4)."""
    S, H = vsm.Scattering, vsm.host_model
    ref = _oracle_dist(FINE_MODE, 0.35, 20)
    assert (ref.host.n_max, ref.host.n_mu) == (10, 19)
    (opt, lin), = S.compute_aerosol_optical_properties_lin(_dist_model(S, FINE_MODE, 0.35, 20), arch)
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
    om = O.build_model(*geo, aerosols=[O.AerosolOptics(O.GreekCoefs(*ref.greek), ref.ssa, 0.0)], **kw)
    ol = OL.LinModel([tau_abs.copy()], tau_aer_dot=tau_aer_dot,
                     lin_aerosol_optics=[OL.LinAerosolOptics([O.GreekCoefs(*ref.greek_dot[s]) for s in range(4)], ref.ssa_dot,
                                                             np.zeros(4))])
    Ro, To, Rdo, Tdo = OL.rt_run_lin(om, ol)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(pm, pl, 1, 1, 1)
    assert Rd.shape == Rdo.shape and Rd.shape[-1] == 9
    print("mie lin end to end: rel d R %.2e  d T %.2e  slots %s" % (_rel(R, Ro), _rel(T, To), " ".join(
        "%.1e" % max(_rel(Rd[..., p], Rdo[..., p]), _rel(Td[..., p], Tdo[..., p])) for p in range(9))))
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9
    for p in range(9):
        assert _rel(Rd[..., p], Rdo[..., p]) < 1e-8 and _rel(Td[..., p], Tdo[..., p]) < 1e-8, p
    h = 1e-5

    def forward(**kwargs):
        o, = S.compute_aerosol_optical_properties(_tabulated(S, FINE_MODE, 0.35, 20, with_dot=False, **kwargs), arch)
        return vsm.CoreRT.rt_run(H.model_from_arrays(arch, *geo, aerosol_optics=[o], **kw))

    n_r, n_i = FINE_MODE[2], FINE_MODE[3]
    steps = [lambda s: dict(n_r=n_r + s), lambda s: dict(n_i=n_i + s), lambda s: dict(d_mu=s), lambda s: dict(d_sigma=s)]
    for k, step in enumerate(steps):
        (Rp, Tp), (Rm, Tm) = forward(**step(h)), forward(**step(-h))
        for an, fd in ((Rd[..., 1 + k], (Rp - Rm) / (2 * h)), (Td[..., 1 + k], (Tp - Tm) / (2 * h))):
            err = np.abs(fd - an) / np.abs(fd).max()
            print("  slot %d (%s): err max %.2e mean %.2e" % (1 + k, ML.SLOTS[k], err.max(), err.mean()))
            assert err.max() < 1e-3 and err.mean() < 1e-4, (k, err.max(), err.mean())


def test_refusals(vsm, arch):
    S = vsm.Scattering
    ln = S.LogNormal(0.3, 2.1)
    run = lambda m, a=arch: S.compute_aerosol_optical_properties_lin(m, a)
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
    with pytest.raises(vsm.VSMError):                       # weights_dot of the wrong shape
        S.TabulatedSizeDistribution([1.0, 2.0], [0.5, 0.5], weights_dot=[[0.1, 0.2]])
    with pytest.raises(TypeError):                          # truncation is not linearized: no such parameter
        S.compute_aerosol_optical_properties_lin(_mono_model(S, 8.5, 1.33, 0.0), arch, truncation=S.DeltaBGE(20))
    (opt, lin), = run(_dist_model(S, TEST_AEROSOL, 3.0, 37))   # truncate_phase keeps working on the optics alone
    t = S.truncate_phase(S.DeltaBGE(20), opt, arch)
    assert len(t.greek_coefs.beta) == 20 and not hasattr(t, "lin_greek_coefs")
    lib = vsm._lib.lib()                                    # the library refuses what the host layer would
    assert lib.vsm_mie_nai2_lin(1, S.MAX_N_MAX + 1, 2 * S.MAX_N_MAX + 1, 1.3, 0.0, 1.0, *([None] * 16)) == 2    # VSM_ERR_UNSUPPORTED
    assert lib.vsm_mie_nai2_lin(1, 4, 7, 1.3, -0.1, 1.0, *([None] * 16)) == 1                                   # VSM_ERR_INVALID_ARG
    assert lib.vsm_mie_lin_work_elems(1, 1, 1) == 0 and lib.vsm_mie_lin_work_elems(1, 4, 7) > lib.vsm_mie_work_elems(1, 4, 7)
