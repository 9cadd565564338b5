"""GPU tests of the albedo Jacobians of the spectrally varying Lambertian surfaces: LambertianSurfaceLegendre (NSurf = number of
coefficients) and LambertianSurfaceSpline (NSurf = tables of albedo_dot, or 1) through vsm_lambertian_surface_spectral_lin_* and the
three linearized drivers, against tests/spectral_albedo_lin_oracle.py (pinned on the CPU by tests/test_oracle_spectral_albedo_lin.py).

The scene (spectral_albedo_lin_oracle.oracle_scene): brdf_lin_oracle's Rayleigh column of 3 layers, 4 spectral points with differing
absorption, one gas slot, N = 6 as Stokes_I, 18 as Stokes_IQU with F0 = (1, 0.2, 0), m = 0..3, over the Legendre albedo
[0.25, 0.08, -0.03]; and the four kernel-family shapes of tests/test_gpu_thermal_lin.py (3 points, 3 layers, two gas slots).

Tolerances, those of tests/test_gpu_brdf_lin.py for the same quantities:
  builder      1e-14 (FP64: products of at most four factors and one exp, as test_brdf_surface_lin_multi_writes_every_block), 2e-6 (FP32:
               four roundings of 6e-8 and an exp whose argument -tau_sum / mu0 >= -5 is rounded once: 5 x 6e-8 more)
  rt_run_lin   1e-8 per array and per slot (FP64), 1e-2 against the FP64 oracle (Float32); R, T against rt_run(model) 1e-9
  rt_run_ss    1e-8 / 1e-2 per slot; multi-sensor 1e-8 per level, Stokes component and slot
  finite differences of the device's FP64 forward run: 10 x spectral_albedo_lin_oracle.FD_FLOOR at FD_STEP
  walks        1e-13 of each array's maximum between walks that reorder the sum over the moments (test_gpu_lin), bit equality for
               the graph replay, the spectral shard and the blocked multi-sensor run; 1e-11 between the m = 0 Stokes_IQ sub-scene and
               the full m = 0 (the same equations at another N: test_gpu_lin's bound for another association, the interaction tree)
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
import spectral_albedo_lin_oracle as A  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import brdf_lin_oracle as B  # noqa: E402
from test_oracle_sif import sif0, sif0_dot  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_RUN = {np.float64: 1e-8, np.float32: 1e-2}
LEVELS = [0, 1, A.N_LAYERS]
FTS = [np.float64, np.float32]
FT_IDS = ["fp64", "fp32"]
SHAPES = [("I", 9), ("IQU", 33), ("IQUV", 25), ("IQUV", 61)]     # tests/test_gpu_thermal_lin.py::SHAPES, one per linearized kernel family
SHAPE_GEO = (40.0, [30.0, 5.0], [0.0, 60.0])
K = len(A.COEFF)


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _host_scene(vsm, arch, pol, surface, FT=np.float64, albedo=0.0, sources=None):
    """(host model, host lin model) of the small scene over `surface` (None: the scalar Lambertian albedo)."""
    H = vsm.host_model
    kw, gas, F0 = A.scene_arrays(O.polarization(pol).n)
    pm = H.model_from_arrays(arch, pol, A.GEO["l_trunc"], A.GEO["sza"], list(A.GEO["vza"]), list(A.GEO["vaz"]), float_type=FT,
                             surface=surface, albedo=albedo, sources=sources, **kw)
    pm.F0 = F0
    return pm, H.LinModel([gas])


def _legendre(vsm, coeff=A.COEFF):
    return vsm.host_model.LambertianSurfaceLegendre(list(coeff))


@functools.lru_cache(maxsize=None)
def _oracle(pol):
    """The oracle's runs of the small scene, computed once per polarization and only read by the tests."""
    om, ol, basis = A.oracle_scene(pol)
    return A.rt_run_lin(om, ol, basis)


_device_runs = {}


def _device_lin(vsm, arch, pol, FT):
    key = (pol, FT)
    if key not in _device_runs:
        pm, hl = _host_scene(vsm, arch, pol, _legendre(vsm), FT)
        _device_runs[key] = vsm.CoreRTLin.rt_run_lin(pm, hl, 0, 1, K)
    return _device_runs[key]


def _check_slots(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = 0.0
    for p in range(ref.shape[-1]):
        assert np.max(np.abs(ref[..., p])) > 0, (what, p)
        e = _rel(got[..., p], ref[..., p])
        worst = max(worst, e)
        assert e <= tol, (what, p, e)
    print("%s: worst slot rel err %.2e" % (what, worst))


# ---- the builder ---------------------------------------------------------------------------------------------------------------------
def _builder_inputs(vsm, arch, pol, FT, S, nK, p_layer):
    H, CR = vsm.host_model, vsm.CoreRT
    hp, op = H.polarization_type(pol), O.polarization(pol)
    qp = H.rt_set_streams(A.GEO["l_trunc"], A.GEO["sza"], list(A.GEO["vza"]), hp, FT)
    oqp = O.rt_set_streams_gausslegquad(A.GEO["l_trunc"], A.GEO["sza"], list(A.GEO["vza"]), op, FT)
    dq = CR.device_quad(qp, hp, arch, FT)
    rng = np.random.default_rng(11)
    r = lambda x: np.asarray(x, dtype=FT)          # the inputs as the kernel sees them: rounded to FT, the oracle takes them in FP64
    albedo, basis = r(rng.uniform(0.05, 0.6, S)), r(rng.standard_normal((nK, S)))
    tau_sum, tsd = r(rng.uniform(0.05, 2.0, S)), r(rng.standard_normal((S, p_layer)))
    F0 = r(rng.uniform(0.2, 1.0, (op.n, S)))       # (all Stokes components of the beam: only F0[0] may enter)
    return dq, op, oqp, albedo, basis, tau_sum, tsd, F0


def _nan_layers(vsm, arch, FT, P, N, S, shared):
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    a, al = CR.AddedLayer(FT, arch, N, S, shared=shared), CL.AddedLayerLin(FT, arch, P, N, S, shared=shared)
    for t in (a.r_mp, a.t_pp, a.r_pm, a.t_mm, a.j0_p, a.j0_m, al.ap_r_mp, al.ap_t_pp, al.ap_r_pm, al.ap_t_mm, al.ap_J0_p, al.ap_J0_m):
        t.fill_(float("nan"))
    return a, al


@pytest.mark.parametrize("FT", FTS, ids=FT_IDS)
@pytest.mark.parametrize("p_layer,gap", [(2, 1), (0, 0)], ids=["two-layer-slots", "no-layer-slot"])
@pytest.mark.parametrize("nK", [1, 3])
@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_builder_writes_every_block(vsm, arch, pol, nK, p_layer, gap, FT):
    """vsm_lambertian_surface_spectral_lin on NaN-filled per-point layers against the oracle's builder: S = 5 points, n = 1 | 3,
    K = 1 | 3 slots at isurf = p_layer + gap, one slot behind them (two layer slots, then a slot that belongs to nobody, then the
    surface slots, then another nobody's; or no layer slot at all), m = 0 and 2, a beam with Q and U.  Vectors-only mode on NaN-filled
    SHARED layers: the same vectors bit for bit, the matrices still NaN."""
    CL = vsm.CoreRTLin
    S = 5
    isurf = p_layer + gap
    P = isurf + nK + 1
    dq, op, oqp, albedo, basis, tau_sum, tsd, F0 = _builder_inputs(vsm, arch, pol, FT, S, nK, p_layer)
    N, n = int(dq.mu.numel()), op.n
    conv = vsm.Architectures.array_type(arch)
    h = vsm.Architectures.to_host
    d_alb, d_basis, d_ts, d_F0 = conv(albedo), conv(np.ascontiguousarray(basis)), conv(tau_sum), conv(np.ascontiguousarray(F0.T))
    d_tsd = CL.to_device_sp(tsd, arch, FT) if p_layer else None
    tol = 1e-14 if FT == np.float64 else 2e-6
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    for m in (0, 2):
        a, al = _nan_layers(vsm, arch, FT, P, N, S, shared=False)
        CL.lambertian_surface_spectral_lin_(dq, S, m, d_alb, d_basis, isurf, d_ts, d_tsd, p_layer, d_F0, a, al)
        va, val = _nan_layers(vsm, arch, FT, P, N, S, shared=True)
        CL.lambertian_surface_spectral_lin_(dq, S, m, d_alb, d_basis, isurf, d_ts, d_tsd, p_layer, d_F0, va, val, vectors_only=True)
        torch.cuda.synchronize()
        oa, oal = O.make_added_layer(np.float64, N, S), OL.make_added_layer_lin(np.float64, P, N, S)
        A.create_surface_layer_spectral_lin(f64(albedo), f64(basis), oa, oal, isurf, m, op, oqp, f64(tau_sum), f64(tsd), f64(F0), np.float64)
        mats = dict(r_mp=h(a.r_mp).transpose(0, 2, 1), r_pm=h(a.r_pm).transpose(0, 2, 1), t_pp=h(a.t_pp).transpose(0, 2, 1),
                    t_mm=h(a.t_mm).transpose(0, 2, 1))
        lmats = {f: h(getattr(al, f)).transpose(0, 1, 3, 2) for f in ("ap_r_mp", "ap_r_pm", "ap_t_pp", "ap_t_mm")}
        j0_p, j0_m, aJp, aJm = h(a.j0_p), h(a.j0_m), h(al.ap_J0_p), h(al.ap_J0_m)
        for t in list(mats.values()) + list(lmats.values()) + [j0_p, j0_m, aJp, aJm]:
            assert np.all(np.isfinite(t))
        # vectors-only mode: the vectors alone, on shared layers
        assert np.array_equal(h(va.j0_p), j0_p) and np.array_equal(h(va.j0_m), j0_m)
        assert np.array_equal(h(val.ap_J0_p), aJp) and np.array_equal(h(val.ap_J0_m), aJm)
        for t in (va.r_mp, va.t_pp, va.r_pm, va.t_mm, val.ap_r_mp, val.ap_t_pp, val.ap_r_pm, val.ap_t_mm):
            assert bool(torch.isnan(t).all())
        # exact zeros wherever the formulas state nothing
        assert np.all(mats["r_pm"] == 0) and np.all(j0_p == 0) and np.all(aJp == 0)
        assert all(np.all(lmats[f] == 0) for f in ("ap_r_pm", "ap_t_pp", "ap_t_mm"))
        if m > 0:
            assert all(np.all(t == 0) for t in mats.values()) and np.all(lmats["ap_r_mp"] == 0) and np.all(j0_m == 0) and np.all(aJm == 0)
            assert np.all(oa.t_pp == 0) and np.all(oal.ap_J0_m == 0)
            continue
        eye = np.broadcast_to(np.eye(N), (S, N, N))
        assert np.array_equal(mats["t_pp"], eye) and np.array_equal(mats["t_mm"], eye)
        e = [_rel(mats["r_mp"], oa.r_mp), _rel(j0_m, oa.j0_m), _rel(lmats["ap_r_mp"], oal.ap_r_mp), _rel(aJm, oal.ap_J0_m)]
        print("%s K %d p_layer %d %s: r-+ %.1e j0- %.1e ap_r-+ %.1e ap_J0- %.1e" % ((pol, nK, p_layer, FT.__name__) + tuple(e)))
        assert max(e) <= tol, e
        nobody = [p for p in range(P) if not (p < p_layer or isurf <= p < isurf + nK)]
        assert len(nobody) == gap + 1
        for p in range(P):
            live_r, live_j = isurf <= p < isurf + nK, p not in nobody
            assert (np.max(np.abs(lmats["ap_r_mp"][p])) > 0) == live_r and (np.max(np.abs(aJm[p])) > 0) == live_j, p
        if n > 1:     # only the I rows and the I -> I elements
            mask = np.ones((N, N), dtype=bool)
            mask[0::n, 0::n] = False
            assert np.all(mats["r_mp"][:, mask] == 0) and np.all(lmats["ap_r_mp"][:, :, mask] == 0)
            rows = np.arange(N) % n != 0
            assert np.all(j0_m[:, rows] == 0) and np.all(aJm[:, :, rows] == 0)


def test_builder_refuses_bad_arguments_before_any_launch(vsm, arch):
    lib = vsm._lib.lib()
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    FT = np.float64
    pm, _ = _host_scene(vsm, arch, "I", None)
    dq = CR.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    N, S, P = int(dq.mu.numel()), 2, 4
    a, al = CR.AddedLayer(FT, arch, N, S, shared=False), CL.AddedLayerLin(FT, arch, P, N, S, shared=False)
    sa, sal = CR.AddedLayer(FT, arch, N, S, shared=True), CL.AddedLayerLin(FT, arch, P, N, S, shared=True)
    da = CR.AddedLayer(FT, arch, N, S, False, 1)      # a d_symmetric layer
    t = torch.zeros(4 * S + 64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    q_ = dq.cstruct()

    def call(nK=2, isurf=2, p_layer=1, albedo=p, basis=p, layers=(a, al), vec=0):
        a_, al_ = layers[0].cstruct(), layers[1].cstruct()
        return lib.vsm_lambertian_surface_spectral_lin_f64(C.byref(q_), S, 0, albedo, basis, nK, isurf, p, p, p_layer, p, C.byref(a_),
                                                           C.byref(al_), vec, None)
    assert call(nK=0) == 1 and call(isurf=-1) == 1 and call(nK=3) == 1 and call(p_layer=3) == 1
    assert call(albedo=None) == 1 and call(basis=None) == 1
    assert call(layers=(da, al)) == 1 and call(layers=(da, al), vec=1) == 1
    assert call(layers=(sa, sal)) == 1                # shared blocks outside the vectors-only mode
    torch.cuda.synchronize()
    for lay in (al, sal):
        assert all(float(getattr(lay, f).abs().max()) == 0 for f in ("ap_r_mp", "ap_t_pp", "ap_r_pm", "ap_t_mm", "ap_J0_p", "ap_J0_m"))
    assert call() == 0 and call(layers=(sa, sal), vec=1) == 0
    torch.cuda.synchronize()


# ---- rt_run_lin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=FT_IDS)
@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_rt_run_lin_against_oracle(vsm, arch, pol, FT):
    """rt_run(model, lin_model, 0, 1, NSurf = 3) over LambertianSurfaceLegendre: R, T and every slot of Rdot, Tdot (the gas slot, then
    c0, c1, c2) against the oracle; R, T are rt_run(model)'s.  Without the feature this call raises the VSMError of
    LinInputs._check_lin_args ("has no linearized builder here")."""
    R, T, Rd, Td = _device_lin(vsm, arch, pol, FT)
    Ro, To, Rdo, Tdo = _oracle(pol)
    assert Rd.shape == R.shape + (1 + K,) and Rd.dtype == FT
    tol = TOL_RUN[FT]
    print("%s %s: R %.2e T %.2e" % (pol, FT.__name__, _rel(R, Ro), _rel(T, To)))
    assert _rel(R, Ro) <= tol and _rel(T, To) <= tol
    _check_slots(Rd, Rdo, tol, "Rdot %s %s" % (pol, FT.__name__))
    _check_slots(Td, Tdo, tol, "Tdot %s %s" % (pol, FT.__name__))
    if FT == np.float64:
        Rf, Tf = vsm.CoreRT.rt_run(_host_scene(vsm, arch, pol, _legendre(vsm))[0])
        print("%s: forward R %.2e T %.2e" % (pol, _rel(R, Rf), _rel(T, Tf)))
        assert _rel(R, Rf) <= 1e-9 and _rel(T, Tf) <= 1e-9


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_rt_run_lin_against_device_finite_differences(vsm, arch, pol):
    """Every coefficient slot against central differences of the device's own FP64 forward rt_run at FD_STEP, relative to the slot's
    maximum; bound: ten times the floor the CPU oracle shows against ITS forward run at that step (FD_FLOOR)."""
    R, T, Rd, Td = _device_lin(vsm, arch, pol, np.float64)
    h = A.FD_STEP
    worst = 0.0
    for k in range(K):
        up = vsm.CoreRT.rt_run(_host_scene(vsm, arch, pol, _legendre(vsm, A.perturbed(A.COEFF, k, h)))[0])
        dn = vsm.CoreRT.rt_run(_host_scene(vsm, arch, pol, _legendre(vsm, A.perturbed(A.COEFF, k, -h)))[0])
        for an, a, b in ((Rd[..., 1 + k], up[0], dn[0]), (Td[..., 1 + k], up[1], dn[1])):
            e = float(np.max(np.abs((a - b) / (2 * h) - an)) / np.max(np.abs(an)))
            worst = max(worst, e)
            print("%s slot c%d: %.3e" % (pol, k, e))
            assert e <= 10 * A.FD_FLOOR, (k, e)
    print("%s: device finite differences %.3e (bound %.1e)" % (pol, worst, 10 * A.FD_FLOOR))


def _shape_arrays():
    """The gas scene of tests/test_gpu_thermal_lin.py: 3 points, 3 layers, two gases."""
    rng = np.random.default_rng(0)
    S, L = 3, 3
    tau_rayl = np.tile(0.03 * np.ones(L), (S, 1))
    ga, gb = 10.0 ** rng.uniform(-2.5, -0.5, (S, L)), 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    return dict(tau_rayl=tau_rayl, tau_abs=ga + gb, depol=0.0279, m_max=2), ga, gb


@pytest.mark.parametrize("pol,l_trunc", SHAPES)
def test_kernel_family_shapes_against_oracle(vsm, arch, pol, l_trunc):
    """One shape per linearized kernel family (operator level N = 7, vsm_striplin 57, vsm_strip128lin 64, past every on-chip kernel
    136): the per-point surface layer and its per-point derivative stacks through each family's surface interaction."""
    H = vsm.host_model
    kw, ga, gb = _shape_arrays()
    pm = H.model_from_arrays(arch, pol, l_trunc, *SHAPE_GEO, surface=_legendre(vsm), **kw)
    got = vsm.CoreRTLin.rt_run_lin(pm, H.LinModel([ga, gb]), 0, 2, K)
    om = O.build_model(pol, l_trunc, *SHAPE_GEO, albedo=O.legendre_albedo(A.COEFF, 3), **kw)
    ref = A.rt_run_lin(om, OL.LinModel([ga, gb]), A.legendre_basis(K, 3))
    assert got[2].shape[-1] == 2 + K
    print("%s %d: R %.2e T %.2e" % (pol, l_trunc, _rel(got[0], ref[0]), _rel(got[1], ref[1])))
    assert _rel(got[0], ref[0]) <= 1e-8 and _rel(got[1], ref[1]) <= 1e-8
    _check_slots(got[2], ref[2], 1e-8, "Rdot %s %d" % (pol, l_trunc))
    _check_slots(got[3], ref[3], 1e-8, "Tdot %s %d" % (pol, l_trunc))


# ---- the walks of SceneLin.run ---------------------------------------------------------------------------------------------------------
def test_scene_lin_walks_agree(vsm, arch, monkeypatch):
    """Every walk carries the per-point surface layers: the default run of this small batch (folded), two lanes and the folded walk
    against the moment-by-moment walk (the order of the sum over the moments differs: 1e-13, test_gpu_lin's bound); the graph replay
    repeats the eager default bit for bit; a spectral shard is the slice of the full run bit for bit (the basis is sliced, not
    rebuilt); the m = 0 Stokes_IQ sub-scene (taken here by lowering LANE_POINTS) agrees with the full m = 0 to 1e-11 and with the
    oracle, and REDUCE_M0 = False switches it off."""
    CL = vsm.CoreRTLin
    pm, hl = _host_scene(vsm, arch, "IQU", _legendre(vsm))
    scene = CL.SceneLin(pm, hl, 0, 1, K)
    assert scene.sub0 is None and scene._layer_slots == (0, 1) and not scene.als.shared
    run = lambda sc, **kw: [t.clone() for t in (sc.run(**kw), torch.cuda.synchronize())[0]]
    seq, par, fold, dflt = run(scene, lanes=1, fold=False), run(scene, lanes=2, fold=False), run(scene, fold=True), run(scene)
    rep = run(scene, graph=True)
    for a, b, c, d, e in zip(seq, par, fold, dflt, rep):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 1e-13 * scale and float((a - c).abs().max()) <= 1e-13 * scale
        assert torch.equal(d, e) and float((a - d).abs().max()) <= 1e-13 * scale
    shard = CL.SceneLin(pm, hl, 0, 1, K, spec_slice=slice(1, 4))
    part = run(shard, lanes=1, fold=False)
    assert np.array_equal(part[0].cpu().numpy(), seq[0][1:4].cpu().numpy()) and np.array_equal(part[1].cpu().numpy(), seq[1][1:4].cpu().numpy())
    assert np.array_equal(part[2].cpu().numpy(), seq[2][:, 1:4].cpu().numpy()) and np.array_equal(part[3].cpu().numpy(), seq[3][:, 1:4].cpu().numpy())
    # the m = 0 sub-scene
    monkeypatch.setattr(CL.SceneLin, "LANE_POINTS", 2)
    sub = CL.SceneLin(pm, hl, 0, 1, K)
    assert sub.sub0 is not None and sub.sub0.N == 2 * pm.quad_points.Nquad and not sub.sub0.als.shared
    red = run(sub)
    for a, b in zip(seq, red):
        assert float((a - b).abs().max()) <= 1e-11 * float(a.abs().max())
    Ro, To, Rdo, Tdo = _oracle("IQU")
    R, T, Rd, Td = sub.results_host()
    assert _rel(R, Ro) <= 1e-8 and _rel(T, To) <= 1e-8
    _check_slots(Rd, Rdo, 1e-8, "Rdot sub0")
    _check_slots(Td, Tdo, 1e-8, "Tdot sub0")
    monkeypatch.setattr(CL, "REDUCE_M0", False)
    full = CL.SceneLin(pm, hl, 0, 1, K)
    assert full.sub0 is None
    for a, b in zip(seq, run(full)):
        assert torch.equal(a, b)


# ---- rt_run_multisensor ----------------------------------------------------------------------------------------------------------------
def _ms_err(got, ref):
    """test_gpu_multisensor_lin._err: max over levels, Stokes components and slots of max |got - ref| / max |ref| of that component."""
    worst = 0.0
    for g, r in zip(got, ref):
        r4 = r if r.ndim == 4 else r[..., None]
        g4 = g if g.ndim == 4 else g[..., None]
        for k in range(r4.shape[1]):
            for p in range(r4.shape[3]):
                sc = float(np.max(np.abs(r4[:, k, :, p])))
                e = float(np.max(np.abs(g4[:, k, :, p] - r4[:, k, :, p])))
                worst = max(worst, e / sc if sc > 0 else e)
    return worst


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_multisensor_lin(vsm, arch, pol):
    """CoreRTLin.rt_run_multisensor at the levels [0, 1, Nz]: level 0 is SceneLin.run(lanes=1, fold=False) bit for bit; levels 1 and
    Nz (the per-point surface layer alone as the bottom: the undamped surface slots) against the multi-sensor oracle; the run in
    blocks of two points is bit-identical to one pass."""
    CL = vsm.CoreRTLin
    pm, hl = _host_scene(vsm, arch, pol, _legendre(vsm))
    got = CL.rt_run_multisensor(pm, hl, 0, 1, K, LEVELS)
    sc = CL.SceneLin(pm, hl, 0, 1, K)
    sc.run(lanes=1, fold=False)
    torch.cuda.synchronize()
    for a, b in zip((got[0][0], got[1][0], got[2][0], got[3][0]), sc.results_host()):
        assert np.array_equal(a, b)
    om, ol, basis = A.oracle_scene(pol)
    ref = A.ms_lin_segmented(om, ol, LEVELS, basis)
    per = [max(_ms_err([g[i]], [r[i]]) for g, r in zip(got, ref)) for i in range(len(LEVELS))]
    print("MS %s levels %s: %s" % (pol, LEVELS, " ".join("%.2e" % x for x in per)))
    assert max(per) <= 1e-8, per
    assert got[2][1].shape[-1] == 1 + K and all(np.abs(got[2][2][..., 1 + k]).max() > 0 for k in range(K))
    blocked = CL.rt_run_multisensor(pm, hl, 0, 1, K, LEVELS, max_points=2)
    for x, y in zip(got, blocked):
        assert all(np.array_equal(a, b) for a, b in zip(x, y))


# ---- rt_run_ss -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=FT_IDS)
@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_rt_run_ss_against_oracle(vsm, arch, pol, FT):
    """CoreRTLin.rt_run_ss: the gas slot and the coefficient slots against the single-scattering oracle with the K-slot per-point
    builder (the vectors-only mode of the kernel on the scene's shared layers); R, T are rt_run_ss(model)'s bit for bit; T does not
    see the surface."""
    pm, hl = _host_scene(vsm, arch, pol, _legendre(vsm), FT)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 1, K)
    fwd = vsm.CoreRT.rt_run_ss(pm)
    assert np.array_equal(R, fwd[0]) and np.array_equal(T, fwd[1])
    om, ol, basis = A.oracle_scene(pol)
    Ro, To, Rdo, Tdo = A.rt_run_ss_lin(om, ol, basis)
    tol = TOL_RUN[FT]
    assert Rd.shape == R.shape + (1 + K,) and _rel(R, Ro) <= tol and _rel(T, To) <= tol
    _check_slots(Rd, Rdo, tol, "SS Rdot %s %s" % (pol, FT.__name__))
    assert _rel(Td[..., 0], Tdo[..., 0]) <= tol and np.all(Td[..., 1:] == 0) and np.all(Tdo[..., 1:] == 0)


# ---- all three source types over the Legendre surface --------------------------------------------------------------------------------
def test_solar_thermal_and_sif_over_the_legendre_surface(vsm, arch):
    """(SolarBeam, ThermalEmission(B_layer, one Planck table), SurfaceSIF(SIF0, two tables)) over the three-coefficient surface:
    Rdot / Tdot are pl + 3 + 1 + 2 wide.  The coefficient slots (solar + thermal slot + the emission's share) against central
    differences of the device's forward run of the same model (10 x FD_FLOOR); the SIF slots by linearity, exact up to 1e-8 as
    test_gpu_sif; the Planck slot is the forward thermal slot of its table (1e-9, test_gpu_thermal_lin.test_planck_block)."""
    H, CL, CR = vsm.host_model, vsm.CoreRTLin, vsm.CoreRT
    S, L = A.S_POINTS, A.N_LAYERS
    Bl = 0.1 + 0.02 * np.arange(L)[:, None] * (1.0 + np.arange(S))[None, :]
    Bd = np.ones((1, L, S))
    t0, td = sif0(S_=S), sif0_dot(S_=S)

    def mk(coeff=A.COEFF, table=t0):
        src = (H.SolarBeam(), H.ThermalEmission(B_layer=Bl, B_layer_dot=Bd), H.SurfaceSIF(table, td))
        return _host_scene(vsm, arch, "IQU", _legendre(vsm, coeff), sources=src)
    pm, hl = mk()
    R, T, Rd, Td = CL.rt_run_lin(pm, hl, 0, 1, K)
    pl = 1
    assert Rd.shape == R.shape + (pl + 3 + 1 + 2,) and Td.shape == Rd.shape
    R0, T0 = CR.rt_run(pm)
    assert _rel(R, R0) <= 1e-9 and _rel(T, T0) <= 1e-9
    h = A.FD_STEP
    for k in range(K):
        up, dn = CR.rt_run(mk(A.perturbed(A.COEFF, k, h))[0]), CR.rt_run(mk(A.perturbed(A.COEFF, k, -h))[0])
        for an, a, b in ((Rd[..., pl + k], up[0], dn[0]), (Td[..., pl + k], up[1], dn[1])):
            e = float(np.max(np.abs((a - b) / (2 * h) - an)) / np.max(np.abs(an)))
            print("all sources, slot c%d: %.3e" % (k, e))
            assert e <= 10 * A.FD_FLOOR, (k, e)
    # the coefficient slots really carry the thermal slot's and the emission's shares: the solar-only run differs
    solar = _device_lin(vsm, arch, "IQU", np.float64)
    assert _rel(Rd[..., pl], solar[2][..., pl]) > 1e-3
    om, _, _ = A.oracle_scene("IQU")
    Rk, Tk = O.rt_run_thermal(om, Bd[0])
    assert _rel(Rd[..., pl + 3], Rk) <= 1e-9 and _rel(Td[..., pl + 3], Tk) <= 1e-9
    for k, table in enumerate(td):
        Rs, Ts = CR.rt_run(mk(table=t0 + 0.5 * table)[0])
        assert np.max(np.abs(Rd[..., pl + 4 + k])) > 0
        assert _rel(Rd[..., pl + 4 + k], (Rs - R0) / 0.5) <= 1e-8 and _rel(Td[..., pl + 4 + k], (Ts - T0) / 0.5) <= 1e-8, k


# ---- LambertianSurfaceSpline ---------------------------------------------------------------------------------------------------------
def test_spline_surface(vsm, arch):
    """albedo = the Legendre surface's spectrum and albedo_dot = its basis: the same device inputs, the same bits as the Legendre run.
    albedo_dot = None: ONE slot, the run with albedo_dot = a table of ones bit for bit -- and, the slots being linear in their
    tables, slot c0 of the Legendre run (P_0 = 1) to rounding."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    S = A.S_POINTS
    leg = _legendre(vsm)
    alb, basis = H.surface_albedo_spectrum(leg, S), H.surface_albedo_basis(leg, S)
    ref = _device_lin(vsm, arch, "IQU", np.float64)
    pm, hl = _host_scene(vsm, arch, "IQU", H.LambertianSurfaceSpline(alb, basis))
    got = CL.rt_run_lin(pm, hl, 0, 1, K)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    one = CL.rt_run_lin(_host_scene(vsm, arch, "IQU", H.LambertianSurfaceSpline(alb))[0], hl, 0, 1, 1)
    ones = CL.rt_run_lin(_host_scene(vsm, arch, "IQU", H.LambertianSurfaceSpline(alb, np.ones((1, S))))[0], hl, 0, 1, 1)
    assert one[2].shape[-1] == 2 and all(np.array_equal(a, b) for a, b in zip(one, ones))
    # (the same arithmetic per slot, but the kernels batch two slots otherwise than four: rounding, not bits)
    assert _rel(one[0], ref[0]) <= 1e-12 and _rel(one[2], ref[2][..., :2]) <= 1e-12 and _rel(one[3], ref[3][..., :2]) <= 1e-12


# ---- refusals and the surfaces that were there before ----------------------------------------------------------------------------------
def test_refusals(vsm, arch, monkeypatch):
    """A wrong NSurf raises VSMError naming the expected count, in every driver, before the library is called; 62 coefficients and
    3 layer slots pass the limit of 64; albedo_dot on another grid is refused."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    calls = []
    real = vsm._lib.call
    monkeypatch.setattr(vsm._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    S = A.S_POINTS
    alb = H.surface_albedo_spectrum(_legendre(vsm), S)
    for surface, bad, want in ((_legendre(vsm), (1, 2, 4), 3), (H.LambertianSurfaceSpline(alb), (2, 3), 1),
                               (H.LambertianSurfaceSpline(alb, np.ones((2, S))), (1, 3), 2)):
        pm, hl = _host_scene(vsm, arch, "I", surface)
        for ns in bad:
            for drv in (lambda: CL.rt_run_lin(pm, hl, 0, 1, ns), lambda: CL.rt_run_ss(pm, hl, 0, 1, ns),
                        lambda: CL.rt_run_multisensor(pm, hl, 0, 1, ns, LEVELS)):
                with pytest.raises(vsm.VSMError, match="NSurf = %d expected" % want):
                    drv()
    assert calls == []
    kw, gas, _ = A.scene_arrays(1)
    many = H.model_from_arrays(arch, "I", A.GEO["l_trunc"], A.GEO["sza"], list(A.GEO["vza"]), list(A.GEO["vaz"]),
                               surface=H.LambertianSurfaceLegendre([0.2] + [0.0] * 61), **kw)
    with pytest.raises(vsm.VSMError, match="limit 64"):
        CL.rt_run_lin(many, H.LinModel([gas, gas, gas]), 0, 3, 62)
    with pytest.raises(ValueError, match="albedo_dot"):
        H.LambertianSurfaceSpline(alb, np.ones((2, S + 1)))
    late = H.LambertianSurfaceSpline(alb, np.ones((2, S)))
    late.albedo_dot = np.ones((2, S + 1))               # (set after construction: the scene refuses it)
    with pytest.raises((ValueError, vsm.VSMError), match="albedo_dot"):
        CL.SceneLin(_host_scene(vsm, arch, "I", late)[0], H.LinModel([gas]), 0, 1, 2)


@pytest.mark.parametrize("kind", ["lambertian", "coxmunk", "rpv"])
def test_other_surfaces_keep_their_code_path(vsm, arch, monkeypatch, kind):
    """Scalar Lambertian, Cox-Munk and RPV: the linearized run never calls the new entry point, still builds its surface with its
    own builder, keeps shared surface layers and agrees with its oracle at the bound of its own tests (1e-8)."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    calls = []
    real = vsm._lib.call
    monkeypatch.setattr(vsm._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    osurf = B.SURFACES["rpv"]
    surface = {"lambertian": None, "coxmunk": H.CoxMunkSurface(wind_speed=5.0),
               "rpv": H.rpvSurfaceScalar(*[getattr(osurf, n) for n in B.param_names(osurf)])}[kind]
    ns = 4 if kind == "rpv" else 1
    pm, hl = _host_scene(vsm, arch, "IQU", surface, albedo=0.2)
    scene = CL.SceneLin(pm, hl, 0, 1, ns)
    assert scene.als.shared and scene.added_s.shared and scene.albedo_basis is None
    first = CL.rt_run_lin(pm, hl, 0, 1, ns)
    builder = {"lambertian": "vsm_lambertian_surface_lin", "coxmunk": "vsm_brdf_surface_lin", "rpv": "vsm_brdf_surface_lin_multi"}[kind]
    assert calls.count(builder) == A.M_MAX + 1
    assert "vsm_lambertian_surface_spectral_lin" not in calls and "vsm_lambertian_surface_spectral" not in calls
    om, ol = B.oracle_scene("IQU")
    om.albedo = 0.2
    ref = {"lambertian": lambda: OL.rt_run_lin(om, ol), "coxmunk": lambda: CM.rt_run_lin(om, ol, CM.CoxMunkSurface(5.0)),
           "rpv": lambda: B.rt_run_lin(om, ol, osurf)}[kind]()
    for a, b in zip(first, ref):
        assert _rel(a, b) <= 1e-8
    # ... and the Legendre run does call it, once per moment
    calls.clear()
    CL.rt_run_lin(_host_scene(vsm, arch, "IQU", _legendre(vsm))[0], hl, 0, 1, K)
    assert calls.count("vsm_lambertian_surface_spectral_lin") == A.M_MAX + 1 and "vsm_lambertian_surface_lin" not in calls
