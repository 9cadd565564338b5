"""GPU tests of the Jacobians with respect to the kernel-driven BRDF parameters: rpvSurfaceScalar (NSurf = 4: rho0, rho_c, k, Theta)
and RossLiSurfaceScalar (NSurf = 3: fvol, fgeo, fiso) through vsm_land_brdf_reflectance_lin_*, vsm_brdf_surface_lin_multi_* and the
three linearized drivers, against tests/brdf_lin_oracle.py (pinned on the CPU by tests/test_oracle_brdf_lin.py).

The scene (brdf_lin_oracle.oracle_scene): a Rayleigh column of 3 layers, 4 spectral points with differing absorption, one gas slot,
3 Gauss streams + the SZA node + 2 VZAs (N = 6 as Stokes_I, 18 as Stokes_IQU with F0 = (1, 0.2, 0)), m = 0..3.

Tolerances, all taken from the existing tests of the same quantities:
  tables       1e-9 (FP64), 5e-4 / 20 x 5e-4 (FP32 block / derivative) of the table maximum: test_gpu_coxmunk.test_coxmunk_reflectance_and_deriv
  rt_run_lin   1e-8 per array and per slot (FP64: test_gpu_coxmunk.test_c3_ocean_coxmunk_linearized, the Cox-Munk wind-speed case),
               1e-2 against the FP64 oracle (Float32: test_gpu_lin.test_rt_run_lin_fp32); R, T against rt_run(model) 1e-9 (test_gpu_lin)
  rt_run_ss    1e-8 / 1e-2 per slot (test_gpu_ss_lin.TOL_RUN)
  multi-sensor 1e-8 in test_gpu_multisensor_lin's measure (per level, Stokes component and slot)
  finite differences of the device's FP64 forward run: 10 x brdf_lin_oracle.FD_FLOOR at brdf_lin_oracle.FD_STEP
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import brdf_lin_oracle as B  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_TABLE = {np.float64: (1e-9, 1e-9), np.float32: (5e-4, 20 * 5e-4)}
TOL_RUN = {np.float64: 1e-8, np.float32: 1e-2}
LEVELS = [0, 1, B.N_LAYERS]
FTS = [np.float64, np.float32]
FT_IDS = ["fp64", "fp32"]


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


def _host_surface(vsm, osurf):
    H = vsm.host_model
    cls = H.rpvSurfaceScalar if isinstance(osurf, B.OB.RPVSurface) else H.RossLiSurfaceScalar
    return cls(*[getattr(osurf, n) for n in B.param_names(osurf)])


def _host_scene(vsm, arch, pol, surface, FT=np.float64, albedo=0.0):
    """(host model, host lin model) of the small scene over `surface` (None: the Lambertian albedo)."""
    H = vsm.host_model
    kw, gas, F0 = B.scene_arrays(O.polarization(pol).n)
    pm = H.model_from_arrays(arch, pol, B.GEO["l_trunc"], B.GEO["sza"], list(B.GEO["vza"]), list(B.GEO["vaz"]), float_type=FT,
                             surface=surface, albedo=albedo, **kw)
    pm.F0 = F0
    return pm, H.LinModel([gas])


@functools.lru_cache(maxsize=None)
def _oracle(pol, name):
    """The oracle's runs of the small scene, computed once per (polarization, surface) and only read by the tests."""
    om, ol = B.oracle_scene(pol)
    return dict(lin=B.rt_run_lin(om, ol, B.SURFACES[name]))


@functools.lru_cache(maxsize=None)
def _oracle_ss(pol, name):
    om, ol = B.oracle_scene(pol)
    return B.rt_run_ss_lin(om, ol, B.SURFACES[name])


_device_runs = {}


def _device_lin(vsm, arch, pol, name, FT):
    key = (pol, name, FT)
    if key not in _device_runs:
        surf = B.SURFACES[name]
        pm, hl = _host_scene(vsm, arch, pol, _host_surface(vsm, surf), FT)
        _device_runs[key] = vsm.CoreRTLin.rt_run_lin(pm, hl, 0, 1, B.n_params(surf))
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


# ---- the tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=FT_IDS)
@pytest.mark.parametrize("name", ["rpv", "rossli", "rpv_black"])
def test_land_brdf_tables(vsm, arch, FT, name):
    """vsm_land_brdf_reflectance_lin: rho[m] against host_model.brdf_reflectance (the table the forward run uses), drho[m][k] against
    the oracle, on the Stokes_IQU streams (every element outside I -> I exactly zero), all moments from one launch.  Ross-Li's
    d/dfiso is exactly zero for m > 0; d/drho0 is finite and right at rho0 = 0."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    surf = B.OB.RPVSurface(0.0, 0.08, 0.75, -0.25) if name == "rpv_black" else B.SURFACES[name]
    hs = _host_surface(vsm, surf)
    pm, _ = _host_scene(vsm, arch, "IQU", hs, FT)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    mu = pm.quad_points.qp_mu.astype(np.float64)
    rho, drho = CL.land_brdf_reflectance_lin(hs, dq, B.M_MAX, arch, FT)
    torch.cuda.synchronize()
    K, N = B.n_params(surf), 3 * len(mu)
    assert tuple(rho.shape) == (B.M_MAX + 1, N, N) and tuple(drho.shape) == (B.M_MAX + 1, K, N, N)
    th = vsm.Architectures.to_host
    r_d, d_d = th(rho).transpose(0, 2, 1), th(drho).transpose(0, 1, 3, 2)
    tol_r, tol_d = TOL_TABLE[FT]
    mask = np.ones((N, N), dtype=bool)
    mask[0::3, 0::3] = False
    for m in range(B.M_MAX + 1):
        r_h = H.brdf_reflectance(hs, 3, mu, m)
        _, d_o = B.reflectance_and_deriv(surf, 3, mu, m)
        assert np.all(r_d[m][mask] == 0) and np.all(d_d[m][:, mask] == 0)
        if name == "rpv_black":
            assert np.all(r_d[m] == 0) and np.all(d_d[m][1:] == 0) and np.all(np.isfinite(d_d[m][0]))
        else:
            e = _rel(r_d[m], r_h)
            print("%s %s m %d: rho %.2e" % (name, FT.__name__, m, e))
            assert e <= tol_r, (m, e)
        for k in range(K):
            if np.max(np.abs(d_o[k])) == 0:
                assert np.all(d_d[m][k] == 0), (m, k)
                continue
            e = _rel(d_d[m][k], d_o[k])
            print("%s %s m %d: drho[%d] %.2e" % (name, FT.__name__, m, k, e))
            assert e <= tol_d, (m, k, e)
        if name == "rossli" and m > 0:
            assert np.all(d_d[m][2] == 0)


def test_brdf_surface_lin_multi_writes_every_block(vsm, arch):
    """vsm_brdf_surface_lin_multi on NaN-filled layers against the oracle's K-slot builder: P = 7 slots = 2 layer slots, K = 3
    surface slots at isurf = 3 (slot 2 and slot 6 belong to nobody: all zero), Stokes_IQU with all components of F0, m = 0 and 2.
    The tables are the oracle's, so the builder is products of three factors and sums of three terms: a few eps (1e-14)."""
    FT = np.float64
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    om, _ = B.oracle_scene("IQU")
    pm, _ = _host_scene(vsm, arch, "IQU", None)
    dq = CR.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    pol, qp = om.pol, om.quad_points
    N, S, P, pl, K, isurf = qp.Nquad * 3, 5, 7, 2, 3, 3
    rng = np.random.default_rng(5)
    tau_sum, tsd, F0 = rng.uniform(0.05, 2.0, S), rng.standard_normal((S, pl)), rng.uniform(0.2, 1.0, (3, S))
    conv = vsm.Architectures.array_type(arch)
    h = vsm.Architectures.to_host
    for m in (0, 2):
        rho, drho = rng.uniform(0.0, 1.0, (N, N)), rng.standard_normal((K, N, N))
        a, al = CR.AddedLayer(FT, arch, N, S, shared=True), CL.AddedLayerLin(FT, arch, P, N, S, shared=True)
        for t in (a.r_mp, a.t_pp, a.r_pm, a.t_mm, a.j0_p, a.j0_m, al.ap_r_mp, al.ap_t_pp, al.ap_r_pm, al.ap_t_mm, al.ap_J0_p, al.ap_J0_m):
            t.fill_(float("nan"))
        d_rho, d_drho = conv(np.ascontiguousarray(rho.T)), conv(np.ascontiguousarray(drho.transpose(0, 2, 1)))
        CL.brdf_surface_lin_multi_(dq, S, m, d_rho, d_drho, isurf, conv(tau_sum), CL.to_device_sp(tsd, arch, FT), pl,
                                   conv(np.ascontiguousarray(F0.T)), a, al)
        torch.cuda.synchronize()
        oa, oal = O.make_added_layer(FT, N, S), OL.make_added_layer_lin(FT, P, N, S)
        B.create_surface_layer_brdf_lin(rho, drho, oa, oal, isurf, m, pol, qp, tau_sum, tsd, F0, FT)
        f3 = lambda t: h(t).transpose(0, 2, 1)
        assert _rel(f3(a.r_mp)[0], oa.r_mp[0]) <= 1e-14 and np.array_equal(f3(a.t_pp)[0], np.eye(N))
        assert np.all(h(a.r_pm) == 0) and np.all(h(a.t_mm) == 0) and np.all(h(a.j0_p) == 0)
        assert _rel(h(a.j0_m), oa.j0_m) <= 1e-14
        ar = h(al.ap_r_mp).transpose(0, 1, 3, 2)[:, 0]
        assert _rel(ar, oal.ap_r_mp[:, 0]) <= 1e-14
        for p in (0, 1, 2, 6):
            assert np.all(ar[p] == 0)
        for t in (al.ap_r_pm, al.ap_t_pp, al.ap_t_mm, al.ap_J0_p):
            assert np.all(h(t) == 0)
        aj = h(al.ap_J0_m)
        assert _rel(aj, oal.ap_J0_m) <= 1e-14 and np.all(aj[2] == 0) and np.all(aj[6] == 0)
        assert all(np.max(np.abs(aj[p])) > 0 for p in (0, 1, 3, 4, 5))


def test_new_entry_points_refuse_bad_arguments_before_any_launch(vsm, arch):
    lib = vsm._lib.lib()
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    FT = np.float64
    pm, _ = _host_scene(vsm, arch, "I", None)
    dq = CR.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    N, S, P = int(dq.mu.numel()), 2, 4
    a, al = CR.AddedLayer(FT, arch, N, S, shared=True), CL.AddedLayerLin(FT, arch, P, N, S, shared=True)
    t = torch.zeros(4 * N * N + 64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    q_, a_, al_ = dq.cstruct(), a.cstruct(), al.cstruct()

    def multi(K=2, isurf=2, p_layer=1):
        return lib.vsm_brdf_surface_lin_multi_f64(C.byref(q_), S, 0, p, p, K, isurf, p, p, p_layer, p, C.byref(a_), C.byref(al_), None)
    assert multi(K=0) == 1 and multi(K=3) == 1 and multi(isurf=-1) == 1 and multi(p_layer=3) == 1
    par = (C.c_double * 4)(0.1, 0.1, 0.8, -0.1)
    phi, w = CR.brdf_azimuth_quadrature(arch, FT)

    def table(kind=0, m_max=0, nphi=100, params=par):
        return lib.vsm_land_brdf_reflectance_lin_f64(C.byref(q_), kind, params, m_max, nphi, CR._ptr(phi), CR._ptr(w), p, p, None)
    assert table(kind=2) != 0 and table(m_max=-1) != 0 and table(nphi=0) != 0 and table(params=None) != 0
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0 and float(al.ap_J0_m.abs().max()) == 0
    assert multi() == 0


# ---- rt_run_lin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=FT_IDS)
@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("name", ["rpv", "rossli"])
def test_rt_run_lin_against_oracle(vsm, arch, name, pol, FT):
    """rt_run(model, lin_model, 0, 1, NSurf = 4 | 3): R, T and every slot of Rdot, Tdot (the gas slot, then the surface slots in
    field order) against the oracle.  Without the feature this call raises the VSMError of LinInputs._check_lin_args."""
    R, T, Rd, Td = _device_lin(vsm, arch, pol, name, FT)
    Ro, To, Rdo, Tdo = _oracle(pol, name)["lin"]
    K = B.n_params(B.SURFACES[name])
    assert Rd.shape == R.shape + (1 + K,) and Rd.dtype == FT
    tol = TOL_RUN[FT]
    print("%s %s %s: R %.2e T %.2e" % (name, pol, FT.__name__, _rel(R, Ro), _rel(T, To)))
    assert _rel(R, Ro) <= tol and _rel(T, To) <= tol
    _check_slots(Rd, Rdo, tol, "Rdot %s %s %s" % (name, pol, FT.__name__))
    _check_slots(Td, Tdo, tol, "Tdot %s %s %s" % (name, pol, FT.__name__))


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("name", ["rpv", "rossli"])
def test_forward_results_and_layer_slots_are_unchanged(vsm, arch, name, pol):
    """R, T of the linearized run are rt_run(model)'s (1e-9, the bound of test_gpu_lin); the gas slot is the oracle's (1e-8) and does
    not depend on how many surface slots follow it: the same bits over the other surface's 3 | 4 slots would be too much to ask
    (another BRDF), but the gas slot of a run is that of the oracle's run of the same scene."""
    R, T, Rd, Td = _device_lin(vsm, arch, pol, name, np.float64)
    pm, _ = _host_scene(vsm, arch, pol, _host_surface(vsm, B.SURFACES[name]))
    Rf, Tf = vsm.CoreRT.rt_run(pm)
    print("%s %s: forward R %.2e T %.2e" % (name, pol, _rel(R, Rf), _rel(T, Tf)))
    assert _rel(R, Rf) <= 1e-9 and _rel(T, Tf) <= 1e-9
    _, _, Rdo, Tdo = _oracle(pol, name)["lin"]
    assert _rel(Rd[..., 0], Rdo[..., 0]) <= 1e-8 and _rel(Td[..., 0], Tdo[..., 0]) <= 1e-8


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("name", ["rpv", "rossli"])
def test_rt_run_lin_against_device_finite_differences(vsm, arch, name, pol):
    """Every surface slot against central differences of the device's own FP64 forward rt_run at brdf_lin_oracle.FD_STEP, relative to
    the slot's maximum; bound: ten times the floor the CPU oracle shows against ITS forward run at that step (FD_FLOOR)."""
    surf = B.SURFACES[name]
    R, T, Rd, Td = _device_lin(vsm, arch, pol, name, np.float64)
    h = B.FD_STEP
    worst = 0.0
    for k in range(B.n_params(surf)):
        up = vsm.CoreRT.rt_run(_host_scene(vsm, arch, pol, _host_surface(vsm, B.perturbed(surf, k, h)))[0])
        dn = vsm.CoreRT.rt_run(_host_scene(vsm, arch, pol, _host_surface(vsm, B.perturbed(surf, k, -h)))[0])
        for an, a, b in ((Rd[..., 1 + k], up[0], dn[0]), (Td[..., 1 + k], up[1], dn[1])):
            e = float(np.max(np.abs((a - b) / (2 * h) - an)) / np.max(np.abs(an)))
            worst = max(worst, e)
            assert e <= 10 * B.FD_FLOOR, (k, e)
    print("%s %s: device finite differences %.3e (bound %.1e)" % (name, pol, worst, 10 * B.FD_FLOOR))


def test_scene_lin_walks_agree(vsm, arch):
    """All walks of SceneLin take these surfaces (the surface step is the same _finish_moment in each): lanes, the folded walk
    (the default for this batch) and the graph replay against the moment-by-moment walk, at test_gpu_lin's bounds (the order of the
    sum over the moments differs: 1e-13; the replay repeats the eager default bit for bit)."""
    surf = B.SURFACES["rpv"]
    pm, hl = _host_scene(vsm, arch, "IQU", _host_surface(vsm, surf))
    scene = vsm.CoreRTLin.SceneLin(pm, hl, 0, 1, 4)
    assert scene.sub0 is None and scene._layer_slots == (0, 1)
    run = lambda **kw: [t.clone() for t in (scene.run(**kw), torch.cuda.synchronize())[0]]
    seq, par, fold, dflt = run(lanes=1, fold=False), run(lanes=4, fold=False), run(lanes=4, fold=True), run(graph=False)
    rep = run(graph=True)
    for a, b, c, d, e in zip(seq, par, fold, dflt, rep):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 1e-13 * scale and float((a - c).abs().max()) <= 1e-13 * scale
        assert torch.equal(d, e) and float((a - d).abs().max()) <= 1e-13 * scale


# ---- rt_run_ss -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=FT_IDS)
@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("name", ["rpv", "rossli"])
def test_rt_run_ss_against_oracle(vsm, arch, name, pol, FT):
    """CoreRTLin.rt_run_ss: the gas slot and the surface slots against the single-scattering oracle with the K-slot surface layer;
    R, T are rt_run_ss(model)'s bit for bit; T does not see the surface."""
    surf = B.SURFACES[name]
    K = B.n_params(surf)
    pm, hl = _host_scene(vsm, arch, pol, _host_surface(vsm, surf), FT)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 1, K)
    fwd = vsm.CoreRT.rt_run_ss(pm)
    assert np.array_equal(R, fwd[0]) and np.array_equal(T, fwd[1])
    Ro, To, Rdo, Tdo = _oracle_ss(pol, name)
    tol = TOL_RUN[FT]
    assert Rd.shape == R.shape + (1 + K,) and _rel(R, Ro) <= tol and _rel(T, To) <= tol
    _check_slots(Rd, Rdo, tol, "SS Rdot %s %s %s" % (name, pol, FT.__name__))
    assert _rel(Td[..., 0], Tdo[..., 0]) <= tol and np.all(Td[..., 1:] == 0) and np.all(Tdo[..., 1:] == 0)


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
@pytest.mark.parametrize("name", ["rpv", "rossli"])
def test_multisensor_lin(vsm, arch, name, pol):
    """CoreRTLin.rt_run_multisensor at the levels [0, 1, Nz]: level 0 is SceneLin.run(lanes=1, fold=False) bit for bit; levels 1 and
    Nz (the surface layer alone as the bottom: the undamped surface slots) against the multi-sensor oracle with the K-slot surface."""
    surf = B.SURFACES[name]
    K = B.n_params(surf)
    pm, hl = _host_scene(vsm, arch, pol, _host_surface(vsm, surf))
    got = vsm.CoreRTLin.rt_run_multisensor(pm, hl, 0, 1, K, LEVELS)
    sc = vsm.CoreRTLin.SceneLin(pm, hl, 0, 1, K)
    sc.run(lanes=1, fold=False)
    torch.cuda.synchronize()
    for a, b in zip((got[0][0], got[1][0], got[2][0], got[3][0]), sc.results_host()):
        assert np.array_equal(a, b)
    om, ol = B.oracle_scene(pol)
    ref = B.ms_lin_segmented(om, ol, LEVELS, surf)
    per = [max(_ms_err([g[i]], [r[i]]) for g, r in zip(got, ref)) for i in range(len(LEVELS))]
    print("MS %s %s levels %s: %s" % (name, pol, LEVELS, " ".join("%.2e" % x for x in per)))
    assert max(per) <= 1e-8, per
    assert got[2][1].shape[-1] == 1 + K and all(np.abs(got[2][2][..., 1 + k]).max() > 0 for k in range(K))


# ---- refusals and the one-slot surfaces ----------------------------------------------------------------------------------------------
def test_refusals(vsm, arch, monkeypatch):
    """rpvSurfaceScalar with NSurf = 1 or 3 and RossLiSurfaceScalar with NSurf = 4 raise VSMError naming the expected count, in
    every driver, before the library is called."""
    calls = []
    real = vsm._lib.call
    monkeypatch.setattr(vsm._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    CL = vsm.CoreRTLin
    for name, bad, want in (("rpv", (1, 3), 4), ("rossli", (4, 1), 3)):
        pm, hl = _host_scene(vsm, arch, "I", _host_surface(vsm, B.SURFACES[name]))
        for ns in bad:
            for drv in (lambda: CL.rt_run_lin(pm, hl, 0, 1, ns), lambda: CL.rt_run_ss(pm, hl, 0, 1, ns),
                        lambda: CL.rt_run_multisensor(pm, hl, 0, 1, ns, LEVELS)):
                with pytest.raises(vsm.VSMError, match="NSurf = %d expected" % want):
                    drv()
    assert calls == []
    pm, hl = _host_scene(vsm, arch, "I", None, albedo=0.2)
    with pytest.raises(vsm.VSMError, match="NSurf = 1"):
        CL.rt_run_lin(pm, hl, 0, 1, 4)


@pytest.mark.parametrize("kind", ["lambertian", "coxmunk"])
def test_one_slot_surfaces_keep_their_code_path(vsm, arch, monkeypatch, kind):
    """Lambertian and Cox-Munk with NSurf = 1: two runs through the public API give the same bits, agree with their oracles at the
    bounds of the existing tests, and still build their surface with vsm_lambertian_surface_lin / vsm_brdf_surface_lin (and
    vsm_coxmunk_reflectance) -- neither new entry point is called."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    calls = []
    real = vsm._lib.call
    monkeypatch.setattr(vsm._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    pm, hl = _host_scene(vsm, arch, "IQU", H.CoxMunkSurface(wind_speed=5.0) if kind == "coxmunk" else None, albedo=0.2)
    first = CL.rt_run_lin(pm, hl, 0, 1, 1)
    second = CL.rt_run_lin(pm, hl, 0, 1, 1)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    builder = "vsm_brdf_surface_lin" if kind == "coxmunk" else "vsm_lambertian_surface_lin"
    assert calls.count(builder) == 2 * (B.M_MAX + 1)
    assert "vsm_brdf_surface_lin_multi" not in calls and "vsm_land_brdf_reflectance_lin" not in calls
    assert ("vsm_coxmunk_reflectance" in calls) == (kind == "coxmunk")
    om, ol = B.oracle_scene("IQU")
    om.albedo = 0.2
    ref = CM.rt_run_lin(om, ol, CM.CoxMunkSurface(5.0)) if kind == "coxmunk" else OL.rt_run_lin(om, ol)
    for a, b in zip(first, ref):
        assert _rel(a, b) <= 1e-8
