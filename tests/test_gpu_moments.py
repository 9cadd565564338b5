"""GPU tests of the Fourier loop past VSM_MM_MAX = 24 moments per launch (csrc/vsm_internal.h): the per-layer phase-matrix mixes
(vsm_mix_Z / vsm_mix_Z_moments) against numpy, the forward rt_run with a second and a partial last moment group, and the
linearized rt_run / SceneLin folded walk past 24 moments and at its structural edges -- against the oracles.

Tolerances: the kernels' own (test_gpu_lin.py, test_gpu_coxmunk.py): mixes 1e-15 (FP64) / 1e-6 (FP32) relative to the float64
sum; rt_run and rt_run_lin 1e-8 (the C3 gate) in FP64; Float32 models 1e-2 against the FP64 oracle and the test_rt_run_lin_fp32
gates (R, T 5e-4, Jacobians 2e-3) against the FP32 oracle.  The oracle runs are cached per configuration (module lru_cache)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vsm_oracle as O
from oracle import vsm_oracle_coxmunk as CM
from oracle import vsm_oracle_lin as OL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M_MAXES = [23, 24, 25, 48]      # 24, 25, 26, 49 moments: one full group, a group of one, a group of two, two full groups + one
VSM_ERR_INVALID_ARG = 1         # include/vsmartmom_hip.h


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- (a) vsm_mix_Z_moments / vsm_mix_Z against numpy ---------------------------------------------------------------------------
_TD = {np.float64: torch.float64, np.float32: torch.float32}
_SFX = {np.float64: "f64", np.float32: "f32"}
_PAD = 37   # NaN guard elements on either side of the output


def _guarded(n, FT):
    """A NaN-filled output of n elements with _PAD guard elements on either side: (buffer, the n-element view)."""
    buf = torch.full((n + 2 * _PAD,), float("nan"), dtype=_TD[FT], device="cuda")
    return buf, buf[_PAD:_PAD + n]


def _mix_inputs(FT, N, S, ncomp, nm, seed):
    """Per moment a component stack of max(ncomp, 3) blocks [N, N] and per point ncomp weights.  Positive entries (the weights are
    mixing fractions): the float64 sum has no cancellation, so the gate is a few ulp of the output's magnitude."""
    rng = np.random.default_rng(seed)
    nb = max(ncomp, 3)
    zp = [(0.1 + rng.random((nb, N, N))).astype(FT) for _ in range(nm)]
    zm = [(0.1 + rng.random((nb, N, N))).astype(FT) for _ in range(nm)]
    f = rng.random((S, max(ncomp, 1))).astype(FT)
    return zp, zm, f


def _mix_ref(stack, f, ncomp, single):
    """[S, N, N] float64: point s's mix of the stack (ncomp = 0: block `single` copied)."""
    st = stack.astype(np.float64)
    if ncomp == 0:
        return np.broadcast_to(st[single], (f.shape[0],) + st.shape[1:])
    return np.einsum("sk,kij->sij", f.astype(np.float64)[:, :ncomp], st[:ncomp])


def _call_mix_moments(vsm, FT, N, S, ncomp, nm, zp_d, zm_d, single, f_d, out_p, out_m):
    fn = getattr(vsm._lib.lib(), "vsm_mix_Z_moments_" + _SFX[FT])
    n_ptr = max(nm, 1)
    pp = (C.c_void_p * n_ptr)(*[zp_d[i % len(zp_d)].data_ptr() for i in range(n_ptr)])
    pm = (C.c_void_p * n_ptr)(*[zm_d[i % len(zm_d)].data_ptr() for i in range(n_ptr)])
    rc = fn(N, S, ncomp, nm, pp, pm, single, f_d.data_ptr() if ncomp else None, out_p.data_ptr(), out_m.data_ptr(),
            vsm.CoreRT._stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("FT,tol", [(np.float64, 1e-15), (np.float32, 1e-6)])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("N", [7, 60, 97])
@pytest.mark.parametrize("nm", [1, 7, 24])
@pytest.mark.parametrize("ncomp", [0, 1, 3, 4])
def test_mix_Z_moments_vs_numpy(vsm, FT, tol, S, N, nm, ncomp):
    """vsm_mix_Z_moments: block (im S + s) of the output is moment im's stack mixed with point s's weights (ncomp = 0: block
    `single` of every stack) -- every block written, nothing outside the nm S blocks."""
    zp, zm, f = _mix_inputs(FT, N, S, ncomp, nm, seed=nm * 100 + ncomp * 10 + N + S)
    single = 2 if ncomp == 0 else 0
    zp_d = [torch.from_numpy(z).cuda() for z in zp]
    zm_d = [torch.from_numpy(z).cuda() for z in zm]
    f_d = torch.from_numpy(np.ascontiguousarray(f[:, :max(ncomp, 1)])).cuda()
    NN = N * N
    bp, op = _guarded(nm * S * NN, FT)
    bm, om = _guarded(nm * S * NN, FT)
    assert _call_mix_moments(vsm, FT, N, S, ncomp, nm, zp_d, zm_d, single, f_d, op, om) == 0
    for buf, out, stacks in ((bp, op, zp), (bm, om, zm)):
        hb = buf.cpu().numpy()
        assert np.all(np.isnan(hb[:_PAD])) and np.all(np.isnan(hb[_PAD + nm * S * NN:])), "write outside the nm S blocks"
        got = out.cpu().numpy().reshape(nm, S, N, N)
        assert not np.any(np.isnan(got)), "a block (im S + s) left unwritten"
        for im in range(nm):
            assert _rel(got[im], _mix_ref(stacks[im], f, ncomp, single)) < tol, im


@pytest.mark.parametrize("FT", [np.float64, np.float32])
def test_mix_Z_moments_limits_and_empty_calls(vsm, FT):
    """nm = VSM_MM_MAX + 1 is refused with VSM_ERR_INVALID_ARG before anything is launched; nm = 0 and S = 0 are no-ops."""
    N, S, ncomp = 7, 2, 2
    zp, zm, f = _mix_inputs(FT, N, S, ncomp, 25, seed=3)
    zp_d = [torch.from_numpy(z).cuda() for z in zp]
    zm_d = [torch.from_numpy(z).cuda() for z in zm]
    f_d = torch.from_numpy(np.ascontiguousarray(f)).cuda()
    mm = vsm.CoreRT.MOMENT_BATCH_MAX
    for nm_, S_, rc_want in ((mm + 1, S, VSM_ERR_INVALID_ARG), (0, S, 0), (3, 0, 0)):
        bp, op = _guarded(25 * S * N * N, FT)
        bm, om = _guarded(25 * S * N * N, FT)
        rc = _call_mix_moments(vsm, FT, N, S_, ncomp, nm_, zp_d, zm_d, 0, f_d, op, om)
        assert rc == rc_want, (nm_, S_, rc)
        if rc:
            assert "limit" in vsm._lib.lib().vsm_last_error().decode()
        assert torch.all(torch.isnan(bp)) and torch.all(torch.isnan(bm)), (nm_, S_)


@pytest.mark.parametrize("FT,tol", [(np.float64, 1e-15), (np.float32, 1e-6)])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("N", [7, 60, 97])
@pytest.mark.parametrize("ncomp", [1, 3, 4])
def test_mix_Z_vs_numpy(vsm, FT, tol, S, N, ncomp):
    """vsm_mix_Z: Z[s] = sum_k fcomp[s, k] Z_k for every point, nothing written outside the S blocks."""
    zp, zm, f = _mix_inputs(FT, N, S, ncomp, 1, seed=ncomp * 10 + N + S)
    zp_d, zm_d = torch.from_numpy(zp[0]).cuda(), torch.from_numpy(zm[0]).cuda()
    f_d = torch.from_numpy(np.ascontiguousarray(f[:, :ncomp])).cuda()
    NN = N * N
    bp, op = _guarded(S * NN, FT)
    bm, om = _guarded(S * NN, FT)
    vsm._lib.call("vsm_mix_Z", _TD[FT], N, S, ncomp, zp_d.data_ptr(), zm_d.data_ptr(), f_d.data_ptr(), op.data_ptr(),
                  om.data_ptr(), vsm.CoreRT._stream_ptr())
    torch.cuda.synchronize()
    for buf, out, stack in ((bp, op, zp[0]), (bm, om, zm[0])):
        hb = buf.cpu().numpy()
        assert np.all(np.isnan(hb[:_PAD])) and np.all(np.isnan(hb[_PAD + S * NN:]))
        got = out.cpu().numpy().reshape(S, N, N)
        assert not np.any(np.isnan(got))
        assert _rel(got, _mix_ref(stack, f, ncomp, 0)) < tol


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
GEO = (35.0, [0.0, 20.0, 40.0], [0.0, 90.0, 180.0])
TAU_RAYL = np.array([0.02, 0.04, 0.06, 0.08])
TAU_AER = np.array([[0.0, 0.1, 0.3, 0.05]])


def _greek(nl=60, g=0.75):
    """A polarized aerosol whose Greek expansion runs to l = nl (Henyey-Greenstein beta, the other five proportional): its phase
    matrices carry every Fourier moment the runs below reach."""
    b = O.hg_greek(g, nl).beta
    hi = np.arange(nl + 1) >= 2
    return dict(alpha=np.where(hi, 0.85 * b, 0.0), beta=b, gamma=np.where(hi, -0.1 * b, 0.0), delta=0.8 * b,
                epsilon=np.where(hi, 0.05 * b, 0.0), zeta=np.where(hi, 0.75 * b, 0.0))


def _tau_abs(S, L, seed):
    """[S, L] absorption whose point 0 is the largest in every layer and whose last point is the smallest: any prefix of the
    points and any batch spanning the two ends has the same per-layer maxima, so the same ndoubl (batch-global) as the oracle's
    run on those points."""
    rng = np.random.default_rng(seed)
    hi, lo = 10.0 ** rng.uniform(-1.5, -1.0, L), 10.0 ** rng.uniform(-3.5, -3.0, L)
    t = np.linspace(0.0, 1.0, S)[:, None] if S > 1 else np.zeros((1, 1))
    return hi[None, :] ** (1 - t) * lo[None, :] ** t


@functools.lru_cache(maxsize=None)
def _oracle_fwd(pol, l_trunc, m_max, FT):
    """CM.rt_run of the two-point Cox-Munk + aerosol scene (the two ends of every forward batch below)."""
    om = O.build_model(pol, l_trunc, *GEO, np.tile(TAU_RAYL, (2, 1)), tau_abs=_tau_abs(2, 4, 11), tau_aer=TAU_AER,
                       aerosols=[O.AerosolOptics(O.GreekCoefs(**_greek()), 0.95, 0.0)], depol=0.0279, m_max=m_max, FT=FT)
    return CM.rt_run(om, CM.CoxMunkSurface(5.0))


def _model_fwd(vsm, arch, pol, l_trunc, S, m_max, FT):
    H = vsm.host_model
    ga = _tau_abs(S, 4, 11)
    return H.model_from_arrays(arch, pol, l_trunc, *GEO, np.tile(TAU_RAYL, (S, 1)), tau_abs=ga, tau_aer=TAU_AER,
                               aerosol_optics=[H.AerosolOptics(H.GreekCoefs(**_greek()), 0.95, 0.0)], depol=0.0279,
                               m_max=m_max, float_type=FT, surface=H.CoxMunkSurface(wind_speed=5.0))


# ---- (b) forward rt_run across moment groups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("S", [2, 1024])      # groups of 24 (4096 // S >= 24) and of MOMENT_BATCH = 4 (4096 // S = 4)
@pytest.mark.parametrize("m_max", M_MAXES)
def test_rt_run_across_moment_groups(vsm, arch, monkeypatch, FT, S, m_max):
    """rt_run on a Cox-Munk ocean under an aerosol with moments past l = 24: the first, full, and partial last moment groups of
    Scene.run (native runs of at most VSM_MM_MAX moments) vs the oracle at the two ends of the batch, and == the moment-by-moment
    walk (MOMENT_BATCHING = False)."""
    CR = vsm.CoreRT
    pol, l_trunc = "IQU", 11
    want = max(CR.MOMENT_BATCH, min(CR.MOMENT_BATCH_MAX, 4096 // S))
    assert want == (24 if S == 2 else 4)
    model = _model_fwd(vsm, arch, pol, l_trunc, S, m_max, FT)
    R, T = CR.rt_run(model)
    assert R.dtype == FT and R.shape == (3, 3, S)
    ends = [0, S - 1]
    Ro, To = _oracle_fwd(pol, l_trunc, m_max, np.float64)
    if FT == np.float64:
        assert _rel(R[..., ends], Ro) < 1e-8 and _rel(T[..., ends], To) < 1e-8, (_rel(R[..., ends], Ro), _rel(T[..., ends], To))
    else:
        assert _rel(R[..., ends], Ro) < 1e-2 and _rel(T[..., ends], To) < 1e-2
        R32, T32 = _oracle_fwd(pol, l_trunc, m_max, np.float32)
        assert _rel(R[..., ends], R32) < 5e-4 and _rel(T[..., ends], T32) < 5e-4, (_rel(R[..., ends], R32), _rel(T[..., ends], T32))
    if FT == np.float64:
        monkeypatch.setattr(CR, "MOMENT_BATCHING", False)
        Rs, Ts = CR.rt_run(model)
        monkeypatch.setattr(CR, "MOMENT_BATCHING", True)
        assert _rel(Rs, R) < 1e-12 and _rel(Ts, T) < 1e-12


def test_rt_run_sees_the_moments_past_24(vsm, arch):
    """The scenes above are sensitive to the high moments: R at m_max = 25 differs from R at m_max = 23 by far more than the gate
    (a dropped, repeated or misplaced group of moments could not pass it)."""
    Ra, _ = _oracle_fwd("IQU", 11, 23, np.float64)
    Rb, _ = _oracle_fwd("IQU", 11, 25, np.float64)
    assert _rel(Ra, Rb) > 100 * 1e-8
    # on the device without the TMS term (it depends on m_max itself): the Fourier sum alone
    R_ = []
    for m_max in (23, 25):
        scene = vsm.CoreRT.prepare_scene(_model_fwd(vsm, arch, "IQU", 11, 2, m_max, np.float64))
        scene.ss_correction = False
        scene.run()
        torch.cuda.synchronize()
        R_.append(scene.results_host()[0])
    assert _rel(R_[0], R_[1]) > 100 * 1e-8


# ---- (c) linearized rt_run / SceneLin past 24 moments --------------------------------------------------------------------------
L_LIN = 4


@functools.lru_cache(maxsize=None)
def _oracle_lin(pol, l_trunc, m_max, FT):
    """CM.rt_run_lin of the three-point Cox-Munk scene (gas + wind-speed slots); the runs with S < 3 take its first S points."""
    ga = _tau_abs(3, L_LIN, 21)
    om = O.build_model(pol, l_trunc, *GEO, np.tile(TAU_RAYL, (3, 1)), tau_abs=ga, depol=0.0279, m_max=m_max, FT=FT)
    return CM.rt_run_lin(om, OL.LinModel([ga]), CM.CoxMunkSurface(5.0))


def _scene_lin(vsm, arch, pol, l_trunc, S, m_max, FT):
    H = vsm.host_model
    ga = _tau_abs(3, L_LIN, 21)[:S]
    model = H.model_from_arrays(arch, pol, l_trunc, *GEO, np.tile(TAU_RAYL, (S, 1)), tau_abs=ga, depol=0.0279, m_max=m_max,
                                float_type=FT, surface=H.CoxMunkSurface(wind_speed=5.0))
    return vsm.CoreRTLin.SceneLin(model, H.LinModel([ga]), 0, 1, 1)


def _clone_run(scene, **kw):
    out = [t.clone() for t in scene.run(**kw)]
    torch.cuda.synchronize()
    return out


def _close(a, b, tol):
    return float((a - b).abs().max()) <= tol * float(b.abs().max())


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("pol,l_trunc", [("IQU", 11), ("IQUV", 9)])   # N = 30, 28
@pytest.mark.parametrize("m_max", M_MAXES)
def test_rt_run_lin_folded_past_24_moments(vsm, arch, FT, S, pol, l_trunc, m_max):
    """SceneLin's default walk of a small batch (the moments folded into the spectral axis, vsm_mix_Z_moments in chunks of at
    most VSM_MM_MAX moments) vs the linearized Cox-Munk oracle; in FP64 also == the moment-by-moment walk, == each form of the
    folded walk (PARALLEL_LAYERS, MERGE_M0, TREE_INTERACTIONS off), and at 26 moments the graph replay == the eager run."""
    CL = vsm.CoreRTLin
    scene = _scene_lin(vsm, arch, pol, l_trunc, S, m_max, FT)
    assert 0 < S < scene.LANE_POINTS and scene.Zall is None and scene.host_zdot is None   # (the default is the folded walk)
    dflt = _clone_run(scene)
    R, T, Rd, Td = scene.results_host()
    assert R.dtype == FT and Rd.shape == (3, scene.pol.n, S, 2)
    Ro, To, Rdo, Tdo = (a[:, :, :S] for a in _oracle_lin(pol, l_trunc, m_max, np.float64))
    if FT == np.float64:
        for name, a, b in (("R", R, Ro), ("T", T, To), ("Rd", Rd, Rdo), ("Td", Td, Tdo)):
            assert _rel(a, b) < 1e-8, (name, _rel(a, b))
        for p in range(2):
            assert _rel(Rd[..., p], Rdo[..., p]) < 1e-8 and _rel(Td[..., p], Tdo[..., p]) < 1e-8, p
    else:
        assert _rel(R, Ro) < 1e-2 and _rel(T, To) < 1e-2
        for p in range(2):
            assert _rel(Rd[..., p], Rdo[..., p]) < 1e-2 and _rel(Td[..., p], Tdo[..., p]) < 1e-2, p
        R32, T32, Rd32, Td32 = (a[:, :, :S] for a in _oracle_lin(pol, l_trunc, m_max, np.float32))
        assert _rel(R, R32) < 5e-4 and _rel(T, T32) < 5e-4, (_rel(R, R32), _rel(T, T32))
        for p in range(2):
            assert _rel(Rd[..., p], Rd32[..., p]) < 2e-3 and _rel(Td[..., p], Td32[..., p]) < 2e-3, p
        return
    seq = _clone_run(scene, lanes=1)
    for a, b in zip(seq, dflt):
        assert _close(b, a, 1e-13)
    SL = CL.SceneLin
    saved = (SL.PARALLEL_LAYERS, SL.MERGE_M0, SL.TREE_INTERACTIONS)
    try:
        for pl_, mg_, tr_ in ((False, False, False), (True, False, False), (False, True, False), (True, True, False), (True, True, True)):
            SL.PARALLEL_LAYERS, SL.MERGE_M0, SL.TREE_INTERACTIONS = pl_, mg_, tr_
            scene._fold = {}
            alt = _clone_run(scene, lanes=4, fold=True)
            for a, b in zip(dflt, alt):
                assert _close(b, a, 1e-11 if tr_ else 1e-13), (pl_, mg_, tr_)
    finally:
        SL.PARALLEL_LAYERS, SL.MERGE_M0, SL.TREE_INTERACTIONS = saved
        scene._fold = {}
    if m_max == 25:
        eager = _clone_run(scene, graph=False)
        graph = _clone_run(scene, graph=True)
        again = _clone_run(scene, graph=True)
        for a, b, c in zip(eager, graph, again):
            assert torch.equal(a, b) and torch.equal(a, c)


# ---- (d) structural edges of the folded walk -----------------------------------------------------------------------------------
@pytest.mark.parametrize("column", ["Nz1", "Nz2", "Nz3", "Nz5", "Nz7", "noscat_in_the_middle", "S40"])
def test_rt_run_lin_folded_walk_structure(vsm, arch, column):
    """The folded walk on columns off its common shape: Nz = 1, 2, 3 (the chain, no tree), 5, 7 (the tree carries a node up a
    level), a non-scattering layer in the middle (a non-11 interface: no tree), and S = 40 with four moments (160 folded pairs >
    PARALLEL_LAYER_POINTS: the layers are doubled inline by the chain) -- vs the oracle and the moment-by-moment walk."""
    H = vsm.host_model
    pol, l_trunc, m_max = "IQU", 9, 3
    S, L = (40, 4) if column == "S40" else (3, 4)
    if column.startswith("Nz"):
        L = int(column[2:])
    rng = np.random.default_rng(L + S)
    tau_rayl = np.tile(np.linspace(0.03, 0.12, L), (S, 1))
    if column == "noscat_in_the_middle":
        tau_rayl[:, 2] = 0.0
    ga = 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    geo = (pol, l_trunc, 40.0, [30.0, 5.0], [0.0, 60.0])
    kw = dict(tau_rayl=tau_rayl, tau_abs=ga, depol=0.0279, m_max=m_max)
    pm = H.model_from_arrays(arch, *geo, albedo=0.2, **kw)
    scene = vsm.CoreRTLin.SceneLin(pm, H.LinModel([ga]), 0, 1, 1)
    nm = m_max + 1
    assert (nm * S > scene.PARALLEL_LAYER_POINTS) == (column == "S40")
    if column == "noscat_in_the_middle":
        assert any(ly["iface"] != "11" for ly in scene.fwd.moments[0]["layers"][1:])
    dflt = _clone_run(scene)
    seq = _clone_run(scene, lanes=1)
    for a, b in zip(seq, dflt):
        assert _close(b, a, 1e-13)
    Ro, To, Rdo, Tdo = OL.rt_run_lin(O.build_model(*geo, albedo=0.2, **kw), OL.LinModel([ga]))
    R, T, Rd, Td = scene.results_host()
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9, (_rel(R, Ro), _rel(T, To))
    assert _rel(Rd, Rdo) < 1e-8 and _rel(Td, Tdo) < 1e-8, (_rel(Rd, Rdo), _rel(Td, Tdo))
