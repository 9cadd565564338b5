"""GPU tests of the linearized multi-sensor run (vsm.CoreRTLin.rt_run_multisensor, core_rt_ms_lin.py) and its level kernel
(vsm_level_radiance_lin_*, csrc/vsm_level.hip): against the numpy restatement (tests/ms_lin_oracle.py, itself pinned by finite
differences of the prototype's transcription), level 0 against SceneLin.run(lanes=1, fold=False) bit for bit, the forward part against
CoreRT.rt_run_multisensor, FP32, the kernel alone against numpy, poisoned work buffers, blocked runs, the number of layer steps,
interactions and level calls the host issues, and the refusals."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ms_lin_oracle as MSL  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _err(got, ref):
    """max over levels, Stokes components and parameters of max |got - ref| relative to that component's max |ref| in the level."""
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


def _pair(vsm, arch, pol, l_trunc, S, L, rng, sza=40.0, vza=(30.0, 0.0, 55.0), vaz=(0.0, 60.0, 120.0), FT=np.float64, m_max=2,
          albedo=0.15, surface=None):
    """(host model, host lin, oracle model, oracle lin) of one column with one gas slot: Rayleigh in every layer (spectrally flat,
    so that every point sees the same doubling decisions as the whole batch), absorption varying over the points."""
    tau_rayl = np.tile(np.linspace(0.3, 0.6, L) / L, (S, 1))
    base = 10.0 ** rng.uniform(-4, 0, (S, 1)) * np.full((1, L), 1.0 / L)
    kw = dict(tau_rayl=tau_rayl, tau_abs=base, depol=0.0279, albedo=albedo, m_max=m_max)
    H = vsm.host_model
    pm = H.model_from_arrays(arch, pol, l_trunc, sza, list(vza), list(vaz), float_type=FT, surface=surface, **kw)
    om = O.build_model(pol, l_trunc, sza, list(vza), list(vaz), FT=np.float64, **kw)
    return pm, H.LinModel([base.copy()]), om, OL.LinModel([base.copy()])


def _sub(om, ol, idx):
    """The oracle scene restricted to the spectral points idx (points are independent; the decisions are the batch's)."""
    import dataclasses
    return (dataclasses.replace(om, tau_rayl=om.tau_rayl[idx], tau_abs=om.tau_abs[idx]),
            OL.LinModel([g[idx] for g in ol.tau_abs_dot]))


def _idx(S):
    return np.unique(np.r_[0, 1, S // 4, S // 2, S - 2, S - 1].clip(0, S - 1)) if S > 8 else np.arange(S)


CASES = [
    # (id, pol, l_trunc, S, Nz, levels, kwargs)
    ("c2lin_n60_iqu_sub0", "IQU", 35, 300, 40, [0, 1, 20, 39, 40], dict(vza=(30.0,), vaz=(0.0,))),
    ("scalar_n8", "I", 9, 5, 6, [3, 0, 6, 1], dict(m_max=3, vza=(30.0, 5.0), vaz=(0.0, 60.0))),
    ("iquv_n128", "IQUV", 57, 2, 3, [1, 2, 3, 0], dict(m_max=1, vza=(30.0, 5.0), vaz=(0.0, 60.0))),
    ("s1", "IQU", 9, 1, 5, [2, 4], dict(m_max=3)),
    ("s3_unsorted_duplicates", "IQU", 9, 3, 6, [5, 2, 5, 0, 2, 6, 1], dict(m_max=3)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_multisensor_lin_against_oracle_fp64(vsm, arch, case):
    name, pol, lt, S, L, levels, kw = case
    pm, pl, om, ol = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(len(name)), **kw)
    N = pm.quad_points.Nquad * pm.polarization_type.n
    uw, dw, uwd, dwd = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    assert N == {"c2lin": 60, "scalar": 8, "iquv": 128}.get(name.split("_")[0], N)
    if name.startswith("c2lin"):
        assert vsm.CoreRTLin.SceneLin(pm, pl, 0, 1, 1).sub0 is not None
    idx = _idx(S)
    ref = MSL.ms_lin_segmented(*_sub(om, ol, idx), levels)
    got = (uw, dw, uwd, dwd)
    per = [max(_err([g[i][..., idx, :] if g[i].ndim == 4 else g[i][..., idx]], [r[i]]) for g, r in zip(got, ref))
           for i in range(len(levels))]
    print("MS-lin %-24s N %3d S %4d levels %s: rel err %s" % (name, N, S, levels, " ".join("%.2e" % x for x in per)))
    assert max(per) <= 1e-8, (name, per)
    for i, l in enumerate(levels):
        assert uwd[i].shape == uw[i].shape + (2,) and all(np.all(np.isfinite(x[i])) for x in got)
        j = levels.index(l)                              # duplicates: the same arrays
        assert all(np.array_equal(x[i], x[j]) for x in got)


def test_multisensor_lin_two_aerosols_iquv(vsm, arch):
    """IQUV, two aerosols with derivative tables: 14 aerosol slots + a gas + the albedo."""
    from tests.test_gpu_optics import _lin_twin
    om, ol, pm, pl = _lin_twin(vsm, arch, 2, 1, S=3, L=5, pol="IQUV", l_trunc=9)
    levels = [0, 2, 3, 5]
    got = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 2, 1, 1, levels)
    assert got[2][0].shape[-1] == 16
    ref = MSL.ms_lin_segmented(om, ol, levels)
    e = max(_err(g, r) for g, r in zip(got, ref))
    assert e <= 1e-8, e


def test_multisensor_lin_coxmunk(vsm, arch):
    """Cox-Munk wind-speed slot.  The oracle takes the device's Fourier reflectance blocks and their wind-speed derivative
    (test_gpu_coxmunk.py checks them against the oracle's to ~1e-9, which the levels just above the surface would show undamped):
    here the level algebra is under test."""
    H = vsm.host_model
    hs = H.CoxMunkSurface(wind_speed=5.0)
    pm, pl, om, ol = _pair(vsm, arch, "IQU", 11, 4, 5, np.random.default_rng(2), surface=hs, m_max=3)
    levels = [0, 2, 4, 5]
    got = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, np.float64)
    th = vsm.Architectures.to_host

    def refl(m):
        rho, drho = vsm.CoreRT.reflectance(hs, dq, m, arch, np.float64, deriv=True)
        return th(rho).T.copy(), th(drho).T.copy()
    ref = MSL.ms_lin_segmented(om, ol, levels, surface=refl)
    e = max(_err(g, r) for g, r in zip(got, ref))
    assert e <= 1e-8, e
    assert np.abs(got[2][1][..., 1]).max() > 0       # the wind-speed slot reaches the interior levels


@pytest.mark.parametrize("S,lt,sub0", [(300, 35, True), (3, 9, False)])
def test_level0_is_scene_lin_run_bit_for_bit(vsm, arch, S, lt, sub0):
    pm, pl, _, _ = _pair(vsm, arch, "IQU", lt, S, 8, np.random.default_rng(4), vza=(30.0,), vaz=(0.0,))
    uw, dw, uwd, dwd = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, [3, 0, 8])
    sc = vsm.CoreRTLin.SceneLin(pm, pl, 0, 1, 1)
    assert (sc.sub0 is not None) == sub0
    sc.run(lanes=1, fold=False)
    torch.cuda.synchronize()
    R, T, Rd, Td = sc.results_host()
    for a, b in ((uw[1], R), (dw[1], T), (uwd[1], Rd), (dwd[1], Td)):
        assert np.array_equal(a, b)
    R2, T2, Rd2, Td2 = vsm.CoreRTLin.rt_run_lin(pm, pl, 0, 1, 1)          # the default lanes / folded walk: to rounding
    for a, b in ((uw[1], R2), (dw[1], T2), (uwd[1], Rd2), (dwd[1], Td2)):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def test_forward_part_is_rt_run_multisensor(vsm, arch):
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 35, 300, 40, np.random.default_rng(6), vza=(30.0,), vaz=(0.0,))
    levels = [0, 1, 20, 39, 40]
    uw, dw, _, _ = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    ue, de = vsm.CoreRT.rt_run_multisensor(pm, levels)
    assert max(_err(uw, ue), _err(dw, de)) <= 1e-12


@pytest.mark.parametrize("pol,lt", [("I", 9), ("IQU", 33)])
def test_multisensor_lin_fp32(vsm, arch, pol, lt):
    """Float32 model (the linearized walk keeps its FP64-on-FP32-storage kernels, the level kernels run in FP32) against the FP64
    oracle at twice the gate of test_gpu_lin.test_rt_run_lin_fp32 (1e-2)."""
    pm, pl, om, ol = _pair(vsm, arch, pol, lt, 3, 5, np.random.default_rng(8), FT=np.float32)
    levels = [0, 2, 4, 5]
    got = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    assert got[0][0].dtype == np.float32 and got[2][0].dtype == np.float32
    ref = MSL.ms_lin_segmented(om, ol, levels)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))      # test_gpu_lin._rel, per level and parameter slot
    e = max(max(rel(g[i], r[i]) for g, r in zip(got[:2], ref[:2])) for i in range(len(levels)))
    e = max(e, max(rel(g[i][..., p], r[i][..., p]) for g, r in zip(got[2:], ref[2:]) for i in range(len(levels)) for p in range(2)))
    print("MS-lin fp32 %s: %.2e" % (pol, e))
    assert e < 2e-2, e


# ---- the kernel alone --------------------------------------------------------------------------------------------------------
def _kernel_inputs(N, S, rng, shared):
    """The signature of level_cases.contractive (which scales by 0.6 / N and draws a before B)."""
    A = 0.9 * rng.uniform(0, 1, (S, N, N)) / N
    B = 0.9 * rng.uniform(0, 1, (1 if shared else S, N, N)) / N
    a, c = rng.uniform(0, 1, (S, N)), rng.uniform(0, 1, (S, N))
    return A, a, B, c


def _kernel_case(vsm, N, P, P_top, shared, S=3, FT=np.float64, ns=3, seed=0, nV=2, inputs=_kernel_inputs):
    rng = np.random.default_rng(seed + N + 7 * P)
    ns = ns if N % ns == 0 else 1
    A, a, B, c = inputs(N, S, rng, shared)
    Ad = rng.normal(0, 1, (P_top, S, N, N)) / N
    ad = rng.normal(0, 1, (P_top, S, N))
    Bd = rng.normal(0, 1, (P,) + B.shape) / N
    cd = rng.normal(0, 1, (P, S, N))
    Adz = np.concatenate([Ad, np.zeros((P - P_top, S, N, N))]) if P > P_top else Ad
    adz = np.concatenate([ad, np.zeros((P - P_top, S, N))]) if P > P_top else ad
    uw, dw, uwd, dwd = MSL.level_lin_push_through(np.float64, A, a, B, c, Adz, adz, Bd, cd)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64 if FT == np.float64 else torch.float32, device="cuda")
    sw = lambda M: np.swapaxes(M, -1, -2)                # math order -> the column-major layout
    row0 = (C.c_int * nV)(0, N - ns, *[ns * (v % (N // ns)) for v in range(2, nV)])
    ct = C.c_double if FT == np.float64 else C.c_float
    wv = rng.uniform(0.5, 1.5, nV * ns)
    w = (ct * (nV * ns))(*wv)
    init_u, init_d = rng.normal(0, 1, (P, S, ns, nV)), rng.normal(0, 1, (P, S, ns, nV))
    t = dict(A=dev(sw(A)), B=dev(sw(B)), dwf=dev(dw), uwf=dev(uw), Ad=dev(sw(Ad)) if P_top else None,
             ad=dev(ad) if P_top else None, Bd=dev(sw(Bd)), cd=dev(cd), uwd=dev(init_u), dwd=dev(init_d),
             dwdf=dev(np.full((P, S, N), np.nan)), uwdf=dev(np.full((P, S, N), np.nan)))
    p_ = lambda x: None if x is None else x.data_ptr()
    NN = N * N
    bstride = 0 if shared and S > 1 else NN
    vsm._lib.call("vsm_level_radiance_lin", t["A"].dtype, N, ns, S, P, P_top, nV, row0, w, p_(t["A"]), p_(t["B"]), bstride,
                  p_(t["dwf"]), p_(t["uwf"]), p_(t["Ad"]), S * NN, p_(t["ad"]), p_(t["Bd"]), bstride, B.shape[0] * NN, p_(t["cd"]),
                  p_(t["uwd"]), p_(t["dwd"]), p_(t["dwdf"]), p_(t["uwdf"]), None)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_radiance_lin test")
    h = lambda x: x.double().cpu().numpy()
    ref_u, ref_d = init_u.copy(), init_d.copy()
    for v in range(nV):
        for k in range(ns):
            ref_u[:, :, k, v] += wv[v + nV * k] * uwd[:, :, row0[v] + k]
            ref_d[:, :, k, v] += wv[v + nV * k] * dwd[:, :, row0[v] + k]
    return (h(t["uwdf"]), h(t["dwdf"]), h(t["uwd"]), h(t["dwd"])), (uwd, dwd, ref_u, ref_d)


@pytest.mark.parametrize("N,P,P_top,shared", [(4, 1, 0, False), (21, 3, 2, True), (60, 17, 16, False), (64, 64, 63, True),
                                              (96, 3, 3, False), (128, 1, 1, True), (128, 13, 12, False), (128, 64, 60, True)])
def test_level_kernel_lin_vs_numpy(vsm, N, P, P_top, shared):
    """N in {4, 21, 60, 64, 96, 128}, P in {1, 3, 17, 64}, P_top < P, a shared bottom (stride 0); FP64 at N = 128 takes 12
    parameters per chunk: P = 13 is just above one chunk."""
    got, ref = _kernel_case(vsm, N, P, P_top, shared)
    for g, r in zip(got, ref):
        assert np.all(np.isfinite(g)) and np.abs(g - r).max() <= 1e-11 * np.abs(r).max(), (N, P)


def test_level_kernel_lin_vs_numpy_many_angles(vsm):
    """70 viewing angles: more than the 64 one launch carries (derivative vectors in full, then vsm_postprocess_vza_lin)."""
    got, ref = _kernel_case(vsm, 21, 3, 2, True, nV=70)
    for g, r in zip(got, ref):
        assert np.all(np.isfinite(g)) and np.abs(g - r).max() <= 1e-11 * np.abs(r).max()


@pytest.mark.parametrize("N,P", [(60, 17), (128, 40)])
def test_level_kernel_lin_vs_numpy_fp32(vsm, N, P):
    got, ref = _kernel_case(vsm, N, P, P - 1, False, FT=np.float32)
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 2e-4 * np.abs(r).max(), (N, P, np.abs(g - r).max() / np.abs(r).max())


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_outputs_finite_with_poisoned_work(vsm, arch, monkeypatch):
    """VSM_POISON_WORK fills every work buffer with NaN (and the LDS holds NaNs before every GPU test)."""
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 21, 16, 10, np.random.default_rng(9))
    res = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, [0, 3, 7, 10])
    for xs in res:
        for x in xs:
            assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0


@pytest.mark.parametrize("S,max_points", [(7, 3), (140, 64)])
def test_blocked_runs_are_bit_identical(vsm, arch, S, max_points):
    """7 points in blocks of 3, 3, 1; 140 points (the m = 0 sub-scene applies) in blocks of 64 and 76 (a tail shorter than
    SceneLin.LANE_POINTS joins the block before it: every block takes the sub-scene, as the one-pass run does)."""
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, S, 6, np.random.default_rng(10), m_max=3)
    levels = [4, 0, 6, 2]
    one = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True)
    blk = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True, max_points=max_points)
    for name in ("uw", "dw", "uw_dot", "dw_dot"):
        assert all(np.array_equal(a, b) for a, b in zip(getattr(one, name), getattr(blk, name))), name
    for name in ("uw_streams", "dw_streams", "uw_dot_streams", "dw_dot_streams"):
        for la, lb in zip(getattr(one, name), getattr(blk, name)):
            assert all(np.array_equal(a, b) for a, b in zip(la, lb)), name
    assert one.uw_dot_streams[0][0].shape == (pm.quad_points.Nquad * 3, 1, S, 2)


def test_streams_match_the_oracle(vsm, arch):
    pm, pl, om, ol = _pair(vsm, arch, "IQU", 9, 3, 5, np.random.default_rng(12), m_max=2)
    levels = [0, 2, 5]
    res = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True)
    full = {}
    MSL.ms_lin_segmented(om, ol, levels, full=full)
    for i, l in enumerate(levels):
        for m in range(3):
            u, d, ud, dd = full[(l, m)]
            for got, ref in ((res.uw_streams[i][m][:, 0].T, u), (res.dw_streams[i][m][:, 0].T, d),
                             (res.uw_dot_streams[i][m][:, 0].transpose(2, 1, 0), ud),
                             (res.dw_dot_streams[i][m][:, 0].transpose(2, 1, 0), dd)):
                assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (l, m)


def test_layer_steps_interactions_and_level_calls(vsm, arch, monkeypatch):
    """Per moment: Nz + (Nz - l_1) linearized layer steps, L + 1 linearized interactions beyond those of the layer steps, one
    elastic and one linearized level call per level other than 0."""
    CL, MS, MSLIN = vsm.CoreRTLin, vsm.core_rt_ms, vsm.core_rt_ms_lin
    counts = dict(steps=0, inter=0, lev=0, levlin=0)

    def wrap(mod, name, key):
        f = getattr(mod, name)

        def g(*args, **kw):
            counts[key] += 1
            return f(*args, **kw)
        monkeypatch.setattr(mod, name, g)
    wrap(CL, "doubling_allparams_", "steps")
    wrap(CL, "interaction_lin_", "inter")
    wrap(MS, "level_radiance_", "lev")
    wrap(MSLIN, "level_radiance_lin_", "levlin")
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, 4, 12, np.random.default_rng(1), m_max=3)
    nm, Nz = pm.m_max + 1, 12
    levels = [0, 4, 9, 12]
    vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    L, l1 = 2, 4
    steps = Nz + (Nz - l1)
    copies = 1 + L
    assert counts == dict(steps=steps * nm, inter=(steps - copies + L + 1) * nm, lev=3 * nm, levlin=3 * nm), counts


def test_refusals(vsm, arch):
    H = vsm.host_model
    pm, pl, _, _ = _pair(vsm, arch, "I", 9, 2, 4, np.random.default_rng(3))
    B = np.full((2, 4), 0.1)
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=B))
    with pytest.raises(vsm.VSMError, match="SolarBeam"):
        vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, [1])
    tr = np.tile(np.full(4, 0.05), (2, 1))
    tr[:, 2] = 0.0
    g = np.full((2, 4), 1e-3)
    pm = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, tau_abs=g, albedo=0.2, m_max=1)
    with pytest.raises(NotImplementedError, match="does not scatter"):
        vsm.CoreRTLin.rt_run_multisensor(pm, H.LinModel([g]), 0, 1, 1, [1])
    pm, pl, _, _ = _pair(vsm, arch, "IQUV", 61, 2, 3, np.random.default_rng(3))
    assert pm.quad_points.Nquad * 4 > 128
    with pytest.raises(vsm.VSMError, match="128"):
        vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, [1])
