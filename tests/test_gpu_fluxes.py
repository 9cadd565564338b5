"""GPU tests of the flux run (vsm.CoreRT.rt_run_fluxes, core_rt_flux.py) and its level kernel (vsm_level_flux_*,
csrc/vsm_level.hip): the kernel against numpy and against its operator-level composition, the driver against the float64
oracle (tests/flux_oracle.py) and against the quadrature of rt_run_multisensor's own level vectors, thermal emission, SurfaceSIF,
conservation over all levels, Float32, blocks of the spectral axis, the library calls the host issues, poisoned work buffers and
the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import flux_oracle as FO  # noqa: E402
import ms_oracle as MS  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from level_cases import contractive  # noqa: E402
from test_gpu_multisensor import _err_per_level, _pair, _sub  # noqa: E402

pytestmark = pytest.mark.gpu

QUANTITIES = ("up", "down_diffuse", "down_direct", "actinic_up", "actinic_down_diffuse", "actinic_direct", "net_down")


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _rel(got, ref):
    """max |got - ref| relative to the largest |ref| (one quantity, all its levels and points)."""
    sc = float(np.max(np.abs(ref)))
    e = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)))
    return e / sc if sc > 0 else e


def _worst(res, ref, points=None):
    out = {}
    for k in QUANTITIES:
        g = getattr(res, k)
        out[k] = _rel(g if points is None else g[:, points], getattr(ref, k))
    if ref.absorbed is not None:
        sc = float(np.max(np.abs(ref.net_down)))
        pick = (lambda x: x) if points is None else (lambda x: x[..., points])
        out["absorbed"] = float(np.max(np.abs(pick(res.absorbed) - ref.absorbed))) / sc
        out["surface_absorbed"] = float(np.max(np.abs(pick(res.surface_absorbed) - ref.surface_absorbed))) / sc
    return out


# ---- the kernel on random inputs -------------------------------------------------------------------------------------------------
def _kernel_case(vsm, N, FT, S, shared, rng, inputs=contractive):
    H = vsm.host_model
    pol = H.polarization_type("IQU" if N % 3 == 0 else "I")
    dt = torch.float64 if FT == np.float64 else torch.float32
    dev = torch.device("cuda", 0)
    rnd = lambda x: np.asarray(x, dtype=FT).astype(np.float64)           # (the reference sees the inputs the device sees)
    A, _, B, _ = inputs(N, S, rng, shared)
    A, B = rnd(A), rnd(B)
    a, c = rnd(rng.random((4, S, N))), rnd(rng.random((4, S, N)))
    Nq = N // pol.n
    q, dir_h = rnd(rng.random((4, Nq))), rnd(rng.random(4))
    tau, F0 = rnd(rng.random(S) * 2), rnd(0.5 + rng.random(S))
    lay = lambda X: torch.tensor(np.ascontiguousarray(X.transpose(0, 2, 1)), dtype=dt, device=dev)
    vec = lambda x: torch.tensor(x, dtype=dt, device=dev)
    vecs = [MS.level_push_through(np.float64, A, a[k], B, c[k]) for k in range(4)]      # (uw_k, dw_k), computed once
    host = dict(A=A, B=B, a=a, c=c, q=q, dir_h=dir_h, tau=tau, F0=F0, vecs=vecs, mu0=float(rnd(0.7)))
    devt = dict(A=lay(A), B=lay(B), a=[vec(x) for x in a], c=[vec(x) for x in c], q=vec(q), tau=vec(tau), F0=vec(F0))
    return pol, dt, dev, host, devt


def _kernel_reference(pol, host, K, nW, top, direct):
    S = host["tau"].shape[0]
    uw = sum(host["vecs"][k][0] for k in range(K)) if top else sum(host["c"][k] for k in range(K))
    dw = sum(host["vecs"][k][1] for k in range(K)) if top else np.zeros_like(uw)
    q = host["q"][:nW]
    ref = np.zeros((3, nW, S))
    ref[0] = (uw[:, ::pol.n] @ q.T).T
    ref[1] = (dw[:, ::pol.n] @ q.T).T
    if direct:
        ref[2] = host["dir_h"][:nW, None] * (host["F0"] * np.exp(-host["tau"] / host["mu0"]))[None, :]
    return ref


@pytest.mark.parametrize("N", [8, 21, 60, 128])
@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_flux_kernel(vsm, N, FT):
    """vsm_level_flux_* against its operator-level composition (the bound of test_level_kernel_fused_vs_oplevel: 1e-12 / 2e-5 of
    the largest reference value) and against numpy (ten times that): n_src and nW in {1, 2, 4}, shared and per-point bottoms,
    with and without the direct term, with and without a top.  The outputs start as NaN: written, not accumulated."""
    FL = vsm.core_rt_flux
    S = 7
    rng = np.random.default_rng(N)
    tol = 1e-12 if FT == np.float64 else 2e-5
    worst = [0.0, 0.0]
    for shared in (False, True):
        pol, dt, dev, host, d = _kernel_case(vsm, N, FT, S, shared, rng)
        for K in (1, 2, 4):
            for nW in (1, 2, 4):
                for top, direct in ((True, True), (True, False), (False, True)) if (K, nW) != (2, 2) else ((True, True), (True, False),
                                                                                                     (False, True), (False, False)):
                    outs = []
                    for op in (False, True):
                        out = torch.full((3, nW, S), float("nan"), dtype=dt, device=dev)
                        FL.level_flux_(pol, d["A"] if top else None, d["a"][:K] if top else None, d["B"] if top else None, d["c"][:K],
                                       d["q"][:nW].contiguous(), host["dir_h"][:nW], host["mu0"], d["tau"] if direct else None,
                                       d["F0"] if direct else None, out, oplevel=op)
                        torch.cuda.synchronize()
                        outs.append(out.cpu().numpy().astype(np.float64))
                    ref = _kernel_reference(pol, host, K, nW, top, direct)
                    assert np.all(np.isfinite(outs[0])) and np.all(np.isfinite(outs[1])), (N, K, nW, top, direct, shared)
                    if not top:
                        assert np.all(outs[0][1] == 0)
                    if not direct:
                        assert np.all(outs[0][2] == 0) and np.all(outs[1][2] == 0)
                    sc = float(np.max(np.abs(ref[:2])))
                    e_op = float(np.max(np.abs(outs[0] - outs[1]))) / sc
                    e_np = float(np.max(np.abs(outs[0] - ref))) / sc
                    worst = [max(worst[0], e_op), max(worst[1], e_np)]
                    assert e_op <= tol and e_np <= 10 * tol, (N, K, nW, top, direct, shared, e_op, e_np)
    vsm._lib.check_device_status("level flux kernel")
    print("level_flux N %3d %s: fused vs composition %.2e, vs numpy %.2e" % (N, np.dtype(FT).name, worst[0], worst[1]))


def test_level_flux_kernel_is_deterministic_in_place(vsm):
    """The order of the additions is fixed: a point gives the same bits wherever it stands in the batch."""
    FL = vsm.core_rt_flux
    N, S = 60, 7
    pol, dt, dev, host, d = _kernel_case(vsm, N, np.float64, S, False, np.random.default_rng(3))
    run = lambda idx: _flux_call(FL, pol, d, host, idx, dt, dev)
    whole = run(list(range(S)))
    perm = [4, 0, 6, 2, 5, 1, 3]
    moved = run(perm)
    assert np.array_equal(moved, whole[:, :, perm])
    assert np.array_equal(run([5]), whole[:, :, [5]])


def _flux_call(FL, pol, d, host, idx, dt, dev):
    ix = torch.as_tensor(idx, device=dev)
    out = torch.full((3, 2, len(idx)), float("nan"), dtype=dt, device=dev)
    FL.level_flux_(pol, d["A"][ix].contiguous(), [x[ix].contiguous() for x in d["a"][:2]], d["B"][ix].contiguous(),
                   [x[ix].contiguous() for x in d["c"][:2]], d["q"][:2].contiguous(), host["dir_h"][:2], host["mu0"],
                   d["tau"][ix].contiguous(), d["F0"][ix].contiguous(), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_flux_kernel_refuses_bad_arguments(vsm, FT):
    """Every argument error returns VSM_ERR_INVALID_ARG before any launch (the NaN-filled output stays); S = 0 is no error."""
    CR = vsm.CoreRT
    N, S, K, nW = 16, 3, 2, 2
    pol, dt, dev, host, d = _kernel_case(vsm, N, FT, S, False, np.random.default_rng(0))
    out = torch.full((3, 4, S), float("nan"), dtype=dt, device=dev)
    ctype = C.c_double if FT == np.float64 else C.c_float
    P = CR._ptr
    pa = (C.c_void_p * 5)(*[P(d["a"][k % 4]) for k in range(5)])
    pc = (C.c_void_p * 5)(*[P(d["c"][k % 4]) for k in range(5)])
    dh = (ctype * 4)(*[1.0] * 4)
    fn = getattr(vsm._lib.lib(), "vsm_level_flux_" + ("f64" if FT == np.float64 else "f32"))
    good = dict(N=N, ns=pol.n, S=S, A=P(d["A"]), K=K, a=pa, B=P(d["B"]), bs=N * N, c=pc, nW=nW, q=P(d["q"]), dh=dh, mu0=0.7,
                tau=P(d["tau"]), F0=P(d["F0"]), out=P(out))

    def call(**kw):
        g = dict(good, **kw)
        return fn(g["N"], g["ns"], g["S"], g["A"], g["K"], g["a"], g["B"], g["bs"], g["c"], g["nW"], g["q"], g["dh"],
                  ctype(g["mu0"]), g["tau"], g["F0"], g["out"], CR._stream_ptr())
    INVALID = 1          # VSM_ERR_INVALID_ARG
    bad = [dict(N=129), dict(N=0), dict(K=0), dict(K=5), dict(nW=0), dict(nW=5), dict(S=-1), dict(ns=3), dict(bs=7), dict(q=None),
           dict(out=None), dict(c=None), dict(a=None), dict(B=None), dict(tau=None), dict(F0=None), dict(dh=None), dict(mu0=0.0)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert vsm._lib.lib().vsm_last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(out)))
    assert call(S=0) == 0 and call(S=0, q=None, out=None, c=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(out)))
    assert call(K=4, nW=4) == 0                                # the largest counts the kernel takes
    assert call(A=None, a=None, B=None, tau=None, F0=None, dh=None) == 0      # no top, no direct term
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level flux kernel")
    assert bool(torch.all(torch.isfinite(out[:, :nW])))
    with pytest.raises(vsm.VSMError, match="n_src"):
        vsm.core_rt_flux.level_flux_(pol, d["A"], d["a"] + d["a"][:1], d["B"], d["c"] + d["c"][:1], d["q"][:2].contiguous(), [1, 1],
                                     0.7, None, None, out)


# ---- the driver against the oracle -----------------------------------------------------------------------------------------------
CASES = [
    # (id, pol, l_trunc, S, Nz, levels (None: all), kwargs)
    ("scalar_n8_unsorted_duplicates", "I", 10, 5, 6, [3, 0, 6, 1, 3, 6], dict(m_max=3, vza=(30.0,), vaz=(0.0,))),
    ("iqu_n27_all_levels", "IQU", 9, 3, 5, None, dict(m_max=3)),
    ("iqu_n60_native_walk", "IQU", 35, 64, 6, None, dict(m_max=1, vza=(30.0,), vaz=(0.0,))),
    ("iquv_n112_aerosols", "IQUV", 50, 3, 5, None, dict(aerosols=True, m_max=1, vza=(30.0,), vaz=(0.0,))),
    ("scalar_n135_composition", "I", 264, 2, 4, None, dict(m_max=1)),
    ("s1", "IQU", 9, 1, 5, [2, 0, 5], dict(m_max=2)),
]


def _rt_run_deviation(vsm, pm, om_sub, idx, oracle_RT=None):
    R, T = vsm.CoreRT.rt_run(pm)
    Ro, To = O.rt_run(om_sub) if oracle_RT is None else oracle_RT
    return max(_err_per_level([R[..., idx]], [Ro]), _err_per_level([T[..., idx]], [To]))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fluxes_against_oracle_fp64(vsm, arch, case):
    """Per quantity, relative to its largest value over the levels: max(1e-10, 2 e_rt), e_rt rt_run's own deviation from O.rt_run on
    the scene (the rule of test_multisensor_against_prototype_fp64)."""
    name, pol, lt, S, L, levels, kw = case
    pm, om = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(len(name)), **kw)
    N = pm.quad_points.Nquad * pm.polarization_type.n
    assert N > 128 if name.startswith("scalar_n135") else "_n%d_" % N in name or name == "s1"
    res = vsm.CoreRT.rt_run_fluxes(pm, levels)
    lv = list(range(L + 1)) if levels is None else levels
    assert res.levels == lv and res.up.shape == (len(lv), S) and res.up.dtype == np.float64
    idx = np.unique(np.r_[0, 1, S // 4, S // 2, S - 2, S - 1].clip(0, S - 1)) if S > 8 else np.arange(S)
    oms = _sub(om, idx)
    ref = FO.fluxes_reference(oms, lv)
    errs = _worst(res, ref, idx)
    e_rt = _rt_run_deviation(vsm, pm, oms, idx)
    print("FLUX %-30s N %3d S %3d: %s (rt_run %.2e)" % (name, N, S, " ".join("%s %.1e" % kv for kv in errs.items()), e_rt))
    assert max(errs.values()) <= max(1e-10, 2 * e_rt), (name, errs, e_rt)
    for k in QUANTITIES:
        assert np.all(np.isfinite(getattr(res, k)))
    for i, l in enumerate(lv):
        j = lv.index(l)                                  # duplicates: the same rows
        assert all(np.array_equal(getattr(res, k)[i], getattr(res, k)[j]) for k in QUANTITIES)
        if l == 0:
            assert np.all(res.down_diffuse[i] == 0) and np.all(res.actinic_down_diffuse[i] == 0)
            np.testing.assert_allclose(res.down_direct[i], float(pm.quad_points.mu0), rtol=1e-15)
    assert np.array_equal(res.net_down, res.down_direct + res.down_diffuse - res.up)
    if levels is None:
        assert res.absorbed.shape == (L, S) and res.surface_absorbed.shape == (S,)
        np.testing.assert_allclose(res.absorbed.sum(0) + res.surface_absorbed + res.up[0], float(pm.quad_points.mu0), rtol=1e-12)
    else:
        assert res.absorbed is None and res.surface_absorbed is None


def _sibling_quadrature(pm, ms, levels):
    """The quantities of rt_run_fluxes from rt_run_multisensor(..., streams=True)'s m = 0 level vectors, in float64, level 0 by the
    rule of the flux run (its uw; no diffuse field enters the TOA)."""
    qp = pm.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    n = pm.polarization_type.n
    rows = {k: [] for k in ("up", "down_diffuse", "actinic_up", "actinic_down_diffuse")}
    assert ms.weight[0] == 0.5 / math.pi
    for i, l in enumerate(levels):
        uw = ms.uw_streams[i][0][::n, 0, :].astype(np.float64)          # [Nquad, S]
        dw = ms.dw_streams[i][0][::n, 0, :].astype(np.float64) * (0.0 if l == 0 else 1.0)
        rows["up"].append((mu * w) @ uw)
        rows["down_diffuse"].append((mu * w) @ dw)
        rows["actinic_up"].append(w @ uw)
        rows["actinic_down_diffuse"].append(w @ dw)
    return {k: np.array(v) for k, v in rows.items()}


@pytest.mark.parametrize("kind", ["m_max_3", "surface_sif", "solar_thermal", "all_sources"])
def test_fluxes_against_the_multisensor_run(vsm, arch, kind):
    """Every diffuse quantity is the float64 quadrature of rt_run_multisensor(..., streams=True)'s own m = 0 level vectors (1e-11
    of its largest value: ten times the kernel's bound against its composition); m_max does not enter; SurfaceSIF and the thermal
    slot are carried as there.  down_diffuse at level Nz is the quadrature of the sibling's level-0 dw (rt_run's T).
    all_sources: SolarBeam + ThermalEmission + SurfaceEmission + SurfaceSIF on levels [2, 0, Nz, 2] -- the one mix in which every
    source list the walk hands the flux run carries two entries and the surface layer emits in both slots (l_trunc 9: N = 27)."""
    H = vsm.host_model
    S, L = 4, 5
    pm, om = _pair(vsm, arch, "IQU", 9 if kind == "all_sources" else 13, S, L, np.random.default_rng(21), m_max=3, albedo=0.2)
    thermal = kind in ("solar_thermal", "all_sources")
    levels = list(range(L + 1))
    if kind == "all_sources":
        B = 0.05 + 0.1 * np.random.default_rng(23).random((L, S))
        pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=B), H.SurfaceEmission(B_surface=0.1 + 0.1 * np.arange(S)),
                      H.SurfaceSIF(0.02 + 0.03 * np.random.default_rng(22).random(S)))
        levels = [2, 0, L, 2]
    elif kind == "surface_sif":
        sif = 0.02 + 0.03 * np.random.default_rng(22).random(S)
        pm.sources = (H.SolarBeam(), H.SurfaceSIF(sif))
    elif thermal:
        B = 0.05 + 0.1 * np.random.default_rng(23).random((L, S))
        pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=B))
    res = vsm.CoreRT.rt_run_fluxes(pm, levels, thermal=thermal)
    ms = vsm.CoreRT.rt_run_multisensor(pm, levels, streams=True, thermal=thermal)
    want = _sibling_quadrature(pm, ms, levels)
    errs = {k: _rel(getattr(res, k), v) for k, v in want.items()}
    print("FLUX vs multisensor (%s): %s" % (kind, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-11, errs
    qp = pm.quad_points
    t_bottom = (np.asarray(qp.qp_mu, dtype=np.float64) * np.asarray(qp.wt_mu, dtype=np.float64)) @ \
        ms.dw_streams[levels.index(0)][0][::pm.polarization_type.n, 0, :].astype(np.float64)
    assert _rel(res.down_diffuse[levels.index(L)], t_bottom) <= 1e-11 and np.max(np.abs(t_bottom)) > 0
    if kind == "m_max_3":
        import dataclasses
        r0 = vsm.CoreRT.rt_run_fluxes(dataclasses.replace(pm, m_max=0), levels)
        assert all(np.array_equal(getattr(r0, k), getattr(res, k)) for k in QUANTITIES)
    if kind == "surface_sif":      # the emission is part of every level
        pm.sources = None
        plain = vsm.CoreRT.rt_run_fluxes(pm, levels)
        assert np.min(res.up - plain.up) > 0 and np.min(res.down_diffuse[1:] - plain.down_diffuse[1:]) > 0
        assert np.array_equal(res.down_direct, plain.down_direct)


# ---- thermal emission ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solar", [True, False], ids=["solar+thermal", "thermal_only"])
@pytest.mark.parametrize("pol,lt", [("I", 10), ("IQU", 9)], ids=["scalar_n8", "iqu_n27"])
def test_fluxes_thermal_against_oracle(vsm, arch, pol, lt, solar):
    """max(1e-9, 2 e_rt): test_multisensor_thermal_against_oracle_fp64's bound (1e-9 is rt_run's thermal slot against the oracle)."""
    H = vsm.host_model
    S, L = 3, 5
    views = dict(vza=(30.0,), vaz=(0.0,)) if pol == "I" else {}          # (one view: N = 8; three: N = 27)
    pm, om = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(31), m_max=2, **views)
    assert pm.quad_points.Nquad * pm.polarization_type.n == (8 if pol == "I" else 27)
    B = 0.05 + 0.1 * np.random.default_rng(32).random((L, S))
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=B)) if solar else (H.ThermalEmission(B_layer=B),)
    levels = [2, 0, 5, 1, 4, 3]
    res = vsm.CoreRT.rt_run_fluxes(pm, levels, thermal=True)
    ref = FO.fluxes_reference(om, levels, B_layer=B, solar=solar)
    only_solar = FO.fluxes_reference(om, levels, solar=solar)
    assert np.min(ref.up - only_solar.up) > 0            # the slot is part of every level
    import dataclasses
    oms = om if solar else dataclasses.replace(om, F0=np.zeros((om.pol.n, S), dtype=om.FT))
    Rs, Ts = O.rt_run(oms)
    Rt, Tt = O.rt_run_thermal(om, B)
    e_rt = _rt_run_deviation(vsm, pm, None, np.arange(S), oracle_RT=(Rs + Rt, Ts + Tt))
    errs = _worst(res, ref)
    print("FLUX-TH %s %s: %s (rt_run %.2e)" % (pol, "solar+thermal" if solar else "thermal_only",
                                               " ".join("%s %.1e" % kv for kv in errs.items()), e_rt))
    assert max(errs.values()) <= max(1e-9, 2 * e_rt), (errs, e_rt)
    assert res.absorbed is not None and res.absorbed.shape == (L, S)
    if not solar:
        assert np.all(res.down_direct == 0) and np.all(res.actinic_direct == 0)


def test_opaque_isothermal_column_on_device(vsm, arch):
    """The T-A7 bound on the device: pi B up and down, 2 pi B actinic, at the interior levels."""
    from test_oracle_multisensor_thermal import opaque_isothermal_column
    H = vsm.host_model
    kw, geo, B = opaque_isothermal_column()
    pm = H.model_from_arrays(arch, *geo, sources=(H.ThermalEmission(B_layer=B),), **kw)
    L = B.shape[0]
    res = vsm.CoreRT.rt_run_fluxes(pm, list(range(1, L)), thermal=True)
    for x, f in ((res.up, 1), (res.down_diffuse, 1), (res.actinic_up, 2), (res.actinic_down_diffuse, 2)):
        assert np.max(np.abs(x / (f * math.pi * B[0][None, :]) - 1)) <= 1e-3
    assert np.all(res.down_direct == 0)


# ---- conservation, Float32, blocks, calls, work buffers, refusals --------------------------------------------------------------------
def test_conservative_column_on_device_all_levels(vsm, arch):
    from test_oracle_multisensor import conservative_model
    om, _ = conservative_model()
    L = om.tau_rayl.shape[1]
    pm = vsm.host_model.model_from_arrays(arch, "I", 15, 40.0, [30.0], [0.0], tau_rayl=om.tau_rayl, depol=0.0, albedo=0.3, m_max=0)
    res = vsm.CoreRT.rt_run_fluxes(pm)
    assert res.levels == list(range(L + 1))
    ref = FO.fluxes_reference(om, res.levels)
    spread = lambda r: float(np.max(np.max(r.net_down, axis=0) - np.min(r.net_down, axis=0))) / float(om.quad_points.mu0)
    print("net_down spread / (mu0 F0), levels 0..Nz: device %.3e oracle %.3e" % (spread(res), spread(ref)))
    assert 0 < spread(res) <= 2 * spread(ref)
    # nothing is absorbed in the column: what enters leaves again or goes into the surface
    assert np.max(np.abs(res.absorbed)) <= 2 * spread(ref) * float(om.quad_points.mu0)


def test_fluxes_float32(vsm, arch):
    """The bound of test_multisensor_float32 (2e-3), per quantity relative to its largest value."""
    pm, om32 = _pair(vsm, arch, "IQU", 35, 5, 8, np.random.default_rng(4), FT=np.float32, m_max=1, vza=(30.0,), vaz=(0.0,))
    assert pm.quad_points.Nquad * 3 == 60
    res = vsm.CoreRT.rt_run_fluxes(pm)
    assert res.up.dtype == np.float32 and res.absorbed.dtype == np.float32
    ref = FO.fluxes_reference(O.exact_model(om32), res.levels)
    errs = {k: _rel(getattr(res, k), getattr(ref, k)) for k in QUANTITIES}
    print("FLUX f32: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 2e-3, errs


def test_blocks_of_the_spectral_axis(vsm, arch):
    """max_points = 4 on 10 points (blocks of 4, 4, 2) against one pass: within 1e-12 of the largest value, and -- the stronger of
    the two statements, which is the one that holds -- the same bits: ndoubl and the interface tags are batch-global, both runs
    land on the same kernels, and a point's arithmetic does not depend on its place in the batch."""
    pm, _ = _pair(vsm, arch, "IQU", 17, 10, 6, np.random.default_rng(8), m_max=2)
    one = vsm.CoreRT.rt_run_fluxes(pm)
    blk = vsm.CoreRT.rt_run_fluxes(pm, max_points=4)
    fields = QUANTITIES + ("absorbed", "surface_absorbed")
    e = max(float(np.max(np.abs(getattr(blk, k) - getattr(one, k)))) / float(np.max(np.abs(one.down_direct))) for k in fields)
    print("blocks vs one pass: %.2e" % e)
    assert e <= 1e-12
    for k in fields:
        assert np.array_equal(getattr(blk, k), getattr(one, k)), k


def test_layer_steps_and_interactions(vsm, arch, monkeypatch):
    """All levels: Nz + (Nz - 1) layer steps (the top pass, one one-layer segment per interior level) and Nz interactions (Nz - 1
    bottoms, the surface step of level 0).  levels = [0]: Nz layer steps and one interaction.  Neither depends on m_max."""
    CR = vsm.CoreRT
    counts = dict(steps=0, inter=0)

    def wrap(name, n_of):
        f = getattr(CR, name)

        def g(*args, **kw):
            counts["inter" if name == "interaction_" else "steps"] += n_of(args)
            return f(*args, **kw)
        monkeypatch.setattr(CR, name, g)
    wrap("run_layer_native_", lambda a: int(a[1]))
    wrap("layer_forward_", lambda a: 1)
    wrap("layer_forward_multi_", lambda a: len(a[4]))
    wrap("interaction_", lambda a: 1)
    Nz = 6
    for pol, lt in (("IQU", 35), ("IQUV", 50)):          # native runs / the reference-layout walk
        for m_max in (0, 3):
            pm, _ = _pair(vsm, arch, pol, lt, 4, Nz, np.random.default_rng(1), m_max=m_max)
            got = {}
            for tag, levels in (("toa", [0]), ("all", None)):
                counts.update(steps=0, inter=0)
                vsm.CoreRT.rt_run_fluxes(pm, levels)
                got[tag] = dict(counts)
            assert got["toa"] == dict(steps=Nz, inter=1), (pol, m_max, got)
            assert got["all"] == dict(steps=Nz + (Nz - 1), inter=Nz), (pol, m_max, got)


def test_outputs_finite_with_poisoned_work(vsm, arch, monkeypatch):
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    H = vsm.host_model
    pm, _ = _pair(vsm, arch, "IQU", 35, 8, 6, np.random.default_rng(9), aerosols=True, m_max=1)
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=0.05 + 0.1 * np.random.default_rng(10).random((6, 8))))
    res = vsm.CoreRT.rt_run_fluxes(pm, thermal=True)
    for k in QUANTITIES + ("absorbed", "surface_absorbed"):
        x = getattr(res, k)
        assert np.all(np.isfinite(x)), k
        assert np.all((x[1:] if k.endswith("down_diffuse") else x) != 0), k


def test_refusals(vsm, arch):
    H = vsm.host_model
    tr = np.tile(np.full(4, 0.05), (2, 1))
    tr[:, 2] = 0.0
    kw = dict(tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=1)
    pm = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, **kw)
    with pytest.raises(NotImplementedError, match="does not scatter"):
        vsm.CoreRT.rt_run_fluxes(pm, [1])
    tr[:, 2] = 0.05
    B = np.full((4, 2), 0.1)
    pm = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, sources=(H.ThermalEmission(B_layer=B),), **kw)
    with pytest.raises(vsm.VSMError, match="thermal=True"):
        vsm.CoreRT.rt_run_fluxes(pm)
    res = vsm.CoreRT.rt_run_fluxes(pm, thermal=True)            # no SolarBeam: F0 = 0
    assert np.all(res.down_direct == 0) and np.all(res.actinic_direct == 0) and np.all(res.up > 0)
