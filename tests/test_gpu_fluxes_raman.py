"""GPU tests of the Raman flux run (vsm.CoreRTRaman.rt_run_fluxes, core_rt_flux_raman.py) and of its level kernel
(vsm_level_flux_ie_*, csrc/vsm_level.hip): the kernel against a numpy restatement (the level equation of ms_raman_oracle and the
quadrature), its TOA branch and its argument checks; the driver against the float64 quadrature of its sibling's level vectors
(CoreRTRaman.rt_run_multisensor(..., streams=True)), against the oracle (tests/flux_raman_oracle.py), m_max, blocked runs, FP32,
poisoned buffers, the level calls the host issues, a column with non-scattering layers and the Lambertian identity."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import flux_raman_oracle as FRO
import ms_raman_oracle as MR
from oracle import vsm_oracle as O
from test_gpu_multisensor_raman import _ie_inputs, _kernel_cases, _models, _rs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DIFFUSE = ("up", "down_diffuse", "actinic_up", "actinic_down_diffuse")
DIFFUSE_IE = tuple(k + "_ie" for k in DIFFUSE)
BUDGET = ("absorbed", "surface_absorbed", "absorbed_ie", "surface_absorbed_ie")
NZ = 5


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


def _rel(got, ref):
    """max |got - ref| relative to the largest |ref| (one quantity, all its levels and points)."""
    sc = float(np.max(np.abs(ref)))
    e = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)))
    return e / sc if sc > 0 else e


# ---- the kernel on random inputs -------------------------------------------------------------------------------------------------
def _kernel_inputs(FT, N, K, bottom, S=None):
    """The inputs of test_gpu_multisensor_raman._level_ie_vs_numpy (same shapes, shift sets and bottoms), rounded to FT, and the
    weight rows and direct-beam operands of the flux epilogue."""
    S = (9 if N <= 33 else 5) if S is None else S
    rng = np.random.default_rng(N * 1000 + K)
    ns = 3 if N % 3 == 0 else 1
    shifts = {1: [2], 9: [-4, -2, -1, 0, 1, 2, 4, S + 3, -(S + 7)]}.get(K, list(range(-35, 35)))
    assert len(shifts) == K
    rnd = lambda x: None if x is None else np.asarray(x, dtype=FT).astype(np.float64)
    A, dwf, B, uwf = map(rnd, _ie_inputs(N, S, rng, bottom == "shared"))
    Aie, aie = rnd(0.05 * rng.random((K, S, N, N)) / N), rnd(0.05 * rng.random((K, S, N)))
    Bie, cie = (None, None) if bottom == "null" else (rnd(0.05 * rng.random((K, S, N, N)) / N), rnd(0.05 * rng.random((K, S, N))))
    q, dir_h = rnd(rng.random((4, N // ns))), rnd(rng.random(4))
    tau, F0 = rnd(rng.random(S) * 2), rnd(0.5 + rng.random(S))
    return dict(N=N, ns=ns, S=S, K=K, shifts=shifts, A=A, B=B, dwf=dwf, uwf=uwf, Aie=Aie, aie=aie, Bie=Bie, cie=cie, q=q,
                dir_h=dir_h, tau=tau, F0=F0, mu0=float(rnd(0.7)))


def _device(FT, h):
    """The device arrays: matrices in math order [..., i, j] -> the reference's column-major blocks (element (i, j) at i + N j)."""
    dt = torch.float64 if FT == np.float64 else torch.float32
    tv = lambda x: None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=FT), dtype=dt, device="cuda")
    tm = lambda x: None if x is None else tv(np.swapaxes(x, -1, -2))
    d = {k: tm(h[k]) for k in ("A", "B", "Aie", "Bie")}
    d.update({k: tv(h[k]) for k in ("dwf", "uwf", "aie", "cie", "q", "tau", "F0")})
    d["shift"] = torch.tensor(np.asarray(h["shifts"], dtype=np.int32), device="cuda")
    return dt, d


def _flux_ie(vsm, FT, h, d, nW, out_t, top=True, direct=True, **over):
    """One vsm_level_flux_ie_* call through the raw symbol; returns its status.  over: operands replaced (None: a NULL pointer)."""
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    ct = C.c_double if FT == np.float64 else C.c_float
    N, S = h["N"], h["S"]
    g = dict(N=N, ns=h["ns"], S=S, K=h["K"], shift=P(d["shift"]), A=P(d["A"]) if top else None, B=P(d["B"]) if top else None,
             bs=0 if h["B"].shape[0] == 1 and S > 1 else N * N, dwf=P(d["dwf"]) if top else None, uwf=P(d["uwf"]),
             Aie=P(d["Aie"]) if top else None, aie=P(d["aie"]) if top else None, Bie=P(d["Bie"]), cie=P(d["cie"]),
             nW=nW, q=P(d["q"]), dh=(ct * 4)(*[float(x) for x in h["dir_h"]]), mu0=h["mu0"],
             tau=P(d["tau"]) if direct else None, F0=P(d["F0"]) if direct else None, out=P(out_t))
    g.update(over)
    fn = getattr(vsm._lib.lib(), "vsm_level_flux_ie_" + ("f64" if FT == np.float64 else "f32"))
    return fn(g["N"], g["ns"], g["S"], g["K"], g["shift"], g["A"], g["B"], g["bs"], g["dwf"], g["uwf"], g["Aie"], g["aie"], g["Bie"],
              g["cie"], g["nW"], g["q"], g["dh"], ct(g["mu0"]), g["tau"], g["F0"], g["out"], None)


def _kernel_reference(h, nW, top=True, direct=True):
    """out [5][nW][S] in float64: level_ie_push_through, then the quadratures of the rows of Stokes I."""
    S, N, ns = h["S"], h["N"], h["ns"]
    if top:
        uwie, dwie = MR.level_ie_push_through(np.float64, h["shifts"], h["A"], h["B"], h["dwf"], h["uwf"], h["Aie"], h["aie"],
                                              h["Bie"], h["cie"])
        dw = h["dwf"]
    else:      # the TOA: no system
        uwie, dwie, dw = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))
        for k, sh in enumerate(h["shifts"]):
            for n1 in range(S):
                if 0 <= n1 + int(sh) < S and h["cie"] is not None:
                    uwie[n1] += h["cie"][k, n1]
    q = h["q"][:nW]
    ref = np.zeros((5, nW, S))
    for row, v in ((0, h["uwf"]), (1, dw), (3, uwie), (4, dwie)):
        ref[row] = (v[:, ::ns] @ q.T).T
    if direct:
        ref[2] = h["dir_h"][:nW, None] * (h["F0"] * np.exp(-h["tau"] / h["mu0"]))[None, :]
    return ref


def _check_rows(got, ref, tol, what):
    """Each of the five rows of out within tol of its own largest reference value; returns the errors."""
    assert np.all(np.isfinite(got)), what
    errs = []
    for row in range(5):
        sc = float(np.max(np.abs(ref[row])))
        e = float(np.max(np.abs(got[row] - ref[row])))
        errs.append(e / sc if sc > 0 else e)
        assert e <= tol * sc, (what, row, e, sc)
    return errs


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N,K,bottom", _kernel_cases())
def test_level_flux_ie_kernel_vs_numpy(vsm, FT, N, K, bottom):
    """Random inputs; shifts in band, partly in band and never in band; a per-point, a shared-block (bot_stride 0) and a NULL
    inelastic bottom; nW = 2 (and 4 at N = 21, K = 9); out starts as NaN and must be overwritten.  The bounds of
    test_level_ie_kernel_vs_numpy: 1e-10 / 5e-4 of the largest reference value, here per row of out."""
    h = _kernel_inputs(FT, N, K, bottom)
    dt, d = _device(FT, h)
    tol = 1e-10 if FT == np.float64 else 5e-4
    for nW in (2, 4) if (N, K) == (21, 9) else (2,):
        out = torch.full((5, nW, h["S"]), float("nan"), dtype=dt, device="cuda")
        assert _flux_ie(vsm, FT, h, d, nW, out) == 0
        torch.cuda.synchronize()
        vsm._lib.check_device_status("level_flux_ie test")
        ref = _kernel_reference(h, nW)
        assert np.max(np.abs(ref[3])) > 0 and np.max(np.abs(ref[4])) > 0
        errs = _check_rows(out.cpu().numpy().astype(np.float64), ref, tol, (N, K, bottom, nW))
        print("level_flux_ie N %3d K %2d %-9s nW %d %s: %s" % (N, K, bottom, nW, np.dtype(FT).name, " ".join("%.1e" % e for e in errs)))


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_flux_ie_kernel_without_lines_and_without_beam(vsm, FT):
    """K = 0 is legal: the ie rows are written as 0; without tau_sum / F0_I the direct row is 0."""
    h = _kernel_inputs(FT, 12, 1, "per_point")
    dt, d = _device(FT, h)
    out = torch.full((5, 2, h["S"]), float("nan"), dtype=dt, device="cuda")
    assert _flux_ie(vsm, FT, h, d, 2, out, direct=False, K=0, shift=None, Aie=None, aie=None, Bie=None, cie=None) == 0
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_flux_ie test")
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(got[2:] == 0)
    ref = _kernel_reference(h, 2, direct=False)
    for row in (0, 1):
        assert np.max(np.abs(got[row] - ref[row])) <= (1e-10 if FT == np.float64 else 5e-4) * np.max(np.abs(ref[row]))


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [12, 128])
def test_level_flux_ie_kernel_toa(vsm, FT, N):
    """top_R_pm = NULL: no system.  uw = uw_full, uw_ie = the sum of bot_ieJ0_m over the in-band lines (the shift set holds one that
    is partly and two that are never in band), both down rows exactly 0; dw_full, B and the top arrays are NULL, so not read (bot_ieR_mp is not read either,
    but comes and goes with bot_ieJ0_m).
    Then a bottom without an inelastic part: up_ie = 0 as well."""
    h = _kernel_inputs(FT, N, 9, "per_point")
    assert sum(1 for s in h["shifts"] if abs(s) >= h["S"]) == 2
    dt, d = _device(FT, h)
    tol = 1e-10 if FT == np.float64 else 5e-4
    out = torch.full((5, 2, h["S"]), float("nan"), dtype=dt, device="cuda")
    assert _flux_ie(vsm, FT, h, d, 2, out, top=False) == 0
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_flux_ie test")
    got = out.cpu().numpy().astype(np.float64)
    ref = _kernel_reference(h, 2, top=False)
    assert np.max(np.abs(ref[3])) > 0
    _check_rows(got, ref, tol, ("toa", N))
    assert np.all(got[1] == 0) and np.all(got[4] == 0)
    # (a line that is never in band does not enter: the sum over ALL lines differs)
    all_lines = (h["cie"].sum(axis=0)[:, ::h["ns"]] @ h["q"][:2].T).T
    assert np.max(np.abs(all_lines - ref[3])) > 0.05 * np.max(np.abs(ref[3]))
    out.fill_(float("nan"))
    assert _flux_ie(vsm, FT, h, d, 2, out, top=False, Bie=None, cie=None) == 0
    torch.cuda.synchronize()
    got2 = out.cpu().numpy().astype(np.float64)
    assert np.array_equal(got2[:3], got[:3]) and np.all(got2[3:] == 0)


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_flux_ie_kernel_refuses_bad_arguments(vsm, FT):
    """Every argument error returns VSM_ERR_INVALID_ARG before any launch (the NaN-filled output stays); S = 0 is no error."""
    h = _kernel_inputs(FT, 16, 9, "per_point")
    dt, d = _device(FT, h)
    out = torch.full((5, 4, h["S"]), float("nan"), dtype=dt, device="cuda")
    call = lambda **kw: _flux_ie(vsm, FT, h, d, kw.pop("nW", 2), out, **kw)
    INVALID = 1          # VSM_ERR_INVALID_ARG
    bad = [dict(N=129), dict(N=0), dict(ns=3), dict(ns=0), dict(S=-1), dict(K=-1), dict(nW=0), dict(nW=5), dict(bs=7), dict(q=None),
           dict(out=None), dict(uwf=None), dict(dwf=None), dict(B=None), dict(shift=None), dict(Aie=None), dict(aie=None),
           dict(Bie=None), dict(cie=None), dict(tau=None), dict(F0=None), dict(dh=None), dict(mu0=0.0)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert vsm._lib.lib().vsm_last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(out)))
    assert call(S=0) == 0 and call(S=0, q=None, out=None, uwf=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(out)))
    assert call(nW=4) == 0          # the largest count the kernel takes
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_flux_ie test")
    assert bool(torch.all(torch.isfinite(out)))


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _sibling_quadrature(pm, ms, levels):
    """The diffuse quantities of CoreRTRaman.rt_run_fluxes from rt_run_multisensor(..., streams=True)'s m = 0 level vectors, in
    float64, level 0 by the rule of the flux run (its uw / uwie; no diffuse field enters the TOA)."""
    qp = pm.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    n = pm.polarization_type.n
    rows = {k: [] for k in DIFFUSE + DIFFUSE_IE}
    assert ms.weight[0] == 0.5 / math.pi
    for i, l in enumerate(levels):
        down = 0.0 if l == 0 else 1.0
        for sfx, us, ds in (("", ms.uw_streams, ms.dw_streams), ("_ie", ms.uwie_streams, ms.dwie_streams)):
            uw = us[i][0][::n, 0, :].astype(np.float64)          # [Nquad, S]
            dw = ds[i][0][::n, 0, :].astype(np.float64) * down
            rows["up" + sfx].append((mu * w) @ uw)
            rows["down_diffuse" + sfx].append((mu * w) @ dw)
            rows["actinic_up" + sfx].append(w @ uw)
            rows["actinic_down_diffuse" + sfx].append(w @ dw)
    return {k: np.array(v) for k, v in rows.items()}


S_DRV = 24


@pytest.fixture(scope="module", params=["I", "IQU"])
def scene(request, vsm, arch):
    """The `_models` scene of test_gpu_multisensor_raman.py (l_trunc 7, S = 24, five layers, SHIFTS / W_IE) and, computed once, the
    flux run over all levels and its sibling's level vectors."""
    om, pm = _models(vsm, arch, request.param, 7, S_DRV, NZ, np.float64)
    ors, prs = _rs(vsm)
    levels = list(range(NZ + 1))
    res = vsm.CoreRTRaman.rt_run_fluxes(prs, pm)
    ms = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, levels, streams=True)
    return dict(om=om, pm=pm, ors=ors, prs=prs, levels=levels, res=res, ms=ms)


def _against_sibling(pm, res, ms, levels):
    want = _sibling_quadrature(pm, ms, levels)
    errs = {k: _rel(getattr(res, k), v) for k, v in want.items()}
    print("RAMAN FLUX vs multisensor %r: %s" % (levels, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(np.max(np.abs(v)) > 0 for v in want.values())
    assert max(errs.values()) <= 1e-11, errs
    # down_diffuse(_ie) at level Nz is the quadrature of the sibling's level-0 dw / dwie (rt_run's T / ieT)
    qp, n = pm.quad_points, pm.polarization_type.n
    muw = np.asarray(qp.qp_mu, dtype=np.float64) * np.asarray(qp.wt_mu, dtype=np.float64)
    for name, st in (("down_diffuse", ms.dw_streams), ("down_diffuse_ie", ms.dwie_streams)):
        t_bottom = muw @ st[levels.index(0)][0][::n, 0, :].astype(np.float64)
        assert np.max(np.abs(t_bottom)) > 0
        assert _rel(getattr(res, name)[levels.index(NZ)], t_bottom) <= 1e-11, name


def test_fluxes_against_the_multisensor_run(scene):
    """Every diffuse quantity, elastic and inelastic, is the float64 quadrature of CoreRTRaman.rt_run_multisensor(...,
    streams=True)'s own m = 0 level vectors within 1e-11 of its largest value over the levels (the bound of
    test_gpu_fluxes.test_fluxes_against_the_multisensor_run); all levels."""
    res, levels = scene["res"], scene["levels"]
    assert res.levels == levels and res.up.dtype == np.float64 and res.up.shape == (NZ + 1, S_DRV)
    _against_sibling(scene["pm"], res, scene["ms"], levels)
    for k in ("down_diffuse", "actinic_down_diffuse", "down_diffuse_ie", "actinic_down_diffuse_ie"):
        assert np.all(getattr(res, k)[0] == 0), k
    assert np.array_equal(res.net_down, res.down_direct + res.down_diffuse - res.up)
    assert np.array_equal(res.net_down_ie, res.down_diffuse_ie - res.up_ie)
    assert np.array_equal(res.absorbed, res.net_down[:-1] - res.net_down[1:]) and np.array_equal(res.surface_absorbed, res.net_down[-1])
    assert np.array_equal(res.absorbed_ie, res.net_down_ie[:-1] - res.net_down_ie[1:])
    assert np.array_equal(res.surface_absorbed_ie, res.net_down_ie[-1])


def test_fluxes_of_some_levels(vsm, scene):
    """Levels [2, 0, Nz, 2]: unsorted, a duplicate; against the sibling on the same levels; the duplicate rows are the same
    array, the rows agree with those of the run over all levels (other segments below level 2, so other rounding: each run is
    within 1e-8 of the prototype, so the two are within 2e-8 of each other); no budget."""
    levels = [2, 0, NZ, 2]
    res = vsm.CoreRTRaman.rt_run_fluxes(scene["prs"], scene["pm"], levels)
    ms = vsm.CoreRTRaman.rt_run_multisensor(scene["prs"], scene["pm"], levels, streams=True)
    assert res.levels == levels
    _against_sibling(scene["pm"], res, ms, levels)
    for k in FRO.FIELDS:
        assert np.array_equal(getattr(res, k)[0], getattr(res, k)[3]), k
        assert _rel(getattr(res, k), getattr(scene["res"], k)[levels]) <= 2e-8, k
    assert all(getattr(res, k) is None for k in BUDGET)


def test_fluxes_against_oracle(scene):
    """Against the statement-order prototype's level vectors (tests/flux_raman_oracle.py): 1e-8 of each quantity's largest value."""
    res = scene["res"]
    ref = FRO.fluxes_raman_reference(scene["om"], scene["ors"], scene["levels"])
    errs = {k: _rel(getattr(res, k), getattr(ref, k)) for k in FRO.FIELDS}
    for k in BUDGET:
        sc = float(np.max(np.abs(ref.net_down_ie if k.endswith("_ie") else ref.net_down)))
        errs[k] = float(np.max(np.abs(getattr(res, k) - getattr(ref, k)))) / sc
    print("RAMAN FLUX vs oracle: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert np.max(np.abs(ref.up_ie)) > 1e-4 * np.max(np.abs(ref.up))
    assert max(errs.values()) <= 1e-8, errs


def test_m_max_does_not_enter(vsm, scene):
    assert scene["pm"].m_max == 2
    r0 = vsm.CoreRTRaman.rt_run_fluxes(scene["prs"], dataclasses.replace(scene["pm"], m_max=0))
    for k in FRO.FIELDS + BUDGET:
        assert np.array_equal(getattr(r0, k), getattr(scene["res"], k)), k


def test_blocked_run_bit_identical(vsm, scene):
    """max_points = 7 on 24 points (blocks of 7, 7, 7, 3, each with its halo of 5 donor points, cropped) against one pass."""
    blk = vsm.CoreRTRaman.rt_run_fluxes(scene["prs"], scene["pm"], max_points=7)
    for k in FRO.FIELDS + BUDGET:
        assert np.array_equal(getattr(blk, k), getattr(scene["res"], k)), k


def test_fluxes_float32(vsm, arch):
    """The FP32 bound of test_gpu_multisensor_raman.test_device_vs_prototype (1e-2), per quantity relative to its largest value."""
    om, pm = _models(vsm, arch, "IQU", 7, S_DRV, NZ, np.float32)
    ors, prs = _rs(vsm)
    res = vsm.CoreRTRaman.rt_run_fluxes(prs, pm)
    assert res.up.dtype == np.float32 and res.up_ie.dtype == np.float32 and res.absorbed_ie.dtype == np.float32
    ref = FRO.fluxes_raman_reference(om, ors, res.levels)
    errs = {k: _rel(getattr(res, k), getattr(ref, k)) for k in FRO.FIELDS}
    print("RAMAN FLUX f32: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1e-2, errs


def test_outputs_finite_with_poisoned_work(vsm, arch, monkeypatch):
    """VSM_POISON_WORK fills every work buffer with NaN."""
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    vsm.CoreRTRaman._work.clear()
    try:
        _, pm = _models(vsm, arch, "IQU", 7, 12, NZ, np.float64)
        _, prs = _rs(vsm)
        res = vsm.CoreRTRaman.rt_run_fluxes(prs, pm)
    finally:
        vsm.CoreRTRaman._work.clear()
    for k in FRO.FIELDS + BUDGET:
        x = getattr(res, k)
        assert np.all(np.isfinite(x)), k
        assert np.all((x[1:] if "down_diffuse" in k else x) != 0), k


def test_level_calls(vsm, arch, monkeypatch):
    """Per distinct level exactly one vsm_level_flux_ie_* call and, below the TOA, one elastic level call without viewing rows; no
    vsm_level_radiance_ie_*, no vsm_level_flux_*, whatever m_max is."""
    _, pm = _models(vsm, arch, "IQU", 7, 8, 6, np.float64, m_max=2)
    _, prs = _rs(vsm)
    names = []
    call = vsm._lib.call

    def counting(name, *a, **kw):
        if name.startswith("vsm_level_"):
            names.append((name, a))
        return call(name, *a, **kw)
    monkeypatch.setattr(vsm._lib, "call", counting)
    for levels, distinct in (([4, 2, 0, 6, 2], 4), (None, 7), ([0], 1), ([3], 1)):
        names.clear()
        vsm.CoreRTRaman.rt_run_fluxes(prs, pm, levels)
        count = lambda n: sum(1 for x, _ in names if x == n)
        below = distinct - (0 if levels == [3] else 1)
        assert count("vsm_level_flux_ie") == distinct, (levels, [x for x, _ in names])
        assert count("vsm_level_radiance") == below
        assert count("vsm_level_radiance_ie") == 0 and count("vsm_level_flux") == 0
        assert len(names) == distinct + below
        assert all(a[4] == 0 for x, a in names if x == "vsm_level_radiance")      # nV = 0: no viewing row


def test_nonscattering_layers(vsm, arch):
    """The "01_10_11" column of test_gpu_multisensor_raman.test_nonscattering_layers: the run takes it, with rt_run(RRS)'s
    convention for the tags, against the prototype at 1e-8."""
    S, L, tiny = 16, 4, 1e-22
    tau_rayl = np.tile([tiny, 0.04, tiny, 0.03], (S, 1))
    om, pm = _models(vsm, arch, "IQU", 7, S, L, np.float64, seed=21, tau_rayl=tau_rayl)
    tags, _ = O.extract_effective_props(O.construct_core_optical_properties(om, 0), np.float64)
    assert list(tags[1:L]) == ["01", "10", "11"]
    ors, prs = _rs(vsm)
    levels = [2, 0, 4, 1, 3]
    res = vsm.CoreRTRaman.rt_run_fluxes(prs, pm, levels)
    ref = FRO.fluxes_raman_reference(om, ors, levels)
    errs = {k: _rel(getattr(res, k), getattr(ref, k)) for k in FRO.FIELDS}
    print("RAMAN FLUX, non-scattering layers: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert np.max(np.abs(ref.up_ie)) > 0
    assert max(errs.values()) <= 1e-8, errs


def test_lambertian_identity_on_device(vsm, arch):
    """up_ie[Nz] = albedo down_diffuse_ie[Nz] and, under the unit beam (the reference's Lambertian surface layer builds its beam
    term with pol.I0, not with F0: DESIGN.md §6), up[Nz] = albedo (down_direct + down_diffuse)[Nz], to 1e-12."""
    _, pm = _models(vsm, arch, "IQU", 7, S_DRV, NZ, np.float64)
    _, prs = _rs(vsm)
    F0 = np.zeros_like(pm.F0)
    F0[0] = 1
    pm.F0 = F0
    res = vsm.CoreRTRaman.rt_run_fluxes(prs, pm, [NZ])
    alb = 0.12
    want = alb * (res.down_direct[0] + res.down_diffuse[0])
    want_ie = alb * res.down_diffuse_ie[0]
    assert np.min(np.abs(want_ie)) > 0
    e = float(np.max(np.abs(res.up[0] - want) / np.abs(want)))
    e_ie = float(np.max(np.abs(res.up_ie[0] - want_ie) / np.abs(want_ie)))
    print("device: up[Nz] vs albedo (direct + diffuse)[Nz]: rel %.2e; up_ie[Nz] vs albedo down_diffuse_ie[Nz]: rel %.2e" % (e, e_ie))
    assert e <= 1e-12 and e_ie <= 1e-12
