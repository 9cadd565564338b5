"""GPU tests of the linearized multi-sensor run with thermal emission (vsm.CoreRTLin.rt_run_multisensor over SolarBeam and / or
ThermalEmission(B_layer, B_layer_dot), core_rt_ms_lin.py) and of its level kernel (vsm_level_radiance_lin_src_*,
csrc/vsm_level.hip): against the numpy restatement (tests/ms_thermal_lin_oracle.py, pinned by finite differences of the forward
oracle in tests/test_oracle_multisensor_thermal_lin.py), level 0 against SceneLin.run(lanes=1, fold=False) bit for bit, the forward
part against CoreRT.rt_run_multisensor(thermal=True), FP32, BRDF surfaces, streams, blocked runs, poisoned work buffers, the calls
the host issues, the untouched path of a model without the source, the refusals, and the kernel alone against numpy.

Bounds: those of tests/test_gpu_multisensor_lin.py for the same shapes and kernels (1e-8 per component against the oracle, 1e-12
for the forward part, 1e-9 for the level vectors, 2e-2 in FP32; the kernel alone 1e-11 in FP64 and 2e-4 in FP32)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
import brdf_lin_oracle as BL  # noqa: E402
import ms_lin_oracle as MSL  # noqa: E402
import ms_thermal_lin_oracle as MTL  # noqa: E402
import thermal_lin_oracle as TL  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
from test_gpu_multisensor_lin import _err, _idx, _kernel_inputs, _pair, _sub  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _B(L, S):
    """B_layer [L, S] with a gradient over the layers and over the points."""
    return 0.1 + 0.02 * np.arange(L)[:, None] * (1.0 + np.arange(S) / S)[None, :]


def _Bdot(L, S, n=3):
    """A uniform table, the unit table of one layer (a weighting function), a gradient."""
    Bd = np.stack([np.ones((L, S)), np.zeros((L, S)), 0.3 + 0.1 * np.arange(L)[:, None] * (1.0 + np.arange(S) / S)[None, :]])
    Bd[1, L // 2] = 1.0
    return Bd[:n]


def _sources(H, which, L, S, n=3, FT=np.float64):
    th = H.ThermalEmission(B_layer=_B(L, S), B_layer_dot=_Bdot(L, S, n) if n else np.zeros((0, L, S)))
    return (H.SolarBeam(), th) if which == "solar+thermal" else (th,)


CASES = {
    # id: (pol, l_trunc, S, Nz, levels, nPlanck, kwargs of test_gpu_multisensor_lin._pair)
    "scalar_n8": ("I", 9, 5, 6, [3, 0, 6, 1], 3, dict(m_max=3, vza=(30.0, 5.0), vaz=(0.0, 60.0))),
    "s3_unsorted_duplicates": ("IQU", 9, 3, 6, [5, 2, 5, 0, 2, 6, 1], 3, dict(m_max=3)),
    "c2lin_n60_iqu_sub0": ("IQU", 35, 300, 40, [0, 1, 20, 39, 40], 2, dict(vza=(30.0,), vaz=(0.0,))),
    "iquv_n128": ("IQUV", 57, 2, 3, [1, 2, 3, 0], 2, dict(m_max=1, vza=(30.0, 5.0), vaz=(0.0, 60.0))),
}


def _case(vsm, arch, name, which="solar+thermal", FT=np.float64):
    pol, lt, S, L, levels, n, kw = CASES[name]
    pm, pl, om, ol = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(len(name)), FT=FT, **kw)
    pm.sources = _sources(vsm.host_model, which, L, S, n)
    return pm, pl, om, ol, levels


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(solar part, thermal part) of a case's oracle on the points _idx(S), computed once and only read.  The solar part of a
    model without a SolarBeam is zero: the linearized surface builders are driven by F0
    (tests/test_oracle_multisensor_thermal_lin.py::test_level0_is_rt_run_thermal_lin_plus_solar)."""
    pol, lt, S, L, levels, n, kw = CASES[name]
    _, _, om, ol = _pair(_oracle.vsm, _oracle.arch, pol, lt, S, L, np.random.default_rng(len(name)), **kw)
    idx = _idx(S)
    oms, ols = _sub(om, ol, idx)
    full_s, full_t = {}, {}
    sol = MSL.ms_lin_segmented(oms, ols, levels, full=full_s)
    th = MTL.ms_thermal_lin_segmented(oms, ols, _B(L, S)[:, idx], _Bdot(L, S, n)[:, :, idx], levels, full=full_t)
    return sol, th, full_s, full_t


def _total(sol, th, which):
    nPl = th[2][0].shape[-1] - sol[2][0].shape[-1]
    pad = lambda x: np.concatenate([x, np.zeros(x.shape[:3] + (nPl,))], axis=3)
    if which == "thermal":
        return th
    return ([a + b for a, b in zip(sol[0], th[0])], [a + b for a, b in zip(sol[1], th[1])],
            [pad(a) + b for a, b in zip(sol[2], th[2])], [pad(a) + b for a, b in zip(sol[3], th[3])])


def _pick(got, idx):
    return tuple([g[..., idx, :] if g.ndim == 4 else g[..., idx] for g in xs] for xs in got)


@pytest.mark.parametrize("which", ["solar+thermal", "thermal"])
@pytest.mark.parametrize("name", list(CASES))
def test_multisensor_thermal_lin_against_oracle_fp64(vsm, arch, name, which):
    _oracle.vsm, _oracle.arch = vsm, arch
    pm, pl, om, ol, levels = _case(vsm, arch, name, which)
    pol, lt, S, L, _, n, _ = CASES[name]
    N = pm.quad_points.Nquad * pm.polarization_type.n
    if name.startswith("c2lin"):     # the solar m = 0 runs as a Stokes_IQ scene at N = 40, the slot on the parent's N = 60
        sc = vsm.CoreRTLin.SceneLin(pm, pl, 0, 1, 1)
        assert sc.sub0 is not None and N == 60 and sc.sub0.N == 40
        del sc
    if name.startswith("iquv"):
        assert N == 128
    got = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    sol, th, _, _ = _oracle(name)
    ref = _total(sol, th, which)
    g = _pick(got, _idx(S))
    per = [max(_err([x[i]], [r[i]]) for x, r in zip(g, ref)) for i in range(len(levels))]
    print("MS-thermal-lin %-24s %-13s N %3d S %4d levels %s: rel err %s" % (name, which, N, S, levels, " ".join("%.2e" % x for x in per)))
    assert max(per) <= 1e-8, (name, which, per)
    for i, l in enumerate(levels):
        assert got[2][i].shape == got[0][i].shape + (2 + n,) and all(np.all(np.isfinite(x[i])) for x in got)
        assert np.abs(got[2][i][..., 2:]).max() + np.abs(got[3][i][..., 2:]).max() > 0       # the Planck slots are there
        j = levels.index(l)
        assert all(np.array_equal(x[i], x[j]) for x in got)


@pytest.mark.parametrize("S,lt,sub0", [(300, 35, True), (3, 9, False)])
def test_level0_is_scene_lin_run_bit_for_bit(vsm, arch, S, lt, sub0):
    pm, pl, _, _ = _pair(vsm, arch, "IQU", lt, S, 8, np.random.default_rng(4), vza=(30.0,), vaz=(0.0,))
    pm.sources = _sources(vsm.host_model, "solar+thermal", 8, S, 2)
    uw, dw, uwd, dwd = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, [3, 0, 8])
    sc = vsm.CoreRTLin.SceneLin(pm, pl, 0, 1, 1)
    assert (sc.sub0 is not None) == sub0
    sc.run(lanes=1, fold=False)
    torch.cuda.synchronize()
    R, T, Rd, Td = sc.results_host()
    assert Rd.shape[-1] == 4 and np.abs(Rd[..., 2:]).max() > 0
    for a, b in ((uw[1], R), (dw[1], T), (uwd[1], Rd), (dwd[1], Td)):
        assert np.array_equal(a, b)


def test_planck_tables_alone_and_slot_alone(vsm, arch):
    """B_layer = 0 with Planck tables: no thermal radiance, the Planck block of the full model bit for bit (the slot's operators
    do not depend on B); B_layer alone: the first Nparams slots of the full model bit for bit."""
    H = vsm.host_model
    S, L, levels = 3, 6, [2, 0, 6]
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, S, L, np.random.default_rng(5))
    run = lambda th: vsm.CoreRTLin.rt_run_multisensor(dataclasses.replace(pm, sources=(H.SolarBeam(), th)), pl, 0, 1, 1, levels)
    both = run(H.ThermalEmission(B_layer=_B(L, S), B_layer_dot=_Bdot(L, S)))
    only = run(H.ThermalEmission(B_layer=np.zeros((L, S)), B_layer_dot=_Bdot(L, S)))
    slot = run(H.ThermalEmission(B_layer=_B(L, S), B_layer_dot=np.zeros((0, L, S))))
    none = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    for i in range(len(levels)):
        assert np.array_equal(only[2][i][..., 2:], both[2][i][..., 2:]) and np.array_equal(only[3][i][..., 2:], both[3][i][..., 2:])
        assert np.array_equal(only[0][i], none[0][i]) and np.array_equal(only[2][i][..., :2], none[2][i])
        assert slot[2][i].shape[-1] == 2
        assert np.array_equal(slot[0][i], both[0][i]) and np.array_equal(slot[3][i], both[3][i][..., :2])


def test_forward_part_is_rt_run_multisensor_thermal(vsm, arch):
    pm, pl, _, _, levels = _case(vsm, arch, "c2lin_n60_iqu_sub0")
    uw, dw, _, _ = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    ue, de = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=True)
    assert max(_err(uw, ue), _err(dw, de)) <= 1e-12
    u0, _ = vsm.CoreRT.rt_run_multisensor(dataclasses.replace(pm, sources=None), levels)
    assert _err(uw, u0) > 1e-3                       # (the thermal radiance is part of it)


def test_multisensor_thermal_lin_fp32(vsm, arch):
    """Float32 model against the FP64 oracle at the FP32 gate of test_gpu_multisensor_lin.py (2e-2), per level and slot."""
    S, L, levels = 3, 5, [0, 2, 4, 5]
    pm, pl, om, ol = _pair(vsm, arch, "IQU", 33, S, L, np.random.default_rng(8), FT=np.float32)
    pm.sources = _sources(vsm.host_model, "solar+thermal", L, S, 2)
    got = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    assert got[0][0].dtype == np.float32 and got[2][0].dtype == np.float32 and got[2][0].shape[-1] == 4
    ref = MTL.ms_thermal_lin_total(om, ol, _B(L, S), _Bdot(L, S, 2), levels)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    e = max(max(rel(g[i], r[i]) for g, r in zip(got[:2], ref[:2])) for i in range(len(levels)))
    e = max(e, max(rel(g[i][..., p], r[i][..., p]) for g, r in zip(got[2:], ref[2:]) for i in range(len(levels)) for p in range(4)))
    print("MS-thermal-lin fp32: %.2e" % e)
    assert e < 2e-2, e


@pytest.mark.parametrize("kind", ["coxmunk", "rpv"])
def test_multisensor_thermal_lin_over_brdf_surfaces(vsm, arch, kind):
    """The scene of test_gpu_thermal_lin.py::test_rt_run_lin_thermal_over_brdf_surfaces (Stokes_IQU, N = 21, two gases) at three
    levels.  Cox-Munk (one slot): solar + thermal.  rpvSurfaceScalar (NSurf = 4): the thermal source alone, whose solar part is
    zero (ms_lin_oracle carries one surface slot only).  The oracles take the device's Fourier reflectance blocks and their
    derivatives, as test_gpu_multisensor_lin.py::test_multisensor_lin_coxmunk does and for its reason."""
    from test_gpu_thermal_lin import GEO, L, S, _arrays
    H, CL = vsm.host_model, vsm.CoreRTLin
    pol, l_trunc, levels = "IQU", 9, [1, 0, 3, 2]
    kw, ga, gb = _arrays()
    om = O.build_model(pol, l_trunc, *GEO, albedo=0.0, **kw)
    lin = OL.LinModel([ga, gb])
    th_host = vsm.Architectures.to_host
    B, Bd = _B(L, S), _Bdot(L, S, 2)
    if kind == "coxmunk":
        hs, K, which = H.CoxMunkSurface(wind_speed=5.0), 1, "solar+thermal"
    else:
        osurf = BL.SURFACES["rpv"]
        hs, K, which = H.rpvSurfaceScalar(*[getattr(osurf, n) for n in BL.param_names(osurf)]), 4, "thermal"
    src = (H.SolarBeam(), H.ThermalEmission(B_layer=B, B_layer_dot=Bd)) if kind == "coxmunk" else (H.ThermalEmission(B_layer=B, B_layer_dot=Bd),)
    pm = H.model_from_arrays(arch, pol, l_trunc, *GEO, surface=hs, sources=src, **kw)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, np.float64)

    def tables(m):
        if kind == "coxmunk":
            rho, drho = vsm.CoreRT.reflectance(hs, dq, m, arch, np.float64, deriv=True)
            return th_host(rho).T.copy(), th_host(drho).T.copy()[None]
        rho, drho = CL.land_brdf_reflectance_lin(hs, dq, m, arch, np.float64)
        return th_host(rho[m]).T.copy(), np.swapaxes(th_host(drho[m]), -1, -2).copy()
    got = CL.rt_run_multisensor(pm, H.LinModel([ga, gb]), 0, 2, K, levels)
    assert got[2][0].shape[-1] == 2 + K + 2
    ref = MTL.ms_thermal_lin_segmented(om, lin, B, Bd, levels, surface=TL.brdf_surface(K, tables))
    if kind == "coxmunk":
        sol = MSL.ms_lin_segmented(om, lin, levels, surface=lambda m: tuple(x[0] if x.ndim == 3 else x for x in tables(m)))
        ref = _total(sol, ref, which)
    e = max(_err(g, r) for g, r in zip(got, ref))
    print("MS-thermal-lin %s: %.2e" % (kind, e))
    assert e <= 1e-8, (kind, e)
    assert min(np.abs(got[2][i][..., 2:2 + K]).max() for i in range(len(levels))) > 0      # the surface slots reach every level


def test_streams_match_the_oracle(vsm, arch):
    _oracle.vsm, _oracle.arch = vsm, arch
    name = "s3_unsorted_duplicates"
    pm, pl, om, ol, levels = _case(vsm, arch, name)
    res = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True)
    _, _, fs, ft = _oracle(name)
    nPl = 3
    assert res.uw_dot_streams[0][0].shape[-1] == 2 + nPl
    for i, l in enumerate(levels):
        for m in range(pm.m_max + 1):
            u, d, ud, dd = fs[(l, m)]
            ud, dd = (np.concatenate([x, np.zeros((nPl,) + x.shape[1:])]) for x in (ud, dd))
            if m == 0:
                u, d, ud, dd = (a + b for a, b in zip((u, d, ud, dd), ft[(l, 0)]))
            for got, ref in ((res.uw_streams[i][m][:, 0].T, u), (res.dw_streams[i][m][:, 0].T, d),
                             (res.uw_dot_streams[i][m][:, 0].transpose(2, 1, 0), ud),
                             (res.dw_dot_streams[i][m][:, 0].transpose(2, 1, 0), dd)):
                assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (l, m)
            if m > 0:
                assert not np.any(res.uw_dot_streams[i][m][..., 2:]) and not np.any(res.dw_dot_streams[i][m][..., 2:])


@pytest.mark.parametrize("S,max_points", [(7, 3), (140, 64)])
def test_blocked_runs_are_bit_identical(vsm, arch, S, max_points):
    """As test_gpu_multisensor_lin.py: 7 points in blocks of 3, 3, 1; 140 points (the m = 0 sub-scene applies) in blocks of 64, 76."""
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, S, 6, np.random.default_rng(10), m_max=3)
    pm.sources = _sources(vsm.host_model, "solar+thermal", 6, S, 2)
    levels = [4, 0, 6, 2]
    one = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True)
    blk = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True, max_points=max_points)
    for name in ("uw", "dw", "uw_dot", "dw_dot"):
        assert all(np.array_equal(a, b) for a, b in zip(getattr(one, name), getattr(blk, name))), name
    for name in ("uw_streams", "dw_streams", "uw_dot_streams", "dw_dot_streams"):
        for la, lb in zip(getattr(one, name), getattr(blk, name)):
            assert all(np.array_equal(a, b) for a, b in zip(la, lb)), name
    assert one.uw_dot_streams[0][0].shape == (pm.quad_points.Nquad * 3, 1, S, 4)
    MSLIN = vsm.core_rt_ms_lin
    base = MSLIN.bytes_per_point(21, 2, 1, 6, 2, True, 4, 3, 3, 8)
    kept = (1 + 1) * (21 * 21 + 21) * 2 * 8              # the thermal tops: (1 + pl)(N^2 + N) elements per kept level
    assert MSLIN.bytes_per_point(21, 2, 1, 6, 2, True, 4, 3, 3, 8, thermal=True, nPlanck=2) >= base + kept


def test_outputs_finite_with_poisoned_work(vsm, arch, monkeypatch):
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 21, 16, 10, np.random.default_rng(9))
    pm.sources = _sources(vsm.host_model, "solar+thermal", 10, 16, 2)
    res = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, [0, 3, 7, 10])
    for xs in res:
        for x in xs:
            assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0


def _count_calls(vsm, fn):
    calls = []
    orig = vsm._lib.call
    try:
        vsm._lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
        out = fn()
    finally:
        vsm._lib.call = orig
    return calls, out


def test_thermal_layer_steps_interactions_and_level_calls(vsm, arch):
    """beside the solar calls, for m = 0 alone, Nz + (Nz - l_1) linearized thermal layer steps (one
    vsm_thermal_source_lin each), L + 1 further linearized interactions, per Planck table the same number of forward thermal layer
    steps, and per level other than 0 one more elastic level call and ONE vsm_level_radiance_lin_src call."""
    CL = vsm.CoreRTLin
    Nz, levels, K = 12, [0, 4, 9, 12], 2
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, 4, Nz, np.random.default_rng(1), m_max=3)
    base, _ = _count_calls(vsm, lambda: CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels))
    pm.sources = _sources(vsm.host_model, "solar+thermal", Nz, 4, K)
    n_inter = [0]
    orig = CL.interaction_lin_

    def counted(*a, **k):
        n_inter[0] += 1
        return orig(*a, **k)
    CL.interaction_lin_ = counted
    try:
        calls, _ = _count_calls(vsm, lambda: CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels))
    finally:
        CL.interaction_lin_ = orig
    nm, L_int, l1 = pm.m_max + 1, 2, 4
    steps = Nz + (Nz - l1)
    cnt = lambda name: sum(c == name for c in calls) - sum(c == name for c in base)
    assert cnt("vsm_thermal_source_lin") == steps
    assert n_inter[0] == (steps - (1 + L_int) + L_int + 1) * (nm + 1)          # the slot is one more "moment" of interactions
    assert cnt("vsm_thermal_source") + cnt("vsm_layer_forward_thermal") == K * steps
    assert cnt("vsm_level_radiance") == 3 and cnt("vsm_level_radiance_lin_src") == 3 and cnt("vsm_level_radiance_lin") == 0
    assert cnt("vsm_level_radiance_src") == 0


def test_model_without_the_source_takes_the_parent_path(vsm, arch, monkeypatch):
    """No ThermalEmission: the calls of the run are those of the solar algorithm alone (none of the slot's kernels, the
    linearized level kernel without source slots), no `_th` state comes to exist and the result repeats bit for bit."""
    CL = vsm.CoreRTLin
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, 4, 6, np.random.default_rng(1), m_max=2)
    scenes = []
    orig = CL.SceneLin.__init__

    def spy(self, *a, **k):
        scenes.append(self)
        return orig(self, *a, **k)
    monkeypatch.setattr(CL.SceneLin, "__init__", spy)
    levels = [0, 2, 6]
    calls, first = _count_calls(vsm, lambda: CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels))
    assert scenes and all(sc._th is None and sc.fwd._thermal is None and sc.nPlanck == 0 for sc in scenes)
    assert not {"vsm_thermal_source_lin", "vsm_thermal_source", "vsm_layer_forward_thermal", "vsm_level_radiance_lin_src"} & set(calls)
    nm = pm.m_max + 1
    assert calls.count("vsm_level_radiance_lin") == 2 * nm and calls.count("vsm_level_radiance") == 2 * nm
    assert first[2][0].shape[-1] == 2
    again = CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    assert all(np.array_equal(a, b) for xs, ys in zip(first, again) for a, b in zip(xs, ys))


def test_refusals(vsm, arch):
    H, CL = vsm.host_model, vsm.CoreRTLin
    S, L = 2, 4
    pm, pl, _, _ = _pair(vsm, arch, "I", 9, S, L, np.random.default_rng(3))
    th = lambda **kw: (H.SolarBeam(), H.ThermalEmission(B_layer=_B(L, S), **dict(dict(B_layer_dot=np.zeros((0, L, S))), **kw)))
    # a source that does not state its Planck tables is forward-only: refused as before the run took thermal sources
    for srcs in (th(B_layer_dot=None), th(B_layer_dot=None)[1:]):
        with pytest.raises(vsm.VSMError, match="SolarBeam.*B_layer_dot"):
            CL.rt_run_multisensor(dataclasses.replace(pm, sources=srcs), pl, 0, 1, 1, [1])
    # a non-scattering layer
    tr = np.tile(np.full(L, 0.05), (S, 1))
    tr[:, 2] = 0.0
    g = np.full((S, L), 1e-3)
    m0 = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, tau_abs=g, albedo=0.2, m_max=1, sources=th())
    with pytest.raises(NotImplementedError, match="does not scatter"):
        CL.rt_run_multisensor(m0, H.LinModel([g]), 0, 1, 1, [1])
    # N > 128
    pb, plb, _, _ = _pair(vsm, arch, "IQUV", 61, 2, 3, np.random.default_rng(3))
    pb.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=_B(3, 2), B_layer_dot=np.zeros((0, 3, 2))))
    with pytest.raises(vsm.VSMError, match="128"):
        CL.rt_run_multisensor(pb, plb, 0, 1, 1, [1])
    # 2 slots + 63 Planck slots; 62 run
    with pytest.raises(vsm.VSMError, match="limit 64"):
        CL.rt_run_multisensor(dataclasses.replace(pm, sources=th(B_layer_dot=np.ones((63, L, S)))), pl, 0, 1, 1, [1])
    out = CL.rt_run_multisensor(dataclasses.replace(pm, sources=th(B_layer_dot=np.ones((62, L, S)))), pl, 0, 1, 1, [1, 4])
    assert out[2][0].shape[-1] == 64 and np.all(np.isfinite(out[2][0])) and np.all(np.isfinite(out[3][1]))
    # the Raman multi-sensor run and the linearized single-scattering run keep refusing the source
    with pytest.raises(NotImplementedError):
        CL.rt_run_ss(dataclasses.replace(pm, sources=th()), pl, 0, 1, 1)
    from test_gpu_multisensor_raman import _models, _rs
    _, pr = _models(vsm, arch, "I", 7, 24, 5, np.float64)
    pr.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=_B(5, 24)))
    with pytest.raises(vsm.VSMError, match="SolarBeam"):
        vsm.CoreRTRaman.rt_run_multisensor(_rs(vsm)[1], pr, [1])


# ---- the kernel alone --------------------------------------------------------------------------------------------------------
def _kernel_case(vsm, N, P, P_top, P_src, shared, S=3, FT=np.float64, ns=3, nV=2, entry="vsm_level_radiance_lin_src",
                 inputs=_kernel_inputs):
    rng = np.random.default_rng(N + 7 * P + 13 * P_src)
    ns = ns if N % ns == 0 else 1
    A, a, B, c = inputs(N, S, rng, shared)
    Ad, ad = rng.normal(0, 1, (P_top, S, N, N)) / N, rng.normal(0, 1, (P_top, S, N))
    Bd, cd = rng.normal(0, 1, (P,) + B.shape) / N, rng.normal(0, 1, (P, S, N))
    ak, ck = rng.normal(0, 1, (P_src, S, N)), rng.normal(0, 1, (P_src, S, N))
    Adz = np.concatenate([Ad, np.zeros((P - P_top, S, N, N))])
    adz = np.concatenate([ad, np.zeros((P - P_top, S, N))])
    uw, dw, uwd, dwd = MSL.level_lin_push_through(np.float64, A, a, B, c, Adz, adz, Bd, cd)
    if P_src:
        us, ds = MTL.level_src_only(np.float64, A, B, ak, ck)
        uwd, dwd = np.concatenate([uwd, us]), np.concatenate([dwd, ds])
    Pa = P + P_src
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64 if FT == np.float64 else torch.float32, device="cuda")
    sw = lambda M: np.swapaxes(M, -1, -2)                # math order -> the column-major layout
    row0 = (C.c_int * nV)(0, N - ns, *[ns * (v % (N // ns)) for v in range(2, nV)])
    ct = C.c_double if FT == np.float64 else C.c_float
    wv = rng.uniform(0.5, 1.5, nV * ns)
    w = (ct * (nV * ns))(*wv)
    init_u, init_d = rng.normal(0, 1, (Pa, S, ns, nV)), rng.normal(0, 1, (Pa, S, ns, nV))
    t = dict(A=dev(sw(A)), B=dev(sw(B)), dwf=dev(dw), uwf=dev(uw), Ad=dev(sw(Ad)) if P_top else None,
             ad=dev(ad) if P_top else None, Bd=dev(sw(Bd)), cd=dev(cd), ak=dev(ak) if P_src else None, ck=dev(ck) if P_src else None,
             uwd=dev(init_u), dwd=dev(init_d), dwdf=dev(np.full((Pa, S, N), np.nan)), uwdf=dev(np.full((Pa, S, N), np.nan)))
    p_ = lambda x: None if x is None else x.data_ptr()
    NN = N * N
    bstride = 0 if shared and S > 1 else NN
    head = (t["A"].dtype, N, ns, S, P, P_top) + ((P_src,) if entry.endswith("_src") else ())
    src = (p_(t["ak"]), p_(t["ck"])) if entry.endswith("_src") else ()
    vsm._lib.call(entry, *head, nV, row0, w, p_(t["A"]), p_(t["B"]), bstride, p_(t["dwf"]), p_(t["uwf"]), p_(t["Ad"]), S * NN,
                  p_(t["ad"]), p_(t["Bd"]), bstride, B.shape[0] * NN, p_(t["cd"]), *src, p_(t["uwd"]), p_(t["dwd"]), p_(t["dwdf"]),
                  p_(t["uwdf"]), None)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_radiance_lin_src test")
    h = lambda x: x.double().cpu().numpy()
    ref_u, ref_d = init_u.copy(), init_d.copy()
    for v in range(nV):
        for k in range(ns):
            ref_u[:, :, k, v] += wv[v + nV * k] * uwd[:, :, row0[v] + k]
            ref_d[:, :, k, v] += wv[v + nV * k] * dwd[:, :, row0[v] + k]
    return (h(t["uwdf"]), h(t["dwdf"]), h(t["uwd"]), h(t["dwd"])), (uwd, dwd, ref_u, ref_d)


KERNEL_CASES = [(8, 2, 1, 3, False), (21, 1, 0, 1, True), (60, 3, 2, 40, False), (128, 5, 4, 9, False), (128, 12, 11, 1, True)]


@pytest.mark.parametrize("N,P,P_top,P_src,shared", KERNEL_CASES)
def test_level_kernel_lin_src_vs_numpy(vsm, N, P, P_top, P_src, shared):
    """(128, 5, 4, 9): FP64 at N = 128 takes 12 slots per chunk, so P + P_src = 14 puts a chunk boundary inside the source-only
    slots and the first chunk holds both kinds; (128, 12, 11, 1): the second chunk is one source-only slot."""
    got, ref = _kernel_case(vsm, N, P, P_top, P_src, shared)
    for g, r in zip(got, ref):
        assert np.all(np.isfinite(g)) and np.abs(g - r).max() <= 1e-11 * np.abs(r).max(), (N, P, P_src)


@pytest.mark.parametrize("N,P,P_top,P_src,shared", KERNEL_CASES)
def test_level_kernel_lin_src_vs_numpy_fp32(vsm, N, P, P_top, P_src, shared):
    got, ref = _kernel_case(vsm, N, P, P_top, P_src, shared, FT=np.float32)
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 2e-4 * np.abs(r).max(), (N, P, P_src, np.abs(g - r).max() / np.abs(r).max())


def test_level_kernel_lin_src_many_angles(vsm):
    """70 viewing angles: more than the 64 one launch carries (derivative vectors in full, then vsm_postprocess_vza_lin)."""
    got, ref = _kernel_case(vsm, 21, 3, 2, 4, True, nV=70)
    for g, r in zip(got, ref):
        assert np.all(np.isfinite(g)) and np.abs(g - r).max() <= 1e-11 * np.abs(r).max()


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("N,P,P_top,shared", [(21, 3, 2, True), (128, 13, 12, False)])
def test_level_kernel_lin_src_without_sources_is_the_lin_kernel_bitwise(vsm, N, P, P_top, shared, FT):
    """vsm_level_radiance_lin_* launches the source-slot kernel with P_src = 0, so this compares an entry point with the kernel
    it forwards to: it pins the forwarding (arguments, chunking, LDS size).  The arithmetic of that one kernel is pinned against
    numpy by test_level_kernel_lin_src_vs_numpy in this file and by test_gpu_multisensor_lin.py::test_level_kernel_lin_vs_numpy
    through the other entry point."""
    a, _ = _kernel_case(vsm, N, P, P_top, 0, shared, FT=FT)
    b, _ = _kernel_case(vsm, N, P, P_top, 0, shared, FT=FT, entry="vsm_level_radiance_lin")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_level_kernel_lin_src_invalid_arguments(vsm):
    """VSM_ERR_INVALID_ARG before any launch: N > 128, P = 0, P + P_src > 64, P_src < 0, P_src > 0 without source stacks."""
    INVALID = 1                                      # VSM_ERR_INVALID_ARG (include/vsmartmom_hip.h)
    t = torch.zeros(64 * 4 * 4 * 3, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    row0, w = (C.c_int * 1)(0), (C.c_double * 1)(1.0)

    def rc(N, P, P_top, P_src, src=True):
        return vsm._lib.lib().vsm_level_radiance_lin_src_f64(N, 1, 1, P, P_top, P_src, 1, row0, w, p, p, N * N, p, p, p, N * N, p, p, N * N,
                                                             N * N, p, p if src else None, p if src else None, p, p, None, None, None)
    for args in ((129, 1, 0, 1), (4, 0, 0, 1), (4, 2, 1, 63), (4, 1, 0, -1), (4, 1, 2, 1)):
        assert rc(*args) == INVALID, args
    assert rc(4, 1, 0, 1, src=False) == INVALID
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_radiance_lin_src invalid arguments")
