"""GPU tests of the Raman multi-sensor run (vsm.CoreRTRaman.rt_run_multisensor, core_rt_ms_raman.py) and of its inelastic level
kernel (vsm_level_radiance_ie_*, csrc/vsm_level.hip): the device against the transcription of the reference's prototype
(tests/ms_raman_oracle.py), level 0 against CoreRTRaman.rt_run bit for bit, FP32, blocked vs one-pass runs, the kernel against a
numpy restatement, poisoned buffers, the number of layer steps and interactions the host issues, and non-scattering layers."""
import ctypes as C

import numpy as np
import pytest

import ms_raman_oracle as MR
from oracle import vsm_oracle as O
from oracle import vsm_oracle_raman as OR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHIFTS = np.array([-5, -2, -1, 1, 3, 40, 0])      # 40: never in band for S <= 40
W_IE = np.array([0.004, 0.012, 0.02, 0.018, 0.007, 0.3, 0.009])
LEVELS = [3, 0, 5, 1, 3]


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


def _rel_per_component(a, b):
    """max over VZA / points of |a - b|, per Stokes component, relative to that component's max |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = []
    for k in range(b.shape[1]):
        sc = float(np.max(np.abs(b[:, k])))
        out.append(float(np.max(np.abs(a[:, k] - b[:, k]))) / sc if sc > 0 else float(np.max(np.abs(a[:, k]))))
    return max(out)


def _models(vsm, arch, pol, l_trunc, S, L, FT, seed=11, m_max=2, tau_rayl=None):
    """As test_gpu_raman._raman_models: spectrally varying absorption and source, Lambertian surface."""
    rng = np.random.default_rng(seed)
    if tau_rayl is None:
        tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    tau_abs = (10.0 ** rng.uniform(-3, 0.3, (S, 1))) * np.linspace(0.5, 1.5, L)[None, :] / L
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=0.12, m_max=m_max)
    om = O.build_model(pol, l_trunc, 35.0, [20.0, 50.0], [0.0, 60.0], FT=FT, **kw)
    om.varpi_cabannes = 0.96
    pm = vsm.host_model.model_from_arrays(arch, pol, l_trunc, 35.0, [20.0, 50.0], [0.0, 60.0], float_type=FT, **kw)
    pm.varpi_Cabannes = 0.96
    F0 = np.zeros((om.pol.n, S))
    F0[0] = 0.8 + 0.4 * rng.random(S)
    om.F0, pm.F0 = F0, F0
    return om, pm


def _rs(vsm, shifts=SHIFTS, w_ie=W_IE):
    graman = O.get_greek_rayleigh(6.0 / 7.0 * 0.5)
    return (OR.RRS(i_shift=shifts, varpi_ie=w_ie, greek_raman=graman),
            vsm.CoreRTRaman.RRS(shifts, w_ie, vsm.host_model.GreekCoefs(**vars(graman))))


@pytest.mark.parametrize("FT,pol,l_trunc,S,tol", [(np.float64, "I", 7, 24, 1e-8), (np.float64, "IQU", 7, 24, 1e-8),
                                                  (np.float64, "IQU", 35, 8, 1e-8), (np.float32, "IQU", 7, 24, 1e-2)])
def test_device_vs_prototype(vsm, arch, FT, pol, l_trunc, S, tol):
    om, pm = _models(vsm, arch, pol, l_trunc, S, 5, FT)
    ors, prs = _rs(vsm)
    ref = MR.ms_raman_reference(om, ors, LEVELS)
    got = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, LEVELS)
    assert len(got) == 4
    for name, g_list, r_list in zip(("uw", "dw", "uwie", "dwie"), got, ref):
        assert len(g_list) == len(LEVELS)
        for i, l in enumerate(LEVELS):
            assert g_list[i].shape == r_list[i].shape == (2, om.pol.n, S)
            e = _rel_per_component(g_list[i], r_list[i])
            assert e <= tol, (name, l, e)
    assert np.max(np.abs(ref[2][0])) > 1e-5 and np.max(np.abs(ref[3][3])) > 1e-5


@pytest.mark.parametrize("reduce_m0", [True, False])
def test_level0_is_rt_run_bit_for_bit(vsm, arch, monkeypatch, reduce_m0):
    monkeypatch.setattr(vsm.CoreRTRaman, "REDUCE_M0", reduce_m0)
    _, pm = _models(vsm, arch, "IQU", 7, 16, 4, np.float64)
    _, prs = _rs(vsm)
    scene = vsm.CoreRTRaman.SceneRRS(prs, pm, 1)
    assert (scene.sub0 is not None) == reduce_m0
    ref = vsm.CoreRTRaman.rt_run(prs, pm, 1)
    got = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, [2, 0, 4])
    for g, r in zip(got, ref):
        assert np.array_equal(g[1], r)


def test_blocked_runs_bit_identical(vsm, arch):
    """max_points = 10 and 3 (ragged, shorter than the halo of 5): each block a SceneRRS over the block and its halo."""
    _, pm = _models(vsm, arch, "IQU", 7, 24, 5, np.float64)
    _, prs = _rs(vsm)
    one = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, LEVELS, streams=True)
    for mp in (10, 3):
        blk = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, LEVELS, streams=True, max_points=mp)
        for name in ("uw", "dw", "uwie", "dwie", "uw_streams", "dw_streams", "uwie_streams", "dwie_streams"):
            a, b = getattr(one, name), getattr(blk, name)
            assert np.array_equal(np.asarray(a), np.asarray(b)), (mp, name)


def test_streams_match_prototype(vsm, arch):
    om, pm = _models(vsm, arch, "IQU", 7, 12, 5, np.float64, m_max=1)
    ors, prs = _rs(vsm)
    full = {}
    MR.ms_raman_reference(om, ors, LEVELS, full=full)
    res = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, LEVELS, streams=True)
    assert res.levels == LEVELS and len(res.weight) == 2
    for i, l in enumerate(LEVELS):
        for m in range(2):
            for k, name in enumerate(("uw_streams", "dw_streams", "uwie_streams", "dwie_streams")):
                g = getattr(res, name)[i][m][:, 0, :].T
                r = full[(l, m)][k]
                assert np.max(np.abs(g - r)) <= 1e-8 * np.max(np.abs(r)), (l, m, name)


def _level_ie_call(vsm, FT, N, ns, S, K, shifts, A, B, dwf, uwf, Aie, aie, Bie, cie, row0, wv, uwie, dwie, dwief, uwief):
    dev = torch.device("cuda")
    dt = torch.float64 if FT == np.float64 else torch.float32
    # matrices in math order [..., i, j] -> the reference's column-major blocks (element (i, j) at i + N j)
    tv = lambda x: None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=FT), dtype=dt, device=dev)
    tm = lambda x: None if x is None else tv(np.swapaxes(x, -1, -2))
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    sh = torch.tensor(np.asarray(shifts, dtype=np.int32), device=dev)
    ct = C.c_double if FT == np.float64 else C.c_float
    nV = len(row0)
    r0 = (C.c_int * nV)(*row0)
    w = (ct * (nV * ns))(*[float(x) for x in wv])
    dA, dB, dAie, dBie = map(tm, (A, B, Aie, Bie))
    ddw, duw, daie, dcie = map(tv, (dwf, uwf, aie, cie))
    bstride = 0 if B.shape[0] == 1 and S > 1 else N * N
    vsm._lib.call("vsm_level_radiance_ie", dt, N, ns, S, K, P(sh), nV, r0, w, P(dA), P(dB), bstride, P(ddw), P(duw), P(dAie),
                  P(daie), P(dBie), P(dcie), P(uwie), P(dwie), P(dwief), P(uwief), None)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level_radiance_ie test")


def _kernel_cases():
    out = []
    for iN, N in enumerate((3, 12, 21, 33, 64, 128)):
        for iK, K in enumerate((1, 9, 70)):
            out.append((N, K, ("per_point", "shared", "null")[(iN + iK) % 3]))
    return out


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("N,K,bottom", _kernel_cases())
def test_level_ie_kernel_vs_numpy(vsm, FT, N, K, bottom):
    """Random inputs; shifts in band, partly in band and never in band; a per-point, a shared-block (bot_stride 0) and a NULL
    inelastic bottom; the stream outputs start as NaN and must be overwritten."""
    _level_ie_vs_numpy(vsm, FT, N, K, bottom, 3)


@pytest.mark.parametrize("FT", [np.float64, np.float32])
def test_level_ie_kernel_vs_numpy_many_angles(vsm, FT):
    """70 viewing angles: more than the 64 one launch carries (full vectors, then vsm_postprocess_vza)."""
    _level_ie_vs_numpy(vsm, FT, 21, 9, "per_point", 70)


def _ie_inputs(N, S, rng, shared):
    """(A, dw, B, uw): the operators and the elastic level vectors of the donors; the signature of level_cases.contractive."""
    A = 0.5 * rng.random((S, N, N)) / N
    B = 0.5 * rng.random((1 if shared else S, N, N)) / N
    dwf, uwf = rng.random((S, N)), rng.random((S, N))
    return A, dwf, B, uwf


def _level_ie_vs_numpy(vsm, FT, N, K, bottom, nV, inputs=_ie_inputs, S=None, shifts=None):
    """Returns the four relative errors (dw_ie, uw_ie in full, then their viewing rows) it has asserted."""
    S = (9 if N <= 33 else 5) if S is None else S
    rng = np.random.default_rng(N * 1000 + K)
    ns = 3 if N % 3 == 0 else 1
    if shifts is None:
        shifts = {1: [2], 9: [-4, -2, -1, 0, 1, 2, 4, S + 3, -(S + 7)]}.get(K, list(range(-35, 35)))
    A, dwf, B, uwf = inputs(N, S, rng, bottom == "shared")
    Aie, aie = 0.05 * rng.random((K, S, N, N)) / N, 0.05 * rng.random((K, S, N))
    Bie, cie = (None, None) if bottom == "null" else (0.05 * rng.random((K, S, N, N)) / N, 0.05 * rng.random((K, S, N)))
    cast = lambda x: None if x is None else x.astype(FT).astype(np.float64)
    uwie_r, dwie_r = MR.level_ie_push_through(np.float64, shifts, *map(cast, (A, B, dwf, uwf, Aie, aie, Bie, cie)))
    row0 = [0, ns * ((N // ns) // 2), N - ns] + [ns * (v % (N // ns)) for v in range(3, nV)]
    wv = rng.uniform(0.1, 1.0, len(row0) * ns)
    dt = torch.float64 if FT == np.float64 else torch.float32
    uwie = torch.zeros((S, ns, nV), dtype=dt, device="cuda")
    dwie = torch.zeros((S, ns, nV), dtype=dt, device="cuda")
    dwief = torch.full((S, N), float("nan"), dtype=dt, device="cuda")
    uwief = torch.full((S, N), float("nan"), dtype=dt, device="cuda")
    _level_ie_call(vsm, FT, N, ns, S, K, shifts, A, B, dwf, uwf, Aie, aie, Bie, cie, row0, wv, uwie, dwie, dwief, uwief)
    tol = 1e-10 if FT == np.float64 else 5e-4
    errs = []
    for got, ref in ((dwief, dwie_r), (uwief, uwie_r)):
        g = got.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(g))
        errs.append(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))
        assert np.max(np.abs(g - ref)) <= tol * np.max(np.abs(ref))
    for got, ref in ((uwie, uwie_r), (dwie, dwie_r)):
        rows = np.stack([np.stack([wv[v + nV * k] * ref[:, row0[v] + k] for v in range(nV)], axis=-1) for k in range(ns)], axis=1)
        g = got.cpu().numpy().astype(np.float64)
        errs.append(np.max(np.abs(g - rows)) / np.max(np.abs(rows)))
        assert np.max(np.abs(g - rows)) <= tol * np.max(np.abs(rows))
    return errs


def test_outputs_finite_with_poisoned_buffers(vsm, arch, monkeypatch):
    """VSM_POISON_WORK fills every work buffer with NaN; the stream outputs are handed over uninitialised."""
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    vsm.CoreRTRaman._work.clear()
    try:
        _, pm = _models(vsm, arch, "IQU", 7, 12, 5, np.float64)
        _, prs = _rs(vsm)
        res = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, LEVELS, streams=True)
    finally:
        vsm.CoreRTRaman._work.clear()
    for name in ("uw", "dw", "uwie", "dwie", "uw_streams", "dw_streams", "uwie_streams", "dwie_streams"):
        assert np.all(np.isfinite(np.asarray(getattr(res, name)))), name


def test_layer_step_and_interaction_counts(vsm, arch, monkeypatch):
    """Per moment: Nz + (Nz - l1) RRS layer steps, L + 1 interactions beyond the layer walks (one bottom per interior level and the
    surface interaction of level 0), one elastic and one inelastic level call per level other than 0."""
    RR, MSR, MS = vsm.CoreRTRaman, vsm.core_rt_ms_raman, vsm.core_rt_ms
    n = dict(layer=0, copy=0, ia=0, lev=0, lev_ie=0)

    def wrap(mod, name, key, pred=None):
        f = getattr(mod, name)

        def g(*a, **kw):
            n[key] += 1
            if pred is not None and pred(a, kw):
                n["copy"] += 1
            return f(*a, **kw)
        monkeypatch.setattr(mod, name, g)

    wrap(RR, "rt_kernel_rrs_", "layer", lambda a, kw: a[11] == 1)
    wrap(RR, "interaction_inelastic_", "ia")
    wrap(MS, "level_radiance_", "lev")
    wrap(MSR, "level_radiance_ie_", "lev_ie")
    _, pm = _models(vsm, arch, "IQU", 7, 8, 6, np.float64, m_max=2)
    _, prs = _rs(vsm)
    levels = [4, 2, 0, 6, 2]
    vsm.CoreRTRaman.rt_run_multisensor(prs, pm, levels)
    Nz, l1, L, moments = 6, 2, 2, 3
    assert n["layer"] == moments * (Nz + (Nz - l1))
    assert n["copy"] == moments * (1 + L)
    assert n["ia"] - (n["layer"] - n["copy"]) == moments * (L + 1)
    assert n["lev"] == n["lev_ie"] == moments * (L + 1)


@pytest.mark.parametrize("pattern", ["01_10_11", "00_01_11"])
def test_nonscattering_layers(vsm, arch, pattern):
    """Columns whose layers leave the _11 interface (the patterns of test_gpu_raman's non-scattering test): rt_run(RRS)'s
    convention for the _00 / _01 / _10 tags in the segments, against the transcription."""
    S, L = 16, 4
    tiny = 1e-22
    tau_rayl = np.tile({"01_10_11": [tiny, 0.04, tiny, 0.03], "00_01_11": [tiny, tiny, 0.04, 0.03]}[pattern], (S, 1))
    om, pm = _models(vsm, arch, "IQU", 7, S, L, np.float64, seed=21, tau_rayl=tau_rayl)
    tags, _ = O.extract_effective_props(O.construct_core_optical_properties(om, 0), np.float64)
    assert list(tags[1:L]) == pattern.split("_")
    ors, prs = _rs(vsm)
    levels = [2, 0, 4, 1, 3]
    ref = MR.ms_raman_reference(om, ors, levels)
    got = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, levels)
    for name, g_list, r_list in zip(("uw", "dw", "uwie", "dwie"), got, ref):
        for i, l in enumerate(levels):
            e = _rel_per_component(g_list[i], r_list[i])
            assert e <= 1e-8, (pattern, name, l, e)
