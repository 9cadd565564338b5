"""GPU tests of the identity surface step of the native runs (core_rt.NATIVE_IDENTITY_SURFACE; vsm_run_surface,
vsm_run_export_sources, vsm_run_guard_once, vsm_run_counters of csrc/vsm_native.hip): a LambertianSurfaceScalar layer at m >= 1 is
r = 0, t = I, j = 0, and interaction!(_11) with it adds exact zeros to everything read below it -- so Scene.run with the switch on
(no interaction, J0+- exported alone) must equal the switch off (full export + interaction for every moment) under np.array_equal,
on the smallest shapes that take each path: Stokes_IQU, N = 24 (the (I,Q) block of m = 0 has n = 16: no spare rider columns) and
N = 18 (n = 12 / 6 / 18), 3 layers, S = 3, m = 0 .. 2."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

S, GEO = 3, (40.0, [30.0], [0.0])
LTS = [11, 7]          # Nquad = (l_trunc + 5) / 2 = 8 / 6: N = 24 / 18
OUT = ("R", "T", "hdr", "bhr_uw", "bhr_dw")


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _kw(seed=5):
    rng = np.random.default_rng(seed)
    return dict(tau_rayl=np.tile(np.linspace(0.02, 0.3, 3), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0.5, (S, 3)), depol=0.03,
                albedo=0.2, m_max=2)


def _model(vsm, arch, l_trunc, surface=None, sources=None):
    return vsm.host_model.model_from_arrays(arch, "IQU", l_trunc, *GEO, surface=surface, sources=sources, **_kw())


def _run(vsm, monkeypatch, model, on, reference_order=False, streams=None, graph=False):
    """Scene.run with the switch `on`: (outputs, counters, scene)."""
    CR = vsm.CoreRT
    for k in ("NATIVE_RUN", "NATIVE_SOURCES_ONLY", "NATIVE_VIEW_ROWS", "NATIVE_DROPIN"):
        monkeypatch.setattr(CR, k, True)
    monkeypatch.setattr(CR, "REFERENCE_ORDER", reference_order)
    monkeypatch.setattr(CR, "NATIVE_IDENTITY_SURFACE", on)
    sc = CR.prepare_scene(model)
    assert reference_order or len(sc._native_moments()) == 3, "the scene must take the native run"
    sc.compute_hdrf = True
    if graph:
        sc.run_graph()
        sc.run_graph()
    else:
        sc.run(streams=streams)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("identity surface run")
    counts = sc.run_counters()
    full = sc.results_host_full()
    out = dict(R=full[0], T=full[1], hdr=full[4], bhr_uw=full[5], bhr_dw=full[6])
    return out, counts, sc


def _assert_equal(a, b):
    for k in OUT:
        assert np.all(np.isfinite(a[k])), k
        assert np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k] - b[k]))))


@pytest.mark.parametrize("reference_order", [False, True])
@pytest.mark.parametrize("l_trunc", LTS)
def test_scalar_lambertian_skips_the_identity_steps(vsm, arch, monkeypatch, l_trunc, reference_order):
    """Scalar Lambertian: the outputs with the switch on equal the switch off bit for bit; on: 1 surface interaction, 1 full export
    and 2 source-only exports per run (off: 3, 3, 0) -- on the native walk and on the REFERENCE_ORDER drop-in walk."""
    model = _model(vsm, arch, l_trunc)
    off, c_off, _ = _run(vsm, monkeypatch, model, False, reference_order)
    on, c_on, _ = _run(vsm, monkeypatch, model, True, reference_order)
    print(l_trunc, reference_order, c_off, c_on)
    _assert_equal(on, off)
    assert (c_on["surface_interactions"], c_on["exports_full"], c_on["exports_src"]) == (1, 1, 2), c_on
    assert (c_off["surface_interactions"], c_off["exports_full"], c_off["exports_src"]) == (3, 3, 0), c_off
    # the guard of the masks: once per run of the scene's own walk, once per layer step on the drop-in registry (3 moments x 3)
    assert c_on["guard_launches"] == c_off["guard_launches"] == (9 if reference_order else 1), (c_on, c_off)


@pytest.mark.parametrize("l_trunc", LTS)
def test_streams_walk_exports_the_whole_composite(vsm, arch, monkeypatch, l_trunc):
    """streams=[]: the caller reads R-+ / T++ -- full exports, no interaction for m >= 1; the clones equal the switch off."""
    model = _model(vsm, arch, l_trunc)
    st_off, st_on = [], []
    off, c_off, _ = _run(vsm, monkeypatch, model, False, streams=st_off)
    on, c_on, _ = _run(vsm, monkeypatch, model, True, streams=st_on)
    _assert_equal(on, off)
    assert (c_on["surface_interactions"], c_on["exports_full"], c_on["exports_src"]) == (1, 3, 0), c_on
    assert [d["m"] for d in st_on] == [d["m"] for d in st_off] == [0, 1, 2]
    for a, b in zip(st_on, st_off):
        for k in ("R_mp", "T_pp", "J0_m", "J0_p"):
            x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
            assert np.all(np.isfinite(x)), (a["m"], k)
            assert np.array_equal(x, y), (a["m"], k)


@pytest.mark.parametrize("l_trunc", LTS)
def test_graph_replay(vsm, arch, monkeypatch, l_trunc):
    """run_graph(): the captured launch sequence with the switch on replays to the outputs of the captured one with it off."""
    model = _model(vsm, arch, l_trunc)
    off, _, _ = _run(vsm, monkeypatch, model, False, graph=True)
    on, c_on, _ = _run(vsm, monkeypatch, model, True, graph=True)
    _assert_equal(on, off)
    assert (c_on["surface_interactions"], c_on["exports_src"]) == (1, 2), c_on


def _other_surfaces(H):
    B = np.linspace(0.5, 1.5, S)
    return {
        "legendre": dict(surface=H.LambertianSurfaceLegendre([0.2, 0.05])),
        "rpv": dict(surface=H.rpvSurfaceScalar(0.1, 0.1, 0.7, -0.1)),
        "coxmunk": dict(surface=H.CoxMunkSurface(5.0)),
        "sif": dict(sources=(H.SolarBeam(), H.SurfaceSIF(np.linspace(0.01, 0.03, S)))),
        "emission": dict(sources=(H.SolarBeam(), H.SurfaceEmission(B_surface=B))),
    }


@pytest.mark.parametrize("which", ["legendre", "rpv", "coxmunk", "sif", "emission"])
def test_no_skip_over_other_surfaces_and_surface_sources(vsm, arch, monkeypatch, which):
    """The spectral Lambertian builder (t = 0 at m >= 1), the BRDF surfaces and a scene with a surface source keep the full surface
    step at every moment: 3 interactions with the switch on, and the switch-off result bit for bit."""
    model = _model(vsm, arch, 11, **_other_surfaces(vsm.host_model)[which])
    off, c_off, _ = _run(vsm, monkeypatch, model, False)
    on, c_on, _ = _run(vsm, monkeypatch, model, True)
    _assert_equal(on, off)
    assert (c_on["surface_interactions"], c_on["exports_full"], c_on["exports_src"]) == (3, 3, 0), (which, c_on)
    assert c_off == c_on


@pytest.mark.parametrize("l_trunc", LTS)
def test_matrix_read_after_a_skipped_step_exports_the_composite(vsm, arch, monkeypatch, l_trunc):
    """After a skipped step the composite's matrices are still in the run: reading comp.R_pm exports them (one more full export)
    and gives the array of the switch-off run, whose interaction added exact zeros to it."""
    model = _model(vsm, arch, l_trunc)
    _, _, sc_off = _run(vsm, monkeypatch, model, False)
    _, c_on, sc_on = _run(vsm, monkeypatch, model, True)
    for im in (1, 2):
        comp = sc_on._composites[im]
        assert comp._native is not None and comp._vectors_current
        jp = comp.J0_p.cpu().numpy()                        # (the vectors are current: no export)
        assert comp._native is not None
        R_on = comp.R_pm.cpu().numpy()
        assert comp._native is None and not comp._vectors_current
        R_off = sc_off._composites[im].R_pm.cpu().numpy()
        assert np.all(np.isfinite(R_on)) and np.array_equal(R_on, R_off), im
        assert np.array_equal(jp, sc_off._composites[im].J0_p.cpu().numpy()), im
        assert np.array_equal(comp.J0_m.cpu().numpy(), sc_off._composites[im].J0_m.cpu().numpy(), equal_nan=True), im
    after = sc_on.run_counters()
    assert after["exports_full"] == c_on["exports_full"] + 2 and after["surface_interactions"] == 1, after


def _counters(L, run):
    c = (C.c_int * 4)()
    assert L.vsm_run_counters(run, c) == 0
    return list(c)


def test_guard_and_source_export_through_the_c_abi(vsm, arch):
    """Direct callers keep the guard of the masks on every layer step; vsm_run_guard_once leaves the first one; vsm_run_import ends
    it.  vsm_run_export_sources writes J0+- as vsm_run_export does and touches no matrix."""
    CR, L = vsm.CoreRT, vsm._lib.lib()
    sc = CR.prepare_scene(_model(vsm, arch, 11))
    N, ns, dt = sc.N, sc.pol.n, sc.dt
    mom = sc.moments[1]
    m = int(mom["m"])
    marr, carr = (C.c_int * 1)(m), (C.c_int * 1)(int(sc.coupling[m]))
    nbytes = int(L.vsm_run_workspace_bytes(N, ns, S, 1, carr))
    q = sc.dq.cstruct()

    def open_run(once):
        ws = torch.full((max(nbytes // 8, 2),), float("nan"), dtype=torch.float64, device="cuda")
        run = C.c_void_p()
        vsm._lib.check(L.vsm_run_create_ex_f64(C.byref(q), S, 1, marr, carr, C.c_void_p(ws.data_ptr()), nbytes, 1, C.byref(run)))
        if once:
            vsm._lib.check(L.vsm_run_guard_once(run))
        return run, ws

    def layers(run, first, end):
        for iz in range(first, end):
            ly = mom["layers"][iz]
            p = ly["props"]
            zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
            lc = (C.c_int * 1)(sc._layer_coupling(m, iz))
            CR.run_layer_native_(run, 1, int(ly["nd"]), ly["dtau"], p.varpi, ly["tau_sum"], sc.F0, 0, zpp, zmp, p.z_stride, None,
                                 iz == 0, lc, dt)

    run, ws = open_run(False)
    try:
        layers(run, 0, sc.Nz)
        assert _counters(L, run) == [0, 0, 0, sc.Nz]
        assert L.vsm_run_guard_once(run) != 0                 # (not after a layer step)
    finally:
        L.vsm_run_destroy(run)
    run, ws = open_run(True)
    try:
        layers(run, 0, sc.Nz)
        assert _counters(L, run) == [0, 0, 0, 1]
        full = CR.make_composite_layer(np.float64, arch, (N, N), S)
        cf = full._cstruct_raw()
        vsm._lib.check(L.vsm_run_export_moment_f64(run, 0, C.byref(cf), None))
        src = CR.make_composite_layer(np.float64, arch, (N, N), S)
        for t in src._arr.values():
            t.fill_(7.0)
        cs = src._cstruct_raw()
        vsm._lib.check(L.vsm_run_export_sources_f64(run, 0, C.byref(cs), None))
        assert L.vsm_run_export_sources_f64(run, 1, C.byref(cs), None) != 0      # (the run has one moment)
        torch.cuda.synchronize()
        assert _counters(L, run) == [1, 1, 0, 1]
        h = lambda t: t.cpu().numpy()
        assert np.all(np.isfinite(h(full._arr["J0_p"])))
        for k in ("J0_p", "J0_m"):
            assert np.array_equal(h(src._arr[k]), h(full._arr[k]), equal_nan=True), k
        for k in ("R_mp", "R_pm", "T_pp", "T_mm"):
            assert np.all(h(src._arr[k]) == 7.0), k
        # a run that continues from imported arrays: guarded on every layer step again
        run2, ws2 = open_run(True)
        try:
            vsm._lib.check(L.vsm_run_import_f64(run2, (type(cf) * 1)(cf), None))
            layers(run2, 1, sc.Nz)
            assert _counters(L, run2) == [0, 0, 0, sc.Nz - 1]
        finally:
            L.vsm_run_destroy(run2)
    finally:
        L.vsm_run_destroy(run)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("guard test")
