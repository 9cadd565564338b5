"""GPU tests of the view-row native run (VSM_RUN_VIEW_ROWS, csrc/vsm_native.hip nia_body_src<VW>; core_rt.NATIVE_VIEW_ROWS):
Scene.run with the switch on against the switch off (the plain sources-only run) and against the oracle, at the tolerances of
tests/test_gpu_sources_only.py (1e-12 relative between the runs, 1e-8 against the oracle); the exported T-- / J0- through the C
ABI (equal in the viewing rows, NaN elsewhere); several VZAs, one of them on a Gauss-Legendre node; a graph-captured run."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import vsm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _aer(M):
    return [M.AerosolOptics(M.GreekCoefs(**vars(O.hg_greek(0.7, 12))), 0.95, 0.1),
            M.AerosolOptics(M.GreekCoefs(**vars(O.hg_greek(0.5, 8))), 0.9, 0.0)]


def _scene_kw(kind, S, rng):
    """thin Rayleigh / thick (long series orders and pivoted inverses) / mixed aerosols: the scenes of test_gpu_sources_only.py"""
    if kind == "thick":
        tau_rayl = np.tile(np.array([0.5, 4.0, 30.0]), (S, 1))
        tau_abs = np.tile(np.array([1e-4, 1e-5, 1e-6]), (S, 1)) * (1 + rng.random((S, 1)))
        return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.03, albedo=0.6, m_max=2)
    if kind == "aerosol":
        return dict(tau_rayl=np.tile(np.array([0.03, 0.05, 0.1, 0.2]), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0, (S, 4)),
                    depol=0.03, albedo=0.1, m_max=4, tau_aer=np.array([[0.0, 0.0, 0.2, 0.1], [0.03, 0.0, 0.1, 0.3]]))
    return dict(tau_rayl=np.tile(np.linspace(0.02, 0.3, 3), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0.5, (S, 3)), depol=0.03,
                albedo=0.2, m_max=2)


def _model(vsm, arch, pol, l_trunc, kind, vza, S, seed):
    H = vsm.host_model
    kw = _scene_kw(kind, S, np.random.default_rng(seed))
    extra = dict(aerosol_optics=_aer(H)) if kind == "aerosol" else {}
    return H.model_from_arrays(arch, pol, l_trunc, 40.0, list(vza), [0.0, 35.0, 120.0, 250.0][:len(vza)], **extra, **kw), kw


def _run_both(vsm, arch, monkeypatch, pol, l_trunc, kind, vza=(30.0,), S=5, seed=3):
    model, kw = _model(vsm, arch, pol, l_trunc, kind, vza, S, seed)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_RUN", True)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_SOURCES_ONLY", True)
    out = {}
    for view in (False, True):
        monkeypatch.setattr(vsm.CoreRT, "NATIVE_VIEW_ROWS", view)
        sc = vsm.CoreRT.prepare_scene(model)
        assert sc._native_moments(), "the scene must take the native run"
        sc.compute_hdrf = True
        sc.run()
        torch.cuda.synchronize()
        vsm._lib.check_device_status("view-row run")
        out[view] = sc.results_host_full()
    return model, kw, out


# Nquad = (l_trunc + 5) / 2 with one VZA: N in 13..16 / 40 / 60 / 61..64 and the shapes between (IQU: m = 0 runs (I,Q) + U)
CASES = [
    ("IQU", 35, "thin"),      # N = 60: the C2 shape, <4, 15> + <3, 10>
    ("IQU", 35, "aerosol"),
    ("IQU", 35, "thick"),     # long series orders and pivoted inverses
    ("IQUV", 25, "thin"),     # N = 60, (I,Q) | (U,V) blocks of 30 at m = 0 (mat-vec sources)
    ("IQUV", 25, "thick"),
    ("IQUV", 15, "aerosol"),  # N = 40
    ("IQU", 21, "thin"),      # N = 39 / 26 / 13
    ("IQU", 23, "thick"),     # N = 42 / 28 / 14
    ("IQU", 25, "aerosol"),   # N = 45 / 30 / 15: every block on the mat-vec source path
    ("IQUV", 3, "thin"),      # N = 16
    ("IQUV", 27, "thin"),     # N = 64 / 32
    ("IQU", 37, "thin"),      # N = 63 / 42 / 21
    ("IQU", 37, "thick"),
    ("IQUV", 29, "thin"),     # N = 68: five row tiles, the surface step beyond the native interaction
    ("I", 117, "thin"),       # N = 61
    ("I", 119, "aerosol"),    # N = 62
    ("I", 21, "thin"),        # N = 13
    ("I", 25, "thick"),       # N = 15
]


@pytest.mark.parametrize("pol,l_trunc,kind", CASES)
def test_view_rows_match_sources_only_run(vsm, arch, monkeypatch, pol, l_trunc, kind):
    """R_SFI, T_SFI, hdr and the bhr with NATIVE_VIEW_ROWS on equal the plain sources-only run's up to rounding (1e-12 relative),
    and every output is finite."""
    _, _, out = _run_both(vsm, arch, monkeypatch, pol, l_trunc, kind)
    for k, (a, b) in enumerate(zip(out[True], out[False])):
        a, b = np.asarray(a), np.asarray(b)
        print(pol, l_trunc, kind, k, _rel(a, b) if np.max(np.abs(b)) > 0 else 0.0)
        assert np.all(np.isfinite(a)), k
        if np.max(np.abs(b)) > 0:
            assert _rel(a, b) < 1e-12, (k, _rel(a, b))
    # the viewing rows go through the very operations of the full product (one row tile of it): the same bits
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])


@pytest.mark.parametrize("pol,l_trunc,kind", [("IQU", 35, "thin"), ("IQUV", 25, "thin"), ("IQU", 35, "aerosol"),
                                               ("IQU", 35, "thick"), ("IQU", 21, "thin"), ("IQUV", 27, "thin")])
def test_view_rows_against_oracle(vsm, arch, monkeypatch, pol, l_trunc, kind):
    """The view-row run against the oracle, at the gate of test_gpu_sources_only.py (1e-8 relative)."""
    model, kw, out = _run_both(vsm, arch, monkeypatch, pol, l_trunc, kind, S=3, seed=11)
    extra = dict(aerosols=_aer(O)) if kind == "aerosol" else {}
    Ro, To = O.rt_run(O.build_model(pol, l_trunc, 40.0, [30.0], [0.0], **extra, **kw))
    R, T = out[True][0], out[True][1]
    print(pol, l_trunc, kind, _rel(R, Ro), _rel(T, To))
    assert _rel(R, Ro) < 1e-8 and _rel(T, To) < 1e-8, (_rel(R, Ro), _rel(T, To))


@pytest.mark.parametrize("pol,l_trunc", [("IQU", 31), ("IQUV", 19)])
def test_several_vzas_one_on_a_gauss_legendre_node(vsm, arch, monkeypatch, pol, l_trunc):
    """Three VZAs, one of them a Gauss-Legendre node of the quadrature (an inner row of the blocks, no stream appended for it):
    the switch on against off, and the oracle."""
    probe, _ = _model(vsm, arch, pol, l_trunc, "thin", (30.0,), 2, 1)
    qp = vsm.CoreRT.prepare_scene(probe).qp
    nq0 = (l_trunc + 1) // 2
    gl = float(np.degrees(np.arccos(float(qp.qp_mu[nq0 // 2]))))     # a node of the Gauss-Legendre part
    vza = (gl, 30.0, 55.0)
    model, kw, out = _run_both(vsm, arch, monkeypatch, pol, l_trunc, "thin", vza=vza, S=3, seed=4)
    sc = vsm.CoreRT.prepare_scene(model)
    rows = vsm.CoreRT.view_rows_of(sc.pol, list(vza), sc.qp)
    assert len(rows) == 3 * len(pol) and min(rows) < (nq0 // 2 + 1) * len(pol)
    for k, (a, b) in enumerate(zip(out[True], out[False])):
        a, b = np.asarray(a), np.asarray(b)
        assert np.all(np.isfinite(a)), k
        if np.max(np.abs(b)) > 0:
            assert _rel(a, b) < 1e-12, (k, _rel(a, b))
    Ro, To = O.rt_run(O.build_model(pol, l_trunc, 40.0, list(vza), [0.0, 35.0, 120.0], **kw))
    assert _rel(out[True][0], Ro) < 1e-8 and _rel(out[True][1], To) < 1e-8


def _direct_run(vsm, arch, model, rows, S):
    """vsm_run_create_ex (+ vsm_run_view_rows) -> vsm_run_layer -> vsm_run_export after every layer, per moment."""
    CR = vsm.CoreRT
    sc = CR.prepare_scene(model)
    L = vsm._lib.lib()
    N, ns, dt = sc.N, sc.pol.n, sc.dt
    res = []
    for mom in sc.moments:
        m = int(mom["m"])
        marr, carr = (C.c_int * 1)(m), (C.c_int * 1)(int(sc.coupling[m]))
        nbytes = int(L.vsm_run_workspace_bytes(N, ns, S, 1, carr))
        ws = torch.full((max(nbytes // 8, 2),), float("nan"), dtype=torch.float64, device="cuda")
        q = sc.dq.cstruct()
        run = C.c_void_p()
        vsm._lib.check(L.vsm_run_create_ex_f64(C.byref(q), S, 1, marr, carr, C.c_void_p(ws.data_ptr()), nbytes, 1, C.byref(run)))
        if rows:
            vsm._lib.check(L.vsm_run_view_rows(run, len(rows), (C.c_int * len(rows))(*rows)))
        comp = CR.make_composite_layer(np.float64, arch, (N, N), S)
        steps = []
        try:
            for iz in range(sc.Nz):
                ly = mom["layers"][iz]
                p = ly["props"]
                ncomp = 0 if p.fcomp is None else int(p.fcomp.shape[1])
                zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
                lc = (C.c_int * 1)(sc._layer_coupling(m, iz))
                CR.run_layer_native_(run, 1, int(ly["nd"]), ly["dtau"], p.varpi, ly["tau_sum"], sc.F0, ncomp, zpp, zmp,
                                     0 if ncomp else p.z_stride, p.fcomp, iz == 0, lc, dt)
                cc = (type(comp.cstruct()) * 1)(comp.cstruct())
                vsm._lib.check(L.vsm_run_export_f64(run, cc, None))
                torch.cuda.synchronize()
                steps.append({k: getattr(comp, k).detach().cpu().numpy().copy() for k in ("R_pm", "T_mm", "J0_p", "J0_m")})
        finally:
            L.vsm_run_destroy(run)
        res.append(steps)
    return res


@pytest.mark.parametrize("pol,l_trunc,kind", [("IQU", 35, "thin"), ("IQUV", 25, "thin"), ("IQU", 25, "aerosol"), ("I", 25, "thick"),
                                               ("IQUV", 27, "thin"), ("I", 9, "thin")])
def test_exported_rows(vsm, arch, pol, l_trunc, kind):
    """Through the C ABI, layer by layer: T-- and J0- of a view-row run equal the sources-only run's in the viewing rows (bit for
    bit) and are NaN in every other row; R+- and J0+ are the sources-only run's."""
    S = 3
    model, _ = _model(vsm, arch, pol, l_trunc, kind, (30.0,), S, 7)
    sc = vsm.CoreRT.prepare_scene(model)
    ns = sc.pol.n
    rows = vsm.CoreRT.view_rows_of(sc.pol, [30.0], sc.qp) + [ns * 2 + (ns - 1), 0]      # and two inner rows
    ref = _direct_run(vsm, arch, model, None, S)
    got = _direct_run(vsm, arch, model, rows, S)
    other = [i for i in range(sc.N) if i not in rows]
    for im, (fs, ss) in enumerate(zip(ref, got)):
        for iz, (f, s) in enumerate(zip(fs, ss)):
            for k in ("R_pm", "J0_p"):
                assert np.all(np.isfinite(s[k])) and _rel(s[k], f[k]) < 1e-12, (im, iz, k)
            # (S, column, row) layout tensors of the reference's [N, N, S] arrays: the row index is the last one
            tv, tf = s["T_mm"][:, :, rows], f["T_mm"][:, :, rows]
            assert np.all(np.isfinite(tv)), (im, iz)
            assert float(np.max(np.abs(tv - tf))) <= 1e-12 * float(np.max(np.abs(f["T_mm"]))), (im, iz)
            assert np.array_equal(tv, tf), (im, iz)
            assert np.all(np.isnan(s["T_mm"][:, :, other])), (im, iz)
            jv, jf = s["J0_m"][:, rows], f["J0_m"][:, rows]
            assert np.all(np.isfinite(jv)), (im, iz)
            assert float(np.max(np.abs(jv - jf))) <= 1e-12 * max(float(np.max(np.abs(f["J0_m"]))), 1e-300), (im, iz)
            assert np.array_equal(jv, jf), (im, iz)
            assert np.all(np.isnan(s["J0_m"][:, other])), (im, iz)


def test_import_round_trip(vsm, arch):
    """vsm_run_export of a view-row run after layer k, vsm_run_import into a fresh view-row run, the remaining layers: the viewing
    rows of T-- / J0-, R+- and J0+ equal those of the uninterrupted run (the same kernels on the same values: bit for bit)."""
    CR, S, k = vsm.CoreRT, 3, 2
    model, _ = _model(vsm, arch, "IQU", 35, "aerosol", (30.0,), S, 13)
    sc = CR.prepare_scene(model)
    L = vsm._lib.lib()
    N, ns, dt = sc.N, sc.pol.n, sc.dt
    rows = CR.view_rows_of(sc.pol, [30.0], sc.qp) + [4]
    other = [i for i in range(N) if i not in rows]
    rarr = (C.c_int * len(rows))(*rows)
    for mom in sc.moments:
        m = int(mom["m"])
        marr, carr = (C.c_int * 1)(m), (C.c_int * 1)(int(sc.coupling[m]))
        nbytes = int(L.vsm_run_workspace_bytes(N, ns, S, 1, carr))
        q = sc.dq.cstruct()

        def open_run():
            ws = torch.full((max(nbytes // 8, 2),), float("nan"), dtype=torch.float64, device="cuda")
            run = C.c_void_p()
            vsm._lib.check(L.vsm_run_create_ex_f64(C.byref(q), S, 1, marr, carr, C.c_void_p(ws.data_ptr()), nbytes, 1, C.byref(run)))
            vsm._lib.check(L.vsm_run_view_rows(run, len(rows), rarr))
            return run, ws

        def layers(run, first, end):
            for iz in range(first, end):
                ly = mom["layers"][iz]
                p = ly["props"]
                ncomp = 0 if p.fcomp is None else int(p.fcomp.shape[1])
                zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
                lc = (C.c_int * 1)(sc._layer_coupling(m, iz))
                CR.run_layer_native_(run, 1, int(ly["nd"]), ly["dtau"], p.varpi, ly["tau_sum"], sc.F0, ncomp, zpp, zmp,
                                     0 if ncomp else p.z_stride, p.fcomp, iz == 0, lc, dt)

        def export(run):
            comp = CR.make_composite_layer(np.float64, arch, (N, N), S)
            cc = (type(comp.cstruct()) * 1)(comp.cstruct())
            vsm._lib.check(L.vsm_run_export_f64(run, cc, None))
            torch.cuda.synchronize()
            return comp, cc

        run, ws = open_run()
        try:
            layers(run, 0, sc.Nz)
            ref, _ = export(run)
        finally:
            L.vsm_run_destroy(run)
        run, ws = open_run()
        try:
            layers(run, 0, k)
            mid, cc = export(run)
        finally:
            L.vsm_run_destroy(run)
        run, ws2 = open_run()
        try:
            vsm._lib.check(L.vsm_run_import_f64(run, cc, None))
            assert L.vsm_run_view_rows(run, len(rows), rarr) != 0      # (not after an import)
            layers(run, k, sc.Nz)
            got, _ = export(run)
        finally:
            L.vsm_run_destroy(run)
        h = lambda t: t.detach().cpu().numpy()
        assert np.array_equal(h(got.R_pm), h(ref.R_pm)) and np.array_equal(h(got.J0_p), h(ref.J0_p)), m
        assert np.all(np.isfinite(h(ref.T_mm)[:, :, rows])) and np.all(np.isfinite(h(ref.J0_m)[:, rows])), m
        assert np.array_equal(h(got.T_mm)[:, :, rows], h(ref.T_mm)[:, :, rows]), m
        assert np.array_equal(h(got.J0_m)[:, rows], h(ref.J0_m)[:, rows]), m
        assert np.all(np.isnan(h(got.T_mm)[:, :, other])) and np.all(np.isnan(h(got.J0_m)[:, other])), m


def test_graph_captured_run(vsm, arch, monkeypatch):
    """A view-row Scene.run captured into a graph and replayed gives the eager run's outputs (a captured run keeps the dense
    products: the zero-weight tail is not taken under capture, so up to rounding)."""
    model, _ = _model(vsm, arch, "IQU", 35, "thin", (30.0, 50.0), 4, 9)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_RUN", True)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_SOURCES_ONLY", True)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_VIEW_ROWS", True)
    sc = vsm.CoreRT.prepare_scene(model)
    sc.compute_hdrf = True
    sc.run()
    torch.cuda.synchronize()
    eager = [np.asarray(x).copy() for x in sc.results_host_full()]
    sc.R_SFI.zero_()
    sc.run_graph()                      # (warm-up on the capture's own stream, capture, replay)
    sc.R_SFI.zero_()
    sc.run_graph()                      # (replay alone)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("captured view-row run")
    for k, (a, b) in enumerate(zip(sc.results_host_full(), eager)):
        a, b = np.asarray(a), np.asarray(b)
        assert np.all(np.isfinite(a)), k
        if np.max(np.abs(b)) > 0:
            assert _rel(a, b) < 1e-12, (k, _rel(a, b))
