"""GPU tests of the zero-weight tail of the FP64 native run (vsm_run_create_ex with VSM_RUN_ZW_TAIL, core_rt.NATIVE_ZW_TAIL): the
products of the layer steps skip the k-steps of the zero-weight VZA / SZA streams and add their diagonal terms instead.  Against
the dense run on the same scenes (1e-12 relative) and against the oracle at the gates of the existing parity tests."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import vsm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
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
    if kind == "thick":   # long series orders, order 7 and pivoted inverses
        tau_rayl = np.tile(np.array([0.5, 4.0, 30.0]), (S, 1))
        tau_abs = np.tile(np.array([1e-4, 1e-5, 1e-6]), (S, 1)) * (1 + rng.random((S, 1)))
        return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.03, albedo=0.6, m_max=2)
    if kind == "aerosol":   # per-point Z, all moments
        return dict(tau_rayl=np.tile(np.array([0.03, 0.05, 0.1, 0.2]), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0, (S, 4)),
                    depol=0.03, albedo=0.1, m_max=4, tau_aer=np.array([[0.0, 0.0, 0.2, 0.1], [0.03, 0.0, 0.1, 0.3]]))
    return dict(tau_rayl=np.tile(np.linspace(0.02, 0.3, 3), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0.5, (S, 3)), depol=0.03,
                albedo=0.2, m_max=2)


def _gl_angle(l_trunc, k):
    x, _ = O.gauleg((l_trunc + 2) // 2, 0.0, 1.0)
    return float(np.degrees(np.arccos(x[k])))


def _run(vsm, arch, monkeypatch, pol, l_trunc, kind, sza, vza, streams, zw, S=5, seed=3, FT=np.float64):
    H = vsm.host_model
    kw = _scene_kw(kind, S, np.random.default_rng(seed))
    extra = dict(aerosol_optics=_aer(H)) if kind == "aerosol" else {}
    model = H.model_from_arrays(arch, pol, l_trunc, sza, vza, [0.0] * len(vza), float_type=FT, **extra, **kw)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_RUN", True)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_ZW_TAIL", zw)
    sc = vsm.CoreRT.prepare_scene(model)
    assert sc._native_moments(), "the scene must take the native run"
    if streams:
        out = [x.detach().cpu().numpy().copy() for x in sc.run(streams=[])]
    else:
        sc.compute_hdrf = True
        sc.run()
        torch.cuda.synchronize()
        out = [np.asarray(x) for x in sc.results_host_full()]
    vsm._lib.check_device_status("zero-weight tail run")
    return model, out


@pytest.mark.parametrize("pol,l_trunc,kind,sza,vza", [
    ("IQU", 35, "thin", 40.0, [30.0]),                 # N = 60: <4, 15> dense, m = 0 <3, 10> + <2, 5> (the C2 shape)
    ("IQU", 35, "aerosol", 40.0, [30.0]),
    ("IQU", 35, "thick", 40.0, [30.0]),
    ("I", 35, "thin", 40.0, [30.0]),
    ("I", 27, "thick", 40.0, [30.0]),                   # N = 16: one row tile, the mat-vec source path
    ("IQUV", 21, "thin", 40.0, [30.0]),                 # N = 52 / 26
    ("IQU", 25, "thin", 40.0, [30.0]),                  # N = 45 / 30 / 15: mat-vec source path
    ("IQU", 35, "thin", 40.0, [10.0, 30.0, 60.0]),      # a tail of several k-steps
    ("IQU", 35, "thin", "gl", "gl"),                    # VZA and SZA on Gauss-Legendre nodes: no zero-weight node
])
@pytest.mark.parametrize("streams", [False, True])
def test_tail_matches_dense_run(vsm, arch, monkeypatch, pol, l_trunc, kind, sza, vza, streams):
    """NATIVE_ZW_TAIL on against off: every output within 1e-12 relative (sources-only and full runs)."""
    if sza == "gl":
        sza, vza = _gl_angle(l_trunc, 4), [_gl_angle(l_trunc, 4)]
    _, on = _run(vsm, arch, monkeypatch, pol, l_trunc, kind, sza, vza, streams, True)
    _, off = _run(vsm, arch, monkeypatch, pol, l_trunc, kind, sza, vza, streams, False)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.all(np.isfinite(a)), k
        if np.max(np.abs(b)) > 0:
            assert _rel(a, b) < 1e-12, (k, _rel(a, b))


@pytest.mark.parametrize("kind", ["thin", "thick"])
def test_tail_against_oracle(vsm, arch, monkeypatch, kind):
    """The C2-shaped scene with the tail against the oracle, at the gates of the existing parity tests."""
    model, out = _run(vsm, arch, monkeypatch, "IQU", 35, kind, 40.0, [30.0], False, True, S=4, seed=11)
    kw = _scene_kw(kind, 4, np.random.default_rng(11))
    Ro, To = O.rt_run(O.build_model("IQU", 35, 40.0, [30.0], [0.0], **kw))
    R, T = out[0], out[1]
    assert _rel(R, Ro) < 1e-8 and _rel(T, To) < 1e-8, (_rel(R, Ro), _rel(T, To))


def test_float32_run_ignores_the_flag(vsm, arch, monkeypatch):
    """A Float32 model's native run accepts VSM_RUN_ZW_TAIL and keeps its dense products: the same bits."""
    _, on = _run(vsm, arch, monkeypatch, "IQU", 35, "thin", 40.0, [30.0], False, True, FT=np.float32)
    _, off = _run(vsm, arch, monkeypatch, "IQU", 35, "thin", 40.0, [30.0], False, False, FT=np.float32)
    for a, b in zip(on, off):
        assert np.array_equal(a, b, equal_nan=True)


def _direct(vsm, arch, flags, import_at=None, S=4, seed=7):
    """vsm_run_create_ex -> vsm_run_layer per layer -> vsm_run_export; import_at: after that layer the exported composite is
    imported back (vsm_run_import: from there on the run's products are dense)."""
    H, CR = vsm.host_model, vsm.CoreRT
    kw = _scene_kw("thin", S, np.random.default_rng(seed))
    model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], **kw)
    sc = CR.prepare_scene(model)
    L = vsm._lib.lib()
    N, ns, dt = sc.N, sc.pol.n, sc.dt
    res = []
    for mom in sc.moments:
        m = int(mom["m"])
        marr, carr = (C.c_int * 1)(m), (C.c_int * 1)(int(sc.coupling[m]))
        nbytes = int(L.vsm_run_workspace_bytes(N, ns, S, 1, carr))
        ws = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device="cuda")
        q = sc.dq.cstruct()
        run = C.c_void_p()
        vsm._lib.check(L.vsm_run_create_ex_f64(C.byref(q), S, 1, marr, carr, C.c_void_p(ws.data_ptr()), nbytes, flags, C.byref(run)))
        comp = CR.make_composite_layer(np.float64, arch, (N, N), S)
        steps = []
        try:
            for iz in range(sc.Nz):
                ly = mom["layers"][iz]
                p = ly["props"]
                zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
                lc = (C.c_int * 1)(sc._layer_coupling(m, iz))
                CR.run_layer_native_(run, 1, int(ly["nd"]), ly["dtau"], p.varpi, ly["tau_sum"], sc.F0, 0, zpp, zmp, p.z_stride,
                                     p.fcomp, iz == 0, lc, dt)
                cc = (type(comp.cstruct()) * 1)(comp.cstruct())
                vsm._lib.check(L.vsm_run_export_f64(run, cc, None))
                if import_at == iz:
                    vsm._lib.check(L.vsm_run_import_f64(run, cc, None))
                torch.cuda.synchronize()
                steps.append({k: getattr(comp, k).detach().cpu().numpy().copy()
                              for k in ("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m")})
        finally:
            L.vsm_run_destroy(run)
        res.append(steps)
    return res


@pytest.mark.parametrize("import_at", [None, 0, 1])
def test_direct_run_layer_by_layer_and_import(vsm, arch, import_at):
    """Through the C ABI, layer by layer, full and sources-only: the composite of a run with the flag equals the dense run's to
    1e-12 relative, also when the run continues from imported arrays."""
    for base in (0, 1):
        dense = _direct(vsm, arch, base)
        tail = _direct(vsm, arch, base | 2, import_at=import_at)
        for im, (fs, ts) in enumerate(zip(dense, tail)):
            for iz, (f, t) in enumerate(zip(fs, ts)):
                for k in (("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m") if base == 0 else ("R_pm", "T_mm", "J0_p", "J0_m")):
                    assert np.all(np.isfinite(t[k])), (base, im, iz, k)
                    if np.max(np.abs(f[k])) > 0:
                        assert _rel(t[k], f[k]) < 1e-12, (base, im, iz, k, _rel(t[k], f[k]))
