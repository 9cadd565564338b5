"""GPU tests of the sources-only native run (vsm_run_create_ex with VSM_RUN_SOURCES_ONLY, csrc/vsm_native.hip nia_body_src): the
layer steps keep R+-, T-- and J0+- of the composite only (interaction.jl:207-266 re-associated around (I - r-+ R+-)^-1).  Against
the full run on the same scenes: the kept members and R_SFI / T_SFI up to rounding, R-+ / T++ exported as NaN, and the paths that
read R-+ / T++ (rt_run_streams, rt_kernel_ called on a caller's composite, traced runs) still on full runs."""
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
    """(polarization, l_trunc, model keywords): thin / thick (long series orders and pivoted inverses) / mixed aerosols."""
    if kind == "thick":
        tau_rayl = np.tile(np.array([0.5, 4.0, 30.0]), (S, 1))
        tau_abs = np.tile(np.array([1e-4, 1e-5, 1e-6]), (S, 1)) * (1 + rng.random((S, 1)))
        return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.03, albedo=0.6, m_max=2)
    if kind == "aerosol":
        return dict(tau_rayl=np.tile(np.array([0.03, 0.05, 0.1, 0.2]), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0, (S, 4)),
                    depol=0.03, albedo=0.1, m_max=4, tau_aer=np.array([[0.0, 0.0, 0.2, 0.1], [0.03, 0.0, 0.1, 0.3]]))
    return dict(tau_rayl=np.tile(np.linspace(0.02, 0.3, 3), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, 0.5, (S, 3)), depol=0.03,
                albedo=0.2, m_max=2)


def _run_both(vsm, arch, monkeypatch, pol, l_trunc, kind, S=5, seed=3):
    H = vsm.host_model
    kw = _scene_kw(kind, S, np.random.default_rng(seed))
    extra = dict(aerosol_optics=_aer(H)) if kind == "aerosol" else {}
    model = H.model_from_arrays(arch, pol, l_trunc, 40.0, [30.0], [0.0], **extra, **kw)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_RUN", True)
    out = {}
    for src in (False, True):
        monkeypatch.setattr(vsm.CoreRT, "NATIVE_SOURCES_ONLY", src)
        sc = vsm.CoreRT.prepare_scene(model)
        assert sc._native_moments(), "the scene must take the native run"
        sc.compute_hdrf = True
        sc.run()
        torch.cuda.synchronize()
        vsm._lib.check_device_status("sources-only run")
        out[src] = sc.results_host_full()
    return model, out


# (one viewing angle: Nquad = (l_trunc + 5) / 2; the blocks of IQU: m = 0 (I,Q) of 2 Nquad rows + U of Nquad, m >= 1 dense)
@pytest.mark.parametrize("pol,l_trunc,kind", [
    ("IQU", 35, "thin"),      # N = 60: <4, 15> dense, m = 0 <3, 10> + <2, 5> (the C2 shape)
    ("IQU", 25, "thin"),      # N = 45 / 30 / 15: every block on the mat-vec source path (no spare column)
    ("IQU", 21, "thin"),      # N = 39 / 26 / 13
    ("I", 27, "thin"),        # N = 16: one row tile without spare columns
    ("I", 9, "thin"),         # N = 7: one row tile with riders
    ("IQUV", 21, "thin"),     # N = 52: four row tiles; m = 0 two blocks of 26
    ("IQUV", 29, "thin"),     # N = 68: five row tiles
    ("IQU", 35, "thick"),     # long series orders and pivoted inverses
    ("I", 27, "thick"),
    ("IQU", 21, "aerosol"),   # two aerosols mixed per point, more moments
])
def test_sources_only_matches_full_run(vsm, arch, monkeypatch, pol, l_trunc, kind):
    """R_SFI, T_SFI, ieR/ieT, hdr and the bhr of a sources-only run equal the full run's up to rounding (1e-12 relative)."""
    _, out = _run_both(vsm, arch, monkeypatch, pol, l_trunc, kind)
    for k, (a, b) in enumerate(zip(out[True], out[False])):
        a, b = np.asarray(a), np.asarray(b)
        assert np.all(np.isfinite(a)), k
        if np.max(np.abs(b)) > 0:
            assert _rel(a, b) < 1e-12, (k, _rel(a, b))


def test_sources_only_against_oracle(vsm, arch, monkeypatch):
    """The C2-shaped scene (IQU, N = 60) on the sources-only run against the oracle, at the gates of the existing parity tests."""
    model, out = _run_both(vsm, arch, monkeypatch, "IQU", 35, "thin", S=4, seed=11)
    kw = _scene_kw("thin", 4, np.random.default_rng(11))
    Ro, To = O.rt_run(O.build_model("IQU", 35, 40.0, [30.0], [0.0], **kw))
    R, T = out[True][0], out[True][1]
    assert _rel(R, Ro) < 1e-8 and _rel(T, To) < 1e-8, (_rel(R, Ro), _rel(T, To))


def _direct_run(vsm, arch, pol, l_trunc, kind, flags, S=4, seed=7):
    """vsm_run_create_ex -> vsm_run_layer -> vsm_run_export after every layer; returns the exported composites per layer."""
    H, CR = vsm.host_model, vsm.CoreRT
    kw = _scene_kw(kind, S, np.random.default_rng(seed))
    model = H.model_from_arrays(arch, pol, l_trunc, 40.0, [30.0], [0.0], **kw)
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
                ncomp = 0 if p.fcomp is None else int(p.fcomp.shape[1])
                zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
                lc = (C.c_int * 1)(sc._layer_coupling(m, iz))
                CR.run_layer_native_(run, 1, int(ly["nd"]), ly["dtau"], p.varpi, ly["tau_sum"], sc.F0, ncomp, zpp, zmp,
                                     0 if ncomp else p.z_stride, p.fcomp, iz == 0, lc, dt)
                cc = (type(comp.cstruct()) * 1)(comp.cstruct())
                vsm._lib.check(L.vsm_run_export_f64(run, cc, None))
                torch.cuda.synchronize()
                steps.append({k: getattr(comp, k).detach().cpu().numpy().copy()
                              for k in ("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m")})
        finally:
            L.vsm_run_destroy(run)
        res.append(steps)
    return res


@pytest.mark.parametrize("pol,l_trunc,kind", [("IQU", 35, "thin"), ("IQU", 25, "thin"), ("I", 27, "thick"), ("IQUV", 21, "thin"),
                                               ("I", 9, "thin")])
def test_direct_run_kept_members_and_poisoned_ones(vsm, arch, pol, l_trunc, kind):
    """Through the C ABI, layer by layer: R+-, T-- and J0+- of a sources-only run equal the full run's (1e-12 relative); its R-+
    and T++ come out of vsm_run_export as NaN (never stale values)."""
    full = _direct_run(vsm, arch, pol, l_trunc, kind, 0)
    src = _direct_run(vsm, arch, pol, l_trunc, kind, 1)
    for im, (fs, ss) in enumerate(zip(full, src)):
        for iz, (f, s) in enumerate(zip(fs, ss)):
            for k in ("R_pm", "T_mm", "J0_p", "J0_m"):
                assert np.all(np.isfinite(s[k])), (im, iz, k)
                if np.max(np.abs(f[k])) > 0:
                    assert _rel(s[k], f[k]) < 1e-12, (im, iz, k, _rel(s[k], f[k]))
            for k in ("R_mp", "T_pp"):
                assert np.all(np.isnan(s[k])), (im, iz, k)
                assert np.all(np.isfinite(f[k])), (im, iz, k)


def test_unknown_run_flags_are_refused(vsm, arch):
    H = vsm.host_model
    model = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=np.full((2, 2), 0.1), tau_abs=np.full((2, 2), 0.01),
                                depol=0.03, albedo=0.1, m_max=1)
    sc = vsm.CoreRT.prepare_scene(model)
    L = vsm._lib.lib()
    ws = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    q = sc.dq.cstruct()
    run = C.c_void_p()
    rc = L.vsm_run_create_ex_f64(C.byref(q), 2, 1, (C.c_int * 1)(0), (C.c_int * 1)(-1), C.c_void_p(ws.data_ptr()), 8 << 16, 6,
                                 C.byref(run))
    assert rc != 0


def test_mode_selection(vsm, arch, monkeypatch):
    """Scene.run picks sources-only runs without `streams` only (its REFERENCE_ORDER walk included: the registry's runs then serve
    Scene.run alone); rt_run_streams, traced runs and rt_kernel_ on a caller's composite create full runs.  rt_run_streams returns
    the same R-+ / T++ with the switch on and off."""
    H, CR = vsm.host_model, vsm.CoreRT
    kw = _scene_kw("thin", 3, np.random.default_rng(5))
    model = H.model_from_arrays(arch, "IQU", 21, 40.0, [30.0], [0.0], **kw)
    seen = []
    orig = vsm._lib.call

    def spy(name, dtype, *args):
        if name == "vsm_run_create_ex":
            seen.append(("ex", int(args[7])))
        elif name == "vsm_run_create":
            seen.append(("plain", -1))
        return orig(name, dtype, *args)

    monkeypatch.setattr(vsm._lib, "call", spy)
    monkeypatch.setattr(CR, "NATIVE_RUN", True)
    monkeypatch.setattr(CR, "NATIVE_SOURCES_ONLY", True)
    CR.rt_run(model)
    assert seen and all(s == ("ex", 1) for s in seen), seen
    seen.clear()
    st_on = CR.rt_run_streams(model)
    assert seen and all(s[1] == 0 for s in seen), seen
    seen.clear()
    CR.rt_run(model, trace=[])
    assert all(s[1] == 0 for s in seen), seen
    seen.clear()
    monkeypatch.setattr(CR, "REFERENCE_ORDER", True)
    Rr, Tr = CR.rt_run(model)
    assert seen and all(s == ("ex", 1) for s in seen), seen         # (the drop-in registry, driven by Scene.run)
    seen.clear()
    CR.rt_run_streams(model)
    assert seen and all(s == ("ex", 0) for s in seen), seen
    monkeypatch.setattr(CR, "REFERENCE_ORDER", False)
    Rn, Tn = CR.rt_run(model)
    assert np.array_equal(Rr, Rn) and np.array_equal(Tr, Tn)           # (the same kernels, the same bits)
    seen.clear()
    monkeypatch.setattr(CR, "NATIVE_SOURCES_ONLY", False)
    CR.rt_run(model)
    assert seen and all(s == ("ex", 0) for s in seen), seen
    seen.clear()
    sc = CR.prepare_scene(model)                                        # rt_kernel_ on a composite of its caller: full runs
    monkeypatch.setattr(CR, "NATIVE_SOURCES_ONLY", True)
    comp = CR.make_composite_layer(sc.FT, arch, (sc.N, sc.N), sc.S)
    mom = sc.moments[1]
    for iz, ly in enumerate(mom["layers"]):
        CR.rt_kernel_(sc.pol, sc.added, comp, ly["props"], ly["iface"], ly["tau_sum"], mom["m"], sc.dq, arch, iz + 1, sc.F0, sc.FT,
                      model.numerics, dtau=ly["dtau"], ndoubl=ly["nd"])
    torch.cuda.synchronize()
    assert seen and all(s == ("ex", 0) for s in seen), seen
    assert torch.isfinite(comp.R_mp).all() and torch.isfinite(comp.T_pp).all()
    monkeypatch.setattr(CR, "NATIVE_SOURCES_ONLY", False)
    st_off = CR.rt_run_streams(model)
    for a, b in zip(st_on.R_mp_per_m + st_on.T_pp_per_m, st_off.R_mp_per_m + st_off.T_pp_per_m):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
