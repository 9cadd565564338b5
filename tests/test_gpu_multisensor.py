"""GPU tests of the multi-sensor run (vsm.CoreRT.rt_run_multisensor, core_rt_ms.py) and its level kernel (vsm_level_radiance_*,
csrc/vsm_level.hip): against the statement-order transcription of the reference's prototype (tests/ms_oracle.py ms_reference),
level 0 against rt_run bit for bit, the fused level kernel against its operator-level twin, flux conservation on the device's
full level vectors, poisoned work buffers and the number of layer steps and interactions the host issues."""
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ms_oracle as MS  # noqa: E402
from level_cases import contractive  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _err_per_level(got, ref):
    """max over levels, VZA, points of |got - ref| per Stokes component relative to that component's max |ref| (in the level)."""
    worst = 0.0
    for g, r in zip(got, ref):
        for k in range(r.shape[1]):
            sc = float(np.max(np.abs(r[:, k])))
            e = float(np.max(np.abs(g[:, k] - r[:, k])))
            worst = max(worst, e / sc if sc > 0 else e)
    return worst


def _aer(M):
    gk = (lambda g: M.GreekCoefs(**vars(g))) if M is not O else (lambda g: g)
    return [M.AerosolOptics(gk(O.hg_greek(0.7, 10)), 0.95, 0.1), M.AerosolOptics(gk(O.hg_greek(0.5, 6)), 0.9, 0.0)]


def _pair(vsm, arch, pol, l_trunc, S, L, rng, sza=40.0, vza=(30.0, 0.0, 55.0), vaz=(0.0, 60.0, 120.0), aerosols=False, FT=np.float64,
          surface=None, m_max=2, albedo=0.15):
    """(host model, oracle model) of one column: Rayleigh in every layer (spectrally flat, so that every point sees the same
    doubling decisions as the whole batch), absorption varying over the points."""
    tau_rayl = np.tile(np.linspace(0.3, 0.6, L) / L, (S, 1))
    tau_abs = 10.0 ** rng.uniform(-4, 0, (S, 1)) * np.full((1, L), 1.0 / L)
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=albedo, m_max=m_max)
    if aerosols:
        tau_aer = np.zeros((2, L))
        tau_aer[0, L // 3:L // 2 + 1] = 0.1
        tau_aer[1, L // 2:] = 0.05
        kw["tau_aer"] = tau_aer
    H = vsm.host_model
    pm = H.model_from_arrays(arch, pol, l_trunc, sza, list(vza), list(vaz), float_type=FT, surface=surface,
                             aerosol_optics=_aer(H) if aerosols else (), **kw)
    om = O.build_model(pol, l_trunc, sza, list(vza), list(vaz), FT=FT, aerosols=_aer(O) if aerosols else (), **kw)
    return pm, om


def _sub(om, idx):
    """The oracle model restricted to the spectral points idx (points are independent; the decisions are the batch's)."""
    import dataclasses
    return dataclasses.replace(om, tau_rayl=om.tau_rayl[idx], tau_abs=om.tau_abs[idx])


CASES = [
    # (id, pol, l_trunc, S, Nz, levels, kwargs)
    ("c2_like_n60_iqu", "IQU", 35, 2000, 40, [0, 1, 20, 39, 40], dict()),
    ("scalar_n8", "I", 10, 5, 6, [3, 0, 6, 1], dict(m_max=3)),
    ("scalar_n33", "I", 60, 4, 5, [2, 4], dict()),
    ("iquv_n112_aerosols", "IQUV", 50, 3, 5, [1, 3, 5], dict(aerosols=True, m_max=4)),
    ("scalar_n135_oplevel", "I", 264, 2, 4, [1, 2, 0], dict()),
    ("s1", "IQU", 9, 1, 5, [2, 4], dict(m_max=3)),
    ("s3_unsorted_duplicates", "IQU", 9, 3, 6, [5, 2, 5, 0, 2, 6, 1], dict(m_max=3)),
    ("aerosols_many_moments", "IQU", 17, 6, 8, [7, 3, 1], dict(aerosols=True, m_max=8)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_multisensor_against_prototype_fp64(vsm, arch, case):
    name, pol, lt, S, L, levels, kw = case
    pm, om = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(len(name)), **kw)
    N = pm.quad_points.Nquad * pm.polarization_type.n
    if name.startswith("scalar_n135"):
        assert N > 128
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels)
    R, T = vsm.CoreRT.rt_run(pm)
    idx = np.unique(np.r_[0, 1, S // 4, S // 2, S - 2, S - 1].clip(0, S - 1)) if S > 8 else np.arange(S)
    ur, dr = MS.ms_reference(_sub(om, idx), levels)
    per = [max(_err_per_level([uw[i][..., idx]], [ur[i]]), _err_per_level([dw[i][..., idx]], [dr[i]])) for i in range(len(levels))]
    e = max(per)
    print("MS %-28s N %3d S %4d levels %s: rel err %s" % (name, N, S, levels, " ".join("%.2e" % x for x in per)))
    # 1e-10, or twice rt_run's own deviation from the oracle on the same scene where that is larger (N > 128: level 0 IS rt_run)
    Ro, To = O.rt_run(_sub(om, idx))
    e_rt = max(_err_per_level([R[..., idx]], [Ro]), _err_per_level([T[..., idx]], [To]))
    assert e <= max(1e-10, 2 * e_rt), (name, e, e_rt)
    for i, l in enumerate(levels):
        assert np.all(np.isfinite(uw[i])) and np.all(np.isfinite(dw[i]))
        if l == 0:
            assert np.array_equal(uw[i], R) and np.array_equal(dw[i], T)
    for i, l in enumerate(levels):           # duplicates: the same arrays
        j = levels.index(l)
        assert np.array_equal(uw[i], uw[j]) and np.array_equal(dw[i], dw[j])


def _surface_fn(refl, om):
    pol, qp, FT = om.pol, om.quad_points, om.FT
    return lambda m, a, ts: CM.create_surface_layer_brdf(refl(m), a, m, pol, qp, ts, FT)


@pytest.mark.parametrize("kind", ["coxmunk", "rpv"])
def test_multisensor_brdf_surfaces(vsm, arch, kind):
    H = vsm.host_model
    if kind == "coxmunk":
        hs, osurf, pol, lt, brdf = H.CoxMunkSurface(wind_speed=5.0), CM.CoxMunkSurface(5.0), "IQU", 11, False
    else:
        hs, osurf, pol, lt, brdf = H.rpvSurfaceScalar(0.12, 0.08, 0.75, -0.25), OB.RPVSurface(0.12, 0.08, 0.75, -0.25), "I", 13, True
    pm, om = _pair(vsm, arch, pol, lt, 4, 5, np.random.default_rng(2), surface=hs, m_max=4)
    levels = [0, 2, 4, 5]
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels)
    mu = om.quad_points.qp_mu.astype(np.float64)
    if brdf:
        refl = lambda m: OB.reflectance(osurf, om.pol.n, mu, m)
    else:
        # the device's Fourier reflectance blocks (vsm_coxmunk_reflectance; test_gpu_coxmunk.py checks them against the oracle's
        # to ~1e-9, which the levels just above the surface would show undamped): here the level algebra is under test
        dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, np.float64)
        refl = lambda m: vsm.Architectures.to_host(vsm.CoreRT.reflectance(hs, dq, m, arch, np.float64)[0]).T.copy()
    ur, dr = MS.ms_reference(om, levels, surface=_surface_fn(refl, om))
    e = max(_err_per_level(uw, ur), _err_per_level(dw, dr))
    scene = vsm.CoreRT.prepare_scene(pm)     # level 0 = rt_run without the Cox-Munk single-scattering correction
    scene.ss_correction = False
    scene.compute_hdrf = False
    scene.run()
    torch.cuda.synchronize()
    R, T = scene.results_host()
    assert np.array_equal(uw[0], R) and np.array_equal(dw[0], T)
    # (1e-10, or twice rt_run's own deviation from the oracle on the same scene where that is larger)
    e_rt = max(_err_per_level([R], [ur[0]]), _err_per_level([T], [dr[0]]))
    print("MS %s: rel err %.2e (rt_run vs oracle %.2e)" % (kind, e, e_rt))
    assert e <= max(1e-10, 2 * e_rt), (kind, e, e_rt)


@pytest.mark.parametrize("pol,lt", [("IQU", 58), ("IQU", 35)], ids=["n96_iqu_c4_like", "n60_iqu"])
def test_multisensor_float32(vsm, arch, pol, lt):
    pm, om32 = _pair(vsm, arch, pol, lt, 5, 8, np.random.default_rng(4), FT=np.float32, m_max=3)
    levels = [0, 2, 5, 8]
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels)
    R, T = vsm.CoreRT.rt_run(pm)
    assert uw[0].dtype == np.float32
    assert np.array_equal(uw[0], R) and np.array_equal(dw[0], T)
    ur, dr = MS.ms_reference(O.exact_model(om32), levels)
    for i in range(1, len(levels)):
        for got, ref in ((uw[i], ur[i]), (dw[i], dr[i])):
            scale = float(np.max(np.abs(ref[:, 0])))
            e = float(np.max(np.abs(got.astype(np.float64) - ref))) / scale
            assert e <= 2e-3, (levels[i], e)


@pytest.mark.parametrize("N", [8, 60, 64, 96, 112, 128])
@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_kernel_fused_vs_oplevel(vsm, N, FT):
    _fused_vs_oplevel(vsm, N, FT, [0.0, 30.0, 60.0], [0.0, 45.0, 120.0])


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_kernel_fused_vs_oplevel_many_angles(vsm, FT):
    """70 viewing angles: more than the 64 one launch of the fused kernel carries (full vectors, then vsm_postprocess_vza)."""
    _fused_vs_oplevel(vsm, 60, FT, list(np.linspace(0.0, 80.0, 70)), list(np.linspace(0.0, 345.0, 70)))


def _fused_and_oplevel_calls(vsm, N, FT, vza, vaz, inputs=contractive, S=7, ops=(False, True)):
    """vsm_level_radiance_* and its operator-level twin on the same inputs, per-point then shared bottom: per bottom
    (shared, (A, a, B, c), [fused, oplevel] each [uw, dw, uw_full, dw_full] in float64), and what the row checks need (ops: which of
    the two to call, oplevel = False / True).
    inputs(N, S, rng, shared_bot) -> (A, a, B, c) in math order (tests/level_cases.py)."""
    MSd = vsm.core_rt_ms
    H = vsm.host_model
    pol = H.polarization_type("IQU" if N % 3 == 0 else "I")
    rng = np.random.default_rng(N)
    qp = types.SimpleNamespace(qp_mu=np.linspace(1.0, 0.05, N // pol.n))     # (the rows of the viewing angles: all _vza_rows_weights reads)
    dev = torch.device("cuda", 0)
    runs = []
    for shared in (False, True):
        A, a, B, c = inputs(N, S, rng, shared)
        lay = lambda X: torch.tensor(np.ascontiguousarray(X.transpose(0, 2, 1)), dtype=torch.float64 if FT == np.float64 else torch.float32,
                                     device=dev)
        vec = lambda x: torch.tensor(x, dtype=lay(A).dtype, device=dev)
        tA, tB, ta, tc = lay(A), lay(B), vec(a), vec(c)
        outs = []
        for op in ops:
            uw = torch.full((S, pol.n, len(vza)), 0.25, dtype=tA.dtype, device=dev)     # accumulated into
            dw = torch.full_like(uw, -0.5)
            uwf, dwf = torch.empty((S, N), dtype=tA.dtype, device=dev), torch.empty((S, N), dtype=tA.dtype, device=dev)
            MSd.level_radiance_(pol, qp, vza, vaz, 1, 1.0 / math.pi, tA, ta, tB, tc, uw, dw, dwf, uwf, oplevel=op)
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy().astype(np.float64) for x in (uw, dw, uwf, dwf)])
        vsm._lib.check_device_status("level kernel")
        runs.append((shared, (A, a, B, c), outs))
    return pol, qp, runs


def _check_vza_rows(vsm, pol, qp, vza, vaz, out, tol):
    """the VZA rows are the full vectors' rows, weighted (out: [uw, dw, uw_full, dw_full] of one call)"""
    row0, w = vsm.CoreRT._vza_rows_weights(pol, vza, vaz, qp, 1, 1.0 / math.pi, torch.float64)
    for v in range(len(vza)):
        for k in range(pol.n):
            wk = w[v + len(vza) * k]
            np.testing.assert_allclose(out[0][:, k, v] - 0.25, wk * out[2][:, row0[v] + k], rtol=tol * 10, atol=tol)
            np.testing.assert_allclose(out[1][:, k, v] + 0.5, wk * out[3][:, row0[v] + k], rtol=tol * 10, atol=tol)
    return list(row0)


def _fused_vs_oplevel(vsm, N, FT, vza, vaz):
    pol, qp, runs = _fused_and_oplevel_calls(vsm, N, FT, vza, vaz)
    for shared, (A, a, B, c), outs in runs:
        tol = 1e-12 if FT == np.float64 else 2e-5
        for xf, xo in zip(outs[0], outs[1]):
            assert np.max(np.abs(xf - xo)) <= tol * np.max(np.abs(xo)), (N, shared)
        uwr, dwr = MS.level_push_through(np.float64, A, a, B.astype(np.float64), c)
        assert np.max(np.abs(outs[0][2] - uwr)) <= 10 * tol * np.max(np.abs(uwr))
        assert np.max(np.abs(outs[0][3] - dwr)) <= 10 * tol * np.max(np.abs(dwr))
        _check_vza_rows(vsm, pol, qp, vza, vaz, outs[0], tol)


def test_conservative_column_flux_on_device(vsm, arch):
    from test_oracle_multisensor import conservative_model, flux_spread
    om, levels = conservative_model()
    H = vsm.host_model
    pm = H.model_from_arrays(arch, "I", 15, 40.0, [30.0], [0.0], tau_rayl=om.tau_rayl, depol=0.0, albedo=0.3, m_max=0)
    res = vsm.CoreRT.rt_run_multisensor(pm, levels, streams=True)
    assert res.levels == levels and len(res.uw_streams) == len(levels) and res.weight == [0.5 / math.pi]
    full = {(l, 0): (res.uw_streams[i][0][:, 0, :].T, res.dw_streams[i][0][:, 0, :].T) for i, l in enumerate(levels)}
    fo = {}
    MS.ms_reference(om, levels, full=fo)
    dev_spread, or_spread = flux_spread(om, full, levels), flux_spread(om, fo, levels)
    print("net-flux spread / (mu0 F0): device %.3e oracle %.3e" % (dev_spread, or_spread))
    assert dev_spread <= 2 * or_spread


def test_outputs_finite_with_poisoned_work(vsm, arch, monkeypatch):
    """VSM_POISON_WORK fills every work buffer with NaN: a bottom built from a sources-only segment (R-+ / T++ exported as NaN)
    or a level call reading unwritten scratch would surface here."""
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    pm, _ = _pair(vsm, arch, "IQU", 35, 16, 10, np.random.default_rng(9), aerosols=True)
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, [0, 3, 7, 10])
    for x in uw + dw:
        assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0


def test_layer_steps_and_interactions(vsm, arch, monkeypatch):
    """Interior levels add at most Nz - l_1 layer steps per moment and one interaction per interior level -- none per layer."""
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
    for pol, lt in (("IQU", 35), ("IQUV", 50)):          # native runs / the reference-layout walk
        pm, _ = _pair(vsm, arch, pol, lt, 8, 12, np.random.default_rng(1), m_max=3)
        nm = pm.m_max + 1
        got = {}
        for levels in ([0], [0, 4, 9, 12]):
            counts.update(steps=0, inter=0)
            vsm.CoreRT.rt_run_multisensor(pm, levels)
            got[len(levels)] = dict(counts)
        assert got[1] == dict(steps=12 * nm, inter=nm), (pol, got)
        assert got[4]["steps"] - got[1]["steps"] <= (12 - 4) * nm, (pol, got)
        assert got[4]["inter"] - got[1]["inter"] == 2 * nm, (pol, got)


def test_non_scattering_layer_is_refused(vsm, arch):
    H = vsm.host_model
    tr = np.tile(np.full(4, 0.05), (2, 1))
    tr[:, 2] = 0.0
    pm = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=1)
    with pytest.raises(NotImplementedError, match="scatter = true"):
        vsm.CoreRT.rt_run_multisensor(pm, [1])
