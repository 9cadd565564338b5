"""The linearized run with thermal emission on the device: vsm_thermal_source_lin, the thermal slot of
CoreRTLin.rt_run_lin and its Planck slots against tests/thermal_lin_oracle.py (itself pinned by central differences of the forward
oracle, tests/test_oracle_thermal_lin.py) plus the solar oracles, and against finite differences of the device's forward run.

Bounds: those of tests/test_gpu_lin.py for the same scenes and kernels -- R, T 1e-9 and Jacobians 1e-8 of each array's maximum in
FP64 (test_rt_run_lin_vs_oracle_and_fd, test_rt_run_lin_aerosol_slots), the albedo / aerosol finite differences max 1e-3, mean
1e-4 (the reference's own gate), FP32 1e-2 against the FP64 oracle and 5e-4 / 2e-3 against the FP32 oracle
(test_rt_run_lin_fp32); over the BRDF surfaces 1e-8 for all four arrays, the bound of their own tests (test_gpu_coxmunk,
test_gpu_brdf_lin: the device's reflectance tables agree with the oracle's to 1e-9 only)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import brdf_lin_oracle as BL  # noqa: E402
import thermal_lin_oracle as TL  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S, L = 3, 3
GEO = (40.0, [30.0, 5.0], [0.0, 60.0])
# one shape per linearized kernel family: operator level, vsm_striplin, vsm_strip128lin, past every on-chip kernel (N = 7, 57, 64, 136)
SHAPES = [("I", 9), ("IQU", 33), ("IQUV", 25), ("IQUV", 61)]


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _B(rows=L, n=S):
    return 0.1 + 0.02 * np.arange(rows)[:, None] * (1.0 + np.arange(n))[None, :]


def _arrays():
    rng = np.random.default_rng(0)
    tau_rayl = np.tile(0.03 * np.ones(L), (S, 1))
    ga, gb = 10.0 ** rng.uniform(-2.5, -0.5, (S, L)), 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    return dict(tau_rayl=tau_rayl, tau_abs=ga + gb, depol=0.0279, m_max=2), ga, gb


def _sources(H, which, **kw):
    th = H.ThermalEmission(B_layer=_B(), **kw)
    return (H.SolarBeam(), th) if which == "solar+thermal" else (th,)


@functools.lru_cache(maxsize=None)
def _oracle(pol, l_trunc, which, FT=np.float64):
    """Solar + thermal oracle of the gas scene, computed once per case and only read."""
    kw, ga, gb = _arrays()
    om = O.build_model(pol, l_trunc, *GEO, albedo=0.2, FT=FT, **kw)
    lin = OL.LinModel([ga, gb])
    th = TL.rt_run_thermal_lin(om, lin, _B())
    if which == "thermal":     # without a SolarBeam the solar slot runs with F0 = 0
        om.F0 = np.zeros((om.pol.n, S), dtype=FT)
    so = OL.rt_run_lin(om, lin)
    return tuple(a + b for a, b in zip(so, th))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_layer", [1, 3])
@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol_name,l_trunc", [("I", 9), ("IQU", 9)])
def test_thermal_source_lin_kernel(vsm, arch, pol_name, l_trunc, FT, p_layer):
    """vsm_thermal_source_lin_*: j0+- the bits of vsm_thermal_source_*, ap_J0+- the oracle's formula, exact zeros on the Q / U rows
    and in the slot behind the layer slots (written, not left: the stacks are filled with 7 first)."""
    CR, CL, H = vsm.CoreRT, vsm.CoreRTLin, vsm.host_model
    rng = np.random.default_rng(4)
    pol, opol = H.polarization_type(pol_name), O.polarization(pol_name)
    qp = H.rt_set_streams(l_trunc, 40.0, [30.0, 5.0], pol, FT)
    oqp = O.rt_set_streams_gausslegquad(l_trunc, 40.0, [30.0, 5.0], opol, FT)
    dq = CR.device_quad(qp, pol, arch, FT)
    N, P = qp.Nquad * pol.n, p_layer + 1
    dtau = np.array([1e-4, 0.05, 0.7]).astype(FT)
    varpi = np.array([0.0, 0.4, 0.95]).astype(FT)
    B = np.array([10.0, 0.3, 2.0]).astype(FT)
    td = (rng.standard_normal((S, p_layer)) * dtau[:, None]).astype(FT)
    wd = (0.1 * rng.standard_normal((S, p_layer))).astype(FT)
    conv = vsm.Architectures.array_type(arch)
    to_host = vsm.Architectures.to_host
    added, ref_added = CR.AddedLayer(FT, arch, N, S), CR.AddedLayer(FT, arch, N, S)
    al = CL.AddedLayerLin(FT, arch, P, N, S)
    for t in (added.j0_p, added.j0_m, al.ap_J0_p, al.ap_J0_m):
        t.fill_(7.0)
    q, a, a0, al_ = dq.cstruct(), added.cstruct(), ref_added.cstruct(), al.cstruct()
    dev = [conv(x) for x in (dtau, varpi, B)]
    dtd, dvd = CL.to_device_sp(td, arch, FT), CL.to_device_sp(wd, arch, FT)
    vsm._lib.call("vsm_thermal_source_lin", added.dtype, C.byref(q), S, CR._ptr(dev[0]), CR._ptr(dev[1]), CR._ptr(dev[2]), p_layer,
                  CR._ptr(dtd), CR._ptr(dvd), C.byref(a), C.byref(al_), CR._stream_ptr())
    vsm._lib.call("vsm_thermal_source", added.dtype, C.byref(q), S, CR._ptr(dev[0]), CR._ptr(dev[1]), CR._ptr(dev[2]), C.byref(a0),
                  CR._stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(added.j0_p, ref_added.j0_p) and torch.equal(added.j0_m, ref_added.j0_m)
    assert float(added.j0_p.abs().max()) > 0
    # the oracle in double precision on the inputs as the kernel saw them (rounded to FT)
    _, jd = TL.thermal_source_lin(opol, oqp, dtau.astype(np.float64), varpi.astype(np.float64), B.astype(np.float64),
                                  td.astype(np.float64), wd.astype(np.float64), np.float64, DT=FT)
    gp, gm = to_host(al.ap_J0_p), to_host(al.ap_J0_m)
    tol = 1e-13 if FT == np.float64 else 1e-5
    assert np.max(np.abs(jd)) > 0
    assert _rel(gp[:p_layer], jd) < tol and _rel(gm[:p_layer], jd) < tol, (_rel(gp[:p_layer], jd), _rel(gm[:p_layer], jd))
    assert np.all(gp[p_layer:] == 0) and np.all(gm[p_layer:] == 0)                     # the surface slot
    for k in range(1, pol.n):
        assert np.all(gp[:, :, k::pol.n] == 0) and np.all(gm[:, :, k::pol.n] == 0)     # the Q / U rows
        assert np.all(to_host(added.j0_p)[:, k::pol.n] == 0)


# ---- rt_run_lin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["solar+thermal", "thermal"])
@pytest.mark.parametrize("pol,l_trunc", SHAPES)
def test_rt_run_lin_thermal_vs_oracle_and_fd(vsm, arch, pol, l_trunc, which):
    """rt_run_lin over (SolarBeam(), ThermalEmission(B)) and over the thermal source alone: R, T = the oracle's solar + thermal
    slot, the Jacobians = OL.rt_run_lin + the thermal-lin oracle, the albedo Jacobian also a finite difference of the device's
    forward run.  (Before the slot existed R lacked the thermal radiance: this test failed in its first comparison.)

    The finite difference of the thermal-only model: CoreRT.rt_run's Lambertian layer carries its beam term with pol.I0 even at
    F0 = 0 (tests/test_gpu_thermal.py::test_rt_run_thermal_slot_vs_oracle), the linearized builder uses F0
    (lambertian_surface_lin.jl); so that term's own difference quotient -- CoreRT.rt_run of the same model with F0 = 0 and no
    thermal source -- is taken off the forward run's."""
    H = vsm.host_model
    kw, ga, gb = _arrays()
    mk = lambda alb, src: H.model_from_arrays(arch, pol, l_trunc, *GEO, albedo=alb, sources=src, **kw)
    pm = mk(0.2, _sources(H, which))
    Ro, To, Rdo, Tdo = _oracle(pol, l_trunc, which)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(pm, H.LinModel([ga, gb]), 0, 2, 1)
    print("thermal lin %s %s %d: R %.2e T %.2e Rd %.2e Td %.2e" % (which, pol, l_trunc, _rel(R, Ro), _rel(T, To), _rel(Rd, Rdo),
                                                                  _rel(Td, Tdo)))
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9, (_rel(R, Ro), _rel(T, To))
    for p in range(3):
        assert _rel(Rd[..., p], Rdo[..., p]) < 1e-8, p
        assert _rel(Td[..., p], Tdo[..., p]) < 1e-8, p
    h = 1e-4
    fd = (vsm.CoreRT.rt_run(mk(0.2 + h, _sources(H, which)))[0] - vsm.CoreRT.rt_run(pm)[0]) / h
    if which == "thermal":
        def beam_term(alb):
            m0 = mk(alb, None)
            m0.F0 = np.zeros((m0.polarization_type.n, S))
            return vsm.CoreRT.rt_run(m0)[0]
        fd = fd - (beam_term(0.2 + h) - beam_term(0.2)) / h
    err = np.abs(fd - Rd[..., 2]) / np.abs(fd).max()
    print("  albedo finite difference: max %.2e mean %.2e" % (err.max(), err.mean()))
    assert err.max() < 1e-3 and err.mean() < 1e-4


@pytest.mark.parametrize("kind", ["coxmunk", "rpv"])
def test_rt_run_lin_thermal_over_brdf_surfaces(vsm, arch, kind):
    """The slot's surface step with the Cox-Munk and the rpvSurfaceScalar builders (beam terms zeroed), Stokes_IQU, N = 21."""
    H = vsm.host_model
    pol, l_trunc = "IQU", 9
    kw, ga, gb = _arrays()
    om = O.build_model(pol, l_trunc, *GEO, albedo=0.0, **kw)
    lin = OL.LinModel([ga, gb])
    mu = om.quad_points.qp_mu.astype(np.float64)
    if kind == "coxmunk":
        hs, osurf, K = H.CoxMunkSurface(wind_speed=5.0), CM.CoxMunkSurface(5.0), 1
        so = CM.rt_run_lin(om, lin, osurf)

        def tables(m):
            rho, drho = CM.reflectance_and_deriv(osurf, 3, mu, m)
            return rho, drho[None]
    else:
        osurf = BL.SURFACES["rpv"]
        hs, K = H.rpvSurfaceScalar(*[getattr(osurf, n) for n in BL.param_names(osurf)]), 4
        so = BL.rt_run_lin(om, lin, osurf)
        tables = lambda m: BL.reflectance_and_deriv(osurf, 3, mu, m)
    th = TL.rt_run_thermal_lin(om, lin, _B(), surface=TL.brdf_surface(K, tables))
    pm = H.model_from_arrays(arch, pol, l_trunc, *GEO, surface=hs, sources=_sources(H, "solar+thermal"), **kw)
    got = vsm.CoreRTLin.rt_run_lin(pm, H.LinModel([ga, gb]), 0, 2, K)
    assert got[2].shape[-1] == 2 + K
    for name, g, s_, t_ in zip(("R", "T", "Rd", "Td"), got, so, th):
        assert np.max(np.abs(t_)) > 1e-3 * np.max(np.abs(s_ + t_)), name          # the slot contributes
        assert _rel(g, s_ + t_) < 1e-8, (kind, name, _rel(g, s_ + t_))
    for p in range(2 + K):
        assert _rel(got[2][..., p], so[2][..., p] + th[2][..., p]) < 1e-8, (kind, p)
        assert _rel(got[3][..., p], so[3][..., p] + th[3][..., p]) < 1e-8, (kind, p)


def test_rt_run_lin_thermal_aerosol_slots(vsm, arch):
    """NAer = 1, NGas = 1, NSurf = 1 with a thermal source (the component-mixed elemental, vsm_elemental_lin_mix, in the slot):
    9 slots against the oracles, tau_ref / n_r / p0 against central differences of the device's forward run."""
    from tests.test_gpu_lin import _host_aerosol_scene
    H = vsm.host_model
    pol, l_trunc = "IQU", 9
    om, ol, pm, pl = _host_aerosol_scene(vsm, arch, pol, l_trunc)
    S_, L_ = om.tau_rayl.shape
    B = _B(L_, S_)
    src = lambda: (H.SolarBeam(), H.ThermalEmission(B_layer=B))
    pm.sources = src()
    ref = tuple(a + b for a, b in zip(OL.rt_run_lin(om, ol), TL.rt_run_thermal_lin(om, ol, B)))
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(pm, pl, 1, 1, 1)
    assert Rd.shape == ref[2].shape and Rd.shape[-1] == 9
    assert _rel(R, ref[0]) < 1e-9 and _rel(T, ref[1]) < 1e-9
    for p in range(9):
        assert _rel(Rd[..., p], ref[2][..., p]) < 1e-8 and _rel(Td[..., p], ref[3][..., p]) < 1e-8, p
    h = 1e-5
    for k in (0, 1, 5):
        e = np.zeros(7)
        e[k] = h
        runs = []
        for sgn in (1.0, -1.0):
            m_ = _host_aerosol_scene(vsm, arch, pol, l_trunc, sgn * e)[2]
            m_.sources = src()
            runs.append(vsm.CoreRT.rt_run(m_))
        for an, fd in ((Rd[..., k], (runs[0][0] - runs[1][0]) / (2 * h)), (Td[..., k], (runs[0][1] - runs[1][1]) / (2 * h))):
            err = np.abs(fd - an) / np.abs(fd).max()
            assert err.max() < 1e-3 and err.mean() < 1e-4, (k, err.max())


def test_rt_run_lin_thermal_fp32(vsm, arch):
    """Float32 (Stokes_IQU, N = 57): against the FP64 oracle at the reference's FP32 gate and against the FP32 oracle."""
    H = vsm.host_model
    pol, l_trunc = "IQU", 33
    kw, ga, gb = _arrays()
    pm = H.model_from_arrays(arch, pol, l_trunc, *GEO, albedo=0.2, float_type=np.float32, sources=_sources(H, "solar+thermal"), **kw)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(pm, H.LinModel([ga, gb]), 0, 2, 1)
    Ro, To, Rdo, Tdo = _oracle(pol, l_trunc, "solar+thermal")
    assert R.dtype == np.float32 and Rd.dtype == np.float32 and Rd.shape == Rdo.shape
    assert _rel(R, Ro) < 1e-2 and _rel(T, To) < 1e-2
    for p in range(3):
        assert _rel(Rd[..., p], Rdo[..., p]) < 1e-2 and _rel(Td[..., p], Tdo[..., p]) < 1e-2, p
    R32, T32, Rd32, Td32 = _oracle(pol, l_trunc, "solar+thermal", np.float32)
    print("thermal lin fp32: R %.2e T %.2e Rd %.2e Td %.2e" % (_rel(R, R32), _rel(T, T32), _rel(Rd, Rd32), _rel(Td, Td32)))
    assert _rel(R, R32) < 5e-4 and _rel(T, T32) < 5e-4
    for p in range(3):
        assert _rel(Rd[..., p], Rd32[..., p]) < 2e-3 and _rel(Td[..., p], Td32[..., p]) < 2e-3, p
    # ... and the thermal part alone is there: the run without the source differs by the oracle's slot
    pm0 = H.model_from_arrays(arch, pol, l_trunc, *GEO, albedo=0.2, float_type=np.float32, **kw)
    R0 = vsm.CoreRTLin.rt_run_lin(pm0, H.LinModel([ga, gb]), 0, 2, 1)[0]
    om = O.build_model(pol, l_trunc, *GEO, albedo=0.2, **kw)
    assert _rel(R - R0, O.rt_run_thermal(om, _B())[0]) < 1e-2


# ---- Planck slots ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol,l_trunc", [("IQU", 9), ("IQUV", 19)])     # N = 21: operator-level slot; N = 52: the fused thermal layer kernel
def test_planck_block(vsm, arch, pol, l_trunc):
    """ThermalEmission(B_layer_dot = [uniform table, unit table of layer 2]): slots P, P + 1 of Rdot / Tdot are the forward slot of
    each table; every earlier slot, R and T do not change by a bit."""
    H = vsm.host_model
    kw, ga, gb = _arrays()
    Bd = np.stack([np.ones((L, S)), np.zeros((L, S))])
    Bd[1, 1] = 1.0
    mk = lambda **th: H.model_from_arrays(arch, pol, l_trunc, *GEO, albedo=0.2, sources=_sources(H, "solar+thermal", **th), **kw)
    hl = H.LinModel([ga, gb])
    base = vsm.CoreRTLin.rt_run_lin(mk(), hl, 0, 2, 1)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(mk(B_layer_dot=Bd), hl, 0, 2, 1)
    assert Rd.shape[-1] == 5 and Td.shape[-1] == 5 and base[2].shape[-1] == 3
    assert np.array_equal(R, base[0]) and np.array_equal(T, base[1])
    assert np.array_equal(Rd[..., :3], base[2]) and np.array_equal(Td[..., :3], base[3])
    om = O.build_model(pol, l_trunc, *GEO, albedo=0.2, **kw)
    for k in range(2):
        Rk, Tk = O.rt_run_thermal(om, Bd[k])
        assert _rel(Rd[..., 3 + k], Rk) < 1e-9 and _rel(Td[..., 3 + k], Tk) < 1e-9, (k, _rel(Rd[..., 3 + k], Rk))
    # Planck tables alone (B_layer = 0: no thermal radiance, the block is still there)
    only = H.model_from_arrays(arch, pol, l_trunc, *GEO, albedo=0.2,
                               sources=(H.SolarBeam(), H.ThermalEmission(B_layer=np.zeros((L, S)), B_layer_dot=Bd)), **kw)
    R1, T1, Rd1, Td1 = vsm.CoreRTLin.rt_run_lin(only, hl, 0, 2, 1)
    assert np.array_equal(Rd1[..., 3:], Rd[..., 3:]) and np.array_equal(Td1[..., 3:], Td[..., 3:])


def test_thermal_slot_beside_the_m0_stokes_iq_subscene(vsm, arch):
    """A batch large enough for the m = 0 reduction (SceneLin.sub0): the sub-scene carries no thermal slot and no Planck slot,
    the parent runs both on its own Stokes dimension."""
    H = vsm.host_model
    rng = np.random.default_rng(14)
    S_ = 70
    tau_rayl = np.tile(0.03 * np.ones(L), (S_, 1))
    ga = 10.0 ** rng.uniform(-2.5, -0.5, (S_, L))
    kw = dict(tau_rayl=tau_rayl, tau_abs=ga, depol=0.0279, m_max=2)
    B, Bd = _B(L, S_), np.ones((1, L, S_))
    pm = H.model_from_arrays(arch, "IQU", 11, *GEO, albedo=0.2, sources=(H.SolarBeam(), H.ThermalEmission(B_layer=B, B_layer_dot=Bd)),
                             **kw)
    scene = vsm.CoreRTLin.SceneLin(pm, H.LinModel([ga]), 0, 1, 1)
    assert scene.sub0 is not None and scene.sub0.nPlanck == 0 and scene.sub0.fwd.thermal_B is None
    scene.run()
    torch.cuda.synchronize()
    R, T, Rd, Td = scene.results_host()
    om = O.build_model("IQU", 11, *GEO, albedo=0.2, **kw)
    ref = tuple(a + b for a, b in zip(OL.rt_run_lin(om, OL.LinModel([ga])), TL.rt_run_thermal_lin(om, OL.LinModel([ga]), B)))
    assert _rel(R, ref[0]) < 1e-9 and _rel(T, ref[1]) < 1e-9
    assert _rel(Rd[..., :2], ref[2]) < 1e-8 and _rel(Td[..., :2], ref[3]) < 1e-8
    assert _rel(Rd[..., 2], O.rt_run_thermal(om, Bd[0])[0]) < 1e-9


# ---- scope limits and the untouched solar path -----------------------------------------------------------------------------------
def test_refusals(vsm, arch):
    H, CL = vsm.host_model, vsm.CoreRTLin
    kw, ga, gb = _arrays()
    hl = H.LinModel([ga, gb])
    mk = lambda src, **over: H.model_from_arrays(arch, "I", 9, *GEO, albedo=0.2, sources=src, **dict(kw, **over))
    # a non-scattering layer under a thermal source
    tr = kw["tau_rayl"].copy()
    tr[:, 1] = 0.0
    with pytest.raises(NotImplementedError, match="does not scatter"):
        CL.rt_run_lin(mk(_sources(H, "solar+thermal"), tau_rayl=tr), hl, 0, 2, 1)
    CL.rt_run_lin(mk(None, tau_rayl=tr), hl, 0, 2, 1)            # (without the source the column runs as before)
    # graph replay
    scene = CL.SceneLin(mk(_sources(H, "solar+thermal")), hl, 0, 2, 1)
    with pytest.raises(NotImplementedError, match="graph"):
        scene.run(graph=True)
    eager = [t.clone() for t in scene.run(graph=False)]
    scene.graph_replay = True
    dflt = scene.run()                                          # graph=None: such a scene takes the eager path
    torch.cuda.synchronize()
    assert getattr(scene, "_graph", None) is None and all(torch.equal(a, b) for a, b in zip(eager, dflt))
    # the multi-sensor and the single-scattering linearized drivers keep refusing the source
    with pytest.raises(vsm.VSMError, match="SolarBeam"):
        CL.rt_run_multisensor(mk(_sources(H, "solar+thermal")), hl, 0, 2, 1, [1])
    with pytest.raises(NotImplementedError):
        CL.rt_run_ss(mk(_sources(H, "solar+thermal")), hl, 0, 2, 1)
    # 3 slots + 62 Planck slots
    with pytest.raises(vsm.VSMError, match="limit 64"):
        CL.rt_run_lin(mk(_sources(H, "solar+thermal", B_layer_dot=np.ones((62, L, S)))), hl, 0, 2, 1)
    CL.SceneLin(mk(_sources(H, "solar+thermal", B_layer_dot=np.ones((61, L, S)))), hl, 0, 2, 1)
    # shape errors, as for B_layer
    with pytest.raises(vsm.VSMError, match="spectral points"):
        CL.rt_run_lin(mk(_sources(H, "solar+thermal", B_layer_dot=np.ones((1, L, S + 1)))), hl, 0, 2, 1)
    with pytest.raises(ValueError):
        H.ThermalEmission(B_layer=_B(), B_layer_dot=np.ones(S))


def test_model_without_thermal_source_allocates_and_launches_nothing_new(vsm, arch):
    """No thermal source: the slot's objects never come to exist, on the linearized scene or on its forward scene, and the run
    (lanes = 1, fold = False) repeats bit for bit what it gave before the question could arise."""
    H = vsm.host_model
    kw, ga, gb = _arrays()
    pm = H.model_from_arrays(arch, "IQU", 9, *GEO, albedo=0.2, **kw)
    scene = vsm.CoreRTLin.SceneLin(pm, H.LinModel([ga, gb]), 0, 2, 1)
    calls = []
    orig = vsm._lib.call
    try:
        vsm._lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
        first = [t.clone() for t in scene.run(lanes=1, fold=False)]
    finally:
        vsm._lib.call = orig
    torch.cuda.synchronize()
    assert "vsm_thermal_source_lin" not in calls and "vsm_thermal_source" not in calls and "vsm_layer_forward_thermal" not in calls
    assert scene._th is None and scene.nPlanck == 0 and scene.fwd._thermal is None
    assert first[2].shape[0] == 3
    again = scene.run(lanes=1, fold=False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    Ro, To, Rdo, Tdo = OL.rt_run_lin(O.build_model("IQU", 9, *GEO, albedo=0.2, **kw), OL.LinModel([ga, gb]))
    R, T, Rd, Td = scene.results_host()
    assert _rel(R, Ro) < 1e-9 and _rel(Rd, Rdo) < 1e-8
