"""SurfaceEmission on the device, forward: vsm_surface_emission_* through the C ABI, then rt_run,
rt_run_multisensor(thermal=True) and rt_run_fluxes(thermal=True) against tests/surface_emission_oracle.py added to the oracles of the
solar slot and of the Planck volume source; explicit emissivities, blocks, the cavity, idle models, refusals.

Bounds, relative to the maximum of the compared field: the kernel against its formula 1e-14 (FP64) / 1e-6 (FP32); the drivers
against the oracle 1e-12 (FP64) / 2e-5 (FP32), the FP32 runs against the exact reference of their own algorithm (O.exact_model).

Shapes: Nz = 3, levels [0, 1, 3, 1] (a duplicate, and level Nz, where the bottom is the emitting surface layer alone), Stokes_I and
Stokes_IQU on four streams (N = 4 and 12), S = 5 and 23 (N = 12, S = 23: 276 rows, two workgroups, the last one partial), one scene
per surface layout: LambertianSurfaceScalar (shared block), rpvSurfaceScalar (shared, rows that differ), LambertianSurfaceLegendre
(one block per point)."""
import ctypes as C
import dataclasses
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
import flux_oracle as FO  # noqa: E402
import ms_oracle as MS  # noqa: E402
import surface_emission_oracle as SE  # noqa: E402

pytestmark = pytest.mark.gpu

L = 3
LEVELS = [0, 1, 3, 1]
GEO = (40.0, [30.0, 30.0], [0.0, 90.0])       # l_trunc = 3: two Gauss nodes, the SZA node, one VZA node
LT = 3
RPV = (0.12, 0.08, 0.75, -0.25)
COEFF = [0.25, 0.08, -0.03]
CASES = [("lambertian", "I", 5), ("lambertian", "IQU", 23), ("rpv", "I", 23), ("rpv", "IQU", 5), ("legendre", "I", 5),
         ("legendre", "IQU", 23)]
FTS = [np.float64, np.float32]
FLUX_FIELDS = FO.FIELDS


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _tol(FT):
    return 1e-12 if FT == np.float64 else 2e-5


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _arrays(S, FT=np.float64, window=None):
    """The column.  window=False (the FP64 forward runs): layers of optical depth 0.04 .. 0.4, 8 or 9 doublings each.  window=True
    (every FP32 run and every linearized run): a window channel, a hundredth of those optical depths, 1 or 2 doublings.

    Why: every doubling step doubles the absolute rounding error that r and t carry beside the identity, so the field of a column
    holds about c eps 2^ndoubl of rounding, c about 1 for the forward fields and up to about 7 for the gas Jacobians, which
    differentiate the small part I - t.  The bounds of these tests are 4500 eps64 (forward FP64: 9 doublings fit), 330 eps32
    (forward FP32), 450 eps64 and 170 eps32 (rt_run_lin): the last three are bounds for columns of at most about 4 doublings.  The
    kernels under test do not know of ndoubl."""
    rng = np.random.default_rng(S)
    window = (FT != np.float64) if window is None else window
    k = 0.01 if window else 1.0
    tau_rayl = np.tile(k * np.array([0.03, 0.05, 0.08]), (S, 1))
    tau_abs = k * 10.0 ** rng.uniform(-2.0, -0.5, (S, L))
    return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, m_max=2)


def _B_layer(S):
    return 0.4 + 0.05 * np.arange(L)[:, None] + 0.01 * np.arange(S)[None, :]


def _B_surface(S):
    return 0.9 + 0.03 * np.arange(S)


def scene(vsm, arch, kind, pol, S, FT=np.float64, sources=None, albedo=0.3, window=None):
    """(host model, oracle model -- for FP32 the exact reference of the FP32 algorithm --, the oracle's forward surface function
    or None for the Lambertian layers it builds from model.albedo)."""
    H = vsm.host_model
    kw = _arrays(S, FT, window)
    hs = {"lambertian": None, "rpv": H.rpvSurfaceScalar(*RPV), "legendre": H.LambertianSurfaceLegendre(list(COEFF))}[kind]
    pm = H.model_from_arrays(arch, pol, LT, *GEO, float_type=FT, surface=hs, albedo=albedo, sources=sources, **kw)
    om = O.build_model(pol, LT, *GEO, FT=FT, albedo=albedo, **kw)
    if FT != np.float64:
        om = O.exact_model(om)
    fsurf = None
    if kind == "legendre":
        om.albedo = O.legendre_albedo(np.asarray(COEFF, dtype=np.float64), S, np.float64)
    elif kind == "rpv":
        osurf, mu = OB.RPVSurface(*RPV), om.quad_points.qp_mu.astype(np.float64)
        opol, qp = om.pol, om.quad_points
        fsurf = lambda m, a, ts: CM.create_surface_layer_brdf(OB.reflectance(osurf, opol.n, mu, m), a, m, opol, qp, ts, np.float64)
    return pm, om, fsurf


def _sources(H, which, S, **se_kw):
    se = H.SurfaceEmission(B_surface=_B_surface(S), **se_kw)
    return {"emission": (se,), "all": (H.SolarBeam(), H.ThermalEmission(B_layer=_B_layer(S)), se)}[which]


def oracle_levels(om, fsurf, which, S, levels, emissivity=None, full=None):
    """(uw, dw) per level of the oracle: the solar slot (F0 = 0 without a SolarBeam, Scene's rule) + the thermal slot with its
    Planck table over the emitting boundary.  full: {level: (uw, dw) [S, N]} of m = 0, summed."""
    solar = which == "all"
    ms = om if solar else dataclasses.replace(om, F0=np.zeros((om.pol.n, S), dtype=om.FT))
    fs, ft = {}, {}
    us, ds = MS.ms_reference(ms, levels, surface=fsurf, full=fs)
    ut, dt = SE.emission_response(om, _B_surface(S), levels, surface=fsurf, emissivity=emissivity, full=ft,
                                  B_layer=_B_layer(S) if solar else None)
    if full is not None:
        for l in set(levels):
            full[l] = tuple(np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64) for a, b in zip(fs[(l, 0)], ft[(l, 0)]))
    return [a + b for a, b in zip(us, ut)], [a + b for a, b in zip(ds, dt)]


# ---- the kernel through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n,S", [(1, 5), (1, 23), (3, 5), (3, 23)])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_point"])
def test_surface_emission_kernel(vsm, arch, FT, n, S, shared):
    """vsm_surface_emission_* on a random r-+ against the formula, Kirchhoff and explicit; j0- is accumulated into; r-+ and the
    other fields stay; m > 0 and S = 0 do nothing."""
    CR = vsm.CoreRT
    N = 4 * n
    rng = np.random.default_rng(100 * n + S)
    dt = torch.float64 if FT == np.float64 else torch.float32
    dev = torch.device("cuda", 0)
    r = rng.standard_normal((1 if shared else S, N, N)).astype(FT)
    j0 = rng.standard_normal((S, N)).astype(FT)
    B = (0.5 + rng.random(S)).astype(FT)
    em = rng.random(S).astype(FT)
    tol = 1e-14 if FT == np.float64 else 1e-6
    for emissivity in (None, em):
        added = CR.AddedLayer(FT, arch, N, S, shared, 0)
        added.r_mp.copy_(torch.tensor(np.ascontiguousarray(r.transpose(0, 2, 1)), dtype=dt, device=dev))     # (s, j, i)
        added.j0_m.copy_(torch.tensor(j0, dtype=dt, device=dev))
        added.j0_p.fill_(3.0)
        tB = torch.tensor(B, dtype=dt, device=dev)
        tE = None if emissivity is None else torch.tensor(em, dtype=dt, device=dev)
        a = added.cstruct()
        for m in (1, 0):
            vsm._lib.call("vsm_surface_emission", dt, N, n, S, m, CR._ptr(tB), CR._ptr(tE), C.byref(a), CR._stream_ptr())
            torch.cuda.synchronize()
            got = added.j0_m.cpu().numpy().astype(np.float64)
            if m == 1:
                assert np.array_equal(got, j0.astype(np.float64))
        want = j0.astype(np.float64) + SE.emission_vector(r.astype(np.float64), n, B.astype(np.float64),
                                                          None if emissivity is None else em.astype(np.float64))
        e = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print("kernel n %d S %d %s %s %s: %.2e" % (n, S, "shared" if shared else "per point", FT.__name__,
                                                  "kirchhoff" if emissivity is None else "explicit", e))
        assert e <= tol, e
        assert torch.all(added.j0_p == 3.0)
        assert np.array_equal(added.r_mp.cpu().numpy(), np.ascontiguousarray(r.transpose(0, 2, 1)))
    # S = 0 is a no-op (on the layer above: the ABI refuses null fields before it looks at S); n_stokes outside 1..4 is refused
    before = added.j0_m.clone()
    vsm._lib.call("vsm_surface_emission", dt, N, n, 0, 0, CR._ptr(tB), None, C.byref(a), CR._stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(before, added.j0_m)
    with pytest.raises(vsm._lib.VSMError):
        vsm._lib.call("vsm_surface_emission", dt, N, 5, S, 0, CR._ptr(tB), None, C.byref(a), CR._stream_ptr())


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=["fp64", "fp32"])
@pytest.mark.parametrize("which", ["emission", "all"])
@pytest.mark.parametrize("kind,pol,S", CASES, ids=["%s_%s_S%d" % c for c in CASES])
def test_forward_drivers_against_oracle(vsm, arch, kind, pol, S, which, FT):
    """rt_run, rt_run_multisensor(thermal=True) and rt_run_fluxes(thermal=True) with the source alone and beside SolarBeam and
    ThermalEmission; level 0 of the multi-sensor run is rt_run bit for bit; the duplicate level is the same array."""
    H = vsm.host_model
    pm, om, fsurf = scene(vsm, arch, kind, pol, S, FT, sources=None)
    pm.sources = _sources(H, which, S)
    tol = _tol(FT)
    full = {}
    ur, dr = oracle_levels(om, fsurf, which, S, LEVELS, full=full)
    R, T = vsm.CoreRT.rt_run(pm)
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, LEVELS, thermal=True)
    assert R.dtype == FT and np.array_equal(uw[0], R) and np.array_equal(dw[0], T)
    assert np.array_equal(uw[1], uw[3]) and np.array_equal(dw[1], dw[3])
    errs = {"R": _rel(R, ur[0]), "T": _rel(T, dr[0])}
    for i, l in enumerate(LEVELS):
        errs["uw%d" % l], errs["dw%d" % l] = _rel(uw[i], ur[i]), _rel(dw[i], dr[i])
    # the emission is in every level: the oracle without it is far away
    u0, _ = oracle_levels(om, fsurf, which, S, [3], emissivity=0.0)
    assert _rel(uw[2], u0[0]) > 0.1
    # fluxes: the m = 0 level vectors of the same oracles through flux_oracle's quadrature
    om0 = dataclasses.replace(om, m_max=0)
    f0 = {}
    oracle_levels(om0, fsurf, which, S, LEVELS, full=f0)
    ref = FO.fluxes_from_vectors(om0, LEVELS, f0, solar=which == "all")
    res = vsm.CoreRT.rt_run_fluxes(pm, LEVELS, thermal=True)
    for k in FLUX_FIELDS:
        errs[k] = _rel(getattr(res, k), getattr(ref, k))
    print("SE fwd %-10s %-3s S %2d %-8s %s: %s" % (kind, pol, S, which, FT.__name__, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= tol, errs


@pytest.mark.parametrize("FT", FTS, ids=["fp64", "fp32"])
def test_explicit_emissivity_scalar_and_spectral(vsm, arch, FT):
    H = vsm.host_model
    S = 5
    em = np.linspace(0.6, 1.0, S)
    for emissivity in (0.8, em):
        pm, om, fsurf = scene(vsm, arch, "lambertian", "IQU", S, FT)
        pm.sources = _sources(H, "all", S, emissivity=emissivity)
        ur, dr = oracle_levels(om, fsurf, "all", S, LEVELS, emissivity=emissivity)
        uw, dw = vsm.CoreRT.rt_run_multisensor(pm, LEVELS, thermal=True)
        e = max(max(_rel(a, b) for a, b in zip(uw, ur)), max(_rel(a, b) for a, b in zip(dw, dr)))
        print("SE explicit emissivity %s %s: %.2e" % ("scalar" if np.ndim(emissivity) == 0 else "spectral", FT.__name__, e))
        assert e <= _tol(FT), e
    # emissivity = 1 - albedo over the Lambertian surface IS the Kirchhoff emission (to rounding)
    pm, _, _ = scene(vsm, arch, "lambertian", "IQU", S, FT, sources=_sources(H, "emission", S, emissivity=0.7))
    pk, _, _ = scene(vsm, arch, "lambertian", "IQU", S, FT, sources=_sources(H, "emission", S))
    assert _rel(vsm.CoreRT.rt_run(pm)[0], vsm.CoreRT.rt_run(pk)[0]) <= (1e-14 if FT == np.float64 else 1e-6)


def test_empty_spectral_axis(vsm, arch):
    H = vsm.host_model
    kw = _arrays(5)
    kw["tau_rayl"], kw["tau_abs"] = kw["tau_rayl"][:0], kw["tau_abs"][:0]
    pm = H.model_from_arrays(arch, "IQU", LT, *GEO, albedo=0.3, sources=(H.SurfaceEmission(B_surface=np.zeros(0)),), **kw)
    R, T = vsm.CoreRT.rt_run(pm)
    assert R.shape == (2, 3, 0) and T.shape == (2, 3, 0)


def test_flux_blocks_are_bit_identical(vsm, arch):
    """max_points = 2 on 5 points (blocks of 2, 2, 1): every block slices B_surface and the emissivity with its points."""
    H = vsm.host_model
    for se_kw in (dict(), dict(emissivity=np.linspace(0.6, 1.0, 5))):
        pm, _, _ = scene(vsm, arch, "legendre", "IQU", 5, sources=_sources(H, "all", 5, **se_kw))
        one = vsm.CoreRT.rt_run_fluxes(pm, None, thermal=True)
        blk = vsm.CoreRT.rt_run_fluxes(pm, None, thermal=True, max_points=2)
        for k in FLUX_FIELDS + ("absorbed", "surface_absorbed"):
            assert np.array_equal(getattr(one, k), getattr(blk, k)), k
        # a scene over a slice of the axis (what a shard or a block prepares) is that slice of the whole run
        R, _ = vsm.CoreRT.rt_run(pm)
        part = vsm.CoreRT.prepare_scene(pm, slice(1, 4))
        assert tuple(part.surface_B.shape) == (3,) and (not se_kw or tuple(part.surface_emissivity.shape) == (3,))
        part.run()
        torch.cuda.synchronize()
        assert _rel(part.results_host()[0], R[:, :, 1:4]) <= 1e-13


@pytest.mark.parametrize("kind,pol", [("lambertian", "IQU"), ("rpv", "I")])
def test_cavity_on_the_device(vsm, arch, kind, pol):
    """B_layer = B_surface = B0 under an opaque lid, no SolarBeam, albedo 0.3: uw / B0 = 1 at levels 0..Nz, dw / B0 = 1 at 1..Nz,
    Q = U = 0, up = down_diffuse = pi B0 at 1..Nz and surface_absorbed = 0, all to 1e-3 (test_oracle_surface_emission.py)."""
    H = vsm.host_model
    S = 3
    B0 = np.array([0.7, 1.3, 2.1])
    tau_rayl = np.tile(np.array([0.05, 0.05, 0.05]), (S, 1))
    tau_abs = np.tile(np.array([40.0, 0.5, 0.8]), (S, 1)) * np.array([1.0, 1.2, 1.5])[:, None]
    hs = H.rpvSurfaceScalar(*RPV) if kind == "rpv" else None
    src = (H.ThermalEmission(B_layer=np.tile(B0, (L, 1))), H.SurfaceEmission(B_surface=B0))
    pm = H.model_from_arrays(arch, pol, 9, 40.0, [30.0, 5.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279,
                             albedo=0.3, m_max=0, surface=hs, sources=src)
    levels = [0, 1, 2, 3]
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=True)
    for l in levels:
        eu, ed = np.max(np.abs(uw[l][:, 0] / B0 - 1)), np.max(np.abs(dw[l][:, 0] / B0 - 1))
        print("device cavity %s level %d: %.2e %.2e" % (kind, l, eu, ed))
        assert eu <= 1e-3 and (l == 0 or ed <= 1e-3), (l, eu, ed)
        for c in range(1, uw[l].shape[1]):
            assert np.max(np.abs(uw[l][:, c] / B0)) <= 1e-3 and np.max(np.abs(dw[l][:, c] / B0)) <= 1e-3
    res = vsm.CoreRT.rt_run_fluxes(pm, None, thermal=True)
    for l in (1, 2, 3):
        assert np.max(np.abs(res.up[l] / (math.pi * B0) - 1)) <= 1e-3 and np.max(np.abs(res.down_diffuse[l] / (math.pi * B0) - 1)) <= 1e-3
    assert np.max(np.abs(res.surface_absorbed / (math.pi * B0))) <= 1e-3
    # without the source the boundary only reflects
    pm.sources = src[:1]
    u0, _ = vsm.CoreRT.rt_run_multisensor(pm, [3], thermal=True)
    assert np.max(np.abs(u0[0][:, 0] / B0 - 1)) > 0.5


def test_idle_model_is_untouched(vsm, arch):
    """Without a SurfaceEmission, and with an all-zero one, nothing is allocated or launched: the outputs of a second scene object
    are the bits of the first, the scene holds no skin table, and a thermal-free model still has no thermal slot."""
    H = vsm.host_model
    S = 5
    base = (H.SolarBeam(), H.ThermalEmission(B_layer=_B_layer(S)))
    pa, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=base)
    pb, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=base + (H.SurfaceEmission(B_surface=np.zeros(S)),))
    Ra, Ta = vsm.CoreRT.rt_run(pa)
    Rb, Tb = vsm.CoreRT.rt_run(pb)
    assert np.array_equal(Ra, Rb) and np.array_equal(Ta, Tb)
    ua, da = vsm.CoreRT.rt_run_multisensor(pa, LEVELS, thermal=True)
    ub, db = vsm.CoreRT.rt_run_multisensor(pb, LEVELS, thermal=True)
    assert all(np.array_equal(x, y) for x, y in zip(ua + da, ub + db))
    fa, fb = vsm.CoreRT.rt_run_fluxes(pa, None, thermal=True), vsm.CoreRT.rt_run_fluxes(pb, None, thermal=True)
    for k in FLUX_FIELDS + ("absorbed", "surface_absorbed"):
        assert np.array_equal(getattr(fa, k), getattr(fb, k)), k
    sb = vsm.CoreRT.prepare_scene(pb)
    assert sb.surface_B is None and sb.surface_emissivity is None and sb.thermal_B is not None
    pz, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=(H.SolarBeam(), H.SurfaceEmission(B_surface=np.zeros(S))))
    sz = vsm.CoreRT.prepare_scene(pz)
    assert sz.thermal_B is None and sz._thermal is None
    ps, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=(H.SolarBeam(),))       # (the solar run, no thermal slot at all)
    fs, fz = vsm.CoreRT.rt_run_fluxes(ps, None), vsm.CoreRT.rt_run_fluxes(pz, None, thermal=True)
    for k in FLUX_FIELDS + ("absorbed", "surface_absorbed"):
        assert np.array_equal(getattr(fs, k), getattr(fz, k)), k
    us, ds = vsm.CoreRT.rt_run_multisensor(ps, LEVELS)
    uz, dz = vsm.CoreRT.rt_run_multisensor(pz, LEVELS, thermal=True)
    assert all(np.array_equal(x, y) for x, y in zip(us + ds, uz + dz))
    pe, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=_sources(H, "emission", S))
    se = vsm.CoreRT.prepare_scene(pe)
    assert se.thermal_B is not None and tuple(se.thermal_B.shape) == (0, S) and tuple(se.surface_B.shape) == (S,)


def test_refusals(vsm, arch):
    H, CL, RR = vsm.host_model, vsm.CoreRTLin, vsm.CoreRTRaman
    VSMError = vsm._lib.VSMError
    S = 5
    pm, _, _ = scene(vsm, arch, "lambertian", "I", S, sources=_sources(H, "all", S))
    with pytest.raises(VSMError, match="SurfaceEmission"):
        vsm.CoreRT.rt_run_multisensor(pm, [1])
    with pytest.raises(VSMError, match="SurfaceEmission"):
        vsm.CoreRT.rt_run_fluxes(pm, [1])
    bad, _, _ = scene(vsm, arch, "lambertian", "I", S, sources=(H.SurfaceEmission(B_surface=np.ones(S + 1)),))
    for run in (lambda: vsm.CoreRT.rt_run(bad), lambda: vsm.CoreRT.rt_run_multisensor(bad, [1], thermal=True),
                lambda: vsm.CoreRT.rt_run_fluxes(bad, [1], thermal=True)):
        with pytest.raises(VSMError, match="spectral points"):
            run()
    ga = _arrays(S)["tau_abs"]
    hl = H.LinModel([0.5 * ga, 0.5 * ga])
    pm.sources = (H.SolarBeam(), H.SurfaceEmission(B_surface=_B_surface(S)))
    with pytest.raises(NotImplementedError, match="SurfaceEmission"):
        vsm.CoreRT.rt_run_ss(pm)
    with pytest.raises(NotImplementedError, match="SurfaceEmission"):
        CL.rt_run_ss(pm, hl, 0, 2, 1)
    from test_oracle_sif import RAMAN_GEO, RAMAN_SHIFTS, RAMAN_W_IE, raman_arrays
    kw, F0 = raman_arrays(12)
    rpm = H.model_from_arrays(arch, "IQU", 7, *RAMAN_GEO, sources=(H.SolarBeam(), H.SurfaceEmission(B_surface=np.ones(12))), **kw)
    rpm.varpi_Cabannes, rpm.F0 = 0.96, F0
    prs = RR.RRS(RAMAN_SHIFTS, RAMAN_W_IE, H.GreekCoefs(**vars(O.get_greek_rayleigh(6.0 / 7.0 * 0.5))))
    for run in (lambda: RR.rt_run(prs, rpm, 1), lambda: RR.rt_run_multisensor(prs, rpm, [1]), lambda: RR.rt_run_ss(prs, rpm, 1)):
        with pytest.raises(NotImplementedError, match="SurfaceEmission"):
            run()
