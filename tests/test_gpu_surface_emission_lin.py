"""SurfaceEmission on the device, linearized: vsm_surface_emission_lin_* through the C ABI, then rt_run_lin,
CoreRTLin.rt_run_multisensor and CoreRTLin.rt_run_fluxes against tests/surface_emission_oracle.py added to the oracles of the solar
slot and of the Planck volume source: the gas slots (the propagation of the emitted j0-), the surface slots (also the derivative of
the Kirchhoff emissivity), the skin slots behind the Planck slots.

Bounds, relative to the maximum of the compared field: the kernel 1e-14 (FP64) / 1e-6 (FP32); rt_run_lin 1e-13 (FP64) / 1e-5
(FP32); the level runs their forward bound, 1e-12 (FP64) / 2e-5 (FP32).  FP32 against the exact reference of the FP32 algorithm.

Shapes and scenes: those of test_gpu_surface_emission.py, the column its window channel in both precisions (its _arrays says why);
the FP64 level and flux runs also over its ordinary column, at their 1e-12 (test_level_runs_over_the_thick_column).  Over rpvSurfaceScalar (NSurf = 4) and LambertianSurfaceLegendre
(NSurf = 3) the runs have no SolarBeam: the linearized surface builders weigh the beam term by F0, so the solar slot is exactly
zero there and the thermal oracles, which take those surfaces, are the whole reference."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import brdf_lin_oracle as BL  # noqa: E402
import flux_lin_oracle as FL  # noqa: E402
import ms_thermal_lin_oracle as MTL  # noqa: E402
import spectral_albedo_lin_oracle as SA  # noqa: E402
import surface_emission_oracle as SE  # noqa: E402
import thermal_lin_oracle as TL  # noqa: E402
from test_gpu_surface_emission import (CASES, COEFF, FTS, L, LEVELS, RPV, _arrays, _B_layer, _B_surface, _rel, _tol, arch,  # noqa: E402,F401
                                       scene, vsm)

pytestmark = pytest.mark.gpu

NSURF = {"lambertian": 1, "rpv": 4, "legendre": 3}
DOT_FIELDS = FL.DOT_FIELDS


def _gases(S, window=True):
    ta = _arrays(S, window=window)["tau_abs"]
    return 0.6 * ta, 0.4 * ta


def _tables(S):
    """(B_layer_dot [1, L, S], B_surface_dot [2, S])."""
    return (np.ones((1, L, S)) * np.linspace(0.5, 1.0, S)[None, None, :],
            np.stack([np.ones(S), np.linspace(-0.3, 0.4, S)]))


def _sources(H, which, S, **se_kw):
    Bd, Bsd = _tables(S)
    se = H.SurfaceEmission(B_surface=_B_surface(S), B_surface_dot=Bsd, **se_kw)
    th = H.ThermalEmission(B_layer=_B_layer(S), B_layer_dot=Bd)
    return {"emission": (se,), "thermal": (th, se), "all": (H.SolarBeam(), th, se)}[which]


def _lin_surface(kind, om, S):
    """The `surface` argument of the linearized thermal oracles for the scene's surface (None: the model's Lambertian albedo)."""
    if kind == "rpv":
        osurf, mu, n = OB.RPVSurface(*RPV), om.quad_points.qp_mu.astype(np.float64), om.pol.n
        return TL.brdf_surface(4, lambda m: BL.reflectance_and_deriv(osurf, n, mu, m))
    if kind == "legendre":
        basis = SA.legendre_basis(len(COEFF), S, np.float64)
        return 3, (lambda a, al, isurf, m, pol, qp, ts, tsd, F0, FT:
                   SA.create_surface_layer_spectral_lin(om.albedo, basis, a, al, isurf, m, pol, qp, ts, tsd, F0, FT))
    return None


def _join(base, se, P, axis):
    """The slots of a run: `base` (P parameter slots + the Planck slots, or None) and the response `se` (P + the skin slots)."""
    if base is None:
        return se
    se_p, se_k = np.split(se, [P], axis=axis)
    out = np.concatenate([base, se_k], axis=axis)
    idx = [slice(None)] * out.ndim
    idx[axis] = slice(0, P)
    out[tuple(idx)] += se_p
    return out


def oracle_lin_levels(kind, om, S, which, levels, emissivity=None, full=None, window=True):
    """(uw, dw, uw_dot, dw_dot) per level: [solar slot +] the Planck volume source over the boundary that does not emit + the
    response to the surface emission; slots P | nPlanck | nSkin.  full: {level: (uw, dw, uw_dot, dw_dot)} at all streams, m = 0."""
    ga, gb = _gases(S, window)
    lin = OL.LinModel([ga, gb])
    Bd, Bsd = _tables(S)
    surface = _lin_surface(kind, om, S)
    P = 2 + NSURF[kind]
    fs, fb = {}, {}
    se = SE.emission_response_lin(om, lin, _B_surface(S), levels, surface=surface, emissivity=emissivity, B_surface_dot=Bsd, full=fs)
    base = None
    if which == "thermal":
        base = MTL.ms_thermal_lin_segmented(om, lin, _B_layer(S), Bd, levels, surface=surface, full=fb)
    elif which == "all":
        assert kind == "lambertian"
        base = MTL.ms_thermal_lin_total(om, lin, _B_layer(S), Bd, levels, solar=True, full=fb)
    if full is not None:
        for l in set(levels):
            s_ = tuple(np.asarray(x, dtype=np.float64) for x in fs[(l, 0)])
            if base is None:
                full[l] = s_
            else:
                b_ = tuple(np.asarray(x, dtype=np.float64) for x in fb[(l, 0)])
                full[l] = (b_[0] + s_[0], b_[1] + s_[1], _join(b_[2], s_[2], P, 0), _join(b_[3], s_[3], P, 0))
    if base is None:
        return se
    n = len(levels)
    return ([base[0][i] + se[0][i] for i in range(n)], [base[1][i] + se[1][i] for i in range(n)],
            [_join(base[2][i], se[2][i], P, 3) for i in range(n)], [_join(base[3][i], se[3][i], P, 3) for i in range(n)])


# ---- the kernel through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("FT", FTS, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n,S", [(1, 5), (3, 23)])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_point"])
def test_surface_emission_lin_kernel(vsm, arch, FT, n, S, shared):
    """vsm_surface_emission_lin_* on random stacks: the surface slots [isurf, isurf + K) of ap_J0- receive -2 pi B sum_j ap_r-+[.., j n],
    accumulated; the layer slots, a slot behind the range and every other stack keep their bits; m > 0 does nothing."""
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    N, P, isurf, K = 4 * n, 5, 2, 2
    rng = np.random.default_rng(7 * n + S)
    dt = torch.float64 if FT == np.float64 else torch.float32
    dev = torch.device("cuda", 0)
    r = rng.standard_normal((P, 1 if shared else S, N, N)).astype(FT)
    j0 = rng.standard_normal((P, S, N)).astype(FT)
    B = (0.5 + rng.random(S)).astype(FT)
    al = CL.AddedLayerLin(FT, arch, P, N, S, shared=shared)
    al.ap_r_mp.copy_(torch.tensor(np.ascontiguousarray(r.transpose(0, 1, 3, 2)), dtype=dt, device=dev))        # (p, s, j, i)
    al.ap_J0_m.copy_(torch.tensor(j0, dtype=dt, device=dev))
    al.ap_J0_p.fill_(3.0)
    tB = torch.tensor(B, dtype=dt, device=dev)
    a = al.cstruct()
    for m in (1, 0):
        vsm._lib.call("vsm_surface_emission_lin", dt, N, n, S, m, CR._ptr(tB), isurf, K, C.byref(a), CR._stream_ptr())
        torch.cuda.synchronize()
        got = al.ap_J0_m.cpu().numpy().astype(np.float64)
        if m == 1:
            assert np.array_equal(got, j0.astype(np.float64))
    want = j0.astype(np.float64).copy()
    r64 = r.astype(np.float64)
    for p in range(isurf, isurf + K):
        want[p] -= 2 * np.pi * B.astype(np.float64)[:, None] * np.broadcast_to(r64[p][:, :, ::n].sum(axis=2), (S, N))
    e = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("lin kernel n %d S %d %s %s: %.2e" % (n, S, "shared" if shared else "per point", FT.__name__, e))
    assert e <= (1e-14 if FT == np.float64 else 1e-6), e
    for p in (0, 1, 4):
        assert np.array_equal(got[p], j0[p].astype(np.float64))
    assert torch.all(al.ap_J0_p == 3.0)
    assert np.array_equal(al.ap_r_mp.cpu().numpy(), np.ascontiguousarray(r.transpose(0, 1, 3, 2)))
    with pytest.raises(vsm._lib.VSMError):     # the slots must lie within P
        vsm._lib.call("vsm_surface_emission_lin", dt, N, n, S, 0, CR._ptr(tB), 4, 2, C.byref(a), CR._stream_ptr())


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
def _whiches(kind):
    return ["emission", "thermal"] + (["all"] if kind == "lambertian" else [])


PARAMS = [(k, p, s, w) for k, p, s in CASES for w in _whiches(k)]


@pytest.mark.parametrize("FT", FTS, ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,pol,S,which", PARAMS, ids=["%s_%s_S%d_%s" % c for c in PARAMS])
def test_linearized_drivers_against_oracle(vsm, arch, kind, pol, S, which, FT):
    """rt_run_lin, CoreRTLin.rt_run_multisensor (level 0 = SceneLin.run(lanes=1, fold=False) bit for bit) and CoreRTLin.rt_run_fluxes:
    forward fields, gas and surface slots, one Planck slot, two skin slots."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    pm, om, _ = scene(vsm, arch, kind, pol, S, FT, window=True)
    pm.sources = _sources(H, which, S)
    hl = H.LinModel(list(_gases(S)))
    K = NSURF[kind]
    nPl = 0 if which == "emission" else 1
    Pa = 2 + K + nPl + 2
    full = {}
    ref = oracle_lin_levels(kind, om, S, which, LEVELS, full=full)
    # rt_run_lin
    got = CL.rt_run_lin(pm, hl, 0, 2, K)
    assert got[2].shape == (2, om.pol.n, S, Pa) and got[0].dtype == FT
    e_lin = {name: _rel(g, r[0]) for name, g, r in zip(("R", "T", "Rd", "Td"), got, ref)}
    per_slot = {}            # every slot on its own scale as well
    for p in range(Pa):
        assert np.max(np.abs(ref[2][0][..., p])) > 0, p
        per_slot["Rd%d" % p], per_slot["Td%d" % p] = _rel(got[2][..., p], ref[2][0][..., p]), _rel(got[3][..., p], ref[3][0][..., p])
    if FT == np.float64:
        # FP64 holds the bound slot by slot (a slot in the wrong place or a missing term shows here, however small the slot).
        # FP32 is compared field by field: the gas slots of T over an emitting boundary alone are the derivative of the
        # atmosphere's backscatter, and varpi dtau = tau_rayl does not depend on the absorption -- what is left is the difference
        # of two first-order terms, which single precision resolves to a few hundred eps32 of that slot's own maximum and no better
        e_lin.update(per_slot)
    print("SE lin %-10s %-3s S %2d %-8s %s rt_run_lin: %s" % (kind, pol, S, which, FT.__name__,
                                                             " ".join("%s %.1e" % kv for kv in {**e_lin, **per_slot}.items())))
    # the multi-sensor run
    out = CL.rt_run_multisensor(pm, hl, 0, 2, K, LEVELS)
    sc = CL.SceneLin(pm, hl, 0, 2, K)
    sc.run(lanes=1, fold=False)
    torch.cuda.synchronize()
    for g, r in zip(out, sc.results_host()):
        assert np.array_equal(g[0], r)
    e_ms = {}
    for f, name in enumerate(("uw", "dw", "uwd", "dwd")):
        assert np.array_equal(out[f][1], out[f][3])
        for i, l in enumerate(LEVELS[:3]):
            e_ms["%s%d" % (name, l)] = _rel(out[f][i], ref[f][i])
    print("SE lin %-10s %-3s S %2d %-8s %s multisensor: %s" % (kind, pol, S, which, FT.__name__,
                                                              " ".join("%s %.1e" % kv for kv in e_ms.items())))
    # the flux run: the m = 0 level vectors of the same oracles through flux_lin_oracle's quadrature
    om0 = dataclasses.replace(om, m_max=0)
    f0 = {}
    oracle_lin_levels(kind, om0, S, which, LEVELS, full=f0)
    fref = FL.fluxes_lin_from_vectors(om0, OL.LinModel(list(_gases(S))), LEVELS, f0, solar=which == "all")
    res = CL.rt_run_fluxes(pm, hl, 0, 2, K, LEVELS)
    e_fl = {k: _rel(getattr(res, k), getattr(fref, k)) for k in FL.FO.FIELDS + DOT_FIELDS}
    assert res.up_dot.shape == (len(LEVELS), S, Pa)
    print("SE lin %-10s %-3s S %2d %-8s %s fluxes: %s" % (kind, pol, S, which, FT.__name__,
                                                         " ".join("%s %.1e" % kv for kv in e_fl.items())))
    assert max(e_lin.values()) <= (1e-13 if FT == np.float64 else 1e-5), e_lin
    assert max(e_ms.values()) <= _tol(FT), e_ms
    assert max(e_fl.values()) <= _tol(FT), e_fl


def test_explicit_emissivity_has_no_emissivity_derivative(vsm, arch):
    """With a stated emissivity the surface slot carries the reflection alone (no vsm_surface_emission_lin call)."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    S = 5
    pm, om, _ = scene(vsm, arch, "lambertian", "IQU", S, window=True)
    pm.sources = _sources(H, "emission", S, emissivity=0.8)
    hl = H.LinModel(list(_gases(S)))
    ref = oracle_lin_levels("lambertian", om, S, "emission", [0], emissivity=0.8)
    kir = oracle_lin_levels("lambertian", om, S, "emission", [0])
    got = CL.rt_run_lin(pm, hl, 0, 2, 1)
    assert _rel(kir[2][0][..., 2], ref[2][0][..., 2]) > 1e-3
    for g, r in zip(got, ref):
        assert _rel(g, r[0]) <= 1e-13, _rel(g, r[0])


def test_skin_slots_without_a_forward_emission_and_limits(vsm, arch):
    """B_surface = 0 with skin tables: no forward emission, the skin slots still there; slot count above 64 and graph replay refused."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    S = 5
    pm, om, _ = scene(vsm, arch, "lambertian", "I", S, window=True)
    hl = H.LinModel(list(_gases(S)))
    Bsd = _tables(S)[1]
    pm.sources = (H.SurfaceEmission(B_surface=np.zeros(S), B_surface_dot=Bsd),)
    R, T, Rd, Td = CL.rt_run_lin(pm, hl, 0, 2, 1)
    assert Rd.shape[-1] == 5 and np.all(R == 0) and np.all(Rd[..., :3] == 0)
    ref = SE.emission_response(om, Bsd[1], [0])
    assert _rel(Rd[..., 4], ref[0][0]) <= 1e-13 and _rel(Td[..., 4], ref[1][0]) <= 1e-13
    pm.sources = (H.SurfaceEmission(B_surface=_B_surface(S), B_surface_dot=np.ones((62, S))),)
    with pytest.raises(vsm._lib.VSMError, match="skin"):
        CL.SceneLin(pm, hl, 0, 2, 1)
    pm.sources = (H.SurfaceEmission(B_surface=_B_surface(S)),)          # without B_surface_dot: taken, nSkin = 0
    sc = CL.SceneLin(pm, hl, 0, 2, 1)
    assert sc.nSkin == 0 and sc.Rd.shape[0] == 3
    with pytest.raises(NotImplementedError, match="graph"):
        sc.run(graph=True)
    out = CL.rt_run_multisensor(pm, hl, 0, 2, 1, [3])
    assert out[2][0].shape[-1] == 3 and np.max(np.abs(out[0][0])) > 0


def _all_fields(res):
    return [getattr(res, k) for k in FL.FO.FIELDS + DOT_FIELDS + ("absorbed", "surface_absorbed", "absorbed_dot", "surface_absorbed_dot")]


def test_skin_slots_carry_the_stated_emissivity(vsm, arch):
    """B_surface = 0 with emissivity = 0.8 and skin tables: there is no forward emission, and the skin slots of all three linearized
    drivers emit with the STATED emissivity (albedo 0.3: Kirchhoff would give 0.7, an eighth less), against the oracle's response
    for emissivity = 0.8, at the bounds of the driver test."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    S, P = 5, 3
    pm, om, _ = scene(vsm, arch, "lambertian", "IQU", S, window=True)
    Bsd = _tables(S)[1]
    for emissivity in (0.8, np.linspace(0.6, 1.0, S)):
        pm.sources = (H.SurfaceEmission(B_surface=np.zeros(S), emissivity=emissivity, B_surface_dot=Bsd),)
        hl, lin = H.LinModel(list(_gases(S))), OL.LinModel(list(_gases(S)))
        ref = SE.emission_response_lin(om, lin, np.zeros(S), LEVELS, emissivity=emissivity, B_surface_dot=Bsd)
        kir = SE.emission_response_lin(om, lin, np.zeros(S), [0], B_surface_dot=Bsd)
        assert _rel(kir[2][0][..., P:], ref[2][0][..., P:]) > 0.05
        R, T, Rd, Td = CL.rt_run_lin(pm, hl, 0, 2, 1)
        assert Rd.shape[-1] == P + 2 and np.all(R == 0) and np.all(Rd[..., :P] == 0) and np.all(Td[..., :P] == 0)
        e = {}
        for k in (P, P + 1):
            e["Rd%d" % k], e["Td%d" % k] = _rel(Rd[..., k], ref[2][0][..., k]), _rel(Td[..., k], ref[3][0][..., k])
        assert max(e.values()) <= 1e-13, e
        out = CL.rt_run_multisensor(pm, hl, 0, 2, 1, LEVELS)
        e = {}
        for i, l in enumerate(LEVELS):
            e["uwd%d_%d" % (l, i)], e["dwd%d_%d" % (l, i)] = _rel(out[2][i], ref[2][i]), _rel(out[3][i], ref[3][i])
        assert max(e.values()) <= 1e-12, e
        om0 = dataclasses.replace(om, m_max=0)
        vec = SE.level_vectors_lin(om0, lin, LEVELS, np.zeros(S), emissivity=emissivity, B_surface_dot=Bsd)
        fref = FL.fluxes_lin_from_vectors(om0, lin, LEVELS, vec, solar=False)
        res = CL.rt_run_fluxes(pm, hl, 0, 2, 1, LEVELS)
        e = {k: _rel(getattr(res, k), getattr(fref, k)) for k in DOT_FIELDS}
        print("SE lin stated emissivity %s: %s" % (np.ndim(emissivity), " ".join("%s %.1e" % kv for kv in e.items())))
        assert np.max(np.abs(fref.up_dot[..., P:])) > 0 and max(e.values()) <= 1e-12, e


@pytest.mark.parametrize("solar_only", [True, False], ids=["solar", "solar_thermal"])
def test_idle_source_keeps_the_bits_of_the_linearized_runs(vsm, arch, solar_only):
    """An all-zero SurfaceEmission without dot tables runs nothing: rt_run_lin, CoreRTLin.rt_run_multisensor and
    CoreRTLin.rt_run_fluxes give, on a second scene object, the bits and shapes of the model whose source tuple does not hold
    it -- beside a SolarBeam alone (no thermal slot at all: the flux run's sink has no thermal half) and beside a ThermalEmission."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    S = 5
    base = (H.SolarBeam(),) if solar_only else (H.SolarBeam(), H.ThermalEmission(B_layer=_B_layer(S), B_layer_dot=_tables(S)[0]))
    pa, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=base, window=True)
    pb, _, _ = scene(vsm, arch, "lambertian", "IQU", S, sources=base + (H.SurfaceEmission(B_surface=np.zeros(S)),), window=True)
    hl = H.LinModel(list(_gases(S)))
    sb = CL.SceneLin(pb, hl, 0, 2, 1)
    assert sb.nSkin == 0 and sb.has_thermal == (not solar_only) and sb.fwd.surface_B is None and sb.fwd.surface_emissivity is None
    for a, b in zip(CL.rt_run_lin(pa, hl, 0, 2, 1), CL.rt_run_lin(pb, hl, 0, 2, 1)):
        assert np.array_equal(a, b)
    oa, ob = CL.rt_run_multisensor(pa, hl, 0, 2, 1, LEVELS), CL.rt_run_multisensor(pb, hl, 0, 2, 1, LEVELS)
    for fa, fb in zip(oa, ob):
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    fa, fb = CL.rt_run_fluxes(pa, hl, 0, 2, 1), CL.rt_run_fluxes(pb, hl, 0, 2, 1)
    for x, y in zip(_all_fields(fa), _all_fields(fb)):
        assert x.shape == y.shape and np.array_equal(x, y)
    assert np.all(np.isfinite(fb.up_dot)) and np.max(np.abs(fb.up)) > 0


@pytest.mark.parametrize("kirchhoff", [True, False], ids=["kirchhoff", "spectral_emissivity"])
def test_linearized_blocks_are_bit_identical(vsm, arch, kirchhoff):
    """max_points = 2 on 5 points (blocks of 2, 2, 1) over the per-point surface layer: every block of the linearized multi-sensor
    and flux runs slices B_surface, B_surface_dot and the emissivity with its points."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    S = 5
    se_kw = {} if kirchhoff else dict(emissivity=np.linspace(0.6, 1.0, S))
    pm, _, _ = scene(vsm, arch, "legendre", "IQU", S, sources=_sources(H, "all", S, **se_kw), window=True)
    hl = H.LinModel(list(_gases(S)))
    one, blk = CL.rt_run_multisensor(pm, hl, 0, 2, 3, LEVELS), CL.rt_run_multisensor(pm, hl, 0, 2, 3, LEVELS, max_points=2)
    for fa, fb in zip(one, blk):
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert np.max(np.abs(one[2][2][..., -1])) > 0          # (the last skin slot at level Nz)
    fa, fb = CL.rt_run_fluxes(pm, hl, 0, 2, 3), CL.rt_run_fluxes(pm, hl, 0, 2, 3, max_points=2)
    for x, y in zip(_all_fields(fa), _all_fields(fb)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind,pol,S,which", [("lambertian", "IQU", 23, "all"), ("rpv", "I", 5, "thermal")],
                         ids=["lambertian_IQU_S23_all", "rpv_I_S5_thermal"])
def test_level_runs_over_the_thick_column(vsm, arch, kind, pol, S, which):
    """The linearized level runs in FP64 over the ordinary column of the forward tests (optical depths 0.04 .. 0.4 per layer, 8 or 9
    doublings), where users run them, at the bound the issue gives the level runs: their forward tolerance, 1e-12.  (rt_run_lin's
    1e-13 and the FP32 bounds are bounds for columns of few doublings: _arrays of test_gpu_surface_emission.py.)"""
    H, CL = vsm.host_model, vsm.CoreRTLin
    pm, om, _ = scene(vsm, arch, kind, pol, S, window=False)
    pm.sources = _sources(H, which, S)
    gases = list(_gases(S, window=False))
    hl, K = H.LinModel(gases), NSURF[kind]
    ref = oracle_lin_levels(kind, om, S, which, LEVELS, window=False)
    out = CL.rt_run_multisensor(pm, hl, 0, 2, K, LEVELS)
    e = {}
    for f, name in enumerate(("uw", "dw", "uwd", "dwd")):
        for i, l in enumerate(LEVELS[:3]):
            e["%s%d" % (name, l)] = _rel(out[f][i], ref[f][i])
    om0 = dataclasses.replace(om, m_max=0)
    f0 = {}
    oracle_lin_levels(kind, om0, S, which, LEVELS, full=f0, window=False)
    fref = FL.fluxes_lin_from_vectors(om0, OL.LinModel(gases), LEVELS, f0, solar=which == "all")
    res = CL.rt_run_fluxes(pm, hl, 0, 2, K, LEVELS)
    e.update({k: _rel(getattr(res, k), getattr(fref, k)) for k in FL.FO.FIELDS + DOT_FIELDS})
    print("SE lin thick %s %s S %d %s: %s" % (kind, pol, S, which, " ".join("%s %.1e" % kv for kv in e.items())))
    assert max(e.values()) <= 1e-12, e
