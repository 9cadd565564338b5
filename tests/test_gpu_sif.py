"""SurfaceSIF on the device: the injection kernel (vsm_surface_sif_*), the unit-emission response kernel
(vsm_surface_emission_response_*), and the drivers that take the source -- CoreRT.rt_run (every walk), rt_run_multisensor,
CoreRTRaman.rt_run, CoreRTLin.rt_run_lin with its SIF slots -- against tests/sif_oracle.py (itself pinned on the CPU by
tests/test_oracle_sif.py), plus the refusals of every other driver and the idle cost of a model without the source.

Scenes: S = 3 points, 3 layers, geometry (40, [30, 5], [0, 60]), albedo 0.2, two gas columns, as tests/test_gpu_thermal_lin.py.
Source: SIF0[0, s] = a (1 + 0.3 s) with a = 0.1 (tests/test_oracle_sif.py checks that the SIF share of R then lies between 0.1 and
10 times the solar part) and two derivative tables (shape, slope).

Bounds: those of the existing tests of the same walk -- native FP64 run 1e-8 (test_gpu_parity: the golden scenes), the reference
layout walk with a non-scattering layer, the spectral Lambertian surfaces, streams and the full output 1e-9, FP32 1e-2 against the
FP64 oracle; multi-sensor max(1e-10, twice rt_run's own deviation) per Stokes component (test_gpu_multisensor); Raman 1e-8
(test_gpu_raman); rt_run_lin R, T 1e-9 and every slot 1e-8 of each array's maximum, the albedo finite difference max 1e-3 / mean
1e-4, FP32 1e-2 / 5e-4 / 2e-3 (test_gpu_lin, test_gpu_thermal_lin); the response kernel 1e-12 (FP64) / 2e-5 (FP32) against its
operator-level composition and ten times that against numpy (test_gpu_multisensor_thermal::test_level_src_kernel)."""
import ctypes as C
import functools
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import sif_oracle as SO  # noqa: E402
import thermal_lin_oracle as TL  # noqa: E402
import ms_thermal_oracle as MT  # noqa: E402
from test_oracle_sif import (RAMAN_GEO, RAMAN_SHIFTS, RAMAN_W_IE, raman_arrays, raman_oracle_model, sif0, sif0_dot)  # noqa: E402
from test_gpu_multisensor import _err_per_level  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S, L = 3, 3
GEO = (40.0, [30.0, 5.0], [0.0, 60.0])
SHAPES = [("I", 9), ("IQU", 33), ("IQUV", 25), ("IQUV", 61)]     # the shapes of tests/test_gpu_thermal_lin.py, one per kernel family


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


def _arrays():
    rng = np.random.default_rng(0)
    tau_rayl = np.tile(0.03 * np.ones(L), (S, 1))
    ga, gb = 10.0 ** rng.uniform(-2.5, -0.5, (S, L)), 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    return dict(tau_rayl=tau_rayl, tau_abs=ga + gb, depol=0.0279, m_max=2), ga, gb


def _src(H, dot=False, solar=True, table=None):
    sif = H.SurfaceSIF(sif0() if table is None else table, sif0_dot() if dot else None)
    return (H.SolarBeam(), sif) if solar else (sif,)


def _pm(vsm, arch, pol, l_trunc, sources, albedo=0.2, **over):
    kw, _, _ = _arrays()
    kw.update(over)
    if "surface" not in kw:
        kw["albedo"] = albedo
    return vsm.host_model.model_from_arrays(arch, pol, l_trunc, *GEO, sources=sources, **kw)


def _om(pol, l_trunc, albedo=0.2, FT=np.float64, **over):
    kw, _, _ = _arrays()
    kw.update(over)
    return O.build_model(pol, l_trunc, *GEO, albedo=albedo, FT=FT, **kw)


# ---- the injection kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_point"])
@pytest.mark.parametrize("pol_name", ["I", "IQU"])
@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_surface_sif_kernel(vsm, arch, FT, pol_name, shared):
    """vsm_surface_sif_*: j0- = 7 + 2 sif in the layer's float type exactly (one exact doubling, one add), on a layer filled with 7;
    every other array keeps its 7.  More than one block (N S > 256), an odd point count, shared and per-point surface layers."""
    CR, H = vsm.CoreRT, vsm.host_model
    pol = H.polarization_type(pol_name)
    n, Nq, S_ = pol.n, 7, 41
    N = Nq * n
    rng = np.random.default_rng(n)
    sif = (0.3 * rng.standard_normal((n, S_))).astype(FT)
    layer = CR.AddedLayer(FT, arch, N, S_, shared=shared)
    others = [layer.r_mp, layer.t_pp, layer.r_pm, layer.t_mm, layer.j0_p]
    for t in others + [layer.j0_m]:
        t.fill_(7.0)
    table = vsm.Architectures.array_type(arch)(np.ascontiguousarray(sif))
    assert CR.surface_source_contribute_(table, H.LambertianSurfaceScalar(0.2), layer, 0) is True
    torch.cuda.synchronize()
    want = np.full((S_, N), 7.0, dtype=FT)
    for c in range(n):
        want[:, c::n] += (FT(2) * sif[c])[:, None]
    got = vsm.Architectures.to_host(layer.j0_m)
    assert got.dtype == FT and np.array_equal(got, want)
    assert all(bool(torch.all(t == 7.0)) for t in others)
    # the no-op rules of the host sibling: m > 0, no table, a non-Lambertian surface (with the warning)
    assert CR.surface_source_contribute_(table, H.LambertianSurfaceScalar(0.2), layer, 1) is False
    assert CR.surface_source_contribute_(None, H.LambertianSurfaceScalar(0.2), layer, 0) is False
    with pytest.warns(UserWarning, match="SurfaceSIF has no effect"):
        assert CR.surface_source_contribute_(table, H.rpvSurfaceScalar(0.1, 0.1, 0.7, -0.1), layer, 0) is False
    torch.cuda.synchronize()
    assert np.array_equal(vsm.Architectures.to_host(layer.j0_m), want)


# ---- the response kernel ---------------------------------------------------------------------------------------------------------
def _kernel_pol(H, N):
    return H.polarization_type("IQUV" if N % 4 == 0 else ("IQU" if N % 3 == 0 else "I"))


def _response_inputs(N, S_, rng, shared):
    """Random contractive operators, as test_gpu_multisensor._rand_level_inputs builds them, and a transmission block."""
    A = rng.random((S_, N, N)) * (0.6 / N)
    B = rng.random((1 if shared else S_, N, N)) * (0.6 / N)
    T = rng.random((S_, N, N)) * (1.0 / N) + 0.5 * np.eye(N)[None]
    return A, B, T


def _emission_response_case(vsm, N, FT, K, nV, shared, rng, inputs=_response_inputs, S_=5, vza_max=80.0, oplevel=True):
    """One vsm_surface_emission_response_* call, its operator-level composition (oplevel) and numpy on the operators of
    inputs(N, S_, rng, shared) -> (A, B, T): a list of (name, k, fused, composition | None, numpy) over up / dn and the components."""
    MSd, H = vsm.core_rt_ms, vsm.host_model
    pol = _kernel_pol(H, N)
    n = pol.n
    comps = [n - 1] if K == 1 else [c % n for c in (0, 1, 3)]
    dt = torch.float64 if FT == np.float64 else torch.float32
    dev = torch.device("cuda", 0)
    lay = lambda X: torch.tensor(np.ascontiguousarray(X.transpose(0, 2, 1)), dtype=dt, device=dev)
    qp = types.SimpleNamespace(qp_mu=np.linspace(1.0, 0.05, N // n))      # (the rows of the viewing angles)
    w = 0.5 / math.pi
    vza, vaz = list(np.linspace(0.0, vza_max, nV)), list(np.linspace(0.0, 345.0, nV))
    row0, wts = vsm.CoreRT._vza_rows_weights(pol, vza, vaz, qp, 0, w, dt)
    rows = np.array([[row0[v] + c for v in range(nV)] for c in range(n)])
    wt = np.array([[wts[v + nV * c] for v in range(nV)] for c in range(n)], dtype=np.float64)
    A, B, T = inputs(N, S_, rng, shared)
    tA, tB, tT = lay(A), lay(B), lay(T)
    fused = [torch.full((K, S_, n, nV), 0.25, dtype=dt, device=dev) for _ in range(2)]
    opl = [torch.full((K, S_, n, nV), -0.5, dtype=dt, device=dev) for _ in range(2)]
    MSd.surface_emission_response_(pol, qp, vza, vaz, w, tA, tT, tB, comps, *fused)
    if oplevel:
        MSd.surface_emission_response_(pol, qp, vza, vaz, w, tA, tT, tB, comps, *opl, oplevel=True)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("emission response kernel")
    Bf = np.broadcast_to(B, A.shape)
    M = np.eye(N)[None] - Bf @ A
    out = []
    for k, c in enumerate(comps):
        e = np.zeros((S_, N))
        e[:, c::n] = 1
        y = np.linalg.solve(M, e[..., None])[..., 0]
        up = wt[None] * np.einsum("sij,sj->si", T, y)[:, rows]
        dn = wt[None] * np.einsum("sij,sj->si", A, y)[:, rows]
        for name, f, o, r in (("up", fused[0], opl[0], up), ("dn", fused[1], opl[1], dn)):
            xf, xo = f[k].cpu().numpy().astype(np.float64), o[k].cpu().numpy().astype(np.float64)
            out.append((name, k, xf, xo if oplevel else None, r))
    return out


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("N", [3, 16, 61, 128])
@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_emission_response_kernel(vsm, N, FT, K):
    """vsm_surface_emission_response_*: the fused kernel against the operator-level composition (one vsm_level_radiance_oplevel_*
    call per component and a batched row product) and against numpy; shared and per-point B, 3 and 70 viewing angles."""
    rng = np.random.default_rng(N + K)
    tol = 1e-12 if FT == np.float64 else 2e-5
    for nV in (3, 70):
        for shared in (False, True):
            for name, k, xf, xo, r in _emission_response_case(vsm, N, FT, K, nV, shared, rng):
                assert np.max(np.abs(r)) > 0
                assert np.max(np.abs(xf - xo)) <= tol * np.max(np.abs(xo)), (name, N, nV, shared, k)
                assert np.max(np.abs(xf - r)) <= 10 * tol * np.max(np.abs(r)), (name, N, nV, shared, k)


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", [0, 5])
def test_emission_response_kernel_refuses_bad_counts(vsm, FT, K):
    """K outside 1..4 (and N > 128) is an argument error of the entry point: nothing is launched, the outputs stay."""
    CR, H = vsm.CoreRT, vsm.host_model
    N, S_, nV = 16, 3, 3
    pol = _kernel_pol(H, N)
    dt = torch.float64 if FT == np.float64 else torch.float32
    dev = torch.device("cuda", 0)
    A, B, T = _response_inputs(N, S_, np.random.default_rng(0), False)
    lay = lambda X: torch.tensor(np.ascontiguousarray(X.transpose(0, 2, 1)), dtype=dt, device=dev)
    tA, tB, tT = lay(A), lay(B), lay(T)
    qp = types.SimpleNamespace(qp_mu=np.linspace(1.0, 0.05, N // pol.n))
    vza, vaz = [0.0, 30.0, 60.0], [0.0, 45.0, 120.0]
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, 0, 1.0, dt)
    up = torch.full((5, S_, pol.n, nV), 0.25, dtype=dt, device=dev)
    dn = torch.full_like(up, -0.5)
    comps = (C.c_int * 5)(0, 1, 2, 3, 0)
    fn = getattr(vsm._lib.lib(), "vsm_surface_emission_response_" + ("f64" if FT == np.float64 else "f32"))
    args = lambda k, n_=N: (n_, pol.n, S_, k, comps, nV, row0, w, CR._ptr(tA), CR._ptr(tT), CR._ptr(tB), N * N, CR._ptr(up), CR._ptr(dn),
                            CR._stream_ptr())
    assert fn(*args(K)) == 1                                    # VSM_ERR_INVALID_ARG
    assert b"K = " in vsm._lib.lib().vsm_last_error()
    assert fn(*args(2, 132)) == 1                               # N > 128 (no kernel reads the 16-row operands)
    torch.cuda.synchronize()
    assert torch.all(up == 0.25) and torch.all(dn == -0.5)
    with pytest.raises(vsm.VSMError):
        vsm.core_rt_ms.surface_emission_response_(pol, qp, vza, vaz, 1.0, tA, tT, tB, [0] * K, up, dn)
    assert fn(*args(4)) == 0                                    # the largest count the kernel takes
    torch.cuda.synchronize()
    vsm._lib.check_device_status("emission response kernel")
    assert torch.all(torch.isfinite(up[:4])) and not torch.any(up[:4] == 0.25) and torch.all(up[4] == 0.25)


# ---- rt_run ----------------------------------------------------------------------------------------------------------------------
def test_rt_run_native_vs_oracle(vsm, arch):
    """The native run (Stokes_IQU, N = 60) with an unpolarized and with a polarized emission (a U row: the (U,V) block of m = 0)."""
    H = vsm.host_model
    for table in (sif0(), np.stack([sif0(), 0.2 * sif0(), -0.3 * sif0()])):
        pm = _pm(vsm, arch, "IQU", 33, _src(H, table=table))
        scene = vsm.CoreRT.Scene(pm)
        assert len(scene._native_moments()) == 3 and scene.sif is not None
        R, T = vsm.CoreRT.rt_run(pm)
        Ro, To = SO.rt_run_sif(_om("IQU", 33), table)
        print("rt_run SIF native: R %.2e T %.2e" % (_rel(R, Ro), _rel(T, To)))
        assert _rel(R, Ro) < 1e-8 and _rel(T, To) < 1e-8
    R0, _ = vsm.CoreRT.rt_run(_pm(vsm, arch, "IQU", 33, None))
    assert _rel(R, R0) > 0.1                                    # (the source is there)


def test_rt_run_reference_layout_walk_vs_oracle(vsm, arch):
    """A column with a non-scattering layer: no moment runs on the native composite."""
    H = vsm.host_model
    kw, _, _ = _arrays()
    tr = kw["tau_rayl"].copy()
    tr[:, 1] = 0.0
    pm = _pm(vsm, arch, "IQU", 9, _src(H), tau_rayl=tr)
    assert vsm.CoreRT.Scene(pm)._native_moments() == set()
    R, T = vsm.CoreRT.rt_run(pm)
    Ro, To = SO.rt_run_sif(_om("IQU", 9, tau_rayl=tr), sif0())
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9, (_rel(R, Ro), _rel(T, To))


def test_rt_run_legendre_surface_and_shard(vsm, arch):
    """LambertianSurfaceLegendre (per-point surface layer): against the oracle; Scene(model, spec_slice) = the slice of the full
    run bit for bit (the table is sliced with the scene's columns), also over the scalar surface."""
    H = vsm.host_model
    coeff = [0.25, 0.08, -0.03]
    pm = _pm(vsm, arch, "IQU", 9, _src(H), surface=H.LambertianSurfaceLegendre(coeff))
    R, T = vsm.CoreRT.rt_run(pm)
    Ro, To = SO.rt_run_sif(_om("IQU", 9, albedo=np.asarray(O.legendre_albedo(coeff, S))), sif0())
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9, (_rel(R, Ro), _rel(T, To))
    for model, full in ((pm, R), (_pm(vsm, arch, "IQU", 9, _src(H)), None)):
        if full is None:
            full = vsm.CoreRT.rt_run(model)[0]
        part = vsm.CoreRT.Scene(model, slice(1, 3))
        Rp = vsm.Architectures.to_host(part.run()[0]).transpose(2, 1, 0)
        assert np.array_equal(Rp, full[:, :, 1:3])


def test_rt_run_fp32(vsm, arch):
    H = vsm.host_model
    pm = _pm(vsm, arch, "IQU", 33, _src(H), float_type=np.float32)
    R, T = vsm.CoreRT.rt_run(pm)
    Ro, To = SO.rt_run_sif(_om("IQU", 33), sif0())
    assert R.dtype == np.float32
    assert _rel(R, Ro) < 1e-2 and _rel(T, To) < 1e-2, (_rel(R, Ro), _rel(T, To))


def test_rt_run_streams_and_full_output(vsm, arch):
    H = vsm.host_model
    pm = _pm(vsm, arch, "IQU", 9, _src(H))
    om = _om("IQU", 9)
    per_m, hd = [], {}
    Ro, To = SO.rt_run_sif(om, sif0(), per_m=per_m, hdrf=hd)
    st = vsm.CoreRT.rt_run_streams(pm)
    for mi, d in enumerate(per_m):
        assert _rel(st.J_m_per_m[mi][:, 0, :].T, d["J0_m"]) < 1e-9 and _rel(st.J_p_per_m[mi][:, 0, :].T, d["J0_p"]) < 1e-9, mi
    R, T, ieR, ieT, hdr, bhr_uw, bhr_dw = vsm.CoreRT.rt_run(pm, full_output=True)
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9
    assert _rel(hdr, hd["hdr"]) < 1e-9 and _rel(bhr_uw, hd["bhr_uw"][0]) < 1e-9 and _rel(bhr_dw, hd["bhr_dw"][0]) < 1e-9
    hd0 = {}
    O.rt_run(om, hdrf=hd0)
    assert _rel(hd["hdr"], hd0["hdr"]) > 0.1                    # (hdr carries the emission)


def test_run_graph_equals_run(vsm, arch):
    H = vsm.host_model
    scene = vsm.CoreRT.prepare_scene(_pm(vsm, arch, "IQU", 33, _src(H)))
    ref = [x.clone() for x in scene.run()]
    for _ in range(2):
        out = scene.run_graph()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, out))


def test_rpv_surface_is_a_no_op_with_a_warning(vsm, arch):
    H = vsm.host_model
    rpv = H.rpvSurfaceScalar(0.1, 0.1, 0.7, -0.1)
    base = vsm.CoreRT.rt_run(_pm(vsm, arch, "IQU", 9, None, surface=rpv))
    with pytest.warns(UserWarning, match="SurfaceSIF has no effect") as rec:
        got = vsm.CoreRT.rt_run(_pm(vsm, arch, "IQU", 9, _src(H), surface=rpv))
    assert len([r for r in rec if "SurfaceSIF" in str(r.message)]) == 1      # once per scene, not once per moment
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


@pytest.mark.parametrize("thermal", [False, True], ids=["solar", "solar+thermal"])
def test_rt_run_multisensor(vsm, arch, thermal):
    """Levels [0, 1, 3], with and without thermal=True: every level against the oracle, level 0 = rt_run bit for bit."""
    H = vsm.host_model
    levels = [0, 1, 3]
    B = 0.1 + 0.02 * np.arange(L)[:, None] * (1.0 + np.arange(S))[None, :]
    src = _src(H) + ((H.ThermalEmission(B_layer=B),) if thermal else ())
    pm = _pm(vsm, arch, "IQU", 9, src)
    om = _om("IQU", 9)
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=thermal)
    R, T = vsm.CoreRT.rt_run(pm)
    assert np.array_equal(uw[0], R) and np.array_equal(dw[0], T)
    ur, dr = SO.ms_sif(om, levels, sif0())
    Ro, To = SO.rt_run_sif(om, sif0())
    if thermal:
        ut, dth = MT.ms_thermal_reference(om, B, levels)
        ur, dr = [a + b for a, b in zip(ur, ut)], [a + b for a, b in zip(dr, dth)]
        Rt, Tt = O.rt_run_thermal(om, B)
        Ro, To = Ro + Rt, To + Tt
    e = max(_err_per_level(uw, ur), _err_per_level(dw, dr))
    e_rt = max(_err_per_level([R], [Ro]), _err_per_level([T], [To]))
    print("MS SIF thermal=%s: %.2e (rt_run %.2e)" % (thermal, e, e_rt))
    assert e <= max(1e-10, 2 * e_rt), (e, e_rt)
    base = vsm.CoreRT.rt_run_multisensor(_pm(vsm, arch, "IQU", 9, src[:1] + src[2:]), levels, thermal=thermal)
    for i in range(3):
        assert _rel(uw[i], base[0][i]) > 0.1, i                 # every level sees the emission


# ---- Raman -----------------------------------------------------------------------------------------------------------------------
def _raman_pm(vsm, arch, S_, sources):
    kw, F0 = raman_arrays(S_)
    pm = vsm.host_model.model_from_arrays(arch, "IQU", 7, *RAMAN_GEO, sources=sources, **kw)
    pm.varpi_Cabannes = 0.96
    pm.F0 = F0
    graman = O.get_greek_rayleigh(6.0 / 7.0 * 0.5)
    return pm, vsm.CoreRTRaman.RRS(RAMAN_SHIFTS, RAMAN_W_IE, vsm.host_model.GreekCoefs(**vars(graman)))


def test_raman_rt_run_vs_oracle_blocked_and_linear(vsm, arch):
    """CoreRTRaman.rt_run (Stokes_IQU, l_trunc = 7, S = 24) against the oracle; blocked under max_points bit-identical to one pass;
    doubling the table doubles (R, ieR) - (R, ieR)_0."""
    H, RR = vsm.host_model, vsm.CoreRTRaman
    S_ = 24
    tab = sif0(S_=S_)
    pm, prs = _raman_pm(vsm, arch, S_, (H.SolarBeam(), H.SurfaceSIF(tab)))
    got = RR.rt_run(prs, pm, 1)
    om, ors = raman_oracle_model(S_)
    ref = SO.rt_run_rrs_sif(om, ors, tab)
    for name, g, r in zip(("R", "T", "ieR", "ieT"), got, ref):
        assert _rel(g, r) <= 1e-8, (name, _rel(g, r))
    for n_ in (10, 3):
        blk = RR.rt_run(prs, pm, 1, max_points=n_)
        for a, b in zip(got, blk):
            assert a.shape == b.shape and np.array_equal(a, b), n_
    base = RR.rt_run(prs, _raman_pm(vsm, arch, S_, None)[0], 1)
    twice = RR.rt_run(prs, _raman_pm(vsm, arch, S_, (H.SolarBeam(), H.SurfaceSIF(2 * tab)))[0], 1)
    for i in (0, 2):
        d1, d2 = got[i] - base[i], twice[i] - base[i]
        assert np.max(np.abs(d1)) > 1e-3 * np.max(np.abs(base[i]))
        assert np.max(np.abs(d2 - 2 * d1)) <= 1e-9 * np.max(np.abs(twice[i])), i
    # a polarized emission leaves the Stokes_IQ sub-scene of m = 0
    pol_tab = np.stack([tab, 0 * tab, 0.2 * tab])
    assert RR.SceneRRS(prs, pm, 1).sub0 is not None
    pm_u = _raman_pm(vsm, arch, S_, (H.SolarBeam(), H.SurfaceSIF(pol_tab)))[0]
    assert RR.SceneRRS(prs, pm_u, 1).sub0 is None
    for name, g, r in zip(("R", "T", "ieR", "ieT"), RR.rt_run(prs, pm_u, 1), SO.rt_run_rrs_sif(om, ors, pol_tab)):
        assert _rel(g, r) <= 1e-8, (name, _rel(g, r))


# ---- rt_run_lin ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lin_oracle(pol, l_trunc, solar=True, FT=np.float64):
    """The oracle of the gas scene with the source and its two slots, computed once per case and only read."""
    _, ga, gb = _arrays()
    om = _om(pol, l_trunc, FT=FT)
    if not solar:        # without a SolarBeam the solar slot runs with F0 = 0
        om.F0 = np.zeros((om.pol.n, S), dtype=FT)
    return SO.rt_run_lin_sif(om, OL.LinModel([ga, gb]), sif0(), sif0_dot())


def _check_lin(got, ref, nslots):
    R, T, Rd, Td = got
    Ro, To, Rdo, Tdo = ref
    assert Rd.shape == Rdo.shape and Rd.shape[-1] == nslots
    assert _rel(R, Ro) < 1e-9 and _rel(T, To) < 1e-9, (_rel(R, Ro), _rel(T, To))
    for p in range(nslots):
        assert np.max(np.abs(Rdo[..., p])) > 0
        assert _rel(Rd[..., p], Rdo[..., p]) < 1e-8 and _rel(Td[..., p], Tdo[..., p]) < 1e-8, \
            (p, _rel(Rd[..., p], Rdo[..., p]), _rel(Td[..., p], Tdo[..., p]))


def _lin_vs_oracle_and_fd(vsm, arch, pol, l_trunc, solar):
    H = vsm.host_model
    _, ga, gb = _arrays()
    mk = lambda alb, table: _pm(vsm, arch, pol, l_trunc, _src(H, dot=True, solar=solar, table=table), albedo=alb)
    pm = mk(0.2, sif0())
    got = vsm.CoreRTLin.rt_run_lin(pm, H.LinModel([ga, gb]), 0, 2, 1)
    _check_lin(got, _lin_oracle(pol, l_trunc, solar), 5)
    R, T, Rd, Td = got
    R0, T0 = vsm.CoreRT.rt_run(pm)
    h = 1e-4
    fd = (vsm.CoreRT.rt_run(mk(0.2 + h, sif0()))[0] - R0) / h
    if not solar:
        def beam_term(alb):
            m0 = _pm(vsm, arch, pol, l_trunc, None, albedo=alb)
            m0.F0 = np.zeros((m0.polarization_type.n, S))
            return vsm.CoreRT.rt_run(m0)[0]
        fd = fd - (beam_term(0.2 + h) - beam_term(0.2)) / h
    err = np.abs(fd - Rd[..., 2]) / np.abs(fd).max()
    print("SIF lin %s %d: albedo finite difference max %.2e mean %.2e" % (pol, l_trunc, err.max(), err.mean()))
    assert err.max() < 1e-3 and err.mean() < 1e-4
    for k, table in enumerate(sif0_dot()):
        Rk, Tk = vsm.CoreRT.rt_run(mk(0.2, sif0() + 0.5 * table))
        assert _rel(Rd[..., 3 + k], (Rk - R0) / 0.5) < 1e-8 and _rel(Td[..., 3 + k], (Tk - T0) / 0.5) < 1e-8, k


@pytest.mark.parametrize("pol,l_trunc", SHAPES)
def test_rt_run_lin_vs_oracle_and_fd(vsm, arch, pol, l_trunc):
    """rt_run_lin over (SolarBeam(), SurfaceSIF(SIF0, SIF0_dot)): R, T, the gas / albedo slots (which carry the emission's share)
    and the two SIF slots against the oracle; the albedo slot against a finite difference of the device's forward run; the SIF
    slots against (rt_run(SIF0 + h table) - rt_run(SIF0)) / h, exact up to rounding."""
    _lin_vs_oracle_and_fd(vsm, arch, pol, l_trunc, True)


def test_rt_run_lin_sif_only_model(vsm, arch):
    """The SIF source alone (F0 = 0), Stokes_IQU, N = 60.  CoreRT.rt_run's Lambertian layer carries its beam term with pol.I0 even at
    F0 = 0, the linearized builder uses F0 (test_gpu_thermal_lin.py::test_rt_run_lin_thermal_vs_oracle_and_fd): that term's own
    difference quotient is taken off the albedo difference; the SIF difference quotients cancel it."""
    _lin_vs_oracle_and_fd(vsm, arch, "IQU", 33, False)


def test_rt_run_lin_stokes_iq_subscene(vsm, arch, monkeypatch):
    """("IQU", 33) with the m = 0 Stokes_IQ sub-scene (SceneLin.sub0; LANE_POINTS lowered so that three points take it): the
    sub-scene carries the source and its slots.  A table with a U row leaves the sub-scene and still matches the oracle."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    monkeypatch.setattr(CL.SceneLin, "LANE_POINTS", 2)
    _, ga, gb = _arrays()
    hl = H.LinModel([ga, gb])
    pm = _pm(vsm, arch, "IQU", 33, _src(H, dot=True))
    scene = CL.SceneLin(pm, hl, 0, 2, 1)
    assert scene.sub0 is not None and scene.sub0.N == 2 * pm.quad_points.Nquad
    assert scene.sub0.nSIF == 2 and scene.sub0.fwd.sif.shape[0] == 2
    scene.run()
    torch.cuda.synchronize()
    _check_lin(scene.results_host(), _lin_oracle("IQU", 33), 5)
    # a U row in SIF0, and one in a derivative table only
    tab = np.stack([sif0(), 0 * sif0(), 0.2 * sif0()])
    dots = np.zeros((2, 3, S))
    dots[:, 0] = sif0_dot()
    dots[1, 2] = 0.1
    om = _om("IQU", 33)
    for t0, td in ((tab, dots), (sif0(3), dots)):
        sc = CL.SceneLin(_pm(vsm, arch, "IQU", 33, (H.SolarBeam(), H.SurfaceSIF(t0, td))), hl, 0, 2, 1)
        assert sc.sub0 is None and sc._sif_comps == [0, 2]
        sc.run()
        torch.cuda.synchronize()
        _check_lin(sc.results_host(), SO.rt_run_lin_sif(om, OL.LinModel([ga, gb]), t0, td), 5)


def test_rt_run_lin_slot_order_with_planck_slots(vsm, arch):
    """(SolarBeam, ThermalEmission(B, B_layer_dot = one table), SurfaceSIF(SIF0, two tables)): 3 + 1 + 2 slots, the SIF slots last;
    every earlier slot keeps its index and is the sum of the two sources' oracles."""
    H = vsm.host_model
    _, ga, gb = _arrays()
    B = 0.1 + 0.02 * np.arange(L)[:, None] * (1.0 + np.arange(S))[None, :]
    Bd = np.ones((1, L, S))
    src = (H.SolarBeam(), H.ThermalEmission(B_layer=B, B_layer_dot=Bd), H.SurfaceSIF(sif0(), sif0_dot()))
    got = vsm.CoreRTLin.rt_run_lin(_pm(vsm, arch, "IQU", 9, src), H.LinModel([ga, gb]), 0, 2, 1)
    om = _om("IQU", 9)
    sif = _lin_oracle("IQU", 9)
    th = TL.rt_run_thermal_lin(om, OL.LinModel([ga, gb]), B, Bd)
    ref = [sif[0] + th[0], sif[1] + th[1]]
    for a, b in ((sif[2], th[2]), (sif[3], th[3])):
        ref.append(np.concatenate([a[..., :3] + b[..., :3], b[..., 3:], a[..., 3:]], axis=-1))
    _check_lin(got, ref, 6)


def test_rt_run_lin_aerosol_slots(vsm, arch):
    """NAer = 1, NGas = 1, NSurf = 1 with the source: 9 + 2 slots against the oracle."""
    from tests.test_gpu_lin import _host_aerosol_scene
    H = vsm.host_model
    om, ol, pm, pl = _host_aerosol_scene(vsm, arch, "IQU", 9)
    S_ = om.tau_rayl.shape[0]
    t0, td = sif0(S_=S_), sif0_dot(S_)
    pm.sources = (H.SolarBeam(), H.SurfaceSIF(t0, td))
    got = vsm.CoreRTLin.rt_run_lin(pm, pl, 1, 1, 1)
    _check_lin(got, SO.rt_run_lin_sif(om, ol, t0, td), 11)


def test_rt_run_lin_fp32(vsm, arch):
    """Float32 (Stokes_IQU, N = 60): against the FP64 oracle at the reference's FP32 gate and against the FP32 oracle."""
    H = vsm.host_model
    _, ga, gb = _arrays()
    pm = _pm(vsm, arch, "IQU", 33, _src(H, dot=True), float_type=np.float32)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_lin(pm, H.LinModel([ga, gb]), 0, 2, 1)
    Ro, To, Rdo, Tdo = _lin_oracle("IQU", 33)
    assert R.dtype == np.float32 and Rd.dtype == np.float32 and Rd.shape == Rdo.shape
    assert _rel(R, Ro) < 1e-2 and _rel(T, To) < 1e-2
    for p in range(5):
        assert _rel(Rd[..., p], Rdo[..., p]) < 1e-2 and _rel(Td[..., p], Tdo[..., p]) < 1e-2, p
    R32, T32, Rd32, Td32 = _lin_oracle("IQU", 33, True, np.float32)
    print("SIF lin fp32: R %.2e T %.2e Rd %.2e Td %.2e" % (_rel(R, R32), _rel(T, T32), _rel(Rd, Rd32), _rel(Td, Td32)))
    assert _rel(R, R32) < 5e-4 and _rel(T, T32) < 5e-4
    for p in range(5):
        assert _rel(Rd[..., p], Rd32[..., p]) < 2e-3 and _rel(Td[..., p], Td32[..., p]) < 2e-3, p


# ---- refusals and idle cost ------------------------------------------------------------------------------------------------------
def test_refusals(vsm, arch):
    H, CL, RR = vsm.host_model, vsm.CoreRTLin, vsm.CoreRTRaman
    _, ga, gb = _arrays()
    hl = H.LinModel([ga, gb])
    pm = _pm(vsm, arch, "I", 9, _src(H, dot=True))
    # the single-scattering drivers
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        vsm.CoreRT.rt_run_ss(pm)
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        CL.rt_run_ss(pm, hl, 0, 2, 1)
    rpm, prs = _raman_pm(vsm, arch, 12, _src(H, table=sif0(S_=12)))
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        RR.rt_run_ss(prs, rpm, 1)
    # the Raman and the linearized multi-sensor run
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        RR.rt_run_multisensor(prs, rpm, [1])
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        CL.rt_run_multisensor(pm, hl, 0, 2, 1, [1])
    # graph replay of the linearized scene
    scene = CL.SceneLin(pm, hl, 0, 2, 1)
    with pytest.raises(NotImplementedError, match="graph"):
        scene.run(graph=True)
    eager = [t.clone() for t in scene.run(graph=False)]
    scene.graph_replay = True
    dflt = scene.run()                                          # graph=None: such a scene takes the eager path
    torch.cuda.synchronize()
    assert getattr(scene, "_graph", None) is None and all(torch.equal(a, b) for a, b in zip(eager, dflt))
    # 3 slots + 62 SIF slots
    with pytest.raises(vsm.VSMError, match="limit 64"):
        CL.SceneLin(_pm(vsm, arch, "I", 9, (H.SolarBeam(), H.SurfaceSIF(sif0(), np.ones((62, S))))), hl, 0, 2, 1)
    CL.SceneLin(_pm(vsm, arch, "I", 9, (H.SolarBeam(), H.SurfaceSIF(sif0(), np.ones((61, S))))), hl, 0, 2, 1)
    # shape errors, as for B_layer
    with pytest.raises(vsm.VSMError, match="spectral points"):
        vsm.CoreRT.rt_run(_pm(vsm, arch, "I", 9, (H.SolarBeam(), H.SurfaceSIF(np.ones(S + 1)))))
    with pytest.raises(vsm.VSMError, match="Stokes rows"):
        vsm.CoreRT.rt_run(_pm(vsm, arch, "I", 9, (H.SolarBeam(), H.SurfaceSIF(np.ones((3, S))))))
    with pytest.raises(vsm.VSMError, match="spectral points"):
        H.SurfaceSIF(np.ones(S), np.ones((2, S + 1)))
    with pytest.raises(vsm.VSMError, match="dimensions"):
        H.SurfaceSIF(np.ones((1, 1, S)))
    with pytest.raises(vsm.VSMError, match="dimensions"):
        H.SurfaceSIF(np.ones(S), np.ones(S))
    with pytest.raises(vsm.VSMError, match="Stokes rows"):
        CL.SceneLin(_pm(vsm, arch, "I", 9, (H.SolarBeam(), H.SurfaceSIF(sif0(), np.ones((1, 3, S))))), hl, 0, 2, 1)


def test_model_without_the_source_allocates_and_launches_nothing_new(vsm, arch):
    """No SurfaceSIF (and an all-zero table): no table on the device, no SIF slot, neither new entry point is called, and the
    linearized run (lanes = 1, fold = False) gives the bits of the run without the question."""
    H = vsm.host_model
    _, ga, gb = _arrays()
    hl = H.LinModel([ga, gb])
    outs = []
    for src in (None, (H.SolarBeam(), H.SurfaceSIF(np.zeros(S)))):
        scene = vsm.CoreRTLin.SceneLin(_pm(vsm, arch, "IQU", 9, src), hl, 0, 2, 1)
        calls = []
        orig = vsm._lib.call
        try:
            vsm._lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
            outs.append([t.clone() for t in scene.run(lanes=1, fold=False)])
            fwd = vsm.CoreRT.Scene(_pm(vsm, arch, "IQU", 9, src))
            fwd.run()
        finally:
            vsm._lib.call = orig
        torch.cuda.synchronize()
        assert "vsm_surface_sif" not in calls and "vsm_surface_emission_response" not in calls
        assert scene.fwd.sif is None and fwd.sif is None and scene.nSIF == 0 and scene.sif_dot2 is None
        assert all("sif_up" not in w for w in scene._lanes)
        assert outs[-1][2].shape[0] == 3
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    Ro, To, Rdo, Tdo = OL.rt_run_lin(_om("IQU", 9), OL.LinModel([ga, gb]))
    R, T, Rd, Td = scene.results_host()
    assert _rel(R, Ro) < 1e-9 and _rel(Rd, Rdo) < 1e-8
