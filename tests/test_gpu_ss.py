"""GPU tests of the single-scattering runs (vsm.CoreRT.rt_run_ss, vsm.CoreRTRaman.rt_run_ss; core_rt_ss.py) and their column
kernels (vsm_ss_column_*, vsm_ss_column_rrs_*; csrc/vsm_ss.hip) against tests/ss_oracle.py.

Tolerances (the project's own, test_gpu_raman.py): the kernels on the oracle's inputs 1e-10 (FP64) / 5e-4 (FP32) relative to the
array maximum; the 6-tuple of a full run 1e-8 / 1e-2.  The inputs keep |dtau[n0] - dtau[n1]| exactly 0 or >= 1e-2 dtau (absorption
drawn from a 32-level grid), so that no (recipient, donor) pair sits at the 1e-8 switch of get_elem_rt_SFI_RRS!'s near / far branches
(test_oracle_ss.py checks on the CPU that the oracle does not move there)."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ss_oracle as SS  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_raman as OR  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 5e-4}
TOL_RUN = {np.float64: 1e-8, np.float32: 1e-2}
SHIFTS = np.array([-5, -2, -1, 1, 3, 40, 0])      # SHIFTS / W_IE of test_gpu_raman.py (40: never in band for S <= 40)
W_IE = np.array([0.004, 0.012, 0.02, 0.018, 0.007, 0.3, 0.009])
# two workgroups and more of the Raman kernel (128 points each): |shift| beyond a block (150: inside the largest staged halo,
# 200: beyond it, read from global memory), shifts that cross a block boundary in both directions, 400: never in band at S = 300
SHIFTS_BIG = np.array([-200, -150, -5, -2, -1, 0, 1, 3, 5, 150, 200, 400])
W_IE_BIG = np.array([0.01, 0.02, 0.004, 0.012, 0.02, 0.009, 0.018, 0.007, 0.005, 0.015, 0.011, 0.3])
SZA, VZA, VAZ = 35.0, [20.0, 35.0, 50.0, 20.0], [0.0, 60.0, 120.0, 0.0]    # the SZA itself and a repeated angle among the VZAs


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _aer(M):
    gk = (lambda g: M.GreekCoefs(**vars(g))) if M is not O else (lambda g: g)
    return [M.AerosolOptics(gk(O.hg_greek(0.7, 10)), 0.95, 0.1), M.AerosolOptics(gk(O.hg_greek(0.5, 6)), 0.9, 0.0)]


def _models(vsm, arch, pol, l_trunc, S, L, FT, albedo=0.3, vza=VZA, vaz=VAZ, surface=None, aerosols=False, zero_layer=None,
            m_max=2, seed=11):
    pn = O.polarization(pol).n
    tau_rayl, tau_abs, F0 = SS.ss_arrays(pn, S, L, seed, zero_layer)
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=albedo, m_max=m_max)
    if aerosols:
        tau_aer = np.zeros((2, L))
        tau_aer[0, L // 3:L // 2 + 1] = 0.1
        tau_aer[1, L // 2:] = 0.05
        kw["tau_aer"] = tau_aer
    H = vsm.host_model
    om = O.build_model(pol, l_trunc, SZA, list(vza), list(vaz), FT=FT, aerosols=_aer(O) if aerosols else (), **kw)
    pm = H.model_from_arrays(arch, pol, l_trunc, SZA, list(vza), list(vaz), float_type=FT, surface=surface,
                             aerosol_optics=_aer(H) if aerosols else (), **kw)
    om.varpi_cabannes = pm.varpi_Cabannes = 0.96
    om.F0, pm.F0 = F0, F0
    return om, pm


def _rs_pair(vsm, shifts, w_ie):
    graman = O.get_greek_rayleigh(6.0 / 7.0 * 0.5)
    return (OR.RRS(i_shift=shifts, varpi_ie=w_ie, greek_raman=graman),
            vsm.CoreRTRaman.RRS(shifts, w_ie, vsm.host_model.GreekCoefs(**vars(graman))))


def _check_tuple(got, ref, nV, n, S, FT, tol, names=("R", "T", "ieR", "ieT", "hem_R", "hem_T")):
    assert len(got) == 6
    for g in got[:4]:
        assert g.shape == (nV, n, S) and g.dtype == FT
    for g in got[4:]:
        assert g.shape == (S,) and g.dtype == FT
    for name, g, r in zip(names, got, ref):
        if np.max(np.abs(r)) == 0:
            assert np.max(np.abs(g)) == 0, name
        else:
            e = _rel(g, r)
            print("%s: rel err %.2e" % (name, e))
            assert e <= tol, (name, e)


ELASTIC = [
    # (id, FT, pol, l_trunc, S, L, albedo, vza, vaz)
    ("scalar_s1_l1_one_row", np.float64, "I", 7, 1, 1, 0.0, [50.0], [30.0]),        # L = 1: the copy path only; one row < row budget
    ("iqu_s7", np.float64, "IQU", 7, 7, 3, 0.3, VZA, VAZ),
    ("iquv_s70", np.float64, "IQUV", 5, 70, 3, 0.3, VZA, VAZ),
    ("iqu_s300_albedo0", np.float64, "IQU", 9, 300, 3, 0.0, VZA, VAZ),
    ("iqu_s70_fp32", np.float32, "IQU", 7, 70, 3, 0.3, VZA, VAZ),
]


@pytest.mark.parametrize("case", ELASTIC, ids=[c[0] for c in ELASTIC])
def test_rt_run_ss_elastic(vsm, arch, case):
    """vsm.CoreRT.rt_run_ss against the oracle: the 6-tuple, its shapes and types; the inelastic arrays are zero."""
    _, FT, pol, lt, S, L, alb, vza, vaz = case
    om, pm = _models(vsm, arch, pol, lt, S, L, FT, albedo=alb, vza=vza, vaz=vaz)
    ref = SS.rt_run_ss(om)
    got = vsm.CoreRT.rt_run_ss(pm)
    _check_tuple(got, ref, len(vza), om.pol.n, S, FT, TOL_RUN[FT])
    assert np.max(np.abs(ref[0])) > 0 and np.max(np.abs(ref[5])) > 0


RAMAN = [
    # (id, FT, pol, l_trunc, S, L, albedo, shifts, w_ie, zero_layer)
    ("scalar_s1_l1", np.float64, "I", 7, 1, 1, 0.0, SHIFTS, W_IE, None),            # only shift 0 is in band
    ("iqu_s7", np.float64, "IQU", 7, 7, 3, 0.3, SHIFTS, W_IE, None),
    ("iquv_s70", np.float64, "IQUV", 5, 70, 3, 0.3, SHIFTS, W_IE, None),
    ("iqu_s300_three_workgroups", np.float64, "IQU", 7, 300, 3, 0.0, SHIFTS_BIG, W_IE_BIG, None),
    ("iqu_s70_fp32", np.float32, "IQU", 7, 70, 3, 0.3, SHIFTS, W_IE, None),
    ("iqu_s24_varpi0_layer", np.float64, "IQU", 7, 24, 3, 0.3, SHIFTS, W_IE, 1),
    ("iqu_s24_no_lines", np.float64, "IQU", 7, 24, 3, 0.3, SHIFTS[:0], W_IE[:0], None),
]


@pytest.mark.parametrize("case", RAMAN, ids=[c[0] for c in RAMAN])
def test_rt_run_ss_rrs(vsm, arch, case):
    """vsm.CoreRTRaman.rt_run_ss against the oracle."""
    _, FT, pol, lt, S, L, alb, shifts, w_ie, zl = case
    om, pm = _models(vsm, arch, pol, lt, S, L, FT, albedo=alb, zero_layer=zl)
    ors, prs = _rs_pair(vsm, shifts, w_ie)
    fs = None
    if zl is not None:     # fScattRayleigh of a layer without Rayleigh scattering is 0, not 0 / 0
        with np.errstate(invalid="ignore"):
            fs = np.nan_to_num(OR.default_fscatt(om))
        prs.fscattRayl = fs
    ref = SS.rt_run_ss_rrs(om, ors, fscatt=fs)
    got = vsm.CoreRTRaman.rt_run_ss(prs, pm, 1)
    _check_tuple(got, ref, len(VZA), om.pol.n, S, FT, TOL_RUN[FT])
    if len(shifts):
        assert np.max(np.abs(ref[2])) > 1e-6 and np.max(np.abs(ref[3])) > 1e-6
    else:
        assert np.max(np.abs(got[2])) == 0 and np.max(np.abs(got[3])) == 0


def test_rt_run_ss_coxmunk(vsm, arch):
    """A Cox-Munk surface: the existing builder's j0- goes into the column (no single-scattering correction, rt_run.jl:724-732)."""
    FT = np.float64
    hs = vsm.host_model.CoxMunkSurface(wind_speed=5.0)
    om, pm = _models(vsm, arch, "IQU", 9, 7, 3, FT, surface=hs, m_max=3)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    # the device's Fourier reflectance blocks (test_gpu_coxmunk.py pins them to the oracle's): the column is under test here
    refl = lambda m: vsm.Architectures.to_host(vsm.CoreRT.reflectance(hs, dq, m, arch, FT)[0]).T.copy()
    surf = lambda m, a, ts: CM.create_surface_layer_brdf(refl(m), a, m, om.pol, om.quad_points, ts, FT)
    ref = SS.rt_run_ss(om, surface=surf)
    got = vsm.CoreRT.rt_run_ss(pm)
    _check_tuple(got, ref, len(VZA), 3, 7, FT, TOL_RUN[FT])


def test_rt_run_ss_aerosol_per_point_Z(vsm, arch):
    """Two aerosol types mixed per spectral point: the layers' Z are [N,N,S] (z_stride = N*N)."""
    FT = np.float64
    om, pm = _models(vsm, arch, "IQU", 11, 7, 6, FT, aerosols=True, m_max=4)
    ref = SS.rt_run_ss(om)
    got = vsm.CoreRT.rt_run_ss(pm)
    _check_tuple(got, ref, len(VZA), 3, 7, FT, TOL_RUN[FT])


def test_rt_run_ss_refuses_thermal(vsm, arch):
    H = vsm.host_model
    _, pm = _models(vsm, arch, "I", 7, 4, 2, np.float64)
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=np.full((2, 4), 0.1)))
    with pytest.raises(NotImplementedError):
        vsm.CoreRT.rt_run_ss(pm)
    ors, prs = _rs_pair(vsm, SHIFTS, W_IE)
    with pytest.raises(NotImplementedError):
        vsm.CoreRTRaman.rt_run_ss(prs, pm, 1)


# ---- the kernels on the oracle's own inputs ------------------------------------------------------------------------------------
def _kernel_case(vsm, arch, om, pm, FT, rs=None, halo=None):
    """vsm_ss_column_* (and _rrs_*) for m = 0 .. m_max into the same buffers, every input taken from the oracle."""
    CR, SSd = vsm.CoreRT, vsm.core_rt_ss
    conv = vsm.Architectures.array_type(arch)
    pol, qp = om.pol, om.quad_points
    S, L = om.tau_rayl.shape
    N, n, nV = qp.Nquad * pol.n, pol.n, len(om.vza)
    dt = torch.float64 if FT == np.float64 else torch.float32
    dq = CR.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    F0 = conv(np.ascontiguousarray(np.asarray(om.F0, dtype=FT).T))
    out = [torch.zeros((S, n, nV), dtype=dt, device="cuda") for _ in range(4)]
    J = [torch.zeros((S, N), dtype=dt, device="cuda") for _ in range(2)]
    fscatt = OR.default_fscatt(om)
    for m in range(om.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(om, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT)
        los = [O.expand_optical_properties(lo, FT) for lo in lods]
        tau = [conv(lo.tau) for lo in los]
        varpi = [conv(lo.varpi) for lo in los]
        tsum = [conv(tau_sum_all[:, iz].astype(FT)) for iz in range(L)]
        Zpp = [CR.to_device_matrix(np.asarray(lods[iz].Zpp), arch, FT) for iz in range(L)]
        Zmp = [CR.to_device_matrix(np.asarray(lods[iz].Zmp), arch, FT) for iz in range(L)]
        zs = [0 if z.shape[0] == 1 else N * N for z in Zpp]
        surf = O.make_added_layer(FT, N, S)
        O.create_surface_layer_lambertian(om.albedo, surf, m, pol, qp, tau_sum_all[:, -1], FT)
        row0, w = CR._vza_rows_weights(pm.polarization_type, pm.vza, pm.vaz, pm.quad_points, m, float(weight), dt)
        ts_s = conv(tau_sum_all[:, -1].astype(FT))
        SSd.ss_column_(dq, m, tau, varpi, tsum, Zpp, Zmp, zs, F0, conv(surf.j0_m), conv(surf.j0_p), ts_s, row0, w, nV, out[0], out[1],
                       J[0] if m == 0 else None, J[1] if m == 0 else None)
        if rs is not None:
            Zp, Zm = O.compute_Z_moments(pol, qp.qp_mu, rs.greek_raman, m)
            sh = torch.tensor(np.asarray(rs.i_shift, dtype=np.int32), dtype=torch.int32, device="cuda")
            hl = int(np.max(np.abs(rs.i_shift))) if halo is None else halo
            SSd.ss_column_rrs_(dq, m, tau, tsum, [conv(np.ascontiguousarray(fscatt[:, iz].astype(FT))) for iz in range(L)], sh,
                               conv(np.asarray(rs.varpi_ie, dtype=FT)), CR.to_device_matrix(Zp, arch, FT),
                               CR.to_device_matrix(Zm, arch, FT), F0, hl, row0, w, nV, out[2], out[3])
    torch.cuda.synchronize()
    host = vsm.Architectures.to_host
    return [host(t).transpose(2, 1, 0).copy() for t in out] + [host(t) for t in J]


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol,S,L,shifts,w_ie", [("IQU", 70, 3, SHIFTS, W_IE), ("IQUV", 300, 3, SHIFTS_BIG, W_IE_BIG),
                                                 ("I", 7, 1, SHIFTS, W_IE)], ids=["iqu_s70", "iquv_s300", "scalar_s7_l1"])
def test_column_kernels_accumulate_over_moments(vsm, arch, FT, pol, S, L, shifts, w_ie):
    """The column functions for m = 0, 1, 2 into the same buffers equal the oracle's sums at the operator-level gate; the sources
    at all streams of m = 0 equal the oracle's composite J0-+."""
    om, pm = _models(vsm, arch, pol, 7, S, L, FT)
    ors, _ = _rs_pair(vsm, shifts, w_ie)
    per_m = []
    ref = SS.rt_run_ss_rrs(om, ors, per_m=per_m)
    got = _kernel_case(vsm, arch, om, pm, FT, rs=ors)
    for name, g, r in zip(("R", "T", "ieR", "ieT"), got[:4], ref[:4]):
        e = _rel(g, r)
        print("%s: rel err %.2e" % (name, e))
        assert e <= TOL[FT], (name, e)
    assert _rel(got[4], per_m[0]["J0_m"]) <= TOL[FT] and _rel(got[5], per_m[0]["J0_p"]) <= TOL[FT]


def test_raman_halo_does_not_change_results(vsm, arch):
    """Donors staged in LDS and donors read from global memory are the same values: halo = 0 (every shifted line through global
    memory) against the largest staged window."""
    FT = np.float64
    om, pm = _models(vsm, arch, "IQU", 7, 300, 3, FT)
    ors, _ = _rs_pair(vsm, SHIFTS_BIG, W_IE_BIG)
    a = _kernel_case(vsm, arch, om, pm, FT, rs=ors, halo=0)
    b = _kernel_case(vsm, arch, om, pm, FT, rs=ors, halo=10 ** 6)     # clamped to VSM_SS_MAX_HALO
    for x, y in zip(a[2:4], b[2:4]):
        assert _rel(x, y) <= 1e-13


def test_fused_column_equals_operator_chain(vsm, arch):
    """Composition, FP64: the fused runs equal the chain of the existing device operators -- elemental_ / elemental_inelastic_
    with ndoubl = 0 and dtau = tau, the two interaction_ss statements in torch, postprocessing_vza_ / postprocessing_vza_rs_."""
    FT = np.float64
    CR, RR = vsm.CoreRT, vsm.CoreRTRaman
    om, pm = _models(vsm, arch, "IQU", 7, 24, 3, FT)
    _, prs = _rs_pair(vsm, SHIFTS, W_IE)
    scene = vsm.core_rt_ss.SceneSS(pm, prs)
    fused = [t.clone() for t in scene.run()]
    fwd, drs = scene.fwd, scene.drs
    S, N, K = fwd.S, fwd.N, drs.K
    mu = fwd.dq.mu[None, :]
    out = [torch.zeros_like(t) for t in fused[:4]]
    added, comp = CR.make_added_layer(FT, pm.architecture, (N, N), S), CR.make_composite_layer(FT, pm.architecture, (N, N), S)
    ars, crs = RR.AddedLayerRS(FT, pm.architecture, K, N, S), RR.CompositeLayerRS(FT, pm.architecture, K, N, S)
    shifts = [int(x) for x in SHIFTS]
    for mom in fwd.moments:
        m = mom["m"]
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        drs.Zpp, drs.Zmp = scene.Zie[m]
        for iz, ly in enumerate(mom["layers"]):
            p = ly["props"].materialize()
            drs.fscatt = scene.fscatt[iz]
            RR.elemental_inelastic_(drs, ly["tau_sum"], p.tau, fwd.F0, m, 0, fwd.dq, ars)
            CR.elemental_(fwd.pol, ly["tau_sum"], p.tau, fwd.F0, p, m, 0, fwd.dq, added)
            if iz == 0:
                comp.J0_p.copy_(added.j0_p), comp.J0_m.copy_(added.j0_m)
                crs.ieJ0_p.copy_(ars.ieJ0_p), crs.ieJ0_m.copy_(ars.ieJ0_m)
            else:
                et, es = torch.exp(-p.tau[:, None] / mu), torch.exp(-ly["tau_sum"][:, None] / mu)
                comp.J0_p.copy_(comp.J0_p * et + added.j0_p)
                comp.J0_m.copy_(comp.J0_m + added.j0_m * es)
                for dn, sh in enumerate(shifts):
                    lo, hi = max(0, -sh), min(S, S - sh)
                    if hi > lo:
                        crs.ieJ0_p[dn, lo:hi] = crs.ieJ0_p[dn, lo:hi] * et[lo:hi] + ars.ieJ0_p[dn, lo:hi]
                        crs.ieJ0_m[dn, lo:hi] = crs.ieJ0_m[dn, lo:hi] + ars.ieJ0_m[dn, lo:hi] * es[lo:hi]
        CR.create_surface_layer_(pm.surface, fwd.added_surface, m, fwd.dq, mom["tau_sum_surface"], rho=mom["rho"])
        es = torch.exp(-mom["tau_sum_surface"][:, None] / mu)
        comp.J0_p.copy_(comp.J0_p + fwd.added_surface.j0_p)
        comp.J0_m.copy_(comp.J0_m + fwd.added_surface.j0_m * es)
        RR.postprocessing_vza_rs_(fwd.pol, comp, crs, pm.vza, pm.vaz, fwd.qp, m, float(weight), *out)
    torch.cuda.synchronize()
    for name, f, c in zip(("R", "T", "ieR", "ieT"), fused[:4], out):
        e = _rel(f.cpu().numpy(), c.cpu().numpy())
        print("%s: fused vs chain %.2e" % (name, e))
        assert e <= TOL[FT], (name, e)
    assert float(out[2].abs().max()) > 1e-6


def test_rrs_footprint_has_no_per_line_array(vsm, arch):
    """Peak device allocation of CoreRTRaman.rt_run_ss at N = 20 (nominal), S = 70, K = 7 stays below one [N,S,K] FP64 array on top
    of the run's inputs and outputs: the raw optical depths [S,L] x 2 (FP64), the layer vectors tau / varpi / dtau / tau_sum [S]
    per layer and fscatt, the Z moments of the scatterers and of the Raman lines, F0, the surface layer (4 shared N x N blocks and
    its two [N,S] sources), the outputs [nV,n,S] x 4 and J0-+ [N,S] of m = 0.  Small tensors round up to the allocator's 512-byte
    granule: one granule each for the ~40 tables of the scene."""
    FT = np.float64
    om, pm = _models(vsm, arch, "IQU", 7, 70, 3, FT)
    _, prs = _rs_pair(vsm, SHIFTS, W_IE)
    S, L = om.tau_rayl.shape
    N, n, nV, K, M = om.quad_points.Nquad * 3, 3, len(VZA), len(SHIFTS), om.m_max + 1
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = vsm.CoreRTRaman.rt_run_ss(prs, pm, 1)
    peak = torch.cuda.max_memory_allocated() - base
    elems = (2 * S * L) + (4 * L + 1) * S + L * S + L + 4 * M * N * N + n * S + 4 * N * N + 2 * N * S + 4 * nV * n * S + 2 * N * S
    bound = 8 * elems + 40 * 512 + 8 * N * S * K
    print("peak %d bytes, inputs + outputs %d, one [N,S,K] array %d" % (peak, 8 * elems + 40 * 512, 8 * N * S * K))
    assert peak < bound
    assert np.max(np.abs(got[2])) > 0


def test_invalid_arguments_before_any_launch(vsm, arch):
    """K < 0, L < 1 and null tables return VSM_ERR_INVALID_ARG."""
    FT = np.float64
    lib = vsm._lib.lib()
    om, pm = _models(vsm, arch, "I", 7, 4, 1, FT)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    q = dq.cstruct()
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    tab = (C.c_void_p * 1)(t.data_ptr())
    zs = (C.c_longlong * 1)(0)
    row0, w = (C.c_int * 1)(0), (C.c_double * 1)(1.0)
    ok = lambda L_, tau_tab: lib.vsm_ss_column_f64(C.byref(q), 4, L_, 0, tau_tab, tab, tab, tab, tab, zs, p, p, None, p, 1, row0, w, p, p,
                                                   None, None, None)
    assert ok(0, tab) == 1 and ok(1, None) == 1
    rr = lambda K_, tau_tab: lib.vsm_ss_column_rrs_f64(C.byref(q), 4, 1, 0, K_, tau_tab, tab, tab, p, p, p, p, p, 0, 1, row0, w, p, p, None)
    assert rr(-1, tab) == 1 and rr(1, None) == 1
    assert b"K >= 0" in lib.vsm_last_error() or b"null" in lib.vsm_last_error()
