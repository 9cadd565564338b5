"""GPU tests of the linearized single-scattering run with rotational Raman scattering (vsm.CoreRTRaman.rt_run_ss_lin;
core_rt_ss.SceneSSRamanLin) and its column kernel (vsm_ss_column_rrs_lin_*; csrc/vsm_ss.hip) against tests/ss_raman_lin_oracle.py.

Tolerances are test_gpu_ss_lin.py's own: the kernel on the oracle's inputs 1e-10 (FP64) / 5e-4 (FP32), a whole run 1e-8 / 1e-2, per
parameter slot relative to that slot's array maximum; a slot whose reference is all zero must be exactly zero.  The device finite
differences use the figures test_oracle_ss_raman_lin.py measured on the CPU with the same one-decade margin: the gas slot 2.84e-8
at h / 2 = 5e-4, the aerosol optical-depth slot 1.73e-4 at h / 2 = 1e-3 (both the order-2 truncation term of the quotient).
R1, T1, R1dot, T1dot are CoreRTLin.rt_run_ss's and ieR1, ieT1 CoreRTRaman.rt_run_ss's bit for bit, in every run case."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ss_lin_oracle as SSL  # noqa: E402
import ss_raman_lin_oracle as SRL  # noqa: E402
import test_gpu_ss as TG  # noqa: E402
import test_gpu_ss_lin as TGL  # noqa: E402
import test_oracle_ss_raman_lin as TC  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_raman as OR  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, TOL_RUN = TGL.TOL, TGL.TOL_RUN
FD_TOL_GAS = 10 * TC.MEASURED["gas a"]
FD_TOL_AER = 10 * TC.MEASURED["aerosol tau_ref (tau, fscatt)"]
SHIFTS, W_IE, SHIFTS_BIG, W_IE_BIG = TG.SHIFTS, TG.W_IE, TG.SHIFTS_BIG, TG.W_IE_BIG
_rel, _scene, _check_slots, _rs_pair = TGL._rel, TGL._scene, TGL._check_slots, TG._rs_pair


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


def _check_run(vsm, got, ref, pm, hl, prs, naer, ngas, FT, nonzero=True):
    """The 8-tuple of a run against the oracle's, and the bit-for-bit identities with the two existing drivers."""
    P = 7 * naer + ngas + 1
    nV, n, S = ref[0].shape
    assert len(got) == 8
    for g in got[:4]:
        assert g.shape == (nV, n, S) and g.dtype == FT
    for g in got[4:]:
        assert g.shape == (nV, n, S, P) and g.dtype == FT
    el = vsm.CoreRTLin.rt_run_ss(pm, hl, naer, ngas, 1)
    ie = vsm.CoreRTRaman.rt_run_ss(prs, pm, 1)
    assert np.array_equal(got[0], el[0]) and np.array_equal(got[1], el[1])
    assert np.array_equal(got[4], el[2]) and np.array_equal(got[5], el[3])
    assert np.array_equal(got[2], ie[2]) and np.array_equal(got[3], ie[3])
    for name, g, r in zip(("R1", "T1", "ieR1", "ieT1"), got[:4], ref[:4]):
        if np.max(np.abs(r)) == 0:
            assert np.max(np.abs(g)) == 0, name
        else:
            assert _rel(g, r) <= TOL_RUN[FT], (name, _rel(g, r))
    for name, g, r in zip(("R1dot", "T1dot", "ieR1dot", "ieT1dot"), got[4:], ref[4:]):
        _check_slots(g, r, TOL_RUN[FT], name)
    assert np.all(got[6][..., P - 1] == 0) and np.all(got[7][..., P - 1] == 0)      # the surface has no inelastic part
    if nonzero:
        for p in range(P - 1):
            assert np.max(np.abs(ref[6][..., p])) > 0 and np.max(np.abs(ref[7][..., p])) > 0, p


RUNS = [
    # (id, FT, pol, S, NAer, NGas, L, shifts, w_ie)
    ("scalar_s1_p3", np.float64, "I", 1, 0, 2, 3, SHIFTS, W_IE),                # only shift 0 in band: n0 == n1, close on every pair
    ("iqu_s7_p10", np.float64, "IQU", 7, 1, 2, 3, SHIFTS, W_IE),                # every line partly out of band; P odd to the chunk
    ("iquv_s70_p10", np.float64, "IQUV", 70, 1, 2, 3, SHIFTS, W_IE),            # a partial workgroup, several row groups
    ("iqu_s300_p3_three_workgroups", np.float64, "IQU", 300, 0, 2, 3, SHIFTS_BIG, W_IE_BIG),   # donors across workgroup edges
    ("iqu_s70_p10_fp32", np.float32, "IQU", 70, 1, 2, 3, SHIFTS, W_IE),
    ("scalar_s7_l1_p2", np.float64, "I", 7, 0, 1, 1, SHIFTS, W_IE),             # L = 1: the copy path only
]


@pytest.mark.parametrize("case", RUNS, ids=[c[0] for c in RUNS])
def test_rt_run_ss_rrs_lin_against_oracle(vsm, arch, case):
    _, FT, pol, S, naer, ngas, L, shifts, w_ie = case
    om, ol, pm, hl = _scene(vsm, arch, pol, S, naer, ngas, FT, L=L)
    ors, prs = _rs_pair(vsm, shifts, w_ie)
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors)
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, naer, ngas, 1)
    _check_run(vsm, got, ref, pm, hl, prs, naer, ngas, FT)


def test_layer_without_rayleigh_share(vsm, arch):
    """A layer with fscatt = 0 (stated, with its derivative): no inelastic source there, the interaction goes on."""
    FT, S = np.float64, 24
    om, ol, pm, hl = _scene(vsm, arch, "IQU", S, 0, 2, FT)
    ors, prs = _rs_pair(vsm, SHIFTS, W_IE)
    fs = OR.default_fscatt(om).copy()
    fs[:, 1] = 0.0
    fsd = np.zeros((2, S, 3))
    prs.fscattRayl, prs.fscattRayl_dot = fs, fsd
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors, fscatt=fs, fscatt_dot=fsd)
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 2, 1)
    _check_run(vsm, got, ref, pm, hl, prs, 0, 2, FT)


def test_no_lines_and_no_layer_parameters(vsm, arch):
    """K = 0: all-zero inelastic arrays and derivatives (nothing is launched); NAer = NGas = 0: only the surface slot, zeros."""
    FT = np.float64
    om, ol, pm, hl = _scene(vsm, arch, "IQU", 24, 1, 2, FT)
    ors, prs = _rs_pair(vsm, SHIFTS[:0], W_IE[:0])
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors)
    _check_run(vsm, got, ref, pm, hl, prs, 1, 2, FT, nonzero=False)
    assert all(np.all(g == 0) for g in (got[2], got[3], got[6], got[7])) and np.max(np.abs(got[4])) > 0
    om, ol, pm, hl = _scene(vsm, arch, "IQU", 7, 0, 0, FT)
    ors, prs = _rs_pair(vsm, SHIFTS, W_IE)
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 0, 1)
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors)
    _check_run(vsm, got, ref, pm, hl, prs, 0, 0, FT, nonzero=False)
    assert got[6].shape[-1] == 1 and np.all(got[6] == 0) and np.all(got[7] == 0) and np.max(np.abs(got[2])) > 0


# ---- the kernel on the oracle's own inputs ---------------------------------------------------------------------------------------
def _kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=None, p_ranges=(None,)):
    """vsm_ss_column_rrs_lin_* for m = 0 .. m_max into the same buffers, every input taken from the oracle."""
    CR, SSd = vsm.CoreRT, vsm.core_rt_ss
    conv = vsm.Architectures.array_type(arch)
    pol, qp = om.pol, om.quad_points
    S, L = om.tau_rayl.shape
    n, nV = pol.n, len(om.vza)
    pl = ol.n_layer_params
    P = pl + 1
    dt = torch.float64 if FT == np.float64 else torch.float32
    dq = CR.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    F0 = conv(np.ascontiguousarray(np.asarray(om.F0, dtype=FT).T))
    Rd = torch.zeros((P, S, n, nV), dtype=dt, device="cuda")
    Td = torch.zeros_like(Rd)
    sp = lambda x: conv(np.ascontiguousarray(np.asarray(x, dtype=FT).T))      # [S, p] -> (p, S)
    fscatt, fsd = OR.default_fscatt(om), SRL.default_fscatt_dot(om, ol)
    sh = torch.tensor(np.asarray(ors.i_shift, dtype=np.int32), dtype=torch.int32, device="cuda")
    hl = int(np.max(np.abs(ors.i_shift))) if halo is None else halo
    for m in range(om.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(om, m)
        lins = SSL.layer_optics_lin(om, ol, lods, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT)
        los = [O.expand_optical_properties(lo, FT) for lo in lods]
        tsd = np.zeros((S, pl, L + 1))
        for iz in range(L):
            tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
        Zp, Zm = O.compute_Z_moments(pol, qp.qp_mu, ors.greek_raman, m)
        row0, w = CR._vza_rows_weights(pm.polarization_type, pm.vza, pm.vaz, pm.quad_points, m, float(weight), dt)
        for pr in p_ranges:
            SSd.ss_column_rrs_lin_(dq, m, P, pl, [conv(lo.tau) for lo in los], [conv(tau_sum_all[:, iz].astype(FT)) for iz in range(L)],
                                   [conv(np.ascontiguousarray(fscatt[:, iz].astype(FT))) for iz in range(L)],
                                   [sp(lins[iz].tau_dot) for iz in range(L)], [sp(tsd[:, :, iz]) for iz in range(L)],
                                   [conv(np.ascontiguousarray(fsd[:, :, iz].astype(FT))) for iz in range(L)], sh,
                                   conv(np.asarray(ors.varpi_ie, dtype=FT)), CR.to_device_matrix(Zp, arch, FT),
                                   CR.to_device_matrix(Zm, arch, FT), F0, hl, row0, w, nV, Rd, Td, p_range=pr)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("vsm_ss_column_rrs_lin")
    host = vsm.Architectures.to_host
    return host(Rd).transpose(3, 2, 1, 0).copy(), host(Td).transpose(3, 2, 1, 0).copy()


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol,S,naer,shifts,w_ie", [("IQU", 70, 1, SHIFTS, W_IE), ("IQUV", 300, 0, SHIFTS_BIG, W_IE_BIG),
                                                    ("I", 1, 0, SHIFTS, W_IE)], ids=["iqu_s70_p10", "iquv_s300_p3", "scalar_s1_p3"])
def test_column_rrs_lin_kernel_accumulates_over_moments(vsm, arch, FT, pol, S, naer, shifts, w_ie):
    om, ol, pm, _ = _scene(vsm, arch, pol, S, naer, 2, FT)
    ors, _ = _rs_pair(vsm, shifts, w_ie)
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors)
    Rd, Td = _kernel_case(vsm, arch, om, ol, pm, ors, FT)
    _check_slots(Rd, ref[6], TOL[FT], "ieRdot (kernel)")
    _check_slots(Td, ref[7], TOL[FT], "ieTdot (kernel)")
    assert np.max(np.abs(ref[6][..., 0])) > 0


def test_halo_and_slot_ranges_do_not_change_results(vsm, arch):
    """Donors staged in LDS and donors read from global memory are the same values (halo = 0 against the largest staged window,
    1e-13); the slots [0, 3) and [3, 10) in two calls equal one call bit for bit (chunk boundaries shifted: 3 is odd)."""
    FT = np.float64
    om, ol, pm, _ = _scene(vsm, arch, "IQU", 300, 1, 2, FT)
    ors, _ = _rs_pair(vsm, SHIFTS_BIG, W_IE_BIG)
    a = _kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=0)
    b = _kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=10 ** 6)     # clamped to VSM_SS_MAX_HALO
    c = _kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=10 ** 6, p_ranges=((0, 3), (3, 10)))
    for x, y, z in zip(a, b, c):
        assert np.max(np.abs(y)) > 0
        for p in range(9):
            assert _rel(x[..., p], y[..., p]) <= 1e-13, p
        assert np.array_equal(y, z)
        assert np.all(y[..., 9] == 0)


def test_shared_pieces_with_two_live_threads_in_the_second_workgroup(vsm, arch):
    """What the four column kernels share (rows, Z F0, donors, LDS window, recipient set-up, output index), FP64, where their
    bookkeeping is thinnest: S = VSM_SS_BLOCK + 2, so the second workgroup has two live threads beside the barriers; IQU with three
    viewing angles, 9 table items in three row groups, the last holding one row; the middle angle is the solar zenith angle, so
    the sun-row branches run; |shift| up to 5 in band, 150 and more out of it; one aerosol (the Z_dot kernel).  One run launches all
    four kernels: its eight arrays against the oracle at the run tolerance; then the derivative kernel with halo = 0 (every donor
    but shift 0's from global memory) against the clamped halo (every donor staged) at the bound of
    test_halo_and_slot_ranges_do_not_change_results."""
    FT, S = np.float64, 130
    om, ol, pm, hl = _scene(vsm, arch, "IQU", S, 1, 2, FT)
    qp = om.quad_points
    mu = np.asarray(qp.qp_mu)
    assert [int(np.argmin(np.abs(mu - O.cosd(v)))) for v in TGL.VZA][1] == int(qp.imu0)
    ors, prs = _rs_pair(vsm, SHIFTS_BIG, W_IE_BIG)
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors)
    assert all(np.max(np.abs(r)) > 0 for r in ref)
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    _check_run(vsm, got, ref, pm, hl, prs, 1, 2, FT)
    a = _kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=0)
    b = _kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=10 ** 6)     # clamped to VSM_SS_MAX_HALO
    for x, y in zip(a, b):
        for p in range(9):
            assert np.max(np.abs(y[..., p])) > 0 and _rel(x[..., p], y[..., p]) <= 1e-13, p
        assert np.all(x[..., 9] == 0) and np.all(y[..., 9] == 0)


# ---- the close branches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["equal tau", "tau ratio = mu ratio"])
def test_close_branch_scenes_against_oracle(vsm, arch, which):
    """The scenes of test_oracle_ss_raman_lin.py on the device: every coupled pair of points 0 and 1 sits in a close branch of the
    forward kernel and has different gas derivatives on its two sides.  (The as-written derivative misses these by 1.5e-2.)"""
    H = vsm.host_model
    om, ol = (TC.equal_tau_scene() if which == "equal tau" else TC.mu_ratio_scene())[:2]
    pm = H.model_from_arrays(arch, "IQU", 7, TC.TL.SZA, list(TC.TL.VZA), list(TC.TL.VAZ), tau_rayl=om.tau_rayl, tau_abs=om.tau_abs,
                             depol=0.0075, albedo=0.3, m_max=2)
    om.varpi_cabannes = pm.varpi_Cabannes = 0.96
    pm.F0 = om.F0
    hl = H.LinModel([np.asarray(g) for g in ol.tau_abs_dot])
    ors, prs = _rs_pair(vsm, np.array([-1, 0, 1]), np.array([0.02, 0.009, 0.018]))
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors)
    naive = SRL.rt_run_ss_rrs_lin(om, ol, ors, naive_close=True)
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 2, 1)
    _check_run(vsm, got, ref, pm, hl, prs, 0, 2, np.float64)
    assert _rel(naive[7][..., 0], ref[7][..., 0]) > 1e-3


# ---- device finite differences ---------------------------------------------------------------------------------------------------
def test_device_finite_difference_gas_and_aerosol_optical_depth(vsm, arch):
    """The vsm_layer_optics_lin -> fscatt_dot -> kernel chain, FP64: a gas slot and the aerosol optical-depth slot (tau and fscatt
    move) against central differences of two CoreRTRaman.rt_run_ss calls each."""
    ors, prs = _rs_pair(vsm, SHIFTS, W_IE)
    mk = lambda **kw: _scene(vsm, arch, "IQU", 70, 1, 2, **kw)
    om, ol, pm, hl = mk()
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    h = 5e-4
    up, dn = vsm.CoreRTRaman.rt_run_ss(prs, mk(scale=1 + h)[2], 1), vsm.CoreRTRaman.rt_run_ss(prs, mk(scale=1 - h)[2], 1)
    for name, an, k in (("ieRdot gas", got[6][..., 7], 2), ("ieTdot gas", got[7][..., 7], 3)):
        e = _rel(an, (up[k] - dn[k]) / (2 * h))
        print("%s: device FD difference %.3e" % (name, e))
        assert np.max(np.abs(an)) > 0 and e <= FD_TOL_GAS, (name, e)

    def moved(e):
        pmx = mk()[2]
        pmx.tau_aer = np.asarray(pmx.tau_aer, dtype=np.float64) + e * np.asarray(hl.tau_aer_dot)[:, 0, :]
        return vsm.CoreRTRaman.rt_run_ss(prs, pmx, 1)
    h = 1e-3
    up, dn = moved(h), moved(-h)
    for name, an, k in (("ieRdot aerosol tau_ref", got[6][..., 0], 2), ("ieTdot aerosol tau_ref", got[7][..., 0], 3)):
        e = _rel(an, (up[k] - dn[k]) / (2 * h))
        print("%s: device FD difference %.3e" % (name, e))
        assert np.max(np.abs(an)) > 0 and e <= FD_TOL_AER, (name, e)


# ---- fscattRayl ------------------------------------------------------------------------------------------------------------------
def test_stated_fscatt_needs_its_derivative(vsm, arch):
    FT, S = np.float64, 24
    om, ol, pm, hl = _scene(vsm, arch, "IQU", S, 1, 2, FT)
    ors, prs = _rs_pair(vsm, SHIFTS, W_IE)
    rng = np.random.default_rng(2)
    fs = rng.uniform(0.3, 1.0, (S, 3))
    fsd = rng.uniform(-0.5, 0.5, (9, S, 3))
    prs.fscattRayl = fs
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    prs.fscattRayl_dot = fsd[:, :, :2]
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    prs.fscattRayl_dot = fsd
    ref = SRL.rt_run_ss_rrs_lin(om, ol, ors, fscatt=fs, fscatt_dot=fsd)
    got = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    _check_run(vsm, got, ref, pm, hl, prs, 1, 2, FT)
    # the gas slots see the stated derivative (the default's is zero there)
    prs.fscattRayl_dot = np.zeros_like(fsd)
    other = vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 1, 2, 1)
    assert _rel(other[6][..., 7], got[6][..., 7]) > 1e-3


def test_refusals(vsm, arch):
    H = vsm.host_model
    om, ol, pm, hl = _scene(vsm, arch, "I", 4, 0, 2)
    ors, prs = _rs_pair(vsm, SHIFTS, W_IE)
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 2, 1, iBand=2)
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 2, 0)
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 1, 1)
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=np.full((3, 4), 0.1)))
    with pytest.raises(NotImplementedError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm, hl, 0, 2, 1)
    pm.sources = None
    g = H.GreekCoefs(**vars(O.hg_greek(0.6, 7)))
    kw = dict(tau_rayl=om.tau_rayl, tau_abs=om.tau_abs, tau_aer=np.full((4, 3), 0.05), aerosol_optics=[H.AerosolOptics(g, 0.9, 0.0)] * 4)
    pm4 = H.model_from_arrays(arch, "I", 7, TGL.SZA, list(TGL.VZA), list(TGL.VAZ), **kw)
    lao = H.LinAerosolOptics([g] * 4, np.zeros(4), np.zeros(4))
    hl4 = H.LinModel(hl.tau_abs_dot, tau_aer_dot=np.zeros((4, 7, 3)), lin_aerosol_optics=[lao] * 4)
    with pytest.raises(NotImplementedError):
        vsm.CoreRTRaman.rt_run_ss_lin(prs, pm4, hl4, 4, 2, 1)


def test_invalid_arguments_before_any_launch(vsm, arch):
    """K < 0, L < 1, null tables, an empty or outlying slot range and p_layer > P return VSM_ERR_INVALID_ARG; nothing launches."""
    lib = vsm._lib.lib()
    om, ol, pm, hl = _scene(vsm, arch, "I", 4, 0, 2)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, np.float64)
    q = dq.cstruct()
    t = torch.zeros(4096, dtype=torch.float64, device="cuda")
    sh = torch.zeros(1, dtype=torch.int32, device="cuda")
    p, ps = C.c_void_p(t.data_ptr()), C.c_void_p(sh.data_ptr())
    tab = (C.c_void_p * 1)(t.data_ptr())
    w = (C.c_double * 1)(1.0)

    def call(K=1, P=3, L=1, p_layer=2, p_lo=0, p_hi=3, tau_tab=tab, dot_tab=tab, row=0):
        return lib.vsm_ss_column_rrs_lin_f64(C.byref(q), 4, L, 0, K, P, p_layer, p_lo, p_hi, tau_tab, tab, tab, dot_tab, tab, tab, ps, p,
                                             p, p, p, 0, 1, (C.c_int * 1)(row), w, p, p, None)
    assert call(K=-1) == 1 and call(P=0, p_layer=0, p_hi=0) == 1 and call(L=0) == 1
    assert call(tau_tab=None) == 1 and call(dot_tab=None) == 1
    assert call(p_lo=2, p_hi=2) == 1 and call(p_lo=2, p_hi=1) == 1 and call(p_lo=-1) == 1 and call(p_hi=4) == 1
    assert call(p_layer=4) == 1 and call(p_layer=-1) == 1
    assert call(row=dq.N if hasattr(dq, "N") else q.N) == 1 and call(row=-1) == 1
    assert lib.vsm_last_error()
    torch.cuda.synchronize()
    vsm._lib.check_device_status("invalid arguments")
    assert float(t.abs().max()) == 0
    assert call(K=0) == 0 and call(p_layer=0, dot_tab=None) == 0 and call(p_lo=2) == 0     # legal, and nothing to launch
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0


def test_footprint_has_no_line_axis_and_no_operator_stack(vsm, arch):
    """IQU, 7 streams, S = 300, K = 12, P = 3: what the scene holds on top of the linearized elastic scene (SceneSSLin, measured
    here) is the Raman tables of SceneSS (fscatt [S] per layer, the Raman Z moments, the line tables), fscatt_dot [p_layer, S] per
    layer, the two inelastic outputs and their derivatives, and the temporaries of the fscatt_dot expression (none here: no
    aerosol) -- less than one [N, S, K] array and far less than P N^2 S."""
    FT = np.float64
    om, ol, pm, hl = _scene(vsm, arch, "IQU", 300, 0, 2, FT)
    _, prs = _rs_pair(vsm, SHIFTS_BIG, W_IE_BIG)
    S, L = om.tau_rayl.shape
    N, n, nV, K, M, P, pl = om.quad_points.Nquad * 3, 3, len(om.vza), len(SHIFTS_BIG), om.m_max + 1, 3, 2

    def peak(make):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        scene = make()
        scene.run()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, scene
    p_lin, _ = peak(lambda: vsm.core_rt_ss.SceneSSLin(pm, hl, 0, 2, 1))
    p_rrs, scene = peak(lambda: vsm.core_rt_ss.SceneSSRamanLin(prs, pm, hl, 0, 2, 1))
    added = L * S + L * pl * S + 2 * M * N * N + 2 * K + 6 * M * N + 2 * n * nV * S + 2 * P * n * nV * S
    bound = 8 * added + 30 * 512
    print("peak %d bytes (elastic linearized scene %d), allowance %d, one [N,S,K] array %d, P N^2 S %d"
          % (p_rrs, p_lin, bound, 8 * N * S * K, 8 * P * N * N * S))
    assert bound < 8 * N * S * K and bound < 8 * P * N * N * S
    assert p_rrs - p_lin < bound
    assert float(scene.ieRd.abs().max()) > 0
