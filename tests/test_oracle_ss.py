"""CPU tests that pin tests/ss_oracle.py (the statement-order transcription of the reference's rt_run_ss) independently of the
device: the first-order limit of the full drivers, sanity properties, and the distance of the GPU tests' inputs from the 1e-8
switch of the Raman source kernel's near / far branches.

First-order limit.  The epsilon-model keeps every optical depth and scales what scatters: tau_rayl -> eps tau_rayl,
tau_abs -> tau_abs + (1 - eps) tau_rayl, albedo -> eps albedo (and varpi_ie -> eps varpi_ie).  Then L(eps) = R_full(eps) / eps ->
R_ss as eps -> 0, and the Richardson value 2 L(eps) - L(2 eps) leaves a remainder of order eps^2.  Measured (FP64, the models below):
see DESIGN.md section 4.9."""
import dataclasses

import numpy as np
import pytest

import ss_oracle as SS
from oracle import vsm_oracle as O
from oracle import vsm_oracle_raman as OR

SHIFTS = np.array([-5, -2, -1, 1, 3, 40, 0])
W_IE = np.array([0.004, 0.012, 0.02, 0.018, 0.007, 0.3, 0.009])
SZA = 35.0


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _model(pol="IQU", S=6, L=3, vza=(20.0, 50.0), vaz=(0.0, 60.0), albedo=0.3, zero_layer=None, l_trunc=5):
    tau_rayl, tau_abs, F0 = SS.ss_arrays(O.polarization(pol).n, S, L, zero_layer=zero_layer)
    om = O.build_model(pol, l_trunc, SZA, list(vza), list(vaz), tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=albedo,
                       m_max=2)
    om.F0 = F0
    return om


def _eps_model(om, eps):
    return dataclasses.replace(om, tau_rayl=eps * om.tau_rayl, tau_abs=om.tau_abs + (1 - eps) * om.tau_rayl, albedo=eps * om.albedo)


def _rs(w_scale=1.0, shifts=SHIFTS, w_ie=W_IE):
    return OR.RRS(i_shift=shifts, varpi_ie=w_scale * w_ie, greek_raman=O.get_greek_rayleigh(6.0 / 7.0 * 0.5))


@pytest.fixture(scope="module")
def base():
    om = _model()
    return om, SS.rt_run_ss(om)


def _richardson(full_of_eps, eps):
    return 2 * full_of_eps(eps) / eps - full_of_eps(2 * eps) / (2 * eps)


def test_first_order_limit_elastic(base):
    """(a): rt_run(eps-model) / eps -> rt_run_ss(model) for R and for T (VZAs off the SZA row: no direct beam in T_SFI)."""
    om, ss = base
    for k, name in ((0, "R"), (1, "T")):
        full = lambda e: O.rt_run(_eps_model(om, e))[k]
        d1 = _rel(_richardson(full, 1e-3), ss[k])
        d2 = _rel(_richardson(full, 5e-4), ss[k])
        print("%s: Richardson difference %.3e at eps = 1e-3, %.3e at 5e-4 (ratio %.3f)" % (name, d1, d2, d2 / d1))
        assert d1 <= 1e-4, (name, d1)
        assert d2 <= 0.3 * d1, (name, d1, d2)


def test_first_order_limit_raman():
    """(b): rt_run_rrs(eps-model, eps varpi_ie) / eps -> the inelastic arrays of rt_run_ss_rrs(model)."""
    om = _model()
    ss = SS.rt_run_ss_rrs(om, _rs())
    for k, name in ((2, "ieR"), (3, "ieT")):
        full = lambda e: OR.rt_run_rrs(_eps_model(om, e), _rs(e))[k]
        d1 = _rel(_richardson(full, 1e-3), ss[k])
        d2 = _rel(_richardson(full, 5e-4), ss[k])
        print("%s: Richardson difference %.3e at eps = 1e-3, %.3e at 5e-4 (ratio %.3f)" % (name, d1, d2, d2 / d1))
        assert d1 <= 1e-4, (name, d1)
        assert d2 <= 0.3 * d1, (name, d1, d2)


def test_out_of_band_lines_and_no_lines_give_zero():
    om = _model()
    S = om.tau_rayl.shape[0]
    out = SS.rt_run_ss_rrs(om, _rs(shifts=np.array([S, -S, 40]), w_ie=np.array([0.3, 0.2, 0.1])))
    assert np.all(out[2] == 0) and np.all(out[3] == 0)
    none = SS.rt_run_ss_rrs(om, _rs(shifts=SHIFTS[:0], w_ie=W_IE[:0]))
    assert np.all(none[2] == 0) and np.all(none[3] == 0)
    el = SS.rt_run_ss(om)
    for a, b in zip(none, el):
        assert np.array_equal(a, b)
    # an out-of-band line next to in-band ones changes nothing
    a = SS.rt_run_ss_rrs(om, _rs())
    keep = SHIFTS != 40
    b = SS.rt_run_ss_rrs(om, _rs(shifts=SHIFTS[keep], w_ie=W_IE[keep]))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_nonscattering_layer_only_attenuates():
    """A layer with varpi = 0 in the middle: R is that of the column whose middle layer is taken out, the layers below it seen
    through the extra optical depth -- here checked as: its own sources are zero and the run equals the explicit sum."""
    om = _model(zero_layer=1)
    per_m = []
    out = SS.rt_run_ss(om, per_m=per_m)
    FT, pol, qp = om.FT, om.pol, om.quad_points
    mu = qp.qp_muN[None, :]
    for rec in per_m:
        m = rec["m"]
        lods = O.construct_core_optical_properties(om, m)
        _, ts = O.extract_effective_props(lods, FT)
        N, S = len(qp.qp_muN), om.tau_rayl.shape[0]
        Jm = np.zeros((S, N))
        for iz in (0, 2):
            lo = O.expand_optical_properties(lods[iz], FT)
            a = O.make_added_layer(FT, N, S)
            O.elemental(pol, ts[:, iz], lo.tau, om.F0, lo.varpi, lo.Zpp, lo.Zmp, m, 0, qp, a, FT)
            Jm += a.j0_m * np.exp(-ts[:, iz][:, None] / mu)
        surf = O.make_added_layer(FT, N, S)
        O.create_surface_layer_lambertian(om.albedo, surf, m, pol, qp, ts[:, -1], FT)
        Jm += surf.j0_m * np.exp(-ts[:, -1][:, None] / mu)
        assert _rel(rec["J0_m"], Jm) <= 1e-13
    assert np.all(np.isfinite(out[0])) and np.max(np.abs(out[0])) > 0


def test_one_layer_column_is_its_own_sources():
    om = _model(L=1, albedo=0.0)
    per_m = []
    out = SS.rt_run_ss_rrs(om, _rs(), per_m=per_m)
    FT, pol, qp = om.FT, om.pol, om.quad_points
    N, S = len(qp.qp_muN), om.tau_rayl.shape[0]
    R = np.zeros_like(out[0])
    T = np.zeros_like(out[0])
    for rec in per_m:
        m = rec["m"]
        lo = O.expand_optical_properties(O.construct_core_optical_properties(om, m)[0], FT)
        a = O.make_added_layer(FT, N, S)
        O.elemental(pol, np.zeros(S), lo.tau, om.F0, lo.varpi, lo.Zpp, lo.Zmp, m, 0, qp, a, FT)
        surf = O.make_added_layer(FT, N, S)
        O.create_surface_layer_lambertian(0.0, surf, m, pol, qp, lo.tau, FT)
        c = O.CompositeLayer(None, None, None, None, a.j0_p + surf.j0_p, a.j0_m)
        O.postprocessing_vza(pol, c, om.vza, om.vaz, qp, m, rec["weight"], R, T)
    assert _rel(out[0], R) <= 1e-14 and _rel(out[1], T) <= 1e-14


def test_hemispherical_sums_nonnegative_and_ss_below_full(base):
    """hem_R, hem_T >= 0; I_ss <= I_full on Stokes I of the un-scaled model (the reference's test/test_forward_ss.jl)."""
    om, ss = base
    assert np.all(ss[4] >= 0) and np.all(ss[5] >= 0) and np.max(ss[4]) > 0
    R, T = O.rt_run(om)
    assert np.all(ss[0][:, 0, :] <= R[:, 0, :]) and np.all(ss[1][:, 0, :] <= T[:, 0, :])
    assert ss[0].shape == (2, 3, 6) and ss[4].shape == (6,)


def test_inputs_stay_clear_of_the_near_far_switch():
    """The GPU tests' inputs (ss_arrays) keep |dtau[n0] - dtau[n1]| exactly 0 or well above rt_close_tol and mu_i / mu_0 -
    dtau[n1] / dtau[n0] away from it: perturbing every layer's optical depth by one ulp moves the oracle by less than a tenth of the
    FP64 operator gate (1e-10), on both sides of the branches (VZA list with the SZA itself)."""
    om = _model(S=24, vza=(20.0, 35.0, 50.0), vaz=(0.0, 60.0, 120.0))
    a = SS.rt_run_ss_rrs(om, _rs())
    up = dataclasses.replace(om, tau_abs=np.nextafter(om.tau_abs, np.inf))
    b = SS.rt_run_ss_rrs(up, _rs())
    for k in (2, 3):
        assert _rel(b[k], a[k]) < 1e-11, (k, _rel(b[k], a[k]))
    tau = om.tau_rayl + om.tau_abs
    for sh in SHIFTS:
        n0, n1 = OR.get_n0_n1(tau.shape[0], int(sh))
        d = np.abs(tau[n0] - tau[n1])
        assert np.all((d == 0) | (d >= 1e-3 * tau[n1]))
