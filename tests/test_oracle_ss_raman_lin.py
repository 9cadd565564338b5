"""CPU tests that pin tests/ss_raman_lin_oracle.py (the linearized single-scattering run with rotational Raman scattering, our own
restatement: the reference has no linearized Raman driver) independently of the device.  Its forward part is
ss_oracle.rt_run_ss_rrs exactly and its elastic derivatives are ss_lin_oracle.rt_run_ss_lin's; the inelastic derivatives are
checked slot by slot, in FP64, against central finite differences of ss_oracle.rt_run_ss_rrs at the step sizes of
test_oracle_ss_lin.py (gas slots h = 1e-3, aerosol slots h = 2e-3) and at h / 2.

Bounds, as in test_oracle_ss_lin.py: the FD error is the order-2 truncation term, so it must fall by about 4 from h to h / 2
(bound 0.3 on the ratio), and the difference at h / 2 relative to the array maximum, measured per slot (MEASURED below, DESIGN.md
section 4.9c; worse of ieR and ieT), is gated at ten times its own measured value: one decade.

The close-branch scenes.  Two spectral points with the same tau and different gas derivatives (two gases split differently at equal
Rayleigh) sit in the forward kernel's `|d0 - d1| <= 1e-8` branch on the SZA row of every line that couples them; a point whose
tau is mu_i / mu_0 times its donor's sits in the `|mu_i / mu_0 - d1 / d0| < 1e-8` branch at that view.  The central differences
step out of the branch (the function is continuous), and the oracle agrees with them at the gate of the gas slot measured on the
regular scene; the variant that differentiates the close value as written (as a function of d0 alone) misses it by more than four
decades (NAIVE below), so the cases have teeth.

The default fscatt_dot formula against central differences of OR.default_fscatt: fscatt is a rational function of the parameter
(tau_scatt is a cubic along the scene's linear directions), the quotient's truncation term measured at h / 2 = 1e-3 per slot
(FSCATT_MEASURED), gated at ten times that; the gas slots are exact zeros."""
import numpy as np
import pytest

import ss_oracle as SS
import ss_raman_lin_oracle as SRL
import test_oracle_ss_lin as TL
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL
from oracle import vsm_oracle_raman as OR

SHIFTS = np.array([-2, -1, 0, 1, 3, 40])          # 40: never in band
W_IE = np.array([0.012, 0.02, 0.009, 0.018, 0.007, 0.3])
# measured differences at h / 2 (worse of ieR and ieT, relative to the array maximum); gas slots h = 1e-3, aerosol slots h = 2e-3
# (the ratio was 0.250 in every slot)
MEASURED = {"gas a": 2.84e-8, "gas b": 5.23e-9, "aerosol tau_ref (tau, fscatt)": 1.73e-4, "aerosol n_i (ssa, f_trunc only)": 7.97e-9,
            "aerosol r_m (tau, fscatt)": 1.02e-6}
# the close scenes' gas slot: 3.68e-9 at h / 2 in both, held to the regular scene's "gas a" gate; differentiated as written the
# close value misses by 1.72e-2 (equal tau) and 1.49e-2 (tau ratio = mu ratio): lower bounds a decade below
NAIVE = {"equal tau": 1e-3, "tau ratio = mu ratio": 1e-3}
# default_fscatt_dot against central differences of default_fscatt at h = 1e-3 (slot: figure; ratio 0.250 in every slot)
FSCATT_MEASURED = {0: 1.96e-4, 2: 9.13e-9, 3: 2.11e-6, 5: 4.76e-5}
MARGIN = 10.0
RATIO = 0.3


def _rs(shifts=SHIFTS, w_ie=W_IE):
    return OR.RRS(i_shift=np.asarray(shifts), varpi_ie=np.asarray(w_ie), greek_raman=O.get_greek_rayleigh(6.0 / 7.0 * 0.5))


def gas_scene(**kw):
    """test_oracle_ss_lin.gas_scene with Rayleigh scattering in every layer (fscatt = 1 throughout) and six points."""
    kw.setdefault("S", 6)
    return TL.gas_scene(zero_layer=None, **kw)


_TAU_AER0 = None


def aerosol_scene(x=None):
    """test_oracle_ss_lin.aerosol_scene with tau_aer_dot of the n_i slot zeroed: that slot moves ssa, f_trunc and the phase
    function only (fscatt moves through 1 - f_trunc ssa, tau_aer stays)."""
    global _TAU_AER0
    om, lin = TL.aerosol_scene(x=x)
    if _TAU_AER0 is None:
        _TAU_AER0 = TL.aerosol_scene()[0].tau_aer.copy()
    tad = lin.tau_aer_dot.copy()
    tad[0, 2, :] = 0.0
    xx = np.zeros(7) if x is None else np.asarray(x, dtype=float)
    om.tau_aer = _TAU_AER0 + np.einsum("k,akl->al", xx, tad)
    return om, OL.LinModel(lin.tau_abs_dot, tau_aer_dot=tad, lin_aerosol_optics=lin.lin_aerosol_optics)


def _ie(res):
    return res[2], res[3]


def fd_figures(an, run, h):
    out = []
    for step in (h, h / 2):
        up, dn = _ie(run(step)), _ie(run(-step))
        out.append(max(TL._rel(a, (u - d) / (2 * step)) for a, u, d in zip(an, up, dn)))
    return tuple(out)


def _check(name, an, run, h, gate=None):
    assert np.max(np.abs(an[0])) > 0 and np.max(np.abs(an[1])) > 0, name
    d1, d2 = fd_figures(an, run, h)
    print("%s: FD difference %.3e at h = %g, %.3e at h / 2 (ratio %.3f)" % (name, d1, h, d2, d2 / d1))
    assert d2 <= MARGIN * (MEASURED[name] if gate is None else gate), (name, d2)
    assert d2 <= RATIO * d1, (name, d1, d2)
    return d2


def test_forward_and_elastic_parts_are_the_existing_oracles_exactly():
    import ss_lin_oracle as SSL
    rs = _rs()
    for om, lin in (gas_scene(), aerosol_scene()):
        res = SRL.rt_run_ss_rrs_lin(om, lin, rs)
        fwd, el = SS.rt_run_ss_rrs(om, rs), SSL.rt_run_ss_lin(om, lin)
        assert all(np.array_equal(a, b) for a, b in zip(res[:4], fwd[:4]))
        assert np.array_equal(res[4], el[2]) and np.array_equal(res[5], el[3])
        assert res[6].shape == res[0].shape + (lin.n_layer_params + 1,) and res[7].shape == res[6].shape


def test_gas_and_albedo_slots_match_finite_differences():
    rs = _rs()
    om, lin = gas_scene()
    res = SRL.rt_run_ss_rrs_lin(om, lin, rs)
    ieRd, ieTd = res[6], res[7]
    h = 1e-3
    _check("gas a", (ieRd[..., 0], ieTd[..., 0]), lambda e: SS.rt_run_ss_rrs(gas_scene(scale=(1 + e, 1.0))[0], rs), h)
    _check("gas b", (ieRd[..., 1], ieTd[..., 1]), lambda e: SS.rt_run_ss_rrs(gas_scene(scale=(1.0, 1 + e))[0], rs), h)
    # the surface has no inelastic single-scattering part: the albedo slot is identically zero, and the forward does not move
    assert np.all(ieRd[..., 2] == 0) and np.all(ieTd[..., 2] == 0)
    up, dn = SS.rt_run_ss_rrs(gas_scene(albedo=0.3 + h)[0], rs), SS.rt_run_ss_rrs(gas_scene(albedo=0.3 - h)[0], rs)
    assert np.array_equal(up[2], dn[2]) and np.array_equal(up[3], dn[3]) and not np.array_equal(up[0], dn[0])


@pytest.mark.parametrize("k,name", [(0, "tau_ref (tau, fscatt)"), (2, "n_i (ssa, f_trunc only)"), (3, "r_m (tau, fscatt)")])
def test_aerosol_slots_match_finite_differences(k, name):
    rs = _rs([-1, 0, 1], [0.02, 0.009, 0.018])
    om, lin = aerosol_scene()
    res = SRL.rt_run_ss_rrs_lin(om, lin, rs)
    assert res[6].shape[-1] == 9
    if k == 2:       # the slot's tau_aer stays; fscatt moves all the same
        assert np.all(lin.tau_aer_dot[0, 2] == 0) and np.max(np.abs(SRL.default_fscatt_dot(om, lin)[2])) > 0

    def run(e):
        x = np.zeros(7)
        x[k] = e
        return SS.rt_run_ss_rrs(aerosol_scene(x=x)[0], rs)
    _check("aerosol " + name, (res[6][..., k], res[7][..., k]), run, 2e-3)
    assert np.all(res[6][..., 8] == 0) and np.all(res[7][..., 8] == 0)


def test_fscatt_dot_matters():
    """Without fscatt_dot the aerosol optical-depth slot misses its central differences by far more than the gate."""
    rs = _rs([-1, 0, 1], [0.02, 0.009, 0.018])
    om, lin = aerosol_scene()
    fs = OR.default_fscatt(om)
    res = SRL.rt_run_ss_rrs_lin(om, lin, rs, fscatt=fs, fscatt_dot=np.zeros((lin.n_layer_params,) + fs.shape))

    def run(e):
        x = np.zeros(7)
        x[0] = e
        return SS.rt_run_ss_rrs(aerosol_scene(x=x)[0], rs)
    d = fd_figures((res[6][..., 0], res[7][..., 0]), run, 2e-3)[1]
    print("aerosol tau_ref without fscatt_dot: FD difference %.3e" % d)
    assert d > 100 * MARGIN * MEASURED["aerosol tau_ref (tau, fscatt)"]      # (measured 1.70: fscatt' is most of this slot)


# ---- the close branches --------------------------------------------------------------------------------------------------------
def equal_tau_scene(scale=(1.0, 1.0), S=4, L=3):
    """Two gases split differently at points 0 and 1 with equal Rayleigh: tau[0] == tau[1] exactly in every layer at scale 1,
    and d tau / d x_a differs between them (0.25 against 0.5 of the same profile)."""
    prof = np.array([0.03125, 0.0625, 0.125])[:L]
    a = np.outer([0.25, 0.5, 0.375, 0.8], prof)[:S]
    b = np.outer([0.5, 0.25, 0.125, 0.3], prof)[:S]
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    om = O.build_model("IQU", 7, TL.SZA, list(TL.VZA), list(TL.VAZ), tau_rayl=tau_rayl, tau_abs=scale[0] * a + scale[1] * b, depol=0.0075,
                       albedo=0.3, m_max=2)
    om.F0 = TL._f0(om.pol.n, S)
    return om, OL.LinModel([a, b])


def mu_ratio_scene(scale=(1.0, 1.0), S=4, L=3, view=0):
    """Point 0's tau is mu_i / mu_0 times point 1's in every layer, formed in FP64, for the view `view` (20 degrees: not the SZA
    row): on the line n0 = n1 + 1 the recipient 0 sits in the |mu_i / mu_0 - d1 / d0| < 1e-8 branch at that view."""
    om0, _ = equal_tau_scene(S=S, L=L)
    qp = om0.quad_points
    mi = qp.qp_mu[int(np.argmin(np.abs(qp.qp_mu - O.cosd(TL.VZA[view]))))]
    ms = qp.qp_mu[qp.imu0]
    assert mi != ms
    prof = np.array([0.03125, 0.0625, 0.125])[:L]
    a = np.outer([0.0, 0.5, 0.375, 0.8], prof)[:S]
    b = np.outer([0.0, 0.25, 0.125, 0.3], prof)[:S]
    tau_rayl = om0.tau_rayl.astype(np.float64)
    target = (tau_rayl[1] + (a[1] + b[1])) * (mi / ms) - tau_rayl[0]      # tau_abs of point 0
    a[0] = 0.3 * target
    b[0] = target - a[0]
    om = O.build_model("IQU", 7, TL.SZA, list(TL.VZA), list(TL.VAZ), tau_rayl=tau_rayl, tau_abs=scale[0] * a + scale[1] * b, depol=0.0075,
                       albedo=0.3, m_max=2)
    om.F0 = TL._f0(om.pol.n, S)
    return om, OL.LinModel([a, b]), float(mi / ms)


def _layer_tau(om):
    lods = O.construct_core_optical_properties(om, 0)
    return np.stack([O.expand_optical_properties(lo, om.FT).tau for lo in lods], axis=1)      # [S, L]


@pytest.mark.parametrize("which", ["equal tau", "tau ratio = mu ratio"])
def test_close_branch_partials_are_the_limits_not_the_value_differentiated(which):
    rs = _rs([-1, 0, 1], [0.02, 0.009, 0.018])
    if which == "equal tau":
        scene = lambda sc=(1.0, 1.0): equal_tau_scene(sc)[:2]
        om, lin = scene()
        tau = _layer_tau(om)
        assert np.array_equal(tau[0], tau[1]) and not np.array_equal(lin.tau_abs_dot[0][0], lin.tau_abs_dot[0][1])
    else:
        scene = lambda sc=(1.0, 1.0): mu_ratio_scene(sc)[:2]
        om, lin, rm = mu_ratio_scene()
        tau = _layer_tau(om)
        assert np.all(np.abs(rm - tau[0] / tau[1]) < SRL.CLOSE) and np.all(np.abs(tau[0] - tau[1]) > 1e-3 * tau[1])
    res = SRL.rt_run_ss_rrs_lin(om, lin, rs)
    naive = SRL.rt_run_ss_rrs_lin(om, lin, rs, naive_close=True)
    h = 1e-3
    run = lambda e: SS.rt_run_ss_rrs(scene((1 + e, 1.0))[0], rs)
    _check(which + " (gas a)", (res[6][..., 0], res[7][..., 0]), run, h, gate=MEASURED["gas a"])
    d_naive = fd_figures((naive[6][..., 0], naive[7][..., 0]), run, h)[1]
    print("%s: the close value differentiated as written misses the central differences by %.3e" % (which, d_naive))
    assert d_naive > NAIVE[which] > 100 * MARGIN * MEASURED["gas a"]
    # the regular pairs do not see the variant: ieR has no close branch at all
    assert np.array_equal(res[6], naive[6])


# ---- fscatt_dot ----------------------------------------------------------------------------------------------------------------
def test_default_fscatt_dot_matches_finite_differences_of_default_fscatt():
    om, lin = aerosol_scene()
    fd_an = SRL.default_fscatt_dot(om, lin)
    assert fd_an.shape == (8,) + om.tau_rayl.shape
    assert np.all(fd_an[7] == 0)                         # the gas slot
    assert np.all(fd_an[:, :, 0] == 0)                   # the aerosol is absent from the top layer
    for k, meas in FSCATT_MEASURED.items():
        figs = []
        for h in (2e-3, 1e-3):
            x = np.zeros(7)
            x[k] = h
            figs.append(TL._rel(fd_an[k], (OR.default_fscatt(aerosol_scene(x=x)[0]) - OR.default_fscatt(aerosol_scene(x=-x)[0])) / (2 * h)))
        print("fscatt_dot slot %d: FD difference %.3e at h = 2e-3, %.3e at h = 1e-3" % (k, figs[0], figs[1]))
        assert np.max(np.abs(fd_an[k])) > 0
        assert figs[1] <= MARGIN * meas and figs[1] <= RATIO * figs[0], (k, figs)
    # a gas does not move fscatt
    om_g, lin_g = gas_scene()
    assert np.all(SRL.default_fscatt_dot(om_g, lin_g) == 0)
    assert np.array_equal(OR.default_fscatt(gas_scene(scale=(1.5, 1.0))[0]), OR.default_fscatt(om_g))
