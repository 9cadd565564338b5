"""CPU tests of tests/mie_lin_oracle.py (the numpy restatement of the reference's linearized NAI-2 Mie path) against central
differences of tests/mie_oracle.py -- the independent forward restatement, never the code under test --, of the identity the device
relies on (d / d n_i = -i d / d n_r), of the deliberate deviation in the weights' derivatives, and of the host part of
vsm.Scattering's linearized call against the oracle's, bit for bit.  No kernel runs here.

Slot order (n_r, n_i, mu, sigma), mu = ln r_m, sigma = ln sigma_g; mu and sigma are differenced at the unperturbed nodes through
mie_oracle's tabulated form.  Step h = 1e-6, bound 1e-6 (ten times the worst deviation measured, DESIGN.md 4.23: the margin is for
the O(h^2) term, which grows with n_max)."""
import functools
import math

import numpy as np
import pytest

import mie_lin_oracle as ML
import mie_oracle as MO

FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)           # r_m, sigma_g, n_r, n_i, wavelength
TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)
CASES = [(FINE_MODE, 0.35, 20), (TEST_AEROSOL, 3.0, 37), (TEST_AEROSOL, 1.0, 16)]
H_STEP = 1e-6
BOUND = 1e-6


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


@functools.lru_cache(maxsize=None)
def _lin(case, weights=ML.compute_wx_lin):
    (r_m, sigma_g, n_r, n_i, lam), r_max, nquad = case
    return ML.compute_aerosol_optical_properties_lin(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad, weights=weights)


@functools.lru_cache(maxsize=None)
def _central_differences(case):
    """[(d greek, d ssa, d k)] per slot from mie_oracle's forward path."""
    (r_m, sigma_g, n_r, n_i, lam), r_max, nquad = case
    base = MO.LogNormal(r_m, sigma_g)
    r_min = max(base.quantile(1e-8), 1e-6 * r_max)
    r, w_r = MO.gauleg_log(nquad, r_min, r_max)

    def run(dn_r=0.0, dn_i=0.0, dmu=0.0, dsigma=0.0):
        sd = MO.LogNormal(math.exp(base.mu + dmu), math.exp(base.sigma + dsigma))
        return MO.compute_aerosol_optical_properties(None, n_r + dn_r, n_i + dn_i, lam, None, None, tabulated=(r, sd.pdf(r) * w_r))

    out = []
    for name in ("dn_r", "dn_i", "dmu", "dsigma"):
        p, m = run(**{name: H_STEP}), run(**{name: -H_STEP})
        out.append(((p.greek - m.greek) / (2 * H_STEP), (p.ssa - m.ssa) / (2 * H_STEP), (p.k - m.k) / (2 * H_STEP)))
    return out


def _deviations(lin, fds):
    """Worst relative deviations over the slots: Greek (per family, relative to the largest entry of the difference), ssa', k'."""
    dg = ds = dk = 0.0
    for s, (g, ssa, k) in enumerate(fds):
        for c in range(6):
            dg = max(dg, float(np.max(np.abs(lin.greek_dot[s, c] - g[c])) / np.max(np.abs(g[c]))))
        ds = max(ds, abs(lin.ssa_dot[s] - ssa) / abs(ssa))
        dk = max(dk, abs(lin.k_dot[s] - k) / abs(k))
    return dg, ds, dk


@pytest.mark.parametrize("case", CASES)
def test_oracle_against_central_differences(case):
    lin = _lin(case)
    fwd = MO.compute_aerosol_optical_properties(MO.LogNormal(*case[0][:2]), case[0][2], case[0][3], case[0][4], case[1], case[2])
    assert np.array_equal(lin.greek, fwd.greek) and (lin.ssa, lin.k, lin.C_sca) == (fwd.ssa, fwd.k, fwd.C_sca)
    dg, ds, dk = _deviations(lin, _central_differences(case))
    print("mie lin oracle vs central differences, r_max %g nquad %d: greek %.2e  ssa' %.2e  k' %.2e" % (case[1], case[2], dg, ds, dk))
    assert dg <= BOUND and ds <= BOUND and dk <= BOUND, (dg, ds, dk)


@pytest.mark.parametrize("case", CASES)
def test_holomorphy_identity(case):
    """a_n' (n_i) = -i a_n' (n_r), b alike: computed separately by the oracle, as by the reference."""
    an, bn, ad, bd = _lin(case).ab
    for d in (ad, bd):
        dev = float(np.max(np.abs(d[1] + 1j * d[0])) / np.max(np.abs(d[0])))
        print("holomorphy r_max %g: %.2e" % (case[1], dev))
        assert dev <= 1e-12, dev


def test_reference_form_of_the_weight_derivatives_misses_by_one_minus_s():
    """r_max = 1, nquad = 16: the distribution's tail is cut, S = sum pdf(r) w_r = 0.948.  The reference's form is S times the
    derivative: it misses the central difference of k by 1 - S in slots 2 and 3; the corrected form meets the bound."""
    case = CASES[2]
    (r_m, sigma_g, _, _, _), r_max, nquad = case
    sd = MO.LogNormal(r_m, sigma_g)
    r, w_r = MO.gauleg_log(nquad, max(sd.quantile(1e-8), 1e-6 * r_max), r_max)
    total = float(np.sum(sd.pdf(r) * w_r))
    assert 0.04 < 1 - total < 0.06
    fds = _central_differences(case)
    ref_form, good = _lin(case, ML.compute_wx_lin_reference_form), _lin(case)
    for s in (2, 3):
        miss = abs(ref_form.k_dot[s] - fds[s][2]) / abs(fds[s][2])
        print("slot %d: reference form misses k' by %.6e, 1 - S = %.6e" % (s, miss, 1 - total))
        assert abs(miss - (1 - total)) <= 1e-6
        assert abs(good.k_dot[s] - fds[s][2]) / abs(fds[s][2]) <= BOUND
    for s in (0, 1):                                    # the refractive-index slots do not read the weights' derivatives
        assert ref_form.k_dot[s] == good.k_dot[s]


def test_one_node_distribution_and_beta0():
    o = ML.monodisperse_lin(8.5, 1.33, 0.0)
    for s in (2, 3):
        assert not np.any(o.greek_dot[s]) and not np.any(o.bulk_f_dot[s]) and o.ssa_dot[s] == 0 and o.k_dot[s] == 0
        assert o.C_sca_dot[s] == 0
    assert np.any(o.greek_dot[0]) and np.any(o.greek_dot[1])
    for lin in (o, _lin(CASES[0]), _lin(CASES[1])):     # beta_0 = 1 whatever the parameters
        assert np.max(np.abs(lin.greek_dot[:, 1, 0])) <= 1e-9, lin.greek_dot[:, 1, 0]


@pytest.mark.parametrize("case", CASES)
def test_host_part_equals_the_oracles_bit_for_bit(vsm, case):
    S = vsm.Scattering
    (r_m, sigma_g, n_r, n_i, lam), r_max, nquad = case
    h, wx_dot, wr_dot = S.mie_lin_host_inputs(S.make_mie_model(S.Aerosol(S.LogNormal(r_m, sigma_g), n_r, n_i), lam, r_max, nquad))
    ref = _lin(case).host
    assert np.array_equal(wx_dot, ref.wx_dot) and np.array_equal(wr_dot, ref.wr_dot)
    assert np.array_equal(h.wx, ref.wx) and np.array_equal(h.wr, ref.wr) and np.array_equal(h.x, ref.x)
    assert abs(np.sum(wx_dot[0])) <= 1e-12 * np.max(np.abs(wx_dot[0]))      # the normalisation holds: sum wx = 1 for every parameter
    # a tabulated distribution: with weights_dot the same numbers, without it exact zeros
    ln = S.LogNormal(r_m, sigma_g)
    r, w_r = S.gauleg_log(nquad, max(ln.quantile(1e-8), 1e-6 * r_max), r_max)
    raw = ln.pdf(r) * w_r
    tab = S.TabulatedSizeDistribution(r, raw, weights_dot=S.lognormal_raw_dot(ln, r, raw))
    _, wx_t, wr_t = S.mie_lin_host_inputs(S.make_mie_model(S.Aerosol(tab, n_r, n_i), lam))
    assert np.array_equal(wx_t, wx_dot) and np.array_equal(wr_t, wr_dot)
    _, wx_0, wr_0 = S.mie_lin_host_inputs(S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution(r, raw), n_r, n_i), lam))
    assert not np.any(wx_0) and not np.any(wr_0) and wx_0.shape == (2, nquad)
    with pytest.raises(vsm.VSMError):
        S.TabulatedSizeDistribution(r, raw, weights_dot=np.zeros((nquad, 2)))


# ---- the edge cases of tests/mie_cases.py: float64 path unchanged, sensitivity of the n_r slot, rounding floor ---------------------------
import types

import mie_cases as MC

GOLDEN_F64, GOLDEN_CASES, SENSITIVITY = MC.GOLDEN_F64, MC.GOLDEN_CASES, MC.SENSITIVITY
perturbations, greek_move = MC.perturbations, MC.greek_move


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_float64_path_is_the_recorded_one_bit_for_bit(name):
    """The default path against what the oracle returned before it took a dtype (tests/golden/mie_oracle_float64.npz)."""
    want = np.load(GOLDEN_F64)
    h = MC.inputs(MC.BY_NAME[name])
    greek, scal, bulk, greek_dot, scal_dot, bulk_dot, _ab = ML.nai2_lin_reference(*MC.lin_args(h))
    for got, key in ((greek, "lin_greek"), (np.array(scal, dtype=np.float64), "lin_scal"), (bulk, "lin_bulk_f"),
                     (greek_dot, "greek_dot"), (scal_dot, "scal_dot"), (bulk_dot, "bulk_f_dot")):
        assert got.dtype == np.float64 and np.array_equal(got, want[name + "/" + key]), key
    assert np.array_equal(greek, want[name + "/greek"]) and np.array_equal(bulk, want[name + "/bulk_f"])
    # stage 3 factored out: the same numbers from the bulk functions and their derivatives alone
    assert np.array_equal(ML.greek_dot_from_bulk(bulk, scal[0], bulk_dot, scal_dot[:, 0], h.mu, h.w_mu), greek_dot)
    wide = ML.nai2_lin_reference(*MC.lin_args(h), dtype=np.longdouble, scales=True)
    assert all(a.dtype == np.longdouble for a in (wide[0], wide[2], wide[3], wide[4], wide[5]))
    assert all(a.dtype == np.clongdouble for a in wide[6])
    S = wide[7]
    assert S.bulk_dot_abs.shape == (4, h.n_mu) and S.c_dot_abs.shape == (4, 2) and np.all(S.bulk_dot_abs > 0) and np.all(S.c_dot_abs > 0)
    dev = float(np.max(np.abs(greek_dot - wide[3])) / np.max(np.abs(wide[3])))
    assert 0 < dev < 1e-12, dev


@pytest.mark.parametrize("name", MC.NAMES)
def test_a_defect_of_one_order_radius_or_angle_moves_the_n_r_derivatives(name):
    """Sensitivity of the n_r slot: each perturbation of tests/test_oracle_mie.py moves at least one of its six derivative vectors
    by >= 1e-6 of max(1, max |vector|)."""
    c = MC.BY_NAME[name]
    h = MC.inputs(c)
    base = ML.nai2_lin_reference(*MC.lin_args(h))[3][0]
    least = (math.inf, None)
    for what, change in perturbations(h, c.n_max):
        d = dict(vars(h))
        d.update(change)
        move = greek_move(ML.nai2_lin_reference(*MC.lin_args(types.SimpleNamespace(**d)))[3][0], base)
        least = min(least, (move, what))
        assert move >= SENSITIVITY, (name, what, move)
    print("mie lin sensitivity %s: least move %.2e (%s)" % (name, least[0], least[1]))


@pytest.mark.parametrize("name", MC.NAMES)
def test_rounding_floor_of_every_output(name):
    ref, floor = MC.case_floors(name)
    print("mie lin floor %s: %s" % (name, "  ".join("%s %.1e" % (f, floor[f]) for f in MC.FAMILIES)))
    for f in MC.FAMILIES:
        assert MC.MIN_FLOOR <= floor[f] <= MC.FLOOR_LIMIT, (name, f, floor[f])
    if MC.BY_NAME[name].nquad == 1:                           # one radius: its normalised weight has no derivative
        assert not np.any(ref["greek_dot"][2:]) and not np.any(ref["bulk_f_dot"][2:]) and not np.any(ref["scal_dot"][2:])
