"""CPU tests of tests/truncation_oracle.py (the numpy restatement of the reference's delta-BGE truncation, truncate_phase.jl) against
properties that do not depend on how it solves: a series of degree below l_max is a fixed point, the normal equations give what an
independent weighted least-squares solve of the same problem gives, the delta-M scaling that reads f_trunc conserves the absorption
optical depth, and c0 grows towards 1 with l_max.  No kernel runs here."""
import math

import numpy as np
import pytest

import mie_oracle as MO
import truncation_oracle as TO

TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength (test_mie_gpu.jl)
FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)
NAMES = ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


def _mie(aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    return MO.compute_aerosol_optical_properties(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad)


@pytest.fixture(scope="module")
def coarse():
    o = _mie(TEST_AEROSOL, 3.0, 37)
    assert o.greek.shape == (6, 113)
    return o


@pytest.fixture(scope="module")
def fine_padded():
    o = _mie(FINE_MODE, 0.35, 20)
    assert o.greek.shape == (6, 19)
    return np.concatenate([o.greek, np.zeros((6, 21))], axis=1)


@pytest.mark.parametrize("l_max", [19, 24])
def test_a_series_below_l_max_is_returned_unchanged(fine_padded, l_max):
    """Case A: 19 Mie coefficients zero-padded to 40.  The fitted functions lie in the span of the basis, so the fit is exact."""
    g, c0, f_t = TO.truncate_phase(fine_padded, l_max)
    assert g.shape == (6, l_max)
    assert abs(c0 - 1.0) <= 1e-10 and abs(f_t) <= 1e-10
    for i, name in enumerate(NAMES):
        assert np.max(np.abs(g[i] - fine_padded[i, :l_max])) <= 1e-10, name


def test_a_scalar_series_below_l_max_is_returned_unchanged_by_the_lowconf_variant():
    """Case B: Henyey-Greenstein g = 0.3 cut to 12 terms, padded to 40, l_max = 12, cone of 2 degrees.  gamma and epsilon are
    series of exact zeros: they stay exact zeros (the reference returns NaN there)."""
    greek = np.concatenate([TO.henyey_greenstein_greek(0.3, 12), np.zeros((6, 28))], axis=1)
    g, c0, f_t = TO.truncate_phase_lowconf(greek, 12, 2.0)
    assert abs(c0 - 1.0) <= 1e-10 and abs(f_t) <= 1e-10
    assert np.max(np.abs(g - greek[:, :12])) <= 1e-10
    assert not np.any(g[2]) and not np.any(g[4])


@pytest.mark.parametrize("l_max", [8, 20, 40])
def test_normal_equations_equal_an_independent_weighted_lstsq(coarse, l_max):
    """min sum_k w_k ((B c)_k / f_k - 1)^2 solved by lstsq on the scaled design matrix, not through A = B^T W B."""
    greek = coarse.greek
    mu, w = MO.gausslegendre(greek.shape[1])
    f11, f12, f34, P, P2 = TO.reconstruct(greek, mu)
    fac = TO.prefactor(l_max)
    g, c0, _ = TO.truncate_phase(greek, l_max)
    sw = np.sqrt(w)
    cl = np.linalg.lstsq(P[:, :l_max] * (sw / f11)[:, None], sw, rcond=None)[0]
    B2 = fac[2:] * P2[:, 2:l_max]
    gam = np.linalg.lstsq(B2 * (sw / f12)[:, None], sw, rcond=None)[0]
    eps = np.linalg.lstsq(B2 * (sw / f34)[:, None], sw, rcond=None)[0]
    assert abs(cl[0] - c0) <= 1e-6
    assert np.max(np.abs(cl / cl[0] - g[1])) <= 1e-6
    assert np.max(np.abs(gam - g[2, 2:])) <= 1e-6 and np.max(np.abs(eps - g[4, 2:])) <= 1e-6
    assert np.all(g[2, :2] == 0) and np.all(g[4, :2] == 0)
    cut = greek[1, :l_max] - cl
    for i in (0, 3, 5):
        assert np.max(np.abs((greek[i, :l_max] - cut) / cl[0] - g[i])) <= 1e-6, NAMES[i]


def test_bulk_functions_in_place_of_the_reconstruction(coarse):
    """The Mie path hands over f11, f12, f34 at the nodes; they are what the n_mu coefficients reconstruct."""
    f = (coarse.bulk_f[0], coarse.bulk_f[2], coarse.bulk_f[3])
    a = TO.truncate_phase(coarse.greek, 20)
    b = TO.truncate_phase(coarse.greek, 20, f)
    assert np.max(np.abs(a[0] - b[0])) <= 1e-8 and abs(a[1] - b[1]) <= 1e-8


def test_delta_m_budget_is_conserved_through_createAero(vsm, coarse):
    """tau (1 - omega) of the scaled layer equals the unscaled one's for the f_trunc the truncation returns."""
    H = vsm.host_model
    g, c0, f_t = TO.truncate_phase(coarse.greek, 20)
    assert 0.1 < f_t < 0.2
    ao = H.AerosolOptics(H.GreekCoefs(*g), coarse.ssa, f_t)
    tau = 0.37
    core = H.createAero(tau, ao, None, None)
    tau_s, ssa_s = float(core.tau), float(core.varpi)
    assert abs(tau_s * (1 - ssa_s) - tau * (1 - coarse.ssa)) <= 1e-14
    assert abs(tau_s - (1 - f_t * coarse.ssa) * tau) <= 1e-15


def test_c0_grows_towards_one_with_l_max(coarse):
    c0 = [TO.truncate_phase(coarse.greek, l)[1] for l in (8, 20, 40, 64)]
    print("c0 at l_max = 8, 20, 40, 64: " + " ".join("%.6f" % v for v in c0))
    assert all(0.0 < v <= 1.0 for v in c0)
    assert all(b >= a for a, b in zip(c0, c0[1:]))
    for v, want in zip(c0, (0.582, 0.882, 0.994, 1.000)):      # measured with the reference's formulas
        assert abs(v - want) <= 5e-4


def test_lowconf_excludes_the_forward_cone(coarse):
    """Only the nodes below cos(delta) enter: the problems of 2 and 5 degrees differ by the nodes between the two cones."""
    mu, _ = MO.gausslegendre(113)
    n2 = TO.lowconf_problems(coarse.greek, 20, 2.0)[0][0].shape[0]
    n5 = TO.lowconf_problems(coarse.greek, 20, 5.0)[0][0].shape[0]
    assert n2 == np.count_nonzero(mu < math.cos(math.radians(2.0))) and n5 == np.count_nonzero(mu < math.cos(math.radians(5.0)))
    assert 20 <= n5 < n2 <= 113
    g, c0, f_t = TO.truncate_phase_lowconf(coarse.greek, 20, 2.0)
    assert 0.0 < c0 < 1.0 and abs(g[1, 0] - 1.0) <= 1e-15 and f_t == 1.0 - c0


def test_host_types(vsm):
    S = vsm.Scattering
    assert S.δBGE is S.DeltaBGE and S.DeltaBGE(20).delta_angle == 0.0 and S.NoTruncation() == S.NoTruncation()
    assert issubclass(S.TruncatedAerosolOptics, vsm.host_model.AerosolOptics)
    with pytest.raises(vsm.VSMError):
        S.truncate_phase(S.DeltaBGE(20), vsm.host_model.AerosolOptics(vsm.host_model.henyey_greenstein_greek(0.7, 99), 1.0),
                         vsm.Architectures.CPU())
