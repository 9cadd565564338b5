"""CPU tests of tests/truncation_lin_oracle.py (the numpy restatement of the reference's linearized delta-BGE truncation,
truncate_phase_lin.jl): its literal form against the fused form the device computes, against central differences of
truncation_oracle.truncate_phase, on a series that is its own truncation, and end to end through the oracle's rt_run_lin against
central differences of Mie + truncation + rt_run.  No kernel runs here.  The measured figures are in DESIGN.md 4.24."""
import functools
import math

import numpy as np
import pytest

import mie_lin_oracle as ML
import mie_oracle as MO
import truncation_lin_oracle as TL
import truncation_oracle as TO
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL

TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength
COARSE_MODE = (1.0, 1.8, 1.53, 0.008, 0.76)
FINE_MODE = (0.08, 1.6, 1.45, 0.005, 0.76)
SETS = {"test": (TEST_AEROSOL, 3.0, 37, 113), "coarse": (COARSE_MODE, 15.0, 200, 307)}
NAMES = ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")


@functools.lru_cache(maxsize=None)
def _mie_lin(aer, r_max, nquad):
    r_m, sigma_g, n_r, n_i, lam = aer
    return ML.compute_aerosol_optical_properties_lin(MO.LogNormal(r_m, sigma_g), n_r, n_i, lam, r_max, nquad)


def _set(name):
    aer, r_max, nquad, n_mu = SETS[name]
    o = _mie_lin(aer, r_max, nquad)
    assert o.greek.shape == (6, n_mu) and o.greek_dot.shape == (4, 6, n_mu)
    return o


# ---- 1. the two forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_max", [3, 17, 20, 40, 64, 112])
@pytest.mark.parametrize("name", ["test", "coarse"])
def test_literal_and_fused_form_agree(name, l_max):
    """b' - A' x = Bt g without any A'.  The epsilon system of the coarse set is left out: f34 changes sign there, the weights
    1 / f34^3 blow up and the two forms of the reference's own formula part ways in float64 (7.8e-9 at l_max = 20, 3.6e-6 at
    112) -- tests/test_gpu_truncation_lin.py scales its bound with that disagreement."""
    o = _set(name)
    d = TL.form_disagreement(o.greek, o.greek_dot, l_max)
    print("dbge lin forms %s l_max %d: d = %s" % (name, l_max, " ".join("%.2e" % v for v in d)))
    for k, system in enumerate(TL.SYSTEMS):
        if name == "coarse" and system == "epsilon":
            continue
        assert d[k] <= 1e-8, (system, d[k])


# ---- 2. central differences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_max", [3, 17, 20])
def test_literal_form_against_central_differences(l_max):
    """truncate_phase(greek +- h greek_dot[s]) at fixed nodes, h = 1e-6."""
    o = _set("test")
    h = 1e-6
    _, _, _, gtd, c0_dot, ft_dot = TL.truncate_phase_lin(o.greek, o.greek_dot, l_max)
    worst = 0.0
    for s in range(4):
        gp, cp, _ = TO.truncate_phase(o.greek + h * o.greek_dot[s], l_max)
        gm, cm, _ = TO.truncate_phase(o.greek - h * o.greek_dot[s], l_max)
        fd, fd_c0 = (gp - gm) / (2 * h), (cp - cm) / (2 * h)
        for c, fam in enumerate(NAMES):
            err = float(np.max(np.abs(gtd[s, c] - fd[c]))) / max(1.0, float(np.max(np.abs(fd[c]))))
            worst = max(worst, err)
            assert err <= 1e-5, (ML.SLOTS[s], fam, err)
        err = abs(c0_dot[s] - fd_c0) / max(1.0, abs(fd_c0))
        worst = max(worst, err)
        assert err <= 1e-5 and ft_dot[s] == -c0_dot[s], (ML.SLOTS[s], err)
    print("dbge lin central differences l_max %d: worst %.2e" % (l_max, worst))


# ---- 3. fixed point --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_max", [19, 24])
def test_a_series_below_l_max_keeps_its_derivatives(l_max):
    """The fine mode's 19 coefficients and their derivatives zero-padded to 40: f and f' lie in the span of the basis, the fit and
    its derivative are exact, c0 = 1 whatever the parameters."""
    o = _mie_lin(FINE_MODE, 0.35, 20)
    assert o.greek.shape == (6, 19)
    greek = np.concatenate([o.greek, np.zeros((6, 21))], axis=1)
    greek_dot = np.concatenate([o.greek_dot, np.zeros((4, 6, 21))], axis=2)
    for solve in (TL.solve_literal, TL.solve_fused):
        _, c0, _, gtd, c0_dot, ft_dot = TL.truncate_phase_lin(greek, greek_dot, l_max, solve=solve)
        err = float(np.max(np.abs(gtd - greek_dot[:, :, :l_max])))
        print("dbge lin fixed point l_max %d %s: max|d greek'| %.2e  max|f_trunc'| %.2e" % (l_max, solve.__name__, err,
                                                                                             np.max(np.abs(ft_dot))))
        assert err <= 1e-9 and np.max(np.abs(ft_dot)) <= 1e-10 and abs(c0 - 1.0) <= 1e-10


def test_mie_node_functions_are_what_the_coefficients_reconstruct():
    """The bulk_f_dot path hands over f and f' at the nodes; they are what the n_mu coefficients and derivatives reconstruct.
    Analysis (the Greek sums over 113 nodes) and synthesis (113 moments) are n_mu^2 products of magnitude <= max |f| each:
    n_mu^2 2^-53 = 1.4e-12 max |f| in a linear rounding model; the bound is 1e-10 max |f| (1.0e-11 measured for f and for f')."""
    o = _set("test")
    f, f_dot = TL.mie_node_functions(o)
    fr, fr_dot, _, _ = TL.reconstruct_lin(o.greek, o.greek_dot, o.host.mu)
    assert f.shape == fr.shape == (3, 113) and f_dot.shape == fr_dot.shape == (4, 3, 113)
    assert np.max(np.abs(f - fr)) <= 1e-10 * np.max(np.abs(fr))
    assert np.max(np.abs(f_dot - fr_dot)) <= 1e-10 * max(1.0, np.max(np.abs(fr_dot)))


def test_a_scalar_phase_function_keeps_exact_zero_derivatives():
    greek = TO.henyey_greenstein_greek(0.7, 200)
    greek_dot = np.zeros((4, 6, 200))
    l = np.arange(200)
    greek_dot[0, 1] = l * (2 * l + 1) * 0.7 ** np.maximum(l - 1, 0)      # d beta / d g
    gt, c0, _, gtd, c0_dot, _ = TL.truncate_phase_lin(greek, greek_dot, 20)
    assert not np.any(gtd[:, 2]) and not np.any(gtd[:, 4]) and not np.any(gtd[1:]) and np.any(gtd[0, 1])
    assert abs(gtd[0, 1, 0]) <= 1e-12                                    # beta_t[0] = 1 whatever g


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
def _tabulated_mie(aer, r_max, nquad, d_mu=0.0, d_sigma=0.0, n_r=None, n_i=None):
    """The LogNormal's own nodes with the weights of LogNormal(mu + d_mu, sigma + d_sigma) on them."""
    r_m, sigma_g, nr0, ni0, lam = aer
    base = MO.LogNormal(r_m, sigma_g)
    r, w_r = MO.gauleg_log(nquad, max(base.quantile(1e-8), 1e-6 * r_max), r_max)
    ln = MO.LogNormal(math.exp(base.mu + d_mu), math.exp(base.sigma + d_sigma))
    return MO.compute_aerosol_optical_properties(None, nr0 if n_r is None else n_r, ni0 if n_i is None else n_i, lam, None, None,
                                                 tabulated=(r, ln.pdf(r) * w_r))


def test_truncated_jacobians_end_to_end_through_rt_run_lin():
    """The test aerosol (113 coefficients) truncated to l_max = 20 in the scene and with the steps of
    tests/test_gpu_mie_lin.py::test_fine_mode_jacobians_end_to_end_through_rt_run_lin: the oracle's rt_run_lin on the oracle's
    truncated lin optics, slots 1-4, against central differences (h = 1e-5) of oracle Mie + truncate_phase + rt_run, the radius
    nodes held fixed through the tabulated form.  That test's criterion -- and the same run with f_trunc_dot zeroed misses it."""
    aer, r_max, nquad, _ = SETS["test"]
    ref = _set("test")
    l_max = 20
    g_t, c0, f_t, gtd, c0_dot, ft_dot = TL.truncate_phase_lin(ref.greek, ref.greek_dot, l_max)
    assert 0.1 < f_t < 0.2
    rng = np.random.default_rng(11)
    Sp, L = 8, 2
    tau_rayl = np.tile(0.02 * np.ones(L), (Sp, 1))
    tau_abs = 10.0 ** rng.uniform(-3, 0, (Sp, L))
    tau_aer = np.array([[0.05, 0.2]])
    tau_aer_dot = np.zeros((1, 7, L))
    tau_aer_dot[0, 0], tau_aer_dot[0, 5], tau_aer_dot[0, 6] = [0.25, 1.0], [0.5, -0.5], [-0.2, 0.3]
    geo = ("IQU", 20, 40.0, [30.0, 0.0], [0.0, 75.0])
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, tau_aer=tau_aer, depol=0.03, albedo=0.1, m_max=4)
    om = O.build_model(*geo, aerosols=[O.AerosolOptics(O.GreekCoefs(*g_t), ref.ssa, f_t)], **kw)

    def lin_run(f_trunc_dot):
        ol = OL.LinModel([tau_abs.copy()], tau_aer_dot=tau_aer_dot,
                         lin_aerosol_optics=[OL.LinAerosolOptics([O.GreekCoefs(*gtd[s]) for s in range(4)], ref.ssa_dot,
                                                                 f_trunc_dot)])
        return OL.rt_run_lin(om, ol)

    _, _, Rd, Td = lin_run(ft_dot)
    _, _, Rd0, Td0 = lin_run(np.zeros(4))
    h = 1e-5

    def forward(**kwargs):
        o = _tabulated_mie(aer, r_max, nquad, **kwargs)
        g, _, ft = TO.truncate_phase(o.greek, l_max)
        return O.rt_run(O.build_model(*geo, aerosols=[O.AerosolOptics(O.GreekCoefs(*g), o.ssa, ft)], **kw))

    n_r, n_i = aer[2], aer[3]
    steps = [lambda s: dict(n_r=n_r + s), lambda s: dict(n_i=n_i + s), lambda s: dict(d_mu=s), lambda s: dict(d_sigma=s)]
    for k, step in enumerate(steps):
        (Rp, Tp), (Rm, Tm) = forward(**step(h)), forward(**step(-h))
        missed = False
        for an, an0, fd in ((Rd[..., 1 + k], Rd0[..., 1 + k], (Rp - Rm) / (2 * h)), (Td[..., 1 + k], Td0[..., 1 + k], (Tp - Tm) / (2 * h))):
            err = np.abs(fd - an) / np.abs(fd).max()
            err0 = np.abs(fd - an0) / np.abs(fd).max()
            print("  slot %d (%s): err max %.2e mean %.2e   without f_trunc_dot: max %.2e mean %.2e"
                  % (1 + k, ML.SLOTS[k], err.max(), err.mean(), err0.max(), err0.mean()))
            assert err.max() < 1e-3 and err.mean() < 1e-4, (k, err.max(), err.mean())
            missed |= not (err0.max() < 1e-3 and err0.mean() < 1e-4)
        assert missed, "slot %d meets the criterion without f_trunc_dot: the scene does not see it" % (1 + k)
