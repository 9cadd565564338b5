"""CPU tests that pin tests/exact_ss_oracle.py (the numpy restatement of the reference's StandaloneSS solver) without circularity:
a closed form, the invariance of all four paths under splitting a homogeneous layer, the known-answer structure of the reference's
own test geometries (test/StandaloneSS/runtests.jl:398-704), the Jacobians against central differences of the oracle itself, and
the units constant between CoreRT's rt_run_ss and StandaloneSS paths 1 and 2.

Jacobian bounds, chosen as tests/test_oracle_ss_lin.py chooses them.  The central difference of d/dtau_layer has an order-2
truncation term: it must fall by about 4 from h to h / 2 (bound 0.3 on the ratio) and the difference at h / 2 relative to the array
maximum, measured per path (MEASURED below), is gated at ten times its measured value.  Paths 1 and 2 are linear in varpi_eff, P_eff
and the surface BRDF: there the difference is rounding of the quotient only (measured 1.5e-14 .. 9.1e-14 at h = 1e-3), gated at 1e-10:
the quotient divides differences of numbers rounded at 1e-16 by 2h = 2e-3, three decades of margin over that.
"""
import math

import numpy as np
import pytest

import exact_ss_oracle as X
import ss_oracle as SS
from oracle import vsm_oracle as O

MEASURED = {"path1 tau_layer": 5.86e-7, "path2 tau_layer": 5.51e-7}     # at h / 2 = 5e-4; the ratio was 0.250 in both
MARGIN, RATIO, LINEAR = 10.0, 0.3, 1e-10


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def synthetic_greek(g, frac, n):
    """A polarized Henyey-Greenstein-like set of n Greek moments (beta of HG; gamma, alpha, zeta, delta scaled from it)."""
    l = np.arange(n)
    beta = (2 * l + 1) * float(g) ** l
    tail = np.where(l >= 2, 1.0, 0.0)
    return X.SimpleNamespace(alpha=0.8 * beta * tail, beta=beta, gamma=-frac * beta * tail / np.sqrt(6.0), delta=0.9 * beta,
                             epsilon=0.1 * beta * tail, zeta=0.7 * beta * tail)


def mixed_config(L=3, S=4, albedo=0.3, n_stokes=1, seed=2):
    rng = np.random.default_rng(seed)
    tau = lambda lo, hi: rng.uniform(lo, hi, (L, S))
    ctr = [X.RayleighSSContributor(tau(0.02, 0.06), 0.03), X.HGAerosolSSContributor(0.7, 0.9, tau(0.01, 0.05)),
           X.GreekCoefsSSContributor(synthetic_greek(0.6, 0.4, 12), 0.95, tau(0.01, 0.03)), X.AbsorptionSSContributor(tau(0.0, 0.2))]
    if n_stokes > 1:
        del ctr[1]
    return X.ExactSSConfig(X.SSGeometry(0.8, [0.4, 0.7, 0.8], [0.0, 0.9, 2.1]), X.LambertianSSSurface(albedo), ctr,
                           np.linspace(1.0, 0.7, S), n_stokes=n_stokes)


# ---- 1. closed form -------------------------------------------------------------------------------------------------------
def test_one_homogeneous_layer_closed_form():
    tau_r, tau_a, depol, I0 = 0.13, 0.07, 0.02, 0.9
    geo = X.SSGeometry(0.8, [0.4, 0.7], [0.0, 0.9])
    cfg = X.ExactSSConfig(geo, X.LambertianSSSurface(0.0), [X.RayleighSSContributor(np.full((1, 1), tau_r), depol),
                                                            X.AbsorptionSSContributor(np.full((1, 1), tau_a))], I0)
    got = X.run_exact_ss(cfg, "path1").path1
    tau, varpi = tau_r + tau_a, tau_r / (tau_r + tau_a)
    for iv, (mv, dp) in enumerate(zip(geo.mu_v, geo.dphi)):
        x = -geo.mu0 * mv + math.sqrt(1 - geo.mu0 ** 2) * math.sqrt(1 - mv ** 2) * math.cos(dp)
        P = 1 + 0.5 * ((1 - depol) / (1 + depol / 2)) * (3 * x * x - 1) / 2
        a = 1 / geo.mu0 + 1 / mv
        want = I0 * varpi * P * (1 - math.exp(-tau * a)) / (4 * math.pi * mv * a)
        assert abs(got[iv, 0, 0] - want) <= 1e-14 * want


# ---- 2. splitting invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [2, 5])
def test_splitting_a_homogeneous_layer_changes_no_path(parts):
    S = 3
    tr, th, ta = np.array([[0.05, 0.08, 0.02]]), np.array([[0.03, 0.01, 0.06]]), np.array([[0.02, 0.3, 0.0]])
    geo = X.SSGeometry(0.8, [0.4, 0.7], [0.0, 0.9])
    nodes, _ = X.gauss_legendre_01(16)
    assert np.min(np.abs(1 / geo.mu0 - 1 / nodes)) > 1e-3 and min(np.min(np.abs(1 / mv - 1 / nodes)) for mv in geo.mu_v) > 1e-3

    def cfg(k):
        rep = lambda t: np.repeat(t / k, k, axis=0)
        return X.ExactSSConfig(geo, X.LambertianSSSurface(0.3), [X.RayleighSSContributor(rep(tr), 0.03),
                               X.HGAerosolSSContributor(0.7, 0.9, rep(th)), X.AbsorptionSSContributor(rep(ta))], np.linspace(1, 0.7, S))
    one, split = X.run_exact_ss(cfg(1), "all"), X.run_exact_ss(cfg(parts), "all")
    for name in ("path1", "path2", "path3", "path4", "total"):
        e = _rel(getattr(split, name), getattr(one, name))
        print("%s: %d sublayers vs one %.2e" % (name, parts, e))
        assert np.max(np.abs(getattr(one, name))) > 0 and e <= 1e-13, (name, e)


# ---- 3. the reference's test geometries -----------------------------------------------------------------------------------
def _rayleigh_cfg(n):
    return X.ExactSSConfig(X.SSGeometry(0.8, [0.4, 0.7], [0.0, 0.9]), X.LambertianSSSurface(0.3),
                           [X.RayleighSSContributor(np.array([[0.05, 0.07], [0.1, 0.04]]))], [1.0, 0.7], n_stokes=n)


def test_rayleigh_vector_path1_is_scalar_path1_times_phase_column():
    scalar = X.run_exact_ss(_rayleigh_cfg(1), "paths_1_2")
    assert scalar.total.shape == (2, 1, 2)
    for n in (2, 3):
        cfg = _rayleigh_cfg(n)
        vec = X.run_exact_ss(cfg, "paths_1_2")
        for iv in range(2):
            col = X.phase_matrix_first_column(X.get_greek_rayleigh(0.0), 0.8, cfg.geometry.mu_v[iv], cfg.geometry.dphi[iv], n)
            want = scalar.path1[iv, 0][None, :] * (col / col[0])[:, None]
            assert np.allclose(vec.path1[iv], want, rtol=1e-12, atol=1e-14)
        assert np.allclose(vec.path2[:, :1], scalar.path2, rtol=1e-12, atol=1e-14)      # Lambertian path 2: I only
        assert np.all(vec.path2[:, 1:] == 0)
        assert np.allclose(vec.total, vec.path1 + vec.path2, rtol=1e-14)
    assert np.all(X.run_exact_ss(_rayleigh_cfg(3), "path1").path2 == 0)


def _greek_cfg(n=3):
    greek = synthetic_greek(0.62, 0.45, 18)
    return greek, X.ExactSSConfig(X.SSGeometry(0.81, [0.44, 0.68], [0.25, 1.0]), X.LambertianSSSurface(0.23),
                                  [X.GreekCoefsSSContributor(greek, 0.91, np.array([[0.025], [0.04]])),
                                   X.AbsorptionSSContributor(np.array([[0.01], [0.02]]))], [1.0], n_stokes=n)


def test_greek_iquv_has_a_zero_v_row():
    _, cfg = _greek_cfg(4)
    p1 = X.run_exact_ss(cfg, "path1").path1
    assert p1.shape == (2, 4, 1) and np.all(p1[:, 3] == 0) and np.all(p1[:, :3] != 0)


def test_truncation_helpers_and_back_correction():
    greek, cfg = _greek_cfg()
    exact = X.run_exact_ss(cfg, "paths_1_2")
    full, low, lamb = X.truncated_ss_path1(cfg, len(greek.beta)), X.truncated_ss_path1(cfg, 4), X.truncated_ss_path2(cfg, 1)
    assert np.allclose(full, exact.path1, rtol=1e-10, atol=1e-13)
    assert np.allclose(lamb, exact.path2, rtol=1e-12, atol=1e-14)
    assert np.all(np.isfinite(low)) and np.max(np.abs(low - exact.path1)) > 1e-9
    corrected = X.apply_back_correction(low + lamb, cfg, l_trunc=4, max_m=1)
    assert np.allclose(corrected, exact.total, rtol=1e-10, atol=1e-13)
    with pytest.raises(ValueError):
        X.truncated_ss_path1(cfg, 1)
    hg = X.ExactSSConfig(X.SSGeometry(0.79, [0.5], [0.8]), X.LambertianSSSurface(0.0),
                         [X.HGAerosolSSContributor(0.7, 0.9, np.array([[0.03], [0.02]]))], [1.0])
    assert np.max(np.abs(X.truncated_ss_path1(hg, 3) - X.run_exact_ss(hg, "path1").path1)) > 1e-8
    ray = X.ExactSSConfig(cfg.geometry, cfg.surface, [X.RayleighSSContributor(np.array([[0.02], [0.03]]))], [1.0], n_stokes=3)
    assert np.allclose(X.truncated_ss_path1(ray, 3), X.run_exact_ss(ray, "path1").path1, rtol=1e-12, atol=1e-14)


def test_coxmunk_truncation_converges_toward_exact():
    cfg = X.ExactSSConfig(X.SSGeometry(0.78, [0.42], [0.15]), X.CoxMunkSSSurface(5.0, complex(1.34, 1e-8), include_whitecaps=False),
                          [X.AbsorptionSSContributor(np.array([[0.02], [0.06]]))], [1.0], n_stokes=2)
    exact = X.run_exact_ss(cfg, "path2").path2
    m1, m48 = X.truncated_ss_path2(cfg, 1), X.truncated_ss_path2(cfg, 48)
    assert np.all(np.isfinite(m48)) and np.linalg.norm(m48 - exact) < np.linalg.norm(m1 - exact)
    with pytest.raises(ValueError):
        X.truncated_ss_path2(cfg, 0)


def test_mixed_scene_paths_are_positive_and_refusals_raise():
    cfg = mixed_config()
    res = X.run_exact_ss(cfg, "all")
    assert all(np.all(getattr(res, k) > 0) for k in ("path1", "path2", "path3", "path4"))
    assert np.allclose(res.total, res.path1 + res.path2 + res.path3 + res.path4, rtol=1e-14)
    assert np.all(X.run_exact_ss(mixed_config(albedo=0.0), "all").path3 == 0)
    with pytest.raises(ValueError):
        X.run_exact_ss(mixed_config(n_stokes=3), "all")                # vector Stokes: paths 1 and 2 only
    with pytest.raises(ValueError):
        X.run_exact_ss(X.ExactSSConfig(cfg.geometry, cfg.surface, cfg.contributors, cfg.I0, n_stokes=3), "path1")   # HG in a vector run
    with pytest.raises(ValueError):
        X.run_exact_ss(X.ExactSSConfig(cfg.geometry, X.CoxMunkSSSurface(5.0), cfg.contributors, cfg.I0), "path3")
    with pytest.raises(ValueError):
        X.run_exact_ss(cfg, "path5")


# ---- 4. Jacobians ---------------------------------------------------------------------------------------------------------
def test_jacobians_match_central_differences_of_the_oracle():
    cfg = mixed_config(n_stokes=3)
    res = X.run_exact_ss_with_jacobians(cfg, "paths_1_2")
    L, S = cfg.contributors[0].tau.shape
    op = X.precompute_optics(cfg, 3)
    brdf = X.precompute_surface_brdf(cfg, 3, S)
    base = X.run_from_seam(cfg, op.tau_layer, op.varpi_eff, op.P_eff, brdf)
    assert _rel(base[0], res.path1) <= 1e-14 and _rel(base[1], res.path2) <= 1e-14
    j1, j2 = res.jacobians["path1"], res.jacobians["path2"]

    def fd(step, which, iz):
        out = []
        for sgn in (1, -1):
            t, w, P, b = op.tau_layer.copy(), op.varpi_eff.copy(), op.P_eff.copy(), brdf.copy()
            if which == "tau":
                t[iz] += sgn * step
            elif which == "varpi":
                w[iz] += sgn * step
            elif which == "P":
                P[:, :, iz] += sgn * step
            else:
                b += sgn * step
            out.append(X.run_from_seam(cfg, t, w, P, b))
        return [(u - d) / (2 * step) for u, d in zip(*out)]

    h = 1e-3
    d1 = {1: [np.zeros_like(j1["tau_layer"]) for _ in range(2)], 2: [np.zeros_like(j1["tau_layer"]) for _ in range(2)]}
    lin = {"varpi": np.zeros_like(j1["tau_layer"]), "P": np.zeros_like(j1["tau_layer"])}
    for iz in range(L):
        for i, step in enumerate((h, h / 2)):
            q1, q2 = fd(step, "tau", iz)
            d1[1][i][..., iz], d1[2][i][..., iz] = q1, q2
        lin["varpi"][..., iz], lin["P"][..., iz] = fd(h, "varpi", iz)[0], fd(h, "P", iz)[0]
    for name, an, num in (("path1 tau_layer", j1["tau_layer"], d1[1]), ("path2 tau_layer", j2["tau_layer"], d1[2])):
        e1, e2 = _rel(an, num[0]), _rel(an, num[1])
        print("%s: FD difference %.3e at h = %g, %.3e at h / 2 (ratio %.3f)" % (name, e1, h, e2, e2 / e1))
        assert np.max(np.abs(an)) > 0 and e2 <= MARGIN * MEASURED[name] and e2 <= RATIO * e1, (name, e1, e2)
    for name, an, num in (("varpi_eff", j1["varpi_eff"], lin["varpi"]), ("P_eff", j1["P_eff"], lin["P"]),
                          ("surface_brdf", j2["surface_brdf"], fd(h, "rho", 0)[1])):
        e = _rel(an, num)
        print("%s: FD difference %.3e (linear: rounding only)" % (name, e))
        assert np.max(np.abs(an)) > 0 and e <= LINEAR, (name, e)
    assert np.array_equal(res.jacobians["total"]["tau_layer"], j1["tau_layer"] + j2["tau_layer"])


# ---- 5. units --------------------------------------------------------------------------------------------------------------
UNITS_CONSTANT = 1.0     # rt_run_ss R = 1 x StandaloneSS (path 1 + path 2) at I0 = 1: measured 1 to 4e-16 in every Stokes row


def test_rt_run_ss_equals_exact_paths_1_2_at_unit_I0():
    """The constant between CoreRT's single-scattering R (oracle: tests/ss_oracle.py) and StandaloneSS at I0 = 1.  A Rayleigh-only
    Stokes_IQU column, m = 0..2 summed (three Greek moments: the truncated series is exact), viewing angles off the SZA.  Over a
    black surface R against path 1; the share a Lambertian albedo adds against path 2.  StandaloneSS carries 1 / (4 pi) and
    albedo / pi explicitly, CoreRT carries them in the Fourier weights 0.5 / pi, 1 / pi of postprocessing_vza!: the constant is 1,
    not pi, and the Q and U rows agree in sign."""
    S, L, depol = 3, 3, 0.0279
    sza, vza, vaz = 40.0, [20.0, 55.0], [30.0, 140.0]
    tau_rayl = np.tile(np.linspace(0.03, 0.08, L), (S, 1)) * np.linspace(1.0, 2.0, S)[:, None]
    run = lambda a: SS.rt_run_ss(O.build_model("IQU", 7, sza, vza, vaz, tau_rayl=tau_rayl, depol=depol, albedo=a, m_max=2))[0]
    R0, R3 = run(0.0), run(0.3)
    cfg = X.ExactSSConfig(X.SSGeometry(math.cos(math.radians(sza)), [math.cos(math.radians(v)) for v in vza],
                                       [math.radians(a) for a in vaz]), X.LambertianSSSurface(0.3),
                          [X.RayleighSSContributor(tau_rayl.T, depol)], 1.0, n_stokes=3)
    res = X.run_exact_ss(cfg, "paths_1_2")
    ratio = R0 / res.path1
    print("R / path1 per Stokes row: I %s Q %s U %s" % tuple(np.array2string(ratio[:, k].ravel(), precision=15) for k in range(3)))
    print("surface share / path2 (I row): %s" % np.array2string(((R3 - R0)[:, 0] / res.path2[:, 0]).ravel(), precision=15))
    assert np.all(res.path1 != 0)
    assert _rel(R0, UNITS_CONSTANT * res.path1) <= 1e-13
    assert _rel(R3 - R0, UNITS_CONSTANT * res.path2) <= 1e-13
    assert _rel(R3, UNITS_CONSTANT * res.total) <= 1e-13
