"""CPU checks of the linearized multi-sensor oracle (tests/ms_lin_oracle.py): its Jacobians at interior levels, at level Nz and at
level 0 against central finite differences of the prototype's transcription (ms_oracle.ms_reference) for gas, albedo, aerosol
tau_ref and Cox-Munk wind-speed slots; level 0 against OL.rt_run_lin; the forward part against ms_oracle.ms_segmented; the
push-through derivative of the level equation against the explicit two-inverse one; the level just above a black surface."""
import copy

import numpy as np
import pytest

import ms_lin_oracle as MSL
import ms_oracle as MS
from oracle import vsm_oracle as O
from oracle import vsm_oracle_coxmunk as CM
from oracle import vsm_oracle_lin as OL

FD_TOL = 2e-6    # as test_oracle_lin.test_jacobians_match_finite_differences


def _gas_model(pol, S=2, L=5, albedo=0.2, scale=(1.0, 1.0), seed=0):
    """Two gases (x_g = multiplicative scale of gas g's absorption: d tau_abs / d x_g = base_g), a Lambertian albedo."""
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    base_a = 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    base_b = 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    base_b[:, 0] = 0.0                      # gas b is absent from the top layer
    tau_abs = scale[0] * base_a + scale[1] * base_b
    mdl = O.build_model(pol, 9, 40.0, [30.0, 5.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=albedo,
                        m_max=2)
    return mdl, OL.LinModel([base_a, base_b])


def _check_fd(levels, an, plus, minus, h, what):
    """an: per level [nV, n, S] analytic slot; plus / minus: per level forward values at x +- h."""
    for i, l in enumerate(levels):
        fd = (plus[i] - minus[i]) / (2 * h)
        scale = np.abs(fd).max()
        assert scale > 0, (what, l)
        err = np.abs(an[i] - fd).max() / scale
        assert err <= FD_TOL, (what, l, err)


@pytest.mark.parametrize("pol", ["I", "IQU", "IQUV"])
def test_gas_and_albedo_jacobians_match_finite_differences(pol):
    levels = [2, 0, 5, 3]                                   # interior levels, level Nz, level 0
    mdl, lin = _gas_model(pol)
    uw, dw, uwd, dwd = MSL.ms_lin_segmented(mdl, lin, levels)
    assert uwd[0].shape == uw[0].shape + (3,)
    h = 1e-5
    for p, (kp, km) in enumerate([(dict(scale=(1 + h, 1.0)), dict(scale=(1 - h, 1.0))),
                                  (dict(scale=(1.0, 1 + h)), dict(scale=(1.0, 1 - h))),
                                  (dict(albedo=0.2 + h), dict(albedo=0.2 - h))]):
        up, dp = MS.ms_reference(_gas_model(pol, **kp)[0], levels)
        um, dm = MS.ms_reference(_gas_model(pol, **km)[0], levels)
        _check_fd(levels, [x[..., p] for x in uwd], up, um, h, (pol, p, "uw"))
        _check_fd(levels, [x[..., p] for x in dwd], dp, dm, h, (pol, p, "dw"))


def test_aerosol_tau_ref_jacobian_matches_finite_differences():
    from tests.test_oracle_lin import _aerosol_scene
    levels = [0, 1, 2, 3]
    mdl, lin = _aerosol_scene("IQU")
    uw, dw, uwd, dwd = MSL.ms_lin_segmented(mdl, lin, levels)
    assert uwd[0].shape[-1] == 9
    h = 1e-5
    e = np.zeros(7)
    e[0] = h
    up, dp = MS.ms_reference(_aerosol_scene("IQU", e)[0], levels)
    um, dm = MS.ms_reference(_aerosol_scene("IQU", -e)[0], levels)
    _check_fd(levels, [x[..., 0] for x in uwd], up, um, h, "uw tau_ref")
    _check_fd(levels, [x[..., 0] for x in dwd], dp, dm, h, "dw tau_ref")


def _coxmunk_model(S=2, L=4):
    rng = np.random.default_rng(3)
    tau_rayl = np.tile(np.full(L, 0.12 / L), (S, 1))
    g = rng.uniform(0.5, 1.5, (S, L)) * 0.02
    mdl = O.build_model("IQU", 7, 30.0, [45.0, 15.0], [180.0, 0.0], tau_rayl, tau_abs=g, depol=0.03, m_max=3)
    return mdl, OL.LinModel([g])


def _brdf_fill(om, surf):
    mu = om.quad_points.qp_mu.astype(np.float64)
    return lambda m, a, ts: CM.create_surface_layer_brdf(CM.reflectance(surf, om.pol.n, mu, m), a, m, om.pol, om.quad_points, ts,
                                                         om.FT)


def test_coxmunk_wind_speed_jacobian_matches_finite_differences():
    levels = [0, 2, 4]
    mdl, lin = _coxmunk_model()
    U = 5.0
    uw, dw, uwd, dwd = MSL.ms_lin_segmented(mdl, lin, levels, surface=CM.CoxMunkSurface(U))
    h = 1e-4
    up, dp = MS.ms_reference(mdl, levels, surface=_brdf_fill(mdl, CM.CoxMunkSurface(U + h)))
    um, dm = MS.ms_reference(mdl, levels, surface=_brdf_fill(mdl, CM.CoxMunkSurface(U - h)))
    _check_fd(levels, [x[..., 1] for x in uwd], up, um, h, "uw wind")
    # dw at level 0 is T: the Cox-Munk slot reaches it only through the surface, and above the surface the downwelling field does
    # not depend on it at all (exact zeros both ways) -- compare where the derivative is non-zero
    _check_fd(levels[1:], [x[..., 1] for x in dwd[1:]], dp[1:], dm[1:], h, "dw wind")


@pytest.mark.parametrize("pol", ["I", "IQUV"])
def test_level0_is_rt_run_lin_and_forward_part_is_ms_segmented(pol):
    levels = [0, 4, 1, 5]
    mdl, lin = _gas_model(pol, S=3)
    uw, dw, uwd, dwd = MSL.ms_lin_segmented(mdl, lin, levels)
    R, T, Rd, Td = OL.rt_run_lin(mdl, lin)
    for a, b in ((uw[0], R), (dw[0], T), (uwd[0], Rd), (dwd[0], Td)):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-16)
    us, ds = MS.ms_segmented(mdl, levels)
    for i in range(len(levels)):
        for a, b in ((uw[i], us[i]), (dw[i], ds[i])):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (levels[i], np.abs(a - b).max())


@pytest.mark.parametrize("N,S,P,shared", [(6, 3, 4, False), (21, 2, 3, True), (40, 1, 2, False)])
def test_push_through_derivative_equals_explicit_two_inverse_derivative(N, S, P, shared):
    rng = np.random.default_rng(N)
    FT = np.float64
    A = 0.9 * rng.uniform(0, 1, (S, N, N)) / N
    B = 0.9 * rng.uniform(0, 1, (1 if shared else S, N, N)) / N
    a, c = rng.uniform(0, 1, (S, N)), rng.uniform(0, 1, (S, N))
    Ad, Bd = rng.normal(0, 1, (P, S, N, N)) / N, rng.normal(0, 1, (P,) + B.shape) / N
    ad, cd = rng.normal(0, 1, (P, S, N)), rng.normal(0, 1, (P, S, N))
    got = MSL.level_lin_push_through(FT, A, a, B, c, Ad, ad, Bd, cd)
    ref = MSL.level_lin_explicit(FT, A, a, B, c, Ad, ad, Bd, cd)
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 1e-12 * np.abs(r).max()
    # and the derivative is the derivative: a central difference along (A', a', B', c') for one slot
    h = 1e-6
    u1, d1 = MS.level_push_through(FT, A + h * Ad[0], a + h * ad[0], B + h * Bd[0], c + h * cd[0])
    u0, d0 = MS.level_push_through(FT, A - h * Ad[0], a - h * ad[0], B - h * Bd[0], c - h * cd[0])
    for an, fd in ((got[2][0], (u1 - u0) / (2 * h)), (got[3][0], (d1 - d0) / (2 * h))):
        assert np.abs(an - fd).max() <= 1e-7 * np.abs(fd).max()


def test_black_surface_level_nz():
    """Above a black surface the level-Nz upwelling field is zero and so is its derivative with respect to every layer parameter;
    the albedo slot is not (it is the radiance a unit albedo would add: finite differences check it above)."""
    levels = [5, 2]
    mdl, lin = _gas_model("IQU", albedo=0.0)
    uw, dw, uwd, dwd = MSL.ms_lin_segmented(mdl, lin, levels)
    assert np.all(uw[0] == 0) and np.all(uwd[0][..., :2] == 0)
    assert np.abs(uwd[0][..., 2]).max() > 0 and np.abs(dw[0]).max() > 0
    h = 1e-5                                                # (the level equation takes a negative albedo as well)
    up, _ = MS.ms_reference(_gas_model("IQU", albedo=h)[0], levels)
    um, _ = MS.ms_reference(_gas_model("IQU", albedo=-h)[0], levels)
    _check_fd(levels, [x[..., 2] for x in uwd], up, um, h, "uw albedo at a black surface")


def test_refuses_non_scattering_layer():
    mdl, lin = _gas_model("I")
    m2 = copy.deepcopy(mdl)
    m2.tau_rayl = mdl.tau_rayl.copy()
    m2.tau_rayl[:, 2] = 0.0
    with pytest.raises(NotImplementedError):
        MSL.ms_lin_segmented(m2, lin, [1, 3])
