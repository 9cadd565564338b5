"""CPU checks of tests/surface_emission_oracle.py, the numpy oracle of SurfaceEmission, and of the source type's
constructor: the Kirchhoff emissivity of a Lambertian layer, the isothermal cavity (radiance and flux), a transparent column,
linearity in the skin table, the albedo slot against central differences of the forward oracle, the refusals.

Bounds.  The cavity: 1e-3, the bound of test_gpu_thermal.py's opaque isothermal column (the reference's own tolerance for the
single-scattering elemental layer).  Central differences: the step 1e-5 and the bound 1e-6 of test_oracle_thermal_lin.py."""
import dataclasses
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import flux_oracle as FO  # noqa: E402
import ms_thermal_oracle as MT  # noqa: E402
import surface_emission_oracle as SE  # noqa: E402

S, L = 3, 3
B0 = np.array([0.7, 1.3, 2.1])
H_REL = 1e-5
FD_BOUND = 1e-6
CAVITY_TOL = 1e-3


def _cavity(pol, albedo=0.3):
    """3 layers, the top one with an absorption optical depth >= 40 at every point."""
    tau_rayl = np.tile(np.array([0.05, 0.05, 0.05]), (S, 1))
    tau_abs = np.tile(np.array([40.0, 0.5, 0.8]), (S, 1)) * np.array([1.0, 1.2, 1.5])[:, None]
    return O.build_model(pol, 9, 40.0, [30.0, 5.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=albedo,
                         m_max=0)


def _rpv_surface(om):
    osurf = OB.RPVSurface(0.12, 0.08, 0.75, -0.25)
    mu = om.quad_points.qp_mu.astype(np.float64)
    pol, qp, FT = om.pol, om.quad_points, om.FT
    return lambda m, a, ts: CM.create_surface_layer_brdf(OB.reflectance(osurf, pol.n, mu, m), a, m, pol, qp, ts, FT)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("albedo", [0.0, 0.3, 1.0])
def test_lambertian_emissivity_is_one_minus_albedo(pol, albedo):
    """Gauss quadrature gives sum mu w = 1/2, so the row sums of the Lambertian r-+ over the I columns are the albedo in every I
    row, the zero-weight SZA / VZA rows included (the weights sit on the columns); Q, U rows emit nothing."""
    om = _cavity(pol, albedo)
    n, N = om.pol.n, om.quad_points.Nquad * om.pol.n
    assert np.any(np.asarray(om.quad_points.wt_mu) == 0)
    added = O.make_added_layer(om.FT, N, S)
    O.create_surface_layer_lambertian(albedo, added, 0, om.pol, om.quad_points, np.zeros(S), om.FT)
    eps = SE.emissivity_rows(added.r_mp, n)
    assert np.max(np.abs(eps[:, ::n] - (1 - albedo))) <= 4 * np.finfo(np.float64).eps
    for c in range(1, n):
        assert np.all(eps[:, c::n] == 0)
    j = SE.emission_vector(added.r_mp, n, B0)
    np.testing.assert_allclose(j[:, ::n], 2 * math.pi * B0[:, None] * (1 - albedo) * np.ones((1, N // n)), rtol=1e-15, atol=1e-15)
    je = SE.emission_vector(added.r_mp, n, B0, emissivity=0.25)
    np.testing.assert_allclose(je[:, ::n], 2 * math.pi * B0[:, None] * 0.25 * np.ones((1, N // n)), rtol=1e-15)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,pol", [("lambertian", "IQU"), ("rpv", "I")])
def test_cavity_radiance(kind, pol):
    """B_layer = B_surface = B0 under an opaque lid, no SolarBeam: uw / B0 = 1 at levels 0..Nz, dw / B0 = 1 at 1..Nz, Q = U = 0.
    Without the surface emission uw at level Nz is about albedo * B0 (Lambertian): the feature is what closes the cavity."""
    om = _cavity(pol)
    surface = _rpv_surface(om) if kind == "rpv" else None
    levels = [0, 1, 2, 3]
    Bl = np.tile(B0, (L, 1))
    if surface is None:            # the existing oracle's slot over the boundary that does not emit, plus the response
        ut, dt = MT.ms_thermal_reference(om, Bl, levels)
        ue, de = SE.emission_response(om, B0, levels)
    else:                          # (the thermal oracle builds Lambertian layers only: the response oracle walks the table too)
        ut, dt = SE.emission_response(om, np.zeros(S), levels, surface=surface, B_layer=Bl)
        ue, de = SE.emission_response(om, B0, levels, surface=surface)
    for i, l in enumerate(levels):
        uw, dw = ut[i] + ue[i], dt[i] + de[i]
        eu, ed = np.max(np.abs(uw[:, 0] / B0 - 1)), np.max(np.abs(dw[:, 0] / B0 - 1))
        print("cavity %s level %d: |uw/B0 - 1| %.2e  |dw/B0 - 1| %.2e" % (kind, l, eu, ed))
        assert eu <= CAVITY_TOL, (kind, l, eu)
        if l >= 1:
            assert ed <= CAVITY_TOL, (kind, l, ed)
        for c in range(1, om.pol.n):
            assert np.max(np.abs(uw[:, c] / B0)) <= CAVITY_TOL and np.max(np.abs(dw[:, c] / B0)) <= CAVITY_TOL
    if kind == "lambertian":       # the boundary that only reflects sends up about albedo * B0: nowhere near 1
        assert np.max(np.abs(ut[3][:, 0] / B0 - 0.3)) <= 0.01


def test_thermal_slot_total_is_the_existing_oracle_plus_the_response():
    """Linearity: ms_thermal_oracle's slot over the boundary that does not emit, plus the response, is the walk of both sources."""
    mdl, _ = _gas_model("IQU")
    Bl = 0.4 + 0.05 * np.arange(L)[:, None] + 0.01 * np.arange(S)[None, :]
    levels = [0, 1, 3, 1]
    ut, dt = MT.ms_thermal_reference(mdl, Bl, levels)
    ue, de = SE.emission_response(mdl, B0, levels)
    ua, da = SE.emission_response(mdl, B0, levels, B_layer=Bl)
    for i in range(len(levels)):
        assert np.max(np.abs(ut[i] + ue[i] - ua[i])) <= 1e-14 * np.abs(ua[i]).max()
        assert np.max(np.abs(dt[i] + de[i] - da[i])) <= 1e-14 * np.abs(da[i]).max()


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def test_cavity_fluxes_and_transparent_column():
    om = _cavity("IQU")
    levels = [0, 1, 2, 3]
    Bl = np.tile(B0, (L, 1))
    vec = SE.add_vectors(FO.level_vectors(om, levels, B_layer=Bl, solar=False), SE.level_vectors(om, levels, B0))
    res = FO.fluxes_from_vectors(om, levels, vec, solar=False)
    for l in (1, 2, 3):
        eu, ed = np.max(np.abs(res.up[l] / (math.pi * B0) - 1)), np.max(np.abs(res.down_diffuse[l] / (math.pi * B0) - 1))
        print("cavity flux level %d: up %.2e down %.2e" % (l, eu, ed))
        assert eu <= CAVITY_TOL and ed <= CAVITY_TOL
    assert np.max(np.abs(res.surface_absorbed / (math.pi * B0))) <= CAVITY_TOL
    # a transparent column over albedo a: the boundary alone emits, up[Nz] = pi (1 - a) B_s
    a = 0.3
    thin = O.build_model("IQU", 9, 40.0, [30.0], [0.0], tau_rayl=np.full((S, L), 1e-9), tau_abs=np.zeros((S, L)), depol=0.0279,
                         albedo=a, m_max=0)
    up = FO.fluxes_from_vectors(thin, [L], SE.level_vectors(thin, [L], B0), solar=False).up[0]
    assert np.max(np.abs(up / (math.pi * (1 - a) * B0) - 1)) <= 1e-6


# ---- (d), (e) ----------------------------------------------------------------------------------------------------------------------
def _gas_model(pol, albedo=0.2):
    rng = np.random.default_rng(5)
    tau_rayl = np.tile(np.array([0.02, 0.05, 0.1]), (S, 1))
    ga = 10.0 ** rng.uniform(-2.0, -0.3, (S, L))
    gb = 10.0 ** rng.uniform(-2.0, -0.3, (S, L))
    mdl = O.build_model(pol, 9, 40.0, [30.0, 5.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=ga + gb, depol=0.0279, albedo=albedo,
                        m_max=2)
    return mdl, OL.LinModel([ga, gb])


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_skin_slot_is_the_difference_quotient(pol):
    """The response is linear in B_surface: the skin slot equals (f(B_s + d dB) - f(B_s)) / d up to rounding, at every level."""
    mdl, lin = _gas_model(pol)
    levels = [0, 1, 3]
    dB = np.array([[0.3, -0.2, 0.5]])
    uw, dw, uwd, dwd = SE.emission_response_lin(mdl, lin, B0, levels, B_surface_dot=dB)
    u0, d0 = SE.emission_response(mdl, B0, levels)
    u1, d1 = SE.emission_response(mdl, B0 + 0.5 * dB[0], levels)
    for i in range(len(levels)):
        assert uwd[i].shape[-1] == 4
        np.testing.assert_allclose(uw[i], u0[i], rtol=0, atol=1e-13 * np.abs(u0[i]).max())
        for slot, f1, f0 in ((uwd[i][..., 3], u1[i], u0[i]), (dwd[i][..., 3], d1[i], d0[i])):
            assert np.abs(slot).max() > 0
            assert np.max(np.abs((f1 - f0) / 0.5 - slot)) <= 1e-12 * max(np.abs(f1).max(), np.abs(slot).max())


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_albedo_and_gas_slots_match_central_differences(pol):
    """Kirchhoff: d/d albedo reaches the response through the reflection AND through the emissivity (ap_J0- of the surface slot)."""
    mdl, lin = _gas_model(pol)
    levels = [0, 2, 3]
    _, _, uwd, dwd = SE.emission_response_lin(mdl, lin, B0, levels)
    h = H_REL
    up, dp = SE.emission_response(_gas_model(pol, 0.2 * (1 + h))[0], B0, levels)
    um, dm = SE.emission_response(_gas_model(pol, 0.2 * (1 - h))[0], B0, levels)
    for i, l in enumerate(levels):
        for an, fd, name in ((uwd[i][..., 2], (up[i] - um[i]) / (2 * h * 0.2), "uw"), (dwd[i][..., 2], (dp[i] - dm[i]) / (2 * h * 0.2), "dw")):
            scale = np.abs(an).max()
            assert scale > 0
            err = np.abs(an - fd).max() / scale
            print("surface emission albedo slot %s level %d %s: %.2e" % (pol, l, name, err))
            assert err <= FD_BOUND, (pol, l, name, err)
    # a gas slot: the propagation of the forward j0- alone
    ga = lin.tau_abs_dot[0]
    mp = dataclasses.replace(mdl, tau_abs=mdl.tau_abs + h * ga)
    mm = dataclasses.replace(mdl, tau_abs=mdl.tau_abs - h * ga)
    up, _ = SE.emission_response(mp, B0, levels)
    um, _ = SE.emission_response(mm, B0, levels)
    for i, l in enumerate(levels[:2]):
        an, fd = uwd[i][..., 0], (up[i] - um[i]) / (2 * h)
        assert np.abs(an).max() > 0 and np.abs(an - fd).max() / np.abs(an).max() <= FD_BOUND, (pol, l)


def test_explicit_emissivity_has_no_surface_derivative_of_its_own():
    """With a stated emissivity the albedo slot carries the reflection path alone: it differs from the Kirchhoff slot, and matches
    the central difference of the explicit-emissivity response."""
    mdl, lin = _gas_model("I")
    _, _, uk, _ = SE.emission_response_lin(mdl, lin, B0, [0])
    _, _, ue, _ = SE.emission_response_lin(mdl, lin, B0, [0], emissivity=0.8)
    assert np.abs(uk[0][..., 2] - ue[0][..., 2]).max() > 1e-3 * np.abs(uk[0][..., 2]).max()
    h = H_REL
    up, _ = SE.emission_response(_gas_model("I", 0.2 * (1 + h))[0], B0, [0], emissivity=0.8)
    um, _ = SE.emission_response(_gas_model("I", 0.2 * (1 - h))[0], B0, [0], emissivity=0.8)
    fd = (up[0] - um[0]) / (2 * h * 0.2)
    assert np.abs(ue[0][..., 2] - fd).max() <= FD_BOUND * np.abs(fd).max()


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    import vsmartmom_jl_amd as vsm
    H, VSMError = vsm.host_model, vsm._lib.VSMError
    nu = np.array([600.0, 900.0, 1100.0])
    se = H.SurfaceEmission(290.0, nu)
    np.testing.assert_array_equal(se.B_surface, H.planck_spectrum_wn(290.0, nu))
    assert se.emissivity is None and se.nSkin == 0
    assert H.SurfaceEmission(B_surface=B0, B_surface_dot=B0).nSkin == 1             # one [nSpec] table: nSkin = 1
    assert H.SurfaceEmission(B_surface=B0, B_surface_dot=np.ones((2, 3))).nSkin == 2
    np.testing.assert_array_equal(H.SurfaceEmission(B_surface=B0, emissivity=0.5).emissivity, np.full(3, 0.5))
    for bad in (dict(), dict(B_surface=np.ones((2, 3))), dict(B_surface=B0, emissivity=np.ones(2)),
                dict(B_surface=B0, emissivity=1.5), dict(B_surface=B0, emissivity=[0.2, -0.1, 0.3]),
                dict(B_surface=B0, emissivity=float("nan")), dict(B_surface=B0, B_surface_dot=np.ones((2, 4))),
                dict(B_surface=B0, B_surface_dot=np.ones((1, 2, 3)))):
        with pytest.raises(VSMError):
            H.SurfaceEmission(**bad)
    # a spectral length other than the model's
    model = type("M", (), dict(sources=(H.SurfaceEmission(B_surface=np.ones(4)),), tau_rayl=np.zeros((3, 2))))()
    with pytest.raises(VSMError):
        H.surface_emission_of(model)
    model.sources = (H.SurfaceEmission(B_surface=B0), H.SurfaceEmission(B_surface=B0))
    with pytest.raises(VSMError):
        H.surface_emission_of(model)
