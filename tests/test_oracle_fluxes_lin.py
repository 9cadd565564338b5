"""CPU checks of the oracle of the linearized flux run (tests/flux_lin_oracle.py) and of the host side of
vsm.CoreRTLin.rt_run_fluxes: (a) every field's Jacobian against central finite differences of flux_oracle.fluxes_reference (a gas
slot, the Lambertian albedo, an aerosol tau_ref slot, a Planck slot; interior levels, level Nz, level 0); (b) the budget identity
of the derivatives; (c) the albedo Jacobian of the net flux of a conservative column is the same at every level; (d) the host
validation of the driver.

Bounds.  FD_TOL = 2e-6 relative to the largest element of the difference quotient, the bound tests/test_oracle_multisensor_lin.py
uses for the same kind of difference (h = 1e-5).  The Planck slot is linear in B, its quotient has no truncation error; it keeps
the same bound."""
import numpy as np
import pytest

import flux_lin_oracle as FL
import flux_oracle as FO
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL
from test_oracle_multisensor import FLUX_SPREAD_BOUND, _host_model, conservative_model
from test_oracle_multisensor_lin import FD_TOL

S, L = 2, 4
LEVELS = [2, 0, 4, 3, 1]        # interior levels, level 0, level Nz


def _column(pol="I", scale=1.0, albedo=0.2):
    """Four Rayleigh + gas layers, l_trunc 3 (Nquad 4); x = multiplicative scale of the gas: d tau_abs / dx = base."""
    rng = np.random.default_rng(2)
    tau_rayl = np.tile(np.array([0.03, 0.05, 0.08, 0.1]), (S, 1))
    base = 10.0 ** rng.uniform(-2.0, -0.5, (S, L))
    mdl = O.build_model(pol, 3, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=scale * base, depol=0.0279, albedo=albedo, m_max=1)
    assert 3 <= mdl.quad_points.Nquad <= 4
    return mdl, OL.LinModel([base])


def _B():
    return 0.1 + 0.02 * np.arange(L)[:, None] * np.array([1.0, 2.0])[None, :]


def _Bdot():
    Bd = np.stack([np.ones((L, S)), np.zeros((L, S))])
    Bd[1, 2] = 1.0               # a uniform table and the unit table of layer 3 (a weighting function)
    return Bd


def _check_fd(levels, an, plus, minus, den, what, zero=()):
    """Every field and level: an = the oracle result, slot already picked per field by `an(field)`."""
    worst = 0.0
    for k in FO.FIELDS:
        a = an(k)
        fd = (getattr(plus, k) - getattr(minus, k)) / den
        for i, l in enumerate(levels):
            scale = np.abs(fd[i]).max()
            if scale == 0:         # a field this parameter cannot move: exact zeros both ways
                assert (k, l) in zero or k in zero, (what, k, l)
                assert np.all(a[i] == 0), (what, k, l)
                continue
            assert (k, l) not in zero and k not in zero, (what, k, l)
            err = np.abs(a[i] - fd[i]).max() / scale
            worst = max(worst, err)
            assert err <= FD_TOL, (what, k, l, err)
    print("%s: worst |analytic - central difference| / max|difference| over fields and levels = %.2e" % (what, worst))


LEVEL0_ZERO = {("down_diffuse", 0), ("actinic_down_diffuse", 0), ("down_direct", 0), ("actinic_direct", 0)}


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_gas_and_albedo_jacobians_match_finite_differences(pol):
    mdl, lin = _column(pol)
    res = FL.fluxes_lin(mdl, lin, LEVELS)
    assert res.up_dot.shape == (len(LEVELS), S, 2)
    h = 1e-5
    _check_fd(LEVELS, lambda k: getattr(res, k + "_dot")[..., 0], FO.fluxes_reference(_column(pol, scale=1 + h)[0], LEVELS),
              FO.fluxes_reference(_column(pol, scale=1 - h)[0], LEVELS), 2 * h, "gas slot " + pol, zero=LEVEL0_ZERO)
    _check_fd(LEVELS, lambda k: getattr(res, k + "_dot")[..., 1], FO.fluxes_reference(_column(pol, albedo=0.2 + h)[0], LEVELS),
              FO.fluxes_reference(_column(pol, albedo=0.2 - h)[0], LEVELS), 2 * h, "albedo slot " + pol,
              zero=LEVEL0_ZERO | {"down_direct", "actinic_direct"})
    # the forward part is flux_oracle's
    ref = FO.fluxes_segmented(mdl, LEVELS)
    for k in FO.FIELDS:
        assert np.abs(getattr(res, k) - getattr(ref, k)).max() <= 1e-12 * np.abs(getattr(ref, "down_direct")).max(), k


def test_aerosol_tau_ref_jacobian_matches_finite_differences():
    from test_oracle_lin import _aerosol_scene
    mdl, lin = _aerosol_scene("I", l_trunc=5)
    levels = [0, 1, 2, 3]
    res = FL.fluxes_lin(mdl, lin, levels)
    assert res.up_dot.shape[-1] == 9
    h = 1e-5
    e = np.zeros(7)
    e[0] = h
    # the aerosol is absent from the top layer: tau_sum above level 1 does not move, nor does anything at level 0 going down
    _check_fd(levels, lambda k: getattr(res, k + "_dot")[..., 0], FO.fluxes_reference(_aerosol_scene("I", e, l_trunc=5)[0], levels),
              FO.fluxes_reference(_aerosol_scene("I", -e, l_trunc=5)[0], levels), 2 * h, "aerosol tau_ref slot",
              zero=LEVEL0_ZERO | {("down_direct", 1), ("actinic_direct", 1)})


@pytest.mark.parametrize("solar", [True, False], ids=["solar+thermal", "thermal"])
def test_planck_slot_matches_finite_differences(solar):
    mdl, lin = _column("I")
    B, Bd = _B(), _Bdot()
    res = FL.fluxes_lin(mdl, lin, LEVELS, B=B, B_dot=Bd, solar=solar)
    assert res.up_dot.shape == (len(LEVELS), S, 2 + 2)
    h = 1e-4
    for k in range(2):
        _check_fd(LEVELS, lambda f: getattr(res, f + "_dot")[..., 2 + k], FO.fluxes_reference(mdl, LEVELS, B_layer=B + h * Bd[k], solar=solar),
                  FO.fluxes_reference(mdl, LEVELS, B_layer=B - h * Bd[k], solar=solar), 2 * h, "Planck slot %d solar=%s" % (k, solar),
                  zero=LEVEL0_ZERO | {"down_direct", "actinic_direct"})
    if solar:     # the gas slot of the sum of the two slots
        h = 1e-5
        _check_fd(LEVELS, lambda f: getattr(res, f + "_dot")[..., 0], FO.fluxes_reference(_column("I", scale=1 + h)[0], LEVELS, B_layer=B),
                  FO.fluxes_reference(_column("I", scale=1 - h)[0], LEVELS, B_layer=B), 2 * h, "gas slot, solar + thermal",
                  zero=LEVEL0_ZERO)


def test_budget_of_the_derivatives():
    """mu0 F0 = sum_l absorbed + surface_absorbed + up[0] does not depend on a parameter."""
    mdl, lin = _column("IQU")
    levels = list(range(L + 1))
    res = FL.fluxes_lin(mdl, lin, levels)
    assert res.absorbed_dot.shape == (L, S, 2) and res.surface_absorbed_dot.shape == (S, 2)
    total = res.absorbed_dot.sum(axis=0) + res.surface_absorbed_dot + res.up_dot[0]
    scale = np.abs(res.up_dot).max()
    print("budget of the derivatives: |sum| / max|up_dot| = %.2e" % (np.abs(total).max() / scale))
    assert np.abs(total).max() <= 1e-13 * scale
    assert np.all(res.down_diffuse_dot[0] == 0) and np.all(res.down_direct_dot[0] == 0)
    part = FL.fluxes_lin(mdl, lin, [3, 1])
    assert part.absorbed_dot is None and part.surface_absorbed_dot is None
    assert np.abs(part.up_dot - res.up_dot[[3, 1]]).max() <= 1e-12 * scale       # (another segmentation of the same column)


def test_conservative_column_albedo_jacobian_of_the_net_flux():
    """Nothing is absorbed in the column, so net_down is the same at every level (the forward spread: 2.07e-5 of mu0 F0, bound
    FLUX_SPREAD_BOUND) -- and so is its derivative with respect to the albedo.  The derivative field is itself a radiation field
    of the same layers (the response to a unit Lambertian source of strength down[Nz] at the surface), so the layers' truncation
    error reaches it in the same proportion: the same bound, relative to that source, max |up_dot[Nz]| of the albedo slot.
    Measured: 1.99e-5 beside the forward 2.07e-5 (both printed)."""
    model, _ = conservative_model()
    Nz = model.tau_rayl.shape[1]
    levels = list(range(Nz + 1))
    lin = OL.LinModel([np.zeros_like(model.tau_rayl)])       # (a gas slot that moves nothing; the albedo is slot 1)
    res = FL.fluxes_lin(model, lin, levels)
    nd = res.net_down_dot[..., 1]
    spread = float(np.max(nd.max(axis=0) - nd.min(axis=0))) / float(np.abs(res.up_dot[Nz][..., 1]).max())
    fwd = float(np.max(res.net_down.max(axis=0) - res.net_down.min(axis=0))) / float(model.quad_points.mu0)
    print("conservative column: net_down spread %.3e of mu0 F0; net_down_dot (albedo) spread %.3e of max|up_dot[Nz]|" % (fwd, spread))
    assert 0 < fwd < FLUX_SPREAD_BOUND
    assert 0 < spread < FLUX_SPREAD_BOUND
    assert np.abs(nd).max() > 0.1 * float(model.quad_points.mu0)      # (not vacuous: the derivative is of the order of the flux)


def test_rt_run_fluxes_lin_argument_validation():
    """Checked on the host, before any device work: levels, sources, N."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    assert vsm.CoreRTLin.rt_run_fluxes is vsm.core_rt_flux_lin.rt_run_fluxes
    assert issubclass(vsm.CoreRTLin.FluxLinResult, vsm.CoreRT.FluxResult)
    model = _host_model(vsm)
    lin = H.LinModel([np.full((2, 4), 1e-3)])
    run = lambda m, lv=None: vsm.CoreRTLin.rt_run_fluxes(m, lin, 0, 1, 1, lv)
    for bad in ([-1], [0, 5], [1.5], [True], []):
        with pytest.raises(ValueError):
            run(model, bad)
    B = np.full((4, 2), 1e-3)
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        with pytest.raises(vsm.VSMError, match="B_layer_dot"):
            run(_host_model(vsm, sources=srcs), [1])
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        run(_host_model(vsm, sources=(H.SolarBeam(), H.SurfaceSIF(np.full(2, 1e-3)))), [1])

    class OtherSource:
        pass
    for srcs in ((OtherSource(),), (H.SolarBeam(), OtherSource()), ()):
        with pytest.raises(vsm.VSMError):
            run(_host_model(vsm, sources=srcs))
    big = H.model_from_arrays(vsm.Architectures.GPU(0), "IQUV", 61, 40.0, [30.0], [0.0], tau_rayl=np.tile(np.full(4, 0.05), (2, 1)),
                              tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=0)
    assert big.quad_points.Nquad * 4 > 128
    with pytest.raises(vsm.VSMError, match="128"):
        run(big, [1])
    # the level call refuses its sizes before anything is launched, too
    with pytest.raises(vsm.VSMError):
        vsm._lib.call("vsm_level_flux_lin", __import__("torch").float64, 8, 1, 1, 65, 0, 0, *([None] * 2), 64, *([None] * 3), 64,
                      *([None] * 2), 64, 64, *([None] * 3), 2, None, None, __import__("ctypes").c_double(0.5), *([None] * 3), 0, None,
                      None)
