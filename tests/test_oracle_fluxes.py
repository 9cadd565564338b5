"""CPU checks of the flux oracle (tests/flux_oracle.py): conservation over ALL levels of a conservative column (levels 0 and Nz
included, which is where the level-0 convention shows), the Lambertian identity at the surface, the two statement orders, the
opaque isothermal column as a blackbody (pi B, 2 pi B), the budget identities, and the host-side validation of
vsm.CoreRT.rt_run_fluxes."""
import math

import numpy as np
import pytest

import flux_oracle as FO
from oracle import vsm_oracle as O
from test_oracle_multisensor import FLUX_SPREAD_BOUND, _host_model, conservative_model
from test_oracle_multisensor_thermal import SEGMENTED_BOUND, opaque_isothermal_column

QUANTITIES = ("up", "down_diffuse", "down_direct", "actinic_up", "actinic_down_diffuse", "actinic_direct", "net_down")


def absorbing_column(S=3, L=5, albedo=0.15, seed=1):
    """The oracle model of test_gpu_multisensor.py's `_pair` column: Stokes_IQU, l_trunc 9 (N = 27), five Rayleigh layers,
    absorption varying over the points, a Lambertian surface."""
    rng = np.random.default_rng(seed)
    kw = dict(tau_rayl=np.tile(np.linspace(0.3, 0.6, L) / L, (S, 1)), tau_abs=10.0 ** rng.uniform(-4, 0, (S, 1)) * np.full((1, L), 1.0 / L),
              depol=0.0279, albedo=albedo, m_max=2)
    model = O.build_model("IQU", 9, 40.0, [30.0, 0.0, 55.0], [0.0, 60.0, 120.0], **kw)
    assert model.quad_points.Nquad * model.pol.n == 27
    return model


@pytest.fixture(scope="module")
def absorbing():
    model = absorbing_column()
    levels = list(range(model.tau_rayl.shape[1] + 1))
    return model, levels, FO.level_vectors(model, levels)


def _spread(model, res):
    return float(np.max(np.max(res.net_down, axis=0) - np.min(res.net_down, axis=0))) / float(model.quad_points.mu0)


def test_conservative_column_net_flux_all_levels():
    model, _ = conservative_model()
    levels = list(range(model.tau_rayl.shape[1] + 1))          # 0 and Nz on purpose
    vec = FO.level_vectors(model, levels)
    res = FO.fluxes_from_vectors(model, levels, vec)
    spread = _spread(model, res)
    print("oracle net_down spread / (mu0 F0) over levels 0..Nz: %.3e" % spread)
    assert 0 < spread < FLUX_SPREAD_BOUND
    assert np.all(res.down_diffuse[0] == 0) and np.all(res.actinic_down_diffuse[0] == 0)
    np.testing.assert_allclose(res.down_direct[0], float(model.quad_points.mu0), rtol=1e-15)      # mu0 F0 enters the TOA
    assert _spread(model, FO.fluxes_segmented(model, levels)) < FLUX_SPREAD_BOUND
    # the bound is not vacuous: with rt_run_multisensor's level-0 dw (T at the bottom of the column) in the formula it breaks
    wrong = _spread(model, FO.fluxes_from_vectors(model, levels, vec, level0_dw=True))
    print("... with the level-0 dw of the multi-sensor run: %.3e" % wrong)
    assert wrong > 100 * FLUX_SPREAD_BOUND


def test_lambertian_identity_at_the_surface(absorbing):
    model, levels, vec = absorbing
    res = FO.fluxes_from_vectors(model, levels, vec)
    Nz = levels[-1]
    want = float(model.albedo) * (res.down_diffuse[Nz] + res.down_direct[Nz])
    e = float(np.max(np.abs(res.up[Nz] - want) / np.abs(want)))
    print("up[Nz] vs albedo (diffuse + direct)[Nz]: rel %.2e" % e)
    assert e <= 1e-13


def test_two_statement_orders(absorbing):
    model, levels, vec = absorbing
    ref = FO.fluxes_from_vectors(model, levels, vec)
    seg = FO.fluxes_segmented(model, levels)
    worst = 0.0
    for k in QUANTITIES + ("absorbed", "surface_absorbed"):
        a, b = getattr(seg, k), getattr(ref, k)
        sc = float(np.max(np.abs(getattr(ref, "down_direct" if k in ("absorbed", "surface_absorbed") else k))))
        worst = max(worst, float(np.max(np.abs(a - b))) / sc)
    print("fluxes_segmented vs fluxes_reference: %.2e" % worst)
    assert worst <= SEGMENTED_BOUND


def test_opaque_isothermal_column_is_a_blackbody():
    """The T-A7 bound (1e-3 on the ratio) for the hemispheric quantities: pi B up and down, 2 pi B actinic."""
    kw, geo, B = opaque_isothermal_column()
    model = O.build_model(*geo, **kw)
    L = model.tau_rayl.shape[1]
    levels = list(range(1, L))
    for fn in (FO.fluxes_reference, FO.fluxes_segmented):
        res = fn(model, levels, B_layer=B, solar=False)
        assert np.all(res.down_direct == 0) and np.all(res.actinic_direct == 0)
        dev = [float(np.max(np.abs(x / (f * math.pi * B[0][None, :]) - 1)))
               for x, f in ((res.up, 1), (res.down_diffuse, 1), (res.actinic_up, 2), (res.actinic_down_diffuse, 2))]
        print("%s: |F / (pi B) - 1| up %.2e down %.2e, |actinic / (2 pi B) - 1| up %.2e down %.2e" % ((fn.__name__,) + tuple(dev)))
        assert max(dev) <= 1e-3


def test_budget_identities(absorbing):
    model, levels, vec = absorbing
    res = FO.fluxes_from_vectors(model, levels, vec)
    qp = model.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    Nz = levels[-1]
    # level 0's dw vector is T at the bottom of the column: the diffuse downwelling at level Nz
    t_bottom = FO.quadrature(model, vec[0][1], mu * w)
    assert np.max(np.abs(res.down_diffuse[Nz] - t_bottom)) <= SEGMENTED_BOUND * np.max(np.abs(t_bottom))
    assert np.max(np.abs(t_bottom)) > 0
    mu0F0 = float(qp.mu0)
    total = res.absorbed.sum(axis=0) + res.surface_absorbed + res.up[0]
    assert res.absorbed.shape == (Nz, model.tau_rayl.shape[0])
    np.testing.assert_allclose(total, mu0F0, rtol=1e-13)
    assert np.all(res.absorbed >= -1e-12 * mu0F0) and np.all(res.surface_absorbed > 0)
    # a subset of the levels: no budget
    part = FO.fluxes_from_vectors(model, [3, 1], vec)
    assert part.absorbed is None and part.surface_absorbed is None
    assert np.array_equal(part.up, res.up[[3, 1]])


def test_rt_run_fluxes_argument_validation():
    """Checked on the host, before any device work: levels, sources."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    assert vsm.CoreRT.rt_run_fluxes is vsm.core_rt_flux.rt_run_fluxes
    model = _host_model(vsm)
    for bad in ([-1], [0, 5], [1.5], [True], []):
        with pytest.raises(ValueError):
            vsm.CoreRT.rt_run_fluxes(model, bad)
    B = np.full((4, 2), 1e-3)
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        with pytest.raises(vsm.VSMError, match="thermal=True"):
            vsm.CoreRT.rt_run_fluxes(_host_model(vsm, sources=srcs), [1])
        with pytest.raises(ValueError):
            vsm.CoreRT.rt_run_fluxes(_host_model(vsm, sources=srcs), [9], thermal=True)

    class OtherSource:
        pass
    for srcs, th in (((OtherSource(),), False), ((H.SolarBeam(), OtherSource()), True), ((), True)):
        with pytest.raises(vsm.VSMError):
            vsm.CoreRT.rt_run_fluxes(_host_model(vsm, sources=srcs), None, thermal=th)


# ---- the surface hook (tests/driver_surface_cases.py: the scenes of tests/test_gpu_driver_surfaces.py) ------------------------------
import driver_surface_cases as DS  # noqa: E402


@pytest.fixture(scope="module", params=DS.SHAPES, ids=lambda p: "%s_%d" % p)
def grid_scene(request):
    pol, l_trunc = request.param
    om = DS.oracle_model(pol, l_trunc)
    return om, FO.fluxes_reference(om, DS.LEVELS)


def test_default_hook_is_the_lambertian_builder(grid_scene):
    om, base = grid_scene
    got = FO.fluxes_reference(om, DS.LEVELS, surface=DS.lambertian_hook(om))
    for k in FO.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(base, k)), k
    with pytest.raises(ValueError):
        FO.level_vectors(om, DS.LEVELS, sif=np.ones(DS.S), surface=DS.lambertian_hook(om))


@pytest.mark.parametrize("aerosol", [False, True], ids=["rayleigh", "aerosol"])
def test_degenerate_surfaces_and_black_surface(aerosol):
    """A constant BRDF and a constant albedo spectrum are the Lambertian surface (1e-13 of each field's largest value); over a black
    surface `up` at the surface level differs by at least 0.1 (against a vacuous pass on the device; the aerosol scene is that of
    the linearized cells)."""
    for pol, l_trunc in DS.SHAPES:
        om = DS.oracle_model(pol, l_trunc, aerosol=aerosol)
        base = FO.fluxes_reference(om, DS.LEVELS)
        for name, model, hook, _ in DS.degenerate_cases(om):
            got = FO.fluxes_reference(model, DS.LEVELS, surface=hook)
            for k in FO.FIELDS:
                assert DS.rel_max(getattr(got, k), getattr(base, k)) <= 1e-13, (pol, name, k)
        blk = FO.fluxes_reference(DS.black(om), DS.LEVELS)
        i = DS.LEVELS.index(DS.L)
        assert DS.rel_max(blk.up[i], base.up[i]) >= 0.1, pol
