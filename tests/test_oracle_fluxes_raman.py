"""CPU checks of the Raman flux oracle (tests/flux_raman_oracle.py): the statement-order prototype against the segmented walk,
the level-0 rule, the Lambertian identity of the elastic and of the inelastic field at the surface, the exact zeros above a black
surface and of a column without Raman lines, the budget rule, and the host-side refusals of vsm.CoreRTRaman.rt_run_fluxes."""
import dataclasses

import numpy as np
import pytest

import flux_raman_oracle as FRO
from oracle import vsm_oracle as O
from test_oracle_multisensor_raman import SHIFTS, W_IE, _column, _host_model

SEGMENTED_BOUND = 1e-8      # the bound the device has against the prototype
NZ = 5


@pytest.fixture(scope="module", params=["I", "IQU"])
def column(request):
    model, rs = _column(request.param)
    levels = list(range(NZ + 1))
    return model, rs, levels, FRO.fluxes_raman_reference(model, rs, levels)


@pytest.mark.parametrize("levels", [[2, 0, NZ, 2], None])
def test_reference_equals_segmented(column, levels):
    model, rs, all_levels, ref_all = column
    levels = all_levels if levels is None else levels
    ref = FRO.fluxes_raman_reference(model, rs, levels)
    seg = FRO.fluxes_raman_segmented(model, rs, levels)
    assert ref.levels == seg.levels == levels
    worst = 0.0
    for k in FRO.FIELDS:
        a, b = getattr(seg, k), getattr(ref, k)
        assert a.shape == b.shape == (len(levels), model.tau_rayl.shape[0])
        assert np.array_equal(b, getattr(ref_all, k)[levels]), k      # (each level's row does not depend on the others)
        sc = float(np.max(np.abs(b)))
        assert sc > 0, k
        worst = max(worst, float(np.max(np.abs(a - b))) / sc)
    print("fluxes_raman_segmented vs fluxes_raman_reference: %.2e" % worst)
    assert worst <= SEGMENTED_BOUND
    assert np.max(np.abs(ref_all.up_ie)) > 1e-4 * np.max(np.abs(ref_all.up))      # (the Raman field is there)


def test_budget_rule(column):
    model, rs, levels, ref = column
    assert ref.absorbed_ie.shape == ref.absorbed.shape == (NZ, model.tau_rayl.shape[0])
    assert np.array_equal(ref.absorbed_ie, ref.net_down_ie[:-1] - ref.net_down_ie[1:])
    assert np.array_equal(ref.surface_absorbed_ie, ref.net_down_ie[-1])
    assert np.array_equal(ref.net_down_ie, ref.down_diffuse_ie - ref.up_ie)
    part = FRO.fluxes_raman_reference(model, rs, [3, 1])
    assert part.absorbed is None and part.surface_absorbed is None and part.absorbed_ie is None and part.surface_absorbed_ie is None


def test_nothing_diffuse_enters_the_toa(column):
    _, _, _, ref = column
    for k in ("down_diffuse", "actinic_down_diffuse", "down_diffuse_ie", "actinic_down_diffuse_ie"):
        assert np.all(getattr(ref, k)[0] == 0), k
        assert np.max(np.abs(getattr(ref, k)[1])) > 0, k
    assert np.max(np.abs(ref.up_ie[0])) > 0


def unit_beam(model):
    """The same column under F0 = (1, 0, ..): the reference's Lambertian surface layer builds its beam term with pol.I0, not with
    F0, so the elastic identity at the surface holds for the unit beam alone; the inelastic one for any."""
    F0 = np.zeros_like(model.F0)
    F0[0] = 1
    return dataclasses.replace(model, F0=F0)


def test_lambertian_identity_at_the_surface(column):
    model, rs, _, ref = column
    alb = float(model.albedo)
    want_ie = alb * ref.down_diffuse_ie[NZ]      # (the spectrally varying beam)
    assert np.min(np.abs(want_ie)) > 0
    assert float(np.max(np.abs(ref.up_ie[NZ] - want_ie) / np.abs(want_ie))) <= 1e-12
    ref = FRO.fluxes_raman_reference(unit_beam(model), rs, [NZ])
    want = alb * (ref.down_direct[0] + ref.down_diffuse[0])
    e = float(np.max(np.abs(ref.up[0] - want) / np.abs(want)))
    want_ie = alb * ref.down_diffuse_ie[0]
    assert np.min(np.abs(want_ie)) > 0
    e_ie = float(np.max(np.abs(ref.up_ie[0] - want_ie) / np.abs(want_ie)))
    print("up[Nz] vs albedo (direct + diffuse)[Nz]: rel %.2e; up_ie[Nz] vs albedo down_diffuse_ie[Nz]: rel %.2e" % (e, e_ie))
    assert e <= 1e-12 and e_ie <= 1e-12


def test_black_surface_returns_nothing():
    model, rs = _column("IQU", albedo=0.0)
    ref = FRO.fluxes_raman_reference(model, rs, [NZ, 2])
    for k in ("up", "up_ie", "actinic_up", "actinic_up_ie"):
        assert np.all(getattr(ref, k)[0] == 0), k
        assert np.max(np.abs(getattr(ref, k)[1])) > 0, k
    assert np.max(np.abs(ref.down_diffuse_ie[0])) > 0


def test_no_raman_lines_no_inelastic_field():
    model, rs = _column("IQU", varpi_ie=np.zeros(len(W_IE)))
    for fn in (FRO.fluxes_raman_reference, FRO.fluxes_raman_segmented):
        res = fn(model, rs, list(range(NZ + 1)))
        for k in FRO.IE_FIELDS + ("absorbed_ie", "surface_absorbed_ie"):
            assert np.all(getattr(res, k) == 0), (fn.__name__, k)
        assert np.max(np.abs(res.up)) > 0


def test_rt_run_fluxes_refusals():
    """Checked on the host, before any device work: those of CoreRTRaman.rt_run_multisensor, with its exception types."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    assert vsm.CoreRTRaman.rt_run_fluxes is vsm.core_rt_flux_raman.rt_run_fluxes
    assert vsm.CoreRTRaman.RamanFluxResult is vsm.core_rt_flux_raman.RamanFluxResult
    assert issubclass(vsm.CoreRTRaman.RamanFluxResult, vsm.CoreRT.FluxResult)
    rs = vsm.CoreRTRaman.RRS(SHIFTS, W_IE, H.GreekCoefs(**vars(O.get_greek_rayleigh(0.5))))
    model = _host_model(vsm)
    for bad in ([-1], [0, 5], [1.5], [True], []):
        with pytest.raises(ValueError):
            vsm.CoreRTRaman.rt_run_fluxes(rs, model, bad)
    B = np.full((4, 2), 1e-3)
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRTRaman.rt_run_fluxes(rs, _host_model(vsm, sources=srcs), [1])
    for src in (H.SurfaceSIF(np.full(2, 1e-3)), H.SurfaceEmission(B_surface=np.full(2, 1e-3))):
        with pytest.raises(NotImplementedError):
            vsm.CoreRTRaman.rt_run_fluxes(rs, _host_model(vsm, sources=(H.SolarBeam(), src)))
    big = _host_model(vsm, pol="IQU", l_trunc=90)
    assert big.quad_points.Nquad * 3 > 128
    with pytest.raises(vsm.VSMError, match="128"):
        vsm.CoreRTRaman.rt_run_fluxes(rs, big, [1])
    with pytest.raises(vsm.VSMError, match="iBand"):
        vsm.CoreRTRaman.rt_run_fluxes(rs, model, [1], iBand=2)


# ---- the surface hook (tests/driver_surface_cases.py: the scenes of tests/test_gpu_driver_surfaces.py) ------------------------------
import driver_surface_cases as DS  # noqa: E402


@pytest.fixture(scope="module", params=DS.SHAPES, ids=lambda p: "%s_%d" % p)
def grid_scene(request):
    pol, l_trunc = request.param
    om = DS.oracle_model(pol, l_trunc)
    return om, FRO.fluxes_raman_reference(om, DS.oracle_rs(), DS.LEVELS)


def test_default_hook_is_the_lambertian_builder(grid_scene):
    om, base = grid_scene
    got = FRO.fluxes_raman_reference(om, DS.oracle_rs(), DS.LEVELS, surface=DS.lambertian_hook(om))
    seg = FRO.fluxes_raman_segmented(om, DS.oracle_rs(), DS.LEVELS)
    seg_h = FRO.fluxes_raman_segmented(om, DS.oracle_rs(), DS.LEVELS, surface=DS.lambertian_hook(om))
    for k in FRO.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(base, k)) and np.array_equal(getattr(seg_h, k), getattr(seg, k)), k


def test_degenerate_surfaces(grid_scene):
    """A constant BRDF and a constant albedo spectrum are the Lambertian surface: every field within 1e-13 of its largest value."""
    om, base = grid_scene
    for name, model, hook, _ in DS.degenerate_cases(om):
        got = FRO.fluxes_raman_reference(model, DS.oracle_rs(), DS.LEVELS, surface=hook)
        for k in FRO.FIELDS:
            assert DS.rel_max(getattr(got, k), getattr(base, k)) <= 1e-13, (name, k, DS.rel_max(getattr(got, k), getattr(base, k)))


def test_black_surface_is_far_from_the_lambertian_one(grid_scene):
    """Against a vacuous pass on the device: `up` and `up_ie` at the surface level differ by at least 0.1 of their largest value."""
    om, base = grid_scene
    blk = FRO.fluxes_raman_reference(DS.black(om), DS.oracle_rs(), DS.LEVELS)
    i = DS.LEVELS.index(DS.L)
    for k in ("up", "up_ie"):
        assert DS.rel_max(getattr(blk, k)[i], getattr(base, k)[i]) >= 0.1, k
