"""CPU checks of the thermal multi-sensor oracle (tests/ms_thermal_oracle.py): the segmented algorithm of core_rt_ms.py's thermal
slot against the statement-order reference, level 0 against O.rt_run_thermal, an opaque isothermal column as a blackbody at every
interior level (the reference's T-A7, test/test_thermal_emission.jl, generalised), the black non-emitting surface, and the
argument validation of rt_run_multisensor(..., thermal=...) on the host."""
import numpy as np
import pytest

import ms_oracle as MS
import ms_thermal_oracle as MT
from oracle import vsm_oracle as O
from test_oracle_multisensor import _column, _host_model, _rel_per_component

# the bound of test_oracle_multisensor.py::test_segmented_equals_reference
SEGMENTED_BOUND = 1e-12


def _B(model, rng):
    S, L = model.tau_rayl.shape
    return 0.05 + 0.1 * rng.random((L, S))


@pytest.mark.parametrize("kind", ["iqu_rayleigh_abs", "two_aerosols", "legendre_surface", "scalar_all_levels"])
def test_thermal_segmented_equals_reference(kind):
    model, levels = _column(kind, np.random.default_rng(7))
    B = _B(model, np.random.default_rng(8))
    ur, dr = MT.ms_thermal_reference(model, B, levels)
    us, ds = MT.ms_thermal_segmented(model, B, levels)
    assert len(ur) == len(us) == len(levels)
    Nz = model.tau_rayl.shape[1]
    for i, l in enumerate(levels):
        eu, ed = _rel_per_component(us[i], ur[i]), _rel_per_component(ds[i], dr[i])
        print("thermal %s level %d: segmented vs reference uw %.2e dw %.2e" % (kind, l, eu, ed))
        assert eu <= SEGMENTED_BOUND and ed <= SEGMENTED_BOUND, (kind, l, eu, ed)
        assert np.max(np.abs(dr[i])) > 0, (kind, l)
        # (uw at level Nz is what the surface reflects of the thermal field: zero only over a black surface)
        assert np.max(np.abs(ur[i])) > 0 or (l == Nz and np.all(np.asarray(model.albedo) == 0)), (kind, l)


@pytest.mark.parametrize("kind", ["iqu_rayleigh_abs", "two_aerosols", "legendre_surface"])
def test_thermal_level0_is_rt_run_thermal(kind):
    model, _ = _column(kind, np.random.default_rng(3))
    B = _B(model, np.random.default_rng(4))
    R, T = O.rt_run_thermal(model, B)
    assert np.max(np.abs(R)) > 0
    for fn in (MT.ms_thermal_reference, MT.ms_thermal_segmented):
        uw, dw = fn(model, B, [0])
        eu, ed = _rel_per_component(uw[0], R), _rel_per_component(dw[0], T)
        print("thermal %s level 0 (%s) vs rt_run_thermal: %.2e %.2e" % (kind, fn.__name__, eu, ed))
        assert eu <= SEGMENTED_BOUND and ed <= SEGMENTED_BOUND, (kind, fn.__name__, eu, ed)


def opaque_isothermal_column(L=5, S=3):
    """(oracle model kwargs, geometry, B [L, S]): tau_abs >= 10 per layer, weak Rayleigh in every layer, a black surface."""
    tau_abs = np.tile(np.array([10.0, 14.0, 20.0]), (L, 1)).T[:S] * np.linspace(1.0, 1.5, L)[None, :]
    kw = dict(tau_rayl=np.tile(np.full(L, 1e-3), (S, 1)), tau_abs=tau_abs, depol=0.03, albedo=0.0, m_max=2)
    geo = ("IQU", 9, 30.0, [0.0, 35.0, 60.0], [0.0, 60.0, 120.0])
    B = np.tile(np.array([0.7, 1.3, 2.1])[:S], (L, 1))
    return kw, geo, B


def test_opaque_isothermal_column_is_a_blackbody_at_interior_levels():
    """T-A7 at interior levels: with at least one opaque layer (tau >= 10: exp(-10) = 4.5e-5) above and below, the up- and the
    downwelling thermal radiance both equal B (atol 1e-3 on the ratio, test_gpu_thermal.py's T-A7 bound)."""
    kw, geo, B = opaque_isothermal_column()
    model = O.build_model(*geo, **kw)
    L = model.tau_rayl.shape[1]
    levels = list(range(1, L))
    for fn in (MT.ms_thermal_reference, MT.ms_thermal_segmented):
        uw, dw = fn(model, B, levels)
        for i, l in enumerate(levels):
            ru, rd = uw[i][:, 0, :] / B[0][None, :], dw[i][:, 0, :] / B[0][None, :]
            print("%s level %d: uw/B - 1 in [%.2e, %.2e], dw/B - 1 in [%.2e, %.2e]"
                  % (fn.__name__, l, ru.min() - 1, ru.max() - 1, rd.min() - 1, rd.max() - 1))
            assert np.allclose(ru, 1.0, atol=1e-3) and np.allclose(rd, 1.0, atol=1e-3), (fn.__name__, l)


def test_black_surface_reflects_no_thermal_radiance():
    """Level Nz above a black, non-emitting surface: the thermal uw is exactly 0, the thermal dw is not."""
    S, L = 2, 4
    model = O.build_model("IQU", 11, 40.0, [0.0, 25.0, 60.0], [0.0, 30.0, 90.0], tau_rayl=np.tile(np.full(L, 0.05), (S, 1)),
                          tau_abs=np.full((S, L), 0.3), depol=0.03, albedo=0.0, m_max=2)
    B = _B(model, np.random.default_rng(1))
    for fn in (MT.ms_thermal_reference, MT.ms_thermal_segmented):
        uw, dw = fn(model, B, [L])
        assert np.all(uw[0] == 0)
        assert np.min(dw[0][:, 0]) > 0


def test_total_is_solar_plus_thermal():
    model, levels = _column("iqu_rayleigh_abs", np.random.default_rng(7))
    B = _B(model, np.random.default_rng(8))
    us, ds = MS.ms_reference(model, levels)
    ut, dt = MT.ms_thermal_reference(model, B, levels)
    u, d = MT.ms_total_reference(model, B, levels)
    for i in range(len(levels)):
        assert np.array_equal(u[i], us[i] + ut[i]) and np.array_equal(d[i], ds[i] + dt[i])


def test_oracle_refuses_bad_levels_and_non_scattering_layers():
    model, _ = _column("scalar_all_levels", np.random.default_rng(0))
    B = _B(model, np.random.default_rng(0))
    for fn in (MT.ms_thermal_reference, MT.ms_thermal_segmented):
        with pytest.raises(ValueError):
            fn(model, B, [0, 7])
    tr = np.tile(np.full(4, 0.05), (2, 1))
    tr[:, 2] = 0.0
    m2 = O.build_model("I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=1)
    for fn in (MT.ms_thermal_reference, MT.ms_thermal_segmented):
        with pytest.raises(NotImplementedError):
            fn(m2, np.full((4, 2), 0.1), [1])


def test_api_thermal_argument_validation():
    """Host only, before any device work: thermal=True accepts SolarBeam and / or ThermalEmission (the level plan is made) and
    still rejects other source types; thermal=False and the Raman and linearized drivers keep refusing ThermalEmission."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    MSd = vsm.core_rt_ms
    B = np.full((4, 2), 1e-3)

    class OtherSource:
        pass
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        model = _host_model(vsm, sources=srcs)
        plan = MSd._validate(model, [1, 0, 4], thermal=True)
        assert plan.levels == [1, 0, 4] and plan.interior == [1] and plan.tops_at == [1, 4]
        for bad in ([-1], [0, 5], [1.5], []):
            with pytest.raises(ValueError):
                vsm.CoreRT.rt_run_multisensor(model, bad, thermal=True)
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRT.rt_run_multisensor(model, [1])
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRT.rt_run_multisensor(model, [1], thermal=False)
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRTRaman.rt_run_multisensor(None, model, [1])
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRTLin.rt_run_multisensor(model, None, 0, 0, 1, [1])
    for srcs in ((OtherSource(),), (H.SolarBeam(), H.ThermalEmission(B_layer=B), OtherSource()), ()):
        with pytest.raises(vsm.VSMError, match="ThermalEmission"):
            vsm.CoreRT.rt_run_multisensor(_host_model(vsm, sources=srcs), [1], thermal=True)
    assert MSd._validate(_host_model(vsm), [2], thermal=True).levels == [2]        # sources=None: SolarBeam
