"""CPU checks of the oracle of the linearized multi-sensor run with thermal emission (tests/ms_thermal_lin_oracle.py)
against the pinned oracles: its forward part is ms_thermal_oracle.ms_total_reference, its level 0 thermal_lin_oracle's slot, its gas
and albedo Jacobians central differences of ms_total_reference, its Planck slots forward thermal multi-sensor runs, an opaque
isothermal column a blackbody in the Planck slots too, and the kernel's source-only formula the general one with zero operator
derivatives.

Bounds.  1e-12: the bound of test_oracle_multisensor_thermal.py (SEGMENTED_BOUND) for two statement orders of the same algebra.
Central differences: H_REL / FD_BOUND of test_oracle_thermal_lin.py (truncation ~ h^2 = 1e-10, round-off ~ eps / h = 1e-11 of the
function's scale; 1e-6 of the largest Jacobian element leaves four decades)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import ms_lin_oracle as MSL  # noqa: E402
import ms_oracle as MSO  # noqa: E402
import ms_thermal_lin_oracle as MTL  # noqa: E402
import ms_thermal_oracle as MST  # noqa: E402
import thermal_lin_oracle as TL  # noqa: E402
from test_oracle_multisensor_thermal import opaque_isothermal_column  # noqa: E402
from test_oracle_thermal_lin import FD_BOUND, H_REL  # noqa: E402

S, L = 3, 4
LEVELS = [2, 0, 4, 1]        # an interior level with a two-layer segment below it, level 0, level Nz, and a second interior level


def _model(pol, albedo=0.2, scale=1.0):
    rng = np.random.default_rng(5)
    tau_rayl = np.tile(np.array([0.02, 0.05, 0.08, 0.1]), (S, 1))
    ga = 10.0 ** rng.uniform(-2.0, -0.3, (S, L))
    mdl = O.build_model(pol, 9, 40.0, [30.0, 5.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=scale * ga, depol=0.0279, albedo=albedo,
                        m_max=2)
    return mdl, OL.LinModel([ga])                    # x = multiplicative scale of the gas: d tau_abs / dx = base


def _B():
    return 0.1 + 0.02 * np.arange(L)[:, None] * np.array([1.0, 2.0, 3.0])[None, :]


def _Bdot():
    Bd = np.stack([np.ones((L, S)), np.zeros((L, S)), 0.3 + 0.1 * np.arange(L)[:, None] * np.ones((1, S))])
    Bd[1, 2] = 1.0                                   # a uniform table, the unit table of layer 3, a gradient
    return Bd


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module", params=["I", "IQU"])
def run(request):
    pol = request.param
    mdl, lin = _model(pol)
    return pol, mdl, lin, {solar: MTL.ms_thermal_lin_total(mdl, lin, _B(), _Bdot(), LEVELS, solar=solar) for solar in (True, False)}


def test_forward_part_is_ms_total_reference(run):
    pol, mdl, lin, tot = run
    for solar in (True, False):
        ur, dr = MST.ms_total_reference(mdl, _B(), LEVELS, solar=solar)
        if not solar:     # the forward Lambertian layer keeps a beam term at F0 = 0 that the linearized builder does not
            m0 = dataclasses.replace(mdl, F0=np.zeros((mdl.pol.n, S), dtype=mdl.FT))
            us, ds = MSO.ms_reference(m0, LEVELS)
            ur, dr = [a - b for a, b in zip(ur, us)], [a - b for a, b in zip(dr, ds)]
        for i, l in enumerate(LEVELS):
            eu, ed = _rel(tot[solar][0][i], ur[i]), _rel(tot[solar][1][i], dr[i])
            print("ms thermal lin %s solar=%s level %d: forward part vs ms_total_reference uw %.2e dw %.2e" % (pol, solar, l, eu, ed))
            assert eu <= 1e-12 and ed <= 1e-12, (pol, solar, l, eu, ed)


def test_level0_is_rt_run_thermal_lin_plus_solar(run):
    pol, mdl, lin, tot = run
    th = TL.rt_run_thermal_lin(mdl, lin, _B(), _Bdot())
    so = OL.rt_run_lin(mdl, lin)
    i0 = LEVELS.index(0)
    P = so[2].shape[-1]
    assert th[2].shape[-1] == P + 3 and tot[True][2][i0].shape == th[2].shape
    ref = (so[0] + th[0], so[1] + th[1], th[2].copy(), th[3].copy())
    ref[2][..., :P] += so[2]
    ref[3][..., :P] += so[3]
    for k in range(4):
        assert _rel(tot[True][k][i0], ref[k]) <= 1e-12, (pol, k, _rel(tot[True][k][i0], ref[k]))
        assert _rel(tot[False][k][i0], th[k]) <= 1e-12, (pol, k)


@pytest.mark.parametrize("solar", [True, False], ids=["solar+thermal", "thermal"])
def test_gas_and_albedo_jacobians_match_central_differences(run, solar):
    """At an interior level (2, and 1), level Nz and level 0.  Thermal-only: ms_total_reference(solar=False) carries the forward
    Lambertian layer's beam term at F0 = 0, which the linearized surface builder (driven by F0) does not have; that
    term's own difference quotient (ms_reference at F0 = 0) is taken off, as test_gpu_thermal_lin.py does."""
    pol, mdl, lin, tot = run
    h = H_REL

    def fwd(**kw):
        m_ = _model(pol, **kw)[0]
        u, d = MST.ms_total_reference(m_, _B(), LEVELS, solar=solar)
        if not solar:
            us, ds = MSO.ms_reference(dataclasses.replace(m_, F0=np.zeros((m_.pol.n, S), dtype=m_.FT)), LEVELS)
            u, d = [a - b for a, b in zip(u, us)], [a - b for a, b in zip(d, ds)]
        return u, d
    cases = [(dict(scale=1 + h), dict(scale=1 - h), 2 * h), (dict(albedo=0.2 * (1 + h)), dict(albedo=0.2 * (1 - h)), 2 * h * 0.2)]
    for p, (kp, km, den) in enumerate(cases):
        (up, dp), (um, dm) = fwd(**kp), fwd(**km)
        for i, l in enumerate(LEVELS):
            for an, fd, name in ((tot[solar][2][i][..., p], (up[i] - um[i]) / den, "uw"),
                                 (tot[solar][3][i][..., p], (dp[i] - dm[i]) / den, "dw")):
                scale = np.abs(an).max()
                assert scale > 0, (l, p, name)
                err = np.abs(an - fd).max() / scale
                print("ms thermal lin %s solar=%s level %d slot %d %s: |analytic - central difference| / max|analytic| = %.2e"
                      % (pol, solar, l, p, name, err))
                assert err <= FD_BOUND, (pol, solar, l, p, name, err)


def test_planck_slots_are_forward_thermal_runs(run):
    """Slot P + k = ms_thermal_segmented with B := B_dot[k], the thermal part alone, solar source or not; the unit table of
    layer 3 gives that layer's weighting function (non-zero at every level, up or down or both)."""
    pol, mdl, lin, tot = run
    Bd = _Bdot()
    P = 2
    for k in range(len(Bd)):
        uk, dk = MST.ms_thermal_segmented(mdl, Bd[k], LEVELS)
        for i, l in enumerate(LEVELS):
            for solar in (True, False):
                eu, ed = _rel(tot[solar][2][i][..., P + k], uk[i]), _rel(tot[solar][3][i][..., P + k], dk[i])
                assert eu <= 1e-14 and ed <= 1e-14, (pol, k, l, eu, ed)
            assert max(np.abs(uk[i]).max(), np.abs(dk[i]).max()) > 0
    # layer 3 lies below level 2: its weighting function there is upwelling first of all
    i2 = LEVELS.index(2)
    assert np.abs(tot[True][2][i2][..., P + 1]).max() > np.abs(tot[True][3][i2][..., P + 1]).max()


def test_opaque_isothermal_column_planck_slot_is_one():
    """The blackbody test of test_oracle_multisensor_thermal.py for the Planck slots: with a uniform B_dot, d uw / dx = d dw / dx
    = B_dot at the interior levels of an opaque isothermal column (its bound, 1e-3 on the ratio; 7.7e-5 was observed there)."""
    kw, geo, B = opaque_isothermal_column()
    model = O.build_model(*geo, **kw)
    Lc = model.tau_rayl.shape[1]
    lin = OL.LinModel([np.asarray(kw["tau_abs"]).copy()])
    Bd = 0.4 * np.ones((1,) + B.shape)
    levels = list(range(1, Lc))
    uw, dw, uwd, dwd = MTL.ms_thermal_lin_segmented(model, lin, B, Bd, levels)
    for i, l in enumerate(levels):
        ru, rd = uwd[i][:, 0, :, -1] / 0.4, dwd[i][:, 0, :, -1] / 0.4
        print("Planck slot level %d: uw_dot/B_dot - 1 in [%.2e, %.2e], dw_dot/B_dot - 1 in [%.2e, %.2e]"
              % (l, ru.min() - 1, ru.max() - 1, rd.min() - 1, rd.max() - 1))
        assert np.allclose(ru, 1.0, atol=1e-3) and np.allclose(rd, 1.0, atol=1e-3), l


def test_source_only_formula_is_the_general_one_with_zero_operator_derivatives():
    rng = np.random.default_rng(11)
    S_, N, K = 3, 9, 4
    A, B = 0.9 * rng.uniform(0, 1, (S_, N, N)) / N, 0.9 * rng.uniform(0, 1, (1, N, N)) / N
    a, c = rng.uniform(0, 1, (S_, N)), rng.uniform(0, 1, (S_, N))
    ak, ck = rng.normal(0, 1, (K, S_, N)), rng.normal(0, 1, (K, S_, N))
    Z = np.zeros((K, S_, N, N))
    _, _, uwd, dwd = MSL.level_lin_push_through(np.float64, A, a, B, c, Z, ak, Z[:, :1], ck)
    u2, d2 = MTL.level_src_only(np.float64, A, B, ak, ck)
    assert _rel(u2, uwd) <= 1e-14 and _rel(d2, dwd) <= 1e-14
    # ... and it is the level equation itself, which is linear in (a, c)
    uw, dw = MSO.level_push_through(np.float64, A, ak[0], np.broadcast_to(B, A.shape), ck[0])
    assert _rel(u2[0], uw) <= 1e-14 and _rel(d2[0], dw) <= 1e-14


def test_api_source_validation():
    """Host only, before any device work: the linearized driver accepts SolarBeam and / or ThermalEmission (the level plan is
    made: the next complaint is about the levels) and rejects other source types and an empty source tuple.  A ThermalEmission
    that leaves B_layer_dot at None is a forward-only source and stays refused (tests/test_gpu_multisensor_thermal_lin.py runs
    one with an empty table [0, rows, nSpec])."""
    import vsmartmom_jl_amd as vsm
    from test_oracle_multisensor import _host_model
    H = vsm.host_model
    B = np.full((4, 2), 1e-3)

    class OtherSource:
        pass
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B, B_layer_dot=B[None]))):
        for bad in ([-1], [0, 5], [1.5], []):
            with pytest.raises(ValueError):
                vsm.CoreRTLin.rt_run_multisensor(_host_model(vsm, sources=srcs), None, 0, 0, 1, bad)
    for srcs in ((OtherSource(),), (H.SolarBeam(), H.ThermalEmission(B_layer=B), OtherSource()), ()):
        with pytest.raises(vsm.VSMError, match="ThermalEmission"):
            vsm.CoreRTLin.rt_run_multisensor(_host_model(vsm, sources=srcs), None, 0, 0, 1, [1])
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        with pytest.raises(vsm.VSMError, match="SolarBeam.*B_layer_dot"):
            vsm.CoreRTLin.rt_run_multisensor(_host_model(vsm, sources=srcs), None, 0, 0, 1, [1])
