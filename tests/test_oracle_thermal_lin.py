"""The linearized thermal slot's oracle (tests/thermal_lin_oracle.py) against the pinned forward oracle: its forward part is
O.rt_run_thermal, its gas and albedo Jacobians are central differences of O.rt_run_thermal, its Planck slots are forward slots.

Bounds.  Central differences with a relative step h = 1e-5 carry a truncation error ~ h^2 = 1e-10 and a round-off ~ eps / h =
1e-11 of the function's scale: 1e-6 of the largest Jacobian element leaves four decades."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import thermal_lin_oracle as TL  # noqa: E402

S, L = 3, 3
H_REL = 1e-5
FD_BOUND = 1e-6


def _model(pol, albedo=0.2, scale=(1.0, 1.0)):
    rng = np.random.default_rng(5)
    tau_rayl = np.tile(np.array([0.02, 0.05, 0.1]), (S, 1))
    ga = 10.0 ** rng.uniform(-2.0, -0.3, (S, L))
    gb = 10.0 ** rng.uniform(-2.0, -0.3, (S, L))
    gb[:, 0] = 0.0                                   # gas b is absent from the top layer
    mdl = O.build_model(pol, 9, 40.0, [30.0, 5.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=scale[0] * ga + scale[1] * gb,
                        depol=0.0279, albedo=albedo, m_max=2)
    return mdl, OL.LinModel([ga, gb])                # x_g = multiplicative scale of gas g: d tau_abs / d x_g = base_g


def _B():
    return 0.1 + 0.02 * np.arange(L)[:, None] * np.array([1.0, 2.0, 3.0])[None, :]


@pytest.fixture(scope="module", params=["I", "IQU"])
def run(request):
    pol = request.param
    mdl, lin = _model(pol)
    return pol, mdl, lin, TL.rt_run_thermal_lin(mdl, lin, _B())


def test_forward_part_is_rt_run_thermal(run):
    pol, mdl, lin, (R, T, Rd, Td) = run
    R0, T0 = O.rt_run_thermal(mdl, _B())
    assert np.max(np.abs(R0)) > 0
    # (the same statements in the same order; the linearized surface builder's t-- = 0 feeds no source vector)
    assert np.max(np.abs(R - R0)) <= 1e-14 * np.max(np.abs(R0)) and np.max(np.abs(T - T0)) <= 1e-14 * np.max(np.abs(T0))
    assert Rd.shape == R.shape + (3,) and Td.shape == Rd.shape


def test_gas_and_albedo_jacobians_match_central_differences(run):
    pol, mdl, lin, (R, T, Rd, Td) = run
    h = H_REL
    cases = [(dict(scale=(1 + h, 1.0)), dict(scale=(1 - h, 1.0)), 2 * h),
             (dict(scale=(1.0, 1 + h)), dict(scale=(1.0, 1 - h)), 2 * h),
             (dict(albedo=0.2 * (1 + h)), dict(albedo=0.2 * (1 - h)), 2 * h * 0.2)]
    for p, (kp, km, den) in enumerate(cases):
        Rp, Tp = O.rt_run_thermal(_model(pol, **kp)[0], _B())
        Rm, Tm = O.rt_run_thermal(_model(pol, **km)[0], _B())
        for an, fd, name in ((Rd[..., p], (Rp - Rm) / den, "R"), (Td[..., p], (Tp - Tm) / den, "T")):
            scale = np.abs(an).max()
            assert scale > 0
            err = np.abs(an - fd).max() / scale
            print("thermal lin oracle %s slot %d %s: |analytic - central difference| / max|analytic| = %.2e" % (pol, p, name, err))
            assert err <= FD_BOUND, (pol, p, name, err)


def test_planck_slots_are_forward_slots(run):
    pol, mdl, lin, base = run
    Bd = np.stack([np.ones((L, S)), np.zeros((L, S))])
    Bd[1, 1] = 1.0                                   # a uniform table and the unit table of layer 2
    R, T, Rd, Td = TL.rt_run_thermal_lin(mdl, lin, _B(), Bd)
    assert Rd.shape[-1] == 5
    for a, b in zip((R, T, Rd[..., :3], Td[..., :3]), base):
        assert np.array_equal(a, b)                  # the earlier slots do not know of the Planck block
    for k in range(2):
        Rk, Tk = O.rt_run_thermal(mdl, Bd[k])
        assert np.max(np.abs(Rd[..., 3 + k] - Rk)) <= 1e-14 * np.max(np.abs(Rk))
        assert np.max(np.abs(Td[..., 3 + k] - Tk)) <= 1e-14 * np.max(np.abs(Tk))
    # linear in B: the analytic derivative is also the difference quotient, exactly up to rounding
    R2, T2 = O.rt_run_thermal(mdl, _B() + 0.5 * Bd[1])
    R0, T0 = O.rt_run_thermal(mdl, _B())
    assert np.max(np.abs((R2 - R0) / 0.5 - Rd[..., 4])) <= 1e-12 * np.max(np.abs(Rd[..., 4]))


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_elemental_source_derivative_matches_central_differences(pol):
    rng = np.random.default_rng(2)
    p_ = O.polarization(pol)
    qp = O.rt_set_streams_gausslegquad(9, 40.0, [30.0, 5.0], p_, np.float64)
    n = 5
    dtau, varpi, B = 10.0 ** rng.uniform(-4, 0, n), rng.uniform(0.0, 1.0, n), rng.uniform(0.5, 2.0, n)
    td, wd = rng.standard_normal((n, 2)) * dtau[:, None], 0.1 * rng.standard_normal((n, 2))
    j, jd = TL.thermal_source_lin(p_, qp, dtau, varpi, B, td, wd, np.float64)
    assert np.array_equal(j, O.thermal_source(p_, qp, dtau, varpi, B, np.float64))
    assert np.all(jd[:, :, 0::p_.n][:, :, qp.qp_mu > O.eps(np.float64)] != 0)
    if p_.n > 1:
        assert np.all(jd[:, :, 1::p_.n] == 0) and np.all(jd[:, :, 2::p_.n] == 0)
    h = 1e-5
    for p in range(2):
        jp = O.thermal_source(p_, qp, dtau + h * td[:, p], varpi + h * wd[:, p], B, np.float64)
        jm = O.thermal_source(p_, qp, dtau - h * td[:, p], varpi - h * wd[:, p], B, np.float64)
        fd = (jp - jm) / (2 * h)
        assert np.abs(jd[p] - fd).max() <= FD_BOUND * np.abs(jd[p]).max(), p
