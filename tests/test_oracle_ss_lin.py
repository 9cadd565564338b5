"""CPU tests that pin tests/ss_lin_oracle.py (the linearized single-scattering run, our own restatement: the reference has no such
driver) independently of the device: its forward part is ss_oracle.rt_run_ss exactly, and its derivative part is checked slot by
slot, in FP64, against central finite differences of ss_oracle.rt_run_ss at two step sizes h and h / 2.

Inputs: the viewing angles hold the SZA itself (the branch of a viewing row equal to the SZA row) and the gas scene has a layer
without scatterers (varpi = 0), so those branches are differentiated too.  F0[0] = 1 with a non-zero Q component: the linearized
surface builders weigh the direct beam with F0 where the forward builders use I0 = e1, so the surface terms are derivatives of the
forward run for F0[0] = 1 only (as in rt_run_lin).

Bounds.  The FD error is the order-2 truncation term: it must fall by about 4 from h to h / 2 (bound 0.3 on the ratio, as
test_oracle_ss.py uses for its order-2 remainder).  The difference at h / 2 relative to the array maximum was measured per slot
(MEASURED below; the ratio was 0.250 in every slot) and each slot is gated at ten times its own measured
value: one decade.  The truncation term differs by four decades between the slots (tau_ref 1.5e-5, n_r 5.6e-10 at the same h), so
one gate for all of them would check the small ones not at all."""
import numpy as np
import pytest

import ss_lin_oracle as SSL
import ss_oracle as SS
from oracle import vsm_oracle as O
from oracle import vsm_oracle_coxmunk as CM
from oracle import vsm_oracle_lin as OL

SZA = 35.0
VZA, VAZ = [20.0, 35.0, 50.0], [0.0, 60.0, 120.0]
# measured differences at h / 2 (worse of R and T, relative to the array maximum); gas slots h = 1e-3, aerosol slots h = 2e-3
MEASURED = {"gas a": 2.03e-8, "gas b": 2.84e-8, "aerosol tau_ref (tau)": 1.55e-5, "aerosol n_r (tau, varpi, Z)": 5.62e-10,
            "aerosol r_m (tau, varpi, Z)": 2.11e-7, "aerosol p0 (tau)": 1.32e-7,
            # the Cox-Munk scene: gas slot h = 1e-3, wind-speed slot h = 1e-2
            "gas over Cox-Munk": 9.26e-10, "wind speed": 2.29e-7}
ALBEDO_MEASURED = 1e-12    # R is linear in the albedo: rounding of the difference quotient only (measured 6e-14 .. 1e-12)
MARGIN = 10.0
RATIO = 0.3


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _f0(pn, S):
    F0 = np.zeros((pn, S))
    F0[0] = 1.0
    if pn > 1:
        F0[1] = np.linspace(-0.05, 0.05, S)
    return F0


def gas_scene(pol="IQU", S=4, L=3, albedo=0.3, scale=(1.0, 1.0), zero_layer=1):
    """Two gases (x_g = multiplicative scale of gas g's absorption), a Lambertian albedo, a layer without Rayleigh scattering."""
    rng = np.random.default_rng(5)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    if zero_layer is not None:
        tau_rayl[:, zero_layer] = 0.0
    base_a = 10.0 ** rng.uniform(-2.5, -0.7, (S, L))
    base_b = 10.0 ** rng.uniform(-2.5, -0.7, (S, L))
    base_b[:, 0] = 0.0
    om = O.build_model(pol, 7, SZA, list(VZA), list(VAZ), tau_rayl=tau_rayl, tau_abs=scale[0] * base_a + scale[1] * base_b,
                       depol=0.0075, albedo=albedo, m_max=2)
    om.F0 = _f0(om.pol.n, S)
    return om, OL.LinModel([base_a, base_b])


def aerosol_scene(pol="IQU", x=None):
    from test_oracle_lin import _aerosol_scene
    om, lin = _aerosol_scene(pol, x, l_trunc=7)
    om.vza, om.vaz = list(VZA), list(VAZ)
    om.F0 = _f0(om.pol.n, om.tau_rayl.shape[0])
    return om, lin


def fd_figures(an, run, h):
    """Largest difference between the analytic slot `an` = (Rdot_p, Tdot_p) and central differences of `run(x)` = (R, T) at steps
    h and h / 2, relative to the array maximum: (d_h, d_h2), the worse of R and T."""
    out = []
    for step in (h, h / 2):
        up, dn = run(step), run(-step)
        out.append(max(_rel(a, (u - d) / (2 * step)) for a, u, d in zip(an, up[:2], dn[:2])))
    return tuple(out)


def _check(name, an, run, h):
    assert np.max(np.abs(an[0])) > 0, name
    d1, d2 = fd_figures(an, run, h)
    print("%s: FD difference %.3e at h = %g, %.3e at h / 2 (ratio %.3f)" % (name, d1, h, d2, d2 / d1))
    assert d2 <= MARGIN * MEASURED[name], (name, d2)
    assert d2 <= RATIO * d1, (name, d1, d2)


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_forward_part_is_ss_oracle_exactly(pol):
    for om, lin in (gas_scene(pol), aerosol_scene(pol)):
        R, T, Rd, Td = SSL.rt_run_ss_lin(om, lin)
        ref = SS.rt_run_ss(om)
        assert np.array_equal(R, ref[0]) and np.array_equal(T, ref[1])
        assert Rd.shape == R.shape + (lin.n_layer_params + 1,) and Td.shape == Rd.shape


def test_gas_and_albedo_slots_match_finite_differences():
    om, lin = gas_scene()
    R, T, Rd, Td = SSL.rt_run_ss_lin(om, lin)
    h = 1e-3
    _check("gas a", (Rd[..., 0], Td[..., 0]), lambda e: SS.rt_run_ss(gas_scene(scale=(1 + e, 1.0))[0]), h)
    _check("gas b", (Rd[..., 1], Td[..., 1]), lambda e: SS.rt_run_ss(gas_scene(scale=(1.0, 1 + e))[0]), h)
    # the albedo enters linearly (the difference is rounding only: no order-2 term to halve) -- R only, T does not see it
    an = Rd[..., 2]
    up, dn = SS.rt_run_ss(gas_scene(albedo=0.3 + h)[0]), SS.rt_run_ss(gas_scene(albedo=0.3 - h)[0])
    d = _rel(an, (up[0] - dn[0]) / (2 * h))
    print("albedo: FD difference %.3e" % d)
    assert np.max(np.abs(an)) > 0 and d <= MARGIN * ALBEDO_MEASURED
    assert np.all(Td[..., 2] == 0)


@pytest.mark.parametrize("k,name", [(0, "tau_ref (tau)"), (1, "n_r (tau, varpi, Z)"), (3, "r_m (tau, varpi, Z)"), (5, "p0 (tau)")])
def test_aerosol_slots_match_finite_differences(k, name):
    om, lin = aerosol_scene()
    R, T, Rd, Td = SSL.rt_run_ss_lin(om, lin)
    assert Rd.shape[-1] == 9

    def run(e):
        x = np.zeros(7)
        x[k] = e
        return SS.rt_run_ss(aerosol_scene(x=x)[0])
    _check("aerosol " + name, (Rd[..., k], Td[..., k]), run, 2e-3)


def test_surface_slot_is_zero_above_the_surface_and_black_surface_keeps_it():
    """Per moment: the surface slot of J0+' is exactly zero; over a black surface the albedo slot of R is not (it is the
    radiance a unit albedo would add) and every gas slot is that of the atmosphere alone."""
    om, lin = gas_scene(albedo=0.0)
    per_m = []
    R, T, Rd, Td = SSL.rt_run_ss_lin(om, lin, per_m=per_m)
    for rec in per_m:
        assert np.all(rec["J0_p_dot"][-1] == 0)
    assert np.max(np.abs(Rd[..., 2])) > 0
    om3, _ = gas_scene(albedo=0.3)
    Rd3 = SSL.rt_run_ss_lin(om3, lin)[2]
    # R is affine in the albedo: Rdot_gas(a) = Rdot_gas(0) + a d(Rdot_albedo)/d gas, checked through the albedo slot's own FD
    h = 1e-3      # (order-2 truncation of this quotient: 3.2e-5 at h = 2e-2, so 8e-8 here; gate one decade above)
    ra = lambda e: SSL.rt_run_ss_lin(gas_scene(albedo=0.0, scale=(1 + e, 1.0))[0], lin)[2][..., 2]
    cross = (ra(h) - ra(-h)) / (2 * h)
    assert _rel(Rd3[..., 0] - Rd[..., 0], 0.3 * cross) <= 1e-6


def coxmunk_scene(scale=1.0, S=2, L=4):
    """One gas over a Cox-Munk ocean, F0 = e1 (the linearized Cox-Munk builder weighs the beam with all components of F0)."""
    rng = np.random.default_rng(3)
    tau_rayl = np.tile(np.full(L, 0.12 / L), (S, 1))
    g = rng.uniform(0.5, 1.5, (S, L)) * 0.02
    om = O.build_model("IQU", 7, SZA, list(VZA), list(VAZ), tau_rayl, tau_abs=scale * g, depol=0.03, m_max=3)
    return om, OL.LinModel([g])


def _brdf_fill(om, U):
    mu = om.quad_points.qp_mu.astype(np.float64)
    return lambda m, a, ts: CM.create_surface_layer_brdf(CM.reflectance(CM.CoxMunkSurface(U), om.pol.n, mu, m), a, m, om.pol,
                                                         om.quad_points, ts, om.FT)


def test_coxmunk_gas_and_wind_speed_slots_match_finite_differences():
    om, lin = coxmunk_scene()
    U = 5.0
    R, T, Rd, Td = SSL.rt_run_ss_lin(om, lin, surface=CM.CoxMunkSurface(U))
    ref = SS.rt_run_ss(om, surface=_brdf_fill(om, U))
    assert np.array_equal(R, ref[0]) and np.array_equal(T, ref[1])
    _check("gas over Cox-Munk", (Rd[..., 0], Td[..., 0]), lambda e: SS.rt_run_ss(coxmunk_scene(1 + e)[0], surface=_brdf_fill(om, U)), 1e-3)
    # the wind speed reaches R only: T's slot is exactly zero and T does not move
    assert np.all(Td[..., 1] == 0)
    run = lambda e: SS.rt_run_ss(om, surface=_brdf_fill(om, U + e))
    assert np.array_equal(run(1e-2)[1], T)
    _check("wind speed", (Rd[..., 1],), run, 1e-2)
