"""The SurfaceSIF oracle (tests/sif_oracle.py) pinned three ways (CPU only):

1. the reference's own gates (test/test_sif.jl): j0-[0] = 2 SIF0 at m = 0; the layer is untouched at m = 1, over an RPV surface
   and for a zero table; for a thin Rayleigh column at vza = 0, 0.9 SIF / pi < dR < SIF / pi, Q and U change by less than 1e-8;
2. linearity: R(SIF0) - R(0) = sum_c 2 SIF0[c] G_c with G from a direct numpy solve of (I - r-+ R+-) y = e, to 1e-13 of the
   maximum (both sides are O(N) sums of products of the same O(1) operators in FP64: 1e-13 leaves a factor of several hundred
   over eps);
3. finite differences: the gas and albedo slots of rt_run_lin_sif against central differences of rt_run_sif, with the step and
   the bound of tests/test_oracle_thermal_lin.py (h = 1e-5 relative: truncation ~ 1e-10, round-off ~ 1e-11 of the function's
   scale, bound 1e-6 of the largest Jacobian element); the SIF slots are exact by linearity (difference quotient to 1e-12, the
   bound of the Planck slots there).

The GPU tests' source table SIF0[0, s] = a (1 + 0.3 s) with a = 0.1 is checked here to keep the SIF share of R between 0.1 and 10
times the solar part, so that no difference test of tests/test_gpu_sif.py loses more than a digit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
from oracle import vsm_oracle_raman as OR  # noqa: E402
import ms_oracle as MS  # noqa: E402
import sif_oracle as SO  # noqa: E402

S, L = 3, 3
GEO = (40.0, [30.0, 5.0], [0.0, 60.0])
H_REL = 1e-5
FD_BOUND = 1e-6
A_SIF = 0.1


def sif0(n=None, S_=S, a=A_SIF):
    """The table of the GPU tests: SIF0[0, s] = a (1 + 0.3 s); [S] or, with n, [n, S] with zero Q / U / V rows."""
    t = a * (1.0 + 0.3 * np.arange(S_))
    if n is None:
        return t
    out = np.zeros((n, S_))
    out[0] = t
    return out


def sif0_dot(S_=S):
    """Two derivative tables [2, S]: the shape (d/d amplitude, SIF0 / a) and a spectral slope."""
    return np.stack([1.0 + 0.3 * np.arange(S_), np.arange(S_) - 0.5 * (S_ - 1)])


def _gas_model(pol, l_trunc=9, albedo=0.2, scale=(1.0, 1.0), FT=np.float64):
    """The gas scene of tests/test_gpu_thermal_lin.py (S = 3 points, 3 layers, two gases)."""
    rng = np.random.default_rng(0)
    tau_rayl = np.tile(0.03 * np.ones(L), (S, 1))
    ga, gb = 10.0 ** rng.uniform(-2.5, -0.5, (S, L)), 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    om = O.build_model(pol, l_trunc, *GEO, tau_rayl=tau_rayl, tau_abs=scale[0] * ga + scale[1] * gb, depol=0.0279, albedo=albedo,
                       m_max=2, FT=FT)
    return om, OL.LinModel([ga, gb])


# ---- 1. the reference's gates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_injection_gates(pol):
    om, _ = _gas_model(pol)
    n = om.pol.n
    N = om.quad_points.Nquad * n
    layers, layers0 = [], []
    SO.rt_run_sif(om, sif0(), surface_layers=layers)
    SO.rt_run_sif(om, np.zeros(S), surface_layers=layers0)
    (j, r), (j_zero, r_zero) = layers[0], layers0[0]
    base = O.make_added_layer(np.float64, N, S)
    O.create_surface_layer_lambertian(om.albedo, base, 0, om.pol, om.quad_points, np.sum(om.tau_rayl + om.tau_abs, axis=1), np.float64)
    # m = 0: every Stokes-I row gains 2 SIF0, no other row and no other array changes
    d = j - base.j0_m
    assert np.allclose(d[:, 0::n], 2 * sif0()[:, None], rtol=1e-14, atol=0)
    for c in range(1, n):
        assert np.all(d[:, c::n] == 0)
    assert np.array_equal(r, base.r_mp)
    # a zero table and m = 1: untouched
    assert np.array_equal(j_zero, base.j0_m)
    assert np.all(layers[1][0] == 0) and np.array_equal(layers[1][0], layers0[1][0])
    # the dispatch table: a non-Lambertian surface is a no-op
    rpv = O.make_added_layer(np.float64, N, S)
    rpv.j0_m[...] = 0.7
    SO.inject(rpv, SO.sif_table(n, S, sif0()), 0, n, lambertian=False)
    assert np.all(rpv.j0_m == 0.7)
    SO.inject(rpv, SO.sif_table(n, S, sif0()), 1, n)
    assert np.all(rpv.j0_m == 0.7)
    SO.inject(rpv, SO.sif_table(n, S, sif0()), 0, n)
    assert np.allclose(rpv.j0_m[:, 0::n], 0.7 + 2 * sif0()[:, None])


def test_thin_rayleigh_magnitude():
    """test_sif.jl "(1/pi) SIF0 injection magnitude": tau_rayl = 0.025, vza = 0, SIF_I = 0.01."""
    tau = np.tile(np.full(L, 0.025 / L), (S, 1))
    om = O.build_model("IQU", 9, 40.0, [0.0], [0.0], tau_rayl=tau, depol=0.0279, albedo=0.05, m_max=2)
    R0, _ = O.rt_run(om)
    R1, _ = SO.rt_run_sif(om, np.full(S, 0.01))
    d = R1[0, 0] - R0[0, 0]
    assert np.all(0.9 * 0.01 / np.pi < d) and np.all(d < 0.01 / np.pi), d * np.pi / 0.01
    assert np.max(np.abs(R1[:, 1:] - R0[:, 1:])) < 1e-8


def test_zero_table_is_rt_run_bit_for_bit():
    om, _ = _gas_model("IQU")
    for a, b in zip(SO.rt_run_sif(om, np.zeros(S)), O.rt_run(om)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("pol,l_trunc", [("I", 9), ("IQU", 9), ("IQU", 33), ("IQUV", 25)])
def test_sif_share_of_the_gpu_scenes(pol, l_trunc):
    """a = 0.1: the SIF share of R lies between 0.1 and 10 times the solar part (largest elements, and every Stokes-I element)."""
    om, _ = _gas_model(pol, l_trunc)
    R0, _ = O.rt_run(om)
    R1, _ = SO.rt_run_sif(om, sif0())
    ratio = np.abs(R1 - R0)[:, 0] / np.abs(R0)[:, 0]
    print("SIF share / solar part (Stokes I): min %.3f max %.3f" % (ratio.min(), ratio.max()))
    assert 0.1 < ratio.min() and ratio.max() < 10.0
    assert 0.1 < np.abs(R1 - R0).max() / np.abs(R0).max() < 10.0


# ---- 2. linearity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", ["I", "IQU", "IQUV"])
def test_linearity_against_direct_solve(pol):
    om, _ = _gas_model(pol)
    n = om.pol.n
    tab = sif0(n)
    if n >= 3:
        tab[1] = 0.3 * tab[0]
        tab[2] = -0.2 * tab[0]          # a polarized emission: every component's response enters
    R0, T0 = O.rt_run(om)
    R1, T1 = SO.rt_run_sif(om, tab)
    Gu, Gd = SO.unit_response(om)
    for got, ref in ((R1 - R0, SO.combine(Gu, tab)), (T1 - T0, SO.combine(Gd, tab))):
        assert np.max(np.abs(ref)) > 0
        assert np.max(np.abs(got - ref)) <= 1e-13 * max(np.max(np.abs(R1)), np.max(np.abs(T1)))
    # doubling the table doubles the share
    R2, _ = SO.rt_run_sif(om, 2 * tab)
    assert np.max(np.abs((R2 - R0) - 2 * (R1 - R0))) <= 1e-13 * np.max(np.abs(R1))


def test_multisensor_level0_and_levels():
    om, _ = _gas_model("IQU")
    uw, dw = SO.ms_sif(om, [0, 1, 3], sif0())
    R, T = SO.rt_run_sif(om, sif0())
    assert np.max(np.abs(uw[0] - R)) <= 1e-14 * np.max(np.abs(R)) and np.max(np.abs(dw[0] - T)) <= 1e-14 * np.max(np.abs(T))
    uw0, dw0 = MS.ms_reference(om, [0, 1, 3])
    for l in range(3):          # every level sees the emission
        assert np.max(np.abs(uw[l] - uw0[l])) > 0.1 * np.max(np.abs(uw0[l]))
    # level Nz: the surface layer alone below -- the upwelling gains the emission itself, 2 SIF0 weight = SIF0 / pi, and what the
    # atmosphere sends back of it
    assert np.all(uw[2][:, 0] - uw0[2][:, 0] > sif0()[None, :] / np.pi)


RAMAN_SHIFTS = np.array([-5, -2, -1, 1, 3, 40, 0])      # the line table of tests/test_gpu_raman.py (40: never in band)
RAMAN_W_IE = np.array([0.004, 0.012, 0.02, 0.018, 0.007, 0.3, 0.009])
RAMAN_GEO = (35.0, [20.0, 50.0], [0.0, 60.0])


def raman_arrays(S_, L_=3, seed=11):
    """The scene of tests/test_gpu_raman.py::test_rt_run_rrs_end_to_end (its smallest shape: Stokes_IQU, l_trunc = 7, S = 24)."""
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L_), (S_, 1))
    tau_abs = (10.0 ** rng.uniform(-3, 0.3, (S_, 1))) * np.linspace(0.5, 1.5, L_)[None, :] / L_
    F0 = np.zeros((3, S_))
    F0[0] = 0.8 + 0.4 * rng.random(S_)
    return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=0.12, m_max=2), F0


def raman_oracle_model(S_, FT=np.float64):
    kw, F0 = raman_arrays(S_)
    om = O.build_model("IQU", 7, *RAMAN_GEO, FT=FT, **kw)
    om.varpi_cabannes = 0.96
    om.F0 = F0
    return om, OR.RRS(i_shift=RAMAN_SHIFTS, varpi_ie=RAMAN_W_IE, greek_raman=O.get_greek_rayleigh(6.0 / 7.0 * 0.5))


def test_raman_elastic_part_is_rt_run_sif():
    """The elastic fields of the RRS run do not know of the Raman lines: R, T = rt_run_sif of the same (Cabannes) model; the
    inelastic part changes with the source (the emission is Raman-scattered on its way up); a zero table is the run without."""
    S_ = 24
    om, rs = raman_oracle_model(S_)
    tab = sif0(S_=S_)
    out = SO.rt_run_rrs_sif(om, rs, tab)
    out0 = OR.rt_run_rrs(om, rs)
    R, T = SO.rt_run_sif(om, tab)
    assert np.max(np.abs(out[0] - R)) <= 1e-13 * np.max(np.abs(R)) and np.max(np.abs(out[1] - T)) <= 1e-13 * np.max(np.abs(T))
    assert np.max(np.abs(out[2] - out0[2])) > 1e-3 * np.max(np.abs(out0[2]))
    share = np.abs(out[0] - out0[0])[:, 0].max() / np.abs(out0[0])[:, 0].max()
    assert 0.1 < share < 10.0, share
    for a, b in zip(SO.rt_run_rrs_sif(om, rs, np.zeros(S_)), out0):
        assert np.array_equal(a, b)


# ---- 3. the linearized run -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["I", "IQU"])
def lin_run(request):
    pol = request.param
    om, lin = _gas_model(pol)
    return pol, om, lin, SO.rt_run_lin_sif(om, lin, sif0(), sif0_dot())


def test_lin_forward_part_and_slot_count(lin_run):
    pol, om, lin, (R, T, Rd, Td) = lin_run
    R0, T0 = SO.rt_run_sif(om, sif0())
    assert np.max(np.abs(R - R0)) <= 1e-13 * np.max(np.abs(R0)) and np.max(np.abs(T - T0)) <= 1e-13 * np.max(np.abs(T0))
    assert Rd.shape == R.shape + (5,) and Td.shape == Rd.shape
    # without the source: OL.rt_run_lin, bit for bit
    for a, b in zip(SO.rt_run_lin_sif(om, lin, np.zeros(S)), OL.rt_run_lin(om, lin)):
        assert np.array_equal(a, b)


def test_lin_gas_and_albedo_slots_match_central_differences(lin_run):
    pol, om, lin, (R, T, Rd, Td) = lin_run
    h = H_REL
    cases = [(dict(scale=(1 + h, 1.0)), dict(scale=(1 - h, 1.0)), 2 * h),
             (dict(scale=(1.0, 1 + h)), dict(scale=(1.0, 1 - h)), 2 * h),
             (dict(albedo=0.2 * (1 + h)), dict(albedo=0.2 * (1 - h)), 2 * h * 0.2)]
    for p, (kp, km, den) in enumerate(cases):
        Rp, Tp = SO.rt_run_sif(_gas_model(pol, **kp)[0], sif0())
        Rm, Tm = SO.rt_run_sif(_gas_model(pol, **km)[0], sif0())
        for an, fd, name in ((Rd[..., p], (Rp - Rm) / den, "R"), (Td[..., p], (Tp - Tm) / den, "T")):
            scale = np.abs(an).max()
            assert scale > 0
            err = np.abs(an - fd).max() / scale
            print("SIF lin oracle %s slot %d %s: |analytic - central difference| / max|analytic| = %.2e" % (pol, p, name, err))
            assert err <= FD_BOUND, (pol, p, name, err)
    # ... and the SIF share of those slots is there: they differ from the slots of the run without the source
    Rd0 = OL.rt_run_lin(om, lin)[2]
    for p in range(3):
        assert np.abs(Rd[..., p] - Rd0[..., p]).max() > 1e-2 * np.abs(Rd0[..., p]).max(), p


def test_lin_sif_slots_are_exact_by_linearity(lin_run):
    pol, om, lin, (R, T, Rd, Td) = lin_run
    R0, T0 = SO.rt_run_sif(om, sif0())
    for k, tab in enumerate(sif0_dot()):
        Rk, Tk = SO.rt_run_sif(om, sif0() + 0.5 * tab)
        assert np.max(np.abs((Rk - R0) / 0.5 - Rd[..., 3 + k])) <= 1e-12 * np.max(np.abs(Rd[..., 3 + k]))
        assert np.max(np.abs((Tk - T0) / 0.5 - Td[..., 3 + k])) <= 1e-12 * np.max(np.abs(Td[..., 3 + k]))
