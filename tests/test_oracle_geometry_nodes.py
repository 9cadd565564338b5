"""CPU tests of the numpy oracles at geometries where a viewing angle shares the solar stream (tests/geometry_cases.py).

With vza == sza the two nodes merge (rt_set_streams.jl:25-47): Nquad is one smaller, i_mu0 sits inside the zero-weight tail and
a viewing row is the solar row.  The oracles are the reference of the GPU tests there (tests/test_gpu_geometry_nodes.py), so they
are pinned here first: every output finite, OL's Jacobians equal to central differences of OL's OWN forward part, and the
direct-beam table stated as explicit differences.

The direct beam.  The forward LambertianSurfaceScalar builder writes j0+ = I0 exp(-tau/mu0) at the solar rows
(lambertian_surface.jl:75); the linearized builder writes j0+ = 0 (lambertian_surface_lin.jl:107), and so do the Legendre / Spline
builders (lambertian_surface.jl:135,195).  Interaction with the surface adds j0+ to the composite J0+ unchanged, so with a view on
the solar node T(rt_run) - T(rt_run_lin) is exactly the postprocessed beam 1/(2 pi) I0 exp(-tau/mu0) at that view, and zero at every
other view.  "R, T of rt_run_lin equal rt_run's" (test_oracle_lin.test_lin_forward_part_equals_forward_run) holds for R always and
for T off the solar node only."""
import dataclasses

import numpy as np
import pytest

import geometry_cases as G
import ms_lin_oracle as MSL
import ms_oracle as MS
import ss_lin_oracle as SSL
import ss_oracle as SS
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL
from oracle import vsm_oracle_raman as OR

L_TRUNC = 9
POLS = ["I", "IQU"]
FD_TOL = 2e-6            # test_oracle_lin.test_jacobians_match_finite_differences: of the slot's maximum


def _finite(*arrays):
    for a in arrays:
        for x in (a if isinstance(a, (list, tuple)) else [a]):
            assert np.all(np.isfinite(np.asarray(x, dtype=np.float64)))


@pytest.mark.parametrize("case", list(G.CASES))
@pytest.mark.parametrize("FT", [np.float64, np.float32])
def test_stream_layout_of_the_cases(case, FT):
    """Nquad / imu0 / Nstreams of every case, in both precisions (`near` keeps two distinct nodes in Float32 too), and the node
    of every view: the views listed in EXPECT sit on the solar node, no other does."""
    for l_trunc in (9, 21, 33):
        qp = O.rt_set_streams_gausslegquad(l_trunc, G.CASES[case][0], G.CASES[case][1], O.polarization("I"), FT)
        G.check_streams(case, qp, l_trunc)
        rows = G.view_rows(case, qp)
        assert [i for i, r in enumerate(rows) if r == qp.imu0] == G.EXPECT[case][2]
        assert np.all(qp.wt_mu[qp.Nstreams:] == 0) and np.all(qp.wt_mu[:qp.Nstreams] > 0)
    if case == "near":
        d = abs(float(qp.qp_mu[rows[0]]) - float(qp.mu0))
        assert 0.5e-6 < d < 2e-6, d


@pytest.mark.parametrize("pol", POLS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_every_oracle_is_finite(case, pol):
    om = G.oracle_model(case, pol, L_TRUNC, G.scene(aerosol=True), aerosol=True)
    S, L = om.tau_rayl.shape
    _finite(*O.rt_run(om))
    hd = {}
    O.rt_run(om, hdrf=hd)
    _finite(hd["hdr"], hd["bhr_uw"], hd["bhr_dw"])
    _finite(*SS.rt_run_ss(om))
    levels = [0, 1, L]
    _finite(*MS.ms_reference(om, levels))
    _finite(*MS.ms_segmented(om, levels))
    B = 0.05 + 0.01 * np.arange(L)[:, None] * np.ones((1, S))
    _finite(*O.rt_run_thermal(om, B))
    kw, bases = G.gas_scene(S=3)
    og = G.oracle_model(case, pol, L_TRUNC, kw)
    lin = OL.LinModel(bases)
    _finite(*OL.rt_run_lin(og, lin))
    _finite(*SSL.rt_run_ss_lin(og, lin))
    _finite(*MSL.ms_lin_segmented(og, lin, levels))
    rs = OR.RRS(i_shift=np.array([-2, -1, 1, 2, 0]), varpi_ie=np.array([0.004, 0.012, 0.02, 0.018, 0.009]),
                greek_raman=O.get_greek_rayleigh(6.0 / 7.0 * 0.5))
    kw5 = G.scene(S=5)
    orr = G.oracle_model(case, pol, L_TRUNC, kw5)
    orr.varpi_cabannes = 0.96
    out = OR.rt_run_rrs(orr, rs)
    _finite(*out)
    assert np.max(np.abs(out[2])) > 0
    _finite(*SS.rt_run_ss_rrs(orr, rs))


def test_expdiff_neg_mu_is_the_references_statement():
    """O.expdiff_neg_mu(d, mi, mj) against the reference's expdiff_neg(d / mi, d / mj) (rt_helpers.jl:32-40).  On separated nodes
    (every pair of a 12-node Gauss-Legendre rule plus two viewing nodes, d over six decades) the two agree to the rounding of the
    statement itself: the exponent difference b - a of the statement carries one rounding of a and one of b, 2 eps max(a, b) / |b - a| <= 2 eps
    max(mi, mj) / |mi - mj| relative, which is the bound asserted; equal arguments give exactly zero; single-precision arrays take
    the reference's statement bit for bit."""
    mu = np.concatenate([O.gauleg(12, 0.0, 1.0)[0], [O.cosd(30.0), O.cosd(40.0)]])
    mi, mj = mu[:, None, None], mu[None, :, None]
    d = 10.0 ** np.linspace(-5, 1, 13)[None, None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        new, ref = O.expdiff_neg_mu(d, mi, mj), O.expdiff_neg(d / mi, d / mj)
    off = ~np.eye(len(mu), dtype=bool)
    assert np.all(new[~off] == 0) and np.all(ref[~off] == 0)
    eps = np.finfo(np.float64).eps
    bound = (4 + 2 * np.maximum(mi, mj) / np.abs(mi - mj + np.eye(len(mu))[:, :, None])) * eps
    rel = np.abs(new - ref) / np.abs(ref + np.eye(len(mu))[:, :, None])
    assert np.all(np.isfinite(ref[off])) and np.all(ref[off] != 0)
    assert np.all(rel[off] <= np.broadcast_to(bound, rel.shape)[off]), float(np.max(rel[off] / np.broadcast_to(bound, rel.shape)[off]))
    assert np.max(rel[off]) <= 100 * eps, float(np.max(rel[off]) / eps)     # (closest pair here: mu / dmu = 47, bound 98 eps; measured 35)
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        a32, r32 = O.expdiff_neg_mu(d.astype(f), mi.astype(f), mj.astype(f)), O.expdiff_neg(d.astype(f) / mi.astype(f), d.astype(f) / mj.astype(f))
    assert a32.dtype == f and np.array_equal(a32, r32)


def _lin(case, pol, **kw):
    skw, bases = G.gas_scene(**kw)
    return G.oracle_model(case, pol, L_TRUNC, skw), OL.LinModel(bases)


@pytest.mark.parametrize("pol", POLS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_lin_jacobians_match_central_differences_of_the_lin_forward_part(case, pol):
    """Central differences of OL.rt_run_lin's OWN R, T (h = 1e-5): O.rt_run is the wrong forward reference at a view on the
    solar node, where its T carries the direct beam and the linearized run's does not -- a difference of the beam's own
    derivative in the gas slots.

    `near`: the reference's statement expdiff_neg(dtau / mu_i, dtau / mu0) (elemental.jl:379, rt_helpers.jl:32-40) rounds its two
    exponents at eps(Float64) each, 8e-11 of their difference at two nodes 1.1e-6 apart; a central difference divides that by 2 h,
    4e-6 of the slot.  O.expdiff_neg_mu forms the exponent difference in double without that cancellation, and the case reads
    1.7e-8 like the others."""
    R, T, Rd, Td = OL.rt_run_lin(*_lin(case, pol))
    h = 1e-5
    for p, (kp, km) in enumerate([(dict(scale=(1 + h, 1.0)), dict(scale=(1 - h, 1.0))),
                                  (dict(scale=(1.0, 1 + h)), dict(scale=(1.0, 1 - h))),
                                  (dict(albedo=0.2 + h), dict(albedo=0.2 - h))]):
        Rp, Tp, _, _ = OL.rt_run_lin(*_lin(case, pol, **kp))
        Rm, Tm, _, _ = OL.rt_run_lin(*_lin(case, pol, **km))
        for an, fd, name in ((Rd[..., p], (Rp - Rm) / (2 * h), "R"), (Td[..., p], (Tp - Tm) / (2 * h), "T")):
            scale = np.abs(fd).max()
            assert scale > 0
            assert np.abs(an - fd).max() <= FD_TOL * scale, (case, pol, p, name, np.abs(an - fd).max() / scale)
    if G.EXPECT[case][2]:
        # against differences of O.rt_run the gas slots of T are off by the beam's derivative at the coincident view
        v = G.EXPECT[case][2][0]
        Tp, Tm = O.rt_run(_lin(case, pol, scale=(1 + h, 1.0))[0])[1], O.rt_run(_lin(case, pol, scale=(1 - h, 1.0))[0])[1]
        fd = (Tp - Tm) / (2 * h)
        assert np.abs(Td[v, 0, :, 0] - fd[v, 0]).max() > 0.1 * np.abs(Td[v, 0, :, 0]).max()


@pytest.mark.parametrize("pol", POLS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_beam_table_of_the_oracles(case, pol):
    """T(rt_run, LambertianSurfaceScalar) - T(rt_run_lin) = the postprocessed direct beam at the views on the solar node, zero
    elsewhere; R equal everywhere; the Legendre surface (a constant albedo written as one) has no beam either.  Multi-sensor
    level 0 follows its drivers."""
    om, lin = _lin(case, pol)
    R0, T0 = O.rt_run(om)
    R1, T1, _, _ = OL.rt_run_lin(om, lin)
    beam = G.direct_beam(om)
    assert np.min(beam[0]) > 1e-3
    on = G.EXPECT[case][2]
    tol = 1e-15
    assert np.max(np.abs(R0 - R1)) <= tol
    for v in range(len(om.vza)):
        want = beam if v in on else 0.0 * beam
        assert np.max(np.abs((T0[v] - T1[v]) - want)) <= tol, (case, pol, v)
    # Legendre / Spline: R as the scalar surface; its T lacks the beam too.  (Compared at m = 0 alone: for m > 0 that builder
    # also zeroes t++, lambertian_surface.jl:154 / :211, so its T holds the m = 0 term only -- another quirk, kept.)
    S = om.tau_rayl.shape[0]
    R2, _ = O.rt_run(dataclasses.replace(om, albedo=np.full(S, om.albedo)))
    assert np.max(np.abs(R2 - R0)) <= tol
    om0 = dataclasses.replace(om, m_max=0)
    T0m, T2m = O.rt_run(om0)[1], O.rt_run(dataclasses.replace(om0, albedo=np.full(S, om.albedo)))[1]
    for v in range(len(om.vza)):
        want = beam if v in on else 0.0 * beam
        assert np.max(np.abs((T0m[v] - T2m[v]) - want)) <= tol, (case, pol, v)
    uw, dw = MS.ms_reference(om, [0])
    assert np.array_equal(uw[0], R0) and np.array_equal(dw[0], T0)
    uwl, dwl, _, _ = MSL.ms_lin_segmented(om, lin, [0])
    assert np.max(np.abs(uwl[0] - R1)) <= tol and np.max(np.abs(dwl[0] - T1)) <= tol


def test_R_is_continuous_across_the_merge():
    """Moving the SZA by 1e-4 degrees splits the merged node again: R moves by O(1e-6) relative, not by a branch's worth."""
    kw = G.scene()
    for pol in POLS:
        R0, T0 = O.rt_run(G.oracle_model("sun_in_view", pol, L_TRUNC, kw))
        R1, T1 = O.rt_run(G.oracle_model("sun_in_view", pol, L_TRUNC, kw, sza=40.0001))
        assert np.max(np.abs(R1 - R0)) <= 1e-5 * np.max(np.abs(R0))
        off = [v for v in range(3) if v not in G.EXPECT["sun_in_view"][2]]
        assert np.max(np.abs(T1[off] - T0[off])) <= 1e-5 * np.max(np.abs(T0[off]))
