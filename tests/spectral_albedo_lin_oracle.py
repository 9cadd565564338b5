"""Test oracle of the albedo Jacobians of the spectrally varying Lambertian surfaces: LambertianSurfaceLegendre (slot k =
d / d legendre_coeff[k], NSurf = K coefficients) and LambertianSurfaceSpline (slot k = d / d x_k for albedo_dot[k] = d albedo / d x_k).
numpy only; built on oracle/vsm_oracle.py, oracle/vsm_oracle_lin.py, tests/ss_lin_oracle.py, tests/ms_lin_oracle.py and
tests/brdf_lin_oracle.py (its small scene), which it imports and does not change.

The reference linearizes the scalar Lambertian surface only (lambertian_surface_lin.jl), so there is nothing to restate: the
derivative is that of the forward builder O.create_surface_layer_lambertian_spectral, which is LINEAR in the per-point albedo,

    albedo[s] = sum_k x_k basis[k, s]   =>   d (r-+, j0-)[.., s] / d x_k = (r-+, j0-) of the albedo basis[k, .]

and it is pinned by central differences of the forward oracle O.rt_run with the array albedo (tests/test_oracle_spectral_albedo_lin.py).
create_surface_layer_spectral_lin keeps the forward builder's blocks element for element (t++ = t-- = I at m = 0, EVERYTHING zero
for m > 0, j0+ = 0) and weighs the beam with F0[0, s] like the reference's two linearized builders; the layer slots carry
-j0- tau_sum_dot / mu0 as theirs do.

rt_run_lin is OL.rt_run_lin's walk, rt_run_ss_lin is ss_lin_oracle.rt_run_ss_lin's and ms_lin_segmented is ms_lin_oracle.ms_lin_segmented's,
each with the K-slot per-point builder in the surface step (their `surface=` hooks take ONE shared reflectance block per moment and
cannot state a per-point albedo, so the walks are restated here with P = n_layer_params + K).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import brdf_lin_oracle as B  # noqa: E402
import ms_lin_oracle as MSL  # noqa: E402
import ms_oracle as MSO  # noqa: E402
import ss_lin_oracle as SSL  # noqa: E402
import ss_oracle as SS  # noqa: E402


def legendre_basis(K: int, S: int, FT=np.float64) -> np.ndarray:
    """basis [K, S]: column k of the matrix O.legendre_albedo multiplies the coefficients with (its recurrence, applied to e_k)."""
    return np.stack([O.legendre_albedo(np.eye(K, dtype=FT)[k], S, FT) for k in range(K)])


def create_surface_layer_spectral_lin(albedo, basis, added: O.AddedLayer, al: OL.AddedLayerLin, isurf, m, pol, qp, tau_sum,
                                      tau_sum_dot, F0, FT):
    """The linearized per-point Lambertian surface layer with K = len(basis) albedo slots isurf .. isurf + K - 1 and the layer slots
    [0, tau_sum_dot.shape[1]).  Forward half: O.create_surface_layer_lambertian_spectral, j0- times F0[0, s] (exact at F0 = e1)."""
    basis = np.asarray(basis, dtype=FT)
    f0 = np.asarray(F0, dtype=FT)[0][:, None]
    O.create_surface_layer_lambertian_spectral(albedo, added, m, pol, qp, tau_sum, FT)
    added.r_pm[...] = 0
    added.j0_m[...] = added.j0_m * f0
    for arr in (al.ap_r_mp, al.ap_r_pm, al.ap_t_pp, al.ap_t_mm, al.ap_J0_p, al.ap_J0_m):
        arr[...] = 0
    if m > 0:
        return
    tsd = np.asarray(tau_sum_dot, dtype=FT)
    for p in range(tsd.shape[1]):
        al.ap_J0_m[p] = -added.j0_m * (tsd[:, p] / FT(qp.mu0))[:, None]
    S, N = added.j0_p.shape
    unit = O.make_added_layer(FT, N, S)
    for k in range(len(basis)):
        O.create_surface_layer_lambertian_spectral(basis[k], unit, m, pol, qp, tau_sum, FT)
        al.ap_r_mp[isurf + k] = unit.r_mp
        al.ap_J0_m[isurf + k] = unit.j0_m * f0


def _tsd(lins, S, pl, L):
    tsd = np.zeros((S, pl, L + 1))
    for iz in range(L):
        tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
    return tsd


def _copy_toa(cl, al):
    for a, b in ((cl.T_pp, al.ap_t_pp), (cl.T_mm, al.ap_t_mm), (cl.R_mp, al.ap_r_mp), (cl.R_pm, al.ap_r_pm), (cl.J0_p, al.ap_J0_p),
                 (cl.J0_m, al.ap_J0_m)):
        a[...] = b


def rt_run_lin(model: O.RTModel, lin: OL.LinModel, basis):
    """rt_run_lin.jl:102-326 over the per-point albedo model.albedo [S] with the K albedo slots of `basis` [K, S]: OL.rt_run_lin's
    walk with the K-slot builder.  Returns (R, T, Rdot, Tdot): [nVZA, nStokes, S] x 2, [nVZA, nStokes, S, P] x 2, P = pl + K."""
    FT, DT, pol, qp, S, L, N, F0 = MSO._setup(model)
    nV, pl, K = len(model.vza), lin.n_layer_params, len(basis)
    P = pl + K
    R, T = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    Rd, Td = np.zeros((nV, pol.n, S, P), dtype=FT), np.zeros((nV, pol.n, S, P), dtype=FT)
    added, added_s, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    al, als, cl = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S), OL.make_composite_layer_lin(FT, P, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = OL.layer_optics_lin(model, lin, lods, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = _tsd(lins, S, pl, L)
        for iz in range(L):
            lo = O.expand_optical_properties(lods[iz], FT)
            dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
            expk = np.exp(-dtau / FT(qp.mu0)).astype(FT)
            OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd, qp,
                             added, al, FT, DT)
            dall = np.zeros((S, P), dtype=FT)
            dall[:, :pl] = lins[iz].tau_dot / FT(2 ** nd)
            OL.doubling_lin(pol, expk, nd, added, al, dall, qp.mu0, pl, FT)
            if iz == 0:
                O.copy_added_to_composite(comp, added)
                _copy_toa(cl, al)
            else:
                OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
        create_surface_layer_spectral_lin(model.albedo, basis, added_s, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
        OL.interaction_lin(ifaces[-1], comp, cl, added_s, als, FT)
        O.postprocessing_vza(pol, comp, model.vza, model.vaz, qp, m, weight, R, T)
        MSL._vza_rows_lin(model, m, weight, cl.J0_m, cl.J0_p, Rd, Td)
    return R, T, Rd, Td


def rt_run_ss_lin(model: O.RTModel, lin: OL.LinModel, basis):
    """ss_lin_oracle.rt_run_ss_lin's walk with the K-slot per-point builder -> (R, T, Rdot, Tdot), P = pl + K."""
    FT, DT, pol, qp, S, L, N, F0 = MSO._setup(model)
    fill_surface = MSO._surface_fn(model, None)         # (the forward builder of the array albedo)
    nV, pl, K = len(model.vza), lin.n_layer_params, len(basis)
    P = pl + K
    R, T = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    Rd, Td = np.zeros((nV, pol.n, S, P), dtype=FT), np.zeros((nV, pol.n, S, P), dtype=FT)
    added, added_surf, added_sl = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    al, als = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S)
    comp = O.make_composite_layer(FT, N, S)
    Jd_p, Jd_m = np.zeros((P, S, N), dtype=FT), np.zeros((P, S, N), dtype=FT)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = SSL.layer_optics_lin(model, lin, lods, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = np.zeros((S, P, L + 1))                       # surface slots: zero in the atmosphere
        tsd[:, :pl, :] = _tsd(lins, S, pl, L)
        for iz in range(L):
            lo = O.expand_optical_properties(lods[iz], FT)
            tau_sum = tau_sum_all[:, iz].astype(FT)
            OL.elemental_lin(pol, tau_sum, tsd[:, :pl, iz], lo.tau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, 0, qp, added, al, FT, DT)
            if iz == 0:
                comp.J0_p[...], comp.J0_m[...] = added.j0_p, added.j0_m
                Jd_p[...], Jd_m[...] = al.ap_J0_p, al.ap_J0_m
            else:
                td = np.zeros((S, P))
                td[:, :pl] = lins[iz].tau_dot
                SSL.interaction_ss_lin(comp, Jd_p, Jd_m, added, al.ap_J0_p, al.ap_J0_m, tau_sum, tsd[:, :, iz], lo.tau, td, qp, FT)
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        create_surface_layer_spectral_lin(model.albedo, basis, added_sl, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :pl, -1], F0, FT)
        mu = qp.qp_muN.astype(FT)[None, :]
        es = np.exp(-tau_sum_all[:, -1].astype(FT)[:, None] / mu)
        for p in range(P):
            tsd_p = tsd[:, p, -1].astype(FT)[:, None]
            Jd_p[p] = Jd_p[p] + (als.ap_J0_p[p] - added_surf.j0_p * tsd_p / FT(qp.mu0))
            Jd_m[p] = Jd_m[p] + (als.ap_J0_m[p] - added_sl.j0_m * tsd_p / mu) * es
        SS.interaction_ss(comp, added_surf, tau_sum_all[:, -1], np.zeros(S, dtype=FT), qp, FT)
        O.postprocessing_vza(pol, comp, model.vza, model.vaz, qp, m, weight, R, T)
        MSL._vza_rows_lin(model, m, weight, Jd_m, Jd_p, Rd, Td)
    return R, T, Rd, Td


def ms_lin_segmented(model, lin, levels, basis):
    """ms_lin_oracle.ms_lin_segmented's algorithm with the K-slot per-point builder -> (uw, dw, uw_dot, dw_dot), lists over `levels`."""
    levels, Nz = MSO._check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, F0 = MSO._setup(model)
    nV, pl, K = len(model.vza), lin.n_layer_params, len(basis)
    P = pl + K
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    out = {l: (np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S, P), dtype=FT),
               np.zeros((nV, pol.n, S, P), dtype=FT)) for l in distinct}
    added, added_s = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    al, als = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = OL.layer_optics_lin(model, lin, lods, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = _tsd(lins, S, pl, L)
        layers = []
        comp, cl = O.make_composite_layer(FT, N, S), OL.make_composite_layer_lin(FT, P, N, S)
        tops = {}
        for iz in range(L):                              # 1. the top pass
            lo = O.expand_optical_properties(lods[iz], FT)
            dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
            expk = np.exp(-dtau / FT(qp.mu0)).astype(FT)
            OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd, qp,
                             added, al, FT, DT)
            dall = np.zeros((S, P), dtype=FT)
            dall[:, :pl] = lins[iz].tau_dot / FT(2 ** nd)
            OL.doubling_lin(pol, expk, nd, added, al, dall, qp.mu0, pl, FT)
            layers.append((MSO._copy_added(added), MSL._copy_lin(al)))
            if iz == 0:
                O.copy_added_to_composite(comp, added)
                _copy_toa(cl, al)
            else:
                OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
            if iz + 1 in interior or iz + 1 == Nz:
                tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy(), cl.R_pm.copy(), cl.J0_p.copy())
        create_surface_layer_spectral_lin(model.albedo, basis, added_s, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
        res = {}
        if Nz in distinct:                               # level Nz: the surface layer alone below
            A, a, Ad, ad = tops[Nz]
            res[Nz] = MSL.level_lin_push_through(FT, A, a, added_s.r_mp, added_s.j0_m, Ad, ad, als.ap_r_mp, als.ap_J0_m)
        bot = None
        ends = interior[1:] + [Nz]
        for l, end in reversed(list(zip(interior, ends))):   # 2./3. segments and bottoms from the surface up
            seg = O.CompositeLayer(*[x.copy() for x in (layers[l][0].R_mp, layers[l][0].R_pm, layers[l][0].T_pp, layers[l][0].T_mm,
                                                         layers[l][0].J0_p, layers[l][0].J0_m)])
            segl = MSL._copy_comp_lin(layers[l][1])
            for iz in range(l + 1, end):
                OL.interaction_lin(ifaces[iz], seg, segl, MSO._as_added(layers[iz][0]), MSL._as_added_lin(layers[iz][1]), FT)
            if bot is None:
                OL.interaction_lin(ifaces[-1], seg, segl, added_s, als, FT)
            else:
                OL.interaction_lin("11", seg, segl, MSO._as_added(bot[0]), MSL._as_added_lin(bot[1]), FT)
            bot = (seg, segl)
            A, a, Ad, ad = tops[l]
            res[l] = MSL.level_lin_push_through(FT, A, a, seg.R_mp, seg.J0_m, Ad, ad, segl.R_mp, segl.J0_m)   # 4. the level equation
        OL.interaction_lin(ifaces[-1], comp, cl, added_s, als, FT)
        res[0] = (comp.J0_m.copy(), comp.J0_p.copy(), cl.J0_m.copy(), cl.J0_p.copy())
        for l in distinct:
            uw, dw, uwd, dwd = res[l]
            MSO._vza_rows(model, m, weight, uw, dw, out[l][0], out[l][1])
            MSL._vza_rows_lin(model, m, weight, uwd, dwd, out[l][2], out[l][3])
    return tuple([out[l][i].copy() for l in levels] for i in range(4))


# ---- the small scene: brdf_lin_oracle's (3 layers, 4 points, N = 6 n_stokes, m = 0..3) over a three-coefficient Legendre albedo --------
COEFF = [0.25, 0.08, -0.03]
GEO, S_POINTS, N_LAYERS, M_MAX = B.GEO, B.S_POINTS, B.N_LAYERS, B.M_MAX
scene_arrays = B.scene_arrays


def oracle_scene(pol: str, coeff=COEFF, FT=np.float64):
    """(oracle model over the Legendre albedo of `coeff`, oracle lin model, basis [K, S]) of the small scene."""
    om, ol = B.oracle_scene(pol, FT)
    om.albedo = O.legendre_albedo(np.asarray(coeff, dtype=FT), S_POINTS, FT)
    return om, ol, legendre_basis(len(coeff), S_POINTS, FT)


def perturbed(coeff, k: int, h: float):
    c = [float(x) for x in coeff]
    c[k] += h
    return c


# The finite-difference floor of the TOA albedo Jacobians on the small scene: max over the K coefficient slots, R and T, Stokes_I and
# Stokes_IQU, of  max |central difference of O.rt_run - slot| / max |slot|  at FD_STEP.  Measured by
# tests/test_oracle_spectral_albedo_lin.py::test_toa_jacobian_against_central_differences (which asserts it) and reused, times 10, by
# the device's finite-difference tests.  The radiance is a rational function of the albedo (the reflections between the surface
# and the atmosphere are a geometric series in albedo x spherical albedo), so the quotient's truncation term h^2 f''' / 6 is two
# decades below brdf_lin_oracle.FD_FLOOR's and still two above the rounding term eps |R| / h ~ 1e-12: a property of the scene, the
# same on any machine.  Measured: R 1.499e-10, T 1.496e-10 (Stokes_IQU; Stokes_I 1.497e-10 / 1.493e-10).
FD_STEP = 1e-4
FD_FLOOR = 1.6e-10
