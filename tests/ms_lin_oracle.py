"""Test oracle of the linearized multi-sensor run (vsm.CoreRTLin.rt_run_multisensor, core_rt_ms_lin.py), built on
oracle/vsm_oracle_lin.py, oracle/vsm_oracle_coxmunk.py and tests/ms_oracle.py, which it imports and does not change.

The reference has no linearized multi-sensor driver, so this is our own restatement: the segmented algorithm of ms_oracle.ms_segmented
on the linearized layers and composites of vsm_oracle_lin (elemental_lin, doubling_lin, interaction_lin and the linearized surface
builders, statement for statement as OL.rt_run_lin / CM.rt_run_lin walk them), with the derivative of the level equation.  Central
finite differences of ms_oracle.ms_reference (the prototype's transcription) anchor it (tests/test_oracle_multisensor_lin.py).

ms_lin_segmented(model, lin, levels, surface=None, full=None)
    -> (uw, dw, uw_dot, dw_dot): lists in the order of `levels`, [nVZA, nStokes, S] and [nVZA, nStokes, S, P].
level_lin_push_through(FT, A, a, B, c, Ad, ad, Bd, cd)
    the device's form: dw = M^-1 (a + A c), uw = c + B dw; q_p = c'_p + B'_p dw, dw'_p = M^-1 (a'_p + A'_p uw + A q_p),
    uw'_p = q_p + B dw'_p (M = I - A B).
level_lin_explicit(FT, A, a, B, c, Ad, ad, Bd, cd)
    the explicit derivative of interlayer_flux_helper! (interlayer_flux.jl:1-19): both inverses and their derivatives.

`surface`: None = the model's Lambertian albedo (create_surface_layer_lambertian_lin); else a CM.CoxMunkSurface (the linearized
Cox-Munk builder with the oracle's reflectance and its wind-speed derivative) or a function m -> (rho_m, drho_m) that supplies the
reflectance blocks to that builder.  The surface slot is the last (P - 1).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402

import ms_oracle as MSO  # noqa: E402


def _mvp(A, v):
    """[P, S, N, N] x [S, N] -> [P, S, N]"""
    return np.einsum("psij,sj->psi", A, v)


def level_lin_push_through(FT, A, a, B, c, Ad, ad, Bd, cd):
    """(uw, dw, uw_dot, dw_dot): A / B [S, N, N] (B may be [1, N, N]), a / c [S, N], Ad / Bd [P, S | 1, N, N], ad / cd [P, S, N]."""
    N = A.shape[-1]
    B = np.broadcast_to(B, A.shape)
    Bd = np.broadcast_to(Bd, (Bd.shape[0],) + A.shape)
    uw, dw = MSO.level_push_through(FT, A, a, B, c)
    M = np.eye(N, dtype=FT)[None] - A @ B
    q = cd + _mvp(Bd, dw)
    r = ad + _mvp(Ad, uw) + np.einsum("sij,psj->psi", A, q)
    dwd = np.stack([np.linalg.solve(M, r[p][..., None])[..., 0] for p in range(r.shape[0])]).astype(FT)
    uwd = (q + np.einsum("sij,psj->psi", B, dwd)).astype(FT)
    return uw, dw, uwd, dwd


def level_lin_explicit(FT, A, a, B, c, Ad, ad, Bd, cd):
    """interlayer_flux_helper!'s two-inverse formula and its derivative:
        dw = X (a + A c),  X = (I - A B)^-1,  X' = X (A' B + A B') X
        uw = Y (c + B a),  Y = (I - B A)^-1,  Y' = Y (B' A + B A') Y"""
    N = A.shape[-1]
    B = np.broadcast_to(B, A.shape)
    Bd = np.broadcast_to(Bd, (Bd.shape[0],) + A.shape)
    I = np.eye(N, dtype=FT)[None]
    mv = O._mv
    X = O.batch_inv(I - A @ B).astype(FT)
    Y = O.batch_inv(I - B @ A).astype(FT)
    dsrc, usrc = a + mv(A, c), c + mv(B, a)
    dw, uw = mv(X, dsrc), mv(Y, usrc)
    dwd, uwd = [], []
    for p in range(Ad.shape[0]):
        Xd = X @ (Ad[p] @ B + A @ Bd[p]) @ X
        Yd = Y @ (Bd[p] @ A + B @ Ad[p]) @ Y
        dwd.append(mv(Xd, dsrc) + mv(X, ad[p] + mv(Ad[p], c) + mv(A, cd[p])))
        uwd.append(mv(Yd, usrc) + mv(Y, cd[p] + mv(Bd[p], a) + mv(B, ad[p])))
    return uw, dw, np.stack(uwd), np.stack(dwd)


def _copy_lin(al) -> OL.CompositeLayerLin:
    return OL.CompositeLayerLin(al.ap_r_mp.copy(), al.ap_r_pm.copy(), al.ap_t_pp.copy(), al.ap_t_mm.copy(), al.ap_J0_p.copy(),
                                al.ap_J0_m.copy())


def _copy_comp_lin(cl) -> OL.CompositeLayerLin:
    return OL.CompositeLayerLin(*[x.copy() for x in (cl.R_mp, cl.R_pm, cl.T_pp, cl.T_mm, cl.J0_p, cl.J0_m)])


def _as_added_lin(cl) -> OL.AddedLayerLin:
    return OL.AddedLayerLin(cl.R_mp, cl.T_pp, cl.R_pm, cl.T_mm, cl.J0_p, cl.J0_m)


def _vza_rows_lin(model, m, weight, uwd, dwd, uw_out, dw_out):
    """postprocessing_vza_lin!'s rows: [P, S, N] vectors -> [nVZA, nStokes, S, P] (+=)."""
    for p in range(uwd.shape[0]):
        u, d = np.zeros(uw_out.shape[:3], dtype=uw_out.dtype), np.zeros(dw_out.shape[:3], dtype=dw_out.dtype)
        MSO._vza_rows(model, m, weight, uwd[p], dwd[p], u, d)
        uw_out[..., p] += u
        dw_out[..., p] += d


def ms_lin_segmented(model, lin, levels, surface=None, full=None):
    """The linearized multi-sensor run: (uw, dw, uw_dot, dw_dot), lists in the order of `levels`.  full: a dict that receives
    {(level, m): (uw [S, N], dw [S, N], uw_dot [P, S, N], dw_dot [P, S, N])}."""
    levels, Nz = MSO._check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, F0 = MSO._setup(model)
    nV = len(model.vza)
    pl = lin.n_layer_params
    P = pl + 1
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    out = {l: (np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S, P), dtype=FT),
               np.zeros((nV, pol.n, S, P), dtype=FT)) for l in distinct}
    added, added_s = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    al, als = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S)
    mu = qp.qp_mu.astype(np.float64)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = OL.layer_optics_lin(model, lin, lods, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = np.zeros((S, pl, L + 1))
        for iz in range(L):
            tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
        layers = []
        comp, cl = O.make_composite_layer(FT, N, S), OL.make_composite_layer_lin(FT, P, N, S)
        tops = {}
        for iz in range(L):                              # 1. the top pass (OL.rt_run_lin's walk)
            lo = O.expand_optical_properties(lods[iz], FT)
            if not np.max(lo.tau.astype(DT) * lo.varpi.astype(DT)) > 2 * O.eps(DT):
                raise NotImplementedError("non-scattering layer %d" % (iz + 1))
            dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
            expk = np.exp(-dtau / FT(qp.mu0)).astype(FT)
            OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd,
                             qp, added, al, FT, DT)
            dall = np.zeros((S, P), dtype=FT)
            dall[:, :pl] = lins[iz].tau_dot / FT(2 ** nd)
            OL.doubling_lin(pol, expk, nd, added, al, dall, qp.mu0, pl, FT)
            layers.append((MSO._copy_added(added), _copy_lin(al)))
            if iz == 0:
                O.copy_added_to_composite(comp, added)
                for a, b in ((cl.T_pp, al.ap_t_pp), (cl.T_mm, al.ap_t_mm), (cl.R_mp, al.ap_r_mp), (cl.R_pm, al.ap_r_pm),
                             (cl.J0_p, al.ap_J0_p), (cl.J0_m, al.ap_J0_m)):
                    a[...] = b
            else:
                OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
            if iz + 1 in interior or iz + 1 == Nz:
                tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy(), cl.R_pm.copy(), cl.J0_p.copy())
        if surface is None:
            OL.create_surface_layer_lambertian_lin(model.albedo, added_s, als, P - 1, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1],
                                                   F0, FT)
        else:
            rho, drho = surface(m) if callable(surface) else CM.reflectance_and_deriv(surface, pol.n, mu, m)
            CM.create_surface_layer_brdf_lin(rho, drho, added_s, als, P - 1, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
        res = {}
        if Nz in distinct:                               # level Nz: the surface layer alone below
            A, a, Ad, ad = tops[Nz]
            res[Nz] = level_lin_push_through(FT, A, a, added_s.r_mp, added_s.j0_m, Ad, ad, als.ap_r_mp, als.ap_J0_m)
        bot = None
        ends = interior[1:] + [Nz]
        for l, end in reversed(list(zip(interior, ends))):   # 2./3. segments and bottoms from the surface up
            seg = O.CompositeLayer(*[x.copy() for x in (layers[l][0].R_mp, layers[l][0].R_pm, layers[l][0].T_pp, layers[l][0].T_mm,
                                                         layers[l][0].J0_p, layers[l][0].J0_m)])
            segl = _copy_comp_lin(layers[l][1])
            for iz in range(l + 1, end):
                OL.interaction_lin(ifaces[iz], seg, segl, MSO._as_added(layers[iz][0]), _as_added_lin(layers[iz][1]), FT)
            if bot is None:
                OL.interaction_lin(ifaces[-1], seg, segl, added_s, als, FT)
            else:
                OL.interaction_lin("11", seg, segl, MSO._as_added(bot[0]), _as_added_lin(bot[1]), FT)
            bot = (seg, segl)
            A, a, Ad, ad = tops[l]
            res[l] = level_lin_push_through(FT, A, a, seg.R_mp, seg.J0_m, Ad, ad, segl.R_mp, segl.J0_m)   # 4. the level equation
        OL.interaction_lin(ifaces[-1], comp, cl, added_s, als, FT)
        res[0] = (comp.J0_m.copy(), comp.J0_p.copy(), cl.J0_m.copy(), cl.J0_p.copy())
        for l in distinct:
            if full is not None:
                full[(l, m)] = res[l]
            uw, dw, uwd, dwd = res[l]
            MSO._vza_rows(model, m, weight, uw, dw, out[l][0], out[l][1])
            _vza_rows_lin(model, m, weight, uwd, dwd, out[l][2], out[l][3])
    return tuple([out[l][i].copy() for l in levels] for i in range(4))
