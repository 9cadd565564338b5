"""Test oracle of SurfaceEmission, the thermal emission of the lower boundary, in numpy.  Built on
tests/ms_thermal_oracle.py, tests/flux_oracle.py, tests/thermal_lin_oracle.py, tests/ms_thermal_lin_oracle.py and
tests/flux_lin_oracle.py, which it imports and does not change.

The `:thermal` slot is linear in its sources, so the total of a run is the existing oracles' result (solar slot + Planck volume
source over a boundary that does not emit) plus the response to the surface emission alone: a walk of the slot with a Planck table
of zero rows and the emission vector in j0- of the slot's surface layer,

    j0-[i n + c, s] = 2 pi B_surface[s] ( delta_{c,0} - sum_j r-+[i n + c, j n, s] )         (Kirchhoff)
    j0-[i n + c, s] = 2 pi B_surface[s] delta_{c,0} emissivity[s]                            (explicit emissivity)

computed from the oracle's OWN surface r-+ (emission_vector).

emission_response(model, B_surface, levels, ...)          the forward response at the levels (level 0 = the share of rt_run's R, T)
emission_response_lin(model, lin, B_surface, levels, ...) the response and its Jacobians: the layer slots through the propagation
                                                          of j0-, the surface slots also through d j0- / d x (Kirchhoff), then one
                                                          skin slot per table of B_surface_dot (the forward response of that table)
level_vectors / level_vectors_lin                         {level: ...} at all streams, in the form flux_oracle.fluxes_from_vectors /
                                                          flux_lin_oracle.fluxes_lin_from_vectors take

`surface`: as in the oracles underneath -- forward: None (the model's Lambertian albedo) or a function (m, added_surf, tau_sum);
linearized: None or the pair (K, build) of thermal_lin_oracle.
"""
from __future__ import annotations

import math

import numpy as np

import ms_lin_oracle as MSL
import ms_oracle as MSO
import ms_thermal_oracle as MST
import thermal_lin_oracle as TL
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL


def emissivity_rows(r_mp, n):
    """[S | 1, N]: delta_{c,0} - sum_j r-+[i n + c, j n] of every row of a surface r-+ [S | 1, N, N] (Kirchhoff)."""
    r = np.asarray(r_mp)
    delta = np.zeros(r.shape[-1], dtype=r.dtype)
    delta[::n] = 1
    return delta[None, :] - r[:, :, ::n].sum(axis=2)


def emission_vector(r_mp, n, B_surface, emissivity=None):
    """The emission added to j0- of the surface layer, [S, N] in r-+'s precision."""
    r = np.asarray(r_mp)
    FT = r.dtype.type
    B = np.asarray(B_surface, dtype=FT)
    if emissivity is None:
        eps = np.broadcast_to(emissivity_rows(r, n), (B.shape[0], r.shape[-1]))
    else:
        delta = np.zeros(r.shape[-1], dtype=FT)
        delta[::n] = 1
        eps = np.broadcast_to(np.asarray(emissivity, dtype=FT), B.shape)[:, None] * delta[None, :]
    return ((FT(2 * math.pi) * B)[:, None] * eps).astype(FT)


def _emitting_surface(model, surface, added_surf, tau_sum, B_surface, emissivity):
    """The slot's surface layer (ms_thermal_oracle._thermal_surface: no beam terms) with the emission in j0-."""
    MSO._surface_fn(model, surface)(0, added_surf, tau_sum)
    added_surf.j0_p[...] = 0
    added_surf.j0_m[...] = emission_vector(added_surf.r_mp, model.pol.n, B_surface, emissivity)


def emission_response(model, B_surface, levels, surface=None, emissivity=None, full=None, B_layer=None):
    """(uw, dw): lists of [nVZA, nStokes, S] in the order of `levels`, the response of the thermal slot to the surface emission
    alone -- ms_thermal_oracle.ms_thermal_segmented's walk with a Planck table of zero rows over the emitting surface layer.  Level
    Nz: the bottom is the surface layer alone, c = its j0-.  full: receives {(level, 0): (uw [S, N], dw [S, N])}.
    B_layer [rows, S]: walk that Planck table instead of the empty one -- the whole thermal slot, for surfaces the thermal oracle
    underneath does not build (it takes the model's Lambertian albedo only)."""
    S = model.tau_rayl.shape[0]
    levels, Nz, FT, pol, S, L, N, B_layer, lods, ifaces, tau_sum_all, weight = MST._begin(
        model, np.zeros((0, S)) if B_layer is None else B_layer, levels)
    nV = len(model.vza)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    out = {l: (np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)) for l in distinct}
    added, added_surf = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    layers, comp, tops = [], None, {}
    for iz in range(L):
        MST._thermal_layer_step(model, lods, tau_sum_all, iz, B_layer, added)
        layers.append(MSO._copy_added(added))
        if iz == 0:
            comp = MSO._copy_added(added)
        else:
            O.interaction(ifaces[iz], comp, added, FT)
        if iz + 1 in interior or iz + 1 == Nz:
            tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy())
    _emitting_surface(model, surface, added_surf, tau_sum_all[:, -1], B_surface, emissivity)
    res = {}
    if Nz in distinct:
        res[Nz] = MSO.level_push_through(FT, *tops[Nz], added_surf.r_mp, added_surf.j0_m)
    bot = None
    for l, end in reversed(list(zip(interior, interior[1:] + [Nz]))):
        seg = MSO._copy_added(MSO._as_added(layers[l]))
        for iz in range(l + 1, end):
            O.interaction(ifaces[iz], seg, MSO._as_added(layers[iz]), FT)
        if bot is None:
            O.interaction(ifaces[-1], seg, added_surf, FT)
        else:
            O.interaction("11", seg, MSO._as_added(bot), FT)
        bot = seg
        res[l] = MSO.level_push_through(FT, *tops[l], bot.R_mp, bot.J0_m)
    O.interaction(ifaces[-1], comp, added_surf, FT)
    res[0] = (comp.J0_m.copy(), comp.J0_p.copy())
    for l in distinct:
        if full is not None:
            full[(l, 0)] = res[l]
        MSO._vza_rows(model, 0, weight, res[l][0], res[l][1], out[l][0], out[l][1])
    return [out[l][0].copy() for l in levels], [out[l][1].copy() for l in levels]


def emission_response_lin(model, lin, B_surface, levels, surface=None, emissivity=None, B_surface_dot=None, full=None):
    """(uw, dw, uw_dot, dw_dot) of the response to the surface emission alone, uw_dot / dw_dot [nVZA, nStokes, S, P + nSkin]:
    ms_thermal_lin_oracle.ms_thermal_lin_segmented's walk with a Planck table of zero rows; after the beam terms of the surface
    layers are zeroed, j0- receives the emission and, in Kirchhoff mode, the surface slots of ap_J0- receive
    -2 pi B_surface sum_j ap_r-+[.., j n].  The skin slots are forward responses (emission_response of B_surface_dot[k]).
    full: receives {(level, 0): (uw, dw [S, N], uw_dot, dw_dot [P + nSkin, S, N])}."""
    levels, Nz = MSO._check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, _ = MSO._setup(model)
    nV, n = len(model.vza), pol.n
    pl = lin.n_layer_params
    K, build_surface = TL._lambertian(model) if surface is None else surface
    P = pl + K
    Bs = np.asarray(B_surface, dtype=FT)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    F0 = np.zeros((n, S), dtype=FT)
    added, added_s = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    al, als = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S)
    m, weight = 0, FT(0.5 / math.pi)
    lods = O.construct_core_optical_properties(model, m)
    lins = OL.layer_optics_lin(model, lin, lods, m)
    ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
    tsd = np.zeros((S, pl, L + 1))
    for iz in range(L):
        tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
    layers, tops = [], {}
    comp, cl = O.make_composite_layer(FT, N, S), OL.make_composite_layer_lin(FT, P, N, S)
    for iz in range(L):
        lo = O.expand_optical_properties(lods[iz], FT)
        if not np.max(lo.tau.astype(DT) * lo.varpi.astype(DT)) > 2 * O.eps(DT):
            raise NotImplementedError("non-scattering layer %d" % (iz + 1))
        dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
        OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd, qp,
                         added, al, FT, DT)                      # F0 = 0 and no Planck row: the layer emits nothing
        OL.doubling_lin(pol, np.ones(S, dtype=FT), nd, added, al, np.zeros((S, P), dtype=FT), qp.mu0, pl, FT)
        layers.append((MSO._copy_added(added), MSL._copy_lin(al)))
        if iz == 0:
            O.copy_added_to_composite(comp, added)
            for a, b in ((cl.T_pp, al.ap_t_pp), (cl.T_mm, al.ap_t_mm), (cl.R_mp, al.ap_r_mp), (cl.R_pm, al.ap_r_pm),
                         (cl.J0_p, al.ap_J0_p), (cl.J0_m, al.ap_J0_m)):
                a[...] = b
        else:
            OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
        if iz + 1 in interior or iz + 1 == Nz:
            tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy(), cl.R_pm.copy(), cl.J0_p.copy())
    build_surface(added_s, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
    for arr in (added_s.j0_p, added_s.j0_m, als.ap_J0_p, als.ap_J0_m):
        arr[...] = 0
    added_s.j0_m[...] = emission_vector(added_s.r_mp, n, Bs, emissivity)
    if emissivity is None:
        for p in range(pl, P):
            als.ap_J0_m[p][...] = -(FT(2 * math.pi) * Bs)[:, None] * np.broadcast_to(als.ap_r_mp[p][:, :, ::n].sum(axis=2), (S, N))
    res = {}
    if Nz in distinct:
        A, a, Ad, ad = tops[Nz]
        res[Nz] = MSL.level_lin_push_through(FT, A, a, added_s.r_mp, added_s.j0_m, Ad, ad, als.ap_r_mp, als.ap_J0_m)
    bot = None
    for l, end in reversed(list(zip(interior, interior[1:] + [Nz]))):
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
        res[l] = MSL.level_lin_push_through(FT, A, a, seg.R_mp, seg.J0_m, Ad, ad, segl.R_mp, segl.J0_m)
    OL.interaction_lin(ifaces[-1], comp, cl, added_s, als, FT)
    res[0] = (comp.J0_m.copy(), comp.J0_p.copy(), cl.J0_m.copy(), cl.J0_p.copy())
    nSkin = 0 if B_surface_dot is None else len(B_surface_dot)
    if nSkin:
        fsurf = None if surface is None else (lambda m_, a_, ts_: _copy_surface(a_, added_s))
        skins = []
        for k in range(nSkin):
            fk = {}
            emission_response(model, B_surface_dot[k], distinct, surface=fsurf, emissivity=emissivity, full=fk)
            skins.append(fk)
        for l in distinct:
            uw, dw, uwd, dwd = res[l]
            res[l] = (uw, dw, np.concatenate([uwd, np.stack([f[(l, 0)][0] for f in skins])]),
                      np.concatenate([dwd, np.stack([f[(l, 0)][1] for f in skins])]))
    Pa = P + nSkin
    out = {l: (np.zeros((nV, n, S), dtype=FT), np.zeros((nV, n, S), dtype=FT), np.zeros((nV, n, S, Pa), dtype=FT),
               np.zeros((nV, n, S, Pa), dtype=FT)) for l in distinct}
    for l in distinct:
        if full is not None:
            full[(l, 0)] = res[l]
        uw, dw, uwd, dwd = res[l]
        MSO._vza_rows(model, m, weight, uw, dw, out[l][0], out[l][1])
        MSL._vza_rows_lin(model, m, weight, uwd, dwd, out[l][2], out[l][3])
    return tuple([out[l][i].copy() for l in levels] for i in range(4))


def _copy_surface(dst, src):
    """The forward surface layer the linearized builder made, as the forward walk's surface (its matrices; j0+- are set after)."""
    for f in ("r_mp", "r_pm", "t_pp", "t_mm", "j0_p", "j0_m"):
        getattr(dst, f)[...] = getattr(src, f)


def level_vectors(model, levels, B_surface, surface=None, emissivity=None):
    """{level: (uw, dw)} [S, N] float64 of the response, to be added to flux_oracle.level_vectors' (m = 0)."""
    import dataclasses
    full = {}
    distinct = sorted(set(int(l) for l in levels))
    emission_response(dataclasses.replace(model, m_max=0), B_surface, distinct, surface=surface, emissivity=emissivity, full=full)
    return {l: tuple(np.asarray(v, dtype=np.float64) for v in full[(l, 0)]) for l in distinct}


def level_vectors_lin(model, lin, levels, B_surface, surface=None, emissivity=None, B_surface_dot=None):
    """{level: (uw, dw, uw_dot, dw_dot)} float64 of the response, to be added to flux_lin_oracle.level_vectors_lin's."""
    import dataclasses
    full = {}
    distinct = sorted(set(int(l) for l in levels))
    emission_response_lin(dataclasses.replace(model, m_max=0), lin, B_surface, distinct, surface=surface, emissivity=emissivity,
                          B_surface_dot=B_surface_dot, full=full)
    return {l: tuple(np.asarray(v, dtype=np.float64) for v in full[(l, 0)]) for l in distinct}


def add_vectors(a, b):
    """{level: tuple} + {level: tuple}, the derivative stacks of `a` padded with zero slots up to b's (the slots only b has)."""
    out = {}
    for l in a:
        row = []
        for x, y in zip(a[l], b[l]):
            if x.shape != y.shape:
                x = np.concatenate([x, np.zeros((y.shape[0] - x.shape[0],) + x.shape[1:], dtype=x.dtype)])
            row.append(x + y)
        out[l] = tuple(row)
    return out
