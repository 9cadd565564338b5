"""Test oracle of the multi-sensor run (vsm.CoreRT.rt_run_multisensor), built on oracle/vsm_oracle.py, which it imports and does
not change.

ms_reference(model, levels)  the reference's prototype, statement order: rt_run_test_ms(::noRS, sensor_levels, model, iBand)
                             (src/CoreRT/rt_run_multisensor.jl) with rt_kernel_multisensor! (CoreKernel/rt_kernel_multisensor.jl:
                             7-143), interaction_top! / interaction_bot! (CoreKernel/interaction_multisensor.jl:158-240) and
                             postprocessing_vza_ms! (tools/postprocessing_vza_ms.jl:7-52) with interlayer_flux_helper!
                             (CoreKernel/interlayer_flux.jl:1-19): per sensor a top and a bottom composite, one interaction per
                             sensor and layer.
ms_segmented(model, levels)  the device algorithm in numpy: one top pass (snapshots of R+- / J0+ after each interior level), one
                             segment composite per interval between levels, bottoms composed from the surface up, and the level
                             equation by the push-through identity (one solve per level).

Level l is the boundary below layer l counted from the TOA (0 = TOA, Nz = just above the surface).  Level Nz takes the surface
layer alone as its bottom composite: the prototype never initialises that composite (its copy at iz == l + 1 never happens), and
the surface layer is what the level means physically.

`surface`: None = the model's Lambertian albedo (scalar or a per-point spectrum); else a function (m, added_surf, tau_sum) that
fills the surface AddedLayer of moment m (e.g. a BRDF through vsm_oracle_coxmunk.create_surface_layer_brdf).
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


def _check_levels(model, levels):
    Nz = model.tau_rayl.shape[1]
    levels = [int(l) for l in levels]
    bad = [l for l in levels if l < 0 or l > Nz]
    if bad:
        raise ValueError("sensor level %d outside 0..Nz = 0..%d" % (bad[0], Nz))
    return levels, Nz


def _setup(model):
    FT, DT = model.FT, O.deciding_type(model)
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    F0 = model.F0
    if F0 is None:
        F0 = np.zeros((pol.n, S), dtype=FT)
        F0[0, :] = 1
    return FT, DT, pol, qp, S, L, N, F0


def _surface_fn(model, surface):
    if surface is not None:
        return surface
    FT, pol, qp = model.FT, model.pol, model.quad_points

    def fill(m, added_surf, tau_sum):
        if np.ndim(model.albedo) == 1:
            O.create_surface_layer_lambertian_spectral(model.albedo, added_surf, m, pol, qp, tau_sum, FT)
        else:
            O.create_surface_layer_lambertian(model.albedo, added_surf, m, pol, qp, tau_sum, FT)
    return fill


def _layer_step(model, m, lods, ifaces, tau_sum_all, iz, F0, added):
    """elemental! + doubling! of layer iz (0-based) into `added`: rt_kernel!'s scatter branch, the exact operations of O.rt_kernel
    (rt_kernel_multisensor.jl:29 hard-codes scatter = true; the callers refuse non-scattering columns)."""
    FT, DT = model.FT, O.deciding_type(model)
    lo = O.expand_optical_properties(lods[iz], FT)
    if not np.max(lo.tau.astype(DT) * lo.varpi.astype(DT)) > 2 * O.eps(DT):
        raise NotImplementedError("non-scattering layer %d" % (iz + 1))
    scratch = O.make_composite_layer(FT, added.r_mp.shape[1], added.r_mp.shape[0])
    O.rt_kernel(model.pol, added, scratch, lo, ifaces[iz], tau_sum_all[:, iz].astype(FT), m, model.quad_points, 1, F0, FT,
                model.numerics, None, DT)


def _copy_added(added) -> O.CompositeLayer:
    return O.CompositeLayer(added.r_mp.copy(), added.r_pm.copy(), added.t_pp.copy(), added.t_mm.copy(),
                            added.j0_p.copy(), added.j0_m.copy())


def _as_added(comp: O.CompositeLayer) -> O.AddedLayer:
    return O.AddedLayer(comp.R_mp, comp.T_pp, comp.R_pm, comp.T_mm, comp.J0_p, comp.J0_m)


def _vza_rows(model, m, weight, uw_vec, dw_vec, uw_out, dw_out):
    """postprocessing_vza_ms!'s VZA loop (postprocessing_vza_ms.jl:43-51): the rows and weights of _precompute_vza_weights."""
    c = O.CompositeLayer(None, None, None, None, dw_vec, uw_vec)
    O.postprocessing_vza(model.pol, c, model.vza, model.vaz, model.quad_points, m, weight, uw_out, dw_out)


def interlayer_flux_reference(FT, topR_pm, botR_mp, topJ0_p, botJ0_m):
    """interlayer_flux_helper!(::noRS) (interlayer_flux.jl:1-19), statement for statement: two inverses, four products."""
    N = topR_pm.shape[-1]
    I = np.eye(N, dtype=FT)[None]
    tmpR = O.batch_inv(I - topR_pm @ botR_mp).astype(FT)
    dw = O._mv(tmpR, topJ0_p + O._mv(topR_pm, botJ0_m))
    tmpR = O.batch_inv(I - botR_mp @ topR_pm).astype(FT)
    uw = O._mv(tmpR, botJ0_m + O._mv(botR_mp, topJ0_p))
    return uw, dw


def level_push_through(FT, A, a, B, c):
    """The device's level equation: dw = (I - A B)^-1 (a + A c) by one solve, uw = c + B dw."""
    N = A.shape[-1]
    B = np.broadcast_to(B, A.shape)
    M = np.eye(N, dtype=FT)[None] - A @ B
    d = a + O._mv(A, c)
    dw = np.linalg.solve(M, d[..., None])[..., 0].astype(FT)
    uw = (c + O._mv(B, dw)).astype(FT)
    return uw, dw


def ms_reference(model, levels, surface=None, full=None):
    """rt_run_test_ms(::noRS, sensor_levels, model, iBand): (uwJ, dwJ), lists of [nVZA, nStokes, nSpec] in the order of `levels`.
    full: a dict that receives {(level, m): (uw [S, N], dw [S, N])} (the level vectors at all streams, before the VZA rows)."""
    levels, Nz = _check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, F0 = _setup(model)
    fill_surface = _surface_fn(model, surface)
    nV = len(model.vza)
    uwJ = [np.zeros((nV, pol.n, S), dtype=FT) for _ in levels]
    dwJ = [np.zeros((nV, pol.n, S), dtype=FT) for _ in levels]
    added, added_surf = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        top, bot = [None] * len(levels), [None] * len(levels)
        for iz in range(1, L + 1):                       # rt_kernel_multisensor!, iz 1-based
            _layer_step(model, m, lods, ifaces, tau_sum_all, iz - 1, F0, added)
            for ims, lev in enumerate(levels):
                if iz == 1:
                    if lev == 0:
                        bot[ims] = _copy_added(added)
                    else:
                        top[ims] = _copy_added(added)
                elif lev == 0:
                    O.interaction(ifaces[iz - 1], bot[ims], added, FT)       # interaction_bot!
                elif lev == iz - 1:
                    bot[ims] = _copy_added(added)
                elif lev < iz - 1:
                    O.interaction(ifaces[iz - 1], bot[ims], added, FT)       # interaction_bot!
                else:                                                        # lev >= iz
                    O.interaction(ifaces[iz - 1], top[ims], added, FT)       # interaction_top!
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        for ims, lev in enumerate(levels):
            if lev == Nz:
                bot[ims] = _copy_added(added_surf)       # the level-Nz deviation: the surface layer alone
            else:
                O.interaction(ifaces[-1], bot[ims], added_surf, FT)          # interaction_bot! with the surface
        for ims, lev in enumerate(levels):               # postprocessing_vza_ms!
            if lev == 0:
                uw, dw = bot[ims].J0_m.copy(), bot[ims].J0_p.copy()
            else:
                uw, dw = interlayer_flux_reference(FT, top[ims].R_pm, bot[ims].R_mp, top[ims].J0_p, bot[ims].J0_m)
            if full is not None:
                full[(lev, m)] = (uw, dw)
            _vza_rows(model, m, weight, uw, dw, uwJ[ims], dwJ[ims])
    return uwJ, dwJ


def ms_segmented(model, levels, surface=None, full=None):
    """The device algorithm (core_rt_ms.py) in numpy: same outputs as ms_reference up to rounding."""
    levels, Nz = _check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, F0 = _setup(model)
    fill_surface = _surface_fn(model, surface)
    nV = len(model.vza)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    out = {l: (np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)) for l in distinct}
    added, added_surf = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        layers = []
        comp = None
        tops = {}
        for iz in range(L):                              # 1. the top pass
            _layer_step(model, m, lods, ifaces, tau_sum_all, iz, F0, added)
            layers.append(_copy_added(added))
            if iz == 0:
                comp = _copy_added(added)
            else:
                O.interaction(ifaces[iz], comp, added, FT)
            if iz + 1 in interior or iz + 1 == Nz:
                tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy())
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        res = {}
        if Nz in distinct:                               # level Nz: the surface layer alone below
            res[Nz] = level_push_through(FT, *tops[Nz], added_surf.r_mp, added_surf.j0_m)
        bot = None
        ends = interior[1:] + [Nz]
        for l, end in reversed(list(zip(interior, ends))):   # 2./3. segments and bottoms from the surface up
            seg = O.CompositeLayer(*[x.copy() for x in (layers[l].R_mp, layers[l].R_pm, layers[l].T_pp, layers[l].T_mm,
                                                         layers[l].J0_p, layers[l].J0_m)])
            for iz in range(l + 1, end):
                O.interaction(ifaces[iz], seg, _as_added(layers[iz]), FT)
            if bot is None:
                O.interaction(ifaces[-1], seg, added_surf, FT)
            else:
                O.interaction("11", seg, _as_added(bot), FT)
            bot = seg
            res[l] = level_push_through(FT, *tops[l], bot.R_mp, bot.J0_m)     # 4. the level equation
        O.interaction(ifaces[-1], comp, added_surf, FT)
        res[0] = (comp.J0_m.copy(), comp.J0_p.copy())
        for l in distinct:
            if full is not None:
                full[(l, m)] = res[l]
            _vza_rows(model, m, weight, res[l][0], res[l][1], out[l][0], out[l][1])
    return [out[l][0].copy() for l in levels], [out[l][1].copy() for l in levels]


def net_flux(model, full, level, m=0):
    """Net upward flux at a level from the m = 0 level vectors at all streams (Stokes I rows):
    sum_i mu_i w_i (uw_i - dw_i) - mu0 F0 exp(-tau_l / mu0), [S].  Constant over the levels of a conservative column."""
    pol, qp = model.pol, model.quad_points
    uw, dw = full[(level, m)]
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    tau_l = np.sum(np.asarray(model.tau_rayl, dtype=np.float64)[:, :level] + np.asarray(model.tau_abs, dtype=np.float64)[:, :level],
                   axis=1)       # (Rayleigh / absorption columns)
    diff = (uw[:, ::pol.n] - dw[:, ::pol.n]) @ (mu * w)
    return diff - float(qp.mu0) * np.exp(-tau_l / float(qp.mu0))
