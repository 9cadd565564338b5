"""Linearized multi-sensor runs: radiances and their Jacobians at any level of the column, up and down.

The reference has no linearized multi-sensor driver: this is the algorithm of the elastic multi-sensor run (core_rt_ms.py, DESIGN.md
§4.8) on the linearized composites of SceneLin (core_rt_lin.py).  Adding is associative for the linearized composites too
(_CompositeLinAsAdded: composite (+) composite, as in the interaction tree of SceneLin), and every linearized layer source carries its
absolute attenuation derivative from the TOA (tau_sum_dot), so a segment's derivatives are right with respect to the parameters of
the layers above it.  Per Fourier moment, on one stream:

  1. top pass: SceneLin._run_moment's layer walk; after layer l_k the composite's R+-, J0+ and their derivatives (the layer slots
     [0, pl) only: a top's surface slot is exactly zero) are kept as the top of level l_k, before the surface interaction as the top
     of level Nz; the surface interaction and post-processing give level 0 (= SceneLin.run(lanes=1, fold=False) bit for bit, the
     Stokes_IQ sub-scene of m = 0 included: it runs this whole algorithm for m = 0 and its I, Q rows are copied in at every level);
  2. segments: layers l_k+1 .. l_{k+1} (the last one ends at Nz) as linearized composites of their own, the first a copy, every
     layer with its absolute tau_sum and tau_sum_dot;
  3. bottoms from the surface up: bot_K = seg_K (+) surface, bot_k = seg_k (+) bot_{k+1} (interaction_lin_ on ALL parameter slots:
     a bottom carries the surface slot);
  4. per level one elastic level call (vsm_level_radiance_*, its level vectors at all streams feed the derivative) and one
     linearized one (vsm_level_radiance_lin_*), level Nz with the surface layer alone as its bottom.

Per moment: Nz + (Nz - l_1) linearized layer steps, L + 1 further linearized interactions (L interior levels) and one elastic and one
linearized level call per level other than 0.

With a ThermalEmission source the `:thermal` per-source slot of rt_run_lin and its Planck slots follow the solar
moments, for m = 0 alone (_run_thermal): the same four steps on the slot's own linearized composites (SceneLin._thermal_lin_walk:
expk = 1, so a segment needs no tau_sum) and, per Planck table, on the forward thermal composites of CoreRT.ThermalSlot.walk, of which
only the source vectors J0+ (top) and J0- (bottom) are kept.  The slot solves its level equation on ITS OWN operators, not on the
solar ones as the forward run does (§4.8d): the solar m = 0 may have run as a Stokes_IQ sub-scene at another N.  Per level other
than 0: one elastic call on the thermal composites and ONE vsm_level_radiance_lin_src_* call for all Nparams + nPlanck slots.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from . import core_rt_lin as CL
from . import core_rt_ms as MS
from . import host_model as H

LEVEL_LIN_MAX_N = 128   # vsm_level_radiance_lin_*: one workgroup per point; there is no operator-level twin


def level_radiance_lin_(pol, qp, vza, vaz, m: int, weight: float, P: int, P_top: int, top_R_pm, bot_R_mp, dw_full, uw_full,
                        top_R_pm_lin, top_J0_p_lin, bot_R_mp_lin, bot_J0_m_lin, uw_lin, dw_lin, dw_lin_full=None, uw_lin_full=None):
    """The derivative of the level equation at one boundary (+ the VZA rows of postprocessing_vza_lin!): uw_lin / dw_lin
    (P, S, n, nV) layout tensors += weight * rows of
        q_p = c'_p + B'_p dw,   dw'_p = (I - A B)^-1 (a'_p + A'_p uw + A q_p),   uw'_p = q_p + B dw'_p
    A = top_R_pm (S, N, N), B = bot_R_mp ((S | 1, N, N)), dw_full / uw_full (S, N) the elastic level vectors; top_R_pm_lin /
    top_J0_p_lin (P_top, S, N[, N]) (slots >= P_top of the top are zero), bot_R_mp_lin ((P, S | 1, N, N)), bot_J0_m_lin (P, S, N).
    dw_lin_full / uw_lin_full: (P, S, N) tensors that receive the derivative vectors at all streams."""
    setup = MS.level_call_setup(pol, qp, vza, vaz, m, weight, dw_full, bot_R_mp)
    if setup is None:
        return
    S, N, dt, row0, w, bot_stride = setup
    sb = int(bot_R_mp_lin.shape[1])
    bd_stride = 0 if sb == 1 and S > 1 else N * N
    Pt = CR._ptr
    _lib.call("vsm_level_radiance_lin", dt, N, pol.n, S, int(P), int(P_top), len(vza), row0, w, Pt(top_R_pm), Pt(bot_R_mp), bot_stride,
              Pt(dw_full), Pt(uw_full), Pt(top_R_pm_lin) if P_top else None, S * N * N, Pt(top_J0_p_lin) if P_top else None,
              Pt(bot_R_mp_lin), bd_stride, sb * N * N, Pt(bot_J0_m_lin), Pt(uw_lin), Pt(dw_lin), Pt(dw_lin_full), Pt(uw_lin_full),
              CR._stream_ptr())


def level_radiance_lin_src_(pol, qp, vza, vaz, m: int, weight: float, P: int, P_top: int, top_R_pm, bot_R_mp, dw_full, uw_full,
                            top_R_pm_lin, top_J0_p_lin, bot_R_mp_lin, bot_J0_m_lin, src_top_J0_p, src_bot_J0_m, uw_lin, dw_lin,
                            dw_lin_full=None, uw_lin_full=None):
    """level_radiance_lin_ with P_src source-only slots behind the P parameter slots (vsm_level_radiance_lin_src_*): for slot
    P + k, dw' = (I - A B)^-1 (a_k + A c_k), uw' = c_k + B dw', a_k = src_top_J0_p[k], c_k = src_bot_J0_m[k] ((P_src, S, N)
    tensors, or None for P_src = 0).  uw_lin / dw_lin (P + P_src, S, n, nV), dw_lin_full / uw_lin_full (P + P_src, S, N)."""
    setup = MS.level_call_setup(pol, qp, vza, vaz, m, weight, dw_full, bot_R_mp)
    if setup is None:
        return
    S, N, dt, row0, w, bot_stride = setup
    sb = int(bot_R_mp_lin.shape[1])
    bd_stride = 0 if sb == 1 and S > 1 else N * N
    P_src = 0 if src_top_J0_p is None else int(src_top_J0_p.shape[0])
    Pt = CR._ptr
    _lib.call("vsm_level_radiance_lin_src", dt, N, pol.n, S, int(P), int(P_top), P_src, len(vza), row0, w, Pt(top_R_pm), Pt(bot_R_mp),
              bot_stride, Pt(dw_full), Pt(uw_full), Pt(top_R_pm_lin) if P_top else None, S * N * N,
              Pt(top_J0_p_lin) if P_top else None, Pt(bot_R_mp_lin), bd_stride, sb * N * N, Pt(bot_J0_m_lin),
              Pt(src_top_J0_p) if P_src else None, Pt(src_bot_J0_m) if P_src else None, Pt(uw_lin), Pt(dw_lin), Pt(dw_lin_full),
              Pt(uw_lin_full), CR._stream_ptr())


@dataclass
class MultiSensorLinResult(MS.MultiSensorResult):
    """rt_run_multisensor(model, lin_model, ..., streams=True): per entry of sensor_levels the VZA outputs and their Jacobians and,
    per Fourier moment, the level vectors and their derivatives at ALL quadrature streams: the fields of MultiSensorResult and"""
    uw_dot: List[np.ndarray]                # [nVZA, nStokes, nSpec, Nparams (+ nPlanck)] per level
    dw_dot: List[np.ndarray]
    uw_dot_streams: List[List[np.ndarray]]  # [level][moment] -> [N, 1, nSpec, Nparams (+ nPlanck)]
    dw_dot_streams: List[List[np.ndarray]]

    FIELDS = ("uw", "dw", "uw_dot", "dw_dot")


class LevelSink:
    """What a run other than the multi-sensor one does at each level of the walk of _run_scene / _run_thermal, in place of their
    level calls (core_rt_flux_lin.py: the flux Jacobians).  With a sink no VZA output is allocated and no level call is issued
    here; the walk itself -- tops, segments, bottoms -- is the same.  top = (R+-, J0+, R+-', J0+' [:pl]) of the composite above
    the level, bot = (R-+, J0-, R-+', J0-') of the one below, src = the Planck source stacks (a_k, c_k) ((K, S, N) each) or None;
    thermal: the call comes from the `:thermal` slot (on the scene's own N, after the solar moments)."""

    def level(self, sc, mom, l, top, bot, src, thermal):
        raise NotImplementedError

    def level0(self, sc, mom, J0_m, J0_m_lin, src_J0_m, thermal):
        """Level 0, the TOA: J0- of the whole column with the surface, its derivative stack (P, S, N) and the Planck slots'
        J0- ((K, S, N) or None)."""
        raise NotImplementedError


def _run_scene(sc: CL.SceneLin, plan: MS.LevelPlan, streams: bool, sink: Optional[LevelSink] = None):
    """The linearized multi-sensor algorithm on one SceneLin.  Returns ({level: [uw, dw, uw_dot, dw_dot]} of (S, nStokes, nVZA) /
    (P, S, nStokes, nVZA) device tensors, {m: {level: (uw, dw, uw_dot, dw_dot) (S, N) / (P, S, N)}} or None, the Fourier weights).
    sink: see LevelSink (then the first of these holds level 0 alone and streams is not taken); where the scene runs m = 0 on its
    Stokes_IQ sub-scene the sink sees that sub-scene's levels, and the thermal slot's on this scene."""
    model, fwd, FT, dt = sc.model, sc.fwd, sc.FT, sc.dt
    pol, qp = sc.pol, sc.qp
    N, S, P, pl = sc.N, sc.S, sc.P, sc.pl
    w = sc._lane_state(0)      # (the whole run is on one stream: lane 0)
    lane = w["lane"]
    torch._foreach_zero_([w["R"], w["T"], w["Rd"], w["Td"]])
    dev = sc.R.device
    nV = len(model.vza)
    z = lambda *sh: torch.zeros(sh, dtype=dt, device=dev)
    thermal = sc.has_thermal
    Pa = P + sc.nSrc         # (the Planck and skin slots follow the parameter slots; the solar level calls fill the first P)
    out = {} if sink is not None else {l: [z(S, pol.n, nV), z(S, pol.n, nV), z(Pa, S, pol.n, nV), z(Pa, S, pol.n, nV)]
                                       for l in plan.distinct if l != 0}
    out[0] = [sc.R, sc.T, sc.Rd, sc.Td]
    full = {} if streams else None
    weights = [float(MS.fourier_weight(FT, m)) for m in range(model.m_max + 1)]
    if S == 0:
        return out, full, weights
    reduced = sc.sub0 is not None
    if reduced and sink is not None:
        _run_scene(sc.sub0, plan, False, sink)
    elif reduced:      # m = 0 first, like SceneLin.run
        MS.merge_sub0(_run_scene(sc.sub0, plan, streams), pol.n,
                      {l: o[:2] + [o[2][:P], o[3][:P]] for l, o in out.items()} if thermal else out, full)
    segs = [(CR.make_composite_layer(FT, sc.arch, (N, N), S), CL.CompositeLayerLin(FT, sc.arch, P, N, S))
            for _ in range(2 if plan.interior and not (sink is not None and reduced and not thermal) else 0)]
    for mom in fwd.moments:
        m = mom["m"]
        if m == 0 and reduced:
            continue
        weight = float(MS.fourier_weight(FT, m))
        fv = {}
        tops = {}

        def keep(l, comp, cl):
            if l in plan.tops_at:
                tops[l] = (comp.R_pm.clone(), comp.J0_p.clone(), cl.R_pm[:pl].clone(), cl.J0_p[:pl].clone())

        # 1. the top pass, level 0 included (its surface layer stays in w["added_s"] / w["als"] for the bottoms)
        sc._run_moment(mom, w, after_layer=keep)
        if streams:
            fv[0] = (w["comp"].J0_m.clone(), w["comp"].J0_p.clone(), w["cl"].J0_m.clone(), w["cl"].J0_p.clone())
        asurf, als = w["added_s"], w["als"]
        if sink is not None and 0 in plan.distinct:
            sink.level0(sc, mom, w["comp"].J0_m, w["cl"].J0_m, None, False)

        def run_segment(seg, first, end):
            for iz in range(first, end):
                sc._double_layer(mom, iz, w)
                if iz == first:
                    CL.copy_added_to_composite_lin_(seg[0], seg[1], w["added"], w["al"])
                else:
                    CL.interaction_lin_(mom["layers"][iz]["iface"], seg[0], seg[1], w["added"], w["al"], p_range=sc._layer_slots,
                                        lane=lane)

        def level(l, seg):
            top = tops.pop(l)
            bot = (asurf.r_mp, asurf.j0_m, als.ap_r_mp, als.ap_J0_m) if seg is None else (seg[0].R_mp, seg[0].J0_m, seg[1].R_mp,
                                                                                          seg[1].J0_m)
            if sink is not None:
                sink.level(sc, mom, l, top, bot, None, False)
                return
            vs = MS.level_pair_(pol, qp, model.vza, model.vaz, m, weight, top, bot[0], bot[1], out[l],
                                lambda dwf, uwf, dwdf, uwdf: level_radiance_lin_(
                                    pol, qp, model.vza, model.vaz, m, weight, P, pl, top[0], bot[0], dwf, uwf, top[2], top[3],
                                    bot[2], bot[3], out[l][2], out[l][3], dwdf, uwdf), (P, S, N), streams)
            if streams:
                fv[l] = vs
        # 2.-4. linearized segments and bottoms from the surface up, the level calls of each level
        MS.walk_levels(plan, segs, run_segment,
                       lambda seg: CL.interaction_lin_(mom["iface_surface"], seg[0], seg[1], asurf, als, lane=lane),
                       lambda seg, bot, first, end: CL.interaction_lin_("11", seg[0], seg[1], CL._CompositeAsAdded(bot[0]),
                                                                        CL._CompositeLinAsAdded(bot[1]), lane=lane), level)
        if streams:
            full[m] = fv
    if thermal:
        _run_thermal(sc, plan, segs, out, full, sink)
    return out, full, weights


def _run_thermal(sc: CL.SceneLin, plan: MS.LevelPlan, segs, out, full, sink: Optional[LevelSink] = None):
    """The `:thermal` slot and the Planck slots of a linearized multi-sensor run (m = 0), after the solar moments, in the order
    of SceneLin._run_thermal at level 0 (its R, T, Rdot, Tdot bit for bit).  segs: the two segment composites of the solar walk,
    free by now.  The Planck sources come first: their vectors a_k, c_k of every level are kept ((K, S, N) each), the operators of
    those forward walks are not read; then the linearized slot, whose bottoms live only until the level above has used them.
    sink: see LevelSink."""
    model, fwd, dt = sc.model, sc.fwd, sc.dt
    pol, qp = sc.pol, sc.qp
    N, S, P, pl, K = sc.N, sc.S, sc.P, sc.pl, sc.nSrc      # (K source-only slots: the Planck tables, then the skin tables)
    dev = sc.R.device
    mom = fwd.moments[0]
    weight = float(MS.fourier_weight(sc.FT, 0))
    lane = sc._thermal_state()["lane"]
    new = lambda *sh: torch.empty(sh, dtype=dt, device=dev)
    below = [l for l in plan.distinct if l != 0]
    src = {l: (torch.zeros((K, S, N), dtype=dt, device=dev), torch.zeros((K, S, N), dtype=dt, device=dev)) for l in below} if K else {}
    src0 = torch.zeros((K, S, N), dtype=dt, device=dev) if K and sink is not None and 0 in plan.distinct else None
    fv = None
    if full is not None:      # the solar level vectors of m = 0 (the sub-scene's, expanded), their derivative stacks padded to P + K
        pad = (lambda v: torch.cat([v, torch.zeros((K,) + tuple(v.shape[1:]), dtype=dt, device=dev)])) if K else (lambda v: v)
        for m_, f in full.items():
            full[m_] = {l: (vs[0], vs[1], pad(vs[2]), pad(vs[3])) for l, vs in f.items()}
        fv = full[0]
    # 4. the Planck and skin sources: per table the forward slot of B := B_layer_dot[k] (or of B_surface := B_surface_dot[k] under an
    # empty Planck table), cut at the plan's levels as DESIGN 4.8d cuts it
    if K:
        th_segs = [CR.make_composite_layer(sc.FT, sc.arch, (N, N), S) for _ in range(2 if plan.interior else 0)]
        th = fwd.thermal_slot()
        try:
            for k, (B, B_surface) in enumerate(sc.source_tables()):
                th.begin(mom)
                th.walk(mom, th.comp, 0, fwd.Nz, B, after={l: (lambda c, l=l: src[l][0][k].copy_(c.J0_p)) for l in plan.tops_at})
                surf = th.surface(mom, B_surface)

                def keep_bottom(l, seg):     # (level Nz: the surface layer alone, c_k = its j0-: 0 unless table k is a skin table)
                    src[l][1][k].copy_(surf.j0_m if seg is None else seg.J0_m)
                MS.walk_levels(plan, th_segs, lambda seg, first, end: th.walk(mom, seg, first, end, B),
                               lambda seg: CR.interaction_(mom["iface_surface"], seg, surf, oplevel=True, work=fwd.work),
                               lambda seg, bot, first, end: CR.interaction_("11", seg, MS._CompositeAsAdded(bot), oplevel=True,
                                                                            work=fwd.work), keep_bottom)
                th.finish(mom, weight, sc.Rd[P + k], sc.Td[P + k])
                if src0 is not None:
                    src0[k].copy_(th.comp.J0_m)
                if fv is not None:
                    fv[0][2][P + k].copy_(th.comp.J0_m)
                    fv[0][3][P + k].copy_(th.comp.J0_p)
        finally:
            for c in th_segs:
                c.drop_native()
    # 1. the top pass of the linearized slot and level 0 (B_layer = 0 with Planck tables: SceneLin.run adds no slot, the walk
    # still supplies the operators the Planck slots are solved on)
    tops = {}

    def keep(l, comp, cl):
        if l in plan.tops_at:
            tops[l] = (comp.R_pm.clone(), comp.J0_p.clone(), cl.R_pm[:pl].clone(), cl.J0_p[:pl].clone())
    sc._thermal_lin_slot(mom, after_layer=keep, post=fwd.thermal_B is not None)
    t = sc._thermal_state()
    asurf, als = t["added_s"], t["als"]
    if fv is not None and fwd.thermal_B is not None:
        fv[0][0].add_(t["comp"].J0_m)
        fv[0][1].add_(t["comp"].J0_p)
        fv[0][2][:P].add_(t["cl"].J0_m)
        fv[0][3][:P].add_(t["cl"].J0_p)
    if sink is not None and 0 in plan.distinct:
        sink.level0(sc, mom, t["comp"].J0_m, t["cl"].J0_m, src0, True)

    def level(l, seg):
        top = tops.pop(l)
        bot = (asurf.r_mp, asurf.j0_m, als.ap_r_mp, als.ap_J0_m) if seg is None else (seg[0].R_mp, seg[0].J0_m, seg[1].R_mp,
                                                                                      seg[1].J0_m)
        if sink is not None:
            sink.level(sc, mom, l, top, bot, src[l] if K else None, True)
            return
        dwf, uwf = new(S, N), new(S, N)
        MS.level_radiance_(pol, qp, model.vza, model.vaz, 0, weight, top[0], top[1], bot[0], bot[1], out[l][0], out[l][1], dwf, uwf)
        dwd, uwd = (new(P + K, S, N), new(P + K, S, N)) if fv is not None else (None, None)
        a_k, c_k = src[l] if K else (None, None)
        level_radiance_lin_src_(pol, qp, model.vza, model.vaz, 0, weight, P, pl, top[0], bot[0], dwf, uwf, top[2], top[3], bot[2],
                                bot[3], a_k, c_k, out[l][2], out[l][3], dwd, uwd)
        if fv is not None:
            for acc, v in zip(fv[l], (uwf, dwf, uwd, dwd)):
                acc.add_(v)
    # 2.-4. the slot's segments and bottoms from the surface up, the two level calls of each level
    MS.walk_levels(plan, segs, lambda seg, first, end: sc._thermal_lin_walk(mom, seg[0], seg[1], first, end, fwd.thermal_B),
                   lambda seg: CL.interaction_lin_(mom["iface_surface"], seg[0], seg[1], asurf, als, lane=lane),
                   lambda seg, bot, first, end: CL.interaction_lin_("11", seg[0], seg[1], CL._CompositeAsAdded(bot[0]),
                                                                    CL._CompositeLinAsAdded(bot[1]), lane=lane), level)


def bytes_per_point(N: int, P: int, pl: int, Nz: int, n_tops: int, segments: bool, n_levels: int, n_stokes: int, nV: int,
                    itemsize: int, thermal: bool = False, nPlanck: int = 0) -> int:
    """Device bytes per spectral point of a linearized multi-sensor run (an estimate on the safe side): the kept tops, the two
    segment composites, the scene's own added / composite / surface layers (the surface layer counted as a full per-point layer,
    forward and derivative: what it is over LambertianSurfaceLegendre / Spline, more than the shared blocks of the other surfaces),
    its per-layer optics and the outputs.  thermal: what
    the thermal slot keeps beside them (m = 0 only, on the parent's N): its own tops, R and Rdot included ((1 + pl)(N^2 + N) each,
    while the solar tops of the last moment are still alive), its linearized added / composite / surface layers, the forward
    slot's three layers and two segment composites (the Planck walks), the Planck source vectors of every level, the Planck
    slots of the outputs and the padded level vectors.  nPlanck counts every source-only slot of the thermal slot, the Planck
    tables and the skin tables of a SurfaceEmission alike (SceneLin.nSrc; thermal_estimate(model) gives both arguments)."""
    layer = (1 + P) * (4 * N * N + 2 * N)
    elems = (n_tops * (1 + pl) * (N * N + N) + (2 * layer if segments else 0) + 3 * layer + Nz * (8 + 3 * P)
             + n_levels * 2 * (1 + P) * n_stokes * nV + 4 * (1 + P) * N)
    if thermal:
        fwd_layer = 4 * N * N + 2 * N
        elems += (n_tops * (1 + pl) * (N * N + N) + 3 * layer + (5 if segments else 3) * fwd_layer * (1 if nPlanck else 0)
                  + n_levels * 2 * nPlanck * (N + n_stokes * nV) + Nz * (1 + nPlanck) + 4 * (1 + P + nPlanck) * N)
    return elems * itemsize


def thermal_estimate(model: H.RTModel) -> dict:
    """The thermal keywords of bytes_per_point (here and in core_rt_flux_lin.py) for a model, on the safe side: thermal=True for
    any ThermalEmission or SurfaceEmission, nPlanck = the Planck tables + the skin tables, SceneLin.nSrc.  {} for a model without
    the sources, which takes the estimate as it always was."""
    th = [s_ for s_ in (model.sources or ()) if isinstance(s_, H.ThermalEmission)]
    se = H.surface_emission_of(model)
    if not th and se is None:
        return {}
    Bd = getattr(th[0], "B_layer_dot", None) if th else None
    return dict(thermal=True, nPlanck=(0 if Bd is None else int(Bd.shape[0])) + (se.nSkin if se is not None else 0))


def rt_run_multisensor(model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int, sensor_levels, streams: bool = False,
                       max_points: Optional[int] = None):
    """Radiances and Jacobians at any level of the column: (uw, dw, uw_dot, dw_dot), lists with one entry per item of
    `sensor_levels`, in the caller's order: uw / dw [nVZA, nStokes, nSpec] as in CoreRT.rt_run_multisensor, uw_dot / dw_dot
    [nVZA, nStokes, nSpec, Nparams] with the parameter slots of rt_run_lin (7 per aerosol, the gases, the surface).

    Levels as in CoreRT.rt_run_multisensor: 0 = TOA, l = below layer l, Nz = just above the surface (the surface layer alone as the
    bottom); duplicates and any order allowed, each distinct level computed once.  Level 0 is (R, T, Rdot, Tdot) of
    SceneLin.run(lanes=1, fold=False) on the same scene bit for bit (rt_run_lin's default lanes / folded walk agree with it to
    rounding).  Model arguments, surfaces and NSurf as rt_run_lin takes them (1: Lambertian / Cox-Munk; 4: RPV; 3: Ross-Li; K:
    LambertianSurfaceLegendre / LambertianSurfaceSpline, whose per-point surface layer is the bottom of level Nz).

    streams=True: a MultiSensorLinResult, which also carries the level vectors and their derivatives at all quadrature streams per
    moment.  max_points: run the spectral axis in blocks of about that many points (bit-identical to one pass: points are
    independent, ndoubl and the interface tags come from the full axis; a block has at least SceneLin.LANE_POINTS points where the
    axis has, so that the m = 0 sub-scene applies alike); None = as many as fit the device.
    Sources: model.sources may hold SolarBeam and / or ThermalEmission(B_layer=..., B_layer_dot=...), by rt_run_lin's rule
    (without a SolarBeam F0 = 0).  The source must state B_layer_dot ([0, rows, nSpec] for no Planck slot): this run has no
    `thermal=` keyword, and a ThermalEmission with B_layer_dot = None stays refused with a VSMError, as before.  uw / dw per level are then the sum of the solar and the `:thermal` slot, as in
    CoreRT.rt_run_multisensor(thermal=True); uw_dot / dw_dot are [nVZA, nStokes, nSpec, Nparams + nPlanck]: every slot below Nparams
    is the sum of the solar and the thermal derivative, slot Nparams + k is d/dx_k for B_layer_dot[k] (the thermal part alone),
    after the surface slots as rt_run_lin places them; Nparams + nPlanck <= 64.  The slot exists for m = 0 only; with
    streams=True the derivative level vectors of every moment carry all Nparams + nPlanck slots (zero Planck slots for m > 0).
    Level 0 is again SceneLin.run(lanes=1, fold=False) bit for bit.  SurfaceSIF raises NotImplementedError before anything is
    launched (rt_run_lin takes it).  DESIGN.md §4.8e.

    SurfaceEmission (with or without B_surface_dot, with or without a ThermalEmission) is the emission of the slot's
    lower boundary at every level, level Nz included; its nSkin skin slots follow the Planck slots as further source-only slots:
    uw_dot / dw_dot are [nVZA, nStokes, nSpec, Nparams + nPlanck + nSkin].

    Columns with a non-scattering layer raise NotImplementedError; N <= 128."""
    plan = MS._validate(model, sensor_levels, thermal=True, who="rt_run_multisensor (linearized)")
    # There is no `thermal=` keyword here: a ThermalEmission opts into this run by stating its Planck tables ([0, rows, nSpec] for
    # none).  One that leaves B_layer_dot at None is a forward-only source and is refused as it always was (DESIGN 4.8e "Opt-in").
    fwd_only = [s_ for s_ in (model.sources or ()) if isinstance(s_, H.ThermalEmission) and getattr(s_, "B_layer_dot", None) is None]
    if fwd_only:
        raise _lib.VSMError("rt_run_multisensor (linearized): SolarBeam is the only source of this run beside a ThermalEmission that "
                            "states its Planck tables, B_layer_dot = [nPlanck, rows, nSpec] (nPlanck = 0: no Planck slot); "
                            "got %r with B_layer_dot = None" % (fwd_only[0],))
    qp, pol = model.quad_points, model.polarization_type
    N = qp.Nquad * pol.n
    if N > LEVEL_LIN_MAX_N:
        raise _lib.VSMError("rt_run_multisensor (linearized): N = %d streams x Stokes components > %d, the limit of the linearized "
                            "level kernel (vsm_level_radiance_lin_*)" % (N, LEVEL_LIN_MAX_N))
    S_full = int(np.asarray(model.tau_rayl).shape[0])
    if max_points is None and S_full > 0:
        layout = H.ParameterLayout(n_aerosols=NAer, n_gases=NGas, n_surface=NSurf)
        P, pl = layout.n_total, layout.n_layer_params
        isz, nV = np.dtype(model.float_type).itemsize, len(model.vza)
        per = bytes_per_point(N, P, pl, plan.Nz, plan.n_tops, bool(plan.interior), len(plan.distinct), pol.n, nV, isz,
                              **thermal_estimate(model))
        if CL.REDUCE_M0 and pol.n >= 3:     # (the Stokes_IQ scene of m = 0, where it applies)
            per += bytes_per_point(2 * qp.Nquad, P, pl, plan.Nz, plan.n_tops, bool(plan.interior), len(plan.distinct), 2, nV, isz)
        free, _total = torch.cuda.mem_get_info()
        fit = int(0.5 * free // per)
        if fit < S_full:
            if fit < 1:
                raise _lib.VSMError("rt_run_multisensor (linearized): not even one spectral point fits the device (%d bytes per "
                                    "point)" % per)
            max_points = fit
    # SceneLin takes the Stokes_IQ sub-scene of m = 0 only for batches of at least LANE_POINTS points: where the whole axis has
    # that many, so does every block, or the blocks would round differently
    least = CL.SceneLin.LANE_POINTS if S_full >= CL.SceneLin.LANE_POINTS else 1

    def run_block(sl):
        sc = CL.SceneLin(model, lin_model, NAer, NGas, NSurf, spec_slice=sl)
        MS.refuse_non_scattering(sc.fwd.moments[0]["layers"], sc.FT, "rt_run_multisensor (linearized)",
                                 "; columns with a non-scattering layer are not supported (as for CoreRT.rt_run_multisensor)")
        return _run_scene(sc, plan, bool(streams))
    return MS.gather_blocks(model, plan, MS.spectral_blocks(S_full, max_points, least), run_block,
                            "rt_run_multisensor (linearized)", bool(streams), MultiSensorLinResult)
