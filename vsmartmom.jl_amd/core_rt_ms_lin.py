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
"""
from __future__ import annotations

import ctypes as C
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


@dataclass
class MultiSensorLinResult(MS.MultiSensorResult):
    """rt_run_multisensor(model, lin_model, ..., streams=True): per entry of sensor_levels the VZA outputs and their Jacobians and,
    per Fourier moment, the level vectors and their derivatives at ALL quadrature streams: the fields of MultiSensorResult and"""
    uw_dot: List[np.ndarray]                # [nVZA, nStokes, nSpec, Nparams] per level
    dw_dot: List[np.ndarray]
    uw_dot_streams: List[List[np.ndarray]]  # [level][moment] -> [N, 1, nSpec, Nparams]
    dw_dot_streams: List[List[np.ndarray]]

    FIELDS = ("uw", "dw", "uw_dot", "dw_dot")


def _run_scene(sc: CL.SceneLin, plan: MS.LevelPlan, streams: bool):
    """The linearized multi-sensor algorithm on one SceneLin.  Returns ({level: [uw, dw, uw_dot, dw_dot]} of (S, nStokes, nVZA) /
    (P, S, nStokes, nVZA) device tensors, {m: {level: (uw, dw, uw_dot, dw_dot) (S, N) / (P, S, N)}} or None, the Fourier weights)."""
    model, fwd, FT, dt = sc.model, sc.fwd, sc.FT, sc.dt
    pol, qp = sc.pol, sc.qp
    N, S, P, pl = sc.N, sc.S, sc.P, sc.pl
    w = sc._lane_state(0)
    torch._foreach_zero_([w["R"], w["T"], w["Rd"], w["Td"]])
    dev = sc.R.device
    nV = len(model.vza)
    z = lambda *sh: torch.zeros(sh, dtype=dt, device=dev)
    out = {l: [z(S, pol.n, nV), z(S, pol.n, nV), z(P, S, pol.n, nV), z(P, S, pol.n, nV)] for l in plan.distinct if l != 0}
    out[0] = [sc.R, sc.T, sc.Rd, sc.Td]
    full = {} if streams else None
    weights = [float(MS.fourier_weight(FT, m)) for m in range(model.m_max + 1)]
    if S == 0:
        return out, full, weights
    reduced = sc.sub0 is not None
    if reduced:      # m = 0 first, like SceneLin.run
        MS.merge_sub0(_run_scene(sc.sub0, plan, streams), pol.n, out, full)
    segs = [(CR.make_composite_layer(FT, sc.arch, (N, N), S), CL.CompositeLayerLin(FT, sc.arch, P, N, S))
            for _ in range(2 if plan.interior else 0)]
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

        def run_segment(seg, first, end):
            for iz in range(first, end):
                sc._double_layer(mom, iz, w)
                if iz == first:
                    CR.copy_added_to_composite_(seg[0], w["added"])
                    a_, c_ = w["al"].cstruct(), seg[1].cstruct()
                    _lib.call("vsm_copy_added_to_composite_lin", dt, N, S, C.byref(a_), C.byref(c_), CR._stream_ptr())
                else:
                    CL.interaction_lin_(mom["layers"][iz]["iface"], seg[0], seg[1], w["added"], w["al"], p_range=sc._layer_slots)

        def level(l, seg):
            top = tops.pop(l)
            bot = (asurf.r_mp, asurf.j0_m, als.ap_r_mp, als.ap_J0_m) if seg is None else (seg[0].R_mp, seg[0].J0_m, seg[1].R_mp,
                                                                                          seg[1].J0_m)
            vs = MS.level_pair_(pol, qp, model.vza, model.vaz, m, weight, top, bot[0], bot[1], out[l],
                                lambda dwf, uwf, dwdf, uwdf: level_radiance_lin_(
                                    pol, qp, model.vza, model.vaz, m, weight, P, pl, top[0], bot[0], dwf, uwf, top[2], top[3],
                                    bot[2], bot[3], out[l][2], out[l][3], dwdf, uwdf), (P, S, N), streams)
            if streams:
                fv[l] = vs
        # 2.-4. linearized segments and bottoms from the surface up, the level calls of each level
        MS.walk_levels(plan, segs, run_segment,
                       lambda seg: CL.interaction_lin_(mom["iface_surface"], seg[0], seg[1], asurf, als),
                       lambda seg, bot, first, end: CL.interaction_lin_("11", seg[0], seg[1], CL._CompositeAsAdded(bot[0]),
                                                                        CL._CompositeLinAsAdded(bot[1])), level)
        if streams:
            full[m] = fv
    return out, full, weights


def bytes_per_point(N: int, P: int, pl: int, Nz: int, n_tops: int, segments: bool, n_levels: int, n_stokes: int, nV: int,
                    itemsize: int) -> int:
    """Device bytes per spectral point of a linearized multi-sensor run (an estimate on the safe side): the kept tops, the two
    segment composites, the scene's own added / composite / surface layers, its per-layer optics and the outputs."""
    layer = (1 + P) * (4 * N * N + 2 * N)
    elems = (n_tops * (1 + pl) * (N * N + N) + (2 * layer if segments else 0) + 3 * layer + Nz * (8 + 3 * P)
             + n_levels * 2 * (1 + P) * n_stokes * nV + 4 * (1 + P) * N)
    return elems * itemsize


def rt_run_multisensor(model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int, sensor_levels, streams: bool = False,
                       max_points: Optional[int] = None):
    """Radiances and Jacobians at any level of the column: (uw, dw, uw_dot, dw_dot), lists with one entry per item of
    `sensor_levels`, in the caller's order: uw / dw [nVZA, nStokes, nSpec] as in CoreRT.rt_run_multisensor, uw_dot / dw_dot
    [nVZA, nStokes, nSpec, Nparams] with the parameter slots of rt_run_lin (7 per aerosol, the gases, the surface).

    Levels as in CoreRT.rt_run_multisensor: 0 = TOA, l = below layer l, Nz = just above the surface (the surface layer alone as the
    bottom); duplicates and any order allowed, each distinct level computed once.  Level 0 is (R, T, Rdot, Tdot) of
    SceneLin.run(lanes=1, fold=False) on the same scene bit for bit (rt_run_lin's default lanes / folded walk agree with it to
    rounding).  Model arguments, surfaces and NSurf as rt_run_lin takes them (1: Lambertian / Cox-Munk; 4: RPV; 3: Ross-Li).

    streams=True: a MultiSensorLinResult, which also carries the level vectors and their derivatives at all quadrature streams per
    moment.  max_points: run the spectral axis in blocks of about that many points (bit-identical to one pass: points are
    independent, ndoubl and the interface tags come from the full axis; a block has at least SceneLin.LANE_POINTS points where the
    axis has, so that the m = 0 sub-scene applies alike); None = as many as fit the device.
    SolarBeam sources only; columns with a non-scattering layer raise NotImplementedError; N <= 128."""
    plan = MS._validate(model, sensor_levels)
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
        per = bytes_per_point(N, P, pl, plan.Nz, plan.n_tops, bool(plan.interior), len(plan.distinct), pol.n, nV, isz)
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
