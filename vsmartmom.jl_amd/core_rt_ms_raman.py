"""Multi-sensor runs with rotational Raman scattering: elastic and inelastic radiances at any level of the column.

Mirrors rt_run_test_ms(::RRS, sensor_levels, model, iBand) (src/CoreRT/rt_run_multisensor.jl) -- the reference's prototype driver
with rt_kernel_multisensor!(::RRS) (CoreKernel/rt_kernel_multisensor.jl:146-283), interaction_top! / interaction_bot! and
interaction_helper_ms!(::RRS, ...) (CoreKernel/interaction_multisensor.jl:248-640, 778-893), interlayer_flux_helper!(::RRS)
(CoreKernel/interlayer_flux.jl:21-77) and postprocessing_vza_ms!(::RRS) (tools/postprocessing_vza_ms.jl:55-118) -- with the
algorithm of the elastic multi-sensor run (core_rt_ms.py) on RS composites.  Per Fourier moment:

  1. top pass: SceneRRS.run's layer walk; after layer l_k the composite's R+-, J0+, ieR+- and ieJ0+ are kept as the top of level
     l_k, before the surface interaction as the top of level Nz; the surface interaction and post-processing give level 0
     (= CoreRTRaman.rt_run's R_SFI, T_SFI, ieR_SFI, ieT_SFI bit for bit, the Stokes_IQ reduction of m = 0 included);
  2. segments: layers l_k+1 .. l_{k+1} run through rt_kernel_rrs_ into an RS composite of their own (the first a copy, every layer
     with its absolute tau_sum, fScattRayleigh row and interface tag);
  3. bottoms from the surface up: bot_K = seg_K (+) surface, bot_k = seg_k (+) bot_{k+1} (interaction_inelastic_ with the lower
     composite handed over as an added-layer record, elastic AND inelastic arrays);
  4. per level one elastic level call (vsm_level_radiance_*, its level vectors at all streams are the donor vectors) and one
     inelastic one (vsm_level_radiance_ie_*, the lines summed before one solve per recipient point).

Adding is associative in the first-order Raman algebra (X + eps X_ie, eps^2 = 0), so the segmented order equals the prototype's
per-sensor walk up to rounding.  Per moment: Nz + (Nz - l_1) RRS layer steps, L + 1 further interactions (L interior levels) and at
most 2 (L + 1) level calls.  rt_run(RRS)'s statements for the _00 / _01 / _10 tags (non-scattering layers) drop inelastic terms
and do not associate: a bottom whose lower part holds such a tag is walked layer by layer to the surface instead, like the
prototype's interaction_bot! (Nz - l_k more layer steps for that level).

_run_scene is the one Raman walk.  A run that wants something else than radiances at each level hands it a LevelSink, which
takes the place of the level calls: CoreRTRaman.rt_run_fluxes (core_rt_flux_raman.py) walks m = 0 alone and reduces the elastic
and the inelastic level vectors to fluxes on the device.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from . import core_rt_ms as MS
from . import core_rt_raman as RR
from . import host_model as H

LEVEL_IE_MAX_N = 128   # vsm_level_radiance_ie_*: one workgroup per recipient point; there is no operator-level twin


class _CompositeRSAsAdded:
    """A CompositeLayerRS handed to interaction_inelastic_ as the LOWER operand: a vsm_added_rs record over its six arrays (every
    RS array is per point, [N,N,S,K] / [N,1,S,K], for layers and composites alike)."""

    def __init__(self, comp_rs: RR.CompositeLayerRS):
        self.c = comp_rs
        self.K, self.N, self.nSpec, self.dtype = comp_rs.K, comp_rs.N, comp_rs.nSpec, comp_rs.dtype

    def cstruct(self):
        c = self.c
        return _lib.vsm_added_rs(c.ieR_mp.data_ptr(), c.ieT_pp.data_ptr(), c.ieR_pm.data_ptr(), c.ieT_mm.data_ptr(),
                                 c.ieJ0_p.data_ptr(), c.ieJ0_m.data_ptr(), c.K, 0)


def level_radiance_ie_(pol, qp, vza, vaz, m: int, weight: float, shift, top_R_pm, bot_R_mp, dw_full, uw_full, top_ieR_pm,
                       top_ieJ0_p, bot_ieR_mp, bot_ieJ0_m, uwie, dwie, dwie_full=None, uwie_full=None):
    """The inelastic level equation at one boundary (the first-order part of interlayer_flux_helper!(::RRS), lines summed, + the
    VZA rows of postprocessing_vza_ms!(::RRS)): uwie / dwie (S, n, nV) layout tensors += weight * rows of
        q = sum_k [c_ie,k + B_ie,k dw(n0)],  dw_ie = (I - A B)^-1 (sum_k [a_ie,k + A_ie,k uw(n0)] + A q),  uw_ie = q + B dw_ie
    A = top_R_pm (S, N, N), B = bot_R_mp ((S | 1, N, N)), dw_full / uw_full (S, N) the elastic level vectors, top_ieR_pm /
    bot_ieR_mp (K, S, N, N), top_ieJ0_p / bot_ieJ0_m (K, S, N); bot_ieR_mp = bot_ieJ0_m = None: a bottom without an inelastic part."""
    setup = MS.level_call_setup(pol, qp, vza, vaz, m, weight, dw_full, bot_R_mp)
    if setup is None:
        return
    S, N, dt, row0, w, bot_stride = setup
    K = int(shift.numel())
    P = CR._ptr
    _lib.call("vsm_level_radiance_ie", dt, N, pol.n, S, K, P(shift), len(vza), row0, w, P(top_R_pm), P(bot_R_mp), bot_stride,
              P(dw_full), P(uw_full), P(top_ieR_pm), P(top_ieJ0_p), P(bot_ieR_mp), P(bot_ieJ0_m), P(uwie), P(dwie), P(dwie_full),
              P(uwie_full), CR._stream_ptr())


@dataclass
class MultiSensorRamanResult(MS.MultiSensorResult):
    """rt_run_multisensor(RS_type, ..., streams=True): per entry of sensor_levels the VZA outputs and, per Fourier moment, the level
    vectors at ALL quadrature streams (tuwJ / tdwJ [N, 1, nSpec] of postprocessing_vza_ms!(::RRS), and tuwieJ / tdwieJ summed over
    the lines): the fields of MultiSensorResult and"""
    uwie: List[np.ndarray]                 # [nVZA, nStokes, nSpec] per level, summed over the Raman lines
    dwie: List[np.ndarray]
    uwie_streams: List[List[np.ndarray]]   # [level][moment] -> [N, 1, nSpec]
    dwie_streams: List[List[np.ndarray]]

    FIELDS = ("uw", "dw", "uwie", "dwie")


def _layer(sc: RR.SceneRRS, mom, iz: int, comp, comp_rs, iz_local: int):
    """Layer iz (0-based) of moment `mom` through rt_kernel!(::RRS) into (comp, comp_rs) as its layer iz_local (1 = a copy): the
    statements of SceneRRS.run's walk."""
    fwd, dt = sc.fwd, sc.dt
    ly = mom["layers"][iz]
    sc.drs.fscatt = sc.fscatt[iz]
    mu0 = C.c_double(fwd.qp.mu0) if dt == torch.float64 else C.c_float(fwd.qp.mu0)
    _lib.call("vsm_layer_expk", dt, sc.S, CR._ptr(ly["dtau"]), mu0, CR._ptr(sc.expk), CR._stream_ptr())
    RR.rt_kernel_rrs_(sc.drs, fwd.pol, fwd.added, sc.added_rs, comp, comp_rs, ly["props"].materialize(), ly["tau_sum"], mom["m"],
                      fwd.dq, sc.arch, iz_local, fwd.F0, sc.FT, sc.model.numerics, dtau=ly["dtau"], ndoubl=ly["nd"], expk=sc.expk,
                      iface=ly["iface"])


class LevelSink:
    """What a run other than the multi-sensor one does at each level of the walk of _run_scene, in place of its level calls
    (core_rt_flux_raman.py: the fluxes), as core_rt_ms.LevelSink does for the elastic walk.  With a sink no VZA output is
    allocated or zeroed, no level call and no post-processing is issued here and no level vector is collected; the walk itself --
    tops, segments, bottoms -- is the same, and level 0 is walked only if the plan asks for it.  The scene handed over is the one
    that walks the moment: there is no Stokes_IQ detour here (the caller passes SceneRRS.sub0 itself where it wants that)."""

    def level(self, mom, l, top, bot):
        """Level l > 0: top = (R+-, J0+, ieR+-, ieJ0+) of the composite above it, bot = (R-+, J0-, ieR-+, ieJ0-) of the one below
        (the last two None: the surface layer alone)."""
        raise NotImplementedError

    def level0(self, mom, comp, comp_rs):
        """Level 0, the TOA: the composite of the whole column after the surface interaction."""
        raise NotImplementedError


def _run_scene(sc: RR.SceneRRS, plan: MS.LevelPlan, streams: bool, sink: Optional[LevelSink] = None):
    """The multi-sensor algorithm on one SceneRRS (its whole extended spectral axis).  Returns ({level: [uw, dw, uwie, dwie]} of
    (S, nStokes, nVZA) device tensors, {m: {level: (uw, dw, uwie, dwie) (S, N)}} or None, the Fourier weights); with a sink (see
    LevelSink) the first is empty and streams is not taken."""
    model, fwd, FT, dt = sc.model, sc.fwd, sc.FT, sc.dt
    pol, qp, drs = fwd.pol, fwd.qp, sc.drs
    Nz, N, S = fwd.Nz, sc.N, sc.S
    dev = sc.out[0].device
    nV = len(model.vza)
    if sink is None:
        for t in sc.out:
            t.zero_()
        out = {l: [torch.zeros((S, pol.n, nV), dtype=dt, device=dev) for _ in range(4)] for l in plan.distinct if l != 0}
        out[0] = list(sc.out)
    else:
        out = {}
    full = {} if streams and sink is None else None
    weights = [float(MS.fourier_weight(FT, m)) for m in range(model.m_max + 1)]
    if S == 0:
        return out, full, weights
    reduced = sc.sub0 is not None and sink is None
    if reduced:      # m = 0 first, like SceneRRS.run
        MS.merge_sub0(_run_scene(sc.sub0, plan, streams), pol.n, out, full)
    comp, comp_rs = fwd.composite, sc.comp_rs
    asurf = fwd.added_surface
    segs = [(CR.make_composite_layer(FT, sc.arch, (N, N), S), RR.CompositeLayerRS(FT, sc.arch, sc.drs.K, N, S))
            for _ in range(2 if plan.interior else 0)]
    for mom in fwd.moments:
        m = mom["m"]
        if m == 0 and reduced:
            continue
        weight = float(MS.fourier_weight(FT, m))
        drs.Zpp, drs.Zmp = sc.Zie[m]
        fv = {}
        tops = {}
        # 1. the top pass
        for iz in range(Nz):
            _layer(sc, mom, iz, comp, comp_rs, iz + 1)
            if iz + 1 in plan.tops_at:
                tops[iz + 1] = (comp.R_pm.clone(), comp.J0_p.clone(), comp_rs.ieR_pm.clone(), comp_rs.ieJ0_p.clone())
        CR.create_surface_layer_(model.surface, asurf, m, fwd.dq, mom["tau_sum_surface"], rho=mom["rho"])
        tags = [ly["iface"] for ly in mom["layers"]]

        def layers(seg, first, lo, hi):      # layers lo+1 .. hi into seg, a composite that starts with layer first+1
            for iz in range(lo, hi):
                _layer(sc, mom, iz, seg[0], seg[1], iz - first + 1)

        def join_surface(seg):
            RR.interaction_inelastic_(drs, mom["iface_surface"], seg[0], seg[1], asurf, sc.surf_rs)

        def join_bottom(seg, bot, first, end):
            # seg (+) bot equals the prototype's walk only if that walk applies every layer below `end` with the _11 statements:
            # rt_run(RRS)'s _00 / _01 / _10 drop inelastic terms, so they do not associate.  Otherwise this bottom is walked
            # layer by layer down to the surface, as the prototype does.
            if all(t == "11" for t in tags[end:]) and mom["iface_surface"] in ("11", "10"):
                RR.interaction_inelastic_(drs, "11", seg[0], seg[1], MS._CompositeAsAdded(bot[0]), _CompositeRSAsAdded(bot[1]))
            else:
                layers(seg, first, end, Nz)
                join_surface(seg)

        def level(l, seg):      # (the surface layer alone has no inelastic part)
            top = tops.pop(l)
            bot = (asurf.r_mp, asurf.j0_m, None, None) if seg is None else (seg[0].R_mp, seg[0].J0_m, seg[1].ieR_mp, seg[1].ieJ0_m)
            if sink is not None:
                sink.level(mom, l, top, bot)
                return
            vs = MS.level_pair_(pol, qp, model.vza, model.vaz, m, weight, top, bot[0], bot[1], out[l],
                                lambda dwf, uwf, dwief, uwief: level_radiance_ie_(
                                    pol, qp, model.vza, model.vaz, m, weight, drs.shift, top[0], bot[0], dwf, uwf, top[2], top[3],
                                    bot[2], bot[3], out[l][2], out[l][3], dwief, uwief), (S, N), streams)
            if streams:
                fv[l] = vs
        # 2.-4. RS segments and bottoms from the surface up, the level calls of each level
        MS.walk_levels(plan, segs, lambda seg, first, end: layers(seg, first, first, end), join_surface, join_bottom, level)
        if sink is not None:      # level 0, the TOA itself: the whole column with the surface
            if 0 in plan.distinct:
                RR.interaction_inelastic_(drs, mom["iface_surface"], comp, comp_rs, asurf, sc.surf_rs)
                sink.level0(mom, comp, comp_rs)
            continue
        # level 0: SceneRRS.run's surface interaction and post-processing
        RR.interaction_inelastic_(drs, mom["iface_surface"], comp, comp_rs, asurf, sc.surf_rs)
        RR.postprocessing_vza_rs_(pol, comp, comp_rs, model.vza, model.vaz, qp, m, weight, *sc.out)
        if streams:
            fv[0] = (comp.J0_m.clone(), comp.J0_p.clone(), comp_rs.ieJ0_m.sum(dim=0), comp_rs.ieJ0_p.sum(dim=0))
            full[m] = fv
    return out, full, weights


def _validate(RS_type: RR.RRS, model: H.RTModel, sensor_levels, iBand: int):
    if any(isinstance(s_, H.SurfaceEmission) for s_ in (model.sources or ())):
        raise NotImplementedError("rt_run_multisensor (RRS): SurfaceEmission is not a source of the Raman runs "
                                  "(CoreRT.rt_run_multisensor(..., thermal=True) takes it)")
    plan = MS._validate(model, sensor_levels, who="rt_run_multisensor (RRS)")
    if iBand != 1:
        raise _lib.VSMError("rt_run_multisensor (RRS): single-band models only (iBand = 1), got %r" % (iBand,))
    N = model.quad_points.Nquad * model.polarization_type.n
    if N > LEVEL_IE_MAX_N:
        raise _lib.VSMError("rt_run_multisensor (RRS): N = %d streams x Stokes components > %d, the limit of the inelastic level "
                            "kernel (vsm_level_radiance_ie_*)" % (N, LEVEL_IE_MAX_N))
    return plan


def rt_run_multisensor(RS_type: RR.RRS, model: H.RTModel, sensor_levels, iBand: int = 1, streams: bool = False,
                       max_points: Optional[int] = None):
    """rt_run_test_ms(::RRS, sensor_levels, model, iBand) (rt_run_multisensor.jl): (uw, dw, uwie, dwie), lists with one
    [nVZA, nStokes, nSpec] host array per entry of `sensor_levels`, in the caller's order; uwie / dwie are summed over the Raman
    lines (postprocessing_vza_ms!(::RRS)).

    Levels as in CoreRT.rt_run_multisensor: 0 = TOA, l = below layer l, Nz = just above the surface (the surface layer alone as the
    bottom, whose inelastic part is zero: DESIGN.md §6); duplicates and any order allowed, each distinct level computed once.  Level
    0 is CoreRTRaman.rt_run(RS_type, model)'s (R_SFI, T_SFI, ieR_SFI, ieT_SFI) bit for bit.  Columns with non-scattering layers
    run (both reference RRS drivers hard-wire scatter = true) with rt_run(RRS)'s convention for the _00 / _01 / _10 tags.

    Surfaces: model.surface, every type CoreRTRaman.rt_run takes (scalar and spectral Lambertian, RPV, Ross-Li, Cox-Munk); like
    CoreRT.rt_run_multisensor, no Cox-Munk single-scattering correction -- over a CoxMunkSurface level 0 is rt_run's field before it.

    streams=True: a MultiSensorRamanResult, which also carries the level vectors at all quadrature streams per moment.
    max_points: walk the recipient axis in blocks of at most that many points, each extended by the halo of max|shift| donor
    points (bit-identical to the one-pass run: a recipient reads only elastic fields of its donors, its level vectors included);
    None = as many as fit the device (raman_bytes_per_point with the kept tops and the two segment composites).
    SolarBeam sources only (SurfaceSIF: NotImplementedError, before anything is launched -- CoreRTRaman.rt_run takes it;
    SurfaceEmission: NotImplementedError as well); N <= 128."""
    plan = _validate(RS_type, model, sensor_levels, iBand)
    S_full = int(model.tau_rayl.shape[0])
    shifts = np.asarray(RS_type.i_lambda1lambda0).ravel()
    if max_points is None and S_full > 0:
        qp, pol = model.quad_points, model.polarization_type
        N, K, isz = qp.Nquad * pol.n, len(shifts), np.dtype(model.float_type).itemsize
        per = RR.raman_bytes_per_point(N, K, isz, n_tops=plan.n_tops, segments=bool(plan.interior))
        if RR.REDUCE_M0 and pol.n >= 3:
            per += RR.raman_bytes_per_point(2 * qp.Nquad, K, isz, n_tops=plan.n_tops, segments=bool(plan.interior))
        free, _total = torch.cuda.mem_get_info()
        halo = max([abs(int(x)) for x in shifts if abs(int(x)) < S_full] or [0])
        fit = int(0.8 * free // per) - 2 * halo
        if fit < S_full:
            if fit < 1:
                raise _lib.VSMError("rt_run_multisensor (RRS): not even one block of recipient points fits the device (%d bytes "
                                    "per point, halo %d)" % (per, halo))
            max_points = fit

    def run_block(sl):      # a SceneRRS over the block and its halo, its outputs cropped to the block
        sc = RR.SceneRRS(RS_type, model, iBand, sl)
        out, full, weights = _run_scene(sc, plan, bool(streams))
        crop = lambda ts: [t[sc.crop] for t in ts]
        return ({l: crop(ts) for l, ts in out.items()},
                full and {m: {l: crop(vs) for l, vs in fv.items()} for m, fv in full.items()}, weights)
    return MS.gather_blocks(model, plan, MS.spectral_blocks(S_full, max_points), run_block, "rt_run_multisensor (RRS)",
                            bool(streams), MultiSensorRamanResult)
