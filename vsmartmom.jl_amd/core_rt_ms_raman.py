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
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from . import core_rt_ms as MS
from . import core_rt_raman as RR
from . import host_model as H
from .architectures import synchronize_if_gpu, to_host

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
    S, N = int(dw_full.shape[0]), int(dw_full.shape[1])
    if S == 0:
        return
    dt = dw_full.dtype
    K = int(shift.numel())
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, m, weight, dt)
    bot_stride = 0 if int(bot_R_mp.shape[0]) == 1 and S > 1 else N * N
    P = CR._ptr
    _lib.call("vsm_level_radiance_ie", dt, N, pol.n, S, K, P(shift), len(vza), row0, w, P(top_R_pm), P(bot_R_mp), bot_stride,
              P(dw_full), P(uw_full), P(top_ieR_pm), P(top_ieJ0_p), P(bot_ieR_mp), P(bot_ieJ0_m), P(uwie), P(dwie), P(dwie_full),
              P(uwie_full), CR._stream_ptr())


@dataclass
class MultiSensorRamanResult:
    """rt_run_multisensor(RS_type, ..., streams=True): per entry of sensor_levels the VZA outputs and, per Fourier moment, the level
    vectors at ALL quadrature streams (tuwJ / tdwJ [N, 1, nSpec] of postprocessing_vza_ms!(::RRS), and tuwieJ / tdwieJ summed over
    the lines)."""
    levels: List[int]
    uw: List[np.ndarray]                   # [nVZA, nStokes, nSpec] per level, like rt_run_test_ms's uwJ
    dw: List[np.ndarray]
    uwie: List[np.ndarray]                 # summed over the Raman lines
    dwie: List[np.ndarray]
    uw_streams: List[List[np.ndarray]]     # [level][moment] -> [N, 1, nSpec]
    dw_streams: List[List[np.ndarray]]
    uwie_streams: List[List[np.ndarray]]
    dwie_streams: List[List[np.ndarray]]
    weight: List[float]                    # Fourier weight per moment
    qp_mu: np.ndarray
    i_mu0: int                             # 1-based, like StreamRTResult
    mu0: float
    pol_n: int


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


def _expand_iq(v: torch.Tensor, n: int) -> torch.Tensor:
    """(..., 2 Nquad) level vectors of the Stokes_IQ scene -> (..., n Nquad) with U = V = 0."""
    lead, N2 = tuple(v.shape[:-1]), int(v.shape[-1])
    out = torch.zeros(lead + (N2 // 2, n), dtype=v.dtype, device=v.device)
    out[..., :2] = v.reshape(lead + (N2 // 2, 2))
    return out.reshape(lead + (-1,))


def _run_scene(sc: RR.SceneRRS, levels: List[int], streams: bool):
    """The multi-sensor algorithm on one SceneRRS (its whole extended spectral axis).  Returns ({level: [uw, dw, uwie, dwie]} of
    (S, nStokes, nVZA) device tensors, {m: {level: (uw, dw, uwie, dwie) (S, N)}} or None, the Fourier weights)."""
    model, fwd, FT, dt = sc.model, sc.fwd, sc.FT, sc.dt
    pol, qp, drs = fwd.pol, fwd.qp, sc.drs
    Nz, N, S = fwd.Nz, sc.N, sc.S
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    tops_at = set(interior + ([Nz] if Nz in distinct else []))
    dev = sc.out[0].device
    nV = len(model.vza)
    for t in sc.out:
        t.zero_()
    out = {l: [torch.zeros((S, pol.n, nV), dtype=dt, device=dev) for _ in range(4)] for l in distinct if l != 0}
    out[0] = list(sc.out)
    full = {} if streams else None
    weights = [float(FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)) for m in range(model.m_max + 1)]
    if S == 0:
        return out, full, weights
    reduced = sc.sub0 is not None
    if reduced:      # m = 0 first, like SceneRRS.run: the I, Q rows of the Stokes_IQ scene, the later moments accumulate on top
        sub_out, sub_full, _ = _run_scene(sc.sub0, levels, streams)
        for l in distinct:
            for whole, part in zip(out[l], sub_out[l]):
                whole[:, :2, :].copy_(part)
        if streams:
            full[0] = {l: tuple(_expand_iq(v, pol.n) for v in vs) for l, vs in sub_full[0].items()}
    comp, comp_rs = fwd.composite, sc.comp_rs
    asurf = fwd.added_surface
    segs = [(CR.make_composite_layer(FT, sc.arch, (N, N), S), RR.CompositeLayerRS(FT, sc.arch, sc.drs.K, N, S))
            for _ in range(2 if interior else 0)]
    for mom in fwd.moments:
        m = mom["m"]
        if m == 0 and reduced:
            continue
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        drs.Zpp, drs.Zmp = sc.Zie[m]
        fv = {}
        tops = {}
        # 1. the top pass
        for iz in range(Nz):
            _layer(sc, mom, iz, comp, comp_rs, iz + 1)
            if iz + 1 in tops_at:
                tops[iz + 1] = (comp.R_pm.clone(), comp.J0_p.clone(), comp_rs.ieR_pm.clone(), comp_rs.ieJ0_p.clone())
        CR.create_surface_layer_(model.albedo, asurf, m, fwd.dq, mom["tau_sum_surface"])

        def level(l, bot_R_mp, bot_J0_m, bot_ieR_mp, bot_ieJ0_m):
            A, a, A_ie, a_ie = tops.pop(l)
            dwf = torch.empty((S, N), dtype=dt, device=dev)
            uwf = torch.empty((S, N), dtype=dt, device=dev)
            MS.level_radiance_(pol, qp, model.vza, model.vaz, m, float(weight), A, a, bot_R_mp, bot_J0_m, out[l][0], out[l][1],
                               dwf, uwf)
            dwief = torch.empty((S, N), dtype=dt, device=dev) if streams else None
            uwief = torch.empty((S, N), dtype=dt, device=dev) if streams else None
            level_radiance_ie_(pol, qp, model.vza, model.vaz, m, float(weight), drs.shift, A, bot_R_mp, dwf, uwf, A_ie, a_ie,
                               bot_ieR_mp, bot_ieJ0_m, out[l][2], out[l][3], dwief, uwief)
            if streams:
                fv[l] = (uwf, dwf, uwief, dwief)
        # 4. level Nz: the surface layer alone below it (no inelastic part)
        if Nz in distinct:
            level(Nz, asurf.r_mp, asurf.j0_m, None, None)
        # 2.-4. RS segments and bottoms from the surface up, the level calls of each interior level
        bot = None
        ends = interior[1:] + [Nz]
        tags = [ly["iface"] for ly in mom["layers"]]
        for i, (l, end) in enumerate(reversed(list(zip(interior, ends)))):
            seg, seg_rs = segs[i % 2]
            # seg (+) bot_{k+1} equals the prototype's walk only if that walk applies every layer below `end` with the _11
            # statements: rt_run(RRS)'s _00 / _01 / _10 drop inelastic terms, so they do not associate.  Otherwise this bottom
            # is walked layer by layer down to the surface, as the prototype does.
            walk = bot is not None and not (all(t == "11" for t in tags[end:]) and mom["iface_surface"] in ("11", "10"))
            for iz in range(l, Nz if walk else end):
                _layer(sc, mom, iz, seg, seg_rs, iz - l + 1)
            if bot is None or walk:
                RR.interaction_inelastic_(drs, mom["iface_surface"], seg, seg_rs, asurf, sc.surf_rs)
            else:
                RR.interaction_inelastic_(drs, "11", seg, seg_rs, MS._CompositeAsAdded(bot[0]), _CompositeRSAsAdded(bot[1]))
            level(l, seg.R_mp, seg.J0_m, seg_rs.ieR_mp, seg_rs.ieJ0_m)
            bot = (seg, seg_rs)
        # level 0: SceneRRS.run's surface interaction and post-processing
        RR.interaction_inelastic_(drs, mom["iface_surface"], comp, comp_rs, asurf, sc.surf_rs)
        RR.postprocessing_vza_rs_(pol, comp, comp_rs, model.vza, model.vaz, qp, m, float(weight), *sc.out)
        if streams:
            fv[0] = (comp.J0_m.clone(), comp.J0_p.clone(), comp_rs.ieJ0_m.sum(dim=0), comp_rs.ieJ0_p.sum(dim=0))
            full[m] = fv
    return out, full, weights


def _validate(RS_type: RR.RRS, model: H.RTModel, sensor_levels, iBand: int):
    levels, Nz = MS._validate(model, sensor_levels)
    if iBand != 1:
        raise _lib.VSMError("rt_run_multisensor (RRS): single-band models only (iBand = 1), got %r" % (iBand,))
    N = model.quad_points.Nquad * model.polarization_type.n
    if N > LEVEL_IE_MAX_N:
        raise _lib.VSMError("rt_run_multisensor (RRS): N = %d streams x Stokes components > %d, the limit of the inelastic level "
                            "kernel (vsm_level_radiance_ie_*)" % (N, LEVEL_IE_MAX_N))
    return levels, Nz


def rt_run_multisensor(RS_type: RR.RRS, model: H.RTModel, sensor_levels, iBand: int = 1, streams: bool = False,
                       max_points: Optional[int] = None):
    """rt_run_test_ms(::RRS, sensor_levels, model, iBand) (rt_run_multisensor.jl): (uw, dw, uwie, dwie), lists with one
    [nVZA, nStokes, nSpec] host array per entry of `sensor_levels`, in the caller's order; uwie / dwie are summed over the Raman
    lines (postprocessing_vza_ms!(::RRS)).

    Levels as in CoreRT.rt_run_multisensor: 0 = TOA, l = below layer l, Nz = just above the surface (the surface layer alone as the
    bottom, whose inelastic part is zero: DESIGN.md §6); duplicates and any order allowed, each distinct level computed once.  Level
    0 is CoreRTRaman.rt_run(RS_type, model)'s (R_SFI, T_SFI, ieR_SFI, ieT_SFI) bit for bit.  Columns with non-scattering layers
    run (both reference RRS drivers hard-wire scatter = true) with rt_run(RRS)'s convention for the _00 / _01 / _10 tags.

    streams=True: a MultiSensorRamanResult, which also carries the level vectors at all quadrature streams per moment.
    max_points: walk the recipient axis in blocks of at most that many points, each extended by the halo of max|shift| donor
    points (bit-identical to the one-pass run: a recipient reads only elastic fields of its donors, its level vectors included);
    None = as many as fit the device (raman_bytes_per_point with the kept tops and the two segment composites).
    SolarBeam sources only; N <= 128."""
    levels, Nz = _validate(RS_type, model, sensor_levels, iBand)
    S_full = int(model.tau_rayl.shape[0])
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    n_tops = len(interior) + (1 if Nz in distinct else 0)
    shifts = np.asarray(RS_type.i_lambda1lambda0).ravel()
    if max_points is None and S_full > 0:
        qp, pol = model.quad_points, model.polarization_type
        N, K, isz = qp.Nquad * pol.n, len(shifts), np.dtype(model.float_type).itemsize
        per = RR.raman_bytes_per_point(N, K, isz, n_tops=n_tops, segments=bool(interior))
        if RR.REDUCE_M0 and pol.n >= 3:
            per += RR.raman_bytes_per_point(2 * qp.Nquad, K, isz, n_tops=n_tops, segments=bool(interior))
        free, _total = torch.cuda.mem_get_info()
        halo = max([abs(int(x)) for x in shifts if abs(int(x)) < S_full] or [0])
        fit = int(0.8 * free // per) - 2 * halo
        if fit < S_full:
            if fit < 1:
                raise _lib.VSMError("rt_run_multisensor (RRS): not even one block of recipient points fits the device (%d bytes "
                                    "per point, halo %d)" % (per, halo))
            max_points = fit
    if max_points is None or max_points >= S_full:
        blocks = [None]
    else:
        blocks = [slice(b0, min(b0 + int(max_points), S_full)) for b0 in range(0, S_full, int(max_points))]
    parts = []
    weights = None
    for sl in blocks:
        sc = RR.SceneRRS(RS_type, model, iBand, sl)
        out, full, weights = _run_scene(sc, levels, bool(streams))
        synchronize_if_gpu()
        _lib.check_device_status("rt_run_multisensor (RRS)")
        crop = sc.crop
        res = {l: [to_host(t[crop]).transpose(2, 1, 0).copy() for t in out[l]] for l in distinct}
        vec = None
        if streams:
            vec = {m: {l: [to_host(v[crop]).T[:, None, :].copy() for v in vs] for l, vs in fv.items()} for m, fv in full.items()}
        parts.append((res, vec))
        del sc
        if len(blocks) > 1:
            torch.cuda.empty_cache()
    cat = (lambda xs: xs[0]) if len(parts) == 1 else (lambda xs: np.concatenate(xs, axis=-1))
    res = {l: [cat([p[0][l][i] for p in parts]) for i in range(4)] for l in distinct}
    outs = tuple([res[l][i].copy() for l in levels] for i in range(4))
    if not streams:
        return outs
    ms = sorted(parts[0][1])
    st = [[[cat([p[1][m][l][i] for p in parts]) for m in ms] for l in levels] for i in range(4)]
    qp = model.quad_points
    return MultiSensorRamanResult(levels, *outs, *st, weights, np.asarray(qp.qp_mu, dtype=model.float_type).copy(),
                                  int(qp.imu0) + 1, float(qp.mu0), model.polarization_type.n)
