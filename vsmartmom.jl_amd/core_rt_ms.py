"""Multi-sensor runs: radiances at any level of the column, up and down.

Mirrors rt_run_test_ms(::noRS, sensor_levels, model, iBand) (src/CoreRT/rt_run_multisensor.jl) -- the reference's prototype driver
with rt_kernel_multisensor! (CoreKernel/rt_kernel_multisensor.jl:7-143), interaction_top! / interaction_bot!
(CoreKernel/interaction_multisensor.jl:158-240), postprocessing_vza_ms! (tools/postprocessing_vza_ms.jl:7-52) and
compute_interlayer_flux! / interlayer_flux_helper! (CoreKernel/interlayer_flux.jl:1-19, 185-201) -- but not its algorithm: the
prototype runs one interaction per sensor and layer, O(Nz K) for K sensors.  Adding is associative, so here, per Fourier moment:

  1. top pass: the column exactly as Scene.run walks it (native sources-only runs where Scene._native_moments() allows, rt_kernel_
     otherwise); after layer l_k the composite's R+- and J0+ are kept as the top of level l_k, and before the surface interaction
     as the top of level Nz; the surface interaction and post-processing give level 0 (= rt_run's R_SFI / T_SFI);
  2. segments: layers l_k+1 .. l_{k+1} (the last one ends at Nz) run as a composite of their own in full mode, their first layer a
     TOA copy, every layer with its absolute tau_sum (the beam attenuation from the TOA);
  3. bottoms from the surface up: bot_K = seg_K (+) surface, bot_k = seg_k (+) bot_{k+1} (vsm_interaction_* with the lower
     composite handed over as a vsm_added record, d_symmetric = 0, mat_stride = N*N);
  4. one level-kernel call per level (vsm_level_radiance_*), level Nz with the surface layer alone as its bottom.

Per moment: Nz + (Nz - l_1) layer steps, K + 1 further interactions and at most K + 1 level calls.

thermal=True adds the `:thermal` per-source slot of rt_run (CoreRT.ThermalSlot) for m = 0, the one moment an isotropic source
has: the same four steps on thermal composites of its own (ThermalSlot.walk: the top pass keeps J0+ after each level, the
segments need no tau_sum), thermal bottoms built beside the solar ones, and per level ONE call of vsm_level_radiance_src_*, which
solves the solar and the thermal right-hand side on one elimination of [I - A B | .] with A, B of the solar pass (the thermal
composites' own R differ from them only by rounding and are not read).  DESIGN.md §4.8d.

_run is the one elastic walk.  A run that wants something else than radiances at each level hands it a LevelSink, which takes
the place of the level calls: rt_run_fluxes (core_rt_flux.py) walks m = 0 alone and reduces the level vectors to fluxes on the
device.  The linearized walk has the same arrangement (core_rt_ms_lin.LevelSink, core_rt_flux_lin.py).

The Raman (core_rt_ms_raman.py) and linearized (core_rt_ms_lin.py) runs are the same algorithm on their own composites.  What the
three share lives here: the level plan, the walk below the top pass (walk_levels), the two-call level of the runs that solve a
second equation on the elastic level vectors (level_pair_), the Stokes_IQ sub-scene of m = 0 (merge_sub0), the blocks of the
spectral axis and the assembly of the results (spectral_blocks, gather_blocks).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from . import host_model as H
from .architectures import synchronize_if_gpu, to_host

LEVEL_FUSED_MAX_N = 128   # vsm_level_radiance_*: the fused kernel up to N = 128, the operator-level twin above
LEVEL_OPLEVEL = False     # True: every level call on the operator-level twin (tests / tools)


class _CompositeAsAdded:
    """A CompositeLayer handed to interaction_ as the LOWER operand (a vsm_added record over its six arrays): a composite is
    not D-symmetric, so d_symmetric = 0 and every matrix is per point (mat_stride = N*N)."""

    def __init__(self, comp: CR.CompositeLayer):
        self.comp = comp

    def cstruct(self):
        c = self.comp.materialize()._arr
        return _lib.vsm_added(c["R_mp"].data_ptr(), c["T_pp"].data_ptr(), c["R_pm"].data_ptr(), c["T_mm"].data_ptr(),
                              c["J0_p"].data_ptr(), c["J0_m"].data_ptr(), self.comp.N * self.comp.N, 0, 0)


_level_work = {}


def bot_stride_of(bot_R_mp, S: int, N: int) -> int:
    """bot_stride of a level call: 0 for a bottom R-+ of ONE block shared by every point ((1, N, N) with S > 1), else N * N."""
    return 0 if int(bot_R_mp.shape[0]) == 1 and S > 1 else N * N


def level_call_setup(pol, qp, vza, vaz, m: int, weight: float, vec, bot_R_mp):
    """(S, N, dtype, row0, w, bot_stride) of a level call, from one of its (S, N) vectors and the bottom's R-+; None for S = 0."""
    S, N = int(vec.shape[0]), int(vec.shape[1])
    if S == 0:
        return None
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, m, weight, vec.dtype)
    return S, N, vec.dtype, row0, w, bot_stride_of(bot_R_mp, S, N)


def level_radiance_(pol, qp, vza, vaz, m: int, weight: float, top_R_pm, top_J0_p, bot_R_mp, bot_J0_m, uw, dw,
                    dw_full=None, uw_full=None, oplevel: bool = False):
    """The level equation at one boundary (interlayer_flux_helper!, interlayer_flux.jl:1-19, + the VZA rows of
    postprocessing_vza_ms!): uw / dw (S, n, nV) layout tensors += weight * rows of
        dw = (I - A B)^-1 (a + A c),   uw = (I - B A)^-1 (c + B a)  [= c + B dw]
    with A = top_R_pm, a = top_J0_p (S, N[, N]), B = bot_R_mp ((S | 1, N, N): one block shared by every point is bot_stride 0),
    c = bot_J0_m.  dw_full / uw_full: (S, N) tensors that receive the level vectors at all streams."""
    setup = level_call_setup(pol, qp, vza, vaz, m, weight, top_J0_p, bot_R_mp)
    if setup is None:
        return
    S, N, dt, row0, w, bot_stride = setup
    oplevel = oplevel or LEVEL_OPLEVEL
    work = None
    if oplevel or N > LEVEL_FUSED_MAX_N:
        key = (N, S, dt, str(top_J0_p.device))
        work = _level_work.get(key)
        if work is None:
            _level_work.clear()
            work = _lib.poison(torch.empty(int(_lib.lib().vsm_level_radiance_work_elems(N, S)), dtype=dt, device=top_J0_p.device))
            _level_work[key] = work
    name = "vsm_level_radiance_oplevel" if oplevel else "vsm_level_radiance"
    P = CR._ptr
    _lib.call(name, dt, N, pol.n, S, len(vza), row0, w, P(top_R_pm), P(top_J0_p), P(bot_R_mp), bot_stride, P(bot_J0_m), P(uw),
              P(dw), P(dw_full), P(uw_full), P(work), CR._stream_ptr())


def surface_emission_response_(pol, qp, vza, vaz, weight: float, top_R_pm, top_T_mm, bot_R_mp, comps, up, dn,
                               oplevel: bool = False):
    """The response of the column to a unit surface emission in the Stokes components `comps` (a list of K indices), at m = 0
    (vsm_surface_emission_response_*): with A = top_R_pm, T = top_T_mm (R+-, T-- of the atmosphere's composite before the surface
    interaction), B = bot_R_mp (the surface r-+, (S | 1, N, N)) and e_k the unit pattern of component comps[k],
        dw_k = (I - A B)^-1 A e_k,   y_k = e_k + B dw_k,
        up[k] (S, n, nV) = weight * rows of T y_k,   dn[k] (S, n, nV) = weight * rows of dw_k       (written, not accumulated).
    N <= 128: ONE call, one elimination for all K <= 4 right-hand sides.  N > 128 or operator level: one
    vsm_level_radiance_oplevel_* call per component (a = 0, c = e_k, uw_full = y_k, dw_full = dw_k) and a batched row product."""
    S, N = int(top_R_pm.shape[0]), int(top_R_pm.shape[1])
    K, n, nV, dt, dev = len(comps), pol.n, len(vza), top_R_pm.dtype, top_R_pm.device
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, 0, weight, dt)
    P = CR._ptr
    if not (oplevel or LEVEL_OPLEVEL or N > LEVEL_FUSED_MAX_N):
        _lib.call("vsm_surface_emission_response", dt, N, n, S, K, (C.c_int * max(K, 1))(*[int(c) for c in comps]), nV, row0, w,
                  P(top_R_pm), P(top_T_mm), P(bot_R_mp), bot_stride_of(bot_R_mp, S, N), P(up), P(dn), CR._stream_ptr())
        return
    if not 1 <= K <= 4 or any(not 0 <= int(c) < n for c in comps):
        raise _lib.VSMError("surface_emission_response_: %d components %r (1..4 of 0..%d)" % (K, list(comps), n - 1))
    if S == 0 or nV == 0:
        return
    rows = torch.as_tensor([row0[v] + c for c in range(n) for v in range(nV)], dtype=torch.long, device=dev)
    wt = torch.as_tensor([w[v + nV * c] for c in range(n) for v in range(nV)], dtype=dt, device=dev).view(1, n, nV)
    T_rows = top_T_mm[:, :, rows].contiguous()                       # (S, N, n nV): the [n nV, N] row blocks of T--
    zero = torch.zeros((S, N), dtype=dt, device=dev)
    sink = torch.zeros((2, S, n, nV), dtype=dt, device=dev)          # (the call's own VZA rows, without T--: not used)
    for k, c in enumerate(comps):
        e = torch.zeros((S, N), dtype=dt, device=dev)
        e[:, int(c)::n] = 1
        d, y = torch.empty_like(e), torch.empty_like(e)
        level_radiance_(pol, qp, vza, vaz, 0, weight, top_R_pm, zero, bot_R_mp, e, sink[0], sink[1], d, y, oplevel=True)
        up[k].copy_(CR.batched_mul(T_rows, y).view(S, n, nV) * wt)
        dn[k].copy_(d[:, rows].view(S, n, nV) * wt)


LEVEL_MAX_SRC = 4          # VSM_LEVEL_MAX_SRC


def level_radiance_src_(pol, qp, vza, vaz, m: int, weight: float, top_R_pm, tops_J0_p, bot_R_mp, bots_J0_m, uw, dw,
                        dw_full=None, uw_full=None, oplevel: bool = False):
    """level_radiance_ for several sources on the same operators: tops_J0_p / bots_J0_m are lists of (S, N) vectors, one pair per
    source (the solar and the thermal slot); uw / dw and dw_full / uw_full receive the SUM over the sources.  N <= 128: ONE call
    of vsm_level_radiance_src_* (one elimination for all right-hand sides).  N > 128 or operator level: one
    vsm_level_radiance_oplevel_* call per source, the full vectors added here."""
    n_src = len(tops_J0_p)
    if n_src == 0 or n_src != len(bots_J0_m):
        raise _lib.VSMError("level_radiance_src_: %d top and %d bottom source vectors" % (n_src, len(bots_J0_m)))
    setup = level_call_setup(pol, qp, vza, vaz, m, weight, tops_J0_p[0], bot_R_mp)
    if setup is None:
        return
    S, N, dt, row0, w, bot_stride = setup
    oplevel = oplevel or LEVEL_OPLEVEL
    if oplevel or N > LEVEL_FUSED_MAX_N:
        for k, (a, c) in enumerate(zip(tops_J0_p, bots_J0_m)):
            dwk = dw_full if k == 0 or dw_full is None else torch.empty_like(dw_full)
            uwk = uw_full if k == 0 or uw_full is None else torch.empty_like(uw_full)
            level_radiance_(pol, qp, vza, vaz, m, weight, top_R_pm, a, bot_R_mp, c, uw, dw, dwk, uwk, oplevel=oplevel)
            if k and dw_full is not None:
                dw_full += dwk
            if k and uw_full is not None:
                uw_full += uwk
        return
    P = CR._ptr
    pa = (C.c_void_p * n_src)(*[P(t) for t in tops_J0_p])      # (n_src > LEVEL_MAX_SRC: the library refuses before any launch)
    pc = (C.c_void_p * n_src)(*[P(t) for t in bots_J0_m])
    _lib.call("vsm_level_radiance_src", dt, N, pol.n, S, len(vza), row0, w, P(top_R_pm), n_src, pa, P(bot_R_mp), bot_stride, pc,
              P(uw), P(dw), P(dw_full), P(uw_full), None, CR._stream_ptr())


def level_pair_(pol, qp, vza, vaz, m: int, weight: float, top, bot_R_mp, bot_J0_m, out, second, shape2, streams: bool):
    """The level of the Raman and linearized runs: the elastic call (top[0], top[1] = R+-, J0+ of the top) into out[0], out[1],
    then second(dwf, uwf, dw2, uw2), the flavour's call on the elastic level vectors (S, N), with dw2 / uw2 `shape2` tensors for
    its own level vectors if `streams`, else None.  Returns (uwf, dwf, uw2, dw2)."""
    a = top[1]
    S, N = int(a.shape[0]), int(a.shape[1])
    new = lambda *sh: torch.empty(sh, dtype=a.dtype, device=a.device)
    dwf, uwf = new(S, N), new(S, N)
    level_radiance_(pol, qp, vza, vaz, m, weight, top[0], a, bot_R_mp, bot_J0_m, out[0], out[1], dwf, uwf)
    dw2, uw2 = (new(*shape2), new(*shape2)) if streams else (None, None)
    second(dwf, uwf, dw2, uw2)
    return uwf, dwf, uw2, dw2


@dataclass
class MultiSensorResult:
    """rt_run_multisensor(..., streams=True): per entry of sensor_levels the VZA outputs and, per Fourier moment, the level vectors
    at ALL quadrature streams (the arrays postprocessing_vza_ms! reads its rows from: tuwJ / tdwJ [N, 1, nSpec]).  The Raman and
    linearized results add their own fields to these."""
    levels: List[int]
    uw: List[np.ndarray]                 # [nVZA, nStokes, nSpec] per level, like rt_run_test_ms's uwJ
    dw: List[np.ndarray]
    uw_streams: List[List[np.ndarray]]   # [level][moment] -> [N, 1, nSpec]
    dw_streams: List[List[np.ndarray]]
    weight: List[float]                  # Fourier weight per moment
    qp_mu: np.ndarray
    i_mu0: int                           # 1-based, like StreamRTResult
    mu0: float
    pol_n: int

    FIELDS = ("uw", "dw")                # the outputs of a run, in the order rt_run_multisensor returns them


@dataclass(frozen=True)
class LevelPlan:
    """Which levels a run computes and how the column splits into segments between them."""
    levels: List[int]      # the caller's sensor_levels, validated
    distinct: List[int]    # sorted, each once
    interior: List[int]    # those with 0 < l < Nz
    tops_at: List[int]     # the levels whose top composite is kept: interior, and Nz if asked for
    ends: List[int]        # per interior level, the last layer of the segment below it (the next interior level, or Nz)
    Nz: int

    @property
    def n_tops(self) -> int:
        return len(self.tops_at)


def _validate(model: H.RTModel, sensor_levels, thermal: bool = False, sif: bool = False,
              who: str = "rt_run_multisensor") -> LevelPlan:
    """The level plan of a run.  thermal: ThermalEmission and SurfaceEmission are accepted beside (or instead of) SolarBeam --
    rt_run_multisensor's thermal=True; the Raman run leaves it off.  sif: SurfaceSIF is accepted too (CoreRT.rt_run_multisensor alone:
    the Raman and the linearized multi-sensor run refuse it with NotImplementedError, before anything is launched)."""
    Nz = int(np.asarray(model.tau_rayl).shape[1])
    levels = []
    for l in sensor_levels:
        if isinstance(l, (bool, np.bool_)) or int(l) != l:
            raise ValueError("sensor levels are integers (layer boundaries counted from the TOA), got %r" % (l,))
        if not 0 <= int(l) <= Nz:
            raise ValueError("sensor level %d outside 0..Nz = 0..%d (0 = TOA, Nz = just above the surface)" % (int(l), Nz))
        levels.append(int(l))
    if not levels:
        raise ValueError("rt_run_multisensor: no sensor level given")
    srcs = tuple(model.sources) if model.sources is not None else (H.SolarBeam(),)
    if not sif and any(isinstance(s, H.SurfaceSIF) for s in srcs):
        raise NotImplementedError("%s: SurfaceSIF is not a source of this run (CoreRT.rt_run_multisensor takes it)" % who)
    accepted = (((H.SolarBeam, H.ThermalEmission, H.SurfaceEmission) if thermal else (H.SolarBeam,))
                + ((H.SurfaceSIF,) if sif else ()))
    other = [s for s in srcs if not isinstance(s, accepted)]
    if other or not srcs:
        if thermal:
            raise _lib.VSMError("rt_run_multisensor(thermal=True): SolarBeam, ThermalEmission and SurfaceEmission are the sources of "
                                "a multi-sensor run; got %r" % (other[0] if other else None,))
        raise _lib.VSMError("rt_run_multisensor: SolarBeam is the only source of a multi-sensor run (the prototype passes F0 alone, "
                            "rt_kernel_multisensor.jl:21; CoreRT.rt_run_multisensor(..., thermal=True) also takes ThermalEmission "
                            "and SurfaceEmission); got %r" % (other[0] if other else None,))
    if thermal:
        H.surface_emission_of(model)      # (its shape against the model, before anything is launched)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    return LevelPlan(levels, distinct, interior, interior + ([Nz] if Nz in distinct else []), interior[1:] + [Nz], Nz)


fourier_weight = CR.fourier_weight


def refuse_non_scattering(layers, FT, who: str, why: str):
    eps2 = 2 * np.finfo(FT).eps
    noscat = [iz + 1 for iz, ly in enumerate(layers) if ly["props"].max_tau_varpi <= eps2]
    if noscat:
        raise NotImplementedError("%s: layer %d does not scatter (tau * varpi <= 2 eps)%s" % (who, noscat[0], why))


def walk_levels(plan: LevelPlan, segs, run_segment, join_surface, join_bottom, level):
    """The levels of one moment below the top pass (steps 2.-4.): level Nz against the surface layer alone, then the interior
    levels from the surface up, their bottoms on the two alternating segment composites `segs`.  The flavour supplies
        run_segment(seg, first, end)        layers first+1 .. end into seg, the first a copy
        join_surface(seg)                   seg (+) surface
        join_bottom(seg, bot, first, end)   seg (+) bot, the previous bottom (layers end+1 .. Nz and the surface)
        level(l, seg)                       the level call(s) of level l on the bottom seg; seg None: the surface layer alone"""
    if plan.Nz in plan.distinct:
        level(plan.Nz, None)
    bot = None
    for i, (l, end) in enumerate(reversed(list(zip(plan.interior, plan.ends)))):
        seg = segs[i % 2]
        run_segment(seg, l, end)
        if bot is None:
            join_surface(seg)
        else:
            join_bottom(seg, bot, l, end)
        level(l, seg)
        bot = seg


def _expand_iq(v: torch.Tensor, n: int) -> torch.Tensor:
    """(..., 2 Nquad) level vectors of the Stokes_IQ scene -> (..., n Nquad) with U = V = 0."""
    lead, N2 = tuple(v.shape[:-1]), int(v.shape[-1])
    out = torch.zeros(lead + (N2 // 2, n), dtype=v.dtype, device=v.device)
    out[..., :2] = v.reshape(lead + (N2 // 2, 2))
    return out.reshape(lead + (-1,))


def merge_sub0(sub, n: int, out, full):
    """m = 0 from the Stokes_IQ sub-scene: sub = (out, full, weights) of the whole algorithm run on it.  Its I, Q rows are copied
    into every level of `out`, where the later moments accumulate on top; its level vectors, expanded to n components, are full[0]."""
    sub_out, sub_full, _ = sub
    for l, parts in sub_out.items():
        for whole, part in zip(out[l], parts):
            whole[..., :2, :].copy_(part)
    if full is not None:
        full[0] = {l: tuple(_expand_iq(v, n) for v in vs) for l, vs in sub_full[0].items()}


def spectral_blocks(S_full: int, max_points, least: int = 1):
    """The spectral axis in blocks of max_points points (None or >= S_full: one block, None); no block shorter than `least`: the
    last one absorbs a shorter tail."""
    if max_points is None or max_points >= S_full:
        return [None]
    bs = max(int(max_points), least)
    blocks = [slice(b0, min(b0 + bs, S_full)) for b0 in range(0, S_full, bs)]
    if len(blocks) > 1 and blocks[-1].stop - blocks[-1].start < least:
        blocks[-2:] = [slice(blocks[-2].start, S_full)]
    return blocks


def gather_blocks(model: H.RTModel, plan: LevelPlan, blocks, run_block, who: str, streams: bool, result_cls):
    """Run every block, bring its outputs to the host, join the blocks along the spectral axis and order the levels as the caller
    gave them.  run_block(sl) -> ({level: outputs (S, nStokes, nVZA) / (P, S, nStokes, nVZA)}, {m: {level: level vectors (S, N) /
    (P, S, N)}} or None, Fourier weights) of the block's own points, as many per level as result_cls.FIELDS.  Returns one list
    per output ([nVZA, nStokes, nSpec(, P)] per entry of plan.levels), or, with `streams`, a result_cls."""
    parts = []
    weights = None
    for sl in blocks:
        out, full, weights = run_block(sl)
        synchronize_if_gpu()
        _lib.check_device_status(who)
        res = {l: [to_host(t).transpose().copy() for t in out[l]] for l in plan.distinct}
        vec = None
        if streams:
            vec = {m: {l: [to_host(v).transpose()[:, None].copy() for v in vs] for l, vs in fv.items()} for m, fv in full.items()}
        parts.append((res, vec))
        del out, full
        if len(blocks) > 1:
            torch.cuda.empty_cache()
    cat = (lambda xs: xs[0]) if len(parts) == 1 else (lambda xs: np.concatenate(xs, axis=2))
    nf = len(result_cls.FIELDS)
    res = {l: [cat([p[0][l][i] for p in parts]) for i in range(nf)] for l in plan.distinct}
    outs = tuple([res[l][i].copy() for l in plan.levels] for i in range(nf))
    if not streams:
        return outs
    ms = sorted(parts[0][1])
    st = [[[cat([p[1][m][l][i] for p in parts]) for m in ms] for l in plan.levels] for i in range(nf)]
    qp = model.quad_points
    return result_cls(levels=plan.levels, weight=weights, qp_mu=np.asarray(qp.qp_mu, dtype=model.float_type).copy(),
                      i_mu0=int(qp.imu0) + 1, mu0=float(qp.mu0), pol_n=model.polarization_type.n,
                      **dict(zip(result_cls.FIELDS, outs)), **{f + "_streams": x for f, x in zip(result_cls.FIELDS, st)})


def _run_segment(scene: CR.Scene, mom, seg: CR.CompositeLayer, first: int, end: int):
    """Layers first+1 .. end (1-based) as a composite of their own, full mode: the first is a TOA copy (iz = 1), every layer keeps
    its absolute tau_sum.  rt_kernel_ takes the native drop-in path where the shape allows."""
    model = scene.model
    for iz in range(first, end):
        ly = mom["layers"][iz]
        CR.rt_kernel_(scene.pol, scene.added, seg, ly["props"], ly["iface"], ly["tau_sum"], mom["m"], scene.dq, scene.arch,
                      iz - first + 1, scene.F0, scene.FT, model.numerics, dtau=ly["dtau"], ndoubl=ly["nd"], work=scene.work)


class LevelSink:
    """What a run other than the multi-sensor one does at each level of the walk of _run, in place of its level calls
    (core_rt_flux.py: the fluxes).  With a sink no VZA output is allocated, no level call and no post-processing is issued here and
    no level vector is collected; the walk itself -- tops, segments, bottoms -- is the same, and level 0 is walked only if the
    plan asks for it.  The lists carry one vector per source: the solar one, then the thermal slot's where it runs (m = 0)."""

    def level(self, mom, l, A, tops_J0_p, bot_R_mp, bots_J0_m):
        """Level l > 0: A = R+- of the composite above it and its J0+ per source, R-+ of the one below and its J0- per source."""
        raise NotImplementedError

    def level0(self, mom, J0_m_list):
        """Level 0, the TOA: J0- of the whole column with the surface, per source, after the surface interactions."""
        raise NotImplementedError


def _run(scene: CR.Scene, plan: LevelPlan, streams: bool, sink: Optional[LevelSink] = None):
    """The elastic walk on one Scene, every moment of it.  Returns ({level: (uw, dw)} of (S, nStokes, nVZA) device tensors, {m:
    {level: (uw, dw) (S, N)}} or None, the Fourier weights); with a sink (see LevelSink) the first holds level 0 alone, untouched,
    and streams is not taken."""
    model, pol, FT = scene.model, scene.pol, scene.FT
    Nz, N, S = scene.Nz, scene.N, scene.S
    tops_at = plan.tops_at
    dev, dt = scene.dev, scene.dt
    nV = len(model.vza)
    out = {0: (scene.R_SFI, scene.T_SFI)}
    full = {} if streams and sink is None else None
    if sink is None:
        refuse_non_scattering(scene.moments[0]["layers"], FT, "rt_run_multisensor",
                              ".  rt_run keeps the reference's stale-j0+ quirk there (DESIGN.md §6) while the prototype hard-codes "
                              "scatter = true (rt_kernel_multisensor.jl:29), so the two reference drivers disagree on such columns; "
                              "columns with a non-scattering layer are not supported")
        for l in plan.distinct:
            if l != 0:
                out[l] = (torch.zeros((S, pol.n, nV), dtype=dt, device=dev), torch.zeros((S, pol.n, nV), dtype=dt, device=dev))
        scene.R_SFI.zero_()
        scene.T_SFI.zero_()
    weights = []
    if S == 0:
        return out, full, [float(fourier_weight(FT, m)) for m in range(model.m_max + 1)]
    scene.added.j0_p.zero_()
    # the moment groups of Scene.run (level 0 is then rt_run's result bit for bit), fewer where the tops would not fit the device
    nb = scene._group_size(not CR.MOMENT_BATCHING or CR.REFERENCE_ORDER)
    thermal = scene.thermal_B is not None
    if nb > 1 and tops_at and dev.type == "cuda":
        elt = torch.finfo(dt).bits // 8
        per_moment = len(tops_at) * (N * N + N) * S * elt + (4 * N * N + 2 * N) * S * elt
        if thermal:   # the thermal tops (J0+ alone), counted for every moment of a group although only m = 0 keeps them
            per_moment += len(tops_at) * N * S * elt
        free = torch.cuda.mem_get_info(dev)[0]
        nb = max(1, min(nb, int(0.5 * free // per_moment)))
    # the two alternating segment composites, each with its thermal twin (m = 0 only; never in native layout: the slot's calls
    # take the reference's arrays) or None
    new_comp = lambda: CR.make_composite_layer(FT, scene.arch, (N, N), S)
    segs = [(new_comp(), new_comp() if thermal else None) for _ in range(2 if plan.interior else 0)]
    native = scene._native_moments() if not CR.REFERENCE_ORDER else set()
    with contextlib.ExitStack() as stack:
        stack.callback(lambda: [seg[0].drop_native() for seg in segs])
        stack.enter_context(scene._walk_composites(nb, CR.REFERENCE_ORDER, None))
        for g0 in range(0, len(scene.moments), nb):
            group = scene.moments[g0:g0 + nb]
            comps = scene._composites[:len(group)]
            tops = [dict() for _ in group]
            # 1. the top pass: Scene.run's walk, the tops kept on the way
            scene._walk_layers(group, comps, [k for k in range(len(group)) if (g0 + k) in native], sources_only=True, view_rows=None,
                               tops_at=tops_at, keep_top=lambda k, l, top, tops=tops: tops[k].__setitem__(l, top))
            for k, (mom, comp) in enumerate(zip(group, comps)):
                m = mom["m"]
                weight = fourier_weight(FT, m)
                weights.append(float(weight))
                fv = {}
                asurf = scene.added_surface
                CR.create_surface_layer_(model.surface, asurf, m, scene.dq, mom["tau_sum_surface"], rho=mom["rho"])
                # SurfaceSIF (m = 0, Lambertian surfaces): the bottoms are built upward from this layer, so every level sees it
                CR.surface_source_contribute_(scene, model.surface, asurf, m)
                # the thermal slot (m = 0): its top pass on the slot's own composite, J0+ kept after each level of tops_at
                th = thermal and m == 0
                th_tops, th_surf = {}, None
                if th:
                    slot = scene.thermal_slot()
                    slot.begin(mom)
                    slot.walk(mom, slot.comp, 0, Nz, scene.thermal_B,
                              after={l: (lambda c, l=l: th_tops.__setitem__(l, c.J0_p.clone())) for l in tops_at})
                    th_surf = slot.surface(mom)

                def level(l, seg):
                    A, a = tops[k].pop(l)
                    bot_R_mp, bot_J0_m = (asurf.r_mp, asurf.j0_m) if seg is None else (seg[0].R_mp, seg[0].J0_m)
                    aa, cc = [a], [bot_J0_m]
                    if th:   # the solar and the thermal right-hand side on ONE system (A, B of the solar pass)
                        aa.append(th_tops.pop(l))
                        cc.append(th_surf.j0_m if seg is None else seg[1].J0_m)
                    if sink is not None:
                        sink.level(mom, l, A, aa, bot_R_mp, cc)
                        return
                    dwf = torch.empty((S, N), dtype=dt, device=dev) if streams else None
                    uwf = torch.empty((S, N), dtype=dt, device=dev) if streams else None
                    if th:
                        level_radiance_src_(pol, scene.qp, model.vza, model.vaz, m, float(weight), A, aa, bot_R_mp, cc, out[l][0],
                                            out[l][1], dwf, uwf)
                    else:
                        level_radiance_(pol, scene.qp, model.vza, model.vaz, m, float(weight), A, a, bot_R_mp, bot_J0_m, out[l][0],
                                        out[l][1], dwf, uwf)
                    if streams:
                        fv[l] = (uwf, dwf)

                def run_segment(seg, first, end):
                    _run_segment(scene, mom, seg[0], first, end)
                    if th:
                        slot.walk(mom, seg[1], first, end, scene.thermal_B)

                def join_surface(seg):
                    CR.interaction_(mom["iface_surface"], seg[0], asurf, work=scene.work)
                    if th:
                        CR.interaction_(mom["iface_surface"], seg[1], th_surf, oplevel=True, work=scene.work)

                def join_bottom(seg, bot, first, end):
                    CR.interaction_("11", seg[0], _CompositeAsAdded(bot[0]), work=scene.work)
                    if th:
                        CR.interaction_("11", seg[1], _CompositeAsAdded(bot[1]), oplevel=True, work=scene.work)
                # 2.-4. the levels below the top pass
                walk_levels(plan, segs, run_segment, join_surface, join_bottom, level)
                tops[k].clear()
                if sink is not None:
                    # level 0, the TOA itself: J0- of the whole column with the surface, and the thermal slot's (ThermalSlot.finish
                    # without its post-processing)
                    if 0 in plan.distinct:
                        CR.interaction_(mom["iface_surface"], comp, asurf, work=scene.work)
                        J0_m = [comp.J0_m]
                        if th:
                            CR.interaction_(mom["iface_surface"], slot.comp, th_surf, oplevel=True, work=scene.work)
                            J0_m.append(slot.comp.J0_m)
                        sink.level0(mom, J0_m)
                    continue
                # level 0: rt_run's surface interaction and post-processing (no Cox-Munk single-scattering correction), then the
                # thermal slot's, in rt_run's order of accumulation into R_SFI / T_SFI
                CR.interaction_(mom["iface_surface"], comp, asurf, work=scene.work)
                CR.postprocessing_vza_(pol, comp, model.vza, model.vaz, scene.qp, m, float(weight), scene.R_SFI, scene.T_SFI)
                if th:
                    slot.finish(mom, float(weight), scene.R_SFI, scene.T_SFI)
                if streams:
                    fv[0] = (comp.J0_m.clone(), comp.J0_p.clone())
                    if th:     # per-source slots added, as Scene.run(streams=...) sums J0
                        fv[0][0].add_(slot.comp.J0_m)
                        fv[0][1].add_(slot.comp.J0_p)
                    full[m] = fv
    return out, full, weights


def rt_run_multisensor(model: H.RTModel, sensor_levels, streams: bool = False, thermal: bool = False):
    """rt_run_test_ms(::noRS, sensor_levels, model, iBand) (rt_run_multisensor.jl): its first two return values (uwJ, dwJ), lists
    with one [nVZA, nStokes, nSpec] host array per entry of `sensor_levels`, in the caller's order (the inelastic uwieJ / dwieJ are
    zero for noRS and not returned).

    sensor_levels: layer boundaries counted from the TOA: 0 = TOA, l = below layer l, Nz = just above the surface; duplicates and
    any order allowed (each distinct level is computed once).  Level 0 is the whole column with the surface: uw = rt_run's R_SFI,
    dw = rt_run's T_SFI (postprocessing_vza_ms.jl:33-35), bit for bit, without the Cox-Munk single-scattering correction
    (rt_run.jl:520-524), which the prototype never applies.  Levels 1..Nz-1: the level equation of interlayer_flux_helper! between
    layers 1..l above and layers l+1..Nz with the surface below.  Level Nz takes the surface layer alone as the bottom (the
    prototype leaves that composite uninitialised).  VZA rows and azimuth weights as in postprocessing_vza!, the
    same rows for uw and dw.

    streams=True: a MultiSensorResult, which also carries the level vectors at all quadrature streams per moment.
    SolarBeam sources only; columns with a non-scattering layer raise NotImplementedError.

    thermal=True: model.sources may hold SolarBeam and / or ThermalEmission (Scene.__init__'s rule: without a SolarBeam F0 = 0;
    the surface layer is built as rt_run builds it, with the Lambertian beam term of DESIGN.md §6); any other source raises.  uw /
    dw per level are the sum of the solar and the thermal slot, as rt_run's R_SFI / T_SFI are, level 0 again rt_run's result bit
    for bit; with streams=True the level vectors of m = 0 are the sum as well.  Columns with a non-scattering layer are refused
    as before, so the slot-state behaviour of such layers never arises here and
    ThermalEmission.reset_slot_in_nonscattering_layers has no effect.  SurfaceEmission (thermal=True only; VSMError without it)
    is the emission of the slot's lower boundary: every bottom of the slot is built upward from the emitting surface layer, so every
    level carries it, level Nz included (there the bottom is the surface layer alone and c is its j0-); DESIGN.md §4.18.

    SurfaceSIF (with or without thermal=True): injected into the solar slot's surface layer at m = 0 as rt_run injects it
    (rt_run_multisensor.jl:140); every bottom composite is built upward from that layer, so every level carries the emission,
    and level 0 stays rt_run's result bit for bit."""
    plan = _validate(model, sensor_levels, thermal=bool(thermal), sif=True)

    def run_block(_sl):
        scene = CR.prepare_scene(model)
        scene.compute_hdrf = False
        return _run(scene, plan, bool(streams))
    return gather_blocks(model, plan, [None], run_block, "rt_run_multisensor", bool(streams), MultiSensorResult)
