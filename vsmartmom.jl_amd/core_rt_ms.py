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


def level_radiance_(pol, qp, vza, vaz, m: int, weight: float, top_R_pm, top_J0_p, bot_R_mp, bot_J0_m, uw, dw,
                    dw_full=None, uw_full=None, oplevel: bool = False):
    """The level equation at one boundary (interlayer_flux_helper!, interlayer_flux.jl:1-19, + the VZA rows of
    postprocessing_vza_ms!): uw / dw (S, n, nV) layout tensors += weight * rows of
        dw = (I - A B)^-1 (a + A c),   uw = (I - B A)^-1 (c + B a)  [= c + B dw]
    with A = top_R_pm, a = top_J0_p (S, N[, N]), B = bot_R_mp ((S | 1, N, N): one block shared by every point is bot_stride 0),
    c = bot_J0_m.  dw_full / uw_full: (S, N) tensors that receive the level vectors at all streams."""
    S, N = int(top_J0_p.shape[0]), int(top_J0_p.shape[1])
    if S == 0:
        return
    dt = top_J0_p.dtype
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, m, weight, dt)
    bot_stride = 0 if int(bot_R_mp.shape[0]) == 1 and S > 1 else N * N
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


@dataclass
class MultiSensorResult:
    """rt_run_multisensor(..., streams=True): per entry of sensor_levels the VZA outputs and, per Fourier moment, the level vectors
    at ALL quadrature streams (the arrays postprocessing_vza_ms! reads its rows from: tuwJ / tdwJ [N, 1, nSpec])."""
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


def _validate(model: H.RTModel, sensor_levels):
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
    other = [s for s in srcs if not isinstance(s, H.SolarBeam)]
    if other or not srcs:
        raise _lib.VSMError("rt_run_multisensor: SolarBeam is the only source of a multi-sensor run (the prototype passes F0 alone, "
                            "rt_kernel_multisensor.jl:21); got %r" % (other[0] if other else None,))
    return levels, Nz


def _snapshot(comp: CR.CompositeLayer):
    """(R+-, J0+) of a composite in the middle of its walk, without disturbing the walk: a composite that rt_kernel_ keeps in
    native layout is exported (vsm_run_export leaves the run as it is) instead of materialised (which would end the run)."""
    slot = comp._native
    if slot is not None:
        cc = (_lib.vsm_composite * 1)(comp._cstruct_raw())
        _lib.call("vsm_run_export", comp.dtype, slot.run, cc, CR._stream_ptr())
        a = comp._arr
    else:
        a = comp.materialize()._arr
    return a["R_pm"].clone(), a["J0_p"].clone()


def _run_segment(scene: CR.Scene, mom, seg: CR.CompositeLayer, first: int, end: int):
    """Layers first+1 .. end (1-based) as a composite of their own, full mode: the first is a TOA copy (iz = 1), every layer keeps
    its absolute tau_sum.  rt_kernel_ takes the native drop-in path where the shape allows."""
    model = scene.model
    for iz in range(first, end):
        ly = mom["layers"][iz]
        CR.rt_kernel_(scene.pol, scene.added, seg, ly["props"], ly["iface"], ly["tau_sum"], mom["m"], scene.dq, scene.arch,
                      iz - first + 1, scene.F0, scene.FT, model.numerics, dtau=ly["dtau"], ndoubl=ly["nd"], work=scene.work)


def _run(scene: CR.Scene, levels: List[int], streams: bool):
    model, pol, FT = scene.model, scene.pol, scene.FT
    Nz, N, S = scene.Nz, scene.N, scene.S
    eps2 = 2 * np.finfo(FT).eps
    noscat = [iz + 1 for iz, ly in enumerate(scene.moments[0]["layers"]) if ly["props"].max_tau_varpi <= eps2]
    if noscat:
        raise NotImplementedError(
            "rt_run_multisensor: layer %d does not scatter (tau * varpi <= 2 eps).  rt_run keeps the reference's stale-j0+ "
            "quirk there (DESIGN.md §6) while the prototype hard-codes scatter = true (rt_kernel_multisensor.jl:29), so the two "
            "reference drivers disagree on such columns; columns with a non-scattering layer are not supported" % noscat[0])
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    tops_at = interior + ([Nz] if Nz in distinct else [])
    dev, dt = scene.dev, scene.dt
    nV = len(model.vza)
    out = {l: (torch.zeros((S, pol.n, nV), dtype=dt, device=dev), torch.zeros((S, pol.n, nV), dtype=dt, device=dev))
           for l in distinct if l != 0}
    out[0] = (scene.R_SFI, scene.T_SFI)
    full = {} if streams else None
    scene.R_SFI.zero_()
    scene.T_SFI.zero_()
    weights = []
    if S == 0:
        return out, full, [float(FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)) for m in range(model.m_max + 1)]
    scene.added.j0_p.zero_()
    # the moment groups of Scene.run (level 0 is then rt_run's result bit for bit), fewer where the tops would not fit the device
    sequential = not CR.MOMENT_BATCHING or CR.REFERENCE_ORDER
    want = max(CR.MOMENT_BATCH, min(CR.MOMENT_BATCH_MAX, 4096 // max(S, 1)))
    nb = 1 if sequential else min(want, len(scene.moments))
    if tops_at and dev.type == "cuda":
        elt = torch.finfo(dt).bits // 8
        per_moment = len(tops_at) * (N * N + N) * S * elt + (4 * N * N + 2 * N) * S * elt
        free = torch.cuda.mem_get_info(dev)[0]
        nb = max(1, min(nb, int(0.5 * free // per_moment)))
    while len(scene._composites) < nb:
        scene._composites.append(CR.make_composite_layer(FT, scene.arch, (N, N), S))
    segs = [CR.make_composite_layer(FT, scene.arch, (N, N), S) for _ in range(2 if interior else 0)]
    native = scene._native_moments() if not CR.REFERENCE_ORDER else set()
    for c in scene._composites:
        c._sources_only = CR.REFERENCE_ORDER
    try:
        for g0 in range(0, len(scene.moments), nb):
            group = scene.moments[g0:g0 + nb]
            comps = scene._composites[:len(group)]
            tops = [dict() for _ in group]
            nat = [k for k in range(len(group)) if (g0 + k) in native]
            # 1. the top pass
            if nat:
                def keep(l):
                    def cb(cs):
                        for k, c in zip(nat, cs):
                            tops[k][l] = (c._arr["R_pm"].clone(), c._arr["J0_p"].clone())
                    return cb
                scene._run_layers_native([group[k] for k in nat], [comps[k] for k in nat], sources_only=True,
                                         export_at={l: keep(l) for l in tops_at})
            rest = [k for k in range(len(group)) if (g0 + k) not in native]
            group_l, comps_l = [group[k] for k in rest], [comps[k] for k in rest]
            for iz in range(Nz if rest else 0):
                ly0 = group_l[0]["layers"][iz]
                if len(group_l) > 1 and (iz == 0 or ly0["iface"] == "11"):
                    CR.layer_forward_multi_(ly0["tau_sum"], ly0["dtau"], scene.F0, [mom["layers"][iz]["props"] for mom in group_l],
                                            [mom["m"] for mom in group_l], ly0["nd"], scene.dq, iz == 0, comps_l, scene.added)
                else:
                    for mom, comp in zip(group_l, comps_l):
                        ly = mom["layers"][iz]
                        CR.rt_kernel_(pol, scene.added, comp, ly["props"], ly["iface"], ly["tau_sum"], mom["m"], scene.dq,
                                      scene.arch, iz + 1, scene.F0, FT, model.numerics, dtau=ly["dtau"], ndoubl=ly["nd"],
                                      work=scene.work)
                if iz + 1 in tops_at:
                    for k, comp in zip(rest, comps_l):
                        tops[k][iz + 1] = _snapshot(comp)
            for k, (mom, comp) in enumerate(zip(group, comps)):
                m = mom["m"]
                weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
                weights.append(float(weight))
                fv = {}
                asurf = scene.added_surface
                CR.create_surface_layer_(model.surface, asurf, m, scene.dq, mom["tau_sum_surface"], rho=mom["rho"])

                def level(l, bot_R_mp, bot_J0_m):
                    A, a = tops[k][l]
                    dwf = torch.empty((S, N), dtype=dt, device=dev) if streams else None
                    uwf = torch.empty((S, N), dtype=dt, device=dev) if streams else None
                    level_radiance_(pol, scene.qp, model.vza, model.vaz, m, float(weight), A, a, bot_R_mp, bot_J0_m, out[l][0],
                                    out[l][1], dwf, uwf)
                    if streams:
                        fv[l] = (uwf, dwf)
                # 4. level Nz: the surface layer alone below it
                if Nz in distinct:
                    level(Nz, asurf.r_mp, asurf.j0_m)
                # 2.-4. segments and bottoms from the surface up, one level call per interior level
                bot = None
                ends = interior[1:] + [Nz]
                for i, (l, end) in enumerate(reversed(list(zip(interior, ends)))):
                    seg = segs[i % 2]
                    _run_segment(scene, mom, seg, l, end)
                    if bot is None:
                        CR.interaction_(mom["iface_surface"], seg, asurf, work=scene.work)
                    else:
                        CR.interaction_("11", seg, _CompositeAsAdded(bot), work=scene.work)
                    level(l, seg.R_mp, seg.J0_m)
                    bot = seg
                    del tops[k][l]
                # level 0: rt_run's surface interaction and post-processing (no Cox-Munk single-scattering correction)
                CR.interaction_(mom["iface_surface"], comp, asurf, work=scene.work)
                CR.postprocessing_vza_(pol, comp, model.vza, model.vaz, scene.qp, m, float(weight), scene.R_SFI, scene.T_SFI)
                if streams:
                    fv[0] = (comp.J0_m.clone(), comp.J0_p.clone())
                    full[m] = fv
                tops[k].clear()
    finally:
        for c in scene._composites:
            c._sources_only = False
        for c in segs:
            c.drop_native()
    return out, full, weights


def rt_run_multisensor(model: H.RTModel, sensor_levels, streams: bool = False):
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
    SolarBeam sources only; columns with a non-scattering layer raise NotImplementedError."""
    levels, Nz = _validate(model, sensor_levels)
    scene = CR.prepare_scene(model)
    scene.compute_hdrf = False
    out, full, weights = _run(scene, levels, bool(streams))
    synchronize_if_gpu()
    _lib.check_device_status("rt_run_multisensor")
    host = lambda t: to_host(t).transpose(2, 1, 0).copy()
    res = {l: (host(u), host(d)) for l, (u, d) in out.items()}
    uw = [res[l][0].copy() for l in levels]
    dw = [res[l][1].copy() for l in levels]
    if not streams:
        return uw, dw
    vec = lambda t: to_host(t).T[:, None, :].copy()
    ms = sorted(full) if full else []
    qp = model.quad_points
    return MultiSensorResult(levels, uw, dw, [[vec(full[m][l][0]) for m in ms] for l in levels],
                             [[vec(full[m][l][1]) for m in ms] for l in levels], weights,
                             np.asarray(qp.qp_mu, dtype=model.float_type).copy(), int(qp.imu0) + 1, float(qp.mu0),
                             model.polarization_type.n)
