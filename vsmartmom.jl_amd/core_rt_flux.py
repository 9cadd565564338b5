"""Hemispheric fluxes at the layer boundaries of the column: rt_run_fluxes.

The level vectors of the multi-sensor run (core_rt_ms.py) at m = 0, the one Fourier moment that survives the azimuth integral,
reduced on the device to their hemispheric quadratures: per level ONE call of vsm_level_flux_* (csrc/vsm_level.hip), which solves
the level equation for every source on one elimination and leaves 3 nW scalars per spectral point -- no [S, N] level vector is
allocated, none is brought to the host.  There is no walk here: the run hands core_rt_ms._run, the one elastic walk, a scene of
that one moment and a sink (_FluxSink) that takes the place of its level calls.

Convention (the reference's hem_R / hem_T, rt_run.jl:745): with uw / dw the m = 0 level vectors (rows of Stokes I), mu, w the
quadrature nodes and weights, F = sum_i mu_i w_i v_i and the actinic flux sum_i w_i v_i; the Fourier weight 0.5 / pi and the 2 pi
of the azimuth integral cancel.  The direct beam, which the diffuse vectors do not contain, is mu0 F0 exp(-tau_sum / mu0)
(actinic: without the mu0), tau_sum the run's own (delta-M scaled) optical depth above the level.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from . import core_rt_ms as MS
from . import host_model as H
from .architectures import synchronize_if_gpu, to_host

WHO = "rt_run_fluxes"
FLUX_MAX_W = 4             # weight rows of one vsm_level_flux_* call


def level_flux_(pol, top_R_pm, tops_J0_p, bot_R_mp, bots_J0_m, q, dir_h, mu0: float, tau_sum, F0_I, out, oplevel: bool = False):
    """The hemispheric quadratures of the level vectors at one boundary (vsm_level_flux_*): with A = top_R_pm (S, N, N), a_k =
    tops_J0_p[k], B = bot_R_mp ((S | 1, N, N): one block shared by every point is bot_stride 0), c_k = bots_J0_m[k] (lists of
    (S, N) vectors, one pair per source) and the weight rows q (nW, N / n) on the device,
        dw_k = (I - A B)^-1 (a_k + A c_k),   uw_k = c_k + B dw_k,
        out[0][r] = sum_i q[r][i] sum_k uw_k[:, i n],   out[1][r] likewise of dw,   out[2][r] = dir_h[r] F0_I exp(-tau_sum / mu0)
    (tau_sum, F0_I: (S,) tensors, both or neither; neither: out[2] = 0).  out (3, nW, S) is written, not accumulated.
    top_R_pm None: no layer above the boundary (the TOA): dw = 0, uw = sum_k c_k, tops_J0_p and bot_R_mp are not read.
    N <= 128: ONE call.  N > 128 or operator level: one vsm_level_radiance_oplevel_* call per source with full vectors, the
    vectors summed, a batched product with q, the direct term in torch."""
    n_src, nW = len(bots_J0_m), int(q.shape[0])
    if n_src == 0 or (top_R_pm is not None and n_src != len(tops_J0_p)):
        raise _lib.VSMError("level_flux_: %d top and %d bottom source vectors" % (len(tops_J0_p or ()), n_src))
    S, N = int(bots_J0_m[0].shape[0]), int(bots_J0_m[0].shape[1])
    dt = bots_J0_m[0].dtype
    if (tau_sum is None) != (F0_I is None):
        raise _lib.VSMError("level_flux_: tau_sum and F0_I are given together or not at all")
    bot_stride = N * N if bot_R_mp is None else MS.bot_stride_of(bot_R_mp, S, N)
    P = CR._ptr
    ctype = C.c_double if dt == torch.float64 else C.c_float
    if not (oplevel or MS.LEVEL_OPLEVEL or N > MS.LEVEL_FUSED_MAX_N):
        pc = (C.c_void_p * n_src)(*[P(t) for t in bots_J0_m])
        pa = None if top_R_pm is None else (C.c_void_p * n_src)(*[P(t) for t in tops_J0_p])
        dh = (ctype * max(nW, 1))(*[float(x) for x in dir_h])
        _lib.call("vsm_level_flux", dt, N, pol.n, S, P(top_R_pm), n_src, pa, None if top_R_pm is None else P(bot_R_mp), bot_stride,
                  pc, nW, P(q), dh, ctype(float(mu0)), P(tau_sum), P(F0_I), P(out), CR._stream_ptr())
        return
    if not 1 <= n_src <= MS.LEVEL_MAX_SRC or not 1 <= nW <= FLUX_MAX_W:
        raise _lib.VSMError("level_flux_: n_src = %d (1..%d), nW = %d (1..%d)" % (n_src, MS.LEVEL_MAX_SRC, nW, FLUX_MAX_W))
    if S == 0:
        return
    if top_R_pm is None:
        uw, dw = torch.zeros_like(bots_J0_m[0]), torch.zeros_like(bots_J0_m[0])
        for c in bots_J0_m:
            uw += c
    else:
        uw = dw = None
        for a, c in zip(tops_J0_p, bots_J0_m):
            dwk, uwk = torch.empty_like(c), torch.empty_like(c)
            MS.level_radiance_(pol, None, [], [], 0, 1.0, top_R_pm, a, bot_R_mp, c, None, None, dwk, uwk, oplevel=True)
            uw, dw = (uwk, dwk) if uw is None else (uw + uwk, dw + dwk)
    qT = q.t().contiguous()                                      # (N / n, nW)
    out[0].copy_((uw[:, ::pol.n] @ qT).t())
    out[1].copy_((dw[:, ::pol.n] @ qT).t())
    if tau_sum is None:
        out[2].zero_()
    else:
        beam = F0_I * torch.exp(-tau_sum / mu0)
        out[2].copy_(torch.as_tensor([float(x) for x in dir_h], dtype=dt, device=out.device)[:, None] * beam[None, :])


@dataclass
class FluxResult:
    """rt_run_fluxes: host arrays in the model's float type; the rows follow `levels`, the caller's order."""
    levels: List[int]
    up: np.ndarray                       # [nLevels, nSpec]  sum_i mu_i w_i uw_I[i]
    down_diffuse: np.ndarray             # sum_i mu_i w_i dw_I[i]; exactly 0 at level 0
    down_direct: np.ndarray              # mu0 F0[0] exp(-tau_sum(level) / mu0)
    actinic_up: np.ndarray               # sum_i w_i uw_I[i]
    actinic_down_diffuse: np.ndarray     # sum_i w_i dw_I[i]
    actinic_direct: np.ndarray           # F0[0] exp(-tau_sum(level) / mu0)
    net_down: np.ndarray                 # down_direct + down_diffuse - up
    absorbed: Optional[np.ndarray]       # [Nz, nSpec] net_down[l - 1] - net_down[l] of layer l; None unless every level was computed
    surface_absorbed: Optional[np.ndarray]   # [nSpec] net_down[Nz]; same rule


def bytes_per_point(N: int, Nz: int, n_tops: int, segments: bool, thermal: bool, itemsize: int) -> int:
    """Device bytes per spectral point of a flux run (an estimate on the safe side): the kept tops (R+- and J0+ of every level
    but the TOA: what dominates a run over all levels -- N = 60, 40 levels, FP64: 1.17 MB per point), the thermal tops (J0+), the
    two segment composites, the scene's composite, added and surface layer (the surface counted as a full per-point layer), as
    much again for the layer kernels' workspace, the per-layer optics and the outputs; with the thermal slot its three layers and
    the twins of the segment composites."""
    layer = 4 * N * N + 2 * N
    elems = n_tops * (N * N + N) + (2 * layer if segments else 0) + 5 * layer + 8 * Nz + 3 * FLUX_MAX_W * (Nz + 1)
    if thermal:
        elems += n_tops * N + 3 * layer + (2 * layer if segments else 0)
    return elems * itemsize


class _FluxSink(MS.LevelSink):
    """The flux run's place in the walk of core_rt_ms._run: one level_flux_ call per level into its row of ONE (len(plan.distinct),
    3, 2, S) device tensor -- per level [up, down, direct] x [flux, actinic] --, so that ONE copy brings a block home."""

    def __init__(self, scene: CR.Scene, plan: MS.LevelPlan):
        MS.refuse_non_scattering(scene.moments[0]["layers"], scene.FT, WHO,
                                 ".  rt_run keeps the reference's stale-j0+ quirk there (DESIGN.md §6), which the level equation "
                                 "does not carry; columns with a non-scattering layer are not supported (as for rt_run_multisensor)")
        self.pol, self.Nz = scene.pol, scene.Nz
        self.buf = torch.empty((len(plan.distinct), 3, 2, scene.S), dtype=scene.dt, device=scene.dev)
        self.out = {l: self.buf[i] for i, l in enumerate(plan.distinct)}
        qp = scene.qp
        mu, wt = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
        # the flux row and the actinic row, uploaded once
        self.q = torch.as_tensor(np.stack([mu * wt, wt]).astype(scene.FT), device=scene.dev)
        self.mu0 = float(qp.mu0)
        self.dir_h = (self.mu0, 1.0)
        self.F0_I = scene.F0[:, 0].contiguous()

    def _flux(self, mom, l, A, aa, bot_R_mp, cc):
        tau_sum = mom["tau_sum_surface"] if l == self.Nz else mom["layers"][l]["tau_sum"]
        level_flux_(self.pol, A, aa, bot_R_mp, cc, self.q, self.dir_h, self.mu0, tau_sum, self.F0_I, self.out[l])

    def level(self, mom, l, A, tops_J0_p, bot_R_mp, bots_J0_m):
        self._flux(mom, l, A, tops_J0_p, bot_R_mp, bots_J0_m)

    def level0(self, mom, J0_m_list):      # nothing diffuse goes down at the TOA
        self._flux(mom, 0, None, None, None, J0_m_list)


def rt_run_fluxes(model: H.RTModel, levels=None, thermal: bool = False, max_points: Optional[int] = None) -> FluxResult:
    """Up-, downwelling and actinic fluxes at layer boundaries of the column, as a FluxResult of [nLevels, nSpec] host arrays.

    levels: layer boundaries counted from the TOA, as in rt_run_multisensor: 0 = TOA, l = below layer l, Nz = just above the
    surface; None = all of 0..Nz; duplicates and any order allowed (each distinct level is computed once, the rows follow the
    caller's order).  With uw / dw the m = 0 level vectors of rt_run_multisensor (rows of Stokes I), mu, w = quad_points.qp_mu /
    wt_mu (the zero-weight SZA / VZA nodes drop out by themselves) and mu0 the SZA node:
        up = sum_i mu_i w_i uw_i            down_diffuse = sum_i mu_i w_i dw_i         down_direct = mu0 F0[0] exp(-tau_sum / mu0)
        actinic_up = sum_i w_i uw_i         actinic_down_diffuse = sum_i w_i dw_i      actinic_direct = F0[0] exp(-tau_sum / mu0)
        net_down = down_direct + down_diffuse - up
    tau_sum: the run's own optical depth above the level (delta-M scaled, as the layer kernels see it).  No further factor: the
    Fourier weight 0.5 / pi and the 2 pi of the azimuth integral cancel (the reference's hem_R / hem_T, rt_run.jl:745), so the
    flux entering the TOA is mu0 F0, a Lambertian surface returns albedo (diffuse + direct), an opaque isothermal layer gives pi B.
    Level 0 is the TOA itself: `up` is J0- of the whole column with the surface, and nothing diffuse enters, so the diffuse down
    terms are exactly 0 there -- NOT rt_run_multisensor's level-0 dw, which is rt_run's T, the field at the bottom of the column
    (that is down_diffuse at level Nz).  With every level computed, absorbed [Nz, nSpec] = net_down[l - 1] - net_down[l] is the flux
    convergence of layer l and surface_absorbed [nSpec] = net_down[Nz]; otherwise both are None.

    Only m = 0 is walked, whatever model.m_max is.  Only the I row is reported: no Q / U / V fluxes; no Cox-Munk single-scattering
    correction, as the multi-sensor run has none.  Jacobians of every field: CoreRTLin.rt_run_fluxes (core_rt_flux_lin.py).

    Sources as the elastic rt_run_multisensor takes them: SolarBeam and SurfaceSIF always, ThermalEmission and SurfaceEmission
    under thermal=True (VSMError without it; the emitting boundary enters through the slot's surface layer), any other source VSMError; every result is the sum over the sources.  Without a SolarBeam F0 = 0 and
    both direct terms are 0.  Columns with a non-scattering layer raise NotImplementedError.

    max_points: run the spectral axis in blocks of that many points (ndoubl and the interface tags stay batch-global); None = as
    many as fit the device (bytes_per_point: a run over all levels keeps a top per level)."""
    Nz = int(np.asarray(model.tau_rayl).shape[1])
    plan = MS._validate(model, range(Nz + 1) if levels is None else levels, thermal=bool(thermal), sif=True, who=WHO)
    model0 = dataclasses.replace(model, m_max=0)
    qp, pol = model.quad_points, model.polarization_type
    N = qp.Nquad * pol.n
    S_full = int(np.asarray(model.tau_rayl).shape[0])
    has_th = any(isinstance(s_, (H.ThermalEmission, H.SurfaceEmission)) for s_ in (model.sources or ()))
    if max_points is None and S_full > 0:
        per = bytes_per_point(N, Nz, plan.n_tops, bool(plan.interior), has_th, np.dtype(model.float_type).itemsize)
        free, _total = torch.cuda.mem_get_info()
        fit = int(0.5 * free // per)
        if fit < S_full:
            if fit < 1:
                raise _lib.VSMError("%s: not even one spectral point fits the device (%d bytes per point)" % (WHO, per))
            max_points = fit
    parts = []
    blocks = MS.spectral_blocks(S_full, max_points)
    for sl in blocks:
        scene = CR.prepare_scene(model0, sl)          # (m = 0 alone)
        sink = _FluxSink(scene, plan)
        MS._run(scene, plan, False, sink)
        out = sink.buf
        del scene, sink
        synchronize_if_gpu()
        _lib.check_device_status(WHO)
        parts.append(to_host(out))
        del out
        if len(blocks) > 1:
            torch.cuda.empty_cache()
    host = np.concatenate(parts, axis=3)
    res = {l: host[i] for i, l in enumerate(plan.distinct)}                                  # (3, 2, nSpec)
    pick = lambda d, r: np.stack([res[l][d, r] for l in plan.levels]).astype(model.float_type, copy=False)
    up, dn, direct = pick(0, 0), pick(1, 0), pick(2, 0)
    net = direct + dn - up
    absorbed = surface_absorbed = None
    if plan.distinct == list(range(Nz + 1)):
        net_l = np.stack([res[l][2, 0] + res[l][1, 0] - res[l][0, 0] for l in range(Nz + 1)]).astype(model.float_type, copy=False)
        absorbed, surface_absorbed = net_l[:-1] - net_l[1:], net_l[-1].copy()
    return FluxResult(levels=list(plan.levels), up=up, down_diffuse=dn, down_direct=direct, actinic_up=pick(0, 1),
                      actinic_down_diffuse=pick(1, 1), actinic_direct=pick(2, 1), net_down=net, absorbed=absorbed,
                      surface_absorbed=surface_absorbed)
