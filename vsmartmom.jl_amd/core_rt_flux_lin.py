"""Hemispheric fluxes and their Jacobians at the layer boundaries of the column: CoreRTLin.rt_run_fluxes.

The linearized twin of core_rt_flux.py.  The walk is that of the linearized multi-sensor run (core_rt_ms_lin._run_scene /
_run_thermal) for the one Fourier moment m = 0 -- the top pass with the tops kept, the segments and bottoms from the surface up,
the thermal slot on its own operators -- with a LevelSink in place of its level calls: per level the elastic level call leaves the
level vectors at all streams, and ONE call of vsm_level_flux_lin_* (csrc/vsm_level.hip) solves the derivative of the level
equation for every slot and reduces each derivative vector on the chip to its hemispheric quadratures.  No [P, S, N] derivative
level vector is allocated; 6 (1 + P) scalars per level and spectral point come home (as many again, with the Planck slots, for
the thermal slot), in one array per block.

Conventions, row order and the level-0 rule are core_rt_flux.py's.  The direct beam mu0 F0 exp(-tau_sum / mu0) has the derivative
-direct * tau_sum_dot[p] / mu0 for the layer slots p (tau_sum_dot: the scene's table, core_rt_lin.py) and 0 for the surface and
Planck slots.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from . import core_rt_flux as FX
from . import core_rt_lin as CL
from . import core_rt_ms as MS
from . import core_rt_ms_lin as MSL
from . import host_model as H
from .architectures import synchronize_if_gpu, to_host

WHO = "rt_run_fluxes (linearized)"


def level_flux_lin_(pol, P: int, P_top: int, top_R_pm, bot_R_mp, dw_full, uw_full, top_R_pm_lin, top_J0_p_lin, bot_R_mp_lin,
                    bot_J0_m_lin, src_top_J0_p, src_bot_J0_m, q, dir_h, mu0: float, tau_sum, F0_I, tau_sum_dot, p_layer: int, out):
    """The hemispheric quadratures of the level vectors and of their derivatives at one boundary (vsm_level_flux_lin_*): the
    operands of core_rt_ms_lin.level_radiance_lin_src_ (A = top_R_pm (S, N, N), B = bot_R_mp ((S | 1, N, N)), dw_full / uw_full
    (S, N) the elastic level vectors, top_R_pm_lin / top_J0_p_lin (P_top, S, N[, N]), bot_R_mp_lin ((P, S | 1, N, N)), bot_J0_m_lin
    (P, S, N), src_top_J0_p / src_bot_J0_m (P_src, S, N) or None) and the weight rows and direct-beam operands of
    core_rt_flux.level_flux_ (q (nW, N / n) on the device, dir_h, mu0, tau_sum / F0_I (S,) or both None) with tau_sum_dot
    ((>= p_layer, S): d tau_sum / d x_p of the first p_layer slots).  out (3, nW, 1 + P + P_src, S) is written: slot 0 the
    forward quadratures of uw_full / dw_full and the direct beam, slot 1 + p those of uw'_p / dw'_p and -direct tau_sum_dot[p] /
    mu0 (p < p_layer; 0 beyond, and all of out[2] without tau_sum).  top_R_pm None: the TOA -- dw = 0, dw' = 0, uw = uw_full,
    uw'_p = bot_J0_m_lin[p] or src_bot_J0_m[k]; bot_R_mp, dw_full and the operator derivatives are not read.  N <= 128."""
    S, N = int(uw_full.shape[0]), int(uw_full.shape[1])
    dt = uw_full.dtype
    nW = int(q.shape[0])
    P_src = 0 if src_bot_J0_m is None else int(src_bot_J0_m.shape[0])
    toa = top_R_pm is None
    bot_stride = 0 if not toa and int(bot_R_mp.shape[0]) == 1 and S > 1 else N * N
    sb = 1 if toa or bot_R_mp_lin is None else int(bot_R_mp_lin.shape[1])
    bd_stride = 0 if sb == 1 and S > 1 else N * N
    ctype = C.c_double if dt == torch.float64 else C.c_float
    dh = (ctype * max(nW, 1))(*[float(x) for x in dir_h])
    Pt = CR._ptr
    top_lin = not toa and P_top > 0
    _lib.call("vsm_level_flux_lin", dt, N, pol.n, S, int(P), int(P_top), P_src, Pt(top_R_pm), None if toa else Pt(bot_R_mp),
              bot_stride, None if toa else Pt(dw_full), Pt(uw_full), Pt(top_R_pm_lin) if top_lin else None, S * N * N,
              Pt(top_J0_p_lin) if top_lin else None, None if toa else Pt(bot_R_mp_lin), bd_stride, sb * N * N,
              Pt(bot_J0_m_lin) if P else None, Pt(src_top_J0_p) if P_src and not toa else None,
              Pt(src_bot_J0_m) if P_src else None, nW, Pt(q), dh, ctype(float(mu0)), Pt(tau_sum), Pt(F0_I),
              Pt(tau_sum_dot) if tau_sum is not None and p_layer else None, int(p_layer), Pt(out), CR._stream_ptr())


@dataclass
class FluxLinResult(FX.FluxResult):
    """CoreRTLin.rt_run_fluxes: the fields of FluxResult and their derivatives, [nLevels, nSpec, Nparams (+ nPlanck)] in
    rt_run_lin's slot order (7 per aerosol, the gases, the surface, then the Planck slots)."""
    up_dot: np.ndarray
    down_diffuse_dot: np.ndarray          # exactly 0 at level 0
    down_direct_dot: np.ndarray           # -down_direct tau_sum_dot / mu0: layer slots only; exactly 0 at level 0
    actinic_up_dot: np.ndarray
    actinic_down_diffuse_dot: np.ndarray
    actinic_direct_dot: np.ndarray
    net_down_dot: np.ndarray              # down_direct_dot + down_diffuse_dot - up_dot
    absorbed_dot: Optional[np.ndarray]    # [Nz, nSpec, .]; None unless every level was computed
    surface_absorbed_dot: Optional[np.ndarray]   # [nSpec, .]; same rule


class _FluxSink(MSL.LevelSink):
    """The levels of a flux run: per level one elastic level call (the level vectors at all streams, no VZA row) and one
    level_flux_lin_ call, for the solar slot and, with a ThermalEmission, for the thermal slot.  buf (nLevels, 6 (nS + nT), S): per
    level the solar call's out (3, 2, nS = 1 + P, S) and the thermal call's (3, 2, nT = 1 + P + nPlanck, S), ONE array."""

    def __init__(self, sc: CL.SceneLin, plan: MS.LevelPlan, thermal: bool):
        self.plan, self.thermal = plan, thermal
        self.nS, self.nT = 1 + sc.P, (1 + sc.P + sc.nSrc) if thermal else 0
        dt, dev = sc.dt, sc.R.device
        self.buf = torch.empty((len(plan.distinct), 6 * (self.nS + self.nT), sc.S), dtype=dt, device=dev)
        self.row = {l: i for i, l in enumerate(plan.distinct)}
        qp = sc.qp
        mu, wt = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
        self.q = torch.as_tensor(np.stack([mu * wt, wt]).astype(sc.FT), device=dev)   # the flux row and the actinic row
        self.mu0 = float(qp.mu0)
        self.dir_h = (self.mu0, 1.0)
        self._F0_I = {}

    def _out(self, sc, l, thermal):
        b = self.buf[self.row[l]]
        n6 = 6 * self.nS
        return b[n6:].view(3, 2, self.nT, sc.S) if thermal else b[:n6].view(3, 2, self.nS, sc.S)

    def _beam(self, sc, mom, l, thermal):
        """(tau_sum, F0_I, tau_sum_dot) of level l: the solar slot's direct term; the thermal slot has none."""
        if thermal:
            return None, None, None
        if id(sc) not in self._F0_I:
            self._F0_I[id(sc)] = sc.F0[:, 0].contiguous()
        Nz = sc.fwd.Nz
        return (mom["tau_sum_surface"] if l == Nz else mom["layers"][l]["tau_sum"]), self._F0_I[id(sc)], sc.tau_sum_dot[l]

    def level(self, sc, mom, l, top, bot, src, thermal):
        S, N = sc.S, sc.N
        new = lambda: torch.empty((S, N), dtype=sc.dt, device=self.buf.device)
        dwf, uwf = new(), new()
        MS.level_radiance_(sc.pol, None, [], [], 0, 1.0, top[0], top[1], bot[0], bot[1], None, None, dwf, uwf)
        a_k, c_k = src if src is not None else (None, None)
        tau_sum, F0_I, tsd = self._beam(sc, mom, l, thermal)
        level_flux_lin_(sc.pol, sc.P, sc.pl, top[0], bot[0], dwf, uwf, top[2], top[3], bot[2], bot[3], a_k, c_k, self.q, self.dir_h,
                        self.mu0, tau_sum, F0_I, tsd, sc.pl, self._out(sc, l, thermal))

    def level0(self, sc, mom, J0_m, J0_m_lin, src_J0_m, thermal):
        tau_sum, F0_I, tsd = self._beam(sc, mom, 0, thermal)
        level_flux_lin_(sc.pol, sc.P, sc.pl, None, None, None, J0_m, None, None, None, J0_m_lin, None, src_J0_m, self.q, self.dir_h,
                        self.mu0, tau_sum, F0_I, tsd, sc.pl, self._out(sc, 0, thermal))


def bytes_per_point(N: int, P: int, pl: int, Nz: int, n_tops: int, segments: bool, n_levels: int, n_stokes: int, itemsize: int,
                    thermal: bool = False, nPlanck: int = 0) -> int:
    """Device bytes per spectral point of a linearized flux run: the estimate of the linearized multi-sensor run
    (core_rt_ms_lin.bytes_per_point) without its VZA outputs, and the 6 (1 + P) (+ 6 (1 + P + nPlanck)) scalars per level.
    nPlanck counts the Planck and the skin tables, as there (core_rt_ms_lin.thermal_estimate)."""
    per = MSL.bytes_per_point(N, P, pl, Nz, n_tops, segments, n_levels, n_stokes, 0, itemsize, thermal=thermal, nPlanck=nPlanck)
    return per + n_levels * 6 * ((1 + P) + ((1 + P + nPlanck) if thermal else 0)) * itemsize


def rt_run_fluxes(model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int, levels=None,
                  max_points: Optional[int] = None) -> FluxLinResult:
    """Up-, downwelling and actinic fluxes at layer boundaries of the column and their Jacobians, as a FluxLinResult: every field
    of CoreRT.rt_run_fluxes' FluxResult with the same meaning, row order (the caller's `levels`; None = all of 0..Nz) and level-0
    rule, and per field its derivative [nLevels, nSpec, Nparams (+ nPlanck)] in rt_run_lin's slot order:
        up_dot, down_diffuse_dot, down_direct_dot, actinic_up_dot, actinic_down_diffuse_dot, actinic_direct_dot, net_down_dot
    and, with every level computed, absorbed_dot [Nz, nSpec, .] and surface_absorbed_dot [nSpec, .].  The diffuse terms are the
    hemispheric quadratures of the derivative level vectors of CoreRTLin.rt_run_multisensor at m = 0 (rows of Stokes I), reduced
    on the device; down_direct_dot = -down_direct tau_sum_dot / mu0 for the layer slots (aerosols, gases), 0 for the surface and
    Planck slots.  At level 0 the diffuse-down terms and their derivatives are exactly 0, and so is down_direct_dot (tau_sum = 0).

    Model arguments, surfaces and NSurf as rt_run_lin takes them.  Only m = 0 is walked, whatever model.m_max is; where SceneLin
    runs m = 0 on its Stokes_IQ sub-scene, that sub-scene alone is walked.  Only the I row is reported.

    Sources: SolarBeam, and a ThermalEmission that states B_layer_dot ([0, rows, nSpec] for no Planck slot), by the opt-in rule of
    the linearized multi-sensor run; the thermal slot is solved on its own operators, its nPlanck slots follow the surface slots,
    and every field is the sum of the two slots.  SurfaceEmission: the slot's emitting lower boundary, its nSkin
    skin slots after the Planck slots.  ThermalEmission with B_layer_dot = None raises VSMError, SurfaceSIF and columns
    with a non-scattering layer NotImplementedError, N > 128 VSMError (the level kernel has no operator-level twin) -- each before
    any layer or level kernel is launched.

    max_points: run the spectral axis in blocks of about that many points (bit-identical to one pass; a block has at least
    SceneLin.LANE_POINTS points where the axis has); None = as many as fit the device."""
    Nz = int(np.asarray(model.tau_rayl).shape[1])
    plan = MS._validate(model, range(Nz + 1) if levels is None else levels, thermal=True, who=WHO)
    th = [s_ for s_ in (model.sources or ()) if isinstance(s_, H.ThermalEmission)]
    fwd_only = [s_ for s_ in th if getattr(s_, "B_layer_dot", None) is None]
    if fwd_only:
        raise _lib.VSMError("%s: a ThermalEmission takes part in this run by stating its Planck tables, B_layer_dot = [nPlanck, rows, "
                            "nSpec] (nPlanck = 0: no Planck slot); got %r with B_layer_dot = None" % (WHO, fwd_only[0]))
    qp, pol = model.quad_points, model.polarization_type
    N = qp.Nquad * pol.n
    if N > MSL.LEVEL_LIN_MAX_N:
        raise _lib.VSMError("%s: N = %d streams x Stokes components > %d, the limit of the linearized level kernel "
                            "(vsm_level_flux_lin_*)" % (WHO, N, MSL.LEVEL_LIN_MAX_N))
    model0 = dataclasses.replace(model, m_max=0)
    FT = model.float_type
    S_full = int(np.asarray(model.tau_rayl).shape[0])
    if max_points is None and S_full > 0:
        layout = H.ParameterLayout(n_aerosols=NAer, n_gases=NGas, n_surface=NSurf)
        P, pl = layout.n_total, layout.n_layer_params
        isz = np.dtype(FT).itemsize
        per = bytes_per_point(N, P, pl, Nz, plan.n_tops, bool(plan.interior), len(plan.distinct), pol.n, isz,
                              **MSL.thermal_estimate(model))
        if CL.REDUCE_M0 and pol.n >= 3:     # (the Stokes_IQ scene of m = 0, where it applies)
            per += bytes_per_point(2 * qp.Nquad, P, pl, Nz, plan.n_tops, bool(plan.interior), len(plan.distinct), 2, isz)
        free, _total = torch.cuda.mem_get_info()
        fit = int(0.5 * free // per)
        if fit < S_full:
            if fit < 1:
                raise _lib.VSMError("%s: not even one spectral point fits the device (%d bytes per point)" % (WHO, per))
            max_points = fit
    least = CL.SceneLin.LANE_POINTS if S_full >= CL.SceneLin.LANE_POINTS else 1
    parts = []
    nS = nT = 0
    blocks = MS.spectral_blocks(S_full, max_points, least)
    for sl in blocks:
        sc = CL.SceneLin(model0, lin_model, NAer, NGas, NSurf, spec_slice=sl)
        MS.refuse_non_scattering(sc.fwd.moments[0]["layers"], sc.FT, WHO,
                                 "; columns with a non-scattering layer are not supported (as for CoreRT.rt_run_fluxes)")
        # the thermal half of the sink exists where _run_scene runs the slot (SceneLin.has_thermal), and only there: a source that
        # emits nothing and states no table (an all-zero ThermalEmission or SurfaceEmission) would leave that half unwritten
        sink = _FluxSink(sc, plan, sc.has_thermal)
        nS, nT = sink.nS, sink.nT
        MSL._run_scene(sc, plan, False, sink)
        synchronize_if_gpu()
        _lib.check_device_status(WHO)
        parts.append(to_host(sink.buf))
        del sink, sc
        if len(blocks) > 1:
            torch.cuda.empty_cache()
    host = parts[0] if len(parts) == 1 else np.concatenate(parts, axis=2)
    nL, S = len(plan.distinct), host.shape[2]
    tot = np.zeros((nL, 3, 2, max(nS, nT), S), dtype=host.dtype)         # [level][up, down, direct][flux, actinic][slot][point]
    tot[:, :, :, :nS] = host[:, :6 * nS].reshape(nL, 3, 2, nS, S)
    if nT:
        tot += host[:, 6 * nS:].reshape(nL, 3, 2, nT, S)                 # the host adds the two slots
    row = {l: i for i, l in enumerate(plan.distinct)}
    idx = [row[l] for l in plan.levels]
    val = lambda d, r: tot[idx, d, r, 0].astype(FT, copy=True)
    dot = lambda d, r: np.ascontiguousarray(tot[idx, d, r, 1:].transpose(0, 2, 1)).astype(FT, copy=False)
    up, dn, direct = val(0, 0), val(1, 0), val(2, 0)
    upd, dnd, dird = dot(0, 0), dot(1, 0), dot(2, 0)
    net, netd = direct + dn - up, dird + dnd - upd
    absorbed = surface_absorbed = absorbed_dot = surface_absorbed_dot = None
    if plan.distinct == list(range(Nz + 1)):
        al = [row[l] for l in range(Nz + 1)]
        net_l = (tot[al, 2, 0, 0] + tot[al, 1, 0, 0] - tot[al, 0, 0, 0]).astype(FT, copy=False)
        netd_l = np.ascontiguousarray((tot[al, 2, 0, 1:] + tot[al, 1, 0, 1:] - tot[al, 0, 0, 1:]).transpose(0, 2, 1)).astype(FT, copy=False)
        absorbed, surface_absorbed = net_l[:-1] - net_l[1:], net_l[-1].copy()
        absorbed_dot, surface_absorbed_dot = netd_l[:-1] - netd_l[1:], netd_l[-1].copy()
    return FluxLinResult(levels=list(plan.levels), up=up, down_diffuse=dn, down_direct=direct, actinic_up=val(0, 1),
                         actinic_down_diffuse=val(1, 1), actinic_direct=val(2, 1), net_down=net, absorbed=absorbed,
                         surface_absorbed=surface_absorbed, up_dot=upd, down_diffuse_dot=dnd, down_direct_dot=dird,
                         actinic_up_dot=dot(0, 1), actinic_down_diffuse_dot=dot(1, 1), actinic_direct_dot=dot(2, 1),
                         net_down_dot=netd, absorbed_dot=absorbed_dot, surface_absorbed_dot=surface_absorbed_dot)
