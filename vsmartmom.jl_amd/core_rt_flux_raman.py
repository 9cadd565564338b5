"""Hemispheric fluxes with rotational Raman scattering at the layer boundaries of the column: CoreRTRaman.rt_run_fluxes
(DESIGN.md §4.19).

The level vectors of the Raman multi-sensor run (core_rt_ms_raman.py) at m = 0, the one Fourier moment that survives the azimuth
integral, reduced on the device to their hemispheric quadratures.  Per level: one elastic level call without viewing rows (its
level vectors at all streams are what the donors of the inelastic equation need in any case) and ONE call of vsm_level_flux_ie_*
(csrc/vsm_level.hip), which streams the lines of every recipient point, solves the inelastic level equation and leaves 5 nW
scalars per spectral point: the quadratures of the point's own elastic vectors, the direct beam, and those of its inelastic
vectors, which exist in LDS alone -- no (S, N) inelastic vector is allocated anywhere.  There is no walk here: the run hands
core_rt_ms_raman._run_scene a scene of that one moment and a sink (_FluxSink) that takes the place of its level calls.

Convention as in core_rt_flux.py, for the elastic (Cabannes) field and for the `_ie` field alike; the direct beam has no inelastic
part, and the total field is the sum of the two.
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
from . import core_rt_ms as MS
from . import core_rt_ms_raman as MSR
from . import core_rt_raman as RR
from . import host_model as H
from .architectures import synchronize_if_gpu, to_host

WHO = "rt_run_fluxes (RRS)"


def level_flux_ie_(pol, shift, top_R_pm, bot_R_mp, dw_full, uw_full, top_ieR_pm, top_ieJ0_p, bot_ieR_mp, bot_ieJ0_m, q, dir_h,
                   mu0: float, tau_sum, F0_I, out):
    """The hemispheric quadratures of the elastic and the inelastic level vectors at one boundary (vsm_level_flux_ie_*): the
    operands of core_rt_ms_raman.level_radiance_ie_ (A = top_R_pm (S, N, N), B = bot_R_mp ((S | 1, N, N)), dw_full / uw_full (S, N)
    the elastic level vectors, top_ieR_pm / bot_ieR_mp (K, S, N, N), top_ieJ0_p / bot_ieJ0_m (K, S, N); bot_ieR_mp = bot_ieJ0_m =
    None: a bottom without an inelastic part) and the weight rows and direct-beam operands of core_rt_flux.level_flux_ (q (nW,
    N / n) on the device, dir_h, mu0, tau_sum / F0_I (S,) or both None).  out (5, nW, S) is written, not accumulated:
        out[0][r] = sum_i q[r][i] uw_full[:, i n],   out[1][r] likewise of dw_full,   out[2][r] = dir_h[r] F0_I exp(-tau_sum / mu0),
        out[3][r], out[4][r] the same quadratures of uw_ie / dw_ie of level_radiance_ie_.
    top_R_pm None: the TOA -- dw = dw_ie = 0, uw = uw_full, uw_ie = the sum of bot_ieJ0_m over the in-band lines; bot_R_mp, dw_full
    and the other inelastic operands are not read (bot_ieR_mp is still given with bot_ieJ0_m, or both are None).  N <= 128."""
    S, N = int(uw_full.shape[0]), int(uw_full.shape[1])
    dt = uw_full.dtype
    nW = int(q.shape[0])
    K = int(shift.numel())
    toa = top_R_pm is None
    if (tau_sum is None) != (F0_I is None):
        raise _lib.VSMError("level_flux_ie_: tau_sum and F0_I are given together or not at all")
    bot_stride = N * N if toa else MS.bot_stride_of(bot_R_mp, S, N)
    ctype = C.c_double if dt == torch.float64 else C.c_float
    dh = (ctype * max(nW, 1))(*[float(x) for x in dir_h])
    P = CR._ptr
    _lib.call("vsm_level_flux_ie", dt, N, pol.n, S, K, P(shift), P(top_R_pm), None if toa else P(bot_R_mp), bot_stride,
              None if toa else P(dw_full), P(uw_full), None if toa else P(top_ieR_pm), None if toa else P(top_ieJ0_p),
              P(bot_ieR_mp), P(bot_ieJ0_m), nW, P(q), dh, ctype(float(mu0)), P(tau_sum), P(F0_I), P(out),
              CR._stream_ptr())


@dataclass
class RamanFluxResult(FX.FluxResult):
    """CoreRTRaman.rt_run_fluxes: the fields of FluxResult for the elastic (Cabannes) field and, summed over the Raman lines, the
    inelastic field, host arrays in the model's float type; the rows follow `levels`.  The direct beam has no inelastic part; the
    total field is the sum of the elastic and the `_ie` fields."""
    up_ie: np.ndarray                        # [nLevels, nSpec]  sum_i mu_i w_i uwie_I[i]
    down_diffuse_ie: np.ndarray              # sum_i mu_i w_i dwie_I[i]; exactly 0 at level 0
    actinic_up_ie: np.ndarray                # sum_i w_i uwie_I[i]
    actinic_down_diffuse_ie: np.ndarray      # sum_i w_i dwie_I[i]; exactly 0 at level 0
    net_down_ie: np.ndarray                  # down_diffuse_ie - up_ie
    absorbed_ie: Optional[np.ndarray]        # [Nz, nSpec] net_down_ie[l - 1] - net_down_ie[l]; None unless every level was computed
    surface_absorbed_ie: Optional[np.ndarray]    # [nSpec] net_down_ie[Nz]; same rule


class _FluxSink(MSR.LevelSink):
    """The flux run's place in the walk of core_rt_ms_raman._run_scene: per level one elastic level call (the level vectors at
    all streams, no VZA row) and one level_flux_ie_ call into its row of ONE (len(plan.distinct), 5, 2, S) device tensor -- per
    level [up, down, direct, up_ie, down_ie] x [flux, actinic] --, so that ONE copy brings a block home."""

    def __init__(self, sc: RR.SceneRRS, plan: MS.LevelPlan):
        fwd = sc.fwd
        self.sc, self.pol, self.Nz = sc, fwd.pol, fwd.Nz
        dev = sc.out[0].device
        self.buf = torch.empty((len(plan.distinct), 5, 2, sc.S), dtype=sc.dt, device=dev)
        self.out = {l: self.buf[i] for i, l in enumerate(plan.distinct)}
        qp = fwd.qp
        mu, wt = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
        self.q = torch.as_tensor(np.stack([mu * wt, wt]).astype(sc.FT), device=dev)   # the flux row and the actinic row
        self.mu0 = float(qp.mu0)
        self.dir_h = (self.mu0, 1.0)
        self.F0_I = fwd.F0[:, 0].contiguous()

    def _flux(self, mom, l, A, B, dwf, uwf, Aie, aie, Bie, cie):
        tau_sum = mom["tau_sum_surface"] if l == self.Nz else mom["layers"][l]["tau_sum"]
        level_flux_ie_(self.pol, self.sc.drs.shift, A, B, dwf, uwf, Aie, aie, Bie, cie, self.q, self.dir_h, self.mu0, tau_sum,
                       self.F0_I, self.out[l])

    def level(self, mom, l, top, bot):
        sc = self.sc
        new = lambda: torch.empty((sc.S, sc.N), dtype=sc.dt, device=self.buf.device)
        dwf, uwf = new(), new()
        MS.level_radiance_(self.pol, None, [], [], 0, 1.0, top[0], top[1], bot[0], bot[1], None, None, dwf, uwf)
        self._flux(mom, l, top[0], bot[0], dwf, uwf, top[2], top[3], bot[2], bot[3])

    def level0(self, mom, comp, comp_rs):      # nothing diffuse goes down at the TOA
        self._flux(mom, 0, None, None, None, comp.J0_m, None, None, comp_rs.ieR_mp, comp_rs.ieJ0_m)


def rt_run_fluxes(RS_type: RR.RRS, model: H.RTModel, levels=None, iBand: int = 1,
                  max_points: Optional[int] = None) -> RamanFluxResult:
    """Up-, downwelling and actinic fluxes with rotational Raman scattering at layer boundaries of the column, as a
    RamanFluxResult of [nLevels, nSpec] host arrays: the Ring effect in an irradiance or an actinic flux, without a level vector
    on the host.

    levels as in CoreRT.rt_run_fluxes: 0 = TOA, l = below layer l, Nz = just above the surface; None = all of 0..Nz; duplicates and
    any order allowed (each distinct level is computed once, the rows follow the caller's order).  Every field of FluxResult
    describes the elastic (Cabannes) field, with CoreRT.rt_run_fluxes' formulae, units and level-0 rule, from the m = 0 level
    vectors uw / dw of CoreRTRaman.rt_run_multisensor; with uwie / dwie its inelastic level vectors, summed over the lines,
        up_ie = sum_i mu_i w_i uwie_i              down_diffuse_ie = sum_i mu_i w_i dwie_i
        actinic_up_ie = sum_i w_i uwie_i           actinic_down_diffuse_ie = sum_i w_i dwie_i
        net_down_ie = down_diffuse_ie - up_ie
    (the rows of Stokes I).  The direct beam has no inelastic part; the total field is the sum of the elastic and the `_ie`
    fields.  Level 0 is the TOA itself: up / up_ie are J0- / the line sum of ieJ0- of the whole column with the surface, and every
    diffuse down term, elastic and inelastic, is exactly 0 there -- NOT rt_run_multisensor's level-0 dw / dwie, which are rt_run's
    T / ieT, the field at the bottom of the column (that is down_diffuse(_ie) at level Nz).  Level Nz takes the surface layer alone
    as the bottom, whose inelastic part is zero.  With every level computed, absorbed_ie [Nz, nSpec] = net_down_ie[l - 1] -
    net_down_ie[l] and surface_absorbed_ie [nSpec] = net_down_ie[Nz] beside absorbed / surface_absorbed; otherwise all four are
    None.

    Only m = 0 is walked, whatever model.m_max is, on the scene SceneRRS itself uses for that moment: the Stokes_IQ sub-scene
    where it reduces m = 0.  Only the I row is reported: no Q / U / V fluxes.  No Jacobian, no sharding through vsm.parallel.
    Surfaces: model.surface, as CoreRTRaman.rt_run_multisensor takes it (no Cox-Munk single-scattering correction, like
    CoreRT.rt_run_fluxes).

    Sources and refusals are those of CoreRTRaman.rt_run_multisensor, before anything is launched: SolarBeam only (SurfaceSIF,
    SurfaceEmission: NotImplementedError; ThermalEmission: VSMError), iBand = 1, N <= 128 (VSMError).  Columns with non-scattering
    layers run, with rt_run(RRS)'s convention for the _00 / _01 / _10 tags, as there.

    max_points: walk the recipient axis in blocks of at most that many points, each extended by the halo of max|shift| donor
    points and cropped (bit-identical to the one-pass run); None = as many as fit the device (raman_bytes_per_point with the
    kept tops).  Those tops dominate a run over all levels: (1 + K)(N^2 + N) elements per level and point (R+-, J0+ and, per
    line, ieR+-, ieJ0+) -- N = 40, K = 70, 40 levels, FP64: 37 MB per point."""
    Nz = int(np.asarray(model.tau_rayl).shape[1])
    plan = MSR._validate(RS_type, model, range(Nz + 1) if levels is None else levels, iBand)
    model0 = dataclasses.replace(model, m_max=0)
    S_full = int(np.asarray(model.tau_rayl).shape[0])
    shifts = np.asarray(RS_type.i_lambda1lambda0).ravel()
    if max_points is None and S_full > 0:
        qp, pol = model.quad_points, model.polarization_type
        N, K, isz = qp.Nquad * pol.n, len(shifts), np.dtype(model.float_type).itemsize
        per = RR.raman_bytes_per_point(N, K, isz, n_tops=plan.n_tops, segments=bool(plan.interior))
        if RR.REDUCE_M0 and pol.n >= 3:   # (the outer scene holds no tops: the walk is the sub-scene's)
            per = RR.raman_bytes_per_point(N, K, isz) + RR.raman_bytes_per_point(2 * qp.Nquad, K, isz, n_tops=plan.n_tops,
                                                                                 segments=bool(plan.interior))
        per += 10 * len(plan.distinct) * isz
        free, _total = torch.cuda.mem_get_info()
        halo = max([abs(int(x)) for x in shifts if abs(int(x)) < S_full] or [0])
        fit = int(0.8 * free // per) - 2 * halo
        if fit < S_full:
            if fit < 1:
                raise _lib.VSMError("%s: not even one block of recipient points fits the device (%d bytes per point, halo %d)"
                                    % (WHO, per, halo))
            max_points = fit
    parts = []
    blocks = MS.spectral_blocks(S_full, max_points)
    for sl in blocks:
        sc = RR.SceneRRS(RS_type, model0, iBand, sl)      # (m = 0 alone), a SceneRRS over the block and its halo
        if sc.sub0 is not None:
            sc = sc.sub0
        sink = _FluxSink(sc, plan)
        MSR._run_scene(sc, plan, False, sink)
        out = sink.buf[..., sc.crop]
        del sc, sink
        synchronize_if_gpu()
        _lib.check_device_status(WHO)
        parts.append(to_host(out))
        del out
        if len(blocks) > 1:
            torch.cuda.empty_cache()
    host = np.concatenate(parts, axis=3)
    res = {l: host[i] for i, l in enumerate(plan.distinct)}                                  # (5, 2, nSpec)
    FT = model.float_type
    pick = lambda d, r: np.stack([res[l][d, r] for l in plan.levels]).astype(FT, copy=False)
    up, dn, direct, up_ie, dn_ie = (pick(d, 0) for d in range(5))
    absorbed = surface_absorbed = absorbed_ie = surface_absorbed_ie = None
    if plan.distinct == list(range(Nz + 1)):
        net_l = np.stack([res[l][2, 0] + res[l][1, 0] - res[l][0, 0] for l in range(Nz + 1)]).astype(FT, copy=False)
        absorbed, surface_absorbed = net_l[:-1] - net_l[1:], net_l[-1].copy()
        net_l = np.stack([res[l][4, 0] - res[l][3, 0] for l in range(Nz + 1)]).astype(FT, copy=False)
        absorbed_ie, surface_absorbed_ie = net_l[:-1] - net_l[1:], net_l[-1].copy()
    return RamanFluxResult(levels=list(plan.levels), up=up, down_diffuse=dn, down_direct=direct, actinic_up=pick(0, 1),
                           actinic_down_diffuse=pick(1, 1), actinic_direct=pick(2, 1), net_down=direct + dn - up, absorbed=absorbed,
                           surface_absorbed=surface_absorbed, up_ie=up_ie, down_diffuse_ie=dn_ie, actinic_up_ie=pick(3, 1),
                           actinic_down_diffuse_ie=pick(4, 1), net_down_ie=dn_ie - up_ie, absorbed_ie=absorbed_ie,
                           surface_absorbed_ie=surface_absorbed_ie)
