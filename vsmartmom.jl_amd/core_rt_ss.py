"""Single-scattering runs: rt_run_ss(model) and rt_run_ss(RS_type::RRS, model, iBand) (src/CoreRT/rt_run.jl:574-755) on the MI355X,
through vsm_ss_column_* / vsm_ss_column_rrs_* (vsmartmom.jl_amd/csrc/vsm_ss.hip).

Mirrors rt_kernel_ss! (CoreKernel/rt_kernel_ss.jl:156-337: elemental! / elemental_inelastic! with ndoubl = 0 and dtau = the layer's
tau, scatter hard-wired to true), interaction_ss! / interaction_inelastic_ss! (CoreKernel/interaction_ss.jl), the surface's
interaction_ss! (rt_run.jl:715-722), postprocessing_vza! and the hemispherical sums of the moment m = 0 (rt_run.jl:737-748).  Per
Fourier moment the whole column is ONE launch (two for m = 0, whose second one writes the sources at all streams for hem_R /
hem_T; one more per moment for the Raman lines).  The run holds [S]- and [nVZA, nStokes, S]-sized arrays only (plus the surface
layer the existing builders fill, and [N,N,S] phase matrices for layers that mix scatterers per spectral point): no composite
layer, no [N,S,K] source array.
"""
from __future__ import annotations

import ctypes as C
import math
import numpy as np
import torch

from . import _lib
from . import host_model as H
from . import core_rt as CR
from .architectures import array_type, synchronize_if_gpu, to_host

MAX_HALO = 192   # VSM_SS_MAX_HALO of the library


def _ptr_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def ss_column_(dq: CR.DeviceQuad, m: int, tau, varpi, tau_sum, Zpp, Zmp, z_stride, F0, surf_j0_m, surf_j0_p, tau_sum_surface,
               row0, w, nV: int, R_SFI, T_SFI, J0_m=None, J0_p=None):
    """vsm_ss_column_*: one Fourier moment of the elastic single-scattering column.  tau / varpi / tau_sum / Zpp / Zmp: lists of L
    device tensors, z_stride: list of L ints (0 or N*N); row0 / w: _vza_rows_weights.  R_SFI / T_SFI (S, nStokes, nVZA) accumulate."""
    L, S = len(tau), int(F0.shape[0])
    q = dq.cstruct()
    zs = (C.c_longlong * L)(*[int(z) for z in z_stride])
    _lib.call("vsm_ss_column", dq.dtype, C.byref(q), S, L, m, _ptr_table(tau), _ptr_table(varpi), _ptr_table(tau_sum),
              _ptr_table(Zpp), _ptr_table(Zmp), zs, CR._ptr(F0), CR._ptr(surf_j0_m), CR._ptr(surf_j0_p), CR._ptr(tau_sum_surface),
              nV, row0, w, CR._ptr(R_SFI), CR._ptr(T_SFI), CR._ptr(J0_m), CR._ptr(J0_p), CR._stream_ptr())


def ss_column_rrs_(dq: CR.DeviceQuad, m: int, tau, tau_sum, fscatt, shift, varpi_ie, Zpp_ie, Zmp_ie, F0, halo: int, row0, w,
                   nV: int, ieR_SFI, ieT_SFI):
    """vsm_ss_column_rrs_*: one Fourier moment of the rotational-Raman single-scattering column (lists of L device tensors)."""
    L, S, K = len(tau), int(F0.shape[0]), int(shift.numel())
    q = dq.cstruct()
    _lib.call("vsm_ss_column_rrs", dq.dtype, C.byref(q), S, L, m, K, _ptr_table(tau), _ptr_table(tau_sum), _ptr_table(fscatt),
              CR._ptr(shift), CR._ptr(varpi_ie), CR._ptr(Zpp_ie), CR._ptr(Zmp_ie), CR._ptr(F0), int(halo), nV, row0, w,
              CR._ptr(ieR_SFI), CR._ptr(ieT_SFI), CR._stream_ptr())


def _refuse_sources(model: H.RTModel):
    for s_ in (model.sources or ()):
        if isinstance(s_, H.ThermalEmission):
            raise NotImplementedError("rt_run_ss: SolarBeam is the only source of a single-scattering run (got ThermalEmission)")


class SceneSS:
    """What rt_run_ss needs, resident in HBM: layer optics, Z moments and the surface layer exactly as CoreRT.Scene builds them for
    rt_run (a Scene with layers_only=True), plus, with an RRS type, the Raman phase matrices, fScattRayleigh and the line tables
    as SceneRRS builds them."""

    def __init__(self, model: H.RTModel, RS_type=None, iBand: int = 1):
        _refuse_sources(model)
        if iBand != 1:
            raise _lib.VSMError("single-band models only (iBand = 1)")
        self.model, self.rs = model, RS_type
        self.fwd = fwd = CR.Scene(model, layers_only=True)
        arch, FT = model.architecture, model.float_type
        self.FT, self.dt, dev = FT, fwd.dt, fwd.dev
        S, N, n, nV = fwd.S, fwd.N, fwd.pol.n, len(model.vza)
        self.J0_m = torch.zeros((S, N), dtype=self.dt, device=dev)   # the composite sources of m = 0 at all streams (hem_R / hem_T)
        self.J0_p = torch.zeros((S, N), dtype=self.dt, device=dev)
        self.out = [fwd.R_SFI, fwd.T_SFI] + [torch.zeros((S, n, nV), dtype=self.dt, device=dev) for _ in range(2)]
        self.drs = None
        if RS_type is not None:
            from . import core_rt_raman as RR
            conv = array_type(arch)
            self.drs = RR.device_rrs(RS_type, arch, FT)
            fscatt = RS_type.fscattRayl if RS_type.fscattRayl is not None else RR.default_fscatt(model)
            self.fscatt = conv(np.ascontiguousarray(np.asarray(fscatt, dtype=FT).T))          # (Nz, S): _expand_layer_rayleigh!
            g = RS_type.greek_raman
            tab = np.stack([np.asarray(getattr(g, k), dtype=np.float64) for k in ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")])
            gd = conv(np.ascontiguousarray(tab))
            q = fwd.dq.cstruct()
            self.Zie = []
            for m in range(model.m_max + 1):     # computeRamanZλ! (inelastic_helper.jl:917-924)
                Zp = torch.empty((1, N, N), dtype=self.dt, device=dev)
                Zm = torch.empty_like(Zp)
                _lib.call("vsm_compute_Z_moments", self.dt, C.byref(q), m, tab.shape[1], CR._ptr(gd), CR._ptr(Zp), CR._ptr(Zm),
                          CR._stream_ptr())
                self.Zie.append((Zp, Zm))
            sh = [abs(int(x)) for x in np.asarray(RS_type.i_lambda1lambda0).ravel() if abs(int(x)) < max(S, 1)]
            self.halo = min(max(sh or [0]), MAX_HALO)     # lines that can be in band at all; larger shifts read global memory

    def run(self):
        """rt_run.jl:671-749.  Asynchronous; returns the four (S, nStokes, nVZA) device tensors and J0-, J0+ (S, N) of m = 0."""
        model, fwd = self.model, self.fwd
        pol, qp, FT = fwd.pol, fwd.qp, self.FT
        for t in self.out + [self.J0_m, self.J0_p]:
            t.zero_()
        if fwd.S == 0:
            return tuple(self.out) + (self.J0_m, self.J0_p)
        R_SFI, T_SFI, ieR_SFI, ieT_SFI = self.out
        nV = len(model.vza)
        for mom in fwd.moments:
            m = mom["m"]
            weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
            layers = mom["layers"]
            props = [ly["props"].materialize() for ly in layers]     # Z[N,N,S] only where a layer mixes scatterers per point
            tau, tau_sum = [p.tau for p in props], [ly["tau_sum"] for ly in layers]
            CR.create_surface_layer_(model.surface, fwd.added_surface, m, fwd.dq, mom["tau_sum_surface"], rho=mom["rho"])
            row0, w = CR._vza_rows_weights(pol, model.vza, model.vaz, qp, m, float(weight), self.dt)
            full = m == 0
            ss_column_(fwd.dq, m, tau, [p.varpi for p in props], tau_sum, [p.Zpp for p in props], [p.Zmp for p in props],
                       [p.z_stride for p in props], fwd.F0, fwd.added_surface.j0_m, fwd.added_surface.j0_p, mom["tau_sum_surface"],
                       row0, w, nV, R_SFI, T_SFI, self.J0_m if full else None, self.J0_p if full else None)
            if self.drs is not None:
                Zp, Zm = self.Zie[m]
                ss_column_rrs_(fwd.dq, m, tau, tau_sum, [self.fscatt[iz] for iz in range(len(layers))], self.drs.shift,
                               self.drs.varpi_ie, Zp, Zm, fwd.F0, self.halo, row0, w, nV, ieR_SFI, ieT_SFI)
            del props
        return tuple(self.out) + (self.J0_m, self.J0_p)

    def results_host(self):
        """(R_SFI, T_SFI, ieR_SFI, ieT_SFI, hem_R, hem_T): [nVZA, nStokes, nSpec] x 4 and [nSpec] x 2 host arrays."""
        qp, n = self.fwd.qp, self.fwd.pol.n
        four = tuple(to_host(t).transpose(2, 1, 0).copy() for t in self.out)
        FT = self.FT
        mw = (np.asarray(qp.qp_mu, dtype=FT) * np.asarray(qp.wt_mu, dtype=FT)).astype(FT)
        hem_R = (to_host(self.J0_m)[:, ::n] * mw[None, :]).sum(axis=1).astype(FT)     # rt_run.jl:743-747: the Stokes-I rows
        hem_T = (to_host(self.J0_p)[:, ::n] * mw[None, :]).sum(axis=1).astype(FT)
        return four + (hem_R, hem_T)


def _run(model, RS_type, iBand):
    scene = SceneSS(model, RS_type, iBand)
    scene.run()
    synchronize_if_gpu()
    return scene.results_host()


def rt_run_ss(model: H.RTModel):
    """rt_run_ss(model) (rt_run.jl:574-576): the elastic single-scattering run.  Returns (R_SFI, T_SFI, ieR_SFI, ieT_SFI, hem_R,
    hem_T) as host arrays, the two inelastic arrays zero.  Every surface rt_run takes; SolarBeam is the only source."""
    return _run(model, None, 1)


def rt_run_ss_rrs(RS_type, model: H.RTModel, iBand: int = 1):
    """rt_run_ss(RS_type::RRS, model, iBand) (rt_run.jl:593-755): the single-scattering run with rotational Raman scattering -- the
    single-scatter inelastic correction.  Same inputs as CoreRTRaman.rt_run; K = 0 lines is legal."""
    return _run(model, RS_type, iBand)
