"""Single-scattering runs: rt_run_ss(model) and rt_run_ss(RS_type::RRS, model, iBand) (src/CoreRT/rt_run.jl:574-755) on the MI355X,
through vsm_ss_column_* / vsm_ss_column_rrs_* (vsmartmom.jl_amd/csrc/vsm_ss.hip), and the linearized elastic run
rt_run_ss(model, lin_model, NAer, NGas, NSurf) through vsm_ss_column_lin_* (SceneSSLin; the reference has no such driver), and
the linearized Raman run rt_run_ss_rrs_lin(RS_type, model, lin_model, ...) through vsm_ss_column_rrs_lin_* (SceneSSRamanLin; ours too).

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
import numpy as np
import torch

from . import _lib
from . import host_model as H
from . import core_rt as CR
from . import core_rt_lin as CL
from .architectures import array_type, synchronize_if_gpu, to_host

MAX_HALO = 192   # VSM_SS_MAX_HALO of the library


def _ptr_table(tensors, L=None):
    """A host table of device pointers (L entries where given); None stays None, a None entry is a null pointer."""
    if tensors is None:
        return None
    return (C.c_void_p * (len(tensors) if L is None else L))(*[None if t is None else t.data_ptr() for t in tensors])


def _tr(t):
    """A device result (S, nStokes, nVZA) or (P, S, nStokes, nVZA) on the host, axes reversed: [nVZA, nStokes, nSpec(, Nparams)]."""
    return to_host(t).T.copy()


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
        if isinstance(s_, H.SurfaceSIF):
            raise NotImplementedError("rt_run_ss: SolarBeam is the only source of a single-scattering run (got SurfaceSIF)")
        if isinstance(s_, H.SurfaceEmission):
            raise NotImplementedError("rt_run_ss: SolarBeam is the only source of a single-scattering run (got SurfaceEmission)")


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

    def run(self, after_moment=None):
        """rt_run.jl:671-749.  Asynchronous; returns the four (S, nStokes, nVZA) device tensors and J0-, J0+ (S, N) of m = 0.
        after_moment(mom, props, row0, w): called once per Fourier moment after its launches, with the materialised layer optics
        and the viewing-row tables of the moment while fwd.added_surface still holds the moment's surface layer (the linearized
        run launches its column there)."""
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
            weight = CR.fourier_weight(FT, m)
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
            if after_moment is not None:
                after_moment(mom, props, row0, w)
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


def ss_column_lin_(dq: CR.DeviceQuad, m: int, P: int, p_layer: int, p_zdot: int, tau, varpi, tau_sum, Zpp, Zmp, z_stride, tau_dot, varpi_dot,
                   tau_sum_dot, zdcoef, CT: int, Zc_pp, Zc_mp, F0, surf_j0_m, surf_j0_p, surf_j0_m_lin, surf_j0_p_lin,
                   tau_sum_surface, tau_sum_dot_surface, row0, w, nV: int, Rdot, Tdot, p_range=None):
    """vsm_ss_column_lin_*: one Fourier moment of the linearized single-scattering column.  Layer lists as in ss_column_, plus
    tau_dot / varpi_dot / tau_sum_dot (lists of L device tensors (p_layer, S); tau_dot of the layer's full tau) and zdcoef (None, or
    a list whose entries are None or (S, p_layer, CT) tensors, read for the first p_zdot slots: the aerosols').  Rdot / Tdot (P, S, nStokes, nVZA) accumulate the slots of
    p_range = (p_lo, p_hi) (default: all P)."""
    L, S = len(tau), int(F0.shape[0])
    q = dq.cstruct()
    zs = (C.c_longlong * L)(*[int(z) for z in z_stride])
    p_lo, p_hi = (0, P) if p_range is None else p_range
    tabs = [_ptr_table(t, L) for t in (tau, varpi, tau_sum, Zpp, Zmp, tau_dot, varpi_dot, tau_sum_dot, zdcoef)]
    _lib.call("vsm_ss_column_lin", dq.dtype, C.byref(q), S, L, m, P, p_layer, int(p_zdot), int(p_lo), int(p_hi), *tabs[:5], zs,
              *tabs[5:], int(CT), CR._ptr(Zc_pp), CR._ptr(Zc_mp), CR._ptr(F0), CR._ptr(surf_j0_m), CR._ptr(surf_j0_p),
              CR._ptr(surf_j0_m_lin), CR._ptr(surf_j0_p_lin), CR._ptr(tau_sum_surface), CR._ptr(tau_sum_dot_surface), nV, row0, w,
              CR._ptr(Rdot), CR._ptr(Tdot), CR._stream_ptr())


class SceneSSLin(CL.LinInputs):
    """What the linearized single-scattering run needs, resident in HBM: a SceneSS without Raman lines (R, T and the surface layer
    of the forward run come from it, through the same launches as rt_run_ss) plus the derivative optics of SceneLin
    (CoreRTLin.LinInputs: dtau_dot_all -- here of the layers' FULL tau, vsm_layer_optics_lin with an all-zero doubling table --,
    varpi_dot, tau_sum_dot, fz, zdcoef, Zall, the Cox-Munk (rho, drho)).  The one derivative layer it owns is the SHARED surface
    AddedLayerLin the linearized surface builders write (4 P N^2 + 2 P N S elements), with a shared forward AddedLayer beside it
    for the builder's own j0-: no added or composite layer, no derivative stack, nothing of size P N^2 S -- over the spectrally
    varying Lambertian surfaces too, whose builder runs in its vectors-only mode here (the column kernel reads j0- and ap_J0-+
    alone; the forward scene keeps its per-point surface layer)."""

    def __init__(self, model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int, RS_type=None, iBand: int = 1):
        _refuse_sources(model)
        self._check_lin_args(model, lin_model, NAer, NGas, NSurf)
        if 1 + 5 * NAer > 16:
            raise NotImplementedError("rt_run_ss (linearized): at most three aerosols (16 component blocks of Z_dot); got %d" % NAer)
        self.ss = SceneSS(model, RS_type, iBand)     # (an RS_type: SceneSSRamanLin's; the scene then launches the Raman column too)
        self.fwd = fwd = self.ss.fwd
        self._alloc_lin_optics()
        self._nd0 = torch.zeros(fwd.Nz, dtype=torch.int32, device=fwd.dev)
        self.upload()
        self.prepare()
        self._surface_tables()
        arch, FT, pol = self.arch, self.FT, self.pol
        self.added_s = CR.make_added_layer(FT, arch, (self.N, self.N), self.S, shared=True)
        self.als = CL.AddedLayerLin(FT, arch, self.P, self.N, self.S, shared=True)
        self.R, self.T = fwd.R_SFI, fwd.T_SFI
        self.Rd = torch.zeros((self.P, self.S, pol.n, len(model.vza)), dtype=self.dt, device=fwd.dev)
        self.Td = torch.zeros_like(self.Rd)

    def _ndoubl_table(self):
        return self._nd0       # tau_dot itself: this run's layers are not doubled

    def run(self):
        """Asynchronous; returns R, T (S, nStokes, nVZA) and Rdot, Tdot (P, S, nStokes, nVZA) on the device."""
        model, fwd = self.model, self.fwd
        S, P, pl, L = self.S, self.P, self.pl, fwd.Nz
        self.Rd.zero_()
        self.Td.zero_()
        if S == 0:
            self.ss.run()
            return self.R, self.T, self.Rd, self.Td
        nV = len(model.vza)
        tsd_s = self.tau_sum_dot[L]

        def lin_moment(mom, props, row0, w):
            """After the forward launches of the moment (fwd.added_surface holds the forward builder's surface layer: its j0+ is
            read here): the linearized builder's j0- and ap_J0-+ of all P slots, then the linearized column."""
            m, layers, tau_sum_s = mom["m"], mom["layers"], mom["tau_sum_surface"]
            self.surface_layer_lin_(mom, self.added_s, self.als, self.F0, vectors_only=True)
            zall = self.Zall[m] if self.Zall is not None else (None, None)
            ss_column_lin_(fwd.dq, m, P, pl, 7 * self.nAer if self.Zall is not None else 0, [p.tau for p in props],
                           [p.varpi for p in props], [ly["tau_sum"] for ly in layers], [p.Zpp for p in props],
                           [p.Zmp for p in props], [p.z_stride for p in props], [self.dtau_dot_all[iz] for iz in range(L)],
                           [self.varpi_dot[iz] for iz in range(L)], [self.tau_sum_dot[iz] for iz in range(L)],
                           None if self.zdcoef is None else [self.zdcoef[iz] for iz in range(L)], self.CT if self.Zall else 0,
                           zall[0], zall[1], self.F0, self.added_s.j0_m, fwd.added_surface.j0_p, self.als.ap_J0_m, self.als.ap_J0_p,
                           tau_sum_s, tsd_s, row0, w, nV, self.Rd, self.Td)
            self._after_lin_moment(mom, props, row0, w)

        self.ss.run(after_moment=lin_moment)     # R, T: the launches of rt_run_ss (bit for bit); one walk over the moments
        return self.R, self.T, self.Rd, self.Td

    def _after_lin_moment(self, mom, props, row0, w):
        """Further launches of the moment, after the linearized elastic column (SceneSSRamanLin: the linearized Raman column)."""

    def results_host(self):
        """(R, T, Rdot, Tdot): [nVZA, nStokes, nSpec] and [nVZA, nStokes, nSpec, Nparams], as rt_run_lin returns them."""
        return _tr(self.R), _tr(self.T), _tr(self.Rd), _tr(self.Td)


def rt_run_ss_lin(model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int):
    """The linearized elastic single-scattering run -> (R, T, Rdot, Tdot).  R, T are rt_run_ss(model)'s, bit for bit; Rdot / Tdot
    [nVZA, nStokes, nSpec, Nparams] are their analytic Jacobians in the parameter slots of rt_run_lin (ParameterLayout: 7 per
    aerosol, the gases, the surface slots: the Lambertian albedo or the Cox-Munk wind speed, the 4 / 3 parameters of an RPV / Ross-Li
    surface, or the K albedo slots of LambertianSurfaceLegendre / LambertianSurfaceSpline).  Same arguments and refusals as
    rt_run_lin; SolarBeam is the only source, at most three aerosols, no Cox-Munk single-scattering correction.  The surface
    slot and the surface's share of every slot are those of the reference's linearized surface builders, which weigh the direct
    beam with F0 where the forward builders use I0 = e1: with F0[0] = 1 (and, over Cox-Munk, F0 = e1) they are the exact
    derivatives of rt_run_ss, as in rt_run_lin."""
    scene = SceneSSLin(model, lin_model, NAer, NGas, NSurf)
    scene.run()
    synchronize_if_gpu()
    _lib.check_device_status("rt_run_ss (linearized)")
    return scene.results_host()


def ss_column_rrs_lin_(dq: CR.DeviceQuad, m: int, P: int, p_layer: int, tau, tau_sum, fscatt, tau_dot, tau_sum_dot, fscatt_dot, shift,
                       varpi_ie, Zpp_ie, Zmp_ie, F0, halo: int, row0, w, nV: int, ieRdot, ieTdot, p_range=None):
    """vsm_ss_column_rrs_lin_*: one Fourier moment of the linearized rotational-Raman single-scattering column.  Layer lists as in
    ss_column_rrs_, plus tau_dot / tau_sum_dot / fscatt_dot (lists of L device tensors (>= p_layer, S); tau_dot of the layer's full
    tau; None where p_layer = 0).  ieRdot / ieTdot (P, S, nStokes, nVZA) accumulate the slots of p_range = (p_lo, p_hi) (default:
    all P) below p_layer; the others are not touched."""
    L, S, K = len(tau), int(F0.shape[0]), int(shift.numel())
    q = dq.cstruct()
    p_lo, p_hi = (0, P) if p_range is None else p_range
    tabs = [_ptr_table(t, L) for t in (tau, tau_sum, fscatt, tau_dot, tau_sum_dot, fscatt_dot)]
    _lib.call("vsm_ss_column_rrs_lin", dq.dtype, C.byref(q), S, L, m, K, P, p_layer, int(p_lo), int(p_hi), *tabs, CR._ptr(shift),
              CR._ptr(varpi_ie), CR._ptr(Zpp_ie), CR._ptr(Zmp_ie), CR._ptr(F0), int(halo), nV, row0, w, CR._ptr(ieRdot),
              CR._ptr(ieTdot), CR._stream_ptr())


class SceneSSRamanLin(SceneSSLin):
    """The linearized single-scattering run with rotational Raman scattering: a SceneSSLin whose SceneSS carries the RS_type, so
    that one walk over the moments launches the elastic column, the Raman column (rt_run_ss_rrs's launches, bit for bit), the
    linearized elastic column (rt_run_ss_lin's) and, in the same after_moment hook, the linearized Raman column
    (vsm_ss_column_rrs_lin_*).  What it adds to the two scenes: fscatt_dot (Nz, max(p_layer, 1), S) and the two derivative outputs
    (P, S, nStokes, nVZA) -- nothing with a line axis, nothing of size P N^2 S.

    fscatt_dot: with RS_type.fscattRayl None, fscatt = tau_rayl / tau_scatt (default_fscatt) moves with the aerosol slots alone,
    whose tau_dot is d tau_scatt / dx exactly: fscatt_dot[p] = -fscatt^2 tau_dot[p] / tau_rayl there (0 where tau_rayl = 0), 0 on
    the gas slots; formed on the device from dtau_dot_all and the uploaded tau_rayl.  A stated fscattRayl needs a stated
    RS_type.fscattRayl_dot [7 NAer + NGas, nSpec, Nz]."""

    def __init__(self, RS_type, model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int, iBand: int = 1):
        if iBand != 1:
            raise _lib.VSMError("single-band models only (iBand = 1)")
        fsd = getattr(RS_type, "fscattRayl_dot", None)
        if RS_type.fscattRayl is not None and fsd is None:
            raise _lib.VSMError("rt_run_ss (linearized, RRS): a stated fscattRayl needs fscattRayl_dot [7 NAer + NGas, nSpec, Nz]: "
                                "its dependence on the parameters cannot be guessed")
        if fsd is not None:
            fsd = np.asarray(fsd, dtype=model.float_type)
            want = (7 * NAer + NGas,) + tuple(model.tau_rayl.shape)
            if fsd.shape != want:
                raise _lib.VSMError("RRS.fscattRayl_dot: [7 NAer + NGas, nSpec, Nz] = %r expected, got %r" % (want, fsd.shape))
        super().__init__(model, lin_model, NAer, NGas, NSurf, RS_type=RS_type, iBand=iBand)
        fwd, L, S, pl = self.fwd, self.fwd.Nz, self.S, self.pl
        self.fscatt_dot = torch.zeros((L, max(pl, 1), S), dtype=self.dt, device=fwd.dev)
        if fsd is not None:
            if pl:
                self.fscatt_dot.copy_(array_type(self.arch)(np.ascontiguousarray(fsd.transpose(2, 0, 1))))
        elif NAer:
            na = 7 * NAer
            rayl = fwd.tau_rayl_d[:, fwd.lo:fwd.lo + S]                                          # (L, S), FP64
            fs = self.ss.fscatt.to(torch.float64)
            d = -(fs * fs / rayl)[:, None, :] * self.dtau_dot_all[:, :na, :].to(torch.float64)
            self.fscatt_dot[:, :na, :] = torch.where((rayl > 0)[:, None, :], d, torch.zeros_like(d)).to(self.dt)
        self.ieR, self.ieT = self.ss.out[2], self.ss.out[3]
        self.ieRd, self.ieTd = torch.zeros_like(self.Rd), torch.zeros_like(self.Rd)

    def _after_lin_moment(self, mom, props, row0, w):
        L, ss, pl = self.fwd.Nz, self.ss, self.pl
        Zp, Zm = ss.Zie[mom["m"]]
        dots = lambda t: [t[iz] for iz in range(L)] if pl else None
        ss_column_rrs_lin_(self.fwd.dq, mom["m"], self.P, pl, [p.tau for p in props], [ly["tau_sum"] for ly in mom["layers"]],
                           [ss.fscatt[iz] for iz in range(L)], dots(self.dtau_dot_all), dots(self.tau_sum_dot),
                           dots(self.fscatt_dot), ss.drs.shift, ss.drs.varpi_ie, Zp, Zm, self.F0, ss.halo, row0, w,
                           len(self.model.vza), self.ieRd, self.ieTd)

    def run(self):
        """Asynchronous; returns R, T, ieR, ieT (S, nStokes, nVZA) and Rdot, Tdot, ieRdot, ieTdot (P, S, nStokes, nVZA)."""
        self.ieRd.zero_()
        self.ieTd.zero_()
        R, T, Rd, Td = super().run()
        return R, T, self.ieR, self.ieT, Rd, Td, self.ieRd, self.ieTd

    def results_host(self):
        """(R1, T1, ieR1, ieT1, R1dot, T1dot, ieR1dot, ieT1dot): [nVZA, nStokes, nSpec] x 4, [nVZA, nStokes, nSpec, Nparams] x 4."""
        return (_tr(self.R), _tr(self.T), _tr(self.ieR), _tr(self.ieT), _tr(self.Rd), _tr(self.Td), _tr(self.ieRd), _tr(self.ieTd))


def rt_run_ss_rrs_lin(RS_type, model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int, iBand: int = 1):
    """The linearized single-scattering run with rotational Raman scattering -> (R1, T1, ieR1, ieT1, R1dot, T1dot, ieR1dot,
    ieT1dot).  R1, T1, R1dot, T1dot are rt_run_ss_lin(model, lin_model, ...)'s and ieR1, ieT1 rt_run_ss_rrs(RS_type, model)'s, bit
    for bit; ieR1dot / ieT1dot [nVZA, nStokes, nSpec, Nparams] are the analytic Jacobians of the inelastic arrays in the slots of
    rt_run_lin (the surface slots exact zeros: the surface has no inelastic single-scattering part).  The parameters act through
    the layers' tau and tau_sum and through fScattRayleigh (SceneSSRamanLin); the line strengths and the Raman phase matrix are
    no parameters.  Refusals: those of rt_run_ss_lin and of rt_run_ss_rrs, and a stated RS_type.fscattRayl without
    fscattRayl_dot.  No sharding, no hem_R / hem_T derivatives, no spectral blocking."""
    scene = SceneSSRamanLin(RS_type, model, lin_model, NAer, NGas, NSurf, iBand)
    scene.run()
    synchronize_if_gpu()
    _lib.check_device_status("rt_run_ss (linearized, RRS)")
    return scene.results_host()
