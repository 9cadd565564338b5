"""Linearized (Jacobian) CoreRT host layer: rt_run(model, lin_model, NAer, NGas, NSurf)
(src/CoreRT/rt_run_lin.jl:72-78, :102-326) on the MI355X, through the C ABI.

Mirrors: make_added_layer / make_composite_layer (LinMode) (tools/rt_helper_functions_lin.jl:15-80),
elemental! / doubling_allparams! / interaction! (lin) (CoreKernel/*_lin.jl), create_surface_layer! (lin),
postprocessing_vza! (lin).  FP64 with 8 <= N <= 60 runs the fused column-strip kernels (vsm_striplin.hip: one launch
per doubling step, two per interaction); other shapes run operator level (batched MFMA products over (spectral point,
parameter)); inverses are shared by all parameters like in the reference.  `SceneLin` keeps every input in HBM.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import host_model as H
from . import core_rt as CR
from . import core_rt_ms as MS
from .architectures import array_type, devi, synchronize_if_gpu, to_host


class AddedLayerLin:
    """types_lin.jl:20-60 AddedLayerLin (`ap_*` all-parameter fields)."""

    def __init__(self, FT, arch, P, N, nSpec, shared=False):
        dev, dt = devi(arch), CR._torch_dtype(FT)
        sm = 1 if shared else nSpec
        z = lambda: torch.zeros((P, sm, N, N), dtype=dt, device=dev)
        self.ap_r_mp, self.ap_t_pp, self.ap_r_pm, self.ap_t_mm = z(), z(), z(), z()
        self.ap_J0_p = torch.zeros((P, nSpec, N), dtype=dt, device=dev)
        self.ap_J0_m = torch.zeros((P, nSpec, N), dtype=dt, device=dev)
        self.P, self.N, self.nSpec, self.shared, self.dtype = P, N, nSpec, shared, dt

    def cstruct(self):
        return _lib.vsm_added_lin(self.ap_r_mp.data_ptr(), self.ap_t_pp.data_ptr(), self.ap_r_pm.data_ptr(),
                                  self.ap_t_mm.data_ptr(), self.ap_J0_p.data_ptr(), self.ap_J0_m.data_ptr(), self.P, 0,
                                  0 if self.shared else self.N * self.N)


class CompositeLayerLin:
    """types_lin.jl:62-97 CompositeLayerLin."""

    def __init__(self, FT, arch, P, N, nSpec):
        dev, dt = devi(arch), CR._torch_dtype(FT)
        z = lambda: torch.zeros((P, nSpec, N, N), dtype=dt, device=dev)
        self.R_mp, self.R_pm, self.T_pp, self.T_mm = z(), z(), z(), z()
        self.J0_p = torch.zeros((P, nSpec, N), dtype=dt, device=dev)
        self.J0_m = torch.zeros((P, nSpec, N), dtype=dt, device=dev)
        self.P, self.N, self.nSpec, self.dtype = P, N, nSpec, dt

    def cstruct(self):
        return _lib.vsm_composite_lin(self.R_mp.data_ptr(), self.R_pm.data_ptr(), self.T_pp.data_ptr(),
                                      self.T_mm.data_ptr(), self.J0_p.data_ptr(), self.J0_m.data_ptr(), self.P, 0)


class _CompositeAsAdded:
    """A composite of LOWER layers handed to interaction! as its added layer: the adding equations are associative and the sources
    of every layer carry their absolute attenuation from the top of the atmosphere, so composites of sub-columns combine like layers
    (SceneLin: the interactions of a small batch as a tree).  All four matrices are in memory (no D-symmetry is assumed)."""

    def __init__(self, comp: CR.CompositeLayer):
        self.comp, self.N, self.nSpec, self.dtype = comp, comp.N, comp.nSpec, comp.dtype

    def cstruct(self):
        c = self.comp.cstruct()
        return _lib.vsm_added(c.R_mp, c.T_pp, c.R_pm, c.T_mm, c.J0_p, c.J0_m, self.N * self.N, 0, 0)


class _CompositeLinAsAdded:
    def __init__(self, cl: "CompositeLayerLin"):
        self.cl, self.P = cl, cl.P

    def cstruct(self):
        c = self.cl
        return _lib.vsm_added_lin(c.R_mp.data_ptr(), c.T_pp.data_ptr(), c.R_pm.data_ptr(), c.T_mm.data_ptr(), c.J0_p.data_ptr(),
                                  c.J0_m.data_ptr(), c.P, 0, c.N * c.N)


def to_device_sp(x: np.ndarray, arch, FT) -> torch.Tensor:
    """[S, p] host array -> device tensor in the reference's [S, p] column-major order (shape (p, S))."""
    return array_type(arch)(np.ascontiguousarray(np.asarray(x, dtype=FT).T))


def to_device_zdot(Zd: Optional[np.ndarray], arch, FT):
    """[p,N,N] or [p,S,N,N] math order -> layout tensor + (stride_s, stride_p) in elements."""
    if Zd is None:
        return None, 0, 0
    Zd = np.asarray(Zd, dtype=FT)
    if Zd.ndim == 3:
        t = array_type(arch)(np.ascontiguousarray(Zd.transpose(0, 2, 1)))
        N = Zd.shape[-1]
        return t, 0, N * N
    t = array_type(arch)(np.ascontiguousarray(Zd.transpose(0, 1, 3, 2)))
    P, S, N, _ = Zd.shape
    return t, N * N, N * N * S


def elemental_lin_(pol, tau_sum, tau_sum_dot, dtau, dtau_dot, F0, props: CR.DeviceLayerOptics, varpi_dot, Zpp_dot,
                   Zmp_dot, zd_strides, p_layer, m, ndoubl, dq: CR.DeviceQuad, added: CR.AddedLayer, added_lin: AddedLayerLin,
                   n_m0: int = 0):
    """elemental! (lin): elemental_lin.jl:77-206.  n_m0 > 0: a batch with Fourier moments folded into it whose first n_m0 points are
    (moment 0, point) pairs and the others pairs of moments m > 0 (vsm_elemental_lin_fold)."""
    q, a, al = dq.cstruct(), added.cstruct(), added_lin.cstruct()
    if n_m0:
        _lib.call("vsm_elemental_lin_fold", added.dtype, C.byref(q), added.nSpec, m, int(n_m0), ndoubl, CR._ptr(dtau),
                  CR._ptr(props.varpi), CR._ptr(tau_sum), CR._ptr(F0), CR._ptr(props.Zpp), CR._ptr(props.Zmp), props.z_stride, p_layer,
                  CR._ptr(dtau_dot), CR._ptr(varpi_dot), CR._ptr(tau_sum_dot), C.byref(a), C.byref(al), CR._stream_ptr())
        return
    _lib.call("vsm_elemental_lin", added.dtype, C.byref(q), added.nSpec, m, ndoubl, CR._ptr(dtau), CR._ptr(props.varpi),
              CR._ptr(tau_sum), CR._ptr(F0), CR._ptr(props.Zpp), CR._ptr(props.Zmp), props.z_stride, p_layer,
              CR._ptr(dtau_dot), CR._ptr(varpi_dot), CR._ptr(tau_sum_dot), CR._ptr(Zpp_dot), CR._ptr(Zmp_dot),
              zd_strides[0], zd_strides[1], C.byref(a), C.byref(al), CR._stream_ptr())


# The kernel-driven land BRDFs and their Jacobian slots, in the order of the dataclass fields (the reference linearizes neither):
# surface type -> (kind of vsm_land_brdf_reflectance_lin_*, number of parameters = the NSurf the linearized drivers take)
LAND_BRDF = {H.rpvSurfaceScalar: (0, 4), H.RossLiSurfaceScalar: (1, 3)}


SPECTRAL_LAMBERTIAN = (H.LambertianSurfaceLegendre, H.LambertianSurfaceSpline)   # per-point albedo: per-point surface layers
LAMBERTIAN = (H.LambertianSurfaceScalar,) + SPECTRAL_LAMBERTIAN


def surface_param_names(surface):
    """The surface's Jacobian slots in order: the fields of its dataclass; the coefficients c0 .. c{K-1} of
    LambertianSurfaceLegendre; the tables albedo_dot[k] of LambertianSurfaceSpline."""
    if isinstance(surface, SPECTRAL_LAMBERTIAN):
        fmt = "c%d" if isinstance(surface, H.LambertianSurfaceLegendre) else "albedo_dot[%d]"
        return [fmt % k for k in range(H.surface_albedo_slots(surface))]
    return [f.name for f in dataclasses.fields(surface)]


def land_brdf_reflectance_lin(surface, dq: CR.DeviceQuad, m_max: int, arch, FT):
    """vsm_land_brdf_reflectance_lin_*: the Fourier blocks of a kernel-driven land BRDF and their parameter derivatives for the
    moments 0 .. m_max in one launch -> layout tensors rho (m_max + 1, N, N), drho (m_max + 1, K, N, N) [column-major blocks];
    the integral host_model.brdf_reflectance evaluates, on the azimuth nodes of brdf_azimuth_quadrature."""
    kind, K = LAND_BRDF[type(surface)]
    N = int(dq.mu.numel())
    rho = torch.empty((m_max + 1, N, N), dtype=dq.dtype, device=dq.mu.device)
    drho = torch.empty((m_max + 1, K, N, N), dtype=dq.dtype, device=dq.mu.device)
    phi, w = CR.brdf_azimuth_quadrature(arch, FT)
    ctype = C.c_double if dq.dtype == torch.float64 else C.c_float
    params = (ctype * K)(*[float(getattr(surface, n)) for n in surface_param_names(surface)])
    q = dq.cstruct()
    _lib.call("vsm_land_brdf_reflectance_lin", dq.dtype, C.byref(q), kind, params, int(m_max), int(phi.numel()), CR._ptr(phi),
              CR._ptr(w), CR._ptr(rho), CR._ptr(drho), CR._stream_ptr())
    return rho, drho


def brdf_surface_lin_multi_(dq: CR.DeviceQuad, S: int, m: int, rho, drho, isurf: int, tau_sum, tau_sum_dot, p_layer: int, F0,
                            added_s: CR.AddedLayer, als: AddedLayerLin):
    """vsm_brdf_surface_lin_multi_*: the linearized BRDF surface layer with the K = drho.shape[0] surface slots isurf .. isurf + K - 1
    into the shared surface layers `added_s` / `als`."""
    q_, a_, al_ = dq.cstruct(), added_s.cstruct(), als.cstruct()
    _lib.call("vsm_brdf_surface_lin_multi", added_s.dtype, C.byref(q_), S, m, CR._ptr(rho), CR._ptr(drho), int(drho.shape[0]),
              int(isurf), CR._ptr(tau_sum), CR._ptr(tau_sum_dot), p_layer, CR._ptr(F0), C.byref(a_), C.byref(al_), CR._stream_ptr())


def lambertian_surface_spectral_lin_(dq: CR.DeviceQuad, S: int, m: int, albedo, basis, isurf: int, tau_sum, tau_sum_dot, p_layer: int,
                                     F0, added_s: CR.AddedLayer, als: AddedLayerLin, vectors_only: bool = False):
    """vsm_lambertian_surface_spectral_lin_*: the linearized surface layer of a spectrally varying Lambertian albedo -- albedo (S,),
    basis (K, S) device tensors -- with the K = basis.shape[0] albedo slots isurf .. isurf + K - 1 into the PER-POINT surface
    layers `added_s` / `als`; vectors_only: j0+-, ap_J0+- alone (the layers may then be the shared ones)."""
    q_, a_, al_ = dq.cstruct(), added_s.cstruct(), als.cstruct()
    _lib.call("vsm_lambertian_surface_spectral_lin", added_s.dtype, C.byref(q_), S, m, CR._ptr(albedo), CR._ptr(basis),
              int(basis.shape[0]), int(isurf), CR._ptr(tau_sum), CR._ptr(tau_sum_dot), p_layer, CR._ptr(F0), C.byref(a_), C.byref(al_),
              1 if vectors_only else 0, CR._stream_ptr())


_lin_work = {}


def _work(kind, n, dtype, device, lane):
    """The scratch buffer of kernel `kind` on moment lane `lane` (the stream the caller launches on): one per lane, grow-only."""
    key = (kind, dtype, str(device), lane)
    w = _lin_work.get(key)
    if w is None or w.numel() < n:
        w = _lib.poison(torch.empty(int(n), dtype=dtype, device=device))
        _lin_work[key] = w
    return w


def doubling_allparams_(pol, expk, ndoubl, added: CR.AddedLayer, added_lin: AddedLayerLin, dtau_dot_all, mu0, N_active, lane=0):
    """doubling_allparams! (doubling_lin.jl:216-339).  lane: the moment lane the caller launches on (its scratch buffer)."""
    n = _lib.lib().vsm_doubling_lin_work_elems(added.N, added.nSpec, max(N_active, 1) if N_active else added_lin.P)
    work = _work("dbl", max(int(n), 1), added.dtype, added.r_mp.device, lane)
    a, al = added.cstruct(), added_lin.cstruct()
    mu = C.c_double(mu0) if added.dtype == torch.float64 else C.c_float(mu0)
    _lib.call("vsm_doubling_lin", added.dtype, added.N, pol.n, added.nSpec, ndoubl, CR._ptr(expk), CR._ptr(dtau_dot_all),
              mu, N_active, C.byref(a), C.byref(al), CR._ptr(work), CR._stream_ptr())


def interaction_lin_(scattering_interface, comp: CR.CompositeLayer, comp_lin: CompositeLayerLin, added: CR.AddedLayer,
                     added_lin: AddedLayerLin, p_range=None, lane=0):
    """interaction! (lin) (interaction_lin.jl:337-351).  `p_range = (p_lo, p_hi)`: only these parameter slots (the caller knows
    the others to be zero in both operands, where the reference's loop over all Nparams computes exact zeros).  lane: as in
    doubling_allparams_."""
    n = _lib.lib().vsm_interaction_lin_work_elems(comp.N, comp.nSpec, comp_lin.P)
    work = _work("ia", int(n), comp.dtype, comp.R_mp.device, lane)
    c, cl, a, al = comp.cstruct(), comp_lin.cstruct(), added.cstruct(), added_lin.cstruct()
    if p_range is not None and (p_range[0] > 0 or p_range[1] < comp_lin.P) and p_range[1] > p_range[0]:
        _lib.call("vsm_interaction_lin_range", comp.dtype, CR.IFACE[scattering_interface], comp.N, comp.nSpec, C.byref(c),
                  C.byref(cl), C.byref(a), C.byref(al), int(p_range[0]), int(p_range[1]), CR._ptr(work), CR._stream_ptr())
        return
    _lib.call("vsm_interaction_lin", comp.dtype, CR.IFACE[scattering_interface], comp.N, comp.nSpec, C.byref(c),
              C.byref(cl), C.byref(a), C.byref(al), CR._ptr(work), CR._stream_ptr())


def copy_added_to_composite_lin_(comp: CR.CompositeLayer, comp_lin: CompositeLayerLin, added: CR.AddedLayer, added_lin: AddedLayerLin):
    """The TOA layer of a walk: the added layer and its derivative stacks become the composite."""
    CR.copy_added_to_composite_(comp, added)
    a, c = added_lin.cstruct(), comp_lin.cstruct()
    _lib.call("vsm_copy_added_to_composite_lin", added.dtype, added.N, added.nSpec, C.byref(a), C.byref(c), CR._stream_ptr())


def postprocessing_vza_lin_(pol, comp: CR.CompositeLayer, comp_lin: CompositeLayerLin, vza, vaz, qp, m, weight: float, R, T, Rd, Td):
    """postprocessing_vza! and its linearized twin (postprocessing_vza.jl:23-94): R / T (S, nStokes, nVZA) and Rd / Td
    (P, S, nStokes, nVZA) accumulate the moment's viewing rows."""
    CR.postprocessing_vza_(pol, comp, vza, vaz, qp, m, weight, R, T)
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, m, weight, comp.dtype)
    _lib.call("vsm_postprocess_vza_lin", comp.dtype, comp.N, pol.n, comp.nSpec, len(vza), comp_lin.P, row0, w,
              CR._ptr(comp_lin.J0_m), CR._ptr(comp_lin.J0_p), CR._ptr(Rd), CR._ptr(Td), CR._stream_ptr())


# Fourier moments per vsm_mix_Z_moments call (VSM_MM_MAX of the library: the kernel's argument block holds that many stacks)
MIX_Z_MOMENTS_MAX = 24
REDUCE_M0 = True   # A/B switch (module attribute): False = the moment m = 0 with all Stokes components of the model


class LinInputs:
    """The upload / prepare half of a linearized scene: the argument checks of rt_run(model, lin_model, NAer, NGas, NSurf), the
    derivative tables of lin_model in HBM (`upload`), the derivative layer optics of vsm_layer_optics_lin -- dtau_dot_all,
    varpi_dot, tau_sum_dot, fz, zdcoef -- with the component blocks Zall of every moment (`prepare`), and the Cox-Munk
    (rho, drho) pairs.  It owns nothing N x N per spectral point and no layer: SceneLin adds those for the full run, the
    single-scattering scene (core_rt_ss.SceneSSLin) does without them.  A subclass sets `self.fwd` (a CoreRT.Scene) between
    `_check_lin_args` and `_alloc_lin_optics`."""

    def _check_lin_args(self, model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int):
        land = LAND_BRDF.get(type(model.surface))
        if isinstance(model.surface, SPECTRAL_LAMBERTIAN):   # K albedo slots: treated like a K-parameter land surface below
            land = (None, H.surface_albedo_slots(model.surface))
            if land[1] < 2 and isinstance(model.surface, H.LambertianSurfaceLegendre):
                raise _lib.VSMError("rt_run (linearized): LambertianSurfaceLegendre needs at least two coefficients")
        if land is not None and NSurf != land[1]:
            raise _lib.VSMError("rt_run (linearized): %s has %d parameters (%s): NSurf = %d expected, got %r"
                                % (type(model.surface).__name__, land[1], ", ".join(surface_param_names(model.surface)), land[1],
                                   NSurf))
        if (NAer != lin_model.n_aer or NAer != len(model.aerosol_optics) or (land is None and NSurf != 1)
                or NGas != len(lin_model.tau_abs_dot)):
            raise _lib.VSMError("rt_run (linearized): NAer must equal the aerosols of model and lin_model, NGas = "
                                "len(lin_model.tau_abs_dot), NSurf = 1")
        if land is None and not isinstance(model.surface, (H.LambertianSurfaceScalar, H.CoxMunkSurface)):
            raise _lib.VSMError("rt_run (linearized): surface %r has no linearized builder here" % (model.surface,))
        self.nSurf = NSurf
        arch, FT = model.architecture, model.float_type
        CR._require_gpu(arch)
        self.model, self.lin_model, self.arch, self.FT = model, lin_model, arch, FT
        pol, qp = model.polarization_type, model.quad_points
        self.pol, self.qp = pol, qp
        self.layout = H.ParameterLayout(n_aerosols=NAer, n_gases=NGas, n_surface=NSurf)
        P, pl = self.layout.n_total, self.layout.n_layer_params
        self.P, self.pl, self.nAer, self.nGas = P, pl, NAer, NGas
        if P > 64:
            raise _lib.VSMError("rt_run (linearized): %d parameter slots (limit 64)" % P)

    def _alloc_lin_optics(self):
        fwd = self.fwd
        self.sl, self.S, self.N, self.dq, self.F0 = fwd.sl, fwd.S, fwd.N, fwd.dq, fwd.F0
        S, L, P, pl, NAer = self.S, fwd.Nz, self.P, self.pl, self.nAer
        dt, dev = CR._torch_dtype(self.FT), devi(self.arch)
        self.dt = dt
        self.C_, self.CT = 1 + NAer, 1 + NAer + 4 * NAer
        z = lambda *sh: torch.empty(sh, dtype=dt, device=dev)
        # layouts: the reference's column-major [nSpec, p] per layer -> tensors (L, p, S)
        self.dtau_dot_all, self.varpi_dot, self.tau_sum_dot = z(L, P, S), z(L, max(pl, 1), S), z(L + 1, max(pl, 1), S)
        self.fz = z(L, S, self.C_) if NAer else None
        self.zdcoef = z(L, S, pl, self.CT) if NAer else None
        self.Zall = None          # per moment ((CT, N, N), (CT, N, N)): component blocks of Z and of the Greek derivatives
        self.host_zdot = None     # host_optics: per moment and layer the materialised Z_dot

    # -- inputs -----------------------------------------------------------------------------------------------------------
    def upload(self):
        """H2D of what the linearization adds to Scene.upload(): lin_model.tau_abs_dot [nSpec, Nz, nGas] (FP64) and the
        aerosol derivative tables."""
        model, lin = self.model, self.lin_model
        conv = array_type(self.arch)
        S_full, L = model.tau_rayl.shape
        if getattr(self, "sub0", None) is not None:   # (a step re-uploads: the Stokes_IQ scene of m = 0 follows -- with the
            # parent's CURRENT model and lin_model: dataclasses.replace() is a shallow snapshot, so it is taken again here)
            self.sub0.model = self.sub0.fwd.model = self._sub0_model()
            self.sub0.lin_model = self.lin_model
            self.sub0.fwd.upload()
            self.sub0.upload()
        if self.nGas:
            g = np.stack([np.asarray(t, dtype=np.float64) for t in lin.tau_abs_dot])            # (nGas, S, L)
            if g.shape != (self.nGas, S_full, L):
                raise _lib.VSMError("lin_model.tau_abs_dot: %d arrays of [nSpec, Nz] = [%d, %d] expected" % (self.nGas, S_full, L))
            self.tau_abs_dot_d = conv(g).transpose(1, 2).contiguous()                           # (nGas, L, S)
        else:
            self.tau_abs_dot_d = None
        if self.nAer:
            tad = np.asarray(lin.tau_aer_dot, dtype=np.float64)                                 # [nAer, 7, L]
            if tad.shape != (self.nAer, 7, L):
                raise _lib.VSMError("lin_model.tau_aer_dot: [nAer, 7, Nz] expected")
            self.tau_aer_dot_d = conv(np.ascontiguousarray(tad.transpose(2, 0, 1)))             # (L, nAer, 7)
            self.ssa_dot_d = conv(np.ascontiguousarray(np.stack([np.asarray(l_.ssa_dot, dtype=np.float64)
                                                                  for l_ in lin.lin_aerosol_optics])))     # (nAer, 4)
            self.ftr_dot_d = conv(np.ascontiguousarray(np.stack([np.asarray(l_.f_trunc_dot, dtype=np.float64)
                                                                  for l_ in lin.lin_aerosol_optics])))
            self.greek_dot_dev = []
            for l_ in lin.lin_aerosol_optics:
                for g in l_.lin_greek_coefs:
                    tab = np.stack([np.asarray(getattr(g, k), dtype=np.float64) for k in
                                    ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")])
                    self.greek_dot_dev.append((conv(np.ascontiguousarray(tab)), tab.shape[1]))
        else:
            self.tau_aer_dot_d = self.ssa_dot_d = self.ftr_dot_d = None
            self.greek_dot_dev = []

    # -- device optics ----------------------------------------------------------------------------------------------------
    def prepare(self):
        model, fwd, dt = self.model, self.fwd, self.dt
        self._fold = {}   # (the folded per-layer inputs are copies of the optics)
        if getattr(self, "sub0", None) is not None:
            self.sub0.fwd.prepare()
            self.sub0.prepare()
        S_full, L = model.tau_rayl.shape
        _lib.call("vsm_layer_optics_lin", dt, S_full, fwd.lo, self.S, L, self.nAer, self.nGas, self.P, CR._ptr(fwd.tau_rayl_d),
                  CR._ptr(fwd.tau_abs_d), C.c_double(float(model.varpi_Cabannes)), CR._ptr(fwd.tau_aer_d), CR._ptr(fwd.ssa_d),
                  CR._ptr(fwd.ftr_d), CR._ptr(self.tau_abs_dot_d), CR._ptr(self.tau_aer_dot_d), CR._ptr(self.ssa_dot_d),
                  CR._ptr(self.ftr_dot_d), CR._ptr(self._ndoubl_table()), CR._ptr(self.dtau_dot_all), CR._ptr(self.varpi_dot),
                  CR._ptr(self.tau_sum_dot), CR._ptr(self.fz), CR._ptr(self.zdcoef), CR._stream_ptr())
        if self.nAer:
            q = self.dq.cstruct()
            N = self.N
            self.Zall = []
            for m in range(model.m_max + 1):
                Zp = torch.empty((self.CT, N, N), dtype=dt, device=devi(self.arch))
                Zm = torch.empty_like(Zp)
                for k, (gd, lmax) in enumerate(fwd.greek_dev + self.greek_dot_dev):
                    _lib.call("vsm_compute_Z_moments", dt, C.byref(q), m, lmax, CR._ptr(gd), CR._ptr(Zp[k]), CR._ptr(Zm[k]),
                              CR._stream_ptr())
                self.Zall.append((Zp, Zm))

    def _ndoubl_table(self):
        """The doubling numbers vsm_layer_optics_lin scales tau_dot by (device int[L])."""
        return self.fwd.nd_dev

    def _surface_tables(self):
        model = self.model
        self.surf = []
        # the albedo basis of a spectrally varying Lambertian surface, (K, S): formed on the FULL spectral axis and sliced like the
        # forward scene's albedo_d (a shard must not rebuild the Legendre abscissa on its own length)
        self.albedo_basis = None
        if isinstance(model.surface, SPECTRAL_LAMBERTIAN):
            basis = H.surface_albedo_basis(model.surface, model.tau_rayl.shape[0], self.FT)
            self.albedo_basis = array_type(self.arch)(np.ascontiguousarray(basis[:, self.sl].astype(self.FT)))
        if type(model.surface) in LAND_BRDF:       # all moments and parameters in one launch: (rho[m], drho[m][K])
            rho, drho = land_brdf_reflectance_lin(model.surface, self.dq, model.m_max, self.arch, self.FT)
            self.surf = [(rho[m], drho[m]) for m in range(model.m_max + 1)]
            return
        for m in range(model.m_max + 1):
            rho = drho = None
            if isinstance(model.surface, H.CoxMunkSurface):
                rho, drho = CR.reflectance(model.surface, self.dq, m, self.arch, self.FT, deriv=True)
            self.surf.append((rho, drho))

    def surface_layer_lin_(self, mom, added_s, als, F0, vectors_only=False):
        """create_surface_layer! (lin) of one Fourier moment into the surface layers `added_s` / `als`, driven by the beam F0.
        vectors_only: the spectral Lambertian builder's mode that leaves the matrices of shared layers unwritten."""
        model, dt, S, pl = self.model, self.dt, self.S, self.pl
        isurf = self.layout.surface_index(0)
        q_ = self.dq.cstruct()
        m = mom["m"]
        a_, al_ = added_s.cstruct(), als.cstruct()
        tau_sum_s, tsd_s = mom["tau_sum_surface"], self.tau_sum_dot[self.fwd.Nz]
        rho, drho = self.surf[m]
        if isinstance(model.surface, H.CoxMunkSurface):
            _lib.call("vsm_brdf_surface_lin", dt, C.byref(q_), S, m, CR._ptr(rho), CR._ptr(drho), isurf, CR._ptr(tau_sum_s),
                      CR._ptr(tsd_s), pl, CR._ptr(F0), C.byref(a_), C.byref(al_), CR._stream_ptr())
        elif type(model.surface) in LAND_BRDF:
            brdf_surface_lin_multi_(self.dq, S, m, rho, drho, isurf, tau_sum_s, tsd_s, pl, F0, added_s, als)
        elif isinstance(model.surface, SPECTRAL_LAMBERTIAN):   # (mom["rho"]: the forward scene's per-point albedo)
            lambertian_surface_spectral_lin_(self.dq, S, m, mom["rho"], self.albedo_basis, isurf, tau_sum_s, tsd_s, pl, F0, added_s, als,
                                             vectors_only=vectors_only)
        else:
            alb = C.c_double(model.surface.albedo) if dt == torch.float64 else C.c_float(model.surface.albedo)
            _lib.call("vsm_lambertian_surface_lin", dt, C.byref(q_), S, m, alb, isurf, CR._ptr(tau_sum_s), CR._ptr(tsd_s), pl,
                      CR._ptr(F0), C.byref(a_), C.byref(al_), CR._stream_ptr())


class SceneLin(LinInputs):
    """Everything rt_run(model, lin_model, NAer, NGas, NSurf) needs, resident in HBM (the linearized twin of CoreRT.Scene).
    The raw inputs -- tau_rayl, tau_abs, lin_model.tau_abs_dot [nSpec, Nz] and the small aerosol tables (tau_aer,
    tau_aer_dot, ssa / f_trunc and their Mie derivatives, Greek coefficients and their derivatives) -- are uploaded ONCE; the
    forward layer optics come from CoreRT.Scene's device pass (vsm_layer_optics, vsm_compute_Z_moments, vsm_layer_dtau) and
    their parameter derivatives from vsm_layer_optics_lin (tau_dot, varpi_dot, tau_sum_dot and the COEFFICIENTS of Z_dot over
    the component phase matrices: constructCoreOpticalProperties with lin_model, compEffectiveLayerProperties_lin.jl:43-197,
    types_lin.jl:196-380).  Z_dot[N, N, nSpec, P] is never materialised: elemental! (lin) forms it from the coefficients
    (vsm_elemental_lin_mix).  `run()` only launches kernels; exp(-dtau / mu0) is refreshed on the device per layer.

    `spec_slice` selects this rank's spectral shard; ndoubl and the tags always come from the FULL spectral axis
    (rt_kernel_lin.jl:87-95 uses batch-global maxima like the forward kernel).  `host_optics=True` builds the same inputs with
    the host mirror (host_model.constructCoreOpticalPropertiesLin, Z_dot materialised on the host) -- kept as a cross-check.

    Parameter slots (parameter_layout.jl:28-56): 7 per aerosol (tau_ref, n_r, n_i, r_m, sigma_r, p0, sigma_p; their optics
    derivatives are inputs: LinModel.tau_aer_dot / lin_aerosol_optics), the gases, then the surface slots -- ONE for the
    Lambertian albedo (lambertian_surface_lin.jl:48-162) or the Cox-Munk wind speed (coxmunk_surface_lin.jl:27-102); FOUR for
    rpvSurfaceScalar (rho0, rho_c, k, Theta) and THREE for RossLiSurfaceScalar (fvol, fgeo, fiso), whose derivatives are ours
    (LAND_BRDF, vsm_land_brdf_reflectance_lin / vsm_brdf_surface_lin_multi); K for the K coefficients of
    LambertianSurfaceLegendre or the K tables of LambertianSurfaceSpline.albedo_dot (one without them), also ours
    (vsm_lambertian_surface_spectral_lin on PER-POINT surface layers, forward and derivative).  With a ThermalEmission source the
    `:thermal` slot and its derivatives are added for m = 0 (_run_thermal, vsm_thermal_source_lin), and the nPlanck slots of
    ThermalEmission.B_layer_dot follow the surface slots in Rd / Td."""

    def __init__(self, model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int,
                 spec_slice: Optional[slice] = None, host_optics: bool = False, _reduce_m0: bool = True):
        self._check_lin_args(model, lin_model, NAer, NGas, NSurf)
        arch, FT = model.architecture, model.float_type
        # vsm_elemental_lin_mix forms Z_dot from at most 16 component blocks (1 + 5 NAer: VSM_LIN_CT_MAX of vsm_lin.hip), i.e. three
        # aerosols; the reference has no such limit, so beyond it the scene takes the host-optics path (Z_dot materialised per
        # layer and moment, vsm_elemental_lin) from the start instead of failing inside run()
        if 1 + 5 * NAer > 16:
            host_optics = True
        pol, qp = self.pol, self.qp
        P, pl = self.P, self.pl
        # Planck slots: ThermalEmission.B_layer_dot [nPlanck, rows, nSpec], appended after the surface slots
        th_src = [s_ for s_ in (model.sources or ()) if isinstance(s_, H.ThermalEmission)]
        Bd = getattr(th_src[0], "B_layer_dot", None) if th_src else None
        self.nPlanck = 0 if Bd is None else int(Bd.shape[0])
        # SIF slots: SurfaceSIF.SIF0_dot [nSIF, nStokes, nSpec], appended after the Planck slots
        sif_src = [s_ for s_ in (model.sources or ()) if isinstance(s_, H.SurfaceSIF)]
        self.nSIF = sif_src[0].nSIF if sif_src else 0
        # skin slots: SurfaceEmission.B_surface_dot [nSkin, nSpec], between the Planck and the SIF slots
        se_src = H.surface_emission_of(model)
        self.nSkin = se_src.nSkin if se_src is not None else 0
        if P + self.nPlanck + self.nSkin + self.nSIF > 64:
            if self.nSkin:
                raise _lib.VSMError("rt_run (linearized): %d parameter slots + %d Planck slots + %d skin slots + %d SIF slots "
                                    "(limit 64)" % (P, self.nPlanck, self.nSkin, self.nSIF))
            if self.nSIF:
                raise _lib.VSMError("rt_run (linearized): %d parameter slots + %d Planck slots + %d SIF slots (limit 64)"
                                    % (P, self.nPlanck, self.nSIF))
            raise _lib.VSMError("rt_run (linearized): %d parameter slots + %d Planck slots (limit 64)" % (P, self.nPlanck))
        sif_dot = sif_src[0].dot_tables(pol.n, model.tau_rayl.shape[0]) if self.nSIF else None
        if Bd is not None and Bd.shape[2] != model.tau_rayl.shape[0]:
            raise _lib.VSMError("ThermalEmission: B_layer_dot has %d spectral points, the model %d" % (Bd.shape[2], model.tau_rayl.shape[0]))
        # forward optics, quadrature, F0, composite / added / surface layers and R, T: the forward scene's device state
        # (rt_kernel_lin.jl:87 hard-codes scatter = true: a layer with tau*varpi <= 2 eps still goes through elemental! and
        # doubling! with ndoubl = 0 -- Scene.prepare gives such a layer ndoubl = 0 as well -- and only its interaction
        # follows the 00 / 01 / 10 tag of extractEffectiveProps)
        self.fwd = CR.Scene(model, spec_slice, host_optics=host_optics, full_added_layer=True)
        self.fwd.compute_hdrf = False
        fwd = self.fwd
        self._alloc_lin_optics()
        S, N = self.S, self.N
        dt, dev = self.dt, devi(arch)
        nV = len(model.vza)
        self.upload()
        if host_optics:
            self._prepare_host()
        else:
            self.prepare()
        self._surface_tables()
        self.added, self.added_s, self.comp = fwd.added, fwd.added_surface, fwd.composite
        self.al, self.als = AddedLayerLin(FT, arch, P, N, S), self._new_surface_added_lin()
        self.cl = CompositeLayerLin(FT, arch, P, N, S)
        self.expk = torch.empty(max(S, 1), dtype=dt, device=dev)
        self.R, self.T = fwd.R_SFI, fwd.T_SFI
        # the thermal slot: its layers are allocated on first use (_thermal_state); the Planck tables as (nPlanck, rows, S)
        self.thermal_B_dot = (array_type(arch)(np.ascontiguousarray(Bd[:, :, self.sl].astype(FT))) if self.nPlanck else None)
        self.surface_B_dot = (array_type(arch)(np.ascontiguousarray(se_src.B_surface_dot[:, self.sl].astype(FT))) if self.nSkin
                              else None)
        self._th = None
        self._check_thermal()
        # the SIF slots: 2 SIF0_dot as (nSIF, nStokes, S) and the Stokes components some table uses -- the right-hand sides of the
        # response solve (_sif_slots), chosen on the FULL spectral axis so that every shard solves the same ones.  Over a surface
        # that is not Lambertian the source does nothing (CoreRT.surface_source_contribute_) and the slots stay zero.
        self.sif_dot2, self._sif_comps = None, []
        if self.nSIF and isinstance(model.surface, CR.SIF_SURFACES):
            self._sif_comps = [c for c in range(pol.n) if np.any(sif_dot[:, c, :] != 0)]
            self.sif_dot2 = array_type(arch)(np.ascontiguousarray((2.0 * sif_dot[:, :, self.sl]).astype(FT)))
        self.Rd = torch.zeros((P + self.nPlanck + self.nSkin + self.nSIF, S, pol.n, nV), dtype=dt, device=dev)
        self.Td = torch.zeros_like(self.Rd)
        self._lanes = []
        self._fold = {}
        # The composite above the surface does not depend on a surface parameter: in the atmospheric layers the surface slots of
        # the added layer's AND of the composite's derivative stacks are zero, and the reference's loop over all Nparams
        # (interaction_lin.jl:242,291) computes exact zeros for them.  The layer interactions therefore run on the layer slots
        # [0, n_layer_params) only; the surface interaction on all of them.
        self._layer_slots = (0, pl) if 0 < pl < P else None
        # The Fourier moment m = 0 as a Stokes_IQ run (large batches; models without aerosol Jacobian slots over a Lambertian
        # surface).  At m = 0 no phase matrix couples (I,Q) with (U,V) (compute_Z_matrices.jl:26-110; the forward scene reads the
        # exact zeros off the device: `coupling`), the Lambertian surface (scalar or per-point albedo) reflects into I only, the gas and albedo derivatives
        # inherit the structure, and a beam without U / V components drives nothing in the (U,V) block: R, T, Rdot, Tdot of m = 0
        # are those of the same model carried with two Stokes components, U = V = 0.
        self.sub0 = None
        F0m = model.F0
        c0 = fwd.coupling[0] if getattr(fwd, "coupling", None) else None
        if (_reduce_m0 and REDUCE_M0 and pol.n >= 3 and S >= self.LANE_POINTS and NAer == 0 and not host_optics and c0 is not None
                and isinstance(model.surface, LAMBERTIAN) and (F0m is None or not np.any(np.asarray(F0m)[2:] != 0))
                and not any(s_.has_uv() for s_ in sif_src)   # (a surface emission with a U / V row drives the (U,V) block)
                and not any(c0 >> (4 * a + b) & 1 or c0 >> (4 * b + a) & 1 for a in (0, 1) for b in range(2, pol.n))):
            self.sub0 = SceneLin(self._sub0_model(), lin_model, NAer, NGas, NSurf, spec_slice, _reduce_m0=False)

    def _sub0_model(self):
        """The Stokes_IQ model of the moment m = 0, derived from the parent's model AS IT IS NOW (a step rebinds model.tau_abs,
        scene.lin_model, ... and re-uploads: the sub-scene must see the new arrays, not the constructor-time snapshot)."""
        model, qp = self.model, self.model.quad_points
        F0m = model.F0
        if model.sources is not None:   # (the sub-scene carries no thermal slot; without a SolarBeam its F0 stays 0; a SurfaceSIF
            # without U / V rows -- the constructor's condition -- comes along with its I, Q rows and its SIF slots)
            model = dataclasses.replace(model, sources=tuple(s_.stokes_iq() if isinstance(s_, H.SurfaceSIF) else s_
                                                             for s_ in model.sources
                                                             if not isinstance(s_, (H.ThermalEmission, H.SurfaceEmission))))
        qi = H.QuadPoints(qp.mu0, qp.imu0, qp.qp_mu, qp.wt_mu, np.repeat(qp.qp_mu, 2), np.repeat(qp.wt_mu, 2), qp.Nquad, qp.Nstreams)
        return dataclasses.replace(model, polarization_type=H.Stokes_IQ(), quad_points=qi, m_max=0,
                                   F0=None if F0m is None else np.ascontiguousarray(np.asarray(F0m)[:2]))

    def _prepare_host(self):
        """The same derivative inputs from the host mirror (numpy, Z_dot materialised per layer and moment)."""
        model, lin, FT, fwd = self.model, self.lin_model, self.FT, self.fwd
        S_full, L = model.tau_rayl.shape
        sl, pl = self.sl, self.pl
        conv = array_type(self.arch)
        self.host_zdot = []
        for m in range(model.m_max + 1):
            lods = H.constructCoreOpticalProperties(model, m)
            lins = H.constructCoreOpticalPropertiesLin(model, lin, lods, m)
            zd = []
            tsd = np.zeros((S_full, pl))
            for iz in range(L):
                if m == 0:
                    nd = fwd.moments[0]["layers"][iz]["nd"]
                    dall = np.zeros((S_full, self.P))
                    dall[:, :pl] = lins[iz].tau_dot / FT(2 ** nd)
                    self.dtau_dot_all[iz].copy_(to_device_sp(dall[sl], self.arch, FT))
                    if pl:
                        self.varpi_dot[iz].copy_(to_device_sp(lins[iz].varpi_dot[sl], self.arch, FT))
                        self.tau_sum_dot[iz].copy_(to_device_sp(tsd[sl], self.arch, FT))
                    tsd = tsd + lins[iz].tau_dot
                Zpd, Zmd = lins[iz].Zpp_dot, lins[iz].Zmp_dot
                if Zpd is not None and Zpd.ndim == 4:      # per-point Z_dot: this rank's spectral block
                    Zpd, Zmd = Zpd[:, sl], Zmd[:, sl]
                zpd, zs_, zp_ = to_device_zdot(Zpd, self.arch, FT)
                zmd, _, _ = to_device_zdot(Zmd, self.arch, FT)
                zd.append((zpd, zmd, (zs_, zp_)))
            if m == 0 and pl:
                self.tau_sum_dot[L].copy_(to_device_sp(tsd[sl], self.arch, FT))
            self.host_zdot.append(zd)

    # Small spectral batches are latency bound: a linearized layer step of ONE workgroup is ~0.4 ms and the 33 layers of a moment
    # are a dependent chain (C3: 2 points, 22 moments x 33 layers = 0.3 s moment by moment).  The Fourier moments are independent
    # until post-processing (rt_run_lin.jl:200-322), so below LANE_POINTS spectral points they run on up to LANES HIP streams, each
    # lane with its own added / composite layers (+ derivatives), work buffers and R / T / Rdot / Tdot accumulators, summed at the
    # end.  (The sum over moments is then taken lane by lane: equal to the sequential walk up to the rounding of the reordering.)
    LANES = 8
    LANE_POINTS = 64
    # A folded group of at most PARALLEL_LAYER_POINTS (moment, point) pairs doubles all its layers side by side on the lane streams
    # (each layer into an added layer of its own: 12 (1 + P) N^2 elements per pair and layer) before the interactions walk the
    # column (_run_folded)
    PARALLEL_LAYERS = True
    PARALLEL_LAYER_POINTS = 128
    MERGE_M0 = True          # the folded walk takes m = 0 and the moments m > 0 as one batch (False: two batches, two chains)
    TREE_INTERACTIONS = True  # the interactions of a pre-doubled column whose tags are all 11 as a tree over the lane streams

    def _lane_state(self, k):
        """Workspace of moment lane k (lane 0: the scene's own buffers); its `lane` entry picks the scratch buffers of its kernels."""
        while len(self._lanes) <= k:
            if not self._lanes:
                self._lanes.append(dict(added=self.added, al=self.al, comp=self.comp, cl=self.cl, added_s=self.added_s, als=self.als,
                                        expk=self.expk, R=self.R, T=self.T, Rd=self.Rd, Td=self.Td, stream=None, lane=0))
                continue
            FT, arch, P, N, S = self.FT, self.arch, self.P, self.N, self.S
            self._lanes.append(dict(
                added=CR.make_added_layer(FT, arch, (N, N), S), al=AddedLayerLin(FT, arch, P, N, S),
                comp=CR.make_composite_layer(FT, arch, (N, N), S), cl=CompositeLayerLin(FT, arch, P, N, S),
                added_s=self._new_surface_added(), als=self._new_surface_added_lin(),
                expk=torch.empty_like(self.expk), R=torch.zeros_like(self.R), T=torch.zeros_like(self.T),
                Rd=torch.zeros_like(self.Rd), Td=torch.zeros_like(self.Td), stream=torch.cuda.Stream(), lane=len(self._lanes)))
        return self._lanes[k]

    def _new_surface_added(self):
        a0 = self.added_s
        return CR.AddedLayer(self.FT, self.arch, self.N, self.S, a0.shared, a0.d_symmetric)

    def _new_surface_added_lin(self):
        """The derivative stacks of a surface layer: shared blocks or one per spectral point, as the forward surface layer has them
        (per point for the spectrally varying Lambertian surfaces: 4 P N^2 S elements instead of 4 P N^2)."""
        return AddedLayerLin(self.FT, self.arch, self.P, self.N, self.S, shared=self.added_s.shared)

    def run(self, lanes: Optional[int] = None, fold: Optional[bool] = None, graph: Optional[bool] = None):
        """The device-resident part of rt_run_lin.jl:200-322: Fourier loop -> layers -> surface -> post-processing.
        `lanes`: number of concurrent moment lanes (default: LANES for batches below LANE_POINTS points, else 1);
        `fold`: walk the layers with the Fourier moments folded into the spectral axis (_run_folded; default: for such small
        batches when the scene has no aerosol Jacobian slots);
        `graph`: replay the pass from a HIP graph (default: `self.graph_replay`, which a caller that steps the SAME scene many
        times -- a retrieval loop, the bench -- switches on; the first such call costs a warm-up pass and the capture).  A small
        batch is bound by the HOST: a pass of the C3 scene is ~ 2500 launches and library calls of ~ 15 us each, issued by one
        thread, so its two layer chains never overlap on the device (`tools/trace_timeline.py`: chain after chain, 14 ms each, with
        5 ms of launch-bound input folding in front of either).  The launch sequence depends only on the layer structure (ndoubl,
        interface tags, lanes / fold) -- the graph is captured once per such key, on buffers the scene owns, and reads the
        optics where `prepare()` puts them."""
        thermal = self._check_thermal()
        sif = self.fwd.sif is not None or self.nSIF > 0
        if graph is None:
            graph = (bool(getattr(self, "graph_replay", False)) and self.S > 0 and not torch.cuda.is_current_stream_capturing()
                     and not thermal and not sif)
        if graph and sif:
            raise NotImplementedError("SceneLin.run(graph=True): a scene with a SurfaceSIF source is not captured "
                                      "(run it with graph=False or graph=None)")
        if graph and thermal:
            raise NotImplementedError("SceneLin.run(graph=True): a scene with a ThermalEmission or SurfaceEmission source is not "
                                      "captured (run it with graph=False or graph=None)")
        if graph:
            return self._run_graph(lanes, fold)
        return self._run_eager(lanes, fold)

    def _check_thermal(self) -> bool:
        """Is there a thermal slot to run (a non-zero B_layer or Planck tables)?  Its scope limit is checked here, on host values,
        before anything is launched: every layer must scatter (the slot state the reference's forward run carries through
        non-scattering layers, CoreRT.ThermalSlot, has no linearized meaning)."""
        if not self.has_thermal:
            return False
        eps2 = 2 * np.finfo(self.FT).eps
        for iz, ly in enumerate(self.fwd.moments[0]["layers"]):
            if not ly["props"].max_tau_varpi > eps2:
                raise NotImplementedError("rt_run (linearized): layer %d does not scatter; a ThermalEmission or SurfaceEmission "
                                          "source needs a column whose layers all scatter" % (iz + 1))
        return True

    def _run_graph(self, lanes, fold):
        key = (lanes, fold, tuple((ly["nd"], ly["iface"]) for ly in self.fwd.moments[0]["layers"]), len(self.fwd.moments),
               self.fwd.moments[0]["iface_surface"])
        if getattr(self, "_graph_key", None) != key:
            self._graph = None
            # The library's scratch is keyed by (device, stream) and may not grow under a capture: the warm-up pass runs on the
            # very stream the capture uses (and on the same lane streams), so every buffer the captured launches need exists.
            if getattr(self, "_graph_stream", None) is None:
                self._graph_stream = torch.cuda.Stream()
            gs = self._graph_stream
            gs.wait_stream(torch.cuda.current_stream())
            self._fold = {}                       # (the folded per-layer inputs are copies of the optics: they must be formed
            with torch.cuda.stream(gs):           #  INSIDE the graph, not come out of the cache of an earlier pass)
                self._run_eager(lanes, fold)
            torch.cuda.synchronize()
            self._fold = {}
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=gs):
                self._run_eager(lanes, fold)
            self._graph, self._graph_key = g, key
        self._graph.replay()
        return self.R, self.T, self.Rd, self.Td

    def _run_eager(self, lanes: Optional[int] = None, fold: Optional[bool] = None):
        out = self._run_solar(lanes, fold)
        if self.S > 0 and self.has_thermal:
            self._run_thermal()
        return out

    def _run_solar(self, lanes: Optional[int] = None, fold: Optional[bool] = None):
        S = self.S
        nm = len(self.fwd.moments)
        small = 0 < S < self.LANE_POINTS
        if lanes is None:
            lanes = self.LANES if small else 1
        lanes = max(1, min(lanes, nm))
        can_fold = self.Zall is None and self.host_zdot is None and nm > 2 and S > 0
        if fold is None:
            fold = small and can_fold and lanes > 1
        if fold and not can_fold:
            raise _lib.VSMError("SceneLin.run(fold=True): needs a scene without aerosol Jacobian slots and more than two moments")
        st = [self._lane_state(k) for k in range(lanes)]
        torch._foreach_zero_([t for w in st for t in (w["R"], w["T"], w["Rd"], w["Td"])])
        if S == 0:
            return self.R, self.T, self.Rd, self.Td
        if fold:
            return self._run_folded(st)
        if lanes == 1:
            reduced = self.sub0 is not None
            if reduced:   # m = 0 first, like the Fourier loop: its I, Q rows are copied in, the later moments accumulate on top
                r0, t0, rd0, td0 = self.sub0.run(lanes=1, fold=False)
                self.R[:, :2, :].copy_(r0)
                self.T[:, :2, :].copy_(t0)
                self.Rd[:self.P, :, :2, :].copy_(rd0[:self.P])
                self.Td[:self.P, :, :2, :].copy_(td0[:self.P])
                if self.nSIF:      # (the sub-scene has no Planck or skin slot: its SIF slots follow its surface slots)
                    o = self.P + self.nSrc
                    self.Rd[o:, :, :2, :].copy_(rd0[self.P:])
                    self.Td[o:, :, :2, :].copy_(td0[self.P:])
            for mom in self.fwd.moments:
                if reduced and mom["m"] == 0:
                    continue
                self._run_moment(mom, st[0])
            return self.R, self.T, self.Rd, self.Td
        main = torch.cuda.current_stream()
        for w in st[1:]:
            w["stream"].wait_stream(main)       # (the zeroing above and whatever produced the inputs)
        for i, mom in enumerate(self.fwd.moments):
            k = i % lanes
            if k == 0:
                self._run_moment(mom, st[0])
            else:
                with torch.cuda.stream(st[k]["stream"]):
                    self._run_moment(mom, st[k])
        for w in st[1:]:
            main.wait_stream(w["stream"])
        for w in st[1:]:
            self.R += w["R"]
            self.T += w["T"]
            self.Rd += w["Rd"]
            self.Td += w["Td"]
        return self.R, self.T, self.Rd, self.Td

    # ---- moments folded into the spectral axis -------------------------------------------------------------------------------
    # The layer kernels are batched over the spectral axis with per-point dtau, varpi, Z (stride N^2) and derivatives; the Fourier
    # moment enters elemental! (lin) only through m == 0 (the weight factor 1/2 vs 1/4, elemental_lin.jl:77-206).  For a small
    # batch the moments m >= 1 therefore walk the layers as ONE batch of (moment, point) pairs -- and m = 0 as another --: two
    # dependent chains of layer steps instead of one per moment (C3: 22).  Each moment's block of the folded composite is then
    # copied to a lane and finished there (surface layer, its interaction, post-processing: these depend on m).
    def _fold_group(self, gi, group):
        """Workspace and per-layer inputs of a folded group (cached until the optics change)."""
        key = (gi, len(group))
        g = self._fold.get(key)
        if g is not None:
            return g
        FT, arch, P, N, S = self.FT, self.arch, self.P, self.N, self.S
        n = len(group)
        Sf = n * S
        g = dict(added=CR.make_added_layer(FT, arch, (N, N), Sf), al=AddedLayerLin(FT, arch, P, N, Sf),
                 comp=CR.make_composite_layer(FT, arch, (N, N), Sf), cl=CompositeLayerLin(FT, arch, P, N, Sf),
                 expk=torch.empty(Sf, dtype=self.dt, device=self.expk.device), F0=self.F0.repeat(n, 1).contiguous(), layers=[])
        # per-layer inputs of the folded walk: the optics of a layer do not depend on the moment (repeated along the folded axis, all
        # layers in one operation each), its phase matrices do (vsm_mix_Z_moments: every moment's Z of a layer in one launch)
        fwd = self.fwd
        lo, hi, L = fwd.lo, fwd.hi, fwd.Nz
        tau_f, varpi_f = fwd.tau[:L, lo:hi].repeat(1, n), fwd.varpi[:L, lo:hi].repeat(1, n)
        dtau_f, tsum_f = fwd.dtau[:L, lo:hi].repeat(1, n), fwd.tau_sum[:L, lo:hi].repeat(1, n)
        dtd_f, vd_f = self.dtau_dot_all.repeat(1, 1, n), self.varpi_dot.repeat(1, 1, n)
        tsd_f = self.tau_sum_dot.repeat(1, 1, n)
        Zf = torch.empty((2, L, Sf, N, N), dtype=self.dt, device=self.expk.device)
        for iz in range(L):
            props_m = [mom["layers"][iz]["props"] for mom in group]
            p0 = props_m[0]
            mixed = p0.fcomp is not None
            single = 0
            if not mixed:   # (one scatterer: the props hold the one-block views Zc[m][k : k + 1])
                single = int(fwd.zcomp[iz][1])
            # (at most MIX_Z_MOMENTS_MAX moments per launch: chunk i0 writes the blocks (im S + s) of moments i0 .. i0 + nc - 1)
            for i0 in range(0, n, MIX_Z_MOMENTS_MAX):
                chunk = group[i0:i0 + MIX_Z_MOMENTS_MAX]
                nc = len(chunk)
                zp = (C.c_void_p * nc)(*[fwd.Zc[mom["m"]][0].data_ptr() for mom in chunk])
                zm = (C.c_void_p * nc)(*[fwd.Zc[mom["m"]][1].data_ptr() for mom in chunk])
                _lib.call("vsm_mix_Z_moments", self.dt, N, S, int(p0.fcomp.shape[1]) if mixed else 0, nc, zp, zm, single,
                          CR._ptr(p0.fcomp) if mixed else None, CR._ptr(Zf[0, iz, i0 * S:]), CR._ptr(Zf[1, iz, i0 * S:]),
                          CR._stream_ptr())
            props = CR.DeviceLayerOptics(tau_f[iz], varpi_f[iz], Zf[0, iz], Zf[1, iz], p0.max_tau_varpi, p0.tau_h, p0.varpi_h)
            g["layers"].append(dict(props=props, dtau=dtau_f[iz], tau_sum=tsum_f[iz], dtd=dtd_f[iz], vd=vd_f[iz], tsd=tsd_f[iz]))
        if self.PARALLEL_LAYERS and 0 < Sf <= self.PARALLEL_LAYER_POINTS:
            g["per_layer"] = [dict(added=CR.make_added_layer(FT, arch, (N, N), Sf), al=AddedLayerLin(FT, arch, P, N, Sf),
                                   expk=torch.empty(Sf, dtype=self.dt, device=self.expk.device)) for _ in range(self.fwd.Nz)]
        self._fold[key] = g
        return g

    def _run_folded(self, st):
        pol, qp, dt, S, N, P, pl = self.pol, self.qp, self.dt, self.S, self.N, self.P, self.pl
        moms = self.fwd.moments
        groups = [[m_ for m_ in moms if m_["m"] == 0], [m_ for m_ in moms if m_["m"] > 0]]
        if self.MERGE_M0 and groups[0] and groups[1]:
            # ONE folded batch: the pairs of m = 0 in front (vsm_elemental_lin_fold tells them apart; doubling! and interaction!
            # do not know the moment) -- half the launches of the layer walk, one chain of interactions instead of two
            groups = [[], groups[0] + groups[1]]
        mu0 = C.c_double(qp.mu0) if dt == torch.float64 else C.c_float(qp.mu0)
        main = torch.cuda.current_stream()
        lanes = len(st)
        for w in st[1:]:
            w["stream"].wait_stream(main)       # (the zeroing of the accumulators and whatever produced the inputs)

        def double_layer(gi, group, iz, lane, added, al, expk):
            """elemental! (lin) + doubling! (lin) of layer iz of a folded group on the current stream (work buffers of `lane`)."""
            g = self._fold_group(gi, group)
            fl, ly0 = g["layers"][iz], group[0]["layers"][iz]
            n_m0 = S * sum(1 for m_ in group if m_["m"] == 0) if group[-1]["m"] > 0 else 0
            elemental_lin_(pol, fl["tau_sum"], fl["tsd"], fl["dtau"], fl["dtd"], g["F0"], fl["props"], fl["vd"], None, None, (0, 0),
                           pl, group[-1]["m"], ly0["nd"], self.dq, added, al, n_m0=n_m0)
            _lib.call("vsm_layer_expk", dt, len(group) * S, CR._ptr(fl["dtau"]), mu0, CR._ptr(expk), CR._stream_ptr())
            doubling_allparams_(pol, expk, ly0["nd"], added, al, fl["dtd"], qp.mu0, pl, lane=lane)

        # elemental! + doubling! of a layer depend on nothing but its own optics (rt_kernel_lin.jl:87-160: the added layer is built
        # before interaction! is called).  With so few (moment, point) pairs that one layer's launch fills a sixth of the chip, ALL
        # layers of both groups are doubled side by side on the lane streams, each into an added layer of its own, and only the
        # interactions -- the one sequential part of the adding method -- walk the column in order.  (Plain fork / join of the lane
        # streams from the main stream: what a HIP graph capture takes; layer streams forked from a lane stream crashed
        # hipStreamEndCapture.)
        gstate = [self._fold_group(gi, grp) if grp else None for gi, grp in enumerate(groups)]
        pre = lanes > 1 and all(g_ is None or g_.get("per_layer") is not None for g_ in gstate)
        if pre:
            cnt = 0
            for gi, grp in enumerate(groups):
                if not grp:
                    continue
                for iz in range(self.fwd.Nz):
                    k = 1 + cnt % (lanes - 1)
                    cnt += 1
                    b = gstate[gi]["per_layer"][iz]
                    with torch.cuda.stream(st[k]["stream"]):
                        double_layer(gi, grp, iz, k, b["added"], b["al"], b["expk"])
            for w in st[1:]:
                main.wait_stream(w["stream"])
            for w in st[1:]:
                w["stream"].wait_stream(main)

        def tree(gi, group):
            """The interactions of a pre-doubled column as a tree (every tag 11): pairs of neighbouring sub-columns are combined
            level by level -- composite (upper) (+) composite-as-added-layer (lower) -- on the lane streams, ceil(log2 Nz) dependent
            interactions instead of Nz - 1.  Same equations, another association: results agree with the chain to rounding."""
            g = gstate[gi]
            Sf = len(group) * S
            FT, arch = self.FT, self.arch
            pool = g.setdefault("tree_pool", [])
            used = 0
            nodes = [("leaf", iz) for iz in range(self.fwd.Nz)]
            while len(nodes) > 1:
                nxt = []
                for w in st[1:]:
                    w["stream"].wait_stream(main)
                for ip in range(len(nodes) // 2):
                    a, b = nodes[2 * ip], nodes[2 * ip + 1]
                    k = ip % lanes
                    ctx = torch.cuda.stream(st[k]["stream"]) if st[k]["stream"] is not None else contextlib.nullcontext()
                    with ctx:
                        if a[0] == "leaf":
                            if used == len(pool):
                                pool.append((CR.make_composite_layer(FT, arch, (N, N), Sf), CompositeLayerLin(FT, arch, P, N, Sf)))
                            comp, cl = pool[used]
                            used += 1
                            la = g["per_layer"][a[1]]
                            copy_added_to_composite_lin_(comp, cl, la["added"], la["al"])
                        else:
                            comp, cl = a[1], a[2]
                        if b[0] == "leaf":
                            added, al = g["per_layer"][b[1]]["added"], g["per_layer"][b[1]]["al"]
                        else:
                            added, al = _CompositeAsAdded(b[1]), _CompositeLinAsAdded(b[2])
                        interaction_lin_("11", comp, cl, added, al, p_range=self._layer_slots, lane=k)
                    nxt.append(("comp", comp, cl))
                if len(nodes) % 2:
                    nxt.append(nodes[-1])
                for w in st[1:]:
                    main.wait_stream(w["stream"])
                nodes = nxt
            return nodes[0][1], nodes[0][2]

        def chain(gi, group, lane):
            """The layer walk of a folded group on the current stream (work buffers of `lane`)."""
            g = gstate[gi]
            comp, cl = g["comp"], g["cl"]
            if (pre and self.TREE_INTERACTIONS and lane == 0 and self.fwd.Nz >= 4
                    and all(group[0]["layers"][iz]["iface"] == "11" for iz in range(1, self.fwd.Nz))):
                return tree(gi, group)
            for iz in range(self.fwd.Nz):
                ly0 = group[0]["layers"][iz]
                if pre:
                    added, al = g["per_layer"][iz]["added"], g["per_layer"][iz]["al"]
                else:
                    added, al = g["added"], g["al"]
                    double_layer(gi, group, iz, lane, added, al, g["expk"])
                if iz == 0:
                    copy_added_to_composite_lin_(comp, cl, added, al)
                else:
                    interaction_lin_(ly0["iface"], comp, cl, added, al, p_range=self._layer_slots, lane=lane)
            return comp, cl

        def finish(mom, w, comp, cl, im):
            """Moment `im` of a folded composite -> lane workspace `w`, then surface / interaction / post-processing there."""
            sl = slice(im * S, (im + 1) * S)
            fields = ("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m")
            torch._foreach_copy_([getattr(w["comp"], f) for f in fields] + [getattr(w["cl"], f) for f in fields],
                                 [getattr(comp, f)[sl] for f in fields] + [getattr(cl, f)[:, sl] for f in fields])   # (one multi-tensor launch)
            self._finish_moment(mom, w)

        # the m = 0 chain (and its finish) on lane 1's stream, concurrent with the m >= 1 chain on the main stream
        if groups[0]:
            if lanes > 1:
                with torch.cuda.stream(st[1]["stream"]):
                    comp0, cl0 = chain(0, groups[0], 1)
                    for im, mom in enumerate(groups[0]):
                        finish(mom, st[1], comp0, cl0, im)
            else:
                comp0, cl0 = chain(0, groups[0], 0)
                for im, mom in enumerate(groups[0]):
                    finish(mom, st[0], comp0, cl0, im)
        if groups[1]:
            comp1, cl1 = chain(1, groups[1], 0)
            for w in st[1:]:
                w["stream"].wait_stream(main)
            for im, mom in enumerate(groups[1]):
                kk = im % lanes
                if st[kk]["stream"] is None:
                    finish(mom, st[kk], comp1, cl1, im)
                else:
                    with torch.cuda.stream(st[kk]["stream"]):
                        finish(mom, st[kk], comp1, cl1, im)
        for w in st[1:]:
            main.wait_stream(w["stream"])
        for w in st[1:]:
            torch._foreach_add_([self.R, self.T, self.Rd, self.Td], [w["R"], w["T"], w["Rd"], w["Td"]])
        return self.R, self.T, self.Rd, self.Td

    def _run_moment(self, mom, w, after_layer=None):
        """One Fourier moment on the workspace `w` (launches on the current stream).  after_layer(l, comp, cl): called after layer l
        (1-based) has joined the composite (the multi-sensor run keeps its tops there)."""
        added, al, comp, cl = w["added"], w["al"], w["comp"], w["cl"]
        for iz, ly in enumerate(mom["layers"]):
            self._double_layer(mom, iz, w)
            if iz == 0:
                copy_added_to_composite_lin_(comp, cl, added, al)
            else:
                interaction_lin_(ly["iface"], comp, cl, added, al, p_range=self._layer_slots, lane=w["lane"])
            if after_layer is not None:
                after_layer(iz + 1, comp, cl)
        self._finish_moment(mom, w)

    def _elemental_layer(self, mom, iz, added, al, F0):
        """elemental! (lin) of layer iz (0-based) of one moment into added / al, driven by the beam F0 (the thermal slot's is zero:
        r, t and their derivatives as in the solar walk, j and jdot reset to zero)."""
        dt, fwd, S, pl, m = self.dt, self.fwd, self.S, self.pl, mom["m"]
        ly = mom["layers"][iz]
        props = ly["props"]
        dtd, vd, tsd = self.dtau_dot_all[iz], self.varpi_dot[iz], self.tau_sum_dot[iz]
        if self.Zall is not None:
            mixed, k = fwd.zcomp[iz]
            q_, a_, al_ = self.dq.cstruct(), added.cstruct(), al.cstruct()
            _lib.call("vsm_elemental_lin_mix", dt, C.byref(q_), S, m, ly["nd"], CR._ptr(ly["dtau"]), CR._ptr(props.varpi),
                      CR._ptr(ly["tau_sum"]), CR._ptr(F0), self.C_, self.CT, CR._ptr(self.Zall[m][0]),
                      CR._ptr(self.Zall[m][1]), -1 if mixed else k, CR._ptr(self.fz[iz]), pl, CR._ptr(dtd), CR._ptr(vd),
                      CR._ptr(tsd), CR._ptr(self.zdcoef[iz]), C.byref(a_), C.byref(al_), CR._stream_ptr())
        else:
            zpd, zmd, zds = self.host_zdot[m][iz] if self.host_zdot is not None else (None, None, (0, 0))
            elemental_lin_(self.pol, ly["tau_sum"], tsd, ly["dtau"], dtd, F0, props.materialize(), vd, zpd, zmd, zds, pl,
                           m, ly["nd"], self.dq, added, al)

    def _double_layer(self, mom, iz, w):
        """elemental! (lin) + doubling! (lin) of layer iz (0-based) of one moment into w["added"] / w["al"]."""
        qp, dt = self.qp, self.dt
        added, al = w["added"], w["al"]
        ly = mom["layers"][iz]
        self._elemental_layer(mom, iz, added, al, self.F0)
        mu0 = C.c_double(qp.mu0) if dt == torch.float64 else C.c_float(qp.mu0)
        _lib.call("vsm_layer_expk", dt, self.S, CR._ptr(ly["dtau"]), mu0, CR._ptr(w["expk"]), CR._stream_ptr())
        doubling_allparams_(self.pol, w["expk"], ly["nd"], added, al, self.dtau_dot_all[iz], qp.mu0, self.pl, lane=w["lane"])

    def _finish_moment(self, mom, w):
        """Surface layer, its interaction and the post-processing of one Fourier moment on the workspace `w`."""
        model = self.model
        comp, cl = w["comp"], w["cl"]
        m = mom["m"]
        weight = float(CR.fourier_weight(self.FT, m))
        self._surface_lin(mom, w["added_s"], w["als"], self.F0)
        if m == 0 and self._sif_comps:
            self._sif_slots(comp, w, weight)     # (reads the composite BEFORE its surface interaction)
        interaction_lin_(mom["iface_surface"], comp, cl, w["added_s"], w["als"], lane=w["lane"])
        postprocessing_vza_lin_(self.pol, comp, cl, model.vza, model.vaz, self.qp, m, weight, w["R"], w["T"], w["Rd"], w["Td"])

    def _sif_slots(self, comp, w, weight):
        """The SIF slots.  The radiance is linear in SIF0 and the emission is the same at every stream, so
        dR / dx_k = sum_c 2 SIF0_dot[k, c, s] G_c(s) with G_c the response of the column to a unit emission in Stokes component c:
        ONE elimination per point for the components some table uses (MS.surface_emission_response_), combined here into the slots
        P + nPlanck + k of the workspace's Rdot / Tdot.  Like the Planck slots they are forward quantities: no derivative stack and
        no layer kernel knows of them."""
        model, pol = self.model, self.pol
        comps, K, nV = self._sif_comps, len(self._sif_comps), len(model.vza)
        if w.get("sif_up") is None:
            w["sif_up"] = torch.empty((K, self.S, pol.n, nV), dtype=self.dt, device=self.expk.device)
            w["sif_dn"] = torch.empty_like(w["sif_up"])
        up, dn = w["sif_up"], w["sif_dn"]
        MS.surface_emission_response_(pol, self.qp, model.vza, model.vaz, weight, comp.R_pm, comp.T_mm, w["added_s"].r_mp, comps,
                                      up, dn)
        coef = self.sif_dot2[:, comps, :]                       # (nSIF, K, S)
        o = self.P + self.nSrc
        w["Rd"][o:o + self.nSIF].add_(torch.einsum("kis,iscv->kscv", coef, up))
        w["Td"][o:o + self.nSIF].add_(torch.einsum("kis,iscv->kscv", coef, dn))

    def _surface_lin(self, mom, added_s, als, F0):
        """The linearized surface layer (surface_layer_lin_); at m = 0 SurfaceSIF is then injected into the forward j0-
        (rt_run_lin.jl:292; it depends on no parameter, so the derivative stacks stay what the builder wrote -- and the builder
        has formed its -tau_sum_dot / mu0 terms from the beam term alone)."""
        self.surface_layer_lin_(mom, added_s, als, F0)
        CR.surface_source_contribute_(self.fwd, self.model.surface, added_s, mom["m"])

    # ---- the thermal slot ----------------------------------------------------------------------------------------
    def _thermal_state(self):
        """The slot's own layers, forward and derivative (allocated on first use), its zero beam, its expk = 1 and the zero
        dtau_dot table that makes doubling! (lin) form ekl = 0.  The slot runs on the main stream: lane 0."""
        if self._th is None:
            FT, arch, P, N, S = self.FT, self.arch, self.P, self.N, self.S
            dev = self.expk.device
            self._th = dict(added=CR.make_added_layer(FT, arch, (N, N), S), al=AddedLayerLin(FT, arch, P, N, S),
                            comp=CR.make_composite_layer(FT, arch, (N, N), S), cl=CompositeLayerLin(FT, arch, P, N, S),
                            added_s=self._new_surface_added(), als=self._new_surface_added_lin(),
                            F0=torch.zeros_like(self.F0), ones=torch.empty(max(S, 1), dtype=self.dt, device=dev),
                            zero_dtd=torch.zeros((P, max(S, 1)), dtype=self.dt, device=dev), lane=0)
        return self._th

    def _run_thermal(self):
        """The `:thermal` per-source slot of the linearized run, on the current stream after the solar moments (whatever lanes
        they ran on have joined it): ThermalSlot step by step with the derivative stacks beside it, m = 0 only (the
        source is isotropic), into the same R, T, Rdot, Tdot; then the Planck block."""
        fwd = self.fwd
        mom = fwd.moments[0]
        if fwd.thermal_B is not None:
            self._thermal_lin_slot(mom)
        if self.nSrc:
            self._planck_block(mom)

    @property
    def nSrc(self) -> int:
        """The source-only slots of the thermal slot: nPlanck Planck tables, then nSkin skin tables."""
        return self.nPlanck + self.nSkin

    @property
    def has_thermal(self) -> bool:
        """Does this scene run a `:thermal` slot: a forward emission (a non-zero B_layer or B_surface) or a source-only slot?  The
        one rule of every linearized driver -- a source that states neither (an all-zero SurfaceEmission, say) runs nothing."""
        return self.fwd.thermal_B is not None or self.nSrc > 0

    def source_tables(self):
        """Per source-only slot the pair (B, B_surface) its forward slot runs on: (B_layer_dot[k], None) for the Planck tables, then
        (a Planck table of 0 rows, B_surface_dot[k]) for the skin tables."""
        none = torch.empty((0, self.S), dtype=self.dt, device=self.expk.device)
        return ([(self.thermal_B_dot[k], None) for k in range(self.nPlanck)]
                + [(none, self.surface_B_dot[k]) for k in range(self.nSkin)])

    def _thermal_lin_walk(self, mom, comp, cl, first, end, B, after_layer=None):
        """Layers first+1 .. end (1-based) of the linearized slot for the Planck table B ((rows, S), or None) into the thermal
        composite `comp` / `cl`, the first one a copy (the linearized twin of ThermalSlot.walk: expk = 1 and no beam attenuation,
        so a range that starts below the TOA needs no absolute tau_sum).  after_layer(l, comp, cl): called once layer l is in the
        composite (the multi-sensor run keeps its thermal tops there, core_rt_ms_lin.py)."""
        dt, S, pl = self.dt, self.S, self.pl
        t = self._thermal_state()
        added, al = t["added"], t["al"]
        rows = B.shape[0] if B is not None else 0
        for iz in range(first, end):
            ly = mom["layers"][iz]
            self._elemental_layer(mom, iz, added, al, t["F0"])
            if iz < rows:      # contribute! and its derivatives
                q_, a_, al_ = self.dq.cstruct(), added.cstruct(), al.cstruct()
                _lib.call("vsm_thermal_source_lin", dt, C.byref(q_), S, CR._ptr(ly["dtau"]), CR._ptr(ly["props"].varpi),
                          CR._ptr(B[iz]), pl, CR._ptr(self.dtau_dot_all[iz]), CR._ptr(self.varpi_dot[iz]), C.byref(a_),
                          C.byref(al_), CR._stream_ptr())
            t["ones"].fill_(1.0)    # the slot's expk = 1 (the doubling kernels square it in place); zero_dtd: ekl = 0
            doubling_allparams_(self.pol, t["ones"], ly["nd"], added, al, t["zero_dtd"], self.qp.mu0, pl, lane=t["lane"])
            if iz == first:
                copy_added_to_composite_lin_(comp, cl, added, al)
            else:
                interaction_lin_(ly["iface"], comp, cl, added, al, p_range=self._layer_slots, lane=t["lane"])
            if after_layer is not None:
                after_layer(iz + 1, comp, cl)

    def _thermal_lin_surface(self, mom):
        """The slot's surface layers: those of the solar walk without their beam terms (what _surface_lin injected for SurfaceSIF
        is zeroed with the beam term: that emission counts once, in the solar slot), then the scene's SurfaceEmission: the forward
        emission in j0- and, in Kirchhoff mode, its derivative in the surface slots of ap_J0- (vsm_surface_emission_lin; the layer
        slots need nothing here, the linearized interaction differentiates the propagation of the forward j0-).  DESIGN 4.18."""
        t = self._thermal_state()
        fwd, added_s, als = self.fwd, t["added_s"], t["als"]
        self._surface_lin(mom, added_s, als, t["F0"])
        torch._foreach_zero_([added_s.j0_p, added_s.j0_m, als.ap_J0_p, als.ap_J0_m])
        if (CR.surface_emission_contribute_(fwd.surface_B, fwd.surface_emissivity, added_s, self.pol.n, mom["m"])
                and fwd.surface_emissivity is None):
            isurf = self.layout.surface_index(0)
            al_ = als.cstruct()
            _lib.call("vsm_surface_emission_lin", self.dt, self.N, self.pol.n, self.S, mom["m"], CR._ptr(fwd.surface_B), isurf,
                      self.P - isurf, C.byref(al_), CR._stream_ptr())
        return added_s, als

    def _thermal_lin_slot(self, mom, after_layer=None, post=True):
        """Walk layers 1 .. Nz (_thermal_lin_walk), surface, post-process into R, T, Rdot, Tdot (post=False: the composite is left
        after its surface interaction and nothing is added to the outputs)."""
        model = self.model
        t = self._thermal_state()
        comp, cl = t["comp"], t["cl"]
        self._thermal_lin_walk(mom, comp, cl, 0, len(mom["layers"]), self.fwd.thermal_B, after_layer)
        added_s, als = self._thermal_lin_surface(mom)
        interaction_lin_(mom["iface_surface"], comp, cl, added_s, als, lane=t["lane"])
        if post:
            postprocessing_vza_lin_(self.pol, comp, cl, model.vza, model.vaz, self.qp, mom["m"], float(CR.fourier_weight(self.FT, 0)),
                                    self.R, self.T, self.Rd, self.Td)

    def _planck_block(self, mom):
        """The slot is linear in B and in B_surface: dR / dx_k is the FORWARD thermal slot (CoreRT.ThermalSlot, fused layer kernels
        included) of B := B_layer_dot[k] over a boundary that does not emit, or, for a skin table, of an empty Planck table over
        B_surface := B_surface_dot[k] (source_tables), post-processed into slot P + k of Rdot / Tdot."""
        fwd, P = self.fwd, self.P
        weight = float(CR.fourier_weight(self.FT, 0))
        th = fwd.thermal_slot()
        for k, (B, B_surface) in enumerate(self.source_tables()):
            th.begin(mom)
            th.walk(mom, th.comp, 0, fwd.Nz, B)
            th.surface(mom, B_surface)
            th.finish(mom, weight, self.Rd[P + k], self.Td[P + k])

    def results_host(self):
        """(R, T, Rdot, Tdot) as the reference returns them: [nVZA, nStokes, nSpec] and [nVZA, nStokes, nSpec, Nparams]."""
        tr = lambda t: to_host(t).transpose(2, 1, 0).copy()
        tr4 = lambda t: to_host(t).transpose(3, 2, 1, 0).copy()
        return tr(self.R), tr(self.T), tr4(self.Rd), tr4(self.Td)

    def flops_per_point(self) -> float:
        """ALGORITHMIC flops per spectral point: forward + per parameter nd (24N^3+16N^2) per layer for
        the layer parameters and (48N^3+16N^2) per interaction for every parameter."""
        N = float(self.N)
        tot = 0.0
        for mom in self.fwd.moments:
            for iz, ly in enumerate(mom["layers"]):
                tot += ly["nd"] * ((12 + 24 * self.pl) * N ** 3 + (8 + 16 * self.pl) * N ** 2)
                if iz > 0:
                    tot += (24 + 48 * self.P) * N ** 3 + (8 + 16 * self.P) * N ** 2
            tot += (24 + 48 * self.P) * N ** 3 + (8 + 16 * self.P) * N ** 2
        return tot


def prepare_scene_lin(model, lin_model, NAer, NGas, NSurf, spec_slice: Optional[slice] = None) -> SceneLin:
    return SceneLin(model, lin_model, NAer, NGas, NSurf, spec_slice)


def rt_run_lin(model: H.RTModel, lin_model: H.LinModel, NAer: int, NGas: int, NSurf: int):
    """rt_run(model, lin_model, NAer, NGas, NSurf) (rt_run_lin.jl:72-78 -> :102-326) -> (R, T, Rdot, Tdot);
    Rdot/Tdot: [nVZA, nStokes, nSpec, Nparams].  Supported: NAer = number of aerosols of the model (7 slots each, optics
    derivatives supplied in lin_model), NGas = len(lin_model.tau_abs_dot), NSurf = 1
    (Lambertian albedo or Cox-Munk wind speed, by the model's surface), NSurf = 4 for rpvSurfaceScalar (rho0, rho_c, k, Theta)
    or NSurf = 3 for RossLiSurfaceScalar (fvol, fgeo, fiso), NSurf = K for LambertianSurfaceLegendre with K coefficients (slot k =
    d / d legendre_coeff[k]) and for LambertianSurfaceSpline with albedo_dot [K, nSpec] (slot k = d / d x_k, albedo_dot[k] =
    d albedo / d x_k on the band grid; without albedo_dot NSurf = 1, a table of ones); the surface slots come last.  Like the
    reference's linearized driver this path applies no TMS correction.

    Sources: model.sources may hold SolarBeam and / or ThermalEmission, as CoreRT.rt_run takes them (without a SolarBeam F0 = 0).
    R, T then include the thermal radiance and every slot of Rdot / Tdot the derivative of the thermal slot (m = 0
    only, no surface emission).  ThermalEmission(B_layer_dot=[nPlanck, rows, nSpec]) appends nPlanck Planck (temperature) slots
    after the surface slots: Nparams = 7 NAer + NGas + NSurf + nPlanck <= 64, slot k of the block = d/dx_k for B_layer_dot[k] =
    dB_layer / dx_k.  Not supported with a thermal source: a column with a non-scattering layer (NotImplementedError).

    SurfaceEmission(B_surface=..., B_surface_dot=...): the emission of the thermal slot's lower boundary, with or without
    a ThermalEmission; in Kirchhoff mode the surface slots carry the derivative of the emissivity.  B_surface_dot [nSkin, nSpec]
    appends nSkin skin slots after the Planck slots (slot k = d/dx_k for B_surface_dot[k] = dB_surface / dx_k) and before the SIF
    slots: Nparams | nPlanck | nSkin | nSIF, at most 64 in all.

    SurfaceSIF(SIF0, SIF0_dot): R, T and every slot carry the emission's share (m = 0, Lambertian surface);
    SIF0_dot [nSIF, nStokes, nSpec] appends nSIF slots after the Planck slots, slot k of the block = d/dx_k for SIF0_dot[k] =
    dSIF0 / dx_k; 7 NAer + NGas + NSurf + nPlanck + nSIF <= 64."""
    scene = SceneLin(model, lin_model, NAer, NGas, NSurf)
    scene.run()
    synchronize_if_gpu()
    _lib.check_device_status("rt_run (linearized)")
    return scene.results_host()
