"""Exact single scattering: the reference's StandaloneSS module (src/StandaloneSS) on the MI355X, through vsm_exact_ss_*
(vsmartmom.jl_amd/csrc/vsm_exact_ss.hip).

run_exact_ss evaluates the phase matrix at the true scattering angle of every viewing geometry -- no Fourier series, no l_trunc --
and splits the first-order field into four paths: (1) one scattering in the atmosphere, (2) the direct beam reflected by the
surface, (3) atmosphere -> surface -> sensor, (4) surface -> atmosphere -> sensor.  apply_back_correction adds
exact(path 1 + 2) - truncated(path 1 + 2) to a radiance array: the post-hoc correction of a low-order run.

The host computes only small, spectrally flat tables per contributor (solver.jl:143-197, Scattering.phase_matrix_first_column):
p_c[C][nGeom][nStokes] and the azimuthal averages pbar_c[C][nGeom][nQuad].  The contributors' optical depths go to the device as
they are; the kernels mix them per (layer, point), so the reference's P_eff[nGeom, nStokes, nLayer, nSpec] and
Pbar[nGeom, nLayer, nSpec, nQuad] arrays are never allocated.

Units.  Path 1 carries 1 / (4 pi) and path 2 albedo / pi explicitly; CoreRT carries the same factors in the Fourier weights
0.5 / pi, 1 / pi of postprocessing_vza!.  At I0 = 1 (what exact_ss_config_from_model sets) CoreRT.rt_run_ss's R equals
path 1 + path 2 with constant 1 in every Stokes row (tests/test_oracle_exact_ss.py), so the back-correction
adds straight onto an rt_run radiance computed with F0 = e1.  I0 passes through for any other solar scaling; nothing is rescaled.

Sources.  Every path here is SOLAR single scattering: model.sources is not read.  A ThermalEmission, SurfaceSIF or SurfaceEmission source of the model
is ignored on purpose -- the emission is no part of the first-order solar field, and the back-correction of a thermal or SIF run
(exact - truncated solar single scattering, added onto that run's radiance) is legitimate.

Not built: the measurement selector, the determine_required_* diagnostics, the chain-rule helpers, the ForwardDiff path, vector
Stokes paths 3 and 4 (the reference has none), a per-point n_water table.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, replace
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import host_model as H
from . import core_rt as CR
from .architectures import GPU, array_type, default_architecture, synchronize_if_gpu, to_host

SUPPORTED_PATHS = ("path1", "path2", "path3", "path4", "paths_1_2", "all", "all_four")
_WANTS = {1: ("path1", "paths_1_2", "all", "all_four"), 2: ("path2", "paths_1_2", "all", "all_four"),
          3: ("path3", "all", "all_four"), 4: ("path4", "all", "all_four")}


def _wants(paths, i):
    return paths in _WANTS[i]


# ---- types.jl ------------------------------------------------------------------------------------------------------------
@dataclass
class SSGeometry:
    """mu0: the positive solar cosine; mu_v: positive upward viewing cosines; dphi: view-sun relative azimuths [rad]."""
    mu0: float
    mu_v: Sequence[float]
    dphi: Sequence[float]


@dataclass
class LambertianSSSurface:
    albedo: object                        # scalar or [nSpec]


@dataclass
class CoxMunkSSSurface:
    wind_speed: float
    n_water: Optional[complex] = None     # scalar; None = 1.34 + 0i (surfaces.jl:222)
    whitecap_albedo: float = 0.22
    include_whitecaps: bool = True
    shadowing: bool = True


@dataclass
class RayleighSSContributor:
    tau: np.ndarray                       # (nLayer, nSpec)
    depol: float = 0.0


@dataclass
class HGAerosolSSContributor:
    g: float
    varpi: float
    tau: np.ndarray


@dataclass
class GreekCoefsSSContributor:
    greek_coefs: H.GreekCoefs
    varpi: float
    tau: np.ndarray


@dataclass
class AbsorptionSSContributor:
    tau: np.ndarray


@dataclass
class ExactSSConfig:
    geometry: SSGeometry
    surface: object
    contributors: Sequence
    I0: object                            # scalar or [nSpec]
    n_stokes: int = 1
    polarization_type: Optional[H.PolarizationType] = None     # when given it sets the Stokes count
    inner_nquad: int = 16
    azimuth_nquad: int = 64
    architecture: object = None           # None = default_architecture()
    float_type: type = np.float64


class ExactSSResult(NamedTuple):
    total: np.ndarray
    path1: np.ndarray
    path2: np.ndarray
    path3: np.ndarray
    path4: np.ndarray
    quadrature_info: dict
    metadata: dict


def single_scattering_albedo(c) -> float:
    if isinstance(c, RayleighSSContributor):
        return 1.0
    if isinstance(c, AbsorptionSSContributor):
        return 0.0
    return float(c.varpi)


def _n_stokes(cfg) -> int:
    return int(cfg.n_stokes) if cfg.polarization_type is None else int(cfg.polarization_type.n)


def _depol_scale(depol):
    return (1 - depol) / (1 + depol / 2)


# ---- Scattering: reconstruct_phase at one angle, the rotation into the meridian plane ----------------------------------------
def _legendre_p0_p2(x: float, nmax: int):
    """compute_legendre_poly (legendre_functions.jl:223-265) at one x: P0[l], P2[l], l < nmax."""
    if nmax <= 1:
        raise ValueError("Greek coefficients need at least two moments")
    P0, P2 = np.zeros(nmax), np.zeros(nmax)
    P0[0], P0[1] = 1.0, x
    if nmax > 2:
        P2[2] = 3 * (1 - x * x)
    for n in range(2, nmax):
        l = n - 1
        P0[n] = ((2 * l + 1) * x * P0[n - 1] - l * P0[n - 2]) / (l + 1)
        if n > 2:
            P2[n] = ((2 * l + 1) * x * P2[n - 1] - (l + 2) * P2[n - 2]) / (l - 1)
    return P0, P2


def reconstruct_phase(greek: H.GreekCoefs, x: float):
    """(f11, f12) of reconstruct_phase (mie_helper_functions.jl:415-446) at cos(Theta) = x."""
    lmax = len(greek.alpha)
    P0, P2 = _legendre_p0_p2(float(x), lmax)
    fac = np.zeros(lmax)
    for l in range(2, lmax):
        fac[l] = math.sqrt(1.0 / ((l - 1) * l * (l + 1) * (l + 2)))
    return float(P0 @ np.asarray(greek.beta, dtype=np.float64)), float(P2 @ (fac * np.asarray(greek.gamma, dtype=np.float64)))


def scattering_angle_cosine(mu0, mu_v, dphi):
    return -mu0 * mu_v + math.sqrt(max(0.0, 1 - mu0 * mu0)) * math.sqrt(max(0.0, 1 - mu_v * mu_v)) * math.cos(dphi)


def phase_matrix_first_column(greek: H.GreekCoefs, mu0, mu_v, dphi, n: int):
    """Scattering.phase_matrix_first_column (analytic_phase_functions.jl:165-208)."""
    cosT = scattering_angle_cosine(mu0, mu_v, dphi)
    f11, f12 = reconstruct_phase(greek, cosT)
    sin2 = max(0.0, 1 - cosT * cosT)
    if sin2 <= np.finfo(np.float64).eps:
        c2, s2 = 1.0, 0.0
    else:
        sinT = math.sqrt(sin2)
        s0, sv = math.sqrt(max(0.0, 1 - mu0 * mu0)), math.sqrt(max(0.0, 1 - mu_v * mu_v))
        cchi = (mu0 * sv + mu_v * s0 * math.cos(dphi)) / sinT
        schi = s0 * math.sin(dphi) / sinT
        c2, s2 = cchi * cchi - schi * schi, 2 * schi * cchi
    return [f11, f12 * c2, f12 * s2, 0.0][:n]


def exact_phase_function(c, cosT) -> float:
    """types.jl:150-171."""
    if isinstance(c, RayleighSSContributor):
        return 1 + 0.5 * _depol_scale(c.depol) * (3 * cosT * cosT - 1) / 2
    if isinstance(c, HGAerosolSSContributor):
        return (1 - c.g ** 2) / (1 + c.g ** 2 - 2 * c.g * cosT) ** 1.5
    if isinstance(c, GreekCoefsSSContributor):
        return reconstruct_phase(c.greek_coefs, cosT)[0]
    return 0.0


def azimuthal_average_phase(c, mu_a, mu_b, n_phi: int) -> float:
    """_azimuthal_average_phase (solver.jl:143-167): analytic for Rayleigh, an n_phi-point mean otherwise."""
    a = mu_a * mu_b
    b = math.sqrt(max(0.0, 1 - mu_a * mu_a)) * math.sqrt(max(0.0, 1 - mu_b * mu_b))
    if isinstance(c, RayleighSSContributor):
        return 1 + 0.5 * _depol_scale(c.depol) * (3 * (a * a + 0.5 * b * b) - 1) / 2
    total = 0.0
    for k in range(n_phi):
        total += exact_phase_function(c, min(max(a + b * math.cos(2 * math.pi * k / n_phi), -1.0), 1.0))
    return total / n_phi


def gauss_legendre_01(n: int):
    if n <= 0:
        raise ValueError("inner_nquad must be positive")
    x, w = np.polynomial.legendre.leggauss(n)
    return (x + 1) / 2, w / 2


def phase_table(cfg, n: int) -> np.ndarray:
    """p_c[C][nGeom][n]: scalar runs take exact_phase_function at cos(Theta) (solver.jl:199-252), vector runs the first column of
    the phase matrix (:254-317)."""
    g = cfg.geometry
    tab = np.zeros((len(cfg.contributors), len(g.mu_v), n))
    for ic, c in enumerate(cfg.contributors):
        if isinstance(c, AbsorptionSSContributor):
            continue
        for iv, (mv, dp) in enumerate(zip(g.mu_v, g.dphi)):
            if n == 1:
                tab[ic, iv, 0] = exact_phase_function(c, scattering_angle_cosine(float(g.mu0), float(mv), float(dp)))
            else:
                greek = H.get_greek_rayleigh(c.depol) if isinstance(c, RayleighSSContributor) else c.greek_coefs
                tab[ic, iv] = phase_matrix_first_column(greek, float(g.mu0), float(mv), float(dp), n)
    return tab


def pbar_table(cfg, mu_nodes, reference_mu) -> np.ndarray:
    """pbar_c[C][nGeom][nQuad]: the azimuthal average of contributor c between inner node k and reference_mu[iv]."""
    tab = np.zeros((len(cfg.contributors), len(reference_mu), len(mu_nodes)))
    for ic, c in enumerate(cfg.contributors):
        if single_scattering_albedo(c) == 0:
            continue
        cache = {}
        for iv, mr in enumerate(reference_mu):
            if float(mr) not in cache:
                cache[float(mr)] = [azimuthal_average_phase(c, float(mk), float(mr), cfg.azimuth_nquad) for mk in mu_nodes]
            tab[ic, iv] = cache[float(mr)]
    return tab


# ---- validation (solver.jl:86-105, 483-505) ---------------------------------------------------------------------------------
def _dims(contributors):
    if len(contributors) == 0:
        raise ValueError("ExactSSConfig requires at least one contributor")
    shp = np.shape(contributors[0].tau)
    if len(shp) != 2:
        raise ValueError("contributor optical depths must be matrices with shape (nLayer, nSpec)")
    for c in contributors:
        if np.shape(c.tau) != shp:
            raise ValueError("all contributor optical-depth matrices must have the same shape")
    return shp


def _validate_vector_path1(contributors):
    for c in contributors:
        if not isinstance(c, (RayleighSSContributor, GreekCoefsSSContributor, AbsorptionSSContributor)):
            raise ValueError("StandaloneSS vector path1 supports RayleighSSContributor, GreekCoefsSSContributor and "
                             "AbsorptionSSContributor only; got %s" % type(c).__name__)


def _validate_config(cfg, paths):
    if paths not in SUPPORTED_PATHS:
        raise ValueError("StandaloneSS supports paths %s; got %r" % (", ".join(SUPPORTED_PATHS), paths))
    n = _n_stokes(cfg)
    if not 1 <= n <= 4:
        raise ValueError("n_stokes must be 1..4")
    if n != 1 and paths not in ("path1", "path2", "paths_1_2"):
        raise ValueError("StandaloneSS vector Stokes kernels support only paths 'path1', 'path2' and 'paths_1_2'; received "
                         "n_stokes=%d and paths=%r" % (n, paths))
    if n != 1 and _wants(paths, 1):
        _validate_vector_path1(cfg.contributors)
    if (_wants(paths, 3) or _wants(paths, 4)) and not isinstance(cfg.surface, LambertianSSSurface):
        raise ValueError("StandaloneSS paths 3 and 4 support LambertianSSSurface only")
    g = cfg.geometry
    if not float(g.mu0) > 0:
        raise ValueError("SSGeometry.mu0 must be positive")
    if len(g.mu_v) == 0 or not all(float(m) > 0 for m in g.mu_v):
        raise ValueError("all SSGeometry.mu_v entries must be positive")
    if len(g.mu_v) != len(g.dphi):
        raise ValueError("SSGeometry.mu_v and SSGeometry.dphi must have the same length")
    if cfg.inner_nquad <= 0 or cfg.azimuth_nquad <= 0:
        raise ValueError("ExactSSConfig.inner_nquad and azimuth_nquad must be positive")
    L, S = _dims(cfg.contributors)
    if L < 1 or S < 1:
        raise ValueError("ExactSSConfig requires at least one layer and one spectral point")
    if isinstance(cfg.surface, CoxMunkSSSurface) and cfg.surface.n_water is not None and np.ndim(cfg.surface.n_water) != 0:
        raise NotImplementedError("CoxMunkSSSurface: a per-point n_water table is not built (scalar n_water only)")
    if not isinstance(cfg.surface, (LambertianSSSurface, CoxMunkSSSurface)):
        raise ValueError("surface %r is not a StandaloneSS surface" % (cfg.surface,))
    return L, S


def _vectorize(x, S, what, FT):
    a = np.asarray(x, dtype=FT)
    if a.ndim == 0:
        return np.full(S, a, dtype=FT)
    if a.shape != (S,):
        raise ValueError("%s length must match nSpec" % what)
    return np.ascontiguousarray(a)


# ---- the device side ------------------------------------------------------------------------------------------------------
class _Device:
    """The inputs of one config resident in HBM: per contributor its (nLayer, nSpec) optical depths, I0, and the small host tables."""

    def __init__(self, cfg, paths):
        self.cfg, self.paths = cfg, paths
        self.L, self.S = _validate_config(cfg, paths)
        self.n, self.nV, self.Cn = _n_stokes(cfg), len(cfg.geometry.mu_v), len(cfg.contributors)
        self.FT = np.dtype(cfg.float_type).type
        self.dt = torch.float64 if self.FT == np.float64 else torch.float32
        _lib.suffix(self.dt)
        arch = cfg.architecture if cfg.architecture is not None else default_architecture()
        if not isinstance(arch, GPU):
            raise _lib.VSMError("StandaloneSS runs on Architectures.GPU() only (there is no CPU fallback)")
        _lib.lib()
        self.arch, self.conv = arch, array_type(arch)
        self.ct = C.c_double if self.dt == torch.float64 else C.c_float
        self.tau = [self.conv(np.ascontiguousarray(np.asarray(c.tau, dtype=self.FT))) for c in cfg.contributors]
        self.tau_tab = (C.c_void_p * (self.Cn * self.L))(*[t[iz].data_ptr() for t in self.tau for iz in range(self.L)])
        self.varpi = self._host([single_scattering_albedo(c) for c in cfg.contributors])
        self.I0 = self.conv(_vectorize(cfg.I0, self.S, "ExactSSConfig.I0", self.FT))
        self.mu_v = self._host(cfg.geometry.mu_v)
        self.mu0 = self.ct(float(self.FT(cfg.geometry.mu0)))
        self._p = None

    def _host(self, x):
        a = np.ascontiguousarray(np.asarray(x, dtype=self.FT)).ravel()
        return (self.ct * a.size)(*a.tolist())

    def _out(self, *shape):
        return torch.empty(shape, dtype=self.dt, device=self.I0.device)

    def p_table(self):
        if self._p is None:
            self._p = self._host(phase_table(self.cfg, self.n))
        return self._p

    def path1(self):
        out = self._out(self.S, self.n, self.nV)
        _lib.call("vsm_exact_ss_path1", self.dt, self.S, self.L, self.Cn, self.nV, self.n, self.tau_tab, self.varpi, self.p_table(),
                  CR._ptr(self.I0), self.mu0, self.mu_v, CR._ptr(out), CR._stream_ptr())
        return out

    def surface_brdf(self, max_m=None):
        """(brdf, spectral): [nGeom, nStokes] or [nGeom, nStokes, nSpec] as a layout tensor (nStokes, nGeom) / (nSpec, nStokes, nGeom).
        max_m: the Fourier reconstruction from the moments m < max_m instead (truncated.jl:116-184; a Lambertian surface is its own)."""
        sf, g = self.cfg.surface, self.cfg.geometry
        if isinstance(sf, LambertianSSSurface):
            if np.ndim(sf.albedo) == 0:
                b = np.zeros((self.n, self.nV), dtype=self.FT)
                b[0] = self.FT(sf.albedo) / self.FT(math.pi)
                return self.conv(b), 0
            b = np.zeros((self.S, self.n, self.nV), dtype=self.FT)
            b[:, 0, :] = (_vectorize(sf.albedo, self.S, "LambertianSSSurface.albedo", self.FT) / self.FT(math.pi))[:, None]
            return self.conv(b), 1
        core = H.CoxMunkSurface(float(sf.wind_speed), complex(1.34, 0.0) if sf.n_water is None else complex(sf.n_water),
                                float(sf.whitecap_albedo), bool(sf.include_whitecaps), bool(sf.shadowing))
        cs = CR._coxmunk_cstruct(core, self.dt)
        phi, w = CR.brdf_azimuth_quadrature(self.arch, self.FT)
        out = self._out(self.n, self.nV)
        exact, trunc = (CR._ptr(out), None) if max_m is None else (None, CR._ptr(out))
        _lib.call("vsm_coxmunk_first_column", self.dt, C.byref(cs), self.n, self.nV, self.mu_v, self._host(g.dphi), self.mu0,
                  1 if max_m is None else int(max_m), int(phi.numel()), CR._ptr(phi), CR._ptr(w), exact, trunc, CR._stream_ptr())
        return out, 0

    def path2(self, max_m=None):
        brdf, spectral = self.surface_brdf(max_m)
        out = self._out(self.S, self.n, self.nV)
        _lib.call("vsm_exact_ss_path2", self.dt, self.S, self.L, self.Cn, self.nV, self.n, self.tau_tab, CR._ptr(brdf), spectral,
                  CR._ptr(self.I0), self.mu0, self.mu_v, CR._ptr(out), CR._stream_ptr())
        return out

    def path34(self, want3, want4, nodes=None):
        cfg, g = self.cfg, self.cfg.geometry
        mu_n, wq = gauss_legendre_01(cfg.inner_nquad) if nodes is None else nodes
        albedo = self.conv(_vectorize(cfg.surface.albedo, self.S, "LambertianSSSurface.albedo", self.FT))
        pb3 = self._host(pbar_table(cfg, mu_n, [g.mu0] * self.nV)) if want3 else None
        pb4 = self._host(pbar_table(cfg, mu_n, g.mu_v)) if want4 else None
        o3 = self._out(self.S, 1, self.nV) if want3 else None
        o4 = self._out(self.S, 1, self.nV) if want4 else None
        _lib.call("vsm_exact_ss_path34", self.dt, self.S, self.L, self.Cn, self.nV, len(mu_n), self.tau_tab, self.varpi, pb3, pb4,
                  self._host(mu_n), self._host(wq), CR._ptr(albedo), CR._ptr(self.I0), self.mu0, self.mu_v, CR._ptr(o3), CR._ptr(o4),
                  CR._stream_ptr())
        return o3, o4

    def jac12(self, want1, want2):
        shape4, dev = (self.L, self.S, self.n, self.nV), self.I0.device
        j1 = [self._out(*shape4) for _ in range(3)] if want1 else [None] * 3
        j2 = [self._out(*shape4), self._out(self.S, self.n, self.nV)] if want2 else [None] * 2
        brdf, spectral = self.surface_brdf() if want2 else (None, 0)
        _lib.call("vsm_exact_ss_jac12", self.dt, self.S, self.L, self.Cn, self.nV, self.n, self.tau_tab, self.varpi,
                  self.p_table() if want1 else None, CR._ptr(brdf), spectral, CR._ptr(self.I0), self.mu0, self.mu_v,
                  *[CR._ptr(t) for t in j1 + j2], CR._stream_ptr())
        z4 = lambda: torch.zeros(shape4, dtype=self.dt, device=dev)
        if not want1:
            j1 = [z4(), z4(), z4()]
        if not want2:
            j2 = [z4(), torch.zeros((self.S, self.n, self.nV), dtype=self.dt, device=dev)]
        return j1, j2


def _host3(t):
    return to_host(t).transpose(2, 1, 0).copy()        # (nSpec, nStokes, nGeom) layout tensor -> [nGeom, nStokes, nSpec]


def _host4(t):
    return to_host(t).transpose(3, 2, 1, 0).copy()     # (nLayer, nSpec, nStokes, nGeom) -> [nGeom, nStokes, nSpec, nLayer]


def _run_device(cfg, paths, inner_nodes=None):
    d = _Device(cfg, paths)
    p = [None] * 4
    if _wants(paths, 1):
        p[0] = d.path1()
    if _wants(paths, 2):
        p[1] = d.path2()
    if _wants(paths, 3) or _wants(paths, 4):
        p[2], p[3] = d.path34(_wants(paths, 3), _wants(paths, 4), inner_nodes)
    return d, p


def _as_config(config_or_model, i_band, I0):
    if isinstance(config_or_model, ExactSSConfig):
        return config_or_model if I0 is None else replace(config_or_model, I0=I0)
    return exact_ss_config_from_model(config_or_model, i_band=i_band, I0=I0)


def run_exact_ss(config_or_model, paths: str = "paths_1_2", i_band: int = 1, I0=None, inner_nodes=None) -> ExactSSResult:
    """run_exact_ss(config; paths) / run_exact_ss(model; i_band, paths, I0) (solver.jl:516-598, model_adapter.jl:34-38).
    Returns (total, path1, path2, path3, path4, quadrature_info, metadata); radiances [nGeom, nStokes, nSpec] host arrays, the
    paths not asked for zero.  inner_nodes = (nodes, weights): an inner quadrature on (0, 1) other than inner_nquad-point
    Gauss-Legendre."""
    cfg = _as_config(config_or_model, i_band, I0)
    d, p = _run_device(cfg, paths, inner_nodes)
    synchronize_if_gpu()
    host = [np.zeros((d.nV, d.n, d.S), dtype=d.FT) if t is None else _host3(t) for t in p]
    total = np.zeros_like(host[0])
    for i in range(4):               # _requested_total (solver.jl:46-65)
        if _wants(paths, i + 1):
            total = total + host[i]
    return ExactSSResult(total, host[0], host[1], host[2], host[3],
                         dict(paths=paths, kernel_backend="ROCm", inner_quadrature=cfg.inner_nquad, azimuth_quadrature=cfg.azimuth_nquad),
                         dict(n_layers=d.L, n_spec=d.S, n_geom=d.nV, n_stokes=d.n))


# ---- model_adapter.jl ----------------------------------------------------------------------------------------------------
def exact_ss_config_from_model(model: H.RTModel, i_band: int = 1, I0=None) -> ExactSSConfig:
    """exact_ss_config_from_model (model_adapter.jl:13-131): Rayleigh as a Greek contributor with varpi = 1, absorption, one Greek
    contributor per aerosol.  Refuses truncated aerosol optics, non-scalar aerosol albedos and surfaces other than Lambertian /
    Cox-Munk."""
    if i_band != 1:
        raise _lib.VSMError("single-band models only (i_band = 1)")
    FT = model.float_type
    S, L = model.tau_rayl.shape
    sf = model.surface
    if isinstance(sf, H.LambertianSurfaceScalar):
        surface = LambertianSSSurface(float(sf.albedo))
    elif isinstance(sf, (H.LambertianSurfaceLegendre, H.LambertianSurfaceSpline)):
        surface = LambertianSSSurface(H.surface_albedo_spectrum(sf, S, FT))
    elif isinstance(sf, H.CoxMunkSurface):
        surface = CoxMunkSSSurface(float(sf.wind_speed), sf.n_water, float(sf.whitecap_albedo), bool(sf.include_whitecaps),
                                   bool(sf.shadowing))
    else:
        raise ValueError("exact_ss_config_from_model does not support surface %s" % type(sf).__name__)
    contributors = []
    tau_rayl = np.asarray(model.tau_rayl, dtype=np.float64).T
    if np.any(tau_rayl != 0):
        contributors.append(GreekCoefsSSContributor(model.greek_rayleigh, 1.0, tau_rayl))
    tau_abs = np.asarray(model.tau_abs, dtype=np.float64).T
    if np.any(tau_abs != 0):
        contributors.append(AbsorptionSSContributor(tau_abs))
    for ia, ao in enumerate(model.aerosol_optics):
        tau_aer = np.repeat(np.asarray(model.tau_aer[ia], dtype=np.float64)[:, None], S, axis=1)
        if not np.any(tau_aer != 0):
            continue
        if np.any(np.asarray(ao.f_trunc) != 0):
            raise ValueError("exact_ss_config_from_model supports only untruncated aerosol optics (f_trunc == 0)")
        if np.ndim(ao.ssa) != 0:
            raise ValueError("exact_ss_config_from_model supports scalar aerosol single-scattering albedo only")
        contributors.append(GreekCoefsSSContributor(ao.greek_coefs, float(ao.ssa), tau_aer))
    if not contributors:
        raise ValueError("model has no nonzero Rayleigh, aerosol, or absorption optical depth in band %d" % i_band)
    geometry = SSGeometry(H.cosd(float(model.sza)), [H.cosd(float(v)) for v in model.vza], [math.radians(float(a)) for a in model.vaz])
    return ExactSSConfig(geometry, surface, tuple(contributors), np.ones(S) if I0 is None else I0,
                         polarization_type=model.polarization_type, architecture=model.architecture, float_type=FT)


# ---- truncated.jl --------------------------------------------------------------------------------------------------------
_GREEK = ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")


def _validate_l_trunc(l_trunc):
    if isinstance(l_trunc, bool) or not isinstance(l_trunc, (int, np.integer)):
        raise ValueError("truncated_ss_path1 requires an integer l_trunc; got %s" % type(l_trunc).__name__)
    if l_trunc < 2:
        raise ValueError("truncated_ss_path1 requires l_trunc >= 2")
    return int(l_trunc)


def _validate_max_m(max_m):
    if isinstance(max_m, bool) or not isinstance(max_m, (int, np.integer)):
        raise ValueError("truncated_ss_path2 requires an integer max_m; got %s" % type(max_m).__name__)
    if max_m <= 0:
        raise ValueError("truncated_ss_path2 requires max_m > 0")
    return int(max_m)


def _truncate_greek(greek, n):
    n = min([n] + [len(getattr(greek, k)) for k in _GREEK])
    if n < 2:
        raise ValueError("Greek coefficient truncation requires at least two retained moments")
    return H.GreekCoefs(*(np.asarray(getattr(greek, k), dtype=np.float64)[:n] for k in _GREEK))


def _moment_limited_contributor(c, n):
    if isinstance(c, AbsorptionSSContributor):
        return c
    if isinstance(c, RayleighSSContributor):
        return GreekCoefsSSContributor(_truncate_greek(H.get_greek_rayleigh(c.depol), n), 1.0, c.tau)
    if isinstance(c, HGAerosolSSContributor):
        if not abs(c.g) < 1:
            raise ValueError("Henyey-Greenstein asymmetry parameter must satisfy abs(g) < 1")
        z = np.zeros(n)
        beta = np.array([(2 * l + 1) * float(c.g) ** l for l in range(n)])
        return GreekCoefsSSContributor(H.GreekCoefs(z.copy(), beta, z.copy(), z.copy(), z.copy(), z.copy()), c.varpi, c.tau)
    return GreekCoefsSSContributor(_truncate_greek(c.greek_coefs, n), c.varpi, c.tau)


def _truncated_path1_device(cfg, l_trunc):
    n = _validate_l_trunc(l_trunc)
    return _run_device(replace(cfg, contributors=tuple(_moment_limited_contributor(c, n) for c in cfg.contributors)), "path1")[1][0]


def truncated_ss_path1(config: ExactSSConfig, l_trunc) -> np.ndarray:
    """Path 1 with the phase functions reconstructed from the first l_trunc Greek moments; optical depths and albedos unchanged."""
    t = _truncated_path1_device(config, l_trunc)
    synchronize_if_gpu()
    return _host3(t)


def truncated_ss_path2(config: ExactSSConfig, max_m) -> np.ndarray:
    """Path 2 with the surface BRDF reconstructed from the Fourier moments m = 0 .. max_m - 1."""
    t = _Device(config, "path2").path2(_validate_max_m(max_m))
    synchronize_if_gpu()
    return _host3(t)


def _back_correction_device(cfg, l_trunc, max_m):
    m = _validate_max_m(max_m)
    d, p = _run_device(cfg, "paths_1_2")
    return (p[0] + p[1]) - (_truncated_path1_device(cfg, l_trunc) + d.path2(m))


def apply_back_correction(R_SFI, config_or_model, l_trunc=None, max_m=None, i_band: int = 1, I0=None):
    """apply_back_correction! (truncated.jl:258-277): R_SFI + exact(path 1 + 2) - truncated(path 1 + 2), as the reference states it.
    R_SFI [nGeom, nStokes, nSpec]: a host array (a new array is returned) or a device tensor in the (nSpec, nStokes, nGeom) layout
    of CoreRT's R_SFI (corrected in place and returned).  With a model, max_m defaults to the model's (the number
    of Fourier moments, m_max + 1; the RTModel does not record l_trunc, which must be given) and I0 passes through to
    exact_ss_config_from_model (default 1: the units of rt_run with F0 = e1, module docstring)."""
    if isinstance(config_or_model, ExactSSConfig):
        cfg = config_or_model if I0 is None else replace(config_or_model, I0=I0)
        if l_trunc is None or max_m is None:
            raise ValueError("apply_back_correction(R_SFI, config): l_trunc and max_m are required")
    else:
        model = config_or_model
        cfg = exact_ss_config_from_model(model, i_band=i_band, I0=I0)
        if l_trunc is None:      # the reference reads model.solver.l_max; this RTModel keeps the streams l_trunc made, not l_trunc
            raise ValueError("apply_back_correction(R_SFI, model): the RTModel does not record l_trunc; pass l_trunc")
        if max_m is None:
            max_m = int(model.m_max) + 1
    corr = _back_correction_device(cfg, l_trunc, max_m)
    if isinstance(R_SFI, torch.Tensor):
        if tuple(R_SFI.shape) != tuple(corr.shape):
            raise ValueError("R_SFI has shape %r; expected %r" % (tuple(R_SFI.shape), tuple(corr.shape)))
        R_SFI += corr.to(R_SFI.dtype)
        return R_SFI
    synchronize_if_gpu()
    corr = _host3(corr)
    if np.shape(R_SFI) != corr.shape:
        raise ValueError("R_SFI has shape %r; expected %r" % (np.shape(R_SFI), corr.shape))
    return np.asarray(R_SFI) + corr


# ---- linearized_f2.jl ----------------------------------------------------------------------------------------------------
def run_exact_ss_with_jacobians(config: ExactSSConfig, paths: str = "paths_1_2") -> dict:
    """run_exact_ss_with_jacobians (linearized_f2.jl:145-182) without the measurement selector: the result of run_exact_ss as a dict
    plus "jacobians" = {total, path1, path2}; path1: tau_layer / varpi_eff / P_eff, path2: tau_layer / surface_brdf, total: the
    four, [nGeom, nStokes, nSpec, nLayer] ([nGeom, nStokes, nSpec] for surface_brdf) -- with respect to the seam variables, the
    others held fixed."""
    if paths not in ("path1", "path2", "paths_1_2"):
        raise ValueError("StandaloneSS Jacobians support 'path1', 'path2' and 'paths_1_2'; got %r" % (paths,))
    res = run_exact_ss(config, paths)
    d = _Device(config, paths)
    j1, j2 = d.jac12(_wants(paths, 1), _wants(paths, 2))
    synchronize_if_gpu()
    p1 = dict(tau_layer=_host4(j1[0]), varpi_eff=_host4(j1[1]), P_eff=_host4(j1[2]))
    p2 = dict(tau_layer=_host4(j2[0]), surface_brdf=_host3(j2[1]))
    total = dict(tau_layer=p1["tau_layer"] + p2["tau_layer"], varpi_eff=p1["varpi_eff"], P_eff=p1["P_eff"],
                 surface_brdf=p2["surface_brdf"])
    out = res._asdict()
    out["jacobians"] = dict(total=total, path1=p1, path2=p2)
    return out
