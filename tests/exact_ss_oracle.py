"""Test oracle of vsm.StandaloneSS: a numpy restatement of the reference's exact single-scattering solver (src/StandaloneSS), host
statements and kernel statements alike.  It materialises P_eff[nGeom, nStokes, nLayer, nSpec] and the azimuthal averages
Pbar[nGeom, nLayer, nSpec, nQuad] exactly as the reference does (solver.jl:199-397) -- the arrays the device kernels never form.

types.jl            SSGeometry, the surfaces, the four contributors, ExactSSConfig, exact_phase_function
solver.jl           precompute_optics (:199-317), azimuthal_average_phase (:143-167), precompute_azimuthal_phase (:319-345),
                    run_exact_ss (:516-598)
kernels.jl          path1 (:1-38), path2 (:40-60), tau_integral (:62-71), inner_scatter_sum (:73-90), path34 (:199-231)
surfaces.jl         precompute_surface_brdf (:46-106), the Cox-Munk Mueller matrix from oracle/vsm_oracle_coxmunk.py
truncated.jl        truncated_ss_path1 / truncated_ss_path2 / apply_back_correction
linearized_f2.jl    path1_jacobians (:34-71, the O(L^2) loop as written), path2_jacobians (:78-102)
Scattering          reconstruct_phase (mie_helper_functions.jl:415-446), compute_legendre_poly (legendre_functions.jl:223-265),
                    phase_matrix_first_column (analytic_phase_functions.jl:165-208), get_greek_rayleigh

Optical depths are (nLayer, nSpec) matrices; radiances [nGeom, nStokes, nSpec]; Jacobians [nGeom, nStokes, nSpec, nLayer].
All arithmetic in FP64.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass, field, replace
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import vsm_oracle_coxmunk as CM  # noqa: E402

PATHS = ("path1", "path2", "path3", "path4", "paths_1_2", "all", "all_four")
GREEK_KEYS = ("alpha", "beta", "gamma", "delta", "epsilon", "zeta")


def wants(paths, i):
    return paths in {1: ("path1", "paths_1_2", "all", "all_four"), 2: ("path2", "paths_1_2", "all", "all_four"),
                     3: ("path3", "all", "all_four"), 4: ("path4", "all", "all_four")}[i]


# ---- types.jl ------------------------------------------------------------------------------------------------------------
@dataclass
class SSGeometry:
    mu0: float
    mu_v: Sequence[float]
    dphi: Sequence[float]


@dataclass
class LambertianSSSurface:
    albedo: object            # scalar or [nSpec]


@dataclass
class CoxMunkSSSurface:
    wind_speed: float
    n_water: Optional[complex] = None     # None -> 1.34 + 0i (surfaces.jl:222)
    whitecap_albedo: float = 0.22
    include_whitecaps: bool = True
    shadowing: bool = True


@dataclass
class RayleighSSContributor:
    tau: np.ndarray
    depol: float = 0.0


@dataclass
class HGAerosolSSContributor:
    g: float
    varpi: float
    tau: np.ndarray


@dataclass
class GreekCoefsSSContributor:
    greek_coefs: object       # .alpha .beta .gamma .delta .epsilon .zeta
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
    I0: object
    n_stokes: int = 1
    inner_nquad: int = 16
    azimuth_nquad: int = 64
    mu_nodes: Optional[tuple] = None      # (nodes, weights) instead of Gauss-Legendre on (0, 1): the kernel-level tests


def single_scattering_albedo(c):
    if isinstance(c, RayleighSSContributor):
        return 1.0
    if isinstance(c, AbsorptionSSContributor):
        return 0.0
    return float(c.varpi)


def get_greek_rayleigh(depol):
    p = (1 - depol) / (1 + depol / 2)
    r = (1 - 2 * depol) / (1 - depol)
    z = np.zeros(3)
    return SimpleNamespace(alpha=np.array([0, 0, 3 * p]), beta=np.array([1, 0, 0.5 * p]), gamma=np.array([0, 0, p * math.sqrt(1.5)]),
                           delta=np.array([0, 1.5 * p * r, 0]), epsilon=z.copy(), zeta=z.copy())


def _depol_scale(depol):
    return (1 - depol) / (1 + depol / 2)


def compute_legendre_poly(x, nmax):
    """legendre_functions.jl:223-265: P0, P2 [len(x), nmax] (R2 / T2 are not needed for the first column)."""
    assert nmax > 1
    x = np.asarray(x, dtype=np.float64)
    P0, P2 = np.zeros((len(x), nmax)), np.zeros((len(x), nmax))
    P0[:, 0] = 1
    P0[:, 1] = x
    if nmax > 2:
        P2[:, 2] = 3 * (1 - x ** 2)
    for n in range(2, nmax):
        l = n - 1
        P0[:, n] = ((2 * l + 1) * x * P0[:, n - 1] - l * P0[:, n - 2]) / (l + 1)
        if n > 2:
            P2[:, n] = ((2 * l + 1) * x * P2[:, n - 1] - (l + 2) * P2[:, n - 2]) / (l - 1)
    return P0, P2


def reconstruct_phase(greek, mu):
    """f11, f12 of reconstruct_phase (mie_helper_functions.jl:415-446)."""
    beta, gamma = np.asarray(greek.beta, dtype=np.float64), np.asarray(greek.gamma, dtype=np.float64)
    lmax = len(np.asarray(greek.alpha))
    P0, P2 = compute_legendre_poly(np.atleast_1d(mu), lmax)
    fac = np.zeros(lmax)
    for l in range(2, lmax):
        fac[l] = math.sqrt(1.0 / ((l - 1) * l * (l + 1) * (l + 2)))
    return P0 @ beta, P2 @ (fac * gamma)


def scattering_angle_cosine(mu0, mu_v, dphi):
    return -mu0 * mu_v + math.sqrt(max(0.0, 1 - mu0 ** 2)) * math.sqrt(max(0.0, 1 - mu_v ** 2)) * math.cos(dphi)


def phase_matrix_first_column(greek, mu0, mu_v, dphi, n):
    """analytic_phase_functions.jl:169-208."""
    cosT = scattering_angle_cosine(mu0, mu_v, dphi)
    f11, f12 = reconstruct_phase(greek, [cosT])
    f11, f12 = float(f11[0]), float(f12[0])
    sin2 = max(0.0, 1 - cosT ** 2)
    if sin2 <= np.finfo(np.float64).eps:
        c2, s2 = 1.0, 0.0
    else:
        sinT = math.sqrt(sin2)
        s0, sv = math.sqrt(max(0.0, 1 - mu0 ** 2)), math.sqrt(max(0.0, 1 - mu_v ** 2))
        cchi = (mu0 * sv + mu_v * s0 * math.cos(dphi)) / sinT
        schi = s0 * math.sin(dphi) / sinT
        c2, s2 = cchi ** 2 - schi ** 2, 2 * schi * cchi
    return np.array([f11, f12 * c2, f12 * s2, 0.0][:n])


def exact_phase_function(c, cosT):
    if isinstance(c, RayleighSSContributor):
        return 1 + 0.5 * _depol_scale(c.depol) * (3 * cosT ** 2 - 1) / 2
    if isinstance(c, HGAerosolSSContributor):
        return (1 - c.g ** 2) / (1 + c.g ** 2 - 2 * c.g * cosT) ** 1.5
    if isinstance(c, GreekCoefsSSContributor):
        return float(reconstruct_phase(c.greek_coefs, [cosT])[0][0])
    return 0.0


def phase_first_column(c, n, mu0, mu_v, dphi):
    greek = get_greek_rayleigh(c.depol) if isinstance(c, RayleighSSContributor) else c.greek_coefs
    return phase_matrix_first_column(greek, mu0, mu_v, dphi, n)


# ---- solver.jl -----------------------------------------------------------------------------------------------------------
def validate_config(cfg, paths):
    if paths not in PATHS:
        raise ValueError("StandaloneSS supports paths %s; got %r" % (", ".join(PATHS), paths))
    n = cfg.n_stokes
    if n != 1 and paths not in ("path1", "path2", "paths_1_2"):
        raise ValueError("StandaloneSS vector Stokes kernels support only path1, path2 and paths_1_2")
    if n != 1 and wants(paths, 1):
        for c in cfg.contributors:
            if isinstance(c, HGAerosolSSContributor):
                raise ValueError("StandaloneSS vector path1 supports Rayleigh, Greek and absorption contributors only")
    if (wants(paths, 3) or wants(paths, 4)) and not isinstance(cfg.surface, LambertianSSSurface):
        raise ValueError("StandaloneSS paths 3 and 4 support LambertianSSSurface only")
    g = cfg.geometry
    if not g.mu0 > 0 or not all(m > 0 for m in g.mu_v) or len(g.mu_v) != len(g.dphi):
        raise ValueError("bad SSGeometry")
    if not cfg.contributors:
        raise ValueError("ExactSSConfig requires at least one contributor")
    shp = np.asarray(cfg.contributors[0].tau).shape
    if len(shp) != 2 or any(np.asarray(c.tau).shape != shp for c in cfg.contributors):
        raise ValueError("contributor optical depths must be (nLayer, nSpec) matrices of one shape")
    return shp


def _vec(x, n, what):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 0:
        return np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError("%s length must match nSpec" % what)
    return a.copy()


def precompute_optics(cfg, n):
    """solver.jl:199-317 -> tau_layer, tau_scat [L,S], tau_cum [L+1,S], varpi_eff [L,S], P_eff [nGeom,n,L,S]."""
    L, S = np.asarray(cfg.contributors[0].tau).shape
    g = cfg.geometry
    nG = len(g.mu_v)
    tau_layer, tau_scat, weighted = np.zeros((L, S)), np.zeros((L, S)), np.zeros((nG, n, L, S))
    for c in cfg.contributors:
        tau, w = np.asarray(c.tau, dtype=np.float64), single_scattering_albedo(c)
        tau_layer += tau
        tau_scat += tau * w
        if w == 0 or isinstance(c, AbsorptionSSContributor):
            continue
        for iv in range(nG):
            if n == 1:
                col = [exact_phase_function(c, scattering_angle_cosine(g.mu0, g.mu_v[iv], g.dphi[iv]))]
            else:
                col = phase_first_column(c, n, g.mu0, g.mu_v[iv], g.dphi[iv])
            for k in range(n):
                weighted[iv, k] += (tau * w) * col[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        varpi_eff = np.where(tau_layer == 0, 0.0, tau_scat / tau_layer)
        P_eff = np.where(tau_scat[None, None] != 0, weighted / tau_scat[None, None], 0.0)
    tau_cum = np.zeros((L + 1, S))
    for iz in range(L):
        tau_cum[iz + 1] = tau_cum[iz] + tau_layer[iz]
    return SimpleNamespace(tau_layer=tau_layer, tau_scat=tau_scat, tau_cum=tau_cum, varpi_eff=varpi_eff, P_eff=P_eff)


def rayleigh_azimuthal_average(mu_a, mu_b, depol):
    a = mu_a * mu_b
    b = math.sqrt(max(0.0, 1 - mu_a ** 2)) * math.sqrt(max(0.0, 1 - mu_b ** 2))
    return 1 + 0.5 * _depol_scale(depol) * (3 * (a * a + 0.5 * b * b) - 1) / 2


def azimuthal_average_phase(c, mu_a, mu_b, n_phi):
    """solver.jl:143-167."""
    if isinstance(c, RayleighSSContributor):
        return rayleigh_azimuthal_average(mu_a, mu_b, c.depol)
    a = mu_a * mu_b
    b = math.sqrt(max(0.0, 1 - mu_a ** 2)) * math.sqrt(max(0.0, 1 - mu_b ** 2))
    total = 0.0
    for k in range(n_phi):
        phi = 2 * math.pi * k / n_phi
        total += exact_phase_function(c, min(max(a + b * math.cos(phi), -1.0), 1.0))
    return total / n_phi


def precompute_azimuthal_phase(cfg, tau_scat, mu_nodes, reference_mu):
    """solver.jl:319-357 -> Pbar [nGeom, L, S, nQ]."""
    L, S = tau_scat.shape
    nG, nQ = len(reference_mu), len(mu_nodes)
    Pbar = np.zeros((nG, L, S, nQ))
    for c in cfg.contributors:
        w = single_scattering_albedo(c)
        if w == 0:
            continue
        sw = np.asarray(c.tau, dtype=np.float64) * w
        for iv in range(nG):
            for k in range(nQ):
                Pbar[iv, :, :, k] += sw * azimuthal_average_phase(c, float(mu_nodes[k]), float(reference_mu[iv]), cfg.azimuth_nquad)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tau_scat[None, :, :, None] != 0, Pbar / tau_scat[None, :, :, None], Pbar)


def gauss_legendre_01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return (x + 1) / 2, w / 2


# ---- surfaces.jl / truncated.jl -------------------------------------------------------------------------------------------
def _cm_core(surface):
    return CM.CoxMunkSurface(surface.wind_speed, None, surface.whitecap_albedo, surface.include_whitecaps, surface.shadowing)


def _cm_n_water(surface):
    return complex(1.34, 0.0) if surface.n_water is None else complex(surface.n_water)


def precompute_surface_brdf(cfg, n, S):
    """surfaces.jl:46-106 -> [nGeom, n, S]."""
    g, sf = cfg.geometry, cfg.surface
    rho = np.zeros((len(g.mu_v), n, S))
    if isinstance(sf, LambertianSSSurface):
        rho[:, 0, :] = _vec(sf.albedo, S, "albedo")[None, :] / math.pi
        return rho
    core, nw = _cm_core(sf), _cm_n_water(sf)
    for iv in range(len(g.mu_v)):
        M = CM.coxmunk_brdf_mueller(core, n, g.mu_v[iv], g.mu0, g.dphi[iv], n_water=nw)
        rho[iv] = np.asarray(M)[:n, 0][:, None]
    return rho


def _az_kernel(si, m, dphi):
    return math.cos(m * dphi) if si <= 1 else math.sin(m * dphi)     # column 1 (sj = 1): rows I, Q cos; U, V sin


def precompute_surface_brdf_fourier(cfg, n, S, max_m):
    """truncated.jl:116-184 (100-point Gauss-Legendre on (0, pi)); Lambertian: the exact BRDF (:209-211)."""
    g, sf = cfg.geometry, cfg.surface
    if isinstance(sf, LambertianSSSurface):
        return precompute_surface_brdf(cfg, n, S)
    core, nw = _cm_core(sf), _cm_n_water(sf)
    x, w = np.polynomial.legendre.leggauss(100)
    phi, wphi = (math.pi / 2) * (x + 1), (math.pi / 2) * w
    rho = np.zeros((len(g.mu_v), n, S))
    for iv in range(len(g.mu_v)):
        cols = np.asarray(CM.coxmunk_brdf_mueller(core, n, g.mu_v[iv], g.mu0, phi, n_water=nw))[:, :n, 0]   # [nphi, n]
        for si in range(n):
            value = 0.0
            for m in range(max_m):
                coeff = sum(wphi[i] * cols[i, si] * _az_kernel(si, m, phi[i]) for i in range(len(phi)))
                coeff = (1.0 if m == 0 else 2.0) * coeff / math.pi
                value += (0.5 if m == 0 else 1.0) * _az_kernel(si, m, g.dphi[iv]) * coeff
            rho[iv, si] = value
    return rho


# ---- kernels.jl ----------------------------------------------------------------------------------------------------------
def path1_kernel(tau_cum, varpi_eff, P_eff, mu0, mu_v, I0):
    nG, n, L, S = P_eff.shape
    out = np.zeros((nG, n, S))
    for iv in range(nG):
        a = 1 / mu0 + 1 / mu_v[iv]
        pre = I0 / (4 * math.pi * mu_v[iv] * a)
        for iz in range(L):
            lf = np.exp(-tau_cum[iz] * a) - np.exp(-tau_cum[iz + 1] * a)
            out[iv] += pre * varpi_eff[iz] * P_eff[iv, :, iz] * lf
    return out


def path2_kernel(tau_total, mu0, mu_v, brdf, I0):
    mv = np.asarray(mu_v, dtype=np.float64)[:, None, None]
    return (mu0 * I0[None, None, :] * brdf) * np.exp(-tau_total / mu0)[None, None, :] * np.exp(-tau_total[None, None, :] / mv)


def tau_integral(t_top, t_bot, t_tot, m1, m2):
    b = 1 / m1 - 1 / m2
    f_top = np.exp(-t_top / m1 - (t_tot - t_top) / m2)
    f_bot = np.exp(-t_bot / m1 - (t_tot - t_bot) / m2)
    if abs(b) < 1e-10:
        return 0.5 * (f_top + f_bot) * (t_bot - t_top)
    return (f_top - f_bot) / b


def inner_scatter_sum(tau_cum, varpi_eff, Pbar, iv, iz, mu_first, mu_nodes, mu_w):
    t_tot = tau_cum[-1]
    s = np.zeros_like(t_tot)
    for k in range(len(mu_nodes)):
        s += mu_w[k] * Pbar[iv, iz, :, k] * tau_integral(tau_cum[iz], tau_cum[iz + 1], t_tot, mu_first, mu_nodes[k]) * 0.5
    return varpi_eff[iz] * s


def path34_kernel(tau_cum, varpi_eff, Pbar3, Pbar4, mu0, mu_v, albedo, I0, mu_nodes, mu_w):
    L, S = varpi_eff.shape
    nG = len(mu_v)
    p3, p4 = np.zeros((nG, 1, S)), np.zeros((nG, 1, S))
    rho = albedo / math.pi
    t_tot = tau_cum[-1]
    for iv in range(nG):
        F, s4 = np.zeros(S), np.zeros(S)
        for iz in range(L):
            if Pbar3 is not None:
                F += I0 * inner_scatter_sum(tau_cum, varpi_eff, Pbar3, iv, iz, mu0, mu_nodes, mu_w)
            if Pbar4 is not None:
                s4 += inner_scatter_sum(tau_cum, varpi_eff, Pbar4, iv, iz, mu_v[iv], mu_nodes, mu_w)
        p3[iv, 0] = np.where(rho == 0, 0.0, rho * F * np.exp(-t_tot / mu_v[iv]))
        p4[iv, 0] = np.where(rho == 0, 0.0, rho * mu0 * I0 * np.exp(-t_tot / mu0) * s4 / mu_v[iv])
    return p3, p4


def run_exact_ss(cfg, paths="paths_1_2", brdf=None, keep=None):
    """solver.jl:516-598 -> SimpleNamespace(total, path1..path4, quadrature_info, metadata).  brdf: a surface BRDF [nGeom, n, S] to
    use for path 2 instead of the surface's own (truncated_ss_path2).  keep: a dict that receives optics / Pbar3 / Pbar4."""
    L, S = validate_config(cfg, paths)
    g, n = cfg.geometry, cfg.n_stokes
    nG = len(g.mu_v)
    op = precompute_optics(cfg, n if wants(paths, 1) else 1)
    I0 = _vec(cfg.I0, S, "I0")
    z = lambda: np.zeros((nG, n, S))
    p1 = path1_kernel(op.tau_cum, op.varpi_eff, op.P_eff, g.mu0, g.mu_v, I0) if wants(paths, 1) else None
    p2 = None
    if wants(paths, 2):
        p2 = path2_kernel(op.tau_cum[-1], g.mu0, g.mu_v, precompute_surface_brdf(cfg, n, S) if brdf is None else brdf, I0)
    p3 = p4 = None
    if wants(paths, 3) or wants(paths, 4):
        albedo = _vec(cfg.surface.albedo, S, "albedo")
        nodes, wq = cfg.mu_nodes if cfg.mu_nodes is not None else gauss_legendre_01(cfg.inner_nquad)
        Pb3 = precompute_azimuthal_phase(cfg, op.tau_scat, nodes, [g.mu0] * nG) if wants(paths, 3) else None
        Pb4 = precompute_azimuthal_phase(cfg, op.tau_scat, nodes, g.mu_v) if wants(paths, 4) else None
        q3, q4 = path34_kernel(op.tau_cum, op.varpi_eff, Pb3, Pb4, g.mu0, g.mu_v, albedo, I0, nodes, wq)
        p3, p4 = (q3 if wants(paths, 3) else None), (q4 if wants(paths, 4) else None)
        if keep is not None:
            keep.update(Pbar3=Pb3, Pbar4=Pb4)
    if keep is not None:
        keep.update(optics=op)
    total = sum(p for p in (p1, p2, p3, p4) if p is not None)
    return SimpleNamespace(total=total.copy(), path1=z() if p1 is None else p1, path2=z() if p2 is None else p2,
                           path3=z() if p3 is None else p3, path4=z() if p4 is None else p4,
                           quadrature_info=dict(paths=paths, inner_quadrature=cfg.inner_nquad, azimuth_quadrature=cfg.azimuth_nquad),
                           metadata=dict(n_layers=L, n_spec=S, n_geom=nG, n_stokes=n))


# ---- truncated.jl --------------------------------------------------------------------------------------------------------
def _truncate_greek(greek, n):
    n = min([n] + [len(np.asarray(getattr(greek, k))) for k in GREEK_KEYS])
    if n < 2:
        raise ValueError("Greek coefficient truncation requires at least two retained moments")
    return SimpleNamespace(**{k: np.asarray(getattr(greek, k), dtype=np.float64)[:n] for k in GREEK_KEYS})


def moment_limited_contributor(c, n):
    if isinstance(c, AbsorptionSSContributor):
        return c
    if isinstance(c, RayleighSSContributor):
        return GreekCoefsSSContributor(_truncate_greek(get_greek_rayleigh(c.depol), n), 1.0, c.tau)
    if isinstance(c, HGAerosolSSContributor):
        if not abs(c.g) < 1:
            raise ValueError("Henyey-Greenstein asymmetry parameter must satisfy abs(g) < 1")
        z = np.zeros(n)
        greek = SimpleNamespace(alpha=z.copy(), beta=np.array([(2 * l + 1) * c.g ** l for l in range(n)]), gamma=z.copy(),
                                delta=z.copy(), epsilon=z.copy(), zeta=z.copy())
        return GreekCoefsSSContributor(greek, c.varpi, c.tau)
    return GreekCoefsSSContributor(_truncate_greek(c.greek_coefs, n), c.varpi, c.tau)


def truncated_ss_path1(cfg, l_trunc):
    if not isinstance(l_trunc, (int, np.integer)) or l_trunc < 2:
        raise ValueError("truncated_ss_path1 requires an integer l_trunc >= 2")
    return run_exact_ss(replace(cfg, contributors=[moment_limited_contributor(c, int(l_trunc)) for c in cfg.contributors]), "path1").path1


def truncated_ss_path2(cfg, max_m):
    if not isinstance(max_m, (int, np.integer)) or max_m <= 0:
        raise ValueError("truncated_ss_path2 requires an integer max_m > 0")
    L, S = validate_config(cfg, "path2")
    return run_exact_ss(cfg, "path2", brdf=precompute_surface_brdf_fourier(cfg, cfg.n_stokes, S, int(max_m))).path2


def ss_back_correction(cfg, l_trunc, max_m):
    return run_exact_ss(cfg, "paths_1_2").total - (truncated_ss_path1(cfg, l_trunc) + truncated_ss_path2(cfg, max_m))


def apply_back_correction(R_SFI, cfg, l_trunc, max_m):
    corr = ss_back_correction(cfg, l_trunc, max_m)
    if np.shape(R_SFI) != corr.shape:
        raise ValueError("R_SFI has shape %r; expected %r" % (np.shape(R_SFI), corr.shape))
    return np.asarray(R_SFI, dtype=np.float64) + corr


# ---- linearized_f2.jl ----------------------------------------------------------------------------------------------------
def path1_jacobians(cfg, op, I0):
    """:34-71, the attenuation-from-above term by the reference's loop over the layers above."""
    nG, n, L, S = op.P_eff.shape
    g = cfg.geometry
    dt, dw, dP = (np.zeros((nG, n, S, L)) for _ in range(3))
    for iv in range(nG):
        a = 1 / g.mu0 + 1 / g.mu_v[iv]
        c0 = I0 / (4 * math.pi * g.mu_v[iv])
        pre = c0 / a
        for iz in range(L):
            w, P = op.varpi_eff[iz], op.P_eff[iv, :, iz]
            lf = np.exp(-op.tau_cum[iz] * a) - np.exp(-op.tau_cum[iz + 1] * a)
            dw[iv, :, :, iz] += pre * P * lf
            dP[iv, :, :, iz] += pre * w * lf
            dt[iv, :, :, iz] += c0 * w * P * np.exp(-op.tau_cum[iz + 1] * a)
            for above in range(iz):
                dt[iv, :, :, above] += -c0 * w * P * lf
    return dict(tau_layer=dt, varpi_eff=dw, P_eff=dP)


def path2_jacobians(cfg, op, I0, path2):
    nG, n, S = path2.shape
    L = op.varpi_eff.shape[0]
    g = cfg.geometry
    dt, dr = np.zeros((nG, n, S, L)), np.zeros((nG, n, S))
    t = op.tau_cum[-1]
    for iv in range(nG):
        dr[iv] = (g.mu0 * I0 * (np.exp(-t / g.mu0) * np.exp(-t / g.mu_v[iv])))[None, :]
        dt[iv] = (-path2[iv] * (1 / g.mu0 + 1 / g.mu_v[iv]))[:, :, None]
    return dict(tau_layer=dt, surface_brdf=dr)


def run_exact_ss_with_jacobians(cfg, paths="paths_1_2"):
    if paths not in ("path1", "path2", "paths_1_2"):
        raise ValueError("StandaloneSS Jacobians support path1, path2 and paths_1_2; got %r" % (paths,))
    res = run_exact_ss(cfg, paths)
    L, S = np.asarray(cfg.contributors[0].tau).shape
    n, nG = cfg.n_stokes, len(cfg.geometry.mu_v)
    op, I0 = precompute_optics(cfg, n), _vec(cfg.I0, S, "I0")
    z4 = lambda: np.zeros((nG, n, S, L))
    j1 = path1_jacobians(cfg, op, I0) if wants(paths, 1) else dict(tau_layer=z4(), varpi_eff=z4(), P_eff=z4())
    j2 = path2_jacobians(cfg, op, I0, res.path2) if wants(paths, 2) else dict(tau_layer=z4(), surface_brdf=np.zeros((nG, n, S)))
    res.jacobians = dict(total=dict(tau_layer=j1["tau_layer"] + j2["tau_layer"], varpi_eff=j1["varpi_eff"], P_eff=j1["P_eff"],
                                    surface_brdf=j2["surface_brdf"]), path1=j1, path2=j2)
    return res


def run_from_seam(cfg, tau_layer, varpi_eff, P_eff, brdf):
    """Paths 1 and 2 as functions of the seam variables (the central differences of the Jacobian tests perturb these)."""
    S = tau_layer.shape[1]
    I0 = _vec(cfg.I0, S, "I0")
    tau_cum = np.vstack([np.zeros((1, S)), np.cumsum(tau_layer, axis=0)])
    g = cfg.geometry
    return path1_kernel(tau_cum, varpi_eff, P_eff, g.mu0, g.mu_v, I0), path2_kernel(tau_cum[-1], g.mu0, g.mu_v, brdf, I0)
