"""Test oracle of the Jacobians with respect to the parameters of the kernel-driven land BRDFs: rpvSurfaceScalar (rho0, rho_c, k,
Theta: NSurf = 4) and RossLiSurfaceScalar (fvol, fgeo, fiso: NSurf = 3).  numpy only; built on oracle/vsm_oracle_brdf.py,
oracle/vsm_oracle_lin.py, oracle/vsm_oracle_coxmunk.py, tests/ss_lin_oracle.py and tests/ms_lin_oracle.py, which it imports and does
not change.

The reference linearizes neither surface, so there is nothing to restate: the derivatives are analytic and pinned by central
differences of the forward oracle (tests/test_oracle_brdf_lin.py).  With rho = OB.brdf_value (the I -> I element):

    RPV      rho = rho0 M F H,  M = (mu_i mu_r (mu_i + mu_r))^(k - 1),  F = (1 - t^2) / D^(3/2),  D = 1 + t^2 + 2 t cos g,
             t = -Theta,  H = 1 + (1 - rho_c) / (1 + G)
             d/drho0 = M F H,  d/drho_c = -rho0 M F / (1 + G),  d/dk = rho ln(mu_i mu_r (mu_i + mu_r)),
             d/dTheta = -rho0 M H dF/dt,  dF/dt = -2 t / D^(3/2) - 3 (1 - t^2)(t + cos g) / D^(5/2)
    Ross-Li  rho = fvol K_vol + fgeo K_geo + fiso:  d/dfvol = K_vol,  d/dfgeo = K_geo,  d/dfiso = 1

reflectance_and_deriv integrates them over azimuth exactly as OB.reflectance integrates rho.  The slots follow the dataclass fields.

create_surface_layer_brdf_lin is CM.create_surface_layer_brdf_lin with K derivative blocks in the slots isurf .. isurf + K - 1, and
rt_run_lin is CM.rt_run_lin's walk with it (P = n_layer_params + K, the surface slots last).

The single-scattering and the multi-sensor oracles (ss_lin_oracle.rt_run_ss_lin, ms_lin_oracle.ms_lin_segmented) carry ONE surface
slot and take the surface as a function m -> (rho_m, drho_m).  Every statement of theirs is linear in the derivative stacks, the
slots do not mix, and the layer slots do not read drho; so slot k of a K-slot run is the surface slot of their run with
(rho_m, drho_m[k]), and the layer slots are those of any of these runs.  rt_run_ss_lin / ms_lin_segmented here assemble the K runs;
test_oracle_brdf_lin.py checks the same assembly of CM.rt_run_lin against the K-slot rt_run_lin above.
"""
from __future__ import annotations

import dataclasses
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402


def param_names(surf):
    return [f.name for f in dataclasses.fields(surf)]


def n_params(surf) -> int:
    return len(param_names(surf))


def perturbed(surf, k: int, h: float):
    """The surface with its k-th parameter moved by h."""
    name = param_names(surf)[k]
    return dataclasses.replace(surf, **{name: getattr(surf, name) + h})


def brdf_value_and_deriv(surf, mu_i, mu_r, dphi):
    """(rho, [d rho / d parameter k]) of the I -> I element, with OB.brdf_value's own intermediates."""
    mu_i, mu_r = np.asarray(mu_i, dtype=np.float64), np.asarray(mu_r, dtype=np.float64)
    th_i, th_r = np.arccos(mu_i), np.arccos(mu_r)
    if isinstance(surf, OB.RPVSurface):
        cosg = -mu_i * mu_r + np.sin(th_i) * np.sin(th_r) * math.cos(dphi)
        G = np.sqrt(np.tan(th_i) ** 2 + np.tan(th_r) ** 2 + 2 * np.tan(th_i) * np.tan(th_r) * math.cos(dphi))
        base = mu_i * mu_r * (mu_i + mu_r)
        M = (mu_i * mu_r) ** (surf.k - 1) / (mu_i + mu_r) ** (1 - surf.k)
        th = -surf.Theta
        D = 1 + th ** 2 + 2 * th * cosg
        F = (1 - th ** 2) / D ** 1.5
        Hh = 1 + (1 - surf.rho_c) / (1 + G)
        dF = -2 * th / D ** 1.5 - 3 * (1 - th ** 2) * (th + cosg) / D ** 2.5
        rho = surf.rho0 * M * F * Hh
        return rho, [M * F * Hh, -surf.rho0 * M * F / (1 + G), rho * np.log(base), -surf.rho0 * M * Hh * dF]
    if isinstance(surf, OB.RossLiSurface):
        one = np.ones(np.broadcast(mu_i, mu_r).shape)
        K_vol = OB.brdf_value(OB.RossLiSurface(1.0, 0.0, 0.0), 1, mu_i, mu_r, dphi)      # (linear in the weights: the kernels are
        K_geo = OB.brdf_value(OB.RossLiSurface(0.0, 1.0, 0.0), 1, mu_i, mu_r, dphi)      #  the BRDF of a unit weight)
        return surf.fiso * one + surf.fvol * K_vol + surf.fgeo * K_geo, [K_vol * one, K_geo * one, one]
    raise TypeError(surf)


def reflectance_and_deriv(surf, n_stokes: int, mu, m: int, nquad: int = 100):
    """(R [N, N], dR [K, N, N]): OB.reflectance's quadrature (ff / pi sum_phi w rho cos(m phi) on the I -> I elements, ff = 1 | 2, the
    m = 0 block not doubled) on rho and on each of its parameter derivatives, in the same loop."""
    mu = np.asarray(mu, dtype=np.float64)
    x, w = np.polynomial.legendre.leggauss(nquad)
    phi, wphi = 0.5 * math.pi * (x + 1.0), 0.5 * math.pi * w
    n, K = len(mu), n_params(surf)
    c, dc = np.zeros((n, n)), np.zeros((K, n, n))
    for p, wp in zip(phi, wphi):
        r, d = brdf_value_and_deriv(surf, mu[:, None], mu[None, :], p)
        c += wp * r * math.cos(m * p)
        for k in range(K):
            dc[k] += wp * d[k] * math.cos(m * p)
    if isinstance(surf, OB.RossLiSurface) and m > 0:
        dc[2] = 0.0             # d/dfiso = 1 has no azimuthal dependence: its moments m > 0 are exactly zero, not the sum's rounding
    ff = 1.0 if m == 0 else 2.0
    N = n * n_stokes
    R, dR = np.zeros((N, N)), np.zeros((K, N, N))
    R[0::n_stokes, 0::n_stokes] = ff * c / math.pi
    dR[:, 0::n_stokes, 0::n_stokes] = ff * dc / math.pi
    return R, dR


def create_surface_layer_brdf_lin(rho_m, drho_m, added: O.AddedLayer, al: OL.AddedLayerLin, isurf, m, pol, qp, tau_sum, tau_sum_dot,
                                  F0, FT):
    """CM.create_surface_layer_brdf_lin (coxmunk_surface_lin.jl:27-102) with K = len(drho_m) surface slots isurf .. isurf + K - 1:
    the forward blocks, the beam-attenuation derivatives of the layer slots [0, tau_sum_dot.shape[1]) and the builder's quirks
    (j0+ = 0, t-- = 0, F0 instead of I0) come from it; slot isurf + k gets ap_r-+ = (f drho_k) diag(mu w) and
    ap_J0- = mu0 (f drho_k) F0_N att."""
    K = len(drho_m)
    CM.create_surface_layer_brdf_lin(rho_m, drho_m[0], added, al, isurf, m, pol, qp, tau_sum, tau_sum_dot, F0, FT)
    S, N = added.j0_p.shape
    n = pol.n
    f = FT(2) if m == 0 else FT(1)
    i0 = n * qp.imu0
    att = np.exp(-np.asarray(tau_sum, dtype=FT) / FT(qp.mu0))
    F0N = np.zeros((S, N), dtype=FT)
    F0N[:, i0:i0 + n] = (np.asarray(F0, dtype=FT) * att[None, :]).T
    sc = (qp.qp_muN.astype(FT) * qp.wt_muN.astype(FT))[None, :]
    for k in range(1, K):
        Rd = (f * drho_m[k]).astype(FT)
        al.ap_J0_m[isurf + k] = FT(qp.mu0) * (F0N @ Rd.T)
        al.ap_r_mp[isurf + k] = (Rd * sc)[None]


def _f0(model):
    S = model.tau_rayl.shape[0]
    F0 = model.F0
    if F0 is None:
        F0 = np.zeros((model.pol.n, S), dtype=model.FT)
        F0[0, :] = 1
    return F0


def rt_run_lin(model: O.RTModel, lin: OL.LinModel, surf, tables=None):
    """rt_run_lin.jl:102-326 over a land BRDF: CM.rt_run_lin's walk with the K-slot surface builder.  P = n_layer_params + K.
    Returns (R, T, Rdot, Tdot): [nVZA, nStokes, S] x 2 and [nVZA, nStokes, S, P] x 2.  tables: m -> (rho_m, drho_m[K]) to use
    instead of reflectance_and_deriv."""
    FT = model.FT
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    nV = len(model.vza)
    pl, K = lin.n_layer_params, n_params(surf)
    P = pl + K
    R, T = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    Rd, Td = np.zeros((nV, pol.n, S, P), dtype=FT), np.zeros((nV, pol.n, S, P), dtype=FT)
    F0 = _f0(model)
    added, added_s, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    al, als, cl = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S), OL.make_composite_layer_lin(FT, P, N, S)
    mu = qp.qp_mu.astype(np.float64)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = OL.layer_optics_lin(model, lin, lods)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT)
        tsd = np.zeros((S, pl, L + 1))
        for iz in range(L):
            tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
        for iz in range(L):
            lo = O.expand_optical_properties(lods[iz], FT)
            dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics)
            expk = np.exp(-dtau / FT(qp.mu0)).astype(FT)
            OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m,
                             nd, qp, added, al, FT)
            dall = np.zeros((S, P), dtype=FT)
            dall[:, :pl] = lins[iz].tau_dot / FT(2 ** nd)
            OL.doubling_lin(pol, expk, nd, added, al, dall, qp.mu0, pl, FT)
            if iz == 0:
                O.copy_added_to_composite(comp, added)
                for a, b in ((cl.T_pp, al.ap_t_pp), (cl.T_mm, al.ap_t_mm), (cl.R_mp, al.ap_r_mp), (cl.R_pm, al.ap_r_pm),
                             (cl.J0_p, al.ap_J0_p), (cl.J0_m, al.ap_J0_m)):
                    a[...] = b
            else:
                OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
        rho, drho = tables(m) if tables is not None else reflectance_and_deriv(surf, pol.n, mu, m)
        create_surface_layer_brdf_lin(rho, drho, added_s, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
        OL.interaction_lin(ifaces[-1], comp, cl, added_s, als, FT)
        n = pol.n
        for i in range(nV):
            imu = int(np.argmin(np.abs(qp.qp_mu - qp.qp_mu.dtype.type(O.cosd(model.vza[i])))))
            c_, s_ = O.cosd(m * model.vaz[i]), O.sind(m * model.vaz[i])
            w = weight * np.array([c_, c_, s_, s_][:n])
            R[i] += w[:, None] * comp.J0_m[:, imu * n:(imu + 1) * n].T
            T[i] += w[:, None] * comp.J0_p[:, imu * n:(imu + 1) * n].T
            for p in range(P):
                Rd[i, :, :, p] += w[:, None] * cl.J0_m[p][:, imu * n:(imu + 1) * n].T
                Td[i, :, :, p] += w[:, None] * cl.J0_p[p][:, imu * n:(imu + 1) * n].T
    return R, T, Rd, Td


def _tables(model, surf):
    mu = model.quad_points.qp_mu.astype(np.float64)
    return [reflectance_and_deriv(surf, model.pol.n, mu, m) for m in range(model.m_max + 1)]


def assemble_slots(runs, pl):
    """K one-surface-slot results (each a tuple of arrays whose derivative arrays end in P = pl + 1 slots) -> the K-slot result:
    the layer slots of the first run, then the surface slot of each run."""
    out = []
    for arrs in zip(*runs):
        if arrs[0].ndim == 4:
            out.append(np.concatenate([arrs[0][..., :pl]] + [a[..., pl:pl + 1] for a in arrs], axis=-1))
        else:
            out.append(arrs[0])
    return tuple(out)


def rt_run_lin_by_slots(model, lin, surf):
    """rt_run_lin assembled from K runs of CM.rt_run_lin's one-slot walk (the check of the assembly argument)."""
    tabs = _tables(model, surf)
    runs = [rt_run_lin(model, lin, _OneSlot(), tables=lambda m, k=k: (tabs[m][0], tabs[m][1][k:k + 1])) for k in range(n_params(surf))]
    return assemble_slots(runs, lin.n_layer_params)


@dataclasses.dataclass
class _OneSlot:
    only: float = 0.0


def rt_run_ss_lin(model, lin, surf):
    """ss_lin_oracle.rt_run_ss_lin with the K surface slots of `surf` -> (R, T, Rdot, Tdot), P = n_layer_params + K."""
    import ss_lin_oracle as SSL
    tabs = _tables(model, surf)
    runs = [SSL.rt_run_ss_lin(model, lin, surface=lambda m, k=k: (tabs[m][0], tabs[m][1][k])) for k in range(n_params(surf))]
    return assemble_slots(runs, lin.n_layer_params)


def ms_lin_segmented(model, lin, levels, surf):
    """ms_lin_oracle.ms_lin_segmented with the K surface slots of `surf` -> (uw, dw, uw_dot, dw_dot), lists over `levels`."""
    import ms_lin_oracle as MSL
    tabs = _tables(model, surf)
    runs = [MSL.ms_lin_segmented(model, lin, levels, surface=lambda m, k=k: (tabs[m][0], tabs[m][1][k])) for k in range(n_params(surf))]
    pl = lin.n_layer_params
    per_level = [assemble_slots([tuple(r[i][j] for i in range(4)) for r in runs], pl) for j in range(len(levels))]
    return tuple([lv[i] for lv in per_level] for i in range(4))


# ---- the small scene of tests/test_oracle_brdf_lin.py and tests/test_gpu_brdf_lin.py ----------------------------------------------
SURFACES = {"rpv": OB.RPVSurface(0.12, 0.08, 0.75, -0.25), "rossli": OB.RossLiSurface(0.05, 0.03, 0.10)}
GEO = dict(l_trunc=5, sza=40.0, vza=[30.0, 5.0], vaz=[0.0, 60.0])     # 3 Gauss streams + the SZA node + 2 VZAs: N = 6 n_stokes
S_POINTS, N_LAYERS, M_MAX = 4, 3, 3


def scene_arrays(n_stokes: int):
    """(keyword arrays of the model, the gas derivative [S, L], F0 [n_stokes, S]): a Rayleigh column of 3 layers, 4 spectral
    points with differing absorption, one gas slot, and -- with more than one Stokes component -- a beam with a non-zero Q."""
    tau_rayl = np.tile(np.array([0.02, 0.05, 0.08]), (S_POINTS, 1))
    gas = np.array([[0.001], [0.02], [0.15], [0.6]]) * np.array([[0.2, 0.3, 0.5]])
    F0 = np.zeros((n_stokes, S_POINTS))
    F0[0] = 1.0
    if n_stokes > 1:
        F0[1] = 0.2
    return dict(tau_rayl=tau_rayl, tau_abs=gas.copy(), depol=0.0279, m_max=M_MAX), gas.copy(), F0


def oracle_scene(pol: str, FT=np.float64):
    """(oracle model, oracle lin model) of the small scene."""
    kw, gas, F0 = scene_arrays(O.polarization(pol).n)
    om = O.build_model(pol, GEO["l_trunc"], GEO["sza"], list(GEO["vza"]), list(GEO["vaz"]), FT=FT, **kw)
    om.F0 = F0.astype(FT)
    return om, OL.LinModel([gas])


# The finite-difference floor of the TOA Jacobians on the small scene: max over the surface parameters of both surfaces, R and T,
# Stokes_I and Stokes_IQU, of  max |central difference of OB.rt_run - rt_run_lin| / max |rt_run_lin|  at FD_STEP.  Measured by
# tests/test_oracle_brdf_lin.py::test_toa_jacobian_against_central_differences (which asserts it) and reused, times 10, by the
# device's finite-difference test.
# At h = 1e-4 the quotient's truncation term (h^2 / 6 times the third derivative) dominates its rounding (eps |R| / h ~ 1e-12) by
# four decades: the figure is a property of the scene, the same on any machine.  Measured: 2.53e-8 (RPV Theta, R, Stokes_I); the
# other RPV slots 1.59e-8 (k), 8.5e-10 (rho0), 2.1e-11 (rho_c); Ross-Li 2.2e-10 at most.
FD_STEP = 1e-4
FD_FLOOR = 2.6e-8
