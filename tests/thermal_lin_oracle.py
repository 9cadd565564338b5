"""Test oracle of the linearized `:thermal` per-source slot: rt_run_thermal_lin(model, lin_model, B, B_dot) -> the slot's own
(R, T, Rdot, Tdot), which the linearized run adds to its solar ones.  numpy only; built on oracle/vsm_oracle.py (thermal_source,
rt_run_thermal), oracle/vsm_oracle_lin.py and, for BRDF surfaces, tests/brdf_lin_oracle.py, which it imports and does not change.

The reference linearizes no thermal source (rt_helper_functions_lin.jl:70), so there is nothing to restate: the slot is
O.rt_run_thermal's walk (elemental! with F0 = 0, contribute!, doubling! with the slot's expk = 1, interaction!, the surface layer
without its beam terms) with the derivative stacks of OL beside it, and is pinned by central differences of O.rt_run_thermal
(tests/test_oracle_thermal_lin.py).  The one new formula is the derivative of the elemental source: with x = dtau / mu_i on the
Stokes-I rows,

    j0+ = j0- = 2 pi (1 - varpi) B (1 - e^-x)
    d/dp      = 2 pi B [ -varpi_dot_p (1 - e^-x) + (1 - varpi) e^-x dtau_dot_p / mu_i ]

expk = 1 has no parameter derivative, so doubling! (lin) runs with a zero dtau_dot table (ek_lin = 0).  Every layer is taken as
scattering, like OL.rt_run_lin does (rt_kernel_lin.jl:87); columns with a non-scattering layer are outside the slot's scope.

The slot is linear in B: the Planck slot k, appended after the surface slots, is the forward slot of B := B_dot[k].
"""
from __future__ import annotations

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
from oracle import vsm_oracle_lin as OL  # noqa: E402


def thermal_source_lin(pol, qp, dtau, varpi, B, dtau_dot, varpi_dot, FT, DT=None):
    """(j [S, N], jdot [p, S, N]): O.thermal_source and its derivatives.  dtau_dot [S, p] = tau_dot / 2^ndoubl, varpi_dot [S, p]."""
    DT = FT if DT is None else DT
    j = O.thermal_source(pol, qp, dtau, varpi, B, FT, DT)
    mu = qp.qp_mu.astype(FT)
    n = pol.n
    d, w, b = (np.asarray(x, dtype=FT) for x in (dtau, varpi, B))
    td, wd = np.asarray(dtau_dot, dtype=FT), np.asarray(varpi_dot, dtype=FT)
    p = td.shape[1]
    jd = np.zeros((p,) + j.shape, dtype=FT)
    two_pi = FT(2 * math.pi)
    for i, mi in enumerate(mu):
        if mi > O.eps(DT):
            em1 = -np.expm1(-d / mi)                       # 1 - e^-x
            ex = np.exp(-d / mi)
            jd[:, :, i * n] = ((two_pi * b)[:, None] * (-wd * em1[:, None] + ((FT(1) - w) * ex / mi)[:, None] * td)).T
    return j, jd


def _lambertian(model):
    def build(added_s, als, isurf, m, pol, qp, tau_sum, tsd, F0, FT):
        OL.create_surface_layer_lambertian_lin(model.albedo, added_s, als, isurf, m, pol, qp, tau_sum, tsd, F0, FT)
    return 1, build


def brdf_surface(K, tables):
    """The `surface` argument for a BRDF surface with K parameter slots; tables: m -> (rho_m [N, N], drho_m [K, N, N])."""
    import brdf_lin_oracle as BL

    def build(added_s, als, isurf, m, pol, qp, tau_sum, tsd, F0, FT):
        rho, drho = tables(m)
        BL.create_surface_layer_brdf_lin(rho, drho, added_s, als, isurf, m, pol, qp, tau_sum, tsd, F0, FT)
    return K, build


def rt_run_thermal_lin(model: O.RTModel, lin: OL.LinModel, B, B_dot=None, surface=None):
    """The thermal slot alone -> (R, T, Rdot, Tdot): [nVZA, nStokes, S] x 2 and [nVZA, nStokes, S, P + nPlanck] x 2, with
    P = n_layer_params + K.  B [rows, S]; B_dot None or [nPlanck, rows, S]; surface: None = the model's Lambertian albedo
    (K = 1), or brdf_surface(K, tables)."""
    FT, DT = model.FT, O.deciding_type(model)
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    nV = len(model.vza)
    pl = lin.n_layer_params
    K, build_surface = _lambertian(model) if surface is None else surface
    P = pl + K
    B = np.asarray(B, dtype=FT)
    nPl = 0 if B_dot is None else len(B_dot)
    R, T = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    Rd, Td = np.zeros((nV, pol.n, S, P + nPl), dtype=FT), np.zeros((nV, pol.n, S, P + nPl), dtype=FT)
    F0 = np.zeros((pol.n, S), dtype=FT)                                # no beam in this slot
    added, added_s, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    al, als, cl = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S), OL.make_composite_layer_lin(FT, P, N, S)
    m = 0                                                              # thermal emission is isotropic
    weight = FT(0.5 / math.pi)
    lods = O.construct_core_optical_properties(model, m)
    lins = OL.layer_optics_lin(model, lin, lods, m)
    ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
    tsd = np.zeros((S, pl, L + 1))
    for iz in range(L):
        tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
    for iz in range(L):
        lo = O.expand_optical_properties(lods[iz], FT)
        dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
        OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd, qp,
                         added, al, FT, DT)                            # F0 = 0: j and jdot are reset
        if iz < B.shape[0]:
            j, jd = thermal_source_lin(pol, qp, dtau, lo.varpi, B[iz], lins[iz].tau_dot / FT(2 ** nd), lins[iz].varpi_dot, FT, DT)
            added.j0_p[...], added.j0_m[...] = j, j
            al.ap_J0_p[:pl], al.ap_J0_m[:pl] = jd, jd
        OL.doubling_lin(pol, np.ones(S, dtype=FT), nd, added, al, np.zeros((S, P), dtype=FT), qp.mu0, pl, FT)
        if iz == 0:
            O.copy_added_to_composite(comp, added)
            for a, b in ((cl.T_pp, al.ap_t_pp), (cl.T_mm, al.ap_t_mm), (cl.R_mp, al.ap_r_mp), (cl.R_pm, al.ap_r_pm),
                         (cl.J0_p, al.ap_J0_p), (cl.J0_m, al.ap_J0_m)):
                a[...] = b
        else:
            OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
    build_surface(added_s, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
    for arr in (added_s.j0_p, added_s.j0_m, als.ap_J0_p, als.ap_J0_m):   # no solar beam in this slot
        arr[...] = 0
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
    for k in range(nPl):                                               # linear in B: the forward slot of B_dot[k]
        Rk, Tk, _, _ = rt_run_thermal_lin(model, lin, B_dot[k], None, surface)
        Rd[..., P + k], Td[..., P + k] = Rk, Tk
    return R, T, Rd, Td
