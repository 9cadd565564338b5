"""Test oracle of the linearized flux run (vsm.CoreRTLin.rt_run_fluxes, core_rt_flux_lin.py), built on tests/flux_oracle.py,
tests/ms_lin_oracle.py and tests/ms_thermal_lin_oracle.py, which it imports and does not change.

fluxes_lin(model, lin, levels, B=None, B_dot=None, solar=True, ...)
    the quantities of CoreRTLin.rt_run_fluxes in float64: the fields of flux_oracle.fluxes_from_vectors from the forward level
    vectors of the linearized multi-sensor oracle (ms_lin_oracle.ms_lin_segmented(full=...); with thermal emission
    ms_thermal_lin_oracle.ms_thermal_lin_total) at m = 0, and per field `<name>_dot` [nLevels, S, P (+ nPlanck)], the same
    quadratures of the derivative level vectors, plus the analytic derivative of the direct beam
        d/dx_p [mu0 F0 exp(-tau_sum / mu0)] = -F0 exp(-tau_sum / mu0) d tau_sum / dx_p        (layer slots; 0 for the others)
    with d tau_sum / dx_p summed from the oracle's own layer derivatives (vsm_oracle_lin.layer_optics_lin: tau_dot of the delta-M
    scaled layers, what ms_lin_segmented feeds its layers as tau_sum_dot).

Level 0 follows flux_oracle: uw = J0- of the whole column, nothing diffuse goes down, so the down terms and their derivatives are 0.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import flux_oracle as FO
import ms_lin_oracle as MSL
import ms_thermal_lin_oracle as MTL
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL

DOT_FIELDS = tuple(k + "_dot" for k in FO.FIELDS)


def tau_sum_dot_levels(model, lin):
    """[S, pl, Nz + 1]: d tau_sum(level l) / d x_p for the layer slots."""
    m0 = dataclasses.replace(model, m_max=0)
    lods = O.construct_core_optical_properties(m0, 0)
    lins = OL.layer_optics_lin(m0, lin, lods, 0)
    S, L = model.tau_rayl.shape
    tsd = np.zeros((S, lin.n_layer_params, L + 1))
    for iz in range(L):
        tsd[:, :, iz + 1] = tsd[:, :, iz] + np.asarray(lins[iz].tau_dot, dtype=np.float64)
    return tsd


def level_vectors_lin(model, lin, levels, B=None, B_dot=None, solar=True, surface=None, solar_surface=None):
    """{level: (uw, dw [S, N], uw_dot, dw_dot [Pa, S, N])} float64, m = 0, summed over the solar and the thermal slot."""
    m0 = dataclasses.replace(model, m_max=0)
    distinct = sorted(set(int(l) for l in levels))
    full = {}
    if B is None:
        ms = m0 if solar else dataclasses.replace(m0, F0=np.zeros((model.pol.n, model.tau_rayl.shape[0]), dtype=model.FT))
        MSL.ms_lin_segmented(ms, lin, distinct, surface=solar_surface, full=full)
    else:
        MTL.ms_thermal_lin_total(m0, lin, B, B_dot, distinct, solar=solar, surface=surface, solar_surface=solar_surface, full=full)
    return {l: tuple(np.asarray(v, dtype=np.float64) for v in full[(l, 0)]) for l in distinct}


def fluxes_lin_from_vectors(model, lin, levels, vec, solar=True):
    """The fields of CoreRTLin.rt_run_fluxes from {level: (uw, dw, uw_dot, dw_dot)}."""
    levels = [int(l) for l in levels]
    res = FO.fluxes_from_vectors(model, levels, {l: v[:2] for l, v in vec.items()}, solar)
    qp = model.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    mu0 = float(qp.mu0)
    S = model.tau_rayl.shape[0]
    tsd = tau_sum_dot_levels(model, lin)
    pl = tsd.shape[1]
    n = model.pol.n
    rows = {k: [] for k in DOT_FIELDS}
    for i, l in enumerate(levels):
        uwd, dwd = vec[l][2], vec[l][3]
        Pa = uwd.shape[0]
        if l == 0:
            dwd = np.zeros_like(dwd)
        quad = lambda v, wts: (v[:, :, ::n] @ wts).T                       # [Pa, S, N] -> [S, Pa]
        beam_dot = np.zeros((S, Pa))
        beam_dot[:, :pl] = -res.actinic_direct[i][:, None] * tsd[:, :, l] / mu0
        rows["up_dot"].append(quad(uwd, mu * w))
        rows["down_diffuse_dot"].append(quad(dwd, mu * w))
        rows["down_direct_dot"].append(mu0 * beam_dot)
        rows["actinic_up_dot"].append(quad(uwd, w))
        rows["actinic_down_diffuse_dot"].append(quad(dwd, w))
        rows["actinic_direct_dot"].append(beam_dot)
        rows["net_down_dot"].append(rows["down_direct_dot"][-1] + rows["down_diffuse_dot"][-1] - rows["up_dot"][-1])
    for k, v in rows.items():
        setattr(res, k, np.array(v))
    Nz = model.tau_rayl.shape[1]
    res.absorbed_dot = res.surface_absorbed_dot = None
    if sorted(set(levels)) == list(range(Nz + 1)):
        net = np.array([res.net_down_dot[levels.index(l)] for l in range(Nz + 1)])
        res.absorbed_dot, res.surface_absorbed_dot = net[:-1] - net[1:], net[-1].copy()
    return res


def fluxes_lin(model, lin, levels, B=None, B_dot=None, solar=True, surface=None, solar_surface=None):
    vec = level_vectors_lin(model, lin, levels, B, B_dot, solar, surface, solar_surface)
    return fluxes_lin_from_vectors(model, lin, levels, vec, solar)
