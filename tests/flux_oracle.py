"""Test oracle of the flux run (vsm.CoreRT.rt_run_fluxes), built on tests/ms_oracle.py, tests/ms_thermal_oracle.py and
tests/sif_oracle.py, which it imports and does not change.

fluxes_reference(model, levels, ...)  the quantities of rt_run_fluxes in float64 from the level vectors at all streams of the
                             statement-order prototypes (ms_oracle.ms_reference, ms_thermal_oracle.ms_thermal_reference), m = 0.
fluxes_segmented(model, levels, ...)  the same from the device algorithm in numpy (ms_segmented / ms_thermal_segmented).

Convention (the reference's hem_R / hem_T, rt_run.jl:745; ms_oracle.net_flux): with uw / dw the m = 0 level vectors (rows of
Stokes I), mu, w the quadrature nodes and weights, up = sum_i mu_i w_i uw_i and down_diffuse likewise of dw; the actinic terms
without the mu_i; the direct beam mu0 F0[0] exp(-tau_sum(level) / mu0) with the run's own tau_sum (actinic: without the mu0).
Level 0 is the TOA itself: uw is J0- of the whole column, and nothing diffuse enters, so the diffuse down terms are 0 there --
the prototypes' level-0 dw is rt_run's T, the field at the BOTTOM of the column, and is not used.
"""
from __future__ import annotations

import dataclasses
import types

import numpy as np

import ms_oracle as MS
import ms_thermal_oracle as MT
import sif_oracle as SIF
from oracle import vsm_oracle as O

FIELDS = ("up", "down_diffuse", "down_direct", "actinic_up", "actinic_down_diffuse", "actinic_direct", "net_down")


def tau_sum_levels(model):
    """[S, Nz + 1]: the optical depth above level l as the layer kernels see it (delta-M scaled; column Nz = the surface's)."""
    FT, DT = model.FT, O.deciding_type(model)
    _, tau_sum_all = O.extract_effective_props(O.construct_core_optical_properties(model, 0), FT, DT)
    return np.asarray(tau_sum_all, dtype=np.float64)


def level_vectors(model, levels, B_layer=None, solar=True, sif=None, segmented=False, surface=None):
    """{level: (uw, dw)} [S, N] float64, m = 0, summed over the sources: the solar slot (solar=False: the same slot at F0 = 0,
    ms_thermal_oracle.ms_total_reference's rule), SurfaceSIF in its surface layer (sif: the table, [S] or [n, S]), the thermal slot
    (B_layer [Nz, S]).  surface: the hook (m, added_surf, tau_sum) of ms_oracle for the solar slot (None = the model's Lambertian
    albedo); not together with sif or B_layer, whose slots build their own Lambertian surface."""
    if surface is not None and (sif is not None or B_layer is not None):
        raise ValueError("level_vectors: a surface hook goes with the solar slot alone (no sif, no B_layer)")
    m0 = dataclasses.replace(model, m_max=0)
    ms = m0 if solar else dataclasses.replace(m0, F0=np.zeros((model.pol.n, model.tau_rayl.shape[0]), dtype=model.FT))
    if sif is not None:
        tab = SIF.sif_table(model.pol.n, model.tau_rayl.shape[0], sif)

        def surface(m, added_surf, tau_sum):
            SIF._fill_lambertian(ms, added_surf, m, tau_sum)
            SIF.inject(added_surf, tab, m, model.pol.n)
    distinct = sorted(set(int(l) for l in levels))
    full = {}
    (MS.ms_segmented if segmented else MS.ms_reference)(ms, distinct, surface=surface, full=full)
    vec = {l: tuple(np.asarray(v, dtype=np.float64) for v in full[(l, 0)]) for l in distinct}
    if B_layer is not None:
        ft = {}
        (MT.ms_thermal_segmented if segmented else MT.ms_thermal_reference)(m0, B_layer, distinct, full=ft)
        vec = {l: (vec[l][0] + ft[(l, 0)][0], vec[l][1] + ft[(l, 0)][1]) for l in distinct}
    return vec


def quadrature(model, vec, weights):
    """sum_i weights_i vec[:, i n] (the rows of Stokes I), [S]."""
    return np.asarray(vec, dtype=np.float64)[:, ::model.pol.n] @ weights


def fluxes_from_vectors(model, levels, vec, solar=True, level0_dw=False):
    """The fields of rt_run_fluxes ([nLevels, S] float64, rows in the order of `levels`) from {level: (uw, dw)}.  level0_dw: put
    the prototypes' level-0 dw into the formulae instead of 0 -- the WRONG convention, for the tests that show it matters."""
    qp = model.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    mu0 = float(qp.mu0)
    S = model.tau_rayl.shape[0]
    F0 = MS._setup(model)[7]
    F0_I = np.asarray(F0[0], dtype=np.float64) if solar else np.zeros(S)
    ts = tau_sum_levels(model)
    levels = [int(l) for l in levels]
    rows = {k: [] for k in FIELDS}
    for l in levels:
        uw, dw = vec[l]
        if l == 0 and not level0_dw:
            dw = np.zeros_like(dw)
        beam = F0_I * np.exp(-ts[:, l] / mu0)
        rows["up"].append(quadrature(model, uw, mu * w))
        rows["down_diffuse"].append(quadrature(model, dw, mu * w))
        rows["down_direct"].append(mu0 * beam)
        rows["actinic_up"].append(quadrature(model, uw, w))
        rows["actinic_down_diffuse"].append(quadrature(model, dw, w))
        rows["actinic_direct"].append(beam)
        rows["net_down"].append(rows["down_direct"][-1] + rows["down_diffuse"][-1] - rows["up"][-1])
    res = types.SimpleNamespace(levels=levels, **{k: np.array(v).reshape(len(levels), S) for k, v in rows.items()})
    Nz = model.tau_rayl.shape[1]
    res.absorbed = res.surface_absorbed = None
    if sorted(set(levels)) == list(range(Nz + 1)):
        net = np.array([res.net_down[levels.index(l)] for l in range(Nz + 1)])
        res.absorbed, res.surface_absorbed = net[:-1] - net[1:], net[-1].copy()
    return res


def fluxes_reference(model, levels, B_layer=None, solar=True, sif=None, surface=None):
    return fluxes_from_vectors(model, levels, level_vectors(model, levels, B_layer, solar, sif, surface=surface), solar)


def fluxes_segmented(model, levels, B_layer=None, solar=True, sif=None):
    return fluxes_from_vectors(model, levels, level_vectors(model, levels, B_layer, solar, sif, segmented=True), solar)
