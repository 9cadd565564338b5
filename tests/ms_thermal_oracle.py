"""Test oracle of the thermal slot of the multi-sensor run (vsm.CoreRT.rt_run_multisensor(..., thermal=True)), built on
oracle/vsm_oracle.py and tests/ms_oracle.py, which it imports and does not change.

ms_thermal_reference(model, B_layer, levels)  the prototype's statement order (ms_oracle.ms_reference: per sensor a top and a
                             bottom composite, interaction_top! / interaction_bot! layer by layer) with the `:thermal` slot's
                             recurrences of O.rt_run_thermal in place of the solar ones: slot reset (elemental! with F0 = 0),
                             O.thermal_source, doubling with expk = 1, the per-source J0 recurrences of the interaction; the
                             surface layer without its beam terms; then interlayer_flux_reference on the thermal vectors.
ms_thermal_segmented(model, B_layer, levels)  the device algorithm in numpy: one top pass that keeps J0+ after each level, one
                             thermal segment composite per interval, thermal bottoms from the surface up, the level equation
                             by the push-through identity.  (The device takes A, B of the level equation from its solar pass;
                             r, t of a layer do not depend on the source, so here the slot's own composites carry the same R.)

Both return the THERMAL part alone (uw, dw: lists of [nVZA, nStokes, nSpec] in the order of `levels`); the total of a run with
SolarBeam + ThermalEmission is ms_oracle.ms_reference(model, levels) plus it.  Thermal emission is isotropic: m = 0 only (every
layer scatters -- non-scattering columns are refused like in ms_oracle -- so the slot is zero on entry to every later moment).
Level conventions as in ms_oracle: level Nz takes the surface layer alone as its bottom (thermal c = 0).

The layer step restates the scatter branch of O.rt_run_thermal, which does not export it.
"""
from __future__ import annotations

import math

import numpy as np

import ms_oracle as MS
from oracle import vsm_oracle as O


def _thermal_layer_step(model, lods, tau_sum_all, iz, B_layer, added):
    """The scatter branch of O.rt_run_thermal for layer iz (0-based), m = 0, statement for statement: elemental! with F0 = 0 (the
    slot reset of rt_kernel.jl:217-221), contribute! (O.thermal_source), doubling! with the slot's own expk = 1."""
    FT, DT = model.FT, O.deciding_type(model)
    pol, qp = model.pol, model.quad_points
    lo = O.expand_optical_properties(lods[iz], FT)
    tau, varpi = lo.tau, lo.varpi
    if not np.max(tau.astype(DT) * varpi.astype(DT)) > 2 * O.eps(DT):
        raise NotImplementedError("non-scattering layer %d" % (iz + 1))
    S, N = added.j0_p.shape
    dtau, nd = O.get_dtau_ndoubl(tau, varpi, qp, FT, model.numerics, DT)
    O.elemental(pol, tau_sum_all[:, iz].astype(FT), dtau, np.zeros((pol.n, S), dtype=FT), varpi, lo.Zpp, lo.Zmp, 0, nd, qp, added,
                FT, DT)
    j = O.thermal_source(pol, qp, dtau, varpi, B_layer[iz], FT, DT) if iz < B_layer.shape[0] else np.zeros((S, N), dtype=FT)
    added.j0_p[...] = j
    added.j0_m[...] = j
    O.doubling(pol, np.ones(S, dtype=FT), nd, added, FT)


def _thermal_surface(model, added_surf, tau_sum):
    """The slot's surface layer: the model's Lambertian layer of m = 0 without its beam terms (O.rt_run_thermal)."""
    MS._surface_fn(model, None)(0, added_surf, tau_sum)
    added_surf.j0_p[...] = 0
    added_surf.j0_m[...] = 0


def _begin(model, B_layer, levels):
    levels, Nz = MS._check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, _ = MS._setup(model)
    B_layer = np.asarray(B_layer, dtype=FT)
    lods = O.construct_core_optical_properties(model, 0)
    ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
    return levels, Nz, FT, pol, S, L, N, B_layer, lods, ifaces, tau_sum_all, FT(0.5 / math.pi)


def ms_thermal_reference(model, B_layer, levels, full=None):
    """The thermal slot of rt_run_test_ms, statement order (see the module docstring).  full: a dict that receives
    {(level, 0): (uw [S, N], dw [S, N])}."""
    levels, Nz, FT, pol, S, L, N, B_layer, lods, ifaces, tau_sum_all, weight = _begin(model, B_layer, levels)
    nV = len(model.vza)
    uwJ = [np.zeros((nV, pol.n, S), dtype=FT) for _ in levels]
    dwJ = [np.zeros((nV, pol.n, S), dtype=FT) for _ in levels]
    added, added_surf = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    top, bot = [None] * len(levels), [None] * len(levels)
    for iz in range(1, L + 1):                           # rt_kernel_multisensor!, iz 1-based
        _thermal_layer_step(model, lods, tau_sum_all, iz - 1, B_layer, added)
        for ims, lev in enumerate(levels):
            if iz == 1:
                if lev == 0:
                    bot[ims] = MS._copy_added(added)
                else:
                    top[ims] = MS._copy_added(added)
            elif lev == 0:
                O.interaction(ifaces[iz - 1], bot[ims], added, FT)           # interaction_bot!
            elif lev == iz - 1:
                bot[ims] = MS._copy_added(added)
            elif lev < iz - 1:
                O.interaction(ifaces[iz - 1], bot[ims], added, FT)           # interaction_bot!
            else:                                                            # lev >= iz
                O.interaction(ifaces[iz - 1], top[ims], added, FT)           # interaction_top!
    _thermal_surface(model, added_surf, tau_sum_all[:, -1])
    for ims, lev in enumerate(levels):
        if lev == Nz:
            bot[ims] = MS._copy_added(added_surf)        # the surface layer alone: nothing emitted below the level
        else:
            O.interaction(ifaces[-1], bot[ims], added_surf, FT)
    for ims, lev in enumerate(levels):
        if lev == 0:
            uw, dw = bot[ims].J0_m.copy(), bot[ims].J0_p.copy()
        else:
            uw, dw = MS.interlayer_flux_reference(FT, top[ims].R_pm, bot[ims].R_mp, top[ims].J0_p, bot[ims].J0_m)
        if full is not None:
            full[(lev, 0)] = (uw, dw)
        MS._vza_rows(model, 0, weight, uw, dw, uwJ[ims], dwJ[ims])
    return uwJ, dwJ


def ms_thermal_segmented(model, B_layer, levels, full=None):
    """The device algorithm for the thermal slot (core_rt_ms.py, thermal=True) in numpy."""
    levels, Nz, FT, pol, S, L, N, B_layer, lods, ifaces, tau_sum_all, weight = _begin(model, B_layer, levels)
    nV = len(model.vza)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    out = {l: (np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)) for l in distinct}
    added, added_surf = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    layers, comp, tops = [], None, {}
    for iz in range(L):                                  # 1. the top pass
        _thermal_layer_step(model, lods, tau_sum_all, iz, B_layer, added)
        layers.append(MS._copy_added(added))
        if iz == 0:
            comp = MS._copy_added(added)
        else:
            O.interaction(ifaces[iz], comp, added, FT)
        if iz + 1 in interior or iz + 1 == Nz:
            tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy())
    _thermal_surface(model, added_surf, tau_sum_all[:, -1])
    res = {}
    if Nz in distinct:                                   # level Nz: the surface layer alone below (c = 0)
        res[Nz] = MS.level_push_through(FT, *tops[Nz], added_surf.r_mp, added_surf.j0_m)
    bot = None
    for l, end in reversed(list(zip(interior, interior[1:] + [Nz]))):    # 2./3. segments and bottoms from the surface up
        seg = MS._copy_added(MS._as_added(layers[l]))
        for iz in range(l + 1, end):
            O.interaction(ifaces[iz], seg, MS._as_added(layers[iz]), FT)
        if bot is None:
            O.interaction(ifaces[-1], seg, added_surf, FT)
        else:
            O.interaction("11", seg, MS._as_added(bot), FT)
        bot = seg
        res[l] = MS.level_push_through(FT, *tops[l], bot.R_mp, bot.J0_m)   # 4. the level equation
    O.interaction(ifaces[-1], comp, added_surf, FT)
    res[0] = (comp.J0_m.copy(), comp.J0_p.copy())
    for l in distinct:
        if full is not None:
            full[(l, 0)] = res[l]
        MS._vza_rows(model, 0, weight, res[l][0], res[l][1], out[l][0], out[l][1])
    return [out[l][0].copy() for l in levels], [out[l][1].copy() for l in levels]


def ms_total_reference(model, B_layer, levels, solar=True):
    """rt_run_multisensor(thermal=True)'s total: the solar slot (ms_oracle.ms_reference; solar=False: the same slot at F0 = 0,
    which over a reflecting Lambertian surface still carries the surface layer's beam term) plus the thermal one."""
    import dataclasses
    ms = model if solar else dataclasses.replace(model, F0=np.zeros((model.pol.n, model.tau_rayl.shape[0]), dtype=model.FT))
    us, ds = MS.ms_reference(ms, levels)
    ut, dt = ms_thermal_reference(model, B_layer, levels)
    return [a + b for a, b in zip(us, ut)], [a + b for a, b in zip(ds, dt)]
