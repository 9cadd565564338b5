"""Test oracle of the Raman flux run (vsm.CoreRTRaman.rt_run_fluxes), built on tests/ms_raman_oracle.py and tests/flux_oracle.py,
which it imports and does not change.

fluxes_raman_reference(model, rs, levels)  the quantities of CoreRTRaman.rt_run_fluxes in float64 from the `full` level vectors
                                           of the statement-order prototype (ms_raman_oracle.ms_raman_reference), m = 0.
fluxes_raman_segmented(model, rs, levels)  the same from the device algorithm in numpy (ms_raman_segmented).

Convention as in tests/flux_oracle.py, for the elastic (Cabannes) field and, with the inelastic level vectors summed over the
lines, for the `_ie` fields; the direct beam has no inelastic part.  Level 0 is the TOA itself: uw / uwie are J0- / the line sum
of ieJ0- of the whole column, and every diffuse-down term, elastic and inelastic, is 0 there (the prototypes' level-0 dw / dwie
are rt_run's T / ieT, the field at the BOTTOM of the column, and are not used).
"""
from __future__ import annotations

import dataclasses

import numpy as np

import flux_oracle as FO
import ms_raman_oracle as MRO

IE_FIELDS = ("up_ie", "down_diffuse_ie", "actinic_up_ie", "actinic_down_diffuse_ie", "net_down_ie")
FIELDS = FO.FIELDS + IE_FIELDS


def level_vectors(model, rs, levels, fscatt=None, segmented=False, surface=None):
    """{level: (uw, dw, uwie, dwie)} [S, N] float64 of m = 0, the inelastic ones summed over the lines.  surface: the hook of
    ms_raman_oracle (None = the model's Lambertian albedo)."""
    m0 = dataclasses.replace(model, m_max=0)
    distinct = sorted(set(int(l) for l in levels))
    full = {}
    (MRO.ms_raman_segmented if segmented else MRO.ms_raman_reference)(m0, rs, distinct, fscatt=fscatt, full=full, surface=surface)
    return {l: tuple(np.asarray(v, dtype=np.float64) for v in full[(l, 0)]) for l in distinct}


def fluxes_from_vectors(model, levels, vec):
    """The fields of CoreRTRaman.rt_run_fluxes ([nLevels, S] float64, rows in the order of `levels`) from {level: (uw, dw, uwie,
    dwie)}: flux_oracle.fluxes_from_vectors of the elastic pair, and the same quadratures of the inelastic one."""
    res = FO.fluxes_from_vectors(model, levels, {l: v[:2] for l, v in vec.items()})
    qp = model.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    S = model.tau_rayl.shape[0]
    levels = [int(l) for l in levels]
    rows = {k: [] for k in IE_FIELDS}
    for l in levels:
        uwie, dwie = vec[l][2], vec[l][3]
        if l == 0:
            dwie = np.zeros_like(dwie)
        rows["up_ie"].append(FO.quadrature(model, uwie, mu * w))
        rows["down_diffuse_ie"].append(FO.quadrature(model, dwie, mu * w))
        rows["actinic_up_ie"].append(FO.quadrature(model, uwie, w))
        rows["actinic_down_diffuse_ie"].append(FO.quadrature(model, dwie, w))
        rows["net_down_ie"].append(rows["down_diffuse_ie"][-1] - rows["up_ie"][-1])
    for k, v in rows.items():
        setattr(res, k, np.array(v).reshape(len(levels), S))
    Nz = model.tau_rayl.shape[1]
    res.absorbed_ie = res.surface_absorbed_ie = None
    if sorted(set(levels)) == list(range(Nz + 1)):
        net = np.array([res.net_down_ie[levels.index(l)] for l in range(Nz + 1)])
        res.absorbed_ie, res.surface_absorbed_ie = net[:-1] - net[1:], net[-1].copy()
    return res


def fluxes_raman_reference(model, rs, levels, fscatt=None, surface=None):
    return fluxes_from_vectors(model, levels, level_vectors(model, rs, levels, fscatt, surface=surface))


def fluxes_raman_segmented(model, rs, levels, fscatt=None, surface=None):
    return fluxes_from_vectors(model, levels, level_vectors(model, rs, levels, fscatt, segmented=True, surface=surface))
