"""Test oracle of the thermal slot of the linearized multi-sensor run (vsm.CoreRTLin.rt_run_multisensor with a ThermalEmission
source, core_rt_ms_lin.py), built on oracle/vsm_oracle*.py and tests/ms_oracle.py, ms_lin_oracle.py,
ms_thermal_oracle.py and thermal_lin_oracle.py, which it imports and does not change.

The reference has no such run.  This is the device algorithm in numpy: the segmented walk of ms_lin_oracle.ms_lin_segmented on the
linearized THERMAL layers of thermal_lin_oracle (elemental! (lin) with F0 = 0, contribute! and its derivatives, doubling! (lin)
with expk = 1, the surface layers without their beam terms), m = 0 only, with the derivative of the level equation
(ms_lin_oracle.level_lin_push_through) on the slot's own composites; and, per Planck table B_dot[k], the forward thermal walk of
ms_thermal_oracle cut at the same levels, of which only the source vectors a_k = J0+(top), c_k = J0-(bottom) are kept and solved
on the slot's operators by the source-only formula (level_src_only).  Central differences of ms_thermal_oracle.ms_total_reference
anchor it (tests/test_oracle_multisensor_thermal_lin.py).

ms_thermal_lin_segmented(model, lin, B, B_dot, levels, surface=None, full=None)
    -> the THERMAL part alone, (uw, dw, uw_dot, dw_dot): lists in the order of `levels`, [nVZA, nStokes, S] and
       [nVZA, nStokes, S, P + nPlanck].  surface as thermal_lin_oracle.rt_run_thermal_lin takes it.
ms_thermal_lin_total(model, lin, B, B_dot, levels, solar=True, **solar_kw)
    -> the run's total: ms_lin_oracle.ms_lin_segmented (solar=False: at F0 = 0, where the linearized surface builders carry no beam
       term) plus the thermal part, the Planck slots appended.
level_src_only(FT, A, B, a, c)
    the kernel's formula for a source-only slot: dw' = (I - A B)^-1 (a + A c), uw' = c + B dw'.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import ms_lin_oracle as MSL
import ms_oracle as MSO
import ms_thermal_oracle as MST
import thermal_lin_oracle as TL
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL


def level_src_only(FT, A, B, a, c):
    """(uw', dw') of source-only slots: A [S, N, N], B [S | 1, N, N], a / c [K, S, N]."""
    N = A.shape[-1]
    B = np.broadcast_to(B, A.shape)
    M = np.eye(N, dtype=FT)[None] - A @ B
    r = a + np.einsum("sij,ksj->ksi", A, c)
    dwd = np.stack([np.linalg.solve(M, r[k][..., None])[..., 0] for k in range(r.shape[0])]).astype(FT)
    uwd = (c + np.einsum("sij,ksj->ksi", B, dwd)).astype(FT)
    return uwd, dwd


def planck_sources(model, Bk, levels, added_s=None):
    """The forward thermal slot of B := Bk cut at the levels (ms_thermal_oracle.ms_thermal_segmented's walk): {l: (a, c)} with
    a = J0+ of the top, c = J0- of the bottom ([S, N]; level Nz: c = 0), and (J0-, J0+) of the whole column for level 0.
    added_s: the slot's forward surface layer (None: the model's Lambertian one)."""
    levels, Nz, FT, pol, S, L, N, Bk, lods, ifaces, tau_sum_all, _ = MST._begin(model, Bk, levels)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    added = O.make_added_layer(FT, N, S)
    if added_s is None:
        added_s = O.make_added_layer(FT, N, S)
        MST._thermal_surface(model, added_s, tau_sum_all[:, -1])
    layers, comp, a_top = [], None, {}
    for iz in range(L):
        MST._thermal_layer_step(model, lods, tau_sum_all, iz, Bk, added)
        layers.append(MSO._copy_added(added))
        if iz == 0:
            comp = MSO._copy_added(added)
        else:
            O.interaction(ifaces[iz], comp, added, FT)
        if iz + 1 in interior or iz + 1 == Nz:
            a_top[iz + 1] = comp.J0_p.copy()
    res = {}
    if Nz in distinct:
        res[Nz] = (a_top[Nz], np.zeros((S, N), dtype=FT))
    bot = None
    for l, end in reversed(list(zip(interior, interior[1:] + [Nz]))):
        seg = MSO._copy_added(MSO._as_added(layers[l]))
        for iz in range(l + 1, end):
            O.interaction(ifaces[iz], seg, MSO._as_added(layers[iz]), FT)
        if bot is None:
            O.interaction(ifaces[-1], seg, added_s, FT)
        else:
            O.interaction("11", seg, MSO._as_added(bot), FT)
        bot = seg
        res[l] = (a_top[l], bot.J0_m.copy())
    O.interaction(ifaces[-1], comp, added_s, FT)
    res[0] = (comp.J0_m.copy(), comp.J0_p.copy())
    return res


def ms_thermal_lin_segmented(model, lin, B, B_dot, levels, surface=None, full=None):
    """The thermal part of the linearized multi-sensor run (see the module docstring).  full: a dict that receives
    {(level, 0): (uw [S, N], dw [S, N], uw_dot [P + nPlanck, S, N], dw_dot [P + nPlanck, S, N])}."""
    levels, Nz = MSO._check_levels(model, levels)
    FT, DT, pol, qp, S, L, N, _ = MSO._setup(model)
    nV = len(model.vza)
    pl = lin.n_layer_params
    K, build_surface = TL._lambertian(model) if surface is None else surface
    P = pl + K
    B = np.asarray(B, dtype=FT)
    nPl = 0 if B_dot is None else len(B_dot)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    F0 = np.zeros((pol.n, S), dtype=FT)                   # no beam in this slot
    added, added_s = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    al, als = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S)
    m, weight = 0, FT(0.5 / math.pi)
    lods = O.construct_core_optical_properties(model, m)
    lins = OL.layer_optics_lin(model, lin, lods, m)
    ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
    tsd = np.zeros((S, pl, L + 1))
    for iz in range(L):
        tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
    layers, tops = [], {}
    comp, cl = O.make_composite_layer(FT, N, S), OL.make_composite_layer_lin(FT, P, N, S)
    for iz in range(L):                                   # 1. the top pass (TL.rt_run_thermal_lin's walk)
        lo = O.expand_optical_properties(lods[iz], FT)
        if not np.max(lo.tau.astype(DT) * lo.varpi.astype(DT)) > 2 * O.eps(DT):
            raise NotImplementedError("non-scattering layer %d" % (iz + 1))
        dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
        OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd, qp,
                         added, al, FT, DT)
        if iz < B.shape[0]:
            j, jd = TL.thermal_source_lin(pol, qp, dtau, lo.varpi, B[iz], lins[iz].tau_dot / FT(2 ** nd), lins[iz].varpi_dot, FT, DT)
            added.j0_p[...], added.j0_m[...] = j, j
            al.ap_J0_p[:pl], al.ap_J0_m[:pl] = jd, jd
        OL.doubling_lin(pol, np.ones(S, dtype=FT), nd, added, al, np.zeros((S, P), dtype=FT), qp.mu0, pl, FT)
        layers.append((MSO._copy_added(added), MSL._copy_lin(al)))
        if iz == 0:
            O.copy_added_to_composite(comp, added)
            for a, b in ((cl.T_pp, al.ap_t_pp), (cl.T_mm, al.ap_t_mm), (cl.R_mp, al.ap_r_mp), (cl.R_pm, al.ap_r_pm),
                         (cl.J0_p, al.ap_J0_p), (cl.J0_m, al.ap_J0_m)):
                a[...] = b
        else:
            OL.interaction_lin(ifaces[iz], comp, cl, added, al, FT)
        if iz + 1 in interior or iz + 1 == Nz:
            tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy(), cl.R_pm.copy(), cl.J0_p.copy())
    build_surface(added_s, als, pl, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
    for arr in (added_s.j0_p, added_s.j0_m, als.ap_J0_p, als.ap_J0_m):
        arr[...] = 0
    ops, res = {}, {}
    if Nz in distinct:                                    # level Nz: the surface layer alone below (c = 0, c' = 0)
        A, a, Ad, ad = tops[Nz]
        ops[Nz] = (A, added_s.r_mp.copy())
        res[Nz] = MSL.level_lin_push_through(FT, A, a, added_s.r_mp, added_s.j0_m, Ad, ad, als.ap_r_mp, als.ap_J0_m)
    bot = None
    for l, end in reversed(list(zip(interior, interior[1:] + [Nz]))):   # 2./3. segments and bottoms from the surface up
        seg = O.CompositeLayer(*[x.copy() for x in (layers[l][0].R_mp, layers[l][0].R_pm, layers[l][0].T_pp, layers[l][0].T_mm,
                                                     layers[l][0].J0_p, layers[l][0].J0_m)])
        segl = MSL._copy_comp_lin(layers[l][1])
        for iz in range(l + 1, end):
            OL.interaction_lin(ifaces[iz], seg, segl, MSO._as_added(layers[iz][0]), MSL._as_added_lin(layers[iz][1]), FT)
        if bot is None:
            OL.interaction_lin(ifaces[-1], seg, segl, added_s, als, FT)
        else:
            OL.interaction_lin("11", seg, segl, MSO._as_added(bot[0]), MSL._as_added_lin(bot[1]), FT)
        bot = (seg, segl)
        A, a, Ad, ad = tops[l]
        ops[l] = (A, seg.R_mp.copy())
        res[l] = MSL.level_lin_push_through(FT, A, a, seg.R_mp, seg.J0_m, Ad, ad, segl.R_mp, segl.J0_m)   # 4. the level equation
    OL.interaction_lin(ifaces[-1], comp, cl, added_s, als, FT)
    res[0] = (comp.J0_m.copy(), comp.J0_p.copy(), cl.J0_m.copy(), cl.J0_p.copy())
    if nPl:                                               # the Planck slots: source vectors of the forward walks, the slot's operators
        srcs = [planck_sources(model, B_dot[k], levels, None if surface is None else added_s) for k in range(nPl)]
        for l in distinct:
            if l == 0:
                ud, dd = np.stack([s_[0][0] for s_ in srcs]), np.stack([s_[0][1] for s_ in srcs])
            else:
                ud, dd = level_src_only(FT, ops[l][0], ops[l][1], np.stack([s_[l][0] for s_ in srcs]),
                                        np.stack([s_[l][1] for s_ in srcs]))
            uw, dw, uwd, dwd = res[l]
            res[l] = (uw, dw, np.concatenate([uwd, ud]), np.concatenate([dwd, dd]))
    out = {l: (np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S, P + nPl), dtype=FT),
               np.zeros((nV, pol.n, S, P + nPl), dtype=FT)) for l in distinct}
    for l in distinct:
        if full is not None:
            full[(l, 0)] = res[l]
        uw, dw, uwd, dwd = res[l]
        MSO._vza_rows(model, m, weight, uw, dw, out[l][0], out[l][1])
        MSL._vza_rows_lin(model, m, weight, uwd, dwd, out[l][2], out[l][3])
    return tuple([out[l][i].copy() for l in levels] for i in range(4))


def ms_thermal_lin_total(model, lin, B, B_dot, levels, solar=True, surface=None, solar_surface=None, full=None):
    """Solar + thermal: ms_lin_oracle.ms_lin_segmented (solar=False: the same walk at F0 = 0) plus the thermal part; the Planck
    slots, which the solar part does not have, are the thermal part's alone.  surface / solar_surface: the two oracles' own
    `surface` arguments for the same surface.  full: {(level, m): (uw, dw, uw_dot, dw_dot)}, the Planck slots zero for m > 0."""
    ms = model if solar else dataclasses.replace(model, F0=np.zeros((model.pol.n, model.tau_rayl.shape[0]), dtype=model.FT))
    fs, ft = ({}, {}) if full is not None else (None, None)
    sol = MSL.ms_lin_segmented(ms, lin, levels, surface=solar_surface, full=fs)
    th = ms_thermal_lin_segmented(model, lin, B, B_dot, levels, surface=surface, full=ft)
    nPl = 0 if B_dot is None else len(B_dot)
    pad = lambda x, ax: np.concatenate([x, np.zeros(x.shape[:ax] + (nPl,) + x.shape[ax + 1:], dtype=x.dtype)], axis=ax)
    if full is not None:
        for (l, m), (u, d, ud, dd) in fs.items():
            ud, dd = pad(ud, 0), pad(dd, 0)
            if m == 0:
                tu, td, tud, tdd = ft[(l, 0)]
                u, d, ud, dd = u + tu, d + td, ud + tud, dd + tdd
            full[(l, m)] = (u, d, ud, dd)
    return ([a + b for a, b in zip(sol[0], th[0])], [a + b for a, b in zip(sol[1], th[1])],
            [pad(a, 3) + b for a, b in zip(sol[2], th[2])], [pad(a, 3) + b for a, b in zip(sol[3], th[3])])
