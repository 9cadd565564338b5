"""Test oracle of the Raman multi-sensor run (vsm.CoreRTRaman.rt_run_multisensor), built on oracle/vsm_oracle.py and
oracle/vsm_oracle_raman.py, which it imports and does not change.

ms_raman_reference(model, rs, levels)  the reference's prototype, statement order: rt_run_test_ms(::RRS, sensor_levels, model,
                                       iBand) (src/CoreRT/rt_run_multisensor.jl) with rt_kernel_multisensor!(::RRS)
                                       (CoreKernel/rt_kernel_multisensor.jl:146-283), interaction_top! / interaction_bot!
                                       (CoreKernel/interaction_multisensor.jl:778-893), interaction_helper_ms!(::RRS, ::_11)
                                       (:517-638), postprocessing_vza_ms!(::RRS) (tools/postprocessing_vza_ms.jl:55-118) and
                                       interlayer_flux_helper!(::RRS) (CoreKernel/interlayer_flux.jl:21-77): per sensor a top and
                                       a bottom composite, one interaction per sensor and layer, two inverses and per-line loops
                                       in the level equation.
ms_raman_segmented(model, rs, levels)  the device algorithm in numpy: one top pass (snapshots of R+-, J0+, ieR+-, ieJ0+ after
                                       each interior level), one RS segment composite per interval between levels, bottoms
                                       composed from the surface up, and the level equations by the push-through identity with
                                       the lines summed before ONE solve per recipient point.

Both return (uw, dw, uwie, dwie): lists with one [nVZA, nStokes, nSpec] array per entry of `levels`, uwie / dwie summed over the
Raman lines like postprocessing_vza_ms!(::RRS).  Level conventions as in tests/ms_oracle.py (level Nz: the surface layer alone
below, whose inelastic part is zero).  `surface`: as in tests/ms_oracle.py -- None = the model's Lambertian albedo, else a function
(m, added_surf, tau_sum) that fills the surface AddedLayer of moment m.

interaction_helper_ms!(::RRS, ::_11) vs interaction_helper!(::RRS, ::_11) (interaction_inelastic.jl:319-521), statement by
statement: the same right-hand sides; the prototype updates the composite in place (every right-hand side still reads pre-update
values: ieJ0-, ieR-+ / ieT-- and the elastic J0-, R-+, T-- of pass 1 are not read by pass 2, and each (n1, dn) block reads only its
own old value) where rt_run writes zero-initialised temporaries, so out-of-band (n1, dn) blocks keep their old value instead of
becoming zero -- they are zero anyway, since elemental_inelastic! zeroes them in every added layer.  _ms_interaction_11 below is the
prototype's in-place form.  The _00 / _01 / _10 tags follow rt_run(RRS)'s convention (OR.interaction_inelastic), as the issue
records: upstream names an undefined ieJ1+ in both drivers, and the prototype's _00 zeroes only ieJ0+- where rt_run's zeroes all six.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_raman as OR  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import ms_oracle as MS  # noqa: E402


def _f0(model):
    F0 = model.F0
    if F0 is None:
        F0 = np.zeros((model.pol.n, model.tau_rayl.shape[0]), dtype=model.FT)
        F0[0, :] = 1
    return F0


def _copy_pair(add: O.AddedLayer, ars: OR.AddedLayerRS):
    """copy_added_to_composite_ie!: a fresh (CompositeLayer, CompositeLayerRS) pair from an added layer."""
    c = O.CompositeLayer(add.r_mp.copy(), add.r_pm.copy(), add.t_pp.copy(), add.t_mm.copy(), add.j0_p.copy(), add.j0_m.copy())
    cr = OR.CompositeLayerRS(ars.ier_mp.copy(), ars.ier_pm.copy(), ars.iet_pp.copy(), ars.iet_mm.copy(), ars.ieJ0_p.copy(),
                             ars.ieJ0_m.copy())
    return c, cr


def _as_added_pair(comp: O.CompositeLayer, crs: OR.CompositeLayerRS):
    """A composite handed to the interaction as the LOWER operand (composite-as-added-layer)."""
    return (O.AddedLayer(comp.R_mp, comp.T_pp, comp.R_pm, comp.T_mm, comp.J0_p, comp.J0_m),
            OR.AddedLayerRS(crs.ieR_mp, crs.ieT_pp, crs.ieR_pm, crs.ieT_mm, crs.ieJ0_p, crs.ieJ0_m))


def _layer_step(model, rs, m, lods, ifaces, tau_sum_all, iz, F0, fscatt, added, add_rs):
    """elemental_inelastic! + elemental! + doubling_inelastic! of layer iz (0-based) into (added, add_rs): rt_kernel!(::RRS)'s
    operations without the interaction (scatter hard-wired to true, rt_kernel_multisensor.jl:170)."""
    FT = model.FT
    N, S = added.r_mp.shape[1], added.r_mp.shape[0]
    rs.fscatt_rayl = np.asarray(fscatt[:, iz], dtype=FT)
    lo = O.expand_optical_properties(lods[iz], FT)
    scratch = O.make_composite_layer(FT, N, S)
    scratch_rs = OR.make_composite_layer_rs(FT, len(rs.i_shift), N, S)
    OR.rt_kernel_rrs(rs, model.pol, added, add_rs, scratch, scratch_rs, lo, tau_sum_all[:, iz].astype(FT), m, model.quad_points, 1,
                     F0, FT, model.numerics)


def _ms_interaction_11(rs, comp, crs, add, ars, FT):
    """interaction_helper_ms!(RS_type::RRS, ::ScatteringInterface_11, SFI = true) (interaction_multisensor.jl:517-638), in place and
    in the prototype's statement order."""
    r_mp, r_pm, t_pp, t_mm, j0_p, j0_m = add.r_mp, add.r_pm, add.t_pp, add.t_mm, add.j0_p, add.j0_m
    ier_mp, ier_pm, iet_pp, iet_mm, iej0_p, iej0_m = ars.ier_mp, ars.ier_pm, ars.iet_pp, ars.iet_mm, ars.ieJ0_p, ars.ieJ0_m
    S, N = r_mp.shape[0], r_mp.shape[1]
    I = np.eye(N, dtype=FT)[None]
    mv = O._mv
    tmp_inv = O.batch_inv(I - r_mp @ comp.R_pm).astype(FT)
    T01 = comp.T_mm @ tmp_inv
    for dn, shift in enumerate(rs.i_shift):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        crs.ieJ0_m[dn, n1] = crs.ieJ0_m[dn, n1] + mv(T01[n1], mv(ier_mp[dn, n1], comp.J0_p[n0]) + mv(r_mp[n1], crs.ieJ0_p[dn, n1])
                                                     + iej0_m[dn, n1]) \
            + mv((T01[n1] @ (ier_mp[dn, n1] @ comp.R_pm[n0] + r_mp[n1] @ crs.ieR_pm[dn, n1]) + crs.ieT_mm[dn, n1])
                 @ tmp_inv[n0], j0_m[n0] + mv(r_mp[n0], comp.J0_p[n0]))
    comp.J0_m[...] = comp.J0_m + mv(T01, mv(r_mp, comp.J0_p) + j0_m)
    for dn, shift in enumerate(rs.i_shift):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        Y = T01[n1] @ (ier_mp[dn, n1] @ comp.R_pm[n0] + r_mp[n1] @ crs.ieR_pm[dn, n1]) + crs.ieT_mm[dn, n1]
        crs.ieR_mp[dn, n1] = crs.ieR_mp[dn, n1] + T01[n1] @ (ier_mp[dn, n1] @ comp.T_pp[n0] + r_mp[n1] @ crs.ieT_pp[dn, n1]) \
            + Y @ tmp_inv[n0] @ r_mp[n0] @ comp.T_pp[n0]
        crs.ieT_mm[dn, n1] = T01[n1] @ iet_mm[dn, n1] + Y @ tmp_inv[n0] @ t_mm[n0]
    comp.R_mp[...] = comp.R_mp + T01 @ r_mp @ comp.T_pp
    comp.T_mm[...] = T01 @ t_mm
    tmp_inv = O.batch_inv(I - comp.R_pm @ r_mp).astype(FT)
    T21 = t_pp @ tmp_inv
    for dn, shift in enumerate(rs.i_shift):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        crs.ieJ0_p[dn, n1] = iej0_p[dn, n1] + mv(T21[n1], crs.ieJ0_p[dn, n1] + mv(crs.ieR_pm[dn, n1], j0_m[n0])
                                                 + mv(comp.R_pm[n1], iej0_m[dn, n1])) \
            + mv((T21[n1] @ (crs.ieR_pm[dn, n1] @ r_mp[n0] + comp.R_pm[n1] @ ier_mp[dn, n1]) + iet_pp[dn, n1]) @ tmp_inv[n0],
                 comp.J0_p[n0] + mv(comp.R_pm[n0], j0_m[n0]))
    comp.J0_p[...] = j0_p + mv(T21, comp.J0_p + mv(comp.R_pm, j0_m))
    for dn, shift in enumerate(rs.i_shift):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        Y = T21[n1] @ (crs.ieR_pm[dn, n1] @ r_mp[n0] + comp.R_pm[n1] @ ier_mp[dn, n1]) + iet_pp[dn, n1]
        crs.ieT_pp[dn, n1] = T21[n1] @ crs.ieT_pp[dn, n1] + Y @ tmp_inv[n0] @ comp.T_pp[n0]
        crs.ieR_pm[dn, n1] = ier_pm[dn, n1] + T21[n1] @ (crs.ieR_pm[dn, n1] @ t_mm[n0] + comp.R_pm[n1] @ iet_mm[dn, n1]) \
            + Y @ tmp_inv[n0] @ comp.R_pm[n0] @ t_mm[n0]
    comp.T_pp[...] = T21 @ comp.T_pp
    comp.R_pm[...] = r_pm + T21 @ comp.R_pm @ t_mm


def _ms_interaction(iface, rs, comp, crs, add, ars, FT):
    if iface == "11":
        return _ms_interaction_11(rs, comp, crs, add, ars, FT)
    return OR.interaction_inelastic(iface, rs, comp, crs, add, ars, FT)


def interlayer_flux_rrs_reference(FT, shifts, A, B, a, c, A_ie, B_ie, a_ie, c_ie):
    """interlayer_flux_helper!(::RRS) (interlayer_flux.jl:21-77), statement for statement: two inverses, per-line products.
    A = top R+- [S,N,N], B = bottom R-+ ([S|1,N,N]), a = top J0+, c = bottom J0- [S,N]; A_ie = top ieR+- [K,S,N,N], a_ie = top
    ieJ0+ [K,S,N], B_ie / c_ie = bottom ieR-+ / ieJ0- (None: zero).  Returns (uw, dw [S,N], uwie, dwie [K,S,N])."""
    S, N = a.shape
    K = len(shifts)
    B = np.broadcast_to(B, A.shape)
    if B_ie is None:
        B_ie, c_ie = np.zeros_like(A_ie), np.zeros_like(a_ie)
    I = np.eye(N, dtype=FT)[None]
    mv = O._mv
    dwie, uwie = np.zeros((K, S, N), dtype=FT), np.zeros((K, S, N), dtype=FT)
    tmpR = O.batch_inv(I - A @ B).astype(FT)
    dw = mv(tmpR, a + mv(A, c))
    for dn, shift in enumerate(shifts):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        dwie[dn, n1] = mv(tmpR[n1], a_ie[dn, n1] + mv(A_ie[dn, n1], c[n0]) + mv(A[n1], c_ie[dn, n1])
                          + mv((A[n1] @ B_ie[dn, n1] + A_ie[dn, n1] @ B[n0]) @ tmpR[n0], a[n0] + mv(A[n0], c[n0])))
    tmpR = O.batch_inv(I - B @ A).astype(FT)
    uw = mv(tmpR, c + mv(B, a))
    for dn, shift in enumerate(shifts):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        uwie[dn, n1] = mv(tmpR[n1], c_ie[dn, n1] + mv(B_ie[dn, n1], a[n0]) + mv(B[n1], a_ie[dn, n1])
                          + mv((B[n1] @ A_ie[dn, n1] + B_ie[dn, n1] @ A[n0]) @ tmpR[n0], c[n0] + mv(B[n0], a[n0])))
    return uw, dw, uwie, dwie


def level_ie_push_through(FT, shifts, A, B, dw, uw, A_ie, a_ie, B_ie=None, c_ie=None):
    """The device's inelastic level equation (vsm_level_radiance_ie_*), lines summed before ONE solve per recipient point n1:
        q = sum_k [c_ie,k + B_ie,k dw(n0)],  r = sum_k [a_ie,k + A_ie,k uw(n0)] + A q,  dw_ie = (I - A B)^-1 r,  uw_ie = q + B dw_ie
    over the in-band lines (n0 = n1 + shift[k] in 0..S-1); dw / uw = the ELASTIC level vectors [S,N].  Returns (uwie, dwie) [S,N]."""
    S, N = dw.shape
    B = np.broadcast_to(B, A.shape)
    mv = O._mv
    q, p = np.zeros((S, N), dtype=FT), np.zeros((S, N), dtype=FT)
    for k, shift in enumerate(shifts):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        if B_ie is not None:
            q[n1] += c_ie[k, n1] + mv(B_ie[k, n1], dw[n0])
        p[n1] += a_ie[k, n1] + mv(A_ie[k, n1], uw[n0])
    r = p + mv(A, q)
    M = np.eye(N, dtype=FT)[None] - A @ B
    dwie = np.linalg.solve(M, r[..., None])[..., 0].astype(FT)
    uwie = (q + mv(B, dwie)).astype(FT)
    return uwie, dwie


def _check(model, levels):
    return MS._check_levels(model, levels)


def _setup_rs(model, rs, fscatt):
    FT, pol, qp = model.FT, model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    K = len(rs.i_shift)
    return FT, pol, qp, S, L, N, K, _f0(model), (OR.default_fscatt(model) if fscatt is None else fscatt)


def _surface(model, surface=None):
    """The surface hook (m, added_surf, tau_sum): None = the model's Lambertian albedo (scalar or a per-point spectrum), else
    `surface` itself (e.g. vsm_oracle_coxmunk.surface_layer_hook of a BRDF's Fourier blocks), as in tests/ms_oracle.py."""
    return MS._surface_fn(model, surface)


def ms_raman_reference(model, rs: OR.RRS, levels, fscatt=None, full=None, surface=None):
    """rt_run_test_ms(::RRS, sensor_levels, model, iBand): (uwJ, dwJ, uwieJ, dwieJ) in the order of `levels`, the ie outputs summed
    over the lines.  full: a dict that receives {(level, m): (uw, dw, uwie, dwie)} ([S,N]; ie summed over the lines)."""
    levels, Nz = _check(model, levels)
    FT, pol, qp, S, L, N, K, F0, fscatt = _setup_rs(model, rs, fscatt)
    nV = len(model.vza)
    fill_surface = _surface(model, surface)
    outs = [[np.zeros((nV, pol.n, S), dtype=FT) for _ in levels] for _ in range(4)]
    added, add_rs = O.make_added_layer(FT, N, S), OR.make_added_layer_rs(FT, K, N, S)
    added_surf, surf_rs = O.make_added_layer(FT, N, S), OR.make_added_layer_rs(FT, K, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        rs.Zpp_ie, rs.Zmp_ie = O.compute_Z_moments(pol, qp.qp_mu, rs.greek_raman, m)
        lods = O.construct_core_optical_properties(model, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT)
        top, bot = [None] * len(levels), [None] * len(levels)
        for iz in range(1, L + 1):                       # rt_kernel_multisensor!(::RRS), iz 1-based
            _layer_step(model, rs, m, lods, ifaces, tau_sum_all, iz - 1, F0, fscatt, added, add_rs)
            for ims, lev in enumerate(levels):
                if iz == 1:
                    if lev == 0:
                        bot[ims] = _copy_pair(added, add_rs)
                    else:
                        top[ims] = _copy_pair(added, add_rs)
                elif lev == iz - 1:
                    bot[ims] = _copy_pair(added, add_rs)
                elif lev < iz - 1:
                    _ms_interaction(ifaces[iz - 1], rs, *bot[ims], added, add_rs, FT)    # interaction_bot!
                else:
                    _ms_interaction(ifaces[iz - 1], rs, *top[ims], added, add_rs, FT)    # interaction_top!
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        for ims, lev in enumerate(levels):
            if lev == Nz:
                bot[ims] = _copy_pair(added_surf, surf_rs)                                # the level-Nz deviation
            else:
                _ms_interaction(ifaces[-1], rs, *bot[ims], added_surf, surf_rs, FT)       # interaction_bot! with the surface
        for ims, lev in enumerate(levels):               # postprocessing_vza_ms!(::RRS)
            (bc, br) = bot[ims]
            if lev == 0:
                uw, dw, uwie, dwie = bc.J0_m.copy(), bc.J0_p.copy(), br.ieJ0_m.copy(), br.ieJ0_p.copy()
            else:
                tc, tr = top[ims]
                uw, dw, uwie, dwie = interlayer_flux_rrs_reference(FT, rs.i_shift, tc.R_pm, bc.R_mp, tc.J0_p, bc.J0_m, tr.ieR_pm,
                                                                   br.ieR_mp, tr.ieJ0_p, br.ieJ0_m)
            if full is not None:
                full[(lev, m)] = (uw, dw, uwie.sum(axis=0), dwie.sum(axis=0))
            MS._vza_rows(model, m, weight, uw, dw, outs[0][ims], outs[1][ims])
            for t in range(K):                           # the per-line accumulation of postprocessing_vza_ms.jl:110-113
                MS._vza_rows(model, m, weight, uwie[t], dwie[t], outs[2][ims], outs[3][ims])
    return tuple(outs)


def ms_raman_segmented(model, rs: OR.RRS, levels, fscatt=None, full=None, counts=None, surface=None):
    """The device algorithm (core_rt_ms_raman.py) in numpy: same outputs as ms_raman_reference up to rounding; level 0 is
    OR.rt_run_rrs's (R, T, ieR, ieT) exactly.  counts: a dict that receives the number of layer steps and interactions."""
    levels, Nz = _check(model, levels)
    FT, pol, qp, S, L, N, K, F0, fscatt = _setup_rs(model, rs, fscatt)
    nV = len(model.vza)
    fill_surface = _surface(model, surface)
    distinct = sorted(set(levels))
    interior = [l for l in distinct if 0 < l < Nz]
    out = {l: [np.zeros((nV, pol.n, S), dtype=FT) for _ in range(4)] for l in distinct}
    added, add_rs = O.make_added_layer(FT, N, S), OR.make_added_layer_rs(FT, K, N, S)
    added_surf, surf_rs = O.make_added_layer(FT, N, S), OR.make_added_layer_rs(FT, K, N, S)
    comp, comp_rs = O.make_composite_layer(FT, N, S), OR.make_composite_layer_rs(FT, K, N, S)
    if counts is not None:
        counts.update(layers=0, interactions=0)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        rs.Zpp_ie, rs.Zmp_ie = O.compute_Z_moments(pol, qp.qp_mu, rs.greek_raman, m)
        lods = O.construct_core_optical_properties(model, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT)
        tops = {}
        for iz in range(L):                              # 1. the top pass: rt_run_rrs's walk
            rs.fscatt_rayl = np.asarray(fscatt[:, iz], dtype=FT)
            lo = O.expand_optical_properties(lods[iz], FT)
            OR.rt_kernel_rrs(rs, pol, added, add_rs, comp, comp_rs, lo, tau_sum_all[:, iz].astype(FT), m, qp, iz + 1, F0, FT,
                             model.numerics, None, ifaces[iz])
            if counts is not None:
                counts["layers"] += 1
            if iz + 1 in interior or iz + 1 == Nz:
                tops[iz + 1] = (comp.R_pm.copy(), comp.J0_p.copy(), comp_rs.ieR_pm.copy(), comp_rs.ieJ0_p.copy())
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        res = {}

        def level(l, bc, br):
            A, a, A_ie, a_ie = tops[l]
            uw, dw = MS.level_push_through(FT, A, a, bc.R_mp, bc.J0_m)
            uwie, dwie = level_ie_push_through(FT, rs.i_shift, A, bc.R_mp, dw, uw, A_ie, a_ie,
                                               None if br is None else br.ieR_mp, None if br is None else br.ieJ0_m)
            res[l] = (uw, dw, uwie, dwie)

        if Nz in distinct:                               # level Nz: the surface layer alone below, no inelastic part
            level(Nz, O.CompositeLayer(added_surf.r_mp, None, None, None, None, added_surf.j0_m), None)
        bot = None
        ends = interior[1:] + [Nz]
        for l, end in reversed(list(zip(interior, ends))):   # 2./3. RS segments and bottoms from the surface up
            # a join associates only if every layer below `end` interacts with the _11 statements (see core_rt_ms_raman.py)
            walk = bot is not None and not (all(t == "11" for t in ifaces[end:L]) and ifaces[-1] in ("11", "10"))
            for iz in range(l, L if walk else end):
                _layer_step(model, rs, m, lods, ifaces, tau_sum_all, iz, F0, fscatt, added, add_rs)
                if counts is not None:
                    counts["layers"] += 1
                if iz == l:
                    seg = _copy_pair(added, add_rs)
                else:
                    OR.interaction_inelastic(ifaces[iz], rs, *seg, added, add_rs, FT)
            if bot is None or walk:
                OR.interaction_inelastic(ifaces[-1], rs, *seg, added_surf, surf_rs, FT)
            else:
                OR.interaction_inelastic("11", rs, *seg, *_as_added_pair(*bot), FT)
            if counts is not None:
                counts["interactions"] += 1
            bot = seg
            level(l, *bot)                               # 4. the level equations
        OR.interaction_inelastic(ifaces[-1], rs, comp, comp_rs, added_surf, surf_rs, FT)
        if counts is not None:
            counts["interactions"] += 1
        o0 = out[0] if 0 in distinct else [np.zeros((nV, pol.n, S), dtype=FT) for _ in range(4)]
        OR.postprocessing_vza_rs(pol, comp, comp_rs, model.vza, model.vaz, qp, m, weight, *o0)
        res[0] = (comp.J0_m.copy(), comp.J0_p.copy(), comp_rs.ieJ0_m.sum(axis=0), comp_rs.ieJ0_p.sum(axis=0))
        for l in distinct:
            if full is not None:
                full[(l, m)] = res[l]
            if l != 0:
                uw, dw, uwie, dwie = res[l]
                MS._vza_rows(model, m, weight, uw, dw, out[l][0], out[l][1])
                MS._vza_rows(model, m, weight, uwie, dwie, out[l][2], out[l][3])
    return tuple([out[l][i].copy() for l in levels] for i in range(4))
