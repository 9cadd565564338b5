"""Test oracle of the SurfaceSIF source (vsm.host_model.SurfaceSIF), built on the blocks of oracle/ and of tests/ms_oracle.py,
which it imports and does not change.

The source (src/CoreRT/Sources/surface_sif.jl:168-179, the same statement as inject_surface_SIF!, Surfaces/lambertian_surface.jl:
239-254): hemispheric isotropic emission at the lower boundary, applied after create_surface_layer! and before the surface
interaction!, at Fourier moment m = 0, over Lambertian surfaces only:

    j0-_surface[i n + c, s] += 2 SIF0[c, s]        for every stream i and Stokes component c

rt_run_sif          rt_run with the source: the loop of O.rt_run (rt_run.jl:454-455)
ms_sif              the multi-sensor run, through the `surface=` hook of ms_oracle.ms_reference (rt_run_multisensor.jl:140)
rt_run_rrs_sif      the rotational-Raman run, from the blocks of vsm_oracle_raman (rt_run.jl:711-712)
rt_run_lin_sif      the linearized run (rt_run_lin.jl:292) from the blocks of vsm_oracle_lin, with the SIF slots: the radiance is
                    linear in SIF0 and the emission is the same at every stream, so d/dx_k = sum_c 2 SIF0_dot[k, c, s] G_c(s)
unit_response       G_c: the response to a unit emission in Stokes component c, by a direct solve of (I - r-+ R+-) y = e_c
"""
from __future__ import annotations

import math

import numpy as np

import ms_oracle as MS
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL
from oracle import vsm_oracle_raman as OR


def sif_table(n: int, S: int, SIF0) -> np.ndarray:
    """[S] (Stokes I only) or [n, S] -> [n, S]."""
    SIF0 = np.asarray(SIF0, dtype=np.float64)
    if SIF0.ndim == 1:
        out = np.zeros((n, S))
        out[0] = SIF0
        return out
    assert SIF0.shape == (n, S), SIF0.shape
    return SIF0


def inject(added_surf: O.AddedLayer, sif, m: int, n: int, lambertian: bool = True):
    """contribute!(::SurfaceSIF): j0- += 2 SIF0 on the rows of every stream; no-op for m > 0, over a non-Lambertian surface and
    for an all-zero table (which adds nothing)."""
    if m != 0 or not lambertian or not np.any(sif != 0):
        return
    FT = added_surf.j0_m.dtype
    for c in range(n):
        added_surf.j0_m[:, c::n] += (FT.type(2) * sif[c].astype(FT))[:, None]


def _F0(model):
    FT, pol, S = model.FT, model.pol, model.tau_rayl.shape[0]
    F0 = model.F0
    if F0 is None:
        F0 = np.zeros((pol.n, S), dtype=FT)
        F0[0, :] = 1
    return F0


def _fill_lambertian(model, added_surf, m, tau_sum):
    FT, pol, qp = model.FT, model.pol, model.quad_points
    if np.ndim(model.albedo) == 1:
        O.create_surface_layer_lambertian_spectral(model.albedo, added_surf, m, pol, qp, tau_sum, FT)
    else:
        O.create_surface_layer_lambertian(model.albedo, added_surf, m, pol, qp, tau_sum, FT)


def rt_run_sif(model: O.RTModel, SIF0, per_m=None, hdrf=None, surface_layers=None):
    """O.rt_run (rt_run.jl:238-539) with the injection between the surface layer and its interaction.  hdrf: as O.rt_run.
    surface_layers: a list that receives, per moment, a copy of the surface layer's (j0-, r-+) after the injection."""
    FT, DT = model.FT, O.deciding_type(model)
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    nV = len(model.vza)
    sif = sif_table(pol.n, S, SIF0)
    R_SFI, T_SFI = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    F0 = _F0(model)
    added, added_surf, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        for iz in range(L):
            lo = O.expand_optical_properties(lods[iz], FT)
            O.rt_kernel(pol, added, comp, lo, ifaces[iz], tau_sum_all[:, iz].astype(FT), m, qp, iz + 1, F0, FT, model.numerics, None, DT)
        _fill_lambertian(model, added_surf, m, tau_sum_all[:, -1])
        inject(added_surf, sif, m, pol.n)
        if surface_layers is not None:
            surface_layers.append((added_surf.j0_m.copy(), added_surf.r_mp.copy()))
        O.interaction(ifaces[-1], comp, added_surf, FT)
        if per_m is not None:
            per_m.append(dict(m=m, J0_m=comp.J0_m.copy(), J0_p=comp.J0_p.copy(), weight=weight))
        if hdrf is not None:
            if m == 0:
                hdrf.update(hdr=np.zeros((nV, pol.n, S), dtype=FT), bhr_uw=np.zeros((pol.n, S), dtype=FT),
                            bhr_dw=np.zeros((pol.n, S), dtype=FT))
            hj = O.interaction_hdrf(comp, added_surf, m, pol, qp, hdrf["bhr_uw"], hdrf["bhr_dw"])
            hc = O.CompositeLayer(None, None, None, None, np.zeros_like(hj), hj)
            O.postprocessing_vza(pol, hc, model.vza, model.vaz, qp, m, weight, hdrf["hdr"], np.zeros_like(hdrf["hdr"]))
        O.postprocessing_vza(pol, comp, model.vza, model.vaz, qp, m, weight, R_SFI, T_SFI)
    return R_SFI, T_SFI


def ms_sif(model: O.RTModel, levels, SIF0):
    """ms_oracle.ms_reference with the emission in the surface layer every bottom composite is built from."""
    sif = sif_table(model.pol.n, model.tau_rayl.shape[0], SIF0)

    def fill(m, added_surf, tau_sum):
        _fill_lambertian(model, added_surf, m, tau_sum)
        inject(added_surf, sif, m, model.pol.n)
    return MS.ms_reference(model, levels, surface=fill)


def rt_run_rrs_sif(model: O.RTModel, rs: OR.RRS, SIF0, fscatt=None):
    """OR.rt_run_rrs with the injection: the elastic j0- carries the emission, interaction_inelastic scatters it."""
    FT = model.FT
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    K = len(rs.i_shift)
    nV = len(model.vza)
    sif = sif_table(pol.n, S, SIF0)
    out = [np.zeros((nV, pol.n, S), dtype=FT) for _ in range(4)]
    F0 = _F0(model)
    if fscatt is None:
        fscatt = OR.default_fscatt(model)
    added, added_surf, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    add_rs, surf_rs, comp_rs = OR.make_added_layer_rs(FT, K, N, S), OR.make_added_layer_rs(FT, K, N, S), OR.make_composite_layer_rs(FT, K, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        rs.Zpp_ie, rs.Zmp_ie = O.compute_Z_moments(pol, qp.qp_mu, rs.greek_raman, m)
        lods = O.construct_core_optical_properties(model, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT)
        for iz in range(L):
            rs.fscatt_rayl = np.asarray(fscatt[:, iz], dtype=FT)
            lo = O.expand_optical_properties(lods[iz], FT)
            OR.rt_kernel_rrs(rs, pol, added, add_rs, comp, comp_rs, lo, tau_sum_all[:, iz].astype(FT), m, qp, iz + 1, F0, FT,
                             model.numerics, None, ifaces[iz])
        O.create_surface_layer_lambertian(model.albedo, added_surf, m, pol, qp, tau_sum_all[:, -1], FT)
        inject(added_surf, sif, m, pol.n)
        OR.interaction_inelastic(ifaces[-1], rs, comp, comp_rs, added_surf, surf_rs, FT)
        OR.postprocessing_vza_rs(pol, comp, comp_rs, model.vza, model.vaz, qp, m, weight, *out)
    return tuple(out)


def _vza_rows(model, weight, vec):
    """[S, N] vector at all streams -> weight * its VZA rows at m = 0, [nVZA, nStokes, S]."""
    pol = model.pol
    out = np.zeros((len(model.vza), pol.n, vec.shape[0]), dtype=vec.dtype)
    c = O.CompositeLayer(None, None, None, None, np.zeros_like(vec), vec)
    O.postprocessing_vza(pol, c, model.vza, model.vaz, model.quad_points, 0, weight, out, np.zeros_like(out))
    return out


def response_from_layers(model, R_pm, T_mm, r_mp):
    """(G_up, G_dn) [nStokes(c), nVZA, nStokes, S] from the atmosphere's composite before the surface interaction and the surface
    r-+: y_c = (I - r-+ R+-)^-1 e_c by a direct solve, the TOA leg T-- y_c, the BOA leg R+- y_c (t++ = I at m = 0)."""
    FT, n = model.FT, model.pol.n
    S, N = R_pm.shape[0], R_pm.shape[1]
    weight = FT(0.5 / math.pi)
    r_mp = np.broadcast_to(r_mp, R_pm.shape)
    M = np.eye(N, dtype=FT)[None] - r_mp @ R_pm
    Gu, Gd = [], []
    for c in range(n):
        e = np.zeros((S, N), dtype=FT)
        e[:, c::n] = 1
        y = np.linalg.solve(M, e[..., None])[..., 0]
        Gu.append(_vza_rows(model, weight, O._mv(T_mm, y)))
        Gd.append(_vza_rows(model, weight, O._mv(R_pm, y)))
    return np.stack(Gu), np.stack(Gd)


def unit_response(model: O.RTModel):
    """G_c of the model: (G_up, G_dn), [nStokes(c), nVZA, nStokes, S] each -- R(SIF0) - R(0) = sum_c 2 SIF0[c] G_up[c]."""
    FT, DT = model.FT, O.deciding_type(model)
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    F0 = _F0(model)
    added, added_surf, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    lods = O.construct_core_optical_properties(model, 0)
    ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
    for iz in range(L):
        lo = O.expand_optical_properties(lods[iz], FT)
        O.rt_kernel(pol, added, comp, lo, ifaces[iz], tau_sum_all[:, iz].astype(FT), 0, qp, iz + 1, F0, FT, model.numerics, None, DT)
    _fill_lambertian(model, added_surf, 0, tau_sum_all[:, -1])
    return response_from_layers(model, comp.R_pm, comp.T_mm, added_surf.r_mp)


def combine(G, tables):
    """sum_c 2 tables[..., c, s] G[c, v, c', s] -> [..., v, c', s]."""
    return 2.0 * np.einsum("...cs,cvds->...vds", np.asarray(tables, dtype=np.float64), G)


def rt_run_lin_sif(model: O.RTModel, lin: OL.LinModel, SIF0, SIF0_dot=None):
    """OL.rt_run_lin (rt_run_lin.jl:102-326) with the injection after the linearized surface builder at m = 0 (the source depends
    on no parameter: the derivative stacks stay as built) and the nSIF slots appended: (R, T, Rdot, Tdot) with Rdot / Tdot
    [nVZA, nStokes, S, P + nSIF].  SIF0_dot: None, [nSIF, S] or [nSIF, nStokes, S]."""
    FT, DT = model.FT, O.deciding_type(model)
    pol, qp = model.pol, model.quad_points
    S, L = model.tau_rayl.shape
    N = qp.Nquad * pol.n
    nV = len(model.vza)
    pl = lin.n_layer_params
    P = pl + 1
    sif = sif_table(pol.n, S, SIF0)
    dots = np.zeros((0, pol.n, S)) if SIF0_dot is None else np.stack([sif_table(pol.n, S, t) for t in np.asarray(SIF0_dot)])
    nSIF = len(dots)
    R, T = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    Rd, Td = np.zeros((nV, pol.n, S, P + nSIF), dtype=FT), np.zeros((nV, pol.n, S, P + nSIF), dtype=FT)
    F0 = _F0(model)
    added, added_s, comp = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_composite_layer(FT, N, S)
    al, als, cl = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S), OL.make_composite_layer_lin(FT, P, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = OL.layer_optics_lin(model, lin, lods, m)
        ifaces, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = np.zeros((S, pl, L + 1))
        for iz in range(L):
            tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
        for iz in range(L):
            lo = O.expand_optical_properties(lods[iz], FT)
            dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT, model.numerics, DT)
            expk = np.exp(-dtau / FT(qp.mu0)).astype(FT)
            OL.elemental_lin(pol, tau_sum_all[:, iz].astype(FT), tsd[:, :, iz], dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, nd, qp,
                             added, al, FT, DT)
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
        OL.create_surface_layer_lambertian_lin(model.albedo, added_s, als, P - 1, m, pol, qp, tau_sum_all[:, -1], tsd[:, :, -1], F0, FT)
        inject(added_s, sif, m, pol.n)
        if m == 0 and nSIF:
            Gu, Gd = response_from_layers(model, comp.R_pm, comp.T_mm, added_s.r_mp)
            Rd[..., P:] += np.moveaxis(combine(Gu, dots), 0, -1).astype(FT)
            Td[..., P:] += np.moveaxis(combine(Gd, dots), 0, -1).astype(FT)
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
