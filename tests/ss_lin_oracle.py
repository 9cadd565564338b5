"""Test oracle of the linearized single-scattering run (vsm.CoreRTLin.rt_run_ss, core_rt_ss.SceneSSLin), built on
oracle/vsm_oracle_lin.py, oracle/vsm_oracle_coxmunk.py and tests/ss_oracle.py, which it imports and does not change.

The reference has no linearized single-scattering driver, so this is our own restatement: ss_oracle.rt_run_ss's walk, statement
for statement, with OL.elemental_lin(ndoubl = 0, dtau = the layer's tau) in place of O.elemental, the two statements of
get_interaction_ss! differentiated (on J0+ before its update),

    J0+'_p = (J0+'_p - J0+ tau'_p / mu_i) exp(-tau / mu_i) + j0+'_p
    J0-'_p += (j0-'_p - j0- tau_sum'_p / mu_i) exp(-tau_sum / mu_i),

the linearized surface builders (OL.create_surface_layer_lambertian_lin, CM.create_surface_layer_brdf_lin) for the surface's
j0- and j0-+' of all P slots, the FORWARD builder's j0+ (the direct beam, ~ exp(-tau_sum / mu_0)) with its derivative
-j0+ tau_sum' / mu_0, and postprocessing_vza per slot.  Central finite differences of ss_oracle.rt_run_ss anchor it
(tests/test_oracle_ss_lin.py).  The linearized builders weigh the direct beam with F0 where the forward builders use I0 = e1
(a quirk of the reference that rt_run_lin shares): the surface terms are derivatives of the forward run for F0[0] = 1 only.

rt_run_ss_lin(model, lin, surface=None, per_m=None) -> (R, T, Rdot, Tdot): [nVZA, nStokes, S] x 2, [nVZA, nStokes, S, P] x 2.
`surface`: None = the model's Lambertian albedo; else a CM.CoxMunkSurface or a function m -> (rho_m, drho_m).  The surface slot is
the last (P - 1).  `per_m` receives per moment dict(m, J0_m, J0_p [S,N], J0_m_dot, J0_p_dot [P,S,N], weight).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
import ms_oracle as MS  # noqa: E402
import ss_oracle as SS  # noqa: E402


def layer_optics_lin(model, lin, lods, m):
    """OL.layer_optics_lin; a model without layer parameters (the surface slot alone) gets empty [S, 0] derivative blocks."""
    if lin.n_layer_params == 0:
        S = model.tau_rayl.shape[0]
        return [OL.LayerOpticsLin(np.zeros((S, 0)), np.zeros((S, 0)), None, None) for _ in lods]
    return OL.layer_optics_lin(model, lin, lods, m)


def interaction_ss_lin(comp: O.CompositeLayer, Jd_p, Jd_m, added: O.AddedLayer, ad_p, ad_m, tau_sum, tau_sum_dot, tau, tau_dot,
                       qp, FT):
    """The derivative of get_interaction_ss! for every slot, then the forward statements.  Jd_p / Jd_m / ad_p / ad_m [P,S,N];
    tau_dot / tau_sum_dot [S,P]."""
    mu = qp.qp_muN.astype(FT)[None, :]
    ts, t = np.asarray(tau_sum, dtype=FT)[:, None], np.asarray(tau, dtype=FT)[:, None]
    for p in range(Jd_p.shape[0]):
        td = np.asarray(tau_dot, dtype=FT)[:, p][:, None]
        tsd = np.asarray(tau_sum_dot, dtype=FT)[:, p][:, None]
        Jd_p[p] = (Jd_p[p] - comp.J0_p * td / mu) * np.exp(-t / mu) + ad_p[p]
        Jd_m[p] = Jd_m[p] + (ad_m[p] - added.j0_m * tsd / mu) * np.exp(-ts / mu)
    SS.interaction_ss(comp, added, tau_sum, tau, qp, FT)


def rt_run_ss_lin(model: O.RTModel, lin: OL.LinModel, surface=None, per_m=None):
    FT, DT, pol, qp, S, L, N, F0 = MS._setup(model)
    fill_surface = MS._surface_fn(model, None)
    if surface is not None:
        rd = surface if callable(surface) else (lambda m: CM.reflectance_and_deriv(surface, pol.n, qp.qp_mu.astype(np.float64), m))
        fill_surface = lambda m, a, ts: CM.create_surface_layer_brdf(rd(m)[0], a, m, pol, qp, ts, FT)
    nV = len(model.vza)
    pl = lin.n_layer_params
    P = pl + 1
    R, T = np.zeros((nV, pol.n, S), dtype=FT), np.zeros((nV, pol.n, S), dtype=FT)
    Rd, Td = np.zeros((nV, pol.n, S, P), dtype=FT), np.zeros((nV, pol.n, S, P), dtype=FT)
    added, added_surf, added_sl = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    al, als = OL.make_added_layer_lin(FT, P, N, S), OL.make_added_layer_lin(FT, P, N, S)
    comp = O.make_composite_layer(FT, N, S)
    Jd_p, Jd_m = np.zeros((P, S, N), dtype=FT), np.zeros((P, S, N), dtype=FT)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(model, m)
        lins = layer_optics_lin(model, lin, lods, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = np.zeros((S, P, L + 1))                       # surface slots: zero in the atmosphere
        for iz in range(L):
            tsd[:, :pl, iz + 1] = tsd[:, :pl, iz] + lins[iz].tau_dot
        for iz in range(L):
            lo = O.expand_optical_properties(lods[iz], FT)
            tau_sum = tau_sum_all[:, iz].astype(FT)
            OL.elemental_lin(pol, tau_sum, tsd[:, :pl, iz], lo.tau, F0, lo.varpi, lo.Zpp, lo.Zmp, lins[iz], m, 0, qp, added, al, FT,
                             DT)
            if iz == 0:
                comp.J0_p[...] = added.j0_p
                comp.J0_m[...] = added.j0_m
                Jd_p[...] = al.ap_J0_p
                Jd_m[...] = al.ap_J0_m
            else:
                td = np.zeros((S, P))
                td[:, :pl] = lins[iz].tau_dot
                interaction_ss_lin(comp, Jd_p, Jd_m, added, al.ap_J0_p, al.ap_J0_m, tau_sum, tsd[:, :, iz], lo.tau, td, qp, FT)
        # the surface: forward builder (the forward run's j0-+), linearized builder (j0- and j0-+' of all P slots)
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        if surface is None:
            OL.create_surface_layer_lambertian_lin(model.albedo, added_sl, als, P - 1, m, pol, qp, tau_sum_all[:, -1],
                                                   tsd[:, :pl, -1], F0, FT)
        else:
            rho, drho = rd(m)
            CM.create_surface_layer_brdf_lin(rho, drho, added_sl, als, P - 1, m, pol, qp, tau_sum_all[:, -1], tsd[:, :pl, -1], F0, FT)
        mu = qp.qp_muN.astype(FT)[None, :]
        es = np.exp(-tau_sum_all[:, -1].astype(FT)[:, None] / mu)
        for p in range(P):
            tsd_p = tsd[:, p, -1].astype(FT)[:, None]
            Jd_p[p] = Jd_p[p] + (als.ap_J0_p[p] - added_surf.j0_p * tsd_p / FT(qp.mu0))
            Jd_m[p] = Jd_m[p] + (als.ap_J0_m[p] - added_sl.j0_m * tsd_p / mu) * es
        SS.interaction_ss(comp, added_surf, tau_sum_all[:, -1], np.zeros(S, dtype=FT), qp, FT)
        if per_m is not None:
            per_m.append(dict(m=m, J0_m=comp.J0_m.copy(), J0_p=comp.J0_p.copy(), J0_m_dot=Jd_m.copy(), J0_p_dot=Jd_p.copy(),
                              weight=weight))
        O.postprocessing_vza(pol, comp, model.vza, model.vaz, qp, m, weight, R, T)
        for p in range(P):
            cp = O.CompositeLayer(None, None, None, None, Jd_p[p], Jd_m[p])
            r, t = np.zeros_like(R), np.zeros_like(T)
            O.postprocessing_vza(pol, cp, model.vza, model.vaz, qp, m, weight, r, t)
            Rd[..., p] += r
            Td[..., p] += t
    return R, T, Rd, Td
