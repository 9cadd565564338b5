"""Test oracle of the single-scattering runs (vsm.CoreRT.rt_run_ss, vsm.CoreRTRaman.rt_run_ss), built on oracle/vsm_oracle.py and
oracle/vsm_oracle_raman.py, which it imports and does not change.

rt_run_ss(model)               rt_run_ss(::noRS, model, iBand) (src/CoreRT/rt_run.jl:574-755), statement order: per Fourier moment
                               and layer rt_kernel_ss! (CoreKernel/rt_kernel_ss.jl:156-238) = elemental! with ndoubl = 0 and
                               dtau = the layer's tau (scatter hard-wired to true), the TOA copy or interaction_ss!
                               (CoreKernel/interaction_ss.jl:14-43); create_surface_layer! and one more interaction_ss! with layer
                               tau = 0 (rt_run.jl:700-722); postprocessing_vza!; the hemispherical sums of m = 0 (:737-748).
rt_run_ss_rrs(model, rs, ...)  the same with rt_kernel_ss!(::RRS) (:240-337): elemental_inelastic! with ndoubl = 0 and
                               interaction_inelastic_ss! (interaction_ss.jl:45-90) on the [K,S,N] ieJ0 arrays, summed over the lines
                               only by postprocessing_vza!(::RRS).

Both return (R_SFI, T_SFI, ieR_SFI, ieT_SFI, hem_R, hem_T): [nVZA, nStokes, nSpec] x 4, [nSpec] x 2.
`surface`: None = the model's Lambertian albedo; else a function (m, added_surf, tau_sum) as in tests/ms_oracle.py.
`per_m`: a list that receives, per moment, dict(m, J0_m, J0_p [S,N], ieJ0_m, ieJ0_p [K,S,N] or None, weight).
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
from oracle import vsm_oracle_raman as OR  # noqa: E402
import ms_oracle as MS  # noqa: E402


def ss_arrays(pol_n, S, L, seed=11, zero_layer=None):
    """Optical depths and the beam as _raman_models (test_gpu_raman.py) draws them, the absorption on a 32-level grid."""
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    if zero_layer is not None:
        tau_rayl[:, zero_layer] = 0.0
    tau_abs = (10.0 ** (-2 + 2.3 * rng.integers(0, 32, (S, 1)) / 32.0)) * np.linspace(0.5, 1.5, L)[None, :] / L
    F0 = np.zeros((pol_n, S))
    F0[0] = 0.8 + 0.4 * rng.random(S)
    if pol_n > 1:
        F0[1] = 0.1 * rng.random(S) - 0.05
    return tau_rayl, tau_abs, F0


def interaction_ss(comp: O.CompositeLayer, added: O.AddedLayer, tau_sum, tau, qp, FT):
    """get_interaction_ss! (interaction_ss.jl:14-19)."""
    mu = qp.qp_muN.astype(FT)[None, :]
    tau_sum, tau = np.asarray(tau_sum, dtype=FT)[:, None], np.asarray(tau, dtype=FT)[:, None]
    comp.J0_p[...] = comp.J0_p * np.exp(-tau / mu) + added.j0_p
    comp.J0_m[...] = comp.J0_m + added.j0_m * np.exp(-tau_sum / mu)


def interaction_inelastic_ss(rs: OR.RRS, comp_rs: OR.CompositeLayerRS, add_rs: OR.AddedLayerRS, tau_sum, tau, qp, FT):
    """get_interaction_ss_RRS! (interaction_ss.jl:79-90): the in-band (n1, dn) pairs only."""
    mu = qp.qp_muN.astype(FT)[None, :]
    tau_sum, tau = np.asarray(tau_sum, dtype=FT), np.asarray(tau, dtype=FT)
    S = len(tau)
    for dn, shift in enumerate(rs.i_shift):
        n0, n1 = OR.get_n0_n1(S, int(shift))
        if n1.stop <= n1.start:
            continue
        comp_rs.ieJ0_p[dn, n1] = comp_rs.ieJ0_p[dn, n1] * np.exp(-tau[n1][:, None] / mu) + add_rs.ieJ0_p[dn, n1]
        comp_rs.ieJ0_m[dn, n1] = comp_rs.ieJ0_m[dn, n1] + add_rs.ieJ0_m[dn, n1] * np.exp(-tau_sum[n1][:, None] / mu)


def _run(model, rs, fscatt, surface, per_m):
    FT, DT, pol, qp, S, L, N, F0 = MS._setup(model)
    fill_surface = MS._surface_fn(model, surface)
    nV = len(model.vza)
    R_SFI, T_SFI, ieR_SFI, ieT_SFI = [np.zeros((nV, pol.n, S), dtype=FT) for _ in range(4)]
    hem_R, hem_T = np.zeros(S, dtype=FT), np.zeros(S, dtype=FT)
    added, added_surf = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
    comp = O.make_composite_layer(FT, N, S)
    K = 0
    if rs is not None:
        K = len(rs.i_shift)
        if fscatt is None:
            fscatt = OR.default_fscatt(model)
        add_rs, comp_rs = OR.make_added_layer_rs(FT, K, N, S), OR.make_composite_layer_rs(FT, K, N, S)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        if rs is not None:
            rs.Zpp_ie, rs.Zmp_ie = O.compute_Z_moments(pol, qp.qp_mu, rs.greek_raman, m)
        lods = O.construct_core_optical_properties(model, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        for iz in range(L):                                 # rt_kernel_ss!
            lo = O.expand_optical_properties(lods[iz], FT)
            tau_sum = tau_sum_all[:, iz].astype(FT)
            if rs is not None:
                rs.fscatt_rayl = np.asarray(fscatt[:, iz], dtype=FT)
                OR.elemental_inelastic(rs, pol, tau_sum, lo.tau, F0, m, 0, qp, add_rs, FT)
            O.elemental(pol, tau_sum, lo.tau, F0, lo.varpi, lo.Zpp, lo.Zmp, m, 0, qp, added, FT, DT)
            if iz == 0:
                comp.J0_p[...] = added.j0_p
                comp.J0_m[...] = added.j0_m
                if rs is not None:
                    comp_rs.ieJ0_p[...] = add_rs.ieJ0_p
                    comp_rs.ieJ0_m[...] = add_rs.ieJ0_m
            else:
                interaction_ss(comp, added, tau_sum, lo.tau, qp, FT)
                if rs is not None:
                    interaction_inelastic_ss(rs, comp_rs, add_rs, tau_sum, lo.tau, qp, FT)
        fill_surface(m, added_surf, tau_sum_all[:, -1])
        interaction_ss(comp, added_surf, tau_sum_all[:, -1], np.zeros(S, dtype=FT), qp, FT)
        if per_m is not None:
            per_m.append(dict(m=m, J0_m=comp.J0_m.copy(), J0_p=comp.J0_p.copy(), weight=weight,
                              ieJ0_m=None if rs is None else comp_rs.ieJ0_m.copy(),
                              ieJ0_p=None if rs is None else comp_rs.ieJ0_p.copy()))
        if rs is None:
            O.postprocessing_vza(pol, comp, model.vza, model.vaz, qp, m, weight, R_SFI, T_SFI)
        else:
            OR.postprocessing_vza_rs(pol, comp, comp_rs, model.vza, model.vaz, qp, m, weight, R_SFI, T_SFI, ieR_SFI, ieT_SFI)
        if m == 0:
            for s in range(S):
                for j in range(qp.Nquad):
                    j_I = j * pol.n
                    hem_R[s] += comp.J0_m[s, j_I] * qp.qp_mu[j] * qp.wt_mu[j]
                    hem_T[s] += comp.J0_p[s, j_I] * qp.qp_mu[j] * qp.wt_mu[j]
    return R_SFI, T_SFI, ieR_SFI, ieT_SFI, hem_R, hem_T


def rt_run_ss(model: O.RTModel, surface=None, per_m=None):
    return _run(model, None, None, surface, per_m)


def rt_run_ss_rrs(model: O.RTModel, rs: OR.RRS, fscatt=None, surface=None, per_m=None):
    return _run(model, rs, fscatt, surface, per_m)
