"""Test oracle of vsm.Scattering's linearized Mie: a numpy restatement of the reference's linearized NAI-2 path
(src/Scattering/compute_NAI2_lin.jl, mie_helper_functions_lin.jl), in float64 and, with dtype = np.longdouble, in the x87 format
on the same float64 inputs (see mie_oracle).  It imports only mie_oracle.

compute_mie_ab_lin, compute_wx_lin restate the linearized compute_mie_ab! and compute_w_x; nai2_lin_reference takes what
vsm_mie_nai2_lin takes and returns what it returns; compute_aerosol_optical_properties_lin chains the host part and it.
D_n', a_n', b_n' and S1', S2' are computed for n_r and for n_i separately, as the reference does: the device computes n_r alone and
uses d / d n_i = -i d / d n_r, so the comparison checks that identity.

Slot order (n_r, n_i, mu, sigma), mu = ln r_m and sigma = ln sigma_g of LogNormal(mu, sigma).  The nodes are held fixed.

One place where this is not the reference's text: the derivative of the normalised weights.  With
raw = pdf(r) w_r, S = sum raw, wx = raw / S the derivative is (raw' - (sum raw') wx) / S; the reference normalises wx first and then
divides by sum(wx) = 1, which loses the 1 / S.  compute_wx_lin is the correct form, compute_wx_lin_reference_form the
reference's (kept for the test of the deviation only)."""
from __future__ import annotations

import math
import types

import numpy as np

import mie_oracle as MO

SLOTS = ("n_r", "n_i", "mu", "sigma")


def compute_mie_ab_lin(x, m, nmax_i, n_max, dtype=np.float64):
    """The linearized compute_mie_ab! for every radius at once: a_n, b_n [n_max, nquad] and their derivatives [2, n_max, nquad]
    with respect to n_r and n_i, exact zeros above n_max_i."""
    R, Cx, _ = MO.arithmetic(dtype)
    nmx = MO.start_orders(x, m, nmax_i)
    x = np.asarray(x, dtype=np.float64).astype(R)
    m = complex(m) if R is np.float64 else Cx(m)
    nq = len(x)
    nmax_i = np.asarray(nmax_i, dtype=np.int64)
    y = x * m
    Dn = np.zeros((n_max + 1, nq), dtype=Cx)
    Dd = np.zeros((2, n_max + 1, nq), dtype=Cx)
    prev = np.zeros(nq, dtype=Cx)
    prev_d = np.zeros((2, nq), dtype=Cx)
    for n in range(int(nmx.max()) - 1, 0, -1):
        on = n <= nmx - 1
        ratio = (n + 1) / y
        denom_inv = 1 / (prev + ratio)
        dratio = np.stack([-ratio * x / y, ratio * x * 1j / y])
        cur_d = dratio + denom_inv ** 2 * (prev_d + dratio)
        prev_d = np.where(on, cur_d, prev_d)
        prev = np.where(on, ratio - denom_inv, prev)
        if n <= n_max:
            Dn[n] = prev
            Dd[:, n] = prev_d
    an = np.zeros((n_max, nq), dtype=Cx)
    bn = np.zeros((n_max, nq), dtype=Cx)
    ad = np.zeros((2, n_max, nq), dtype=Cx)
    bd = np.zeros((2, n_max, nq), dtype=Cx)
    psi0, psi1, chi0, chi1 = np.cos(x), np.sin(x), -np.sin(x), np.cos(x)
    xi1 = psi1 + 1j * chi1
    with np.errstate(all="ignore"):       # (a small radius' chi overflows above its own n_max_i, where nothing is kept)
        for n in range(1, n_max + 1):
            psi = (2 * n - 1) * psi1 / x - psi0
            chi = (2 * n - 1) * chi1 / x - chi0
            xi = psi + 1j * chi
            t_a = Dn[n] / m + n / x
            t_b = Dn[n] * m + n / x
            on = n <= nmax_i
            an[n - 1] = np.where(on, (t_a * psi - psi1) / (t_a * xi - xi1), 0)
            bn[n - 1] = np.where(on, (t_b * psi - psi1) / (t_b * xi - xi1), 0)
            for i, dm in enumerate((1.0, -1j)):           # d m / d n_r = 1, d m / d n_i = -i
                td_a = Dd[i, n] / m - (Dn[n] / m ** 2) * dm
                td_b = Dd[i, n] * m + Dn[n] * dm
                ad[i, n - 1] = np.where(on, (td_a * psi) / (t_a * xi - xi1) - (t_a * psi - psi1) * (td_a * xi) / (t_a * xi - xi1) ** 2, 0)
                bd[i, n - 1] = np.where(on, (td_b * psi) / (t_b * xi - xi1) - (t_b * psi - psi1) * (td_b * xi) / (t_b * xi - xi1) ** 2, 0)
            psi0, psi1, chi0, chi1 = psi1, psi, chi1, chi
            xi1 = psi1 + 1j * chi1
    return an, bn, ad, bd


def raw_weights_lin(size_distribution, w_r, r):
    """raw = pdf(r) w_r and its derivatives [2, nquad] with respect to (mu, sigma)."""
    r = np.asarray(r, dtype=np.float64)
    raw = size_distribution.pdf(r) * w_r
    d = np.log(r) - size_distribution.mu
    s = size_distribution.sigma
    return raw, np.stack([d / s ** 2 * raw, (d ** 2 / s ** 3 - 1 / s) * raw])


def compute_wx_lin(r, raw, raw_dot):
    """wx_dot, wr_dot [2, nquad] from the unnormalised weights and their derivatives: the correct form."""
    total = np.sum(raw)
    wx = raw / total
    wx_dot = np.stack([(raw_dot[k] - np.sum(raw_dot[k]) * wx) / total for k in range(2)])
    return wx_dot, 4 * math.pi * r ** 2 * wx_dot


def compute_wx_lin_reference_form(r, raw, raw_dot):
    """The reference's compute_w_x(lin, .): wx is normalised first, then wx' = raw' / sum(wx) - (sum raw') wx / sum(wx)^2 with
    sum(wx) = 1 -- the factor 1 / sum(raw) is missing."""
    wx = raw / np.sum(raw)
    s = np.sum(wx)
    wx_dot = np.stack([raw_dot[k] / s - np.sum(raw_dot[k]) * wx / s ** 2 for k in range(2)])
    return wx_dot, 4 * math.pi * r ** 2 * wx_dot


def greek_dot_from_bulk(bulk_f, C_sca, bulk_f_dot, C_sca_dot, mu, w_mu, dtype=np.float64):
    """Stage 3 alone, linearized: greek_dot [4, 6, n_mu] from the unnormalised bulk functions [4, n_mu], their derivatives
    [4, 4, n_mu], the bulk C_sca and its derivatives [4] -- mie_oracle.greek_from_bulk's counterpart."""
    R = MO.arithmetic(dtype)[0]
    bn_ = np.asarray(bulk_f).astype(R) / R(C_sca)
    bulk_dot, cd = np.asarray(bulk_f_dot).astype(R), np.asarray(C_sca_dot).astype(R)
    return MO.greek_quadrature([(bulk_dot[s] - bn_ * cd[s]) / R(C_sca) for s in range(4)], mu, w_mu, dtype)


def nai2_lin_reference(x, wx, wr, wx_dot, wr_dot, nmax_i, mu, w_mu, n_r, n_i, k_wave, n_max, dtype=np.float64, scales=False):
    """compute_aerosol_optical_properties(lin, .) (compute_NAI2_lin.jl:86-253) from the host part's arrays.  Returns greek [6, n_mu],
    (C_sca, C_ext, ssa), bulk_f [4, n_mu] (unnormalised) as mie_oracle.nai2_reference, and greek_dot [4, 6, n_mu], scal_dot [4, 3]
    (C_sca', C_ext', ssa' per slot), bulk_f_dot [4, 4, n_mu] (unnormalised: the sums over the radii alone).  scales = True adds the
    sums of the absolute terms behind stage 2's sums: bulk_abs [n_mu] and c_abs as mie_oracle.nai2_reference, bulk_dot_abs
    [4, n_mu] = sum_i |wr_i 0.5 / x_i^2| 2 (|S1'| |S1| + |S2'| |S2|) for n_r and n_i, sum_i |wr_dot_i 0.5 / x_i^2| (|S1|^2 + |S2|^2)
    for the two weight slots, and c_dot_abs [4, 2] for C_sca' and C_ext' alike."""
    R, _, pi = MO.arithmetic(dtype)
    x, wx, wr = (np.asarray(a, dtype=np.float64).astype(R) for a in (x, wx, wr))
    wx_dot, wr_dot = (np.asarray(a, dtype=np.float64).astype(R) for a in (wx_dot, wr_dot))
    m = complex(n_r, -n_i)
    pi_, tau_ = MO.compute_mie_pi_tau(mu, n_max, dtype)
    an, bn, ad, bd = compute_mie_ab_lin(x, m, nmax_i, n_max, dtype)
    S1, S2 = MO.compute_mie_S1S2(an, bn, pi_, tau_, dtype)
    Sd = [MO.compute_mie_S1S2(ad[i], bd[i], pi_, tau_, dtype) for i in range(2)]
    n_ = (2.0 * np.arange(1, n_max + 1) + 1)[:, None]
    coef = 2 * pi / k_wave ** 2
    C_sca = coef * np.sum(n_ * (np.abs(an) ** 2 + np.abs(bn) ** 2), axis=0)
    C_ext = coef * np.sum(n_ * np.real(an + bn), axis=0)
    inv_x2 = 0.5 / x ** 2
    cj = np.conj
    f = np.stack([inv_x2 * (np.abs(S1) ** 2 + np.abs(S2) ** 2), inv_x2 * np.real(S1 * cj(S2) + S2 * cj(S1)),
                  -inv_x2 * (np.abs(S1) ** 2 - np.abs(S2) ** 2), -inv_x2 * np.imag(S1 * cj(S2) - S2 * cj(S1))])
    bulk_C_sca, bulk_C_ext = R(np.sum(wx * C_sca)), R(np.sum(wx * C_ext))
    ssa = bulk_C_sca / bulk_C_ext
    bulk = f @ wr
    Cd = np.zeros((4, 2), dtype=R)                          # (C_sca', C_ext') per slot
    bulk_dot = np.zeros((4, 4, len(mu)), dtype=R)
    for i in range(2):
        d1, d2 = Sd[i]
        cs = coef * np.sum(n_ * np.real(an * cj(ad[i]) + ad[i] * cj(an) + bn * cj(bd[i]) + bd[i] * cj(bn)), axis=0)
        ce = coef * np.sum(n_ * np.real(ad[i] + bd[i]), axis=0)
        Cd[i] = np.sum(wx * cs), np.sum(wx * ce)
        fd = np.stack([inv_x2 * np.real(d1 * cj(S1) + S1 * cj(d1) + d2 * cj(S2) + S2 * cj(d2)),
                       inv_x2 * np.real(d1 * cj(S2) + S1 * cj(d2) + d2 * cj(S1) + S2 * cj(d1)),
                       -inv_x2 * np.real(d1 * cj(S1) + S1 * cj(d1) - d2 * cj(S2) - S2 * cj(d2)),
                       -inv_x2 * np.imag(d1 * cj(S2) + S1 * cj(d2) - d2 * cj(S1) - S2 * cj(d1))])
        bulk_dot[i] = fd @ wr
    for k in range(2):
        Cd[2 + k] = np.sum(wx_dot[k] * C_sca), np.sum(wx_dot[k] * C_ext)
        bulk_dot[2 + k] = f @ wr_dot[k]
    scal_dot = np.stack([Cd[:, 0], Cd[:, 1], (Cd[:, 0] - ssa * Cd[:, 1]) / bulk_C_ext], axis=1)
    bn_ = bulk / bulk_C_sca
    sets = [bn_] + [(bulk_dot[s] - bn_ * Cd[s, 0]) / bulk_C_sca for s in range(4)]
    out = MO.greek_quadrature(sets, mu, w_mu, dtype)
    res = out[0], (bulk_C_sca, bulk_C_ext, ssa), bulk, out[1:], scal_dot, bulk_dot, (an, bn, ad, bd)
    if scales:
        c_ext_abs = coef * np.sum(n_ * np.abs(np.real(an + bn)), axis=0)
        awx, awr = np.abs(wx), np.abs(wr)
        bulk_dot_abs = np.zeros((4, len(mu)), dtype=R)
        c_dot_abs = np.zeros((4, 2), dtype=R)
        for i in range(2):
            d1, d2 = Sd[i]
            bulk_dot_abs[i] = (inv_x2 * 2 * (np.abs(d1) * np.abs(S1) + np.abs(d2) * np.abs(S2))) @ awr
            cs = coef * np.sum(n_ * 2 * (np.abs(an) * np.abs(ad[i]) + np.abs(bn) * np.abs(bd[i])), axis=0)
            ce = coef * np.sum(n_ * np.abs(np.real(ad[i] + bd[i])), axis=0)
            c_dot_abs[i] = np.sum(awx * cs), np.sum(awx * ce)
        for k in range(2):
            bulk_dot_abs[2 + k] = f[0] @ np.abs(wr_dot[k])
            c_dot_abs[2 + k] = np.sum(np.abs(wx_dot[k]) * C_sca), np.sum(np.abs(wx_dot[k]) * c_ext_abs)
        res += (types.SimpleNamespace(bulk_abs=f[0] @ awr, c_abs=(np.sum(awx * C_sca), np.sum(awx * c_ext_abs)),
                                      bulk_dot_abs=bulk_dot_abs, c_dot_abs=c_dot_abs),)
    return res


def mie_lin_inputs(size_distribution, wavelength, r_max, nquad_radius, tabulated=None, weights=compute_wx_lin):
    """mie_oracle.mie_inputs plus wx_dot, wr_dot [2, nquad].  tabulated = (r, raw) or (r, raw, raw_dot): exact zeros without
    raw_dot.  weights: compute_wx_lin (correct) or compute_wx_lin_reference_form."""
    if tabulated is None:
        h = MO.mie_inputs(size_distribution, wavelength, r_max, nquad_radius)
        _, w_r = MO.gauleg_log(nquad_radius, max(size_distribution.quantile(1e-8), 1e-6 * r_max), r_max)
        raw, raw_dot = raw_weights_lin(size_distribution, w_r, h.r)
        h.wx_dot, h.wr_dot = weights(h.r, raw, raw_dot)
    else:
        h = MO.mie_inputs(None, wavelength, None, None, tabulated=tabulated[:2])
        if len(tabulated) > 2:
            h.wx_dot, h.wr_dot = weights(h.r, np.asarray(tabulated[1], dtype=np.float64), np.asarray(tabulated[2], dtype=np.float64))
        else:
            h.wx_dot, h.wr_dot = np.zeros((2, len(h.r))), np.zeros((2, len(h.r)))
    return h


def compute_aerosol_optical_properties_lin(size_distribution, n_r, n_i, wavelength, r_max, nquad_radius, tabulated=None,
                                           weights=compute_wx_lin):
    """greek, ssa, k, C_sca, bulk_f (unnormalised here), and greek_dot [4, 6, n_mu], ssa_dot, k_dot, C_sca_dot [4], bulk_f_dot."""
    assert n_i >= 0
    h = mie_lin_inputs(size_distribution, wavelength, r_max, nquad_radius, tabulated, weights)
    greek, (C_sca, C_ext, ssa), bulk, greek_dot, scal_dot, bulk_dot, ab = nai2_lin_reference(
        h.x, h.wx, h.wr, h.wx_dot, h.wr_dot, h.nmax_i, h.mu, h.w_mu, n_r, n_i, h.k_wave, h.n_max)
    return types.SimpleNamespace(greek=greek, ssa=ssa, k=C_ext, C_sca=C_sca, C_ext=C_ext, bulk_f=bulk, greek_dot=greek_dot,
                                 ssa_dot=scal_dot[:, 2], k_dot=scal_dot[:, 1], C_sca_dot=scal_dot[:, 0], bulk_f_dot=bulk_dot,
                                 host=h, ab=ab)


def monodisperse_lin(x, n_r, n_i):
    """One sphere of size parameter x: slots 2 and 3 are exact zeros."""
    return compute_aerosol_optical_properties_lin(None, n_r, n_i, MO.MONO_WAVELENGTH, None, 1, tabulated=([x], [1.0]))
