"""Test oracle of the linearized single-scattering run with rotational Raman scattering (vsm.CoreRTRaman.rt_run_ss_lin,
core_rt_ss.SceneSSRamanLin, vsm_ss_column_rrs_lin_*), built on tests/ss_oracle.py, tests/ss_lin_oracle.py and
oracle/vsm_oracle_raman.py, which it imports and does not change.

The reference has no linearized Raman driver, so this is our own restatement: the walk of ss_oracle.rt_run_ss_rrs over the in-band
(recipient n1, line, donor n0 = n1 + shift) pairs with the kernel's statements.  A pair's source depends on the run's parameters
through d0 = tau[n0], d1 = tau[n1] and g0 = fscatt[n0] exp(-tau_sum[n0] / mu_0) only:

    j+ = c+ g0 G(d0, d1),  G = (e^-v - e^-u) / (mu_i / mu_0 - d1 / d0) = (d0 / mu_i) phi(u, v),   u = d0 / mu_0, v = d1 / mu_i
    j- = c- g0 H(d0, d1),  H = (1 - e^-(u + v)) / (mu_i / mu_0 + d1 / d0) = (d0 / mu_i) psi(u + v)
    g0' = fscatt'[n0] exp(-tau_sum[n0] / mu_0) - g0 tau_sum'[n0] / mu_0
    G_d0 = (phi + u phi_u) / mu_i,  G_d1 = (d0 / mu_i^2) phi_v,  phi_v = -phi - phi_u
    H_d0 = (psi + u psi') / mu_i,   H_d1 = (d0 / mu_i^2) psi'

with psi(x) = (1 - e^-x) / x, phi(u, v) = (e^-v - e^-u) / (u - v) = e^-v psi(u - v), phi_u = e^-v psi'(u - v): the partials of the
regular expression in a form that does not cancel like eps / (u - v)^2 (psi' by its series below 1/8).  In the forward kernel's
close branches (|d0 - d1| <= 1e-8 on the SZA rows, |mu_i / mu_0 - d1 / d0| < 1e-8 elsewhere: u = v) G = (d0 / mu_i) e^-u and the
partials are the limits phi = e^-u, phi_u = phi_v = -e^-u / 2: G_d0 = e^-u / mu_i (1 - d0 / (2 mu_0)), G_d1 = -d0 e^-u / (2 mu_i^2).
`naive_close=True` differentiates the close value as written, as a function of d0 alone (G_d0 = e^-u / mu_i (1 - d0 / mu_0),
G_d1 = 0): the wrong derivative the tests show to be wrong.  The line sums then go through the differentiated interaction, on S+
before its update,

    S+' = (S+' - S+ tau'[n1] / mu_i) exp(-tau[n1] / mu_i) + s+',    S-' += (s-' - s- tau_sum'[n1] / mu_i) exp(-tau_sum[n1] / mu_i).

rt_run_ss_rrs_lin(model, lin, rs, fscatt=None, fscatt_dot=None) -> (R1, T1, ieR1, ieT1, R1dot, T1dot, ieR1dot, ieT1dot):
[nVZA, nStokes, S] x 4 (ss_oracle.rt_run_ss_rrs's), [nVZA, nStokes, S, P] x 4 (R1dot, T1dot: ss_lin_oracle.rt_run_ss_lin's).
fscatt [S, L] and fscatt_dot [p_layer, S, L]; both None = default_fscatt and default_fscatt_dot.
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
import ss_lin_oracle as SSL  # noqa: E402
import ss_oracle as SS  # noqa: E402

CLOSE = 1e-8    # rt_close_tol, the switch of both close branches of the forward kernel


def default_fscatt_dot(model, lin):
    """The derivative of OR.default_fscatt = tau_rayl / tau_scatt, [p_layer, S, L]: only the aerosol slots move tau_scatt, and
    their tau_dot is d tau_scatt / dx exactly, so fscatt_dot[p] = -fscatt^2 tau_dot[p] / tau_rayl there (0 where tau_rayl = 0)
    and 0 on the gas slots."""
    S, L = model.tau_rayl.shape
    pl, na = lin.n_layer_params, 7 * lin.n_aer
    out = np.zeros((pl, S, L))
    if na == 0:
        return out
    lods = O.construct_core_optical_properties(model, 0)
    lins = SSL.layer_optics_lin(model, lin, lods, 0)
    fs = OR.default_fscatt(model)
    for iz in range(L):
        rayl = model.tau_rayl[:, iz].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = -(fs[:, iz] ** 2 / rayl)[None, :] * np.asarray(lins[iz].tau_dot, dtype=np.float64)[:, :na].T
        out[:na, :, iz] = np.where((rayl > 0)[None, :], d, 0.0)
    return out


_PSI1 = [(-1.0) ** (j + 1) * (j + 1) / math.factorial(j + 2) for j in range(11)]


def psi1(x, em, FT):
    """psi'(x) = (x e^-x - (1 - e^-x)) / x^2 for x >= 0 with em = expm1(-x): the closed form cancels like eps / x^2, so below 1/8
    the series sum_j (-1)^(j+1) (j + 1) / (j + 2)! x^j (11 terms), as the kernel."""
    p = np.full_like(x, FT(_PSI1[-1]))
    for c in _PSI1[-2::-1]:
        p = p * x + FT(c)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        closed = (x * (FT(1) + em) + em) / x / x
    return np.where(x < FT(0.125), p, closed)


def line_partials(sun, d0, d1, mi, ms, FT, naive_close=False):
    """(G, G_d0, G_d1, H, H_d0, H_d1) of one (donor, recipient) pair at the rows mi [N] (sun [N]: the SZA rows); d0, d1 [n].
    G = (d0 / mu_i) phi(u, v), H = (d0 / mu_i) psi(u + v), u = d0 / mu_0, v = d1 / mu_i, psi(x) = (1 - e^-x) / x,
    phi = e^-v psi(u - v) = e^-u psi(v - u); psi and psi' are taken at |u - v|, from the side that cannot overflow."""
    d0, d1, mi = d0[:, None], d1[:, None], mi[None, :]
    one, half = FT(1), FT(0.5)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rm = mi / ms
        ratio = d1 / d0
        x0, x1 = d0 / ms + 0 * mi, d1 / mi
        e0, e1 = np.exp(-x0), np.exp(-x1)
        c = d0 / mi
        close = np.where(sun[None, :], ~(np.abs(d0 - d1) > CLOSE), np.abs(rm - ratio) < CLOSE)
        t = x0 - x1
        at = np.abs(t)
        em = np.expm1(-at)
        psi = np.where(at == 0, one, -em / at)
        p1 = psi1(at, em, FT)
        phi = np.where(t > 0, e1, e0) * psi
        phi_u = np.where(t > 0, e1 * p1, -phi - e0 * p1)
        G, G0, G1 = c * phi, (phi + x0 * phi_u) / mi, -c / mi * (phi + phi_u)
        Gc = c * e0
        if naive_close:
            G0c, G1c = (e0 / mi) * (one - x0), np.zeros_like(Gc)
        else:
            G0c, G1c = (e0 / mi) * (one - half * x0), -half * c / mi * e0
        G, G0, G1 = np.where(close, Gc, G), np.where(close, G0c, G0), np.where(close, G1c, G1)
        s = x0 + x1
        A = -np.expm1(-s)
        psi_s = np.where(s == 0, one, A / s)
        p1s = psi1(s, -A, FT)
        H, H0, H1 = c * psi_s, (psi_s + x0 * p1s) / mi, c / mi * p1s
    return G, G0, G1, H, H0, H1


def rt_run_ss_rrs_lin(model: O.RTModel, lin, rs: OR.RRS, fscatt=None, fscatt_dot=None, naive_close=False):
    FT, DT, pol, qp, S, L, N, F0 = MS._setup(model)
    nV, n = len(model.vza), pol.n
    pl = lin.n_layer_params
    P = pl + 1
    fwd = SS.rt_run_ss_rrs(model, rs, fscatt=fscatt)
    _, _, Rd, Td = SSL.rt_run_ss_lin(model, lin)
    if fscatt is None:
        if fscatt_dot is not None:
            raise ValueError("fscatt_dot without fscatt")
        fscatt, fscatt_dot = OR.default_fscatt(model), default_fscatt_dot(model, lin)
    elif fscatt_dot is None:
        raise ValueError("a stated fscatt needs fscatt_dot")
    fscatt_dot = np.asarray(fscatt_dot, dtype=FT).reshape(pl, S, L)
    ieRd, ieTd = np.zeros((nV, n, S, P), dtype=FT), np.zeros((nV, n, S, P), dtype=FT)
    mu = qp.qp_muN.astype(FT)
    i_start = n * qp.imu0
    sun = np.zeros(N, dtype=bool)
    sun[i_start:i_start + n] = True
    ms = mu[i_start]
    F0 = np.asarray(F0, dtype=FT)
    for m in range(model.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        wct02 = FT(0.5) if m == 0 else FT(0.25)
        Zpp, Zmp = (np.asarray(z, dtype=FT) for z in O.compute_Z_moments(pol, qp.qp_mu, rs.greek_raman, m))
        lods = O.construct_core_optical_properties(model, m)
        lins = SSL.layer_optics_lin(model, lin, lods, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT, DT)
        tsd = np.zeros((S, pl, L + 1))
        for iz in range(L):
            tsd[:, :, iz + 1] = tsd[:, :, iz] + lins[iz].tau_dot
        Sp = np.zeros((S, N), dtype=FT)
        Dp, Dm = np.zeros((pl, S, N), dtype=FT), np.zeros((pl, S, N), dtype=FT)
        for iz in range(L):
            tau = O.expand_optical_properties(lods[iz], FT).tau.astype(FT)
            ts = tau_sum_all[:, iz].astype(FT)
            td, tsd_z = np.asarray(lins[iz].tau_dot, dtype=FT), tsd[:, :, iz].astype(FT)
            fs, fsd = np.asarray(fscatt[:, iz], dtype=FT), fscatt_dot[:, :, iz]
            att = np.exp(-ts / ms)
            g0_all = fs * att
            sp, sm = np.zeros((S, N), dtype=FT), np.zeros((S, N), dtype=FT)
            spd, smd = np.zeros((pl, S, N), dtype=FT), np.zeros((pl, S, N), dtype=FT)
            for shift, w_ie in zip(rs.i_shift, rs.varpi_ie):
                n0, n1 = OR.get_n0_n1(S, int(shift))
                if n1.stop <= n1.start:
                    continue
                G, G0, G1, H, H0, H1 = line_partials(sun, tau[n0], tau[n1], mu, ms, FT, naive_close)
                cp = wct02 * FT(w_ie) * np.einsum("ik,ks->si", Zpp[:, i_start:i_start + n], F0[:, n0])
                cm = wct02 * FT(w_ie) * np.einsum("ik,ks->si", Zmp[:, i_start:i_start + n], F0[:, n0])
                g0 = g0_all[n0][:, None]
                sp[n1] += cp * g0 * G
                sm[n1] += cm * g0 * H
                for p in range(pl):
                    gd = (fsd[p][n0] * att[n0] - g0_all[n0] * tsd_z[n0, p] / ms)[:, None]
                    d0d, d1d = td[n0, p][:, None], td[n1, p][:, None]
                    spd[p, n1] += cp * (gd * G + g0 * (G0 * d0d + G1 * d1d))
                    smd[p, n1] += cm * (gd * H + g0 * (H0 * d0d + H1 * d1d))
            if iz == 0:
                Sp[...], Dp[...], Dm[...] = sp, spd, smd
            else:
                e1 = np.exp(-tau[:, None] / mu[None, :])
                es = np.exp(-ts[:, None] / mu[None, :])
                for p in range(pl):
                    Dp[p] = (Dp[p] - Sp * td[:, p][:, None] / mu[None, :]) * e1 + spd[p]
                    Dm[p] = Dm[p] + (smd[p] - sm * tsd_z[:, p][:, None] / mu[None, :]) * es
                Sp[...] = Sp * e1 + sp
        for p in range(pl):
            cl = O.CompositeLayer(None, None, None, None, Dp[p], Dm[p])
            r, t = np.zeros((nV, n, S), dtype=FT), np.zeros((nV, n, S), dtype=FT)
            O.postprocessing_vza(pol, cl, model.vza, model.vaz, qp, m, weight, r, t)
            ieRd[..., p] += r
            ieTd[..., p] += t
    return fwd[0], fwd[1], fwd[2], fwd[3], Rd, Td, ieRd, ieTd
