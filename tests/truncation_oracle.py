"""Test oracle of Scattering.truncate_phase: a numpy restatement of the reference's delta-BGE truncation
(src/Scattering/truncate_phase.jl) on top of tests/mie_oracle.py, float64 throughout.  It imports nothing from the package.

truncate_phase (:149-273) is the variant the reference applies to Mie optics: three normal-equation systems over all Gauss-Legendre
nodes with the weights w / f^2, solved with np.linalg.solve.  truncate_phase_lowconf (:56-128) fits only the nodes with
mu < cos(delta_angle), weights w / max(|y|, 1e-8), with np.linalg.lstsq.  Both return (greek_t [6, l_max], c0, f_trunc = 1 - c0).

One place where this is not the reference's text: a gamma (epsilon) series of exact zeros from l = 2 on is returned
as exact zeros; the reference divides by f12 = 0 there and returns NaN.
"""
from __future__ import annotations

import math

import numpy as np

import mie_oracle as MO


def prefactor(n):
    """fac[l] = sqrt(1 / ((l - 1) l (l + 1) (l + 2))) for 2 <= l < n, else 0."""
    fac = np.zeros(n)
    for l in range(2, n):
        fac[l] = math.sqrt(1 / ((l - 1) * l * (l + 1) * (l + 2)))
    return fac


def reconstruct(greek, mu):
    """reconstruct_phase(greek_coefs, mu; returnLeg = true): f11, f12, f34, P, P2 with all len(beta) moments."""
    L = greek.shape[1]
    P, P2, _, _ = MO.compute_legendre_poly(mu, L)
    fac = prefactor(L)
    return P @ greek[1], P2 @ (fac * greek[2]), P2 @ (fac * greek[4]), P, P2


def zero_series(c):
    return not np.any(c[2:] != 0.0)


def closing(greek, cl, gamma_t, eps_t, l_max):
    """truncate_phase.jl:255-262 (the same lines in both variants)."""
    alpha, beta, _, delta, _, zeta = greek
    c0 = float(cl[0])
    cut = beta[:l_max] - cl
    out = np.stack([(alpha[:l_max] - cut) / c0, cl / c0, gamma_t, (delta[:l_max] - cut) / c0, eps_t, (zeta[:l_max] - cut) / c0])
    return out, c0, 1.0 - c0


def normal_equations(greek, l_max, f=None):
    """The three systems of truncate_phase (:182-247): [(A, b)] for beta (size l_max), gamma, epsilon (size l_max - 2; None for a
    series of exact zeros).  f = (f11, f12, f34) at the nodes replaces the reconstruction."""
    L = greek.shape[1]
    mu, w = MO.gausslegendre(L)
    f11, f12, f34, P, P2 = reconstruct(greek, mu)
    if f is not None:
        f11, f12, f34 = f
    fac = prefactor(l_max)
    B1 = P[:, :l_max]
    B2 = fac[2:] * P2[:, 2:l_max]
    out = []
    for B, y, series in ((B1, f11, None), (B2, f12, greek[2]), (B2, f34, greek[4])):
        if series is not None and zero_series(series):
            out.append(None)
            continue
        G = B / y[:, None]
        out.append(((G * w[:, None]).T @ G, (w[:, None] * G).sum(axis=0)))
    return out


def truncate_phase(greek, l_max, f=None):
    """truncate_phase(deltaBGE(l_max, .), aero) for greek [6, L], L > l_max."""
    greek = np.asarray(greek, dtype=np.float64)
    sol = [None if s is None else np.linalg.solve(*s) for s in normal_equations(greek, l_max, f)]
    tail = [np.zeros(l_max) if s is None else np.concatenate([[0.0, 0.0], s]) for s in sol[1:]]
    return closing(greek, sol[0], tail[0], tail[1], l_max)


def lowconf_problems(greek, l_max, delta_angle):
    """The three least-squares problems (W A, W y) of truncate_phase_lowconf (:71-98)."""
    L = greek.shape[1]
    mu, w = MO.gausslegendre(L)
    f11, f12, f34, P, P2 = reconstruct(greek, mu)
    sel = mu < math.cos(math.radians(delta_angle))
    fac = prefactor(l_max)
    A = P[sel, :l_max]
    B = fac[2:] * P2[sel][:, 2:l_max]
    out = []
    for M, y, series in ((A, f11[sel], None), (B, f12[sel], greek[2]), (B, f34[sel], greek[4])):
        if series is not None and zero_series(series):
            out.append(None)
            continue
        W = w[sel] / np.maximum(np.abs(y), 1e-8)
        out.append((W[:, None] * M, W * y))
    return out


def truncate_phase_lowconf(greek, l_max, delta_angle):
    """truncate_phase_lowconf(deltaBGE(l_max, delta_angle), aero) for greek [6, L], L > l_max."""
    greek = np.asarray(greek, dtype=np.float64)
    sol = [None if p is None else np.linalg.lstsq(p[0], p[1], rcond=None)[0] for p in lowconf_problems(greek, l_max, delta_angle)]
    tail = [np.zeros(l_max) if s is None else np.concatenate([[0.0, 0.0], s]) for s in sol[1:]]
    return closing(greek, sol[0], tail[0], tail[1], l_max)


def henyey_greenstein_greek(g, n):
    """Scalar Henyey-Greenstein series: beta_l = (2 l + 1) g^l, everything else zero."""
    greek = np.zeros((6, n))
    l = np.arange(n)
    greek[1] = (2 * l + 1) * float(g) ** l
    return greek
