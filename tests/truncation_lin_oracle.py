"""Test oracle of Scattering.truncate_phase_lin: a numpy restatement of the reference's linearized delta-BGE truncation
(src/Scattering/truncate_phase_lin.jl) on top of tests/truncation_oracle.py and tests/mie_lin_oracle.py, float64 throughout.  It
imports nothing from the package.

Per system A x = b with A = sum_k w_k B_i B_j / f^2, b = sum_k w_k B_i / f (beta: B = P, f = f11; gamma, epsilon: B = fac P2,
f = f12, f34) and four derivative slots:

  solve_literal   the reference's text (:73-171): A'_s = -2 sum w B_i B_j f'_s / f^3,  b'_s = -sum w B_i f'_s / f^2,
                  x'_s = A^-1 (b'_s - A'_s x), with np.linalg.solve.
  solve_fused     what the device computes: with Bt_ik = sqrt(w_k) B_i(mu_k) / f_k (A = Bt Bt^T),  t = Bt^T x,
                  g_s = (f'_s / f) (2 t - sqrt(w)),  x'_s = A^-1 Bt g_s.  The same numbers in exact arithmetic: b'_s - A'_s x =
                  sum_k w B_i (f'_s / f^2) (2 (B x)_k / f - 1).
  closing_lin     :183-207.

f' at the nodes is reconstructed from all L derivative coefficients (reconstruct_lin) or handed over (mie_node_functions: the
linearized Mie oracle's bulk functions, normalised the way compute_NAI2_lin.jl normalises them).  A gamma (epsilon) series of exact
zeros from l = 2 on keeps exact-zero derivatives, as it keeps exact zeros in truncation_oracle."""
from __future__ import annotations

import numpy as np

import mie_oracle as MO
import truncation_oracle as TO

SYSTEMS = ("beta", "gamma", "epsilon")
ROWS = {"beta": (0, 1, 3, 5), "gamma": (2,), "epsilon": (4,)}     # the coefficient families a system's solution reaches


def reconstruct_lin(greek, greek_dot, mu):
    """f [3, n] = (f11, f12, f34) and f_dot [4, 3, n] at the nodes from all L coefficients and their derivatives, with P, P2."""
    L = greek.shape[1]
    P, P2, _, _ = MO.compute_legendre_poly(mu, L)
    fac = TO.prefactor(L)
    one = lambda g: np.stack([P @ g[1], P2 @ (fac * g[2]), P2 @ (fac * g[4])])
    return one(greek), np.stack([one(greek_dot[s]) for s in range(4)]), P, P2


def mie_node_functions(o):
    """(f [3, n], f_dot [4, 3, n]) of a mie_lin_oracle result: bulk_f / C_sca and (bulk_f' - (bulk_f / C_sca) C_sca') / C_sca for
    f11, f12, f34 (rows 0, 2, 3 of the bulk functions)."""
    rows = [0, 2, 3]
    f = o.bulk_f[rows] / o.C_sca
    return f, np.stack([(o.bulk_f_dot[s][rows] - f * o.C_sca_dot[s]) / o.C_sca for s in range(4)])


def problems(greek, greek_dot, l_max, f=None, f_dot=None):
    """Per system (B [n, size], f [n], f_dot [4, n], w [n]) or None for a skipped one."""
    L = greek.shape[1]
    mu, w = MO.gausslegendre(L)
    fr, fr_dot, P, P2 = reconstruct_lin(greek, greek_dot, mu)
    if f is None:
        f, f_dot = fr, fr_dot
    fac = TO.prefactor(l_max)
    B1 = P[:, :l_max]
    B2 = fac[2:] * P2[:, 2:l_max]
    out = []
    for k, (B, series) in enumerate(((B1, None), (B2, greek[2]), (B2, greek[4]))):
        skipped = series is not None and TO.zero_series(series)
        out.append(None if skipped else (B, np.asarray(f[k]), np.asarray(f_dot)[:, k], w))
    return out


def solve_literal(problem):
    """(x, x_dot [4, size]) of one system, the reference's text."""
    B, f, f_dot, w = problem
    G = B / f[:, None]
    A = (G * w[:, None]).T @ G
    x = np.linalg.solve(A, (w[:, None] * G).sum(axis=0))
    x_dot = []
    for s in range(4):
        A_dot = -2.0 * (B * (w * f_dot[s] / f ** 3)[:, None]).T @ B
        b_dot = -(B * (w * f_dot[s] / f ** 2)[:, None]).sum(axis=0)
        x_dot.append(np.linalg.solve(A, b_dot - A_dot @ x))
    return x, np.stack(x_dot)


def solve_fused(problem):
    """(x, x_dot [4, size]) of one system without any A': one product with Bt^T, one with Bt, four more solves with A."""
    B, f, f_dot, w = problem
    sw = np.sqrt(w)
    Bt = B * (sw / f)[:, None]                          # [n, size]: the device's rows, transposed
    A = Bt.T @ Bt
    x = np.linalg.solve(A, Bt.T @ sw)
    t = Bt @ x
    g = (f_dot / f) * (2.0 * t - sw)                    # [4, n]
    return x, np.linalg.solve(A, Bt.T @ g.T).T


def closing_lin(greek, greek_dot, greek_t, c0, xb_dot, gam_dot, eps_dot, l_max):
    """truncate_phase_lin.jl:183-207: greek_t_dot [4, 6, l_max], c0_dot [4], f_trunc_dot [4] = -c0_dot.  gam_dot, eps_dot
    [4, l_max] with their two leading zeros; they are not divided by c0, as the forward fit's are not."""
    out = np.zeros((4, 6, l_max))
    for s in range(4):
        cd = xb_dot[s, 0]
        cut = greek_dot[s, 1, :l_max] - xb_dot[s]
        out[s, 1] = (xb_dot[s] - greek_t[1] * cd) / c0
        for row in (0, 3, 5):
            out[s, row] = (greek_dot[s, row, :l_max] - cut - greek_t[row] * cd) / c0
        out[s, 2], out[s, 4] = gam_dot[s], eps_dot[s]
    c0_dot = xb_dot[:, 0].copy()
    return out, c0_dot, -c0_dot


def truncate_phase_lin(greek, greek_dot, l_max, f=None, f_dot=None, solve=solve_literal):
    """truncate_phase(deltaBGE(l_max, .), aero, lin_aero) for greek [6, L], greek_dot [4, 6, L], L > l_max:
    (greek_t, c0, f_trunc) as truncation_oracle.truncate_phase returns them, then (greek_t_dot, c0_dot, f_trunc_dot)."""
    greek = np.asarray(greek, dtype=np.float64)
    greek_dot = np.asarray(greek_dot, dtype=np.float64)
    greek_t, c0, f_trunc = TO.truncate_phase(greek, l_max, None if f is None else tuple(f))
    dots = []
    for k, p in enumerate(problems(greek, greek_dot, l_max, f, f_dot)):
        size = l_max if k == 0 else l_max - 2
        dots.append(np.zeros((4, size)) if p is None else solve(p)[1])
    pad = lambda d: np.concatenate([np.zeros((4, 2)), d], axis=1)
    return (greek_t, c0, f_trunc) + closing_lin(greek, greek_dot, greek_t, c0, dots[0], pad(dots[1]), pad(dots[2]), l_max)


def form_disagreement(greek, greek_dot, l_max, f=None, f_dot=None):
    """d [3]: per system max |x'_literal - x'_fused| in units of max(1, max |x'_literal|) (0 for a skipped system): how far two
    algebraically equal forms of the reference's own formula lie apart in float64."""
    d = []
    for p in problems(np.asarray(greek, dtype=np.float64), np.asarray(greek_dot, dtype=np.float64), l_max, f, f_dot):
        if p is None:
            d.append(0.0)
            continue
        a, b = solve_literal(p)[1], solve_fused(p)[1]
        d.append(float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(a)))))
    return np.array(d)
