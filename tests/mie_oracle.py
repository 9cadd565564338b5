"""Test oracle of vsm.Scattering: a numpy restatement of the reference's NAI-2 Mie path (src/Scattering/compute_NAI2.jl,
mie_helper_functions.jl, legendre_functions.jl), in float64 -- and, with dtype = np.longdouble, in the x87 format (64-bit mantissa)
on the same float64 inputs: the reference against which the float64 path's own rounding is measured (tests/test_oracle_mie.py,
tests/test_gpu_mie_edges.py).  The float64 path is the default and is pinned to the bit by recorded values.  It imports nothing
from the package.

get_n_max, compute_mie_ab, compute_mie_pi_tau, compute_mie_S1S2, gauleg_log, compute_wx, compute_legendre_poly restate the
functions of the same names; the recurrences run in the reference's order of operations, vectorised over the radii (and, for the
Legendre functions, over the angles) only.  nai2_reference takes what vsm_mie_nai2 takes and returns what it returns;
mie_inputs is the host part (compute_NAI2.jl:80-113, :161); compute_aerosol_optical_properties chains the two.

Two places where this is not the reference's text, both stated in DESIGN.md 4.21:
  * D_n(y) starts its downward recurrence at the radius' own nmx_i = round(max(n_max_i, |y_i|) + 51); compute_NAI2.jl hands every
    radius the buffer of the largest one.  The recurrence has converged long before n_max_i either way.
  * n_max = max(get_n_max(x_max), 2): compute_mie_pi_tau writes two orders and compute_legendre_poly two moments, so the
    reference cannot run a distribution whose largest x gives n_max = 1 (x < 0.0019) at all.
The result's f_trunc is 0 (untruncated coefficients); the reference stores 1 there and relies on a later truncate_phase.
"""
from __future__ import annotations

import math
import statistics
import types

import numpy as np


# ---- size distributions (Distributions.jl LogNormal(mu, sigma) as the reference's LogNormal(log(r_m), log(sigma_g))) ----------
class LogNormal:
    def __init__(self, r_m, sigma_g):
        self.mu, self.sigma = math.log(r_m), math.log(sigma_g)

    def pdf(self, r):
        r = np.asarray(r, dtype=np.float64)
        z = (np.log(r) - self.mu) / self.sigma
        return np.exp(-0.5 * z * z) / (r * self.sigma * math.sqrt(2 * math.pi))

    def quantile(self, p):
        return math.exp(self.mu + self.sigma * statistics.NormalDist().inv_cdf(p))


# ---- mie_helper_functions.jl ---------------------------------------------------------------------------------------------
def get_n_max(x):
    """mie_helper_functions.jl:22 (round = to nearest, ties to even, as Julia's round(Int, .))."""
    x = float(x)
    return int(round(x + 4.05 * x ** (1 / 3) + 10)) if x > 8.0 else int(round(x + 4.0 * x ** (1 / 3) + 1))


def arithmetic(dtype):
    """(real type, complex type, pi) of np.float64 -- the default everywhere, the oracle as it always was, to the bit -- or of
    np.longdouble with np.clongdouble.  The inputs are the same float64 arrays in both; only the arithmetic widens."""
    if dtype == np.float64:
        return np.float64, np.complex128, math.pi
    if dtype == np.longdouble:
        return np.longdouble, np.clongdouble, 4 * np.arctan(np.longdouble(1))
    raise ValueError("dtype %r: np.float64 or np.longdouble" % (dtype,))


def start_orders(x, m, nmax_i):
    """nmx_i = round(max(n_max_i, |y_i|) + 51), in float64 whatever the arithmetic: both formats walk the same recurrence."""
    y = np.asarray(x, dtype=np.float64) * complex(m)
    return np.rint(np.maximum(np.asarray(nmax_i, dtype=np.int64), np.abs(y)) + 51).astype(np.int64)


def compute_mie_ab(x, m, nmax_i, n_max, dtype=np.float64):
    """compute_mie_ab! (:42-88) for every radius at once: a_n, b_n [n_max, nquad] complex, exact zeros above n_max_i."""
    R, Cx, _ = arithmetic(dtype)
    nmx = start_orders(x, m, nmax_i)
    x = np.asarray(x, dtype=np.float64).astype(R)
    m = complex(m) if R is np.float64 else Cx(m)
    nq = len(x)
    nmax_i = np.asarray(nmax_i, dtype=np.int64)
    y = x * m
    Dn = np.zeros((n_max + 1, nq), dtype=Cx)                      # Dn[n], 1 <= n <= n_max, of each radius
    prev = np.zeros(nq, dtype=Cx)
    for n in range(int(nmx.max()) - 1, 0, -1):
        on = n <= nmx - 1
        ratio = (n + 1) / y
        prev = np.where(on, ratio - 1 / (prev + ratio), prev)
        if n <= n_max:
            Dn[n] = prev
    an = np.zeros((n_max, nq), dtype=Cx)
    bn = np.zeros((n_max, nq), dtype=Cx)
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
            psi0, psi1, chi0, chi1 = psi1, psi, chi1, chi
            xi1 = psi1 + 1j * chi1
    return an, bn


def compute_mie_S1S2(an, bn, pi_, tau_, dtype=np.float64):
    """compute_mie_S1S2! (:307-320) for every radius: S1, S2 [n_mu, nquad]."""
    R = arithmetic(dtype)[0]
    n = np.arange(1, an.shape[0] + 1)
    if R is not np.float64:
        n = n.astype(R)
    c = ((2 * n + 1) / (n * (n + 1)))[:, None]
    return tau_ @ (c * an) + pi_ @ (c * bn), pi_ @ (c * an) + tau_ @ (c * bn)


def gausslegendre(n):
    return np.polynomial.legendre.leggauss(n)


def gauleg_log(n, r_min, r_max):
    """gauleg_log (:369-379), norm = false."""
    xi, w = gausslegendre(n)
    ln_min, ln_max = math.log(r_min), math.log(r_max)
    r = np.exp((ln_max - ln_min) / 2 * xi + (ln_max + ln_min) / 2)
    return r, w * r * (ln_max - ln_min) / 2


def compute_wx(size_distribution, w_r, r):
    """compute_w_x (:511-521)."""
    wx = size_distribution.pdf(r) * w_r
    return wx / np.sum(wx)


def get_greek_rayleigh(depol):
    """get_greek_rayleigh (:454-468): alpha, beta, gamma, delta, epsilon, zeta."""
    p = (1 - depol) / (1 + depol / 2)
    r = (1 - 2 * depol) / (1 - depol)
    return (np.array([0, 0, 3 * p]), np.array([1, 0, 0.5 * p]), np.array([0, 0, p * math.sqrt(1.5)]),
            np.array([0, 1.5 * p * r, 0]), np.zeros(3), np.zeros(3))


# ---- legendre_functions.jl -----------------------------------------------------------------------------------------------
def compute_mie_pi_tau(mu, nmax, dtype=np.float64):
    """compute_mie_pi_tau (:195-214): pi_n, tau_n [n_mu, nmax], n = 1 .. nmax in column n - 1."""
    R = arithmetic(dtype)[0]
    mu = np.asarray(mu, dtype=np.float64).astype(R)
    pi_ = np.zeros((len(mu), nmax), dtype=R)
    tau_ = np.zeros((len(mu), nmax), dtype=R)
    pi_[:, 0], pi_[:, 1] = 1.0, 3 * mu
    tau_[:, 0], tau_[:, 1] = mu, 6 * mu ** 2 - 3
    for n in range(2, nmax):
        pi_[:, n] = ((2 * n + 1) * mu * pi_[:, n - 1] - (n + 1) * pi_[:, n - 2]) / n
        tau_[:, n] = (n + 1) * mu * pi_[:, n] - (n + 2) * pi_[:, n - 1]
    return pi_, tau_


def compute_legendre_poly(x, nmax, dtype=np.float64):
    """compute_legendre_poly (:223-265): P, P2, R2, T2 [len(x), nmax], moment l in column l."""
    assert nmax > 1
    R = arithmetic(dtype)[0]
    x = np.asarray(x, dtype=np.float64).astype(R)
    P0, P2, R2, T2 = (np.zeros((len(x), nmax), dtype=R) for _ in range(4))
    P0[:, 0], P0[:, 1] = 1, x
    if nmax > 2:
        P2[:, 2] = 3 * (1 - x ** 2)
        R2[:, 2] = np.sqrt(R(1.5)) * (1 + x ** 2)
        T2[:, 2] = np.sqrt(R(6)) * x
    for n in range(2, nmax):
        l = n - 1
        P0[:, n] = ((2 * l + 1) * x * P0[:, n - 1] - l * P0[:, n - 2]) / (l + 1)
        if n > 2:
            ia = (2 * l + 1) * x
            ib = np.sqrt(R((l + 2) * (l - 2))) * (l + 2) / l
            ic = R(4.0) * (2 * l + 1) / ((l + 1) * l)
            id_ = np.sqrt(R((l + 3) * (l - 1))) * (l - 1) / (l + 1)
            P2[:, n] = (ia * P2[:, n - 1] - (l + 2) * P2[:, n - 2]) / (l - 1)
            R2[:, n] = (ia * R2[:, n - 1] - ib * R2[:, n - 2] - ic * T2[:, n - 1]) / id_
            T2[:, n] = (ia * T2[:, n - 1] - ib * T2[:, n - 2] - ic * R2[:, n - 1]) / id_
    return P0, P2, R2, T2


def reconstruct_phase(greek, mu):
    """reconstruct_phase (mie_helper_functions.jl:415-446): f11, f12 at the cosines mu from (alpha .. zeta) [6, l_max]."""
    l_max = greek.shape[1]
    P, P2, _, _ = compute_legendre_poly(mu, l_max)
    fac = np.zeros(l_max)
    for l in range(2, l_max):
        fac[l] = math.sqrt(1 / ((l - 1) * l * (l + 1) * (l + 2)))
    return P @ greek[1], P2 @ (fac * greek[2])


# ---- compute_NAI2.jl -----------------------------------------------------------------------------------------------------
def greek_quadrature(sets, mu, w_mu, dtype=np.float64):
    """The six quadratures of compute_NAI2.jl:188-202 for each set (b11, b33, b12, b34) [4, n_mu] of normalised functions at the
    nodes mu: [len(sets), 6, n_mu] (alpha, beta, gamma, delta, epsilon, zeta)."""
    R = arithmetic(dtype)[0]
    w_mu = np.asarray(w_mu, dtype=np.float64).astype(R)
    l_max = len(mu)
    P, P2, R2, T2 = compute_legendre_poly(mu, l_max, dtype)
    out = np.zeros((len(sets), 6, l_max), dtype=R)
    for v, (b11, b33, b12, b34) in enumerate(sets):
        for l in range(l_max):
            fac = R(2 * l + 1) / 2 * np.sqrt(1 / R((l - 1) * l * (l + 1) * (l + 2))) if l >= 2 else 0.0
            out[v, 3, l] = R(2 * l + 1) / 2 * (w_mu @ (b33 * P[:, l]))
            out[v, 1, l] = R(2 * l + 1) / 2 * (w_mu @ (b11 * P[:, l]))
            out[v, 2, l] = fac * (w_mu @ (b12 * P2[:, l]))
            out[v, 4, l] = fac * (w_mu @ (b34 * P2[:, l]))
            out[v, 5, l] = fac * (w_mu @ (b33 * R2[:, l] + b11 * T2[:, l]))
            out[v, 0, l] = fac * (w_mu @ (b11 * R2[:, l] + b33 * T2[:, l]))
    return out


def greek_from_bulk(bulk_f, C_sca, mu, w_mu, dtype=np.float64):
    """Stage 3 alone (compute_NAI2.jl:161-202): greek [6, n_mu] from the unnormalised bulk functions [4, n_mu] at the nodes and the
    bulk C_sca -- of the oracle's own stage 2 in nai2_reference, of the device's in the tests of its stage 3."""
    R = arithmetic(dtype)[0]
    return greek_quadrature([np.asarray(bulk_f).astype(R) / R(C_sca)], mu, w_mu, dtype)[0]


def nai2_reference(x, wx, wr, nmax_i, mu, w_mu, n_r, n_i, k_wave, n_max, dtype=np.float64, scales=False):
    """compute_aerosol_optical_properties (compute_NAI2.jl:99-202) from the host part's arrays: the inputs of vsm_mie_nai2.
    Returns greek [6, n_mu] (alpha, beta, gamma, delta, epsilon, zeta), (C_sca, C_ext, ssa), bulk_f [4, n_mu] (f11, f33, f12, f34,
    NOT yet divided by C_sca: stage 2's output).  scales = True adds the sums of the absolute terms behind the sums of stage 2, the
    scales a rounding error of theirs is measured on: bulk_abs [n_mu] = sum_i |wr_i 0.5 / x_i^2| (|S1|^2 + |S2|^2) per angle,
    c_abs = sum_i |wx_i| 2 pi / k^2 sum_n (2n + 1) (|a_n|^2 + |b_n|^2  and  |Re(a_n + b_n)|) for C_sca and C_ext."""
    R, _, pi = arithmetic(dtype)
    x, wx, wr = (np.asarray(a, dtype=np.float64).astype(R) for a in (x, wx, wr))
    m = complex(n_r, -n_i)
    pi_, tau_ = compute_mie_pi_tau(mu, n_max, dtype)
    an, bn = compute_mie_ab(x, m, nmax_i, n_max, dtype)
    S1, S2 = compute_mie_S1S2(an, bn, pi_, tau_, dtype)
    n_ = (2.0 * np.arange(1, n_max + 1) + 1)[:, None]
    C_sca = 2 * pi / k_wave ** 2 * np.sum(n_ * (np.abs(an) ** 2 + np.abs(bn) ** 2), axis=0)
    C_ext = 2 * pi / k_wave ** 2 * np.sum(n_ * np.real(an + bn), axis=0)
    inv_x2 = 0.5 / x ** 2
    f11 = inv_x2 * (np.abs(S1) ** 2 + np.abs(S2) ** 2)
    f33 = inv_x2 * np.real(S1 * np.conj(S2) + S2 * np.conj(S1))
    f12 = -inv_x2 * (np.abs(S1) ** 2 - np.abs(S2) ** 2)
    f34 = -inv_x2 * np.imag(S1 * np.conj(S2) - S2 * np.conj(S1))
    bulk_C_sca, bulk_C_ext = R(np.sum(wx * C_sca)), R(np.sum(wx * C_ext))
    bulk = np.stack([f11 @ wr, f33 @ wr, f12 @ wr, f34 @ wr])
    greek = greek_from_bulk(bulk, bulk_C_sca, mu, w_mu, dtype)
    out = greek, (bulk_C_sca, bulk_C_ext, bulk_C_sca / bulk_C_ext), bulk
    if scales:
        c_ext_abs = 2 * pi / k_wave ** 2 * np.sum(n_ * np.abs(np.real(an + bn)), axis=0)
        out += (types.SimpleNamespace(bulk_abs=f11 @ np.abs(wr), c_abs=(np.sum(np.abs(wx) * C_sca), np.sum(np.abs(wx) * c_ext_abs))),)
    return out


def mie_inputs(size_distribution, wavelength, r_max, nquad_radius, tabulated=None):
    """The host part (compute_NAI2.jl:80-100, :113, :161).  tabulated = (r, pdf * w_r): the nodes and unnormalised weights of any
    other distribution, in place of gauleg_log and the pdf."""
    if tabulated is None:
        r_min = max(size_distribution.quantile(1e-8), 1e-6 * r_max)
        r, w_r = gauleg_log(nquad_radius, r_min, r_max)
        wx = compute_wx(size_distribution, w_r, r)
    else:
        r = np.asarray(tabulated[0], dtype=np.float64)
        wx = np.asarray(tabulated[1], dtype=np.float64)
        wx = wx / np.sum(wx)
    k_wave = 2 * math.pi / wavelength
    x = k_wave * r
    nmax_i = np.array([get_n_max(v) for v in x], dtype=np.int32)
    n_max = max(get_n_max(np.max(x)), 2)
    n_mu = 2 * n_max - 1
    mu, w_mu = gausslegendre(n_mu)
    wr = 4 * math.pi * r ** 2 * wx
    return types.SimpleNamespace(r=r, wx=wx, wr=wr, x=x, nmax_i=nmax_i, n_max=n_max, n_mu=n_mu, mu=mu, w_mu=w_mu, k_wave=k_wave)


def compute_aerosol_optical_properties(size_distribution, n_r, n_i, wavelength, r_max, nquad_radius, tabulated=None):
    """compute_aerosol_optical_properties(model): greek [6, n_mu], ssa, k (= bulk C_ext), C_sca, bulk_f [4, n_mu] (normalised by
    C_sca), mu, and the host part."""
    assert n_i >= 0
    h = mie_inputs(size_distribution, wavelength, r_max, nquad_radius, tabulated)
    greek, (C_sca, C_ext, ssa), bulk = nai2_reference(h.x, h.wx, h.wr, h.nmax_i, h.mu, h.w_mu, n_r, n_i, h.k_wave, h.n_max)
    return types.SimpleNamespace(greek=greek, ssa=ssa, k=C_ext, C_sca=C_sca, C_ext=C_ext, bulk_f=bulk / C_sca, mu=h.mu, host=h)


MONO_WAVELENGTH = 2 * math.pi     # k = 2 pi / lambda = 1 exactly: a sphere of radius x has size parameter x to the bit


def monodisperse(x, n_r, n_i):
    """One sphere of size parameter x as a tabulated distribution of one node."""
    return compute_aerosol_optical_properties(None, n_r, n_i, MONO_WAVELENGTH, None, 1, tabulated=([x], [1.0]))
