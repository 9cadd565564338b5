"""Seeded synthetic line tables, isotopologue data and profiles shared by the Absorption tests (CPU and GPU), in the two forms
the tests need: the dict of arrays tests/absorption_oracle.py takes and the public objects of vsm.Absorption."""
import os

import numpy as np

# the reference's 16-line test/test_profiles/testCO2.data, unchanged
GOLDEN_PAR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hitran_testCO2.par")

# Two made-up isotopologues with different mass and partition tables (this project ships no TIPS table): Q(T) smooth and growing,
# tabulated coarsely enough that the spline matters.
_TT = np.arange(100.0, 420.0, 20.0)
ISOTOPOLOGUES = {
    (2, 1): (43.98983, _TT, 286.09 * (_TT / 296.0) ** 1.02 * (1.0 + 0.04 * (_TT / 296.0) ** 3)),
    (7, 1): (31.98983, _TT, 215.73 * (_TT / 296.0) ** 1.01 * (1.0 + 0.002 * (_TT / 296.0) ** 2)),
}

# 0.1 .. 1013 hPa and 180 .. 320 K: with the widths below y = sqrt(ln 2) gamma_l / gamma_d runs from about 1e-4 to about 10
P3, T3 = np.array([0.1, 97.3, 1013.0]), np.array([180.0, 251.5, 320.0])
P1, T1 = np.array([301.7]), np.array([223.4])


def uniform_grid(n, lo=6000.0, hi=6050.0):
    return np.array([0.5 * (lo + hi)]) if n == 1 else np.linspace(lo, hi, n)


def nonuniform_grid(n, seed, lo=6000.0, hi=6050.0):
    """Strictly ascending, steps varying by a factor of about 20."""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.1, 2.0, n - 1)
    g = np.concatenate([[0.0], np.cumsum(steps)])
    return lo + (hi - lo) * g / g[-1]


def synthetic_table(seed, n_lines, lo=6015.0, hi=6035.0, two_species=False, no_E_share=0.0):
    """n_lines lines with nu0 in (lo, hi), unsorted (the host sorts), strengths over four decades, both signs of delta_air."""
    rng = np.random.default_rng(seed)
    t = dict(
        mol=np.full(n_lines, 2), iso=np.ones(n_lines, dtype=int),
        nu=rng.uniform(lo, hi, n_lines), S=10.0 ** rng.uniform(-26.0, -22.0, n_lines),
        gamma_air=rng.uniform(0.03, 0.1, n_lines), gamma_self=rng.uniform(0.04, 0.13, n_lines),
        n_air=rng.uniform(0.5, 0.8, n_lines), delta_air=rng.uniform(-0.012, 0.006, n_lines),
        E_low=rng.uniform(0.0, 2500.0, n_lines))
    if two_species:
        t["mol"] = np.where(rng.uniform(size=n_lines) < 0.4, 7, 2)
    if no_E_share > 0:
        t["E_low"] = np.where(rng.uniform(size=n_lines) < no_E_share, -1.0, t["E_low"])
    return t


def deviation_case():
    """(table, grid, wing_cutoff, p, T): one line with negative delta_air just inside the unshifted filter (nu0 > grid[0] - cutoff)
    whose window at p = 1013.25 hPa ends below grid[0]: 5999.001 - 0.01 + 1 = 5999.991 < 6000."""
    t = dict(mol=np.array([2]), iso=np.array([1]), nu=np.array([5999.001]), S=np.array([1e-22]), gamma_air=np.array([0.07]),
             gamma_self=np.array([0.09]), n_air=np.array([0.7]), delta_air=np.array([-0.01]), E_low=np.array([300.0]))
    return t, np.linspace(6000.0, 6010.0, 101), 1.0, np.array([1013.25]), np.array([296.0 - 10.0])


def hitran_table(A, t):
    z = np.zeros(len(t["nu"]))
    return A.HitranTable(mol=t["mol"], iso=t["iso"], nu=t["nu"], S=t["S"], A=z, gamma_air=t["gamma_air"], gamma_self=t["gamma_self"],
                         E_low=t["E_low"], n_air=t["n_air"], delta_air=t["delta_air"])


def table_dict(ht):
    return dict(mol=ht.mol, iso=ht.iso, nu=ht.nu, S=ht.S, gamma_air=ht.gamma_air, gamma_self=ht.gamma_self, n_air=ht.n_air,
                delta_air=ht.delta_air, E_low=ht.E_low)


def isotopologues(A):
    return {k: A.IsotopologueData(*v) for k, v in ISOTOPOLOGUES.items()}


def make_model(A, t, broadening="Voigt", cef="HumlicekWeidemann32SDErrorFunction", wing_cutoff=5.0, vmr=0.0, architecture=None):
    return A.make_hitran_model(hitran_table(A, t), getattr(A, broadening)(), wing_cutoff=wing_cutoff, vmr=vmr, CEF=getattr(A, cef)(),
                               architecture=architecture, isotopologues=isotopologues(A))
