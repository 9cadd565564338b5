"""Seeded inputs shared by the continuum tests (CPU and GPU): CIA tables, an MT_CKD table, grids, profiles and the named sets, in the
form tests/continuum_oracle.py takes; `module_set` turns a set into the public objects of vsm.Absorption."""
import numpy as np

LAYERS = 4               # VSM_CONT_LAYERS; pinned to the library's getter in test_gpu_continuum.py
MAX_TABLES = 8           # VSM_CONT_MAX_TABLES

# block temperatures by nT
TS = {1: np.array([250.0]), 2: np.array([210.0, 290.0]), 5: np.array([200.0, 225.0, 250.0, 275.0, 300.0])}

# 11 layers (2 LAYERS + 3).  Against TS[5]: inside a cell, on an interior node, on the first node, on the last node, below, above;
# then the two nodes of TS[2] (on TS[1] every layer is clamped), and three more inside cells.  180 .. 320 K.
T_LAYERS = np.array([237.3, 250.0, 200.0, 300.0, 180.0, 320.0, 210.0, 290.0, 262.9, 225.0, 301.4])
P_LAYERS = np.array([1013.0, 840.2, 611.7, 433.0, 270.5, 151.9, 77.3, 31.8, 9.6, 2.2, 0.4])
DZ_LAYERS = np.array([812.0, 1530.5, 2240.0, 2611.3, 3050.0, 3502.7, 4120.0, 5230.9, 7011.0, 9400.0, 12350.0])
H2O_LAYERS = np.array([0.04, 0.013, 2.1e-3, 0.0, 3.3e-4, 5.0e-5, 1.0e-6, 4.2e-6, 7.7e-6, 0.021, 1.5e-4])
VMR = {"CO2": 4.1e-4, "CH4": np.linspace(1.9e-6, 0.4e-6, 11)}

SET_PAIRS = {
    "AA": [("O2-O2", 5)],
    "AB": [("O2-N2", 2)],
    "three": [("O2-O2", 5), ("O2-N2", 2), ("N2-N2", 1)],
    "band": [],
    "three_band": [("O2-O2", 5), ("O2-N2", 2), ("N2-N2", 1)],
    "eight": [("O2-O2", 5), ("O2-N2", 2), ("N2-N2", 1), ("CO2-CO2", 2), ("N2-H2O", 5), ("H2O-H2O", 1), ("CH4-N2", 2), ("O2-CO2", 5)],
}
HAS_BAND = ("band", "three_band")


def grid(nSpec):
    """-15, 0 and 5 cm^-1, then up to 20500 (the MT_CKD table ends at 20000: the last points lie outside it)."""
    if nSpec == 1:
        return np.array([1600.0])
    if nSpec < 4:
        return np.array([-15.0, 0.0, 5.0])[:nSpec]
    return np.concatenate([[-15.0, 0.0, 5.0], np.linspace(50.0, 20500.0, nSpec - 3)])


def profile(Nz):
    vmr = {"H2O": H2O_LAYERS[:Nz].copy(), "CO2": VMR["CO2"], "CH4": VMR["CH4"][:Nz].copy()}
    return P_LAYERS[:Nz].copy(), T_LAYERS[:Nz].copy(), DZ_LAYERS[:Nz].copy(), vmr


def cia_values(seed, nSpec, nT):
    """sig [nSpec, nT]: 1e-47 .. 1e-44 with a stretch of exact zeros."""
    rng = np.random.default_rng(seed)
    sig = 10.0 ** rng.uniform(-47.0, -44.0, (nSpec, nT))
    if nSpec >= 8:
        lo = nSpec // 3
        sig[lo:lo + max(1, nSpec // 10)] = 0.0
    return sig


def mtckd_table(seed=7):
    """An MT_CKD-shaped table: nu = -20 : 10 : 20000, coefficients over some decades, texp in [0, 10] with exact zeros."""
    rng = np.random.default_rng(seed)
    nu = np.arange(-20.0, 20000.0 + 5.0, 10.0)
    n = len(nu)
    C_self = 10.0 ** rng.uniform(-28.0, -24.0, n)        # (tau of the band within a few decades of the CIA tables' on this profile:
    C_for = 10.0 ** rng.uniform(-30.0, -26.0, n)         #  a finite difference of the summed forward still resolves the tables)
    texp = rng.uniform(0.0, 10.0, n)
    texp[rng.uniform(size=n) < 0.1] = 0.0
    texp[100:140] = 0.0
    return dict(nu=nu, C_self=C_self, C_for=C_for, texp=texp, p_ref=1013.0, T_ref=296.0)


def oracle_set(name, g, CO):
    """(tables, band) of a named set on the grid g, in the oracle's form; CO is tests/continuum_oracle.py."""
    tables = []
    for i, (pair, nT) in enumerate(SET_PAIRS[name]):
        a, b = pair.split("-")
        tables.append((a, b, TS[nT], cia_values(100 * len(g) + 10 * i + nT, len(g), nT)))
    band = None
    if name in HAS_BAND:
        t = mtckd_table()
        Cs, Cf, te = CO.mtckd_band(t["nu"], t["C_self"], t["C_for"], t["texp"], g)
        band = dict(nu=g, C_self=Cs, C_for=Cf, texp=te, p_ref=t["p_ref"], T_ref=t["T_ref"])
    return tables, band


def module_set(A, tables, band, g, arch=None):
    """The same set as CIATable / MTCKDBand objects."""
    members = [A.CIATable.from_arrays("%s-%s" % (a, b), Ts, sig, g, architecture=arch) for a, b, Ts, sig in tables]
    if band is not None:
        members.append(A.MTCKDBand(band["C_self"], band["C_for"], band["texp"], band["p_ref"], band["T_ref"], g, architecture=arch))
    return members
