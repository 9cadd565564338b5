"""CPU model of the sources-only interaction of the FP64 native layer kernel (csrc/vsm_native.hip, nia_body_src): the
re-associated interaction_helper!(::ScatteringInterface_11) (interaction.jl:207-266) around G1 = (I - r-+ R+-)^-1, with the source
terms riding in the spare column c1 = 4 KS of the padded strips, against the oracle's interaction.  Also the order-7 form of the
inverse and the mode switch of core_rt."""
import numpy as np
import pytest

from oracle import vsm_oracle as O

EPS = np.finfo(np.float64).eps


def _series_order(nrm):
    """nseries_order (vsm_native_dev.h): 0 = the pivoted inverse."""
    if not nrm < 0.3:
        return 0
    lim = EPS * 0.25 * (1.0 - nrm)
    n2 = nrm * nrm
    n4, n8 = n2 * n2, n2 * n2 * n2 * n2
    n16 = n8 * n8
    for K, v in ((1, n2), (2, n2 * nrm), (3, n4), (4, n4 * nrm), (7, n8), (8, n8 * nrm), (15, n16), (16, n16 * nrm), (31, n16 * n16)):
        if v <= lim:
            return K
    return 0


def _inverse(E, n):
    """G = (I - E)^-1 of the kernel's paths, on the padded matrix (rider columns kept, as the series leaves them)."""
    NP = E.shape[0]
    I = np.zeros((NP, NP))
    I[np.arange(n), np.arange(n)] = 1.0
    Ek = E.copy()
    Ek[:, n:] = 0.0
    K = _series_order(np.sqrt(np.sum(E[:, :n] ** 2)) * 1.001)
    if K == 0:
        G = np.zeros((NP, NP))
        G[:n, :n] = np.linalg.inv(np.eye(n) - E[:n, :n])
        return G, K
    if K == 7:   # ninvert7: (I + E)(I + E^2)(I + E^4) in four products
        X = E + Ek @ E
        Y = E + Ek @ X
        W4 = Ek @ (Y - X)
        return I + Y + W4 + W4[:, :n] @ Y[:n], K
    G = E.copy()
    for _ in range(K - 1):   # Horner: X_{j+1} = E + E X_j
        G = E + Ek @ G
    return I + G, K


def _src_interaction(n, comp, add):
    """nia_body_src on padded strips (NP = 16 RT rows and columns, c1 = 4 KS): returns R+-', T--', J0+', J0-'."""
    KS = (n + 3) // 4
    RT = KS // 4 if (KS % 4 == 0) else (4 * KS + 2 + 15) // 16
    NP, c1 = 16 * RT, 4 * KS
    rid = c1 + 1 < NP

    def pad(A):
        P = np.zeros((NP, NP))
        P[:n, :n] = A
        return P

    def pv(v):
        P = np.zeros(NP)
        P[:n] = v
        return P

    def mm(A, B):   # [A] B: the contraction runs over k < 4 KS only
        return A[:, :c1] @ B[:c1]

    r_mp, r_pm, t_pp, t_mm = pad(add.r_mp), pad(add.r_pm), pad(add.t_pp), pad(add.t_mm)
    j0p, j0m = pv(add.j0_p), pv(add.j0_m)
    R_pm, T_mm = pad(comp.R_pm), pad(comp.T_mm)
    J0p, J0m = pv(comp.J0_p), pv(comp.J0_m)
    B = R_pm.copy()
    Bs = t_mm.copy()
    addend = r_pm.copy()
    if rid:
        B[:, c1] = J0p
    E, P = mm(r_mp, B), mm(t_pp, B)
    if rid:
        Bs[:, c1] = E[:, c1] + j0m
        addend[:, c1] = P[:, c1] + j0p
    else:
        u, tJ = r_mp @ J0p + j0m, t_pp @ J0p + j0p
    G, K = _inverse(E, n)
    W = mm(G, Bs)
    Tn = mm(T_mm, W)
    Rn = addend + mm(P, W)
    if rid:
        return Rn[:n, :n], Tn[:n, :n], Rn[:n, c1], J0m[:n] + Tn[:n, c1], K
    g = G[:, :c1] @ u[:c1]
    return Rn[:n, :n], Tn[:n, :n], (tJ + P @ g)[:n], (J0m + T_mm @ g)[:n], K


def _layers(n, scale, dsym, rng):
    refl = lambda s: s * rng.random((n, n)) / n
    trans = lambda: np.diag(rng.uniform(0.3, 0.95, n)) + 0.05 * rng.random((n, n)) / n
    comp = O.CompositeLayer(refl(scale), refl(scale), trans(), trans(), rng.random(n), rng.random(n))
    r, t = refl(scale), trans()
    if dsym:
        D = np.where(np.arange(n) % 3 >= 2, -1.0, 1.0)
        add = O.AddedLayer(r, t, D[:, None] * r * D[None], D[:, None] * t * D[None], rng.random(n), rng.random(n))
    else:
        add = O.AddedLayer(r, t, refl(scale), trans(), rng.random(n), rng.random(n))
    return comp, add


def _batch(x):
    return np.asarray(x)[None].copy()


@pytest.mark.parametrize("n", [5, 12, 15, 16, 20, 30, 40, 45, 52, 60, 64, 68, 96])
@pytest.mark.parametrize("scale", [1e-4, 1e-2, 0.05, 0.1, 0.3, 1.0, 1.9])
@pytest.mark.parametrize("dsym", [True, False])
def test_reassociated_interaction_matches_oracle(n, scale, dsym):
    """J0+-, R+- and T-- of the rider-column form equal interaction_helper!(_11) to 1e-13 relative (||R r|| from ~1e-4 to ~0.5)."""
    rng = np.random.default_rng(1000 * n + int(100 * scale) + dsym)
    comp, add = _layers(n, scale, dsym, rng)
    Rn, Tn, Jp, Jm, _ = _src_interaction(n, comp, add)
    c = O.CompositeLayer(*(_batch(getattr(comp, k)) for k in ("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m")))
    a = O.AddedLayer(*(_batch(getattr(add, k)) for k in ("r_mp", "t_pp", "r_pm", "t_mm", "j0_p", "j0_m")))
    O.interaction("11", c, a, np.float64)
    rel = lambda x, y: np.max(np.abs(x - y)) / np.max(np.abs(y))
    assert rel(Rn, c.R_pm[0]) < 1e-13
    assert rel(Tn, c.T_mm[0]) < 1e-13
    assert rel(Jp, c.J0_p[0]) < 1e-13
    assert rel(Jm, c.J0_m[0]) < 1e-13


def test_every_inverse_path_is_exercised():
    """The scales above reach the Horner orders, order 7, the long series and the pivoted inverse."""
    seen = set()
    for n in (20, 60):
        for scale in (1e-4, 1e-2, 0.05, 0.1, 0.3, 1.0, 1.9):
            comp, add = _layers(n, scale, True, np.random.default_rng(n))
            seen.add(_src_interaction(n, comp, add)[4])
    assert 0 in seen and 7 in seen and any(1 <= k <= 4 for k in seen) and any(k >= 15 for k in seen), seen


def test_mode_switch_defaults():
    """The sources-only run is the default of Scene.run, beside NATIVE_RUN; full runs stay reachable on the same build."""
    import inspect

    import vsmartmom_jl_amd as vsm
    CR = vsm.CoreRT
    assert CR.NATIVE_SOURCES_ONLY is True and CR.NATIVE_RUN is True
    sig = inspect.signature(CR.Scene._run_layers_native)
    assert sig.parameters["sources_only"].default is True
    assert "vsm_run_create_ex_f64" in vsm._lib.exported_symbols() and "vsm_run_create_f64" in vsm._lib.exported_symbols()
