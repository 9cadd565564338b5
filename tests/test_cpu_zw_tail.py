"""CPU model of the zero-weight tail of the FP64 native layer kernels (VSM_RUN_ZW_TAIL, csrc/vsm_native_dev.h nmm / nzw_fix):
the VZA / SZA nodes that rt_set_streams appends with weight 0 give every matrix of the doubling and interaction recurrences columns
that are zero off the diagonal, so the products may skip the k-steps of those streams and add A[k, k] B[k, :] instead.
Also the choice of the k-steps formed per block (zw_tail in vsm_native.hip)."""
import numpy as np
import pytest

from oracle import vsm_oracle as O


def _zw_cols(qp):
    return np.flatnonzero(qp.wt_muN == 0.0)


def _offdiag_max(M, cols):
    """largest |M[i, j]|, i != j, over the zero-weight columns j (M: [S, N, N])"""
    X = M[:, :, cols].copy()
    X[:, cols, np.arange(len(cols))] = 0.0
    return np.max(np.abs(X)) if X.size else 0.0


def _series_inv(A):
    """(I - E)^-1 by the Neumann series in plain products (the kernels' Horner path), E = I - A"""
    E = np.eye(A.shape[-1])[None] - A
    G = np.eye(A.shape[-1])[None] + E
    P = E
    for _ in range(80):
        P = P @ E
        G = G + P
        if np.max(np.abs(P)) < 1e-30:
            break
    return G


def _scene(pol_name, vza, depol=0.03, sza=40.0, l_trunc=34, tau=(0.05, 0.4), m=0):
    pol = O.polarization(pol_name)
    qp = O.rt_set_streams_gausslegquad(l_trunc, sza, vza, pol)
    N = len(qp.qp_muN)
    greek = O.get_greek_rayleigh(depol)
    Zpp, Zmp = O.compute_Z_moments(pol, qp.qp_mu, greek, m)
    return pol, qp, N, Zpp, Zmp


@pytest.mark.parametrize("pol_name", ["I", "IQU"])
@pytest.mark.parametrize("m", [0, 1, 2])
def test_recurrences_keep_zero_weight_columns_exactly(pol_name, m, monkeypatch):
    """elemental -> ndoubl doubling steps -> interactions (full and sources-only association): every zero-weight column of every
    matrix is exactly 0.0 off the diagonal (series inverses; the pivoted inverse keeps it only up to rounding)."""
    monkeypatch.setattr(O, "batch_inv", _series_inv)
    pol, qp, N, Zpp, Zmp = _scene(pol_name, [0.0, 25.0], m=m)
    cols = _zw_cols(qp)
    assert len(cols) == 3 * pol.n
    S = 2
    comp = O.make_composite_layer(np.float64, N, S)
    F0 = np.zeros((pol.n, S))
    F0[0] = 1.0
    tau_sum = np.zeros(S)
    for iz, (dtau, varpi, nd) in enumerate([(0.02, 0.9, 2), (0.005, 0.99, 4), (0.01, 0.5, 3)]):
        add = O.make_added_layer(np.float64, N, S)
        dt = np.full(S, dtau)
        O.elemental(pol, tau_sum, dt, F0, np.full(S, varpi), Zpp, Zmp, m, nd, qp, add, np.float64)
        for M in (add.r_mp, add.t_pp):
            assert _offdiag_max(M, cols) == 0.0
        O.doubling(pol, np.exp(-dt / qp.mu0), nd, add, np.float64)
        for M in (add.r_mp, add.r_pm, add.t_pp, add.t_mm):
            assert _offdiag_max(M, cols) == 0.0
        if iz == 0:
            O.copy_added_to_composite(comp, add)
        else:
            # the sources-only association: E1 = r-+ R+-, G1, P = t++ R+-, W = G1 t--
            E1 = add.r_mp @ comp.R_pm
            G1 = _series_inv(np.eye(N)[None] - E1)
            for M in (E1, G1, add.t_pp @ comp.R_pm, G1 @ add.t_mm, comp.T_mm @ G1 @ add.t_mm):
                assert _offdiag_max(M, cols) == 0.0
            O.interaction("11", comp, add, np.float64)
        for M in (comp.R_mp, comp.R_pm, comp.T_pp, comp.T_mm):
            assert _offdiag_max(M, cols) == 0.0
        tau_sum = tau_sum + dt * 2 ** nd


def test_pivoted_inverse_keeps_the_columns_up_to_rounding():
    """G of a pivoted inverse (LAPACK getrf: the kernels' ngj_lds keeps the dense products for exactly this reason) is in the
    class up to rounding only: its off-diagonal zero-weight entries are at most ~1e-16 of the matrix."""
    pol, qp, N, Zpp, Zmp = _scene("IQU", [0.0])
    cols = _zw_cols(qp)
    S = 1
    add = O.make_added_layer(np.float64, N, S)
    O.elemental(pol, np.zeros(S), np.full(S, 3.0), np.ones((pol.n, S)), np.full(S, 0.999), Zpp, Zmp, 0, 0, qp, add, np.float64)
    G = np.linalg.inv(np.eye(N)[None] - add.r_mp @ add.r_mp)
    assert _offdiag_max(G, cols) <= 1e-15 * np.max(np.abs(G))


def _truncated(A, B, n_real):
    """nmm with KZ < KS: the MFMA k-steps over k < 4 KZ, then out[row] += A[row, row] B[row] for the rows of the skipped k-steps"""
    n = A.shape[0]
    KS, KZ = (n + 3) // 4, (n_real + 3) // 4
    k = 4 * KZ
    out = A[:, :k] @ B[:k]
    for row in range(k, min(4 * KS, n)):
        out[row] += A[row, row] * B[row]
    return out


@pytest.mark.parametrize("pol_name,vza", [("I", [0.0]), ("IQU", [0.0]), ("IQU", [0.0, 30.0, 60.0]), ("IQUV", [10.0, 20.0])])
def test_truncated_product_matches_dense(pol_name, vza):
    """the truncated product plus the fix-up equals the dense product to 1e-15 relative for left operands of the class, any right
    operand (rider columns included)"""
    pol, qp, N, Zpp, Zmp = _scene(pol_name, vza)
    S = 1
    add = O.make_added_layer(np.float64, N, S)
    O.elemental(pol, np.zeros(S), np.full(S, 0.1), np.ones((pol.n, S)), np.full(S, 0.9), Zpp, Zmp, 0, 1, qp, add, np.float64)
    O.doubling(pol, np.exp(-np.full(S, 0.1) / qp.mu0), 1, add, np.float64)
    n_real = int(np.count_nonzero(qp.wt_muN))
    rng = np.random.default_rng(len(vza))
    B = rng.standard_normal((N, N + 2))
    for A in (add.r_mp[0], add.t_pp[0], add.t_pp[0] @ add.r_mp[0], add.t_mm[0] @ add.t_mm[0]):
        dense = A @ B
        assert np.max(np.abs(_truncated(A, B, n_real) - dense)) <= 1e-15 * np.max(np.abs(dense))


def _kz(wt_nodes, ns, gsz):
    """zw_tail (vsm_native.hip): k-steps over real streams of a block of gsz components"""
    nq = len(wt_nodes)
    z = 0
    for w in wt_nodes[::-1]:
        if w != 0.0:
            break
        z += 1
    if z == nq:
        z = 0
    return ((nq - z) * gsz + 3) // 4


def test_kz_selection():
    pol = O.polarization("IQU")
    # C2: 18 Gauss-Legendre nodes + one VZA + the SZA -> dense 60 rows, m = 0 (I,Q) block 40 rows
    qp = O.rt_set_streams_gausslegquad(34, 40.0, [0.0], pol)
    assert qp.Nquad == 20 and qp.Nstreams == 18
    assert ((60 + 3) // 4, _kz(qp.wt_mu, 3, 3)) == (15, 14)
    assert ((40 + 3) // 4, _kz(qp.wt_mu, 3, 2)) == (10, 9)
    assert _kz(qp.wt_mu, 3, 1) == 5   # U block of m = 0: 20 rows, no whole k-step of zero-weight streams
    # a VZA on a Gauss-Legendre node and the SZA too: no zero-weight node is left
    x, _ = O.gauleg(18, 0.0, 1.0)
    on = float(np.degrees(np.arccos(x[3])))
    q2 = O.rt_set_streams_gausslegquad(34, on, [on], pol)
    if q2.Nquad == 18:
        assert _kz(q2.wt_mu, 3, 3) == 15
    # three VZAs: a tail of two or more k-steps in the dense block
    q3 = O.rt_set_streams_gausslegquad(34, 40.0, [0.0, 30.0, 60.0], pol)
    assert (q3.Nquad * 3 + 3) // 4 - _kz(q3.wt_mu, 3, 3) >= 2
    # zero weights that are not trailing do not count
    w = np.ones(20)
    w[5] = 0.0
    assert _kz(w, 3, 3) == 15
    w[-1] = 0.0
    assert _kz(w, 3, 3) == 15   # (57 real rows: the last k-step still holds real rows)
    w[-2] = 0.0
    assert _kz(w, 3, 3) == 14
