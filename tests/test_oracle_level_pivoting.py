"""CPU checks of the inputs of tests/test_gpu_level_pivoting.py (tests/level_cases.py): conditions on the INPUTS, not on the
kernel.  For every N, both precisions and both kinds of bottom the GPU tests use, the `pivoting` family must

  * be well conditioned: kappa_1(I - A B) <= 10 at every point;
  * make the kernel's pivot rule (level_cases.kernel_pivot_trace) exchange a row at N / 2 steps or more, and for N > 64 find at
    least one pivot in a row >= 64 at a step k < 64 (the second ballot of the wave-0 search);
  * be solved by LAPACK in precision FT, on the system formed in precision FT, within a quarter of the GPU tests' tolerance
    (so the tolerance is not the obstacle);
  * be missed by the same elimination WITHOUT the exchange by 1000 tolerances or more, or come out non-finite (so a kernel that does
    not pivot cannot pass).

tol = max(floor, 50 kappa eps(FT)) with the floor of the elastic kernel's sibling test, 1e-11 (FP64) / 2e-4 (FP32): the smallest
floor any GPU test of the family uses in FP64 and the one most use in FP32 (the inelastic kernel's are 1e-10 / 5e-4)."""
import numpy as np
import pytest

import level_cases as LC

FLOOR = {np.float64: 1e-11, np.float32: 2e-4}
FTS = [np.float64, np.float32]
S = LC.S_POINTS


def _rel(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


def _systems(A, a, B, c, FT):
    """Per point: (M, d) formed in FT, and the float64 solve of the float64 system, from the same (cast) inputs."""
    M64, MFT = LC.system(A, B), LC.system(A, B, FT)
    d64 = a + np.einsum("sij,sj->si", A, c)
    dFT = a.astype(FT) + np.einsum("sij,sj->si", A.astype(FT), c.astype(FT))
    assert MFT.dtype == FT and dFT.dtype == FT
    x64 = np.linalg.solve(M64, d64[..., None])[..., 0]
    return MFT, dFT, x64


@pytest.mark.parametrize("shared", [False, True], ids=["per_point", "shared"])
@pytest.mark.parametrize("FT", FTS, ids=["f64", "f32"])
@pytest.mark.parametrize("N", LC.SIZES)
def test_pivoting_inputs(N, FT, shared):
    A, a, B, c = LC.fixed("pivoting", FT)(N, S, None, shared)
    assert B.shape[0] == (1 if shared else S)
    for x in (A, a, B, c):
        assert np.array_equal(x, x.astype(FT).astype(np.float64))        # exact in FT: the cast is no error source
    kappa = LC.kappa1(A, B)
    assert kappa <= 10, kappa
    tol = LC.tolerance(FLOOR[FT], kappa, FT)
    MFT, dFT, x64 = _systems(A, a, B, c, FT)
    worst_lapack, least_miss, swaps = 0.0, np.inf, []
    Bf = np.broadcast_to(B, A.shape)
    for s in range(S):
        # element (0, 0) of the device's M is exactly 0 in FT, whatever the order of the additions (exact partial sums)
        terms = A[s, 0].astype(FT) * Bf[s, :, 0].astype(FT)
        for order in (np.arange(N), np.arange(N)[::-1], np.random.default_rng(s).permutation(N)):
            acc = FT(0)
            for t in terms[order]:
                acc = FT(acc + t)
            assert FT(1) - acc == 0
        assert MFT[s][0, 0] == 0
        rows = LC.kernel_pivot_trace(MFT[s])
        ex = [(k, p) for k, p in enumerate(rows) if p != k]
        swaps.append(len(ex))
        assert all(p >= k for k, p in enumerate(rows))
        assert len(ex) >= N / 2, (s, len(ex))
        if N > 64:
            assert any(k < 64 <= p for k, p in ex), s
        sc = np.max(np.abs(x64[s]))
        xl = np.linalg.solve(MFT[s], dFT[s])
        assert xl.dtype == FT
        worst_lapack = max(worst_lapack, float(np.max(np.abs(xl - x64[s])) / sc))
        xk = LC.eliminate_with_exchange(MFT[s], dFT[s])[:, 0]                   # (the transcription itself solves the system)
        assert np.max(np.abs(xk - x64[s])) / sc <= tol / 4
        xn = LC.eliminate_no_exchange(MFT[s], dFT[s])[:, 0]
        miss = float(np.max(np.abs(xn - x64[s])) / sc) if np.all(np.isfinite(xn)) else np.inf
        least_miss = min(least_miss, miss)
    print("pivoting N %3d %s %-9s: kappa_1 %.2f, exchanges %s of %d steps, LAPACK in FT %.2e (tol %.1e), no exchange off by %.2e"
          % (N, np.dtype(FT).name, "shared" if shared else "per point", kappa, swaps, N, worst_lapack, tol, least_miss))
    assert worst_lapack <= tol / 4
    assert least_miss > 1000 * tol


@pytest.mark.parametrize("FT", FTS, ids=["f64", "f32"])
@pytest.mark.parametrize("N", [17, 65, 128])
def test_an_exchange_that_skips_right_hand_sides_is_caught(N, FT):
    """The multi-source GPU cases feed sources of magnitude 1 and 1e3 in alternating columns, once in each order, and assert the
    SUM of the level vectors: an exchange that stops after the first right-hand side leaves the second column unexchanged, and
    with the large source there the sum is off by far more than 1000 tolerances (with the small one it may hide in FP32, which
    is why both orders run)."""
    A, a, B, c = LC.fixed("pivoting", FT)(N, S, None, False)
    tol = LC.tolerance(FLOOR[FT], LC.kappa1(A, B), FT)
    MFT, dFT, _ = _systems(A, a, B, c, FT)
    rng = np.random.default_rng(N)
    for s in range(S):
        d = np.stack([dFT[s], (1e3 * rng.random(N)).astype(FT)], axis=1)
        ref = np.linalg.solve(MFT[s].astype(np.float64), d.astype(np.float64)).sum(axis=1)
        good = LC.eliminate_with_exchange(MFT[s], d).sum(axis=1)
        bad = LC.eliminate_exchange_first_rhs_only(MFT[s], d).sum(axis=1)
        sc = np.max(np.abs(ref))
        assert np.max(np.abs(good - ref)) / sc <= tol
        assert not np.all(np.isfinite(bad)) or np.max(np.abs(bad - ref)) / sc > 1000 * tol


@pytest.mark.parametrize("FT", FTS, ids=["f64", "f32"])
@pytest.mark.parametrize("N", [17, 127])
def test_exact_ties_inputs(N, FT):
    A, a, B, c = LC.exact_ties(N, FT)
    for x in (A, a, B, c):
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    M32, M64 = LC.system(A, B, np.float32), LC.system(A, B)
    assert np.array_equal(M32.astype(np.float64), M64)                   # the device's M is exact in both precisions
    assert np.array_equal(M64 * 8, np.round(M64 * 8)) and np.max(np.abs(M64)) <= 2
    kappa = LC.kappa1(A, B)
    assert kappa <= 10, kappa
    tol = LC.tolerance(FLOOR[FT], kappa, FT)
    MFT, dFT, x64 = _systems(A, a, B, c, FT)
    for s in range(S):
        col = np.abs(M64[s][:, 0])
        top = np.nonzero(col == col.max())[0]
        assert len(top) == 2 and M64[s][top[0], 0] == -M64[s][top[1], 0]
        assert top[0] < 64 and (top[1] >= 64) == (N > 64)
        ties = []
        rows = LC.kernel_pivot_trace(MFT[s], ties)
        assert ties[0] == 2 and rows[0] == top[0]                         # first occurrence
        assert sum(p != k for k, p in enumerate(rows)) >= N / 2
        sc = np.max(np.abs(x64[s]))
        assert np.max(np.abs(np.linalg.solve(MFT[s], dFT[s]) - x64[s])) / sc <= tol / 4
        xn = LC.eliminate_no_exchange(MFT[s], dFT[s])[:, 0]
        assert not np.all(np.isfinite(xn)) or np.max(np.abs(xn - x64[s])) / sc > 1000 * tol


@pytest.mark.parametrize("N", [17, 128])
def test_singular_inputs(N):
    A, a, B, c = LC.singular(N, np.float64)
    M = LC.system(A, B, np.float32).astype(np.float64)
    assert np.array_equal(M, LC.system(A, B))
    for s in range(S):
        assert np.all(M[s][:, N // 3] == 0) and np.linalg.matrix_rank(M[s]) == N - 1
        L = M[s].copy()                                                  # the kernel's steps up to N // 3: the pivot there is exactly 0
        rows = LC.kernel_pivot_trace(L)
        assert rows[N // 3] == N // 3


def test_contractive_never_exchanges():
    """What the sibling kernel tests feed: no step exchanges a row (why this file and its GPU twin exist)."""
    for N in (8, 60, 128):
        A, a, B, c = LC.contractive(N, S, np.random.default_rng(N), False)
        for M in LC.system(A, B):
            assert LC.kernel_pivot_trace(M) == list(range(N))


def test_cycle_is_one_long_cycle():
    for N in LC.SIZES:
        perm, i, n = LC.cycle(N), 0, 0
        while True:
            i, n = int(perm[i]), n + 1
            if i == 0:
                break
        assert n == N and not np.any(perm == np.arange(N)), N
