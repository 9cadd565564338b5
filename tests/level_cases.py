"""Inputs of the level kernels (vsm_level_radiance_* and kin, csrc/vsm_level.hip) for tests/test_oracle_level_pivoting.py (CPU) and
tests/test_gpu_level_pivoting.py (GPU), and a numpy transcription of the kernels' elimination.

Every fused level kernel solves [M | r_1 .. r_k], M = I - A B, by Gauss-Jordan elimination with partial pivoting (level_eliminate:
largest |m_ik| over the rows i >= k, first occurrence).  `contractive` is the family the kernel tests have always used: A, B
positive with row sums 0.3, so M is strongly diagonally dominant and no step ever exchanges a row.  The other families are built
so that the exchange matters:

    pivoting     M = Pi (D + E), well conditioned, large entries OFF the diagonal, the natural diagonal exactly 0
    exact_ties   M exact in both precisions, column 0 carries its largest magnitude twice (opposite signs)
    singular     M exact with one all-zero column: an exactly zero pivot

All return (A, a, B, c) in math order: A [S, N, N], B [S | 1, N, N], a / c [S, N], float64 arrays whose values are exact in FT (the
arrays are cast to FT and back), so a float64 reference computed from them sees the inputs the device sees."""
import numpy as np

# every N a GPU test of tests/test_gpu_level_pivoting.py uses (tests/test_oracle_level_pivoting.py checks the inputs at all of them)
SIZES = (2, 3, 16, 17, 21, 61, 63, 65, 127, 128)
S_POINTS = 3


def contractive(N, S, rng, shared_bot):
    A = rng.random((S, N, N)) * (0.6 / N)
    B = rng.random((1 if shared_bot else S, N, N)) * (0.6 / N)
    a, c = rng.random((S, N)), rng.random((S, N))
    return A, a, B, c


def _cast(x, FT):
    return np.asarray(x, dtype=FT).astype(np.float64)


def cycle(N):
    """The row permutation of `pivoting`: perm = roll(arange(N), N // 2 + 1), so row i carries the large entry of column
    perm[i] = i - (N // 2 + 1) mod N and column 0 finds its pivot in row N // 2 + 1 (>= 64 for N >= 127).  One long cycle for every
    N of SIZES (gcd(N // 2 + 1, N) = 1); N = 2: a roll by 1 (N // 2 + 1 = N would be the identity)."""
    shift = N // 2 + 1
    return np.roll(np.arange(N), shift if shift % N else 1)


def pivoting(N, S, rng, shared_bot, FT):
    """M = Pi (D + E): D = diag(+-(1 .. 2)), E dense with |E_ij| <= 0.3 / N and zero diagonal, Pi = cycle(N), the natural diagonal
    of M set to exactly 0.  B = 0.5 I + (rng - 0.5) 0.6 / N (dense, well conditioned), cast to FT; A = (I - M) B^-1 in float64 from
    the cast B, then cast.  shared_bot: one B for every point, A per point.  ||D^-1 E||_1 <= 0.3, so kappa_1(M) <= 2 (1.3 / 0.7)
    < 4 before the casts.

    The casts alone would leave rounding noise of a few eps(FT) on the diagonal of the DEVICE's M = I - fl(A) fl(B), and an
    elimination that never exchanges rows would then be wrong by a random amount (0.02 .. 1 of the solution, whatever the
    precision).  So element (0, 0) is made exactly zero on the device as well, in both precisions and in any order of the
    additions: column 0 of B is rounded to multiples of 2^-12 with B_00 = 1/2, row 0 of A to multiples of 2^-10, and A_00 =
    2 (1 - sum_{k > 0} A_0k B_k0).  Every product of (A B)_00 is then a multiple of 2^-22 and every partial sum is below 4: 24 bits,
    exact in Float32.  Step 0 of an elimination without exchange divides by exactly 0.  (Row 0 of M moves by less than 2^-11.)"""
    nB = 1 if shared_bot else S
    B = 0.5 * np.eye(N)[None] + (rng.random((nB, N, N)) - 0.5) * (0.6 / N)
    B[:, :, 0] = np.round(B[:, :, 0] * 4096.0) / 4096.0
    B[:, 0, 0] = 0.5
    B = _cast(B, FT)
    perm = cycle(N)
    A = np.empty((S, N, N))
    for s in range(S):
        D = np.diag(rng.choice([-1.0, 1.0], N) * (1.0 + rng.random(N)))
        E = (2.0 * rng.random((N, N)) - 1.0) * (0.3 / N)
        np.fill_diagonal(E, 0.0)
        M = (D + E)[perm]
        np.fill_diagonal(M, 0.0)
        A[s] = (np.eye(N) - M) @ np.linalg.inv(B[s % nB])
        A[s, 0] = np.round(A[s, 0] * 1024.0) / 1024.0
        A[s, 0, 0] = 2.0 * (1.0 - A[s, 0, 1:] @ B[s % nB, 1:, 0])     # (dyadic terms: exact in float64)
    a, c = rng.random((S, N)), rng.random((S, N))
    return _cast(A, FT), _cast(a, FT), B, _cast(c, FT)


def _dyadic_cycle_matrix(N, rng):
    """Pi (D + E) in multiples of 1/8: D = diag(+-{1, 1.125, .. 2}), E = one +-1/8 per row next to the diagonal of D (N > 2)."""
    D = rng.choice([-1.0, 1.0], N) * (1.0 + rng.integers(0, 9, N) / 8.0)
    DE = np.diag(D)
    if N > 2:
        for i in range(N):
            DE[i, (i + 1) % N] = rng.choice([-0.125, 0.125])
    return DE, D


def exact_ties(N, FT, S=S_POINTS):
    """B = 0.5 (signed permutation), A = 2 (I - M) (signed permutation)^T: every element of A B is ONE exact product, so the
    device's M = I - A B is M itself in both precisions.  M = Pi (D + E) in multiples of 1/8, |m| <= 2, and column 0 carries its
    largest magnitude (1) twice with opposite signs: in row N // 2 + 1 (its cycle row; >= 64 for N >= 127) and in row 1.  Either
    choice is a valid pivot; the kernel's rule takes row 1.  a, c: multiples of 1/8 in [0, 1]."""
    rng = np.random.default_rng(1000 + N)
    perm = cycle(N)
    r0 = int(np.nonzero(perm == 0)[0][0])          # the row of column 0's large entry
    r1 = 1 if r0 != 1 else 0
    Bs = rng.choice([-1.0, 1.0], N)
    permB = rng.permutation(N)
    P = np.zeros((N, N))
    P[np.arange(N), permB] = Bs                    # signed permutation
    A = np.empty((S, N, N))
    for s in range(S):
        DE, D = _dyadic_cycle_matrix(N, rng)
        DE[0, 0] = np.sign(D[0])                   # column 0: magnitude 1 in its cycle row ...
        DE[perm[r1], perm[r1]] = 2.0 * np.sign(D[perm[r1]])   # (row r1's own pivot: 2, so the tie perturbs M by a factor <= 1/2)
        M = DE[perm]
        M[:, 0] = np.where(np.arange(N) == r0, M[:, 0], 0.0)
        M[r1, 0] = -M[r0, 0]                       # ... and the same magnitude, opposite sign, in row r1
        A[s] = 2.0 * (np.eye(N) - M) @ P.T
    B = np.broadcast_to(0.5 * P, (S, N, N)).copy()
    a, c = rng.integers(0, 9, (S, N)) / 8.0, rng.integers(0, 9, (S, N)) / 8.0
    return _cast(A, FT), a, B, c


def singular(N, FT, S=S_POINTS):
    """B = I, A = I - M with M = Pi D in multiples of 1/8 and column N // 3 all zero: M = I - A B exactly on the device, the column
    stays exactly zero under every row operation, and step N // 3 finds a pivot that is exactly 0."""
    rng = np.random.default_rng(2000 + N)
    perm = cycle(N)
    A = np.empty((S, N, N))
    for s in range(S):
        DE, _ = _dyadic_cycle_matrix(N, rng)
        M = DE[perm]
        M[:, N // 3] = 0.0
        A[s] = np.eye(N) - M
    B = np.broadcast_to(np.eye(N), (S, N, N)).copy()
    a, c = rng.integers(0, 9, (S, N)) / 8.0, rng.integers(0, 9, (S, N)) / 8.0
    return _cast(A, FT), a, B, c


def system(A, B, FT=np.float64):
    """M = I - A B [S, N, N], formed in precision FT."""
    A, B = np.asarray(A, dtype=FT), np.asarray(B, dtype=FT)
    return np.eye(A.shape[-1], dtype=FT)[None] - A @ np.broadcast_to(B, A.shape)


def kappa1(A, B):
    """max over the points of the 1-norm condition number of I - A B."""
    return max(float(np.linalg.cond(M, 1)) for M in system(A, B))


def tolerance(floor, kappa, FT):
    """The bound of test_gpu_parity::test_strip128_pivoted_inverse_near_and_beyond_unit_spectral_radius."""
    return max(floor, 50.0 * kappa * float(np.finfo(FT).eps))


def _eliminate(M, d, exchange, ties=None, exchange_cols=None):
    """level_eliminate in numpy, in the precision of M: unnormalised Gauss-Jordan on [M | d], at step k the pivot row p = the first
    row i >= k with the largest |m_ik| (exchange) or p = k.  exchange_cols: the exchange stops before that column (a WRONG kernel
    that leaves right-hand sides behind).  Returns (rows chosen, d_i / m_ii)."""
    M = np.array(M)
    N = M.shape[0]
    L = np.concatenate([M, np.asarray(d, dtype=M.dtype).reshape(N, -1)], axis=1)
    rows = []
    with np.errstate(all="ignore"):
        for k in range(N):
            col = np.abs(L[k:, k])
            p = k + int(np.argmax(col)) if exchange and not np.isnan(col).all() else k      # (argmax: first occurrence)
            if ties is not None:
                ties.append(int(np.sum(col == col[p - k])))
            rows.append(p)
            if p != k:
                L[[k, p], k:exchange_cols] = L[[p, k], k:exchange_cols]
            f = L[:, k] / L[k, k]
            f[k] = 0
            L[:, k + 1:] -= f[:, None] * L[k, k + 1:][None, :]
        x = L[:, N:] / np.diag(L)[:, None]
    return rows, x


def kernel_pivot_trace(M, ties=None):
    """The pivot rows level_eliminate chooses for M, step by step.  ties: a list that receives, per step, the number of candidate
    rows whose magnitude equals the largest one."""
    return _eliminate(M, np.zeros(np.shape(M)[0], dtype=np.asarray(M).dtype), True, ties)[0]


def eliminate_no_exchange(M, d):
    """The same elimination with p = k forced (a kernel that never pivots): the solution it would return, [N, columns of d]."""
    return _eliminate(M, d, False)[1]


def eliminate_with_exchange(M, d):
    """The kernel's own elimination, in numpy."""
    return _eliminate(M, d, True)[1]


def fixed(family, FT):
    """An `inputs=` generator for the call helpers of the kernel tests (signature of `contractive`) that is a function of
    (N, S, shared_bot, FT) alone -- the caller's rng is not used -- so that tests/test_oracle_level_pivoting.py checks on the CPU
    the very arrays the GPU tests feed.  family: "pivoting", "exact_ties", "singular" (both with the same B at every point: a shared
    bottom is its first block) or "nonfinite" (`pivoting` with one NaN in A of point 1)."""
    def gen(N, S, rng, shared_bot):
        if family in ("pivoting", "nonfinite"):
            A, a, B, c = pivoting(N, S, np.random.default_rng([N, S, int(shared_bot)]), shared_bot, FT)
            if family == "nonfinite":
                A[1, 3 % N, 5 % N] = np.nan
            return A, a, B, c
        A, a, B, c = {"exact_ties": exact_ties, "singular": singular}[family](N, FT, S)
        return A, a, (B[:1] if shared_bot else B), c
    return gen


def eliminate_exchange_first_rhs_only(M, d):
    """A kernel whose row exchange covers M and the FIRST right-hand side only (columns k .. N): the solutions it would return."""
    return _eliminate(M, d, True, exchange_cols=np.shape(M)[0] + 1)[1]
