"""The series-order rule of the FP64 native layer kernels (vsm_native_dev.h nnorm / ninv_order), restated in numpy, and the inputs
on which it departs from the Frobenius rule of tests/inverse_order_cases.py (no GPU, no library).

The kernels bound E twice: F >= ||E||_F as before and n1 >= ||E||_1 = max_j sum_i |E_ij|, the induced 1-norm.  The pivoted inverse is
taken where F is not below 0.3, exactly as before; below that the order is what the unchanged rule `order` gives for min(F, n1).
Any induced norm bounds the tail, || sum_{k > K} E^k ||_1 <= ||E||_1^(K+1) / (1 - ||E||_1), and a 1-norm of eps / 4 bounds every
element by eps / 4 -- the guarantee of the Frobenius rule, element by element.

`order_sq` is the further rule that is NOT in the kernels ("Series order from the induced norm"): with
b2 = max_j sum_k c_k |E_kj| >= ||E^2||_1 (c_k = sum_i |E_ik|) the tail of order K is bounded by b2^((K+1) // 2) n1^((K+1) % 2) / (1 - n1).
It is restated here so that its rigour and its count on the benchmark's atmosphere stay on record beside the rule that ships."""
import numpy as np

import inverse_order_cases as X

LD, F32, F64 = X.LD, X.F32, X.F64
FAM = "native64"
# products an inverse of order K costs beyond the E it starts from (vsm_native_dev.h): Horner K - 1 up to order 8; 15, 16, 31 level by
# level (ninvert_slow_body); order 7 of an interaction in four (ninvert7); the pivoted inverse forms no product
PRODUCTS = {X.PIVOT: 0, 1: 0, 2: 1, 3: 2, 4: 3, 7: 6, 8: 7, 15: 6, 16: 7, 31: 8}
PRODUCTS_IA = {**PRODUCTS, 7: 4}


def _float_up(x):
    """__double2float_ru"""
    x = np.asarray(x, dtype=F64)
    f = x.astype(F32)
    return np.where(f.astype(F64) < x, np.nextafter(f, F32(np.inf)), f).astype(F32)


def bound_fro(E):
    return X.bound(E, FAM)


def bound_one(E):
    """The kernels' bound on ||E||_1 of a batch E[S,N,N]: column sums of |E| in double, handed on as floats (rounded up), their
    maximum, times 1.001f.  (The kernels convert the four partial sums of a column to the nearest float and add them in float: a few
    1e-7 of the bound either way, inside the factor -- the points of the tests keep 5 % from every band edge.)"""
    c = np.sum(np.abs(np.asarray(E, dtype=F64)), axis=-2)
    return (np.max(_float_up(c), axis=-1) * F32(1.001)).astype(F32)


def bound_sq(E):
    """b2 >= ||E^2||_1, formed like bound_one."""
    A = np.abs(np.asarray(E, dtype=F64))
    c = np.sum(A, axis=-2)
    return (np.max(_float_up(np.einsum("sk,skj->sj", c, A)), axis=-1) * F32(1.001)).astype(F32)


def order_fro(E):
    return [X.order(f, FAM) for f in bound_fro(E)]


def order_one(E):
    """What the kernels select."""
    return [X.order(min(f, a), FAM) if f < F32(0.3) else X.PIVOT for f, a in zip(bound_fro(E), bound_one(E))]


def order_sq(E):
    """The rule with b2 on top: evaluated where order_one is 2 or more, never above it."""
    out = []
    tol = F64(np.finfo(F64).eps) * 0.25
    for K1, a, b in zip(order_one(E), bound_one(E).astype(F64), bound_sq(E).astype(F64)):
        K = K1
        if K1 >= 2 and a < 0.3:
            lim = tol * (1.0 - a)
            K = next((k for k in X.SERIES if b ** ((k + 1) // 2) * a ** ((k + 1) % 2) <= lim), K1)
        out.append(min(K, K1))
    return out


def tail_max(E, K):
    """max_ij | sum_{k > K} E^k | = | E^(K+1) (I - E)^-1 | of one matrix, in long double."""
    E = np.asarray(E, dtype=LD)
    P = E.copy()
    for _ in range(K):
        P = P @ E
    return float(np.max(np.abs(P @ X.inv_newton(E))))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def scale_to(E, want):
    """E[s] rescaled so that the Frobenius bound of the kernels lands on want[s]."""
    E = np.asarray(E, dtype=F64).copy()
    for _ in range(4):
        E *= (np.asarray(want, dtype=F64) / bound_fro(E).astype(F64))[:, None, None]
    return E


def grazing(rng, S, N, background=1e-3):
    """Nonnegative matrices with ONE dominant row (the grazing stream of a thin layer: E = r r and E = R+- r-+ are all but rank one)
    over a dense background: ||E||_1 is about max_j |E_kj|, ||E||_F about the 2-norm of the whole row."""
    E = background * rng.random((S, N, N)) / N
    k = rng.integers(0, N, S)
    E[np.arange(S), k] += rng.uniform(0.5, 1.0, (S, N))
    return E


def departing_targets():
    """Per series band K above the first: (K, the next lower order, F, n1) with F 5 % above the band's lower edge and n1 10 % below it
    -- the Frobenius rule takes K, the kernels' rule the order below."""
    b = X.bands(FAM)
    ser = [k for k in b if k != X.PIVOT]
    return [(K, ser[i], 1.05 * b[K][0], 0.9 * b[K][0]) for i, K in enumerate(ser[1:])]


def mix_to_ratio(make_E, graze, dense, want_f, want_one):
    """Per point the weight beta of the dense part in graze + beta dense (bisection on log beta) at which the kernels' two bounds on
    E = make_E(matrix) stand in the ratio want_one / want_f, then the scale that puts F on want_f.  make_E must be linear."""
    want_f, want_one = np.asarray(want_f, dtype=F64), np.asarray(want_one, dtype=F64)
    lo, hi = np.full(len(want_f), -12.0), np.full(len(want_f), 6.0)

    def ratio(lb):
        E = make_E(graze + np.exp(lb)[:, None, None] * dense)
        return bound_one(E).astype(F64) / bound_fro(E).astype(F64)
    assert np.all(ratio(lo) < want_one / want_f) and np.all(ratio(hi) > want_one / want_f), "the mixture does not span the ratio"
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        up = ratio(mid) < want_one / want_f
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    M = graze + np.exp(0.5 * (lo + hi))[:, None, None] * dense
    for _ in range(4):
        M = M * (want_f / bound_fro(make_E(M)).astype(F64))[:, None, None]
    return M
