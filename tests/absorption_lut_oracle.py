"""numpy restatement of the InterpolationModel's interpolant, the reference the LUT tests compare against.

Arrays are in the reference's axis order: values [nν, nP, nT], cubic coefficients [nν + 2, nP + 2, nT + 2].  An axis is
(first, step, n) with the float64 nodes x_k = first + k step; x lies in cell i = [x_i, x_i+1) (clamped to 0 .. n - 2) at
t = (x - x_i) / (x_i+1 - x_i) -- in float64 whatever `dtype` is: that quotient is part of the definition, the device forms it the
same way.  It is (x - first) / step - i up to the rounding of the nodes themselves, and exactly 0 on a node.

    system_matrix, prefilter_axis, prefilter     the (n + 2) system per axis; float64 by numpy's dense solve, long double by
                                                 Gaussian elimination written out here (numpy has no long double solve)
    weights                                      the tap weights and their derivatives with respect to t
    evaluate                                     sigma [Nz, nSpec], d sigma / dT, d sigma / dp and the sums of |w C| and |w' C| that
                                                 the rounding bounds of the GPU tests are made of
Everything is computed in `dtype` (np.float64 or np.longdouble)."""
import numpy as np


def system_matrix(n, dtype=np.float64):
    """Rows 0 and n + 1: c[0] - 2 c[1] + c[2] = 0 and its mirror; rows 1 .. n: c[i-1]/6 + 2 c[i]/3 + c[i+1]/6 = y[i]."""
    one = dtype(1)
    M = np.zeros((n + 2, n + 2), dtype=dtype)
    M[0, :3] = [1, -2, 1]
    M[n + 1, n - 1:] = [1, -2, 1]
    for i in range(1, n + 1):
        M[i, i - 1:i + 2] = [one / 6, 2 * one / 3, one / 6]
    return M


def _solve(M, Y):
    """M X = Y.  float64: numpy's dense LU.  Otherwise elimination with partial pivoting among the rows the band can fill."""
    if M.dtype == np.float64:
        return np.linalg.solve(M, Y)
    M, Y = M.copy(), Y.copy()
    N = len(M)
    for i in range(N):
        rows = list(range(i, min(i + 3, N)))
        piv = rows[int(np.argmax(np.abs(M[rows, i])))]
        if piv != i:
            M[[i, piv]], Y[[i, piv]] = M[[piv, i]], Y[[piv, i]]
        for r in rows[1:]:
            f = M[r, i] / M[i, i]
            if f != 0:
                M[r] -= f * M[i]
                Y[r] -= f * Y[i]
    X = np.zeros_like(Y)
    for i in range(N - 1, -1, -1):
        X[i] = (Y[i] - M[i, i + 1:] @ X[i + 1:]) / M[i, i]
    return X


def prefilter_axis(y, axis, dtype=np.float64):
    """The coefficients along `axis` (n -> n + 2 entries)."""
    y = np.moveaxis(np.asarray(y, dtype=dtype), axis, 0)
    n = y.shape[0]
    rhs = np.zeros((n + 2, int(np.prod(y.shape[1:], dtype=np.int64))), dtype=dtype)
    rhs[1:n + 1] = y.reshape(n, -1)
    c = _solve(system_matrix(n, dtype), rhs)
    return np.moveaxis(c.reshape((n + 2,) + y.shape[1:]), 0, axis)


def prefilter(values, dtype=np.float64):
    """values [nν, nP, nT] -> coefficients [nν + 2, nP + 2, nT + 2]: the three axes one after the other."""
    c = np.asarray(values, dtype=dtype)
    for axis in range(3):
        c = prefilter_axis(c, axis, dtype)
    return c


def locate(x, axis, dtype=np.float64):
    """(i, t, h) of x on axis = (first, step, n): the nodes are the float64 numbers x_k = first + k step, cell i is [x_i, x_i+1)
    along the axis (the last one closed; an x outside falls into the end cell), h = x_i+1 - x_i and t = (x - x_i) / h, both formed
    in float64 as the device forms them."""
    first, step, n = np.float64(axis[0]), np.float64(axis[1]), axis[2]
    x = np.asarray(x, dtype=np.float64)
    nodes = first + np.arange(n) * step
    if step > 0:
        i = np.searchsorted(nodes, x, side="right") - 1
    else:
        i = np.searchsorted(-nodes, -x, side="right") - 1
    i = np.clip(i, 0, n - 2)
    h = nodes[i + 1] - nodes[i]
    return i.astype(np.int64), ((x - nodes[i]) / h).astype(dtype), h


def weights(t, cubic, dtype=np.float64):
    """(w, dw / dt) [..., 4 or 2]."""
    t = np.asarray(t, dtype=dtype)
    if not cubic:
        return np.stack([1 - t, t], -1), np.stack([-np.ones_like(t), np.ones_like(t)], -1)
    t2, t3, s = t * t, t * t * t, 1 - t
    w = np.stack([s ** 3, 3 * t3 - 6 * t2 + 4, -3 * t3 + 3 * t2 + 3 * t + 1, t3], -1) / 6
    d = np.stack([-3 * s * s, 9 * t2 - 12 * t, -9 * t2 + 6 * t + 3, 3 * t2], -1) / 6
    return w, d


def axis_ends(axis):
    first, step, n = axis
    last = np.float64(first) + np.float64(n - 1) * np.float64(step)
    return min(first, last), max(first, last)


def evaluate(coef, nu_axis, p_axis, t_axis, grid, p, T, cubic=True, dtype=np.float64):
    """The interpolant at (grid[s], p[z], T[z]) from coefficients in the reference's axis order.  Returns a dict of [Nz, nSpec]
    arrays: sigma, dT, dp, and mag / mag_dT / mag_dp = sum |w_abc C_abc| with the weights of each; points with ν outside the axis
    are exact zeros in all of them."""
    C = np.asarray(coef).astype(dtype)
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    p, T = np.atleast_1d(np.asarray(p, dtype=np.float64)), np.atleast_1d(np.asarray(T, dtype=np.float64))
    NT = 4 if cubic else 2
    lo, hi = axis_ends(nu_axis)
    inside = (grid >= lo) & (grid <= hi)
    inu, tnu, _ = locate(grid, nu_axis, dtype)
    wn, _ = weights(tnu, cubic, dtype)
    taps = np.arange(NT)
    out = {k: np.zeros((len(p), len(grid)), dtype=dtype) for k in ("sigma", "dT", "dp", "mag", "mag_dT", "mag_dp")}
    for z in range(len(p)):
        ip, tp, hp = locate(p[z], p_axis, dtype)
        it, tt, ht = locate(T[z], t_axis, dtype)
        wp, dwp = weights(tp, cubic, dtype)
        wt, dwt = weights(tt, cubic, dtype)
        dwp, dwt = dwp / dtype(hp), dwt / dtype(ht)
        sub = C[(inu[:, None] + taps)[:, :, None, None], (ip + taps)[None, None, :, None], (it + taps)[None, None, None, :]]
        for key, a, b in (("sigma", wp, wt), ("dT", wp, dwt), ("dp", dwp, wt)):
            w3 = wn[:, :, None, None] * a[None, None, :, None] * b[None, None, None, :]
            out[key][z] = np.where(inside, np.sum(w3 * sub, axis=(1, 2, 3)), 0)
            mk = "mag" if key == "sigma" else "mag_" + key
            out[mk][z] = np.where(inside, np.sum(np.abs(w3 * sub), axis=(1, 2, 3)), 0)
    return out
