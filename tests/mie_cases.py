"""Seeded synthetic inputs of the Mie entry points (vsm_mie_nai2, vsm_mie_nai2_lin) shared by the Mie edge tests (CPU and GPU): the
arrays both oracles take (mie_oracle.nai2_reference, mie_lin_oracle.nai2_lin_reference) and a Scattering.MieHostInputs holds.

Through the public functions every radius carries its natural cut-off n_max_i = get_n_max(x_i), the order at which its series has
converged: the terms next to it are 1e-8 and smaller, and a kernel that drops or doubles one of them is wrong by less than any bound
worth asserting.  Here the cut-offs are prescribed BELOW the size parameter -- x_i = (n_max_i + 1) u_i, u_i in [1, 1.3] --, where
the last kept term is O(1): a defect of one order, one radius or one angle moves the outputs by 1e-6 to 0.6
(tests/test_oracle_mie.py measures it per case) and the upward psi / chi recurrences are stable, so rounding stays near 1e-15.

A case is (nquad, n_max, m, seed) with k_wave = 1 (r = x).  The cut-offs are drawn from 1 .. n_max (1 .. cap where a cap is given),
unsorted, with at least one at n_max (at cap), one at 1 and, from n_max >= 6 on, a multiple of 4 with both neighbours (the k-step of
stage 2).  wx is positive, within a factor 3 of uniform, and sums to 1; wr = 4 pi x^2 wx; mu, w_mu = leggauss(2 n_max - 1); wx_dot
[2, nquad] has both signs and rows that sum to 0, as Scattering.weight_derivatives produces; wr_dot = 4 pi x^2 wx_dot."""
import collections
import functools
import math
import os
import types

import numpy as np

Case = collections.namedtuple("Case", "name nquad n_max m seed cap")

M_DEFAULT = (1.4, 0.01)                  # n_r, n_i of m = n_r - i n_i

# nquad at 1, 15 / 16 / 17 (a radius tile), 31 / 32 / 33 (a group), 63 / 64 / 65 (the padding to 64: a wholly dead group, a group with
# one live radius), 129; n_max at 2 .. 9 (the padding of the orders to 4, the k-step); n_mu = 2 n_max - 1 = 15, 17, 63, 65, 127, 129,
# 193 (the 16-angle tiles, the 64-angle chunks, the 16-moment transpositions)
SHAPES = [(1, 2), (15, 3), (16, 4), (17, 5), (31, 8), (32, 9), (33, 32), (63, 33), (64, 64), (65, 65), (129, 97)]


def _case(nquad, n_max, m=M_DEFAULT, seed=None, cap=None, tag=""):
    return Case("q%d_n%d%s" % (nquad, n_max, tag), nquad, n_max, m, 7 * nquad + n_max if seed is None else seed, cap)


CASES = [_case(q, n) for q, n in SHAPES] + [
    _case(33, 32, cap=20, tag="_cap20"),                 # rows 21 .. 32 of every radius and the moments above 40 are zeros
    _case(33, 32, m=(1.33, 0.0), tag="_real"),           # n_i = 0: the single-scattering albedo is 1
    _case(33, 32, m=(2.0, 1.0), tag="_absorbing"),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def _is_sorted(v):
    return len(v) > 2 and (np.all(np.diff(v) >= 0) or np.all(np.diff(v) <= 0))


def cutoffs(rng, nquad, top):
    """nquad cut-offs from 1 .. top, unsorted, holding top, 1 and (top >= 6) a multiple of 4 with its two neighbours."""
    if nquad == 1:
        return np.array([top], dtype=np.int32)
    v = rng.integers(1, top + 1, nquad)
    need = [top, 1]
    if top >= 6:
        j = int(rng.integers(1, (top - 1) // 4 + 1))     # 4 j + 1 <= top
        need += [4 * j - 1, 4 * j, 4 * j + 1]
    assert nquad >= len(need), (nquad, need)
    v[rng.choice(nquad, len(need), replace=False)] = need
    while _is_sorted(v):
        v = rng.permutation(v)
    return v.astype(np.int32)


def inputs(case):
    """The arrays of one case: x, wx, wr, wx_dot, wr_dot, nmax_i, mu, w_mu, n_r, n_i, k_wave, n_max, n_mu (all float64 / int32)."""
    rng = np.random.default_rng(case.seed)
    nmax_i = cutoffs(rng, case.nquad, case.n_max if case.cap is None else case.cap)
    x = (nmax_i + 1) * rng.uniform(1.0, 1.3, case.nquad)
    wx = rng.uniform(0.6, 1.6, case.nquad)
    wx = wx / np.sum(wx)
    raw_dot = rng.uniform(-1.0, 1.0, (2, case.nquad)) * wx
    wx_dot = np.stack([raw_dot[k] - np.sum(raw_dot[k]) * wx for k in range(2)])
    n_mu = 2 * case.n_max - 1
    mu, w_mu = np.polynomial.legendre.leggauss(n_mu)
    return types.SimpleNamespace(x=x, wx=wx, wr=4 * math.pi * x ** 2 * wx, wx_dot=wx_dot, wr_dot=4 * math.pi * x ** 2 * wx_dot,
                                 nmax_i=nmax_i, mu=mu, w_mu=w_mu, n_r=case.m[0], n_i=case.m[1], k_wave=1.0, n_max=case.n_max,
                                 n_mu=n_mu)


def with_dead_radii(h, total, seed):
    """h with radii of weight zero (wx = wr = wx_dot = wr_dot = 0) appended up to `total`: cut-offs anywhere in 1 .. n_max and size
    parameters by the recipe above, so that their a_n, b_n, S1, S2 are ordinary numbers which only the weights remove."""
    rng = np.random.default_rng(seed)
    extra = total - len(h.x)
    assert extra > 0
    nm = rng.integers(1, h.n_max + 1, extra).astype(np.int32)
    x = (nm + 1) * rng.uniform(1.0, 1.3, extra)
    z, z2 = np.zeros(extra), np.zeros((2, extra))
    d = dict(vars(h))
    d.update(x=np.concatenate([h.x, x]), nmax_i=np.concatenate([h.nmax_i, nm]), wx=np.concatenate([h.wx, z]),
             wr=np.concatenate([h.wr, z]), wx_dot=np.concatenate([h.wx_dot, z2], axis=1),
             wr_dot=np.concatenate([h.wr_dot, z2], axis=1))
    return types.SimpleNamespace(**d)


def forward_args(h):
    """The positional arguments of mie_oracle.nai2_reference."""
    return h.x, h.wx, h.wr, h.nmax_i, h.mu, h.w_mu, h.n_r, h.n_i, h.k_wave, h.n_max


def lin_args(h):
    """The positional arguments of mie_lin_oracle.nai2_lin_reference."""
    return h.x, h.wx, h.wr, h.wx_dot, h.wr_dot, h.nmax_i, h.mu, h.w_mu, h.n_r, h.n_i, h.k_wave, h.n_max


# ---- the comparison measure and the rounding floor, shared by tests/test_oracle_mie*.py (CPU) and tests/test_gpu_mie_edges.py ------
FORWARD = ("greek", "bulk_f", "scal")
FAMILIES = FORWARD + ("greek_dot", "bulk_f_dot", "scal_dot")
MIN_FLOOR = 1e-14
FLOOR_LIMIT = 1e-10                      # a case whose floor is above this is ill-conditioned and has no place here
REALISATIONS = 8


def oracle(h, dtype=np.float64, x=None):
    """Every output of mie_lin_oracle.nai2_lin_reference on the arrays of h (its forward outputs are mie_oracle.nai2_reference's,
    bit for bit), as a dict with the term sums under "scales"; x replaces h.x."""
    import mie_lin_oracle as ML
    args = list(lin_args(h))
    if x is not None:
        args[0] = x
    g, sc, bulk, gd, sd, bd, _ab, S = ML.nai2_lin_reference(*args, dtype=dtype, scales=True)
    return dict(greek=g, scal=np.array(sc), bulk_f=bulk, greek_dot=gd, scal_dot=sd, bulk_f_dot=bd, scales=S)


def vector_deviation(got, ref):
    """One coefficient vector on max(1, max |ref|)."""
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref)))))


def _on_scale(got, ref, scale):
    """max |got - ref| / scale; where the scale is an exact zero (no term at all) only an exact zero is no deviation."""
    dev = np.abs(np.asarray(got) - ref)
    live = scale > 0
    worst = float(np.max(dev[live] / scale[live])) if np.any(live) else 0.0
    return worst if not np.any(dev[~live]) else math.inf


def measure(out, ref, families=FAMILIES, base=None):
    """The deviation of `out` from the long-double oracle `ref` (from `base`, another set of outputs, where one is given: the scales
    stay those of `ref`) per output family, each on the scale its rounding lives on:
    a coefficient vector (and a derivative vector per slot) on max(1, max |ref|); a bulk_f row per angle on that angle's
    sum_i |wr_i 0.5 / x_i^2| (|S1|^2 + |S2|^2) (bulk_f_dot on the like sums of its own terms); C_sca, C_ext and their derivatives
    on sum |wx| |term| over radii and orders, the albedo on C_sca's over C_ext and its derivative on
    (sum |C_sca' terms| + ssa sum |C_ext' terms|) / C_ext."""
    S = ref["scales"]
    c_sca, c_ext, ssa = ref["scal"]
    res = {}
    for fam in families:
        got, want = out[fam], (ref if base is None else base)[fam]
        assert got.shape == ref[fam].shape == want.shape, (fam, got.shape, ref[fam].shape, want.shape)
        vec = lambda g, w, r: float(np.max(np.abs(g - w)) / max(1.0, float(np.max(np.abs(r)))))
        if fam == "greek":
            res[fam] = max(vec(got[c], want[c], ref[fam][c]) for c in range(6))
        elif fam == "greek_dot":
            res[fam] = max(vec(got[s, c], want[s, c], ref[fam][s, c]) for s in range(4) for c in range(6))
        elif fam == "bulk_f":
            res[fam] = _on_scale(got, want, np.broadcast_to(S.bulk_abs, got.shape))
        elif fam == "bulk_f_dot":
            res[fam] = _on_scale(got, want, np.broadcast_to(S.bulk_dot_abs[:, None, :], got.shape))
        elif fam == "scal":
            res[fam] = _on_scale(got, want, np.array([S.c_abs[0], S.c_abs[1], S.c_abs[0] / abs(c_ext)]))
        else:
            a = S.c_dot_abs
            res[fam] = _on_scale(got, want, np.stack([a[:, 0], a[:, 1], (a[:, 0] + ssa * a[:, 1]) / abs(c_ext)], axis=1))
    return res


def floors(h, seed=0):
    """(long-double oracle, floor per family): the floor is the largest deviation from the long-double oracle, on the scales of
    `measure`, of the float64 oracle itself and of REALISATIONS seeded float64 runs with every x_i times 1 +- 2^-52, and at least
    MIN_FLOOR.  What a correct float64 evaluation in another order of operations may deviate by is a small multiple of it."""
    ref = oracle(h, np.longdouble)
    worst = measure(oracle(h), ref)
    rng = np.random.default_rng(1000003 + seed)
    for _ in range(REALISATIONS):
        xp = h.x * (1.0 + rng.choice([-1.0, 1.0], len(h.x)) * 2.0 ** -52)
        d = measure(oracle(h, x=xp), ref)
        worst = {f: max(worst[f], d[f]) for f in FAMILIES}
    return ref, {f: max(worst[f], MIN_FLOOR) for f in FAMILIES}


@functools.lru_cache(maxsize=None)
def case_floors(name):
    """floors of a named case: computed once per run, shared, never changed."""
    case = BY_NAME[name]
    return floors(inputs(case), case.seed)


# ---- what the CPU tests of both oracles share ----------------------------------------------------------------------------------------
GOLDEN_F64 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mie_oracle_float64.npz")   # the float64 oracles'
GOLDEN_CASES = ("q17_n5", "q33_n32")                                              # outputs, recorded before they took a dtype
SENSITIVITY = 1e-6


def _moves(h, n_max):
    """Every radius' cut-off one up and one down, wherever it stays in 1 .. n_max."""
    for i in range(len(h.x)):
        for step in (-1, 1):
            if 1 <= h.nmax_i[i] + step <= n_max:
                nm = h.nmax_i.copy()
                nm[i] += step
                yield "n_max_i[%d] %+d" % (i, step), dict(nmax_i=nm)


def perturbations(h, n_max):
    """The defects a kernel edge can produce, as changes of the oracle's inputs: one cut-off off by one, the last radius without
    weight, the last angle without weight."""
    yield from _moves(h, n_max)
    if len(h.x) > 1:                                         # (a distribution of one radius has nothing left without it)
        z = lambda a: np.concatenate([a[..., :-1], np.zeros_like(a[..., -1:])], axis=-1)
        yield "last radius", dict(wx=z(h.wx), wr=z(h.wr), wx_dot=z(h.wx_dot), wr_dot=z(h.wr_dot))
    yield "last angle", dict(w_mu=np.concatenate([h.w_mu[:-1], [0.0]]))


def greek_move(got, base):
    return max(vector_deviation(got[c], base[c]) for c in range(6))
