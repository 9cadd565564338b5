"""CPU checks of tests/inverse_order_cases.py, for every family, precision, size and target that tests/test_gpu_inverse_orders.py
runs on the GPU: the restated selection rule assigns the intended order (2 % from both band edges), the per-case tolerance comes
from the own-precision restatement, a series cut at K // 2 misses that tolerance at least threefold at the point that pins each
order, the long-double reference says the same operation as the oracle, and every reachable (family, precision, order) triple is
pinned by at least one case."""
from functools import lru_cache

import numpy as np
import pytest

import inverse_order_cases as X
from oracle import vsm_oracle as O


def test_long_double_is_wider_than_double():
    assert X.have_long_double(), np.finfo(np.longdouble).eps


@pytest.mark.parametrize("fam", ["native64", "strip64", "strip128", "strip128_f32"])
def test_bands_of_the_fp64_rule(fam):
    """nseries_order / series_order128: all ten branches are reachable, k_ia128<float> included (it selects by the FP64 tolerance)."""
    b = X.bands(fam)
    assert list(b) == [1, 2, 3, 4, 7, 8, 15, 16, 31, X.PIVOT]
    assert b[31][1] < 0.3 <= b[X.PIVOT][0] and np.float32(b[X.PIVOT][0]) == np.float32(0.3)
    for K in X.SERIES:          # the rule as a formula: nrm^(K+1) <= eps / 4 (1 - nrm), and not so one order lower
        hi = b[K][1]
        assert hi ** (K + 1) <= 2.0 ** -54 * (1 - hi) * (1 + 1e-6) and (hi * (1 + 1e-6)) ** (K + 1) > 2.0 ** -54 * (1 - hi) * (1 - 1e-6) or K == 31


@pytest.mark.parametrize("fam", ["fused32", "strip32", "native32"])
def test_bands_of_the_fp32_rule(fam):
    """n32series_order / series_order (vsm_strip32.hip) / invert_one_minus<float>: order 15 covers everything below 0.3, so orders
    16 and 31 are unreachable; the upper edges are those of the formula in Float32."""
    b = X.bands(fam)
    assert list(b) == [1, 2, 3, 4, 7, 8, 15, X.PIVOT]
    for K, want in ((1, 1.73e-4), (2, 3.1e-3), (3, 1.31e-2), (4, 3.11e-2), (7, 0.113), (8, 0.143)):
        assert abs(b[K][1] / want - 1) < 1e-2, (K, b[K])
    assert b[15][1] < 0.3 <= b[X.PIVOT][0]
    assert 0.3 ** 16 <= 2.0 ** -25 * 0.7                # why 16 and 31 are unreachable: the order-15 test passes up to 0.3


def test_the_strip32_bound_is_not_the_other_families():
    """vsm_strip32.hip scales the sum of squares by 1.0001f before the square root: its bound on the same E is 5e-5 larger."""
    E = (np.random.default_rng(0).random((3, 70, 70)) / 70).astype(np.float32)
    a, b = X.bound(E, "strip32").astype(float), X.bound(E, "native32").astype(float)
    assert np.all(np.abs(a / b - (1 + 5e-5)) < 1e-6)
    nf = np.sqrt(np.sum(E.astype(float) ** 2, axis=(1, 2)))
    assert np.all(b >= nf) and np.all(b / nf < 1.0011)


def _check(fam_name, tg, c, names, what):
    fam = X.FAMILIES[fam_name]
    b = X.bands(fam_name)
    bounds, ks = c["sel"][0]
    # 1. branch
    for s, t in enumerate(tg):
        assert abs(bounds[s] / t.bound - 1) < 1e-5, (what, t, bounds[s])
        assert abs(c["bounds"][s] / t.bound - 1) < 1e-5
        assert ks[s] in t.orders, (what, t, ks[s])
        if not t.edge and fam.sel is not None:
            lo, hi = b[ks[s]]
            assert bounds[s] >= 1.02 * lo and bounds[s] <= hi / 1.02, (what, t, lo, hi)
    # 2. tolerance: finite, from the own-precision restatement; every reference element is positive (no cancellation: the
    #    elementwise relative error is meaningful)
    eps = float(np.finfo(fam.io).eps)
    assert np.all(np.isfinite(c["tol"])) and np.all(c["tol"] >= 32 * eps) and np.all(c["tol"] == np.maximum(6 * c["err_own"], 32 * eps))
    assert np.all(c["tol"] < 2e4 * eps), (what, c["tol"].max() / eps)        # (the own-precision evaluation is a sane one)
    for k in names:
        assert np.all(c["ref"][k] > 0), (what, k)
    # 3. sensitivity, at the point that pins each order
    for s, t in enumerate(tg):
        if t.pin and ks[s] != X.PIVOT and X.pinned(fam_name):
            assert c["err_mut"][s] >= 3 * c["tol"][s], (what, t, c["err_mut"][s], c["tol"][s])
    return {(fam_name, ks[s]) for s, t in enumerate(tg)
            if (t.pin and X.pinned(fam_name) and c["err_mut"][s] >= 3 * c["tol"][s]) or (ks[s] == X.PIVOT and not t.edge)}


@pytest.mark.parametrize("fam,N,ns,dsym", X.IA_CASES)
def test_interaction_cases(fam, N, ns, dsym):
    tg, c = X.ia_case(fam, N, ns, dsym, True)
    _check(fam, tg, c, X.IA_OUT, (fam, N, ns, dsym))
    # 4. the long-double reference says interaction!(_11) as the oracle does (two inverses there, one here)
    comp = O.CompositeLayer(**{k: v.astype(np.float64) for k, v in c["comp"].items()})
    add = O.AddedLayer(**{k: v.astype(np.float64) for k, v in c["add"].items()})
    O.interaction("11", comp, add, np.float64)
    for k in X.IA_OUT:
        assert X.relerr(getattr(comp, k), c["ref"][k]).max() < 1e-12, (k, X.relerr(getattr(comp, k), c["ref"][k]).max())


@pytest.mark.parametrize("fam,N,nd", X.DBL_CASES)
def test_doubling_cases(fam, N, nd):
    tg, c = X.dbl_case(fam, N, nd, True)
    _check(fam, tg, c, X.DBL_OUT, (fam, N, nd))
    assert len(c["sel"]) == nd
    for b, ks in c["sel"]:                                 # every step stays a contraction, and no bound sits next to 0.3
        assert b.max() < 0.95
    if nd > 1 and X.FAMILIES[fam].sel is not None:        # the order climbs inside the launch, for most points
        first, last = c["sel"][0][1], c["sel"][-1][1]
        assert sum(a != b for a, b in zip(first, last)) > len(tg) // 2, (first, last)
    lay = c["lay"]
    add = O.AddedLayer(lay["r_mp"].astype(np.float64), lay["t_pp"].astype(np.float64), np.zeros((len(tg), N, N)), np.zeros((len(tg), N, N)),
                       lay["j0_p"].astype(np.float64), lay["j0_m"].astype(np.float64))
    O.doubling(O.polarization("I"), lay["expk"].astype(np.float64), nd, add, np.float64)
    for k in X.DBL_OUT:
        assert X.relerr(getattr(add, k), c["ref"][k]).max() < 1e-12, k
    assert np.array_equal(add.r_pm, add.r_mp) and np.array_equal(add.t_mm, add.t_pp)


def oracle_layer(n, FT):
    """The thin Rayleigh layer of X.LAYER_CASES from the oracle's elemental! (the GPU test reads it back from the device's)."""
    pol = O.polarization("I")
    l = X.l_trunc_for(n, lambda l: O.rt_set_streams_gausslegquad(l, X.LAYER_SZA, [X.LAYER_VZA], pol).Nquad)
    qp = O.rt_set_streams_gausslegquad(l, X.LAYER_SZA, [X.LAYER_VZA], pol)
    Zpp, Zmp = O.compute_Z_moments(pol, qp.qp_mu, O.get_greek_rayleigh(X.LAYER_DEPOL), 0)
    added = O.make_added_layer(FT, n, 1)
    with np.errstate(over="ignore"):          # (Float32: the branch of expdiff that np.where does not take overflows)
        O.elemental(pol, np.zeros(1), np.array([X.LAYER_DTAU]), np.ones((1, 1)), np.array([X.LAYER_VARPI]), Zpp, Zmp, 0, 0, qp, added,
                    FT)
    return {k: getattr(added, k)[0] for k in ("r_mp", "t_pp", "r_pm", "t_mm", "j0_p", "j0_m")}


@lru_cache(maxsize=None)
def _layer(fam, n):
    add1 = oracle_layer(n, X.FAMILIES[fam].io)
    assert all(np.all(v >= 0) for v in add1.values()) and np.all(add1["j0_p"] + add1["j0_m"] > 0)
    return X.layer_case(fam, n, add1, True)


@pytest.mark.parametrize("fam,n", X.LAYER_CASES + X.FORWARD_CASES)
def test_layer_kernel_cases(fam, n):
    tg, c = _layer(fam, n)
    _check(fam, tg, c, X.IA_OUT, (fam, n))


PAIR_CASES = [("strip32", 65), ("strip32", 78), ("strip32", 96)]
PAIR_LAYER_CASES = [("native32", 65), ("native32", 96)]


@lru_cache(maxsize=None)
def _pairs(fam, N):
    tg, perm = X.pair_targets(fam)
    return tg, X.interaction_case(fam, N, tg, 17 * N, with_mutant=True)


@lru_cache(maxsize=None)
def _pairs_layer(fam, n):
    tg, perm = X.pair_targets(fam)
    return X.layer_case(fam, n, oracle_layer(n, X.FAMILIES[fam].io), True, tg=tg)


@pytest.mark.parametrize("fam,N", PAIR_CASES)
def test_pair_batches(fam, N):
    """Batch A holds every ordered pair of the family's branches in adjacent points; batch B pairs each point with its own order."""
    tg, perm = X.pair_targets(fam)
    ks = [t.orders[0] for t in tg]
    nb = len(X.bands(fam))
    assert len(tg) == 2 * nb * nb + 1 and sorted(perm) == list(range(len(tg)))
    assert {(ks[2 * w], ks[2 * w + 1]) for w in range(nb * nb)} == {(a, b) for a in X.bands(fam) for b in X.bands(fam)}
    kb = [ks[i] for i in perm]
    assert all(kb[2 * w] == kb[2 * w + 1] for w in range(nb * nb)) and perm[-1] == len(tg) - 1
    _, c = _pairs(fam, N)
    _check(fam, tg, c, X.IA_OUT, (fam, N, "pairs"))


@pytest.mark.parametrize("fam,n", PAIR_LAYER_CASES)
def test_pair_batches_of_the_native_layer_kernel(fam, n):
    tg, c = _pairs_layer(fam, n)
    _check(fam, tg, c, X.IA_OUT, (fam, n, "pairs"))


@pytest.mark.parametrize("grid", [256, 304, 7])
def test_persistent_plan_walks_every_branch_in_every_workgroup(grid):
    seq, plan = X.persistent_plan("strip128", grid)
    ks = list(X.bands("strip128"))
    assert len(plan) >= 3 * grid and seq[:3] == [X.PIVOT, 1, 31]
    for w in range(grid):
        walk = [ks[i] for i in plan[w::grid]]
        assert sorted(walk) == sorted(ks), (w, walk)
    w0 = [ks[i] for i in plan[0::grid]]                      # workgroup 0 walks seq itself
    assert w0 == seq


def test_every_reachable_order_of_every_family_is_pinned():
    """From the restated rule, not by hand: every order the rule of a family can select occurs in a case above whose bound sits 2 %
    inside the band and whose series, cut at K // 2, misses the tolerance threefold (the pivoted branch: a point at 0.31 .. 0.9).
    k_ia128<float> / k_dbl128<float> pin no series order (X.pinned): they are left out by name, and only their pivoted branch is
    asked for.  (The cases are those of the tests above, evaluated once per process.)"""
    covered = set()
    for fam, N, ns, dsym in X.IA_CASES:
        covered |= _check(fam, *X.ia_case(fam, N, ns, dsym, True), X.IA_OUT, (fam, N))
    for fam, N, nd in X.DBL_CASES:
        covered |= _check(fam, *X.dbl_case(fam, N, nd, True), X.DBL_OUT, (fam, N, nd))
    for fam, n in X.LAYER_CASES + X.FORWARD_CASES:
        covered |= _check(fam, *_layer(fam, n), X.IA_OUT, (fam, n))
    fams = {c[0] for c in X.IA_CASES + X.DBL_CASES + X.LAYER_CASES + X.FORWARD_CASES if X.FAMILIES[c[0]].sel is not None}
    assert fams == {"native64", "strip64", "strip128", "strip128_f32", "fused32", "strip32", "native32"}
    missing = [(f, K) for f in sorted(fams) for K in X.reachable(f) if (f, K) not in covered and (X.pinned(f) or K == X.PIVOT)]
    assert not missing, missing
    assert not X.pinned("strip128_f32") and all(X.pinned(f) for f in fams - {"strip128_f32"})
    assert sum(len(X.reachable(f)) for f in fams if X.pinned(f)) == 3 * 10 + 3 * 8
