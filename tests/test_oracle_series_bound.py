"""The series order from the induced 1-norm (tests/series_bound_cases.py restates vsm_native_dev.h nnorm / ninv_order): never above
the Frobenius rule's order, rigorous -- the dropped tail stays below eps / 4 in every element, evaluated in long double -- and
cheaper on the benchmark's own atmosphere.  numpy only."""
import numpy as np
import pytest

import inverse_order_cases as X
import series_bound_cases as B

TOL = float(np.finfo(np.float64).eps) * 0.25
RULES = (("1-norm", B.order_one), ("1-norm and E^2", B.order_sq))
pytestmark = pytest.mark.skipif(not X.have_long_double(), reason="needs an extended long double")


def _targets(pivoted=True):
    return X.targets(B.FAM, True, pivoted)


def _dense(N):
    tg = _targets()
    comp, add, _ = X.interaction_inputs(B.FAM, N, tg, 31 * N)
    return comp["R_pm"].astype(np.float64) @ add["r_mp"].astype(np.float64)


def _signed(N):
    tg = _targets()
    rng = np.random.default_rng(5 * N)
    return B.scale_to(rng.standard_normal((len(tg), N, N)), [t.bound for t in tg])


def _grazing(N):
    tg = _targets()
    return B.scale_to(B.grazing(np.random.default_rng(7 * N), len(tg), N), [t.bound for t in tg])


def _departing(N):
    dep = B.departing_targets()
    rng = np.random.default_rng(11 * N)
    return B.mix_to_ratio(lambda M: M, B.grazing(rng, len(dep), N), rng.random((len(dep), N, N)) / N, [d[2] for d in dep], [d[3] for d in dep])


CLASSES = {"dense": _dense, "signed": _signed, "grazing": _grazing, "departing": _departing}


@pytest.mark.parametrize("N", [16, 40, 60])
@pytest.mark.parametrize("kind", sorted(CLASSES))
def test_order_is_never_higher_and_the_tail_stays_below_a_quarter_eps(kind, N):
    """(a) the order is the Frobenius rule's or lower, and it is the pivoted inverse exactly where the Frobenius rule says so;
    (b) max_ij |sum_{k > K} E^k| <= eps / 4 at the selected K -- on the dense nonnegative inputs of inverse_order_cases, on signed
    matrices and on matrices with one dominant row, the Frobenius bound inside every band and next to every band edge."""
    E = CLASSES[kind](N)
    kf = B.order_fro(E)
    worst = 0.0
    for name, rule in RULES:
        ks = rule(E)
        for s, (K, Kf) in enumerate(zip(ks, kf)):
            assert (K == X.PIVOT) == (Kf == X.PIVOT), (name, kind, N, s, K, Kf)
            if K == X.PIVOT:
                continue
            assert K <= Kf and K in X.SERIES, (name, kind, N, s, K, Kf)
            t = B.tail_max(E[s], K)
            worst = max(worst, t / TOL)
            assert t <= TOL, (name, kind, N, s, K, Kf, t)
    print("series bound %s N=%d: largest tail / (eps / 4) = %.3f" % (kind, N, worst))


@pytest.mark.parametrize("N", [16, 40, 60, 79])
def test_one_dominant_row_takes_the_next_lower_order(N):
    """The inputs of the GPU test: per band one point where the Frobenius rule selects K and the kernels' rule the order below."""
    dep = B.departing_targets()
    E = _departing(N)
    assert B.order_fro(E) == [d[0] for d in dep]
    assert B.order_one(E) == [d[1] for d in dep]
    # a dominant row alone: the 1-norm bound is a fraction of the Frobenius bound, and orders fall wherever a band is narrower than that
    G = _grazing(N)
    assert np.all(B.bound_one(G) < 0.6 * B.bound_fro(G))
    ser = [(a, b) for a, b in zip(B.order_one(G), B.order_fro(G)) if b != X.PIVOT]
    assert all(a <= b for a, b in ser) and sum(a < b for a, b in ser) >= len(ser) // 3, ser


def _c2_orders():
    """E of every doubling step and of every interaction!(_11) of a cut-down C2: 4 evenly spaced points of the benchmark's O2-A
    atmosphere, its first 6 layers, m = 0..2, recorded from the oracle's batch_inv (of the two inverses of an interaction the first,
    I - r-+ R+-: the one the sources-only kernels form).  m = 0 splits into the (I, Q) and the U block, as the native run does."""
    import bench
    from oracle import vsm_oracle as O
    tau_rayl, tau_abs = bench.o2a_atmosphere(10000, 40)
    idx = np.linspace(0, 9999, 4).round().astype(int)
    cfg = bench.CONFIGS["C2"]
    model = O.build_model(cfg["pol"], cfg["l_trunc"], 40.0, [30.0], [0.0], tau_rayl=tau_rayl[idx, :6], tau_abs=tau_abs[idx, :6],
                          depol=0.0279, albedo=0.15, m_max=2)
    rec, state = [], dict(kind=None, first=True, m=0)
    inv0, dbl0, ia0, core0 = O.batch_inv, O.doubling, O.interaction, O.construct_core_optical_properties

    def batch_inv(A):
        if state["kind"] == "doubling" or (state["kind"] == "interaction" and state["first"]):
            E = np.eye(A.shape[-1])[None] - A
            blocks = [np.arange(A.shape[-1])]
            if state["m"] == 0:
                c = np.arange(A.shape[-1]) % 3
                blocks = [np.nonzero(c < 2)[0], np.nonzero(c == 2)[0]]
                assert np.all(E[:, blocks[0]][:, :, blocks[1]] == 0) and np.all(E[:, blocks[1]][:, :, blocks[0]] == 0)
            rec.extend((state["kind"], E[:, b][:, :, b]) for b in blocks)
        state["first"] = False
        return inv0(A)

    def wrap(kind, f):
        def g(*a, **k):
            state.update(kind=kind, first=True)
            try:
                return f(*a, **k)
            finally:
                state["kind"] = None
        return g

    def core(model, m):
        state["m"] = m
        return core0(model, m)
    try:
        O.batch_inv, O.doubling, O.interaction, O.construct_core_optical_properties = batch_inv, wrap("doubling", dbl0), wrap("interaction", ia0), core
        O.rt_run(model)
    finally:
        O.batch_inv, O.doubling, O.interaction, O.construct_core_optical_properties = inv0, dbl0, ia0, core0
    return rec


def test_fewer_series_products_on_the_benchmark_atmosphere():
    """(c) mean series products per inverse on the cut-down C2: the kernels' rule strictly below the Frobenius rule, the rule with
    the bound on E^2 not above the kernels'."""
    rec = _c2_orders()
    assert sum(k == "doubling" for k, _ in rec) >= 3 * 6 * 8 and sum(k == "interaction" for k, _ in rec) >= 3 * 5
    cost = {}
    for name, rule in (("Frobenius", B.order_fro),) + RULES:
        tot = n = 0
        for kind, E in rec:
            table = B.PRODUCTS_IA if kind == "interaction" else B.PRODUCTS
            ks = rule(E)
            tot += sum(table[K] for K in ks)
            n += len(ks)
        cost[name] = tot / n
    print("series products per inverse on the cut-down C2: %s" % ", ".join("%s %.3f" % kv for kv in cost.items()))
    assert cost["1-norm"] < cost["Frobenius"], cost
    assert cost["1-norm and E^2"] <= cost["1-norm"], cost
