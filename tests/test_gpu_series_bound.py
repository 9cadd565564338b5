"""The FP64 native layer kernels where their series order leaves the Frobenius rule's (vsm_native_dev.h nnorm / ninv_order: the order
from min(Frobenius bound, induced 1-norm); tests/series_bound_cases.py restates it, tests/test_oracle_series_bound.py proves it on
the CPU).  One layer step through the C ABI, driven as test_gpu_inverse_orders.py drives it, at 16 rows (one row tile, no spare
column: the source vectors by mat-vecs), 40 (three row tiles, the parked strips), 60 (four row tiles, rider columns) and 79 (five):

  a. the interaction on an imported composite whose R+- has one dominant row: per series band one point where the Frobenius bound
     selects K and the kernels' rule the order below, and three points the Frobenius bound sends to the pivoted inverse whatever
     the 1-norm says -- elementwise against the long-double interaction, the pivoted inverses counted exactly;
  b. three doubling steps of a thin Stokes_I layer with a grazing viewing stream against the oracle at the 1e-10 gate of
     test_gpu_native.py."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import inverse_order_cases as X  # noqa: E402
import series_bound_cases as B  # noqa: E402
import test_gpu_inverse_orders as T  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
vsm, arch = T.vsm, T.arch
ROWS = [16, 40, 60, 79]
F64, LD = np.float64, np.longdouble


def _ia_targets():
    dep = B.departing_targets()
    tg = [X.Target("K%d by F, K%d by the 1-norm" % (K, Kl), f, (Kl,)) for K, Kl, f, _ in dep]
    return dep, tuple(tg + [X.Target("pivoted %.2f" % x, x, (X.PIVOT,)) for x in X.PIVOT_TARGETS])


def _ia_case(n, add1):
    """comp, add, long-double reference and tolerance of the batch: the random composite of inverse_order_cases with R+- replaced by
    a dominant row over a dense background, the background weighted so that the two bounds on E = R+- r-+ straddle a band edge."""
    dep, tg = _ia_targets()
    S, nd = len(tg), len(dep)
    rng = np.random.default_rng(53 * n)
    add = {k: np.broadcast_to(np.asarray(v, dtype=F64), (S,) + np.shape(v)).copy() for k, v in add1.items()}
    comp = dict(R_mp=X._refl(rng, S, n), T_pp=X._trans(rng, S, n), T_mm=X._trans(rng, S, n), J0_p=rng.random((S, n)), J0_m=rng.random((S, n)))
    graze, dense = B.grazing(rng, S, n), rng.random((S, n, n)) / n
    R = np.empty((S, n, n))
    R[:nd] = B.mix_to_ratio(lambda M: M @ add["r_mp"][:nd], graze[:nd], dense[:nd], [d[2] for d in dep], [d[3] for d in dep])
    R[nd:] = graze[nd:]
    for _ in range(4):
        R[nd:] *= (np.array(X.PIVOT_TARGETS) / B.bound_fro(R[nd:] @ add["r_mp"][nd:]).astype(F64))[:, None, None]
    comp["R_pm"] = R
    E = R @ add["r_mp"]
    assert B.order_fro(E) == [d[0] for d in dep] + [X.PIVOT] * 3 and B.order_one(E) == [t.orders[0] for t in tg], (n, B.order_fro(E), B.order_one(E))
    assert B.bound_one(E[nd:nd + 1])[0] < 0.3         # (the first pivoted point: the 1-norm alone would have taken a series)
    ref, _ = X.interaction_step(comp, add, LD, X.inv_newton)
    own, _ = X.interaction_step(comp, add, F64, lambda e: X.inv_by_orders(e, B.order_one(e)))
    err_own = np.max([X.relerr(own[k], ref[k]) for k in X.IA_OUT], axis=0)
    return tg, dict(comp=comp, add=add, ref=ref, tol=X.tolerance(err_own, F64))


@pytest.mark.parametrize("n", ROWS)
def test_interaction_where_the_one_norm_lowers_the_order(vsm, arch, n):
    nl = T._NativeLayer(vsm, arch, B.FAM, n, len(_ia_targets()[1]))
    tg, c = _ia_case(n, nl.add1)
    got, st = nl.step(c["comp"])
    what = "series bound, native layer rows=%d" % n
    assert st[0] == 0 and st[2] == 0 and st[3] == 0, (what, st)
    assert st[1] == len(X.PIVOT_TARGETS), (what, st)             # the pivot decision is the Frobenius bound's
    T._assert_within_tolerance(what, tg, c, got, X.IA_OUT)


# ---- b. doubling ----------------------------------------------------------------------------------------------------------------
DBL_S, DBL_ND, DBL_TAU, DBL_SZA, DBL_VZA = 4, 3, 0.016, 40.0, 88.0


def _dbl_kw():
    return dict(tau_rayl=np.full((DBL_S, 1), DBL_TAU), tau_abs=np.geomspace(1e-3, 0.05, DBL_S)[:, None], depol=0.03, albedo=0.0, m_max=1)


@lru_cache(maxsize=None)
def _dbl_oracle(l_trunc):
    """The oracle's elemental! + doubling! (ndoubl = 3) of the layer; also the orders the two rules take in its three steps."""
    om = O.build_model("I", l_trunc, DBL_SZA, [DBL_VZA], [0.0], **_dbl_kw())
    props = O.expand_optical_properties(O.construct_core_optical_properties(om, 0)[0], F64)
    qp, N = om.quad_points, om.quad_points.Nquad
    added = O.make_added_layer(F64, N, DBL_S)
    dtau = (props.tau / 2 ** DBL_ND).astype(F64)
    F0 = np.ones((1, DBL_S))
    O.elemental(om.pol, np.zeros(DBL_S), dtau, F0, props.varpi, props.Zpp, props.Zmp, 0, DBL_ND, qp, added, F64)
    steps, inv0 = [], O.batch_inv

    def batch_inv(A):
        steps.append(np.eye(N)[None] - A)
        return inv0(A)
    try:
        O.batch_inv = batch_inv
        O.doubling(om.pol, np.exp(-dtau / F64(qp.mu0)), DBL_ND, added, F64)
    finally:
        O.batch_inv = inv0
    return added, dtau, [(B.order_fro(E), B.order_one(E)) for E in steps]


@pytest.mark.parametrize("n", ROWS)
def test_doubling_with_a_grazing_stream(vsm, arch, n):
    H, L, CR = vsm.host_model, vsm._lib.lib(), vsm.CoreRT
    pol = H.polarization_type("I")
    l = X.l_trunc_for(n, lambda l: H.rt_set_streams(l, DBL_SZA, [DBL_VZA], pol, F64).Nquad)
    ref, dtau, orders = _dbl_oracle(l)
    assert len(orders) == DBL_ND and all(kf != X.PIVOT for step in orders for kf in step[0])
    assert any(k1 < kf for step in orders for kf, k1 in zip(*step)), orders      # the case is one where the rules part
    model = H.model_from_arrays(arch, "I", l, DBL_SZA, [DBL_VZA], [0.0], **_dbl_kw())
    sc = CR.prepare_scene(model)
    assert sc.N == n
    p = sc.moments[0]["layers"][0]["props"]
    conv = vsm.Architectures.array_type(arch)
    carr, marr = (C.c_int * 1)(int(sc.coupling[0])), (C.c_int * 1)(0)
    nbytes = int(L.vsm_run_workspace_bytes(n, 1, DBL_S, 1, carr))
    assert nbytes > 0
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda:0")
    comp = CR.make_composite_layer(F64, arch, (n, n), DBL_S)
    q = sc.dq.cstruct()
    run = C.c_void_p()
    vsm._lib.check(L.vsm_run_create_f64(C.byref(q), DBL_S, 1, marr, carr, C.c_void_p(ws.data_ptr()), nbytes, C.byref(run)))
    try:
        T._status(vsm)
        zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
        CR.run_layer_native_(run, 1, DBL_ND, conv(dtau), p.varpi, conv(np.zeros(DBL_S)), sc.F0, 0, zpp, zmp, p.z_stride, None, True)
        st = T._status(vsm)
        cc = (type(comp.cstruct()) * 1)(comp.cstruct())
        vsm._lib.check(L.vsm_run_export_f64(run, cc, None))
        torch.cuda.synchronize()
    finally:
        L.vsm_run_destroy(run)
    assert st[0] == 0 and st[1] == 0, st
    got = T._download(vsm, comp, X.IA_OUT)
    worst = 0.0
    for name, want in (("R_mp", ref.r_mp), ("R_pm", ref.r_pm), ("T_pp", ref.t_pp), ("T_mm", ref.t_mm), ("J0_p", ref.j0_p), ("J0_m", ref.j0_m)):
        want = np.asarray(want).reshape(got[name].shape)
        assert np.all(np.isfinite(got[name])), name
        rel = np.max(np.abs(got[name] - want)) / np.max(np.abs(want))
        worst = max(worst, rel)
        assert rel < 1e-10, (n, name, rel)
    print("series bound, doubling rows=%d: largest deviation from the oracle %.2e; orders by (F, 1-norm) per step: %s"
          % (n, worst, [(max(a), max(b)) for a, b in orders]))
