"""Every inverse order of the layer-step kernels, alone and paired, against a long-double reference (tests/inverse_order_cases.py;
its CPU checks: tests/test_oracle_inverse_orders.py).  Each batch holds one point per band of the family's selection rule (0.9 x the
upper edge, 1.1 x the lower edge), the pivoted bounds 0.31, 0.5, 0.9 and two points next to every band edge; every output array is
compared elementwise and relatively, with a tolerance sized by the own-precision restatement of the same step (never by a kernel).
Each test asserts the kernel family it landed on where vsm_device_status says so (words [2] / [3]: points of k_dbl128 / k_ia128)
and the exact number of pivoted inverses (word [1]) where the family counts them.

  a. interaction!(_11) on arbitrary arrays: k_ia_native, k_ia128, k_interaction11<float>, k_ia_strip32, k_ia128<float>
  b. doubling! on arbitrary arrays: k_dbl128 (double and float) and the operator-level chain, one step and three
  c. the native run's layer kernels k_layer_native / k_layer_native32 through the C ABI (import, one layer step, export), and the
     reference-layout layer kernels k_layer_strip / k_layer_strip32 through vsm_layer_forward
  d. two points per workgroup (k_ia_strip32, k_layer_native32): every ordered pair of branches, bit-identical to own-order pairs
  e. persistent workgroups (k_ia128, k_dbl128): one workgroup walks through all ten branches, bit-identical to single launches"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import inverse_order_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _status(vsm):
    """Read and reset vsm_device_status (raises on a singular / non-finite flag in word [0])."""
    torch.cuda.synchronize()
    vsm._lib.check_device_status("inverse orders")
    return list(vsm._lib.last_device_status)


def _upload(vsm, arch, obj, arrays, io):
    CR = vsm.CoreRT
    conv_v = vsm.Architectures.array_type(arch)
    for k, v in arrays.items():
        if getattr(obj, k, None) is None:
            continue                                    # (r+- / t-- of a D-symmetric layer: derived in the kernel)
        getattr(obj, k).copy_(CR.to_device_matrix(v, arch, io) if v.ndim == 3 else conv_v(np.ascontiguousarray(v, dtype=io)))


def _download(vsm, obj, names):
    f, h = vsm.CoreRT.from_device_matrix, vsm.Architectures.to_host
    return {k: (f(getattr(obj, k)) if getattr(obj, k).dim() == 3 else h(getattr(obj, k))) for k in names}


def _interaction(vsm, arch, comp, add, io, d_symmetric=0):
    CR = vsm.CoreRT
    S, N = comp["J0_p"].shape
    pc = CR.make_composite_layer(io, arch, (N, N), S)
    pa = CR.make_added_layer(io, arch, (N, N), S, d_symmetric=d_symmetric)
    _upload(vsm, arch, pc, comp, io)
    _upload(vsm, arch, pa, add, io)
    _status(vsm)
    CR.interaction_("11", pc, pa)
    st = _status(vsm)
    return _download(vsm, pc, X.IA_OUT), st


def _doubling(vsm, arch, lay, io, nd):
    CR = vsm.CoreRT
    S, N = lay["j0_p"].shape
    pa = CR.make_added_layer(io, arch, (N, N), S)
    _upload(vsm, arch, pa, {k: lay[k] for k in X.DBL_OUT}, io)
    expk = vsm.Architectures.array_type(arch)(np.ascontiguousarray(lay["expk"], dtype=io))
    _status(vsm)
    CR.doubling_(vsm.host_model.polarization_type("I"), expk, nd, pa)
    st = _status(vsm)
    got = _download(vsm, pa, X.DBL_OUT + ("r_pm", "t_mm"))
    assert np.array_equal(got["r_pm"], got["r_mp"]) and np.array_equal(got["t_mm"], got["t_pp"])     # apply_D! with n_stokes = 1
    return got, st


def _assert_within_tolerance(what, tg, c, got, names):
    """Every array within the per-point tolerance of the reference, elementwise; prints the largest error / tol of the batch."""
    err = np.max([X.relerr(got[k], c["ref"][k]) for k in names], axis=0)
    for k in names:
        assert np.all(np.isfinite(got[k])), (what, k)
    ratio = err / c["tol"]
    s = int(np.argmax(ratio))
    print("inverse orders %s: max error / tol %.3f at '%s' (error %.2e, tol %.2e); median %.3f"
          % (what, ratio[s], tg[s].label, err[s], c["tol"][s], float(np.median(ratio))))
    bad = [(tg[i].label, "%.2e" % err[i], "%.2e" % c["tol"][i]) for i in np.nonzero(ratio > 1)[0]]
    assert not bad, (what, bad)


def _assert_status(what, fam, st, sel, S, word):
    """word: the status word that counts the family's points (2: k_dbl128, 3: k_ia128), None for the other families."""
    assert st[0] == 0, (what, st)
    for w in (2, 3):
        assert st[w] == (S if w == word else 0), (what, st)
    if X.FAMILIES[fam].counts:
        lo, hi = X.pivot_count_range(sel)
        assert lo <= st[1] <= hi, (what, st, lo, hi)


# ---- a. interaction, every order, every family ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,N,ns,dsym", X.IA_CASES)
def test_interaction_every_order(vsm, arch, fam, N, ns, dsym):
    """CoreRT.interaction_("11") on arbitrary nonnegative arrays whose R+- puts the kernel's bound on E = R+- r-+ on every target:
    FP64 N <= 64 k_ia_native (row tiles 1-4; 16 and 64 have no spare column), 65..128 k_ia128 (5-8 row tiles); Float32 N <= 64
    k_interaction11, 65..96 k_ia_strip32 (its three launch variants: N % 4 != 0, N <= 80, N > 80), 97..128 k_ia128<float>; general
    added layers, and D-symmetric ones with D = I (n_stokes 1, 2) where the family takes them."""
    tg, c = X.ia_case(fam, N, ns, dsym)
    io = X.FAMILIES[fam].io
    assert (N <= 64) == (fam in ("native64", "fused32")) and (fam != "strip32" or N <= 96) and (fam != "strip128_f32" or N > 96)
    got, st = _interaction(vsm, arch, c["comp"], c["add"], io, d_symmetric=ns if dsym else 0)
    what = "interaction %s N=%d%s" % (fam, N, " D-symmetric" if dsym else "")
    _assert_status(what, fam, st, c["sel"], len(tg), 3 if fam.startswith("strip128") else None)
    if X.FAMILIES[fam].counts:
        assert st[1] == sum(t.orders == (X.PIVOT,) for t in tg), (what, st)
    _assert_within_tolerance(what, tg, c, got, X.IA_OUT)


# ---- b. doubling, every order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,N,nd", X.DBL_CASES)
def test_doubling_every_order(vsm, arch, fam, N, nd):
    """CoreRT.doubling_ on arbitrary nonnegative added layers (n_stokes = 1) with the bound on r r placed the same way: one step (one
    inverse at a known order) and three against three reference steps (the order climbs inside the launch).  vsm_doubling reaches
    k_dbl128 for FP64 65..128 and Float32 97..128 and the operator-level chain (gemm + batch_inv: no series) elsewhere."""
    tg, c = X.dbl_case(fam, N, nd)
    got, st = _doubling(vsm, arch, c["lay"], X.FAMILIES[fam].io, nd)
    what = "doubling %s N=%d ndoubl=%d" % (fam, N, nd)
    _assert_status(what, fam, st, c["sel"], len(tg), 2 if fam.startswith("strip128") else None)
    _assert_within_tolerance(what, tg, c, got, X.DBL_OUT)


# ---- c. the native run's layer kernels ------------------------------------------------------------------------------------------
class _NativeLayer:
    """One thin Rayleigh layer step (ndoubl = 0) of a native-layout run of one Stokes_I moment on an imported composite, as
    test_native_run_layer_by_layer_through_the_c_abi drives the C ABI.  The added layer of the reference is read back from the
    device's elemental_doubling_ for the same optics (not from the kernel under test)."""

    def __init__(self, vsm, arch, fam, n, S):
        H, CR = vsm.host_model, vsm.CoreRT
        self.vsm, self.arch, self.fam, self.n, self.S = vsm, arch, fam, n, S
        self.io = io = X.FAMILIES[fam].io
        pol = H.polarization_type("I")
        l = X.l_trunc_for(n, lambda l: H.rt_set_streams(l, X.LAYER_SZA, [X.LAYER_VZA], pol, io).Nquad)   # (as SHAPES in test_gpu_native.py)
        model = H.model_from_arrays(arch, "I", l, X.LAYER_SZA, [X.LAYER_VZA], [0.0], tau_rayl=np.full((S, 1), X.LAYER_DTAU),
                                    tau_abs=np.full((S, 1), X.LAYER_DTAU * (1 / X.LAYER_VARPI - 1)), depol=X.LAYER_DEPOL, albedo=0.0,
                                    m_max=1, float_type=io)
        self.sc = sc = CR.prepare_scene(model)
        assert sc.N == n
        self.props = sc.moments[0]["layers"][0]["props"]
        conv = vsm.Architectures.array_type(arch)
        self.dtau, self.varpi = conv(np.full(S, X.LAYER_DTAU, dtype=io)), self.props.varpi      # (varpi: tau_rayl / (tau_rayl + tau_abs))
        assert abs(float(self.varpi[0]) - X.LAYER_VARPI) < 1e-6 and tuple(self.varpi.shape) == (S,)
        self.tau_sum = conv(np.zeros(S, dtype=io))
        added = CR.make_added_layer(io, arch, (n, n), S)
        CR.elemental_doubling_(pol, self.tau_sum, self.dtau, sc.F0, self.props, 0, 0, sc.dq, added)
        torch.cuda.synchronize()
        for k in ("r_mp", "t_pp", "r_pm", "t_mm", "j0_p", "j0_m"):
            assert torch.equal(getattr(added, k)[0], getattr(added, k)[S - 1]), k       # the same optics at every point
        self.add1 = {k: v[0] for k, v in _download(vsm, added, ("r_mp", "t_pp", "r_pm", "t_mm", "j0_p", "j0_m")).items()}

    def step(self, comp):
        """import comp, one vsm_run_layer, export; returns (composite, status words)."""
        vsm, sc, n, S, io = self.vsm, self.sc, self.n, self.S, self.io
        L, CR = vsm._lib.lib(), vsm.CoreRT
        f32 = io == np.float32
        tdt = torch.float32 if f32 else torch.float64
        ci, co = CR.make_composite_layer(io, self.arch, (n, n), S), CR.make_composite_layer(io, self.arch, (n, n), S)
        _upload(vsm, self.arch, ci, comp, io)
        for t in (co.R_mp, co.R_pm, co.T_pp, co.T_mm, co.J0_p, co.J0_m):
            t.fill_(float("nan"))
        carr, marr = (C.c_int * 1)(int(sc.coupling[0])), (C.c_int * 1)(0)
        nbytes = int((L.vsm_run_workspace_bytes_f32 if f32 else L.vsm_run_workspace_bytes)(n, 1, S, 1, carr))
        assert nbytes > 0
        ws = torch.full((nbytes // np.dtype(io).itemsize,), float("nan"), dtype=tdt, device="cuda:0")     # NaN-poisoned workspace
        q = sc.dq.cstruct()
        run = C.c_void_p()
        vsm._lib.check((L.vsm_run_create_f32 if f32 else L.vsm_run_create_f64)(C.byref(q), S, 1, marr, carr, C.c_void_p(ws.data_ptr()),
                                                                              nbytes, C.byref(run)))
        try:
            cin, cout = (type(ci.cstruct()) * 1)(ci.cstruct()), (type(co.cstruct()) * 1)(co.cstruct())
            vsm._lib.check((L.vsm_run_import_f32 if f32 else L.vsm_run_import_f64)(run, cin, None))
            _status(vsm)
            p = self.props
            zpp, zmp = (C.c_void_p * 1)(p.Zpp.data_ptr()), (C.c_void_p * 1)(p.Zmp.data_ptr())
            CR.run_layer_native_(run, 1, 0, self.dtau, self.varpi, self.tau_sum, sc.F0, 0, zpp, zmp, p.z_stride, None, False, dtype=tdt)
            st = _status(vsm)
            vsm._lib.check((L.vsm_run_export_f32 if f32 else L.vsm_run_export_f64)(run, cout, None))
            torch.cuda.synchronize()
        finally:
            L.vsm_run_destroy(run)
        return _download(vsm, co, X.IA_OUT), st


    def forward(self, comp):
        """vsm_layer_forward (elemental! + interaction!(_11) in the reference-layout layer kernel) in place on comp."""
        vsm, sc, n, S, io = self.vsm, self.sc, self.n, self.S, self.io
        CR = vsm.CoreRT
        pc = CR.make_composite_layer(io, self.arch, (n, n), S)
        _upload(vsm, self.arch, pc, comp, io)
        _status(vsm)
        CR.layer_forward_(self.tau_sum, self.dtau, sc.F0, self.props, 0, 0, sc.dq, False, pc, CR.make_added_layer(io, self.arch, (n, n), S))
        st = _status(vsm)
        return _download(vsm, pc, X.IA_OUT), st


@pytest.mark.parametrize("fam,n", X.FORWARD_CASES)
def test_reference_layout_layer_kernels_every_order(vsm, arch, fam, n):
    """The layer kernels behind vsm_layer_forward on the reference's arrays: k_layer_strip (FP64, 33..64 rows -- the inverse of
    vsm_strip_dev.h, which interaction_ no longer reaches) and k_layer_strip32 (Float32, 65..96: the inverse of vsm_strip32.hip once
    more, behind an elemental pre-pass), one thin Rayleigh layer (ndoubl = 0) on an arbitrary composite."""
    nl = _NativeLayer(vsm, arch, fam, n, len(X.targets(fam)))
    tg, c = X.layer_case(fam, n, nl.add1)
    got, st = nl.forward(c["comp"])
    what = "layer_forward %s rows=%d" % (fam, n)
    _assert_status(what, fam, st, c["sel"], len(tg), None)
    _assert_within_tolerance(what, tg, c, got, X.IA_OUT)


@pytest.mark.parametrize("fam,n", X.LAYER_CASES)
def test_native_layer_kernels_every_order(vsm, arch, fam, n):
    """k_layer_native (FP64: 16, 40, 64, 79, 96 rows) and k_layer_native32 (60 rows: one point per workgroup; 65, 80, 96: two; 112,
    128: seven / eight row tiles): E = R+- r-+ with the imported R+- scaled per point onto every target, against the long-double
    interaction of the imported composite with the added layer."""
    nl = _NativeLayer(vsm, arch, fam, n, len(X.targets(fam)))
    tg, c = X.layer_case(fam, n, nl.add1)
    got, st = nl.step(c["comp"])
    what = "native layer %s rows=%d" % (fam, n)
    _assert_status(what, fam, st, c["sel"], len(tg), None)
    assert st[1] == sum(t.orders == (X.PIVOT,) for t in tg), (what, st)
    _assert_within_tolerance(what, tg, c, got, X.IA_OUT)


# ---- d. two points per workgroup: every ordered pair ----------------------------------------------------------------------------
def _assert_pairs(what, tg, perm, c, got_a, got_b):
    for k in X.IA_OUT:       # batch B is batch A permuted: every point's outputs bit-identical whatever its partner's order
        same = np.all((got_b[k] == got_a[k][perm]).reshape(len(tg), -1), axis=1)
        bad = [(tg[perm[2 * (i // 2)]].label, tg[perm[min(2 * (i // 2) + 1, len(tg) - 1)]].label) for i in np.nonzero(~same)[0]]
        assert not bad, (what, k, [(tg[perm[i]].label, "in A beside", tg[perm[i] ^ 1].label if perm[i] < len(tg) - 1 else "nobody")
                                   for i in np.nonzero(~same)[0]])
    _assert_within_tolerance(what + " (batch A)", tg, c, got_a, X.IA_OUT)


@pytest.mark.parametrize("N", [65, 78, 96])
def test_strip32_interaction_every_ordered_pair(vsm, arch, N):
    """k_ia_strip32 puts the points 2w and 2w + 1 in workgroup w (launch_ia32: grid (S + 1) / 2, 2 FNT threads; the point of a thread
    is 2 blockIdx.x + threadIdx.x / FNT), and the two must walk the same barrier sequence whatever their orders: inverse_barriers
    and the padding barriers of invert_strip.  Batch A: every ordered pair of the eight Float32 branches in adjacent points (and a
    lone 129th point); batch B: the same points, each beside a point of its own order."""
    tg, perm = X.pair_targets("strip32")
    assert len(tg) == 129
    c = X.interaction_case("strip32", N, tg, 17 * N, with_mutant=False)
    got_a, st = _interaction(vsm, arch, c["comp"], c["add"], np.float32)
    assert st[0] == 0 and st[2] == 0 and st[3] == 0, st
    got_b, st = _interaction(vsm, arch, X._pick(c["comp"], perm), X._pick(c["add"], perm), np.float32)
    assert st[0] == 0, st
    _assert_pairs("strip32 pairs N=%d" % N, tg, perm, c, got_a, got_b)


@pytest.mark.parametrize("n", [65, 96])
def test_native32_layer_every_ordered_pair(vsm, arch, n):
    """k_layer_native32 at five / six row tiles: the points 2w and 2w + 1 share workgroup w (k_layer_native32: s = blockIdx.x PP + pt,
    pt = wave / RT, PP = 2), each walking the other's inverse as well (n32invert_pair, the two passes with the `mine` flag)."""
    tg, perm = X.pair_targets("native32")
    nl = _NativeLayer(vsm, arch, "native32", n, len(tg))
    _, c = X.layer_case("native32", n, nl.add1, tg=tg)
    got_a, st = nl.step(c["comp"])
    assert st[0] == 0 and st[1] == sum(t.orders == (X.PIVOT,) for t in tg), st
    got_b, st = nl.step(X._pick(c["comp"], perm))
    assert st[0] == 0 and st[1] == sum(t.orders == (X.PIVOT,) for t in tg), st
    _assert_pairs("native32 layer pairs rows=%d" % n, tg, perm, c, got_a, got_b)


# ---- e. persistent workgroups ---------------------------------------------------------------------------------------------------
def _persistent(vsm, arch, N, kind):
    """k_ia128 / k_dbl128 launch min(S, number of CUs) workgroups, workgroup w walking the points w, w + grid, ...: a batch of ten
    times the grid in which every workgroup meets all ten branches one after the other (one point's inverse leaves LDS state for
    the next point of another order), against the same points run one per launch."""
    CR = vsm.CoreRT
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    seq, plan = X.persistent_plan("strip128", grid)
    ks = list(X.bands("strip128"))
    tg = tuple(X.Target("pivoted", 0.5, (X.PIVOT,)) if K == X.PIVOT else next(t for t in X.targets("strip128") if t.pin and t.orders == (K,))
               for K in ks)
    S = len(plan)
    assert S >= 3 * grid
    idx = torch.as_tensor(plan, device="cuda:0")
    if kind == "interaction":
        c = X.interaction_case("strip128", N, tg, 3 * N, with_mutant=False)
        groups, names, word = (("comp", CR.make_composite_layer), ("add", CR.make_added_layer)), X.IA_OUT, 3
        inputs = dict(comp=c["comp"], add=c["add"])
    else:
        c = X.doubling_case("strip128", N, tg, 3 * N, with_mutant=False)
        groups, names, word = (("add", CR.make_added_layer),), X.DBL_OUT, 2
        inputs = dict(add={k: c["lay"][k] for k in X.DBL_OUT})
    pol = vsm.host_model.polarization_type("I")
    conv = vsm.Architectures.array_type(arch)

    def run(n_pts, pick):
        objs = {g: make(np.float64, arch, (N, N), n_pts) for g, make in groups}
        small = {g: make(np.float64, arch, (N, N), len(tg)) for g, make in groups}
        for g in objs:
            _upload(vsm, arch, small[g], inputs[g], np.float64)
            for k in inputs[g]:
                getattr(objs[g], k).copy_(getattr(small[g], k)[pick])
        _status(vsm)
        if kind == "interaction":
            CR.interaction_("11", objs["comp"], objs["add"])
            out = objs["comp"]
        else:
            CR.doubling_(pol, conv(c["lay"]["expk"].astype(np.float64))[pick].contiguous(), 1, objs["add"])
            out = objs["add"]
        st = _status(vsm)
        assert st[0] == 0 and st[word] == n_pts, st
        return {k: getattr(out, k).clone() for k in names}, st
    big, st = run(S, idx)
    assert st[1] == int(np.sum(np.array(ks)[plan] == X.PIVOT)), st
    singles = [run(1, torch.as_tensor([b], device="cuda:0"))[0] for b in range(len(tg))]
    for k in names:
        one = torch.cat([s_[k] for s_ in singles])
        same = (big[k] == one[idx]).reshape(S, -1).all(dim=1)
        bad = torch.nonzero(~same).flatten().tolist()
        assert not bad, (kind, N, k, [(s_, "workgroup %d" % (s_ % grid), "after order %s" % (ks[plan[s_ - grid]] if s_ >= grid else "-"),
                                       "order %s" % ks[plan[s_]]) for s_ in bad[:8]])
    got = {k: (vsm.CoreRT.from_device_matrix(torch.cat([s_[k] for s_ in singles])) if singles[0][k].dim() == 3
               else vsm.Architectures.to_host(torch.cat([s_[k] for s_ in singles]))) for k in names}
    _assert_within_tolerance("persistent %s N=%d (single launches)" % (kind, N), tg, c, got, names)


@pytest.mark.parametrize("N", [97, 128])
def test_persistent_interaction_walks_every_branch(vsm, arch, N):
    _persistent(vsm, arch, N, "interaction")


@pytest.mark.parametrize("N", [97, 128])
def test_persistent_doubling_walks_every_branch(vsm, arch, N):
    _persistent(vsm, arch, N, "doubling")
