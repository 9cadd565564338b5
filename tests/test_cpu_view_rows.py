"""CPU tests of the view-row native run (VSM_RUN_VIEW_ROWS, csrc/vsm_native.hip): the flag plumbing of core_rt, the mapping of the
global viewing rows to (block, local row) through the Stokes groups of a run, and the error paths of the C ABI."""
import ctypes as C

import numpy as np
import pytest

VIEW_MAX = 16
SRC, ZW, VIEW = 1, 2, 4


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


def _create(vsm, N, ns, coupling, flags, rows, view_entry=True):
    """A run of S = 0 points on a dummy workspace (nothing is launched): returns (rc, run)."""
    L = vsm._lib.lib()
    nm = len(coupling)
    mu = (C.c_double * N)(*([0.5] * N))
    wt = (C.c_double * N)(*([1.0] * N))
    q = vsm._lib.vsm_quad_f64(C.cast(mu, C.c_void_p).value, C.cast(wt, C.c_void_p).value, N, ns, 0, 0.5)
    marr, carr = (C.c_int * nm)(*range(nm)), (C.c_int * nm)(*coupling)
    ws = (C.c_double * 2)()
    run = C.c_void_p()
    if view_entry:
        rarr = (C.c_int * max(len(rows), 1))(*rows)
        rc = L.vsm_run_create_view_f64(C.byref(q), 0, nm, marr, carr, C.cast(ws, C.c_void_p), 16, flags, len(rows), rarr,
                                       C.byref(run))
    else:
        rc = L.vsm_run_create_ex_f64(C.byref(q), 0, nm, marr, carr, C.cast(ws, C.c_void_p), 16, flags, C.byref(run))
    return rc, run, (mu, wt, ws, q)


def _blocks(vsm, run):
    L = vsm._lib.lib()
    out, b = [], 0
    while True:
        im, n, nv = C.c_int(), C.c_int(), C.c_int()
        rows = (C.c_int * VIEW_MAX)()
        if L.vsm_run_view_block(run, b, C.byref(im), C.byref(n), C.byref(nv), rows):
            return out
        out.append((im.value, n.value, list(rows[:nv.value])))
        b += 1


def test_switch_and_symbols(vsm):
    """The view-row run is the default of Scene.run beside the sources-only run; the plain sources-only run stays reachable."""
    import inspect
    CR = vsm.CoreRT
    assert CR.NATIVE_VIEW_ROWS is True and CR.NATIVE_SOURCES_ONLY is True and CR.VIEW_ROWS_MAX == VIEW_MAX
    sig = inspect.signature(CR.Scene._run_layers_native)
    assert sig.parameters["view_rows"].default is None          # multi-sensor runs and direct callers: the whole T--
    syms = vsm._lib.exported_symbols()
    for s in ("vsm_run_create_view_f64", "vsm_run_create_view_f32", "vsm_run_view_rows", "vsm_run_view_block"):
        assert s in syms


def test_view_rows_of_index_rule(vsm):
    """view_rows_of: the n_stokes rows of each VZA's node (postprocessing_vza_'s argmin rule), each node once."""
    CR, H = vsm.CoreRT, vsm.host_model

    class QP:
        qp_mu = np.array([0.1, 0.5, 0.9, H.cosd(30.0), H.cosd(40.0)])

    class Pol:
        n = 3

    assert CR.view_rows_of(Pol, [30.0], QP) == [9, 10, 11]
    assert CR.view_rows_of(Pol, [40.0, 30.0, 40.0], QP) == [12, 13, 14, 9, 10, 11]
    QP.qp_mu = np.array([0.1, H.cosd(60.0), 0.9, H.cosd(30.0)])       # a VZA on a Gauss-Legendre node: an inner row
    assert CR.view_rows_of(Pol, [60.0, 30.0], QP) == [3, 4, 5, 9, 10, 11]


def test_run_create_flags(vsm, monkeypatch):
    """run_create_: sources-only + rows -> vsm_run_create_ex(flags = 1) then vsm_run_view_rows; every other combination leaves
    the rows alone (the switch off, a full run, too many rows, a Float32 model)."""
    import torch
    CR = vsm.CoreRT
    calls = []

    class FakeLib:
        def vsm_run_view_rows(self, run, n, rows):
            calls.append(("rows", n, list(rows[:n])))
            return 0

        def vsm_run_destroy(self, run):
            return 0

    monkeypatch.setattr(vsm._lib, "call", lambda name, dtype, *a: calls.append((name, int(a[7]))))
    monkeypatch.setattr(vsm._lib, "lib", lambda: FakeLib())
    monkeypatch.setattr(CR, "_ptr", lambda t: None)
    q = C.c_int(0)
    args = (q, 1, 1, None, None, None, 0)
    CR.run_create_(torch.float64, *args, True, [9, 10, 11], C.c_void_p())
    assert calls == [("vsm_run_create_ex", 1), ("rows", 3, [9, 10, 11])]
    for dtype, src, rows, switch in ((torch.float64, False, [9], True), (torch.float64, True, None, True),
                                     (torch.float64, True, list(range(17)), True), (torch.float32, True, [9], True),
                                     (torch.float64, True, [9], False)):
        calls.clear()
        monkeypatch.setattr(CR, "NATIVE_VIEW_ROWS", switch)
        CR.run_create_(dtype, *args, src, rows, C.c_void_p())
        assert calls == [("vsm_run_create_ex", 1 if src else 0)], (dtype, src, rows, switch, calls)


@pytest.mark.parametrize("ns,nq", [(3, 20), (4, 13), (1, 16)])
def test_row_mapping_through_the_groups(vsm, ns, nq):
    """m = 0 ((I,Q) | (U,V) blocks, and every component on its own) and m > 0 (dense): global row node ns + a lies in the block of
    component a at local row node gsz + (position of a in the block); a block without viewing rows carries none."""
    L = vsm._lib.lib()
    N = ns * nq
    iq_uv = sum(1 << (4 * a + b) for a in range(ns) for b in range(ns) if (a < 2) == (b < 2))
    diag = sum(1 << (5 * a) for a in range(ns))
    nodes = [nq - 1, 3]
    rows = [nd * ns + a for nd in nodes for a in range(ns)]
    rc, run, keep = _create(vsm, N, ns, [iq_uv, -1, diag], SRC | VIEW, rows)
    assert rc == 0, L.vsm_last_error()
    try:
        blocks = _blocks(vsm, run)
    finally:
        L.vsm_run_destroy(run)
    groups0 = [[a for a in range(ns) if a < 2], [a for a in range(ns) if a >= 2]]
    groups0 = [g for g in groups0 if g]
    expect = [(0, nq * len(g), [nd * len(g) + k for nd in nodes for k in range(len(g))]) for g in groups0]
    expect += [(1, N, rows)]
    expect += [(2, nq, [nd for nd in nodes]) for _ in range(ns)]
    assert blocks == expect
    # rows of I alone: the (U,V) block of m = 0 and the blocks of Q, U, V of the third moment carry no row
    rc, run, keep = _create(vsm, N, ns, [iq_uv, -1, diag], SRC | VIEW, [nd * ns for nd in nodes])
    assert rc == 0
    try:
        blocks = _blocks(vsm, run)
    finally:
        L.vsm_run_destroy(run)
    assert [len(b[2]) for b in blocks] == [2] + [0] * (len(groups0) - 1) + [2] + [2] + [0] * (ns - 1)


def test_setter_equals_create_time_list(vsm):
    L = vsm._lib.lib()
    rows = [57, 58, 59, 3]
    rc, run, keep = _create(vsm, 60, 3, [0x033 | 0x400, -1], SRC, [], view_entry=False)
    assert rc == 0
    try:
        assert _blocks(vsm, run)[0][2] == []
        assert L.vsm_run_view_rows(run, len(rows), (C.c_int * 4)(*rows)) == 0
        a = _blocks(vsm, run)
    finally:
        L.vsm_run_destroy(run)
    rc, run, keep = _create(vsm, 60, 3, [0x033 | 0x400, -1], SRC | VIEW, rows)
    assert rc == 0
    try:
        assert _blocks(vsm, run) == a and a[0][2] == [38, 39, 2] and a[1][2] == [19] and a[2][2] == rows
    finally:
        L.vsm_run_destroy(run)


def test_error_paths(vsm):
    """Too many rows, an empty list, the flag without sources-only, the flag without a list, rows outside 0 .. N - 1 or listed
    twice, rows without the flag: errors, never a silent fallback."""
    L = vsm._lib.lib()
    bad = [
        (SRC | VIEW, list(range(VIEW_MAX + 1)), True),
        (SRC | VIEW, [], True),
        (VIEW, [3, 4, 5], True),
        (ZW | VIEW, [3], True),
        (SRC | VIEW, [], False),            # vsm_run_create_ex has no list
        (SRC | VIEW, [60], True),
        (SRC | VIEW, [-1], True),
        (SRC | VIEW, [5, 5], True),
        (SRC, [5], True),
        (SRC | VIEW | 8, [5], True),
    ]
    for flags, rows, entry in bad:
        rc, run, keep = _create(vsm, 60, 3, [-1], flags, rows, view_entry=entry)
        assert rc != 0, (flags, rows, entry)
        assert L.vsm_last_error()
    rc, run, keep = _create(vsm, 60, 3, [-1], SRC | VIEW, list(range(VIEW_MAX)))
    assert rc == 0
    L.vsm_run_destroy(run)
    # the setter: a full run refuses the rows
    rc, run, keep = _create(vsm, 60, 3, [-1], 0, [], view_entry=False)
    assert rc == 0
    try:
        assert L.vsm_run_view_rows(run, 1, (C.c_int * 1)(5)) != 0
        assert L.vsm_run_view_rows(run, 0, None) != 0
    finally:
        L.vsm_run_destroy(run)


def test_setter_refused_after_import(vsm):
    """vsm_run_import writes the whole T-- record; the row vectors live at its head: the rows must be set before any import."""
    L = vsm._lib.lib()
    rc, run, keep = _create(vsm, 60, 3, [-1], SRC, [], view_entry=False)
    assert rc == 0
    try:
        buf = (C.c_double * 4)()
        ptr = C.cast(buf, C.c_void_p).value
        cc = (vsm._lib.vsm_composite * 1)(vsm._lib.vsm_composite(ptr, ptr, ptr, ptr, ptr, ptr))
        assert L.vsm_run_import_f64(run, cc, None) == 0          # (S = 0: nothing is read)
        assert L.vsm_run_view_rows(run, 1, (C.c_int * 1)(5)) != 0
    finally:
        L.vsm_run_destroy(run)
