"""GPU tests of thermal emission in the multi-sensor run (vsm.CoreRT.rt_run_multisensor(..., thermal=True), core_rt_ms.py) and of
its multi-source level kernel (vsm_level_radiance_src_*, csrc/vsm_level.hip): against the statement-order oracle
(tests/ms_thermal_oracle.py + tests/ms_oracle.py), level 0 against rt_run bit for bit, the kernel against the one-source entry point
(n_src = 1, bit for bit) and against accumulated operator-level calls (n_src = 2), the flags, poisoned work buffers and the
library calls the host issues."""
import collections
import ctypes as C
import dataclasses
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ms_oracle as MS  # noqa: E402
import ms_thermal_oracle as MT  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from level_cases import contractive  # noqa: E402
from test_gpu_multisensor import _err_per_level, _pair, _sub  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _sources(vsm, B, solar):
    H = vsm.host_model
    return (H.SolarBeam(), H.ThermalEmission(B_layer=B)) if solar else (H.ThermalEmission(B_layer=B),)


def _solar_oracle_model(om, solar):
    """The oracle model of the solar slot: F0 = 0 without a SolarBeam (Scene.__init__'s rule; the Lambertian surface layer keeps
    its beam term)."""
    return om if solar else dataclasses.replace(om, F0=np.zeros((om.pol.n, om.tau_rayl.shape[0]), dtype=om.FT))


CASES = [
    # (id, pol, l_trunc, S, Nz, levels, kwargs): shapes of test_gpu_multisensor.py's CASES
    ("scalar_n8", "I", 10, 5, 6, [3, 0, 6, 1], dict(m_max=3)),
    ("c2_like_n60_iqu", "IQU", 35, 2000, 40, [0, 1, 20, 39, 40], dict()),
    ("iquv_n112_aerosols", "IQUV", 50, 3, 5, [1, 3, 5], dict(aerosols=True, m_max=4)),
    ("scalar_n135_oplevel", "I", 264, 2, 4, [1, 2, 0], dict()),
    ("s3_unsorted_duplicates", "IQU", 9, 3, 6, [5, 2, 5, 0, 2, 6, 1], dict(m_max=3)),
    ("iqu_n60_fused_slot", "IQU", 31, 6, 7, [2, 0, 5, 7], dict(m_max=3)),     # the slot's layer step in vsm_layer_forward_thermal
]


@pytest.mark.parametrize("solar", [True, False], ids=["solar+thermal", "thermal_only"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_multisensor_thermal_against_oracle_fp64(vsm, arch, case, solar):
    """e <= max(1e-9, 2 e_rt): 1e-9 is test_gpu_thermal.py's bound of rt_run's slot against the oracle, e_rt the deviation of the
    device's rt_run with the same sources from O.rt_run + O.rt_run_thermal on the same points (test_gpu_multisensor.py's rule)."""
    name, pol, lt, S, L, levels, kw = case
    pm, om = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(len(name)), **kw)
    B = 0.05 + 0.1 * np.random.default_rng(len(name) + 1).random((L, S))
    pm.sources = _sources(vsm, B, solar)
    N = pm.quad_points.Nquad * pm.polarization_type.n
    if name.startswith("scalar_n135"):
        assert N > 128
    assert bool(vsm._lib.lib().vsm_layer_thermal_fused(N, 1)) == name.endswith("fused_slot")
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=True)
    R, T = vsm.CoreRT.rt_run(pm)
    idx = np.unique(np.r_[0, 1, S // 4, S // 2, S - 2, S - 1].clip(0, S - 1)) if S > 8 else np.arange(S)
    oms, Bs = _sub(om, idx), B[:, idx]
    ur, dr = MT.ms_total_reference(oms, Bs, levels, solar=solar)
    ut, _ = MT.ms_thermal_reference(oms, Bs, levels)
    per = [max(_err_per_level([uw[i][..., idx]], [ur[i]]), _err_per_level([dw[i][..., idx]], [dr[i]])) for i in range(len(levels))]
    e = max(per)
    Rs, Ts = O.rt_run(_solar_oracle_model(oms, solar))
    Rt, Tt = O.rt_run_thermal(oms, Bs)
    e_rt = max(_err_per_level([R[..., idx]], [Rs + Rt]), _err_per_level([T[..., idx]], [Ts + Tt]))
    print("MS-TH %-24s %-13s N %3d S %4d levels %s: rel err %s (rt_run %.2e)"
          % (name, "solar+thermal" if solar else "thermal_only", N, S, levels, " ".join("%.2e" % x for x in per), e_rt))
    assert e <= max(1e-9, 2 * e_rt), (name, solar, e, e_rt)
    for i, l in enumerate(levels):
        assert np.all(np.isfinite(uw[i])) and np.all(np.isfinite(dw[i]))
        if l < L or om.albedo != 0:      # the thermal slot is part of every level
            assert np.max(np.abs(ut[i][:, 0])) > 0, (name, l)
        if l == 0:                       # level 0 is rt_run with the same sources, bit for bit
            assert np.array_equal(uw[i], R) and np.array_equal(dw[i], T)
    for i, l in enumerate(levels):       # duplicates: the same arrays
        j = levels.index(l)
        assert np.array_equal(uw[i], uw[j]) and np.array_equal(dw[i], dw[j])


@pytest.mark.parametrize("solar", [True, False], ids=["solar+thermal", "thermal_only"])
def test_level0_is_rt_run_bit_for_bit(vsm, arch, solar):
    pm, _ = _pair(vsm, arch, "IQU", 35, 12, 8, np.random.default_rng(5), aerosols=True, m_max=4)
    pm.sources = _sources(vsm, 0.05 + 0.1 * np.random.default_rng(6).random((8, 12)), solar)
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, [0, 3, 0], thermal=True)
    R, T = vsm.CoreRT.rt_run(pm)
    for i in (0, 2):
        assert np.array_equal(uw[i], R) and np.array_equal(dw[i], T)
    assert np.max(np.abs(R)) > 0


@pytest.mark.parametrize("pol,lt", [("I", 35), ("IQU", 55)], ids=["scalar_n22", "n96_iqu_fused_slot"])
def test_multisensor_thermal_float32(vsm, arch, pol, lt):
    """The bound of test_gpu_multisensor.py::test_multisensor_float32."""
    pm, om32 = _pair(vsm, arch, pol, lt, 5, 8, np.random.default_rng(4), FT=np.float32, m_max=3)
    B = (0.05 + 0.1 * np.random.default_rng(5).random((8, 5))).astype(np.float32)
    pm.sources = _sources(vsm, B, True)
    N = pm.quad_points.Nquad * pm.polarization_type.n
    assert bool(vsm._lib.lib().vsm_layer_thermal_fused(N, 0)) == (pol == "IQU")      # FP32, 64 < N <= 96: the fused slot step
    levels = [0, 2, 5, 8]
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=True)
    R, T = vsm.CoreRT.rt_run(pm)
    assert uw[0].dtype == np.float32
    assert np.array_equal(uw[0], R) and np.array_equal(dw[0], T)
    ur, dr = MT.ms_total_reference(O.exact_model(om32), B.astype(np.float64), levels)
    ut, _ = MT.ms_thermal_reference(O.exact_model(om32), B.astype(np.float64), levels)
    for i in range(1, len(levels)):
        assert np.max(np.abs(ut[i][:, 0])) > 0
        for got, ref in ((uw[i], ur[i]), (dw[i], dr[i])):
            scale = float(np.max(np.abs(ref[:, 0])))
            e = float(np.max(np.abs(got.astype(np.float64) - ref))) / scale
            print("MS-TH f32 %s level %d: %.2e" % (pol, levels[i], e))
            assert e <= 2e-3, (levels[i], e)


# ---- the kernel on random inputs -------------------------------------------------------------------------------------------------
def _kernel_setup(vsm, N, FT, nV, vza_max=80.0):
    H = vsm.host_model
    pol = H.polarization_type("IQU" if N % 3 == 0 else "I")
    qp = types.SimpleNamespace(qp_mu=np.linspace(1.0, 0.05, N // pol.n))      # (the rows of the viewing angles)
    vza, vaz = list(np.linspace(0.0, vza_max, nV)), list(np.linspace(0.0, 345.0, nV))
    dt = torch.float64 if FT == np.float64 else torch.float32
    dev = torch.device("cuda", 0)
    lay = lambda X: torch.tensor(np.ascontiguousarray(X.transpose(0, 2, 1)), dtype=dt, device=dev)
    vec = lambda x: torch.tensor(x, dtype=dt, device=dev)
    return pol, qp, vza, vaz, dt, dev, lay, vec


def _outputs(S, N, pol, nV, dt, dev):
    uw = torch.full((S, pol.n, nV), 0.25, dtype=dt, device=dev)      # accumulated into
    dw = torch.full_like(uw, -0.5)
    return uw, dw, torch.empty((S, N), dtype=dt, device=dev), torch.empty((S, N), dtype=dt, device=dev)


def _src_inputs(N, S, rng, shared, inputs=contractive, scales=(1.0, 1.0), FT=None):
    """(A, [a_k], B, [c_k]): the pair of inputs(N, S, rng, shared) times scales[0] and one further random pair per further scale.
    FT: the sources rounded to FT (a reference computed from them then sees what the device sees)."""
    A, a, B, c = inputs(N, S, rng, shared)
    tops, bots = [a * scales[0]], [c * scales[0]]
    for sc in scales[1:]:
        a2, c2 = rng.random((S, N)), rng.random((S, N))
        tops.append(a2 * sc)
        bots.append(c2 * sc)
    if FT is not None:
        tops, bots = ([np.asarray(x, dtype=FT).astype(np.float64) for x in xs] for xs in (tops, bots))
    return A, tops, B, bots


def _level_src_call(vsm, setup, S, N, nV, tA, tops, tB, bots, oplevel=False):
    """One vsm_level_radiance_src_* call (or its operator-level twin) on device operands: [uw, dw, uw_full, dw_full] on the host."""
    pol, qp, vza, vaz, dt, dev, lay, vec = setup
    out = _outputs(S, N, pol, nV, dt, dev)
    vsm.core_rt_ms.level_radiance_src_(pol, qp, vza, vaz, 1, 1.0 / math.pi, tA, tops, tB, bots, out[0], out[1], out[3], out[2],
                                       oplevel=oplevel)
    torch.cuda.synchronize()
    return [x.cpu().numpy().astype(np.float64) for x in out]


@pytest.mark.parametrize("N", [3, 16, 61, 128])
@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_src_kernel(vsm, N, FT):
    """n_src = 1: the bits of vsm_level_radiance_* -- which for N <= 128 launches this kernel with one source, so the comparison
    now pins the forwarding (arguments, LDS size, the path above 64 viewing angles), not two bodies; the arithmetic of the one
    body is pinned against numpy below (n_src = 2), by test_gpu_multisensor.py::test_level_kernel_fused_vs_oplevel and by
    test_gpu_level_pivoting.py::test_level_radiance_pivoting / test_level_src_pivoting.  n_src = 2: two accumulated
    operator-level calls, within the tolerance of test_gpu_multisensor.py::_fused_vs_oplevel.  Shared and per-point bottoms, 3
    and 70 viewing angles."""
    MSd = vsm.core_rt_ms
    S = 7
    rng = np.random.default_rng(N)
    tol = 1e-12 if FT == np.float64 else 2e-5
    host = lambda xs: [x.cpu().numpy().astype(np.float64) for x in xs]
    for nV in (3, 70):
        setup = _kernel_setup(vsm, N, FT, nV)
        pol, qp, vza, vaz, dt, dev, lay, vec = setup
        for shared in (False, True):
            A, (a, a2), B, (c, c2) = _src_inputs(N, S, rng, shared)
            tA, tB, ta, tc, ta2, tc2 = lay(A), lay(B), vec(a), vec(c), vec(a2), vec(c2)
            w = 1.0 / math.pi
            # n_src = 1 against the one-source entry point
            one = _outputs(S, N, pol, nV, dt, dev)
            MSd.level_radiance_(pol, qp, vza, vaz, 1, w, tA, ta, tB, tc, one[0], one[1], one[3], one[2])
            src1 = _outputs(S, N, pol, nV, dt, dev)
            MSd.level_radiance_src_(pol, qp, vza, vaz, 1, w, tA, [ta], tB, [tc], src1[0], src1[1], src1[3], src1[2])
            torch.cuda.synchronize()
            for x, y in zip(host(one), host(src1)):
                assert np.array_equal(x, y), (N, nV, shared)
            # without the full vectors: the same VZA rows
            src1n = _outputs(S, N, pol, nV, dt, dev)
            MSd.level_radiance_src_(pol, qp, vza, vaz, 1, w, tA, [ta], tB, [tc], src1n[0], src1n[1])
            torch.cuda.synchronize()
            assert np.array_equal(host(src1n[:2])[0], host(one[:2])[0]) and np.array_equal(host(src1n[:2])[1], host(one[:2])[1])
            # n_src = 2 against two accumulated operator-level calls
            src2 = _level_src_call(vsm, setup, S, N, nV, tA, [ta, ta2], tB, [tc, tc2])
            op2 = _level_src_call(vsm, setup, S, N, nV, tA, [ta, ta2], tB, [tc, tc2], oplevel=True)
            vsm._lib.check_device_status("level src kernel")
            for xf, xo in zip(src2, op2):
                assert np.max(np.abs(xf - xo)) <= tol * np.max(np.abs(xo)), (N, nV, shared)
            # ... and the level vectors against numpy: the equation is linear in (a, c)
            uwr, dwr = MS.level_push_through(np.float64, A, a + a2, B.astype(np.float64), c + c2)
            assert np.max(np.abs(src2[2] - uwr)) <= 10 * tol * np.max(np.abs(uwr))
            assert np.max(np.abs(src2[3] - dwr)) <= 10 * tol * np.max(np.abs(dwr))


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_src", [0, 5])
def test_level_src_kernel_refuses_bad_source_counts(vsm, FT, n_src):
    """n_src outside 1..VSM_LEVEL_MAX_SRC is an argument error of the entry point: nothing is launched, the outputs stay."""
    CR, MSd = vsm.CoreRT, vsm.core_rt_ms
    assert MSd.LEVEL_MAX_SRC == 4
    N, S, nV = 16, 3, 3
    pol, qp, vza, vaz, dt, dev, lay, vec = _kernel_setup(vsm, N, FT, nV)
    A, a, B, c = contractive(N, S, np.random.default_rng(0), False)
    tA, tB, ta, tc = lay(A), lay(B), vec(a), vec(c)
    uw, dw, _, _ = _outputs(S, N, pol, nV, dt, dev)
    row0, w = CR._vza_rows_weights(pol, vza, vaz, qp, 1, 1.0, dt)
    ptrs = (C.c_void_p * 5)(*[CR._ptr(ta)] * 5)
    ptrc = (C.c_void_p * 5)(*[CR._ptr(tc)] * 5)
    fn = getattr(vsm._lib.lib(), "vsm_level_radiance_src_" + ("f64" if FT == np.float64 else "f32"))
    args = lambda k: (N, pol.n, S, nV, row0, w, CR._ptr(tA), k, ptrs, CR._ptr(tB), N * N, ptrc, CR._ptr(uw), CR._ptr(dw), None, None,
                      None, CR._stream_ptr())
    assert fn(*args(n_src)) != 0
    assert b"n_src" in vsm._lib.lib().vsm_last_error()
    torch.cuda.synchronize()
    assert torch.all(uw == 0.25) and torch.all(dw == -0.5)
    assert fn(*args(4)) == 0                                   # the largest count the kernel takes
    torch.cuda.synchronize()
    vsm._lib.check_device_status("level src kernel")
    assert torch.all(torch.isfinite(uw)) and not torch.all(uw == 0.25)
    if n_src == 5:
        with pytest.raises(vsm.VSMError, match="n_src"):
            MSd.level_radiance_src_(pol, qp, vza, vaz, 1, 1.0, tA, [ta] * 5, tB, [tc] * 5, uw, dw)
    else:
        with pytest.raises(vsm.VSMError):
            MSd.level_radiance_src_(pol, qp, vza, vaz, 1, 1.0, tA, [], tB, [], uw, dw)


# ---- flags, work buffers, call counts ----------------------------------------------------------------------------------------------
def test_thermal_flag_without_a_thermal_source_changes_nothing(vsm, arch):
    pm, _ = _pair(vsm, arch, "IQU", 17, 6, 7, np.random.default_rng(2), m_max=3)
    levels = [0, 2, 5, 7]
    a = vsm.CoreRT.rt_run_multisensor(pm, levels)
    b = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=True)
    pm.sources = (vsm.host_model.SolarBeam(),)
    c = vsm.CoreRT.rt_run_multisensor(pm, levels, thermal=True)
    for x, y, z in zip(a[0] + a[1], b[0] + b[1], c[0] + c[1]):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_streams_are_the_summed_level_vectors(vsm, arch):
    """streams=True: the m = 0 level vectors are the sum of the solar and the thermal slot (the oracle's), and the VZA outputs
    are their rows, weighted."""
    CR = vsm.CoreRT
    S, L = 4, 6
    pm, om = _pair(vsm, arch, "IQU", 13, S, L, np.random.default_rng(3), m_max=0)
    B = 0.05 + 0.1 * np.random.default_rng(4).random((L, S))
    pm.sources = _sources(vsm, B, True)
    levels = [0, 2, 4, 6]
    res = CR.rt_run_multisensor(pm, levels, streams=True, thermal=True)
    uw, dw = CR.rt_run_multisensor(pm, levels, thermal=True)
    assert res.levels == levels and res.weight == [0.5 / math.pi]
    fs, ft = {}, {}
    MS.ms_reference(om, levels, full=fs)
    MT.ms_thermal_reference(om, B, levels, full=ft)
    n, nV = om.pol.n, len(om.vza)
    row0, w = CR._vza_rows_weights(pm.polarization_type, pm.vza, pm.vaz, pm.quad_points, 0, 0.5 / math.pi, torch.float64)
    for i, l in enumerate(levels):
        assert np.array_equal(res.uw[i], uw[i]) and np.array_equal(res.dw[i], dw[i])
        for got, k in ((res.uw_streams[i][0][:, 0, :].T, 0), (res.dw_streams[i][0][:, 0, :].T, 1)):
            ref = fs[(l, 0)][k] + ft[(l, 0)][k]
            assert np.max(np.abs(ft[(l, 0)][k])) > 0 or (k == 0 and l == L and om.albedo == 0)
            assert np.max(np.abs(got - ref)) <= 1e-9 * np.max(np.abs(ref)), (l, k)
            out = (res.uw, res.dw)[k][i]
            for v in range(nV):
                for c in range(n):
                    np.testing.assert_allclose(out[v, c, :], w[v + nV * c] * got[:, row0[v] + c], rtol=1e-13, atol=1e-16)


def test_outputs_finite_with_poisoned_work(vsm, arch, monkeypatch):
    """VSM_POISON_WORK fills every work buffer with NaN: a thermal bottom or level call reading unwritten scratch shows here."""
    monkeypatch.setenv("VSM_POISON_WORK", "1")
    pm, _ = _pair(vsm, arch, "IQU", 35, 16, 10, np.random.default_rng(9), aerosols=True)
    pm.sources = _sources(vsm, 0.05 + 0.1 * np.random.default_rng(10).random((10, 16)), True)
    uw, dw = vsm.CoreRT.rt_run_multisensor(pm, [0, 3, 7, 10], thermal=True)
    for x in uw + dw:
        assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0


def test_thermal_layer_steps_interactions_and_level_calls(vsm, arch, monkeypatch):
    """What the thermal slot adds to the library calls of a run, for m = 0 only: Nz + (Nz - l_1) layer steps, K + 1 interactions
    (K interior levels) and no level call -- the level calls of m = 0 become ONE vsm_level_radiance_src call each."""
    lib = vsm._lib
    counts = collections.Counter()
    call = lib.call

    def counting(name, *args):
        counts[name] += 1
        return call(name, *args)
    monkeypatch.setattr(lib, "call", counting)
    Nz, levels = 12, [0, 4, 9, 12]
    K, l1, below = 2, 4, 3                               # interior levels, the first of them, levels >= 1
    steps = lambda c: c["vsm_layer_forward_thermal"] + c["vsm_thermal_source"]
    for pol, lt, fused in (("IQU", 31, True), ("IQUV", 50, False)):      # N = 60: the fused slot step; N = 120: operator level
        pm, _ = _pair(vsm, arch, pol, lt, 8, Nz, np.random.default_rng(1), m_max=3)
        nm = pm.m_max + 1
        got = {}
        for tag, lv, th in (("solar", levels, False), ("toa", [0], True), ("all", levels, True)):
            pm.sources = _sources(vsm, np.full((Nz, 8), 0.1), True) if th else None
            counts.clear()
            vsm.CoreRT.rt_run_multisensor(pm, lv, thermal=True)
            got[tag] = collections.Counter(counts)
        N = pm.quad_points.Nquad * pm.polarization_type.n
        assert bool(lib.lib().vsm_layer_thermal_fused(N, 1)) == fused
        assert steps(got["solar"]) == 0 and got["solar"]["vsm_level_radiance_src"] == 0
        assert got["solar"]["vsm_level_radiance"] == below * nm
        assert steps(got["toa"]) == Nz and steps(got["all"]) == Nz + (Nz - l1), (pol, got)
        assert got["all"]["vsm_level_radiance_src"] == below and got["all"]["vsm_level_radiance"] == below * (nm - 1), (pol, got)
        assert got["all"]["vsm_level_radiance_oplevel"] == 0
        # the solar pass is unchanged: what differs are the slot's own calls
        diff = {k: got["all"][k] - got["solar"][k] for k in set(got["all"]) | set(got["solar"]) if got["all"][k] != got["solar"][k]}
        solar_names = [k for k in diff if k.startswith(("vsm_run_", "vsm_layer_forward")) and k != "vsm_layer_forward_thermal"]
        assert not solar_names and "vsm_interaction" not in diff, (pol, diff)
        added = got["all"]["vsm_interaction_oplevel"] - got["solar"]["vsm_interaction_oplevel"]
        if fused:       # every slot step is one launch: the interactions left are the K bottoms and the level-0 surface step
            assert added == K + 1, (pol, got)
        else:           # an operator-level step carries its own interaction, except the first of each of the K + 1 ranges (a copy)
            assert added == (K + 1) + (steps(got["all"]) - (K + 1)), (pol, got)
