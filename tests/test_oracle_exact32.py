"""O.exact_model: a model's decisions taken in its own float type, its arithmetic in FP64 -- the exact reference of a Float32
model's algorithm (tests/test_gpu_fp32_accuracy.py measures the FP32 kernels against it)."""
import numpy as np
import pytest

from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL


def _comp_err(x, ref):
    """Per Stokes component: max |x_k - ref_k| / max |ref_k| (absolute on I's scale where ref_k is zero)."""
    sI = np.max(np.abs(ref[:, 0]))
    return np.array([np.max(np.abs(x[:, k] - ref[:, k])) / (np.max(np.abs(ref[:, k])) if np.max(np.abs(ref[:, k])) > 1e-12 * sI else sI)
                     for k in range(ref.shape[1])])


def _trace(model):
    tr = []
    R, T = O.rt_run(model, trace=tr)
    return R, T, [(t["ndoubl"], t["iface"]) for t in tr], [t["scatter"] for t in tr]


GEO = ("IQU", 35, 50.0, [0.0, 60.0], [30.0, 120.0])
STRIP_ABS = np.array([[1e-3, 1e-4, 1e-5], [0.5, 0.2, 0.1], [5.0, 1.0, 3.0], [0.0, 0.0, 0.0], [1e-2, 30.0, 1e-2]])


def test_default_and_float64_decisions_are_bit_identical():
    """decide_FT unset or float64 on an FP64 model, and decide_FT = float32 set explicitly on a Float32 model: the bits of the
    plain run (rt_run, rt_run_thermal, rt_run_lin)."""
    kw = dict(tau_rayl=np.tile([0.05, 0.0, 0.5], (3, 1)), tau_abs=STRIP_ABS[:3], depol=0.03, albedo=0.3, m_max=2)
    B = 0.1 + 0.01 * np.arange(9).reshape(3, 3)
    for FT in (np.float64, np.float32):
        a = O.build_model(*GEO, FT=FT, **kw)
        b = O.build_model(*GEO, FT=FT, **kw)
        b.decide_FT = FT
        for fa, fb in ((O.rt_run(a), O.rt_run(b)), (O.rt_run_thermal(a, B), O.rt_run_thermal(b, B))):
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(fa, fb))
    kw = dict(kw, tau_rayl=np.tile([0.05, 0.1, 0.5], (3, 1)))
    lin = OL.LinModel([kw["tau_abs"]])
    a = O.build_model("IQU", 9, 40.0, [30.0], [0.0], **kw)
    b = O.build_model("IQU", 9, 40.0, [30.0], [0.0], **kw)
    b.decide_FT = np.float64
    assert all(np.array_equal(x, y) for x, y in zip(OL.rt_run_lin(a, lin), OL.rt_run_lin(b, lin)))


def test_exact_model_keeps_the_float32_inputs_of_the_algorithm():
    om32 = O.build_model(*GEO, tau_rayl=[[0.1]], FT=np.float32)
    ex = O.exact_model(om32)
    assert ex.FT == np.float64 and ex.decide_FT == np.float32 and om32.decide_FT is None
    q, qx = om32.quad_points, ex.quad_points
    for a, b in ((q.qp_mu, qx.qp_mu), (q.wt_mu, qx.wt_mu), (q.qp_muN, qx.qp_muN), (q.wt_muN, qx.wt_muN)):
        assert b.dtype == np.float64 and np.array_equal(b, a.astype(np.float64))
    assert qx.mu0 == q.mu0 == float(np.float32(O.cosd(50.0)))
    q64 = O.build_model(*GEO, tau_rayl=[[0.1]]).quad_points
    assert not np.array_equal(qx.qp_mu, q64.qp_mu)             # not the FP64 nodes


# Float32 scenes: the 1024 eps(Float32) floor deciding ndoubl, a thick near-conservative column, a non-scattering layer in the
# middle, layers too thin to double
SCENES = {
    "floor": (GEO, dict(tau_rayl=np.tile([2e-4, 5e-4, 0.05], (3, 1)), tau_abs=STRIP_ABS[:3], depol=0.03, albedo=0.2, m_max=2)),
    "thick": (("IQU", 57, 50.0, [0.0, 60.0], [30.0, 120.0]),
              dict(tau_rayl=np.tile([1.0, 3.0], (2, 1)), tau_abs=np.array([[0.0, 0.0], [1e-4, 1e-5]]), depol=0.03, albedo=0.9,
                   m_max=2)),
    "noscat": (("IQUV", 41, 35.0, [20.0, 0.0], [0.0, 100.0]),
               dict(tau_rayl=np.tile([0.05, 0.1, 0.0, 0.2], (3, 1)), tau_abs=np.tile([0.01, 0.2, 0.3, 0.05], (3, 1)), depol=0.03,
                    albedo=0.3, m_max=2)),
    "nodoubl": (("IQU", 19, 35.0, [20.0, 0.0], [0.0, 100.0]),
                dict(tau_rayl=np.tile([1e-6, 0.05, 5e-7, 0.1, 8e-7], (3, 1)), tau_abs=np.tile([1e-8, 0.02, 1e-9, 0.3, 1e-8], (3, 1)),
                     depol=0.03, albedo=0.3, m_max=2)),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_exact_reference_takes_the_float32_decisions(name):
    geo, kw = SCENES[name]
    om32 = O.build_model(*geo, FT=np.float32, **kw)
    R32, T32, t32, s32 = _trace(om32)
    Rx, Tx, tx, sx = _trace(O.exact_model(om32))
    _, _, t64, _ = _trace(O.build_model(*geo, **kw))
    assert tx == t32 and sx == s32
    nd32, nd64 = [t[0] for t in t32], [t[0] for t in t64]
    if name == "floor":                          # the FP32 floor (1.2e-4) lies above 0.001 mu_min: fewer doublings than FP64
        assert all(a <= b for a, b in zip(nd32, nd64)) and any(a < b for a, b in zip(nd32, nd64))
    if name == "thick":
        assert max(nd32) >= 15
    if name == "noscat":
        assert s32[:4] == [True, True, False, True]
    if name == "nodoubl":
        assert nd32[:5].count(0) == 3
    for a, b in ((R32, Rx), (T32, Tx)):          # rounding apart: single precision is within its own accumulation of it
        assert np.max(_comp_err(a, b)) < 2e-3


# The two scenes of the FP32 strip-kernel test geometry: per Stokes component, the FP32 oracle lies closer to the exact
# reference than the FP64 oracle, whose ndoubl and nodes differ (measured: thick N = 93, FP32 R 2.6e-4 .. 3.5e-4,
# T 1.9e-4 .. 6.2e-4; FP64 R 7e-4 .. 2.6e-3, T 6.6e-4 .. 6.6e-3.  Thin N = 63: FP32 R 4.8e-5 .. 8.3e-5, T 6.4e-5 .. 1.9e-4;
# FP64 R 3.2e-4 .. 6.7e-4, T 2.3e-4 .. 8.1e-4)
TABLE = {
    "thick": (("IQU", 57, 50.0, [0.0, 60.0], [30.0, 120.0]), [[0.05, 0.5, 1.0]] * 5, 0.6, 1e-3, 2e-2),
    "thin": (GEO, [[0.02, 0.03, 0.05]] * 5, 0.2, 4e-4, 2e-3),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_float32_oracle_is_closer_to_the_exact_reference_than_fp64(name):
    geo, rayl, albedo, cap32, cap64 = TABLE[name]
    kw = dict(tau_rayl=np.array(rayl), tau_abs=STRIP_ABS, depol=0.03, albedo=albedo, m_max=3)
    om32 = O.build_model(*geo, FT=np.float32, **kw)
    R32, T32 = O.rt_run(om32)
    R64, T64 = O.rt_run(O.build_model(*geo, **kw))
    Rx, Tx = O.rt_run(O.exact_model(om32))
    for a32, a64, ax in ((R32, R64, Rx), (T32, T64, Tx)):
        e32, e64 = _comp_err(a32, ax), _comp_err(a64, ax)
        assert np.all(e32 < e64), (e32, e64)
        assert e32.max() < cap32 and e64.max() < cap64, (e32, e64)
        assert e64.max() > 3 * e32.max()


def test_float32_linearized_oracle_is_closer_to_its_exact_reference():
    """OL.rt_run_lin of the exact model (elemental_lin's active mask and ndoubl decided in single): the FP32 linearized oracle lies
    closer to it than the FP64 linearized oracle, in R, T and every Jacobian column."""
    rng = np.random.default_rng(0)
    S, L = 3, 3
    ga, gb = 10.0 ** rng.uniform(-2.5, -0.5, (S, L)), 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    kw = dict(tau_rayl=np.tile(0.03 * np.ones(L), (S, 1)), tau_abs=ga + gb, depol=0.0279, albedo=0.2, m_max=2)
    geo = ("IQU", 31, 40.0, [30.0, 5.0], [0.0, 60.0])
    lin = OL.LinModel([ga, gb])
    om32 = O.build_model(*geo, FT=np.float32, **kw)
    o32 = OL.rt_run_lin(om32, lin)
    o64 = OL.rt_run_lin(O.build_model(*geo, **kw), lin)
    ox = OL.rt_run_lin(O.exact_model(om32), lin)
    for i in range(4):
        cols = [(o32[i], o64[i], ox[i])] if i < 2 else [(o32[i][..., p], o64[i][..., p], ox[i][..., p]) for p in range(3)]
        for a32, a64, ax in cols:
            e32, e64 = _comp_err(a32, ax), _comp_err(a64, ax)
            assert e32.max() < e64.max(), (i, e32, e64)
