"""The doubling loop of the FP64 native layer kernels (ned_body, csrc/vsm_native.hip) at the smallest shapes that reach each of its
paths, rt_run on three spectral points against the numpy oracle at the gates of tests/test_gpu_native.py (1e-8; T of the thick
stack 1e-7):

  * rider columns (the source vectors ride in the spare columns c1 = 4 KS, c1 + 1 of the strips and change places at the end of a
    step through a DPP move restricted to one 4-lane bank): one block per row-tile count RT and per bank (c1 & 15) >> 2;
  * ndoubl = 0, 1, 2, 3, 8 per block, forced through the layers' optical depth: no step at all (the riders never leave the
    vectors), odd and even counts, the last step (no store back), thin layers whose every inverse is the order-1 series
    (no barrier in front of the [tt] store);
  * a thick near-conservative stack: later steps take the Horner orders >= 2 (that barrier is kept), the long series and the
    pivoted inverse out of line (both use the A-form as scratch);
  * a block without spare columns (the mat-vec source path);
  * the zero-weight tail on and off (KZ < KS instantiations)."""
from functools import lru_cache

import numpy as np
import pytest

from oracle import vsm_oracle as O

SZA, VZA, VAZ = 40.0, [30.0], [0.0]
S = 3
# (pol, l_trunc) -> the blocks the native run walks: rows n, row tiles RT, k-steps KS, DPP bank of the rider columns (None: mat-vec path)
SHAPES = {
    ("I", 6): [(6, 1, 2, 2)],
    ("I", 34): [(20, 2, 5, 1)],
    ("I", 50): [(28, 2, 7, 3)],
    ("IQU", 35): [(40, 3, 10, 2), (60, 4, 15, 3)],      # m = 0: the (I,Q) block of 40 rows; m = 1, 2: dense
    ("I", 26): [(16, 1, 4, None)],
}
NDOUBL = (0, 1, 2, 3, 8)
THICK = (0.5, 4.0, 30.0)


def _geometry(n):
    ks = (n + 3) // 4
    rt = ks // 4 if ks % 4 == 0 else (4 * ks + 2 + 15) // 16
    bank = None if ks % 4 == 0 else ((4 * ks) & 15) >> 2
    return rt, ks, bank


def _mu_min(pol, l_trunc):
    q = O.rt_set_streams_gausslegquad(l_trunc, SZA, VZA, O.polarization(pol), np.float64)
    return float(np.min(q.qp_mu[q.wt_mu > np.finfo(np.float64).eps]))


def _scene_kw(pol, l_trunc, kind):
    """kind = an int: two layers that both take that many doubling steps (rt_kernel.jl:266-287: dtau_max = 0.001 mu_min, ndoubl =
    ceil(log2(tau varpi / dtau_max)); the layers sit half an octave inside their band), no surface reflection -- R and T are the
    layers' own scattering, so the gate is relative to what the doubling produced.  kind = "thick": the stack of
    test_native_run_thick_layers_series_orders_and_pivoted_inverse."""
    rng = np.random.default_rng(41)
    if kind == "thick":
        tau_rayl = np.tile(np.array(THICK), (S, 1))
        tau_abs = np.tile(np.array([1e-4, 1e-5, 1e-6]), (S, 1)) * (1 + rng.random((S, 1)))
        return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.03, albedo=0.6, m_max=2)
    dmax = 0.001 * _mu_min(pol, l_trunc)
    t = dmax * (0.5 if kind == 0 else 2.0 ** (kind - 0.5))
    tau_rayl = np.tile(np.array([t, 0.8 * t]), (S, 1))
    tau_abs = tau_rayl * rng.uniform(0.0, 0.5, (S, 2))
    return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.03, albedo=0.0, m_max=2)


def _beam(pol):
    ns = O.polarization(pol).n
    rng = np.random.default_rng(43)
    F0 = np.zeros((ns, S))
    F0[0] = 1.0 + 0.1 * rng.random(S)
    if ns >= 3:
        F0[1], F0[2] = 0.05 * rng.standard_normal(S), 0.04 * rng.standard_normal(S)      # a polarized beam drives the U rows
    return F0


@lru_cache(maxsize=None)
def _oracle(pol, l_trunc, kind):
    om = O.build_model(pol, l_trunc, SZA, VZA, VAZ, **_scene_kw(pol, l_trunc, kind))
    om.F0 = _beam(pol)
    R, T = O.rt_run(om)
    R.setflags(write=False)
    T.setflags(write=False)
    return R, T


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def test_shapes_reach_the_blocks_they_name():
    """The table above against the quadrature and the launcher's geometry (vsm_native.hip: KS = ceil(n / 4), RT = KS / 4 without
    spare columns, else ceil((4 KS + 2) / 16)); every row-tile count 1..4 and every bank 1..3 occurs; the ndoubl scenes land on
    their counts by the rule of rt_kernel.jl:266-287 (oracle: doubling_number)."""
    seen = set()
    for (pol, l_trunc), blocks in SHAPES.items():
        pt = O.polarization(pol)
        q = O.rt_set_streams_gausslegquad(l_trunc, SZA, VZA, pt, np.float64)
        nquad = q.Nquad
        sizes = {nquad * pt.n} | ({nquad * 2} if pt.n >= 3 else set())
        for n, rt, ks, bank in blocks:
            assert n in sizes, (pol, l_trunc, n, sizes)
            assert _geometry(n) == (rt, ks, bank), (n, _geometry(n))
            seen.add((rt, bank))
        assert int(np.count_nonzero(q.wt_mu == 0.0)) == 2               # the VZA and the SZA stream: the zero-weight tail
        for nd in NDOUBL:                                               # (tau varpi of a layer = its tau_rayl: varpi_Cabannes = 1)
            kw = _scene_kw(pol, l_trunc, nd)
            for iz in range(2):
                tau = kw["tau_rayl"][:, iz] + kw["tau_abs"][:, iz]
                assert O.get_dtau_ndoubl(tau, kw["tau_rayl"][:, iz] / tau, q, np.float64)[1] == nd, (pol, l_trunc, nd, iz)
    assert {rt for rt, b in seen if b is not None} == {1, 2, 3, 4} and {b for _, b in seen} == {1, 2, 3, None}
    assert (2, 1) in seen and (2, 3) in seen and (1, 2) in seen and (3, 2) in seen and (4, 3) in seen


gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    pytest.importorskip("torch")
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _run(vsm, arch, monkeypatch, pol, l_trunc, kind, zw):
    import torch
    model = vsm.host_model.model_from_arrays(arch, pol, l_trunc, SZA, VZA, VAZ, **_scene_kw(pol, l_trunc, kind))
    model.F0 = _beam(pol)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_RUN", True)
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_ZW_TAIL", zw)
    sc = vsm.CoreRT.prepare_scene(model)
    assert sc._native_moments() == {0, 1, 2}, sc._native_moments()
    sc.run()
    torch.cuda.synchronize()
    vsm._lib.check_device_status("doubling chain")
    R, T = sc.results_host()
    return sc, np.asarray(R), np.asarray(T)


@gpu
@pytest.mark.parametrize("zw", [True, False], ids=["tail", "dense"])
@pytest.mark.parametrize("nd", NDOUBL)
@pytest.mark.parametrize("pol,l_trunc", list(SHAPES))
def test_doubling_steps_by_count(vsm, arch, monkeypatch, pol, l_trunc, nd, zw):
    """Two thin layers of nd doubling steps each (every inverse of the first steps is the order-1 series), per block shape."""
    sc, R, T = _run(vsm, arch, monkeypatch, pol, l_trunc, nd, zw)
    assert [ly["nd"] for ly in sc.moments[0]["layers"]] == [nd, nd]
    Ro, To = _oracle(pol, l_trunc, nd)
    eR, eT = _rel(R, Ro), _rel(T, To)
    print("doubling chain %s l_trunc %d ndoubl %d zw %s: rel R %.3e T %.3e" % (pol, l_trunc, nd, zw, eR, eT))
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(T))
    assert eR < 1e-8 and eT < 1e-8, (eR, eT)


@gpu
@pytest.mark.parametrize("zw", [True, False], ids=["tail", "dense"])
@pytest.mark.parametrize("pol,l_trunc", list(SHAPES))
def test_doubling_steps_thick_stack(vsm, arch, monkeypatch, pol, l_trunc, zw):
    """Thick near-conservative layers over a bright surface: the late steps leave order 1 for the Horner orders, the long series and
    the pivoted inverse (counted in vsm_device_status; no flag raised)."""
    sc, R, T = _run(vsm, arch, monkeypatch, pol, l_trunc, "thick", zw)
    nds = [ly["nd"] for ly in sc.moments[0]["layers"]]
    assert min(nds) >= 9 and nds == sorted(nds), nds
    st = list(vsm._lib.last_device_status)
    assert st[0] == 0, st
    Ro, To = _oracle(pol, l_trunc, "thick")
    eR, eT = _rel(R, Ro), _rel(T, To)
    print("doubling chain %s l_trunc %d thick zw %s: ndoubl %s pivoted %d rel R %.3e T %.3e" % (pol, l_trunc, zw, nds, st[1], eR, eT))
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(T))
    assert eR < 1e-8 and eT < 1e-7, (eR, eT)    # (T: e^-34 of the beam, as in test_gpu_native.py)
