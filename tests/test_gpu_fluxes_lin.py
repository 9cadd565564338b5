"""GPU tests of the linearized flux run (vsm.CoreRTLin.rt_run_fluxes, core_rt_flux_lin.py) and its level kernel
(vsm_level_flux_lin_*, csrc/vsm_level.hip): the kernel against a numpy float64 composition of the same inputs and against the
float64 quadrature of vsm_level_radiance_lin_src_*'s own derivative vectors, its argument errors and its determinism; the driver
against the float64 oracle (tests/flux_lin_oracle.py), against the quadrature of CoreRTLin.rt_run_multisensor(streams=True)'s own
m = 0 vectors, against CoreRT.rt_run_fluxes, with thermal emission and Planck slots, Float32, blocks of the spectral axis, the
level calls the host issues and the refusals.

Kernel bounds.  Against numpy: what tests/test_gpu_multisensor_lin.py allows vsm_level_radiance_lin_* for its derivative vectors,
1e-11 (FP64) / 2e-4 (FP32) of the largest reference value -- a quadrature with positive weights of order one does not amplify a
vector's error.  Against the kernel's own vectors (vsm_level_radiance_lin_src_* with full outputs) reduced in float64, element by
element: (N / n_stokes + 2) eps sum_i |q_i v_i|, the classical bound of a sum of N / n_stokes products in any order plus the
rounding of the stored result.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import flux_lin_oracle as FL  # noqa: E402
import ms_lin_oracle as MSL  # noqa: E402
import ms_thermal_lin_oracle as MTL  # noqa: E402
from level_cases import contractive  # noqa: E402
from test_gpu_multisensor_lin import _idx, _pair, _sub  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("up", "down_diffuse", "down_direct", "actinic_up", "actinic_down_diffuse", "actinic_direct", "net_down")
INVALID = 1          # VSM_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


# ---- the kernel on random inputs -------------------------------------------------------------------------------------------------
class _Case:
    """One set of inputs on the host (float64 values exact in FT) and on the device, with the float64 reference vectors."""

    def __init__(self, N, P, P_top, P_src, shared, S, FT, ns, seed=0):
        rng = np.random.default_rng(seed + N + 7 * P + 3 * P_src)
        rnd = lambda x: np.asarray(x, dtype=FT).astype(np.float64)
        self.N, self.P, self.P_top, self.P_src, self.S, self.FT, self.ns, self.shared = N, P, P_top, P_src, S, FT, ns, shared
        A, a, B, c = (rnd(x) for x in contractive(N, S, rng, shared))
        Ad, ad = rnd(rng.normal(0, 1, (P_top, S, N, N)) / N), rnd(rng.normal(0, 1, (P_top, S, N)))
        Bd, cd = rnd(rng.normal(0, 1, (P,) + B.shape) / N), rnd(rng.normal(0, 1, (P, S, N)))
        asrc, csrc = rnd(rng.normal(0, 1, (P_src, S, N))), rnd(rng.normal(0, 1, (P_src, S, N)))
        Adz = np.concatenate([Ad, np.zeros((P - P_top, S, N, N))])
        adz = np.concatenate([ad, np.zeros((P - P_top, S, N))])
        uw, dw, uwd, dwd = MSL.level_lin_push_through(np.float64, A, a, B, c, Adz, adz, Bd, cd)
        if P_src:
            us, ds = MTL.level_src_only(np.float64, A, B, asrc, csrc)
            uwd, dwd = np.concatenate([uwd, us]), np.concatenate([dwd, ds])
        self.uw, self.dw = rnd(uw), rnd(dw)          # (the elastic vectors are inputs of the call: what the device sees)
        self.uwd, self.dwd = uwd, dwd
        self.c, self.cd, self.csrc = c, cd, csrc
        Nq = N // ns
        self.q, self.dir_h = rnd(rng.uniform(0.5, 1.5, (4, Nq))), rnd(rng.uniform(0.5, 1.5, 4))
        self.tau, self.F0 = rnd(rng.random(S) * 2), rnd(0.5 + rng.random(S))
        self.tsd = rnd(rng.normal(0, 1, (max(P, 1), S)))
        self.mu0 = float(rnd(0.7))
        dt = torch.float64 if FT == np.float64 else torch.float32
        dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
        sw = lambda M: np.swapaxes(M, -1, -2)                # math order -> the column-major layout
        self.dt = dt
        self.t = dict(A=dev(sw(A)), B=dev(sw(B)), dwf=dev(self.dw), uwf=dev(self.uw), Ad=dev(sw(Ad)), ad=dev(ad), Bd=dev(sw(Bd)),
                      cd=dev(cd), asrc=dev(asrc), csrc=dev(csrc), q=dev(self.q), tau=dev(self.tau), F0=dev(self.F0), tsd=dev(self.tsd),
                      c=dev(c))

    def call(self, vsm, nW, top=True, direct=True, p_layer=None, idx=None, raw=None):
        """One vsm_level_flux_lin_* call into a NaN-filled output; idx: the points (a gathered batch); raw: argument overrides,
        then the return code comes back instead of the output."""
        N, S, P, P_top, P_src, NN = self.N, self.S, self.P, self.P_top, self.P_src, self.N * self.N
        t = self.t
        if idx is not None:
            ix = torch.as_tensor(idx, device="cuda")
            pick = lambda x, ax: x.index_select(ax, ix).contiguous()
            t = dict(t, A=pick(t["A"], 0), B=t["B"] if self.shared else pick(t["B"], 0), dwf=pick(t["dwf"], 0), uwf=pick(t["uwf"], 0),
                     Ad=pick(t["Ad"], 1), ad=pick(t["ad"], 1), Bd=t["Bd"] if self.shared else pick(t["Bd"], 1), cd=pick(t["cd"], 1),
                     asrc=pick(t["asrc"], 1), csrc=pick(t["csrc"], 1), tau=pick(t["tau"], 0), F0=pick(t["F0"], 0),
                     tsd=pick(t["tsd"], 1), c=pick(t["c"], 0))
            S = len(idx)
        p_layer = P_top if p_layer is None else p_layer
        ct = C.c_double if self.FT == np.float64 else C.c_float
        out = torch.full((3, nW, 1 + P + P_src, S), float("nan"), dtype=self.dt, device="cuda")
        p_ = lambda x, on=True: x.data_ptr() if on and x is not None and x.numel() else None
        bstride = 0 if self.shared and S > 1 else NN
        g = dict(N=N, ns=self.ns, S=S, P=P, P_top=P_top, P_src=P_src, A=p_(t["A"], top), B=p_(t["B"], top), bs=bstride,
                 dwf=p_(t["dwf"], top), uwf=p_(t["uwf"] if top else t["c"]), Ad=p_(t["Ad"], top), aps=S * NN, ad=p_(t["ad"], top),
                 Bd=p_(t["Bd"], top), bds=bstride, bps=(1 if self.shared else S) * NN, cd=p_(t["cd"]), asrc=p_(t["asrc"], top),
                 csrc=p_(t["csrc"]), nW=nW, q=p_(t["q"][:nW].contiguous()), dh=(ct * 4)(*self.dir_h), mu0=self.mu0,
                 tau=p_(t["tau"], direct), F0=p_(t["F0"], direct), tsd=p_(t["tsd"], direct), pl=p_layer, out=p_(out))
        g.update(raw or {})
        fn = getattr(vsm._lib.lib(), "vsm_level_flux_lin_" + ("f64" if self.FT == np.float64 else "f32"))
        rc = fn(g["N"], g["ns"], g["S"], g["P"], g["P_top"], g["P_src"], g["A"], g["B"], g["bs"], g["dwf"], g["uwf"], g["Ad"], g["aps"],
                g["ad"], g["Bd"], g["bds"], g["bps"], g["cd"], g["asrc"], g["csrc"], g["nW"], g["q"], g["dh"], ct(g["mu0"]), g["tau"],
                g["F0"], g["tsd"], g["pl"], g["out"], None)
        torch.cuda.synchronize()
        if raw is not None:
            return rc, out
        assert rc == 0, vsm._lib.lib().vsm_last_error()
        return out.double().cpu().numpy()

    def reference(self, nW, top, direct, p_layer, uw=None, dw=None, uwd=None, dwd=None):
        """out [3][nW][1 + P + P_src][S] in float64, from the reference vectors (or the ones given) and the bound of the sums."""
        ns, S = self.ns, self.S
        if top:
            uw, dw = (self.uw, self.dw) if uw is None else (uw, dw)
            uwd, dwd = (self.uwd, self.dwd) if uwd is None else (uwd, dwd)
        else:
            uw, dw = self.c, np.zeros_like(self.c)
            uwd = np.concatenate([self.cd, self.csrc])
            dwd = np.zeros_like(uwd)
        q = self.q[:nW]
        ref, mag = np.zeros((3, nW, 1 + uwd.shape[0], S)), np.zeros((3, nW, 1 + uwd.shape[0], S))
        for d, (v0, vd) in enumerate(((uw, uwd), (dw, dwd))):
            allv = np.concatenate([v0[None], vd])[:, :, ::ns]                 # [1 + Ptot, S, Nq]
            ref[d] = np.einsum("rq,psq->rps", q, allv)
            mag[d] = np.einsum("rq,psq->rps", np.abs(q), np.abs(allv))
        if direct:
            beam = self.dir_h[:nW, None] * (self.F0 * np.exp(-self.tau / self.mu0))[None, :]
            ref[2, :, 0] = beam
            ref[2, :, 1:1 + p_layer] = -beam[:, None, :] * self.tsd[None, :p_layer] / self.mu0
        return ref, mag

    def lin_src_vectors(self, vsm):
        """(uw', dw') (P + P_src, S, N) of vsm_level_radiance_lin_src_* on the same inputs, in float64."""
        N, S, P, P_top, P_src, NN, t = self.N, self.S, self.P, self.P_top, self.P_src, self.N * self.N, self.t
        full = [torch.full((P + P_src, S, N), float("nan"), dtype=self.dt, device="cuda") for _ in range(2)]
        p_ = lambda x: x.data_ptr() if x.numel() else None
        bstride = 0 if self.shared and S > 1 else NN
        vsm._lib.call("vsm_level_radiance_lin_src", self.dt, N, self.ns, S, P, P_top, P_src, 0, None, None, p_(t["A"]), p_(t["B"]), bstride,
                      p_(t["dwf"]), p_(t["uwf"]), p_(t["Ad"]), S * NN, p_(t["ad"]), p_(t["Bd"]), bstride, (1 if self.shared else S) * NN,
                      p_(t["cd"]), p_(t["asrc"]), p_(t["csrc"]), None, None, full[0].data_ptr(), full[1].data_ptr(), None)
        torch.cuda.synchronize()
        return full[1].double().cpu().numpy(), full[0].double().cpu().numpy()


KERNEL_CASES = [
    # N, P, P_top, P_src, nW, shared, ns, S, FT
    (8, 1, 0, 0, 1, False, 1, 3, np.float64),
    (21, 3, 2, 1, 2, True, 3, 5, np.float64),
    (60, 3, 3, 4, 4, False, 3, 4, np.float64),
    (60, 1, 1, 0, 2, True, 4, 3, np.float64),
    (128, 64, 60, 0, 2, True, 4, 3, np.float64),        # six chunks of 12, the last one of 4
    (128, 10, 9, 4, 4, False, 4, 3, np.float64),        # chunk 0 = slots 0..11: ten parameter slots and two source-only ones
    (128, 3, 1, 1, 1, False, 1, 3, np.float64),         # Nq = 128: both strides of a lane
    (8, 3, 2, 1, 2, False, 1, 3, np.float32),
    (21, 1, 1, 0, 1, True, 3, 3, np.float32),
    (60, 3, 2, 4, 4, False, 3, 4, np.float32),
    (128, 64, 60, 0, 2, True, 4, 3, np.float32),
    (128, 10, 9, 4, 2, False, 4, 3, np.float32),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "N%d_P%d_top%d_src%d_nW%d_%s_%s" % (c[:5] + ("shared" if c[5] else "perpoint",
                                                                                                       np.dtype(c[8]).name)))
def test_level_flux_lin_kernel(vsm, case):
    """With a top (with and without the direct term) and without one (the TOA), NaN-filled outputs."""
    N, P, P_top, P_src, nW, shared, ns, S, FT = case
    k = _Case(N, P, P_top, P_src, shared, S, FT, ns)
    eps = float(np.finfo(FT).eps)
    tol = 1e-11 if FT == np.float64 else 2e-4
    dvec = k.lin_src_vectors(vsm)
    vsm._lib.check_device_status("level_radiance_lin_src")
    worst = dict(numpy=0.0, own=0.0)
    for top, direct in ((True, True), (True, False), (False, True), (False, False)):
        p_layer = P_top
        got = k.call(vsm, nW, top, direct, p_layer)
        ref, _ = k.reference(nW, top, direct, p_layer)
        assert np.all(np.isfinite(got)), (case, top, direct)
        for d in (0, 1):
            for sl in (slice(0, 1), slice(1, None)):
                sc = np.abs(ref[d][:, sl]).max()
                e = np.abs(got[d][:, sl] - ref[d][:, sl]).max()
                if sc == 0:
                    assert e == 0
                    continue
                worst["numpy"] = max(worst["numpy"], e / sc)
                assert e <= tol * sc, (case, top, direct, d, e / sc)
        if not top:
            assert np.all(got[1] == 0)
        if direct:
            assert np.abs(got[2] - ref[2]).max() <= 8 * eps * np.abs(ref[2]).max()
            assert np.all(got[2][:, 1 + p_layer:] == 0)
        else:
            assert np.all(got[2] == 0)
        if top:      # the kernel's own vectors, reduced in float64
            own, mag = k.reference(nW, True, direct, p_layer, k.uw, k.dw, *dvec)
            bound = (N // ns + 2) * eps * mag[:2]
            ratio = np.abs(got[:2] - own[:2]) / np.where(bound > 0, bound, 1)
            worst["own"] = max(worst["own"], float(ratio.max()))
            assert np.all(np.abs(got[:2] - own[:2]) <= bound), (case, direct, float(ratio.max()))
    vsm._lib.check_device_status("level_flux_lin")
    print("level_flux_lin %s: vs numpy %.2e of the largest value (bound %.0e); vs its own vectors %.2f of (Nq + 2) eps sum|q v|"
          % (case[:8] + (np.dtype(FT).name,), worst["numpy"], tol, worst["own"]))


def test_level_flux_lin_kernel_is_deterministic_in_place(vsm):
    """The order of the additions is fixed: a point gives the same bits wherever it stands in the batch, and alone."""
    k = _Case(60, 14, 12, 2, False, 7, np.float64, 3, seed=5)
    whole = k.call(vsm, 2)
    perm = [4, 0, 6, 2, 5, 1, 3]
    assert np.array_equal(k.call(vsm, 2, idx=perm), whole[..., perm])
    assert np.array_equal(k.call(vsm, 2, idx=[5]), whole[..., [5]])
    k = _Case(128, 14, 12, 2, True, 4, np.float64, 4, seed=6)          # two chunks, a shared bottom
    whole = k.call(vsm, 2)
    assert np.array_equal(k.call(vsm, 2, idx=[2, 0, 3, 1]), whole[..., [2, 0, 3, 1]])
    assert np.array_equal(k.call(vsm, 2, idx=[3]), whole[..., [3]])


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["f64", "f32"])
def test_level_flux_lin_kernel_refuses_bad_arguments(vsm, FT):
    """Every argument error returns VSM_ERR_INVALID_ARG before any launch (the NaN-filled output stays); S = 0 is no error."""
    k = _Case(16, 3, 2, 2, False, 3, FT, 1)
    bad = [dict(N=129), dict(N=0), dict(ns=3), dict(ns=5), dict(S=-1), dict(P=-1), dict(P=63, P_src=2), dict(P=0, P_src=0, P_top=0),
           dict(P_top=4), dict(P_top=-1), dict(P_src=-1), dict(nW=0), dict(nW=5), dict(bs=7), dict(bds=7), dict(bps=16), dict(aps=16),
           dict(q=None), dict(out=None), dict(uwf=None), dict(dwf=None), dict(B=None), dict(Bd=None), dict(cd=None), dict(Ad=None),
           dict(ad=None), dict(asrc=None), dict(csrc=None), dict(tau=None), dict(F0=None), dict(dh=None), dict(mu0=0.0),
           dict(tsd=None), dict(pl=4), dict(pl=-1)]
    for kw in bad:
        rc, out = k.call(vsm, 2, raw=kw)
        assert rc == INVALID, kw
        assert vsm._lib.lib().vsm_last_error()
        assert bool(torch.all(torch.isnan(out))), kw
    rc, out = k.call(vsm, 2, raw=dict(S=0))
    assert rc == 0 and bool(torch.all(torch.isnan(out)))
    assert k.call(vsm, 2, raw=dict(S=0, q=None, out=None, uwf=None, cd=None))[0] == 0
    # what the TOA and a call without the direct term may leave out
    rc, out = k.call(vsm, 4, raw=dict(A=None, B=None, dwf=None, Ad=None, ad=None, Bd=None, asrc=None, tau=None, F0=None, dh=None,
                                      tsd=None))
    assert rc == 0 and bool(torch.all(torch.isfinite(out)))
    rc, out = k.call(vsm, 2, raw=dict(P_top=0, Ad=None, ad=None, pl=0, tsd=None))
    assert rc == 0 and bool(torch.all(torch.isfinite(out)))
    vsm._lib.check_device_status("level flux lin kernel")


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    sc = float(np.max(np.abs(ref)))
    e = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)))
    return e / sc if sc > 0 else e


def _worst(res, ref, points=None, dots=True):
    """Per field (and per field and slot for the derivatives): max |got - ref| relative to the largest |ref| over levels and points."""
    pick = (lambda x: x) if points is None else (lambda x: x[:, points])
    out = {k: _rel(pick(getattr(res, k)), getattr(ref, k)) for k in FIELDS}
    if dots:
        for k in FIELDS:
            g, r = pick(getattr(res, k + "_dot")), getattr(ref, k + "_dot")
            assert g.shape == r.shape, (k, g.shape, r.shape)
            out[k + "_dot"] = max(_rel(g[..., p], r[..., p]) for p in range(r.shape[-1]))
        if ref.absorbed_dot is not None:
            pk = (lambda x: x) if points is None else (lambda x: x[..., points, :])
            for k in ("absorbed_dot", "surface_absorbed_dot"):
                out[k] = max(float(np.max(np.abs(pk(getattr(res, k))[..., p] - getattr(ref, k)[..., p])))
                             / float(np.max(np.abs(ref.net_down_dot[..., p]))) for p in range(ref.net_down_dot.shape[-1]))
    return out


def _check_level0_and_identities(res, lv):
    for i, l in enumerate(lv):
        j = lv.index(l)                                  # duplicates: the same rows
        assert all(np.array_equal(getattr(res, k + s)[i], getattr(res, k + s)[j]) for k in FIELDS for s in ("", "_dot"))
        if l == 0:
            for k in ("down_diffuse", "actinic_down_diffuse"):
                assert np.all(getattr(res, k)[i] == 0) and np.all(getattr(res, k + "_dot")[i] == 0)
            assert np.all(res.down_direct_dot[i] == 0) and np.all(res.actinic_direct_dot[i] == 0)
    assert np.array_equal(res.net_down, res.down_direct + res.down_diffuse - res.up)
    assert np.array_equal(res.net_down_dot, res.down_direct_dot + res.down_diffuse_dot - res.up_dot)
    for k in FIELDS:
        assert np.all(np.isfinite(getattr(res, k))) and np.all(np.isfinite(getattr(res, k + "_dot")))


CASES = [
    # (id, pol, l_trunc, S, Nz, levels (None: all), sub0, kwargs)
    ("scalar_n8_unsorted_duplicates", "I", 10, 5, 3, [2, 0, 3, 2, 3], False, dict(m_max=3, vza=(30.0,), vaz=(0.0,))),
    ("iqu_n27_sub0_all_levels", "IQU", 9, 70, 4, None, True, dict(m_max=1)),
    ("iquv_n128", "IQUV", 57, 2, 3, None, False, dict(m_max=1, vza=(30.0, 5.0), vaz=(0.0, 60.0))),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fluxes_lin_against_oracle_fp64(vsm, arch, case):
    """1e-8 per field and slot, relative to the largest value over levels and points: the bound of
    test_multisensor_lin_against_oracle_fp64 for the vectors these quantities are quadratures of."""
    name, pol, lt, S, L, levels, sub0, kw = case
    pm, pl, om, ol = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(len(name)), **kw)
    N = pm.quad_points.Nquad * pm.polarization_type.n
    assert "_n%d" % N in name
    m0 = dataclasses.replace(pm, m_max=0)
    assert (vsm.CoreRTLin.SceneLin(m0, pl, 0, 1, 1).sub0 is not None) == sub0
    res = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1, levels)
    lv = list(range(L + 1)) if levels is None else levels
    assert res.levels == lv and res.up.shape == (len(lv), S) and res.up_dot.shape == (len(lv), S, 2) and res.up_dot.dtype == np.float64
    idx = _idx(S)
    ref = FL.fluxes_lin(*_sub(om, ol, idx), lv)
    errs = _worst(res, ref, idx)
    print("FLUX-LIN %-30s N %3d S %3d: %s" % (name, N, S, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-8, (name, errs)
    _check_level0_and_identities(res, lv)
    if levels is None:
        assert res.absorbed_dot.shape == (L, S, 2) and res.surface_absorbed_dot.shape == (S, 2)
        tot = res.absorbed_dot.sum(0) + res.surface_absorbed_dot + res.up_dot[0]
        assert np.abs(tot).max() <= 1e-12 * np.abs(res.up_dot).max()
    else:
        assert res.absorbed_dot is None and res.surface_absorbed_dot is None and res.absorbed is None


def test_fluxes_lin_with_an_aerosol(vsm, arch):
    """Stokes_IQU, one aerosol with its seven slots, a gas and the albedo (NSurf = 1): 9 slots.  (A model with an aerosol slot
    does not take the m = 0 sub-scene, SceneLin's rule; the sub-scene is the case above.)"""
    from test_gpu_optics import _lin_twin
    om, ol, pm, pl = _lin_twin(vsm, arch, 1, 1, S=3, L=4, pol="IQU", l_trunc=9)
    levels = [0, 2, 3, 4, 1]
    res = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 1, 1, 1, levels)
    assert res.up_dot.shape == (5, 3, 9)
    errs = _worst(res, FL.fluxes_lin(om, ol, levels))
    print("FLUX-LIN aerosol: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1e-8, errs
    _check_level0_and_identities(res, levels)


def _sibling(pm, ms, levels):
    """The diffuse fields and their derivatives from rt_run_multisensor(streams=True)'s m = 0 vectors, in float64."""
    qp = pm.quad_points
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    n = pm.polarization_type.n
    rows = {}
    for i, l in enumerate(levels):
        z = 0.0 if l == 0 else 1.0
        uw, dw = ms.uw_streams[i][0][::n, 0].astype(np.float64), z * ms.dw_streams[i][0][::n, 0].astype(np.float64)        # [Nq, S]
        ud, dd = ms.uw_dot_streams[i][0][::n, 0].astype(np.float64), z * ms.dw_dot_streams[i][0][::n, 0].astype(np.float64)  # [Nq, S, P]
        for k, wt, v in (("up", mu * w, uw), ("down_diffuse", mu * w, dw), ("actinic_up", w, uw), ("actinic_down_diffuse", w, dw)):
            rows.setdefault(k, []).append(wt @ v)
        for k, wt, v in (("up", mu * w, ud), ("down_diffuse", mu * w, dd), ("actinic_up", w, ud), ("actinic_down_diffuse", w, dd)):
            rows.setdefault(k + "_dot", []).append(np.tensordot(wt, v, axes=(0, 0)))
    return {k: np.array(v) for k, v in rows.items()}


@pytest.mark.parametrize("thermal", [False, True], ids=["solar", "solar_thermal"])
def test_fluxes_lin_against_the_multisensor_run(vsm, arch, thermal):
    """The level algebra is that of CoreRTLin.rt_run_multisensor; only the reduction differs (one wave's butterfly against a
    float64 dot product): 4 (N / n_stokes) eps of the largest value per field and slot.  m_max does not enter: m_max = 3 gives
    the bits of m_max = 0.  The forward fields are CoreRT.rt_run_fluxes' to 1e-12 (the bound of
    test_forward_part_is_rt_run_multisensor for the linearized walk against the forward one)."""
    H = vsm.host_model
    S, L = 4, 5
    pm, pl, om, ol = _pair(vsm, arch, "IQU", 13, S, L, np.random.default_rng(21), m_max=3, albedo=0.2)
    if thermal:
        B = 0.05 + 0.1 * np.random.default_rng(23).random((L, S))
        Bd = np.stack([np.ones((L, S)), 0.3 + 0.1 * np.arange(L)[:, None] * np.ones((1, S))])
        pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=B, B_layer_dot=Bd))
    levels = list(range(L + 1))
    res = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1, levels)
    ms = vsm.CoreRTLin.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True)
    want = _sibling(pm, ms, levels)
    Nq = pm.quad_points.Nquad
    errs = {k: (_rel(getattr(res, k), v) if v.ndim == 2 else max(_rel(getattr(res, k)[..., p], v[..., p]) for p in range(v.shape[-1])))
            for k, v in want.items()}
    bound = 4 * Nq * np.finfo(np.float64).eps
    print("FLUX-LIN vs multisensor (thermal %s): %s (bound %.1e)" % (thermal, " ".join("%s %.1e" % kv for kv in errs.items()), bound))
    assert max(errs.values()) <= bound, errs
    assert res.up_dot.shape[-1] == (4 if thermal else 2)
    r0 = vsm.CoreRTLin.rt_run_fluxes(dataclasses.replace(pm, m_max=0), pl, 0, 1, 1, levels)
    assert all(np.array_equal(getattr(r0, k + s), getattr(res, k + s)) for k in FIELDS for s in ("", "_dot"))
    if thermal:
        pm = dataclasses.replace(pm, sources=(H.SolarBeam(), H.ThermalEmission(B_layer=B)))
    fwd = vsm.CoreRT.rt_run_fluxes(pm, levels, thermal=thermal)
    e = {k: _rel(getattr(res, k), getattr(fwd, k).astype(np.float64)) for k in FIELDS + ("absorbed", "surface_absorbed")}
    print("FLUX-LIN forward fields vs CoreRT.rt_run_fluxes: %s" % " ".join("%s %.1e" % kv for kv in e.items()))
    assert max(e[k] for k in FIELDS) <= 1e-12, e
    assert np.array_equal(res.down_direct, fwd.down_direct)


@pytest.mark.parametrize("solar", [True, False], ids=["solar+thermal", "thermal_only"])
def test_fluxes_lin_thermal_against_oracle(vsm, arch, solar):
    """ThermalEmission with two Planck tables: slots gas, albedo, Planck 0, Planck 1.  1e-8 as above."""
    H = vsm.host_model
    S, L = 3, 4
    pm, pl, om, ol = _pair(vsm, arch, "IQU", 9, S, L, np.random.default_rng(31), m_max=2)
    B = 0.05 + 0.1 * np.random.default_rng(32).random((L, S))
    Bd = np.stack([np.ones((L, S)), np.zeros((L, S))])
    Bd[1, 2] = 1.0
    th = H.ThermalEmission(B_layer=B, B_layer_dot=Bd)
    pm.sources = (H.SolarBeam(), th) if solar else (th,)
    levels = [2, 0, 4, 1, 3]
    res = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1, levels)
    assert res.up_dot.shape == (5, S, 4)
    ref = FL.fluxes_lin(om, ol, levels, B=B, B_dot=Bd, solar=solar)
    errs = _worst(res, ref)
    print("FLUX-LIN-TH %s: %s" % ("solar+thermal" if solar else "thermal_only", " ".join("%s %.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-8, errs
    _check_level0_and_identities(res, levels)
    assert np.all(res.down_direct_dot[..., 1:] == 0)            # the albedo and the Planck slots do not move the beam
    assert np.abs(res.up_dot[..., 2:]).min() > 0
    if not solar:
        assert np.all(res.down_direct == 0) and np.all(res.down_direct_dot == 0)


def test_fluxes_lin_float32(vsm, arch):
    """A Float32 model against the FP64 oracle at the bound of test_multisensor_lin_fp32 (2e-2), per field and slot."""
    pm, pl, om, ol = _pair(vsm, arch, "IQU", 9, 3, 5, np.random.default_rng(8), FT=np.float32)
    res = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1)
    assert res.up.dtype == np.float32 and res.up_dot.dtype == np.float32 and res.absorbed_dot.dtype == np.float32
    ref = FL.fluxes_lin(om, ol, res.levels)
    errs = _worst(res, ref)
    print("FLUX-LIN f32: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < 2e-2, errs


@pytest.mark.parametrize("S,max_points", [(7, 3), (140, 64)])
def test_blocked_runs_are_bit_identical(vsm, arch, S, max_points):
    """7 points in blocks of 3, 3, 1; 140 points (the m = 0 sub-scene applies) in blocks of 64 and 76."""
    H = vsm.host_model
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, S, 4, np.random.default_rng(10), m_max=3)
    if S == 7:
        pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=np.full((4, S), 0.1), B_layer_dot=np.ones((1, 4, S))))
    one = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1)
    blk = vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1, max_points=max_points)
    for k in FIELDS + ("absorbed", "surface_absorbed"):
        assert np.array_equal(getattr(one, k), getattr(blk, k)), k
        assert np.array_equal(getattr(one, k + "_dot"), getattr(blk, k + "_dot")), k


def test_level_calls(vsm, arch, monkeypatch):
    """Per level other than 0 one elastic and one flux call per slot kind (solar, thermal), one flux call at level 0, no
    vsm_level_radiance_lin* call, no [P, S, N] vector."""
    H = vsm.host_model
    MS, MSLIN, FXL = vsm.core_rt_ms, vsm.core_rt_ms_lin, vsm.core_rt_flux_lin
    counts = dict(lev=0, flux=0, levlin=0)

    def wrap(mod, name, key):
        f = getattr(mod, name)

        def g(*args, **kw):
            counts[key] += 1
            return f(*args, **kw)
        monkeypatch.setattr(mod, name, g)
    wrap(MS, "level_radiance_", "lev")
    wrap(FXL, "level_flux_lin_", "flux")
    wrap(MSLIN, "level_radiance_lin_", "levlin")
    wrap(MSLIN, "level_radiance_lin_src_", "levlin")
    pm, pl, _, _ = _pair(vsm, arch, "IQU", 9, 4, 8, np.random.default_rng(1), m_max=3)
    vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1, [0, 3, 6, 8])
    assert counts == dict(lev=3, flux=4, levlin=0), counts
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=np.full((8, 4), 0.1), B_layer_dot=np.ones((2, 8, 4))))
    counts.update(lev=0, flux=0)
    vsm.CoreRTLin.rt_run_fluxes(pm, pl, 0, 1, 1, [3, 6, 8])
    assert counts == dict(lev=6, flux=6, levlin=0), counts


def test_refusals(vsm, arch, monkeypatch):
    """Each before any layer or level kernel is launched."""
    H, CL = vsm.host_model, vsm.CoreRTLin
    launched = []
    for mod, name in ((CL, "doubling_allparams_"), (vsm.core_rt_flux_lin, "level_flux_lin_"), (vsm.core_rt_ms, "level_radiance_")):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **k: launched.append(_n))
    pm, pl, _, _ = _pair(vsm, arch, "I", 9, 2, 4, np.random.default_rng(3))
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=np.full((4, 2), 0.1)))
    with pytest.raises(vsm.VSMError, match="B_layer_dot"):
        CL.rt_run_fluxes(pm, pl, 0, 1, 1, [1])
    pm.sources = (H.SolarBeam(), H.SurfaceSIF(np.full(2, 1e-3)))
    with pytest.raises(NotImplementedError, match="SurfaceSIF"):
        CL.rt_run_fluxes(pm, pl, 0, 1, 1, [1])
    tr = np.tile(np.full(4, 0.05), (2, 1))
    tr[:, 2] = 0.0
    g = np.full((2, 4), 1e-3)
    pm = H.model_from_arrays(arch, "I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, tau_abs=g, albedo=0.2, m_max=1)
    with pytest.raises(NotImplementedError, match="does not scatter"):
        CL.rt_run_fluxes(pm, H.LinModel([g]), 0, 1, 1, [1])
    pm, pl, _, _ = _pair(vsm, arch, "IQUV", 61, 2, 3, np.random.default_rng(3))
    with pytest.raises(vsm.VSMError, match="128"):
        CL.rt_run_fluxes(pm, pl, 0, 1, 1, [1])
    with pytest.raises(ValueError):
        CL.rt_run_fluxes(pm, pl, 0, 1, 1, [4])
    assert launched == []
