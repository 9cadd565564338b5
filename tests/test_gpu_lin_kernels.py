"""The linearized doubling and interaction kernels at kernel level: k_dbl128_lin<RT, ST> / k_ia128_lin<RT, ST>
(vsm_strip128lin.hip; every Jacobian goes through them) and, for FP64 at N = 49..60, k_dbl_lin_multi / k_dbl_lin_step
(vsm_striplin.hip), driven through CoreRTLin.doubling_allparams_ / interaction_lin_ on directly constructed layers and compared
with oracle/vsm_oracle_lin.py in float64:

  1  every N in 1..128, both storage types (FP64; FP32 arrays with FP64 arithmetic)
  2  parameter counts 1, 3, 4, 17, 64 and the doubling's N_active = P - 1
  3  the shared surface block (mat_stride 0, parameter stride N N) at the row-tile seams, all four interfaces
  4  slot ranges (vsm_interaction_lin_range_*): slots outside [p_lo, p_hi) keep their bits
  5  a second spectral point per persistent workgroup at every residency / occupancy policy
  6  the pivoted inverse near and beyond unit spectral radius, with derivatives

Tolerances.  FP64: 1e-10 of an array's maximum for the forward arrays, 1e-9 for the derivative arrays (as tests/test_gpu_lin.py),
taken per spectral point over the array's global maximum so that a failure names the point.  FP32 storage: the reference is the
float64 oracle on float32-rounded inputs (doubling_lin_storage restates the roundings of the storage contract); the ceiling of a
part is twice the worst error measured on the MI355X (FP32_MEASURED, in units of 2^-23 of the array's maximum) and never above
8 * 2^-23: the reference's own storage rounding is <= 0.46 * 2^-23 on these inputs, an all-FP32 evaluation reaches 3 .. 40 * 2^-23.
Every test prints its worst errors (pytest -s)."""
import copy

import numpy as np
import pytest

from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
TOL64 = {False: 1e-10, True: 1e-9}      # forward / derivative arrays
FP32_CONDITION = 8.0                    # in units of EPS32 of the array's maximum: holds whatever is measured
# FP32 storage: worst error of any of the twelve arrays measured on the MI355X, per part, in units of EPS32 of the array's maximum
# (all below 0.5: the rounding of the output to float32 and nothing else -- every ceiling is the floor 2^-23)
FP32_MEASURED = {1: 0.490, 2: 0.452, 3: 0.473, 4: 0.462, 5: 0.427}
MU0 = 0.766044443118978                 # cos(40 deg)
FWD_C, FWD_A = ("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m"), ("r_mp", "t_pp", "r_pm", "t_mm", "j0_p", "j0_m")
LIN_A = tuple("ap_" + k for k in ("r_mp", "t_pp", "r_pm", "t_mm", "J0_p", "J0_m"))
IDS = {np.float64: "fp64", np.float32: "fp32"}


def fp32_ceiling(part):
    """Twice the measured worst error, not below one unit of 2^-23 (and the test asserts the 8 * 2^-23 condition beside it)."""
    return max(2.0 * FP32_MEASURED[part], 1.0)


# ---- reference helpers (no GPU) -------------------------------------------------------------------------------------------------
def stokes_for(N):
    """The Stokes count whose apply_D! epilogue flips signs wherever N allows it."""
    return O.polarization("IQUV" if N % 4 == 0 else ("IQU" if N % 3 == 0 else "I"))


def doubling_lin_storage(pol, expk, ndoubl, added, added_lin, dtau_dot_all, mu0, N_active, ST):
    """OL.doubling_lin in float64 with the roundings of the kernels' storage contract for arrays of type ST restated -- what
    k_dbl128_lin<RT, ST> (vsm_strip128lin.hip) keeps in the caller's arrays BETWEEN the doubling steps:
      * the ekl table: set up by k_ekl_init<ST> in ST arithmetic, (-expk / mu0) * dtau_dot, then read and written back as
        ST(2 expk ekl) in every step;
      * the derivative source vectors ap_J0+-: read from and written to the caller's arrays in every step.
    expk is read once per point and squared in double; r, t, their derivatives and j0+- stay in double (registers / scratch / LDS)
    over all steps.  The values the last step leaves are not rounded here: that is the output rounding under test.  With
    ST = float64 this is OL.doubling_lin statement by statement."""
    if ndoubl == 0:
        return
    FT = np.float64
    st = lambda x: np.asarray(x, dtype=ST).astype(FT)
    r, t = added.r_mp.copy(), added.t_pp.copy()
    jp, jm = added.j0_p.copy(), added.j0_m.copy()
    ar, at = added_lin.ap_r_mp, added_lin.ap_t_pp
    aJp, aJm = added_lin.ap_J0_p, added_lin.ap_J0_m
    P_all = ar.shape[0]
    Np = N_active if N_active > 0 else P_all
    N = r.shape[1]
    I = np.eye(N, dtype=FT)[None]
    expk = expk.astype(FT).copy()
    ek_lin = (np.stack([(-expk.astype(ST) / ST(mu0) * dtau_dot_all[:, p].astype(ST)).astype(FT) for p in range(Np)]) if Np
              else np.zeros((0, len(expk)), dtype=FT))
    mv = O._mv
    for step in range(ndoubl):
        last = step == ndoubl - 1
        G = np.linalg.inv(I - r @ r).astype(FT)
        tt = t @ G
        G_lin = [G @ (ar[p] @ r + r @ ar[p]) @ G for p in range(Np)]
        tt_lin = [at[p] @ G + t @ G_lin[p] for p in range(Np)]
        J1p, J1m = jp * expk[:, None], jm * expk[:, None]
        A = J1m + mv(r, jp)
        B = jp + mv(r, J1m)
        for p in range(Np):
            aJ1p = aJp[p] * expk[:, None] + jp * ek_lin[p][:, None]
            aJ1m = aJm[p] * expk[:, None] + jm * ek_lin[p][:, None]
            ek_lin[p] = st(2 * expk * ek_lin[p])
            new_m = aJm[p] + mv(tt_lin[p], A) + mv(tt, aJ1m + mv(ar[p], jp) + mv(r, aJp[p]))
            new_p = aJ1p + mv(tt_lin[p], B) + mv(tt, aJp[p] + mv(ar[p], J1m) + mv(r, aJ1m))
            aJm[p], aJp[p] = (new_m, new_p) if last else (st(new_m), st(new_p))
        jm_new = jm + mv(tt, A)
        jp_new = J1p + mv(tt, B)
        jm, jp = jm_new, jp_new
        expk = expk ** 2
        rt = r @ t
        for p in range(Np):
            ar_new = ar[p] + tt_lin[p] @ rt + tt @ (ar[p] @ t + r @ at[p])
            at[p] = tt_lin[p] @ t + tt @ at[p]
            ar[p] = ar_new
        r = r + tt @ rt
        t = tt @ t
    D = O._dsign(pol, N).astype(FT)
    par = (D[:, None] * D[None, :])[None]
    if pol.n == 1:
        added.r_mp[...], added.t_pp[...], added.r_pm[...], added.t_mm[...] = r, t, r, t
        added.j0_p[...], added.j0_m[...] = jp, jm
        added_lin.ap_r_pm[...] = ar
        added_lin.ap_t_mm[...] = at
        return
    r = r * D[None, :, None]
    added.r_mp[...], added.t_pp[...] = r, t
    added.r_pm[...], added.t_mm[...] = par * r, par * t
    added.j0_p[...], added.j0_m[...] = jp, jm * D[None, :]
    ar *= D[None, None, :, None]
    added_lin.ap_r_pm[...] = par[None] * ar
    added_lin.ap_t_mm[...] = par[None] * at
    aJm *= D[None, None, :]


def random_layers(rng, N, S, P, ST, shared=False):
    """Physically shaped operators as _random_layers of tests/test_gpu_parity.py -- small reflections, near-diagonal transmissions --
    and derivative arrays 0.1 N(0, 1) as test_interaction_lin: float64 arrays holding values of the storage type ST.
    shared: ONE added layer and one set of its derivative matrices for all points."""
    q = lambda x: x.astype(ST).astype(np.float64)
    refl = lambda sc: q(sc * rng.random((S, N, N)) / N)
    trans = lambda: q(np.eye(N) * rng.uniform(0.3, 0.95, (S, N, 1)) + 0.05 * rng.random((S, N, N)) / N)
    vec = lambda: q(rng.random((S, N)))
    dm, dv = lambda: q(0.1 * rng.standard_normal((P, S, N, N))), lambda: q(0.1 * rng.standard_normal((P, S, N)))
    comp = O.CompositeLayer(refl(1.5), refl(1.5), trans(), trans(), vec(), vec())
    add = O.AddedLayer(refl(1.0), trans(), refl(1.0), trans(), vec(), vec())
    cl = OL.CompositeLayerLin(dm(), dm(), dm(), dm(), dv(), dv())
    al = OL.AddedLayerLin(dm(), dm(), dm(), dm(), dv(), dv())
    if shared:
        for k in FWD_A[:4]:
            getattr(add, k)[...] = getattr(add, k)[:1]
        for k in LIN_A[:4]:
            getattr(al, k)[...] = getattr(al, k)[:, :1]
    return comp, add, cl, al


def doubling_inputs(rng, N, S, P, ST, n_active=0):
    """An added layer for the doubling (r_mp *= 0.2), expk in U(0.5, 0.99), a nonzero dtau_dot_all; n_active > 0: the slots from
    n_active on are zero in every input (the caller's contract for N_active)."""
    q = lambda x: x.astype(ST).astype(np.float64)
    _, add, _, al = random_layers(rng, N, S, P, ST)
    add.r_mp[...] = q(0.2 * add.r_mp)
    expk, dall = q(rng.uniform(0.5, 0.99, S)), q(0.1 * rng.standard_normal((S, P)))
    if n_active:
        dall[:, n_active:] = 0.0
        for k in ("ap_r_mp", "ap_t_pp", "ap_J0_p", "ap_J0_m"):     # (ap_r_pm / ap_t_mm are outputs: what they hold must not matter)
            getattr(al, k)[n_active:] = 0.0
    return add, al, expk, dall


def tile_points(x, S, axis):
    """S points along `axis` by repeating the points that are there."""
    return np.take(x, np.arange(S) % x.shape[axis], axis=axis)


class Worst:
    """Collects the error of every compared array; done() prints the worst ones and fails on what went over its tolerance."""

    def __init__(self, ST, part, tol=None):
        self.ST, self.part, self.tol, self.worst, self.bad = ST, part, tol, {False: 0.0, True: 0.0}, []

    def check(self, tag, got, ref, lin):
        """max over the spectral points of the point's own error over the array's global maximum (the spectral axis is the first
        of a forward array and the second of a derivative array)."""
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (tag, got.shape, ref.shape)
        d = np.moveaxis(np.abs(got - ref), 1 if lin else 0, 0)
        per_point = d.reshape(d.shape[0], -1).max(axis=1) / max(np.abs(ref).max(), 1e-300)
        e = float(np.nan_to_num(per_point, nan=np.inf).max())
        self.worst[lin] = max(self.worst[lin], e)
        if self.tol is not None:
            tol = self.tol[lin]
        elif self.ST == np.float64:
            tol = TOL64[lin]
        else:
            tol = min(fp32_ceiling(self.part), FP32_CONDITION) * EPS32
        if not e < tol:
            self.bad.append((tag, "point %d" % int(np.argmax(np.nan_to_num(per_point, nan=np.inf))), e, tol))

    def done(self, name):
        unit, u = (EPS32, " x 2^-23") if self.ST == np.float32 else (1.0, "")
        print("\n%s [%s]: worst forward %.3g%s, worst derivative %.3g%s"
              % (name, IDS[self.ST], self.worst[False] / unit, u, self.worst[True] / unit, u))
        assert not self.bad, (len(self.bad), self.bad[:6])


# ---- device side ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vsm():
    import torch
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU()


def _up(vsm, arch, ST, x, matrix):
    """math order [..., i, j] -> the column-major layout tensor of type ST"""
    x = np.swapaxes(x, -1, -2) if matrix else x
    return vsm.Architectures.array_type(arch)(np.ascontiguousarray(x, dtype=ST))


def _down(vsm, t, matrix):
    x = vsm.Architectures.to_host(t)
    return np.swapaxes(x, -1, -2).copy() if matrix else x.copy()


def upload_added(vsm, arch, ST, add, al, shared=False):
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    P, S, N = al.ap_J0_p.shape
    pa, pal = CR.AddedLayer(ST, arch, N, S, shared=shared), CL.AddedLayerLin(ST, arch, P, N, S, shared=shared)
    for k in FWD_A:
        x = getattr(add, k)
        getattr(pa, k).copy_(_up(vsm, arch, ST, x[:1] if shared and x.ndim == 3 else x, x.ndim == 3))
    for k in LIN_A:
        x = getattr(al, k)
        getattr(pal, k).copy_(_up(vsm, arch, ST, x[:, :1] if shared and x.ndim == 4 else x, x.ndim == 4))
    return pa, pal


def upload_composite(vsm, arch, ST, comp, cl):
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    P, S, N = cl.J0_p.shape
    pc, pcl = CR.CompositeLayer(ST, arch, N, S), CL.CompositeLayerLin(ST, arch, P, N, S)
    for k in FWD_C:
        getattr(pc, k).copy_(_up(vsm, arch, ST, getattr(comp, k), getattr(comp, k).ndim == 3))
        getattr(pcl, k).copy_(_up(vsm, arch, ST, getattr(cl, k), getattr(cl, k).ndim == 4))
    return pc, pcl


def download(vsm, obj, keys):
    return {k: _down(vsm, getattr(obj, k), "j0" not in k.lower()) for k in keys}


def device_status(vsm):
    import ctypes as C
    flags = (C.c_int * 4)()
    assert vsm._lib.lib().vsm_device_status(flags, 1, None) == 0
    return list(flags)


def same_bits_in_every_repeat(x, axis, n0):
    """every point s of x along `axis` has the bits of point s mod n0"""
    return np.array_equal(x, tile_points(np.take(x, np.arange(n0), axis=axis), x.shape[axis], axis), equal_nan=True)


def run_doubling(vsm, arch, w, tag, rng, N, S, P, ST, nd=2, n_active=0, S_dev=None):
    """doubling_allparams_ on random layers vs the oracle: six forward arrays, expk and six derivative arrays.  S_dev: the S points
    are tiled to S_dev on the device; every repeat must have the bits of the first."""
    pol = stokes_for(N)
    hpol = vsm.host_model.polarization_type(pol.name)
    add, al, expk, dall = doubling_inputs(rng, N, S, P, ST, n_active)
    d_add, d_al, d_expk, d_dall = add, al, expk, dall
    if S_dev:
        d_add, d_al = copy.copy(add), copy.copy(al)
        for k in FWD_A:
            setattr(d_add, k, tile_points(getattr(add, k), S_dev, 0))
        for k in LIN_A:
            setattr(d_al, k, tile_points(getattr(al, k), S_dev, 1))
        d_expk, d_dall = tile_points(expk, S_dev, 0), tile_points(dall, S_dev, 0)
    pa, pal = upload_added(vsm, arch, ST, d_add, d_al)
    t_expk = _up(vsm, arch, ST, d_expk, False)
    CL = vsm.CoreRTLin
    CL.doubling_allparams_(hpol, t_expk, nd, pa, pal, CL.to_device_sp(d_dall, arch, ST), MU0, n_active)
    got, gotl, got_k = download(vsm, pa, FWD_A), download(vsm, pal, LIN_A), _down(vsm, t_expk, False)
    if ST == np.float64:
        OL.doubling_lin(pol, expk, nd, add, al, dall, MU0, n_active, np.float64)
    else:
        doubling_lin_storage(pol, expk, nd, add, al, dall, MU0, n_active, ST)
    if S_dev:
        for k, v in list(got.items()) + [("expk", got_k)]:
            assert same_bits_in_every_repeat(v, 0, S), (tag, k)
        for k, v in gotl.items():
            assert same_bits_in_every_repeat(v, 1, S), (tag, k)
        got, gotl, got_k = {k: v[:S] for k, v in got.items()}, {k: v[:, :S] for k, v in gotl.items()}, got_k[:S]
    for k in FWD_A:
        w.check(tag + (k,), got[k], getattr(add, k), False)
    w.check(tag + ("expk",), got_k, expk ** (2 ** nd), False)
    for k in LIN_A:
        w.check(tag + (k,), gotl[k], getattr(al, k), True)


def run_interaction(vsm, arch, w, tag, rng, N, S, P, ST, iface="11", shared=False, p_range=None, S_dev=None, layers=None):
    """interaction_lin_ on random layers (or `layers`) vs the oracle: the composite's six forward and six derivative arrays.
    p_range = (p_lo, p_hi): the slots outside it hold a recognisable pattern in all twelve derivative arrays and must keep its bits;
    the oracle runs on the slices.  S_dev as in run_doubling."""
    comp, add, cl, al = layers if layers is not None else random_layers(rng, N, S, P, ST, shared)
    lo, hi = p_range if p_range else (0, P)
    outside = [p for p in range(P) if not lo <= p < hi]
    for i, arr in enumerate([getattr(cl, k) for k in FWD_C] + [getattr(al, k) for k in LIN_A]):
        for p in outside:
            arr[p] = 7.0 + p + 0.125 * i          # (exact in float32 too)
    d_comp, d_add, d_cl, d_al = comp, add, cl, al
    if S_dev:
        d_comp, d_add, d_cl, d_al = copy.copy(comp), copy.copy(add), copy.copy(cl), copy.copy(al)
        for o, src, keys, ax in ((d_comp, comp, FWD_C, 0), (d_add, add, FWD_A, 0), (d_cl, cl, FWD_C, 1), (d_al, al, LIN_A, 1)):
            for k in keys:
                setattr(o, k, tile_points(getattr(src, k), S_dev, ax))
    pc, pcl = upload_composite(vsm, arch, ST, d_comp, d_cl)
    pa, pal = upload_added(vsm, arch, ST, d_add, d_al, shared)
    vsm.CoreRTLin.interaction_lin_(iface, pc, pcl, pa, pal, p_range=p_range)
    got, gotl = download(vsm, pc, FWD_C), download(vsm, pcl, FWD_C)
    if outside:
        got_al = download(vsm, pal, LIN_A)
        for i, k in enumerate(FWD_C):
            assert np.array_equal(gotl[k][outside], getattr(cl, k)[outside].astype(ST)), (tag, "composite", k)
        for k in LIN_A:
            src = getattr(al, k)
            src = src[:, :1] if shared and src.ndim == 4 else src
            assert np.array_equal(got_al[k][outside], src[outside].astype(ST)), (tag, "added", k)
        cl, al = copy.copy(cl), copy.copy(al)
        for k in FWD_C:
            setattr(cl, k, getattr(cl, k)[lo:hi].copy())
        for k in LIN_A:
            setattr(al, k, getattr(al, k)[lo:hi].copy())
        gotl = {k: v[lo:hi] for k, v in gotl.items()}
    OL.interaction_lin(iface, comp, cl, add, al, np.float64)
    if S_dev:
        for k in FWD_C:
            assert same_bits_in_every_repeat(got[k], 0, S), (tag, k)
            assert same_bits_in_every_repeat(gotl[k], 1, S), (tag, "d" + k)
        got, gotl = {k: v[:S] for k, v in got.items()}, {k: v[:, :S] for k, v in gotl.items()}
    for k in FWD_C:
        w.check(tag + (k,), got[k], getattr(comp, k), False)
        w.check(tag + ("d" + k,), gotl[k], getattr(cl, k), True)


# ---- 1. every size, both storage types ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ST", [np.float64, np.float32], ids=IDS.get)
@pytest.mark.parametrize("first", range(1, 129, 16))
def test_lin_kernels_every_size(vsm, arch, first, ST):
    """Every N of one row-tile window (RT = ceil(N / 16): the last row and column at every position of a tile, the seams 16 k /
    16 k + 1): interaction 11 and two doubling steps with S = 3, P = 2; FP64 at N = 49..60 is k_dbl_lin_multi, and with P = 4
    k_dbl_lin_step."""
    w = Worst(ST, 1)
    for N in range(first, first + 16):
        rng = np.random.default_rng(1000 + N)
        run_interaction(vsm, arch, w, (N, "ia"), rng, N, 3, 2, ST)
        run_doubling(vsm, arch, w, (N, "dbl"), rng, N, 3, 2, ST)
        if 49 <= N <= 60:
            run_doubling(vsm, arch, w, (N, "dbl P=4"), rng, N, 3, 4, ST)
    w.done("every size %d..%d" % (first, first + 15))


# ---- 2. parameter-count edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,ST", [(N, P, np.float64) for N in (21, 80) for P in (1, 3, 4, 17, 64)] + [(128, 64, np.float64)] +
                         [(21, 17, np.float32), (80, 17, np.float32)], ids=lambda v: IDS.get(v, str(v)))
def test_lin_kernels_parameter_counts(vsm, arch, N, P, ST):
    """P up to the drivers' limit of 64 slots: the doubling scratch has DL_FIXED + 2 P slots, the parameter loops of both kernels
    walk P slots of stride N N S; strips in registers (N = 21) and parked in scratch (N = 80, 128).  And the doubling with
    N_active = P - 1 and a zero last slot: all of that slot's arrays as the oracle's."""
    w = Worst(ST, 2)
    rng = np.random.default_rng(2000 + 100 * N + P)
    run_interaction(vsm, arch, w, ("ia",), rng, N, 2, P, ST)
    run_doubling(vsm, arch, w, ("dbl",), rng, N, 2, P, ST)
    if P > 1:
        run_doubling(vsm, arch, w, ("dbl N_active=P-1",), rng, N, 2, P, ST, n_active=P - 1)
    w.done("N = %d, P = %d" % (N, P))


# ---- 3. shared surface block at the seams ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ST", [(N, ST) for ST in (np.float64, np.float32) for N in (16, 17, 80, 128)],
                         ids=lambda v: IDS.get(v, str(v)))
def test_interaction_lin_shared_surface_block_at_the_seams(vsm, arch, N, ST):
    """One added layer and one set of derivative matrices for all points (mat_stride == 0, parameter stride N N instead of
    N N S) with P = 5, S = 3: all four interfaces in FP64, interface 11 with FP32 storage."""
    w = Worst(ST, 3)
    for iface in (("11", "01", "10", "00") if ST == np.float64 else ("11",)):
        rng = np.random.default_rng(3000 + N)
        run_interaction(vsm, arch, w, (iface,), rng, N, 3, 5, ST, iface=iface, shared=True)
    w.done("shared, N = %d" % N)


# ---- 4. slot ranges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["per-point", "shared"])
@pytest.mark.parametrize("N,ST", [(N, ST) for ST in (np.float64, np.float32) for N in (21, 72)], ids=lambda v: IDS.get(v, str(v)))
def test_interaction_lin_slot_ranges(vsm, arch, N, ST, shared):
    """interaction_lin_(..., p_range=(p_lo, p_hi)) with P = 6: the slots outside the range keep their bits in all twelve derivative
    arrays, the slots inside and the forward arrays are the oracle's on the sliced arrays."""
    w = Worst(ST, 4)
    for iface in (("11", "01", "10", "00") if ST == np.float64 else ("11",)):
        for p_range in ((2, 5), (0, 3), (5, 6)):
            rng = np.random.default_rng(4000 + N)
            run_interaction(vsm, arch, w, (iface, p_range), rng, N, 3, 6, ST, iface=iface, shared=shared, p_range=p_range)
    w.done("slot ranges, N = %d, %s" % (N, "shared" if shared else "per-point"))


# ---- 5. a second point per workgroup --------------------------------------------------------------------------------------------
def wg_per_cu(N):
    """wg_per_cu<RT>::value, vsm_strip128lin.hip:82: RT == 1 ? 8 : (RT == 2 ? 4 : (RT <= 4 ? 2 : 1)), i.e. 8 / 4 / 2 / 2 / 1
    persistent workgroups per CU for RT = 1 / 2 / 3 / 4 / >= 5; the launches use that many times the CU count (:613-614, :628-629)."""
    RT = (N + 15) // 16
    return 8 if RT == 1 else (4 if RT == 2 else (2 if RT <= 4 else 1))


@pytest.mark.parametrize("N,ST", [(N, np.float64) for N in (16, 32, 48, 96, 113)] + [(16, np.float32), (113, np.float32)],
                         ids=lambda v: IDS.get(v, str(v)))
def test_lin_kernels_second_point_per_workgroup(vsm, arch, N, ST):
    """Three more spectral points than the launch has workgroups (RT = 1, 2, 3, 6, 8; 4 and 5 are walked end to end by
    test_strip128lin_persistent_workgroups_walk_the_spectral_axis): three workgroups take a second point and reuse their LDS
    tables, reduction slots and scratch.  The points are 3 distinct ones tiled: every repeat the bits of the first, the first
    three the oracle's.  Two doubling steps with P = 2 and interaction 11."""
    import torch
    S_dev = wg_per_cu(N) * torch.cuda.get_device_properties(0).multi_processor_count + 3
    w = Worst(ST, 5)
    rng = np.random.default_rng(5000 + N)
    run_doubling(vsm, arch, w, ("dbl",), rng, N, 3, 2, ST, S_dev=S_dev)
    run_interaction(vsm, arch, w, ("ia",), rng, N, 3, 2, ST, S_dev=S_dev)
    w.done("second point, N = %d, S = %d" % (N, S_dev))


# ---- 6. the inverse near and beyond unit spectral radius, with derivatives --------------------------------------------------------
def ill_conditioned_layers(N, rho, S=3, P=2):
    """random_layers with R+- and r-+ positive matrices scaled so that the Perron root of R+- r-+ is rho; and the worst condition
    number of I - R+- r-+ over the points."""
    rng = np.random.default_rng(6000 + N)
    comp, add, cl, al = random_layers(rng, N, S, P, np.float64)
    comp.R_pm[...] = rng.random((S, N, N)) / N
    add.r_mp[...] = rng.random((S, N, N)) / N
    for s in range(S):
        ev = np.max(np.abs(np.linalg.eigvals(comp.R_pm[s] @ add.r_mp[s])))
        comp.R_pm[s] *= np.sqrt(rho / ev)
        add.r_mp[s] *= np.sqrt(rho / ev)
    cond = max(np.linalg.cond(np.eye(N) - comp.R_pm[s] @ add.r_mp[s]) for s in range(S))
    return (comp, add, cl, al), cond


@pytest.mark.parametrize("N", [24, 64, 72, 128])
@pytest.mark.parametrize("rho", [0.9, 0.97, 0.995, 1.7])
def test_interaction_lin_pivoted_inverse_near_and_beyond_unit_spectral_radius(vsm, arch, N, rho):
    """The linearized twin of test_strip128_pivoted_inverse_near_and_beyond_unit_spectral_radius: interaction 11 with the spectral
    radius of R+- r-+ at rho, where the kernel forms Y G with the pivoted inverse G = (I - E)^-1 (both halves: the second has the
    composite as left operand and other strides).  Both sides solve the same ill-conditioned systems: forward arrays within
    max(1e-10, 50 cond eps), derivative arrays -- G enters them twice -- within max(1e-9, 50 cond^2 eps); every rho asked for keeps
    the derivative tolerance below 1e-6 (test_ill_conditioned_cases_keep_their_tolerance, on the CPU).  No device flag."""
    layers, cond = ill_conditioned_layers(N, rho)
    eps = np.finfo(np.float64).eps
    tol = {False: max(1e-10, 50 * cond * eps), True: max(1e-9, 50 * cond ** 2 * eps)}
    assert tol[True] < 1e-6, (cond, tol)
    w = Worst(np.float64, 6, tol)
    device_status(vsm)
    run_interaction(vsm, arch, w, (rho,), None, N, 3, 2, np.float64, layers=layers)
    st = device_status(vsm)
    assert st[0] == 0, st
    w.done("rho = %g, N = %d, cond = %.3g" % (rho, N, cond))
