"""Inputs and references that pin every inverse order of the layer-step kernels (numpy only; no GPU, no library).

Every layer step ends in (I - E)^-1 -- E = r r in doubling!, E = R+- r-+ in interaction!(_11) -- and every kernel family picks
its own way to compute it from a Frobenius bound on E: a Neumann series of order 1, 2, 3, 4, 7, 8, 15, 16 or 31, or the pivoted
Gauss-Jordan from 0.3 upwards.  This module restates that selection per family (read from each source file, see FAMILIES), builds
nonnegative inputs whose bound lands on a target inside every band and next to every edge, and evaluates the same step

  * in np.longdouble with a Newton-refined inverse (the reference),
  * in the kernel's own precision with Horner at the selected order (only to size the tolerance),
  * with the series cut at degree K // 2 (the mutant: a lost product or a lost squaring level).

Nonnegative data means no cancellation anywhere in the step, so every output array is compared ELEMENTWISE and relatively."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

LD = np.longdouble
F32, F64 = np.float32, np.float64
SERIES = (1, 2, 3, 4, 7, 8, 15, 16, 31)
PIVOT = 0                                    # the order the kernels' rule returns where no series is taken
PIVOT_TARGETS = (0.31, 0.5, 0.9)
EDGE_OFFSET = 4e-4                           # edge points: the bound within +-0.05 % of a band edge
IA_OUT = ("R_mp", "R_pm", "T_pp", "T_mm", "J0_p", "J0_m")
DBL_OUT = ("r_mp", "t_pp", "j0_p", "j0_m")


def have_long_double():
    return np.finfo(LD).eps < 2e-19


# ---- the selection rule, per family ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Family:
    """How one kernel family bounds E and selects the order.
    sel: the type the rule is evaluated in (tol = eps(sel) / 4); arith: the type of the step's arithmetic; io: the type of the
    arrays; pre: a factor on the sum of squares in front of the square root; counts: vsm_device_status word [1] counts the
    family's pivoted inverses."""
    name: str
    sel: type
    arith: type
    io: type
    pre: float
    counts: bool


FAMILIES = {
    # vsm_native_dev.h nnorm / nseries_order: k_ia_native, k_layer_native
    "native64": Family("native64", F64, F64, F64, 1.0, True),
    # vsm_strip_dev.h strip_norm_bound / series_order / invert_strip*: the reference-layout layer kernel k_layer_strip (FP64, 33..64)
    "strip64": Family("strip64", F64, F64, F64, 1.0, False),
    # vsm_strip128_dev.h norm128 / series_order128: k_ia128<double>, k_dbl128<double>
    "strip128": Family("strip128", F64, F64, F64, 1.0, True),
    # ... and the same kernels over Float32 arrays (k_ia128<float>, k_dbl128<float>): FP64 arithmetic and the FP64 tolerance
    "strip128_f32": Family("strip128_f32", F64, F64, F32, 1.0, True),
    # vsm_fused.hip acc_norm_bound / invert_one_minus<float>: k_interaction11<float>
    "fused32": Family("fused32", F32, F32, F32, 1.0, False),
    # vsm_strip32.hip strip_norm_bound / series_order: k_ia_strip32 (the partial sums carry a factor 1.0001f of their own)
    "strip32": Family("strip32", F32, F32, F32, 1.0001, False),
    # vsm_native32_dev.h n32norm / n32series_order: k_layer_native32
    "native32": Family("native32", F32, F32, F32, 1.0, True),
    # the operator-level chain (gemm + batch_inv, vsm_generic.hip doubling): always the pivoted inverse, nothing counted
    "oplevel64": Family("oplevel64", None, F64, F64, 1.0, False),
    "oplevel32": Family("oplevel32", None, F32, F32, 1.0, False),
}


def bound(E, fam):
    """The kernels' bound on ||E||_F for a batch E[S,N,N]: the sum of squares in the family's arithmetic, handed on as a float
    (rounded up), sqrtf, times 1.001f.  (The kernels sum per wave and then over the waves, in float: another order of the same
    sum, which moves the bound by a few 1e-7 -- every target keeps 2 % from the edges, the edge points admit both orders.)"""
    fam = FAMILIES[fam] if isinstance(fam, str) else fam
    E = np.asarray(E, dtype=fam.arith)
    ss = np.sum(E * E, axis=(-2, -1), dtype=fam.arith)
    f = ss.astype(F32)
    f = np.where(f.astype(F64) < ss.astype(F64), np.nextafter(f, F32(np.inf)), f).astype(F32)     # __double2float_ru
    if fam.pre != 1.0:
        f = (f * F32(fam.pre)).astype(F32)
    return (np.sqrt(f, dtype=F32) * F32(1.001)).astype(F32)


def order(nrm, fam):
    """The order the family's rule selects for the bound nrm (a float, as the kernels hold it): the smallest K of SERIES with
    nrm^(K+1) <= tol (1 - nrm), tol = eps / 4, every operation in the rule's own type; PIVOT where nrm is not below 0.3."""
    fam = FAMILIES[fam] if isinstance(fam, str) else fam
    if fam.sel is None:
        return PIVOT
    T = fam.sel
    nrm = T(F32(nrm))
    tol = T(np.finfo(T).eps) * T(0.25)
    if not nrm < T(0.3):
        return PIVOT
    lim = T(tol * T(T(1) - nrm))
    n2 = T(nrm * nrm)
    n4 = T(n2 * n2)
    n8 = T(n4 * n4)
    n16 = T(n8 * n8)
    for K, v in ((1, n2), (2, T(n2 * nrm)), (3, n4), (4, T(n4 * nrm)), (7, n8), (8, T(n8 * nrm)), (15, n16), (16, T(n16 * nrm)),
                 (31, T(n16 * n16))):
        if v <= lim:
            return K
    return PIVOT


@lru_cache(maxsize=None)
def bands(fam_name):
    """{K: (lo, hi)} from the restated rule: per order the smallest and the largest float bound that selects it (lo of the first
    band: 0).  Found by a scan over the floats' exponent range and a bisection over adjacent floats -- not from constants."""
    fam = FAMILIES[fam_name]
    if fam.sel is None:
        return {PIVOT: (0.0, np.inf)}
    grid = np.exp(np.linspace(np.log(1e-12), np.log(0.5), 2001)).astype(F32)
    ks = [order(x, fam) for x in grid]
    out = {ks[0]: [0.0, None]}
    for i in range(1, len(grid)):
        if ks[i] == ks[i - 1]:
            continue
        a, b = grid[i - 1], grid[i]                               # order(a) = ks[i-1], order(b) = ks[i]
        while np.nextafter(a, F32(1)) < b:
            m = F32(0.5) * (a + b)
            if order(m, fam) == ks[i - 1]:
                a = m
            else:
                assert order(m, fam) == ks[i], "the rule is not monotone"
                b = m
        out[ks[i - 1]][1] = float(a)
        assert ks[i] not in out, "the rule is not monotone"
        out[ks[i]] = [float(b), None]
    out[ks[-1]][1] = np.inf
    return {k: (v[0], v[1]) for k, v in out.items()}


def reachable(fam_name):
    """The orders the family's rule can select, in ascending bound."""
    return list(bands(fam_name).keys())


# ---- targets --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Target:
    label: str
    bound: float
    orders: tuple          # the admissible orders: one inside a band, the two neighbours at an edge point
    pin: bool = False      # the point that pins its order: 0.9 x the band's upper edge, where a series cut at K // 2 must show

    @property
    def edge(self):
        return len(self.orders) > 1


@lru_cache(maxsize=None)
def targets(fam_name, edges=True, pivoted=True, cap=None):
    """Per reachable series order one bound at 0.9 x the band's upper edge and one at 1.1 x its lower edge (order 1 has no lower
    edge: 0.01 x the upper one), the pivoted bounds 0.31, 0.5, 0.9, and two edge points at every edge between two series orders.
    The edge at 0.3 is left out (vsm_device_status counts the pivoted inverses exactly).  cap: drop bounds above it."""
    b = bands(fam_name)
    if FAMILIES[fam_name].sel is None:      # no rule: bounds across the range, every one through the pivoted inverse
        out = [Target("bound %.0e" % x, x, (PIVOT,)) for x in (1e-6, 1e-3, 0.015) + (PIVOT_TARGETS if pivoted else ())]
        return tuple(t for t in out if cap is None or t.bound <= cap)
    ser = [k for k in b if k != PIVOT]
    out = []
    for i, K in enumerate(ser):
        lo, hi = b[K]
        hi = min(hi, 0.3)
        out.append(Target("K%d hi" % K, 0.9 * hi, (K,), True))
        out.append(Target("K%d lo" % K, 1.1 * lo if lo > 0 else 0.01 * hi, (K,)))
        if edges and i + 1 < len(ser):
            nxt = ser[i + 1]
            out.append(Target("K%d|K%d -" % (K, nxt), hi * (1 - EDGE_OFFSET), (K, nxt)))
            out.append(Target("K%d|K%d +" % (K, nxt), hi * (1 + EDGE_OFFSET), (K, nxt)))
    if pivoted and PIVOT in b:
        out += [Target("pivoted %.2f" % x, x, (PIVOT,)) for x in PIVOT_TARGETS]
    if cap is not None:
        out = [t for t in out if t.bound <= cap]
    return tuple(out)


def shuffled(tg, seed):
    """The targets in a fixed random order: neighbouring points of a batch take different orders."""
    idx = np.random.default_rng(seed).permutation(len(tg))
    return tuple(tg[i] for i in idx)


# ---- inverses -------------------------------------------------------------------------------------------------------------------
def inv_newton(E):
    """(I - E)^-1 in long double: three Newton steps X <- X + X (I - (I - E) X) from the float64 inverse."""
    E = np.asarray(E, dtype=LD)
    I = np.eye(E.shape[-1], dtype=LD)
    A = I - E
    X = np.linalg.inv(A.astype(F64)).astype(LD)
    for _ in range(3):
        X = X + X @ (I - A @ X)
    return X


def series(E, degree):
    """sum_{k <= degree} E^k by Horner, in E's type (E: one matrix or a batch)."""
    I = np.eye(E.shape[-1], dtype=E.dtype)
    G = I + E if degree >= 1 else np.broadcast_to(I, E.shape).copy()
    for _ in range(degree - 1):
        G = (I + E @ G).astype(E.dtype)
    return G


def inv_by_orders(E, orders, degree_of=lambda K: K):
    """Per point s: Horner of degree degree_of(orders[s]), np.linalg.inv of I - E where orders[s] is PIVOT; in E's type."""
    out = np.empty_like(E)
    I = np.eye(E.shape[-1], dtype=E.dtype)
    for s, K in enumerate(orders):
        if K == PIVOT:
            out[s] = np.linalg.inv(I - E[s]) if E.dtype != LD else inv_newton(E[s])
        else:
            out[s] = series(E[s], degree_of(K))
    return out


# ---- the steps ------------------------------------------------------------------------------------------------------------------
def _mv(A, v):
    return np.einsum("sij,sj->si", A, v)


def interaction_step(comp, add, T, inv):
    """interaction!(::ScatteringInterface_11) (interaction.jl:207-266) in type T with ONE inverse, G2 = inv(R+- r-+), and the
    push-through identities (I - r R)^-1 r = r G2, (I - r R)^-1 = I + r G2 R -- the form every kernel family evaluates; each
    term is a product of nonnegative matrices.  Returns (outputs, E)."""
    c = {k: np.asarray(v, dtype=T) for k, v in comp.items()}
    a = {k: np.asarray(v, dtype=T) for k, v in add.items()}
    E = (c["R_pm"] @ a["r_mp"]).astype(T)
    G2 = np.asarray(inv(E), dtype=T)
    Z = c["R_pm"] @ a["t_mm"]
    z = c["J0_p"] + _mv(c["R_pm"], a["j0_m"])
    T21 = a["t_pp"] @ G2
    Y = (c["T_mm"] @ a["r_mp"]) @ G2
    out = dict(R_pm=a["r_pm"] + T21 @ Z, T_pp=T21 @ c["T_pp"], J0_p=a["j0_p"] + _mv(T21, z),
               R_mp=c["R_mp"] + Y @ c["T_pp"], T_mm=c["T_mm"] @ a["t_mm"] + Y @ Z,
               J0_m=c["J0_m"] + _mv(c["T_mm"], a["j0_m"]) + _mv(Y, z))
    return {k: np.asarray(v, dtype=T) for k, v in out.items()}, E


def doubling_step(lay, T, inv):
    """One step of doubling! (rt_helpers.jl:102-166) for n_stokes = 1 in type T: lay = dict(r_mp, t_pp, j0_p, j0_m, expk).
    Returns (the layer after the step, E = r r)."""
    r, t, jp, jm, ek = (np.asarray(lay[k], dtype=T) for k in ("r_mp", "t_pp", "j0_p", "j0_m", "expk"))
    E = (r @ r).astype(T)
    G = np.asarray(inv(E), dtype=T)
    tt = t @ G
    j1p, j1m = jp * ek[:, None], jm * ek[:, None]
    out = dict(j0_m=jm + _mv(tt, j1m + _mv(r, jp)), j0_p=j1p + _mv(tt, jp + _mv(r, j1m)), r_mp=r + tt @ r @ t, t_pp=tt @ t,
               expk=ek * ek)
    return {k: np.asarray(v, dtype=T) for k, v in out.items()}, E


# ---- input builders -------------------------------------------------------------------------------------------------------------
def _refl(rng, S, N):
    return rng.random((S, N, N)) / N


def _trans(rng, S, N):
    return np.eye(N)[None] * rng.uniform(0.3, 0.95, (S, N, 1)) + 0.05 * rng.random((S, N, N)) / N


def _land(fam, make_E, apply, tg, power):
    """Rescale one factor per point until the family's bound on E sits on the targets (E is of degree `power` in that factor)."""
    want = np.array([t.bound for t in tg])
    for _ in range(4):
        b = bound(make_E(), fam).astype(F64)
        apply((want / b) ** (1.0 / power))
    return bound(make_E(), fam).astype(F64)


def interaction_inputs(fam_name, N, tg, seed, add=None):
    """A general added layer and a composite, random and nonnegative, in the family's array type; R+- of point s is rescaled so
    that the family's bound on E = R+- r-+ lands on tg[s].bound.  add: an added layer given by the caller (the native run's
    elemental layer) instead of the random one.  Returns (comp, add, bounds)."""
    fam = FAMILIES[fam_name]
    rng = np.random.default_rng(seed)
    S = len(tg)
    io = fam.io
    comp = dict(R_mp=_refl(rng, S, N), R_pm=_refl(rng, S, N), T_pp=_trans(rng, S, N), T_mm=_trans(rng, S, N),
                J0_p=rng.random((S, N)), J0_m=rng.random((S, N)))
    if add is None:
        add = dict(r_mp=_refl(rng, S, N), t_pp=_trans(rng, S, N), r_pm=_refl(rng, S, N), t_mm=_trans(rng, S, N),
                   j0_p=rng.random((S, N)), j0_m=rng.random((S, N)))
    comp = {k: v.astype(io) for k, v in comp.items()}
    add = {k: np.asarray(v).astype(io) for k, v in add.items()}

    def rescale(f):
        comp["R_pm"] = (comp["R_pm"].astype(F64) * f[:, None, None]).astype(io)
    b = _land(fam, lambda: comp["R_pm"].astype(fam.arith) @ add["r_mp"].astype(fam.arith), rescale, tg, 1)
    return comp, add, b


def dsym_added(add):
    """The D-symmetric form of an added layer with D = I (n_stokes 1 and 2 have no U / V rows): r+- = r-+, t-- = t++."""
    return dict(add, r_pm=add["r_mp"].copy(), t_mm=add["t_pp"].copy())


def doubling_inputs(fam_name, N, tg, seed):
    """An added layer (n_stokes = 1) whose r-+ is rescaled per point so that the bound on E = r r lands on the targets."""
    fam = FAMILIES[fam_name]
    rng = np.random.default_rng(seed)
    S = len(tg)
    io = fam.io
    lay = dict(r_mp=_refl(rng, S, N), t_pp=_trans(rng, S, N), j0_p=rng.random((S, N)), j0_m=rng.random((S, N)),
               expk=rng.uniform(0.5, 0.99, S))
    lay = {k: v.astype(io) for k, v in lay.items()}

    def rescale(f):
        lay["r_mp"] = (lay["r_mp"].astype(F64) * f[:, None, None]).astype(io)
    b = _land(fam, lambda: (lambda r: r @ r)(lay["r_mp"].astype(fam.arith)), rescale, tg, 2)
    return lay, b


# ---- reference, own-precision restatement, mutant -------------------------------------------------------------------------------
def selected(E, fam_name):
    """(bounds, orders) of the restated rule on a batch E in the family's arithmetic."""
    b = bound(E, fam_name)
    return b.astype(F64), [order(x, fam_name) for x in b]


def relerr(got, ref):
    """max over the elements of |got - ref| / |ref|, per point (the references here have no zero element)."""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    e = np.abs(got - ref) / np.abs(ref)
    return np.asarray(e.reshape(e.shape[0], -1).max(axis=1), dtype=F64)


def tolerance(err_own, io):
    """tol = max(6 err_own, 32 eps): 6 covers another summation order, FMA and the MFMA's four-wide k-steps for an error of the
    same statistical size as the own-precision restatement's -- a margin over the reference's evaluation, never over a kernel."""
    return np.maximum(6.0 * np.asarray(err_own), 32.0 * float(np.finfo(io).eps))


def _own_inv(fam, tg, record, side):
    """The inverse of the own-precision restatement: the rule's order on the restatement's own E; at an edge point (tg given: the
    first step) the lower (side 0) or the higher (side 1) of the two admissible orders."""
    def inv(E):
        b, ks = selected(E, fam.name)
        record.append((b, list(ks)))
        if tg is not None:
            ks = [t.orders[side] if t.edge else k for t, k in zip(tg, ks)]
        return inv_by_orders(E, ks)
    return inv


def _sides(tg):
    return (0, 1) if any(t.edge for t in tg) else (0,)


def _mutant_inv(ks):
    return lambda E: inv_by_orders(np.asarray(E, dtype=LD), ks, degree_of=lambda K: K // 2)


def _pick(d, idx):
    return {k: v[idx] for k, v in d.items()}


def _finish(fam, ref, owns, own_sel, names):
    io = fam.io                                                            # (.astype(io): what the kernel stores)
    err_own = np.max([relerr(own[k].astype(io), ref[k]) for own in owns for k in names], axis=0)
    return dict(ref=ref, err_own=err_own, tol=tolerance(err_own, io), sel=own_sel)


def _mutant_error(res, tg, names, step):
    """err_mut[s] at the pins (NaN elsewhere): the step evaluated in long double on the pins alone, their series cut at K // 2."""
    idx = [s for s, t in enumerate(tg) if t.pin and res["sel"][0][1][s] != PIVOT]
    err = np.full(len(tg), np.nan)
    if idx:
        mut = step(idx, _mutant_inv([res["sel"][0][1][s] for s in idx]))
        err[idx] = np.max([relerr(mut[k], res["ref"][k][idx]) for k in names], axis=0)
    res["err_mut"] = err


def interaction_case(fam_name, N, tg, seed, dsym=False, with_mutant=True, add=None):
    """Inputs, long-double reference, own-precision restatement, tolerance and mutant error of one interaction batch.
    Returns dict(comp, add, bounds, ref, err_own, tol, err_mut, sel) -- per point where it applies; sel: per step the
    restatement's (bounds, orders).  At edge points err_own is the larger of the two admissible orders' errors."""
    fam = FAMILIES[fam_name]
    comp, add, b = interaction_inputs(fam_name, N, tg, seed, add)
    if dsym:
        add = dsym_added(add)
    ref, _ = interaction_step(comp, add, LD, inv_newton)
    rec = []
    owns = [interaction_step(comp, add, fam.arith, _own_inv(fam, tg, rec, side))[0] for side in _sides(tg)]
    res = _finish(fam, ref, owns, rec[:1], IA_OUT)
    if with_mutant:
        _mutant_error(res, tg, IA_OUT, lambda idx, inv: interaction_step(_pick(comp, idx), _pick(add, idx), LD, inv)[0])
    res.update(comp=comp, add=add, bounds=b)
    return res


def doubling_case(fam_name, N, tg, seed, ndoubl=1, with_mutant=True):
    """The same for ndoubl doubling steps; the mutant cuts the series of the FIRST step.  sel: per step (bounds, orders)."""
    fam = FAMILIES[fam_name]
    lay, b = doubling_inputs(fam_name, N, tg, seed)
    recs, owns = [], []
    for side in _sides(tg):
        rec, own = [], lay
        for n in range(ndoubl):
            own, _ = doubling_step(own, fam.arith, _own_inv(fam, tg if n == 0 else None, rec, side))
        recs.append(rec)
        owns.append(own)

    def steps(x, first_inv):
        for n in range(ndoubl):
            x, _ = doubling_step(x, LD, first_inv if n == 0 else inv_newton)
        return x
    res = _finish(fam, steps(lay, inv_newton), owns, recs[0], DBL_OUT)
    if with_mutant:
        _mutant_error(res, tg, DBL_OUT, lambda idx, inv: steps(_pick(lay, idx), inv))
    res.update(lay=lay, bounds=b)
    return res


def pivot_count_range(sel):
    """(fewest, most) pivoted inverses the kernels may count for the recorded (bounds, orders) of every step: a bound within 2 %
    of 0.3 may fall on either side in the kernel's own summation order."""
    lo = sum(int(np.sum(b >= 0.3 * 1.02)) for b, _ in sel)
    hi = sum(int(np.sum(b >= 0.3 * 0.98)) for b, _ in sel)
    return lo, hi


def pinned(fam_name):
    """A family whose cut series show in its outputs.  k_ia128<float> / k_dbl128<float> select by the FP64 tolerance and store
    Float32: the rule takes every series to eps(Float64), so a series cut at half its degree is still right to far below
    eps(Float32) (the largest such error, order 31 cut at 15, is 0.3^16 = 4e-9): their cases assert the result, no order."""
    fam = FAMILIES[fam_name]
    return fam.sel is not None and not (fam.sel is F64 and fam.io is F32)


# ---- what runs on the GPU (shared with the CPU checks: every case used there is checked here) -----------------------------------
# interaction_ : (family, N, n_stokes, D-symmetric); n_stokes is the d_symmetric argument of the D-symmetric layers (D = I for 1, 2)
IA_CASES = ([("native64", N, ns, False) for N, ns in ((13, 1), (16, 4), (33, 3), (47, 1), (60, 3), (64, 4))]
            + [("native64", 30, 1, True), ("native64", 64, 2, True)]
            + [("strip128", N, ns, False) for N, ns in ((65, 1), (80, 4), (96, 3), (97, 1), (112, 4), (128, 4))]
            + [("fused32", 16, 1, False), ("fused32", 60, 1, False), ("fused32", 60, 2, True)]
            + [("strip32", N, 1, False) for N in (65, 78, 80, 96)] + [("strip32", 78, 2, True), ("strip32", 96, 1, True)]
            + [("strip128_f32", 97, 1, False), ("strip128_f32", 128, 1, False)])
# doubling_ : (family, N, ndoubl) -- vsm_doubling reaches k_dbl128 (FP64: 65..128, Float32: 97..128) and the operator-level chain
DBL_CASES = [(f, N, nd) for f, N in (("oplevel64", 48), ("strip128", 65), ("strip128", 96), ("strip128", 128), ("oplevel32", 96),
                                     ("strip128_f32", 128)) for nd in (1, 3)]
DBL3_CAP = 0.125       # ndoubl = 3: first bounds up to here (E about doubles per step: the third step stays a contraction)
# the native run's layer kernels: (family, rows) of a Stokes_I model with one viewing angle
LAYER_CASES = [("native64", n) for n in (16, 40, 64, 79, 96)] + [("native32", n) for n in (60, 65, 80, 96, 112, 128)]
# the reference-layout layer kernels behind vsm_layer_forward: k_layer_strip (FP64, 33..64 rows), k_layer_strip32 (Float32, 65..96)
FORWARD_CASES = [("strip64", 40), ("strip64", 64), ("strip32", 78), ("strip32", 80), ("strip32", 96)]
LAYER_DTAU, LAYER_VARPI, LAYER_DEPOL = 0.05, 0.999, 0.03   # the thin Rayleigh layer of LAYER_CASES (one elemental step, ndoubl = 0)
LAYER_SZA, LAYER_VZA = 40.0, 30.0


def l_trunc_for(rows, nquad_of):
    """The l_trunc whose quadrature (Gauss-Legendre nodes + the viewing and solar streams) has `rows` nodes."""
    return next(l for l in range(1, 4 * rows) if nquad_of(l) == rows)


def ia_seed(N, ns, dsym):
    return 1000 * N + 10 * ns + int(dsym)


@lru_cache(maxsize=None)
def ia_case(fam_name, N, ns, dsym, with_mutant=False):
    tg = shuffled(targets(fam_name), ia_seed(N, ns, dsym))
    return tg, interaction_case(fam_name, N, tg, ia_seed(N, ns, dsym), dsym=dsym, with_mutant=with_mutant)


@lru_cache(maxsize=None)
def dbl_case(fam_name, N, nd, with_mutant=False):
    tg = shuffled(targets(fam_name, nd == 1, nd == 1, DBL3_CAP if nd > 1 else None), 7 * N + nd)     # (ndoubl = 3: no edge points)
    return tg, doubling_case(fam_name, N, tg, 7 * N + nd, ndoubl=nd, with_mutant=with_mutant)


def layer_case(fam_name, n, add1, with_mutant=False, tg=None):
    """A layer kernel's interaction step on n rows: add1 = the elemental added layer of ONE point (dict of [n,n] / [n] arrays), the same
    for every point of the batch; the imported composite is random, its R+- rescaled per point."""
    tg = shuffled(targets(fam_name), 31 * n) if tg is None else tg
    add = {k: np.broadcast_to(np.asarray(v), (len(tg),) + np.shape(v)).copy() for k, v in add1.items()}
    return tg, interaction_case(fam_name, n, tg, 31 * n, with_mutant=with_mutant, add=add)


# ---- two points per workgroup: every ordered pair of branches -------------------------------------------------------------------
def pair_targets(fam_name):
    """Batch A: for every ordered pair (Ka, Kb) of the family's branches two adjacent points (0.9 x the band's upper edge; the
    pivoted branch at 0.5), then one lone trailing point.  Returns (targets, perm): batch B = batch A's points in the order
    perm, where every point shares its pair with a point of its own order (each order occurs an even number of times)."""
    b = bands(fam_name)
    one = {K: (Target("pivoted", 0.5, (PIVOT,)) if K == PIVOT else Target("K%d" % K, 0.9 * min(b[K][1], 0.3), (K,), True)) for K in b}
    tg, seen = [], set()
    for Ka in b:
        for Kb in b:
            for K in (Ka, Kb):        # (the first occurrence of an order is the pin: one mutant evaluation per order)
                tg.append(one[K] if K not in seen else Target(one[K].label, one[K].bound, one[K].orders))
                seen.add(K)
    perm = sorted(range(len(tg)), key=lambda s: (list(b).index(tg[s].orders[0]), s))
    last = one[list(b)[len(b) // 2]]
    return tuple(tg) + (last,), np.array(perm + [len(tg)])


# ---- persistent workgroups: one workgroup walks through every branch ------------------------------------------------------------
def persistent_plan(fam_name, grid, rounds=None):
    """Which distinct point (index into the family's branches, one point per branch) the batch point s takes when `grid` persistent
    workgroups walk a batch of rounds x grid points (workgroup w takes s = w, w + grid, ...): the j-th point of workgroup w is
    branch seq[(w + j d_w) mod L], d_w one of the strides coprime to L -- pivoted -> order 1 -> the longest series is part of seq."""
    ks = list(bands(fam_name))
    ser = [k for k in ks if k != PIVOT]
    seq = [PIVOT, ser[0], ser[-1]] + [k for pair in zip(ser[1:-1], reversed(ser[1:-1])) for k in pair][:len(ser) - 2]
    assert sorted(seq) == sorted(ks)
    L = len(seq)
    rounds = L if rounds is None else rounds
    strides = [d for d in range(1, L) if np.gcd(d, L) == 1]
    s = np.arange(rounds * grid)
    w, j = s % grid, s // grid
    d = np.array(strides)[w % len(strides)]
    return seq, np.array([ks.index(k) for k in seq])[(w + j * d) % L]
