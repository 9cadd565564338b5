"""GPU tests of the pivoted elimination inside the one solve body (level_solve_columns: level_form_system + level_eliminate) of
the fused level kernels of csrc/vsm_level.hip, through seven entry points (radiance and src share a kernel, as do lin and
lin_src): every entry point on inputs whose I - A B has its large entries OFF the diagonal (tests/level_cases.py), so that
almost every step of the Gauss-Jordan elimination exchanges a row -- the wave-0 pivot search with its two ballots (rows 0..63 and
64..127) and first-occurrence rule, the row exchange over ALL columns k .. NC-1 (the right-hand sides included: K sources, the PC
parameter columns of a linearized chunk), and the SINGULAR / NONFINITE bits of vsm_device_status raised by this file.

tests/test_oracle_level_pivoting.py checks on the CPU, for the very arrays used here (level_cases.fixed), that kappa_1(I - A B) <= 10,
that the kernel's pivot rule exchanges a row at N / 2 steps or more (N - 1 in fact) and finds a pivot in a row >= 64 at a step < 64
for N > 64, and that the same elimination without exchange is non-finite (element (0, 0) of the device's system is exactly 0).

Reference: a float64 numpy solve of the same equation from the same (already cast) inputs, through the sibling tests' call helpers
and oracles.  Bound: tol = max(floor, 50 kappa_1 eps(FT)) (test_gpu_parity::test_strip128_pivoted_inverse_near_and_beyond_unit_
spectral_radius), relative to the largest reference value, with `floor` the bound of the sibling test of the same kernel against
numpy (FLOOR below); kappa_1 is computed per case.  S = 3 points everywhere.

Largest error observed on an MI355X (FP64 / FP32; kappa_1 <= 2.4, exact_ties 3.3, so tol = floor everywhere): radiance 5.5e-15 /
3.2e-6, src 4.6e-15 / 2.2e-6, flux 4.7e-16 / 1.4e-7, ie 3.6e-15 / 1.9e-6, lin 3.9e-15 / 7.9e-7, lin_src 3.1e-15, emission 4.0e-14 /
1.4e-5 (DESIGN 4.8 has the table); kernel_pivot_trace reports 127 exchanging steps of 128 at N = 128."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import level_cases as LC  # noqa: E402
import ms_oracle as MS  # noqa: E402
import test_gpu_fluxes as TF  # noqa: E402
import test_gpu_multisensor as TM  # noqa: E402
import test_gpu_multisensor_lin as TL  # noqa: E402
import test_gpu_multisensor_raman as TR  # noqa: E402
import test_gpu_multisensor_thermal as TT  # noqa: E402
import test_gpu_multisensor_thermal_lin as TTL  # noqa: E402
import test_gpu_sif as TS  # noqa: E402

pytestmark = pytest.mark.gpu

S = LC.S_POINTS
F64, F32 = np.float64, np.float32
FTS = pytest.mark.parametrize("FT", [F64, F32], ids=["f64", "f32"])
# the bound of each kernel's sibling test against numpy: test_level_kernel_fused_vs_oplevel / test_level_src_kernel /
# test_level_flux_kernel / test_emission_response_kernel (10 x 1e-12, 10 x 2e-5), test_level_ie_kernel_vs_numpy,
# test_level_kernel_lin_vs_numpy(_fp32), test_level_kernel_lin_src_vs_numpy
FLOOR = {"radiance": (1e-11, 2e-4), "src": (1e-11, 2e-4), "flux": (1e-11, 2e-4), "ie": (1e-10, 5e-4), "lin": (1e-11, 2e-4),
         "lin_src": (1e-11, 2e-4), "emission": (1e-11, 2e-4)}
VZA, VAZ = [0.0, 30.0, 88.0], [0.0, 45.0, 120.0]      # 88 degrees: the last stream of linspace(1, 0.05), a row >= 64 for N > 64
VZA_MAX = 88.0


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


def _rel(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


def _tol(kernel, A, B, FT):
    kappa = LC.kappa1(A, B)
    assert np.isfinite(kappa) and kappa <= 10, kappa
    return LC.tolerance(FLOOR[kernel][0 if FT == F64 else 1], kappa, FT), kappa


def _report(kernel, N, FT, what, err, tol, kappa):
    print("LEVELPIV %-8s N %3d %s %-28s err %.2e tol %.1e kappa_1 %.2f" % (kernel, N, np.dtype(FT).name, what, err, tol, kappa))


def _rows(vsm, pol, qp, vza, vaz, m, weight, full):
    """(S, n, nV): the viewing rows of a level vector [S, N], weighted (vsm_postprocess_vza's rule); and row0."""
    row0, w = vsm.CoreRT._vza_rows_weights(pol, vza, vaz, qp, m, weight, torch.float64)
    nV = len(vza)
    out = np.stack([np.stack([w[v + nV * k] * full[:, row0[v] + k] for v in range(nV)], axis=-1) for k in range(pol.n)], axis=1)
    return out, list(row0)


def _clean(vsm, what):
    vsm._lib.check_device_status(what)
    assert vsm._lib.last_device_status[0] == 0


# ---- vsm_level_radiance_*: fused, and its operator-level twin on the same inputs -----------------------------------------------------
def _radiance(vsm, N, FT, family="pivoting", vza=VZA, vaz=VAZ, ops=(False, True)):
    pol, qp, runs = TM._fused_and_oplevel_calls(vsm, N, FT, vza, vaz, inputs=LC.fixed(family, FT), S=S, ops=ops)
    for shared, (A, a, B, c), outs in runs:
        tol, kappa = _tol("radiance", A, B, FT)
        uwr, dwr = MS.level_push_through(F64, A, a, B, c)
        ur, row0 = _rows(vsm, pol, qp, vza, vaz, 1, 1.0 / math.pi, uwr)
        dr, _ = _rows(vsm, pol, qp, vza, vaz, 1, 1.0 / math.pi, dwr)
        if N > 64:
            assert max(row0) >= 64
        for op, out in zip(ops, outs):
            e = max(_rel(out[2], uwr), _rel(out[3], dwr))
            # (the viewing rows are accumulated into the siblings' non-zero fill, 0.25 / -0.5)
            er = max(_rel(out[0] - 0.25, ur), _rel(out[1] + 0.5, dr))
            _report("radiance", N, FT, "%s %s %s" % (family, "oplevel" if op else "fused", "shared" if shared else "per-point"),
                    max(e, er), tol, kappa)
            assert e <= tol and er <= tol, (N, shared, op, e, er, tol)
            TM._check_vza_rows(vsm, pol, qp, vza, vaz, out, FLOOR["radiance"][0 if FT == F64 else 1] / 10)


@FTS
@pytest.mark.parametrize("N", [2, 3, 17, 63, 65, 127, 128])
def test_level_radiance_pivoting(vsm, N, FT):
    """N = 2, 3: below one MFMA k-step; 17, 63, 65, 127: the k < N guard of the k-loop and a partial 16-row tile; 65, 127, 128: pivots
    in rows >= 64.  Per-point and shared bottom; full vectors and viewing rows, fused and operator level."""
    _radiance(vsm, N, FT)
    _clean(vsm, "level pivoting")


@FTS
def test_level_radiance_pivoting_many_angles(vsm, FT):
    """70 viewing angles at N = 65: full vectors, then vsm_postprocess_vza."""
    _radiance(vsm, 65, FT, vza=list(np.linspace(0.0, VZA_MAX, 70)), vaz=list(np.linspace(0.0, 345.0, 70)))
    _clean(vsm, "level pivoting")


@FTS
@pytest.mark.parametrize("N", [17, 127])
def test_level_radiance_exact_ties(vsm, N, FT):
    """Column 0 carries its largest magnitude twice (rows 1 and N // 2 + 1; 64 at N = 127: one in each ballot), exactly, in both
    precisions: either pivot solves the system."""
    _radiance(vsm, N, FT, family="exact_ties")
    _clean(vsm, "level pivoting")


# ---- vsm_level_radiance_src_* -------------------------------------------------------------------------------------------------------
def _src(vsm, N, FT, n_src, family="pivoting"):
    """Sources of very different magnitude (x1, x1e3, alternating; then the other way round, so that every right-hand-side column
    carries the large one once): a column the exchange skipped shows in the sum."""
    setup = TT._kernel_setup(vsm, N, FT, 3, vza_max=VZA_MAX)
    pol, qp, vza, vaz, dt, dev, lay, vec = setup
    for shared in (False, True):
        for first in (1.0, 1e3):
            scales = tuple(first if k % 2 == 0 else 1e3 / first for k in range(n_src))
            A, tops, B, bots = TT._src_inputs(N, S, np.random.default_rng(N), shared, inputs=LC.fixed(family, FT), scales=scales, FT=FT)
            out = TT._level_src_call(vsm, setup, S, N, 3, lay(A), [vec(x) for x in tops], lay(B), [vec(x) for x in bots])
            vsm._lib.check_device_status("level src pivoting")
            tol, kappa = _tol("src", A, B, FT)
            uwr, dwr = MS.level_push_through(F64, A, sum(tops), B, sum(bots))        # (the equation is linear in (a, c))
            ur, row0 = _rows(vsm, pol, qp, vza, vaz, 1, 1.0 / math.pi, uwr)
            dr, _ = _rows(vsm, pol, qp, vza, vaz, 1, 1.0 / math.pi, dwr)
            assert N <= 64 or max(row0) >= 64
            e = max(_rel(out[2], uwr), _rel(out[3], dwr), _rel(out[0] - 0.25, ur), _rel(out[1] + 0.5, dr))
            _report("src", N, FT, "%s K %d x%g first %s" % (family, n_src, first, "shared" if shared else "per-point"), e, tol, kappa)
            assert e <= tol, (N, n_src, shared, first, e, tol)


@FTS
@pytest.mark.parametrize("n_src", [2, 4])
@pytest.mark.parametrize("N", [17, 65, 128])
def test_level_src_pivoting(vsm, N, FT, n_src):
    assert vsm.core_rt_ms.LEVEL_MAX_SRC == 4
    _src(vsm, N, FT, n_src)
    _clean(vsm, "level pivoting")


# ---- vsm_level_flux_* ---------------------------------------------------------------------------------------------------------------
def _flux(vsm, N, FT, family="pivoting"):
    """K = 2 sources, nW = 2 weight rows, with the direct term; and the A = NULL (TOA) call, which has no system."""
    FL = vsm.core_rt_flux
    K = nW = 2
    for shared in (False, True):
        pol, dt, dev, host, d = TF._kernel_case(vsm, N, FT, S, shared, np.random.default_rng(N), inputs=LC.fixed(family, FT))
        for top in (True, False):
            out = torch.full((3, nW, S), float("nan"), dtype=dt, device=dev)
            FL.level_flux_(pol, d["A"] if top else None, d["a"][:K] if top else None, d["B"] if top else None, d["c"][:K],
                           d["q"][:nW].contiguous(), host["dir_h"][:nW], host["mu0"], d["tau"], d["F0"], out)
            torch.cuda.synchronize()
            vsm._lib.check_device_status("level flux pivoting")
            got = out.cpu().numpy().astype(F64)
            tol, kappa = _tol("flux", host["A"], host["B"], FT)
            ref = TF._kernel_reference(pol, host, K, nW, top, True)
            e = float(np.max(np.abs(got - ref))) / float(np.max(np.abs(ref[:2])))
            _report("flux", N, FT, "%s %s %s" % (family, "level" if top else "TOA", "shared" if shared else "per-point"), e, tol, kappa)
            assert np.all(np.isfinite(got)) and e <= tol, (N, shared, top, e, tol)
            if not top:
                assert np.all(got[1] == 0)


@FTS
@pytest.mark.parametrize("N", [21, 65, 128])
def test_level_flux_pivoting(vsm, N, FT):
    _flux(vsm, N, FT)
    _clean(vsm, "level pivoting")


# ---- vsm_level_radiance_ie_* --------------------------------------------------------------------------------------------------------
def _ie(vsm, N, FT, bottom, family="pivoting"):
    """K = 7 lines with the shifts of tests/test_gpu_raman.py (S = 3: four in band or partly in band, three never); the elastic level
    vectors of the donors are the family's (a, c).  Full vectors and viewing rows (0, the middle stream, N - n)."""
    inputs = LC.fixed(family, FT)
    errs = TR._level_ie_vs_numpy(vsm, FT, N, 7, bottom, 3, inputs=inputs, S=S, shifts=[int(x) for x in TR.SHIFTS])
    A, _, B, _ = inputs(N, S, None, bottom == "shared")
    tol, kappa = _tol("ie", A, B, FT)
    _report("ie", N, FT, "%s %s" % (family, bottom), max(errs), tol, kappa)
    assert max(errs) <= tol, (N, bottom, errs, tol)


@FTS
@pytest.mark.parametrize("bottom", ["per_point", "shared"])
@pytest.mark.parametrize("N", [21, 65, 127])
def test_level_ie_pivoting(vsm, N, FT, bottom):
    _ie(vsm, N, FT, bottom)
    _clean(vsm, "level pivoting")


# ---- vsm_level_radiance_lin_* and _lin_src_* ----------------------------------------------------------------------------------------
def _lin(vsm, N, P, P_top, shared, FT, family="pivoting"):
    """Full derivative vectors and the accumulated viewing rows (row0 = 0 and N - n)."""
    inputs = LC.fixed(family, FT)
    got, ref = TL._kernel_case(vsm, N, P, P_top, shared, S=S, FT=FT, inputs=inputs)
    A, _, B, _ = inputs(N, S, None, shared)
    tol, kappa = _tol("lin", A, B, FT)
    e = max(_rel(g, r) for g, r in zip(got, ref))
    _report("lin", N, FT, "%s P %d P_top %d" % (family, P, P_top), e, tol, kappa)
    assert all(np.all(np.isfinite(g)) for g in got) and e <= tol, (N, P, e, tol)


@pytest.mark.parametrize("N,P,P_top,shared,FT", [(17, 3, 2, True, F64), (65, 17, 16, False, F64), (65, 17, 16, False, F32),
                                                  (128, 13, 12, False, F64)],
                         ids=["n17_f64", "n65_f64", "n65_f32", "n128_two_chunks_f64"])
def test_level_lin_pivoting(vsm, N, P, P_top, shared, FT):
    """(128, 13, 12): FP64 takes 12 slots per chunk, so the second chunk repeats the whole elimination (the same exchanges) with one
    right-hand side; (65, 17): 17 columns ride every exchange."""
    _lin(vsm, N, P, P_top, shared, FT)
    _clean(vsm, "level pivoting")


def test_level_lin_exact_ties(vsm):
    _lin(vsm, 127, 3, 2, False, F64, family="exact_ties")
    _clean(vsm, "level pivoting")


def _lin_src(vsm, N, P, P_top, P_src, shared, family="pivoting"):
    inputs = LC.fixed(family, F64)
    got, ref = TTL._kernel_case(vsm, N, P, P_top, P_src, shared, S=S, inputs=inputs)
    A, _, B, _ = inputs(N, S, None, shared)
    tol, kappa = _tol("lin_src", A, B, F64)
    e = max(_rel(g, r) for g, r in zip(got, ref))
    _report("lin_src", N, F64, "%s P %d P_top %d P_src %d" % (family, P, P_top, P_src), e, tol, kappa)
    assert all(np.all(np.isfinite(g)) for g in got) and e <= tol, (N, P, P_src, e, tol)


@pytest.mark.parametrize("N,P,P_top,P_src,shared", [(21, 3, 2, 2, True), (128, 5, 4, 9, False)], ids=["n21", "n128_boundary_in_sources"])
def test_level_lin_src_pivoting(vsm, N, P, P_top, P_src, shared):
    """(128, 5, 4, 9): 14 slots, 12 per chunk: the chunk boundary lies inside the source-only slots."""
    _lin_src(vsm, N, P, P_top, P_src, shared)
    _clean(vsm, "level pivoting")


@pytest.mark.parametrize("N,P,P_top,shared", [(21, 3, 2, True), (128, 13, 12, False)])
def test_level_lin_src_without_sources_is_the_lin_kernel_bitwise_pivoting(vsm, N, P, P_top, shared):
    """vsm_level_radiance_lin_* launches the source-slot kernel with P_src = 0: an entry point against the kernel it forwards to,
    on pivoting inputs.  The arithmetic is pinned against numpy by test_level_lin_pivoting and test_level_lin_src_pivoting above."""
    inputs = LC.fixed("pivoting", F64)
    a, _ = TTL._kernel_case(vsm, N, P, P_top, 0, shared, S=S, inputs=inputs)
    b, _ = TTL._kernel_case(vsm, N, P, P_top, 0, shared, S=S, inputs=inputs, entry="vsm_level_radiance_lin")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _clean(vsm, "level pivoting")


# ---- vsm_surface_emission_response_* ------------------------------------------------------------------------------------------------
def _emission_inputs(family, FT):
    """(A, B, T) for test_gpu_sif._emission_response_case: the family's operators and that file's transmission block, rounded to FT."""
    def gen(N, S_, rng, shared):
        A, _, B, _ = LC.fixed(family, FT)(N, S_, None, shared)
        T = (np.random.default_rng(N).random((S_, N, N)) * (1.0 / N) + 0.5 * np.eye(N)[None]).astype(FT).astype(F64)
        return A, B, T
    return gen


def _emission(vsm, N, FT, K, family="pivoting"):
    """Viewing rows only (the entry point offers no full vectors): up through T--, dn = the rows of dw."""
    for shared in (False, True):
        res = TS._emission_response_case(vsm, N, FT, K, 3, shared, None, inputs=_emission_inputs(family, FT), S_=S, vza_max=VZA_MAX,
                                         oplevel=False)
        A, B, _ = _emission_inputs(family, FT)(N, S, None, shared)
        tol, kappa = _tol("emission", A, B, FT)
        e = max(_rel(xf, r) for _, _, xf, _, r in res)
        _report("emission", N, FT, "%s K %d %s" % (family, K, "shared" if shared else "per-point"), e, tol, kappa)
        assert all(np.max(np.abs(r)) > 0 for *_, r in res) and e <= tol, (N, K, shared, e, tol)


@FTS
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("N", [16, 61, 128])
def test_emission_response_pivoting(vsm, N, FT, K):
    _emission(vsm, N, FT, K)
    _clean(vsm, "level pivoting")


# ---- the status bits of this file ---------------------------------------------------------------------------------------------------
def _solve_or_zero(solve):
    """numpy's LAPACK solve raises on the exactly singular systems fed below; the helpers' references are not used there."""
    def f(a, b):
        try:
            return solve(a, b)
        except np.linalg.LinAlgError:
            return np.zeros(np.shape(b))       # (every caller passes b with the batch shape of a)
    return f


ENTRY_POINTS = {
    "radiance": lambda vsm, N, fam: _radiance(vsm, N, F64, family=fam, ops=(False,)),
    "src": lambda vsm, N, fam: _src(vsm, N, F64, 2, family=fam),
    "flux": lambda vsm, N, fam: _flux(vsm, N, F64, family=fam),
    "ie": lambda vsm, N, fam: _ie(vsm, N, F64, "per_point", family=fam),
    "lin": lambda vsm, N, fam: _lin(vsm, N, 3, 2, False, F64, family=fam),
    "lin_src": lambda vsm, N, fam: _lin_src(vsm, N, 3, 2, 2, False, family=fam),
    "emission": lambda vsm, N, fam: _emission(vsm, N, F64, 1, family=fam),
}


@pytest.mark.parametrize("N", [17, 128])
@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_level_status_bits(vsm, monkeypatch, entry, N):
    """An exactly zero pivot raises VSM_DEVSTAT_SINGULAR (bit 1), a NaN operand VSM_DEVSTAT_NONFINITE (bit 2) -- flags on finite
    launches, read through check_device_status (which resets them) -- and a well-posed call afterwards is clean and within
    tolerance: test_gpu_parity::test_strip128_inverse_flags_singular_and_nonfinite for the level kernels (fused calls only)."""
    call = ENTRY_POINTS[entry]
    vsm._lib.check_device_status("before the level status test")
    with monkeypatch.context() as m:
        m.setattr(np.linalg, "solve", _solve_or_zero(np.linalg.solve))
        with pytest.raises(vsm.VSMError, match="singular"):
            call(vsm, N, "singular")
        assert vsm._lib.last_device_status[0] & 3 == 1
        with pytest.raises(vsm.VSMError, match="NaN"):
            call(vsm, N, "nonfinite")
        assert vsm._lib.last_device_status[0] & 2
    torch.cuda.synchronize()
    call(vsm, N, "pivoting")
    _clean(vsm, "level pivoting after the flags")
