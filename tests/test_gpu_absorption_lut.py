"""GPU tests of Absorption.InterpolationModel (csrc/vsm_absorption_lut.hip) against tests/absorption_lut_oracle.py.

Tables are synthetic and seeded: positive, over six decades, with one-node peaks, so the cubic interpolant overshoots and goes
negative between nodes -- a relative bound would be meaningless; every bound below is absolute and made of the terms of the sum.

    prefilter     |device - long double oracle| <= 10 floor max|y|, floor = max(max|c64 - c_ld| / max|y|, 1e-14) from the oracle alone
                  (the convention of test_gpu_absorption.py)
    evaluation    on GIVEN coefficients: |device - long double oracle| <= 128 2^-53 sum |w_abc C_abc| per point -- a 64-term sum,
                  three weight products per term and a few ulp in each axis's weights -- and the same pattern of exact zeros
    planes        the same bound with the derivative weights over the step
    FP32          the oracle on the rounded coefficients within the evaluation bound; at most 2^-24 sum |w C| from the FP64 model
Measured maxima are printed (DESIGN 4.27 quotes them)."""
import functools

import numpy as np
import pytest
import torch

import absorption_cases as AC
import absorption_lut_oracle as LO
import absorption_oracle as AO

pytestmark = pytest.mark.gpu

EVAL = 128 * 2.0 ** -53


def _lib():
    import vsmartmom_jl_amd as v
    return v._lib.lib()


CHUNK, SPAN = 32, 1024               # test_constants_are_the_exported_ones pins them to the loaded library
NNU = (2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)
NPT = ((2, 2), (3, 4), (5, 2), (2, 4), (3, 2), (5, 4))


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU()


def test_constants_are_the_exported_ones(vsm):
    assert _lib().vsm_absorption_lut_chunk() == CHUNK and _lib().vsm_absorption_lut_span() == SPAN


# ---- tables, axes, grids, layers ---------------------------------------------------------------------------------------------------------
def _axes(nNu, nP, nT):
    return [(6000.0, 0.25, nNu), (250.0, 1000.0 / (nP - 1), nP), (320.0, -140.0 / (nT - 1), nT)]       # (T descending)


@functools.lru_cache(maxsize=None)
def _values(nNu, nP, nT):
    """[nν, nP, nT]: a smooth floor near 1e-26 times a smooth (p, T) factor, and one-node peaks up to 1e-20."""
    rng = np.random.default_rng(1000 * nNu + 10 * nP + nT)
    y = 1e-26 * (1.0 + rng.uniform(0.0, 1.0, (nNu, 1, 1))) * (1.0 + 0.3 * np.arange(nP)[None, :, None]) * (1.0 + 0.2 * np.arange(nT))
    peaks = rng.choice(nNu, size=max(1, nNu // 8), replace=False)
    y[peaks] *= 10.0 ** rng.uniform(3.0, 6.0, (len(peaks), 1, 1)) * rng.uniform(0.5, 1.5, (len(peaks), nP, nT))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _coefficients(nNu, nP, nT):
    """(c64, c_ld, floor) of the oracle's prefilter."""
    y = _values(nNu, nP, nT)
    c64, cld = LO.prefilter(y, np.float64), LO.prefilter(y, np.longdouble)
    floor = max(float(np.max(np.abs(c64 - cld)) / np.max(y)), 1e-14)
    c64.setflags(write=False)
    return c64, cld, floor


def _grids(nNu, seed):
    """name -> evaluation grid; nSpec = nν, 1000, 1, 255, 257, 256 and the 7th nodes."""
    rng = np.random.default_rng(seed)
    first, step, n = _axes(nNu, 2, 2)[0]
    nodes, last = first + step * np.arange(n), first + step * (n - 1)
    fine = np.sort(rng.uniform(first, last, 1000))
    inside = rng.uniform(first, last, 257)
    ends = np.concatenate([[first - 1e-9, first, last, last + 1e-9, first - 40.0, last + 40.0], rng.uniform(first - 1.0, last + 1.0, 250)])
    return {"own axis": nodes, "finer": fine, "every 7th node": nodes[::7], "descending": np.sort(inside[:255])[::-1].copy(),
            "shuffled": inside, "ends and outside": ends, "one point": np.array([0.5 * (first + last)])}


def _layers(nP, nT):
    """(p, T) [3]: exactly (first, first), exactly (last, last), the interior of a cell; and [1]: a node (interior if there is one)."""
    (_, _, _), (p0, dp, _), (t0, dt, _) = _axes(2, nP, nT)
    pl, tl = p0 + dp * (nP - 1), t0 + dt * (nT - 1)
    three = np.array([p0, pl, p0 + 0.37 * dp]), np.array([t0, tl, t0 + (nT - 1 - 0.81) * dt])
    one = np.array([p0 + dp * ((nP - 1) // 2)]), np.array([t0 + dt * (nT // 2)])
    return three, one


def _model(vsm, arch, coef, axes, interp, storage=np.float64):
    A = vsm.Absorption
    return A.InterpolationModel.from_coefficients(coef, 2, 1, *[A.UniformRange(*a) for a in axes], interp_type=interp,
                                                  storage_type=storage, architecture=arch)


def _check(got, ref, mag, what, worst):
    """|got - ref| <= EVAL mag per point, the same exact zeros; the largest ratio goes into worst[what]."""
    assert got.shape == ref.shape, what
    assert np.array_equal(got == 0, np.asarray(ref == 0)), what
    err, lim = np.abs(got - ref).astype(np.float64), (EVAL * mag).astype(np.float64)
    ratio = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0))) if err.size else 0.0
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), ratio)
    assert np.all(err <= lim), "%s: max |device - oracle| / (128 2^-53 sum |w C|) = %.3f" % (what, ratio)


# ---- prefilter ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nNu", NNU)
def test_prefilter_against_oracle(vsm, arch, nNu):
    A = vsm.Absorption
    worst = 0.0
    for nP, nT in NPT:
        y, axes = _values(nNu, nP, nT), [A.UniformRange(*a) for a in _axes(nNu, nP, nT)]
        c64, cld, floor = _coefficients(nNu, nP, nT)
        m = A.InterpolationModel.from_values(y, 2, 1, *axes, architecture=arch)
        assert m.resident and m.coefficients.shape == (nNu + 2, nP + 2, nT + 2) and m.coefficients.dtype == np.float64
        dev = float(np.max(np.abs(m.coefficients - cld)) / np.max(y))
        worst = max(worst, dev / floor)
        assert dev <= 10 * floor, (nP, nT, dev, floor)
        amp = float(np.max(np.abs(cld)) / np.max(y))
        assert amp <= 27.0                                                                 # 3 per axis
        again = A.InterpolationModel.from_values(y, 2, 1, *axes, architecture=arch)
        assert np.array_equal(again.coefficients, m.coefficients)
        m32 = A.InterpolationModel.from_values(y, 2, 1, *axes, storage_type=np.float32, architecture=arch)
        assert m32.coefficients.dtype == np.float32 and np.array_equal(m32.coefficients, m.coefficients.astype(np.float32))
    print("lut prefilter nNu = %d: max deviation / floor = %.2f" % (nNu, worst))


def test_cubic_interpolant_of_these_tables_goes_negative():
    ev = LO.evaluate(_coefficients(NNU[-1], 3, 4)[0], *_axes(NNU[-1], 3, 4), _grids(NNU[-1], 5)["finer"], 600.0, 250.0)
    assert ev["sigma"].min() < 0 < ev["sigma"].max()


# ---- evaluation and linearized planes on given coefficients --------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("interp", ["cubic", "linear"])
@pytest.mark.parametrize("nNu", NNU)
def test_evaluation_and_planes_against_oracle(vsm, arch, nNu, interp, storage):
    A = vsm.Absorption
    cubic = interp == "cubic"
    worst = {}
    for nP, nT in NPT[NNU.index(nNu) % 2::2]:                      # three (nP, nT) per size; every pair over the sizes
        axes = _axes(nNu, nP, nT)
        coef = (_coefficients(nNu, nP, nT)[0] if cubic else _values(nNu, nP, nT)).astype(storage)
        m = _model(vsm, arch, coef, axes, interp, storage)
        m64 = _model(vsm, arch, coef.astype(np.float64), axes, interp) if storage is np.float32 else None
        for (p, T) in _layers(nP, nT):
            for name, grid in _grids(nNu, 7 * nNu + nP).items():
                ref = LO.evaluate(coef, *axes, grid, p, T, cubic, np.longdouble)
                sig = A.compute_absorption_cross_section(m, grid, p, T)
                sig2, dot = A.compute_absorption_cross_section_lin(m, grid, p, T)
                what = "%s %d x %d x %d, Nz = %d, %s" % (interp, nNu, nP, nT, len(p), name)
                _check(sig, ref["sigma"], ref["mag"], "sigma: " + what, worst)
                _check(dot[0], ref["dT"], ref["mag_dT"], "dT: " + what, worst)
                _check(dot[1], ref["dp"], ref["mag_dp"], "dp: " + what, worst)
                assert np.array_equal(sig2, sig) and np.all(dot[2] == 0), what
                assert np.array_equal(A.compute_absorption_cross_section(m, grid, p, T), sig), what
                if len(p) > 1:                                     # the layers of a profile against single-layer (scalar) calls
                    for z in range(len(p)):
                        one = A.compute_absorption_cross_section(m, grid, float(p[z]), float(T[z]))
                        assert one.shape == (len(grid),) and np.array_equal(one, sig[z]), (what, z)
                if m64 is not None:                                # coefficients rounded to FP32: the same, exactly, in FP64 storage
                    assert np.array_equal(A.compute_absorption_cross_section(m64, grid, p, T), sig), what
    print("lut eval %s nNu = %d %s: max |device - oracle| / bound: %s" % (
        interp, nNu, np.dtype(storage).name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_fp32_storage_is_within_half_an_fp32_ulp_of_the_terms(vsm, arch, interp):
    A = vsm.Absorption
    nNu, nP, nT = NNU[-1], 3, 4
    axes, cubic = _axes(nNu, nP, nT), interp == "cubic"
    coef = _coefficients(nNu, nP, nT)[0] if cubic else _values(nNu, nP, nT)
    m64, m32 = _model(vsm, arch, coef, axes, interp), _model(vsm, arch, coef, axes, interp, np.float32)
    assert m32.coefficients.dtype == np.float32
    (p, T), _ = _layers(nP, nT)
    grid = _grids(nNu, 3)["finer"]
    mag = LO.evaluate(coef, *axes, grid, p, T, cubic, np.longdouble)["mag"].astype(np.float64)
    d = np.abs(A.compute_absorption_cross_section(m32, grid, p, T) - A.compute_absorption_cross_section(m64, grid, p, T))
    print("lut FP32 storage %s: max difference / (2^-24 sum |w C|) = %.3f" % (interp, np.max(d / (2.0 ** -24 * mag))))
    assert d.max() > 0 and np.all(d <= 2.0 ** -24 * mag)


# ---- the two paths of the evaluation kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_grids_wider_than_the_staged_span_take_the_direct_path_with_the_same_bits(vsm, arch, interp):
    """nν = 2 SPAN + 500: 256 points on every 7th node, or shuffled ones, span more than SPAN columns (direct gathers); a sorted fine
    grid stays below it (staged in LDS), and the first 256 nodes span SPAN / 4 + 3.  Points are independent: a permutation of the
    grid permutes the result, bit for bit, whichever path a point lands on; SPAN - 3 .. SPAN + 1 columns straddle the threshold."""
    A = vsm.Absorption
    nNu, nP, nT = 2 * SPAN + 500, 3, 2
    cubic, pad = interp == "cubic", 2 if interp == "cubic" else 0
    rng = np.random.default_rng(77)
    coef = rng.standard_normal((nNu + pad, nP + pad, nT + pad)) * 10.0 ** rng.uniform(-26, -20, (nNu + pad, 1, 1))
    axes = _axes(nNu, nP, nT)
    m = _model(vsm, arch, coef, axes, interp)
    (p, T), _ = _layers(nP, nT)
    first, step, _ = axes[0]
    nodes = first + step * np.arange(nNu)
    fine = np.sort(rng.uniform(first, nodes[-1], 3000))
    taps = 4 if cubic else 2
    edge = [np.concatenate([[nodes[5]], rng.uniform(nodes[5], nodes[5 + k], 254), [nodes[5 + k] + 0.5 * step]])
            for k in range(SPAN - taps - 2, SPAN - taps + 3)]         # kmax - kmin + taps = SPAN - 2 .. SPAN + 2
    worst = {}
    for name, grid in (("own axis", nodes), ("every 7th node", nodes[::7]), ("finer", fine), ("threshold", np.concatenate(edge))):
        ref = LO.evaluate(coef, *axes, grid, p, T, cubic, np.longdouble)
        sig, dot = A.compute_absorption_cross_section_lin(m, grid, p, T)
        _check(sig, ref["sigma"], ref["mag"], "sigma: " + name, worst)
        _check(dot[0], ref["dT"], ref["mag_dT"], "dT: " + name, worst)
        _check(dot[1], ref["dp"], ref["mag_dp"], "dp: " + name, worst)
        assert np.array_equal(A.compute_absorption_cross_section(m, grid, p, T), sig)
        perm = rng.permutation(len(grid))
        sp, dp_ = A.compute_absorption_cross_section_lin(m, grid[perm], p, T)
        assert np.array_equal(sp, sig[:, perm]) and np.array_equal(dp_, dot[:, :, perm]), name
    print("lut eval %s, both paths: max |device - oracle| / bound: %s" % (interp, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_wavelength_flag_is_the_reversed_wavenumber_result(vsm, arch):
    A = vsm.Absorption
    nNu, nP, nT = NNU[-1], 5, 4
    axes = _axes(nNu, nP, nT)
    m = _model(vsm, arch, _coefficients(nNu, nP, nT)[0], axes, "cubic")
    (p, T), _ = _layers(nP, nT)
    wn = _grids(nNu, 9)["ends and outside"]
    wl = (1e7 / wn)[::-1].copy()
    wn = (1e7 / wl)[::-1].copy()                                    # (what the conversion gives back)
    a, ad = A.compute_absorption_cross_section_lin(m, wl, p, T, wavelength_flag=True)
    b, bd = A.compute_absorption_cross_section_lin(m, wn, p, T)
    assert np.count_nonzero(b) > 0 and np.array_equal(a, b[:, ::-1]) and np.array_equal(ad, bd[:, :, ::-1])
    assert np.array_equal(A.compute_absorption_cross_section(m, wl, p, T, wavelength_flag=True), a)


# ---- make_interpolation_model on the reference's 16-line file ---------------------------------------------------------------------------------
def test_make_interpolation_model_reproduces_the_line_by_line_nodes(vsm, arch, tmp_path):
    """The reference's interpolator testset (test/test_Absorption.jl:162-193) with the line-by-line call in place of HAPI files: at
    every (p_i, T_j) node, on the table's own ν axis, within the prefilter's 10 floor max|y| plus the evaluation bound.  Between
    nodes the error is the method's, not the code's: printed, not asserted."""
    A = vsm.Absorption
    ht = A.read_hitran(AC.GOLDEN_PAR, mol=2, iso=1)
    iso = AC.isotopologues(A)
    nu, pg, tg = A.UniformRange(6286.0, 0.002, 401), A.UniformRange(250.0, 250.0, 5), A.UniformRange(180.0, 35.0, 4 + 1)
    m = A.make_interpolation_model(ht, A.Voigt(), nu, pg, tg, architecture=arch, isotopologues=iso)
    assert (m.mol, m.iso, m.interp_type, m.storage_type, m.resident) == (2, 1, "cubic", np.dtype(np.float64), True)
    hm = A.make_hitran_model(ht, A.Voigt(), architecture=arch, isotopologues=iso)
    ps, Ts = np.repeat(pg.values(), 5), np.tile(tg.values(), 5)
    lbl = A.compute_absorption_cross_section(hm, nu.values(), ps, Ts)                     # [25, 401]
    assert lbl.max() > 0
    got = A.compute_absorption_cross_section(m, nu.values(), ps, Ts)
    y = np.transpose(lbl.reshape(5, 5, 401), (2, 0, 1))
    c64, cld = LO.prefilter(y, np.float64), LO.prefilter(y, np.longdouble)
    floor = max(float(np.max(np.abs(c64 - cld)) / np.max(y)), 1e-14)
    axes = [(a.first, a.step, a.n) for a in (nu, pg, tg)]
    assert m.coefficients.shape == (403, 7, 7)
    dev = float(np.max(np.abs(m.coefficients - cld)) / np.max(y))
    assert dev <= 10 * floor
    mag = LO.evaluate(m.coefficients, *axes, nu.values(), ps, Ts, True, np.longdouble)["mag"].astype(np.float64)
    err = np.abs(got - lbl)
    print("make_interpolation_model: coefficients %.2e of max|y| (floor %.2e); nodes: max |table - line-by-line| / max|y| = %.2e"
          % (dev, floor, err.max() / y.max()))
    assert np.all(err <= 10 * floor * y.max() + EVAL * mag)
    # between the nodes: the interpolation error of the method at this spacing (printed only)
    pm, Tm = pg.values()[:-1] + 125.0, tg.values()[:-1] + 17.5
    mid = nu.values()[:-1] + 0.001
    a, b = A.compute_absorption_cross_section(m, mid, pm, Tm), A.compute_absorption_cross_section(hm, mid, pm, Tm)
    print("make_interpolation_model: between nodes max |table - line-by-line| / max sigma = %.2e" % (np.max(np.abs(a - b)) / b.max()))
    # linear and FP32 builds hold the values themselves; save / load keeps every bit and evaluates the same
    ml = A.make_interpolation_model(ht, A.Voigt(), nu, pg, tg, architecture=arch, isotopologues=iso, interp_type="linear",
                                    storage_type=np.float32)
    assert np.array_equal(ml.coefficients, y.astype(np.float32))
    path = str(tmp_path / "co2.npz")
    A.save_interpolation_model(m, path)
    back = A.load_interpolation_model(path, architecture=arch)
    assert not back.resident and np.array_equal(back.coefficients, m.coefficients)
    assert np.array_equal(A.compute_absorption_cross_section(back, mid, pm, Tm), a) and back.resident
    # a build in blocks of states gives the same table
    cap = A._LUT_WORK_CAP
    try:
        A._LUT_WORK_CAP = 16                                        # one state per vsm_absorption_xsec call
        blocked = A.make_interpolation_model(ht, A.Voigt(), nu, pg, tg, architecture=arch, isotopologues=iso)
    finally:
        A._LUT_WORK_CAP = cap
    assert np.array_equal(blocked.coefficients, m.coefficients)


# ---- profiles ------------------------------------------------------------------------------------------------------------------------------
def _two_gases(vsm, arch):
    A = vsm.Absorption
    t = AC.synthetic_table(41, 70, no_E_share=0.1)
    nNu, nP, nT = NNU[-1], 5, 4
    axes = [(5995.0, 0.6, nNu), (0.1, 300.0, nP), (170.0, 55.0, nT)]                     # covers the grid and AC.P3, AC.T3
    coef = _coefficients(nNu, nP, nT)[0] * 1e-2
    lut = _model(vsm, arch, coef, axes, "cubic")
    vmr_a, vmr_t = 4.1e-4, np.array([0.21, 0.2, 0.19])
    pairs = [(AC.make_model(A, t, vmr=vmr_a, architecture=arch), vmr_a), (lut, vmr_t)]
    return pairs, (t, vmr_a), (coef, axes, vmr_t), np.array([3.1e21, 2.2e23, 1.9e24])


def test_profile_of_a_line_by_line_gas_and_a_table_gas(vsm, arch):
    A = vsm.Absorption
    pairs, (t, vmr_a), (coef, axes, vmr_t), vcd = _two_gases(vsm, arch)
    grid = AC.nonuniform_grid(300, 12)
    tau, dots = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd, lin=True)
    assert np.array_equal(A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd), tau)
    # each gas alone is its own call; the sum on the device is one rounding away from the sum of the two
    tau_a = A.compute_absorption_profile(pairs[:1], grid, AC.P3, AC.T3, vcd)
    tau_t = A.compute_absorption_profile(pairs[1:], grid, AC.P3, AC.T3, vcd)
    assert np.all(np.abs(tau - (tau_a + tau_t)) <= np.spacing(np.abs(tau_a) + np.abs(tau_t)))
    # the table gas against its oracle (the line-by-line gas has test_gpu_absorption.py)
    ev = LO.evaluate(coef, *axes, grid, AC.P3, AC.T3, True, np.longdouble)
    s = (vcd * vmr_t)[:, None]
    lim = (EVAL + 2.0 ** -52) * (ev["mag"] * s).astype(np.float64)                        # and the product with the scale
    assert np.all(np.abs(tau_t.T - (ev["sigma"] * s).astype(np.float64)) <= lim)
    assert np.all(np.abs(dots[1].T - (ev["sigma"] * vcd[:, None]).astype(np.float64))
                  <= (EVAL + 2.0 ** -52) * (ev["mag"] * vcd[:, None]).astype(np.float64))
    assert np.array_equal(dots[0], A.compute_absorption_profile(pairs[:1], grid, AC.P3, AC.T3, vcd, lin=True)[1][0])
    # the sum against the sum of the two oracles: the line-by-line part within test_gpu_absorption.py's 10 floors of its FP64 oracle
    # (11 of the long-double one), the table part within its evaluation bound, and the rounding of the sum
    gas = [(t, AC.ISOTOPOLOGUES, vmr_a, vmr_a)]
    a64 = AO.absorption_profile(gas, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0)[0]
    ald = AO.absorption_profile(gas, grid, AC.P3, AC.T3, vcd, wing_cutoff=5.0, dtype=np.longdouble)[0]
    floor = max(float(np.max(np.abs(a64 - ald)[ald != 0] / ald[ald != 0])), 1e-14)
    want = ald + (ev["sigma"] * s).T
    assert np.all(np.abs(tau - want) <= 11 * floor * np.abs(ald) + lim.T + np.spacing(np.abs(tau)))
    # linearized: the same tau and gas slots, bit for bit; the table adds to dT and dp and has no vmr_self plane
    T_dot = np.vstack([np.eye(3), np.ones((1, 3))])
    r = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd, T_dot=T_dot)
    assert np.array_equal(r.tau_abs, tau) and all(np.array_equal(a, b) for a, b in zip(r.tau_abs_dot, dots))
    assert np.all(r.dtau_dvmr_self[1] == 0) and np.count_nonzero(r.dtau_dvmr_self[0]) > 0
    ra = A.compute_absorption_profile_lin(pairs[:1], grid, AC.P3, AC.T3, vcd)
    rt = A.compute_absorption_profile_lin(pairs[1:], grid, AC.P3, AC.T3, vcd, T_dot=T_dot)
    for both, a, b in ((r.dtau_dT, ra.dtau_dT, rt.dtau_dT), (r.dtau_dp, ra.dtau_dp, rt.dtau_dp)):
        assert np.all(np.abs(both - (a + b)) <= np.spacing(np.abs(a) + np.abs(b)))
    for got, key in ((rt.dtau_dT, "dT"), (rt.dtau_dp, "dp")):
        assert np.all(np.abs(got.T - (ev[key] * s).astype(np.float64)) <= (EVAL + 2.0 ** -52) * (ev["mag_" + key] * s).astype(np.float64))
    assert np.array_equal(rt.tau_abs, tau_t) and np.array_equal(ra.dtau_dvmr_self[0], r.dtau_dvmr_self[0])
    for k in range(3):                                              # the unit-table slots: layer k's own column of dtau_dT
        want = np.zeros((300, 3))
        want[:, k] = r.dtau_dT[:, k]
        assert np.array_equal(r.profile_slots[k], want), k
    assert np.array_equal(r.profile_slots[3], r.dtau_dT)            # T_dot = 1, p_dot = 0: dT 1 + dp 0


def test_table_profile_feeds_rt_run_and_rt_run_lin(vsm, arch):
    """The scene of test_gpu_absorption_lin.py's end-to-end test (nSpec = 64, Nz = 3, Stokes_IQU, Rayleigh) with the table gas:
    rt_run on the model's tau_abs against the run on the oracle's, and rt_run_lin's T-shift slot from lin_model_slots() against
    the run on the oracle's slots, both within the 1e-8 of test_gpu_parity.py."""
    A, H = vsm.Absorption, vsm.host_model
    nNu, nP, nT = NNU[-1], 5, 4
    axes = [(6005.0, 0.4, nNu), (0.1, 300.0, nP), (170.0, 55.0, nT)]
    # a smooth positive table (tau_abs of a radiative-transfer run must not be negative), with a T dependence worth a slot
    y = 1e-22 * (1.2 + np.sin(0.3 * np.arange(nNu)))[:, None, None] * (1.0 + 0.3 * np.arange(nP))[None, :, None] * \
        ((np.arange(nT) + 1.0) ** 2 / 4.0)[None, None, :]
    coef = LO.prefilter(y)
    lut = _model(vsm, arch, coef, axes, "cubic")
    grid = AC.nonuniform_grid(64, 13, lo=6010.0, hi=6040.0)
    vmr, vcd = 4.1e-4, 2.0 * np.array([3.1e21, 2.2e23, 1.9e24])
    r = A.compute_absorption_profile_lin([(lut, vmr)], grid, AC.P3, AC.T3, vcd, T_dot=np.ones((1, 3)))
    slots = r.lin_model_slots()
    assert len(slots) == 2 and r.tau_abs.shape == (64, 3)
    ev = LO.evaluate(coef, *axes, grid, AC.P3, AC.T3, True)
    tau_o = np.ascontiguousarray((ev["sigma"] * (vcd * vmr)[:, None]).T)
    dot_o = np.ascontiguousarray((ev["sigma"] * vcd[:, None]).T)
    dT_o = np.ascontiguousarray((ev["dT"] * (vcd * vmr)[:, None]).T)
    assert tau_o.min() > 0 and 1e-3 < tau_o.sum(axis=1).max() < 5.0
    tau_rayl = np.tile(0.02 * np.array([0.05, 0.25, 0.7]), (64, 1))

    def model(ta):
        return H.model_from_arrays(arch, "IQU", 8, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=ta, depol=0.0279, albedo=0.15, m_max=2)

    R, T = vsm.CoreRT.rt_run(model(r.tau_abs))
    Ro, To = vsm.CoreRT.rt_run(model(tau_o))
    for got, want in ((R, Ro), (T, To)):
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-8
    _, _, Rd, Td = vsm.CoreRTLin.rt_run_lin(model(r.tau_abs), H.LinModel(tau_abs_dot=slots), 0, 2, 1)
    _, _, Rdo, Tdo = vsm.CoreRTLin.rt_run_lin(model(tau_o), H.LinModel(tau_abs_dot=[dot_o, dT_o]), 0, 2, 1)
    assert np.max(np.abs(Rdo[..., 1])) > 0
    for got, want in ((Rd[..., 0], Rdo[..., 0]), (Td[..., 0], Tdo[..., 0]), (Rd[..., 1], Rdo[..., 1]), (Td[..., 1], Tdo[..., 1])):
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-8
