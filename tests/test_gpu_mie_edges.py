"""GPU tests of vsm_mie_nai2 and vsm_mie_nai2_lin (csrc/vsm_mie.hip) at every tile edge, on inputs whose cut-offs lie below the size
parameter (tests/mie_cases.py): the last kept order of every radius is O(1), so a dropped or doubled order, a mishandled radius of a
partly filled tile or a mishandled angle chunk moves the outputs by 1e-6 and more (tests/test_oracle_mie.py and
tests/test_oracle_mie_lin.py assert that on the CPU, per case, for every radius), while rounding stays at 1e-14 .. 1e-12.
The entry points are called through Scattering.launch_nai2 / launch_nai2_lin on a hand-built MieHostInputs.

Acceptance, per case and output family: |device - oracle64| <= 10 x floor on the family's scale (mie_cases.measure), the floor
being the float64 oracle's own deviation from the long-double oracle over nine realisations (mie_cases.floors; computed on the
CPU, never from the device), at least 1e-14.  The factor 10 is the project's convention (tests/test_gpu_absorption.py): the device
forms 1 / x by v_rcp_f64 and two Newton steps where the oracle divides, contracts to FMA, sums the orders four at a time and the
radii and angles in tiles.  No asserted bound exceeds 1e-9: three decades under the smallest defect.  Stage 3 is also held
alone, against mie_oracle.greek_from_bulk (mie_lin_oracle.greek_dot_from_bulk) in long double on the DEVICE's bulk functions.
The worst ratio deviation / bound per case and family is printed; the measured ones are in DESIGN.md 4.21 and 4.23."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest

import mie_cases as MC
import mie_lin_oracle as ML
import mie_oracle as MO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FACTOR = 10.0
BOUND_LIMIT = 1e-9
TEST_AEROSOL = (0.3, 2.1, 1.3, 0.001, 0.55)      # r_m, sigma_g, n_r, n_i, wavelength


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


@contextlib.contextmanager
def _poisoned_work(on):
    before = os.environ.get("VSM_POISON_WORK")
    if on:
        os.environ["VSM_POISON_WORK"] = "1"
    else:
        os.environ.pop("VSM_POISON_WORK", None)
    try:
        yield
    finally:
        if before is None:
            os.environ.pop("VSM_POISON_WORK", None)
        else:
            os.environ["VSM_POISON_WORK"] = before


def _launch(vsm, arch, h, lin, poison=True):
    """One call of vsm_mie_nai2 (lin: vsm_mie_nai2_lin) on the arrays of h, synchronised and fetched: a dict of float64 arrays."""
    S, A = vsm.Scattering, vsm.Architectures
    host = S.MieHostInputs(h.x / h.k_wave, h.wx, h.wr, h.x, np.asarray(h.nmax_i, dtype=np.int32), h.n_max, h.n_mu, h.mu, h.w_mu,
                           h.k_wave)
    model = S.make_mie_model(S.Aerosol(None, h.n_r, h.n_i), 2 * math.pi / h.k_wave)
    conv = A.array_type(arch)
    dev = S.device_inputs(host, conv)
    with _poisoned_work(poison):
        if lin:
            dev_dot = (conv(h.wx_dot), conv(h.wr_dot))
            run = S.launch_nai2_lin(model, host, dev, dev_dot)
        else:
            run = S.launch_nai2(model, host, dev)
    A.synchronize_if_gpu()
    names = MC.FAMILIES if lin else MC.FORWARD
    order = ("greek", "bulk_f", "scal", "greek_dot", "bulk_f_dot", "scal_dot")
    out = {n: A.to_host(t).copy() for n, t in zip(order, run) if n in names}
    assert all(v.dtype == np.float64 for v in out.values())
    return out


@functools.lru_cache(maxsize=None)
def _device(vsm, arch, name):
    """(forward call, linearized call) of a case with poisoned work buffers: launched once, shared, never changed."""
    h = MC.inputs(MC.BY_NAME[name])
    out = _launch(vsm, arch, h, False), _launch(vsm, arch, h, True)
    for o in out:
        for v in o.values():
            v.setflags(write=False)
    return out


def _bounds(floor):
    bound = {f: FACTOR * floor[f] for f in floor}
    for f, b in bound.items():                            # condition, not measurement: computed on the CPU alone
        assert floor[f] <= MC.FLOOR_LIMIT and b <= BOUND_LIMIT, (f, floor[f], b)
    return bound


def _accept(what, out, ref, bound, families, base=None):
    """Prints the ratio deviation / bound per family, then asserts each <= 1."""
    for f in families:
        assert np.all(np.isfinite(out[f])), (what, f)
    dev = MC.measure(out, ref, families, base=base)
    ratio = {f: dev[f] / bound[f] for f in families}
    print("mie edges %s: deviation / bound  %s" % (what, "  ".join("%s %.3f" % (f, ratio[f]) for f in families)))
    for f in families:
        assert ratio[f] <= 1.0, (what, f, dev[f], bound[f])
    return ratio


def _same(a, b, families):
    for f in families:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("name", MC.NAMES)
def test_both_entry_points_against_the_oracle(vsm, arch, name):
    ref, floor = MC.case_floors(name)
    bound = _bounds(floor)
    fwd, lin = _device(vsm, arch, name)
    o64 = MC.oracle(MC.inputs(MC.BY_NAME[name]))
    _accept(name + " vsm_mie_nai2", fwd, ref, bound, MC.FORWARD, base=o64)
    _accept(name + " vsm_mie_nai2_lin", lin, ref, bound, MC.FAMILIES, base=o64)
    if MC.BY_NAME[name].m[1] == 0.0:                       # no absorption: the albedo is 1 within the bound on its scale
        scale = float(ref["scales"].c_abs[0] / abs(ref["scal"][1]))
        assert abs(fwd["scal"][2] - 1.0) <= bound["scal"] * scale, fwd["scal"][2]
    if MC.BY_NAME[name].nquad == 1:                        # one radius: the weight slots are exact zeros
        assert not np.any(lin["greek_dot"][2:]) and not np.any(lin["bulk_f_dot"][2:]) and not np.any(lin["scal_dot"][2:])


@pytest.mark.parametrize("name", MC.NAMES)
def test_stage_3_alone_on_the_devices_bulk_functions(vsm, arch, name):
    """greek against greek_from_bulk(device's bulk_f, device's C_sca) in long double, greek_dot alike; the floor is that
    function's own float64-against-long-double deviation on the same inputs."""
    h = MC.inputs(MC.BY_NAME[name])
    _, lin = _device(vsm, arch, name)
    wide = MO.greek_from_bulk(lin["bulk_f"], lin["scal"][0], h.mu, h.w_mu, np.longdouble)
    own = MO.greek_from_bulk(lin["bulk_f"], lin["scal"][0], h.mu, h.w_mu)
    args = (lin["bulk_f"], lin["scal"][0], lin["bulk_f_dot"], lin["scal_dot"][:, 0], h.mu, h.w_mu)
    wide_dot, own_dot = ML.greek_dot_from_bulk(*args, np.longdouble), ML.greek_dot_from_bulk(*args)
    dev = lambda got, want: max(MC.vector_deviation(g, w) for g, w in zip(got.reshape(-1, h.n_mu), want.reshape(-1, h.n_mu)))
    floor = dict(greek=max(dev(own, wide), MC.MIN_FLOOR), greek_dot=max(dev(own_dot, wide_dot), MC.MIN_FLOOR))
    bound = _bounds(floor)
    ratio = dict(greek=dev(lin["greek"], wide) / bound["greek"], greek_dot=dev(lin["greek_dot"], wide_dot) / bound["greek_dot"])
    print("mie edges %s stage 3: deviation / bound  greek %.3f (floor %.1e)  greek_dot %.3f (floor %.1e)"
          % (name, ratio["greek"], floor["greek"], ratio["greek_dot"], floor["greek_dot"]))
    assert ratio["greek"] <= 1.0 and ratio["greek_dot"] <= 1.0, ratio


@pytest.mark.parametrize("name", MC.NAMES)
def test_calls_are_bit_identical(vsm, arch, name):
    """Two calls; a call with and one without poisoned work; the forward outputs of vsm_mie_nai2_lin against vsm_mie_nai2."""
    h = MC.inputs(MC.BY_NAME[name])
    fwd, lin = _device(vsm, arch, name)
    _same(lin, fwd, MC.FORWARD)
    _same(_launch(vsm, arch, h, False), fwd, MC.FORWARD)
    _same(_launch(vsm, arch, h, True), lin, MC.FAMILIES)
    _same(_launch(vsm, arch, h, False, poison=False), fwd, MC.FORWARD)
    _same(_launch(vsm, arch, h, True, poison=False), lin, MC.FAMILIES)


def test_exact_zeros_above_every_cutoff(vsm, arch):
    """Every cut-off at most 20 under n_max = 32: rows 21 .. 32 of every radius hold zeros, S1 and S2 are polynomials of degree
    20 in mu and the moments above 40 of every coefficient vector vanish -- as far as the float64 nodes and weights integrate
    exactly: the oracle's own values there (1e-11 and below, the same in both formats) set the comparison, and the device, whose
    work buffers are poisoned with NaN, is within the bound of them.  bulk_f and every other output are finite."""
    name = "q33_n32_cap20"
    ref, floor = MC.case_floors(name)
    bound = _bounds(floor)
    fwd, lin = _device(vsm, arch, name)
    o64 = MC.oracle(MC.inputs(MC.BY_NAME[name]))
    assert MC.inputs(MC.BY_NAME[name]).nmax_i.max() == 20 and ref["greek"].shape == (6, 63)
    assert all(np.all(np.isfinite(v)) for o in (fwd, lin) for v in o.values())
    sets = [(fwd["greek"], o64["greek"], ref["greek"], "greek")]
    sets += [(lin["greek_dot"][s], o64["greek_dot"][s], ref["greek_dot"][s], "greek_dot") for s in range(4)]
    worst = 0.0
    for got, want, wide, fam in sets:
        for c in range(6):
            scale = max(1.0, float(np.max(np.abs(wide[c]))))
            assert float(np.max(np.abs(wide[c, 41:]))) <= BOUND_LIMIT * scale                  # the premise, from the oracle
            d = float(np.max(np.abs(got[c, 41:] - want[c, 41:]))) / (bound[fam] * scale)
            worst = max(worst, d)
            assert d <= 1.0, (fam, c, d)
    print("mie edges %s moments above 40: deviation / bound %.3f" % (name, worst))
    assert np.max(np.abs(fwd["greek"][1, :41])) >= 1.0                                          # (and not everywhere)


@pytest.mark.parametrize("name", MC.NAMES)
def test_radii_without_weight_are_dead(vsm, arch, name):
    """Radii with wx = wr = 0 (and no weight derivatives) appended up to the next multiple of 64 and past it, with cut-offs anywhere
    in 1 .. n_max: the weights remove them, not the padding.  Every output stays within the bound of the shorter call's."""
    case = MC.BY_NAME[name]
    h = MC.inputs(case)
    ref, floor = MC.case_floors(name)
    bound = _bounds(floor)
    fwd, lin = _device(vsm, arch, name)
    full = (case.nquad // 64 + 1) * 64
    for total in (full, full + 7):
        longer = MC.with_dead_radii(h, total, case.seed + total)
        assert len(longer.x) == total and not np.any(longer.wr[case.nquad:]) and longer.nmax_i[case.nquad:].max() > 1
        _accept("%s + %d dead radii, vsm_mie_nai2" % (name, total - case.nquad), _launch(vsm, arch, longer, False), ref, bound,
                MC.FORWARD, base=fwd)
        _accept("%s + %d dead radii, vsm_mie_nai2_lin" % (name, total - case.nquad), _launch(vsm, arch, longer, True), ref, bound,
                MC.FAMILIES, base=lin)


def _public(vsm, arch, model):
    """compute_aerosol_optical_properties and _lin of one model as the dicts of _launch."""
    S = vsm.Scattering
    stack = lambda g: np.stack([g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta])
    opt, = S.compute_aerosol_optical_properties(model, arch)
    (lopt, lin), = S.compute_aerosol_optical_properties_lin(model, arch)
    fwd = dict(greek=stack(opt.greek_coefs), bulk_f=opt.bulk_f, scal=np.array([opt.C_sca, opt.C_ext, opt.ssa]))
    both = dict(greek=stack(lopt.greek_coefs), bulk_f=lopt.bulk_f, scal=np.array([lopt.C_sca, lopt.C_ext, lopt.ssa]),
                greek_dot=np.stack([stack(g) for g in lin.lin_greek_coefs]), bulk_f_dot=lin.bulk_f_dot,
                scal_dot=np.stack([lin.C_sca_dot, lin.k_dot, lin.ssa_dot], axis=1))
    assert opt.k == opt.C_ext and np.array_equal(lin.k_dot, lin.C_ext_dot)
    return fwd, both


def test_public_api_with_unsorted_radii(vsm, arch):
    """A TabulatedSizeDistribution of the test aerosol's 37 gauleg_log nodes, shuffled: natural cut-offs, n_max_i not monotone (the
    group's largest n_max_i is no longer its last radius').  Against the oracle's tabulated path at the bound above, and against
    the call on the sorted nodes within twice that bound."""
    S = vsm.Scattering
    r_m, sigma_g, n_r, n_i, lam = TEST_AEROSOL
    ln = S.LogNormal(r_m, sigma_g)
    r, w_r = S.gauleg_log(37, max(ln.quantile(1e-8), 1e-6 * 3.0), 3.0)
    raw = ln.pdf(r) * w_r
    raw_dot = S.lognormal_raw_dot(ln, r, raw)
    perm = np.random.default_rng(37).permutation(37)
    assert np.any(np.diff(perm) < 0) and np.any(np.diff(perm) > 0)

    def model(p):
        return S.make_mie_model(S.Aerosol(S.TabulatedSizeDistribution(r[p], raw[p], weights_dot=raw_dot[:, p]), n_r, n_i), lam)

    h = ML.mie_lin_inputs(None, lam, None, None, tabulated=(r[perm], raw[perm], raw_dot[:, perm]))
    h.n_r, h.n_i = n_r, n_i
    assert h.n_max == 57 and np.any(np.diff(h.nmax_i) < 0) and np.any(np.diff(h.nmax_i) > 0)
    ref, floor = MC.floors(h, 37)
    bound = _bounds(floor)
    o64 = MC.oracle(h)
    fwd, lin = _public(vsm, arch, model(perm))
    _same(lin, fwd, MC.FORWARD)
    _accept("shuffled test aerosol, compute_aerosol_optical_properties", fwd, ref, bound, MC.FORWARD, base=o64)
    _accept("shuffled test aerosol, compute_aerosol_optical_properties_lin", lin, ref, bound, MC.FAMILIES, base=o64)
    fwd_s, lin_s = _public(vsm, arch, model(np.arange(37)))
    twice = {f: 2 * b for f, b in bound.items()}
    _accept("shuffled against sorted, forward", fwd, ref, twice, MC.FORWARD, base=fwd_s)
    _accept("shuffled against sorted, linearized", lin, ref, twice, MC.FAMILIES, base=lin_s)
