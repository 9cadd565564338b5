"""GPU tests of the Absorption continua (vsm_absorption_continuum(_lin), csrc/vsm_absorption_continuum.hip) against
tests/continuum_oracle.py, on the seeded sets of tests/continuum_cases.py.

 * CIA-only sets: every plane is array_equal to oracle (a), forward and linearized, written over NaN (accumulate 0) and added to a
   random buffer (accumulate 1).  Only IEEE + - x run on the device and the host's coefficients are restated in the oracle, so
   equality is the expectation.
 * Planes with MT_CKD: |device - long-double oracle| <= (16 + 2 |texp|) 2^-53 sum|terms| per point and plane -- a count: about 8
   product roundings, up to 2 ulp each for tanh / sinh and pow, and the rounding of T_ref / T amplified by texp -- and the exact
   zeros (nu = 0, points outside the table) match the oracle's.  The measured maxima are printed.
 * Bit identity: the forward plane of the linearized call, a repetition, layers of a profile against single-layer calls, a
   permuted grid.
 * compute_absorption_profile(_lin) with continua=, the refusals, and the scene of DESIGN 4.26 end to end.

Shapes: nSpec in {1, 255, 256, 257, 1000}, Nz in {1, 2, L - 1, L, L + 1, 2 L + 3} with L = VSM_CONT_LAYERS, nT in {1, 2, 5}; the
layer temperatures of continuum_cases.T_LAYERS lie below, on the first node, inside a cell, on an interior node, on the last node
and above the range of the five-temperature tables."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import absorption_cases as AC
import absorption_lin_oracle as AL
import absorption_oracle as AO
import continuum_cases as CC
import continuum_oracle as CO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
EPS = 2.0 ** -53
Lz = CC.LAYERS

CIA_CASES = [("AA", 1, 1), ("AB", 255, 2), ("three", 256, Lz - 1), ("three", 257, Lz), ("eight", 1000, Lz + 1),
             ("eight", 257, 2 * Lz + 3), ("AA", 1000, 2 * Lz + 3), ("AB", 256, 2 * Lz + 3)]
BAND_CASES = [("band", 1, 1), ("band", 256, Lz), ("band", 1000, 2 * Lz + 3), ("three_band", 255, 2), ("three_band", 256, Lz - 1),
              ("three_band", 1000, Lz + 1), ("three_band", 257, 2 * Lz + 3)]


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


@functools.lru_cache(maxsize=None)
def _case(name, nSpec, Nz):
    g = CC.grid(nSpec)
    tables, band = CC.oracle_set(name, g, CO)
    for _, _, Ts, sig in tables:
        sig.setflags(write=False)
    return g, tables, band, CC.profile(Nz)


@functools.lru_cache(maxsize=None)
def _oracle_ld(name, nSpec, Nz):
    g, tables, band, (p, T, dz, vmr) = _case(name, nSpec, Nz)
    return CO.planes_ld(tables, band, g, p, T, dz, vmr)


def _run(vsm, arch, case, lin, prefill=None):
    """The planes [Nz, nSpec] of one entry-point call on a case: over NaN with accumulate 0, or added to `prefill`."""
    A = vsm.Absorption
    g, tables, band, (p, T, dz, vmr) = case
    job = A._prepare_continuum(CC.module_set(A, tables, band, g, arch), g, p, T, dz, vmr)
    dev = A._Device(arch)
    n = job.n_planes if lin else 1
    if prefill is None:
        planes = [torch.full((job.Nz, job.nSpec), float("nan"), dtype=torch.float64, device="cuda") for _ in range(n)]
    else:
        planes = [torch.as_tensor(np.array(prefill[m])).cuda() for m in range(n)]
    acc = 0 if prefill is None else 1
    if lin:
        dev.continuum_lin(job, planes, [acc] * n)
    else:
        dev.continuum(job, planes[0], acc)
    return dev.fetch(planes)


def test_constants_are_the_exported_ones(vsm):
    A = vsm.Absorption
    assert vsm._lib.lib().vsm_absorption_continuum_layers() == CC.LAYERS == A.CONT_LAYERS
    header = open(os.path.join(ROOT, "include", "vsmartmom_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+VSM_CONT_(\w+)\s+(\d+)", header)}
    assert defs == dict(MAX_TABLES=CC.MAX_TABLES, MAX_PLANES=A.CONT_MAX_PLANES, LAYERS=CC.LAYERS, BAND_FIELDS=A.CONT_BAND_FIELDS)
    assert A.CONT_MAX_TABLES == CC.MAX_TABLES == 8 and A.k_B == CO.K_B and A.MTCKD_C2 == CO.C2


@pytest.mark.parametrize("name,nSpec,Nz", CIA_CASES)
def test_cia_sets_equal_the_float64_chain_to_the_bit(vsm, arch, name, nSpec, Nz):
    case = _case(name, nSpec, Nz)
    g, tables, band, (p, T, dz, vmr) = case
    want = CO.planes64(tables, band, g, p, T, dz, vmr)
    fwd, lin = _run(vsm, arch, case, False), _run(vsm, arch, case, True)
    assert len(lin) == len(want) == 4 + len(CO.species_of(tables, band))
    assert np.all(np.isfinite(fwd[0])) and np.array_equal(fwd[0], want[0]) and want[0].max() > 0
    for m, (got, w) in enumerate(zip(lin, want)):
        assert np.all(np.isfinite(got)) and np.array_equal(got, w), (m, np.abs(got - w).max())
    rng = np.random.default_rng(nSpec + Nz)
    pre = [np.abs(w).max() * rng.uniform(-1.0, 1.0, w.shape) for w in want]
    want = CO.planes64(tables, band, g, p, T, dz, vmr, prefill=pre)
    assert np.array_equal(_run(vsm, arch, case, False, pre)[0], want[0])
    for m, (got, w) in enumerate(zip(_run(vsm, arch, case, True, pre), want)):
        assert np.array_equal(got, w), (m, np.abs(got - w).max())
    # the public call: the same planes, transposed
    r = vsm.Absorption.compute_continuum_profile(CC.module_set(vsm.Absorption, tables, band, g, arch), g, p, T, dz, vmr, lin=True)
    tau = vsm.Absorption.compute_continuum_profile(CC.module_set(vsm.Absorption, tables, band, g, arch), g, p, T, dz, vmr)
    sp = CO.species_of(tables, band)
    assert tau.shape == (nSpec, Nz) and np.array_equal(tau, lin[0].T) and np.array_equal(r.tau, tau)
    assert np.array_equal(r.dtau_dT, lin[1].T) and np.array_equal(r.dtau_dp, lin[2].T) and np.array_equal(r.dtau_ddz, lin[-1].T)
    assert list(r.dtau_dvmr) == sp and all(np.array_equal(r.dtau_dvmr[s], lin[3 + i].T) for i, s in enumerate(sp))


@pytest.mark.parametrize("name,nSpec,Nz", BAND_CASES)
def test_planes_with_mtckd_inside_the_rounding_count(vsm, arch, name, nSpec, Nz):
    case = _case(name, nSpec, Nz)
    g, tables, band, _ = case
    val, mag = _oracle_ld(name, nSpec, Nz)
    fwd, lin = _run(vsm, arch, case, False), _run(vsm, arch, case, True)
    assert np.array_equal(fwd[0], lin[0])
    bound = (16.0 + 2.0 * np.abs(band["texp"]))[None, :] * EPS
    names = ["tau", "dT", "dp"] + CO.species_of(tables, band) + ["ddz"]
    for m, got in enumerate(lin):
        assert got.dtype == np.float64 and np.all(np.isfinite(got)), names[m]
        err = np.abs(got.astype(LD) - val[m])
        live = mag[m] > 0
        worst = float(np.max((err / (bound * np.where(live, mag[m], 1)))[live])) if live.any() else 0.0
        print("continuum %s nSpec %d Nz %d plane %s: %d exact zeros, max error %.3f of the bound"
              % (name, nSpec, Nz, names[m], int((val[m] == 0).sum()), worst))
        assert np.array_equal(got == 0, val[m] == 0), names[m]
        assert np.all(err <= bound * mag[m]), (names[m], worst)
    if name == "band" and nSpec >= 4:
        dead = (g == 0) | (g > 20000.0)
        assert dead.sum() >= 2 and all(np.all(pl[:, dead] == 0) for pl in lin) and np.all(lin[0][:, ~dead][CC.H2O_LAYERS[:Nz] > 0] > 0)


@pytest.mark.parametrize("name", ["eight", "three_band"])
def test_bit_identity_of_repetitions_layers_and_permutations(vsm, arch, name):
    nSpec, Nz = 257, 2 * Lz + 3
    case = _case(name, nSpec, Nz)
    g, tables, band, (p, T, dz, vmr) = case
    lin = _run(vsm, arch, case, True)
    assert np.array_equal(_run(vsm, arch, case, False)[0], lin[0])
    for a, b in zip(lin, _run(vsm, arch, case, True)):
        assert np.array_equal(a, b)
    # layer z of the profile against the single-layer call: another layer tile, another Nz
    for z in range(Nz):
        one = {k: (v[z:z + 1] if np.ndim(v) else v) for k, v in vmr.items()}
        single = _run(vsm, arch, (g, tables, band, (p[z:z + 1], T[z:z + 1], dz[z:z + 1], one)), True)
        for m, (a, b) in enumerate(zip(lin, single)):
            assert np.array_equal(a[z], b[0]), (z, m)
    # a permuted grid, with the tables on the permuted grid: another lane and another workgroup for every point
    perm = np.random.default_rng(5).permutation(nSpec)
    tables_p = [(a, b, Ts, np.ascontiguousarray(sig[perm])) for a, b, Ts, sig in tables]
    band_p = None if band is None else dict(band, nu=g[perm], C_self=band["C_self"][perm], C_for=band["C_for"][perm], texp=band["texp"][perm])
    for a, b in zip(lin, _run(vsm, arch, (g[perm], tables_p, band_p, (p, T, dz, vmr)), True)):
        assert np.array_equal(a[:, perm], b)


def _golden(vsm, arch):
    A = vsm.Absorption
    ht = A.read_hitran(AC.GOLDEN_PAR, ν_min=6000, ν_max=6400)
    iso = dict(AC.ISOTOPOLOGUES)
    iso[(2, 2)] = (44.99318, iso[(2, 1)][1], 2.0 * iso[(2, 1)][2])
    iso[(1, 1)] = (18.01056, iso[(7, 1)][1], 0.8 * iso[(7, 1)][2])
    model = A.make_hitran_model(ht, A.Voigt(), vmr=4e-4, architecture=arch, isotopologues={k: A.IsotopologueData(*v) for k, v in iso.items()})
    return model, [(AC.table_dict(ht), iso, 4e-4, 4e-4)]


def _small_set(vsm, arch, g):
    """One CIA table (five temperatures) and the band on the grid g, as oracle tuples and as module objects."""
    tables = [("O2", "O2", CC.TS[5], CC.cia_values(77, len(g), 5))]
    t = CC.mtckd_table()
    Cs, Cf, te = CO.mtckd_band(t["nu"], t["C_self"], t["C_for"], t["texp"], g)
    band = dict(nu=g, C_self=Cs, C_for=Cf, texp=te, p_ref=t["p_ref"], T_ref=t["T_ref"])
    return tables, band, CC.module_set(vsm.Absorption, tables, band, g, arch)


def test_profile_calls_with_and_without_continua(vsm, arch):
    A, H = vsm.Absorption, vsm.host_model
    model, gases = _golden(vsm, arch)
    grid = np.linspace(6250.0, 6400.0, 257)
    p, T, vcd = AC.P3, AC.T3, np.array([3.1e21, 2.2e23, 1.9e24])
    dz, vmr = np.array([9100.0, 2300.0, 780.0]), {"H2O": np.array([4e-6, 2.5e-3, 0.031])}
    T_dot = np.ones((1, 3))
    pairs = [(model, 4e-4)]
    # continua=None: the call without the keyword, to the bit
    tau0 = A.compute_absorption_profile(pairs, grid, p, T, vcd)
    assert np.array_equal(A.compute_absorption_profile(pairs, grid, p, T, vcd, continua=None), tau0)
    r0 = A.compute_absorption_profile_lin(pairs, grid, p, T, vcd, T_dot=T_dot)
    rn = A.compute_absorption_profile_lin(pairs, grid, p, T, vcd, T_dot=T_dot, continua=None, dz=None, vmr=None, dz_dot=None)
    for a, b in zip(r0.lin_model_slots() + [r0.tau_abs, r0.dtau_dT, r0.dtau_dp], rn.lin_model_slots() + [rn.tau_abs, rn.dtau_dT, rn.dtau_dp]):
        assert np.array_equal(a, b)
    assert r0.dtau_ddz is None and r0.dtau_dvmr_continuum == {}
    # the set behind the gas
    tables, band, members = _small_set(vsm, arch, grid)
    c = A.compute_continuum_profile(members, grid, p, T, dz, vmr, lin=True)
    val, mag = CO.planes_ld(tables, band, grid, p, T, dz, vmr)
    r = A.compute_absorption_profile_lin(pairs, grid, p, T, vcd, T_dot=T_dot, continua=members, dz=dz, vmr=vmr, dz_dot=dz / T * T_dot)
    assert np.array_equal(A.compute_absorption_profile(pairs, grid, p, T, vcd, continua=members, dz=dz, vmr=vmr), r.tau_abs)
    # lines alone + set alone: the set adds k terms to a plane (tau and dp: the table and the band's two; dT: the slope too), summed
    # onto the lines in the one call and among themselves in the other; each of the k sums of either order rounds once, by at most
    # 2^-53 of the magnitudes summed
    for k, m, got, lines, alone in ((3, 0, r.tau_abs, tau0, c.tau), (4, 1, r.dtau_dT, r0.dtau_dT, c.dtau_dT), (3, 2, r.dtau_dp, r0.dtau_dp, c.dtau_dp)):
        tol = 2 * k * EPS * (np.abs(lines) + mag[m].T.astype(np.float64))
        assert np.all(np.abs(got - (lines + alone)) <= tol), m
        assert np.abs(alone).max() > 1e-6 * np.abs(lines).max()        # (the set is no negligible share of this plane)
    assert list(r.dtau_dvmr_continuum) == ["O2", "H2O"] and all(np.array_equal(r.dtau_dvmr_continuum[s], c.dtau_dvmr[s]) for s in ("O2", "H2O"))
    assert np.array_equal(r.dtau_ddz, c.dtau_ddz) and all(np.array_equal(a, b) for a, b in zip(r.tau_abs_dot, r0.tau_abs_dot))
    # the hydrostatic T-shift slot: d tau / dT + d tau / dΔz Δz / T, lines and set, within the two bounds added
    (dT64, _, _), _ = AL.absorption_profile_lin(gases, grid, p, T, vcd, wing_cutoff=40.0)
    (dTld, _, _), (AT, _, _) = AL.absorption_profile_lin(gases, grid, p, T, vcd, wing_cutoff=40.0, dtype=LD)
    floor = float(np.max(np.abs(dT64.astype(LD) - dTld)[AT > 0] / AT[AT > 0]))
    b_lines = 10 * max(floor, 1e-14) * AT
    hyd = (dz / T).astype(LD)[:, None]
    want = dT64.astype(LD) + (val[1] + val[-1] * hyd).T       # (the lines' bound is relative to their float64 oracle, as in their tests)
    b_set = ((16.0 + 2.0 * np.abs(band["texp"]))[None, :] * EPS * (mag[1] + mag[-1] * hyd)).T
    assert r.profile_slots.shape == (1, 257, 3)
    err = np.abs(r.profile_slots[0].astype(LD) - want)
    print("continuum profile slot: max error %.3f of the two bounds added" % float(np.max(err / (b_lines + b_set))))
    assert np.all(err <= b_lines + b_set)
    slots = r.lin_model_slots()
    assert len(slots) == 2 and slots[1] is not None and np.array_equal(slots[1], r.profile_slots[0])
    assert len(H.LinModel(tau_abs_dot=slots).tau_abs_dot) == 2
    with pytest.raises(vsm.VSMError, match="no \\(model, vmr\\) pair"):
        A.compute_absorption_profile([], grid, p, T, vcd, continua=members, dz=dz, vmr=vmr)


class _NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a refusal came after the device was asked for")


def test_refusals_leave_the_device_untouched(vsm, arch, monkeypatch):
    A = vsm.Absorption
    g, tables, band, (p, T, dz, vmr) = _case("three_band", 255, 2)
    members = CC.module_set(A, tables, band, g, arch)
    job = A._prepare_continuum(members, g, p, T, dz, vmr)
    # the library: VSM_ERR_INVALID_ARG before any launch -- the planes keep their NaN
    dev = A._Device(arch)
    planes = [torch.full((job.Nz, job.nSpec), float("nan"), dtype=torch.float64, device="cuda") for _ in range(job.n_planes)]
    n, hp, hn, d, b = dev._continuum_args(job, job.n_planes)
    lib, P, S = vsm._lib.lib(), A.CR._ptr, A.CR._stream_ptr()
    pl, acc = (C.c_void_p * len(planes))(*[t.data_ptr() for t in planes]), (C.c_int * len(planes))(*([0] * len(planes)))
    h2o, nP = 3 + job.species.index("H2O"), job.n_planes

    def lin(nSpec=job.nSpec, Nz=job.Nz, n=n, hp=hp, hn=hn, nP=nP, B=P(d[3]), nu=P(b[0]), h2o=h2o, ddz=nP - 1, acc=acc, pl=pl):
        return lib.vsm_absorption_continuum_lin(nSpec, Nz, n, hp, hn, P(d[0]), P(d[1]), nP, P(d[2]), B, nu, P(b[1]), P(b[2]), P(b[3]),
                                                P(b[4]), h2o, ddz, acc, pl, S)

    def fwd(nSpec=job.nSpec, Nz=job.Nz, n=n, accumulate=0, out=P(planes[0]), nu=P(b[0])):
        return lib.vsm_absorption_continuum(nSpec, Nz, n, hp, hn, P(d[0]), P(d[1]), P(d[2]), nu, P(b[1]), P(b[2]), P(b[3]), P(b[4]),
                                            accumulate, out, S)

    bad_nT = (C.c_int * 3)(5, 0, 1)
    same = (C.c_void_p * nP)(*([planes[0].data_ptr()] * 2 + [t.data_ptr() for t in planes[2:]]))
    bad_acc = (C.c_int * nP)(*([0, 2] + [0] * (nP - 2)))
    calls = [fwd(nSpec=0), fwd(Nz=0), fwd(Nz=65536), fwd(n=9), fwd(n=-1), fwd(accumulate=2), fwd(out=None), fwd(nu=None),
             lin(nSpec=0), lin(Nz=65536), lin(n=9), lin(hn=bad_nT), lin(nP=2), lin(nP=25), lin(B=None), lin(nu=None), lin(h2o=-1),
             lin(h2o=nP), lin(ddz=h2o), lin(ddz=2), lin(acc=bad_acc), lin(pl=same), lin(pl=None)]
    assert all(rc == 1 for rc in calls), calls                                   # VSM_ERR_INVALID_ARG
    assert b"vsm_absorption_continuum" in lib.vsm_last_error()
    out = torch.full((2, 3, 5), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.vsm_absorption_profile_slots_add(5, 3, 0, P(out), P(out), P(out), S) == 1
    assert lib.vsm_absorption_profile_slots_add(5, 3, 2, None, P(out), P(out), S) == 1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in planes + [out])
    assert lin() == 0 and fwd() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in planes)
    # the host: every refusal before a device object exists
    monkeypatch.setattr(A, "_Device", _NoDevice)
    E, f = vsm.VSMError, A.compute_continuum_profile
    model, _ = _golden(vsm, arch)
    refused = [
        lambda: f(members, g[::-1].copy(), p, T, dz, vmr), lambda: f(members[:3] * 3, g, p, T, dz, vmr),
        lambda: f(members + [members[-1]], g, p, T, dz, vmr), lambda: f([], g, p, T, dz, vmr),
        lambda: f(members, g, p * np.array([1.0, 0.0]), T, dz, vmr), lambda: f(members, g, p, T * np.array([-1.0, 1.0]), dz, vmr),
        lambda: f(members, g, p, T, dz * np.array([1.0, 0.0]), vmr), lambda: f(members, g, p, T, dz, dict(vmr, H2O=1.5)),
        lambda: f(members, g, p, T, dz, dict(vmr, H2O=-0.1)), lambda: f(members, g, p, T[:1], dz, vmr),
        lambda: f(members, g, p, T, dz, dict(vmr, H2O=np.full(3, 0.01))), lambda: f(members, g, p, T, dz, {}),
        lambda: A.compute_absorption_profile([(model, 4e-4)], g, p, T, np.ones(2), continua=members, vmr=vmr),
        lambda: A.compute_absorption_profile([(model, 4e-4)], g + 1.0, p, T, np.ones(2), continua=members, dz=dz, vmr=vmr),
        lambda: A.compute_absorption_profile_lin([(model, 4e-4)], g, p, T, np.ones(2), dz_dot=np.ones((1, 2))),
        lambda: A.compute_absorption_profile_lin([(model, 4e-4)], g, p, T, np.ones(2), T_dot=np.ones((2, 2)), continua=members, dz=dz,
                                                 vmr=vmr, dz_dot=np.ones((1, 2))),
    ]
    for n_call, call in enumerate(refused):
        with pytest.raises(E):
            call()


def test_scene_end_to_end(vsm, arch):
    """The scene of DESIGN 4.26 (nSpec = 64, Nz = 3, Stokes_IQU, Rayleigh, one line gas) with one CIA table and the band: rt_run and the
    hydrostatic T-shift slot of rt_run_lin on the module's arrays against the same runs on the oracles' arrays, within the 1e-8 of
    test_gpu_parity.py."""
    A, H = vsm.Absorption, vsm.host_model
    table = AC.synthetic_table(41, 120, no_E_share=0.1)
    grid = AC.nonuniform_grid(64, 13, lo=6010.0, hi=6040.0)
    p, T, vcd = AC.P3, AC.T3, 2.0 * np.array([3.1e21, 2.2e23, 1.9e24])
    dz, vmr_c = np.array([9100.0, 2300.0, 780.0]), {"H2O": np.array([4e-6, 2.5e-3, 0.031])}
    vmr, cutoff = 4.1e-4, 60.0
    tables, band, members = _small_set(vsm, arch, grid)
    pair = [(AC.make_model(A, table, wing_cutoff=cutoff, vmr=vmr, architecture=arch), vmr)]
    gases = [(table, AC.ISOTOPOLOGUES, vmr, vmr)]
    T_dot = np.ones((1, 3))
    r = A.compute_absorption_profile_lin(pair, grid, p, T, vcd, T_dot=T_dot, continua=members, dz=dz, vmr=vmr_c, dz_dot=dz / T * T_dot)
    slots = r.lin_model_slots()
    assert len(slots) == 2 and r.tau_abs.shape == (64, 3)
    tau_l, dots_o = AO.absorption_profile(gases, grid, p, T, vcd, wing_cutoff=cutoff)
    (dT_l, _, _), _ = AL.absorption_profile_lin(gases, grid, p, T, vcd, wing_cutoff=cutoff)
    pl = CO.planes64(tables, band, grid, p, T, dz, vmr_c)
    tau_o = tau_l + pl[0].T
    dT_o = dT_l + (pl[1] + pl[-1] * (dz / T)[:, None]).T
    assert (pl[0].T / tau_o).max() > 0.05                                 # (the set is a visible share of tau somewhere)
    tau_rayl = np.tile(0.02 * np.array([0.05, 0.25, 0.7]), (64, 1))

    def model(ta):
        return H.model_from_arrays(arch, "IQU", 8, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=ta, depol=0.0279, albedo=0.15, m_max=2)

    R0, T0 = vsm.CoreRT.rt_run(model(r.tau_abs))
    R0o, T0o = vsm.CoreRT.rt_run(model(tau_o))
    R, Tr, Rd, Td = vsm.CoreRTLin.rt_run_lin(model(r.tau_abs), H.LinModel(tau_abs_dot=slots), 0, 2, 1)
    Ro, To, Rdo, Tdo = vsm.CoreRTLin.rt_run_lin(model(tau_o), H.LinModel(tau_abs_dot=[dots_o[0], dT_o]), 0, 2, 1)
    for got, want in ((R0, R0o), (T0, T0o), (R, Ro), (Tr, To), (Rd[..., 1], Rdo[..., 1]), (Td[..., 1], Tdo[..., 1])):
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-8
