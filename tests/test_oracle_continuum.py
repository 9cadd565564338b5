"""CPU tests of the Absorption continua: the host side of vsm.Absorption -- the .cia parser, the projections, the layer
thickness, the refusals -- against the reference's loops typed again in tests/continuum_oracle.py, and the oracles against each
other: every derivative of the long-double oracle against central differences of its forward, and the float64 restatement of the
device's MT_CKD arithmetic inside the bound the device is held to, (16 + 2 |texp|) 2^-53 sum |terms| per point and plane."""
import functools

import numpy as np
import pytest

import continuum_cases as CC
import continuum_oracle as CO

L = np.longdouble
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def A():
    import vsmartmom_jl_amd as v
    return v.Absorption


def _header(formula, lo, hi, n, T):
    return "%-20s%10.3f%10.3f%7d%7.1f%10.3E%6.3f%27s%3d" % (formula, lo, hi, n, T, 1.0e-44, -0.999, "a reference", 1)


def _write_cia(path):
    """Two temperatures; 200 K comes in two blocks with overlapping ranges; a blank line, a short line and a third data column."""
    blocks = [("O2-N2", 200.0, np.array([100.0, 101.5, 104.0, 110.0]), np.array([1.0e-46, 3.0e-46, 0.0, 2.5e-45])),
              ("O2-N2", 250.0, np.array([95.0, 105.0, 125.0]), np.array([4.0e-46, 6.5e-45, 1.5e-46])),
              ("O2-N2", 200.0, np.array([105.0, 107.0, 120.0]), np.array([7.0e-45, 8.0e-46, 9.0e-47]))]
    with open(path, "w") as f:
        for n, (formula, T, nu, sig) in enumerate(blocks):
            f.write(_header(formula, nu[0], nu[-1], len(nu), T) + "\n")
            for a, b in zip(nu, sig):
                f.write("%10.4f %10.3E %8.2E\n" % (a, b, 1.0e-47) if n == 0 else "%10.4f %10.3E\n" % (a, b))
            f.write("\n" if n == 0 else "too short to be a header\n")
    return blocks


GRID = np.array([90.0, 95.0, 99.999, 100.0, 100.7, 101.5, 103.0, 104.9, 105.0, 106.1, 107.0, 109.0, 110.0, 110.001, 115.0, 120.0,
                 122.5, 125.0, 125.001, 130.0])


def test_parser_and_projection_equal_the_literal_loops(A, tmp_path):
    path = str(tmp_path / "O2-N2_test.cia")
    want = _write_cia(path)
    blocks = A.parse_cia_file(path)
    assert len(blocks) == 3
    for blk, (formula, T, nu, sig) in zip(blocks, want):
        assert blk.formula == formula and blk.T == T
        assert np.array_equal(blk.ν, nu) and np.array_equal(blk.σ, sig)
    for g in (GRID, GRID[::-1].copy()):                                  # ascending and descending
        t = A.load_cia_table(path, g)
        Ts, sig = CO.build_table([(T, nu, s) for _, T, nu, s in want], g)
        assert (t.pair, t.species_a, t.species_b) == ("O2-N2", "O2", "N2")
        assert np.array_equal(t.Ts, Ts) and np.array_equal(t.Ts, [200.0, 250.0]) and np.array_equal(t.ν_grid, g)
        assert t.σ_νT.shape == (len(g), 2) and np.array_equal(t.σ_νT, sig)
    t = A.load_cia_table(path, GRID)
    at = dict(zip(GRID.tolist(), t.σ_νT[:, 0].tolist()))
    assert at[99.999] == 0.0 and at[100.0] == 1.0e-46 and at[120.0] == 9.0e-47 and at[122.5] == 0.0       # the ends of a range
    assert at[105.0] == 7.0e-45 and at[110.0] == np.float64(CO.project_block(np.zeros(1), [110.0], want[2][2], want[2][3])[0])
    assert at[104.9] != 0.0 and at[104.9] == CO.project_block(np.zeros(1), [104.9], want[0][2], want[0][3])[0]   # below the overlap
    assert np.array_equal(A.build_cia_table(blocks, GRID).σ_νT, t.σ_νT)


def test_projection_refuses_blocks_that_do_not_ascend(A):
    good = A.CIABlock("N2-N2", 250.0, [1.0, 2.0, 3.0], [1e-46, 2e-46, 3e-46])
    for nu in ([1.0, 2.0, 2.0], [3.0, 2.0, 1.0], []):
        bad = A.CIABlock("N2-N2", 250.0, nu, [1e-46] * len(nu))
        with pytest.raises(A._lib.VSMError, match="strictly ascending"):
            A.build_cia_table([good, bad], GRID)
    with pytest.raises(A._lib.VSMError, match="no blocks"):
        A.build_cia_table([], GRID)
    with pytest.raises(A._lib.VSMError, match="not recognised"):
        A.build_cia_table([A.CIABlock("N2", 250.0, [1.0, 2.0], [1e-46, 2e-46])], GRID)


def test_from_arrays_checks_its_arrays(A):
    g = CC.grid(16)
    t = A.CIATable.from_arrays("CO2-CO2", CC.TS[2], CC.cia_values(1, 16, 2), g)
    assert (t.species_a, t.species_b) == ("CO2", "CO2") and t.σ_νT.shape == (16, 2)
    with pytest.raises(A._lib.VSMError):
        A.CIATable.from_arrays("CO2-CO2", CC.TS[2][::-1], CC.cia_values(1, 16, 2), g)
    with pytest.raises(A._lib.VSMError):
        A.CIATable.from_arrays("CO2-CO2", CC.TS[2], CC.cia_values(1, 15, 2), g)


def test_mtckd_npz_and_band_projection(A, tmp_path):
    t = CC.mtckd_table()
    path = str(tmp_path / "mtckd.npz")
    np.savez(path, wavenumbers=t["nu"], self_absco_ref=t["C_self"], for_absco_ref=t["C_for"], self_texp=t["texp"],
             ref_press=np.array(t["p_ref"]), ref_temp=np.array([t["T_ref"]]))
    table = A.load_mtckd(path)
    assert table.p_ref == t["p_ref"] and table.T_ref == t["T_ref"] and np.array_equal(table.self_texp, t["texp"])
    g = np.concatenate([CC.grid(257), [-20.0, -20.001, 20000.0, 20000.001, 10.0, 15.0]])      # table ends, nodes, outside
    band = A.build_mtckd_band(table, g)
    want = CO.mtckd_band(t["nu"], t["C_self"], t["C_for"], t["texp"], g)
    for got, w in zip((band.C_self, band.C_for, band.texp), want):
        assert np.array_equal(got, w)
    out = (g < -20.0) | (g > 20000.0)
    assert out.sum() >= 3 and np.all(band.C_self[out] == 0) and np.all(band.C_for[out] == 0) and np.all(band.texp[out] == 0)
    assert np.all(band.C_self[~out] > 0) and np.array_equal(band.ν_grid, g)
    np.savez(path, wavenumbers=t["nu"])
    with pytest.raises(A._lib.VSMError, match="lacks"):
        A.load_mtckd(path)


def test_layer_thickness_equals_the_formula(A):
    p_half = np.array([0.1, 3.0, 77.5, 420.0, 1013.25])
    T, v = np.array([221.0, 216.5, 243.2, 288.1]), np.array([3e-6, 1e-5, 2e-3, 0.031])
    got, want = A.layer_thickness(p_half, T, v), CO.layer_thickness(p_half, T, v)
    assert got.shape == (4,) and np.all(got > 0)
    assert np.all(np.abs(got - want) <= 2 * np.spacing(want))     # (numpy's vector log may differ from its scalar log in the last bit)
    assert 6000.0 < got[-1] < 8000.0                              # 420 -> 1013 hPa near 288 K: about 7.4 km
    with pytest.raises(A._lib.VSMError):
        A.layer_thickness(p_half, T[:3], v[:3])


@functools.lru_cache(maxsize=None)
def _case(name, nSpec, Nz):
    g = CC.grid(nSpec)
    tables, band = CC.oracle_set(name, g, CO)
    return g, tables, band, CC.profile(Nz)


def test_chains_reproduce_the_reference_forward():
    """tau of oracle (a): a CIA-only set is the reference's loop to the bit (one product and one sum per table in both); with the
    band the two differ in the order of the products alone."""
    g, tables, band, (p, T, dz, vmr) = _case("three", 40, 11)
    ref = CO.reference_tau(tables, None, g, p, T, dz, vmr)
    assert np.array_equal(CO.planes64(tables, None, g, p, T, dz, vmr)[0].T, ref) and ref.max() > 0
    g, tables, band, (p, T, dz, vmr) = _case("three_band", 40, 11)
    ref, got = CO.reference_tau(tables, band, g, p, T, dz, vmr), CO.planes64(tables, band, g, p, T, dz, vmr)[0].T
    assert np.all(np.abs(got - ref) <= 1e-13 * np.abs(ref)) and np.array_equal(got == 0, ref == 0)


def _perturbed(p, T, dz, vmr, what, sign, species=None):
    """The profile with one input moved by a relative 1e-6 (an absolute 1e-6 for a vmr, which may be 0), in long double."""
    p, T, dz = p.astype(L), T.astype(L), dz.astype(L)
    vmr = {k: np.broadcast_to(np.asarray(v, dtype=L), p.shape).copy() for k, v in vmr.items()}
    for sp, v in CO.VMR_DEFAULTS.items():
        vmr.setdefault(sp, np.full(p.shape, v, dtype=L))
    h = {"T": L(1e-6) * T, "p": L(1e-6) * p, "dz": L(1e-6) * dz}.get(what, L(1e-6))
    if what == "T":
        T = T + sign * h
    elif what == "p":
        p = p + sign * h
    elif what == "dz":
        dz = dz + sign * h
    else:
        vmr[species] = vmr[species] + sign * h
    return (p, T, dz, vmr), h


@pytest.mark.parametrize("name", ["three_band", "eight", "band"])
def test_long_double_derivatives_against_central_differences(name):
    """Layers whose T sits inside a cell or outside the range of every table (a node is a kink of the interpolant): T_LAYERS moved
    off the nodes by 1.3 K."""
    g, tables, band, (p, T, dz, vmr) = _case(name, 40, 11)
    T = T + 1.3
    val, mag = CO.planes_ld(tables, band, g, p, T, dz, vmr)
    species = CO.species_of(tables, band)
    slots = [("T", 1, None), ("p", 2, None), ("dz", len(val) - 1, None)] + [("vmr", 3 + i, sp) for i, sp in enumerate(species)]
    for what, m, sp in slots:
        (up, h), (dn, _) = _perturbed(p, T, dz, vmr, what, +1, sp), _perturbed(p, T, dz, vmr, what, -1, sp)
        fp, fm = CO.planes_ld(tables, band, g, *up)[0][0], CO.planes_ld(tables, band, g, *dn)[0][0]
        fd = (fp - fm) / (2 * (h[:, None] if np.ndim(h) else h))
        live = mag[m] > 0
        err = float(np.max(np.abs(fd - val[m])[live] / mag[m][live])) if live.any() else 0.0
        print("continuum oracle %s d/d%s%s: max |fd - analytic| / sum|terms| = %.2e" % (name, what, "" if sp is None else " " + sp, err))
        assert np.all(val[m][~live] == 0) and np.all(fd[~live] == 0)
        assert err <= 1e-8, (what, sp, err)


def test_float64_restatement_of_the_band_stays_inside_the_device_bound():
    for name, nSpec in (("band", 1000), ("three_band", 257)):
        g, tables, band, (p, T, dz, vmr) = _case(name, nSpec, 11)
        got = CO.planes64(tables, band, g, p, T, dz, vmr)
        val, mag = CO.planes_ld(tables, band, g, p, T, dz, vmr)
        bound = (16.0 + 2.0 * np.abs(band["texp"]))[None, :] * EPS
        worst = 0.0
        for m in range(len(val)):
            err = np.abs(got[m].astype(L) - val[m])
            assert np.array_equal(got[m] == 0, val[m] == 0), m
            live = mag[m] > 0
            worst = max(worst, float(np.max((err / (bound * np.where(live, mag[m], 1)))[live])))
            assert np.all(err <= bound * mag[m]), m
        print("continuum oracle %s: float64 restatement at %.2f of the device bound" % (name, worst))
        zero = (g == 0) | (g < -20.0) | (g > 20000.0)
        assert zero.sum() >= 2 and (name != "band" or all(np.all(pl[:, zero] == 0) for pl in got))


def test_set_refusals_need_no_device(A):
    """Every refusal of a set is raised by the host before a device is asked for (this machine has none)."""
    g, tables, band, (p, T, dz, vmr) = _case("three_band", 40, 4)
    members = CC.module_set(A, tables, band, g)
    E = A._lib.VSMError
    f = A.compute_continuum_profile
    with pytest.raises(E, match="ν_grid"):
        f(members, g[::-1].copy(), p, T, dz, vmr)
    with pytest.raises(E, match="ν_grid"):
        f(members, g + 1e-9, p, T, dz, vmr)
    with pytest.raises(E, match="above 8"):
        f(members[:3] * 3, g, p, T, dz, vmr)
    with pytest.raises(E, match="MTCKDBands"):
        f(members + [members[-1]], g, p, T, dz, vmr)
    with pytest.raises(E, match="empty"):
        f([], g, p, T, dz, vmr)
    for bad in (0.0, -1.0, np.nan):
        for i in range(3):
            args = [p.copy(), T.copy(), dz.copy()]
            args[i][1] = bad
            with pytest.raises(E, match="positive"):
                f(members, g, *args, vmr)
    for v in (-1e-9, 1.0 + 1e-9):
        with pytest.raises(E, match="outside"):
            f(members, g, p, T, dz, dict(vmr, H2O=v))
    with pytest.raises(E, match="layers"):
        f(members, g, p, T[:3], dz, vmr)
    with pytest.raises(E, match="layers"):
        f(members, g, p, T, dz[:2], vmr)
    with pytest.raises(E, match="shape"):
        f(members, g, p, T, dz, dict(vmr, H2O=np.full(3, 0.01)))
    with pytest.raises(E, match='no vmr for "H2O"'):
        f(members, g, p, T, dz, {})
    with pytest.raises(E, match='no vmr for "CO2"'):
        f([A.CIATable.from_arrays("CO2-CO2", CC.TS[1], CC.cia_values(3, 40, 1), g)], g, p, T, dz, {})
    with pytest.raises(E, match="neither"):
        f(members + [object()], g, p, T, dz, vmr)
