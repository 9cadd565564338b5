"""CPU tests of tests/absorption_lut_oracle.py (the reference of the GPU tests of Absorption.InterpolationModel) and of the model's
host side: axes, refusals, save / load, and the bookkeeping of a mixed-gas profile with the device replaced by the oracles.

The cubic interpolant is checked against scipy's natural cubic spline applied axis by axis: the reference's
BSpline(Cubic(Line(OnGrid()))) IS the natural spline through the nodes."""
import ctypes as C

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

import absorption_cases as AC
import absorption_lin_oracle as AL
import absorption_lut_oracle as LO
import absorption_oracle as AO


@pytest.fixture(scope="module")
def A():
    import vsmartmom_jl_amd as v
    return v.Absorption


def _table(seed, shape):
    rng = np.random.default_rng(seed)
    return 10.0 ** rng.uniform(-26.0, -20.0, shape)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 7, 50])
def test_cubic_interpolant_is_the_natural_spline_axis_by_axis(n):
    shape = (n, 3, 4) if n != 4 else (5, 4, 3)
    if n == 50:
        shape = (6, 3, 50)
    y = _table(n, shape)
    axes = [(6000.0, 0.25, shape[0]), (200.0, 150.0, shape[1]), (310.0, -12.5, shape[2])]       # (a descending T axis)
    rng = np.random.default_rng(100 + n)
    grid = rng.uniform(6000.0, 6000.0 + 0.25 * (shape[0] - 1), 40)
    p = rng.uniform(200.0, 200.0 + 150.0 * (shape[1] - 1), 5)
    T = rng.uniform(310.0 - 12.5 * (shape[2] - 1), 310.0, 5)
    nodes = [a[0] + a[1] * np.arange(a[2]) for a in axes]
    ref = np.empty((5, 40))
    for z in range(5):
        v = CubicSpline(nodes[0], y, axis=0, bc_type="natural")(grid)                              # [40, nP, nT]
        v = CubicSpline(nodes[1], v, axis=1, bc_type="natural")(p[z])                              # [40, nT]
        order = np.argsort(nodes[2])
        ref[z] = CubicSpline(nodes[2][order], v[:, order], axis=1, bc_type="natural")(T[z])
    for dtype in (np.float64, np.longdouble):
        got = LO.evaluate(LO.prefilter(y, dtype), *axes, grid, p, T, True, dtype)["sigma"]
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(y)))
        print("n = %d %s: max |oracle - scipy| / max |y| = %.2e" % (n, np.dtype(dtype).name, err))
        assert err <= 1e-13


def test_two_nodes_give_the_straight_line_and_nodes_are_reproduced():
    y = _table(1, (2, 2, 2))
    axes = [(6000.0, 1.0, 2), (100.0, 900.0, 2), (200.0, 100.0, 2)]
    c = LO.prefilter(y, np.longdouble)
    grid, p, T = np.array([6000.0, 6000.3, 6001.0]), np.array([100.0, 550.0, 1000.0]), np.array([200.0, 225.0, 300.0])
    cub = LO.evaluate(c, *axes, grid, p, T, True, np.longdouble)["sigma"]
    lin = LO.evaluate(y, *axes, grid, p, T, False, np.longdouble)["sigma"]
    assert np.max(np.abs(cub - lin)) <= 1e-17 * np.max(y)
    y = _table(2, (9, 5, 4))
    axes = [(6000.0, 0.5, 9), (250.0, 250.0, 5), (180.0, 35.0, 4)]
    for cubic, coef in ((True, LO.prefilter(y, np.longdouble)), (False, y)):
        for ip in range(5):
            for it in range(4):
                got = LO.evaluate(coef, *axes, 6000.0 + 0.5 * np.arange(9), 250.0 + 250.0 * ip, 180.0 + 35.0 * it, cubic,
                                  np.longdouble)["sigma"][0]
                assert np.max(np.abs(got - y[:, ip, it])) <= 1e-17 * np.max(y)
    # float64 coefficients against long double ones: the amplification of the filter stays below 3 per axis
    c64, cld = LO.prefilter(y, np.float64), LO.prefilter(y, np.longdouble)
    assert np.max(np.abs(c64 - cld)) <= 1e-14 * np.max(y) and np.max(np.abs(cld)) <= 27 * np.max(y)


@pytest.mark.parametrize("cubic", [True, False])
def test_oracle_derivatives_against_central_differences(cubic):
    y = _table(3, (7, 5, 4))
    axes = [(6000.0, 0.5, 7), (250.0, 250.0, 5), (180.0, 35.0, 4)]
    coef = LO.prefilter(y, np.longdouble) if cubic else y
    grid = np.array([6000.1, 6001.7, 6002.9, 5999.0])
    p, T = np.array([300.0, 777.0, 1240.0]), np.array([185.0, 251.0, 284.9])           # cell interiors
    ev = LO.evaluate(coef, *axes, grid, p, T, cubic, np.longdouble)
    for key, hp, hT in (("dp", 1e-3, 0.0), ("dT", 0.0, 1e-4)):
        up = LO.evaluate(coef, *axes, grid, p + hp, T + hT, cubic, np.longdouble)["sigma"]
        dn = LO.evaluate(coef, *axes, grid, p - hp, T - hT, cubic, np.longdouble)["sigma"]
        fd = (up - dn) / (2 * (hp + hT))
        # the step's truncation error is h^2 / 6 f''' (cubic; linear: none): 1e-8 of the derivative's scale is far above it
        scale = np.max(np.abs(ev[key]))
        assert scale > 0 and np.max(np.abs(fd - ev[key])) <= 1e-8 * scale
    assert np.all(ev["sigma"][:, 3] == 0) and np.all(ev["dT"][:, 3] == 0) and np.all(ev["dp"][:, 3] == 0)


# ---- the model's host side, with the device replaced by the oracles ------------------------------------------------------------------------
class OracleDevice:
    """Stands in for absorption._Device: line tables by tests/absorption_oracle.py, tables by tests/absorption_lut_oracle.py."""
    calls = []

    def __init__(self, architecture):
        pass

    def empty(self, Nz, nSpec):
        return np.full((Nz, nSpec), np.nan)

    def zeros(self, Nz, nSpec):
        return np.zeros((Nz, nSpec))

    def profile(self, job, lin=False):
        return job

    profile_lin = profile

    def xsec(self, job, handle, scale, out, accumulate):
        sig = AO.cross_section_lines(job.grid, job.lines, job.lines["species"], job.molar_mass, job.qratio, job.p, job.T, job.vmr_self,
                                     AO.BROADENINGS[job.broadening], AO.CEFS[job.cef], job.wing_cutoff)
        OracleDevice.calls.append(("xsec", int(accumulate)))
        out[...] = (out if accumulate else 0.0) + sig * np.asarray(scale)[:, None]

    def xsec_lin(self, job, handle, scale, out, out_dT, out_dp, out_dvmr, accumulate):
        sig = AO.cross_section_lines(job.grid, job.lines, job.lines["species"], job.molar_mass, job.qratio, job.p, job.T, job.vmr_self,
                                     AO.BROADENINGS[job.broadening], AO.CEFS[job.cef], job.wing_cutoff)
        dot = AL.cross_section_lin_lines(job.grid, job.lines, job.lines["species"], job.molar_mass, job.qratio, job.qratio_dlnT, job.p,
                                         job.T, job.vmr_self, AO.BROADENINGS[job.broadening], AO.CEFS[job.cef], job.wing_cutoff)[0]
        OracleDevice.calls.append(("xsec_lin", int(accumulate)))
        for o, v in zip((out, out_dT, out_dp, out_dvmr), (sig, dot[0], dot[1], dot[2])):
            o[...] = (o if accumulate else 0.0) + v * np.asarray(scale)[:, None]

    def _lut(self, job):
        m = job.model
        assert m._coef_host is not None and m._coef_host.dtype == m.storage_type
        axes = [(a.first, a.step, a.n) for a in (m.ν_grid, m.p_grid, m.t_grid)]
        return LO.evaluate(m.coefficients, *axes, job.grid, job.p, job.T, m.interp_type == "cubic")

    def lut_eval(self, job, scale, out, accumulate):
        OracleDevice.calls.append(("lut", int(accumulate)))
        out[...] = (out if accumulate else 0.0) + self._lut(job)["sigma"] * np.asarray(scale)[:, None]

    def lut_eval_lin(self, job, scale, out, out_dT, out_dp, accumulate):
        OracleDevice.calls.append(("lut_lin", int(accumulate)))
        ev = self._lut(job)
        for o, k in ((out, "sigma"), (out_dT, "dT"), (out_dp, "dp")):
            o[...] = (o if accumulate else 0.0) + ev[k] * np.asarray(scale)[:, None]

    def profile_slots(self, dT, dp, T_dot, p_dot):
        return dT[None] * np.asarray(T_dot)[:, :, None] + dp[None] * np.asarray(p_dot)[:, :, None]

    def fetch(self, outs):
        return [np.array(o) for o in outs]


@pytest.fixture()
def oracle_device(A, monkeypatch):
    monkeypatch.setattr(A, "_Device", OracleDevice)
    OracleDevice.calls = []
    return OracleDevice


def test_outside_band_testset_of_the_reference(A, oracle_device):
    """test/test_Absorption.jl:195-212, restated: the values are 100 iν + 10 ip + it with the reference's 1-based indices."""
    iv, ip, it = np.meshgrid(np.arange(1, 4), np.arange(1, 3), np.arange(1, 3), indexing="ij")
    coefs = (100 * iv + 10 * ip + it).astype(np.float64)
    model = A.InterpolationModel.from_values(coefs, 1, 1, A.UniformRange(6000.0, 1.0, 3), np.array([1000.0, 1100.0]),
                                             np.array([280.0, 290.0]), interp_type="linear")
    assert not model.resident and np.array_equal(model.coefficients, coefs) and np.array_equal(model.itp, coefs)
    sigma = A.absorption_cross_section(model, [6003.0, 6002.0, 6001.0, 6000.0, 5999.0], 1000.0, 280.0)
    assert sigma.shape == (5,) and sigma[0] == 0 and sigma[-1] == 0
    assert np.array_equal(sigma[1:4], [coefs[2, 0, 0], coefs[1, 0, 0], coefs[0, 0, 0]])
    assert oracle_device.calls == [("lut", 0)]
    # exactly on the far ends of p and T is inside; wavelength_flag reverses and reverses back
    s2 = A.compute_absorption_cross_section(model, [6000.5, 6001.0], np.array([1100.0, 1000.0]), np.array([290.0, 285.0]))
    assert s2.shape == (2, 2) and s2[0, 1] == coefs[1, 1, 1] and s2[1, 1] == 0.5 * (coefs[1, 0, 0] + coefs[1, 0, 1])
    wl = np.array([1e7 / 6002.0, 1e7 / 6001.5, 1e7 / 5990.0])
    a = A.compute_absorption_cross_section(model, wl, 1000.0, 280.0, wavelength_flag=True)
    b = A.compute_absorption_cross_section(model, (1e7 / wl)[::-1], 1000.0, 280.0)
    assert np.array_equal(a, b[::-1]) and a[2] == 0 and a[1] == pytest.approx(0.5 * (coefs[1, 0, 0] + coefs[2, 0, 0]), rel=1e-12)
    sig, dot = A.compute_absorption_cross_section_lin(model, [6001.0, 7000.0], 1050.0, 281.0)
    assert dot.shape == (3, 2) and A.SLOTS == ("T", "p", "vmr_self")
    assert dot[0, 0] == pytest.approx(0.1, rel=1e-13) and dot[1, 0] == pytest.approx(0.1, rel=1e-13)      # 1 per 10 K, 10 per 100 hPa
    assert np.all(dot[2] == 0) and np.all(dot[:, 1] == 0) and sig[1] == 0


def test_refusals_before_any_launch(A, oracle_device):
    import vsmartmom_jl_amd as vsm
    y = _table(4, (4, 3, 3))
    ax = (A.UniformRange(6000.0, 0.5, 4), np.array([250.0, 500.0, 750.0]), range(200, 350, 50))
    m = A.InterpolationModel.from_values(y, 2, -1, *ax, interp_type="linear")
    assert (m.t_grid.first, m.t_grid.step, m.t_grid.n) == (200.0, 50.0, 3) and m.iso == -1
    for p, T in ((249.9, 250.0), (750.1, 250.0), (500.0, 199.9), (500.0, 300.1), (np.array([500.0, 800.0]), np.array([250.0, 250.0]))):
        with pytest.raises(vsm.VSMError, match="outside the table"):
            A.compute_absorption_cross_section(m, [6000.2], p, T)
        with pytest.raises(vsm.VSMError, match="outside the table"):
            A.compute_absorption_profile([(m, 1e-3)], [6000.2], np.atleast_1d(p), np.atleast_1d(T), np.ones(np.size(p)))
    assert oracle_device.calls == []
    with pytest.raises(vsm.VSMError, match="finite"):
        A.compute_absorption_cross_section(m, [6000.2, np.nan], 500.0, 250.0)
    with pytest.raises(vsm.VSMError, match="not uniform"):
        A.InterpolationModel.from_values(y, 2, 1, ax[0], np.array([250.0, 500.0, 750.1]), ax[2], interp_type="linear")
    with pytest.raises(vsm.VSMError, match="two nodes"):
        A.InterpolationModel.from_values(y[:, :1], 2, 1, ax[0], np.array([250.0]), ax[2], interp_type="linear")
    with pytest.raises(vsm.VSMError, match="two nodes"):
        A.UniformRange(1.0, 1.0, 1)
    with pytest.raises(vsm.VSMError, match="step"):
        A.UniformRange(1.0, 0.0, 3)
    with pytest.raises(vsm.VSMError, match="interp_type"):
        A.InterpolationModel.from_values(y, 2, 1, *ax, interp_type="quadratic")
    with pytest.raises(vsm.VSMError, match="storage_type"):
        A.InterpolationModel.from_values(y, 2, 1, *ax, interp_type="linear", storage_type=np.float16)
    with pytest.raises(vsm.VSMError, match="shape"):
        A.InterpolationModel.from_coefficients(y, 2, 1, *ax, interp_type="cubic")                  # cubic wants [6, 5, 5]
    with pytest.raises(vsm.VSMError, match="neither"):
        A.compute_absorption_cross_section(object(), [6000.0], 500.0, 250.0)
    t = AC.synthetic_table(5, 6)
    with pytest.raises(vsm.VSMError, match="scalar"):
        A.make_interpolation_model(AC.hitran_table(A, t), A.Voigt(), *ax, vmr=np.zeros(3), isotopologues=AC.isotopologues(A))


@pytest.mark.parametrize("storage", [np.float64, np.float32])
@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_npz_round_trip_is_bit_exact(A, tmp_path, interp, storage):
    pad = 2 if interp == "cubic" else 0
    rng = np.random.default_rng(6)
    coef = (rng.standard_normal((5 + pad, 3 + pad, 2 + pad)) * 1e-22).astype(storage)
    m = A.InterpolationModel.from_coefficients(coef, 2, -1, A.UniformRange(6286.0, 0.002, 5), A.UniformRange(1250.0, -500.0, 3),
                                               A.UniformRange(180.0, 0.1 + 0.2, 2), interp_type=interp)
    assert m.storage_type == np.dtype(storage)
    path = str(tmp_path / "model.npz")
    A.save_interpolation_model(m, path)
    with np.load(path, allow_pickle=False) as z:                      # plain arrays only
        assert sorted(z.files) == ["coefficients", "interp_type", "iso", "mol", "nu_range", "p_range", "storage", "t_range"]
    back = A.load_interpolation_model(path)
    assert back.coefficients.dtype == np.dtype(storage) and back.coefficients.tobytes() == np.ascontiguousarray(coef).tobytes()
    assert (back.mol, back.iso, back.interp_type, back.storage_type) == (2, -1, interp, np.dtype(storage))
    for a, b in ((m.ν_grid, back.ν_grid), (m.p_grid, back.p_grid), (m.t_grid, back.t_grid)):
        assert (a.first, a.step, a.n) == (b.first, b.step, b.n)
    assert not back.resident


def test_mixed_profile_bookkeeping(A, oracle_device):
    """A table gas between two line-by-line gases: launches, accumulate flags, slots and the exact zeros of dtau_dvmr_self."""
    ta, tb = AC.synthetic_table(21, 12), AC.synthetic_table(22, 9)
    grid = AC.nonuniform_grid(40, 9)
    vcd = np.array([3.1e21, 2.2e23, 1.9e24])
    y = _table(7, (11, 3, 4))
    axes = [(6000.0, 5.0, 11), (0.1, 600.0, 3), (180.0, 50.0, 4)]
    lut = A.InterpolationModel.from_coefficients(LO.prefilter(y), 7, 1, *[A.UniformRange(*a) for a in axes])
    vmr_a, vmr_t, vmr_b = 4.1e-4, np.array([0.21, 0.2, 0.19]), 1e-6
    pairs = [(AC.make_model(A, ta, vmr=vmr_a), vmr_a), (lut, vmr_t), (AC.make_model(A, tb), vmr_b)]
    tau, dots = A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd, lin=True)
    assert oracle_device.calls == [("xsec", 0), ("xsec", 0), ("lut", 1), ("lut", 0), ("xsec", 1), ("xsec", 0)]
    ev = LO.evaluate(lut.coefficients, *axes, grid, AC.P3, AC.T3)
    ref_a = AO.cross_section(ta, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, vmr_a, wing_cutoff=5.0)
    ref_b = AO.cross_section(tb, AC.ISOTOPOLOGUES, grid, AC.P3, AC.T3, 0.0, wing_cutoff=5.0)
    ref = (ref_a * (vcd * vmr_a)[:, None] + ev["sigma"] * (vcd * vmr_t)[:, None]) + ref_b * (vcd * vmr_b)[:, None]
    assert tau.shape == (40, 3) and np.array_equal(tau, ref.T)
    assert np.array_equal(dots[1], (ev["sigma"] * vcd[:, None]).T)
    assert np.array_equal(A.compute_absorption_profile(pairs, grid, AC.P3, AC.T3, vcd), tau)
    # a table gas first: it writes, the line-by-line gas adds
    oracle_device.calls.clear()
    A.compute_absorption_profile(pairs[1:], grid, AC.P3, AC.T3, vcd)
    assert oracle_device.calls == [("lut", 0), ("xsec", 1)]
    # the table alone, linearized: T_dot = unit table
    oracle_device.calls.clear()
    r = A.compute_absorption_profile_lin([(lut, vmr_t)], grid, AC.P3, AC.T3, vcd, T_dot=np.eye(3))
    assert oracle_device.calls == [("lut_lin", 0), ("lut", 0)]
    assert np.array_equal(r.tau_abs, (ev["sigma"] * (vcd * vmr_t)[:, None]).T)
    assert np.array_equal(r.dtau_dT, (ev["dT"] * (vcd * vmr_t)[:, None]).T)
    assert np.array_equal(r.dtau_dp, (ev["dp"] * (vcd * vmr_t)[:, None]).T)
    assert len(r.dtau_dvmr_self) == 1 and np.all(r.dtau_dvmr_self[0] == 0) and r.dtau_dvmr_self[0].shape == (40, 3)
    assert r.profile_slots.shape == (3, 40, 3)
    for k in range(3):
        assert np.array_equal(r.profile_slots[k][:, k], r.dtau_dT[:, k]) and np.count_nonzero(np.delete(r.profile_slots[k], k, 1)) == 0
    assert len(r.lin_model_slots()) == 1 + 3
    # the mix, linearized: the table adds to the shared T and p planes; only the line-by-line gases have a vmr_self plane
    oracle_device.calls.clear()
    rm = A.compute_absorption_profile_lin(pairs, grid, AC.P3, AC.T3, vcd)
    assert oracle_device.calls == [("xsec_lin", 0), ("xsec", 0), ("lut_lin", 1), ("lut", 0), ("xsec_lin", 1), ("xsec", 0)]
    ra, rb = (A.compute_absorption_profile_lin([pr], grid, AC.P3, AC.T3, vcd) for pr in (pairs[0], pairs[2]))
    assert np.array_equal(rm.tau_abs, tau) and all(np.array_equal(a, b) for a, b in zip(rm.tau_abs_dot, dots))
    assert np.array_equal(rm.dtau_dT, (ra.dtau_dT + r.dtau_dT) + rb.dtau_dT) and np.array_equal(rm.dtau_dp, (ra.dtau_dp + r.dtau_dp) + rb.dtau_dp)
    assert np.array_equal(rm.dtau_dvmr_self[0], ra.dtau_dvmr_self[0]) and np.array_equal(rm.dtau_dvmr_self[2], rb.dtau_dvmr_self[0])
    assert np.all(rm.dtau_dvmr_self[1] == 0) and rm.profile_slots.shape == (0, 40, 3)


def test_entries_refuse_bad_arguments_before_any_launch():
    """The three entries check sizes, steps, enums and null pointers before they touch the device: the codes come back on a machine
    without one."""
    import vsmartmom_jl_amd as vsm
    lib = vsm._lib.lib()
    buf = (C.c_double * 64)()
    P = C.cast(buf, C.c_void_p)
    INVALID = 1

    def call(lin, nSpec=4, Nz=1, nNu=3, nP=2, nT=2, steps=(1.0, 100.0, 10.0), first=(6000.0, 1000.0, 280.0), interp=1, storage=0,
             accumulate=0, null=None):
        ax = [C.c_double(v) for pair in zip(first, steps) for v in pair]
        ptrs = [None if i == null else P for i in range(8 if lin else 6)]
        fn = lib.vsm_absorption_lut_eval_lin if lin else lib.vsm_absorption_lut_eval
        return fn(nSpec, Nz, nNu, nP, nT, *ax, interp, storage, *ptrs[:5], accumulate, *ptrs[5:], None)

    for lin in (0, 1):
        for kw in (dict(nSpec=0), dict(Nz=0), dict(Nz=65536), dict(nNu=1), dict(nP=1), dict(nT=1), dict(steps=(0.0, 100.0, 10.0)),
                   dict(steps=(1.0, float("nan"), 10.0)), dict(steps=(1.0, 100.0, float("inf"))), dict(first=(float("nan"), 0.0, 0.0)),
                   dict(interp=2), dict(interp=-1), dict(storage=2), dict(accumulate=2)):
            assert call(lin, **kw) == INVALID, kw
            assert b"vsm_absorption_lut_eval" in lib.vsm_last_error()
        for null in range(8 if lin else 6):
            assert call(lin, null=null) == INVALID, null
    for kw in (dict(nNu=1), dict(nP=1), dict(nT=0), dict(storage=3), dict(null=0), dict(null=1), dict(null=2)):
        a = dict(nNu=5, nP=2, nT=2, storage=0, null=None)
        a.update(kw)
        ptrs = [None if i == a["null"] else P for i in range(3)]
        assert lib.vsm_absorption_lut_prefilter(a["nNu"], a["nP"], a["nT"], ptrs[0], a["storage"], ptrs[1], ptrs[2], None) == INVALID, kw
    assert lib.vsm_absorption_lut_work_elems(10, 3, 4, 0) == 3 * 4 * 12 + 3 * 6 * 12
    assert lib.vsm_absorption_lut_work_elems(10, 3, 4, 1) == 3 * 4 * 12 + 3 * 6 * 12 + 5 * 6 * 12
    assert lib.vsm_absorption_lut_work_elems(1, 3, 4, 0) == 0 and lib.vsm_absorption_lut_work_elems(10, 3, 4, 2) == 0
    assert lib.vsm_absorption_lut_chunk() == 32 and lib.vsm_absorption_lut_span() == 1024
