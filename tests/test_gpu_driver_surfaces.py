"""GPU tests of every driver over every surface type, as a grid.

(a) Degenerate identities.  A constant BRDF is a Lambertian surface: each of the thirteen drivers gives, over rpvSurfaceScalar(a, 1,
    1, 0), RossLiSurfaceScalar(0, 0, a), LambertianSurfaceLegendre([a, 0]), LambertianSurfaceSpline([a] * S) and the bare albedo = a,
    what it gives over LambertianSurfaceScalar(a).  Both sides are device runs of the same kernels.  Beside a surface object the
    models are built with albedo = 0.6 (a = 0.25; the spline: the default 0), which model.albedo keeps for every surface but the
    scalar Lambertian one: a driver that reads the float is off by half the signal -- the CPU guards next to the oracles (test_oracle_raman.py ...: a black surface is >= 0.1 away on these scenes)
    keep that from hiding in a bound.
    The two spectral surfaces take the reference's own builder (lambertian_surface.jl:97-213), which differs from the scalar one
    where the albedo does not enter: j0+ = 0, and t++ = t-- = 0 for m > 0 (lambertian_surface.jl:135,154-156 against :75,90-91).  r-+
    and j0- are the scalar builder's, so every field that leaves the surface upwards agrees; what arrives at the bottom of the whole
    column -- T, ieT, their derivatives, dw / dwie of level 0, bhr_dw: J0+ of the composite that includes the surface layer -- does
    not, by the reference's statements.  Those outputs (`down` below) are compared between the Legendre and the spline cell, which
    share a builder, and not against the scalar cell.
    Linearized drivers: the forward outputs, every aerosol and gas column, and the one surface column that means the same on both
    sides (rho0, fiso, c0, the spline's table of ones against the albedo slot); the other surface columns have to be finite.
(b) Real BRDFs -- rpvSurfaceScalar(0.12, 0.08, 0.75, -0.25) on the scalar shape, CoxMunkSurface(5) on the IQU shape -- in the three
    Raman drivers, CoreRT.rt_run_fluxes and CoreRTLin.rt_run_fluxes (forward fields) against the oracles with their surface hooks.
(c) A non-constant Legendre surface in CoreRTRaman.rt_run: blocks with halos and a spectral slice are bit-identical to one pass.
(d) check_device_status after every driver.

Shapes: ("I", 9) N = 8 and ("IQU", 7) N = 21; S = 14, three layers, m_max 2, two viewing angles, levels [0, 2, 3]
(tests/driver_surface_cases.py).  The linearized cells carry one aerosol (7 columns) and two gases.

Bounds: none of its own.  Each cell takes the bound its driver's sibling test has against its oracle, in that precision (BOUNDS);
the error is measured per Stokes component (and per level, per parameter column) relative to that part's largest reference value
in FP64 -- at least as strict as every sibling's measure -- and in FP32 as the sibling measures it.  A component whose largest
reference value is below the bound times the array's (U just above a Cox-Munk surface at nadir: 1e-13 of I) is measured against
the array's largest value, as the siblings measure a component that is exactly zero (_err).

Measured on an MI355X, worst cell per driver (pytest -s prints every cell; bounds in BOUNDS):
  (a)  driver                          FP64 (five surfaces)    FP32 (RPV cell)
       rt_run / rt_run_full            6.2e-15 / 8.0e-15       0
       multisensor                     8.0e-15                 0
       fluxes                          0                       0
       ss, ss_rrs                      7.2e-15                 0
       lin                             1.1e-13                 8.5e-7
       multisensor_lin                 1.2e-13                 1.6e-6
       fluxes_lin                      2.3e-15                 9.7e-7
       ss_lin, ss_rrs_lin              1.1e-14                 2.4e-7
       raman                           6.2e-15                 0
       multisensor_raman               8.0e-15                 0
       fluxes_raman                    0                       0
       The Legendre, spline and bare-albedo cells: 0 in every forward driver, <= 2.4e-15 in the linearized ones; spline against
       Legendre: 0 everywhere.  The 1e-13 of the linearized RPV / Ross-Li cells is the 100-node azimuth quadrature of
       vsm_land_brdf_reflectance_lin_* on the device against the closed-form albedo column (the CPU oracle shows 3e-15 for the
       forward identity, which the forward cells repeat).
  (b)  RPV: <= 1.4e-13 in all five drivers.  Cox-Munk: <= 1.1e-13, and 1.2e-9 in R of CoreRTRaman.rt_run (per Stokes component
       1.1e-8), where the single-scattering correction is the oracle's own; REDUCE_M0 on against off 0 (Cox-Munk), 3.8e-16 (RPV,
       IQU shape).
  Without the change to the surface step of the Raman drivers the RPV and Ross-Li cells of all three miss by 1.22 of the signal
  and their Legendre and spline cells raise VSMError.
"""
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import driver_surface_cases as DS  # noqa: E402
import flux_lin_oracle as FL  # noqa: E402
import flux_oracle as FO  # noqa: E402
import flux_raman_oracle as FRO  # noqa: E402
import ms_raman_oracle as MR  # noqa: E402
import test_gpu_multisensor_raman as TMR  # noqa: E402
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
from oracle import vsm_oracle_raman as OR  # noqa: E402

pytestmark = pytest.mark.gpu

FP64, FP32 = np.float64, np.float32
FLUX_FIELDS = FO.FIELDS
FLUX_IE_FIELDS = FRO.IE_FIELDS

# driver -> (FP64 bound, FP32 bound, where the sibling has them)
BOUNDS = {
    "rt_run": (1e-9, 2e-3, "test_gpu_parity: the small scenes against O.rt_run"),
    "rt_run_full": (1e-9, 2e-3, "test_rt_run_full_output_hdrf_bhr"),
    "multisensor": (1e-10, 2e-3, "test_gpu_multisensor: max(1e-10, ...) / test_multisensor_float32"),
    "fluxes": (1e-11, 2e-3, "test_gpu_fluxes: 1e-11 / test_fluxes_float32"),
    "ss": (1e-8, 1e-2, "test_gpu_ss.TOL_RUN"),
    "lin": (1e-8, 1e-2, "test_gpu_lin: Rdot, Tdot 1e-8 (R, T: 1e-9, LIN_FORWARD) / test_rt_run_lin_fp32"),
    "multisensor_lin": (1e-8, 2e-2, "test_gpu_multisensor_lin"),
    "fluxes_lin": (1e-8, 2e-2, "test_gpu_fluxes_lin"),
    "ss_lin": (1e-8, 1e-2, "test_gpu_ss_lin.TOL_RUN"),
    "raman": (1e-8, 1e-2, "test_gpu_raman: the runs against OR.rt_run_rrs"),
    "multisensor_raman": (1e-8, 1e-2, "test_gpu_multisensor_raman.test_device_vs_prototype"),
    "fluxes_raman": (1e-8, 1e-2, "test_gpu_fluxes_raman"),
    "ss_rrs": (1e-8, 1e-2, "test_gpu_ss.TOL_RUN"),
    "ss_rrs_lin": (1e-8, 1e-2, "test_gpu_ss_raman_lin (test_gpu_ss_lin.TOL_RUN)"),
}
LIN_FORWARD = 1e-9      # R, T of CoreRTLin.rt_run_lin in FP64 (test_gpu_lin)
LIN_DRIVERS = ("lin", "multisensor_lin", "fluxes_lin", "ss_lin", "ss_rrs_lin")
# the surfaces of (a), in the issue's order: (id, NSurf, the surface column that is the albedo's)
SURFACES = [("lambertian", 1, "albedo"), ("rpv", 4, "rho0"), ("rossli", 3, "fiso"), ("legendre", 2, "c0"),
            ("spline", 1, "albedo_dot[0]"), ("albedo", 1, "albedo")]
SPECTRAL = ("legendre", "spline")


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def test_the_raman_lines_are_the_siblings():
    assert np.array_equal(DS.SHIFTS, TMR.SHIFTS) and np.array_equal(DS.W_IE, TMR.W_IE)


# ---- models ------------------------------------------------------------------------------------------------------------------------
def _surface(vsm, kind):
    H = vsm.host_model
    a = DS.A
    return {"lambertian": lambda: H.LambertianSurfaceScalar(a), "rpv": lambda: H.rpvSurfaceScalar(a, 1.0, 1.0, 0.0),
            "rossli": lambda: H.RossLiSurfaceScalar(0.0, 0.0, a), "legendre": lambda: H.LambertianSurfaceLegendre([a, 0.0]),
            "spline": lambda: H.LambertianSurfaceSpline([a] * DS.S), "albedo": lambda: None,
            "rpv_real": lambda: H.rpvSurfaceScalar(*DS.RPV), "coxmunk": lambda: H.CoxMunkSurface(wind_speed=DS.WIND)}[kind]()


def _host_model(vsm, arch, pol, l_trunc, FT, kind, aerosol=False):
    """The scene of driver_surface_cases over the surface `kind`, with albedo = ALBEDO_FIELD passed beside the surface object (the
    bare-albedo cell: a; the spline cell: the default, 0)."""
    H = vsm.host_model
    albedo = {"albedo": DS.A, "spline": 0.0}.get(kind, DS.ALBEDO_FIELD)
    kw = DS.model_kwargs(pol, albedo)
    aer = []
    if aerosol:
        kw["tau_aer"] = DS.AER_TAU
        aer = [H.AerosolOptics(H.GreekCoefs(**vars(DS.aerosol_greek())), DS.AER_SSA, DS.AER_FTRUNC)]
    pm = H.model_from_arrays(arch, pol, l_trunc, DS.SZA, list(DS.VZA), list(DS.VAZ), float_type=FT, surface=_surface(vsm, kind),
                             aerosol_optics=aer, **kw)
    pm.varpi_Cabannes = DS.VARPI_CABANNES
    pm.F0 = DS.arrays(pol)[2]
    # (RTModel copies the albedo of a LambertianSurfaceScalar into the field; every other surface leaves what was passed)
    assert pm.albedo == (DS.A if kind == "lambertian" else albedo)
    return pm


def _host_lin(vsm, pol, aerosol):
    H = vsm.host_model
    gases, tad, aer = DS.lin_tables(pol, aerosol)
    if not aerosol:
        return H.LinModel(gases), 0, len(gases)
    gdot, ssa_dot, f_dot = aer
    lao = [H.LinAerosolOptics([H.GreekCoefs(**vars(g)) for g in gdot], ssa_dot, f_dot)]
    return H.LinModel(gases, tau_aer_dot=tad, lin_aerosol_optics=lao), 1, len(gases)


def _host_rs(vsm):
    return TMR._rs(vsm, DS.SHIFTS, DS.W_IE)[1]


# ---- the drivers: name -> [(output name, array, kind, down)] ------------------------------------------------------------------------
# kind: "rad" [nVZA, nStokes, nSpec], "rad_dot" [nVZA, nStokes, nSpec, P], "flux" [nLevels, nSpec] (or any array measured as a
# whole), "flux_dot" [nLevels, nSpec, P]; down: J0+ of the composite that includes the surface layer (see the module docstring)
def _levels(names, lists, downs):
    out = []
    for name, lst, down0 in zip(names, lists, downs):
        kind = "rad_dot" if lst[0].ndim == 4 else "rad"
        out += [("%s[level %d]" % (name, l), x, kind, down0 and l == 0) for l, x in zip(DS.LEVELS, lst)]
    return out


def _flux_outputs(res, fields, dot=False):
    out = [(k, getattr(res, k), "flux", False) for k in fields]
    if dot:
        out += [(k + "_dot", getattr(res, k + "_dot"), "flux_dot", False) for k in FO.FIELDS]
    return out


def _run(vsm, driver, pm, lin=None):
    CR, CL, RR = vsm.CoreRT, vsm.CoreRTLin, vsm.CoreRTRaman
    if lin is not None:
        hl, naer, ngas, nsurf = lin
    if driver == "rt_run":
        R, T = CR.rt_run(pm)
        out = [("R", R, "rad", False), ("T", T, "rad", True)]
    elif driver == "rt_run_full":
        R, T, ieR, ieT, hdr, bhr_uw, bhr_dw = CR.rt_run(pm, full_output=True)
        out = [("R", R, "rad", False), ("T", T, "rad", True), ("hdr", hdr, "rad", False), ("bhr_uw", bhr_uw, "flux", False),
               ("bhr_dw", bhr_dw, "flux", True)]
    elif driver == "multisensor":
        out = _levels(("uw", "dw"), CR.rt_run_multisensor(pm, DS.LEVELS), (False, True))
    elif driver == "fluxes":
        out = _flux_outputs(CR.rt_run_fluxes(pm, DS.LEVELS), FLUX_FIELDS)
    elif driver == "ss":
        got = CR.rt_run_ss(pm)
        out = [("R1", got[0], "rad", False), ("T1", got[1], "rad", False)]
    elif driver == "lin":
        R, T, Rd, Td = CL.rt_run_lin(pm, hl, naer, ngas, nsurf)
        out = [("R", R, "rad", False), ("T", T, "rad", True), ("Rdot", Rd, "rad_dot", False), ("Tdot", Td, "rad_dot", True)]
    elif driver == "multisensor_lin":
        out = _levels(("uw", "dw", "uw_dot", "dw_dot"), CL.rt_run_multisensor(pm, hl, naer, ngas, nsurf, DS.LEVELS),
                      (False, True, False, True))
    elif driver == "fluxes_lin":
        out = _flux_outputs(CL.rt_run_fluxes(pm, hl, naer, ngas, nsurf, DS.LEVELS), FLUX_FIELDS, dot=True)
    elif driver == "ss_lin":
        R, T, Rd, Td = CL.rt_run_ss(pm, hl, naer, ngas, nsurf)
        out = [("R1", R, "rad", False), ("T1", T, "rad", False), ("R1dot", Rd, "rad_dot", False), ("T1dot", Td, "rad_dot", False)]
    elif driver == "raman":
        R, T, ieR, ieT = RR.rt_run(_host_rs(vsm), pm, 1)
        out = [("R", R, "rad", False), ("T", T, "rad", True), ("ieR", ieR, "rad", False), ("ieT", ieT, "rad", True)]
    elif driver == "multisensor_raman":
        out = _levels(("uw", "dw", "uwie", "dwie"), RR.rt_run_multisensor(_host_rs(vsm), pm, DS.LEVELS), (False, True, False, True))
    elif driver == "fluxes_raman":
        out = _flux_outputs(RR.rt_run_fluxes(_host_rs(vsm), pm, DS.LEVELS), FLUX_FIELDS + FLUX_IE_FIELDS)
    elif driver == "ss_rrs":
        got = RR.rt_run_ss(_host_rs(vsm), pm, 1)
        out = [(k, x, "rad", False) for k, x in zip(("R1", "T1", "ieR1", "ieT1"), got)]
    elif driver == "ss_rrs_lin":
        got = RR.rt_run_ss_lin(_host_rs(vsm), pm, hl, naer, ngas, nsurf)
        out = ([(k, x, "rad", False) for k, x in zip(("R1", "T1", "ieR1", "ieT1"), got[:4])]
               + [(k, x, "rad_dot", False) for k, x in zip(("R1dot", "T1dot", "ieR1dot", "ieT1dot"), got[4:])])
    else:
        raise KeyError(driver)
    torch.cuda.synchronize()
    vsm._lib.check_device_status("driver grid: %s" % driver)      # (d)
    for name, x, _, _ in out:
        assert x.dtype == pm.float_type, (driver, name, x.dtype)
    return out


def _run_cell(vsm, arch, driver, pol, l_trunc, FT, kind, nsurf):
    is_lin = driver in LIN_DRIVERS
    pm = _host_model(vsm, arch, pol, l_trunc, FT, kind, aerosol=is_lin)
    lin = None
    if is_lin:
        hl, naer, ngas = _host_lin(vsm, pol, True)
        lin = (hl, naer, ngas, nsurf)
    return pm, _run(vsm, driver, pm, lin)


# ---- the measure -------------------------------------------------------------------------------------------------------------------
def _err(g, r, kind, per_component, tol):
    """max |g - r| relative to the largest |r|: of the array (a parameter column at a time), or per Stokes component of it.  A
    component whose largest reference value is below tol times the array's carries nothing the bound could resolve (U just above a
    Cox-Munk surface at nadir: 1e-13 of I, the rounding of the reflectance blocks): its error is taken relative to the array's
    largest value, as the siblings do with a component that is exactly zero.  No reference value at all: the absolute error."""
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    cols = [(g[..., p], r[..., p]) for p in range(r.shape[-1])] if kind.endswith("_dot") else [(g, r)]
    worst = 0.0
    for gc, rc in cols:
        whole = float(np.max(np.abs(rc))) if rc.size else 0.0
        parts = [(gc[:, k], rc[:, k]) for k in range(rc.shape[1])] if kind.startswith("rad") and per_component else [(gc, rc)]
        for gk, rk in parts:
            e = float(np.max(np.abs(gk - rk))) if rk.size else 0.0
            sc = float(np.max(np.abs(rk))) if rk.size else 0.0
            sc = sc if sc > tol * whole else whole
            worst = max(worst, e / sc if sc > 0 else e)
    return worst


def _compare(driver, FT, got, ref, got_slot, ref_slot, pl, skip_down):
    """The worst error of the outputs `got` of a cell against those of the reference cell: forward outputs whole, derivative
    outputs on the pl layer columns and on the one surface column (got_slot against ref_slot); the other columns finite."""
    per_component = FT == FP64 or driver in ("multisensor", "multisensor_raman")
    worst, compared = 0.0, 0
    for (name, g, kind, down), (rname, r, _, _) in zip(got, ref):
        assert name == rname and np.all(np.isfinite(g)), (driver, name)
        if down and skip_down:
            continue
        if kind.endswith("_dot"):
            assert g.shape[-1] > got_slot and r.shape[-1] > ref_slot
            g = np.concatenate([g[..., :pl], g[..., got_slot:got_slot + 1]], axis=-1)
            r = np.concatenate([r[..., :pl], r[..., ref_slot:ref_slot + 1]], axis=-1)
        tol = BOUNDS[driver][0 if FT == FP64 else 1]
        if driver == "lin" and FT == FP64 and not kind.endswith("_dot"):
            tol = LIN_FORWARD
        e = _err(g, r, kind, per_component, tol)
        assert e <= tol, (driver, name, e, tol)
        worst, compared = max(worst, e), compared + 1
    assert compared > 0
    return worst


def _slots(vsm, pm, column, nsurf, pl):
    names = vsm.CoreRTLin.surface_param_names(pm.surface)
    assert len(names) == nsurf
    return pl + names.index(column)


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
_cells = {}


def _cell(vsm, arch, driver, pol, l_trunc, FT, kind):
    """(outputs, the slot of the albedo's column) of one cell; the Lambertian and the Legendre cell, which others are compared
    with, are run once and only read."""
    key = (driver, pol, FT, kind)
    if key in _cells:
        return _cells[key]
    nsurf, column = {k: (n, c) for k, n, c in SURFACES}[kind]
    pl = 7 + 2 if driver in LIN_DRIVERS else 0
    pm, out = _run_cell(vsm, arch, driver, pol, l_trunc, FT, kind, nsurf)
    cell = (out, _slots(vsm, pm, column, nsurf, pl) if pl else 0, pl)
    if kind in ("lambertian", "legendre"):
        _cells[key] = cell
    return cell


GRID = ([(d, p, l, FP64, k) for d in BOUNDS for p, l in DS.SHAPES for k, _, _ in SURFACES[1:]]
        + [(d, p, l, FP32, "rpv") for d in BOUNDS for p, l in DS.SHAPES])


@pytest.mark.parametrize("driver,pol,l_trunc,FT,kind", GRID,
                         ids=["%s-%s-%s-%s" % (d, p, "fp64" if f == FP64 else "fp32", k) for d, p, l, f, k in GRID])
def test_degenerate_surface_equals_lambertian(vsm, arch, driver, pol, l_trunc, FT, kind):
    """(a), one cell: the driver over surface `kind` against the same driver over LambertianSurfaceScalar(a) -- FP64 over all five
    other surfaces, FP32 over the RPV cell.  The spline cell also against the Legendre cell, with the outputs the spectral cells
    leave out against the scalar one (the two share a builder)."""
    ref, ref_slot, pl = _cell(vsm, arch, driver, pol, l_trunc, FT, "lambertian")
    got, slot, _ = _cell(vsm, arch, driver, pol, l_trunc, FT, kind)
    worst = {kind: _compare(driver, FT, got, ref, slot, ref_slot, pl, skip_down=kind in SPECTRAL)}
    if kind == "spline":
        leg, leg_slot, _ = _cell(vsm, arch, driver, pol, l_trunc, FT, "legendre")
        worst["spline/legendre"] = _compare(driver, FT, got, leg, slot, leg_slot, pl, skip_down=False)
    print("GRID (a) %-18s %-3s %s: %s" % (driver, pol, "fp64" if FT == FP64 else "fp32",
                                          "  ".join("%s %.1e" % kv for kv in worst.items())))


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
BRDF_CASES = [("rpv_real", "I", 9), ("coxmunk", "IQU", 7)]


def _oracle_surface(kind):
    return OB.RPVSurface(*DS.RPV) if kind == "rpv_real" else CM.CoxMunkSurface(DS.WIND)


_oracle_runs = {}


def _oracle(vsm, arch, pm, kind, pol, l_trunc, what):
    """The oracle's run `what` of the (b) scene, computed once and only read.  RPV: the oracle's own Fourier blocks.  Cox-Munk: the
    device's blocks, as in test_gpu_multisensor.test_multisensor_brdf_surfaces (test_gpu_coxmunk.py pins them against the oracle's
    to ~1e-9, which the flux bound of 1e-11 would show undamped; with the oracle's own blocks CoreRTRaman.rt_run measured 1.1e-9):
    the drivers are under test here.  The single-scattering correction of R is the oracle's own in either case."""
    key = (kind, what)
    if key not in _oracle_runs:
        om = DS.oracle_model(pol, l_trunc, albedo=DS.ALBEDO_FIELD)
        if kind == "coxmunk":
            dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, FP64)
            refl = lambda m: vsm.Architectures.to_host(vsm.CoreRT.reflectance(pm.surface, dq, m, arch, FP64)[0]).T.copy()
            hook = CM.surface_layer_hook(om, refl, coxmunk=_oracle_surface(kind))
        else:
            mu = om.quad_points.qp_mu.astype(np.float64)
            refl = lambda m: OB.reflectance(_oracle_surface(kind), om.pol.n, mu, m)
            hook = DS.brdf_hook(om, _oracle_surface(kind))

        def fluxes_lin():
            # the linearized surface builders carry the beam as F0 where the forward ones carry I0 = e1 (core_rt_ss.rt_run_ss_lin's
            # docstring; this scene's F0 varies along the band), so the forward fields of the linearized run have the linearized
            # oracle as their reference: its surface hook m -> (rho, drho), the derivative block not compared (zeros)
            ol = OL.LinModel(DS.lin_tables(pol, False)[0])
            return FL.fluxes_lin(om, ol, DS.LEVELS, solar_surface=lambda m: (refl(m), np.zeros_like(refl(m))))
        _oracle_runs[key] = {
            "raman": lambda: OR.rt_run_rrs(om, DS.oracle_rs(), surface=hook),
            "multisensor_raman": lambda: MR.ms_raman_reference(om, DS.oracle_rs(), DS.LEVELS, surface=hook),
            "fluxes_raman": lambda: FRO.fluxes_raman_reference(om, DS.oracle_rs(), DS.LEVELS, surface=hook),
            "fluxes": lambda: FO.fluxes_reference(om, DS.LEVELS, surface=hook), "fluxes_lin": fluxes_lin}[what]()
    return _oracle_runs[key]


@pytest.mark.parametrize("kind,pol,l_trunc", BRDF_CASES, ids=[c[0] for c in BRDF_CASES])
@pytest.mark.parametrize("driver", ["raman", "multisensor_raman", "fluxes_raman", "fluxes", "fluxes_lin"])
def test_brdf_surfaces_against_the_oracles(vsm, arch, monkeypatch, driver, kind, pol, l_trunc):
    """(b): the device over a real BRDF against the oracle with that BRDF's surface hook, at the sibling's bound (FP64); forward
    fields only for CoreRTLin.rt_run_fluxes.  Cox-Munk in CoreRTRaman.rt_run: REDUCE_M0 on and off within the same bound."""
    pm = _host_model(vsm, arch, pol, l_trunc, FP64, kind)
    lin = None
    if driver == "fluxes_lin":
        hl, naer, ngas = _host_lin(vsm, pol, False)
        lin = (hl, naer, ngas, 4 if kind == "rpv_real" else 1)
    got = _run(vsm, driver, pm, lin)
    tol = BOUNDS[driver][0]
    if driver == "raman":
        ref = list(zip(("R", "T", "ieR", "ieT"), _oracle(vsm, arch, pm, kind, pol, l_trunc, "raman")))
    elif driver == "multisensor_raman":
        r = _oracle(vsm, arch, pm, kind, pol, l_trunc, "multisensor_raman")
        ref = [("%s[level %d]" % (n, l), x) for n, lst in zip(("uw", "dw", "uwie", "dwie"), r) for l, x in zip(DS.LEVELS, lst)]
    elif driver == "fluxes_raman":
        r = _oracle(vsm, arch, pm, kind, pol, l_trunc, "fluxes_raman")
        ref = [(k, getattr(r, k)) for k in FLUX_FIELDS + FLUX_IE_FIELDS]
    else:
        r = _oracle(vsm, arch, pm, kind, pol, l_trunc, driver)
        ref = [(k, getattr(r, k)) for k in FLUX_FIELDS]
    # the sibling's measure: per Stokes component in test_gpu_multisensor_raman, per array in test_gpu_raman, per field in the flux files
    per_component = driver == "multisensor_raman"
    worst = strict = 0.0
    for (name, g, okind, _), (rname, r) in zip(got, ref):      # (zip: the derivative fields of fluxes_lin come after the forward ones)
        assert name == rname
        assert float(np.max(np.abs(r))) > 0, name
        e = _err(g, r, okind, per_component, tol)
        worst, strict = max(worst, e), max(strict, _err(g, r, okind, True, tol))
        assert e <= tol, (driver, kind, name, e, tol)
    print("GRID (b) %-18s %-8s: %.1e (bound %.0e; per Stokes component %.1e)" % (driver, kind, worst, tol, strict))
    if driver == "raman" and pol == "IQU":
        monkeypatch.setattr(vsm.CoreRTRaman, "REDUCE_M0", False)
        off = _run(vsm, driver, pm)
        e = max(_err(a[1], b[1], "rad", False, tol) for a, b in zip(got, off))
        print("GRID (b) raman %s REDUCE_M0 on vs off: %.1e" % (kind, e))
        assert e <= tol, e


def test_raman_reduce_m0_over_a_scalar_brdf(vsm, arch, monkeypatch):
    """The Stokes_IQ reduction of m = 0 stays on over a surface that reflects I into I only: the RPV surface of (b) under the IQU
    shape, REDUCE_M0 on (the sub-scene is there) against off, at the driver's bound."""
    pol, l_trunc = DS.SHAPES[1]
    pm = _host_model(vsm, arch, pol, l_trunc, FP64, "rpv_real")
    RR = vsm.CoreRTRaman
    assert RR.SceneRRS(_host_rs(vsm), pm, 1).sub0 is not None
    assert RR.SceneRRS(_host_rs(vsm), _host_model(vsm, arch, pol, l_trunc, FP64, "coxmunk"), 1).sub0 is None
    on = _run(vsm, "raman", pm)
    monkeypatch.setattr(RR, "REDUCE_M0", False)
    assert RR.SceneRRS(_host_rs(vsm), pm, 1).sub0 is None
    off = _run(vsm, "raman", pm)
    e = max(_err(a[1], b[1], "rad", True, BOUNDS["raman"][0]) for a, b in zip(on, off))
    print("GRID raman rpv IQU REDUCE_M0 on vs off: %.1e" % e)
    assert e <= BOUNDS["raman"][0], e


def test_surface_sif_warns_once_over_a_brdf_in_the_raman_run(vsm, arch):
    """SurfaceSIF has no effect over a non-Lambertian surface and says so once, as in CoreRT.rt_run: the run is the run without it."""
    H = vsm.host_model
    pol, l_trunc = DS.SHAPES[0]
    pm = _host_model(vsm, arch, pol, l_trunc, FP64, "rpv_real")
    base = vsm.CoreRTRaman.rt_run(_host_rs(vsm), pm, 1)
    pm.sources = (H.SolarBeam(), H.SurfaceSIF(np.full(DS.S, 1e-2)))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = vsm.CoreRTRaman.rt_run(_host_rs(vsm), pm, 1)
    assert len([x for x in w if "SurfaceSIF has no effect" in str(x.message)]) == 1
    assert all(np.array_equal(a, b) for a, b in zip(got, base))


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol,l_trunc", DS.SHAPES, ids=["I_n8", "IQU_n21"])
def test_raman_legendre_blocks_and_slices_are_bit_identical(vsm, arch, pol, l_trunc):
    """(c), after test_rt_run_rrs_blocked_equals_one_pass / _halo_shard_equals_full: blocks of 5 points with their halos, and the
    slice 4..9, over an albedo that varies along the band -- an albedo spectrum cut by the owned range instead of the extended one
    shows here."""
    H = vsm.host_model
    pm = _host_model(vsm, arch, pol, l_trunc, FP64, "legendre")
    pm.surface = H.LambertianSurfaceLegendre(list(DS.LEGENDRE))
    alb = H.surface_albedo_spectrum(pm.surface, DS.S)
    assert np.ptp(alb) > 0.1
    prs = _host_rs(vsm)
    full = vsm.CoreRTRaman.rt_run(prs, pm, 1)
    blk = vsm.CoreRTRaman.rt_run(prs, pm, 1, max_points=5)
    part = vsm.CoreRTRaman.rt_run(prs, pm, 1, spec_slice=slice(4, 10))
    torch.cuda.synchronize()
    vsm._lib.check_device_status("driver grid: raman blocks")
    for name, f, b, p in zip(("R", "T", "ieR", "ieT"), full, blk, part):
        assert np.max(np.abs(f)) > 0 and f.shape == b.shape and p.shape[2] == 6, name
        assert np.array_equal(f, b), (name, "max_points=5")
        assert np.array_equal(p, f[:, :, 4:10]), (name, "spec_slice")
    # the surface is seen: the same run over the band's mean albedo is another run
    pm.surface = H.LambertianSurfaceLegendre([float(np.mean(alb)), 0.0])
    flat = vsm.CoreRTRaman.rt_run(prs, pm, 1)
    assert DS.rel_max(flat[0], full[0]) > 1e-2
