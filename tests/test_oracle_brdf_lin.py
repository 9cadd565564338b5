"""CPU checks of tests/brdf_lin_oracle.py, the oracle of the RPV / Ross-Li surface Jacobians (NSurf = 4 / 3): the analytic parameter
derivatives of the Fourier reflectance blocks and the TOA Jacobians built on them against central differences of the forward oracle
(oracle/vsm_oracle_brdf.py), and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

import brdf_lin_oracle as B
from oracle import vsm_oracle_brdf as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
MOMENTS = (0, 1, 3)
RPV_STEPS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7)
RPV_DRHO_BOUND = 10 * 8.6e-11


def _mu():
    return B.oracle_scene("I")[0].quad_points.qp_mu.astype(np.float64)


def _central(surf, k, h, n_stokes, mu, m):
    return (OB.reflectance(B.perturbed(surf, k, h), n_stokes, mu, m) - OB.reflectance(B.perturbed(surf, k, -h), n_stokes, mu, m)) / (2 * h)


@pytest.mark.parametrize("name", ["rpv", "rossli"])
@pytest.mark.parametrize("n_stokes", [1, 3])
def test_forward_block_is_the_oracles_and_only_I_to_I(name, n_stokes):
    """reflectance_and_deriv's forward block is OB.reflectance (the same quadrature, statement for statement); the derivative
    blocks live on the I -> I elements only."""
    surf, mu = B.SURFACES[name], _mu()
    for m in MOMENTS:
        R, dR = B.reflectance_and_deriv(surf, n_stokes, mu, m)
        Ro = OB.reflectance(surf, n_stokes, mu, m)
        assert np.max(np.abs(R - Ro)) <= 4 * EPS * np.max(np.abs(Ro))
        assert dR.shape == (B.n_params(surf),) + R.shape
        mask = np.ones(R.shape, dtype=bool)
        mask[0::n_stokes, 0::n_stokes] = False
        assert np.all(dR[:, mask] == 0) and np.all(R[mask] == 0)


def test_rossli_drho_equals_the_difference_quotient_to_rounding():
    """Ross-Li is linear in its weights, so the central difference quotient of OB.reflectance IS the derivative, up to rounding: each
    table is a sum of 100 rounded terms whose magnitudes add up to about the m = 0 table (the factor cos(m phi) only signs them):
    error at most 100 eps ff max |R(m = 0)|, and the quotient divides the difference of two tables by 2 h."""
    surf, mu = B.SURFACES["rossli"], _mu()
    h = 1e-2
    scale = 2 * np.max(np.abs(B.reflectance_and_deriv(surf, 1, mu, 0)[0]))
    for m in MOMENTS:
        R, dR = B.reflectance_and_deriv(surf, 1, mu, m)
        for k in range(3):
            fd = _central(surf, k, h, 1, mu, m)
            bound = 100 * EPS * scale / h + 4 * EPS * np.max(np.abs(dR[k]))
            err = float(np.max(np.abs(fd - dR[k])))
            print("Ross-Li m %d slot %d: |fd - analytic| %.2e (bound %.2e)" % (m, k, err, bound))
            assert err <= bound, (m, k, err, bound)


def test_rpv_drho_against_central_differences():
    """RPV, every parameter, m = 0, 1, 3: the best agreement of the analytic block with the central difference quotient of
    OB.reflectance over the steps 1e-2 .. 1e-7, relative to max |analytic block|.

    Measured on this CPU (the worst slot of each parameter over the three moments, with the step that gave it):
        rho0   3.5e-15 (1e-2: linear, rounding only)    rho_c  1.2e-13 (1e-2: linear)
        k      4.0e-11 (1e-6)                           Theta  8.6e-11 (1e-6)
    Bound: ten times the worst, 8.6e-10."""
    surf, mu = B.SURFACES["rpv"], _mu()
    for m in MOMENTS:
        _, dR = B.reflectance_and_deriv(surf, 1, mu, m)
        for k, pname in enumerate(B.param_names(surf)):
            errs = [float(np.max(np.abs(_central(surf, k, h, 1, mu, m) - dR[k])) / np.max(np.abs(dR[k]))) for h in RPV_STEPS]
            print("RPV m %d d/d%-5s: %s" % (m, pname, " ".join("%.1e" % e for e in errs)))
            assert min(errs) <= RPV_DRHO_BOUND, (m, pname, errs)


def test_fiso_moments_are_exactly_zero_and_rho0_slot_is_finite_at_zero():
    mu = _mu()
    for m in (1, 2, 3):
        _, dR = B.reflectance_and_deriv(B.SURFACES["rossli"], 3, mu, m)
        assert np.all(dR[2] == 0) and np.max(np.abs(dR[0])) > 0 and np.max(np.abs(dR[1])) > 0
    _, dR0 = B.reflectance_and_deriv(B.SURFACES["rossli"], 1, mu, 0)
    assert np.max(np.abs(dR0[2] - 1.0)) <= 4 * EPS          # (1 / pi) int_0^pi d phi
    black = OB.RPVSurface(0.0, 0.08, 0.75, -0.25)
    for m in MOMENTS:
        R, dR = B.reflectance_and_deriv(black, 1, mu, m)
        assert np.all(R == 0) and np.all(np.isfinite(dR)) and np.max(np.abs(dR[0])) > 0
        assert np.all(dR[1:] == 0)                           # the other three carry the factor rho0
        want = B.reflectance_and_deriv(B.SURFACES["rpv"], 1, mu, m)[1][0]
        assert np.max(np.abs(dR[0] - want)) <= 4 * EPS * np.max(np.abs(want))    # M F H does not depend on rho0


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("name", ["rpv", "rossli"])
def test_toa_jacobian_against_central_differences(pol, name):
    """rt_run_lin's surface slots against central differences of OB.rt_run at B.FD_STEP on the small scene, relative to each slot's
    maximum: the finite-difference floor B.FD_FLOOR that the device test reuses.  R, T of the linearized run are OB.rt_run's (with
    F0[0] = 1 the linearized builder's F0 and the forward builder's I0 weigh the beam alike on a scalar BRDF; the viewing rows do
    not see the builders' different j0+ and t--); the K-slot run equals the assembly of K one-slot runs; the gas slot matches
    too."""
    om, ol = B.oracle_scene(pol)
    surf = B.SURFACES[name]
    K, pl = B.n_params(surf), ol.n_layer_params
    R, T, Rd, Td = B.rt_run_lin(om, ol, surf)
    assert Rd.shape == R.shape + (pl + K,)
    Rf, Tf = OB.rt_run(om, surf)
    assert np.max(np.abs(R - Rf)) <= 1e-13 * np.max(np.abs(Rf)) and np.max(np.abs(T - Tf)) <= 1e-13 * np.max(np.abs(Tf))
    for a, b in zip((R, T, Rd, Td), B.rt_run_lin_by_slots(om, ol, surf)):
        assert np.array_equal(a, b)
    h = B.FD_STEP
    worst = 0.0
    for k in range(K):
        up, dn = OB.rt_run(om, B.perturbed(surf, k, h)), OB.rt_run(om, B.perturbed(surf, k, -h))
        for an, a, b in ((Rd[..., pl + k], up[0], dn[0]), (Td[..., pl + k], up[1], dn[1])):
            assert np.max(np.abs(an)) > 0
            e = float(np.max(np.abs((a - b) / (2 * h) - an)) / np.max(np.abs(an)))
            worst = max(worst, e)
    print("%s %s: finite-difference floor %.3e at h = %g" % (pol, name, worst, h))
    assert worst <= B.FD_FLOOR, worst
    # the gas slot: the absorption scaled as a whole
    import dataclasses
    g = ol.tau_abs_dot[0]
    e = 1e-4
    up = OB.rt_run(dataclasses.replace(om, tau_abs=om.tau_abs + e * g), surf)
    dn = OB.rt_run(dataclasses.replace(om, tau_abs=om.tau_abs - e * g), surf)
    for an, a, b in ((Rd[..., 0], up[0], dn[0]), (Td[..., 0], up[1], dn[1])):
        assert np.max(np.abs((a - b) / (2 * e) - an)) <= 1e-6 * np.max(np.abs(an))


def test_single_scattering_and_multisensor_assemblies_have_the_slots():
    """The K-slot assemblies of the one-slot oracles: shapes, the layer slot shared, level 0 of the multi-sensor run = rt_run_lin."""
    om, ol = B.oracle_scene("I")
    surf = B.SURFACES["rossli"]
    R, T, Rd, Td = B.rt_run_ss_lin(om, ol, surf)
    assert Rd.shape == R.shape + (4,) and np.all(Td[..., 1:] == 0) and all(np.max(np.abs(Rd[..., p])) > 0 for p in range(4))
    uw, dw, uwd, dwd = B.ms_lin_segmented(om, ol, [0, 3], surf)
    full = B.rt_run_lin(om, ol, surf)
    for a, b in zip((uw[0], dw[0], uwd[0], dwd[0]), full):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
    assert uwd[1].shape == uw[1].shape + (4,)


def test_header_declares_the_new_entry_points():
    """include/vsmartmom_hip.h declares the four new symbols, and the ctypes table binds them with as many arguments."""
    import vsmartmom_jl_amd as vsm
    header = open(os.path.join(ROOT, "include", "vsmartmom_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = set(vsm._lib.exported_symbols())
    for base, nargs in (("vsm_land_brdf_reflectance_lin", 10), ("vsm_brdf_surface_lin_multi", 14)):
        for sfx in ("f64", "f32"):
            mt = re.search(r"\bint\s+%s_%s\s*\(([^;]*?)\)\s*;" % (base, sfx), header, flags=re.S)
            assert mt, (base, sfx)
            assert len(mt.group(1).split(",")) == nargs
            assert "%s_%s" % (base, sfx) in bound
        assert len(vsm._lib._SIGS[base + "_{T}"][1]) == nargs
    assert re.search(r"#define\s+VSM_LAND_BRDF_RPV\s+0", header) and re.search(r"#define\s+VSM_LAND_BRDF_ROSSLI\s+1", header)
