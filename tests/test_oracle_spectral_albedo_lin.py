"""CPU checks of tests/spectral_albedo_lin_oracle.py, the oracle of the albedo Jacobians of LambertianSurfaceLegendre /
LambertianSurfaceSpline: its builder's forward half is the forward oracle's, its run reproduces O.rt_run with the array albedo, every
slot agrees with central differences of that forward run (which measures FD_FLOOR), and in R slot k is basis[k, s] times the albedo
slot of OL.rt_run_lin run per point with that point's scalar albedo.  No GPU."""
import os
import re

import numpy as np
import pytest

import spectral_albedo_lin_oracle as A
from oracle import vsm_oracle as O
from oracle import vsm_oracle_lin as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_builder_forward_half_is_the_forward_builder(pol):
    """At F0 = e1 the forward half equals O.create_surface_layer_lambertian_spectral exactly, m = 0 and m = 2; every derivative
    block is zero for m > 0, and at m = 0 the slots are linear in their tables: the K = 1 slot with basis = albedo is the forward
    layer itself."""
    om, ol, basis = A.oracle_scene(pol)
    FT, p, qp = np.float64, om.pol, om.quad_points
    S, N = A.S_POINTS, om.quad_points.Nquad * om.pol.n
    rng = np.random.default_rng(3)
    tau_sum, tsd = rng.uniform(0.05, 2.0, S), rng.standard_normal((S, 2))
    F0 = np.zeros((p.n, S))
    F0[0] = 1
    for m in (0, 2):
        a, b = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
        al = OL.make_added_layer_lin(FT, 6, N, S)
        for t in (al.ap_r_mp, al.ap_r_pm, al.ap_t_pp, al.ap_t_mm, al.ap_J0_p, al.ap_J0_m, a.r_pm):
            t[...] = np.nan
        A.create_surface_layer_spectral_lin(om.albedo, basis, a, al, 3, m, p, qp, tau_sum, tsd, F0, FT)
        O.create_surface_layer_lambertian_spectral(om.albedo, b, m, p, qp, tau_sum, FT)
        for f in ("r_mp", "r_pm", "t_pp", "t_mm", "j0_p", "j0_m"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (m, f)
        stacks = (al.ap_r_mp, al.ap_r_pm, al.ap_t_pp, al.ap_t_mm, al.ap_J0_p, al.ap_J0_m)
        assert all(np.all(np.isfinite(t)) for t in stacks)
        if m > 0:
            assert all(np.all(t == 0) for t in stacks)
            continue
        assert all(np.all(t == 0) for t in (al.ap_r_pm, al.ap_t_pp, al.ap_t_mm, al.ap_J0_p))
        assert np.all(al.ap_r_mp[:3] == 0) and np.all(al.ap_J0_m[2] == 0)
        for q in (0, 1):
            assert np.array_equal(al.ap_J0_m[q], -a.j0_m * (tsd[:, q] / qp.mu0)[:, None]) and np.max(np.abs(al.ap_J0_m[q])) > 0
        for k in range(3):
            assert np.max(np.abs(al.ap_r_mp[3 + k])) > 0 and np.max(np.abs(al.ap_J0_m[3 + k])) > 0
        # albedo = sum_k c_k basis[k]: the forward blocks are the same combination of the slots' blocks
        comb_r = sum(c * al.ap_r_mp[3 + k] for k, c in enumerate(A.COEFF))
        comb_j = sum(c * al.ap_J0_m[3 + k] for k, c in enumerate(A.COEFF))
        assert _rel(comb_r, a.r_mp) <= 1e-15 and _rel(comb_j, a.j0_m) <= 1e-15
        # a beam of another strength scales j0- and the vectors, not the matrices
        a2, al2 = O.make_added_layer(FT, N, S), OL.make_added_layer_lin(FT, 6, N, S)
        A.create_surface_layer_spectral_lin(om.albedo, basis, a2, al2, 3, m, p, qp, tau_sum, tsd, 0.5 * F0, FT)
        assert np.array_equal(a2.r_mp, a.r_mp) and np.array_equal(a2.j0_m, 0.5 * a.j0_m) and np.array_equal(al2.ap_J0_m, 0.5 * al.ap_J0_m)


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_toa_jacobian_against_central_differences(pol):
    """R, T of the oracle run are O.rt_run's with the array albedo (the same builders' blocks and the same algebra in another order
    of operations: 1e-13); every coefficient slot, in R and in T, against central differences of O.rt_run at A.FD_STEP, relative to
    the slot's maximum -- the floor A.FD_FLOOR that the device tests reuse times ten; the gas slot likewise (1e-6).

    Measured (max over the three slots): Stokes_I  R 1.497e-10, T 1.493e-10;  Stokes_IQU  R 1.499e-10, T 1.496e-10."""
    om, ol, basis = A.oracle_scene(pol)
    K, pl = len(basis), ol.n_layer_params
    R, T, Rd, Td = A.rt_run_lin(om, ol, basis)
    assert Rd.shape == R.shape + (pl + K,)
    Rf, Tf = O.rt_run(om)
    print("%s: forward R %.2e T %.2e" % (pol, _rel(R, Rf), _rel(T, Tf)))
    assert _rel(R, Rf) <= 1e-13 and _rel(T, Tf) <= 1e-13
    h = A.FD_STEP
    worst = {"R": 0.0, "T": 0.0}
    for k in range(K):
        up = O.rt_run(A.oracle_scene(pol, A.perturbed(A.COEFF, k, h))[0])
        dn = O.rt_run(A.oracle_scene(pol, A.perturbed(A.COEFF, k, -h))[0])
        for what, an, a, b in (("R", Rd[..., pl + k], up[0], dn[0]), ("T", Td[..., pl + k], up[1], dn[1])):
            assert np.max(np.abs(an)) > 0
            e = float(np.max(np.abs((a - b) / (2 * h) - an)) / np.max(np.abs(an)))
            worst[what] = max(worst[what], e)
    print("%s: finite-difference floor R %.3e T %.3e at h = %g" % (pol, worst["R"], worst["T"], h))
    assert max(worst.values()) <= A.FD_FLOOR, worst
    import dataclasses
    g, e = ol.tau_abs_dot[0], 1e-4
    up = O.rt_run(dataclasses.replace(om, tau_abs=om.tau_abs + e * g))
    dn = O.rt_run(dataclasses.replace(om, tau_abs=om.tau_abs - e * g))
    for an, a, b in ((Rd[..., 0], up[0], dn[0]), (Td[..., 0], up[1], dn[1])):
        assert np.max(np.abs((a - b) / (2 * e) - an)) <= 1e-6 * np.max(np.abs(an))


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_slots_are_the_basis_times_the_scalar_albedo_slot(pol):
    """In R, slot k at point s is basis[k, s] times the albedo slot of OL.rt_run_lin run with that point's scalar albedo (the points
    are independent and the scalar builder's m = 0 blocks are this builder's at a constant albedo), within 10 x FD_FLOOR of the slot's
    maximum.  T is left out: for m > 0 the scalar builder keeps t++ = I where this one follows the spectral forward builder's zero."""
    om, ol, basis = A.oracle_scene(pol)
    K, pl = len(basis), ol.n_layer_params
    _, _, Rd, _ = A.rt_run_lin(om, ol, basis)
    import dataclasses
    ref = np.zeros(Rd.shape[:3])
    for s in range(A.S_POINTS):
        one = dataclasses.replace(om, albedo=float(om.albedo[s]))
        ref[:, :, s] = OL.rt_run_lin(one, ol)[2][:, :, s, pl]
    for k in range(K):
        want = ref * basis[k][None, None, :]
        e = _rel(Rd[..., pl + k], want)
        print("%s slot %d: %.2e" % (pol, k, e))
        assert e <= 10 * A.FD_FLOOR, (k, e)


def test_single_scattering_and_multisensor_runs_have_the_slots():
    """The restated walks: shapes, every slot alive, T of the single-scattering run blind to the surface, level 0 of the multi-sensor
    run = rt_run_lin, and level Nz carries the undamped surface slots."""
    om, ol, basis = A.oracle_scene("I")
    R, T, Rd, Td = A.rt_run_ss_lin(om, ol, basis)
    assert Rd.shape == R.shape + (4,) and np.all(Td[..., 1:] == 0) and all(np.max(np.abs(Rd[..., p])) > 0 for p in range(4))
    uw, dw, uwd, dwd = A.ms_lin_segmented(om, ol, [0, 1, 3], basis)
    full = A.rt_run_lin(om, ol, basis)
    for a, b in zip((uw[0], dw[0], uwd[0], dwd[0]), full):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
    assert uwd[2].shape == uw[2].shape + (4,) and all(np.max(np.abs(uwd[2][..., 1 + k])) > 0 for k in range(3))


def test_host_basis_and_refusals():
    """host_model: the Legendre basis is the oracle's and reproduces surface_albedo_spectrum; LambertianSurfaceSpline takes albedo_dot
    [K, nSpec] (None: one table of ones) and refuses another shape; surface_param_names names the slots."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    S = 7
    leg = H.LambertianSurfaceLegendre(A.COEFF)
    basis = H.surface_albedo_basis(leg, S, np.float64)
    assert basis.shape == (3, S) and np.array_equal(basis, A.legendre_basis(3, S))
    assert _rel(np.asarray(A.COEFF) @ basis, H.surface_albedo_spectrum(leg, S)) <= 4e-16
    assert np.array_equal(H.surface_albedo_spectrum(leg, S), O.legendre_albedo(A.COEFF, S))
    assert H.surface_albedo_slots(leg) == 3 and H.surface_albedo_slots(H.LambertianSurfaceScalar(0.1)) is None
    alb = H.surface_albedo_spectrum(leg, S)
    sp = H.LambertianSurfaceSpline(alb)
    assert sp.albedo_dot is None and H.surface_albedo_slots(sp) == 1 and np.array_equal(H.surface_albedo_basis(sp, S), np.ones((1, S)))
    sp2 = H.LambertianSurfaceSpline(alb, basis[:2])
    assert H.surface_albedo_slots(sp2) == 2 and np.array_equal(H.surface_albedo_basis(sp2, S), basis[:2])
    with pytest.raises(ValueError, match="albedo_dot"):
        H.LambertianSurfaceSpline(alb, basis[:, :5])
    with pytest.raises(ValueError, match="albedo_dot"):
        H.LambertianSurfaceSpline(alb, basis[0])
    with pytest.raises(ValueError, match="albedo_dot"):
        H.surface_albedo_basis(sp2, S + 1)
    with pytest.raises(ValueError):
        H.surface_albedo_basis(H.LambertianSurfaceLegendre([0.2]), S)
    CL = vsm.CoreRTLin
    assert CL.surface_param_names(leg) == ["c0", "c1", "c2"] and CL.surface_param_names(sp2) == ["albedo_dot[0]", "albedo_dot[1]"]
    assert CL.surface_param_names(H.rpvSurfaceScalar(0.1, 0.1, 0.7, -0.1)) == ["rho0", "rho_c", "k", "Theta"]


def test_header_declares_the_new_entry_points():
    """include/vsmartmom_hip.h declares both entry points, and the ctypes table binds them with as many arguments."""
    import vsmartmom_jl_amd as vsm
    header = open(os.path.join(ROOT, "include", "vsmartmom_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = set(vsm._lib.exported_symbols())
    base, nargs = "vsm_lambertian_surface_spectral_lin", 15
    for sfx in ("f64", "f32"):
        mt = re.search(r"\bint\s+%s_%s\s*\(([^;]*?)\)\s*;" % (base, sfx), header, flags=re.S)
        assert mt, (base, sfx)
        assert len(mt.group(1).split(",")) == nargs
        assert "%s_%s" % (base, sfx) in bound
    assert len(vsm._lib._SIGS[base + "_{T}"][1]) == nargs
