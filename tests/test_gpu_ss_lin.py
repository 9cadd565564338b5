"""GPU tests of the linearized single-scattering run (vsm.CoreRTLin.rt_run_ss; core_rt_ss.SceneSSLin) and its column kernel
(vsm_ss_column_lin_*; csrc/vsm_ss.hip) against tests/ss_lin_oracle.py.

Tolerances are test_gpu_ss.py's own: the kernel on the oracle's inputs 1e-10 (FP64) / 5e-4 (FP32), a whole run 1e-8 / 1e-2, per
parameter slot relative to that slot's array maximum.  The device finite differences use the figures test_oracle_ss_lin.py measured
on the CPU with the same one-decade margin: the gas slot 2.84e-8 at h / 2 = 5e-4 (truncation), the albedo slot 1e-12 (R is linear in
the albedo: rounding of the quotient only).  The wind-speed slot of the ocean scene: the CPU oracle on that very scene differs from
its own central differences by 8.0e-7 at h = 5e-3 (3.2e-6 at 1e-2: the order-2 term), gated at ten times that."""
import copy
import json
import os
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ss_lin_oracle as SSL  # noqa: E402
import ss_oracle as SS  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 5e-4}
TOL_RUN = {np.float64: 1e-8, np.float32: 1e-2}
FD_TOL = 10 * 2.84e-8
FD_TOL_ALBEDO = 10 * 1e-12
FD_TOL_WIND = 10 * 8.0e-7
SZA, VZA, VAZ = 35.0, [20.0, 35.0, 50.0], [0.0, 60.0, 120.0]     # the SZA itself among the VZAs; 3 VZAs x 3 Stokes = 9 rows


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


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _scene(vsm, arch, pol, S, naer, ngas, FT=np.float64, albedo=0.3, L=3, scale=1.0, unit_f0=False, surface=None):
    """(oracle model, oracle lin, host model, host lin): Rayleigh + `ngas` gases (x_g scales gas g; `scale` scales gas 0) + `naer`
    synthetic aerosols with their 7 derivative blocks (the directions of test_oracle_lin._aerosol_scene), L = 3, m_max = 2."""
    from test_oracle_lin import _hg_greek
    H = vsm.host_model
    pn = O.polarization(pol).n
    tau_rayl, tau_abs0, F0 = SS.ss_arrays(pn, S, L, seed=11)
    if unit_f0:
        F0[0] = 1.0
    rng = np.random.default_rng(3)
    gases = [tau_abs0 * w for w in ([1.0] if ngas == 1 else [0.6, 0.4])] if ngas else []
    if ngas == 2:
        gases[1] = gases[1] * rng.uniform(0.5, 1.5, (S, L))
        gases[1][:, 0] = 0.0
    tau_abs = scale * gases[0] + sum(gases[1:]) if ngas else tau_abs0
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=albedo, m_max=2)
    oaer, haer, olao, hlao, tad = [], [], [], [], None
    if naer:
        lmax = 7
        g0 = _hg_greek(0.65, lmax)
        gdot = [_hg_greek(0.5 + 0.1 * k, lmax, 0.2 + 0.05 * k) for k in range(4)]
        for k, gd in enumerate(gdot):
            for name in ("alpha", "beta", "gamma", "delta", "epsilon", "zeta"):
                setattr(gd, name, 0.05 * (k + 1) * (getattr(gd, name) - getattr(g0, name)))
        ssa_dot, f_dot = np.array([0.02, -0.3, 0.05, 0.01]), np.array([0.01, 0.02, 0.2, -0.05])
        kw["tau_aer"] = np.array([[0.0, 0.05, 0.15]])
        tad = np.array([[[0.0, 1.0, 3.0], [0.0, 0.02, -0.05], [0.0, -0.03, 0.02], [0.0, 0.1, 0.2], [0.0, 0.01, 0.04],
                         [0.0, 0.5, -0.5], [0.0, -0.2, 0.3]]])
        gk = lambda g: H.GreekCoefs(**vars(g))
        oaer, haer = [O.AerosolOptics(g0, 0.93, 0.12)], [H.AerosolOptics(gk(g0), 0.93, 0.12)]
        olao, hlao = [OL.LinAerosolOptics(gdot, ssa_dot, f_dot)], [H.LinAerosolOptics([gk(g) for g in gdot], ssa_dot, f_dot)]
    om = O.build_model(pol, 7, SZA, list(VZA), list(VAZ), FT=FT, aerosols=oaer, **kw)
    pm = H.model_from_arrays(arch, pol, 7, SZA, list(VZA), list(VAZ), float_type=FT, surface=surface, aerosol_optics=haer, **kw)
    om.varpi_cabannes = pm.varpi_Cabannes = 0.96
    om.F0, pm.F0 = F0, F0
    ol = OL.LinModel(gases, tau_aer_dot=tad, lin_aerosol_optics=olao or None)
    hl = H.LinModel(gases, tau_aer_dot=tad, lin_aerosol_optics=hlao or None)
    return om, ol, pm, hl


def _check_slots(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = 0.0
    for p in range(ref.shape[-1]):
        g, r = got[..., p], ref[..., p]
        if np.max(np.abs(r)) == 0:
            assert np.max(np.abs(g)) == 0, (what, p)
            continue
        e = _rel(g, r)
        worst = max(worst, e)
        assert e <= tol, (what, p, e)
    print("%s: worst slot rel err %.2e" % (what, worst))


RUNS = [
    # (id, FT, pol, S, NAer, NGas)
    ("iqu_s70_p1", np.float64, "IQU", 70, 0, 0),          # surface slot only (pl = 0); one partial workgroup, three row groups
    ("iqu_s70_p10", np.float64, "IQU", 70, 1, 2),         # aerosol slots; P = 10 is no multiple of the chunk width
    ("iquv_s300_p3", np.float64, "IQUV", 300, 0, 2),      # three workgroups, ragged
    ("iquv_s300_p10", np.float64, "IQUV", 300, 1, 2),
    ("scalar_s1_p3", np.float64, "I", 1, 0, 2),
    ("scalar_s1_p10", np.float64, "I", 1, 1, 2),
    ("iqu_s70_p10_fp32", np.float32, "IQU", 70, 1, 2),
    ("iquv_s300_p3_fp32", np.float32, "IQUV", 300, 0, 2),
    ("scalar_s1_p1_fp32", np.float32, "I", 1, 0, 0),
]


@pytest.mark.parametrize("case", RUNS, ids=[c[0] for c in RUNS])
def test_rt_run_ss_lin_against_oracle(vsm, arch, case):
    """The whole run against the oracle, per slot; R, T bit-equal to CoreRT.rt_run_ss."""
    _, FT, pol, S, naer, ngas = case
    om, ol, pm, hl = _scene(vsm, arch, pol, S, naer, ngas, FT)
    Ro, To, Rdo, Tdo = SSL.rt_run_ss_lin(om, ol)
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(pm, hl, naer, ngas, 1)
    P = 7 * naer + ngas + 1
    assert R.shape == (len(VZA), om.pol.n, S) and Rd.shape == R.shape + (P,) and Rd.dtype == FT
    fwd = vsm.CoreRT.rt_run_ss(pm)
    assert np.array_equal(R, fwd[0]) and np.array_equal(T, fwd[1])
    assert _rel(R, Ro) <= TOL_RUN[FT] and _rel(T, To) <= TOL_RUN[FT]
    _check_slots(Rd, Rdo, TOL_RUN[FT], "Rdot")
    _check_slots(Td, Tdo, TOL_RUN[FT], "Tdot")
    assert np.max(np.abs(Rdo[..., P - 1])) > 0


def _kernel_case(vsm, arch, om, ol, pm, FT, p_range=None):
    """vsm_ss_column_lin_* for m = 0 .. m_max into the same buffers, every input taken from the oracle (gas and surface slots)."""
    CR, SSd = vsm.CoreRT, vsm.core_rt_ss
    conv = vsm.Architectures.array_type(arch)
    pol, qp = om.pol, om.quad_points
    S, L = om.tau_rayl.shape
    N, n, nV = qp.Nquad * pol.n, pol.n, len(om.vza)
    pl = ol.n_layer_params
    P = pl + 1
    dt = torch.float64 if FT == np.float64 else torch.float32
    dq = CR.device_quad(pm.quad_points, pm.polarization_type, arch, FT)
    F0 = conv(np.ascontiguousarray(np.asarray(om.F0, dtype=FT).T))
    Rd = torch.zeros((P, S, n, nV), dtype=dt, device="cuda")
    Td = torch.zeros_like(Rd)
    sp = lambda x: conv(np.ascontiguousarray(np.asarray(x, dtype=FT).T))      # [S, p] -> (p, S)
    for m in range(om.m_max + 1):
        weight = FT(0.5 / math.pi) if m == 0 else FT(1.0 / math.pi)
        lods = O.construct_core_optical_properties(om, m)
        lins = SSL.layer_optics_lin(om, ol, lods, m)
        _, tau_sum_all = O.extract_effective_props(lods, FT)
        los = [O.expand_optical_properties(lo, FT) for lo in lods]
        tsd = np.zeros((S, max(pl, 1), L + 1))
        for iz in range(L):
            tsd[:, :pl, iz + 1] = tsd[:, :pl, iz] + lins[iz].tau_dot
        pad = lambda x: x if pl else np.zeros((S, 1))
        Zpp = [CR.to_device_matrix(np.asarray(lods[iz].Zpp), arch, FT) for iz in range(L)]
        Zmp = [CR.to_device_matrix(np.asarray(lods[iz].Zmp), arch, FT) for iz in range(L)]
        surf, surf_l = O.make_added_layer(FT, N, S), O.make_added_layer(FT, N, S)
        als = OL.make_added_layer_lin(FT, P, N, S)
        O.create_surface_layer_lambertian(om.albedo, surf, m, pol, qp, tau_sum_all[:, -1], FT)
        OL.create_surface_layer_lambertian_lin(om.albedo, surf_l, als, P - 1, m, pol, qp, tau_sum_all[:, -1], tsd[:, :pl, -1], om.F0, FT)
        row0, w = CR._vza_rows_weights(pm.polarization_type, pm.vza, pm.vaz, pm.quad_points, m, float(weight), dt)
        SSd.ss_column_lin_(dq, m, P, pl, 0, [conv(lo.tau) for lo in los], [conv(lo.varpi) for lo in los],
                           [conv(tau_sum_all[:, iz].astype(FT)) for iz in range(L)], Zpp, Zmp, [0] * L,
                           [sp(pad(lins[iz].tau_dot)) for iz in range(L)], [sp(pad(lins[iz].varpi_dot)) for iz in range(L)],
                           [sp(tsd[:, :, iz]) for iz in range(L)], None, 0, None, None, F0, conv(surf_l.j0_m), conv(surf.j0_p),
                           conv(als.ap_J0_m), conv(als.ap_J0_p), conv(tau_sum_all[:, -1].astype(FT)), sp(tsd[:, :, -1]), row0, w, nV,
                           Rd, Td, p_range=p_range)
    torch.cuda.synchronize()
    host = vsm.Architectures.to_host
    return host(Rd).transpose(3, 2, 1, 0).copy(), host(Td).transpose(3, 2, 1, 0).copy()


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol,S,ngas", [("IQU", 70, 2), ("IQUV", 300, 0), ("I", 1, 2)], ids=["iqu_s70_p3", "iquv_s300_p1", "scalar_s1_p3"])
def test_column_lin_kernel_accumulates_over_moments(vsm, arch, FT, pol, S, ngas):
    om, ol, pm, _ = _scene(vsm, arch, pol, S, 0, ngas, FT)
    _, _, Rdo, Tdo = SSL.rt_run_ss_lin(om, ol)
    Rd, Td = _kernel_case(vsm, arch, om, ol, pm, FT)
    _check_slots(Rd, Rdo, TOL[FT], "Rdot (kernel)")
    _check_slots(Td, Tdo, TOL[FT], "Tdot (kernel)")


def test_slot_subrange_equals_full_call_bit_for_bit(vsm, arch):
    """Slots [3, 9) of P = 10 in a call of their own (two chunks, the second partial, chunk boundaries shifted against the full
    call's) equal the same slots of the full call; the other slots stay untouched."""
    FT = np.float64
    om, ol, pm, hl = _scene(vsm, arch, "IQU", 70, 1, 2, FT)
    scene = vsm.core_rt_ss.SceneSSLin(pm, hl, 1, 2, 1)
    _, _, Rd, Td = [t.clone() for t in scene.run()]
    orig = vsm.core_rt_ss.ss_column_lin_
    try:
        vsm.core_rt_ss.ss_column_lin_ = lambda *a, **k: orig(*a, **dict(k, p_range=(3, 9)))
        _, _, Rs, Ts = [t.clone() for t in scene.run()]
    finally:
        vsm.core_rt_ss.ss_column_lin_ = orig
    torch.cuda.synchronize()
    assert torch.equal(Rs[3:9], Rd[3:9]) and torch.equal(Ts[3:9], Td[3:9])
    assert float(Rs[:3].abs().max()) == 0 and float(Rs[9:].abs().max()) == 0 and float(Rd[3:9].abs().max()) > 0


def test_device_finite_difference_gas_and_albedo(vsm, arch):
    """The vsm_layer_optics_lin -> kernel chain, FP64: a gas slot and the albedo slot against central differences of two
    CoreRT.rt_run_ss calls (F0[0] = 1: the linearized surface builders weigh the beam with F0)."""
    h = 5e-4
    mk = lambda **kw: _scene(vsm, arch, "IQU", 70, 0, 2, unit_f0=True, **kw)
    om, ol, pm, hl = mk()
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 2, 1)
    up, dn = vsm.CoreRT.rt_run_ss(mk(scale=1 + h)[2]), vsm.CoreRT.rt_run_ss(mk(scale=1 - h)[2])
    for name, an, k in (("Rdot gas", Rd[..., 0], 0), ("Tdot gas", Td[..., 0], 1)):
        e = _rel(an, (up[k] - dn[k]) / (2 * h))
        print("%s: device FD difference %.3e" % (name, e))
        assert e <= FD_TOL, (name, e)
    up, dn = vsm.CoreRT.rt_run_ss(mk(albedo=0.3 + h)[2]), vsm.CoreRT.rt_run_ss(mk(albedo=0.3 - h)[2])
    e = _rel(Rd[..., 2], (up[0] - dn[0]) / (2 * h))
    print("Rdot albedo: device FD difference %.3e" % e)
    assert e <= FD_TOL_ALBEDO and np.max(np.abs(Rd[..., 2])) > 0
    assert np.all(Td[..., 2] == 0) and np.array_equal(up[1], dn[1])      # T does not see the albedo, on either side


LAND_YAML = """
# the shape of the reference's config/lambertian_land.yaml: IQUV, 11 streams, 9 viewing angles, two points, a 6-layer profile
radiative_transfer:
  spec_bands: ["[19417.0 19418.0]"]
  surface: [LambertianSurfaceScalar(0.15)]
  nstreams: 11
  truncation: auto
  polarization_type: Stokes_IQUV()
  depol: -1
  float_type: Float64
  architecture: default_architecture
geometry: {sza: 30, vza: [60, 45, 30, 15, 0, 15, 30, 45, 60], vaz: [180, 180, 180, 180, 0, 0, 0, 0, 0], obs_alt: 1000.0}
atmospheric_profile: {T: [220.0, 230.0, 250.0, 265.0, 280.0, 287.0], p: [1.0, 50.0, 200.0, 400.0, 650.0, 850.0, 1000.0], profile_reduction: -1}
"""


def test_device_finite_difference_yaml_model(vsm, arch):
    """The model-construction path: parameters_from_yaml -> model_from_parameters -> SceneSSLin (vsm_layer_optics_lin -> kernel),
    FP64, IQUV, N = 60, the SZA among the VZAs.  The gas slot (a synthetic absorber, as test_c3_ocean_coxmunk_linearized gives the
    scene's `q` slot one) and the albedo slot against central differences of two CoreRT.rt_run_ss calls each."""
    io, H = vsm.io_yaml, vsm.host_model
    model = io.model_from_parameters(io.parameters_from_yaml(LAND_YAML), arch)
    assert isinstance(model.surface, H.LambertianSurfaceScalar) and model.F0 is None
    S, L = model.tau_rayl.shape
    prof = np.linspace(0.2, 1.8, L)[None, :] * np.array([[0.02], [0.005]])
    g = prof * np.random.default_rng(7).uniform(0.8, 1.2, (S, L))
    model.tau_abs = prof * 1.0
    lin = H.LinModel([g])
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(model, lin, 0, 1, 1)
    assert Rd.shape == (9, 4, S, 2)

    def fwd(dabs=0.0, dalb=0.0):
        mm = copy.copy(model)
        mm.tau_abs = model.tau_abs + dabs * g
        mm.surface = H.LambertianSurfaceScalar(0.15 + dalb)
        return vsm.CoreRT.rt_run_ss(mm)
    h = 5e-4
    up, dn = fwd(dabs=h), fwd(dabs=-h)
    for name, an, k in (("Rdot gas", Rd[..., 0], 0), ("Tdot gas", Td[..., 0], 1)):
        e = _rel(an, (up[k] - dn[k]) / (2 * h))
        print("%s (YAML model): device FD difference %.3e" % (name, e))
        assert np.max(np.abs(an)) > 0 and e <= FD_TOL, (name, e)
    up, dn = fwd(dalb=h), fwd(dalb=-h)
    e = _rel(Rd[..., 1], (up[0] - dn[0]) / (2 * h))
    print("Rdot albedo (YAML model): device FD difference %.3e" % e)
    assert np.max(np.abs(Rd[..., 1])) > 0 and e <= FD_TOL_ALBEDO
    assert np.all(Td[..., 1] == 0)


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_coxmunk_against_oracle(vsm, arch, FT):
    """A Cox-Munk surface: vsm_brdf_surface_lin's sources of all slots go into the column (gas slots and the wind-speed slot),
    against the oracle with its own reflectance and wind-speed derivative; m = 0..3."""
    H = vsm.host_model
    om, ol, pm, hl = _scene(vsm, arch, "IQU", 70, 0, 2, FT, surface=H.CoxMunkSurface(wind_speed=5.0))
    om.m_max = pm.m_max = 3
    Ro, To, Rdo, Tdo = SSL.rt_run_ss_lin(om, ol, surface=CM.CoxMunkSurface(5.0))
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 2, 1)
    fwd = vsm.CoreRT.rt_run_ss(pm)
    assert np.array_equal(R, fwd[0]) and np.array_equal(T, fwd[1])
    assert _rel(R, Ro) <= TOL_RUN[FT] and _rel(T, To) <= TOL_RUN[FT]
    _check_slots(Rd, Rdo, TOL_RUN[FT], "Rdot (Cox-Munk)")
    _check_slots(Td, Tdo, TOL_RUN[FT], "Tdot (Cox-Munk)")
    assert np.max(np.abs(Rdo[..., 2])) > 0 and np.all(Td[..., 2] == 0)


def test_coxmunk_wind_speed_slot_device_finite_difference(vsm, arch):
    """The ocean fixture's scene (config/ocean_coxmunk.yaml: IQUV, N = 60, 33 layers, m = 0..21, F0 = e1) at its two points: the
    wind-speed slot of Rdot against central differences of two CoreRT.rt_run_ss calls; T does not see the surface."""
    import yaml
    io, H = vsm.io_yaml, vsm.host_model
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocean_coxmunk_scene.json")) as f:
        d = json.load(f)
    d.pop("source")
    model = io.model_from_parameters(io.parameters_from_yaml(yaml.safe_dump(d)), arch)
    assert isinstance(model.surface, H.CoxMunkSurface) and model.surface.wind_speed == 5.0 and model.F0 is None
    S, L = model.tau_rayl.shape
    prof = np.linspace(0.2, 1.8, L)[None, :] * np.array([[0.004], [0.0015]])
    model.tau_abs = prof * 1.0
    lin = H.LinModel([prof * np.random.default_rng(7).uniform(0.8, 1.2, (S, L))])
    R, T, Rd, Td = vsm.CoreRTLin.rt_run_ss(model, lin, 0, 1, 1)
    assert Rd.shape == (9, 4, S, 2)

    def fwd(U):
        mm = copy.copy(model)
        mm.surface = H.CoxMunkSurface(wind_speed=U)
        return vsm.CoreRT.rt_run_ss(mm)
    h = 5e-3
    up, dn = fwd(5.0 + h), fwd(5.0 - h)
    e = _rel(Rd[..., 1], (up[0] - dn[0]) / (2 * h))
    print("Rdot wind speed: device FD difference %.3e" % e)
    assert np.max(np.abs(Rd[..., 1])) > 0 and e <= FD_TOL_WIND, e
    assert np.all(Td[..., 1] == 0) and np.array_equal(up[1], dn[1])
    assert np.max(np.abs(Rd[..., 0])) > 0 and np.max(np.abs(Td[..., 0])) > 0


def test_black_surface_keeps_the_albedo_slot(vsm, arch):
    """Albedo 0: the albedo slot of Rdot is non-zero, and the oracle match holds on both albedos (the gas slots of the two runs
    differ by the surface term's share, which the oracle carries)."""
    FT = np.float64
    for alb in (0.0, 0.3):
        om, ol, pm, hl = _scene(vsm, arch, "IQU", 70, 0, 2, FT, albedo=alb)
        _, _, Rdo, Tdo = SSL.rt_run_ss_lin(om, ol)
        _, _, Rd, Td = vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 2, 1)
        _check_slots(Rd, Rdo, TOL_RUN[FT], "Rdot albedo %.1f" % alb)
        _check_slots(Td, Tdo, TOL_RUN[FT], "Tdot albedo %.1f" % alb)
        assert np.max(np.abs(Rd[..., 2])) > 0


def test_refusals(vsm, arch):
    H = vsm.host_model
    om, ol, pm, hl = _scene(vsm, arch, "I", 4, 0, 2)
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 2, 0)
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=np.full((3, 4), 0.1)))
    with pytest.raises(NotImplementedError):
        vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 2, 1)
    pm.sources = None
    pm.surface = H.rpvSurfaceScalar(0.1, 0.8, -0.1, 0.5)
    with pytest.raises(vsm.VSMError):
        vsm.CoreRTLin.rt_run_ss(pm, hl, 0, 2, 1)
    # four aerosols: 21 component blocks of Z_dot
    g = H.GreekCoefs(**vars(O.hg_greek(0.6, 7)))
    kw = dict(tau_rayl=om.tau_rayl, tau_abs=om.tau_abs, tau_aer=np.full((4, 3), 0.05), aerosol_optics=[H.AerosolOptics(g, 0.9, 0.0)] * 4)
    pm4 = H.model_from_arrays(arch, "I", 7, SZA, list(VZA), list(VAZ), **kw)
    lao = H.LinAerosolOptics([g] * 4, np.zeros(4), np.zeros(4))
    hl4 = H.LinModel(hl.tau_abs_dot, tau_aer_dot=np.zeros((4, 7, 3)), lin_aerosol_optics=[lao] * 4)
    with pytest.raises(NotImplementedError):
        vsm.CoreRTLin.rt_run_ss(pm4, hl4, 4, 2, 1)


def test_invalid_arguments_before_any_launch(vsm, arch):
    """P < 1, L < 1, null tables, a row outside N and a slot range outside P return VSM_ERR_INVALID_ARG; nothing launches."""
    lib = vsm._lib.lib()
    om, ol, pm, hl = _scene(vsm, arch, "I", 4, 0, 2)
    dq = vsm.CoreRT.device_quad(pm.quad_points, pm.polarization_type, arch, np.float64)
    q = dq.cstruct()
    N = dq.N if hasattr(dq, "N") else q.N
    t = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    tab = (C.c_void_p * 1)(t.data_ptr())
    zs = (C.c_longlong * 1)(0)
    w = (C.c_double * 1)(1.0)

    def call(P=3, L=1, p_lo=0, p_hi=3, tau_tab=tab, dot_tab=tab, row=0):
        return lib.vsm_ss_column_lin_f64(C.byref(q), 4, L, 0, P, min(2, max(P - 1, 0)), 0, p_lo, p_hi, tau_tab, tab, tab, tab, tab, zs,
                                         dot_tab, tab, tab, None, 0, None, None, p, p, None, p, p, p, p, 1, (C.c_int * 1)(row), w,
                                         p, p, None)
    assert call(P=0, p_hi=0) == 1 and call(L=0) == 1 and call(tau_tab=None) == 1 and call(dot_tab=None) == 1
    assert call(row=N) == 1 and call(row=-1) == 1
    assert call(p_lo=2, p_hi=4) == 1 and call(p_lo=-1) == 1 and call(p_lo=2, p_hi=2) == 1
    assert lib.vsm_last_error()
    torch.cuda.synchronize()
    vsm._lib.check_device_status("invalid arguments")
    assert float(t.abs().max()) == 0
    assert call() == 0


def test_footprint_below_one_added_layer_lin(vsm, arch):
    """IQU, 7 streams, S = 300, P = 3, Rayleigh + gas: peak device allocation over scene construction plus run() stays below the
    bytes of ONE non-shared AddedLayerLin(FT, arch, P, N, S): 12 (1 + P) N^2 S elements, which rt_run_lin cannot avoid."""
    om, ol, pm, hl = _scene(vsm, arch, "IQU", 300, 0, 2)
    N, S, P = pm.quad_points.Nquad * 3, 300, 3
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    scene = vsm.core_rt_ss.SceneSSLin(pm, hl, 0, 2, 1)
    scene.run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = 8 * 12 * (1 + P) * N * N * S
    print("peak %d bytes, one AddedLayerLin %d" % (peak, bound))
    assert peak < bound
    assert float(scene.Rd.abs().max()) > 0
