"""GPU tests of vsm.StandaloneSS (standalone_ss.py) and its kernels (vsm_exact_ss_*, vsm_coxmunk_first_column_*;
csrc/vsm_exact_ss.hip, csrc/vsm_surface.hip) against tests/exact_ss_oracle.py, which materialises P_eff and Pbar as the reference
does.

Tolerances: those tests/test_gpu_ss.py uses for kernels on oracle inputs, relative to the array maximum: FP64 1e-10, FP32 5e-4.
Shapes: S in {1, 70, 130} (a lone point, a partial workgroup, two workgroups of 128 with a ragged tail), L in {1, 2, 5} with one
layer of tau = 0 and one of varpi_eff = 0, nV in {1, 3} with one viewing cosine equal to mu0, C = 1..4 contributors (Rayleigh,
Henyey-Greenstein, Greek, absorption; the last scatterer has tau = 0 everywhere), 16 inner nodes -- one of them moved onto mu0, so
that 1 / mu_first - 1 / mu_node = 0 takes the trapezoid branch of the tau integral in path 3 (every geometry) and in path 4 (the
geometry with mu_v = mu0) -- and 64 azimuth nodes."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import exact_ss_oracle as X  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from test_oracle_exact_ss import synthetic_greek  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 5e-4}
VSM_ERR_INVALID_ARG = 1
MU0 = 0.8
MU_V, DPHI = [0.4, MU0, 0.7], [0.0, 0.9, 2.1]


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


def nodes_with_mu0():
    x, w = X.gauss_legendre_01(16)
    x = x.copy()
    x[int(np.argmin(np.abs(x - MU0)))] = MU0
    return x, w


def build(vsm, arch, FT, S, L, nV, Cn, n_stokes=1, surface="spectral", vector=False):
    """The same scene as an oracle config and as a StandaloneSS config."""
    SSm = vsm.StandaloneSS
    rng = np.random.default_rng(100 * S + 10 * L + Cn)
    tau = lambda lo, hi: rng.uniform(lo, hi, (L, S))
    greek = synthetic_greek(0.6, 0.4, 12)
    pg = vsm.host_model.GreekCoefs(**vars(greek))
    taus = [tau(0.02, 0.06), tau(0.0, 0.2), tau(0.01, 0.05), np.zeros((L, S))]     # the last scatterer: tau = 0 everywhere
    if L >= 2:
        for t in taus:
            t[1] = 0.0                        # a layer with tau = 0
    if L >= 5:
        for i in (0, 2, 3):
            taus[i][3] = 0.0                  # a layer with varpi_eff = 0: absorption only
    kinds = ["rayleigh", "absorption", "greek" if vector else "hg", "greek"][:Cn]
    if Cn == 1:
        kinds = ["rayleigh"]
    oc, pc = [], []
    for kind, t in zip(kinds, taus):
        if kind == "rayleigh":
            oc.append(X.RayleighSSContributor(t, 0.03)), pc.append(SSm.RayleighSSContributor(t, 0.03))
        elif kind == "absorption":
            oc.append(X.AbsorptionSSContributor(t)), pc.append(SSm.AbsorptionSSContributor(t))
        elif kind == "hg":
            oc.append(X.HGAerosolSSContributor(0.7, 0.9, t)), pc.append(SSm.HGAerosolSSContributor(0.7, 0.9, t))
        else:
            oc.append(X.GreekCoefsSSContributor(greek, 0.95, t)), pc.append(SSm.GreekCoefsSSContributor(pg, 0.95, t))
    mu_v, dphi = ([0.55], [0.4]) if nV == 1 else (MU_V, DPHI)
    I0 = np.linspace(1.0, 0.7, S)
    if surface == "spectral":
        alb = np.linspace(0.1, 0.4, S)
        if S > 1:
            alb[0] = 0.0                      # a point of zero albedo
        osf, psf = X.LambertianSSSurface(alb), SSm.LambertianSSSurface(alb)
    elif surface == "coxmunk":
        kw = dict(wind_speed=5.0, n_water=complex(1.34, 1e-8), shadowing=True)
        osf, psf = X.CoxMunkSSSurface(**kw), SSm.CoxMunkSSSurface(**kw)
    else:
        osf, psf = X.LambertianSSSurface(float(surface)), SSm.LambertianSSSurface(float(surface))
    ocfg = X.ExactSSConfig(X.SSGeometry(MU0, mu_v, dphi), osf, oc, I0, n_stokes=n_stokes, mu_nodes=nodes_with_mu0())
    pcfg = SSm.ExactSSConfig(SSm.SSGeometry(MU0, mu_v, dphi), psf, pc, I0, n_stokes=n_stokes, architecture=arch, float_type=FT)
    return ocfg, pcfg


def _check(name, got, want, FT, nonzero=True):
    e = _rel(got, want)
    print("%s: rel. to max %.2e" % (name, e))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert e <= TOL[FT], (name, e)
    if nonzero:
        assert np.max(np.abs(want)) > 0, name


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("S,L,nV,Cn", [(1, 1, 1, 1), (70, 2, 3, 2), (130, 5, 3, 4), (70, 5, 1, 3)])
def test_scalar_all_four_paths_match_the_oracle(vsm, arch, FT, S, L, nV, Cn):
    ocfg, pcfg = build(vsm, arch, FT, S, L, nV, Cn)
    want = X.run_exact_ss(ocfg, "all")
    got = vsm.StandaloneSS.run_exact_ss(pcfg, "all", inner_nodes=nodes_with_mu0())
    for k in ("path1", "path2", "path3", "path4", "total"):
        _check(k, getattr(got, k), getattr(want, k), FT)
    if S > 1:       # albedo[0] = 0
        assert np.all(got.path3[:, :, 0] == 0) and np.all(got.path4[:, :, 0] == 0) and np.all(got.path2[:, :, 0] == 0)
    assert got.metadata == dict(n_layers=L, n_spec=S, n_geom=nV, n_stokes=1) and got.quadrature_info["inner_quadrature"] == 16
    # path 3 alone and path 4 alone: the same kernel with one output null
    for k in ("path3", "path4"):
        one = vsm.StandaloneSS.run_exact_ss(pcfg, k, inner_nodes=nodes_with_mu0())
        assert np.array_equal(getattr(one, k), getattr(got, k)) and np.array_equal(one.total, getattr(got, k))
        assert np.all(one.path1 == 0) and np.all(getattr(one, "path4" if k == "path3" else "path3") == 0)


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_vector_paths_1_and_2_match_the_oracle(vsm, arch, FT, n):
    ocfg, pcfg = build(vsm, arch, FT, 70, 5, 3, 4, n_stokes=n, surface="0.3", vector=True)
    want = X.run_exact_ss(ocfg, "paths_1_2")
    got = vsm.StandaloneSS.run_exact_ss(pcfg, "paths_1_2")
    for k in ("path1", "path2", "total"):
        _check(k, getattr(got, k), getattr(want, k), FT)
    assert np.all(got.path2[:, 1:] == 0) and np.all(got.path3 == 0)
    if n == 4:
        assert np.all(got.path1[:, 3] == 0)
    pol = vsm.StandaloneSS.run_exact_ss(vsm.StandaloneSS.replace(pcfg, n_stokes=1, polarization_type=vsm.host_model.polarization_type(
        {2: "IQ", 3: "IQU", 4: "IQUV"}[n])), "path1")
    assert np.array_equal(pol.path1, got.path1)


@pytest.mark.parametrize("FT", [np.float64, np.float32])
def test_coxmunk_path2_exact_and_truncated(vsm, arch, FT):
    ocfg, pcfg = build(vsm, arch, FT, 70, 2, 3, 2, n_stokes=3, surface="coxmunk", vector=True)
    _check("path2", vsm.StandaloneSS.run_exact_ss(pcfg, "path2").path2, X.run_exact_ss(ocfg, "path2").path2, FT)
    _check("truncated path2 (3 moments)", vsm.StandaloneSS.truncated_ss_path2(pcfg, 3), X.truncated_ss_path2(ocfg, 3), FT)
    with pytest.raises(ValueError):
        vsm.StandaloneSS.truncated_ss_path2(pcfg, 0)


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("n,S,L", [(1, 130, 5), (3, 70, 5), (4, 1, 1)])
def test_jacobians_of_paths_1_and_2_match_the_oracle(vsm, arch, FT, n, S, L):
    ocfg, pcfg = build(vsm, arch, FT, S, L, 3, 4 if L > 1 else 1, n_stokes=n, surface="spectral", vector=n > 1)
    want = X.run_exact_ss_with_jacobians(ocfg, "paths_1_2").jacobians
    got = vsm.StandaloneSS.run_exact_ss_with_jacobians(pcfg, "paths_1_2")["jacobians"]
    for path, keys in (("path1", ("tau_layer", "varpi_eff", "P_eff")), ("path2", ("tau_layer", "surface_brdf")),
                       ("total", ("tau_layer", "varpi_eff", "P_eff", "surface_brdf"))):
        for k in keys:
            _check("%s d/d%s" % (path, k), got[path][k], want[path][k], FT)
    only1 = vsm.StandaloneSS.run_exact_ss_with_jacobians(pcfg, "path1")["jacobians"]
    assert np.array_equal(only1["path1"]["tau_layer"], got["path1"]["tau_layer"]) and np.all(only1["path2"]["tau_layer"] == 0)
    with pytest.raises(ValueError):
        vsm.StandaloneSS.run_exact_ss_with_jacobians(pcfg, "all")


def _model(vsm, arch, FT, surface=None, S=70, L=5):
    H = vsm.host_model
    rng = np.random.default_rng(4)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    tau_abs = rng.uniform(0.0, 0.1, (S, L))
    tau_aer = np.zeros((1, L))
    tau_aer[0, 1:3] = 0.08
    g = O.hg_greek(0.7, 10)
    aer = [H.AerosolOptics(H.GreekCoefs(**vars(g)), 0.95, 0.0)]
    pm = H.model_from_arrays(arch, "IQU", 7, 35.0, [20.0, 50.0], [30.0, 120.0], tau_rayl=tau_rayl, tau_abs=tau_abs, tau_aer=tau_aer,
                             aerosol_optics=aer, depol=0.03, albedo=0.25, m_max=2, float_type=FT, surface=surface)
    geo = (math.cos(math.radians(35.0)), [math.cos(math.radians(v)) for v in (20.0, 50.0)], [math.radians(a) for a in (30.0, 120.0)])
    oc = [X.GreekCoefsSSContributor(X.get_greek_rayleigh(0.03), 1.0, tau_rayl.T), X.AbsorptionSSContributor(tau_abs.T),
          X.GreekCoefsSSContributor(g, 0.95, np.repeat(tau_aer[0][:, None], S, axis=1))]
    return pm, geo, oc


def test_run_exact_ss_of_a_model_equals_the_explicit_config(vsm, arch):
    FT, SSm = np.float64, vsm.StandaloneSS
    pm, geo, oc = _model(vsm, arch, FT)
    total, p1, p2, p3, p4, *_ = SSm.run_exact_ss(pm)                       # the README line
    cfg = SSm.exact_ss_config_from_model(pm)
    assert [type(c).__name__ for c in cfg.contributors] == ["GreekCoefsSSContributor", "AbsorptionSSContributor",
                                                            "GreekCoefsSSContributor"]
    explicit = SSm.run_exact_ss(cfg)
    assert np.array_equal(total, explicit.total) and np.array_equal(p1, explicit.path1) and np.array_equal(p2, explicit.path2)
    want = X.run_exact_ss(X.ExactSSConfig(X.SSGeometry(*geo), X.LambertianSSSurface(0.25), oc, 1.0, n_stokes=3), "paths_1_2")
    _check("total", total, want.total, FT)
    assert total.shape == (2, 3, 70) and np.all(p3 == 0) and np.all(p4 == 0)
    twice = SSm.run_exact_ss(pm, I0=2.0)
    assert _rel(twice.total, 2 * total) <= 1e-15
    # refusals of the adapter
    bad = vsm.host_model.model_from_arrays(arch, "I", 7, 35.0, [20.0], [0.0], tau_rayl=np.full((2, 2), 0.02), albedo=0.1,
                                           surface=vsm.host_model.rpvSurfaceScalar(0.1, 0.1, 0.8, -0.1))
    with pytest.raises(ValueError):
        SSm.exact_ss_config_from_model(bad)
    pm.aerosol_optics[0].f_trunc = 0.1
    with pytest.raises(ValueError):
        SSm.exact_ss_config_from_model(pm)
    with pytest.raises(ValueError):
        SSm.exact_ss_config_from_model(vsm.host_model.model_from_arrays(arch, "I", 7, 35.0, [20.0], [0.0], tau_rayl=np.zeros((2, 2))))


@pytest.mark.parametrize("FT", [np.float64, np.float32])
def test_back_correction_on_a_device_tensor_equals_the_oracle(vsm, arch, FT):
    SSm = vsm.StandaloneSS
    ocfg, pcfg = build(vsm, arch, FT, 70, 5, 3, 4, n_stokes=3, surface="coxmunk", vector=True)
    want = X.ss_back_correction(ocfg, 4, 2)
    assert np.max(np.abs(want)) > 1e-6
    R = torch.full((70, 3, 3), 0.5, dtype=torch.float64 if FT == np.float64 else torch.float32, device="cuda")
    out = SSm.apply_back_correction(R, pcfg, l_trunc=4, max_m=2)
    assert out is R
    _check("correction (device tensor)", R.cpu().numpy().transpose(2, 1, 0) - 0.5, want, FT)
    host = SSm.apply_back_correction(np.full((3, 3, 70), 0.5), pcfg, l_trunc=4, max_m=2)
    _check("correction (host array)", host - 0.5, want, FT)
    _check("truncated path1", SSm.truncated_ss_path1(pcfg, 4), X.truncated_ss_path1(ocfg, 4), FT)
    with pytest.raises(ValueError):
        SSm.apply_back_correction(np.zeros((3, 3, 71)), pcfg, l_trunc=4, max_m=2)
    with pytest.raises(ValueError):
        SSm.truncated_ss_path1(pcfg, 1)
    pm, geo, oc = _model(vsm, arch, FT)
    ocm = X.ExactSSConfig(X.SSGeometry(*geo), X.LambertianSSSurface(0.25), oc, 1.0, n_stokes=3)
    got = SSm.apply_back_correction(np.zeros((2, 3, 70)), pm, l_trunc=4)       # max_m: the model's m_max + 1
    _check("correction (model)", got, X.ss_back_correction(ocm, 4, 3), FT)
    with pytest.raises(ValueError):
        SSm.apply_back_correction(np.zeros((2, 3, 70)), pm)


def test_refusals_raise(vsm, arch):
    SSm, FT = vsm.StandaloneSS, np.float64
    _, scalar = build(vsm, arch, FT, 4, 2, 3, 3)
    _, vector = build(vsm, arch, FT, 4, 2, 3, 3, n_stokes=3, surface="0.3", vector=True)
    _, cox = build(vsm, arch, FT, 4, 2, 3, 2, surface="coxmunk")
    with pytest.raises(ValueError):
        SSm.run_exact_ss(vector, "all")                                    # vector Stokes: paths 1 and 2 only
    with pytest.raises(ValueError):
        SSm.run_exact_ss(SSm.replace(scalar, n_stokes=3), "path1")        # a Henyey-Greenstein contributor in a vector path 1
    SSm.run_exact_ss(SSm.replace(scalar, n_stokes=3), "path2")            # ... which path 2 does not read
    with pytest.raises(ValueError):
        SSm.run_exact_ss(cox, "path3")                                     # paths 3 and 4: Lambertian only
    with pytest.raises(ValueError):
        SSm.run_exact_ss(scalar, "path5")
    g = scalar.geometry
    for geo in (SSm.SSGeometry(0.0, g.mu_v, g.dphi), SSm.SSGeometry(g.mu0, [0.4, -0.1, 0.7], g.dphi), SSm.SSGeometry(g.mu0, g.mu_v, [0.0])):
        with pytest.raises(ValueError):
            SSm.run_exact_ss(SSm.replace(scalar, geometry=geo))
    with pytest.raises(ValueError):
        SSm.run_exact_ss(SSm.replace(scalar, I0=np.ones(5)))
    with pytest.raises(ValueError):
        SSm.run_exact_ss(SSm.replace(scalar, contributors=list(scalar.contributors) + [SSm.AbsorptionSSContributor(np.zeros((3, 4)))]))
    with pytest.raises(ValueError):
        SSm.run_exact_ss(SSm.replace(scalar, contributors=[]))
    with pytest.raises(ValueError):
        SSm.run_exact_ss(SSm.replace(scalar, inner_nquad=0), "all")
    with pytest.raises(NotImplementedError):
        SSm.run_exact_ss(SSm.replace(cox, surface=SSm.CoxMunkSSSurface(5.0, n_water=np.full(4, 1.34 + 0j))), "path2")
    with pytest.raises(vsm.VSMError):
        SSm.run_exact_ss(SSm.replace(scalar, architecture=vsm.Architectures.CPU()))


def test_invalid_arguments_return_before_any_launch(vsm):
    lib = vsm._lib.lib()
    S, L = 4, 2
    t = torch.zeros((L, S), dtype=torch.float64, device="cuda")
    I0 = torch.ones(S, dtype=torch.float64, device="cuda")
    out = torch.zeros((S, 1, 1), dtype=torch.float64, device="cuda")
    tab = (C.c_void_p * L)(*[t[i].data_ptr() for i in range(L)])
    one, mv = (C.c_double * 1)(1.0), (C.c_double * 1)(0.5)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda S_=S, L_=L, C_=1, nV=1, n=1, tab_=tab, mu0=0.8, mv_=mv: lib.vsm_exact_ss_path1_f64(
        S_, L_, C_, nV, n, tab_, one, one, ptr(I0), C.c_double(mu0), mv_, ptr(out), st)
    assert call() == 0
    hole = (C.c_void_p * L)(t[0].data_ptr(), None)
    for bad in (dict(L_=0), dict(C_=0), dict(nV=0), dict(n=5), dict(n=0), dict(S_=-1), dict(tab_=None), dict(tab_=hole), dict(mu0=0.0),
                dict(mv_=(C.c_double * 1)(-0.5))):
        assert call(**bad) == VSM_ERR_INVALID_ARG, bad
    assert b"exact_ss_path1" in lib.vsm_last_error()
    args34 = lambda nQ, o3, o4: lib.vsm_exact_ss_path34_f64(S, L, 1, 1, nQ, tab, one, one, one, mv, one, ptr(I0), ptr(I0),
                                                            C.c_double(0.8), mv, o3, o4, st)
    assert args34(1, ptr(out), None) == 0
    assert args34(0, ptr(out), None) == VSM_ERR_INVALID_ARG and args34(1, None, None) == VSM_ERR_INVALID_ARG
    assert lib.vsm_exact_ss_jac12_f64(S, L, 1, 1, 1, tab, one, one, None, 0, ptr(I0), C.c_double(0.8), mv, ptr(out), None, None, None,
                                      None, st) == VSM_ERR_INVALID_ARG
    assert lib.vsm_exact_ss_path2_f64(S, L, 1, 1, 1, tab, None, 0, ptr(I0), C.c_double(0.8), mv, ptr(out), st) == VSM_ERR_INVALID_ARG
    torch.cuda.synchronize()


def test_footprint_has_no_pbar_array(vsm, arch):
    """Peak device allocation of run_exact_ss(paths = "all") at S = 70, L = 5, nQ = 16, nV = 3 (FP64) stays below the run's inputs
    and outputs plus ONE [nV, L, S, nQ] array -- the reference allocates two (Pbar3, Pbar4), and P_eff [nV, 1, L, S] besides.  Inputs:
    the optical depths [L, S] of the C = 4 contributors, I0 and the albedo [S], the surface BRDF [nV, 1, S]; outputs: four paths
    [nV, 1, S].  Small tensors round up to the allocator's 512-byte granule: one granule for each of the 11 tensors.  (The
    contributor tables live in the library's scratch: C L pointers and a few hundred table entries, not the allocator's.)"""
    FT, S, L, nV, Cn, nQ = np.float64, 70, 5, 3, 4, 16
    _, pcfg = build(vsm, arch, FT, S, L, nV, Cn)
    vsm.StandaloneSS.run_exact_ss(pcfg, "path1")          # library and scratch are up before the measurement
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = vsm.StandaloneSS.run_exact_ss(pcfg, "all")
    peak = torch.cuda.max_memory_allocated() - base
    elems = Cn * L * S + 2 * S + nV * S + 4 * nV * S
    bound = 8 * elems + 11 * 512 + 8 * nV * L * S * nQ
    print("peak %d bytes, inputs + outputs %d, one [nV,L,S,nQ] array %d" % (peak, 8 * elems + 11 * 512, 8 * nV * L * S * nQ))
    assert peak < bound
    assert np.max(np.abs(got.path3)) > 0 and np.max(np.abs(got.path4)) > 0
