"""CPU checks of the Raman multi-sensor oracle (tests/ms_raman_oracle.py): the summed single-solve inelastic level equation against
the reference's per-line two-inverse interlayer_flux_helper!(::RRS), the segmented algorithm of core_rt_ms_raman.py against the
statement-order transcription of rt_run_test_ms(::RRS), level 0 against OR.rt_run_rrs, and the exact zeros of a column without
Raman scattering or above a black surface."""
import numpy as np
import pytest

import ms_raman_oracle as MR
from oracle import vsm_oracle as O
from oracle import vsm_oracle_raman as OR

SHIFTS = np.array([-5, -2, -1, 1, 3, 40, 0])      # 40: never in band for S <= 40
W_IE = np.array([0.004, 0.012, 0.02, 0.018, 0.007, 0.3, 0.009])


def _rel_per_component(a, b):
    """max over VZA / points of |a - b|, per Stokes component, relative to that component's max |b|."""
    out = []
    for k in range(b.shape[1]):
        sc = float(np.max(np.abs(b[:, k])))
        out.append(float(np.max(np.abs(a[:, k] - b[:, k]))) / sc if sc > 0 else float(np.max(np.abs(a[:, k]))))
    return max(out)


def _column(pol, S=6, L=5, albedo=0.12, varpi_ie=W_IE, seed=3, m_max=2):
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(np.linspace(0.02, 0.06, L), (S, 1))
    tau_abs = (10.0 ** rng.uniform(-3, 0.0, (S, 1))) * np.linspace(0.5, 1.5, L)[None, :] / L
    model = O.build_model(pol, 7, 35.0, [20.0, 50.0], [0.0, 60.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075,
                          albedo=albedo, m_max=m_max)
    model.varpi_cabannes = 0.96
    F0 = np.zeros((model.pol.n, S))
    F0[0] = 0.8 + 0.4 * rng.random(S)
    model.F0 = F0
    rs = OR.RRS(i_shift=SHIFTS, varpi_ie=np.asarray(varpi_ie, dtype=np.float64),
                greek_raman=O.get_greek_rayleigh(6.0 / 7.0 * 0.5))
    return model, rs


@pytest.mark.parametrize("N,S,shared_bottom,null_bottom", [(3, 7, False, False), (8, 9, True, False), (12, 6, False, True)])
def test_single_solve_equals_two_inverse_per_line(N, S, shared_bottom, null_bottom):
    """q = sum_k (c_ie + B_ie dw(n0)), r = sum_k (a_ie + A_ie uw(n0)) + A q, dw_ie = (I - A B)^-1 r, uw_ie = q + B dw_ie equals the
    line sum of interlayer_flux_helper!(::RRS)'s two-inverse per-line formula; shifts include lines partly and never in band."""
    rng = np.random.default_rng(N * 100 + S)
    FT = np.float64
    shifts = np.array([-3, -1, 2, 0, S + 4, -(S + 1), 1])
    K = len(shifts)
    A = 0.3 * rng.random((S, N, N)) / N
    B = 0.4 * rng.random((1 if shared_bottom else S, N, N)) / N
    a, c = rng.random((S, N)), rng.random((S, N))
    A_ie, a_ie = 0.05 * rng.random((K, S, N, N)) / N, 0.05 * rng.random((K, S, N))
    B_ie, c_ie = (None, None) if null_bottom else (0.05 * rng.random((K, S, N, N)) / N, 0.05 * rng.random((K, S, N)))
    uw, dw, uwie_k, dwie_k = MR.interlayer_flux_rrs_reference(FT, shifts, A, B, a, c, A_ie, B_ie, a_ie, c_ie)
    uwie, dwie = MR.level_ie_push_through(FT, shifts, A, B, dw, uw, A_ie, a_ie, B_ie, c_ie)
    for got, ref in ((uwie, uwie_k.sum(axis=0)), (dwie, dwie_k.sum(axis=0))):
        assert np.max(np.abs(ref)) > 1e-3
        assert np.max(np.abs(got - ref)) / np.max(np.abs(ref)) <= 1e-12


@pytest.mark.parametrize("pol,levels", [("I", [3, 0, 5, 1, 3]), ("IQU", [3, 0, 5, 1, 3]), ("IQU", [4, 2])])
def test_segmented_equals_reference(pol, levels):
    model, rs = _column(pol)
    ref = MR.ms_raman_reference(model, rs, levels)
    seg = MR.ms_raman_segmented(model, rs, levels)
    for name, r_list, s_list in zip(("uw", "dw", "uwie", "dwie"), ref, seg):
        assert len(r_list) == len(s_list) == len(levels)
        for i, l in enumerate(levels):
            assert np.max(np.abs(r_list[i])) > 0, (name, l)
            e = _rel_per_component(s_list[i], r_list[i])
            assert e <= 1e-12, (pol, name, l, e)


@pytest.mark.parametrize("pol", ["I", "IQU"])
def test_level0_is_rt_run_rrs(pol):
    model, rs = _column(pol)
    ref = OR.rt_run_rrs(model, rs)
    seg = MR.ms_raman_segmented(model, rs, [2, 0, 5])
    for r, s in zip(ref, seg):
        assert np.array_equal(s[1], r)


def test_no_raman_gives_zero_ie_and_black_surface_nz():
    model, rs = _column("IQU", varpi_ie=np.zeros(len(W_IE)))
    levels = [0, 1, 3, 5]
    out = MR.ms_raman_segmented(model, rs, levels)
    for i in range(len(levels)):
        assert not np.any(out[2][i]) and not np.any(out[3][i])
        assert np.max(np.abs(out[0][i])) > 0
    model, rs = _column("IQU", albedo=0.0)
    uw, dw, uwie, dwie = MR.ms_raman_segmented(model, rs, [5, 2])
    assert not np.any(uwie[0])
    assert np.max(np.abs(dwie[0])) > 0 and np.max(np.abs(uwie[1])) > 0


def test_segment_counts():
    """Nz + (Nz - l1) layer steps and L + 1 interactions beyond the layer walks per moment (L interior levels: one bottom each,
    and the surface interaction of level 0)."""
    model, rs = _column("I", m_max=1)
    counts = {}
    MR.ms_raman_segmented(model, rs, [4, 2, 0, 5], counts=counts)
    Nz, l1, L = 5, 2, 2
    assert counts == dict(layers=2 * (Nz + (Nz - l1)), interactions=2 * (L + 1))


def _host_model(vsm, pol="I", l_trunc=9, **kw):
    H = vsm.host_model
    base = dict(tau_rayl=np.tile(np.full(4, 0.05), (2, 1)), tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=1)
    base.update(kw)
    return H.model_from_arrays(vsm.Architectures.GPU(0), pol, l_trunc, 40.0, [30.0], [0.0], **base)


def test_api_argument_validation():
    """Checked on the host, before any device work: levels outside 0..Nz or not integers, sources other than SolarBeam,
    N > 128 (no operator-level twin of the inelastic level kernel) and iBand != 1."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    rs = vsm.CoreRTRaman.RRS(SHIFTS, W_IE, H.GreekCoefs(**vars(O.get_greek_rayleigh(0.5))))
    model = _host_model(vsm)
    for bad in ([-1], [0, 5], [1.5], []):
        with pytest.raises(ValueError):
            vsm.CoreRTRaman.rt_run_multisensor(rs, model, bad)
    B = np.full((4, 2), 1e-3)
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRTRaman.rt_run_multisensor(rs, _host_model(vsm, sources=srcs), [1])
    big = _host_model(vsm, pol="IQU", l_trunc=90)
    assert big.quad_points.Nquad * 3 > 128
    with pytest.raises(vsm.VSMError, match="128"):
        vsm.CoreRTRaman.rt_run_multisensor(rs, big, [1])
    with pytest.raises(vsm.VSMError, match="iBand"):
        vsm.CoreRTRaman.rt_run_multisensor(rs, model, [1], iBand=2)


@pytest.mark.parametrize("pattern", ["01_10_11", "00_01_11"])
def test_segmented_equals_reference_nonscattering_layers(pattern):
    """Numerically non-scattering layers (the _00 / _01 / _10 tags, rt_run(RRS)'s statements): those drop inelastic terms and do
    not associate, so a bottom whose lower part holds one is walked layer by layer, as in the prototype."""
    S, L, tiny = 8, 4, 1e-22
    model, rs = _column("IQU", S=S, L=L)
    model.tau_rayl[...] = np.tile({"01_10_11": [tiny, 0.04, tiny, 0.03], "00_01_11": [tiny, tiny, 0.04, 0.03]}[pattern], (S, 1))
    tags, _ = O.extract_effective_props(O.construct_core_optical_properties(model, 0), np.float64)
    assert list(tags[1:L]) == pattern.split("_")
    levels = [2, 0, 4, 1, 3]
    ref = MR.ms_raman_reference(model, rs, levels)
    seg = MR.ms_raman_segmented(model, rs, levels)
    for name, r_list, s_list in zip(("uw", "dw", "uwie", "dwie"), ref, seg):
        for i, l in enumerate(levels):
            e = _rel_per_component(s_list[i], r_list[i])
            assert e <= 1e-12, (pattern, name, l, e)


# ---- the surface hook (tests/driver_surface_cases.py: the scenes of tests/test_gpu_driver_surfaces.py) ------------------------------
import driver_surface_cases as DS  # noqa: E402


@pytest.fixture(scope="module", params=DS.SHAPES, ids=lambda p: "%s_%d" % p)
def grid_scene(request):
    pol, l_trunc = request.param
    om = DS.oracle_model(pol, l_trunc)
    return om, MR.ms_raman_reference(om, DS.oracle_rs(), DS.LEVELS)


def test_default_hook_is_the_lambertian_builder(grid_scene):
    """surface=None builds what both walks had hard-wired: the same bits as the scalar Lambertian builder handed in as a hook."""
    om, base = grid_scene
    for fn, ref in ((MR.ms_raman_reference, base), (MR.ms_raman_segmented, MR.ms_raman_segmented(om, DS.oracle_rs(), DS.LEVELS))):
        got = fn(om, DS.oracle_rs(), DS.LEVELS, surface=DS.lambertian_hook(om))
        for g_list, r_list in zip(got, ref):
            assert all(np.array_equal(g, r) for g, r in zip(g_list, r_list))


def test_degenerate_surfaces(grid_scene):
    """A constant BRDF and a constant albedo spectrum are the Lambertian surface, at every level: 1e-13 of the largest value (over
    the albedo spectrum all but dw / dwie of level 0, which are rt_run's T / ieT: DS.degenerate_cases)."""
    om, base = grid_scene
    for name, model, hook, spectral in DS.degenerate_cases(om):
        got = MR.ms_raman_reference(model, DS.oracle_rs(), DS.LEVELS, surface=hook)
        for what, g_list, r_list in zip(("uw", "dw", "uwie", "dwie"), got, base):
            for l, g, r in zip(DS.LEVELS, g_list, r_list):
                if spectral and l == 0 and what in ("dw", "dwie"):
                    continue
                assert DS.rel_max(g, r) <= 1e-13, (name, what, l, DS.rel_max(g, r))


def test_black_surface_is_far_from_the_lambertian_one(grid_scene):
    """Against a vacuous pass on the device: uw and uwie of every level differ by at least 0.1 of their largest value."""
    om, base = grid_scene
    blk = MR.ms_raman_reference(DS.black(om), DS.oracle_rs(), DS.LEVELS)
    for k, what in ((0, "uw"), (2, "uwie")):
        for l, b, r in zip(DS.LEVELS, blk[k], base[k]):
            assert DS.rel_max(b, r) >= 0.1, (what, l, DS.rel_max(b, r))
