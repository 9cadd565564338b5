"""CPU checks of the multi-sensor oracle (tests/ms_oracle.py): the segmented algorithm of core_rt_ms.py against the statement-order
transcription of the reference's prototype (rt_run_test_ms, rt_run_multisensor.jl), level 0 against rt_run, the black-surface
bottom level, flux conservation in a conservative column (independent of the transcription), and argument validation."""
import numpy as np
import pytest

import ms_oracle as MS
from oracle import vsm_oracle as O


def _rel_per_component(a, b):
    """max over VZA / points of |a - b|, per Stokes component, relative to that component's max |b|."""
    out = []
    for k in range(b.shape[1]):
        sc = float(np.max(np.abs(b[:, k])))
        out.append(float(np.max(np.abs(a[:, k] - b[:, k]))) / sc if sc > 0 else float(np.max(np.abs(a[:, k]))))
    return max(out)


def _aerosols():
    return [O.AerosolOptics(O.hg_greek(0.7, 10), 0.95, 0.1), O.AerosolOptics(O.hg_greek(0.5, 6), 0.9, 0.0)]


def _column(kind, rng):
    """(model, levels) of the four scenes."""
    if kind == "iqu_rayleigh_abs":
        S, L = 3, 5
        kw = dict(tau_rayl=np.tile(np.linspace(0.01, 0.06, L), (S, 1)), tau_abs=10.0 ** rng.uniform(-4, -0.5, (S, L)), depol=0.03,
                  albedo=0.25, m_max=3)
        return O.build_model("IQU", 9, 40.0, [30.0, 0.0, 55.0], [0.0, 60.0, 120.0], **kw), [3, 0, 1, 5, 3]
    if kind == "two_aerosols":
        S, L = 2, 5
        tau_aer = np.array([[0.0, 0.05, 0.2, 0.1, 0.0], [0.02, 0.0, 0.1, 0.3, 0.05]])
        kw = dict(tau_rayl=np.tile(np.full(L, 0.02), (S, 1)), tau_abs=np.full((S, L), 1e-3), tau_aer=tau_aer, aerosols=_aerosols(),
                  depol=0.03, albedo=0.1, m_max=6)
        return O.build_model("IQU", 11, 35.0, [20.0, 45.0], [30.0, 90.0], **kw), [4, 2, 5]
    if kind == "legendre_surface":
        S, L = 4, 4
        kw = dict(tau_rayl=np.tile(np.full(L, 0.03), (S, 1)), tau_abs=10.0 ** rng.uniform(-3, -1, (S, L)), depol=0.0,
                  albedo=O.legendre_albedo([0.2, 0.05, -0.02], S), m_max=2)
        return O.build_model("IQU", 9, 30.0, [10.0, 50.0], [0.0, 45.0], **kw), [2, 1, 4, 0]
    if kind == "scalar_all_levels":
        S, L = 2, 6
        kw = dict(tau_rayl=np.tile(np.linspace(0.02, 0.12, L), (S, 1)), tau_abs=np.full((S, L), 5e-3), depol=0.0, albedo=0.3,
                  m_max=2)
        return O.build_model("I", 13, 50.0, [0.0, 30.0, 60.0], [0.0, 90.0, 180.0], **kw), list(range(L + 1))
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["iqu_rayleigh_abs", "two_aerosols", "legendre_surface", "scalar_all_levels"])
def test_segmented_equals_reference(kind):
    model, levels = _column(kind, np.random.default_rng(7))
    ur, dr = MS.ms_reference(model, levels)
    us, ds = MS.ms_segmented(model, levels)
    assert len(ur) == len(us) == len(levels)
    for i, l in enumerate(levels):
        eu, ed = _rel_per_component(us[i], ur[i]), _rel_per_component(ds[i], dr[i])
        assert eu <= 1e-12 and ed <= 1e-12, (kind, l, eu, ed)
        assert np.max(np.abs(ur[i])) > 0 and np.max(np.abs(dr[i])) > 0, (kind, l)


@pytest.mark.parametrize("kind", ["iqu_rayleigh_abs", "two_aerosols", "legendre_surface"])
def test_level0_is_rt_run_bit_for_bit(kind):
    model, _ = _column(kind, np.random.default_rng(3))
    R, T = O.rt_run(model)
    ur, dr = MS.ms_reference(model, [0])
    assert np.array_equal(ur[0], R) and np.array_equal(dr[0], T)


def test_interaction_helper_ms_11_is_interaction_11():
    """interaction_helper_ms!(::ScatteringInterface_11) (interaction_multisensor.jl:93-148) computes every update from the
    pre-update operands, like interaction!(::ScatteringInterface_11): the same algebra as O.interaction("11")."""
    rng = np.random.default_rng(5)
    S, N = 3, 8
    rnd = lambda *sh: 0.1 * rng.standard_normal(sh)
    add = O.AddedLayer(rnd(S, N, N), rnd(S, N, N) + np.eye(N), rnd(S, N, N), rnd(S, N, N) + np.eye(N), rnd(S, N), rnd(S, N))
    comp = O.CompositeLayer(rnd(S, N, N), rnd(S, N, N), rnd(S, N, N) + np.eye(N), rnd(S, N, N) + np.eye(N), rnd(S, N), rnd(S, N))
    # the prototype's statements, transcribed
    I = np.eye(N)[None]
    r_pm, r_mp, t_mm, t_pp, j0_p, j0_m = add.r_pm, add.r_mp, add.t_mm, add.t_pp, add.j0_p, add.j0_m
    R_mp, R_pm, T_pp, T_mm, J0_p, J0_m = comp.R_mp, comp.R_pm, comp.T_pp, comp.T_mm, comp.J0_p, comp.J0_m
    tmp_inv = np.linalg.inv(I - r_mp @ R_pm)
    T01_inv = T_mm @ tmp_inv
    tmpJ0_m = J0_m + O._mv(T01_inv, O._mv(r_mp, J0_p) + j0_m)
    tmpR_mp = R_mp + T01_inv @ r_mp @ T_pp
    tmpT_mm = T01_inv @ t_mm
    tmp_inv = np.linalg.inv(I - R_pm @ r_mp)
    T21_inv = t_pp @ tmp_inv
    tmpJ0_p = j0_p + O._mv(T21_inv, J0_p + O._mv(R_pm, j0_m))
    tmpT_pp = T21_inv @ T_pp
    tmpR_pm = r_pm + T21_inv @ R_pm @ t_mm
    O.interaction("11", comp, add, np.float64)
    for got, want in ((comp.J0_m, tmpJ0_m), (comp.R_mp, tmpR_mp), (comp.T_mm, tmpT_mm), (comp.J0_p, tmpJ0_p),
                      (comp.T_pp, tmpT_pp), (comp.R_pm, tmpR_pm)):
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


def test_push_through_equals_two_inverses():
    rng = np.random.default_rng(11)
    S, N = 4, 12
    A, B = 0.2 * rng.random((S, N, N)), 0.2 * rng.random((S, N, N))
    a, c = rng.random((S, N)), rng.random((S, N))
    uw, dw = MS.level_push_through(np.float64, A, a, B, c)
    uw0, dw0 = MS.interlayer_flux_reference(np.float64, A, B, a, c)
    np.testing.assert_allclose(dw, dw0, rtol=1e-13)
    np.testing.assert_allclose(uw, uw0, rtol=1e-13)


def test_black_surface_bottom_level():
    """Level Nz above a black surface: nothing comes up (uw = 0), and the diffuse field going down is rt_run's T_SFI at every
    VZA row other than the SZA row (T_SFI carries the direct beam there)."""
    S, L = 2, 4
    sza, vza = 40.0, [0.0, 25.0, 40.0, 60.0]
    model = O.build_model("IQU", 11, sza, vza, [0.0, 30.0, 0.0, 90.0], tau_rayl=np.tile(np.full(L, 0.05), (S, 1)),
                          tau_abs=np.full((S, L), 2e-3), depol=0.03, albedo=0.0, m_max=2)
    R, T = O.rt_run(model)
    for fn in (MS.ms_reference, MS.ms_segmented):
        uw, dw = fn(model, [L])
        assert np.all(uw[0] == 0)
        off = [i for i, v in enumerate(vza) if v != sza]
        np.testing.assert_allclose(dw[0][off], T[off], rtol=1e-12, atol=1e-15 * np.max(np.abs(T)))
        isza = vza.index(sza)
        assert np.max(np.abs(T[isza] - dw[0][isza])) > 1e-3 * np.max(np.abs(T[isza]))      # the direct beam


# Conservative Rayleigh column (varpi = 1, no absorption): the net flux is the same at every level.  The thin-layer start of
# doubling leaves a spread; measured on the oracle at 1.7e-5 of mu0 F0 (l_trunc 15, six layers of tau 0.05, albedo 0.3).
FLUX_SPREAD_BOUND = 3e-5


def conservative_model(FT=np.float64):
    L = 6
    return O.build_model("I", 15, 40.0, [30.0], [0.0], tau_rayl=np.tile(np.full(L, 0.05), (2, 1)), depol=0.0, albedo=0.3, m_max=0,
                         FT=FT), list(range(1, L + 1))


def flux_spread(model, full, levels):
    f = np.array([MS.net_flux(model, full, l) for l in levels])          # [levels, S]
    return float(np.max(np.max(f, axis=0) - np.min(f, axis=0))) / float(model.quad_points.mu0)


def test_conservative_column_net_flux():
    model, levels = conservative_model()
    full = {}
    MS.ms_reference(model, levels, full=full)
    spread = flux_spread(model, full, levels)
    print("oracle net-flux spread / (mu0 F0): %.3e" % spread)
    assert 0 < spread < FLUX_SPREAD_BOUND
    full_s = {}
    MS.ms_segmented(model, levels, full=full_s)
    assert flux_spread(model, full_s, levels) < FLUX_SPREAD_BOUND
    # the bound is not vacuous: without the direct beam the "net flux" changes by tens of percent over the column
    f = [float(np.mean(full[(l, 0)][0][:, 0] - full[(l, 0)][1][:, 0])) for l in levels]
    assert max(f) - min(f) > 100 * FLUX_SPREAD_BOUND


def test_oracle_argument_validation():
    model, _ = _column("scalar_all_levels", np.random.default_rng(0))
    for bad in (-1, 7):
        with pytest.raises(ValueError):
            MS.ms_reference(model, [0, bad])
        with pytest.raises(ValueError):
            MS.ms_segmented(model, [bad])
    tr = np.tile(np.full(4, 0.05), (2, 1))
    tr[:, 2] = 0.0                                          # a non-scattering layer
    m2 = O.build_model("I", 9, 40.0, [30.0], [0.0], tau_rayl=tr, tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=1)
    with pytest.raises(NotImplementedError):
        MS.ms_reference(m2, [1])
    with pytest.raises(NotImplementedError):
        MS.ms_segmented(m2, [1])


def _host_model(vsm, **kw):
    H = vsm.host_model
    base = dict(tau_rayl=np.tile(np.full(4, 0.05), (2, 1)), tau_abs=np.full((2, 4), 1e-3), albedo=0.2, m_max=1)
    base.update(kw)
    return H.model_from_arrays(vsm.Architectures.GPU(0), "I", 9, 40.0, [30.0], [0.0], **base)


def test_api_argument_validation():
    """Checked on the host, before any device work: levels outside 0..Nz, non-integer levels, sources other than SolarBeam."""
    import vsmartmom_jl_amd as vsm
    H = vsm.host_model
    model = _host_model(vsm)
    for bad in ([-1], [0, 5], [1.5], []):
        with pytest.raises(ValueError):
            vsm.CoreRT.rt_run_multisensor(model, bad)
    B = np.full((4, 2), 1e-3)
    for srcs in ((H.ThermalEmission(B_layer=B),), (H.SolarBeam(), H.ThermalEmission(B_layer=B))):
        with pytest.raises(vsm.VSMError, match="SolarBeam"):
            vsm.CoreRT.rt_run_multisensor(_host_model(vsm, sources=srcs), [1])
