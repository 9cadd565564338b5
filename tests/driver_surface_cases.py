"""The scenes of the driver-by-surface grid (tests/test_gpu_driver_surfaces.py), oracle side: what the GPU tests and the CPU tests
that guard them (tests/test_oracle_raman.py, test_oracle_multisensor_raman.py, test_oracle_fluxes_raman.py, test_oracle_fluxes.py)
share.  Nothing here needs a GPU.

One column per shape: sza 40, vza [30, 0], three layers, m_max 2, S = 14 spectral points with differing absorption and a spectrally
varying unpolarized beam; the Raman lines are those of test_gpu_multisensor_raman.py (at S = 14 every line but the 40 is in band).
`aerosol=True` adds the synthetic aerosol of test_gpu_ss_lin._scene to the two lower layers (the linearized cells, whose Jacobians
have aerosol columns)."""
from __future__ import annotations

import numpy as np

from oracle import vsm_oracle as O
from oracle import vsm_oracle_brdf as OB
from oracle import vsm_oracle_coxmunk as CM
from oracle import vsm_oracle_raman as OR

SZA, VZA, VAZ = 40.0, [30.0, 0.0], [0.0, 60.0]
SHAPES = [("I", 9), ("IQU", 7)]          # N = 8 and N = 21
S, L, M_MAX = 14, 3, 2
LEVELS = [0, 2, 3]
A = 0.25                                 # the albedo of the degenerate identities
ALBEDO_FIELD = 0.6                       # what model.albedo holds where the surface object carries the albedo: never to be read
SHIFTS = np.array([-5, -2, -1, 1, 3, 40, 0])
W_IE = np.array([0.004, 0.012, 0.02, 0.018, 0.007, 0.3, 0.009])
VARPI_CABANNES = 0.96
RPV = (0.12, 0.08, 0.75, -0.25)          # the RPV surface of (b), on the scalar shape
WIND = 5.0                               # the Cox-Munk surface of (b), on the IQU shape
LEGENDRE = [0.25, 0.08, -0.03]           # the non-constant Legendre surface of (c)
AER_TAU = np.array([[0.0, 0.05, 0.15]])
AER_SSA, AER_FTRUNC, AER_G, AER_LMAX = 0.93, 0.12, 0.65, 7


def arrays(pol: str, seed: int = 11):
    """(tau_rayl, tau_abs [S, L], F0 [n, S])."""
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    tau_abs = (10.0 ** rng.uniform(-3, 0.3, (S, 1))) * np.linspace(0.5, 1.5, L)[None, :] / L
    F0 = np.zeros((O.polarization(pol).n, S))
    F0[0] = 0.8 + 0.4 * rng.random(S)
    return tau_rayl, tau_abs, F0


def model_kwargs(pol: str, albedo=A):
    tau_rayl, tau_abs, _ = arrays(pol)
    return dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=albedo, m_max=M_MAX)


def aerosol_greek():
    from test_oracle_lin import _hg_greek
    return _hg_greek(AER_G, AER_LMAX)


def oracle_model(pol: str, l_trunc: int, FT=np.float64, albedo=A, aerosol: bool = False) -> O.RTModel:
    """The oracle's model of the scene over a Lambertian surface (albedo: a scalar or a spectrum [S])."""
    kw = model_kwargs(pol, albedo)
    aer = []
    if aerosol:
        kw["tau_aer"] = AER_TAU
        aer = [O.AerosolOptics(aerosol_greek(), AER_SSA, AER_FTRUNC)]
    om = O.build_model(pol, l_trunc, SZA, list(VZA), list(VAZ), FT=FT, aerosols=aer, **kw)
    om.varpi_cabannes = VARPI_CABANNES
    om.F0 = arrays(pol)[2]
    return om


def oracle_rs() -> OR.RRS:
    return OR.RRS(i_shift=SHIFTS, varpi_ie=W_IE, greek_raman=O.get_greek_rayleigh(6.0 / 7.0 * 0.5))


def brdf_hook(om: O.RTModel, osurf):
    """The surface hook (m, added_surf, tau_sum) of the oracles for an OB.RPVSurface, OB.RossLiSurface or CM.CoxMunkSurface."""
    mu = om.quad_points.qp_mu.astype(np.float64)
    if isinstance(osurf, CM.CoxMunkSurface):
        return CM.surface_layer_hook(om, lambda m: CM.reflectance(osurf, om.pol.n, mu, m), coxmunk=osurf)
    return CM.surface_layer_hook(om, lambda m: OB.reflectance(osurf, om.pol.n, mu, m))


def rel_max(a, b) -> float:
    """max |a - b| relative to the largest |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def lambertian_hook(om: O.RTModel):
    """What the Raman and flux oracles had hard-wired before they took a hook: the scalar Lambertian builder on model.albedo."""
    return lambda m, a, ts: O.create_surface_layer_lambertian(om.albedo, a, m, om.pol, om.quad_points, ts, om.FT)


def degenerate_cases(om: O.RTModel):
    """[(name, model, hook, spectral)]: the Lambertian(A) scene `om` written as a constant BRDF or a constant albedo spectrum.  The
    BRDF cases carry ALBEDO_FIELD in model.albedo: a hook that is not honoured shows as half the signal.

    spectral: the surface layer comes from the reference's builder for LambertianSurfaceLegendre / Spline, which differs from the
    scalar one where the albedo does not enter (lambertian_surface.jl:135,154-156 against :75,90-91): j0+ = 0, and t++ = t-- = 0
    for m > 0.  r-+ and j0- are the scalar builder's, so every field that leaves the surface upwards is the same; the field that
    arrives at the bottom of the whole column (T, ieT, level-0 dw / dwie: J0+ of the composite that includes the surface layer)
    is not, and is left out of the comparison for this case."""
    import dataclasses
    other = dataclasses.replace(om, albedo=ALBEDO_FIELD)
    return [("rpv", other, brdf_hook(other, OB.RPVSurface(A, 1.0, 1.0, 0.0)), False),
            ("rossli", other, brdf_hook(other, OB.RossLiSurface(0.0, 0.0, A)), False),
            ("legendre", dataclasses.replace(om, albedo=O.legendre_albedo([A, 0.0], S, om.FT)), None, True)]


def black(om: O.RTModel) -> O.RTModel:
    import dataclasses
    return dataclasses.replace(om, albedo=0.0)


def lin_tables(pol: str, aerosol: bool):
    """What a LinModel of the scene takes: (gases [two [S, L] tables whose sum is tau_abs], tau_aer_dot [1, 7, L] or None, the
    aerosol's (greek_dot [4 GreekCoefs], ssa_dot, f_dot) or None) -- the directions of test_gpu_ss_lin._scene."""
    from test_oracle_lin import _hg_greek
    _, tau_abs, _ = arrays(pol)
    share = np.random.default_rng(3).uniform(0.3, 0.7, tau_abs.shape)
    share[:, 0] = 1.0                                      # the second gas is absent from the top layer
    gases = [tau_abs * share, tau_abs * (1.0 - share)]
    if not aerosol:
        return gases, None, None
    g0 = aerosol_greek()
    gdot = [_hg_greek(0.5 + 0.1 * k, AER_LMAX, 0.2 + 0.05 * k) for k in range(4)]
    for k, gd in enumerate(gdot):
        for name in ("alpha", "beta", "gamma", "delta", "epsilon", "zeta"):
            setattr(gd, name, 0.05 * (k + 1) * (getattr(gd, name) - getattr(g0, name)))
    tad = np.array([[[0.0, 1.0, 3.0], [0.0, 0.02, -0.05], [0.0, -0.03, 0.02], [0.0, 0.1, 0.2], [0.0, 0.01, 0.04],
                     [0.0, 0.5, -0.5], [0.0, -0.2, 0.3]]])
    return gases, tad, (gdot, np.array([0.02, -0.3, 0.05, 0.01]), np.array([0.01, 0.02, 0.2, -0.05]))
