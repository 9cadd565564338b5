"""Geometries in which a viewing zenith angle shares the solar stream, for tests/test_oracle_geometry_nodes.py (CPU) and
tests/test_gpu_geometry_nodes.py (GPU).

rt_set_streams removes duplicate nodes (rt_set_streams.jl:25-47, Julia's `unique`): with vza == sza the viewing node and the
solar node merge.  Then Nquad is one smaller, i_mu0 points into the middle of the zero-weight tail, and a viewing row is the
solar row: the `mu_i == mu_j` / solar-row branches of the elemental and single-scattering source kernels run, and whatever a
surface builder writes into j0+ at the solar rows reaches T.

CASES[id] = (sza, vza, vaz); EXPECT[id] = (Nquad - nq, imu0 - nq, views on the solar node) with nq = (l_trunc + 2) // 2 the
number of weighted Gauss nodes, which every test asserts (check_streams) so that a change of the stream rule cannot turn the
cases into ordinary ones."""
import numpy as np

from oracle import vsm_oracle as O

CASES = {
    "sun_in_view": (40.0, [30.0, 40.0, 5.0], [0.0, 180.0, 60.0]),       # the solar node inside the tail
    "sun_only": (40.0, [40.0], [180.0]),                                 # a tail of one node that is both
    "repeated": (40.0, [30.0, 30.0, 40.0, 40.0], [0.0, 90.0, 0.0, 180.0]),   # repeated views, two of them on the sun
    "zenith": (0.0, [0.0, 30.0], [0.0, 10.0]),                           # mu0 = mu_v = 1, the end of the quadrature interval
    "near": (40.0, [40.0001, 30.0], [180.0, 0.0]),                       # two nodes ~1.1e-6 apart in mu, distinct in FP32 too
}
COINCIDENT = ["sun_in_view", "sun_only", "repeated", "zenith"]
# (tail length, position of the solar node in the tail, indices of the views that sit on the solar node)
EXPECT = {
    "sun_in_view": (3, 1, [1]),
    "sun_only": (1, 0, [0]),
    "repeated": (2, 1, [2, 3]),
    "zenith": (2, 0, [0]),
    "near": (3, 2, []),
}
# the table of the issue at nq = 5 (l_trunc = 9): (Nquad, imu0)
AT_NQ5 = {"sun_in_view": (8, 6), "sun_only": (6, 5), "repeated": (7, 6), "zenith": (7, 5), "near": (8, 7)}


def check_streams(case, qp, l_trunc):
    """Assert the stream layout of `case` on a QuadPoints-like object (oracle or host): Nquad, imu0, Nstreams."""
    nq = (l_trunc + 2) // 2
    tail, pos, _ = EXPECT[case]
    assert int(qp.Nquad) == nq + tail, (case, qp.Nquad, nq + tail)
    assert int(qp.imu0) == nq + pos, (case, qp.imu0, nq + pos)
    assert int(qp.Nstreams) == nq, (case, qp.Nstreams)
    if l_trunc == 9:
        assert (int(qp.Nquad), int(qp.imu0)) == AT_NQ5[case]


def view_rows(case, qp):
    """Node index of every view (postprocessing_vza.jl: the nearest node)."""
    _, vza, _ = CASES[case]
    mu = np.asarray(qp.qp_mu)
    return [int(np.argmin(np.abs(mu - mu.dtype.type(O.cosd(v))))) for v in vza]


def scene(S=3, L=3, aerosol=False, seed=5):
    """A small column: Rayleigh everywhere, one strongly absorbing layer (tau_abs ~ 3: a thick elemental layer at some points),
    a bright surface, and optionally an aerosol in the lowest layer (m_max 4).  Keyword arguments of O.build_model /
    model_from_arrays except the aerosol itself (see aerosols())."""
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(np.linspace(0.03, 0.12, L), (S, 1))
    tau_abs = 10.0 ** rng.uniform(-3, -0.5, (S, L))
    tau_abs[:, 1] = 3.0 * (1 + 0.1 * np.arange(S))
    kw = dict(tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.03, albedo=0.6, m_max=2)
    if aerosol:
        tau_aer = np.zeros((1, L))
        tau_aer[0, -1] = 0.2
        kw.update(tau_aer=tau_aer, m_max=4)
    return kw


def aerosols(M=O):
    """The aerosol of scene(aerosol=True) as objects of module M (the oracle or the host model)."""
    g = O.hg_greek(0.7, 8)
    greek = g if M is O else M.GreekCoefs(**vars(g))
    return [M.AerosolOptics(greek, 0.95, 0.1)]


def direct_beam(om):
    """The postprocessed direct beam of a forward run over a surface whose builder writes j0+ = I0 exp(-tau/mu0) at the solar
    rows (lambertian_surface.jl:75): [nStokes, S], the m = 0 weight 1/(2 pi) times I0 times the attenuation.  Interaction with
    the surface adds j0+ unchanged to the composite J0+ (interaction.jl: J0+ <- j0+ + t++ (I - R+- r-+)^-1 (...)), and m > 0
    builders write none."""
    lods = O.construct_core_optical_properties(om, 0)            # (the delta-M scaled optical depths the run walks)
    tau_total = O.extract_effective_props(lods, om.FT, O.deciding_type(om))[1][:, -1]
    att = np.exp(-tau_total / float(om.quad_points.mu0))
    return (0.5 / np.pi) * np.asarray(om.pol.I0, dtype=np.float64)[:om.pol.n, None] * att[None, :]


def gas_scene(S=2, L=3, scale=(1.0, 1.0), albedo=0.2, seed=0):
    """The linearized scene: two gases (x_g = multiplicative scale of gas g: d tau_abs / d x_g = base_g) and a Lambertian
    albedo, as test_oracle_lin._model.  Returns (keyword arguments of build_model / model_from_arrays, [base_a, base_b])."""
    rng = np.random.default_rng(seed)
    tau_rayl = np.tile(0.03 * np.ones(L), (S, 1))
    base_a = 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    base_b = 10.0 ** rng.uniform(-2.5, -0.5, (S, L))
    base_b[:, 0] = 0.0
    kw = dict(tau_rayl=tau_rayl, tau_abs=scale[0] * base_a + scale[1] * base_b, depol=0.0279, albedo=albedo, m_max=2)
    return kw, [base_a, base_b]


def oracle_model(case, pol, l_trunc, kw, aerosol=False, FT=np.float64, sza=None):
    """O.build_model of `case` (sza overrides the case's own: the continuity checks), with the stream layout asserted."""
    sza0, vza, vaz = CASES[case]
    om = O.build_model(pol, l_trunc, sza0 if sza is None else sza, vza, vaz, aerosols=aerosols() if aerosol else (), FT=FT, **kw)
    if sza is None:
        check_streams(case, om.quad_points, l_trunc)
    return om
