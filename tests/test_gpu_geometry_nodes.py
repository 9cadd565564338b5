"""GPU tests at geometries where a viewing zenith angle shares the solar stream (tests/geometry_cases.py).

rt_set_streams removes duplicate nodes, so with vza == sza the viewing node and the solar node merge: Nquad is one smaller, i_mu0
points into the middle of the zero-weight tail and a viewing row is the solar row.  Then
  * the source kernels take their solar-row branch (`mu_i == mu_j` off the diagonal in elemental_pair, vsm_elemental.h; the index
    test i_start <= i < i_start + ns in k_elemental_sfi_lin, k_elemental_sfi, k_elemental_sfi_rrs and the k_ss_column* kernels);
  * what a surface builder writes into j0+ at the solar rows -- the direct beam -- lands in T (the beam table below);
  * the native run picks its view rows, its zero-weight tail and its sources-only rows from a node list with the solar node
    inside.

The beam table (read from the reference's builders; pinned in test_beam_table and, on the CPU, in test_oracle_geometry_nodes.py).
T at a view on the solar node holds the postprocessed direct beam w_m I0 exp(-tau / mu0):
  rt_run, LambertianSurfaceScalar          yes, at m = 0 only            lambertian_surface.jl:75 (m > 0: j0+ = 0, :92)
  rt_run, rpv / RossLi / CoxMunk           yes, at EVERY Fourier moment  rpv_surface.jl:85 is outside `if m == 0`, and CoxMunk
                                           has no forward builder of its own: the sum is (1/2pi + sum_m cos(m vaz) / pi) I0 att
  rt_run, LambertianSurfaceLegendre/Spline no                            lambertian_surface.jl:135,195 (j0+ = 0)
  rt_run_lin, Lambertian                   no                            lambertian_surface_lin.jl:107,149
  rt_run_lin, CoxMunk                      no                            coxmunk_surface_lin.jl:72
  rt_run_lin, rpv / RossLi                 no: the reference has no linearized builder for them; k_brdf_src_lin follows
                                           coxmunk_surface_lin.jl:72 (j0+ = 0)
  full output                              bhr_dw adds j0+[i_mu0] mu0 of the surface layer (interaction_hdrf.jl), against the oracle
So "R, T of rt_run_lin equal rt_run's" holds for R always and for T at every view off the solar node; at a view on it the two
differ by the beam, and the reference of a device central difference is the device's own rt_run_lin forward part.

Tolerances are those of the neighbouring test of each driver (named at each use)."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import geometry_cases as G  # noqa: E402
import ms_lin_oracle as MSL  # noqa: E402
import ms_oracle as MS  # noqa: E402
import ss_lin_oracle as SSL  # noqa: E402
import ss_oracle as SS  # noqa: E402
from oracle import vsm_oracle as O  # noqa: E402
from oracle import vsm_oracle_brdf as OB  # noqa: E402
from oracle import vsm_oracle_coxmunk as CM  # noqa: E402
from oracle import vsm_oracle_lin as OL  # noqa: E402
from oracle import vsm_oracle_raman as OR  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _rel_views(a, b):
    """The worst view's own relative error: at a view on the solar node T holds the direct beam, which would otherwise set
    the scale for the diffuse T of every other view."""
    return max(_rel(a[v], b[v]) for v in range(len(b)))


def _host_model(vsm, arch, case, pol, l_trunc, kw, aerosol=False, FT=np.float64, sza=None, **more):
    H = vsm.host_model
    sza0, vza, vaz = G.CASES[case]
    pm = H.model_from_arrays(arch, pol, l_trunc, sza0 if sza is None else sza, vza, vaz, float_type=FT,
                             aerosol_optics=G.aerosols(H) if aerosol else (), **more, **kw)
    if sza is None:
        G.check_streams(case, pm.quad_points, l_trunc)
    return pm


def _run(vsm, monkeypatch, pm, native):
    """Scene.run with NATIVE_RUN on / off: (R, T, moments on the native run)."""
    monkeypatch.setattr(vsm.CoreRT, "NATIVE_RUN", native)
    sc = vsm.CoreRT.prepare_scene(pm)
    nat = sc._native_moments()
    sc.run()
    torch.cuda.synchronize()
    vsm._lib.check_device_status("geometry run")
    R, T = sc.results_host()
    return R, T, nat


_ORACLE = {}


def _oracle(case, pol, l_trunc, aerosol, sza=None):
    """O.rt_run of the forward scene, computed once per geometry and shared."""
    key = (case, pol, l_trunc, aerosol, sza)
    if key not in _ORACLE:
        om = G.oracle_model(case, pol, l_trunc, G.scene(aerosol=aerosol), aerosol=aerosol, sza=sza)
        _ORACLE[key] = (om,) + tuple(O.rt_run(om))
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------------------------
# (a) forward rt_run, every kernel family, + (g) continuity across the merge
# ---------------------------------------------------------------------------------------------------------------------
# (pol, l_trunc, aerosol): fused kernels (N <= 32) | FP64 / FP32 strips | native run with 1-4 row tiles | five / six row tiles |
# n = 61..64 (no spare columns: the source vectors by mat-vecs), the ("I", 117) shape of test_gpu_native
FORWARD = [("I", 9, False), ("IQU", 9, False), ("IQU", 33, False), ("I", 21, True), ("IQU", 21, True), ("IQU", 35, False),
           ("I", 123, False), ("I", 117, False)]
# Gate (b) of test_gpu_fp32_accuracy.py: a ceiling per shape of about six times the error measured on MI355X (the worst of R, T and
# T off the solar node over the merged cases and both runs), never above 2e-3.
FP32_CEIL = {("I", 9): 2e-4,        # measured 2.9e-5
             ("IQU", 9): 2.1e-4,    # 3.4e-5
             ("IQU", 33): 2.1e-4,   # 3.5e-5
             ("I", 21): 8.1e-4,     # 1.35e-4 (the aerosol scenes: m_max = 4)
             ("IQU", 21): 8.3e-4,   # 1.38e-4
             ("IQU", 35): 2.1e-4,   # 3.5e-5
             ("I", 123): 2e-4,      # 3.2e-5
             ("I", 117): 2.1e-4,    # 3.4e-5
             ("I", 119): 2.1e-4}    # 5.8e-6 (sun_only; the ceiling of its sibling shape)
LIN32_CEIL = dict(R=1.7e-4, T=5.3e-5, Rd=2.6e-4, Td=1.7e-4)   # measured 2.7e-5, 8.8e-6, 4.3e-5, 2.8e-5


@pytest.mark.parametrize("pol,l_trunc,aerosol", FORWARD)
@pytest.mark.parametrize("case", list(G.CASES))
def test_forward_run_every_kernel_family(vsm, arch, monkeypatch, case, pol, l_trunc, aerosol):
    """rt_run with NATIVE_RUN on and off, FP64 and FP32.  FP64: 1e-8 against the oracle (T per view), 1e-10 between the native and
    the reference-layout run (test_gpu_native).  FP32: the exact-FP32 reference and gates of test_gpu_fp32_accuracy (T also on the
    views off the solar node alone); at `near` T of the view next to the sun answers to gate (a) alone."""
    from tests.test_gpu_fp32_accuracy import _device_run, _gate, _oracles
    kw = G.scene(aerosol=aerosol)
    if (pol, l_trunc) == ("I", 117):
        l_trunc += 2 * (3 - G.EXPECT[case][0] > 1)           # a tail of one node (sun_only): one more weighted node
    om, Ro, To = _oracle(case, pol, l_trunc, aerosol)
    N = om.quad_points.Nquad * om.pol.n
    if pol == "I" and l_trunc in (117, 119):
        assert 61 <= N <= 64, N
    pm = _host_model(vsm, arch, case, pol, l_trunc, kw, aerosol)
    Rn, Tn, nat = _run(vsm, monkeypatch, pm, True)
    Rl, Tl, natl = _run(vsm, monkeypatch, pm, False)
    assert nat == set(range(om.m_max + 1)) and natl == set(), (nat, natl)
    for name, (R, T) in (("native", (Rn, Tn)), ("layout", (Rl, Tl))):
        assert np.all(np.isfinite(R)) and np.all(np.isfinite(T)), name
        e = (_rel(R, Ro), _rel_views(T, To))
        print("GEO fwd %s %s/%d N=%d %s: R %.2e T %.2e" % (case, pol, l_trunc, N, name, e[0], e[1]))
        assert max(e) < 1e-8, (name, e)
    assert _rel(Rn, Rl) < 1e-10 and _rel_views(Tn, Tl) < 1e-10, (_rel(Rn, Rl), _rel_views(Tn, Tl))
    if case == "sun_in_view":
        # (g): R (and T off the solar node) is continuous across the merge: the device's step to sza = 40.0001 equals the
        # oracle's within the driver's tolerance.  Independent of the oracle's same-mu formulas being right.
        _, Ro2, To2 = _oracle(case, pol, l_trunc, aerosol, sza=40.0001)
        off = [v for v in range(len(To)) if v not in G.EXPECT[case][2]]
        step_o = np.max(np.abs(Ro2 - Ro)) / np.max(np.abs(Ro))
        assert step_o < 1e-4
        pm2 = _host_model(vsm, arch, case, pol, l_trunc, kw, aerosol, sza=40.0001)
        for native, (R1, T1) in ((True, (Rn, Tn)), (False, (Rl, Tl))):
            R2, T2, _ = _run(vsm, monkeypatch, pm2, native)
            print("GEO continuity %s/%d native=%d: oracle step %.2e device step %.2e"
                  % (pol, l_trunc, native, step_o, np.max(np.abs(R2 - R1)) / np.max(np.abs(Ro))))
            assert np.max(np.abs((R2 - R1) - (Ro2 - Ro))) <= 1e-8 * np.max(np.abs(Ro))
            assert np.max(np.abs((T2[off] - T1[off]) - (To2[off] - To[off]))) <= 1e-8 * np.max(np.abs(To[off]))
    # ---- FP32 ----
    pm32 = _host_model(vsm, arch, case, pol, l_trunc, kw, aerosol, FT=np.float32)
    om32 = G.oracle_model(case, pol, l_trunc, kw, aerosol=aerosol, FT=np.float32)
    (R32, T32), (Rx, Tx), tx = _oracles(om32)
    off = [v for v in range(len(Tx)) if v not in G.EXPECT[case][2]]
    c = FP32_CEIL[(pol, l_trunc)]
    ceil = dict(R=c, T=c, Toff=c)
    if case == "near":
        # the view 1.1e-6 from the solar node: no fixed ceiling exists there (test_near_nodes_fp32), so T at that view answers to
        # gate (a) alone -- at most 5 times the FP32 numpy oracle's own error against the exact reference -- and the rest as usual
        off, ceil = [1], dict(R=c, Toff=c, Tnear=np.inf)
    pm32_2 = _host_model(vsm, arch, case, pol, l_trunc, kw, aerosol, FT=np.float32, sza=40.0001) if case == "sun_in_view" else None
    for native in (True, False):
        R, T, nat, st, (trace, _) = _device_run(vsm, monkeypatch, pm32, native)
        assert trace == tx
        outs = dict(R=(R, R32, Rx))
        if case == "near":
            outs["Tnear"] = (T[[0]], T32[[0]], Tx[[0]])
        else:
            outs["T"] = (T, T32, Tx)
        if off:
            outs["Toff"] = (T[off], T32[off], Tx[off])
        _gate("geo %s %s/%d N=%d native=%d" % (case, pol, l_trunc, N, native), outs, ceil)
        if pm32_2 is not None:          # (g) in Float32: the step within the driver's FP32 ceiling of the oracle's FP64 step
            R2, T2, _ = _run(vsm, monkeypatch, pm32_2, native)
            _, Ro2, To2 = _oracle(case, pol, l_trunc, aerosol, sza=40.0001)
            assert np.max(np.abs((R2.astype(np.float64) - R) - (Ro2 - Ro))) <= c * np.max(np.abs(Ro))
            assert np.max(np.abs((T2[off].astype(np.float64) - T[off]) - (To2[off] - To[off]))) <= c * np.max(np.abs(To[off]))


@pytest.mark.parametrize("pol,l_trunc,aerosol", [("I", 9, False), ("IQU", 21, True), ("IQU", 35, False), ("I", 123, False)])
def test_sun_in_view_native_run_invariants(vsm, arch, monkeypatch, pol, l_trunc, aerosol):
    """The invariants the suite holds at ordinary geometries, with the solar node inside the tail and among the viewing rows:
    zero-weight-tail skip on vs off (1e-12, test_gpu_zw_tail), view-row and sources-only runs vs the full run (1e-12,
    test_gpu_sources_only / test_gpu_view_rows), rt_run_streams recovering rt_run (atol 1e-12, rtol 1e-10,
    test_rt_run_streams_recovers_rt_run), a graph replay bit for bit (test_scene_run_graph_replay_is_identical)."""
    CR = vsm.CoreRT
    kw = G.scene(aerosol=aerosol)
    pm = _host_model(vsm, arch, "sun_in_view", pol, l_trunc, kw, aerosol)
    monkeypatch.setattr(CR, "NATIVE_RUN", True)

    def full(**flags):
        for k, v in flags.items():
            monkeypatch.setattr(CR, k, v)
        sc = CR.prepare_scene(pm)
        assert sc._native_moments()
        sc.compute_hdrf = True
        sc.run()
        torch.cuda.synchronize()
        vsm._lib.check_device_status("invariants")
        return [np.asarray(x) for x in sc.results_host_full()]

    base = full(NATIVE_ZW_TAIL=True, NATIVE_SOURCES_ONLY=True, NATIVE_VIEW_ROWS=True)
    variants = dict(no_tail=full(NATIVE_ZW_TAIL=False, NATIVE_SOURCES_ONLY=True, NATIVE_VIEW_ROWS=True),
                    no_view_rows=full(NATIVE_ZW_TAIL=True, NATIVE_SOURCES_ONLY=True, NATIVE_VIEW_ROWS=False),
                    full_run=full(NATIVE_ZW_TAIL=True, NATIVE_SOURCES_ONLY=False, NATIVE_VIEW_ROWS=False),
                    dense_full_run=full(NATIVE_ZW_TAIL=False, NATIVE_SOURCES_ONLY=False, NATIVE_VIEW_ROWS=False))
    for name, out in variants.items():
        for k, (a, b) in enumerate(zip(base, out)):
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (name, k)
            if np.max(np.abs(b)) > 0:
                assert _rel(a, b) < 1e-12, (name, k, _rel(a, b))
    for k in ("NATIVE_ZW_TAIL", "NATIVE_SOURCES_ONLY", "NATIVE_VIEW_ROWS"):
        monkeypatch.setattr(CR, k, True)
    # full output against the oracle (test_rt_run_full_output_hdrf_bhr: 1e-9): bhr_dw carries its beam entry at i_mu0
    hd = {}
    O.rt_run(G.oracle_model("sun_in_view", pol, l_trunc, kw, aerosol=aerosol), hdrf=hd)
    R, T, ieR, ieT, hdr, bhr_uw, bhr_dw = base
    assert _rel(hdr, hd["hdr"]) < 1e-9 and _rel(bhr_uw, hd["bhr_uw"][0]) < 1e-9 and _rel(bhr_dw, hd["bhr_dw"][0]) < 1e-9
    # rt_run_streams
    st = CR.rt_run_streams(pm)
    n = st.pol_n
    assert st.i_mu0 == pm.quad_points.imu0 + 1
    R_rec, T_rec = np.zeros_like(R), np.zeros_like(T)
    for i, (vz, va) in enumerate(zip(pm.vza, pm.vaz)):
        imu = int(np.argmin(np.abs(st.qp_mu - st.qp_mu.dtype.type(O.cosd(vz)))))
        for mi, w in enumerate(st.weight):
            c_, s_ = O.cosd(mi * va), O.sind(mi * va)
            sw = np.array([c_, c_, s_, s_][:n])
            R_rec[i] += w * sw[:, None] * st.J_m_per_m[mi][imu * n:(imu + 1) * n, 0, :]
            T_rec[i] += w * sw[:, None] * st.J_p_per_m[mi][imu * n:(imu + 1) * n, 0, :]
    assert np.allclose(R_rec, R, atol=1e-12, rtol=1e-10) and np.allclose(T_rec, T, atol=1e-12, rtol=1e-10)
    # graph replay (run_graph captures scenes that run entirely in the fused layer kernels: one scatterer per layer, N on chip)
    if aerosol or l_trunc == 123:
        return
    scene = CR.prepare_scene(pm)
    ref = [x.clone() for x in scene.run()]
    for _ in range(2):
        out = scene.run_graph()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, out))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the beam table
# ---------------------------------------------------------------------------------------------------------------------
def _beam_every_moment(om, vaz):
    """The BRDF builders write the beam at every Fourier moment (rpv_surface.jl:80-87 is outside `if m == 0`): I0 = e1, so the
    I component alone gets (1/2pi + sum_{m >= 1} cos(m vaz) / pi) att."""
    b = G.direct_beam(om)
    f = 0.5 / np.pi + sum(O.cosd(m * vaz) / np.pi for m in range(1, om.m_max + 1))
    return b * (f / (0.5 / np.pi))


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("case", ["sun_in_view", "repeated"])
def test_beam_table(vsm, arch, case, pol):
    """Every row of the table in the module docstring against the oracle of the same builder (1e-9: test_gpu_parity's bound for
    the surfaces, test_gpu_brdf's for rpv / RossLi; 1e-8 for CoxMunk and the Jacobians), and as a hard check: each "yes" run
    differs from a "no" run over the same reflectance by the oracle's beam term at the views on the solar node and by nothing
    (1e-12 of T's scale) elsewhere, and that beam term is not zero."""
    H, CR, CL = vsm.host_model, vsm.CoreRT, vsm.CoreRTLin
    l_trunc = 9
    kw, bases = G.gas_scene(S=3)
    geo = (case, pol, l_trunc)
    om = G.oracle_model(*geo, kw)
    S = om.tau_rayl.shape[0]
    on = G.EXPECT[case][2]
    vaz = G.CASES[case][2]
    beam = G.direct_beam(om)
    assert np.min(beam[0]) > 1e-3
    lin_o, lin_h = OL.LinModel(bases), H.LinModel(bases)

    def check_difference(T_yes, T_no, beam_of_view, what):
        scale = np.max(np.abs(T_yes))
        for v in range(len(T_yes)):
            want = beam_of_view(v) if v in on else 0.0 * beam
            d = T_yes[v] - T_no[v]
            assert np.max(np.abs(d - want)) <= 1e-12 * scale, (what, v, np.max(np.abs(d - want)) / scale)
            if v in on:
                assert np.max(np.abs(d[0])) > 1e-3, (what, v)

    # LambertianSurfaceScalar: rt_run yes, rt_run_lin no
    R, T = CR.rt_run(_host_model(vsm, arch, *geo, kw))
    Ro, To = O.rt_run(om)
    assert _rel(R, Ro) < 1e-9 and _rel_views(T, To) < 1e-9
    Rl, Tl, Rd, Td = CL.rt_run_lin(_host_model(vsm, arch, *geo, kw), lin_h, 0, 2, 1)
    Rlo, Tlo, Rdo, Tdo = OL.rt_run_lin(om, lin_o)
    assert _rel(Rl, Rlo) < 1e-9 and _rel_views(Tl, Tlo) < 1e-9
    assert _rel(Rl, R) < 1e-12
    check_difference(T, Tl, lambda v: beam, "Lambertian rt_run - rt_run_lin")
    # full output: bhr_dw with its beam entry j0+[i_mu0] mu0 (interaction_hdrf.jl:4-42), 1e-9 as test_rt_run_full_output_hdrf_bhr
    hd = {}
    O.rt_run(om, hdrf=hd)
    full = CR.rt_run(_host_model(vsm, arch, *geo, kw), full_output=True)
    assert _rel(full[4], hd["hdr"]) < 1e-9 and _rel(full[5], hd["bhr_uw"][0]) < 1e-9 and _rel(full[6], hd["bhr_dw"][0]) < 1e-9
    mu0 = om.quad_points.mu0
    diffuse = np.sum(hd["bhr_dw"][0]) - np.sum(np.pi * 2 * beam[0] * mu0)      # the beam entry is exp(-tau/mu0) mu0 = 2 pi beam mu0
    assert diffuse > 0 and np.min(2 * np.pi * beam[0] * mu0) > 1e-2
    # Legendre / Spline with the same constant albedo: no beam; their m > 0 builders also zero t++ (lambertian_surface.jl:154,
    # :211), so T is compared on the m = 0 runs
    kw0 = dict(kw, m_max=0)
    noalb = {k: v for k, v in kw0.items() if k != "albedo"}
    T0 = CR.rt_run(_host_model(vsm, arch, *geo, kw0))[1]
    for surf in (H.LambertianSurfaceLegendre([kw["albedo"], 0.0]), H.LambertianSurfaceSpline(np.full(S, kw["albedo"]))):
        Rs, Ts = CR.rt_run(_host_model(vsm, arch, *geo, noalb, surface=surf))
        Rso, Tso = O.rt_run(dataclasses.replace(om, m_max=0, albedo=np.full(S, kw["albedo"])))
        assert _rel(Rs, Rso) < 1e-9 and _rel_views(Ts, Tso) < 1e-9, type(surf).__name__
        check_difference(T0, Ts, lambda v: beam, "Scalar - " + type(surf).__name__)
    # rpv / RossLi: rt_run yes (every moment); their rt_run_lin (NSurf 4 / 3) no
    import brdf_lin_oracle as BL
    nokw = {k: v for k, v in kw.items() if k != "albedo"}
    for hs, osurf, nsurf in ((H.rpvSurfaceScalar(0.12, 0.08, 0.75, -0.25), OB.RPVSurface(0.12, 0.08, 0.75, -0.25), 4),
                             (H.RossLiSurfaceScalar(0.05, 0.03, 0.10), OB.RossLiSurface(0.05, 0.03, 0.10), 3)):
        pmb = _host_model(vsm, arch, *geo, nokw, surface=hs)
        Rb, Tb = CR.rt_run(pmb)
        Rbo, Tbo = OB.rt_run(om, osurf)
        assert _rel(Rb, Rbo) < 1e-9 and _rel_views(Tb, Tbo) < 1e-9, type(hs).__name__
        Rbl, Tbl, Rbd, Tbd = CL.rt_run_lin(pmb, lin_h, 0, 2, nsurf)
        ref = BL.rt_run_lin(om, lin_o, osurf)
        assert _rel(Rbl, ref[0]) < 1e-9 and _rel_views(Tbl, ref[1]) < 1e-9, type(hs).__name__
        for p in range(Rbd.shape[-1]):
            assert _rel(Rbd[..., p], ref[2][..., p]) < 1e-8 and _rel(Tbd[..., p], ref[3][..., p]) < 1e-8, (type(hs).__name__, p)
        assert _rel(Rbl, Rb) < 1e-12
        check_difference(Tb, Tbl, lambda v: _beam_every_moment(om, vaz[v]), type(hs).__name__ + " rt_run - rt_run_lin")
    # CoxMunk: the generic forward builder (rpv_surface.jl:51-97, no builder of its own): yes; rt_run_lin: no
    hcm, ocm = H.CoxMunkSurface(5.0), CM.CoxMunkSurface(5.0)
    pmc = _host_model(vsm, arch, *geo, nokw, surface=hcm)
    sc = CR.prepare_scene(pmc)
    sc.ss_correction = False                     # (the TMS term touches R only; rt_run_lin applies none)
    sc.run()
    torch.cuda.synchronize()
    Rc, Tc = sc.results_host()
    Rco, Tco = CM.rt_run(om, ocm, ss_correction=False)
    assert _rel(Rc, Rco) < 1e-8 and _rel_views(Tc, Tco) < 1e-8
    Rcl, Tcl, Rcd, Tcd = CL.rt_run_lin(pmc, lin_h, 0, 2, 1)
    ref = CM.rt_run_lin(om, lin_o, ocm)
    assert _rel(Rcl, ref[0]) < 1e-8 and _rel_views(Tcl, ref[1]) < 1e-8
    for p in range(Rcd.shape[-1]):
        assert _rel(Rcd[..., p], ref[2][..., p]) < 1e-8 and _rel(Tcd[..., p], ref[3][..., p]) < 1e-8, ("CoxMunk", p)
    check_difference(Tc, Tcl, lambda v: _beam_every_moment(om, vaz[v]), "CoxMunk rt_run - rt_run_lin")


# ---------------------------------------------------------------------------------------------------------------------
# (c) rt_run_lin
# ---------------------------------------------------------------------------------------------------------------------
LIN_N = {9: "operator level", 31: "fused strip kernels", 41: "strip128lin"}


@pytest.mark.parametrize("l_trunc", list(LIN_N))
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only", "zenith"])
def test_rt_run_lin_lanes_fold_precisions(vsm, arch, case, l_trunc):
    """rt_run_lin (IQU; N = 24 / 57 / 72 at sun_in_view) against OL: 1e-9 forward, 1e-8 Jacobians (test_rt_run_lin_vs_oracle_and_fd);
    lanes = 1 / 2 and fold on / off against the sequential walk at 1e-13 (test_rt_run_lin_moment_lanes_equal_sequential); FP32
    against the exact-FP32 reference at test_linearized_fp32_run's gates (ceilings of six times the measured error); and against central
    differences (h = 1e-4; max 1e-3, mean 1e-4 of the slot's maximum: test_rt_run_lin_vs_oracle_and_fd's bound) of the device's OWN
    rt_run_lin forward part -- rt_run's forward part is the wrong reference here: at the view on the solar node its T carries the
    direct beam, whose gas derivative the linearized T does not have."""
    from tests.test_gpu_fp32_accuracy import _gate
    H, CL = vsm.host_model, vsm.CoreRTLin
    pol = "IQU"
    kw, bases = G.gas_scene(S=3)
    om = G.oracle_model(case, pol, l_trunc, kw)
    ref = OL.rt_run_lin(om, OL.LinModel(bases))
    pm = _host_model(vsm, arch, case, pol, l_trunc, kw)
    scene = CL.SceneLin(pm, H.LinModel(bases), 0, 2, 1)
    if case == "sun_in_view":
        assert scene.N == {9: 24, 31: 57, 41: 72}[l_trunc]
    runs = {}
    for name, args in (("seq", dict(lanes=1)), ("lanes2", dict(lanes=2, fold=False)), ("fold", dict(lanes=2, fold=True)),
                       ("default", dict())):
        scene.run(**args)
        torch.cuda.synchronize()
        vsm._lib.check_device_status("rt_run_lin " + name)
        runs[name] = scene.results_host()
    names = ("R", "T", "Rd", "Td")
    for name, out in runs.items():
        for k, (a, b) in enumerate(zip(out, ref)):
            assert np.all(np.isfinite(a)), (name, names[k])
            if k < 2:
                e = _rel(a, b) if k == 0 else _rel_views(a, b)
                assert e < 1e-9, (name, names[k], e)
            else:
                for p in range(b.shape[-1]):
                    assert _rel(a[..., p], b[..., p]) < 1e-8, (name, names[k], p, _rel(a[..., p], b[..., p]))
        for k, (a, b) in enumerate(zip(out, runs["seq"])):
            assert _rel(a, b) < 1e-13, (name, names[k], _rel(a, b))
    # central differences of the device's own linearized forward part (gas a, albedo)
    R, T, Rd, Td = runs["seq"]
    h = 1e-4
    for p, (kp, km) in ((0, (dict(scale=(1 + h, 1.0)), dict(scale=(1 - h, 1.0)))), (2, (dict(albedo=0.2 + h), dict(albedo=0.2 - h)))):
        outp = CL.rt_run_lin(_host_model(vsm, arch, case, pol, l_trunc, G.gas_scene(S=3, **kp)[0]), H.LinModel(bases), 0, 2, 1)
        outm = CL.rt_run_lin(_host_model(vsm, arch, case, pol, l_trunc, G.gas_scene(S=3, **km)[0]), H.LinModel(bases), 0, 2, 1)
        for an, fd, name in ((Rd[..., p], (outp[0] - outm[0]) / (2 * h), "R"), (Td[..., p], (outp[1] - outm[1]) / (2 * h), "T")):
            err = np.abs(fd - an) / np.abs(fd).max()
            assert err.max() < 1e-3 and err.mean() < 1e-4, (p, name, err.max(), err.mean())
    # FP32
    pm32 = _host_model(vsm, arch, case, pol, l_trunc, kw, FT=np.float32)
    om32 = G.oracle_model(case, pol, l_trunc, kw, FT=np.float32)
    got = CL.rt_run_lin(pm32, H.LinModel(bases), 0, 2, 1)
    o32, ox = OL.rt_run_lin(om32, OL.LinModel(bases)), OL.rt_run_lin(O.exact_model(om32), OL.LinModel(bases))
    outs, ceil = dict(R=(got[0], o32[0], ox[0]), T=(got[1], o32[1], ox[1])), dict(R=LIN32_CEIL["R"], T=LIN32_CEIL["T"])
    for p in range(3):
        outs["Rd%d" % p], outs["Td%d" % p] = (got[2][..., p], o32[2][..., p], ox[2][..., p]), (got[3][..., p], o32[3][..., p], ox[3][..., p])
        ceil["Rd%d" % p], ceil["Td%d" % p] = LIN32_CEIL["Rd"], LIN32_CEIL["Td"]
    _gate("geo lin %s IQU/%d" % (case, l_trunc), outs, ceil)


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("surface", ["coxmunk", "legendre", "rpv", "rossli"])
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only", "zenith"])
def test_rt_run_lin_surface_slots(vsm, arch, case, surface, FT):
    """rt_run_lin with NSurf = 1 (CoxMunk wind speed), 3 (LambertianSurfaceLegendre; RossLi) and 4 (rpv) at the merged node, a
    tail of one node and mu0 = mu_v = 1 (NSurf = 1 Lambertian: test_rt_run_lin_lanes_fold_precisions), against the oracle of each
    builder.  Bounds of test_gpu_brdf_lin / test_gpu_spectral_albedo_lin / test_c3_ocean_coxmunk_linearized: FP64 1e-8 per array
    and slot (R at 1e-9 where those files hold it; T per view), Float32 1e-2 against the FP64 oracle."""
    import brdf_lin_oracle as BL
    import spectral_albedo_lin_oracle as SA
    H, CL = vsm.host_model, vsm.CoreRTLin
    kw, bases = G.gas_scene(S=3)
    noalb = {k: v for k, v in kw.items() if k != "albedo"}
    lin_o, lin_h = OL.LinModel(bases), H.LinModel(bases)
    coeff = [0.25, 0.08, -0.03]
    if surface == "legendre":
        om = G.oracle_model(case, "IQU", 9, dict(noalb, albedo=O.legendre_albedo(coeff, 3)))
        hs, nsurf, ref = H.LambertianSurfaceLegendre(coeff), 3, SA.rt_run_lin(om, lin_o, SA.legendre_basis(3, 3))
    else:
        om = G.oracle_model(case, "IQU", 9, kw)
        if surface == "coxmunk":
            hs, nsurf, ref = H.CoxMunkSurface(5.0), 1, CM.rt_run_lin(om, lin_o, CM.CoxMunkSurface(5.0))
        elif surface == "rpv":
            hs, nsurf, ref = H.rpvSurfaceScalar(0.12, 0.08, 0.75, -0.25), 4, BL.rt_run_lin(om, lin_o, OB.RPVSurface(0.12, 0.08, 0.75, -0.25))
        else:
            hs, nsurf, ref = H.RossLiSurfaceScalar(0.05, 0.03, 0.10), 3, BL.rt_run_lin(om, lin_o, OB.RossLiSurface(0.05, 0.03, 0.10))
    got = CL.rt_run_lin(_host_model(vsm, arch, case, "IQU", 9, noalb, FT=FT, surface=hs), lin_h, 0, 2, nsurf)
    assert got[2].shape == ref[2].shape == ref[0].shape + (2 + nsurf,)
    t_fwd, t_jac = (1e-8, 1e-8) if FT == np.float64 else (1e-2, 1e-2)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert _rel(got[0], ref[0]) < t_fwd and _rel_views(got[1], ref[1]) < t_fwd, (_rel(got[0], ref[0]), _rel_views(got[1], ref[1]))
    for p in range(2 + nsurf):
        assert np.max(np.abs(ref[2][..., p])) > 0
        e = (_rel(got[2][..., p], ref[2][..., p]), _rel(got[3][..., p], ref[3][..., p]))
        assert max(e) < t_jac, (p, e)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the other drivers
# ---------------------------------------------------------------------------------------------------------------------
def _rs_pair(vsm):
    shifts, w_ie = np.array([-2, -1, 1, 2, 0]), np.array([0.004, 0.012, 0.02, 0.018, 0.009])
    graman = O.get_greek_rayleigh(6.0 / 7.0 * 0.5)
    return (OR.RRS(i_shift=shifts, varpi_ie=w_ie, greek_raman=graman),
            vsm.CoreRTRaman.RRS(shifts, w_ie, vsm.host_model.GreekCoefs(**vars(graman))))


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only"])
def test_single_scattering_runs(vsm, arch, case, pol):
    """rt_run_ss elastic, Raman and linearized: a viewing row that IS the solar row in the k_ss_column* kernels.  1e-8 for a whole
    run (TOL_RUN of test_gpu_ss.py / test_gpu_ss_lin.py)."""
    H = vsm.host_model
    kw = G.scene(S=5)
    om, pm = G.oracle_model(case, pol, 9, kw), _host_model(vsm, arch, case, pol, 9, kw)
    om.varpi_cabannes = pm.varpi_Cabannes = 0.96
    got, ref = vsm.CoreRT.rt_run_ss(pm), SS.rt_run_ss(om)
    for k in (0, 1, 4, 5):                            # R, T, hem_R, hem_T
        assert np.max(np.abs(ref[k])) > 0 and _rel(got[k], ref[k]) <= 1e-8, ("elastic", k, _rel(got[k], ref[k]))
    for k in (2, 3):                                  # the elastic run's inelastic slots are zero
        assert not np.any(ref[k]) and not np.any(got[k]), ("elastic", k)
    ors, prs = _rs_pair(vsm)
    got, ref = vsm.CoreRTRaman.rt_run_ss(prs, pm, 1), SS.rt_run_ss_rrs(om, ors)
    assert np.max(np.abs(ref[2])) > 0 and np.max(np.abs(ref[3])) > 0
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.max(np.abs(r)) > 0 and _rel(g, r) <= 1e-8, ("raman", k, _rel(g, r))
    gkw, bases = G.gas_scene(S=3)
    om, pm = G.oracle_model(case, pol, 9, gkw), _host_model(vsm, arch, case, pol, 9, gkw)
    got = vsm.CoreRTLin.rt_run_ss(pm, H.LinModel(bases), 0, 2, 1)
    ref = SSL.rt_run_ss_lin(om, OL.LinModel(bases))
    assert _rel(got[0], ref[0]) <= 1e-8 and _rel(got[1], ref[1]) <= 1e-8
    for p in range(3):
        assert _rel(got[2][..., p], ref[2][..., p]) <= 1e-8, ("ss lin Rdot", p)
        if p < 2:
            assert _rel(got[3][..., p], ref[3][..., p]) <= 1e-8, ("ss lin Tdot", p)
        else:                                         # the albedo does not reach the single-scattering T
            assert not np.any(ref[3][..., p]) and not np.any(got[3][..., p])


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only"])
def test_raman_run(vsm, arch, case, pol):
    """CoreRTRaman.rt_run: k_elemental_sfi_rrs at a viewing row that is the solar row (test_gpu_raman's FP64 bound for a run: 1e-8)."""
    kw = G.scene(S=5)
    om, pm = G.oracle_model(case, pol, 9, kw), _host_model(vsm, arch, case, pol, 9, kw)
    om.varpi_cabannes = pm.varpi_Cabannes = 0.96
    ors, prs = _rs_pair(vsm)
    ref = OR.rt_run_rrs(om, ors)
    got = vsm.CoreRTRaman.rt_run(prs, pm, 1)
    assert np.max(np.abs(ref[2])) > 0 and np.max(np.abs(ref[3])) > 0
    for k, name in enumerate(("R", "T", "ieR", "ieT")):
        e = _rel(got[k], ref[k]) if k != 1 else _rel_views(got[k], ref[k])
        assert e < 1e-8, (name, e)


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only"])
def test_multisensor_runs(vsm, arch, monkeypatch, case, pol):
    """rt_run_multisensor at levels [0, 1, Nz], plain, thermal=True and linearized.  Level 0 is the matching rt_run bit for bit;
    every level against ms_oracle / ms_thermal_oracle / ms_lin_oracle at test_gpu_multisensor's 1e-10 (or twice rt_run's own
    deviation from the oracle on the scene, where that is larger), the Jacobians at 1e-8.  The down-welling radiance at the solar
    node of the inner levels is a view here, so it is checked with the rest."""
    import ms_thermal_oracle as MT
    H, CR = vsm.host_model, vsm.CoreRT
    kw = G.scene()
    S, L = kw["tau_rayl"].shape
    levels = [0, 1, L]
    om, pm = G.oracle_model(case, pol, 9, kw), _host_model(vsm, arch, case, pol, 9, kw)
    R, T = CR.rt_run(pm)
    Ro, To = O.rt_run(om)
    e_rt = max(_rel(R, Ro), _rel(T, To))
    tol = max(1e-10, 2 * e_rt)
    uw, dw = CR.rt_run_multisensor(pm, levels)
    assert np.array_equal(uw[0], R) and np.array_equal(dw[0], T)
    uo, do = MS.ms_reference(om, levels)
    for i, l in enumerate(levels):
        assert np.all(np.isfinite(uw[i])) and np.all(np.isfinite(dw[i]))
        assert _rel(uw[i], uo[i]) <= tol and _rel_views(dw[i], do[i]) <= tol, (l, _rel(uw[i], uo[i]), _rel_views(dw[i], do[i]))
    # thermal
    B = 0.05 + 0.01 * np.arange(L)[:, None] * np.ones((1, S))
    pmt = _host_model(vsm, arch, case, pol, 9, kw, sources=(H.SolarBeam(), H.ThermalEmission(B_layer=B)))
    Rt, Tt = CR.rt_run(pmt)
    Rto, Tto = O.rt_run_thermal(om, B)
    assert _rel(Rt - R, Rto) < 1e-8 and _rel(Tt - T, Tto) < 1e-8          # (test_gpu_thermal's bound for the slot)
    uwt, dwt = CR.rt_run_multisensor(pmt, levels, thermal=True)
    assert np.array_equal(uwt[0], Rt) and np.array_equal(dwt[0], Tt)
    uto, dto = MT.ms_total_reference(om, B, levels)
    for i, l in enumerate(levels):
        assert _rel(uwt[i], uto[i]) <= max(tol, 1e-8) and _rel_views(dwt[i], dto[i]) <= max(tol, 1e-8), ("thermal", l)
    # linearized: level 0 is rt_run_lin (no beam in dw at the solar node: the exception the beam table states)
    gkw, bases = G.gas_scene(S=3)
    omg, pmg = G.oracle_model(case, pol, 9, gkw), _host_model(vsm, arch, case, pol, 9, gkw)
    sl = vsm.CoreRTLin.SceneLin(pmg, H.LinModel(bases), 0, 2, 1)     # (level 0 is the sequential walk bit for bit:
    sl.run(lanes=1, fold=False)                                      #  test_gpu_multisensor_lin)
    torch.cuda.synchronize()
    out = sl.results_host()
    got = vsm.CoreRTLin.rt_run_multisensor(pmg, H.LinModel(bases), 0, 2, 1, levels)
    ref = MSL.ms_lin_segmented(omg, OL.LinModel(bases), levels)
    for k in range(4):
        assert np.array_equal(got[k][0], out[k]), k
        for i, l in enumerate(levels):
            e = _rel(got[k][i], ref[k][i])
            assert e <= (1e-9 if k < 2 else 1e-8), ("lin", k, l, e)
    on = G.EXPECT[case][2]
    T_fwd = CR.rt_run(pmg)[1]
    assert np.max(np.abs(T_fwd[on[0]] - got[1][0][on[0]] - G.direct_beam(omg))) <= 1e-12 * np.max(np.abs(T_fwd))


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only"])
def test_surface_sif_and_coxmunk_tms(vsm, arch, case, pol):
    """rt_run with SurfaceSIF against sif_oracle (1e-8: test_gpu_sif's bound for the native FP64 run), and rt_run over CoxMunk
    with its single-scattering (TMS) correction on, against CM.rt_run (1e-8: test_c3_ocean_coxmunk_forward) -- the correction's
    coefficients are evaluated at a view whose mu equals mu0, in the backscattering direction for vaz = 180."""
    import sif_oracle as SO
    H, CR = vsm.host_model, vsm.CoreRT
    kw = G.scene()
    S = kw["tau_rayl"].shape[0]
    sif0 = 0.01 * (1 + 0.2 * np.arange(S))
    om = G.oracle_model(case, pol, 9, kw)
    R, T = CR.rt_run(_host_model(vsm, arch, case, pol, 9, kw, sources=(H.SolarBeam(), H.SurfaceSIF(sif0))))
    Ro, To = SO.rt_run_sif(om, sif0)
    assert _rel(R, Ro) < 1e-8 and _rel_views(T, To) < 1e-8, (_rel(R, Ro), _rel_views(T, To))
    R0, _ = O.rt_run(om)
    assert _rel(Ro, R0) > 1e-3                       # the emission is in R
    nokw = {k: v for k, v in kw.items() if k != "albedo"}
    Rc, Tc = CR.rt_run(_host_model(vsm, arch, case, pol, 9, nokw, surface=H.CoxMunkSurface(5.0)))
    Rco, Tco = CM.rt_run(om, CM.CoxMunkSurface(5.0))
    Rc0, _ = CM.rt_run(om, CM.CoxMunkSurface(5.0), ss_correction=False)
    assert _rel(Rc, Rco) < 1e-8 and _rel_views(Tc, Tco) < 1e-8, (_rel(Rc, Rco), _rel_views(Tc, Tco))
    assert np.max(np.abs(Rco - Rc0)) > 0             # the correction is not zero here


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("n", [3, 4])
def test_standalone_ss_exact_back_and_forward_scattering(vsm, arch, FT, n):
    """StandaloneSS vector paths 1 and 2 at mu_v = mu0 with dphi = 0 and pi -- scattering angles of exactly 0 and pi in one of
    the two hemispheres, where the rotation angles of the phase matrix are 0 / 0 -- and at nadir (mu_v = 1, any dphi), against
    exact_ss_oracle at test_gpu_exact_ss's bounds (1e-10 / 5e-4).  The existing tests have mu_v = mu0 only at dphi = 0.9."""
    import math

    import exact_ss_oracle as X
    from tests.test_gpu_exact_ss import MU0, _check, build
    ocfg, pcfg = build(vsm, arch, FT, 70, 5, 3, 4, n_stokes=n, surface="0.3", vector=True)
    mu_v, dphi = [MU0, MU0, 1.0], [0.0, math.pi, 0.7]
    ocfg = dataclasses.replace(ocfg, geometry=X.SSGeometry(MU0, mu_v, dphi))
    pcfg = vsm.StandaloneSS.replace(pcfg, geometry=vsm.StandaloneSS.SSGeometry(MU0, mu_v, dphi))
    want = X.run_exact_ss(ocfg, "paths_1_2")
    got = vsm.StandaloneSS.run_exact_ss(pcfg, "paths_1_2")
    for k in ("path1", "path2", "total"):
        assert np.all(np.isfinite(getattr(want, k))) and np.all(np.isfinite(getattr(got, k))), k
        _check(k, getattr(got, k), getattr(want, k), FT)


@pytest.mark.parametrize("pol", ["I", "IQU"])
@pytest.mark.parametrize("case", ["sun_in_view", "sun_only"])
def test_multisensor_raman_run(vsm, arch, case, pol):
    """CoreRTRaman.rt_run_multisensor at levels [0, 1, Nz]: level 0 is CoreRTRaman.rt_run bit for bit, every level against
    ms_raman_oracle at test_gpu_multisensor_raman's 1e-8 per Stokes component."""
    import ms_raman_oracle as MR
    from tests.test_gpu_multisensor_raman import _rel_per_component
    kw = G.scene(S=5)
    L = kw["tau_rayl"].shape[1]
    levels = [0, 1, L]
    om, pm = G.oracle_model(case, pol, 9, kw), _host_model(vsm, arch, case, pol, 9, kw)
    om.varpi_cabannes = pm.varpi_Cabannes = 0.96
    ors, prs = _rs_pair(vsm)
    ref = MR.ms_raman_reference(om, ors, levels)
    got = vsm.CoreRTRaman.rt_run_multisensor(prs, pm, levels)
    run = vsm.CoreRTRaman.rt_run(prs, pm, 1)
    assert len(got) == 4
    for k, name in enumerate(("uw", "dw", "uwie", "dwie")):
        assert np.array_equal(got[k][0], run[k]), name
        for i, l in enumerate(levels):
            assert np.all(np.isfinite(got[k][i])) and np.max(np.abs(ref[k][i])) > 0, (name, l)
            e = _rel_per_component(got[k][i], ref[k][i])
            assert e <= 1e-8, (name, l, e)


# ---------------------------------------------------------------------------------------------------------------------
# (e) kernel level: i_mu0 anywhere
# ---------------------------------------------------------------------------------------------------------------------
def _quad_with_sun_at(qp, pos):
    """The oracle's QuadPoints with the solar node moved to node `pos` (imu0 is a plain field; mu0 follows)."""
    return dataclasses.replace(qp, imu0=int(pos), mu0=float(qp.qp_mu[pos]))


def _sun_positions(qp):
    return {"first": 0, "weighted": qp.Nstreams // 2, "tail_first": qp.Nstreams, "last": qp.Nquad - 1}


@pytest.mark.parametrize("FT", [np.float64, np.float32])
@pytest.mark.parametrize("pol_name,l_trunc", [("I", 9), ("IQU", 9), ("I", 115)])            # N = 7, 21, 60
@pytest.mark.parametrize("where", ["first", "weighted", "tail_first", "last"])
def test_elemental_kernels_with_the_sun_at_any_node(vsm, arch, pol_name, l_trunc, FT, where):
    """vsm_elemental (ndoubl = 0 and 3, m = 0 and 1) and the fused vsm_elemental_doubling with i_mu0 set by hand to the first
    node, a weighted node in the middle, the first tail node and the last node, against O.elemental / O.doubling at
    test_elemental's bounds (1e-12 FP64, 1e-5 FP32; fused: see below / 5e-4).  With the solar node on a weighted stream and F0 = e1,
    the source vectors are the matrix columns j = i_mu0 up to known factors: j0+ = (t++[:, i0] - delta exp(-d/mu0)) wct02 att / w_j
    and j0- = r-+[:, i0] wct02 att / w_j, which ties elemental_pair's two uses together (the `mu_i == mu_j` branch with
    diag == true in the matrix, with diag == false in the source)."""
    from tests.test_gpu_parity import _added_to_host, _product_props, _product_quad, _scene
    pol, qp0, props, rng = _scene(pol_name, l_trunc, 40.0, [30.0], FT)
    qp = _quad_with_sun_at(qp0, _sun_positions(qp0)[where])
    n = pol.n
    S, N = len(props[0].tau), qp.Nquad * n
    assert N == {("I", 9): 7, ("IQU", 9): 21, ("I", 115): 60}[(pol_name, l_trunc)]
    dq, hpol = _product_quad(vsm, arch, qp, pol, FT)
    conv = vsm.Architectures.array_type(arch)
    tau_sum = rng.random(S).astype(FT)
    F0 = np.zeros((n, S), dtype=FT)
    F0[0] = 1.0
    tol = 1e-12 if FT == np.float64 else 1e-5
    for m in (0, 1):
        lo = props[m]
        pp = _product_props(vsm, arch, lo, FT)
        for ndoubl in (0, 3):
            dtau = (lo.tau / FT(2 ** ndoubl)).astype(FT)
            oa = O.make_added_layer(FT, N, S)
            O.elemental(pol, tau_sum, dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, m, ndoubl, qp, oa, FT)
            pa = vsm.CoreRT.make_added_layer(FT, arch, (N, N), S)
            vsm.CoreRT.elemental_(hpol, conv(tau_sum), conv(dtau), conv(np.ascontiguousarray(F0.T)), pp, m, ndoubl, dq, pa)
            got = _added_to_host(vsm, pa)
            for k in ["r_mp", "t_pp", "j0_p", "j0_m"] + (["r_pm", "t_mm"] if ndoubl == 0 else []):
                assert np.all(np.isfinite(got[k])), (m, ndoubl, k)
                assert _rel(got[k], getattr(oa, k)) < tol, (m, ndoubl, k, _rel(got[k], getattr(oa, k)))
            if where in ("first", "weighted") and ndoubl == 0:
                i0 = n * qp.imu0
                wj = float(qp.wt_muN[i0]) / (2 if m == 0 else 4)
                c = (0.5 if m == 0 else 0.25) * np.exp(-tau_sum.astype(np.float64) / qp.mu0) / wj
                t_col = got["t_pp"][:, :, i0].astype(np.float64).copy()
                t_col[:, i0] -= np.exp(-dtau.astype(np.float64) / qp.mu0)
                tie = 1e-12 if FT == np.float64 else 2e-5
                assert _rel(got["j0_p"], t_col * c[:, None]) < tie, (m, _rel(got["j0_p"], t_col * c[:, None]))
                assert _rel(got["j0_m"], got["r_mp"][:, :, i0] * c[:, None]) < tie, m
        # fused elemental + doubling (the layer kernels' own pre-pass of the source vectors)
        dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT)
        oa = O.make_added_layer(FT, N, S)
        O.elemental(pol, tau_sum, dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, m, nd, qp, oa, FT)
        O.doubling(pol, np.exp(-dtau / FT(qp.mu0)).astype(FT), nd, oa, FT)
        pa = vsm.CoreRT.make_added_layer(FT, arch, (N, N), S)
        vsm.CoreRT.elemental_doubling_(hpol, conv(tau_sum), conv(dtau), conv(np.ascontiguousarray(F0.T)), pp, m, nd, dq, pa)
        got = _added_to_host(vsm, pa)
        # FP64: test_layer_forward_entry_point's bound for these kernels, max(1e-10, 50 2^nd eps): the squarings amplify one ulp
        # by 2^nd, and the 58 weighted nodes of ("I", 115) take nd = 19, where 2^19 eps = 1.2e-10 by itself (measured there:
        # 1.06e-10 in t++, the same at every position of the sun).  At nd <= 16, which is all test_elemental_doubling_fused_and_oplevel
        # reaches, this is that test's flat 1e-10.
        ftol = max(1e-10, 50 * 2.0 ** nd * np.finfo(np.float64).eps) if FT == np.float64 else 5e-4
        for k in ("r_mp", "t_pp", "j0_p", "j0_m"):
            assert _rel(got[k], getattr(oa, k)) < ftol, ("fused", m, nd, k, _rel(got[k], getattr(oa, k)))


@pytest.mark.parametrize("FT,pol_name,l_trunc,vza", [(np.float64, "IQU", 9, [30.0]), (np.float64, "IQU", 35, [30.0, 0.0]),
                                                     (np.float64, "IQUV", 41, [30.0, 0.0]), (np.float32, "IQU", 35, [30.0, 0.0]),
                                                     (np.float32, "IQU", 9, [30.0])])
@pytest.mark.parametrize("where", ["first", "weighted", "tail_first", "last"])
def test_layer_forward_with_the_sun_at_any_node(vsm, arch, FT, pol_name, l_trunc, vza, where):
    """vsm_layer_forward (elemental -> doubling -> copy | interaction 11 in the layer kernels: fused N = 21, strip N = 63,
    strip128 N = 96, FP32) with i_mu0 at any node, as test_layer_forward_entry_point checks it at the last node."""
    from tests.test_gpu_parity import _comp_to_host, _product_props, _product_quad, _random_layers, _scene, _upload_layers
    pol, qp0, props, rng = _scene(pol_name, l_trunc, 40.0, vza, FT)
    qp = _quad_with_sun_at(qp0, _sun_positions(qp0)[where])
    lo = props[1]
    S, N = len(lo.tau), qp.Nquad * pol.n
    assert N == {("IQU", 9): 21, ("IQU", 35): 63, ("IQUV", 41): 96}[(pol_name, l_trunc)]
    dtau, nd = O.get_dtau_ndoubl(lo.tau, lo.varpi, qp, FT)
    tau_sum = rng.random(S).astype(FT)
    F0 = np.zeros((pol.n, S), dtype=FT)
    F0[0] = 1.0
    dq, hpol = _product_quad(vsm, arch, qp, pol, FT)
    conv = vsm.Architectures.array_type(arch)
    pp = _product_props(vsm, arch, lo, FT)
    for toa in (True, False):
        oa = O.make_added_layer(FT, N, S)
        O.elemental(pol, tau_sum, dtau, F0, lo.varpi, lo.Zpp, lo.Zmp, 1, nd, qp, oa, FT)
        O.doubling(pol, np.exp(-dtau / FT(qp.mu0)).astype(FT), nd, oa, FT)
        comp, _ = _random_layers(rng, N, S, FT, None)
        pc, _pa = _upload_layers(vsm, arch, comp, oa, FT)
        if toa:
            O.copy_added_to_composite(comp, oa)
        else:
            O.interaction("11", comp, oa, FT)
        scratch = vsm.CoreRT.make_added_layer(FT, arch, (N, N), S)
        vsm.CoreRT.layer_forward_(conv(tau_sum), conv(dtau), conv(np.ascontiguousarray(F0.T)), pp, 1, nd, dq, toa, pc, scratch)
        got = _comp_to_host(vsm, pc)
        tol = max(1e-10, 50 * 2.0 ** nd * np.finfo(FT).eps) if FT == np.float64 else 5e-4
        for k, v in got.items():
            assert np.all(np.isfinite(v)), (toa, k)
            assert _rel(v, getattr(comp, k)) < tol, (toa, k, _rel(v, getattr(comp, k)))


@pytest.mark.parametrize("FT,tol", [(np.float64, 1e-12), (np.float32, 1e-5)])
@pytest.mark.parametrize("pol_name", ["I", "IQU"])
@pytest.mark.parametrize("where", ["first", "weighted", "tail_first", "last"])
def test_forward_surface_builders_with_the_sun_at_any_node(vsm, arch, pol_name, where, FT, tol):
    """vsm_lambertian_surface, vsm_lambertian_surface_spectral and vsm_brdf_surface (rpv) with i_mu0 at any node, m = 0 and 1:
    which rows of j0+ hold the beam and which column of the reflectance makes j0- (lambertian_surface.jl:71-76, :135-137,
    rpv_surface.jl:80-87), against the oracle's builders."""
    H, CR = vsm.host_model, vsm.CoreRT
    pol = O.polarization(pol_name)
    qp0 = O.rt_set_streams_gausslegquad(9, 40.0, [30.0, 10.0], pol, FT)
    qp = _quad_with_sun_at(qp0, _sun_positions(qp0)[where])
    hq = H.QuadPoints(qp.mu0, qp.imu0, qp.qp_mu, qp.wt_mu, qp.qp_muN, qp.wt_muN, qp.Nquad, qp.Nstreams)
    dq = CR.device_quad(hq, H.polarization_type(pol_name), arch, FT)
    conv = vsm.Architectures.array_type(arch)
    N, S = qp.Nquad * pol.n, 5
    tau_sum = np.random.default_rng(2).uniform(0.05, 2.0, S).astype(FT)
    albedo = np.linspace(0.1, 0.5, S)
    i0 = pol.n * qp.imu0
    f = CR.from_device_matrix
    h = vsm.Architectures.to_host
    for m in (0, 1):
        # LambertianSurfaceScalar
        a = CR.AddedLayer(FT, arch, N, S, shared=True)
        CR.create_surface_layer_(H.LambertianSurfaceScalar(0.3), a, m, dq, conv(tau_sum))
        oa = O.make_added_layer(FT, N, S)
        O.create_surface_layer_lambertian(0.3, oa, m, pol, qp, tau_sum, FT)
        for k in ("j0_p", "j0_m"):
            got, want = h(getattr(a, k)), getattr(oa, k)
            assert np.max(np.abs(got - want)) <= tol * max(np.max(np.abs(want)), 1.0), ("scalar", m, k)
        if m == 0:
            assert np.all(h(a.j0_p)[:, i0] > 0) and np.count_nonzero(h(a.j0_p)) == S      # the beam: the I row of the solar node alone
        assert _rel(f(a.r_mp)[0], oa.r_mp[0]) < tol or m == 1
        # LambertianSurfaceLegendre / Spline: per-point blocks, no beam
        a = CR.AddedLayer(FT, arch, N, S)
        CR.create_surface_layer_(H.LambertianSurfaceSpline(albedo), a, m, dq, conv(tau_sum), rho=conv(albedo.astype(FT)))
        oa = O.make_added_layer(FT, N, S)
        O.create_surface_layer_lambertian_spectral(albedo, oa, m, pol, qp, tau_sum, FT)
        assert np.all(h(a.j0_p) == 0)
        assert np.max(np.abs(h(a.j0_m) - oa.j0_m)) <= tol * max(np.max(np.abs(oa.j0_m)), 1.0), ("spectral", m)
        # rpv through the generic BRDF builder: the beam at every moment, j0- from column i_mu0 of the reflectance
        surf = H.rpvSurfaceScalar(0.12, 0.08, 0.75, -0.25)
        a = CR.AddedLayer(FT, arch, N, S, shared=True)
        CR.create_surface_layer_(surf, a, m, dq, conv(tau_sum), arch=arch, FT=FT)
        oa = O.make_added_layer(FT, N, S)
        rho = OB.reflectance(OB.RPVSurface(0.12, 0.08, 0.75, -0.25), pol.n, qp.qp_mu.astype(np.float64), m)
        CM.create_surface_layer_brdf(rho, oa, m, pol, qp, tau_sum, FT)
        for k in ("j0_p", "j0_m"):
            got, want = h(getattr(a, k)), getattr(oa, k)
            # (1e-8: test_brdf_surface_layer_forward_and_lin's bound for the source vectors of a BRDF block; FP32 as the others)
            assert _rel(got, want) <= (1e-8 if FT == np.float64 else tol), ("rpv", m, k, _rel(got, want))
        assert np.all(h(a.j0_p)[:, i0] > 0)


@pytest.mark.parametrize("pol_name,l_trunc", [("I", 7), ("IQU", 7), ("I", 113)])             # N = 7, 21, 60
@pytest.mark.parametrize("where", ["first", "weighted", "tail_first", "last"])
def test_elemental_lin_kernel_with_the_sun_at_any_node(vsm, arch, pol_name, l_trunc, where):
    """vsm_elemental_lin (k_elemental_sfi_lin's solar-row branch, vsm_lin.hip) with i_mu0 at any node, against OL.elemental_lin
    at test_elemental_and_doubling_lin's 1e-11 / 1e-12."""
    from tests.test_gpu_lin import _al_host, _dev, _layer
    FT = np.float64
    pol, qp0, N, tau, varpi, Zpp, Zmp, lin, rng = _layer(pol_name, l_trunc, FT, P=2)
    qp = _quad_with_sun_at(qp0, _sun_positions(qp0)[where])
    S, P_layer = len(tau), lin.tau_dot.shape[1]
    P = P_layer + 1
    assert N == {("I", 7): 7, ("IQU", 7): 21, ("I", 113): 60}[(pol_name, l_trunc)]
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    conv = vsm.Architectures.array_type(arch)
    dq, hpol = _dev(vsm, arch, FT, qp, pol)
    tau_sum = rng.random(S)
    tsd = rng.standard_normal((S, P_layer)) * 0.1
    F0 = np.zeros((pol.n, S))
    F0[0] = 1.0
    if pol.n > 1:
        F0[1] = 0.2
    props = CR.expandOpticalProperties(vsm.host_model.CoreScatteringOpticalProperties(tau, varpi, Zpp, Zmp), arch, FT)
    zpd, zs_, zp_ = CL.to_device_zdot(lin.Zpp_dot, arch, FT)
    zmd, _, _ = CL.to_device_zdot(lin.Zmp_dot, arch, FT)
    for ndoubl in (0, 3):
        dtau = (tau / 2 ** ndoubl).astype(FT)
        dtd = lin.tau_dot / 2 ** ndoubl
        oa, oal = O.make_added_layer(FT, N, S), OL.make_added_layer_lin(FT, P, N, S)
        OL.elemental_lin(pol, tau_sum, tsd, dtau, F0, varpi, Zpp, Zmp, lin, 0, ndoubl, qp, oa, oal, FT)
        pa, pal = CR.AddedLayer(FT, arch, N, S), CL.AddedLayerLin(FT, arch, P, N, S)
        CL.elemental_lin_(hpol, conv(tau_sum), CL.to_device_sp(tsd, arch, FT), conv(dtau), CL.to_device_sp(dtd, arch, FT),
                          conv(np.ascontiguousarray(F0.T)), props, CL.to_device_sp(lin.varpi_dot, arch, FT), zpd, zmd,
                          (zs_, zp_), P_layer, 0, ndoubl, dq, pa, pal)
        got = _al_host(vsm, pal)
        for k in ["ap_r_mp", "ap_t_pp", "ap_J0_p", "ap_J0_m"] + (["ap_r_pm", "ap_t_mm"] if ndoubl == 0 else []):
            assert _rel(got[k], getattr(oal, k)) < 1e-11, (ndoubl, k, _rel(got[k], getattr(oal, k)))
        assert _rel(CR.from_device_matrix(pa.r_mp), oa.r_mp) < 1e-12 and _rel(CR.from_device_matrix(pa.t_pp), oa.t_pp) < 1e-12
        assert _rel(vsm.Architectures.to_host(pa.j0_p), oa.j0_p) < 1e-12 and _rel(vsm.Architectures.to_host(pa.j0_m), oa.j0_m) < 1e-12


def _move_sun(om, pm, where):
    """Both models with the solar node moved by hand (imu0 and mu0 are plain fields of the two QuadPoints)."""
    pos = _sun_positions(om.quad_points)[where]
    om.quad_points = _quad_with_sun_at(om.quad_points, pos)
    pm.quad_points = dataclasses.replace(pm.quad_points, imu0=int(pos), mu0=float(pm.quad_points.qp_mu[pos]))
    return om, pm


WHERE = ["first", "weighted", "tail_first", "last"]


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol,l_trunc", [("I", 7), ("IQU", 7), ("I", 113)])                  # N = 7, 21, 60
@pytest.mark.parametrize("where", WHERE)
def test_ss_column_kernels_with_the_sun_at_any_node(vsm, arch, pol, l_trunc, where, FT):
    """vsm_ss_column and vsm_ss_column_rrs through core_rt_ss.ss_column_ / ss_column_rrs_ on the oracle's inputs, with i_mu0 at
    any node (test_column_kernels_accumulate_over_moments has it in the tail): R, T, ieR, ieT and the m = 0 sources at all
    streams, at test_gpu_ss.TOL (1e-10 / 5e-4).  These kernels build no matrices, so there is no column to tie the sources to;
    the sources at all streams against the oracle's composite J0-+ are the check of the solar-row branch on a weighted row."""
    from tests.test_gpu_ss import SHIFTS, TOL, W_IE, _kernel_case, _models
    from tests.test_gpu_ss import _rs_pair as ss_rs_pair
    om, pm = _move_sun(*_models(vsm, arch, pol, l_trunc, 7, 3, FT), where)
    assert om.quad_points.Nquad * om.pol.n == {("I", 7): 7, ("IQU", 7): 21, ("I", 113): 60}[(pol, l_trunc)]
    ors, _ = ss_rs_pair(vsm, SHIFTS, W_IE)
    per_m = []
    ref = SS.rt_run_ss_rrs(om, ors, per_m=per_m)
    got = _kernel_case(vsm, arch, om, pm, FT, rs=ors)
    for name, g, r in zip(("R", "T", "ieR", "ieT"), got[:4], ref[:4]):
        assert np.all(np.isfinite(g)) and np.max(np.abs(r)) > 0, name
        assert _rel(g, r) <= TOL[FT], (name, _rel(g, r))
    assert _rel(got[4], per_m[0]["J0_m"]) <= TOL[FT] and _rel(got[5], per_m[0]["J0_p"]) <= TOL[FT]


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol", ["I", "IQU"])                                                # N = 7, 21 (the helper's scene: l_trunc = 7)
@pytest.mark.parametrize("where", WHERE)
def test_ss_column_lin_kernel_with_the_sun_at_any_node(vsm, arch, pol, where, FT):
    """vsm_ss_column_lin through core_rt_ss.ss_column_lin_ on the oracle's inputs with i_mu0 at any node, at test_gpu_ss_lin.TOL."""
    from tests.test_gpu_ss_lin import TOL, _check_slots, _kernel_case, _scene
    om, ol, pm, _ = _scene(vsm, arch, pol, 5, 0, 2, FT)
    om, pm = _move_sun(om, pm, where)
    assert om.quad_points.Nquad * om.pol.n == {"I": 7, "IQU": 21}[pol]
    _, _, Rdo, Tdo = SSL.rt_run_ss_lin(om, ol)
    Rd, Td = _kernel_case(vsm, arch, om, ol, pm, FT)
    _check_slots(Rd, Rdo, TOL[FT], "Rdot (kernel)")
    _check_slots(Td, Tdo, TOL[FT], "Tdot (kernel)")


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol,l_trunc", [("I", 7), ("IQU", 7), ("I", 113)])                  # N = 7, 21, 60
@pytest.mark.parametrize("where", WHERE)
def test_elemental_inelastic_kernel_with_the_sun_at_any_node(vsm, arch, pol, l_trunc, where, FT):
    """vsm_elemental_inelastic_rrs (k_elemental_sfi_rrs' solar-row branch) with i_mu0 at any node, m = 0 and 1, without and with
    doubling, against OR.elemental_inelastic at test_elemental_inelastic's 1e-12 / 2e-5."""
    from tests.test_gpu_raman import SHIFTS, _check_rs, _device_side, _oracle_added, _setup
    c = _setup(vsm, arch, FT, pol, l_trunc=l_trunc)
    assert c["N"] == {("I", 7): 7, ("IQU", 7): 21, ("I", 113): 60}[(pol, l_trunc)]
    pos = _sun_positions(c["qp"])[where]
    c["qp"] = _quad_with_sun_at(c["qp"], pos)
    c["hqp"] = dataclasses.replace(c["hqp"], imu0=int(pos), mu0=float(c["hqp"].qp_mu[pos]))
    for m, ndmode in ((0, 0), (0, -1), (1, -1)):
        rs, add, ars, dtau, nd, _ = _oracle_added(c, FT, m, ndmode)
        dq, drs, conv = _device_side(vsm, arch, c, FT, rs, m)
        pr = vsm.CoreRTRaman.AddedLayerRS(FT, arch, len(SHIFTS), c["N"], c["S"])
        vsm.CoreRTRaman.elemental_inelastic_(drs, conv(c["tau_sum"]), conv(dtau), conv(np.ascontiguousarray(c["F0"].T)), m, nd, dq, pr)
        mats = ("ier_mp", "iet_pp") + (("ier_pm", "iet_mm") if (nd < 1 or c["pol"].n == 1) else ())
        _check_rs(vsm, pr, ars, 1e-12 if FT == np.float64 else 2e-5, mats, ("ieJ0_p", "ieJ0_m"))


@pytest.mark.parametrize("FT", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol,l_trunc", [("I", 9), ("IQU", 9), ("I", 115)])                  # N = 7, 21, 60 (one view)
@pytest.mark.parametrize("where", WHERE)
def test_native_run_with_the_sun_at_any_node(vsm, arch, monkeypatch, pol, l_trunc, where, FT):
    """vsm_run_layer (the native pre-pass builds the elemental layer and its sources from the run's quad) with i_mu0 set by hand:
    the whole native run of a model whose QuadPoints have the solar node moved, against O.rt_run of the same QuadPoints and against
    the reference-layout run (1e-8 / 1e-10 as test_gpu_native; Float32: the exact reference at this file's ceilings)."""
    from tests.test_gpu_fp32_accuracy import _gate
    kw = G.scene()
    om = O.build_model(pol, l_trunc, 40.0, [30.0], [60.0], FT=FT, **kw)
    pm = vsm.host_model.model_from_arrays(arch, pol, l_trunc, 40.0, [30.0], [60.0], float_type=FT, **kw)
    om, pm = _move_sun(om, pm, where)
    assert om.quad_points.Nquad * om.pol.n == {("I", 9): 7, ("IQU", 9): 21, ("I", 115): 60}[(pol, l_trunc)]
    Rn, Tn, nat = _run(vsm, monkeypatch, pm, True)
    Rl, Tl, _ = _run(vsm, monkeypatch, pm, False)
    assert nat == set(range(om.m_max + 1))
    if FT == np.float64:
        Ro, To = O.rt_run(om)
        assert _rel(Rn, Ro) < 1e-8 and _rel(Tn, To) < 1e-8, (_rel(Rn, Ro), _rel(Tn, To))
        assert _rel(Rn, Rl) < 1e-10 and _rel(Tn, Tl) < 1e-10
    else:
        (R32, T32), (Rx, Tx) = O.rt_run(om), O.rt_run(O.exact_model(om))
        c = FP32_CEIL[(pol, {115: 117}.get(l_trunc, l_trunc))]
        for R, T, name in ((Rn, Tn, "native"), (Rl, Tl, "layout")):
            _gate("geo sun %s %s/%d %s" % (where, pol, l_trunc, name), dict(R=(R, R32, Rx), T=(T, T32, Tx)), dict(R=c, T=c))


@pytest.mark.parametrize("pol,l_trunc", [("I", 7), ("IQU", 7), ("I", 113)])                  # N = 7, 21, 60
@pytest.mark.parametrize("where", WHERE)
def test_lin_mix_and_fold_kernels_with_the_sun_at_any_node(vsm, arch, pol, l_trunc, where):
    """vsm_elemental_lin_mix (an aerosol mixed per point inside the linearized elemental kernel) and vsm_elemental_lin_fold (the
    moments folded into the spectral axis) with i_mu0 set by hand: SceneLin over the aerosol scene of test_gpu_lin (mix) and over a
    gas scene (sequential and folded) with the solar node moved, against OL.rt_run_lin of the same QuadPoints (1e-9 / 1e-8, the folded walk 1e-13 from the
    sequential one: test_gpu_lin)."""
    from tests.test_gpu_lin import _host_aerosol_scene
    om, ol, pm, pl = _host_aerosol_scene(vsm, arch, pol, l_trunc)
    om, pm = _move_sun(om, pm, where)
    assert om.quad_points.Nquad * om.pol.n == {("I", 7): 7, ("IQU", 7): 21, ("I", 113): 60}[(pol, l_trunc)]
    kw, bases = G.gas_scene(S=3)                       # (the folded walk takes no aerosol slots: a gas scene of the same geometry)
    og = O.build_model(pol, l_trunc, 35.0, [20.0, 50.0], [0.0, 120.0], **kw)
    pg = vsm.host_model.model_from_arrays(arch, pol, l_trunc, 35.0, [20.0, 50.0], [0.0, 120.0], **kw)
    og, pg = _move_sun(og, pg, where)
    calls = []
    real = vsm._lib.call
    vsm._lib.call = lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1]
    try:
        scene = vsm.CoreRTLin.SceneLin(pm, pl, 1, 1, 1)
        scene.run(lanes=1, fold=False)
        torch.cuda.synchronize()
        mix = scene.results_host()
        n_mix = len(calls)
        sg = vsm.CoreRTLin.SceneLin(pg, vsm.host_model.LinModel(bases), 0, 2, 1)
        sg.run(lanes=1, fold=False)
        torch.cuda.synchronize()
        seq = sg.results_host()
        sg.run(lanes=2, fold=True)
        torch.cuda.synchronize()
        fold = sg.results_host()
    finally:
        vsm._lib.call = real
    assert "vsm_elemental_lin_mix" in calls[:n_mix] and "vsm_elemental_lin_fold" in calls[n_mix:], sorted(set(calls))
    for out, ref in ((mix, OL.rt_run_lin(om, ol)), (seq, OL.rt_run_lin(og, OL.LinModel(bases))), (fold, OL.rt_run_lin(og, OL.LinModel(bases)))):
        assert _rel(out[0], ref[0]) < 1e-9 and _rel(out[1], ref[1]) < 1e-9
        for p in range(ref[2].shape[-1]):
            assert _rel(out[2][..., p], ref[2][..., p]) < 1e-8 and _rel(out[3][..., p], ref[3][..., p]) < 1e-8, p
    for a, b in zip(fold, seq):
        assert _rel(a, b) < 1e-13


@pytest.mark.parametrize("FT,tol", [(np.float64, 1e-14), (np.float32, 2e-6)], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pol_name", ["I", "IQU"])
@pytest.mark.parametrize("where", WHERE)
def test_lin_surface_builders_with_the_sun_at_any_node(vsm, arch, pol_name, where, FT, tol):
    """vsm_lambertian_surface_lin (k_lambertian_lin_src), vsm_lambertian_surface_spectral_lin (vectors) and
    vsm_brdf_surface_lin_multi (k_brdf_src_lin, which reads column i_mu0 of rho and drho) with i_mu0 at any node, m = 0 and 1:
    j0+ = 0 and ap_J0+ = 0 wherever the sun is (lambertian_surface_lin.jl:107, coxmunk_surface_lin.jl:72), j0- and its
    derivatives from the solar column, against the oracles' builders at the builder bounds of test_gpu_brdf_lin /
    test_gpu_spectral_albedo_lin (1e-14 / 2e-6)."""
    import ctypes as C

    import brdf_lin_oracle as BL
    import spectral_albedo_lin_oracle as SA
    H, CR, CL = vsm.host_model, vsm.CoreRT, vsm.CoreRTLin
    pol = O.polarization(pol_name)
    qp0 = O.rt_set_streams_gausslegquad(9, 40.0, [30.0, 10.0], pol, FT)
    qp = _quad_with_sun_at(qp0, _sun_positions(qp0)[where])
    hq = H.QuadPoints(qp.mu0, qp.imu0, qp.qp_mu, qp.wt_mu, qp.qp_muN, qp.wt_muN, qp.Nquad, qp.Nstreams)
    dq = CR.device_quad(hq, H.polarization_type(pol_name), arch, FT)
    conv = vsm.Architectures.array_type(arch)
    h = vsm.Architectures.to_host
    dt = torch.float64 if FT == np.float64 else torch.float32
    n, N, S, pl, K = pol.n, qp.Nquad * pol.n, 5, 2, 3
    P = pl + K
    rng = np.random.default_rng(7)
    tau_sum, tsd = rng.uniform(0.05, 2.0, S).astype(FT), rng.standard_normal((S, pl)).astype(FT)
    F0 = rng.uniform(0.2, 1.0, (n, S)).astype(FT)
    albedo, basis = np.linspace(0.1, 0.5, S).astype(FT), rng.uniform(0.2, 1.0, (K, S)).astype(FT)
    d_ts, d_tsd, d_F0 = conv(tau_sum), CL.to_device_sp(tsd, arch, FT), conv(np.ascontiguousarray(F0.T))

    def layers():
        a, al = CR.AddedLayer(FT, arch, N, S, shared=True), CL.AddedLayerLin(FT, arch, P, N, S, shared=True)
        for t in (a.j0_p, a.j0_m, al.ap_J0_p, al.ap_J0_m):
            t.fill_(float("nan"))
        return a, al

    def check(what, a, al, oa, oal, m):
        assert np.all(h(a.j0_p) == 0) and np.all(h(al.ap_J0_p) == 0), (what, m)
        for got, want, name in ((h(a.j0_m), oa.j0_m, "j0-"), (h(al.ap_J0_m), oal.ap_J0_m, "ap_J0-")):
            sc = max(float(np.max(np.abs(want))), 1e-300)
            assert np.max(np.abs(got - want)) <= tol * sc, (what, m, name, np.max(np.abs(got - want)) / sc)
        if m == 0 or what == "brdf":
            assert np.max(np.abs(oa.j0_m)) > 0 and np.max(np.abs(oal.ap_J0_m)) > 0, (what, m)

    for m in (0, 1):
        # k_lambertian_lin_src
        a, al = layers()
        q_, a_, al_ = dq.cstruct(), a.cstruct(), al.cstruct()
        alb = C.c_double(0.3) if FT == np.float64 else C.c_float(0.3)
        vsm._lib.call("vsm_lambertian_surface_lin", dt, C.byref(q_), S, m, alb, P - 1, CR._ptr(d_ts), CR._ptr(d_tsd), pl, CR._ptr(d_F0),
                      C.byref(a_), C.byref(al_), CR._stream_ptr())
        torch.cuda.synchronize()
        oa, oal = O.make_added_layer(FT, N, S), OL.make_added_layer_lin(FT, P, N, S)
        OL.create_surface_layer_lambertian_lin(FT(0.3), oa, oal, P - 1, m, pol, qp, tau_sum, tsd, F0, FT)
        check("lambertian", a, al, oa, oal, m)
        # the spectral builder, vectors only (shared layers)
        a, al = layers()
        CL.lambertian_surface_spectral_lin_(dq, S, m, conv(albedo), conv(np.ascontiguousarray(basis)), pl, d_ts, d_tsd, pl, d_F0, a, al,
                                            vectors_only=True)
        torch.cuda.synchronize()
        oa, oal = O.make_added_layer(FT, N, S), OL.make_added_layer_lin(FT, P, N, S)
        SA.create_surface_layer_spectral_lin(albedo, basis, oa, oal, pl, m, pol, qp, tau_sum, tsd, F0, FT)
        check("spectral", a, al, oa, oal, m)
        # k_brdf_src_lin: column i_mu0 of a random rho and of its K derivative blocks
        rho, drho = rng.uniform(0.0, 1.0, (N, N)).astype(FT), rng.standard_normal((K, N, N)).astype(FT)
        a, al = layers()
        CL.brdf_surface_lin_multi_(dq, S, m, conv(np.ascontiguousarray(rho.T)), conv(np.ascontiguousarray(drho.transpose(0, 2, 1))), pl,
                                   d_ts, d_tsd, pl, d_F0, a, al)
        torch.cuda.synchronize()
        oa, oal = O.make_added_layer(FT, N, S), OL.make_added_layer_lin(FT, P, N, S)
        BL.create_surface_layer_brdf_lin(rho, drho, oa, oal, pl, m, pol, qp, tau_sum, tsd, F0, FT)
        check("brdf", a, al, oa, oal, m)
        i0 = n * qp.imu0
        f = 2.0 if m == 0 else 1.0
        col = np.exp(-tau_sum.astype(np.float64) / qp.mu0)[:, None] * qp.mu0 * f * (F0.astype(np.float64).T @ rho[:, i0:i0 + n].astype(np.float64).T)
        assert np.max(np.abs(h(a.j0_m) - col)) <= 10 * max(tol, 1e-13) * np.max(np.abs(col))     # j0- IS column i_mu0 of rho


# ---------------------------------------------------------------------------------------------------------------------
# (f) `near`: two nodes about 1.1e-6 apart in mu
# ---------------------------------------------------------------------------------------------------------------------
def _near_row_errors(FT_dev_j0p, qp32, dtau, varpi, ZF, tau_sum, wct02):
    """(device error, plain-numpy-float32 error) of j0+ at the row next to the solar row, both against the double-precision
    value of the same formula on the SAME single-precision inputs (elemental.jl:348-392: wct02 varpi ZF mu0 / (mu_i - mu0)
    expdiff_neg(dtau / mu_i, dtau / mu0) exp(-tau_sum / mu0)), relative to that value."""
    f32, f64 = np.float32, np.float64

    def formula(T):
        mi, m0 = T(qp32["mu_i"]), T(qp32["mu0"])
        d, w, zf, ts = dtau.astype(T), varpi.astype(T), ZF.astype(T), tau_sum.astype(T)
        return T(wct02) * w * zf * (m0 / (mi - m0)) * O.expdiff_neg(d / mi, d / m0) * np.exp(-ts / m0)

    exact, plain = formula(f64), formula(f32)
    return (np.max(np.abs(FT_dev_j0p.astype(f64) - exact) / np.abs(exact)),
            np.max(np.abs(plain.astype(f64) - exact) / np.abs(exact)))


def test_near_nodes_fp32(vsm, arch, monkeypatch):
    """FP32, two nodes ~1.1e-6 apart in mu (40.0001 and 40 degrees): d/mu_i - d/mu_j loses most of its digits, in the reference's
    FP32 arithmetic as on the device, so no fixed bound exists.  Measured instead: the device's error of j0+ at the row next to
    the solar row (vsm_elemental_f32, the kernel every FP32 path shares) and the error of a plain numpy float32 evaluation of the
    reference's own expdiff_neg formula, both against the double evaluation on the same single-precision inputs.  The device may
    be at most 4 times worse (same formula; the slack covers summation order and v_rcp_f32).  Measured on MI355X: see
    DESIGN.md, the FP32 accuracy section.  The run itself must stay finite and meet the FP32 ceiling away from that row; in FP64
    the case meets the ordinary 1e-8 (test_forward_run_every_kernel_family[near-*])."""
    from tests.test_gpu_parity import _added_to_host, _product_props, _product_quad
    FT = np.float32
    pol = O.polarization("I")
    sza, vza, _ = G.CASES["near"]
    qp = O.rt_set_streams_gausslegquad(9, sza, vza, pol, FT)
    G.check_streams("near", qp, 9)
    row = G.view_rows("near", qp)[0]
    assert row != qp.imu0 and 0.5e-6 < abs(float(qp.qp_mu[row]) - float(qp.mu0)) < 2e-6
    rng = np.random.default_rng(3)
    S, N = 64, qp.Nquad
    tau = (10.0 ** rng.uniform(-3, 0.5, S)).astype(FT)
    varpi = rng.uniform(0.3, 1.0, S).astype(FT)
    Zpp, Zmp = O.compute_Z_moments(pol, qp.qp_mu.astype(np.float64), O.get_greek_rayleigh(0.03), 0)
    lo = O.expand_optical_properties(O.CoreScatteringOpticalProperties(tau, varpi, Zpp, Zmp), FT)
    tau_sum = rng.random(S).astype(FT)
    F0 = np.ones((1, S), dtype=FT)
    dq, hpol = _product_quad(vsm, arch, qp, pol, FT)
    conv = vsm.Architectures.array_type(arch)
    worst = (0.0, 0.0)
    for ndoubl in (0, 4, 8):
        dtau = (tau / FT(2 ** ndoubl)).astype(FT)
        pa = vsm.CoreRT.make_added_layer(FT, arch, (N, N), S)
        vsm.CoreRT.elemental_(hpol, conv(tau_sum), conv(dtau), conv(np.ascontiguousarray(F0.T)), _product_props(vsm, arch, lo, FT),
                              0, ndoubl, dq, pa)
        j0p = _added_to_host(vsm, pa)["j0_p"]
        assert np.all(np.isfinite(j0p))
        ZF = lo.Zpp[:, row, qp.imu0]
        e_dev, e_np = _near_row_errors(j0p[:, row], dict(mu_i=qp.qp_mu[row], mu0=FT(qp.mu0)), dtau, lo.varpi, ZF, tau_sum, 0.5)
        print("GEO near FP32 ndoubl=%d: device %.3e, numpy float32 %.3e (relative error of j0+ at the row next to the sun)"
              % (ndoubl, e_dev, e_np))
        assert e_dev <= 4 * e_np, (ndoubl, e_dev, e_np)
        worst = (max(worst[0], e_dev), max(worst[1], e_np))
    print("GEO near FP32 worst: device %.3e, numpy float32 %.3e" % worst)
    # the whole FP32 run at `near`: finite everywhere, the view away from the pair within the FP32 ceiling of the exact reference
    kw = G.scene()
    pm32 = _host_model(vsm, arch, "near", "IQU", 21, kw, FT=np.float32)
    om32 = G.oracle_model("near", "IQU", 21, kw, FT=np.float32)
    Rx, Tx = O.rt_run(O.exact_model(om32))
    for native in (True, False):
        R, T, _ = _run(vsm, monkeypatch, pm32, native)
        assert np.all(np.isfinite(R)) and np.all(np.isfinite(T))
        print("GEO near FP32 run native=%d: R %.2e, T[near view] %.2e, T[30 deg] %.2e"
              % (native, _rel(R, Rx), _rel(T[0], Tx[0]), _rel(T[1], Tx[1])))
        assert _rel(R, Rx) < FP32_CEIL[("IQU", 21)] and _rel(T[1], Tx[1]) < FP32_CEIL[("IQU", 21)]
