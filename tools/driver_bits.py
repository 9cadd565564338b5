"""Every driver entry point on a fixed list of small scenes, array by array: the check that a change to the Python drivers
(core_rt*.py) that only re-sequences the same launches changes no bit of any result.

  python tools/driver_bits.py --dump DIR [--tree TREE]    every scene in ONE fresh child process (this process never opens the
                                                          device); every returned array as DIR/<scene>.<k>.npy.  --tree: run the
                                                          package, the oracle and the tests' builders of another checkout (its
                                                          library built), e.g. a copy of the parent commit
                                                          --only NAME[,NAME]: those scenes alone
  python tools/driver_bits.py --compare DIR_A DIR_B       exit 1 on any array that is missing on one side or differs (shape, dtype,
                                                          any element; NaNs must sit in the same places)

The models come from the tests' own builders (tests/ on sys.path, as the test files have it), at the tests' smallest shapes."""
import argparse
import dataclasses
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--dump", metavar="DIR")
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--only", default="", help="comma-separated scene names (default: all)")
ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()

if a.compare:
    names = [sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "*.npy"))) for d in a.compare]
    bad = sorted(set(names[0]) ^ set(names[1]))
    for f in sorted(set(names[0]) & set(names[1])):
        x, y = (np.load(os.path.join(d, f)) for d in a.compare)
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=True):
            bad.append(f)
    print("%d arrays compared, %d differ or are missing: %s" % (len(set(names[0]) | set(names[1])), len(bad), " ".join(bad)))
    sys.exit(1 if bad or not names[0] else 0)

if not a.dump:
    ap.error("--dump DIR or --compare DIR_A DIR_B")
if not a.child:
    os.makedirs(a.dump, exist_ok=True)
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--dump", os.path.abspath(a.dump), "--tree",
                             os.path.abspath(a.tree), "--only", a.only], cwd=a.tree).returncode)

sys.path[:0] = [a.tree, os.path.join(a.tree, "tests")]
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
import brdf_lin_oracle as B  # noqa: E402
import level_cases as LC  # noqa: E402
import test_gpu_brdf_lin as TB  # noqa: E402
import test_gpu_fluxes as TF  # noqa: E402
import test_gpu_fluxes_lin as TFL  # noqa: E402
import test_gpu_lin as TLIN  # noqa: E402
import test_gpu_multisensor as TMS  # noqa: E402
import test_gpu_multisensor_lin as TML  # noqa: E402
import test_gpu_multisensor_raman as TMR  # noqa: E402
import test_gpu_multisensor_thermal as TMT  # noqa: E402
import test_gpu_multisensor_thermal_lin as TMTL  # noqa: E402
import test_gpu_sif as TS  # noqa: E402
import test_gpu_surface_emission as TSE  # noqa: E402
import test_gpu_surface_emission_lin as TSEL  # noqa: E402
import test_gpu_ss as TSS  # noqa: E402
import test_gpu_ss_lin as TSL  # noqa: E402
import test_gpu_ss_raman_lin as TSRL  # noqa: E402

H, CR, CL, RR = vsm.host_model, vsm.CoreRT, vsm.CoreRTLin, vsm.CoreRTRaman
arch = vsm.Architectures.GPU(0)
rng = lambda: np.random.default_rng(7)
SCENES = {}


def scene(f):
    SCENES[f.__name__] = f
    return f


def flatten(x):
    """The arrays of a result, in a fixed order: tuples, lists, dicts, result dataclasses, device tensors; None holds none."""
    if x is None:
        return []
    if torch.is_tensor(x):
        return [x.detach().cpu().numpy()]
    if dataclasses.is_dataclass(x):
        x = [getattr(x, f.name) for f in dataclasses.fields(x)]
    if isinstance(x, dict):
        x = [x[k] for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [y for v in x for y in flatten(v)]
    return [np.asarray(x)]


class switch:
    """A module switch of CoreRT for the length of a scene."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = getattr(CR, self.name)
        setattr(CR, self.name, self.value)

    def __exit__(self, *exc):
        setattr(CR, self.name, self.old)


# ---- forward rt_run ----------------------------------------------------------------------------------------------------------------
def small(pol="IQU", lt=9, S=3, L=4, **kw):
    return TMS._pair(vsm, arch, pol, lt, S, L, rng(), **kw)[0]


N128 = dict(pol="IQUV", lt=57, S=2, L=3, vza=(30.0, 5.0), vaz=(0.0, 60.0))


@scene
def fwd_native():
    return CR.rt_run(small(), full_output=True)


@scene
def fwd_n128_grouped():
    return CR.rt_run(small(m_max=1, **N128)), CR.rt_run(small(m_max=2, **N128))


@scene
def fwd_native_off():
    with switch("NATIVE_RUN", False):
        return CR.rt_run(small(aerosols=True))


@scene
def fwd_reference_order():
    with switch("REFERENCE_ORDER", True):
        return CR.rt_run(small()), CR.rt_run_streams(small())


@scene
def fwd_streams():
    return CR.rt_run_streams(small()), CR.rt_run_streams(small(aerosols=True))


@scene
def fwd_trace():
    tr = []
    return CR.rt_run(small(), trace=tr), len(tr)


def noscat_model(rayl, sources=None, pol="IQUV", lt=9):
    S = 3
    tau_abs = np.tile(np.array([0.3, 0.5, 0.2, 0.4]), (S, 1)) * (1 + 0.5 * np.arange(S))[:, None]
    return H.model_from_arrays(arch, pol, lt, 30.0, [0.0, 35.0], [0.0, 60.0], tau_rayl=np.tile(np.array(rayl), (S, 1)),
                               tau_abs=tau_abs, depol=0.03, albedo=0.1, m_max=2, sources=sources)


@scene
def fwd_noscat_layer():
    return CR.rt_run(noscat_model([0.05, 0.0, 0.1, 0.2])), CR.rt_run_streams(noscat_model([0.0, 0.05, 0.1, 0.2]))


# ---- thermal (IQUV, l_trunc 19: N = 52, the fused slot kernel's range) ---------------------------------------------------------------
def thermal_sources(L, S, reset=False, n=None):
    th = H.ThermalEmission(B_layer=TMTL._B(L, S), reset_slot_in_nonscattering_layers=reset,
                           **({} if n is None else dict(B_layer_dot=TMTL._Bdot(L, S, n))))
    return (H.SolarBeam(), th)


@scene
def thermal_fused():
    return CR.rt_run(noscat_model([0.02, 0.05, 0.1, 0.2], thermal_sources(4, 3), lt=19), full_output=True)


@scene
def thermal_operator_level():
    with switch("THERMAL_FUSION", False):
        return CR.rt_run(noscat_model([0.02, 0.05, 0.1, 0.2], thermal_sources(4, 3), lt=19))


@scene
def thermal_carried_into_m1():
    pm = noscat_model([0.0, 0.05, 0.1, 0.2], thermal_sources(4, 3), lt=19)
    return CR.rt_run(pm), CR.rt_run_streams(pm)


@scene
def thermal_reset_noscat():
    return CR.rt_run(noscat_model([0.05, 0.0, 0.1, 0.2], thermal_sources(4, 3, reset=True), lt=19))


@scene
def sif_and_run_graph():
    out = [CR.rt_run(TS._pm(vsm, arch, "IQU", 9, TS._src(H)), full_output=True)]
    sc = CR.prepare_scene(TS._pm(vsm, arch, "IQU", 33, TS._src(H)))
    for _ in range(2):
        sc.run_graph()
        torch.cuda.synchronize()
        out.append(sc.results_host())
    sc = CR.prepare_scene(small())
    sc.run_graph()
    torch.cuda.synchronize()
    return out, sc.results_host()


# ---- rt_run_multisensor ------------------------------------------------------------------------------------------------------------
MS_CASES = [("I", 9, 5, 6, [3, 0, 6, 1], dict(m_max=3, vza=(30.0, 5.0), vaz=(0.0, 60.0))),
            ("IQU", 9, 3, 6, [5, 2, 5, 0, 2, 6, 1], dict(m_max=3))]


@scene
def ms_forward():
    out = []
    for pol, lt, S, L, levels, kw in MS_CASES:
        pm = small(pol, lt, S, L, **kw)
        out.append(CR.rt_run_multisensor(pm, levels))
        pm.sources = thermal_sources(L, S)
        out.append(CR.rt_run_multisensor(pm, levels, thermal=True))
        out.append(CR.rt_run_multisensor(pm, levels, thermal=True, streams=True))
    pm = small("IQU", 9, 3, 6, aerosols=True)
    pm.sources = (H.SolarBeam(), H.SurfaceSIF(np.linspace(0.1, 0.3, 3)))
    out.append(CR.rt_run_multisensor(pm, [2, 0, 6], streams=True))
    with switch("REFERENCE_ORDER", True):
        out.append(CR.rt_run_multisensor(small("IQU", 9, 3, 6), [5, 0, 6]))
    return out


@scene
def ms_forward_n128():
    pm = small(m_max=1, **N128)
    out = [CR.rt_run_multisensor(pm, [1, 2, 3, 0])]
    pm.sources = thermal_sources(3, 2)
    return out, CR.rt_run_multisensor(pm, [1, 2, 3, 0], thermal=True)


@scene
def ms_surface_emission():
    """SurfaceEmission in the forward run with level vectors, and in the linearized run with its two skin slots."""
    S = 5
    out = []
    for se_kw in ({}, dict(emissivity=0.8)):          # Kirchhoff, explicit
        pm, _, _ = TSE.scene(vsm, arch, "lambertian", "IQU", S, sources=TSE._sources(H, "all", S, **se_kw))
        out.append(CR.rt_run_multisensor(pm, TSE.LEVELS, thermal=True, streams=True))
    pm, _, _ = TSE.scene(vsm, arch, "lambertian", "IQU", S, window=True)
    pm.sources = TSEL._sources(H, "all", S)
    return out, CL.rt_run_multisensor(pm, H.LinModel(list(TSEL._gases(S))), 0, 2, 1, TSE.LEVELS, streams=True)


# ---- rt_run_fluxes -------------------------------------------------------------------------------------------------------------------
def emitting_sources(L, S, **se_kw):
    return thermal_sources(L, S) + (H.SurfaceEmission(B_surface=0.9 + 0.03 * np.arange(S), **se_kw),)


@scene
def fluxes():
    out = []
    for pol, lt in (("IQU", 35), ("IQUV", 50)):          # native runs / the reference-layout walk
        for levels in (None, [4, 0, 2, 4]):
            pm = small(pol, lt, 4, 6, m_max=1)
            out.append(CR.rt_run_fluxes(pm, levels))
            for se_kw in ({}, dict(emissivity=0.8)):      # Kirchhoff, explicit
                pm.sources = emitting_sources(6, 4, **se_kw)
                out.append(CR.rt_run_fluxes(pm, levels, thermal=True))
    pm = small("IQU", 35, 4, 6)
    pm.sources = (H.SolarBeam(), H.SurfaceSIF(np.linspace(0.1, 0.3, 4)))
    out.append(CR.rt_run_fluxes(pm, [4, 0, 2, 4]))
    pm.sources = emitting_sources(6, 4) + (H.SurfaceSIF(np.linspace(0.1, 0.3, 4)),)
    out.append(CR.rt_run_fluxes(pm, None, thermal=True, max_points=3))
    with switch("REFERENCE_ORDER", True):
        out.append(CR.rt_run_fluxes(small("IQU", 35, 4, 6), None))
    pm = small(m_max=1, **N128)
    out.append(CR.rt_run_fluxes(pm, None))
    pm.sources = emitting_sources(3, 2)
    return out, CR.rt_run_fluxes(pm, None, thermal=True)


# ---- the level kernels, called directly (the call helpers of tests/test_gpu_level_pivoting.py) -------------------------------------
def level_kernels_at(N, FT, vza, vaz, many):
    """Every entry point of csrc/vsm_level.hip at one size, S = 3, on level_cases.fixed("pivoting", FT); many: the calls that take
    a viewing-angle table alone (radiance, src, emission response), with the angles given."""
    S, nV, inputs = 3, len(vza), LC.fixed("pivoting", FT)
    out = [outs for _, _, outs in TMS._fused_and_oplevel_calls(vsm, N, FT, vza, vaz, inputs=inputs, S=S, ops=(False,))[2]]
    setup = TMT._kernel_setup(vsm, N, FT, nV, vza_max=88.0)
    lay, vec = setup[6], setup[7]
    for shared in (False, True):
        for n_src in (1, 2, 4):
            scales = tuple(1.0 if k % 2 == 0 else 1e3 for k in range(n_src))
            A, tops, B, bots = TMT._src_inputs(N, S, np.random.default_rng(N), shared, inputs=inputs, scales=scales, FT=FT)
            out.append(TMT._level_src_call(vsm, setup, S, N, nV, lay(A), [vec(x) for x in tops], lay(B), [vec(x) for x in bots]))
        for K in (1, 3):
            res = TS._emission_response_case(vsm, N, FT, K, nV, shared, None, inputs=emission_inputs(FT), S_=S, vza_max=88.0,
                                             oplevel=False)
            out.append([xf for _, _, xf, _, _ in res])
    if many:
        return out
    for shared in (False, True):
        pol, dt, dev, host, d = TF._kernel_case(vsm, N, FT, S, shared, np.random.default_rng(N), inputs=inputs)
        for K in (1, 2, 4):
            for top in (True, False):
                o = torch.full((3, 2, S), float("nan"), dtype=dt, device=dev)
                vsm.core_rt_flux.level_flux_(pol, d["A"] if top else None, d["a"][:K] if top else None, d["B"] if top else None,
                                             d["c"][:K], d["q"][:2].contiguous(), host["dir_h"][:2], host["mu0"], d["tau"], d["F0"], o)
                out.append(o)
        out.append(level_ie(N, FT, S, shared, inputs))
        # FP64 at N = 128 takes 12 slots per chunk: a chunk boundary inside the parameter slots, and inside the source-only ones
        two_chunks = N == 128 and FT == np.float64
        P, P_top = (13, 12) if two_chunks else (3, 2)
        out.append(TML._kernel_case(vsm, N, P, P_top, shared, S=S, FT=FT, inputs=inputs)[0])
        P, P_top, P_src = (5, 4, 9) if two_chunks else (3, 2, 2)
        out.append(TMTL._kernel_case(vsm, N, P, P_top, P_src, shared, S=S, FT=FT, inputs=inputs)[0])
        case = TFL._Case(N, P, P_top, P_src, shared, S, FT, 3 if N % 3 == 0 else 1)
        out += [case.call(vsm, 2, top=True), case.call(vsm, 2, top=False)]
    return out


def emission_inputs(FT):
    """(A, B, T) of the response call: the family's operators and test_gpu_sif's transmission block, rounded to FT."""
    def gen(N, S, rng, shared):
        A, _, B, _ = LC.fixed("pivoting", FT)(N, S, None, shared)
        T = (np.random.default_rng(N).random((S, N, N)) * (1.0 / N) + 0.5 * np.eye(N)[None]).astype(FT).astype(np.float64)
        return A, B, T
    return gen


def level_ie(N, FT, S, shared, inputs):
    """vsm_level_radiance_ie_* with 7 lines, as test_gpu_multisensor_raman._level_ie_vs_numpy feeds it: [uwie, dwie, dwie_full,
    uwie_full]."""
    K, nV = 7, 3
    rng = np.random.default_rng(N * 1000 + K)
    ns = 3 if N % 3 == 0 else 1
    A, dwf, B, uwf = inputs(N, S, rng, shared)
    Aie, aie = 0.05 * rng.random((K, S, N, N)) / N, 0.05 * rng.random((K, S, N))
    Bie, cie = 0.05 * rng.random((K, S, N, N)) / N, 0.05 * rng.random((K, S, N))
    row0 = [0, ns * ((N // ns) // 2), N - ns]
    wv = rng.uniform(0.1, 1.0, nV * ns)
    dt = torch.float64 if FT == np.float64 else torch.float32
    outs = [torch.zeros((S, ns, nV), dtype=dt, device="cuda") for _ in range(2)]
    outs += [torch.full((S, N), float("nan"), dtype=dt, device="cuda") for _ in range(2)]
    TMR._level_ie_call(vsm, FT, N, ns, S, K, [int(x) for x in TMR.SHIFTS], A, B, dwf, uwf, Aie, aie, Bie, cie, row0, wv, *outs)
    torch.cuda.synchronize()
    return outs


@scene
def level_kernels():
    vza, vaz = [0.0, 30.0, 88.0], [0.0, 45.0, 120.0]
    out = [level_kernels_at(N, FT, vza, vaz, False) for FT in (np.float64, np.float32) for N in (3, 17, 65, 128)]
    vza, vaz = list(np.linspace(0.0, 88.0, 70)), list(np.linspace(0.0, 345.0, 70))
    return out, [level_kernels_at(65, FT, vza, vaz, True) for FT in (np.float64, np.float32)]


# ---- rt_run_lin --------------------------------------------------------------------------------------------------------------------
def lin_pair(pol="IQU", lt=9, S=3, L=6, **kw):
    return TML._pair(vsm, arch, pol, lt, S, L, rng(), **kw)[:2]


def scene_lin_run(pm, pl, nsurf=1, naer=0, host_optics=False, **kw):
    sc = CL.SceneLin(pm, pl, naer, len(pl.tau_abs_dot), nsurf, host_optics=host_optics)
    sc.run(**kw)
    torch.cuda.synchronize()
    return sc.results_host()


@scene
def lin_walks():
    out = [scene_lin_run(*lin_pair(m_max=3), lanes=1, fold=False), CL.rt_run_lin(*lin_pair(S=2, m_max=3), 0, 1, 1),
           scene_lin_run(*lin_pair(m_max=3), lanes=3, fold=False), scene_lin_run(*lin_pair(S=2, m_max=3), fold=True, lanes=1)]
    sc = CL.SceneLin(*lin_pair(S=2, m_max=3), 0, 1, 1)
    for _ in range(2):
        sc.run(graph=True)
        torch.cuda.synchronize()
        out.append(sc.results_host())
    return out


@scene
def lin_aerosol_slots():
    _, _, pm, pl = TLIN._host_aerosol_scene(vsm, arch, "IQU", 9)
    return CL.rt_run_lin(pm, pl, 1, 1, 1), scene_lin_run(pm, pl, naer=1, host_optics=True), scene_lin_run(pm, pl, naer=1, lanes=1)


@scene
def lin_land_brdf():
    out = []
    for name, surf in B.SURFACES.items():
        pm, hl = TB._host_scene(vsm, arch, "IQU", TB._host_surface(vsm, surf))
        out.append(CL.rt_run_lin(pm, hl, 0, 1, B.n_params(surf)))
    return out


@scene
def lin_thermal_planck():
    out = []
    for pol, S in (("I", 5), ("IQU", 2)):
        pm, pl = lin_pair(pol, 9, S, 6, m_max=3)
        pm.sources = thermal_sources(6, S, n=2)
        out += [CL.rt_run_lin(pm, pl, 0, 1, 1), scene_lin_run(pm, pl, lanes=1, fold=False)]
    _, _, pm, pl = TLIN._host_aerosol_scene(vsm, arch, "IQU", 9)
    S, L = pm.tau_rayl.shape
    pm.sources = thermal_sources(L, S, n=2)
    return out, CL.rt_run_lin(pm, pl, 1, 1, 1), scene_lin_run(pm, pl, naer=1, host_optics=True)


@scene
def lin_sif_slots():
    _, ga, gb = TS._arrays()
    return CL.rt_run_lin(TS._pm(vsm, arch, "IQU", 9, TS._src(H, dot=True)), H.LinModel([ga, gb]), 0, 2, 1)


@scene
def lin_n60_sub0():
    pm, pl = lin_pair("IQU", 35, 300, 8, vza=(30.0,), vaz=(0.0,))
    sc = CL.SceneLin(pm, pl, 0, 1, 1)
    assert sc.sub0 is not None
    sc.run()
    torch.cuda.synchronize()
    return sc.results_host()


# ---- linearized rt_run_multisensor ---------------------------------------------------------------------------------------------------
def ms_lin_case(name):
    def run():
        out = []
        for which in ("solar+thermal", "thermal"):
            pm, pl, _, _, levels = TMTL._case(vsm, arch, name, which)
            out.append(CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels))
        if name == "scalar_n8":
            out.append(CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels, max_points=3))
            pm, pl, _, _, levels = TMTL._case(vsm, arch, name)
            out.append(CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True))
            pm.sources = None
            out.append(CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels, streams=True))
        return out
    run.__name__ = "ms_lin_" + name
    return scene(run)


for name_ in TMTL.CASES:
    ms_lin_case(name_)


# ---- linearized rt_run_fluxes (the cases of tests/test_gpu_fluxes_lin.py) -----------------------------------------------------------------
@scene
def fluxes_lin():
    levels = list(range(6))
    pm, pl = TML._pair(vsm, arch, "IQU", 13, 4, 5, np.random.default_rng(21), m_max=3, albedo=0.2)[:2]
    out = [CL.rt_run_fluxes(pm, pl, 0, 1, 1, levels)]
    Bd = np.stack([np.ones((5, 4)), 0.3 + 0.1 * np.arange(5)[:, None] * np.ones((1, 4))])
    pm.sources = (H.SolarBeam(), H.ThermalEmission(B_layer=0.05 + 0.1 * np.random.default_rng(23).random((5, 4)), B_layer_dot=Bd))
    out.append(CL.rt_run_fluxes(pm, pl, 0, 1, 1, levels))
    out.append(CL.rt_run_fluxes(pm, pl, 0, 1, 1, [2, 0, 5, 2], max_points=3))
    pm, _, _ = TSE.scene(vsm, arch, "lambertian", "IQU", 5, window=True)
    pm.sources = TSEL._sources(H, "all", 5)          # one Planck slot, two skin slots
    return out, CL.rt_run_fluxes(pm, H.LinModel(list(TSEL._gases(5))), 0, 2, 1, TSE.LEVELS)


# ---- Raman and single scattering (they share the row / weight table and the Fourier weight) -------------------------------------------
@scene
def raman_and_ss():
    pm, prs = TS._raman_pm(vsm, arch, 24, None)
    out = [RR.rt_run(prs, pm, 1)]
    _, pm = TMR._models(vsm, arch, "IQU", 7, 24, 5, np.float64)
    out.append(RR.rt_run_multisensor(TMR._rs(vsm)[1], pm, TMR.LEVELS))
    _, pm = TSS._models(vsm, arch, "IQU", 7, 6, 3, np.float64)
    return out, CR.rt_run_ss(pm)


# ---- the single-scattering column kernels (csrc/vsm_ss.hip): the four drivers and the tests' kernel helpers ---------------------------
FTS = (np.float64, np.float32)
SS_SHAPES = [("IQU", 70, TSS.SHIFTS, TSS.W_IE), ("IQUV", 300, TSS.SHIFTS_BIG, TSS.W_IE_BIG), ("I", 1, TSS.SHIFTS, TSS.W_IE),
             ("I", 7, TSS.SHIFTS, TSS.W_IE)]


@scene
def ss_forward_runs():
    """rt_run_ss and rt_run_ss_rrs (the columns with hem_R / hem_T, the Raman column with staged and global donors)."""
    out = []
    for FT in FTS:
        for pol, S, shifts, w_ie in SS_SHAPES:
            _, pm = TSS._models(vsm, arch, pol, 7, S, 3, FT)
            out += [CR.rt_run_ss(pm), RR.rt_run_ss(TSS._rs_pair(vsm, shifts, w_ie)[1], pm, 1)]
    return out


@scene
def ss_lin_runs():
    """rt_run_ss_lin with one aerosol (the Z_dot kernel), without one, and over Cox-Munk; rt_run_ss_rrs_lin."""
    out = []
    for FT in FTS:
        for pol, S, shifts, w_ie in SS_SHAPES[:3]:
            for naer in (1, 0):
                _, _, pm, hl = TSL._scene(vsm, arch, pol, S, naer, 2, FT)
                out.append(CL.rt_run_ss(pm, hl, naer, 2, 1))
            out.append(RR.rt_run_ss_lin(TSS._rs_pair(vsm, shifts, w_ie)[1], pm, hl, 0, 2, 1))
        _, _, pm, hl = TSL._scene(vsm, arch, "IQU", 70, 1, 2, FT)
        out.append(RR.rt_run_ss_lin(TSS._rs_pair(vsm, TSS.SHIFTS, TSS.W_IE)[1], pm, hl, 1, 2, 1))
        _, _, pm, hl = TSL._scene(vsm, arch, "IQU", 70, 0, 2, FT, surface=H.CoxMunkSurface(wind_speed=5.0))
        pm.m_max = 3
        out.append(CL.rt_run_ss(pm, hl, 0, 2, 1))
    return out


@scene
def ss_kernel_cases():
    """The _kernel_case helpers of the three test files: the four kernels on the oracle's inputs, with halo = 0 (donors from global
    memory) and the clamped halo (donors staged), and with a slot sub-range."""
    out = []
    for FT in FTS:
        for pol, S, shifts, w_ie in SS_SHAPES[:3]:
            om, pm = TSS._models(vsm, arch, pol, 7, S, 3, FT)
            ors = TSS._rs_pair(vsm, shifts, w_ie)[0]
            out += [TSS._kernel_case(vsm, arch, om, pm, FT, rs=ors, halo=h) for h in (0, 10 ** 6)]
            om, ol, pm, _ = TSL._scene(vsm, arch, pol, S, 0, 2, FT)
            out += [TSL._kernel_case(vsm, arch, om, ol, pm, FT), TSL._kernel_case(vsm, arch, om, ol, pm, FT, p_range=(1, 3))]
            om, ol, pm, _ = TSL._scene(vsm, arch, pol, S, 1, 2, FT)
            out += [TSRL._kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=h) for h in (0, 10 ** 6)]
            out.append(TSRL._kernel_case(vsm, arch, om, ol, pm, ors, FT, halo=10 ** 6, p_ranges=((0, 3), (3, 10))))
    return out


for name_, f in SCENES.items():
    if a.only and name_ not in a.only.split(","):
        continue
    arrays = flatten(f())
    for k, x in enumerate(arrays):
        np.save(os.path.join(a.dump, "%s.%03d.npy" % (name_, k)), x)
    print("%-28s %3d arrays" % (name_, len(arrays)), flush=True)
vsm._lib.check_device_status("driver_bits")
