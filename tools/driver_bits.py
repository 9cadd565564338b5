"""Every driver entry point on a fixed list of small scenes, array by array: the check that a change to the Python drivers
(core_rt*.py) that only re-sequences the same launches changes no bit of any result.

  python tools/driver_bits.py --dump DIR [--tree TREE]    every scene in ONE fresh child process (this process never opens the
                                                          device); every returned array as DIR/<scene>.<k>.npy.  --tree: run the
                                                          package, the oracle and the tests' builders of another checkout (its
                                                          library built), e.g. a copy of the parent commit
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
                             os.path.abspath(a.tree)], cwd=a.tree).returncode)

sys.path[:0] = [a.tree, os.path.join(a.tree, "tests")]
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
import brdf_lin_oracle as B  # noqa: E402
import test_gpu_brdf_lin as TB  # noqa: E402
import test_gpu_lin as TLIN  # noqa: E402
import test_gpu_multisensor as TMS  # noqa: E402
import test_gpu_multisensor_lin as TML  # noqa: E402
import test_gpu_multisensor_raman as TMR  # noqa: E402
import test_gpu_multisensor_thermal_lin as TMTL  # noqa: E402
import test_gpu_sif as TS  # noqa: E402
import test_gpu_ss as TSS  # noqa: E402

H, CR, CL, RR = vsm.host_model, vsm.CoreRT, vsm.CoreRTLin, vsm.CoreRTRaman
arch = vsm.Architectures.GPU(0)
rng = lambda: np.random.default_rng(7)
SCENES = {}


def scene(f):
    SCENES[f.__name__] = f
    return f


def flatten(x):
    """The arrays of a result, in a fixed order: tuples, lists, dicts, result dataclasses, device tensors."""
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


# ---- Raman and single scattering (they share the row / weight table and the Fourier weight) -------------------------------------------
@scene
def raman_and_ss():
    pm, prs = TS._raman_pm(vsm, arch, 24, None)
    out = [RR.rt_run(prs, pm, 1)]
    _, pm = TMR._models(vsm, arch, "IQU", 7, 24, 5, np.float64)
    out.append(RR.rt_run_multisensor(TMR._rs(vsm)[1], pm, TMR.LEVELS))
    _, pm = TSS._models(vsm, arch, "IQU", 7, 6, 3, np.float64)
    return out, CR.rt_run_ss(pm)


for name_, f in SCENES.items():
    arrays = flatten(f())
    for k, x in enumerate(arrays):
        np.save(os.path.join(a.dump, "%s.%03d.npy" % (name_, k)), x)
    print("%-28s %3d arrays" % (name_, len(arrays)), flush=True)
vsm._lib.check_device_status("driver_bits")
