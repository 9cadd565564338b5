#!/usr/bin/env python3
"""Thermal multi-sensor run on the C2 scene shape (Stokes_IQU, N = 60, 40 layers, 10^4 points, FP64), levels 0 10 40: wall-clock
per call of
  ms_th  rt_run_multisensor(thermal=True) with SolarBeam + ThermalEmission,
  ms     rt_run_multisensor without a thermal source,
  rt_th  rt_run with SolarBeam + ThermalEmission,
three runs per arm, alternated; then the same two multi-sensor arms with m_max = 0, whose difference over the thermal arm is
the share of moment m = 0 spent in the thermal slot.  `--arm NAME` runs one arm only (for a `rocprofv3 --kernel-trace --stats`
run)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["all", "ms_th", "ms", "rt_th"], default="all")
ap.add_argument("--levels", type=int, nargs="+", default=[0, 10, 40])
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

arch = vsm.Architectures.GPU(0)
H = vsm.host_model
S, L = a.points, 40
rng = np.random.default_rng(0)
tau_rayl = np.tile(0.1 * np.full(L, 1.0 / L), (S, 1))
tau_abs = 10.0 ** rng.uniform(-4, 1, (S, 1)) * np.full((1, L), 1.0 / L)
B = 0.05 + 0.1 * rng.random((L, S))


def model(m_max, thermal):
    src = (H.SolarBeam(), H.ThermalEmission(B_layer=B)) if thermal else None
    return H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=0.15,
                               m_max=m_max, sources=src)


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(arms, use):
    for k in use:
        arms[k]()                   # warm-up (library initialisation, workspaces)
    t = {k: [] for k in use}
    for _ in range(a.reps):
        for k in use:
            t[k].append(timed(arms[k]))
    for k in use:
        print("%s: %s s (min %.4f)" % (k, " ".join("%.4f" % x for x in t[k]), min(t[k])))
    return {k: min(v) for k, v in t.items()}


th, so = model(2, True), model(2, False)
arms = {"ms_th": lambda: vsm.CoreRT.rt_run_multisensor(th, a.levels, thermal=True),
        "ms": lambda: vsm.CoreRT.rt_run_multisensor(so, a.levels),
        "rt_th": lambda: vsm.CoreRT.rt_run(th)}
t = measure(arms, list(arms) if a.arm == "all" else [a.arm])
if a.arm == "all":
    print("levels %s: thermal / plain multisensor = %.3f, thermal multisensor / rt_run = %.3f (min over runs)"
          % (a.levels, t["ms_th"] / t["ms"], t["ms_th"] / t["rt_th"]))
    th0, so0 = model(0, True), model(0, False)
    print("m_max = 0:")
    t0 = measure({"ms_th": lambda: vsm.CoreRT.rt_run_multisensor(th0, a.levels, thermal=True),
                  "ms": lambda: vsm.CoreRT.rt_run_multisensor(so0, a.levels)}, ["ms_th", "ms"])
    print("share of m = 0 spent in the thermal slot: %.3f" % ((t0["ms_th"] - t0["ms"]) / t0["ms_th"]))
