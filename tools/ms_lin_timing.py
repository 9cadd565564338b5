#!/usr/bin/env python3
"""Linearized multi-sensor run against rt_run_lin on the C2-lin scene shape (Stokes_IQU, N = 60, 40 layers, one gas slot + the
albedo, 2048 points, FP64): wall-clock per call, three runs per arm, alternated.  `--arm ms` / `--arm lin` runs one arm only (for a
`rocprofv3 --kernel-trace --stats` run).  `--levels` sets the sensor levels (default 0 10 20 30 40)."""
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
ap.add_argument("--arm", choices=["both", "ms", "lin"], default="both")
ap.add_argument("--levels", type=int, nargs="+", default=[0, 10, 20, 30, 40])
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

arch = vsm.Architectures.GPU(0)
S, L = a.points, 40
rng = np.random.default_rng(0)
tau_rayl = np.tile(0.1 * np.full(L, 1.0 / L), (S, 1))
base = 10.0 ** rng.uniform(-4, 1, (S, 1)) * np.full((1, L), 1.0 / L)
H = vsm.host_model
model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=base, depol=0.0279, albedo=0.15,
                            m_max=2)
lin = H.LinModel([base])


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


arms = {"lin": lambda: vsm.CoreRTLin.rt_run_lin(model, lin, 0, 1, 1),
        "ms": lambda: vsm.CoreRTLin.rt_run_multisensor(model, lin, 0, 1, 1, a.levels)}
use = ["lin", "ms"] if a.arm == "both" else [a.arm]
for k in use:
    arms[k]()                       # warm-up (library initialisation, workspaces)
t = {k: [] for k in use}
for _ in range(a.reps):
    for k in use:
        t[k].append(timed(arms[k]))
for k in use:
    print("%s: %s s (min %.4f)" % (k, " ".join("%.4f" % x for x in t[k]), min(t[k])))
if len(use) == 2:
    print("levels %s: linearized multisensor / rt_run_lin = %.3f (min over runs)" % (a.levels, min(t["ms"]) / min(t["lin"])))
