#!/usr/bin/env python3
"""Raman multi-sensor run against CoreRTRaman.rt_run on the C5 scene shape (Stokes_IQU, N = 21, 12 layers, K = 40 Raman lines,
m = 0..2, 2 10^4 points, FP64, bench.py's C5 inputs): wall-clock per call, three runs per arm, alternated.  `--arm ms` / `--arm rt`
runs one arm only (for a `rocprofv3 --kernel-trace --stats` run).  `--levels` sets the sensor levels (default 0 6 12)."""
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
ap.add_argument("--arm", choices=["both", "ms", "rt"], default="both")
ap.add_argument("--levels", type=int, nargs="+", default=[0, 6, 12])
ap.add_argument("--points", type=int, default=20000)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

arch = vsm.Architectures.GPU(0)
S, L, K = a.points, 12, 40
H = vsm.host_model
rng = np.random.default_rng(20260929)
dp = np.full(L, 1.0 / L)
tau_rayl = np.tile(0.3 * dp, (S, 1))
tau_abs = (10.0 ** rng.uniform(-4, 0, (S, 1))) * dp[None, :]
model = H.model_from_arrays(arch, "IQU", 9, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=0.05,
                            m_max=2)
model.varpi_Cabannes = 0.96
shifts = np.unique(np.concatenate([np.arange(-K // 2, 0), np.arange(1, K - K // 2 + 1)]) * 7)
rs = vsm.CoreRTRaman.RRS(shifts, np.full(len(shifts), 0.04 / len(shifts)), H.get_greek_rayleigh(0.75))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


arms = {"rt": lambda: vsm.CoreRTRaman.rt_run(rs, model, 1),
        "ms": lambda: vsm.CoreRTRaman.rt_run_multisensor(rs, model, a.levels)}
use = ["rt", "ms"] if a.arm == "both" else [a.arm]
for k in use:
    arms[k]()                       # warm-up (library initialisation, workspaces)
t = {k: [] for k in use}
for _ in range(a.reps):
    for k in use:
        t[k].append(timed(arms[k]))
for k in use:
    print("%s: %s s (min %.4f)" % (k, " ".join("%.4f" % x for x in t[k]), min(t[k])))
if len(use) == 2:
    print("levels %s: multisensor (RRS) / rt_run (RRS) = %.3f (min over runs)" % (a.levels, min(t["ms"]) / min(t["rt"])))
