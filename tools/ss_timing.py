#!/usr/bin/env python3
"""Single-scattering runs against the full runs: wall-clock per call, three runs per arm, alternated.
  elastic  rt_run_ss vs rt_run on the C2 scene shape (Stokes_IQU, N = 60, 40 layers, 10^4 points, FP64)
  raman    CoreRTRaman.rt_run_ss vs CoreRTRaman.rt_run on the C5 shape (Stokes_IQU, N = 21, 12 layers, 40 lines, 4000 points, FP64)
`--arm ss_rrs` (or ss / rt / rrs) runs one arm only, three calls after a warm-up (for a `rocprofv3 --kernel-trace --stats` run)."""
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
ap.add_argument("--arm", choices=["both", "rt", "ss", "rrs", "ss_rrs"], default="both")
ap.add_argument("--points", type=int, default=10000, help="spectral points of the C2 shape")
ap.add_argument("--raman-points", type=int, default=4000, help="spectral points of the C5 shape")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

arch = vsm.Architectures.GPU(0)
H = vsm.host_model
rng = np.random.default_rng(0)
S, L = a.points, 40
c2 = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=np.tile(0.1 * np.full(L, 1.0 / L), (S, 1)),
                         tau_abs=10.0 ** rng.uniform(-4, 1, (S, 1)) * np.full((1, L), 1.0 / L), depol=0.0279, albedo=0.15, m_max=2)
S5, L5, K = a.raman_points, 12, 40
dp = np.full(L5, 1.0 / L5)
c5 = H.model_from_arrays(arch, "IQU", 9, 40.0, [30.0], [0.0], tau_rayl=np.tile(0.3 * dp, (S5, 1)),
                         tau_abs=(10.0 ** rng.uniform(-4, 0, (S5, 1))) * dp[None, :], depol=0.0075, albedo=0.05, m_max=2)
c5.varpi_Cabannes = 0.96
shifts = np.unique(np.concatenate([np.arange(-K // 2, 0), np.arange(1, K - K // 2 + 1)]) * 7)
rs = vsm.CoreRTRaman.RRS(shifts, np.full(len(shifts), 0.04 / len(shifts)), H.get_greek_rayleigh(0.75))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


arms = {"rt": lambda: vsm.CoreRT.rt_run(c2), "ss": lambda: vsm.CoreRT.rt_run_ss(c2),
        "rrs": lambda: vsm.CoreRTRaman.rt_run(rs, c5, 1), "ss_rrs": lambda: vsm.CoreRTRaman.rt_run_ss(rs, c5, 1)}
pairs = [("rt", "ss"), ("rrs", "ss_rrs")] if a.arm == "both" else [(a.arm,)]
for pair in pairs:
    for k in pair:
        arms[k]()                       # warm-up (library initialisation, workspaces)
    t = {k: [] for k in pair}
    for _ in range(a.reps):
        for k in pair:
            t[k].append(timed(arms[k]))
    for k in pair:
        print("%s: %s s (min %.4f)" % (k, " ".join("%.4f" % x for x in t[k]), min(t[k])))
    if len(pair) == 2:
        pts = S if pair[0] == "rt" else S5
        print("%s / %s = %.1f x (min over runs); %s: %.0f spectral-points/s" % (pair[0], pair[1], min(t[pair[0]]) / min(t[pair[1]]),
                                                                               pair[1], pts / min(t[pair[1]])))
