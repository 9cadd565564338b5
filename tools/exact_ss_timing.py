#!/usr/bin/env python3
"""Exact single-scattering runs (vsm.StandaloneSS.run_exact_ss) on the C2 scene shape (40 layers, 10^4 points, 3 viewing angles,
FP64): wall-clock of whole calls -- host tables, H2D of the contributors' optical depths, the kernels, D2H of the paths -- three
runs per arm, alternated.
  iqu12   Stokes_IQU, paths 1 + 2 (Rayleigh + absorption + one Greek aerosol)
  all     scalar, all four paths, 16 inner nodes, 64 azimuth nodes
  ss      CoreRT.rt_run_ss on the same model, for scale (the truncated first-order field)
`--arm iqu12` (or all / ss) runs one arm only, three calls after a warm-up (for a `rocprofv3 --kernel-trace --stats` run)."""
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
ap.add_argument("--arm", choices=["every", "iqu12", "all", "ss"], default="every")
ap.add_argument("--points", type=int, default=10000, help="spectral points of the C2 shape")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

arch = vsm.Architectures.GPU(0)
H, SS = vsm.host_model, vsm.StandaloneSS
rng = np.random.default_rng(0)
S, L = a.points, 40
tau_aer = np.zeros((1, L))
tau_aer[0, 25:35] = 0.02
g = H.henyey_greenstein_greek(0.7, 19)
kw = dict(tau_rayl=np.tile(0.1 * np.full(L, 1.0 / L), (S, 1)), tau_abs=10.0 ** rng.uniform(-4, 1, (S, 1)) * np.full((1, L), 1.0 / L),
          tau_aer=tau_aer, aerosol_optics=[H.AerosolOptics(g, 0.95, 0.0)], depol=0.0279, albedo=0.15, m_max=2)
vza, vaz = [30.0, 45.0, 60.0], [0.0, 60.0, 120.0]
c2 = H.model_from_arrays(arch, "IQU", 35, 40.0, vza, vaz, **kw)
c2_scalar = H.model_from_arrays(arch, "I", 35, 40.0, vza, vaz, **kw)


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


arms = {"iqu12": lambda: SS.run_exact_ss(c2, "paths_1_2"), "all": lambda: SS.run_exact_ss(c2_scalar, "all"),
        "ss": lambda: vsm.CoreRT.rt_run_ss(c2)}
names = list(arms) if a.arm == "every" else [a.arm]
for k in names:
    arms[k]()                       # warm-up (library initialisation, scratch)
t = {k: [] for k in names}
for _ in range(a.reps):
    for k in names:
        t[k].append(timed(arms[k]))
for k in names:
    print("%s: %s s (min %.4f); %.0f spectral-points/s" % (k, " ".join("%.4f" % x for x in t[k]), min(t[k]), S / min(t[k])))
