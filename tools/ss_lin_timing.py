#!/usr/bin/env python3
"""The linearized single-scattering run against what it replaces: wall-clock per call, three runs per arm, alternated.  Shape
C2-lin (tools/lin_timing.py: Stokes_IQU, N = 60, 40 layers, 2000 points, one gas slot + albedo, FP64).
  lin     CoreRTLin.rt_run_lin        the full linearized run (exact Jacobians)
  ss      CoreRT.rt_run_ss            one forward single-scattering run ((P + 1) of them = the finite-difference Jacobian)
  ss_lin  CoreRTLin.rt_run_ss         the analytic single-scattering Jacobian
`--aerosols 1` adds one synthetic aerosol in the lower half of the column with its 7 Jacobian slots (P = 8 + gases: the kernel form
that forms Z_dot from component blocks).  `--arm ss_lin` (or lin / ss) runs one arm only, three calls after a warm-up (for a
`rocprofv3 --kernel-trace --stats` run).
Run each GPU step under a time limit of its own, e.g. `timeout -k 10 300 python tools/ss_lin_timing.py`."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["all", "lin", "ss", "ss_lin"], default="all")
ap.add_argument("--points", type=int, default=2000)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--gases", type=int, default=1)
ap.add_argument("--aerosols", type=int, default=0, choices=[0, 1])
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

arch = vsm.Architectures.GPU(0)
H = vsm.host_model
S, L, G = a.points, a.layers, a.gases
tau_rayl, tau_abs = bench.o2a_atmosphere(S, L)
kw, lkw, A = {}, {}, a.aerosols
if A:
    import numpy as np  # noqa: E402
    l_ = np.arange(36)
    greek = lambda g, f: H.GreekCoefs(alpha=np.where(l_ >= 2, 0.8, 0.0) * f * (2 * l_ + 1) * g ** l_, beta=f * (2 * l_ + 1) * g ** l_,
                                      gamma=np.where(l_ >= 2, -0.3, 0.0) * f * (2 * l_ + 1) * g ** l_ / (1 + 0.3 * l_),
                                      delta=np.where(l_ >= 1, 0.7, 0.0) * f * (2 * l_ + 1) * g ** l_,
                                      epsilon=np.where(l_ >= 2, 0.1, 0.0) * f * (2 * l_ + 1) * g ** l_ / (1 + l_),
                                      zeta=np.where(l_ >= 2, 0.6, 0.0) * f * (2 * l_ + 1) * g ** l_)
    tau_aer = np.zeros((1, L))
    tau_aer[0, L // 2:] = 0.2 / (L - L // 2)
    tad = np.zeros((1, 7, L))
    tad[0, :, L // 2:] = np.array([1.0, 0.02, -0.03, 0.1, 0.01, 0.5, -0.2])[:, None] / (L - L // 2)
    kw = dict(tau_aer=tau_aer, aerosol_optics=[H.AerosolOptics(greek(0.65, 1.0), 0.93, 0.12)])
    lkw = dict(tau_aer_dot=tad, lin_aerosol_optics=[H.LinAerosolOptics([greek(0.5 + 0.05 * k, 0.01 * (k + 1)) for k in range(4)],
                                                                       np.array([0.02, -0.3, 0.05, 0.01]),
                                                                       np.array([0.01, 0.02, 0.2, -0.05]))])
model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=0.15,
                            m_max=2, **kw)
lin = H.LinModel([tau_abs / G for _ in range(G)], **lkw)
P = 7 * A + G + 1


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


arms = {"lin": lambda: vsm.CoreRTLin.rt_run_lin(model, lin, A, G, 1), "ss": lambda: vsm.CoreRT.rt_run_ss(model),
        "ss_lin": lambda: vsm.CoreRTLin.rt_run_ss(model, lin, A, G, 1)}
names = list(arms) if a.arm == "all" else [a.arm]
for k in names:
    arms[k]()                       # warm-up (library initialisation, workspaces)
t = {k: [] for k in names}
for _ in range(a.reps):
    for k in names:
        t[k].append(timed(arms[k]))
for k in names:
    print("%s: %s s (min %.4f)" % (k, " ".join("%.4f" % x for x in t[k]), min(t[k])))
if a.arm == "all":
    m = {k: min(v) for k, v in t.items()}
    print("P = %d; rt_run_lin / ss_lin = %.1f x; (P + 1) rt_run_ss / ss_lin = %.2f x; ss_lin: %.0f spectral-points/s"
          % (P, m["lin"] / m["ss_lin"], (P + 1) * m["ss"] / m["ss_lin"], S / m["ss_lin"]))
