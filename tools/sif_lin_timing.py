"""The linearized C2-shaped step (bench_secondary.c2_lin: Stokes_IQU, N = 60, 40 layers, m = 0..2, one gas column + albedo, FP64)
with or without a SurfaceSIF source and two SIF slots: step = H2D + device optics + run + D2H, host clock around a device
synchronise (the method of 4.12).  One process times one arm; alternate the arms from the shell.
   python tools/sif_lin_timing.py --sif 1 [--points 2048]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--sif", type=int, default=1)
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--steps", type=int, default=6)
a = ap.parse_args()

import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
from bench import o2a_atmosphere  # noqa: E402

arch = vsm.Architectures.GPU(0)
L = 40
tau_rayl, tau_abs = o2a_atmosphere(a.points, L)
H = vsm.host_model
src = None
if a.sif:
    x = np.linspace(-1.0, 1.0, a.points)
    sif0 = 0.05 * (1.0 + 0.3 * x)
    src = (H.SolarBeam(), H.SurfaceSIF(sif0, np.stack([sif0 / 0.05, x])))      # two tables: amplitude, slope
model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=0.15, m_max=2,
                            sources=src)
scene = vsm.CoreRTLin.SceneLin(model, H.LinModel([tau_abs]), 0, 1, 1)


def step():
    scene.fwd.upload(); scene.fwd.prepare(); scene.upload(); scene.prepare()
    scene.run()
    return scene.results_host()


step(); step()
torch.cuda.synchronize()
ts = []
for _ in range(a.steps):
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
vsm._lib.check_device_status("sif_lin_timing")
print(json.dumps(dict(sif=a.sif, points=a.points, ms=[round(1e3 * t, 2) for t in ts], median_ms=round(1e3 * float(np.median(ts)), 2))))
