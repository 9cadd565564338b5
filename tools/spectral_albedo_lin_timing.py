"""The linearized C2-shaped step (bench_secondary.c2_lin: Stokes_IQU, N = 60, 40 layers, m = 0..2, one gas column, FP64) over the
scalar Lambertian albedo (NSurf = 1) or over a three-coefficient LambertianSurfaceLegendre (NSurf = 3): step = H2D + device optics +
run + D2H, host clock around a device synchronise (the method of 4.12).  One process times one arm; alternate the arms
from the shell.
    python tools/spectral_albedo_lin_timing.py --surface legendre [--points 2048] [--tree DIR]
--tree DIR: import the package (and bench.py) of another checkout -- the parent commit's arm, which has the scalar surface only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--surface", choices=["scalar", "legendre"], default="legendre")
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
from bench import o2a_atmosphere  # noqa: E402

arch = vsm.Architectures.GPU(0)
L = 40
tau_rayl, tau_abs = o2a_atmosphere(a.points, L)
H = vsm.host_model
kw = dict(albedo=0.15) if a.surface == "scalar" else dict(surface=H.LambertianSurfaceLegendre([0.15, 0.03, -0.01]))
nsurf = 1 if a.surface == "scalar" else 3
model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, m_max=2, **kw)
scene = vsm.CoreRTLin.SceneLin(model, H.LinModel([tau_abs]), 0, 1, nsurf)


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
vsm._lib.check_device_status("spectral_albedo_lin_timing")
als = scene.als
surface_lin_bytes = sum(int(getattr(als, f).numel()) for f in ("ap_r_mp", "ap_t_pp", "ap_r_pm", "ap_t_mm", "ap_J0_p", "ap_J0_m")) * als.ap_r_mp.element_size()
print(json.dumps(dict(surface=a.surface, tree=os.path.abspath(a.tree) != os.path.dirname(os.path.dirname(os.path.abspath(__file__))) and "other" or "this",
                      points=a.points, sub0=scene.sub0 is not None, ms=[round(1e3 * t, 2) for t in ts],
                      median_ms=round(1e3 * float(np.median(ts)), 2), surface_lin_bytes=surface_lin_bytes)))
