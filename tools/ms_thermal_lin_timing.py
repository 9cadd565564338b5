"""The linearized multi-sensor run on the shape of DESIGN 4.8c (Stokes_IQU, N = 60, 40 layers, one gas slot + albedo, m = 0..2, 2048
points, FP64, levels {0, 10, 20, 30, 40}) with or without a thermal source and Planck slots: one call of
CoreRTLin.rt_run_multisensor per step, host clock around it (the call ends with the device synchronised and the results on the host).

One process times one arm:       python tools/ms_thermal_lin_timing.py --thermal 0|1 [--planck K] [--points 2048] [--steps 4]
All arms, alternated, three processes each (a fresh child process per measurement; the parent never opens the device):
                                 python tools/ms_thermal_lin_timing.py --arms [--parent-tree DIR]
--parent-tree: a checkout of the parent commit with its library built; its no-thermal arm is run from there (this tool is copied
in) and reported beside this tree's, with the spread of each arm's three medians -- the two issue the same calls."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--thermal", type=int, default=1)
ap.add_argument("--planck", type=int, default=0)
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--arms", action="store_true")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--root", default=ROOT)
a = ap.parse_args()

if a.arms:
    arms = [("no_thermal", a.root, ["--thermal", "0"]), ("thermal_planck0", a.root, ["--thermal", "1", "--planck", "0"]),
            ("thermal_planck40", a.root, ["--thermal", "1", "--planck", "40"])]
    if a.parent_tree:
        tool = os.path.join(a.parent_tree, "tools", "_ms_thermal_lin_timing_parent.py")
        shutil.copyfile(os.path.abspath(__file__), tool)
        arms.insert(0, ("no_thermal_parent", a.parent_tree, ["--thermal", "0"]))
    med = {name: [] for name, _, _ in arms}
    for rep in range(3):
        for name, root, args in arms:
            script = os.path.abspath(__file__) if root == a.root else tool
            cmd = [sys.executable, script, "--root", root, "--points", str(a.points), "--steps", str(a.steps)] + args
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout.strip().splitlines()[-1]
            med[name].append(json.loads(out)["median_ms"])
    print(json.dumps({name: dict(median_ms=v, spread_ms=round(max(v) - min(v), 2)) for name, v in med.items()}))
    sys.exit(0)

sys.path.insert(0, a.root)
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
from bench import o2a_atmosphere  # noqa: E402

arch = vsm.Architectures.GPU(0)
L, S = 40, a.points
tau_rayl, tau_abs = o2a_atmosphere(S, L)
H = vsm.host_model
src = None
if a.thermal:
    B = np.linspace(0.05, 0.2, L)[:, None] * np.ones((1, S))
    Bd = np.zeros((a.planck, L, S))      # (no table: the source still states B_layer_dot, its ticket into this run)
    for k in range(a.planck):            # unit tables: one weighting function per layer
        Bd[k, k % L] = 1.0
    src = (H.SolarBeam(), H.ThermalEmission(B_layer=B, B_layer_dot=Bd))
model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279, albedo=0.15, m_max=2,
                            sources=src)
lin = H.LinModel([tau_abs])
levels = [0, 10, 20, 30, 40]


def step():
    return vsm.CoreRTLin.rt_run_multisensor(model, lin, 0, 1, 1, levels)


step()
torch.cuda.synchronize()
ts = []
for _ in range(a.steps):
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
print(json.dumps(dict(thermal=a.thermal, planck=a.planck, points=S, ms=[round(1e3 * t, 2) for t in ts],
                      median_ms=round(1e3 * float(np.median(ts)), 2))))
