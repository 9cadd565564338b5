#!/usr/bin/env python3
"""What flux Jacobians at every layer boundary cost: ONE arm per process, on the C2-lin shape of
tools/ms_lin_timing.py (Stokes_IQU, N = 60, 40 layers, one gas slot + the albedo, 2048 points, FP64, all 41 levels), two warm-up
steps, then `--steps` steps timed with a host clock around a device synchronise; prints one JSON line with the steps and their
median.

  --arm ms        CoreRTLin.rt_run_multisensor(model, ..., all levels, streams=True) and the numpy quadrature of its m = 0 level
                  vectors and derivative vectors, the direct beam differentiated by hand: what a user did before
                  CoreRTLin.rt_run_fluxes (the only arm a tree without it can run)
  --arm flux      CoreRTLin.rt_run_fluxes(model, ...)

`--root DIR` imports the package of another checkout (the parent commit, built in its own tree), so that both trees are measured
by the same script in one session; alternate the processes of the arms."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["ms", "flux"], required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tag", default="")
a = ap.parse_args()

sys.path.insert(0, os.path.abspath(a.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

arch = vsm.Architectures.GPU(0)
S, L = a.points, a.layers
rng = np.random.default_rng(0)
tau_rayl = np.tile(0.1 * np.full(L, 1.0 / L), (S, 1))
base = 10.0 ** rng.uniform(-4, 1, (S, 1)) * np.full((1, L), 1.0 / L)
H = vsm.host_model
model = H.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=base, depol=0.0279, albedo=0.15, m_max=2)
lin = H.LinModel([base])
levels = list(range(L + 1))


def quadrature_of_streams():
    """The fluxes and their Jacobians by hand: every level with streams=True, the m = 0 vectors of Stokes I and their derivative
    vectors, the mu w quadrature, the direct beam and its derivative with respect to the gas."""
    res = vsm.CoreRTLin.rt_run_multisensor(model, lin, 0, 1, 1, levels, streams=True)
    qp, n = model.quad_points, res.pol_n
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    cum = lambda x: np.concatenate([np.zeros((S, 1)), np.cumsum(x, axis=1)], axis=1)
    tau, tau_dot = cum(tau_rayl + base), cum(base)                       # (Rayleigh: no delta-M scaling)
    out = {}
    for i, l in enumerate(levels):
        z = 0.0 if l == 0 else 1.0
        uw, dw = res.uw_streams[i][0][::n, 0], res.dw_streams[i][0][::n, 0]
        ud, dd = res.uw_dot_streams[i][0][::n, 0], res.dw_dot_streams[i][0][::n, 0]
        beam = np.exp(-tau[:, l] / res.mu0)
        beam_dot = np.stack([-beam * tau_dot[:, l] / res.mu0, np.zeros(S)], axis=1)
        out[l] = ((mu * w) @ uw, z * ((mu * w) @ dw), res.mu0 * beam, w @ uw, z * (w @ dw), beam,
                  np.tensordot(mu * w, ud, axes=(0, 0)), z * np.tensordot(mu * w, dd, axes=(0, 0)), res.mu0 * beam_dot,
                  np.tensordot(w, ud, axes=(0, 0)), z * np.tensordot(w, dd, axes=(0, 0)), beam_dot)
    return out


arms = {"ms": quadrature_of_streams, "flux": lambda: vsm.CoreRTLin.rt_run_fluxes(model, lin, 0, 1, 1)}
f = arms[a.arm]
for _ in range(a.warmup):
    f()
t = []
for _ in range(a.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    t.append(time.perf_counter() - t0)
print(json.dumps(dict(arm=a.arm, tag=a.tag, points=S, layers=L, steps_s=[round(x, 5) for x in t],
                      median_s=round(statistics.median(t), 5), build=vsm._lib.build_info().get("source_hash"))))
