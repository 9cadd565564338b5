#!/usr/bin/env python3
"""What fluxes at every layer boundary cost: ONE arm per process, on the C2-shaped model of tools/ms_timing.py
(Stokes_IQU, N = 60, 40 layers, m = 0..2, 2048 points, FP64), two warm-up steps, then `--steps` steps timed with a host clock
around a device synchronise; prints one JSON line with the steps and their median.

  --arm ms        rt_run_multisensor(model, all levels, streams=True) and the numpy quadrature of its m = 0 level vectors: what a
                  user did before rt_run_fluxes (the only arm a tree without rt_run_fluxes can run)
  --arm flux      rt_run_fluxes(model)
  --arm flux_toa_boa   rt_run_fluxes(model, levels=[0, Nz])

`--root DIR` imports the package of another checkout (the parent commit, built in its own tree), so that both trees are measured
by the same script in one session; alternate the processes of the arms."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["ms", "flux", "flux_toa_boa"], required=True)
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
tau_abs = 10.0 ** rng.uniform(-4, 1, (S, 1)) * np.full((1, L), 1.0 / L)
model = vsm.host_model.model_from_arrays(arch, "IQU", 35, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0279,
                                         albedo=0.15, m_max=2)
levels = list(range(L + 1))


def quadrature_of_streams():
    """The fluxes by hand: every level with streams=True, the m = 0 vectors of Stokes I, the mu w quadrature, the direct beam."""
    res = vsm.CoreRT.rt_run_multisensor(model, levels, streams=True)
    qp, n = model.quad_points, res.pol_n
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    tau = np.concatenate([np.zeros((S, 1)), np.cumsum(tau_rayl + tau_abs, axis=1)], axis=1)      # (Rayleigh: no delta-M scaling)
    out = {}
    for i, l in enumerate(levels):
        uw, dw = res.uw_streams[i][0][::n, 0, :], res.dw_streams[i][0][::n, 0, :]
        beam = np.exp(-tau[:, l] / res.mu0)
        out[l] = ((mu * w) @ uw, np.zeros(S) if l == 0 else (mu * w) @ dw, res.mu0 * beam, w @ uw, w @ dw, beam)
    return out


arms = {"ms": quadrature_of_streams, "flux": lambda: vsm.CoreRT.rt_run_fluxes(model),
        "flux_toa_boa": lambda: vsm.CoreRT.rt_run_fluxes(model, levels=[0, L])}
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
