#!/usr/bin/env python3
"""vsm_absorption_xsec at one shape: a seeded synthetic table of `--lines` lines, `--points` grid points over
12 987 .. 13 175 cm^-1, `--layers` layers from 1 to 1013 hPa, Voigt with the default error function, the default cutoff of 40 cm^-1.
  xsec          the two launches of one call on device-resident inputs, device events around `--reps` back-to-back calls, three windows
                after a warm-up
  evaluations   line-shape evaluations of one call, counted from the windows the parameter pass wrote: sum of (istop - istart + 1)
  call          compute_absorption_cross_section as a user calls it (host part, upload and the one synchronisation), host clock
  paths         of those, the evaluations with |x| + y < 8 (Weideman's 32-term polynomial); the rest take Humlicek's region II
The share of the vector-FP64 rate uses the as-written operation counts of one Voigt evaluation (every multiply, add and divide
counted once, a fused multiply-add twice): 247 on the Weideman path, of which 217 are the 31 complex Horner steps, 38 on the
Humlicek path."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

OPS_WEIDEMAN, OPS_HUMLICEK = 247, 38
PEAK_VECTOR_FP64 = 78.6e12     # FLOP/s, the card's published vector FP64 rate

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=2000)
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("absorption_timing: no MI355X visible (there is nothing to time on a CPU)")
A = vsm.Absorption
arch = vsm.Architectures.GPU(0)
rng = np.random.default_rng(0)
n = a.lines
TT = np.arange(100.0, 420.0, 20.0)
table = A.HitranTable(mol=np.full(n, 7), iso=np.ones(n, dtype=int), nu=rng.uniform(12987.0, 13175.0, n), S=10.0 ** rng.uniform(-27, -23, n),
                      A=np.zeros(n), gamma_air=rng.uniform(0.03, 0.06, n), gamma_self=rng.uniform(0.03, 0.06, n),
                      E_low=rng.uniform(0.0, 2000.0, n), n_air=rng.uniform(0.6, 0.75, n), delta_air=rng.uniform(-0.01, 0.0, n))
model = A.make_hitran_model(table, A.Voigt(), architecture=arch,
                            isotopologues={(7, 1): A.IsotopologueData(31.98983, TT, 215.73 * (TT / 296.0) ** 1.01)})
grid = np.linspace(12987.0, 13175.0, a.points)
p = np.geomspace(1.0, 1013.0, a.layers)
T = np.linspace(200.0, 295.0, a.layers)

job = A._prepare(model, grid, p, T)
dev = A._Device(arch)
h = dev.profile(job)
out = dev.empty(a.layers, a.points)
ones = np.ones(a.layers)
dev.xsec(job, h, ones, out, 0)
torch.cuda.synchronize()
win = h["work"].view(a.layers, job.n_lines, 8)[:, :, 7].contiguous().view(torch.int32).view(a.layers, job.n_lines, 2).cpu().numpy()
evals = int(np.sum(np.maximum(win[..., 1].astype(np.int64) - win[..., 0] + 1, 0)))
rec = h["work"].view(a.layers, job.n_lines, 8).cpu().numpy()
nu, y, sx = rec[..., 0], rec[..., 3], rec[..., 6]
half = np.maximum(8.0 - y, 0.0) / sx                              # |x| + y < 8  <=>  |nu_i - nu| < (8 - y) / sx
i0 = np.maximum(np.searchsorted(grid, (nu - half).ravel(), side="right").reshape(nu.shape) + 1, win[..., 0])
i1 = np.minimum(np.searchsorted(grid, (nu + half).ravel(), side="left").reshape(nu.shape), win[..., 1])
n_w = int(np.sum(np.maximum(i1.astype(np.int64) - i0 + 1, 0)))
ops = n_w * OPS_WEIDEMAN + (evals - n_w) * OPS_HUMLICEK
print("shape: %d lines, %d points, %d layers; %d line-shape evaluations per call (%.1f %% of lines x points x layers)"
      % (job.n_lines, a.points, a.layers, evals, 100.0 * evals / (job.n_lines * a.points * a.layers)))
print("paths: %d evaluations (%.2f %%) on the Weideman path, %d on the Humlicek path; %.3e operations per call as written"
      % (n_w, 100.0 * n_w / evals, evals - n_w, ops))
times = []
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        dev.xsec(job, h, ones, out, 0)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / a.reps)
t = min(times) * 1e-3
print("xsec: %s ms per call (%d calls per window, min %.4f ms)" % (" ".join("%.4f" % v for v in times), a.reps, min(times)))
print("      %.3e evaluations/s; %.2f TFLOP/s as written = %.1f %% of %.1f TFLOP/s vector FP64"
      % (evals / t, ops / t / 1e12, 100.0 * ops / t / PEAK_VECTOR_FP64, PEAK_VECTOR_FP64 / 1e12))
dev.fetch([])
calls = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sig = A.compute_absorption_cross_section(model, grid, p, T)
    calls.append(time.perf_counter() - t0)
print("call: %s s (host part, upload, one synchronisation, download)  sigma max %.3e" % (" ".join("%.4f" % c for c in calls), sig.max()))
