#!/usr/bin/env python3
"""vsm_absorption_xsec_lin against vsm_absorption_xsec at the shape of DESIGN.md 4.25 / 4.26: a seeded synthetic table of `--lines`
lines, `--points` grid points over 12 987 .. 13 175 cm^-1, `--layers` layers from 1 to 1013 hPa, Voigt with the default error function,
the default cutoff of 40 cm^-1 -- the inputs of tools/absorption_timing.py.  Both calls are timed in this one process on
device-resident inputs: device events around `--reps` back-to-back calls, three windows each after a warm-up, the two calls
alternating.  The linearized call contains the forward call (sigma comes from its unchanged launches), so `lin - forward` is the cost
of the three slots.  The line the linearized call has to stay under is FOUR forward calls: one-sided differences in three parameters
plus the base state."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=2000)
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("absorption_lin_timing: no MI355X visible (there is nothing to time on a CPU)")
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

job = A._prepare_lin(model, grid, p, T)
dev = A._Device(arch)
h = dev.profile_lin(job)
outs = [dev.empty(a.layers, a.points) for _ in range(4)]
ones = np.ones(a.layers)


def forward():
    dev.xsec(job, h, ones, outs[0], 0)


def lin():
    dev.xsec_lin(job, h, ones, *outs, 0)


def window(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    dev.keep[:] = dev.keep[:1]                      # (the per-call scale arrays; the profile handle stays)
    return e0.elapsed_time(e1) / a.reps


for call in (forward, lin):                         # warm-up
    window(call)
times = {"forward": [], "lin": []}
for _ in range(3):
    times["forward"].append(window(forward))
    times["lin"].append(window(lin))
f, l = min(times["forward"]), min(times["lin"])
print("shape: %d lines, %d points, %d layers, Voigt, HW32 SD, cutoff %g" % (job.n_lines, a.points, a.layers, job.wing_cutoff))
print("forward: %s ms per call (min %.4f)" % (" ".join("%.4f" % v for v in times["forward"]), f))
print("lin:     %s ms per call (min %.4f)" % (" ".join("%.4f" % v for v in times["lin"]), l))
print("lin / forward = %.3f (the slots alone: %.4f ms = %.3f forward calls); the line is 4 forward calls = %.4f ms: %s"
      % (l / f, l - f, (l - f) / f, 4 * f, "under" if l < 4 * f else "NOT under"))
sig, dot = (t.cpu().numpy() for t in (outs[0], torch.stack(outs[1:])))
print("sigma max %.3e; max |d sigma / dT| %.3e, |d sigma / dp| %.3e, |d sigma / dvmr_self| %.3e"
      % (sig.max(), np.abs(dot[0]).max(), np.abs(dot[1]).max(), np.abs(dot[2]).max()))
dev.fetch([])
