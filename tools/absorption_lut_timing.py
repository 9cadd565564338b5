#!/usr/bin/env python3
"""Absorption.InterpolationModel against the line-by-line call at the shape of DESIGN.md 4.25: the seeded synthetic table of
`--lines` lines, `--points` grid points over 12 987 .. 13 175 cm^-1, `--layers` layers from 1 to 1013 hPa, Voigt with the default
error function and cutoff (the inputs of tools/absorption_timing.py and tools/absorption_lin_timing.py), and a sigma(nu, p, T) table
of `--np` x `--nt` states on those grid points.  The method of tools/absorption_lin_timing.py: everything is resident on the device
(the library is called with device pointers, nothing is uploaded inside a window), device events around `--reps` back-to-back calls,
three windows after a warm-up, the calls alternating in this one process.

    build       vsm_absorption_xsec over the nP nT states, and vsm_absorption_lut_prefilter
    forward     vsm_absorption_lut_eval (cubic and linear, FP64 and FP32) against vsm_absorption_xsec on the same profile
    linearized  vsm_absorption_lut_eval_lin against vsm_absorption_lut_eval (and vsm_absorption_xsec_lin beside it)
    traffic     the evaluation's algorithmic bytes -- 16 (linear: 4) coefficient rows read and 1 (linearized: 3) row written per
                layer -- over the measured time"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
from vsmartmom_jl_amd import core_rt as CR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=2000)
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--np", type=int, default=25)
ap.add_argument("--nt", type=int, default=15)
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("absorption_lut_timing: no MI355X visible (there is nothing to time on a CPU)")
A, lib = vsm.Absorption, vsm._lib.lib()
arch = vsm.Architectures.GPU(0)
rng = np.random.default_rng(0)
n = a.lines
TT = np.arange(100.0, 420.0, 20.0)
table = A.HitranTable(mol=np.full(n, 7), iso=np.ones(n, dtype=int), nu=rng.uniform(12987.0, 13175.0, n), S=10.0 ** rng.uniform(-27, -23, n),
                      A=np.zeros(n), gamma_air=rng.uniform(0.03, 0.06, n), gamma_self=rng.uniform(0.03, 0.06, n),
                      E_low=rng.uniform(0.0, 2000.0, n), n_air=rng.uniform(0.6, 0.75, n), delta_air=rng.uniform(-0.01, 0.0, n))
iso = {(7, 1): A.IsotopologueData(31.98983, TT, 215.73 * (TT / 296.0) ** 1.01)}
model = A.make_hitran_model(table, A.Voigt(), architecture=arch, isotopologues=iso)
nu = A.UniformRange(12987.0, (13175.0 - 12987.0) / (a.points - 1), a.points)
pg, tg = A.UniformRange(1.0, 1012.0 / (a.np - 1), a.np), A.UniformRange(195.0, 105.0 / (a.nt - 1), a.nt)
grid = nu.values()
p = np.geomspace(1.0, 1013.0, a.layers)
T = np.linspace(200.0, 295.0, a.layers)
dev = A._Device(arch)
ones = dev.conv(np.ones(max(a.layers, a.np * a.nt)))


def window(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(calls, reps):
    """{name: [three window means in ms]}: a warm-up window each, then three rounds with the calls alternating."""
    for c in calls.values():
        window(c, max(1, reps // 4))
    times = {k: [] for k in calls}
    for _ in range(3):
        for k, c in calls.items():
            times[k].append(window(c, reps))
    return times


def xsec_call(job, h, out, lin_outs=None):
    d = h["dev"]
    head = [len(job.grid), job.n_lines, len(job.molar_mass), len(job.p)] + [CR._ptr(t) for t in d[:13]] + [CR._ptr(ones), CR._ptr(h["q"])]
    tail = [C.c_double(job.wing_cutoff), C.c_double(job.delta_max), job.broadening, job.cef, 0, CR._ptr(out)]
    if lin_outs is None:
        return lambda: vsm._lib.check(lib.vsm_absorption_xsec(*head, *tail, CR._ptr(h["work"]), None))
    return lambda: vsm._lib.check(lib.vsm_absorption_xsec_lin(*head, CR._ptr(h["qd"]), *tail, *[CR._ptr(o) for o in lin_outs],
                                                              CR._ptr(h["work"]), None))


def lut_call(m, dgrid, dp, dT, outs, lin):
    ax = [C.c_double(v) for r in (m.ν_grid, m.p_grid, m.t_grid) for v in (r.first, r.step)]
    args = [a.points, a.layers, m.ν_grid.n, m.p_grid.n, m.t_grid.n] + ax + [A._LUT_INTERP[m.interp_type], A._LUT_STORAGE[m.storage_type]] + \
        [CR._ptr(t) for t in (dev.lut_coef(m), dgrid, dp, dT, ones)] + [0] + [CR._ptr(o) for o in outs[:3 if lin else 1]] + [None]
    fn = lib.vsm_absorption_lut_eval_lin if lin else lib.vsm_absorption_lut_eval
    return lambda: vsm._lib.check(fn(*args))


# ---- the build: the states as the layers of one line-by-line call, then the prefilter ------------------------------------------------------
states = A._prepare(model, grid, np.repeat(pg.values(), a.nt), np.tile(tg.values(), a.np))
hs = dev.profile(states)
values = dev.empty(a.np * a.nt, a.points)
elems = int(lib.vsm_absorption_lut_work_elems(a.points, a.np, a.nt, 0))
work = torch.empty(elems, dtype=torch.float64, device=values.device)
coef = torch.empty((a.np + 2, a.nt + 2, a.points + 2), dtype=torch.float64, device=values.device)
build = measure({"xsec over the states": xsec_call(states, hs, values),
                 "prefilter": lambda: vsm._lib.check(lib.vsm_absorption_lut_prefilter(a.points, a.np, a.nt, CR._ptr(values), 0, CR._ptr(coef),
                                                                                      CR._ptr(work), None))}, max(1, a.reps // 20))
print("shape: %d lines, %d points, %d layers; table %d x %d states on the %d points, Voigt, HW32 SD, cutoff %g"
      % (states.n_lines, a.points, a.layers, a.np, a.nt, a.points, states.wing_cutoff))
for k, v in build.items():
    print("build, %-22s %s ms per call (min %.4f)" % (k + ":", " ".join("%.4f" % x for x in v), min(v)))
print("build: values %.1f MB, coefficients %.1f MB, prefilter work %.1f MB"
      % (values.numel() * 8 / 1e6, coef.numel() * 8 / 1e6, elems * 8 / 1e6))

# ---- forward and linearized profile calls -------------------------------------------------------------------------------------------------
models = {"cubic f64": A.InterpolationModel(7, 1, nu, pg, tg, "cubic", np.float64, arch, _coef_dev=coef)}
models["cubic f32"] = A.InterpolationModel(7, 1, nu, pg, tg, "cubic", np.float32, arch, _coef_dev=coef.to(torch.float32))
lin_values = values.reshape(a.np, a.nt, a.points)
models["linear f64"] = A.InterpolationModel(7, 1, nu, pg, tg, "linear", np.float64, arch, _coef_dev=lin_values)
models["linear f32"] = A.InterpolationModel(7, 1, nu, pg, tg, "linear", np.float32, arch, _coef_dev=lin_values.to(torch.float32))
job = A._prepare_lin(model, grid, p, T)
h = dev.profile_lin(job)
outs = [dev.empty(a.layers, a.points) for _ in range(4)]
louts = [dev.empty(a.layers, a.points) for _ in range(3)]
dgrid, dp, dT = dev.conv(grid), dev.conv(p), dev.conv(T)
calls = {"line-by-line": xsec_call(job, h, outs[0]), "line-by-line lin": xsec_call(job, h, outs[0], outs[1:])}
for k, m in models.items():
    calls["table " + k] = lut_call(m, dgrid, dp, dT, louts, False)
    calls["table " + k + " lin"] = lut_call(m, dgrid, dp, dT, louts, True)
times = measure(calls, a.reps)
best = {k: min(v) for k, v in times.items()}
for k, v in times.items():
    print("%-22s %s ms per call (min %.4f)" % (k + ":", " ".join("%.4f" % x for x in v), best[k]))
for k, m in models.items():
    rows, size = (16 if m.interp_type == "cubic" else 4), m.storage_type.itemsize
    for lin, planes in (("", 1), (" lin", 3)):
        t = best["table " + k + lin]
        byts = a.layers * a.points * (rows * size + planes * 8)
        print("table %-14s %.4f ms = %.3f of line-by-line%s; algorithmic traffic %.1f MB -> %.0f GB/s"
              % (k + lin + ":", t, t / best["line-by-line" + lin], lin, byts / 1e6, byts / t / 1e6))
    print("table %-14s lin / forward = %.3f" % (k + ":", best["table " + k + " lin"] / best["table " + k]))
print("line-by-line lin / forward = %.3f" % (best["line-by-line lin"] / best["line-by-line"]))
calls["table cubic f64"]()
calls["line-by-line"]()
torch.cuda.synchronize()
lbl, tab = outs[0].cpu().numpy(), louts[0].cpu().numpy()
print("table against line-by-line on this profile (the method's interpolation error at %d x %d states): max |difference| / max sigma = %.2e"
      % (a.np, a.nt, np.max(np.abs(tab - lbl)) / lbl.max()))
dev.fetch([])
