#!/usr/bin/env python3
"""The continuum set call (vsm_absorption_continuum) at the shape of 4.25: `--points` grid points over 12 987 ..
13 175 cm^-1 and `--layers` layers from 1 to 1013 hPa, with a set of three CIA tables (nT = 15, 5, 1) and one MT_CKD band.  The method
of tools/absorption_lut_timing.py: everything is resident on the device (the library is called with device pointers, nothing is
uploaded inside a window), device events around `--reps` back-to-back calls, three windows after a warm-up, the calls alternating
in this one process.

    set          the forward and the linearized call on the whole set
    members      the same four members as four single-member sets called one after the other: what fusing saves
    table        vsm_absorption_lut_eval on a cubic FP64 table of 25 x 15 states (4.27), measured again in this process
    traffic      the algorithmic bytes of a set call -- per (point, layer) two rows of each table read and every plane written -- over
                 the measured time; the tables of a few layers stay in the Infinity Cache, so this is no HBM rate (the caveat of 4.27)"""
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
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("continuum_timing: no MI355X visible (there is nothing to time on a CPU)")
A, lib = vsm.Absorption, vsm._lib.lib()
arch = vsm.Architectures.GPU(0)
rng = np.random.default_rng(0)
grid = np.linspace(12987.0, 13175.0, a.points)
p = np.geomspace(1.0, 1013.0, a.layers)
T = np.linspace(200.0, 295.0, a.layers)
v_h2o = np.geomspace(4e-6, 0.02, a.layers)
dz = A.layer_thickness(np.geomspace(0.5, 1030.0, a.layers + 1), T, v_h2o)
vmr = {"H2O": v_h2o}
members = [A.CIATable.from_arrays(pair, np.linspace(190.0, 330.0, nT) if nT > 1 else [296.0], 10.0 ** rng.uniform(-47, -44, (a.points, nT)),
                                  grid, architecture=arch) for pair, nT in (("O2-O2", 15), ("O2-N2", 5), ("N2-N2", 1))]
nu_t = np.arange(-20.0, 20005.0, 10.0)
members.append(A.build_mtckd_band(A.MTCKDTable(nu_t, 10.0 ** rng.uniform(-28, -24, len(nu_t)), 10.0 ** rng.uniform(-30, -26, len(nu_t)),
                                               rng.uniform(0.0, 10.0, len(nu_t)), 1013.0, 296.0), grid, architecture=arch))
dev = A._Device(arch)


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


def set_call(ms, lin, accumulate, planes):
    """One entry-point call on the set `ms` with everything uploaded before: a closure over the argument list."""
    job = A._prepare_continuum(ms, grid, p, T, dz, vmr)
    nP = job.n_planes if lin else 1
    n, hp, hn, d, b = dev._continuum_args(job, nP)
    P = CR._ptr
    if not lin:
        args = [job.nSpec, job.Nz, n, hp, hn, P(d[0]), P(d[1]), P(d[2])] + [P(x) for x in b] + [accumulate, P(planes[0]), None]
        return (lambda: vsm._lib.check(lib.vsm_absorption_continuum(*args))), job
    pl = (C.c_void_p * nP)(*[t.data_ptr() for t in planes[:nP]])
    acc = (C.c_int * nP)(*([accumulate] * nP))
    h2o = 3 + job.species.index("H2O") if job.band is not None else -1
    args = [job.nSpec, job.Nz, n, hp, hn, P(d[0]), P(d[1]), nP, P(d[2]), P(d[3])] + [P(x) for x in b] + [h2o, nP - 1, acc, pl, None]
    return (lambda: vsm._lib.check(lib.vsm_absorption_continuum_lin(*args))), job


planes = [dev.empty(a.layers, a.points) for _ in range(A.CONT_MAX_PLANES)]
calls, jobs = {}, {}
for lin in (False, True):
    tag = " lin" if lin else ""
    calls["set" + tag], jobs["set" + tag] = set_call(members, lin, 0, planes)
    singles = [set_call([m], lin, 1 if i else 0, planes)[0] for i, m in enumerate(members)]
    calls["four single-member sets" + tag] = lambda singles=singles: [c() for c in singles]

# the cubic FP64 table call of 4.27 on the same grid and profile (its time does not depend on the coefficients' values)
nP_t, nT_t = 25, 15
nu_r = A.UniformRange(grid[0], (grid[-1] - grid[0]) / (a.points - 1), a.points)
pg, tg = A.UniformRange(1.0, 1012.0 / (nP_t - 1), nP_t), A.UniformRange(195.0, 105.0 / (nT_t - 1), nT_t)
coef = torch.rand((nP_t + 2, nT_t + 2, a.points + 2), dtype=torch.float64, device="cuda")
m = A.InterpolationModel(7, 1, nu_r, pg, tg, "cubic", np.float64, arch, _coef_dev=coef)
dgrid, dp, dT, ones = dev.conv(grid), dev.conv(p), dev.conv(T), dev.conv(np.ones(a.layers))
ax = [C.c_double(v) for r in (m.ν_grid, m.p_grid, m.t_grid) for v in (r.first, r.step)]
targs = [a.points, a.layers, m.ν_grid.n, m.p_grid.n, m.t_grid.n] + ax + [A._LUT_INTERP["cubic"], A._LUT_STORAGE[m.storage_type]] + \
    [CR._ptr(t) for t in (coef, dgrid, dp, dT, ones)] + [0, CR._ptr(planes[-1]), None]
calls["table cubic f64 (4.27)"] = lambda: vsm._lib.check(lib.vsm_absorption_lut_eval(*targs))

times = measure(calls, a.reps)
best = {k: min(v) for k, v in times.items()}
print("shape: %d points, %d layers; CIA tables nT = 15, 5, 1 and one MT_CKD band; %d layers per workgroup"
      % (a.points, a.layers, lib.vsm_absorption_continuum_layers()))
for k, v in times.items():
    print("%-32s %s ms per call (min %.4f)" % (k + ":", " ".join("%.4f" % x for x in v), best[k]))
for tag in ("", " lin"):
    job = jobs["set" + tag]
    nP = job.n_planes if tag else 1
    byts = a.layers * a.points * 8 * (2 * len(job.tables) + nP) + a.points * 8 * 4 * -(-a.layers // A.CONT_LAYERS)
    t = best["set" + tag]
    print("set%-5s %.4f ms = %.3f of four single-member sets; %d planes; algorithmic traffic %.1f MB -> %.0f GB/s (derived; the tables "
          "sit in the Infinity Cache)" % (tag + ":", t, t / best["four single-member sets" + tag], nP, byts / 1e6, byts / t / 1e6))
print("set lin / forward = %.3f; set / table cubic f64 = %.3f" % (best["set lin"] / best["set"], best["set"] / best["table cubic f64 (4.27)"]))
dev.fetch([])
