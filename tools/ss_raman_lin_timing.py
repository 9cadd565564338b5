#!/usr/bin/env python3
"""What the linearized Raman single-scattering column costs per Fourier moment: the device time of one
vsm_ss_column_rrs_lin_* call for P = 3 and P = 10 parameter slots (all of them layer slots here) beside the unchanged forward
vsm_ss_column_rrs_* call on the same inputs, at a C5-like shape: Stokes_IQU, three viewing angles (nine rows), three layers,
S = 10^4 spectral points, K = 101 lines (shifts -50 .. 50, all inside the staged window), FP64.

Every call uploads its small layer table and synchronises the stream before its launch, so a call is timed alone with a pair of
device events and the same call at S = 1 is printed beside it: the fixed cost of a call (upload, synchronise, an almost empty
launch), to be subtracted.  `--warmup` calls first, then the median of `--steps`.  Prints one JSON line; no threshold."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--lines", type=int, default=101)
ap.add_argument("--layers", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--fp32", action="store_true")
a = ap.parse_args()

sys.path.insert(0, os.path.abspath(a.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

arch = vsm.Architectures.GPU(0)
H, CR, SSd = vsm.host_model, vsm.CoreRT, vsm.core_rt_ss
FT = np.float32 if a.fp32 else np.float64
VZA, VAZ = [20.0, 35.0, 50.0], [0.0, 60.0, 120.0]
shifts = np.arange(a.lines) - a.lines // 2
w_ie = np.full(a.lines, 0.3 / a.lines)


def scene(S):
    L = a.layers
    rng = np.random.default_rng(0)
    tau_rayl = np.tile(np.linspace(0.02, 0.05, L), (S, 1))
    tau_abs = 10.0 ** rng.uniform(-2, 0.3, (S, 1)) * np.linspace(0.5, 1.5, L)[None, :] / L
    model = H.model_from_arrays(arch, "IQU", 7, 35.0, VZA, VAZ, float_type=FT, tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075,
                                albedo=0.3, m_max=2)
    return SSd.SceneSS(model, vsm.CoreRTRaman.RRS(shifts, w_ie, H.get_greek_rayleigh(6.0 / 7.0 * 0.5)))


def timed(f):
    for _ in range(a.warmup):
        f()
    t = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(t)


def arms(S):
    ss = scene(S)
    fwd, L, m = ss.fwd, ss.fwd.Nz, 0
    mom = fwd.moments[m]
    props = [ly["props"].materialize() for ly in mom["layers"]]
    tau, tau_sum = [p.tau for p in props], [ly["tau_sum"] for ly in mom["layers"]]
    fscatt = [ss.fscatt[iz] for iz in range(L)]
    row0, w = CR._vza_rows_weights(fwd.pol, ss.model.vza, ss.model.vaz, fwd.qp, m, float(CR.fourier_weight(FT, m)), ss.dt)
    nV, n = len(VZA), fwd.pol.n
    Zp, Zm = ss.Zie[m]
    out = {}
    ie = [torch.zeros((S, n, nV), dtype=ss.dt, device=fwd.dev) for _ in range(2)]
    out["forward"] = timed(lambda: SSd.ss_column_rrs_(fwd.dq, m, tau, tau_sum, fscatt, ss.drs.shift, ss.drs.varpi_ie, Zp, Zm, fwd.F0,
                                                      ss.halo, row0, w, nV, ie[0], ie[1]))
    for P in (3, 10):
        g = torch.Generator(device=fwd.dev).manual_seed(P)
        dots = [[torch.rand((P, S), dtype=ss.dt, device=fwd.dev, generator=g) * 0.1 for _ in range(L)] for _ in range(3)]
        d = [torch.zeros((P, S, n, nV), dtype=ss.dt, device=fwd.dev) for _ in range(2)]
        out["lin_P%d" % P] = timed(lambda: SSd.ss_column_rrs_lin_(fwd.dq, m, P, P, tau, tau_sum, fscatt, dots[0], dots[1], dots[2],
                                                                 ss.drs.shift, ss.drs.varpi_ie, Zp, Zm, fwd.F0, ss.halo, row0, w, nV,
                                                                 d[0], d[1]))
    return out


big, one = arms(a.points), arms(1)
vsm._lib.check_device_status("ss_raman_lin_timing")
r = lambda x: round(x * 1e6, 1)
print(json.dumps(dict(points=a.points, lines=a.lines, layers=a.layers, fp=32 if a.fp32 else 64,
                      call_us={k: r(v) for k, v in big.items()}, fixed_cost_us={k: r(v) for k, v in one.items()},
                      ratio_to_forward={k: round((big[k] - one[k]) / (big["forward"] - one["forward"]), 2) for k in big if k != "forward"},
                      build=vsm._lib.build_info().get("source_hash"))))
