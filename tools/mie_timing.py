#!/usr/bin/env python3
"""One Mie (NAI-2) problem at the reference's own test shape (test_mie_gpu.jl): LogNormal(0.3, 2.1), 1.3 - 0.001i, 0.55 um,
r_max = 30 um, nquad_radius = 2500 -> n_max = 381, n_mu = 761.
  device   vsm_mie_nai2 alone on device-resident inputs: device events around `--reps` back-to-back calls after a warm-up
  call     vsm.Scattering.compute_aerosol_optical_properties as a user calls it (host part, H2D, kernels, D2H), host clock
  host     the host part alone (dominated by the Gauss-Legendre nodes of the two quadratures)
  oracle   tests/mie_oracle.py's numpy restatement on the same inputs (`--oracle`; a CPU figure, for scale only)
Stage 2 forms 8 n_mu n_max nquad real products (two flop each); its kernel time comes from a `rocprofv3 --kernel-trace --stats`
run of `--arm device`, and the fraction of the 78.6 TFLOP/s FP64 MFMA peak printed here from `--stage2-ms`.
`--lin` times vsm_mie_nai2_lin (compute_aerosol_optical_properties_lin) instead: sixteen real products per (angle, order, radius)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["every", "device"], default="every")
ap.add_argument("--nquad", type=int, default=2500)
ap.add_argument("--r-max", type=float, default=30.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--group", type=int, default=32, help="radii per workgroup of k_mie_bulk (16 MIE_RT of csrc/vsm_mie.hip)")
ap.add_argument("--oracle", action="store_true")
ap.add_argument("--lin", action="store_true", help="the linearized call vsm_mie_nai2_lin")
ap.add_argument("--stage2-ms", type=float, default=None, help="k_mie_bulk's time per call from a kernel trace")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("mie_timing: no MI355X visible (there is nothing to time on a CPU)")
S = vsm.Scattering
arch = vsm.Architectures.GPU(0)
model = S.make_mie_model(S.Aerosol(S.LogNormal(0.3, 2.1), 1.3, 0.001), 0.55, a.r_max, a.nquad)
t0 = time.perf_counter()
if a.lin:
    h, wx_dot, wr_dot = S.mie_lin_host_inputs(model)
else:
    h = S.mie_host_inputs(model)
t_host = time.perf_counter() - t0
per = 16.0 if a.lin else 8.0                          # real products per (angle, order, radius)
products = per * h.n_mu * h.n_max * len(h.x)
print("shape: nquad %d  n_max %d  n_mu %d  stage-2 products %.3e (%.3e flop)" % (len(h.x), h.n_max, h.n_mu, products, 2 * products))
# what k_mie_bulk issues: 16-angle tiles x groups of `--group` radii, the k loop of a group ending at its largest n_max_i (in steps of 4)
nm = np.concatenate([h.nmax_i, np.zeros(-len(h.x) % 64, dtype=h.nmax_i.dtype)]).reshape(-1, a.group).max(axis=1)
issued = per * (-(-h.n_mu // 16) * 16) * a.group * float(np.sum(-(-nm // 4) * 4))
print("  issued on the MFMA (padding in, orders above a group's n_max_i out): %.3e products = %.3f of that" % (issued, issued / products))
print("host part: %.3f s (first call: the Gauss-Legendre nodes are kept per size afterwards)" % t_host)

conv = vsm.Architectures.array_type(arch)
dev = S.device_inputs(h, conv)
if a.lin:
    dev_dot = (conv(wx_dot), conv(wr_dot))
    launch = lambda: S.launch_nai2_lin(model, h, dev, dev_dot)
else:
    launch = lambda: S.launch_nai2(model, h, dev)
keep = launch()                                          # warm-up: code objects
torch.cuda.synchronize()
times = []
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        keep = launch()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / a.reps)
print("%s: " % ("vsm_mie_nai2_lin" if a.lin else "vsm_mie_nai2"), end="")
print("device: %s ms per call (%d calls per window, min %.4f ms)" % (" ".join("%.4f" % t for t in times), a.reps, min(times)))
print("  all five kernels over the stage-2 flop: %.2f TFLOP/s = %.3f of 78.6" % (2 * products / (min(times) * 1e-3) / 1e12,
                                                                               2 * products / (min(times) * 1e-3) / 78.6e12))
if a.stage2_ms:
    r = 2 * products / (a.stage2_ms * 1e-3)
    print("stage 2 (k_mie_bulk %.4f ms): %.2f TFLOP/s = %.3f of the 78.6 TFLOP/s FP64 MFMA peak by the 8 n_mu n_max nquad products; "
          "%.2f TFLOP/s = %.3f by the products issued" % (a.stage2_ms, r / 1e12, r / 78.6e12, r * issued / products / 1e12,
                                                       r * issued / products / 78.6e12))
if a.arm == "device":
    sys.exit(0)

call = (lambda: S.compute_aerosol_optical_properties_lin(model, arch)[0]) if a.lin else \
    (lambda: S.compute_aerosol_optical_properties(model, arch))
call()
calls = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt = call()[0]
    calls.append(time.perf_counter() - t0)
print("call: %s s (host part included)" % " ".join("%.3f" % t for t in calls))
print("  ssa %.12f  k %.9e  beta_0 - 1 %.2e" % (opt.ssa, opt.k, opt.greek_coefs.beta[0] - 1.0))

if a.oracle:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mie_oracle as MO  # noqa: E402
    t0 = time.perf_counter()
    greek, (c_sca, c_ext, ssa), _ = MO.nai2_reference(h.x, h.wx, h.wr, h.nmax_i, h.mu, h.w_mu, 1.3, 0.001, h.k_wave, h.n_max)
    t_or = time.perf_counter() - t0
    g = opt.greek_coefs
    d = max(float(np.max(np.abs(v - greek[i]))) for i, v in enumerate((g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta)))
    print("oracle (numpy, CPU, %d threads): %.2f s for the same inputs; max |d greek| %.2e  rel d ssa %.2e"
          % (torch.get_num_threads(), t_or, d, abs(opt.ssa - ssa) / ssa))
