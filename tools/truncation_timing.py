#!/usr/bin/env python3
"""delta-BGE truncation behind one Mie (NAI-2) problem at the shape of tools/mie_timing.py: LogNormal(0.3, 2.1), 1.3 - 0.001i,
0.55 um, r_max = 30 um, nquad_radius = 2500 -> n_max = 381, n_mu = 761, at each `--l-max` (20 and 64).
  mie           vsm_mie_nai2 alone on device-resident inputs
  mie + bulk    the Mie call and vsm_truncate_dbge on its device arrays greek, bulk_f, scal: what the truncation= keyword enqueues
  reconstruct   vsm_truncate_dbge alone, f11, f12, f34 rebuilt from the 761 coefficients
  bulk          vsm_truncate_dbge alone on bulk_f and scal
each with device events around `--reps` back-to-back calls, three windows after a warm-up;
  call          compute_aerosol_optical_properties(model, arch, truncation=DeltaBGE(l_max)) as a user calls it, host clock
  host fit      what a caller had before: the untruncated call's D2H, then tests/truncation_oracle.py's numpy fit (a CPU figure, for
                scale only)
--lin: the linearized chain at the same shape, the same windows:
  mie lin            vsm_mie_nai2_lin alone
  mie lin + bulk     the linearized Mie call and vsm_truncate_dbge_lin on its device arrays: what
                     compute_truncated_aerosol_optical_properties_lin enqueues
  lin reconstruct    vsm_truncate_dbge_lin alone, f and f' rebuilt from the 761 coefficients and their derivatives
  lin bulk           vsm_truncate_dbge_lin alone on bulk_f, scal, bulk_f_dot, scal_dot
  fwd bulk           vsm_truncate_dbge alone, for the ratio
  8 x (mie + bulk)   what the call replaces: eight forward Mie + truncation calls for central differences"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402
import truncation_oracle as TO  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nquad", type=int, default=2500)
ap.add_argument("--r-max", type=float, default=30.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--l-max", type=int, nargs="+", default=[20, 64])
ap.add_argument("--lin", action="store_true")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("truncation_timing: no MI355X visible (there is nothing to time on a CPU)")
S = vsm.Scattering
arch = vsm.Architectures.GPU(0)
model = S.make_mie_model(S.Aerosol(S.LogNormal(0.3, 2.1), 1.3, 0.001), 0.55, a.r_max, a.nquad)
h = S.mie_host_inputs(model)
dev = S.device_inputs(h, vsm.Architectures.array_type(arch))
print("shape: nquad %d  n_max %d  n_mu %d" % (len(h.x), h.n_max, h.n_mu))


def windows(enqueue):
    keep = enqueue()                                     # warm-up: code objects
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            keep = enqueue()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / a.reps)
    del keep
    return out


def line(what, t):
    print("%-22s %s ms per call (%d calls per window, min %.4f ms)" % (what, " ".join("%.4f" % v for v in t), a.reps, min(t)))
    return min(t)


def lin_timing():
    conv = vsm.Architectures.array_type(arch)
    _, wx_dot, wr_dot = S.mie_lin_host_inputs(model)
    dev_dot = (conv(wx_dot), conv(wr_dot))
    run = S.launch_nai2_lin(model, h, dev, dev_dot)
    g, b, s, gd, bd, sd = run[:6]
    torch.cuda.synchronize()
    line("mie", windows(lambda: S.launch_nai2(model, h, dev)))
    t_lin = line("mie lin", windows(lambda: S.launch_nai2_lin(model, h, dev, dev_dot)))
    for l_max in a.l_max:
        print("l_max = %d" % l_max)

        def both_lin():
            r = S.launch_nai2_lin(model, h, dev, dev_dot)
            return r, S.launch_dbge_lin(h.n_mu, l_max, *r[:6], dev[4], dev[5])

        def both():
            r = S.launch_nai2(model, h, dev)
            return r, S.launch_dbge(h.n_mu, l_max, 0, 1.0, r[0], r[1], r[2], dev[4], dev[5])

        t_both = line("  mie lin + bulk", windows(both_lin))
        line("  lin reconstruct", windows(lambda: S.launch_dbge_lin(h.n_mu, l_max, g, None, None, gd, None, None, dev[4], dev[5])))
        t_lb = line("  lin bulk", windows(lambda: S.launch_dbge_lin(h.n_mu, l_max, g, b, s, gd, bd, sd, dev[4], dev[5])))
        t_fb = line("  fwd bulk", windows(lambda: S.launch_dbge(h.n_mu, l_max, 0, 1.0, g, b, s, dev[4], dev[5])))
        t_fd = line("  mie + bulk", windows(both))
        print("  the linearized truncation adds %.4f ms to the %.4f ms linearized Mie call; alone it is %.2f x the forward fit; "
              "8 x (mie + bulk) = %.4f ms against %.4f ms" % (t_both - t_lin, t_lin, t_lb / t_fb, 8 * t_fd, t_both))
        (opt, lin), = S.compute_truncated_aerosol_optical_properties_lin(model, S.DeltaBGE(l_max), arch)
        print("  c0 %.9f  f_trunc_dot %s  info %r" % (opt.c0, " ".join("%.6f" % v for v in lin.f_trunc_dot), opt.info))


if a.lin:
    lin_timing()
    sys.exit(0)
greek, bulk_f, scal, _work = S.launch_nai2(model, h, dev)
torch.cuda.synchronize()
t_mie = line("mie", windows(lambda: S.launch_nai2(model, h, dev)))
untruncated, = S.compute_aerosol_optical_properties(model, arch)
for l_max in a.l_max:
    print("l_max = %d" % l_max)

    def both():
        g, b, s, w = S.launch_nai2(model, h, dev)
        return w, S.launch_dbge(h.n_mu, l_max, 0, 1.0, g, b, s, dev[4], dev[5])

    t_both = line("  mie + bulk", windows(both))
    line("  reconstruct", windows(lambda: S.launch_dbge(h.n_mu, l_max, 0, 1.0, greek, None, None, dev[4], dev[5])))
    line("  bulk", windows(lambda: S.launch_dbge(h.n_mu, l_max, 0, 1.0, greek, bulk_f, scal, dev[4], dev[5])))
    print("  the truncation adds %.4f ms to the %.4f ms Mie call" % (t_both - t_mie, t_mie))
    method = S.DeltaBGE(l_max)
    S.compute_aerosol_optical_properties(model, arch, truncation=method)
    calls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt, = S.compute_aerosol_optical_properties(model, arch, truncation=method)
        calls.append(time.perf_counter() - t0)
    print("  call: %s s (host part included)  c0 %.9f  info %r" % (" ".join("%.4f" % t for t in calls), opt.c0, opt.info))
    g = untruncated.greek_coefs
    g_in = np.stack([g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta])
    f = tuple(untruncated.bulk_f[i] / untruncated.C_sca for i in (0, 2, 3))
    t0 = time.perf_counter()
    g_ref, c0_ref, _ = TO.truncate_phase(g_in, l_max, f)
    t_or = time.perf_counter() - t0
    t = opt.greek_coefs
    d = np.max(np.abs(np.stack([t.alpha, t.beta, t.gamma, t.delta, t.epsilon, t.zeta]) - g_ref))
    print("  host fit (numpy, CPU, %d threads): %.4f s on the same input; max |d greek| %.2e  rel d c0 %.2e"
          % (torch.get_num_threads(), t_or, d, abs(opt.c0 - c0_ref) / c0_ref))
