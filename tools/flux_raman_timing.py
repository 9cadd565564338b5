#!/usr/bin/env python3
"""What fluxes with rotational Raman scattering cost: ONE arm per process, on the m = 0 scene of the C5 shape of
tools/ms_raman_timing.py (Stokes_IQU, l_trunc 9: the Stokes_IQ sub-scene of m = 0 has N = 14; 12 layers, K = 40 Raman lines, FP64)
at 4000 points and all 13 levels, `--warmup` warm-up steps, then `--steps` steps timed with a host clock around a device
synchronise; prints one JSON line with the steps and their median.

  --arm ms              rt_run_multisensor(RS_type, model at m_max = 0, all levels, streams=True) and the numpy quadrature of its
                        level vectors: what a user did before CoreRTRaman.rt_run_fluxes (a tree without it can run this arm)
  --arm flux            CoreRTRaman.rt_run_fluxes(RS_type, model); with --split also the device time between events recorded around
                        its level calls (the elastic call and vsm_level_flux_ie_*), as sums over the levels
  --arm level_composed  ONE level on synthetic operands of that shape, composed of existing kernels: vsm_level_radiance_ie_* with
                        full vectors and no viewing row, four torch products with the weight rows (elastic and inelastic, up and
                        down) and the direct beam in torch (a tree without the fused kernel can run this arm)
  --arm level_fused     the same level as ONE vsm_level_flux_ie_* call

`--root DIR` imports the package of another checkout (the parent commit, built in its own tree), so that both trees are measured
by the same script in one session; alternate the processes of the arms."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["ms", "flux", "level_composed", "level_fused"], required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--points", type=int, default=4000)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--lines", type=int, default=40)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=50, help="level calls per step of the level_* arms")
ap.add_argument("--split", action="store_true")
ap.add_argument("--tag", default="")
a = ap.parse_args()

sys.path.insert(0, os.path.abspath(a.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vsmartmom_jl_amd as vsm  # noqa: E402

arch = vsm.Architectures.GPU(0)
S, L, K = a.points, a.layers, a.lines
H = vsm.host_model
rng = np.random.default_rng(20260929)
dp = np.full(L, 1.0 / L)
tau_rayl = np.tile(0.3 * dp, (S, 1))
tau_abs = (10.0 ** rng.uniform(-4, 0, (S, 1))) * dp[None, :]
model = H.model_from_arrays(arch, "IQU", 9, 40.0, [30.0], [0.0], tau_rayl=tau_rayl, tau_abs=tau_abs, depol=0.0075, albedo=0.05,
                            m_max=2)
model.varpi_Cabannes = 0.96
shifts = np.unique(np.concatenate([np.arange(-K // 2, 0), np.arange(1, K - K // 2 + 1)]) * 7)
rs = vsm.CoreRTRaman.RRS(shifts, np.full(len(shifts), 0.04 / len(shifts)), H.get_greek_rayleigh(0.75))
levels = list(range(L + 1))
extra = {}


def quadrature_of_streams():
    """The fluxes by hand: every level with streams=True at m_max = 0, the vectors of Stokes I, the mu w quadrature."""
    res = vsm.CoreRTRaman.rt_run_multisensor(rs, dataclasses.replace(model, m_max=0), levels, streams=True)
    qp, n = model.quad_points, res.pol_n
    mu, w = np.asarray(qp.qp_mu, dtype=np.float64), np.asarray(qp.wt_mu, dtype=np.float64)
    tau = np.concatenate([np.zeros((S, 1)), np.cumsum(tau_rayl + tau_abs, axis=1)], axis=1)      # (Rayleigh: no delta-M scaling)
    out = {}
    for i, l in enumerate(levels):
        down = 0.0 if l == 0 else 1.0
        row = []
        for us, ds in ((res.uw_streams, res.dw_streams), (res.uwie_streams, res.dwie_streams)):
            uw, dw = us[i][0][::n, 0, :], ds[i][0][::n, 0, :] * down
            row += [(mu * w) @ uw, (mu * w) @ dw, w @ uw, w @ dw]
        beam = np.exp(-tau[:, l] / res.mu0)
        out[l] = row + [res.mu0 * beam, beam]
    return out


def flux_run():
    if not a.split:
        return vsm.CoreRTRaman.rt_run_fluxes(rs, model)
    FXR, MS = vsm.core_rt_flux_raman, vsm.core_rt_ms
    marks = {"level_flux_ie_": [], "level_radiance_": []}
    orig = {"level_flux_ie_": FXR.level_flux_ie_, "level_radiance_": MS.level_radiance_}

    def wrap(name):
        def g(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig[name](*args, **kw)
            e1.record()
            marks[name].append((e0, e1))
        return g
    FXR.level_flux_ie_, MS.level_radiance_ = wrap("level_flux_ie_"), wrap("level_radiance_")
    try:
        res = vsm.CoreRTRaman.rt_run_fluxes(rs, model)
    finally:
        FXR.level_flux_ie_, MS.level_radiance_ = orig["level_flux_ie_"], orig["level_radiance_"]
    torch.cuda.synchronize()
    for name, ev in marks.items():
        extra.setdefault(name + "calls", len(ev))
        extra.setdefault(name + "device_s", []).append(round(sum(e0.elapsed_time(e1) for e0, e1 in ev) / 1e3, 5))
    return res


def level_arm(fused):
    """One level at the shape of the m = 0 sub-scene: N = 2 Nquad, n = 2, contractive random operators."""
    Nq, n = model.quad_points.Nquad, 2
    N = n * Nq
    dev, dt = torch.device("cuda", 0), torch.float64
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rnd = lambda *sh: torch.rand(sh, dtype=dt, device=dev, generator=g)
    A, B = 0.5 * rnd(S, N, N) / N, 0.5 * rnd(S, N, N) / N
    dwf, uwf = rnd(S, N), rnd(S, N)
    Aie, Bie = 0.05 * rnd(K, S, N, N) / N, 0.05 * rnd(K, S, N, N) / N
    aie, cie = 0.05 * rnd(K, S, N), 0.05 * rnd(K, S, N)
    q, tau, F0 = rnd(2, Nq), 2 * rnd(S), 0.5 + rnd(S)
    sh = torch.as_tensor(np.asarray(shifts, dtype=np.int32), device=dev)
    pol = H.polarization_type("IQ")
    mu0, dir_h = 0.7, (0.7, 1.0)
    out = torch.empty((5, 2, S), dtype=dt, device=dev)
    if fused:
        FXR = vsm.core_rt_flux_raman
        return lambda: [FXR.level_flux_ie_(pol, sh, A, B, dwf, uwf, Aie, aie, Bie, cie, q, dir_h, mu0, tau, F0, out)
                        for _ in range(a.calls)]
    MSR = vsm.core_rt_ms_raman
    qT = q.t().contiguous()
    dh = torch.as_tensor(dir_h, dtype=dt, device=dev)

    def composed():
        for _ in range(a.calls):
            dwie, uwie = torch.empty((S, N), dtype=dt, device=dev), torch.empty((S, N), dtype=dt, device=dev)
            MSR.level_radiance_ie_(pol, None, [], [], 0, 1.0, sh, A, B, dwf, uwf, Aie, aie, Bie, cie, None, None, dwie, uwie)
            out[0].copy_((uwf[:, ::n] @ qT).t())
            out[1].copy_((dwf[:, ::n] @ qT).t())
            out[3].copy_((uwie[:, ::n] @ qT).t())
            out[4].copy_((dwie[:, ::n] @ qT).t())
            out[2].copy_(dh[:, None] * (F0 * torch.exp(-tau / mu0))[None, :])
    return composed


arms = {"ms": quadrature_of_streams, "flux": flux_run}
f = arms[a.arm] if a.arm in arms else level_arm(a.arm == "level_fused")
for _ in range(a.warmup):
    f()
extra.clear()
t = []
for _ in range(a.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    t.append(time.perf_counter() - t0)
vsm._lib.check_device_status("flux_raman_timing")
print(json.dumps(dict(arm=a.arm, tag=a.tag, points=S, layers=L, lines=len(shifts), steps_s=[round(x, 5) for x in t],
                      median_s=round(statistics.median(t), 5), **extra,
                      **({"calls_per_step": a.calls} if a.arm.startswith("level_") else {}),
                      build=vsm._lib.build_info().get("source_hash"))))
