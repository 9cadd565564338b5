"""Scattering: Mie aerosol optics by the Siewert NAI-2 method (src/Scattering/types.jl, make_mie_model.jl, compute_NAI2.jl) on the
MI355X, through vsm_mie_nai2 (vsmartmom.jl_amd/csrc/vsm_mie.hip).

    aerosol = Scattering.Aerosol(Scattering.LogNormal(0.3, 2.1), 1.3, 0.001)          # r_m, sigma_g [um]; n_r - i n_i
    model   = Scattering.make_mie_model(aerosol, 0.55, r_max=30.0, nquad_radius=2500)   # wavelength, r_max in the radius' unit
    optics, = Scattering.compute_aerosol_optical_properties(model, vsm.Architectures.GPU())
    host_model.model_from_arrays(..., tau_aer=..., aerosol_optics=[optics])

The host computes what is small (compute_NAI2.jl:80-100, :113, :161): r_min = max(quantile(1e-8), 1e-6 r_max), the gauleg_log
nodes and weights, compute_w_x normalised to sum 1, x = 2 pi r / lambda, n_max_i = get_n_max(x_i), n_max, n_mu = 2 n_max - 1, the
Gauss-Legendre nodes in mu, wr_i = 4 pi r_i^2 wx_i.  Everything with an n_max, n_mu or nquad loop -- D_n, a_n, b_n, S1, S2, the
bulk functions, the Greek coefficients -- runs on the device in FP64 (the reference forces Float64 there too).  There is no CPU
path: Architectures.CPU() raises.

The result is a host_model.AerosolOptics with the reference's k (= the bulk extinction cross-section, in the squared unit of the
radii) and the bulk C_ext / C_sca beside it.  Its f_trunc is 0: the coefficients are untruncated, and 0 is what this package's
delta-M scaling (host_model.createAero) needs for them.  The reference stores f_trunc = 1 there and relies on a later
truncate_phase.

n_max = max(get_n_max(x_max), 2): the reference's compute_mie_pi_tau and compute_legendre_poly write two columns unconditionally,
so it cannot run a distribution whose largest x gives n_max = 1 (x < 0.0019); two orders (three coefficients) is the least here.

delta-BGE truncation (src/Scattering/truncate_phase.jl) through vsm_truncate_dbge (csrc/vsm_truncate.hip): a coarse-mode aerosol
has hundreds of coefficients, a run keeps l_trunc of them, and the forward peak that the cut removes belongs into f_trunc.

    optics, = Scattering.compute_aerosol_optical_properties(model, arch, truncation=Scattering.DeltaBGE(20, 2.0))
    optics  = Scattering.truncate_phase(Scattering.DeltaBGE(20), any_aerosol_optics, arch)     # Mie, Henyey-Greenstein, hand-made

truncate_phase is the variant the reference applies to Mie optics (all nodes, weights w / f^2; delta_angle is carried and not
read), truncate_phase_lowconf the one it applies to analytic phase functions (the nodes outside the forward cone).  A gamma or
epsilon series of exact zeros from l = 2 on -- every scalar phase function -- stays exact zeros; the reference divides by
f12 = 0 there and returns NaN.

Linearized Mie (compute_NAI2_lin.jl, mie_helper_functions_lin.jl) through vsm_mie_nai2_lin: the same optics and, in the same
call, their derivatives with respect to (n_r, n_i, mu, sigma), mu = ln r_m and sigma = ln sigma_g being the parameters of the
reference's LogNormal(log r_m, log sigma_g), as a host_model.LinAerosolOptics that LinModel takes as it is.

    (optics, lin_optics), = Scattering.compute_aerosol_optical_properties_lin(model, arch)
    host_model.LinModel(tau_abs_dot, tau_aer_dot=..., lin_aerosol_optics=[lin_optics])

The host adds the derivatives of the weights at fixed nodes (mie_lin_host_inputs); they deviate from the reference's on purpose
(the reference normalises wx before it differentiates the normalisation and loses a factor 1 / sum).

Linearized truncation (truncate_phase_lin.jl) through vsm_truncate_dbge_lin: the truncated coefficients, f_trunc = 1 - c0 and
their derivatives in one call, for an aerosol whose series does not fit into l_trunc.

    (optics, lin_optics), = Scattering.compute_truncated_aerosol_optical_properties_lin(model, Scattering.DeltaBGE(20), arch)
    optics, lin_optics    = Scattering.truncate_phase_lin(Scattering.DeltaBGE(20), any_optics, any_lin_optics, arch)

Not built: the linearized low-confidence variant (the reference has none), l_max above 128, PCW, the YAML `scattering:` block
(io_yaml keeps refusing it).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import statistics
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import host_model as H
from . import core_rt as CR
from .architectures import array_type, default_architecture, synchronize_if_gpu, to_host

MAX_N_MAX = 1024      # VSM_MIE_MAX_NMAX of the library: the largest n_max the kernels take (x = 500 needs 542)
MAX_DBGE_L = 128      # VSM_DBGE_MAX_L of the library: the largest l_max the truncation's solve keeps in LDS


# ---- types.jl ------------------------------------------------------------------------------------------------------------
class LogNormal:
    """LogNormal(r_m, sigma_g): median radius and geometric standard deviation -- the reference's
    LogNormal(log(r_m), log(sigma_g)) of Distributions.jl."""

    def __init__(self, r_m: float, sigma_g: float):
        if not (r_m > 0 and sigma_g > 1):
            raise _lib.VSMError("LogNormal needs r_m > 0 and sigma_g > 1 (got %r, %r)" % (r_m, sigma_g))
        self.r_m, self.sigma_g = float(r_m), float(sigma_g)
        self.mu, self.sigma = math.log(r_m), math.log(sigma_g)

    def pdf(self, r):
        r = np.asarray(r, dtype=np.float64)
        z = (np.log(r) - self.mu) / self.sigma
        return np.exp(-0.5 * z * z) / (r * self.sigma * math.sqrt(2 * math.pi))

    def quantile(self, p: float) -> float:
        return math.exp(self.mu + self.sigma * statistics.NormalDist().inv_cdf(p))

    def __repr__(self):
        return "LogNormal(%r, %r)" % (self.r_m, self.sigma_g)


class TabulatedSizeDistribution:
    """Any other size distribution (gamma, bimodal, measured): radius nodes r [nquad] and the unnormalised weights pdf(r_i) w_r,i
    of the caller's own quadrature.  The nodes are used as they are; r_max and nquad_radius of the model are not read.
    weights_dot [2, nquad] (optional, read by compute_aerosol_optical_properties_lin only): the derivatives of these unnormalised
    weights with respect to two parameters of the caller's own choosing, which take slots 2 and 3; without it those slots are
    exact zeros."""

    def __init__(self, r: Sequence[float], weights: Sequence[float], weights_dot=None):
        self.r = np.array(r, dtype=np.float64).reshape(-1)
        self.weights = np.array(weights, dtype=np.float64).reshape(-1)
        if self.r.shape != self.weights.shape:
            raise _lib.VSMError("TabulatedSizeDistribution: %d radii, %d weights" % (len(self.r), len(self.weights)))
        self.weights_dot = None
        if weights_dot is not None:
            self.weights_dot = np.array(weights_dot, dtype=np.float64)
            if self.weights_dot.shape != (2, len(self.r)):
                raise _lib.VSMError("TabulatedSizeDistribution: weights_dot of shape %r, not (2, %d)"
                                    % (self.weights_dot.shape, len(self.r)))


@dataclass
class Aerosol:
    """Aerosol(size_distribution, n_r, n_i) (types.jl): refractive index n_r - i n_i, n_i >= 0."""
    size_distribution: object
    n_r: float
    n_i: float


@dataclass
class MieModel:
    aerosol: Aerosol
    wavelength: float
    r_max: Optional[float]
    nquad_radius: Optional[int]


def make_mie_model(aerosol: Aerosol, wavelength: float, r_max: Optional[float] = None, nquad_radius: Optional[int] = None) -> MieModel:
    """make_mie_model(NAI2(), aerosol, wavelength, ., ., r_max, nquad_radius) (make_mie_model.jl:24-32); wavelength, r_max and the
    distribution's radii in one unit.  A TabulatedSizeDistribution brings its own nodes: r_max and nquad_radius may be omitted."""
    return MieModel(aerosol, float(wavelength), r_max, nquad_radius)


@dataclass
class MieHostInputs:
    """What the host hands the device: the inputs of vsm_mie_nai2."""
    r: np.ndarray
    wx: np.ndarray
    wr: np.ndarray
    x: np.ndarray
    nmax_i: np.ndarray
    n_max: int
    n_mu: int
    mu: np.ndarray
    w_mu: np.ndarray
    k_wave: float


@dataclass
class MieAerosolOptics(H.AerosolOptics):
    """host_model.AerosolOptics plus the reference's k and the bulk cross-sections (squared unit of the radii); mu and bulk_f
    [4, n_mu] are the angle nodes and the bulk f11, f33, f12, f34 there, before the division by C_sca."""
    k: float = 0.0
    C_ext: float = 0.0
    C_sca: float = 0.0
    mu: Optional[np.ndarray] = None
    bulk_f: Optional[np.ndarray] = None


@dataclass
class MieLinAerosolOptics(H.LinAerosolOptics):
    """host_model.LinAerosolOptics from linearized Mie.  Slot order (n_r, n_i, mu, sigma) with mu = ln r_m, sigma = ln sigma_g --
    what the reference differentiates (compute_w_x(lin, .) forms d / d mu and d / d sigma of LogNormal(mu, sigma)); d / d r_m is
    slot 2 divided by r_m.  For a TabulatedSizeDistribution slots 2 and 3 are the two parameters of its weights_dot.
    f_trunc_dot is exact zeros (f_trunc is 0 here).  k_dot, C_ext_dot, C_sca_dot [4]: derivatives of the bulk cross-sections
    (k = C_ext); bulk_f_dot [4, 4, n_mu]: derivatives of the unnormalised bulk f11, f33, f12, f34 at the angle nodes."""
    k_dot: Optional[np.ndarray] = None
    C_ext_dot: Optional[np.ndarray] = None
    C_sca_dot: Optional[np.ndarray] = None
    bulk_f_dot: Optional[np.ndarray] = None


# ---- mie_helper_functions.jl: the host part -------------------------------------------------------------------------------------
def get_n_max(size_parameter: float) -> int:
    """mie_helper_functions.jl:22 (Sanghavi 2014 eq. 6); round to nearest, ties to even, as Julia's round(Int, .)."""
    x = float(size_parameter)
    if x > 8.0:
        return int(round(x + 4.05 * x ** (1 / 3) + 10))
    return int(round(x + 4.0 * x ** (1 / 3) + 1))


@functools.lru_cache(maxsize=16)
def gausslegendre(n: int):
    """Gauss-Legendre nodes and weights on (-1, 1), kept per n (read-only arrays): at nquad_radius = 2500 they are nearly all of
    the host part's time, and a retrieval asks for the same two sizes per band, aerosol and iteration."""
    xi, w = np.polynomial.legendre.leggauss(int(n))
    xi.flags.writeable = False
    w.flags.writeable = False
    return xi, w


def gauleg_log(n: int, r_min: float, r_max: float):
    """gauleg_log(n, r_min, r_max; norm = false) (mie_helper_functions.jl:369-379): Gauss-Legendre nodes in ln r."""
    xi, w = gausslegendre(n)
    ln_min, ln_max = math.log(r_min), math.log(r_max)
    r = np.exp((ln_max - ln_min) / 2 * xi + (ln_max + ln_min) / 2)
    return r, w * r * (ln_max - ln_min) / 2


def compute_wx(size_distribution, w_r, r):
    """compute_w_x (mie_helper_functions.jl:511-521)."""
    wx = size_distribution.pdf(r) * w_r
    return wx / np.sum(wx)


def weight_derivatives(r, raw, raw_dot):
    """wx_dot, wr_dot [2, nquad] at fixed nodes from the unnormalised weights raw_i = pdf(r_i) w_r,i and their derivatives
    raw_dot [2, nquad]: with S = sum raw and wx = raw / S,  wx_dot = (raw_dot - (sum raw_dot) wx) / S,  wr_dot = 4 pi r^2 wx_dot.
    (The reference divides by sum(wx) = 1 where S belongs: DESIGN.md 6.)"""
    total = np.sum(raw)
    wx = raw / total
    wx_dot = np.stack([(raw_dot[k] - np.sum(raw_dot[k]) * wx) / total for k in range(2)])
    return wx_dot, 4 * math.pi * r ** 2 * wx_dot


def lognormal_raw_dot(sd: LogNormal, r, raw):
    """d raw / d mu = (ln r - mu) / sigma^2 raw,  d raw / d sigma = ((ln r - mu)^2 / sigma^3 - 1 / sigma) raw."""
    d = np.log(r) - sd.mu
    return np.stack([d / sd.sigma ** 2 * raw, (d ** 2 / sd.sigma ** 3 - 1 / sd.sigma) * raw])


def mie_lin_host_inputs(model: MieModel):
    """mie_host_inputs plus (wx_dot, wr_dot) [2, nquad]: the weights' derivatives with respect to (mu, sigma) of a LogNormal, with
    respect to the two parameters of weights_dot of a TabulatedSizeDistribution (exact zeros without it)."""
    h = mie_host_inputs(model)
    sd = model.aerosol.size_distribution
    if isinstance(sd, TabulatedSizeDistribution):
        if sd.weights_dot is None:
            return h, np.zeros((2, len(h.r))), np.zeros((2, len(h.r)))
        raw, raw_dot = sd.weights, sd.weights_dot
    else:
        _, w_r = gauleg_log(int(model.nquad_radius), max(sd.quantile(1e-8), 1e-6 * model.r_max), float(model.r_max))
        raw = sd.pdf(h.r) * w_r
        raw_dot = lognormal_raw_dot(sd, h.r, raw)
    return (h,) + weight_derivatives(h.r, raw, raw_dot)


def mie_host_inputs(model: MieModel) -> MieHostInputs:
    """compute_NAI2.jl:72-100, :113, :161, with the refusals of this backend (VSMError)."""
    aer = model.aerosol
    sd = aer.size_distribution
    if not (aer.n_i >= 0):
        raise _lib.VSMError("Aerosol: n_i = %r < 0 (the refractive index is n_r - i n_i with n_i >= 0)" % (aer.n_i,))
    if not (aer.n_r > 0 and model.wavelength > 0):
        raise _lib.VSMError("Aerosol: n_r = %r and the wavelength %r must be positive" % (aer.n_r, model.wavelength))
    if isinstance(sd, TabulatedSizeDistribution):
        if len(sd.r) < 1:
            raise _lib.VSMError("TabulatedSizeDistribution: nquad_radius = 0 < 1")
        total = float(np.sum(sd.weights))
        if not (np.all(sd.r > 0) and np.all(np.isfinite(sd.r)) and np.all(sd.weights >= 0) and 0 < total < math.inf):
            raise _lib.VSMError("TabulatedSizeDistribution: radii must be positive, weights non-negative with a positive sum")
        r, wx = sd.r.copy(), sd.weights / total
    else:
        if model.nquad_radius is None or int(model.nquad_radius) < 1:
            raise _lib.VSMError("nquad_radius = %r < 1" % (model.nquad_radius,))
        if model.r_max is None or not math.isfinite(model.r_max):
            raise _lib.VSMError("r_max = %r: a finite largest radius is needed" % (model.r_max,))
        r_min = max(sd.quantile(1e-8), 1e-6 * model.r_max)
        if not (model.r_max > r_min):
            raise _lib.VSMError("r_max = %r <= r_min = %r = max(quantile(1e-8), 1e-6 r_max)" % (model.r_max, r_min))
        r, w_r = gauleg_log(int(model.nquad_radius), r_min, float(model.r_max))
        wx = compute_wx(sd, w_r, r)
    k_wave = 2 * math.pi / model.wavelength
    x = k_wave * r
    nmax_i = np.array([get_n_max(v) for v in x], dtype=np.int32)
    n_max = max(get_n_max(np.max(x)), 2)
    if n_max > MAX_N_MAX:
        raise _lib.VSMError("n_max = %d (largest size parameter %.1f) above the %d orders the Mie kernels take "
                            "(VSM_MIE_MAX_NMAX)" % (n_max, float(np.max(x)), MAX_N_MAX))
    n_mu = 2 * n_max - 1
    mu, w_mu = gausslegendre(n_mu)
    wr = 4 * math.pi * r ** 2 * wx
    return MieHostInputs(r, wx, wr, x, nmax_i, n_max, n_mu, mu, w_mu, k_wave)


# ---- compute_NAI2.jl: the driver ------------------------------------------------------------------------------------------------
def device_inputs(h: MieHostInputs, conv):
    """The six device arrays of vsm_mie_nai2, in its argument order."""
    return [conv(a) for a in (h.x, h.nmax_i, h.wx, h.wr, h.mu, h.w_mu)]


def launch_nai2(model: MieModel, h: MieHostInputs, dev):
    """Enqueues vsm_mie_nai2 on the current stream: (greek [6, n_mu], bulk_f [4, n_mu], scal [3], work) device tensors.  Nothing is
    synchronised; the inputs and the work buffer must outlive the work."""
    nq, like = len(h.x), dev[0]
    greek = torch.empty((6, h.n_mu), dtype=torch.float64, device=like.device)
    bulk_f = torch.empty((4, h.n_mu), dtype=torch.float64, device=like.device)
    scal = torch.empty(3, dtype=torch.float64, device=like.device)
    elems = int(_lib.lib().vsm_mie_work_elems(nq, h.n_max, h.n_mu))
    if elems == 0:
        raise _lib.VSMError("vsm_mie_work_elems refuses nquad = %d, n_max = %d, n_mu = %d" % (nq, h.n_max, h.n_mu))
    work = _lib.poison(torch.empty(elems, dtype=torch.float64, device=like.device))
    _lib.check(_lib.lib().vsm_mie_nai2(nq, h.n_max, h.n_mu, C.c_double(model.aerosol.n_r), C.c_double(model.aerosol.n_i),
                                       C.c_double(h.k_wave), *[CR._ptr(t) for t in dev], CR._ptr(greek), CR._ptr(bulk_f),
                                       CR._ptr(scal), CR._ptr(work), CR._stream_ptr()))
    return greek, bulk_f, scal, work


def compute_aerosol_optical_properties(model_or_list, architecture=None, truncation=None):
    """compute_aerosol_optical_properties(model) (compute_NAI2.jl:63-217) for one MieModel or a list of them: a list with one
    MieAerosolOptics per model (greek_coefs, ssa, f_trunc = 0 -- see the module's docstring --, k, C_ext, C_sca).  All models are
    enqueued on the current stream before the one synchronisation that brings the results back.

    truncation = DeltaBGE(l_max, .): each model's vsm_truncate_dbge is enqueued directly behind its vsm_mie_nai2, on the device
    arrays greek, bulk_f and scal (truncate_phase, the variant the reference applies to Mie optics), and the list holds
    TruncatedAerosolOptics whose `untruncated` is the MieAerosolOptics.  NoTruncation() wraps without a fit."""
    models = [model_or_list] if isinstance(model_or_list, MieModel) else list(model_or_list)
    arch = architecture if architecture is not None else default_architecture()
    CR._require_gpu(arch)
    _lib.lib()
    if truncation is not None:
        _check_method(truncation)
    conv = array_type(arch)
    hosts = [mie_host_inputs(m) for m in models]         # (every refusal before the first launch)
    devs = [device_inputs(h, conv) for h in hosts]
    runs, fits = [], []
    for m, h, d in zip(models, hosts, devs):
        runs.append(launch_nai2(m, h, d))
        fit = None
        if isinstance(truncation, DeltaBGE) and h.n_mu > truncation.l_max:
            greek, bulk_f, scal, _work = runs[-1]
            fit = launch_dbge(h.n_mu, truncation.l_max, 0, 1.0, greek, bulk_f, scal, d[4], d[5])
        fits.append(fit)
    synchronize_if_gpu()
    out = []
    for h, (greek, bulk_f, scal, _work), fit in zip(hosts, runs, fits):
        g = to_host(greek)
        c_sca, c_ext, ssa = (float(v) for v in to_host(scal))
        opt = MieAerosolOptics(H.GreekCoefs(*(g[i].copy() for i in range(6))), ssa, 0.0, k=c_ext, C_ext=c_ext, C_sca=c_sca,
                               mu=h.mu, bulk_f=to_host(bulk_f))
        if truncation is not None:
            opt = _untruncated(opt) if fit is None else _collect_dbge(truncation, opt, fit)
        out.append(opt)
    return out


def launch_nai2_lin(model: MieModel, h: MieHostInputs, dev, dev_dot):
    """Enqueues vsm_mie_nai2_lin on the current stream: (greek, bulk_f, scal, greek_dot [4, 6, n_mu], bulk_f_dot [4, 4, n_mu],
    scal_dot [4, 3], work) device tensors; dev as for launch_nai2, dev_dot = (wx_dot, wr_dot) [2, nquad].  Nothing is synchronised."""
    nq, like = len(h.x), dev[0]
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=like.device)
    greek, bulk_f, scal = new(6, h.n_mu), new(4, h.n_mu), new(3)
    greek_dot, bulk_f_dot, scal_dot = new(4, 6, h.n_mu), new(4, 4, h.n_mu), new(4, 3)
    elems = int(_lib.lib().vsm_mie_lin_work_elems(nq, h.n_max, h.n_mu))
    if elems == 0:
        raise _lib.VSMError("vsm_mie_lin_work_elems refuses nquad = %d, n_max = %d, n_mu = %d" % (nq, h.n_max, h.n_mu))
    work = _lib.poison(new(elems))
    x, nmax_i, wx, wr, mu, w_mu = dev
    args = (x, nmax_i, wx, wr, dev_dot[0], dev_dot[1], mu, w_mu, greek, bulk_f, scal, greek_dot, bulk_f_dot, scal_dot, work)
    _lib.check(_lib.lib().vsm_mie_nai2_lin(nq, h.n_max, h.n_mu, C.c_double(model.aerosol.n_r), C.c_double(model.aerosol.n_i),
                                           C.c_double(h.k_wave), *[CR._ptr(t) for t in args], CR._stream_ptr()))
    return greek, bulk_f, scal, greek_dot, bulk_f_dot, scal_dot, work


def compute_aerosol_optical_properties_lin(model_or_list, architecture=None):
    """compute_aerosol_optical_properties(lin, model) (compute_NAI2_lin.jl:16-279) for one MieModel or a list of them: a list of
    (MieAerosolOptics, MieLinAerosolOptics) pairs.  The first is bit for bit what compute_aerosol_optical_properties returns; the
    second holds the derivatives in the slot order (n_r, n_i, mu, sigma) -- see MieLinAerosolOptics -- and goes into
    host_model.LinModel(lin_aerosol_optics=[...]) as it is.  All models are enqueued before the one synchronisation.  This call
    does not truncate: truncate_phase_lin on a pair, or compute_truncated_aerosol_optical_properties_lin, does."""
    return compute_truncated_aerosol_optical_properties_lin(model_or_list, None, architecture)


def _collect_nai2_lin(h: MieHostInputs, run):
    """After the synchronisation: the (MieAerosolOptics, MieLinAerosolOptics) pair of one launch_nai2_lin."""
    greek, bulk_f, scal, greek_dot, bulk_f_dot, scal_dot, _work = run
    g, gd, sd = to_host(greek), to_host(greek_dot), to_host(scal_dot)
    c_sca, c_ext, ssa = (float(v) for v in to_host(scal))
    opt = MieAerosolOptics(H.GreekCoefs(*(g[i].copy() for i in range(6))), ssa, 0.0, k=c_ext, C_ext=c_ext, C_sca=c_sca,
                           mu=h.mu, bulk_f=to_host(bulk_f))
    lin = MieLinAerosolOptics([H.GreekCoefs(*(gd[s, i].copy() for i in range(6))) for s in range(4)], sd[:, 2].copy(),
                              np.zeros(4), k_dot=sd[:, 1].copy(), C_ext_dot=sd[:, 1].copy(), C_sca_dot=sd[:, 0].copy(),
                              bulk_f_dot=to_host(bulk_f_dot))
    return opt, lin


def compute_truncated_aerosol_optical_properties_lin(model_or_list, truncation, architecture=None):
    """compute_aerosol_optical_properties_lin and truncate_phase_lin in one pass over the device: each model's
    vsm_truncate_dbge_lin is enqueued directly behind its vsm_mie_nai2_lin, on the device arrays greek, bulk_f, scal, greek_dot,
    bulk_f_dot and scal_dot, and one synchronisation brings the whole list back.  A list of (TruncatedAerosolOptics,
    TruncatedLinAerosolOptics) pairs, bit for bit those of truncate_phase_lin on compute_aerosol_optical_properties_lin's pairs
    (which are their `untruncated`).  truncation: DeltaBGE(l_max, .) or NoTruncation(); None returns the untruncated
    (MieAerosolOptics, MieLinAerosolOptics) pairs themselves -- compute_aerosol_optical_properties_lin is that call."""
    models = [model_or_list] if isinstance(model_or_list, MieModel) else list(model_or_list)
    arch = architecture if architecture is not None else default_architecture()
    CR._require_gpu(arch)
    _lib.lib()
    if truncation is not None:
        _check_method(truncation)
    conv = array_type(arch)
    hosts = [mie_lin_host_inputs(m) for m in models]     # (every refusal before the first launch)
    devs = [(device_inputs(h, conv), (conv(wxd), conv(wrd))) for h, wxd, wrd in hosts]
    runs, fits = [], []
    for m, (h, _, _), (d, dd) in zip(models, hosts, devs):
        runs.append(launch_nai2_lin(m, h, d, dd))
        fit = None
        if isinstance(truncation, DeltaBGE) and h.n_mu > truncation.l_max:
            fit = launch_dbge_lin(h.n_mu, int(truncation.l_max), *runs[-1][:6], d[4], d[5])
        fits.append(fit)
    synchronize_if_gpu()
    out = []
    for (h, _, _), run, fit in zip(hosts, runs, fits):
        opt, lin = _collect_nai2_lin(h, run)
        if truncation is None:
            out.append((opt, lin))
        elif fit is None:
            out.append((_untruncated(opt), _untruncated_lin(lin)))
        else:
            out.append(_collect_dbge_lin(truncation, opt, lin, fit))
    return out


# ---- truncate_phase.jl ----------------------------------------------------------------------------------------------------------
class NoTruncation:
    """NoTruncation(): the coefficients as they are, f_trunc = 0."""

    def __repr__(self):
        return "NoTruncation()"

    def __eq__(self, other):
        return isinstance(other, NoTruncation)

    def __hash__(self):
        return hash(NoTruncation)


@dataclass(frozen=True)
class DeltaBGE:
    """deltaBGE(l_max, delta_angle) (types.jl): keep l_max coefficients; delta_angle [degrees] is the half-angle of the forward
    cone that truncate_phase_lowconf leaves out of its fit (truncate_phase carries it and does not read it)."""
    l_max: int
    delta_angle: float = 0.0


δBGE = DeltaBGE


@dataclass
class TruncatedAerosolOptics(H.AerosolOptics):
    """host_model.AerosolOptics after truncate_phase: greek_coefs of l_max entries, ssa unchanged, f_trunc = 1 - c0 -- what
    host_model.createAero's delta-M scaling reads --, the method, and the object that went in (the exact single-scattering
    correction of a truncated run wants the untruncated phase function).  k, C_ext, C_sca are carried over where it has them;
    info is the device's status of the beta, gamma and epsilon fits (0 = solved, 1 = skipped: a series of exact zeros)."""
    c0: float = 1.0
    method: object = field(default_factory=NoTruncation)
    untruncated: Optional[H.AerosolOptics] = None
    k: Optional[float] = None
    C_ext: Optional[float] = None
    C_sca: Optional[float] = None
    info: tuple = ()


@dataclass
class TruncatedLinAerosolOptics(H.LinAerosolOptics):
    """host_model.LinAerosolOptics after truncate_phase_lin: lin_greek_coefs of l_max entries per slot, ssa_dot unchanged,
    f_trunc_dot = -c0_dot -- what host_model.createAeroLin's delta-M scaling reads --, the method, and the derivatives that went
    in.  k_dot, C_ext_dot, C_sca_dot are carried over where they have them.  LinModel(lin_aerosol_optics=[...]) takes it as it
    is."""
    c0_dot: Optional[np.ndarray] = None
    method: object = field(default_factory=NoTruncation)
    untruncated: Optional[H.LinAerosolOptics] = None
    k_dot: Optional[np.ndarray] = None
    C_ext_dot: Optional[np.ndarray] = None
    C_sca_dot: Optional[np.ndarray] = None


SYSTEMS = ("beta", "gamma", "epsilon")     # the three fits, in the order of vsm_truncate_dbge's info


def _check_method(method):
    if isinstance(method, NoTruncation):
        return
    if not isinstance(method, DeltaBGE):
        raise _lib.VSMError("truncation method %r: NoTruncation() or DeltaBGE(l_max, delta_angle)" % (method,))
    if int(method.l_max) != method.l_max or method.l_max < 3:
        raise _lib.VSMError("DeltaBGE: l_max = %r < 3 (the gamma and epsilon fits start at l = 2)" % (method.l_max,))
    if method.l_max > MAX_DBGE_L:
        raise _lib.VSMError("DeltaBGE: l_max = %d above the %d coefficients the truncation kernels take (VSM_DBGE_MAX_L)"
                            % (method.l_max, MAX_DBGE_L))
    if not (0.0 <= method.delta_angle < 180.0):
        raise _lib.VSMError("DeltaBGE: delta_angle = %r outside [0, 180) degrees" % (method.delta_angle,))


def _carry(optics):
    return {n: getattr(optics, n) for n in ("k", "C_ext", "C_sca") if getattr(optics, n, None) is not None}


def _untruncated(optics):
    """truncate_phase(NoTruncation(), .): the very same coefficient arrays, f_trunc = 0."""
    return TruncatedAerosolOptics(optics.greek_coefs, optics.ssa, 0.0, c0=1.0, method=NoTruncation(), untruncated=optics,
                                  **_carry(optics))


def launch_dbge(n_mu, l_max, lowconf, cos_delta, greek, bulk_f, scal, mu, w_mu):
    """Enqueues vsm_truncate_dbge on the current stream: (greek_t [6, l_max], scal_t [2], info [3], work) device tensors.  Nothing
    is synchronised; the inputs and the work buffer must outlive the work."""
    dev = greek.device
    greek_t = torch.empty((6, l_max), dtype=torch.float64, device=dev)
    scal_t = torch.empty(2, dtype=torch.float64, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    elems = int(_lib.lib().vsm_dbge_work_elems(n_mu, l_max))
    if elems == 0:
        raise _lib.VSMError("vsm_dbge_work_elems refuses n_mu = %d, l_max = %d" % (n_mu, l_max))
    work = _lib.poison(torch.empty(elems, dtype=torch.float64, device=dev))
    _lib.check(_lib.lib().vsm_truncate_dbge(n_mu, l_max, lowconf, C.c_double(cos_delta), CR._ptr(greek), CR._ptr(bulk_f),
                                            CR._ptr(scal), CR._ptr(mu), CR._ptr(w_mu), CR._ptr(greek_t), CR._ptr(scal_t),
                                            CR._ptr(info), CR._ptr(work), CR._stream_ptr()))
    return greek_t, scal_t, info, work


def _collect_dbge(method, optics, fit):
    """After the synchronisation: the device's status per system, then the TruncatedAerosolOptics."""
    greek_t, scal_t, info, _work = fit
    status = [int(v) for v in to_host(info)]
    for name, st in zip(SYSTEMS, status):
        if st == 2:
            raise _lib.VSMError("truncate_phase: the %s fit at l_max = %d failed on the device (info = %r): its normal equations "
                                "are not positive definite or not finite, or f11 is not positive at a node"
                                % (name, method.l_max, tuple(status)))
    g = to_host(greek_t)
    c0, f_trunc = (float(v) for v in to_host(scal_t))
    return TruncatedAerosolOptics(H.GreekCoefs(*(g[i].copy() for i in range(6))), optics.ssa, f_trunc, c0=c0, method=method,
                                  untruncated=optics, info=tuple(status), **_carry(optics))


def _greek_matrix(optics):
    g = optics.greek_coefs
    rows = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta)]
    if len({len(r) for r in rows}) != 1:
        raise _lib.VSMError("truncate_phase: the six coefficient vectors have lengths %r" % ([len(r) for r in rows],))
    return np.stack(rows)


def _truncate(method, optics_or_list, architecture, lowconf):
    single = isinstance(optics_or_list, H.AerosolOptics)
    sets = [optics_or_list] if single else list(optics_or_list)
    arch = architecture if architecture is not None else default_architecture()
    CR._require_gpu(arch)
    _lib.lib()
    _check_method(method)
    conv = array_type(arch)
    plans = []                                           # (every refusal before the first launch)
    for o in sets:
        if not isinstance(o, H.AerosolOptics):
            raise _lib.VSMError("truncate_phase: %r is no host_model.AerosolOptics" % (type(o).__name__,))
        greek = _greek_matrix(o)
        L = greek.shape[1]
        if isinstance(method, NoTruncation) or L <= method.l_max:      # (the guard at the reference's call sites)
            plans.append(None)
            continue
        mu, w_mu = gausslegendre(L)
        count, cos_delta = 0, 1.0
        if lowconf:
            cos_delta = math.cos(math.radians(method.delta_angle))
            count = int(np.count_nonzero(mu < cos_delta))
            if count < method.l_max:
                raise _lib.VSMError("truncate_phase_lowconf: %d of the %d nodes lie outside the cone of %g degrees, fewer than "
                                    "l_max = %d unknowns" % (count, L, method.delta_angle, method.l_max))
        bulk = getattr(o, "bulk_f", None)                # Mie optics bring f11, f12, f34 at these very nodes
        if bulk is not None and (np.shape(bulk) != (4, L) or not getattr(o, "C_sca", None)):
            bulk = None
        plans.append((L, count, cos_delta, greek, bulk, mu, w_mu))
    fits = []
    for o, plan in zip(sets, plans):
        if plan is None:
            fits.append(None)
            continue
        L, count, cos_delta, greek, bulk, mu, w_mu = plan
        bulk_d = scal_d = None
        if bulk is not None:
            bulk_d, scal_d = conv(np.asarray(bulk, dtype=np.float64)), conv(np.array([o.C_sca, o.C_ext, o.ssa], dtype=np.float64))
        inputs = (conv(greek), bulk_d, scal_d, conv(mu), conv(w_mu))       # (kept until the synchronisation)
        fits.append((launch_dbge(L, int(method.l_max), count, cos_delta, *inputs), inputs))
    synchronize_if_gpu()
    out = [_untruncated(o) if fit is None else _collect_dbge(method, o, fit[0]) for o, fit in zip(sets, fits)]
    return out[0] if single else out


def truncate_phase(method, optics_or_list, architecture=None):
    """truncate_phase(method, aero) (truncate_phase.jl:29, :149-273) for one host_model.AerosolOptics (Mie, Henyey-Greenstein or
    hand-made) or a list of them; a TruncatedAerosolOptics, or a list of them for a list.  The Gauss-Legendre nodes are those of
    order len(beta).  MieAerosolOptics bring their bulk_f at these nodes and are fitted to it; every other set is reconstructed
    from its coefficients on the device.  A series with len(beta) <= l_max comes back as NoTruncation() returns it.  All sets are
    enqueued before the one synchronisation; a fit the device could not solve raises VSMError after it."""
    return _truncate(method, optics_or_list, architecture, False)


def truncate_phase_lowconf(method, optics_or_list, architecture=None):
    """truncate_phase_lowconf(method, aero) (truncate_phase.jl:39, :56-128): the fit over the nodes with
    mu < cos(delta_angle), weights w / max(|f|, 1e-8) -- the variant the reference applies to analytic phase functions."""
    return _truncate(method, optics_or_list, architecture, True)


# ---- truncate_phase_lin.jl ------------------------------------------------------------------------------------------------------
def _carry_dot(lin):
    return {n: getattr(lin, n) for n in ("k_dot", "C_ext_dot", "C_sca_dot") if getattr(lin, n, None) is not None}


def _untruncated_lin(lin):
    """truncate_phase(NoTruncation(), aero, lin_aero) (truncate_phase_lin.jl:221-229): the very same derivative arrays,
    f_trunc_dot = 0."""
    return TruncatedLinAerosolOptics(lin.lin_greek_coefs, lin.ssa_dot, np.zeros(4), c0_dot=np.zeros(4), method=NoTruncation(),
                                     untruncated=lin, **_carry_dot(lin))


def launch_dbge_lin(n_mu, l_max, greek, bulk_f, scal, greek_dot, bulk_f_dot, scal_dot, mu, w_mu):
    """Enqueues vsm_truncate_dbge_lin on the current stream: (greek_t [6, l_max], scal_t [2], info [3], work, greek_t_dot
    [4, 6, l_max], scal_t_dot [4, 2]) device tensors -- the first four as launch_dbge returns them.  Nothing is synchronised; the
    inputs and the work buffer must outlive the work."""
    dev = greek.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    greek_t, scal_t, greek_t_dot, scal_t_dot = new(6, l_max), new(2), new(4, 6, l_max), new(4, 2)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    elems = int(_lib.lib().vsm_dbge_lin_work_elems(n_mu, l_max))
    if elems == 0:
        raise _lib.VSMError("vsm_dbge_lin_work_elems refuses n_mu = %d, l_max = %d" % (n_mu, l_max))
    work = _lib.poison(new(elems))
    args = (greek, bulk_f, scal, greek_dot, bulk_f_dot, scal_dot, mu, w_mu, greek_t, scal_t, greek_t_dot, scal_t_dot, info, work)
    _lib.check(_lib.lib().vsm_truncate_dbge_lin(n_mu, l_max, 0, C.c_double(1.0), *[CR._ptr(t) for t in args], CR._stream_ptr()))
    return greek_t, scal_t, info, work, greek_t_dot, scal_t_dot


def _collect_dbge_lin(method, optics, lin, fit):
    """After the synchronisation: the status per system (a derivative that is not finite is a failed system too), then the
    pair."""
    trunc = _collect_dbge(method, optics, fit[:4])
    gd, sd = to_host(fit[4]), to_host(fit[5])
    lin_t = TruncatedLinAerosolOptics([H.GreekCoefs(*(gd[s, i].copy() for i in range(6))) for s in range(4)], lin.ssa_dot,
                                      sd[:, 1].copy(), c0_dot=sd[:, 0].copy(), method=method, untruncated=lin, **_carry_dot(lin))
    return trunc, lin_t


def _greek_dot_matrix(lin, L):
    """greek_dot [4, 6, L] of a LinAerosolOptics whose coefficient vectors must have the L entries of the optics'."""
    slots = list(lin.lin_greek_coefs)
    if len(slots) != 4:
        raise _lib.VSMError("truncate_phase_lin: %d derivative slots, not 4" % len(slots))
    out = np.empty((4, 6, L))
    for s, g in enumerate(slots):
        for c, v in enumerate((g.alpha, g.beta, g.gamma, g.delta, g.epsilon, g.zeta)):
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            if len(v) != L:
                raise _lib.VSMError("truncate_phase_lin: a derivative vector of slot %d has %d entries, the coefficients %d"
                                    % (s, len(v), L))
            out[s, c] = v
    return out


def truncate_phase_lin(method, optics_or_list, lin_optics_or_list, architecture=None):
    """truncate_phase(method, aero, lin_aero) (truncate_phase_lin.jl:24-208) for one host_model.AerosolOptics with its
    host_model.LinAerosolOptics, or two lists of them: (TruncatedAerosolOptics, TruncatedLinAerosolOptics), or a list of such
    pairs.  The fit is truncate_phase's (all nodes, weights w / f^2); the first of a pair is what truncate_phase returns, bit for
    bit.  A MieAerosolOptics with a MieLinAerosolOptics is fitted to bulk_f and differentiated through bulk_f_dot; every other
    pair is reconstructed from its coefficients and their derivatives on the device -- f and f' always from the same source, so a
    MieAerosolOptics paired with derivatives that bring no bulk_f_dot is reconstructed too (then, and only then, the first of
    the pair differs from truncate_phase's in the last bits).  NoTruncation() or len(beta) <= l_max returns the very same arrays
    with f_trunc = 0 and f_trunc_dot zeros.  All pairs are enqueued before the one synchronisation; a fit the device could not
    solve, or whose derivatives are not finite, raises VSMError after it."""
    single = isinstance(optics_or_list, H.AerosolOptics)
    if single != isinstance(lin_optics_or_list, H.LinAerosolOptics):
        raise _lib.VSMError("truncate_phase_lin: one AerosolOptics with one LinAerosolOptics, or two lists")
    sets = [optics_or_list] if single else list(optics_or_list)
    lins = [lin_optics_or_list] if single else list(lin_optics_or_list)
    if len(sets) != len(lins):
        raise _lib.VSMError("truncate_phase_lin: %d optics and %d linearized optics" % (len(sets), len(lins)))
    arch = architecture if architecture is not None else default_architecture()
    CR._require_gpu(arch)
    _lib.lib()
    _check_method(method)
    conv = array_type(arch)
    plans = []                                           # (every refusal before the first launch)
    for o, lo in zip(sets, lins):
        if not isinstance(o, H.AerosolOptics) or not isinstance(lo, H.LinAerosolOptics):
            raise _lib.VSMError("truncate_phase_lin: (%s, %s) is no (host_model.AerosolOptics, host_model.LinAerosolOptics)"
                                % (type(o).__name__, type(lo).__name__))
        greek = _greek_matrix(o)
        L = greek.shape[1]
        greek_dot = _greek_dot_matrix(lo, L)
        for row, name in ((2, "gamma"), (4, "epsilon")):
            if not np.any(greek[row, 2:] != 0.0) and np.any(greek_dot[:, row, 2:] != 0.0):
                raise _lib.VSMError("truncate_phase_lin: the %s series is exact zeros from l = 2 on (its fit is skipped) and its "
                                    "derivative series is not" % name)
        if isinstance(method, NoTruncation) or L <= method.l_max:
            plans.append(None)
            continue
        mu, w_mu = gausslegendre(L)
        bulk, bulk_dot, csca_dot = getattr(o, "bulk_f", None), getattr(lo, "bulk_f_dot", None), getattr(lo, "C_sca_dot", None)
        mie = (bulk is not None and np.shape(bulk) == (4, L) and bool(getattr(o, "C_sca", None)) and bulk_dot is not None
               and np.shape(bulk_dot) == (4, 4, L) and csca_dot is not None and np.shape(csca_dot) == (4,))
        plans.append((L, greek, greek_dot, mie, mu, w_mu))
    fits = []
    for o, lo, plan in zip(sets, lins, plans):
        if plan is None:
            fits.append(None)
            continue
        L, greek, greek_dot, mie, mu, w_mu = plan
        bulk_d = scal_d = bulk_dot_d = scal_dot_d = None
        if mie:
            f64 = lambda a: np.asarray(a, dtype=np.float64)
            bulk_d, scal_d = conv(f64(o.bulk_f)), conv(np.array([o.C_sca, o.C_ext, o.ssa], dtype=np.float64))
            c_ext_dot = lo.C_ext_dot if getattr(lo, "C_ext_dot", None) is not None else np.zeros(4)     # (not read by the fit)
            scal_dot = np.ascontiguousarray(np.stack([f64(lo.C_sca_dot), f64(c_ext_dot), f64(lo.ssa_dot)], axis=1))
            bulk_dot_d, scal_dot_d = conv(np.ascontiguousarray(f64(lo.bulk_f_dot))), conv(scal_dot)
        inputs = (conv(greek), bulk_d, scal_d, conv(greek_dot), bulk_dot_d, scal_dot_d, conv(mu), conv(w_mu))
        fits.append((launch_dbge_lin(L, int(method.l_max), *inputs), inputs))      # (inputs kept until the synchronisation)
    synchronize_if_gpu()
    out = [(_untruncated(o), _untruncated_lin(lo)) if fit is None else _collect_dbge_lin(method, o, lo, fit[0])
           for o, lo, fit in zip(sets, lins, fits)]
    return out[0] if single else out
