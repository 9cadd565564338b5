"""Absorption: line-by-line gas cross-sections and tau_abs on the device (src/Absorption of the reference).

    HitranTable, read_hitran                      a HITRAN line table from arrays or from a local 160-column .par file
    Doppler, Lorentz, Voigt                       broadening functions
    HumlicekWeidemann32VoigtErrorFunction, HumlicekWeidemann32SDErrorFunction, CPF12ErrorFunction
                                                  the complex error functions the device evaluates
    IsotopologueData, qoft                        molar mass and the partition sum table of one (mol, iso); Q(T_ref) / Q(T)
    make_hitran_model, HitranModel
    compute_absorption_cross_section (alias absorption_cross_section)
                                                  sigma [nSpec] at one (p, T), or [Nz, nSpec] for a whole profile in ONE
                                                  vsm_absorption_xsec call
    compute_absorption_profile                    tau_abs [nSpec, Nz] of a list of gases, summed on the device, and with lin=True
                                                  the gas slots sigma_g vcd_dry of LinModel.tau_abs_dot
    SLOTS, qoft_lin, compute_absorption_cross_section_lin, compute_absorption_profile_lin, AbsorptionProfileLin
                                                  ours (the reference has no such derivative): sigma and d sigma / d(T, p, vmr_self)
                                                  per layer in ONE vsm_absorption_xsec_lin call; tau_abs with dtau_dT, dtau_dp,
                                                  dtau_dvmr_self[g] and profile slots that LinModel.tau_abs_dot takes

Names follow the reference; its non-ASCII field names are spelled out: nu (νᵢ), S (Sᵢ), A (Aᵢ), gamma_air, gamma_self, E_low (E″),
n_air, delta_air, g_upper (g′), g_lower (g″).

What stays on the host: reading and filtering the table, sorting it by nu0 (the reference sums in file order; the sums here run in
nu0 order), the partition-sum spline, one value per (layer, isotopologue).  Everything with a line or grid-point loop runs in
csrc/vsm_absorption.hip.  No TIPS or molar-mass table ships with this package: `isotopologues` hands them in.

Not built: InterpolationModel / ABSCO tables, CIA, MT_CKD, linearized CPF12, FP32, the Erfc* error functions
(they need a complex erfcx) and HumlicekErrorFunction (no `w` method in the reference either).

One deviation from the reference: a line whose pressure-shifted window misses the grid contributes nothing; the
reference gives such a line the window [1, N]."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import core_rt as CR
from .architectures import array_type, default_architecture, devi, synchronize_if_gpu, to_host

# constants/constants.jl (the device holds the same values)
p_ref = 1013.25
t_ref = 296.0
nm_per_m = 1.0e7


class HitranEmptyError(_lib.VSMError):
    """read_hitran: no line matches the filters."""


# ---- types.jl ------------------------------------------------------------------------------------------------------------------------
@dataclass
class HitranTable:
    mol: np.ndarray
    iso: np.ndarray
    nu: np.ndarray            # νᵢ: vacuum wavenumber of the transition, cm^-1
    S: np.ndarray             # Sᵢ: line intensity at 296 K
    A: np.ndarray             # Aᵢ: Einstein A
    gamma_air: np.ndarray
    gamma_self: np.ndarray
    E_low: np.ndarray         # E″: lower-state energy, cm^-1 (-1: no temperature correction)
    n_air: np.ndarray
    delta_air: np.ndarray
    g_upper: Optional[np.ndarray] = None   # g′
    g_lower: Optional[np.ndarray] = None   # g″
    global_upper_quanta: Sequence[str] = ()
    global_lower_quanta: Sequence[str] = ()
    local_upper_quanta: Sequence[str] = ()
    local_lower_quanta: Sequence[str] = ()
    ierr: Sequence[str] = ()
    iref: Sequence[str] = ()
    line_mixing_flag: Sequence[str] = ()

    def __post_init__(self):
        self.mol = np.asarray(self.mol, dtype=np.int64).reshape(-1)
        self.iso = np.asarray(self.iso, dtype=np.int64).reshape(-1)
        n = len(self.mol)
        for name in ("nu", "S", "A", "gamma_air", "gamma_self", "E_low", "n_air", "delta_air", "g_upper", "g_lower"):
            v = getattr(self, name)
            if v is None:
                continue
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            if len(v) != n or len(self.iso) != n:
                raise _lib.VSMError("HitranTable: %s has %d entries, mol %d" % (name, len(v), n))
            setattr(self, name, v)

    def __len__(self):
        return len(self.mol)


class AbstractBroadeningFunction:
    code = -1

    def __repr__(self):
        return "%s()" % type(self).__name__


class Doppler(AbstractBroadeningFunction):
    code = 0


class Lorentz(AbstractBroadeningFunction):
    code = 1


class Voigt(AbstractBroadeningFunction):
    code = 2


class AbstractComplexErrorFunction:
    code = -1

    def __repr__(self):
        return "%s()" % type(self).__name__


class HumlicekWeidemann32VoigtErrorFunction(AbstractComplexErrorFunction):
    code = 0


class HumlicekWeidemann32SDErrorFunction(AbstractComplexErrorFunction):
    code = 1


class CPF12ErrorFunction(AbstractComplexErrorFunction):
    code = 2


class _NotBuiltCEF(AbstractComplexErrorFunction):
    why = ""

    def __init__(self):
        raise NotImplementedError("%s is not built: %s" % (type(self).__name__, self.why))


class HumlicekErrorFunction(_NotBuiltCEF):
    why = "the reference defines no w(::HumlicekErrorFunction, z) either"


class ErfcHumliErrorFunctionVoigt(_NotBuiltCEF):
    why = "it needs a complex erfcx on the device"


class ErfcHumliErrorFunctionSD(_NotBuiltCEF):
    why = "it needs a complex erfcx on the device"


class ErfcErrorFunction(_NotBuiltCEF):
    why = "it needs a complex erfcx on the device"


@dataclass
class IsotopologueData:
    """What the reference reads from its TIPS 2017 and molar-mass files for one (mol, iso): the molar mass (g / mol) and the
    partition sum Q at the temperatures TT."""
    molar_mass: float
    TT: np.ndarray
    TQ: np.ndarray

    def __post_init__(self):
        self.TT = np.asarray(self.TT, dtype=np.float64).reshape(-1)
        self.TQ = np.asarray(self.TQ, dtype=np.float64).reshape(-1)
        if len(self.TT) != len(self.TQ) or len(self.TT) < 2 or not np.all(np.diff(self.TT) > 0):
            raise _lib.VSMError("IsotopologueData: TT and TQ need the same length >= 2 and TT strictly ascending")
        if not self.molar_mass > 0:
            raise _lib.VSMError("IsotopologueData: molar_mass = %r must be positive" % (self.molar_mass,))


@dataclass
class HitranModel:
    hitran: HitranTable
    broadening: AbstractBroadeningFunction
    wing_cutoff: float = 40.0
    vmr: object = 0.0
    CEF: AbstractComplexErrorFunction = field(default_factory=HumlicekWeidemann32SDErrorFunction)
    architecture: object = None
    isotopologues: Dict[Tuple[int, int], IsotopologueData] = field(default_factory=dict)


# ---- read_hitran.jl ------------------------------------------------------------------------------------------------------------------
_VAR_LENGTHS = (2, 1, 12, 10, 10, 5, 5, 10, 4, 8, 15, 15, 15, 15, 6, 12, 1, 7, 7)
_VAR_KINDS = "ii" + "f" * 8 + "s" * 7 + "ff"
_VAR_STARTS = tuple(int(v) for v in np.concatenate([[0], np.cumsum(_VAR_LENGTHS)]))


def _parse(kind, text):
    if kind == "s":
        return text
    try:
        return int(text) if kind == "i" else float(text)
    except ValueError:
        return 0 if kind == "i" else 0.0     # something(tryparse(...), 0)


def read_hitran(path, mol=-1, iso=-1, ν_min=0, ν_max=math.inf, min_strength=0):
    """read_hitran(filepath; mol, iso, ν_min, ν_max, min_strength) of read_hitran.jl on a local 160-column .par file: the lines with
    the molecule and isotopologue asked for (-1: all), ν_min <= nu <= ν_max and S >= min_strength, in file order.  Nothing is
    downloaded and no artifact is looked up.  HitranEmptyError if nothing matches."""
    assert len(_VAR_KINDS) == len(_VAR_LENGTHS)
    rows = []
    with open(path, "r") as f:
        for ln in f:
            ln = ln.rstrip("\r\n")
            if not ln:
                continue
            v = [_parse(k, ln[a:b]) for k, a, b in zip(_VAR_KINDS, _VAR_STARTS[:-1], _VAR_STARTS[1:])]
            if (v[0] == mol or mol == -1) and (v[1] == iso or iso == -1) and ν_min <= v[2] <= ν_max and v[3] >= min_strength:
                rows.append(v)
    if not rows:
        raise HitranEmptyError("read_hitran: no line of %s matches mol = %r, iso = %r, %r <= nu <= %r" % (path, mol, iso, ν_min, ν_max))
    c = list(zip(*rows))
    return HitranTable(mol=c[0], iso=c[1], nu=c[2], S=c[3], A=c[4], gamma_air=c[5], gamma_self=c[6], E_low=c[7], n_air=c[8],
                       delta_air=c[9], global_upper_quanta=list(c[10]), global_lower_quanta=list(c[11]),
                       local_upper_quanta=list(c[12]), local_lower_quanta=list(c[13]), ierr=list(c[14]), iref=list(c[15]),
                       line_mixing_flag=list(c[16]), g_upper=c[17], g_lower=c[18])


# ---- make_model_helpers.jl -----------------------------------------------------------------------------------------------------------
def make_hitran_model(hitran, broadening, wing_cutoff=40, vmr=0, CEF=None, architecture=None, isotopologues=None):
    """make_hitran_model(hitran, broadening; wing_cutoff, vmr, CEF, architecture) with the isotopologue data the reference reads from
    its own files: isotopologues = {(mol, iso): IsotopologueData(molar_mass, TT, TQ)}.  Every (mol, iso) of the table must be there."""
    if not isinstance(hitran, HitranTable):
        raise _lib.VSMError("make_hitran_model: %r is no HitranTable" % (type(hitran).__name__,))
    if not isinstance(broadening, AbstractBroadeningFunction) or broadening.code < 0:
        raise _lib.VSMError("make_hitran_model: broadening %r: Doppler(), Lorentz() or Voigt()" % (broadening,))
    CEF = HumlicekWeidemann32SDErrorFunction() if CEF is None else CEF
    if not isinstance(CEF, AbstractComplexErrorFunction) or CEF.code < 0:
        raise _lib.VSMError("make_hitran_model: CEF %r is none of the three error functions the device evaluates" % (CEF,))
    if not (float(wing_cutoff) >= 0):
        raise _lib.VSMError("make_hitran_model: wing_cutoff = %r < 0" % (wing_cutoff,))
    isotopologues = dict(isotopologues or {})
    for key, d in isotopologues.items():
        if not isinstance(d, IsotopologueData):
            raise _lib.VSMError("make_hitran_model: isotopologues[%r] is no IsotopologueData" % (key,))
    missing = sorted(set(zip(hitran.mol.tolist(), hitran.iso.tolist())) - set(isotopologues))
    if missing:
        raise _lib.VSMError("make_hitran_model: no IsotopologueData for (mol, iso) = %s (this package ships no TIPS or molar-mass "
                            "table)" % (missing,))
    return HitranModel(hitran=hitran, broadening=broadening, wing_cutoff=float(wing_cutoff), vmr=vmr, CEF=CEF,
                       architecture=architecture if architecture is not None else default_architecture(),
                       isotopologues=isotopologues)


# ---- qoft! ---------------------------------------------------------------------------------------------------------------------------
def _natural_spline_second_derivatives(t, u):
    n = len(t)
    z = np.zeros(n)
    if n > 2:
        h = np.diff(t)
        M = np.zeros((n - 2, n - 2))
        i = np.arange(n - 2)
        M[i, i] = 2.0 * (h[:-1] + h[1:])
        M[i[:-1], i[:-1] + 1] = h[1:-1]
        M[i[1:], i[1:] - 1] = h[1:-1]
        z[1:-1] = np.linalg.solve(M, 6.0 * (np.diff(u[1:]) / h[1:] - np.diff(u[:-1]) / h[:-1]))
    return z


def _spline_eval(t, u, z, x):
    i = np.clip(np.searchsorted(t, x, side="right"), 1, len(t) - 1)
    h = t[i] - t[i - 1]
    return (z[i - 1] * (t[i] - x) ** 3 / (6.0 * h) + z[i] * (x - t[i - 1]) ** 3 / (6.0 * h)
            + (u[i] / h - z[i] * h / 6.0) * (x - t[i - 1]) + (u[i - 1] / h - z[i - 1] * h / 6.0) * (t[i] - x))


def qoft(iso_data: IsotopologueData, T, T_ref=t_ref):
    """Q(T_ref) / Q(T) (qoft!): a natural cubic spline through (TT, TQ), as the reference's DI_CS, on the host.  T a scalar or an
    array; a T outside (min TT, max TT) raises, which is the reference's assertion."""
    Tv = np.asarray(T, dtype=np.float64)
    lo, hi = iso_data.TT[0], iso_data.TT[-1]
    if not np.all((lo < Tv) & (Tv < hi)):
        raise _lib.VSMError("qoft: T (%s) must be between %g K and %g K" % (np.array2string(Tv, threshold=8), lo, hi))
    z = _natural_spline_second_derivatives(iso_data.TT, iso_data.TQ)
    q = _spline_eval(iso_data.TT, iso_data.TQ, z, np.atleast_1d(Tv))
    q_ref = _spline_eval(iso_data.TT, iso_data.TQ, z, np.asarray([float(T_ref)]))[0]
    r = q_ref / q
    return float(r[0]) if Tv.ndim == 0 else r


def _spline_eval_derivative(t, u, z, x):
    i = np.clip(np.searchsorted(t, x, side="right"), 1, len(t) - 1)
    h = t[i] - t[i - 1]
    return (-z[i - 1] * (t[i] - x) ** 2 / (2.0 * h) + z[i] * (x - t[i - 1]) ** 2 / (2.0 * h)
            + (u[i] / h - z[i] * h / 6.0) - (u[i - 1] / h - z[i - 1] * h / 6.0))


def qoft_lin(iso_data: IsotopologueData, T, T_ref=t_ref):
    """(Q(T_ref) / Q(T), d/dT of it): qoft and the analytic derivative of the same natural spline, -Q(T_ref) Q'(T) / Q(T)^2.  The first
    value is qoft's bit for bit; the same refusal."""
    Tv = np.asarray(T, dtype=np.float64)
    r = qoft(iso_data, Tv, T_ref)
    z = _natural_spline_second_derivatives(iso_data.TT, iso_data.TQ)
    q = _spline_eval(iso_data.TT, iso_data.TQ, z, np.atleast_1d(Tv))
    dq = _spline_eval_derivative(iso_data.TT, iso_data.TQ, z, np.atleast_1d(Tv))
    q_ref = _spline_eval(iso_data.TT, iso_data.TQ, z, np.asarray([float(T_ref)]))[0]
    d = -q_ref * dq / (q * q)
    return (r, float(d[0])) if Tv.ndim == 0 else (r, d)


# ---- compute_absorption_cross_section.jl: the host part ------------------------------------------------------------------------------
@dataclass
class _Job:
    """One vsm_absorption_xsec call, on the host: the grid in wavenumbers, the selected lines sorted by nu0 and the profile."""
    grid: np.ndarray
    lines: Dict[str, np.ndarray]     # nu, S, gamma_air, gamma_self, n_air, delta_air, E_low [nLines]; species [nLines] int32
    molar_mass: np.ndarray           # [nSpecies]
    p: np.ndarray
    T: np.ndarray
    vmr_self: np.ndarray
    qratio: np.ndarray               # [Nz, nSpecies]
    wing_cutoff: float
    delta_max: float
    broadening: int
    cef: int
    reverse: bool                    # wavelength_flag: the result is reversed along the grid
    species_keys: Sequence[Tuple[int, int]] = ()   # the (mol, iso) behind each species index
    qratio_dlnT: Optional[np.ndarray] = None   # [Nz, nSpecies] d ln(Q(T_ref) / Q(T)) / dT: the linearized calls only

    @property
    def n_lines(self):
        return len(self.lines["nu"])


def _prepare(model: HitranModel, grid, pressure, temperature, wavelength_flag=False) -> _Job:
    """:44-105 for a whole profile: unit conversion, the (min - cutoff, max + cutoff) filter on the unshifted nu0, the sort, the species
    index and Q(T_ref) / Q(T) per (layer, species).  Raises before anything is launched."""
    if not isinstance(model, HitranModel):
        raise _lib.VSMError("compute_absorption_cross_section: %r is no HitranModel (InterpolationModel is not built)"
                            % (type(model).__name__,))
    ht = model.hitran
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    if grid.size < 1 or not np.all(np.isfinite(grid)):
        raise _lib.VSMError("compute_absorption_cross_section: the grid needs at least one finite point")
    cutoff = float(model.wing_cutoff)
    grid_max, grid_min = grid.max() + cutoff, grid.min() - cutoff
    if wavelength_flag:
        grid = (nm_per_m / grid)[::-1].copy()
        grid_min, grid_max = nm_per_m / grid_max, nm_per_m / grid_min
    if not np.all(np.diff(grid) > 0):
        raise _lib.VSMError("compute_absorption_cross_section: the grid must be strictly ascending")
    p = np.atleast_1d(np.asarray(pressure, dtype=np.float64))
    T = np.atleast_1d(np.asarray(temperature, dtype=np.float64))
    if p.ndim != 1 or p.shape != T.shape or p.size < 1:
        raise _lib.VSMError("compute_absorption_cross_section: pressure %r and temperature %r must be scalars or vectors of one "
                            "length" % (p.shape, T.shape))
    vmr = np.asarray(model.vmr, dtype=np.float64)
    if vmr.ndim > 0 and vmr.shape != p.shape:
        raise _lib.VSMError("compute_absorption_cross_section: model.vmr of shape %r for %d layers" % (vmr.shape, p.size))
    vmr = np.ascontiguousarray(np.broadcast_to(vmr, p.shape))

    keep = np.nonzero((grid_min < ht.nu) & (ht.nu < grid_max))[0]
    keep = keep[np.argsort(ht.nu[keep], kind="stable")]
    lines = {k: np.ascontiguousarray(getattr(ht, k)[keep]) for k in ("nu", "S", "gamma_air", "gamma_self", "n_air", "delta_air", "E_low")}
    keys = sorted(set(zip(ht.mol[keep].tolist(), ht.iso[keep].tolist())))
    missing = [k for k in keys if k not in model.isotopologues]
    if missing:
        raise _lib.VSMError("compute_absorption_cross_section: no IsotopologueData for (mol, iso) = %s" % (missing,))
    index = {k: i for i, k in enumerate(keys)}
    species = np.asarray([index[k] for k in zip(ht.mol[keep].tolist(), ht.iso[keep].tolist())], dtype=np.int32)
    lines["species"] = species
    qratio = np.ones((p.size, max(len(keys), 1)))
    for k, i in index.items():
        if np.any(lines["E_low"][species == i] != -1):       # (the reference calls qoft! only for such lines)
            qratio[:, i] = qoft(model.isotopologues[k], T)
    mass = np.asarray([model.isotopologues[k].molar_mass for k in keys] or [1.0], dtype=np.float64)
    dmax = float(np.max(np.abs(lines["delta_air"]))) if len(keep) else 0.0
    return _Job(grid=grid, lines=lines, molar_mass=mass, p=p, T=T, vmr_self=vmr, qratio=qratio, wing_cutoff=cutoff, delta_max=dmax,
                broadening=model.broadening.code, cef=model.CEF.code, reverse=bool(wavelength_flag), species_keys=tuple(keys))


class _Device:
    """The device side of this module: buffers, the vsm_absorption_xsec launches of a list of jobs, and the one synchronisation that
    brings results back.  (The CPU tests replace this class to check the host bookkeeping around it.)"""

    def __init__(self, architecture):
        self.arch = architecture if architecture is not None else default_architecture()
        CR._require_gpu(self.arch)
        _lib.lib()
        self.conv = array_type(self.arch)
        self.keep = []               # inputs and work buffers must outlive the enqueued work

    def empty(self, Nz, nSpec):
        return torch.empty((Nz, nSpec), dtype=torch.float64, device=devi(self.arch))

    def zeros(self, Nz, nSpec):
        return self.empty(Nz, nSpec).zero_()

    def profile(self, job: _Job, lin=False):
        """The device arrays that do not depend on the scale: uploaded once per job.  lin: the work buffer of the linearized call
        and qratio_dlnT beside qratio; such a handle serves xsec() too."""
        names = ("nu", "S", "gamma_air", "gamma_self", "n_air", "delta_air", "E_low", "species")
        dev = [self.conv(job.grid)] + [self.conv(job.lines[k]) for k in names]
        dev += [self.conv(a) for a in (job.molar_mass, job.p, job.T, job.vmr_self)]
        sizer = "vsm_absorption_lin_work_elems" if lin else "vsm_absorption_work_elems"
        elems = int(getattr(_lib.lib(), sizer)(len(job.p), job.n_lines))
        if elems == 0:
            raise _lib.VSMError("%s refuses Nz = %d, nLines = %d" % (sizer, len(job.p), job.n_lines))
        work = _lib.poison(torch.empty(elems, dtype=torch.float64, device=dev[0].device))
        h = dict(dev=dev, q=self.conv(job.qratio), work=work)
        if lin:
            h["qd"] = self.conv(job.qratio_dlnT)
        self.keep.append(h)
        return h

    def xsec(self, job: _Job, handle, scale, out, accumulate):
        """Enqueues one vsm_absorption_xsec on the current stream: out [Nz, nSpec] = (accumulate ? out : 0) + scale[layer] sigma."""
        sc = self.conv(np.ascontiguousarray(scale, dtype=np.float64))
        self.keep.append(sc)
        d = handle["dev"]
        _lib.check(_lib.lib().vsm_absorption_xsec(
            len(job.grid), job.n_lines, len(job.molar_mass), len(job.p), *[CR._ptr(t) for t in d[:13]], CR._ptr(sc),
            CR._ptr(handle["q"]), C.c_double(job.wing_cutoff), C.c_double(job.delta_max), job.broadening, job.cef, int(accumulate),
            CR._ptr(out), CR._ptr(handle["work"]), CR._stream_ptr()))

    def profile_lin(self, job: _Job):
        return self.profile(job, lin=True)

    def xsec_lin(self, job: _Job, handle, scale, out, out_dT, out_dp, out_dvmr, accumulate):
        """Enqueues one vsm_absorption_xsec_lin: out as xsec's, and the three slot planes [Nz, nSpec] = (accumulate ? plane : 0) +
        scale[layer] d sigma / d(T, p, vmr_self)."""
        sc = self.conv(np.ascontiguousarray(scale, dtype=np.float64))
        self.keep.append(sc)
        d = handle["dev"]
        _lib.check(_lib.lib().vsm_absorption_xsec_lin(
            len(job.grid), job.n_lines, len(job.molar_mass), len(job.p), *[CR._ptr(t) for t in d[:13]], CR._ptr(sc),
            CR._ptr(handle["q"]), CR._ptr(handle["qd"]), C.c_double(job.wing_cutoff), C.c_double(job.delta_max), job.broadening,
            job.cef, int(accumulate), CR._ptr(out), CR._ptr(out_dT), CR._ptr(out_dp), CR._ptr(out_dvmr), CR._ptr(handle["work"]),
            CR._stream_ptr()))

    def profile_slots(self, dT, dp, T_dot, p_dot):
        """Enqueues vsm_absorption_profile_slots: [K, Nz, nSpec] = dT T_dot[k] + dp p_dot[k] from the planes on the device."""
        K, (Nz, nSpec) = len(T_dot), dT.shape
        td, pd = self.conv(np.ascontiguousarray(T_dot, dtype=np.float64)), self.conv(np.ascontiguousarray(p_dot, dtype=np.float64))
        out = torch.empty((K, Nz, nSpec), dtype=torch.float64, device=dT.device)
        self.keep += [td, pd]
        _lib.check(_lib.lib().vsm_absorption_profile_slots(nSpec, Nz, K, CR._ptr(dT), CR._ptr(dp), CR._ptr(td), CR._ptr(pd),
                                                           CR._ptr(out), CR._stream_ptr()))
        return out

    def fetch(self, outs):
        synchronize_if_gpu()
        self.keep.clear()
        return [to_host(o) for o in outs]


def compute_absorption_cross_section(model, grid, pressure, temperature, wavelength_flag=False):
    """compute_absorption_cross_section(model::HitranModel, grid, pressure, temperature; wavelength_flag) (:32-179).  Scalar pressure
    (hPa) and temperature (K): sigma [nSpec] (cm^2 / molecule), the reference's call.  Vectors of length Nz, with model.vmr a scalar
    or [Nz]: sigma [Nz, nSpec] from ONE vsm_absorption_xsec call and one synchronisation.  wavelength_flag: the grid is in nm; it is
    converted to wavenumbers and reversed, and the result is reversed back, as the reference does.  An empty selection of lines
    returns exact zeros without a launch."""
    scalar = np.ndim(pressure) == 0 and np.ndim(temperature) == 0
    job = _prepare(model, grid, pressure, temperature, wavelength_flag)
    Nz, nSpec = len(job.p), len(job.grid)
    if job.n_lines == 0:
        sig = np.zeros((Nz, nSpec))
    else:
        dev = _Device(model.architecture)
        out = dev.empty(Nz, nSpec)
        dev.xsec(job, dev.profile(job), np.ones(Nz), out, 0)
        sig = dev.fetch([out])[0]
    if job.reverse:
        sig = sig[:, ::-1].copy()
    return sig[0] if scalar else sig


absorption_cross_section = compute_absorption_cross_section


def compute_absorption_profile(models_and_vmrs, grid, p_full, T, vcd_dry, lin=False, architecture=None):
    """compute_absorption_profile! (atmo_prof.jl:464-486) for a list of (model, vmr) pairs -- vmr the gas's volume mixing ratio, a
    scalar or [Nz] --: tau_abs [nSpec, Nz] = sum_g sigma_g(p_full[z], T[z]) vcd_dry[z] vmr_g[z], the layout model_from_arrays takes.
    The gases are summed on the device (`accumulate`); there is no per-layer host loop and one synchronisation for the whole list.
    lin=True: (tau_abs, tau_abs_dot) with tau_abs_dot[g] = sigma_g vcd_dry [nSpec, Nz] (atmo_prof_lin.jl:153), the gas slots of
    LinModel.tau_abs_dot; tau_abs is bit for bit the one of lin=False."""
    pairs = list(models_and_vmrs)
    if not pairs:
        raise _lib.VSMError("compute_absorption_profile: no (model, vmr) pair")
    p = np.asarray(p_full, dtype=np.float64).reshape(-1)
    Tz = np.asarray(T, dtype=np.float64).reshape(-1)
    vcd = np.asarray(vcd_dry, dtype=np.float64).reshape(-1)
    Nz = len(p)
    if len(Tz) != Nz or len(vcd) != Nz or Nz < 1:
        raise _lib.VSMError("compute_absorption_profile: p_full, T and vcd_dry have %d, %d and %d layers" % (Nz, len(Tz), len(vcd)))
    jobs, scales = [], []
    for model, vmr in pairs:                                        # (every refusal before the first launch)
        v = np.asarray(vmr, dtype=np.float64)
        if v.ndim > 0 and v.shape != (Nz,):
            raise _lib.VSMError("compute_absorption_profile: the length of a vmr array (%r) has to match the profile (%d) or be "
                                "uniform" % (v.shape, Nz))
        jobs.append(_prepare(model, grid, p, Tz, False))
        scales.append(vcd * v)
    nSpec = len(jobs[0].grid)
    if all(j.n_lines == 0 for j in jobs):
        z = np.zeros((nSpec, Nz))
        return (z, [z.copy() for _ in jobs]) if lin else z
    dev = _Device(architecture if architecture is not None else pairs[0][0].architecture)
    tau, dots, started = dev.empty(Nz, nSpec), [], False
    for job, scale in zip(jobs, scales):
        if job.n_lines == 0:
            dots.append(None)
            continue
        h = dev.profile(job)
        dev.xsec(job, h, scale, tau, 1 if started else 0)
        started = True
        if lin:
            d = dev.empty(Nz, nSpec)
            dev.xsec(job, h, vcd, d, 0)
            dots.append(d)
    live = [d for d in dots if d is not None] if lin else []
    host = dev.fetch([tau] + live)
    tau_abs = np.ascontiguousarray(host[0].T)
    if not lin:
        return tau_abs
    it = iter(host[1:])
    return tau_abs, [np.zeros((nSpec, Nz)) if d is None else np.ascontiguousarray(next(it).T) for d in dots]


# ---- linearized: d sigma / d(T, p, vmr_self) per layer and the profile slots of tau_abs (ours) ---------------------------
SLOTS = ("T", "p", "vmr_self")       # K^-1, hPa^-1, 1


def _prepare_lin(model, grid, pressure, temperature, wavelength_flag=False) -> _Job:
    """_prepare with its refusals, the CPF12 refusal, and d ln(Q(T_ref) / Q(T)) / dT per (layer, species) beside qratio."""
    job = _prepare(model, grid, pressure, temperature, wavelength_flag)
    if isinstance(model.broadening, Voigt) and model.CEF.code == CPF12ErrorFunction.code:
        raise NotImplementedError("linearized CPF12 is not built (its region II is no analytic formula): use "
                                  "HumlicekWeidemann32SDErrorFunction or HumlicekWeidemann32VoigtErrorFunction")
    dln = np.zeros_like(job.qratio)
    for i, k in enumerate(job.species_keys):
        if np.any(job.lines["E_low"][job.lines["species"] == i] != -1):
            r, d = qoft_lin(model.isotopologues[k], job.T)
            dln[:, i] = d / r
    job.qratio_dlnT = dln
    return job


def compute_absorption_cross_section_lin(model, grid, pressure, temperature, wavelength_flag=False):
    """(sigma, sigma_dot): compute_absorption_cross_section's sigma, bit for bit, and its derivatives for SLOTS = (T [K^-1],
    p [hPa^-1], vmr_self [1]) of each layer: sigma_dot [3, nSpec] for scalar p, T, [3, Nz, nSpec] for a profile (layer z depends on
    p[z], T[z], vmr[z] alone).  It is the derivative of the function the device evaluates with the index windows of the wing cutoff
    and, per (line, point), the region of the error function frozen: the derivative almost everywhere.  ONE vsm_absorption_xsec_lin
    call and one synchronisation; wavelength_flag reverses every slot as sigma; an empty selection returns exact zeros without a
    launch.  Refuses what the forward refuses, and Voigt with CPF12ErrorFunction (NotImplementedError)."""
    scalar = np.ndim(pressure) == 0 and np.ndim(temperature) == 0
    job = _prepare_lin(model, grid, pressure, temperature, wavelength_flag)
    Nz, nSpec = len(job.p), len(job.grid)
    if job.n_lines == 0:
        sig, dot = np.zeros((Nz, nSpec)), np.zeros((3, Nz, nSpec))
    else:
        dev = _Device(model.architecture)
        outs = [dev.empty(Nz, nSpec) for _ in range(4)]
        dev.xsec_lin(job, dev.profile_lin(job), np.ones(Nz), *outs, 0)
        host = dev.fetch(outs)
        sig, dot = host[0], np.stack(host[1:])
    if job.reverse:
        sig, dot = sig[:, ::-1].copy(), dot[:, :, ::-1].copy()
    return (sig[0], dot[:, 0]) if scalar else (sig, dot)


@dataclass
class AbsorptionProfileLin:
    """What compute_absorption_profile_lin returns; every array [nSpec, Nz] unless said otherwise."""
    tau_abs: np.ndarray                    # bit for bit compute_absorption_profile's
    tau_abs_dot: list                      # [g]: sigma_g vcd_dry, as lin=True
    dtau_dT: np.ndarray                    # sum_g vcd_dry vmr_g d sigma_g / dT of the layer's own T (the Jacobian is diagonal in the layer)
    dtau_dp: np.ndarray                    # the same for p
    dtau_dvmr_self: list                   # [g]: vcd_dry vmr_g d sigma_g / d vmr_self: add it to tau_abs_dot[g] if the gas broadens itself
    profile_slots: np.ndarray              # [K, nSpec, Nz]: dtau_dT T_dot[k] + dtau_dp p_dot[k]

    def lin_model_slots(self):
        """tau_abs_dot + list(profile_slots): what host_model.LinModel(tau_abs_dot=...) takes; NGas is its length."""
        return list(self.tau_abs_dot) + list(self.profile_slots)


def compute_absorption_profile_lin(models_and_vmrs, grid, p_full, T, vcd_dry, T_dot=None, p_dot=None, architecture=None):
    """compute_absorption_profile(..., lin=True) and the T, p and vmr_self Jacobians of tau_abs: an AbsorptionProfileLin.
    T_dot, p_dot [K, Nz] (either may be None = zeros) are K perturbation profiles, shaped as B_layer_dot is: a unit table per layer
    for weighting functions, a row of ones for a profile shift, p_full / p_surf for surface pressure; profile_slots[k] =
    dtau_dT T_dot[k] + dtau_dp p_dot[k] is formed on the device.  The gases are summed on the device through `accumulate`; one
    synchronisation for the whole list.  vcd_dry is held FIXED: the caller owns d vcd_dry / d p_surf.  Refuses what
    compute_absorption_profile refuses, Voigt with CPF12ErrorFunction (NotImplementedError) and tables that are not [K, Nz], all
    before the first launch."""
    pairs = list(models_and_vmrs)
    if not pairs:
        raise _lib.VSMError("compute_absorption_profile: no (model, vmr) pair")
    p = np.asarray(p_full, dtype=np.float64).reshape(-1)
    Tz = np.asarray(T, dtype=np.float64).reshape(-1)
    vcd = np.asarray(vcd_dry, dtype=np.float64).reshape(-1)
    Nz = len(p)
    if len(Tz) != Nz or len(vcd) != Nz or Nz < 1:
        raise _lib.VSMError("compute_absorption_profile: p_full, T and vcd_dry have %d, %d and %d layers" % (Nz, len(Tz), len(vcd)))
    tabs = [None if t is None else np.asarray(t, dtype=np.float64) for t in (T_dot, p_dot)]
    for name, t in zip(("T_dot", "p_dot"), tabs):
        if t is not None and (t.ndim != 2 or t.shape[1] != Nz or t.shape[0] < 1):
            raise _lib.VSMError("compute_absorption_profile_lin: %s of shape %r is not [K, %d]" % (name, t.shape, Nz))
    if tabs[0] is not None and tabs[1] is not None and tabs[0].shape != tabs[1].shape:
        raise _lib.VSMError("compute_absorption_profile_lin: T_dot %r and p_dot %r differ in K" % (tabs[0].shape, tabs[1].shape))
    K = next((len(t) for t in tabs if t is not None), 0)
    if K > 65535:
        raise _lib.VSMError("compute_absorption_profile_lin: K = %d above 65535 profile slots" % K)
    tabs = [np.zeros((K, Nz)) if t is None else t for t in tabs]
    jobs, scales = [], []
    for model, vmr in pairs:                                        # (every refusal before the first launch)
        v = np.asarray(vmr, dtype=np.float64)
        if v.ndim > 0 and v.shape != (Nz,):
            raise _lib.VSMError("compute_absorption_profile: the length of a vmr array (%r) has to match the profile (%d) or be "
                                "uniform" % (v.shape, Nz))
        jobs.append(_prepare_lin(model, grid, p, Tz, False))
        scales.append(vcd * v)
    nSpec = len(jobs[0].grid)

    def z():
        return np.zeros((nSpec, Nz))

    if all(j.n_lines == 0 for j in jobs):
        return AbsorptionProfileLin(z(), [z() for _ in jobs], z(), z(), [z() for _ in jobs], np.zeros((K, nSpec, Nz)))
    dev = _Device(architecture if architecture is not None else pairs[0][0].architecture)
    tau, dT, dp = dev.empty(Nz, nSpec), dev.empty(Nz, nSpec), dev.empty(Nz, nSpec)
    dots, dvs, started = [], [], False
    for job, scale in zip(jobs, scales):
        if job.n_lines == 0:
            dots.append(None)
            dvs.append(None)
            continue
        h = dev.profile_lin(job)
        dv = dev.zeros(Nz, nSpec) if started else dev.empty(Nz, nSpec)      # `accumulate` holds for all four outputs of a call
        dev.xsec_lin(job, h, scale, tau, dT, dp, dv, 1 if started else 0)
        started = True
        d = dev.empty(Nz, nSpec)
        dev.xsec(job, h, vcd, d, 0)
        dots.append(d)
        dvs.append(dv)
    live = [a for pair in zip(dots, dvs) if pair[0] is not None for a in pair]
    slots = [dev.profile_slots(dT, dp, tabs[0], tabs[1])] if K else []
    host = dev.fetch([tau, dT, dp] + slots + live)
    it = iter(host[3 + len(slots):])
    out_dots, out_dvs = [], []
    for d in dots:
        out_dots.append(z() if d is None else np.ascontiguousarray(next(it).T))
        out_dvs.append(z() if d is None else np.ascontiguousarray(next(it).T))
    ps = np.ascontiguousarray(np.transpose(host[3], (0, 2, 1))) if K else np.zeros((0, nSpec, Nz))
    return AbsorptionProfileLin(np.ascontiguousarray(host[0].T), out_dots, np.ascontiguousarray(host[1].T),
                                np.ascontiguousarray(host[2].T), out_dvs, ps)
