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
    InterpolationModel, make_interpolation_model, UniformRange, save_interpolation_model, load_interpolation_model
                                                  a sigma(nu, p, T) table, linear or cubic B-spline, FP64 or FP32, built in one
                                                  vsm_absorption_xsec call over the nP nT states and prefiltered on the device; it stays
                                                  resident there; every entry point below and above takes it where it takes a
                                                  HitranModel, alone or mixed (csrc/vsm_absorption_lut.hip)
    SLOTS, qoft_lin, compute_absorption_cross_section_lin, compute_absorption_profile_lin, AbsorptionProfileLin
                                                  ours (the reference has no such derivative): sigma and d sigma / d(T, p, vmr_self)
                                                  per layer in ONE vsm_absorption_xsec_lin call; tau_abs with dtau_dT, dtau_dp,
                                                  dtau_dvmr_self[g] and profile slots that LinModel.tau_abs_dot takes
    CIABlock, parse_cia_file, CIATable, build_cia_table, load_cia_table
                                                  HITRAN collision-induced absorption (cia.jl): a local .cia file projected on the
                                                  grid once, on the host; the table stays resident on the device in FP64
    MTCKDTable, load_mtckd, MTCKDBand, build_mtckd_band
                                                  the MT_CKD H2O continuum (mtckd.jl) from a .npz with the AER file's six variables
    layer_thickness                               the reference's hydrostatic layer thickness (atmo_prof.jl:67)
    compute_continuum_profile, ContinuumProfileLin
                                                  tau [nSpec, Nz] of a continuum set -- up to 8 CIATables and one MTCKDBand -- in ONE
                                                  vsm_absorption_continuum launch, and with lin=True its T, p, vmr and dz derivatives
                                                  (ours); compute_absorption_profile(_lin) take the set as continua= and add it behind
                                                  the gases on the device (csrc/vsm_absorption_continuum.hip)

Names follow the reference; its non-ASCII field names are spelled out: nu (νᵢ), S (Sᵢ), A (Aᵢ), gamma_air, gamma_self, E_low (E″),
n_air, delta_air, g_upper (g′), g_lower (g″).

What stays on the host: reading and filtering the table, sorting it by nu0 (the reference sums in file order; the sums here run in
nu0 order), the partition-sum spline, one value per (layer, isotopologue).  Everything with a line or grid-point loop runs in
csrc/vsm_absorption.hip.  No TIPS or molar-mass table ships with this package: `isotopologues` hands them in.

Not built: ABSCO / HDF5 tables and their mixed linear / quadratic interpolant, a vmr axis or extrapolation in p or T of an
InterpolationModel, NetCDF ingestion and FP32 storage of the continua, linearized CPF12, FP32 line-by-line sums, the Erfc* error functions (they need a complex erfcx) and
HumlicekErrorFunction (no `w` method in the reference either).

Deviations from the reference: a line whose pressure-shifted window misses the grid contributes nothing (the
reference gives such a line the window [1, N]); a continuum set is refused unless the grid is array_equal to the one its members
were built on (the reference compares lengths); a CIA block whose nu does not ascend strictly is refused (the reference divides
by zero); load_mtckd reads a .npz, not NetCDF."""
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
        raise _lib.VSMError("compute_absorption_cross_section: %r is neither a HitranModel nor an InterpolationModel"
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

    def lut_coef(self, model):
        """The model's coefficients on the device: uploaded on first use and cached on the model."""
        if model._coef_dev is None:
            model._coef_dev = self.conv(model._coef_host)
        return model._coef_dev

    def _lut_args(self, job, coef):
        m = job.model
        g, p, T = self.conv(job.grid), self.conv(job.p), self.conv(job.T)
        self.keep += [g, p, T, coef]
        return [len(job.grid), len(job.p), m.ν_grid.n, m.p_grid.n, m.t_grid.n] + \
            [C.c_double(v) for ax in (m.ν_grid, m.p_grid, m.t_grid) for v in (ax.first, ax.step)] + \
            [_LUT_INTERP[m.interp_type], _LUT_STORAGE[m.storage_type], CR._ptr(coef), CR._ptr(g), CR._ptr(p), CR._ptr(T)]

    def lut_eval(self, job, scale, out, accumulate):
        """Enqueues one vsm_absorption_lut_eval: out [Nz, nSpec] = (accumulate ? out : 0) + scale[layer] sigma_itp."""
        sc = self.conv(np.ascontiguousarray(scale, dtype=np.float64))
        self.keep.append(sc)
        _lib.check(_lib.lib().vsm_absorption_lut_eval(*self._lut_args(job, self.lut_coef(job.model)), CR._ptr(sc), int(accumulate),
                                                      CR._ptr(out), CR._stream_ptr()))

    def lut_eval_lin(self, job, scale, out, out_dT, out_dp, accumulate):
        """Enqueues one vsm_absorption_lut_eval_lin: out as lut_eval's and the T and p planes beside it."""
        sc = self.conv(np.ascontiguousarray(scale, dtype=np.float64))
        self.keep.append(sc)
        _lib.check(_lib.lib().vsm_absorption_lut_eval_lin(*self._lut_args(job, self.lut_coef(job.model)), CR._ptr(sc),
                                                          int(accumulate), CR._ptr(out), CR._ptr(out_dT), CR._ptr(out_dp),
                                                          CR._stream_ptr()))

    def lut_prefilter(self, values, nNu, nP, nT, storage_type):
        """Enqueues vsm_absorption_lut_prefilter on values [nP nT, nNu] (a device array): the coefficients [nP + 2, nT + 2, nNu + 2]."""
        st = _LUT_STORAGE[storage_type]
        elems = int(_lib.lib().vsm_absorption_lut_work_elems(nNu, nP, nT, st))
        if elems == 0:
            raise _lib.VSMError("vsm_absorption_lut_work_elems refuses nNu = %d, nP = %d, nT = %d" % (nNu, nP, nT))
        work = _lib.poison(torch.empty(elems, dtype=torch.float64, device=values.device))
        coef = torch.empty((nP + 2, nT + 2, nNu + 2), dtype=torch.float32 if st else torch.float64, device=values.device)
        self.keep += [values, work]
        _lib.check(_lib.lib().vsm_absorption_lut_prefilter(nNu, nP, nT, CR._ptr(values), st, CR._ptr(coef), CR._ptr(work),
                                                           CR._stream_ptr()))
        return coef

    def member(self, m):
        """A continuum member's arrays on the device: uploaded on first use and cached on the member."""
        if m._dev is None:
            m._dev = self.conv(m._host_image())
        return m._dev

    def _continuum_args(self, job, n_planes):
        """The arguments both continuum entry points share, up to band_layer; A (and B) cut to the first n_planes planes."""
        tabs = [self.member(t) for t in job.tables]
        n = len(tabs)
        hp = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in tabs])
        hn = (C.c_int * max(n, 1))(*[len(t.Ts) for t in job.tables])
        dev = [self.conv(a) for a in (job.rows, job.w, np.ascontiguousarray(job.A[:n_planes]), np.ascontiguousarray(job.B[:n_planes]))] \
            if n else [None] * 4
        band = [None] * 5
        if job.band is not None:
            b = self.member(job.band)
            band = [b[0], b[1], b[2], b[3], self.conv(job.band_layer)]
        self.keep += tabs + dev + band + [hp, hn]
        return n, hp, hn, dev, band

    def continuum(self, job, out, accumulate):
        """Enqueues one vsm_absorption_continuum: out [Nz, nSpec] = (accumulate ? out : 0) + the whole set."""
        n, hp, hn, dev, band = self._continuum_args(job, 1)
        _lib.check(_lib.lib().vsm_absorption_continuum(
            job.nSpec, job.Nz, n, hp, hn, CR._ptr(dev[0]), CR._ptr(dev[1]), CR._ptr(dev[2]), *[CR._ptr(b) for b in band],
            int(accumulate), CR._ptr(out), CR._stream_ptr()))

    def continuum_lin(self, job, planes, accumulate):
        """Enqueues one vsm_absorption_continuum_lin on the planes (tau, dT, dp, one per species of the set, ddz), each with its own
        accumulate flag."""
        nP = job.n_planes
        n, hp, hn, dev, band = self._continuum_args(job, nP)
        pl = (C.c_void_p * nP)(*[t.data_ptr() for t in planes])
        acc = (C.c_int * nP)(*[int(a) for a in accumulate])
        h2o = 3 + job.species.index("H2O") if job.band is not None else -1
        _lib.check(_lib.lib().vsm_absorption_continuum_lin(
            job.nSpec, job.Nz, n, hp, hn, CR._ptr(dev[0]), CR._ptr(dev[1]), nP, CR._ptr(dev[2]), CR._ptr(dev[3]),
            *[CR._ptr(b) for b in band], h2o, nP - 1, acc, pl, CR._stream_ptr()))

    def profile_slots_add(self, plane, tab, out):
        """Enqueues vsm_absorption_profile_slots_add: out [K, Nz, nSpec] += plane [Nz, nSpec] tab [K, Nz]."""
        K, (Nz, nSpec) = len(tab), plane.shape
        td = self.conv(np.ascontiguousarray(tab, dtype=np.float64))
        self.keep.append(td)
        _lib.check(_lib.lib().vsm_absorption_profile_slots_add(nSpec, Nz, K, CR._ptr(plane), CR._ptr(td), CR._ptr(out),
                                                               CR._stream_ptr()))

    def fetch(self, outs):
        synchronize_if_gpu()
        self.keep.clear()
        return [to_host(o) for o in outs]


def compute_absorption_cross_section(model, grid, pressure, temperature, wavelength_flag=False):
    """compute_absorption_cross_section(model::HitranModel, grid, pressure, temperature; wavelength_flag) (:32-179).  Scalar pressure
    (hPa) and temperature (K): sigma [nSpec] (cm^2 / molecule), the reference's call.  Vectors of length Nz, with model.vmr a scalar
    or [Nz]: sigma [Nz, nSpec] from ONE vsm_absorption_xsec call and one synchronisation.  wavelength_flag: the grid is in nm; it is
    converted to wavenumbers and reversed, and the result is reversed back, as the reference does.  An empty selection of lines
    returns exact zeros without a launch.
    compute_absorption_cross_section(model::InterpolationModel, ...) (:181-233): the table's interpolant in ONE
    vsm_absorption_lut_eval call.  The grid may be any finite array, unsorted or descending; a point outside [min, max] of the
    table's ν axis gives exact 0, on the boundary it is interpolated; p or T outside their axes raise VSMError before the launch."""
    if isinstance(model, InterpolationModel):
        return _lut_cross_section(model, grid, pressure, temperature, wavelength_flag, lin=False)
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


def compute_absorption_profile(models_and_vmrs, grid, p_full, T, vcd_dry, lin=False, architecture=None, continua=None, dz=None,
                               vmr=None):
    """compute_absorption_profile! (atmo_prof.jl:464-486) for a list of (model, vmr) pairs -- vmr the gas's volume mixing ratio, a
    scalar or [Nz] --: tau_abs [nSpec, Nz] = sum_g sigma_g(p_full[z], T[z]) vcd_dry[z] vmr_g[z], the layout model_from_arrays takes.
    The gases are summed on the device (`accumulate`); there is no per-layer host loop and one synchronisation for the whole list.
    lin=True: (tau_abs, tau_abs_dot) with tau_abs_dot[g] = sigma_g vcd_dry [nSpec, Nz] (atmo_prof_lin.jl:153), the gas slots of
    LinModel.tau_abs_dot; tau_abs is bit for bit the one of lin=False.
    A model may be a HitranModel or an InterpolationModel, in any mix: a table gas is one vsm_absorption_lut_eval launch with the
    same scale / accumulate contract; a list of HitranModels alone issues the launches it always issued.
    continua: a continuum set (compute_continuum_profile: CIATables and at most one MTCKDBand built on `grid`), with the layer
    thicknesses dz [m] and the species' vmr dict; its tau is added behind the gases on the device, in one more launch, through
    `accumulate`.  None: every launch is the one it always was."""
    pairs = list(models_and_vmrs)
    if not pairs:
        raise _lib.VSMError("compute_absorption_profile: no (model, vmr) pair")
    cjob = _profile_continuum(continua, grid, p_full, T, dz, vmr, None)
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
        jobs.append(_prepare_any(model, grid, p, Tz, False))
        scales.append(vcd * v)
    nSpec = len(jobs[0].grid)
    if all(j.n_lines == 0 for j in jobs) and cjob is None:
        z = np.zeros((nSpec, Nz))
        return (z, [z.copy() for _ in jobs]) if lin else z
    dev = _Device(architecture if architecture is not None else pairs[0][0].architecture)
    tau, dots, started = dev.empty(Nz, nSpec), [], False
    for job, scale in zip(jobs, scales):
        if job.n_lines == 0:
            dots.append(None)
            continue
        if isinstance(job, _LutJob):                                # a table gas: the same scale / accumulate contract
            dev.lut_eval(job, scale, tau, 1 if started else 0)
            started = True
            if lin:
                d = dev.empty(Nz, nSpec)
                dev.lut_eval(job, vcd, d, 0)
                dots.append(d)
            continue
        h = dev.profile(job)
        dev.xsec(job, h, scale, tau, 1 if started else 0)
        started = True
        if lin:
            d = dev.empty(Nz, nSpec)
            dev.xsec(job, h, vcd, d, 0)
            dots.append(d)
    if cjob is not None:
        dev.continuum(cjob, tau, 1 if started else 0)
    live = [d for d in dots if d is not None] if lin else []
    host = dev.fetch([tau] + live)
    tau_abs = np.ascontiguousarray(host[0].T)
    if not lin:
        return tau_abs
    it = iter(host[1:])
    return tau_abs, [np.zeros((nSpec, Nz)) if d is None else np.ascontiguousarray(next(it).T) for d in dots]


def _profile_continuum(continua, grid, p_full, T, dz, vmr, dz_dot):
    """The continuum job of a profile call, with its refusals; None without continua."""
    if continua is None:
        if dz_dot is not None:
            raise _lib.VSMError("compute_absorption_profile_lin: dz_dot without continua (no term depends on Δz)")
        return None
    if dz is None:
        raise _lib.VSMError("compute_absorption_profile: continua need the layer thicknesses dz (layer_thickness)")
    return _prepare_continuum(continua, grid, p_full, T, dz, vmr, fn="compute_absorption_profile")


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
    launch.  Refuses what the forward refuses, and Voigt with CPF12ErrorFunction (NotImplementedError).
    An InterpolationModel: sigma of its forward call, bit for bit, and the exact derivative of the interpolant in T and p (linear:
    of the cell the forward evaluates in) from ONE vsm_absorption_lut_eval_lin call; the vmr_self plane is exact zeros, the table
    having been built at a fixed vmr."""
    if isinstance(model, InterpolationModel):
        return _lut_cross_section(model, grid, pressure, temperature, wavelength_flag, lin=True)
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
    profile_slots: np.ndarray              # [K, nSpec, Nz]: dtau_dT T_dot[k] + dtau_dp p_dot[k] (+ dtau_ddz dz_dot[k])
    dtau_dvmr_continuum: dict = field(default_factory=dict)   # species -> d tau / d vmr of the continuum set (continua=)
    dtau_ddz: Optional[np.ndarray] = None  # tau_continuum / Δz [m^-1]; None without continua

    def lin_model_slots(self):
        """tau_abs_dot + list(profile_slots): what host_model.LinModel(tau_abs_dot=...) takes; NGas is its length."""
        return list(self.tau_abs_dot) + list(self.profile_slots)


def compute_absorption_profile_lin(models_and_vmrs, grid, p_full, T, vcd_dry, T_dot=None, p_dot=None, architecture=None, continua=None,
                                   dz=None, vmr=None, dz_dot=None):
    """compute_absorption_profile(..., lin=True) and the T, p and vmr_self Jacobians of tau_abs: an AbsorptionProfileLin.
    T_dot, p_dot [K, Nz] (either may be None = zeros) are K perturbation profiles, shaped as B_layer_dot is: a unit table per layer
    for weighting functions, a row of ones for a profile shift, p_full / p_surf for surface pressure; profile_slots[k] =
    dtau_dT T_dot[k] + dtau_dp p_dot[k] is formed on the device.  The gases are summed on the device through `accumulate`; one
    synchronisation for the whole list.  vcd_dry is held FIXED: the caller owns d vcd_dry / d p_surf.  Refuses what
    compute_absorption_profile refuses, Voigt with CPF12ErrorFunction (NotImplementedError) and tables that are not [K, Nz], all
    before the first launch.  InterpolationModels mix in as in compute_absorption_profile: they add to dtau_dT and dtau_dp (and so
    to profile_slots) through vsm_absorption_lut_eval_lin, and their dtau_dvmr_self[g] is exact zeros.
    continua, dz, vmr: a continuum set as in compute_absorption_profile; ONE vsm_absorption_continuum_lin launch adds it to tau_abs,
    dtau_dT and dtau_dp behind the gases and fills dtau_dvmr_continuum[species] and dtau_ddz.  These partial derivatives hold Δz
    FIXED, as vcd_dry is held fixed; dtau_ddz = tau_continuum / Δz, and dz_dot [K, Nz] adds dtau_ddz dz_dot[k] to profile_slots[k] on
    the device -- a hydrostatic caller passes dz / T T_dot.  dz_dot without continua is refused."""
    pairs = list(models_and_vmrs)
    if not pairs:
        raise _lib.VSMError("compute_absorption_profile: no (model, vmr) pair")
    cjob = _profile_continuum(continua, grid, p_full, T, dz, vmr, dz_dot)
    p = np.asarray(p_full, dtype=np.float64).reshape(-1)
    Tz = np.asarray(T, dtype=np.float64).reshape(-1)
    vcd = np.asarray(vcd_dry, dtype=np.float64).reshape(-1)
    Nz = len(p)
    if len(Tz) != Nz or len(vcd) != Nz or Nz < 1:
        raise _lib.VSMError("compute_absorption_profile: p_full, T and vcd_dry have %d, %d and %d layers" % (Nz, len(Tz), len(vcd)))
    tabs = [None if t is None else np.asarray(t, dtype=np.float64) for t in (T_dot, p_dot, dz_dot)]
    for name, t in zip(("T_dot", "p_dot", "dz_dot"), tabs):
        if t is not None and (t.ndim != 2 or t.shape[1] != Nz or t.shape[0] < 1):
            raise _lib.VSMError("compute_absorption_profile_lin: %s of shape %r is not [K, %d]" % (name, t.shape, Nz))
    if tabs[0] is not None and tabs[1] is not None and tabs[0].shape != tabs[1].shape:
        raise _lib.VSMError("compute_absorption_profile_lin: T_dot %r and p_dot %r differ in K" % (tabs[0].shape, tabs[1].shape))
    K = next((len(t) for t in tabs if t is not None), 0)
    if K > 65535:
        raise _lib.VSMError("compute_absorption_profile_lin: K = %d above 65535 profile slots" % K)
    if tabs[2] is not None and tabs[2].shape[0] != K:
        raise _lib.VSMError("compute_absorption_profile_lin: dz_dot %r differs in K (%d)" % (tabs[2].shape, K))
    dz_tab = tabs[2]
    tabs = [np.zeros((K, Nz)) if t is None else t for t in tabs[:2]]
    jobs, scales = [], []
    for model, vmr in pairs:                                        # (every refusal before the first launch)
        v = np.asarray(vmr, dtype=np.float64)
        if v.ndim > 0 and v.shape != (Nz,):
            raise _lib.VSMError("compute_absorption_profile: the length of a vmr array (%r) has to match the profile (%d) or be "
                                "uniform" % (v.shape, Nz))
        jobs.append(_prepare_any(model, grid, p, Tz, False, lin=True))
        scales.append(vcd * v)
    nSpec = len(jobs[0].grid)

    def z():
        return np.zeros((nSpec, Nz))

    if all(j.n_lines == 0 for j in jobs) and cjob is None:
        return AbsorptionProfileLin(z(), [z() for _ in jobs], z(), z(), [z() for _ in jobs], np.zeros((K, nSpec, Nz)))
    dev = _Device(architecture if architecture is not None else pairs[0][0].architecture)
    tau, dT, dp = dev.empty(Nz, nSpec), dev.empty(Nz, nSpec), dev.empty(Nz, nSpec)
    dots, dvs, started = [], [], False
    for job, scale in zip(jobs, scales):
        if job.n_lines == 0:
            dots.append(None)
            dvs.append(None)
            continue
        if isinstance(job, _LutJob):                                # a table gas adds to tau, dT and dp; it has no vmr_self plane
            dev.lut_eval_lin(job, scale, tau, dT, dp, 1 if started else 0)
            started = True
            d = dev.empty(Nz, nSpec)
            dev.lut_eval(job, vcd, d, 0)
            dots.append(d)
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
    live = [a for pair in zip(dots, dvs) for a in pair if a is not None]
    cplanes = []
    if cjob is not None:                                            # the set: behind the gases on tau, dT and dp; its own planes fresh
        cplanes = [dev.empty(Nz, nSpec) for _ in range(cjob.n_planes - 3)]
        acc = 1 if started else 0
        dev.continuum_lin(cjob, [tau, dT, dp] + cplanes, [acc, acc, acc] + [0] * len(cplanes))
    slots = [dev.profile_slots(dT, dp, tabs[0], tabs[1])] if K else []
    if K and dz_tab is not None:
        dev.profile_slots_add(cplanes[-1], dz_tab, slots[0])
    host = dev.fetch([tau, dT, dp] + slots + live + cplanes)
    chost = host[len(host) - len(cplanes):]
    it = iter(host[3 + len(slots):])
    out_dots, out_dvs = [], []
    for d, dv in zip(dots, dvs):
        out_dots.append(z() if d is None else np.ascontiguousarray(next(it).T))
        out_dvs.append(z() if dv is None else np.ascontiguousarray(next(it).T))
    ps = np.ascontiguousarray(np.transpose(host[3], (0, 2, 1))) if K else np.zeros((0, nSpec, Nz))
    r = AbsorptionProfileLin(np.ascontiguousarray(host[0].T), out_dots, np.ascontiguousarray(host[1].T),
                             np.ascontiguousarray(host[2].T), out_dvs, ps)
    if cjob is not None:
        r.dtau_dvmr_continuum = {sp: np.ascontiguousarray(chost[i].T) for i, sp in enumerate(cjob.species)}
        r.dtau_ddz = np.ascontiguousarray(chost[-1].T)
    return r


# ---- InterpolationModel: sigma(nu, p, T) lookup tables (make_model_helpers.jl:55-122, :181-233) --------------------------
_LUT_INTERP = {"linear": 0, "cubic": 1}
_LUT_STORAGE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}
_LUT_WORK_CAP = 1 << 27              # doubles of vsm_absorption_xsec work per block of states (1 GiB)


@dataclass(frozen=True)
class UniformRange:
    """first : step : first + (n - 1) step, the reference's AbstractRange: an axis of an InterpolationModel."""
    first: float
    step: float
    n: int

    def __post_init__(self):
        object.__setattr__(self, "first", float(self.first))
        object.__setattr__(self, "step", float(self.step))
        object.__setattr__(self, "n", int(self.n))
        if self.n < 2:
            raise _lib.VSMError("UniformRange: an axis needs at least two nodes (n = %d)" % self.n)
        if not (math.isfinite(self.first) and math.isfinite(self.step) and self.step != 0.0):
            raise _lib.VSMError("UniformRange: first = %r, step = %r: finite, step != 0" % (self.first, self.step))

    @property
    def last(self):
        return self.first + (self.n - 1) * self.step

    @property
    def lo(self):
        return min(self.first, self.last)

    @property
    def hi(self):
        return max(self.first, self.last)

    def values(self):
        return self.first + np.arange(self.n) * self.step

    def __len__(self):
        return self.n


def _as_range(x, name):
    """A UniformRange from a UniformRange, a Python range or an array that is uniform to 1e-9 of its step."""
    if isinstance(x, UniformRange):
        return x
    if isinstance(x, range):
        return UniformRange(x.start, x.step, len(x))
    a = np.asarray(x, dtype=np.float64).reshape(-1)
    if a.size < 2:
        raise _lib.VSMError("%s: an axis needs at least two nodes (n = %d)" % (name, a.size))
    if not np.all(np.isfinite(a)):
        raise _lib.VSMError("%s: the axis is not finite" % name)
    step = (a[-1] - a[0]) / (a.size - 1)
    if step == 0.0 or not np.all(np.abs(np.diff(a) - step) <= 1e-9 * abs(step)):
        raise _lib.VSMError("%s: the axis is not uniform to 1e-9 of its step" % name)
    return UniformRange(a[0], step, a.size)


class InterpolationModel:
    """The reference's InterpolationModel (types.jl:185-): itp, mol, iso, ν_grid, p_grid, t_grid, with the interpolant spelled out:
    interp_type "linear" or "cubic", storage_type float64 or float32.  The coefficients live on the device in the layout
    [nP (+2), nT (+2), nν (+2)] (ν contiguous; +2 for cubic) and are cached on the model; `coefficients` (alias itp) is their host
    copy in the reference's axis order [ν, p, T], fetched when first asked for."""

    def __init__(self, mol, iso, ν_grid, p_grid, t_grid, interp_type="cubic", storage_type=np.float64, architecture=None,
                 _coef_host=None, _coef_dev=None, _pending=False):
        if interp_type not in _LUT_INTERP:
            raise _lib.VSMError("InterpolationModel: interp_type must be 'linear' or 'cubic', got %r" % (interp_type,))
        try:
            storage = np.dtype(storage_type)
        except TypeError:
            storage = None
        if storage not in _LUT_STORAGE:
            raise _lib.VSMError("InterpolationModel: storage_type must be float64 or float32, got %r" % (storage_type,))
        self.mol, self.iso = int(mol), int(iso)
        self.ν_grid, self.p_grid, self.t_grid = _as_range(ν_grid, "ν_grid"), _as_range(p_grid, "p_grid"), _as_range(t_grid, "t_grid")
        self.interp_type, self.storage_type = interp_type, storage
        self.architecture = architecture if architecture is not None else default_architecture()
        self._coef_host, self._coef_dev = _coef_host, _coef_dev
        if _coef_host is None and _coef_dev is None and not _pending:     # (_pending: the builder attaches them after its launches)
            raise _lib.VSMError("InterpolationModel: use make_interpolation_model, from_values or from_coefficients")
        for c in (_coef_host, _coef_dev):
            if c is not None and tuple(c.shape) != self.table_shape:
                raise _lib.VSMError("InterpolationModel: coefficients of shape %r for a table of %r" % (tuple(c.shape), self.table_shape))

    @property
    def table_shape(self):
        pad = 2 if self.interp_type == "cubic" else 0
        return (self.p_grid.n + pad, self.t_grid.n + pad, self.ν_grid.n + pad)

    @property
    def resident(self):
        return self._coef_dev is not None

    @property
    def coefficients(self):
        if self._coef_host is None:
            synchronize_if_gpu()
            self._coef_host = np.ascontiguousarray(to_host(self._coef_dev))
        return np.transpose(self._coef_host, (2, 0, 1))

    itp = coefficients

    def __repr__(self):
        return "InterpolationModel(mol=%d, iso=%d, %s, %s, table %r%s)" % (
            self.mol, self.iso, self.interp_type, self.storage_type.name, self.table_shape, ", resident" if self.resident else "")

    @classmethod
    def from_coefficients(cls, coefficients, mol, iso, ν_grid, p_grid, t_grid, interp_type="cubic", storage_type=None,
                          architecture=None):
        """A model from ready coefficients [nν (+2), nP (+2), nT (+2)] (the reference's axis order; +2 for cubic); host only.
        storage_type None: float32 if the array is float32, else float64."""
        c = np.asarray(coefficients)
        if storage_type is None:
            storage_type = np.float32 if c.dtype == np.float32 else np.float64
        if c.ndim != 3:
            raise _lib.VSMError("InterpolationModel.from_coefficients: coefficients of shape %r are not [ν, p, T]" % (c.shape,))
        host = np.ascontiguousarray(np.transpose(c, (1, 2, 0)), dtype=np.dtype(storage_type))
        return cls(mol, iso, ν_grid, p_grid, t_grid, interp_type, storage_type, architecture, _coef_host=host)

    @classmethod
    def from_values(cls, values, mol, iso, ν_grid, p_grid, t_grid, interp_type="cubic", storage_type=np.float64, architecture=None):
        """A model through the values [nν, nP, nT] (the reference's cs_matrix).  Linear: the coefficients are the values, no device.
        Cubic: prefiltered on the device in FP64 (vsm_absorption_lut_prefilter); the coefficients stay there."""
        v = np.asarray(values, dtype=np.float64)
        axes = _as_range(ν_grid, "ν_grid"), _as_range(p_grid, "p_grid"), _as_range(t_grid, "t_grid")
        if v.shape != tuple(a.n for a in axes):
            raise _lib.VSMError("InterpolationModel.from_values: values of shape %r for axes of %r" % (v.shape, tuple(a.n for a in axes)))
        if interp_type == "linear":
            return cls.from_coefficients(v, mol, iso, *axes, "linear", storage_type, architecture)
        model = cls(mol, iso, *axes, interp_type, storage_type, architecture, _pending=True)   # (checks interp_type, storage_type)
        dev = _Device(model.architecture)
        flat = dev.conv(np.ascontiguousarray(np.transpose(v, (1, 2, 0))).reshape(axes[1].n * axes[2].n, axes[0].n))
        model._coef_dev = dev.lut_prefilter(flat, axes[0].n, axes[1].n, axes[2].n, model.storage_type)
        dev.fetch([])
        return model


def make_interpolation_model(hitran, broadening, wave_grid, p_grid, t_grid, wavelength_flag=False, wing_cutoff=40, vmr=0, CEF=None,
                             architecture=None, interp_type="cubic", storage_type=np.float64, isotopologues=None):
    """make_interpolation_model(hitran, broadening, wave_grid, p_grid, t_grid; ...) (make_model_helpers.jl:55-111): the line-by-line
    cross-sections at every (p_grid[i], t_grid[j]) on the ν axis, and their interpolant.  The nP nT states are the layers of ONE
    vsm_absorption_xsec call (the reference launches and synchronises nP nT times), in blocks where Nz <= 65535 or the work buffer
    ask for it; the prefilter follows on the same stream, the table never visits the host, and there is one synchronisation.
    wavelength_flag: wave_grid is in nm and the ν axis is reverse(1e7 / wave_grid), which must come out uniform.  Scalar vmr only,
    as in the reference.  mol is the table's first, iso its common isotopologue or -1."""
    if np.ndim(vmr) != 0:
        raise _lib.VSMError("make_interpolation_model: vmr must be a scalar (the table has no vmr axis)")
    hm = make_hitran_model(hitran, broadening, wing_cutoff=wing_cutoff, vmr=float(vmr), CEF=CEF, architecture=architecture,
                           isotopologues=isotopologues)
    if wavelength_flag:
        nm = wave_grid.values() if isinstance(wave_grid, UniformRange) else np.asarray(wave_grid, dtype=np.float64)
        wave_grid = (nm_per_m / nm)[::-1]
    axes = _as_range(wave_grid, "wave_grid"), _as_range(p_grid, "p_grid"), _as_range(t_grid, "t_grid")
    nNu, nP, nT = (a.n for a in axes)
    mol = int(hitran.mol[0])
    iso = int(hitran.iso[0]) if np.all(hitran.iso == hitran.iso[0]) else -1
    model = InterpolationModel(mol, iso, *axes, interp_type, storage_type, hm.architecture, _pending=True)
    p_states, T_states = np.repeat(axes[1].values(), nT), np.tile(axes[2].values(), nP)
    job = _prepare(hm, axes[0].values(), p_states, T_states, False)
    dev = _Device(hm.architecture)
    Nz = nP * nT
    values = dev.zeros(Nz, nNu) if job.n_lines == 0 else dev.empty(Nz, nNu)
    if job.n_lines:
        per_state = int(_lib.lib().vsm_absorption_work_elems(1, job.n_lines))
        block = int(max(1, min(65535, _LUT_WORK_CAP // per_state)))
        for b0 in range(0, Nz, block):
            b1 = min(Nz, b0 + block)
            part = _Job(**{**job.__dict__, "p": job.p[b0:b1], "T": job.T[b0:b1], "vmr_self": job.vmr_self[b0:b1],
                           "qratio": np.ascontiguousarray(job.qratio[b0:b1])})
            dev.xsec(part, dev.profile(part), np.ones(b1 - b0), values[b0:b1], 0)
    if interp_type == "cubic":
        coef = dev.lut_prefilter(values, nNu, nP, nT, model.storage_type)
    else:
        coef = values.reshape(nP, nT, nNu)
        if model.storage_type == np.dtype(np.float32):
            coef = coef.to(torch.float32)
    model._coef_host, model._coef_dev = None, coef
    dev.fetch([])
    return model


def save_interpolation_model(model, path):
    """One .npz (no pickle): the coefficients in the reference's axis order, the three ranges as (first, step, n), mol, iso,
    interp_type and storage; load_interpolation_model gives the same bits back."""
    if not isinstance(model, InterpolationModel):
        raise _lib.VSMError("save_interpolation_model: %r is no InterpolationModel" % (type(model).__name__,))
    rng = {k: np.asarray([a.first, a.step, float(a.n)]) for k, a in (("nu_range", model.ν_grid), ("p_range", model.p_grid),
                                                                      ("t_range", model.t_grid))}
    with open(path, "wb") as f:
        np.savez(f, coefficients=np.ascontiguousarray(model.coefficients), mol=np.int64(model.mol), iso=np.int64(model.iso),
                 interp_type=np.asarray(model.interp_type), storage=np.asarray(model.storage_type.name), **rng)


def load_interpolation_model(path, architecture=None):
    with np.load(path, allow_pickle=False) as z:
        ax = [UniformRange(z[k][0], z[k][1], int(z[k][2])) for k in ("nu_range", "p_range", "t_range")]
        return InterpolationModel.from_coefficients(z["coefficients"], int(z["mol"]), int(z["iso"]), *ax, str(z["interp_type"]),
                                                    np.dtype(str(z["storage"])), architecture)


@dataclass
class _LutJob:
    """One vsm_absorption_lut_eval call, on the host: the grid in wavenumbers (any order) and the profile."""
    model: InterpolationModel
    grid: np.ndarray
    p: np.ndarray
    T: np.ndarray
    reverse: bool
    n_lines = -1                     # (never the empty selection of a line table)


def _prepare_lut(model, grid, pressure, temperature, wavelength_flag=False) -> _LutJob:
    """:198-233 for a whole profile.  p or T outside their axes raise here, before any launch (the reference throws a BoundsError);
    exactly on an end is inside."""
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    if grid.size < 1 or not np.all(np.isfinite(grid)):
        raise _lib.VSMError("compute_absorption_cross_section: the grid needs at least one finite point")
    if wavelength_flag:
        grid = (nm_per_m / grid)[::-1].copy()
    p = np.atleast_1d(np.asarray(pressure, dtype=np.float64))
    T = np.atleast_1d(np.asarray(temperature, dtype=np.float64))
    if p.ndim != 1 or p.shape != T.shape or p.size < 1:
        raise _lib.VSMError("compute_absorption_cross_section: pressure %r and temperature %r must be scalars or vectors of one "
                            "length" % (p.shape, T.shape))
    if p.size > 65535:
        raise _lib.VSMError("compute_absorption_cross_section: %d layers above 65535" % p.size)
    for name, v, ax in (("pressure", p, model.p_grid), ("temperature", T, model.t_grid)):
        if not np.all((v >= ax.lo) & (v <= ax.hi)):
            raise _lib.VSMError("compute_absorption_cross_section: %s (%s) outside the table's axis [%g, %g] (no extrapolation)"
                                % (name, np.array2string(v, threshold=8), ax.lo, ax.hi))
    return _LutJob(model=model, grid=np.ascontiguousarray(grid), p=p, T=T, reverse=bool(wavelength_flag))


def _prepare_any(model, grid, pressure, temperature, wavelength_flag=False, lin=False):
    if isinstance(model, InterpolationModel):
        return _prepare_lut(model, grid, pressure, temperature, wavelength_flag)
    return (_prepare_lin if lin else _prepare)(model, grid, pressure, temperature, wavelength_flag)


def _lut_cross_section(model, grid, pressure, temperature, wavelength_flag, lin):
    scalar = np.ndim(pressure) == 0 and np.ndim(temperature) == 0
    job = _prepare_lut(model, grid, pressure, temperature, wavelength_flag)
    Nz, nSpec = len(job.p), len(job.grid)
    dev = _Device(model.architecture)
    outs = [dev.empty(Nz, nSpec) for _ in range(3 if lin else 1)]
    if lin:
        dev.lut_eval_lin(job, np.ones(Nz), *outs, 0)
    else:
        dev.lut_eval(job, np.ones(Nz), outs[0], 0)
    host = dev.fetch(outs)
    sig = host[0]
    if job.reverse:
        sig = sig[:, ::-1].copy()
    if not lin:
        return sig[0] if scalar else sig
    dot = np.stack([host[1], host[2], np.zeros((Nz, nSpec))])       # SLOTS; the table was built at a fixed vmr
    if job.reverse:
        dot = dot[:, :, ::-1].copy()
    return (sig[0], dot[:, 0]) if scalar else (sig, dot)


# ---- continua: HITRAN CIA (cia.jl) and the MT_CKD H2O continuum (mtckd.jl), with Jacobians (ours) ------------------------
k_B = 1.380649e-23                   # _CIA_K_B, J / K
VMR_DEFAULTS = {"O2": 0.20946, "N2": 0.78084}      # _layer_vmr's USS dry-air fall-backs
MTCKD_C2 = 1.4388                    # _MTCKD_C2, cm K (the device holds the same value)
R_GAS = 8.3144598                    # atmo_prof.jl:43
CONT_MAX_TABLES = 8                  # VSM_CONT_MAX_TABLES
CONT_MAX_PLANES = 24                 # VSM_CONT_MAX_PLANES
CONT_LAYERS = 4                      # VSM_CONT_LAYERS
CONT_BAND_FIELDS = 10                # VSM_CONT_BAND_FIELDS


@dataclass
class CIABlock:
    """One (T, ν, σ) block of a HITRAN .cia file; σ in cm^5 / molecule^2."""
    formula: str
    T: float
    ν: np.ndarray
    σ: np.ndarray

    def __post_init__(self):
        self.T = float(self.T)
        self.ν = np.asarray(self.ν, dtype=np.float64).reshape(-1)
        self.σ = np.asarray(self.σ, dtype=np.float64).reshape(-1)
        if len(self.ν) != len(self.σ):
            raise _lib.VSMError("CIABlock: ν has %d entries, σ %d" % (len(self.ν), len(self.σ)))


def parse_cia_file(path):
    """parse_cia_file(path) of cia.jl: the blocks of a local HITRAN .cia file, in file order.  A header is read by its fixed columns:
    1-20 formula, 41-47 n_pts, 48-54 T; a line shorter than 54 characters or blank where a header is expected is skipped; of each of
    the n_pts data lines the first two fields are taken."""
    blocks = []
    with open(path, "r") as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    i = 0
    while i < len(lines):
        header = lines[i]
        i += 1
        if len(header) < 54 or not header.strip():
            continue
        formula = header[0:20].strip()
        n_pts, T_K = int(header[40:47].strip()), float(header[47:54].strip())
        if i + n_pts > len(lines):
            raise _lib.VSMError("parse_cia_file: %s ends inside a block of %d points" % (path, n_pts))
        vals = [ln.split() for ln in lines[i:i + n_pts]]
        i += n_pts
        blocks.append(CIABlock(formula, T_K, [float(v[0]) for v in vals], [float(v[1]) for v in vals]))
    return blocks


def _split_pair(formula):
    parts = str(formula).strip().split("-")
    if len(parts) < 2:
        raise _lib.VSMError('CIA pair formula "%s" not recognised (expected "A-B")' % (formula,))
    return parts[0], parts[1]


def _project_linear(x, y_list, xq):
    """_accumulate_σ! / build_mtckd_band for one block and several columns: (inside, values) with values[c] the linear interpolant of
    (x, y_list[c]) at the points xq[inside] in the reference's arithmetic, w = (νq - ν1) / (ν2 - ν1), (1 - w) s1 + w s2; a point on
    the block's first node takes its value."""
    inside = ~((xq < x[0]) | (xq > x[-1]))
    q = xq[inside]
    j = np.searchsorted(x, q, side="left")            # searchsortedfirst, 0-based; <= len(x) - 1 inside the range
    first = j == 0
    j1 = np.where(first, 1 if len(x) > 1 else 0, j)
    j0 = j1 - 1 if len(x) > 1 else j1
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (q - x[j0]) / (x[j1] - x[j0])
        for y in y_list:
            out.append(np.where(first, y[0], (1 - w) * y[j0] + w * y[j1]))
    return inside, out


class CIATable:
    """The reference's CIATable (pair, species_a, species_b, Ts ascending, σ_νT [nSpec, nT]) with the grid it was projected on.
    FP64 only: σ is about 1e-45 cm^5 / molecule^2.  The device copy is [nT, nSpec]; it is uploaded where an MI355X is visible,
    else on first use, and stays resident."""

    def __init__(self, pair, species_a, species_b, Ts, σ_νT, ν_grid, architecture=None):
        self.pair, self.species_a, self.species_b = str(pair), str(species_a), str(species_b)
        self.Ts = np.asarray(Ts, dtype=np.float64).reshape(-1)
        self.ν_grid = np.asarray(ν_grid, dtype=np.float64).reshape(-1)
        self.σ_νT = np.asarray(σ_νT, dtype=np.float64)
        if self.σ_νT.shape != (len(self.ν_grid), len(self.Ts)) or len(self.Ts) < 1 or len(self.ν_grid) < 1:
            raise _lib.VSMError("CIATable: σ_νT of shape %r for %d grid points and %d temperatures"
                                % (self.σ_νT.shape, len(self.ν_grid), len(self.Ts)))
        if not np.all(np.diff(self.Ts) > 0):
            raise _lib.VSMError("CIATable: Ts must be strictly ascending")
        if not (np.all(np.isfinite(self.Ts)) and np.all(np.isfinite(self.ν_grid)) and np.all(np.isfinite(self.σ_νT))):
            raise _lib.VSMError("CIATable: Ts, ν_grid and σ_νT must be finite")
        self.architecture = architecture if architecture is not None else default_architecture()
        self._dev = None
        _make_resident(self)

    @property
    def resident(self):
        return self._dev is not None

    def _host_image(self):
        return np.ascontiguousarray(self.σ_νT.T)

    @classmethod
    def from_arrays(cls, pair, Ts, σ_νT, ν_grid, architecture=None):
        """A table from elsewhere: σ_νT [nSpec, nT] already on ν_grid, Ts strictly ascending."""
        a, b = _split_pair(pair)
        return cls(pair, a, b, Ts, σ_νT, ν_grid, architecture)

    def __repr__(self):
        return "CIATable(%s, %d temperatures, %d points%s)" % (self.pair, len(self.Ts), len(self.ν_grid),
                                                                ", resident" if self.resident else "")


def _make_resident(member):
    """Uploads a continuum member where its architecture is a visible GPU; otherwise it is uploaded on first use."""
    from .architectures import GPU, has_gpu
    if member._dev is None and isinstance(member.architecture, GPU) and has_gpu():
        member._dev = array_type(member.architecture)(member._host_image())
    return member._dev


def build_cia_table(blocks, ν_grid, architecture=None):
    """build_cia_table(blocks, ν_grid) of cia.jl, on the host, once per band: per block temperature the blocks are projected on
    ν_grid in file order, linear in ν inside a block's range and exact 0 outside; a later block of the same temperature overwrites
    an earlier one where they overlap.  The grid may be in any order.  A block whose ν is not strictly ascending is refused (the
    reference divides by zero there)."""
    blocks = list(blocks)
    if not blocks:
        raise _lib.VSMError("build_cia_table: no blocks")
    for n, blk in enumerate(blocks):
        if not isinstance(blk, CIABlock):
            raise _lib.VSMError("build_cia_table: block %d is no CIABlock" % n)
        if len(blk.ν) < 1 or not np.all(np.diff(blk.ν) > 0):
            raise _lib.VSMError("build_cia_table: block %d (%s, %g K): ν is empty or not strictly ascending" % (n, blk.formula, blk.T))
    pair = blocks[0].formula
    a, b = _split_pair(pair)
    Ts = np.unique(np.asarray([blk.T for blk in blocks], dtype=np.float64))
    grid = np.asarray(ν_grid, dtype=np.float64).reshape(-1)
    σ = np.zeros((len(grid), len(Ts)))
    for jt, T_pick in enumerate(Ts):
        for blk in blocks:
            if blk.T != T_pick:
                continue
            inside, (vals,) = _project_linear(blk.ν, [blk.σ], grid)
            σ[inside, jt] = vals
    return CIATable(pair, a, b, Ts, σ, grid, architecture)


def load_cia_table(path, ν_grid, architecture=None):
    return build_cia_table(parse_cia_file(path), ν_grid, architecture)


@dataclass
class MTCKDTable:
    """The six variables of the AER reference file absco-ref_wv-mt-ckd: ν ascending (cm^-1), the self and foreign continuum
    coefficients at T_ref (cm^2 / molecule / cm^-1), the self temperature exponent, p_ref (hPa) and T_ref (K)."""
    ν: np.ndarray
    C_self: np.ndarray
    C_for: np.ndarray
    self_texp: np.ndarray
    p_ref: float
    T_ref: float

    def __post_init__(self):
        for name in ("ν", "C_self", "C_for", "self_texp"):
            setattr(self, name, np.asarray(getattr(self, name), dtype=np.float64).reshape(-1))
        self.p_ref, self.T_ref = float(np.asarray(self.p_ref).reshape(-1)[0]), float(np.asarray(self.T_ref).reshape(-1)[0])
        n = len(self.ν)
        if n < 1 or any(len(getattr(self, k)) != n for k in ("C_self", "C_for", "self_texp")):
            raise _lib.VSMError("MTCKDTable: ν, C_self, C_for and self_texp need one length >= 1")
        if not np.all(np.diff(self.ν) > 0):
            raise _lib.VSMError("MTCKDTable: ν must be strictly ascending")
        if not (self.p_ref > 0 and self.T_ref > 0 and all(np.all(np.isfinite(getattr(self, k)))
                                                          for k in ("ν", "C_self", "C_for", "self_texp"))):
            raise _lib.VSMError("MTCKDTable: p_ref and T_ref must be positive and the arrays finite")


def load_mtckd(path):
    """load_mtckd(path) on a .npz that holds the AER file's six variables under its own names: wavenumbers, self_absco_ref,
    for_absco_ref, self_texp, ref_press, ref_temp.  (NetCDF itself is not read: DESIGN 6.)"""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("wavenumbers", "self_absco_ref", "for_absco_ref", "self_texp", "ref_press", "ref_temp") if k not in z]
        if missing:
            raise _lib.VSMError("load_mtckd: %s lacks %s" % (path, missing))
        return MTCKDTable(z["wavenumbers"], z["self_absco_ref"], z["for_absco_ref"], z["self_texp"], z["ref_press"], z["ref_temp"])


class MTCKDBand:
    """The reference's MTCKDBand (C_self, C_for, texp on the model grid, p_ref, T_ref) with that grid; the device copy is
    [4, nSpec] = (ν, C_self, C_for, texp)."""

    def __init__(self, C_self, C_for, texp, p_ref, T_ref, ν_grid, architecture=None):
        self.ν_grid = np.asarray(ν_grid, dtype=np.float64).reshape(-1)
        self.C_self, self.C_for, self.texp = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (C_self, C_for, texp))
        self.p_ref, self.T_ref = float(p_ref), float(T_ref)
        n = len(self.ν_grid)
        if n < 1 or any(len(a) != n for a in (self.C_self, self.C_for, self.texp)):
            raise _lib.VSMError("MTCKDBand: C_self, C_for, texp and ν_grid need one length >= 1")
        if not (self.p_ref > 0 and self.T_ref > 0 and all(np.all(np.isfinite(a)) for a in (self.ν_grid, self.C_self, self.C_for, self.texp))):
            raise _lib.VSMError("MTCKDBand: p_ref and T_ref must be positive and the arrays finite")
        self.architecture = architecture if architecture is not None else default_architecture()
        self._dev = None
        _make_resident(self)

    @property
    def resident(self):
        return self._dev is not None

    def _host_image(self):
        return np.ascontiguousarray(np.stack([self.ν_grid, self.C_self, self.C_for, self.texp]))


def build_mtckd_band(table, ν_grid, architecture=None):
    """build_mtckd_band(table, ν_grid) of mtckd.jl: the three coefficient arrays linear in ν on ν_grid, exact 0 outside the table."""
    if not isinstance(table, MTCKDTable):
        raise _lib.VSMError("build_mtckd_band: %r is no MTCKDTable" % (type(table).__name__,))
    grid = np.asarray(ν_grid, dtype=np.float64).reshape(-1)
    cols = [np.zeros(len(grid)) for _ in range(3)]
    inside, vals = _project_linear(table.ν, [table.C_self, table.C_for, table.self_texp], grid)
    for c, v in zip(cols, vals):
        c[inside] = v
    return MTCKDBand(cols[0], cols[1], cols[2], table.p_ref, table.T_ref, grid, architecture)


def layer_thickness(p_half, T, vmr_h2o):
    """The reference's hydrostatic Δz [m] per layer (atmo_prof.jl:67): (ln p_half[i+1] - ln p_half[i]) / (g0 M / (R T[i])) with
    M = (1 - vmr_h2o) dry_mass + vmr_h2o wet_mass."""
    from .raman_inputs import DRY_MASS, G0, WET_MASS
    ph, Tz = np.asarray(p_half, dtype=np.float64).reshape(-1), np.asarray(T, dtype=np.float64).reshape(-1)
    v = np.asarray(vmr_h2o, dtype=np.float64)
    if len(ph) != len(Tz) + 1 or (v.ndim > 0 and v.shape != Tz.shape):
        raise _lib.VSMError("layer_thickness: %d half levels, %d layers, vmr_h2o of shape %r" % (len(ph), len(Tz), v.shape))
    M = (1 - v) * DRY_MASS + v * WET_MASS
    return (np.log(ph[1:]) - np.log(ph[:-1])) / (G0 * M / (R_GAS * Tz))


@dataclass
class ContinuumProfileLin:
    """What compute_continuum_profile(..., lin=True) returns; every array [nSpec, Nz].  The partial derivatives hold Δz FIXED (as
    vcd_dry is held fixed in AbsorptionProfileLin); dtau_ddz = tau / Δz [m^-1] is the caller's to chain: a hydrostatic column has
    dΔz / dT = Δz / T."""
    tau: np.ndarray                        # bit for bit the forward call's
    dtau_dT: np.ndarray                    # K^-1, of the layer's own T
    dtau_dp: np.ndarray                    # hPa^-1
    dtau_dvmr: dict                        # species -> d tau / d vmr of that species
    dtau_ddz: np.ndarray                   # m^-1


@dataclass
class _ContinuumJob:
    """One vsm_absorption_continuum(_lin) call, on the host."""
    tables: list
    band: object
    nSpec: int
    Nz: int
    species: list                    # the vmr planes of the linearized call, in plane order
    rows: np.ndarray                 # [nTables, Nz, 2] int32
    w: np.ndarray                    # [nTables, Nz]
    A: np.ndarray                    # [nPlanes, nTables, Nz] (plane 0 alone serves the forward call)
    B: np.ndarray
    band_layer: Optional[np.ndarray]   # [Nz, CONT_BAND_FIELDS]

    @property
    def n_planes(self):
        return 4 + len(self.species)


def _cia_cells(Ts, T):
    """cia_σ_at_T! per layer: (j0, j1, w, 1 / (T2 - T1) or 0 where T is clamped).  T <= Ts[0] and T >= Ts[-1] give the end column back
    exactly (w = 0, w = 1 on one row); a layer on an interior node lies in the cell below it (searchsortedfirst), with w = 1."""
    nT = len(Ts)
    lo, hi = T <= Ts[0], T >= Ts[-1]
    j = np.clip(np.searchsorted(Ts, T, side="left"), 1, max(nT - 1, 1))
    j0 = np.where(lo, 0, np.where(hi, nT - 1, j - 1))
    j1 = np.where(lo, 0, np.where(hi, nT - 1, np.minimum(j, nT - 1)))
    inner = ~(lo | hi)
    T1, T2 = Ts[j0], Ts[j1]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(inner, (T - T1) / (T2 - T1), np.where(lo, 0.0, 1.0))
        inv = np.where(inner, 1.0, 0.0)
        span = np.where(inner, T2 - T1, 1.0)
    return j0.astype(np.int32), j1.astype(np.int32), w, inv, span


def _prepare_continuum(continua, grid, p_full, T, dz, vmr, fn="compute_continuum_profile") -> _ContinuumJob:
    """Every refusal of a continuum set, and the per-layer coefficients of DESIGN 4.28 in the reference's order of operations."""
    members = list(continua)
    tables = [m for m in members if isinstance(m, CIATable)]
    bands = [m for m in members if isinstance(m, MTCKDBand)]
    if len(tables) + len(bands) != len(members):
        raise _lib.VSMError("%s: continua holds something that is neither a CIATable nor an MTCKDBand" % fn)
    if not members:
        raise _lib.VSMError("%s: an empty continuum set" % fn)
    if len(tables) > CONT_MAX_TABLES:
        raise _lib.VSMError("%s: %d CIA tables above %d" % (fn, len(tables), CONT_MAX_TABLES))
    if len(bands) > 1:
        raise _lib.VSMError("%s: %d MTCKDBands; a set takes one" % (fn, len(bands)))
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    for m in members:
        if not np.array_equal(grid, m.ν_grid):
            raise _lib.VSMError("%s: the grid is not the ν_grid a member of the set was built on" % fn)
    p, Tz, dzv = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (p_full, T, dz))
    Nz = len(p)
    if Nz < 1 or len(Tz) != Nz or len(dzv) != Nz:
        raise _lib.VSMError("%s: p_full, T and dz have %d, %d and %d layers" % (fn, Nz, len(Tz), len(dzv)))
    if Nz > 65535:
        raise _lib.VSMError("%s: %d layers above 65535" % (fn, Nz))
    for name, a in (("p_full", p), ("T", Tz), ("dz", dzv)):
        if not np.all(np.isfinite(a) & (a > 0)):
            raise _lib.VSMError("%s: %s must be finite and positive" % (fn, name))
    species = []
    for t in tables:
        for sp in (t.species_a, t.species_b):
            if sp not in species:
                species.append(sp)
    if bands and "H2O" not in species:
        species.append("H2O")
    vmr = dict(vmr or {})
    vs = {}
    for sp in species:
        if sp in vmr:
            v = np.asarray(vmr[sp], dtype=np.float64)
        elif sp in VMR_DEFAULTS:
            v = np.asarray(VMR_DEFAULTS[sp])
        else:
            raise _lib.VSMError('%s: no vmr for "%s" and no default defined' % (fn, sp))
        if v.ndim > 0 and v.shape != (Nz,):
            raise _lib.VSMError('%s: vmr["%s"] of shape %r is neither a scalar nor [%d]' % (fn, sp, v.shape, Nz))
        v = np.ascontiguousarray(np.broadcast_to(v, (Nz,)))
        if not np.all((v >= 0) & (v <= 1)):
            raise _lib.VSMError('%s: vmr["%s"] outside [0, 1]' % (fn, sp))
        vs[sp] = v
    nP, nTab = 4 + len(species), len(tables)
    if nP > CONT_MAX_PLANES:
        raise _lib.VSMError("%s: %d species above the %d the planes hold" % (fn, len(species), CONT_MAX_PLANES - 4))
    n_air = p * 1e2 / (k_B * Tz) * 1e-6
    dz_cm = dzv * 100.0
    rows, w = np.zeros((nTab, Nz, 2), dtype=np.int32), np.zeros((nTab, Nz))
    A, B = np.zeros((nP, nTab, Nz)), np.zeros((nP, nTab, Nz))
    for k, t in enumerate(tables):
        j0, j1, wk, inner, span = _cia_cells(t.Ts, Tz)
        rows[k, :, 0], rows[k, :, 1], w[k] = j0, j1, wk
        va, vb = vs[t.species_a], vs[t.species_b]
        prod = va * vb * n_air * n_air * dz_cm
        n2dz = n_air * n_air * dz_cm
        A[0, k] = prod
        A[1, k] = -2.0 * prod / Tz
        B[1, k] = inner * (prod / span)
        A[2, k] = 2.0 * prod / p
        if t.species_a == t.species_b:
            A[3 + species.index(t.species_a), k] = 2.0 * va * n2dz
        else:
            A[3 + species.index(t.species_a), k] = vb * n2dz
            A[3 + species.index(t.species_b), k] = va * n2dz
        A[nP - 1, k] = prod / dzv
    bl = None
    if bands:
        b, v = bands[0], vs["H2O"]
        ppr = p / b.p_ref
        S = v * p / b.p_ref * (v * n_air) * dz_cm
        F = (p - v * p) / b.p_ref * (v * n_air) * dz_cm
        bl = np.stack([Tz, b.T_ref / Tz, S, F, 2.0 * S / p, 2.0 * F / p, 2.0 * v * ppr * n_air * dz_cm,
                       (1.0 - 2.0 * v) * ppr * n_air * dz_cm, S / dzv, F / dzv], axis=1)
    return _ContinuumJob(tables=tables, band=bands[0] if bands else None, nSpec=len(grid), Nz=Nz, species=species, rows=rows, w=w,
                         A=A, B=B, band_layer=None if bl is None else np.ascontiguousarray(bl))


def _continuum_architecture(continua, architecture):
    return architecture if architecture is not None else continua[0].architecture


def compute_continuum_profile(continua, grid, p_full, T, dz, vmr, lin=False, architecture=None):
    """compute_τ_cia! and compute_τ_h2o_continuum! for a whole SET -- a list of up to 8 CIATables and at most one MTCKDBand, all built
    on `grid` -- and all layers: tau [nSpec, Nz], from ONE vsm_absorption_continuum launch and one synchronisation.  p_full [hPa], T
    [K], dz [m] per layer (layer_thickness); vmr: species -> scalar or [Nz]; "O2" and "N2" default to 0.20946 and 0.78084, any other
    species of the set that is missing raises, "H2O" with a band included.  The tables are added in list order, then the band's self
    and foreign term.
    lin=True: a ContinuumProfileLin -- tau (bit for bit the forward's), d tau / d(T, p, vmr of each species, Δz) at fixed Δz -- from
    ONE vsm_absorption_continuum_lin launch.  The T derivative of a CIA table is that of the linear interpolant in the cell the
    forward evaluates in, 0 where T is clamped to the table's range.
    Refused before any launch (VSMError): a grid that is not array_equal to a member's ν_grid, more than 8 tables, two bands, an
    empty set, p, T or dz <= 0, a vmr outside [0, 1], wrong lengths."""
    continua = list(continua)
    job = _prepare_continuum(continua, grid, p_full, T, dz, vmr)
    dev = _Device(_continuum_architecture(continua, architecture))
    if not lin:
        out = dev.empty(job.Nz, job.nSpec)
        dev.continuum(job, out, 0)
        return np.ascontiguousarray(dev.fetch([out])[0].T)
    planes = [dev.empty(job.Nz, job.nSpec) for _ in range(job.n_planes)]
    dev.continuum_lin(job, planes, [0] * job.n_planes)
    return _continuum_lin_result(job, dev.fetch(planes))


def _continuum_lin_result(job, host):
    t = [np.ascontiguousarray(h.T) for h in host]
    return ContinuumProfileLin(t[0], t[1], t[2], {sp: t[3 + i] for i, sp in enumerate(job.species)}, t[-1])
