"""vsmartmom.jl_amd -- MI355X (gfx950) engine for vSmartMOM.jl's `rt_run` CoreRT hot path.

The directory name carries a dot (it mirrors the reference's name), so it cannot
be imported with a plain `import` statement; use the shim at the repo root:

    import vsmartmom_jl_amd as vsm
    vsm.CoreRT.rt_run(model)

Sub-modules
    Architectures   CPU()/GPU() dispatch surface (src/Architectures.jl)
    CoreRT          batched_mul / batch_inv_ / elemental_ / doubling_ / interaction_ / rt_kernel_ / rt_run /
                    rt_run_multisensor (core_rt_ms: radiances at any level of the column) / rt_run_ss (core_rt_ss: the
                    single-scattering run) / rt_run_fluxes (core_rt_flux: up, down and actinic fluxes at the layer boundaries)
    host_model      host-side producers of the hot path's inputs (streams, Z moments, layer mixing)
    CoreRTLin       linearized (Jacobian) pass: rt_run(model, lin_model, ...),
                    rt_run_multisensor(model, lin_model, ..., sensor_levels) (core_rt_ms_lin: Jacobians at any level),
                    rt_run_ss(model, lin_model, ...) (core_rt_ss: analytic single-scattering Jacobians),
                    rt_run_fluxes(model, lin_model, ...) (core_rt_flux_lin: flux and heating Jacobians at the layer boundaries)
    CoreRTRaman     rotational-Raman pass: rt_run(RS_type::RRS, model, iBand),
                    rt_run_multisensor(RS_type, model, sensor_levels) (core_rt_ms_raman),
                    rt_run_fluxes(RS_type, model, levels) (core_rt_flux_raman: elastic and inelastic fluxes at the boundaries),
                    rt_run_ss(RS_type, model, iBand) (core_rt_ss: the single-scatter inelastic correction),
                    rt_run_ss_lin(RS_type, model, lin_model, ...) (core_rt_ss: its analytic Jacobians, elastic and inelastic)
    StandaloneSS    exact single scattering at the true scattering angle (standalone_ss: run_exact_ss, the four paths,
                    apply_back_correction = exact - truncated first-order field, Jacobians of paths 1 and 2)
    Scattering      Mie aerosol optics (scattering: LogNormal / TabulatedSizeDistribution, Aerosol, make_mie_model,
                    compute_aerosol_optical_properties = the Siewert NAI-2 path on the device, FP64: a size distribution and a
                    refractive index in, a host_model.AerosolOptics with k, C_ext, C_sca out; truncate_phase /
                    truncate_phase_lowconf with DeltaBGE(l_max, delta_angle) = the delta-BGE fit on the device, f_trunc = 1 - c0;
                    compute_aerosol_optical_properties_lin = linearized Mie: the same optics and a host_model.LinAerosolOptics
                    with their derivatives for (n_r, n_i, ln r_m, ln sigma_g); truncate_phase_lin /
                    compute_truncated_aerosol_optical_properties_lin = the linearized delta-BGE fit: the truncated optics and
                    their derivatives, f_trunc_dot = -c0_dot)
    Absorption      line-by-line gas absorption (absorption: HitranTable / read_hitran, Doppler / Lorentz / Voigt, three complex error
                    functions, make_hitran_model, compute_absorption_cross_section = Voigt cross-sections of a whole (p, T, vmr)
                    profile in one call on the device, FP64; compute_absorption_profile = tau_abs [nSpec, Nz] of a list of gases,
                    summed on the device, and the gas slots of LinModel.tau_abs_dot; compute_absorption_cross_section_lin /
                    compute_absorption_profile_lin = the same with the analytic T, p and vmr_self derivatives of sigma and tau_abs;
                    make_interpolation_model / InterpolationModel = the sigma(nu, p, T) lookup table, linear or cubic B-spline,
                    built, prefiltered and evaluated on the device, which every one of these calls takes in place of a line table)
    parallel        spectral-axis sharding over the GPUs of one node (torch.distributed / RCCL)
"""
from . import _lib, host_model  # noqa: F401
from . import architectures as Architectures  # noqa: F401
from . import core_rt as CoreRT  # noqa: F401
from . import core_rt_ms  # noqa: F401
from . import parallel  # noqa: F401
from . import core_rt_lin as CoreRTLin  # noqa: F401
from . import core_rt_raman as CoreRTRaman  # noqa: F401
from . import core_rt_ms_raman  # noqa: F401
from . import core_rt_ms_lin  # noqa: F401
from . import core_rt_ss  # noqa: F401
from . import core_rt_flux  # noqa: F401
from . import core_rt_flux_lin  # noqa: F401
from . import core_rt_flux_raman  # noqa: F401
from . import standalone_ss as StandaloneSS  # noqa: F401
from . import scattering as Scattering  # noqa: F401
from . import absorption as Absorption  # noqa: F401
from . import raman_inputs  # noqa: F401
from . import io_yaml  # noqa: F401
from ._lib import VSMError, LIB_PATH  # noqa: F401

CoreRT.rt_run_multisensor = core_rt_ms.rt_run_multisensor
CoreRT.MultiSensorResult = core_rt_ms.MultiSensorResult
CoreRTRaman.rt_run_multisensor = core_rt_ms_raman.rt_run_multisensor
CoreRTRaman.MultiSensorRamanResult = core_rt_ms_raman.MultiSensorRamanResult
CoreRTLin.rt_run_multisensor = core_rt_ms_lin.rt_run_multisensor
CoreRT.rt_run_ss = core_rt_ss.rt_run_ss
CoreRTRaman.rt_run_ss = core_rt_ss.rt_run_ss_rrs
CoreRTLin.rt_run_ss = core_rt_ss.rt_run_ss_lin
CoreRTRaman.rt_run_ss_lin = core_rt_ss.rt_run_ss_rrs_lin
CoreRTLin.MultiSensorLinResult = core_rt_ms_lin.MultiSensorLinResult
CoreRT.rt_run_fluxes = core_rt_flux.rt_run_fluxes
CoreRT.FluxResult = core_rt_flux.FluxResult
CoreRTLin.rt_run_fluxes = core_rt_flux_lin.rt_run_fluxes
CoreRTLin.FluxLinResult = core_rt_flux_lin.FluxLinResult
CoreRTRaman.rt_run_fluxes = core_rt_flux_raman.rt_run_fluxes
CoreRTRaman.RamanFluxResult = core_rt_flux_raman.RamanFluxResult

__version__ = "0.1.0"
