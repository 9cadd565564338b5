/*
 * vsmartmom_hip.h -- C ABI of libvsmartmom_hip.so, the MI355X (gfx950) engine for
 * vSmartMOM.jl's rt_run CoreRT hot path.
 *
 * This is the drop-in boundary: every entry point replaces one
 * method that the reference's CUDA extension defines for CuArray, or one
 * host-level CoreKernel function whose KernelAbstractions kernels the AMD
 * backend overrides.  The reference-side binding (Julia `ccall`) is shown in
 * INTEGRATION.md and julia/vSmartMOMROCmExt.jl.
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (HBM) unless the name ends in _h.
 *  - Layout is the reference's: Julia column-major. A matrix batch `A[N,N,S]`
 *    has element (i,j,s) at  i + N*j + N*N*s  (0-based); a vector batch
 *    `v[N,1,S]` has (i,s) at i + N*s. Per-spectral-point scalars are `x[S]`.
 *    Each spectral point's N*N block is contiguous; the spectral (batch) axis is
 *    the slowest, so one workgroup streams one point with fully coalesced reads.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    are asynchronous w.r.t. the host, like the CUBLAS calls they replace.
 *  - STREAM CONTRACT (every entry point that takes `stream`): all device work of
 *    a call is enqueued on `stream` and nowhere else; calls on one stream execute
 *    in call order; calls on DIFFERENT streams are independent and may be issued
 *    concurrently from one or several host threads as long as the arrays they
 *    write do not overlap.  Scratch the caller passes (`work`, `z_scratch`, ...)
 *    belongs to the call's stream until the call's work has completed.  Scratch
 *    the LIBRARY owns (the entry points marked "library scratch" below) is keyed
 *    by (current device, stream): two streams never share it, an outgrown buffer
 *    is freed only after the work queued on its stream has completed, and no
 *    call synchronises the device.  vsm_release_scratch() returns it.
 *  - DEVICE CONTRACT: a call runs on the device that is current in the calling
 *    host thread (hipSetDevice) and `stream` must belong to that device.  One
 *    process may drive several devices (one host thread per device or
 *    hipSetDevice between calls): per-kernel launch attributes and the library
 *    scratch are kept per device.  The library never calls hipSetDevice.
 *  - Return value: 0 = VSM_OK, otherwise a vsm_status; vsm_last_error() returns
 *    a thread-local message.  No C++ exception crosses this boundary.
 *  - Suffix _f64 / _f32 = the reference's `FT` (Float64 / Float32).
 *  - N = Nquad*nStokes (the reference's NquadN), S = nSpec.
 */
#ifndef VSMARTMOM_HIP_H
#define VSMARTMOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vsm_status {
  VSM_OK = 0,
  VSM_ERR_INVALID_ARG = 1,   /* bad size / null pointer */
  VSM_ERR_UNSUPPORTED = 2,   /* shape outside what the kernels are built for */
  VSM_ERR_HIP = 3,           /* a HIP runtime call failed; see vsm_last_error() */
  VSM_ERR_NO_DEVICE = 4
} vsm_status;

/* ScatteringInterface tags (src/CoreRT/types.jl ScatteringInterface_00/01/10/11;
 * selection rule src/CoreRT/tools/rt_helper_functions.jl:15-33). */
typedef enum vsm_iface {
  VSM_IFACE_00 = 0,
  VSM_IFACE_01 = 1,
  VSM_IFACE_10 = 2,
  VSM_IFACE_11 = 3
} vsm_iface;

/* ---- library / device ---------------------------------------------------- */
int vsm_version(void);                 /* 10000*major + 100*minor + patch */
const char* vsm_last_error(void);      /* thread-local, never NULL */
const char* vsm_build_id(void);        /* 16 hex digits: SHA-256 over the library's sources (csrc/Makefile); profiles name it */
int vsm_device_count(int* count);      /* Architectures.jl:68-96 `_has_cuda`-style probe */
int vsm_device_name(int device, char* buf, size_t buflen);
int vsm_sync(void* stream);            /* Architectures.synchronize_if_gpu (Architectures.jl:96) */
/* Device-side status of kernels that invert inside an asynchronous launch and therefore cannot return `info` the way
 * vsm_batch_inv does (the reference's LU raises SingularException on the host, cpu_batched.jl:32-47).  flags_h[0] = OR of the
 * vsm_devstat bits raised on the CURRENT device since the last reset; flags_h[1] = number of pivoted (Gauss-Jordan) inverses the
 * 64 < N <= 128 kernels ran (k_dbl128 / k_ia128 / k_inv1m128: every inverse whose norm bound gives no series order);
 * flags_h[2] / flags_h[3] = spectral points k_dbl128 / k_ia128 processed (which kernel family a run landed on).  SYNCHRONOUS: waits for `stream` before it reads.  reset != 0 clears the words afterwards. */
typedef enum vsm_devstat {
  VSM_DEVSTAT_SINGULAR = 1,    /* an exactly zero pivot: (I - R r) or (I - r r) is singular; the results of that point are not finite */
  VSM_DEVSTAT_NONFINITE = 2,   /* an operand of an in-kernel inverse was NaN / Inf */
  VSM_DEVSTAT_MASK = 4         /* vsm_run_layer: a phase matrix has a non-zero element outside the declared Stokes coupling (the run's
                                  `coupling`, or a block that `layer_coupling_h` called zero): that coupling was dropped, the results of
                                  the run are not those of the dense walk */
} vsm_devstat;
int vsm_device_status(int* flags_h, int reset, void* stream);
/* Frees the library-owned scratch of the CURRENT device (all streams) after a
 * device synchronisation.  Optional: the scratch is grow-only and reused. */
int vsm_release_scratch(void);
/* Largest N the fused (LDS-resident) layer kernels accept for the element size
 * (8 = f64, 4 = f32); larger N use the operator-level kernels below. */
int vsm_fused_max_n(int elem_size);

/* ---- L1 operator API: batched_mul / batch_inv! ---------------------------
 * Replace ext/gpu_batched_cuda.jl:208-233 (CUBLAS.gemm_strided_batched) and
 * :97-182 (getrf/getri batched); CPU semantics src/CoreRT/tools/cpu_batched.jl:25-82.
 * C[M,Nc,S] = A[M,K,S] * B[K,Nc,S].  A batch stride of 0 broadcasts one matrix
 * over all S (sa/sb are element strides between consecutive slices; pass M*K and
 * K*Nc for dense batches). S==1 is handled natively (no singleton-batch guard needed). */
int vsm_batched_mul_f64(int M, int Nc, int K, int S, const double* A, long long sa,
                        const double* B, long long sb, double* C, void* stream);
int vsm_batched_mul_f32(int M, int Nc, int K, int S, const float* A, long long sa,
                        const float* B, long long sb, float* C, void* stream);
/* X[:,:,s] = inv(A[:,:,s]), partial pivoting (same pivot rule as getrf). A is NOT
 * clobbered (the reference allows clobbering; callers may alias X == A).
 * info (nullable, int[S]): 0 ok, k>0 = exact zero pivot at step k (LAPACK convention). */
int vsm_batch_inv_f64(int N, int S, const double* A, double* X, int* info, void* stream);
int vsm_batch_inv_f32(int N, int S, const float* A, float* X, int* info, void* stream);

/* batch_solve!(X, A, B) (ext/gpu_batched_cuda.jl:72-94 getrf+getrs; CPU: cpu_batched.jl:25-29): X[:,:,s] = A[:,:,s] \ B[:,:,s],
 * A [N,N,S], B and X [N,Nrhs,S].  Executed as the pivoted Gauss-Jordan inverse of vsm_batch_inv into `work` (N*N*S elements)
 * followed by one batched product; A and B are not clobbered; X must not alias B.  info as in vsm_batch_inv.  (Unused on
 * the reference's forward hot path; exported because it is part of the operator API a backend extension provides.) */
int vsm_batch_solve_f64(int N, int Nrhs, int S, const double* A, const double* B, double* X, double* work, int* info,
                        void* stream);
int vsm_batch_solve_f32(int N, int Nrhs, int S, const float* A, const float* B, float* X, float* work, int* info,
                        void* stream);

/* ---- L2 CoreKernel API ----------------------------------------------------
 * Layer state containers (src/CoreRT/types.jl:155-230 AddedLayer / CompositeLayer). */
typedef struct vsm_added_f64 {
  double *r_mp, *t_pp, *r_pm, *t_mm;  /* r⁻⁺ t⁺⁺ r⁺⁻ t⁻⁻  [N,N,S] */
  double *j0_p, *j0_m;                /* j₀⁺ j₀⁻          [N,1,S] */
  long long mat_stride;               /* element stride between spectral slices of the
                                         matrices: N*N, or 0 if one matrix is shared by all S
                                         (surface layers) */
  int d_symmetric;                    /* 0: all four matrices are materialised (the reference's AddedLayer).
                                         n>0 (= nStokes): r⁺⁻/t⁻⁻ are NOT read or written; consumers derive
                                         them by the D-symmetry r⁺⁻ = D r⁻⁺ D, t⁻⁻ = D t⁺⁺ D
                                         (doubling.jl:178-201), halving the layer's HBM traffic.  Only the
                                         fused kernels accept n>0. */
  int reserved;
} vsm_added_f64;
typedef struct vsm_added_f32 {
  float *r_mp, *t_pp, *r_pm, *t_mm;
  float *j0_p, *j0_m;
  long long mat_stride;
  int d_symmetric;
  int reserved;
} vsm_added_f32;
typedef struct vsm_composite_f64 {
  double *R_mp, *R_pm, *T_pp, *T_mm;  /* R⁻⁺ R⁺⁻ T⁺⁺ T⁻⁻  [N,N,S] */
  double *J0_p, *J0_m;                /* J₀⁺ J₀⁻          [N,1,S] */
} vsm_composite_f64;
typedef struct vsm_composite_f32 {
  float *R_mp, *R_pm, *T_pp, *T_mm;
  float *J0_p, *J0_m;
} vsm_composite_f32;

/* Quadrature + polarization, as rt_kernel! sees them (QuadPoints, types.jl; pol_type.n). */
typedef struct vsm_quad_f64 {
  const double* mu;   /* qp_μN[N]  (device) */
  const double* wt;   /* wt_μN[N]  (device) */
  int N;              /* Nquad*nStokes */
  int n_stokes;       /* pol_type.n  (1..4) */
  int i_mu0;          /* 0-based node index of the SZA stream (iμ₀-1) */
  double mu0;         /* quad_points.μ₀ */
} vsm_quad_f64;
typedef struct vsm_quad_f32 {
  const float* mu;
  const float* wt;
  int N;
  int n_stokes;
  int i_mu0;
  float mu0;
} vsm_quad_f32;

/* elemental! + doubling! for one homogeneous layer and one Fourier moment m
 * (src/CoreRT/CoreKernel/elemental.jl:174-230 with kernels :289-334,:348-392,:403-422;
 *  doubling.jl:38-99 with rt_helpers.jl:102-166 and apply_D doubling.jl:178-252).
 * Inputs per spectral point: dtau[S] (= τ/2^ndoubl, rt_kernel.jl:266-287 -- ndoubl is
 * decided by the host from the batch-global max(τϖ), exactly as the reference does),
 * varpi[S], tau_sum[S] (optical depth above the layer), F0[n_stokes,S].
 * Zpp/Zmp are Z⁺⁺/Z⁻⁺ [N,N,S] with slice stride z_stride (0 = one Z for all S).
 * Fills all six fields of `added`.  ndoubl == 0 reproduces the un-doubled branch.
 * Stream: see Conventions; library scratch (doubling work of the operator-level path, N > vsm_fused_max_n). */
int vsm_elemental_doubling_f64(const vsm_quad_f64* q, int S, int m, int ndoubl,
                               const double* dtau, const double* varpi, const double* tau_sum,
                               const double* F0, const double* Zpp, const double* Zmp,
                               long long z_stride, const vsm_added_f64* added, void* stream);
int vsm_elemental_doubling_f32(const vsm_quad_f32* q, int S, int m, int ndoubl,
                               const float* dtau, const float* varpi, const float* tau_sum,
                               const float* F0, const float* Zpp, const float* Zmp,
                               long long z_stride, const vsm_added_f32* added, void* stream);

/* The two halves separately (operator-for-operator with the reference; used for
 * N above vsm_fused_max_n and by the per-kernel parity tests).  vsm_doubling_f64 with 64 < N <= 128 is ONE launch for all
 * ndoubl steps (k_dbl128); vsm_interaction_f64 (interface 11) likewise one launch (k_ia128).
 * Stream: see Conventions; vsm_doubling_f64 / vsm_interaction_f64 with 64 < N <= 128 park strips in library scratch (keyed by
 * device and stream). */
int vsm_elemental_f64(const vsm_quad_f64* q, int S, int m, int ndoubl, const double* dtau,
                      const double* varpi, const double* tau_sum, const double* F0,
                      const double* Zpp, const double* Zmp, long long z_stride,
                      const vsm_added_f64* added, void* stream);
int vsm_elemental_f32(const vsm_quad_f32* q, int S, int m, int ndoubl, const float* dtau,
                      const float* varpi, const float* tau_sum, const float* F0,
                      const float* Zpp, const float* Zmp, long long z_stride,
                      const vsm_added_f32* added, void* stream);
/* doubling!: expk[S] = exp(-dtau/μ₀) is updated in place (squared ndoubl times) like the
 * reference does.  work = scratch of vsm_doubling_work_elems(N,S) elements. */
size_t vsm_doubling_work_elems(int N, int S);
int vsm_doubling_f64(int N, int n_stokes, int S, int ndoubl, double* expk,
                     const vsm_added_f64* added, double* work, void* stream);
int vsm_doubling_f32(int N, int n_stokes, int S, int ndoubl, float* expk,
                     const vsm_added_f32* added, float* work, void* stream);

/* Non-scattering layer (rt_helpers.jl:174-180 zero_added_noscat! + rt_kernel.jl:36-45):
 * r⁻⁺ = r⁺⁻ = 0, j₀⁻ = 0, t±± = diag exp(-τ/μ).  j₀⁺ is left untouched, as in the reference. */
int vsm_noscat_layer_f64(const vsm_quad_f64* q, int S, const double* tau,
                         const vsm_added_f64* added, void* stream);
int vsm_noscat_layer_f32(const vsm_quad_f32* q, int S, const float* tau,
                         const vsm_added_f32* added, void* stream);

/* Thermal-emission source slot (`:thermal` of j₀_by_src): contribute!(::PreparedThermalEmission, ...)
 * (src/CoreRT/Sources/thermal_emission.jl:241-301) -- j₀⁺ = j₀⁻ = 2π (1-ϖ) B (1 - exp(-dτ/μᵢ)) on the Stokes-I rows of the
 * elemental layer, zero on Q/U/V; B[S] = Planck radiance of the layer per spectral point.  Written into added->j0_p / j0_m
 * AFTER vsm_elemental_* and BEFORE vsm_doubling_*, which then runs with the slot's own expk = 1 (doubling.jl:62-81). */
int vsm_thermal_source_f64(const vsm_quad_f64* q, int S, const double* dtau, const double* varpi, const double* B,
                           const vsm_added_f64* added, void* stream);
int vsm_thermal_source_f32(const vsm_quad_f32* q, int S, const float* dtau, const float* varpi, const float* B,
                           const vsm_added_f32* added, void* stream);

/* copy_added_to_composite! (rt_helpers.jl:188-200), TOA layer. */
int vsm_copy_added_to_composite_f64(int N, int S, const vsm_added_f64* added,
                                    const vsm_composite_f64* comp, void* stream);
int vsm_copy_added_to_composite_f32(int N, int S, const vsm_added_f32* added,
                                    const vsm_composite_f32* comp, void* stream);

/* interaction! (src/CoreRT/CoreKernel/interaction.jl:52-285): composite (above) ⊕ added
 * (below) -> composite, in place, statement order as in the reference.
 * work = scratch of vsm_interaction_work_elems(N,S) elements (only used when
 * N > vsm_fused_max_n; may be NULL otherwise -- and NULL beyond the fused limit = library scratch).
 * Stream: see Conventions. */
size_t vsm_interaction_work_elems(int N, int S);
int vsm_interaction_f64(int iface, int N, int S, const vsm_composite_f64* comp,
                        const vsm_added_f64* added, double* work, void* stream);
int vsm_interaction_f32(int iface, int N, int S, const vsm_composite_f32* comp,
                        const vsm_added_f32* added, float* work, void* stream);
/* Same contract, but always executed operator-for-operator (batched products + batch_inv!,
 * the way the reference issues it); work must be non-NULL.  Used for N above the fused limit
 * and as an independent cross-check of the fused kernel. */
int vsm_interaction_oplevel_f64(int iface, int N, int S, const vsm_composite_f64* comp,
                                const vsm_added_f64* added, double* work, void* stream);
int vsm_interaction_oplevel_f32(int iface, int N, int S, const vsm_composite_f32* comp,
                                const vsm_added_f32* added, float* work, void* stream);

/* create_surface_layer!(::LambertianSurfaceScalar) (src/CoreRT/Surfaces/lambertian_surface.jl:41-95).
 * Writes ONE shared N×N block into each matrix of `added` (added->mat_stride must be 0)
 * and the per-point source vectors j₀±[N,1,S] from tau_sum[S] (total column). */
int vsm_lambertian_surface_f64(const vsm_quad_f64* q, int S, int m, double albedo,
                               const double* tau_sum, const vsm_added_f64* added, void* stream);
int vsm_lambertian_surface_f32(const vsm_quad_f32* q, int S, int m, float albedo,
                               const float* tau_sum, const vsm_added_f32* added, void* stream);

/* postprocessing_vza! noRS/SFI (src/CoreRT/tools/postprocessing_vza.jl:23-94):
 *   R[v,k,s] += w[v,k] * J₀⁻[row0[v]+k, s],  T[v,k,s] += w[v,k] * J₀⁺[row0[v]+k, s]
 * R,T are [nV,n_stokes,S] column-major (v fastest); row0_h[nV] (host) = n_stokes*(iμ_v-1),
 * w_h[nV*n_stokes] (host, (v,k) at v + nV*k) = weight*{cos mφ,cos mφ,sin mφ,sin mφ}. */
int vsm_postprocess_vza_f64(int N, int n_stokes, int S, int nV, const int* row0_h,
                            const double* w_h, const double* J0_m, const double* J0_p,
                            double* R, double* T, void* stream);
int vsm_postprocess_vza_f32(int N, int n_stokes, int S, int nV, const int* row0_h,
                            const float* w_h, const float* J0_m, const float* J0_p,
                            float* R, float* T, void* stream);

/* ---- linearized (Jacobian) pass: rt_run(model, lin_model, NAer, NGas, NSurf) ----------------------
 * Derivative stacks follow the reference's layout [N,N,S,P] / [N,1,S,P] (parameter axis slowest;
 * src/CoreRT/types_lin.jl:20-97 AddedLayerLin `ap_*` fields / CompositeLayerLin). */
typedef struct vsm_added_lin_f64 {
  double *ap_r_mp, *ap_t_pp, *ap_r_pm, *ap_t_mm;  /* ap_ṙ⁻⁺ ap_ṫ⁺⁺ ap_ṙ⁺⁻ ap_ṫ⁻⁻ */
  double *ap_J0_p, *ap_J0_m;                      /* ap_J̇₀⁺ ap_J̇₀⁻ */
  int P;                                          /* Nparams */
  int reserved;
  long long mat_stride;                           /* N*N, or 0: one block per parameter shared by all S */
} vsm_added_lin_f64;
typedef struct vsm_added_lin_f32 {
  float *ap_r_mp, *ap_t_pp, *ap_r_pm, *ap_t_mm;
  float *ap_J0_p, *ap_J0_m;
  int P;
  int reserved;
  long long mat_stride;
} vsm_added_lin_f32;
typedef struct vsm_composite_lin_f64 {
  double *R_mp, *R_pm, *T_pp, *T_mm, *J0_p, *J0_m;  /* Ṙ⁻⁺ Ṙ⁺⁻ Ṫ⁺⁺ Ṫ⁻⁻ J̇₀⁺ J̇₀⁻ */
  int P;
  int reserved;
} vsm_composite_lin_f64;
typedef struct vsm_composite_lin_f32 {
  float *R_mp, *R_pm, *T_pp, *T_mm, *J0_p, *J0_m;
  int P;
  int reserved;
} vsm_composite_lin_f32;

/* elemental! (lin) = get_elem_rt_fused! + get_elem_rt_SFI_fused! (elemental_lin.jl:77-206,456-712): forward
 * r,t,j AND the chain rule to the first p_layer parameter slots.  dtau_dot[S,p_layer] = τ̇/2^ndoubl,
 * varpi_dot[S,p_layer], tau_sum_dot[S,p_layer]; Zpp_dot/Zmp_dot (nullable = 0): element (i,j,s,p) at
 * i + N*j + s*zd_stride_s + p*zd_stride_p.  All P slots of added_lin are zeroed first. */
int vsm_elemental_lin_f64(const vsm_quad_f64* q, int S, int m, int ndoubl, const double* dtau, const double* varpi,
                          const double* tau_sum, const double* F0, const double* Zpp, const double* Zmp,
                          long long z_stride, int p_layer, const double* dtau_dot, const double* varpi_dot,
                          const double* tau_sum_dot, const double* Zpp_dot, const double* Zmp_dot,
                          long long zd_stride_s, long long zd_stride_p, const vsm_added_f64* added,
                          const vsm_added_lin_f64* added_lin, void* stream);
int vsm_elemental_lin_f32(const vsm_quad_f32* q, int S, int m, int ndoubl, const float* dtau, const float* varpi,
                          const float* tau_sum, const float* F0, const float* Zpp, const float* Zmp,
                          long long z_stride, int p_layer, const float* dtau_dot, const float* varpi_dot,
                          const float* tau_sum_dot, const float* Zpp_dot, const float* Zmp_dot,
                          long long zd_stride_s, long long zd_stride_p, const vsm_added_f32* added,
                          const vsm_added_lin_f32* added_lin, void* stream);
/* vsm_elemental_lin_fold_*: vsm_elemental_lin_* (no Z_dot) for a batch with Fourier moments folded into it -- a small batch walks
 * the layers with its (moment, point) pairs as ONE batch (per-point Z: z_stride = N*N), and the moment enters elemental! only
 * through m == 0 (the weight 1/2 against 1/4, elemental_lin.jl:77-206): the first n_m0 points of the batch are pairs of m = 0, the
 * others of moments m > 0 (`m`: any of them). */
int vsm_elemental_lin_fold_f64(const vsm_quad_f64* q, int S, int m, int n_m0, int ndoubl, const double* dtau, const double* varpi,
                               const double* tau_sum, const double* F0, const double* Zpp, const double* Zmp, long long z_stride,
                               int p_layer, const double* dtau_dot, const double* varpi_dot, const double* tau_sum_dot,
                               const vsm_added_f64* added, const vsm_added_lin_f64* al, void* stream);
int vsm_elemental_lin_fold_f32(const vsm_quad_f32* q, int S, int m, int n_m0, int ndoubl, const float* dtau, const float* varpi,
                               const float* tau_sum, const float* F0, const float* Zpp, const float* Zmp, long long z_stride,
                               int p_layer, const float* dtau_dot, const float* varpi_dot, const float* tau_sum_dot,
                               const vsm_added_f32* added, const vsm_added_lin_f32* al, void* stream);
/* elemental! (lin) for a layer whose phase matrix is a per-point mix of component matrices (aerosol Jacobians): as
 * vsm_elemental_lin_* with Z = sum_{c < ncomp} fz[c, s] Zc[c] (zsel < 0) or Z = Zc[zsel] (zsel >= 0, fz unused) and
 * Z_dot[:, :, s, p] = sum_{c < ncomp_total} zdcoef[c, p, s] Zc[c]; Zc_pp / Zc_mp: [N, N, ncomp_total] blocks of one Fourier
 * moment, fz [ncomp, S], zdcoef [ncomp_total, p_layer, S] (the layer's slices of vsm_layer_optics_lin_*'s outputs).
 * ncomp_total <= 16. */
int vsm_elemental_lin_mix_f64(const vsm_quad_f64* q, int S, int m, int ndoubl, const double* dtau, const double* varpi,
                              const double* tau_sum, const double* F0, int ncomp, int ncomp_total, const double* Zc_pp,
                              const double* Zc_mp, int zsel, const double* fz, int p_layer, const double* dtau_dot,
                              const double* varpi_dot, const double* tau_sum_dot, const double* zdcoef,
                              const vsm_added_f64* added, const vsm_added_lin_f64* added_lin, void* stream);
int vsm_elemental_lin_mix_f32(const vsm_quad_f32* q, int S, int m, int ndoubl, const float* dtau, const float* varpi,
                              const float* tau_sum, const float* F0, int ncomp, int ncomp_total, const float* Zc_pp,
                              const float* Zc_mp, int zsel, const float* fz, int p_layer, const float* dtau_dot,
                              const float* varpi_dot, const float* tau_sum_dot, const float* zdcoef,
                              const vsm_added_f32* added, const vsm_added_lin_f32* added_lin, void* stream);
/* The linearized elemental thermal source (the `:thermal` slot of a linearized run; called after vsm_elemental_lin* with F0 = 0
 * and before vsm_doubling_lin_*, which then runs with the slot's expk = 1 and a zero dtau_dot table, i.e. ekl = 0).  On the
 * Stokes-I rows, x = dtau / mu_i:  j0+ = j0- = 2 pi (1 - varpi) B (1 - e^-x)  -- the bits of vsm_thermal_source_* -- and
 * ap_J0+-[p] = 2 pi B [ -varpi_dot_p (1 - e^-x) + (1 - varpi) e^-x dtau_dot_p / mu_i ]  for p < p_layer; zero on the Q/U/V rows
 * and in every slot p >= p_layer of added_lin.  dtau_dot[S,p_layer] = tau_dot / 2^ndoubl, varpi_dot[S,p_layer]. */
int vsm_thermal_source_lin_f64(const vsm_quad_f64* q, int S, const double* dtau, const double* varpi, const double* B,
                               int p_layer, const double* dtau_dot, const double* varpi_dot, const vsm_added_f64* added,
                               const vsm_added_lin_f64* added_lin, void* stream);
int vsm_thermal_source_lin_f32(const vsm_quad_f32* q, int S, const float* dtau, const float* varpi, const float* B,
                               int p_layer, const float* dtau_dot, const float* varpi_dot, const vsm_added_f32* added,
                               const vsm_added_lin_f32* added_lin, void* stream);
/* doubling_allparams! (doubling_lin.jl:216-339): forward + the first n_active parameter slots; the D-symmetry at
 * the end covers all P slots.  dtau_dot_all[S,P] (zero beyond the layer parameters); expk[S] updated in place. */
size_t vsm_doubling_lin_work_elems(int N, int S, int P);
int vsm_doubling_lin_f64(int N, int n_stokes, int S, int ndoubl, double* expk, const double* dtau_dot_all, double mu0,
                         int n_active, const vsm_added_f64* added, const vsm_added_lin_f64* added_lin, double* work,
                         void* stream);
int vsm_doubling_lin_f32(int N, int n_stokes, int S, int ndoubl, float* expk, const float* dtau_dot_all, float mu0,
                         int n_active, const vsm_added_f32* added, const vsm_added_lin_f32* added_lin, float* work,
                         void* stream);
/* interaction! (lin), ScatteringInterface_11 (interaction_lin.jl:217-331); forward composite updated as well. */
size_t vsm_interaction_lin_work_elems(int N, int S, int P);
int vsm_interaction_lin_f64(int iface, int N, int S, const vsm_composite_f64* comp, const vsm_composite_lin_f64* comp_lin,
                            const vsm_added_f64* added, const vsm_added_lin_f64* added_lin, double* work, void* stream);
int vsm_interaction_lin_f32(int iface, int N, int S, const vsm_composite_f32* comp, const vsm_composite_lin_f32* comp_lin,
                            const vsm_added_f32* added, const vsm_added_lin_f32* added_lin, float* work, void* stream);
/* The same for the parameter slots [p_lo, p_hi) only (0 <= p_lo < p_hi <= P); the other slots of comp_lin are left as they are.
 * For callers that KNOW the other slots to be zero in both operands -- the reference's loop `for iparam = 1:Nparams`
 * (interaction_lin.jl:242,291) then computes exact zeros for them: the composite above the surface does not depend on a surface
 * parameter, so rt_run's atmospheric layers need the layer slots only (n_layer_params of parameter_layout.jl) and only the
 * surface interaction needs all.  Identical results; the forward composite is updated as in vsm_interaction_lin. */
int vsm_interaction_lin_range_f64(int iface, int N, int S, const vsm_composite_f64* comp, const vsm_composite_lin_f64* comp_lin,
                                  const vsm_added_f64* added, const vsm_added_lin_f64* added_lin, int p_lo, int p_hi, double* work,
                                  void* stream);
int vsm_interaction_lin_range_f32(int iface, int N, int S, const vsm_composite_f32* comp, const vsm_composite_lin_f32* comp_lin,
                                  const vsm_added_f32* added, const vsm_added_lin_f32* added_lin, int p_lo, int p_hi, float* work,
                                  void* stream);
/* TOA copy of the derivative stacks (rt_kernel_lin.jl:148-166). */
int vsm_copy_added_to_composite_lin_f64(int N, int S, const vsm_added_lin_f64* added_lin,
                                        const vsm_composite_lin_f64* comp_lin, void* stream);
int vsm_copy_added_to_composite_lin_f32(int N, int S, const vsm_added_lin_f32* added_lin,
                                        const vsm_composite_lin_f32* comp_lin, void* stream);
/* create_surface_layer! (lin, LambertianSurfaceScalar; lambertian_surface_lin.jl:48-162).  iparam = slot of the
 * albedo (0-based); shared blocks (mat_stride 0) for the matrices of `added` and `added_lin`. */
int vsm_lambertian_surface_lin_f64(const vsm_quad_f64* q, int S, int m, double albedo, int iparam, const double* tau_sum,
                                   const double* tau_sum_dot, int p_layer, const double* F0, const vsm_added_f64* added,
                                   const vsm_added_lin_f64* added_lin, void* stream);
int vsm_lambertian_surface_lin_f32(const vsm_quad_f32* q, int S, int m, float albedo, int iparam, const float* tau_sum,
                                   const float* tau_sum_dot, int p_layer, const float* F0, const vsm_added_f32* added,
                                   const vsm_added_lin_f32* added_lin, void* stream);
/* postprocessing_vza! (lin) (postprocessing_vza_lin.jl:18-48): Rdot/Tdot [nV,n_stokes,S,P] += w * Jdot0∓. */
int vsm_postprocess_vza_lin_f64(int N, int n_stokes, int S, int nV, int P, const int* row0_h, const double* w_h,
                                const double* Jdot0_m, const double* Jdot0_p, double* Rdot, double* Tdot, void* stream);
int vsm_postprocess_vza_lin_f32(int N, int n_stokes, int S, int nV, int P, const int* row0_h, const float* w_h,
                                const float* Jdot0_m, const float* Jdot0_p, float* Rdot, float* Tdot, void* stream);

/* create_surface_layer!(::LambertianSurfaceLegendre / ::LambertianSurfaceSpline) (src/CoreRT/Surfaces/lambertian_surface.jl:97-213):
 * Lambertian surface whose albedo varies over the band, albedo[S] (device; the host evaluates the Legendre series / the spline
 * on the band grid).  One block per spectral point (added->mat_stride = N*N): r-+[:,:,s] = 2 albedo[s] E11 (x) (mu w), r+- = 0,
 * t++ = t-- = I, j0- = mu0 2 albedo[s] exp(-tau_sum/mu0) on the I rows; as in the reference j0+ = 0 and for m > 0 ALL blocks
 * (including t++ / t--) are zero. */
int vsm_lambertian_surface_spectral_f64(const vsm_quad_f64* q, int S, int m, const double* albedo, const double* tau_sum,
                                        const vsm_added_f64* added, void* stream);
int vsm_lambertian_surface_spectral_f32(const vsm_quad_f32* q, int S, int m, const float* albedo, const float* tau_sum,
                                        const vsm_added_f32* added, void* stream);
/* The same surface with K albedo Jacobian slots isurf .. isurf + K - 1 (the reference linearizes LambertianSurfaceScalar only: this
 * is the exact derivative of the builder above).  albedo[S] and basis[K][S] (device, table k contiguous over the spectral axis):
 * basis[k][s] = d albedo[s] / d x_k -- the Legendre polynomial P_k on the band grid for the coefficients of
 * LambertianSurfaceLegendre, the values of the user's basis functions for LambertianSurfaceSpline.  With n = n_stokes,
 * Rw[i, j] = [i % n == 0 and j % n == 0] mu[j] wt[j] and att_s = exp(-tau_sum[s] / mu0):
 *   m = 0, forward (what vsm_lambertian_surface_spectral_* writes, the beam weighted by F0[0, s] like the other linearized builders):
 *     r-+[:, :, s] = 2 albedo[s] Rw,  r+- = 0,  t++ = t-- = I,  j0+ = 0,  j0-[i, s] = [i % n == 0] mu0 F0[0, s] 2 albedo[s] att_s
 *   m = 0, derivatives (all six stacks of all P slots are written, zero where nothing is stated):
 *     layer slots p < p_layer (p_layer <= isurf):  ap_J0-[p][i, s] = -j0-[i, s] tau_sum_dot[p][s] / mu0, with the j0- formed here
 *       (a SurfaceSIF injected into j0- afterwards does not enter it)
 *     surface slots k < K:  ap_r-+[isurf + k][:, :, s] = 2 basis[k][s] Rw,
 *                           ap_J0-[isurf + k][i, s] = [i % n == 0] mu0 F0[0, s] 2 basis[k][s] att_s
 *   m > 0: every forward block (t++ and t-- included, the forward builder's quirk) and every derivative block is zero.
 * tau_sum_dot [S, p_layer] and F0 [n_stokes, S] as vsm_lambertian_surface_lin_* takes them.  added / added_lin: one block per
 * spectral point (mat_stride = N*N) in both.  vectors_only != 0: only j0+-, ap_J0+- are written and the matrices may be shared
 * blocks (mat_stride 0), for callers that read the vectors alone (the single-scattering run).  One thread per matrix element, the
 * row axis fastest.  VSM_ERR_INVALID_ARG before any launch: K < 1, isurf < 0, isurf + K > P, p_layer > isurf, a null table, a
 * d_symmetric layer. */
int vsm_lambertian_surface_spectral_lin_f64(const vsm_quad_f64* q, int S, int m, const double* albedo, const double* basis, int K,
                                            int isurf, const double* tau_sum, const double* tau_sum_dot, int p_layer,
                                            const double* F0, const vsm_added_f64* added, const vsm_added_lin_f64* added_lin,
                                            int vectors_only, void* stream);
int vsm_lambertian_surface_spectral_lin_f32(const vsm_quad_f32* q, int S, int m, const float* albedo, const float* basis, int K,
                                            int isurf, const float* tau_sum, const float* tau_sum_dot, int p_layer,
                                            const float* F0, const vsm_added_f32* added, const vsm_added_lin_f32* added_lin,
                                            int vectors_only, void* stream);

/* ---- BRDF surfaces: Cox-Munk ocean + the generic BRDF surface layer ------------------------------------------
 * CoxMunkSurface{FT} (src/CoreRT/types.jl:525-536); n_water is the complex index the reference's call sites use
 * (`_get_n_water(surf, 550)`, coxmunk_surface.jl:434-444: the Segelstein table at 550 nm unless the surface carries one). */
typedef struct vsm_coxmunk_f64 {
  double wind_speed, n_water_re, n_water_im, whitecap_albedo;
  int include_whitecaps, shadowing;
} vsm_coxmunk_f64;
typedef struct vsm_coxmunk_f32 {
  float wind_speed, n_water_re, n_water_im, whitecap_albedo;
  int include_whitecaps, shadowing;
} vsm_coxmunk_f32;
/* reflectance(surf, pol, qp_mu, m) and reflectance_and_deriv (coxmunk_surface.jl:381-460): the Fourier moment m of the
 * BRDF Mueller matrix over the streams of `q` (node k = q->mu[k*n_stokes]) and, if drho_dU != NULL, of its derivative
 * with respect to wind speed: rho[N,N] column-major, rho[(i n+a) + N (j n+b)] = ff/pi sum_phi w M_ab(mu_i, mu_j, phi) az_ab(m phi),
 * ff = 1 (m = 0) | 2.  phi/wphi (device, nphi <= 128) are the azimuth quadrature on [0, pi] the host hands over (the
 * reference: 100-point Gauss-Legendre, CanopyOptics.gauleg). */
int vsm_coxmunk_reflectance_f64(const vsm_coxmunk_f64* surf, const vsm_quad_f64* q, int m, int nphi, const double* phi,
                                const double* wphi, double* rho, double* drho_dU, void* stream);
int vsm_coxmunk_reflectance_f32(const vsm_coxmunk_f32* surf, const vsm_quad_f32* q, int m, int nphi, const float* phi,
                                const float* wphi, float* rho, float* drho_dU, void* stream);
/* create_surface_layer!(brdf::AbstractSurfaceType, ...) (src/CoreRT/Surfaces/rpv_surface.jl:51-97) from a Fourier
 * reflectance block rho[N,N] = reflectance(brdf, pol, qp_mu, m): r-+ = f rho diag(mu w) (f = 2 for m = 0, else 1), r+- = 0,
 * t++ = t-- = I, j0+ = I0_N exp(-tau_sum/mu0), j0- = mu0 (f rho I0_N) exp(-tau_sum/mu0).  Shared block (mat_stride 0). */
int vsm_brdf_surface_f64(const vsm_quad_f64* q, int S, int m, const double* rho, const double* tau_sum,
                         const vsm_added_f64* added, void* stream);
int vsm_brdf_surface_f32(const vsm_quad_f32* q, int S, int m, const float* rho, const float* tau_sum,
                         const vsm_added_f32* added, void* stream);
/* create_surface_layer!(::noRS, ::CoxMunkSurface, added, added_lin, iparam, ...) (coxmunk_surface_lin.jl:27-102): the same
 * with the surface-parameter derivative block drho[N,N] in slot iparam, the beam-attenuation derivatives in the first
 * p_layer slots, F0 [n_stokes,S] instead of I0, and the linearized builder's quirks (j0+ = 0, t-- = 0). */
int vsm_brdf_surface_lin_f64(const vsm_quad_f64* q, int S, int m, const double* rho, const double* drho, int iparam,
                             const double* tau_sum, const double* tau_sum_dot, int p_layer, const double* F0,
                             const vsm_added_f64* added, const vsm_added_lin_f64* added_lin, void* stream);
int vsm_brdf_surface_lin_f32(const vsm_quad_f32* q, int S, int m, const float* rho, const float* drho, int iparam,
                             const float* tau_sum, const float* tau_sum_dot, int p_layer, const float* F0,
                             const vsm_added_f32* added, const vsm_added_lin_f32* added_lin, void* stream);
/* Kernel-driven land BRDFs with analytic parameter derivatives (the reference linearizes neither surface).
 * kind = VSM_LAND_BRDF_RPV: rpvSurfaceScalar (types.jl:482-491), params (host) = {rho0, rho_c, k, Theta}, K = 4;
 * kind = VSM_LAND_BRDF_ROSSLI: RossLiSurfaceScalar (types.jl:505-512), params (host) = {fvol, fgeo, fiso}, K = 3.
 * For every Fourier moment m = 0 .. m_max, in one launch: rho[m][N,N] = reflectance(brdf, pol, qp_mu, m) (rpv_surface.jl:160-190:
 * ff/pi sum_phi w rho(mu_i, mu_j, phi) cos(m phi) on the I -> I elements, ff = 1 (m = 0) | 2; the m = 0 block is NOT doubled) and
 * drho[m][k][N,N], its derivative with respect to parameter k (field order), both column-major blocks like
 * vsm_coxmunk_reflectance_*'s.  phi / wphi (device, nphi nodes): the azimuth quadrature on [0, pi]. */
#define VSM_LAND_BRDF_RPV 0
#define VSM_LAND_BRDF_ROSSLI 1
int vsm_land_brdf_reflectance_lin_f64(const vsm_quad_f64* q, int kind, const double* params, int m_max, int nphi, const double* phi,
                                      const double* wphi, double* rho, double* drho, void* stream);
int vsm_land_brdf_reflectance_lin_f32(const vsm_quad_f32* q, int kind, const float* params, int m_max, int nphi, const float* phi,
                                      const float* wphi, float* rho, float* drho, void* stream);
/* vsm_brdf_surface_lin_* for a surface with K parameters: drho[K][N,N], slot isurf + k takes ap_r-+ = (f drho_k) diag(mu w) and
 * ap_J0- = mu0 sum_s (f drho_k)[:, i0 + s] F0_s exp(-tau_sum/mu0); all other blocks of the surface slots are zero; the layer slots
 * [0, p_layer), p_layer <= isurf, carry -j0- tau_sum_dot / mu0; j0+ = 0, t-- = 0 as in the one-slot builder. */
int vsm_brdf_surface_lin_multi_f64(const vsm_quad_f64* q, int S, int m, const double* rho, const double* drho, int K, int isurf,
                                   const double* tau_sum, const double* tau_sum_dot, int p_layer, const double* F0,
                                   const vsm_added_f64* added, const vsm_added_lin_f64* added_lin, void* stream);
int vsm_brdf_surface_lin_multi_f32(const vsm_quad_f32* q, int S, int m, const float* rho, const float* drho, int K, int isurf,
                                   const float* tau_sum, const float* tau_sum_dot, int p_layer, const float* F0,
                                   const vsm_added_f32* added, const vsm_added_lin_f32* added_lin, void* stream);
/* SurfaceSIF (src/CoreRT/Sources/surface_sif.jl:168-179; the same statement as inject_surface_SIF!, Surfaces/lambertian_surface.jl:
 * 239-254): hemispheric isotropic emission at the lower boundary, applied to the surface AddedLayer AFTER its builder
 * (vsm_lambertian_surface_* / vsm_lambertian_surface_spectral_*) and BEFORE the surface interaction, at Fourier moment m = 0 only:
 *   j0_m[i n_stokes + c, s] += 2 sif[c, s]     for every stream i and Stokes component c
 * sif: DEVICE array [n_stokes][S] (the spectral axis contiguous).  Only added_surface->j0_m ([N,1,S], per point whether the
 * layer's matrices are shared or not) is read and written; one thread per (row, point).  The caller carries the no-op rules
 * (m > 0, an all-zero table, a non-Lambertian surface: no call). */
int vsm_surface_sif_f64(int N, int n_stokes, int S, const double* sif, const vsm_added_f64* added_surface, void* stream);
int vsm_surface_sif_f32(int N, int n_stokes, int S, const float* sif, const vsm_added_f32* added_surface, void* stream);

/* SurfaceEmission (ours; the reference has no surface thermal source): thermal emission of the lower boundary, applied to the surface
 * AddedLayer of the `:thermal` slot AFTER its builder and BEFORE the surface interaction, at Fourier moment m = 0 only (m > 0:
 * VSM_OK, nothing launched).  B_surface: DEVICE array [S], the Planck radiance of the skin in the units of vsm_thermal_source_*'s B.
 * emissivity == NULL (Kirchhoff): for every row (stream i, Stokes component c, n = n_stokes) and point s
 *   j0_m[i n + c, s] += 2 pi B_surface[s] ( delta_{c,0} - sum_j r_mp[i n + c, j n, s] )
 * -- the sum over the I column of every stream j: the surface builders fold 2 mu_j w_j into column j at m = 0, so it is the
 * directional-hemispherical reflectance of that row for unpolarized isotropic illumination, zero-weight rows included.
 * emissivity: DEVICE array [S]: the bracket is delta_{c,0} emissivity[s] (isotropic, unpolarized).
 * added_surface->r_mp is read with mat_stride 0 (one shared block) or N*N (one per point), j0_m [N,1,S] is read and written,
 * nothing else is touched; one thread per (row, point).  S = 0: VSM_OK. */
int vsm_surface_emission_f64(int N, int n_stokes, int S, int m, const double* B_surface, const double* emissivity,
                             const vsm_added_f64* added_surface, void* stream);
int vsm_surface_emission_f32(int N, int n_stokes, int S, int m, const float* B_surface, const float* emissivity,
                             const vsm_added_f32* added_surface, void* stream);
/* The derivative of the Kirchhoff emission in the K surface slots isurf .. isurf + K - 1 of the linearized surface layer, after its
 * builder, m = 0 only:  ap_J0_m[p][i n + c, s] += -2 pi B_surface[s] sum_j ap_r_mp[p][i n + c, j n, s].  An explicit emissivity
 * depends on no parameter (no call); the layer slots need nothing here (the linearized interaction differentiates the propagation
 * of the forward j0_m).  al->mat_stride 0 or N*N as in the forward layer. */
int vsm_surface_emission_lin_f64(int N, int n_stokes, int S, int m, const double* B_surface, int isurf, int K,
                                 const vsm_added_lin_f64* added_surface_lin, void* stream);
int vsm_surface_emission_lin_f32(int N, int n_stokes, int S, int m, const float* B_surface, int isurf, int K,
                                 const vsm_added_lin_f32* added_surface_lin, void* stream);

/* interaction_hdrf! (src/CoreRT/CoreKernel/interaction_hdrf.jl:4-42), called after the surface interaction of each Fourier
 * moment (rt_run.jl:467-476): hdr_J[N,S] = r-+_surf J0+ + j0-_surf; for m == 0 also the hemispheric fluxes bhr_uw / bhr_dw
 * [n_stokes, S] (for m > 0 they are not touched).  The surface layer may be shared (mat_stride 0) or per point. */
int vsm_interaction_hdrf_f64(const vsm_quad_f64* q, int S, int m, const vsm_composite_f64* comp,
                             const vsm_added_f64* added_surface, double* hdr_J, double* bhr_uw, double* bhr_dw, void* stream);
int vsm_interaction_hdrf_f32(const vsm_quad_f32* q, int S, int m, const vsm_composite_f32* comp,
                             const vsm_added_f32* added_surface, float* hdr_J, float* bhr_uw, float* bhr_dw, void* stream);
/* postprocessing_vza_hdrf! (tools/postprocessing_vza.jl:103-115): hdr[v,k,s] += w[v,k] hdr_J[row0[v]+k, s]; row0_h / w_h as in
 * vsm_postprocess_vza_*. */
int vsm_postprocess_vza_hdrf_f64(int N, int n_stokes, int S, int nV, const int* row0_h, const double* w_h, const double* hdr_J,
                                 double* hdr, void* stream);
int vsm_postprocess_vza_hdrf_f32(int N, int n_stokes, int S, int nV, const int* row0_h, const float* w_h, const float* hdr_J,
                                 float* hdr, void* stream);
/* apply_ss_correction! (TMS; coxmunk_surface.jl:481-569, called at rt_run.jl:520-524):
 *   coef[v + nV k] = M_exact[k,1](mu_v, mu0, dphi_v) - sum_{m<=m_max} w_m az_k1(m dphi_v) c_m[k,1](mu_v, mu0)
 *   R_SFI[v,k,s]  += mu0 exp(-tau_total[s]/mu0) coef[v + nV k]
 * mu_v_h / dphi_h: host arrays [nV] (cos of the viewing zenith, relative azimuth in radians); coef: device [nV*n_stokes]
 * (output); R_SFI [nV,n_stokes,S] may be NULL (coefficients only). */
int vsm_coxmunk_ss_correction_f64(const vsm_coxmunk_f64* surf, int n_stokes, int S, int nV, const double* mu_v_h,
                                  const double* dphi_h, double mu0, int m_max, int nphi, const double* phi,
                                  const double* wphi, const double* tau_total, double* coef, double* R_SFI, void* stream);
int vsm_coxmunk_ss_correction_f32(const vsm_coxmunk_f32* surf, int n_stokes, int S, int nV, const float* mu_v_h,
                                  const float* dphi_h, float mu0, int m_max, int nphi, const float* phi, const float* wphi,
                                  const float* tau_total, float* coef, float* R_SFI, void* stream);
/* The two terms of that coefficient on their own, for StandaloneSS path 2 (surfaces.jl:88-106, truncated.jl:116-184):
 *   exact[v + nV k] = M[k,1](mu_v, mu0, dphi_v),   trunc[v + nV k] = sum_{m < m_count} w_m az_k1(m dphi_v) c_m[k,1](mu_v, mu0)
 * (device [nV*n_stokes] each, either may be NULL), by the same kernel and the same Mueller function.  Any nV >= 1. */
int vsm_coxmunk_first_column_f64(const vsm_coxmunk_f64* surf, int n_stokes, int nV, const double* mu_v_h, const double* dphi_h,
                                 double mu0, int m_count, int nphi, const double* phi, const double* wphi, double* exact,
                                 double* trunc, void* stream);
int vsm_coxmunk_first_column_f32(const vsm_coxmunk_f32* surf, int n_stokes, int nV, const float* mu_v_h, const float* dphi_h,
                                 float mu0, int m_count, int nphi, const float* phi, const float* wphi, float* exact, float* trunc,
                                 void* stream);

/* ---- per-scene layer optics on the device ---------------------------------------------------
 * The reference builds these on the host once per Fourier moment (rt_run.jl:390-394) and ships per-layer arrays inside
 * the layer loop (expandOpticalProperties, compEffectiveLayerProperties.jl:106-117).  Here the raw optical depths are
 * uploaded once per scene and the inputs of the layer kernels are produced in HBM.
 *
 * compute_Z_moments(pol, mu, greek_coefs, m) (src/Scattering/compute_Z_matrices.jl:26-110): Z++ / Z-+ [N,N] over the
 * streams of `q` (node k = q->mu[k*n_stokes]) from the Greek coefficients greek[6*lmax] = alpha | beta | gamma | delta |
 * epsilon | zeta (device, FP64), each of length lmax. */
int vsm_compute_Z_moments_f64(const vsm_quad_f64* q, int m, int lmax, const double* greek, double* Zpp, double* Zmp,
                              void* stream);
int vsm_compute_Z_moments_f32(const vsm_quad_f32* q, int m, int lmax, const double* greek, float* Zpp, float* Zmp,
                              void* stream);
/* constructCoreOpticalProperties + extractEffectiveProps (compEffectiveLayerProperties.jl:11-93) for one band, noRS:
 * Rayleigh (tau_rayl[S,L], varpi_cabannes) + nAer aerosols (tau_aer[nAer,L], ssa[nAer], ftrunc[nAer]; createAero delta-M
 * scaling :67-72) + absorption (tau_abs[S,L]); arrays are the reference's column-major [nSpec, Nz] ((s,l) at s + S*l), all
 * device pointers, FP64 inputs.  mode[nAer,L] (int, (ia,l) at ia + nAer*l) resolves the batch-global branches of the
 * mixing `+` (types.jl:1262-1292): 0 = per-point mix, 1 = no point scatters before this aerosol (take its Z),
 * 2 = the aerosol does not scatter (keep Z).  Outputs: tau, varpi [S,L]; tau_sum [S,L+1] (column l = optical depth above
 * layer l, column L = total); fcomp (nullable) [nAer+1, S, L] per-point weights of the component phase matrices
 * (Rayleigh, aerosol 1, ...) as consumed by vsm_layer_forward_mix_*; max_tau_varpi[L] = maximum(tau .* varpi) per layer
 * (rt_kernel.jl:197,282 -- the host turns it into ndoubl and the scattering-interface tags). */
int vsm_layer_optics_f64(int S, int L, int nAer, const double* tau_rayl, const double* tau_abs, double varpi_cabannes,
                         const double* tau_aer, const double* ssa, const double* ftrunc, const int* mode, double* tau,
                         double* varpi, double* tau_sum, double* fcomp, double* max_tau_varpi, void* stream);
int vsm_layer_optics_f32(int S, int L, int nAer, const double* tau_rayl, const double* tau_abs, double varpi_cabannes,
                         const double* tau_aer, const double* ssa, const double* ftrunc, const int* mode, float* tau,
                         float* varpi, float* tau_sum, float* fcomp, float* max_tau_varpi, void* stream);
/* dtau[S,L] = tau ./ 2^ndoubl[l] (get_dtau_ndoubl, rt_kernel.jl:266-287); ndoubl: device int[L]. */
int vsm_layer_dtau_f64(int S, int L, const int* ndoubl, const double* tau, double* dtau, void* stream);
int vsm_layer_dtau_f32(int S, int L, const int* ndoubl, const float* tau, float* dtau, void* stream);
/* constructCoreOpticalProperties with lin_model (compEffectiveLayerProperties_lin.jl:43-197; createAero with derivatives
 * :330-395; quotient rule of the pairwise `+`, types_lin.jl:196-380) for the rank's block [lo, lo + S) of a band of S_full
 * points: the derivatives of the layer optics with respect to the pl = 7 nAer + nGas layer parameters (slot order of
 * parameter_layout.jl:28-56: per aerosol tau_ref, n_r, n_i, r_m, sigma_r, p0, sigma_p; then the gases).  Inputs (device, FP64,
 * indexed on the FULL axis): tau_rayl, tau_abs [S_full, L]; tau_aer [nAer, L]; ssa, ftrunc [nAer]; tau_abs_dot [S_full, L, nGas]
 * (lin_model.tau_abs_dot); tau_aer_dot [7, nAer, L] (lin_model.tau_aer_dot); ssa_dot, ftrunc_dot [4, nAer]
 * (lin_aerosol_optics: d/d(n_r, n_i, r_m, sigma_r)); ndoubl: device int[L].  Outputs (block-local, column-major):
 * dtau_dot_all [S, P, L] = tau_dot / 2^ndoubl (columns >= pl zero: the surface slots of doubling_allparams!),
 * varpi_dot [S, pl, L], tau_sum_dot [S, pl, L+1] (layer l: derivative of the optical depth above it; L: total), and for
 * nAer > 0 the per-point weights fz [nAer+1, S, L] of the component phase matrices in Z and the coefficients
 * zdcoef [CT, pl, S, L] of Z_dot over the CT = (nAer+1) + 4 nAer component blocks
 * [Z_Rayleigh, Z_aer1.., dZ_aer1/d(n_r, n_i, r_m, sigma_r), dZ_aer2/d.., ..] -- Z_dot itself is never materialised
 * (vsm_elemental_lin_mix_* forms it where it is consumed). */
int vsm_layer_optics_lin_f64(int S_full, int lo, int S, int L, int nAer, int nGas, int P, const double* tau_rayl,
                             const double* tau_abs, double varpi_cabannes, const double* tau_aer, const double* ssa,
                             const double* ftrunc, const double* tau_abs_dot, const double* tau_aer_dot,
                             const double* ssa_dot, const double* ftrunc_dot, const int* ndoubl, double* dtau_dot_all,
                             double* varpi_dot, double* tau_sum_dot, double* fz, double* zdcoef, void* stream);
int vsm_layer_optics_lin_f32(int S_full, int lo, int S, int L, int nAer, int nGas, int P, const double* tau_rayl,
                             const double* tau_abs, double varpi_cabannes, const double* tau_aer, const double* ssa,
                             const double* ftrunc, const double* tau_abs_dot, const double* tau_aer_dot,
                             const double* ssa_dot, const double* ftrunc_dot, const int* ndoubl, float* dtau_dot_all,
                             float* varpi_dot, float* tau_sum_dot, float* fz, float* zdcoef, void* stream);
/* expk[S] = exp(-dtau / mu0) (init_layer, rt_kernel.jl:339-349); doubling! squares it in place. */
int vsm_layer_expk_f64(int S, const double* dtau, double mu0, double* expk, void* stream);
int vsm_layer_expk_f32(int S, const float* dtau, float mu0, float* expk, void* stream);

/* rt_kernel!(::noRS) for ONE scattering layer (src/CoreRT/CoreKernel/rt_kernel.jl:175-250): elemental! + doubling!
 * followed by copy_added_to_composite! (toa != 0, i.e. iz == 1; rt_helpers.jl:188-200) or
 * interaction!(::ScatteringInterface_11) (interaction.jl:207-266).  Arguments as vsm_elemental_doubling_*.
 * FP64 with 32 < N <= 64 (and FP32 with 64 < N <= 96) runs as a pre-pass + ONE launch whose added layer never leaves the chip
 * (`added_scratch` is then not touched and may be NULL); other shapes run elemental / doubling / interaction as separate
 * launches through `added_scratch` -- FP64 with 64 < N <= 128: the whole doubling loop and the interaction of a point each in
 * one persistent workgroup (vsm_strip128.hip).
 * Stream: see Conventions; library scratch (the pre-pass images of the layer; parked strips for 64 < N <= 128). */
int vsm_layer_forward_f64(const vsm_quad_f64* q, int S, int m, int ndoubl, const double* dtau, const double* varpi,
                          const double* tau_sum, const double* F0, const double* Zpp, const double* Zmp, long long z_stride,
                          int toa, const vsm_composite_f64* comp, const vsm_added_f64* added_scratch, void* stream);
int vsm_layer_forward_f32(const vsm_quad_f32* q, int S, int m, int ndoubl, const float* dtau, const float* varpi,
                          const float* tau_sum, const float* F0, const float* Zpp, const float* Zmp, long long z_stride,
                          int toa, const vsm_composite_f32* comp, const vsm_added_f32* added_scratch, void* stream);

/* vsm_layer_forward(_mix)_* for nm Fourier moments of ONE layer (the moments of rt_run's outer loop, rt_run.jl:383, are
 * independent until post-processing): m[nm] (host), Zpp[nm] / Zmp[nm] (host arrays of device pointers: the moment's Z block or
 * component stack), comps[nm] (host array: one CompositeLayer per moment); dtau, varpi, tau_sum, F0, fcomp, ndoubl are the
 * layer's and shared.  FP64 with 32 < N <= 60 runs the moments in ONE launch (three times the workgroups per launch: a third of
 * the launch tails); other shapes run vsm_layer_forward(_mix) moment by moment through `added_scratch` / `z_scratch`.
 * Stream: see Conventions; library scratch as vsm_layer_forward_*. */
int vsm_layer_forward_multi_f64(const vsm_quad_f64* q, int S, int nm, const int* m, int ndoubl, const double* dtau,
                                const double* varpi, const double* tau_sum, const double* F0, int ncomp,
                                const double* const* Zpp, const double* const* Zmp, long long z_stride, const double* fcomp,
                                double* z_scratch, int toa, const vsm_composite_f64* comps, const vsm_added_f64* added_scratch,
                                void* stream);
int vsm_layer_forward_multi_f32(const vsm_quad_f32* q, int S, int nm, const int* m, int ndoubl, const float* dtau,
                                const float* varpi, const float* tau_sum, const float* F0, int ncomp, const float* const* Zpp,
                                const float* const* Zmp, long long z_stride, const float* fcomp, float* z_scratch, int toa,
                                const vsm_composite_f32* comps, const vsm_added_f32* added_scratch, void* stream);

/* The `:thermal` per-source slot of one scattering layer (rt_kernel.jl:205-232: contribute!(::PreparedThermalEmission)
 * between elemental! and doubling!, Sources/thermal_emission.jl:241-301; the slot's own expk = 1, doubling.jl:62-81; the
 * per-source recurrences of interaction.jl) in the launch of vsm_layer_forward(_mix)_*: m = 0, the solar source replaced by
 * j0+- = 2 pi (1 - varpi) B (1 - exp(-dtau/mu_i)) on the I rows, thermal_B[S] = Planck radiance of the layer per point.
 * ncomp = 0: Zpp / Zmp [N,N,S] with z_stride (0 = shared block); ncomp >= 1: component stacks [N,N,ncomp] + fcomp[ncomp,S].
 * `comp` is the composite of the thermal slot.  Fused for FP64 with 32 < N <= 60 and FP32 with 64 < N <= 96, ncomp <= 4
 * (vsm_layer_thermal_fused(N, is_f64) != 0); any other shape returns VSM_ERR_UNSUPPORTED (callers then run
 * vsm_elemental + vsm_thermal_source + vsm_doubling + vsm_interaction). */
int vsm_layer_thermal_fused(int N, int is_f64);
int vsm_layer_forward_thermal_f64(const vsm_quad_f64* q, int S, int ndoubl, const double* dtau, const double* varpi,
                                  const double* thermal_B, int ncomp, const double* Zpp, const double* Zmp, long long z_stride,
                                  const double* fcomp, int toa, const vsm_composite_f64* comp, void* stream);
int vsm_layer_forward_thermal_f32(const vsm_quad_f32* q, int S, int ndoubl, const float* dtau, const float* varpi,
                                  const float* thermal_B, int ncomp, const float* Zpp, const float* Zmp, long long z_stride,
                                  const float* fcomp, int toa, const vsm_composite_f32* comp, void* stream);

/* Layer optics with several scatterers: the reference mixes Z per spectral point on the host,
 * Z = sum_k (tau_k varpi_k Z_k) / sum_k (tau_k varpi_k)  (`+` of CoreScatteringOpticalProperties, src/CoreRT/types.jl:1262-1292;
 * compEffectiveLayerProperties.jl:43-54) and ships [N,N,nSpec] arrays to the device.  Here the ncomp component
 * matrices Zpp_comp / Zmp_comp [N,N,ncomp] (one stack per Fourier moment) and the per-point weights fcomp [ncomp,S]
 * (fcomp[k + ncomp*s]) are handed over instead.
 * vsm_layer_forward_mix_*: as vsm_layer_forward_*, mixing Z where the elemental step consumes it (fused strip kernel,
 *   ncomp <= 4); other shapes materialise Z into z_scratch (2*N*N*S elements; NULL = library scratch) first.
 * vsm_mix_Z_*: the materialising kernel on its own: Zpp/Zmp [N,N,S]. */
int vsm_layer_forward_mix_f64(const vsm_quad_f64* q, int S, int m, int ndoubl, const double* dtau, const double* varpi,
                              const double* tau_sum, const double* F0, int ncomp, const double* Zpp_comp,
                              const double* Zmp_comp, const double* fcomp, double* z_scratch, int toa,
                              const vsm_composite_f64* comp, const vsm_added_f64* added_scratch, void* stream);
int vsm_layer_forward_mix_f32(const vsm_quad_f32* q, int S, int m, int ndoubl, const float* dtau, const float* varpi,
                              const float* tau_sum, const float* F0, int ncomp, const float* Zpp_comp, const float* Zmp_comp,
                              const float* fcomp, float* z_scratch, int toa, const vsm_composite_f32* comp,
                              const vsm_added_f32* added_scratch, void* stream);
int vsm_mix_Z_f64(int N, int S, int ncomp, const double* Zpp_comp, const double* Zmp_comp, const double* fcomp, double* Zpp,
                  double* Zmp, void* stream);
int vsm_mix_Z_f32(int N, int S, int ncomp, const float* Zpp_comp, const float* Zmp_comp, const float* fcomp, float* Zpp,
                  float* Zmp, void* stream);
/* vsm_mix_Z_moments_*: the same for nm <= 24 Fourier moments of one layer in one launch, the moments folded into the batch axis
 * (the layer walk of a small batch takes its moments as ONE batch: rt_kernel!'s arguments of layer iz for (moment, point) pairs):
 * Zpp_comp_h / Zmp_comp_h[nm] = HOST arrays of device pointers to the moments' component stacks [N,N,ncomp]; block im * S + s of
 * Zpp / Zmp [N,N,nm*S] = sum_k fcomp[k + ncomp*s] Z_k(moment im).  ncomp = 0: a layer with one scatterer -- block `single` of
 * every stack, copied (fcomp unused). */
int vsm_mix_Z_moments_f64(int N, int S, int ncomp, int nm, const double* const* Zpp_comp_h, const double* const* Zmp_comp_h, int single,
                          const double* fcomp, double* Zpp, double* Zmp, void* stream);
int vsm_mix_Z_moments_f32(int N, int S, int ncomp, int nm, const float* const* Zpp_comp_h, const float* const* Zmp_comp_h, int single,
                          const float* fcomp, float* Zpp, float* Zmp, void* stream);

/* ---- a run with the CompositeLayer in kernel-native layout ---------------------
 * The layer loop of rt_run (src/CoreRT/rt_run.jl:383-453: `for iz = 1:Nz ... rt_kernel!(RS_type, pol_type, SFI, added_layer,
 * composite_layer, ...)`) reads and writes the CompositeLayer (make_composite_layer, tools/rt_helper_functions.jl:259-270;
 * allocated once per run, rt_run.jl:326-335) in every layer step, and nothing else touches it until the surface interaction
 * (rt_run.jl:455-470).  A vsm_run is that CompositeLayer for nm Fourier moments of S points, kept in the layer kernels' own
 * strip layout for the whole loop:
 *   vsm_run_create   = make_composite_layer (the storage is the caller's `workspace`: vsm_run_workspace_bytes bytes, 16-byte
 *                      aligned device memory that must outlive the run; q->mu / q->wt must outlive it too)
 *   vsm_run_layer    = rt_kernel!(::noRS) for ONE scattering layer and all nm moments (rt_kernel.jl:175-250: elemental! +
 *                      doubling! + interaction!(::ScatteringInterface_11), or copy_added_to_composite! when toa != 0); arguments as
 *                      vsm_layer_forward_multi_f64 (Zpp[nm] / Zmp[nm]: host arrays of device pointers, ncomp <= 4)
 *   vsm_run_export   = the composite as the reference's arrays (comps[nm]: one CompositeLayer per moment), for the surface
 *                      step and postprocessing_vza!; vsm_run_import is the inverse (a run that continues from existing arrays)
 *   vsm_run_destroy  frees the host-side handle only.
 * Stokes blocks.  `coupling[nm]` (NULL or -1 per moment = dense) tells per moment which Stokes components the phase matrices
 * couple: bit 4 a + b set = some element Z[i, j] with i % n_stokes == a, j % n_stokes == b is non-zero.  Components that do not
 * couple run as independent sub-problems (for m = 0 every phase matrix has exactly zero (I,Q) x (U,V) blocks,
 * src/Scattering/compute_Z_matrices.jl:26-110: N = 60, n_stokes = 3 runs as 40 x 40 + 20 x 20) -- products with exact zeros are
 * not formed, results are those of the dense run.  The mask MUST cover every Z later handed to vsm_run_layer (every call checks
 * the layer's matrices against the masks on the device and raises VSM_DEVSTAT_MASK, vsm_device_status, on a violation):
 * vsm_stokes_coupling_f64 computes one mask per matrix of a stack of `nblocks` matrices on the device (mask_d[nblocks]: DEVICE
 * ints, written asynchronously on `stream`); OR the masks of all scatterers of a moment.
 * `layer_coupling_h[nm]` of vsm_run_layer (NULL = the run's) is the same mask for the phase matrices of THIS layer (the OR over the
 * scatterers present in it): a block the layer's phase matrices leave exactly zero (U at m = 0 in a Rayleigh layer; any block of
 * a Rayleigh-only layer at m >= 3, where the Rayleigh phase matrix vanishes) has r = 0, j = 0, t = diag(exp(-tau / mu)) and its
 * interaction is a scaling of the composite's rows and columns -- one elementwise pass instead of the products.
 * Every block of coupled components must fit the native
 * kernels: (N / n_stokes) * (components in the block) <= 64 (vsm_run_supported != 0), else VSM_ERR_UNSUPPORTED.
 * _f32: the same for a Float32 model in the model's own float type, as the reference runs it (doubling.jl:38-131 and
 * interaction.jl:207-266 compute in FT): the caller's arrays, the native records and the arithmetic (v_mfma_f32_16x16x4_f32) are
 * single precision, blocks of up to 128 rows (vsm_run_supported_f32; workspace: vsm_run_workspace_bytes_f32 -- half of
 * vsm_run_workspace_bytes, which stays sufficient).  A run is used with the entry points of its own type.
 * Sources-only runs.  vsm_run_create_ex_* with flags = VSM_RUN_SOURCES_ONLY creates a run for callers that read only R+-, T--,
 * J0+ and J0- of the composite (rt_run's SFI outputs: R_SFI, T_SFI, hdr and bhr read J0+- after the surface step, whose own
 * R+-, T--, J0+- depend on the composite's R+-, T--, J0+- alone).  Its layer steps neither read nor write R-+ and T++ (five
 * products fewer per interaction, half the composite traffic); vsm_run_export writes R-+ and T++ as quiet NaNs -- they are
 * UNDEFINED, and everything derived from them (the R-+ and T++ of a later interaction) is too.  R+-, T--, J0+- equal those of a
 * full run up to rounding (the interaction is re-associated around (I - r-+ R+-)^-1).  FP64 runs only: an _f32 run accepts the
 * flag and keeps the full recurrences.  vsm_run_create_* = vsm_run_create_ex_* with flags = 0 (the full composite).
 * Zero-weight tail.  flags |= VSM_RUN_ZW_TAIL (or vsm_run_zw_tail(run) before the run's first layer step: the same): the library
 * reads q->wt once (a synchronous copy on the legacy stream -- not while a stream is being captured into a graph), and
 * finds the trailing run of quadrature nodes whose weight is exactly 0 (rt_set_streams appends the VZA and SZA nodes behind the
 * Gauss-Legendre nodes with weight 0; a zero weight elsewhere does not count).  Their streams are the last rows of every block
 * (rows are node-major), and every matrix the layer steps form has their columns zero off the diagonal (elemental! gives r a zero
 * column and t a diagonal one there; sums, products and the inverses keep that): the products of the layer steps skip the k-steps
 * that cover only such streams and add their diagonal terms lane by lane instead.  Per block: real rows = (real nodes) x (components
 * of the block), k-steps formed = ceil(real rows / 4).  No trailing zero-weight node (e.g. a VZA that is a Gauss-Legendre node):
 * the dense products, bit for bit.  The composite must then come from this run's own layer steps: vsm_run_import drops the flag
 * for the rest of the run (a caller's arrays need not have those zero columns).  R+-, T--, J0+- (and R-+, T++ of a full run) equal
 * those of a run without the flag up to rounding.  FP64 runs only: an _f32 run accepts the flag and ignores it.
 * Viewing rows.  A sources-only run whose caller reads T-- and J0- in a few rows alone: rt_run's SFI outputs after a surface step,
 * where T-- enters only as the left operand of T01_inv = T-- G1 (row i of it and of the new J0- needs row i of T-- and J0- only,
 * interaction.jl:207-266), postprocessing_vza! reads J0- at the n_stokes rows of each VZA node, and interaction_hdrf! reads J0+
 * alone.  Two equal ways to create one: vsm_run_create_view_* with flags = VSM_RUN_SOURCES_ONLY | VSM_RUN_VIEW_ROWS and rows_h[nrows]
 * (global rows 0 .. N - 1, distinct, 1 <= nrows <= VSM_RUN_VIEW_MAX), or vsm_run_view_rows(run, nrows, rows_h) on a sources-only
 * run before its first layer step and before any vsm_run_import.  The flag is valid only with VSM_RUN_SOURCES_ONLY; vsm_run_create_ex_*
 * with it has no list and is refused, as is a list that is empty or too long (no silent fallback).  The layer steps carry T-- as
 * nrows row vectors: they pass through the product T-- W as ONE row tile (1 / RT of the product's MFMAs) and J0- is updated in
 * those rows only; the full T-- record is neither read nor written.  Every element goes through the operations of the full
 * product, so T-- and J0- in the viewing rows, R+- and J0+ equal those of a plain sources-only run bit for bit.  vsm_run_export
 * writes T-- and J0- valid in the viewing rows and quiet NaN elsewhere (undefined, never stale); vsm_run_import reads T-- and J0-
 * in the viewing rows only.  FP64 runs only: an _f32 run accepts the calls and keeps the full recurrences.
 * Viewing rows.  vsm_run_create_view_* with flags = VSM_RUN_SOURCES_ONLY | VSM_RUN_VIEW_ROWS (the second flag is valid only with the
 * first and only through this entry point) and rows_h[nrows] (global rows 0 .. N - 1, 1 <= nrows <= VSM_RUN_VIEW_MAX, distinct)
 * (or vsm_run_view_rows(run, nrows, rows_h) on a sources-only run before its first layer step: the same; vsm_run_create_ex_* with
 * the flag has no list and is refused)
 * creates a sources-only run for callers that read T-- and J0- in those rows alone: rt_run's SFI outputs after a surface step,
 * where T-- enters only as the left operand of T01_inv = T-- G1 (row i of it and of the new J0- needs row i of T-- and J0- only,
 * interaction.jl:207-266), postprocessing_vza! reads J0- at the n_stokes rows of each VZA node, and interaction_hdrf! reads J0+
 * alone.  The layer steps carry T-- as nrows row vectors (row v of T--' = T-- W is (row v of T--) W: a handful of vector x matrix
 * products instead of one matrix product) and update J0- in those rows only; the full T-- record is neither read nor written.
 * vsm_run_export writes T-- and J0- valid in the viewing rows and quiet NaN elsewhere (undefined, never stale); vsm_run_import
 * reads T-- and J0- in the viewing rows only.  R+- and J0+ are those of a sources-only run; T-- and J0- in the viewing rows
 * equal its values up to rounding.  FP64 runs only: an _f32 run accepts the call and keeps the full recurrences.
 * Stream: see Conventions; library scratch (the pre-pass images of the layer). */
typedef struct vsm_run vsm_run;
enum { VSM_RUN_SOURCES_ONLY = 1, VSM_RUN_ZW_TAIL = 2, VSM_RUN_VIEW_ROWS = 4 };
enum { VSM_RUN_VIEW_MAX = 16 };   /* viewing rows per run: four VZAs x IQUV */
int vsm_run_supported(int N, int n_stokes, int coupling);
size_t vsm_run_workspace_bytes(int N, int n_stokes, int S, int nm, const int* coupling_h);
int vsm_run_supported_f32(int N, int n_stokes, int coupling);
size_t vsm_run_workspace_bytes_f32(int N, int n_stokes, int S, int nm, const int* coupling_h);
int vsm_run_create_f64(const vsm_quad_f64* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                       size_t workspace_bytes, vsm_run** run);
int vsm_run_create_f32(const vsm_quad_f32* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                       size_t workspace_bytes, vsm_run** run);
int vsm_run_create_ex_f64(const vsm_quad_f64* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                          size_t workspace_bytes, unsigned flags, vsm_run** run);
int vsm_run_create_ex_f32(const vsm_quad_f32* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                          size_t workspace_bytes, unsigned flags, vsm_run** run);
int vsm_run_create_view_f64(const vsm_quad_f64* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                            size_t workspace_bytes, unsigned flags, int nrows, const int* rows_h, vsm_run** run);
int vsm_run_create_view_f32(const vsm_quad_f32* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                            size_t workspace_bytes, unsigned flags, int nrows, const int* rows_h, vsm_run** run);
int vsm_run_create_view_f64(const vsm_quad_f64* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                            size_t workspace_bytes, unsigned flags, int nrows, const int* rows_h, vsm_run** run);
int vsm_run_create_view_f32(const vsm_quad_f32* q, int S, int nm, const int* m_h, const int* coupling_h, void* workspace,
                            size_t workspace_bytes, unsigned flags, int nrows, const int* rows_h, vsm_run** run);
int vsm_run_layer_f64(vsm_run* run, int ndoubl, const double* dtau, const double* varpi, const double* tau_sum,
                      const double* F0, int ncomp, const double* const* Zpp, const double* const* Zmp, long long z_stride,
                      const double* fcomp, int toa, const int* layer_coupling_h, void* stream);
int vsm_run_layer_f32(vsm_run* run, int ndoubl, const float* dtau, const float* varpi, const float* tau_sum,
                      const float* F0, int ncomp, const float* const* Zpp, const float* const* Zmp, long long z_stride,
                      const float* fcomp, int toa, const int* layer_coupling_h, void* stream);
int vsm_run_export_f64(vsm_run* run, const vsm_composite_f64* comps, void* stream);
int vsm_run_export_f32(vsm_run* run, const vsm_composite_f32* comps, void* stream);
int vsm_run_import_f64(vsm_run* run, const vsm_composite_f64* comps, void* stream);
int vsm_run_import_f32(vsm_run* run, const vsm_composite_f32* comps, void* stream);
int vsm_run_zw_tail(vsm_run* run);
int vsm_run_view_rows(vsm_run* run, int nrows, const int* rows_h);
/* block `block` (0 .. blocks - 1, moment-major; VSM_ERR_INVALID_ARG past the last) of the run: its moment index, its rows and the
 * viewing rows that fall into it as local rows (local_rows[VSM_RUN_VIEW_MAX]; *nv = 0: the block carries no row of T--) */
int vsm_run_view_block(const vsm_run* run, int block, int* im, int* n, int* nv, int* local_rows);
int vsm_run_view_rows(vsm_run* run, int nrows, const int* rows_h);
/* block `block` (0 .. blocks - 1, moment-major; VSM_ERR_INVALID_ARG past the last) of the run: its moment index, its rows and the
 * viewing rows that fall into it as local rows (local_rows[VSM_RUN_VIEW_MAX]; *nv = 0: the block carries no row of T--) */
int vsm_run_view_block(const vsm_run* run, int block, int* im, int* n, int* nv, int* local_rows);
int vsm_run_destroy(vsm_run* run);
/* The surface step of a run.  A surface layer with r-+ = r+- = 0, t++ = t-- = I and j0+- = 0 leaves everything that is read below
 * it as it was under interaction!(::ScatteringInterface_11): J0-' = J0- + T-- G (...) 0, J0+' = I I (J0+ + R+- 0), R' = R + (...) 0,
 * T' = I G T with G = I -- every added term an exact zero, so the values are those of the full step (only the sign of a zero can
 * differ).  vsm_surface_layer_flags(kind, m, has_surface_source) tells from the surface type and the Fourier moment alone -- nothing
 * is read from the device -- whether a builder's layer is such a layer (VSM_SURFACE_LAYER_IDENTITY): only the scalar Lambertian
 * builder (vsm_lambertian_surface_*) at m >= 1 in a scene without a surface source (SurfaceSIF, SurfaceEmission).  The spectral
 * Lambertian builders (t = 0 at m >= 1) and the BRDF builders never are.
 *   vsm_run_export_moment  = vsm_run_export for moment `im` (0 .. nm - 1) of the run alone (comp: ONE composite).
 *   vsm_run_export_sources = of that, J0+ and J0- (with vsm_run_export's viewing-row / NaN rule) alone: no matrix is read or
 *                            written, comp's matrix pointers may be NULL.
 *   vsm_run_surface        = the surface step of moment `im`.  identity == 0: vsm_run_export_moment, then vsm_interaction(iface, N,
 *                            S, comp, added_surface, work): the kernels and arguments of the two calls.  identity != 0 (the caller
 *                            vouches for VSM_SURFACE_LAYER_IDENTITY; added_surface may be NULL): no interaction;
 *                            vsm_run_export_sources when matrices == 0 (the caller reads J0+- alone), vsm_run_export_moment else.
 * None of them synchronises with the host; all can be captured into a graph, like vsm_run_export.
 * vsm_run_guard_once(run), before the run's first layer step and any import: the caller's coupling masks come from
 * vsm_stokes_coupling on the very Z arrays it hands to vsm_run_layer, so the guard of the masks (VSM_DEVSTAT_MASK) runs on the first
 * layer step alone.  The contract is the caller's: Z arrays overwritten in place after the masks were taken are outside it, and a
 * coupling that appears that way below the first layer is dropped without a flag.  vsm_run_import ends it (every later layer step is
 * guarded again).
 * vsm_run_counters: launches of the run so far, counts_h[4] = { full exports (one per moment), source-only exports, surface
 * interactions, guard launches }. */
enum { VSM_SURFACE_LAMBERTIAN_SCALAR = 0, VSM_SURFACE_LAMBERTIAN_SPECTRAL = 1, VSM_SURFACE_BRDF = 2 };
enum { VSM_SURFACE_LAYER_IDENTITY = 1 };
unsigned vsm_surface_layer_flags(int kind, int m, int has_surface_source);
int vsm_run_export_moment_f64(vsm_run* run, int im, const vsm_composite_f64* comp, void* stream);
int vsm_run_export_moment_f32(vsm_run* run, int im, const vsm_composite_f32* comp, void* stream);
int vsm_run_export_sources_f64(vsm_run* run, int im, const vsm_composite_f64* comp, void* stream);
int vsm_run_export_sources_f32(vsm_run* run, int im, const vsm_composite_f32* comp, void* stream);
int vsm_run_surface_f64(vsm_run* run, int im, int iface, const vsm_added_f64* added_surface, int identity, int matrices,
                        const vsm_composite_f64* comp, double* work, void* stream);
int vsm_run_surface_f32(vsm_run* run, int im, int iface, const vsm_added_f32* added_surface, int identity, int matrices,
                        const vsm_composite_f32* comp, float* work, void* stream);
int vsm_run_guard_once(vsm_run* run);
int vsm_run_counters(const vsm_run* run, int* counts_h);
int vsm_stokes_coupling_f64(int N, int n_stokes, int nblocks, const double* Zpp, const double* Zmp, int* mask_d, void* stream);
int vsm_stokes_coupling_f32(int N, int n_stokes, int nblocks, const float* Zpp, const float* Zmp, int* mask_d, void* stream);

/* ---- rotational Raman scattering (RRS), operator level ---------------------
 * Inelastic layer state (src/CoreRT/types.jl:278-335 AddedLayerRS / CompositeLayerRS): 4-D arrays
 * [N,N,S,K] / [N,1,S,K], K = number of Raman offsets (length of RS_type.i_lambda1lambda0); element
 * (i,j,n1,dn) at i + N*j + N*N*n1 + N*N*S*dn.  Block (n1,dn) couples recipient point n1 with donor point
 * n0 = n1 + shift[dn] (src/Inelastic/inelastic_helper.jl:19-26); pairs with n0 outside [0,S) stay zero. */
typedef struct vsm_added_rs_f64 {
  double *ier_mp, *iet_pp, *ier_pm, *iet_mm;  /* ier-+ iet++ ier+- iet--  [N,N,S,K] */
  double *ieJ0_p, *ieJ0_m;                    /* ieJ0+ ieJ0-              [N,1,S,K] */
  int K;
  int reserved;
} vsm_added_rs_f64;
typedef struct vsm_added_rs_f32 {
  float *ier_mp, *iet_pp, *ier_pm, *iet_mm;
  float *ieJ0_p, *ieJ0_m;
  int K;
  int reserved;
} vsm_added_rs_f32;
typedef struct vsm_composite_rs_f64 {
  double *ieR_mp, *ieR_pm, *ieT_pp, *ieT_mm;
  double *ieJ0_p, *ieJ0_m;
  int K;
  int reserved;
} vsm_composite_rs_f64;
typedef struct vsm_composite_rs_f32 {
  float *ieR_mp, *ieR_pm, *ieT_pp, *ieT_mm;
  float *ieJ0_p, *ieJ0_m;
  int K;
  int reserved;
} vsm_composite_rs_f32;
/* The fields of RRS{FT} (src/Inelastic/types.jl) read by the CoreRT kernels; all DEVICE pointers. */
typedef struct vsm_rrs_f64 {
  const int* shift;        /* i_lambda1lambda0[K] */
  const double* varpi_ie;  /* varpi_lambda1lambda0[K] */
  const double* fscatt;    /* fscattRayl[S] of the current layer (rt_run.jl:221-223) */
  const double* Zpp;       /* Z++_lambda1lambda0 [N,N] of the current Fourier moment (inelastic_helper.jl:917-924) */
  const double* Zmp;       /* Z-+_lambda1lambda0 [N,N] */
} vsm_rrs_f64;
typedef struct vsm_rrs_f32 {
  const int* shift;
  const float* varpi_ie;
  const float* fscatt;
  const float* Zpp;
  const float* Zmp;
} vsm_rrs_f32;
/* elemental_inelastic!(::RRS) (CoreKernel/elemental_inelastic.jl:23-105; kernels get_elem_rt_RRS! :117-206,
 * get_elem_rt_SFI_RRS! :479-610, apply_D_elemental_RRS! :619-637).  Fills the six fields of added_rs
 * (ier+-/iet-- only when ndoubl < 1, like the reference). */
int vsm_elemental_inelastic_rrs_f64(const vsm_quad_f64* q, int S, int m, int ndoubl, const double* dtau,
                                    const double* tau_sum, const double* F0, const vsm_rrs_f64* rs,
                                    const vsm_added_rs_f64* added_rs, void* stream);
int vsm_elemental_inelastic_rrs_f32(const vsm_quad_f32* q, int S, int m, int ndoubl, const float* dtau,
                                    const float* tau_sum, const float* F0, const vsm_rrs_f32* rs,
                                    const vsm_added_rs_f32* added_rs, void* stream);
/* doubling_inelastic! = doubling_helper!(::RRS) (CoreKernel/doubling_inelastic.jl:13-164): doubles the elastic AND
 * the inelastic fields together (the elastic recurrences are interleaved with the inelastic ones), then applies
 * the D-matrix kernels (:336-356, :408-416).  expk[S] is squared in place ndoubl times.  `added` must be a full
 * per-point AddedLayer.  work: vsm_doubling_inelastic_work_elems(N,S,K) elements. */
size_t vsm_doubling_inelastic_work_elems(int N, int S, int K);
int vsm_doubling_inelastic_rrs_f64(int N, int n_stokes, int S, int ndoubl, double* expk, const int* shift,
                                   const vsm_added_f64* added, const vsm_added_rs_f64* added_rs, double* work, void* stream);
int vsm_doubling_inelastic_rrs_f32(int N, int n_stokes, int S, int ndoubl, float* expk, const int* shift,
                                   const vsm_added_f32* added, const vsm_added_rs_f32* added_rs, float* work, void* stream);
/* interaction!(RS_type::RRS, scattering_interface, ...) (CoreKernel/interaction_inelastic.jl:523-539): updates the
 * inelastic composite from pre-update elastic/inelastic values, then the elastic composite.  iface = VSM_IFACE_11:
 * interaction_helper!(::RRS, ::ScatteringInterface_11) (:319-521, fused line kernels for N <= 30); VSM_IFACE_00 / _01 / _10:
 * the statements of :74-101, :103-154, :215-262 over the in-band (recipient, line) pairs, operator level (the RRS rt_kernel!
 * hard-wires scatter = true, rt_kernel.jl:365, but dispatches the interaction on the tag, :385).  `added` may be a
 * shared-block surface layer (mat_stride 0) with an all-zero added_rs.
 * work: vsm_interaction_inelastic_work_elems(N,S,K) elements. */
size_t vsm_interaction_inelastic_work_elems(int N, int S, int K);
int vsm_interaction_inelastic_rrs_f64(int iface, int N, int S, const int* shift, const vsm_composite_f64* comp,
                                      const vsm_composite_rs_f64* comp_rs, const vsm_added_f64* added,
                                      const vsm_added_rs_f64* added_rs, double* work, void* stream);
int vsm_interaction_inelastic_rrs_f32(int iface, int N, int S, const int* shift, const vsm_composite_f32* comp,
                                      const vsm_composite_rs_f32* comp_rs, const vsm_added_f32* added,
                                      const vsm_added_rs_f32* added_rs, float* work, void* stream);
/* copy_added_to_composite_ie! (rt_helpers.jl:222-228), inelastic fields only (pair with vsm_copy_added_to_composite). */
int vsm_copy_added_to_composite_ie_f64(int N, int S, const vsm_added_rs_f64* added_rs, const vsm_composite_rs_f64* comp_rs,
                                       void* stream);
int vsm_copy_added_to_composite_ie_f32(int N, int S, const vsm_added_rs_f32* added_rs, const vsm_composite_rs_f32* comp_rs,
                                       void* stream);
/* postprocessing_vza!(::RRS) inelastic accumulation (tools/postprocessing_vza.jl:139-142):
 * ieR/ieT [nV,n_stokes,S] += w * sum_dn ieJ0-/+[rows(vza), 1, s, dn].  row0_h/w_h as in vsm_postprocess_vza. */
int vsm_postprocess_vza_ie_f64(int N, int n_stokes, int S, int K, int nV, const int* row0_h, const double* w_h,
                               const double* ieJ0_m, const double* ieJ0_p, double* ieR, double* ieT, void* stream);
int vsm_postprocess_vza_ie_f32(int N, int n_stokes, int S, int K, int nV, const int* row0_h, const float* w_h,
                               const float* ieJ0_m, const float* ieJ0_p, float* ieR, float* ieT, void* stream);

/* ---- multi-sensor runs: radiances at an interior level of the column ---------------------------------------------------
 * The level equation of rt_run_test_ms (rt_run_multisensor.jl; interlayer_flux_helper!, CoreKernel/interlayer_flux.jl:1-19,
 * applied by postprocessing_vza_ms!, tools/postprocessing_vza_ms.jl:7-52) at ONE boundary, for S spectral points:
 *   dw = (I - A B)^-1 (a + A c),   uw = (I - B A)^-1 (c + B a)
 * A = top_R_pm (R⁺⁻ of the composite above the level) [N,N,S], a = top_J0_p (its J₀⁺) [N,1,S], B = bot_R_mp (R⁻⁺ of the composite
 * below) [N,N,S] with bot_stride = N*N, or one [N,N] block shared by every point with bot_stride = 0 (a surface layer alone),
 * c = bot_J0_m (its J₀⁻) [N,1,S].  Only these four arrays are read: a sources-only run (VSM_RUN_SOURCES_ONLY) may supply the top.
 * uw = c + B dw (push-through identity), so the kernel does ONE pivoted elimination of [I - A B | a + A c] and no inverse.
 * Level conventions of the multi-sensor driver (vsmartmom.jl_amd/core_rt_ms.py): level l = the boundary below layer l counted from
 * the TOA; level 0 is the TOA composite after its surface interaction (uw = J₀⁻, dw = J₀⁺: no call here); levels 1..Nz-1 take the
 * top composite of layers 1..l and the bottom composite of layers l+1..Nz with the surface; level Nz takes the surface layer
 * ALONE as the bottom (the prototype never initialises that composite: a documented deviation).
 * Outputs: uw / dw [nV,n_stokes,S] are ACCUMULATED, R[v,k,s] += w[v,k] * level[row0[v]+k, s], with row0_h / w_h exactly as in
 * vsm_postprocess_vza (the same rows for uw and dw).  dw_full / uw_full (nullable, [N,1,S]): the level vectors at all streams.
 * N <= 128: one fused kernel, that of vsm_level_radiance_src_* with one source (MFMA product into LDS, Gauss-Jordan with the pivot
 * rule of vsm_batch_inv, mat-vec, VZA rows; work may be NULL); N > 128: the operator-level twin, which needs work = vsm_level_radiance_work_elems(N, S) elements.
 * An exactly zero pivot raises VSM_DEVSTAT_SINGULAR, a NaN / Inf in [I - A B | a + A c] VSM_DEVSTAT_NONFINITE (fused path). */
size_t vsm_level_radiance_work_elems(int N, int S);
int vsm_level_radiance_f64(int N, int n_stokes, int S, int nV, const int* row0_h, const double* w_h, const double* top_R_pm,
                           const double* top_J0_p, const double* bot_R_mp, long long bot_stride, const double* bot_J0_m,
                           double* uw, double* dw, double* dw_full, double* uw_full, double* work, void* stream);
int vsm_level_radiance_f32(int N, int n_stokes, int S, int nV, const int* row0_h, const float* w_h, const float* top_R_pm,
                           const float* top_J0_p, const float* bot_R_mp, long long bot_stride, const float* bot_J0_m,
                           float* uw, float* dw, float* dw_full, float* uw_full, float* work, void* stream);
/* Same contract, always operator level (batched products + vsm_batch_inv + products + vsm_postprocess_vza): the path for
 * N > 128 and the cross-check of the fused kernel.  work is required. */
int vsm_level_radiance_oplevel_f64(int N, int n_stokes, int S, int nV, const int* row0_h, const double* w_h,
                                   const double* top_R_pm, const double* top_J0_p, const double* bot_R_mp, long long bot_stride,
                                   const double* bot_J0_m, double* uw, double* dw, double* dw_full, double* uw_full,
                                   double* work, void* stream);
int vsm_level_radiance_oplevel_f32(int N, int n_stokes, int S, int nV, const int* row0_h, const float* w_h,
                                   const float* top_R_pm, const float* top_J0_p, const float* bot_R_mp, long long bot_stride,
                                   const float* bot_J0_m, float* uw, float* dw, float* dw_full, float* uw_full, float* work,
                                   void* stream);

/* The level equation for several SOURCES on the same operators: the per-source slots of a multi-sensor run (the solar slot and
 * the `:thermal` slot of rt_run_multisensor(thermal=True), vsmartmom.jl_amd/core_rt_ms.py).  The equation is linear in (a, c), so
 * for source pairs k = 0 .. n_src-1, a_k = top_J0_p[k], c_k = bot_J0_m[k] (HOST arrays of n_src device pointers, each [N,1,S]),
 *   dw_k = (I - A B)^-1 (a_k + A c_k),   uw_k = c_k + B dw_k
 * come from ONE pivoted elimination of [I - A B | d_0 .. d_{n_src-1}] per point (the c_k ride as spare columns of B in the MFMA
 * product that forms the system), A = top_R_pm, B = bot_R_mp / bot_stride as in vsm_level_radiance_*.  Outputs: the SUM over k:
 * its VZA rows ACCUMULATED into uw / dw [nV,n_stokes,S] (row0_h / w_h as in vsm_postprocess_vza), dw_full / uw_full (nullable,
 * [N,1,S]) the summed level vectors.  1 <= n_src <= VSM_LEVEL_MAX_SRC and N <= 128, anything else is VSM_ERR_INVALID_ARG before
 * any launch (larger N: one vsm_level_radiance_oplevel_* call per source, whose outputs accumulate).  n_src = 1 is what
 * vsm_level_radiance_* launches for N <= 128, so the two return the same bits.  Status words and pivot rule as there.
 * work is not used and may be NULL. */
#define VSM_LEVEL_MAX_SRC 4
int vsm_level_radiance_src_f64(int N, int n_stokes, int S, int nV, const int* row0_h, const double* w_h, const double* top_R_pm,
                               int n_src, const double* const* top_J0_p, const double* bot_R_mp, long long bot_stride,
                               const double* const* bot_J0_m, double* uw, double* dw, double* dw_full, double* uw_full,
                               double* work, void* stream);
int vsm_level_radiance_src_f32(int N, int n_stokes, int S, int nV, const int* row0_h, const float* w_h, const float* top_R_pm,
                               int n_src, const float* const* top_J0_p, const float* bot_R_mp, long long bot_stride,
                               const float* const* bot_J0_m, float* uw, float* dw, float* dw_full, float* uw_full, float* work,
                               void* stream);

/* Hemispheric quadratures of the level vectors at ONE boundary: the up, down and actinic fluxes of rt_run_fluxes
 * (vsmartmom.jl_amd/core_rt_flux.py).  The system of vsm_level_radiance_src_* for the source pairs k = 0 .. n_src-1 (top_J0_p /
 * bot_J0_m: HOST arrays of n_src device pointers, each [N,1,S]; A = top_R_pm, B = bot_R_mp / bot_stride as there), ONE pivoted
 * elimination per point, dw_k = (I - A B)^-1 (a_k + A c_k), uw_k = c_k + B dw_k.  The vectors never leave the chip: with the nW
 * weight rows q [nW][N / n_stokes] (a DEVICE array, one weight per stream, applied to the rows of Stokes I),
 *   out[0][r][s] = sum_i q[r][i] sum_k uw_k[i n_stokes, s]      out[1][r][s] = sum_i q[r][i] sum_k dw_k[i n_stokes, s]
 *   out[2][r][s] = dir_h[r] F0_I[s] exp(-tau_sum[s] / mu0)      (tau_sum, F0_I: [S], given together or both NULL: then 0)
 * out [3][nW][S] is WRITTEN, not accumulated; dir_h is a HOST array of nW factors (read only with tau_sum / F0_I).  The additions
 * of a quadrature have a fixed order (one wave per (r, direction), lanes over i, a butterfly), so a point's result depends on
 * neither its place in the batch nor the run.  top_R_pm == NULL: no layer lies above the boundary (the TOA): no system is formed,
 * dw = 0 and uw = sum_k c_k (top_J0_p, bot_R_mp are not read).  1 <= n_src <= VSM_LEVEL_MAX_SRC, 1 <= nW <= 4, N <= 128, S >= 0,
 * the required pointers non-NULL; anything else is VSM_ERR_INVALID_ARG before any launch (larger N: one
 * vsm_level_radiance_oplevel_* call per source with full vectors, then a batched product with q).  S = 0 launches nothing.
 * Status words and pivot rule as in vsm_level_radiance_*. */
int vsm_level_flux_f64(int N, int n_stokes, int S, const double* top_R_pm, int n_src, const double* const* top_J0_p,
                       const double* bot_R_mp, long long bot_stride, const double* const* bot_J0_m, int nW, const double* q,
                       const double* dir_h, double mu0, const double* tau_sum, const double* F0_I, double* out, void* stream);
int vsm_level_flux_f32(int N, int n_stokes, int S, const float* top_R_pm, int n_src, const float* const* top_J0_p,
                       const float* bot_R_mp, long long bot_stride, const float* const* bot_J0_m, int nW, const float* q,
                       const float* dir_h, float mu0, const float* tau_sum, const float* F0_I, float* out, void* stream);

/* The response of the column to a UNIT surface emission (the SIF Jacobian slots of the linearized run, vsmartmom.jl_amd/
 * core_rt_lin.py).  vsm_surface_sif_* adds the same value to j0- of the surface layer at every stream, so the radiance is
 * sum_c 2 sif[c, s] G_c(s), G_c = the response to the pattern e_c (1 on the rows of Stokes component c, 0 elsewhere).  For the K
 * components comp_h[0..K-1] (HOST array, each in 0..n_stokes-1), with A = top_R_pm (R+- of the atmosphere's composite BEFORE the
 * surface interaction), B = bot_R_mp (the surface r-+, bot_stride 0 or N*N) and T = top_T_mm (T-- of the same composite):
 *   dw_k = (I - A B)^-1 A e_k,   y_k = e_k + B dw_k      (ONE pivoted elimination of [I - A B | A e_0 .. A e_{K-1}] per point)
 *   up[k][s][c][v] = w[v,c] sum_j T[row0[v] + c, j] y_k[j]      dn[k][s][c][v] = w[v,c] dw_k[row0[v] + c]
 * WRITTEN (not accumulated), per component and not summed; row0_h / w_h as in vsm_postprocess_vza at m = 0.  up is the share of
 * interaction!'s J0- (TOA), dn that of its J0+ (BOA; the surface layer's t++ = I).  1 <= K <= 4 and N <= 128, anything else is
 * VSM_ERR_INVALID_ARG before any launch (larger N: one vsm_level_radiance_oplevel_* call per component with top_J0_p = 0,
 * bot_J0_m = e_k and uw_full = y_k, then the row products).  Status words and pivot rule as in vsm_level_radiance_*. */
int vsm_surface_emission_response_f64(int N, int n_stokes, int S, int K, const int* comp_h, int nV, const int* row0_h,
                                      const double* w_h, const double* top_R_pm, const double* top_T_mm, const double* bot_R_mp,
                                      long long bot_stride, double* up, double* dn, void* stream);
int vsm_surface_emission_response_f32(int N, int n_stokes, int S, int K, const int* comp_h, int nV, const int* row0_h,
                                      const float* w_h, const float* top_R_pm, const float* top_T_mm, const float* bot_R_mp,
                                      long long bot_stride, float* up, float* dn, void* stream);

/* The inelastic (rotational-Raman) level equation of rt_run_test_ms(::RRS) (interlayer_flux_helper!(::RRS), CoreKernel/
 * interlayer_flux.jl:21-77, applied by postprocessing_vza_ms!(::RRS), tools/postprocessing_vza_ms.jl:55-118) at ONE boundary, the
 * lines summed: for recipient point n1 and line k with donor n0 = n1 + shift[k] (in-band pairs only, 0 <= n0 < S),
 *   q = sum_k [c_ie,k + B_ie,k dw(n0)],   r = sum_k [a_ie,k + A_ie,k uw(n0)] + A(n1) q,
 *   dw_ie = (I - A(n1) B(n1))^-1 r,       uw_ie = q + B(n1) dw_ie
 * which is the line sum of the reference's per-line two-inverse formula (push-through identity).  A = top_R_pm [N,N,S], B = bot_R_mp
 * with bot_stride (N*N, or 0: one block shared by every point), dw / uw = dw_full / uw_full [N,1,S] of the ELASTIC level call
 * (vsm_level_radiance_*) at the same level; A_ie = top_ieR_pm [N,N,S,K], a_ie = top_ieJ0_p [N,1,S,K] (the RS layout above);
 * B_ie = bot_ieR_mp, c_ie = bot_ieJ0_m in the same layout, both NULL for a bottom without an inelastic part (the surface layer
 * alone: q = 0).  shift [K] (device).  Outputs as in vsm_level_radiance_*: uwie / dwie [nV,n_stokes,S] ACCUMULATED with row0_h /
 * w_h, dwie_full / uwie_full (nullable) [N,1,S] the summed inelastic level vectors at all streams.  N <= 128: one workgroup per
 * recipient point streams its 2K inelastic blocks, then solves [I - A B | r] by the elastic kernel's elimination (same pivot rule,
 * VSM_DEVSTAT_SINGULAR / _NONFINITE).  No work buffer. */
int vsm_level_radiance_ie_f64(int N, int n_stokes, int S, int K, const int* shift, int nV, const int* row0_h, const double* w_h,
                              const double* top_R_pm, const double* bot_R_mp, long long bot_stride, const double* dw_full,
                              const double* uw_full, const double* top_ieR_pm, const double* top_ieJ0_p, const double* bot_ieR_mp,
                              const double* bot_ieJ0_m, double* uwie, double* dwie, double* dwie_full, double* uwie_full,
                              void* stream);
int vsm_level_radiance_ie_f32(int N, int n_stokes, int S, int K, const int* shift, int nV, const int* row0_h, const float* w_h,
                              const float* top_R_pm, const float* bot_R_mp, long long bot_stride, const float* dw_full,
                              const float* uw_full, const float* top_ieR_pm, const float* top_ieJ0_p, const float* bot_ieR_mp,
                              const float* bot_ieJ0_m, float* uwie, float* dwie, float* dwie_full, float* uwie_full, void* stream);

/* Hemispheric quadratures of the elastic AND the inelastic level vectors at ONE boundary: the fluxes of
 * CoreRTRaman.rt_run_fluxes (vsmartmom.jl_amd/core_rt_flux_raman.py).  The system of vsm_level_radiance_ie_* per recipient point
 * n1, operands, layouts, in-band rule, elimination and pivots as there (the two return the same dw_ie / uw_ie bits), but the
 * vectors never leave the chip and no [N,1,S] inelastic vector exists anywhere: with the nW weight rows q [nW][N / n_stokes]
 * (a DEVICE array, one weight per stream, applied to the rows of Stokes I) as in vsm_level_flux_*,
 *   out[0][r][n1] = sum_i q[r][i] uw[i n_stokes, n1]          out[1][r][n1] = sum_i q[r][i] dw[i n_stokes, n1]
 *   out[3][r][n1] = sum_i q[r][i] uw_ie[i n_stokes]           out[4][r][n1] = sum_i q[r][i] dw_ie[i n_stokes]
 *   out[2][r][n1] = dir_h[r] F0_I[n1] exp(-tau_sum[n1] / mu0)   (tau_sum, F0_I: [S], given together or both NULL: then 0)
 * uw / dw = uw_full / dw_full [N,1,S] of the ELASTIC level call at the same level, read at the donors for the solve and at n1
 * itself for rows 0 and 1.  out [5][nW][S] is WRITTEN, not accumulated; dir_h is a HOST array of nW factors (read only with
 * tau_sum / F0_I).  The additions of a quadrature have the fixed order of vsm_level_flux_*.  top_R_pm == NULL: no layer lies
 * above the boundary (the TOA): no system is formed, dw = dw_ie = 0, uw = uw_full (J0- of the whole column) and uw_ie = the sum
 * of bot_ieJ0_m over the in-band lines, in the order of k; dw_full, bot_R_mp, top_ieR_pm, top_ieJ0_p and bot_ieR_mp are not read.
 * bot_ieR_mp = bot_ieJ0_m = NULL, both or neither, at the TOA too: a bottom without an inelastic part.  K = 0 is legal: rows 3 and 4 are 0.  1 <= nW <= 4,
 * 1 <= N <= 128, n_stokes divides N, S >= 0, the required pointers non-NULL; anything else is VSM_ERR_INVALID_ARG before any
 * launch.  S = 0 launches nothing.  Status words and pivot rule as in vsm_level_radiance_*.  No work buffer. */
int vsm_level_flux_ie_f64(int N, int n_stokes, int S, int K, const int* shift, const double* top_R_pm, const double* bot_R_mp,
                          long long bot_stride, const double* dw_full, const double* uw_full, const double* top_ieR_pm,
                          const double* top_ieJ0_p, const double* bot_ieR_mp, const double* bot_ieJ0_m, int nW, const double* q,
                          const double* dir_h, double mu0, const double* tau_sum, const double* F0_I, double* out, void* stream);
int vsm_level_flux_ie_f32(int N, int n_stokes, int S, int K, const int* shift, const float* top_R_pm, const float* bot_R_mp,
                          long long bot_stride, const float* dw_full, const float* uw_full, const float* top_ieR_pm,
                          const float* top_ieJ0_p, const float* bot_ieR_mp, const float* bot_ieJ0_m, int nW, const float* q,
                          const float* dir_h, float mu0, const float* tau_sum, const float* F0_I, float* out, void* stream);

/* The derivative of the level equation (vsm_level_radiance_*) with respect to the Jacobian parameters of a linearized multi-sensor
 * run (vsmartmom.jl_amd/core_rt_ms_lin.py) at ONE boundary: for every parameter p, with dw / uw = dw_full / uw_full [N,1,S] of the
 * elastic level call at the same level and M = I - A B,
 *   q_p = c'_p + B'_p dw,   dw'_p = M^-1 (a'_p + A'_p uw + A q_p),   uw'_p = q_p + B dw'_p
 * (the derivative of interlayer_flux_helper!, CoreKernel/interlayer_flux.jl:1-19, in the push-through form).  A = top_R_pm [N,N,S],
 * B = bot_R_mp with bot_stride (N*N, or 0: one block shared by every point).  Derivative stacks, the parameter axis slowest:
 * A' = top_R_pm_lin with top_lin_pstride elements per parameter and N*N per point, a' = top_J0_p_lin [N,1,S,P_top]; slots
 * >= P_top of the top are zero and not read (P_top = 0: both may be NULL).  B' = bot_R_mp_lin with bot_lin_stride per point (N*N,
 * or 0: one block per parameter shared by every point) and bot_lin_pstride per parameter, c' = bot_J0_m_lin [N,1,S,P].
 * Outputs: uw_lin / dw_lin [nV,n_stokes,S,P] ACCUMULATED with row0_h / w_h as in vsm_postprocess_vza_lin; dw_lin_full /
 * uw_lin_full (nullable) [N,1,S,P] the derivative vectors at all streams.  N <= 128, 1 <= P <= 64: one workgroup per point, the
 * parameters in chunks as extra right-hand sides of ONE Gauss-Jordan elimination of [M | r_1 .. r_PC] per chunk (the pivot rule
 * of vsm_level_radiance_*, VSM_DEVSTAT_SINGULAR / _NONFINITE).  No work buffer. */
int vsm_level_radiance_lin_f64(int N, int n_stokes, int S, int P, int P_top, int nV, const int* row0_h, const double* w_h,
                               const double* top_R_pm, const double* bot_R_mp, long long bot_stride, const double* dw_full,
                               const double* uw_full, const double* top_R_pm_lin, long long top_lin_pstride,
                               const double* top_J0_p_lin, const double* bot_R_mp_lin, long long bot_lin_stride,
                               long long bot_lin_pstride, const double* bot_J0_m_lin, double* uw_lin, double* dw_lin,
                               double* dw_lin_full, double* uw_lin_full, void* stream);
int vsm_level_radiance_lin_f32(int N, int n_stokes, int S, int P, int P_top, int nV, const int* row0_h, const float* w_h,
                               const float* top_R_pm, const float* bot_R_mp, long long bot_stride, const float* dw_full,
                               const float* uw_full, const float* top_R_pm_lin, long long top_lin_pstride,
                               const float* top_J0_p_lin, const float* bot_R_mp_lin, long long bot_lin_stride,
                               long long bot_lin_pstride, const float* bot_J0_m_lin, float* uw_lin, float* dw_lin,
                               float* dw_lin_full, float* uw_lin_full, void* stream);

/* vsm_level_radiance_lin_* with P_src >= 0 further SOURCE-ONLY slots behind the P parameter slots: the Planck (temperature) slots
 * of a linearized multi-sensor run with thermal emission (vsmartmom.jl_amd/core_rt_ms_lin.py).  The level equation
 * is linear in (a, c), so for a parameter x_k that enters through the sources alone, with a_k = d top_J0_p / dx_k = src_top_J0_p
 * [N,1,S,P_src] and c_k = d bot_J0_m / dx_k = src_bot_J0_m [N,1,S,P_src] (the parameter axis slowest),
 *   dw'_(P+k) = M^-1 (a_k + A c_k),   uw'_(P+k) = c_k + B dw'_(P+k)
 * on the same M = I - A B; no operator derivative is read for such a slot.  Slots p < P exactly as in vsm_level_radiance_lin_*.
 * Outputs: uw_lin / dw_lin [nV,n_stokes,S,P+P_src] ACCUMULATED, dw_lin_full / uw_lin_full (nullable) [N,1,S,P+P_src].  All
 * P + P_src slots run in the chunks of vsm_level_radiance_lin_* as right-hand sides of ONE elimination per chunk; a chunk may hold
 * both kinds.  N <= 128, 1 <= P, P + P_src <= 64, anything else is VSM_ERR_INVALID_ARG before any launch (P_src = 0: both source
 * stacks may be NULL: this is the call vsm_level_radiance_lin_* makes, so the two return the same bits).  Status words and pivot
 * rule as there.  No work buffer. */
int vsm_level_radiance_lin_src_f64(int N, int n_stokes, int S, int P, int P_top, int P_src, int nV, const int* row0_h,
                                   const double* w_h, const double* top_R_pm, const double* bot_R_mp, long long bot_stride,
                                   const double* dw_full, const double* uw_full, const double* top_R_pm_lin,
                                   long long top_lin_pstride, const double* top_J0_p_lin, const double* bot_R_mp_lin,
                                   long long bot_lin_stride, long long bot_lin_pstride, const double* bot_J0_m_lin,
                                   const double* src_top_J0_p, const double* src_bot_J0_m, double* uw_lin, double* dw_lin,
                                   double* dw_lin_full, double* uw_lin_full, void* stream);
int vsm_level_radiance_lin_src_f32(int N, int n_stokes, int S, int P, int P_top, int P_src, int nV, const int* row0_h,
                                   const float* w_h, const float* top_R_pm, const float* bot_R_mp, long long bot_stride,
                                   const float* dw_full, const float* uw_full, const float* top_R_pm_lin,
                                   long long top_lin_pstride, const float* top_J0_p_lin, const float* bot_R_mp_lin,
                                   long long bot_lin_stride, long long bot_lin_pstride, const float* bot_J0_m_lin,
                                   const float* src_top_J0_p, const float* src_bot_J0_m, float* uw_lin, float* dw_lin,
                                   float* dw_lin_full, float* uw_lin_full, void* stream);

/* Hemispheric quadratures of the DERIVATIVE level vectors at ONE boundary: the flux Jacobians of CoreRTLin.rt_run_fluxes
 * (vsmartmom.jl_amd/core_rt_flux_lin.py).  The operators, vectors and slots of vsm_level_radiance_lin_src_* (P parameter slots, of
 * which the first P_top have a top derivative, then P_src source-only slots; the same chunks as right-hand sides of ONE pivoted
 * elimination each, the same LDS bound) without its viewing-angle arguments, and the weight rows and direct-beam arguments of
 * vsm_level_flux_*: q [nW][N / n_stokes] (DEVICE), dir_h [nW] (HOST), mu0, tau_sum / F0_I [S] (given together or both NULL), and
 * tau_sum_dot [p_layer][S] (DEVICE; the parameter axis slowest), the derivative of tau_sum with respect to the first p_layer
 * slots (0 <= p_layer <= P).  The derivative vectors never leave the chip.  out [3][nW][1 + P + P_src][S] is WRITTEN, not
 * accumulated; for weight row r and point s
 *   out[0][r][0]     = sum_i q[r][i] uw[i n_stokes]        out[1][r][0]     = sum_i q[r][i] dw[i n_stokes]   (uw_full / dw_full)
 *   out[0][r][1 + p] = sum_i q[r][i] uw'_p[i n_stokes]     out[1][r][1 + p] = sum_i q[r][i] dw'_p[i n_stokes]
 *   out[2][r][0]     = dir_h[r] F0_I exp(-tau_sum / mu0)   out[2][r][1 + p] = -out[2][r][0] tau_sum_dot[p] / mu0   (p < p_layer)
 * and out[2][r][1 + p] = 0 for every other slot; tau_sum == NULL: all of out[2] is 0.  The additions of a quadrature have the
 * fixed order of vsm_level_flux_* (one wave per (slot, r, direction), lanes over i, a butterfly): a point's bits depend on
 * neither its place in the batch nor the batch size.  top_R_pm == NULL: no layer lies above the boundary (the TOA), no system is
 * formed: dw = 0 and every dw' = 0, uw = uw_full (the column's J0-), uw'_p = bot_J0_m_lin[p], or src_bot_J0_m[k] for a
 * source-only slot; bot_R_mp, dw_full, the operator derivatives and src_top_J0_p are not read.  N <= 128, P >= 0, P_src >= 0,
 * 1 <= P + P_src <= 64, 1 <= nW <= 4, strides as in vsm_level_radiance_lin_*, the required pointers non-NULL; anything else is
 * VSM_ERR_INVALID_ARG before any launch.  S = 0 launches nothing.  Status words and pivot rule as in vsm_level_radiance_*. */
int vsm_level_flux_lin_f64(int N, int n_stokes, int S, int P, int P_top, int P_src, const double* top_R_pm, const double* bot_R_mp,
                           long long bot_stride, const double* dw_full, const double* uw_full, const double* top_R_pm_lin,
                           long long top_lin_pstride, const double* top_J0_p_lin, const double* bot_R_mp_lin,
                           long long bot_lin_stride, long long bot_lin_pstride, const double* bot_J0_m_lin,
                           const double* src_top_J0_p, const double* src_bot_J0_m, int nW, const double* q, const double* dir_h,
                           double mu0, const double* tau_sum, const double* F0_I, const double* tau_sum_dot, int p_layer,
                           double* out, void* stream);
int vsm_level_flux_lin_f32(int N, int n_stokes, int S, int P, int P_top, int P_src, const float* top_R_pm, const float* bot_R_mp,
                           long long bot_stride, const float* dw_full, const float* uw_full, const float* top_R_pm_lin,
                           long long top_lin_pstride, const float* top_J0_p_lin, const float* bot_R_mp_lin,
                           long long bot_lin_stride, long long bot_lin_pstride, const float* bot_J0_m_lin,
                           const float* src_top_J0_p, const float* src_bot_J0_m, int nW, const float* q, const float* dir_h,
                           float mu0, const float* tau_sum, const float* F0_I, const float* tau_sum_dot, int p_layer, float* out,
                           void* stream);

/* ---- single-scattering runs: rt_run_ss (src/CoreRT/rt_run.jl:574-755) -----------------------------------------------------
 * One Fourier moment of the single-scattering column walk, all layers and the surface in ONE launch: per layer the exact
 * finite-tau sources of elemental! with ndoubl = 0 and dtau = the layer's tau (get_elem_rt_SFI!, CoreKernel/elemental.jl:348-392;
 * rt_kernel_ss!, CoreKernel/rt_kernel_ss.jl:156-238 hard-wires scatter = true and ndoubl_ss = 0, so no D sign goes on j0-), the
 * TOA copy for the first layer and for every later one the two statements of get_interaction_ss! (CoreKernel/interaction_ss.jl:
 * 14-19):   J0+[i,n] = J0+[i,n] exp(-tau_iz[n] / mu_i) + j0+[i,n],   J0-[i,n] += j0-[i,n] exp(-tau_sum_iz[n] / mu_i),
 * then once more with the surface layer's sources (rt_run.jl:715-722: layer tau = 0, tau_sum = tau_sum_surface) and the viewing
 * rows of postprocessing_vza! (tools/postprocessing_vza.jl:23-94, SFI branch).  No N x N array is formed or read: of Z only the
 * n_stokes SZA columns.
 * Layer tables: HOST arrays of L device pointers, tau_h / varpi_h / tau_sum_h [S] each, Zpp_h / Zmp_h with z_stride_h[iz] elements
 * per spectral point (0 = one [N,N] block shared by every point, N*N = per point [N,N,S]); they reach the device through the
 * library's scratch, L >= 1 is not capped.  F0 [n_stokes,S] with the F0 / Z indexing of vsm_elemental_* (the j0+- of a layer are
 * those of vsm_elemental_*(ndoubl = 0, dtau = tau)).  surf_j0_m [N,1,S] = j0- of the surface AddedLayer; surf_j0_p (nullable =
 * zero) its j0+ (the scalar Lambertian builder puts the direct beam there for m = 0, lambertian_surface.jl:75, and interaction_ss!
 * adds it); tau_sum_surface [S].  row0_h / w_h [nV] / [nV * n_stokes] exactly as in vsm_postprocess_vza (any nV >= 1).
 * Outputs: R_SFI / T_SFI [nV,n_stokes,S] are ACCUMULATED (R[v,k,s] += w[v,k] J0-[row0[v]+k, s]); J0_m / J0_p (nullable, [N,1,S])
 * receive the composite sources at all streams (the driver's hem_R / hem_T read them for m = 0, rt_run.jl:737-748). */
int vsm_ss_column_f64(const vsm_quad_f64* q, int S, int L, int m, const double* const* tau_h, const double* const* varpi_h,
                      const double* const* tau_sum_h, const double* const* Zpp_h, const double* const* Zmp_h,
                      const long long* z_stride_h, const double* F0, const double* surf_j0_m, const double* surf_j0_p,
                      const double* tau_sum_surface, int nV, const int* row0_h, const double* w_h, double* R_SFI, double* T_SFI,
                      double* J0_m, double* J0_p, void* stream);
int vsm_ss_column_f32(const vsm_quad_f32* q, int S, int L, int m, const float* const* tau_h, const float* const* varpi_h,
                      const float* const* tau_sum_h, const float* const* Zpp_h, const float* const* Zmp_h,
                      const long long* z_stride_h, const float* F0, const float* surf_j0_m, const float* surf_j0_p,
                      const float* tau_sum_surface, int nV, const int* row0_h, const float* w_h, float* R_SFI, float* T_SFI,
                      float* J0_m, float* J0_p, void* stream);
/* The linearized twin of vsm_ss_column_*: d R_SFI / d x_p and d T_SFI / d x_p of one Fourier moment for the parameter slots
 * [p_lo, p_hi) of P (slot order of parameter_layout.jl:28-56; the first p_layer slots are layer parameters, the others belong to
 * the surface).  The reference has no linearized single-scattering driver; the statements are those of its linearized full run
 * taken at ndoubl = 0: per layer the source derivatives of get_elem_rt_SFI_fused! (CoreKernel/elemental_lin.jl:602-712: chain
 * rule through tau, varpi, Z and the beam term -tau_sum' / mu_0) with dtau = the layer's tau, and the derivative of the two
 * statements of get_interaction_ss! (CoreKernel/interaction_ss.jl:14-19), taken on J0+ before its update:
 *   J0+'[i,n] = (J0+'[i,n] - J0+[i,n] tau'[n] / mu_i) exp(-tau[n] / mu_i) + j0+'[i,n],
 *   J0-'[i,n] += (j0-'[i,n] - j0-[i,n] tau_sum'[n] / mu_i) exp(-tau_sum[n] / mu_i),
 * the TOA layer copied (rt_kernel_ss.jl:213-216), the branch of a viewing row equal to the SZA row as elemental_lin.jl writes it;
 * then the same update with the surface layer (tau = 0, tau_sum = tau_sum_surface) and the rows of postprocessing_vza! (lin)
 * (tools/postprocessing_vza_lin.jl:18-48).  Surface slots are exact zeros in the atmospheric layers.
 * Layer tables (HOST arrays of L device pointers, as in vsm_ss_column_*): the forward tau_h / varpi_h / tau_sum_h / Zpp_h / Zmp_h /
 * z_stride_h, and tau_dot_h / varpi_dot_h / tau_sum_dot_h [S,p_layer] per layer -- the layer slices of vsm_layer_optics_lin_*'s
 * outputs computed with an all-zero ndoubl table, so that tau_dot is the derivative of the layer's FULL tau.  zdcoef_h (nullable
 * table, nullable entries = Z_dot is zero): per layer [CT,p_layer,S] coefficients of Z_dot over the CT component blocks
 * Zc_pp / Zc_mp [N,N,CT] of the moment (vsm_elemental_lin_mix_*), read for the first p_zdot <= p_layer slots only (7 per aerosol:
 * the coefficients of the gas slots behind them are exact zeros and are skipped): of every block only the n_stokes SZA columns at the viewing
 * rows are read, and neither Z_dot nor a per-slot source array is ever formed.
 * Surface: surf_j0_m [N,1,S] and surf_j0_m_lin / surf_j0_p_lin [N,1,S,P] are j0- and ap_J0-+ as vsm_lambertian_surface_lin_* /
 * vsm_brdf_surface_lin_* write them (all P slots); surf_j0_p (nullable = zero) is the FORWARD builder's j0+ -- the direct beam,
 * proportional to exp(-tau_sum / mu_0) (lambertian_surface.jl:75) -- and contributes -j0+ tau_sum' / mu_0 to the layer slots;
 * tau_sum_dot_surface [S,p_layer].  Rdot / Tdot [nV,n_stokes,S,P] are ACCUMULATED for the slots of the range only, each slot
 * computed independently of the range it is called in.  Invalid arguments (P < 1, L < 1, null tables, rows outside N, a slot
 * range outside P) return VSM_ERR_INVALID_ARG before any launch. */
int vsm_ss_column_lin_f64(const vsm_quad_f64* q, int S, int L, int m, int P, int p_layer, int p_zdot, int p_lo, int p_hi,
                          const double* const* tau_h, const double* const* varpi_h, const double* const* tau_sum_h,
                          const double* const* Zpp_h, const double* const* Zmp_h, const long long* z_stride_h,
                          const double* const* tau_dot_h, const double* const* varpi_dot_h, const double* const* tau_sum_dot_h,
                          const double* const* zdcoef_h, int CT, const double* Zc_pp, const double* Zc_mp, const double* F0,
                          const double* surf_j0_m, const double* surf_j0_p, const double* surf_j0_m_lin, const double* surf_j0_p_lin,
                          const double* tau_sum_surface, const double* tau_sum_dot_surface, int nV, const int* row0_h,
                          const double* w_h, double* Rdot, double* Tdot, void* stream);
int vsm_ss_column_lin_f32(const vsm_quad_f32* q, int S, int L, int m, int P, int p_layer, int p_zdot, int p_lo, int p_hi,
                          const float* const* tau_h, const float* const* varpi_h, const float* const* tau_sum_h,
                          const float* const* Zpp_h, const float* const* Zmp_h, const long long* z_stride_h,
                          const float* const* tau_dot_h, const float* const* varpi_dot_h, const float* const* tau_sum_dot_h,
                          const float* const* zdcoef_h, int CT, const float* Zc_pp, const float* Zc_mp, const float* F0,
                          const float* surf_j0_m, const float* surf_j0_p, const float* surf_j0_m_lin, const float* surf_j0_p_lin,
                          const float* tau_sum_surface, const float* tau_sum_dot_surface, int nV, const int* row0_h,
                          const float* w_h, float* Rdot, float* Tdot, void* stream);
/* The rotational-Raman twin (rt_kernel_ss!(::RRS), rt_kernel_ss.jl:240-337): per layer the sources of get_elem_rt_SFI_RRS!
 * (CoreKernel/elemental_inelastic.jl:479-603; near / far branches on rt_close_tol and on the viewing row being the SZA row as
 * written there) with ndoubl = 0 and dtau = tau, composed by get_interaction_ss_RRS! (interaction_ss.jl:79-90) and summed over the
 * lines by postprocessing_vza!(::RRS) (postprocessing_vza.jl:139-142); the surface adds nothing.  Donor n0 = n1 + shift[dn];
 * pairs with n0 outside [0, S) contribute exactly zero.  The line sum is taken inside the kernel and only the viewing rows are
 * evaluated: no [N,S,K] array exists.  tau_h / tau_sum_h / fscatt_h: HOST arrays of L device pointers ([S] each; fscatt = the
 * layer's fScattRayleigh); shift [K] (int) and varpi_ie [K] on the device, Zpp_ie / Zmp_ie the flat [N,N] Raman phase matrices of
 * the moment.  K = 0 is legal (nothing is launched).  ieR_SFI / ieT_SFI [nV,n_stokes,S] are ACCUMULATED.
 * A workgroup owns VSM_SS_BLOCK consecutive recipient points and stages the per-layer donor factors of the points within `halo`
 * of its block in LDS (0 <= halo, clamped to VSM_SS_MAX_HALO; the host passes the largest |shift| it wants staged); a line whose
 * donor lies outside that window reads global memory instead -- the same values, so `halo` never changes a result. */
#define VSM_SS_BLOCK 128
#define VSM_SS_MAX_HALO 192
int vsm_ss_column_rrs_f64(const vsm_quad_f64* q, int S, int L, int m, int K, const double* const* tau_h,
                          const double* const* tau_sum_h, const double* const* fscatt_h, const int* shift,
                          const double* varpi_ie, const double* Zpp_ie, const double* Zmp_ie, const double* F0, int halo,
                          int nV, const int* row0_h, const double* w_h, double* ieR_SFI, double* ieT_SFI, void* stream);
int vsm_ss_column_rrs_f32(const vsm_quad_f32* q, int S, int L, int m, int K, const float* const* tau_h,
                          const float* const* tau_sum_h, const float* const* fscatt_h, const int* shift, const float* varpi_ie,
                          const float* Zpp_ie, const float* Zmp_ie, const float* F0, int halo, int nV, const int* row0_h,
                          const float* w_h, float* ieR_SFI, float* ieT_SFI, void* stream);
/* The linearized twin of vsm_ss_column_rrs_* (the reference has no linearized Raman driver): d ieR_SFI / d x_p and
 * d ieT_SFI / d x_p of one Fourier moment for the parameter slots [p_lo, min(p_hi, p_layer)) of P.  A (recipient n1, line, donor
 * n0) source depends on the run's parameters through d0 = tau[n0], d1 = tau[n1] and g0 = fscatt[n0] exp(-tau_sum[n0] / mu_0) only,
 * and the interaction through exp(-tau[n1] / mu_i) and exp(-tau_sum[n1] / mu_i); varpi_ie, Z_ie, F0, the layers' varpi and the
 * surface do not enter.  Statement by statement: the forward factors again, the chain rule through (d0, d1, g0) with
 * g0' = fscatt'[n0] exp(-tau_sum[n0] / mu_0) - g0 tau_sum'[n0] / mu_0, and on the running line sums BEFORE their update
 *   S+' = (S+' - S+ tau'[n1] / mu_i) exp(-tau[n1] / mu_i) + s+',   S-' += (s-' - s- tau_sum'[n1] / mu_i) exp(-tau_sum[n1] / mu_i),
 * the TOA layer copied.  In the two close branches of the forward kernel (|d0 - d1| <= 1e-8 on the SZA rows,
 * |mu_i / mu_0 - d1 / d0| < 1e-8 elsewhere) the partials are the analytic limits of the regular expression's,
 *   d/d d0 = exp(-d0 / mu_0) / mu_i (1 - d0 / (2 mu_0)),   d/d d1 = -d0 exp(-d0 / mu_0) / (2 mu_i^2),
 * not derivatives of the close value taken as a function of d0 alone.
 * Forward tables and `halo` as in vsm_ss_column_rrs_*; tau_dot_h / tau_sum_dot_h / fscatt_dot_h: HOST arrays of L device pointers,
 * [S,p_layer] each (tau_dot of the layer's FULL tau, the layout of vsm_ss_column_lin_*; a table may have more than p_layer
 * slots, only the first p_layer are read), each read at n0 and at n1.  ieRdot / ieTdot [nV,n_stokes,S,P] are ACCUMULATED for the
 * slots of the range below p_layer, each slot computed independently of the range it is called in; slots >= p_layer (the
 * surface's) are exact zeros and are not touched.  K = 0, S = 0 and p_lo >= p_layer launch nothing.  Invalid arguments (K < 0,
 * P < 1, p_layer outside [0, P], a slot range outside P or empty, L < 1, null tables, rows outside N) return
 * VSM_ERR_INVALID_ARG before any launch. */
int vsm_ss_column_rrs_lin_f64(const vsm_quad_f64* q, int S, int L, int m, int K, int P, int p_layer, int p_lo, int p_hi,
                              const double* const* tau_h, const double* const* tau_sum_h, const double* const* fscatt_h,
                              const double* const* tau_dot_h, const double* const* tau_sum_dot_h,
                              const double* const* fscatt_dot_h, const int* shift, const double* varpi_ie, const double* Zpp_ie,
                              const double* Zmp_ie, const double* F0, int halo, int nV, const int* row0_h, const double* w_h,
                              double* ieRdot, double* ieTdot, void* stream);
int vsm_ss_column_rrs_lin_f32(const vsm_quad_f32* q, int S, int L, int m, int K, int P, int p_layer, int p_lo, int p_hi,
                              const float* const* tau_h, const float* const* tau_sum_h, const float* const* fscatt_h,
                              const float* const* tau_dot_h, const float* const* tau_sum_dot_h,
                              const float* const* fscatt_dot_h, const int* shift, const float* varpi_ie, const float* Zpp_ie,
                              const float* Zmp_ie, const float* F0, int halo, int nV, const int* row0_h, const float* w_h,
                              float* ieRdot, float* ieTdot, void* stream);

/* ---- exact single scattering: StandaloneSS (src/StandaloneSS/kernels.jl, linearized_f2.jl) ---------------------------------
 * The first-order field at the true scattering angle of every viewing geometry, in four paths: (1) one scattering in the
 * atmosphere, (2) the direct beam reflected by the surface, (3) atmosphere -> surface -> sensor, (4) surface -> atmosphere ->
 * sensor; (3) and (4) for scalar radiance over a Lambertian surface, as the reference restricts them.
 * Contributors: tau_c_h is a HOST array of C * L device pointers, entry c * L + iz the [S] optical depths of contributor c in
 * layer iz; varpi_c_h [C] (host) their single-scattering albedos; the phase functions are spectrally flat and arrive as small HOST
 * tables per contributor.  The kernels mix them per (layer, point):
 *   tau = sum_c tau_c,   varpi_eff P_eff = (sum_c tau_c varpi_c p_c) / tau   (zero where tau = 0),
 * so neither P_eff[nV,n_stokes,L,S] nor the azimuthal averages Pbar[nV,L,S,nQ] of the reference exist.  The tables reach the
 * device through the library's scratch; L, C and nV <= 65535 are not capped otherwise.  I0 [S], albedo [S] and brdf are device
 * arrays, mu_v_h [nV] host.  Outputs [nV,n_stokes,S] are WRITTEN.  Invalid arguments (L < 1, C < 1, nV < 1, n_stokes outside 1..4,
 * nQ < 1, null tables or entries, a cosine <= 0) return VSM_ERR_INVALID_ARG before any launch; S = 0 launches nothing.
 *   path1: p_c_h [C][nV][n_stokes] = the first column of contributor c's phase matrix at geometry v, rotated into the meridian
 *          plane (Scattering.phase_matrix_first_column); path1 = I0 / (4 pi mu_v a) sum_iz varpi_eff P_eff (e^{-tau_top a} -
 *          e^{-tau_bot a}), a = 1 / mu0 + 1 / mu_v, the layer factor as e^{-tau_top a} (-expm1(-tau a)).
 *   path2: brdf [nV,n_stokes] (brdf_spectral = 0) or [nV,n_stokes,S]; path2 = mu0 I0 brdf e^{-tau/mu0} e^{-tau/mu_v}.
 *   path34: pbar3_c_h / pbar4_c_h [C][nV][nQ] = the azimuthal averages of contributor c's phase function between inner node k and
 *          mu0 / mu_v; mu_nodes_h / w_h [nQ] the inner quadrature on (0, 1); _inner_scatter_sum and _tau_integral with its
 *          |1 / mu_first - 1 / mu_second| < 1e-10 trapezoid branch.  path3 or path4 may be NULL (its table is then not read); a
 *          point of zero albedo writes zeros.
 *   jac12: d1_tau / d1_varpi / d1_P [nV,n_stokes,S,L] (together, or all NULL) = d path1 / d (tau_layer, varpi_eff, P_eff);
 *          d2_tau [nV,n_stokes,S,L] and d2_rho [nV,n_stokes,S] (together, or both NULL) = d path2 / d (tau_layer, brdf). */
int vsm_exact_ss_path1_f64(int S, int L, int C, int nV, int n_stokes, const double* const* tau_c_h, const double* varpi_c_h,
                               const double* p_c_h, const double* I0, double mu0, const double* mu_v_h, double* path1, void* stream);
int vsm_exact_ss_path2_f64(int S, int L, int C, int nV, int n_stokes, const double* const* tau_c_h, const double* brdf,
                               int brdf_spectral, const double* I0, double mu0, const double* mu_v_h, double* path2, void* stream);
int vsm_exact_ss_path34_f64(int S, int L, int C, int nV, int nQ, const double* const* tau_c_h, const double* varpi_c_h,
                                const double* pbar3_c_h, const double* pbar4_c_h, const double* mu_nodes_h, const double* w_h, const double* albedo,
                                const double* I0, double mu0, const double* mu_v_h, double* path3, double* path4, void* stream);
int vsm_exact_ss_jac12_f64(int S, int L, int C, int nV, int n_stokes, const double* const* tau_c_h, const double* varpi_c_h,
                               const double* p_c_h, const double* brdf, int brdf_spectral, const double* I0, double mu0, const double* mu_v_h,
                               double* d1_tau, double* d1_varpi, double* d1_P, double* d2_tau, double* d2_rho, void* stream);
int vsm_exact_ss_path1_f32(int S, int L, int C, int nV, int n_stokes, const float* const* tau_c_h, const float* varpi_c_h,
                               const float* p_c_h, const float* I0, float mu0, const float* mu_v_h, float* path1, void* stream);
int vsm_exact_ss_path2_f32(int S, int L, int C, int nV, int n_stokes, const float* const* tau_c_h, const float* brdf,
                               int brdf_spectral, const float* I0, float mu0, const float* mu_v_h, float* path2, void* stream);
int vsm_exact_ss_path34_f32(int S, int L, int C, int nV, int nQ, const float* const* tau_c_h, const float* varpi_c_h,
                                const float* pbar3_c_h, const float* pbar4_c_h, const float* mu_nodes_h, const float* w_h, const float* albedo,
                                const float* I0, float mu0, const float* mu_v_h, float* path3, float* path4, void* stream);
int vsm_exact_ss_jac12_f32(int S, int L, int C, int nV, int n_stokes, const float* const* tau_c_h, const float* varpi_c_h,
                               const float* p_c_h, const float* brdf, int brdf_spectral, const float* I0, float mu0, const float* mu_v_h,
                               float* d1_tau, float* d1_varpi, float* d1_P, float* d2_tau, float* d2_rho, void* stream);

/* ---- Scattering: Mie (Siewert NAI-2) aerosol optics (src/Scattering/compute_NAI2.jl) ----------------------------------------
 * The optics of one aerosol -- a size distribution on nquad radius nodes and a refractive index n_r - i n_i at one wavelength --
 * as the Greek coefficients of its phase matrix, its bulk cross-sections and its single-scattering albedo.  FP64 only: the
 * reference forces Float64 for the D_n recurrence even in Float32 models.  The host part is small and stays with the caller
 * (compute_NAI2.jl:80-100, :113, :161); everything with an n_max, n_mu or nquad loop runs here, in three stages on `stream`:
 *   1. one lane per radius: D_n(y) downwards from round(max(n_max_i, |y|) + 51), a_n, b_n upwards (compute_mie_ab!), C_sca_i, C_ext_i;
 *   2. S1, S2 of every (angle, radius) on the FP64 MFMA with pi_n, tau_n generated in registers, turned into f11, f33, f12, f34,
 *      weighted with wr_i 0.5 / x_i^2 and summed over the radii -- no [n_mu, nquad] array exists; partial sums are combined in a
 *      fixed order, so a call is bit-identical to its repetition;
 *   3. the Greek coefficients alpha .. zeta, l = 0 .. n_mu - 1, from the quadrature sums of compute_NAI2.jl:188-202 with P, P2, R2,
 *      T2 generated by the recurrences of compute_legendre_poly.
 * Device arrays: x [nquad] size parameters 2 pi r_i / lambda (> 0), nmax_i [nquad] = get_n_max(x_i) (int; clamped to 1 .. n_max),
 * wx [nquad] the distribution's weights (sum 1), wr [nquad] = 4 pi r_i^2 wx_i, mu / w_mu [n_mu] the Gauss-Legendre nodes and
 * weights on (-1, 1).  Scalars: n_max >= 2 orders (>= every nmax_i), n_mu = 2 n_max - 1, k_wave = 2 pi / lambda.
 * Outputs (WRITTEN): greek [6, n_mu] row-major (alpha, beta, gamma, delta, epsilon, zeta; coefficient l at [c * n_mu + l]),
 * bulk_f [4, n_mu] (f11, f33, f12, f34 summed over the distribution, NOT divided by C_sca), scal [3] = bulk C_sca, bulk C_ext,
 * their ratio (the single-scattering albedo).  work: vsm_mie_work_elems(nquad, n_max, n_mu) doubles, uninitialised (0 is returned
 * for arguments vsm_mie_nai2 refuses).  No host synchronisation, no library scratch.
 * n_max above VSM_MIE_MAX_NMAX returns VSM_ERR_UNSUPPORTED (x = 500 needs 542); nquad < 1, n_max < 2, n_mu != 2 n_max - 1,
 * n_i < 0, n_r <= 0, k_wave <= 0 or a null pointer return VSM_ERR_INVALID_ARG; both before any launch. */
#define VSM_MIE_MAX_NMAX 1024
size_t vsm_mie_work_elems(int nquad, int n_max, int n_mu);
int vsm_mie_nai2(int nquad, int n_max, int n_mu, double n_r, double n_i, double k_wave, const double* x, const int* nmax_i,
                 const double* wx, const double* wr, const double* mu, const double* w_mu, double* greek, double* bulk_f,
                 double* scal, double* work, void* stream);

/* Linearized Mie (src/Scattering/compute_NAI2_lin.jl): vsm_mie_nai2 with the derivatives of all its outputs with respect to four
 * parameters, slots (n_r, n_i, p, q); p, q are the two parameters of the size distribution that the caller's wx_dot / wr_dot
 * [2, nquad] differentiate (d wx / d p, d wx / d q at fixed nodes, and 4 pi r_i^2 times them) -- for the reference's
 * LogNormal(mu, sigma): mu = ln r_m, sigma = ln sigma_g.  The three stages carry D_n', a_n', b_n', S1', S2' for n_r only: all of
 * them are holomorphic in m = n_r - i n_i, so d / d n_i = -i d / d n_r.
 * greek, bulk_f, scal: bit for bit those of vsm_mie_nai2 on the same inputs.  greek_dot [4, 6, n_mu], bulk_f_dot [4, 4, n_mu]
 * (unnormalised, like bulk_f), scal_dot [4, 3] = (C_sca', C_ext', ssa') per slot.  work: vsm_mie_lin_work_elems doubles.
 * Contract, limits and return codes: those of vsm_mie_nai2. */
size_t vsm_mie_lin_work_elems(int nquad, int n_max, int n_mu);
int vsm_mie_nai2_lin(int nquad, int n_max, int n_mu, double n_r, double n_i, double k_wave, const double* x, const int* nmax_i,
                     const double* wx, const double* wr, const double* wx_dot, const double* wr_dot, const double* mu,
                     const double* w_mu, double* greek, double* bulk_f, double* scal, double* greek_dot, double* bulk_f_dot,
                     double* scal_dot, double* work, void* stream);

/* ---- delta-BGE truncation of a phase matrix (src/Scattering/truncate_phase.jl) ----------------------------------------------------
 * Fits l_max truncated Greek coefficients to a phase matrix given by n_mu of them (Sanghavi & Stephens 2015): beta on the Legendre
 * polynomials, gamma and epsilon on fac_l P2_l (l = 2 .. l_max - 1), each a weighted least-squares fit over the Gauss-Legendre
 * nodes mu, w_mu of order n_mu, solved through its normal equations.  FP64 only.  Three stages on `stream`:
 *   1. one lane per node: f11, f12, f34 there -- bulk_f / scal[0] if vsm_mie_nai2's bulk_f [4, n_mu] and scal are handed over,
 *      else reconstructed from the n_mu coefficients (reconstruct_phase) -- and the basis functions times the square root of the
 *      node's weight, with one more row that makes the right-hand side;
 *   2. [A | b] = B B^T per system on the FP64 MFMA, tiles on and above the diagonal; the angle axis is split over workgroups whose
 *      partial sums are added in a fixed order, so a call is bit-identical to its repetition;
 *   3. one workgroup per system: Cholesky (as L D L^T) and the triangular solves in LDS, then c0 = cl_0, beta_t = cl / c0,
 *      alpha_t = (alpha - (beta - cl)) / c0 (delta_t, zeta_t alike), gamma_t and epsilon_t the solutions themselves (NOT divided
 *      by c0, as in the reference).
 * lowconf = 0: truncate_phase -- all nodes, weights w / f^2 (cos_delta is not read).  lowconf = m > 0: truncate_phase_lowconf --
 * only the nodes with mu < cos_delta, of which the caller has counted m, weights (w / max(|f|, 1e-8))^2.
 * Inputs (device, READ): greek [6, n_mu] row-major (alpha .. zeta), bulk_f and scal (both or neither), mu, w_mu [n_mu].
 * Outputs (WRITTEN): greek_t [6, l_max], scal_t [2] = c0, f_trunc = 1 - c0, info [3] per system (beta, gamma, epsilon):
 * 0 = solved, 1 = skipped -- a gamma / epsilon series of exact zeros from l = 2 on stays exact zeros (the reference divides by
 * f12 = 0 there) --, 2 = the normal equations are not positive definite or not finite, or (lowconf = 0) f11 is not positive at
 * a node; that system's outputs are NaN.  work: vsm_dbge_work_elems(n_mu, l_max) doubles, uninitialised (0 is returned for
 * arguments vsm_truncate_dbge refuses).  No host synchronisation, no library scratch, no atomics.
 * l_max above VSM_DBGE_MAX_L returns VSM_ERR_UNSUPPORTED; l_max < 3, n_mu <= l_max, lowconf < 0, 0 < lowconf < l_max,
 * lowconf > n_mu, exactly one of bulk_f and scal null or a null required pointer return VSM_ERR_INVALID_ARG; both before any
 * launch. */
#define VSM_DBGE_MAX_L 128
size_t vsm_dbge_work_elems(int n_mu, int l_max);
int vsm_truncate_dbge(int n_mu, int l_max, int lowconf, double cos_delta, const double* greek, const double* bulk_f,
                      const double* scal, const double* mu, const double* w_mu, double* greek_t, double* scal_t, int* info,
                      double* work, void* stream);

/* Linearized delta-BGE truncation (src/Scattering/truncate_phase_lin.jl): vsm_truncate_dbge and, in the same call, the
 * derivatives of its outputs with respect to four parameters (the slots of vsm_mie_nai2_lin), FP64.  Only the all-nodes fit is
 * linearized: lowconf must be 0.  With A x = b the normal equations of a system and B the basis rows sqrt(w) B_i / f that
 * vsm_truncate_dbge already forms (A = B B^T), x' = A^-1 B g with g_k = (f'_k / f_k) (2 (B^T x)_k - sqrt(w_k)): no second Gram
 * product; the four right-hand sides go through the factor the forward solve holds.
 * Inputs beyond vsm_truncate_dbge's: greek_dot [4, 6, n_mu]; bulk_f_dot [4, 4, n_mu] and scal_dot [4, 3] of vsm_mie_nai2_lin,
 * which come with bulk_f and scal or not at all (without them f' is reconstructed from greek_dot as f is from greek).
 * Outputs: greek_t, scal_t, info -- bit for bit those of vsm_truncate_dbge on the same inputs --, greek_t_dot [4, 6, l_max],
 * scal_t_dot [4, 2] = (c0', f_trunc' = -c0') per slot.  A skipped system (info = 1) has exact-zero derivative rows; a failed
 * one (2) NaN rows; a non-finite derivative of a solved system sets its info to 2 and its derivative rows to NaN.
 * work: vsm_dbge_lin_work_elems(n_mu, l_max) doubles, uninitialised (0 for refused shapes).  Contract and return codes: those
 * of vsm_truncate_dbge; lowconf != 0 returns VSM_ERR_UNSUPPORTED; a null greek_dot, greek_t_dot or scal_t_dot, or bulk_f_dot /
 * scal_dot without bulk_f / scal (or the reverse) VSM_ERR_INVALID_ARG; all before any launch. */
size_t vsm_dbge_lin_work_elems(int n_mu, int l_max);
int vsm_truncate_dbge_lin(int n_mu, int l_max, int lowconf, double cos_delta, const double* greek, const double* bulk_f,
                          const double* scal, const double* greek_dot, const double* bulk_f_dot, const double* scal_dot,
                          const double* mu, const double* w_mu, double* greek_t, double* scal_t, double* greek_t_dot,
                          double* scal_t_dot, int* info, double* work, void* stream);

/* ---- Absorption: line-by-line cross-sections of a whole profile (src/Absorption/compute_absorption_cross_section.jl) ---------
 * sigma(nu_i) of one gas at every layer of a (p, T, vmr) profile from a HITRAN line table, FP64: per line the pressure shift, the
 * Lorentz and Doppler widths, S(T) (:108-153, constants of constants/constants.jl) and the index window of the wing cutoff; per
 * grid point the sum of the line shapes of line_shape_batch! (:252-319) over the lines whose window holds the point, in table
 * order.  Two launches on `stream` whatever Nz is:
 *   1. one lane per (layer, line): the line parameters into work [Nz, nLines, VSM_ABS_WORK_FIELDS] = (nu, gamma_d, gamma_l, y, S,
 *      S c / gamma_d, sqrt(ln 2) / gamma_d, (istart, istop) as two ints).  The window is the fractional 1-based index of nu -/+
 *      wing_cutoff by linear interpolation on the grid (binary search), clamped to 1 / nSpec, rounded to nearest, ties to even;
 *      nSpec = 1 gives [1, 1].  A line whose shifted window [nu - wing_cutoff, nu + wing_cutoff] misses the grid gets an EMPTY
 *      window (the reference extrapolates its upper index with nSpec on both sides and gives such a line every point);
 *   2. one workgroup per (tile of 256 points, layer), one point per lane: the lines with nu0 within the tile widened by one point,
 *      wing_cutoff and delta_max p / p_ref (binary search on nu0) pass through LDS in chunks of VSM_ABS_CHUNK lines; a line whose
 *      window misses all 64 points of a wave is skipped by that wave; scale[layer] multiplies the sum once.
 * Device arrays (READ): grid [nSpec] wavenumbers, strictly ascending (not necessarily uniform); the table sorted by nu0 ascending:
 * nu0, S_ref, gamma_air, gamma_self, n_air, delta_air, E_low [nLines] (E_low = -1: S(T) = S_ref), species [nLines] (int, 0 ..
 * nSpecies - 1); molar_mass [nSpecies]; p (hPa), T (K), vmr_self, scale [Nz] (1 for sigma, vcd vmr for tau); qratio [Nz, nSpecies]
 * = Q(T_ref) / Q(T), computed by the caller.  Scalars: wing_cutoff >= 0; delta_max >= max |delta_air| of the table (a smaller
 * value drops lines); broadening VSM_ABS_DOPPLER / LORENTZ / VOIGT; cef VSM_ABS_CEF_* (read under Voigt only; the |x| + y and
 * CPF12 region branches are taken per lane); accumulate 0: out is WRITTEN, 1: the result is added to out.
 * out [Nz, nSpec].  work: vsm_absorption_work_elems(Nz, nLines) = VSM_ABS_WORK_FIELDS Nz nLines doubles, uninitialised (0 for
 * Nz < 1 or nLines < 1).  No host synchronisation, no library scratch, no atomics; a call is bit-identical to its repetition.
 * A size < 1, Nz > 65535, wing_cutoff or delta_max negative or NaN, a broadening, cef or accumulate outside its values or a null
 * pointer return VSM_ERR_INVALID_ARG before any launch. */
#define VSM_ABS_CHUNK 256
#define VSM_ABS_WORK_FIELDS 8
#define VSM_ABS_DOPPLER 0
#define VSM_ABS_LORENTZ 1
#define VSM_ABS_VOIGT 2
#define VSM_ABS_CEF_HW32_VOIGT 0 /* HumlicekWeidemann32VoigtErrorFunction */
#define VSM_ABS_CEF_HW32_SD 1    /* HumlicekWeidemann32SDErrorFunction */
#define VSM_ABS_CEF_CPF12 2      /* CPF12ErrorFunction */
int vsm_absorption_chunk(void); /* VSM_ABS_CHUNK of the loaded library */
size_t vsm_absorption_work_elems(int Nz, int nLines);
int vsm_absorption_xsec(int nSpec, int nLines, int nSpecies, int Nz, const double* grid, const double* nu0, const double* S_ref,
                        const double* gamma_air, const double* gamma_self, const double* n_air, const double* delta_air,
                        const double* E_low, const int* species, const double* molar_mass, const double* p, const double* T,
                        const double* vmr_self, const double* scale, const double* qratio, double wing_cutoff, double delta_max,
                        int broadening, int cef, int accumulate, double* out, double* work, void* stream);

/* ---- Linearized Absorption: d sigma / d(T, p, vmr_self) per layer, beside sigma (ours; the reference has no such derivative) ----
 * The derivative of the function vsm_absorption_xsec evaluates, with the index windows [istart, istop] and, per (line, point), the
 * region of the error function (Weideman / Humlicek I / II) frozen at the unperturbed state.  With term = pre F(x, y),
 * x = sx (nu_i - nu): d term / d theta = pre (dlnpre_theta F + F_x x_theta + F_y y_theta), F_x = Re w', F_y = -Im w' under Voigt,
 * w' the closed-form derivative of each approximant (never -2 z w + 2 i / sqrt(pi)); Doppler and Lorentz have elementary F.
 *   T:        dlnpre = dlnS/dT - 1/(2T) (Lorentz: dlnS/dT), x_T = -x/(2T) (Lorentz: 0), y_T = -y (n_air + 1/2)/T (Lorentz: -n_air gamma_l/T)
 *   p:        x_p = -sx delta_air / p_ref, y_p = y / p
 *   vmr_self: y_v = sqrt(ln 2)/gamma_d (gamma_self - gamma_air) (p/p_ref) (T_ref/T)^n_air (Lorentz: without sqrt(ln 2)/gamma_d; Doppler: 0)
 *   dlnS/dT = qratio_dlnT + c2 E_low / T^2 - (a/T) / expm1(a), a = c2 nu0 / T; 0 for E_low = -1.
 * Four launches on `stream`: the two of vsm_absorption_xsec, unchanged, on the first VSM_ABS_WORK_FIELDS Nz nLines doubles of
 * `work` -- `out` is bit for bit that call's --; k_abs_params_lin, one lane per (layer, line), which takes nu, the window, pre, sx
 * and y from that record (so x, y, the windows and the regions are the forward's to the bit) and adds the five derivative factors,
 * VSM_ABS_LIN_WORK_FIELDS doubles per (layer, line) behind the forward's; k_abs_accum_lin, decomposed as the forward's second
 * kernel (one workgroup per (256 points, layer), binary search on nu0, LDS chunks of VSM_ABS_LIN_CHUNK lines, scalar window skip per
 * wave, table-order sums), w and w' once per (line, point), three sums per lane.
 * Inputs: those of vsm_absorption_xsec (p > 0), and qratio_dlnT [Nz, nSpecies] = d ln(Q(T_ref)/Q(T)) / dT.
 * Outputs: out [Nz, nSpec] as vsm_absorption_xsec's; out_dT (K^-1), out_dp (hPa^-1), out_dvmr (1), each [Nz, nSpec] -- the three
 * planes of one [3, Nz, nSpec] array or separate arrays (a caller that sums gases through `accumulate` shares the T and p planes
 * and gives each gas a zeroed vmr plane).  scale[layer] and accumulate apply to all four outputs alike.
 * work: vsm_absorption_lin_work_elems(Nz, nLines) = (VSM_ABS_WORK_FIELDS + VSM_ABS_LIN_WORK_FIELDS) Nz nLines doubles.
 * Refusals, before any launch: those of vsm_absorption_xsec; a null qratio_dlnT or output plane; broadening = VSM_ABS_VOIGT with
 * cef = VSM_ABS_CEF_CPF12 (not linearized: its region II is no analytic formula), all VSM_ERR_INVALID_ARG. */
#define VSM_ABS_LIN_CHUNK 256
#define VSM_ABS_LIN_WORK_FIELDS 10
int vsm_absorption_lin_chunk(void);
size_t vsm_absorption_lin_work_elems(int Nz, int nLines);
int vsm_absorption_xsec_lin(int nSpec, int nLines, int nSpecies, int Nz, const double* grid, const double* nu0, const double* S_ref,
                            const double* gamma_air, const double* gamma_self, const double* n_air, const double* delta_air,
                            const double* E_low, const int* species, const double* molar_mass, const double* p, const double* T,
                            const double* vmr_self, const double* scale, const double* qratio, const double* qratio_dlnT,
                            double wing_cutoff, double delta_max, int broadening, int cef, int accumulate, double* out,
                            double* out_dT, double* out_dp, double* out_dvmr, double* work, void* stream);
/* profile slots of compute_absorption_profile_lin: out [K, Nz, nSpec] = dT [Nz, nSpec] T_dot [K, Nz] + dp [Nz, nSpec] p_dot [K, Nz];
 * one launch on `stream`.  A size < 1, Nz or K > 65535 or a null pointer returns VSM_ERR_INVALID_ARG before it. */
int vsm_absorption_profile_slots(int nSpec, int Nz, int K, const double* dT, const double* dp, const double* T_dot,
                                 const double* p_dot, double* out, void* stream);

/* ---- Absorption.InterpolationModel: sigma(nu, p, T) lookup tables (make_model_helpers.jl:55-122, ----------------------------
 * compute_absorption_cross_section.jl:181-233).  Three uniform axes (first, step != 0, n >= 2) with the FP64 nodes x_k = first +
 * k step; x lies in cell i = [x_i, x_i+1) (the last cell closed; i clamped to 0 .. n - 2) at t = (x - x_i) / (x_i+1 - x_i): that is
 * (x - first) / step - i up to the rounding of the nodes, and exactly 0 on a node.  VSM_LUT_LINEAR: the coefficients are the values, [nP, nT, nNu] (nu contiguous),
 * trilinear.  VSM_LUT_CUBIC (the reference's BSpline(Cubic(Line(OnGrid())))): coefficients [nP + 2, nT + 2, nNu + 2], per axis
 * c[i-1]/6 + 2c[i]/3 + c[i+1]/6 = y[i], c[0] - 2c[1] + c[2] = 0 = c[n-1] - 2c[n] + c[n+1]; 4 taps per axis on c[i .. i+3] with
 * weights (1-t)^3/6, (3t^3 - 6t^2 + 4)/6, (-3t^3 + 3t^2 + 3t + 1)/6, t^3/6.  Storage VSM_LUT_F64 / VSM_LUT_F32 (float
 * coefficients, FP64 arithmetic).
 *
 * vsm_absorption_lut_prefilter: values [nP nT, nNu] (the layout vsm_absorption_xsec leaves for the nP nT states, T fastest) ->
 * cubic coefficients, FP64, on `stream`: the nu axis by lanes that each solve VSM_LUT_CHUNK unknowns on a window widened by 32
 * nodes per side, then the T and the p axis one lane per system; FP32 storage rounds once at the end.  work:
 * vsm_absorption_lut_work_elems(nNu, nP, nT, storage) doubles, uninitialised (0 for refused sizes).  No atomics.
 *
 * vsm_absorption_lut_eval: out [Nz, nSpec] = (accumulate ? out : 0) + scale[z] sigma_itp(grid[s], p[z], T[z]); one launch.  grid
 * [nSpec] is any finite array (unsorted, descending); a point outside [min, max] of the nu axis gives exact 0 (adds nothing).
 * p[z], T[z] are the CALLER's to keep inside their axes: outside they are evaluated in the end cell (no fault).  A workgroup
 * collapses the (p, T) taps once per table column its 256 points touch, in LDS, unless they span more than VSM_LUT_SPAN columns:
 * then per point from memory; the same fma chain either way.
 * vsm_absorption_lut_eval_lin: the same sigma, bit for bit, and out_dT (K^-1), out_dp (hPa^-1) [Nz, nSpec] from the derivative
 * weights of the T and p axis over the step; linear: the derivative of the cell the forward evaluates in.  scale and accumulate
 * apply to all three outputs.
 * Contract of vsm_absorption_xsec: no host synchronisation, no library scratch, bit-identical repetitions.  An axis with n < 2, a
 * size < 1, Nz > 65535, a step that is 0 or not finite, a bad enum or a null pointer return VSM_ERR_INVALID_ARG before any launch. */
#define VSM_LUT_CHUNK 32
#define VSM_LUT_SPAN 1024
#define VSM_LUT_LINEAR 0
#define VSM_LUT_CUBIC 1
#define VSM_LUT_F64 0
#define VSM_LUT_F32 1
int vsm_absorption_lut_chunk(void); /* VSM_LUT_CHUNK of the loaded library */
int vsm_absorption_lut_span(void);  /* VSM_LUT_SPAN of the loaded library */
size_t vsm_absorption_lut_work_elems(int nNu, int nP, int nT, int storage);
int vsm_absorption_lut_prefilter(int nNu, int nP, int nT, const double* values, int storage, void* coef, double* work,
                                 void* stream);
int vsm_absorption_lut_eval(int nSpec, int Nz, int nNu, int nP, int nT, double nu_first, double nu_step, double p_first,
                            double p_step, double T_first, double T_step, int interp, int storage, const void* coef,
                            const double* grid, const double* p, const double* T, const double* scale, int accumulate, double* out,
                            void* stream);
int vsm_absorption_lut_eval_lin(int nSpec, int Nz, int nNu, int nP, int nT, double nu_first, double nu_step, double p_first,
                                double p_step, double T_first, double T_step, int interp, int storage, const void* coef,
                                const double* grid, const double* p, const double* T, const double* scale, int accumulate,
                                double* out, double* out_dT, double* out_dp, void* stream);

/* ---- Absorption continua: HITRAN CIA (src/Absorption/cia.jl) and the MT_CKD H2O continuum (src/Absorption/mtckd.jl) -----------
 * A continuum SET is nTables <= VSM_CONT_MAX_TABLES CIA tables plus at most one MT_CKD band, all on one spectral grid of nSpec
 * points.  ONE launch on `stream` adds the whole set to its output planes [Nz, nSpec] for all Nz layers: a workgroup owns 256 points
 * and a tile of VSM_CONT_LAYERS layers, a lane keeps nu and the band values of its point in registers over the tile, and a plane
 * is read (if it accumulates) and written once per set: plane = (accumulate ? plane : 0) + value, per plane.
 *
 * CIA, per table k in list order, FP64, only + - x and no contraction (the chain is fixed and tested to the bit):
 *   a = table_k[j0, s], b = table_k[j1, s];  s_k = (1 - w) a + w b;  plane_m += s_k A[m, k, z];  plane_1 += (b - a) B[1, k, z].
 * tables: HOST array of nTables DEVICE pointers, table k [nT[k], nSpec] (nu contiguous); nT: host array.  Device arrays: rows
 * [nTables, Nz, 2] ints (j0, j1; clamped into the table by the kernel), w [nTables, Nz], A (and B) [nPlanes, nTables, Nz]: the
 * caller's per-layer coefficients (cia_σ_at_T!'s cell and weight; v_a v_b n_air^2 Δz_cm and its derivatives).  Of B only plane 1
 * is read.
 * MT_CKD, behind the tables, self then foreign: nu, C_self, C_for, texp [nSpec] on the device (all null: no band) and band_layer
 * [Nz, VSM_CONT_BAND_FIELDS] = (T, T_ref / T, S, F, 2S/p, 2F/p, dS/dv, dF/dv, S/Δz, F/Δz) with S = (v p / p_ref) v n_air Δz_cm and
 * F = ((1 - v) p / p_ref) v n_air Δz_cm.  With x = 1.4388 nu / (2T): g_s = nu tanh(x) C_self (T_ref/T)^texp, g_f = nu tanh(x) C_for,
 *   tau += g_s S, += g_f F;  d/dT += g_s S t_s, += g_f F t_f, t_s = -(q + texp + 1)/T, t_f = -(q + 1)/T, q = 2x / sinh(2x) (1 at
 *   nu = 0);  d/dp, d/dv(H2O), d/dΔz += g_s and g_f times fields 4/5, 6/7, 8/9.  nu = 0 and zero coefficients give exact 0.
 * Planes of vsm_absorption_continuum_lin (HOST arrays `planes` of nPlanes device pointers and `accumulate` of nPlanes flags):
 * 0 tau, 1 d/dT, 2 d/dp, 3 .. nPlanes - 1 the caller's: vmr planes, which the band enters at h2o_plane, and d/dΔz at ddz_plane (-1:
 * none).  Plane 0 has the bits of vsm_absorption_continuum with the same inputs.  3 <= nPlanes <= VSM_CONT_MAX_PLANES.
 * Contract of vsm_absorption_lut_eval: no host synchronisation, no library scratch, no atomics, bit-identical repetitions; a
 * point's result does not depend on its lane, its layer tile or Nz.  A size < 1, Nz > 65535, nTables outside 0 ..
 * VSM_CONT_MAX_TABLES, an empty set, nT[k] < 1, a band with one of its five arrays missing, nPlanes, h2o_plane (3 .. nPlanes - 1
 * with a band, -1 without) or ddz_plane out of range, an accumulate flag outside 0 / 1, two planes that are one array or a null
 * pointer return VSM_ERR_INVALID_ARG before any launch.
 *
 * vsm_absorption_profile_slots_add: out [K, Nz, nSpec] += plane [Nz, nSpec] tab [K, Nz], one launch (the Δz share of the profile
 * slots behind vsm_absorption_profile_slots); refusals as that call's. */
#define VSM_CONT_MAX_TABLES 8
#define VSM_CONT_MAX_PLANES 24
#define VSM_CONT_LAYERS 4
#define VSM_CONT_BAND_FIELDS 10
int vsm_absorption_continuum_layers(void); /* VSM_CONT_LAYERS of the loaded library */
int vsm_absorption_continuum(int nSpec, int Nz, int nTables, const double* const* tables, const int* nT, const int* rows,
                             const double* w, const double* A, const double* nu, const double* C_self, const double* C_for,
                             const double* texp, const double* band_layer, int accumulate, double* out, void* stream);
int vsm_absorption_continuum_lin(int nSpec, int Nz, int nTables, const double* const* tables, const int* nT, const int* rows,
                                 const double* w, int nPlanes, const double* A, const double* B, const double* nu,
                                 const double* C_self, const double* C_for, const double* texp, const double* band_layer,
                                 int h2o_plane, int ddz_plane, const int* accumulate, double* const* planes, void* stream);
int vsm_absorption_profile_slots_add(int nSpec, int Nz, int K, const double* plane, const double* tab, double* out, void* stream);

/* ---- diagnostics used by the parity tests -------------------------------- */
/* Runs the LDS-resident MFMA tile product used inside the fused kernels on plain
 * [N,N,S] inputs: C = A*B.  (Checks fragment layouts / swizzle independently.) */
int vsm_test_lds_mm_f64(int N, int S, const double* A, const double* B, double* C, void* stream);
int vsm_test_lds_mm_f32(int N, int S, const float* A, const float* B, float* C, void* stream);
/* Inverse via the fused kernels' LDS path (series fast path + pivoted Gauss-Jordan fallback).
 * mode: 0 = automatic, 1 = force Gauss-Jordan, 2 = force Neumann series. path_out (nullable,
 * int[S]) receives the path taken per point (1 = GJ, 2.. = series order + 1). */
int vsm_test_lds_inv_f64(int N, int S, const double* A, double* X, int mode, int* path_out, void* stream);
int vsm_test_lds_inv_f32(int N, int S, const float* A, float* X, int mode, int* path_out, void* stream);

/* Fills the whole LDS of every CU with NaN bit patterns (the GPU tests call it before every test: no kernel may depend
 * on what a previous workgroup left in LDS). */
int vsm_test_poison_lds(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSMARTMOM_HIP_H */
