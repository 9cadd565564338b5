// Exact single-scattering (src/StandaloneSS): the first-order field at the true scattering angle of every viewing geometry,
// split into four paths (StandaloneSS/kernels.jl), and the hand-coded Jacobians of paths 1 and 2 (linearized_f2.jl:34-101).
//   vsm_exact_ss_path1_*   _path1_kernel! / _path1_stokes_kernel!   one scattering in the atmosphere
//   vsm_exact_ss_path2_*   _path2_kernel! / _path2_stokes_kernel!   the direct beam reflected by the surface
//   vsm_exact_ss_path34_*  _path34_kernel! (_path3_kernel! / _path4_kernel! with one output null), _inner_scatter_sum, _tau_integral
//   vsm_exact_ss_jac12_*   _path1_jacobians / _path2_jacobians
// The reference mixes the contributors on the host into P_eff[nGeom, nStokes, nLayer, nSpec] and, for paths 3 and 4, into two
// arrays Pbar[nGeom, nLayer, nSpec, nQuad].  Every contributor's phase function is spectrally flat, so here a thread mixes them per
// (layer, point) from the contributors' optical depths tau_c[L][S], their albedos and one small table per contributor:
//   varpi_eff P_eff = (sum_c tau_c varpi_c p_c) / tau      (zero where tau = 0)
// and none of those arrays exists.  Lanes run along the spectral axis; a thread walks the layers of its point for one viewing
// geometry (grid.y) and carries the running optical depth in registers.  Nothing here is N x N.
#include "vsm_common.h"
#include "vsm_internal.h"

namespace vsm {

constexpr int XS_TB = VSM_SS_BLOCK;   // spectral points (= threads) per workgroup: two waves
constexpr int XS_SLOT = 6;            // library scratch slot of the device tables
constexpr int XS_CR = 4;              // path 3/4: contributors whose layer weight tau_c varpi_c a thread keeps in registers

template <typename T>
__device__ __forceinline__ T xs_pi() {
  return T(3.141592653589793238462643383279502884);
}

// One layer of one point: tau = sum_c tau_c, ts = sum_c tau_c varpi_c, sp[k] = sum_c tau_c varpi_c p_c[c][v][k]
template <typename T>
__device__ __forceinline__ void xs_mix(const T* const* __restrict__ tc, const T* __restrict__ wc, const T* __restrict__ pc, int C, int L,
                                       int nV, int ns, int v, int iz, long long s, T& tau, T& ts, T (&sp)[4]) {
  tau = ts = T(0);
#pragma unroll
  for (int k = 0; k < 4; ++k) sp[k] = T(0);
  for (int c = 0; c < C; ++c) {
    const T t = tc[(long long)c * L + iz][s];
    const T sw = t * wc[c];
    tau += t;
    ts += sw;
    const T* p = pc + ((long long)c * nV + v) * ns;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < ns) sp[k] += sw * p[k];
  }
}
template <typename T>
__device__ __forceinline__ T xs_layer_tau(const T* const* __restrict__ tc, int C, int L, int iz, long long s) {
  T tau = T(0);
  for (int c = 0; c < C; ++c) tau += tc[(long long)c * L + iz][s];
  return tau;
}

// ---------------------------------------------------------------------------------------------------------------------
// path 1
// ---------------------------------------------------------------------------------------------------------------------
// path1[v, k, s] = I0 / (4 pi mu_v a) sum_iz varpi_eff P_eff[k] (e^{-tau_top a} - e^{-tau_bot a}),  a = 1 / mu_0 + 1 / mu_v.
// The layer factor is e^{-tau_top a} (-expm1(-tau a)): no cancellation in a thin layer.
template <typename T>
__global__ __launch_bounds__(XS_TB) void k_xs_path1(int S, int L, int C, int nV, int ns, const T* const* __restrict__ tc,
                                                    const T* __restrict__ wc, const T* __restrict__ pc, const T* __restrict__ I0, T mu0,
                                                    const T* __restrict__ muv, T* out) {
  const long long s = (long long)blockIdx.x * XS_TB + threadIdx.x;
  if (s >= S) return;
  const int v = blockIdx.y;
  const T mv = muv[v];
  const T a = T(1) / mu0 + T(1) / mv;
  const T pre = I0[s] / (T(4) * xs_pi<T>() * mv * a);
  T acc[4] = {0, 0, 0, 0};
  T tcum = T(0), etop = T(1);
  for (int iz = 0; iz < L; ++iz) {
    T tau, ts, sp[4];
    xs_mix<T>(tc, wc, pc, C, L, nV, ns, v, iz, s, tau, ts, sp);
    const T tbot = tcum + tau;
    const T ebot = exp(-tbot * a);
    if (tau != T(0)) {
      const T f = etop * (-expm1(-tau * a)) / tau;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += sp[k] * f;
    }
    tcum = tbot;
    etop = ebot;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < ns) out[v + (long long)nV * (k + (long long)ns * s)] = pre * acc[k];
}

// ---------------------------------------------------------------------------------------------------------------------
// path 2
// ---------------------------------------------------------------------------------------------------------------------
// path2[v, k, s] = mu_0 I0 brdf[v, k(, s)] e^{-tau / mu_0} e^{-tau / mu_v}
template <typename T>
__global__ __launch_bounds__(XS_TB) void k_xs_path2(int S, int L, int C, int nV, int ns, const T* const* __restrict__ tc,
                                                    const T* __restrict__ brdf, int spectral, const T* __restrict__ I0, T mu0,
                                                    const T* __restrict__ muv, T* out) {
  const long long s = (long long)blockIdx.x * XS_TB + threadIdx.x;
  if (s >= S) return;
  const int v = blockIdx.y;
  const T mv = muv[v];
  T tau = T(0);
  for (int iz = 0; iz < L; ++iz) tau += xs_layer_tau<T>(tc, C, L, iz, s);
  const T att = exp(-tau / mu0) * exp(-tau / mv);
  for (int k = 0; k < ns; ++k) {
    const long long o = v + (long long)nV * (k + (long long)ns * s);
    out[o] = (mu0 * I0[s] * brdf[spectral ? o : (long long)(v + nV * k)]) * att;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// paths 3 and 4 (scalar radiance, Lambertian surface)
// ---------------------------------------------------------------------------------------------------------------------
// _tau_integral (kernels.jl:62-71)
template <typename T>
__device__ __forceinline__ T xs_tau_integral(T ttop, T tbot, T ttot, T m1, T m2) {
  const T b = T(1) / m1 - T(1) / m2;
  const T ft = exp(-ttop / m1 - (ttot - ttop) / m2);
  const T fb = exp(-tbot / m1 - (ttot - tbot) / m2);
  if (fabs(b) < T(1e-10)) return T(0.5) * (ft + fb) * (tbot - ttop);
  return (ft - fb) / b;
}

// varpi_eff Pbar[v, iz, s, k] = (sum_c tau_c varpi_c pbar_c[c][v][k]) / tau is formed per inner node from the layer weights of the
// contributors: the first XS_CR of them wait in registers, further ones are read again (the same cache lines) per node.
template <typename T>
__global__ __launch_bounds__(XS_TB) void k_xs_path34(int S, int L, int C, int nV, int nQ, const T* const* __restrict__ tc,
                                                     const T* __restrict__ wc, const T* __restrict__ pb3, const T* __restrict__ pb4,
                                                     const T* __restrict__ mun, const T* __restrict__ wq, const T* __restrict__ albedo,
                                                     const T* __restrict__ I0, T mu0, const T* __restrict__ muv, T* out3, T* out4) {
  const long long s = (long long)blockIdx.x * XS_TB + threadIdx.x;
  if (s >= S) return;
  const int v = blockIdx.y;
  const long long o = v + (long long)nV * s;
  const T rho = albedo[s] / xs_pi<T>();
  if (rho == T(0)) {
    if (out3) out3[o] = T(0);
    if (out4) out4[o] = T(0);
    return;
  }
  const T mv = muv[v];
  T ttot = T(0);
  for (int iz = 0; iz < L; ++iz) ttot += xs_layer_tau<T>(tc, C, L, iz, s);
  T sum3 = T(0), sum4 = T(0), tcum = T(0);
  for (int iz = 0; iz < L; ++iz) {
    T sw[XS_CR], tau = T(0), ts = T(0);
#pragma unroll
    for (int c = 0; c < XS_CR; ++c) {
      sw[c] = T(0);
      if (c < C) {
        const T t = tc[(long long)c * L + iz][s];
        sw[c] = t * wc[c];
        tau += t;
        ts += sw[c];
      }
    }
    for (int c = XS_CR; c < C; ++c) {
      const T t = tc[(long long)c * L + iz][s];
      tau += t;
      ts += t * wc[c];
    }
    const T ttop = tcum, tbot = tcum + tau;
    tcum = tbot;
    if (ts == T(0)) continue;   // varpi_eff = 0 (_inner_scatter_sum returns zero); tau = 0 implies it
    T l3 = T(0), l4 = T(0);
    for (int k = 0; k < nQ; ++k) {
      const T mk = mun[k];
      T m3 = T(0), m4 = T(0);
#pragma unroll
      for (int c = 0; c < XS_CR; ++c)
        if (c < C) {
          const long long q = ((long long)c * nV + v) * nQ + k;
          if (out3) m3 += sw[c] * pb3[q];
          if (out4) m4 += sw[c] * pb4[q];
        }
      for (int c = XS_CR; c < C; ++c) {
        const T swc = tc[(long long)c * L + iz][s] * wc[c];
        const long long q = ((long long)c * nV + v) * nQ + k;
        if (out3) m3 += swc * pb3[q];
        if (out4) m4 += swc * pb4[q];
      }
      const T hw = wq[k] * T(0.5);
      if (out3) l3 += hw * m3 * xs_tau_integral<T>(ttop, tbot, ttot, mu0, mk);
      if (out4) l4 += hw * m4 * xs_tau_integral<T>(ttop, tbot, ttot, mv, mk);
    }
    sum3 += l3 / tau;
    sum4 += l4 / tau;
  }
  if (out3) out3[o] = rho * (I0[s] * sum3) * exp(-ttot / mv);
  if (out4) out4[o] = rho * mu0 * I0[s] * exp(-ttot / mu0) * sum4 / mv;
}

// ---------------------------------------------------------------------------------------------------------------------
// Jacobians of paths 1 and 2 with respect to the seam variables tau_layer, varpi_eff, P_eff and the surface BRDF
// ---------------------------------------------------------------------------------------------------------------------
// Path 1, layer iz (linearized_f2.jl:49-67), c0 = I0 / (4 pi mu_v), lf = e^{-tau_top a} - e^{-tau_bot a}:
//   d/dvarpi = c0 / a P lf,   d/dP = c0 / a varpi lf,   d/dtau = c0 varpi P e^{-tau_bot a} - sum_{j > iz} c0 varpi_j P_j lf_j.
// The last term is a suffix sum: the walk goes upward from the surface and carries it (the reference adds it layer by layer).
// Path 2: d/dtau = -path2 (1 / mu_0 + 1 / mu_v) in every layer, d/drho = mu_0 I0 e^{-tau / mu_0} e^{-tau / mu_v}.
template <typename T>
__global__ __launch_bounds__(XS_TB) void k_xs_jac12(int S, int L, int C, int nV, int ns, const T* const* __restrict__ tc,
                                                    const T* __restrict__ wc, const T* __restrict__ pc, const T* __restrict__ brdf,
                                                    int spectral, const T* __restrict__ I0, T mu0, const T* __restrict__ muv, T* d1t,
                                                    T* d1w, T* d1p, T* d2t, T* d2r) {
  const long long s = (long long)blockIdx.x * XS_TB + threadIdx.x;
  if (s >= S) return;
  const int v = blockIdx.y;
  const T mv = muv[v];
  const T a = T(1) / mu0 + T(1) / mv;
  T ttot = T(0);
  for (int iz = 0; iz < L; ++iz) ttot += xs_layer_tau<T>(tc, C, L, iz, s);
  const long long per = (long long)nV * ns * S;
  const long long o0 = v + (long long)nV * ns * s;
  if (d2t) {
    const T att = exp(-ttot / mu0) * exp(-ttot / mv);
    for (int k = 0; k < ns; ++k) {
      const long long o = o0 + (long long)nV * k;
      const T dr = mu0 * I0[s] * att;
      const T p2 = (mu0 * I0[s] * brdf[spectral ? o : (long long)(v + nV * k)]) * att;
      d2r[o] = dr;
      for (int iz = 0; iz < L; ++iz) d2t[o + per * iz] = -p2 * a;
    }
  }
  if (!d1t) return;
  const T c0 = I0[s] / (T(4) * xs_pi<T>() * mv);
  const T pre = c0 / a;
  T suf[4] = {0, 0, 0, 0};
  T tbot = ttot, ebot = exp(-ttot * a);
  for (int iz = L - 1; iz >= 0; --iz) {
    T tau, ts, sp[4];
    xs_mix<T>(tc, wc, pc, C, L, nV, ns, v, iz, s, tau, ts, sp);
    const T ttop = (iz == 0) ? T(0) : tbot - tau;
    const T etop = exp(-ttop * a);
    const T lf = etop * (-expm1(-tau * a));
    const T w = (tau == T(0)) ? T(0) : ts / tau;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= ns) continue;
      const T P = (ts == T(0)) ? T(0) : sp[k] / ts;
      const long long o = o0 + (long long)nV * k + per * iz;
      d1w[o] = pre * P * lf;
      d1p[o] = pre * w * lf;
      d1t[o] = c0 * w * P * ebot - suf[k];
      suf[k] += c0 * w * P * lf;
    }
    tbot = ttop;
    ebot = etop;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// Device tables of one call: a packed_image in the library's scratch (vsm_internal.h) -- the C L layer pointers, then the small
// tables.  L, C and the number of geometries are not capped by it.
template <typename T>
static int xs_check(const char* who, int S, int L, int C, int nV, const T* const* tau_c_h, const T* I0, T mu0, const T* mu_v_h) {
  VSM_REQUIRE(S >= 0 && L >= 1 && C >= 1, "%s: S >= 0, L >= 1 and C >= 1 required (S = %d, L = %d, C = %d)", who, S, L, C);
  VSM_REQUIRE(nV >= 1 && nV <= 65535, "%s: 1 <= nV <= 65535 viewing geometries (got %d)", who, nV);
  VSM_REQUIRE(tau_c_h && I0 && mu_v_h, "%s: null argument", who);
  VSM_REQUIRE(mu0 > T(0), "%s: mu0 must be positive", who);
  for (int v = 0; v < nV; ++v) VSM_REQUIRE(mu_v_h[v] > T(0), "%s: mu_v[%d] must be positive", who, v);
  for (long long e = 0; e < (long long)C * L; ++e)
    VSM_REQUIRE(tau_c_h[e], "%s: null entry in the contributor table (contributor %lld, layer %lld)", who, e / L, e % L);
  return VSM_OK;
}
#define XS_GRID dim3((unsigned)((S + XS_TB - 1) / XS_TB), (unsigned)nV), dim3(XS_TB), 0, st

template <typename T>
static int xs_path1(int S, int L, int C, int nV, int ns, const T* const* tau_c_h, const T* varpi_c_h, const T* p_c_h, const T* I0, T mu0,
                    const T* mu_v_h, T* path1, void* stream) {
  int rc;
  if ((rc = xs_check<T>("exact_ss_path1", S, L, C, nV, tau_c_h, I0, mu0, mu_v_h))) return rc;
  VSM_REQUIRE(ns >= 1 && ns <= 4, "exact_ss_path1: n_stokes must be 1..4 (got %d)", ns);
  VSM_REQUIRE(varpi_c_h && p_c_h && path1, "exact_ss_path1: null argument");
  if (S == 0) return VSM_OK;
  hipStream_t st = as_stream(stream);
  packed_image img;
  const size_t o_t = img.add(tau_c_h, sizeof(T*) * (size_t)C * L), o_w = img.add(varpi_c_h, sizeof(T) * (size_t)C);
  const size_t o_p = img.add(p_c_h, sizeof(T) * (size_t)C * nV * ns), o_m = img.add(mu_v_h, sizeof(T) * (size_t)nV);
  unsigned char* d;
  if ((rc = upload_image(img, XS_SLOT, st, &d))) return rc;
  hipLaunchKernelGGL(k_xs_path1<T>, XS_GRID, S, L, C, nV, ns, (const T* const*)(d + o_t), (const T*)(d + o_w), (const T*)(d + o_p), I0,
                     mu0, (const T*)(d + o_m), path1);
  VSM_LAUNCH_CHECK("k_xs_path1");
  return VSM_OK;
}

template <typename T>
static int xs_path2(int S, int L, int C, int nV, int ns, const T* const* tau_c_h, const T* brdf, int spectral, const T* I0, T mu0,
                    const T* mu_v_h, T* path2, void* stream) {
  int rc;
  if ((rc = xs_check<T>("exact_ss_path2", S, L, C, nV, tau_c_h, I0, mu0, mu_v_h))) return rc;
  VSM_REQUIRE(ns >= 1 && ns <= 4, "exact_ss_path2: n_stokes must be 1..4 (got %d)", ns);
  VSM_REQUIRE(brdf && path2, "exact_ss_path2: null argument");
  if (S == 0) return VSM_OK;
  hipStream_t st = as_stream(stream);
  packed_image img;
  const size_t o_t = img.add(tau_c_h, sizeof(T*) * (size_t)C * L), o_m = img.add(mu_v_h, sizeof(T) * (size_t)nV);
  unsigned char* d;
  if ((rc = upload_image(img, XS_SLOT, st, &d))) return rc;
  hipLaunchKernelGGL(k_xs_path2<T>, XS_GRID, S, L, C, nV, ns, (const T* const*)(d + o_t), brdf, spectral != 0, I0, mu0,
                     (const T*)(d + o_m), path2);
  VSM_LAUNCH_CHECK("k_xs_path2");
  return VSM_OK;
}

template <typename T>
static int xs_path34(int S, int L, int C, int nV, int nQ, const T* const* tau_c_h, const T* varpi_c_h, const T* pbar3_c_h,
                     const T* pbar4_c_h, const T* mu_nodes_h, const T* w_h, const T* albedo, const T* I0, T mu0, const T* mu_v_h,
                     T* path3, T* path4, void* stream) {
  int rc;
  if ((rc = xs_check<T>("exact_ss_path34", S, L, C, nV, tau_c_h, I0, mu0, mu_v_h))) return rc;
  VSM_REQUIRE(nQ >= 1, "exact_ss_path34: nQ >= 1 inner nodes required (got %d)", nQ);
  VSM_REQUIRE(path3 || path4, "exact_ss_path34: both outputs are null");
  VSM_REQUIRE(varpi_c_h && mu_nodes_h && w_h && albedo && (!path3 || pbar3_c_h) && (!path4 || pbar4_c_h),
              "exact_ss_path34: null argument");
  for (int k = 0; k < nQ; ++k) VSM_REQUIRE(mu_nodes_h[k] > T(0), "exact_ss_path34: mu_nodes[%d] must be positive", k);
  if (S == 0) return VSM_OK;
  hipStream_t st = as_stream(stream);
  packed_image img;
  const size_t nb = sizeof(T) * (size_t)C * nV * nQ;
  const size_t o_t = img.add(tau_c_h, sizeof(T*) * (size_t)C * L), o_w = img.add(varpi_c_h, sizeof(T) * (size_t)C);
  const size_t o_3 = img.add(pbar3_c_h, path3 ? nb : 0), o_4 = img.add(pbar4_c_h, path4 ? nb : 0);
  const size_t o_n = img.add(mu_nodes_h, sizeof(T) * (size_t)nQ), o_q = img.add(w_h, sizeof(T) * (size_t)nQ);
  const size_t o_m = img.add(mu_v_h, sizeof(T) * (size_t)nV);
  unsigned char* d;
  if ((rc = upload_image(img, XS_SLOT, st, &d))) return rc;
  hipLaunchKernelGGL(k_xs_path34<T>, XS_GRID, S, L, C, nV, nQ, (const T* const*)(d + o_t), (const T*)(d + o_w), (const T*)(d + o_3),
                     (const T*)(d + o_4), (const T*)(d + o_n), (const T*)(d + o_q), albedo, I0, mu0, (const T*)(d + o_m), path3, path4);
  VSM_LAUNCH_CHECK("k_xs_path34");
  return VSM_OK;
}

template <typename T>
static int xs_jac12(int S, int L, int C, int nV, int ns, const T* const* tau_c_h, const T* varpi_c_h, const T* p_c_h, const T* brdf,
                    int spectral, const T* I0, T mu0, const T* mu_v_h, T* d1t, T* d1w, T* d1p, T* d2t, T* d2r, void* stream) {
  int rc;
  if ((rc = xs_check<T>("exact_ss_jac12", S, L, C, nV, tau_c_h, I0, mu0, mu_v_h))) return rc;
  VSM_REQUIRE(ns >= 1 && ns <= 4, "exact_ss_jac12: n_stokes must be 1..4 (got %d)", ns);
  VSM_REQUIRE(d1t || d2t, "exact_ss_jac12: no output requested");
  VSM_REQUIRE((d1t != nullptr) == (d1w != nullptr) && (d1t != nullptr) == (d1p != nullptr),
              "exact_ss_jac12: the three path-1 Jacobians go together");
  VSM_REQUIRE((d2t != nullptr) == (d2r != nullptr), "exact_ss_jac12: the two path-2 Jacobians go together");
  VSM_REQUIRE((!d1t || (varpi_c_h && p_c_h)) && (!d2t || brdf), "exact_ss_jac12: null argument");
  if (S == 0) return VSM_OK;
  hipStream_t st = as_stream(stream);
  packed_image img;
  const size_t o_t = img.add(tau_c_h, sizeof(T*) * (size_t)C * L), o_w = img.add(varpi_c_h, d1t ? sizeof(T) * (size_t)C : 0);
  const size_t o_p = img.add(p_c_h, d1t ? sizeof(T) * (size_t)C * nV * ns : 0), o_m = img.add(mu_v_h, sizeof(T) * (size_t)nV);
  unsigned char* d;
  if ((rc = upload_image(img, XS_SLOT, st, &d))) return rc;
  hipLaunchKernelGGL(k_xs_jac12<T>, XS_GRID, S, L, C, nV, ns, (const T* const*)(d + o_t), (const T*)(d + o_w), (const T*)(d + o_p), brdf,
                     spectral != 0, I0, mu0, (const T*)(d + o_m), d1t, d1w, d1p, d2t, d2r);
  VSM_LAUNCH_CHECK("k_xs_jac12");
  return VSM_OK;
}

}  // namespace vsm

using namespace vsm;

extern "C" {

#define VSM_XS_API(T, SFX)                                                                                                      \
  int vsm_exact_ss_path1_##SFX(int S, int L, int C, int nV, int n_stokes, const T* const* tau_c_h, const T* varpi_c_h,           \
                               const T* p_c_h, const T* I0, T mu0, const T* mu_v_h, T* path1, void* stream) {                    \
    return xs_path1<T>(S, L, C, nV, n_stokes, tau_c_h, varpi_c_h, p_c_h, I0, mu0, mu_v_h, path1, stream);                        \
  }                                                                                                                             \
  int vsm_exact_ss_path2_##SFX(int S, int L, int C, int nV, int n_stokes, const T* const* tau_c_h, const T* brdf,                \
                               int brdf_spectral, const T* I0, T mu0, const T* mu_v_h, T* path2, void* stream) {                 \
    return xs_path2<T>(S, L, C, nV, n_stokes, tau_c_h, brdf, brdf_spectral, I0, mu0, mu_v_h, path2, stream);                     \
  }                                                                                                                             \
  int vsm_exact_ss_path34_##SFX(int S, int L, int C, int nV, int nQ, const T* const* tau_c_h, const T* varpi_c_h,                \
                                const T* pbar3_c_h, const T* pbar4_c_h, const T* mu_nodes_h, const T* w_h, const T* albedo,      \
                                const T* I0, T mu0, const T* mu_v_h, T* path3, T* path4, void* stream) {                         \
    return xs_path34<T>(S, L, C, nV, nQ, tau_c_h, varpi_c_h, pbar3_c_h, pbar4_c_h, mu_nodes_h, w_h, albedo, I0, mu0, mu_v_h,     \
                        path3, path4, stream);                                                                                  \
  }                                                                                                                             \
  int vsm_exact_ss_jac12_##SFX(int S, int L, int C, int nV, int n_stokes, const T* const* tau_c_h, const T* varpi_c_h,           \
                               const T* p_c_h, const T* brdf, int brdf_spectral, const T* I0, T mu0, const T* mu_v_h,            \
                               T* d1_tau, T* d1_varpi, T* d1_P, T* d2_tau, T* d2_rho, void* stream) {                            \
    return xs_jac12<T>(S, L, C, nV, n_stokes, tau_c_h, varpi_c_h, p_c_h, brdf, brdf_spectral, I0, mu0, mu_v_h, d1_tau,           \
                       d1_varpi, d1_P, d2_tau, d2_rho, stream);                                                                  \
  }
VSM_XS_API(double, f64)
VSM_XS_API(float, f32)

}  // extern "C"
