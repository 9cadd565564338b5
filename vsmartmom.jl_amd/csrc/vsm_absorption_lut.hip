// Absorption.InterpolationModel: sigma(nu, p, T) lookup tables (src/Absorption/make_model_helpers.jl:55-122 and
// compute_absorption_cross_section.jl:181-233).  The interpolant is the reference's BSpline(Linear()) or
// BSpline(Cubic(Line(OnGrid()))) on three uniform axes; DESIGN 4.27 writes its definition out.
//
//   prefilter   values [nP nT, nNu] -> cubic B-spline coefficients [nP + 2, nT + 2, nNu + 2], FP64, one axis after the other:
//     k_lut_filter_nu    the long systems.  One lane per (row, chunk of VSM_LUT_CHUNK unknowns): the lane solves the tridiagonal
//                        system on its chunk widened by LUT_HALO nodes on each side, with c = y at the artificial ends (the true
//                        ends have c = y exactly: the natural end equation and its interior neighbour give c[1] = y[1]).  The error
//                        of an artificial end decays by 2 - sqrt(3) per node: below 2^-53 of it after 28 nodes.
//     k_lut_filter_axis  the short strided systems of the T and the p axis: one lane per system, lanes along nu (coalesced); the
//                        forward sweep keeps its right-hand sides in the output array.
//   evaluation  k_lut_eval<storage, cubic, lin>: one workgroup per (256 grid points, layer).  The (p, T) weights are the layer's;
//               the 16 (4 when linear) coefficient rows are collapsed with them once per table column the workgroup's points touch,
//               into LDS, and each point applies its nu taps to that row.  A workgroup whose points span more than VSM_LUT_SPAN
//               columns (a grid much coarser than the table, or a shuffled one) collapses the columns of each point directly
//               from memory instead.  Both paths run the same fma chain in the same order, and so does the linearized
//               instantiation: sigma has the same bits whichever produced it.
// No atomics, no library scratch, no host synchronisation; a call is bit-identical to its repetition.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "vsm_common.h"
#include "vsm_internal.h"

// every product and sum below is written out; fma() where one is meant
#pragma clang fp contract(off)

namespace vsm {

constexpr int LUT_CHUNK = VSM_LUT_CHUNK;   // unknowns a lane of k_lut_filter_nu owns
constexpr int LUT_HALO = 32;               // (2 - sqrt(3))^32 = 5e-19
constexpr int LUT_LANES = 64;              // lanes (= chunks) per workgroup of k_lut_filter_nu
constexpr int LUT_WINDOW = LUT_CHUNK + 2 * LUT_HALO;
constexpr int LUT_TILE = 256;              // grid points per workgroup of k_lut_eval
constexpr int LUT_SPAN = VSM_LUT_SPAN;     // table columns a workgroup collapses into LDS

// Thomas factors of tridiag(1, 4, 1): w[0] = 1 / 4, w[k] = 1 / (4 - w[k - 1]).  The distance to the fixed point 2 - sqrt(3)
// shrinks by (2 - sqrt(3))^2 = 0.072 per step: below half an ulp from k = 14; the table's last entry serves every k past it.
constexpr int LUT_WN = 24;
struct lut_w_table {
  double w[LUT_WN];
  constexpr lut_w_table() : w() {
    w[0] = 0.25;
    for (int k = 1; k < LUT_WN; ++k) w[k] = 1.0 / (4.0 - w[k - 1]);
  }
};
__device__ const lut_w_table LUT_W = lut_w_table();
__device__ __forceinline__ double lut_w(int k) { return LUT_W.w[k < LUT_WN ? k : LUT_WN - 1]; }

// in [rows, n] -> out [rows, n + 2].  blockIdx.x: row; blockIdx.y * LUT_LANES + lane: chunk.
__global__ __launch_bounds__(LUT_LANES) void k_lut_filter_nu(int n, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double scr[LUT_WINDOW + 1][LUT_LANES];   // the lane's window, lanes interleaved: no bank conflicts
  const int lane = threadIdx.x;
  const long long chunk = (long long)blockIdx.y * LUT_LANES + lane;
  if (chunk * LUT_CHUNK >= n) return;
  const double* y = in + (long long)blockIdx.x * n;   // y[q - 1] is the value at padded index q = 1 .. n
  double* c = out + (long long)blockIdx.x * (n + 2);
  const int s = 1 + (int)chunk * LUT_CHUNK, e = min(s + LUT_CHUNK, n + 1);   // this lane writes c[s .. e - 1]
  const int lo = max(1, s - LUT_HALO), hi = min(n, e - 1 + LUT_HALO), m = hi - lo;   // window: q = lo + j, j = 0 .. m
  scr[0][lane] = y[lo - 1];
  scr[m][lane] = y[hi - 1];
  double d = 0.0;
  for (int j = 1; j < m; ++j) {
    double r = 6.0 * y[lo + j - 1];
    if (j == 1) r -= scr[0][lane];
    if (j == m - 1) r -= scr[m][lane];
    d = (r - d) * lut_w(j - 1);
    scr[j][lane] = d;
  }
  double x = d;
  for (int j = m - 2; j >= 1; --j) {
    x = scr[j][lane] - lut_w(j - 1) * x;
    scr[j][lane] = x;
  }
  for (int q = s; q < e; ++q) c[q] = scr[q - lo][lane];
  if (s == 1) c[0] = 2.0 * scr[0][lane] - scr[1][lane];               // c[0] - 2 c[1] + c[2] = 0 (lo = 1 here)
  if (e == n + 1) c[n + 1] = 2.0 * scr[m][lane] - scr[m - 1][lane];   // hi = n here
}

// in [outer, n, inner] -> out [outer, n + 2, inner]: one lane per (outer, inner) system
__global__ __launch_bounds__(256) void k_lut_filter_axis(int n, long long inner, long long systems, const double* __restrict__ in,
                                                         double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= systems) return;
  const long long o = t / inner, x = t - o * inner;
  const double* y = in + o * n * inner + x;
  double* c = out + o * (n + 2) * inner + x;
  const double y1 = y[0], yn = y[(long long)(n - 1) * inner];
  c[inner] = y1;
  c[(long long)n * inner] = yn;
  double d = 0.0;
  for (int q = 2; q < n; ++q) {                 // unknowns c[2 .. n - 1]
    double r = 6.0 * y[(long long)(q - 1) * inner];
    if (q == 2) r -= y1;
    if (q == n - 1) r -= yn;
    d = (r - d) * lut_w(q - 2);
    c[(long long)q * inner] = d;
  }
  double v = d;
  for (int q = n - 2; q >= 2; --q) {
    v = c[(long long)q * inner] - lut_w(q - 2) * v;
    c[(long long)q * inner] = v;
  }
  c[0] = 2.0 * y1 - c[2 * inner];
  c[(long long)(n + 1) * inner] = 2.0 * yn - c[(long long)(n - 1) * inner];
}

__global__ __launch_bounds__(256) void k_lut_round(long long count, const double* __restrict__ in, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < count) out[t] = (float)in[t];
}

// Cell and weights of x on the axis (first, step, n).  The nodes are the FP64 numbers x_k = first + k step -- where the table's
// values were computed -- and cell i is [x_i, x_i+1) (the last one closed), clamped into the table whatever x is, with
// t = (x - x_i) / (x_i+1 - x_i): t is exactly 0 on a node, where (x - first) / step is off by the rounding of x_k itself (2e-10 of
// a cell at 6286 cm^-1 with a step of 0.002).  d: the derivative of the weights with respect to x, over the same cell width.
template <int CUBIC, int LIN>
__device__ __forceinline__ int lut_weights(double x, double first, double step, int n, double* w, double* d) {
  const double sgn = step > 0.0 ? 1.0 : -1.0;
  double fi = fmin(fmax(floor((x - first) / step), 0.0), (double)(n - 2));
  double x0 = first + fi * step;
  if (sgn * (x - x0) < 0.0 && fi > 0.0) {
    fi -= 1.0;
    x0 = first + fi * step;
  }
  double x1 = first + (fi + 1.0) * step;
  if (sgn * (x - x1) >= 0.0 && fi < (double)(n - 2)) {
    fi += 1.0;
    x0 = x1;
    x1 = first + (fi + 1.0) * step;
  }
  const double h = x1 - x0;
  const double t = (x - x0) / h;
  if (CUBIC) {
    // Horner forms of (1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3 (over 6) and of their derivatives; the factored
    // derivatives keep their relative accuracy where they vanish (t = 0 and t = 1, a layer on a node)
    const double t2 = t * t, s = 1.0 - t;   // (s is exact for t in [0, 1])
    w[0] = s * s * s / 6.0;
    w[1] = (t2 * (3.0 * t - 6.0) + 4.0) / 6.0;
    w[2] = (((3.0 - 3.0 * t) * t + 3.0) * t + 1.0) / 6.0;
    w[3] = t2 * t / 6.0;
    if (LIN) {
      d[0] = -0.5 * s * s / h;
      d[1] = t * (1.5 * t - 2.0) / h;
      d[2] = s * (1.5 * t + 0.5) / h;
      d[3] = 0.5 * t2 / h;
    }
  } else {
    w[0] = 1.0 - t;
    w[1] = t;
    if (LIN) {
      d[0] = -1.0 / h;
      d[1] = 1.0 / h;
    }
  }
  return (int)fi;
}

// one table column collapsed over the (p, T) taps: base points at coefficient (ip, iT, 0)
template <typename TS, int NT, int LIN>
__device__ __forceinline__ void lut_collapse(const TS* __restrict__ base, long long sP, long long sT, long long k, const double* wab,
                                             const double* wabT, const double* wabP, double& r, double& rT, double& rP) {
  r = 0.0;
  rT = 0.0;
  rP = 0.0;
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const double c = (double)base[a * sP + b * sT + k];
      r = fma(wab[a * NT + b], c, r);
      if (LIN) {
        rT = fma(wabT[a * NT + b], c, rT);
        rP = fma(wabP[a * NT + b], c, rP);
      }
    }
}

__device__ __forceinline__ int lut_wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

template <typename TS, int CUBIC, int LIN>
__global__ __launch_bounds__(LUT_TILE) void k_lut_eval(int nSpec, int nNu, int nP, int nT, double nu_first, double nu_step,
                                                       double p_first, double p_step, double T_first, double T_step,
                                                       const TS* __restrict__ coef, const double* __restrict__ grid,
                                                       const double* __restrict__ p, const double* __restrict__ T,
                                                       const double* __restrict__ scale, int accumulate, double* __restrict__ out,
                                                       double* __restrict__ out_dT, double* __restrict__ out_dp) {
  constexpr int NT = CUBIC ? 4 : 2, PAD = CUBIC ? 2 : 0, NL = LIN ? 3 : 1, RT = LIN ? 1 : 0, RP = LIN ? 2 : 0;
  __shared__ double rows[NL][LUT_SPAN];
  __shared__ int wlo[LUT_TILE / 64], whi[LUT_TILE / 64];
  const int z = blockIdx.y, tid = threadIdx.x;
  const int s = blockIdx.x * LUT_TILE + tid;
  const long long sT = nNu + PAD, sP = (long long)(nT + PAD) * sT;

  // the layer's (p, T) cell and the 16 (4) products of its weights
  double wp[NT], wt[NT], dp[NT], dt[NT];
  const int ip = lut_weights<CUBIC, LIN>(p[z], p_first, p_step, nP, wp, dp);
  const int it = lut_weights<CUBIC, LIN>(T[z], T_first, T_step, nT, wt, dt);
  double wab[NT * NT], wabT[LIN ? NT * NT : 1], wabP[LIN ? NT * NT : 1];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      wab[a * NT + b] = wp[a] * wt[b];
      if (LIN) {
        wabT[a * NT + b] = wp[a] * dt[b];
        wabP[a * NT + b] = dp[a] * wt[b];
      }
    }
  const TS* base = coef + ip * sP + it * sT;

  // the point's nu cell; outside [min, max] of the axis: exact 0
  const double nu_last = nu_first + (double)(nNu - 1) * nu_step;
  const double nu_lo = fmin(nu_first, nu_last), nu_hi = fmax(nu_first, nu_last);
  const double nu = s < nSpec ? grid[s] : 0.0;
  const bool inside = s < nSpec && nu >= nu_lo && nu <= nu_hi;
  double wn[NT], dn[NT];
  const int in = lut_weights<CUBIC, 0>(nu, nu_first, nu_step, nNu, wn, dn);

  // the columns this workgroup touches
  const int lo_w = lut_wave_min(inside ? in : INT_MAX), hi_w = -lut_wave_min(inside ? -in : INT_MAX);
  if ((tid & 63) == 0) {
    wlo[tid >> 6] = lo_w;
    whi[tid >> 6] = hi_w;
  }
  __syncthreads();
  int kmin = INT_MAX, kmax = -INT_MAX;
#pragma unroll
  for (int w = 0; w < LUT_TILE / 64; ++w) {
    kmin = min(kmin, wlo[w]);
    kmax = max(kmax, whi[w]);
  }
  if (kmax < kmin) {             // no point of this workgroup is inside the table
    if (s < nSpec && !accumulate) {
      const long long o = (long long)z * nSpec + s;
      out[o] = 0.0;
      if (LIN) {
        out_dT[o] = 0.0;
        out_dp[o] = 0.0;
      }
    }
    return;
  }
  const int span = kmax - kmin + NT;
  const bool staged = span <= LUT_SPAN;      // (uniform over the workgroup)
  if (staged) {
    for (int k = tid; k < span; k += LUT_TILE) {
      double r, rT, rP;
      lut_collapse<TS, NT, LIN>(base, sP, sT, (long long)kmin + k, wab, wabT, wabP, r, rT, rP);
      rows[0][k] = r;
      if (LIN) {
        rows[RT][k] = rT;
        rows[RP][k] = rP;
      }
    }
    __syncthreads();
  }
  if (s >= nSpec) return;
  const long long o = (long long)z * nSpec + s;
  if (!inside) {
    if (!accumulate) {
      out[o] = 0.0;
      if (LIN) {
        out_dT[o] = 0.0;
        out_dp[o] = 0.0;
      }
    }
    return;
  }
  double v = 0.0, vT = 0.0, vP = 0.0;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    double r, rT, rP;
    if (staged) {
      r = rows[0][in - kmin + j];
      rT = LIN ? rows[RT][in - kmin + j] : 0.0;
      rP = LIN ? rows[RP][in - kmin + j] : 0.0;
    } else {
      lut_collapse<TS, NT, LIN>(base, sP, sT, (long long)in + j, wab, wabT, wabP, r, rT, rP);
    }
    v = fma(wn[j], r, v);
    if (LIN) {
      vT = fma(wn[j], rT, vT);
      vP = fma(wn[j], rP, vP);
    }
  }
  const double sc = scale[z];
  out[o] = (accumulate ? out[o] : 0.0) + sc * v;
  if (LIN) {
    out_dT[o] = (accumulate ? out_dT[o] : 0.0) + sc * vT;
    out_dp[o] = (accumulate ? out_dp[o] : 0.0) + sc * vP;
  }
}

static size_t lut_elems(int nNu, int nP, int nT, int padP, int padT) {
  return (size_t)(nP + padP) * (size_t)(nT + padT) * (size_t)(nNu + 2);
}

template <int LIN>
static int lut_eval_entry(const char* fn, int nSpec, int Nz, int nNu, int nP, int nT, double nu_first, double nu_step, double p_first,
                          double p_step, double T_first, double T_step, int interp, int storage, const void* coef, const double* grid,
                          const double* p, const double* T, const double* scale, int accumulate, double* out, double* out_dT,
                          double* out_dp, void* stream) {
  VSM_REQUIRE(nSpec >= 1 && Nz >= 1, "%s: nSpec = %d, Nz = %d must be >= 1", fn, nSpec, Nz);
  VSM_REQUIRE(Nz <= 65535, "%s: Nz = %d above 65535 layers", fn, Nz);
  VSM_REQUIRE(nNu >= 2 && nP >= 2 && nT >= 2, "%s: a table axis needs two nodes (nNu = %d, nP = %d, nT = %d)", fn, nNu, nP, nT);
  VSM_REQUIRE(nNu <= INT_MAX - 2 && nP <= INT_MAX - 2 && nT <= INT_MAX - 2, "%s: an axis is too long", fn);
  VSM_REQUIRE(std::isfinite(nu_first) && std::isfinite(p_first) && std::isfinite(T_first) && std::isfinite(nu_step) &&
                  std::isfinite(p_step) && std::isfinite(T_step) && nu_step != 0.0 && p_step != 0.0 && T_step != 0.0,
              "%s: an axis needs a finite first node and a finite step != 0", fn);
  VSM_REQUIRE(interp == VSM_LUT_LINEAR || interp == VSM_LUT_CUBIC, "%s: interp = %d (0 linear, 1 cubic)", fn, interp);
  VSM_REQUIRE(storage == VSM_LUT_F64 || storage == VSM_LUT_F32, "%s: storage = %d (0 FP64, 1 FP32)", fn, storage);
  VSM_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate = %d (0 writes, 1 adds)", fn, accumulate);
  VSM_REQUIRE(coef && grid && p && T && scale && out && (!LIN || (out_dT && out_dp)), "%s: null pointer", fn);
  const dim3 g((unsigned)((nSpec + LUT_TILE - 1) / LUT_TILE), (unsigned)Nz), b(LUT_TILE);
  hipStream_t st = as_stream(stream);
#define LUT_LAUNCH(TS, CUBIC)                                                                                                     \
  hipLaunchKernelGGL((k_lut_eval<TS, CUBIC, LIN>), g, b, 0, st, nSpec, nNu, nP, nT, nu_first, nu_step, p_first, p_step, T_first, \
                     T_step, (const TS*)coef, grid, p, T, scale, accumulate, out, out_dT, out_dp)
  if (storage == VSM_LUT_F64) {
    if (interp == VSM_LUT_CUBIC)
      LUT_LAUNCH(double, 1);
    else
      LUT_LAUNCH(double, 0);
  } else {
    if (interp == VSM_LUT_CUBIC)
      LUT_LAUNCH(float, 1);
    else
      LUT_LAUNCH(float, 0);
  }
#undef LUT_LAUNCH
  VSM_LAUNCH_CHECK("k_lut_eval");
  return VSM_OK;
}

}  // namespace vsm

using namespace vsm;

extern "C" int vsm_absorption_lut_chunk(void) { return LUT_CHUNK; }

extern "C" int vsm_absorption_lut_span(void) { return LUT_SPAN; }

extern "C" size_t vsm_absorption_lut_work_elems(int nNu, int nP, int nT, int storage) {
  if (nNu < 2 || nP < 2 || nT < 2 || nNu > INT_MAX - 2 || nP > INT_MAX - 2 || nT > INT_MAX - 2 ||
      (storage != VSM_LUT_F64 && storage != VSM_LUT_F32))
    return 0;
  return lut_elems(nNu, nP, nT, 0, 0) + lut_elems(nNu, nP, nT, 0, 2) + (storage == VSM_LUT_F32 ? lut_elems(nNu, nP, nT, 2, 2) : 0);
}

extern "C" int vsm_absorption_lut_prefilter(int nNu, int nP, int nT, const double* values, int storage, void* coef, double* work,
                                            void* stream) {
  const char* fn = "vsm_absorption_lut_prefilter";
  VSM_REQUIRE(nNu >= 2 && nP >= 2 && nT >= 2, "%s: a table axis needs two nodes (nNu = %d, nP = %d, nT = %d)", fn, nNu, nP, nT);
  VSM_REQUIRE(nNu <= INT_MAX - 2 && nP <= INT_MAX - 2 && nT <= INT_MAX - 2, "%s: an axis is too long", fn);
  VSM_REQUIRE(storage == VSM_LUT_F64 || storage == VSM_LUT_F32, "%s: storage = %d (0 FP64, 1 FP32)", fn, storage);
  VSM_REQUIRE(values && coef && work, "%s: null pointer", fn);
  const long long rows = (long long)nP * nT, Lnu = (long long)nNu + 2;
  const long long chunks = ((long long)nNu + LUT_CHUNK - 1) / LUT_CHUNK, groups = (chunks + LUT_LANES - 1) / LUT_LANES;
  const long long sysT = (long long)nP * Lnu, sysP = (long long)(nT + 2) * Lnu, total = (long long)lut_elems(nNu, nP, nT, 2, 2);
  VSM_REQUIRE(rows <= 0x7fffffffLL && groups <= 65535 && (sysT + 255) / 256 <= 0x7fffffffLL && (sysP + 255) / 256 <= 0x7fffffffLL &&
                  (total + 255) / 256 <= 0x7fffffffLL,
              "%s: nNu = %d, nP = %d, nT = %d above the launch limits", fn, nNu, nP, nT);
  hipStream_t st = as_stream(stream);
  double* A = work;                                        // [nP, nT, nNu + 2]
  double* B = A + lut_elems(nNu, nP, nT, 0, 0);             // [nP, nT + 2, nNu + 2]
  double* F = storage == VSM_LUT_F64 ? (double*)coef : B + lut_elems(nNu, nP, nT, 0, 2);   // [nP + 2, nT + 2, nNu + 2]
  hipLaunchKernelGGL(k_lut_filter_nu, dim3((unsigned)rows, (unsigned)groups), dim3(LUT_LANES), 0, st, nNu, values, A);
  VSM_LAUNCH_CHECK("k_lut_filter_nu");
  hipLaunchKernelGGL(k_lut_filter_axis, dim3((unsigned)((sysT + 255) / 256)), dim3(256), 0, st, nT, Lnu, sysT, (const double*)A, B);
  VSM_LAUNCH_CHECK("k_lut_filter_axis");
  hipLaunchKernelGGL(k_lut_filter_axis, dim3((unsigned)((sysP + 255) / 256)), dim3(256), 0, st, nP, sysP, sysP, (const double*)B, F);
  VSM_LAUNCH_CHECK("k_lut_filter_axis");
  if (storage == VSM_LUT_F32) {
    hipLaunchKernelGGL(k_lut_round, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, (const double*)F, (float*)coef);
    VSM_LAUNCH_CHECK("k_lut_round");
  }
  return VSM_OK;
}

extern "C" int vsm_absorption_lut_eval(int nSpec, int Nz, int nNu, int nP, int nT, double nu_first, double nu_step, double p_first,
                                       double p_step, double T_first, double T_step, int interp, int storage, const void* coef,
                                       const double* grid, const double* p, const double* T, const double* scale, int accumulate,
                                       double* out, void* stream) {
  return lut_eval_entry<0>("vsm_absorption_lut_eval", nSpec, Nz, nNu, nP, nT, nu_first, nu_step, p_first, p_step, T_first, T_step,
                           interp, storage, coef, grid, p, T, scale, accumulate, out, nullptr, nullptr, stream);
}

extern "C" int vsm_absorption_lut_eval_lin(int nSpec, int Nz, int nNu, int nP, int nT, double nu_first, double nu_step,
                                           double p_first, double p_step, double T_first, double T_step, int interp, int storage,
                                           const void* coef, const double* grid, const double* p, const double* T,
                                           const double* scale, int accumulate, double* out, double* out_dT, double* out_dp,
                                           void* stream) {
  return lut_eval_entry<1>("vsm_absorption_lut_eval_lin", nSpec, Nz, nNu, nP, nT, nu_first, nu_step, p_first, p_step, T_first,
                           T_step, interp, storage, coef, grid, p, T, scale, accumulate, out, out_dT, out_dp, stream);
}
