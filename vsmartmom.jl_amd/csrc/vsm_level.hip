// Level equation of the multi-sensor run (vsm_level_radiance_*): the radiance field at an interior boundary of the column from the
// composite above it (top) and the composite below it (bottom).  Restates interlayer_flux_helper! (CoreKernel/interlayer_flux.jl:
// 1-19; called through compute_interlayer_flux!, :185-201, by postprocessing_vza_ms!, tools/postprocessing_vza_ms.jl:7-52):
//
//   dw = (I - A B)^-1 (a + A c),   uw = (I - B A)^-1 (c + B a),   A = top R+-, a = top J0+, B = bottom R-+, c = bottom J0-
//
// The reference forms two inverses and four products.  Here uw comes from dw by the push-through identity
// (I - B A)^-1 (c + B a) = c + B (I - A B)^-1 (a + A c) = c + B dw, and dw from ONE pivoted Gauss-Jordan elimination of [M | d].
// Every fused kernel is the same solve body (level_solve_columns) for K right-hand sides at once:
//   1. [M | d_k] = [I - A B | a_k + A c_k] in one MFMA product (the c_k ride as the spare columns of B), written to LDS;
//   2. Gauss-Jordan on [M | d_k] in LDS, the pivot rule of vsm_inverse.h (largest |m_ik|, first occurrence) -- no inverse;
//   3. dw_k = d_k / m_ii,  uw_k = c_k + B dw_k (mat-vec);
// what differs is where the right-hand sides come from and what is done with the vectors.  One spectral point per 256-thread
// workgroup, N <= 128 (FP64 [M | d]: 129 KiB of LDS at N = 128).  Seven fused kernels:
//   k_level_radiance_src   vsm_level_radiance_* (K = 1) and vsm_level_radiance_src_* (up to VSM_LEVEL_MAX_SRC source pairs (a_k,
//                          c_k) on the same A, B: the solar and the thermal slot): the level vectors summed over the sources,
//                          their VZA rows added into the caller's [nV, n_stokes, S] outputs;
//   k_level_flux           vsm_level_flux_*: the level vectors of the same sources reduced in LDS to hemispheric quadratures (the
//                          fluxes of rt_run_fluxes), and the TOA itself, which has no system;
//   k_level_radiance_ie    vsm_level_radiance_ie_*: the first-order (Raman) part of the same equation, interlayer_flux_helper!(::RRS)
//                          (interlayer_flux.jl:21-77), per recipient point with the lines summed before ONE solve of [I - A B | r];
//   k_level_flux_ie        vsm_level_flux_ie_*: the same solve (level_ie_solve), its vectors and the point's own elastic ones
//                          reduced to the hemispheric quadratures (the fluxes of CoreRTRaman.rt_run_fluxes), and the TOA;
//   k_level_radiance_lin_src   vsm_level_radiance_lin_* (P_src = 0) and vsm_level_radiance_lin_src_*: the derivative with respect
//                          to the Jacobian parameters, the parameters as right-hand sides of ONE solve per chunk, and P_src
//                          further SOURCE-ONLY slots (the Planck slots of a linearized run with thermal emission); level_lin_body;
//   k_level_flux_lin       vsm_level_flux_lin_*: the same derivative vectors reduced to the quadratures, one per slot (the flux
//                          Jacobians of CoreRTLin.rt_run_fluxes); level_lin_body's other epilogue;
//   k_emission_response    vsm_surface_emission_response_*: the system between the atmosphere and the surface layer for the unit
//                          emission patterns of SurfaceSIF, kept per component.
// Larger N (vsm_level_radiance_* alone): the operator-level twin (batched products + vsm_batch_inv + products +
// vsm_postprocess_vza), the same contract.
#include "vsm_common.h"
#include "vsm_internal.h"
#include "vsm_inverse.h"

namespace vsm {

constexpr int LEVEL_FUSED_MAX_N = 128;
constexpr int LEVEL_NT = 256;

struct level_pp {
  int row0[64];
  double w[256];
};

// The two halves of every fused level kernel, on [M | r_1 .. r_{NC-N}] in L (row-major, leading dimension LD >= NC).  The whole
// workgroup enters both; sh: 2 ints of LDS (pivot row, non-finite flag).

// [M | r] = [I | s] - [A B | -A q]: 16 x 16 output tiles over the N x NC block, round-robin over the four waves, ONE MFMA product
// (the q ride as the spare columns N .. NC-1 of B).  Before the barrier that precedes the call: the q in Q [NC - N][N], the s in
// columns N .. NC-1 of L, sh[1] = 0.
template <typename T>
__device__ __forceinline__ void level_form_system(int N, int NC, int LD, const T* As, const T* Bs, const T* Q, T* L, int* sh,
                                                  int* status) {
  int& s_flag = sh[1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
  const int MT = (N + 15) / 16, CT = (NC + 15) / 16;
  bool bad = false;
  for (int t = wave; t < MT * CT; t += LEVEL_NT / 64) {
    const int ti = t / CT, tj = t % CT;
    const int row = 16 * ti + li, col = 16 * tj + li;
    typename mfma<T>::acc_t acc = acc_zero<T>();
    for (int k0 = 0; k0 < N; k0 += 4) {
      const int k = k0 + kq;
      const T av = (row < N && k < N) ? As[(long long)k * N + row] : T(0);
      const T bv = (k < N) ? (col < N ? Bs[(long long)col * N + k] : (col < NC ? Q[(col - N) * N + k] : T(0))) : T(0);
      acc = mfma<T>::mma(av, bv, acc);
    }
    const int ocol = 16 * tj + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = 16 * ti + mfma<T>::crow(lane, r);
      if (orow < N && ocol < NC) {
        const T v = ocol < N ? ((orow == ocol ? T(1) : T(0)) - acc[r]) : L[orow * LD + ocol] + acc[r];
        bad |= !isfinite(v);
        L[orow * LD + ocol] = v;
      }
    }
  }
  if (bad) s_flag = 1;
  __syncthreads();
  if (s_flag && tid == 0) atomicOr(&status[0], (int)VSM_DEVSTAT_NONFINITE);
}

// Gauss-Jordan elimination of [M | r] over NC columns, the pivot rule of vsm_inverse.h (largest |m_ik|, first occurrence): row k
// is the pivot row of step k and is not normalised; the solutions are r_i / m_ii afterwards.
template <typename T>
__device__ __forceinline__ void level_eliminate(int N, int NC, int LD, T* L, int* sh, int* status) {
  int& s_piv = sh[0];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tj = tid & 63, ti = tid >> 6;
  for (int k = 0; k < N; ++k) {
    if (wave == 0) {
      const bool in0 = lane >= k && lane < N, in1 = lane + 64 >= k && lane + 64 < N;
      const T v0 = in0 ? fabs(L[lane * LD + k]) : T(-1);
      const T v1 = in1 ? fabs(L[(lane + 64) * LD + k]) : T(-1);
      const T best = wave_max(v0 > v1 ? v0 : v1);
      const unsigned long long m0 = __ballot(in0 && v0 == best), m1 = __ballot(in1 && v1 == best);
      const int p = m0 ? (__ffsll((long long)m0) - 1) : (m1 ? 64 + __ffsll((long long)m1) - 1 : k);
      if (lane == 0) s_piv = p;
    }
    __syncthreads();
    const int p = s_piv;
    if (p != k) {
      for (int j = k + tid; j < NC; j += LEVEL_NT) {
        const T tmp = L[k * LD + j];
        L[k * LD + j] = L[p * LD + j];
        L[p * LD + j] = tmp;
      }
      __syncthreads();
    }
    const T pv = L[k * LD + k];
    if (pv == T(0) && tid == 0) atomicOr(&status[0], (int)VSM_DEVSTAT_SINGULAR);
    const T inv = T(1) / pv;
    for (int i = ti; i < N; i += LEVEL_NT / 64) {
      if (i == k) continue;
      const T f = L[i * LD + k] * inv;
      for (int j = k + 1 + tj; j < NC; j += 64) L[i * LD + j] -= f * L[k * LD + j];
    }
    __syncthreads();
  }
}

// The solve body of every fused level kernel, for K right-hand sides (LD >= N + K).  Before the barrier that precedes the call:
// the right-hand sides s_k in columns N .. N + K - 1 of L, the q_k in Q [K][N], sh[1] = 0.  After it, behind a barrier:
//   dw_k = (I - A B)^-1 (s_k + A q_k) in column N + k of L,   uw_k = q_k + B dw_k in Q[k].
template <typename T>
__device__ __forceinline__ void level_solve_columns(int N, int K, int LD, const T* As, const T* Bs, T* L, T* Q, int* sh, int* status) {
  const int tid = threadIdx.x;
  level_form_system<T>(N, N + K, LD, As, Bs, Q, L, sh, status);
  level_eliminate<T>(N, N + K, LD, L, sh, status);
  // dw_k = column / m_ii (in place: each element is read and written by its own thread)
  for (int e = tid; e < N * K; e += LEVEL_NT) {
    const int i = e % N, k = e / N;
    L[i * LD + N + k] = L[i * LD + N + k] / L[i * LD + i];
  }
  __syncthreads();
  for (int e = tid; e < N * K; e += LEVEL_NT) {
    const int i = e % N, k = e / N;
    T y = Q[k * N + i];
    for (int j = 0; j < N; ++j) y += Bs[(long long)j * N + i] * L[j * LD + N + k];
    Q[k * N + i] = y;   // (row i of Q[k] is read by this thread alone until the barrier)
  }
  __syncthreads();
}

// The sum over the K sources, in place: column N of L = dw_1 + dw_2 + .. and Q[0] = uw_1 + uw_2 + .., added in that order (each
// row by its own thread), then a barrier.  K = 1: nothing to do.
template <typename T>
__device__ __forceinline__ void level_sum_columns(int N, int K, int LD, T* L, T* Q) {
  if (K == 1) return;
  for (int i = threadIdx.x; i < N; i += LEVEL_NT) {
    T x = L[i * LD + N], y = Q[i];
    for (int k = 1; k < K; ++k) {
      x += L[i * LD + N + k];
      y += Q[k * N + i];
    }
    L[i * LD + N] = x;
    Q[i] = y;
  }
  __syncthreads();
}

// The epilogue of the radiance kernels for ONE vector pair, dw in column N of L and uw in Q[0]: dw_full / uw_full [N,1,S]
// (nullable) and the VZA rows accumulated into uw / dw [nV, n_stokes, S].
template <typename T>
__device__ __forceinline__ void level_radiance_out(int N, int ns, int LD, int nV, const level_pp& pa, long long s, const T* L,
                                                   const T* Q, T* uw, T* dw, T* dw_full, T* uw_full) {
  const int tid = threadIdx.x;
  if (dw_full || uw_full) {
    for (int i = tid; i < N; i += LEVEL_NT) {
      if (dw_full) dw_full[s * N + i] = L[i * LD + N];
      if (uw_full) uw_full[s * N + i] = Q[i];
    }
  }
  for (int e = tid; e < nV * ns; e += LEVEL_NT) {
    const int v = e % nV, c = e / nV, row = pa.row0[v] + c;
    const T w = (T)pa.w[v + nV * c];
    const long long dst = (s * ns + c) * nV + v;
    uw[dst] += w * Q[row];
    dw[dst] += w * L[row * LD + N];
  }
}

// The level equation for K = n_src source pairs (a_k, c_k) on the SAME operators (vsm_level_radiance_src_*: the solar and the
// thermal slot of a multi-sensor run), point s = blockIdx.x:
//   level_solve_columns on [M | d_1 .. d_K] = [I - A B | a_k + A c_k],  then the SUM over k (level_sum_columns) and
//   level_radiance_out of that one vector pair.
// K = 1 is vsm_level_radiance_* itself (N <= 128): one right-hand side, nothing to sum.  LDS: L [N][N + K], Q [K][N].
template <typename T>
struct level_srcs {
  const T* a[VSM_LEVEL_MAX_SRC];
  const T* c[VSM_LEVEL_MAX_SRC];
};

template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_radiance_src(int N, int ns, int K, int nV, level_pp pa, const T* __restrict__ A,
                                                                 level_srcs<T> src, const T* __restrict__ B, long long bstride,
                                                                 T* uw, T* dw, T* dw_full, T* uw_full, int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + K;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | d_1 .. d_K], row-major, leading dimension N + K
  T* Q = L + (size_t)N * LD;                     // c_k, then uw_k
  __shared__ int sh[2];
  const int tid = threadIdx.x;
  const long long s = blockIdx.x;
  const T* Bs = B + s * bstride;
  if (tid == 0) sh[1] = 0;
#pragma unroll
  for (int k = 0; k < VSM_LEVEL_MAX_SRC; ++k) {
    if (k < K) {
      for (int i = tid; i < N; i += LEVEL_NT) {
        L[i * LD + N + k] = src.a[k][s * N + i];
        Q[k * N + i] = src.c[k][s * N + i];
      }
    }
  }
  __syncthreads();
  level_solve_columns<T>(N, K, LD, A + s * (long long)N * N, Bs, L, Q, sh, status);
  level_sum_columns<T>(N, K, LD, L, Q);
  level_radiance_out<T>(N, ns, LD, nV, pa, s, L, Q, uw, dw, dw_full, uw_full);
}

// The hemispheric quadratures of n_vec vector pairs in LDS (level_lin_body; k_level_flux has the same reduction with the sum
// over its sources inside it): wave e % 4 takes item e = (v, r, d) and writes, for weight row r < nW (q: DEVICE [nW][N / ns], one weight per stream) and direction d,
//   out[d][r][slot0 + v][s] = sum_i q[r][i] vec_d[v][i ns]      (d = 0: up[v up_vs + row up_is], d = 1: dn likewise; !has_dn: 0)
// the rows of Stokes I.  A lane adds its stream i = lane, then lane + 64, then a butterfly over the wave: the order of the
// additions depends on N and ns alone.
template <typename T>
__device__ __forceinline__ void level_flux_reduce(int Nq, int ns, int nW, int n_vec, const T* __restrict__ q, const T* up, int up_vs,
                                                  int up_is, const T* dn, int dn_vs, int dn_is, bool has_dn, T* out, int slot0,
                                                  int slots, long long S, long long s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int e = wave; e < 2 * nW * n_vec; e += LEVEL_NT / 64) {
    const int d = e & 1, r = (e >> 1) % nW, v = e / (2 * nW);
    T acc = T(0);
    if (d == 0 || has_dn) {
      for (int i = lane; i < Nq; i += 64) {
        const int row = i * ns;
        const T x = d ? dn[v * dn_vs + row * dn_is] : up[v * up_vs + row * up_is];
        acc += q[r * Nq + i] * x;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) out[(((long long)d * nW + r) * slots + slot0 + v) * S + s] = acc;
  }
}

// Hemispheric quadratures of the level vectors (vsm_level_flux_*: the up, down and actinic fluxes of rt_run_fluxes), point
// s = blockIdx.x.  k_level_radiance_src's system for the K source pairs (level_solve_columns); A == nullptr: no layer above the
// level (the TOA), no system: dw = 0, uw_k = c_k.  The vectors stay in LDS; for each weight row r < nW (q: DEVICE [nW][N / ns], one
// weight per stream) and direction d, wave (2 r + d) % 4 takes
//   out[d][r][s] = sum_i q[r][i] * sum_k v_k[i ns]      (v = uw for d = 0, dw for d = 1: the rows of Stokes I)
// lanes over i (a lane adds its stream i = lane, then lane + 64), then a butterfly over the wave: the order of the additions
// depends on N, K and nW alone.  The sum over k stays inside this reduction and is not level_sum_columns + level_flux_reduce:
// that form gives the same bits but was measured 2.7 % slower per call.  out[2][r][s] = dir[r] F0_I[s]
// exp(-tau_sum[s] / mu0) with both arrays given, else 0.  Every element of out [3][nW][S] is WRITTEN.  LDS: L [N][N + K], Q [K][N].
template <typename T>
struct level_flux_dir {
  T h[4];
  T mu0;
};

template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_flux(int N, int ns, int K, int nW, long long S, const T* __restrict__ A,
                                                         level_srcs<T> src, const T* __restrict__ B, long long bstride,
                                                         const T* __restrict__ q, level_flux_dir<T> dir,
                                                         const T* __restrict__ tau_sum, const T* __restrict__ F0_I, T* out,
                                                         int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + K;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | d_1 .. d_K], row-major, leading dimension N + K
  T* Q = L + (size_t)N * LD;                     // c_k, then uw_k
  __shared__ int sh[2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long s = blockIdx.x;
  if (tid == 0) sh[1] = 0;
#pragma unroll
  for (int k = 0; k < VSM_LEVEL_MAX_SRC; ++k) {
    if (k < K) {
      for (int i = tid; i < N; i += LEVEL_NT) {
        if (A) L[i * LD + N + k] = src.a[k][s * N + i];
        Q[k * N + i] = src.c[k][s * N + i];
      }
    }
  }
  __syncthreads();
  if (A)   // (the same for the whole grid)
    level_solve_columns<T>(N, K, LD, A + s * (long long)N * N, B + s * bstride, L, Q, sh, status);
  const int Nq = N / ns;
  for (int p = wave; p < 2 * nW; p += LEVEL_NT / 64) {
    const int r = p >> 1, d = p & 1;
    T acc = T(0);
    if (d == 0 || A) {
      for (int i = lane; i < Nq; i += 64) {
        const int row = i * ns;
        T v = d ? L[row * LD + N] : Q[row];
        for (int k = 1; k < K; ++k) v += d ? L[row * LD + N + k] : Q[k * N + row];
        acc += q[r * Nq + i] * v;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) out[((long long)d * nW + r) * S + s] = acc;
  }
  if (tid < nW) out[((long long)2 * nW + tid) * S + s] = tau_sum ? dir.h[tid] * F0_I[s] * exp(-tau_sum[s] / dir.mu0) : T(0);
}

// The column-group streaming of the inelastic and the linearized kernel.  Thread (g, i) = (tid / N, tid % N) of the G = 256 / N
// column groups takes row i of columns j = g, g + G, ... of a block [M | v] (column N = the vector, taken by the group next in
// turn), so the workgroup reads G consecutive columns, G N contiguous elements, per step.  level_stream_pair adds [M1 | v1] x1 to
// s1 and [M2 | v2] x2 to s2 (M2 == nullptr: no second block); level_stream_reduce adds the per-group partial sums in group order
// (part: [2][G][N] of LDS) and writes row i of the two sums to d1[i ld1] and d2[i ld2].  The whole workgroup enters the reduction.
template <typename T>
struct level_sums {
  T s1, s2;
};

template <typename T>
__device__ __forceinline__ level_sums<T> level_stream_pair(int N, int G, int g, int i, const T* M1, const T* v1, const T* x1,
                                                           const T* M2, const T* v2, const T* x2, level_sums<T> acc) {
  for (int j = g; j < N; j += G) {
    acc.s1 += M1[(long long)j * N + i] * x1[j];
    if (M2) acc.s2 += M2[(long long)j * N + i] * x2[j];
  }
  if (g == (N % G)) {
    acc.s1 += v1[i];
    if (M2) acc.s2 += v2[i];
  }
  return acc;
}

template <typename T>
__device__ __forceinline__ void level_stream_reduce(int N, int G, int g, int i, level_sums<T> acc, T* part, T* d1, int ld1, T* d2,
                                                    int ld2) {
  const int tid = threadIdx.x;
  if (g < G) {
    part[g * N + i] = acc.s1;
    part[(G + g) * N + i] = acc.s2;
  }
  __syncthreads();
  if (tid < N) {
    T t1 = T(0), t2 = T(0);
    for (int h = 0; h < G; ++h) {
      t1 += part[h * N + tid];
      t2 += part[(G + h) * N + tid];
    }
    d1[tid * ld1] = t1;
    d2[tid * ld2] = t2;
  }
  __syncthreads();
}

// The solve of the two inelastic kernels for recipient point n1, lines summed before it:
//   q = sum_k [c_ie,k + B_ie,k dw(n0)],  r = sum_k [a_ie,k + A_ie,k uw(n0)] + A q,  dw_ie = (I - A B)^-1 r,  uw_ie = q + B dw_ie
// over the in-band lines k (n0 = n1 + shift[k] in 0..S-1); dw / uw are the ELASTIC level vectors of the donors.
// Phase 1 streams the 2K ie blocks of the point by column groups; phase 2 is level_solve_columns with ONE right-hand side,
// (s, q) = (r - A q, q).  After it, behind a barrier: dw_ie in column N of L [N][N + 1], uw_ie in qs [N].  part: [2][G][N].
template <typename T>
__device__ __forceinline__ void level_ie_solve(int N, int S, int K, const int* __restrict__ shift, int n1, const T* __restrict__ A,
                                               const T* __restrict__ B, long long bstride, const T* __restrict__ dwf,
                                               const T* __restrict__ uwf, const T* __restrict__ Aie, const T* __restrict__ aie,
                                               const T* __restrict__ Bie, const T* __restrict__ cie, T* L, T* qs, T* part, int* sh,
                                               int* status) {
  const int LD = N + 1;
  const int tid = threadIdx.x;
  const long long NN = (long long)N * N;
  const int G = LEVEL_NT / N, g = tid / N, i = tid - g * N;
  level_sums<T> acc = {T(0), T(0)};
  if (tid == 0) sh[1] = 0;
  if (g < G) {
    for (int k = 0; k < K; ++k) {
      const int n0 = n1 + shift[k];
      if (n0 < 0 || n0 >= S) continue;
      const long long blk = (long long)k * S + n1;
      acc = level_stream_pair<T>(N, G, g, i, Aie + blk * NN, aie + blk * N, uwf + (long long)n0 * N, Bie ? Bie + blk * NN : nullptr,
                                 cie ? cie + blk * N : nullptr, dwf + (long long)n0 * N, acc);
    }
  }
  level_stream_reduce<T>(N, G, g, i, acc, part, L + N, LD, qs, 1);
  level_solve_columns<T>(N, 1, LD, A + n1 * NN, B + n1 * bstride, L, qs, sh, status);
}

// The inelastic level equation (vsm_level_radiance_ie_*) of recipient point n1 = blockIdx.x: level_ie_solve, then
// level_radiance_out of its vector pair.  LDS: L [N][N + 1], q [N], partial sums [2][G][N].
template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_radiance_ie(int N, int ns, int S, int K, const int* __restrict__ shift, int nV,
                                                                level_pp pa, const T* __restrict__ A,
                                                                const T* __restrict__ B, long long bstride,
                                                                const T* __restrict__ dwf, const T* __restrict__ uwf,
                                                                const T* __restrict__ Aie, const T* __restrict__ aie,
                                                                const T* __restrict__ Bie, const T* __restrict__ cie, T* uwie,
                                                                T* dwie, T* dwie_full, T* uwie_full, int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + 1;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | r], row-major, leading dimension N + 1; column N: then dw_ie
  T* qs = L + (size_t)N * LD;                    // q, then uw_ie
  T* part = qs + N;                              // [2][G][N] partial sums
  __shared__ int sh[2];
  const int n1 = blockIdx.x;
  level_ie_solve<T>(N, S, K, shift, n1, A, B, bstride, dwf, uwf, Aie, aie, Bie, cie, L, qs, part, sh, status);
  level_radiance_out<T>(N, ns, LD, nV, pa, n1, L, qs, uwie, dwie, dwie_full, uwie_full);
}

// Hemispheric quadratures of the elastic AND the inelastic level vectors (vsm_level_flux_ie_*: the fluxes of
// CoreRTRaman.rt_run_fluxes) of recipient point n1 = blockIdx.x.  level_ie_solve leaves dw_ie / uw_ie in LDS; the point's own
// elastic vectors dwf[n1] / uwf[n1] are read from global memory; level_flux_reduce (one vector pair each) writes
//   out[0][r][n1] = sum_i q[r][i] uw[i ns]   out[1] likewise of dw   out[3] of uw_ie   out[4] of dw_ie   (the rows of Stokes I)
//   out[2][r][n1] = dir[r] F0_I[n1] exp(-tau_sum[n1] / mu0) with both arrays given, else 0.
// A == nullptr (the same for the whole grid): no layer above the level (the TOA), no system: dw = dw_ie = 0, uw = uwf[n1],
// uw_ie = sum over the in-band k of c_ie,k, added in the order of k (cie == nullptr: 0); dwf, B, Aie, aie, Bie are not read.
// Every element of out [5][nW][S] is WRITTEN.  LDS: that of k_level_radiance_ie.
template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_flux_ie(int N, int ns, int S, int K, const int* __restrict__ shift, int nW,
                                                            const T* __restrict__ A, const T* __restrict__ B, long long bstride,
                                                            const T* __restrict__ dwf, const T* __restrict__ uwf,
                                                            const T* __restrict__ Aie, const T* __restrict__ aie,
                                                            const T* __restrict__ Bie, const T* __restrict__ cie,
                                                            const T* __restrict__ q, level_flux_dir<T> dir,
                                                            const T* __restrict__ tau_sum, const T* __restrict__ F0_I, T* out,
                                                            int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + 1;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | r], row-major, leading dimension N + 1; column N: then dw_ie
  T* qs = L + (size_t)N * LD;                    // q, then uw_ie
  T* part = qs + N;                              // [2][G][N] partial sums
  __shared__ int sh[2];
  const int tid = threadIdx.x;
  const int n1 = blockIdx.x;
  if (A) {
    level_ie_solve<T>(N, S, K, shift, n1, A, B, bstride, dwf, uwf, Aie, aie, Bie, cie, L, qs, part, sh, status);
  } else {
    if (tid < N) {
      T y = T(0);
      if (cie) {
        for (int k = 0; k < K; ++k) {
          const int n0 = n1 + shift[k];
          if (n0 >= 0 && n0 < S) y += cie[((long long)k * S + n1) * N + tid];
        }
      }
      qs[tid] = y;
    }
    __syncthreads();
  }
  const int Nq = N / ns;
  const T* own = uwf + (long long)n1 * N;
  level_flux_reduce<T>(Nq, ns, nW, 1, q, own, 0, 1, A ? dwf + (long long)n1 * N : own, 0, 1, A != nullptr, out, 0, 1, (long long)S,
                       (long long)n1);
  level_flux_reduce<T>(Nq, ns, nW, 1, q, qs, 0, 1, L + N, 0, LD, A != nullptr, out + 3 * (long long)nW * S, 0, 1, (long long)S,
                       (long long)n1);
  if (tid < nW) out[((long long)2 * nW + tid) * S + n1] = tau_sum ? dir.h[tid] * F0_I[n1] * exp(-tau_sum[n1] / dir.mu0) : T(0);
}

// The VZA table of one launch and what to do above the 64 viewing angles it carries: the level vectors in full (the caller's
// buffers, or scratch for full_elems each), a launch with nV = 0, then the VZA rows by post(uw_full, dw_full).
// launch(nV, pa, dw_full, uw_full) launches the kernel and returns its launch status.
template <typename T, typename Launch, typename Post>
static int level_launch(int ns, int nV, const int* row0_h, const T* w_h, size_t full_elems, T* dw_full, T* uw_full, hipStream_t st,
                        Launch launch, Post post) {
  level_pp pa = {};
  if (nV <= 64) {
    for (int v = 0; v < nV; ++v) pa.row0[v] = row0_h[v];
    for (int k = 0; k < ns; ++k)
      for (int v = 0; v < nV; ++v) pa.w[v + nV * k] = (double)w_h[v + nV * k];
    return launch(nV, pa, dw_full, uw_full);
  }
  if (!dw_full || !uw_full) {
    T* full = static_cast<T*>(scratch(2 * full_elems * sizeof(T), 0, st));
    if (!full) return VSM_ERR_HIP;
    if (!dw_full) dw_full = full;
    if (!uw_full) uw_full = full + full_elems;
  }
  const int rc = launch(0, pa, dw_full, uw_full);
  return rc ? rc : post(uw_full, dw_full);
}

// LDS of the K-source kernels (radiance-src, flux, emission response), checked against 160 KiB less room for the static words
template <typename T>
static size_t level_src_lds(int N, int K) {
  return ((size_t)N * (N + K) + (size_t)K * N) * sizeof(T);
}

template <typename T>
static int level_radiance_src_fused(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, int K,
                                    const T* const* a, const T* B, long long bstride, const T* const* c, T* uw, T* dw, T* dw_full,
                                    T* uw_full, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = level_src_lds<T>(N, K);
  VSM_REQUIRE(lds <= 160 * 1024 - 256, "level_radiance_src: N = %d with %d sources needs %zu bytes of LDS", N, K, lds);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_radiance_src<T>), lds, "hipFuncSetAttribute(k_level_radiance_src)");
  if (rc) return rc;
  level_srcs<T> src = {};
  for (int k = 0; k < K; ++k) {
    src.a[k] = a[k];
    src.c[k] = c[k];
  }
  return level_launch<T>(
      ns, nV, row0_h, w_h, (size_t)N * S, dw_full, uw_full, st,
      [&](int nv, const level_pp& pa, T* dwf, T* uwf) {
        hipLaunchKernelGGL(k_level_radiance_src<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, K, nv, pa, A, src, B, bstride, uw, dw,
                           dwf, uwf, status);
        VSM_LAUNCH_CHECK("k_level_radiance_src");
        return (int)VSM_OK;
      },
      [&](const T* uwf, const T* dwf) { return postprocess_vza<T>(N, ns, S, nV, row0_h, w_h, uwf, dwf, uw, dw, st); });
}

// vsm_level_radiance_* (N <= 128): the K-source kernel with one source
template <typename T>
static int level_radiance_fused(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, const T* a, const T* B,
                                long long bstride, const T* c, T* uw, T* dw, T* dw_full, T* uw_full, hipStream_t st) {
  return level_radiance_src_fused<T>(N, ns, S, nV, row0_h, w_h, A, 1, &a, B, bstride, &c, uw, dw, dw_full, uw_full, st);
}

template <typename T>
static int level_flux_fused(int N, int ns, int S, const T* A, int K, const T* const* a, const T* B, long long bstride,
                            const T* const* c, int nW, const T* q, const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, T* out,
                            hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = level_src_lds<T>(N, K);
  VSM_REQUIRE(lds <= 160 * 1024 - 256, "level_flux: N = %d with %d sources needs %zu bytes of LDS", N, K, lds);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_flux<T>), lds, "hipFuncSetAttribute(k_level_flux)");
  if (rc) return rc;
  level_srcs<T> src = {};
  for (int k = 0; k < K; ++k) {
    src.a[k] = A ? a[k] : nullptr;
    src.c[k] = c[k];
  }
  level_flux_dir<T> dir = {};
  for (int r = 0; r < nW; ++r) dir.h[r] = tau_sum ? dir_h[r] : T(0);
  dir.mu0 = mu0;
  hipLaunchKernelGGL(k_level_flux<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, K, nW, (long long)S, A, src, B, bstride, q, dir, tau_sum,
                     F0_I, out, status);
  VSM_LAUNCH_CHECK("k_level_flux");
  return VSM_OK;
}

// LDS of the two inelastic kernels: [M | r], q and the partial sums of the column groups
template <typename T>
static size_t level_ie_lds(int N) {
  return ((size_t)N * (N + 1) + (size_t)N + 2 * (size_t)LEVEL_NT) * sizeof(T);
}

template <typename T>
static int level_radiance_ie_fused(int N, int ns, int S, int K, const int* shift, int nV, const int* row0_h, const T* w_h, const T* A,
                                   const T* B, long long bstride, const T* dwf, const T* uwf, const T* Aie, const T* aie,
                                   const T* Bie, const T* cie, T* uwie, T* dwie, T* dwie_full, T* uwie_full, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = level_ie_lds<T>(N);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_radiance_ie<T>), lds, "hipFuncSetAttribute(k_level_radiance_ie)");
  if (rc) return rc;
  return level_launch<T>(
      ns, nV, row0_h, w_h, (size_t)N * S, dwie_full, uwie_full, st,
      [&](int nv, const level_pp& pa, T* df, T* uf) {
        hipLaunchKernelGGL(k_level_radiance_ie<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, K, shift, nv, pa, A, B, bstride,
                           dwf, uwf, Aie, aie, Bie, cie, uwie, dwie, df, uf, status);
        VSM_LAUNCH_CHECK("k_level_radiance_ie");
        return (int)VSM_OK;
      },
      [&](const T* uf, const T* df) { return postprocess_vza<T>(N, ns, S, nV, row0_h, w_h, uf, df, uwie, dwie, st); });
}

template <typename T>
static int level_flux_ie_fused(int N, int ns, int S, int K, const int* shift, const T* A, const T* B, long long bstride, const T* dwf,
                               const T* uwf, const T* Aie, const T* aie, const T* Bie, const T* cie, int nW, const T* q,
                               const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, T* out, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = level_ie_lds<T>(N);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_flux_ie<T>), lds, "hipFuncSetAttribute(k_level_flux_ie)");
  if (rc) return rc;
  level_flux_dir<T> dir = {};
  for (int r = 0; r < nW; ++r) dir.h[r] = tau_sum ? dir_h[r] : T(0);
  dir.mu0 = mu0;
  hipLaunchKernelGGL(k_level_flux_ie<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, K, shift, nW, A, B, bstride, dwf, uwf, Aie, aie,
                     Bie, cie, q, dir, tau_sum, F0_I, out, status);
  VSM_LAUNCH_CHECK("k_level_flux_ie");
  return VSM_OK;
}

// The derivative of the level equation (vsm_level_radiance_lin_*) at point s = blockIdx.x, for every parameter p:
//   q_p = c'_p + B'_p dw,   r_p = a'_p + A'_p uw + A q_p,   dw'_p = (I - A B)^-1 r_p,   uw'_p = q_p + B dw'_p
// with dw / uw the elastic level vectors of the point (vsm_level_radiance_* dw_full / uw_full).  The parameters run in chunks of
// PC; per chunk:
//   1. the bottom blocks B'_p, c'_p (every slot) and the top blocks A'_p, a'_p (slots < P_top) streamed by column groups:
//      q_p -> Q[pc], s_p = a'_p + A'_p uw -> column N + pc of L;
//   2. level_solve_columns on [M | r_1 .. r_PC] = [I - A B | s + A q]: ONE Gauss-Jordan elimination of the whole block (same M,
//      same rule as the elastic call, hence its pivots), dw'_p in column N + pc of L, uw'_p = q_p + B dw'_p in Q[pc];
//   3. dwd_full / uwd_full (nullable) and the VZA rows ACCUMULATED into [P, S, n_stokes, nV].
// LDS (level_lin_lds): L [N][N + PC], Q [PC][N], dw / uw [2][N], partial sums [2][G][N].
// P_src further slots p = P .. P + P_src - 1 carry a SOURCE alone (vsm_level_radiance_lin_src_*: the equation is linear
// in (a, c), so the derivative with respect to a parameter that only scales the sources is the level equation of those sources):
//   q_p = c_k,   r_p = a_k + A c_k,   dw'_p = (I - A B)^-1 r_p,   uw'_p = c_k + B dw'_p        (k = p - P)
// a_k = asrc [N,1,S,P_src], c_k = csrc likewise.  Such a slot reads no operator derivative: step 1 copies c_k into Q[pc] and a_k into
// column N + pc of L, and steps 2-3 do not tell the two kinds apart (the c_k ride as spare columns of B like every q_p), so a chunk
// may mix them.  P_src = 0 is vsm_level_radiance_lin_* itself: no slot takes that branch.
// FLUX (vsm_level_flux_lin_*): steps 1-2 as they are, but the derivative vectors stay in LDS and another epilogue
// (level_flux_reduce) writes their hemispheric quadratures, slot 1 + p of fx.out [3][nW][1 + P + P_src][S]; slot 0 is the same
// quadrature of the elastic vectors dwf / uwf, and row 2 the direct beam and its derivative -direct tau_sum_dot[p] / mu0 (slots
// p < p_layer; 0 elsewhere and without tau_sum).  A == nullptr (FLUX only; the same for the whole grid): the TOA, no system:
// dw = 0 and dw'_p = 0, uw = uwf, uw'_p = c'_p (c_k for a source-only slot); B, Ad, ad, Bd, dwf are not read.
template <typename T>
struct level_flux_lin_args {
  const T* q;             // DEVICE [nW][N / ns]
  level_flux_dir<T> dir;
  const T* tau_sum;       // [S] or nullptr
  const T* F0_I;          // [S]
  const T* tau_sum_dot;   // [p_layer][S]
  int p_layer, nW;
  T* out;                 // [3][nW][1 + P + P_src][S], written
};

template <typename T, bool FLUX>
__device__ __forceinline__ void level_lin_body(int N, int ns, int S, int P, int P_top, int P_src, int PC, int nV, const level_pp& pa,
                                               const T* __restrict__ A, const T* __restrict__ B, long long bstride,
                                               const T* __restrict__ dwf, const T* __restrict__ uwf, const T* __restrict__ Ad,
                                               long long ad_pstride, const T* __restrict__ ad, const T* __restrict__ Bd,
                                               long long bd_stride, long long bd_pstride, const T* __restrict__ cd,
                                               const T* __restrict__ asrc, const T* __restrict__ csrc, T* uwd, T* dwd, T* dwd_full,
                                               T* uwd_full, int* status,
                                               const level_flux_lin_args<T>& fx = level_flux_lin_args<T>{}) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + PC;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | r_1 .. r_PC], row-major, leading dimension N + PC
  T* Q = L + (size_t)N * LD;                     // q_p, then uw'_p
  T* xs = Q + (size_t)PC * N;                    // dw
  T* ys = xs + N;                                // uw
  T* part = ys + N;                              // [2][G][N] partial sums
  __shared__ int sh[2];
  const int tid = threadIdx.x;
  const long long s = blockIdx.x;
  const long long NN = (long long)N * N, SN = (long long)S * N;
  const bool toa = FLUX && !A;
  const T* As = toa ? nullptr : A + s * NN;
  const T* Bs = toa ? nullptr : B + s * bstride;
  const int G = LEVEL_NT / N, g = tid / N, i1 = tid - g * N;
  for (int i = tid; i < N; i += LEVEL_NT) {
    xs[i] = toa ? T(0) : dwf[s * N + i];
    ys[i] = uwf[s * N + i];
  }
  const int Ptot = P + P_src;
  if (FLUX) {   // slot 0: the quadratures of the elastic vectors; row 2: the direct beam and its derivatives
    __syncthreads();
    level_flux_reduce<T>(N / ns, ns, fx.nW, 1, fx.q, ys, 0, 1, xs, 0, 1, !toa, fx.out, 0, 1 + Ptot, S, s);
    for (int e = tid; e < fx.nW * (1 + Ptot); e += LEVEL_NT) {
      const int r = e / (1 + Ptot), slot = e - r * (1 + Ptot);
      T v = T(0);
      if (fx.tau_sum && slot <= fx.p_layer) {
        v = fx.dir.h[r] * fx.F0_I[s] * exp(-fx.tau_sum[s] / fx.dir.mu0);
        if (slot) v = -v * fx.tau_sum_dot[(long long)(slot - 1) * S + s] / fx.dir.mu0;
      }
      fx.out[(((long long)2 * fx.nW + r) * (1 + Ptot) + slot) * S + s] = v;
    }
  }
  for (int p0 = 0; p0 < Ptot; p0 += PC) {
    const int pc_n = Ptot - p0 < PC ? Ptot - p0 : PC;
    if (tid == 0) sh[1] = 0;
    __syncthreads();   // (dw / uw loaded; the previous chunk's outputs read L and Q)
    // 1. q_p and s_p of the chunk
    for (int pc = 0; pc < pc_n; ++pc) {
      const int p = p0 + pc;
      if (toa) {   // no layer above: uw'_p = c'_p or c_k, dw'_p = 0
        const T* cp = p >= P ? csrc + (long long)(p - P) * SN + s * N : cd + p * SN + s * N;
        for (int i = tid; i < N; i += LEVEL_NT) {
          Q[pc * N + i] = cp[i];
          L[i * LD + N + pc] = T(0);
        }
        continue;
      }
      if (p >= P) {   // a source-only slot (the whole workgroup takes this branch together)
        const long long o = (long long)(p - P) * SN + s * N;
        for (int i = tid; i < N; i += LEVEL_NT) {
          Q[pc * N + i] = csrc[o + i];
          L[i * LD + N + pc] = asrc[o + i];
        }
        continue;
      }
      const bool top = p < P_top;
      level_sums<T> acc = {T(0), T(0)};
      if (g < G)
        acc = level_stream_pair<T>(N, G, g, i1, Bd + p * bd_pstride + s * bd_stride, cd + p * SN + s * N, xs,
                                   top ? Ad + p * ad_pstride + s * NN : nullptr, top ? ad + p * SN + s * N : nullptr, ys, acc);
      level_stream_reduce<T>(N, G, g, i1, acc, part, Q + pc * N, 1, L + N + pc, LD);
    }
    __syncthreads();   // (a chunk may end with source-only slots, which end without a barrier)
    // 2. [M | r], its elimination, dw'_p and uw'_p = q_p + B dw'_p
    if (!toa) level_solve_columns<T>(N, pc_n, LD, As, Bs, L, Q, sh, status);
    if (FLUX) {   // the quadratures of the chunk's vectors, written
      level_flux_reduce<T>(N / ns, ns, fx.nW, pc_n, fx.q, Q, N, 1, L + N, 1, LD, true, fx.out, 1 + p0, 1 + Ptot, S, s);
      continue;
    }
    // 3. the full vectors and the VZA rows
    if (dwd_full || uwd_full) {
      for (int e = tid; e < N * pc_n; e += LEVEL_NT) {
        const int i = e % N, pc = e / N;
        const long long o = (long long)(p0 + pc) * SN + s * N + i;
        if (dwd_full) dwd_full[o] = L[i * LD + N + pc];
        if (uwd_full) uwd_full[o] = Q[pc * N + i];
      }
    }
    for (int e = tid; e < nV * ns * pc_n; e += LEVEL_NT) {
      const int v = e % nV, k = (e / nV) % ns, pc = e / (nV * ns);
      const T w = (T)pa.w[v + nV * k];
      const long long dst = (((long long)(p0 + pc) * S + s) * ns + k) * nV + v;
      uwd[dst] += w * Q[pc * N + pa.row0[v] + k];
      dwd[dst] += w * L[(pa.row0[v] + k) * LD + N + pc];
    }
  }
}

// vsm_level_flux_lin_*: level_lin_body<T, true> (no VZA table, no full vectors out)
template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_flux_lin(int N, int ns, int S, int P, int P_top, int P_src, int PC,
                                                             const T* __restrict__ A, const T* __restrict__ B, long long bstride,
                                                             const T* __restrict__ dwf, const T* __restrict__ uwf,
                                                             const T* __restrict__ Ad, long long ad_pstride,
                                                             const T* __restrict__ ad, const T* __restrict__ Bd, long long bd_stride,
                                                             long long bd_pstride, const T* __restrict__ cd,
                                                             const T* __restrict__ asrc, const T* __restrict__ csrc,
                                                             level_flux_lin_args<T> fx, int* status) {
  const level_pp pa = {};
  level_lin_body<T, true>(N, ns, S, P, P_top, P_src, PC, 0, pa, A, B, bstride, dwf, uwf, Ad, ad_pstride, ad, Bd, bd_stride,
                          bd_pstride, cd, asrc, csrc, nullptr, nullptr, nullptr, nullptr, status, fx);
}

// vsm_level_radiance_lin_* (P_src = 0) and vsm_level_radiance_lin_src_*: level_lin_body<T, false>
template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_radiance_lin_src(int N, int ns, int S, int P, int P_top, int P_src, int PC, int nV,
                                                                     level_pp pa, const T* __restrict__ A, const T* __restrict__ B,
                                                                     long long bstride, const T* __restrict__ dwf,
                                                                     const T* __restrict__ uwf, const T* __restrict__ Ad,
                                                                     long long ad_pstride, const T* __restrict__ ad,
                                                                     const T* __restrict__ Bd, long long bd_stride,
                                                                     long long bd_pstride, const T* __restrict__ cd,
                                                                     const T* __restrict__ asrc, const T* __restrict__ csrc, T* uwd,
                                                                     T* dwd, T* dwd_full, T* uwd_full, int* status) {
  level_lin_body<T, false>(N, ns, S, P, P_top, P_src, PC, nV, pa, A, B, bstride, dwf, uwf, Ad, ad_pstride, ad, Bd, bd_stride,
                           bd_pstride, cd, asrc, csrc, uwd, dwd, dwd_full, uwd_full, status);
}

// LDS of the linearized kernels with PC parameters per chunk (level_lin_body's layout)
template <typename T>
static size_t level_lin_lds(int N, int PC) {
  return ((size_t)N * (N + PC) + (size_t)PC * N + 2 * (size_t)N + 2 * (size_t)LEVEL_NT) * sizeof(T);
}

// What a launch of a linearized kernel over Ptot slots needs: the status word, the parameters per chunk -- as many as the LDS
// holds (160 KiB less room for the static words), at most Ptot -- and the LDS of that chunk, granted to `kernel`.
struct level_lin_launch {
  int* status;
  int PC;
  size_t lds;
};

template <typename T>
static int level_lin_setup(const void* kernel, const char* what, int N, int Ptot, level_lin_launch& su) {
  su.status = device_status();
  if (!su.status) return VSM_ERR_HIP;
  const int pc = (int)((160 * 1024 - 256 - level_lin_lds<T>(N, 0)) / (2 * (size_t)N * sizeof(T)));
  su.PC = pc < Ptot ? pc : Ptot;
  su.lds = level_lin_lds<T>(N, su.PC);
  return ensure_dyn_lds(kernel, su.lds, what);
}

// vsm_level_radiance_lin_* (P_src = 0) and vsm_level_radiance_lin_src_*: the chunks over all P + P_src slots
template <typename T>
static int level_radiance_lin_src_fused(int N, int ns, int S, int P, int P_top, int P_src, int nV, const int* row0_h, const T* w_h,
                                        const T* A, const T* B, long long bstride, const T* dwf, const T* uwf, const T* Ad,
                                        long long ad_pstride, const T* ad, const T* Bd, long long bd_stride, long long bd_pstride,
                                        const T* cd, const T* asrc, const T* csrc, T* uwd, T* dwd, T* dwd_full, T* uwd_full,
                                        hipStream_t st) {
  const int Ptot = P + P_src;
  level_lin_launch su;
  const int rc = level_lin_setup<T>(reinterpret_cast<const void*>(k_level_radiance_lin_src<T>),
                                    "hipFuncSetAttribute(k_level_radiance_lin_src)", N, Ptot, su);
  if (rc) return rc;
  return level_launch<T>(
      ns, nV, row0_h, w_h, (size_t)Ptot * N * S, dwd_full, uwd_full, st,
      [&](int nv, const level_pp& pa, T* df, T* uf) {
        hipLaunchKernelGGL(k_level_radiance_lin_src<T>, dim3(S), dim3(LEVEL_NT), su.lds, st, N, ns, S, P, P_top, P_src, su.PC, nv, pa,
                           A, B, bstride, dwf, uwf, Ad, ad_pstride, ad, Bd, bd_stride, bd_pstride, cd, asrc, csrc, uwd, dwd, df, uf,
                           su.status);
        VSM_LAUNCH_CHECK("k_level_radiance_lin_src");
        return (int)VSM_OK;
      },
      [&](const T* uf, const T* df) { return postprocess_vza_lin<T>(N, ns, S, nV, Ptot, row0_h, w_h, uf, df, uwd, dwd, st); });
}

// vsm_level_flux_lin_*: the chunks and the LDS layout of vsm_level_radiance_lin_src_*
template <typename T>
static int level_flux_lin_fused(int N, int ns, int S, int P, int P_top, int P_src, const T* A, const T* B, long long bstride,
                                const T* dwf, const T* uwf, const T* Ad, long long ad_pstride, const T* ad, const T* Bd,
                                long long bd_stride, long long bd_pstride, const T* cd, const T* asrc, const T* csrc, int nW, const T* q,
                                const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, const T* tau_sum_dot, int p_layer, T* out,
                                hipStream_t st) {
  level_lin_launch su;
  const int rc =
      level_lin_setup<T>(reinterpret_cast<const void*>(k_level_flux_lin<T>), "hipFuncSetAttribute(k_level_flux_lin)", N, P + P_src, su);
  if (rc) return rc;
  level_flux_lin_args<T> fx = {};
  fx.q = q;
  for (int r = 0; r < nW; ++r) fx.dir.h[r] = tau_sum ? dir_h[r] : T(0);
  fx.dir.mu0 = mu0;
  fx.tau_sum = tau_sum;
  fx.F0_I = F0_I;
  fx.tau_sum_dot = tau_sum_dot;
  fx.p_layer = tau_sum ? p_layer : 0;
  fx.nW = nW;
  fx.out = out;
  hipLaunchKernelGGL(k_level_flux_lin<T>, dim3(S), dim3(LEVEL_NT), su.lds, st, N, ns, S, P, P_top, P_src, su.PC, A, B, bstride, dwf,
                     uwf, Ad, ad_pstride, ad, Bd, bd_stride, bd_pstride, cd, asrc, csrc, fx, su.status);
  VSM_LAUNCH_CHECK("k_level_flux_lin");
  return VSM_OK;
}

// operator-level twin: M = I - A B, d = a + A c (two batched products), dw = M^-1 d (vsm_batch_inv + product), uw = c + B dw
template <typename T>
static int level_radiance_oplevel(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, const T* a, const T* B,
                                  long long bstride, const T* c, T* uw, T* dw, T* dw_full, T* uw_full, T* work, hipStream_t st) {
  const long long NN = (long long)N * N;
  T* M = work;
  T* Minv = M + NN * S;
  T* d = Minv + NN * S;
  T* x = dw_full ? dw_full : d + (long long)N * S;
  T* y = uw_full ? uw_full : d + 2 * (long long)N * S;
  int rc = gemm<T>(N, N, N, S, A, NN, B, bstride, M, NN, T(-1), (const T*)nullptr, 0, T(0), T(1), st);
  if (!rc) rc = gemm<T>(N, 1, N, S, A, NN, c, N, d, N, T(1), a, N, T(1), T(0), st);
  if (!rc) rc = batch_inv<T>(N, S, M, Minv, nullptr, st);
  if (!rc) rc = gemm<T>(N, 1, N, S, Minv, NN, d, N, x, N, T(1), (const T*)nullptr, 0, T(0), T(0), st);
  if (!rc) rc = gemm<T>(N, 1, N, S, B, bstride, x, N, y, N, T(1), c, N, T(1), T(0), st);
  if (!rc) rc = postprocess_vza<T>(N, ns, S, nV, row0_h, w_h, y, x, uw, dw, st);
  return rc;
}

// What every level entry point checks of its sizes, bot_stride and viewing-angle table (max_N = 0: any N)
template <typename T>
static int level_check_common(const char* who, int N, int max_N, int ns, int S, int nV, const int* row0_h, const T* w_h,
                              long long bstride, const T* uw, const T* dw) {
  VSM_REQUIRE(N > 0 && ns >= 1 && ns <= 4 && N % ns == 0 && S >= 0 && nV >= 0, "%s: bad size (N %d, n_stokes %d, S %d, nV %d)", who, N,
              ns, S, nV);
  VSM_REQUIRE(max_N == 0 || N <= max_N, "%s: N = %d > %d, the limit of its kernel", who, N, max_N);
  VSM_REQUIRE(bstride == 0 || bstride == (long long)N * N, "%s: bot_stride must be 0 or N*N", who);
  VSM_REQUIRE(S == 0 || nV == 0 || (row0_h && w_h && uw && dw), "%s: null output / viewing-angle table", who);
  for (int v = 0; v < nV; ++v)
    VSM_REQUIRE(row0_h[v] >= 0 && row0_h[v] + ns <= N, "%s: row0[%d] = %d outside the %d streams", who, v, row0_h[v], N);
  return VSM_OK;
}

template <typename T>
static int level_check(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, const T* a, const T* B,
                       long long bstride, const T* c, T* uw, T* dw) {
  const int rc = level_check_common<T>("level_radiance", N, 0, ns, S, nV, row0_h, w_h, bstride, uw, dw);
  if (rc) return rc;
  VSM_REQUIRE(S == 0 || (A && a && B && c), "level_radiance: null operand");
  return VSM_OK;
}

template <typename T>
static int level_src_check(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, int K, const T* const* a,
                           const T* B, long long bstride, const T* const* c, T* uw, T* dw) {
  VSM_REQUIRE(K >= 1 && K <= VSM_LEVEL_MAX_SRC, "level_radiance_src: n_src = %d outside 1..%d", K, (int)VSM_LEVEL_MAX_SRC);
  const int rc = level_check_common<T>("level_radiance_src", N, LEVEL_FUSED_MAX_N, ns, S, nV, row0_h, w_h, bstride, uw, dw);
  if (rc) return rc;
  VSM_REQUIRE(S == 0 || (A && B && a && c), "level_radiance_src: null operand");
  for (int k = 0; k < K && S > 0; ++k) VSM_REQUIRE(a[k] && c[k], "level_radiance_src: null source %d", k);
  return VSM_OK;
}

template <typename T>
static int level_ie_check(int N, int ns, int S, int K, const int* shift, int nV, const int* row0_h, const T* w_h, const T* A,
                          const T* B, long long bstride, const T* dwf, const T* uwf, const T* Aie, const T* aie, const T* Bie,
                          const T* cie, T* uwie, T* dwie) {
  const int rc = level_check_common<T>("level_radiance_ie", N, LEVEL_FUSED_MAX_N, ns, S, nV, row0_h, w_h, bstride, uwie, dwie);
  if (rc) return rc;
  VSM_REQUIRE(K >= 0, "level_radiance_ie: bad size (K %d)", K);
  VSM_REQUIRE(S == 0 || (A && B && dwf && uwf), "level_radiance_ie: null elastic operand");
  VSM_REQUIRE(S == 0 || K == 0 || (shift && Aie && aie), "level_radiance_ie: null shift / top inelastic operand");
  VSM_REQUIRE((Bie == nullptr) == (cie == nullptr), "level_radiance_ie: bot_ieR_mp and bot_ieJ0_m are both given or both NULL");
  return VSM_OK;
}

// vsm_level_flux_ie_*: level_check_common without a viewing-angle table; the TOA (no top) reads the point's own uw and the
// bottom's c_ie alone
template <typename T>
static int level_flux_ie_check(int N, int ns, int S, int K, const int* shift, const T* A, const T* B, long long bstride, const T* dwf,
                               const T* uwf, const T* Aie, const T* aie, const T* Bie, const T* cie, int nW, const T* q,
                               const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, const T* out) {
  VSM_REQUIRE(nW >= 1 && nW <= 4, "level_flux_ie: nW = %d outside 1..4", nW);
  const int rc = level_check_common<T>("level_flux_ie", N, LEVEL_FUSED_MAX_N, ns, S, 0, nullptr, nullptr, bstride, nullptr, nullptr);
  if (rc) return rc;
  VSM_REQUIRE(K >= 0, "level_flux_ie: bad size (K %d)", K);
  VSM_REQUIRE((tau_sum == nullptr) == (F0_I == nullptr), "level_flux_ie: tau_sum and F0_I are both given or both NULL");
  VSM_REQUIRE(!tau_sum || (dir_h && mu0 > T(0)), "level_flux_ie: the direct term needs dir_h and mu0 > 0");
  VSM_REQUIRE(S == 0 || (uwf && q && out), "level_flux_ie: null elastic uw / weight rows / output");
  VSM_REQUIRE(S == 0 || !A || (B && dwf), "level_flux_ie: a top needs the bottom's R-+ and the elastic dw");
  VSM_REQUIRE(S == 0 || K == 0 || shift, "level_flux_ie: null shift");
  VSM_REQUIRE(S == 0 || K == 0 || !A || (Aie && aie), "level_flux_ie: null top inelastic operand");
  VSM_REQUIRE((Bie == nullptr) == (cie == nullptr), "level_flux_ie: bot_ieR_mp and bot_ieJ0_m are both given or both NULL");
  return VSM_OK;
}

template <typename T>
static int level_lin_check(const char* who, int N, int ns, int S, int P, int P_top, int nV, const int* row0_h, const T* w_h,
                           const T* A, const T* B, long long bstride, const T* dwf, const T* uwf, const T* Ad, long long ad_pstride,
                           const T* ad, const T* Bd, long long bd_stride, long long bd_pstride, const T* cd, const T* uwd,
                           const T* dwd) {
  const int rc = level_check_common<T>(who, N, LEVEL_FUSED_MAX_N, ns, S, nV, row0_h, w_h, bstride, uwd, dwd);
  if (rc) return rc;
  VSM_REQUIRE(P >= 1 && P <= 64 && P_top >= 0 && P_top <= P, "%s: bad parameter count (P %d in 1..64, P_top %d in 0..P)", who, P, P_top);
  VSM_REQUIRE(bd_stride == 0 || bd_stride == (long long)N * N, "%s: bot_lin_stride must be 0 or N*N", who);
  VSM_REQUIRE(bd_pstride >= (bd_stride ? (long long)S * N * N : (long long)N * N) && (P_top == 0 || ad_pstride >= (long long)S * N * N),
              "%s: a per-parameter stride is shorter than one parameter's blocks", who);
  VSM_REQUIRE(S == 0 || (A && B && dwf && uwf && Bd && cd), "%s: null operand", who);
  VSM_REQUIRE(S == 0 || P_top == 0 || (Ad && ad), "%s: null top derivative operand", who);
  return VSM_OK;
}

template <typename T>
static int level_lin_src_check(int P, int P_src, int S, const T* asrc, const T* csrc) {
  VSM_REQUIRE(P_src >= 0 && P + P_src <= 64, "level_radiance_lin_src: bad slot count (P %d + P_src %d, P_src >= 0, at most 64 in all)", P,
              P_src);
  VSM_REQUIRE(S == 0 || P_src == 0 || (asrc && csrc), "level_radiance_lin_src: null source operand");
  return VSM_OK;
}

// vsm_level_flux_*: level_check_common without a viewing-angle table, the source lists of level_src_check (a top is optional)
template <typename T>
static int level_flux_check(int N, int ns, int S, const T* A, int K, const T* const* a, const T* B, long long bstride,
                            const T* const* c, int nW, const T* q, const T* dir_h, T mu0, const T* tau_sum, const T* F0_I,
                            const T* out) {
  VSM_REQUIRE(K >= 1 && K <= VSM_LEVEL_MAX_SRC, "level_flux: n_src = %d outside 1..%d", K, (int)VSM_LEVEL_MAX_SRC);
  VSM_REQUIRE(nW >= 1 && nW <= 4, "level_flux: nW = %d outside 1..4", nW);
  const int rc = level_check_common<T>("level_flux", N, LEVEL_FUSED_MAX_N, ns, S, 0, nullptr, nullptr, bstride, nullptr, nullptr);
  if (rc) return rc;
  VSM_REQUIRE((tau_sum == nullptr) == (F0_I == nullptr), "level_flux: tau_sum and F0_I are both given or both NULL");
  VSM_REQUIRE(!tau_sum || (dir_h && mu0 > T(0)), "level_flux: the direct term needs dir_h and mu0 > 0");
  VSM_REQUIRE(S == 0 || (c && q && out), "level_flux: null bottom source list / weight rows / output");
  VSM_REQUIRE(S == 0 || !A || (a && B), "level_flux: a top needs its sources and the bottom's R-+");
  for (int k = 0; k < K && S > 0; ++k) VSM_REQUIRE(c[k] && (!A || a[k]), "level_flux: null source %d", k);
  return VSM_OK;
}

// vsm_level_flux_lin_*: with a top and parameter slots, level_lin_check without a viewing-angle table; the TOA and a call with
// source-only slots alone read no operator derivative and leave those operands out
template <typename T>
static int level_flux_lin_check(int N, int ns, int S, int P, int P_top, int P_src, const T* A, const T* B, long long bstride,
                                const T* dwf, const T* uwf, const T* Ad, long long ad_pstride, const T* ad, const T* Bd,
                                long long bd_stride, long long bd_pstride, const T* cd, const T* asrc, const T* csrc, int nW, const T* q,
                                const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, const T* tau_sum_dot, int p_layer,
                                const T* out) {
  const char* who = "level_flux_lin";
  VSM_REQUIRE(P >= 0 && P_src >= 0 && P + P_src >= 1 && P + P_src <= 64 && P_top >= 0 && P_top <= P,
              "level_flux_lin: bad slot count (P %d + P_src %d in 1..64, P_top %d in 0..P)", P, P_src, P_top);
  VSM_REQUIRE(nW >= 1 && nW <= 4, "level_flux_lin: nW = %d outside 1..4", nW);
  if (A && P > 0) {
    const int rc = level_lin_check<T>(who, N, ns, S, P, P_top, 0, nullptr, nullptr, A, B, bstride, dwf, uwf, Ad, ad_pstride, ad, Bd,
                                      bd_stride, bd_pstride, cd, nullptr, nullptr);
    if (rc) return rc;
  } else {
    const int rc = level_check_common<T>(who, N, LEVEL_FUSED_MAX_N, ns, S, 0, nullptr, nullptr, bstride, nullptr, nullptr);
    if (rc) return rc;
    VSM_REQUIRE(bd_stride == 0 || bd_stride == (long long)N * N, "level_flux_lin: bot_lin_stride must be 0 or N*N");
    VSM_REQUIRE(S == 0 || (uwf && (P == 0 || cd) && (!A || (B && dwf))), "level_flux_lin: null operand");
  }
  VSM_REQUIRE((tau_sum == nullptr) == (F0_I == nullptr), "level_flux_lin: tau_sum and F0_I are both given or both NULL");
  VSM_REQUIRE(!tau_sum || (dir_h && mu0 > T(0)), "level_flux_lin: the direct term needs dir_h and mu0 > 0");
  VSM_REQUIRE(p_layer >= 0 && p_layer <= P, "level_flux_lin: p_layer = %d outside 0..P = %d", p_layer, P);
  VSM_REQUIRE(!tau_sum || p_layer == 0 || tau_sum_dot, "level_flux_lin: the direct term's derivative needs tau_sum_dot");
  VSM_REQUIRE(S == 0 || (q && out), "level_flux_lin: null weight rows / output");
  VSM_REQUIRE(S == 0 || P_src == 0 || (csrc && (!A || asrc)), "level_flux_lin: null source operand");
  return VSM_OK;
}

// The response of the column to a unit hemispheric emission at the lower boundary (vsm_surface_emission_response_*: the SIF
// Jacobian slots of the linearized run).  SurfaceSIF adds the SAME value to j0- of the surface layer at every stream, so the
// radiance is sum_c 2 SIF0[c, s] G_c(s) with G_c the response to the unit pattern e_c (1 on the rows of Stokes component c, 0
// elsewhere): the level equation at the boundary between the atmosphere (A = its R+-, a = 0) and the surface (B = its r-+,
// c_k = e_comp[k]), k_level_radiance_src's system with K <= 4 right-hand sides and no top source, point s = blockIdx.x:
//   level_solve_columns on [M | d_1 .. d_K] = [I - A B | A c_k]:  dw_k,  y_k = c_k + B dw_k  (kept apart, not summed),
//   up_k[v, c, s] = w[v, c] sum_j T--[row0[v] + c, j] y_k[j]   (the TOA leg: interaction!'s J0- = .. + T-- (I - r-+ R+-)^-1 (j0- + r-+ J0+))
//   dn_k[v, c, s] = w[v, c] dw_k[row0[v] + c]                  (the BOA leg: J0+ = t++ (I - R+- r-+)^-1 R+- j0-, t++ = I at m = 0)
// written (not accumulated) per component into up / dn [K][S][n_stokes][nVtot].  y_full / dw_full [K][S][N] (nullable): the
// vectors at all streams, for the caller's own row products above 64 viewing angles.  LDS: L [N][N + K], Q [K][N].
struct emission_comps {
  int c[4];
};

template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_emission_response(int N, int ns, int S, int K, emission_comps comps, int nV, level_pp pa,
                                                                const T* __restrict__ A, const T* __restrict__ Tmm,
                                                                const T* __restrict__ B, long long bstride, T* up, T* dn,
                                                                T* y_full, T* dw_full, int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + K;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | d_1 .. d_K], row-major, leading dimension N + K
  T* Q = L + (size_t)N * LD;                     // c_k, then y_k
  __shared__ int sh[2];
  const int tid = threadIdx.x;
  const long long s = blockIdx.x;
  const long long NN = (long long)N * N;
  const T* Bs = B + s * bstride;
  const T* Ts = Tmm + s * NN;
  if (tid == 0) sh[1] = 0;
  for (int e = tid; e < N * K; e += LEVEL_NT) {
    const int i = e % N, k = e / N;
    L[i * LD + N + k] = T(0);
    Q[k * N + i] = (i % ns == comps.c[k]) ? T(1) : T(0);
  }
  __syncthreads();
  level_solve_columns<T>(N, K, LD, A + s * NN, Bs, L, Q, sh, status);
  if (y_full) {   // (both or neither: the launch above 64 viewing angles)
    for (int e = tid; e < N * K; e += LEVEL_NT) {
      const int i = e % N, k = e / N;
      const long long o = ((long long)k * S + s) * N + i;
      y_full[o] = Q[k * N + i];
      dw_full[o] = L[i * LD + N + k];
    }
  }
  for (int e = tid; e < nV * ns * K; e += LEVEL_NT) {
    const int v = e % nV, c = (e / nV) % ns, k = e / (nV * ns), row = pa.row0[v] + c;
    const T w = (T)pa.w[v + nV * c];
    T u = T(0);
    for (int j = 0; j < N; ++j) u += Ts[(long long)j * N + row] * Q[k * N + j];
    const long long dst = (((long long)k * S + s) * ns + c) * nV + v;
    up[dst] = w * u;
    dn[dst] = w * L[row * LD + N + k];
  }
}

// The row products of k_emission_response for a chunk of at most 64 viewing angles [v0, v0 + nV) out of nVtot, from the vectors at
// all streams: one thread per (v, c, point, k).
template <typename T>
__global__ void __launch_bounds__(256) k_emission_rows(int N, int ns, long long S, int K, int nV, int nVtot, int v0, level_pp pa,
                                                       const T* __restrict__ Tmm, const T* __restrict__ y_full,
                                                       const T* __restrict__ dw_full, T* up, T* dn) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)nV * ns * S * K) return;
  const int v = (int)(e % nV), c = (int)((e / nV) % ns);
  const long long ks = e / ((long long)nV * ns);   // k S + s
  const long long s = ks % S;
  const int row = pa.row0[v] + c;
  const T w = (T)pa.w[v + nV * c];
  const T* Ts = Tmm + s * (long long)N * N;
  const T* y = y_full + ks * N;
  T u = T(0);
  for (int j = 0; j < N; ++j) u += Ts[(long long)j * N + row] * y[j];
  const long long dst = (ks * ns + c) * nVtot + v0 + v;
  up[dst] = w * u;
  dn[dst] = w * dw_full[ks * N + row];
}

template <typename T>
static int emission_response_fused(int N, int ns, int S, int K, const int* comp_h, int nV, const int* row0_h, const T* w_h, const T* A,
                                   const T* Tmm, const T* B, long long bstride, T* up, T* dn, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = level_src_lds<T>(N, K);
  VSM_REQUIRE(lds <= 160 * 1024 - 256, "surface_emission_response: N = %d with %d components needs %zu bytes of LDS", N, K, lds);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_emission_response<T>), lds, "hipFuncSetAttribute(k_emission_response)");
  if (rc) return rc;
  emission_comps comps = {};
  for (int k = 0; k < K; ++k) comps.c[k] = comp_h[k];
  level_pp pa = {};
  if (nV <= 64) {
    for (int v = 0; v < nV; ++v) pa.row0[v] = row0_h[v];
    for (int c = 0; c < ns; ++c)
      for (int v = 0; v < nV; ++v) pa.w[v + nV * c] = (double)w_h[v + nV * c];
    hipLaunchKernelGGL(k_emission_response<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, K, comps, nV, pa, A, Tmm, B, bstride, up, dn,
                       (T*)nullptr, (T*)nullptr, status);
    VSM_LAUNCH_CHECK("k_emission_response");
    return VSM_OK;
  }
  // more viewing angles than one table carries: the vectors at all streams, then the row products in chunks of 64 angles
  const size_t full_elems = (size_t)K * S * N;
  T* full = static_cast<T*>(scratch(2 * full_elems * sizeof(T), 0, st));
  if (!full) return VSM_ERR_HIP;
  hipLaunchKernelGGL(k_emission_response<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, K, comps, 0, pa, A, Tmm, B, bstride, up, dn, full,
                     full + full_elems, status);
  VSM_LAUNCH_CHECK("k_emission_response");
  for (int v0 = 0; v0 < nV; v0 += 64) {
    const int nc = nV - v0 < 64 ? nV - v0 : 64;
    for (int v = 0; v < nc; ++v) pa.row0[v] = row0_h[v0 + v];
    for (int c = 0; c < ns; ++c)
      for (int v = 0; v < nc; ++v) pa.w[v + nc * c] = (double)w_h[v0 + v + nV * c];
    const long long tot = (long long)nc * ns * S * K;
    hipLaunchKernelGGL(k_emission_rows<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, N, ns, (long long)S, K, nc, nV, v0, pa,
                       Tmm, full, full + full_elems, up, dn);
    VSM_LAUNCH_CHECK("k_emission_rows");
  }
  return VSM_OK;
}

template <typename T>
static int emission_response_check(int N, int ns, int S, int K, const int* comp_h, int nV, const int* row0_h, const T* w_h, const T* A,
                                   const T* Tmm, const T* B, long long bstride, const T* up, const T* dn) {
  VSM_REQUIRE(K >= 1 && K <= 4, "surface_emission_response: K = %d outside 1..4", K);
  const int rc = level_check_common<T>("surface_emission_response", N, LEVEL_FUSED_MAX_N, ns, S, nV, row0_h, w_h, bstride, up, dn);
  if (rc) return rc;
  VSM_REQUIRE(comp_h, "surface_emission_response: null component list");
  for (int k = 0; k < K; ++k)
    VSM_REQUIRE(comp_h[k] >= 0 && comp_h[k] < ns, "surface_emission_response: component %d = %d outside 0..%d", k, comp_h[k], ns - 1);
  VSM_REQUIRE(S == 0 || (A && Tmm && B), "surface_emission_response: null operand");
  return VSM_OK;
}

}  // namespace vsm

using namespace vsm;

extern "C" {

size_t vsm_level_radiance_work_elems(int N, int S) {
  return N <= 0 || S <= 0 ? 0 : 2 * (size_t)N * N * S + 3 * (size_t)N * S;
}

#define VSM_LEVEL_API(T, SFX)                                                                                                   \
  int vsm_level_radiance_##SFX(int N, int n_stokes, int S, int nV, const int* row0_h, const T* w_h, const T* top_R_pm,          \
                               const T* top_J0_p, const T* bot_R_mp, long long bot_stride, const T* bot_J0_m, T* uw, T* dw,    \
                               T* dw_full, T* uw_full, T* work, void* stream) {                                                \
    int rc = level_check<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, uw, dw);      \
    if (rc || S == 0) return rc;                                                                                                \
    if (N <= LEVEL_FUSED_MAX_N)                                                                                                 \
      return level_radiance_fused<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, uw, \
                                     dw, dw_full, uw_full, as_stream(stream));                                                  \
    VSM_REQUIRE(work, "level_radiance: N = %d > %d takes the operator-level path: work (vsm_level_radiance_work_elems) required", \
                N, LEVEL_FUSED_MAX_N);                                                                                          \
    return level_radiance_oplevel<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, uw,  \
                                     dw, dw_full, uw_full, work, as_stream(stream));                                            \
  }                                                                                                                             \
  int vsm_level_radiance_oplevel_##SFX(int N, int n_stokes, int S, int nV, const int* row0_h, const T* w_h, const T* top_R_pm,  \
                                       const T* top_J0_p, const T* bot_R_mp, long long bot_stride, const T* bot_J0_m, T* uw,    \
                                       T* dw, T* dw_full, T* uw_full, T* work, void* stream) {                                  \
    int rc = level_check<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, uw, dw);      \
    if (rc || S == 0) return rc;                                                                                                \
    VSM_REQUIRE(work, "level_radiance_oplevel: work (vsm_level_radiance_work_elems) required");                                 \
    return level_radiance_oplevel<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, uw,  \
                                     dw, dw_full, uw_full, work, as_stream(stream));                                            \
  }
VSM_LEVEL_API(double, f64)
VSM_LEVEL_API(float, f32)

#define VSM_LEVEL_SRC_API(T, SFX)                                                                                               \
  int vsm_level_radiance_src_##SFX(int N, int n_stokes, int S, int nV, const int* row0_h, const T* w_h, const T* top_R_pm,     \
                                   int n_src, const T* const* top_J0_p, const T* bot_R_mp, long long bot_stride,              \
                                   const T* const* bot_J0_m, T* uw, T* dw, T* dw_full, T* uw_full, T* work, void* stream) {   \
    (void)work;                                                                                                                \
    int rc = level_src_check<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, n_src, top_J0_p, bot_R_mp, bot_stride, bot_J0_m,   \
                                uw, dw);                                                                                       \
    if (rc || S == 0) return rc;                                                                                               \
    return level_radiance_src_fused<T>(N, n_stokes, S, nV, row0_h, w_h, top_R_pm, n_src, top_J0_p, bot_R_mp, bot_stride,      \
                                       bot_J0_m, uw, dw, dw_full, uw_full, as_stream(stream));                                \
  }
VSM_LEVEL_SRC_API(double, f64)
VSM_LEVEL_SRC_API(float, f32)

#define VSM_LEVEL_FLUX_API(T, SFX)                                                                                              \
  int vsm_level_flux_##SFX(int N, int n_stokes, int S, const T* top_R_pm, int n_src, const T* const* top_J0_p,                 \
                           const T* bot_R_mp, long long bot_stride, const T* const* bot_J0_m, int nW, const T* q,              \
                           const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, T* out, void* stream) {                     \
    int rc = level_flux_check<T>(N, n_stokes, S, top_R_pm, n_src, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, nW, q, dir_h,      \
                                 mu0, tau_sum, F0_I, out);                                                                     \
    if (rc || S == 0) return rc;                                                                                               \
    return level_flux_fused<T>(N, n_stokes, S, top_R_pm, n_src, top_J0_p, bot_R_mp, bot_stride, bot_J0_m, nW, q, dir_h, mu0,  \
                               tau_sum, F0_I, out, as_stream(stream));                                                         \
  }
VSM_LEVEL_FLUX_API(double, f64)
VSM_LEVEL_FLUX_API(float, f32)

#define VSM_LEVEL_IE_API(T, SFX)                                                                                              \
  int vsm_level_radiance_ie_##SFX(int N, int n_stokes, int S, int K, const int* shift, int nV, const int* row0_h, const T* w_h,  \
                                  const T* top_R_pm, const T* bot_R_mp, long long bot_stride, const T* dw_full,               \
                                  const T* uw_full, const T* top_ieR_pm, const T* top_ieJ0_p, const T* bot_ieR_mp,            \
                                  const T* bot_ieJ0_m, T* uwie, T* dwie, T* dwie_full, T* uwie_full, void* stream) {          \
    int rc = level_ie_check<T>(N, n_stokes, S, K, shift, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride, dw_full, uw_full,     \
                               top_ieR_pm, top_ieJ0_p, bot_ieR_mp, bot_ieJ0_m, uwie, dwie);                                   \
    if (rc || S == 0) return rc;                                                                                                \
    return level_radiance_ie_fused<T>(N, n_stokes, S, K, shift, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride, dw_full,       \
                                      uw_full, top_ieR_pm, top_ieJ0_p, bot_ieR_mp, bot_ieJ0_m, uwie, dwie, dwie_full,          \
                                      uwie_full, as_stream(stream));                                                            \
  }
VSM_LEVEL_IE_API(double, f64)
VSM_LEVEL_IE_API(float, f32)

#define VSM_LEVEL_FLUX_IE_API(T, SFX)                                                                                           \
  int vsm_level_flux_ie_##SFX(int N, int n_stokes, int S, int K, const int* shift, const T* top_R_pm, const T* bot_R_mp,        \
                              long long bot_stride, const T* dw_full, const T* uw_full, const T* top_ieR_pm,                   \
                              const T* top_ieJ0_p, const T* bot_ieR_mp, const T* bot_ieJ0_m, int nW, const T* q,               \
                              const T* dir_h, T mu0, const T* tau_sum, const T* F0_I, T* out, void* stream) {                  \
    int rc = level_flux_ie_check<T>(N, n_stokes, S, K, shift, top_R_pm, bot_R_mp, bot_stride, dw_full, uw_full, top_ieR_pm,    \
                                    top_ieJ0_p, bot_ieR_mp, bot_ieJ0_m, nW, q, dir_h, mu0, tau_sum, F0_I, out);                \
    if (rc || S == 0) return rc;                                                                                               \
    return level_flux_ie_fused<T>(N, n_stokes, S, K, shift, top_R_pm, bot_R_mp, bot_stride, dw_full, uw_full, top_ieR_pm,      \
                                  top_ieJ0_p, bot_ieR_mp, bot_ieJ0_m, nW, q, dir_h, mu0, tau_sum, F0_I, out,                   \
                                  as_stream(stream));                                                                          \
  }
VSM_LEVEL_FLUX_IE_API(double, f64)
VSM_LEVEL_FLUX_IE_API(float, f32)

#define VSM_LEVEL_LIN_API(T, SFX)                                                                                               \
  int vsm_level_radiance_lin_##SFX(int N, int n_stokes, int S, int P, int P_top, int nV, const int* row0_h, const T* w_h,      \
                                   const T* top_R_pm, const T* bot_R_mp, long long bot_stride, const T* dw_full,             \
                                   const T* uw_full, const T* top_R_pm_lin, long long top_lin_pstride, const T* top_J0_p_lin, \
                                   const T* bot_R_mp_lin, long long bot_lin_stride, long long bot_lin_pstride,               \
                                   const T* bot_J0_m_lin, T* uw_lin, T* dw_lin, T* dw_lin_full, T* uw_lin_full,               \
                                   void* stream) {                                                                            \
    int rc = level_lin_check<T>("level_radiance_lin", N, n_stokes, S, P, P_top, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride, \
                                dw_full, uw_full, top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin, bot_lin_stride,  \
                                bot_lin_pstride, bot_J0_m_lin, uw_lin, dw_lin);                                               \
    if (rc || S == 0) return rc;                                                                                              \
    return level_radiance_lin_src_fused<T>(N, n_stokes, S, P, P_top, 0, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride,      \
                                           dw_full, uw_full, top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin,       \
                                           bot_lin_stride, bot_lin_pstride, bot_J0_m_lin, (const T*)nullptr,                  \
                                           (const T*)nullptr, uw_lin, dw_lin, dw_lin_full, uw_lin_full, as_stream(stream));   \
  }
VSM_LEVEL_LIN_API(double, f64)
VSM_LEVEL_LIN_API(float, f32)

#define VSM_LEVEL_LIN_SRC_API(T, SFX)                                                                                          \
  int vsm_level_radiance_lin_src_##SFX(int N, int n_stokes, int S, int P, int P_top, int P_src, int nV, const int* row0_h,    \
                                       const T* w_h, const T* top_R_pm, const T* bot_R_mp, long long bot_stride,              \
                                       const T* dw_full, const T* uw_full, const T* top_R_pm_lin, long long top_lin_pstride,  \
                                       const T* top_J0_p_lin, const T* bot_R_mp_lin, long long bot_lin_stride,                \
                                       long long bot_lin_pstride, const T* bot_J0_m_lin, const T* src_top_J0_p,               \
                                       const T* src_bot_J0_m, T* uw_lin, T* dw_lin, T* dw_lin_full, T* uw_lin_full,           \
                                       void* stream) {                                                                        \
    int rc = level_lin_check<T>("level_radiance_lin", N, n_stokes, S, P, P_top, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride, \
                                dw_full, uw_full, top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin, bot_lin_stride,  \
                                bot_lin_pstride, bot_J0_m_lin, uw_lin, dw_lin);                                               \
    if (!rc) rc = level_lin_src_check<T>(P, P_src, S, src_top_J0_p, src_bot_J0_m);                                            \
    if (rc || S == 0) return rc;                                                                                              \
    return level_radiance_lin_src_fused<T>(N, n_stokes, S, P, P_top, P_src, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride,  \
                                           dw_full, uw_full, top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin,       \
                                           bot_lin_stride, bot_lin_pstride, bot_J0_m_lin, src_top_J0_p, src_bot_J0_m, uw_lin, \
                                           dw_lin, dw_lin_full, uw_lin_full, as_stream(stream));                              \
  }
VSM_LEVEL_LIN_SRC_API(double, f64)
VSM_LEVEL_LIN_SRC_API(float, f32)

#define VSM_LEVEL_FLUX_LIN_API(T, SFX)                                                                                         \
  int vsm_level_flux_lin_##SFX(int N, int n_stokes, int S, int P, int P_top, int P_src, const T* top_R_pm, const T* bot_R_mp,  \
                               long long bot_stride, const T* dw_full, const T* uw_full, const T* top_R_pm_lin,               \
                               long long top_lin_pstride, const T* top_J0_p_lin, const T* bot_R_mp_lin,                       \
                               long long bot_lin_stride, long long bot_lin_pstride, const T* bot_J0_m_lin,                    \
                               const T* src_top_J0_p, const T* src_bot_J0_m, int nW, const T* q, const T* dir_h, T mu0,       \
                               const T* tau_sum, const T* F0_I, const T* tau_sum_dot, int p_layer, T* out, void* stream) {    \
    int rc = level_flux_lin_check<T>(N, n_stokes, S, P, P_top, P_src, top_R_pm, bot_R_mp, bot_stride, dw_full, uw_full,       \
                                     top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin, bot_lin_stride,               \
                                     bot_lin_pstride, bot_J0_m_lin, src_top_J0_p, src_bot_J0_m, nW, q, dir_h, mu0, tau_sum,   \
                                     F0_I, tau_sum_dot, p_layer, out);                                                        \
    if (rc || S == 0) return rc;                                                                                              \
    return level_flux_lin_fused<T>(N, n_stokes, S, P, P_top, P_src, top_R_pm, bot_R_mp, bot_stride, dw_full, uw_full,         \
                                   top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin, bot_lin_stride,                 \
                                   bot_lin_pstride, bot_J0_m_lin, src_top_J0_p, src_bot_J0_m, nW, q, dir_h, mu0, tau_sum,     \
                                   F0_I, tau_sum_dot, p_layer, out, as_stream(stream));                                       \
  }
VSM_LEVEL_FLUX_LIN_API(double, f64)
VSM_LEVEL_FLUX_LIN_API(float, f32)

#define VSM_EMISSION_RESPONSE_API(T, SFX)                                                                                       \
  int vsm_surface_emission_response_##SFX(int N, int n_stokes, int S, int K, const int* comp_h, int nV, const int* row0_h,      \
                                          const T* w_h, const T* top_R_pm, const T* top_T_mm, const T* bot_R_mp,               \
                                          long long bot_stride, T* up, T* dn, void* stream) {                                  \
    int rc = emission_response_check<T>(N, n_stokes, S, K, comp_h, nV, row0_h, w_h, top_R_pm, top_T_mm, bot_R_mp, bot_stride,  \
                                        up, dn);                                                                               \
    if (rc || S == 0 || nV == 0) return rc;                                                                                    \
    return emission_response_fused<T>(N, n_stokes, S, K, comp_h, nV, row0_h, w_h, top_R_pm, top_T_mm, bot_R_mp, bot_stride,    \
                                      up, dn, as_stream(stream));                                                              \
  }
VSM_EMISSION_RESPONSE_API(double, f64)
VSM_EMISSION_RESPONSE_API(float, f32)

}  // extern "C"
