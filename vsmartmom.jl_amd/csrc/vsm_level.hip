// Level equation of the multi-sensor run (vsm_level_radiance_*): the radiance field at an interior boundary of the column from the
// composite above it (top) and the composite below it (bottom).  Restates interlayer_flux_helper! (CoreKernel/interlayer_flux.jl:
// 1-19; called through compute_interlayer_flux!, :185-201, by postprocessing_vza_ms!, tools/postprocessing_vza_ms.jl:7-52):
//
//   dw = (I - A B)^-1 (a + A c),   uw = (I - B A)^-1 (c + B a),   A = top R+-, a = top J0+, B = bottom R-+, c = bottom J0-
//
// The reference forms two inverses and four products.  Here uw comes from dw by the push-through identity
// (I - B A)^-1 (c + B a) = c + B (I - A B)^-1 (a + A c) = c + B dw, and dw from ONE pivoted Gauss-Jordan elimination of [M | d]:
//   1. [M | d] = [I - A B | a + A c] in one MFMA product (c rides as the spare column N of B), written to LDS;
//   2. Gauss-Jordan on [M | d] in LDS, the pivot rule of vsm_inverse.h (largest |m_ik|, first occurrence) -- no inverse;
//   3. uw = c + B dw (mat-vec), then the VZA rows of uw / dw added into the caller's [nV, n_stokes, S] outputs.
// One spectral point per 256-thread workgroup, N <= 128 (FP64 [M | d]: 129 KiB of LDS at N = 128).  Larger N: the operator-level
// twin (batched products + vsm_batch_inv + products + vsm_postprocess_vza), the same contract.
//
// vsm_level_radiance_ie_*: the first-order (Raman) part of the same equation, interlayer_flux_helper!(::RRS) (interlayer_flux.jl:
// 21-77), per recipient point with the lines summed before ONE solve of the same [I - A B | r] (k_level_radiance_ie, below).
// vsm_level_radiance_lin_*: its derivative with respect to the Jacobian parameters, the parameters as extra right-hand sides of
// ONE solve per chunk (k_level_radiance_lin, below).
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

// Steps 1-3 for ONE point: [M | d] = [I - A B | a + A c] into L, Gauss-Jordan, dw -> xs, uw = c + B dw -> ys, then dw_full /
// uw_full [N,1,S] (nullable) and the VZA rows accumulated into uw / dw.  Shared by the elastic level kernel and the inelastic one
// (vsm_level_radiance_ie_*), which hands over its line sums (r, q) from LDS as (a, c).  The whole workgroup enters; sh: 2 ints of
// LDS (pivot row, non-finite flag).
template <typename T>
__device__ __forceinline__ void level_solve_point(int N, int ns, int nV, int nVtot, const level_pp& pa, long long s, const T* As,
                                                  const T* as_, const T* Bs, const T* cs, T* L, T* xs, T* ys, T* uw, T* dw,
                                                  T* dw_full, T* uw_full, int* sh, int* status) {
  const int LD = N + 1;
  int& s_piv = sh[0];
  int& s_flag = sh[1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
  if (tid == 0) s_flag = 0;
  __syncthreads();

  // 1. [M | d] = [I | a] - [A B | -A c]: 16 x 16 output tiles over the N x (N + 1) block, round-robin over the four waves
  const int MT = (N + 15) / 16, CT = (N + 16) / 16;
  bool bad = false;
  for (int t = wave; t < MT * CT; t += LEVEL_NT / 64) {
    const int ti = t / CT, tj = t % CT;
    const int row = 16 * ti + li, col = 16 * tj + li;
    typename mfma<T>::acc_t acc = acc_zero<T>();
    for (int k0 = 0; k0 < N; k0 += 4) {
      const int k = k0 + kq;
      const T av = (row < N && k < N) ? As[(long long)k * N + row] : T(0);
      const T bv = (k < N) ? (col < N ? Bs[(long long)col * N + k] : (col == N ? cs[k] : T(0))) : T(0);
      acc = mfma<T>::mma(av, bv, acc);
    }
    const int ocol = 16 * tj + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = 16 * ti + mfma<T>::crow(lane, r);
      if (orow < N && ocol <= N) {
        const T v = ocol < N ? ((orow == ocol ? T(1) : T(0)) - acc[r]) : as_[orow] + acc[r];
        bad |= !isfinite(v);
        L[orow * LD + ocol] = v;
      }
    }
  }
  if (bad) s_flag = 1;
  __syncthreads();
  if (s_flag && tid == 0) atomicOr(&status[0], (int)VSM_DEVSTAT_NONFINITE);

  // 2. Gauss-Jordan elimination of [M | d]: row k is the pivot row of step k and is not normalised; dw_i = d_i / m_ii at the end
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
      for (int j = k + tid; j <= N; j += LEVEL_NT) {
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
      for (int j = k + 1 + tj; j <= N; j += 64) L[i * LD + j] -= f * L[k * LD + j];
    }
    __syncthreads();
  }
  for (int i = tid; i < N; i += LEVEL_NT) xs[i] = L[i * LD + N] / L[i * LD + i];
  __syncthreads();

  // 3. uw = c + B dw
  for (int i = tid; i < N; i += LEVEL_NT) {
    T y = cs[i];
    for (int j = 0; j < N; ++j) y += Bs[(long long)j * N + i] * xs[j];
    ys[i] = y;
    if (dw_full) dw_full[s * N + i] = xs[i];
    if (uw_full) uw_full[s * N + i] = y;
  }
  __syncthreads();
  for (int e = tid; e < nV * ns; e += LEVEL_NT) {
    const int v = e % nV, k = e / nV;
    const T w = (T)pa.w[v + nV * k];
    const long long dst = (s * ns + k) * nVtot + v;
    uw[dst] += w * ys[pa.row0[v] + k];
    dw[dst] += w * xs[pa.row0[v] + k];
  }
}

template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_radiance(int N, int ns, int nV, int nVtot, level_pp pa, const T* __restrict__ A,
                                                             const T* __restrict__ a, const T* __restrict__ B, long long bstride,
                                                             const T* __restrict__ c, T* uw, T* dw, T* dw_full, T* uw_full,
                                                             int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | d], row-major, leading dimension LD = N + 1
  T* xs = L + (size_t)N * (N + 1);               // dw
  T* ys = xs + N;                                // uw
  __shared__ int sh[2];
  const long long s = blockIdx.x;
  level_solve_point<T>(N, ns, nV, nVtot, pa, s, A + s * (long long)N * N, a + s * N, B + s * bstride, c + s * N, L, xs, ys, uw, dw,
                       dw_full, uw_full, sh, status);
}

// The inelastic level equation (vsm_level_radiance_ie_*) of recipient point n1 = blockIdx.x, lines summed before the solve:
//   q = sum_k [c_ie,k + B_ie,k dw(n0)],  r = sum_k [a_ie,k + A_ie,k uw(n0)] + A q,  dw_ie = (I - A B)^-1 r,  uw_ie = q + B dw_ie
// over the in-band lines k (n0 = n1 + shift[k] in 0..S-1); dw / uw are the ELASTIC level vectors of the donors.
// Phase 1 streams the 2K ie blocks of the point: thread (g, i) = (tid / N, tid % N) of G = 256 / N column groups takes row i of
// columns j = g, g + G, ... (column N = the vector), so the workgroup reads G consecutive columns, G N contiguous elements, per
// step; the per-group partial sums are added in group order in LDS.  Phase 2 is level_solve_point with (a, c) = (r - A q, q).
template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_radiance_ie(int N, int ns, int S, int K, const int* __restrict__ shift, int nV,
                                                                int nVtot, level_pp pa, const T* __restrict__ A,
                                                                const T* __restrict__ B, long long bstride,
                                                                const T* __restrict__ dwf, const T* __restrict__ uwf,
                                                                const T* __restrict__ Aie, const T* __restrict__ aie,
                                                                const T* __restrict__ Bie, const T* __restrict__ cie, T* uwie,
                                                                T* dwie, T* dwie_full, T* uwie_full, int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | r], row-major, leading dimension N + 1
  T* xs = L + (size_t)N * (N + 1);               // dw_ie
  T* ys = xs + N;                                // uw_ie
  T* qs = ys + N;                                // q
  T* ps = qs + N;                                // sum_k [a_ie + A_ie uw(n0)]
  T* part = ps + N;                              // [2][G][N] partial sums
  __shared__ int sh[2];
  const int tid = threadIdx.x;
  const int n1 = blockIdx.x;
  const long long NN = (long long)N * N;
  const int G = LEVEL_NT / N, g = tid / N, i = tid - g * N;
  T sp = T(0), sq = T(0);
  if (g < G) {
    for (int k = 0; k < K; ++k) {
      const int n0 = n1 + shift[k];
      if (n0 < 0 || n0 >= S) continue;
      const long long blk = (long long)k * S + n1;
      const T* Ak = Aie + blk * NN;
      const T* Bk = Bie ? Bie + blk * NN : nullptr;
      const T* u0 = uwf + (long long)n0 * N;
      const T* d0 = dwf + (long long)n0 * N;
      for (int j = g; j < N; j += G) {
        sp += Ak[(long long)j * N + i] * u0[j];
        if (Bk) sq += Bk[(long long)j * N + i] * d0[j];
      }
      if (g == (N % G)) {                          // column N: the vectors, taken by the group next in turn
        sp += aie[blk * N + i];
        if (cie) sq += cie[blk * N + i];
      }
    }
    part[g * N + i] = sp;
    part[(G + g) * N + i] = sq;
  }
  __syncthreads();
  if (tid < N) {
    T p = T(0), q = T(0);
    for (int h = 0; h < G; ++h) {
      p += part[h * N + tid];
      q += part[(G + h) * N + tid];
    }
    ps[tid] = p;
    qs[tid] = q;
  }
  __syncthreads();
  level_solve_point<T>(N, ns, nV, nVtot, pa, n1, A + n1 * NN, ps, B + n1 * bstride, qs, L, xs, ys, uwie, dwie, dwie_full, uwie_full,
                       sh, status);
}

template <typename T>
static int level_radiance_fused(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, const T* a, const T* B,
                                long long bstride, const T* c, T* uw, T* dw, T* dw_full, T* uw_full, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = ((size_t)N * (N + 1) + 2 * (size_t)N) * sizeof(T);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_radiance<T>), lds, "hipFuncSetAttribute(k_level_radiance)");
  if (rc) return rc;
  level_pp pa = {};
  if (nV <= 64) {
    for (int v = 0; v < nV; ++v) pa.row0[v] = row0_h[v];
    for (int k = 0; k < ns; ++k)
      for (int v = 0; v < nV; ++v) pa.w[v + nV * k] = (double)w_h[v + nV * k];
    hipLaunchKernelGGL(k_level_radiance<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, nV, nV, pa, A, a, B, bstride, c, uw, dw,
                       dw_full, uw_full, status);
    VSM_LAUNCH_CHECK("k_level_radiance");
    return VSM_OK;
  }
  // more than the 64 viewing angles one launch carries: the level vectors in full, then the VZA rows by vsm_postprocess_vza
  T* full = dw_full && uw_full ? nullptr : static_cast<T*>(scratch(2 * (size_t)N * S * sizeof(T), 0, st));
  if (!dw_full || !uw_full) {
    if (!full) return VSM_ERR_HIP;
    if (!dw_full) dw_full = full;
    if (!uw_full) uw_full = full + (size_t)N * S;
  }
  hipLaunchKernelGGL(k_level_radiance<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, 0, 0, pa, A, a, B, bstride, c, uw, dw, dw_full,
                     uw_full, status);
  VSM_LAUNCH_CHECK("k_level_radiance");
  return postprocess_vza<T>(N, ns, S, nV, row0_h, w_h, uw_full, dw_full, uw, dw, st);
}

template <typename T>
static int level_radiance_ie_fused(int N, int ns, int S, int K, const int* shift, int nV, const int* row0_h, const T* w_h, const T* A,
                                   const T* B, long long bstride, const T* dwf, const T* uwf, const T* Aie, const T* aie,
                                   const T* Bie, const T* cie, T* uwie, T* dwie, T* dwie_full, T* uwie_full, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const size_t lds = ((size_t)N * (N + 1) + 4 * (size_t)N + 2 * (size_t)LEVEL_NT) * sizeof(T);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_radiance_ie<T>), lds, "hipFuncSetAttribute(k_level_radiance_ie)");
  if (rc) return rc;
  level_pp pa = {};
  if (nV <= 64) {
    for (int v = 0; v < nV; ++v) pa.row0[v] = row0_h[v];
    for (int k = 0; k < ns; ++k)
      for (int v = 0; v < nV; ++v) pa.w[v + nV * k] = (double)w_h[v + nV * k];
    hipLaunchKernelGGL(k_level_radiance_ie<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, K, shift, nV, nV, pa, A, B, bstride, dwf,
                       uwf, Aie, aie, Bie, cie, uwie, dwie, dwie_full, uwie_full, status);
    VSM_LAUNCH_CHECK("k_level_radiance_ie");
    return VSM_OK;
  }
  // more than the 64 viewing angles one launch carries: the level vectors in full, then the VZA rows by vsm_postprocess_vza
  T* full = dwie_full && uwie_full ? nullptr : static_cast<T*>(scratch(2 * (size_t)N * S * sizeof(T), 0, st));
  if (!dwie_full || !uwie_full) {
    if (!full) return VSM_ERR_HIP;
    if (!dwie_full) dwie_full = full;
    if (!uwie_full) uwie_full = full + (size_t)N * S;
  }
  hipLaunchKernelGGL(k_level_radiance_ie<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, K, shift, 0, 0, pa, A, B, bstride, dwf, uwf,
                     Aie, aie, Bie, cie, uwie, dwie, dwie_full, uwie_full, status);
  VSM_LAUNCH_CHECK("k_level_radiance_ie");
  return postprocess_vza<T>(N, ns, S, nV, row0_h, w_h, uwie_full, dwie_full, uwie, dwie, st);
}

// The derivative of the level equation (vsm_level_radiance_lin_*) at point s = blockIdx.x, for every parameter p:
//   q_p = c'_p + B'_p dw,   r_p = a'_p + A'_p uw + A q_p,   dw'_p = (I - A B)^-1 r_p,   uw'_p = q_p + B dw'_p
// with dw / uw the elastic level vectors of the point (vsm_level_radiance_* dw_full / uw_full).  The parameters run in chunks of
// PC; per chunk:
//   1. the bottom blocks B'_p, c'_p (every slot) and the top blocks A'_p, a'_p (slots < P_top) streamed by the column groups of
//      k_level_radiance_ie (thread (g, i) of G = 256 / N groups, column N = the vector, partial sums added in group order):
//      q_p -> Q[pc], s_p = a'_p + A'_p uw -> column N + pc of L;
//   2. [M | r_1 .. r_PC] = [I - A B | s + A q] in ONE MFMA product (the q_p ride as extra columns of B, as c does in the elastic
//      kernel), then ONE Gauss-Jordan elimination of the whole block with the pivot rule of level_solve_point (same M, same rule:
//      the elastic call's pivots);
//   3. dw'_p = column / m_ii (in place), uw'_p = q_p + B dw'_p (into Q), the VZA rows ACCUMULATED into [P, S, n_stokes, nV].
// LDS: L [N][N + PC], Q [PC][N], dw / uw [2][N], partial sums [2][G][N].
template <typename T>
__global__ void __launch_bounds__(LEVEL_NT) k_level_radiance_lin(int N, int ns, int S, int P, int P_top, int PC, int nV, level_pp pa,
                                                                 const T* __restrict__ A, const T* __restrict__ B, long long bstride,
                                                                 const T* __restrict__ dwf, const T* __restrict__ uwf,
                                                                 const T* __restrict__ Ad, long long ad_pstride,
                                                                 const T* __restrict__ ad, const T* __restrict__ Bd,
                                                                 long long bd_stride, long long bd_pstride, const T* __restrict__ cd,
                                                                 T* uwd, T* dwd, T* dwd_full, T* uwd_full, int* status) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int LD = N + PC;
  T* L = reinterpret_cast<T*>(lds_raw);          // [M | r_1 .. r_PC], row-major, leading dimension N + PC
  T* Q = L + (size_t)N * LD;                     // q_p, then uw'_p
  T* xs = Q + (size_t)PC * N;                    // dw
  T* ys = xs + N;                                // uw
  T* part = ys + N;                              // [2][G][N] partial sums
  __shared__ int sh[2];
  int& s_piv = sh[0];
  int& s_flag = sh[1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
  const long long s = blockIdx.x;
  const long long NN = (long long)N * N, SN = (long long)S * N;
  const T* As = A + s * NN;
  const T* Bs = B + s * bstride;
  const int G = LEVEL_NT / N, g = tid / N, i1 = tid - g * N;
  for (int i = tid; i < N; i += LEVEL_NT) {
    xs[i] = dwf[s * N + i];
    ys[i] = uwf[s * N + i];
  }
  for (int p0 = 0; p0 < P; p0 += PC) {
    const int pc_n = P - p0 < PC ? P - p0 : PC;
    if (tid == 0) s_flag = 0;
    __syncthreads();   // (dw / uw loaded; the previous chunk's outputs read L and Q)
    // 1. q_p and s_p of the chunk
    for (int pc = 0; pc < pc_n; ++pc) {
      const int p = p0 + pc;
      if (g < G) {
        const bool top = p < P_top;
        const T* Bk = Bd + p * bd_pstride + s * bd_stride;
        const T* Ak = top ? Ad + p * ad_pstride + s * NN : nullptr;
        T sq = T(0), sp = T(0);
        for (int j = g; j < N; j += G) {
          sq += Bk[(long long)j * N + i1] * xs[j];
          if (top) sp += Ak[(long long)j * N + i1] * ys[j];
        }
        if (g == (N % G)) {                          // column N: the vectors, taken by the group next in turn
          sq += cd[p * SN + s * N + i1];
          if (top) sp += ad[p * SN + s * N + i1];
        }
        part[g * N + i1] = sq;
        part[(G + g) * N + i1] = sp;
      }
      __syncthreads();
      if (tid < N) {
        T q = T(0), sp = T(0);
        for (int h = 0; h < G; ++h) {
          q += part[h * N + tid];
          sp += part[(G + h) * N + tid];
        }
        Q[pc * N + tid] = q;
        L[tid * LD + N + pc] = sp;
      }
      __syncthreads();
    }
    // 2. [M | r] = [I | s] - [A B | -A q]: 16 x 16 output tiles over the N x (N + pc_n) block, round-robin over the four waves
    const int NC = N + pc_n;
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
    // Gauss-Jordan elimination of [M | r]: the pivot rule and row operations of level_solve_point over NC columns
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
    // 3. dw'_p = r_p / m_ii (in place: each element is read and written by its own thread), then uw'_p = q_p + B dw'_p
    for (int e = tid; e < N * pc_n; e += LEVEL_NT) {
      const int i = e % N, pc = e / N;
      L[i * LD + N + pc] = L[i * LD + N + pc] / L[i * LD + i];
    }
    __syncthreads();
    for (int e = tid; e < N * pc_n; e += LEVEL_NT) {
      const int i = e % N, pc = e / N;
      T y = Q[pc * N + i];
      for (int j = 0; j < N; ++j) y += Bs[(long long)j * N + i] * L[j * LD + N + pc];
      Q[pc * N + i] = y;
      const long long o = (long long)(p0 + pc) * SN + s * N + i;
      if (dwd_full) dwd_full[o] = L[i * LD + N + pc];
      if (uwd_full) uwd_full[o] = y;
    }
    __syncthreads();
    for (int e = tid; e < nV * ns * pc_n; e += LEVEL_NT) {
      const int v = e % nV, k = (e / nV) % ns, pc = e / (nV * ns);
      const T w = (T)pa.w[v + nV * k];
      const long long dst = (((long long)(p0 + pc) * S + s) * ns + k) * nV + v;
      uwd[dst] += w * Q[pc * N + pa.row0[v] + k];
      dwd[dst] += w * L[(pa.row0[v] + k) * LD + N + pc];
    }
  }
}

// Parameters per chunk of k_level_radiance_lin: as many as the LDS holds (160 KiB less room for the static words), at most P
template <typename T>
static int level_lin_chunk(int N, int P) {
  const size_t budget = (160 * 1024 - 256) / sizeof(T), fixed = (size_t)N * N + 2 * (size_t)N + 2 * (size_t)LEVEL_NT;
  const int pc = (int)((budget - fixed) / (2 * (size_t)N));
  return pc < P ? pc : P;
}

template <typename T>
static size_t level_lin_lds(int N, int PC) {
  return ((size_t)N * (N + PC) + (size_t)PC * N + 2 * (size_t)N + 2 * (size_t)LEVEL_NT) * sizeof(T);
}

template <typename T>
static int level_radiance_lin_fused(int N, int ns, int S, int P, int P_top, int nV, const int* row0_h, const T* w_h, const T* A,
                                    const T* B, long long bstride, const T* dwf, const T* uwf, const T* Ad, long long ad_pstride,
                                    const T* ad, const T* Bd, long long bd_stride, long long bd_pstride, const T* cd, T* uwd,
                                    T* dwd, T* dwd_full, T* uwd_full, hipStream_t st) {
  int* status = device_status();
  if (!status) return VSM_ERR_HIP;
  const int PC = level_lin_chunk<T>(N, P);
  const size_t lds = level_lin_lds<T>(N, PC);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_level_radiance_lin<T>), lds, "hipFuncSetAttribute(k_level_radiance_lin)");
  if (rc) return rc;
  level_pp pa = {};
  if (nV <= 64) {
    for (int v = 0; v < nV; ++v) pa.row0[v] = row0_h[v];
    for (int k = 0; k < ns; ++k)
      for (int v = 0; v < nV; ++v) pa.w[v + nV * k] = (double)w_h[v + nV * k];
    hipLaunchKernelGGL(k_level_radiance_lin<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, P, P_top, PC, nV, pa, A, B, bstride, dwf,
                       uwf, Ad, ad_pstride, ad, Bd, bd_stride, bd_pstride, cd, uwd, dwd, dwd_full, uwd_full, status);
    VSM_LAUNCH_CHECK("k_level_radiance_lin");
    return VSM_OK;
  }
  // more than the 64 viewing angles one launch carries: the derivative vectors in full, then the VZA rows by postprocess_vza_lin
  T* full = dwd_full && uwd_full ? nullptr : static_cast<T*>(scratch(2 * (size_t)P * N * S * sizeof(T), 0, st));
  if (!dwd_full || !uwd_full) {
    if (!full) return VSM_ERR_HIP;
    if (!dwd_full) dwd_full = full;
    if (!uwd_full) uwd_full = full + (size_t)P * N * S;
  }
  hipLaunchKernelGGL(k_level_radiance_lin<T>, dim3(S), dim3(LEVEL_NT), lds, st, N, ns, S, P, P_top, PC, 0, pa, A, B, bstride, dwf, uwf,
                     Ad, ad_pstride, ad, Bd, bd_stride, bd_pstride, cd, uwd, dwd, dwd_full, uwd_full, status);
  VSM_LAUNCH_CHECK("k_level_radiance_lin");
  return postprocess_vza_lin<T>(N, ns, S, nV, P, row0_h, w_h, uwd_full, dwd_full, uwd, dwd, st);
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

template <typename T>
static int level_check(int N, int ns, int S, int nV, const int* row0_h, const T* w_h, const T* A, const T* a, const T* B,
                       long long bstride, const T* c, T* uw, T* dw) {
  VSM_REQUIRE(N > 0 && ns >= 1 && ns <= 4 && N % ns == 0 && S >= 0 && nV >= 0, "level_radiance: bad size (N %d, n_stokes %d, S %d, nV %d)",
              N, ns, S, nV);
  VSM_REQUIRE(bstride == 0 || bstride == (long long)N * N, "level_radiance: bot_stride must be 0 or N*N");
  VSM_REQUIRE(S == 0 || (A && a && B && c), "level_radiance: null operand");
  VSM_REQUIRE(S == 0 || nV == 0 || (row0_h && w_h && uw && dw), "level_radiance: null output / viewing-angle table");
  for (int v = 0; v < nV; ++v)
    VSM_REQUIRE(row0_h[v] >= 0 && row0_h[v] + ns <= N, "level_radiance: row0[%d] = %d outside the %d streams", v, row0_h[v], N);
  return VSM_OK;
}

template <typename T>
static int level_ie_check(int N, int ns, int S, int K, const int* shift, int nV, const int* row0_h, const T* w_h, const T* A,
                          const T* B, long long bstride, const T* dwf, const T* uwf, const T* Aie, const T* aie, const T* Bie,
                          const T* cie, T* uwie, T* dwie) {
  VSM_REQUIRE(N > 0 && N <= LEVEL_FUSED_MAX_N && ns >= 1 && ns <= 4 && N % ns == 0 && S >= 0 && K >= 0 && nV >= 0,
              "level_radiance_ie: bad size (N %d <= %d, n_stokes %d, S %d, K %d, nV %d)", N, LEVEL_FUSED_MAX_N, ns, S, K, nV);
  VSM_REQUIRE(bstride == 0 || bstride == (long long)N * N, "level_radiance_ie: bot_stride must be 0 or N*N");
  VSM_REQUIRE(S == 0 || (A && B && dwf && uwf), "level_radiance_ie: null elastic operand");
  VSM_REQUIRE(S == 0 || K == 0 || (shift && Aie && aie), "level_radiance_ie: null shift / top inelastic operand");
  VSM_REQUIRE((Bie == nullptr) == (cie == nullptr), "level_radiance_ie: bot_ieR_mp and bot_ieJ0_m are both given or both NULL");
  VSM_REQUIRE(S == 0 || nV == 0 || (row0_h && w_h && uwie && dwie), "level_radiance_ie: null output / viewing-angle table");
  for (int v = 0; v < nV; ++v)
    VSM_REQUIRE(row0_h[v] >= 0 && row0_h[v] + ns <= N, "level_radiance_ie: row0[%d] = %d outside the %d streams", v, row0_h[v], N);
  return VSM_OK;
}

template <typename T>
static int level_lin_check(int N, int ns, int S, int P, int P_top, int nV, const int* row0_h, const T* w_h, const T* A, const T* B,
                           long long bstride, const T* dwf, const T* uwf, const T* Ad, long long ad_pstride, const T* ad,
                           const T* Bd, long long bd_stride, long long bd_pstride, const T* cd, T* uwd, T* dwd) {
  VSM_REQUIRE(N > 0 && N <= LEVEL_FUSED_MAX_N && ns >= 1 && ns <= 4 && N % ns == 0 && S >= 0 && nV >= 0,
              "level_radiance_lin: bad size (N %d <= %d, n_stokes %d, S %d, nV %d)", N, LEVEL_FUSED_MAX_N, ns, S, nV);
  VSM_REQUIRE(P >= 1 && P <= 64 && P_top >= 0 && P_top <= P, "level_radiance_lin: bad parameter count (P %d in 1..64, P_top %d in 0..P)",
              P, P_top);
  VSM_REQUIRE(bstride == 0 || bstride == (long long)N * N, "level_radiance_lin: bot_stride must be 0 or N*N");
  VSM_REQUIRE(bd_stride == 0 || bd_stride == (long long)N * N, "level_radiance_lin: bot_lin_stride must be 0 or N*N");
  VSM_REQUIRE(bd_pstride >= (bd_stride ? (long long)S * N * N : (long long)N * N) && (P_top == 0 || ad_pstride >= (long long)S * N * N),
              "level_radiance_lin: a per-parameter stride is shorter than one parameter's blocks");
  VSM_REQUIRE(S == 0 || (A && B && dwf && uwf && Bd && cd), "level_radiance_lin: null operand");
  VSM_REQUIRE(S == 0 || P_top == 0 || (Ad && ad), "level_radiance_lin: null top derivative operand");
  VSM_REQUIRE(S == 0 || nV == 0 || (row0_h && w_h && uwd && dwd), "level_radiance_lin: null output / viewing-angle table");
  for (int v = 0; v < nV; ++v)
    VSM_REQUIRE(row0_h[v] >= 0 && row0_h[v] + ns <= N, "level_radiance_lin: row0[%d] = %d outside the %d streams", v, row0_h[v], N);
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

#define VSM_LEVEL_IE_API(T, SFX)                                                                                                \
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

#define VSM_LEVEL_LIN_API(T, SFX)                                                                                               \
  int vsm_level_radiance_lin_##SFX(int N, int n_stokes, int S, int P, int P_top, int nV, const int* row0_h, const T* w_h,      \
                                   const T* top_R_pm, const T* bot_R_mp, long long bot_stride, const T* dw_full,             \
                                   const T* uw_full, const T* top_R_pm_lin, long long top_lin_pstride, const T* top_J0_p_lin, \
                                   const T* bot_R_mp_lin, long long bot_lin_stride, long long bot_lin_pstride,               \
                                   const T* bot_J0_m_lin, T* uw_lin, T* dw_lin, T* dw_lin_full, T* uw_lin_full,               \
                                   void* stream) {                                                                            \
    int rc = level_lin_check<T>(N, n_stokes, S, P, P_top, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride, dw_full, uw_full,  \
                                top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin, bot_lin_stride, bot_lin_pstride,   \
                                bot_J0_m_lin, uw_lin, dw_lin);                                                                \
    if (rc || S == 0) return rc;                                                                                              \
    return level_radiance_lin_fused<T>(N, n_stokes, S, P, P_top, nV, row0_h, w_h, top_R_pm, bot_R_mp, bot_stride, dw_full,    \
                                       uw_full, top_R_pm_lin, top_lin_pstride, top_J0_p_lin, bot_R_mp_lin, bot_lin_stride,    \
                                       bot_lin_pstride, bot_J0_m_lin, uw_lin, dw_lin, dw_lin_full, uw_lin_full,               \
                                       as_stream(stream));                                                                    \
  }
VSM_LEVEL_LIN_API(double, f64)
VSM_LEVEL_LIN_API(float, f32)

}  // extern "C"
