// Single-scattering column walks: rt_run_ss (src/CoreRT/rt_run.jl:574-755), one launch per Fourier moment.
//   vsm_ss_column_*      rt_kernel_ss!(::noRS) (CoreKernel/rt_kernel_ss.jl:156-238): get_elem_rt_SFI! (elemental.jl:348-392) with
//                        ndoubl = 0 and dtau = tau, get_interaction_ss! (interaction_ss.jl:14-19), the surface's interaction_ss!
//                        (rt_run.jl:715-722) and the viewing rows of postprocessing_vza! (postprocessing_vza.jl:23-94)
//   vsm_ss_column_rrs_*  rt_kernel_ss!(::RRS) (:240-337): get_elem_rt_SFI_RRS! (elemental_inelastic.jl:479-603),
//                        get_interaction_ss_RRS! (interaction_ss.jl:79-90), postprocessing_vza!(::RRS) (:139-142)
//   vsm_ss_column_lin_*  the parameter derivative of vsm_ss_column_*: the source derivatives of get_elem_rt_SFI_fused!
//                        (elemental_lin.jl:602-712) with ndoubl = 0 and dtau = tau, the two differentiated statements of
//                        get_interaction_ss!, the linearized surface builders' sources and postprocessing_vza! (lin)
//   vsm_ss_column_rrs_lin_*  the parameter derivative of vsm_ss_column_rrs_* (the reference has none): the chain rule through
//                        tau[n0], tau[n1] and fscatt[n0] exp(-tau_sum[n0] / mu_0), the close branches by their limit partials
// Lanes run along the spectral axis; a thread carries the running sources of SS_RB rows of its point in registers through all
// layers.  Nothing here is N x N: of the phase matrices only the n_stokes SZA columns are read.
#include "vsm_common.h"
#include "vsm_internal.h"

namespace vsm {

constexpr int SS_TB = VSM_SS_BLOCK;   // spectral points (= threads) per workgroup: two waves
constexpr int SS_RB = 4;              // rows per thread; more rows go to further workgroups along grid.y
constexpr int SS_PC = 4;              // parameter slots a thread of the elastic derivative carries; further slots go along grid.z
constexpr int SS_RPC = 2;             // parameter slots a thread of the Raman derivative carries: (12 + 2 SS_RPC) staged values per window
                                      // point = 64 KB of LDS at FP64 with the maximal halo (the forward kernel's 12 values: 48 KB)
constexpr int SS_SLOT = 5;            // library scratch slot of the device tables

template <typename T>
struct ss_layer {
  const T *tau, *varpi, *tau_sum, *zpp, *zmp, *fscatt;
  long long zs;
};
template <typename T>
struct ss_layer_lin {
  const T *tau, *varpi, *tau_sum, *zpp, *zmp;
  const T *tau_dot, *varpi_dot, *tau_sum_dot;   // [S, p_layer] each (tau_dot: of the layer's full tau)
  const T* zdcoef;                              // [CT, p_layer, S] or null (Z_dot = 0)
  long long zs;
};
template <typename T>
struct ss_layer_rrs_lin {
  const T *tau, *tau_sum, *fscatt;
  const T *tau_dot, *tau_sum_dot, *fscatt_dot;   // [S, p_layer] each (tau_dot: of the layer's full tau)
};

template <typename T>
struct ss_tol {
  static __device__ __forceinline__ T close() { return T(1e-8); }   // rt_close_tol (rt_helpers.jl:66-68)
};

// ---------------------------------------------------------------------------------------------------------------------
// the pieces the four column kernels share
// ---------------------------------------------------------------------------------------------------------------------
// The rows a thread owns.  VIEW: item e = v + nV k of the viewing table (row row0[v] + k, weight w[e], output (s, k, v));
// otherwise item e = stream row e of the full source vectors.
template <typename T>
struct ss_rows {
  int i[SS_RB];
  bool on[SS_RB];
  T mi[SS_RB];
};
template <typename T>
__device__ __forceinline__ ss_rows<T> ss_pick_rows(bool view, int N, int ns, int nV, const int* __restrict__ row0,
                                                   const T* __restrict__ mu, int item0) {
  ss_rows<T> r;
  const int nitems = view ? nV * ns : N;
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    const int e = item0 + j;
    r.on[j] = e < nitems;
    const int ec = r.on[j] ? e : 0;
    r.i[j] = view ? row0[ec % nV] + ec / nV : ec;
    r.mi[j] = mu[r.i[j]];
  }
  return r;
}
// where item e of the viewing table goes in an output (S, n_stokes, nV), or in slot p of an output (P, S, n_stokes, nV)
__device__ __forceinline__ long long ss_view_index(long long s, int ns, int nV, int e, int p = 0, long long S = 0) {
  return (((long long)p * S + s) * ns + e / nV) * nV + e % nV;
}

template <typename T>
struct ss_pair {
  T p, m;   // the + and the - direction
};
// (Z F0) at one row: of the phase matrices Z++ / Z-+ only the n_stokes SZA columns are read.  beam: the point's F0, in registers
// or in global memory (F0 + ns * n0).
template <typename T>
__device__ __forceinline__ ss_pair<T> ss_zf0(const T* zpp, const T* zmp, int N, int ns, int i_start, int row, const T* beam) {
  T zp = 0, zm = 0;
  for (int q = 0; q < ns; ++q) {
    const long long zo = row + (long long)N * (i_start + q);
    const T f = beam[q];
    zp += zpp[zo] * f;
    zm += zmp[zo] * f;
  }
  return {zp, zm};
}

// The elastic sources of one row in one layer: get_elem_rt_SFI! with dtau = tau, ndoubl = 0 (the statements of k_elemental_sfi,
// vsm_generic.hip), times the beam's attenuation att.  LIN: with their partial derivatives in tau, varpi and (Z F0) (the
// statements of k_elemental_sfi_lin, vsm_lin.hip); the forward kernel compiles none of them.
template <typename T, bool LIN>
struct ss_elastic {
  T jp, jm;
};
template <typename T>
struct ss_elastic<T, true> {
  T jp, jm, jp_tau, jp_w, jp_Z, jm_tau, jm_w, jm_Z;
};
template <typename T, bool LIN>
__device__ __forceinline__ ss_elastic<T, LIN> ss_elastic_src(bool sun, T wct02, T wv, ss_pair<T> z, T d, T mi, T ms, T att) {
  ss_elastic<T, LIN> r;
  if (sun) {
    r.jp = wct02 * wv * z.p * (d / mi) * exp(-d / mi);
    if constexpr (LIN) r.jp_tau = r.jp * (T(1) / d - T(1) / mi);
  } else {
    r.jp = wct02 * wv * z.p * (ms / (mi - ms)) * expdiff_neg<T>(d / mi, d / ms);
    if constexpr (LIN) r.jp_tau = -wct02 * wv * z.p * (ms / (mi - ms)) * (exp(-d / mi) / mi - exp(-d / ms) / ms);
  }
  const T gm = ms / (mi + ms);
  const T narg = -d * ((T(1) / mi) + (T(1) / ms));
  r.jm = wct02 * wv * z.m * gm * (-expm1(narg));
  if constexpr (LIN) {
    r.jp_w = (wv == T(0)) ? T(0) : r.jp / wv;
    r.jp_Z = (z.p == T(0)) ? T(0) : r.jp / z.p;
    r.jm_tau = wct02 * wv * z.m * gm * exp(narg) * ((T(1) / mi) + (T(1) / ms));
    r.jm_w = (wv == T(0)) ? T(0) : r.jm / wv;
    r.jm_Z = (z.m == T(0)) ? T(0) : r.jm / z.m;
    r.jp_tau *= att; r.jp_w *= att; r.jp_Z *= att;
    r.jm_tau *= att; r.jm_w *= att; r.jm_Z *= att;
  }
  r.jp *= att;
  r.jm *= att;
  return r;
}

// What a (recipient, line) pair of the Raman columns reads of its donor n0 in one layer: d0 = tau[n0], x0 = d0 / mu0 as
// e0 = exp(-x0) and a0 = expm1(-x0), g0 = fscatt[n0] exp(-tau_sum[n0] / mu0).  The fill values are those of a window point
// outside the band, which no line reads.
template <typename T>
struct ss_donor {
  T d0 = T(1), e0 = T(0), a0 = T(0), g0 = T(0);
  static __device__ __forceinline__ ss_donor load(const ss_layer<T>& ly, long long n0, T ms) {
    ss_donor r;
    r.d0 = ly.tau[n0];
    const T x0 = r.d0 / ms;
    r.e0 = exp(-x0);
    r.a0 = expm1(-x0);
    r.g0 = ly.fscatt[n0] * exp(-ly.tau_sum[n0] / ms);
    return r;
  }
};

// The LDS window of a workgroup of the Raman columns: the points within `halo` of its SS_TB recipients.  Per point the donor
// factors of the current layer -- formed once per (point, layer), not once per line --, per row of the thread Z_ie F0[:, n0] (layer
// independent: staged once per workgroup) and, in the derivative kernel, the donor's derivatives:
//   sd | se0 | sa0 | sg [W] each | szp | szm [SS_RB][W] | sdd | sgd [SS_RPC][W].
// A line whose donor lies outside the window takes the same values from global memory.  The launchers take the byte count from
// here and k_ss_column_rrs_lin its carve-up; k_ss_column_rrs carves the same layout by hand (through this struct it measures
// 0.5 % slower).
template <typename T, bool LIN>
struct ss_window {
  static constexpr int values = 4 + 2 * SS_RB + (LIN ? 2 * SS_RPC : 0);   // staged per window point
  static constexpr size_t bytes(int halo) { return sizeof(T) * (size_t)values * (size_t)(SS_TB + 2 * halo); }
  int W;
  T *sd, *se0, *sa0, *sg, *szp, *szm, *sdd, *sgd;   // (sdd, sgd: LIN only)
  long long w0;                                     // the window's first point
  __device__ __forceinline__ ss_window(unsigned char* smem, int halo) {
    W = SS_TB + 2 * halo;
    sd = reinterpret_cast<T*>(smem), se0 = sd + W, sa0 = se0 + W, sg = sa0 + W;
    szp = sg + W, szm = szp + SS_RB * W;
    sdd = LIN ? szm + SS_RB * W : nullptr, sgd = LIN ? sdd + SS_RPC * W : nullptr;
    w0 = (long long)blockIdx.x * SS_TB - halo;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// elastic column
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, bool VIEW>
__global__ __launch_bounds__(SS_TB) void k_ss_column(int N, int ns, int S, int L, int m, int i_mu0,
                                                     const ss_layer<T>* __restrict__ lay, const T* __restrict__ F0,
                                                     const T* __restrict__ sj_m, const T* __restrict__ sj_p,
                                                     const T* __restrict__ ts_surf, const T* __restrict__ mu, int nV,
                                                     const int* __restrict__ row0, const T* __restrict__ w, T* R, T* Tt) {
  const long long s = (long long)blockIdx.x * SS_TB + threadIdx.x;
  if (s >= S) return;
  const int i_start = ns * i_mu0;
  const ss_rows<T> rw = ss_pick_rows<T>(VIEW, N, ns, nV, row0, mu, blockIdx.y * SS_RB);
  const T ms = mu[i_start];
  const T wct02 = (m == 0) ? T(0.5) : T(0.25);
  T f0[4] = {0, 0, 0, 0};
  for (int q = 0; q < ns; ++q) f0[q] = F0[q + (long long)ns * s];
  T Jp[SS_RB], Jm[SS_RB];
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) Jp[j] = Jm[j] = T(0);
  for (int iz = 0; iz < L; ++iz) {
    const ss_layer<T> ly = lay[iz];
    const T d = ly.tau[s], wv = ly.varpi[s], ts = ly.tau_sum[s];
    const T att = exp(-ts / ms);
    const T* zpp = ly.zpp + s * ly.zs;
    const T* zmp = ly.zmp + s * ly.zs;
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      if (!rw.on[j]) continue;
      const int i = rw.i[j];
      const T mi = rw.mi[j];
      const ss_elastic<T, false> e = ss_elastic_src<T, false>(i >= i_start && i < i_start + ns, wct02, wv,
                                                              ss_zf0<T>(zpp, zmp, N, ns, i_start, i, f0), d, mi, ms, att);
      if (iz == 0) {   // rt_kernel_ss.jl:213-216: the TOA layer is copied
        Jp[j] = e.jp;
        Jm[j] = e.jm;
      } else {         // get_interaction_ss! (interaction_ss.jl:17-18)
        Jp[j] = Jp[j] * exp(-d / mi) + e.jp;
        Jm[j] = Jm[j] + e.jm * exp(-ts / mi);
      }
    }
  }
  // interaction_ss! with the surface layer (rt_run.jl:715-722): layer tau = 0, tau_sum = tau_sum_all[:, Nz + 1]
  const T tss = ts_surf[s];
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    if (!rw.on[j]) continue;
    const long long src = s * N + rw.i[j];
    Jp[j] = Jp[j] * exp(-T(0) / rw.mi[j]) + (sj_p ? sj_p[src] : T(0));
    Jm[j] = Jm[j] + sj_m[src] * exp(-tss / rw.mi[j]);
    if (VIEW) {
      const int e = blockIdx.y * SS_RB + j;
      const long long dst = ss_view_index(s, ns, nV, e);
      R[dst] += w[e] * Jm[j];
      Tt[dst] += w[e] * Jp[j];
    } else {
      R[src] = Jm[j];
      Tt[src] = Jp[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Raman column
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SS_TB) void k_ss_column_rrs(int N, int ns, int S, int L, int K, int m, int i_mu0, int halo,
                                                         const ss_layer<T>* __restrict__ lay, const int* __restrict__ shift,
                                                         const T* __restrict__ varpi_ie, const T* __restrict__ Zpp,
                                                         const T* __restrict__ Zmp, const T* __restrict__ F0,
                                                         const T* __restrict__ mu, int nV, const int* __restrict__ row0,
                                                         const T* __restrict__ w, T* ieR, T* ieT) {
  extern __shared__ __align__(16) unsigned char ss_smem[];
  const int W = SS_TB + 2 * halo;   // ss_window<T, false>, carved by hand (see there)
  T *sd = reinterpret_cast<T*>(ss_smem), *se0 = sd + W, *sa0 = se0 + W, *sg = sa0 + W, *szp = sg + W, *szm = szp + SS_RB * W;
  const long long b0 = (long long)blockIdx.x * SS_TB, w0 = b0 - halo, n1 = b0 + threadIdx.x;
  const bool live = n1 < S;
  const int i_start = ns * i_mu0;
  const ss_rows<T> rw = ss_pick_rows<T>(true, N, ns, nV, row0, mu, blockIdx.y * SS_RB);
  const T ms = mu[i_start];
  const T wct02 = (m == 0) ? T(0.5) : T(0.25);
  for (int p = threadIdx.x; p < W; p += SS_TB) {   // Z_ie F0 of the thread's rows at every window point, once per workgroup
    const long long n0 = w0 + p;
    const bool in = n0 >= 0 && n0 < S;
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      ss_pair<T> z{T(0), T(0)};
      if (in && rw.on[j]) z = ss_zf0<T>(Zpp, Zmp, N, ns, i_start, rw.i[j], F0 + (long long)ns * n0);
      szp[j * W + p] = z.p;
      szm[j * W + p] = z.m;
    }
  }
  T rm[SS_RB], Sp[SS_RB], Sm[SS_RB];
  bool sun[SS_RB];
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    rm[j] = rw.mi[j] / ms;
    sun[j] = rw.i[j] >= i_start && rw.i[j] < i_start + ns;
    Sp[j] = Sm[j] = T(0);
  }
  for (int iz = 0; iz < L; ++iz) {
    const ss_layer<T> ly = lay[iz];
    __syncthreads();   // the previous layer's readers are done (first pass: nothing to wait for but the Z F0 stage)
    for (int p = threadIdx.x; p < W; p += SS_TB) {   // the donor factors of this layer at every window point
      const long long n0 = w0 + p;
      ss_donor<T> don;
      if (n0 >= 0 && n0 < S) don = ss_donor<T>::load(ly, n0, ms);
      sd[p] = don.d0, se0[p] = don.e0, sa0[p] = don.a0, sg[p] = don.g0;
    }
    __syncthreads();
    if (!live) continue;
    const T d1 = ly.tau[n1], ts1 = ly.tau_sum[n1];
    T x1[SS_RB], e1[SS_RB], a1[SS_RB], sp[SS_RB], sm[SS_RB];
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      x1[j] = d1 / rw.mi[j];
      e1[j] = exp(-x1[j]);
      a1[j] = expm1(-x1[j]);
      sp[j] = sm[j] = T(0);
    }
    for (int dn = 0; dn < K; ++dn) {
      const long long n0 = n1 + shift[dn];
      if (n0 < 0 || n0 >= S) continue;   // out of band: exactly zero (elemental_inelastic.jl:500)
      const T wl = varpi_ie[dn];
      const long long p = n0 - w0;
      const bool staged = p >= 0 && p < W;
      T d0, e0, a0, g0;
      if (staged) {
        d0 = sd[p], e0 = se0[p], a0 = sa0[p], g0 = sg[p];
      } else {   // a shift beyond the staged window: the same factors from global memory
        const ss_donor<T> don = ss_donor<T>::load(ly, n0, ms);
        d0 = don.d0, e0 = don.e0, a0 = don.a0, g0 = don.g0;
      }
      const T x0 = d0 / ms;
      const T ratio = d1 / d0;
#pragma unroll
      for (int j = 0; j < SS_RB; ++j) {
        if (!rw.on[j]) continue;
        const ss_pair<T> z = staged ? ss_pair<T>{szp[j * W + p], szm[j * W + p]}
                                           : ss_zf0<T>(Zpp, Zmp, N, ns, i_start, rw.i[j], F0 + (long long)ns * n0);
        const T zp = z.p, zm = z.m;
        const T mi = rw.mi[j];
        // expdiff_neg(d1 / mu_i, d0 / mu_0) (rt_helpers.jl:32-40) from e1 = exp(-x1), e0 = exp(-x0): one expm1 is left
        const T xa = x1[j];
        const T ed = (xa == x0) ? T(0) : ((xa < x0) ? e1[j] * (-expm1(-(x0 - xa))) : -e0 * (-expm1(-(xa - x0))));
        // The line source stays this formulation (not the G / H of ss_rrs_line below): rt_run_ss_rrs promises these bits
        T jp;
        if (sun[j]) {   // elemental_inelastic.jl:508-548 (mu_i = mu_0 on these rows)
          if (fabs(d0 - d1) > ss_tol<T>::close())
            jp = wl * g0 * zp * wct02 * ed / (T(1) - ratio);
          else
            jp = (d0 / mi) * wct02 * wl * g0 * zp * e0;
        } else {        // :549-560
          const T den = rm[j] - ratio;
          if (fabs(den) < ss_tol<T>::close())
            jp = (d0 / mi) * wct02 * wl * g0 * zp * e0;
          else
            jp = wct02 * wl * g0 * zp * (T(1) / den) * ed;
        }
        // :577-579; 1 - exp(-(x1 + x0)) = -(a1 + a0 + a1 a0) with a = expm1(-x): no cancellation, no transcendental
        const T jm = wct02 * wl * g0 * zm * (T(1) / (rm[j] + ratio)) * (-(a1[j] + a0 + a1[j] * a0));
        sp[j] += jp;
        sm[j] += jm;
      }
    }
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      if (iz == 0) {   // rt_kernel_ss.jl:308-314
        Sp[j] = sp[j];
        Sm[j] = sm[j];
      } else {         // get_interaction_ss_RRS! (interaction_ss.jl:87-88) on the line sums: exp(-tau[n1] / mu_i) has no line index
        Sp[j] = Sp[j] * e1[j] + sp[j];
        Sm[j] = Sm[j] + sm[j] * exp(-ts1 / rw.mi[j]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    if (!rw.on[j]) continue;
    const int e = blockIdx.y * SS_RB + j;
    const long long dst = ss_view_index(n1, ns, nV, e);
    ieR[dst] += w[e] * Sm[j];
    ieT[dst] += w[e] * Sp[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// elastic column, linearized
// ---------------------------------------------------------------------------------------------------------------------
// The derivative of k_ss_column<T, true> for the slots [p_lo + SS_PC blockIdx.z, +SS_PC) below p_hi.  Per layer the forward
// factors of the thread's rows are formed again (they are cheap: ss_elastic_src with its partials), the slot loop applies the
// chain rule of get_elem_rt_SFI_fused! and the derivative of get_interaction_ss!, taken on J0+ BEFORE its update:
//   J0+' = (J0+' - J0+ tau' / mu_i) exp(-tau / mu_i) + j0+',    J0-' += (j0-' - j0- tau_sum' / mu_i) exp(-tau_sum / mu_i).
// Z_dot F0 at a row is sum_c zdcoef[c, p, s] (Zc[c] F0)_row over the CT component blocks of the moment, for the first p_zdot slots
// (the aerosols'; the gases' coefficients are exact zeros and are not read): no Z_dot array exists.  ZD = false: no layer has one.
// Slots >= p_layer (the surface's) are exact zeros in the atmospheric layers and are not touched there.
template <typename T, bool ZD>
__global__ __launch_bounds__(SS_TB) void k_ss_column_lin(int N, int ns, int S, int L, int m, int i_mu0, int P, int p_layer,
                                                         int p_zdot, int p_lo, int p_hi, const ss_layer_lin<T>* __restrict__ lay, int CT,
                                                         const T* __restrict__ Zc_pp, const T* __restrict__ Zc_mp,
                                                         const T* __restrict__ F0, const T* __restrict__ sj_m,
                                                         const T* __restrict__ sj_p, const T* __restrict__ sjd_m,
                                                         const T* __restrict__ sjd_p, const T* __restrict__ ts_surf,
                                                         const T* __restrict__ tsd_surf, const T* __restrict__ mu, int nV,
                                                         const int* __restrict__ row0, const T* __restrict__ w, T* Rd, T* Td) {
  const long long s = (long long)blockIdx.x * SS_TB + threadIdx.x;
  if (s >= S) return;
  const int i_start = ns * i_mu0;
  const int p0 = p_lo + (int)blockIdx.z * SS_PC;
  const ss_rows<T> rw = ss_pick_rows<T>(true, N, ns, nV, row0, mu, blockIdx.y * SS_RB);
  const T ms = mu[i_start];
  const T wct02 = (m == 0) ? T(0.5) : T(0.25);
  const long long NN = (long long)N * N;
  T f0[4] = {0, 0, 0, 0};
  for (int q = 0; q < ns; ++q) f0[q] = F0[q + (long long)ns * s];
  T Jp[SS_RB], Dp[SS_RB][SS_PC], Dm[SS_RB][SS_PC];
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    Jp[j] = T(0);
#pragma unroll
    for (int k = 0; k < SS_PC; ++k) Dp[j][k] = Dm[j][k] = T(0);
  }
  for (int iz = 0; iz < L; ++iz) {
    const ss_layer_lin<T> ly = lay[iz];
    const T d = ly.tau[s], wv = ly.varpi[s], ts = ly.tau_sum[s];
    const T att = exp(-ts / ms);
    const T* zpp = ly.zpp + s * ly.zs;
    const T* zmp = ly.zmp + s * ly.zs;
    // the slots of this chunk in the layer: tau', varpi', the beam term -tau_sum' / mu_0 (elemental_lin.jl:602-712)
    T td[SS_PC], wd[SS_PC], tsd[SS_PC];
#pragma unroll
    for (int k = 0; k < SS_PC; ++k) {
      const int p = p0 + k;
      const bool in = p < p_hi && p < p_layer;
      const long long o = s + (long long)S * (in ? p : 0);
      td[k] = in ? ly.tau_dot[o] : T(0);
      wd[k] = in ? ly.varpi_dot[o] : T(0);
      tsd[k] = in ? ly.tau_sum_dot[o] : T(0);
    }
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      if (!rw.on[j]) continue;
      const int i = rw.i[j];
      const T mi = mu[i];
      const ss_elastic<T, true> e = ss_elastic_src<T, true>(i >= i_start && i < i_start + ns, wct02, wv,
                                                            ss_zf0<T>(zpp, zmp, N, ns, i_start, i, f0), d, mi, ms, att);
      const T ed = exp(-d / mi), es = exp(-ts / mi);
      // (Z_dot F0) at this row for the slots of the chunk that have one (the first p_zdot: the aerosols'; gas slots have none):
      // the component products (Zc[c] F0)_row do not depend on the slot, so c is the outer loop
      T zpd[SS_PC], zmd[SS_PC];
#pragma unroll
      for (int k = 0; k < SS_PC; ++k) zpd[k] = zmd[k] = T(0);
      if constexpr (ZD) {
        if (ly.zdcoef && p0 < p_zdot) {
          const T* cf = ly.zdcoef + (long long)CT * (long long)p_layer * s;
          for (int c = 0; c < CT; ++c) {
            const ss_pair<T> zc = ss_zf0<T>(Zc_pp + c * NN, Zc_mp + c * NN, N, ns, i_start, i, f0);
#pragma unroll
            for (int k = 0; k < SS_PC; ++k) {
              const int p = p0 + k;
              const T a = (p < p_hi && p < p_zdot) ? cf[c + (long long)CT * p] : T(0);
              zpd[k] += a * zc.p;
              zmd[k] += a * zc.m;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < SS_PC; ++k) {
        const int p = p0 + k;
        if (p >= p_hi || p >= p_layer) continue;
        const T beam = -tsd[k] / ms;
        const T ajp = e.jp_tau * td[k] + e.jp_w * wd[k] + e.jp_Z * zpd[k] + e.jp * beam;
        const T ajm = e.jm_tau * td[k] + e.jm_w * wd[k] + e.jm_Z * zmd[k] + e.jm * beam;
        if (iz == 0) {   // rt_kernel_ss.jl:213-216: the TOA layer is copied
          Dp[j][k] = ajp;
          Dm[j][k] = ajm;
        } else {         // get_interaction_ss! (interaction_ss.jl:17-18), differentiated
          Dp[j][k] = (Dp[j][k] - Jp[j] * td[k] / mi) * ed + ajp;
          Dm[j][k] = Dm[j][k] + (ajm - e.jm * tsd[k] / mi) * es;
        }
      }
      Jp[j] = (iz == 0) ? e.jp : Jp[j] * ed + e.jp;
    }
  }
  // the surface layer: the same update with tau = 0 and tau_sum = tau_sum_all[:, Nz + 1]; j0-+' of all P slots from the linearized
  // surface builder, whose own j0- multiplies tau_sum'; the forward builder's j0+ (the direct beam, ~ exp(-tau_sum / mu_0))
  // contributes -j0+ tau_sum' / mu_0
  const T tss = ts_surf[s];
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    if (!rw.on[j]) continue;
    const int e = blockIdx.y * SS_RB + j;
    const long long src = s * N + rw.i[j];
    const T mi = mu[rw.i[j]];
    const T es = exp(-tss / mi);
    const T bp = sj_p ? sj_p[src] : T(0), bm = sj_m[src];
#pragma unroll
    for (int k = 0; k < SS_PC; ++k) {
      const int p = p0 + k;
      if (p >= p_hi) continue;
      const T tsd = (p < p_layer) ? tsd_surf[s + (long long)S * p] : T(0);
      const long long sp = (long long)N * S * p + src;
      const T dp = Dp[j][k] + (sjd_p[sp] - bp * tsd / ms);
      const T dm = Dm[j][k] + (sjd_m[sp] - bm * tsd / mi) * es;
      const long long dst = ss_view_index(s, ns, nV, e, p, S);
      Rd[dst] += w[e] * dm;
      Td[dst] += w[e] * dp;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Raman column, linearized
// ---------------------------------------------------------------------------------------------------------------------
// The partial derivatives of the two line sources of k_ss_column_rrs in (d0, d1) = (tau[n0], tau[n1]).  With u = d0 / mu_0,
// v = d1 / mu_i, psi(x) = (1 - e^-x) / x and phi(u, v) = (e^-v - e^-u) / (u - v) the forward statements are
//   j+ = c+ g0 G,  G = (e^-v - e^-u) / (mu_i / mu_0 - d1 / d0) = (d0 / mu_i) phi(u, v)
//   j- = c- g0 H,  H = (1 - e^-(u + v)) / (mu_i / mu_0 + d1 / d0) = (d0 / mu_i) psi(u + v)
// (the SZA rows are mu_i = mu_0), so that
//   G_d0 = (phi + u phi_u) / mu_i,        G_d1 = (d0 / mu_i^2) phi_v,      phi_v = -phi - phi_u
//   H_d0 = (psi + u psi') / mu_i,         H_d1 = (d0 / mu_i^2) psi'        (psi, psi' at u + v).
// phi = e^-v psi(t) = e^-u psi(-t) with t = u - v, and phi_u = e^-v psi'(t) = -phi - e^-u psi'(-t): psi and psi' are taken at
// |t| from the side that cannot overflow, as expdiff_neg does.  Written as quotients of the regular expression the partials
// cancel like eps / (u - v)^2; psi' below does not.  In the close branches of the forward kernel (its tests, on d0 - d1 and on
// mu_i / mu_0 - d1 / d0: u = v) G = (d0 / mu_i) e^-u, and the partials are the limits phi = e^-u, phi_u = phi_v = -e^-u / 2:
//   G_d0 = e^-u / mu_i (1 - d0 / (2 mu_0)),   G_d1 = -d0 e^-u / (2 mu_i^2);
// the close value is NOT differentiated as a function of d0 alone.
template <typename T>
struct ss_rrs_partials {
  T G, G0, G1, H, H0, H1;
};
// psi'(x) = (x e^-x - (1 - e^-x)) / x^2 for x >= 0, em = expm1(-x), ix = 1 / x: the closed form cancels like eps / x^2, so below
// 1/8 the series sum_j (-1)^(j+1) (j + 1) / (j + 2)! x^j (11 terms: 2e-17 at 1/8)
template <typename T>
__device__ __forceinline__ T ss_psi1(T x, T em, T ix) {
  if (x < T(0.125)) {
    T p = T(-1.0 / 43545600.0);
    p = p * x + T(1.0 / 3991680.0);
    p = p * x - T(1.0 / 403200.0);
    p = p * x + T(1.0 / 45360.0);
    p = p * x - T(1.0 / 5760.0);
    p = p * x + T(1.0 / 840.0);
    p = p * x - T(1.0 / 144.0);
    p = p * x + T(1.0 / 30.0);
    p = p * x - T(0.125);
    p = p * x + T(1.0 / 3.0);
    return p * x - T(0.5);
  }
  return (x * (T(1) + em) + em) * ix * ix;
}
// (ratio = d1 / d0 once per line; imi = 1 / mu_i and ims = 1 / mu_0 once per thread: two divisions are left per line and row)
template <typename T>
__device__ __forceinline__ ss_rrs_partials<T> ss_rrs_line(bool sun, T d0, T d1, T ratio, T x0, T e0, T a0, T x1, T e1, T a1, T imi,
                                                          T ims, T rm) {
  ss_rrs_partials<T> r;
  const T c = d0 * imi;
  const bool close = sun ? !(fabs(d0 - d1) > ss_tol<T>::close()) : (fabs(rm - ratio) < ss_tol<T>::close());
  if (close) {
    r.G = c * e0;
    r.G0 = e0 * imi * (T(1) - T(0.5) * x0);
    r.G1 = -T(0.5) * c * imi * e0;
  } else {
    const T t = x0 - x1, at = fabs(t);
    const T em = expm1(-at), it = T(1) / at;
    const T psi = (at == T(0)) ? T(1) : -em * it;
    const T p1 = ss_psi1<T>(at, em, it);
    const T phi = (t > T(0) ? e1 : e0) * psi;
    const T phi_u = (t > T(0)) ? e1 * p1 : -phi - e0 * p1;
    r.G = c * phi;
    r.G0 = imi * (phi + x0 * phi_u);
    r.G1 = -c * imi * (phi + phi_u);
  }
  const T sm = x0 + x1;
  const T A = -(a1 + a0 + a1 * a0), is = T(1) / sm;   // 1 - exp(-(x1 + x0)) = -(a1 + a0 + a1 a0) with a = expm1(-x)
  const T psi = (sm == T(0)) ? T(1) : A * is;
  const T p1 = ss_psi1<T>(sm, -A, is);
  r.H = c * psi;
  r.H0 = imi * (psi + x0 * p1);
  r.H1 = c * imi * p1;
  return r;
}

// The derivative of k_ss_column_rrs for the slots [p_lo + SS_RPC blockIdx.z, +SS_RPC) below min(p_hi, p_layer).  The run's
// parameters reach a (recipient n1, line, donor n0) source through d0, d1 and g0 = fscatt[n0] exp(-tau_sum[n0] / mu_0) only
// (varpi_ie, Z_ie, F0, the layers' varpi and the surface do not enter), so per slot the donor side is TWO more staged values per
// (window point, layer): d0' and g0' = fscatt' att - g0 tau_sum' / mu_0.  The forward factors are formed again; the interaction is differentiated on
// the running line sums before their update:
//   S+' = (S+' - S+ tau'[n1] / mu_i) e1 + s+',    S-' += (s-' - s- tau_sum'[n1] / mu_i) exp(-tau_sum[n1] / mu_i).
template <typename T>
__global__ __launch_bounds__(SS_TB) void k_ss_column_rrs_lin(int N, int ns, int S, int L, int K, int m, int i_mu0, int halo,
                                                             int p_layer, int p_lo, int p_hi,
                                                             const ss_layer_rrs_lin<T>* __restrict__ lay,
                                                             const int* __restrict__ shift, const T* __restrict__ varpi_ie,
                                                             const T* __restrict__ Zpp, const T* __restrict__ Zmp,
                                                             const T* __restrict__ F0, const T* __restrict__ mu, int nV,
                                                             const int* __restrict__ row0, const T* __restrict__ w, T* ieRd,
                                                             T* ieTd) {
  extern __shared__ __align__(16) unsigned char ss_smem[];
  const ss_window<T, true> win(ss_smem, halo);
  const int W = win.W;
  T *sd = win.sd, *se0 = win.se0, *sa0 = win.sa0, *sg = win.sg, *szp = win.szp, *szm = win.szm, *sdd = win.sdd, *sgd = win.sgd;
  const long long w0 = win.w0, n1 = (long long)blockIdx.x * SS_TB + threadIdx.x;   // n1: the thread's recipient
  const bool live = n1 < S;
  const int i_start = ns * i_mu0;
  const int p0 = p_lo + (int)blockIdx.z * SS_RPC;
  const int p_end = p_hi < p_layer ? p_hi : p_layer;
  const ss_rows<T> rw = ss_pick_rows<T>(true, N, ns, nV, row0, mu, blockIdx.y * SS_RB);
  const T ms = mu[i_start];
  const T wct02 = (m == 0) ? T(0.5) : T(0.25);
  for (int p = threadIdx.x; p < W; p += SS_TB) {   // Z_ie F0 of the thread's rows at every window point, once per workgroup
    const long long n0 = w0 + p;
    const bool in = n0 >= 0 && n0 < S;
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      T zp = 0, zm = 0;
      if (in && rw.on[j])
        for (int q = 0; q < ns; ++q) {
          const long long zo = rw.i[j] + (long long)N * (i_start + q);
          const T f = F0[q + (long long)ns * n0];
          zp += Zpp[zo] * f;
          zm += Zmp[zo] * f;
        }
      szp[j * W + p] = zp;
      szm[j * W + p] = zm;
    }
  }
  T rm[SS_RB], imi[SS_RB], Sp[SS_RB], Dp[SS_RB][SS_RPC], Dm[SS_RB][SS_RPC];
  bool sun[SS_RB];
  const T ims = T(1) / ms;
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    rm[j] = rw.mi[j] / ms;
    imi[j] = T(1) / rw.mi[j];
    sun[j] = rw.i[j] >= i_start && rw.i[j] < i_start + ns;
    Sp[j] = T(0);
#pragma unroll
    for (int k = 0; k < SS_RPC; ++k) Dp[j][k] = Dm[j][k] = T(0);
  }
  for (int iz = 0; iz < L; ++iz) {
    const ss_layer_rrs_lin<T> ly = lay[iz];
    __syncthreads();   // the previous layer's readers are done (first pass: nothing to wait for but the Z F0 stage)
    for (int p = threadIdx.x; p < W; p += SS_TB) {   // the donor factors of this layer and their derivatives at every window point
      const long long n0 = w0 + p;
      T d0 = T(1), e0 = T(0), a0 = T(0), g0 = T(0), dd[SS_RPC], gd[SS_RPC];
#pragma unroll
      for (int k = 0; k < SS_RPC; ++k) dd[k] = gd[k] = T(0);
      if (n0 >= 0 && n0 < S) {
        d0 = ly.tau[n0];
        const T x0 = d0 / ms;
        e0 = exp(-x0);
        a0 = expm1(-x0);
        const T att = exp(-ly.tau_sum[n0] / ms);
        g0 = ly.fscatt[n0] * att;
#pragma unroll
        for (int k = 0; k < SS_RPC; ++k)
          if (p0 + k < p_end) {
            const long long o = n0 + (long long)S * (p0 + k);
            dd[k] = ly.tau_dot[o];
            gd[k] = ly.fscatt_dot[o] * att - g0 * ly.tau_sum_dot[o] / ms;
          }
      }
      sd[p] = d0;
      se0[p] = e0;
      sa0[p] = a0;
      sg[p] = g0;
#pragma unroll
      for (int k = 0; k < SS_RPC; ++k) {
        sdd[k * W + p] = dd[k];
        sgd[k * W + p] = gd[k];
      }
    }
    __syncthreads();
    if (!live) continue;
    const T d1 = ly.tau[n1], ts1 = ly.tau_sum[n1];
    T d1d[SS_RPC], ts1d[SS_RPC];
#pragma unroll
    for (int k = 0; k < SS_RPC; ++k) {
      const bool in = p0 + k < p_end;
      const long long o = n1 + (long long)S * (in ? p0 + k : 0);
      d1d[k] = in ? ly.tau_dot[o] : T(0);
      ts1d[k] = in ? ly.tau_sum_dot[o] : T(0);
    }
    T x1[SS_RB], e1[SS_RB], a1[SS_RB], sp[SS_RB], sm[SS_RB], spd[SS_RB][SS_RPC], smd[SS_RB][SS_RPC];
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      x1[j] = d1 / rw.mi[j];
      e1[j] = exp(-x1[j]);
      a1[j] = expm1(-x1[j]);
      sp[j] = sm[j] = T(0);
#pragma unroll
      for (int k = 0; k < SS_RPC; ++k) spd[j][k] = smd[j][k] = T(0);
    }
    for (int dn = 0; dn < K; ++dn) {
      const long long n0 = n1 + shift[dn];
      if (n0 < 0 || n0 >= S) continue;   // out of band: exactly zero (elemental_inelastic.jl:500)
      const T wl = varpi_ie[dn];
      const long long p = n0 - w0;
      const bool staged = p >= 0 && p < W;
      T d0, e0, a0, g0, dd[SS_RPC], gd[SS_RPC];
      if (staged) {
        d0 = sd[p];
        e0 = se0[p];
        a0 = sa0[p];
        g0 = sg[p];
#pragma unroll
        for (int k = 0; k < SS_RPC; ++k) {
          dd[k] = sdd[k * W + p];
          gd[k] = sgd[k * W + p];
        }
      } else {   // a shift beyond the staged window: the same factors from global memory
        d0 = ly.tau[n0];
        const T x0g = d0 / ms;
        e0 = exp(-x0g);
        a0 = expm1(-x0g);
        const T att = exp(-ly.tau_sum[n0] / ms);
        g0 = ly.fscatt[n0] * att;
#pragma unroll
        for (int k = 0; k < SS_RPC; ++k) {
          dd[k] = gd[k] = T(0);
          if (p0 + k < p_end) {
            const long long o = n0 + (long long)S * (p0 + k);
            dd[k] = ly.tau_dot[o];
            gd[k] = ly.fscatt_dot[o] * att - g0 * ly.tau_sum_dot[o] / ms;
          }
        }
      }
      const T x0 = d0 / ms, ratio = d1 / d0;
#pragma unroll
      for (int j = 0; j < SS_RB; ++j) {
        if (!rw.on[j]) continue;
        T zp, zm;
        if (staged) {
          zp = szp[j * W + p];
          zm = szm[j * W + p];
        } else {
          const ss_pair<T> z = ss_zf0<T>(Zpp, Zmp, N, ns, i_start, rw.i[j], F0 + (long long)ns * n0);
          zp = z.p, zm = z.m;
        }
        const ss_rrs_partials<T> f = ss_rrs_line<T>(sun[j], d0, d1, ratio, x0, e0, a0, x1[j], e1[j], a1[j], imi[j], ims, rm[j]);
        const T cp = wct02 * wl * zp, cm = wct02 * wl * zm;
        sp[j] += cp * g0 * f.G;
        sm[j] += cm * g0 * f.H;
#pragma unroll
        for (int k = 0; k < SS_RPC; ++k) {
          spd[j][k] += cp * (gd[k] * f.G + g0 * (f.G0 * dd[k] + f.G1 * d1d[k]));
          smd[j][k] += cm * (gd[k] * f.H + g0 * (f.H0 * dd[k] + f.H1 * d1d[k]));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SS_RB; ++j) {
      if (iz == 0) {   // rt_kernel_ss.jl:308-314: the TOA layer is copied
#pragma unroll
        for (int k = 0; k < SS_RPC; ++k) {
          Dp[j][k] = spd[j][k];
          Dm[j][k] = smd[j][k];
        }
        Sp[j] = sp[j];
      } else {         // get_interaction_ss_RRS! (interaction_ss.jl:87-88) on the line sums, differentiated
        const T es = exp(-ts1 / rw.mi[j]);
#pragma unroll
        for (int k = 0; k < SS_RPC; ++k) {
          Dp[j][k] = (Dp[j][k] - Sp[j] * d1d[k] * imi[j]) * e1[j] + spd[j][k];
          Dm[j][k] = Dm[j][k] + (smd[j][k] - sm[j] * ts1d[k] * imi[j]) * es;
        }
        Sp[j] = Sp[j] * e1[j] + sp[j];
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    if (!rw.on[j]) continue;
    const int e = blockIdx.y * SS_RB + j;
#pragma unroll
    for (int k = 0; k < SS_RPC; ++k) {
      const int p = p0 + k;
      if (p >= p_end) continue;
      const long long dst = ss_view_index(n1, ns, nV, e, p, S);
      ieRd[dst] += w[e] * Dm[j][k];
      ieTd[dst] += w[e] * Dp[j][k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, typename Q>
static int ss_check_common(const char* who, const Q* q, int S, int L, int nV, const int* row0_h, const T* w_h) {
  VSM_REQUIRE(q && q->mu && q->wt, "%s: null quad", who);
  VSM_REQUIRE(q->N > 0 && q->n_stokes >= 1 && q->n_stokes <= 4 && q->N % q->n_stokes == 0 && q->i_mu0 >= 0 &&
                  (q->i_mu0 + 1) * q->n_stokes <= q->N,
              "%s: bad quad", who);
  VSM_REQUIRE(S >= 0 && L >= 1, "%s: S >= 0 and L >= 1 required (S = %d, L = %d)", who, S, L);
  VSM_REQUIRE(nV >= 1 && row0_h && w_h, "%s: nV >= 1 viewing rows and their tables required", who);
  VSM_REQUIRE((long long)nV * q->n_stokes <= 65535LL * SS_RB, "%s: too many viewing rows (%d)", who, nV);
  for (int v = 0; v < nV; ++v)
    VSM_REQUIRE(row0_h[v] >= 0 && row0_h[v] + q->n_stokes <= q->N, "%s: row0[%d] = %d out of range", who, v, row0_h[v]);
  return VSM_OK;
}
// The per-layer tables a call requires (what: "layer" or "derivative"): each is there (iz < 0; a call's first checks) or has its
// entry of layer iz (where the call builds that layer's struct, so that the checks keep their order).
template <typename T>
using ss_tabs = std::initializer_list<const T* const*>;
template <typename T>
static int ss_check_layers(const char* who, const char* what, ss_tabs<T> tabs, int iz = -1) {
  for (const T* const* t : tabs) {
    if (iz < 0) VSM_REQUIRE(t, "%s: null %s table", who, what);
    else VSM_REQUIRE(t[iz], "%s: null entry in %s table %d", who, what, iz);
  }
  return VSM_OK;
}
// the slot arguments of a derivative column whose threads carry PC slots each (grid.z: the chunks of [p_lo, p_hi)); p_zdot: the
// elastic column's
static int ss_check_slots(const char* who, int P, int p_layer, int p_lo, int p_hi, int PC, int p_zdot = 0) {
  VSM_REQUIRE(P >= 1 && p_layer >= 0 && p_layer <= P, "%s: P >= 1 and 0 <= p_layer <= P required (P = %d, p_layer = %d)", who, P,
              p_layer);
  VSM_REQUIRE(p_zdot >= 0 && p_zdot <= p_layer, "%s: 0 <= p_zdot <= p_layer required (p_zdot = %d)", who, p_zdot);
  VSM_REQUIRE(p_lo >= 0 && p_lo < p_hi && p_hi <= P, "%s: slot range [%d, %d) outside [0, %d)", who, p_lo, p_hi, P);
  VSM_REQUIRE((p_hi - p_lo + PC - 1) / PC <= 65535, "%s: too many slots", who);
  return VSM_OK;
}
// What a launch needs beside the caller's arrays: the device tables of the call -- its layer structs, w[nV n_stokes], row0[nV],
// one packed_image in the scratch of SS_SLOT --, grid.x and grid.y over the `items` rows of a point and, for the Raman columns
// (halo >= 0, `bytes` of their ss_window), the clamped halo with the LDS bytes of its window.
static_assert(ss_window<double, true>::bytes(VSM_SS_MAX_HALO) <= 65536, "k_ss_column_rrs_lin: a workgroup stays within 64 KB of LDS");
template <typename T, typename LAY>
struct ss_launch {
  hipStream_t st;
  const LAY* lay;   // the three device tables
  const T* w;
  const int* row0;
  unsigned gx, gv;
  int halo;
  size_t lds;
  int prepare(const std::vector<LAY>& lay_h, int S, int items, int nV, const int* row0_h, const T* w_h, void* stream, int halo_ = -1,
              size_t (*bytes)(int) = nullptr) {
    st = as_stream(stream);
    packed_image img;
    const size_t o_l = img.add(lay_h.data(), sizeof(LAY) * lay_h.size()), o_w = img.add(w_h, sizeof(T) * (size_t)items);
    const size_t o_r = img.add(row0_h, sizeof(int) * (size_t)nV);
    unsigned char* d;
    if (int rc = upload_image(img, SS_SLOT, st, &d)) return rc;
    lay = reinterpret_cast<const LAY*>(d + o_l);
    w = reinterpret_cast<const T*>(d + o_w);
    row0 = reinterpret_cast<const int*>(d + o_r);
    gx = (unsigned)((S + SS_TB - 1) / SS_TB);
    gv = (unsigned)((items + SS_RB - 1) / SS_RB);
    halo = halo_ > VSM_SS_MAX_HALO ? VSM_SS_MAX_HALO : halo_;
    lds = bytes ? bytes(halo) : 0;
    return VSM_OK;
  }
};

template <typename T, typename Q>
static int ss_column(const Q* q, int S, int L, int m, const T* const* tau_h, const T* const* varpi_h, const T* const* tau_sum_h,
                     const T* const* Zpp_h, const T* const* Zmp_h, const long long* zs_h, const T* F0, const T* sj_m, const T* sj_p,
                     const T* ts_surf, int nV, const int* row0_h, const T* w_h, T* R, T* Tt, T* J0_m, T* J0_p, void* stream) {
  int rc;
  if ((rc = ss_check_common<T>("ss_column", q, S, L, nV, row0_h, w_h))) return rc;
  const ss_tabs<T> tabs = {tau_h, varpi_h, tau_sum_h, Zpp_h, Zmp_h};
  if ((rc = ss_check_layers<T>("ss_column", "layer", tabs))) return rc;
  VSM_REQUIRE(zs_h, "ss_column: null layer table");
  VSM_REQUIRE(F0 && sj_m && ts_surf && R && Tt, "ss_column: null argument");
  VSM_REQUIRE((J0_m == nullptr) == (J0_p == nullptr), "ss_column: J0_m and J0_p go together");
  VSM_REQUIRE(m >= 0, "ss_column: m >= 0");
  std::vector<ss_layer<T>> lay((size_t)L);
  for (int iz = 0; iz < L; ++iz) {
    if ((rc = ss_check_layers<T>("ss_column", "layer", tabs, iz))) return rc;
    VSM_REQUIRE(zs_h[iz] == 0 || zs_h[iz] == (long long)q->N * q->N, "ss_column: z_stride[%d] must be 0 or N*N", iz);
    lay[iz] = ss_layer<T>{tau_h[iz], varpi_h[iz], tau_sum_h[iz], Zpp_h[iz], Zmp_h[iz], nullptr, zs_h[iz]};
  }
  if (S == 0) return VSM_OK;
  ss_launch<T, ss_layer<T>> g;
  if ((rc = g.prepare(lay, S, nV * q->n_stokes, nV, row0_h, w_h, stream))) return rc;
  hipLaunchKernelGGL((k_ss_column<T, true>), dim3(g.gx, g.gv), dim3(SS_TB), 0, g.st, q->N, q->n_stokes, S, L, m, q->i_mu0, g.lay, F0,
                     sj_m, sj_p, ts_surf, q->mu, nV, g.row0, g.w, R, Tt);
  VSM_LAUNCH_CHECK("k_ss_column");
  if (J0_m) {
    hipLaunchKernelGGL((k_ss_column<T, false>), dim3(g.gx, (unsigned)((q->N + SS_RB - 1) / SS_RB)), dim3(SS_TB), 0, g.st, q->N, q->n_stokes, S,
                       L, m, q->i_mu0, g.lay, F0, sj_m, sj_p, ts_surf, q->mu, nV, g.row0, g.w, J0_m, J0_p);
    VSM_LAUNCH_CHECK("k_ss_column (all streams)");
  }
  return VSM_OK;
}

template <typename T, typename Q>
static int ss_column_lin(const Q* q, int S, int L, int m, int P, int p_layer, int p_zdot, int p_lo, int p_hi, const T* const* tau_h,
                         const T* const* varpi_h, const T* const* tau_sum_h, const T* const* Zpp_h, const T* const* Zmp_h,
                         const long long* zs_h, const T* const* tau_dot_h, const T* const* varpi_dot_h,
                         const T* const* tau_sum_dot_h, const T* const* zdcoef_h, int CT, const T* Zc_pp, const T* Zc_mp,
                         const T* F0, const T* sj_m, const T* sj_p, const T* sjd_m, const T* sjd_p, const T* ts_surf,
                         const T* tsd_surf, int nV, const int* row0_h, const T* w_h, T* Rd, T* Td, void* stream) {
  int rc;
  if ((rc = ss_check_common<T>("ss_column_lin", q, S, L, nV, row0_h, w_h))) return rc;
  if ((rc = ss_check_slots("ss_column_lin", P, p_layer, p_lo, p_hi, SS_PC, p_zdot))) return rc;
  const ss_tabs<T> tabs = {tau_h, varpi_h, tau_sum_h, Zpp_h, Zmp_h}, dots = {tau_dot_h, varpi_dot_h, tau_sum_dot_h};
  if ((rc = ss_check_layers<T>("ss_column_lin", "layer", tabs))) return rc;
  VSM_REQUIRE(zs_h, "ss_column_lin: null layer table");
  if (p_layer && (rc = ss_check_layers<T>("ss_column_lin", "derivative", dots))) return rc;
  VSM_REQUIRE(p_layer == 0 || tsd_surf, "ss_column_lin: null derivative table");
  VSM_REQUIRE(F0 && sj_m && sjd_m && sjd_p && ts_surf && Rd && Td, "ss_column_lin: null argument");
  VSM_REQUIRE(m >= 0 && CT >= 0, "ss_column_lin: m >= 0 and CT >= 0");
  std::vector<ss_layer_lin<T>> lay((size_t)L);
  bool any_zd = false;
  for (int iz = 0; iz < L; ++iz) {
    if ((rc = ss_check_layers<T>("ss_column_lin", "layer", tabs, iz))) return rc;
    if (p_layer && (rc = ss_check_layers<T>("ss_column_lin", "derivative", dots, iz))) return rc;
    VSM_REQUIRE(zs_h[iz] == 0 || zs_h[iz] == (long long)q->N * q->N, "ss_column_lin: z_stride[%d] must be 0 or N*N", iz);
    const T* zc = (zdcoef_h && p_zdot > 0) ? zdcoef_h[iz] : nullptr;
    any_zd = any_zd || zc;
    VSM_REQUIRE(!zc || (CT >= 1 && Zc_pp && Zc_mp), "ss_column_lin: Z_dot coefficients without component blocks (layer %d)", iz);
    lay[iz] = ss_layer_lin<T>{tau_h[iz], varpi_h[iz], tau_sum_h[iz], Zpp_h[iz], Zmp_h[iz],
                              p_layer ? tau_dot_h[iz] : nullptr, p_layer ? varpi_dot_h[iz] : nullptr,
                              p_layer ? tau_sum_dot_h[iz] : nullptr, zc, zs_h[iz]};
  }
  if (S == 0) return VSM_OK;
  ss_launch<T, ss_layer_lin<T>> g;
  if ((rc = g.prepare(lay, S, nV * q->n_stokes, nV, row0_h, w_h, stream))) return rc;
  const unsigned gp = (unsigned)((p_hi - p_lo + SS_PC - 1) / SS_PC);
  if (any_zd)
    hipLaunchKernelGGL((k_ss_column_lin<T, true>), dim3(g.gx, g.gv, gp), dim3(SS_TB), 0, g.st, q->N, q->n_stokes, S, L, m, q->i_mu0, P,
                       p_layer, p_zdot, p_lo, p_hi, g.lay, CT, Zc_pp, Zc_mp, F0, sj_m, sj_p, sjd_m, sjd_p, ts_surf, tsd_surf, q->mu,
                       nV, g.row0, g.w, Rd, Td);
  else
    hipLaunchKernelGGL((k_ss_column_lin<T, false>), dim3(g.gx, g.gv, gp), dim3(SS_TB), 0, g.st, q->N, q->n_stokes, S, L, m, q->i_mu0, P,
                       p_layer, 0, p_lo, p_hi, g.lay, 0, (const T*)nullptr, (const T*)nullptr, F0, sj_m, sj_p, sjd_m, sjd_p, ts_surf,
                       tsd_surf, q->mu, nV, g.row0, g.w, Rd, Td);
  VSM_LAUNCH_CHECK("k_ss_column_lin");
  return VSM_OK;
}

template <typename T, typename Q>
static int ss_column_rrs(const Q* q, int S, int L, int m, int K, const T* const* tau_h, const T* const* tau_sum_h,
                         const T* const* fscatt_h, const int* shift, const T* varpi_ie, const T* Zpp_ie, const T* Zmp_ie,
                         const T* F0, int halo, int nV, const int* row0_h, const T* w_h, T* ieR, T* ieT, void* stream) {
  int rc;
  if ((rc = ss_check_common<T>("ss_column_rrs", q, S, L, nV, row0_h, w_h))) return rc;
  VSM_REQUIRE(K >= 0, "ss_column_rrs: K >= 0 required (K = %d)", K);
  const ss_tabs<T> tabs = {tau_h, tau_sum_h, fscatt_h};
  if ((rc = ss_check_layers<T>("ss_column_rrs", "layer", tabs))) return rc;
  VSM_REQUIRE(F0 && ieR && ieT && Zpp_ie && Zmp_ie, "ss_column_rrs: null argument");
  VSM_REQUIRE(K == 0 || (shift && varpi_ie), "ss_column_rrs: null line table");
  VSM_REQUIRE(m >= 0 && halo >= 0, "ss_column_rrs: m >= 0 and halo >= 0");
  std::vector<ss_layer<T>> lay((size_t)L);
  for (int iz = 0; iz < L; ++iz) {
    if ((rc = ss_check_layers<T>("ss_column_rrs", "layer", tabs, iz))) return rc;
    lay[iz] = ss_layer<T>{tau_h[iz], nullptr, tau_sum_h[iz], nullptr, nullptr, fscatt_h[iz], 0};
  }
  if (S == 0 || K == 0) return VSM_OK;
  ss_launch<T, ss_layer<T>> g;
  if ((rc = g.prepare(lay, S, nV * q->n_stokes, nV, row0_h, w_h, stream, halo, ss_window<T, false>::bytes))) return rc;
  hipLaunchKernelGGL(k_ss_column_rrs<T>, dim3(g.gx, g.gv), dim3(SS_TB), g.lds, g.st, q->N, q->n_stokes, S, L, K, m, q->i_mu0, g.halo,
                     g.lay, shift, varpi_ie, Zpp_ie, Zmp_ie, F0, q->mu, nV, g.row0, g.w, ieR, ieT);
  VSM_LAUNCH_CHECK("k_ss_column_rrs");
  return VSM_OK;
}

template <typename T, typename Q>
static int ss_column_rrs_lin(const Q* q, int S, int L, int m, int K, int P, int p_layer, int p_lo, int p_hi, const T* const* tau_h,
                             const T* const* tau_sum_h, const T* const* fscatt_h, const T* const* tau_dot_h,
                             const T* const* tau_sum_dot_h, const T* const* fscatt_dot_h, const int* shift, const T* varpi_ie,
                             const T* Zpp_ie, const T* Zmp_ie, const T* F0, int halo, int nV, const int* row0_h, const T* w_h,
                             T* ieRd, T* ieTd, void* stream) {
  int rc;
  if ((rc = ss_check_common<T>("ss_column_rrs_lin", q, S, L, nV, row0_h, w_h))) return rc;
  VSM_REQUIRE(K >= 0, "ss_column_rrs_lin: K >= 0 required (K = %d)", K);
  if ((rc = ss_check_slots("ss_column_rrs_lin", P, p_layer, p_lo, p_hi, SS_RPC))) return rc;
  const ss_tabs<T> tabs = {tau_h, tau_sum_h, fscatt_h}, dots = {tau_dot_h, tau_sum_dot_h, fscatt_dot_h};
  if ((rc = ss_check_layers<T>("ss_column_rrs_lin", "layer", tabs))) return rc;
  if (p_layer && (rc = ss_check_layers<T>("ss_column_rrs_lin", "derivative", dots))) return rc;
  VSM_REQUIRE(F0 && ieRd && ieTd && Zpp_ie && Zmp_ie, "ss_column_rrs_lin: null argument");
  VSM_REQUIRE(K == 0 || (shift && varpi_ie), "ss_column_rrs_lin: null line table");
  VSM_REQUIRE(m >= 0 && halo >= 0, "ss_column_rrs_lin: m >= 0 and halo >= 0");
  std::vector<ss_layer_rrs_lin<T>> lay((size_t)L);
  for (int iz = 0; iz < L; ++iz) {
    if ((rc = ss_check_layers<T>("ss_column_rrs_lin", "layer", tabs, iz))) return rc;
    if (p_layer && (rc = ss_check_layers<T>("ss_column_rrs_lin", "derivative", dots, iz))) return rc;
    lay[iz] = ss_layer_rrs_lin<T>{tau_h[iz], tau_sum_h[iz], fscatt_h[iz], p_layer ? tau_dot_h[iz] : nullptr,
                                  p_layer ? tau_sum_dot_h[iz] : nullptr, p_layer ? fscatt_dot_h[iz] : nullptr};
  }
  const int p_end = p_hi < p_layer ? p_hi : p_layer;   // the surface's slots (and any later ones) are exact zeros: not touched
  if (S == 0 || K == 0 || p_lo >= p_end) return VSM_OK;
  ss_launch<T, ss_layer_rrs_lin<T>> g;
  if ((rc = g.prepare(lay, S, nV * q->n_stokes, nV, row0_h, w_h, stream, halo, ss_window<T, true>::bytes))) return rc;
  const unsigned gp = (unsigned)((p_end - p_lo + SS_RPC - 1) / SS_RPC);
  hipLaunchKernelGGL(k_ss_column_rrs_lin<T>, dim3(g.gx, g.gv, gp), dim3(SS_TB), g.lds, g.st, q->N, q->n_stokes, S, L, K, m, q->i_mu0,
                     g.halo, p_layer, p_lo, p_hi, g.lay, shift, varpi_ie, Zpp_ie, Zmp_ie, F0, q->mu, nV, g.row0, g.w, ieRd, ieTd);
  VSM_LAUNCH_CHECK("k_ss_column_rrs_lin");
  return VSM_OK;
}

}  // namespace vsm

using namespace vsm;

extern "C" {

#define VSM_SS_API(T, SFX)                                                                                                     \
  int vsm_ss_column_##SFX(const vsm_quad_##SFX* q, int S, int L, int m, const T* const* tau_h, const T* const* varpi_h,        \
                          const T* const* tau_sum_h, const T* const* Zpp_h, const T* const* Zmp_h, const long long* z_stride_h, \
                          const T* F0, const T* surf_j0_m, const T* surf_j0_p, const T* tau_sum_surface, int nV,               \
                          const int* row0_h, const T* w_h, T* R_SFI, T* T_SFI, T* J0_m, T* J0_p, void* stream) {               \
    return ss_column<T>(q, S, L, m, tau_h, varpi_h, tau_sum_h, Zpp_h, Zmp_h, z_stride_h, F0, surf_j0_m, surf_j0_p,             \
                        tau_sum_surface, nV, row0_h, w_h, R_SFI, T_SFI, J0_m, J0_p, stream);                                   \
  }                                                                                                                            \
  int vsm_ss_column_rrs_##SFX(const vsm_quad_##SFX* q, int S, int L, int m, int K, const T* const* tau_h,                      \
                              const T* const* tau_sum_h, const T* const* fscatt_h, const int* shift, const T* varpi_ie,        \
                              const T* Zpp_ie, const T* Zmp_ie, const T* F0, int halo, int nV, const int* row0_h,              \
                              const T* w_h, T* ieR_SFI, T* ieT_SFI, void* stream) {                                            \
    return ss_column_rrs<T>(q, S, L, m, K, tau_h, tau_sum_h, fscatt_h, shift, varpi_ie, Zpp_ie, Zmp_ie, F0, halo, nV, row0_h,  \
                            w_h, ieR_SFI, ieT_SFI, stream);                                                                    \
  }                                                                                                                            \
  int vsm_ss_column_lin_##SFX(const vsm_quad_##SFX* q, int S, int L, int m, int P, int p_layer, int p_zdot, int p_lo,          \
                              int p_hi,                                                                                        \
                              const T* const* tau_h, const T* const* varpi_h, const T* const* tau_sum_h,                       \
                              const T* const* Zpp_h, const T* const* Zmp_h, const long long* z_stride_h,                       \
                              const T* const* tau_dot_h, const T* const* varpi_dot_h, const T* const* tau_sum_dot_h,           \
                              const T* const* zdcoef_h, int CT, const T* Zc_pp, const T* Zc_mp, const T* F0,                   \
                              const T* surf_j0_m, const T* surf_j0_p, const T* surf_j0_m_lin, const T* surf_j0_p_lin,          \
                              const T* tau_sum_surface, const T* tau_sum_dot_surface, int nV, const int* row0_h,               \
                              const T* w_h, T* Rdot, T* Tdot, void* stream) {                                                  \
    return ss_column_lin<T>(q, S, L, m, P, p_layer, p_zdot, p_lo, p_hi, tau_h, varpi_h, tau_sum_h, Zpp_h, Zmp_h, z_stride_h,   \
                            tau_dot_h, varpi_dot_h, tau_sum_dot_h, zdcoef_h, CT, Zc_pp, Zc_mp, F0, surf_j0_m, surf_j0_p,       \
                            surf_j0_m_lin, surf_j0_p_lin, tau_sum_surface, tau_sum_dot_surface, nV, row0_h, w_h, Rdot, Tdot,   \
                            stream);                                                                                           \
  }                                                                                                                            \
  int vsm_ss_column_rrs_lin_##SFX(const vsm_quad_##SFX* q, int S, int L, int m, int K, int P, int p_layer, int p_lo, int p_hi, \
                                  const T* const* tau_h, const T* const* tau_sum_h, const T* const* fscatt_h,                  \
                                  const T* const* tau_dot_h, const T* const* tau_sum_dot_h, const T* const* fscatt_dot_h,      \
                                  const int* shift, const T* varpi_ie, const T* Zpp_ie, const T* Zmp_ie, const T* F0,          \
                                  int halo, int nV, const int* row0_h, const T* w_h, T* ieRdot, T* ieTdot, void* stream) {     \
    return ss_column_rrs_lin<T>(q, S, L, m, K, P, p_layer, p_lo, p_hi, tau_h, tau_sum_h, fscatt_h, tau_dot_h, tau_sum_dot_h,   \
                                fscatt_dot_h, shift, varpi_ie, Zpp_ie, Zmp_ie, F0, halo, nV, row0_h, w_h, ieRdot, ieTdot,      \
                                stream);                                                                                       \
  }
VSM_SS_API(double, f64)
VSM_SS_API(float, f32)

}  // extern "C"
