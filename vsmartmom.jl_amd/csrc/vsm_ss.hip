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
#include <string.h>

#include <vector>

#include "vsm_common.h"
#include "vsm_internal.h"

namespace vsm {

constexpr int SS_TB = VSM_SS_BLOCK;   // spectral points (= threads) per workgroup: two waves
constexpr int SS_RB = 4;              // rows per thread; more rows go to further workgroups along grid.y
constexpr int SS_SLOT = 5;            // library scratch slot of the device tables

template <typename T>
struct ss_layer {
  const T *tau, *varpi, *tau_sum, *zpp, *zmp, *fscatt;
  long long zs;
};

template <typename T>
struct ss_tol {
  static __device__ __forceinline__ T close() { return T(1e-8); }   // rt_close_tol (rt_helpers.jl:66-68)
};

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
      T zp = 0, zm = 0;
      for (int q = 0; q < ns; ++q) {
        const long long zo = i + (long long)N * (i_start + q);
        zp += zpp[zo] * f0[q];
        zm += zmp[zo] * f0[q];
      }
      // get_elem_rt_SFI! with dtau = tau, ndoubl = 0 (the statements of k_elemental_sfi, vsm_generic.hip)
      T jp;
      if (i >= i_start && i < i_start + ns)
        jp = wct02 * wv * zp * (d / mi) * exp(-d / mi);
      else
        jp = wct02 * wv * zp * (ms / (mi - ms)) * expdiff_neg<T>(d / mi, d / ms);
      T jm = wct02 * wv * zm * (ms / (mi + ms)) * (-expm1(-d * ((T(1) / mi) + (T(1) / ms))));
      jp *= att;
      jm *= att;
      if (iz == 0) {   // rt_kernel_ss.jl:213-216: the TOA layer is copied
        Jp[j] = jp;
        Jm[j] = jm;
      } else {         // get_interaction_ss! (interaction_ss.jl:17-18)
        Jp[j] = Jp[j] * exp(-d / mi) + jp;
        Jm[j] = Jm[j] + jm * exp(-ts / mi);
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
      const long long dst = (s * ns + e / nV) * nV + e % nV;
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
// What a (recipient, line) pair reads of its donor n0 in one layer: d0 = tau[n0], x0 = d0 / mu0 as e0 = exp(-x0) and
// a0 = expm1(-x0), g0 = fscatt[n0] exp(-tau_sum[n0] / mu0) -- formed once per (point, layer) in LDS for the window of the
// workgroup, not once per line -- and, per row of the thread, Z_ie F0[:, n0] (layer independent: staged once per workgroup).
template <typename T>
__global__ __launch_bounds__(SS_TB) void k_ss_column_rrs(int N, int ns, int S, int L, int K, int m, int i_mu0, int halo,
                                                         const ss_layer<T>* __restrict__ lay, const int* __restrict__ shift,
                                                         const T* __restrict__ varpi_ie, const T* __restrict__ Zpp,
                                                         const T* __restrict__ Zmp, const T* __restrict__ F0,
                                                         const T* __restrict__ mu, int nV, const int* __restrict__ row0,
                                                         const T* __restrict__ w, T* ieR, T* ieT) {
  extern __shared__ __align__(16) unsigned char ss_smem[];
  const int W = SS_TB + 2 * halo;
  T* sd = reinterpret_cast<T*>(ss_smem);   // [W] each
  T* se0 = sd + W;
  T* sa0 = se0 + W;
  T* sg = sa0 + W;
  T* szp = sg + W;                         // [SS_RB][W]
  T* szm = szp + SS_RB * W;
  const long long b0 = (long long)blockIdx.x * SS_TB;
  const long long w0 = b0 - halo;
  const long long n1 = b0 + threadIdx.x;
  const bool live = n1 < S;
  const int i_start = ns * i_mu0;
  const ss_rows<T> rw = ss_pick_rows<T>(true, N, ns, nV, row0, mu, blockIdx.y * SS_RB);
  const T ms = mu[i_start];
  const T wct02 = (m == 0) ? T(0.5) : T(0.25);
  for (int p = threadIdx.x; p < W; p += SS_TB) {
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
    for (int p = threadIdx.x; p < W; p += SS_TB) {
      const long long n0 = w0 + p;
      T d0 = T(1), e0 = T(0), a0 = T(0), g0 = T(0);
      if (n0 >= 0 && n0 < S) {
        d0 = ly.tau[n0];
        const T x0 = d0 / ms;
        e0 = exp(-x0);
        a0 = expm1(-x0);
        g0 = ly.fscatt[n0] * exp(-ly.tau_sum[n0] / ms);
      }
      sd[p] = d0;
      se0[p] = e0;
      sa0[p] = a0;
      sg[p] = g0;
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
        d0 = sd[p];
        e0 = se0[p];
        a0 = sa0[p];
        g0 = sg[p];
      } else {   // a shift beyond the staged window: the same factors from global memory
        d0 = ly.tau[n0];
        const T x0g = d0 / ms;
        e0 = exp(-x0g);
        a0 = expm1(-x0g);
        g0 = ly.fscatt[n0] * exp(-ly.tau_sum[n0] / ms);
      }
      const T x0 = d0 / ms;
      const T ratio = d1 / d0;
#pragma unroll
      for (int j = 0; j < SS_RB; ++j) {
        if (!rw.on[j]) continue;
        T zp, zm;
        if (staged) {
          zp = szp[j * W + p];
          zm = szm[j * W + p];
        } else {
          zp = zm = T(0);
          for (int q = 0; q < ns; ++q) {
            const long long zo = rw.i[j] + (long long)N * (i_start + q);
            const T f = F0[q + (long long)ns * n0];
            zp += Zpp[zo] * f;
            zm += Zmp[zo] * f;
          }
        }
        const T mi = rw.mi[j];
        // expdiff_neg(d1 / mu_i, d0 / mu_0) (rt_helpers.jl:32-40) from e1 = exp(-x1), e0 = exp(-x0): one expm1 is left
        const T xa = x1[j];
        const T ed = (xa == x0) ? T(0) : ((xa < x0) ? e1[j] * (-expm1(-(x0 - xa))) : -e0 * (-expm1(-(xa - x0))));
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
    const long long dst = (n1 * ns + e / nV) * nV + e % nV;
    ieR[dst] += w[e] * Sm[j];
    ieT[dst] += w[e] * Sp[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// elastic column, linearized
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SS_PC = 4;   // parameter slots a thread carries; further slots go to further workgroups along grid.z

template <typename T>
struct ss_layer_lin {
  const T *tau, *varpi, *tau_sum, *zpp, *zmp;
  const T *tau_dot, *varpi_dot, *tau_sum_dot;   // [S, p_layer] each (tau_dot: of the layer's full tau)
  const T* zdcoef;                              // [CT, p_layer, S] or null (Z_dot = 0)
  long long zs;
};

// The derivative of k_ss_column<T, true> for the slots [p_lo + SS_PC blockIdx.z, +SS_PC) below p_hi.  Per layer the forward
// factors of the thread's rows are formed again (they are cheap), the slot loop applies the chain rule of get_elem_rt_SFI_fused!
// (the statements of k_elemental_sfi_lin, vsm_lin.hip) and the derivative of get_interaction_ss!, taken on J0+ BEFORE its update:
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
      const int e = blockIdx.y * SS_RB + j;   // item e = v + nV k of the viewing table (ss_pick_rows, VIEW form)
      if (e >= nV * ns) continue;
      const int i = row0[e % nV] + e / nV;
      const T mi = mu[i];
      T zp = 0, zm = 0;
      for (int q = 0; q < ns; ++q) {
        const long long zo = i + (long long)N * (i_start + q);
        zp += zpp[zo] * f0[q];
        zm += zmp[zo] * f0[q];
      }
      // forward sources and their partial derivatives (k_elemental_sfi_lin with dtau = tau, ndoubl = 0)
      T jp, jp_tau;
      if (i >= i_start && i < i_start + ns) {
        jp = wct02 * wv * zp * (d / mi) * exp(-d / mi);
        jp_tau = jp * (T(1) / d - T(1) / mi);
      } else {
        jp = wct02 * wv * zp * (ms / (mi - ms)) * expdiff_neg<T>(d / mi, d / ms);
        jp_tau = -wct02 * wv * zp * (ms / (mi - ms)) * (exp(-d / mi) / mi - exp(-d / ms) / ms);
      }
      T jp_w = (wv == T(0)) ? T(0) : jp / wv;
      T jp_Z = (zp == T(0)) ? T(0) : jp / zp;
      const T gm = ms / (mi + ms);
      const T arg = d * ((T(1) / mi) + (T(1) / ms));
      T jm = wct02 * wv * zm * gm * (-expm1(-arg));
      T jm_tau = wct02 * wv * zm * gm * exp(-arg) * ((T(1) / mi) + (T(1) / ms));
      T jm_w = (wv == T(0)) ? T(0) : jm / wv;
      T jm_Z = (zm == T(0)) ? T(0) : jm / zm;
      jp *= att; jp_tau *= att; jp_w *= att; jp_Z *= att;
      jm *= att; jm_tau *= att; jm_w *= att; jm_Z *= att;
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
            T cp = 0, cm = 0;
            for (int q = 0; q < ns; ++q) {
              const long long zo = c * NN + i + (long long)N * (i_start + q);
              cp += Zc_pp[zo] * f0[q];
              cm += Zc_mp[zo] * f0[q];
            }
#pragma unroll
            for (int k = 0; k < SS_PC; ++k) {
              const int p = p0 + k;
              const T a = (p < p_hi && p < p_zdot) ? cf[c + (long long)CT * p] : T(0);
              zpd[k] += a * cp;
              zmd[k] += a * cm;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < SS_PC; ++k) {
        const int p = p0 + k;
        if (p >= p_hi || p >= p_layer) continue;
        const T beam = -tsd[k] / ms;
        const T ajp = jp_tau * td[k] + jp_w * wd[k] + jp_Z * zpd[k] + jp * beam;
        const T ajm = jm_tau * td[k] + jm_w * wd[k] + jm_Z * zmd[k] + jm * beam;
        if (iz == 0) {   // rt_kernel_ss.jl:213-216: the TOA layer is copied
          Dp[j][k] = ajp;
          Dm[j][k] = ajm;
        } else {         // get_interaction_ss! (interaction_ss.jl:17-18), differentiated
          Dp[j][k] = (Dp[j][k] - Jp[j] * td[k] / mi) * ed + ajp;
          Dm[j][k] = Dm[j][k] + (ajm - jm * tsd[k] / mi) * es;
        }
      }
      Jp[j] = (iz == 0) ? jp : Jp[j] * ed + jp;
    }
  }
  // the surface layer: the same update with tau = 0 and tau_sum = tau_sum_all[:, Nz + 1]; j0-+' of all P slots from the linearized
  // surface builder, whose own j0- multiplies tau_sum'; the forward builder's j0+ (the direct beam, ~ exp(-tau_sum / mu_0))
  // contributes -j0+ tau_sum' / mu_0
  const T tss = ts_surf[s];
#pragma unroll
  for (int j = 0; j < SS_RB; ++j) {
    const int e = blockIdx.y * SS_RB + j;
    if (e >= nV * ns) continue;
    const int i = row0[e % nV] + e / nV;
    const long long src = s * N + i;
    const T mi = mu[i];
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
      const long long dst = ((((long long)p * S + s) * ns + e / nV) * nV) + e % nV;
      Rd[dst] += w[e] * dm;
      Td[dst] += w[e] * dp;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Raman column, linearized
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SS_RPC = 2;   // parameter slots a thread of the Raman derivative carries: (12 + 2 SS_RPC) staged values per window point
                            // = 64 KB of LDS at FP64 with the maximal halo (the forward kernel's 12 values: 48 KB)

template <typename T>
struct ss_layer_rrs_lin {
  const T *tau, *tau_sum, *fscatt;
  const T *tau_dot, *tau_sum_dot, *fscatt_dot;   // [S, p_layer] each (tau_dot: of the layer's full tau)
};

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
// (window point, layer): d0' and g0' = fscatt'[n0] exp(-tau_sum[n0] / mu_0) - g0 tau_sum'[n0] / mu_0.  The forward factors are
// formed again; the interaction is differentiated on the running line sums before their update:
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
  const int W = SS_TB + 2 * halo;
  T* sd = reinterpret_cast<T*>(ss_smem);   // [W] each
  T* se0 = sd + W;
  T* sa0 = se0 + W;
  T* sg = sa0 + W;
  T* szp = sg + W;                         // [SS_RB][W]
  T* szm = szp + SS_RB * W;
  T* sdd = szm + SS_RB * W;                // [SS_RPC][W]: d0'
  T* sgd = sdd + SS_RPC * W;               // [SS_RPC][W]: g0'
  const long long b0 = (long long)blockIdx.x * SS_TB;
  const long long w0 = b0 - halo;
  const long long n1 = b0 + threadIdx.x;
  const bool live = n1 < S;
  const int i_start = ns * i_mu0;
  const int p0 = p_lo + (int)blockIdx.z * SS_RPC;
  const int p_end = p_hi < p_layer ? p_hi : p_layer;
  const ss_rows<T> rw = ss_pick_rows<T>(true, N, ns, nV, row0, mu, blockIdx.y * SS_RB);
  const T ms = mu[i_start];
  const T wct02 = (m == 0) ? T(0.5) : T(0.25);
  for (int p = threadIdx.x; p < W; p += SS_TB) {
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
    for (int p = threadIdx.x; p < W; p += SS_TB) {
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
          zp = zm = T(0);
          for (int q = 0; q < ns; ++q) {
            const long long zo = rw.i[j] + (long long)N * (i_start + q);
            const T f = F0[q + (long long)ns * n0];
            zp += Zpp[zo] * f;
            zm += Zmp[zo] * f;
          }
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
      const long long dst = ((((long long)p * S + n1) * ns + e / nV) * nV) + e % nV;
      ieRd[dst] += w[e] * Dm[j][k];
      ieTd[dst] += w[e] * Dp[j][k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// Device tables of one call in the library's scratch: ss_layer[L] | w[nV n_stokes] | row0[nV].  One stream-ordered copy of a
// packed host image (pageable memory: staged by the runtime before the call returns), so L and nV are not capped.
template <typename T, typename LAY = ss_layer<T>>
struct ss_tables {
  const LAY* lay;
  const T* w;
  const int* row0;
};
template <typename T, typename LAY>
static int ss_upload(int L, const std::vector<LAY>& lay, int ns, int nV, const int* row0_h, const T* w_h, hipStream_t st,
                     ss_tables<T, LAY>* out) {
  const size_t o_w = sizeof(LAY) * (size_t)L;
  const size_t o_r = o_w + sizeof(T) * (size_t)nV * ns;
  const size_t total = o_r + sizeof(int) * (size_t)nV;
  std::vector<unsigned char> img(total);
  memcpy(img.data(), lay.data(), o_w);
  memcpy(img.data() + o_w, w_h, o_r - o_w);
  memcpy(img.data() + o_r, row0_h, total - o_r);
  unsigned char* dev = static_cast<unsigned char*>(scratch(total, SS_SLOT, st));
  if (!dev) return VSM_ERR_HIP;
  VSM_HIP(hipMemcpyAsync(dev, img.data(), total, hipMemcpyHostToDevice, st));
  VSM_HIP(hipStreamSynchronize(st));   // `img` dies with this frame: the copy (a few hundred bytes, once per moment) must have left it
  out->lay = reinterpret_cast<const LAY*>(dev);
  out->w = reinterpret_cast<const T*>(dev + o_w);
  out->row0 = reinterpret_cast<const int*>(dev + o_r);
  return VSM_OK;
}

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

template <typename T, typename Q>
static int ss_column(const Q* q, int S, int L, int m, const T* const* tau_h, const T* const* varpi_h, const T* const* tau_sum_h,
                     const T* const* Zpp_h, const T* const* Zmp_h, const long long* zs_h, const T* F0, const T* sj_m, const T* sj_p,
                     const T* ts_surf, int nV, const int* row0_h, const T* w_h, T* R, T* Tt, T* J0_m, T* J0_p, void* stream) {
  int rc;
  if ((rc = ss_check_common<T>("ss_column", q, S, L, nV, row0_h, w_h))) return rc;
  VSM_REQUIRE(tau_h && varpi_h && tau_sum_h && Zpp_h && Zmp_h && zs_h, "ss_column: null layer table");
  VSM_REQUIRE(F0 && sj_m && ts_surf && R && Tt, "ss_column: null argument");
  VSM_REQUIRE((J0_m == nullptr) == (J0_p == nullptr), "ss_column: J0_m and J0_p go together");
  VSM_REQUIRE(m >= 0, "ss_column: m >= 0");
  const long long NN = (long long)q->N * q->N;
  std::vector<ss_layer<T>> lay((size_t)L);
  for (int iz = 0; iz < L; ++iz) {
    VSM_REQUIRE(tau_h[iz] && varpi_h[iz] && tau_sum_h[iz] && Zpp_h[iz] && Zmp_h[iz], "ss_column: null entry in layer table %d", iz);
    VSM_REQUIRE(zs_h[iz] == 0 || zs_h[iz] == NN, "ss_column: z_stride[%d] must be 0 or N*N", iz);
    lay[iz] = ss_layer<T>{tau_h[iz], varpi_h[iz], tau_sum_h[iz], Zpp_h[iz], Zmp_h[iz], nullptr, zs_h[iz]};
  }
  if (S == 0) return VSM_OK;
  hipStream_t st = as_stream(stream);
  ss_tables<T> t;
  if ((rc = ss_upload<T, ss_layer<T>>(L, lay, q->n_stokes, nV, row0_h, w_h, st, &t))) return rc;
  const unsigned gx = (unsigned)((S + SS_TB - 1) / SS_TB);
  const unsigned gv = (unsigned)((nV * q->n_stokes + SS_RB - 1) / SS_RB);
  hipLaunchKernelGGL((k_ss_column<T, true>), dim3(gx, gv), dim3(SS_TB), 0, st, q->N, q->n_stokes, S, L, m, q->i_mu0, t.lay, F0,
                     sj_m, sj_p, ts_surf, q->mu, nV, t.row0, t.w, R, Tt);
  VSM_LAUNCH_CHECK("k_ss_column");
  if (J0_m) {
    const unsigned gf = (unsigned)((q->N + SS_RB - 1) / SS_RB);
    hipLaunchKernelGGL((k_ss_column<T, false>), dim3(gx, gf), dim3(SS_TB), 0, st, q->N, q->n_stokes, S, L, m, q->i_mu0, t.lay,
                       F0, sj_m, sj_p, ts_surf, q->mu, nV, t.row0, t.w, J0_m, J0_p);
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
  VSM_REQUIRE(P >= 1 && p_layer >= 0 && p_layer <= P, "ss_column_lin: P >= 1 and 0 <= p_layer <= P required (P = %d, p_layer = %d)",
              P, p_layer);
  VSM_REQUIRE(p_zdot >= 0 && p_zdot <= p_layer, "ss_column_lin: 0 <= p_zdot <= p_layer required (p_zdot = %d)", p_zdot);
  VSM_REQUIRE(p_lo >= 0 && p_lo < p_hi && p_hi <= P, "ss_column_lin: slot range [%d, %d) outside [0, %d)", p_lo, p_hi, P);
  VSM_REQUIRE((p_hi - p_lo + SS_PC - 1) / SS_PC <= 65535, "ss_column_lin: too many slots");
  VSM_REQUIRE(tau_h && varpi_h && tau_sum_h && Zpp_h && Zmp_h && zs_h, "ss_column_lin: null layer table");
  VSM_REQUIRE(p_layer == 0 || (tau_dot_h && varpi_dot_h && tau_sum_dot_h && tsd_surf), "ss_column_lin: null derivative table");
  VSM_REQUIRE(F0 && sj_m && sjd_m && sjd_p && ts_surf && Rd && Td, "ss_column_lin: null argument");
  VSM_REQUIRE(m >= 0 && CT >= 0, "ss_column_lin: m >= 0 and CT >= 0");
  const long long NN = (long long)q->N * q->N;
  std::vector<ss_layer_lin<T>> lay((size_t)L);
  bool any_zd = false;
  for (int iz = 0; iz < L; ++iz) {
    VSM_REQUIRE(tau_h[iz] && varpi_h[iz] && tau_sum_h[iz] && Zpp_h[iz] && Zmp_h[iz], "ss_column_lin: null entry in layer table %d",
                iz);
    VSM_REQUIRE(p_layer == 0 || (tau_dot_h[iz] && varpi_dot_h[iz] && tau_sum_dot_h[iz]),
                "ss_column_lin: null entry in derivative table %d", iz);
    VSM_REQUIRE(zs_h[iz] == 0 || zs_h[iz] == NN, "ss_column_lin: z_stride[%d] must be 0 or N*N", iz);
    const T* zc = (zdcoef_h && p_zdot > 0) ? zdcoef_h[iz] : nullptr;
    any_zd = any_zd || zc;
    VSM_REQUIRE(!zc || (CT >= 1 && Zc_pp && Zc_mp), "ss_column_lin: Z_dot coefficients without component blocks (layer %d)", iz);
    lay[iz] = ss_layer_lin<T>{tau_h[iz], varpi_h[iz], tau_sum_h[iz], Zpp_h[iz], Zmp_h[iz],
                              p_layer ? tau_dot_h[iz] : nullptr, p_layer ? varpi_dot_h[iz] : nullptr,
                              p_layer ? tau_sum_dot_h[iz] : nullptr, zc, zs_h[iz]};
  }
  if (S == 0) return VSM_OK;
  hipStream_t st = as_stream(stream);
  ss_tables<T, ss_layer_lin<T>> t;
  if ((rc = ss_upload<T, ss_layer_lin<T>>(L, lay, q->n_stokes, nV, row0_h, w_h, st, &t))) return rc;
  const unsigned gx = (unsigned)((S + SS_TB - 1) / SS_TB);
  const unsigned gv = (unsigned)((nV * q->n_stokes + SS_RB - 1) / SS_RB);
  const unsigned gp = (unsigned)((p_hi - p_lo + SS_PC - 1) / SS_PC);
  if (any_zd)
    hipLaunchKernelGGL((k_ss_column_lin<T, true>), dim3(gx, gv, gp), dim3(SS_TB), 0, st, q->N, q->n_stokes, S, L, m, q->i_mu0, P,
                       p_layer, p_zdot, p_lo, p_hi, t.lay, CT, Zc_pp, Zc_mp, F0, sj_m, sj_p, sjd_m, sjd_p, ts_surf, tsd_surf, q->mu,
                       nV, t.row0, t.w, Rd, Td);
  else
    hipLaunchKernelGGL((k_ss_column_lin<T, false>), dim3(gx, gv, gp), dim3(SS_TB), 0, st, q->N, q->n_stokes, S, L, m, q->i_mu0, P,
                       p_layer, 0, p_lo, p_hi, t.lay, 0, (const T*)nullptr, (const T*)nullptr, F0, sj_m, sj_p, sjd_m, sjd_p, ts_surf,
                       tsd_surf, q->mu, nV, t.row0, t.w, Rd, Td);
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
  VSM_REQUIRE(tau_h && tau_sum_h && fscatt_h, "ss_column_rrs: null layer table");
  VSM_REQUIRE(F0 && ieR && ieT && Zpp_ie && Zmp_ie, "ss_column_rrs: null argument");
  VSM_REQUIRE(K == 0 || (shift && varpi_ie), "ss_column_rrs: null line table");
  VSM_REQUIRE(m >= 0 && halo >= 0, "ss_column_rrs: m >= 0 and halo >= 0");
  std::vector<ss_layer<T>> lay((size_t)L);
  for (int iz = 0; iz < L; ++iz) {
    VSM_REQUIRE(tau_h[iz] && tau_sum_h[iz] && fscatt_h[iz], "ss_column_rrs: null entry in layer table %d", iz);
    lay[iz] = ss_layer<T>{tau_h[iz], nullptr, tau_sum_h[iz], nullptr, nullptr, fscatt_h[iz], 0};
  }
  if (S == 0 || K == 0) return VSM_OK;
  if (halo > VSM_SS_MAX_HALO) halo = VSM_SS_MAX_HALO;
  hipStream_t st = as_stream(stream);
  ss_tables<T> t;
  if ((rc = ss_upload<T, ss_layer<T>>(L, lay, q->n_stokes, nV, row0_h, w_h, st, &t))) return rc;
  const unsigned gx = (unsigned)((S + SS_TB - 1) / SS_TB);
  const unsigned gv = (unsigned)((nV * q->n_stokes + SS_RB - 1) / SS_RB);
  const size_t lds = sizeof(T) * (size_t)(4 + 2 * SS_RB) * (size_t)(SS_TB + 2 * halo);
  hipLaunchKernelGGL(k_ss_column_rrs<T>, dim3(gx, gv), dim3(SS_TB), lds, st, q->N, q->n_stokes, S, L, K, m, q->i_mu0, halo, t.lay,
                     shift, varpi_ie, Zpp_ie, Zmp_ie, F0, q->mu, nV, t.row0, t.w, ieR, ieT);
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
  VSM_REQUIRE(P >= 1 && p_layer >= 0 && p_layer <= P,
              "ss_column_rrs_lin: P >= 1 and 0 <= p_layer <= P required (P = %d, p_layer = %d)", P, p_layer);
  VSM_REQUIRE(p_lo >= 0 && p_lo < p_hi && p_hi <= P, "ss_column_rrs_lin: slot range [%d, %d) outside [0, %d)", p_lo, p_hi, P);
  VSM_REQUIRE((p_hi - p_lo + SS_RPC - 1) / SS_RPC <= 65535, "ss_column_rrs_lin: too many slots");
  VSM_REQUIRE(tau_h && tau_sum_h && fscatt_h, "ss_column_rrs_lin: null layer table");
  VSM_REQUIRE(p_layer == 0 || (tau_dot_h && tau_sum_dot_h && fscatt_dot_h), "ss_column_rrs_lin: null derivative table");
  VSM_REQUIRE(F0 && ieRd && ieTd && Zpp_ie && Zmp_ie, "ss_column_rrs_lin: null argument");
  VSM_REQUIRE(K == 0 || (shift && varpi_ie), "ss_column_rrs_lin: null line table");
  VSM_REQUIRE(m >= 0 && halo >= 0, "ss_column_rrs_lin: m >= 0 and halo >= 0");
  std::vector<ss_layer_rrs_lin<T>> lay((size_t)L);
  for (int iz = 0; iz < L; ++iz) {
    VSM_REQUIRE(tau_h[iz] && tau_sum_h[iz] && fscatt_h[iz], "ss_column_rrs_lin: null entry in layer table %d", iz);
    VSM_REQUIRE(p_layer == 0 || (tau_dot_h[iz] && tau_sum_dot_h[iz] && fscatt_dot_h[iz]),
                "ss_column_rrs_lin: null entry in derivative table %d", iz);
    lay[iz] = ss_layer_rrs_lin<T>{tau_h[iz], tau_sum_h[iz], fscatt_h[iz], p_layer ? tau_dot_h[iz] : nullptr,
                                  p_layer ? tau_sum_dot_h[iz] : nullptr, p_layer ? fscatt_dot_h[iz] : nullptr};
  }
  const int p_end = p_hi < p_layer ? p_hi : p_layer;   // the surface's slots (and any later ones) are exact zeros: not touched
  if (S == 0 || K == 0 || p_lo >= p_end) return VSM_OK;
  if (halo > VSM_SS_MAX_HALO) halo = VSM_SS_MAX_HALO;
  hipStream_t st = as_stream(stream);
  ss_tables<T, ss_layer_rrs_lin<T>> t;
  if ((rc = ss_upload<T, ss_layer_rrs_lin<T>>(L, lay, q->n_stokes, nV, row0_h, w_h, st, &t))) return rc;
  const unsigned gx = (unsigned)((S + SS_TB - 1) / SS_TB);
  const unsigned gv = (unsigned)((nV * q->n_stokes + SS_RB - 1) / SS_RB);
  const unsigned gp = (unsigned)((p_end - p_lo + SS_RPC - 1) / SS_RPC);
  const size_t lds = sizeof(T) * (size_t)(4 + 2 * SS_RB + 2 * SS_RPC) * (size_t)(SS_TB + 2 * halo);
  static_assert(sizeof(double) * (4 + 2 * SS_RB + 2 * SS_RPC) * (VSM_SS_BLOCK + 2 * VSM_SS_MAX_HALO) <= 65536,
                "k_ss_column_rrs_lin: a workgroup stays within 64 KB of LDS");
  hipLaunchKernelGGL(k_ss_column_rrs_lin<T>, dim3(gx, gv, gp), dim3(SS_TB), lds, st, q->N, q->n_stokes, S, L, K, m, q->i_mu0, halo,
                     p_layer, p_lo, p_hi, t.lay, shift, varpi_ie, Zpp_ie, Zmp_ie, F0, q->mu, nV, t.row0, t.w, ieRd, ieTd);
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
