// FP32 native-layout layer kernels (Float32 models, sub-problems of n <= 96 rows): rt_kernel!'s scattering branch
// (rt_kernel.jl:175-250: elemental! -> doubling! -> interaction!(::ScatteringInterface_11) | TOA copy) in the model's own float
// type -- the reference runs doubling.jl:38-131 / interaction.jl:207-266 in FT -- on v_mfma_f32_16x16x4_f32, with the
// CompositeLayer kept in FP32 strip records between the layer steps of a run (vsm_run_*_f32).  The algebra, the phases and the
// barriers are those of vsm_native.hip (doubling step: rt_helpers.jl:102-166 as [E | W] = r [r | t]; interaction with ONE inverse
// and at most six live strips); what differs is in vsm_native32_dev.h: the permuted A-form that makes the FP32 accumulator layout
// coincide with the FP64 one, 16-byte units of four rows, two spectral points per workgroup from five row tiles on.
//   RT = 1..4 (n <= 64):  RT waves per workgroup, four waves per SIMD (a strip is 4 RT registers)
//   RT = 5, 6 (n <= 96):  two points per workgroup of 2 RT waves, three waves per SIMD (168 registers) -- C4's dense moments (N = 96)
//   RT = 7, 8 (n <= 128): one point per workgroup of 7 / 8 waves, two waves per SIMD (256 registers: six live strips of 32)
#include <stdlib.h>

#include <vector>

#include "vsm_native32_dev.h"
#include "vsm_native_run.h"

#ifndef VSM_N32_PARK_RT
#define VSM_N32_PARK_RT 5
#endif

namespace vsm {

struct n32layer_comps {
  float* c[NSUB_MAX];
};

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// elemental (from the pre-pass images) + ndoubl x doubling step + apply_D
// ---------------------------------------------------------------------------------------------------------------------------
// On return (all waves past a barrier): r_s = strip of the final r-+ (row signs of apply_D applied), t_s = strip of t++ (rider
// columns cleared), sm.vec[0] = j0+, sm.vec[1] = j0- (final sign), sm.usg filled.
template <int RT, int KS>
__device__ __forceinline__ void n32ed_body(n32smem<RT, (4 * KS + 2 > 16 * RT)>& sm, n32pos<RT>& p, int n, int gsz, unsigned uvmask,
                                           int ndoubl, const float* __restrict__ img, n32strip<RT>& r_s, n32strip<RT>& t_s,
                                           int* status) {
  using G = n32geo<RT>;
  constexpr unsigned dP = 0, dQ = G::AF * 4;
  float* jp = sm.vec[0];
  float* jm = sm.vec[1];
  float* rsg = sm.vec[3];   // row sign of apply_D
  const int tid = p.tid;
  constexpr int c1 = 4 * KS, c2 = 4 * KS + 1;   // spare columns (>= n, never read as k) carry j0+ / j1- through a step
  constexpr bool RID = c2 < G::NP;              // KS = 4 RT: no spare column, the source vectors by VALU mat-vecs
  static_assert(RID || KS == 4 * RT, "no spare columns for the source vectors");
  const bool own_wave = RID && p.wave == (c1 >> 4);
  const bool laneA = own_wave && (p.col == c1), laneB = own_wave && (p.col == c2), laneAB = laneA || laneB;
  n32copy_image<RT>(sm.P, img, p);
  n32copy_image<RT>(sm.Q, img + G::AF, p);
  if (tid < G::NP) {
    jp[tid] = img[2 * G::AF + tid];
    jm[tid] = img[2 * G::AF + G::NP + tid];
    const bool uv = (uvmask >> (tid % gsz)) & 1u;
    sm.usg[tid] = uv ? -1.0f : 1.0f;
    rsg[tid] = (ndoubl >= 1 && uv) ? -1.0f : 1.0f;
  }
  const float expk0 = img[2 * G::AF + 2 * G::NP];
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the DMA writes have landed in LDS
  __syncthreads();
  n32load(r_s, dP, p);
  n32load(t_s, dQ, p);
  // ---- doubling (rt_helpers.jl:102-166) -----------------------------------------------------------------------------------
  //   [E | W]   = r [r | t]                 A = P = [r]
  //   G         = (I - E)^-1                Horner series on [E] in P
  //   tt        = t G                       A = Q = [t]
  //   [r' | t'] = [r | 0] + tt [W | t]      A = P = [tt]
  // Sources (rt_helpers.jl:128-134: j0- += tt (j1- + r j0+), j0+ = j1+ + tt (j0+ + r j1-)) ride in the spare columns:
  //   t_s[c1] = j0+, t_s[c2] = j1- = j0- expk  ->  W[c1] = r j0+, W[c2] = r j1-
  //   r_s[c1] = j0-, r_s[c2] = j0+             ->  W[c1] += r_s[c1] expk, W[c2] += r_s[c2], r_s[c2] *= expk: lane-local;
  //                                                r'[c1] = j0- + tt (j1- + r j0+), r'[c2] = j1+ + tt (j0+ + r j1-)
  float expk = expk0;
  int slot = 0;
  const n32inv_ctx cx{dP, sm.P, sm.gjs(), status};
  for (int it = 0; it < ndoubl; ++it) {
    n32strip<RT> W, tt;
    const float fW = laneA ? expk : (laneB ? 1.0f : 0.0f), fR = laneB ? expk : 1.0f;
    if constexpr (!RID) {   // r j0+ , r j1-   (P = [r])
      n32mv_rows<RT, KS>(dP, jp, 1.0f, sm.mv[0], p);
      n32mv_rows<RT, KS>(dP, jm, expk, sm.mv[1], p);
    }
    {
      n32strip<RT> Gs;
      {
        n32strip<RT> E;
        n32mm2<RT, KS, true, true>(E, W, dP, r_s, t_s, p);
        if (own_wave) {
#pragma unroll
          for (int ta = 0; ta < RT; ++ta)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              W.v[ta][r] = fmaf(r_s.v[ta][r], fW, W.v[ta][r]);
              r_s.v[ta][r] *= fR;
            }
        }
        float nrm_o;
        const float nrm = n32norm(E, n, sm, slot, p, nrm_o);   // (its barrier: [r] is free)
        if constexpr (!RID) {   // u1 = j1- + r j0+ , u2 = j0+ + r j1-   (every wave is past the norm reduction's barrier)
          for (int i = tid; i < G::NP; i += G::NTP) {
            sm.vec[4][i] = jm[i] * expk + sm.mv[0][i];
            sm.vec[5][i] = jp[i] + sm.mv[1][i];
          }
        }
        n32invert_pair<RT, KS>(n32inv_order(nrm, status, p.live && tid == 0), n32series_order(nrm_o), E, Gs, n, cx, p);
      }
      n32mm<RT, KS, true>(tt, dQ, Gs, p);    // tt = t G
    }
    n32load(t_s, dQ, p);                     // t's strip (with its riders) is not kept in registers across the inverse
    __syncthreads();                         // P ([E]) and Q ([t]) no longer read
    n32store(dP, tt, p);
    __syncthreads();
    if constexpr (!RID) {   // tt u1 , tt u2
      n32mv_rows<RT, KS>(dP, sm.vec[4], 1.0f, sm.mv[0], p);
      n32mv_rows<RT, KS>(dP, sm.vec[5], 1.0f, sm.mv[1], p);
    }
    {
      n32strip<RT> tn;
      n32mm2<RT, KS, false, true>(r_s, tn, dP, W, t_s, p);   // r' = r + tt W (riders: the new j0-, j0+) ; t' = tt t
      t_s = tn;
    }
    const float expk_step = expk;
    expk = expk * expk;
    if (own_wave) {
      const float ft = laneB ? expk : 1.0f;   // t_s[c1] = j0+', t_s[c2] = j1-' = j0-' expk'
#pragma unroll
      for (int ta = 0; ta < RT; ++ta)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float u = n32dpp_swap1(r_s.v[ta][r]) * ft;
          t_s.v[ta][r] = laneAB ? u : t_s.v[ta][r];
        }
    }
    if (it + 1 < ndoubl || !RID) __syncthreads();   // everybody finished reading P ([tt])
    if constexpr (!RID) {   // j0- += tt u1 ; j0+ = j0+ expk + tt u2   (visible after the barrier below / after the loop)
      for (int i = tid; i < G::NP; i += G::NTP) {
        jm[i] += sm.mv[0][i];
        jp[i] = jp[i] * expk_step + sm.mv[1][i];
      }
    }
    if (it + 1 < ndoubl) {
      n32store(dP, r_s, p);
      n32store(dQ, t_s, p);
      __syncthreads();
    }
  }
  if constexpr (RID) {
    if (ndoubl > 0 && own_wave) {   // the riders go back to the LDS vectors; the strips leave the loop with clean padding
#pragma unroll
      for (int ta = 0; ta < RT; ++ta)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = p.row(ta, r);
          float* dpv = laneA ? jp : sm.vec[7];   // (the other lanes write to a dummy vector)
          float* dmv = laneA ? jm : sm.vec[7];
          dpv[row] = t_s.v[ta][r];          // lane A: j0+
          dmv[row] = r_s.v[ta][r];          // lane A: j0-
          t_s.v[ta][r] = laneAB ? 0.0f : t_s.v[ta][r];
          r_s.v[ta][r] = laneAB ? 0.0f : r_s.v[ta][r];
        }
    }
  }
  __syncthreads();
  // ---- apply_D (doubling.jl:178-252): r-+ = D r*, j0- = D j0-* ------------------------------------------------------------
  if (ndoubl >= 1) {
#pragma unroll
    for (int ta = 0; ta < RT; ++ta)
#pragma unroll
      for (int r = 0; r < 4; ++r) r_s.v[ta][r] *= rsg[p.row(ta, r)];
    for (int i = tid; i < G::NP; i += G::NTP) jm[i] *= rsg[i];
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------
// interaction_helper!(::ScatteringInterface_11) (interaction.jl:207-266) on the run's native records.  With
// G2 = (I - R+- r-+)^-1 and the push-through identities (I - r R)^-1 r = r G2, (I - r R)^-1 = I + r G2 R:
//   [E2 | Z] = R+- [r-+ | t--]          A = P = [R+-]   z  = J0+ + R+- j0-   (j0- rides in a spare column of r-+)
//   G2       = (I - E2)^-1              A = P = [E2]    BEFORE the products of [T--]: V is not live across the series
//   [S  | V] = T-- [r-+ | t--]          A = Q = [T--]   vs = T-- j0-
//   T21 = t++ G2 ;  Y = S G2            A = P = [t++], Q = [S]
//   [R+- | T++] = [r+- | 0] + T21 [Z | T++]      A = P = [T21]   J0+ = j0+ + T21 z   (z rides in a spare column of T++)
//   [R-+ | T--] = [R-+ | V] + Y [T++ | Z]        A = Q = [Y]     J0- = J0- + vs + Y z
// On entry: r_s / t_s = strips of the added layer's r-+ / t++ (columns >= n zero), sm.vec[0] / vec[1] = its j0+ / j0-, all waves
// past a barrier, P and Q free.  r+- = D r-+ D, t-- = D t++ D (added layers from doubling).
// ---------------------------------------------------------------------------------------------------------------------------
template <int RT, int KS>
__device__ __forceinline__ void n32ia_body(n32smem<RT, (4 * KS + 2 > 16 * RT)>& sm, n32pos<RT>& p, int n, float* __restrict__ comp,
                                           n32strip<RT>& r_s, n32strip<RT>& t_s, int* status) {
  using G = n32geo<RT>;
  constexpr unsigned dP = 0, dQ = G::AF * 4;
  float* vjp = sm.vec[0];
  float* vjm = sm.vec[1];
  float* vJp = sm.vec[2];
  float* vJm = sm.vec[3];
  float* vs = sm.vec[4];
  float* vz = sm.vec[5];
  const int tid = p.tid;
  float* R_mp = comp + N32_RMP * G::AF;
  float* R_pm = comp + N32_RPM * G::AF;
  float* T_pp = comp + N32_TPP * G::AF;
  float* T_mm = comp + N32_TMM * G::AF;
  float* J0_p = comp + 4 * G::AF;
  float* J0_m = J0_p + G::NP;
  constexpr int c1 = 4 * KS, c2 = 4 * KS + 1;
  constexpr bool RID = c2 < G::NP;
  // Five and six row tiles (168 registers, strips of 20 / 24): at most FIVE live strips.  Z = R+- t-- is not needed between its
  // product and the closing pairs: it waits in the R+- record of the composite (consumed into P at the entry, overwritten by the
  // new R+- at the end; the lane reads back exactly the addresses it wrote), and R-+ is requested after R+- / T++ have left.
  constexpr bool PARK = VSM_N32_PARK_RT > 0 && RT >= VSM_N32_PARK_RT;
  const bool own_wave = RID && p.wave == (c1 >> 4);
  const bool laneA = own_wave && (p.col == c1), laneB = own_wave && (p.col == c2);
  int slot = 0;
  const n32dpar<RT> dp(sm.usg, p);
  const n32inv_ctx cx{dP, sm.P, sm.gjs(), status};
  // ---- stage: composite vectors, [R+-] -> P, [T--] -> Q ---------------------------------------------------------------------
  for (int i = tid; i < G::NP; i += G::NTP) {
    vJp[i] = J0_p[i];
    vJm[i] = J0_m[i];
  }
  n32strip<RT> Z, Gs;
  {
    n32strip<RT> A1, A2;
    n32ld_native(A1, R_pm, p);
    n32ld_native(A2, T_mm, p);
    n32store(dP, A1, p);
    n32store(dQ, A2, p);
  }
  if constexpr (RID) {
    if (own_wave) {  // j0- rides in the spare column c2 of r-+:  E2[:, c2] = R+- j0-, S[:, c2] = T-- j0-
#pragma unroll
      for (int ta = 0; ta < RT; ++ta)
#pragma unroll
        for (int r = 0; r < 4; ++r) r_s.v[ta][r] = laneB ? vjm[p.row(ta, r)] : r_s.v[ta][r];
    }
  }
  n32dsym(t_s, t_s, dp);   // t-- = D t++ D in place (undone below: D is an involution)
  __syncthreads();                                                                                       // (a)
  if constexpr (!RID) {   // R+- j0- , T-- j0-
    n32mv_rows<RT, KS>(dP, vjm, 1.0f, sm.mv[0], p);
    n32mv_rows<RT, KS>(dQ, vjm, 1.0f, sm.mv[1], p);
  }
  {
    n32strip<RT> E;
    n32mm2<RT, KS, true, true>(E, Z, dP, r_s, t_s, p);
    if constexpr (RID) {
      if (own_wave) {
        float* zd = laneB ? vz : sm.vec[7];   // (the other lanes write to a dummy vector)
#pragma unroll
        for (int ta = 0; ta < RT; ++ta)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = p.row(ta, r);
            zd[row] = vJp[row] + E.v[ta][r];
          }
      }
    }
    if constexpr (PARK) n32st_native(R_pm, Z, p, p.live);   // (its old contents are in P; the new R+- overwrites it at the end)
    float nrm_o;
    const float nrm = n32norm(E, n, sm, slot, p, nrm_o);   // (b): every wave is done reading [R+-]
    if constexpr (!RID) {   // z = J0+ + R+- j0- ; vs = T-- j0-
      for (int i = tid; i < G::NP; i += G::NTP) {
        vz[i] = vJp[i] + sm.mv[0][i];
        vs[i] = sm.mv[1][i];
      }
    }
    n32invert_pair<RT, KS>(n32inv_order(nrm, status, p.live && tid == 0), n32series_order(nrm_o), E, Gs, n, cx, p);   // [E2] -> P, series
  }
  n32strip<RT> V;
  {
    n32strip<RT> S;
    n32mm2<RT, KS, true, true>(S, V, dQ, r_s, t_s, p);   // (Q = [T--] has not been touched since (a))
    if constexpr (RID) {
      if (own_wave) {
        float* sd = laneB ? vs : sm.vec[7];
#pragma unroll
        for (int ta = 0; ta < RT; ++ta)
#pragma unroll
          for (int r = 0; r < 4; ++r) sd[p.row(ta, r)] = S.v[ta][r];
      }
    }
    // r_s <- r+- (the accumulator of the R+- update; its rider column is never used), t_s <- t++
    n32dsym(r_s, r_s, dp);
    n32dsym(t_s, t_s, dp);
    __syncthreads();                      // (d): [E2] (series) and [T--] no longer read
    n32store(dQ, S, p);                   // [S]   -> Q
    n32store(dP, t_s, p);                 // [t++] -> P
  }
  __syncthreads();                        // (e)
  {
    n32strip<RT> X, Y;
    n32mm<RT, KS, true>(X, dP, Gs, p);    // T21 = t++ G2
    n32mm<RT, KS, true>(Y, dQ, Gs, p);    // Y = S G2 = T01 r-+
    __syncthreads();                      // (f): [t++], [S] no longer read
    n32store(dP, X, p);                   // [T21] -> P
    n32store(dQ, Y, p);                   // [Y]   -> Q
  }
  __builtin_amdgcn_sched_barrier(0);      // (the composite strips are requested once X and Y are dead, not above their stores)
  n32strip<RT> Tpp, Rmp;
  n32ld_native(Tpp, T_pp, p);
  if constexpr (PARK) n32ld_native(Z, R_pm, p); else n32ld_native(Rmp, R_mp, p);
  __syncthreads();                        // (g)
  if constexpr (!RID) {   // T21 z , Y z
    n32mv_rows<RT, KS>(dP, vz, 1.0f, sm.mv[0], p);
    n32mv_rows<RT, KS>(dQ, vz, 1.0f, sm.mv[1], p);
  }
  if constexpr (RID) {
    if (own_wave) {  // z rides in the spare column c1 of T++:  (T21 T++)[:, c1] = T21 z, (Y T++)[:, c1] = Y z
#pragma unroll
      for (int ta = 0; ta < RT; ++ta)
#pragma unroll
        for (int r = 0; r < 4; ++r) Tpp.v[ta][r] = laneA ? vz[p.row(ta, r)] : Tpp.v[ta][r];
    }
  }
  {
    n32strip<RT> acc;
    n32mm2<RT, KS, false, true>(r_s, acc, dP, Z, Tpp, p);   // R+- = r+- + T21 Z ; T++ = T21 T++
    n32st_native(R_pm, r_s, p, p.live);
    n32st_native(T_pp, acc, p, p.live);
    if (laneA && p.live) {
#pragma unroll
      for (int ta = 0; ta < RT; ++ta)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = p.row(ta, r);
          J0_p[row] = vjp[row] + acc.v[ta][r];
        }
    }
  }
  if constexpr (PARK) {
    __builtin_amdgcn_sched_barrier(0);      // (requested once r_s and acc have left)
    n32ld_native(Rmp, R_mp, p);
  }
  if constexpr (RID) {
    if (own_wave) {   // (the native record keeps the rider column of the previous layer step)
#pragma unroll
      for (int ta = 0; ta < RT; ++ta)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rmp.v[ta][r] = laneA ? 0.0f : Rmp.v[ta][r];
    }
  }
  n32mm2<RT, KS>(Rmp, V, dQ, Tpp, Z, p);       // R-+ = R-+ + Y T++ ; T-- = V + Y Z
  n32st_native(R_mp, Rmp, p, p.live);
  n32st_native(T_mm, V, p, p.live);
  if (laneA && p.live) {
#pragma unroll
    for (int ta = 0; ta < RT; ++ta)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = p.row(ta, r);
        J0_m[row] = vJm[row] + vs[row] + Rmp.v[ta][r];
      }
  }
  if constexpr (!RID) {   // J0+ = j0+ + T21 z ; J0- = J0- + T-- j0- + Y z
    __syncthreads();
    if (p.live) {
      for (int i = tid; i < G::NP; i += G::NTP) {
        J0_p[i] = vjp[i] + sm.mv[0][i];
        J0_m[i] = vJm[i] + vs[i] + sm.mv[1][i];
      }
    }
  }
}

template <int RT, int KS>
__global__ __launch_bounds__(n32geo<RT>::NT, n32geo<RT>::WPS) void k_layer_native32(int S, int n, int gsz, unsigned uvmask, int ndoubl,
                                                                                    int toa, const float* __restrict__ pre,
                                                                                    n32layer_comps a, int* status) {
  using G = n32geo<RT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  using SM = n32smem<RT, (4 * KS + 2 > 16 * RT)>;
  static_assert(sizeof(SM) % 16 == 0, "the second point's LDS block starts on a 16-byte boundary");
  const int pt = G::PP == 1 ? 0 : (int)(threadIdx.x >> 6) / RT;
  SM& sm = reinterpret_cast<SM*>(smem_raw)[pt];
  n32pos<RT> p(sm.P);
  int s = blockIdx.x * G::PP + pt;
  const int isub = blockIdx.y;
  p.live = s < S;
  s = min(s, S - 1);   // (the filler point of an odd batch walks the last point again, for the barriers; it stores nothing)
  const float* img = pre + ((long long)isub * S + s) * G::PRE_STRIDE;
  float* comp = a.c[isub] + (long long)s * G::COMP_STRIDE;
  n32strip<RT> r_s, t_s;
  n32ed_body<RT, KS>(sm, p, n, gsz, uvmask, ndoubl, img, r_s, t_s, status);
  if (toa) {   // copy_added_to_composite! (rt_helpers.jl:188-200)
    const n32dpar<RT> dp(sm.usg, p);
    n32st_native(comp + N32_RMP * G::AF, r_s, p, p.live);
    n32st_native(comp + N32_TPP * G::AF, t_s, p, p.live);
    n32strip<RT> d;
    n32dsym(d, r_s, dp);
    n32st_native(comp + N32_RPM * G::AF, d, p, p.live);
    n32dsym(d, t_s, dp);
    n32st_native(comp + N32_TMM * G::AF, d, p, p.live);
    if (p.live) {
      for (int i = p.tid; i < G::NP; i += G::NTP) {
        comp[4 * G::AF + i] = sm.vec[0][i];
        comp[4 * G::AF + G::NP + i] = sm.vec[1][i];
      }
    }
    return;
  }
  n32ia_body<RT, KS>(sm, p, n, comp, r_s, t_s, status);
}

}  // namespace

// one object per k-step count (parallel build): vsm_native32_<KS>.o is this file built with -DVSM_NATIVE32_KS=<KS>
#define VSM_N32CAT2(a, b) a##b
#define VSM_N32CAT(a, b) VSM_N32CAT2(a, b)
#define VSM_NATIVE32_DECL(KS) \
  int VSM_N32CAT(launch_layer_native32_, KS)(int, int, int, unsigned, int, int, int, const float*, const n32layer_comps&, int*, hipStream_t);

#ifdef VSM_NATIVE32_KS
VSM_NATIVE32_DECL(VSM_NATIVE32_KS)
int VSM_N32CAT(launch_layer_native32_, VSM_NATIVE32_KS)(int S, int nsub, int n, unsigned uvmask, int gsz, int ndoubl, int toa,
                                                        const float* pre, const n32layer_comps& comps, int* status, hipStream_t st) {
  constexpr int KS = VSM_NATIVE32_KS;
  // KS = 4, 8, ... 24: KS / 4 row tiles without spare columns (mat-vec source path) instead of one row tile more for two columns
  constexpr int RT = rt_of(4 * KS);
  static_assert(RT >= 1 && RT <= 8, "n <= 128");
  using G = n32geo<RT>;
  using SM = n32smem<RT, (4 * KS + 2 > 16 * RT)>;
  auto kern = k_layer_native32<RT, KS>;
  const int prepared = ensure_dyn_lds(reinterpret_cast<const void*>(kern), sizeof(SM) * G::PP, "hipFuncSetAttribute(k_layer_native32)");
  if (prepared) return prepared;
  hipLaunchKernelGGL(kern, dim3((S + G::PP - 1) / G::PP, nsub), dim3(G::NT), sizeof(SM) * G::PP, st, S, n, gsz, uvmask, ndoubl, toa, pre,
                     comps, status);
  VSM_LAUNCH_CHECK("k_layer_native32");
  return VSM_OK;
}
}  // namespace vsm

#else  // ---- dispatcher object: the pre-pass and the two launches the run driver (vsm_native.hip) calls -------------------------------

VSM_NATIVE32_DECL(1)
VSM_NATIVE32_DECL(2)
VSM_NATIVE32_DECL(3)
VSM_NATIVE32_DECL(4)
VSM_NATIVE32_DECL(5)
VSM_NATIVE32_DECL(6)
VSM_NATIVE32_DECL(7)
VSM_NATIVE32_DECL(8)
VSM_NATIVE32_DECL(9)
VSM_NATIVE32_DECL(10)
VSM_NATIVE32_DECL(11)
VSM_NATIVE32_DECL(12)
VSM_NATIVE32_DECL(13)
VSM_NATIVE32_DECL(14)
VSM_NATIVE32_DECL(15)
VSM_NATIVE32_DECL(16)
VSM_NATIVE32_DECL(17)
VSM_NATIVE32_DECL(18)
VSM_NATIVE32_DECL(19)
VSM_NATIVE32_DECL(20)
VSM_NATIVE32_DECL(21)
VSM_NATIVE32_DECL(22)
VSM_NATIVE32_DECL(23)
VSM_NATIVE32_DECL(24)
VSM_NATIVE32_DECL(25)
VSM_NATIVE32_DECL(26)
VSM_NATIVE32_DECL(27)
VSM_NATIVE32_DECL(28)
VSM_NATIVE32_DECL(29)
VSM_NATIVE32_DECL(30)
VSM_NATIVE32_DECL(31)
VSM_NATIVE32_DECL(32)

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// Elemental pre-pass: elemental! incl. the SFI source (elemental.jl:289-392) of every (point, sub-problem) of a layer as two
// A-form images + vectors (n32geo::PRE_STRIDE), in Float32 like the reference's Float32 run (vsm_elemental.h: the formulas of the
// FP32 strip kernels' pre-pass).  Sub-row i of a group g (Stokes components g[0..gsz)) is row (i / gsz) n_stokes + g[i % gsz] of
// the full problem.  Thread = (row tile t, kqr, k' | column phase): it owns the rows 16 t + 4 rr + kqr, rr = 0..3, of the columns
// 4 ks + k', ks = phase, phase + 4, ... -- the four words of an image block that are adjacent (n32af_idx): ONE 16-byte store per
// image and column, sixteen threads (kqr, k') write 256 contiguous bytes.
// ---------------------------------------------------------------------------------------------------------------------------
template <int RT, bool MIX>
__global__ __launch_bounds__(64 * RT) void k_elemental_native32(quad<float> q, int n, int ndoubl, const float* __restrict__ dtau,
                                                                const float* __restrict__ varpi, const float* __restrict__ tau_sum,
                                                                const float* __restrict__ F0, npre_args<float> a, float* __restrict__ pre) {
  using G = n32geo<RT>;
  constexpr int NP = G::NP;
  __shared__ float mus[NP], xs[NP], es[NP], ems[NP], wts[NP];
  __shared__ int frow[NP];
  __shared__ int thick_flag;
  const int s = blockIdx.x, isub = blockIdx.y, tid = threadIdx.x;
  const nsub_pre<float>& sp = a.s[isub];
  const int N = q.N, ns = q.n_stokes, m = sp.m, gsz = sp.gsz;
  const zsrc<float> z = sp.z;
  const float d = dtau[s], w = varpi[s];
  const int ncomp = MIX ? z.ncomp : 0;
  const long long NNz = (long long)N * N;
  const float* Zp = z.Zpp + (ncomp ? 0 : (long long)s * z.zs);
  const float* Zm = z.Zmp + (ncomp ? 0 : (long long)s * z.zs);
  float fk[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < ncomp) fk[k] = z.fcomp[(long long)s * ncomp + k];
  auto zget = [&](const float* Z, long long zo) {
    if (ncomp == 0) return Z[zo];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < ncomp) acc += fk[k] * Z[k * NNz + zo];
    return acc;
  };
  if (tid < NP) {
    const bool in = tid < n;
    const int ga = sp.g[tid % gsz];
    const int fr = in ? (tid / gsz) * ns + ga : 0;
    const float mu = in ? q.mu[fr] : 1.0f;
    const float x = d / mu;
    frow[tid] = fr;
    mus[tid] = mu;
    xs[tid] = x;
    es[tid] = exp(-x);
    ems[tid] = expm1(-x);
    wts[tid] = in ? q.wt[fr] : 0.0f;
  }
  if (tid == 0) thick_flag = 0;
  __syncthreads();
  if (tid < n && xs[tid] >= 0.5f) thick_flag = 1;   // (benign race: every writer stores 1)
  __syncthreads();
  const bool thick = thick_flag != 0;
  float* out = pre + ((long long)isub * gridDim.x + s) * G::PRE_STRIDE;
  float* R = out;
  float* T = out + G::AF;
  const int Kend = ((n + 3) >> 2) << 2;
  const int c1 = Kend, c2 = Kend + 1;
  const bool riders_in = ndoubl > 0 && c2 < NP;   // (no spare column: the layer kernel uses mat-vecs)
  // thread -> (kqr, k', row tile, column phase)
  const int kqr = tid & 3, kk = (tid >> 2) & 3, g16 = tid >> 4, t = g16 % RT, ph = g16 / RT;
  float mi[4], xi[4], ai[4], ei[4], sg[4];
  int fi[4];
  bool rin[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = 16 * t + 4 * rr + kqr;
    mi[rr] = mus[i];
    xi[rr] = xs[i];
    ai[rr] = ems[i];
    ei[rr] = es[i];
    rin[rr] = i < n;
    fi[rr] = frow[min(i, n - 1)];
    const bool uvi = i < n && sp.g[i % gsz] >= 2;
    sg[rr] = (ndoubl >= 1 && uvi) ? -1.0f : 1.0f;   // starred R* = D R (elemental.jl:403-422)
  }
  for (int ks = ph; ks < 4 * RT; ks += 4) {
    const int j = 4 * ks + kk;
    if (riders_in && (j == c1 || j == c2)) continue;   // written below
    f4_t rv = {0.f, 0.f, 0.f, 0.f}, tv = {0.f, 0.f, 0.f, 0.f};
    if (j < n) {
      const float wt = wts[j];
      const float wct = (m == 0) ? wt / 2.0f : wt / 4.0f;
      const bool active = wct > num<float>::eps();   // eps(FT) of the model's float type (elemental.jl:296)
      const float mj = mus[j], xj = xs[j], aj = ems[j], ej = es[j];
      const long long zc = (long long)N * frow[j];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 16 * t + 4 * rr + kqr;
        float rres, tres;
        elemental_pair<float>(w, zget(Zp, fi[rr] + zc), zget(Zm, fi[rr] + zc), mi[rr], xi[rr], ai[rr], ei[rr], mj, xj, aj, ej, wct, i == j,
                              thick, rres, tres);
        const float rvv = rin[rr] ? (active ? rres * sg[rr] : 0.0f) : 0.0f;
        const float tvv = rin[rr] ? (active ? tres : ((i == j) ? ei[rr] : 0.0f)) : 0.0f;
        rv[rr ^ (ks & 3)] = rvv;
        tv[rr ^ (ks & 3)] = tvv;
      }
    }
    const int o = (ks * RT + t) * 64 + ((kk << 4) | (kqr << 2));
    *reinterpret_cast<f4_t*>(R + o) = rv;
    *reinterpret_cast<f4_t*>(T + o) = tv;
  }
  if (tid < NP) {   // SFI source of the solar beam: the same formulas with the solar column (see elemental_pair)
    const int i = tid, ic = min(i, n - 1);
    const int fri = frow[ic];
    const int i0 = ns * q.i_mu0;
    const float mu0n = q.mu[i0];
    const float x0 = d / mu0n, e0 = exp(-x0), a0 = expm1(-x0);
    float zp = 0.0f, zm = 0.0f;
    for (int qq = 0; qq < ns; ++qq) {
      const long long zo = fri + (long long)N * (i0 + qq);
      const float f = F0[qq + (long long)ns * s];
      zp += zget(Zp, zo) * f;
      zm += zget(Zm, zo) * f;
    }
    const bool uvi = i < n && sp.g[i % gsz] >= 2;
    const float sgi = (ndoubl >= 1 && uvi) ? -1.0f : 1.0f;
    float rr, tt;
    // (the diagonal case mu_i == mu_0 of the source never takes the i == j form: elemental.jl:370-382)
    elemental_pair<float>(w, zp, zm, mus[i], xs[i], ems[i], es[i], mu0n, x0, a0, e0, (m == 0) ? 0.5f : 0.25f, false, thick || x0 >= 0.5f,
                          rr, tt);
    const float att = exp(-tau_sum[s] / mu0n);
    const float vp = (i < n) ? tt * att : 0.0f;
    const float vm = (i < n) ? rr * att * sgi : 0.0f;
    const float expk0 = exp(-d / q.mu0);
    out[2 * G::AF + i] = vp;
    out[2 * G::AF + NP + i] = vm;
    out[2 * G::AF + 2 * NP + i] = expk0;
    if (riders_in) {   // t[:, c1] = j0+, t[:, c2] = j1- = j0- expk ;  r[:, c1] = j0-, r[:, c2] = j0+
      T[n32af_idx<RT>(i, c1)] = vp;
      T[n32af_idx<RT>(i, c2)] = vm * expk0;
      R[n32af_idx<RT>(i, c1)] = vm;
      R[n32af_idx<RT>(i, c2)] = vp;
    }
  }
}

}  // namespace

void native32_launch_pre(int rt, bool mix, const quad<float>& q, int S, int nsub, int n, int ndoubl, const float* dtau,
                         const float* varpi, const float* tau_sum, const float* F0, const npre_args<float>& a, float* pre,
                         hipStream_t st) {
  const dim3 grid(S, nsub), block(64 * rt);
#define VSM_N32P(RT)                                                                                                             \
  case RT:                                                                                                                       \
    if (mix)                                                                                                                     \
      hipLaunchKernelGGL((k_elemental_native32<RT, true>), grid, block, 0, st, q, n, ndoubl, dtau, varpi, tau_sum, F0, a, pre);  \
    else                                                                                                                         \
      hipLaunchKernelGGL((k_elemental_native32<RT, false>), grid, block, 0, st, q, n, ndoubl, dtau, varpi, tau_sum, F0, a, pre); \
    break;
  switch (rt) { VSM_N32P(1) VSM_N32P(2) VSM_N32P(3) VSM_N32P(4) VSM_N32P(5) VSM_N32P(6) VSM_N32P(7) VSM_N32P(8) }
#undef VSM_N32P
}

int native32_launch_layer(int ks, int S, int nsub, int n, unsigned uvmask, int gsz, int ndoubl, int toa, const float* pre,
                          float* const* comps, int* status, hipStream_t st) {
  n32layer_comps lc;
  for (int k = 0; k < NSUB_MAX; ++k) lc.c[k] = comps[k];
#define VSM_N32L(KS) \
  case KS: return VSM_N32CAT(launch_layer_native32_, KS)(S, nsub, n, uvmask, gsz, ndoubl, toa, pre, lc, status, st);
  switch (ks) {
    VSM_N32L(1) VSM_N32L(2) VSM_N32L(3) VSM_N32L(4) VSM_N32L(5) VSM_N32L(6) VSM_N32L(7) VSM_N32L(8) VSM_N32L(9) VSM_N32L(10)
    VSM_N32L(11) VSM_N32L(12) VSM_N32L(13) VSM_N32L(14) VSM_N32L(15) VSM_N32L(16) VSM_N32L(17) VSM_N32L(18) VSM_N32L(19)
    VSM_N32L(20) VSM_N32L(21) VSM_N32L(22) VSM_N32L(23) VSM_N32L(24) VSM_N32L(25) VSM_N32L(26) VSM_N32L(27) VSM_N32L(28)
    VSM_N32L(29) VSM_N32L(30) VSM_N32L(31) VSM_N32L(32)
    default: break;
  }
#undef VSM_N32L
  set_error("launch_layer_native32: no kernel for %d k-steps", ks);
  return VSM_ERR_UNSUPPORTED;
}

}  // namespace vsm

#endif  // VSM_NATIVE32_KS
