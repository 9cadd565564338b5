// Absorption continua: HITRAN collision-induced absorption (src/Absorption/cia.jl, compute_τ_cia!) and the MT_CKD water-vapour
// continuum (src/Absorption/mtckd.jl, compute_τ_h2o_continuum!), with their T, p, vmr and Δz derivatives (ours); DESIGN 4.28.
//
//   k_continuum<LIN>  one launch for a whole set -- up to VSM_CONT_MAX_TABLES CIA tables and at most one MT_CKD band on one
//                     spectral grid -- and all Nz layers.  A workgroup owns 256 grid points and a tile of VSM_CONT_LAYERS layers;
//                     a lane keeps its point's nu and the three band values in registers over the tile.  Per (point, layer) the
//                     two table rows of every table are read once and held in registers; every output plane is then read (if it
//                     accumulates) and written ONCE, after the whole set has been added to it in list order.
//   CIA chain         fixed, only + - x, no contraction:  s_k = (1 - w) a + w b;  plane += s_k A[m, k, z];  on the dT plane
//                     plane += (b - a) B[m, k, z].  The host owns every per-layer coefficient.
//   MT_CKD            self, then foreign, behind the tables; tanh, pow and sinh are the device library's.
//   k_slots_add       out [K, Nz, nSpec] += plane [Nz, nSpec] tab [K, Nz]: the Δz share of the profile slots.
// No atomics, no library scratch, no host synchronisation; a call is bit-identical to its repetition, and a point's result does
// not depend on its lane, its layer tile or Nz: lanes share nothing but the tile's per-layer coefficients, copied through LDS.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vsm_common.h"
#include "vsm_internal.h"

// every product and sum below is written out
#pragma clang fp contract(off)

namespace vsm {

constexpr int CONT_TILE = 256;                      // grid points per workgroup
constexpr int CONT_LAYERS = VSM_CONT_LAYERS;        // layers per workgroup
constexpr int CONT_TABLES = VSM_CONT_MAX_TABLES;
constexpr int CONT_PLANES = VSM_CONT_MAX_PLANES;
constexpr int CONT_BF = VSM_CONT_BAND_FIELDS;
constexpr double CONT_C2 = 1.4388;                  // _MTCKD_C2, cm K

// what a launch reads from its kernel arguments: pointers and flags of the set, by value
struct cont_set {
  const double* table[CONT_TABLES];   // [nT_k, nSpec]
  int nT[CONT_TABLES];
  double* plane[CONT_PLANES];         // [Nz, nSpec]
  int accumulate[CONT_PLANES];
};

// planes of the linearized call: 0 tau, 1 d/dT, 2 d/dp, 3 .. the vmr planes; ddz_plane (or -1) d/dΔz.  Forward: plane 0 alone.
// rows [nTables, Nz, 2] (j0, j1), w [nTables, Nz], A and B [nPlanes, nTables, Nz]; band_layer [Nz, CONT_BF] =
// (T, T_ref / T, S, F, 2S/p, 2F/p, dS/dv, dF/dv, S/Δz, F/Δz) with S and F the layer factors of the self and the foreign term.
template <int LIN>
__global__ __launch_bounds__(CONT_TILE) void k_continuum(int nSpec, int Nz, int nTables, int nPlanes, cont_set set,
                                                         const int* __restrict__ rows, const double* __restrict__ w,
                                                         const double* __restrict__ A, const double* __restrict__ B,
                                                         const double* __restrict__ nu, const double* __restrict__ C_self,
                                                         const double* __restrict__ C_for, const double* __restrict__ texp,
                                                         const double* __restrict__ band_layer, int h2o_plane, int ddz_plane) {
  // the tile's per-layer coefficients pass through LDS: every lane reads the same word (a broadcast), no lane holds them
  constexpr int NP = LIN ? CONT_PLANES : 1;
  __shared__ double sA[NP][CONT_TABLES][CONT_LAYERS], sB[CONT_TABLES][CONT_LAYERS], sW[CONT_TABLES][CONT_LAYERS];
  __shared__ double sL[CONT_LAYERS][CONT_BF];
  __shared__ const double* sR[CONT_TABLES][CONT_LAYERS][2];   // the two table rows of (k, layer)
  const int z0 = blockIdx.y * CONT_LAYERS, nz = min(CONT_LAYERS, Nz - z0);
  for (int i = threadIdx.x; i < nPlanes * nTables * nz; i += CONT_TILE) {
    const int m = i / (nTables * nz), r = i - m * (nTables * nz), k = r / nz, zl = r - k * nz;
    const long long mkz = ((long long)m * nTables + k) * Nz + z0 + zl;
    sA[m][k][zl] = A[mkz];
    if (LIN && m == 1) sB[k][zl] = B[mkz];
    if (m == 0) {
      const long long kz = (long long)k * Nz + z0 + zl;
      const int top = set.nT[k] - 1;
      sW[k][zl] = w[kz];
      sR[k][zl][0] = set.table[k] + (long long)min(max(rows[2 * kz], 0), top) * nSpec;   // (never outside the table)
      sR[k][zl][1] = set.table[k] + (long long)min(max(rows[2 * kz + 1], 0), top) * nSpec;
    }
  }
  const bool band = C_self != nullptr;
  if (band && (int)threadIdx.x < nz * CONT_BF)
    sL[threadIdx.x / CONT_BF][threadIdx.x % CONT_BF] = band_layer[(long long)z0 * CONT_BF + threadIdx.x];
  __syncthreads();
  const int s = blockIdx.x * CONT_TILE + threadIdx.x;
  if (s >= nSpec) return;
  const double v_nu = band ? nu[s] : 0.0, cs = band ? C_self[s] : 0.0, cf = band ? C_for[s] : 0.0, te = band ? texp[s] : 0.0;
#pragma unroll 1   // (unrolled, the math calls' constants of several layers outgrow the scalar registers)
  for (int zl = 0; zl < nz; ++zl) {
    const int z = z0 + zl;
    // the tables' two rows at this point: s_k and the slope b - a
    double sk[CONT_TABLES], dk[CONT_TABLES];
#pragma unroll
    for (int k = 0; k < CONT_TABLES; ++k) {
      sk[k] = 0.0;
      dk[k] = 0.0;
      if (k < nTables) {
        const double wk = sW[k][zl];
        const double a = sR[k][zl][0][s], b = sR[k][zl][1][s];
        sk[k] = (1.0 - wk) * a + wk * b;
        if (LIN) dk[k] = b - a;
      }
    }
    // the band: g_self = nu tanh(x) C_self (T_ref / T)^texp, g_for = nu tanh(x) C_for, and the T factors of both
    double gs = 0.0, gf = 0.0, ts = 0.0, tf = 0.0;
    const double* bl = sL[zl];
    if (band) {
      const double T = bl[0];
      const double x = CONT_C2 * v_nu / (2.0 * T);
      const double rad = v_nu * tanh(x);
      gs = rad * cs * pow(bl[1], te);
      gf = rad * cf;
      if (LIN) {
        // d ln(nu tanh x) / dT = -(2x / T) / sinh(2x), never through 1 - tanh^2; 2x / sinh(2x) -> 1 at nu = 0, where rad = 0
        const double x2 = x + x;
        const double q = x2 == 0.0 ? 1.0 : x2 / sinh(x2);
        const double invT = 1.0 / T;
        ts = -((q + te + 1.0) * invT);   // ... - texp / T of the power, - 1 / T of n_air
        tf = -((q + 1.0) * invT);
      }
    }
    const long long o = (long long)z * nSpec + s;
#pragma unroll 1
    for (int m = 0; m < nPlanes; ++m) {
      double acc = set.accumulate[m] ? set.plane[m][o] : 0.0;
#pragma unroll
      for (int k = 0; k < CONT_TABLES; ++k)
        if (k < nTables) {
          acc = acc + sk[k] * sA[m][k][zl];
          if (LIN && m == 1) acc = acc + dk[k] * sB[k][zl];
        }
      if (band) {
        if (m == 0) {
          acc = acc + gs * bl[2];
          acc = acc + gf * bl[3];
        } else if (m == 1) {
          acc = acc + (gs * bl[2]) * ts;
          acc = acc + (gf * bl[3]) * tf;
        } else if (m == 2) {
          acc = acc + gs * bl[4];
          acc = acc + gf * bl[5];
        } else if (m == h2o_plane) {
          acc = acc + gs * bl[6];
          acc = acc + gf * bl[7];
        } else if (m == ddz_plane) {
          acc = acc + gs * bl[8];
          acc = acc + gf * bl[9];
        }
      }
      set.plane[m][o] = acc;
    }
  }
}

// out [K, Nz, nSpec] += plane [Nz, nSpec] tab [K, Nz]
__global__ __launch_bounds__(256) void k_slots_add(int nSpec, int Nz, const double* __restrict__ plane, const double* __restrict__ tab,
                                                   double* __restrict__ out) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= nSpec) return;
  const int iz = (int)blockIdx.y, k = (int)blockIdx.z;
  const long long o = (long long)iz * nSpec + i, ko = (long long)k * Nz * nSpec + o;
  out[ko] = out[ko] + plane[o] * tab[(long long)k * Nz + iz];
}

template <int LIN>
static int continuum_entry(const char* fn, int nSpec, int Nz, int nTables, const double* const* tables, const int* nT,
                           const int* rows, const double* w, int nPlanes, const double* A, const double* B, const double* nu,
                           const double* C_self, const double* C_for, const double* texp, const double* band_layer, int h2o_plane,
                           int ddz_plane, const int* accumulate, double* const* planes, void* stream) {
  VSM_REQUIRE(nSpec >= 1 && Nz >= 1, "%s: nSpec = %d, Nz = %d must be >= 1", fn, nSpec, Nz);
  VSM_REQUIRE(Nz <= 65535, "%s: Nz = %d above 65535 layers", fn, Nz);
  VSM_REQUIRE(nTables >= 0 && nTables <= CONT_TABLES, "%s: nTables = %d outside 0 .. %d", fn, nTables, CONT_TABLES);
  const bool band = nu || C_self || C_for || texp || band_layer;
  VSM_REQUIRE(!band || (nu && C_self && C_for && texp && band_layer), "%s: a band needs nu, C_self, C_for, texp and band_layer", fn);
  VSM_REQUIRE(nTables >= 1 || band, "%s: an empty set (no table, no band)", fn);
  VSM_REQUIRE(nTables == 0 || (tables && nT && rows && w && A && (!LIN || B)), "%s: null pointer", fn);
  VSM_REQUIRE(accumulate && planes, "%s: null pointer", fn);
  VSM_REQUIRE(LIN ? (nPlanes >= 3 && nPlanes <= CONT_PLANES) : nPlanes == 1, "%s: nPlanes = %d outside 3 .. %d", fn, nPlanes,
              CONT_PLANES);
  if (LIN) {
    VSM_REQUIRE(band ? (h2o_plane >= 3 && h2o_plane < nPlanes) : h2o_plane == -1,
                "%s: h2o_plane = %d (3 .. nPlanes - 1 with a band, -1 without)", fn, h2o_plane);
    VSM_REQUIRE(ddz_plane == -1 || (ddz_plane >= 3 && ddz_plane < nPlanes && ddz_plane != h2o_plane),
                "%s: ddz_plane = %d (-1, or 3 .. nPlanes - 1 and not h2o_plane)", fn, ddz_plane);
  }
  cont_set set = {};
  for (int k = 0; k < nTables; ++k) {
    VSM_REQUIRE(tables[k] && nT[k] >= 1, "%s: table %d is null or has nT = %d < 1", fn, k, nT[k]);
    set.table[k] = tables[k];
    set.nT[k] = nT[k];
  }
  for (int m = 0; m < nPlanes; ++m) {
    VSM_REQUIRE(planes[m], "%s: plane %d is null", fn, m);
    VSM_REQUIRE(accumulate[m] == 0 || accumulate[m] == 1, "%s: accumulate[%d] = %d (0 writes, 1 adds)", fn, m, accumulate[m]);
    for (int n = 0; n < m; ++n) VSM_REQUIRE(planes[n] != planes[m], "%s: planes %d and %d are one array", fn, n, m);
    set.plane[m] = planes[m];
    set.accumulate[m] = accumulate[m];
  }
  const dim3 g((unsigned)((nSpec + CONT_TILE - 1) / CONT_TILE), (unsigned)((Nz + CONT_LAYERS - 1) / CONT_LAYERS)), b(CONT_TILE);
  hipLaunchKernelGGL((k_continuum<LIN>), g, b, 0, as_stream(stream), nSpec, Nz, nTables, nPlanes, set, rows, w, A, B, nu, C_self, C_for,
                     texp, band_layer, h2o_plane, ddz_plane);
  VSM_LAUNCH_CHECK("k_continuum");
  return VSM_OK;
}

}  // namespace vsm

using namespace vsm;

extern "C" int vsm_absorption_continuum_layers(void) { return CONT_LAYERS; }

extern "C" int vsm_absorption_continuum(int nSpec, int Nz, int nTables, const double* const* tables, const int* nT, const int* rows,
                                        const double* w, const double* A, const double* nu, const double* C_self,
                                        const double* C_for, const double* texp, const double* band_layer, int accumulate,
                                        double* out, void* stream) {
  double* const planes[1] = {out};
  const int acc[1] = {accumulate};
  return continuum_entry<0>("vsm_absorption_continuum", nSpec, Nz, nTables, tables, nT, rows, w, 1, A, nullptr, nu, C_self, C_for,
                            texp, band_layer, -1, -1, acc, planes, stream);
}

extern "C" int vsm_absorption_continuum_lin(int nSpec, int Nz, int nTables, const double* const* tables, const int* nT,
                                            const int* rows, const double* w, int nPlanes, const double* A, const double* B,
                                            const double* nu, const double* C_self, const double* C_for, const double* texp,
                                            const double* band_layer, int h2o_plane, int ddz_plane, const int* accumulate,
                                            double* const* planes, void* stream) {
  return continuum_entry<1>("vsm_absorption_continuum_lin", nSpec, Nz, nTables, tables, nT, rows, w, nPlanes, A, B, nu, C_self,
                            C_for, texp, band_layer, h2o_plane, ddz_plane, accumulate, planes, stream);
}

extern "C" int vsm_absorption_profile_slots_add(int nSpec, int Nz, int K, const double* plane, const double* tab, double* out,
                                                void* stream) {
  const char* fn = "vsm_absorption_profile_slots_add";
  VSM_REQUIRE(nSpec >= 1 && Nz >= 1 && K >= 1, "%s: nSpec = %d, Nz = %d, K = %d must be >= 1", fn, nSpec, Nz, K);
  VSM_REQUIRE(Nz <= 65535 && K <= 65535, "%s: Nz = %d, K = %d above 65535", fn, Nz, K);
  VSM_REQUIRE(plane && tab && out, "%s: null pointer", fn);
  hipLaunchKernelGGL(k_slots_add, dim3((unsigned)((nSpec + 255) / 256), (unsigned)Nz, (unsigned)K), dim3(256), 0, as_stream(stream),
                     nSpec, Nz, plane, tab, out);
  VSM_LAUNCH_CHECK("k_slots_add");
  return VSM_OK;
}
