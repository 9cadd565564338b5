// The run object behind vsm_run_* (a CompositeLayer kept in the layer kernels' native strip layout, include/vsmartmom_hip.h) as the
// two kernel families see it: vsm_native.hip (FP64 records and arithmetic: FP64 models) and vsm_native32.hip (FP32 records and
// arithmetic: Float32 models).
#pragma once
#include <vector>

#include "vsm_internal.h"

namespace vsm {

constexpr int NSUB_MAX = VSM_MM_MAX;   // sub-problems per launch (gridDim.y)

struct nat_sub {
  int im;          // index of the Fourier moment in the run's list
  int m;
  int gsz, g[4];   // the Stokes components of the block
  unsigned uvmask;
  int n, rt, ks;
  int kz;          // k-steps over real streams (VSM_RUN_ZW_TAIL; else ks): ks - kz trailing k-steps cover zero-weight streams only
  size_t comp_off;   // elements (of the run's record type) from the workspace base
  int nv;                        // VSM_RUN_VIEW_ROWS: viewing rows that fall into this block (0: it carries no T-- rows at all)
  int vrow[VSM_RUN_VIEW_MAX];    // ... as local rows of the block, in the order of the run's list
};

// the viewing rows of the sub-problems of one launch / of the groups of one moment (local rows of a block: < 96)
// (dwords, four rows each: the kernels read them with scalar loads)
struct nview {
  int nv[NSUB_MAX];
  unsigned pk[NSUB_MAX][VSM_RUN_VIEW_MAX / 4];
  __host__ __device__ int row(int k, int v) const { return (int)((pk[k][v >> 2] >> (8 * (v & 3))) & 255u); }
  // index of local row `r` in the list of slot k, -1: not a viewing row
  __host__ __device__ int find(int k, int r) const {
    int at = -1;
    for (int v = 0; v < nv[k]; ++v) at = row(k, v) == r ? v : at;
    return at;
  }
};

}  // namespace vsm

struct vsm_run {
  const void *mu, *wt;     // the quadrature arrays of the caller (element type: elem_size)
  int N, ns, i_mu0;
  double mu0;
  int elem_size;           // 8: FP64 model (FP64 records and arithmetic), 4: Float32 model (FP32 records and arithmetic)
  int S, nm;
  unsigned flags;          // vsm_run_create_ex: VSM_RUN_SOURCES_ONLY, VSM_RUN_ZW_TAIL (FP64 runs; the latter dropped by vsm_run_import),
                           // vsm_run_create_view: VSM_RUN_VIEW_ROWS (FP64 runs)
  std::vector<int> view_rows;   // VSM_RUN_VIEW_ROWS: the global viewing rows
  std::vector<int> m;
  std::vector<vsm::nat_sub> subs;
  std::vector<std::vector<int>> classes;   // indices into subs with equal (n, gsz, uvmask)
  void* ws;
  size_t ws_elems;
  int layers = 0;                // vsm_run_layer calls so far
  int imports = 0;               // vsm_run_import calls so far
  std::vector<char> pure_diag;   // per sub-problem: its composite is still (R = 0, T = diag, J = 0): only diagonal steps so far
  bool guard_once = false;       // vsm_run_guard_once: k_coupling_guard on the first layer step alone (dropped by vsm_run_import)
  // vsm_run_counters: launches so far -- k_native_export per moment, k_native_export_src, surface interactions, k_coupling_guard
  int exports_full = 0, exports_src = 0, surface_ia = 0, guards = 0;
};

namespace vsm {

constexpr int NATIVE_MAX_ROWS = 96;      // FP64 family (vsm_native.hip): blocks of up to six row tiles
constexpr int NATIVE32_MAX_ROWS = 128;   // FP32 family (vsm_native32.hip): up to eight row tiles

// Geometry of a block of n rows, in elements of the record type (the same for both families).  Row tiles: n = 13..16, 29..32, ...
// (a multiple of four k-steps) take ks / 4 row tiles without spare columns (mat-vec source path) instead of one row tile more for
// the two rider columns -- as the launchers of the layer kernels choose it.
constexpr int rt_of(int n) {
  const int ks = (n + 3) / 4;
  return (ks % 4 == 0 && ks >= 4) ? ks / 4 : (4 * ks + 2 + 15) / 16;
}
constexpr size_t comp_stride_rt(int rt) { return (size_t)4 * (16 * rt) * (16 * rt) + 2 * 16 * rt; }   // native composite of a point
constexpr size_t pre_stride_rt(int rt) { return (size_t)2 * (16 * rt) * (16 * rt) + 3 * 16 * rt; }    // pre-pass record of a point

// the sub-problems of one pre-pass launch (both elemental pre-pass kernels)
template <typename T>
struct nsub_pre {
  int m, gsz;
  int g[4];
  zsrc<T> z;
};
template <typename T>
struct npre_args {
  nsub_pre<T> s[NSUB_MAX];
};

// ---- what the run driver (vsm_native.hip) needs from the FP32 family (vsm_native32.hip) ---------------------------------------
void native32_launch_pre(int rt, bool mix, const quad<float>& q, int S, int nsub, int n, int ndoubl, const float* dtau,
                         const float* varpi, const float* tau_sum, const float* F0, const npre_args<float>& a, float* pre,
                         hipStream_t st);
int native32_launch_layer(int ks, int S, int nsub, int n, unsigned uvmask, int gsz, int ndoubl, int toa, const float* pre,
                          float* const* comps, int* status, hipStream_t st);   // comps: NSUB_MAX native composites

}  // namespace vsm
