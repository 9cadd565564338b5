// delta-BGE truncation of a phase matrix's Greek coefficients: src/Scattering/truncate_phase.jl on the device, FP64 only (it sits
// behind vsm_mie_nai2, which is FP64 only).  Both of the reference's variants: truncate_phase (all nodes, weights w / f^2: what it
// applies to Mie optics) and truncate_phase_lowconf (the nodes outside the forward cone, weights (w / max(|f|, 1e-8))^2).
//   vsm_dbge_work_elems  size of the caller's work buffer
//   vsm_truncate_dbge    the three stages below on the caller's stream
// The three fits (beta on P, gamma and epsilon on fac P2) are weighted least-squares problems over the angle nodes.  Each is solved
// through its normal equations [A | b] = B B^T, where B holds the basis functions scaled by the square root of the node's weight
// and one more row that turns the same product into the right-hand side.
// Stage 1  k_dbge_basis  one lane per angle node.  f11, f12, f34 are either bulk_f / scal[0] of vsm_mie_nai2 or reconstructed from
//                        the n_mu coefficients (reconstruct_phase, mie_helper_functions.jl:415-446) with the recurrences of
//                        compute_legendre_poly as k_mie_greek has them: their angle-independent factors once per 64 moments, one
//                        lane per moment.  Then the first l_max moments are walked again and the three planes B [system][row][angle]
//                        are written, angle fastest, exact zeros for the padding rows, the padding angles, the nodes a
//                        low-confidence fit leaves out and a skipped system.  Every workgroup finds the skipped systems (a gamma or
//                        epsilon series of exact zeros from l = 2 on); workgroup 0 writes them to info.
// Stage 2  k_dbge_gram   [A | b] = B B^T on v_mfma_f64_16x16x4, one wave per (16 x 16 tile on or above the diagonal, chunk of 128
//                        angles, system).  Fragments as in k_mie_bulk; lane group kq walks its own quarter of the chunk, so that a
//                        lane reads consecutive doubles of its row, one k-step ahead of their use.  A chunk's tile goes to the work
//                        buffer; nothing is added across workgroups here.
// Stage 3  k_dbge_solve  one workgroup per system: sums the chunks' tiles in chunk order into LDS (bit-identical from call to call),
//                        Cholesky in its L D L^T form (no column scaling: one barrier per column) with the right-hand side
//                        carried as one more row (the forward substitution comes with the factorisation), back substitution,
//                        and the closing formulas of truncate_phase.jl:255-262: the beta workgroup writes c0, alpha, beta,
//                        delta, zeta and scal_t, the other two their own vector.
#include "vsm_common.h"
#include "vsm_internal.h"

namespace vsm {

constexpr int DBGE_KC = 128;             // angles per chunk of stage 2 (a multiple of 64: stage 1's workgroups tile a chunk)
constexpr int DBGE_KQ = DBGE_KC / 4;     // k-steps per chunk = consecutive angles of one lane group
constexpr int DBGE_NT = 256;             // threads of stage 3

__host__ __device__ inline long long dbge_up(long long a, long long m) { return (a + m - 1) / m * m; }

struct dbge_layout {
  long long RP, KP, CH;                  // padded rows of a system (basis + right-hand side), padded angles, angle chunks
  long long o_basis, o_part, total;
};
static dbge_layout dbge_make_layout(int n_mu, int l_max) {
  dbge_layout L;
  L.RP = dbge_up(l_max + 1, 16);
  L.CH = (n_mu + DBGE_KC - 1) / DBGE_KC;
  L.KP = L.CH * DBGE_KC;
  L.o_basis = 0;
  L.o_part = L.o_basis + 3 * L.RP * L.KP;
  L.total = L.o_part + L.CH * 3 * L.RP * L.RP;
  return L;
}
// stage 3's LDS: the lower triangle of [A | b] as rows of odd stride, and the solution
static size_t dbge_lds_bytes(int l_max) { return ((size_t)(l_max + 1) * ((l_max + 1) | 1) + (l_max + 1)) * sizeof(double); }

// does the series c[2 .. n) hold exact zeros only?  (the same answer in every thread of the workgroup)
__device__ __forceinline__ bool dbge_zero_series(const double* __restrict__ c, int n) {
  int nz = 0;
  for (int l = 2 + threadIdx.x; l < n; l += blockDim.x) nz |= (c[l] != 0.0);
  return __syncthreads_or(nz) == 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 1
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_dbge_basis(int n_mu, int l_max, int lowconf, double cos_delta, long long RP, long long KP,
                                                  const double* __restrict__ greek, const double* __restrict__ bulk_f,
                                                  const double* __restrict__ scal, const double* __restrict__ mu_,
                                                  const double* __restrict__ w_mu, double* __restrict__ basis,
                                                  int* __restrict__ info) {
  __shared__ double cf[5][64];          // per moment of a chunk of 64: 1 / (l + 1), 1 / (l - 1) of the recurrences, then fac and the coefficients
  const int lane = threadIdx.x;
  const long long ia = (long long)blockIdx.x * 64 + lane;
  const bool skip_g = dbge_zero_series(greek + 2LL * n_mu, n_mu);
  const bool skip_e = dbge_zero_series(greek + 4LL * n_mu, n_mu);
  if (blockIdx.x == 0 && lane == 0) {
    info[0] = 0;
    info[1] = skip_g ? 1 : 0;
    info[2] = skip_e ? 1 : 0;
  }
  const bool live = ia < n_mu;
  const double x = live ? mu_[ia] : 0.0;
  const double w = live ? w_mu[ia] : 0.0;
  const bool on = live && (!lowconf || x < cos_delta);
  double f11 = 0.0, f12 = 0.0, f34 = 0.0;
  if (bulk_f) {
    const double csca = scal[0];
    if (live) {
      f11 = bulk_f[ia] / csca;
      f12 = bulk_f[2LL * n_mu + ia] / csca;
      f34 = bulk_f[3LL * n_mu + ia] / csca;
    }
  } else {                               // reconstruct_phase over all n_mu moments
    double p0a = 0.0, p0b = 0.0, p2a = 0.0, p2b = 0.0;
    for (int c0 = 0; c0 < n_mu; c0 += 64) {
      const int c = c0 + lane;
      const double dl = (double)(c - 1);
      const bool in = c < n_mu;
      const double dc = (double)c;
      const double fac = (in && c >= 2) ? sqrt(1.0 / ((dc - 1) * dc * (dc + 1) * (dc + 2))) : 0.0;
      __syncthreads();
      cf[0][lane] = c >= 1 ? 1.0 / (dl + 1) : 0.0;
      cf[1][lane] = c >= 3 ? 1.0 / (dl - 1) : 0.0;
      cf[2][lane] = in ? greek[1LL * n_mu + c] : 0.0;
      cf[3][lane] = in ? fac * greek[2LL * n_mu + c] : 0.0;
      cf[4][lane] = in ? fac * greek[4LL * n_mu + c] : 0.0;
      __syncthreads();
      const int nj = min(64, n_mu - c0);
      for (int j = 0; j < nj; ++j) {
        const int cc = c0 + j, l = cc - 1;
        const double ia_ = (2 * l + 1) * x;
        double p0 = (ia_ * p0b - l * p0a) * cf[0][j];
        double p2 = (ia_ * p2b - (l + 2) * p2a) * cf[1][j];
        p0 = cc == 0 ? 1.0 : p0;
        p2 = cc == 2 ? 3.0 * (1.0 - x * x) : p2;
        p0a = p0b; p0b = p0;
        p2a = p2b; p2b = p2;
        f11 += p0 * cf[2][j];
        f12 += p2 * cf[3][j];
        f34 += p2 * cf[4][j];
      }
    }
  }
  // the square root of the node's weight in each system, and the entry of the row that makes the right-hand side
  double s[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
  if (on) {
    const double f[3] = {f11, f12, f34};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (lowconf) {                     // W = w / max(|y|, 1e-8):  A = sum W^2 B B,  b = sum W^2 B y
        s[k] = w / fmax(fabs(f[k]), 1e-8);
        r[k] = s[k] * f[k];
      } else {                           // A = sum w B B / f^2,  b = sum w B / f
        s[k] = sqrt(w) / f[k];
        r[k] = sqrt(w);
      }
    }
    // the weights w / f11^2 are relative errors of a phase function: a node where it is not positive (or not finite) fails the fit
    if (!lowconf && !(f11 > 0.0 && f11 <= 1.79769313486231570815e308)) r[0] = __builtin_nan("");
  }
  if (skip_g) s[1] = r[1] = 0.0;
  if (skip_e) s[2] = r[2] = 0.0;
  const long long plane = RP * KP;
  double* b0 = basis + ia;               // (ia < KP: the grid is KP / 64 workgroups)
  double p0a = 0.0, p0b = 0.0, p2a = 0.0, p2b = 0.0;
  for (int c0 = 0; c0 < l_max; c0 += 64) {
    const int c = c0 + lane;
    const double dl = (double)(c - 1), dc = (double)c;
    __syncthreads();
    cf[0][lane] = c >= 1 ? 1.0 / (dl + 1) : 0.0;
    cf[1][lane] = c >= 3 ? 1.0 / (dl - 1) : 0.0;
    cf[2][lane] = c >= 2 ? sqrt(1.0 / ((dc - 1) * dc * (dc + 1) * (dc + 2))) : 0.0;
    __syncthreads();
    const int nj = min(64, l_max - c0);
    for (int j = 0; j < nj; ++j) {
      const int cc = c0 + j, l = cc - 1;
      const double ia_ = (2 * l + 1) * x;
      double p0 = (ia_ * p0b - l * p0a) * cf[0][j];
      double p2 = (ia_ * p2b - (l + 2) * p2a) * cf[1][j];
      p0 = cc == 0 ? 1.0 : p0;
      p2 = cc == 2 ? 3.0 * (1.0 - x * x) : p2;
      p0a = p0b; p0b = p0;
      p2a = p2b; p2b = p2;
      b0[(long long)cc * KP] = on ? s[0] * p0 : 0.0;
      if (cc >= 2) {
        const double q = cf[2][j] * p2;
        b0[plane + (long long)(cc - 2) * KP] = (on && !skip_g) ? s[1] * q : 0.0;
        b0[2 * plane + (long long)(cc - 2) * KP] = (on && !skip_e) ? s[2] * q : 0.0;
      }
    }
  }
  b0[(long long)l_max * KP] = r[0];
  b0[plane + (long long)(l_max - 2) * KP] = r[1];
  b0[2 * plane + (long long)(l_max - 2) * KP] = r[2];
  for (long long row = l_max + 1; row < RP; ++row) b0[row * KP] = 0.0;
  for (long long row = l_max - 1; row < RP; ++row) {
    b0[plane + row * KP] = 0.0;
    b0[2 * plane + row * KP] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 2
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_dbge_gram(int l_max, long long RP, long long KP, const double* __restrict__ basis,
                                                 const int* __restrict__ info, double* __restrict__ part) {
  using MM = mfma<double>;
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  const int sys = blockIdx.z;
  const long long chunk = blockIdx.y;
  // tile pair (ti <= tj) number blockIdx.x, counted row by row
  const int T = (int)(RP / 16);
  int ti = 0, rest = blockIdx.x;
  while (rest >= T - ti) {
    rest -= T - ti;
    ++ti;
  }
  const int tj = ti + rest;
  const int rows = (sys == 0 ? l_max : l_max - 2) + 1;         // rows of [A | b] that stage 3 reads
  if (ti * 16 >= rows || tj * 16 >= rows) return;              // (the whole wave)
  MM::acc_t acc = acc_zero<double>();
  if (info[sys] != 1) {
    const double* pa = basis + (sys * RP + ti * 16 + col) * KP + chunk * DBGE_KC + kq * DBGE_KQ;
    const double* pb = basis + (sys * RP + tj * 16 + col) * KP + chunk * DBGE_KC + kq * DBGE_KQ;
    double na = pa[0], nb = pb[0];
#pragma unroll 8
    for (int s = 0; s < DBGE_KQ; ++s) {
      const double a = na, b = nb;
      const int sn = s + 1 < DBGE_KQ ? s + 1 : s;              // (the last k-step loads its own elements again)
      na = pa[sn];
      nb = pb[sn];
      acc = MM::mma(a, b, acc);
    }
  }
  double* out = part + ((chunk * 3 + sys) * RP + ti * 16) * RP + tj * 16 + col;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(long long)MM::crow(lane, r) * RP] = acc[r];
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 3
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DBGE_NT) void k_dbge_solve(int n_mu, int l_max, long long RP, long long CH,
                                                       const double* __restrict__ part, const double* __restrict__ greek,
                                                       double* __restrict__ greek_t, double* __restrict__ scal_t,
                                                       int* __restrict__ info) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ int bad;
  const int t = threadIdx.x, sys = blockIdx.x;
  const int n = sys == 0 ? l_max : l_max - 2;                  // unknowns; row n of the triangle is the right-hand side
  const int off = sys == 0 ? 0 : 2;                            // first coefficient the system fits
  const int ST = (l_max + 1) | 1;
  double* A = reinterpret_cast<double*>(lds_raw);
  double* xs = A + (size_t)(l_max + 1) * ST;
  double* gt = greek_t + (long long)(sys == 0 ? 1 : sys == 1 ? 2 : 4) * l_max;
  if (sys != 0 && info[sys] == 1) {                            // a series of exact zeros stays one
    for (int l = t; l < l_max; l += DBGE_NT) gt[l] = 0.0;
    return;
  }
  if (t == 0) bad = 0;
  // [A | b]: the lower triangle from the tiles on and above the diagonal, chunks added in chunk order
  int nonfinite = 0;
  const long long tile_plane = RP * RP;
  for (int e = t; e < (n + 1) * (n + 1); e += DBGE_NT) {
    const int k = e / (n + 1), i = e % (n + 1);
    if (i < k) continue;
    const double* p = part + sys * tile_plane + (long long)k * RP + i;
    double v = 0.0;
    for (long long ch = 0; ch < CH; ++ch) v += p[ch * 3 * tile_plane];
    A[i * ST + k] = v;
    nonfinite |= !(fabs(v) <= 1.79769313486231570815e308);
  }
  if (__syncthreads_or(nonfinite)) {
    if (t == 0) bad = 1;
  } else {
    const int tx = t & 15, ty = t >> 4;
    for (int j = 0; j < n; ++j) {
      const double d = A[j * ST + j];                          // (final since the barrier that ended step j - 1)
      if (!(d > 0.0 && d <= 1.79769313486231570815e308)) {     // the same value in every thread: all leave together
        if (t == 0) bad = 1;
        break;
      }
      // column j stays as it is, u_ij = l_ij d_j of A = L D L^T: step j reads it and writes only columns k > j, so one barrier
      // per column is enough
      const double invd = 1.0 / d;
      for (int i = j + 1 + ty; i <= n; i += 16) {
        const double lij = A[i * ST + j] * invd;
        const int kend = i < n ? i : n - 1;                    // (the right-hand side's row has no diagonal)
        for (int k = j + 1 + tx; k <= kend; k += 16) A[i * ST + k] -= lij * A[k * ST + j];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  const bool failed = bad != 0;
  if (!failed) {
    // row n now holds u_nj = d_j (D^-1 L^-1 b)_j;  L^T x = D^-1 L^-1 b backwards:  x_j = (u_nj - sum_{i > j} u_ij x_i) / d_j
    for (int j = n - 1; j >= 0; --j) {
      const double xj = A[n * ST + j] / A[j * ST + j];         // (final since the barrier that ended step j + 1)
      for (int i = t; i < j; i += DBGE_NT) A[n * ST + i] -= A[j * ST + i] * xj;
      if (t == 0) xs[j] = xj;
      __syncthreads();
    }
    for (int i = t; i < n; i += DBGE_NT) nonfinite |= !(fabs(xs[i]) <= 1.79769313486231570815e308);
  }
  const bool fail_all = failed || __syncthreads_or(nonfinite) != 0 || (sys == 0 && !(xs[0] != 0.0));
  if (t == 0) info[sys] = fail_all ? 2 : 0;
  const double qnan = __builtin_nan("");
  if (sys != 0) {
    for (int l = t; l < l_max; l += DBGE_NT) gt[l] = l < off ? 0.0 : (fail_all ? qnan : xs[l - off]);
    return;
  }
  // truncate_phase.jl:255-262
  const double c0 = fail_all ? qnan : xs[0];
  for (int l = t; l < l_max; l += DBGE_NT) {
    const double cl = fail_all ? qnan : xs[l];
    const double cut = greek[1LL * n_mu + l] - cl;             // beta - cl
    greek_t[0LL * l_max + l] = (greek[0LL * n_mu + l] - cut) / c0;
    greek_t[1LL * l_max + l] = cl / c0;
    greek_t[3LL * l_max + l] = (greek[3LL * n_mu + l] - cut) / c0;
    greek_t[5LL * l_max + l] = (greek[5LL * n_mu + l] - cut) / c0;
  }
  if (t == 0) {
    scal_t[0] = c0;
    scal_t[1] = 1.0 - c0;
  }
}

}  // namespace vsm

using namespace vsm;

static bool dbge_shape_ok(int n_mu, int l_max) { return l_max >= 3 && l_max <= VSM_DBGE_MAX_L && n_mu > l_max; }

extern "C" size_t vsm_dbge_work_elems(int n_mu, int l_max) {
  if (!dbge_shape_ok(n_mu, l_max)) return 0;
  return (size_t)dbge_make_layout(n_mu, l_max).total;
}

extern "C" int vsm_truncate_dbge(int n_mu, int l_max, int lowconf, double cos_delta, const double* greek, const double* bulk_f,
                                 const double* scal, const double* mu, const double* w_mu, double* greek_t, double* scal_t,
                                 int* info, double* work, void* stream) {
  if (l_max > VSM_DBGE_MAX_L) {
    set_error("vsm_truncate_dbge: l_max = %d above VSM_DBGE_MAX_L = %d", l_max, VSM_DBGE_MAX_L);
    return VSM_ERR_UNSUPPORTED;
  }
  VSM_REQUIRE(l_max >= 3, "vsm_truncate_dbge: l_max = %d < 3", l_max);
  VSM_REQUIRE(n_mu > l_max, "vsm_truncate_dbge: n_mu = %d <= l_max = %d (nothing to truncate)", n_mu, l_max);
  VSM_REQUIRE(lowconf >= 0 && lowconf <= n_mu, "vsm_truncate_dbge: lowconf = %d is no count of the %d nodes", lowconf, n_mu);
  VSM_REQUIRE(lowconf == 0 || lowconf >= l_max, "vsm_truncate_dbge: %d nodes below cos_delta = %g for l_max = %d unknowns", lowconf,
              cos_delta, l_max);
  VSM_REQUIRE((bulk_f == nullptr) == (scal == nullptr), "vsm_truncate_dbge: bulk_f and scal come together or not at all");
  VSM_REQUIRE(greek && mu && w_mu && greek_t && scal_t && info && work, "vsm_truncate_dbge: null pointer");
  const dbge_layout L = dbge_make_layout(n_mu, l_max);
  VSM_REQUIRE(L.CH <= 65535, "vsm_truncate_dbge: n_mu = %d above %d", n_mu, 65535 * DBGE_KC);
  const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_dbge_solve), dbge_lds_bytes(VSM_DBGE_MAX_L),
                                "hipFuncSetAttribute(k_dbge_solve)");
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  double* basis = work + L.o_basis;
  double* part = work + L.o_part;
  hipLaunchKernelGGL(k_dbge_basis, dim3((unsigned)(L.KP / 64)), dim3(64), 0, st, n_mu, l_max, lowconf, cos_delta, L.RP, L.KP, greek,
                     bulk_f, scal, mu, w_mu, basis, info);
  VSM_LAUNCH_CHECK("k_dbge_basis");
  const unsigned T = (unsigned)(L.RP / 16);
  hipLaunchKernelGGL(k_dbge_gram, dim3(T * (T + 1) / 2, (unsigned)L.CH, 3), dim3(64), 0, st, l_max, L.RP, L.KP, (const double*)basis,
                     (const int*)info, part);
  VSM_LAUNCH_CHECK("k_dbge_gram");
  hipLaunchKernelGGL(k_dbge_solve, dim3(3), dim3(DBGE_NT), dbge_lds_bytes(l_max), st, n_mu, l_max, L.RP, L.CH, (const double*)part,
                     greek, greek_t, scal_t, info);
  VSM_LAUNCH_CHECK("k_dbge_solve");
  return VSM_OK;
}
