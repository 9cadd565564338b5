// delta-BGE truncation of a phase matrix's Greek coefficients: src/Scattering/truncate_phase.jl on the device, FP64 only (it sits
// behind vsm_mie_nai2, which is FP64 only).  Both of the reference's variants: truncate_phase (all nodes, weights w / f^2: what it
// applies to Mie optics) and truncate_phase_lowconf (the nodes outside the forward cone, weights (w / max(|f|, 1e-8))^2).
//   vsm_dbge_work_elems  size of the caller's work buffer
//   vsm_truncate_dbge    the three stages below on the caller's stream
//   vsm_truncate_dbge_lin  the same and, behind them, stages 4 and 5: the derivatives of the outputs for four parameters
//                        (truncate_phase_lin.jl).  With B the rows of stage 1 (A = B B^T), t = B^T x and
//                        g_slot = (f'_slot / f) (2 t - sqrt(w)):  b' - A' x = B g_slot, so x'_slot = A^-1 B g_slot -- no second
//                        Gram product; the four right-hand sides go through the factor stage 3 holds.
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
  long long o_fd, o_fac, o_x, o_rhs, total_lin;      // the linearized call's four more regions, behind the forward call's
};
static dbge_layout dbge_make_layout(int n_mu, int l_max) {
  dbge_layout L;
  L.RP = dbge_up(l_max + 1, 16);
  L.CH = (n_mu + DBGE_KC - 1) / DBGE_KC;
  L.KP = L.CH * DBGE_KC;
  L.o_basis = 0;
  L.o_part = L.o_basis + 3 * L.RP * L.KP;
  L.total = L.o_part + L.CH * 3 * L.RP * L.RP;
  L.o_fd = L.total;                                  // [system][slot][angle] f', [system][angle] 1 / f, [angle] sqrt(w)
  L.o_fac = L.o_fd + 16 * L.KP;                      // [system][row][column] the factored triangles
  L.o_x = L.o_fac + 3LL * l_max * l_max;             // [system][row] the solutions
  L.o_rhs = L.o_x + 3LL * l_max;                     // [chunk][system][slot][row] the chunks' B g
  L.total_lin = L.o_rhs + L.CH * 3 * 4 * L.RP;
  return L;
}
// stage 3's LDS: the lower triangle of [A | b] as rows of odd stride, and the solution
static size_t dbge_lds_bytes(int l_max) { return ((size_t)(l_max + 1) * ((l_max + 1) | 1) + (l_max + 1)) * sizeof(double); }
// stage 5's LDS: the same triangle and four right-hand sides
static size_t dbge_lin_lds_bytes(int l_max) { return dbge_lds_bytes(l_max) + (size_t)4 * l_max * sizeof(double); }

// does the series c[2 .. n) hold exact zeros only?  (the same answer in every thread of the workgroup)
__device__ __forceinline__ bool dbge_zero_series(const double* __restrict__ c, int n) {
  int nz = 0;
  for (int l = 2 + threadIdx.x; l < n; l += blockDim.x) nz |= (c[l] != 0.0);
  return __syncthreads_or(nz) == 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 1
// ---------------------------------------------------------------------------------------------------------------------
// LIN (lowconf = 0 only): a grid of five rows of workgroups.  Row 0 is the forward workgroup and also leaves 1 / f per system
// (planes 12 .. 14 of fd) and sqrt(w) (plane 15), exact zeros in the padding angles and in a skipped system.  Row 1 + slot runs the
// same text on the slot's derivatives up to f11, f12, f34 -- bulk_f_dot and scal_dot as k_mie_greek<true> normalises them, or the
// reconstruction from the slot's n_mu derivative coefficients -- and leaves them as f' [system][slot][angle] (planes 0 .. 11),
// exact zeros in the padding angles.
template <bool LIN>
__global__ __launch_bounds__(64) void k_dbge_basis(int n_mu, int l_max, int lowconf, double cos_delta, long long RP, long long KP,
                                                  const double* __restrict__ greek, const double* __restrict__ bulk_f,
                                                  const double* __restrict__ scal, const double* __restrict__ mu_,
                                                  const double* __restrict__ w_mu, double* __restrict__ basis,
                                                  int* __restrict__ info, const double* __restrict__ greek_dot,
                                                  const double* __restrict__ bulk_f_dot, const double* __restrict__ scal_dot,
                                                  double* __restrict__ fd) {
  __shared__ double cf[5][64];          // per moment of a chunk of 64: 1 / (l + 1), 1 / (l - 1) of the recurrences, then fac and the coefficients
  const int lane = threadIdx.x;
  const long long ia = (long long)blockIdx.x * 64 + lane;
  const int slot = LIN ? (int)blockIdx.y - 1 : -1;             // (the same value in every thread)
  const double* __restrict__ series = greek;                   // the coefficients the reconstruction sums
  if constexpr (LIN) {
    if (slot >= 0) series = greek_dot + (long long)slot * 6 * n_mu;
  }
  bool skip_g = false, skip_e = false;
  if (slot < 0) {
    skip_g = dbge_zero_series(greek + 2LL * n_mu, n_mu);
    skip_e = dbge_zero_series(greek + 4LL * n_mu, n_mu);
    if (blockIdx.x == 0 && lane == 0) {
      info[0] = 0;
      info[1] = skip_g ? 1 : 0;
      info[2] = skip_e ? 1 : 0;
    }
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
      if constexpr (LIN) {
        if (slot >= 0) {                 // (f' - f C_sca') / C_sca of the unnormalised f', as k_mie_greek<true> has it
          const double* bd = bulk_f_dot + (long long)slot * 4 * n_mu;
          const double cd = scal_dot[3 * slot];
          f11 = (bd[ia] - f11 * cd) / csca;
          f12 = (bd[2LL * n_mu + ia] - f12 * cd) / csca;
          f34 = (bd[3LL * n_mu + ia] - f34 * cd) / csca;
        }
      }
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
      cf[2][lane] = in ? series[1LL * n_mu + c] : 0.0;
      cf[3][lane] = in ? fac * series[2LL * n_mu + c] : 0.0;
      cf[4][lane] = in ? fac * series[4LL * n_mu + c] : 0.0;
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
  if constexpr (LIN) {
    if (slot >= 0) {                     // a derivative row of workgroups ends here
      fd[(0 + slot) * KP + ia] = live ? f11 : 0.0;
      fd[(4 + slot) * KP + ia] = live ? f12 : 0.0;
      fd[(8 + slot) * KP + ia] = live ? f34 : 0.0;
      return;
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
  if constexpr (LIN) {
    const double f[3] = {f11, f12, f34};
    const bool keep[3] = {live, live && !skip_g, live && !skip_e};
#pragma unroll
    for (int k = 0; k < 3; ++k) fd[(12 + k) * KP + ia] = keep[k] ? 1.0 / f[k] : 0.0;
    fd[15 * KP + ia] = live ? sqrt(w) : 0.0;
  }
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
// LIN: a solved system also leaves its factored triangle (column j as l_ij d_j, the diagonal d) in fac [system][row][column] and its
// solution in xsol [system][row], for stages 4 and 5.
template <bool LIN>
__global__ __launch_bounds__(DBGE_NT) void k_dbge_solve(int n_mu, int l_max, long long RP, long long CH,
                                                       const double* __restrict__ part, const double* __restrict__ greek,
                                                       double* __restrict__ greek_t, double* __restrict__ scal_t,
                                                       int* __restrict__ info, double* __restrict__ fac,
                                                       double* __restrict__ xsol) {
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
  if constexpr (LIN) {
    if (!fail_all) {
      double* fo = fac + (long long)sys * l_max * l_max;
      for (int e = t; e < n * n; e += DBGE_NT) {
        const int i = e / n, k = e % n;
        if (k <= i) fo[i * l_max + k] = A[i * ST + k];
      }
      for (int i = t; i < n; i += DBGE_NT) xsol[sys * l_max + i] = xs[i];
    }
  }
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

// ---------------------------------------------------------------------------------------------------------------------
// stage 4 (linearized call)
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (chunk of 128 angles, system).  t_k = sum_j B_jk x_j, a lane per node and half of the rows each, the halves
// added in a fixed order; g_slot,k = f'_slot,k (1 / f_k) (2 t_k - sqrt(w_k)); then the chunk's B g for every row of the system on
// v_mfma_f64_16x16x4, one wave per tile of 16 rows: the A fragment is stage 2's (a lane reads consecutive doubles of its row),
// the B fragment holds g in columns 0 .. 3 and zeros in the other twelve.
__global__ __launch_bounds__(256) void k_dbge_lin_rhs(int l_max, long long RP, long long KP, const double* __restrict__ basis,
                                                     const double* __restrict__ fd, const double* __restrict__ xsol,
                                                     const int* __restrict__ info, double* __restrict__ rhs) {
  using MM = mfma<double>;
  __shared__ double xs[VSM_DBGE_MAX_L];
  __shared__ double th[DBGE_KC];
  __shared__ double g[4][DBGE_KC];
  const int t = threadIdx.x, sys = blockIdx.y;
  const long long chunk = blockIdx.x;
  if (info[sys] != 0) return;                                  // skipped or failed: stage 5 reads nothing of it
  const int n = sys == 0 ? l_max : l_max - 2;
  for (int j = t; j < n; j += 256) xs[j] = xsol[sys * l_max + j];
  __syncthreads();
  const int k = t & (DBGE_KC - 1), half = t >> 7;
  const double* bk = basis + sys * RP * KP + chunk * DBGE_KC + k;
  double tk = 0.0;
#pragma unroll 4
  for (int j = half; j < n; j += 2) tk += bk[(long long)j * KP] * xs[j];
  if (half) th[k] = tk;
  __syncthreads();
  if (!half) {
    tk += th[k];
    const double* fk = fd + chunk * DBGE_KC + k;
    const double u = (2.0 * tk - fk[15 * KP]) * fk[(12 + sys) * KP];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q][k] = fk[(4 * sys + q) * KP] * u;
  }
  __syncthreads();
  const int lane = t & 63, wave = t >> 6, col = lane & 15, kq = lane >> 4;
  const int tiles = (n + 15) / 16;                             // (tiles * 16 <= RP: RP = up(l_max + 1, 16))
  for (int ti = wave; ti < tiles; ti += 4) {
    const double* pa = basis + (sys * RP + ti * 16 + col) * KP + chunk * DBGE_KC + kq * DBGE_KQ;
    MM::acc_t acc = acc_zero<double>();
    double na = pa[0];
#pragma unroll 8
    for (int s = 0; s < DBGE_KQ; ++s) {
      const double a = na;
      const int sn = s + 1 < DBGE_KQ ? s + 1 : s;
      na = pa[sn];
      const double b = col < 4 ? g[col & 3][kq * DBGE_KQ + s] : 0.0;
      acc = MM::mma(a, b, acc);
    }
    if (col < 4) {
      double* out = rhs + ((chunk * 3 + sys) * 4 + col) * RP + ti * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[MM::crow(lane, r)] = acc[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 5 (linearized call)
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup per system: the factor back into LDS, the chunks' B g added in chunk order, the four right-hand sides through
// L, D, L^T together (thread = (row, slot)), and the closing formulas of truncate_phase_lin.jl:183-207.
__global__ __launch_bounds__(DBGE_NT) void k_dbge_lin_solve(int n_mu, int l_max, long long RP, long long CH,
                                                           const double* __restrict__ fac, const double* __restrict__ rhs,
                                                           const double* __restrict__ greek_dot,
                                                           const double* __restrict__ greek_t, const double* __restrict__ scal_t,
                                                           double* __restrict__ greek_t_dot, double* __restrict__ scal_t_dot,
                                                           int* __restrict__ info) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int t = threadIdx.x, sys = blockIdx.x;
  const int n = sys == 0 ? l_max : l_max - 2;
  const int off = sys == 0 ? 0 : 2;
  const int ST = (l_max + 1) | 1;
  double* A = reinterpret_cast<double*>(lds_raw);
  double* R = A + (size_t)(l_max + 1) * ST + (l_max + 1);      // [row][slot]
  const int fam = sys == 0 ? 1 : sys == 1 ? 2 : 4;
  const int status = info[sys];                                // (the same value in every thread)
  if (sys != 0 && status == 1) {                               // a series of exact zeros keeps exact-zero derivatives
    for (int e = t; e < 4 * l_max; e += DBGE_NT) greek_t_dot[((long long)(e / l_max) * 6 + fam) * l_max + e % l_max] = 0.0;
    return;
  }
  bool fail = status != 0;
  if (!fail) {
    const double* fi = fac + (long long)sys * l_max * l_max;
    for (int e = t; e < n * n; e += DBGE_NT) {
      const int i = e / n, k = e % n;
      if (k <= i) A[i * ST + k] = fi[i * l_max + k];
    }
    for (int e = t; e < 4 * n; e += DBGE_NT) {
      const int i = e >> 2, q = e & 3;
      const double* p = rhs + ((long long)sys * 4 + q) * RP + i;
      double v = 0.0;
      for (long long ch = 0; ch < CH; ++ch) v += p[ch * 12 * RP];
      R[e] = v;
    }
    __syncthreads();
    const int q = t & 3, i0 = t >> 2;
    // y = L^-1 r:  column j of L is u_ij / d_j
    for (int j = 0; j < n - 1; ++j) {
      const double c = R[4 * j + q] / A[j * ST + j];           // (final since the barrier that ended step j - 1)
      for (int i = j + 1 + i0; i < n; i += DBGE_NT / 4) R[4 * i + q] -= A[i * ST + j] * c;
      __syncthreads();
    }
    // L^T x = D^-1 y backwards:  x_j = (y_j - sum_{i > j} u_ij x_i) / d_j; R[j] keeps the numerator, nobody writes it after step j
    for (int j = n - 1; j > 0; --j) {
      const double xj = R[4 * j + q] / A[j * ST + j];
      for (int i = i0; i < j; i += DBGE_NT / 4) R[4 * i + q] -= A[j * ST + i] * xj;
      __syncthreads();
    }
    int nonfinite = 0;
    for (int e = t; e < 4 * n; e += DBGE_NT) {
      const double x = R[e] / A[(e >> 2) * ST + (e >> 2)];
      nonfinite |= !(fabs(x) <= 1.79769313486231570815e308);
    }
    fail = __syncthreads_or(nonfinite) != 0;
    for (int e = t; e < 4 * n; e += DBGE_NT) R[e] = R[e] / A[(e >> 2) * ST + (e >> 2)];     // (each element by its own thread)
    __syncthreads();
    if (fail && t == 0) info[sys] = 2;
  }
  const double qnan = __builtin_nan("");
  if (sys != 0) {
    for (int e = t; e < 4 * l_max; e += DBGE_NT) {
      const int q = e / l_max, l = e % l_max;
      greek_t_dot[((long long)q * 6 + fam) * l_max + l] = l < off ? 0.0 : (fail ? qnan : R[4 * (l - off) + q]);
    }
    return;
  }
  // truncate_phase_lin.jl:183-207
  const double c0 = scal_t[0];
  for (int e = t; e < 4 * l_max; e += DBGE_NT) {
    const int q = e / l_max, l = e % l_max;
    const double* gd = greek_dot + (long long)q * 6 * n_mu;
    double* gtd = greek_t_dot + (long long)q * 6 * l_max;
    const double xd = fail ? qnan : R[4 * l + q], cd = fail ? qnan : R[q];
    const double cut = gd[1LL * n_mu + l] - xd;                // beta' - x'
    gtd[0LL * l_max + l] = (gd[0LL * n_mu + l] - cut - greek_t[0LL * l_max + l] * cd) / c0;
    gtd[1LL * l_max + l] = (xd - greek_t[1LL * l_max + l] * cd) / c0;
    gtd[3LL * l_max + l] = (gd[3LL * n_mu + l] - cut - greek_t[3LL * l_max + l] * cd) / c0;
    gtd[5LL * l_max + l] = (gd[5LL * n_mu + l] - cut - greek_t[5LL * l_max + l] * cd) / c0;
  }
  if (t < 4) {
    const double cd = fail ? qnan : R[t];
    scal_t_dot[2 * t] = cd;
    scal_t_dot[2 * t + 1] = -cd;
  }
}

}  // namespace vsm

using namespace vsm;

static bool dbge_shape_ok(int n_mu, int l_max) { return l_max >= 3 && l_max <= VSM_DBGE_MAX_L && n_mu > l_max; }

extern "C" size_t vsm_dbge_work_elems(int n_mu, int l_max) {
  if (!dbge_shape_ok(n_mu, l_max)) return 0;
  return (size_t)dbge_make_layout(n_mu, l_max).total;
}

extern "C" size_t vsm_dbge_lin_work_elems(int n_mu, int l_max) {
  if (!dbge_shape_ok(n_mu, l_max)) return 0;
  return (size_t)dbge_make_layout(n_mu, l_max).total_lin;
}

// the refusals the two entries share, in the forward entry's order
static int dbge_check(const char* fn, int n_mu, int l_max, int lowconf, double cos_delta, const double* bulk_f, const double* scal,
                      bool pointers) {
  if (l_max > VSM_DBGE_MAX_L) {
    set_error("%s: l_max = %d above VSM_DBGE_MAX_L = %d", fn, l_max, VSM_DBGE_MAX_L);
    return VSM_ERR_UNSUPPORTED;
  }
  VSM_REQUIRE(l_max >= 3, "%s: l_max = %d < 3", fn, l_max);
  VSM_REQUIRE(n_mu > l_max, "%s: n_mu = %d <= l_max = %d (nothing to truncate)", fn, n_mu, l_max);
  VSM_REQUIRE(lowconf >= 0 && lowconf <= n_mu, "%s: lowconf = %d is no count of the %d nodes", fn, lowconf, n_mu);
  VSM_REQUIRE(lowconf == 0 || lowconf >= l_max, "%s: %d nodes below cos_delta = %g for l_max = %d unknowns", fn, lowconf, cos_delta,
              l_max);
  VSM_REQUIRE((bulk_f == nullptr) == (scal == nullptr), "%s: bulk_f and scal come together or not at all", fn);
  VSM_REQUIRE(pointers, "%s: null pointer", fn);
  VSM_REQUIRE((n_mu + DBGE_KC - 1) / DBGE_KC <= 65535, "%s: n_mu = %d above %d", fn, n_mu, 65535 * DBGE_KC);
  return VSM_OK;
}

extern "C" int vsm_truncate_dbge(int n_mu, int l_max, int lowconf, double cos_delta, const double* greek, const double* bulk_f,
                                 const double* scal, const double* mu, const double* w_mu, double* greek_t, double* scal_t,
                                 int* info, double* work, void* stream) {
  int rc = dbge_check("vsm_truncate_dbge", n_mu, l_max, lowconf, cos_delta, bulk_f, scal,
                      greek && mu && w_mu && greek_t && scal_t && info && work);
  if (rc) return rc;
  const dbge_layout L = dbge_make_layout(n_mu, l_max);
  rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_dbge_solve<false>), dbge_lds_bytes(VSM_DBGE_MAX_L),
                      "hipFuncSetAttribute(k_dbge_solve)");
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  double* basis = work + L.o_basis;
  double* part = work + L.o_part;
  const double* none = nullptr;
  hipLaunchKernelGGL(k_dbge_basis<false>, dim3((unsigned)(L.KP / 64)), dim3(64), 0, st, n_mu, l_max, lowconf, cos_delta, L.RP, L.KP,
                     greek, bulk_f, scal, mu, w_mu, basis, info, none, none, none, (double*)nullptr);
  VSM_LAUNCH_CHECK("k_dbge_basis");
  const unsigned T = (unsigned)(L.RP / 16);
  hipLaunchKernelGGL(k_dbge_gram, dim3(T * (T + 1) / 2, (unsigned)L.CH, 3), dim3(64), 0, st, l_max, L.RP, L.KP, (const double*)basis,
                     (const int*)info, part);
  VSM_LAUNCH_CHECK("k_dbge_gram");
  hipLaunchKernelGGL(k_dbge_solve<false>, dim3(3), dim3(DBGE_NT), dbge_lds_bytes(l_max), st, n_mu, l_max, L.RP, L.CH,
                     (const double*)part, greek, greek_t, scal_t, info, (double*)nullptr, (double*)nullptr);
  VSM_LAUNCH_CHECK("k_dbge_solve");
  return VSM_OK;
}

extern "C" int vsm_truncate_dbge_lin(int n_mu, int l_max, int lowconf, double cos_delta, const double* greek, const double* bulk_f,
                                     const double* scal, const double* greek_dot, const double* bulk_f_dot, const double* scal_dot,
                                     const double* mu, const double* w_mu, double* greek_t, double* scal_t, double* greek_t_dot,
                                     double* scal_t_dot, int* info, double* work, void* stream) {
  const char* fn = "vsm_truncate_dbge_lin";
  if (l_max <= VSM_DBGE_MAX_L && lowconf != 0) {
    set_error("%s: lowconf = %d: only the all-nodes fit is linearized", fn, lowconf);
    return VSM_ERR_UNSUPPORTED;
  }
  int rc = dbge_check(fn, n_mu, l_max, lowconf, cos_delta, bulk_f, scal,
                      greek && greek_dot && mu && w_mu && greek_t && scal_t && greek_t_dot && scal_t_dot && info && work);
  if (rc) return rc;
  VSM_REQUIRE((bulk_f_dot == nullptr) == (bulk_f == nullptr) && (scal_dot == nullptr) == (bulk_f == nullptr),
              "%s: bulk_f_dot and scal_dot come with bulk_f and scal or not at all", fn);
  const dbge_layout L = dbge_make_layout(n_mu, l_max);
  rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_dbge_solve<true>), dbge_lds_bytes(VSM_DBGE_MAX_L),
                      "hipFuncSetAttribute(k_dbge_solve<lin>)");
  if (rc) return rc;
  rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_dbge_lin_solve), dbge_lin_lds_bytes(VSM_DBGE_MAX_L),
                      "hipFuncSetAttribute(k_dbge_lin_solve)");
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  double* basis = work + L.o_basis;
  double* part = work + L.o_part;
  double* fd = work + L.o_fd;
  double* fac = work + L.o_fac;
  double* xsol = work + L.o_x;
  double* rhs = work + L.o_rhs;
  hipLaunchKernelGGL(k_dbge_basis<true>, dim3((unsigned)(L.KP / 64), 5), dim3(64), 0, st, n_mu, l_max, 0, cos_delta, L.RP, L.KP, greek,
                     bulk_f, scal, mu, w_mu, basis, info, greek_dot, bulk_f_dot, scal_dot, fd);
  VSM_LAUNCH_CHECK("k_dbge_basis<lin>");
  const unsigned T = (unsigned)(L.RP / 16);
  hipLaunchKernelGGL(k_dbge_gram, dim3(T * (T + 1) / 2, (unsigned)L.CH, 3), dim3(64), 0, st, l_max, L.RP, L.KP, (const double*)basis,
                     (const int*)info, part);
  VSM_LAUNCH_CHECK("k_dbge_gram");
  hipLaunchKernelGGL(k_dbge_solve<true>, dim3(3), dim3(DBGE_NT), dbge_lds_bytes(l_max), st, n_mu, l_max, L.RP, L.CH,
                     (const double*)part, greek, greek_t, scal_t, info, fac, xsol);
  VSM_LAUNCH_CHECK("k_dbge_solve<lin>");
  hipLaunchKernelGGL(k_dbge_lin_rhs, dim3((unsigned)L.CH, 3), dim3(256), 0, st, l_max, L.RP, L.KP, (const double*)basis,
                     (const double*)fd, (const double*)xsol, (const int*)info, rhs);
  VSM_LAUNCH_CHECK("k_dbge_lin_rhs");
  hipLaunchKernelGGL(k_dbge_lin_solve, dim3(3), dim3(DBGE_NT), dbge_lin_lds_bytes(l_max), st, n_mu, l_max, L.RP, L.CH,
                     (const double*)fac, (const double*)rhs, greek_dot, (const double*)greek_t, (const double*)scal_t, greek_t_dot,
                     scal_t_dot, info);
  VSM_LAUNCH_CHECK("k_dbge_lin_solve");
  return VSM_OK;
}

