// Absorption: line-by-line cross-sections of a whole (p, T, vmr) profile (src/Absorption/compute_absorption_cross_section.jl).
//
// Two launches per call, whatever Nz is:
//   k_abs_params   one lane per (layer, line): the reference's host loop :108-153 -- pressure-shifted nu, gamma_l, gamma_d, y, S(T)
//                  and the index window [istart, istop] of the line on the grid -- into work [Nz, nLines, 8].
//   k_abs_accum    one workgroup per (tile of 256 grid points, layer), one point per lane: line_shape_batch! (:252-319) over the
//                  lines whose window can touch the tile, staged through LDS in chunks of VSM_ABS_CHUNK lines and summed in table
//                  order, so a call is bit-identical to its repetition.  No atomics, no library scratch, no host synchronisation.
//
// The one deviation from the reference: a line whose pressure-shifted window [nu - cutoff, nu + cutoff] misses the
// grid has an empty window here; the reference's upper interpolator extrapolates with N on both sides and gives it [1, N].
#include <hip/hip_runtime.h>

#include "vsm_common.h"
#include "vsm_internal.h"

namespace vsm {

// constants/constants.jl
constexpr double ABS_C2 = 1.4387769;
constexpr double ABS_MASSMOL = 1.66053873e-27;
constexpr double ABS_SQRTLN2_SQRTPI = 0.469718639319144059835;
constexpr double ABS_LN2 = 0.6931471805599;
constexpr double ABS_SQRTLN2 = 0.8325546111577;
constexpr double ABS_SQRT2LN2 = 1.1774100225;
constexpr double ABS_CC = 2.99792458e8;
constexpr double ABS_BOLTZ = 1.3806503e-23;
constexpr double ABS_P_REF = 1013.25;
constexpr double ABS_T_REF = 296.0;
constexpr double ABS_PI = 3.14159265358979323846;
constexpr double ABS_RSQRTPI = 0.56418958354775628695;   // 1 / sqrt(pi)

constexpr int ABS_TILE = 256;                 // grid points per workgroup, one per lane
constexpr int ABS_CHUNK = VSM_ABS_CHUNK;      // lines staged through LDS at a time
constexpr int ABS_FIELDS = VSM_ABS_WORK_FIELDS;
// work [Nz, nLines, 8]: the record of one (layer, line)
enum { AF_NU = 0, AF_GD = 1, AF_GL = 2, AF_Y = 3, AF_S = 4, AF_PRE = 5, AF_SX = 6, AF_WIN = 7 };

// fractional 1-based index of x on the grid by linear interpolation; needs grid[0] <= x <= grid[n - 1], n >= 2
__device__ inline double abs_frac_index(const double* __restrict__ grid, int n, double x) {
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (grid[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return (double)(lo + 1) + (x - grid[lo]) / (grid[lo + 1] - grid[lo]);
}

__global__ __launch_bounds__(256) void k_abs_params(int nSpec, int nLines, int nSpecies, int Nz, const double* __restrict__ grid,
                                                    const double* __restrict__ nu0, const double* __restrict__ S_ref,
                                                    const double* __restrict__ g_air, const double* __restrict__ g_self,
                                                    const double* __restrict__ n_air, const double* __restrict__ d_air,
                                                    const double* __restrict__ E_low, const int* __restrict__ species,
                                                    const double* __restrict__ molar_mass, const double* __restrict__ p,
                                                    const double* __restrict__ T, const double* __restrict__ vmr_self,
                                                    const double* __restrict__ qratio, double cutoff, double* __restrict__ work) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Nz * nLines) return;
  const int iz = (int)(i / nLines);
  const int j = (int)(i - (long long)iz * nLines);
  const double pr = p[iz], Tz = T[iz], vmr = vmr_self[iz];
  const double v0 = nu0[j];
  int sp = species[j];
  sp = sp < 0 ? 0 : (sp >= nSpecies ? nSpecies - 1 : sp);   // (a species index outside the table cannot read out of bounds)

  const double nu = v0 + pr / ABS_P_REF * d_air[j];
  const double gl = (g_air[j] * (1.0 - vmr) * pr / ABS_P_REF + g_self[j] * vmr * pr / ABS_P_REF) * pow(ABS_T_REF / Tz, n_air[j]);
  const double gd = (ABS_SQRT2LN2 / ABS_CC) * sqrt(ABS_BOLTZ / ABS_MASSMOL) * sqrt(Tz) * v0 / sqrt(molar_mass[sp]);
  const double y = sqrt(ABS_LN2) * gl / gd;
  double S = S_ref[j];
  const double E = E_low[j];
  if (E != -1.0)
    S = S * qratio[(long long)iz * nSpecies + sp] * exp(ABS_C2 * E * (1.0 / ABS_T_REF - 1.0 / Tz)) * (-expm1(-ABS_C2 * v0 / Tz)) /
        (-expm1(-ABS_C2 * v0 / ABS_T_REF));

  int istart = 1, istop = 1;
  if (nSpec > 1) {
    const double xl = nu - cutoff, xh = nu + cutoff;
    const double g0 = grid[0], g1 = grid[nSpec - 1];
    if (xh < g0 || xl > g1 || !(xl <= xh)) {
      istart = 1;
      istop = 0;   // the shifted window misses the grid: no point
    } else {
      istart = xl <= g0 ? 1 : (int)rint(abs_frac_index(grid, nSpec, xl));
      istop = xh >= g1 ? nSpec : (int)rint(abs_frac_index(grid, nSpec, xh));
    }
  }
  double* w = work + i * ABS_FIELDS;
  w[AF_NU] = nu;
  w[AF_GD] = gd;
  w[AF_GL] = gl;
  w[AF_Y] = y;
  w[AF_S] = S;
  w[AF_PRE] = S * ABS_SQRTLN2_SQRTPI / gd;   // the Voigt prefactor and argument scale, in the reference's operation order
  w[AF_SX] = ABS_SQRTLN2 / gd;
  w[AF_WIN] = __hiloint2double(istop, istart);
}

// ---- complex error functions: Re w(x + i y), y >= 0 (complex_error_functions.jl) ------------------------------------------------
// weideman32a: Weideman (1994) eq. (38.I), N = 32
__device__ inline double abs_weideman32_re(double x, double y) {
  constexpr double L32 = 4.7568284600108841;   // sqrt(32 / sqrt(2))
  constexpr double a[32] = {
      2.5722534081245696e+00,  2.2635372999002676e+00,  1.8256696296324824e+00,  1.3455441692345453e+00,  9.0192548936480144e-01,
      5.4601397206393498e-01,  2.9544451071508926e-01,  1.4060716226893769e-01,  5.7304403529837900e-02,  1.9006155784845689e-02,
      4.5195411053501429e-03,  3.9259136070122748e-04,  -2.4532980269928922e-04, -1.3075449254548613e-04, -2.1409619200870880e-05,
      6.8210319440412389e-06,  4.4015317319048931e-06,  4.2558331390536872e-07,  -4.1840763666294341e-07, -1.4813078891201116e-07,
      2.2930439569075392e-08,  2.3797557105844622e-08,  8.1248960947953431e-10,  -3.2080150458594088e-09, -5.2310170266050247e-10,
      4.1537465934749353e-10,  1.1658312885903929e-10,  -5.5441820344468828e-11, -2.1542618451370239e-11, 8.0314997274316680e-12,
      3.7424975634801558e-12,  -1.3031797863050087e-12};
  // iz = -y + i x;  lpiz = L + iz;  lmiz = L - iz;  rec = 1 / lmiz;  Z = lpiz rec
  const double pr = L32 - y, pi = x;
  const double mr = L32 + y, mi = -x;
  const double d = mr * mr + mi * mi;
  const double rr = mr / d, ri = -mi / d;
  const double Zr = pr * rr - pi * ri, Zi = pr * ri + pi * rr;
  double qr = a[31], qi = 0.0;
#pragma unroll
  for (int k = 30; k >= 0; --k) {
    const double tr = qr * Zr - qi * Zi;
    const double ti = qr * Zi + qi * Zr;
    qr = a[k] + tr;
    qi = ti;
  }
  // w = (1 / sqrt(pi) + 2 polynom rec) rec
  const double br = 2.0 * qr, bi = 2.0 * qi;
  const double Ar = ABS_RSQRTPI + (br * rr - bi * ri);
  const double Ai = br * ri + bi * rr;
  return Ar * rr - Ai * ri;
}

// humlicek1: i / sqrt(pi) z / (z z - 0.5)
__device__ inline double abs_humlicek1_re(double x, double y) {
  const double nr = -ABS_RSQRTPI * y, ni = ABS_RSQRTPI * x;
  const double dr = x * x - y * y - 0.5, di = 2.0 * (x * y);
  return (nr * dr + ni * di) / (dr * dr + di * di);
}

// humlicek2: t = y - i x, u = t t, w = t (1.410474 + u / sqrt(pi)) / (3/4 + u (3 + u))
__device__ inline double abs_humlicek2_re(double x, double y) {
  const double tr = y, ti = -x;
  const double ur = tr * tr - ti * ti, ui = 2.0 * (tr * ti);
  const double ar = 1.410474 + ur * ABS_RSQRTPI, ai = ui * ABS_RSQRTPI;
  const double nr = tr * ar - ti * ai, ni = tr * ai + ti * ar;
  const double sr = 3.0 + ur, si = ui;
  const double dr = 0.75 + (ur * sr - ui * si), di = ur * si + ui * sr;
  return (nr * dr + ni * di) / (dr * dr + di * di);
}

// CPF12 (Humlicek 1979): cpf12a where |x| < 18.1 y + 1.65 or y > 0.85, cpf12b elsewhere
__device__ inline double abs_cpf12_re(double x, double y) {
  constexpr double ct[6] = {.3142403762544, .9477883912402, 1.5976826351526, 2.2795070805011, 3.0206370251209, 3.88972489786978};
  constexpr double ca[6] = {-1.393236997981977,    -0.2311524061886763,  +0.1553514656420944,
                            -0.006218366236965554, 9.190829861057117e-5, +6.275259577e-7};
  constexpr double cb[6] = {1.011728045548831,   -0.7519714696746353,    0.01255772699323164,
                            0.01002200814515897, -2.420681348155727e-4, 5.008480613664576e-7};
  constexpr double cr = 1.5, crr = 2.25;
  const double ry = cr + y;
  if ((fabs(x) < 18.1 * y + 1.65) || (y > 0.85)) {
    const double ryy = ry * ry;
    double wk = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double xm = x - ct[k], xp = x + ct[k];
      wk += (ca[k] * xm + cb[k] * ry) / (xm * xm + ryy);
      wk -= (ca[k] * xp - cb[k] * ry) / (xp * xp + ryy);
    }
    return wk;
  }
  const double y2r = y + 2.0 * cr, rry = cr * ry, ryry = ry * ry;
  double wk = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double xm = x - ct[k], xp = x + ct[k];
    const double xm2 = xm * xm, xp2 = xp * xp;
    wk += (cb[k] * (xm2 - rry) - ca[k] * xm * y2r) / ((xm2 + crr) * (xm2 + ryry));
    wk += (cb[k] * (xp2 - rry) + ca[k] * xp * y2r) / ((xp2 + crr) * (xp2 + ryry));
  }
  return exp(-x * x) + y * wk;
}

template <int CEF>
__device__ inline double abs_cef_re(double x, double y) {
  if (CEF == VSM_ABS_CEF_HW32_VOIGT) return fabs(x) + y > 15.0 ? abs_humlicek1_re(x, y) : abs_weideman32_re(x, y);
  if (CEF == VSM_ABS_CEF_HW32_SD) return fabs(x) + y >= 8.0 ? abs_humlicek2_re(x, y) : abs_weideman32_re(x, y);
  return abs_cpf12_re(x, y);
}

// BROAD: 0 Doppler, 1 Lorentz, 2 Voigt
template <int BROAD, int CEF>
__global__ __launch_bounds__(ABS_TILE) void k_abs_accum(int nSpec, int nLines, const double* __restrict__ grid,
                                                        const double* __restrict__ nu0, const double* __restrict__ p,
                                                        const double* __restrict__ scale, double cutoff, double delta_max,
                                                        const double* __restrict__ work, int accumulate, double* __restrict__ out) {
  __shared__ double rec[ABS_CHUNK * ABS_FIELDS];
  const int t = (int)threadIdx.x;
  const int iz = (int)blockIdx.y;
  const int first = (int)blockIdx.x * ABS_TILE;                                  // 0-based first point of the tile (< nSpec)
  const int last = first + ABS_TILE - 1 < nSpec - 1 ? first + ABS_TILE - 1 : nSpec - 1;
  const int i0 = first + t;
  const bool live = i0 < nSpec;
  const int I = i0 + 1;                                                          // the reference's 1-based index
  const double nu_i = grid[live ? i0 : nSpec - 1];
  // 1-based point range of this wave (empty for a wave past the end of the grid: it skips every line)
  const int wfirst = first + (t & ~63) + 1;
  const int wlast = wfirst + 63 < nSpec ? wfirst + 63 : nSpec;

  // Lines whose window can touch the tile.  A point I lies in a window only if grid[I - 1] < nu + cutoff and nu - cutoff < grid[I + 1]
  // (rounding to nearest moves a window edge by less than one point), and |nu - nu0| <= delta_max p / p_ref.
  const double widen = cutoff + delta_max * (p[iz] / ABS_P_REF);
  double lo = grid[first > 0 ? first - 1 : 0] - widen;
  double hi = grid[last + 1 < nSpec ? last + 1 : nSpec - 1] + widen;
  lo -= 1e-9 * (fabs(lo) + 1.0);
  hi += 1e-9 * (fabs(hi) + 1.0);
  int j0, j1;
  {
    int a = 0, b = nLines;   // first line with nu0 >= lo
    while (a < b) {
      const int m = (int)(((unsigned)a + (unsigned)b) >> 1);
      if (nu0[m] < lo)
        a = m + 1;
      else
        b = m;
    }
    j0 = a;
    b = nLines;              // first line with nu0 > hi
    while (a < b) {
      const int m = (int)(((unsigned)a + (unsigned)b) >> 1);
      if (nu0[m] <= hi)
        a = m + 1;
      else
        b = m;
    }
    j1 = a;
  }
  j0 = __builtin_amdgcn_readfirstlane(j0);
  j1 = __builtin_amdgcn_readfirstlane(j1);

  const double* __restrict__ W = work + (long long)iz * nLines * ABS_FIELDS;
  double acc = 0.0;
  for (int c = j0; c < j1; c += ABS_CHUNK) {
    const int m = j1 - c < ABS_CHUNK ? j1 - c : ABS_CHUNK;
    __syncthreads();
    for (int k = t; k < m * ABS_FIELDS; k += ABS_TILE) rec[k] = W[(long long)c * ABS_FIELDS + k];
    __syncthreads();
    for (int l = 0; l < m; ++l) {
      const double* r = rec + l * ABS_FIELDS;
      const double win = r[AF_WIN];
      const int istart = __builtin_amdgcn_readfirstlane(__double2loint(win));
      const int istop = __builtin_amdgcn_readfirstlane(__double2hiint(win));
      if (istop < wfirst || istart > wlast) continue;   // wave-uniform: the window misses all 64 points of this wave
      if (istart <= I && I <= istop) {
        const double nu = r[AF_NU];
        if (BROAD == VSM_ABS_DOPPLER) {
          const double gd = r[AF_GD];
          const double u = (nu_i - nu) / gd;
          acc += r[AF_S] * ABS_SQRTLN2_SQRTPI * exp(-ABS_LN2 * (u * u)) / gd;
        } else if (BROAD == VSM_ABS_LORENTZ) {
          const double gl = r[AF_GL];
          const double dn = nu_i - nu;
          acc += r[AF_S] * gl / (ABS_PI * (gl * gl + dn * dn));
        } else {
          acc += r[AF_PRE] * abs_cef_re<CEF>(r[AF_SX] * (nu_i - nu), r[AF_Y]);
        }
      }
    }
  }
  if (live) {
    const long long o = (long long)iz * nSpec + i0;
    const double v = acc * scale[iz];
    out[o] = accumulate ? out[o] + v : v;
  }
}

// ---- linearized: d sigma / d(T, p, vmr_self), windows and error-function regions frozen ---------------------------
// Every line shape is term = pre F(x, y) with x = sx (nu_i - nu):
//   Voigt    pre = S c / gamma_d, sx = sqrt(ln 2) / gamma_d, y = sqrt(ln 2) gamma_l / gamma_d, F = Re w(x + i y)
//   Doppler  pre = S c / gamma_d, sx = 1 / gamma_d,                                            F = exp(-ln 2 x^2)
//   Lorentz  pre = S / pi,        sx = 1,                    y = gamma_l,                      F = y / (x^2 + y^2)
// and d term / d theta = pre (dlnpre_theta F + F_x x_theta + F_y y_theta); x_T = -x / (2 T) (Lorentz: 0) needs no field.
constexpr int ABS_LIN_CHUNK = VSM_ABS_LIN_CHUNK;
constexpr int ABS_LIN_FIELDS = VSM_ABS_LIN_WORK_FIELDS;
enum { LF_NU = 0, LF_WIN = 1, LF_PRE = 2, LF_SX = 3, LF_Y = 4, LF_DLNPRE_T = 5, LF_X_P = 6, LF_Y_T = 7, LF_Y_P = 8, LF_Y_V = 9 };

// One lane per (layer, line), behind k_abs_params on the same stream: nu, the window, pre, sx and y are taken from its record `fwd`,
// so the windows, x and y -- and with them the region of the error function -- are the forward's to the bit.
__global__ __launch_bounds__(256) void k_abs_params_lin(int nLines, int nSpecies, int Nz, const double* __restrict__ nu0,
                                                        const double* __restrict__ g_air, const double* __restrict__ g_self,
                                                        const double* __restrict__ n_air, const double* __restrict__ d_air,
                                                        const double* __restrict__ E_low, const int* __restrict__ species,
                                                        const double* __restrict__ p, const double* __restrict__ T,
                                                        const double* __restrict__ qratio_dlnT, int broadening,
                                                        const double* __restrict__ fwd, double* __restrict__ work) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Nz * nLines) return;
  const int iz = (int)(i / nLines);
  const int j = (int)(i - (long long)iz * nLines);
  const double pr = p[iz], Tz = T[iz];
  const double v0 = nu0[j], n = n_air[j], dl = d_air[j], E = E_low[j];
  int sp = species[j];
  sp = sp < 0 ? 0 : (sp >= nSpecies ? nSpecies - 1 : sp);
  const double* f = fwd + i * ABS_FIELDS;
  const double gd = f[AF_GD], gl = f[AF_GL];

  double dlnS = 0.0;   // d ln S / dT of :136; S(T) = S_ref for E'' = -1
  if (E != -1.0) {
    const double a = ABS_C2 * v0 / Tz;
    dlnS = qratio_dlnT[(long long)iz * nSpecies + sp] + ABS_C2 * E / (Tz * Tz) - (a / Tz) / expm1(a);
  }
  const double gl_v = (g_self[j] - g_air[j]) * pr / ABS_P_REF * pow(ABS_T_REF / Tz, n);   // d gamma_l / d vmr_self

  double* w = work + i * ABS_LIN_FIELDS;
  w[LF_NU] = f[AF_NU];
  w[LF_WIN] = f[AF_WIN];
  if (broadening == VSM_ABS_LORENTZ) {
    w[LF_PRE] = f[AF_S] / ABS_PI;
    w[LF_SX] = 1.0;
    w[LF_Y] = gl;
    w[LF_DLNPRE_T] = dlnS;
    w[LF_X_P] = -dl / ABS_P_REF;
    w[LF_Y_T] = -n * gl / Tz;
    w[LF_Y_P] = gl / pr;
    w[LF_Y_V] = gl_v;
  } else {
    const bool voigt = broadening == VSM_ABS_VOIGT;
    const double sx = voigt ? f[AF_SX] : 1.0 / gd;
    const double y = voigt ? f[AF_Y] : 0.0;
    w[LF_PRE] = f[AF_PRE];
    w[LF_SX] = sx;
    w[LF_Y] = y;
    w[LF_DLNPRE_T] = dlnS - 0.5 / Tz;
    w[LF_X_P] = -sx * dl / ABS_P_REF;
    w[LF_Y_T] = -y * (n + 0.5) / Tz;
    w[LF_Y_P] = y / pr;
    w[LF_Y_V] = voigt ? sqrt(ABS_LN2) * gl_v / gd : 0.0;
  }
}

// F, dF/dx, dF/dy.  Under Voigt F = Re w, F_x = Re w', F_y = -Im w' with w' the closed-form derivative of the approximant itself:
// the identity w' = -2 z w + 2 i / sqrt(pi) cancels to order 1 / x^2 in the far wing and differentiates the true function.
struct AbsLin {
  double f, fx, fy;
};

// weideman32a: w = (1/sqrt(pi) + 2 P(Z) rec) rec, rec = 1 / (L - i z), Z = (L + i z) rec; dZ/dz = i rec (1 + Z), d rec/dz = i rec^2, so
// w' = i rec^2 (1/sqrt(pi) + 2 rec (2 P + P' (1 + Z))); P' from a second Horner chain.
__device__ inline AbsLin abs_weideman32_lin(double x, double y) {
  constexpr double L32 = 4.7568284600108841;
  constexpr double a[32] = {
      2.5722534081245696e+00,  2.2635372999002676e+00,  1.8256696296324824e+00,  1.3455441692345453e+00,  9.0192548936480144e-01,
      5.4601397206393498e-01,  2.9544451071508926e-01,  1.4060716226893769e-01,  5.7304403529837900e-02,  1.9006155784845689e-02,
      4.5195411053501429e-03,  3.9259136070122748e-04,  -2.4532980269928922e-04, -1.3075449254548613e-04, -2.1409619200870880e-05,
      6.8210319440412389e-06,  4.4015317319048931e-06,  4.2558331390536872e-07,  -4.1840763666294341e-07, -1.4813078891201116e-07,
      2.2930439569075392e-08,  2.3797557105844622e-08,  8.1248960947953431e-10,  -3.2080150458594088e-09, -5.2310170266050247e-10,
      4.1537465934749353e-10,  1.1658312885903929e-10,  -5.5441820344468828e-11, -2.1542618451370239e-11, 8.0314997274316680e-12,
      3.7424975634801558e-12,  -1.3031797863050087e-12};
  const double pr = L32 - y, pi = x;
  const double mr = L32 + y, mi = -x;
  const double d = mr * mr + mi * mi;
  const double rr = mr / d, ri = -mi / d;
  const double Zr = pr * rr - pi * ri, Zi = pr * ri + pi * rr;
  double qr = a[31], qi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
  for (int k = 30; k >= 0; --k) {
    const double ur = dr * Zr - di * Zi + qr;   // P' <- P' Z + P
    const double ui = dr * Zi + di * Zr + qi;
    const double tr = qr * Zr - qi * Zi;        // P  <- P Z + a_k
    const double ti = qr * Zi + qi * Zr;
    dr = ur;
    di = ui;
    qr = a[k] + tr;
    qi = ti;
  }
  const double br = 2.0 * qr, bi = 2.0 * qi;
  const double Ar = ABS_RSQRTPI + (br * rr - bi * ri);
  const double Ai = br * ri + bi * rr;
  // g = 2 P + P' (1 + Z);  h = 1/sqrt(pi) + 2 rec g;  w' = i rec^2 h
  const double gr = br + (dr * (1.0 + Zr) - di * Zi), gi = bi + (dr * Zi + di * (1.0 + Zr));
  const double hr = ABS_RSQRTPI + 2.0 * (rr * gr - ri * gi), hi = 2.0 * (rr * gi + ri * gr);
  const double r2r = rr * rr - ri * ri, r2i = 2.0 * (rr * ri);
  const double er = r2r * hr - r2i * hi, ei = r2r * hi + r2i * hr;   // rec^2 h;  w' = i (er + i ei) = -ei + i er
  return {Ar * rr - Ai * ri, -ei, -er};
}

// humlicek1: w = i / sqrt(pi) z / (z z - 1/2);  w' = -i / sqrt(pi) (z z + 1/2) / (z z - 1/2)^2
__device__ inline AbsLin abs_humlicek1_lin(double x, double y) {
  const double qr = x * x - y * y, qi = 2.0 * (x * y);
  const double dr = qr - 0.5;
  const double s = 1.0 / (dr * dr + qi * qi);
  const double ir = dr * s, ii = -qi * s;                              // 1 / (z z - 1/2)
  const double zi = x * ii + y * ir;                                   // Im z / (z z - 1/2);  Re w = -c0 of it
  const double nr = qr + 0.5;
  const double ar = nr * ir - qi * ii, ai = nr * ii + qi * ir;
  const double mr = ar * ir - ai * ii, mi = ar * ii + ai * ir;         // (z z + 1/2) / (z z - 1/2)^2;  w' = -i c0 (mr + i mi)
  return {-ABS_RSQRTPI * zi, ABS_RSQRTPI * mi, ABS_RSQRTPI * mr};
}

// humlicek2: t = y - i x, u = t t, w = N / D, N = t (1.410474 + u / sqrt(pi)), D = 3/4 + u (3 + u);  dw/dt = (N' - w D') / D with
// N' = 1.410474 + 3 u / sqrt(pi), D' = t (6 + 4 u);  dt/dx = -i, dt/dy = 1: F_x = Im dw/dt, F_y = Re dw/dt.  One division.
__device__ inline AbsLin abs_humlicek2_lin(double x, double y) {
  const double tr = y, ti = -x;
  const double ur = tr * tr - ti * ti, ui = 2.0 * (tr * ti);
  const double ar = 1.410474 + ur * ABS_RSQRTPI, ai = ui * ABS_RSQRTPI;
  const double nr = tr * ar - ti * ai, ni = tr * ai + ti * ar;
  const double sr = 3.0 + ur, si = ui;
  const double dr = 0.75 + (ur * sr - ui * si), di = ur * si + ui * sr;
  const double s = 1.0 / (dr * dr + di * di);
  const double ir = dr * s, ii = -di * s;                              // 1 / D
  const double wr = nr * ir - ni * ii, wi = nr * ii + ni * ir;
  const double er = 6.0 + 4.0 * ur, ei = 4.0 * ui;
  const double pr = tr * er - ti * ei, pi = tr * ei + ti * er;         // D'
  const double gr = 1.410474 + 3.0 * ABS_RSQRTPI * ur - (wr * pr - wi * pi);
  const double gi = 3.0 * ABS_RSQRTPI * ui - (wr * pi + wi * pr);
  return {wr, gr * ii + gi * ir, gr * ir - gi * ii};
}

template <int BROAD, int CEF>
__device__ inline AbsLin abs_shape_lin(double x, double y) {
  if (BROAD == VSM_ABS_DOPPLER) {
    const double F = exp(-ABS_LN2 * (x * x));
    return {F, -2.0 * ABS_LN2 * x * F, 0.0};
  }
  if (BROAD == VSM_ABS_LORENTZ) {
    const double s = 1.0 / (y * y + x * x);
    return {y * s, -2.0 * (x * y) * (s * s), (x * x - y * y) * (s * s)};
  }
  if (CEF == VSM_ABS_CEF_HW32_VOIGT) return fabs(x) + y > 15.0 ? abs_humlicek1_lin(x, y) : abs_weideman32_lin(x, y);
  return fabs(x) + y >= 8.0 ? abs_humlicek2_lin(x, y) : abs_weideman32_lin(x, y);
}

// The forward's decomposition: one workgroup per (tile of 256 points, layer), one point per lane, the same binary search on nu0, the
// records through LDS in chunks, the scalar window skip per wave, table-order sums per lane.
template <int BROAD, int CEF>
__global__ __launch_bounds__(ABS_TILE) void k_abs_accum_lin(int nSpec, int nLines, const double* __restrict__ grid,
                                                            const double* __restrict__ nu0, const double* __restrict__ p,
                                                            const double* __restrict__ T, const double* __restrict__ scale,
                                                            double cutoff, double delta_max, const double* __restrict__ work,
                                                            int accumulate, double* __restrict__ out_dT, double* __restrict__ out_dp,
                                                            double* __restrict__ out_dv) {
  __shared__ double rec[ABS_LIN_CHUNK * ABS_LIN_FIELDS];
  const int t = (int)threadIdx.x;
  const int iz = (int)blockIdx.y;
  const int first = (int)blockIdx.x * ABS_TILE;
  const int last = first + ABS_TILE - 1 < nSpec - 1 ? first + ABS_TILE - 1 : nSpec - 1;
  const int i0 = first + t;
  const bool live = i0 < nSpec;
  const int I = i0 + 1;
  const double nu_i = grid[live ? i0 : nSpec - 1];
  const int wfirst = first + (t & ~63) + 1;
  const int wlast = wfirst + 63 < nSpec ? wfirst + 63 : nSpec;
  const double hT = BROAD == VSM_ABS_LORENTZ ? 0.0 : -0.5 / T[iz];   // x_T = x hT

  const double widen = cutoff + delta_max * (p[iz] / ABS_P_REF);
  double lo = grid[first > 0 ? first - 1 : 0] - widen;
  double hi = grid[last + 1 < nSpec ? last + 1 : nSpec - 1] + widen;
  lo -= 1e-9 * (fabs(lo) + 1.0);
  hi += 1e-9 * (fabs(hi) + 1.0);
  int j0, j1;
  {
    int a = 0, b = nLines;   // first line with nu0 >= lo
    while (a < b) {
      const int m = (int)(((unsigned)a + (unsigned)b) >> 1);
      if (nu0[m] < lo)
        a = m + 1;
      else
        b = m;
    }
    j0 = a;
    b = nLines;              // first line with nu0 > hi
    while (a < b) {
      const int m = (int)(((unsigned)a + (unsigned)b) >> 1);
      if (nu0[m] <= hi)
        a = m + 1;
      else
        b = m;
    }
    j1 = a;
  }
  j0 = __builtin_amdgcn_readfirstlane(j0);
  j1 = __builtin_amdgcn_readfirstlane(j1);

  const double* __restrict__ W = work + (long long)iz * nLines * ABS_LIN_FIELDS;
  double accT = 0.0, accP = 0.0, accV = 0.0;
  for (int c = j0; c < j1; c += ABS_LIN_CHUNK) {
    const int m = j1 - c < ABS_LIN_CHUNK ? j1 - c : ABS_LIN_CHUNK;
    __syncthreads();
    for (int k = t; k < m * ABS_LIN_FIELDS; k += ABS_TILE) rec[k] = W[(long long)c * ABS_LIN_FIELDS + k];
    __syncthreads();
    for (int l = 0; l < m; ++l) {
      const double* r = rec + l * ABS_LIN_FIELDS;
      const double win = r[LF_WIN];
      const int istart = __builtin_amdgcn_readfirstlane(__double2loint(win));
      const int istop = __builtin_amdgcn_readfirstlane(__double2hiint(win));
      if (istop < wfirst || istart > wlast) continue;   // wave-uniform: the window misses all 64 points of this wave
      if (istart <= I && I <= istop) {
        const double x = r[LF_SX] * (nu_i - r[LF_NU]);
        const AbsLin s = abs_shape_lin<BROAD, CEF>(x, r[LF_Y]);
        const double pre = r[LF_PRE];
        if (BROAD == VSM_ABS_DOPPLER) {   // F_y = 0
          accT += pre * (r[LF_DLNPRE_T] * s.f + s.fx * (x * hT));
          accP += pre * (s.fx * r[LF_X_P]);
        } else {
          accT += pre * (r[LF_DLNPRE_T] * s.f + s.fx * (x * hT) + s.fy * r[LF_Y_T]);
          accP += pre * (s.fx * r[LF_X_P] + s.fy * r[LF_Y_P]);
          accV += pre * (s.fy * r[LF_Y_V]);
        }
      }
    }
  }
  if (live) {
    const long long o = (long long)iz * nSpec + i0;
    const double sc = scale[iz];
    const double vT = accT * sc, vP = accP * sc, vV = accV * sc;
    out_dT[o] = accumulate ? out_dT[o] + vT : vT;
    out_dp[o] = accumulate ? out_dp[o] + vP : vP;
    out_dv[o] = accumulate ? out_dv[o] + vV : vV;
  }
}

// out [K, Nz, nSpec] = dT [Nz, nSpec] T_dot [K, Nz] + dp [Nz, nSpec] p_dot [K, Nz]
__global__ __launch_bounds__(256) void k_abs_profile_slots(int nSpec, int Nz, const double* __restrict__ dT, const double* __restrict__ dp,
                                                           const double* __restrict__ T_dot, const double* __restrict__ p_dot,
                                                           double* __restrict__ out) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= nSpec) return;
  const int iz = (int)blockIdx.y, k = (int)blockIdx.z;
  const long long o = (long long)iz * nSpec + i;
  out[(long long)k * Nz * nSpec + o] = dT[o] * T_dot[(long long)k * Nz + iz] + dp[o] * p_dot[(long long)k * Nz + iz];
}

}  // namespace vsm

using namespace vsm;

extern "C" int vsm_absorption_chunk(void) { return ABS_CHUNK; }

extern "C" size_t vsm_absorption_work_elems(int Nz, int nLines) {
  return Nz >= 1 && nLines >= 1 ? (size_t)Nz * (size_t)nLines * ABS_FIELDS : 0;
}

extern "C" int vsm_absorption_xsec(int nSpec, int nLines, int nSpecies, int Nz, const double* grid, const double* nu0,
                                   const double* S_ref, const double* gamma_air, const double* gamma_self, const double* n_air,
                                   const double* delta_air, const double* E_low, const int* species, const double* molar_mass,
                                   const double* p, const double* T, const double* vmr_self, const double* scale,
                                   const double* qratio, double wing_cutoff, double delta_max, int broadening, int cef,
                                   int accumulate, double* out, double* work, void* stream) {
  const char* fn = "vsm_absorption_xsec";
  VSM_REQUIRE(nSpec >= 1 && nLines >= 1 && nSpecies >= 1 && Nz >= 1, "%s: nSpec = %d, nLines = %d, nSpecies = %d, Nz = %d must be >= 1",
              fn, nSpec, nLines, nSpecies, Nz);
  VSM_REQUIRE(Nz <= 65535, "%s: Nz = %d above 65535 layers", fn, Nz);
  VSM_REQUIRE((long long)Nz * nLines <= 256LL * 0x7fffffffLL, "%s: Nz nLines = %lld above the launch limit", fn, (long long)Nz * nLines);
  VSM_REQUIRE(wing_cutoff >= 0.0 && delta_max >= 0.0, "%s: wing_cutoff = %g, delta_max = %g must be >= 0 (and not NaN)", fn,
              wing_cutoff, delta_max);
  VSM_REQUIRE(broadening >= VSM_ABS_DOPPLER && broadening <= VSM_ABS_VOIGT, "%s: broadening = %d (0 Doppler, 1 Lorentz, 2 Voigt)", fn,
              broadening);
  VSM_REQUIRE(cef >= VSM_ABS_CEF_HW32_VOIGT && cef <= VSM_ABS_CEF_CPF12, "%s: cef = %d (0 HW32 Voigt, 1 HW32 SD, 2 CPF12)", fn, cef);
  VSM_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate = %d (0 writes, 1 adds)", fn, accumulate);
  VSM_REQUIRE(grid && nu0 && S_ref && gamma_air && gamma_self && n_air && delta_air && E_low && species && molar_mass && p && T &&
                  vmr_self && scale && qratio && out && work,
              "%s: null pointer", fn);
  hipStream_t st = as_stream(stream);
  const long long lanes = (long long)Nz * nLines;
  hipLaunchKernelGGL(k_abs_params, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, nSpec, nLines, nSpecies, Nz, grid, nu0,
                     S_ref, gamma_air, gamma_self, n_air, delta_air, E_low, species, molar_mass, p, T, vmr_self, qratio, wing_cutoff,
                     work);
  VSM_LAUNCH_CHECK("k_abs_params");
  const dim3 g((unsigned)((nSpec + ABS_TILE - 1) / ABS_TILE), (unsigned)Nz), b(ABS_TILE);
#define ABS_LAUNCH(B, C)                                                                                                     \
  hipLaunchKernelGGL((k_abs_accum<B, C>), g, b, 0, st, nSpec, nLines, grid, nu0, p, scale, wing_cutoff, delta_max, \
                     (const double*)work, accumulate, out)
  if (broadening == VSM_ABS_DOPPLER)
    ABS_LAUNCH(VSM_ABS_DOPPLER, 0);
  else if (broadening == VSM_ABS_LORENTZ)
    ABS_LAUNCH(VSM_ABS_LORENTZ, 0);
  else if (cef == VSM_ABS_CEF_HW32_VOIGT)
    ABS_LAUNCH(VSM_ABS_VOIGT, VSM_ABS_CEF_HW32_VOIGT);
  else if (cef == VSM_ABS_CEF_HW32_SD)
    ABS_LAUNCH(VSM_ABS_VOIGT, VSM_ABS_CEF_HW32_SD);
  else
    ABS_LAUNCH(VSM_ABS_VOIGT, VSM_ABS_CEF_CPF12);
#undef ABS_LAUNCH
  VSM_LAUNCH_CHECK("k_abs_accum");
  return VSM_OK;
}

extern "C" int vsm_absorption_lin_chunk(void) { return ABS_LIN_CHUNK; }

extern "C" size_t vsm_absorption_lin_work_elems(int Nz, int nLines) {
  return Nz >= 1 && nLines >= 1 ? (size_t)Nz * (size_t)nLines * (ABS_FIELDS + ABS_LIN_FIELDS) : 0;
}

extern "C" int vsm_absorption_xsec_lin(int nSpec, int nLines, int nSpecies, int Nz, const double* grid, const double* nu0,
                                       const double* S_ref, const double* gamma_air, const double* gamma_self, const double* n_air,
                                       const double* delta_air, const double* E_low, const int* species, const double* molar_mass,
                                       const double* p, const double* T, const double* vmr_self, const double* scale,
                                       const double* qratio, const double* qratio_dlnT, double wing_cutoff, double delta_max,
                                       int broadening, int cef, int accumulate, double* out, double* out_dT, double* out_dp,
                                       double* out_dvmr, double* work, void* stream) {
  const char* fn = "vsm_absorption_xsec_lin";
  // the forward's refusals, under this entry's name, and this entry's own: all before the first launch
  VSM_REQUIRE(nSpec >= 1 && nLines >= 1 && nSpecies >= 1 && Nz >= 1, "%s: nSpec = %d, nLines = %d, nSpecies = %d, Nz = %d must be >= 1",
              fn, nSpec, nLines, nSpecies, Nz);
  VSM_REQUIRE(Nz <= 65535, "%s: Nz = %d above 65535 layers", fn, Nz);
  VSM_REQUIRE((long long)Nz * nLines <= 256LL * 0x7fffffffLL, "%s: Nz nLines = %lld above the launch limit", fn, (long long)Nz * nLines);
  VSM_REQUIRE(wing_cutoff >= 0.0 && delta_max >= 0.0, "%s: wing_cutoff = %g, delta_max = %g must be >= 0 (and not NaN)", fn,
              wing_cutoff, delta_max);
  VSM_REQUIRE(broadening >= VSM_ABS_DOPPLER && broadening <= VSM_ABS_VOIGT, "%s: broadening = %d (0 Doppler, 1 Lorentz, 2 Voigt)", fn,
              broadening);
  VSM_REQUIRE(cef >= VSM_ABS_CEF_HW32_VOIGT && cef <= VSM_ABS_CEF_CPF12, "%s: cef = %d (0 HW32 Voigt, 1 HW32 SD, 2 CPF12)", fn, cef);
  VSM_REQUIRE(!(broadening == VSM_ABS_VOIGT && cef == VSM_ABS_CEF_CPF12), "%s: CPF12 is not linearized (cef 0 HW32 Voigt or 1 HW32 SD)", fn);
  VSM_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate = %d (0 writes, 1 adds)", fn, accumulate);
  VSM_REQUIRE(grid && nu0 && S_ref && gamma_air && gamma_self && n_air && delta_air && E_low && species && molar_mass && p && T &&
                  vmr_self && scale && qratio && qratio_dlnT && out && out_dT && out_dp && out_dvmr && work,
              "%s: null pointer", fn);
  // sigma: the unchanged forward call on the head of `work`
  const int rc = vsm_absorption_xsec(nSpec, nLines, nSpecies, Nz, grid, nu0, S_ref, gamma_air, gamma_self, n_air, delta_air, E_low,
                                     species, molar_mass, p, T, vmr_self, scale, qratio, wing_cutoff, delta_max, broadening, cef,
                                     accumulate, out, work, stream);
  if (rc != VSM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const long long lanes = (long long)Nz * nLines;
  double* lin = work + lanes * ABS_FIELDS;
  hipLaunchKernelGGL(k_abs_params_lin, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, nLines, nSpecies, Nz, nu0, gamma_air,
                     gamma_self, n_air, delta_air, E_low, species, p, T, qratio_dlnT, broadening, (const double*)work, lin);
  VSM_LAUNCH_CHECK("k_abs_params_lin");
  const dim3 g((unsigned)((nSpec + ABS_TILE - 1) / ABS_TILE), (unsigned)Nz), b(ABS_TILE);
#define ABS_LAUNCH_LIN(B, C)                                                                                                   \
  hipLaunchKernelGGL((k_abs_accum_lin<B, C>), g, b, 0, st, nSpec, nLines, grid, nu0, p, T, scale, wing_cutoff, delta_max, \
                     (const double*)lin, accumulate, out_dT, out_dp, out_dvmr)
  if (broadening == VSM_ABS_DOPPLER)
    ABS_LAUNCH_LIN(VSM_ABS_DOPPLER, 0);
  else if (broadening == VSM_ABS_LORENTZ)
    ABS_LAUNCH_LIN(VSM_ABS_LORENTZ, 0);
  else if (cef == VSM_ABS_CEF_HW32_VOIGT)
    ABS_LAUNCH_LIN(VSM_ABS_VOIGT, VSM_ABS_CEF_HW32_VOIGT);
  else
    ABS_LAUNCH_LIN(VSM_ABS_VOIGT, VSM_ABS_CEF_HW32_SD);
#undef ABS_LAUNCH_LIN
  VSM_LAUNCH_CHECK("k_abs_accum_lin");
  return VSM_OK;
}

extern "C" int vsm_absorption_profile_slots(int nSpec, int Nz, int K, const double* dT, const double* dp, const double* T_dot,
                                            const double* p_dot, double* out, void* stream) {
  const char* fn = "vsm_absorption_profile_slots";
  VSM_REQUIRE(nSpec >= 1 && Nz >= 1 && K >= 1, "%s: nSpec = %d, Nz = %d, K = %d must be >= 1", fn, nSpec, Nz, K);
  VSM_REQUIRE(Nz <= 65535 && K <= 65535, "%s: Nz = %d, K = %d above 65535", fn, Nz, K);
  VSM_REQUIRE(dT && dp && T_dot && p_dot && out, "%s: null pointer", fn);
  hipLaunchKernelGGL(k_abs_profile_slots, dim3((unsigned)((nSpec + 255) / 256), (unsigned)Nz, (unsigned)K), dim3(256), 0,
                     as_stream(stream), nSpec, Nz, dT, dp, T_dot, p_dot, out);
  VSM_LAUNCH_CHECK("k_abs_profile_slots");
  return VSM_OK;
}
