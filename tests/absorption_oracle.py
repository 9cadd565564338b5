"""numpy restatement of the reference's line-by-line absorption (src/Absorption): the parameter pass of
compute_absorption_cross_section.jl:108-153 with the constants of constants/constants.jl, the index windows, the three line shapes of
line_shape_batch!, the three complex error functions of complex_error_functions.jl that vsm.Absorption builds, and the natural cubic
spline of qoft! (DataInterpolations.CubicSpline).  Test infrastructure: nothing here is imported by the package.

Every function takes `dtype` (np.float64 or np.longdouble); the same code then runs in the 80-bit format, which is how the GPU tests
measure the rounding floor of a case.  Literal constants are the reference's Float64 literals in both formats.

One deliberate deviation from the reference: a line whose pressure-shifted window [nu - cutoff, nu + cutoff] misses the grid
contributes nothing.  The reference's upper index interpolator extrapolates with N on both sides, so there such a line gets [1, N].

The lines are summed in the order of the table sorted by nu0 (stable), which is the order of the device."""
import math

import numpy as np

C2 = 1.4387769
MASSMOL = 1.66053873e-27
SQRTLN2_SQRTPI = 0.469718639319144059835
LN2 = 0.6931471805599
SQRTLN2 = 0.8325546111577
SQRT2LN2 = 1.1774100225
CC = 2.99792458e8
BOLTZ = 1.3806503e-23
P_REF = 1013.25
T_REF = 296.0
NM_PER_M = 1.0e7
RSQRTPI = 1 / math.sqrt(math.pi)          # FT(1/sqrt(pi))

BROADENINGS = ("Doppler", "Lorentz", "Voigt")
CEFS = ("HumlicekWeidemann32VoigtErrorFunction", "HumlicekWeidemann32SDErrorFunction", "CPF12ErrorFunction")

HALF_INTEGER_GUARD = 1e-6


def _ctype(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


# ---- complex error functions ---------------------------------------------------------------------------------------------------------
_W32 = [2.5722534081245696e+00, 2.2635372999002676e+00, 1.8256696296324824e+00, 1.3455441692345453e+00, 9.0192548936480144e-01,
        5.4601397206393498e-01, 2.9544451071508926e-01, 1.4060716226893769e-01, 5.7304403529837900e-02, 1.9006155784845689e-02,
        4.5195411053501429e-03, 3.9259136070122748e-04, -2.4532980269928922e-04, -1.3075449254548613e-04, -2.1409619200870880e-05,
        6.8210319440412389e-06, 4.4015317319048931e-06, 4.2558331390536872e-07, -4.1840763666294341e-07, -1.4813078891201116e-07,
        2.2930439569075392e-08, 2.3797557105844622e-08, 8.1248960947953431e-10, -3.2080150458594088e-09, -5.2310170266050247e-10,
        4.1537465934749353e-10, 1.1658312885903929e-10, -5.5441820344468828e-11, -2.1542618451370239e-11, 8.0314997274316680e-12,
        3.7424975634801558e-12, -1.3031797863050087e-12]


def weideman32a(z, dtype=np.float64):
    FT, CT = np.dtype(dtype).type, _ctype(dtype)
    z = np.asarray(z, dtype=CT)
    L32 = FT(math.sqrt(32 / math.sqrt(2)))
    iz = CT(1j) * z.real - z.imag
    lpiz = L32 + iz
    lmiz = L32 - iz
    rec = FT(1) / lmiz
    Z = lpiz * rec
    poly = np.full(z.shape, FT(_W32[31]), dtype=CT)
    for k in range(30, -1, -1):
        poly = FT(_W32[k]) + poly * Z
    return (FT(RSQRTPI) + FT(2) * poly * rec) * rec


def humlicek1(z, dtype=np.float64):
    FT, CT = np.dtype(dtype).type, _ctype(dtype)
    z = np.asarray(z, dtype=CT)
    return CT(1j) * FT(RSQRTPI) * z / (z * z - FT(0.5))


def humlicek2(z, dtype=np.float64):
    FT, CT = np.dtype(dtype).type, _ctype(dtype)
    z = np.asarray(z, dtype=CT)
    t = z.imag - CT(1j) * z.real
    u = t * t
    return (t * (FT(1.410474) + u * FT(RSQRTPI))) / (FT(3) / FT(4) + (u * (FT(3) + u)))


_CT12 = [.3142403762544, .9477883912402, 1.5976826351526, 2.2795070805011, 3.0206370251209, 3.88972489786978]
_CA12 = [-1.393236997981977, -0.2311524061886763, +0.1553514656420944, -0.006218366236965554, 9.190829861057117e-5, +6.275259577e-7]
_CB12 = [1.011728045548831, -0.7519714696746353, 0.01255772699323164, 0.01002200814515897, -2.420681348155727e-4, 5.008480613664576e-7]


def cpf12a(z, dtype=np.float64):
    FT, CT = np.dtype(dtype).type, _ctype(dtype)
    z = np.asarray(z, dtype=CT)
    x, y = z.real, z.imag
    ry = FT(1.5) + y
    ryy = ry * ry
    wk = np.zeros(x.shape, dtype=FT)
    wl = np.zeros(x.shape, dtype=FT)
    for ct, ca, cb in zip(_CT12, _CA12, _CB12):
        ct, ca, cb = FT(ct), FT(ca), FT(cb)
        wk = wk + (ca * (x - ct) + cb * ry) / ((x - ct) ** 2 + ryy)
        wk = wk - (ca * (x + ct) - cb * ry) / ((x + ct) ** 2 + ryy)
        wl = wl + (cb * (x - ct) - ca * ry) / ((x - ct) ** 2 + ryy)
        wl = wl + (cb * (x + ct) + ca * ry) / ((x + ct) ** 2 + ryy)
    return wk + CT(1j) * wl


def cpf12b(z, dtype=np.float64):
    FT, CT = np.dtype(dtype).type, _ctype(dtype)
    z = np.asarray(z, dtype=CT)
    x, y = z.real, z.imag
    cr, crr = FT(1.5), FT(2.25)
    ry = cr + y
    y2r = y + FT(2) * cr
    rry = cr * ry
    ryry = ry ** 2
    wk = np.zeros(x.shape, dtype=FT)
    wl = np.zeros(x.shape, dtype=FT)
    for ct, ca, cb in zip(_CT12, _CA12, _CB12):
        ct, ca, cb = FT(ct), FT(ca), FT(cb)
        wk = wk + (cb * ((x - ct) ** 2 - rry) - ca * (x - ct) * y2r) / (((x - ct) ** 2 + crr) * ((x - ct) ** 2 + ryry))
        wk = wk + (cb * ((x + ct) ** 2 - rry) + ca * (x + ct) * y2r) / (((x + ct) ** 2 + crr) * ((x + ct) ** 2 + ryry))
        wl = wl + (cb * (x - ct) - ca * ry) / ((x - ct) ** 2 + ryry)
        wl = wl + (cb * (x + ct) + ca * ry) / ((x + ct) ** 2 + ryry)
    return np.exp(-x * x) + y * wk + CT(1j) * wl


def w(cef, z, dtype=np.float64):
    """w(CEF, z) of complex_error_functions.jl:224-263, region by region, for an array z = x + i y."""
    FT, CT = np.dtype(dtype).type, _ctype(dtype)
    z = np.atleast_1d(np.asarray(z, dtype=CT))
    x, y = z.real, z.imag
    if cef == "HumlicekWeidemann32VoigtErrorFunction":
        return np.where(np.abs(x) + y > FT(15), humlicek1(z, dtype), weideman32a(z, dtype))
    if cef == "HumlicekWeidemann32SDErrorFunction":
        return np.where(np.abs(x) + y >= FT(8), humlicek2(z, dtype), weideman32a(z, dtype))
    if cef == "CPF12ErrorFunction":
        return np.where((np.abs(x) < FT(18.1) * y + FT(1.65)) | (y > FT(0.85)), cpf12a(z, dtype), cpf12b(z, dtype))
    raise ValueError(cef)


# ---- natural cubic spline (qoft!) ----------------------------------------------------------------------------------------------------
def natural_spline(t, u, x, dtype=np.float64):
    """The natural cubic spline through (t, u) at x: second derivatives zero at both ends (DataInterpolations.CubicSpline)."""
    FT = np.dtype(dtype).type
    t = np.asarray(t, dtype=FT)
    u = np.asarray(u, dtype=FT)
    x = np.atleast_1d(np.asarray(x, dtype=FT))
    n = len(t)
    h = np.diff(t)
    zs = np.zeros(n, dtype=FT)
    if n > 2:                              # Thomas algorithm on the interior second derivatives
        a = h[:-1].copy()
        b = FT(2) * (h[:-1] + h[1:])
        c = h[1:].copy()
        d = FT(6) * ((u[2:] - u[1:-1]) / h[1:] - (u[1:-1] - u[:-2]) / h[:-1])
        m = n - 2
        cp = np.zeros(m, dtype=FT)
        dp = np.zeros(m, dtype=FT)
        cp[0], dp[0] = c[0] / b[0], d[0] / b[0]
        for i in range(1, m):
            den = b[i] - a[i] * cp[i - 1]
            cp[i] = c[i] / den
            dp[i] = (d[i] - a[i] * dp[i - 1]) / den
        sol = np.zeros(m, dtype=FT)
        sol[-1] = dp[-1]
        for i in range(m - 2, -1, -1):
            sol[i] = dp[i] - cp[i] * sol[i + 1]
        zs[1:-1] = sol
    i = np.clip(np.searchsorted(t, x, side="right"), 1, n - 1)
    hi = h[i - 1]
    return (zs[i - 1] * (t[i] - x) ** 3 / (FT(6) * hi) + zs[i] * (x - t[i - 1]) ** 3 / (FT(6) * hi)
            + (u[i] / hi - zs[i] * hi / FT(6)) * (x - t[i - 1]) + (u[i - 1] / hi - zs[i - 1] * hi / FT(6)) * (t[i] - x))


def qoft(TT, TQ, T, T_ref=T_REF, dtype=np.float64):
    """Q(T_ref) / Q(T) (qoft!)."""
    return natural_spline(TT, TQ, [T_ref], dtype)[0] / natural_spline(TT, TQ, T, dtype)


# ---- the table, as the host hands it to the device -----------------------------------------------------------------------------------
def select_lines(table, grid, wing_cutoff, wavelength_flag=False):
    """(grid in wavenumbers ascending, indices of the lines with grid_min < nu0 < grid_max sorted by nu0): :62-68 and :86."""
    grid = np.asarray(grid, dtype=np.float64)
    gmax, gmin = grid.max() + wing_cutoff, grid.min() - wing_cutoff
    if wavelength_flag:
        grid = (NM_PER_M / grid)[::-1]
        gmin, gmax = NM_PER_M / gmax, NM_PER_M / gmin
    nu = np.asarray(table["nu"], dtype=np.float64)
    keep = np.nonzero((gmin < nu) & (nu < gmax))[0]
    return grid, keep[np.argsort(nu[keep], kind="stable")]


def frac_index(grid, x):
    """1-based fractional index of x (grid[0] <= x <= grid[-1]) by linear interpolation."""
    n = len(grid)
    k = int(np.clip(np.searchsorted(grid, x, side="right") - 1, 0, n - 2))
    return (k + 1) + (x - grid[k]) / (grid[k + 1] - grid[k])


def window(grid, nu, wing_cutoff, fracs=None):
    """(istart, istop), 1-based and inclusive; istop < istart is the empty window of the deviation."""
    n = len(grid)
    if n == 1:
        return 1, 1
    xl, xh = nu - wing_cutoff, nu + wing_cutoff
    if xh < grid[0] or xl > grid[-1]:
        return 1, 0
    out = []
    for x, clamped, end in ((xl, xl <= grid[0], 1), (xh, xh >= grid[-1], n)):
        if clamped:
            out.append(end)
            continue
        f = frac_index(grid, x)
        if fracs is not None:
            fracs.append(float(f))
        out.append(int(np.rint(f)))        # ties to even, as Julia's round
    return out[0], out[1]


def line_parameters(table, j, p, T, vmr, qratio, molar_mass, dtype=np.float64):
    """(nu, gamma_l, gamma_d, y, S) of line j at one layer: :108-136."""
    FT = np.dtype(dtype).type
    p, T, vmr = FT(p), FT(T), FT(vmr)
    v0 = FT(table["nu"][j])
    nu = v0 + p / FT(P_REF) * FT(table["delta_air"][j])
    gl = ((FT(table["gamma_air"][j]) * (FT(1) - vmr) * p / FT(P_REF) + FT(table["gamma_self"][j]) * vmr * p / FT(P_REF))
          * (FT(T_REF) / T) ** FT(table["n_air"][j]))
    gd = (FT(SQRT2LN2) / FT(CC)) * np.sqrt(FT(BOLTZ) / FT(MASSMOL)) * np.sqrt(T) * v0 / np.sqrt(FT(molar_mass))
    y = np.sqrt(FT(LN2)) * gl / gd
    S = FT(table["S"][j])
    E = FT(table["E_low"][j])
    if E != -1:
        S = (S * FT(qratio) * np.exp(FT(C2) * E * (FT(1) / FT(T_REF) - FT(1) / T)) * (-np.expm1(-FT(C2) * v0 / T))
             / (-np.expm1(-FT(C2) * v0 / FT(T_REF))))
    return nu, gl, gd, y, S


def cross_section_lines(grid, lines, species, molar_mass, qratio, p, T, vmr, broadening="Voigt", cef=CEFS[1], wing_cutoff=40.0,
                        dtype=np.float64, check_windows=True):
    """sigma [Nz, nSpec] from what the host hands the device: the grid in wavenumbers, `lines` a dict of arrays sorted by nu0,
    species [nLines], molar_mass [nSpecies], qratio [Nz, nSpecies] (in `dtype`), p, T, vmr [Nz].  The windows are found in float64
    in both formats (they are integers; the device finds them in float64)."""
    FT = np.dtype(dtype).type
    grid = np.asarray(grid, dtype=np.float64)
    gridF = grid.astype(FT)
    out = np.zeros((len(p), len(grid)), dtype=FT)
    fracs = []
    for iz in range(len(p)):
        for j in range(len(lines["nu"])):
            sp = int(species[j])
            nu, gl, gd, y, S = line_parameters(lines, j, p[iz], T[iz], vmr[iz], qratio[iz][sp], molar_mass[sp], dtype)
            nu64 = line_parameters(lines, j, p[iz], T[iz], vmr[iz], 1.0, molar_mass[sp], np.float64)[0]
            i0, i1 = window(grid, float(nu64), wing_cutoff, fracs)
            if i1 < i0:
                continue
            g = gridF[i0 - 1:i1]
            if broadening == "Doppler":
                term = S * FT(SQRTLN2_SQRTPI) * np.exp(-FT(LN2) * ((g - nu) / gd) ** 2) / gd
            elif broadening == "Lorentz":
                term = S * gl / (FT(math.pi) * (gl ** 2 + (g - nu) ** 2))
            elif broadening == "Voigt":
                z = (FT(SQRTLN2) / gd * (g - nu)) + _ctype(dtype)(1j) * y
                term = S * FT(SQRTLN2_SQRTPI) / gd * w(cef, z, dtype).real
            else:
                raise ValueError(broadening)
            out[iz, i0 - 1:i1] += term
    if check_windows and fracs:
        f = np.asarray(fracs)
        near = np.abs(f - np.floor(f) - 0.5)
        assert near.min() > HALF_INTEGER_GUARD, ("a fractional window index lies within %g of a half-integer: %r -- choose another "
                                                 "case" % (HALF_INTEGER_GUARD, f[np.argmin(near)]))
    return out


def cross_section(table, isotopologues, grid, p, T, vmr=0.0, broadening="Voigt", cef=CEFS[1], wing_cutoff=40.0,
                  wavelength_flag=False, dtype=np.float64, check_windows=True):
    """sigma [Nz, nSpec] of one gas: `table` a dict of arrays (mol, iso, nu, S, gamma_air, gamma_self, n_air, delta_air, E_low),
    `isotopologues` {(mol, iso): (molar_mass, TT, TQ)}, p / T [Nz], vmr a scalar or [Nz] (the self-broadening share)."""
    FT = np.dtype(dtype).type
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    vmr = np.broadcast_to(np.asarray(vmr, dtype=np.float64), p.shape)
    grid, sel = select_lines(table, grid, wing_cutoff, wavelength_flag)
    lines = {k: np.asarray(table[k])[sel] for k in ("nu", "S", "gamma_air", "gamma_self", "n_air", "delta_air", "E_low")}
    keys = sorted(set((int(table["mol"][j]), int(table["iso"][j])) for j in sel))
    species = np.asarray([keys.index((int(table["mol"][j]), int(table["iso"][j]))) for j in sel], dtype=int)
    qratio = np.ones((len(p), max(len(keys), 1)), dtype=FT)
    for i, key in enumerate(keys):
        if np.any(lines["E_low"][species == i] != -1):
            qratio[:, i] = qoft(isotopologues[key][1], isotopologues[key][2], T, dtype=dtype)
    mass = [isotopologues[key][0] for key in keys]
    out = cross_section_lines(grid, lines, species, mass, qratio, p, T, vmr, broadening, cef, wing_cutoff, dtype, check_windows)
    return out[:, ::-1] if wavelength_flag else out


def absorption_profile(gases, grid, p_full, T, vcd_dry, dtype=np.float64, **kw):
    """atmo_prof.jl:464-486 for a list of (table, isotopologues, self_vmr, vmr) gases: tau_abs [nSpec, Nz] and the per-gas
    sigma vcd_dry [nSpec, Nz] of atmo_prof_lin.jl:153."""
    FT = np.dtype(dtype).type
    vcd = np.asarray(vcd_dry, dtype=FT)
    tau = np.zeros((len(np.asarray(grid)), len(vcd)), dtype=FT)
    dots = []
    for table, isotopologues, self_vmr, vmr in gases:
        sig = cross_section(table, isotopologues, grid, p_full, T, self_vmr, dtype=dtype, **kw)
        vm = np.broadcast_to(np.asarray(vmr, dtype=FT), vcd.shape)
        tau = tau + (sig * (vcd * vm)[:, None]).T
        dots.append((sig * vcd[:, None]).T)
    return tau, dots
