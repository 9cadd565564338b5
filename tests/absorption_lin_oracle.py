"""numpy restatement of the linearized line-by-line absorption (vsm_absorption_xsec_lin): d sigma / d(T, p, vmr_self) per layer, with
the index windows and, per (line, point), the region of the error function frozen at the unperturbed state.  It builds on
tests/absorption_oracle.py (line parameters, windows, selection, spline); nothing here is imported by the package.

Every line shape is written term = pre F(x, y), x = sx (nu_i - nu):
    Voigt    pre = S c / gamma_d, sx = sqrt(ln 2) / gamma_d, y = sqrt(ln 2) gamma_l / gamma_d, F = Re w(x + i y)
    Doppler  pre = S c / gamma_d, sx = 1 / gamma_d,          y = 0,                            F = exp(-ln 2 x^2)
    Lorentz  pre = S / pi,        sx = 1,                    y = gamma_l,                      F = y / (x^2 + y^2)
and d term / d theta = pre (dlnpre_theta F + F_x x_theta + F_y y_theta).  The six factors that are not identically zero:
    ("T", "pre") dlnS/dT - 1/(2T) (Lorentz: dlnS/dT)     ("T", "x") -x/(2T) (Lorentz: 0)     ("T", "y") -y (n_air + 1/2)/T (Lorentz: -n_air y/T)
    ("p", "x") -sx delta_air/p_ref                        ("p", "y") y/p
    ("vmr_self", "y") sqrt(ln 2)/gamma_d (gamma_self - gamma_air) p/p_ref (T_ref/T)^n_air (Lorentz: without sqrt(ln 2)/gamma_d)
`drop` names one of them to leave out: the CPU test shows that each one matters.  F_x = Re w', F_y = -Im w' with w' the closed-form
derivative of each approximant.

Every function takes `dtype` (np.float64 or np.longdouble).  Besides the three slot sums the functions return A, the sum over lines
of |pre dlnpre F| + |pre F_x x_theta| + |pre F_y y_theta|: the scale against which a deviation is measured."""
import math

import numpy as np

import absorption_oracle as AO

SLOTS = ("T", "p", "vmr_self")
TERMS = (("T", "pre"), ("T", "x"), ("T", "y"), ("p", "x"), ("p", "y"), ("vmr_self", "y"))


# ---- the approximants and their derivatives: (w, dw/dz) --------------------------------------------------------------------------------
def weideman32a_lin(z, dtype=np.float64):
    """w = (1/sqrt(pi) + 2 P(Z) rec) rec, rec = 1 / (L - i z), Z = (L + i z) rec; dZ/dz = i rec (1 + Z), d rec/dz = i rec^2:
    w' = i rec^2 (1/sqrt(pi) + 2 rec (2 P + P' (1 + Z)))."""
    FT, CT = np.dtype(dtype).type, AO._ctype(dtype)
    z = np.asarray(z, dtype=CT)
    L32 = FT(math.sqrt(32 / math.sqrt(2)))
    iz = CT(1j) * z.real - z.imag
    rec = FT(1) / (L32 - iz)
    Z = (L32 + iz) * rec
    P = np.full(z.shape, FT(AO._W32[31]), dtype=CT)
    dP = np.zeros(z.shape, dtype=CT)
    for k in range(30, -1, -1):
        dP = dP * Z + P
        P = FT(AO._W32[k]) + P * Z
    w = (FT(AO.RSQRTPI) + FT(2) * P * rec) * rec
    dw = CT(1j) * rec * rec * (FT(AO.RSQRTPI) + FT(2) * rec * (FT(2) * P + dP * (FT(1) + Z)))
    return w, dw


def humlicek1_lin(z, dtype=np.float64):
    FT, CT = np.dtype(dtype).type, AO._ctype(dtype)
    z = np.asarray(z, dtype=CT)
    q = z * z
    inv = FT(1) / (q - FT(0.5))
    return CT(1j) * FT(AO.RSQRTPI) * z * inv, -CT(1j) * FT(AO.RSQRTPI) * (q + FT(0.5)) * inv * inv


def humlicek2_lin(z, dtype=np.float64):
    """t = -i z, w = N / D: dw/dz = -i (N' - w D') / D."""
    FT, CT = np.dtype(dtype).type, AO._ctype(dtype)
    z = np.asarray(z, dtype=CT)
    t = z.imag - CT(1j) * z.real
    u = t * t
    N = t * (FT(1.410474) + u * FT(AO.RSQRTPI))
    inv = FT(1) / (FT(3) / FT(4) + (u * (FT(3) + u)))
    w = N * inv
    dN = FT(1.410474) + FT(3) * FT(AO.RSQRTPI) * u
    dD = t * (FT(6) + FT(4) * u)
    return w, -CT(1j) * ((dN - w * dD) * inv)


def region(cef, x, y, dtype=np.float64):
    """True where w(CEF, x + i y) takes its Humlicek formula, False where Weideman's: the switch the forward function takes."""
    FT = np.dtype(dtype).type
    if cef == AO.CEFS[0]:
        return np.abs(x) + y > FT(15)
    if cef == AO.CEFS[1]:
        return np.abs(x) + y >= FT(8)
    raise ValueError("%s is not linearized" % cef)


def w_lin(cef, z, dtype=np.float64, humlicek=None):
    """(w, dw/dz) with the region chosen at z, or given (`humlicek`, a mask: the frozen region of a perturbed evaluation)."""
    CT = AO._ctype(dtype)
    z = np.atleast_1d(np.asarray(z, dtype=CT))
    if humlicek is None:
        humlicek = region(cef, z.real, z.imag, dtype)
    h = (humlicek1_lin if cef == AO.CEFS[0] else humlicek2_lin)(z, dtype)
    g = weideman32a_lin(z, dtype)
    return np.where(humlicek, h[0], g[0]), np.where(humlicek, h[1], g[1])


def shape(broadening, cef, x, y, dtype=np.float64, humlicek=None):
    """(F, F_x, F_y) at arrays x and a scalar y."""
    FT, CT = np.dtype(dtype).type, AO._ctype(dtype)
    if broadening == "Doppler":
        F = np.exp(-FT(AO.LN2) * (x * x))
        return F, -FT(2) * FT(AO.LN2) * x * F, np.zeros(x.shape, dtype=FT)
    if broadening == "Lorentz":
        s = FT(1) / (y * y + x * x)
        return y * s, -FT(2) * (x * y) * (s * s), (x * x - y * y) * (s * s)
    if broadening == "Voigt":
        w, dw = w_lin(cef, x + CT(1j) * y, dtype, humlicek)
        return w.real, dw.real, -dw.imag
    raise ValueError(broadening)


# ---- the per-line record -----------------------------------------------------------------------------------------------------------
def line_record(lines, j, p, T, vmr, qratio, dlnq, molar_mass, broadening, dtype=np.float64):
    """dict(nu, pre, sx, y and the factors (slot, kind) of TERMS; x_T = x r[("T", "x")]) of line j at one layer."""
    FT = np.dtype(dtype).type
    nu, gl, gd, y, S = AO.line_parameters(lines, j, p, T, vmr, qratio, molar_mass, dtype)
    p, T = FT(p), FT(T)
    v0, n, dl, E = FT(lines["nu"][j]), FT(lines["n_air"][j]), FT(lines["delta_air"][j]), FT(lines["E_low"][j])
    dlnS = FT(0)
    if E != -1:
        a = FT(AO.C2) * v0 / T
        dlnS = FT(dlnq) + FT(AO.C2) * E / (T * T) - (a / T) / np.expm1(a)
    gl_v = (FT(lines["gamma_self"][j]) - FT(lines["gamma_air"][j])) * p / FT(AO.P_REF) * (FT(AO.T_REF) / T) ** n
    if broadening == "Lorentz":
        r = {"pre": S / FT(math.pi), "sx": FT(1), "y": gl, ("T", "x"): FT(0)}
        r[("T", "pre")], r[("T", "y")], r[("p", "y")], r[("vmr_self", "y")] = dlnS, -n * gl / T, gl / p, gl_v
    else:
        voigt = broadening == "Voigt"
        r = {"pre": S * FT(AO.SQRTLN2_SQRTPI) / gd, "sx": (FT(AO.SQRTLN2) if voigt else FT(1)) / gd, "y": y if voigt else FT(0),
             ("T", "x"): -FT(0.5) / T}
        r[("T", "pre")] = dlnS - FT(0.5) / T
        r[("T", "y")], r[("p", "y")] = -r["y"] * (n + FT(0.5)) / T, r["y"] / p
        r[("vmr_self", "y")] = np.sqrt(FT(AO.LN2)) * gl_v / gd if voigt else FT(0)
    r[("p", "x")] = -r["sx"] * dl / FT(AO.P_REF)
    r["nu"] = nu
    return r


def cross_section_lin_lines(grid, lines, species, molar_mass, qratio, dlnq, p, T, vmr, broadening="Voigt", cef=AO.CEFS[1],
                            wing_cutoff=40.0, dtype=np.float64, drop=None):
    """(dot, A), each [3, Nz, nSpec], from what the host hands the device (see AO.cross_section_lines; dlnq [Nz, nSpecies] beside
    qratio).  The windows are found in float64 in both formats."""
    FT = np.dtype(dtype).type
    grid = np.asarray(grid, dtype=np.float64)
    gridF = grid.astype(FT)
    dot = np.zeros((3, len(p), len(grid)), dtype=FT)
    A = np.zeros((3, len(p), len(grid)), dtype=FT)
    for iz in range(len(p)):
        for j in range(len(lines["nu"])):
            sp = int(species[j])
            nu64 = AO.line_parameters(lines, j, p[iz], T[iz], vmr[iz], 1.0, molar_mass[sp], np.float64)[0]
            i0, i1 = AO.window(grid, float(nu64), wing_cutoff)
            if i1 < i0:
                continue
            r = line_record(lines, j, p[iz], T[iz], vmr[iz], qratio[iz][sp], dlnq[iz][sp], molar_mass[sp], broadening, dtype)
            x = r["sx"] * (gridF[i0 - 1:i1] - r["nu"])
            mask = None
            if broadening == "Voigt":                  # the region, like the window, is found in float64 in both formats
                r64 = r if FT is np.float64 else line_record(lines, j, p[iz], T[iz], vmr[iz], float(qratio[iz][sp]),
                                                             float(dlnq[iz][sp]), molar_mass[sp], broadening, np.float64)
                mask = region(cef, r64["sx"] * (grid[i0 - 1:i1] - r64["nu"]), r64["y"])
            F, Fx, Fy = shape(broadening, cef, x, r["y"], dtype, mask)
            fac = {k: (FT(0) if k == drop else r[k]) for k in TERMS}
            terms = {"T": (fac[("T", "pre")] * F, Fx * (x * fac[("T", "x")]), Fy * fac[("T", "y")]),
                     "p": (Fx * fac[("p", "x")], Fy * fac[("p", "y")]),
                     "vmr_self": (Fy * fac[("vmr_self", "y")],)}
            for k, slot in enumerate(SLOTS):
                dot[k, iz, i0 - 1:i1] += r["pre"] * sum(terms[slot])
                A[k, iz, i0 - 1:i1] += sum(np.abs(r["pre"] * t) for t in terms[slot])
    return dot, A


def natural_spline_lin(t, u, x, dtype=np.float64):
    """(value, derivative) of AO.natural_spline at x: the spline's own analytic derivative, from the same second derivatives (Thomas
    algorithm on the interior knots, zero at both ends)."""
    FT = np.dtype(dtype).type
    t = np.asarray(t, dtype=FT)
    u = np.asarray(u, dtype=FT)
    x = np.atleast_1d(np.asarray(x, dtype=FT))
    n = len(t)
    h = np.diff(t)
    zs = np.zeros(n, dtype=FT)
    if n > 2:
        b = FT(2) * (h[:-1] + h[1:])
        d = FT(6) * ((u[2:] - u[1:-1]) / h[1:] - (u[1:-1] - u[:-2]) / h[:-1])
        cp, dp = np.zeros(n - 2, dtype=FT), np.zeros(n - 2, dtype=FT)
        cp[0], dp[0] = h[1] / b[0], d[0] / b[0]
        for i in range(1, n - 2):
            den = b[i] - h[i] * cp[i - 1]
            cp[i], dp[i] = h[i + 1] / den, (d[i] - h[i] * dp[i - 1]) / den
        for i in range(n - 3, -1, -1):
            zs[i + 1] = dp[i] - (cp[i] * zs[i + 2] if i < n - 3 else FT(0))
    i = np.clip(np.searchsorted(t, x, side="right"), 1, n - 1)
    hi = h[i - 1]
    d = (-zs[i - 1] * (t[i] - x) ** 2 / (FT(2) * hi) + zs[i] * (x - t[i - 1]) ** 2 / (FT(2) * hi)
         + (u[i] / hi - zs[i] * hi / FT(6)) - (u[i - 1] / hi - zs[i - 1] * hi / FT(6)))
    return AO.natural_spline(t, u, x, dtype), d


def qoft_lin(TT, TQ, T, T_ref=AO.T_REF, dtype=np.float64):
    """(Q(T_ref) / Q(T), d/dT of it)."""
    q, dq = natural_spline_lin(TT, TQ, T, dtype)
    q_ref = AO.natural_spline(TT, TQ, [T_ref], dtype)[0]
    return q_ref / q, -q_ref * dq / (q * q)


def _selection(table, isotopologues, grid, p, T, vmr, wing_cutoff, wavelength_flag, dtype):
    FT = np.dtype(dtype).type
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    vmr = np.broadcast_to(np.asarray(vmr, dtype=np.float64), p.shape)
    grid, sel = AO.select_lines(table, grid, wing_cutoff, wavelength_flag)
    lines = {k: np.asarray(table[k])[sel] for k in ("nu", "S", "gamma_air", "gamma_self", "n_air", "delta_air", "E_low")}
    keys = sorted(set((int(table["mol"][j]), int(table["iso"][j])) for j in sel))
    species = np.asarray([keys.index((int(table["mol"][j]), int(table["iso"][j]))) for j in sel], dtype=int)
    qratio = np.ones((len(p), max(len(keys), 1)), dtype=FT)
    dlnq = np.zeros((len(p), max(len(keys), 1)), dtype=FT)
    for i, key in enumerate(keys):
        if np.any(lines["E_low"][species == i] != -1):
            r, d = qoft_lin(isotopologues[key][1], isotopologues[key][2], T, dtype=dtype)
            qratio[:, i], dlnq[:, i] = r, d / r
    mass = [isotopologues[key][0] for key in keys]
    return grid, lines, species, mass, qratio, dlnq, p, T, vmr


def cross_section_lin(table, isotopologues, grid, p, T, vmr=0.0, broadening="Voigt", cef=AO.CEFS[1], wing_cutoff=40.0,
                      wavelength_flag=False, dtype=np.float64, drop=None):
    """(dot, A), each [3, Nz, nSpec], of one gas; the arguments of AO.cross_section."""
    grid, lines, species, mass, qratio, dlnq, p, T, vmr = _selection(table, isotopologues, grid, p, T, vmr, wing_cutoff,
                                                                     wavelength_flag, dtype)
    dot, A = cross_section_lin_lines(grid, lines, species, mass, qratio, dlnq, p, T, vmr, broadening, cef, wing_cutoff, dtype, drop)
    return (dot[:, :, ::-1], A[:, :, ::-1]) if wavelength_flag else (dot, A)


def absorption_profile_lin(gases, grid, p_full, T, vcd_dry, dtype=np.float64, **kw):
    """For a list of (table, isotopologues, self_vmr, vmr) gases: (dtau_dT, dtau_dp [nSpec, Nz], dtau_dvmr_self [g][nSpec, Nz]) and
    the matching A's, in the same layout."""
    FT = np.dtype(dtype).type
    vcd = np.asarray(vcd_dry, dtype=FT)
    n = len(np.asarray(grid))
    tot, totA = np.zeros((2, n, len(vcd)), dtype=FT), np.zeros((2, n, len(vcd)), dtype=FT)
    dv, dvA = [], []
    for table, isotopologues, self_vmr, vmr in gases:
        dot, A = cross_section_lin(table, isotopologues, grid, p_full, T, self_vmr, dtype=dtype, **kw)
        sc = (vcd * np.broadcast_to(np.asarray(vmr, dtype=FT), vcd.shape))[None, :, None]
        d, a = np.transpose(dot * sc, (0, 2, 1)), np.transpose(A * np.abs(sc), (0, 2, 1))
        tot, totA = tot + d[:2], totA + a[:2]
        dv.append(d[2])
        dvA.append(a[2])
    return (tot[0], tot[1], dv), (totA[0], totA[1], dvA)


# ---- the finite-difference side: frozen windows, frozen regions ------------------------------------------------------------------------
def forward_frozen(grid, lines, species, molar_mass, isotopologue_tables, p, T, vmr, base, broadening, cef, wing_cutoff,
                   dtype=np.longdouble):
    """sigma [Nz, nSpec] of the FORWARD oracle's pieces (AO.line_parameters, the AO approximants) at a perturbed (p, T, vmr), with the
    windows and the Humlicek / Weideman masks of the base state `base` = (p, T, vmr).  isotopologue_tables[sp] = (TT, TQ) or None."""
    FT, CT = np.dtype(dtype).type, AO._ctype(dtype)
    grid = np.asarray(grid, dtype=np.float64)
    gridF = grid.astype(FT)
    out = np.zeros((len(p), len(grid)), dtype=FT)
    hum = AO.humlicek1 if cef == AO.CEFS[0] else AO.humlicek2
    for iz in range(len(p)):
        for j in range(len(lines["nu"])):
            sp = int(species[j])
            nu64 = AO.line_parameters(lines, j, base[0][iz], base[1][iz], base[2][iz], 1.0, molar_mass[sp], np.float64)[0]
            i0, i1 = AO.window(grid, float(nu64), wing_cutoff)
            if i1 < i0:
                continue
            tab = isotopologue_tables[sp]
            q = FT(1) if tab is None else AO.qoft(tab[0], tab[1], [T[iz]], dtype=dtype)[0]
            _, gl, gd, y, S = AO.line_parameters(lines, j, p[iz], T[iz], vmr[iz], q, molar_mass[sp], dtype)
            # nu_i - nu = (nu_i - nu0) - p / p_ref delta_air: the forward's value without the rounding of nu near 6000, which a
            # difference over a pressure step of 2e-4 hPa (a shift of 1e-9 cm^-1) would otherwise magnify
            dn = (gridF[i0 - 1:i1] - FT(lines["nu"][j])) - FT(p[iz]) / FT(AO.P_REF) * FT(lines["delta_air"][j])
            if broadening == "Doppler":
                term = S * FT(AO.SQRTLN2_SQRTPI) * np.exp(-FT(AO.LN2) * (dn / gd) ** 2) / gd
            elif broadening == "Lorentz":
                term = S * gl / (FT(math.pi) * (gl ** 2 + dn ** 2))
            else:
                nub, _, gdb, yb, _ = AO.line_parameters(lines, j, base[0][iz], base[1][iz], base[2][iz], 1.0, molar_mass[sp], np.float64)
                mask = region(cef, AO.SQRTLN2 / gdb * (grid[i0 - 1:i1] - nub), yb)
                z = (FT(AO.SQRTLN2) / gd * dn) + CT(1j) * y
                term = S * FT(AO.SQRTLN2_SQRTPI) / gd * np.where(mask, hum(z, dtype), AO.weideman32a(z, dtype)).real
            out[iz, i0 - 1:i1] += term
    return out


def richardson_differences(table, isotopologues, grid, p, T, vmr, broadening="Voigt", cef=AO.CEFS[1], wing_cutoff=40.0, rel_step=2e-3,
                           dtype=np.longdouble):
    """[3, Nz, nSpec]: two-level Richardson central differences (steps h and h / 2, error O(h^4)) of forward_frozen in T, p and
    vmr_self, relative step rel_step (absolute for vmr_self, which may be zero)."""
    FT = np.dtype(dtype).type
    grid, lines, species, mass, _, _, p, T, vmr = _selection(table, isotopologues, grid, p, T, vmr, wing_cutoff, False, dtype)
    keys = sorted(set((int(table["mol"][j]), int(table["iso"][j])) for j in AO.select_lines(table, grid, wing_cutoff)[1]))
    tabs = []
    for i, key in enumerate(keys):
        needs = np.any(lines["E_low"][species == i] != -1)
        tabs.append((isotopologues[key][1], isotopologues[key][2]) if needs else None)
    base = (p, T, vmr)
    out = []
    for k in (1, 0, 2):                                # SLOTS order: T, p, vmr_self
        def f(step):
            state = [np.asarray(a, dtype=FT) for a in base]
            h = state[k] * FT(step) if k < 2 else np.full(state[k].shape, FT(step))
            hi, lo = list(state), list(state)
            hi[k], lo[k] = state[k] + h, state[k] - h
            fp = forward_frozen(grid, lines, species, mass, tabs, hi[0], hi[1], hi[2], base, broadening, cef, wing_cutoff, dtype)
            fm = forward_frozen(grid, lines, species, mass, tabs, lo[0], lo[1], lo[2], base, broadening, cef, wing_cutoff, dtype)
            return (fp - fm) / (FT(2) * h)[:, None]
        d1, d2 = f(rel_step), f(rel_step / 2)
        out.append((FT(4) * d2 - d1) / FT(3))
    return np.stack(out)
