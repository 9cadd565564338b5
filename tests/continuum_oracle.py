"""numpy oracles of the Absorption continua (HITRAN CIA and the MT_CKD H2O continuum).

(a) float64:  `planes64` restates the fixed chains of csrc/vsm_absorption_continuum.hip, the per-layer coefficient formulas
    included, operation for operation (numpy neither contracts nor reorders): a CIA-only set has to come out of the device with
    these bits.  `project_block`, `build_table`, `mtckd_band`, `sigma_at_T`, `reference_tau` and `layer_thickness` are the
    reference's loops (src/Absorption/cia.jl, mtckd.jl, CoreRT/tools/atmo_prof.jl:67) typed again, one element at a time.
(b) long double:  `planes_ld` evaluates every plane in the 80-bit format from the same FP64 inputs, and returns beside each plane
    the per-point sum of the absolute values of its terms: the scale every bound of the tests is relative to.  The T weight w of a
    CIA cell is an INPUT of the device chain (the host computes it in FP64), so (b) takes it rounded to FP64 too.

A set is (tables, band): tables a list of (species_a, species_b, Ts [nT], sig [nSpec, nT]); band None or a dict(nu, C_self, C_for,
texp, p_ref, T_ref).  Planes are ordered tau, dT, dp, one per species (`species_of`), ddz; each [Nz, nSpec]."""
import numpy as np

K_B = 1.380649e-23
C2 = 1.4388
VMR_DEFAULTS = {"O2": 0.20946, "N2": 0.78084}
R_GAS, DRY_MASS, WET_MASS, G0 = 8.3144598, 28.9644e-3, 18.01534e-3, 9.8032465


# ---- the reference's loops, literally ------------------------------------------------------------------------------------------
def searchsortedfirst(a, x):
    """1-based index of the first element >= x; len(a) + 1 if there is none."""
    return int(np.searchsorted(np.asarray(a), x, side="left")) + 1


def project_block(out, grid, nu_blk, sig_blk):
    """_accumulate_σ!"""
    lo, hi, n = nu_blk[0], nu_blk[-1], len(nu_blk)
    for k, q in enumerate(grid):
        if q < lo or q > hi:
            continue
        j = searchsortedfirst(nu_blk, q)
        if j <= 1:
            out[k] = sig_blk[0]
        elif j > n:
            out[k] = sig_blk[-1]
        else:
            n1, n2, s1, s2 = nu_blk[j - 2], nu_blk[j - 1], sig_blk[j - 2], sig_blk[j - 1]
            w = (q - n1) / (n2 - n1)
            out[k] = (1 - w) * s1 + w * s2
    return out


def build_table(blocks, grid):
    """build_cia_table: blocks a list of (T, nu, sig) in file order -> (Ts ascending, sig [nSpec, nT])."""
    Ts = sorted(set(float(b[0]) for b in blocks))
    sig = np.zeros((len(grid), len(Ts)))
    for jt, T_pick in enumerate(Ts):
        for T, nu, s in blocks:
            if T == T_pick:
                project_block(sig[:, jt], grid, nu, s)
    return np.asarray(Ts), sig


def mtckd_band(nu_t, C_self, C_for, texp, grid):
    """build_mtckd_band"""
    out = np.zeros((3, len(grid)))
    cols = (C_self, C_for, texp)
    for k, q in enumerate(grid):
        if q < nu_t[0] or q > nu_t[-1]:
            continue
        j = searchsortedfirst(nu_t, q)
        if j <= 1:
            out[:, k] = [c[0] for c in cols]
        elif j > len(nu_t):
            out[:, k] = [c[-1] for c in cols]
        else:
            n1, n2 = nu_t[j - 2], nu_t[j - 1]
            w = (q - n1) / (n2 - n1)
            out[:, k] = [(1 - w) * c[j - 2] + w * c[j - 1] for c in cols]
    return out


def sigma_at_T(Ts, sig, T):
    """cia_σ_at_T!"""
    if T <= Ts[0]:
        return sig[:, 0].copy()
    if T >= Ts[-1]:
        return sig[:, -1].copy()
    j = searchsortedfirst(Ts, T)
    T1, T2 = Ts[j - 2], Ts[j - 1]
    w = (T - T1) / (T2 - T1)
    return (1 - w) * sig[:, j - 2] + w * sig[:, j - 1]


def layer_vmr(species, vmr, iz):
    if species in vmr:
        v = vmr[species]
        return float(v[iz]) if np.ndim(v) else float(v)
    return VMR_DEFAULTS[species]


def reference_tau(tables, band, grid, p, T, dz, vmr):
    """compute_τ_cia! per table, then compute_τ_h2o_continuum!, into one tau [nSpec, Nz] of zeros."""
    tau = np.zeros((len(grid), len(p)))
    for a, b, Ts, sig in tables:
        for iz in range(len(p)):
            s_layer = sigma_at_T(Ts, sig, T[iz])
            n_air = p[iz] * 1e2 / (K_B * T[iz]) * 1e-6
            prod = layer_vmr(a, vmr, iz) * layer_vmr(b, vmr, iz) * n_air * n_air * (dz[iz] * 100.0)
            for k in range(len(grid)):
                tau[k, iz] += s_layer[k] * prod
    if band is not None:
        for iz in range(len(p)):
            v_h = layer_vmr("H2O", vmr, iz)
            n_air = p[iz] * 1e2 / (K_B * T[iz]) * 1e-6
            n_h2o, p_h2o = v_h * n_air, v_h * p[iz]
            p_dry, dz_cm = p[iz] - p_h2o, dz[iz] * 100.0
            self_ps, for_ps = p_h2o / band["p_ref"], p_dry / band["p_ref"]
            for k in range(len(grid)):
                nu = grid[k]
                rad = nu * np.tanh(C2 * nu / (2.0 * T[iz]))
                s_self = band["C_self"][k] * rad * self_ps * (band["T_ref"] / T[iz]) ** band["texp"][k]
                s_for = band["C_for"][k] * rad * for_ps
                tau[k, iz] += (s_self + s_for) * n_h2o * dz_cm
    return tau


def layer_thickness(p_half, T, vmr_h2o):
    dz = np.zeros(len(T))
    for i in range(len(T)):
        M = (1 - vmr_h2o[i]) * DRY_MASS + vmr_h2o[i] * WET_MASS
        dz[i] = (np.log(p_half[i + 1]) - np.log(p_half[i])) / (G0 * M / (R_GAS * T[i]))
    return dz


# ---- shared -------------------------------------------------------------------------------------------------------------------
def species_of(tables, band):
    sp = []
    for a, b, _, _ in tables:
        for s in (a, b):
            if s not in sp:
                sp.append(s)
    if band is not None and "H2O" not in sp:
        sp.append("H2O")
    return sp


def cell(Ts, T):
    """(j0, j1, w in FP64, clamped) of one layer: cia_σ_at_T!'s branches; clamped layers return an end column exactly."""
    Ts = np.asarray(Ts, dtype=np.float64)
    T = float(T)
    if T <= Ts[0]:
        return 0, 0, 0.0, True
    if T >= Ts[-1]:
        return len(Ts) - 1, len(Ts) - 1, 1.0, True
    j = searchsortedfirst(Ts, T)
    return j - 2, j - 1, (T - Ts[j - 2]) / (Ts[j - 1] - Ts[j - 2]), False


def _vmrs(species, vmr, Nz, dtype):
    out = {}
    for sp in species:
        v = vmr[sp] if sp in vmr else VMR_DEFAULTS[sp]
        out[sp] = np.broadcast_to(np.asarray(v, dtype=dtype), (Nz,))
    return out


# ---- (a): the device's chains in float64 ----------------------------------------------------------------------------------------
def planes64(tables, band, grid, p, T, dz, vmr, prefill=None):
    """Every plane [Nz, nSpec] as the device forms it: plane = prefill (or 0), then per table in list order
    plane += s_k A, on dT plane += (b - a) B, then the band's self and foreign term.  Returns a list in plane order."""
    f = np.float64
    grid, p, T, dz = (np.asarray(a, dtype=f) for a in (grid, p, T, dz))
    Nz, nSpec = len(p), len(grid)
    species = species_of(tables, band)
    vs = _vmrs(species, vmr, Nz, f)
    nP = 4 + len(species)
    out = [np.zeros((Nz, nSpec)) if prefill is None else np.array(prefill[m], dtype=f) for m in range(nP)]
    for z in range(Nz):
        n_air = p[z] * 1e2 / (K_B * T[z]) * 1e-6
        dz_cm = dz[z] * 100.0
        for a_sp, b_sp, Ts, sig in tables:
            j0, j1, w, clamped = cell(Ts, T[z])
            a, b = sig[:, j0], sig[:, j1]
            va, vb = vs[a_sp][z], vs[b_sp][z]
            prod = va * vb * n_air * n_air * dz_cm
            n2dz = n_air * n_air * dz_cm
            sk = (1.0 - w) * a + w * b
            out[0][z] = out[0][z] + sk * prod
            out[1][z] = out[1][z] + sk * (-2.0 * prod / T[z])
            out[1][z] = out[1][z] + (b - a) * (0.0 if clamped else prod / (Ts[j1] - Ts[j0]))
            out[2][z] = out[2][z] + sk * (2.0 * prod / p[z])
            for i, sp in enumerate(species):           # (a plane no species of the table owns gets + s_k 0)
                if a_sp == b_sp:
                    A = 2.0 * va * n2dz if sp == a_sp else 0.0
                else:
                    A = vb * n2dz if sp == a_sp else va * n2dz if sp == b_sp else 0.0
                out[3 + i][z] = out[3 + i][z] + sk * A
            out[nP - 1][z] = out[nP - 1][z] + sk * (prod / dz[z])
        if band is not None:
            v = vs["H2O"][z]
            ppr = p[z] / band["p_ref"]
            S = v * p[z] / band["p_ref"] * (v * n_air) * dz_cm
            F = (p[z] - v * p[z]) / band["p_ref"] * (v * n_air) * dz_cm
            te = band["texp"]
            x = C2 * grid / (2.0 * T[z])
            rad = grid * np.tanh(x)
            gs = rad * band["C_self"] * np.power(band["T_ref"] / T[z], te)
            gf = rad * band["C_for"]
            x2 = x + x
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                q = np.where(x2 == 0.0, 1.0, x2 / np.sinh(x2))
            invT = 1.0 / T[z]
            ts, tf = -((q + te + 1.0) * invT), -((q + 1.0) * invT)
            pairs = {0: (gs * S, gf * F), 1: ((gs * S) * ts, (gf * F) * tf), 2: (gs * (2.0 * S / p[z]), gf * (2.0 * F / p[z])),
                     3 + species.index("H2O"): (gs * (2.0 * v * ppr * n_air * dz_cm), gf * ((1.0 - 2.0 * v) * ppr * n_air * dz_cm)),
                     nP - 1: (gs * (S / dz[z]), gf * (F / dz[z]))}
            for m, (t_self, t_for) in pairs.items():
                out[m][z] = out[m][z] + t_self
                out[m][z] = out[m][z] + t_for
    return out


# ---- (b): long double, with the sums of absolute terms ---------------------------------------------------------------------------
def planes_ld(tables, band, grid, p, T, dz, vmr):
    """(planes, abs_sums): two lists in plane order, each [Nz, nSpec] in long double.  p, T, dz and the vmrs may be long doubles (the
    finite-difference checks perturb them); the cell of a CIA table and its FP64 weight are taken at the FP64 value of T."""
    L = np.longdouble
    grid = np.asarray(grid, dtype=L)
    p, T, dz = (np.asarray(a, dtype=L) for a in (p, T, dz))
    Nz, nSpec = len(p), len(grid)
    species = species_of(tables, band)
    vs = _vmrs(species, vmr, Nz, L)
    nP = 4 + len(species)
    val = [np.zeros((Nz, nSpec), dtype=L) for _ in range(nP)]
    mag = [np.zeros((Nz, nSpec), dtype=L) for _ in range(nP)]

    def add(m, z, term):
        val[m][z] += term
        mag[m][z] += np.abs(term)

    for z in range(Nz):
        n_air = p[z] * L(1e2) / (L(K_B) * T[z]) * L(1e-6)
        dz_cm = dz[z] * L(100.0)
        for a_sp, b_sp, Ts, sig in tables:
            j0, j1, w64, clamped = cell(Ts, np.float64(T[z]))
            a, b = sig[:, j0].astype(L), sig[:, j1].astype(L)
            if clamped:
                w = L(w64)
            else:       # the FP64 weight of the cell, moved with T in long double so that finite differences see a smooth function
                T1, T2 = L(Ts[j0]), L(Ts[j1])
                w = L(w64) + (T[z] - L(np.float64(T[z]))) / (T2 - T1)
            va, vb = vs[a_sp][z], vs[b_sp][z]
            n2dz = n_air * n_air * dz_cm
            prod = va * vb * n2dz
            sk = (1 - w) * a + w * b
            add(0, z, sk * prod)
            add(1, z, sk * (-2 * prod / T[z]))
            if not clamped:
                add(1, z, (b - a) * (prod / (T2 - T1)))
            add(2, z, sk * (2 * prod / p[z]))
            if a_sp == b_sp:
                add(3 + species.index(a_sp), z, sk * (2 * va * n2dz))
            else:
                add(3 + species.index(a_sp), z, sk * (vb * n2dz))
                add(3 + species.index(b_sp), z, sk * (va * n2dz))
            add(nP - 1, z, sk * (prod / dz[z]))
        if band is not None:
            v = vs["H2O"][z]
            ppr = p[z] / L(band["p_ref"])
            K = ppr * n_air * dz_cm
            te = band["texp"].astype(L)
            x = L(C2) * grid / (2 * T[z])
            rad = grid * np.tanh(x)
            gs = rad * band["C_self"].astype(L) * np.power(L(band["T_ref"]) / T[z], te)
            gf = rad * band["C_for"].astype(L)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                q = np.where(x == 0, L(1), 2 * x / np.sinh(2 * x))
            S, F = v * v * K, (1 - v) * v * K
            h = 3 + species.index("H2O")
            add(0, z, gs * S)
            add(0, z, gf * F)
            for g, c, extra in ((gs * S, te, True), (gf * F, None, False)):
                add(1, z, -g * q / T[z])
                if extra:
                    add(1, z, -g * c / T[z])
                add(1, z, -g / T[z])
            add(2, z, gs * S * 2 / p[z])
            add(2, z, gf * F * 2 / p[z])
            add(h, z, gs * (2 * v * K))
            add(h, z, gf * K)
            add(h, z, -gf * (2 * v * K))
            add(nP - 1, z, gs * S / dz[z])
            add(nP - 1, z, gf * F / dz[z])
    return val, mag
