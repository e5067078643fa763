"""Seeded input families, per-variable physical scales and block layouts shared by
tests/golden/make_reference_vectors.py and tests/test_reference_vectors.py (test infrastructure).

Everything here is plain numpy; nothing is taken from the code under test.  States are rows in NATURAL variable
order (rho, v1, v2, v3, p[, B1, B2, B3, psi]); a "case for direction ivx" is the x1 case with its vector components
rotated cyclically (x1 -> x_ivx), which is the permutation the reference's solvers apply on load and store."""
import numpy as np

from oracle import oracle as O

NV = {"euler": 5, "glmmhd": 9}
GAMMA = 5.0 / 3.0
RECONS = ("dc", "plm", "ppm", "wenoz", "weno3", "limo3")
RADIUS = {"dc": 0, "plm": 1, "weno3": 1, "limo3": 1, "ppm": 2, "wenoz": 2}      # stencil half-width in cells
SOLVERS = {"euler": ("hlle", "hllc", "llf"), "glmmhd": ("hlle", "hlld", "llf")}
RIEMANN_FAMILIES = {"euler": ("subsonic", "supersonic", "cgs"),
                    "glmmhd": ("subsonic", "supersonic", "b0", "bx0", "cgs")}
RECON_FAMILIES = ("uniform", "logmag", "noise")
C2P_REGIMES = ("floors_off", "dfloor", "pfloor", "efloor", "vceil", "eceil")
PENCIL_COMBOS = [(f, rc, rs) for f, rs in (("euler", "hllc"), ("glmmhd", "hlld")) for rc in ("plm", "ppm", "wenoz", "weno3", "limo3")]
PENCIL_NX, PENCIL_NG, PENCIL_DX = 70, 3, 0.1
CGS_C_H = 1.0e8


# ---- rotations ---------------------------------------------------------------------------------------------------
def _perm(nv, ivx):
    """index array p with rotated[..., p[a]] = x1case[..., a]"""
    p = np.arange(nv)
    for k in range(3):
        p[1 + k] = 1 + (ivx - 1 + k) % 3
        if nv >= 9:
            p[5 + k] = 5 + (ivx - 1 + k) % 3
    return p


def rotate(w, ivx, axis=-1):
    """the x1 case (states or fluxes, variables along `axis`) as a case for direction ivx"""
    w = np.asarray(w)
    p = _perm(w.shape[axis], ivx)
    out = np.empty_like(w)
    idx = [slice(None)] * w.ndim
    src = [slice(None)] * w.ndim
    for a in range(w.shape[axis]):
        idx[axis], src[axis] = p[a], a
        out[tuple(idx)] = w[tuple(src)]
    return out


def unrotate(w, ivx, axis=-1):
    w = np.asarray(w)
    return np.take(w, _perm(w.shape[axis], ivx), axis=axis)


# ---- Riemann state families ----------------------------------------------------------------------------------------
def riemann_family(fluid, family, n, rng):
    """(wl, wr, c_h): n admissible left/right primitive pairs [n][nv] for a sweep along x1"""
    nv = NV[fluid]

    def side():
        w = np.zeros((n, nv))
        w[:, 0] = rng.uniform(0.1, 2.0, n)
        w[:, 1:4] = rng.uniform(-0.3, 0.3, (n, 3))
        w[:, 4] = rng.uniform(0.5, 3.0, n)
        if nv == 9:
            w[:, 5:8] = rng.uniform(-1.0, 1.0, (n, 3))
            w[:, 8] = rng.uniform(-0.3, 0.3, n)
        return w
    wl, wr, c_h = side(), side(), 2.0
    if family == "subsonic":
        pass
    elif family == "supersonic":
        sgn = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
        wl[:, 1] = sgn * rng.uniform(3.0, 8.0, n)
        wr[:, 1] = sgn * rng.uniform(3.0, 8.0, n)
    elif family == "b0":            # a hydro wave through the MHD solver: the whole magnetic subsystem is
        wl[:, 5:] = 0.0             # off, psi included -- with psi != 0 the GLM interface field -(psi_R - psi_L) / (2 c_h)
        wr[:, 5:] = 0.0             # is not zero and the case is no B = 0 case (the solvers then return a transverse
                                    # field flux that the scale below, built from the two states alone, does not contain)
    elif family == "bx0":
        wl[:, 5] = 0.0
        wr[:, 5] = 0.0
    elif family == "cgs":           # rho ~ 1e-27 g/cm^3, p ~ 1e-13 erg/cm^3, v ~ 1e7 cm/s, B ~ 3e-7 (code units), c_h = 1e8
        for w in (wl, wr):
            w[:, 0] = 1e-27 * rng.uniform(0.5, 2.0, n)
            w[:, 1:4] = 1e7 * rng.uniform(-1.0, 1.0, (n, 3))
            w[:, 4] = 1e-13 * rng.uniform(0.5, 2.0, n)
            if nv == 9:
                w[:, 5:8] = 3e-7 * rng.uniform(-1.0, 1.0, (n, 3))
                w[:, 8] = 3e-7 * 1e7 * rng.uniform(-0.1, 0.1, n)
        c_h = CGS_C_H
    else:
        raise ValueError(family)
    return wl, wr, (c_h if fluid == "glmmhd" else 0.0)


# ---- per-variable scale --------------------------------------------------------------------------------------------
def cell_scale(fluid, w, ivx, gamma, c_h):
    """max(|F_v(W)|, S |U_v(W)|) per cell and variable, natural order, for the physical flux F along direction ivx, the
    conserved state U and S = max(|v_n| + c_fast, c_h): the magnitude of the terms a Riemann solver adds up."""
    w = np.asarray(w, dtype=np.float64)
    nv = w.shape[-1]
    d, v, p = w[..., 0], w[..., 1:4], w[..., 4]
    n = ivx - 1
    vn = v[..., n]
    F, U = np.zeros_like(w), np.zeros_like(w)
    ke = 0.5 * d * np.sum(v * v, axis=-1)
    if nv == 5:
        E = p / (gamma - 1.0) + ke
        ptot = p
        cf = np.sqrt(gamma * p / d)
        S = np.abs(vn) + cf
    else:
        B, psi = w[..., 5:8], w[..., 8]
        Bn = B[..., n]
        b2 = np.sum(B * B, axis=-1)
        E = p / (gamma - 1.0) + ke + 0.5 * b2
        ptot = p + 0.5 * b2
        asq, ct2 = gamma * p, b2 - Bn * Bn
        cf = np.sqrt(0.5 * (b2 + asq + np.sqrt((b2 - asq) ** 2 + 4.0 * asq * ct2)) / d)
        S = np.maximum(np.abs(vn) + cf, c_h)
    F[..., 0], U[..., 0] = d * vn, d
    for i in range(3):
        F[..., 1 + i] = d * vn * v[..., i] + (ptot if i == n else 0.0)
        U[..., 1 + i] = d * v[..., i]
    F[..., 4], U[..., 4] = (E + ptot) * vn, E
    if nv == 9:
        vb = np.sum(v * B, axis=-1)
        for i in range(3):
            F[..., 1 + i] -= Bn * B[..., i]
            F[..., 5 + i] = psi if i == n else B[..., i] * vn - v[..., i] * Bn
            U[..., 5 + i] = B[..., i]
        F[..., 4] -= Bn * vb
        F[..., 8], U[..., 8] = c_h * c_h * Bn, psi
    return np.maximum(np.abs(F), S[..., None] * np.abs(U))


def riemann_scale(fluid, wl, wr, ivx, gamma, c_h):
    return np.maximum(cell_scale(fluid, wl, ivx, gamma, c_h), cell_scale(fluid, wr, ivx, gamma, c_h))


def pencil_scale(fluid, w, recon, gamma, c_h):
    """[ncell][nv]: scale of face i (the lower face of cell i) = max over the cells i-1-r .. i+r that feed it"""
    cs = cell_scale(fluid, w, 1, gamma, c_h)
    n, r = cs.shape[0], RADIUS[recon]
    out = np.zeros_like(cs)
    for i in range(n):
        out[i] = cs[max(0, i - 1 - r):min(n, i + r + 1)].max(axis=0)
    return out


def floor32(a):
    """the largest float32 <= a (a >= 0): scales are stored in single precision, never rounded up"""
    a = np.asarray(a, dtype=np.float64)
    f = a.astype(np.float32)
    up = f.astype(np.float64) > a
    f[up] = np.nextafter(f[up], np.float32(0.0))
    assert np.all(f.astype(np.float64) <= a)
    return f


# ---- reconstruction stencils -----------------------------------------------------------------------------------------
def recon_family(family, n, rng):
    if family == "uniform":
        return rng.uniform(-1.0, 1.0, (n, 5))
    if family == "logmag":
        return np.where(rng.uniform(size=(n, 5)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-12.0, 6.0, (n, 5))
    if family == "noise":
        return 1.0 + 10.0 ** rng.uniform(-16.0, -8.0, (n, 5)) * rng.uniform(-1.0, 1.0, (n, 5))
    raise ValueError(family)


# ---- ConsToPrim states ---------------------------------------------------------------------------------------------
def c2p_family(fluid, regime, n, rng, gamma=GAMMA):
    """(eos kwargs, u [n][nv + 1]): conserved states with one passive scalar; in every regime but floors_off about half
    of the states trip the floor or ceiling that is on.  No state has a non-positive density or pressure while the
    matching floor is off (the reference aborts on those)."""
    nv = NV[fluid]
    d = rng.uniform(0.2, 2.0, n)
    v = rng.uniform(-0.5, 0.5, (n, 3))
    p = rng.uniform(0.2, 2.0, n)
    B = rng.uniform(-0.7, 0.7, (n, 3)) if nv == 9 else np.zeros((n, 3))
    eos = {}
    if regime == "dfloor":
        eos = dict(dfloor=0.8, pfloor=1e-3)
    elif regime == "pfloor":
        eos = dict(pfloor=0.5)
        p = 10.0 ** rng.uniform(-1.3, 0.9, n) * np.where(rng.uniform(size=n) < 0.2, -1.0, 1.0)
    elif regime == "efloor":
        eos = dict(efloor=1.2)      # p / ((gamma - 1) rho) against 1.2
    elif regime == "vceil":
        eos = dict(vceil=0.45)
    elif regime == "eceil":
        eos = dict(eceil=1.2)
    elif regime != "floors_off":
        raise ValueError(regime)
    u = np.zeros((n, nv + 1))
    u[:, 0] = d
    u[:, 1:4] = d[:, None] * v
    u[:, 4] = p / (gamma - 1.0) + 0.5 * d * np.sum(v * v, axis=1) + 0.5 * np.sum(B * B, axis=1)
    if nv == 9:
        u[:, 5:8] = B
        u[:, 8] = rng.uniform(-0.2, 0.2, n)
    u[:, nv] = d * rng.uniform(0.0, 1.0, n)
    return eos, u


def c2p_scale(fluid, u, u_after, w, gamma):
    """[2][n][nv+1] scales of (cons after floors, prim): the magnitude of the terms each entry is made of -- vector
    norms for momentum / velocity / field components, the total energy for the energy and (times gamma - 1) for the
    pressure, which is a difference of energies"""
    nv = NV[fluid]
    d = np.abs(u_after[:, 0])
    m = np.sqrt(np.sum(u_after[:, 1:4] ** 2, axis=1))
    e = np.maximum(np.abs(u[:, 4]), np.abs(u_after[:, 4]))
    su, sw = np.zeros_like(u), np.zeros_like(u)
    su[:, 0], sw[:, 0] = d, d
    su[:, 1:4], sw[:, 1:4] = m[:, None], (m / d)[:, None]
    su[:, 4], sw[:, 4] = e, (gamma - 1.0) * e
    if nv == 9:
        b = np.sqrt(np.sum(u[:, 5:8] ** 2, axis=1))
        su[:, 5:8], sw[:, 5:8] = b[:, None], b[:, None]
        su[:, 8], sw[:, 8] = np.abs(u[:, 8]), np.abs(u[:, 8])
    su[:, nv], sw[:, nv] = np.abs(u[:, nv]), np.abs(u[:, nv]) / d
    return np.stack([su, sw])


# ---- pencils -----------------------------------------------------------------------------------------------------
def pencil(fluid, kind, rng, ncell=PENCIL_NX + 2 * PENCIL_NG):
    """[ncell][nv] admissible primitive states along a line: 'smooth' (sines + 1e-3 noise) or 'jumps' (piecewise
    constant with five discontinuities + 1e-3 noise)"""
    nv = NV[fluid]
    x = np.arange(ncell) / ncell
    base = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.3, 0.0, 0.0, 0.0])[:nv]
    amp = np.array([0.3, 0.4, 0.3, 0.2, 0.4, 0.2, 0.5, 0.5, 0.05])[:nv]
    w = np.zeros((ncell, nv))
    if kind == "smooth":
        ph = rng.uniform(0, 2 * np.pi, nv)
        for a in range(nv):
            w[:, a] = base[a] + amp[a] * np.sin(2 * np.pi * (1 + a % 3) * x + ph[a])
    elif kind == "jumps":
        edges = np.sort(rng.choice(np.arange(6, ncell - 6), 5, replace=False))
        seg = np.searchsorted(edges, np.arange(ncell), side="right")
        lev = rng.uniform(-1.0, 1.0, (6, nv))
        for a in range(nv):
            w[:, a] = base[a] + amp[a] * lev[seg, a]
    else:
        raise ValueError(kind)
    w += 1e-3 * rng.standard_normal((ncell, nv)) * (amp > 0)
    assert w[:, 0].min() > 0.3 and w[:, 4].min() > 0.3
    return w


def pencil_block(pencils, d, ng=PENCIL_NG):
    """primitives [1][nv][Nk][Nj][Ni] of the (nx,) + 2 x 2 block whose lines along x1 are the given x1 pencils
    ([ncell][nv], ncell = nx + 2 ng; line (k, j) holds pencil (j + k) % len), transposed and rotated for sweep direction
    d so that the same lines run along x_d.  Returns (nx tuple, prim)."""
    ncell, nv = pencils[0].shape
    N = 2 + 2 * ng
    w = np.zeros((nv, N, N, ncell))
    for k in range(N):
        for j in range(N):
            w[:, k, j, :] = pencils[(j + k) % len(pencils)].T
    nx = [ncell - 2 * ng, 2, 2]
    if d == 2:      # (i', j', k') = (k, i, j)
        w, nx = rotate(w, 2, axis=0).transpose(0, 2, 3, 1), [2, nx[0], 2]
    elif d == 3:    # (i', j', k') = (j, k, i)
        w, nx = rotate(w, 3, axis=0).transpose(0, 3, 1, 2), [2, 2, nx[0]]
    return tuple(nx), np.ascontiguousarray(w)[None]


def pencil_block_faces(flux, d, npencils, ng=PENCIL_NG):
    """from the d-flux [nv][Nk][Nj][Ni] of pencil_block(..., d): the face fluxes of the interior lines as x1 cases,
    [npencils-or-more lines][ncell][nv] with line l = pencil index of (j, k) = (ng + l, ng); faces outside
    ng .. ncell - ng are not meaningful"""
    f = np.asarray(flux)
    if d == 2:
        f = unrotate(f.transpose(0, 3, 1, 2), 2, axis=0)
    elif d == 3:
        f = unrotate(f.transpose(0, 2, 3, 1), 3, axis=0)
    out = []
    for j, k in ((ng, ng), (ng + 1, ng), (ng, ng + 1), (ng + 1, ng + 1)):     # all four interior lines
        out.append(((j + k) % npencils, f[:, k, j, :].T))
    return out


# ---- the reference binary (oracle/_ref/ref_vectors, see oracle/ref/ref_vectors.cpp) -----------------------------------
def ref_recon(method, q, dx, positivity):
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 5)
    out = O.ref_run(["recon", method, q.shape[0], float(dx), int(positivity)], q)
    return out[:q.shape[0]], out[q.shape[0]:]


def ref_riemann(fluid, solver, ivx, wl, wr, gamma, c_h):
    nv = NV[fluid]
    wl = np.ascontiguousarray(wl, dtype=np.float64).reshape(-1, nv)
    wr = np.ascontiguousarray(wr, dtype=np.float64).reshape(-1, nv)
    return O.ref_run(["riemann", fluid, solver, wl.shape[0], ivx, float(gamma), float(c_h)], wl, wr).reshape(-1, nv)


def ref_c2p(fluid, u, gamma, nscalars, pfloor=-1.0, dfloor=-1.0, efloor=-1.0, vceil=float("inf"), eceil=float("inf")):
    u = np.ascontiguousarray(u, dtype=np.float64)
    n, nv = u.shape
    out = O.ref_run(["c2p", fluid, n, float(gamma), float(pfloor), float(dfloor), float(efloor), float(vceil), float(eceil),
                     nscalars], u).reshape(2, n, nv)
    return out[0], out[1]


def ref_pencil(fluid, recon, solver, d, w, gamma, c_h, dx):
    """face fluxes [ncell][nv] of the x1 pencil w run along direction d, brought back to the x1 case"""
    n, nv = w.shape
    f = O.ref_run(["pencil", fluid, recon, solver, d, n, float(gamma), float(c_h), float(dx)], rotate(w, d)).reshape(n, nv)
    return unrotate(f, d)
