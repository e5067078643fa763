"""What tests/golden/make_reference_physics.py and tests/test_reference_physics.py share: the deck entries of every case
(lists of "block/key=value", handed both to oracle/_ref/ref_physics and, as overrides, to the host's deck parser), the
input families (crafted edges + seeded random), and thin wrappers that pipe them through the reference binary.

Inputs are chosen with plain float arithmetic; nothing here is an expected value.  Where an input family needs a scale
of the model (r_nfw_s, mbar (gamma - 1) / k_B) it is only to aim the inputs at the interesting places."""
import math
import os

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHURE_REL = os.path.join("tests", "golden", "schure.cooling_1.0Z")
SCHURE = os.path.join(ROOT, SCHURE_REL)
EPS = np.finfo(np.float64).eps
LD = np.longdouble
GAMMA_TEXT = "1.6666666666666667"
GAMMA = float(GAMMA_TEXT)

# ---- unit systems ----------------------------------------------------------------------------------------------------
UNITS = {
    "cgs": [],
    "hse": ["units/code_length_cgs=3.0856775809623245e+24", "units/code_mass_cgs=1.98841586e+47", "units/code_time_cgs=3.15576e+16"],
    "odd": ["units/code_length_cgs=3.0856775809623245e+21", "units/code_mass_cgs=1.98841586e+43", "units/code_time_cgs=7.3e+13"],
}
HSE = UNITS["hse"]


def ref(args, *arrays, text=False):
    return O.ref_run(args, *arrays, which="ref_physics", text=text)


def ref_units(keys):
    out = {}
    for line in ref(["units"] + list(keys), text=True).splitlines():
        name, value = line.split()
        out[name] = float(value)
    return out


# ---- gravity ---------------------------------------------------------------------------------------------------------
G = "problem/cluster/gravity/"
GRAVITY_SET = ["problem/cluster/hubble_parameter=0.0715898515654728", G + "m_nfw_200=10.0", G + "c_nfw=6.0", G + "m_bcg_s=0.001",
               G + "r_bcg_s=0.004", G + "m_smbh=1e-06"]
GRAVITY_KEYS = ("hubble_parameter", "m_nfw_200", "c_nfw", "m_bcg_s", "r_bcg_s", "m_smbh", "g_smoothing_radius")


def components(nfw, bcg, smbh):
    return [G + "include_nfw_g=%s" % ("true" if nfw else "false"), G + "which_bcg_g=%s" % bcg,
            G + "include_smbh_g=%s" % ("true" if smbh else "false")]


SMOOTH = [G + "g_smoothing_radius=1e-6"]
# name -> (deck entries, smoothing radius, approximate r_nfw_s the radii are aimed with)
GRAVITY_DECKS = {
    "nfw": (HSE + components(True, "NONE", False) + GRAVITY_SET + SMOOTH, 1e-6, 0.39),
    "bcg": (HSE + components(False, "HERNQUIST", False) + GRAVITY_SET + SMOOTH, 1e-6, 0.39),
    "smbh": (HSE + components(False, "NONE", True) + GRAVITY_SET + SMOOTH, 1e-6, 0.39),
    "all": (HSE + components(True, "HERNQUIST", True) + GRAVITY_SET + SMOOTH, 1e-6, 0.39),
    "all_unsmoothed": (HSE + components(True, "HERNQUIST", True) + GRAVITY_SET + [G + "g_smoothing_radius=0.0"], 0.0, 0.39),
    "defaults_hse": (HSE + components(True, "HERNQUIST", True), 0.0, 0.43),
    "defaults_cgs": (components(True, "HERNQUIST", True), 0.0, 1.3e24),
}
GRAVITY_RANDOM = {"nfw": 128, "bcg": 32, "smbh": 32, "all": 128, "all_unsmoothed": 64, "defaults_hse": 64, "defaults_cgs": 64}


def gravity_radii(name, rng, n):
    """crafted: r / r_nfw_s from 1e-12 to 1e3 (the cancellation of log(1 + x) - x / (1 + x)), and radii below, at and just
    above the smoothing radius; then n random ones, log-uniform over 1e-9 .. 30 r_nfw_s"""
    _, smoothing, r_s = GRAVITY_DECKS[name]
    r = list(r_s * 10.0 ** np.linspace(-12, 3, 61))
    if smoothing > 0:
        r += [0.25 * smoothing, 0.5 * smoothing, np.nextafter(smoothing, 0.0), smoothing, np.nextafter(smoothing, 1.0), 2 * smoothing]
    return np.concatenate([np.array(r), r_s * 10.0 ** rng.uniform(-9, 1.5, n)])


def ref_gravity(name_or_keys, r):
    keys = GRAVITY_DECKS[name_or_keys][0] if isinstance(name_or_keys, str) else name_or_keys
    return ref(["gravity", len(r)] + list(keys), r)


# equidistant radial meshes the host's he_sphere_profile can be asked for (its g and K columns are the host model's
# g_from_r and K_from_r): (r_start, r_end, n_r, r_fix); the first straddles the smoothing radius
HOST_MESHES = [(2.5e-7, 2.5e-5, 200, 1e-5), (1e-3, 4.0, 300, 2.0)]
HOST_DECKS = ("nfw", "bcg", "smbh", "all", "all_unsmoothed", "defaults_hse")


def host_mesh_radii(mesh):
    r_start, r_end, n_r, _ = mesh
    dr = (np.float64(r_end) - np.float64(r_start)) / (n_r - 1.0)
    return np.float64(r_start) + np.arange(n_r, dtype=np.float64) * dr


# ---- entropy ---------------------------------------------------------------------------------------------------------
E = "problem/cluster/entropy_profile/"
ENTROPY_DECKS = {
    "deck": (HSE + [E + "k_0=8.851356669953344e-121", E + "k_100=1.3277035004930017e-119", E + "r_k=0.1", E + "alpha_k=1.1"], 0.1),
    "defaults_hse": (HSE, 0.1),
    "defaults_cgs": ([], 3.0856775809623245e+23),
}
ENTROPY_RANDOM = {"deck": 256, "defaults_hse": 128, "defaults_cgs": 128}


def entropy_radii(name, rng, n):
    r_k = ENTROPY_DECKS[name][1]
    return np.concatenate([r_k * 10.0 ** np.linspace(-6, 3, 37), r_k * 10.0 ** rng.uniform(-6, 3, n)])


def ref_entropy(name_or_keys, r):
    keys = ENTROPY_DECKS[name_or_keys][0] if isinstance(name_or_keys, str) else name_or_keys
    return ref(["entropy", len(r)] + list(keys), r)


# ---- jet -------------------------------------------------------------------------------------------------------------
# (theta, phi0, phi_dot, time)
JET_CASES = {"aligned": (0.0, 0.0, 0.0, 0.0), "tilted": (0.2, 0.3, 0.7, 1.3), "tilted_static": (1.1, -2.0, 0.0, 5.0)}
JET_RANDOM = {"aligned": 128, "tilted": 256, "tilted_static": 128}


def jet_inputs(name, rng, n):
    """points [m][3] and vectors (cos, sin, v_r, v_theta, v_h) [m][5]: on the axis (r_jet == 0 where the axis is aligned),
    x_jet == 0 or y_jet == 0, negative h; then n random ones"""
    p = [(0.0, 0.0, 0.5), (0.0, 0.0, -0.5), (0.0, 0.0, 0.0), (0.0, 0.3, 0.2), (0.0, -0.3, -0.2), (0.4, 0.0, 0.1), (-0.4, 0.0, -0.1),
         (0.1, 0.2, -0.3), (1e-160, 0.0, 1.0), (3e-170, -4e-170, -1.0)]
    p = np.concatenate([np.array(p), rng.uniform(-1, 1, (n, 3))])
    m = p.shape[0]
    ang = rng.uniform(-np.pi, np.pi, m)
    v = np.column_stack([np.cos(ang), np.sin(ang), rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)])
    v[0, :2] = 0.0                      # what the transforms hand on at r_jet == 0
    v[1] = (1.0, 0.0, 0.0, 0.0, 1.0)    # a pure axial vector
    v[2] = (0.0, 1.0, 1.0, 0.0, 0.0)    # a pure radial one
    return p, v


def ref_jet(case, p, v):
    theta, phi0, phidot, time = case
    out = ref(["jet", float(theta), float(phi0), float(phidot), float(time), len(p)], p, v)
    n = len(p)
    return out[:4 * n].reshape(n, 4), out[4 * n:].reshape(n, 3)


# ---- tower -----------------------------------------------------------------------------------------------------------
T = "problem/cluster/magnetic_tower/"
TOWER_OFFSET, TOWER_THICKNESS = 0.0078125, 0.015625       # 2^-7, 2^-6: |h| == offset + thickness is exact
TOWER_DECKS = {
    "li": [T + "potential_type=li", T + "li_alpha=20", T + "l_scale=0.01", T + "l_mass_scale=0.005"],
    "donut": [T + "potential_type=donut", T + "l_scale=0.01", T + "donut_offset=%r" % TOWER_OFFSET,
              T + "donut_thickness=%r" % TOWER_THICKNESS, T + "l_mass_scale=0.005"],
}
TOWER_FIELD, TOWER_DENSITY = 0.7, 1.3
J = "problem/cluster/precessing_jet/"
TOWER_JETS = {"aligned": ([], 0.0), "tilted": ([J + "jet_theta=0.2", J + "jet_phi0=0.3", J + "jet_phi_dot=0.7"], 1.3),
              "block": ([J + "jet_theta=0.2", J + "jet_phi0=0.3"], 0.0)}     # (no precession: the host's initial field is at time 0)
TOWER_RANDOM = 128


def tower_points(jet, rng, n):
    """aligned axis (h == z exactly): |h| exactly the donut's offset, exactly offset + thickness and one ulp outside
    either, r = 0, r / l_scale up to 30 (the exponential underflows); tilted: n random points within 3 l_scale"""
    if jet != "aligned":
        return rng.uniform(-0.03, 0.03, (n, 3))
    lo, hi = TOWER_OFFSET, TOWER_OFFSET + TOWER_THICKNESS
    hs = [lo, np.nextafter(lo, 0.0), np.nextafter(lo, 1.0), hi, np.nextafter(hi, 0.0), np.nextafter(hi, 1.0), 0.0, 0.012]
    p = [(x, y, s * h) for h in hs for s in (1.0, -1.0) for (x, y) in ((0.003, -0.004), (0.0, 0.0))]
    p += [(0.01 * q, 0.0, 0.01) for q in (1.0, 5.0, 20.0, 26.0, 27.5, 30.0)]
    return np.concatenate([np.array(p), rng.uniform(-0.03, 0.03, (n, 3))])


def ref_tower(potential, jet, p, field=TOWER_FIELD, density=TOWER_DENSITY):
    keys, time = TOWER_JETS[jet]
    n = len(p)
    out = ref(["tower", float(field), float(density), float(time), n] + TOWER_DECKS[potential] + keys, p)
    return out[:3 * n].reshape(n, 3), out[3 * n:6 * n].reshape(n, 3), out[6 * n:]


# the block of the GPU tower tests: 8 x 6 x 5 interior cells of width 2^-8, the origin inside
BLOCK_NX, BLOCK_NG, BLOCK_DX = (8, 6, 5), 2, 0.00390625
BLOCK_XMIN = (-4 * BLOCK_DX, -3 * BLOCK_DX, -2.5 * BLOCK_DX)
BLOCK_MESH = ["parthenon/mesh/nx%d=%d" % (d + 1, BLOCK_NX[d]) for d in range(3)] + \
             ["parthenon/meshblock/nx%d=%d" % (d + 1, BLOCK_NX[d]) for d in range(3)] + \
             ["parthenon/mesh/x%dmin=%r" % (d + 1, BLOCK_XMIN[d]) for d in range(3)] + \
             ["parthenon/mesh/x%dmax=%r" % (d + 1, -BLOCK_XMIN[d]) for d in range(3)]


# the donut's edges: a 4 x 4 x 13 block, axis ALIGNED, whose centres along x3 are (-6 ... 6) dx: with offset = 2 dx and
# thickness = 4 dx the planes k = +-2 sit exactly on |h| == offset and k = +-6 exactly on |h| == offset + thickness
EDGE_NX = (4, 4, 13)
EDGE_XMIN = (-2 * BLOCK_DX, -2 * BLOCK_DX, -6.5 * BLOCK_DX)


def mesh_keys(nx, xmin):
    return ["parthenon/mesh/nx%d=%d" % (d + 1, nx[d]) for d in range(3)] + ["parthenon/meshblock/nx%d=%d" % (d + 1, nx[d]) for d in range(3)] + \
           ["parthenon/mesh/x%dmin=%r" % (d + 1, xmin[d]) for d in range(3)] + ["parthenon/mesh/x%dmax=%r" % (d + 1, -xmin[d]) for d in range(3)]


def block_centres(extend=0, nx=BLOCK_NX, xmin=BLOCK_XMIN):
    """the block's cell centres xmin + ((g + i) + 1/2) dx (cluster_reference.cell_centres), `extend` cells beyond both ends"""
    return [np.float64(xmin[d]) + ((np.float64(-extend) + np.arange(nx[d] + 2 * extend, dtype=np.float64)) + 0.5)
            * np.float64(BLOCK_DX) for d in range(3)]


def block_points(extend=0, nx=BLOCK_NX, xmin=BLOCK_XMIN):
    """[k][j][i][3] flattened to [m][3]"""
    x1, x2, x3 = block_centres(extend, nx, xmin)
    Z, Y, X = np.meshgrid(x3, x2, x1, indexing="ij")
    return np.stack([X, Y, Z], axis=-1).reshape(-1, 3)


# ---- cooling ---------------------------------------------------------------------------------------------------------
COOLING_DECK = HSE + ["hydro/gamma=" + GAMMA_TEXT, "hydro/He_mass_fraction=0.25", "cooling/lambda_units_cgs=1"]
HE = 0.25
RHO0 = 147.7557589278723


def read_table(path=SCHURE):
    lt, ll = [], []
    with open(path) as f:
        for line in f:
            s = line.strip()
            if s and not s.startswith("#"):
                a, b = s.split()
                lt.append(float(a))
                ll.append(float(b))
    return lt, ll


def mbar_gm1_over_kb(units):
    """mu mh / k_B (gamma - 1) in the operation order of hydro.cpp:495, :503 and tabular_cooling.hpp:124, from the
    reference's own mh and k_boltzmann (`units` is ref_units' dict)"""
    mu = 1 / (HE * 3. / 4. + (1 - HE) * 2)
    return mu * units["mh"] / units["k_boltzmann"] * (GAMMA - 1)


def _lookup_ok(lt, log_temp):
    """would DeDt's table lookup pass its REQUIRE at this log T (inside the table)?"""
    start, d = lt[0], lt[1] - lt[0]
    i = int((log_temp - start) / d)
    lti = start + d * i
    return lti <= log_temp <= lti + d


def _e_with_log_temp(c, target, span=4096):
    """an e whose log10(c e), as libm rounds it, is exactly `target` (None if no double within `span` ulps gives it)"""
    e = 10.0 ** target / c
    down = e
    for _ in range(span):
        if math.log10(c * e) == target:
            return e
        if math.log10(c * down) == target:
            return down
        e, down = np.nextafter(e, np.inf), np.nextafter(down, 0.0)
    return None


def dedt_inputs(c, rng, n, crafted=True):
    """(e, rho)[m][2], labels.  c = mbar (gamma - 1) / k_B.  Crafted: e < 0 and NaN (valid = 0), log T below the table,
    exactly on the first node, an interior node and the last node, one ulp either side of an interior node, inside the
    last interval, above the table (free-free); then n random ones with log T uniform over 3 .. 9.5.  Inputs whose
    lookup would fail the reference's REQUIRE (it aborts) are left out."""
    lt, _ = read_table()
    e, labels = [], []
    if crafted:
        e += [-1.0e-3, float("nan"), 10 ** 3.5 / c, 10 ** 4.1999 / c]
        labels += ["negative", "nan", "below", "just_below"]
        interior = None
        for k in range(40, 60):
            cand = [_e_with_log_temp(c, x) for x in (lt[k], np.nextafter(lt[k], 0.0), np.nextafter(lt[k], 10.0))]
            if all(v is not None for v in cand) and all(_lookup_ok(lt, math.log10(c * v)) for v in cand):
                interior = (k, cand)
                break
        assert interior is not None, "no interior node is reachable with its two neighbours"
        for name, x in (("first_node", lt[0]), ("last_node", lt[-1])):
            v = _e_with_log_temp(c, x)
            assert v is not None, name
            e.append(v)
            labels.append(name)
        e += interior[1]
        labels += ["node_%d" % interior[0], "node_%d_minus_ulp" % interior[0], "node_%d_plus_ulp" % interior[0]]
        e += [10 ** (lt[-1] - 0.017) / c, 10 ** (lt[-2] + 1e-9) / c, np.nextafter(e[labels.index("last_node")], np.inf) * (1 + 1e-12),
              10 ** 8.5 / c, 10 ** 9.4 / c]
        labels += ["last_interval", "last_interval_start", "just_above", "above", "far_above"]
    e += list(10 ** rng.uniform(3.0, 9.5, n) / c)
    labels += ["random"] * n
    keep = []
    for v in e:
        x = math.log10(c * v) if v > 0 else None
        keep.append(x is None or x < lt[0] or x > lt[-1] or x == lt[-1] or _lookup_ok(lt, x))
    e = np.array(e)[keep]
    labels = [s for s, k in zip(labels, keep) if k]
    rho = RHO0 * 10 ** rng.uniform(-2, 2, len(e))
    return np.column_stack([e, rho]), labels


def ref_dedt(x, keys=COOLING_DECK, table=SCHURE):
    out = ref(["dedt", table, len(x)] + list(keys), x)
    return out[:len(x)], out[len(x):] != 0.0


def rk_inputs(c, dedt_of, rng, n):
    """(e0, rho, h)[m][3] and (h, err, tol)[m][3].  h = f e0 / |de/dt(e0)| (dedt_of: a callable (e, rho)[m][2] -> de/dt[m] used
    only to size the steps): f = 1e-3 stays inside one interval, 0.05 .. 0.5 crosses nodes, starts just above the lowest
    node and just above the highest leave the table at either end, f >= 1.2 drives y negative (valid cleared by the
    second evaluation)"""
    lt, _ = read_table()
    rows = []
    for log_t, f in ((5.013, 1e-3), (6.01, 1e-3), (5.03, 0.05), (6.5, 0.3), (7.1, 0.5), (lt[0] + 0.003, 0.2), (lt[0] + 0.03, 0.4),
                     (lt[-1] + 0.002, 0.1), (lt[-1] + 0.3, 0.5), (8.9, 0.02), (5.5, 1.2), (6.2, 1.5), (4.5, 3.0), (8.6, 2.0)):
        rows.append((10 ** log_t / c, RHO0, f))
    for _ in range(n):
        f = 10 ** rng.uniform(-3, 0.3) if rng.uniform() < 0.85 else rng.uniform(1.05, 3.0)
        rows.append((10 ** rng.uniform(4.25, 9.0) / c, RHO0 * 10 ** rng.uniform(-2, 2), f))
    x = np.array(rows)
    rate = np.abs(dedt_of(x[:, :2]))
    x[:, 2] = x[:, 2] * x[:, 0] / rate
    m = len(x)
    opt = np.column_stack([10 ** rng.uniform(-6, 0, m), 10 ** rng.uniform(-12, -2, m), 10 ** rng.uniform(-10, -4, m)])
    opt[0] = (0.5, 1e-8, 1e-8)          # tol == err
    # ratios whose square libm's pow does not round correctly (about one in a thousand): pow(r, 2) against r * r
    k = 1
    while k < 5:
        err, tol = 10 ** rng.uniform(-12, -2), 10 ** rng.uniform(-10, -4)
        if math.pow(tol / err, 2) != (tol / err) * (tol / err):
            opt[k] = (0.25 * k, err, tol)
            k += 1
    return x, opt


def ref_rkstep(stepper, x, opt, keys=COOLING_DECK, table=SCHURE):
    n = len(x)
    out = ref(["rkstep", stepper, table, n] + list(keys), x, opt)
    return out[:n], out[n:2 * n], out[2 * n:3 * n] != 0.0, out[3 * n:]


def ref_keep(run, *arrays):
    """a boolean mask of the rows on which `run(rows...)` (a ref_* call) does not abort: the whole set if it passes, else
    halves, down to single rows.  The reference's REQUIRE in the table lookup aborts the process, so such a row cannot be
    stored or compared."""
    n = len(arrays[0])
    keep = np.ones(n, dtype=bool)

    def go(lo, hi):
        try:
            run(*[a[lo:hi] for a in arrays])
        except RuntimeError:
            if hi - lo == 1:
                keep[lo] = False
            else:
                mid = (lo + hi) // 2
                go(lo, mid)
                go(mid, hi)

    go(0, n)
    return keep


# ---- limiters --------------------------------------------------------------------------------------------------------
def limiter_inputs(rng, n):
    """all sign patterns of (A, B, C, D) over {-1.5, 0, 0.75}, equal arguments, and tiny same-sign pairs whose product
    underflows to 0; then n random quadruples"""
    vals = (-1.5, 0.0, 0.75)
    q = [(a, b, c, d) for a in vals for b in vals for c in vals for d in vals]
    q += [(0.3, 0.3, 0.3, 0.3), (-2.0, -2.0, 1.0, 1.0), (1e-200, 3e-200, 2e-200, 1e-200), (-1e-200, -3e-200, -2e-170, -1e-170),
          (1e-160, 1e-160, 5.0, 7.0), (4.0, 1.0, 1.0, 4.0), (1.0, 4.0, -1.0, -4.0), (1.0, 3.0, 1.0, 3.0), (3.0, 1.0, 10.0, 0.1)]
    r = rng.uniform(-1, 1, (n, 4)) * 10.0 ** rng.uniform(-3, 3, (n, 4))
    return np.concatenate([np.array(q), r])


def ref_limiters(q):
    return ref(["limiters", len(q)], q).reshape(5, len(q))


# ---- add-density helpers ---------------------------------------------------------------------------------------------
DELTAS = (0.25, -0.25, 0.0, 0.0123, 0.37, -0.11, 1.7, -0.003)


def adddensity_inputs(rng, n):
    """(delta, cons[5], prim[5]) rows: positive and negative delta, zero velocity; then n random rows.  delta takes one of
    the eight values of DELTAS, so that the rows of one value can go through a source term that adds one density to all
    its cells"""
    m = n + 6
    w = np.column_stack([rng.uniform(0.5, 2.0, m), rng.uniform(-1, 1, (m, 3)), rng.uniform(0.1, 2.0, m)])
    w[0, 1:4] = 0.0
    w[1, 1:4] = 0.0
    w[2, 2:4] = 0.0
    u = np.column_stack([w[:, 0], w[:, 0:1] * w[:, 1:4], w[:, 4] / (GAMMA - 1) + 0.5 * w[:, 0] * (w[:, 1:4] ** 2).sum(axis=1)])
    delta = np.array(DELTAS)[rng.integers(0, len(DELTAS), m)]
    delta[0], delta[1], delta[3] = 0.25, -0.25, 0.0
    return np.column_stack([delta, u, w])


def ref_adddensity(kind, rows, gamma=GAMMA):
    return ref(["adddensity", kind, float(gamma), len(rows)], rows).reshape(len(rows), 5)


# ---- scales S_i of the tolerance rule: the sum of the absolute values of the addends of the reference's final
# ---- expression before cancellation, in numpy.longdouble from the stored inputs ------------------------------------------------
def gravity_scale(c, r_in):
    """c: the host's lib.ClusterGravity constants (or any object with its fields)"""
    r = np.maximum(np.asarray(r_in, dtype=LD), LD(c.smoothing_r))
    s = np.zeros_like(r)
    if c.include_nfw:
        x = r / LD(c.r_nfw_s)
        s = s + LD(c.g_const_nfw) / (r * r) * (np.abs(np.log1p(x)) + np.abs(x / (1 + x)))
    if c.which_bcg:
        s = s + LD(c.g_const_bcg) / ((1 + r / LD(c.r_bcg_s)) ** 2)
    if c.include_smbh:
        s = s + LD(c.g_const_smbh) / (r * r)
    return s.astype(np.float64)


# ---- the states and blocks of the GPU tests ------------------------------------------------------------------------------------------
def dyadic_state(rng, shape, mhd=False):
    """(cons, prim) [5 or 9][k][j][i] whose every number but the pressure is a small dyadic rational: rho in {1/2, 1, 2},
    v and B multiples of 1/8, E - e_k - e_B a multiple of 1/8 in [1, 3], psi = 0.  ConsToPrim of such a state rounds once
    (p = (gamma - 1) (E - e_k - e_B)) whatever the build contracts, so the primitives the device derives are these bits"""
    n = 9 if mhd else 5
    u, w = np.zeros((n,) + tuple(shape)), np.zeros((n,) + tuple(shape))
    w[0] = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, shape)]
    w[1:4] = rng.integers(-8, 9, (3,) + tuple(shape)) / 8.0
    e_int = rng.integers(8, 25, shape) / 8.0
    u[0] = w[0]
    u[1:4] = w[0] * w[1:4]
    u[4] = e_int + 0.5 * w[0] * (w[1] * w[1] + w[2] * w[2] + w[3] * w[3])
    if mhd:
        w[5:8] = u[5:8] = rng.integers(-2, 3, (3,) + tuple(shape)) / 8.0
        u[4] += 0.5 * (u[5] * u[5] + u[6] * u[6] + u[7] * u[7])
    w[4] = (GAMMA - 1.0) * e_int
    return u, w


def rows_of(delta, u, w):
    """(delta, cons[5], prim[5]) rows of the cells of [nvar][...] arrays, in array order"""
    m = u[0].size
    d = np.broadcast_to(np.asarray(delta, dtype=np.float64), u[0].shape).reshape(m)
    return np.column_stack([d, u[:5].reshape(5, m).T, w[:5].reshape(5, m).T])


# AGN feedback on the 8 x 6 x 5 block, axis aligned: the centres along x3 are (-2, -1, 0, 1, 2) dx, so that with
# offset = thickness = dx cells sit exactly on |h| == offset and on |h| == offset + thickness.  The thermal radius 1.9 dx
# lies between the centres' radii (r^2 / dx^2 = 3.5 and 4.5): no cell is within rounding of the sphere's edge
AGN_SEED, AGN_DELTA = 811, 0.37
AGN_CFG = dict(thermal_feedback=0.0, thermal_density=AGN_DELTA, thermal_radius=1.9 * BLOCK_DX, jet_density=0.0625, jet_momentum=0.125,
               jet_feedback=0.03125, kinetic_jet_radius=1.6 * BLOCK_DX, kinetic_jet_thickness=BLOCK_DX, kinetic_jet_offset=BLOCK_DX,
               vceil=float("inf"), eceil=float("inf"))


def agn_block_state():
    """(cons, prim) [5][k][j][i] with ghost cells of the feedback test's block"""
    shape = tuple(BLOCK_NX[d] + 2 * BLOCK_NG for d in (2, 1, 0))
    return dyadic_state(np.random.default_rng(AGN_SEED), shape)


def interior(a, nx=BLOCK_NX, ng=BLOCK_NG):
    return a[..., ng:ng + nx[2], ng:ng + nx[1], ng:ng + nx[0]]


# gravity source: two blocks of 7 x 5 x 5 cells side by side along x1, the first centred on the origin (its cell (3, 2, 2)
# has r == 0), cell width 2^-7 (Mpc), no smoothing
GRAV_NX, GRAV_NG, GRAV_DX, GRAV_DECK, GRAV_SEED, GRAV_BETA_DT = (7, 5, 5), 2, 0.0078125, "all_unsmoothed", 812, 0.0009765625
GRAV_XMIN = (-3.5 * GRAV_DX, -2.5 * GRAV_DX, -2.5 * GRAV_DX)


def grav_centres(b):
    """cell centres of block b (0, 1) of the gravity test: xmin + ((g + i) + 1/2) dx with g = 7 b along x1"""
    return [np.float64(GRAV_XMIN[d]) + ((np.float64(7 * b if d == 0 else 0) + np.arange(GRAV_NX[d], dtype=np.float64)) + 0.5)
            * np.float64(GRAV_DX) for d in range(3)]


def grav_radii():
    """[2][k][j][i]: sqrt(x x + y y + z z) of the interior centres, the sum in the kernel's order"""
    out = []
    for b in (0, 1):
        x, y, z = grav_centres(b)
        X, Y, Z = x[None, None, :], y[None, :, None], z[:, None, None]
        out.append(np.sqrt(X * X + Y * Y + Z * Z))
    return np.array(out)


def grav_state():
    """(cons, prim) [2][5][k][j][i] with ghost cells"""
    rng = np.random.default_rng(GRAV_SEED)
    shape = tuple(GRAV_NX[d] + 2 * GRAV_NG for d in (2, 1, 0))
    s = [dyadic_state(rng, shape) for _ in (0, 1)]
    return np.array([a for a, _ in s]), np.array([b for _, b in s])


# triggering: one block of 8^3 cells on [-1/2, 1/2]^3; accretion_radius = 0.32 reaches the centres with |x| <= 0.1875 in
# every direction but the eight corners of that 4 x 4 x 4 box; everything is cold; dt and cold_t_acc are powers of two, so
# that the removed density -rho / cold_t_acc * dt is exact
TRIG_SEED, TRIG_DT, TRIG_T_ACC, TRIG_RADIUS = 813, 0.00390625, 0.25, 0.32
TRIG_MESH = ["parthenon/mesh/nx%d=8" % d for d in (1, 2, 3)] + ["parthenon/meshblock/nx%d=8" % d for d in (1, 2, 3)] + \
            ["parthenon/mesh/x%dmin=-0.5" % d for d in (1, 2, 3)] + ["parthenon/mesh/x%dmax=0.5" % d for d in (1, 2, 3)]
TRIG_BOX = (slice(4, 8),) * 3        # the 4 x 4 x 4 box in the block's arrays (ng = 2)


def trig_state():
    """(cons, prim) [5][12][12][12] with ghost cells"""
    return dyadic_state(np.random.default_rng(TRIG_SEED), (12, 12, 12))
