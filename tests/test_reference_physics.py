"""The cluster, tower and cooling arithmetic against values that the REFERENCE's own compiled headers computed.

tests/golden/reference_physics.npz (+ .json, made by tests/golden/make_reference_physics.py) stores inputs, the outputs
of oracle/_ref/ref_physics for them -- the reference's src/units.hpp, src/pgen/cluster/{cluster_gravity, entropy_profiles,
jet_coords, magnetic_tower, cluster_utils}.hpp, src/hydro/srcterms/tabular_cooling.hpp and the limiters of
src/hydro/diffusion/diffusion.hpp, compiled unmodified against the stand-in names of oracle/ref/standin -- and the deck
entries each case ran with, so that the reference's own constructors, defaults and key names produced them.

  CPU stored : the host models (through HostPlan's accessors) and the numpy restatements the other tests use as their
               yardstick, against the stored values (needs neither the binary nor the tree)
  CPU live   : where oracle/_ref/ref_physics exists, 20 000 fresh inputs per subcommand through the same comparisons
  GPU stored : the kernels, both builds
  GPU live   : 4096 fresh radii and (e, rho) points with expected values from the binary, if it travelled with the tree

NOT pinned: ClusterGravity::rho_from_r.  It reads rho_const_nfw_ and rho_const_bcg_, which the reference's constructor
never initialises (README, the SNIa paragraph); the binary does not offer it.  vanleer is stored, but the project has no
van Leer limiter to hold against it.

Tolerances.  A path with no transcendental call and no declared deviation is held to every bit in the strict build, in
the host models and in the restatements: the limiters, the add-density helpers, the jet transforms given the axis's sines
and cosines, the masks.  Product-build comparisons of such paths use the project's 1e-12 x scale rule per case
(test_reference_vectors.PRODUCT_TOL).  The host models call the same libm as the reference binary in the reference's
operation order, so they too are held to every bit, transcendentals included; OBSERVED: this holds on all stored inputs,
also where the README declares a deviation (x * x for pow(x, 2) in the jet frame and the tower: glibc's pow returns the
correctly rounded square on every stored input).  cooling_reference.py computes with `math`, the same libm: every bit.

Where another library's transcendental is on the path (numpy's, the device's) case i is bounded by K x eps x S_i, S_i the
sum of the absolute values of the addends of the reference's final expression before cancellation, in numpy.longdouble
from the stored inputs.  The budget per transcendental call is 2 ulp per side (the ROCm device library's accuracy table
is not installed with the toolkit here, so the fallback of 2 ulp is used, for numpy as well); every IEEE operation that
follows a changed operand adds one.
  g_from_r   K = 8: log 2 + 2; then L - q, the product with g_const_nfw, the quotient by r^2, the sum of the components.
             S_i = g_nfw / r^2 (|log(1 + x)| + |x / (1 + x)|) + g_bcg / (1 + r / r_bcg)^2 + g_smbh / r^2
  K_from_r   K = 6: pow 2 + 2, the product with k_100, the sum.  S_i = |k_0| + |k_100 (r / r_k)^alpha_k|
  tower A, B K = 11: exp 2 + 2; one product onto a_theta / a_h (b_r, b_theta, b_h): 5; a product and a difference into
             v_x_jet / v_y_jet: 7; two more products in a component's longest addend: 9; the component's two sums: 11.
             S_i = per component, the sum of the absolute values of the addends of JetCylToSimCartVector, with
             |v_x_jet| <= |v_r cos| + |v_theta sin| expanded likewise and b_h's 1 - (r / l)^2 as 1 + (r / l)^2
  density    K = 5: exp 2 + 2, one product.  S_i = |density exp(..)|
  DeDt (device): the rate is -10^(log lambda) x_H^2 rho; pow 2 + 2 and two products: 6 eps, plus ln 10 times what log
             lambda itself may differ by: the device's log10 against glibc's (2 + 2 ulp of a log T below 16: 32 eps) times
             the slope of the table's interval or its neighbours', one ulp of log lambda for the interpolation's final
             sum, and one extra ulp of log10 lambda for the table-cell decision when log T lands within an ulp of a node
             -- log10 is not correctly rounded on either side, so a table lookup may land one ulp apart
             (test_gpu_cooling._loglam_tol).  bound_i = eps |de/dt| (6 + ln 10 (32 slope_i + 2 ulp(log lambda) / eps)).
             OBSERVED on an MI355X: the strict build's DeDt equals the reference in every bit on all stored and 4096
             live points, the product build within 4e-16 |de/dt|
Measured max |got - ref| / (eps S_i): restated g 0.49, device g 0.52 (K = 8); restated K 1.36 (K = 6); restated tower A / B
1.31 / 1.48 (K = 11), density 1.45 (K = 5); device tower B 0.29 and density 0.20 of their bounds.  The two logs stay so far
inside the 2 ulp the count may assume that g fills less than a tenth of its bound; the count cannot go lower without
assuming more about the libraries than is documented.
"""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as CR  # noqa: E402
import cluster_sources_reference as CS  # noqa: E402
import cooling_reference as CO  # noqa: E402
import diffusion_reference as DR  # noqa: E402
import feedback_reference as FB  # noqa: E402
import reference_physics_cases as P  # noqa: E402
import spitzer_reference as SR  # noqa: E402
import triggering_reference as TR  # noqa: E402
from oracle import oracle as O  # noqa: E402

GDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
PRODUCT_TOL = 1e-12
N_LIVE, N_LIVE_GPU = 20000, 4096
K_G, K_K, K_TOWER, K_DENSITY = 8, 6, 11, 5
MEASURED = {}


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(GDIR, "reference_physics.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GDIR, "reference_physics.json")) as f:
        return json.load(f)


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.argwhere((got != want) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError("%s: %d entries differ bitwise, first at %s: %r vs %r" % (
            what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _within(got, want, K, scale, what):
    """|got - want| <= K eps scale per entry; prints and records the measured maximum of |got - want| / (eps scale)"""
    got, want, scale = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), what + ": non-finite entries differ"
    err = np.abs(got - want)
    pos = scale > 0
    assert np.all(err[~pos] == 0.0), "%s: %d entries of scale 0 differ" % (what, int((err[~pos] != 0).sum()))
    worst = float(np.max(err[pos] / (EPS * scale[pos]), initial=0.0))
    MEASURED[what] = max(MEASURED.get(what, 0.0), worst)
    print("MEASURED %s: max |got - ref| / (eps S) = %.3f of K = %g" % (what, worst, K))
    assert worst <= K, "%s: %.3f eps S exceeds K = %g" % (what, worst, K)


def _product(got, want, scale, what):
    """the product build's rule: |got - want| <= 1e-12 scale per entry"""
    got, want, scale = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), what + ": non-finite entries differ"
    err = np.abs(got - want)
    pos = scale > 0
    assert np.all(err[~pos] == 0.0), "%s: %d entries of scale 0 differ" % (what, int((err[~pos] != 0).sum()))
    worst = float(np.max(err[pos] / scale[pos], initial=0.0))
    print("MEASURED product build, %s: worst err / scale %.3e" % (what, worst))
    assert worst <= PRODUCT_TOL, "%s: %.3e exceeds 1e-12 x scale" % (what, worst)


# ---- the host side: HostPlan of a deck with the case's entries as overrides ----------------------------------------------------
def _strip(deck, keys):
    """the deck without the lines that set `keys` (so that their defaults act)"""
    return "\n".join(line for line in deck.split("\n") if line.split("=")[0].strip() not in keys or "=" not in line)


def _plan(name, keys, strip=()):
    from athenapk_amd import decks, driver
    return driver.HostPlan(_strip(decks.load(name), strip), list(keys))


def _gravity_plan(m, extra=()):
    keys = list(m["keys"]) + list(extra)
    set_keys = {k.split("=")[0].split("/")[-1] for k in keys}
    return _plan("cluster_hse", keys, [k for k in P.GRAVITY_KEYS if k not in set_keys])


UNIT_FIELDS = {"cluster_options": ("gravitational_constant", "msun", "kpc", "mpc", "km_s", "kev", "mh", "k_boltzmann"),
               "units": ("mh", "k_boltzmann", "atomic_mass_unit", "erg", "cm", "s"), "agn_feedback_options": ("speed_of_light",)}


# ---- CPU, stored ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", sorted(P.UNITS))
def test_host_units_equal_the_references(meta, system):
    """every constant of src/units.hpp that the host derives (the three accessors' fields), in three unit systems: bit for
    bit.  The reference's other accessors (gauss, dyne_cm2, ...) are stored; the project derives none of them."""
    m = meta["units"][system]
    keys = m["keys"] or ["units/code_length_cgs=1", "units/code_mass_cgs=1", "units/code_time_cgs=1"]
    p = _plan("cluster_agn_feedback", keys)
    n = 0
    for accessor, fields in UNIT_FIELDS.items():
        o = getattr(p, accessor)()
        for f in fields:
            assert getattr(o, f) == m["values"][f], (system, accessor, f, getattr(o, f), m["values"][f])
            n += 1
    assert n == 15
    o = p.units()
    assert (o.code_length_cgs, o.code_mass_cgs, o.code_time_cgs) == tuple(m["values"]["code_%s_cgs" % q] for q in ("length", "mass", "time"))


@pytest.mark.parametrize("system", sorted(P.UNITS))
def test_restated_units_equal_the_references(meta, system):
    """cluster_reference.Units and cooling_reference.Units: products and quotients, bit for bit; the gravitational
    constant goes through numpy's power: 2 + 2 ulp for each of its two calls and three roundings"""
    v = meta["units"][system]["values"]
    u = CR.Units(v["code_length_cgs"], v["code_mass_cgs"], v["code_time_cgs"])
    for f in ("k_boltzmann", "kev", "g", "cm", "km_s", "kpc", "mpc", "msun", "mh"):
        assert getattr(u, f)() == v[f], (f, getattr(u, f)(), v[f])
    _within(u.gravitational_constant(), v["gravitational_constant"], 11, abs(v["gravitational_constant"]), "restated G " + system)
    c = CO.Units(v["code_length_cgs"], v["code_mass_cgs"], v["code_time_cgs"])
    for f in ("mh", "k_boltzmann", "atomic_mass_unit", "erg", "cm", "s"):
        assert getattr(c, f) == v[f], (f, getattr(c, f), v[f])
    want = v["erg"] * math.pow(v["cm"], 3) / v["s"]
    assert c.lambda_units(1.0) == 1.0 / want


@pytest.mark.parametrize("deck", P.HOST_DECKS)
def test_host_gravity_and_entropy_equal_the_references_on_profile_meshes(ref, meta, deck):
    """the g and K columns of he_sphere_profile are the host model's g_from_r and K_from_r at r_start + i dr: every bit, on
    a mesh that straddles the smoothing radius and on a wide one; each component alone, all, smoothed and not, keys set
    and keys at their defaults (which also pins the constructor's constants: r_nfw_s, g_const_nfw, g_const_bcg,
    g_const_smbh enter every value)"""
    m = meta["gravity"][deck]
    entropy = "defaults_hse" if deck == "defaults_hse" else "deck"
    strip_entropy = ("k_0", "k_100", "r_k", "alpha_k") if deck == "defaults_hse" else ()
    for n, (r_start, r_end, n_r, r_fix) in enumerate(meta["host_meshes"]):
        keys = list(m["keys"]) + ["problem/cluster/hydrostatic_equilibrium/r_fix=%r" % r_fix]
        set_keys = {k.split("=")[0].split("/")[-1] for k in keys}
        from athenapk_amd import decks, driver
        p = driver.HostPlan(_strip(decks.load("cluster_hse"), [k for k in P.GRAVITY_KEYS if k not in set_keys] + list(strip_entropy)), keys)
        got = p.he_sphere_profile(r_start, r_end, n_r)
        _bits(got["r"], P.host_mesh_radii((r_start, r_end, n_r, r_fix)), "%s mesh %d r" % (deck, n))
        _bits(got["g"], ref["gravity_host_%s_%d_g" % (deck, n)], "%s mesh %d g" % (deck, n))
        _bits(got["K"], ref["entropy_host_%s_%d_K" % (entropy, n)], "%s mesh %d K" % (deck, n))


def _host_constants(m, extra=()):
    return _gravity_plan(m, extra).cluster_options().gravity


def _restated_gravity(c):
    """cluster_reference.Gravity with the host's constants (held to the reference above; the restatement's own come from
    numpy's log and power and are compared with the host's in test_cluster_host.py)"""
    g = CR.Gravity.__new__(CR.Gravity)
    g.include_nfw, g.which_bcg, g.include_smbh = bool(c.include_nfw), "HERNQUIST" if c.which_bcg else "NONE", bool(c.include_smbh)
    g.r_nfw_s, g.g_const_nfw, g.r_bcg_s = np.float64(c.r_nfw_s), np.float64(c.g_const_nfw), np.float64(c.r_bcg_s)
    g.g_const_bcg, g.g_const_smbh, g.smoothing_r = np.float64(c.g_const_bcg), np.float64(c.g_const_smbh), np.float64(c.smoothing_r)
    return g


@pytest.mark.parametrize("deck", sorted(P.GRAVITY_DECKS))
def test_restated_gravity_within_the_counted_bound(ref, meta, deck):
    m = meta["gravity"][deck]
    if deck == "defaults_cgs":
        from athenapk_amd import decks, driver
        keys = ["units/code_length_cgs=1", "units/code_mass_cgs=1", "units/code_time_cgs=1"] + m["keys"]
        c = driver.HostPlan(_strip(decks.load("cluster_hse"), list(P.GRAVITY_KEYS) + ["r_fix", "rho_fix"]), keys).cluster_options().gravity
    else:
        c = _host_constants(m)
    r, want = ref["gravity_%s_r" % deck], ref["gravity_%s_g" % deck]
    got = _restated_gravity(c).g_from_r(r)
    if not c.include_nfw:
        _bits(got, want, "restated g " + deck)
    else:
        _within(got, want, K_G, P.gravity_scale(c, r), "restated g " + deck)


@pytest.mark.parametrize("deck", sorted(P.ENTROPY_DECKS))
def test_restated_entropy_within_the_counted_bound(ref, meta, deck):
    v = meta["units"]["cgs" if deck == "defaults_cgs" else "hse"]["values"]
    if deck == "deck":
        q = {k.split("=")[0].split("/")[-1]: float(k.split("=")[1]) for k in meta["entropy"][deck]["keys"] if "entropy_profile" in k}
    else:
        q = {"k_0": 20 * v["kev"] * v["cm"] * v["cm"], "k_100": 120 * v["kev"] * v["cm"] * v["cm"], "r_k": 100 * v["kpc"], "alpha_k": 1.75}
    s = CR.Sphere(None, q["k_0"], q["k_100"], q["r_k"], q["alpha_k"], 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    r, want = ref["entropy_%s_r" % deck], ref["entropy_%s_K" % deck]
    scale = (LD(q["k_0"]) + LD(q["k_100"]) * (r.astype(LD) / LD(q["r_k"])) ** LD(q["alpha_k"])).astype(np.float64)
    _within(s.K_from_r(r), want, K_K, scale, "restated K " + deck)


# ---- the jet frame ---------------------------------------------------------------------------------------------------------------
def _host_jet(m):
    """lib.JetCoords the host hands the kernels for a stage at the case's time"""
    keys = [P.J + "jet_theta=%r" % m["theta"], P.J + "jet_phi0=%r" % m["phi0"], P.J + "jet_phi_dot=%r" % m["phi_dot"]]
    return _plan("cluster_agn_feedback", keys).agn_feedback_stage_numbers(1e-3, m["time"])[1]


def _check_jet(jc, p, v, cyl, sim, what):
    got = np.column_stack(FB.sim_cart_to_jet_cyl(jc, p[:, 0], p[:, 1], p[:, 2]))
    _bits(got, cyl, what + " SimCartToJetCylCoords")
    _bits(np.column_stack(FB.jet_cyl_to_sim_cart_vector(jc, *v.T)), sim, what + " JetCylToSimCartVector")


@pytest.mark.parametrize("case", sorted(P.JET_CASES))
def test_host_jet_frame_and_restated_transforms_equal_the_references(ref, meta, case):
    """The host's cos and sin of the axis angles at the case's time (phi = phi0 + time phi_dot) are not observable in the
    reference (private members), their effect is: feedback_reference's two transforms -- IEEE products, sums, one sqrt and
    two quotients, x * x where the reference writes pow(fabs(x), 2) -- with the HOST's four numbers reproduce every stored
    r, cos_theta, sin_theta, h and every stored sim-Cartesian vector bit for bit, on the axis (both ?: branches), with
    x_jet == 0, y_jet == 0 and h < 0 included.  The restatement's own four numbers (math.cos, math.sin: the same libm)
    equal the host's.  OBSERVED: the product for pow(.., 2) is bit for bit on all stored inputs."""
    m = meta["jet"][case]
    jet = _host_jet(m)
    jc = FB.jet_coords(m["theta"], m["phi_dot"], m["phi0"], m["time"])
    for f in ("cos_theta", "sin_theta", "cos_phi", "sin_phi"):
        assert getattr(jet, f) == getattr(jc, f), (case, f)
    p, cyl = ref["jet_%s_p" % case], ref["jet_%s_cyl" % case]
    _check_jet(jet, p, ref["jet_%s_v" % case], cyl, ref["jet_%s_sim" % case], case)
    if case == "aligned":
        assert np.count_nonzero(cyl[:, 0] == 0) >= 3 and np.count_nonzero(cyl[:, 3] < 0) > 10


# ---- the tower ------------------------------------------------------------------------------------------------------------------
def _tower_ns(pot):
    q = {k.split("=")[0].split("/")[-1]: k.split("=")[1] for k in P.TOWER_DECKS[pot]}
    return FB.tower(pot, float(q["l_scale"]), float(q.get("li_alpha", 0)), float(q.get("donut_offset", 0)),
                    float(q.get("donut_thickness", 0)), float(q["l_mass_scale"]))


def _tower_jc(jet):
    q = {k.split("=")[0].split("/")[-1]: float(k.split("=")[1]) for k in P.TOWER_JETS[jet][0]}
    return FB.jet_coords(q.get("jet_theta", 0.0), q.get("jet_phi_dot", 0.0), q.get("jet_phi0", 0.0), P.TOWER_JETS[jet][1])


def _vector_scale(jc, cos_t, sin_t, v_r, v_theta, v_h):
    """per component, the sum of the absolute values of the addends of JetCylToSimCartVector (longdouble), [n][3]"""
    ct, st, cp, sp = (abs(LD(getattr(jc, f))) for f in ("cos_theta", "sin_theta", "cos_phi", "sin_phi"))
    X = np.abs(v_r * cos_t) + np.abs(v_theta * sin_t)
    Y = np.abs(v_r * sin_t) + np.abs(v_theta * cos_t)
    Z = np.abs(v_h)
    return np.column_stack([X * cp * ct + Y * sp + Z * st * cp, X * sp * ct + Y * cp + Z * sp * st, X * st + Z * ct])


def _tower_scales(t, jc, field, p):
    """(S of the potential [n][3], S of the field [n][3]) at the points p, in longdouble from the inputs"""
    ld = SimpleNamespace(**{f: LD(getattr(jc, f)) for f in ("cos_theta", "sin_theta", "cos_phi", "sin_phi")})
    x, y, z = (p[:, d].astype(LD) for d in range(3))
    r, cos_t, sin_t, h = FB.sim_cart_to_jet_cyl(ld, x, y, z)
    l, field = LD(t.l_scale), LD(field)
    zero = np.zeros_like(r)
    if t.potential == FB.DONUT:
        e = np.exp(-(r / l) ** 2)
        inside = (np.abs(h) >= t.donut_offset) & (np.abs(h) <= t.donut_offset + t.donut_thickness)
        a = (zero, zero, np.where(inside, field * l * e, zero))
        b = (zero, np.where(inside, 2 * field * r / l * e, zero), zero)
    else:
        e = np.exp(-(r / l) ** 2 - (h / l) ** 2)
        a = (zero, field * r * e, field * l * LD(t.li_alpha) / 2 * e)
        # b_h = 2 field (1 - (r / l)^2) e: its two addends before the cancellation
        b = (field * 2 * (h / l) * (r / l) * e, field * LD(t.li_alpha) * (r / l) * e, field * 2 * (1 + (r / l) ** 2) * e)
    return (_vector_scale(ld, cos_t, sin_t, *a).astype(np.float64), _vector_scale(ld, cos_t, sin_t, *b).astype(np.float64))


@pytest.mark.parametrize("jet", ["aligned", "tilted"])
@pytest.mark.parametrize("pot", sorted(P.TOWER_DECKS))
def test_restated_tower_within_the_counted_bound(ref, meta, pot, jet):
    """feedback_reference's potential, field and density (numpy's exp) against PotentialInSimCart, FieldInSimCart and
    DensityFromSimCart: K = 11 and 5 (module docstring).  Which points lie inside the donut is decided before the exp:
    where the reference returns an exact zero vector so does the restatement, with |h| exactly offset and exactly
    offset + thickness inside and one ulp beyond either outside."""
    t, jc = _tower_ns(pot), _tower_jc(jet)
    key = "tower_%s_%s" % (pot, jet)
    p = ref[key + "_p"]
    x, y, z = p.T
    s_a, s_b = _tower_scales(t, jc, P.TOWER_FIELD, p)
    a = np.column_stack(FB.tower_potential(t, jc, P.TOWER_FIELD, x, y, z))
    b = np.column_stack(FB.tower_field(t, jc, P.TOWER_FIELD, x, y, z))
    assert np.array_equal(a == 0, ref[key + "_A"] == 0) and np.array_equal(b == 0, ref[key + "_B"] == 0)
    _within(a, ref[key + "_A"], K_TOWER, s_a, "restated tower A %s %s" % (pot, jet))
    _within(b, ref[key + "_B"], K_TOWER, s_b, "restated tower B %s %s" % (pot, jet))
    rho = FB.tower_density(t, jc, P.TOWER_DENSITY, x, y, z)
    _within(rho, ref[key + "_rho"], K_DENSITY, np.abs(ref[key + "_rho"]), "restated tower density %s %s" % (pot, jet))
    if pot == "donut" and jet == "aligned":
        lo, hi = P.TOWER_OFFSET, P.TOWER_OFFSET + P.TOWER_THICKNESS
        on_edge = np.isin(np.abs(z), (lo, hi)) & (np.hypot(x, y) < 0.02)
        outside = np.isin(np.abs(z), (np.nextafter(lo, 0.0), np.nextafter(hi, 1.0)))
        assert on_edge.sum() == 8 and outside.sum() == 8
        assert np.all(ref[key + "_A"][on_edge, 2] != 0) and not ref[key + "_A"][outside].any()
        assert not ref[key + "_A"][np.abs(x) >= 0.27].any()      # exp(-(27.5)^2) has underflowed


ALIGNED = [P.J + "jet_theta=0", P.J + "jet_phi0=0", P.J + "jet_phi_dot=0"]


def _block_potential(ref, pot, key="tower_block_%s_A", nx=P.BLOCK_NX):
    """the stored potential on the block's centres one cell beyond every side: [3][k][j][i]"""
    return ref[key % pot].reshape(nx[2] + 2, nx[1] + 2, nx[0] + 2, 3).transpose(3, 0, 1, 2)


def test_host_tower_initial_field_on_the_donuts_edges(ref):
    """as the test below, on the 4 x 4 x 13 block with the axis ALIGNED (h == x3 exactly): the planes k = +-2 sit exactly
    on |h| == donut_offset, the planes k = +-6 exactly on |h| == donut_offset + donut_thickness, and both are inside (the
    reference's >= and <=).  Every bit; the field next to either edge is the difference between a potential and an exact 0"""
    keys = P.mesh_keys(P.EDGE_NX, P.EDGE_XMIN) + P.TOWER_DECKS["donut"] + ALIGNED + [
        P.T + "initial_field=%r" % P.TOWER_FIELD, P.T + "li_alpha=0", "problem/cluster/agn_feedback/fixed_power=0"]
    u = _plan("cluster_magnetic_tower", keys).pgen_block(0)
    a = _block_potential(ref, "donut", "tower_edge_%s_A", P.EDGE_NX)
    assert a[2][1 + 6 + 6].any() and a[2][1 + 6 - 6].any() and not a[2][1 + 6 + 7].any() and not a[2][0].any()
    assert a[2][1 + 6 + 2].any() and not a[2][1 + 6 + 1].any() and not a[2][1 + 6].any()
    b, _ = FB.curl(a, (P.BLOCK_DX,) * 3)
    assert np.abs(b).max() > 0.1
    _bits(u[5:8], b, "host initial field on the donut's edges")


@pytest.mark.parametrize("pot", sorted(P.TOWER_DECKS))
def test_host_tower_initial_field_equals_the_curl_of_the_references_potential(ref, pot):
    """the host side of the tower: the problem generator's initial field of one 8 x 6 x 5 GLM-MHD block, axis tilted, is the
    central-difference curl ((A+ - A-) / dx / 2.0, feedback_reference.curl: IEEE operations only) of the reference's
    PotentialInSimCart at the six neighbours' centres (fixture: tower_block_<potential>_A on
    reference_physics_cases.block_centres(1)): every bit, the host's exp being the reference's"""
    keys = P.BLOCK_MESH + P.TOWER_DECKS[pot] + P.TOWER_JETS["block"][0] + [P.T + "initial_field=%r" % P.TOWER_FIELD,
                                                                          "problem/cluster/agn_feedback/fixed_power=0"]
    if pot == "donut":
        keys.append(P.T + "li_alpha=0")
    u = _plan("cluster_magnetic_tower", keys).pgen_block(0)
    b, _ = FB.curl(_block_potential(ref, pot), (P.BLOCK_DX,) * 3)
    assert np.abs(b).max() > 0.1
    _bits(u[5:8], b, "host initial field " + pot)


# ---- cooling ------------------------------------------------------------------------------------------------------------------------
def _restated_table(meta):
    v = meta["units"]["hse"]["values"]
    U = CO.Units(v["code_length_cgs"], v["code_mass_cgs"], v["code_time_cgs"])
    lt, ll = CO.read_table(P.SCHURE)
    return CO.Table(lt, ll, U.lambda_units(1.0), P.GAMMA, CO.composition(U, P.HE)[3], P.HE, U.mh), U


def _check_cooling(T, x, d, valid, what):
    got = np.array([T.dedt(e, rho) for e, rho in x])
    _bits(got[:, 0], d, what + " DeDt")
    assert np.array_equal(got[:, 1].astype(bool), valid), what + " valid"


def _check_rk(T, stepper, x, opt, yh, yl, valid, best, what):
    step, order = CO.STEPPERS[stepper]
    got = np.array([step(h, e0, lambda y: T.dedt(y, rho)) for e0, rho, h in x], dtype=np.float64)
    _bits(got[:, 0], yh, what + " y1_h")
    _bits(got[:, 1], yl, what + " y1_l")
    assert np.array_equal(got[:, 2].astype(bool), valid), what + " valid"
    _bits(np.array([CO.optimal_step(order, h, err, tol) for h, err, tol in opt]), best, what + " OptimalStep")


def test_restated_cooling_equals_the_references(ref, meta):
    """cooling_reference.Table computes with `math` (the reference binary's libm) in the reference's operation order: DeDt
    bit for bit with `valid`, on every crafted case -- e < 0, NaN, below the table, exactly on the first, an interior and the
    last node, one ulp either side of the interior node, the last interval, the free-free branch above -- and on the
    random ones.  On the last node the reference reads log_lambdas_(n_temp_), one past the end, times an exact zero (the
    stand-in pads that element); the restatement clamps the interval index instead: the same value."""
    T, _ = _restated_table(meta)
    labels = meta["cooling"]["labels"]
    _check_cooling(T, ref["dedt_x"], ref["dedt_out"], ref["dedt_valid"], "restated")
    d = dict(zip(labels, ref["dedt_out"]))
    assert d["below"] == 0 and d["just_below"] == 0 and d["first_node"] != 0 and d["last_node"] != 0 and d["far_above"] != 0
    assert list(np.flatnonzero(~ref["dedt_valid"])) == [labels.index("negative"), labels.index("nan")]


@pytest.mark.parametrize("stepper", ["rk12", "rk45"])
def test_restated_rk_steps_equal_the_references(ref, meta, stepper):
    """one RK12Stepper / RK45Stepper::Step with f = DeDt as tabular_cooling.cpp forms it, and OptimalStep: bit for bit,
    `valid` included (cleared by a later evaluation where the step drives y negative)"""
    T, _ = _restated_table(meta)
    valid = ref[stepper + "_valid"]
    assert 10 <= (~valid).sum() < len(valid) // 2
    _check_rk(T, stepper, ref[stepper + "_x"], ref[stepper + "_opt"], ref[stepper + "_yh"], ref[stepper + "_yl"], valid,
              ref[stepper + "_optimal"], "restated " + stepper)


def test_host_cooling_table_and_parameters_equal_what_reproduces_the_reference(ref, meta):
    """the host's parsed table (log lambda in code units) and CoolingParams are those of the restatement that reproduces
    every stored DeDt bit for bit: lambda_units, mbar_over_kb, mh, gamma, the rows; and mbar (gamma - 1) / k_B from the
    reference's own Units"""
    T, U = _restated_table(meta)
    p = _plan("cooling", meta["cooling"]["keys"])
    enabled, cp, _ = p.cooling_options()
    assert enabled and cp.lambda_units == U.lambda_units(1.0) and cp.mh == U.mh and cp.gamma == P.GAMMA
    assert cp.mbar_over_kb == CO.composition(U, P.HE)[3] and cp.He_mass_fraction == P.HE
    assert cp.mbar_over_kb * (cp.gamma - 1) == meta["cooling"]["mbar_gm1_over_kb"] == T.mbar_gm1_over_kb
    _bits(p.cooling_table("log_lambdas"), np.array(T.log_lambdas), "host log_lambdas")
    _bits(p.cooling_table("log_temps"), np.array(T.log_temps), "host log_temps")


# ---- limiters and the add-density helpers ------------------------------------------------------------------------------------------------
def _check_limiters(q, out):
    a, b, c, d = q.T
    with np.errstate(under="ignore"):
        _bits(DR._minmod(a, b), out[1], "minmod")
        _bits(DR._mc(a, b), out[2], "mc")
        _bits(DR._mc(a, b), out[3], "lim2")
        _bits(DR.lim4(a, b, c, d), out[4], "lim4")


def test_restated_limiters_equal_the_references(ref):
    """diffusion_reference's minmod, mc (= lim2) and lim4, which spitzer_reference imports: no transcendental, bit for bit,
    all sign patterns, zeros, equal arguments and same-sign pairs whose product underflows to 0 (the limiter returns 0)"""
    assert SR.lim4 is DR.lim4
    q, out = ref["limiters_q"], ref["limiters_out"]
    _check_limiters(q, out)
    tiny = (np.abs(q[:, 0]) < 1e-150) & (q[:, 0] * q[:, 1] == 0) & (q[:, 0] != 0) & (q[:, 1] != 0)
    assert tiny.sum() >= 2 and not out[:, tiny].any()


def _rows_as_block(rows):
    n = len(rows)
    return rows[:, 1:6].T.reshape(5, 1, 1, n).copy(), rows[:, 6:11].T.reshape(5, 1, 1, n).copy()


def _check_adddensity(rows, fixedvel, fixedveltemp):
    n = len(rows)
    u, w = _rows_as_block(rows)
    un, _ = TR.add_density_fixed_vel_temp(u, w, np.ones((1, 1, n), bool), rows[:, 0].reshape(1, 1, n), P.GAMMA)
    _bits(un.reshape(5, n).T, fixedveltemp, "triggering_reference AddDensityToConsAtFixedVelTemp")
    ones, zero = np.ones(1), np.zeros(1)
    for delta in sorted(set(rows[:, 0])):
        sel = rows[:, 0] == delta
        m = int(sel.sum())
        u, w = _rows_as_block(rows[sel])
        # SNIa feedback at r = 1 with rho_const_bcg = r_bcg_s ... = 1: the BCG density is exactly 1, the energy added 0
        c = CS.snia_cfg(0.0, delta, 1.0, 0.0)
        un, _, rho_bcg = CS.snia_feedback_src(u, w, np.ones(m), zero, zero, np.ones((1, 1, m), bool), c, 1.0, P.GAMMA)
        assert np.all(rho_bcg == 1.0)
        _bits(un.reshape(5, m).T, fixedvel[sel], "cluster_sources_reference AddDensityToConsAtFixedVel, delta %g" % delta)
        if delta > 0:    # AGN feedback's thermal sphere adds a positive density only
            cfg = SimpleNamespace(thermal_feedback=0.0, thermal_density=delta, thermal_radius=2.0, jet_density=0.0)
            un, _, info = FB.agn_feedback_src(u, w, ones.repeat(m), zero, zero, cfg, None, P.GAMMA)
            assert info.sphere.all()
            _bits(un.reshape(5, m).T, fixedvel[sel], "feedback_reference AddDensityToConsAtFixedVel, delta %g" % delta)


def test_restated_add_density_helpers_equal_the_references(ref):
    """AddDensityToConsAtFixedVel as restated inside feedback_reference.agn_feedback_src (the thermal sphere) and
    cluster_sources_reference.snia_feedback_src, AddDensityToConsAtFixedVelTemp as triggering_reference restates it: bit
    for bit on positive, negative and zero delta, with zero velocity among the rows"""
    rows = ref["adddensity_rows"]
    assert (rows[:, 0] > 0).any() and (rows[:, 0] < 0).any() and (rows[:, 0] == 0).any() and not rows[0, 7:10].any()
    _check_adddensity(rows, ref["adddensity_fixedvel"], ref["adddensity_fixedveltemp"])


# ---- CPU, live: fresh inputs through the binary ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_bin():
    path = O.build_ref(which="ref_physics") or O.ref_binary("ref_physics")   # (a binary that travelled here serves as well)
    if path is None:
        pytest.skip("oracle/_ref/ref_physics is missing and the reference tree (APK_REFERENCE_SRC, default %s) it is built "
                    "from is absent; the stored values above were checked without it" % O.REF_SRC_DEFAULT)
    return path


@pytest.mark.parametrize("deck", ["nfw", "all", "all_unsmoothed", "defaults_hse"])
def test_live_gravity_and_entropy(ref_bin, meta, deck):
    """20 000 equidistant radii through the host model (every bit) and 20 000 random ones through the restatement (K = 8,
    K = 6), expected values from the binary"""
    m = meta["gravity"][deck]
    entropy = "defaults_hse" if deck == "defaults_hse" else "deck"
    mesh = (1e-7, 3.0, N_LIVE, 1.0)
    from athenapk_amd import decks, driver
    keys = list(m["keys"]) + ["problem/cluster/hydrostatic_equilibrium/r_fix=%r" % mesh[3]]
    set_keys = {k.split("=")[0].split("/")[-1] for k in keys}
    strip = [k for k in P.GRAVITY_KEYS if k not in set_keys] + (["k_0", "k_100", "r_k", "alpha_k"] if deck == "defaults_hse" else [])
    p = driver.HostPlan(_strip(decks.load("cluster_hse"), strip), keys)
    got = p.he_sphere_profile(*mesh[:3])
    r = P.host_mesh_radii(mesh)
    _bits(got["r"], r, deck + " live r")
    _bits(got["g"], P.ref_gravity(deck, r), deck + " live host g")
    _bits(got["K"], P.ref_entropy(entropy, r), deck + " live host K")
    rng = np.random.default_rng(7000 + sorted(P.GRAVITY_DECKS).index(deck))
    r = P.gravity_radii(deck, rng, N_LIVE)
    c = p.cluster_options().gravity
    _within(_restated_gravity(c).g_from_r(r), P.ref_gravity(deck, r), K_G, P.gravity_scale(c, r), "live restated g " + deck)
    o = p.cluster_options()
    r = P.entropy_radii(entropy, rng, N_LIVE)
    s = CR.Sphere(None, o.k_0, o.k_100, o.r_k, o.alpha_k, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    scale = (LD(o.k_0) + LD(o.k_100) * (r.astype(LD) / LD(o.r_k)) ** LD(o.alpha_k)).astype(np.float64)
    _within(s.K_from_r(r), P.ref_entropy(entropy, r), K_K, scale, "live restated K " + entropy)


@pytest.mark.parametrize("case", sorted(P.JET_CASES))
def test_live_jet_transforms(ref_bin, meta, case):
    rng = np.random.default_rng(7100 + sorted(P.JET_CASES).index(case))
    p, v = P.jet_inputs(case, rng, N_LIVE)
    cyl, sim = P.ref_jet(P.JET_CASES[case], p, v)
    _check_jet(_host_jet(meta["jet"][case]), p, v, cyl, sim, "live " + case)


@pytest.mark.parametrize("jet", ["aligned", "tilted"])
@pytest.mark.parametrize("pot", sorted(P.TOWER_DECKS))
def test_live_tower(ref_bin, pot, jet):
    rng = np.random.default_rng(7200 + 2 * sorted(P.TOWER_DECKS).index(pot) + (jet == "tilted"))
    p = P.tower_points(jet, rng, N_LIVE)
    t, jc = _tower_ns(pot), _tower_jc(jet)
    a, b, rho = P.ref_tower(pot, jet, p)
    x, y, z = p.T
    s_a, s_b = _tower_scales(t, jc, P.TOWER_FIELD, p)
    _within(np.column_stack(FB.tower_potential(t, jc, P.TOWER_FIELD, x, y, z)), a, K_TOWER, s_a, "live restated tower A %s %s" % (pot, jet))
    _within(np.column_stack(FB.tower_field(t, jc, P.TOWER_FIELD, x, y, z)), b, K_TOWER, s_b, "live restated tower B %s %s" % (pot, jet))
    _within(FB.tower_density(t, jc, P.TOWER_DENSITY, x, y, z), rho, K_DENSITY, np.abs(rho), "live restated tower density %s %s" % (pot, jet))


def test_live_cooling(ref_bin, meta):
    T, _ = _restated_table(meta)
    c = meta["cooling"]["mbar_gm1_over_kb"]
    rng = np.random.default_rng(7300)
    x, _ = P.dedt_inputs(c, rng, N_LIVE)
    x = x[P.ref_keep(P.ref_dedt, x)]
    assert len(x) > 0.99 * N_LIVE
    d, valid = P.ref_dedt(x)
    _check_cooling(T, x, d, valid, "live restated")
    for stepper in ("rk12", "rk45"):
        xs, opt = P.rk_inputs(c, lambda a: P.ref_dedt(a)[0], rng, N_LIVE)
        keep = P.ref_keep(lambda a, b: P.ref_rkstep(stepper, a, b), xs, opt)
        assert keep.sum() > 0.99 * N_LIVE
        xs, opt = xs[keep], opt[keep]
        _check_rk(T, stepper, xs, opt, *P.ref_rkstep(stepper, xs, opt), "live restated " + stepper)


def test_live_limiters_and_add_density(ref_bin):
    rng = np.random.default_rng(7400)
    q = P.limiter_inputs(rng, N_LIVE)
    _check_limiters(q, P.ref_limiters(q))
    rows = P.adddensity_inputs(rng, N_LIVE)
    _check_adddensity(rows, P.ref_adddensity("fixedvel", rows), P.ref_adddensity("fixedveltemp", rows))


# ---- GPU, stored: the kernels of both builds ------------------------------------------------------------------------------------------------
BUILDS = pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])


def _ctx(request, strict):
    return request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")


def _held(got, want, K, scale, strict, what):
    """strict build: K eps S per entry (K = 0: every bit); product build: the project's 1e-12 x S"""
    if not strict:
        _product(got, want, scale, what)
    elif K == 0:
        _bits(got, want, what)
    else:
        _within(got, want, K, scale, "gpu " + what)


def _gravity_struct(c):
    from athenapk_amd import hydro
    return hydro.make_cluster_gravity(c.include_nfw, "HERNQUIST" if c.which_bcg else "NONE", c.include_smbh, c.r_nfw_s, c.g_const_nfw,
                                      c.r_bcg_s, c.g_const_bcg, c.g_const_smbh, c.smoothing_r)


@pytest.mark.gpu
@BUILDS
@pytest.mark.parametrize("deck", [d for d in sorted(P.GRAVITY_DECKS) if d != "defaults_cgs"])
def test_hip_g_from_r_against_reference_values(request, ref, meta, deck, strict):
    """ClusterGFromR on the stored radii with the host's constants of the stored deck entries.  Strict build: K = 8 (the
    device's log, budget 2 ulp, against glibc's); without NFW every bit.  Below the smoothing radius the value at it."""
    from athenapk_amd import hydro
    c = _host_constants(meta["gravity"][deck])
    r, want = ref["gravity_%s_r" % deck], ref["gravity_%s_g" % deck]
    got = hydro.ClusterGFromR(_ctx(request, strict), _gravity_struct(c), r)
    _held(got, want, K_G if c.include_nfw else 0, P.gravity_scale(c, r), strict, "g_from_r " + deck)
    if c.smoothing_r > 0:
        below = r < c.smoothing_r
        assert below.sum() >= 3 and np.all(got[below] == got[r == c.smoothing_r][0])


def _corners(xmins, mesh_xmin):
    return np.array([list(x) for x in xmins] + [list(mesh_xmin)])


@pytest.mark.gpu
@BUILDS
def test_hip_gravity_source_against_reference_values(request, ref, meta, strict):
    """GravitationalFieldSrcTerm on two blocks of 7 x 5 x 5 interior cells, nghost = 2, the first centred on the origin: its
    cell (3, 2, 2) has r == 0, where g_from_r is not finite (no smoothing) and only the src = 0 branch leaves the cell
    unchanged.  Expected: src = beta_dt rho g / r with the stored reference g at the cells' radii (fixture gravity_src_r,
    gravity_src_g), M_d -= src x_d, E -= src (x v1 + y v2 + z v3) (include/apk_amd.h).  Strict build: g carries
    K = 8 eps S_g; the two products and the quotient into src add 3 eps, the product with x_d and the final subtraction
    one each: |dM - dM_ref| <= eps ((8 S_g / g + 4) |src x_d| + |M|); for E the three products and two sums of x . v add
    3 eps of |x v1| + |y v2| + |z v3| instead of one.  Product build: 1e-12 (|M| + |src x_d|)."""
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    c = _host_constants(meta["gravity"][P.GRAV_DECK])
    u, w = P.grav_state()
    nx, ng, dx = P.GRAV_NX, P.GRAV_NG, P.GRAV_DX
    md = hydro.MeshData(ctx, nx, ng, 5, dx=(dx,) * 3, nblocks=2, cons=u, prim=w, with_flux=False)
    xmin_b = [P.GRAV_XMIN, (P.GRAV_XMIN[0] + 7 * dx, P.GRAV_XMIN[1], P.GRAV_XMIN[2])]
    hydro.GravitationalFieldSrcTerm(md, _gravity_struct(c), _corners(xmin_b, P.GRAV_XMIN), P.GRAV_BETA_DT)
    got = md.cons_host()
    r, g = ref["gravity_src_r"], ref["gravity_src_g"]
    _bits(r, P.grav_radii(), "the stored radii are the block's")
    assert r[0, 2, 2, 3] == 0 and np.count_nonzero(r == 0) == 1
    inner = (slice(ng, ng + nx[2]), slice(ng, ng + nx[1]), slice(ng, ng + nx[0]))
    s_g = P.gravity_scale(c, np.where(r == 0, 1.0, r))
    for b in (0, 1):
        x, y, z = P.grav_centres(b)
        X, Y, Z = np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])
        u0, w0, u1 = u[b][(slice(None),) + inner], w[b][(slice(None),) + inner], got[b][(slice(None),) + inner]
        with np.errstate(divide="ignore", invalid="ignore"):
            src = np.where(r[b] == 0, 0.0, P.GRAV_BETA_DT * w0[0] * g[b] / r[b])
            amp = np.where(r[b] == 0, 0.0, K_G * s_g[b] / np.where(g[b] == 0, 1.0, g[b]) + 4)
        _bits(u1[0], u0[0], "density, block %d" % b)
        for d, xd in enumerate((X, Y, Z)):
            want = u0[1 + d] - src * xd
            _held(u1[1 + d], want, 1, amp * np.abs(src * xd) + np.abs(want), strict, "gravity source M%d block %d" % (d + 1, b))
        dots = np.abs(X * w0[1]) + np.abs(Y * w0[2]) + np.abs(Z * w0[3])
        want = u0[4] - src * (X * w0[1] + Y * w0[2] + Z * w0[3])
        _held(u1[4], want, 1, (amp + 2) * np.abs(src) * dots + np.abs(want), strict, "gravity source E block %d" % b)
        mask = np.ones(got[b].shape, bool)
        mask[(slice(None),) + inner] = False
        _bits(got[b][mask], u[b][mask], "ghost cells, block %d" % b)
    _bits(got[0][:, ng + 2, ng + 2, ng + 3], u[0][:, ng + 2, ng + 2, ng + 3], "the cell at r == 0")
    assert np.all(np.isfinite(got))


def _dedt_bound(T, x, d):
    """eps |de/dt| (6 + ln 10 (32 slope + 2 ulp(log lambda) / eps)) per case (module docstring): 32 eps is 2 + 2 ulp of a
    log T below 16; one ulp of log lambda for its final sum, one for the table-cell decision"""
    k = np.zeros(len(x))
    for n, (e, _) in enumerate(x):
        ll = T.log_lambda(e)
        if ll is None:
            continue
        lt = math.log10(T.mbar_gm1_over_kb * e)
        i = min(max(int((lt - T.log_temp_start) / T.d_log_temp), 0), T.n - 2)
        near = [abs(T.log_lambdas[j + 1] - T.log_lambdas[j]) / T.d_log_temp for j in (max(i - 1, 0), i, min(i + 1, T.n - 2))]
        slope = 0.5 if lt > T.log_temp_final else max(near)
        k[n] = 6 + math.log(10.0) * (32 * slope + 2 * np.spacing(abs(ll)) / EPS)
    return k * np.abs(d)


def _device_table(ctx, meta):
    from athenapk_amd import hydro
    p = _plan("cooling", meta["cooling"]["keys"])
    _, cp, _ = p.cooling_options()
    lt, ll = CO.read_table(P.SCHURE)
    return hydro.TabularCooling(ctx, lt, ll, cp)


@pytest.mark.gpu
@BUILDS
def test_hip_dedt_against_reference_values(request, ref, meta, strict):
    """CoolingTable.DeDt on the stored (e, rho), the table built from the committed file with the host's CoolingParams of
    the stored deck entries.  `valid` matches exactly; where the reference returns 0 (below the table, invalid e) so does
    the kernel; else strict build within bound_i of the module docstring (S_i = |de/dt|), product build 1e-12 |de/dt|"""
    T, _ = _restated_table(meta)
    x, want, valid = ref["dedt_x"], ref["dedt_out"], ref["dedt_valid"]
    got, v = _device_table(_ctx(request, strict), meta).DeDt(x[:, 0], x[:, 1])
    assert np.array_equal(v, valid)
    assert np.array_equal(got == 0, want == 0)
    bound = _dedt_bound(T, x, want)
    if strict:
        _within(got, want, 1, bound / EPS, "gpu DeDt (fraction of bound_i)")
    else:
        _product(got, want, np.abs(want), "DeDt")


def _tower_setup(pot):
    """(lib.MagneticTowerCfg, lib.JetCoords) as the host parses the stored deck entries"""
    keys = P.TOWER_DECKS[pot] + P.TOWER_JETS["block"][0] + (["problem/cluster/magnetic_tower/li_alpha=0"] if pot == "donut" else [])
    p = _plan("cluster_magnetic_tower", keys)
    return p.magnetic_tower_cfg(), p.agn_feedback_stage_numbers(1e-3, P.TOWER_JETS["block"][1])[1]


def _tower_block_state():
    shape = tuple(P.BLOCK_NX[d] + 2 * P.BLOCK_NG for d in (2, 1, 0))
    return P.dyadic_state(np.random.default_rng(814), shape, mhd=True)


def _tree_sum(terms):
    """the block sum of the contributions kernel for fewer than 256 cells: one term per lane, then red[i] += red[i + s] for
    s = 128 ... 1"""
    a = np.zeros(256)
    a[:terms.size] = terms.ravel()
    s = 128
    while s > 0:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return a[0]


@pytest.mark.gpu
@BUILDS
@pytest.mark.parametrize("pot", sorted(P.TOWER_DECKS))
def test_hip_magnetic_tower_against_reference_values(request, ref, meta, pot, strict):
    """MagneticTowerSrcTerm and MagneticTowerPowerContribs on one 8 x 6 x 5 GLM-MHD block, axis tilted.

    Source: the expected added field b is the central-difference curl, (A+ - A-) / dx / 2.0 per term as include/apk_amd.h
    documents (feedback_reference.curl: IEEE operations only), of the REFERENCE's PotentialInSimCart at the centres of the
    cells' six neighbours -- fixture tower_block_<potential>_A, on reference_physics_cases.block_centres(1).  Strict build:
    each potential value carries K = 11 eps S_A (device exp); a term's difference and its two quotients add 3:
    |b - b_ref| <= 14 eps sum_terms (S_A+ + S_A-) / (2 dx); B = B0 + b one more eps |B|; E as test_gpu_cluster_feedback:
    sum_d (|B0_d| + |b_d|) tol_d + eps |E|.  The density from the reference's DensityFromSimCart at unit density (fixture
    tower_block_<potential>_rho1) times density_to_add: K = 5, plus eps |rho|.  Product build: 1e-12 of the same sizes.

    Contributions: from the reference's FieldInSimCart at unit strength (fixture tower_block_<potential>_B1), the 240
    terms added in the kernel's tree order.  lin: eps (sum_i vol (K + 2) sum_d |B0_d| S_B,d + 9 sum_i |t_i|), the 9 being
    the tree's eight levels and the term's product with vol; quad likewise with |b_d| for |B0_d|."""
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    tower, jet = _tower_setup(pot)
    u, w = _tower_block_state()
    nx, ng, dx = P.BLOCK_NX, P.BLOCK_NG, P.BLOCK_DX
    inner = (slice(None), slice(ng, ng + nx[2]), slice(ng, ng + nx[1]), slice(ng, ng + nx[0]))
    corners = _corners([P.BLOCK_XMIN], P.BLOCK_XMIN)
    md = hydro.MeshData(ctx, nx, ng, 9, dx=(dx,) * 3, nblocks=1, cons=u[None], prim=w[None], with_flux=False)
    contribs = hydro.MagneticTowerPowerContribs(md, tower, jet, corners)[0]
    mass = 2e-4
    hydro.MagneticTowerSrcTerm(md, tower, jet, corners, P.TOWER_FIELD, mass)
    got = md.cons_host()[0]
    u0, w0, u1 = u[inner], w[inner], got[inner]

    t, jc = _tower_ns(pot), _tower_jc("block")
    for f in ("cos_theta", "sin_theta", "cos_phi", "sin_phi"):
        assert getattr(jet, f) == getattr(jc, f)
    b, _ = FB.curl(_block_potential(ref, pot), (dx,) * 3)
    s_a, _ = _tower_scales(t, jc, P.TOWER_FIELD, P.block_points(1))
    _, size = FB.curl(s_a.reshape(nx[2] + 2, nx[1] + 2, nx[0] + 2, 3).transpose(3, 0, 1, 2), (dx,) * 3)
    tol = (K_TOWER + 3) * size
    assert np.abs(b).max() > 0.1
    for d in range(3):
        want = u0[5 + d] + b[d]
        _held(u1[5 + d], want, 1, tol[d] + np.abs(want), strict, "tower source B%d %s" % (d + 1, pot))
    want_e = u0[4] + (w0[5] * b[0] + w0[6] * b[1] + w0[7] * b[2] + 0.5 * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]))
    tol_e = sum((np.abs(w0[5 + d]) + np.abs(b[d])) * tol[d] for d in range(3)) + np.abs(want_e)
    _held(u1[4], want_e, 1, tol_e, strict, "tower source E " + pot)
    rho_add = FB.density_to_add(mass, float(t.l_mass_scale))
    d_rho = rho_add * ref["tower_block_%s_rho1" % pot].reshape(nx[2], nx[1], nx[0])
    assert np.all(d_rho > 0)
    _held(u1[0], u0[0] + d_rho, 1, K_DENSITY * d_rho + np.abs(u0[0] + d_rho), strict, "tower source rho " + pot)
    mask = np.ones(got.shape, bool)
    for v in (0, 4, 5, 6, 7):
        mask[(v,) + inner[1:]] = False
    _bits(got[mask], u[mask], "everything else")

    b1 = ref["tower_block_%s_B1" % pot].reshape(nx[2], nx[1], nx[0], 3).transpose(3, 0, 1, 2)
    _, s_b = _tower_scales(t, jc, 1.0, P.block_points(0))
    s_b = s_b.reshape(nx[2], nx[1], nx[0], 3).transpose(3, 0, 1, 2)
    vol = np.float64(dx) * np.float64(dx) * np.float64(dx)
    lin = (w0[5] * b1[0] + w0[6] * b1[1] + w0[7] * b1[2]) * vol
    quad = 0.5 * (b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]) * vol
    s_lin = (K_TOWER + 2) * vol * sum(np.abs(w0[5 + d]) * s_b[d] for d in range(3)).sum() + 9 * np.abs(lin).sum()
    s_quad = (K_TOWER + 2) * vol * sum(np.abs(b1[d]) * s_b[d] for d in range(3)).sum() + 9 * np.abs(quad).sum()
    assert quad.sum() > 0
    _held(contribs[0], _tree_sum(lin), 1, s_lin, strict, "tower linear contribution " + pot)
    _held(contribs[1], _tree_sum(quad), 1, s_quad, strict, "tower quadratic contribution " + pot)


@pytest.mark.gpu
@BUILDS
def test_hip_magnetic_tower_on_the_donuts_edges(request, ref, meta, strict):
    """MagneticTowerSrcTerm on the 4 x 4 x 13 block of test_host_tower_initial_field_on_the_donuts_edges (axis aligned, the
    planes k = +-2 and k = +-6 exactly on the donut's two edges, both inside): the added field against the curl of the
    reference's potential, bound as in test_hip_magnetic_tower_against_reference_values.  A kernel that took either edge
    for outside would miss the field of the neighbouring planes by the whole potential."""
    from athenapk_amd import hydro
    p = _plan("cluster_magnetic_tower", P.TOWER_DECKS["donut"] + ALIGNED + ["problem/cluster/magnetic_tower/li_alpha=0"])
    tower, jet = p.magnetic_tower_cfg(), p.agn_feedback_stage_numbers(1e-3, 0.0)[1]
    assert (jet.cos_theta, jet.sin_theta, jet.cos_phi, jet.sin_phi) == (1.0, 0.0, 1.0, 0.0)
    nx, ng, dx = P.EDGE_NX, P.BLOCK_NG, P.BLOCK_DX
    shape = tuple(nx[d] + 2 * ng for d in (2, 1, 0))
    u, w = P.dyadic_state(np.random.default_rng(815), shape, mhd=True)
    inner = (slice(None), slice(ng, ng + nx[2]), slice(ng, ng + nx[1]), slice(ng, ng + nx[0]))
    md = hydro.MeshData(_ctx(request, strict), nx, ng, 9, dx=(dx,) * 3, nblocks=1, cons=u[None], prim=w[None], with_flux=False)
    hydro.MagneticTowerSrcTerm(md, tower, jet, _corners([P.EDGE_XMIN], P.EDGE_XMIN), P.TOWER_FIELD, 0.0)
    got = md.cons_host()[0]
    b, _ = FB.curl(_block_potential(ref, "donut", "tower_edge_%s_A", P.EDGE_NX), (dx,) * 3)
    s_a, _ = _tower_scales(_tower_ns("donut"), _tower_jc("aligned"), P.TOWER_FIELD, P.block_points(1, P.EDGE_NX, P.EDGE_XMIN))
    _, size = FB.curl(s_a.reshape(nx[2] + 2, nx[1] + 2, nx[0] + 2, 3).transpose(3, 0, 1, 2), (dx,) * 3)
    for d in range(3):
        want = u[inner][5 + d] + b[d]
        _held(got[inner][5 + d], want, 1, (K_TOWER + 3) * size[d] + np.abs(want), strict, "tower source B%d on the donut's edges" % (d + 1))
    _bits(got[inner][0], u[inner][0], "no mass is added")


@pytest.mark.gpu
@BUILDS
def test_hip_agn_feedback_against_reference_values(request, ref, meta, strict):
    """AgnFeedbackSrcTerm on one 8 x 6 x 5 Euler block, axis aligned, thermal sphere and kinetic jet together.  The cells
    it changes are exactly those inside the sphere or the cylinders, derived from the REFERENCE's r and h at the cell
    centres (fixture jet_block_aligned_cyl): cylinders r < R_jet and offset <= |h| <= offset + thickness, with cells whose
    |h| is exactly the offset and exactly offset + thickness (both inclusive: they change); sphere r^2 + h^2 <= R_th^2 (no
    centre lies within rounding of that edge).  Inside the sphere and outside the cylinders the new conserved state is
    the reference's AddDensityToConsAtFixedVel on the same (cons, prim) rows (fixture agn_block_rows, agn_block_fixedvel):
    no transcendental, strict build every bit, product build 1e-12 (|u| + |delta terms|)."""
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    ctx = _ctx(request, strict)
    u, w = P.agn_block_state()
    nx, ng, dx = P.BLOCK_NX, P.BLOCK_NG, P.BLOCK_DX
    rows = ref["agn_block_rows"]
    _bits(rows, P.rows_of(P.AGN_DELTA, P.interior(u), P.interior(w)), "the stored rows are the block's state")
    cfg = L.AgnFeedbackCfg()
    for k, v in P.AGN_CFG.items():
        setattr(cfg, k, v)
    jet = _host_jet(meta["jet"]["aligned"])
    md = hydro.MeshData(ctx, nx, ng, 5, dx=(dx,) * 3, nblocks=1, cons=u[None], prim=w[None], with_flux=False)
    hydro.AgnFeedbackSrcTerm(md, "euler", L.make_eos(P.GAMMA), cfg, jet, _corners([P.BLOCK_XMIN], P.BLOCK_XMIN))
    got = md.cons_host()[0]
    ctx.poll_flags()
    u1 = P.interior(got).reshape(5, -1).T
    u0 = rows[:, 1:6]
    r, h = ref["jet_block_aligned_cyl"][:, 0], ref["jet_block_aligned_cyl"][:, 3]
    c = P.AGN_CFG
    in_jet = (r < c["kinetic_jet_radius"]) & (np.abs(h) >= c["kinetic_jet_offset"]) & \
             (np.abs(h) <= c["kinetic_jet_offset"] + c["kinetic_jet_thickness"])
    in_sphere = r * r + h * h <= c["thermal_radius"] ** 2
    on_edges = in_jet & ((np.abs(h) == c["kinetic_jet_offset"]) | (np.abs(h) == c["kinetic_jet_offset"] + c["kinetic_jet_thickness"]))
    assert in_jet.sum() == 48 and on_edges.sum() == 48 and (in_sphere & ~in_jet).sum() >= 8 and (in_jet & ~in_sphere).sum() >= 4
    changed = np.any(u1 != u0, axis=1)
    assert np.array_equal(changed, in_jet | in_sphere), np.flatnonzero(changed != (in_jet | in_sphere))
    only = in_sphere & ~in_jet
    want = ref["agn_block_fixedvel"][only]
    scale = np.abs(u0[only]) + np.abs(want - u0[only])
    _held(u1[only], want, 0, scale, strict, "AddDensityToConsAtFixedVel in the thermal sphere")
    assert np.all(u1[in_jet, 0] == u0[in_jet, 0] + c["jet_density"] + np.where(in_sphere[in_jet], P.AGN_DELTA, 0.0))
    ghost = np.ones(got.shape, bool)
    ghost[:, ng:ng + nx[2], ng:ng + nx[1], ng:ng + nx[0]] = False
    _bits(got[ghost], u[ghost], "ghost cells")


@pytest.mark.gpu
@BUILDS
def test_hip_triggering_removal_against_reference_values(ref, strict):
    """The cold-gas removal of AGN triggering on one 8^3 block: the accretion sphere's active box is 4 x 4 x 4 cells, of
    which the eight corners lie outside the sphere.  Everything is cold; dt and cold_t_acc are powers of two, so the
    removed density -rho / cold_t_acc dt is exact.  The new conserved state of the 56 cells equals the reference's
    AddDensityToConsAtFixedVelTemp on the same rows (fixture trig_rows, trig_fixedveltemp): strict build every bit, product
    build 1e-12 (|u| + |delta terms|); the corners and every other cell keep their bits."""
    from cluster_cases import read as _read, sim as _deck_sim
    TRIG = "problem/cluster/agn_triggering/"
    ov = P.TRIG_MESH + [TRIG + "triggering_mode=COLD_GAS", TRIG + "accretion_radius=%r" % P.TRIG_RADIUS,
                        TRIG + "cold_t_acc=%r" % P.TRIG_T_ACC, TRIG + "cold_temp_thresh=1e300", "hydro/fluid=euler"]
    s = _deck_sim("cluster_agn_triggering", ov, strict=strict).initialize()
    u, w = P.trig_state()
    s.write_block(0, u)
    s.fill_derived()
    (u0, w0), = _read(s)
    box = (slice(None),) + P.TRIG_BOX
    _bits(u0[box], u[box], "the state as written")
    _bits(w0[box], w[box], "the primitives the device derives are the dyadic state's")
    rows = ref["trig_rows"]
    _bits(rows, P.rows_of(-w[box][0] / P.TRIG_T_ACC * P.TRIG_DT, u[box], w[box]), "the stored rows are the box's state")
    s.agn_triggering_reduce(P.TRIG_DT)
    (u1, _), = _read(s)
    s.close()
    x = -0.5 + (np.arange(-2, 10) + 0.5) * 0.125
    X, Y, Z = np.broadcast_arrays(x[None, None, :], x[None, :, None], x[:, None, None])
    sphere = X * X + Y * Y + Z * Z < P.TRIG_RADIUS ** 2
    in_box = np.zeros(sphere.shape, bool)
    in_box[P.TRIG_BOX] = True
    assert sphere.sum() == 56 and np.all(in_box[sphere])
    changed = np.any(u1 != u0, axis=0)
    assert np.array_equal(changed, sphere)
    sel = sphere[P.TRIG_BOX].ravel()
    got = u1[box].reshape(5, -1).T
    want = ref["trig_fixedveltemp"]
    scale = np.abs(rows[:, 1:6]) + np.abs(want - rows[:, 1:6])
    _held(got[sel], want[sel], 0, scale[sel], strict, "AddDensityToConsAtFixedVelTemp in the accretion sphere")


# ---- GPU, live: fresh inputs, expected values from the binary if it travelled ---------------------------------------------------------------
def _travelled_binary():
    path = O.ref_binary("ref_physics")
    if path is None:
        pytest.skip("oracle/_ref/ref_physics is not here (it is built only where the reference tree is, and is not committed)")
    try:
        r = subprocess.run([path, "limiters", "0"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=20)
    except OSError as e:
        pytest.skip("oracle/_ref/ref_physics does not start here: %s" % e)
    if r.returncode != 0:
        pytest.skip("oracle/_ref/ref_physics does not run here: exit %d" % r.returncode)
    return path


@pytest.mark.gpu
@BUILDS
def test_live_hip_g_from_r_and_dedt_against_the_reference_binary(request, meta, strict):
    """4096 fresh radii (all three components, smoothed) and 4096 fresh (e, rho) points: the comparisons of the stored tier"""
    from athenapk_amd import hydro
    _travelled_binary()
    ctx = _ctx(request, strict)
    rng = np.random.default_rng(8000)
    c = _host_constants(meta["gravity"]["all"])
    r = P.gravity_radii("all", rng, N_LIVE_GPU)
    _held(hydro.ClusterGFromR(ctx, _gravity_struct(c), r), P.ref_gravity("all", r), K_G, P.gravity_scale(c, r), strict, "live g_from_r")
    T, _ = _restated_table(meta)
    x, _ = P.dedt_inputs(meta["cooling"]["mbar_gm1_over_kb"], rng, N_LIVE_GPU)
    x = x[P.ref_keep(P.ref_dedt, x)]
    want, valid = P.ref_dedt(x)
    got, v = _device_table(ctx, meta).DeDt(x[:, 0], x[:, 1])
    assert np.array_equal(v, valid) and np.array_equal(got == 0, want == 0)
    if strict:
        _within(got, want, 1, _dedt_bound(T, x, want) / EPS, "gpu live DeDt (fraction of bound_i)")
    else:
        _product(got, want, np.abs(want), "live DeDt")
