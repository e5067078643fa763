"""CPU tests of the cluster problem's AGN feedback on the host side (no GPU): the derived jet numbers and the five
consistency requirements, the refusals, the magnetic tower's initial field through the problem generator, the power
scaling's quadratic, and the energy the discrete curl injects -- against the numpy restatement
(tests/feedback_reference.py)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402
import feedback_reference as FB  # noqa: E402

EPS = np.finfo(np.float64).eps
AGN = "problem/cluster/agn_feedback/"
TOWER = "problem/cluster/magnetic_tower/"
JET = "problem/cluster/precessing_jet/"


def _plan(overrides=(), deck="cluster_agn_feedback"):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides), strict=True)


def _refused(overrides=(), deck="cluster_agn_feedback"):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def _units_numbers():
    """speed_of_light and mbar_over_kb (gamma - 1) of the decks' units and composition, restated"""
    u = R.DECK_UNITS
    c = FB.C_CGS / (u.l / u.t)
    mu, _ = R.composition(R.DECK_HE)
    mbar_over_kb = mu * u.mh() / u.k_boltzmann()
    return float(c), float(mbar_over_kb * (np.float64(R.DECK_GAMMA) - 1.0))


def _model(**kw):
    c, mb = _units_numbers()
    base = dict(fixed_power=0.3319965633348794, efficiency=1e-3, thermal_fraction=0.5, kinetic_fraction=0.5,
                thermal_radius=0.1, kinetic_jet_radius=0.05, kinetic_jet_thickness=0.05, kinetic_jet_offset=0.01)
    base.update(kw)
    return FB.agn_model(c, mb, **base)


def _jet_overrides(v, T):
    """the deck gives the temperature; a case without it has to take the key out"""
    from athenapk_amd import decks
    deck = decks.load("cluster_agn_feedback")
    line = [ln for ln in deck.splitlines() if ln.startswith("kinetic_jet_temperature")]
    assert len(line) == 1
    deck = deck.replace(line[0] + "\n", "")
    ov = []
    if v is not None:
        ov.append(AGN + "kinetic_jet_velocity=%r" % v)
    if T is not None:
        ov.append(AGN + "kinetic_jet_temperature=%r" % T)
    return deck, ov


def _plan_jet(v, T, efficiency=1e-3):
    from athenapk_amd import driver
    deck, ov = _jet_overrides(v, T)
    return driver.HostPlan(deck, ov + [AGN + "efficiency=%r" % efficiency], strict=True)


# ---- 1. the derived jet numbers --------------------------------------------------------------------------------------------
def test_the_units_the_derivations_take():
    o = _plan().agn_feedback_options()
    c, mb = _units_numbers()
    assert o.configured == 1 and o.active == 1 and o.tower_power_scaling == 0
    assert o.speed_of_light == c and o.mbar_gm1_over_kb == mb


@pytest.mark.parametrize("case", ["neither", "temperature", "velocity", "both"])
def test_derived_jet_numbers_bit_for_bit(case):
    """velocity and / or temperature given: the three derivations of AGNFeedback's constructor, every number equal to the
    restatement's (products, quotients, sums and correctly rounded roots of the same numbers in the same order)"""
    if case == "neither":
        v, T = None, None
    elif case == "temperature":
        v, T = None, 1e7
    elif case == "velocity":
        # (a velocity whose round trip through e_jet comes back within the reference's 10 eps, an ABSOLUTE bound in code
        # units: the restatement says so before the host is asked)
        v, T = 8.0, None
    else:
        T = 3e6
        v = _model(kinetic_jet_temperature=T).kinetic_jet_velocity
    want = _model(kinetic_jet_velocity=v, kinetic_jet_temperature=T)
    o = _plan_jet(v, T).agn_feedback_options()
    assert o.assumed_cold_jet == (1 if case == "neither" else 0)
    assert (o.kinetic_jet_velocity, o.kinetic_jet_temperature, o.kinetic_jet_e) == \
        (want.kinetic_jet_velocity, want.kinetic_jet_temperature, want.kinetic_jet_e)
    assert (o.thermal_fraction, o.kinetic_fraction, o.magnetic_fraction) == (0.5, 0.5, 0.0)
    assert (o.thermal_mass_fraction, o.kinetic_mass_fraction, o.magnetic_mass_fraction) == (0.5, 0.5, 0.0)
    assert o.power == want.power and o.mass_rate == want.mass_rate and o.eceil == math.inf


def test_fractions_are_normalised_and_mass_fractions_follow_the_switch():
    ov = [AGN + "thermal_fraction=1", AGN + "kinetic_fraction=2", AGN + "magnetic_fraction=1", "hydro/fluid=glmmhd",
          TOWER + "potential_type=li", TOWER + "l_scale=0.01"]
    o = _plan(ov).agn_feedback_options()
    want = _model(thermal_fraction=1, kinetic_fraction=2, magnetic_fraction=1, kinetic_jet_temperature=1e7)
    assert (o.thermal_fraction, o.kinetic_fraction, o.magnetic_fraction) == (0.25, 0.5, 0.25)
    assert o.magnetic_mass_fraction == 0.25 and o.tower_power_scaling == 1
    o = _plan(ov + [AGN + "enable_magnetic_tower_mass_injection=false"]).agn_feedback_options()
    want = _model(thermal_fraction=1, kinetic_fraction=2, magnetic_fraction=1, kinetic_jet_temperature=1e7,
                  enable_magnetic_tower_mass_injection=False)
    assert (o.thermal_mass_fraction, o.kinetic_mass_fraction, o.magnetic_mass_fraction) == \
        (want.thermal_mass_fraction, want.kinetic_mass_fraction, 0.0)
    assert o.thermal_mass_fraction == 0.25 / 0.75


def test_tceil_gives_eceil_and_stage_numbers_bit_for_bit():
    p = _plan([AGN + "Tceil=5e8", AGN + "vceil=12.5", JET + "jet_phi_dot=3.0"])
    o = p.agn_feedback_options()
    want = _model(kinetic_jet_temperature=1e7, Tceil=5e8, vceil=12.5)
    assert o.eceil == want.eceil and o.vceil == 12.5 and o.Tceil == 5e8
    for beta_dt, time in ((1e-4, 0.0), (0.37e-3, 0.0125)):
        cfg, jet = p.agn_feedback_stage_numbers(beta_dt, time)
        c = FB.stage_numbers(want, beta_dt)
        for name in ("thermal_feedback", "thermal_density", "thermal_radius", "jet_density", "jet_momentum", "jet_feedback",
                     "kinetic_jet_radius", "kinetic_jet_thickness", "kinetic_jet_offset", "vceil", "eceil"):
            assert getattr(cfg, name) == getattr(c, name), name
        jc = FB.jet_coords(0.4, 3.0, 1.2, time)
        assert (jet.cos_theta, jet.sin_theta, jet.cos_phi, jet.sin_phi) == (jc.cos_theta, jc.sin_theta, jc.cos_phi, jc.sin_phi)


def _edge_temperatures(eff):
    """Temperatures at the upper end of what the efficiency allows, where e_jet = T / (mbar (gamma - 1) / k_B) makes the
    radicand 2 (eps c^2 - (1 - eps) e_jet) exactly zero: split by whether e_jet then exceeds c^2 eps / (1 - eps) in
    floating point (the third requirement's only way to fire: any larger e_jet fails the first one on a NaN)."""
    c, mb = _units_numbers()
    bound = (c * c) * eff / (1 - eff)
    above, within = [], []
    T = bound * mb
    for k in range(-64, 65):
        Tk = T * (1 + k * EPS)
        e = Tk / mb
        if 2 * (eff * (c * c) - (1 - eff) * e) == 0.0:
            (above if e > bound else within).append(float(Tk))
    return above, within


REQUIREMENTS = {
    "incompatible": "Specified kinetic jet velocity and temperature are incompatible with mass to energy conversion efficiency",
    "negative_temperature": "Kinetic jet velocity implies negative temperature of the jet",
    "negative_kinetic": "Kinetic jet temperature implies negative kinetic energy of the jet",
    "velocity_sign": "Kinetic jet velocity must be non-negative",
    "temperature_sign": "Kinetic jet temperature must be non-negative",
}


@pytest.mark.parametrize("which", sorted(REQUIREMENTS))
def test_each_consistency_requirement_with_its_message(which):
    """The five PARTHENON_REQUIREs of AGNFeedback's constructor in their order.  The later ones are shadowed by the earlier
    ones except at the edges: a negative velocity never equals a root (first requirement) unless the root is 0 and the
    velocity -tiny; a negative temperature gives a velocity above the limit (second) unless it is -tiny; an e_jet above
    its limit gives a NaN root (first) unless the radicand rounds to zero -- which in the decks' units happens at an
    efficiency of 0.37, not at 1e-3.  Each case is first put to the restatement, which must raise this very message."""
    c, _ = _units_numbers()
    eff = 0.37 if which == "negative_kinetic" else 1e-3
    above, within = _edge_temperatures(eff)
    if which == "incompatible":
        v, T = 5.0, 1e7
    elif which == "negative_temperature":
        v, T = 1.001 * c * math.sqrt(2e-3), None
    elif which == "negative_kinetic":
        assert above, "no temperature found whose e_jet exceeds its limit while the radicand rounds to zero"
        v, T = 0.0, above[0]
    elif which == "velocity_sign":
        assert within
        v, T = -1e-300, within[0]
    else:
        v, T = None, -1e-20
    with pytest.raises(FB.RequirementError) as e:
        _model(kinetic_jet_velocity=v, kinetic_jet_temperature=T, efficiency=eff)
    assert REQUIREMENTS[which] in str(e.value)
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan_jet(v, T, eff)
    assert REQUIREMENTS[which] in str(e.value)


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------
MHD = ["hydro/fluid=glmmhd"]
LI_TOWER = [TOWER + "potential_type=li", TOWER + "l_scale=0.01", TOWER + "li_alpha=20"]
REFUSALS = [
    ([AGN + "thermal_fraction=0", AGN + "kinetic_fraction=0"], None, AGN + "fixed_power"),
    ([AGN + "magnetic_fraction=0.5"], None, AGN + "magnetic_fraction"),
    (LI_TOWER + [TOWER + "initial_field=0.1"], None, TOWER + "initial_field"),
    (LI_TOWER + [TOWER + "fixed_field_rate=0.1"], None, TOWER + "fixed_field_rate"),
    (LI_TOWER + [TOWER + "fixed_mass_rate=0.1"], None, TOWER + "fixed_mass_rate"),
    (MHD + [TOWER + "potential_type=dipole", TOWER + "l_scale=0.01"], None, TOWER + "potential_type"),
    (MHD + [TOWER + "l_scale=0.01", TOWER + "initial_field=0.1"], None, TOWER + "potential_type"),
    ([AGN + "enable_tracer=true"], None, AGN + "enable_tracer"),
    (["problem/cluster/agn_triggering/triggering_mode=COLD_GAS"], None, "problem/cluster/agn_triggering/triggering_mode"),
    (["parthenon/mesh/refinement=static"], None, "parthenon/mesh/refinement"),
    (["problem/cluster/clips/vceil=10"], None, "problem/cluster/clips/vceil"),
    (["problem/cluster/stellar_feedback/efficiency=1e-3"], None, "problem/cluster/stellar_feedback"),
    (["problem/cluster/snia_feedback/disabled=false"], None, "problem/cluster/snia_feedback/disabled"),
]


@pytest.mark.parametrize("overrides,_,key", REFUSALS, ids=[k + "#%d" % n for n, (_, _, k) in enumerate(REFUSALS)])
def test_refusals_name_their_key(overrides, _, key):
    assert key in _refused(overrides)


def test_fixed_power_without_units_or_composition_is_refused():
    from athenapk_amd import decks
    deck = decks.load("cluster_agn_feedback")
    no_he = deck.replace("He_mass_fraction = 0.25\n", "")
    assert no_he != deck
    from athenapk_amd import driver, lib as L
    with pytest.raises(L.ApkError) as e:
        driver.HostPlan(no_he, [], strict=True)
    msg = str(e.value)
    assert AGN + "fixed_power" in msg and "units and gas composition" in msg


def test_combination_checks_of_the_tower_with_the_references_wording():
    assert "Incompatible combination of donut_offset and donut_thickness" in \
        _refused(MHD + [TOWER + "potential_type=donut", TOWER + "l_scale=0.01"])
    assert "Please disable (set to zero) tower li_alpha for the donut model" in \
        _refused(MHD + [TOWER + "potential_type=donut", TOWER + "l_scale=0.01", TOWER + "donut_thickness=0.01",
                        TOWER + "li_alpha=20"])
    assert "Please disable (set to zero) tower offset and thickness for the Li tower model" in \
        _refused(MHD + LI_TOWER + [TOWER + "donut_thickness=0.01"])
    assert "Magnetic Tower Length scale must be strictly postitive" in \
        _refused(MHD + [TOWER + "potential_type=li", TOWER + "initial_field=0.1"])
    assert "AGN feedback energy fractions must be non-negative" in _refused([AGN + "thermal_fraction=-0.5"])


def test_what_the_parser_now_accepts():
    """fixed_power with fractions set; a tower block with its potential_type; both decks as shipped; the sources send
    the run through the flux arrays (no fused stage) by the predicate gravity uses"""
    o = _plan().agn_feedback_options()
    assert o.active == 1 and o.fixed_power == 0.3319965633348794
    p = _plan(deck="cluster_magnetic_tower")
    o = p.agn_feedback_options()
    assert o.active == 1 and o.tower_power_scaling == 1 and o.tower_potential == 1 and o.magnetic_fraction == 1.0
    assert o.li_alpha == 20 and o.l_scale == 0.01 and o.initial_field == 0.1243156000020414 and o.l_mass_scale == 0.005
    o = _plan([TOWER + "potential_type=donut", TOWER + "li_alpha=0", TOWER + "donut_offset=0.005",
               TOWER + "donut_thickness=0.01"], deck="cluster_magnetic_tower").agn_feedback_options()
    assert o.tower_potential == 2 and o.donut_thickness == 0.01
    # disabled, or no power: parsed, not active
    assert _plan([AGN + "disabled=true"]).agn_feedback_options().active == 0
    assert _plan([AGN + "fixed_power=0"]).agn_feedback_options().active == 0
    # the atmosphere deck knows nothing of this
    o = _plan(deck="cluster_hse").agn_feedback_options()
    assert o.configured == 0 and o.active == 0 and o.fixed_power == 0.0


# ---- 3. the initial field ---------------------------------------------------------------------------------------------------------
MESH16 = ["parthenon/mesh/nx%d=16" % d for d in (1, 2, 3)] + ["parthenon/meshblock/nx%d=8" % d for d in (1, 2, 3)]
TILT = [JET + "jet_theta=0.2", JET + "jet_phi0=1"]
POTENTIALS = {
    "li": [TOWER + "potential_type=li", TOWER + "li_alpha=20", TOWER + "l_scale=0.04"],
    "donut": [TOWER + "potential_type=donut", TOWER + "li_alpha=0", TOWER + "l_scale=0.04", TOWER + "donut_offset=0.01",
              TOWER + "donut_thickness=0.05"],
}


def _restated_tower(potential):
    if potential == "li":
        return FB.tower("li", 0.04, li_alpha=20, l_mass_scale=0.005)
    return FB.tower("donut", 0.04, donut_offset=0.01, donut_thickness=0.05, l_mass_scale=0.005)


@pytest.mark.parametrize("potential", sorted(POTENTIALS))
def test_initial_field_of_every_block(potential):
    """cluster_magnetic_tower at 16^3 in 8^3 blocks (l_scale 0.04: a few cells), axis tilted by 0.2 and turned by 1:
    B of pgen_block against the restatement's central-difference curl within
    8 eps sum_terms (|A+| + |A-|) / (2 dx_d) + 2 eps |B| -- the host's exp and numpy's are each within 1 ulp, the IEEE
    operations after them are the same; E - 0.5 B^2 equals the field-free energy to 2 eps; and the central-difference
    divergence of the gathered field, on cells one off the mesh boundary, stays below 64 eps max|A| / min(dx)^2 (zero in
    exact arithmetic: the bound counts the roundings of the differences and quotients on both sides)."""
    p = _plan(MESH16 + TILT + POTENTIALS[potential] + [AGN + "fixed_power=0"], deck="cluster_magnetic_tower")
    info = p.info
    assert tuple(info.mb) == (8, 8, 8) and info.nblocks_local == 8
    t, jc = _restated_tower(potential), FB.jet_coords(0.2, 0.0, 1.0, 0.0)
    field = 0.1243156000020414
    dx = tuple(info.dx)
    e0 = R.pgen_uniform((8, 8, 8), 147.75575892787222, 0, 0, 0, 1.5454368403867558, R.DECK_GAMMA)[4]
    B = np.zeros((3, 16, 16, 16))
    amax, worst, identical = 0.0, 0.0, True
    for lb in range(info.nblocks_local):
        loc = p.block_gid(lb)[1]
        u = p.pgen_block(lb)
        xe = [R.cell_centres(info.xmin[d], dx[d], loc[d] * 8 - 1, 10) for d in range(3)]
        want, size, a = FB.tower_curl_field(t, jc, field, xe[0], xe[1], xe[2], dx)
        tol = FB.tol_b(want, size)
        err = np.abs(u[5:8] - want)
        assert np.all(err <= tol), lb
        worst = max(worst, float(np.max(err[tol > 0] / tol[tol > 0])))
        identical = identical and np.array_equal(u[5:8], want)
        assert np.any(want != 0)
        e_gas = u[4] - 0.5 * (u[5] * u[5] + u[6] * u[6] + u[7] * u[7])
        assert np.all(np.abs(e_gas - e0) <= 2 * EPS * np.abs(u[4]))
        assert np.all(u[8] == 0) and np.all(u[1:4] == 0) and np.all(u[0] == 147.75575892787222)
        sl = tuple(slice(loc[d] * 8, loc[d] * 8 + 8) for d in (2, 1, 0))
        B[(slice(None),) + sl] = u[5:8]
        amax = max(amax, max(float(np.max(np.abs(c))) for c in a))
    print("%s: max err / bound %.3f; host and numpy identical: %s" % (potential, worst, identical))
    c = slice(1, -1)
    div = ((B[0][c, c, 2:] - B[0][c, c, :-2]) / dx[0] / 2.0 + (B[1][c, 2:, c] - B[1][c, :-2, c]) / dx[1] / 2.0 +
           (B[2][2:, c, c] - B[2][:-2, c, c]) / dx[2] / 2.0)
    bound = 64 * EPS * amax / min(dx) ** 2
    print("max |div B| %.3e, bound %.3e, max |B| %.3e" % (np.max(np.abs(div)), bound, np.max(np.abs(B))))
    assert np.max(np.abs(div)) <= bound


def test_the_uniform_field_is_added_to_the_towers():
    """cluster.cpp:630-653 after 556-625: B = curl A + b, E gains B_tower . b + 0.5 b^2 on top of 0.5 B_tower^2"""
    base = MESH16 + TILT + POTENTIALS["li"] + [AGN + "fixed_power=0"]
    b = (0.3, -0.2, 0.1)
    ub = ["problem/cluster/uniform_b_field/init_uniform_b_field=true"] + \
         ["problem/cluster/uniform_b_field/b%s=%r" % (n, v) for n, v in zip("xyz", b)]
    u0 = _plan(base, deck="cluster_magnetic_tower").pgen_block(3)
    u1 = _plan(base + ub, deck="cluster_magnetic_tower").pgen_block(3)
    for n in range(3):
        assert np.array_equal(u1[5 + n], u0[5 + n] + b[n])
    want = u0[4] + (u0[5] * b[0] + u0[6] * b[1] + u0[7] * b[2] + 0.5 * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]))
    assert np.array_equal(u1[4], want)


# ---- 4. the power scaling ------------------------------------------------------------------------------------------------------------
def _residual(lin, quad, f, rhs_terms):
    """(|lin f + quad f^2 - beta_dt P|, the larger term), evaluated exactly: the comparison itself must not round"""
    from fractions import Fraction as Q
    beta_dt, power = rhs_terms
    a, b, rhs = Q(lin) * Q(f), Q(quad) * Q(f) * Q(f), Q(beta_dt) * Q(power)
    return abs(a + b - rhs), max(abs(a), abs(b), abs(rhs))


QUAD, BETA_DT, POWER = 0.0213, 1.7e-4, 0.0016599828166743973


@pytest.mark.parametrize("lin", [1e-5, -1e-5, 0.0, 1e-4, -0.37, -2.5e3])
def test_scale_factor_solves_its_quadratic(lin):
    """lin f + quad f^2 = beta_dt P to 4 eps of the larger term, for lin of either sign, and the host equals the
    restatement bit for bit (products, sums, one root, one quotient).  sqrt(4 quad beta_dt P) = 1.6e-4 here: the
    positive lin of these cases stay below it, so that -lin + sqrt(lin^2 + ...) keeps its digits; a negative lin adds
    two positive numbers at any size.  (The cancelling case is the next test.)"""
    from fractions import Fraction as Q
    p = _plan(deck="cluster_magnetic_tower")
    f = p.magnetic_tower_field_to_add(lin, QUAD, BETA_DT, POWER)
    assert f == FB.field_to_add(lin, QUAD, BETA_DT, POWER) and f > 0
    res, larger = _residual(lin, QUAD, f, (BETA_DT, POWER))
    print("lin %g: f = %.17g, residual / (eps larger) = %.3f" % (lin, f, float(res / (Q(EPS) * larger))))
    assert res <= 4 * Q(EPS) * larger


def test_scale_factor_with_a_dominant_positive_linear_term_is_the_references_formula():
    """lin = 0.37 against sqrt(4 quad beta_dt P) = 1.6e-4: the reference's -lin + sqrt(lin^2 + ...) subtracts two numbers
    that agree in seven digits, and the residual of the quadratic is that loss, about lin^2 / (quad beta_dt P) eps of the
    larger term -- the formula's own, restated operation for operation: the host equals the restatement bit for bit, and
    the residual is printed, not bounded by 4 eps."""
    from fractions import Fraction as Q
    p = _plan(deck="cluster_magnetic_tower")
    f = p.magnetic_tower_field_to_add(0.37, QUAD, BETA_DT, POWER)
    assert f == FB.field_to_add(0.37, QUAD, BETA_DT, POWER) and f > 0
    res, larger = _residual(0.37, QUAD, f, (BETA_DT, POWER))
    print("lin 0.37: residual / (eps larger) = %.3g" % float(res / (Q(EPS) * larger)))
    assert res <= Q(0.37 * 0.37 / (QUAD * BETA_DT * POWER)) * Q(EPS) * larger


def test_scale_factor_failures():
    from athenapk_amd import lib as L
    p = _plan(deck="cluster_magnetic_tower")
    with pytest.raises(L.ApkError) as e:
        p.magnetic_tower_field_to_add(0.0, 0.0, 1e-4, 1.0)
    assert "mt_linear_contrib and mt_quadratic_contrib are both zero" in str(e.value)
    with pytest.raises(L.ApkError) as e:
        p.magnetic_tower_field_to_add(1.0, -1.0, 1.0, 1.0)  # negative discriminant
    assert "No field rate is viable linear_contrib: 1.000000 quadratic_contrib: -1.000000" in str(e.value)
    with pytest.raises(L.ApkError) as e:
        p.magnetic_tower_field_to_add(1.0, 0.0, 1.0, 1.0)  # quad = 0
    assert "No field rate is viable" in str(e.value)
    # still usable
    assert p.magnetic_tower_field_to_add(0.0, 1.0, 1.0, 1.0) == 1.0


# ---- 5. the energy the discrete curl injects --------------------------------------------------------------------------------------------
def _energy_ratio(n):
    t, jc = FB.tower("li", 0.125, li_alpha=20), FB.jet_coords(0.0, 0.0, 0.0, 0.0)
    dx = np.float64(1.0) / n
    x = R.cell_centres(-0.5, dx, 0, n)
    xe = R.cell_centres(-0.5, dx, -1, n + 2)
    _, quad, _, _ = FB.tower_contribs(np.zeros((3, n, n, n)), x, x, x, (dx, dx, dx), t, jc)
    beta_dt_power = 1e-3
    f = FB.field_to_add(0.0, quad, 1.0, beta_dt_power)
    b, _, _ = FB.tower_curl_field(t, jc, f, xe, xe, xe, (dx, dx, dx))
    injected = math.fsum((0.5 * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]) * (dx * dx * dx)).ravel())
    return injected / beta_dt_power


def test_energy_ratio_of_the_discrete_curl_converges():
    """Restatement alone, unit box, li with l_scale = 0.125 and li_alpha = 20, zero initial field: the scale factor is
    sized with the ANALYTIC field's energy, the injected field is the discrete curl of the potential, whose energy is
    lower on a coarse mesh.  Measured ratio injected / (beta_dt P): 0.786 at 16^3 (2 cells per l_scale), 0.940 at 32^3;
    1 - ratio falls by a factor 3.6, at least the factor 3 asked of it (a second-order difference: 4 in the limit).
    The reference's own 1e-2 needs about ten cells per l_scale."""
    r16, r32 = _energy_ratio(16), _energy_ratio(32)
    print("ratio 16^3 %.4f, 32^3 %.4f, (1 - r16) / (1 - r32) = %.3f" % (r16, r32, (1 - r16) / (1 - r32)))
    assert r16 < r32 < 1.0
    assert (1 - r16) >= 3 * (1 - r32)
