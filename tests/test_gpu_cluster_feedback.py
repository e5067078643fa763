"""AGN feedback and the magnetic tower of the cluster problem on the GPU against the numpy restatement
(tests/feedback_reference.py): the thermal sphere's and the jet cylinders' edges, a tilted and precessing jet, the
ceilings, the pressure flag, the tower's source and power contributions, whole cycles of both decks, two ranks.  Strict
build unless stated."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402
import feedback_reference as FB  # noqa: E402
from cluster_cases import assert_two_ranks_equal_one, box as _box, centres as _centres, geom as _geom, mesh as _mesh  # noqa: E402
from cluster_cases import next_dt as _next_dt, random_block as _random_block, read as _read, sim as _sim  # noqa: E402

EPS = np.finfo(np.float64).eps
GAMMA = R.DECK_GAMMA
AGN = "problem/cluster/agn_feedback/"
TOWER = "problem/cluster/magnetic_tower/"
JET = "problem/cluster/precessing_jet/"


# the gravity test's shapes (tests/test_gpu_cluster.py SRC_MESHES)
MESHES = {
    "two_blocks": _mesh((32, 8, 8), (16, 8, 8)) + _box((-0.4, -0.1, -0.1), (0.4, 0.1, 0.1)),
    "odd_block": _mesh((33, 5, 3), (33, 5, 3)) + _box((-0.3, -0.11, -0.07), (0.36, 0.14, 0.05)),
    "centre_at_zero": _mesh(8, 8) + _box((-0.4375,) * 3, (0.5625,) * 3),
    "eight_blocks": _mesh(16, 8) + _box((-0.1,) * 3, (0.1,) * 3),
}


def _inner(g):
    return (slice(g.ng, g.ng + g.mb[2]), slice(g.ng, g.ng + g.mb[1]), slice(g.ng, g.ng + g.mb[0]))


def _random_state(s, fluid, seed, speed=(0.5, 1.0)):
    """a random state written through write_block, built like the gravity test's: rho in [0.5, 1.5], v in [0.5, 1]^3 (or
    `speed`), E in [4, 5], B in [-0.3, 0.3]^3 and psi; FillDerived after it"""
    rng = np.random.default_rng(seed)
    for lb in range(s.info.nblocks_local):
        s.write_block(lb, _random_block(rng, s.block_shape, fluid, speed))
    s.exchange_ghosts()
    s.fill_derived()


def _ns(struct):
    return SimpleNamespace(**{n: getattr(struct, n) for n, _ in struct._fields_})


def _restate_agn(before, g, cfg, jc):
    """the restatement's (u, w, info) of every block, ghost cells as before"""
    inner = _inner(g)
    out = []
    for (u0, w0), loc in zip(before, g.loc):
        xs = _centres(g, loc)
        sl = (slice(None),) + inner
        nh = 9 if u0.shape[0] >= 9 else 5
        u1, w1, info = FB.agn_feedback_src(u0[sl][:nh], w0[sl][:nh], xs[0], xs[1], xs[2], cfg, jc, GAMMA)
        u, w = u0.copy(), w0.copy()
        u[(slice(0, nh),) + inner] = u1
        w[(slice(0, nh),) + inner] = w1
        out.append((u, w, info))
    return out


def _run_agn(mesh, fluid, overrides, strict=True, beta_dt=1e-3, time=0.0, seed=5, prepare=None):
    s = _sim("cluster_agn_feedback", MESHES[mesh] + ["hydro/fluid=" + fluid] + list(overrides), strict=strict)
    s.initialize()
    _random_state(s, fluid, seed)
    if prepare is not None:
        prepare(s)
    before = _read(s)
    cfg, jet = s.agn_feedback_stage_numbers(beta_dt, time)
    s.agn_feedback_src(beta_dt, time)
    after = _read(s)
    g = _geom(s)
    s.close()
    return before, after, g, _ns(cfg), _ns(jet)


# ---- A. inclusive and strict edges ----------------------------------------------------------------------------------------
EDGE_OV = [AGN + "thermal_radius=0.25", AGN + "kinetic_jet_radius=0.25", AGN + "kinetic_jet_offset=0.125",
           AGN + "kinetic_jet_thickness=0.25", JET + "jet_theta=0", JET + "jet_phi0=0"]


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_sphere_and_cylinder_edges(fluid):
    """The 8^3 block with corner -0.4375 and dx = 0.125: centres are exact multiples of 1/8, from -0.375 to 0.5.
    z-aligned jet, thermal_radius = kinetic_jet_radius = 0.25, offset 0.125, thickness 0.25.

    The restatement finds 33 cells in the thermal sphere, six of them exactly on it (r2 == R^2: included, the lone <=);
    and 54 cells in the jet volume, 9 per plane on the 6 planes z = +-0.125, +-0.25, +-0.375 (both ends of |h| inclusive;
    z = 0.5 is outside), SIX of them on the axis with r == 0 -- one per plane; the issue's "eight" cannot go with its own
    54 = 9 x 6 -- and none of the cells at r == 0.25 in those planes (strict <).  With < for the sphere there would be 27.
    These counts are asserted on the restatement first.  Then the conserved state and the stored primitives after
    agn_feedback_src equal the restatement's bit for bit -- every operation is an IEEE product, quotient, sum or root in
    the same order -- and the ghost cells are unchanged."""
    before, after, g, cfg, jc = _run_agn("centre_at_zero", fluid, EDGE_OV)
    assert cfg.thermal_feedback > 0 and cfg.thermal_density > 0 and cfg.jet_density > 0
    (u_want, w_want, info), = _restate_agn(before, g, cfg, jc)
    assert info.sphere.sum() == 33 and info.on_sphere.sum() == 6 and (info.sphere & ~info.on_sphere).sum() == 27
    assert info.jet.sum() == 54 and info.on_axis.sum() == 6
    planes = (np.abs(info.h) >= 0.125) & (np.abs(info.h) <= 0.375)
    assert ((info.r == 0.25) & planes).sum() > 0 and not np.any(info.jet & (info.r == 0.25))
    assert (np.abs(info.h[info.jet]) == 0.125).sum() == 18 and (np.abs(info.h[info.jet]) == 0.375).sum() == 18
    (u1, w1), = after
    assert np.array_equal(u1, u_want)
    assert np.array_equal(w1, w_want)
    inner = _inner(g)
    ghost = np.ones(u1.shape[1:], bool)
    ghost[inner] = False
    assert np.array_equal(u1[:, ghost], before[0][0][:, ghost]) and np.array_equal(w1[:, ghost], before[0][1][:, ghost])
    changed = np.any(u1[(slice(None),) + inner] != before[0][0][(slice(None),) + inner], axis=0)
    assert np.array_equal(changed, info.sphere | info.jet)


# ---- B. tilted and precessing jet -------------------------------------------------------------------------------------------
TILT_OV = [AGN + "thermal_radius=0.09", AGN + "kinetic_jet_radius=0.06", AGN + "kinetic_jet_offset=0.02",
           AGN + "kinetic_jet_thickness=0.2", JET + "jet_theta=0.4", JET + "jet_phi0=1.2", JET + "jet_phi_dot=25.0"]


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("mesh", ["two_blocks", "odd_block"])
def test_tilted_precessing_jet(mesh, fluid):
    """jet_theta = 0.4, jet_phi0 = 1.2, jet_phi_dot = 25, at time 0 and 0.05 (the axis turned by 1.25 rad), random state
    with velocities in [0.5, 1]^3: bit for bit at both times, the set of changed cells differs between them, and the
    product build agrees with the strict one within 1e-12 relative on the changed variables (the gravity test's bound)."""
    sets = []
    for time in (0.0, 0.05):
        before, after, g, cfg, jc = _run_agn(mesh, fluid, TILT_OV, time=time)
        want = _restate_agn(before, g, cfg, jc)
        inner = (slice(None),) + _inner(g)
        changed = []
        for (u1, w1), (u_w, w_w, info), (u0, _) in zip(after, want, before):
            assert np.array_equal(u1, u_w) and np.array_equal(w1, w_w)
            assert info.jet.sum() > 0 and info.sphere.sum() > 0
            changed.append(np.any(u1[inner] != u0[inner], axis=0))
        sets.append(changed)
        _, fast, _, _, _ = _run_agn(mesh, fluid, TILT_OV, strict=False, time=time)
        for (u_f, _), (u_s, _), (u0, _) in zip(fast, after, before):
            m = u_s != u0
            assert np.array_equal(u_f[~m], u_s[~m])
            assert np.all(np.abs(u_f[m] - u_s[m]) <= 1e-12 * np.abs(u_s[m])), np.max(np.abs(u_f[m] / u_s[m] - 1))
    assert any(not np.array_equal(a, b) for a, b in zip(*sets))


# ---- C. ceilings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_ceilings_judge_cells_outside_the_cylinders_by_their_stored_primitives(fluid):
    """vceil = 1.3 and an eceil of 4.5 (Tceil = 4.5 mbar (gamma - 1) / k_B) on the two-block mesh.  After FillDerived the
    conserved state is written AGAIN with another random state, so that the stored primitives (of the first) and the
    current conserved state differ: a cell outside the cylinders is clipped where its STORED speed or internal energy
    exceeds the ceiling, and its momentum is scaled by the stored speed.  The restatement has cells of each kind outside
    the cylinders (and inside); bit for bit."""
    mb_gm1 = 45789051.9600219  # the decks' mbar (gamma - 1) / k_B (tests/test_cluster_feedback_host.py checks it)

    def second_state(s):
        rng = np.random.default_rng(77)
        for lb in range(s.info.nblocks_local):
            s.write_block(lb, _random_block(rng, s.block_shape, fluid))

    ov = TILT_OV + [AGN + "vceil=1.3", AGN + "Tceil=%r" % (4.5 * mb_gm1)]
    before, after, g, cfg, jc = _run_agn("two_blocks", fluid, ov, prepare=second_state)
    assert cfg.vceil == 1.3 and abs(cfg.eceil / 4.5 - 1) < 1e-15
    n_v = n_e = n_v_in = 0
    for (u1, w1), (u_w, w_w, info), (u0, w0) in zip(after, _restate_agn(before, g, cfg, jc), before):
        sl = (slice(None),) + _inner(g)
        assert not np.array_equal(FB.cons_to_prim(u0[sl][:5], GAMMA)[1], w0[sl][1])  # (stored and current do differ)
        n_v += int((info.vceil & ~info.jet).sum())
        n_e += int((info.eceil & ~info.jet).sum())
        n_v_in += int(((info.vceil | info.eceil) & info.jet).sum())
        assert np.array_equal(u1, u_w) and np.array_equal(w1, w_w)
    print("clipped outside the cylinders: %d by vceil, %d by eceil; inside: %d" % (n_v, n_e, n_v_in))
    assert n_v >= 1 and n_e >= 1


# ---- D. non-positive pressure ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_non_positive_pressure_fails_the_step_and_not_the_process():
    """In exact arithmetic the deposit cannot lower the pressure: adding jet_density at the jet's velocity v to gas moving
    at V along the axis raises the internal energy by jet_density rho (v - V)^2 / (2 (rho + jet_density)) plus the jet's
    own.  It vanishes for a cold jet (neither velocity nor temperature given: e_jet = 0) into gas moving at exactly the
    jet's speed -- "fast enough" is V = v -- and then rounding decides: with a pressure of one ulp of E, some jet cells
    end at or below zero (29 of 386 in a first evaluation of the restatement).  The restatement says which (asserted: at least one); a step() then raises the reference's message,
    and the process goes on: the flag is read and cleared, and a fresh simulation steps."""
    from athenapk_amd import decks, driver, lib as L
    deck = decks.load("cluster_agn_feedback")
    line, = [ln for ln in deck.splitlines() if ln.startswith("kinetic_jet_temperature")]
    deck = deck.replace(line + "\n", "")
    ov = MESHES["eight_blocks"] + [AGN + "thermal_fraction=0", AGN + "kinetic_fraction=1", "parthenon/time/integrator=rk1"]
    s = driver.Simulation(deck, ov, strict=True).initialize()
    o = s.agn_feedback_options()
    assert o.assumed_cold_jet == 1 and o.kinetic_jet_e == 0.0
    jc0 = FB.jet_coords(0.4, 0.0, 1.2, 0.0)
    axis = FB.jet_cyl_to_sim_cart_vector(jc0, 0.0, 0.0, 0.0, 0.0, 1.0)
    rng = np.random.default_rng(11)
    for lb in range(s.info.nblocks_local):
        shape = s.block_shape
        u = np.zeros(shape)
        u[0] = rng.uniform(0.5, 1.5, shape[1:])
        for d in range(3):
            u[1 + d] = u[0] * (o.kinetic_jet_velocity * float(axis[d]))
        # (with E = 0 ConsToPrim's pressure is -(gamma - 1) e_k: e_k as it forms it; the pressure is then a few ulps of E)
        e_k = -FB.cons_to_prim(np.concatenate([u[:4], np.zeros((1,) + shape[1:])]), GAMMA)[4] / (np.float64(GAMMA) - 1.0)
        u[4] = e_k * (1 + EPS)
        s.write_block(lb, u)
    s.exchange_ghosts()
    s.fill_derived()
    before = _read(s)
    assert all(np.all(w[4] > 0) for _, w in before)
    dt = _next_dt(s)
    cfg, jet = s.agn_feedback_stage_numbers(dt, 0.0)
    g = _geom(s)
    bad = 0
    for _, w_w, info in _restate_agn(before, g, _ns(cfg), _ns(jet)):
        bad += int((w_w[(4,) + _inner(g)][info.jet] <= 0).sum())
        assert info.jet.sum() > 0
    print("jet cells whose restated final pressure is not positive: %d" % bad)
    assert bad >= 1
    with pytest.raises(L.ApkError) as e:
        s.step()
    assert "Kinetic injection leads to negative pressure" in str(e.value)
    s.close()
    s = _sim("cluster_agn_feedback", MESHES["eight_blocks"]).initialize()
    s.step()
    assert s.ncycle == 1 and np.all(np.isfinite(s.gather("cons")))
    s.close()


# ---- E. the tower's source ---------------------------------------------------------------------------------------------------------
POTENTIALS = {
    "li": [TOWER + "potential_type=li", TOWER + "li_alpha=20", TOWER + "l_scale=0.04", TOWER + "l_mass_scale=0.03"],
    "donut": [TOWER + "potential_type=donut", TOWER + "li_alpha=0", TOWER + "l_scale=0.04", TOWER + "donut_offset=0.01",
              TOWER + "donut_thickness=0.05", TOWER + "l_mass_scale=0.03"],
}
TOWER_BASE = [AGN + "fixed_power=0", TOWER + "initial_field=0", JET + "jet_theta=0.2", JET + "jet_phi0=1"]


def _tower_ns(s):
    t = _ns(s.magnetic_tower_cfg())
    return FB.tower(t.potential, t.l_scale, t.li_alpha, t.donut_offset, t.donut_thickness, t.l_mass_scale)


def _divergence_check(B, a_max, dx):
    c = slice(1, -1)
    div = ((B[0][c, c, 2:] - B[0][c, c, :-2]) / dx[0] / 2.0 + (B[1][c, 2:, c] - B[1][c, :-2, c]) / dx[1] / 2.0 +
           (B[2][2:, c, c] - B[2][:-2, c, c]) / dx[2] / 2.0)
    bound = 64 * EPS * a_max / min(dx) ** 2
    print("max |div b| %.3e, bound %.3e" % (np.max(np.abs(div)), bound))
    assert np.max(np.abs(div)) <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("potential", sorted(POTENTIALS))
@pytest.mark.parametrize("mesh", ["eight_blocks", "odd_block"])
def test_tower_source(mesh, potential):
    """2 x 2 x 2 blocks of 8^3 with nghost = 2 (every cell next to a block face takes potential values from beyond its
    block) and the odd 33 x 5 x 3 block, both potentials, axis tilted by 0.2 and turned by 1, random GLM-MHD state.
    B, E and rho against the restatement: b within 8 eps sum_terms (|A+| + |A-|) / (2 dx_d) + 2 eps |b| (tol_b, the host
    test's), cons B within tol_b + eps |B|, E within |prim_B| tol_b + |b| tol_b summed over the components plus eps |E|
    for the final addition, rho within 4 eps of the added density (one exp, three roundings) plus eps |rho|.  Everything
    else is unchanged bit for bit, field = mass = 0 changes nothing at all, and the central-difference divergence of the
    gathered added field obeys the host test's bound."""
    s = _sim("cluster_magnetic_tower", MESHES[mesh] + TOWER_BASE + POTENTIALS[potential]).initialize()
    _random_state(s, "glmmhd", 9)
    before = _read(s)
    s.magnetic_tower_src(0.0, 0.0, 0.0)
    for (u0, w0), (u1, w1) in zip(before, _read(s)):
        assert np.array_equal(u0, u1) and np.array_equal(w0, w1)
    field, mass = 0.37, 2e-4
    s.magnetic_tower_src(field, mass, 0.0)
    after = _read(s)
    g, t = _geom(s), _tower_ns(s)
    o = s.agn_feedback_options()
    b_gathered = None
    if mesh == "eight_blocks":  # the source once more on a field-free state: the gathered B is then the added field itself
        for lb in range(g.nb):
            u = before[lb][0].copy()
            u[5:9] = 0.0
            s.write_block(lb, u)
        s.fill_derived()
        s.magnetic_tower_src(field, 0.0, 0.0)
        b_gathered = s.gather("cons")[5:8].copy()
    s.close()
    jc = FB.jet_coords(o.jet_theta, o.jet_phi_dot, o.jet_phi0, 0.0)
    inner = _inner(g)
    a_max, worst = 0.0, 0.0
    for (u0, w0), (u1, w1), loc in zip(before, after, g.loc):
        assert np.array_equal(w0, w1)  # the stored primitives
        xe = _centres(g, loc, 1)
        sl = (slice(None),) + inner
        want, b, tb = FB.tower_src(u0[sl], w0[sl], xe[0], xe[1], xe[2], g.dx, t, jc, field, mass)
        _, _, a = FB.tower_curl_field(t, jc, field, xe[0], xe[1], xe[2], g.dx)
        a_max = max(a_max, max(float(np.max(np.abs(c))) for c in a))
        got = u1[sl]
        mask = np.ones(u1.shape, bool)
        for v in (0, 4, 5, 6, 7):
            mask[(v,) + inner] = False
        assert np.array_equal(u1[mask], u0[mask])
        for d in range(3):
            err = np.abs(got[5 + d] - want[5 + d])
            bound = tb[d] + EPS * np.abs(want[5 + d])
            assert np.all(err <= bound), (d, np.max(err - bound))
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        tol_e = sum(np.abs(w0[(5 + d,) + inner]) * tb[d] + np.abs(b[d]) * tb[d] for d in range(3)) + EPS * np.abs(want[4])
        assert np.all(np.abs(got[4] - want[4]) <= tol_e)
        d_rho = want[0] - u0[(0,) + inner]
        # (far from the axis the Gaussian underflows: nothing is added there)
        assert np.all(np.abs(got[0] - want[0]) <= 4 * EPS * np.abs(d_rho) + EPS * np.abs(want[0]))
        assert np.all(d_rho >= 0) and np.any(d_rho > 0)
        assert np.any(b != 0)
    print("%s %s: max err / bound of B %.3f" % (mesh, potential, worst))
    if b_gathered is not None:
        _divergence_check(b_gathered, a_max, g.dx)


# ---- F. the power contributions --------------------------------------------------------------------------------------------------------
def _contribs_case(mb):
    s = _sim("cluster_magnetic_tower", _mesh(16, mb) + _box((-0.1,) * 3, (0.1,) * 3) + TOWER_BASE + POTENTIALS["li"]).initialize()
    # (the same global state whatever the blocks: a smooth function of the global cell index)
    g = _geom(s)
    for lb, loc in enumerate(g.loc):
        u = np.zeros(s.block_shape)
        idx = [np.arange(-g.ng, g.mb[d] + g.ng) + loc[d] * g.mb[d] for d in range(3)]
        I, J, K = np.meshgrid(idx[0], idx[1], idx[2], indexing="ij")
        I, J, K = I.transpose(2, 1, 0), J.transpose(2, 1, 0), K.transpose(2, 1, 0)
        u[0] = 1.0
        u[5], u[6], u[7] = 0.3 * np.sin(0.7 * I + 0.2 * K), 0.2 * np.cos(0.5 * J - 0.3 * I), 0.25 * np.sin(0.4 * K + 0.6 * J)
        u[4] = 3.0
        s.write_block(lb, u)
    s.fill_derived()
    first, second = s.magnetic_tower_contribs(0.0), s.magnetic_tower_contribs(0.0)
    t = _tower_ns(s)
    o = s.agn_feedback_options()
    jc = FB.jet_coords(o.jet_theta, o.jet_phi_dot, o.jet_phi0, 0.0)
    sums = np.zeros(4)
    inner = _inner(g)
    for lb, loc in enumerate(g.loc):
        w = s.read_block(lb, "prim")
        xs = _centres(g, loc)
        sums += np.array(FB.tower_contribs(w[(slice(5, 8),) + inner], xs[0], xs[1], xs[2], g.dx, t, jc))
    s.close()
    return first, second, sums


@pytest.mark.gpu
def test_power_contributions():
    """magnetic_tower_contribs against the restatement's sums within (N + 8) eps sum |t_i|, N = 4096 cells (any order of
    summation, plus each term's exp and products); two calls return identical bits; and the mesh as one block of 16^3
    against the same mesh and state as eight blocks of 8^3, the two totals within the same bound."""
    N = 16 ** 3
    one, one_again, sums1 = _contribs_case(16)
    eight, eight_again, sums8 = _contribs_case(8)
    assert one == one_again and eight == eight_again
    for got, sums in ((one, sums1), (eight, sums8)):
        for q in range(2):
            bound = (N + 8) * EPS * sums[2 + q]
            print("contrib %d: %.17g, restated %.17g, |diff| / bound %.3e" % (q, got[q], sums[q], abs(got[q] - sums[q]) / bound))
            assert abs(got[q] - sums[q]) <= bound
    for q in range(2):
        assert abs(one[q] - eight[q]) <= (N + 8) * EPS * sums1[2 + q]
    assert one[1] > 0 and one[0] != 0


# ---- G. whole cycles of the feedback deck ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["thermal_only", "kinetic_only", "combined"])
def test_whole_cycles_deposit_at_constant_rates(mode):
    """cluster_agn_feedback at 16^3 in 8^3 blocks (riemann = none, tilted axis), 5 cycles.  With the rates of the
    reference's regression analysis -- rho: P f / (eps c^2 V), E: P f / V, M: rho-rate v_jet n sign(h), V the sphere's
    or the two cylinders' volume, n = (sin theta cos phi, sin theta sin phi, cos theta) -- every deposited variable
    equals initial + t * rate within (ncycles + 4) eps |value|, and cells outside the volumes are unchanged bit for bit.
    One exception, in `combined` only, where the sphere contains the cylinders: AddDensityToConsAtFixedVel adds the
    thermal mass AT THE CELL'S VELOCITY, which the jet has made non-zero, so M and E of a cell in both volumes gain
    thermal_density v and 0.5 thermal_density v^2 on top of the constant rates, a physical second-order term the
    regression's 1e-3 tolerance absorbs and this bound does not.  There rho still obeys the law, and M and E are asserted
    to exceed it by less than that term's size, (rho-rate t / rho) of the deposit."""
    tf, kf = {"thermal_only": (1, 0), "kinetic_only": (0, 1), "combined": (0.5, 0.5)}[mode]
    s = _sim("cluster_agn_feedback", MESHES["eight_blocks"] + [AGN + "thermal_fraction=%r" % tf, AGN + "kinetic_fraction=%r" % kf,
                                                               "parthenon/time/cfl=0.01", "parthenon/time/tlim=1.0"])
    s.initialize()
    o = s.agn_feedback_options()
    u0 = s.gather("cons").copy()
    ncycles = 5
    for _ in range(ncycles):
        s.step()
    t, u1 = s.time, s.gather("cons").copy()
    g = _geom(s)
    s.close()
    x = [R.cell_centres(g.xmin[d], g.dx[d], 0, 16) for d in range(3)]
    X, Y, Z = FB.grid(*x)
    jc = FB.jet_coords(o.jet_theta, 0.0, o.jet_phi0, 0.0)
    r, _, _, h = FB.sim_cart_to_jet_cyl(jc, X, Y, Z)
    sphere = (X * X + Y * Y + Z * Z <= o.thermal_radius * o.thermal_radius) & (tf > 0)
    jet = (r < o.kinetic_jet_radius) & (np.abs(h) >= o.kinetic_jet_offset) & \
          (np.abs(h) <= o.kinetic_jet_offset + o.kinetic_jet_thickness) & (kf > 0)
    assert (kf == 0 or jet.sum() > 0) and (tf == 0 or sphere.sum() > 0)
    n = (math.sin(o.jet_theta) * math.cos(o.jet_phi0), math.sin(o.jet_theta) * math.sin(o.jet_phi0), math.cos(o.jet_theta))
    c2 = o.speed_of_light ** 2
    v_sphere = 4.0 / 3.0 * math.pi * o.thermal_radius ** 3
    v_jet = 2 * math.pi * o.kinetic_jet_radius ** 2 * o.kinetic_jet_thickness
    rate = np.zeros_like(u0)
    rate[0] = sphere * (o.fixed_power * o.thermal_fraction / (o.efficiency * c2) / v_sphere) + \
        jet * (o.fixed_power * o.kinetic_fraction / (o.efficiency * c2) / v_jet)
    rho_rate_jet = o.fixed_power * o.kinetic_fraction / (o.efficiency * c2) / v_jet
    for d in range(3):
        rate[1 + d] = jet * np.where(h > 0, 1.0, -1.0) * rho_rate_jet * o.kinetic_jet_velocity * n[d]
    rate[4] = sphere * (o.fixed_power * o.thermal_fraction / v_sphere) + jet * (o.fixed_power * o.kinetic_fraction / v_jet)
    want = u0 + t * rate
    outside = ~(sphere | jet)
    assert np.array_equal(u1[:, outside], u0[:, outside])
    both = sphere & jet
    tol = (ncycles + 4) * EPS * np.abs(want)
    # (the momentum's direction cosines are products of a sine and a cosine here and of the jet frame's four numbers in
    # the kernel: one more rounding each, inside the +4)
    err = np.abs(u1 - want)
    print("%s: t = %.6g, max err / bound outside the overlap %.3f; %d cells in both volumes" %
          (mode, t, np.max((err / np.where(tol > 0, tol, 1))[:, ~both]), both.sum()))
    assert np.all(err[0] <= tol[0])
    assert np.all(err[:, ~both] <= tol[:, ~both])
    if both.any():
        second_order = (rate[0] * t / u0[0]) * np.abs(t * rate)
        assert np.all(err[1:5, both] <= (second_order + tol)[1:5, both])


# ---- H. whole cycles of the tower deck -------------------------------------------------------------------------------------------------------
TOWER_MODES = {
    "power": [],
    "fixed_rate": [AGN + "fixed_power=0", TOWER + "fixed_field_rate=12.431560000204142", TOWER + "fixed_mass_rate=1.765856233359438e-05"],
}
TOWER_CYCLE_OV = MESHES["eight_blocks"] + [TOWER + "l_scale=0.04", TOWER + "l_mass_scale=0.03", "parthenon/time/tlim=1.0"]


def _tower_stage(u, w, g, loc, t, jc, calls):
    """one stage's tower sources on one block's interior: new u and the bound of its E"""
    tol_e = np.zeros(u.shape[1:])
    tol_b = np.zeros((3,) + u.shape[1:])
    xe = _centres(g, loc, 1)
    for field, mass in calls:
        if field == 0 and mass == 0:
            continue
        u, b, tb = FB.tower_src(u, w, xe[0], xe[1], xe[2], g.dx, t, jc, field, mass)
        tol_e += sum(np.abs(w[5 + d]) * tb[d] + np.abs(b[d]) * tb[d] for d in range(3)) + EPS * np.abs(u[4])
        tol_b += tb + EPS * np.abs(u[5:8])
    return u, tol_b, tol_e


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(TOWER_MODES))
def test_tower_cycles_against_the_restatement(mode):
    """cluster_magnetic_tower at 16^3 in 8^3 blocks (l_scale of a few cells), 3 VL2 cycles, the power-scaled and the
    fixed-rate mode, cycle for cycle: each cycle is restated from the state the driver held before it -- the two sums
    of the power scaling as the driver reduces them (magnetic_tower_contribs; test_power_contributions bounds them),
    field_to_add for beta_dt = dt / 2 and dt, the predictor's source on the state, ConsToPrim, the corrector's source on
    the same state -- and B, E, rho must agree within the propagated bound of the tower source test, summed over the calls
    that touch them.  The field in the energy term is the STORED primitive one: in the fixed-rate mode the corrector reads
    what the predictor's FillDerived left, the half-step field; in the power mode AGNFeedback::FeedbackSrcTerm has just
    run its closing ConsToPrim on the stage's own input (agn_feedback.cpp:406, every cell, whenever the power is not
    zero), so both stages read the field of the state they update."""
    s = _sim("cluster_magnetic_tower", TOWER_CYCLE_OV + TOWER_MODES[mode]).initialize()
    o, t, g = s.agn_feedback_options(), _tower_ns(s), _geom(s)
    jc = FB.jet_coords(o.jet_theta, o.jet_phi_dot, o.jet_phi0, 0.0)
    inner = (slice(None),) + _inner(g)
    assert (o.tower_power_scaling == 1) == (mode == "power")
    for cycle in range(3):
        before = _read(s)
        lin, quad = s.magnetic_tower_contribs() if mode == "power" else (0.0, 0.0)
        dt = _next_dt(s)
        s.step()
        after = _read(s)
        for (u0, w0), (u1, _), loc in zip(before, after, g.loc):
            stage_w, tol_b_prev = w0[inner], 0.0
            for beta_dt in (0.5 * dt, dt):
                calls = []
                if mode == "power":
                    calls.append((FB.field_to_add(lin, quad, beta_dt, o.power * o.magnetic_fraction),
                                  o.mass_rate * o.magnetic_mass_fraction * beta_dt))
                else:
                    calls.append((o.fixed_field_rate * beta_dt, o.fixed_mass_rate * beta_dt))
                if mode == "power":
                    stage_w, tol_b_prev = FB.cons_to_prim(u0[inner], GAMMA), 0.0
                u, tol_b, tol_e = _tower_stage(u0[inner], stage_w, g, loc, t, jc, calls)
                # (the corrector's energy term reads the predictor's stored field, which carries the predictor's bound)
                b_added = u[5:8] - u0[inner][5:8]
                tol_e = tol_e + sum(np.abs(b_added[d]) * tol_b_prev for d in range(3)) if np.ndim(tol_b_prev) else tol_e
                stage_w = FB.cons_to_prim(u, GAMMA)
                tol_b_prev = tol_b
            got = u1[inner]
            assert np.all(np.abs(got[5:8] - u[5:8]) <= tol_b), cycle
            assert np.all(np.abs(got[4] - u[4]) <= tol_e), cycle
            assert np.all(np.abs(got[0] - u[0]) <= 8 * EPS * np.abs(u[0])), cycle
            assert np.array_equal(got[1:4], u0[inner][1:4]) and np.array_equal(got[8], u0[inner][8])
            # (far from the axis the Gaussian density underflows against rho)
            assert np.any(got[5:8] != u0[inner][5:8]) and np.all(got[0] >= u0[inner][0]) and np.any(got[0] > u0[inner][0])
    s.close()


@pytest.mark.gpu
def test_gravity_then_feedback_then_tower_power_then_tower_fixed(gpu_ctx_strict):
    """The order of ClusterUnsplitSrcTerm (cluster.cpp:63-84), in the style of the cooling-then-gravity test: the tower
    deck with the static field of an SMBH + BCG, a kinetic and a magnetic share of the power and a fixed field rate on
    top, rk1 (a cycle IS a stage), riemann = none (the fluxes vanish, Dedner's source acts on psi = 0).  One cycle is
    assembled from the entry points on the state the driver held before it: gravity, then AGN feedback, then the tower
    with the power-scaled field, then the tower with the fixed rate -- and equals the driver's bit for bit on every
    interior cell.  Feedback before gravity does not (gravity reads the stored density and velocity, which feedback's
    closing ConsToPrim has replaced), and neither does the power-scaled tower before feedback (that ConsToPrim then stores
    the tower's field, which the fixed-rate call's energy term reads)."""
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    ctx = gpu_ctx_strict
    ov = TOWER_CYCLE_OV + ["parthenon/time/integrator=rk1", "problem/cluster/gravity/gravity_srcterm=true",
                           "problem/cluster/gravity/include_smbh_g=true", "problem/cluster/gravity/which_bcg_g=HERNQUIST",
                           "problem/cluster/gravity/g_smoothing_radius=1e-3",
                           AGN + "kinetic_fraction=1", AGN + "kinetic_jet_radius=0.05", AGN + "kinetic_jet_thickness=0.05",
                           AGN + "kinetic_jet_offset=0.01", TOWER + "fixed_field_rate=12.431560000204142",
                           TOWER + "fixed_mass_rate=1.765856233359438e-05",
                           "problem/cluster/uniform_gas/ux=0.3", "problem/cluster/uniform_gas/uy=-0.2",
                           "problem/cluster/uniform_gas/uz=0.1"]
    s = _sim("cluster_magnetic_tower", ov).initialize()
    o, g = s.agn_feedback_options(), _geom(s)
    assert o.tower_power_scaling == 1 and o.kinetic_fraction == 0.5 and o.fixed_field_rate != 0
    nb, ng, mb, dx = g.nb, g.ng, g.mb, g.dx
    grav, tower, eos = s.cluster_options().gravity, s.magnetic_tower_cfg(), L.make_eos(GAMMA)
    corners = np.array([[g.xmin[d] + float(loc[d] * mb[d]) * dx[d] for d in range(3)] for loc in g.loc] + [list(g.xmin)])
    inner = (slice(None), slice(None)) + _inner(g)
    u = np.stack([s.read_block(lb, "cons") for lb in range(nb)])
    w = np.stack([s.read_block(lb, "prim") for lb in range(nb)])
    lin, quad = s.magnetic_tower_contribs()
    dt = _next_dt(s)
    s.step()
    got = np.stack([s.read_block(lb, "cons") for lb in range(nb)])
    s.close()
    cfg, jet = L.AgnFeedbackCfg(), L.JetCoords()
    want_cfg = FB.stage_numbers(SimpleNamespace(**{k: getattr(o, k) for k in (
        "thermal_fraction", "kinetic_fraction", "thermal_mass_fraction", "kinetic_mass_fraction", "power", "mass_rate",
        "thermal_radius", "kinetic_jet_radius", "kinetic_jet_thickness", "kinetic_jet_offset", "kinetic_jet_velocity",
        "vceil", "eceil")}), dt)
    for name, _ in cfg._fields_:
        setattr(cfg, name, getattr(want_cfg, name))
    jc = FB.jet_coords(o.jet_theta, o.jet_phi_dot, o.jet_phi0, 0.0)
    for name, _ in jet._fields_:
        setattr(jet, name, float(getattr(jc, name)))
    f_power = FB.field_to_add(lin, quad, dt, o.power * o.magnetic_fraction)
    m_power = o.mass_rate * o.magnetic_mass_fraction * dt

    def gravity(md):
        hydro.GravitationalFieldSrcTerm(md, grav, corners, dt)

    def feedback(md):
        hydro.AgnFeedbackSrcTerm(md, "glmmhd", eos, cfg, jet, corners)

    def tower_power(md):
        hydro.MagneticTowerSrcTerm(md, tower, jet, corners, f_power, m_power)

    def tower_fixed(md):
        hydro.MagneticTowerSrcTerm(md, tower, jet, corners, o.fixed_field_rate * dt, o.fixed_mass_rate * dt)

    results = {}
    for name, order in (("reference", (gravity, feedback, tower_power, tower_fixed)),
                        ("feedback_first", (feedback, gravity, tower_power, tower_fixed)),
                        ("tower_first", (tower_power, gravity, feedback, tower_fixed))):
        md = hydro.MeshData(ctx, mb, ng, 9, dx=dx, nblocks=nb, cons=u, prim=w, with_flux=False)
        for src in order:
            src(md)
        results[name] = md.cons_host()[inner]
    assert np.array_equal(results["reference"], got[inner])
    assert not np.array_equal(results["feedback_first"], got[inner])
    assert not np.array_equal(results["tower_first"], got[inner])


# ---- I. two ranks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_equal_one_in_power_mode(tmp_path):
    """the tower deck in power mode at 16^3 in 8^3 blocks, 2 cycles, two ranks sharing the GPU (gloo): every block equals
    the one-rank run's bit for bit -- the scale factor comes from sums whose slots are added in global block order,
    whatever the distribution of the blocks"""
    assert_two_ranks_equal_one(tmp_path, "cluster_magnetic_tower", TOWER_CYCLE_OV, 2)
