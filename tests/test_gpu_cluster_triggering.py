"""AGN triggering of the cluster problem on the GPU against the numpy restatement (tests/triggering_reference.py): the
Bondi sums, the strict edge of the sphere, the inclusive temperature threshold, the cold-gas and the Bondi removal on
every cell of a block (ghost cells included), whole cycles of the new deck in each mode, the coupling to the feedback
source, two ranks, and a sphere that holds no cell.  Strict build throughout."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402
import feedback_reference as FB  # noqa: E402
import triggering_reference as TR  # noqa: E402
from cluster_cases import assert_two_ranks_equal_one, box as _box, centres as _centres, geom as _geom, mesh as _mesh  # noqa: E402
from cluster_cases import next_dt as _next_dt, random_block as _random_block, read as _read, sim as _deck_sim  # noqa: E402

EPS = np.finfo(np.float64).eps
GAMMA = R.DECK_GAMMA
TRIG = "problem/cluster/agn_triggering/"
AGN = "problem/cluster/agn_feedback/"
DECK = "cluster_agn_triggering"


# the feedback test's shapes (tests/test_gpu_cluster_feedback.py MESHES), each with an accretion radius of a few cells:
# eight_blocks -- dx = 0.0125, radius 2.4 cells, the sphere lies in all eight blocks and in their ghost cells;
# one_block -- the same mesh as a single block; odd_block -- dx = (0.02, 0.05, 0.04), the radius reaches the x3 ghost
# cells (centres at +-0.07 ... ) of the 33 x 5 x 3 block; centre_at_zero -- centres are exact multiples of 1/8
MESHES = {
    "eight_blocks": _mesh(16, 8) + _box((-0.1,) * 3, (0.1,) * 3) + [TRIG + "accretion_radius=0.03"],
    "one_block": _mesh(16, 16) + _box((-0.1,) * 3, (0.1,) * 3) + [TRIG + "accretion_radius=0.03"],
    "odd_block": _mesh((33, 5, 3), (33, 5, 3)) + _box((-0.3, -0.11, -0.07), (0.36, 0.14, 0.05)) + [TRIG + "accretion_radius=0.08"],
    "centre_at_zero": _mesh(8, 8) + _box((-0.4375,) * 3, (0.5625,) * 3) + [TRIG + "accretion_radius=0.25"],
}


def _sim(overrides, strict=True, **kw):
    return _deck_sim(DECK, overrides, strict=strict, **kw)


def _interior_mask(g):
    m = np.zeros((g.mb[2] + 2 * g.ng, g.mb[1] + 2 * g.ng, g.mb[0] + 2 * g.ng), bool)
    m[g.ng:g.ng + g.mb[2], g.ng:g.ng + g.mb[1], g.ng:g.ng + g.mb[0]] = True
    return m


def _spheres(g, radius):
    """per block the [k][j][i] mask of the extended cells with r2 < R^2"""
    return [TR.sphere(*_centres(g, loc, g.ng), radius) for loc in g.loc]


def _random_sim(mesh, fluid, overrides=(), seed=5, strict=True):
    s = _sim(MESHES[mesh] + ["hydro/fluid=" + fluid] + list(overrides), strict=strict).initialize()
    rng = np.random.default_rng(seed)
    for lb in range(s.info.nblocks_local):
        s.write_block(lb, _random_block(rng, s.block_shape, fluid))
    s.exchange_ghosts()
    s.fill_derived()
    return s


def _bondi_sums(state, g, masks):
    """the restatement's four sums over the interior cells of the sphere, with sum |t_i| and the number of cells"""
    inner = _interior_mask(g)
    terms = [TR.bondi_terms(w, m & inner, g.vol, GAMMA) for (_, w), m in zip(state, masks)]
    t = np.concatenate(terms, axis=1)
    return t.sum(axis=1), np.abs(t).sum(axis=1), t.shape[1]


def _state_sums(st):
    return np.array([st.total_mass, st.mass_weighted_density, st.mass_weighted_velocity, st.mass_weighted_cs])


def _model(s):
    o = s.agn_triggering_options()
    return TR.model(o.mode, accretion_radius=o.accretion_radius, cold_temp_thresh=o.cold_temp_thresh, cold_t_acc=o.cold_t_acc,
                    bondi_alpha=o.bondi_alpha, bondi_M_smbh=o.bondi_M_smbh, bondi_n0=o.bondi_n0, bondi_beta=o.bondi_beta,
                    accretion_cfl=o.accretion_cfl, mean_molecular_mass=o.mean_molecular_mass,
                    gravitational_constant=o.gravitational_constant)


# ---- A. the Bondi sums --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_bondi_reduce(fluid):
    """Random state on eight 8^3 blocks and the same state on one 16^3 block.  Each of the four sums agrees with the
    restatement's within (N + 8) eps sum |t_i|, N the cells in the sphere: any order of adding N numbers stays within
    (N - 1) eps sum |t_i| of the exact sum, on both sides, and a term carries at most 4 roundings more (the tower
    contributions' bound).  Two calls give identical bits; one block against eight within the same bound; the reduction
    leaves the state alone."""
    ov = [TRIG + "triggering_mode=BOOSTED_BONDI"]
    s = _random_sim("eight_blocks", fluid, ov)
    g, before = _geom(s), _read(s)
    radius = s.agn_triggering_options().accretion_radius
    want, mag, n = _bondi_sums(before, g, _spheres(g, radius))
    first = _state_sums(s.agn_triggering_reduce(1e-3))
    second = _state_sums(s.agn_triggering_reduce(1e-3))
    for (u0, w0), (u1, w1) in zip(before, _read(s)):
        assert np.array_equal(u0, u1) and np.array_equal(w0, w1)
    glob = s.gather("cons")
    s.close()
    bound = (n + 8) * EPS * mag
    print("cells in the sphere %d, errors / bound %s" % (n, np.abs(first - want) / bound))
    assert n > 30 and np.all(want > 0)
    assert np.array_equal(first, second)
    assert np.all(np.abs(first - want) <= bound)

    one = _sim(MESHES["one_block"] + ["hydro/fluid=" + fluid] + ov).initialize()
    ng = one.info.ng
    u = np.ones(one.block_shape)
    u[:, ng:-ng, ng:-ng, ng:-ng] = glob
    one.write_block(0, u)
    one.exchange_ghosts()
    one.fill_derived()
    g1 = _geom(one)
    want1, _, n1 = _bondi_sums(_read(one), g1, _spheres(g1, radius))
    got1 = _state_sums(one.agn_triggering_reduce(1e-3))
    assert one.agn_triggering_options().active_blocks == 1
    one.close()
    assert n1 == n and np.all(np.abs(got1 - want1) <= bound) and np.all(np.abs(got1 - first) <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_bondi_sums_in_the_shared_order(fluid):
    """The order of the additions, which the bound of test_bondi_reduce cannot see.  One 16^3 block on +-0.1 with
    accretion_radius = 0.3: every cell, ghost cells included, lies inside the sphere (the farthest centre is at
    sqrt(3) (0.1 + (ng - 1/2) dx) < 0.25), so the active box is the block's whole arrays, (16 + 2 ng)^3 > 4096 cells: two or
    more workgroups share it.  The four sums equal TR.block_sum of the restated terms in array order, zero on ghost cells,
    bit for bit (strict build; a skipped cell and an added zero are the same bits)."""
    s = _random_sim("one_block", fluid, [TRIG + "triggering_mode=BOOSTED_BONDI", TRIG + "accretion_radius=0.3"])
    g, o, ((_, w),) = _geom(s), s.agn_triggering_options(), _read(s)
    got = _state_sums(s.agn_triggering_reduce(1e-3))
    s.close()
    ncell = (16 + 2 * g.ng) ** 3
    assert _spheres(g, o.accretion_radius)[0].all() and o.active_blocks == 1 and o.active_box_cells == ncell
    P = TR.block_sum_groups(o.active_box_cells)
    assert P >= 2
    terms = TR.bondi_terms(w, np.ones(w.shape[1:], bool), g.vol, GAMMA)
    want = TR.block_sum(np.where(_interior_mask(g).ravel(), terms, 0.0), P)
    print("P = %d, device %s, restated %s" % (P, got, want))
    assert np.array_equal(got, want)


# ---- B. the strict edge ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_sphere_is_strict():
    """The 8^3 block with corner -0.4375 and dx = 0.125, accretion_radius = 0.25: the cell centred at (0.25, 0, 0) has r2 ==
    R^2 exactly and is left out; a radius one ulp larger takes it in.  Seen in the removal (the cells it changes are the
    restatement's mask, bit for bit) and in the total mass (the two sums differ by that cell's and its five likes' mass)."""
    changed, masses = [], []
    for radius in (0.25, float(np.nextafter(0.25, 1.0))):
        s = _random_sim("centre_at_zero", "euler", [TRIG + "triggering_mode=BOOSTED_BONDI", TRIG + "accretion_radius=%r" % radius,
                                                    "problem/cluster/gravity/m_smbh=0.3"])  # (removes about 1 % in 1e-3)
        g, before = _geom(s), _read(s)
        mask, = _spheres(g, radius)
        xs = _centres(g, g.loc[0], g.ng)
        i, j, k = (int(np.nonzero(xs[0] == 0.25)[0][0]), int(np.nonzero(xs[1] == 0.0)[0][0]), int(np.nonzero(xs[2] == 0.0)[0][0]))
        on = (radius == 0.25)
        assert mask[k, j, i] == (not on)
        st = s.agn_triggering_reduce(1e-3)
        want, mag, n = _bondi_sums(before, g, [mask])
        assert np.all(np.abs(_state_sums(st) - want) <= (n + 8) * EPS * mag)
        s.agn_triggering_remove_bondi(1e-3)
        (u1, w1), = _read(s)
        s.close()
        u0, w0 = before[0]
        u_want, w_want = TR.add_density_fixed_vel_temp(u0, w0, mask, TR.bondi_delta(w0, st.total_mass, st.accretion_rate, 1e-3), GAMMA)
        assert np.array_equal(u1, u_want) and np.array_equal(w1, w_want)
        assert np.array_equal(np.any(u1 != u0, axis=0), mask)
        changed.append(int(mask.sum()))
        masses.append(st.total_mass)
    # 27 + 6 cells: the six at distance exactly 0.25 along the axes
    assert changed == [27, 33] and masses[1] > masses[0]


# ---- C. the inclusive threshold -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_cold_threshold_is_inclusive():
    """cold_temp_thresh set to the restated temperature of one chosen interior cell of the sphere: that cell is cold (<=),
    and a threshold one ulp lower leaves it out -- in the mass (it differs by the cell's) and in the removal."""
    base = [TRIG + "triggering_mode=COLD_GAS"]
    s = _random_sim("eight_blocks", "euler", base)
    g, state = _geom(s), _read(s)
    o = s.agn_triggering_options()
    s.close()
    masks, inner = _spheres(g, o.accretion_radius), _interior_mask(g)
    temps = [TR.temperature(w, o.mean_molecular_mass_by_kb) for _, w in state]
    cand = np.argwhere(masks[0] & inner)
    k, j, i = cand[len(cand) // 2]
    thresh = float(temps[0][k, j, i])
    got = []
    for th in (thresh, float(np.nextafter(thresh, 0.0))):
        s = _random_sim("eight_blocks", "euler", base + [TRIG + "cold_temp_thresh=%r" % th])
        before = _read(s)
        assert np.array_equal(before[0][1], state[0][1])
        st = s.agn_triggering_reduce(1e-3)
        after = _read(s)
        s.close()
        cold = [TR.cold_mask(w, m, o.mean_molecular_mass_by_kb, th) for (_, w), m in zip(before, masks)]
        assert cold[0][k, j, i] == (th == thresh)
        terms = np.concatenate([(w[0] * g.vol)[c & inner] for (_, w), c in zip(before, cold)])
        assert abs(st.cold_mass - terms.sum()) <= (len(terms) + 8) * EPS * terms.sum()
        assert (after[0][0][0, k, j, i] != before[0][0][0, k, j, i]) == (th == thresh)
        got.append((st.cold_mass, len(terms)))
    cell_mass = state[0][1][0, k, j, i] * g.vol
    assert got[0][1] == got[1][1] + 1 and abs((got[0][0] - got[1][0]) - cell_mass) <= 2 * (got[0][1] + 8) * EPS * got[0][0]


# ---- D. the cold removal ----------------------------------------------------------------------------------------------------------
def _median_threshold(mesh, fluid):
    s = _random_sim(mesh, fluid, [TRIG + "triggering_mode=COLD_GAS"])
    g, o = _geom(s), s.agn_triggering_options()
    temps = np.concatenate([TR.temperature(w, o.mean_molecular_mass_by_kb)[m]
                            for (_, w), m in zip(_read(s), _spheres(g, o.accretion_radius))])
    s.close()
    return float(np.median(temps))


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("mesh", ["odd_block", "eight_blocks"])
def test_cold_removal(mesh, fluid):
    """cold_temp_thresh = the median temperature inside the sphere, dt = 3e-3 (3 % of the cold gas).  Conserved state and
    stored primitives of EVERY cell, ghost cells included, equal the restatement's bit for bit; cells outside the sphere or
    above the threshold are unchanged bit for bit; on eight blocks the ghost cells equal the neighbour's interior cells
    after the call (an exchange and FillDerived change no bit); with removed_accreted_mass = false the state is untouched
    and the sum is the same bits."""
    dt = 3e-3
    ov = [TRIG + "triggering_mode=COLD_GAS", TRIG + "cold_temp_thresh=%r" % _median_threshold(mesh, fluid)]
    s = _random_sim(mesh, fluid, ov)
    g, o, before = _geom(s), s.agn_triggering_options(), _read(s)
    st = s.agn_triggering_reduce(dt)
    after = _read(s)
    inner, n_cold, n_ghost, mass = _interior_mask(g), 0, 0, []
    for (u0, w0), (u1, w1), m in zip(before, after, _spheres(g, o.accretion_radius)):
        cold = TR.cold_mask(w0, m, o.mean_molecular_mass_by_kb, o.cold_temp_thresh)
        u_want, w_want = TR.add_density_fixed_vel_temp(u0, w0, cold, TR.cold_delta(w0, o.cold_t_acc, dt), GAMMA)
        assert np.array_equal(u1, u_want) and np.array_equal(w1, w_want)
        assert np.array_equal(u1[:, ~cold], u0[:, ~cold]) and np.array_equal(w1[:, ~cold], w0[:, ~cold])
        assert np.all(u1[0][cold] < u0[0][cold])
        n_cold += int((cold & inner).sum())
        n_ghost += int((cold & ~inner).sum())
        mass.append((w0[0] * g.vol)[cold & inner])
    mass = np.concatenate(mass)
    print("cold cells: %d interior, %d ghost" % (n_cold, n_ghost))
    assert n_cold >= 4 and n_ghost >= 1
    assert abs(st.cold_mass - mass.sum()) <= (len(mass) + 8) * EPS * mass.sum()
    assert st.accretion_rate == st.cold_mass / o.cold_t_acc
    if mesh == "eight_blocks":
        s.exchange_ghosts()
        s.fill_derived()
        for (u1, w1), (u2, w2) in zip(after, _read(s)):
            assert np.array_equal(u1, u2) and np.array_equal(w1, w2)
    s.close()
    s = _random_sim(mesh, fluid, ov + [TRIG + "removed_accreted_mass=false"])
    st2 = s.agn_triggering_reduce(dt)
    for (u0, w0), (u1, w1) in zip(before, _read(s)):
        assert np.array_equal(u0, u1) and np.array_equal(w0, w1)
    s.close()
    assert st2.cold_mass == st.cold_mass


# ---- E. the Bondi removal ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("mesh", ["odd_block", "eight_blocks"])
def test_bondi_removal(mesh, fluid):
    """delta = -rho / total_mass * accretion_rate * dt with the reduced total mass and its rate (the black hole's mass is
    raised so that a step of 1e-3 removes a few per cent): every cell of every block, ghost cells included, bit for bit;
    outside the sphere nothing changes; on eight blocks the ghost cells equal the neighbours' interior cells afterwards."""
    dt = 1e-3
    s = _random_sim(mesh, fluid, [TRIG + "triggering_mode=BOOSTED_BONDI", "problem/cluster/gravity/m_smbh=0.3", TRIG + "bondi_alpha=1"])
    g, o, before = _geom(s), s.agn_triggering_options(), _read(s)
    st = s.agn_triggering_reduce(dt)
    frac = st.accretion_rate * dt / st.total_mass
    print("fraction removed: %.3e" % frac)
    assert 1e-3 < frac < 0.5
    s.agn_triggering_remove_bondi(dt)
    after = _read(s)
    n_ghost = 0
    for (u0, w0), (u1, w1), m in zip(before, after, _spheres(g, o.accretion_radius)):
        u_want, w_want = TR.add_density_fixed_vel_temp(u0, w0, m, TR.bondi_delta(w0, st.total_mass, st.accretion_rate, dt), GAMMA)
        assert np.array_equal(u1, u_want) and np.array_equal(w1, w_want)
        assert np.array_equal(u1[:, ~m], u0[:, ~m]) and np.array_equal(w1[:, ~m], w0[:, ~m])
        assert np.all(u1[0][m] < u0[0][m])
        n_ghost += int((m & ~_interior_mask(g)).sum())
    assert n_ghost >= 1
    if mesh == "eight_blocks":
        s.exchange_ghosts()
        s.fill_derived()
        for (u1, w1), (u2, w2) in zip(after, _read(s)):
            assert np.array_equal(u1, u2) and np.array_equal(w1, w2)
    s.close()


@pytest.mark.gpu
def test_product_build_stays_close():
    """the product build (FMA contraction, reciprocal-based divides and roots) compiles the same source: sums and the
    state after the Bondi removal within 1e-12 relative of the strict build's on eight GLM-MHD blocks (the bound the
    gravity and feedback tests use for the product build); cells outside the sphere keep their bits"""
    ov = [TRIG + "triggering_mode=BOOSTED_BONDI", "problem/cluster/gravity/m_smbh=0.3", TRIG + "bondi_alpha=1"]
    out = {}
    for strict in (True, False):
        s = _random_sim("eight_blocks", "glmmhd", ov, strict=strict)
        before = _read(s)
        st = s.agn_triggering_reduce(1e-3)
        s.agn_triggering_remove_bondi(1e-3)
        out[strict] = (before, _state_sums(st), st.accretion_rate, _read(s))
        s.close()
    assert np.all(np.abs(out[False][1] - out[True][1]) <= 1e-12 * out[True][1])
    assert abs(out[False][2] - out[True][2]) <= 1e-12 * out[True][2]
    for (u0, _), (u_s, w_s), (u_f, w_f) in zip(out[True][0], out[True][3], out[False][3]):
        changed = u_s != u0
        assert changed.any() and np.array_equal(u_f[~changed], u_s[~changed])
        assert np.all(np.abs(u_f - u_s) <= 1e-12 * np.abs(u_s)) and np.all(np.abs(w_f[:5] - w_s[:5]) <= 1e-12 * np.abs(w_s[:5]))


# ---- F. whole cycles of the deck ----------------------------------------------------------------------------------------------------
CYCLE_OV = _mesh(16, 8) + ["parthenon/time/tlim=10.0", "parthenon/time/nlim=5", TRIG + "accretion_radius=0.03"]
NCYCLES = 5
# the hydro limit is cfl * 0.905 here (dx / (|v| + c_s)): it sets the first Bondi cycle, which must not remove so much that
# 1 - x cancels (M / mdot of the 30 kpc sphere: BOOSTED_BONDI 2.0, BOOTH_SCHAYE 0.51 -- the first cycle then removes 13 %
# and 18 %), and must stay above the triggering limit, a tenth of M / mdot, which the second cycle meets
CYCLE_CFL = {"COLD_GAS": 0.1, "BOOSTED_BONDI": 0.3, "BOOTH_SCHAYE": 0.1}


def _rate_bound(mode, n):
    """The accretion rate from sums that each carry a relative error of d = (N + 8) eps (all terms are positive).  COLD_GAS:
    d and one quotient.  Bondi-like: rho = S1 / S0 carries 2 d; v and cs carry 2 d each and enter through (v^2 + cs^2)^(3/2),
    at most 3 times 2 d together; BOOTH_SCHAYE's alpha = (n / n0)^2 doubles rho's 2 d once more.  Plus the model's own
    roundings (30 eps, tests/test_cluster_triggering_host.py)."""
    d = (n + 8) * EPS
    return {"COLD_GAS": d + 2 * EPS, "BOOSTED_BONDI": 8 * d + 30 * EPS, "BOOTH_SCHAYE": 12 * d + 30 * EPS}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["COLD_GAS", "BOOSTED_BONDI", "BOOTH_SCHAYE"])
def test_cycles_of_the_deck(mode, tmp_path):
    """inputs/cluster_agn_triggering.in at 16^3 in 8^3 blocks (radius 2.4 cells), 5 VL2 cycles with riemann = none.
    Cycle for cycle the recorded accretion rate is the formula on the restated sums of the state before the cycle, within
    the reduce bound propagated through the formula (_rate_bound).
    After the run, inside the sphere rho = rho0 prod(1 - dt_i mdot_i / M_i) (cold gas: prod(1 - dt_i / t_acc)) within
    8 ncycles eps: per cycle the kernel rounds the quotient, the two products and the sum (4; the first three scaled by
    |delta / rho| < 1), the expectation its product, quotient, difference and the running product (4).  The velocity is
    unchanged within 9 ncycles eps (momentum: product and sum; ConsToPrim: reciprocal and product; and the density's 4 + 1),
    p / rho within 20 ncycles eps (the energy's increment: 8; ConsToPrim's kinetic energy is 1e-3 of E, its 8 roundings
    count as 1; difference, product, quotient: 3; the density's 4; E / (E - e_k) < 1.01 leaves room).  Cells outside the
    sphere keep every bit.  COLD_GAS: every dt is accretion_cfl * cold_t_acc exactly (the hydro limit is nine times
    larger).  Bondi-like: the first cycle has no triggering limit, the second's dt is accretion_cfl * M / mdot of the
    first's sums.  The rows execute() writes to triggering_filename are the accessor's values digit for digit."""
    ov = CYCLE_OV + [TRIG + "triggering_mode=" + mode, "parthenon/time/cfl=%r" % CYCLE_CFL[mode]]
    s = _sim(ov).initialize()
    g, o, m = _geom(s), s.agn_triggering_options(), _model(s)
    masks, inner = _spheres(g, o.accretion_radius), _interior_mask(g)
    start = _read(s)
    assert s.agn_triggering_state().accretion_rate == 0.0
    if mode != "COLD_GAS":
        assert s.agn_triggering_state().dt_limit == sys.float_info.max
    rows, factor = [], 1.0
    for cycle in range(NCYCLES):
        before = _read(s)
        dt, t0 = _next_dt(s), s.time
        s.step()
        st = s.agn_triggering_state()
        assert st.dt == dt and st.time == t0
        if mode == "COLD_GAS":
            cold = [TR.cold_mask(w, mk & inner, o.mean_molecular_mass_by_kb, o.cold_temp_thresh) for (_, w), mk in zip(before, masks)]
            terms = np.concatenate([(w[0] * g.vol)[c] for (_, w), c in zip(before, cold)])
            n = len(terms)
            assert n == sum(int((mk & inner).sum()) for mk in masks)  # (the whole sphere is cold)
            want = TR.accretion_rate(m, terms.sum())
            assert dt == 0.1 * 0.1
            factor *= 1 - dt / o.cold_t_acc
            rows.append((st.time, st.dt, st.accretion_rate, st.cold_mass))
        else:
            sums, _, n = _bondi_sums(before, g, masks)
            want = TR.accretion_rate(m, sums)
            factor *= 1 - dt * st.accretion_rate / st.total_mass
            if cycle == 0:
                assert st.dt_limit < dt  # (the first cycle ran without the limit it would have had)
                assert abs(st.dt_limit - o.accretion_cfl * st.total_mass / st.accretion_rate) <= 2 * EPS * st.dt_limit
                assert s.dt == st.dt_limit
            rows.append((st.time, st.dt, st.accretion_rate, st.total_mass, st.mass_weighted_density / st.total_mass,
                         st.mass_weighted_velocity / st.total_mass, st.mass_weighted_cs / st.total_mass))
        print("cycle %d: dt %.6e rate %.17g restated %.17g (%.2f of the bound)" %
              (cycle, dt, st.accretion_rate, want, abs(st.accretion_rate / want - 1) / _rate_bound(mode, n)))
        assert n > 30 and abs(st.accretion_rate - want) <= _rate_bound(mode, n) * want
    end = _read(s)
    s.close()
    assert 0 < factor < 0.97
    for (u0, w0), (u1, w1), mk in zip(start, end, masks):
        mi = mk & inner
        assert np.array_equal(u1[:, ~mk & inner], u0[:, ~mk & inner]) and np.array_equal(w1[:, ~mk & inner], w0[:, ~mk & inner])
        assert np.all(np.abs(w1[0][mi] - w0[0][mi] * factor) <= 8 * NCYCLES * EPS * w0[0][mi] * factor)
        assert np.array_equal(w1[0][mi], u1[0][mi])
        for n_ in (1, 2, 3):
            assert np.all(np.abs(w1[n_][mi] - w0[n_][mi]) <= 9 * NCYCLES * EPS * np.abs(w0[n_][mi]))
        t0, t1 = w0[4][mi] / w0[0][mi], w1[4][mi] / w1[0][mi]
        assert np.all(np.abs(t1 - t0) <= 20 * NCYCLES * EPS * t0)
    # the file execute() writes
    s = _sim(ov)
    assert s.execute(str(tmp_path)) == NCYCLES
    s.close()
    data = np.loadtxt(os.path.join(str(tmp_path), "agn_triggering.dat"), ndmin=2)
    assert data.shape == (NCYCLES, len(rows[0]))
    assert np.array_equal(data, np.array(rows))


# ---- G. the coupling to the feedback source -----------------------------------------------------------------------------------------
COUPLE_OV = _mesh(16, 8) + ["parthenon/time/tlim=10.0", "parthenon/time/integrator=rk1", TRIG + "accretion_radius=0.03",
                            TRIG + "triggering_mode=COLD_GAS", AGN + "disabled=false", AGN + "fixed_power=0",
                            AGN + "thermal_fraction=1", AGN + "thermal_radius=0.05"]


@pytest.mark.gpu
def test_accretion_drives_the_feedback_power():
    """COLD_GAS with fixed_power = 0, thermal_fraction = 1, feedback enabled, rk1 (a cycle is a stage), riemann = none.
    After one step the power the options report is mdot * efficiency * c^2 in the host model's operation order, bit for
    bit; the state is the thermal source's (tests/feedback_reference.py) with the stage numbers of that power applied to
    the state the removal left -- every cell of the thermal sphere gained thermal_feedback plus the kinetic energy of the
    deposited mass -- bit for bit; the history has the agn_feedback_power column, and without triggering it has not."""
    s = _sim(COUPLE_OV).initialize()
    assert "agn_feedback_power" in s.history_labels()
    o0 = s.agn_feedback_options()
    assert o0.active == 1 and o0.power == 0.0 and o0.fixed_power == 0.0
    g, dt = _geom(s), _next_dt(s)
    # the cycle's first half through the entry: reduce and remove, which sets the rate the stage numbers take
    st = s.agn_triggering_reduce(dt)
    removed = _read(s)
    o = s.agn_feedback_options()
    assert st.accretion_rate > 0
    assert o.power == 0.0 + st.accretion_rate * o.efficiency * math.pow(o.speed_of_light, 2) and o.power == st.power
    assert o.mass_rate == st.accretion_rate * (1 - o.efficiency) + 0.0 / (o.efficiency * math.pow(o.speed_of_light, 2))
    cfg, jet = s.agn_feedback_stage_numbers(dt, 0.0)
    s.close()
    cfg, jet = (SimpleNamespace(**{n: getattr(x, n) for n, _ in x._fields_}) for x in (cfg, jet))
    assert cfg.thermal_feedback > 0 and cfg.thermal_density > 0 and cfg.jet_density == 0

    s = _sim(COUPLE_OV).initialize()
    assert _next_dt(s) == dt
    s.step()
    after = _read(s)
    o1, st1 = s.agn_feedback_options(), s.agn_triggering_state()
    s.close()
    assert st1.accretion_rate == st.accretion_rate and o1.power == o.power and st1.power == o.power
    sl = (slice(None),) + (slice(g.ng, g.ng + g.mb[2]), slice(g.ng, g.ng + g.mb[1]), slice(g.ng, g.ng + g.mb[0]))
    rose = 0
    for (u0, w0), (u1, w1), loc in zip(removed, after, g.loc):
        xs = [x[g.ng:-g.ng] for x in _centres(g, loc, g.ng)]
        u_want, w_want, info = FB.agn_feedback_src(u0[sl], w0[sl], xs[0], xs[1], xs[2], cfg, jet, GAMMA)
        assert np.array_equal(u1[sl], u_want) and np.array_equal(w1[sl], w_want)
        gain = (u1[sl][4] - u0[sl][4])[info.sphere]
        assert np.all(gain >= cfg.thermal_feedback * (1 - 4 * EPS)) and np.all(gain <= cfg.thermal_feedback * (1 + 1e-3))
        assert np.array_equal(u1[sl][:, ~info.sphere], u0[sl][:, ~info.sphere])
        rose += int(info.sphere.sum())
    assert rose > 100

    s = _sim(COUPLE_OV + [TRIG + "triggering_mode=NONE", AGN + "fixed_power=0.1"]).initialize()
    assert "agn_feedback_power" not in s.history_labels()
    s.close()


@pytest.mark.gpu
def test_zero_power_skips_the_feedback_source():
    """a threshold below every cell's temperature: no cold gas, accretion rate and power zero -- the cycle leaves conserved
    state and stored primitives of every cell unchanged bit for bit (the source returns before its closing ConsToPrim,
    agn_feedback.cpp:241) and the step succeeds"""
    s = _sim(COUPLE_OV + [TRIG + "cold_temp_thresh=1.0"]).initialize()
    before = _read(s)
    s.step()
    st = s.agn_triggering_state()
    assert st.cold_mass == 0.0 and st.accretion_rate == 0.0 and st.power == 0.0 and s.agn_feedback_options().power == 0.0
    for (u0, w0), (u1, w1) in zip(before, _read(s)):
        assert np.array_equal(u0, u1) and np.array_equal(w0, w1)
    assert s.ncycle == 1
    s.close()


# ---- H. two ranks -------------------------------------------------------------------------------------------------------------------
RANKS_OV = _mesh(16, 8) + ["parthenon/time/tlim=10.0", TRIG + "accretion_radius=0.03", TRIG + "triggering_mode=BOOSTED_BONDI"]


@pytest.mark.gpu
def test_two_ranks_equal_one(tmp_path):
    """BOOSTED_BONDI with removal on eight 8^3 blocks, 3 cycles, two ranks sharing the GPU (gloo): every block, ghost cells
    included, the time step and the reduced quantities equal the one-rank run's bit for bit -- every block's sums sit in
    their own slot and the slots are added in global block order, whatever the distribution of the blocks"""
    assert_two_ranks_equal_one(tmp_path, DECK, RANKS_OV, 3, triggering=True)


# ---- I. a sphere without a cell -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_empty_bondi_sphere_fails_the_step_and_not_the_process():
    """16^3 on +-0.1: the centres nearest the origin are at (+-0.00625)^3, r = 0.0108.  accretion_radius = 0.008 passes each
    direction's |x| < R, so the boxes are not empty, and holds no centre: the reduced total mass is zero and the step
    fails with its message instead of carrying 0 / 0 into the feedback.  The process goes on: a fresh simulation steps."""
    from athenapk_amd import lib as L
    ov = _mesh(16, 8) + ["parthenon/time/tlim=10.0", TRIG + "triggering_mode=BOOSTED_BONDI", TRIG + "accretion_radius=0.008"]
    s = _sim(ov).initialize()
    o = s.agn_triggering_options()
    assert o.active_blocks == 8 and o.active_box_cells > 0
    g = _geom(s)
    assert not any(m.any() for m in _spheres(g, 0.008))
    with pytest.raises(L.ApkError) as e:
        s.step()
    assert "total_mass" in str(e.value) and "accretion_radius" in str(e.value)
    s.close()
    s = _sim(_mesh(16, 8) + ["parthenon/time/tlim=10.0", TRIG + "triggering_mode=BOOSTED_BONDI", TRIG + "accretion_radius=0.03"]).initialize()
    s.step()
    assert s.ncycle == 1 and np.all(np.isfinite(s.gather("cons"))) and s.agn_triggering_state().total_mass > 0
    s.close()
