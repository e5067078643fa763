"""CPU tests of the cluster problem's AGN triggering on the host side (no GPU): the deck's keys and defaults, the
refusals, the accretion rate of the three modes, the time-step rule, power and mass rate with accretion, and the active
list -- against the numpy restatement (tests/triggering_reference.py)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402
import triggering_reference as TR  # noqa: E402

EPS = np.finfo(np.float64).eps
TRIG = "problem/cluster/agn_triggering/"
AGN = "problem/cluster/agn_feedback/"
MODE_KEY = "problem/cluster/agn_triggering/triggering_mode"


def _plan(overrides=(), deck="cluster_agn_triggering", **kw):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides), strict=True, **kw)


def _refused(overrides=(), deck="cluster_agn_triggering"):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def _mesh(n, mb, lo, hi):
    n = (n,) * 3 if isinstance(n, int) else n
    mb = (mb,) * 3 if isinstance(mb, int) else mb
    return (["parthenon/mesh/nx%d=%d" % (d + 1, n[d]) for d in range(3)] +
            ["parthenon/meshblock/nx%d=%d" % (d + 1, mb[d]) for d in range(3)] +
            ["parthenon/mesh/x%dmin=%r" % (d + 1, lo[d]) for d in range(3)] +
            ["parthenon/mesh/x%dmax=%r" % (d + 1, hi[d]) for d in range(3)])


def _restated_model(o):
    return TR.model(o.mode, accretion_radius=o.accretion_radius, cold_temp_thresh=o.cold_temp_thresh, cold_t_acc=o.cold_t_acc,
                    bondi_alpha=o.bondi_alpha, bondi_M_smbh=o.bondi_M_smbh, bondi_n0=o.bondi_n0, bondi_beta=o.bondi_beta,
                    accretion_cfl=o.accretion_cfl, mean_molecular_mass=o.mean_molecular_mass,
                    gravitational_constant=o.gravitational_constant)


# ---- 1. parsing -------------------------------------------------------------------------------------------------------------
def test_the_deck_keys_are_parsed():
    from athenapk_amd import lib as L
    o = _plan().agn_triggering_options()
    assert o.mode == L.TRIGGERING_MODE["COLD_GAS"] and o.remove_accreted_mass == 1 and o.write_to_file == 1
    assert o.accretion_radius == 0.02 and o.cold_temp_thresh == 7198.523584993223 and o.cold_t_acc == 0.1
    assert o.bondi_alpha == 100 and o.bondi_beta == 2 and o.bondi_n0 == 1.4928506511614273e+74 and o.accretion_cfl == 0.1
    assert o.bondi_M_smbh == 1e-6 and o.triggering_filename == b"agn_triggering.dat"
    u = R.DECK_UNITS
    mu, _ = R.composition(R.DECK_HE)
    mmm = mu * (np.float64(R.AMU_CGS) / u.m)
    assert o.mean_molecular_mass == mmm and o.mean_molecular_mass_by_kb == mmm / u.k_boltzmann()
    assert o.gravitational_constant == u.gravitational_constant()
    # the deck's own comments: the threshold is 1.01 of the gas temperature, n0 is 0.05 of the number density
    T = o.mean_molecular_mass_by_kb * 1.5454368403867558 / 14775.575892787225
    assert abs(o.cold_temp_thresh / (1.01 * T) - 1) < 1e-12 and abs(o.bondi_n0 / (0.05 * 14775.575892787225 / mmm) - 1) < 1e-12


@pytest.mark.parametrize("mode", ["NONE", "COLD_GAS", "BOOSTED_BONDI", "BOOTH_SCHAYE"])
def test_every_mode_is_accepted(mode):
    from athenapk_amd import lib as L
    p = _plan([TRIG + "triggering_mode=" + mode])
    o = p.agn_triggering_options()
    assert o.mode == L.TRIGGERING_MODE[mode]
    assert (o.active_blocks > 0) == (mode != "NONE")


def test_the_defaults_are_the_references():
    """a cluster deck without the block: mode NONE, every number 0 but accretion_cfl = 0.1, removal on, no file"""
    o = _plan(deck="cluster_agn_feedback").agn_triggering_options()
    assert o.mode == 0 and o.remove_accreted_mass == 1 and o.write_to_file == 0 and o.active_blocks == 0 and o.active_box_cells == 0
    assert (o.accretion_radius, o.cold_temp_thresh, o.cold_t_acc, o.bondi_alpha, o.bondi_n0, o.bondi_beta) == (0,) * 6
    assert o.accretion_cfl == 0.1 and o.triggering_filename == b"agn_triggering.dat"
    # (m_smbh keeps the gravity block's default, 3.4e8 Msun)
    assert o.bondi_M_smbh == 3.4e8 * R.DECK_UNITS.msun()


def test_removal_and_file_switches():
    o = _plan([TRIG + "removed_accreted_mass=false", TRIG + "write_to_file=false", TRIG + "triggering_filename=t.dat"]).agn_triggering_options()
    assert o.remove_accreted_mass == 0 and o.write_to_file == 0 and o.triggering_filename == b"t.dat"


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ([TRIG + "triggering_mode=EDDINGTON"], "Unrecognized AGNTriggeringMode"),
    ([TRIG + "triggering_mode=BOOSTED_BONDI", TRIG + "accretion_radius=0"], MODE_KEY),
    ([TRIG + "triggering_mode=COLD_GAS", TRIG + "accretion_radius=-1"], MODE_KEY),
    ([TRIG + "triggering_mode=COLD_GAS", TRIG + "cold_t_acc=0"], MODE_KEY),
    ([TRIG + "triggering_mode=BOOTH_SCHAYE", TRIG + "bondi_n0=0"], TRIG + "bondi_n0"),
    ([TRIG + "accretion_cfl=0"], TRIG + "accretion_cfl"),
    ([TRIG + "triggering_mode=NONE", TRIG + "accretion_cfl=-0.1"], TRIG + "accretion_cfl"),
    (["diffusion/integrator=rkl2", "diffusion/conduction=isotropic", "diffusion/conduction_coeff=fixed",
      "diffusion/thermal_diff_coeff_code=0.01", "diffusion/rkl2_max_dt_ratio=100"], MODE_KEY),
    ([AGN + "disabled=false"], MODE_KEY),
]


@pytest.mark.parametrize("overrides,needle", REFUSALS, ids=[str(n) for n in range(len(REFUSALS))])
def test_refusals_name_their_key(overrides, needle):
    msg = _refused(overrides)
    assert needle in msg, msg


def test_a_mode_alone_on_a_deck_without_the_block_is_refused_for_its_radius():
    """triggering_mode = BOOSTED_BONDI alone (radius 0), and COLD_GAS with a radius but no cold_t_acc"""
    assert MODE_KEY in _refused([TRIG + "triggering_mode=BOOSTED_BONDI"], deck="cluster_agn_feedback")
    msg = _refused([TRIG + "triggering_mode=COLD_GAS", TRIG + "accretion_radius=0.02"], deck="cluster_agn_feedback")
    assert MODE_KEY in msg and "cold_t_acc" in msg


def test_a_mode_without_units_and_composition_is_refused():
    from athenapk_amd import decks, driver, lib as L
    deck = decks.load("cluster_agn_triggering")
    line, = [ln for ln in deck.splitlines() if ln.startswith("He_mass_fraction")]
    with pytest.raises(L.ApkError) as e:
        driver.HostPlan(deck.replace(line + "\n", ""), [], strict=True)
    assert MODE_KEY in str(e.value) and "He_mass_fraction" in str(e.value)


def test_feedback_enabled_needs_a_fraction_and_then_is_active():
    assert "fractions are all zero" in _refused([AGN + "disabled=false"])
    p = _plan([AGN + "disabled=false", AGN + "thermal_fraction=1"])
    o = p.agn_feedback_options()
    assert o.configured == 1 and o.active == 1 and o.fixed_power == 0 and o.tower_power_scaling == 0 and o.power == 0
    assert _plan().agn_feedback_options().active == 0  # (the deck disables feedback)


# ---- 3. the accretion rate, the time step, power and mass rate ------------------------------------------------------------------
def test_cold_gas_rate_and_time_step():
    """cold_mass / cold_t_acc: one rounding; accretion_cfl * cold_t_acc: one rounding, whatever the mass"""
    p = _plan()
    m = _restated_model(p.agn_triggering_options())
    for q in (0.0, 0.37, 12.5):
        got, want = p.agn_triggering_accretion_rate(q), TR.accretion_rate(m, q)
        assert abs(got - want) <= 1 * EPS * abs(want)
        assert p.agn_triggering_timestep(q) == 0.1 * 0.1
    st = p.agn_triggering_state()
    assert st.accretion_rate == 0 and st.cold_mass == 0 and st.dt_limit == 0.1 * 0.1 and st.power == 0


BONDI_Q = [(0.49, 0.49 * 14775.0, 0.49 * 8.9e-4, 0.49 * 0.0132), (3.0, 3.0 * 5.0e4, 3.0 * 0.5, 3.0 * 0.02)]


@pytest.mark.parametrize("q", BONDI_Q)
def test_boosted_bondi_rate(q):
    """alpha 2 pi G^2 M^2 rho / (v^2 + cs^2)^(3/2).  Roundings, pow counted as one: three quotients by total_mass; alpha * 2,
    * pi, pow(G, 2), *, pow(M, 2), *, * rho: 7; pow(v, 2), pow(cs, 2), their sum, pow(., 3/2): 4; the final quotient: 15.
    The errors of v and cs pass through a square and the 3/2 power (weight 3 instead of 1: +4) and those of the two
    squares and the sum through the 3/2 power (weight 3/2: +1.5): 21 eps."""
    p = _plan([TRIG + "triggering_mode=BOOSTED_BONDI"])
    m = _restated_model(p.agn_triggering_options())
    got, want = p.agn_triggering_accretion_rate(q), TR.accretion_rate(m, q)
    print(got, want, abs(got / want - 1) / EPS)
    assert want > 0 and abs(got - want) <= 21 * EPS * want
    # ... and the formula itself, from its parts
    rho, v, cs = q[1] / q[0], q[2] / q[0], q[3] / q[0]
    direct = 100 * 2 * math.pi * m.gravitational_constant ** 2 * 1e-12 * rho / (v * v + cs * cs) ** 1.5
    assert abs(got / direct - 1) < 1e-13
    # the time step: accretion_cfl * total_mass / mdot, two more roundings
    dt = p.agn_triggering_timestep(q)
    assert abs(dt - 0.1 * q[0] / want) <= 23 * EPS * dt


@pytest.mark.parametrize("q", BONDI_Q)
def test_booth_schaye_rate(q):
    """the Bondi rate with alpha = (n / n0)^beta above n0: n = rho / mean_molecular_mass, n / n0 and pow add three
    roundings; with beta = 2 the first two and rho's own quotient weigh twice more (+ 2 each, rho's + 2): 21 + 3 + 6 = 30 eps"""
    p = _plan([TRIG + "triggering_mode=BOOTH_SCHAYE"])
    o = p.agn_triggering_options()
    m = _restated_model(o)
    got, want = p.agn_triggering_accretion_rate(q), TR.accretion_rate(m, q)
    n = q[1] / q[0] / o.mean_molecular_mass
    assert n > o.bondi_n0
    assert abs(got - want) <= 30 * EPS * want
    boosted = TR.accretion_rate(TR.model(TR.BOOSTED_BONDI, **{k: v for k, v in m.__dict__.items() if k != "mode"}), q)
    assert abs(got / (boosted / 100 * (n / o.bondi_n0) ** 2) - 1) < 1e-13


def test_booth_schaye_alpha_is_exactly_one_at_n0():
    """n == n0 takes the <= branch: alpha is 1, not pow(1, beta) of a rounded quotient -- the rate is the boosted rate
    with bondi_alpha = 1 bit for bit; just above n0 it is larger"""
    q = BONDI_Q[0]
    mmm = _plan().agn_triggering_options().mean_molecular_mass
    n = q[1] / q[0] / mmm  # as the model forms it
    p = _plan([TRIG + "triggering_mode=BOOTH_SCHAYE", TRIG + "bondi_n0=%r" % n])
    assert p.agn_triggering_options().bondi_n0 == n
    one = _plan([TRIG + "triggering_mode=BOOSTED_BONDI", TRIG + "bondi_alpha=1"])
    assert p.agn_triggering_accretion_rate(q) == one.agn_triggering_accretion_rate(q)
    below = _plan([TRIG + "triggering_mode=BOOTH_SCHAYE", TRIG + "bondi_n0=%r" % float(np.nextafter(n, 0))])
    assert below.agn_triggering_accretion_rate(q) > one.agn_triggering_accretion_rate(q)


@pytest.mark.parametrize("mode", ["BOOSTED_BONDI", "BOOTH_SCHAYE"])
def test_first_bondi_cycle_is_unconstrained(mode):
    p = _plan([TRIG + "triggering_mode=" + mode])
    assert p.agn_triggering_timestep((0.0, 0.0, 0.0, 0.0)) == sys.float_info.max
    assert p.agn_triggering_state().dt_limit == sys.float_info.max
    assert p.agn_triggering_timestep(BONDI_Q[0]) < 1.0


def test_power_and_mass_rate_with_accretion():
    """fixed_power + mdot * efficiency * pow(c, 2): four roundings; mdot * (1 - efficiency) + fixed_power / (efficiency *
    pow(c, 2)): six.  With the deck's fixed power and without one."""
    for ov, fixed in (([], 0.3319965633348794), ([AGN + "fixed_power=0"], 0.0)):
        p = _plan(ov, deck="cluster_agn_feedback")
        o = p.agn_feedback_options()
        c, eff = o.speed_of_light, o.efficiency
        for mdot in (0.0, 0.81, 37.0):
            power, mass_rate = p.agn_feedback_power_of(mdot)
            want_p = fixed + mdot * eff * math.pow(c, 2)
            want_m = mdot * (1 - eff) + fixed / (eff * math.pow(c, 2))
            assert abs(power - want_p) <= 4 * EPS * abs(want_p) and abs(mass_rate - want_m) <= 6 * EPS * abs(want_m)
        assert p.agn_feedback_power_of(0.0) == (o.power, o.mass_rate)
        assert p.agn_feedback_power_of(1.0)[0] > fixed


# ---- 4. the active list -----------------------------------------------------------------------------------------------------------
def _geometry(p):
    info = p.info
    return info.ng, tuple(info.mb), tuple(info.dx), tuple(info.xmin)


def _extended_centres(p, lb):
    ng, mb, dx, xmin = _geometry(p)
    loc = p.block_gid(lb)[1]
    return [R.cell_centres(xmin[d], dx[d], loc[d] * mb[d] - ng, mb[d] + 2 * ng) for d in range(3)]


def _check_list_covers_sphere(p):
    """every cell of every local block, ghost cells included, that the restatement puts inside the sphere lies in the
    block's box: the list hides no cell.  Returns {local block: (lo, hi)}."""
    radius = p.agn_triggering_options().accretion_radius
    boxes = {lb: (lo, hi) for lb, lo, hi in p.agn_triggering_active_list()}
    assert len(boxes) == p.agn_triggering_options().active_blocks
    cells = 0
    for lb in range(p.info.nblocks_local):
        xs = _extended_centres(p, lb)
        inside = TR.sphere(xs[0], xs[1], xs[2], radius)
        box = np.zeros(inside.shape, bool)
        if lb in boxes:
            lo, hi = boxes[lb]
            box[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
            cells += int(box.sum())
            assert all(0 <= lo[d] < hi[d] <= len(xs[d]) for d in range(3))
            assert (lo, hi) == tuple(zip(*[TR.index_range(xs[d], radius) for d in range(3)]))
        assert not np.any(inside & ~box)
    assert cells == p.agn_triggering_options().active_box_cells
    return boxes


def test_active_list_eight_blocks():
    """16^3 in 8^3 blocks on +-0.1, radius 0.03 (2.4 cells): the sphere touches all eight blocks, and each block's box
    reaches into the ghost cells it has towards the centre"""
    p = _plan(_mesh(16, 8, (-0.1,) * 3, (0.1,) * 3) + [TRIG + "accretion_radius=0.03"])
    boxes = _check_list_covers_sphere(p)
    ng, mb, _, _ = _geometry(p)
    assert ng == 2 and len(boxes) == 8
    for lb, (lo, hi) in boxes.items():
        loc = p.block_gid(lb)[1]
        for d in range(3):
            if loc[d] == 0:  # the centre lies beyond the block's upper face: the box ends in the upper ghost zone
                assert hi[d] > ng + mb[d] and lo[d] >= ng
            else:
                assert lo[d] < ng and hi[d] <= ng + mb[d]


def test_active_list_leaves_out_a_block_the_sphere_does_not_reach():
    """32 x 8 x 8 in 16 x 8 x 8 blocks, the box shifted so that the origin lies well inside the first block's interior:
    the other block is absent, or its box holds ghost cells only"""
    p = _plan(_mesh((32, 8, 8), (16, 8, 8), (-0.2, -0.1, -0.1), (0.6, 0.1, 0.1)) + [TRIG + "accretion_radius=0.06"])
    boxes = _check_list_covers_sphere(p)
    ng, mb, dx, xmin = _geometry(p)
    assert 0 in boxes
    xs = _extended_centres(p, 0)
    inside = TR.sphere(xs[0], xs[1], xs[2], 0.06)
    interior = np.zeros(inside.shape, bool)
    interior[ng:ng + mb[2], ng:ng + mb[1], ng:ng + mb[0]] = True
    assert inside.sum() > 0 and not np.any(inside & ~interior)
    if 1 in boxes:
        lo, hi = boxes[1]
        assert hi[0] <= ng or lo[0] >= ng + mb[0]
    else:
        assert p.agn_triggering_options().active_blocks == 1


def test_active_list_of_each_rank_of_two():
    """two ranks of the eight-block mesh: each rank lists its own four blocks, by local index"""
    ov = _mesh(16, 8, (-0.1,) * 3, (0.1,) * 3) + [TRIG + "accretion_radius=0.03"]
    total = 0
    for rank in range(2):
        p = _plan(ov, rank=rank, nranks=2)
        boxes = _check_list_covers_sphere(p)
        assert sorted(boxes) == list(range(p.info.nblocks_local))
        total += len(boxes)
    assert total == 8


def test_a_radius_smaller_than_a_cell_can_leave_the_list_empty_of_interior_cells():
    """radius 0.001 on the 16^3 mesh (dx = 0.0125): no centre is inside, every direction's range is empty, no block listed"""
    p = _plan(_mesh(16, 8, (-0.1,) * 3, (0.1,) * 3) + [TRIG + "accretion_radius=0.001"])
    assert p.agn_triggering_active_list() == [] and p.agn_triggering_options().active_box_cells == 0


# ---- the restated order of the device's block sum ------------------------------------------------------------------------
def _pairwise(v):
    """the halving tree on a list whose length is a power of two, written as a recursion: (lower half + upper half)"""
    if len(v) == 1:
        return v[0]
    h = len(v) // 2
    return _pairwise([a + b for a, b in zip(v[:h], v[h:])])


@pytest.mark.parametrize("n,P", [(1, 1), (2, 1), (255, 1), (257, 1), (4096, 1), (4097, 2), (13824, 4), (13824, 3), (300, 4)])
def test_block_sum_restatement(n, P):
    """TR.block_sum, the yardstick of the GPU test of the shared sum, on random positive terms: within (N - 1) eps sum |t|
    of math.fsum, which bounds every order of adding N numbers.  Where its order is simple enough to write down another
    way it is that order bit for bit: terms on lane 0 only (cells 0, 256, 512, ...) with P = 1 give the plain in-order sum
    (adding zeros is exact); N <= 2 with P = 1 likewise; N <= 256 with P = 1 gives the halving tree of the terms padded
    with zeros to 256, one term per lane."""
    rng = np.random.default_rng(n + P)
    t = rng.uniform(0.5, 1.5, (3, n))
    got = TR.block_sum(t, P)
    for row, g in zip(t, got):
        assert abs(g - math.fsum(row)) <= max(n - 1, 0) * EPS * math.fsum(np.abs(row))
    if P == 1:
        on_lane0 = np.where(np.arange(n) % TR.BLOCK_SUM_LANES == 0, t[0], 0.0)
        want = 0.0
        for x in on_lane0[::TR.BLOCK_SUM_LANES]:
            want += x
        assert TR.block_sum(on_lane0, 1) == want
        if n <= 2:
            assert got[0] == sum(t[0].tolist())
        if n <= TR.BLOCK_SUM_LANES:
            assert got[0] == _pairwise(t[0].tolist() + [0.0] * (TR.BLOCK_SUM_LANES - n))


def test_block_sum_groups():
    assert [TR.block_sum_groups(n) for n in (0, 1, 4096, 4097, 13824, 64 * 4096, 10 ** 9)] == [1, 1, 1, 2, 4, 64, 64]
