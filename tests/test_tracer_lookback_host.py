"""CPU tests of the tracer lookbacks' host side (no GPU): apk_amd/tracer_lookback as parsed, its refusals, that the
tracer options keep their shape, and the shift cascade of tests/tracer_lookback_reference.py against the rule that says
which cycle's value a level holds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracer_lookback_reference as R  # noqa: E402

ON = ["tracers/enabled=true"]
LOOKBACK = ON + ["apk_amd/tracer_lookback=true"]


def _plan(deck="turbulence", overrides=()):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides))


def test_lookbacks_are_off_by_default_and_on_with_the_switch_or_the_deck():
    assert _plan().tracer_lookback_options() == {"enabled": False, "n_lookback": 12}
    assert _plan(overrides=ON).tracer_lookback_options() == {"enabled": False, "n_lookback": 12}
    assert _plan("turbulence_tracers").tracer_lookback_options()["enabled"] is False
    assert _plan(overrides=ON + ["apk_amd/tracer_lookback=false"]).tracer_lookback_options()["enabled"] is False
    assert _plan(overrides=LOOKBACK).tracer_lookback_options() == {"enabled": True, "n_lookback": 12}
    plan = _plan("turbulence_tracers_lookback")
    assert plan.tracer_lookback_options() == {"enabled": True, "n_lookback": 12}
    assert plan.tracers_options() == _plan("turbulence_tracers").tracers_options()
    # not tied to the problem generator
    box = ["parthenon/mesh/refinement=none", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16",
           "parthenon/meshblock/nx3=16"]
    assert _plan("advection_3d", box + LOOKBACK).tracer_lookback_options()["enabled"] is True


REFUSED = {
    "without_tracers": (["apk_amd/tracer_lookback=true"], "tracer_lookback = true needs tracers/enabled = true"),
    "tracers_switched_off": (["tracers/enabled=false", "apk_amd/tracer_lookback=true"],
                             "tracer_lookback = true needs tracers/enabled = true"),
    "yes": (ON + ["apk_amd/tracer_lookback=yes"], "tracer_lookback must be true or false"),
    "one": (ON + ["apk_amd/tracer_lookback=1"], "tracer_lookback must be true or false"),
    "capital": (ON + ["apk_amd/tracer_lookback=True"], "tracer_lookback must be true or false"),
    "bad_value_without_tracers": (["apk_amd/tracer_lookback=maybe"], "tracer_lookback must be true or false"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_with_a_message(case):
    from athenapk_amd import lib as L
    ov, message = REFUSED[case]
    with pytest.raises(L.ApkError) as e:
        _plan(overrides=ov)
    assert message in str(e.value)
    _plan(overrides=["apk_amd/tracer_lookback=false"])  # (false is accepted without tracers)


def test_the_tracer_options_keep_their_shape_with_the_switch_on():
    o = _plan(overrides=LOOKBACK + ["tracers/initial_seed_method=random_per_block",
                                    "tracers/initial_num_tracers_per_cell=0.125",
                                    "tracers/initial_rng_seed=42"]).tracers_options()
    assert o == {"enabled": True, "initial_seed_method": "random_per_block", "tracer_step": "fused", "nfields": 8,
                 "initial_num_tracers_per_cell": 0.125, "initial_rng_seed": 42,
                 "num_tracers_per_block": int(64 * 32 * 32 * 0.125)}


EMPTY, SEED = -1000.0, -1.0  # markers: the history before the run, and the seed-time update (cycle "-1")


def _marker(cycle):
    return float(cycle) if cycle >= 0 else (SEED if cycle == -1 else EMPTY)


def test_the_cascade_keeps_what_the_rule_predicts_over_2051_cycles():
    """distinct markers: cycle c records the value c at level 0.  After the update of cycle c, level i >= 1 holds the
    marker of cycle (c - c % d) - d with d = 2^(i-1), or the empty marker where that is before the run."""
    levels = np.full(R.N_LOOKBACK, EMPTY)
    for c in range(2051):
        R.cascade(levels, c)
        levels[0] = float(c)
        want = [float(h) if h >= 0 else EMPTY for h in (R.held_cycle(i, c) for i in range(R.N_LOOKBACK))]
        assert levels.tolist() == want, c
    # spot values: after cycle 2050 the deepest level holds cycle 1024 (shifted last at 2048), level 2 holds 2048
    assert levels[11] == 1024.0 and levels[2] == 2048.0 and levels[1] == 2049.0
    assert R.shifting_levels(0) == list(range(11, 0, -1)) and R.shifting_levels(1) == [1]
    assert R.shifting_levels(6) == [2, 1] and R.shifting_levels(1536) == list(range(10, 0, -1))


def test_the_double_shift_at_cycle_zero_leaves_the_seed_in_level_one_of_the_first_row_only():
    """the seed-time update runs with cycle number 0, then the first cycle runs with cycle number 0 again: every level
    shifts twice.  The seed's value is s[1] of the first row, is gone from the second, and never reaches level 2."""
    levels = np.full((3, R.N_LOOKBACK), EMPTY)  # (a few particles at once: the cascade acts on the last axis)
    R.cascade(levels, 0)
    levels[:, 0] = SEED
    assert np.all(levels[:, 1:] == EMPTY)
    rows = []
    for c in range(40):
        R.cascade(levels, c)
        levels[:, 0] = float(c)
        rows.append(levels[0].copy())
        assert levels[0].tolist() == [_marker(R.held_cycle(i, c)) for i in range(R.N_LOOKBACK)], c
    assert rows[0][0] == 0.0 and rows[0][1] == SEED and np.all(rows[0][2:] == EMPTY)
    assert all(SEED not in r.tolist() for r in rows[1:])


def test_update_shifts_active_particles_only_and_sums_what_it_left():
    rng = np.random.default_rng(0)
    n = 50
    s, sdot = rng.standard_normal((n, 12)), rng.standard_normal((n, 12))
    rho = 10.0 ** rng.uniform(-2, 2, n)
    active = (rng.random(n) > 0.2).astype(np.int32)
    s1, sdot1 = R.update(s, sdot, rho, active, 4, 0.25)
    off = active == 0
    assert np.array_equal(s1[off], s[off]) and np.array_equal(sdot1[off], sdot[off])
    on = ~off
    assert np.array_equal(s1[on, 0], np.log(rho[on])) and np.array_equal(s1[on, 1], s[on, 0])
    assert np.array_equal(s1[on, 3], s[on, 2]) and np.array_equal(s1[on, 4], s[on, 4])  # (cycle 4: levels 1, 2, 3)
    assert np.array_equal(sdot1[on, 0], (s1[on, 0] - s1[on, 1]) / 0.25)
    exact, bound = R.sums_and_bounds(s1, sdot1, active)
    assert exact.shape == bound.shape == (R.N_SUMS,)
    assert abs(exact[24] - s1[on, 0].sum()) <= bound[24] and abs(exact[0] - (s1[on, 0] ** 2).sum()) <= bound[0]
