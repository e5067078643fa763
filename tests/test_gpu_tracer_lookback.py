"""The tracers' lookback histories and their correlations on the GPU (csrc/kernels_tracers.hip, csrc/host/tracers.cpp)
against the numpy restatement of tests/tracer_lookback_reference.py: the kernel alone through hydro.TracersLookback, and
the driver with apk_amd/tracer_lookback = true -- fused against passes, switch on against switch off, an outflow box,
growing arrays and correlations.csv.

The rules, used at both levels:
  (a) levels >= 1 after an update equal the numpy cascade of the histories before it, bit for bit (a shift moves bits);
      inactive particles and levels that do not shift keep theirs;
  (b) s[0] is within 4 ulp of np.log(rho) (both libraries document <= 1 ulp, so they differ by <= 2: a margin of 2x);
      sdot[0] equals (s[0] - s[1]) / dt formed in numpy from the kernel's own s, bit for bit in the strict build and
      within 1 ulp in the product build (reciprocal divide);
  (c) each of the 26 sums is within (n_active + 2) 2^-53 sum |term| of math.fsum of the terms formed in numpy from the
      kernel's own s and sdot (tracer_lookback_reference.sums_and_bounds: derived, not measured).
Largest |s[0] - np.log(rho)| seen on an MI355X: 1 ulp (both builds, every case below)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracer_lookback_reference as R  # noqa: E402
from test_gpu_tracers import (BUILDS, EULER_BOX, ON, TURB, USER, V_UNIFORM, _bc, _random_positions, _sim,  # noqa: E402
                              _write_prim)

pytestmark = pytest.mark.gpu

LOOKBACK = ["apk_amd/tracer_lookback=true"]
CYCLES = (0, 1, 2, 3, 4, 6, 512, 1024, 1536)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 256 * 1025 + 3)  # (the last: more than 1024 rows of partial sums)
POISON = 1.2345e300


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _inputs(n, seed):
    """rho log-uniform over four decades, about a fifth of the lanes inactive at scattered positions, random histories"""
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-2.0, 2.0, n)
    active = (rng.random(n) >= 0.2).astype(np.int32)
    if not active.any():
        active[0] = 1
    return rho, active, rng.standard_normal((n, 12)), rng.standard_normal((n, 12))


def _run(ctx, rho, active, s, sdot, cycle, dt):
    """the kernel on copies of numpy inputs [n][12]: (s, sdot, sums26) as numpy arrays"""
    import torch
    from athenapk_amd import hydro
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rho, active, s.T, sdot.T)]
    sums = hydro.TracersLookback(ctx, d[0], d[1], d[2], d[3], cycle, dt)
    return d[2].cpu().numpy().T.copy(), d[3].cpu().numpy().T.copy(), sums.cpu().numpy()


def _check_level0(s1, sdot1, rho, act, dt, strict, worst):
    """(b); returns the largest difference seen, in ulp, next to `worst`"""
    u = R.ulps(s1[act, 0], np.log(rho[act]))
    assert u.max() <= 4.0, "s[0] is %.2f ulp from np.log(rho)" % u.max()
    want = (s1[act, 0] - s1[act, 1]) / dt
    if strict:
        assert _same_bits(sdot1[act, 0], want)
    else:
        assert R.ulps(sdot1[act, 0], want).max() <= 1.0
    return max(worst, float(u.max()))


def _check_sums(sums, s1, sdot1, active, which=range(R.N_SUMS)):
    """(c); returns the largest error as a fraction of its bound"""
    exact, bound = R.sums_and_bounds(s1, sdot1, active)
    worst = 0.0
    for q in which:
        err = abs(sums[q] - exact[q])
        assert err <= bound[q], "sum %d: error %.3e, bound %.3e" % (q, err, bound[q])
        worst = max(worst, err / bound[q] if bound[q] > 0 else 0.0)
    return worst


# ---- the kernel alone ----------------------------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("n", SIZES)
def test_kernel_shifts_fills_level_zero_and_sums(strict, n):
    from athenapk_amd import hydro
    ctx = hydro.Context(strict=strict)
    rho, active, s0, sdot0 = _inputs(n, seed=n)
    act = active != 0
    dt = 0.0078125 * 1.1
    worst_log = worst_sum = 0.0
    for cycle in CYCLES:
        s1, sdot1, sums = _run(ctx, rho, active, s0, sdot0, cycle, dt)
        # (a) the shift moves bits; inactive particles keep every level
        want_s, want_sdot = R.update(s0, sdot0, rho, active, cycle, dt)
        assert _same_bits(s1[:, 1:], want_s[:, 1:]) and _same_bits(sdot1[:, 1:], want_sdot[:, 1:]), cycle
        assert _same_bits(s1[~act], s0[~act]) and _same_bits(sdot1[~act], sdot0[~act]), cycle
        worst_log = _check_level0(s1, sdot1, rho, act, dt, strict, worst_log)
        worst_sum = max(worst_sum, _check_sums(sums, s1, sdot1, active))
        # (a) again on a copy whose unshifted levels are poisoned: they come back as they went in, and a shifting level
        # above one of them takes the poison -- storing a level that does not shift with its own value is allowed,
        # storing anything else there is not
        if n <= 1000:
            keep = [i for i in range(1, 12) if i not in R.shifting_levels(cycle)]
            ps, psdot = s0.copy(), sdot0.copy()
            ps[:, keep], psdot[:, keep] = POISON, -POISON
            s2, sdot2, _ = _run(ctx, rho, active, ps, psdot, cycle, dt)
            want_s, want_sdot = R.update(ps, psdot, rho, active, cycle, dt)
            assert _same_bits(s2[:, 1:], want_s[:, 1:]) and _same_bits(sdot2[:, 1:], want_sdot[:, 1:]), cycle
            assert np.all(s2[:, keep] == POISON) and np.all(sdot2[:, keep] == -POISON), cycle
    print("lookback kernel %s n=%d: s[0] at most %.2f ulp from np.log(rho); worst sum at %.3f of its bound"
          % ("strict" if strict else "fma", n, worst_log, worst_sum))
    ctx.close()


def test_kernel_refuses_what_it_cannot_run():
    import torch
    from athenapk_amd import hydro, lib as L
    ctx = hydro.Context()
    rho = torch.ones(10, dtype=torch.float64, device="cuda")
    active = torch.ones(10, dtype=torch.int32, device="cuda")
    s = torch.zeros((12, 10), dtype=torch.float64, device="cuda")
    with pytest.raises(L.ApkError):
        hydro.TracersLookback(ctx, rho, active, s, s.clone(), -1, 0.1)  # (a negative cycle number)
    with pytest.raises(AssertionError):
        hydro.TracersLookback(ctx, rho, active, s[:11].contiguous(), s[:11].contiguous(), 0, 0.1)  # (12 levels, no fewer)
    ctx.close()


def test_kernel_with_more_particles_than_65535_workgroups():
    """(d) n = 65535 x 256 + 2563 = 16,779,523 particles, product build, cycle 1024 (levels 1 to 11 shift): the
    histories alone are 3.2 GB.  Rule (c) for sum s[0] and corr_s[0], rule (a) for the last particles of the arrays."""
    import torch
    from athenapk_amd import hydro
    n = 65535 * 256 + 2563
    ctx = hydro.Context(strict=False)
    g = torch.Generator(device="cuda").manual_seed(7)
    rho = 10.0 ** (4.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 2.0)
    active = (torch.rand(n, device="cuda", generator=g) >= 0.2).to(torch.int32)
    s = torch.randn((12, n), dtype=torch.float64, device="cuda", generator=g)
    sdot = torch.randn((12, n), dtype=torch.float64, device="cuda", generator=g)
    tail = slice(n - 3000, n)
    s_tail, sdot_tail = s[:, tail].cpu().numpy().T.copy(), sdot[:, tail].cpu().numpy().T.copy()
    sums = hydro.TracersLookback(ctx, rho, active, s, sdot, 1024, 0.01).cpu().numpy()
    act = active.cpu().numpy() != 0
    s0 = s[0].cpu().numpy()[act]
    for q, t in ((24, s0), (0, s0 * s0)):
        err, bound = abs(sums[q] - math.fsum(t.tolist())), (len(t) + 2) * 2.0 ** -53 * np.abs(t).sum()
        print("lookback kernel n=%d sum %d: error %.3e, bound %.3e" % (n, q, err, bound))
        assert err <= bound
    rho_h = rho.cpu().numpy()
    assert R.ulps(s0, np.log(rho_h[act])).max() <= 4.0
    want_s, want_sdot = R.update(s_tail, sdot_tail, rho_h[tail], act[tail], 1024, 0.01)
    assert _same_bits(s[:, tail].cpu().numpy().T[:, 1:], want_s[:, 1:])
    assert _same_bits(sdot[:, tail].cpu().numpy().T[:, 1:], want_sdot[:, 1:])
    ctx.close()


# ---- the driver ----------------------------------------------------------------------------------------------------
def _check_cycle(sim, before, cycle, time, dt, strict, t_lookback):
    """the update the sim just ran with cycle number `cycle` at `time`, from the histories `before` it: rules (a), (b),
    (c) with the rho of tracers() and the kernel's own histories; t_lookback is the host cascade, updated in place.
    Returns the histories after."""
    tr = sim.tracers(["rho", "active"])
    after = sim.tracer_lookbacks()
    assert np.array_equal(after["id"], tr["id"]) and np.array_equal(after["id"], before["id"])
    act = tr["active"] != 0
    want_s, want_sdot = R.update(before["s"], before["sdot"], tr["rho"], tr["active"], cycle, dt)
    assert _same_bits(after["s"][:, 1:], want_s[:, 1:]) and _same_bits(after["sdot"][:, 1:], want_sdot[:, 1:]), cycle
    assert _same_bits(after["s"][~act], before["s"][~act]) and _same_bits(after["sdot"][~act], before["sdot"][~act])
    _check_level0(after["s"], after["sdot"], tr["rho"], act, dt, strict, 0.0)
    row = sim.tracer_correlations()
    n_active = int(act.sum())
    assert row["cycle"] == cycle and row["time"] == time and row["n_active"] == n_active == sim.tracers_count()[0]
    exact, bound = R.sums_and_bounds(after["s"], after["sdot"], tr["active"])
    got = np.concatenate([row["corr_s"], row["corr_sdot"], [row["s"], row["sdot"]]])
    want = exact / n_active
    assert np.all(np.abs(got - want) <= bound / n_active + np.spacing(np.abs(want))), cycle
    R.cascade(t_lookback, cycle)
    t_lookback[0] = time
    assert np.array_equal(row["t_lookback"], t_lookback), cycle
    return after


def test_fused_equals_passes_equals_numpy_over_ten_cycles():
    runs = {}
    for form in ("fused", "passes"):
        sim = _sim("turbulence", ON + TURB + LOOKBACK + ["apk_amd/tracer_step=" + form], True)
        assert sim.tracer_lookback_options() == {"enabled": True, "n_lookback": 12}
        # the seed-time update: cycle 0 with the sim's dt on empty histories
        t_lookback = np.zeros(12)
        seeded = sim.tracers(["rho"])
        empty = {"id": seeded["id"], "s": np.zeros((len(seeded["id"]), 12)), "sdot": np.zeros((len(seeded["id"]), 12))}
        before = _check_cycle(sim, empty, 0, 0.0, sim.dt, True, t_lookback)
        seed_s0 = before["s"][:, 0].copy()
        assert R.ulps(seed_s0, np.log(seeded["rho"])).max() <= 4.0
        for cycle in range(10):
            time, dt = sim.time, sim.dt
            sim.step()
            before = _check_cycle(sim, before, cycle, time, dt, True, t_lookback)
            if cycle == 0:  # the double shift: the seeded state's ln rho is s[1] of the first row
                assert _same_bits(before["s"][:, 1], seed_s0) and np.all(before["s"][:, 2:] == 0.0)
        runs[form] = before
    for k in ("id", "s", "sdot"):
        assert _same_bits(runs["fused"][k], runs["passes"][k]), k


@BUILDS
def test_switch_on_leaves_tracers_and_the_flow_alone(strict):
    off = _sim("turbulence", ON + TURB, strict)
    on = _sim("turbulence", ON + TURB + LOOKBACK, strict)
    for _ in range(10):
        off.step()
        on.step()
    a, b = on.tracers(), off.tracers()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert on.time == off.time and on.dt == off.dt and np.array_equal(on.gather(), off.gather())
    assert on.tracers_stats() == off.tracers_stats() and on.tracers_count() == off.tracers_count()
    assert on.tracers_options() == off.tracers_options()
    assert off.tracer_lookback_options()["enabled"] is False and on.tracer_correlations()["cycle"] == 9
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError):
        off.tracer_lookbacks()


def _advected_density(Z, Y, X):
    """the uniform flow of test_gpu_tracers' outflow box carrying a density that varies (1 <= rho <= 2.5 on the box), so
    that the histories and the sums are not all zero"""
    one = np.ones(np.broadcast(Z, Y, X).shape)
    return [1.5 + X + 0.25 * Y * Z * one, V_UNIFORM[0] * one, V_UNIFORM[1] * one, V_UNIFORM[2] * one, 0.75 * one]


@BUILDS
@pytest.mark.parametrize("form", ["fused", "passes"])
def test_outflow_box_counts_active_particles_and_freezes_lost_histories(strict, form):
    sim = _sim("advection_3d", EULER_BOX + _bc("outflow") + USER + LOOKBACK + ["apk_amd/tracer_step=" + form], strict)
    _write_prim(sim, _advected_density)
    sim.seed_tracers(*_random_positions(sim, 20000, seed=5))
    before = sim.tracer_lookbacks()
    assert np.all(before["s"] == 0.0) and np.all(before["sdot"] == 0.0)  # (no update at user seeding)
    assert sim.tracer_correlations()["cycle"] == -1
    t_lookback = np.zeros(12)
    for cycle in range(10):
        time, dt = sim.time, sim.dt
        sim.step()
        before = _check_cycle(sim, before, cycle, time, dt, strict, t_lookback)  # (lost particles keep every level)
    act = sim.tracers(["active"])["active"] != 0
    assert sim.tracers_count()[1] > 0 and np.all(before["s"][act, 0] > 0.0)  # (rho > 1 everywhere on the box)
    assert np.any(before["s"][~act, 0] == 0.0)  # (lost in the first cycle: never updated)


@BUILDS
def test_growing_arrays_keep_the_histories_and_new_particles_start_empty(strict):
    sim = _sim("turbulence", USER + LOOKBACK, strict)
    sim.seed_tracers(*_random_positions(sim, 300, seed=1))
    for _ in range(3):
        sim.step()
    first = sim.tracer_lookbacks()
    assert np.any(first["s"][:, 0] != 0.0) and np.any(first["sdot"][:, 1] != 0.0)
    sim.seed_tracers(*_random_positions(sim, 5000, seed=2))  # (more than the capacity the first call left)
    both = sim.tracer_lookbacks()
    assert np.array_equal(both["id"], np.arange(5300))
    assert _same_bits(both["s"][:300], first["s"]) and _same_bits(both["sdot"][:300], first["sdot"])
    assert np.all(both["s"][300:] == 0.0) and np.all(both["sdot"][300:] == 0.0)
    t_lookback = sim.tracer_correlations()["t_lookback"].copy()
    time, dt = sim.time, sim.dt
    sim.step()
    _check_cycle(sim, both, 3, time, dt, strict, t_lookback)


def test_reinitialising_empties_the_histories():
    sim = _sim("turbulence", ON + TURB + LOOKBACK, False)
    first = sim.tracer_lookbacks()
    for _ in range(3):
        sim.step()
    sim.initialize()
    again, row = sim.tracer_lookbacks(), sim.tracer_correlations()
    assert _same_bits(again["s"], first["s"]) and _same_bits(again["sdot"], first["sdot"])
    assert row["cycle"] == 0 and np.all(row["t_lookback"] == 0.0) and np.all(again["s"][:, 1:] == 0.0)


def test_execute_writes_correlations_csv(tmp_path):
    from athenapk_amd import decks, driver
    sim = driver.Simulation(decks.load("turbulence_tracers_lookback"), ["parthenon/time/nlim=3"], strict=False)
    assert sim.execute(tmp_path) == 3
    path = os.path.join(str(tmp_path), "correlations.csv")
    lines = open(path).read().splitlines()
    assert len(lines) == 4 and lines[0].startswith("# cycle,time,s,sdot,corr_s[0],") and lines[0].endswith(",t_lookback[11]")
    assert len(lines[0].split(",")) == 40 and not any(l.startswith("#") for l in lines[1:])
    rows = np.loadtxt(path, delimiter=",")
    assert rows.shape == (3, 40) and rows[:, 0].tolist() == [0.0, 1.0, 2.0] and rows[0, 1] == 0.0
    row = sim.tracer_correlations()
    want = np.concatenate([[row["cycle"], row["time"], row["s"], row["sdot"]], row["corr_s"], row["corr_sdot"],
                           row["t_lookback"]])
    assert np.array_equal(rows[2], want)
    off = driver.Simulation(decks.load("turbulence_tracers"), ["parthenon/time/nlim=3"], strict=False)
    out = tmp_path / "off"
    out.mkdir()
    assert off.execute(out) == 3 and not os.path.exists(os.path.join(str(out), "correlations.csv"))
