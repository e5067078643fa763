"""Tracer particles on the GPU (csrc/kernels_tracers.hip, csrc/host/tracers.cpp) against the numpy restatement of
tests/tracers_reference.py: uniform flow, linear fields, one step and a whole run on the turbulence deck (fused against
passes against numpy), bookkeeping in periodic and outflow boxes, passivity of the hydro state, and more particles than
65535 x 256."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracers_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

BUILDS = pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
ON = ["tracers/enabled=true"]
USER = ON + ["tracers/initial_seed_method=user"]
# a 32^3 Euler box of 8 blocks (nghost = 2, PLM + HLLE, VL2), periodic unless said otherwise
EULER_BOX = ["parthenon/mesh/refinement=none", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16",
             "parthenon/meshblock/nx3=16", "parthenon/mesh/x1min=-0.5", "parthenon/mesh/x1max=0.5",
             "parthenon/mesh/x2min=0.0", "parthenon/mesh/x2max=1.0", "parthenon/mesh/x3min=1.0", "parthenon/mesh/x3max=2.0"]
TURB = ["tracers/initial_seed_method=random_per_block", "tracers/initial_num_tracers_per_cell=0.125"]


def _bc(kind):
    return ["parthenon/mesh/%sx%d_bc=%s" % (s, d, kind) for s in "io" for d in (1, 2, 3)]


def _sim(deck, overrides, strict):
    from athenapk_amd import decks, driver
    return driver.Simulation(decks.load(deck), list(overrides), strict=strict).initialize()


def _grid(sim):
    i = sim.info
    return T.Grid(tuple(i.xmin), tuple(i.xmax), tuple(i.nx), tuple(i.mb), i.ng)


def _centres(sim, lb):
    """cell-centre coordinates of local block lb including ghost cells: (Z, Y, X) broadcastable to [Nk][Nj][Ni]"""
    i = sim.info
    _, loc = sim.block_gid(lb)
    ax = []
    for d in range(3):
        idx = np.arange(-i.ng, i.mb[d] + i.ng, dtype=np.float64)
        ax.append(i.xmin[d] + (loc[d] * i.mb[d] + idx + 0.5) * i.dx[d])
    return ax[2][:, None, None], ax[1][None, :, None], ax[0][None, None, :]


def _write_prim(sim, fn):
    """cons of every block from the primitives fn(Z, Y, X) -> [nvar], then ghost exchange, ConsToPrim and a new dt"""
    i = sim.info
    g = i.gamma
    for lb in range(i.nblocks_local):
        Z, Y, X = _centres(sim, lb)
        w = np.empty(sim.block_shape)
        vals = fn(Z, Y, X)
        for v in range(w.shape[0]):
            w[v] = vals[v] if v < len(vals) else 0.0
        u = np.zeros_like(w)
        u[0] = w[0]
        for d in (1, 2, 3):
            u[d] = w[0] * w[d]
        u[4] = w[4] / (g - 1.0) + 0.5 * w[0] * (w[1] ** 2 + w[2] ** 2 + w[3] ** 2)
        if i.nhydro == 9:
            u[4] += 0.5 * (w[5] ** 2 + w[6] ** 2 + w[7] ** 2)
            u[5:9] = w[5:9]
        sim.write_block(lb, u)
    sim.exchange_ghosts()
    sim.fill_derived()
    sim.reset_time_step()


def _prims(sim):
    return {sim.block_gid(lb)[0]: sim.read_block(lb, "prim") for lb in range(sim.info.nblocks_local)}


def _gids(sim, blocks):
    table = np.array([sim.block_gid(lb)[0] for lb in range(sim.info.nblocks_local)], dtype=np.int64)
    return table[blocks]


def _state(sim, tr):
    st = {k: tr[k].copy() for k in tr if k not in ("block", "id")}
    st["gid"] = _gids(sim, tr["block"])
    return st


def _wrap(x, lo, hi):
    return lo + np.mod(x - lo, hi - lo)


def _wrapped_distance(a, b, L):
    d = np.abs(a - b)
    return np.minimum(d, np.abs(L - d))


def _random_positions(sim, n, seed, margin_cells=0.0):
    rng = np.random.default_rng(seed)
    i = sim.info
    return [i.xmin[d] + margin_cells * i.dx[d] + rng.random(n) * ((i.xmax[d] - i.xmin[d]) - 2 * margin_cells * i.dx[d])
            for d in range(3)]


V_UNIFORM = (0.375, -0.25, 0.1875)


def _uniform_state(Z, Y, X):
    one = np.ones(np.broadcast(Z, Y, X).shape)
    return [one, V_UNIFORM[0] * one, V_UNIFORM[1] * one, V_UNIFORM[2] * one, 0.75 * one]


# ---- 1. uniform flow ---------------------------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("form", ["fused", "passes"])
def test_uniform_flow_moves_tracers_with_the_flow(strict, form):
    """Constant velocity in a periodic box, 20 cycles: x = x0 + v t, wrapped, within 1e-13 box lengths.  The bound is
    derived, not measured: 20 additions of dt v, each rounded at 2^-52 relative to a coordinate of at most two box
    lengths in magnitude, accumulate at most 20 x 2 x 2.2e-16 = 9e-15 box lengths (the interpolated velocity, w v + (1 - w) v, is v to a few
    2^-52 and moves a particle by less than a cell per cycle: nothing next to that); 1e-13 leaves a tenfold margin."""
    sim = _sim("advection_3d", EULER_BOX + _bc("periodic") + USER + ["apk_amd/tracer_step=" + form], strict)
    _write_prim(sim, _uniform_state)
    x0 = _random_positions(sim, 5000, seed=1)
    sim.seed_tracers(*x0)
    t0 = sim.time
    for _ in range(20):
        sim.step()
    tr = sim.tracers()
    i = sim.info
    assert sim.tracers_count() == (5000, 0)
    for d, k in enumerate("xyz"):
        L = i.xmax[d] - i.xmin[d]
        want = _wrap(x0[d] + V_UNIFORM[d] * (sim.time - t0), i.xmin[d], i.xmax[d])
        err = _wrapped_distance(tr[k], want, L).max() / L
        print("uniform flow %s %s %s: max error %.3e box lengths" % ("strict" if strict else "fma", form, k, err))
        assert err <= 1e-13
        assert np.max(np.abs(tr["vel_" + k] - V_UNIFORM[d])) <= 4e-16  # (w v + (1 - w) v: a few roundings of v)


# ---- 2. linear fields --------------------------------------------------------------------------------------------
# constant, d/dx, d/dy, d/dz of every primitive: no function comes near zero on either box (|x|, |y|, |z| <= 3)
LIN = np.array([[1.0, 0.03, -0.02, 0.025], [0.6, 0.02, 0.03, -0.025], [-0.5, 0.01, -0.02, 0.03], [0.7, -0.03, 0.01, 0.02],
                [1.5, -0.03, 0.02, 0.03], [0.8, 0.03, -0.025, 0.02], [-0.6, 0.03, 0.02, -0.01], [0.5, -0.02, 0.03, 0.03],
                [0.0, 0.0, 0.0, 0.0]])


def _linear_state(Z, Y, X):
    return [c[0] + c[1] * X + c[2] * Y + c[3] * Z for c in LIN]


@BUILDS
@pytest.mark.parametrize("deck", ["advection_3d", "linear_wave_mhd3d"])
def test_fill_reproduces_linear_fields_across_block_boundaries(strict, deck):
    """Primitives linear in x, y, z in every block, ghost zones exchanged; tracers at least two cells from the domain
    edge (where the periodic exchange breaks the linear function) but on and across block boundaries, where one or both
    cells of the stencil are ghost cells.  Trilinear weights reproduce linear data: within 1e-13 relative to the
    function's value (all of them are of order 0.1 - 1; the conversion to conserved variables and back costs a few
    2^-52 of the total energy, below 1e-15 here)."""
    ov = (EULER_BOX if deck == "advection_3d" else []) + _bc("periodic") + USER
    sim = _sim(deck, ov, strict)
    _write_prim(sim, _linear_state)
    i = sim.info
    x = _random_positions(sim, 4000, seed=2, margin_cells=2.0)
    # on the block faces, and within half a cell on either side of them (the stencil then straddles the boundary)
    rng = np.random.default_rng(3)
    for d in range(3):  # (600 particles per direction; the slices overlap, which puts 200 + 200 on edges)
        size = i.mb[d] * i.dx[d]
        face = i.xmin[d] + size * rng.integers(1, i.nx[d] // i.mb[d], 600)
        x[d][400 * d:400 * d + 600] = face + np.tile([0.0, -0.4999, 0.4999], 200) * i.dx[d]
    sim.seed_tracers(*x)
    tr = sim.tracers()
    nf = 8 if i.nhydro == 9 else 5
    worst = 0.0
    for q in range(nf):
        c = LIN[T.FIELD_VARS[q]]
        want = c[0] + c[1] * tr["x"] + c[2] * tr["y"] + c[3] * tr["z"]
        worst = max(worst, np.max(np.abs(tr[T.FIELD_NAMES[q]] - want) / np.abs(want)))
    print("linear fields %s %s: max relative error %.3e" % (deck, "strict" if strict else "fma", worst))
    assert np.array_equal(tr["x"], x[0]) and worst <= 1e-13


@BUILDS
def test_seeding_in_several_calls_grows_the_arrays_and_keeps_what_they_held(strict):
    """three seed_tracers calls, each larger than the capacity the one before left: ids run on in call order, the earlier
    particles keep their positions and fields, and the new ones are filled"""
    sim = _sim("advection_3d", EULER_BOX + _bc("periodic") + USER, strict)
    _write_prim(sim, _linear_state)
    xs = [_random_positions(sim, n, seed=10 + n, margin_cells=2.0) for n in (100, 1000, 7000)]
    first = None
    for q, x in enumerate(xs):
        sim.seed_tracers(*x)
        tr = sim.tracers()
        if first is None:
            first = tr
        total = sum(len(p[0]) for p in xs[:q + 1])
        assert np.array_equal(tr["id"], np.arange(total)) and sim.tracers_count() == (total, 0)
        for d, k in enumerate("xyz"):
            assert np.array_equal(tr[k], np.concatenate([p[d] for p in xs[:q + 1]])), k
        for k in first:
            assert np.array_equal(tr[k][:100], first[k]), k
    c = LIN[0]
    want = c[0] + c[1] * tr["x"] + c[2] * tr["y"] + c[3] * tr["z"]
    assert np.max(np.abs(tr["rho"] - want) / np.abs(want)) <= 1e-13
    sim.step()
    assert sim.tracers_stats()[0] == 1 and sim.tracers_count() == (8100, 0)


# ---- 3. one tracer step on a real state ----------------------------------------------------------------------------
def _compare(got, want, strict, what, quiet=False):
    """strict build: bit for bit.  Product build: within 1e-13, normalised by the box length for positions (1 here) and by
    the largest magnitude of the field for fields -- NOT per value: a step is a few dozen fp64 operations on identical
    input and only contraction and reciprocal division differ; a gather's rounding scales with the cell values it sums,
    and a velocity or field component near zero is a cancelled sum whose own magnitude says nothing about it.  The worst
    normalised error of every array is printed either way."""
    for k in got:
        scale = 1.0 if k in "xyz" else np.max(np.abs(want[k]))
        err = np.max(np.abs(got[k] - want[k])) / scale
        if not quiet:
            print("%s %s %s: worst error %.3e (normalised)" % (what, "strict" if strict else "fma", k, err))
        if strict:
            assert np.array_equal(got[k], want[k]), "%s: %s differs, max %.3e" % (what, k, np.max(np.abs(got[k] - want[k])))
        else:
            assert err <= 1e-13, (what, k, err)


@BUILDS
def test_one_step_on_the_turbulence_deck_matches_numpy(strict):
    sim = _sim("turbulence", ON + TURB, strict)
    for _ in range(4):
        sim.step()
    grid = _grid(sim)
    prims = _prims(sim)
    tr = sim.tracers()
    want = T.step(grid, prims, _state(sim, tr), sim.dt, 8)
    sim.tracers_step(sim.dt)
    got = sim.tracers()
    assert np.array_equal(got["id"], tr["id"]) and np.any(got["x"] != tr["x"])
    names = ["x", "y", "z"] + list(T.FIELD_NAMES)
    _compare({k: got[k] for k in names}, want, strict, "one step")
    assert np.array_equal(_gids(sim, got["block"]), want["gid"])


# ---- 4. whole run ------------------------------------------------------------------------------------------------
def test_whole_run_fused_equals_passes_equals_numpy():
    """strict build, 10 cycles of the turbulence deck: the fused step and the three passes agree bit for bit, and both
    with the numpy reference stepped on the primitives read back after every cycle"""
    names = ["x", "y", "z"] + list(T.FIELD_NAMES)
    runs = {}
    for form in ("fused", "passes"):
        sim = _sim("turbulence", ON + TURB + ["apk_amd/tracer_step=" + form], True)
        assert sim.tracers_options()["tracer_step"] == form
        grid = _grid(sim)
        tr = sim.tracers()
        ref = T.fill(grid, _prims(sim), _state(sim, tr), 8)
        _compare({k: tr[k] for k in names}, ref, True, form + " initial fill")
        for cycle in range(10):
            dt = sim.dt
            sim.step()
            ref = T.step(grid, _prims(sim), ref, dt, 8)
            got = sim.tracers()
            _compare({k: got[k] for k in names}, ref, True, "%s cycle %d" % (form, cycle), quiet=cycle < 9)
        assert np.array_equal(_gids(sim, got["block"]), ref["gid"])
        runs[form] = got
    for k in runs["fused"]:
        assert np.array_equal(runs["fused"][k], runs["passes"][k]), k


# ---- 5. bookkeeping ----------------------------------------------------------------------------------------------
def _check_owners(sim, tr):
    i = sim.info
    act = tr["active"] != 0
    grid = _grid(sim)
    gids = _gids(sim, tr["block"])
    assert np.array_equal(T.owner(grid, tr["x"][act], tr["y"][act], tr["z"][act]), gids[act])
    for d, k in enumerate("xyz"):
        # (the block grid's floor may round a position one unit in the last place into the neighbour: 4 ulp of the box)
        tol = 4 * np.spacing(max(abs(i.xmin[d]), abs(i.xmax[d])))
        lo = np.array([grid.origin(int(g))[d] for g in gids[act]])
        assert np.all(tr[k][act] >= lo - tol) and np.all(tr[k][act] <= lo + grid.block_size[d] + tol)
    assert len(np.unique(tr["id"])) == len(tr["id"])


@BUILDS
def test_periodic_box_keeps_every_tracer(strict):
    sim = _sim("turbulence", ON + TURB, strict)
    n = sim.tracers_options()["num_tracers_per_block"] * sim.info.nblocks_total
    for _ in range(10):
        sim.step()
        assert sim.tracers_count() == (n, 0)
    tr = sim.tracers()
    assert len(tr["id"]) == n and np.all(tr["active"] == 1)
    _check_owners(sim, tr)


@BUILDS
@pytest.mark.parametrize("form", ["fused", "passes"])
def test_outflow_box_loses_tracers_and_counts_them(strict, form):
    sim = _sim("advection_3d", EULER_BOX + _bc("outflow") + USER + ["apk_amd/tracer_step=" + form], strict)
    _write_prim(sim, _uniform_state)
    sim.seed_tracers(*_random_positions(sim, 20000, seed=5))
    for _ in range(10):
        sim.step()
        active, lost = sim.tracers_count()
        assert active + lost == 20000
        tr = sim.tracers(["active"])
        assert int(np.sum(tr["active"] != 0)) == active
    assert lost > 0
    tr = sim.tracers()
    _check_owners(sim, tr)
    i = sim.info
    gone = tr["active"] == 0
    outside = np.zeros(len(gone), dtype=bool)
    for d, k in enumerate("xyz"):
        outside |= (tr[k] < i.xmin[d]) | (tr[k] >= i.xmax[d])
    assert np.array_equal(gone, outside)


# ---- 6. passivity ------------------------------------------------------------------------------------------------
HEADLINE = ["parthenon/mesh/nx1=128", "parthenon/mesh/nx2=128", "parthenon/mesh/nx3=128", "parthenon/meshblock/nx1=64",
            "parthenon/meshblock/nx2=64", "parthenon/meshblock/nx3=64"]


@BUILDS
@pytest.mark.parametrize("deck", ["synthetic_mhd", "turbulence"])
def test_tracers_leave_the_conserved_state_alone(strict, deck):
    """10 cycles with tracers on against tracers off, bit for bit.  synthetic_mhd is the headline VL2 deck (on 8 blocks
    of 64^3 here), whose cycle stores no primitives and copies no same-rank ghost zones: the completion the tracer step
    asks for must not disturb the stages."""
    base = HEADLINE if deck == "synthetic_mhd" else []
    off = _sim(deck, base, strict)
    on = _sim(deck, base + ON + TURB, strict)
    for _ in range(10):
        off.step()
        on.step()
    if deck == "synthetic_mhd":
        # (the deck is one whose cycle stores no primitives; with tracers the next cycle still derives them itself)
        assert off.prim_is_stale and on.prim_is_stale
    assert on.tracers_count()[0] > 0 and on.time == off.time and on.dt == off.dt
    assert np.array_equal(on.gather(), off.gather())


# ---- 7. size -----------------------------------------------------------------------------------------------------
def test_more_tracers_than_65535_workgroups():
    """520 tracers per cell of the 32^3 box = 17,039,360 > 65535 x 256 = 16,776,960 (two sets of arrays of 96 B per
    particle: 3.3 GB), product build: one step of uniform flow, case 1's identity with its per-step share of the bound."""
    sim = _sim("advection_3d", EULER_BOX + _bc("periodic") + ON + ["tracers/initial_seed_method=random_per_block",
                                                                     "tracers/initial_num_tracers_per_cell=520"], False)
    n = 520 * 32 ** 3
    assert n > 65535 * 256 and sim.tracers_count() == (n, 0)
    _write_prim(sim, _uniform_state)
    sim.tracers_step(0.0)  # (refill on the state just written)
    before = sim.tracers(["x", "y", "z"])
    dt = sim.dt
    sim.tracers_step(dt)
    after = sim.tracers(["x", "y", "z", "active", "vel_x"])
    i = sim.info
    assert np.array_equal(after["id"], np.arange(n)) and np.all(after["active"] == 1)
    assert np.max(np.abs(after["vel_x"] - V_UNIFORM[0])) <= 4e-16
    for d, k in enumerate("xyz"):
        L = i.xmax[d] - i.xmin[d]
        want = _wrap(before[k] + V_UNIFORM[d] * dt, i.xmin[d], i.xmax[d])
        assert _wrapped_distance(after[k], want, L).max() / L <= 1e-13
    assert sim.tracers_count() == (n, 0)


# ---- outputs -----------------------------------------------------------------------------------------------------
def test_execute_writes_the_tracers_next_to_the_history(tmp_path):
    from athenapk_amd import decks, driver
    sim = driver.Simulation(decks.load("turbulence_tracers"), ["parthenon/time/nlim=3"], strict=False)
    assert sim.execute(tmp_path) == 3
    tr = sim.tracers()
    base = os.path.join(str(tmp_path), "parthenon.out1.")
    for row in ("00000", "00001"):
        ids = np.load(base + row + ".tracers.id.npy")
        assert ids.dtype == np.int64 and np.array_equal(ids, np.sort(ids)) and len(ids) == len(tr["id"])
    for k in ["x", "y", "z", "active"] + list(T.FIELD_NAMES):
        assert np.array_equal(np.load(base + "00001.tracers.%s.npy" % k), tr[k]), k
