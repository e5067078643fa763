"""CPU tests of the tracer particles' host side (no GPU): the <tracers> options as parsed, every refusal with its
message, and random_per_block seeding against the numpy generator of tests/tracers_reference.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracers_reference as T  # noqa: E402

ON = ["tracers/enabled=true"]


def _plan(deck="turbulence", overrides=(), rank=0, nranks=1):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides), rank=rank, nranks=nranks)


def test_disabled_by_default_and_reported():
    o = _plan().tracers_options()
    assert o["enabled"] is False and o["nfields"] == 0


def test_options_are_parsed_and_reported():
    o = _plan(overrides=ON + ["tracers/initial_seed_method=random_per_block", "tracers/initial_num_tracers_per_cell=0.125",
                              "tracers/initial_rng_seed=42"]).tracers_options()
    assert o == {"enabled": True, "initial_seed_method": "random_per_block", "tracer_step": "fused", "nfields": 8,
                 "initial_num_tracers_per_cell": 0.125, "initial_rng_seed": 42,
                 "num_tracers_per_block": int(64 * 32 * 32 * 0.125)}
    o = _plan(overrides=ON + ["tracers/initial_seed_method=user", "apk_amd/tracer_step=passes", "hydro/fluid=euler",
                              "hydro/riemann=hlle"]).tracers_options()
    assert o["initial_seed_method"] == "user" and o["tracer_step"] == "passes" and o["nfields"] == 5
    assert _plan(overrides=ON).tracers_options()["initial_seed_method"] == "none"


def test_the_tracer_deck_enables_them():
    o = _plan("turbulence_tracers").tracers_options()
    assert o["enabled"] and o["initial_seed_method"] == "random_per_block" and o["num_tracers_per_block"] > 0
    assert o["nfields"] == 8 and o["tracer_step"] == "fused"


REFUSALS = {
    "two_dimensions": ("orszag_tang", ON, 1, "only supported/tested in 3D"),
    "adaptive": ("blast_3d_amr", ON, 1, "only supported on uniform meshes"),
    "static": ("blast_3d_amr", ON + ["parthenon/mesh/refinement=static"], 1, "only supported on uniform meshes"),
    "two_ranks": ("turbulence", ON, 2, "tracers need a single rank for now"),
    "one_ghost_layer": ("advection_3d", ON + ["parthenon/mesh/refinement=none", "parthenon/mesh/nghost=1",
                                        "hydro/reconstruction=dc"], 1, "nghost >= 2"),
    "unknown_method": ("turbulence", ON + ["tracers/initial_seed_method=lattice"], 1, "Unknown tracer initial_seed_method"),
    "no_count": ("turbulence", ON + ["tracers/initial_seed_method=random_per_block"], 1, "seed at least some tracers"),
    "negative_count": ("turbulence", ON + ["tracers/initial_seed_method=random_per_block",
                                           "tracers/initial_num_tracers_per_cell=-1"], 1, "seed at least some tracers"),
    "count_rounds_to_zero": ("turbulence", ON + ["tracers/initial_seed_method=random_per_block",
                                                 "tracers/initial_num_tracers_per_cell=1e-9"], 1,
                             "number of particles per block is invalid"),
    "unknown_form": ("turbulence", ON + ["apk_amd/tracer_step=both"], 1, "tracer_step must be fused or passes"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_carry_their_message(case):
    from athenapk_amd import lib as L
    deck, ov, nranks, msg = REFUSALS[case]
    _plan(deck, [o for o in ov if not o.startswith("tracers/enabled")], nranks=nranks)  # (accepted without tracers)
    with pytest.raises(L.ApkError) as e:
        _plan(deck, ov, nranks=nranks)
    assert msg in str(e.value)


BLOCKS = {1: (32, 32, 32), 8: (16, 16, 16), 64: (8, 8, 8)}


@pytest.mark.parametrize("nblocks", sorted(BLOCKS))
def test_seeding_matches_the_numpy_generator(nblocks):
    """The same 32^3 cells cut into 1, 8 and 64 blocks: for each cut the positions drawn on the host are identical to
    the numpy generator's, every position lies inside its block, and the ids are unique and the reference's
    (n_per_block * gid + n).  (The generator is keyed on the block, as the reference's pool is seeded per block: the
    three cuts are three different sets of positions, each reproduced exactly.)"""
    mb = BLOCKS[nblocks]
    ov = ON + ["parthenon/mesh/refinement=none", "parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32",
               "parthenon/mesh/x1min=-0.5", "parthenon/mesh/x1max=1.0", "parthenon/mesh/x2min=0.25", "parthenon/mesh/x2max=0.75",
               "parthenon/mesh/x3min=0.0", "parthenon/mesh/x3max=1.0",
               "parthenon/meshblock/nx1=%d" % mb[0], "parthenon/meshblock/nx2=%d" % mb[1], "parthenon/meshblock/nx3=%d" % mb[2],
               "tracers/initial_seed_method=random_per_block", "tracers/initial_num_tracers_per_cell=0.3",
               "tracers/initial_rng_seed=7"]
    plan = _plan("advection_3d", ov)
    got = plan.seeded_tracers()
    grid = T.Grid((-0.5, 0.25, 0.0), (1.0, 0.75, 1.0), (32, 32, 32), mb, 2)
    want = T.seed_random_per_block(grid, 0.3, 7)
    per_block = int(mb[0] * mb[1] * mb[2] * 0.3)
    assert len(got["id"]) == nblocks * per_block == len(want["id"])
    assert np.array_equal(got["id"], want["id"]) and len(np.unique(got["id"])) == len(got["id"])
    for k in "xyz":
        assert np.array_equal(got[k], want[k]), k
    # every particle inside the block that owns it (local index -> gid -> origin)
    for q in range(0, len(got["id"]), max(1, len(got["id"]) // 997)):
        gid, _ = plan.block_gid(int(got["block"][q]))
        assert gid == want["gid"][q] == got["id"][q] // per_block
        o = grid.origin(gid)
        for d, k in enumerate("xyz"):
            assert o[d] <= got[k][q] <= o[d] + grid.block_size[d]
    assert np.array_equal(T.owner(grid, got["x"], got["y"], got["z"]), want["gid"])


def test_seeding_depends_on_the_seed_only_through_the_key():
    """initial_rng_seed + gid is the key: with seed 3, block 1 draws what block 0 draws with seed 4, relative to its
    origin -- through the host library, and against the numpy generator"""
    ov = ON + ["parthenon/mesh/refinement=none", "parthenon/mesh/nx1=16", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16",
               "parthenon/mesh/x1min=0.0", "parthenon/mesh/x1max=1.0", "parthenon/mesh/x2min=0.0", "parthenon/mesh/x2max=1.0",
               "parthenon/mesh/x3min=0.0", "parthenon/mesh/x3max=1.0",
               "parthenon/meshblock/nx1=8", "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8",
               "tracers/initial_seed_method=random_per_block", "tracers/initial_num_tracers_per_cell=0.5"]
    a = _plan("advection_3d", ov + ["tracers/initial_rng_seed=3"]).seeded_tracers()
    b = _plan("advection_3d", ov + ["tracers/initial_rng_seed=4"]).seeded_tracers()
    g = T.Grid((0, 0, 0), (1, 1, 1), (16, 16, 16), (8, 8, 8), 2)
    per = len(a["id"]) // 8
    assert per == 256 and not np.array_equal(a["x"], b["x"])
    for d, k in enumerate("xyz"):
        # (origin + r * size with the same r: equal up to the rounding of the two sums)
        assert np.allclose(a[k][per:2 * per] - g.origin(1)[d], b[k][:per] - g.origin(0)[d], rtol=0, atol=1e-15), k
        assert np.array_equal(a[k], T.seed_random_per_block(g, 0.5, 3)[k])
    r = T.uniform(11, np.arange(100000, dtype=np.uint64), 0)
    assert 0.0 <= r.min() and r.max() < 1.0 and abs(r.mean() - 0.5) < 0.01
