"""Field snapshots without a GPU: the npy output blocks as parsed, what is refused at creation, the JSON index of a
host-only sim, and the reader (athenapk_amd/snapshots.py) on files numpy wrote in the documented format."""
import json
import os

import numpy as np
import pytest

from athenapk_amd import decks, driver, snapshots
from athenapk_amd import lib as L

HYDRO8 = ["parthenon/mesh/nx1=16", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/meshblock/nx1=8",
          "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8", "parthenon/mesh/refinement=none"]
CONS_H = ["cons.rho", "cons.mom1", "cons.mom2", "cons.mom3", "cons.etot"]
PRIM_H = ["prim.rho", "prim.vel1", "prim.vel2", "prim.vel3", "prim.pressure"]
MHD = ["B1", "B2", "B3", "psi"]


def _out(n, **kv):
    return ["parthenon/output%d/%s=%s" % (n, k, v) for k, v in dict(file_type="npy", **kv).items()]


def _plan(deck, ov):
    return driver.HostPlan(decks.load(deck), ov)


# ---- 1. parsing --------------------------------------------------------------------------------------------------------
def test_defaults():
    (o,) = _plan("blast", HYDRO8 + _out(3, dt=0.1)).snapshot_outputs()
    assert o == {"number": 3, "id": "out3", "dt": 0.1, "single": False, "components": CONS_H}


def test_groups_expand_for_hydro_with_two_scalars():
    ov = HYDRO8 + ["hydro/nscalars=2"] + _out(2, dt=0.5, variables="prim, cons")
    (o,) = _plan("blast", ov).snapshot_outputs()
    assert o["components"] == PRIM_H + ["prim.r0", "prim.r1"] + CONS_H + ["cons.s0", "cons.s1"]


def test_groups_expand_for_glmmhd():
    (o,) = _plan("synthetic_mhd", _out(1, dt=0.5, variables="cons,prim")).snapshot_outputs()
    assert o["components"] == CONS_H + ["cons." + m for m in MHD] + PRIM_H + ["prim." + m for m in MHD]


def test_duplicates_collapse_and_order_is_kept():
    ov = _out(1, dt=0.5, variables="prim.pressure, cons.B2, prim, plasma_beta, prim.rho, cons.B2, mach_sonic, plasma_beta")
    (o,) = _plan("synthetic_mhd", ov).snapshot_outputs()
    rest = [p for p in PRIM_H + ["prim." + m for m in MHD] if p != "prim.pressure"]
    assert o["components"] == ["prim.pressure", "cons.B2"] + rest + ["plasma_beta", "mach_sonic"]


def test_id_and_single_precision_and_two_blocks():
    ov = _out(2, dt=0.25, id="fields", single_precision_output="true", variables="prim") + _out(5, dt=1.5, variables="B_mag")
    a, b = _plan("synthetic_mhd", ov).snapshot_outputs()
    assert (a["number"], a["id"], a["single"], a["dt"]) == (2, "fields", True, 0.25)
    assert (b["number"], b["id"], b["single"], b["dt"], b["components"]) == (5, "out5", False, 1.5, ["B_mag"])


def test_temperature_is_accepted_with_units_and_composition():
    table = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schure.cooling_1.0Z")
    ov = ["cooling/table_filename=" + table] + _out(4, dt=1.0, variables="temperature,mach_sonic")
    (o,) = _plan("cooling", ov).snapshot_outputs()
    assert o["components"] == ["temperature", "mach_sonic"]


def test_shape_on_a_host_only_sim():
    p = _plan("blast", HYDRO8 + ["parthenon/meshblock/nx1=16", "parthenon/meshblock/nx3=4"])
    names, shape, dtype = p.snapshot_shape(["prim.rho", "cons"], single=True)
    assert names == ["prim.rho"] + CONS_H and shape == (8, 6, 4, 8, 16) and dtype == np.dtype("<f4")


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------
REFUSED = {
    "unknown_entry": ("blast", HYDRO8 + _out(3, dt=0.1, variables="cons,entropy"), ["parthenon/output3", "variables", "entropy"]),
    "mhd_component_with_euler": ("blast", HYDRO8 + _out(3, dt=0.1, variables="cons.B1"), ["parthenon/output3", "variables", "cons.B1", "glmmhd"]),
    "mhd_psi_with_euler": ("blast", HYDRO8 + _out(3, dt=0.1, variables="prim.psi"), ["parthenon/output3", "variables", "prim.psi", "glmmhd"]),
    "mhd_field_with_euler": ("blast", HYDRO8 + _out(3, dt=0.1, variables="plasma_beta"), ["parthenon/output3", "variables", "plasma_beta", "glmmhd"]),
    "temperature_without_units": ("blast", HYDRO8 + _out(3, dt=0.1, variables="temperature"), ["parthenon/output3", "variables", "temperature", "units"]),
    "scalar_index": ("blast", HYDRO8 + ["hydro/nscalars=2"] + _out(3, dt=0.1, variables="cons.s2"), ["parthenon/output3", "variables", "cons.s2", "nscalars"]),
    "scalar_without_scalars": ("blast", HYDRO8 + _out(3, dt=0.1, variables="prim.r0"), ["parthenon/output3", "variables", "prim.r0", "nscalars"]),
    "dt_zero": ("blast", HYDRO8 + _out(3, dt=0.0), ["parthenon/output3", "dt"]),
    "dt_negative": ("blast", HYDRO8 + _out(7, dt=-1.0), ["parthenon/output7", "dt"]),
    "dt_missing": ("blast", HYDRO8 + _out(3), ["parthenon/output3", "dt"]),
    "empty_list": ("blast", HYDRO8 + _out(3, dt=0.1, variables=""), ["parthenon/output3", "variables", "empty"]),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_at_deck_parsing(case):
    deck, ov, words = REFUSED[case]
    with pytest.raises(L.ApkError) as e:
        _plan(deck, ov)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_hdf5_block_is_still_ignored():
    p = _plan("blast", HYDRO8 + ["parthenon/output4/file_type=hdf5", "parthenon/output4/dt=0.1", "parthenon/output4/variables=nonsense"])
    assert p.snapshot_outputs() == []


def test_api_refuses_a_bad_list_with_a_message():
    p = _plan("blast", HYDRO8)
    with pytest.raises(L.ApkError, match="cons.B3"):
        p.snapshot_shape("cons.B3")


# ---- 3. the index --------------------------------------------------------------------------------------------------------
def _check_index(p, path, names, dtype):
    with open(path) as f:
        ix = json.load(f)
    i = p.info
    assert ix["time"] == 0.0 and ix["cycle"] == 0 and ix["components"] == names and ix["dtype"] == dtype
    assert ix["fluid"] == {1: "euler", 2: "glmmhd"}[i.fluid] and ix["nscalars"] == i.nscalars
    # doubles round-trip exactly
    assert ix["gamma"] == i.gamma and ix["xmin"] == list(i.xmin) and ix["xmax"] == list(i.xmax)
    assert ix["dt"] == np.finfo(np.float64).max  # (no time step before initialisation)
    assert ix["mesh_nx"] == list(i.nx) and ix["block_nx"] == list(i.mb) and ix["nghost"] == i.ng and ix["nranks"] == 1
    assert [b["gid"] for b in ix["blocks"]] == list(range(i.nblocks_total)) and i.nblocks_total == i.nblocks_local
    for lb in range(i.nblocks_local):  # one rank: block lb of the file is local block lb
        gid, loc = p.block_gid(lb)
        b = ix["blocks"][gid]
        assert (b["rank"], b["index"]) == (0, lb)
        assert b["level"] == p.block_level(lb) and (b["lx1"], b["lx2"], b["lx3"]) == loc
    return ix


def test_index_of_a_uniform_mesh(tmp_path):
    p = _plan("blast", HYDRO8 + ["hydro/gamma=1.4000000000000001", "parthenon/mesh/x1min=-0.30000000000000004"])
    path = os.path.join(str(tmp_path), "u.json")
    p.write_snapshot_index(path, "prim.rho,cons", single=True)
    ix = _check_index(p, path, ["prim.rho"] + CONS_H, "<f4")
    assert len(ix["blocks"]) == 8 and all(b["level"] == 0 for b in ix["blocks"])


def test_index_of_a_refined_mesh(tmp_path):
    sr = ["parthenon/mesh/refinement=static", "parthenon/static_refinement0/level=2"]
    sr += ["parthenon/static_refinement0/x%d%s=%s" % (d, m, v) for d in (1, 2, 3) for m, v in (("min", -0.1), ("max", 0.1))]
    p = _plan("blast_3d_amr", sr)
    path = os.path.join(str(tmp_path), "r.json")
    p.write_snapshot_index(path)
    ix = _check_index(p, path, CONS_H, "<f8")
    assert {b["level"] for b in ix["blocks"]} == {0, 1, 2}


def test_index_over_two_ranks_places_every_block_once(tmp_path):
    path = os.path.join(str(tmp_path), "two.json")
    plans = [driver.HostPlan(decks.load("blast"), HYDRO8, rank=r, nranks=2) for r in range(2)]
    plans[0].write_snapshot_index(path)
    with open(path) as f:
        ix = json.load(f)
    assert ix["nranks"] == 2
    for r, p in enumerate(plans):
        for lb in range(p.info.nblocks_local):
            b = ix["blocks"][p.block_gid(lb)[0]]
            assert (b["rank"], b["index"]) == (r, lb)


# ---- 4. the reader on synthetic files --------------------------------------------------------------------------------------
def _write_synthetic(tmp, blocks, mesh_nx, refined_extra=None):
    """numpy writes a dump: two ranks, the given blocks (gid, level, lx) dealt out in a shuffled order"""
    rng = np.random.default_rng(5)
    nx1, nx2, nx3 = 6, 2, 4
    comps = ["cons.rho", "prim.pressure", "mach_sonic"]
    order = rng.permutation(len(blocks))
    table, data = [], {}
    per_rank = [[], []]
    for pos, q in enumerate(order):
        gid, level, lx = blocks[q]
        r = pos % 2
        a = rng.standard_normal((len(comps), nx3, nx2, nx1))
        table.append({"gid": gid, "level": level, "lx1": lx[0], "lx2": lx[1], "lx3": lx[2], "rank": r, "index": len(per_rank[r])})
        per_rank[r].append(a)
        data[gid] = a
    table.sort(key=lambda b: b["gid"])
    prefix = os.path.join(str(tmp), "syn.out1.00000")
    for r in range(2):
        np.save(prefix + ".rank%d.npy" % r, np.stack(per_rank[r]))
    ix = {"time": 0.125, "cycle": 7, "dt": 0.001, "components": comps, "dtype": "<f8", "fluid": "euler", "gamma": 1.4,
          "nscalars": 0, "xmin": [-1.0, 0.0, -0.5], "xmax": [1.0, 1.0, 0.5], "mesh_nx": list(mesh_nx),
          "block_nx": [nx1, nx2, nx3], "nghost": 2, "nranks": 2, "blocks": table}
    with open(prefix + ".json", "w") as f:
        json.dump(ix, f)
    return prefix + ".json", data, comps


def test_reader_assembles_a_uniform_mesh(tmp_path):
    blocks = [(g, 0, (g % 2, (g // 2) % 2, g // 4)) for g in range(8)]
    path, data, comps = _write_synthetic(tmp_path, blocks, (12, 4, 8))
    snap = snapshots.load(path)
    assert (snap.time, snap.cycle, snap.dt, snap.components) == (0.125, 7, 0.001, comps)
    assert [b["gid"] for b in snap.blocks] == list(range(8))
    for c, name in enumerate(comps):
        want = np.empty((8, 4, 12))
        for g, _, (i, j, k) in blocks:
            want[4 * k:4 * k + 4, 2 * j:2 * j + 2, 6 * i:6 * i + 6] = data[g][c]
        assert np.array_equal(snap.component(name), want)
    for g in range(8):
        assert np.array_equal(snap.block(g), data[g])
    assert snap.block_bounds(5) == ((0.0, 0.0, 0.0), (1.0, 0.5, 0.5))


def test_reader_on_a_refined_mesh(tmp_path):
    # a 2 x 1 x 1 root grid whose block 0 is split: 1 + 8 blocks (one left out of the files' 8: seven children + the root)
    blocks = [(0, 0, (1, 0, 0))] + [(1 + c, 1, (c % 2, (c // 2) % 2, c // 4)) for c in range(7)]
    path, data, comps = _write_synthetic(tmp_path, blocks, (12, 2, 4))
    snap = snapshots.load(path)
    assert snap.refined
    with pytest.raises(ValueError, match="iterate over"):
        snap.component("cons.rho")
    # level 1, lx = (1, 1, 0): cells half as wide, so the block spans a quarter of x1 (2 / 2 / 2 wide), half of x2 and x3
    gid = [b[0] for b in blocks if b[1] == 1 and b[2] == (1, 1, 0)][0]
    assert snap.block_bounds(gid) == ((-0.5, 0.5, -0.5), (0.0, 1.0, 0.0))
    assert snap.block_bounds(0) == ((0.0, 0.0, -0.5), (1.0, 1.0, 0.5))
    assert np.array_equal(snap.block(gid), data[gid])


@pytest.mark.parametrize("deck,ncomp", [("turbulence_snapshots", 9), ("blast_3d_amr_snapshots", 5)])
def test_shipped_snapshot_decks_parse(deck, ncomp):
    (o,) = _plan(deck, []).snapshot_outputs()
    assert o["number"] == 2 and o["id"] == "out2" and o["single"] and len(o["components"]) == ncomp
    assert all(c.startswith("prim.") for c in o["components"])
    # the decks they extend have no snapshot output: the runs existing tests make of them write what they wrote
    assert _plan(deck[:-len("_snapshots")], []).snapshot_outputs() == []
