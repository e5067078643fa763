"""Field snapshots on the GPU: the fused pack kernel (apk_output_pack) through Simulation.snapshot / write_snapshot /
execute, in both builds, against what the block accessors deliver for the same state -- and the property the accessors do
not have: a snapshot leaves the run alone."""
import functools
import glob
import json
import os
import sys

import numpy as np
import pytest

from _spawn import spawn
from test_gpu_parity import FAST_TOL, _cmp  # noqa: F401  (the existing comparison rules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])


def _mesh(nx, mb):
    return ["parthenon/mesh/nx%d=%d" % (d + 1, n) for d, n in enumerate(nx)] + \
           ["parthenon/meshblock/nx%d=%d" % (d + 1, n) for d, n in enumerate(mb)]


HYDRO = ["hydro/fluid=euler", "hydro/riemann=hllc", "hydro/reconstruction=plm", "parthenon/mesh/nghost=2"]
CASES = {
    # the smallest shapes at which the kernel can go wrong
    "hydro_8cubed_ng2": ("synthetic_mhd", HYDRO + _mesh((16, 16, 16), (8, 8, 8))),
    "hydro_scalars_24x8x4": ("synthetic_mhd", HYDRO + ["hydro/nscalars=2"] + _mesh((48, 8, 8), (24, 8, 4))),
    "mhd_16cubed_x8": ("synthetic_mhd", _mesh((32, 32, 32), (16, 16, 16))),
    "mhd_padded_rows_64x16x16": ("synthetic_mhd", _mesh((64, 16, 16), (64, 16, 16)) + ["apk_amd/row_pitch=aligned"]),
    "orszag_tang_2d": ("orszag_tang", _mesh((32, 32, 1), (16, 16, 1))),
    "sod_1d": ("sod", _mesh((64, 1, 1), (32, 1, 1))),
}


def _sim(deck, ov, strict):
    from athenapk_amd import decks, driver
    return driver.Simulation(decks.load(deck), ov, strict=strict)


def _interior(s, a):
    """the interior cells of a block as read_block delivers it"""
    i = s.info
    sl = [slice(None)] + [slice(i.ng, i.ng + i.mb[d]) if i.mb[d] > 1 else slice(0, 1) for d in (2, 1, 0)]
    return a[tuple(sl)]


def _accessor(s, field):
    return np.stack([_interior(s, s.read_block(lb, field)) for lb in range(s.info.nblocks_local)])


@functools.lru_cache(maxsize=None)
def _state(case, strict):
    """three cycles, then the snapshot FIRST and the accessors after it; shared by the tests below, never written to"""
    deck, ov = CASES[case]
    s = _sim(deck, ov, strict).initialize()
    for _ in range(3):
        s.step()
    names, snap = s.snapshot(["cons", "prim"])
    return s, names, snap, _accessor(s, "cons"), _accessor(s, "prim")


# ---- 5. against the existing accessors --------------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("case", sorted(CASES))
def test_snapshot_equals_the_block_accessors(case, strict):
    s, names, snap, cons, prim = _state(case, strict)
    i = s.info
    nvar = i.nhydro + i.nscalars
    assert snap.shape == (i.nblocks_local, 2 * nvar, i.mb[2], i.mb[1], i.mb[0]) and snap.dtype == np.float64
    assert len(names) == 2 * nvar and names[0] == "cons.rho" and names[nvar] == "prim.rho"
    assert np.all(np.isfinite(snap)), "padding (NaN) or garbage in the dump"
    assert np.array_equal(snap[:, :nvar], cons), "cons differs from read_block"
    _cmp(snap[:, nvar:], prim, strict, "prim")
    assert np.ptp(snap[:, 0]) > 0  # (not a uniform state)


# ---- 6. single components and order -----------------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
def test_single_components_in_the_order_asked_for(strict):
    s, names, snap, _, _ = _state("mhd_16cubed_x8", strict)
    want = ["prim.pressure", "cons.B2", "prim.rho"]
    got_names, got = s.snapshot(want)
    assert got_names == want and got.shape[1] == 3
    for c, n in enumerate(want):
        assert np.array_equal(got[:, c], snap[:, names.index(n)]), n


@pytest.mark.gpu
def test_scalar_components_alone():
    s, names, snap, _, _ = _state("hydro_scalars_24x8x4", True)
    want = ["prim.r1", "cons.s0", "cons.s1", "prim.rho", "prim.r0"]
    got_names, got = s.snapshot(",".join(want))
    assert got_names == want
    for c, n in enumerate(want):
        assert np.array_equal(got[:, c], snap[:, names.index(n)]), n
    assert np.ptp(got[:, 1]) > 0


# ---- 7. fp32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("case", ["mhd_16cubed_x8", "hydro_scalars_24x8x4"])
def test_single_precision_is_the_rounded_double(case, strict):
    s, names, snap, _, _ = _state(case, strict)
    got_names, got = s.snapshot(["cons", "prim"], single=True)
    assert got_names == names and got.dtype == np.float32
    assert np.array_equal(got, snap.astype(np.float32))


# ---- 8. derived fields ------------------------------------------------------------------------------------------------
def _derived(prim, gamma, mbar_over_kb, mhd):
    """the formulas of include/apk_amd.h on [nb][nvar][k][j][i] primitives, operation for operation"""
    rho, v1, v2, v3, P = (prim[:, n] for n in range(5))
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        v_mag = np.sqrt(v1 * v1 + v2 * v2 + v3 * v3)
        c_s = np.sqrt(gamma * P / rho)
        out["mach_sonic"] = v_mag / c_s
        out["temperature"] = mbar_over_kb * P / rho
        if mhd:
            B2 = prim[:, 5] * prim[:, 5] + prim[:, 6] * prim[:, 6] + prim[:, 7] * prim[:, 7]
            out["B_mag"] = np.sqrt(B2)
            out["mach_alfven"] = out["mach_sonic"] * c_s / np.sqrt(B2 / rho)
            out["plasma_beta"] = np.where(B2 != 0, P / (0.5 * B2), np.nan)
    return out


@pytest.mark.gpu
@BOTH
def test_derived_fields_of_glmmhd_with_a_field_free_cell(strict):
    deck, ov = CASES["mhd_16cubed_x8"]
    s = _sim(deck, ov, strict).initialize()
    s.step()
    u = s.read_block(3, "cons")
    cell = (slice(None), s.info.ng + 5, s.info.ng + 2, s.info.ng + 11)
    assert u[1][cell[1:]] != 0.0  # (a moving cell: mach_alfven = inf, not 0 / 0)
    u[(slice(5, 8),) + cell[1:]] = 0.0
    s.write_block(3, u, "cons")
    fields = ["mach_sonic", "B_mag", "mach_alfven", "plasma_beta"]
    names, snap = s.snapshot(["prim"] + fields)
    want = _derived(snap[:, :9], s.info.gamma, 1.0, True)
    at = (3, slice(None), 5, 2, 11)
    assert np.isnan(snap[at][names.index("plasma_beta")]) and np.isposinf(snap[at][names.index("mach_alfven")])
    assert snap[at][names.index("B_mag")] == 0.0
    for f in fields:
        got = snap[:, names.index(f)]
        assert np.array_equal(np.isnan(got), np.isnan(want[f])) and np.array_equal(np.isinf(got), np.isinf(want[f])), f
        _cmp(got, want[f], strict, f)
    assert np.isnan(want["plasma_beta"]).sum() == 1 and np.isinf(want["mach_alfven"]).sum() == 1


@pytest.mark.gpu
@BOTH
def test_temperature_with_units(strict):
    from athenapk_amd import decks, driver
    table = os.path.join(ROOT, "tests", "golden", "schure.cooling_1.0Z")
    s = driver.Simulation(decks.load("cooling"), ["cooling/table_filename=" + table], strict=strict).initialize()
    u = s.read_block(0, "cons")
    k, j, i = np.meshgrid(*(np.arange(n) for n in u.shape[1:]), indexing="ij")
    u[0] = u[0] * (1.0 + 0.25 * np.sin(0.9 * i - 0.4 * k))  # a density contrast and subsonic motion on the uniform gas
    u[1] = 0.05 * u[0] * np.sin(0.7 * i + 0.3 * j)           # (its sound speed is 0.13)
    u[2] = 0.03 * u[0] * np.cos(0.5 * k)
    u[4] = u[4] + 0.5 * (u[1] ** 2 + u[2] ** 2) / u[0]
    s.write_block(0, u, "cons")
    mbar_over_kb = driver.HostPlan(decks.load("cooling"), ["cooling/table_filename=" + table]).units().mbar_over_kb
    assert mbar_over_kb > 0
    names, snap = s.snapshot("prim, temperature, mach_sonic")
    want = _derived(snap[:, :5], s.info.gamma, mbar_over_kb, False)
    for f in ("temperature", "mach_sonic"):
        _cmp(snap[:, names.index(f)], want[f], strict, f)
    T = snap[:, names.index("temperature")]
    assert np.ptp(T) > 0 and 1e4 < T.min() and T.max() < 1e8  # kelvin: the deck's gas is at 7e5 K


# ---- 9. chunking ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_chunks_the_last_one_partial(tmp_path):
    """18 double components of a 16^3 block are 0.5625 MiB: 2 MB of staging hold three blocks, so 8 blocks go 3 + 3 + 2"""
    s0, names, snap, _, _ = _state("mhd_16cubed_x8", True)
    deck, ov = CASES["mhd_16cubed_x8"]
    s = _sim(deck, ov + ["apk_amd/snapshot_staging_mb=2"], True).initialize()
    for _ in range(3):
        s.step()
    got_names, got = s.snapshot(["cons", "prim"])
    assert got_names == names and np.array_equal(got, snap)
    a, b = os.path.join(str(tmp_path), "chunked"), os.path.join(str(tmp_path), "whole")
    s.write_snapshot(a, ["cons", "prim"])
    s0.write_snapshot(b, ["cons", "prim"])
    for ext in (".rank0.npy", ".json"):
        with open(a + ext, "rb") as fa, open(b + ext, "rb") as fb:
            assert fa.read() == fb.read(), ext
    assert np.array_equal(np.load(a + ".rank0.npy"), snap)
    # (a bound below one block is raised to one block: eight chunks)
    t = _sim(deck, ov + ["apk_amd/snapshot_staging_mb=0.01"], True).initialize()
    for _ in range(3):
        t.step()
    assert np.array_equal(t.snapshot(["cons", "prim"])[1], snap)


# ---- 10. more than 65535 rows -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_rows_than_a_grid_dimension_holds():
    """64 GLM-MHD blocks of 16^3: 64 * 9 * 16 * 16 = 147456 component rows"""
    s = _sim("synthetic_mhd", _mesh((64, 64, 64), (16, 16, 16)), True).initialize()
    s.step()
    names, snap = s.snapshot(["cons", "prim.pressure"])
    assert snap.shape == (64, 10, 16, 16, 16)
    assert np.array_equal(snap[:, :9], _accessor(s, "cons"))
    assert np.array_equal(snap[:, 9], _accessor(s, "prim")[:, 4])


# ---- 11. a snapshot leaves the run alone ------------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
def test_snapshots_do_not_change_the_run(strict):
    deck, ov = CASES["mhd_16cubed_x8"]
    plain, dumped = _sim(deck, ov, strict).initialize(), _sim(deck, ov, strict).initialize()

    def flags(s):
        return (s.prim_is_stale, s.thin_exchanges(), s.x1_direct_exchanges(), s.skipped_local_exchanges())

    stale_seen = False
    for cyc in range(6):
        plain.step()
        dumped.step()
        before = flags(dumped)
        dumped.snapshot(["prim"])
        assert flags(dumped) == before == flags(plain), "cycle %d" % cyc
        stale_seen = stale_seen or plain.prim_is_stale
    assert stale_seen, "the plain run never kept its primitives out of memory: this deck shows nothing"
    assert plain.time == dumped.time and plain.dt == dumped.dt
    assert np.array_equal(plain.gather("cons"), dumped.gather("cons"))


# ---- 12. floors -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
def test_a_floor_changes_the_dump_not_the_state(strict):
    deck, ov = CASES["hydro_8cubed_ng2"]
    s = _sim(deck, ov + ["hydro/dfloor=0.01"], strict).initialize()
    s.step()
    ng = s.info.ng
    u = s.read_block(2, "cons")
    u[0, ng + 3, ng + 1, ng + 6] = 1e-5
    s.write_block(2, u, "cons")
    names, a = s.snapshot(["cons.rho", "prim.rho", "prim.vel1"])
    assert a[2, 0, 3, 1, 6] == 1e-5 and a[2, 1, 3, 1, 6] == 0.01  # the raw value / the floor
    assert abs(a[2, 2, 3, 1, 6] - u[1, ng + 3, ng + 1, ng + 6] / 0.01) <= 1e-13 * abs(a[2, 2, 3, 1, 6])  # v = M / floor
    others = np.ones(a.shape[2:], dtype=bool)
    others[3, 1, 6] = False
    assert np.array_equal(a[2, 0][others], a[2, 1][others])  # no other cell is below the floor
    # the state in memory kept the raw value: a second dump shows it again
    assert np.array_equal(s.snapshot(["cons.rho", "prim.rho", "prim.vel1"])[1], a)


# ---- 13. execute ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_execute_writes_dumps_at_the_cadence_of_the_history(tmp_path):
    from athenapk_amd import snapshots
    deck, ov = CASES["hydro_8cubed_ng2"]
    ov = ov + ["parthenon/time/nlim=8", "parthenon/output1/file_type=hst", "parthenon/output1/dt=0.02",
               "parthenon/output1/data_format=%25.17e", "parthenon/output2/file_type=npy", "parthenon/output2/dt=0.02",
               "parthenon/output2/variables=cons.rho,prim", "parthenon/output2/id=fields",
               "parthenon/output3/file_type=hdf5", "parthenon/output3/dt=0.02"]
    s = _sim(deck, ov, False)
    assert s.execute(tmp_path) == 8
    hst = np.atleast_2d(np.genfromtxt(os.path.join(str(tmp_path), "parthenon.out1.hst")))
    n = len(hst)
    assert n >= 4, "the deck must give the initial dump, at least two on the cadence and the final one: %d rows" % n
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(tmp_path), "parthenon.fields.*"))) == sorted(
        "parthenon.fields.%05d.%s" % (q, e) for q in range(n) for e in ("json", "rank0.npy"))
    for q in range(n):
        snap = snapshots.load(os.path.join(str(tmp_path), "parthenon.fields.%05d.json" % q))
        assert snap.time == hst[q, 0] and snap.cycle == int(hst[q, 2]) and snap.dt == hst[q, 1]
        assert snap.components[0] == "cons.rho" and len(snap.components) == 6
    assert snap.cycle == 8 and hst[0, 2] == 0
    assert np.array_equal(snap.component("cons.rho"), s.gather("cons")[0])
    _cmp(snap.component("prim.pressure"), s.gather("prim")[4], False, "prim.pressure")


# ---- 14. refined mesh -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
def test_refined_mesh_dump_and_its_table(tmp_path, strict):
    from athenapk_amd import snapshots
    # the deck's 4 x 4 x 4 root blocks of 8^3 with one level of refinement (a 2 x 2 x 2 root grid refines everywhere)
    s = _sim("blast_3d_amr", ["parthenon/mesh/numlevel=2"], strict).initialize()
    for _ in range(2):
        s.step()
    nb = s.refresh_info().nblocks_total
    assert nb > 64 and nb == s.info.nblocks_local
    prefix = os.path.join(str(tmp_path), "amr.00000")
    s.write_snapshot(prefix, ["cons", "prim"])
    snap = snapshots.load(prefix + ".json")
    assert len(snap.blocks) == nb and {b["level"] for b in snap.blocks} == {0, 1}
    cons, prim = _accessor(s, "cons"), _accessor(s, "prim")
    for lb in range(nb):
        gid, loc = s.block_gid(lb)
        b = snap.blocks[gid]
        assert (b["gid"], b["rank"], b["index"]) == (gid, 0, lb)
        assert b["level"] == s.block_level(lb) and (b["lx1"], b["lx2"], b["lx3"]) == loc
        assert np.array_equal(snap.block(gid)[:5], cons[lb])
        _cmp(np.asarray(snap.block(gid)[5:]), prim[lb], strict, "prim of block %d" % gid)
    with pytest.raises(ValueError, match="iterate over"):
        snap.component("cons.rho")
    # a regridding pass that changes the mesh: refine one root block more
    tags = [0] * nb
    tags[[lb for lb in range(nb) if s.block_level(lb) == 0][0]] = 1
    assert s.apply_tags(tags)
    nb2 = s.refresh_info().nblocks_total
    assert nb2 > nb
    names, dump = s.snapshot("cons")
    assert dump.shape[0] == nb2 and np.array_equal(dump, _accessor(s, "cons"))
    s.write_snapshot(os.path.join(str(tmp_path), "amr.00001"), "cons")
    assert len(snapshots.load(os.path.join(str(tmp_path), "amr.00001.json")).blocks) == nb2


# ---- 15. two ranks ----------------------------------------------------------------------------------------------------
VARS2 = ["cons", "prim", "plasma_beta"]


def _worker(rank, world, port, prefix):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from athenapk_amd import decks, driver

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        deck, ov = CASES["mhd_16cubed_x8"]
        s = driver.Simulation(decks.load(deck), ov, rank=rank, nranks=world, strict=True).initialize()
        for _ in range(3):
            s.step()
        s.write_snapshot(prefix, VARS2)  # (no collective: the ranks do not wait for each other here)
        dist.barrier()
        s.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_dump_equals_the_one_rank_dump(tmp_path):
    from athenapk_amd import snapshots
    s, names, snap, _, _ = _state("mhd_16cubed_x8", True)
    one = os.path.join(str(tmp_path), "one")
    s.write_snapshot(one, VARS2)
    two = os.path.join(str(tmp_path), "two")
    spawn(_worker, lambda port: (2, port, two), 2)
    a, b = snapshots.load(one + ".json"), snapshots.load(two + ".json")
    assert b.index["nranks"] == 2 and sorted({k["rank"] for k in b.blocks}) == [0, 1]
    assert (a.time, a.cycle, a.dt, a.components) == (b.time, b.cycle, b.dt, b.components)
    for name in a.components:
        assert np.array_equal(a.component(name), b.component(name), equal_nan=True), name
    assert np.array_equal(a.component("cons.etot"), s.gather("cons")[4])


# ---- the command line on a shipped snapshot deck ----------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_leaves_loadable_dumps(tmp_path, capsys):
    """inputs/blast_3d_amr_snapshots.in (prim, single precision, every 0.02) cut short: the dump of t = 0 and the final one"""
    from athenapk_amd import __main__ as cli
    from athenapk_amd import snapshots
    assert cli.main(["-i", "blast_3d_amr_snapshots", "-d", str(tmp_path), "parthenon/time/tlim=0.004"]) == 0
    assert "zone-cycles/wallsecond" in capsys.readouterr().out
    paths = sorted(glob.glob(os.path.join(str(tmp_path), "parthenon.out2.*.json")))
    assert [os.path.basename(p) for p in paths] == ["parthenon.out2.00000.json", "parthenon.out2.00001.json"]
    first, last = snapshots.load(paths[0]), snapshots.load(paths[1])
    assert first.time == 0.0 and first.cycle == 0 and last.time >= 0.004 and last.cycle > 0
    assert last.components == ["prim.rho", "prim.vel1", "prim.vel2", "prim.vel3", "prim.pressure"] and last.dtype == np.float32
    for snap in (first, last):
        assert snap.refined and len(snap.blocks) > 64
        for b in snap.blocks:
            a = snap.block(b["gid"])
            assert a.shape == (5, 8, 8, 8) and np.all(np.isfinite(a)) and np.all(a[0] > 0) and np.all(a[4] > 0)
