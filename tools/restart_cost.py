"""Cost of restart dumps on one MI355X (product build, GLM-MHD), one process; writes JSON rows to the file given as the
first argument (default out/restart_cost.jsonl; profiles/restart_cost.jsonl is such a run) and prints the README's cost
sentence made of them.

(a) apk_restart_unpack alone, device events (warm-up, then 50 launches per window, 5 windows, medians), on the 8 x 128^3
    pack and on a 512 x 16^3 pack -- each next to a device copy of its algorithmic bytes (nvar * 8 read + nvar * 8 written
    per interior cell) timed in the same run: the kernel's time over that copy says how far from the stream rate it is.
(b) Simulation.restore(path) end to end (wall clock around a synchronised call, a new Simulation each time, the dump's
    files in the page cache) against the only other way to load a state: write_block over all blocks (with ghost zones,
    from host arrays already in memory), then exchange_ghosts and fill_derived.
(c) Simulation.write_restart(prefix) end to end against write_snapshot(prefix, "cons") on the same state: what the state
    file and the second name cost on top of the field snapshot the dump is made of.
Not measured: hydro packs, refined meshes, more than one GPU, files that are not in the page cache."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from athenapk_amd import decks, driver, hydro, restart  # noqa: E402

LAUNCHES, WINDOWS, REPS = 50, 5, 3
dev = torch.device("cuda")
rows = []


def window_times(launch):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / LAUNCHES * 1e-3)
    return times


def kernel_rows():
    ctx = hydro.Context(strict=False)
    lib = ctx.lib
    for nb, n in ((8, 128), (512, 16)):
        ng = 3
        md = hydro.MeshData(ctx, (n, n, n), ng, 9, dx=(0.01, 0.01, 0.01), nblocks=nb, with_flux=False)
        cells = nb * n ** 3
        src = torch.empty(cells * 9, dtype=torch.float64, device=dev).normal_()

        def launch():
            rc = lib.apk_restart_unpack(ctx.h, md.h, 0, nb, src.data_ptr(), None)
            assert rc == 0, rc

        times = window_times(launch)
        inner = (slice(None), slice(None)) + (slice(ng, ng + n),) * 3
        assert torch.equal(md.cons[inner].reshape(-1), src)  # (it is the copy it is timed as)
        nbytes = 2 * 9 * 8
        a = torch.empty(cells * 9, dtype=torch.float64, device=dev).normal_()
        b = torch.empty_like(a)
        ctimes = window_times(lambda: b.copy_(a))
        tm, cm = float(np.median(times)), float(np.median(ctimes))
        rows.append({"what": "apk_restart_unpack", "build": "product", "fluid": "glmmhd", "blocks": nb, "block": n, "cells": cells,
                     "seconds_per_launch_median": tm, "seconds_per_launch_min": min(times), "seconds_per_launch_max": max(times),
                     "ns_per_cell": tm / cells * 1e9, "bytes_per_cell": nbytes, "tb_per_s": nbytes * cells / tm * 1e-12,
                     "copy_same_bytes_seconds": cm, "copy_tb_per_s": nbytes * cells / cm * 1e-12, "time_over_copy": tm / cm,
                     "launches_per_window": LAUNCHES, "windows": WINDOWS, "timer": "device events"})
        print(rows[-1], flush=True)
        del md, src, a, b
    ctx.close()


def _mesh(nx, mb):
    return ["parthenon/mesh/nx%d=%d" % (d + 1, nx) for d in range(3)] + ["parthenon/meshblock/nx%d=%d" % (d + 1, mb) for d in range(3)]


def _timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def end_to_end_rows(tmp):
    for nx, mb in ((256, 128), (128, 16)):
        ov = _mesh(nx, mb)
        w = driver.Simulation(decks.load("synthetic_mhd"), ov, strict=False).initialize()
        for _ in range(2):
            w.step()
        nlb = w.info.nblocks_local
        dump, snap = os.path.join(tmp, "dump%d" % mb), os.path.join(tmp, "snap%d" % mb)
        w.write_restart(dump)  # (first use allocates the staging buffers)
        t_rst, t_snap = [], []
        for _ in range(REPS):
            t_rst.append(_timed(lambda: w.write_restart(dump)))
            t_snap.append(_timed(lambda: w.write_snapshot(snap, "cons")))
        tr, ts = float(np.median(t_rst)), float(np.median(t_snap))
        nbytes = os.path.getsize(dump + ".rank0.npy")
        rows.append({"what": "Simulation.write_restart vs write_snapshot('cons')", "build": "product", "fluid": "glmmhd", "blocks": nlb,
                     "block": mb, "write_restart_seconds_median": tr, "write_restart_seconds_all": t_rst,
                     "write_snapshot_seconds_median": ts, "write_snapshot_seconds_all": t_snap, "restart_over_snapshot": tr / ts,
                     "array_file_bytes": nbytes, "state_file_bytes": os.path.getsize(dump + ".rst"), "repetitions": REPS,
                     "timer": "wall clock, device synchronised"})
        print(rows[-1], flush=True)
        # the state as the accessors deliver it, for the write_block path (not timed)
        blocks = [w.read_block(lb, "cons") for lb in range(nlb)]
        want = w.snapshot("cons")[1]
        w.close()
        del w
        text = restart.deck(dump + ".rst")
        t_res, t_wb = [], []
        for _ in range(REPS):
            r = driver.Simulation(text, [], strict=False)
            t_res.append(_timed(lambda: r.restore(dump + ".rst")))
            assert np.array_equal(r.snapshot("cons")[1], want)
            r.close()
            del r
            s = driver.Simulation(decks.load("synthetic_mhd"), ov, strict=False).initialize()

            def load():
                for lb in range(nlb):
                    s.write_block(lb, blocks[lb], "cons")
                s.exchange_ghosts()
                s.fill_derived()

            t_wb.append(_timed(load))
            assert np.array_equal(s.snapshot("cons")[1], want)
            s.close()
            del s
        te, tb = float(np.median(t_res)), float(np.median(t_wb))
        rows.append({"what": "Simulation.restore vs write_block over all blocks + exchange_ghosts + fill_derived", "build": "product",
                     "fluid": "glmmhd", "blocks": nlb, "block": mb, "restore_seconds_median": te, "restore_seconds_all": t_res,
                     "write_block_seconds_median": tb, "write_block_seconds_all": t_wb, "restore_over_write_block": te / tb,
                     "restore_file_bytes": nbytes, "write_block_host_bytes": int(sum(b.nbytes for b in blocks)),
                     "repetitions": REPS, "files": "page cache", "timer": "wall clock, device synchronised"})
        print(rows[-1], flush=True)
        del blocks, want


def sentence():
    k = {r["block"]: r for r in rows if r["what"] == "apk_restart_unpack"}
    w = {r["block"]: r for r in rows if r["what"].startswith("Simulation.write_restart")}
    e = {r["block"]: r for r in rows if r["what"].startswith("Simulation.restore")}
    return ("Cost (`tools/restart_cost.py`, `profiles/restart_cost.jsonl`; one MI355X, product build, GLM-MHD, medians): "
            "`apk_restart_unpack` takes %.3f ms on 8 x 128^3 (144 B per cell, %.2f TB/s, %.2f x a device copy of the same bytes in "
            "the same run) and %.3f ms on 512 x 16^3 (%.2f x).  End to end `restore()` takes %.3f s on 8 x 128^3 against %.3f s for "
            "`write_block` over all blocks plus `exchange_ghosts` and `fill_derived` (%.2f x) and %.3f s against %.3f s on 512 x 16^3 "
            "(%.2f x), the dump's files in the page cache; `write_restart()` takes %.3f s against %.3f s for `write_snapshot(\"cons\")` "
            "on 8 x 128^3 (%.2f x) and %.3f s against %.3f s on 512 x 16^3 (%.2f x).  Not measured: hydro packs, refined meshes, more "
            "than one GPU, files read from disk."
            % (k[128]["seconds_per_launch_median"] * 1e3, k[128]["tb_per_s"], k[128]["time_over_copy"],
               k[16]["seconds_per_launch_median"] * 1e3, k[16]["time_over_copy"],
               e[128]["restore_seconds_median"], e[128]["write_block_seconds_median"], e[128]["restore_over_write_block"],
               e[16]["restore_seconds_median"], e[16]["write_block_seconds_median"], e[16]["restore_over_write_block"],
               w[128]["write_restart_seconds_median"], w[128]["write_snapshot_seconds_median"], w[128]["restart_over_snapshot"],
               w[16]["write_restart_seconds_median"], w[16]["write_snapshot_seconds_median"], w[16]["restart_over_snapshot"]))


kernel_rows()
tmp = tempfile.mkdtemp(prefix="restart_cost_")
try:
    end_to_end_rows(tmp)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "restart_cost.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
print(sentence())
