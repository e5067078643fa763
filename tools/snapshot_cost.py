"""Cost of field snapshots on one MI355X (product build, GLM-MHD), one process; writes JSON rows to the file given as the
first argument (default out/snapshot_cost.jsonl; profiles/snapshot_cost.jsonl is such a run).

(a) apk_output_pack alone, device events (warm-up, then 50 launches per window, 5 windows, medians), for `prim` in float,
    `cons` in double and `cons, prim, temperature, mach_sonic, plasma_beta` in double, on the 8 x 128^3 pack and on a
    512 x 16^3 pack -- each next to a device copy of its algorithmic bytes (nvar * 8 read + ncomp * itemsize written per
    interior cell) timed in the same run: the kernel's time over that copy says how far from the stream rate it is.
(b) Simulation.snapshot("prim") end to end (wall clock around a synchronised call) against the path the accessors offer
    for the same data -- read_block(lb, "prim") over all blocks plus interior slicing in numpy -- on the same state: after
    every cycle the snapshot is taken first, then the accessor path (whose first call completes ghost zones and
    primitives).  For the 8 x 128^3 mesh also with 64 / 256 / 1024 MB of staging (apk_amd/snapshot_staging_mb)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from athenapk_amd import decks, driver, hydro  # noqa: E402
from athenapk_amd import lib as L  # noqa: E402

LAUNCHES, WINDOWS = 50, 5
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
    eos = L.make_eos(5.0 / 3.0)
    CONS, PRIM = list(range(9)), list(range(L.OUT_PRIM, L.OUT_PRIM + 9))
    lists = (("prim", PRIM, True), ("cons", CONS, False),
             ("cons,prim,temperature,mach_sonic,plasma_beta",
              CONS + PRIM + [L.OUT_DERIVED[n] for n in ("temperature", "mach_sonic", "plasma_beta")], False))
    for nb, n in ((8, 128), (512, 16)):
        ng = 3
        N = n + 2 * ng
        gen = torch.Generator(device=dev).manual_seed(1)
        cons = torch.rand((nb, 9, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
        cons[:, 4] += 5.0
        cons[:, 1:4] *= 0.1
        cons[:, 5:9] *= 0.1
        md = hydro.MeshData(ctx, (n, n, n), ng, 9, dx=(0.01, 0.01, 0.01), nblocks=nb, cons=cons, with_flux=False)
        cells = nb * n ** 3
        for name, codes, single in lists:
            item = 4 if single else 8
            out = torch.empty(cells * len(codes) * item, dtype=torch.uint8, device=dev)
            desc = L.make_output_desc(codes, single, 5.0 / 3.0, 1.0)

            def launch():
                rc = lib.apk_output_pack(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), C.byref(desc), 0, nb, out.data_ptr(), None)
                assert rc == 0, rc

            times = window_times(launch)
            nbytes = 9 * 8 + len(codes) * item
            words = cells * nbytes // 16  # a copy reads and writes: half the bytes each way
            src = torch.empty(words, dtype=torch.float64, device=dev).normal_()
            dst = torch.empty_like(src)
            ctimes = window_times(lambda: dst.copy_(src))
            tm, cm = float(np.median(times)), float(np.median(ctimes))
            rows.append({"what": "apk_output_pack", "build": "product", "fluid": "glmmhd", "variables": name,
                         "dtype": "<f4" if single else "<f8", "ncomp": len(codes), "blocks": nb, "block": n, "cells": cells,
                         "seconds_per_launch_median": tm, "seconds_per_launch_min": min(times), "seconds_per_launch_max": max(times),
                         "ns_per_cell": tm / cells * 1e9, "bytes_per_cell": nbytes, "tb_per_s": nbytes * cells / tm * 1e-12,
                         "copy_same_bytes_seconds": cm, "copy_tb_per_s": nbytes * cells / cm * 1e-12, "time_over_copy": tm / cm,
                         "launches_per_window": LAUNCHES, "windows": WINDOWS, "timer": "device events"})
            print(rows[-1], flush=True)
            del src, dst, out
        assert ctx.poll_flags() == 0
        del md, cons
    ctx.close()


def _mesh(nx, mb):
    return ["parthenon/mesh/nx%d=%d" % (d + 1, nx) for d in range(3)] + ["parthenon/meshblock/nx%d=%d" % (d + 1, mb) for d in range(3)]


def end_to_end_rows():
    for nx, mb, staging in ((256, 128, 256), (256, 128, 64), (256, 128, 1024), (128, 16, 256)):
        s = driver.Simulation(decks.load("synthetic_mhd"), _mesh(nx, mb) + ["apk_amd/snapshot_staging_mb=%d" % staging],
                              strict=False).initialize()
        i = s.info
        sl = (slice(None),) + (slice(i.ng, i.ng + mb),) * 3
        s.step()
        s.snapshot("prim")  # (first use allocates the staging buffers)
        t_snap, t_acc = [], []
        for _ in range(3):
            s.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            names, a = s.snapshot("prim")
            t1 = time.perf_counter()
            b = np.stack([s.read_block(lb, "prim")[sl] for lb in range(i.nblocks_local)])
            t2 = time.perf_counter()
            t_snap.append(t1 - t0)
            t_acc.append(t2 - t1)
            assert np.allclose(a, b, rtol=1e-12, atol=0.0)
        ts, ta = float(np.median(t_snap)), float(np.median(t_acc))
        rows.append({"what": "Simulation.snapshot('prim') vs read_block(lb, 'prim') + numpy slicing", "build": "product",
                     "fluid": "glmmhd", "blocks": i.nblocks_local, "block": mb, "snapshot_staging_mb": staging,
                     "snapshot_seconds_median": ts, "snapshot_seconds_all": t_snap, "accessors_seconds_median": ta,
                     "accessors_seconds_all": t_acc, "snapshot_over_accessors": ts / ta,
                     "snapshot_host_bytes": int(a.nbytes), "accessors_host_bytes": int(i.nblocks_local * 9 * (mb + 2 * i.ng) ** 3 * 8),
                     "repetitions": 3, "timer": "wall clock, device synchronised"})
        print(rows[-1], flush=True)
        s.close()
        del s


kernel_rows()
end_to_end_rows()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "snapshot_cost.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
