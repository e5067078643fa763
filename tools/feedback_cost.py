"""Times apk_agn_feedback_src, apk_magnetic_tower_src and apk_magnetic_tower_power_contribs (product build, GLM-MHD packs)
on one 64^3 block and on the 8 x 128^3 pack with device events: warm-up, then 100 launches per window, 5 windows; writes the
rows to the file given as the first argument (default out/feedback_cost.jsonl; profiles/feedback_cost.jsonl is such a
run).  In the same run a device copy of each kernel's algorithmic bytes is timed as the stream yardstick of the box: the
kernel's time as a fraction of that copy says how far from memory-bound it is."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from athenapk_amd import hydro  # noqa: E402
from athenapk_amd import lib as L  # noqa: E402

LAUNCHES, WINDOWS = 100, 5
ctx = hydro.Context(strict=False)
lib = ctx.lib
dev = torch.device("cuda")
eos = L.make_eos(5.0 / 3.0)
jet = L.JetCoords(np.cos(0.2), np.sin(0.2), np.cos(1.0), np.sin(1.0))
# the feedback deck's geometry scaled to the box, thermal and kinetic channels both acting, no ceilings; amounts small
# enough that a thousand launches leave the state where it was
agn = L.AgnFeedbackCfg(1e-12, 1e-12, 0.1, 1e-12, 1e-11, 1e-10, 0.05, 0.05, 0.01, float("inf"), float("inf"))
tower = L.MagneticTowerCfg(L.TOWER_POTENTIAL["li"], 20.0, 0.01, 0.0, 0.0, 0.005)


def window_times(launch):
    for _ in range(10):
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


rows = []
for nb, n in ((1, 64), (8, 128)):
    ng = 2
    N = n + 2 * ng
    gen = torch.Generator(device=dev).manual_seed(1)
    cons = torch.rand((nb, 9, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
    cons[:, 4] += 5.0
    cons[:, 1:4] *= 0.1
    cons[:, 5:9] *= 0.1
    prim = torch.rand((nb, 9, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
    dx = 0.2 / (2 * n)
    md = hydro.MeshData(ctx, (n, n, n), ng, 9, dx=(dx, dx, dx), nblocks=nb, cons=cons, prim=prim, with_flux=False)
    corners = np.array([[-0.1 + (b % 2) * n * dx, -0.1 + ((b // 2) % 2) * n * dx, -0.1 + (b // 4) * n * dx] for b in range(nb)] +
                       [[-0.1, -0.1, -0.1]])
    t = torch.from_numpy(corners).to(dev)
    contribs = torch.zeros((nb, 2), dtype=torch.float64, device=dev)
    cells = nb * n ** 3

    def agn_launch():
        rc = lib.apk_agn_feedback_src(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), C.byref(agn), C.byref(jet), t.data_ptr(), None)
        assert rc == 0, rc

    def tower_launch():
        rc = lib.apk_magnetic_tower_src(ctx.h, md.h, C.byref(tower), C.byref(jet), t.data_ptr(), 1e-9, 1e-12, None)
        assert rc == 0, rc

    def contribs_launch():
        rc = lib.apk_magnetic_tower_power_contribs(ctx.h, md.h, C.byref(tower), C.byref(jet), t.data_ptr(), contribs.data_ptr(), None)
        assert rc == 0, rc

    # bytes per cell the launch must move (the floor): cons and prim of 9 variables read and written; prim B read and
    # cons B, E, rho read and written; prim B read
    for name, launch, nbytes in (("apk_agn_feedback_src", agn_launch, 288), ("apk_magnetic_tower_src", tower_launch, 104),
                                 ("apk_magnetic_tower_power_contribs", contribs_launch, 24)):
        times = window_times(launch)
        words = cells * nbytes // 16  # a copy reads and writes: half the bytes each way
        src = torch.empty(words, dtype=torch.float64, device=dev).normal_()
        dst = torch.empty_like(src)
        ctimes = window_times(lambda: dst.copy_(src))
        tm, cm = float(np.median(times)), float(np.median(ctimes))
        rows.append({"kernel": name, "build": "product", "fluid": "glmmhd", "blocks": nb, "block": n, "cells": cells,
                     "seconds_per_launch_median": tm, "seconds_per_launch_min": min(times), "seconds_per_launch_max": max(times),
                     "ns_per_cell": tm / cells * 1e9, "bytes_per_cell_floor": nbytes, "tb_per_s_at_floor": nbytes * cells / tm * 1e-12,
                     "copy_same_bytes_seconds": cm, "copy_tb_per_s": nbytes * cells / cm * 1e-12, "time_over_copy": tm / cm,
                     "launches_per_window": LAUNCHES, "windows": WINDOWS, "timer": "device events"})
        print(rows[-1], flush=True)
        del src, dst
    flags = ctx.poll_flags()
    assert flags == 0, flags
    del md, cons, prim
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "feedback_cost.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
