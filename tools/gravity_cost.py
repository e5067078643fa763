"""Times apk_gravity_src (product build) on one 64^3 block and on the 8 x 128^3 pack with device events: warm-up, then
200 launches per window, 5 windows; writes the rows to the file given as the first argument (default
out/gravity_cost.jsonl; profiles/gravity_cost.jsonl is such a run).  A device copy of the same bytes is timed alongside as
the stream yardstick of the box."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_reference as R  # noqa: E402
from athenapk_amd import hydro  # noqa: E402

ctx = hydro.Context(strict=False)
g = R.deck_model()[0]
grav = hydro.make_cluster_gravity(True, "HERNQUIST", True, g.r_nfw_s, g.g_const_nfw, g.r_bcg_s, g.g_const_bcg,
                                  g.g_const_smbh, g.smoothing_r)
rows = []
for nb, n in ((1, 64), (8, 128)):
    ng = 2
    N = n + 2 * ng
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    cons = torch.rand((nb, 5, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
    prim = torch.rand((nb, 5, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
    dx = 0.2 / (2 * n)
    md = hydro.MeshData(ctx, (n, n, n), ng, 5, dx=(dx, dx, dx), nblocks=nb, cons=cons, prim=prim, with_flux=False)
    corners = np.array([[-0.1 + (b % 2) * n * dx, -0.1 + ((b // 2) % 2) * n * dx, -0.1 + (b // 4) * n * dx] for b in range(nb)] +
                       [[-0.1, -0.1, -0.1]])
    t = torch.from_numpy(corners).to(dev)
    lib = ctx.lib

    def launch():
        rc = lib.apk_gravity_src(ctx.h, md.h, C.byref(grav), t.data_ptr(), 1e-9, None)
        assert rc == 0, rc

    cells = nb * n ** 3
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    times = []
    for w in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 200 * 1e-3)
    # the stream yardstick: a copy of 48 B per cell read + 48 B written
    src = torch.empty(cells * 6, dtype=torch.float64, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(20):
        dst.copy_(src)
    torch.cuda.synchronize()
    ctimes = []
    for w in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ctimes.append(e0.elapsed_time(e1) / 200 * 1e-3)
    tm, cm = float(np.median(times)), float(np.median(ctimes))
    rows.append({"kernel": "apk_gravity_src", "build": "product", "blocks": nb, "block": n, "cells": cells,
                 "seconds_per_launch_median": tm, "seconds_per_launch_min": min(times), "seconds_per_launch_max": max(times),
                 "ns_per_cell": tm / cells * 1e9, "bytes_per_cell_floor": 96, "tb_per_s_at_floor": 96 * cells / tm * 1e-12,
                 "copy_same_bytes_seconds": cm, "copy_tb_per_s": 96 * cells / cm * 1e-12,
                 "launches_per_window": 200, "windows": 5, "timer": "device events"})
    print(rows[-1])
    del md, cons, prim, src, dst
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "gravity_cost.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
