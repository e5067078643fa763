"""Times apk_agn_triggering_reduce (Bondi sums; cold mass with its removal) and apk_agn_triggering_remove_bondi (product
build, GLM-MHD packs) on one 64^3 block and on the 8 x 128^3 pack, with an accretion radius of four cells at the centre of
the mesh, with device events: warm-up, then 100 launches per window, 5 windows; writes the rows to the file given as the
first argument (default out/triggering_cost.jsonl; profiles/triggering_cost.jsonl is such a run).  In the same run two
yardsticks are timed: apk_magnetic_tower_power_contribs on the same pack, the price of a walk over every cell (24 B per
cell), and a device copy of the bytes the kernel moves for the cells of its boxes."""
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
RADIUS_CELLS = 4
ctx = hydro.Context(strict=False)
lib = ctx.lib
dev = torch.device("cuda")
eos = L.make_eos(5.0 / 3.0)
jet = L.JetCoords(np.cos(0.2), np.sin(0.2), np.cos(1.0), np.sin(1.0))
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


def index_range(x, radius):
    """the active list's range of one direction (csrc/host/feedback_model.cpp: triggering_index_range)"""
    inside = np.nonzero(np.abs(x) < radius)[0]
    if len(inside) == 0:
        return 0, 0
    return max(int(inside[0]) - 1, 0), min(int(inside[-1]) + 2, len(x))


rows = []
for nb, n in ((1, 64), (8, 128)):
    ng = 2
    N = n + 2 * ng
    side = 1 if nb == 1 else 2
    gen = torch.Generator(device=dev).manual_seed(1)
    cons = torch.rand((nb, 9, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
    cons[:, 4] += 5.0
    cons[:, 1:4] *= 0.1
    cons[:, 5:9] *= 0.1
    prim = torch.rand((nb, 9, N, N, N), dtype=torch.float64, device=dev, generator=gen) + 0.5
    dx = 0.2 / (side * n)
    md = hydro.MeshData(ctx, (n, n, n), ng, 9, dx=(dx, dx, dx), nblocks=nb, cons=cons, prim=prim, with_flux=False)
    locs = [(b % side, (b // side) % side, b // (side * side)) for b in range(nb)]
    corners = np.array([[-0.1 + loc[d] * n * dx for d in range(3)] for loc in locs] + [[-0.1, -0.1, -0.1]])
    t = torch.from_numpy(corners).to(dev)
    radius = RADIUS_CELLS * dx
    boxes, box_cells, max_cells = [], 0, 0
    for b, loc in enumerate(locs):
        r = [index_range(-0.1 + ((loc[d] * n - ng + np.arange(N)) + 0.5) * dx, radius) for d in range(3)]
        cells_b = int(np.prod([hi - lo for lo, hi in r]))
        if cells_b == 0:
            continue
        boxes.append(L.TrigBox(b, (C.c_int * 3)(*[lo for lo, _ in r]), (C.c_int * 3)(*[hi for _, hi in r])))
        box_cells += cells_b
        max_cells = max(max_cells, cells_b)
    arr = (L.TrigBox * len(boxes))(*boxes)
    d_boxes = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev)
    sums = torch.zeros((nb, 4), dtype=torch.float64, device=dev)
    contribs = torch.zeros((nb, 2), dtype=torch.float64, device=dev)
    cells = nb * n ** 3
    # amounts small enough that a thousand launches leave the state where it was
    bondi = L.AgnTriggeringCfg(L.TRIGGERING_MODE["BOOSTED_BONDI"], 1, radius, 0.0, 0.0, 1.0)
    cold = L.AgnTriggeringCfg(L.TRIGGERING_MODE["COLD_GAS"], 1, radius, 1e30, 1e12, 1.0)

    def reduce_launch(cfg):
        def launch():
            rc = lib.apk_agn_triggering_reduce(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), C.byref(cfg), d_boxes.data_ptr(), len(boxes),
                                               max_cells, t.data_ptr(), 1e-3, sums.data_ptr(), None)
            assert rc == 0, rc
        return launch

    def remove_launch():
        rc = lib.apk_agn_triggering_remove_bondi(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), radius, d_boxes.data_ptr(), len(boxes),
                                                 max_cells, t.data_ptr(), 1.0, 1e-9, 1e-3, None)
        assert rc == 0, rc

    def contribs_launch():
        rc = lib.apk_magnetic_tower_power_contribs(ctx.h, md.h, C.byref(tower), C.byref(jet), t.data_ptr(), contribs.data_ptr(), None)
        assert rc == 0, rc

    walk = float(np.median(window_times(contribs_launch)))
    # bytes per box cell (the floor, were every cell of the boxes inside the sphere): five primitives read; cons and prim
    # of 9 variables read and written
    for name, launch, nbytes in (("apk_agn_triggering_reduce[BOOSTED_BONDI]", reduce_launch(bondi), 40),
                                 ("apk_agn_triggering_reduce[COLD_GAS+removal]", reduce_launch(cold), 288),
                                 ("apk_agn_triggering_remove_bondi", remove_launch, 288)):
        times = window_times(launch)
        words = max(box_cells * nbytes // 16, 1)  # a copy reads and writes: half the bytes each way
        src = torch.empty(words, dtype=torch.float64, device=dev).normal_()
        dst = torch.empty_like(src)
        ctimes = window_times(lambda: dst.copy_(src))
        tm, cm = float(np.median(times)), float(np.median(ctimes))
        rows.append({"kernel": name, "build": "product", "fluid": "glmmhd", "blocks": nb, "block": n, "cells": cells,
                     "accretion_radius_cells": RADIUS_CELLS, "active_blocks": len(boxes), "box_cells": box_cells,
                     "seconds_per_launch_median": tm, "seconds_per_launch_min": min(times), "seconds_per_launch_max": max(times),
                     "bytes_per_box_cell_floor": nbytes, "copy_box_bytes_seconds": cm, "time_over_copy": tm / cm,
                     "whole_mesh_walk_kernel": "apk_magnetic_tower_power_contribs", "whole_mesh_walk_seconds": walk,
                     "time_over_whole_mesh_walk": tm / walk,
                     "launches_per_window": LAUNCHES, "windows": WINDOWS, "timer": "device events"})
        print(rows[-1], flush=True)
        del src, dst
    flags = ctx.poll_flags()
    assert flags == 0, flags
    assert bool(torch.isfinite(sums).all()) and float(sums[:, 0].sum()) > 0.0
    del md, cons, prim
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "triggering_cost.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
