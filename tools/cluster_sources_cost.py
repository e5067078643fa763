"""Times apk_snia_feedback_src and apk_cluster_split_src (product build, GLM-MHD packs) on one 64^3 block and on the
8 x 128^3 pack with device events: warm-up, then 100 launches per window, 5 windows, medians; writes the rows to the file
given as the first argument (default out/cluster_sources_cost.jsonl; profiles/cluster_sources_cost.jsonl is such a run).
Yardsticks timed in the same run: for SNIa feedback a device copy of its algorithmic bytes (240 B per cell: cons read and
written, the stored velocity read, prim written); for the split sources, with stellar radius and clip radius of four
cells at the centre of the mesh, apk_agn_triggering_reduce (Bondi sums) with an accretion radius of four cells, and a
device copy of the bytes of the boxes' cells (cons and prim read and written, 288 B)."""
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
INF = float("inf")
ctx = hydro.Context(strict=False)
lib = ctx.lib
dev = torch.device("cuda")
eos = L.make_eos(5.0 / 3.0)


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


def copy_times(nbytes):
    words = max(nbytes // 16, 1)  # a copy reads and writes: half the bytes each way
    src = torch.empty(words, dtype=torch.float64, device=dev).normal_()
    dst = torch.empty_like(src)
    return window_times(lambda: dst.copy_(src))


def index_range(x, radius, lo_clip, hi_clip):
    """the active list's range of one direction, clipped to [lo_clip, hi_clip)"""
    inside = np.nonzero(np.abs(x) < radius)[0]
    if len(inside) == 0:
        return 0, 0
    return max(int(inside[0]) - 1, lo_clip), min(int(inside[-1]) + 2, hi_clip)


def box_list(locs, n, ng, dx, radius, interior):
    N = n + 2 * ng
    boxes, cells, max_cells = [], 0, 0
    for b, loc in enumerate(locs):
        lim = (ng, ng + n) if interior else (0, N)
        r = [index_range(-0.1 + ((loc[d] * n - ng + np.arange(N)) + 0.5) * dx, radius, *lim) for d in range(3)]
        cells_b = int(np.prod([max(hi - lo, 0) for lo, hi in r]))
        if cells_b == 0:
            continue
        boxes.append(L.TrigBox(b, (C.c_int * 3)(*[lo for lo, _ in r]), (C.c_int * 3)(*[hi for _, hi in r])))
        cells += cells_b
        max_cells = max(max_cells, cells_b)
    arr = (L.TrigBox * len(boxes))(*boxes)
    return torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev), len(boxes), cells, max_cells


rows, checks = [], []
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
    cells = nb * n ** 3
    common = {"build": "product", "fluid": "glmmhd", "blocks": nb, "block": n, "cells": cells, "launches_per_window": LAUNCHES,
              "windows": WINDOWS, "timer": "device events"}

    # SNIa feedback: rates small enough that a thousand launches leave the state where it was
    snia = L.SniaCfg(1e-9, 1e-9, 7.5e-4 * 0.004 / (2 * np.pi), 0.004, 0.0)

    def snia_launch():
        rc = lib.apk_snia_feedback_src(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), C.byref(snia), t.data_ptr(), 1e-3, None)
        assert rc == 0, rc

    times, ctimes = window_times(snia_launch), copy_times(cells * 240)
    tm, cm = float(np.median(times)), float(np.median(ctimes))
    rows.append(dict(common, kernel="apk_snia_feedback_src", seconds_per_launch_median=tm, seconds_per_launch_min=min(times),
                     seconds_per_launch_max=max(times), bytes_per_cell=240, copy_seconds=cm, time_over_copy=tm / cm,
                     bytes_per_second=cells * 240 / tm))
    print(rows[-1], flush=True)

    # the split sources over their own (interior) list, next to the triggering reduction over its list
    d_split, n_split, split_cells, split_max = box_list(locs, n, ng, dx, radius, True)
    d_trig, n_trig, trig_cells, trig_max = box_list(locs, n, ng, dx, radius, False)
    sums8 = torch.zeros((nb, 8), dtype=torch.float64, device=dev)
    sums4 = torch.zeros((nb, 4), dtype=torch.float64, device=dev)
    # thresholds every launch meets in part: after the first launch a converted cell sits at the threshold and a clipped
    # one at its limit, so a thousand launches leave the state where the first one put it
    stellar = L.StellarCfg(radius, dx, 1.3, 1e30, 1.0, 1.0, 1e-3)
    clips = L.ClipsCfg(radius, 0.6, 0.12, 0.25, 6.0)
    bondi = L.AgnTriggeringCfg(L.TRIGGERING_MODE["BOOSTED_BONDI"], 1, radius, 0.0, 0.0, 1.0)

    def split_launch():
        rc = lib.apk_cluster_split_src(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), C.byref(stellar), C.byref(clips), d_split.data_ptr(),
                                       n_split, split_max, t.data_ptr(), sums8.data_ptr(), None)
        assert rc == 0, rc

    def reduce_launch():
        rc = lib.apk_agn_triggering_reduce(ctx.h, md.h, L.FLUID["glmmhd"], C.byref(eos), C.byref(bondi), d_trig.data_ptr(), n_trig,
                                           trig_max, t.data_ptr(), 1e-3, sums4.data_ptr(), None)
        assert rc == 0, rc

    times, rtimes, ctimes = window_times(split_launch), window_times(reduce_launch), copy_times(split_cells * 288)
    tm, rm, cm = float(np.median(times)), float(np.median(rtimes)), float(np.median(ctimes))
    rows.append(dict(common, kernel="apk_cluster_split_src[stellar+clips]", radius_cells=RADIUS_CELLS, active_blocks=n_split,
                     box_cells=split_cells, seconds_per_launch_median=tm, seconds_per_launch_min=min(times),
                     seconds_per_launch_max=max(times), bytes_per_box_cell_floor=288, copy_box_bytes_seconds=cm, time_over_copy=tm / cm,
                     triggering_reduce_seconds=rm, triggering_reduce_box_cells=trig_cells, time_over_triggering_reduce=tm / rm))
    print(rows[-1], flush=True)
    checks.append((ctx.poll_flags(), bool(torch.isfinite(sums8).all()) and bool(torch.isfinite(md.cons).all())))
    del md, cons, prim
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "cluster_sources_cost.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
# no floor fired and the state stayed finite: the launches timed were the kernels' ordinary work.  The one flag expected is
# stellar feedback's: a cell the first launch left exactly at the threshold converts again with a density of zero, and adding
# zero energy is what the reference's sanity check refuses
assert all((flags & ~L.APK_FLAG_STELLAR_ENERGY) == 0 and finite for flags, finite in checks), checks
