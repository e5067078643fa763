#!/usr/bin/env python
"""What tracer particles cost per cycle, on one GPU in one process (product build): the headline deck (synthetic_mhd,
GLM-MHD PPM + HLLD VL2, whose cycle stores no primitives and copies no same-rank ghost zones) and the turbulence deck,
each
  off      tracers disabled -- the baseline, the code path of a deck without <tracers>;
  empty    tracers enabled, none seeded: nothing is launched (the tracer step returns at once);
  complete ONE tracer (seed method user): the tracer step's completion of primitives and ghost zones that the cycle
           would otherwise have skipped, next to a one-lane kernel;
  fused / passes at 1/8 and at 1 tracer per cell.
Per variant: loop milliseconds per cycle (wall clock around a region of steps, device synchronised; median, minimum and
maximum of `regions` regions after a warm-up, the variants taking turns so that drift hits them alike; a region is as many
cycles as fill `--seconds`, sized per variant from the warm-up), and from the driver's kernel timing, in a region of its
own (event records cost): milliseconds per cycle of the step kernels (advect, re-own, fill or the fused kernel) and of
the counting sort, separately, with the number of steps and sorts of that region.  One JSON line per variant, appended to
--out; the achieved bytes per second divide the byte floor of kernels_tracers.hip by the STEP kernels' time.

--baseline times the `off` variant alone: run it with APK_LIB_PATH pointing at a library built from another commit, and
without, in turns on one box, to compare the cycle of a deck without <tracers> across commits.

  python tools/tracer_cost.py [--seconds 0.6] [--regions 3] [--out profiles/tracer_cost.jsonl] [--small] [--baseline]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per particle and cycle of the header of csrc/kernels_tracers.hip: particle arrays + mesh share at that density
FLOOR = {("fused", 8, 1.0): 152 + 64, ("fused", 8, 0.125): 152 + 512, ("passes", 8, 1.0): 152 + 84 + 64, ("passes", 8, 0.125): 152 + 84 + 512}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.6, help="length of a timed region")
    ap.add_argument("--baseline", action="store_true", help="the `off` variant only (see APK_LIB_PATH above)")
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="headline deck on 8 x 64^3 instead of 8 x 128^3")
    a = ap.parse_args()
    import torch
    from athenapk_amd import decks, driver
    assert torch.cuda.is_available(), "tracer_cost needs a GPU: there is no CPU fallback"
    small = ["parthenon/mesh/nx1=128", "parthenon/mesh/nx2=128", "parthenon/mesh/nx3=128", "parthenon/meshblock/nx1=64",
             "parthenon/meshblock/nx2=64", "parthenon/meshblock/nx3=64"] if a.small else []
    on = ["tracers/enabled=true"]

    def seeded(per_cell, form):
        return on + ["tracers/initial_seed_method=random_per_block", "tracers/initial_num_tracers_per_cell=%g" % per_cell,
                     "apk_amd/tracer_step=" + form]

    variants = [("off", [], False), ("empty", on, False), ("complete", on + ["tracers/initial_seed_method=user"], True)]
    for per_cell in (0.125, 1.0):
        for form in ("fused", "passes"):
            variants.append(("%s_%g" % (form, per_cell), seeded(per_cell, form), False))
    if a.baseline:
        variants = variants[:1]
    lib_label = os.path.basename(os.environ.get("APK_LIB_PATH", "")) or "this commit"
    rows = []
    for deck, base in (("synthetic_mhd", small), ("turbulence", [])):
        sims = {}
        for name, ov, _ in variants:
            sims[name] = driver.Simulation(decks.load(deck), base + ov, strict=False).initialize()
            if name == "complete":
                i = sims[name].info
                sims[name].seed_tracers(*[[0.5 * (i.xmin[d] + i.xmax[d])] for d in range(3)])

        cycles = {}

        def region(name, timing=False, n=None):
            s = sims[name]
            n = n or cycles[name]
            if timing:
                s.kernel_timing(True)
            stats0 = s.tracers_stats() if timing else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                s.step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / n
            if not timing:
                return ms, None
            kt = s.read_kernel_timing()
            s.kernel_timing(False)
            stats1 = s.tracers_stats()
            return ms, {"step_kernels_ms": kt["tracers"][0] / n, "sort_kernels_ms": kt["tracer_sort"][0] / n,
                        "steps": stats1[0] - stats0[0], "sorts": stats1[1] - stats0[1]}

        for name in sims:  # warm-up (first-touch allocations, code objects), and the region's length
            region(name, n=5)
            cycles[name] = max(20, int(a.seconds / (region(name, n=10)[0] * 1e-3)))
        loop = {name: [] for name in sims}
        for _ in range(a.regions):
            for name in sims:
                loop[name].append(region(name)[0])
        for name, ov, _ in variants:
            s = sims[name]
            kt = region(name, timing=True)[1] if ov else None
            i = s.info
            n = s.tracers_count()[0] if ov else 0
            row = {"deck": deck, "variant": name, "lib": lib_label, "blocks": i.nblocks_total, "block": list(i.mb),
                   "cycles_per_region": cycles[name],
                   "loop_ms_median": float(np.median(loop[name])), "loop_ms_min": min(loop[name]), "loop_ms_max": max(loop[name]),
                   "tracers": n, "prim_stale_after_cycle": bool(s.prim_is_stale)}
            if kt:
                row.update(kt)
            parts = name.split("_")
            key = (parts[0], 8, float(parts[1])) if len(parts) == 2 and parts[0] in ("fused", "passes") else None
            if key in FLOOR and kt and kt["step_kernels_ms"]:
                row["floor_bytes_per_tracer"] = FLOOR[key]
                row["achieved_bytes_per_s"] = FLOOR[key] * n / (kt["step_kernels_ms"] * 1e-3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        for s in sims.values():
            s.close()
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
