#!/usr/bin/env python
"""What the tracers' lookback histories cost per cycle on the tracer deck (inputs/turbulence_tracers.in, product build,
one GPU, one process): apk_amd/tracer_lookback off and on, for both forms of apk_amd/tracer_step, with the in-library
kernel timing (HIP events around every launch of the "tracers" and "tracer_sort" slots).  The sims run in turns, a
region each, so that clock drift falls on all of them alike.  One JSON line per variant.

  python tools/tracer_lookback_cost.py [--cycles 40] [--regions 3] [--out profiles/tracer_lookback_cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tracer_lookback_cost needs a GPU: there is no CPU fallback"
    from athenapk_amd import decks, driver
    sims = {}
    for form in ("fused", "passes"):
        for lookback in ("false", "true"):
            name = "%s, lookback %s" % (form, "on" if lookback == "true" else "off")
            sims[name] = driver.Simulation(decks.load("turbulence_tracers"),
                                           ["apk_amd/tracer_step=" + form, "apk_amd/tracer_lookback=" + lookback],
                                           strict=False).initialize()
    for s in sims.values():  # warm-up: first-touch allocations, and a few sorts
        for _ in range(5):
            s.step()
        s.kernel_timing(True)
        s.read_kernel_timing()
    acc = {name: {"step_ms": 0.0, "sort_ms": 0.0, "launches": 0, "wall_ms": 0.0} for name in sims}
    for _ in range(args.regions):
        for name, s in sims.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.cycles):
                s.step()
            torch.cuda.synchronize()
            acc[name]["wall_ms"] += (time.perf_counter() - t0) * 1e3
            kt = s.read_kernel_timing()
            acc[name]["step_ms"] += kt["tracers"][0]
            acc[name]["launches"] += kt["tracers"][1]
            acc[name]["sort_ms"] += kt["tracer_sort"][0]
    cycles = args.cycles * args.regions
    lines = []
    for name, s in sims.items():
        a = acc[name]
        lines.append(json.dumps({"variant": name, "tracers": s.tracers_count()[0], "cycles": cycles,
                                 "tracer_kernels_ms_per_cycle": a["step_ms"] / cycles,
                                 "tracer_kernel_launches_per_cycle": a["launches"] / cycles,
                                 "sort_kernels_ms_per_cycle": a["sort_ms"] / cycles,
                                 "wall_ms_per_cycle_with_timing_on": a["wall_ms"] / cycles}))
        print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
