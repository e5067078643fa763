"""Development aid (GPU box, repo root): when do the waves of ONE finishing-march launch of a bench workload end?

Needs the diagnostic variant build of fused2_kernel.hpp (APK_M12F_WAVE_ENDS):
   make -C athenapk_amd/csrc variant VAR=we VARFLAGS=-DAPK_M12F_WAVE_ENDS=1
   python tools/m12f_wave_ends.py mhd_ppm_hlld_vl2_256 [--static] [--piece-rows R] [--out summary.json]
Every wave of the launch records its start, the end of its whole columns and its end on the 100 MHz wall clock; this
prints (and writes) the kernel's span, the time to the median and to the last wave's end, the share of the span the
average wave slot is occupied, and the same per XCD.  --static keeps the static leftover split, --piece-rows sets the
dynamic phase's piece length (both only exist in the variant build), --table keeps the per-wave table.  Also prints the
march's HIP-event time and ms per cycle of this variant, for sweeps on one box."""
import argparse
import json
import os
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("workload")
ap.add_argument("--lib", default=os.path.join("athenapk_amd", "libapk_amd_we.so"))
ap.add_argument("--static", action="store_true")
ap.add_argument("--piece-rows", type=int, default=0)
ap.add_argument("--call", type=int, default=12, help="which launch of the march to record")
ap.add_argument("--out", default=None)
ap.add_argument("--table", default=None, help="keep the per-wave table (wave, xcd, start, end of whole columns, end) here")
args = ap.parse_args()
dump = args.table or os.path.join(tempfile.mkdtemp(), "wave_ends.txt")
if os.path.exists(dump):
    os.remove(dump)
os.environ["APK_LIB_PATH"] = args.lib
os.environ["APK_M12F_WAVE_ENDS_OUT"] = dump
os.environ["APK_M12F_WAVE_ENDS_CALL"] = str(args.call)
if args.static:
    os.environ["APK_M12F_STATIC"] = "1"
if args.piece_rows:
    os.environ["APK_M12F_PIECE_ROWS"] = str(args.piece_rows)

import numpy as np  # noqa: E402
import torch  # noqa: E402
sys.path.insert(0, ".")
from athenapk_amd import decks, driver  # noqa: E402
import bench  # noqa: E402

deck, fluid, integrator, recon, riemann, brick, mb, desc = bench.WORKLOADS[args.workload]
ov = ["parthenon/mesh/nx%d=%d" % (d + 1, brick) for d in range(3)] + ["parthenon/meshblock/nx%d=%d" % (d + 1, mb) for d in range(3)]
ov += ["parthenon/time/integrator=%s" % integrator, "hydro/reconstruction=%s" % recon, "hydro/riemann=%s" % riemann]
s = driver.Simulation(decks.load(deck), ov, strict=False).initialize()
for _ in range(3):
    s.step()
cyc, reg, med = bench.timed_regions(s.step, torch.cuda.synchronize, probe_cycles=3)
s.kernel_timing(True)
s.read_kernel_timing()
for _ in range(8):
    s.step()
torch.cuda.synchronize()
timing = {k: v[0] / v[1] for k, v in s.read_kernel_timing().items() if v[1]}
for _ in range(args.call):  # (in case the regions above were shorter than --call launches)
    if os.path.exists(dump):
        break
    s.step()
torch.cuda.synchronize()
s.close()

with open(dump) as f:
    head = f.readline().strip("# \n").split()
    rows = np.loadtxt(f, dtype=np.int64, ndmin=2)
meta = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
rows = rows[rows[:, 4] > 0]
xcd, start, cols, end = rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4]
t0 = start.min()
US = 0.01  # microseconds per tick of the 100 MHz wall clock


def stats(m):
    e, c, b = (end[m] - t0) * US, (cols[m] - t0) * US, (start[m] - t0) * US
    span = float(e.max())
    return {"waves": int(m.sum()), "first_start_us": float(b.min()), "last_start_us": float(b.max()),
            "cols_end_median_us": float(np.median(c)), "cols_end_last_us": float(c.max()),
            "end_first_us": float(e.min()), "end_p10_us": float(np.percentile(e, 10)), "end_median_us": float(np.median(e)),
            "end_p90_us": float(np.percentile(e, 90)), "end_last_us": span,
            "whole_columns_duration_us_p1_p10_p50_p90_p99": [float(v) for v in np.percentile(c - b, [1, 10, 50, 90, 99])],
            "leftover_duration_us_p1_p10_p50_p90_p99": [float(v) for v in np.percentile(e - c, [1, 10, 50, 90, 99])],
            "occupied_share_of_own_span": float(np.mean(e - b) / (span - float(b.min())))}


allw = np.ones(len(end), dtype=bool)
span_us = float((end.max() - t0) * US)
out = {"workload": args.workload, "launch": meta, "clock": "wall_clock64, 100 MHz",
       "span_us": span_us, "median_end_share_of_span": float(np.median(end - t0) * US / span_us),
       "occupied_share_of_span": float(np.mean(end - start) * US / span_us),
       "all": stats(allw), "per_xcd": {str(x): stats(xcd == x) for x in sorted(set(xcd.tolist()))},
       "ms_per_cycle_regions": [r / cyc * 1e3 for r in reg], "kernel_ms_hip_events": timing}
text = json.dumps(out, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
