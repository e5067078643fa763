"""Development aid (GPU box, repo root): when do the waves of ONE launch of each headline kernel of a bench workload end?

Needs the diagnostic variant build (APK_M12F_WAVE_ENDS, athenapk_amd/csrc/wave_ends.hpp):
   make -C athenapk_amd/csrc variant VAR=we VARFLAGS=-DAPK_M12F_WAVE_ENDS=1
   python tools/m12f_wave_ends.py mhd_ppm_hlld_vl2_256 [--static] [--piece-rows R] [--x3-nseg N] [--dc-kseg K]
                                  [--priority-off MASK] [--out-dir DIR --tag TAG]
Every wave of the recorded launch of the finishing march (m12f), the x3 sweep (x3) and the donor-cell predictor (dc)
records its start, a mark (m12f: the end of its whole columns), its end on the 100 MHz wall clock and the SIMD it ran
on.  Per kernel this prints (and writes to DIR/wave_ends_<kernel>_<TAG>.json) the launch's span, the share of the span
the average wave slot is occupied, the end-time distributions of the waves dispatched first and second to their SIMD
(by start time; first round of the launch) and of the last two waves every SIMD ran, and the time the SIMDs spend with
fewer than two waves at the end of the launch.  The switches only exist in the variant build: --static keeps the march's
static leftover split, --piece-rows its piece length, --x3-nseg / --dc-kseg the launch shapes, --priority-off MASK (bit
0 m12f, 1 x3) runs those kernels without wave priorities.  Also prints the kernels' HIP-event times and ms per
cycle of this variant, for sweeps on one box; --table-dir keeps the per-wave tables."""
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
ap.add_argument("--x3-nseg", type=int, default=0)
ap.add_argument("--dc-kseg", type=int, default=0)
ap.add_argument("--priority-off", type=int, default=0)
ap.add_argument("--call", type=int, default=12, help="which launch of each kernel to record")
ap.add_argument("--out-dir", default=None)
ap.add_argument("--tag", default="run")
ap.add_argument("--table-dir", default=None, help="keep the per-wave tables (wave, xcd, start, mark, end, where) here")
args = ap.parse_args()
KERNELS = {"m12f": "APK_M12F_WAVE_ENDS_OUT", "x3": "APK_X3_WAVE_ENDS_OUT", "dc": "APK_DC_WAVE_ENDS_OUT"}
tdir = args.table_dir or tempfile.mkdtemp()
os.makedirs(tdir, exist_ok=True)
dumps = {k: os.path.join(tdir, "wave_ends_%s_%s.txt" % (k, args.tag)) for k in KERNELS}
for k, env in KERNELS.items():
    if os.path.exists(dumps[k]):
        os.remove(dumps[k])
    os.environ[env] = dumps[k]
os.environ["APK_LIB_PATH"] = args.lib
os.environ["APK_M12F_WAVE_ENDS_CALL"] = str(args.call)
if args.static:
    os.environ["APK_M12F_STATIC"] = "1"
for name, v in (("APK_M12F_PIECE_ROWS", args.piece_rows), ("APK_X3_NSEG", args.x3_nseg), ("APK_DC_KSEG", args.dc_kseg),
                ("APK_WAVE_PRIORITY_OFF", args.priority_off)):
    if v:
        os.environ[name] = str(v)

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
    if all(os.path.exists(p) for p in dumps.values()):
        break
    s.step()
torch.cuda.synchronize()
s.close()

US = 0.01  # microseconds per tick of the 100 MHz wall clock


def pct(v):
    return [float(x) for x in np.percentile(v, [1, 10, 50, 90, 99])] if len(v) else []


def summarise(path):
    with open(path) as f:
        head = f.readline().strip("# \n").split()
        rows = np.loadtxt(f, dtype=np.int64, ndmin=2)
    meta = {head[i]: (int(head[i + 1]) if head[i + 1].lstrip("-").isdigit() else head[i + 1]) for i in range(0, len(head) - 1, 2)}
    rows = rows[rows[:, 4] > 0]
    xcd, start, mid, end, where = rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
    t0 = start.min()
    b, c, e = (start - t0) * US, (mid - t0) * US, (end - t0) * US
    span = float(e.max())
    # the SIMD a wave ran on: XCC, SE 15:13, SH 12, CU 11:8, SIMD 5:4 of `where` (wave slot 3:0 and pipe 7:6 left out)
    simd = where & ~np.int64(0xcf)
    first, second, last, second_last, solo, pair_gap = [], [], [], [], [], []
    for key in np.unique(simd):
        idx = np.nonzero(simd == key)[0]
        idx = idx[np.argsort(b[idx], kind="stable")]
        if len(idx) >= 2:
            first.append(e[idx[0]] - b[idx[0]])
            second.append(e[idx[1]] - b[idx[1]])
            pair_gap.append(abs(e[idx[0]] - e[idx[1]]))
            ends = np.sort(e[idx])
            last.append(ends[-1])
            second_last.append(ends[-2])
            solo.append((span - ends[-1]) + (span - ends[-2]))  # its two slots' time without a wave before the launch ends
    nsimd = len(np.unique(simd))
    out = {"launch": meta, "clock": "wall_clock64, 100 MHz", "waves": int(len(e)), "simds_seen": int(nsimd),
           "waves_per_simd_min_max": [int(np.min(np.unique(simd, return_counts=True)[1])), int(np.max(np.unique(simd, return_counts=True)[1]))],
           "span_us": span,
           "median_end_share_of_span": float(np.median(e) / span),
           # (slots: two per SIMD seen; the waves' own durations over the slots' span)
           "occupied_share_of_span": float(np.sum(e - b) / (2.0 * nsimd * span)),
           "end_us_p1_p10_p50_p90_p99": pct(e),
           "duration_us_p1_p10_p50_p90_p99": pct(e - b),
           "first_dispatched_duration_us_p1_p10_p50_p90_p99": pct(np.array(first)),
           "second_dispatched_duration_us_p1_p10_p50_p90_p99": pct(np.array(second)),
           "first_round_pair_end_gap_us_p1_p10_p50_p90_p99": pct(np.array(pair_gap)),
           "simd_last_end_us_p1_p10_p50_p90_p99": pct(np.array(last)),
           "simd_second_last_end_us_p1_p10_p50_p90_p99": pct(np.array(second_last)),
           "simd_idle_slot_us_at_end_mean": float(np.mean(solo)) if solo else 0.0,
           "per_xcd_span_us": {str(x): float(e[xcd == x].max()) for x in sorted(set(xcd.tolist()))}}
    if meta.get("kernel") == "m12f":
        out["whole_columns_duration_us_p1_p10_p50_p90_p99"] = pct(c - b)
        out["leftover_duration_us_p1_p10_p50_p90_p99"] = pct(e - c)
        out["cols_end_median_us"], out["cols_end_last_us"] = float(np.median(c)), float(c.max())
    return out


common = {"workload": args.workload, "switches": {k: v for k, v in vars(args).items() if k in ("static", "piece_rows", "x3_nseg", "dc_kseg", "priority_off")},
          "ms_per_cycle_regions": [r / cyc * 1e3 for r in reg], "kernel_ms_hip_events": timing}
for k in KERNELS:
    if not os.path.exists(dumps[k]):
        print("no table for %s (the workload does not launch it)" % k)
        continue
    out = dict(common, **summarise(dumps[k]))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "wave_ends_%s_%s.json" % (k, args.tag)), "w") as f:
            f.write(text + "\n")
