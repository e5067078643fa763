"""bench.py itself, launched the way the driver launches it for N > 1 (round-2 verdict, "Next round" 2: nothing had
ever executed `python -m torch.distributed.run ... bench.py --gpus N`).  The test box has one GPU, so the ranks
share cuda:0 and the messages go through gloo (APK_SHARE_GPU=1 APK_DIST_BACKEND=gloo, the switches bench.py documents
for exactly this); everything else -- rank grid, brick partition, overlapped exchanges, barrier + max-over-ranks
timing, the JSON contract -- is the path an 8-GPU node runs.  N = 1 is checked for the second, copy-inclusive figure.
A plain run prints the headline alone; what --full adds (roofline, N = 1 figures) is checked on runs with --full."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _launch(world, extra, timeout=900):
    env = dict(os.environ, APK_SHARE_GPU="1", APK_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", "--gpus", str(world)] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "bench.py failed on %d ranks:\n%s\n%s" % (world, r.stdout[-3000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 must print exactly ONE JSON line, got %d:\n%s" % (len(lines), r.stdout[-2000:])
    return json.loads(lines[0])


# what only a --full run measures: the kernels' event region and the roofline, and the N = 1 figures
FULL_ONLY = ("kernel_event_region_ms", "roofline", "sustained_500_cycles", "weak_scaling_base_with_ghost_copies",
             "rehearsal_8gpu_rank", "other_workloads", "cpu_baseline")


def _check_contract(d, world, steps, warmup, full):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config") + (("kernel_event_region_ms", "roofline") if full else ()):
        assert key in d, key
    assert d["n_gpus"] == world and d["steps"] == steps and d["warmup"] == warmup
    assert d["unit"] == "cell-updates/s" and d["scaling"] == "weak" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["value"] == d["value"] and d["ms_per_step"] > 0
    if not full:
        assert not [k for k in FULL_ONLY if k in d], sorted(d)
        return
    r = d["roofline"]
    # (`bound` names what binds the stage kernels -- the fp64 vector issue rate for the GLM-MHD marches -- while achieved /
    # peak / frac stay priced against HBM bandwidth, as north_star asks: `priced_against`)
    assert r["bound"] in ("hbm", "fp64_valu_issue") and r["priced_against"] == "hbm" and r["unit"] == "GB/s"
    assert 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12


def test_bench_on_two_ranks_through_the_launcher():
    """128^3 per rank in 64^3 meshblocks (2 x 1 x 1 rank grid): the headline workload's scheme and code path, reduced"""
    d = _launch(2, ["--steps", "2", "--warmup", "1", "--brick", "128", "--meshblock", "64", "--no-cpu-baseline", "--full"])
    _check_contract(d, 2, 2, 1, full=True)
    c = d["config"]
    assert c["mesh"] == [256, 128, 128] and c["blocks_per_gpu"] == 8 and c["parallelism"].endswith("2x1x1 GPU grid")
    assert "gloo" in c["comm_backend"]
    assert c["overlapped_exchanges_per_cycle"] > 0          # the halo messages fly during the next stage's kernels
    assert c["reductions_per_cycle"] == 1.0    # ONE collective per cycle: the time step and the c_h estimate travel together
    assert c["halo_exchanges_per_cycle"] == 2.0  # one per stage
    # both of them with their x1 strips stored into / read from the message buffers by the stage kernels (warm-up included:
    # per cycle of the run)
    assert c["exchanges_with_x1_strips_in_the_buffers_per_cycle"] == 2.0
    assert "cpu_baseline" not in d and "weak_scaling_base_with_ghost_copies" not in d   # N = 1 only
    # value = zones of ALL ranks * steps / max-over-ranks time
    assert abs(d["value"] - 256 * 128 * 128 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]


def test_bench_restarts_on_the_callback_transport_when_a_rank_fails_to_start():
    """a failure on ONE rank during initialisation / warm-up (injected here; on a node it would be the native RCCL
    transport's first real exchange) makes EVERY rank start over with comm='torch' instead of hanging or dying"""
    env = dict(os.environ, APK_SHARE_GPU="1", APK_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1",
               APK_BENCH_INJECT_START_FAILURE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--brick", "64",
           "--meshblock", "32", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "retrying with comm='torch'" in r.stderr and "injected start-up failure on rank 1" in r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    _check_contract(d, 2, 2, 1, full=True)
    assert "torch.distributed callbacks" in d["config"]["comm_backend"]


def test_bench_on_four_ranks_through_the_launcher():
    """the 2 x 2 x 1 rank grid of the 4-GPU run on 64^3 per rank (one GPU shared by four processes: every rank has 3
    peers and a 2 x 2 x 2 brick of meshblocks; the 2 x 2 x 2 grid of the 8-GPU run would put eight processes on the one
    GPU at once; one rank of it is rehearsed in one process: apk_amd/rehearse_remote_faces in tests/test_gpu_driver.py)"""
    d = _launch(4, ["--steps", "2", "--warmup", "1", "--brick", "64", "--meshblock", "32", "--no-cpu-baseline", "--full"],
                timeout=1500)
    _check_contract(d, 4, 2, 1, full=True)
    c = d["config"]
    assert c["mesh"] == [128, 128, 64] and c["blocks_per_gpu"] == 8 and c["parallelism"].endswith("2x2x1 GPU grid")
    assert c["overlapped_exchanges_per_cycle"] > 0 and c["reductions_per_cycle"] == 1.0 and c["halo_exchanges_per_cycle"] == 2.0
    assert c["exchanges_with_x1_strips_in_the_buffers_per_cycle"] == 2.0


def test_bench_on_one_gpu_reports_the_copy_inclusive_base():
    """N = 1 (no launcher): the default figure has no ghost copies at all (direct neighbour addressing); the second
    figure repeats the steps with the same-rank copies an N > 1 run performs between bricks"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--brick", "128", "--meshblock", "64", "--no-cpu-baseline",
                        "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    _check_contract(d, 1, 3, 1, full=True)
    assert d["config"]["same_rank_ghost_copies_skipped_per_cycle"] == 2.0
    base = d["weak_scaling_base_with_ghost_copies"]
    assert 0 < base["value"] <= d["value"] * 1.05 and base["unit"] == "cell-updates/s"
    assert "fused_m12f_kernel" in d["roofline"]["dominant_kernel"] or "fused_dc3" in d["roofline"]["dominant_kernel"]
    assert d["roofline"]["general_stage"]["ms_per_stage"] > 0


def _dump_run(out, extra=()):
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--brick", "64", "--meshblock", "32",
                        "--no-cpu-baseline", "--no-copies-base", "--dump-outputs", str(out)] + list(extra),
                       cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dumps_what_its_timed_steps_computed(tmp_path):
    """--dump-outputs DIR: float64 .npy files of the state the last timed step left (a seeded sample of every meshblock's
    interior), the history sums and time / dt / cycle -- within 64 MB, and the same from run to run: a plain run and one whose
    --full figures follow the timed steps write the same arrays"""
    import numpy as np
    names = ["cons_sample.npy", "cons_sample_index.npy", "history.npy", "time_dt_ncycle.npy"]
    runs = []
    for n, full in enumerate((False, True)):
        out = tmp_path / ("run%d" % n)
        d = _dump_run(out, ["--full"] if full else [])
        _check_contract(d, 1, 2, 1, full)
        assert d["dumped_outputs"]["files"] == names and sorted(os.listdir(out)) == names
        a = {f[:-4]: np.load(out / f) for f in names}
        assert all(v.dtype == np.float64 for v in a.values())
        assert sum(os.path.getsize(out / f) for f in names) <= 64 << 20
        assert a["time_dt_ncycle"][2] == 1 + 3 * 2      # warm-up + three timed regions of --steps cycles, nothing after them
        assert a["time_dt_ncycle"][0] > 0 and a["time_dt_ncycle"][1] > 0
        per_block = 9 * 32 ** 3                          # 8 meshblocks of 32^3 cells, 9 conserved variables of GLM-MHD
        k = d["dumped_outputs"]["values_per_block"]
        assert k == min(per_block, (1 << 21) // 8) and a["cons_sample"].shape == a["cons_sample_index"].shape == (8 * k,)
        idx = a["cons_sample_index"].astype(np.int64)
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 8 * per_block
        assert np.all(np.isfinite(a["cons_sample"]))
        rho = a["cons_sample"][(idx % per_block) < 32 ** 3]     # variable 0 of every block: the density
        assert rho.size > 0 and np.all(rho > 0)
        runs.append(a)
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key


def test_bench_dumps_every_ranks_blocks_through_the_launcher(tmp_path):
    """on N > 1 ranks every rank writes the sample of its own meshblocks; together they cover the mesh once"""
    import numpy as np
    d = _launch(2, ["--steps", "2", "--warmup", "1", "--brick", "64", "--meshblock", "32", "--no-cpu-baseline",
                    "--dump-outputs", str(tmp_path)])
    _check_contract(d, 2, 2, 1, full=False)
    assert sorted(os.listdir(tmp_path)) == ["cons_sample_index_rank0.npy", "cons_sample_index_rank1.npy", "cons_sample_rank0.npy",
                                            "cons_sample_rank1.npy", "history.npy", "time_dt_ncycle.npy"]
    per_block = 9 * 32 ** 3
    gids = []
    for r in range(2):
        v, i = np.load(tmp_path / ("cons_sample_rank%d.npy" % r)), np.load(tmp_path / ("cons_sample_index_rank%d.npy" % r))
        assert v.dtype == i.dtype == np.float64 and v.shape == i.shape and np.all(np.isfinite(v))
        gids.append(set((i.astype(np.int64) // per_block).tolist()))
    assert not gids[0] & gids[1] and gids[0] | gids[1] == set(range(16))
    assert np.load(tmp_path / "time_dt_ncycle.npy")[2] == 1 + 3 * 2
