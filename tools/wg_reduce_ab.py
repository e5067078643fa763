#!/usr/bin/env python
"""What the kernels that end in a workgroup reduction (csrc/wg_reduce.hpp) cost, on one GPU in one process (product
build, or the library APK_LIB_PATH names -- a build of another commit for a same-machine comparison).  On 8 x 128^3 blocks:
  min_dt        apk_estimate_timestep (min_dt_kernel), Euler
  c2p_dt        apk_cons_to_prim_dt, whole blocks (cons_to_prim_kernel<WITH_DT>), Euler
  history       apk_history (history_kernel + final_sum_kernel<8>), Euler
  tag_pgrad     apk_tag_blocks, pressure gradient (tag_kernel), Euler
  cool_dt       apk_estimate_cooling_timestep (cool_dt_kernel), the Schure table on the data of tools/cooling_prof.py
  cond_dt       apk_estimate_diffusion_timestep_v2 (cond_dt_kernel), anisotropic Spitzer conduction on GLM-MHD blocks as
                tools/spitzer_cost.py sets them up
and, because 128^3 blocks are too wide for it and the tracers have no pack,
  tag_from_cons apk_tag_blocks_dt_from_cons (tag_pgrad_from_cons_kernel) on 256 x 32^3 Euler blocks
  lookback      apk_tracers_lookback (its two kernels' wave sums) on 2^22 particles
Every call includes its read-back of the result (a few doubles and a stream synchronisation), the same on both sides of a
comparison.  Per kernel: milliseconds per call from device events around a window of `--calls` calls, `--windows` windows
after a warm-up, the kernels taking turns.  One JSON line per kernel, with what its first call returned (hex floats: the
two sides of a comparison must print the same).  There is no threshold.

  python tools/wg_reduce_ab.py [--label new] [--calls 100] [--windows 5] [--only name,name]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, NB, NG = 128, 8, 2
GAMMA, HE, RHO = 1.6666666666666667, 0.25, 147.7557589278723


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "wg_reduce_ab needs a GPU: there is no CPU fallback"
    import cooling_reference as R
    import spitzer_cases as SC
    from athenapk_amd import hydro
    from athenapk_amd import lib as L

    torch.cuda.set_device(0)
    ctx = hydro.Context(strict=False)
    eos = L.make_eos(GAMMA)
    only = [s for s in a.only.split(",") if s]
    calls = {}

    # Euler, 8 x 128^3: temperatures over 1e4 - 1e8 K as in tools/cooling_prof.py, small velocities that differ by block
    U = R.CLUSTER_UNITS
    mbar_over_kb = R.composition(U, HE)[3]
    nt = N + 2 * NG
    x = (np.arange(nt) - NG + 0.5) / N
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    rng = np.random.default_rng(4)
    prim = np.zeros((NB, 5, nt, nt, nt))
    for b in range(NB):
        logT = 6.0 + 2.0 * np.sin(2 * np.pi * (X + 0.13 * b)) * np.cos(2 * np.pi * Y) * np.cos(np.pi * (Z - 0.5))
        prim[b, 0] = RHO
        prim[b, 1:4] = 0.01 * (1 + b) * rng.standard_normal((3, nt, nt, nt))
        prim[b, 4] = RHO * 10 ** logT.transpose(2, 1, 0) / mbar_over_kb
    import helpers as H
    cons = H.prim_to_cons("euler", prim, GAMMA)
    md = hydro.MeshData(ctx, (N, N, N), NG, 5, dx=(1.0 / N,) * 3, nblocks=NB, cons=cons, prim=prim, with_flux=False)
    rows = R.read_table(os.path.join(ROOT, "tests", "golden", "schure.cooling_1.0Z"))
    tab = hydro.TabularCooling(ctx, rows[0], rows[1], L.make_cooling_params(
        "rk12", cfl=0.1, lambda_units=U.lambda_units(), gamma=GAMMA, mbar_over_kb=mbar_over_kb, He_mass_fraction=HE, mh=U.mh))
    calls["min_dt"] = lambda: hydro.EstimateTimestep(md, "euler", eos, 0.3)
    calls["c2p_dt"] = lambda: hydro.ConservedToPrimitiveDt(md, "euler", eos, 0.3)
    calls["history"] = lambda: hydro.HydroHst(md, "euler")
    calls["tag_pgrad"] = lambda: hydro.TagBlocks(md, "pressure_gradient", 0.5)
    calls["cool_dt"] = lambda: tab.EstimateTimeStep(md)

    # GLM-MHD, 8 x 128^3, Spitzer conduction (tools/spitzer_cost.py's set-up at this size)
    mprim = SC.make_prim((N, N, N), seed=1, nblocks=NB)
    mmd = hydro.MeshData(ctx, (N, N, N), NG, 9, dx=(1.0 / N,) * 3, nblocks=NB, cons=mprim, prim=mprim, with_flux=False)
    spitzer = L.make_spitzer_cfg(*SC.SPITZER)
    cfg = L.make_diff_cfg(conduction="anisotropic", kappa=0.5, sat_phi=SC.SAT_PHI)
    cfg.conduction_coeff = L.DIFF_COEFF["spitzer"]
    cfg.conduction_sat_prefac = SC.SAT_PREFAC
    calls["cond_dt"] = lambda: hydro.EstimateDiffusionTimestep(mmd, cfg, 0.3, spitzer=spitzer)

    # Euler, 256 x 32^3: the criterion and the estimate from the conserved state
    sprim = H.random_prim("euler", (32, 32, 32), NG, seed=5, kind="smooth", nblocks=256)
    smd = hydro.MeshData(ctx, (32, 32, 32), NG, 5, dx=(1.0 / 32,) * 3, nblocks=256, cons=H.prim_to_cons("euler", sprim, GAMMA),
                         with_flux=False)
    calls["tag_from_cons"] = lambda: hydro.TagBlocksDtFromCons(smd, "euler", eos, 0.3, 0.5)

    # 2^22 particles, every one active
    npart = 1 << 22
    g = torch.Generator(device="cuda").manual_seed(6)
    rho = torch.rand(npart, dtype=torch.float64, device="cuda", generator=g) + 0.5
    active = torch.ones(npart, dtype=torch.int32, device="cuda")
    s = torch.randn((L.TRACER_N_LOOKBACK, npart), dtype=torch.float64, device="cuda", generator=g)
    sdot = torch.randn((L.TRACER_N_LOOKBACK, npart), dtype=torch.float64, device="cuda", generator=g)
    calls["lookback"] = lambda: hydro.TracersLookback(ctx, rho, active, s, sdot, 3, 1e-3)

    names = [n for n in calls if not only or n in only]

    def window(name, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            calls[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def flat(r):  # what a call returned, as hex floats: equal bits on both sides of a comparison
        if isinstance(r, torch.Tensor):
            r = r.cpu().numpy()
        if isinstance(r, tuple):
            return [h for x in r for h in flat(x)]
        return [float(v).hex() for v in np.atleast_1d(np.asarray(r, dtype=np.float64)).ravel()]

    result = {}
    for n in names:  # the result of the first call, then a warm-up (code objects, scratch buffers)
        result[n] = flat(calls[n]())
        window(n, 5)
    ms = {n: [] for n in names}
    for _ in range(a.windows):
        for n in names:
            ms[n].append(window(n, a.calls))
    for n in names:
        print(json.dumps({"label": a.label, "kernel": n, "calls_per_window": a.calls, "ms_windows": ms[n],
                          "ms_median": float(np.median(ms[n])), "ms_min": min(ms[n]), "ms_max": max(ms[n]), "first_result": result[n]}), flush=True)
    tab.close()
    ctx.close()


if __name__ == "__main__":
    main()
