#!/usr/bin/env python
"""What Spitzer conduction costs next to a fixed coefficient, on one GPU in one process (product build): the flux-array
pass (apk_calc_diff_fluxes_v2: three launches, one per direction) and the fused RKL2 sub-stage
(apk_rkl2_substage_fused_v2: one launch) on ONE 64^3 GLM-MHD block, anisotropic conduction alone and with viscosity and
resistivity, each with
  fixed    the fixed coefficient (the kernels of a deck without Spitzer)
  spitzer  chi = kappa(T) mbar / (k_B rho) per cell: two evaluations per face in the pass, seven per cell in the sub-stage.
Per variant: milliseconds per call from device events around a region of calls (median, minimum and maximum of
`--regions` regions after a warm-up, the variants taking turns so that drift hits them alike; a region is as many calls
as fill `--seconds`), and the bytes per second the byte models of kernels_diffusion.hip / kernels_sts.hip give at that
time.  One JSON line per variant, appended to --out.  There is no threshold: the numbers are what they are.

  python tools/spitzer_cost.py [--seconds 0.3] [--regions 5] [--out profiles/spitzer_cost.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, NG = 64, 2
DX = (1.0 / N, 1.0 / N, 1.0 / N)
# bytes per cell the launches must move (the models in the headers of kernels_diffusion.hip and kernels_sts.hip), 3-D GLM-MHD:
# a flux pass reads 8 primitives and reads + writes the touched flux components per direction; conduction alone touches
# the energy flux only (64 + 16), every process six components (64 + 96)
BYTES = {("pass", "cond"): 3 * (64 + 16), ("pass", "all"): 3 * 160, ("fused", "cond"): 496, ("fused", "all"): 496}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="length of a timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "spitzer_cost needs a GPU: there is no CPU fallback"
    import spitzer_cases as SC
    from athenapk_amd import hydro
    from athenapk_amd import lib as L

    ctx = hydro.Context(strict=False)
    nx = (N, N, N)
    prim = SC.make_prim(nx, seed=1, nblocks=1)
    rng = np.random.default_rng(2)
    mk = lambda **kw: hydro.MeshData(ctx, nx, NG, 9, dx=DX, nblocks=1, cons=rng.standard_normal(prim.shape), **kw)
    yjm1 = mk(prim=prim)
    y0, yjm2, my0 = (mk(with_flux=False) for _ in range(3))
    coeffs = hydro.rkl2_coefficients(9, 4)
    spitzer = L.make_spitzer_cfg(*SC.SPITZER)
    # the fixed coefficient: chi of the Spitzer runs at 1e7 K, rho = 1
    kappa = float(np.asarray(SC.SP.chi(np.float64(1.0), np.float64(1.0), spitzer=SC.SPITZER)))

    def cfg(procs, coeff):
        extra = dict(viscosity="isotropic", nu=0.3, resistivity="ohmic", eta=0.45) if procs == "all" else {}
        c = L.make_diff_cfg(conduction="anisotropic", kappa=kappa, sat_phi=SC.SAT_PHI, **extra)
        if coeff == "spitzer":
            c.conduction_coeff = L.DIFF_COEFF["spitzer"]
            c.conduction_sat_prefac = SC.SAT_PREFAC
        return c

    def call(kernel, procs, coeff):
        sp = spitzer if coeff == "spitzer" else None
        if kernel == "pass":
            return lambda: hydro.CalcDiffFluxes(yjm1, cfg(procs, coeff), spitzer=sp)
        return lambda: hydro.RKL2SubstageFused(y0, yjm1, yjm2, my0, cfg(procs, coeff), coeffs, 1e-9, first=False, spitzer=sp)

    variants = [(k, p, c) for k in ("pass", "fused") for p in ("cond", "all") for c in ("fixed", "spitzer")]
    calls = {v: call(*v) for v in variants}

    def region(v, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            calls[v]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    count = {}
    for v in variants:  # warm-up (code objects), and the region's length
        region(v, 5)
        count[v] = max(20, int(a.seconds / (region(v, 20) * 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.regions):
        for v in variants:
            ms[v].append(region(v, count[v]))
    rows = []
    for v in variants:
        med = float(np.median(ms[v]))
        row = {"kernel": v[0], "processes": v[1], "coefficient": v[2], "block": list(nx), "calls_per_region": count[v],
               "ms_median": med, "ms_min": min(ms[v]), "ms_max": max(ms[v]), "model_bytes_per_cell": BYTES[v[:2]],
               "model_bytes_per_s": BYTES[v[:2]] * N ** 3 / (med * 1e-3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
