#!/usr/bin/env python
"""Times one RKL2 sub-stage on one GPU three ways, in one process (GLM-MHD, 8 x 128^3, conduction + viscosity +
resistivity, product build):
  (a) the kernels an array sub-stage is made of that exist without super-time-stepping: the three apk_calc_diff_fluxes
      passes and apk_update_with_flux_divergence;
  (b) the full array sub-stage: three flux memsets, apk_calc_diff_fluxes, apk_rkl2_step_other;
  (c) the fused sub-stage kernel, apk_rkl2_substage_fused.
Each figure is the median over three regions of `reps` back-to-back calls between device events, after a warm-up.  Prints
the three times, their ratios and the achieved bytes/s of the byte model of kernels_sts.hip against a device-to-device
copy measured the same way, and appends them to profiles/sts_kernel_stats.csv (--csv).

  python tools/sts_prof.py [--n 128] [--blocks 8] [--reps 20] [--csv profiles/sts_kernel_stats.csv]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--csv", default=None)
    a = ap.parse_args()
    import torch
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    assert torch.cuda.is_available(), "sts_prof needs a GPU: there is no CPU fallback"
    ctx = hydro.Context(strict=False)
    n, nb, ng = a.n, a.blocks, 2
    nx = (n, n, n)
    g = torch.Generator(device="cuda").manual_seed(1)
    shape = (nb, 9, n + 2 * ng, n + 2 * ng, n + 2 * ng)
    prim = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) + 0.5
    dx = (1.0 / n,) * 3
    mk = lambda **kw: hydro.MeshData(ctx, nx, ng, 9, dx=dx, nblocks=nb, cons=prim, row_pitch="aligned", **kw)
    base = mk(prim=prim, with_flux=True)
    y0, yjm2, my0 = (mk(with_flux=False) for _ in range(3))
    cfg = L.make_diff_cfg(conduction="anisotropic", kappa=1e-3, viscosity="isotropic", nu=1e-3, resistivity="ohmic", eta=1e-3)
    k = hydro.rkl2_coefficients(21, 7)
    tau = 1e-6

    def part_a():
        hydro.CalcDiffFluxes(base, cfg)
        hydro.UpdateWithFluxDivergence(base, y0, 1.0, 0.0, tau)

    def part_b():
        for d in range(3):
            base.flux[d].zero_()
        hydro.CalcDiffFluxes(base, cfg)
        hydro.RKL2StepOther(y0, base, yjm2, my0, k[0], k[1], k[2], k[3], tau)

    def part_c():
        hydro.RKL2SubstageFused(y0, base, yjm2, my0, cfg, k, tau, first=False)

    src, dst = base.prim, torch.empty_like(base.prim)

    def copy():
        dst.copy_(src)

    def region(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    parts = {"a_parent_kernels": part_a, "b_array_substage": part_b, "c_fused_substage": part_c, "copy": copy}
    for fn in parts.values():  # warm-up: code objects, caches
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in parts}
    for _ in range(3):  # regions alternate between the variants
        for name, fn in parts.items():
            ms[name].append(region(fn))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    cells = nb * n ** 3
    bytes_model = {"a_parent_kernels": 3 * 160 + 3 * 72 + 3 * 72, "b_array_substage": 1344, "c_fused_substage": 496}
    copy_rate = 2 * src.numel() * 8 / (med["copy"] * 1e-3)
    rows = []
    for name in ("a_parent_kernels", "b_array_substage", "c_fused_substage"):
        rate = bytes_model[name] * cells / (med[name] * 1e-3)
        rows.append((name, med[name], min(ms[name]), max(ms[name]), bytes_model[name], rate, rate / copy_rate))
        print("%-18s %8.3f ms (regions %.3f .. %.3f)  model %4d B/cell  %7.1f GB/s  %.2f of the copy rate"
              % (name, med[name], min(ms[name]), max(ms[name]), bytes_model[name], rate / 1e9, rate / copy_rate))
    print("copy               %8.3f ms  %7.1f GB/s (read + write)" % (med["copy"], copy_rate / 1e9))
    print("a / c = %.3f   b / c = %.3f   fused below the parent kernels: %s"
          % (med["a_parent_kernels"] / med["c_fused_substage"], med["b_array_substage"] / med["c_fused_substage"],
             med["c_fused_substage"] < med["a_parent_kernels"]))
    if a.csv:
        new = not os.path.exists(a.csv)
        with open(a.csv, "a") as f:
            if new:
                f.write("what,blocks,n,median_ms,min_ms,max_ms,model_bytes_per_cell,bytes_per_s,share_of_copy_rate\n")
            for r in rows:
                f.write("%s,%d,%d,%.4f,%.4f,%.4f,%d,%.4e,%.3f\n" % (r[0], nb, n, r[1], r[2], r[3], r[4], r[5], r[6]))
            f.write("copy,%d,%d,%.4f,%.4f,%.4f,16,%.4e,1.000\n" % (nb, n, med["copy"], min(ms["copy"]), max(ms["copy"]), copy_rate))


if __name__ == "__main__":
    main()
