"""The form apk_stage_form reports is the form apk_stage_fused launches: one stage per form on one small block, the
launches per kernel-timing slot against counts recorded before the plan existed (csrc/stage_form.hpp), and the three older
queries on the pack against apk_stage_form on its descriptor."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from helpers import NHYDRO

pytestmark = pytest.mark.gpu

GAMMA, C_H = 5.0 / 3.0, 1.9
MHD_PPM, MHD_DC, HYDRO_PLM = ("glmmhd", "ppm", "hlld"), ("glmmhd", "dc", "hlld"), ("euler", "plm", "hllc")
SLOTS = ("fused_x1", "fused_x2", "fused_x3", "fused_dc_x1", "fused_dc_x2", "fused_dc_x3")
# name, scheme, block, stage arguments, the form, launches per slot of SLOTS.  The counts were recorded from the launch code
# as it was before plan_stage (same calls, same shapes); they are not derived from the plan.
CASES = [
    ("two_kernel", MHD_PPM, (36, 8, 10), dict(fill_derived=2), "TWO_KERNEL", (1, 0, 1, 0, 0, 0)),
    ("three_sweep", MHD_PPM, (36, 8, 10), dict(fill_derived=1), "THREE_SWEEP", (1, 1, 1, 0, 0, 0)),
    ("single_march", HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=1), "SINGLE_MARCH", (1, 0, 0, 0, 0, 0)),
    ("dc_march", MHD_DC, (36, 8, 10), dict(fill_derived=2), "DC_MARCH", (0, 0, 0, 1, 0, 0)),
    ("march12_x3", MHD_DC, (36, 8, 10), dict(fill_derived=1), "MARCH12_X3", (0, 0, 0, 1, 0, 1)),
    # (phase 2 finishes what phase 1 of the case before it left in the flux-difference workspace)
    ("two_kernel_phase1", MHD_PPM, (36, 8, 10), dict(fill_derived=2, phase=1), "TWO_KERNEL", (0, 0, 1, 0, 0, 0)),
    ("two_kernel_phase2", MHD_PPM, (36, 8, 10), dict(fill_derived=2, phase=2), "TWO_KERNEL", (1, 0, 0, 0, 0, 0)),
]


def run_stage(ctx, scheme, nx, kw):
    """one apk_stage_fused of the case with kernel timing on -> (u0, launches per slot of SLOTS)"""
    import torch
    from athenapk_amd import hydro
    fluid, recon, riemann = scheme
    ng = 3 if recon == "ppm" else 2
    prim = H.random_prim(fluid, nx, ng, seed=17, kind="smooth", nblocks=1)
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    m0 = hydro.MeshData(ctx, nx, ng, NHYDRO[fluid], dx=(0.1, 0.07, 0.13), nblocks=1, cons=cons, prim=prim, with_flux=False)
    m1 = hydro.MeshData(ctx, nx, ng, NHYDRO[fluid], dx=(0.1, 0.07, 0.13), nblocks=1, cons=cons, prim=np.zeros_like(prim), with_flux=False)
    kw = dict(kw)
    if kw.get("phase") == 1:  # the whole block as one window
        kw["window"] = torch.tensor([[0, nx[0] + 2 * ng, ng, ng + nx[0] - 1, ng, ng + nx[1] - 1, ng, ng + nx[2] - 1]],
                                    dtype=torch.int32, device="cuda")
    slots = {name: q for q, name in enumerate(hydro.L.TIMING_SLOTS)}

    def launches():
        out = []
        for name in SLOTS:
            ms, cnt = C.c_double(0.0), C.c_longlong(0)
            assert ctx.lib.apk_kernel_timing_read(ctx.h, slots[name], C.byref(ms), C.byref(cnt)) == 0
            out.append(cnt.value)
        return tuple(out)
    ctx.lib.apk_kernel_timing_enable(ctx.h, 1)
    launches()  # (read = reset)
    hydro.StageFused(m0, m1, fluid, recon, riemann, hydro.L.make_eos(GAMMA), C_H, 0.0, 1.0, 0.004,
                     dedner=1 if fluid == "glmmhd" else 0, glmmhd_alpha=0.1, mindx=0.07, **kw)
    torch.cuda.synchronize()
    n = launches()
    ctx.lib.apk_kernel_timing_enable(ctx.h, 0)
    return m0, n


def stage_args(scheme, fill_derived=0, prim_from_cons=0, phase=0, x1_halo=None):
    from athenapk_amd import hydro
    L = hydro.L
    a = L.StageArgs()
    a.cfg = hydro._cfg(*scheme)
    a.eos = L.make_eos(GAMMA)
    a.c_h, a.gam1, a.beta_dt, a.glmmhd_alpha, a.mindx = C_H, 1.0, 0.004, 0.1, 0.07
    a.dedner = 1 if scheme[0] == "glmmhd" else 0
    a.fill_derived, a.prim_from_cons, a.phase = fill_derived, prim_from_cons, phase
    if phase == 1:
        a.window, a.window_rl, a.window_rows = 8, 3, 1  # (only tested for NULL / against the block's extents)
    if x1_halo is not None:
        a.x1_halo = C.addressof(x1_halo)
    return a


def test_the_reported_form_is_the_form_that_runs(gpu_ctx_strict):
    from athenapk_amd import hydro
    ctx, L = gpu_ctx_strict, hydro.L
    table = L.X1Halo(1, 0, 0, 0)  # (a block table that is only tested for NULL)
    for name, scheme, nx, kw, want_form, want_launches in CASES:
        m0, n = run_stage(ctx, scheme, nx, kw)
        assert n == want_launches, (name, n)
        assert ctx.poll_flags() == 0, name
        rc, info = hydro.StageForm(ctx.lib, m0.desc, stage_args(scheme, **kw))
        assert (rc, info["form"]) == (L.APK_OK, want_form), (name, info)
        # the older queries describe whole stages (phase 0) of this scheme on this pack
        fd, pfc = kw.get("fill_derived", 0), kw.get("prim_from_cons", 0)
        cfg, eos = hydro._cfg(*scheme), L.make_eos(GAMMA)
        whole = hydro.StageForm(ctx.lib, m0.desc, stage_args(scheme, fill_derived=fd, prim_from_cons=pfc))[1]["form"]
        axis = {"TWO_KERNEL": 3, "SINGLE_MARCH": 3, "DC_MARCH": 0, "MARCH12_X3": 0}.get(whole, 1)
        assert ctx.lib.apk_stage_split_axis(m0.h, C.byref(cfg), fd) == axis, name
        prim_free = hydro.StageForm(ctx.lib, m0.desc, stage_args(scheme, prim_from_cons=1))[1]["form"]
        assert ctx.lib.apk_stage_single_march(m0.h, C.byref(cfg)) == (1 if prim_free == "SINGLE_MARCH" else 0), name
        follows = hydro.StageForm(ctx.lib, m0.desc, stage_args(scheme, fill_derived=fd, prim_from_cons=pfc, x1_halo=table))[0] == L.APK_OK
        assert ctx.lib.apk_stage_x1_halo(m0.h, C.byref(cfg), C.byref(eos), fd, 1 if scheme[0] == "glmmhd" else 0, pfc) == (1 if follows else 0), name
