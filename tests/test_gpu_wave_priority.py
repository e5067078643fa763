"""The marches of the two-kernel stage set their own issue priority from the share of their march they have left
(wave_priority.hpp): 3 above a half, 2 above a quarter, 1 above an eighth, 0 below -- the x3 sweep per column, the
finishing march per column or ticket piece.  (The donor-cell marches were measured with it and do not keep it; their
stages stay in this test, which is indifferent to where the priority is set.)  A priority changes when a wave's
instructions issue and nothing else, so every stage below must still be the oracle's stage: bit for bit in the parity
build, within the product tolerance in the product build -- state, stored primitives, time step and flag word.

The packs are 5 blocks whose march lengths put the three thresholds in awkward places (a level computed from the wrong
counter, or a threshold of a march shorter than 8 steps, would show up as a march that ends early or late only if it
also changed the loop -- which is what this guards):

  32 x 5 x 12    odd row count: the one-row donor-cell march; 5-row columns (7 steps) in the finishing march
  32 x 6 x 8     8 planes per donor-cell wave (9 steps), 6-row columns (8 steps)
  32 x 16 x 12   one 16-row piece per leftover column
  32 x 42 x 12   pieces of 16, 16 and 10 rows

each at the default wave count (whole columns, the static split) and with APK_MARCH_WAVES=7 (whole columns in
lockstep, then ticket pieces: 40 columns on 7 waves).  One fresh child process per wave count runs everything once
(the hook is read when the library loads); the tests share what it returned and the oracle's stages."""
import functools
import os
import tempfile

import numpy as np
import pytest

import helpers as H
from _spawn import spawn
from helpers import NGHOST, NHYDRO
from test_gpu_parity import _cmp  # (the existing comparison rules: bitwise / FAST_TOL)

pytestmark = pytest.mark.gpu

GAMMA = 5.0 / 3.0
C_H = 1.9
NB = 5
DX = (0.1, 0.07, 0.13)
BDT = 0.004
PACKS = {"32x5x12": (32, 5, 12), "32x6x8": (32, 6, 8), "32x16x12": (32, 16, 12), "32x42x12": (32, 42, 12)}
WAVES = (None, 7)
# name: (recon, gam0, input from the conserved state)
STAGES = {
    "ppm_hlld_gam0_zero": ("ppm", 0.0, False),
    "ppm_hlld_gam0_half": ("ppm", 0.5, False),
    "dc_hlld_from_prim": ("dc", 0.0, False),
    "dc_hlld_from_cons": ("dc", 0.0, True),
}
FLUID, RIEMANN = "glmmhd", "hlld"


def _ng(recon):
    return 2 if recon == "dc" else NGHOST[recon]


@functools.lru_cache(maxsize=None)
def _inputs(stage, pack):
    """(ng, geometry, input primitives, u0.cons, u1.cons) of a case; with input from the conserved state the primitives
    are the ones ConsToPrim derives from it (what the finishing sweep of the stage before would have stored)"""
    recon, gam0, from_cons = STAGES[stage]
    nx, ng = PACKS[pack], _ng(recon)
    prim = H.random_prim(FLUID, nx, ng, seed=31 + len(stage) + nx[1], kind="smooth", nblocks=NB)
    g = H.geom(FLUID, nx, ng, 0, DX)
    cons = H.prim_to_cons(FLUID, prim, GAMMA)
    if from_cons:
        _, prim, bad = H.orc_c2p(FLUID, g, cons.copy(), H.O.make_eos(GAMMA))
        assert bad == 0
    u1c = cons * 1.01 if gam0 != 0.0 else cons
    return ng, g, prim, cons, u1c


@functools.lru_cache(maxsize=None)
def _oracle(stage, pack):
    """(cons, prim, dt) of the reference stage, computed once and left unchanged"""
    recon, gam0, from_cons = STAGES[stage]
    ng, g, prim, cons, u1c = _inputs(stage, pack)
    want = H.orc_stage(FLUID, recon, RIEMANN, g, cons, u1c, prim, GAMMA, C_H, gam0, 1.0 - gam0, BDT, dedner=1, alpha=0.1, mindx=0.07)
    want, want_prim, bad = H.orc_c2p(FLUID, g, want, H.O.make_eos(GAMMA))
    assert bad == 0
    return want, want_prim, 0.3 * H.orc_min_dt(FLUID, g, want_prim, GAMMA)


def _run_stage(ctx, stage, pack):
    """one stage on context ctx: (cons, u1.prim, dt, flags)"""
    from athenapk_amd import hydro
    recon, gam0, from_cons = STAGES[stage]
    nx = PACKS[pack]
    ng, g, prim, cons, u1c = _inputs(stage, pack)
    nv = NHYDRO[FLUID]
    # (input from the conserved state: u0's primitives hold NaN, u1.cons is the state)
    m0 = hydro.MeshData(ctx, nx, ng, nv, dx=DX, nblocks=NB, cons=cons, prim=np.full_like(prim, np.nan) if from_cons else prim, with_flux=False)
    m1 = hydro.MeshData(ctx, nx, ng, nv, dx=DX, nblocks=NB, cons=u1c, prim=np.full_like(prim, -7.0), with_flux=False)
    ctx.poll_flags()
    hydro.StageFused(m0, m1, FLUID, recon, RIEMANN, hydro.L.make_eos(GAMMA), C_H, gam0, 1.0 - gam0, BDT, dedner=1,
                     glmmhd_alpha=0.1, mindx=0.07, fill_derived=2, estimate_dt=True, prim_from_cons=from_cons)
    dt = hydro.StageDt(ctx, 0.3)
    flags = ctx.poll_flags()
    return [m0.cons_host(), m1.prim_host(), np.array([dt]), np.array([flags], dtype=np.int64)]


def _child(rank, port, waves, path):
    if waves is None:
        os.environ.pop("APK_MARCH_WAVES", None)
    else:
        os.environ["APK_MARCH_WAVES"] = str(waves)  # (before the library loads: read once per process)
    import torch
    from athenapk_amd import hydro
    torch.cuda.set_device(0)
    res = {}
    for strict in (True, False):
        ctx = hydro.Context(strict=strict)
        for stage in STAGES:
            for pack in PACKS:
                for q, a in enumerate(_run_stage(ctx, stage, pack)):
                    res["%s/%s/%d/%d" % (stage, pack, int(strict), q)] = a
        ctx.close()
    np.savez(path, **res)


@functools.lru_cache(maxsize=None)
def _results(waves):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.npz")
        spawn(_child, lambda port: (port, waves, path), 1)
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@pytest.mark.parametrize("waves", WAVES, ids=["default_waves", "7_waves"])
@pytest.mark.parametrize("pack", list(PACKS))
@pytest.mark.parametrize("stage", list(STAGES))
def test_stage_with_wave_priorities_is_the_oracle_stage(oracle, stage, pack, waves):
    """parity build: bit for bit; product build: within the product tolerance; no flag raised"""
    nx, ng = PACKS[pack], _ng(STAGES[stage][0])
    want_cons, want_prim, want_dt = _oracle(stage, pack)
    res = _results(waves)
    for strict in (True, False):
        cons, prim, dt, flags = (res["%s/%s/%d/%d" % (stage, pack, int(strict), q)] for q in range(4))
        what = "%s %s %s" % (stage, pack, "strict" if strict else "fma")
        assert flags[0] == 0, what
        _cmp(H.interior(cons, nx, ng), H.interior(want_cons, nx, ng), strict, what + " cons")
        _cmp(H.interior(prim, nx, ng), H.interior(want_prim, nx, ng), strict, what + " u1.prim")
        if strict:
            assert dt[0] == want_dt, what
        else:
            assert dt[0] == pytest.approx(want_dt, rel=1e-12), what


@pytest.mark.parametrize("stage", list(STAGES))
def test_both_wave_counts_give_the_same_bits(stage):
    """whole columns and ticket pieces follow the same rule: 7 waves = the default, both builds, every output"""
    a, b = _results(7), _results(None)
    for k in sorted(a):
        if k.startswith(stage + "/"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
