"""The finishing march's dynamic leftover phase (fused2_kernel.hpp): packs with at least as many columns as the device
holds waves hand their leftover rows out piece by piece, from a ticket word.  Which wave marches a row must not enter its
result, so every stage below is run in fresh child processes that differ only in APK_MARCH_WAVES -- the test hook of
resident_march_waves(), set before the library loads -- and the results are compared bit for bit:

  default  more waves than columns: whole columns only / the static split (today's small-pack schedule)
  32       40 columns on 32 waves: one whole column per wave, 8 leftover columns as tickets
  7        40 columns on 7 waves: five whole columns per wave, 5 leftover columns

The pack is 5 blocks of 32 x 16 x 12 cells: 8 chunks per block, 40 columns, 640 wave-rows -- one 16-row piece per leftover
column.  The 42-row pack has pieces of 16, 16 and 10 rows per leftover column: 24 tickets on 32 waves, 15 on 7 waves,
where every wave draws several.  One child per wave count runs all cases once; the tests share what it returned and
leave it unchanged."""
import functools
import os
import tempfile

import numpy as np
import pytest

import helpers as H
from _spawn import spawn
from helpers import NGHOST, NHYDRO

pytestmark = pytest.mark.gpu

GAMMA = 5.0 / 3.0
C_H = 1.9
NB = 5
NX = (32, 16, 12)
NX_SHORT = (32, 42, 12)  # 42 rows: 16 + 16 + 10, the short last piece (no multiple of 8 or 11 either)
WAVES = (None, 32, 7)

MHD, HYDRO = ("glmmhd", "ppm", "hlld"), ("euler", "plm", "hllc")
# name: (strict, scheme, nx, gam0, x1_halo)
CASES = {
    "parity_gam0_zero": (True, MHD, NX, 0.0, False),
    "parity_gam0_half": (True, MHD, NX, 0.5, False),
    "product": (False, MHD, NX, 0.0, False),
    "product_gam0_half": (False, MHD, NX, 0.5, False),
    "hydro_plm_hllc": (True, HYDRO, NX, 0.5, False),
    "x1_halo": (True, MHD, NX, 0.0, True),
    "short_last_piece": (True, MHD, NX_SHORT, 0.5, False),
}


def _inputs(name):
    strict, (fluid, recon, riemann), nx, gam0, halo = CASES[name]
    ng = NGHOST[recon]
    prim = H.random_prim(fluid, nx, ng, seed=7 + len(name), kind="smooth", nblocks=NB)
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    u1c = cons * 1.01 if gam0 != 0.0 else cons
    return ng, prim, cons, u1c


def _run_stage(ctx, name):
    """one stage of case `name` on context ctx: (cons, u1.prim, dt, flags [, send segments])"""
    import torch
    from athenapk_amd import hydro
    strict, (fluid, recon, riemann), nx, gam0, halo = CASES[name]
    ng, prim, cons, u1c = _inputs(name)
    nv, dx = NHYDRO[fluid], (0.1, 0.07, 0.13)
    m0 = hydro.MeshData(ctx, nx, ng, nv, dx=dx, nblocks=NB, cons=cons, prim=prim, with_flux=False)
    m1 = hydro.MeshData(ctx, nx, ng, nv, dx=dx, nblocks=NB, cons=u1c, prim=np.full_like(prim, -7.0), with_flux=False)
    xh, send = None, []
    if halo:
        # every x1 face has a receive segment holding the block's own ghost columns (so that the stage computes what it
        # computes without the table) and a one-column send segment
        ks, js = slice(ng, ng + nx[2]), slice(ng, ng + nx[1])
        cols = lambda b, side: np.ascontiguousarray(prim[b][:, ks, js, (ng + nx[0] if side else 0):(ng + nx[0] if side else 0) + ng])
        recv = [tuple(torch.tensor(cols(b, side), device="cuda") for side in range(2)) for b in range(NB)]
        send = [tuple(torch.full((nv, nx[2], nx[1], 1), -3.0, dtype=torch.float64, device="cuda") for side in range(2)) for b in range(NB)]
        xh = dict(recv=recv, send=send, recv_depth=ng, send_depth=1, send_field=0)
    ctx.poll_flags()
    hydro.StageFused(m0, m1, fluid, recon, riemann, hydro.L.make_eos(GAMMA), C_H, gam0, 1.0 - gam0, 0.004,
                     dedner=1 if fluid == "glmmhd" else 0, glmmhd_alpha=0.1, mindx=0.07, fill_derived=2, estimate_dt=True, x1_halo=xh)
    dt = hydro.StageDt(ctx, 0.3)
    flags = ctx.poll_flags()
    out = [m0.cons_host(), m1.prim_host(), np.array([dt]), np.array([flags], dtype=np.int64)]
    if halo:
        out.append(np.stack([np.stack([t.cpu().numpy() for t in pair]) for pair in send]))
    return out


def _child(rank, port, waves, path):
    """child process: every case on a context of its own, then the ticket-word sequence on ONE context"""
    if waves is None:
        os.environ.pop("APK_MARCH_WAVES", None)
    else:
        os.environ["APK_MARCH_WAVES"] = str(waves)  # (before the library loads: read once per process)
    import torch
    from athenapk_amd import hydro
    torch.cuda.set_device(0)
    res = {}
    for name, case in CASES.items():
        ctx = hydro.Context(strict=case[0])
        for q, a in enumerate(_run_stage(ctx, name)):
            res["%s/%d" % (name, q)] = a
        ctx.close()
    # the same context three times in a row, the second time on a different pack: a ticket word left over from one
    # launch would send the next launch's waves home early: cells not updated
    ctx = hydro.Context(strict=True)
    for rep, name in enumerate(["parity_gam0_half", "short_last_piece", "parity_gam0_half"]):
        for q, a in enumerate(_run_stage(ctx, name)):
            res["repeat%d/%d" % (rep, q)] = a
    ctx.close()
    np.savez(path, **res)


@functools.lru_cache(maxsize=None)
def _results(waves):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.npz")
        spawn(_child, lambda port: (port, waves, path), 1)
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


def _of(res, name):
    return [res[k] for k in sorted(res) if k.startswith(name + "/")]


def _assert_same(a, b, what):
    assert len(a) == len(b) and len(a) >= 4
    for q, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), \
            "%s: output %d (cons, prim, dt, flags, send) differs in %d entries" % (what, q, int(np.sum(x != y)))


@pytest.mark.parametrize("waves", [32, 7])
@pytest.mark.parametrize("name", ["parity_gam0_zero", "parity_gam0_half"])
def test_parity_build_is_bit_for_bit_across_schedules(name, waves):
    """conserved state, stored primitives, time-step word and flag words: static schedule = 32 waves = 7 waves"""
    _assert_same(_of(_results(waves), name), _of(_results(None), name), "%s, %d waves against the default" % (name, waves))


@pytest.mark.parametrize("name", ["parity_gam0_zero", "parity_gam0_half", "hydro_plm_hllc"])
def test_static_schedule_result_is_the_oracle_stage(oracle, name):
    """... and what they all equal is the reference stage of tests/helpers.py, bit for bit as in the parity suite"""
    strict, (fluid, recon, riemann), nx, gam0, halo = CASES[name]
    ng, prim, cons, u1c = _inputs(name)
    g = H.geom(fluid, nx, ng, 0, (0.1, 0.07, 0.13))
    ded = 1 if fluid == "glmmhd" else 0
    want = H.orc_stage(fluid, recon, riemann, g, cons, u1c, prim, GAMMA, C_H, gam0, 1.0 - gam0, 0.004, dedner=ded, alpha=0.1, mindx=0.07)
    want_cons, want_prim, bad = H.orc_c2p(fluid, g, want, oracle.make_eos(GAMMA))
    got_cons, got_prim, dt, flags = _of(_results(None), name)[:4]
    assert bad == 0 and flags[0] == 0
    assert np.array_equal(H.interior(got_cons, nx, ng), H.interior(want_cons, nx, ng)), "cons"
    assert np.array_equal(H.interior(got_prim, nx, ng), H.interior(want_prim, nx, ng)), "u1.prim"
    assert dt[0] == 0.3 * H.orc_min_dt(fluid, g, want_prim, GAMMA)


@pytest.mark.parametrize("waves", [32, 7])
@pytest.mark.parametrize("name", ["product", "product_gam0_half", "hydro_plm_hllc", "x1_halo"])
def test_product_build_hydro_and_x1_halo_forms_are_bit_for_bit(name, waves):
    """the product build too: the schedule changes no arithmetic instruction"""
    _assert_same(_of(_results(waves), name), _of(_results(None), name), "%s, %d waves against the default" % (name, waves))


@pytest.mark.parametrize("waves", [32, 7])
def test_short_last_piece(waves):
    """42 rows per column: the last piece of every leftover column is shorter than the others, and on 7 waves every
    wave draws several tickets (15 pieces of 5 leftover columns)"""
    _assert_same(_of(_results(waves), "short_last_piece"), _of(_results(None), "short_last_piece"), "%d waves" % waves)


@pytest.mark.parametrize("waves", [32, 7])
def test_ticket_words_are_fresh_for_every_launch(waves):
    """three stages in a row on one context equal the same stages on fresh contexts"""
    res = _results(waves)
    for rep, name in enumerate(["parity_gam0_half", "short_last_piece", "parity_gam0_half"]):
        _assert_same(_of(res, "repeat%d" % rep), _of(res, name), "launch %d on a used context (%s)" % (rep, name))
        _assert_same(_of(res, "repeat%d" % rep), _of(_results(None), name), "launch %d against the static schedule" % rep)
