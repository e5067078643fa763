"""Tabular cooling on the GPU, cell by cell on 360 interior cells (two workgroups, the second partial, the boundary
between the two blocks inside the first): adaptive subcycling (d_e_tol > 0), whose reject / clamp / retry / floor /
grow branches diverge from lane to lane, against the numpy restatement within a tolerance taken from the restatement's
own conditioning; and Townsend's integration against the closed form of the power-law table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cooling_cases as C  # noqa: E402
import cooling_reference as R  # noqa: E402
from cooling_cases import MBAR_GM1_OVER_KB, NB, NG, NX_TWO_WG, T_FLOOR  # noqa: E402
from golden import make_cooling_tables as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _src_flags(ctx, fluid, o, integ):
    """the source term without TabularCooling.SrcTerm's own reading of the flags: (cons on the host, the flag word)"""
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    ctx.poll_flags()
    u, prim = o["u"], o["prim"]
    md = hydro.MeshData(ctx, NX_TWO_WG, NG, u.shape[1], dx=(0.1, 0.1, 0.1), nblocks=NB, cons=u, prim=prim)
    tab = hydro.TabularCooling(ctx, o["rows"][0], o["rows"][1], C.params(integ, **o["kw"]))
    hydro._check(ctx.lib.apk_tabular_cooling_src(ctx.h, md.h, tab.h, L.FLUID[fluid], float(o["dt"]), hydro._stream()),
                 ctx.lib, ctx.h)
    flags = ctx.poll_flags()
    return md.cons_host(), flags


@pytest.mark.parametrize("integ,fluid,table,regime", C.ADAPTIVE_CASES)
def test_adaptive_src_term_per_cell(gpu_ctx_strict, gpu_ctx_fast, integ, fluid, table, regime):
    """rk12 / rk45 with error control, per cell: the parity build within tol_cell of the restatement, the product
    build within tol_cell of the parity build (cooling_cases.adaptive_restated: tol_cell is 1e-12 but for the few
    cells whose restated result itself moves by more under a 1e-13 change of the rates); cells the restatement
    leaves alone or at the floor bit for bit; nothing but IEN of interior cells changes; no failure flag"""
    from athenapk_amd import lib as L
    o = C.adaptive_restated(integ, fluid, table, regime)
    u, mask, want, tol, a, e0 = o["u"], o["mask"], o["want"], o["tol"], o["a"], o["e0"]
    ok = ~np.isnan(want)
    cooled = (a != e0) & ok
    # the inputs: most cells cooled, and all but a few well conditioned, so that the tolerance cannot hide a failure
    assert cooled.sum() >= NB * mask.sum() // 2, "the source cooled too few cells to test anything"
    assert (tol[cooled] > 1e-12).mean() <= 0.08 and (tol[cooled] > 1e-9).mean() <= 0.04, tol[cooled]
    assert tol[cooled].max() <= 1e-6, tol[cooled].max()

    got, flags = _src_flags(gpu_ctx_strict, fluid, o, integ)
    fast, flags_fast = _src_flags(gpu_ctx_fast, fluid, o, integ)
    for f in (flags, flags_fast):
        assert not f & (L.APK_FLAG_COOL_MAX_ITER | L.APK_FLAG_COOL_TABLE), f
    for res in (got, fast):
        for b in range(NB):
            assert np.array_equal(_bits(np.delete(res[b], 4, axis=0)), _bits(np.delete(u[b], 4, axis=0)))
            assert np.array_equal(_bits(res[b][4][~mask]), _bits(u[b][4][~mask]))  # ghost cells are not cooled
    g = np.concatenate([got[b][4][mask] for b in range(NB)])
    f = np.concatenate([fast[b][4][mask] for b in range(NB)])
    assert np.array_equal(np.isnan(g), ~ok) and np.array_equal(np.isnan(f), ~ok)
    err = np.abs(g[ok] - want[ok]) / (tol[ok] * np.abs(want[ok]))
    err_fast = np.abs(f[ok] - g[ok]) / (tol[ok] * np.abs(g[ok]))
    print("adaptive %s %s %s regime %d: parity/restatement %.3g of tol_cell, product/parity %.3g, tol_cell > 1e-12 on "
          "%.1f%% of the cooled cells, largest %.2g" % (integ, fluid, table, regime, err.max(), err_fast.max(),
                                                       100.0 * (tol[cooled] > 1e-12).mean(), tol[cooled].max()))
    assert err.max() <= 1.0, (err.max(), np.flatnonzero(ok)[np.argmax(err)])
    assert err_fast.max() <= 1.0, (err_fast.max(), np.flatnonzero(ok)[np.argmax(err_fast)])
    alone, at_floor = (a == e0) | ~ok, a == o["T"].e_floor_sub  # (NaN is left alone too)
    assert alone.any() and np.array_equal(_bits(g[alone]), _bits(o["ien"][alone]))
    assert np.array_equal(_bits(g[at_floor]), _bits(want[at_floor]))


@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("t_floor", [T_FLOOR, -1.0])
@pytest.mark.parametrize("dt", [2e-2, 1.0])
def test_townsend_against_the_closed_form_per_cell(gpu_ctx_strict, gpu_ctx_fast, fluid, t_floor, dt):
    """Townsend on the power-law table against analytic_e, on the cells that start inside the table and whose exact
    final temperature is 0.1 % above max(T_floor, the table's lower end); with T_floor = -1 e_floor_town is negative
    and the table's lower end is the floor.  Bound: max(1e-12, 8 x the restatement's own largest deviation from the
    closed form on those cells); that deviation is 4.2e-15 at dt = 2e-2 (cells cross up to 5 bins) and 1.3e-14 at
    dt = 1 (up to 54 bins), so 1e-12 binds."""
    rows = C.rows("power_law")
    mhd = fluid == "glmmhd"
    T = C.restated(rows, "townsend", T_floor=t_floor)
    u, prim, mask = C.state(fluid, T, rows[0], C.ADAPTIVE_SEED, NX_TWO_WG)
    rho, e0, ien = (np.concatenate(v) for v in zip(*(C.cells(u[b], mhd, mask) for b in range(NB))))
    crossed = []
    restated = np.array([R.townsend_cell(T, float(r), float(e), dt, crossed) for r, e in zip(rho, e0)])
    with np.errstate(invalid="ignore"):
        exact = R.analytic_e(C.U, C.HE, C.GAMMA, (M.LOG_TEMP0, M.LOG_TEMP1), (M.LOG_LAMBDA0, M.LOG_LAMBDA1), e0, dt)(rho)
        temp0 = MBAR_GM1_OVER_KB * e0
        sel = ((temp0 >= T.temp_cool_floor) & (temp0 <= T.temp_final) &
               (MBAR_GM1_OVER_KB * exact > 1.001 * max(t_floor, T.temp_cool_floor)))
    assert sel.sum() >= 100
    if dt == 1.0:
        assert (np.array(crossed) >= 3).sum() >= 100
    own = np.max(np.abs(restated[sel] - exact[sel]) / exact[sel])
    tol = max(1e-12, 8.0 * own)
    for build, ctx in (("parity", gpu_ctx_strict), ("product", gpu_ctx_fast)):
        got, _, _ = C.src(ctx, fluid, rows, C.params("townsend", T_floor=t_floor), u, prim, dt, NX_TWO_WG)
        g = np.concatenate([got[b][4][mask] for b in range(NB)])
        e1 = e0 + (g - ien) / rho  # (to 3e-14 of e1: the initial IEN is at most 107 times rho * e1 on the selected cells)
        dev = np.abs(e1[sel] - exact[sel]) / exact[sel]
        print("townsend %s T_floor %g dt %g %s: %.3g from the closed form (the restatement: %.3g) on %d cells" %
              (fluid, t_floor, dt, build, dev.max(), own, sel.sum()))
        assert dev.max() <= tol, (build, dev.max(), own)
        # (and the whole pack against the restatement, as the fixed-substep test does)
        want = ien + rho * (restated - e0)
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(g), ~ok)
        assert np.all(np.abs(g[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]))
