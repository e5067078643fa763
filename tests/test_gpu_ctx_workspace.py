"""The scratch a context owns -- its device words, its pinned host block and the buffers that grow on demand -- under a
change of pack: one context sees a small pack, a larger one and the small one again; every result must equal, bit for
bit, what a fresh context that only ever saw that pack returns.  Covers growth of each buffer (partials, FOFC marks,
the two stage workspaces, the tag words), their reuse after growth, the end-of-cycle gather with and without pending
tag criteria, the consume-on-read of the stage's minimum, and that no pinned region is overwritten by a neighbour (a
history read sits between the stage launch and the read of its words).  Parity build; contexts of its own, so that
every buffer starts empty."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

GAMMA, C_H, CFL = 5.0 / 3.0, 1.7, 0.3

# 1 block of 8^3, hydro; 8 blocks of 16^3, GLM-MHD with one passive scalar.  (The fused stage refuses count_unphysical
# on packs with passive scalars, so the larger pack runs the counting stage on its nine hydro variables and a second,
# estimate_dt-only stage with the scalar, which is the one that sizes the mass-flux workspace.)
SMALL = dict(fluid="euler", riemann="hllc", nx=(8, 8, 8), nblocks=1, nscalars=0, fast=4.0, beta_dt=0.1, seed=5)
LARGE = dict(fluid="glmmhd", riemann="hlld", nx=(16, 16, 16), nblocks=8, nscalars=1, fast=1.0, beta_dt=0.002, seed=6)
NG, DX = 2, (0.1, 0.07, 0.13)


def _stage(ctx, m0, m1, fluid, riemann, count):
    """apk_stage_fused with fill_derived = 2, estimate_dt (and count_unphysical); returns the status"""
    from athenapk_amd import hydro, lib as L
    a = L.StageArgs()
    a.cfg = hydro._cfg(fluid, "plm", riemann)
    a.eos = L.make_eos(GAMMA)
    a.c_h, a.gam0, a.gam1, a.beta_dt = C_H, 0.25, 0.75, 0.004
    a.dedner, a.glmmhd_alpha, a.mindx = (1 if fluid == "glmmhd" else 0), 0.1, min(DX)
    a.fill_derived, a.estimate_dt, a.count_unphysical = 2, 1, int(count)
    return ctx.lib.apk_stage_fused(ctx.h, m0.h, m1.h, C.byref(a), hydro._stream())


def _stage_words(ctx, m0, fluid):
    """what the driver reads after a stage, with a history read in between: (history, dt, flags, dt again, bad cells)"""
    from athenapk_amd import hydro
    hst = hydro.HydroHst(m0, fluid)
    dt, flags, n = C.c_double(0.0), C.c_uint(0), C.c_longlong(-1)
    hydro._check(ctx.lib.apk_stage_dt_flags_read(ctx.h, CFL, C.byref(dt), C.byref(flags), hydro._stream()), ctx.lib, ctx.h)
    again = hydro.StageDt(ctx, CFL)  # (the minimum has been taken out of the device word: the context remembers it)
    hydro._check(ctx.lib.apk_stage_unphysical_read(ctx.h, C.byref(n), hydro._stream()), ctx.lib, ctx.h)
    return hst, np.float64(dt.value), flags.value, np.float64(again), n.value


def _visit(ctx, fluid, riemann, nx, nblocks, nscalars, fast, beta_dt, seed):
    """every call that goes through the context's scratch, on packs built from the same seeded arrays"""
    from athenapk_amd import hydro, lib as L
    nh, eos = H.NHYDRO[fluid], L.make_eos(GAMMA)
    prim = H.random_prim(fluid, nx, NG, nscalars=nscalars, seed=seed, kind="shock", nblocks=nblocks)
    prim[:, 4] *= 1e-3  # very cold (and, the hydro pack, fast): an explicit step drives trial pressures negative in
    prim[:, 1:4] *= fast  # part of the cells, so that both counters count something
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    u1 = cons * (1.0 + 1e-3 * np.random.default_rng(seed).standard_normal(cons.shape))

    def pack(c, p=None, scalars=nscalars, flux=False):
        nv = nh + scalars
        return hydro.MeshData(ctx, nx, NG, nh, nscalars=scalars, dx=DX, nblocks=nblocks, cons=c[:, :nv],
                              prim=None if p is None else p[:, :nv], with_flux=flux)

    out = {}
    md = pack(cons, prim)
    out["dt"] = np.float64(hydro.EstimateTimestep(md, fluid, eos, CFL))
    out["history"] = hydro.HydroHst(md, fluid)
    bad = cons.copy()
    ii = H.interior(bad, nx, NG)
    ii[-1, 0, 0, 0, -1] = -1.0
    ii[-1, 0, -1, -1, 0] = -2.0
    ii[0, 4, 1, 2, 3] = 0.0
    out["unphysical"] = hydro.CountUnphysical(pack(bad), fluid)
    assert out["unphysical"] == 3
    # FirstOrderFluxCorrect after a flux call
    m0, m1 = pack(cons, prim, flux=True), pack(cons)
    hydro.CalculateFluxes(m0, fluid, "plm", riemann, eos, C_H)
    out["fofc"] = hydro.FirstOrderFluxCorrect(m0, m1, fluid, eos, C_H, 0.0, 1.0, beta_dt)
    assert 0 < out["fofc"] < nblocks * nx[0] * nx[1] * nx[2], "test data must trigger corrections in part of the cells"
    out["fofc_flux"] = np.stack([m0.flux_host(d) for d in range(3)])
    # the counting stage, its words read the way the driver reads them; criteria of a tag launch ride along with the gather
    m0, m1 = pack(cons, prim, scalars=0), pack(u1, np.full_like(prim, -7.0), scalars=0)
    assert _stage(ctx, m0, m1, fluid, riemann, count=True) == L.APK_OK, ctx.lib.apk_last_error(ctx.h)
    pending, code = C.c_int(0), L.TAG_CRITERIA["pressure_gradient"]
    hydro._check(ctx.lib.apk_tag_blocks_begin(ctx.h, m1.h, code, C.byref(pending), hydro._stream()), ctx.lib, ctx.h)
    out["stage_words"] = _stage_words(ctx, m0, fluid)
    tags, crit = (C.c_int * nblocks)(), (C.c_double * nblocks)()
    hydro._check(ctx.lib.apk_tag_blocks_end(ctx.h, nblocks, code, pending.value, 0.5, 0.0, tags, crit, hydro._stream()), ctx.lib, ctx.h)
    out["stage_cons"], out["stage_prim"] = m0.cons_host(), m1.prim_host()
    out["tags_gathered"] = np.array(tags[:]), np.array(crit[:])
    if nscalars:
        m0, m1 = pack(cons, prim), pack(u1, np.full_like(prim, -7.0))
        assert _stage(ctx, m0, m1, fluid, riemann, count=True) == L.APK_ERR_UNSUPPORTED
        assert _stage(ctx, m0, m1, fluid, riemann, count=False) == L.APK_OK, ctx.lib.apk_last_error(ctx.h)
        out["scalar_stage_words"] = _stage_words(ctx, m0, fluid)[:4]
        out["scalar_stage_cons"], out["scalar_stage_prim"] = m0.cons_host(), m1.prim_host()
    # a tag criterion by itself: begin / end with no gather in between
    out["tags"] = hydro.TagBlocks(md, "pressure_gradient", 0.5)
    out["flags_left"] = ctx.poll_flags()
    return out


def _same(got, want, where):
    if isinstance(want, tuple):
        assert len(got) == len(want), where
        for n, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (where, n))
    elif isinstance(want, np.ndarray):
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), where
    else:
        assert type(got) is type(want) and np.array([got]).tobytes() == np.array([want]).tobytes(), (where, got, want)


def test_results_do_not_depend_on_what_the_context_saw_before():
    from athenapk_amd import hydro
    want = {}
    for name, case in (("small", SMALL), ("large", LARGE)):
        fresh = hydro.Context(strict=True)
        want[name] = _visit(fresh, **case)
        fresh.close()
    # the stage's minimum is there at the second read, and the counting stage of these data counts something
    for w in want.values():
        hst, dt, flags, again, nbad = w["stage_words"]
        _same(again, dt, "repeated read")
        assert nbad > 0
    ctx = hydro.Context(strict=True)
    for name, case in (("small", SMALL), ("large", LARGE), ("small", SMALL)):
        got = _visit(ctx, **case)
        assert got.keys() == want[name].keys()
        for key in got:
            _same(got[key], want[name][key], "%s pack, %s" % (name, key))
    ctx.close()
