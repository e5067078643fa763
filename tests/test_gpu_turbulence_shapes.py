"""The few-modes turbulence kernels (csrc/kernels_turb.hip) across block shapes, mode counts and sum paths.

Where the shapes of the inverse-transform table come from.  The product build's fmft_inverse_rows_kernel works with
  kRowsPerWave = 8    (j, k) rows of a block per wave, and 4 waves per workgroup: a "group" is 32 rows, a block has
                      ceil(nx2 nx3 / 32) groups; rows past nx2 nx3 are clamped to the last one for the loads and guarded
                      at the store; a wave whose first row is past the end does all of it for nothing
  128 columns a pass  two x1 columns per lane (io, io + 64): ceil(nx1 / 128) passes; columns past nx1 are clamped and guarded
  kModeChunk = 10     modes per trip through the registers: Mpad = ceil(M / 10) 10, the padding's coefficients are zero
  LDS                 4 waves x 8 rows x Mpad x 6 doubles = 1536 Mpad bytes; above 65536 (Mpad >= 50, M >= 41) the launch
                      needs hipFuncSetAttribute; a wave forms its coefficients with lane = mode, so Mpad > 64 is a second
                      trip of that loop
  kMaxRowModes = 64   above it the general fmft_inverse_kernel runs in the product build too
  blockIdx.x          = (block * groups + group) * passes + pass
so the table takes, per constant:
  3 x (24, 6, 5),   8 modes  kRowsPerWave: 30 rows, the last wave has 6 live rows and 2 clamped; three different extents
                             (an exchange of nx2 and nx3 in the phase indexing or in k = row / nx2 shows)
  2 x (40, 3, 3),  10 modes  4 waves: 9 rows, waves 2 and 3 wholly past the end; kModeChunk: no padding
  3 x (72, 7, 5),  41 modes  35 rows: two groups, 3 rows in the second; columns: the second column lives in lanes 0..7
                             only; LDS: Mpad = 50, 76800 bytes, the smallest launch that needs the opt-in
  2 x (128, 4, 3), 40 modes  columns: both full; LDS: 61440 bytes, the largest launch without the opt-in
  3 x (130, 6, 6), 30 modes  two passes (the second with 2 live columns), two groups and three blocks at once: the one
                             combination where blockIdx.x can be decoded wrongly without a fault; the deck's mode count
  2 x (16, 8, 4),  64 modes  kMaxRowModes: Mpad = 70, lanes 0..5 take the second trip of the coefficient loop; 107520 bytes
  2 x (16, 8, 4),  65 modes  above kMaxRowModes: the general kernel
  1 x (8, 8, 8),    1 mode   kModeChunk: one live mode, nine padded
  2 x (40, 12, 1),  8 modes  a 2-D pack (nx3 = 1: k = 0 for every row)
If one of these constants moves, the table moves with it.

The sums (csrc/wg_reduce.hpp's contract) are held bit for bit in the parity build, which contracts nothing and rounds
its divides and square roots correctly; tests/helpers.py restates the order, this module the kernels' per-cell terms.
"""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

GAMMA = 5.0 / 3.0
FAST_TOL = 1e-12
NG = 2
BOTH = pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])


def _stream():
    from athenapk_amd import hydro
    return hydro._stream()


def _ctx(request, strict):
    return request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")


def _cmp(got, want, strict, what):
    """test_gpu_parity._cmp on finite data: bit for bit, or FAST_TOL of max|want|; returns the scaled error"""
    scale = np.max(np.abs(want)) + 1e-300
    err = float(np.max(np.abs(got - want)) / scale)
    if strict:
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: %d entries differ bitwise (scaled %.3e), first at %s: %r vs %r" % (
            what, len(bad), err, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    else:
        assert err <= FAST_TOL, "%s: max scaled error %.3e" % (what, err)
    return err


def _ghost_mask(shape, nx):
    m = np.ones(shape, bool)
    H.interior(m, nx, NG)[...] = False
    return m


# ---- 1. the inverse transform ------------------------------------------------------------------------------------------
# (nblocks, (nx1, nx2, nx3), modes): the docstring's table
INVERSE_CASES = [(3, (24, 6, 5), 8), (2, (40, 3, 3), 10), (3, (72, 7, 5), 41), (2, (128, 4, 3), 40), (3, (130, 6, 6), 30),
                 (2, (16, 8, 4), 64), (2, (16, 8, 4), 65), (1, (8, 8, 8), 1), (2, (40, 12, 1), 8)]
# blocks inside a periodic box of GN cells per axis: every block and every axis at an offset of its own (no two phase
# tables alike); the blocks do not tile the box, and the last x1 offset wraps a long row around the box's end
GN = 192
OFFSETS = [(3, 50, 101), (140, 17, 77), (66, 181, 9)]


def _k_vec(nmodes):
    """test_gpu_parity._turb_case's eight wave vectors, extended with integer components in [-3, 3], no zero vector"""
    kv = np.array([[1, 0, 0, 1, 2, 0, -1, 2], [0, 1, 0, 1, -1, 2, 1, 2], [0, 0, 1, -1, 0, 1, 2, 2]], dtype=np.float64)
    if nmodes > 8:
        rng = np.random.default_rng(5)
        kv = np.concatenate([kv, rng.integers(-3, 4, size=(3, nmodes - 8)).astype(np.float64)], axis=1)
        kv[:, np.all(kv == 0, axis=0)] = 1.0
    return np.ascontiguousarray(kv[:, :nmodes])


_INVERSE = {}


def _inverse_case(oracle, nb, nx, nmodes):
    """spectral state, phases and the oracle's field of a case, computed once for both builds"""
    key = (nb, nx, nmodes)
    if key not in _INVERSE:
        f = oracle.Fmft(oracle.load(), _k_vec(nmodes), k_peak=2.0, sol_weight=0.7, t_corr=0.5, rseed=7)
        f.evolve(0.1)
        f.evolve(0.1)
        g = H.geom("glmmhd", nx, NG, 0, (1.0 / GN,) * 3)
        phases = [tuple(f.phases(d, nx[d], OFFSETS[b][d], GN) for d in range(3)) for b in range(nb)]
        want = np.stack([f.inverse(g, *phases[b]) for b in range(nb)])
        want.setflags(write=False)
        _INVERSE[key] = (f.var_hat(), g, phases, want)
    return _INVERSE[key]


@BOTH
@pytest.mark.parametrize("nb,nx,nmodes", INVERSE_CASES, ids=["%dx%dx%dx%d_%dmodes" % ((c[0],) + c[1] + (c[2],)) for c in INVERSE_CASES])
def test_fmft_inverse_across_the_branches(request, oracle, strict, nb, nx, nmodes):
    """FewModesFT.Inverse against the oracle on the docstring's table: nothing outside the interior is written (NaN
    before, NaN after), the interior is finite and is the oracle's -- bit for bit in the parity build, within FAST_TOL of
    max|want| in the product build (whose regrouped sum, in plain float64 without FMA, is within 6e-16 of scale of the
    oracle at these shapes: the bound leaves room for the reference alone)."""
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    var_hat, g, phases, want = _inverse_case(oracle, nb, nx, nmodes)
    md = hydro.MeshData(ctx, nx, NG, 9, dx=tuple(g.dx), nblocks=nb, with_flux=False, row_pitch="natural")
    drv = hydro.FewModesFT(md, [[p.transpose(2, 1, 0) for p in blk] for blk in phases])
    assert drv.num_modes == nmodes
    drv.acc.fill_(float("nan"))
    drv.Inverse(var_hat)
    got = drv.acc_host()
    ghost = _ghost_mask(got.shape, nx)
    assert np.all(np.isnan(got[ghost])), "%d cells outside the interior were written" % np.sum(~np.isnan(got[ghost]))
    gi, wi = H.interior(got, nx, NG), H.interior(want, nx, NG)
    assert np.all(np.isfinite(gi)), "%d interior cells are not finite" % np.sum(~np.isfinite(gi))
    assert np.max(np.abs(wi)) > 0.1
    err = _cmp(gi, wi, strict, "acc")
    print("fmft inverse %d x %s, %d modes, %s build: scaled error %.3e" % (nb, nx, nmodes, "parity" if strict else "product", err))


# ---- 2. the Perturb kernels on non-cubic, tiled and anisotropic packs -------------------------------------------------------
# flattened lanes with isotropic cells; (64, 4) tiles partial in both directions with every factor of the volume distinct
PERTURB_SHAPES = [(3, (24, 6, 5), (1 / 48,) * 3), (3, (72, 7, 5), (1 / 48, 1 / 40, 1 / 36))]
SHAPES = pytest.mark.parametrize("nb,nx,dx", PERTURB_SHAPES, ids=["flat_24x6x5", "tiles_72x7x5_aniso"])
_STATE = {}


def _state(nb, nx, kind="smooth", seed=21):
    """primitives, conserved state and a random acceleration field (ghost zones included), computed once"""
    key = (nb, nx, kind, seed)
    if key not in _STATE:
        prim = H.random_prim("glmmhd", nx, NG, seed=seed, kind=kind, nblocks=nb)
        cons = H.prim_to_cons("glmmhd", prim, GAMMA)
        acc = np.random.default_rng(seed + 10).uniform(-1.0, 1.0, (nb, 3) + prim.shape[2:])
        _STATE[key] = (prim, cons, acc)
    return _STATE[key]


def _box_volume(nb, nx, dx):
    return nb * nx[0] * nx[1] * nx[2] * (dx[0] * dx[1] * dx[2])


def _driver(hydro, ctx, nb, nx, dx, cons, prim, acc, nhydro=9, row_pitch="natural"):
    md = hydro.MeshData(ctx, nx, NG, nhydro, dx=dx, nblocks=nb, cons=cons, prim=prim, with_flux=False, row_pitch=row_pitch)
    ph = [np.zeros((2, 1, n)) for n in nx]  # (one mode; the field is uploaded, not transformed)
    drv = hydro.FewModesFT(md, [ph] * nb)
    import torch
    drv.acc.copy_(torch.from_numpy(np.ascontiguousarray(acc)))
    return md, drv


@BOTH
@SHAPES
def test_perturb_and_history_on_shapes(request, oracle, strict, nb, nx, dx):
    """test_gpu_parity.test_turbulence_perturb_and_history's assertions, on packs whose lanes are flattened rows with a
    tail and (64, 4) tiles partial in both directions, the latter with dx1, dx2, dx3 all different.  box_volume is the
    pack's summed cell volume, so the normalised field's RMS is accel_rms."""
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    prim, cons, acc = _state(nb, nx)
    g = H.geom("glmmhd", nx, NG, 0, dx)
    md, drv = _driver(hydro, ctx, nb, nx, tuple(g.dx), cons, prim, acc)
    vol = _box_volume(nb, nx, tuple(g.dx))
    drv.Perturb(0.01, 0.5, vol)
    want_u, want_a = H.orc_turb_perturb(g, cons, acc, 0.01, 0.5, vol)
    got_u, got_a = md.cons_host(), drv.acc_host()
    # the two global sums are accumulated in a different order than the oracle's serial loop
    np.testing.assert_allclose(got_a, want_a, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got_u, want_u, rtol=1e-12, atol=1e-14)
    assert not np.array_equal(H.interior(got_u, nx, NG)[:, 1:5], H.interior(cons, nx, NG)[:, 1:5])
    # ghost zones untouched, of cons, acc and prim (which this form of the kick leaves alone altogether)
    assert np.array_equal(got_u[_ghost_mask(got_u.shape, nx)], cons[_ghost_mask(cons.shape, nx)])
    assert np.array_equal(got_a[_ghost_mask(got_a.shape, nx)], acc[_ghost_mask(acc.shape, nx)])
    assert np.array_equal(md.prim_host(), prim)
    # RMS of the normalised field is accel_rms
    a = H.interior(got_a, nx, NG)
    assert abs(np.sqrt((a ** 2).sum(axis=1).mean()) - 0.5) < 1e-12
    for fluid in ("glmmhd", "euler"):
        got = hydro.TurbulenceHst(md, fluid, GAMMA)
        want = H.orc_turb_history(fluid, g, prim, GAMMA)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


@BOTH
@pytest.mark.parametrize("floors", [False, True], ids=["nofloor", "floors"])
@SHAPES
def test_kick_with_fill_derived_and_dt_on_shapes(request, oracle, strict, floors, nb, nx, dx):
    """test_gpu_parity.test_turbulence_kick_with_fill_derived_and_dt's assertions on the same two packs: the fused kick =
    the kick, then ConsToPrim of the interior, then the time-step estimate (which, with three different dx, takes
    its minimum over three different ratios)."""
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    prim, cons, acc = _state(nb, nx)
    dx = tuple(H.geom("glmmhd", nx, NG, 0, dx).dx)
    vol = _box_volume(nb, nx, dx)
    eos = hydro.L.make_eos(GAMMA, pfloor=0.9, dfloor=0.95) if floors else hydro.L.make_eos(GAMMA)

    def run(fill):
        md, drv = _driver(hydro, ctx, nb, nx, dx, cons, np.full_like(prim, -3.0), acc)
        if fill is None:
            drv.Perturb(0.01, 0.5, vol)
            hydro.ConservedToPrimitive(md, "glmmhd", eos)
            dt = hydro.EstimateTimestep(md, "glmmhd", eos, 0.3)
        else:
            drv.Perturb(0.01, 0.5, vol, fill=fill)
            dt = hydro.StageDt(ctx, 0.3)
        ctx.poll_flags()
        return md.cons_host(), md.prim_host(), drv.acc_host(), dt
    a, b = run(("glmmhd", eos, True)), run(None)
    # apk_turb_apply_dt: the same kick and estimate, primitives left alone
    c = run(("glmmhd", eos, True, False))
    assert np.array_equal(c[0], a[0]) and np.array_equal(c[2], a[2]) and c[3] == a[3]
    assert np.all(c[1] == -3.0)
    assert np.array_equal(H.interior(a[0], nx, NG), H.interior(b[0], nx, NG)) and np.array_equal(a[2], b[2])
    # (product build: ConsToPrim inlined behind the kick contracts into FMAs differently from the separate kernel)
    _cmp(H.interior(a[1], nx, NG), H.interior(b[1], nx, NG), strict, "prim")
    assert a[3] == b[3] if strict else abs(a[3] - b[3]) <= 1e-12 * b[3]
    assert 0 < a[3] < 1
    ghost = _ghost_mask(a[1].shape, nx)
    assert np.all(a[1][ghost] == -3.0) and np.array_equal(a[0][ghost], cons[ghost])   # ghost zones untouched
    assert np.array_equal(a[2][_ghost_mask(a[2].shape, nx)], acc[_ghost_mask(acc.shape, nx)])
    if floors:  # (the floors act: the density differs from the unfloored kick's, which leaves it alone)
        assert not np.array_equal(H.interior(a[0], nx, NG)[:, 0], H.interior(cons, nx, NG)[:, 0])


# ---- 3. the turbulence sums in the stated order (parity build, bit for bit) -----------------------------------------------
B0 = 0.37


def _at(a, nx, n, dk=0, dj=0, di=0):
    n1, n2, n3 = nx
    return a[:, n, NG + dk:NG + dk + n3, NG + dj:NG + dj + n2, NG + di:NG + di + n1]


def _mean_momentum_terms(nx, dx, cons, acc):
    """turb_mean_momentum_kernel's four terms of every interior cell, operation for operation: [4, nb, n3, n2, n1]"""
    vol = dx[0] * dx[1] * dx[2]
    den = _at(cons, nx, 0)
    return np.stack([den * vol] + [den * _at(acc, nx, c) * vol for c in range(3)])


def _remove_mean_terms(nx, dx, acc, sums4):
    """turb_remove_mean_kernel: the host's three means, the shifted field and the cell's term: ([1, ...], [nb, 3, ...])"""
    sqr = lambda x: x * x
    vol = dx[0] * dx[1] * dx[2]
    a = [_at(acc, nx, c) - sums4[c + 1] / sums4[0] for c in range(3)]
    return (sqr(a[0]) * vol + sqr(a[1]) * vol + sqr(a[2]) * vol)[None], np.stack(a, axis=1)


def _turb_history_terms(fluid, nx, dx, prim, gamma):
    """turb_history_kernel<FLUID>: [3, nb, n3, n2, n1], zeros in the two magnetic columns for Euler"""
    vol = dx[0] * dx[1] * dx[2]
    w = lambda n: _at(prim, nx, n)
    d, p = w(0), w(4)
    vel2 = w(1) * w(1) + w(2) * w(2) + w(3) * w(3)
    c_s = np.sqrt(gamma * p / d)
    e_kin = 0.5 * d * vel2
    h = np.zeros((3,) + d.shape)
    h[0] = np.sqrt(vel2) / c_s * vol
    if fluid == "glmmhd":
        e_mag = 0.5 * (w(5) * w(5) + w(6) * w(6) + w(7) * w(7))
        assert np.all(e_mag != 0)
        h[1] = np.sqrt(e_kin / e_mag) * vol
        h[2] = p / e_mag * vol
    return h


def _reldivb_terms(nx, dx, cons, b0):
    """user_reldivb_kernel on a 3-D pack: [1, nb, n3, n2, n1]"""
    sqr = lambda x: x * x
    vol = dx[0] * dx[1] * dx[2]
    divb = (_at(cons, nx, 5, di=1) - _at(cons, nx, 5, di=-1)) / dx[0] + (_at(cons, nx, 6, dj=1) - _at(cons, nx, 6, dj=-1)) / dx[1]
    divb = divb + (_at(cons, nx, 7, dk=1) - _at(cons, nx, 7, dk=-1)) / dx[2]
    return (0.5 * np.sqrt(sqr(dx[0]) + sqr(dx[1]) + sqr(dx[2])) * np.abs(divb) / b0 * vol)[None]


def _mean_momentum(md, drv):
    ctx, sums = md.ctx, np.zeros(4)
    assert ctx.lib.apk_turb_mean_momentum(ctx.h, md.h, drv.h, sums.ctypes.data_as(C.POINTER(C.c_double)), _stream()) == 0
    return sums


def _remove_mean(md, drv, sums4):
    ctx, ampl = md.ctx, np.zeros(1)
    dp = C.POINTER(C.c_double)
    assert ctx.lib.apk_turb_remove_mean(ctx.h, md.h, drv.h, sums4.ctypes.data_as(dp), ampl.ctypes.data_as(dp), _stream()) == 0
    return ampl


def _reldivb(md, b0):
    ctx, out = md.ctx, np.zeros(1)
    assert ctx.lib.apk_history_user_reldivb(ctx.h, md.h, b0, out.ctypes.data_as(C.POINTER(C.c_double)), _stream()) == 0
    return out


def _single(partial):
    return H.final_sum32(partial)


def _two_level(partial):
    return H.final_sum32(H.mid_sum256(partial))


def _device_sums(hydro, md, drv, fluids, reldivb):
    """every sum of kernels_turb.hip on this pack, in launch order: name -> values.  (remove_mean shifts drv.acc.)"""
    got = {"mean_momentum": _mean_momentum(md, drv)}
    got["remove_mean"] = _remove_mean(md, drv, got["mean_momentum"])
    for fluid in fluids:
        got["history_" + fluid] = hydro.TurbulenceHst(md, fluid, GAMMA)
    if reldivb:
        got["reldivb"] = _reldivb(md, B0)
    return got


def _restated_partials(nx, dx, cons, prim, acc, fluids, reldivb, sums4):
    """the same sums' per-workgroup rows from the restated terms; sums4: the means remove_mean is given.  Also returns
    the shifted acceleration field remove_mean leaves behind and two other sums of every quantity's terms."""
    terms = {"mean_momentum": _mean_momentum_terms(nx, dx, cons, acc)}
    terms["remove_mean"], shifted = _remove_mean_terms(nx, dx, acc, sums4)
    for fluid in fluids:
        terms["history_" + fluid] = _turb_history_terms(fluid, nx, dx, prim, GAMMA)
    if reldivb:
        terms["reldivb"] = _reldivb_terms(nx, dx, cons, B0)
    partial = {k: H.wg_partial_sums(h, nx) for k, h in terms.items()}
    # two other sums of the same terms: the exactly rounded one, and the oracle's serial loop over the cells
    exact = {k: np.array([math.fsum(hq.ravel()) for hq in h]) for k, h in terms.items()}
    serial = {k: np.array([np.cumsum(hq.ravel())[-1] for hq in h]) for k, h in terms.items()}
    return partial, shifted, (exact, serial)


def _check_sums(got, partial, others, level, other_level):
    """got = level(rows) bit for bit for every kernel.  That the data tell orders of additions apart is asserted first:
    a balanced tree over positive terms often lands on the exactly rounded sum of one quantity, so, as in
    test_history_sums_in_the_stated_order, that sum has to differ in at least one of the pack's quantities; the serial
    loop's sum has to differ in at least one quantity of every kernel; and where the pack sits at the threshold between
    one level of sums and two, the other path's sum in at least one of the pack's quantities."""
    exact, serial = others
    want = {name: level(rows) for name, rows in partial.items()}
    for name, rows in partial.items():
        print(name, "rows", len(rows), "got", got[name].tolist(), "want", want[name].tolist(), "exact", exact[name].tolist(),
              "serial", serial[name].tolist())
        live = want[name] != 0  # (Euler's two magnetic columns are sums of zeros)
        assert live[0] and (name == "history_euler" or np.all(live))
        assert np.any(want[name] != serial[name]), name + ": this data does not tell the tree from a serial loop"
    assert any(np.any(want[k] != exact[k]) for k in want), "this data does not tell one order of additions from another"
    if other_level is not None:
        assert any(np.any(want[k] != other_level(partial[k])) for k in want), "this data does not tell one level of sums from two"
    for name in partial:
        assert np.array_equal(got[name], want[name]), name


@SHAPES
def test_turbulence_sums_in_the_stated_order(request, nb, nx, dx):
    """turb_mean_momentum_kernel (4 sums), turb_remove_mean_kernel (1), turb_history_kernel (3, Euler and GLM-MHD) and
    user_reldivb_kernel (1), bit for bit: wg_reduce.hpp's order on the kernels' own per-cell terms, as
    test_history_sums_in_the_stated_order holds history_kernel to it.  The data tell orders apart (_check_sums)."""
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    prim, cons, acc = _state(nb, nx, kind="rough")
    dx = tuple(H.geom("glmmhd", nx, NG, 0, dx).dx)
    md, drv = _driver(hydro, ctx, nb, nx, dx, cons, prim, acc)
    got = _device_sums(hydro, md, drv, ("glmmhd", "euler"), True)
    partial, shifted, exact = _restated_partials(nx, dx, cons, prim, acc, ("glmmhd", "euler"), True, got["mean_momentum"])
    assert len(partial["reldivb"]) <= 2048
    _check_sums(got, partial, exact, _single, None)
    after = drv.acc_host()
    assert np.array_equal(H.interior(after, nx, NG), shifted)
    assert np.array_equal(after[_ghost_mask(after.shape, nx)], acc[_ghost_mask(acc.shape, nx)])


def _random_pack(nb, nx, nhydro, seed):
    """admissible random states without a Python loop over the blocks: (cons, prim, acc), whole arrays"""
    rng = np.random.default_rng(seed)
    shp = (nb,) + H.block_shape(nx, NG, nhydro)
    lo = np.array([0.1, -1.5, -1.5, -1.5, 0.05, -1.2, -1.2, -1.2, -0.3][:nhydro]).reshape(1, -1, 1, 1, 1)
    hi = np.array([2.0, 1.5, 1.5, 1.5, 3.0, 1.2, 1.2, 1.2, 0.3][:nhydro]).reshape(1, -1, 1, 1, 1)
    prim = rng.random(shp)
    prim *= hi - lo
    prim += lo
    cons = prim  # (the sums read the density and B of it only: any admissible values do)
    acc = rng.random((nb, 3) + shp[2:])
    acc -= 0.5
    return cons, prim, acc


@pytest.mark.parametrize("nb,fluid", [(512, "glmmhd"), (513, "glmmhd"), (16385, "euler")],
                         ids=["2048_rows_one_level", "2052_rows_two_levels", "65540_rows_two_rows_a_thread"])
def test_turbulence_sums_across_the_middle_level(request, nb, fluid):
    """finish_sums' two paths on blocks of (8, 4, 4), one workgroup per plane.  512 blocks: 2048 rows, the last pack
    final_sum_kernel takes alone.  513 blocks: 2052 rows, mid_sum_kernel with chunk = 9 and its groups 228..255 empty.
    16385 blocks: 65540 rows, chunk = 257, so thread 0 of every group adds two rows.  Bit for bit against
    helpers.mid_sum256 / final_sum32 on the restated terms, and the data tell the two paths apart."""
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    nx, dx = (8, 4, 4), (1 / 64, 1 / 48, 1 / 40)
    nhydro = H.NHYDRO[fluid]
    cons, prim, acc = _random_pack(nb, nx, nhydro, seed=nb)
    md, drv = _driver(hydro, ctx, nb, nx, dx, cons, prim, acc, nhydro=nhydro)
    mhd = fluid == "glmmhd"
    fluids = ("glmmhd", "euler") if mhd else ("euler",)
    got = _device_sums(hydro, md, drv, fluids, mhd)
    partial, shifted, exact = _restated_partials(nx, dx, cons, prim, acc, fluids, mhd, got["mean_momentum"])
    nwg = len(partial["mean_momentum"])
    assert nwg == 4 * nb
    if nwg > 2048:
        assert -(-nwg // 256) == {513: 9, 16385: 257}[nb]
        _check_sums(got, partial, exact, _two_level, _single)
    else:
        _check_sums(got, partial, exact, _single, _two_level)
    assert np.array_equal(H.interior(drv.acc_host(), nx, NG), shifted)


# ---- 4. through the driver -------------------------------------------------------------------------------------------------
def _deck_k_vec():
    from athenapk_amd import decks
    kv, block = {}, None
    for line in decks.load("turbulence").splitlines():
        line = line.split("#")[0].strip()
        if line.startswith("<"):
            block = line.strip("<>")
        elif "=" in line and block == "modes":
            k, v = [x.strip() for x in line.split("=")]
            kv[k] = int(v)
    n = len(kv) // 3
    return np.array([[kv["k_%d_%d" % (m + 1, d)] for m in range(n)] for d in range(3)], dtype=np.float64)


@BOTH
def test_turbulence_driver_with_a_row_tail_and_45_modes(oracle, strict):
    """The turbulence deck on 24^3 in 24 x 12 x 6 meshblocks -- 8 blocks of 72 rows: two full groups and one of 8 rows,
    nx2 != nx3 -- with 45 modes (the deck's 30 and 15 more by overrides: Mpad = 50, the LDS opt-in), 3 cycles, compared
    with the oracle's mini-driver as test_gpu_driver.test_turbulence_driver_matches_oracle does."""
    import os
    from athenapk_amd import decks, driver
    kv = _deck_k_vec()
    assert kv.shape == (3, 30)
    extra = np.random.default_rng(45).integers(-3, 4, size=(3, 15)).astype(np.float64)
    extra[:, np.all(extra == 0, axis=0)] = 1.0
    kv = np.concatenate([kv, extra], axis=1)
    ov = ["parthenon/mesh/nx1=24", "parthenon/mesh/nx2=24", "parthenon/mesh/nx3=24", "parthenon/meshblock/nx1=24",
          "parthenon/meshblock/nx2=12", "parthenon/meshblock/nx3=6", "problem/turbulence/b_config=0",
          "problem/turbulence/num_modes=45"]
    ov += ["modes/k_%d_%d=%d" % (m + 1, d, int(kv[d, m])) for m in range(30, 45) for d in range(3)]
    s = driver.Simulation(decks.load("turbulence"), ov, strict=strict)
    s.set_fused(True)
    s.initialize()
    o = oracle.Sim(fluid="glmmhd", recon="plm", riemann="hlle", integrator="vl2", nx=(24, 24, 24), mb=(24, 12, 6),
                   ng=2, cfl=0.3, gamma=1.0001, nthreads=min(16, os.cpu_count()))
    o.pgen("turbulence", k_vec=kv, b_config=0)
    np.testing.assert_allclose(s.gather("cons"), o.gather_cons(), rtol=1e-14, atol=0)
    for _ in range(3):
        s.step()
        o.step()
    assert np.array_equal(s.fmft_var_hat(), o.var_hat())
    assert abs(s.time - o.time) <= 1e-13 * o.time
    np.testing.assert_allclose(s.gather("cons"), o.gather_cons(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(s.turbulence_history(), o.turb_history(), rtol=1e-10)
    np.testing.assert_allclose(s.history(), o.history(), rtol=1e-11, atol=1e-14)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
@BOTH
def test_packs_with_explicit_strides_are_refused_and_left_alone(request, strict):
    """The acceleration field is addressed with the pack's cell offsets, so every entry point that touches it refuses
    a pack with explicit strides with APK_ERR_UNSUPPORTED before it writes anything.  (The two history sums read the
    pack alone and take it: the same bits as on the natural layout.)"""
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    ctx = _ctx(request, strict)
    nb, nx, dx = PERTURB_SHAPES[0]
    prim, cons, acc = _state(nb, nx)
    md, drv = _driver(hydro, ctx, nb, nx, dx, cons, prim, acc, row_pitch="aligned")
    assert md.pitch != nx[0] + 2 * NG
    eos = L.make_eos(GAMMA)
    vh = np.ones((3, 1, 2))
    sums4 = np.array([1.0, 0.1, 0.2, 0.3])
    calls = {
        "inverse": lambda: drv.Inverse(vh),
        "mean_momentum, remove_mean, apply": lambda: drv.Perturb(0.01, 0.5, 1.0),
        "remove_mean": lambda: _remove_mean_rc(md, drv, sums4),
        "apply": lambda: hydro._check(ctx.lib.apk_turb_apply(ctx.h, md.h, drv.h, 1.5, 0.01, _stream()), ctx.lib, ctx.h),
        "apply_fill": lambda: hydro._check(ctx.lib.apk_turb_apply_fill(ctx.h, md.h, drv.h, 1.5, 0.01, L.FLUID["glmmhd"], C.byref(eos), 1, _stream()), ctx.lib, ctx.h),
        "apply_fill without dt": lambda: hydro._check(ctx.lib.apk_turb_apply_fill(ctx.h, md.h, drv.h, 1.5, 0.01, L.FLUID["glmmhd"], C.byref(eos), 0, _stream()), ctx.lib, ctx.h),
        "apply_dt": lambda: hydro._check(ctx.lib.apk_turb_apply_dt(ctx.h, md.h, drv.h, 1.5, 0.01, L.FLUID["glmmhd"], C.byref(eos), _stream()), ctx.lib, ctx.h),
    }
    for name, call in calls.items():
        with pytest.raises(L.ApkError) as e:
            call()
        assert e.value.code == L.APK_ERR_UNSUPPORTED, name
        assert np.array_equal(drv.acc_host(), acc), name
        assert np.array_equal(md.cons_host(), cons) and np.array_equal(md.prim_host(), prim), name
    if strict:
        nat, _ = _driver(hydro, ctx, nb, nx, dx, cons, prim, acc)
        for fluid in ("glmmhd", "euler"):
            assert np.array_equal(hydro.TurbulenceHst(md, fluid, GAMMA), hydro.TurbulenceHst(nat, fluid, GAMMA))
        assert np.array_equal(_reldivb(md, B0), _reldivb(nat, B0))


def _remove_mean_rc(md, drv, sums4):
    from athenapk_amd import hydro
    ctx, ampl = md.ctx, np.zeros(1)
    dp = C.POINTER(C.c_double)
    hydro._check(ctx.lib.apk_turb_remove_mean(ctx.h, md.h, drv.h, sums4.ctypes.data_as(dp), ampl.ctypes.data_as(dp), _stream()), ctx.lib, ctx.h)


@BOTH
def test_fmft_create_refuses_empty_descriptors(request, strict):
    from athenapk_amd import lib as L
    ctx = _ctx(request, strict)
    blocks = (L.FmftBlock * 1)()
    for nblocks, num_modes in [(0, 8), (-1, 8), (1, 0), (1, -3)]:
        h = C.c_void_p(0xdead)
        assert ctx.lib.apk_fmft_create(ctx.h, blocks, nblocks, num_modes, C.byref(h)) == L.APK_ERR_INVALID
