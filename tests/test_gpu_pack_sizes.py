"""The HIP kernels at the pack sizes production runs, and past 65535 planes per launch, against the oracle.

The other parity tests use packs of 1-3 small blocks of one dx.  Several launch choices depend on the pack: the segment
count of a march (march_segments), the rows per wave (march_rows_per_wave), the donor-cell predictor's segment length
(its cost model in launch_dc_march), the two-row donor-cell march (even nx2 >= 4), the XCD-dealt grids and du_pitch.
And many launches put nx3 * nblocks (3-D) or nblocks (1-D, 2-D) into grid y or z.  Every pack here gives its blocks
their own data (own phases, every third block a shock instead of a wave) and their own dx (levels 0-2 mixed), so a
mixed-up block index or dx changes the answer.

Rules as in test_gpu_parity.py: the parity build bit for bit (NaNs in the same places), the product build within
FAST_TOL, reductions with the tolerances they have there.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers as H
from helpers import NGHOST, NHYDRO
from test_gpu_parity import FAST_TOL, _cmp  # noqa: F401  (the existing comparison rules)

pytestmark = pytest.mark.gpu

GAMMA = 5.0 / 3.0
C_H = 1.9
CFL = 0.3
DX0 = (0.1, 0.07, 0.13)
THREADS = 16  # oracle threads (ctypes releases the GIL in the oracle's calls)
HOST_BUDGET = 5e9  # bytes of host memory the oracle threads of one test may hold at once
_AMP = [0.3, 0.4, 0.3, 0.2, 0.4, 0.5, 0.5, 0.5, 0.05]
_BASE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
_SHOCK_L = [1.0, 0.75, 0.0, -0.2, 1.0, 0.75, 1.0, 0.0, 0.01]
_SHOCK_R = [0.125, -0.3, 0.4, 0.0, 0.1, 0.75, -1.0, 0.3, -0.02]


class Pack:
    """nblocks blocks of one shape.  Block b has phases of its own, is a shock when b % 3 == 2 (a wave otherwise) and
    sits on level (7 b + seed) % 3: dx = DX0 * 2**-level in the active directions.  prim(b0, b1) rebuilds any range of
    blocks, so that big packs never need the whole host array at once."""

    def __init__(self, fluid, nx, ng, nblocks, seed):
        self.fluid, self.nx, self.ng, self.nblocks = fluid, tuple(nx), ng, nblocks
        self.nh = NHYDRO[fluid]
        rng = np.random.default_rng(seed)
        self.ph = rng.uniform(0.0, 2.0 * np.pi, (nblocks, self.nh, 2))
        self.level = (7 * np.arange(nblocks) + seed) % 3
        self.shape = H.block_shape(nx, ng, self.nh)
        _, nk, nj, ni = self.shape
        k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
        self.arg = 2.0 * np.pi * (i / ni + 0.7 * j / max(nj, 2) + 0.4 * k / max(nk, 2))
        self.ijk = i + j + k
        self._geoms = {}

    def dx(self, b):
        s = 2.0 ** -int(self.level[b])
        return tuple(d * s if n > 1 or q == 0 else d for q, (d, n) in enumerate(zip(DX0, self.nx)))

    def dxs(self):
        return [self.dx(b) for b in range(self.nblocks)]

    def geom(self, b):
        lev = int(self.level[b])
        if lev not in self._geoms:
            self._geoms[lev] = H.geom(self.fluid, self.nx, self.ng, 0, self.dx(b))
        return self._geoms[lev]

    def geoms(self, b0=0, b1=None):
        return [self.geom(b) for b in range(b0, self.nblocks if b1 is None else b1)]

    def mindx(self):
        return min(min(d for d, n in zip(self.dx(b), self.nx) if n > 1) for b in range(min(self.nblocks, 3)))

    def prim(self, b0=0, b1=None):
        b1 = self.nblocks if b1 is None else b1
        nh = self.nh
        amp = np.array(_AMP[:nh])[None, :, None, None, None]
        base = np.array(_BASE[:nh])[None, :, None, None, None]
        ph = self.ph[b0:b1, :, :, None, None, None]
        w = base + amp * np.sin(self.arg + ph[:, :, 0]) + 0.2 * amp * np.sin(2.0 * self.arg + ph[:, :, 1])
        n = self.ijk.max() + 1
        for q, b in enumerate(range(b0, b1)):
            if b % 3 == 2:
                left = self.ijk < n / 2.2 + (self.ph[b, 0, 0] - np.pi) * 0.1 * n
                for v in range(nh):
                    w[q, v] = np.where(left, _SHOCK_L[v], _SHOCK_R[v]) + 0.05 * amp[0, v, 0, 0, 0] * np.sin(self.arg + ph[q, v, 0])
        return w

    def cons(self, b0=0, b1=None):
        return H.prim_to_cons(self.fluid, self.prim(b0, b1), GAMMA)


def _mesh(ctx, pack, cons=None, prim=None, with_flux=False, fill_prim=None):
    """a MeshData of the pack, the blocks' states uploaded one at a time (cons / prim: 'pack' or None)"""
    import torch
    from athenapk_amd import hydro
    m = hydro.MeshData(ctx, pack.nx, pack.ng, pack.nh, dx=pack.dxs(), nblocks=pack.nblocks, with_flux=with_flux)
    step = max(1, (64 << 20) // (8 * int(np.prod(pack.shape))))
    for b0 in range(0, pack.nblocks, step):
        b1 = min(pack.nblocks, b0 + step)
        w = pack.prim(b0, b1)
        if cons == "pack":
            m.cons[b0:b1].copy_(torch.from_numpy(H.prim_to_cons(pack.fluid, w, GAMMA)))
        if prim == "pack":
            m.prim[b0:b1].copy_(torch.from_numpy(w))
    if fill_prim is not None:
        m.prim.fill_(fill_prim)
    return m


def _host(t):
    return t.cpu().numpy()


def _launches(ctx):
    """apk_kernel_timing_* counts per slot since the last read (a read resets)"""
    from athenapk_amd import hydro
    out = {}
    for q, name in enumerate(hydro.L.TIMING_SLOTS):
        ms, cnt = C.c_double(0.0), C.c_longlong(0)
        assert ctx.lib.apk_kernel_timing_read(ctx.h, q, C.byref(ms), C.byref(cnt)) == 0
        out[name] = cnt.value
    return out


# ---- launch choices, restated from csrc/fused_kernel.hpp, fused3_kernel.hpp, fused2_kernel.hpp -------------------------
def march_rows_per_wave(nx1, ntrans):
    rpw = 4 if nx1 <= 16 else (2 if nx1 <= 32 else 1)
    while rpw > 1 and rpw > ntrans:
        rpw //= 2
    return rpw


def march_segments(waves, n_along):
    nseg = (4096 + waves - 1) // waves
    return max(1, min(nseg, max(n_along // 8, 1)))


def x3_sweep_segments(nx):
    """segments of the two-kernel stage's x3 sweep (launch_two_kernel)"""
    rpw = march_rows_per_wave(nx[0], nx[1])
    waves = -(-nx[0] // (64 // rpw)) * -(-nx[1] // rpw)
    return rpw, lambda nb: march_segments(waves * nb, nx[2])


def dc_kseg(nx, nblocks):
    """the donor-cell predictor's segment length (launch_dc_march, two-row march if nx2 even)"""
    two_rows = nx[1] % 2 == 0 and nx[1] >= 4
    wpb = ((nx[1] // 2) * (nx[0] + 2) + 61) // 62 if two_rows else (nx[1] * (nx[0] + 2) + 61) // 62
    kseg = 16 if nx[2] >= 32 else (8 if nx[2] >= 16 else nx[2])
    if nx[2] >= 16 and wpb * ((nx[2] + 7) // 8) * nblocks < 4 * 2048:
        best = 1e300
        for cand in (4, 6, 8, 16):
            if cand > nx[2]:
                continue
            waves = wpb * (-(-nx[2] // cand)) * nblocks
            per_simd = 2.0 / 1.4 if waves <= 1024 else float((waves + 1023) // 1024)
            if per_simd * (cand + 1.5) < best:
                best, kseg = per_simd * (cand + 1.5), cand
    return kseg, two_rows


def _two_kernel(nx, nb):
    rpw, seg = x3_sweep_segments(nx)
    return "two_kernel", "rpw%d_seg%d" % (rpw, seg(nb))


def _dc(nx, nb):
    kseg, two = dc_kseg(nx, nb)
    return "dc_from_cons", "kseg%d_%s" % (kseg, "two_rows" if two else "one_row")


def _s3(nx, nb):
    if nx[0] >= 32 and nx[1] % 2 == 0:   # single_march_stage_applies (stage_form.hpp)
        kseg = min(15, nx[2])
        return "single_march", "kseg%d_nseg%d" % (kseg, -(-nx[2] // kseg))
    return "two_kernel_rk", "nx1_below_32_takes_two_kernel"


# (form, fluid, recon, riemann, block shape, nblocks); the id names the regime the formulas above give
_TABLE = [
    (_two_kernel, "glmmhd", "ppm", "hlld", (128, 128, 128), 1),
    (_two_kernel, "glmmhd", "ppm", "hlld", (128, 128, 128), 4),
    (_two_kernel, "glmmhd", "ppm", "hlld", (128, 128, 128), 8),      # the bench pack
    (_two_kernel, "glmmhd", "ppm", "hlld", (16, 16, 16), 64),
    (_two_kernel, "glmmhd", "ppm", "hlld", (16, 16, 16), 232),       # config 5's refined mesh
    (_two_kernel, "glmmhd", "ppm", "hlld", (16, 16, 16), 1024),
    (_two_kernel, "glmmhd", "ppm", "hlld", (32, 32, 32), 64),
    (_two_kernel, "glmmhd", "ppm", "hlld", (128, 128, 4), 16),       # config 3
    (_two_kernel, "glmmhd", "ppm", "hlld", (24, 24, 24), 232),       # nx1 % 16 != 0: du_pitch 32
    (_dc, "glmmhd", "dc", "hlld", (16, 16, 16), 64),
    (_dc, "glmmhd", "dc", "hlld", (16, 16, 16), 100),
    (_dc, "glmmhd", "dc", "hlld", (16, 16, 16), 300),
    (_dc, "glmmhd", "dc", "hlld", (128, 128, 128), 8),               # no cost model: kseg 16
    (_dc, "glmmhd", "dc", "hlld", (16, 15, 16), 232),                # odd nx2: the one-row march
    (_dc, "glmmhd", "dc", "hlld", (128, 128, 4), 16),                # nx3 < 16: the whole column
    (_dc, "glmmhd", "dc", "hlld", (24, 24, 24), 232),
    (_s3, "euler", "plm", "hllc", (128, 128, 128), 8),
    (_s3, "euler", "plm", "hllc", (16, 16, 16), 232),
    (_s3, "euler", "plm", "hllc", (32, 32, 32), 232),
]
REGIMES = []
for _f, _fl, _rc, _rs, _nx, _nb in _TABLE:
    _form, _what = _f(_nx, _nb)
    REGIMES.append(pytest.param(_form, _fl, _rc, _rs, _nx, _nb,
                                id="%s_%s_%s_%dx%s_%s" % (_form, _rc, _rs, _nb, "x".join(map(str, _nx)), _what)))


def _ng(recon):
    return NGHOST[recon] if recon != "dc" else 2


def _par(fn, n, block_bytes):
    """fn(b) for b < n on oracle threads; a thread holds about ten arrays of one block"""
    workers = max(1, min(THREADS, n, int(HOST_BUDGET // (10 * block_bytes))))
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(fn, range(n)))


@pytest.mark.parametrize("form,fluid,recon,riemann,nx,nblocks", REGIMES)
def test_stage_at_production_pack_sizes(request, form, fluid, recon, riemann, nx, nblocks):
    """One stage in the plain StageFused form of its place in a cycle (the driver's stage arguments without the face table
    and the x1 strips in exchange buffers, which select other instantiations), on both builds, against orc_stage
    (+ orc_c2p, and the reduced dt where the stage estimates it):
      two_kernel     the VL2 corrector (gam0 = 0): FillDerived out of place and the dt estimate;
      dc_from_cons   the VL2 predictor: lean, input from u1's conserved state (prim_from_cons = 1; u0.cons holds something
                     else), FillDerived out of place, no dt;
      single_march / two_kernel_rk
                     the second RK2 stage: input from u0's conserved state (prim_from_cons = 2), result in a third buffer,
                     primitives for the dt estimate only (fill_derived = 3).
    The timing slots must show the kernel family the form takes."""
    import torch
    from athenapk_amd import hydro
    ng = _ng(recon)
    ded = 1 if fluid == "glmmhd" else 0
    pack = Pack(fluid, nx, ng, nblocks, seed=nblocks + nx[0])
    geo = pack.geoms()
    mindx = pack.mindx()
    bdt = 0.2 * mindx
    eos = hydro.L.make_eos(GAMMA)
    rk = form in ("single_march", "two_kernel_rk")
    gam0 = 0.5 if rk else 0.0
    runs = {}
    for strict in (True, False):
        ctx = request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")
        if form == "two_kernel":
            m0 = _mesh(ctx, pack, cons="pack", prim="pack")
            m1 = _mesh(ctx, pack, cons="pack", fill_prim=-7.0)
            out, kw = m0, dict(fill_derived=2, estimate_dt=True)
        elif form == "dc_from_cons":
            m0 = _mesh(ctx, pack, fill_prim=float("nan"))
            m0.cons.fill_(123.0)                  # (gam0 = 0: u0's old state is no input; u1.cons is)
            m1 = _mesh(ctx, pack, cons="pack", fill_prim=-7.0)
            out, kw = m0, dict(fill_derived=2, prim_from_cons=True)
        else:
            m0 = _mesh(ctx, pack, cons="pack", fill_prim=float("nan"))
            m1 = _mesh(ctx, pack, cons="pack", fill_prim=-7.0)
            m1.cons.mul_(1.01)
            out = _mesh(ctx, pack, fill_prim=-7.0)
            kw = dict(fill_derived=3, estimate_dt=True, prim_from_cons=2, cons_out=out)
        ctx.poll_flags()
        ctx.lib.apk_kernel_timing_enable(ctx.h, 1)
        _launches(ctx)
        hydro.StageFused(m0, m1, fluid, recon, riemann, eos, C_H, gam0, 1.0 - gam0, bdt, dedner=ded, glmmhd_alpha=0.1,
                         mindx=mindx, **kw)
        dt = hydro.StageDt(ctx, CFL) if kw.get("estimate_dt") else None
        torch.cuda.synchronize()
        n = _launches(ctx)
        ctx.lib.apk_kernel_timing_enable(ctx.h, 0)
        assert ctx.poll_flags() == 0
        runs[strict] = (out, m1, dt, n)
    # the family that ran (fused_kernel.hpp: two-kernel stage = x3 sweep in slot fused_x3 + finishing march in fused_x1;
    # single march = fused_x1 alone; donor-cell stage = fused_dc_x1 alone; nothing in the three-sweep slot fused_x2)
    want_n = {"two_kernel": dict(fused_x1=1, fused_x3=1), "two_kernel_rk": dict(fused_x1=1, fused_x3=1),
              "single_march": dict(fused_x1=1), "dc_from_cons": dict(fused_dc_x1=1)}[form]
    for strict in (True, False):
        n = runs[strict][3]
        got = {k: v for k, v in n.items() if k.startswith("fused") and v}
        assert got == want_n, "kernel family: %s, expected %s" % (got, want_n)

    def block(b):
        cons = pack.cons(b, b + 1)
        g = geo[b]
        if form == "two_kernel":
            want = H.orc_stage(fluid, recon, riemann, g, cons, cons, pack.prim(b, b + 1), GAMMA, C_H, 0.0, 1.0, bdt,
                               dedner=ded, alpha=0.1, mindx=mindx)
        else:
            _, prim_in, bad = H.orc_c2p(fluid, g, cons.copy(), H.O.make_eos(GAMMA))
            assert bad == 0
            u1 = cons * 1.01 if rk else cons
            want = H.orc_stage(fluid, recon, riemann, g, cons, u1, prim_in, GAMMA, C_H, gam0, 1.0 - gam0, bdt,
                               dedner=ded, alpha=0.1, mindx=mindx)
        want, want_prim, bad = H.orc_c2p(fluid, g, want, H.O.make_eos(GAMMA))
        assert bad == 0
        dtb = H.orc_min_dt(fluid, g, want_prim, GAMMA)
        for strict in (True, False):
            out, m1, _, _ = runs[strict]
            what = "%s block %d" % ("strict" if strict else "fma", b)
            _cmp(H.interior(_host(out.cons[b:b + 1]), nx, ng), H.interior(want, nx, ng), strict, what + " cons")
            if form != "single_march" and form != "two_kernel_rk":
                _cmp(H.interior(_host(m1.prim[b:b + 1]), nx, ng), H.interior(want_prim, nx, ng), strict, what + " u1.prim")
        return dtb

    dts = _par(block, nblocks, 8 * int(np.prod(pack.shape)))
    if runs[True][2] is not None:
        want_dt = CFL * min(dts)
        assert runs[True][2] == want_dt
        assert runs[False][2] == pytest.approx(want_dt, rel=1e-12)


# ---- past 65535 planes ----------------------------------------------------------------------------------------------
# (block shape, nblocks, nghost): grid y / z of nx3 * nblocks (3-D) or nblocks (1-D, 2-D) above 65535
BIG = {"1d": ((8, 1, 1), 66000, 3), "2d": ((8, 4, 1), 66000, 3), "3d": ((8, 4, 4), 16385, 2)}


def _grid_limits():
    """hipDeviceAttributeMaxGridDim{X,Y,Z} of device 0, from the HIP runtime torch has loaded"""
    import torch
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    out = []
    for attr in (29, 30, 31):  # hipDeviceAttributeMaxGridDimX / Y / Z (hip_runtime_api.h)
        v = C.c_int(0)
        assert hip.hipDeviceGetAttribute(C.byref(v), attr, 0) == 0
        out.append(v.value)
    return out


def _big(dim, fluid, seed):
    nx, nb, ng = BIG[dim]
    return Pack(fluid, nx, ng, nb, seed)


def test_device_grid_limits_are_recorded():
    """The device reports its grid limits; the packs below reach past 65535 in grid y and z (these launches pass the
    count unsplit).  Printed for the record: run with -s to see them.  An MI355X under ROCm 7.0 reports
    hipDeviceAttributeMaxGridDimX / Y / Z = 2147483647 / 65536 / 65536, and the launches of 65540 and 66000 in y or z
    below still cover every block (the tests of this section pass without a chunked launch)."""
    lim = _grid_limits()
    print("hipDeviceAttributeMaxGridDim X/Y/Z:", lim)
    assert all(v > 0 for v in lim)
    for nx, nb, _ in BIG.values():
        assert (nx[2] * nb if nx[2] > 1 else nb) > 65535


_FLUX_CASES = [("1d", "euler", "dc", "hllc"), ("1d", "euler", "plm", "hllc"), ("1d", "glmmhd", "ppm", "hlld"),
               ("2d", "euler", "dc", "hllc"), ("2d", "euler", "plm", "hlle"), ("2d", "euler", "ppm", "hllc"),
               ("3d", "euler", "dc", "hllc"), ("3d", "euler", "plm", "hllc")]


@pytest.mark.parametrize("dim,fluid,recon,riemann", _FLUX_CASES, ids=["-".join(c) for c in _FLUX_CASES])
def test_fluxes_and_update_past_65535_planes(request, dim, fluid, recon, riemann):
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    pack = _big(dim, fluid, seed=3)
    nx, ng = pack.nx, pack.ng
    geo = pack.geoms()
    prim, cons = pack.prim(), None
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    m0 = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=pack.nblocks, cons=cons, prim=prim)
    m1 = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=pack.nblocks, cons=cons * 1.01, with_flux=False)
    hydro.CalculateFluxes(m0, fluid, recon, riemann, hydro.L.make_eos(GAMMA), C_H)
    fl = H.orc_fluxes(fluid, recon, riemann, geo, prim, GAMMA, C_H)
    for d in range(m0.ndim):
        _cmp(m0.flux_host(d), fl[d], True, "flux%d" % (d + 1))
    hydro.UpdateWithFluxDivergence(m0, m1, 0.25, 0.75, 0.0123)
    want = H.orc_update(geo, cons, cons * 1.01, fl, 0.25, 0.75, 0.0123)
    _cmp(m0.cons_host(), want, True, "update")


@pytest.mark.parametrize("dim", ["1d", "2d", "3d"])
def test_dedner_source_past_65535_planes(request, dim):
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    pack = _big(dim, "glmmhd", seed=4)
    prim = pack.prim()
    cons = H.prim_to_cons("glmmhd", prim, GAMMA)
    md = hydro.MeshData(ctx, pack.nx, pack.ng, 9, dx=pack.dxs(), nblocks=pack.nblocks, cons=cons, prim=prim, with_flux=False)
    hydro.DednerSource(md, False, 0.1, C_H, pack.mindx(), 0.011)
    _cmp(md.cons_host(), H.orc_dedner(pack.geoms(), cons, prim, False, 0.1, C_H, pack.mindx(), 0.011), True, "dedner")


@pytest.mark.parametrize("dim", ["1d", "2d", "3d"])
def test_cons_to_prim_and_timestep_past_65535_planes(request, dim):
    """ConsToPrim of whole blocks, boxed with the dt estimate (ghost_depth = 1), of the faces; EstimateTimestep with the
    pack's minimum in its LAST block."""
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    fluid = "euler"
    pack = _big(dim, fluid, seed=5)
    nx, ng, nb = pack.nx, pack.ng, pack.nblocks
    geo = pack.geoms()
    prim = pack.prim()
    prim[-1, 1] += 3.0                                 # the fastest cells of the pack: in its last block
    pack.level[-1] = 2
    geo[-1] = pack.geom(nb - 1)
    dxs = pack.dxs()
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    eos = hydro.L.make_eos(GAMMA)
    _, want_prim, bad = H.orc_c2p(fluid, geo, cons, H.O.make_eos(GAMMA))
    assert bad == 0
    per_block = [H.orc_min_dt(fluid, geo[b], want_prim[b:b + 1], GAMMA) for b in (nb - 2, nb - 1)]
    want_dt = CFL * H.orc_min_dt(fluid, geo, want_prim, GAMMA)
    assert want_dt == CFL * per_block[1] < CFL * per_block[0], "the minimum must lie in the last block"
    md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=dxs, nblocks=nb, cons=cons, with_flux=False)
    hydro.ConservedToPrimitive(md, fluid, eos)
    _cmp(md.prim_host(), want_prim, True, "prim (whole blocks)")
    assert hydro.EstimateTimestep(md, fluid, eos, CFL) == want_dt
    md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=dxs, nblocks=nb, cons=cons, with_flux=False)
    assert hydro.ConservedToPrimitiveDt(md, fluid, eos, CFL) == want_dt
    _cmp(md.prim_host(), want_prim, True, "prim (whole blocks, with dt)")
    # boxed: the cells at most one layer outside the interior
    act = [True, nx[1] > 1, nx[2] > 1]
    grids = np.meshgrid(*[np.arange(n + 2 * ng if a else 1) for n, a in zip(nx[::-1], act[::-1])], indexing="ij")
    K, J, I = grids
    deep = np.zeros(cons.shape[2:], dtype=bool)
    nghost = np.zeros(cons.shape[2:], dtype=int)
    for c, n, a in ((I, nx[0], True), (J, nx[1], act[1]), (K, nx[2], act[2])):
        if a:
            deep |= (c < ng - 1) | (c > ng + n)
            nghost += (c < ng) | (c >= ng + n)
    md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=dxs, nblocks=nb, cons=cons, prim=np.full_like(cons, -3.0), with_flux=False)
    assert hydro.ConservedToPrimitiveDt(md, fluid, eos, CFL, ghost_depth=1) == want_dt
    got = md.prim_host()
    assert np.array_equal(got[:, :, ~deep], want_prim[:, :, ~deep]) and np.all(got[:, :, deep] == -3.0)
    # faces: the interior and the ghost cells straight behind a face
    face = nghost <= 1
    for with_dt in (False, True):
        md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=dxs, nblocks=nb, cons=cons, prim=np.full_like(cons, -3.0), with_flux=False)
        if with_dt:
            assert hydro.ConservedToPrimitiveFacesDt(md, fluid, eos, CFL) == want_dt
        else:
            hydro.ConservedToPrimitiveFaces(md, fluid, eos)
        got = md.prim_host()
        assert np.array_equal(got[:, :, face], want_prim[:, :, face]) and np.all(got[:, :, ~face] == -3.0)


@pytest.mark.parametrize("dim", ["1d", "2d", "3d"])
def test_fused_stage_past_65535_planes(request, dim):
    """StageFused in the form the block shape selects: 1-D the x1 kernel (g1.y = nblocks), 2-D x1 kernel + x2 march
    (grid z = nblocks), 3-D 8 x 4 x 4 PLM the three-sweep stage (nx1 < 16: no two-kernel form); with FillDerived and dt in
    2-D and 3-D."""
    import torch
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    # (GLM-MHD where the pack is small enough for the host's copies of it)
    fluid, recon, riemann = {"1d": ("glmmhd", "ppm", "hlld"), "2d": ("euler", "ppm", "hllc"), "3d": ("euler", "plm", "hllc")}[dim]
    nh, ded = NHYDRO[fluid], (1 if fluid == "glmmhd" else 0)
    pack = _big(dim, fluid, seed=6)
    nx, ng, nb = pack.nx, pack.ng, pack.nblocks
    geo = pack.geoms()
    prim = pack.prim()
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    fill = dim != "1d"
    m0 = hydro.MeshData(ctx, nx, ng, nh, dx=pack.dxs(), nblocks=nb, cons=cons, prim=prim, with_flux=False)
    m1 = hydro.MeshData(ctx, nx, ng, nh, dx=pack.dxs(), nblocks=nb, cons=cons, prim=np.full_like(prim, -7.0), with_flux=False)
    ctx.poll_flags()
    ctx.lib.apk_kernel_timing_enable(ctx.h, 1)
    _launches(ctx)
    bdt = 0.2 * pack.mindx()
    hydro.StageFused(m0, m1, fluid, recon, riemann, hydro.L.make_eos(GAMMA), C_H, 0.0, 1.0, bdt, dedner=ded, glmmhd_alpha=0.1,
                     mindx=pack.mindx(), fill_derived=2 if fill else 0, estimate_dt=fill)
    dt = hydro.StageDt(ctx, CFL) if fill else None
    torch.cuda.synchronize()
    n = _launches(ctx)
    ctx.lib.apk_kernel_timing_enable(ctx.h, 0)
    assert ctx.poll_flags() == 0
    want_n = {"1d": dict(fused_x1=1), "2d": dict(fused_x1=1, fused_x2=1), "3d": dict(fused_x1=1, fused_x2=1, fused_x3=1)}[dim]
    assert {k: v for k, v in n.items() if k.startswith("fused") and v} == want_n
    want = H.orc_stage(fluid, recon, riemann, geo, cons, cons, prim, GAMMA, C_H, 0.0, 1.0, bdt, dedner=ded, alpha=0.1,
                       mindx=pack.mindx())
    _cmp(H.interior(m0.cons_host(), nx, ng), H.interior(want, nx, ng), True, "cons")
    if fill:
        _, want_prim, bad = H.orc_c2p(fluid, geo, want, H.O.make_eos(GAMMA))
        assert bad == 0
        _cmp(H.interior(m1.prim_host(), nx, ng), H.interior(want_prim, nx, ng), True, "u1.prim")
        assert dt == CFL * H.orc_min_dt(fluid, geo, want_prim, GAMMA)


@pytest.mark.parametrize("dim", ["1d", "2d", "3d"])
def test_flux_correction_and_unphysical_count_past_65535_planes(request, dim):
    """FirstOrderFluxCorrect and CountUnphysical with the cells that need them in the LAST blocks of the pack only."""
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    fluid = "euler"
    pack = _big(dim, fluid, seed=7)
    nx, ng, nb = pack.nx, pack.ng, pack.nblocks
    geo = pack.geoms()
    prim = pack.prim()
    prim[-3:, 4] *= 1e-4                                # cold and fast: the step drives their trial pressures negative
    prim[-3:, 1:4] *= 10.0
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    fl = H.orc_fluxes(fluid, "plm", "hlle", geo, prim, GAMMA, C_H)
    beta_dt = 0.2 * pack.mindx()
    want_fl, want_n = H.orc_fofc(fluid, geo, cons, prim, cons, fl, GAMMA, C_H, 0.0, 1.0, beta_dt)
    _, n_head = H.orc_fofc(fluid, geo[:-3], cons[:-3], prim[:-3], cons[:-3], [f[:-3] for f in fl], GAMMA, C_H, 0.0, 1.0, beta_dt)
    _, n_last = H.orc_fofc(fluid, geo[-1:], cons[-1:], prim[-1:], cons[-1:], [f[-1:] for f in fl], GAMMA, C_H, 0.0, 1.0, beta_dt)
    assert n_head == 0 and n_last > 0, "the corrections must fall in the last blocks"
    m0 = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=nb, cons=cons, prim=prim)
    for d in range(m0.ndim):
        m0.flux[d].copy_(hydro.torch.from_numpy(fl[d]))
    m1 = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=nb, cons=cons, with_flux=False)
    assert hydro.FirstOrderFluxCorrect(m0, m1, fluid, hydro.L.make_eos(GAMMA), C_H, 0.0, 1.0, beta_dt) == want_n
    for d in range(m0.ndim):
        _cmp(m0.flux_host(d), want_fl[d], True, "corrected flux%d" % (d + 1))
    # CountUnphysical: negative densities in interior cells of the last two blocks
    bad = cons.copy()
    ii = H.interior(bad, nx, ng)
    ii[-1, 0, 0, 0, -1] = -1.0
    ii[-1, 0, -1, -1, 0] = -2.0
    ii[-2, 0, -1, 0, 1] = -0.5
    md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=nb, cons=bad, with_flux=False)
    assert hydro.CountUnphysical(md, fluid) == 3


@pytest.mark.parametrize("dim", ["1d", "2d", "3d"])
def test_history_and_tags_past_65535_planes(request, oracle, dim):
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    fluid = "euler"
    pack = _big(dim, fluid, seed=8)
    nx, ng, nb = pack.nx, pack.ng, pack.nblocks
    geo = pack.geoms()
    prim = pack.prim()
    cons = H.prim_to_cons(fluid, prim, GAMMA)
    md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=nb, cons=cons, prim=prim, with_flux=False)
    np.testing.assert_allclose(hydro.HydroHst(md, fluid), H.orc_history(fluid, geo, cons), rtol=1e-13, atol=1e-15)
    vals_o = [oracle.tag("pressure_gradient", geo[b], np.ascontiguousarray(prim[b]), 1e300)[1] for b in range(nb)]
    p0 = float(np.median(vals_o))
    want = [oracle.tag("pressure_gradient", geo[b], np.ascontiguousarray(prim[b]), p0) for b in range(nb)]
    tags, vals = hydro.TagBlocks(md, "pressure_gradient", p0)
    assert list(vals) == [w[1] for w in want]
    assert list(tags) == [w[0] for w in want]
    assert len(set(tags)) > 1 or dim == "1d"          # (the gradient criteria are 0 on 1-D blocks)
    # the criterion and the time step from the conserved state (3-D packs only: apk_tag_blocks_dt_from_cons)
    if dim == "3d":
        md = hydro.MeshData(ctx, nx, ng, pack.nh, dx=pack.dxs(), nblocks=nb, cons=cons, prim=np.full_like(cons, np.nan),
                            with_flux=False)
        t, v, dt = hydro.TagBlocksDtFromCons(md, fluid, hydro.L.make_eos(GAMMA), CFL, p0)
        _, want_prim, _ = H.orc_c2p(fluid, geo, cons, H.O.make_eos(GAMMA))
        want_v = [oracle.tag("pressure_gradient", geo[b], np.ascontiguousarray(want_prim[b]), p0) for b in range(nb)]
        assert list(v) == [w[1] for w in want_v] and list(t) == [w[0] for w in want_v]
        assert dt == CFL * H.orc_min_dt(fluid, geo, want_prim, GAMMA)


def test_turbulence_apply_past_65535_planes(request, oracle):
    """turbulence::Perturb on 16385 blocks of 8 x 4 x 4 (igrid z = 65540), blocks at scattered places of a 64^3 box.
    (One dx for all blocks: the forcing lives on the uniform box, and orc_turb_perturb takes one geometry.)"""
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict")
    nx, nb, ng = BIG["3d"]
    n = 64
    kv = np.array([[1, 0, 0, 1, 2, 0, -1, 2], [0, 1, 0, 1, -1, 2, 1, 2], [0, 0, 1, -1, 0, 1, 2, 2]], dtype=np.float64)
    f = oracle.Fmft(oracle.load(), kv, k_peak=2.0, sol_weight=0.7, t_corr=0.5, rseed=7)
    f.evolve(0.1)
    rng = np.random.default_rng(9)
    pos = np.stack([rng.integers(0, n // nx[d], nb) * nx[d] for d in range(3)], axis=1)
    cache = {}

    def ph(d, o):
        if (d, o) not in cache:
            cache[(d, o)] = f.phases(d, nx[d], int(o), n)
        return cache[(d, o)]
    phases = [(ph(0, p[0]), ph(1, p[1]), ph(2, p[2])) for p in pos]
    g = H.geom("glmmhd", nx, ng, 0, (1.0 / n,) * 3)
    pack = Pack("glmmhd", nx, ng, nb, seed=10)
    prim = pack.prim()
    cons = H.prim_to_cons("glmmhd", prim, GAMMA)
    md = hydro.MeshData(ctx, nx, ng, 9, dx=tuple(g.dx), nblocks=nb, cons=cons, prim=prim, with_flux=False, row_pitch="natural")
    drv = hydro.FewModesFT(md, [[p.transpose(2, 1, 0) for p in blk] for blk in phases])
    drv.Inverse(f.var_hat())
    acc0 = drv.acc_host()
    want_acc0 = np.stack([f.inverse(g, *phases[b]) for b in range(nb)])
    _cmp(acc0, want_acc0, True, "acc")
    drv.Perturb(0.01, 0.5, 1.0)
    want_u, want_a = H.orc_turb_perturb(g, cons, acc0, 0.01, 0.5, 1.0)
    np.testing.assert_allclose(drv.acc_host(), want_a, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(md.cons_host(), want_u, rtol=1e-12, atol=1e-14)


# ---- one production cycle against the oracle's mini-driver --------------------------------------------------------------
# (oracle.Sim at 256^3 in 128^3 meshblocks, 16 threads, measured: GLM-MHD PPM+HLLD VL2 6.7 s per cycle, 9.2 GB peak RSS;
# hydro PLM+HLLC RK2 2.2 s, 5.0 GB.  The oracle runs first and is freed before the two GPU runs.)
_CYCLES = {
    "mhd_ppm_hlld_vl2_256": ("synthetic_mhd", dict(fluid="glmmhd", recon="ppm", riemann="hlld", integrator="vl2", ng=3,
                                                   xmin=(0.0, 0.0, 0.0), xmax=(1.0, 1.0, 1.0), gamma=1.666666666666667),
                             "synthetic"),
    "hydro_plm_hllc_rk2_256": ("sod", dict(fluid="euler", recon="plm", riemann="hllc", integrator="rk2", ng=2,
                                           bc=("outflow", "periodic", "periodic"), xmin=(0.0, -0.5, -0.5),
                                           xmax=(1.0, 0.5, 0.5), gamma=1.4), "sod"),
}


@pytest.mark.parametrize("workload", list(_CYCLES))
def test_one_bench_cycle_at_256_cubed_matches_the_oracle(oracle, workload):
    """One cycle of the bench's own workloads (bench.py WORKLOADS: the decks as they are, 256^3 in 128^3 meshblocks) on
    the driver -- the VL2 predictor / corrector of the headline, the single-march RK2 stages of the Sod tube -- and on
    oracle.Sim with the same scheme: the parity build bit for bit with the same dt and c_h, the product build within the
    1e-12 rule of test_synthetic_mhd_256_cubed_conserves_and_matches_flux_array_path."""
    from athenapk_amd import decks, driver
    deck, kw, pgen = _CYCLES[workload]
    o = oracle.Sim(nx=(256, 256, 256), mb=(128, 128, 128), cfl=0.3, nthreads=16, **kw).pgen(pgen)
    o.step()
    want, want_dt, want_ch = o.gather_cons(), o.dt, o.c_h
    del o
    for strict in (True, False):
        s = driver.Simulation(decks.load(deck), [], strict=strict).initialize()
        assert s.info.zones_total == 256 ** 3 and s.info.nblocks_local == 8
        s.step()
        got, dt, ch = s.gather(), s.dt, s.c_h
        s.close()
        if strict:
            assert dt == want_dt and ch == want_ch
            assert np.array_equal(got, want), "max abs diff %.3e" % np.max(np.abs(got - want))
        else:
            assert dt == pytest.approx(want_dt, rel=1e-12) and ch == pytest.approx(want_ch, rel=1e-12)
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
