"""Mesh-refinement operators and tagging (SURVEY 8(f) rank 3 building blocks).
CPU: properties of the oracle restatement (the reference holds no vectors for these operators:
parity is unpinned and the properties below are what the upstream operators guarantee).
GPU: the HIP plan kernels against the oracle, bit for bit in the strict build."""
import ctypes as C

import numpy as np
import pytest

import helpers as H


def _fields(r, nvar, seed, kind="smooth"):
    from oracle import oracle as O
    fs, cs = r.dims()
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(cs[0]), np.arange(cs[1]), np.arange(cs[2]), indexing="ij")
    coarse = np.empty((nvar,) + cs)
    for v in range(nvar):
        if kind == "smooth":
            coarse[v] = 1.5 + np.sin(0.7 * i + 0.3 * v) * np.cos(0.5 * j) + 0.3 * np.sin(0.9 * k + v)
        else:
            coarse[v] = rng.uniform(-1.0, 1.0, cs)
    fine = rng.uniform(-1.0, 1.0, (nvar,) + fs)
    return coarse, fine


def _interior_box(r):
    lo = [r.cng if (d == 0 or r.nx[d] > 1) else 0 for d in range(3)]
    hi = [r.cng + r.nx[d] // 2 - 1 if (d == 0 or r.nx[d] > 1) else 0 for d in range(3)]
    return lo, hi


GEOMS = [((16, 16, 16), 2, 2), ((16, 8, 1), 2, 2), ((12, 1, 1), 3, 3), ((8, 8, 8), 3, 3)]


@pytest.mark.parametrize("nx,ng,cng", GEOMS)
def test_prolongation_is_conservative_and_bounded(oracle, nx, ng, cng):
    r = oracle.make_refine_geom(nx, ng, cng, xmin=(0.25, -0.5, 1.0), dx=(0.01, 0.02, 0.04))
    for kind in ("smooth", "rough"):
        coarse, fine = _fields(r, 3, 1, kind)
        lo, hi = _interior_box(r)
        oracle.prolongate(r, coarse, fine, lo, hi)
        ndim = oracle.load().orc_refine_ndim(C.byref(r))
        sl_f = tuple(slice(r.ng, r.ng + nx[d]) if (d == 0 or nx[d] > 1) else slice(0, 1) for d in (2, 1, 0))
        fi = fine[(slice(None),) + sl_f]
        # mean of the 2^d children = parent (offsets are symmetric on a uniform grid)
        shp = (3,) + tuple(x for d in (2, 1, 0) for x in ((nx[d] // 2, 2) if (d == 0 or nx[d] > 1) else (1, 1)))
        child_mean = fi.reshape(shp).mean(axis=(2, 4, 6))
        sl_c = tuple(slice(lo[d], hi[d] + 1) for d in (2, 1, 0))
        parent = coarse[(slice(None),) + sl_c]
        assert np.abs(child_mean - parent).max() < 1e-13
        # no new extrema: children stay within the min/max of the 3^d coarse neighbourhood
        from scipy.ndimage import maximum_filter, minimum_filter
        size = (1,) + tuple(3 if (d == 0 or nx[d] > 1) else 1 for d in (2, 1, 0))
        cmax = maximum_filter(coarse, size=size, mode="nearest")[(slice(None),) + sl_c]
        cmin = minimum_filter(coarse, size=size, mode="nearest")[(slice(None),) + sl_c]
        rep = [2 if (d == 0 or nx[d] > 1) else 1 for d in (2, 1, 0)]
        up = lambda a: a.repeat(rep[0], 1).repeat(rep[1], 2).repeat(rep[2], 3)  # noqa: E731
        assert np.all(fi <= up(cmax) + 1e-14) and np.all(fi >= up(cmin) - 1e-14)
        assert ndim == sum(1 for d in range(3) if d == 0 or nx[d] > 1)


def test_prolongation_reproduces_linear_data_and_restriction_inverts_it(oracle):
    r = oracle.make_refine_geom((16, 16, 16), 2, 2, xmin=(0.0, 0.0, 0.0), dx=(0.5, 0.5, 0.5))
    fs, cs = r.dims()
    k, j, i = np.meshgrid(np.arange(cs[0]), np.arange(cs[1]), np.arange(cs[2]), indexing="ij")
    xc = lambda idx: (idx - r.cng + 0.5) * 1.0  # noqa: E731  coarse centres (cdx = 1)
    coarse = (2.0 + 0.25 * xc(i) - 0.5 * xc(j) + 0.125 * xc(k))[None]
    fine = np.zeros((1,) + fs)
    lo, hi = _interior_box(r)
    oracle.prolongate(r, coarse, fine, lo, hi)
    fk, fj, fi = np.meshgrid(np.arange(fs[0]), np.arange(fs[1]), np.arange(fs[2]), indexing="ij")
    xf = lambda idx: (idx - r.ng + 0.5) * 0.5  # noqa: E731
    want = 2.0 + 0.25 * xf(fi) - 0.5 * xf(fj) + 0.125 * xf(fk)
    s = slice(r.ng, r.ng + 16)
    assert np.abs(fine[0, s, s, s] - want[s, s, s]).max() < 1e-13
    back = np.zeros_like(coarse)
    oracle.restrict(r, 0, fine, back, lo, hi)
    c = slice(r.cng, r.cng + 8)
    assert np.abs(back[0, c, c, c] - coarse[0, c, c, c]).max() < 1e-13


def test_flux_restriction_is_the_area_average(oracle):
    r = oracle.make_refine_geom((8, 8, 8), 2, 2, dx=(0.1, 0.2, 0.4))
    fs, cs = r.dims()
    rng = np.random.default_rng(3)
    for el in (1, 2, 3):
        ax = 3 - el  # numpy axis of the face direction in (k, j, i)
        fshape = tuple(n + (1 if a == ax else 0) for a, n in enumerate(fs))
        cshape = tuple(n + (1 if a == ax else 0) for a, n in enumerate(cs))
        fine = rng.uniform(-1, 1, (2,) + fshape)
        coarse = np.zeros((2,) + cshape)
        lo, hi = _interior_box(r)
        hi[el - 1] += 1  # the upper face of the last coarse cell
        oracle.restrict(r, el, fine, coarse, lo, hi)
        for (k, j, i) in ((2, 3, 4), (5, 5, 2), (2, 2, 2)):
            fk, fj, fi = [(x - r.cng) * 2 + r.ng for x in (k, j, i)]
            sl = [slice(fk, fk + 2), slice(fj, fj + 2), slice(fi, fi + 2)]
            sl[ax] = slice(sl[ax].start, sl[ax].start + 1)
            assert abs(coarse[1, k, j, i] - fine[(1,) + tuple(sl)].mean()) < 1e-15


def test_tagging_criteria(oracle):
    nx, ng = (16, 16, 16), 2
    g = H.geom("euler", nx, ng)
    prim = H.random_prim("euler", nx, ng, seed=4, kind="smooth")[0]
    t, eps = oracle.tag("pressure_gradient", g, prim, 1e9)
    assert t == -1 and eps > 0
    assert oracle.tag("pressure_gradient", g, prim, eps * 0.99)[0] == 1
    assert oracle.tag("pressure_gradient", g, prim, eps * 2.0)[0] == 0      # between thr/4 and thr
    t, vg = oracle.tag("xyvelocity_gradient", g, prim, 1e9)
    assert t == -1 and oracle.tag("xyvelocity_gradient", g, prim, vg * 1.5)[0] == 0
    t, rho = oracle.tag("maxdensity", g, prim, 1e9, 1e-9)
    assert t == 0 and rho == prim[0, ng:-ng, ng:-ng, ng:ng + nx[0] + 1].max()   # i runs to ib.e + 1
    # a constant-pressure block never refines on the pressure criterion
    flat = prim.copy()
    flat[4] = 1.0
    assert oracle.tag("pressure_gradient", g, flat, 1e-3) == (-1, 0.0)
    # 1-D: AmrTag::same
    g1 = H.geom("euler", (16, 1, 1), ng)
    p1 = H.random_prim("euler", (16, 1, 1), ng, seed=4)[0]
    assert oracle.tag("pressure_gradient", g1, p1, 1e-3)[0] == 0


# ---- GPU parity -------------------------------------------------------------------------------------------
def _ctx(request, strict):
    return request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("nx,ng,cng", GEOMS)
def test_refine_plan_matches_oracle(request, oracle, nx, ng, cng, strict):
    """Several blocks x (prolongate interior, prolongate a ghost slab, restrict cells, restrict
    the three face fluxes) in one plan / one launch."""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    dx = (0.01, 0.02, 0.04)
    nvar, nblocks = 3, 3
    dev = torch.device("cuda")
    ops, checks = [], []
    for b in range(nblocks):
        xmin = (0.25 + b * 0.16, -0.5, 1.0 + 0.3 * b)
        r = oracle.make_refine_geom(nx, ng, cng, xmin=xmin, dx=dx)
        ndim = sum(1 for d in range(3) if d == 0 or nx[d] > 1)
        fs, cs = r.dims()
        coarse, fine = _fields(r, nvar, 10 + b, "rough" if b == 1 else "smooth")
        lo, hi = _interior_box(r)
        # ghost slab on the lower x1 side: coarse cells cng-1 (needs cng >= 2 for the stencil)
        glo, ghi = list(lo), list(hi)
        glo[0] = ghi[0] = r.cng - 1
        want_f = fine.copy()
        oracle.prolongate(r, coarse, want_f, lo, hi)
        oracle.prolongate(r, coarse, want_f, glo, ghi)
        cd, fd = torch.from_numpy(coarse).to(dev), torch.from_numpy(fine).to(dev)
        ops += [("prolongate", cd, fd, lo, hi, xmin), ("prolongate", cd, fd, glo, ghi, xmin)]
        checks.append((fd, want_f, "prolongate b%d" % b))
        # restriction of cells into a second coarse buffer
        src = np.random.default_rng(20 + b).uniform(-2, 2, (nvar,) + fs)
        want_c = np.full((nvar,) + cs, 7.0)
        oracle.restrict(r, 0, src, want_c, lo, hi)
        sd, cd2 = torch.from_numpy(src).to(dev), torch.full((nvar,) + cs, 7.0, dtype=torch.float64, device=dev)
        ops.append(("restrict_cell", sd, cd2, lo, hi, xmin))
        checks.append((cd2, want_c, "restrict b%d" % b))
        for el in range(1, ndim + 1):
            ax = 3 - el
            fshape = tuple(n + (1 if a == ax else 0) for a, n in enumerate(fs))
            cshape = tuple(n + (1 if a == ax else 0) for a, n in enumerate(cs))
            fl = np.random.default_rng(30 + b + el).uniform(-2, 2, (nvar,) + fshape)
            want = np.zeros((nvar,) + cshape)
            flo, fhi = list(lo), list(hi)
            fhi[el - 1] += 1
            oracle.restrict(r, el, fl, want, flo, fhi)
            fld, cfd = torch.from_numpy(fl).to(dev), torch.zeros((nvar,) + cshape, dtype=torch.float64, device=dev)
            ops.append(("restrict_face%d" % el, fld, cfd, flo, fhi, xmin))
            checks.append((cfd, want, "flux%d b%d" % (el, b)))
    plan = hydro.RefinePlan(ctx, nx, ng, cng, dx, nvar, ops)
    plan.run()
    torch.cuda.synchronize()
    for t, want, what in checks:
        got = t.cpu().numpy()
        if strict:
            assert np.array_equal(got, want), what
        else:
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), what


@pytest.mark.gpu
def test_refine_plan_rejects_boxes_outside_the_buffer(request):
    import torch
    from athenapk_amd import hydro, lib as L
    ctx = _ctx(request, True)
    t = torch.zeros(3 * 12 * 12 * 12, dtype=torch.float64, device="cuda")
    with pytest.raises(L.ApkError) as e:
        hydro.RefinePlan(ctx, (8, 8, 8), 2, 2, (1, 1, 1), 1, [("prolongate", t, t, (0, 2, 2), (5, 5, 5), (0, 0, 0))])
    assert e.value.code == L.APK_ERR_INVALID
    with pytest.raises(L.ApkError):
        hydro.RefinePlan(ctx, (8, 7, 1), 2, 2, (1, 1, 1), 1, [("restrict_cell", t, t, (2, 2, 0), (5, 5, 0), (0, 0, 0))])


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [(16, 16, 16), (32, 16, 1)])
def test_tag_blocks_matches_oracle(request, oracle, nx):
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    ng, nb = 2, 5
    g = H.geom("glmmhd", nx, ng, 0, (0.1, 0.1, 0.1))
    prim = H.random_prim("glmmhd", nx, ng, seed=8, kind="smooth", nblocks=nb)
    prim[2, 4] = 1.0          # a block with flat pressure
    prim[3, 0] *= 5.0         # a dense block
    md = hydro.MeshData(ctx, nx, ng, 9, dx=tuple(g.dx), nblocks=nb, prim=prim, with_flux=False)
    for crit in ("pressure_gradient", "xyvelocity_gradient", "maxdensity"):
        # thresholds between the blocks' criterion values, so that the pack holds several tags
        vals_o = sorted(oracle.tag(crit, g, prim[b], 1e300, 0.0)[1] for b in range(nb))
        p0 = 0.5 * (vals_o[-1] + vals_o[-2])
        p1 = 0.5 * (vals_o[0] + vals_o[1])
        tags, vals = hydro.TagBlocks(md, crit, p0, p1)
        want = [oracle.tag(crit, g, prim[b], p0, p1) for b in range(nb)]
        assert list(tags) == [w[0] for w in want], crit
        assert list(vals) == [w[1] for w in want], crit       # a max: order independent, bit exact
        assert len(set(tags)) > 1, crit
        # the two halves (launch / read back: the driver reads the time-step estimate in between) give the same
        import ctypes as C
        pending, t2, v2 = C.c_int(0), (C.c_int * nb)(), (C.c_double * nb)()
        code = hydro.L.TAG_CRITERIA[crit]
        assert ctx.lib.apk_tag_blocks_begin(ctx.h, md.h, code, C.byref(pending), hydro._stream()) == 0 and pending.value == 1
        assert ctx.lib.apk_tag_blocks_end(ctx.h, nb, code, pending.value, p0, p1, t2, v2, hydro._stream()) == 0
        assert list(t2) == list(tags) and list(v2) == list(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ng", [((16, 16, 16), 4), ((8, 8, 8), 2), ((32, 16, 1), 2)], ids=["16c", "8c", "2d"])
def test_tag_blocks_through_the_face_table_equals_filled_ghost_zones(request, nx, ng):
    """apk_tag_blocks_begin_skip: a ghost cell straight behind a face whose table entry is >= 0 is read from that
    neighbour's interior -- the values an exchange would have copied there.  Four blocks, some faces joined (a block
    is its own neighbour across a periodic direction too), the zones behind the joined faces poisoned: same criteria
    and tags, bit for bit, as with the zones filled and no table."""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    nb = 4
    g = H.geom("glmmhd", nx, ng, 0, (0.1, 0.1, 0.1))
    prim = H.random_prim("glmmhd", nx, ng, seed=21, kind="smooth", nblocks=nb)
    prim[1, 0] *= 3.0
    tab = np.array([[1, 1, -1, 2, -1, 3], [0, 0, 2, -1, 1, 1], [-1, 3, 0, 2, -1, -1], [2, -1, -1, -1, 0, 3]], dtype=np.int32)
    if nx[2] == 1:
        tab[:, 4:] = -1
    I = [slice(ng, ng + nx[0]), slice(ng, ng + nx[1]), slice(ng, ng + nx[2]) if nx[2] > 1 else slice(None)]
    filled, poisoned = prim.copy(), prim.copy()
    for b in range(nb):
        for f in range(6):
            if tab[b, f] < 0:
                continue
            d, hi = f // 2, f % 2
            dst, src = list(I), list(I)
            dst[d] = slice(ng + nx[d], 2 * ng + nx[d]) if hi else slice(0, ng)
            src[d] = slice(ng, 2 * ng) if hi else slice(nx[d], nx[d] + ng)
            filled[b][:, dst[2], dst[1], dst[0]] = prim[tab[b, f]][:, src[2], src[1], src[0]]
            poisoned[b][:, dst[2], dst[1], dst[0]] = 1e30
    a = hydro.MeshData(ctx, nx, ng, 9, dx=tuple(g.dx), nblocks=nb, prim=filled, with_flux=False)
    b_ = hydro.MeshData(ctx, nx, ng, 9, dx=tuple(g.dx), nblocks=nb, prim=poisoned, with_flux=False)
    dtab = torch.from_numpy(tab).cuda()
    for crit in ("pressure_gradient", "xyvelocity_gradient", "maxdensity"):
        _, vals = hydro.TagBlocks(a, crit, 1e300, 0.0)
        p0, p1 = 0.5 * (sorted(vals)[-1] + sorted(vals)[-2]), 0.5 * (sorted(vals)[0] + sorted(vals)[1])
        want_t, want_v = hydro.TagBlocks(a, crit, p0, p1)
        got_t, got_v = hydro.TagBlocks(b_, crit, p0, p1, face_neighbor=dtab)
        assert np.all(np.isfinite(want_v)) and list(got_v) == list(want_v) and list(got_t) == list(want_t), crit
        assert len(set(want_t)) > 1, crit
        if crit == "pressure_gradient":  # (without the table the poisoned zones are read)
            assert list(hydro.TagBlocks(b_, crit, p0, p1)[1]) != list(want_v)


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("nx,ng", [((16, 16, 16), 4), ((8, 12, 10), 2), ((40, 24, 16), 3)], ids=["16c", "8x12x10", "40x24x16"])
def test_pressure_gradient_and_time_step_from_the_conserved_state(request, nx, ng, fluid, strict):
    """apk_tag_blocks_dt_from_cons: the criterion and the estimate in one pass over the conserved state, against the two
    passes it replaces -- apk_cons_to_prim_dt_select (pressure, two layers) + apk_tag_blocks_begin_skip -- with filled
    ghost zones and through a face table whose zones are poisoned: the same maxima, tags and time step (parity build: bit
    for bit).  Wide blocks, scalars and floors refuse."""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    nb, nh = 4, (9 if fluid == "glmmhd" else 5)
    g = H.geom(fluid, nx, ng, 0, (0.1, 0.07, 0.13))
    prim = H.random_prim(fluid, nx, ng, seed=33, kind="smooth", nblocks=nb)
    prim[1, 4] *= 3.0
    prim[2, 1:4] *= 4.0
    tab = np.array([[1, 1, -1, 2, -1, 3], [0, 0, 2, -1, 1, 1], [-1, 3, 0, 2, -1, -1], [2, -1, -1, -1, 0, 3]], dtype=np.int32)
    I = [slice(ng, ng + nx[0]), slice(ng, ng + nx[1]), slice(ng, ng + nx[2])]
    cons = np.stack([H.prim_to_cons(fluid, prim[b], 5.0 / 3.0) for b in range(nb)])
    filled, poisoned = cons.copy(), cons.copy()
    for b in range(nb):
        for f in range(6):
            if tab[b, f] < 0:
                continue
            d, hi = f // 2, f % 2
            dst, src = list(I), list(I)
            dst[d] = slice(ng + nx[d], 2 * ng + nx[d]) if hi else slice(0, ng)
            src[d] = slice(ng, 2 * ng) if hi else slice(nx[d], nx[d] + ng)
            filled[b][:, dst[2], dst[1], dst[0]] = cons[tab[b, f]][:, src[2], src[1], src[0]]
            poisoned[b][:, dst[2], dst[1], dst[0]] = np.nan
    eos = hydro.L.make_eos(5.0 / 3.0)
    dtab = torch.from_numpy(tab).cuda()
    ref = hydro.MeshData(ctx, nx, ng, nh, dx=tuple(g.dx), nblocks=nb, cons=filled, prim=np.full_like(cons, np.nan), with_flux=False)
    want_dt = hydro.ConservedToPrimitiveDt(ref, fluid, eos, 0.3, ghost_depth=2, store_vars=1 << 4)
    _, vals = hydro.TagBlocks(ref, "pressure_gradient", 1e300)
    p0 = 0.5 * (sorted(vals)[-1] + sorted(vals)[-2])
    want_t, want_v = hydro.TagBlocks(ref, "pressure_gradient", p0)
    assert np.all(np.isfinite(want_v)) and len(set(want_t)) > 1
    # ... and directly against the oracle on the filled state (not only against the HIP passes it replaces): ConsToPrim
    # of every cell, the pressure-gradient criterion and tag of every block, the time step
    _, w_orc, bad = H.orc_c2p(fluid, g, filled, H.O.make_eos(5.0 / 3.0))
    orc = [H.O.tag("pressure_gradient", g, np.ascontiguousarray(w_orc[b]), p0) for b in range(nb)]
    orc_t, orc_v, orc_dt = [o[0] for o in orc], [o[1] for o in orc], 0.3 * H.orc_min_dt(fluid, g, w_orc, 5.0 / 3.0)
    assert bad == 0 and len(set(orc_t)) > 1
    for state, table in ((filled, None), (poisoned, dtab), (filled, dtab)):
        md = hydro.MeshData(ctx, nx, ng, nh, dx=tuple(g.dx), nblocks=nb, cons=state, prim=np.full_like(cons, np.nan), with_flux=False)
        t, v, dt = hydro.TagBlocksDtFromCons(md, fluid, eos, 0.3, p0, face_neighbor=table)
        assert np.all(np.isnan(md.prim_host()))                      # (nothing stored)
        if strict:
            assert list(v) == list(want_v) and list(t) == list(want_t) and dt == want_dt
            assert list(v) == orc_v and list(t) == orc_t and dt == orc_dt, "differs from the oracle"
        else:
            np.testing.assert_allclose(v, want_v, rtol=1e-13)
            assert list(t) == list(want_t) and abs(dt - want_dt) <= 4e-16 * want_dt
            print("product build against the oracle: criterion rel %.3e, dt rel %.3e" % (
                np.max(np.abs(np.array(v) - orc_v) / np.array(orc_v)), abs(dt - orc_dt) / orc_dt))
            np.testing.assert_allclose(v, orc_v, rtol=1e-13, err_msg="differs from the oracle")
            assert list(t) == orc_t and abs(dt - orc_dt) <= 4e-16 * orc_dt, "differs from the oracle"
    with pytest.raises(hydro.L.ApkError):
        hydro.TagBlocksDtFromCons(md, fluid, hydro.L.make_eos(5.0 / 3.0, pfloor=1e-9), 0.3, p0)
    wide = hydro.MeshData(ctx, (128, 128, 8), ng, nh, dx=tuple(g.dx), nblocks=1, with_flux=False)
    with pytest.raises(hydro.L.ApkError):
        hydro.TagBlocksDtFromCons(wide, fluid, eos, 0.3, p0)


# ---- the pieces of the flux correction after a fused stage, through the C-ABI --------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fluid,recon,riemann,ng", [("euler", "plm", "hllc", 2), ("glmmhd", "ppm", "hlld", 4),
                                                    ("glmmhd", "wenoz", "hlle", 3)])
@pytest.mark.parametrize("nx", [(8, 8, 8), (16, 8, 1), (72, 6, 4)], ids=["8x8x8", "2d", "wide"])
def test_boundary_plane_fluxes_equal_the_full_sweeps(request, fluid, recon, riemann, ng, nx):
    """apk_calculate_fluxes_boundary: the two block-boundary planes of every active direction, bit for
    bit what apk_calculate_fluxes puts there; nothing else is written"""
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    nh = 9 if fluid == "glmmhd" else 5
    prim = H.random_prim(fluid, nx, ng, nscalars=1, seed=9, kind="smooth", nblocks=3)
    eos = hydro.L.make_eos(5.0 / 3.0)
    full = hydro.MeshData(ctx, nx, ng, nh, nscalars=1, dx=(0.1, 0.2, 0.3), nblocks=3, prim=prim)
    bnd = hydro.MeshData(ctx, nx, ng, nh, nscalars=1, dx=(0.1, 0.2, 0.3), nblocks=3, prim=prim)
    hydro.CalculateFluxes(full, fluid, recon, riemann, eos, 1.3)
    hydro.CalculateFluxes(bnd, fluid, recon, riemann, eos, 1.3, boundary=True)
    act = [True, nx[1] > 1, nx[2] > 1]
    for d in range(full.ndim):
        a, b = full.flux_host(d), bnd.flux_host(d)
        mask = np.zeros(b.shape, bool)
        for side in (0, 1):
            sl = [slice(None), slice(None)] + [slice(ng, ng + nx[q]) if act[q] else slice(None) for q in (2, 1, 0)]
            sl[4 - d] = ng + (nx[d] if side else 0)
            sl = tuple(sl)
            assert np.array_equal(a[sl], b[sl]) and np.abs(b[sl]).max() > 0
            mask[sl] = True
        assert np.all(b[~mask] == 0.0)
    # ... and with a face list only the planes asked for (the coarse-fine faces of a refined mesh), in one launch
    import torch
    want = np.array([[1, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0], [0, 1, 1, 1, 0, 1]], dtype=np.uint8)
    msk = hydro.MeshData(ctx, nx, ng, nh, nscalars=1, dx=(0.1, 0.2, 0.3), nblocks=3, prim=prim)
    want[:, 2 * full.ndim:] = 0                                   # (inactive directions have no faces)
    codes = [6 * blk + f for blk in range(3) for f in range(6) if want[blk, f]]
    hydro.CalculateFluxes(msk, fluid, recon, riemann, eos, 1.3, boundary=True,
                          face_list=torch.tensor(codes, dtype=torch.int32, device="cuda"))
    for d in range(full.ndim):
        a, m = bnd.flux_host(d), msk.flux_host(d)
        for blk in range(3):
            for side in (0, 1):
                sl = [blk, slice(None)] + [slice(ng, ng + nx[q]) if act[q] else slice(None) for q in (2, 1, 0)]
                sl[4 - d] = ng + (nx[d] if side else 0)
                sl = tuple(sl)
                if want[blk, 2 * d + side]:
                    assert np.array_equal(m[sl], a[sl])
                else:
                    assert np.all(m[sl] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("fluid,recon,riemann,ng", [("euler", "plm", "hllc", 2), ("euler", "dc", "hlle", 2), ("glmmhd", "ppm", "hlld", 4),
                                                    ("glmmhd", "dc", "hlld", 4), ("glmmhd", "wenoz", "hlle", 3)])
def test_boundary_plane_fluxes_from_the_conserved_state(request, strict, fluid, recon, riemann, ng):
    """apk_calculate_fluxes_boundary_list_from_cons: the listed planes from the conserved state of the pack itself or of
    another one, equal to the planes from the primitives ConsToPrim stores (parity build: bit for bit); floors refuse"""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    nx, nb = (16, 8, 8), 3
    nh = 9 if fluid == "glmmhd" else 5
    gamma = 5.0 / 3.0
    prim = H.random_prim(fluid, nx, ng, seed=21, kind="smooth", nblocks=nb)
    cons = np.stack([H.prim_to_cons(fluid, prim[b], gamma) for b in range(nb)])
    eos = hydro.L.make_eos(gamma)
    ref = hydro.MeshData(ctx, nx, ng, nh, dx=(0.1, 0.2, 0.3), nblocks=nb, cons=cons)
    hydro.ConservedToPrimitive(ref, fluid, eos)
    codes = torch.tensor([6 * blk + f for blk in range(nb) for f in range(6) if (blk + f) % 2 == 0], dtype=torch.int32, device="cuda")
    hydro.CalculateFluxes(ref, fluid, recon, riemann, eos, 1.3, boundary=True, face_list=codes)
    own = hydro.MeshData(ctx, nx, ng, nh, dx=(0.1, 0.2, 0.3), nblocks=nb, cons=cons, prim=np.full_like(cons, np.nan))
    hydro.CalculateFluxes(own, fluid, recon, riemann, eos, 1.3, boundary=True, face_list=codes, from_cons=own)
    other = hydro.MeshData(ctx, nx, ng, nh, dx=(0.1, 0.2, 0.3), nblocks=nb, cons=np.full_like(cons, np.nan), prim=np.full_like(cons, np.nan))
    hydro.CalculateFluxes(other, fluid, recon, riemann, eos, 1.3, boundary=True, face_list=codes, from_cons=own)
    for d in range(3):
        want = ref.flux_host(d)
        assert np.abs(want).max() > 0
        for got in (own.flux_host(d), other.flux_host(d)):
            if strict:
                assert np.array_equal(got, want)
            else:
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    # ... and directly against the oracle (not only against the HIP passes it replaces): ConsToPrim of the state, then
    # the fluxes of every listed plane
    g = H.geom(fluid, nx, ng, 0, (0.1, 0.2, 0.3))
    _, w_orc, bad = H.orc_c2p(fluid, g, cons, H.O.make_eos(gamma))
    assert bad == 0
    fl_orc = H.orc_fluxes(fluid, recon, riemann, g, w_orc, gamma, 1.3)
    listed, planes = set(codes.cpu().tolist()), 0
    for d in range(3):
        for got in (own.flux_host(d), other.flux_host(d)):
            for blk in range(nb):
                for side in (0, 1):
                    if 6 * blk + 2 * d + side not in listed:
                        continue
                    sl = [blk, slice(None)] + [slice(ng, ng + nx[q]) for q in (2, 1, 0)]
                    sl[4 - d] = ng + (nx[d] if side else 0)
                    sl = tuple(sl)
                    assert np.abs(fl_orc[d][sl]).max() > 0
                    if strict:
                        assert np.array_equal(got[sl], fl_orc[d][sl]), "plane %d of block %d differs from the oracle" % (2 * d + side, blk)
                    else:
                        np.testing.assert_allclose(got[sl], fl_orc[d][sl], rtol=1e-12, atol=1e-13)
                    planes += 1
    assert planes == 2 * len(listed)
    floored = hydro.L.make_eos(gamma, pfloor=1e-9)
    with pytest.raises(hydro.L.ApkError):
        hydro.CalculateFluxes(own, fluid, recon, riemann, floored, 1.3, boundary=True, face_list=codes, from_cons=own)


@pytest.mark.gpu
def test_flux_fix_plan_against_numpy(request):
    """cons += beta_dt * scale * (fine_avg - coarse_flux), psi scaled by its damping factor; strided
    sources (a message buffer laid out compactly) and destinations (a plane inside a block)"""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    rng = np.random.default_rng(2)
    nvar, n = 9, 12
    cons = torch.from_numpy(rng.standard_normal((nvar, n, n, n))).cuda()
    flux = torch.from_numpy(rng.standard_normal((nvar, n, n, n))).cuda()
    buf = torch.from_numpy(rng.standard_normal((2, nvar, 4, 4))).cuda()   # two compact 4x4 planes
    want = cons.clone()
    beta_dt, psi_factor = 0.37, 0.8
    regions = []
    # lower x face of cells i = 2 (scale +1/dx), upper y face of cells j = 9 (flux at j = 10, scale -1/dx)
    v0 = (slice(None), slice(3, 7), slice(4, 8), slice(2, 3))
    regions.append((buf[0].reshape(nvar, 4, 4, 1), flux[v0], cons[v0], +1.0 / 0.25))
    c1 = (slice(None), slice(2, 6), slice(9, 10), slice(5, 9))
    f1 = (slice(None), slice(2, 6), slice(10, 11), slice(5, 9))
    regions.append((buf[1].reshape(nvar, 4, 1, 4), flux[f1], cons[c1], -1.0 / 0.5))
    for (fa, cf, cc, scale), csel in zip(regions, (v0, c1)):
        d = beta_dt * scale * (fa - cf)
        d[8] = d[8] * psi_factor
        want[csel] += d
    # the plan needs cons and flux views with equal strides: true for same-shaped contiguous parents
    hydro.FluxFixPlan(ctx, regions).run(beta_dt, psi_var=8, psi_factor=psi_factor)
    torch.cuda.synchronize()
    assert torch.equal(cons, want)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [1, 2, 3])
def test_flux_fix_plan_averages_fine_fluxes_like_the_restriction(request, direction):
    """average = d + 1: the fix kernel reads the fine block's x_d flux array and averages the four fine faces under each
    coarse face itself -- the restriction operator's weights and pairwise sums (RestrictAverage on a face), bit for bit."""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    rng = np.random.default_rng(3 + direction)
    nvar, n, nf = 9, 12, 16
    cons = torch.from_numpy(rng.standard_normal((nvar, n, n, n))).cuda()
    flux = torch.from_numpy(rng.standard_normal((nvar, n, n, n))).cuda()
    fine = torch.from_numpy(rng.standard_normal((nvar, nf, nf, nf))).cuda()
    dxf = (0.125, 0.0625, 0.25)
    w = 1.0
    for q in range(3):
        if q != direction - 1:
            w *= dxf[q]
    ax = 3 - (direction - 1)                      # tensor axis of the face normal ([nvar][k][j][i])
    csel, fsel = [slice(None)] * 4, [slice(None)] * 4
    for a in (1, 2, 3):
        if a == ax:
            csel[a], fsel[a] = slice(4, 5), slice(3, 4)          # coarse cells next to face 4 / fine face index 3
        else:
            csel[a], fsel[a] = slice(2, 6), slice(4, 12, 2)      # 4 coarse cells <- fine cells 4..11
    csel, fsel = tuple(csel), tuple(fsel)
    beta_dt, scale, psi_factor = 0.21, 1.0 / 0.5, 0.9
    f = fine.cpu().numpy()
    t = {}
    for ok in range(2):
        for oj in range(2):
            for oi in range(2):
                off = {1: ok, 2: oj, 3: oi}
                inside = off[ax] == 0
                sl = tuple(slice(None) if a == 0 else (slice(3, 4) if a == ax else slice(4 + off[a], 12 + off[a], 2)) for a in range(4))
                t[ok, oj, oi] = w * f[sl] if inside else 0.0
                t["v", ok, oj, oi] = w if inside else 0.0
    tot = ((t[0, 0, 0] + t[0, 1, 0]) + (t[0, 0, 1] + t[0, 1, 1])) + ((t[1, 0, 0] + t[1, 1, 0]) + (t[1, 0, 1] + t[1, 1, 1]))
    vol = ((t["v", 0, 0, 0] + t["v", 0, 1, 0]) + (t["v", 0, 0, 1] + t["v", 0, 1, 1])) + \
          ((t["v", 1, 0, 0] + t["v", 1, 1, 0]) + (t["v", 1, 0, 1] + t["v", 1, 1, 1]))
    avg = tot / vol
    want = cons.cpu().numpy().copy()
    d = (beta_dt * scale) * (avg - flux.cpu().numpy()[csel])
    d[8] = d[8] * psi_factor
    want[csel] += d
    hydro.FluxFixPlan(ctx, [(fine[fsel], flux[csel], cons[csel], scale, direction, 3, w, fine)]).run(beta_dt, psi_var=8, psi_factor=psi_factor)
    torch.cuda.synchronize()
    assert np.array_equal(cons.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_count_unphysical_matches_numpy(request, fluid):
    from athenapk_amd import hydro
    ctx = _ctx(request, True)
    nx, ng = (16, 8, 8), 2
    nh = 9 if fluid == "glmmhd" else 5
    rng = np.random.default_rng(4)
    cons = rng.uniform(0.5, 1.5, (2, nh, 12, 12, 20))
    cons[:, 4] += 3.0
    bad = [(0, 3, 4, 5), (1, 7, 2, 9), (1, 9, 9, 17)]
    cons[0, 0, 3, 4, 5] = -0.1                    # negative density
    cons[1, 4, 7, 2, 9] = 0.01                    # energy below kinetic (+ magnetic)
    cons[1, 0, 9, 9, 17] = 0.0                    # zero density
    cons[0, 0, 0, 0, 0] = -1.0                    # a ghost cell: not counted
    md = hydro.MeshData(ctx, nx, ng, nh, nblocks=2, cons=cons, with_flux=False)
    u = cons[:, :, ng:-ng, ng:-ng, ng:-ng]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = u[:, 4] - 0.5 * (u[:, 1] ** 2 + u[:, 2] ** 2 + u[:, 3] ** 2) / u[:, 0]
        if fluid == "glmmhd":
            p = p - 0.5 * (u[:, 5] ** 2 + u[:, 6] ** 2 + u[:, 7] ** 2)
        want = int(np.sum(~((u[:, 0] > 0) & (p > 0))))
    assert want >= len(bad)
    assert hydro.CountUnphysical(md, fluid) == want


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
def test_merged_flux_fix_plan_equals_the_plans_per_direction(request, strict):
    """apk_flux_fix_plan_create_merged: the regions of all three directions in ONE launch.  Two blocks of 12^3 cells with
    quarter-face regions (6 x 6 coarse cells, as one fine block behind a coarse face gives) on faces that meet along
    edges and in corners: cells next to two or three corrected faces must receive ((u + d1) + d2) + d3, the result of the
    three plans run one after the other, bit for bit; regions that only touch, and a block with a single face, ride along."""
    import torch
    from athenapk_amd import hydro
    ctx = _ctx(request, strict)
    rng = np.random.default_rng(77)
    nvar, ng, nx = 9, 2, 12
    n = nx + 2 * ng
    cons0 = torch.from_numpy(rng.standard_normal((2, nvar, n, n, n))).cuda()
    flux = [torch.from_numpy(rng.standard_normal((2, nvar, n, n, n))).cuda() for _ in range(3)]
    lo, hi = ng, ng + nx - 1

    def region(blk, d, side, a0, b0):
        """the quarter (6 x 6 cells from (a0, b0) in the two transverse directions) of face `side` of direction d"""
        sel = [slice(None)] * 4                                      # [var][k][j][i]
        ax = 3 - d
        cell = lo if side == 0 else hi
        face = lo if side == 0 else hi + 1
        t = [a for a in (3, 2, 1) if a != ax]                        # transverse axes, i first
        csel, fsel = list(sel), list(sel)
        csel[ax], fsel[ax] = slice(cell, cell + 1), slice(face, face + 1)
        for a, o in zip(t, (a0, b0)):
            csel[a] = fsel[a] = slice(lo + o, lo + o + 6)
        csel, fsel = tuple(csel), tuple(fsel)
        shape = cons0[blk][csel].shape
        avg = torch.from_numpy(rng.standard_normal(tuple(shape))).cuda()
        return (blk, d, csel, fsel, avg, (1.0 if side == 0 else -1.0) / (0.1 * (d + 1)))
    spec = []
    for d in range(3):                                               # block 0: the low faces of all three directions, all quarters
        for a0 in (0, 6):
            for b0 in (0, 6):
                spec.append(region(0, d, 0, a0, b0))
    spec.append(region(0, 0, 1, 6, 6))                               # ... and one quarter of the upper x1 face (meets x2 / x3 low? no: touches only)
    spec.append(region(0, 1, 1, 0, 0))                               # upper x2 face, the quarter at low x1, low x3: meets the low x1 and x3 faces
    spec.append(region(1, 2, 1, 6, 0))                               # block 1: a single region
    spec.sort(key=lambda r: r[1])
    n_by_dir = [sum(1 for r in spec if r[1] == d) for d in range(3)]

    def regions_on(cons):
        # (coarse flux views must share the cons views' strides: same-shaped parents)
        return [(avg, flux[d][blk][fsel], cons[blk][csel], scale) for blk, d, csel, fsel, avg, scale in spec]
    beta_dt, psi_factor = 0.013, 0.85
    a = cons0.clone()
    for d in range(3):
        regs = [r for r, sp_ in zip(regions_on(a), spec) if sp_[1] == d]
        hydro.FluxFixPlan(ctx, regs).run(beta_dt, psi_var=8, psi_factor=psi_factor)
    b = cons0.clone()
    hydro.FluxFixPlan(ctx, regions_on(b), merged=(n_by_dir, b)).run(beta_dt, psi_var=8, psi_factor=psi_factor)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    # the corner cell of block 0 got three terms, its edge neighbours two: not what a single term leaves
    changed = (a != cons0)
    assert changed[0, 0, lo, lo, lo] and int(changed.sum()) > 0
    once = cons0.clone()
    hydro.FluxFixPlan(ctx, [r for r, sp_ in zip(regions_on(once), spec) if sp_[1] == 0]).run(beta_dt, psi_var=8, psi_factor=psi_factor)
    torch.cuda.synchronize()
    assert not torch.equal(once[0, :, lo, lo, lo], a[0, :, lo, lo, lo])
