"""SNIa feedback, stellar feedback and the clips of the cluster problem on the GPU against the numpy restatement
(tests/cluster_sources_reference.py): every stored value and every sum bit for bit in the parity build, the edges of the
shell, the sphere and the temperature threshold, which of cons and prim each step reads, the five sums in the device's
order, the product build, whole cycles of inputs/cluster_sources.in, two ranks, and the sanity check that fails a step."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402
import cluster_sources_reference as CS  # noqa: E402
from _spawn import spawn  # noqa: E402
from cluster_cases import ROOT, box as _box, centres as _centres, geom as _geom, mesh as _mesh  # noqa: E402
from cluster_cases import next_dt as _next_dt, random_block as _random_block, read as _read, sim as _deck_sim  # noqa: E402
from test_cluster_sources_host import MESHES as HOST_MESHES  # noqa: E402

EPS = np.finfo(np.float64).eps
GAMMA = R.DECK_GAMMA
INF = float("inf")
SNIA = "problem/cluster/snia_feedback/"
STELLAR = "problem/cluster/stellar_feedback/"
CLIPS = "problem/cluster/clips/"
AGN = "problem/cluster/agn_feedback/"
GRAV = "problem/cluster/gravity/"
DECK = "cluster_sources"
# the host test's shapes, and one 24^3 block on +-0.12 with radii that cover it (the farthest centre is at sqrt(3) 0.115 =
# 0.1992, the nearest at sqrt(3) 0.005 = 0.0087): its interior is the box, 13824 cells, P = 4
MESHES = dict(HOST_MESHES)
MESHES["block24"] = _mesh(24, 24) + _box((-0.12,) * 3, (0.12,) * 3) + [STELLAR + "stellar_radius=0.3", STELLAR + "exclusion_radius=0.001",
                                                                       CLIPS + "clip_r=0.3"]
# random states are of order one in code units: an efficiency that adds an energy of the order of the thermal one
EFF = [STELLAR + "efficiency=1e-6"]
NO_CLIP_LIMITS = [CLIPS + "dfloor=-1", CLIPS + "vceil=inf", CLIPS + "Tceil=inf"]


def _interior(g):
    m = np.zeros((g.mb[2] + 2 * g.ng, g.mb[1] + 2 * g.ng, g.mb[0] + 2 * g.ng), bool)
    m[g.ng:g.ng + g.mb[2], g.ng:g.ng + g.mb[1], g.ng:g.ng + g.mb[0]] = True
    return m


def _random_sim(mesh, fluid, overrides=(), seed=5, strict=True, prim_seed=None):
    """the deck on `mesh` with a seeded random state; prim_seed: the stored primitives of every cell replaced by those of
    an independent draw, so that a step that reads the wrong one of cons and prim cannot pass.  That draw's density,
    momentum and energy are scaled by 0.4 (rho in [0.2, 0.6], same velocities and temperatures): stellar feedback removes
    the STORED density's excess over the threshold from the conserved one, which has to stay positive -- the restatement's
    ConsToPrim is the one without floors."""
    s = _deck_sim(DECK, MESHES[mesh] + ["hydro/fluid=" + fluid] + EFF + list(overrides), strict=strict).initialize()
    rng = np.random.default_rng(seed)
    for lb in range(s.info.nblocks_local):
        s.write_block(lb, _random_block(rng, s.block_shape, fluid))
    s.exchange_ghosts()
    s.fill_derived()
    if prim_seed is not None:
        rng = np.random.default_rng(prim_seed)
        for lb in range(s.info.nblocks_local):
            other = _random_block(rng, s.block_shape, fluid)
            other[:5] *= 0.4
            s.write_block(lb, CS._c2p(other, GAMMA), "prim")
    return s


def _cfgs(s):
    o = s.cluster_source_options()
    snia = CS.snia_cfg(o.power_per_bcg_mass, o.mass_rate_per_bcg_mass, o.rho_const_bcg, s.cluster_options().r_bcg_s,
                       s.cluster_options().g_smoothing_radius)
    stellar = CS.stellar_cfg(o.stellar_radius, o.exclusion_radius, o.number_density_threshold, o.temperature_threshold, o.mbar,
                             o.mbar_over_kb, o.mass_to_energy) if o.stellar_active else None
    clips = CS.clips_cfg(o.clip_r, o.dfloor, o.vceil, o.vAceil, o.eceil) if o.clips_active else None
    return o, snia, stellar, clips


def _between(values):
    """a median that is none of the values: half-way between the two middle ones"""
    v = np.unique(np.asarray(values).ravel())
    assert len(v) >= 2
    return float(0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))


def _global_sums(g, per_block):
    """the blocks' sums added in global block order, as sum_blocks_in_global_order does (absent blocks add zeros)"""
    out = np.zeros(5)
    for gid in sorted(g.gid):
        out = out + per_block[g.gid.index(gid)]
    return out


def _restate_split(s, state, stellar, clips, fluid):
    """per block (u, w, terms, infos) of the restatement and the five global sums in the device's order"""
    g = _geom(s)
    inner = _interior(g)
    boxes = {lb: (lo, hi) for lb, lo, hi in s.cluster_split_active_list()}
    P = CS.block_sum_groups(max((np.prod([h - l for l, h in zip(lo, hi)]) for lo, hi in boxes.values()), default=1))
    out, sums = [], []
    for lb, ((u, w), loc) in enumerate(zip(state, g.loc)):
        xs = _centres(g, loc, g.ng)
        res = CS.split_src(u, w, xs[0], xs[1], xs[2], inner, stellar, clips, g.vol, GAMMA, fluid == "glmmhd")
        out.append(res)
        if lb in boxes:
            lo, hi = boxes[lb]
            # everything that counts lies inside the box
            outside = np.ones(inner.shape, bool)
            outside[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = False
            assert not np.any(res[2][:, outside] != 0.0)
            sums.append(CS.box_sums(res[2], lo, hi, P))
        else:
            assert not np.any(res[2] != 0.0)
            sums.append(np.zeros(5))
    return out, _global_sums(g, sums), P


def _first_difference(a, b):
    d = np.argwhere(a != b)
    n, k, j, i = d[0]
    return "%d values differ; variable %d of cell (k, j, i) = (%d, %d, %d): %r, restated %r" % (len(d), n, k, j, i, float(a[n, k, j, i]), float(b[n, k, j, i]))


def _assert_state(s, want):
    for lb, ((u1, w1), (u_want, w_want, _, _)) in enumerate(zip(_read(s), want)):
        assert np.array_equal(u1, u_want), "cons of block %d: %s" % (lb, _first_difference(u1, u_want))
        assert np.array_equal(w1, w_want), "prim of block %d: %s" % (lb, _first_difference(w1, w_want))


def _quarter(acted, of, what):
    n, m = int(acted.sum()), int(of.sum())
    assert m > 0 and 4 * n >= m and 4 * (m - n) >= m, "%s: %d of %d cells" % (what, n, m)
    return n


# ---- A. SNIa feedback ---------------------------------------------------------------------------------------------------
def _check_snia(s, fluid, beta_dt):
    g, (o, snia, _, _), before = _geom(s), _cfgs(s), _read(s)
    inner = _interior(g)
    s.snia_feedback_src(beta_dt)
    after = _read(s)
    hit = 0
    for (u0, w0), (u1, w1), loc in zip(before, after, g.loc):
        xs = _centres(g, loc, g.ng)
        u_want, w_want, rho_bcg = CS.snia_feedback_src(u0, w0, xs[0], xs[1], xs[2], inner, snia, beta_dt, GAMMA)
        assert np.array_equal(u1, u_want) and np.array_equal(w1, w_want)
        assert np.array_equal(u1[:, ~inner], u0[:, ~inner]) and np.array_equal(w1[:, ~inner], w0[:, ~inner])  # no ghost cell is written
        assert np.all(np.isfinite(rho_bcg[inner])) and np.all(rho_bcg[inner] > 0)
        hit += int(np.sum(u1[4][inner] != u0[4][inner]))
    return before, after, hit


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("mesh", ["eight_blocks", "odd_block"])
def test_snia_feedback(mesh, fluid):
    """A random state whose stored primitives are an independent draw (the mass enters at the STORED velocity), rates that
    change the state by per cents: conserved state and stored primitives of every cell equal the restatement's bit for
    bit, no ghost cell is written, and the stored primitives afterwards are ConsToPrim of the new conserved state."""
    s = _random_sim(mesh, fluid, [SNIA + "power_per_bcg_mass=3e1", SNIA + "mass_rate_per_bcg_mass=2e1"], prim_seed=11)
    g = _geom(s)
    before, after, hit = _check_snia(s, fluid, 2e-3)
    s.close()
    assert hit == g.nb * g.mb[0] * g.mb[1] * g.mb[2]
    inner = _interior(g)
    for (u0, _), (u1, w1) in zip(before, after):
        gain = (u1[0] / u0[0] - 1)[inner]
        assert gain.max() > 1e-3 and gain.min() > 0
        assert np.array_equal(w1[:, inner], CS._c2p(u1, GAMMA)[:, inner])


@pytest.mark.gpu
def test_snia_feedback_uses_the_smoothing_radius_at_the_centre():
    """centres at multiples of 1/8: the cell at r = 0 takes r' = g_smoothing_radius, and every cell nearer than it does"""
    ov = [SNIA + "power_per_bcg_mass=3e1", SNIA + "mass_rate_per_bcg_mass=2e1", GRAV + "g_smoothing_radius=0.13", GRAV + "r_bcg_s=0.05"]
    s = _random_sim("centre_at_zero", "glmmhd", ov, prim_seed=11)
    g = _geom(s)
    xs = _centres(g, g.loc[0], g.ng)
    i, j, k = (int(np.nonzero(x == 0.0)[0][0]) for x in xs)
    before, after, _ = _check_snia(s, "glmmhd", 1e-3)
    _, snia, _, _ = _cfgs(s)
    s.close()
    assert snia.smoothing_r == 0.13
    gain = after[0][0][0] - before[0][0][0]
    assert np.isfinite(gain[k, j, i]) and gain[k, j, i] > 0
    # the six neighbours at r = 0.125 < 0.13 receive the same density as the centre
    d_centre = float(CS.bcg_density(snia, np.float64(0.0)))
    assert d_centre == float(CS.bcg_density(snia, np.float64(0.125))) and d_centre > float(CS.bcg_density(snia, np.float64(0.25)))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["energy", "mass"])
def test_snia_feedback_with_one_rate_alone(which):
    ov = [SNIA + "power_per_bcg_mass=%r" % (3e1 if which == "energy" else 0.0),
          SNIA + "mass_rate_per_bcg_mass=%r" % (2e1 if which == "mass" else 0.0)]
    s = _random_sim("eight_blocks", "euler", ov, prim_seed=11)
    inner = _interior(_geom(s))
    before, after, _ = _check_snia(s, "euler", 2e-3)
    s.close()
    for (u0, _), (u1, _) in zip(before, after):
        assert np.all(u1[4][inner] > u0[4][inner])
        if which == "energy":
            assert np.array_equal(u1[:4], u0[:4])
        else:
            assert np.all(u1[0][inner] > u0[0][inner]) and np.all(u1[1][inner] != u0[1][inner])


# ---- B. stellar feedback --------------------------------------------------------------------------------------------------
def _stellar_thresholds(mesh, fluid, prim_seed=11):
    """thresholds between the two middle values of n and T over the shell's cells of all blocks"""
    s = _random_sim(mesh, fluid, prim_seed=prim_seed)
    g, (o, _, stellar, _), state = _geom(s), _cfgs(s), _read(s)
    s.close()
    inner = _interior(g)
    n, t = [], []
    for (_, w), loc in zip(state, g.loc):
        sh = CS.stellar_shell(*_centres(g, loc, g.ng), stellar) & inner
        n.append((w[0] / stellar.mbar)[sh])
        t.append((stellar.mbar_over_kb * w[4] / w[0])[sh])
    return [STELLAR + "number_density_threshold=%r" % _between(np.concatenate(n)),
            STELLAR + "temperature_threshold=%r" % _between(np.concatenate(t))]


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("mesh", ["eight_blocks", "odd_block"])
def test_stellar_feedback(mesh, fluid):
    """Both thresholds at the medians of the shell (the stored primitives, an independent draw, decide): in every block
    the shell crosses at least a quarter of its cells convert and at least a quarter do not.  Every cell of every block
    equals the restatement bit for bit, cells that do not convert keep their bits, the returned stellar_mass is the
    restated sum in the device's order, and the clips' sums are zero."""
    ov = _stellar_thresholds(mesh, fluid)
    s = _random_sim(mesh, fluid, ov, prim_seed=11)
    g, (o, _, stellar, _), before = _geom(s), _cfgs(s), _read(s)
    want, sums, _ = _restate_split(s, before, stellar, None, fluid)
    got = s.cluster_split_src(1e-3, stellar=True, clips=False)
    _assert_state(s, want)
    after = _read(s)
    totals = s.cluster_source_totals()
    s.close()
    converted = 0
    for (u0, w0), (u1, w1), (_, _, _, infos) in zip(before, after, want):
        info = infos.stellar
        assert not info.failed
        if info.shell.any():
            converted += _quarter(info.converted, info.shell, "converted")
        keep = ~info.converted
        assert np.array_equal(u1[:, keep], u0[:, keep]) and np.array_equal(w1[:, keep], w0[:, keep])
        assert np.all(u1[0][info.converted] < u0[0][info.converted])
    print("converted %d cells; stellar_mass %.17g" % (converted, got[0]))
    assert converted >= 8 and np.array_equal(got, sums) and got[0] > 0 and np.all(got[1:] == 0)
    assert np.array_equal(totals, got)


@pytest.mark.gpu
def test_the_edges_of_the_shell_the_sphere_and_the_temperature():
    """centres at multiples of 1/8.  stellar_radius = 0.25 includes the cells at distance exactly 0.25 (r > R leaves),
    exclusion_radius = 0.125 excludes those at exactly 0.125 (r <= R leaves), clip_r = 0.25 excludes those at exactly
    0.25 (strict, on r2); a temperature equal to the threshold converts (T > threshold leaves) and a threshold one ulp
    lower does not."""
    # (threshold * mbar = 0.1995: every cell's stored density is above; of the clips a velocity ceiling most cells meet)
    low_n = [STELLAR + "number_density_threshold=4e70", CLIPS + "dfloor=-1", CLIPS + "vceil=1.0", CLIPS + "Tceil=inf"]
    s = _random_sim("centre_at_zero", "euler", low_n, prim_seed=11)
    g, (o, _, stellar, clips), (state,) = _geom(s), _cfgs(s), _read(s)
    s.close()
    assert (o.stellar_radius, o.exclusion_radius, o.clip_r) == (0.25, 0.125, 0.25)
    xs = _centres(g, g.loc[0], g.ng)
    at = lambda x, y, z: tuple(int(np.nonzero(c == v)[0][0]) for c, v in ((xs[2], z), (xs[1], y), (xs[0], x)))  # noqa: E731
    shell, sphere = CS.stellar_shell(*xs, stellar), CS.clip_sphere(*xs, clips)
    assert shell[at(0.25, 0.0, 0.0)] and shell[at(0.0, -0.25, 0.0)] and not shell[at(0.125, 0.0, 0.0)] and not shell[at(0.0, 0.0, 0.0)]
    assert shell[at(0.125, 0.125, 0.0)] and not shell[at(0.25, 0.125, 0.0)]
    assert not sphere[at(0.25, 0.0, 0.0)] and sphere[at(0.125, 0.125, 0.125)]
    k, j, i = at(0.25, 0.0, 0.0)
    temp = float((stellar.mbar_over_kb * state[1][4] / state[1][0])[k, j, i])
    for thresh, converts in ((temp, True), (float(np.nextafter(temp, 0.0)), False)):
        s = _random_sim("centre_at_zero", "euler", low_n + [STELLAR + "temperature_threshold=%r" % thresh], prim_seed=11)
        (_, _, stellar, clips), before = _cfgs(s), _read(s)
        want, sums, _ = _restate_split(s, before, stellar, clips, "euler")
        got = s.cluster_split_src(1e-3)
        _assert_state(s, want)
        (u1, _), = _read(s)
        s.close()
        infos = want[0][3]
        assert infos.stellar.converted[k, j, i] == converts and (u1[0][k, j, i] != before[0][0][0][k, j, i]) == converts
        assert np.array_equal(got, sums)
        # the cell on the sphere's edge is not clipped: only the stellar step can have changed it
        assert not infos.clips.inside[k, j, i] and infos.clips.inside.sum() == 27


# ---- C. the clips -----------------------------------------------------------------------------------------------------------
def _clip_limits(mesh, fluid, which):
    """limits between the two middle values of what each clip tests, over the sphere's cells of all blocks, from the
    conserved state (the clips convert first); with all clips together each limit is taken on the state the clips
    before it leave"""
    s = _random_sim(mesh, fluid, [CLIPS + "dfloor=1e-30", CLIPS + "vceil=inf", CLIPS + "Tceil=inf"])
    g, (o, _, _, clips), state = _geom(s), _cfgs(s), _read(s)
    s.close()
    inner, gm1 = _interior(g), GAMMA - 1.0
    xs = [_centres(g, loc, g.ng) for loc in g.loc]
    inside = [CS.clip_sphere(*x, clips) & inner for x in xs]
    lim = CS.clips_cfg(o.clip_r)
    ov = {"dfloor": -1.0, "vceil": INF, "Tceil": INF}

    def run():
        return [CS.cluster_clips(uu, ww, x[0], x[1], x[2], inner, lim, g.vol, GAMMA, fluid == "glmmhd")[1] for (uu, ww), x in zip(state, xs)]

    def over(f):
        return np.concatenate([f(w)[m] for w, m in zip(run(), inside)])

    if "dfloor" in which:
        lim.dfloor = np.float64(_between(over(lambda w: w[0])))
        ov["dfloor"] = float(lim.dfloor)
    if "vceil" in which:
        lim.vceil = np.float64(_between(over(lambda w: np.sqrt(w[1] * w[1] + w[2] * w[2] + w[3] * w[3]))))
        ov["vceil"] = float(lim.vceil)
    if "vAceil" in which and fluid == "glmmhd":
        lim.vAceil = np.float64(_between(over(lambda w: np.sqrt((w[5] * w[5] + w[6] * w[6] + w[7] * w[7]) / w[0]))))
        ov["vAceil"] = float(lim.vAceil)
    if "Tceil" in which:
        ov["Tceil"] = _between(over(lambda w: w[4] / (gm1 * w[0]))) * gm1 * o.mbar_over_kb
    return [CLIPS + "%s=%r" % kv for kv in ov.items()]


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("which", ["dfloor", "vceil", "vAceil", "Tceil", "dfloor+vceil+vAceil+Tceil"])
def test_clips(which, fluid):
    """Each clip alone and all together on eight blocks, limits at medians: in every block at least a quarter of the
    sphere's cells meet each clip and a quarter do not.  The stored primitives are an independent draw that the clips
    must NOT read (they convert first).  Every cell equals the restatement bit for bit; cells outside the sphere keep
    their bits; the four sums are the restated ones in the device's order; after dfloor the stored velocity is the stale
    one, M / rho_old; vAceil is refused for euler at creation (the kernel's own indifference: the test below)."""
    if which == "vAceil" and fluid == "euler":
        from athenapk_amd import lib as L
        with pytest.raises(L.ApkError) as e:
            _random_sim("eight_blocks", fluid, NO_CLIP_LIMITS + [CLIPS + "vAceil=1.0"])
        assert CLIPS + "vAceil" in str(e.value)
        return
    ov = _clip_limits("eight_blocks", fluid, which)
    s = _random_sim("eight_blocks", fluid, ov, prim_seed=11)
    (o, _, _, clips), before = _cfgs(s), _read(s)
    want, sums, _ = _restate_split(s, before, None, clips, fluid)
    got = s.cluster_split_src(1e-3, stellar=False, clips=True)
    _assert_state(s, want)
    after = _read(s)
    s.close()
    names = [n for n in ("dfloor", "vceil", "vAceil", "eceil") if (n if n != "eceil" else "Tceil") in which and (n != "vAceil" or fluid == "glmmhd")]
    for (u0, w0), (u1, w1), (_, _, _, infos) in zip(before, after, want):
        info = infos.clips
        assert info.inside.any()
        for n in names:
            _quarter(getattr(info, n), info.inside, n)
        out = ~info.inside
        assert np.array_equal(u1[:, out], u0[:, out]) and np.array_equal(w1[:, out], w0[:, out])
        if which == "dfloor":  # the momenta are untouched and the velocity is still M / rho_old
            f = info.dfloor
            assert np.all(u1[0][f] == o.dfloor) and np.all(w1[0][f] == o.dfloor)
            assert np.array_equal(u1[1:4][:, f], u0[1:4][:, f])
            assert np.array_equal(w1[1][f], (u0[1] * (1.0 / u0[0]))[f]) and np.all(w1[1][f] != (u1[1] / u1[0])[f])
    slot = {"dfloor": 1, "eceil": 2, "vceil": 3, "vAceil": 4}
    print("sums", got)
    assert np.array_equal(got, sums) and got[0] == 0
    assert all((got[q] > 0) == (n in names) for n, q in slot.items())


@pytest.mark.gpu
def test_the_kernel_ignores_vAceil_on_a_hydro_pack(gpu_ctx_strict):
    """apk_cluster_split_src itself on a hydro pack with a finite vAceil and nothing else: no sum, and only what the
    clips' opening ConsToPrim stores (the deck refuses the key for euler, so the entry is called directly)"""
    import torch
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    ctx, n, ng, dx = gpu_ctx_strict, 8, 2, 0.125
    N = n + 2 * ng
    rng = np.random.default_rng(3)
    cons = _random_block(rng, (5, N, N, N), "euler")[None]
    prim = CS._c2p(_random_block(rng, (5, N, N, N), "euler"), GAMMA)[None]
    md = hydro.MeshData(ctx, (n, n, n), ng, 5, dx=(dx,) * 3, nblocks=1, cons=cons, prim=prim, with_flux=False)
    dev = torch.device("cuda")
    corners = torch.from_numpy(np.array([[-0.4375] * 3, [-0.4375] * 3])).to(dev)
    arr = (L.TrigBox * 1)(L.TrigBox(0, (C.c_int * 3)(ng, ng, ng), (C.c_int * 3)(ng + n, ng + n, ng + n)))
    boxes = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev)
    sums = torch.full((1, 8), 7.0, dtype=torch.float64, device=dev)
    clips, eos = L.ClipsCfg(0.25, -1.0, INF, 1e-3, INF), L.make_eos(GAMMA)
    rc = ctx.lib.apk_cluster_split_src(ctx.h, md.h, L.FLUID["euler"], C.byref(eos), None, C.byref(clips), boxes.data_ptr(), 1, n ** 3,
                                       corners.data_ptr(), sums.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    xs = [R.cell_centres(-0.4375, dx, -ng, N)] * 3
    inner = np.zeros((N, N, N), bool)
    inner[ng:-ng, ng:-ng, ng:-ng] = True
    u_want, w_want, terms, info = CS.cluster_clips(cons[0], prim[0], xs[0], xs[1], xs[2], inner, CS.clips_cfg(0.25, vAceil=1e-3), dx ** 3, GAMMA, False)
    assert np.array_equal(md.cons_host()[0], u_want) and np.array_equal(md.prim_host()[0], w_want)
    assert np.array_equal(u_want, cons[0]) and info.inside.sum() == 27 and not np.any(terms)
    assert np.all(sums.cpu().numpy() == 0.0) and ctx.poll_flags() == 0


# ---- D. both steps, the sums, ghost cells ---------------------------------------------------------------------------------
def _both_overrides(mesh, fluid):
    which = "dfloor+vceil+vAceil+Tceil"
    return _stellar_thresholds(mesh, fluid) + _clip_limits(mesh, fluid, which)


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_one_call_with_both_equals_stellar_then_clips(fluid):
    """eight blocks, stellar feedback and all clips: one call equals the restatement of both steps and, bit for bit, two
    calls -- stellar alone, then the clips alone; the sums of the one call are those of the two (each slot has one source)"""
    ov = _both_overrides("eight_blocks", fluid)
    s = _random_sim("eight_blocks", fluid, ov, prim_seed=11)
    (_, _, stellar, clips), before = _cfgs(s), _read(s)
    want, sums, _ = _restate_split(s, before, stellar, clips, fluid)
    got = s.cluster_split_src(1e-3)
    _assert_state(s, want)
    one = _read(s)
    s.close()
    s = _random_sim("eight_blocks", fluid, ov, prim_seed=11)
    first = s.cluster_split_src(1e-3, stellar=True, clips=False)
    second = s.cluster_split_src(1e-3, stellar=False, clips=True)
    totals = s.cluster_source_totals()
    for (u1, w1), (u2, w2) in zip(one, _read(s)):
        assert np.array_equal(u1, u2) and np.array_equal(w1, w2)
    s.close()
    assert np.array_equal(got, sums) and np.all(got[:4] > 0)
    assert np.array_equal(first + second, got) and np.array_equal(totals, got)


@pytest.mark.gpu
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("mesh", ["block24", "eight_blocks"])
def test_the_five_sums_in_the_shared_order(mesh, fluid):
    """The five sums equal block_sum of the restated terms in box order, bit for bit: on the 24^3 block whose interior is
    the box (13824 cells: P = 4 workgroups share it) and on eight blocks (P = 1, the blocks' sums added in global order).
    On the 24^3 block every interior cell lies in the shell and in the sphere, and no ghost cell is written."""
    ov = _both_overrides(mesh, fluid)
    s = _random_sim(mesh, fluid, ov, prim_seed=11)
    g, (o, _, stellar, clips), before = _geom(s), _cfgs(s), _read(s)
    want, sums, P = _restate_split(s, before, stellar, clips, fluid)
    got = s.cluster_split_src(1e-3)
    _assert_state(s, want)
    after = _read(s)
    s.close()
    inner = _interior(g)
    if mesh == "block24":
        assert o.active_box_cells == 13824 and P == 4
        infos = want[0][3]
        assert np.array_equal(infos.stellar.shell, inner) and np.array_equal(infos.clips.inside, inner)
    else:
        assert o.active_blocks == 8 and P == 1
    for (u0, w0), (u1, w1) in zip(before, after):
        assert np.array_equal(u1[:, ~inner], u0[:, ~inner]) and np.array_equal(w1[:, ~inner], w0[:, ~inner])
        assert np.any(u1[:, inner] != u0[:, inner])
    print("P = %d, device %s, restated %s" % (P, got, sums))
    assert np.array_equal(got, sums) and np.all(got[:4] > 0) and (got[4] > 0) == (fluid == "glmmhd")


# ---- E. the product build ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_product_build_stays_close():
    """eight GLM-MHD blocks, SNIa feedback and then both split steps: every value the parity build changes is within 1e-12
    relative in the product build (the bound the gravity, feedback and triggering tests use), cells the parity build
    leaves alone keep their bits, and the sums agree within 1e-12.  No cell lies within 1e-9 relative of a threshold or
    an edge (asserted on the parity state), so no cell can decide differently."""
    ov = _both_overrides("eight_blocks", "glmmhd") + [SNIA + "power_per_bcg_mass=3e1", SNIA + "mass_rate_per_bcg_mass=2e1"]
    out = {}
    for strict in (True, False):
        s = _random_sim("eight_blocks", "glmmhd", ov, strict=strict, prim_seed=11)
        start = _read(s)
        if strict:
            (_, _, stellar, clips) = _cfgs(s)
            want, _, _ = _restate_split(s, start, stellar, clips, "glmmhd")
            margin = min(min(w[3].stellar.margin, w[3].clips.margin) for w in want)
            print("least distance from a threshold: %.3e" % margin)
            assert margin > 1e-9
        sums = s.cluster_split_src(1e-3)
        mid = _read(s)
        s.snia_feedback_src(2e-3)
        out[strict] = (start, mid, _read(s), sums)
        s.close()
    (start, mid_s, end_s, sums_s), (start_f, mid_f, end_f, sums_f) = out[True], out[False]
    assert np.all(np.abs(sums_f - sums_s) <= 1e-12 * np.abs(sums_s)) and np.all(sums_s > 0)
    for lb in range(len(start)):
        assert np.array_equal(start[lb][0], start_f[lb][0]) and np.array_equal(start[lb][1], start_f[lb][1])
        for a, b, base in ((mid_s[lb], mid_f[lb], start[lb]), (end_s[lb], end_f[lb], mid_s[lb])):
            for q in (0, 1):
                changed = a[q] != base[q]
                assert changed.any() and np.array_equal(b[q][~changed], base[q][~changed] if base is start[lb] else b[q][~changed])
                assert np.all(np.abs(b[q] - a[q]) <= 1e-12 * np.abs(a[q]))
        # cells the split step leaves alone in the parity build keep their bits in the product build
        same = (mid_s[lb][0] == start[lb][0]) & (mid_s[lb][1] == start[lb][1])
        assert np.array_equal(mid_f[lb][0][same], start[lb][0][same]) and np.array_equal(mid_f[lb][1][same], start[lb][1][same])


# ---- F. the driver ----------------------------------------------------------------------------------------------------------
CYCLE_OV = _mesh(16, 8) + ["parthenon/time/tlim=10.0"]
# (cfl = 0.01: an explicit step of the BCG's field ten times longer moves the gas near the centre by more than its sound
# speed, and the energy the gravity source leaves is below the new kinetic energy)
ORDER_OV = CYCLE_OV + ["parthenon/time/integrator=rk1", "parthenon/time/cfl=0.01", GRAV + "gravity_srcterm=true", AGN + "disabled=false",
                       AGN + "fixed_power=0.3319965633348794", AGN + "thermal_fraction=1", AGN + "thermal_radius=0.015"]


@pytest.mark.gpu
def test_gravity_then_agn_feedback_then_snia_then_the_split_sources():
    """rk1 (a cycle IS a stage) and riemann = none: one cycle of the deck at 16^3 in 8^3 blocks, with the BCG's gravity and
    a thermal AGN on top (it heats the eight cells nearest the centre, inside the exclusion radius), equals the same start state advanced by the single calls in order -- gravity, AGN feedback,
    SNIa with dt, then cluster_split_src(dt) -- bit for bit on the conserved state of every interior cell, and after the
    cycle's exchange and FillDerived on everything; the cycle's totals are the call's sums.  SNIa before gravity does not."""
    s = _deck_sim(DECK, ORDER_OV).initialize()
    assert s.cluster_source_options().flux_path_sources == 1 and s.agn_feedback_options().active == 1
    g, dt = _geom(s), _next_dt(s)
    s.step()
    got, totals = _read(s), s.cluster_source_totals()
    s.close()
    results = {}
    for order in ("reference", "snia_first"):
        s = _deck_sim(DECK, ORDER_OV).initialize()
        assert _next_dt(s) == dt
        if order == "snia_first":
            s.snia_feedback_src(dt)
        s.gravity_src(dt)
        s.agn_feedback_src(dt)
        if order == "reference":
            s.snia_feedback_src(dt)
        sums = s.cluster_split_src(dt)
        s.exchange_ghosts()
        s.fill_derived()
        results[order] = (_read(s), sums)
        s.close()
    want, sums = results["reference"]
    for (u1, w1), (u2, w2) in zip(got, want):
        assert np.array_equal(u1, u2) and np.array_equal(w1, w2)
    assert np.array_equal(totals, sums) and np.all(sums[:4] > 0) and sums[4] == 0
    assert any(not np.array_equal(u1, u2) for (u1, _), (u2, _) in zip(got, results["snia_first"][0]))


@pytest.mark.gpu
def test_snia_mass_per_cycle_with_vl2():
    """SNIa feedback alone, VL2, five cycles, the mass rate raised until a cycle adds about a per cent at 10 kpc.  VL2's
    second stage starts again from the cycle's first state, so a cycle adds mass_rate * dt * rho_bcg to every cell and the
    injected mass is mass_rate * dt * sum(rho_bcg * vol).  Both sides are summed exactly (fsum); a cell's new density is one
    rounded sum, within eps / 2 of its value, and the expectation carries three roundings per cell: the bound is
    N eps max(rho) vol / 2 + 3 eps injected for the N cells."""
    from athenapk_amd import decks
    text = "\n".join(ln for ln in decks.load(DECK).split("<problem/cluster/stellar_feedback>")[0].splitlines()) + "\n"
    from athenapk_amd import driver
    s = driver.Simulation(text, CYCLE_OV + [SNIA + "mass_rate_per_bcg_mass=1e3"], strict=True).initialize()
    o = s.cluster_source_options()
    assert (o.snia_active, o.stellar_active, o.clips_active) == (1, 0, 0) and "stellar_mass" not in s.history_labels()
    g, (_, snia, _, _) = _geom(s), _cfgs(s)
    inner = _interior(g)
    rho_bcg = []
    for loc in g.loc:
        xs = _centres(g, loc, g.ng)
        X, Y, Z = CS.FB.grid(*xs)
        rho_bcg.append(CS.bcg_density(snia, np.sqrt(X * X + Y * Y + Z * Z))[inner])
    rho_bcg = np.concatenate(rho_bcg)
    n = len(rho_bcg)
    assert n == 16 ** 3
    for cycle in range(5):
        before = np.concatenate([u[0][inner] for u, _ in _read(s)])
        dt = _next_dt(s)
        s.step()
        after = np.concatenate([u[0][inner] for u, _ in _read(s)])
        injected = math.fsum((after - before) * g.vol)
        want = math.fsum((snia.mass_rate_per_bcg_mass * np.float64(dt)) * rho_bcg * g.vol)
        bound = n * EPS * float(after.max()) * float(g.vol) / 2 + 3 * EPS * want
        # (the difference after - before is exact or rounded once more: within the same eps / 2 per cell)
        print("cycle %d: dt %.4e injected %.17g expected %.17g (%.2f of the bound)" % (cycle, dt, injected, want, abs(injected - want) / (2 * bound)))
        assert want > 1e-4 * math.fsum(before * g.vol) and abs(injected - want) <= 2 * bound
    assert np.all(s.cluster_source_totals() == 0)
    s.close()


@pytest.mark.gpu
def test_history_columns_and_totals_reset(tmp_path):
    """the deck with VL2, five cycles: the totals accumulate from cycle to cycle (SNIa reheats and refills what the
    clips and stellar feedback took), the history carries the five columns under the reference's names after the
    existing ones, the row holds the totals, and writing it resets them"""
    s = _deck_sim(DECK, CYCLE_OV).initialize()
    labels = s.history_labels()
    assert labels[-5:] == list(CS.TOTALS) and labels[:6] == ["mass", "1-mom", "2-mom", "3-mom", "KE", "tot-E"]
    assert np.all(s.cluster_source_totals() == 0)
    prev = np.zeros(5)
    for cycle in range(5):
        s.step()
        t = s.cluster_source_totals()
        print("cycle %d totals %s" % (cycle, t))
        assert np.all(t >= prev) and t[2] > prev[2] and t[4] == 0
        prev = t
    assert np.all(prev[:4] > 0)
    path = os.path.join(str(tmp_path), "cluster_sources.hst")
    s.write_history(path)
    assert np.all(s.cluster_source_totals() == 0)
    row = np.loadtxt(path, ndmin=2)[-1]
    assert len(row) == 4 + len(labels)
    assert np.all(np.abs(row[-5:] - prev) <= 1e-5 * np.abs(prev))  # (the default format prints six digits)
    s.step()
    again = s.cluster_source_totals()
    assert again[2] > 0 and np.all(again <= prev)
    s.write_history(path)
    rows = np.loadtxt(path, ndmin=2)
    assert rows.shape[0] == 2 and np.all(np.abs(rows[1][-5:] - again) <= 1e-5 * np.abs(again) + 1e-300)
    s.close()


def _run_cycles(s, ncycles):
    for _ in range(ncycles):
        s.step()
    scalars = dict(time=s.time, dt=s.dt, totals=s.cluster_source_totals())
    blocks = {s.block_gid(lb)[0]: s.read_block(lb, "cons") for lb in range(s.info.nblocks_local)}
    s.close()
    return scalars, blocks


def _rank_worker(rank, world, port, outdir, overrides, ncycles):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        scalars, blocks = _run_cycles(_deck_sim(DECK, overrides, rank=rank, nranks=world).initialize(), ncycles)
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **scalars, **{"b%d" % g: a for g, a in blocks.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_equal_one(tmp_path):
    """the deck on eight 8^3 blocks, 3 cycles, two ranks sharing the GPU (gloo): every block, ghost cells included, the
    time, the time step and the five totals equal the one-rank run's bit for bit"""
    scalars, one = _run_cycles(_deck_sim(DECK, CYCLE_OV).initialize(), 3)
    assert np.all(scalars["totals"][:4] > 0)
    spawn(_rank_worker, lambda port: (2, port, str(tmp_path), list(CYCLE_OV), 3), 2)
    seen = set()
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert all(np.array_equal(z[name], value) for name, value in scalars.items())
        for key in z.files:
            if key.startswith("b"):
                seen.add(int(key[1:]))
                assert np.array_equal(z[key], one[int(key[1:])]), "rank %d block %s" % (r, key)
    assert seen == set(one) and len(seen) == 8


@pytest.mark.gpu
def test_a_negative_efficiency_fails_the_step_and_not_the_process():
    """efficiency < 0: the energy stellar feedback would add is negative where the reference's sanity check aborts.  The
    kernel latches its flag, the step raises with the reference's message, and a fresh simulation on the same process steps."""
    from athenapk_amd import lib as L
    s = _deck_sim(DECK, CYCLE_OV + [STELLAR + "efficiency=-5e-9"]).initialize()
    with pytest.raises(L.ApkError) as e:
        s.step()
    assert "Sanity check failed. Added thermal energy should be positive." in str(e.value)
    s.close()
    s = _deck_sim(DECK, CYCLE_OV).initialize()
    s.step()
    assert s.ncycle == 1 and np.all(np.isfinite(s.gather("cons"))) and s.cluster_source_totals()[0] > 0
    s.close()
