"""The oracle and both HIP builds against values that the REFERENCE's own compiled headers computed.

tests/golden/reference_vectors.npz (+ .json, made by tests/golden/make_reference_vectors.py) stores inputs, the
outputs of oracle/_ref/ref_vectors for them -- the reference's src/recon/*_simple.hpp, src/hydro/rsolvers/*.hpp and
src/eos/adiabatic_*.hpp compiled unmodified against the stand-in names of oracle/ref/standin -- and a physical scale
per case and variable, max(|F_v(W)|, S |U_v(W)|) over the cells that feed a face (tests/reference_families.py).

  CPU stored : the oracle reproduces every stored output bit for bit (needs neither the binary nor the tree)
  CPU live   : where the reference tree is present (oracle.build_ref()), 20 000 fresh inputs per reconstruction or
               solver per family per direction, and 20 000 ConsToPrim states per fluid and regime: the oracle equals
               the binary in every bit, NaN positions included.  Skips, naming the missing tree, where there is none.
  GPU stored : through the real kernels, as tests/test_edge_cases.py: Riemann cases as neighbouring cells of
               donor-cell blocks along each direction, pencils as the lines of a 70 x 2 x 2 block and its transposes,
               ConsToPrim cases as the cells of a block.  Strict build: every bit.  Product (FMA) build:
               |got - want| <= 1e-12 x scale[case, variable] -- the project's product-build bound
               (test_gpu_parity.FAST_TOL), applied per case and variable and not per array.
  GPU live   : 4096 fresh pairs per fluid with expected values from the binary, if it travelled with the tree.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import reference_families as R
from oracle import oracle as O

GDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRODUCT_TOL = 1e-12
N_LIVE = 20000
LIVE_C_H = (0.5, 2.0, 50.0)


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(GDIR, "reference_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rmeta():
    with open(os.path.join(GDIR, "reference_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GDIR, "edge_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def emeta():
    with open(os.path.join(GDIR, "edge_cases.json")) as f:
        return json.load(f)


def _bits(got, want, what):
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.argwhere((got != want) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError("%s: %d entries differ bitwise, first at %s: %r vs %r" % (
            what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _oracle_c2p(fluid, u, eos_kw, gamma, nscalars):
    """(u after floors, w) of rows u [n][nv + nscalars] through the oracle's block-level ConsToPrim"""
    n = u.shape[0]
    g = H.geom(fluid, (n, 1, 1), 0, nscalars)
    cons = np.ascontiguousarray(u.T).reshape(1, u.shape[1], 1, 1, n)
    ua, w, _ = H.orc_c2p(fluid, g, cons, O.make_eos(gamma, **eos_kw))
    return ua[0, :, 0, 0, :].T, w[0, :, 0, 0, :].T


def _oracle_pencils(fluid, recon, solver, d, ws, gamma, c_h):
    """face fluxes of the pencils laid in a block along direction d, as x1 cases: [(pencil index, [ncell][nv])]"""
    nx, w = R.pencil_block(list(ws), d)
    g = H.geom(fluid, nx, R.PENCIL_NG, 0, (R.PENCIL_DX,) * 3)
    fl = H.orc_fluxes(fluid, recon, solver, g, w, gamma, c_h)
    return R.pencil_block_faces(fl[d - 1][0], d, len(ws))


# ---- CPU, stored: the oracle against what the reference computed ------------------------------------------------------------
def test_oracle_equals_reference_on_crafted_stencils(ref, rmeta, gold):
    c = rmeta["crafted"]
    for m in R.RECONS:
        ql, qr = O.recon_many(m, gold["ppm_q"], dx=c["stencil_dx"], n=0)
        _bits(ql, ref["stencil_%s_ql" % m], m + " ql")
        _bits(qr, ref["stencil_%s_qr" % m], m + " qr")


def test_oracle_equals_reference_on_crafted_riemann_cases(ref, rmeta, gold, emeta):
    c = rmeta["crafted"]
    for n, case in enumerate(emeta["riemann"]):
        nv = R.NV[case["fluid"]]
        for d in (1, 2, 3):
            f = O.riemann_many(case["fluid"], case["riemann"], d, gold["riemann_%02d_wl_dir%d" % (n, d)],
                               gold["riemann_%02d_wr_dir%d" % (n, d)], c["gamma"], c["c_h"])
            _bits(f[0], ref["crafted_riemann_flux"][n, d - 1, :nv], "%s dir %d" % (case["label"], d))


def test_oracle_equals_reference_on_crafted_cons_to_prim_cases(ref, rmeta, gold, emeta):
    for n, case in enumerate(emeta["c2p"]):
        ua, w = _oracle_c2p("glmmhd", gold["c2p_%02d_u" % n][None], case["eos"], rmeta["crafted"]["gamma"], 0)
        _bits(ua[0], ref["crafted_c2p_u_after"][n], case["label"] + " (cons)")
        _bits(w[0], ref["crafted_c2p_w"][n], case["label"] + " (prim)")


def test_oracle_equals_reference_on_stored_riemann_pairs(ref, rmeta):
    n = 0
    for key, m in rmeta["riemann"].items():
        wl, wr = ref[key + "_wl"].astype(np.float64), ref[key + "_wr"].astype(np.float64)
        for solver in m["solvers"]:
            for d in (1, 2, 3):
                f = O.riemann_many(m["fluid"], solver, d, R.rotate(wl, d), R.rotate(wr, d), rmeta["gamma"], m["c_h"])
                _bits(R.unrotate(f, d), ref["%s_%s_flux" % (key, solver)], "%s %s dir %d" % (key, solver, d))
                n += wl.shape[0]
    assert n == 256 * 3 * (3 * 2 + 5 * 2)


def test_oracle_equals_reference_on_stored_cons_to_prim_states(ref, rmeta):
    for key, m in rmeta["c2p"].items():
        ua, w = _oracle_c2p(m["fluid"], ref[key + "_u"], m["eos"], rmeta["gamma"], m["nscalars"])
        _bits(ua, ref[key + "_u_after"], key + " (cons)")
        _bits(w, ref[key + "_w"], key + " (prim)")


@pytest.mark.parametrize("fluid,recon,solver", R.PENCIL_COMBOS)
def test_oracle_equals_reference_on_stored_pencils(ref, rmeta, fluid, recon, solver):
    ws = ref["pencil_%s_w" % fluid]
    want = ref["pencil_%s_%s_%s_flux" % (fluid, recon, solver)]
    lo, hi = R.PENCIL_NG, ws.shape[1] - R.PENCIL_NG
    for d in (1, 2, 3):
        for p, f in _oracle_pencils(fluid, recon, solver, d, ws, rmeta["gamma"], rmeta["pencil"]["c_h_" + fluid]):
            _bits(f[lo:hi + 1], want[p, lo:hi + 1], "%s %s %s dir %d pencil %d" % (fluid, recon, solver, d, p))


def test_scales_are_the_plain_numpy_ones(ref, rmeta):
    """the stored scales are those of reference_families (rounded DOWN to single precision), never anything wider"""
    for key, m in rmeta["riemann"].items():
        s = R.riemann_scale(m["fluid"], ref[key + "_wl"].astype(np.float64), ref[key + "_wr"].astype(np.float64), 1,
                            rmeta["gamma"], m["c_h"])
        assert np.array_equal(ref[key + "_scale"], R.floor32(s)) and np.all(ref[key + "_scale"].astype(np.float64) <= s)
    for fluid, recon, solver in R.PENCIL_COMBOS:
        for p, w in enumerate(ref["pencil_%s_w" % fluid]):
            s = R.pencil_scale(fluid, w, recon, rmeta["gamma"], rmeta["pencil"]["c_h_" + fluid])
            assert np.array_equal(ref["pencil_%s_%s_%s_scale" % (fluid, recon, solver)][p], R.floor32(s))


# ---- CPU, live: fresh inputs through the binary ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_bin():
    path = O.build_ref() or O.ref_binary()          # (a binary that travelled here with the tree serves as well)
    if path is None:
        pytest.skip("the reference tree is absent (APK_REFERENCE_SRC, default %s): oracle/_ref/ref_vectors cannot be "
                    "built; the stored vectors above were checked without it" % O.REF_SRC_DEFAULT)
    return path


@pytest.mark.parametrize("method", R.RECONS)
def test_live_oracle_equals_reference_reconstruction(ref_bin, method):
    rng = np.random.default_rng(1000 + R.RECONS.index(method))
    n = 0
    for fam in R.RECON_FAMILIES:
        q = R.recon_family(fam, N_LIVE, rng)
        for dx in (0.1, 1e-3):
            for pos in ((0, 1) if method == "limo3" else (1,)):       # LimO3 with and without its positivity fallback
                ql, qr = O.recon_many(method, q, dx=dx, n=(0 if pos else 1))
                rl, rr = R.ref_recon(method, q, dx, pos)
                _bits(ql, rl, "%s %s dx %g pos %d ql" % (method, fam, dx, pos))
                _bits(qr, rr, "%s %s dx %g pos %d qr" % (method, fam, dx, pos))
                n += q.shape[0]
            if method not in ("weno3", "limo3"):
                break                                                  # the others do not see dx
    print("live recon %s: %d stencils equal in every bit" % (method, n))


@pytest.mark.parametrize("fluid,solver", [(f, s) for f in ("euler", "glmmhd") for s in R.SOLVERS[f]])
def test_live_oracle_equals_reference_riemann(ref_bin, fluid, solver):
    rng = np.random.default_rng(2000 + 10 * (fluid == "glmmhd") + R.SOLVERS[fluid].index(solver))
    n = nonfinite = 0
    for fam in R.RIEMANN_FAMILIES[fluid]:
        for d in (1, 2, 3):
            wl, wr, c_h = R.riemann_family(fluid, fam, N_LIVE, rng)
            wl, wr = R.rotate(wl, d), R.rotate(wr, d)
            for ch in (LIVE_C_H if (fluid == "glmmhd" and fam != "cgs") else (c_h,)):
                want = R.ref_riemann(fluid, solver, d, wl, wr, R.GAMMA, ch)
                _bits(O.riemann_many(fluid, solver, d, wl, wr, R.GAMMA, ch), want, "%s %s %s dir %d c_h %g" % (fluid, solver, fam, d, ch))
                n += wl.shape[0]
                nonfinite += int((~np.isfinite(want)).sum())
    assert nonfinite == 0
    print("live riemann %s %s: %d pairs equal in every bit" % (fluid, solver, n))


@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_live_oracle_equals_reference_cons_to_prim(ref_bin, fluid):
    rng = np.random.default_rng(3000 + (fluid == "glmmhd"))
    n = 0
    for regime in R.C2P_REGIMES:
        eos, u = R.c2p_family(fluid, regime, N_LIVE, rng)
        ra, rw = R.ref_c2p(fluid, u, R.GAMMA, 1, **eos)
        ua, w = _oracle_c2p(fluid, u, eos, R.GAMMA, 1)
        _bits(ua, ra, "%s %s (cons)" % (fluid, regime))
        _bits(w, rw, "%s %s (prim)" % (fluid, regime))
        n += u.shape[0]
    print("live c2p %s: %d states equal in every bit" % (fluid, n))


def test_live_oracle_equals_reference_wave_speeds(ref_bin):
    rng = np.random.default_rng(4000)
    lib = O.load()
    x = np.empty((N_LIVE, 5))
    x[:, 0] = 10.0 ** rng.uniform(-27, 2, N_LIVE)
    x[:, 1] = 10.0 ** rng.uniform(-13, 2, N_LIVE)
    x[:, 2:] = 10.0 ** rng.uniform(-7, 1, (N_LIVE, 3)) * np.where(rng.uniform(size=(N_LIVE, 3)) < 0.3, 0.0, 1.0)
    out = O.ref_run(["speeds", N_LIVE, R.GAMMA], x).reshape(2, N_LIVE)
    cs = np.array([lib.orc_sound_speed(R.GAMMA, a[0], a[1]) for a in x])
    cf = np.array([lib.orc_fast_speed(R.GAMMA, *a) for a in x])
    _bits(cs, out[0], "SoundSpeed")
    _bits(cf, out[1], "FastMagnetosonicSpeed")


@pytest.mark.parametrize("fluid,recon,solver", R.PENCIL_COMBOS)
def test_live_oracle_equals_reference_pencils(ref_bin, fluid, recon, solver):
    rng = np.random.default_rng(5000 + R.PENCIL_COMBOS.index((fluid, recon, solver)))
    c_h = 2.0 if fluid == "glmmhd" else 0.0
    ws = np.array([R.pencil(fluid, kind, rng) for kind in ("smooth", "jumps")])
    lo, hi = R.PENCIL_NG, ws.shape[1] - R.PENCIL_NG
    for d in (1, 2, 3):
        want = [R.ref_pencil(fluid, recon, solver, d, w, R.GAMMA, c_h, R.PENCIL_DX) for w in ws]
        for p, f in _oracle_pencils(fluid, recon, solver, d, ws, R.GAMMA, c_h):
            _bits(f[lo:hi + 1], want[p][lo:hi + 1], "%s %s %s dir %d pencil %d" % (fluid, recon, solver, d, p))


# ---- GPU: both builds against the stored values -------------------------------------------------------------------------------
def _compare(got, want, scale, strict, what, table=None, family=None):
    """strict: every bit.  product: |got - want| <= 1e-12 scale per entry (an entry whose scale is 0 must be equal);
    records and prints the worst err / scale"""
    if strict:
        _bits(got, want, what)
        return
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), what + ": non-finite entries differ"
    err = np.abs(got - want)
    scale = np.asarray(scale, dtype=np.float64)
    pos = scale > 0.0
    worst = float(np.max(err[pos] / scale[pos], initial=0.0))
    if table is not None:
        table[family] = max(table.get(family, 0.0), worst)
    print("product build, %s: worst err/scale %.3e" % (what, worst))
    assert np.all(err[~pos] == 0.0), "%s: %d entries of scale 0 differ" % (what, int((err[~pos] != 0).sum()))
    bad = np.argwhere(err > PRODUCT_TOL * scale)
    assert bad.size == 0, "%s: %d entries beyond 1e-12 x scale, worst err/scale %.3e, first at %s: got %r want %r scale %r" % (
        what, len(bad), worst, bad[0], got[tuple(bad[0])], want[tuple(bad[0])], scale[tuple(bad[0])])


def _pairs_block(wl, wr, d, ng):
    """donor-cell block with the pairs (already rotated for direction d) along d: interior cells 2c, 2c + 1 hold
    (wl, wr) of case c; two cells wide in the other directions; ghost zones repeat the nearest interior cell"""
    n, nv = wl.shape
    nx = [2, 2, 2]
    nx[d - 1] = 2 * n
    N = [m + 2 * ng for m in nx]
    line = np.empty((nv, N[d - 1]))
    line[:, ng:ng + 2 * n:2] = wl.T
    line[:, ng + 1:ng + 2 * n:2] = wr.T
    line[:, :ng] = line[:, ng:ng + 1]
    line[:, -ng:] = line[:, -ng - 1:-ng]
    shape = [1, 1, 1]
    shape[3 - d] = N[d - 1]
    w = np.zeros((1, nv, N[2], N[1], N[0]))
    w[0] = line.reshape((nv,) + tuple(shape))
    return tuple(nx), w


def _gpu_pair_fluxes(ctx, fluid, solver, d, wl, wr, gamma, c_h):
    """fluxes [n][nv] (as x1 cases) of the x1 pairs wl, wr solved along direction d by the donor-cell flux kernel"""
    from athenapk_amd import hydro
    ng = 2
    nx, w = _pairs_block(R.rotate(wl, d), R.rotate(wr, d), d, ng)
    md = hydro.MeshData(ctx, nx, ng, R.NV[fluid], dx=(0.1, 0.1, 0.1), prim=w)
    hydro.CalculateFluxes(md, fluid, "dc", solver, hydro.L.make_eos(gamma), c_h, tight=(solver == "llf"))
    f = md.flux_host(d - 1)[0]
    f = (f[:, ng, ng, :], f[:, ng, :, ng], f[:, :, ng, ng])[d - 1]                # the line along d through (ng, ng)
    return R.unrotate(f[:, ng + 1:ng + 1 + 2 * wl.shape[0]:2].T, d)               # lower d-face of the cells holding wr


def _riemann_groups(ref, rmeta, gold, emeta, fluid, solver):
    """[(name, gamma, c_h, wl, wr, want, scale, [(family, slice)])]: the crafted cases of this solver, and its stored
    random pairs grouped by c_h (one block per group and direction)"""
    groups = []
    idx = [n for n, c in enumerate(emeta["riemann"]) if c["fluid"] == fluid and c["riemann"] == solver]
    nv, c = R.NV[fluid], rmeta["crafted"]
    if idx:
        wl = np.array([gold["riemann_%02d_wl_dir1" % n] for n in idx])
        wr = np.array([gold["riemann_%02d_wr_dir1" % n] for n in idx])
        want = {d: R.unrotate(ref["crafted_riemann_flux"][idx, d - 1, :nv], d) for d in (1, 2, 3)}
        groups.append(("crafted", c["gamma"], c["c_h"], wl, wr, want, R.riemann_scale(fluid, wl, wr, 1, c["gamma"], c["c_h"]),
                       [("crafted", slice(0, len(idx)))]))
    by_ch = {}
    for key, m in rmeta["riemann"].items():
        if m["fluid"] == fluid and solver in m["solvers"]:
            by_ch.setdefault(m["c_h"], []).append((key, m))
    for c_h, items in sorted(by_ch.items()):
        wl = np.concatenate([ref[k + "_wl"].astype(np.float64) for k, _ in items])
        wr = np.concatenate([ref[k + "_wr"].astype(np.float64) for k, _ in items])
        f1 = np.concatenate([ref["%s_%s_flux" % (k, solver)] for k, _ in items])
        sc = np.concatenate([ref[k + "_scale"].astype(np.float64) for k, _ in items])
        fams, at = [], 0
        for k, m in items:
            fams.append((m["family"], slice(at, at + m["n"])))
            at += m["n"]
        groups.append(("c_h=%g" % c_h, rmeta["gamma"], c_h, wl, wr, {d: f1 for d in (1, 2, 3)}, sc, fams))
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("fluid,solver", [(f, s) for f in ("euler", "glmmhd") for s in R.SOLVERS[f]])
def test_hip_riemann_solvers_against_reference_values(request, ref, rmeta, gold, emeta, fluid, solver, strict):
    ctx = request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")
    groups = _riemann_groups(ref, rmeta, gold, emeta, fluid, solver)
    assert groups
    table = {}
    for name, gamma, c_h, wl, wr, want, scale, fams in groups:
        for d in (1, 2, 3):
            got = _gpu_pair_fluxes(ctx, fluid, solver, d, wl, wr, gamma, c_h)
            for fam, sl in fams:
                _compare(got[sl], want[d][sl], scale[sl], strict, "%s %s %s dir %d" % (fluid, solver, fam, d), table, fam)
    if not strict:
        print("TABLE riemann %s %s: %s" % (fluid, solver, " ".join("%s=%.2e" % kv for kv in table.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("fluid,recon,solver", R.PENCIL_COMBOS)
def test_hip_flux_kernels_against_reference_pencils(request, ref, rmeta, fluid, recon, solver, strict):
    from athenapk_amd import hydro
    ctx = request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")
    ws = ref["pencil_%s_w" % fluid]
    want = ref["pencil_%s_%s_%s_flux" % (fluid, recon, solver)]
    scale = ref["pencil_%s_%s_%s_scale" % (fluid, recon, solver)].astype(np.float64)
    ng, c_h = R.PENCIL_NG, rmeta["pencil"]["c_h_" + fluid]
    lo, hi = ng, ws.shape[1] - ng
    table = {}
    for d in (1, 2, 3):
        nx, w = R.pencil_block(list(ws), d)
        md = hydro.MeshData(ctx, nx, ng, R.NV[fluid], dx=(R.PENCIL_DX,) * 3, prim=w)
        hydro.CalculateFluxes(md, fluid, recon, solver, hydro.L.make_eos(rmeta["gamma"]), c_h)
        for p, f in R.pencil_block_faces(md.flux_host(d - 1)[0], d, len(ws)):
            kind = rmeta["pencil"]["kinds"][p]
            _compare(f[lo:hi + 1], want[p, lo:hi + 1], scale[p, lo:hi + 1], strict,
                     "%s %s %s dir %d %s" % (fluid, recon, solver, d, kind), table, kind)
    if not strict:
        print("TABLE pencil %s %s %s: %s" % (fluid, recon, solver, " ".join("%s=%.2e" % kv for kv in table.items())))


def _gpu_c2p(ctx, fluid, u, eos_kw, gamma, nscalars):
    """(u after floors, w) [n][nvar] of the rows u as the interior cells of one block (ghosts repeat the first row)"""
    from athenapk_amd import hydro
    n, nvar = u.shape
    ng = 2
    cons = np.empty((1, nvar, 1, 1, n + 2 * ng))
    cons[0, :, 0, 0, :] = u[0][:, None]
    cons[0, :, 0, 0, ng:ng + n] = u.T
    md = hydro.MeshData(ctx, (n, 1, 1), ng, R.NV[fluid], nscalars=nscalars, cons=cons, prim=np.zeros_like(cons), with_flux=False)
    hydro.ConservedToPrimitive(md, fluid, hydro.L.make_eos(gamma, **eos_kw))
    ua, w = md.cons_host()[0, :, 0, 0, ng:ng + n].T, md.prim_host()[0, :, 0, 0, ng:ng + n].T
    ctx.poll_flags()                                   # floored negative states latch the unphysical-state flag: clear it
    return ua, w


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_hip_cons_to_prim_against_reference_values(request, ref, rmeta, gold, emeta, fluid, strict):
    ctx = request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")
    table = {}
    for key, m in rmeta["c2p"].items():
        if m["fluid"] != fluid:
            continue
        ua, w = _gpu_c2p(ctx, fluid, ref[key + "_u"], m["eos"], rmeta["gamma"], m["nscalars"])
        sc = ref[key + "_scale"].astype(np.float64)
        _compare(w, ref[key + "_w"], sc[1], strict, key + " (prim)", table, m["regime"])
        _compare(ua, ref[key + "_u_after"], sc[0], strict, key + " (cons)", table, m["regime"])
    if fluid == "glmmhd":
        g = rmeta["crafted"]["gamma"]
        for n, case in enumerate(emeta["c2p"]):
            u = gold["c2p_%02d_u" % n][None]
            ua, w = _gpu_c2p(ctx, fluid, u, case["eos"], g, 0)
            sc = R.c2p_scale(fluid, np.concatenate([u, [[0.0]]], axis=1), np.concatenate([ref["crafted_c2p_u_after"][n][None], [[0.0]]], axis=1),
                             None, g)[:, :, :9]
            _compare(w, ref["crafted_c2p_w"][n][None], sc[1], strict, case["label"] + " (prim)", table, "crafted")
            _compare(ua, ref["crafted_c2p_u_after"][n][None], sc[0], strict, case["label"] + " (cons)", table, "crafted")
    if not strict:
        print("TABLE c2p %s: %s" % (fluid, " ".join("%s=%.2e" % kv for kv in table.items())))


# ---- GPU, live: fresh pairs, expected values from the binary if it travelled -----------------------------------------------
def _travelled_binary():
    path = O.ref_binary()
    if path is None:
        pytest.skip("oracle/_ref/ref_vectors is not here (it is built only where the reference tree is, and is not committed)")
    try:
        r = subprocess.run([path, "speeds", "0", "1.4"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=20)
    except OSError as e:
        pytest.skip("oracle/_ref/ref_vectors does not start here: %s" % e)
    if r.returncode != 0:
        pytest.skip("oracle/_ref/ref_vectors does not run here: exit %d" % r.returncode)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
def test_live_hip_riemann_solvers_against_the_reference_binary(request, fluid, strict):
    _travelled_binary()
    ctx = request.getfixturevalue("gpu_ctx_strict" if strict else "gpu_ctx_fast")
    rng = np.random.default_rng(6000 + (fluid == "glmmhd"))
    fams = R.RIEMANN_FAMILIES[fluid]
    per = 4096 // len(fams)
    table = {}
    for fam in fams:
        wl, wr, c_h = R.riemann_family(fluid, fam, per + (4096 - per * len(fams) if fam == fams[0] else 0), rng)
        scale = R.riemann_scale(fluid, wl, wr, 1, R.GAMMA, c_h)
        for i, solver in enumerate(R.SOLVERS[fluid]):
            d = 1 + (i + fams.index(fam)) % 3
            want = R.unrotate(R.ref_riemann(fluid, solver, d, R.rotate(wl, d), R.rotate(wr, d), R.GAMMA, c_h), d)
            got = _gpu_pair_fluxes(ctx, fluid, solver, d, wl, wr, R.GAMMA, c_h)
            _compare(got, want, scale, strict, "live %s %s %s dir %d" % (fluid, solver, fam, d), table, solver + "/" + fam)
    if not strict:
        print("TABLE live %s: %s" % (fluid, " ".join("%s=%.2e" % kv for kv in table.items())))
