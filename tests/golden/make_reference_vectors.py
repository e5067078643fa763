"""Generates tests/golden/reference_vectors.npz + reference_vectors.json: inputs with the outputs that the REFERENCE's
own compiled headers give for them (oracle/_ref/ref_vectors, built by oracle.build_ref() from the recipe in
oracle/ref/ -- needs the reference tree), and for every case and variable a physical scale computed in plain numpy
(tests/reference_families.py).  The fixture is data only.

  crafted   the 40 stencils of edge_cases.npz through all six reconstructions, its 31 Riemann cases x 3 directions and
            its ConsToPrim cases, re-derived from the reference; ASSERTED equal to what edge_cases.npz stores (which
            came from the oracle)
  riemann   256 random state pairs per family (subsonic, supersonic, B = 0, Bx = 0, cgs-scaled) for euler HLLE / HLLC
            and glmmhd HLLE / HLLD.  The inputs are rounded to single precision (and stored so) to keep the fixture
            within the size of edge_cases.npz; the outputs are full doubles.  Stored for a sweep along x1 only: the
            generator asserts that the reference's results for x2 and x3 are the exact permutation
  c2p       both fluids, floors off and each floor / ceiling acting, one passive scalar
  pencils   2 lines of 70 + 2 x 3 cells (one smooth, one with jumps) per fluid through Reconstruct<recon, DIR> + Solve
            for recon in plm, ppm, wenoz, weno3, limo3 x (euler hllc, glmmhd hlld): face fluxes, stored for x1 only
            under the same assertion

    python tests/golden/make_reference_vectors.py          (deterministic: rewrites the files byte for byte)
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as O  # noqa: E402
import reference_families as R  # noqa: E402

SEED = 20261018
N_RIEMANN, N_C2P = 256, 16


def write_npz(path, arrays):
    """a deterministic .npz: fixed entry times, so that regenerating gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    if O.build_ref() is None:
        raise SystemExit("no reference tree (APK_REFERENCE_SRC): the expected values come from its compiled headers")
    gold = np.load(os.path.join(HERE, "edge_cases.npz"))
    with open(os.path.join(HERE, "edge_cases.json")) as f:
        emeta = json.load(f)
    g, ch = emeta["gamma"], emeta["c_h"]
    out = {}
    meta = {"gamma": R.GAMMA, "seed": SEED, "crafted": {"gamma": g, "c_h": ch, "stencil_dx": 0.1, "stencil_positivity": 1},
            "riemann": {}, "c2p": {}, "pencil": {"nx": R.PENCIL_NX, "ng": R.PENCIL_NG, "dx": R.PENCIL_DX, "kinds": ["smooth", "jumps"]}}

    # ---- crafted sets, re-derived from the reference and compared with edge_cases.npz
    q = gold["ppm_q"]
    for m in R.RECONS:
        ql, qr = R.ref_recon(m, q, 0.1, 1)
        out["stencil_%s_ql" % m], out["stencil_%s_qr" % m] = ql, qr
        if m != "dc":
            assert np.array_equal(ql, gold["%s_ql" % m], equal_nan=True) and np.array_equal(qr, gold["%s_qr" % m], equal_nan=True), m
        else:
            assert np.array_equal(ql, q[:, 2]) and np.array_equal(qr, q[:, 2])
    cf = np.zeros((len(emeta["riemann"]), 3, 9))
    for n, c in enumerate(emeta["riemann"]):
        nv = R.NV[c["fluid"]]
        for d in (1, 2, 3):
            f = R.ref_riemann(c["fluid"], c["riemann"], d, gold["riemann_%02d_wl_dir%d" % (n, d)], gold["riemann_%02d_wr_dir%d" % (n, d)], g, ch)[0]
            assert np.array_equal(f, gold["riemann_%02d_flux_dir%d" % (n, d)], equal_nan=True), (c["label"], d)
            assert np.all(np.isfinite(f)), c["label"]
            cf[n, d - 1, :nv] = f
    out["crafted_riemann_flux"] = cf
    cu, cw = [], []
    for n, c in enumerate(emeta["c2p"]):
        ua, w = R.ref_c2p("glmmhd", gold["c2p_%02d_u" % n][None], g, 0, **c["eos"])
        assert np.array_equal(ua[0], gold["c2p_%02d_u_after" % n]) and np.array_equal(w[0], gold["c2p_%02d_w" % n]), c["label"]
        cu.append(ua[0])
        cw.append(w[0])
    out["crafted_c2p_u_after"], out["crafted_c2p_w"] = np.array(cu), np.array(cw)
    print("crafted: %d stencils x %d methods, %d riemann cases x 3, %d c2p cases: the reference equals edge_cases.npz"
          % (q.shape[0], len(R.RECONS), len(emeta["riemann"]), len(emeta["c2p"])))

    # ---- random Riemann pairs
    rng = np.random.default_rng(SEED)
    gpr = [np.inf, 0.0]
    for fluid in ("euler", "glmmhd"):
        for fam in R.RIEMANN_FAMILIES[fluid]:
            wl, wr, c_h = R.riemann_family(fluid, fam, N_RIEMANN, rng)
            wl32, wr32 = wl.astype(np.float32), wr.astype(np.float32)
            wl, wr = wl32.astype(np.float64), wr32.astype(np.float64)
            key = "riemann_%s_%s" % (fluid, fam)
            out[key + "_wl"], out[key + "_wr"] = wl32, wr32
            out[key + "_scale"] = R.floor32(R.riemann_scale(fluid, wl, wr, 1, R.GAMMA, c_h))
            for w in (wl, wr):
                x = R.GAMMA * w[:, 4] * w[:, 0]
                gpr = [min(gpr[0], x.min()), max(gpr[1], x.max())]
            for solver in R.SOLVERS[fluid]:
                if solver == "llf":
                    continue
                f1 = R.ref_riemann(fluid, solver, 1, wl, wr, R.GAMMA, c_h)
                assert np.all(np.isfinite(f1)), (fluid, fam, solver)
                for d in (2, 3):
                    fd = R.ref_riemann(fluid, solver, d, R.rotate(wl, d), R.rotate(wr, d), R.GAMMA, c_h)
                    assert np.array_equal(R.unrotate(fd, d), f1), "direction %d is not the permutation of x1: %s" % (d, key)
                out["%s_%s_flux" % (key, solver)] = f1
            meta["riemann"][key] = {"fluid": fluid, "family": fam, "c_h": c_h, "n": N_RIEMANN,
                                    "solvers": [s for s in R.SOLVERS[fluid] if s != "llf"]}
    meta["gamma_p_rho_range"] = gpr

    # ---- ConsToPrim
    for fluid in ("euler", "glmmhd"):
        for regime in R.C2P_REGIMES:
            eos, u = R.c2p_family(fluid, regime, N_C2P, rng)
            ua, w = R.ref_c2p(fluid, u, R.GAMMA, 1, **eos)
            key = "c2p_%s_%s" % (fluid, regime)
            out[key + "_u"], out[key + "_u_after"], out[key + "_w"] = u, ua, w
            out[key + "_scale"] = R.floor32(R.c2p_scale(fluid, u, ua, w, R.GAMMA))
            changed = int(np.any(ua != u, axis=1).sum())
            if regime == "floors_off":
                assert changed == 0
            else:
                assert 2 <= changed <= N_C2P - 2, (key, changed)          # the floor / ceiling acts on some, not on all
            meta["c2p"][key] = {"fluid": fluid, "regime": regime, "eos": eos, "n": N_C2P, "nscalars": 1, "changed": changed}

    # ---- pencils
    for fluid in ("euler", "glmmhd"):
        c_h = 2.0 if fluid == "glmmhd" else 0.0
        ws = np.array([R.pencil(fluid, kind, rng) for kind in meta["pencil"]["kinds"]])
        out["pencil_%s_w" % fluid] = ws
        for f_, rc, rs in R.PENCIL_COMBOS:
            if f_ != fluid:
                continue
            fl, sc = [], []
            for w in ws:
                f1 = R.ref_pencil(fluid, rc, rs, 1, w, R.GAMMA, c_h, R.PENCIL_DX)
                lo, hi = R.PENCIL_NG, w.shape[0] - R.PENCIL_NG
                assert np.all(np.isfinite(f1[lo:hi + 1])) and np.all(f1[lo:hi + 1, 0] != 0.0)
                for d in (2, 3):
                    fd = R.ref_pencil(fluid, rc, rs, d, w, R.GAMMA, c_h, R.PENCIL_DX)
                    assert np.array_equal(fd, f1), "direction %d is not the permutation of x1: %s %s %s" % (d, fluid, rc, rs)
                fl.append(f1)
                sc.append(R.pencil_scale(fluid, w, rc, R.GAMMA, c_h))
            key = "pencil_%s_%s_%s" % (fluid, rc, rs)
            out[key + "_flux"], out[key + "_scale"] = np.array(fl), R.floor32(np.array(sc))
        meta["pencil"]["c_h_" + fluid] = c_h

    write_npz(os.path.join(HERE, "reference_vectors.npz"), out)
    with open(os.path.join(HERE, "reference_vectors.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    size = sum(os.path.getsize(os.path.join(HERE, n)) for n in ("reference_vectors.npz", "reference_vectors.json"))
    cap = os.path.getsize(os.path.join(HERE, "edge_cases.npz"))
    print("wrote %d arrays, %d bytes (cap %d: the size of edge_cases.npz)" % (len(out), size, cap))
    assert size <= cap
    print("gamma p rho over the Riemann families: %.3e .. %.3e" % tuple(gpr))


if __name__ == "__main__":
    main()
