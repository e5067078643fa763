"""Generates tests/golden/reference_physics.npz + reference_physics.json: inputs with the outputs that the REFERENCE's own
compiled physics headers give for them (oracle/_ref/ref_physics, built by oracle.build_ref() from the recipe in
oracle/ref/ -- needs the reference tree), and the deck entries every case was run with.  The fixture is data only.

  units      every public accessor of Units in three unit systems (json)
  gravity    g_from_r per deck of reference_physics_cases.GRAVITY_DECKS: each component alone, all three, smoothing 0 and
             positive, keys set and keys default (two unit systems); and on the equidistant meshes the host's
             he_sphere_profile evaluates its own g and K on
  entropy    K_from_r, keys set and default
  jet        SimCartToJetCylCoords and JetCylToSimCartVector through JetCoordsFactory::CreateJetCoords(time), and r, h at
             the cell centres of the GPU tests' block for the aligned axis
  tower      PotentialInSimCart, FieldInSimCart, DensityFromSimCart for li and donut, aligned and tilted axis; and for the
             GPU tests' 8 x 6 x 5 block (reference_physics_cases.block_centres): the potential at field TOWER_FIELD on the
             centres one cell beyond the block on every side, the field at unit strength and the density at unit density
             on the interior centres
  dedt       CoolingTableObj::DeDt on the committed schure.cooling_1.0Z
  rk12/rk45  one Step and OptimalStep each
  limiters   vanleer, minmod, mc, lim2, lim4
  adddensity AddDensityToConsAtFixedVel / AtFixedVelTemp

Every stored input is one on which the binary neither aborts nor returns a non-finite value (asserted here); the two
DeDt cases e < 0 and e = NaN return (0, invalid).

    python tests/golden/make_reference_physics.py          (deterministic: rewrites the files byte for byte)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from oracle import oracle as O  # noqa: E402
import reference_physics_cases as P  # noqa: E402
from make_reference_vectors import write_npz  # noqa: E402

SEED = 20261021


def finite(*arrays):
    for a in arrays:
        assert np.all(np.isfinite(a)), "the reference returned a non-finite value"


def main():
    if O.build_ref(which="ref_physics") is None:
        raise SystemExit("no reference tree (APK_REFERENCE_SRC): the expected values come from its compiled headers")
    rng = np.random.default_rng(SEED)
    out, meta = {}, {"seed": SEED, "gamma": P.GAMMA}

    meta["units"] = {name: {"keys": keys, "values": P.ref_units(keys)} for name, keys in P.UNITS.items()}
    for u in meta["units"].values():
        finite(np.array(list(u["values"].values())))

    meta["gravity"] = {}
    for name, (keys, smoothing, r_s) in P.GRAVITY_DECKS.items():
        r = P.gravity_radii(name, rng, P.GRAVITY_RANDOM[name])
        g = P.ref_gravity(name, r)
        finite(g)
        out["gravity_%s_r" % name], out["gravity_%s_g" % name] = r, g
        meta["gravity"][name] = {"keys": keys, "smoothing": smoothing, "n": len(r)}
        if name in P.HOST_DECKS:
            for m, mesh in enumerate(P.HOST_MESHES):
                out["gravity_host_%s_%d_g" % (name, m)] = P.ref_gravity(name, P.host_mesh_radii(mesh))
                finite(out["gravity_host_%s_%d_g" % (name, m)])
    meta["host_meshes"] = [list(m) for m in P.HOST_MESHES]

    meta["entropy"] = {}
    for name, (keys, r_k) in P.ENTROPY_DECKS.items():
        r = P.entropy_radii(name, rng, P.ENTROPY_RANDOM[name])
        out["entropy_%s_r" % name], out["entropy_%s_K" % name] = r, P.ref_entropy(name, r)
        finite(out["entropy_%s_K" % name])
        meta["entropy"][name] = {"keys": keys, "n": len(r)}
        if name != "defaults_cgs":
            for m, mesh in enumerate(P.HOST_MESHES):
                out["entropy_host_%s_%d_K" % (name, m)] = P.ref_entropy(name, P.host_mesh_radii(mesh))

    meta["jet"] = {}
    for name, case in P.JET_CASES.items():
        p, v = P.jet_inputs(name, rng, P.JET_RANDOM[name])
        cyl, sim = P.ref_jet(case, p, v)
        finite(cyl, sim)
        out["jet_%s_p" % name], out["jet_%s_v" % name], out["jet_%s_cyl" % name], out["jet_%s_sim" % name] = p, v, cyl, sim
        meta["jet"][name] = {"theta": case[0], "phi0": case[1], "phi_dot": case[2], "time": case[3], "n": len(p)}
    pts = P.block_points()
    cyl, _ = P.ref_jet(P.JET_CASES["aligned"], pts, np.zeros((len(pts), 5)))
    out["jet_block_aligned_cyl"] = cyl

    meta["tower"] = {"field": P.TOWER_FIELD, "density": P.TOWER_DENSITY, "decks": P.TOWER_DECKS,
                     "jets": {k: {"keys": v[0], "time": v[1]} for k, v in P.TOWER_JETS.items()},
                     "block": {"nx": list(P.BLOCK_NX), "ng": P.BLOCK_NG, "dx": P.BLOCK_DX, "xmin": list(P.BLOCK_XMIN), "jet": "block"}}
    for pot in P.TOWER_DECKS:
        for jet in ("aligned", "tilted"):
            p = P.tower_points(jet, rng, P.TOWER_RANDOM)
            a, b, rho = P.ref_tower(pot, jet, p)
            finite(a, b, rho)
            key = "tower_%s_%s" % (pot, jet)
            out[key + "_p"], out[key + "_A"], out[key + "_B"], out[key + "_rho"] = p, a, b, rho
        a, _, _ = P.ref_tower(pot, "block", P.block_points(1))
        _, b1, rho1 = P.ref_tower(pot, "block", P.block_points(0), field=1.0, density=1.0)
        finite(a, b1, rho1)
        out["tower_block_%s_A" % pot], out["tower_block_%s_B1" % pot], out["tower_block_%s_rho1" % pot] = a, b1, rho1
        if pot == "donut":
            assert 0 < np.count_nonzero(a.any(axis=1)) < len(a), "the block lies wholly inside or outside the donut"

    pts = P.block_points(1, P.EDGE_NX, P.EDGE_XMIN)
    a, _, _ = P.ref_tower("donut", "aligned", pts)
    finite(a)
    out["tower_edge_donut_A"] = a
    on = np.isin(np.abs(pts[:, 2]), (P.TOWER_OFFSET, P.TOWER_OFFSET + P.TOWER_THICKNESS))
    assert on.sum() == 4 * 36 and np.all(a[on, 2] != 0), "the block has no centres on the donut's two edges"
    meta["tower"]["edge_block"] = {"nx": list(P.EDGE_NX), "xmin": list(P.EDGE_XMIN), "jet": "aligned"}

    c = P.mbar_gm1_over_kb(meta["units"]["hse"]["values"])
    x, labels = P.dedt_inputs(c, rng, 512)
    assert P.ref_keep(P.ref_dedt, x).all(), "a DeDt input aborts the reference"
    d, valid = P.ref_dedt(x)
    finite(d)
    assert list(np.flatnonzero(~valid)) == [labels.index("negative"), labels.index("nan")]
    for must in ("first_node", "last_node", "just_above", "last_interval"):
        assert must in labels, must
    out["dedt_x"], out["dedt_out"], out["dedt_valid"] = x, d, valid
    meta["cooling"] = {"keys": P.COOLING_DECK, "table": P.SCHURE_REL.replace(os.sep, "/"), "labels": labels[:labels.index("random")],
                       "mbar_gm1_over_kb": c, "n": len(x)}

    for stepper in ("rk12", "rk45"):
        x, opt = P.rk_inputs(c, lambda a: P.ref_dedt(a)[0], rng, 256)
        keep = P.ref_keep(lambda a, b: P.ref_rkstep(stepper, a, b), x, opt)
        x, opt = x[keep], opt[keep]
        yh, yl, valid, best = P.ref_rkstep(stepper, x, opt)
        finite(yh, yl, best)
        assert 10 <= np.count_nonzero(~valid) <= len(x) // 2, "too few or too many steps go negative"
        out[stepper + "_x"], out[stepper + "_opt"] = x, opt
        out[stepper + "_yh"], out[stepper + "_yl"], out[stepper + "_valid"], out[stepper + "_optimal"] = yh, yl, valid, best
        meta[stepper] = {"n": len(x), "dropped": int((~keep).sum())}

    q = P.limiter_inputs(rng, 512)
    out["limiters_q"], out["limiters_out"] = q, P.ref_limiters(q)
    finite(out["limiters_out"])

    rows = P.adddensity_inputs(rng, 256)
    out["adddensity_rows"] = rows
    for kind in ("fixedvel", "fixedveltemp"):
        out["adddensity_" + kind] = P.ref_adddensity(kind, rows)
        finite(out["adddensity_" + kind])

    # ---- what the GPU tests of the source terms need on their own blocks (reference_physics_cases: the states are seeded)
    u, w = P.agn_block_state()
    rows = P.rows_of(P.AGN_DELTA, P.interior(u), P.interior(w))
    out["agn_block_rows"], out["agn_block_fixedvel"] = rows, P.ref_adddensity("fixedvel", rows)
    u, w = P.trig_state()
    box = (slice(None),) + P.TRIG_BOX
    rows = P.rows_of(-w[box][0] / P.TRIG_T_ACC * P.TRIG_DT, u[box], w[box])
    out["trig_rows"], out["trig_fixedveltemp"] = rows, P.ref_adddensity("fixedveltemp", rows)
    r = P.grav_radii()
    g = np.zeros(r.size)
    pos = r.ravel() != 0
    assert (~pos).sum() == 1
    g[pos] = P.ref_gravity(P.GRAV_DECK, r.ravel()[pos])
    out["gravity_src_r"], out["gravity_src_g"] = r, g.reshape(r.shape)
    finite(out["agn_block_fixedvel"], out["trig_fixedveltemp"], g)

    write_npz(os.path.join(HERE, "reference_physics.npz"), out)
    with open(os.path.join(HERE, "reference_physics.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    size = sum(os.path.getsize(os.path.join(HERE, n)) for n in ("reference_physics.npz", "reference_physics.json"))
    cap = os.path.getsize(os.path.join(HERE, "reference_vectors.npz"))
    print("wrote %d arrays, %d bytes (cap %d: the size of reference_vectors.npz)" % (len(out), size, cap))
    print("rk12 dropped %d, rk45 dropped %d rows on which the reference's table lookup aborts" % (meta["rk12"]["dropped"], meta["rk45"]["dropped"]))
    assert size < cap


if __name__ == "__main__":
    main()
