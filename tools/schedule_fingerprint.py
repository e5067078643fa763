#!/usr/bin/env python3
"""Schedule fingerprint of the stage loop: for a set of small configurations that between them take every stage form
(single-march donor cell, two-kernel, trial + fallback, flux arrays; prim-free, direct-neighbour, one-layer and x1-direct
exchanges; forcing; refined meshes), run a few cycles in the parity build and print what the host driver did -- its
counters, the launches per kernel-timing slot -- and what it computed: time, dt and a SHA-256 of the conserved state.

A change to host code that is meant to leave the schedule alone must leave this output byte-identical:

    python3 tools/schedule_fingerprint.py > after.txt
    python3 tools/schedule_fingerprint.py --lib-dir DIR > before.txt    # DIR: libapk_amd_strict.so of the other commit
    cmp before.txt after.txt
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bc(kind):
    return ["parthenon/mesh/%sx%d_bc=%s" % (io, d, kind) for d in (1, 2, 3) for io in "io"]


def _mesh(nx, mb):
    return ["parthenon/mesh/nx%d=%d" % (d + 1, nx[d]) for d in range(3)] + ["parthenon/meshblock/nx%d=%d" % (d + 1, mb[d]) for d in range(3)]


def _scheme(fluid, integ, recon, riemann, ng):
    return ["hydro/fluid=%s" % fluid, "parthenon/time/integrator=%s" % integ, "hydro/reconstruction=%s" % recon,
            "hydro/riemann=%s" % riemann, "parthenon/mesh/nghost=%d" % ng]


B8 = _mesh((32, 32, 32), (16, 16, 16))  # 2 x 2 x 2 blocks of 16^3
REH = ["apk_amd/rehearse_remote_faces=true"]
HYDRO_VL2 = B8 + _scheme("euler", "vl2", "plm", "hllc", 2)
BLAST_FOFC = B8 + ["hydro/first_order_flux_correct=true", "problem/blast/radius_outer=0.1", "problem/blast/radius_inner=0.1",
                   "problem/blast/pressure_ratio=1e10", "problem/blast/density_ratio=100.0", "hydro/fluid=euler",
                   "hydro/reconstruction=wenoz", "hydro/riemann=hllc", "parthenon/mesh/nghost=3", "parthenon/time/cfl=0.45"]
WALLS = _mesh((32, 32, 32), (16, 16, 16)) + ["parthenon/mesh/ix2_bc=reflecting", "parthenon/mesh/ox2_bc=reflecting"]
AMR_BLAST = ["parthenon/meshblock/nx%d=16" % d for d in (1, 2, 3)] + [
    "parthenon/mesh/nghost=4", "hydro/fluid=glmmhd", "hydro/riemann=hlld", "hydro/reconstruction=ppm",
    "parthenon/time/integrator=vl2", "parthenon/mesh/check_refine_interval=2", "parthenon/mesh/derefine_count=2",
    "problem/blast/pressure_ambient=1.0", "problem/blast/pressure_ratio=1000", "problem/blast/radius_outer=0.1",
    "problem/blast/radius_inner=0.05", "refinement/type=pressure_gradient", "refinement/threshold_pressure_gradient=0.5"]
SMR = ["parthenon/mesh/refinement=static"] + _mesh((32, 32, 32), (16, 16, 16)) + [
    "parthenon/static_refinement0/x%d%s=%s" % (d, m, v) for d in (1, 2, 3) for m, v in (("min", "-0.05"), ("max", "0.2"))] + [
    "parthenon/static_refinement0/level=1"] + _bc("periodic")
DIFF3 = _mesh((32, 16, 16), (16, 8, 8)) + ["parthenon/time/integrator=rk2", "hydro/reconstruction=plm",
                                            "diffusion/conduction=anisotropic", "diffusion/conduction_coeff=fixed",
                                            "diffusion/thermal_diff_coeff_code=0.2", "diffusion/viscosity=isotropic",
                                            "diffusion/viscosity_coeff=fixed", "diffusion/mom_diff_coeff_code=0.01",
                                            "diffusion/resistivity=ohmic", "diffusion/resistivity_coeff=fixed",
                                            "diffusion/ohm_diff_coeff_code=0.015"]
SCHURE = os.path.join(ROOT, "tests", "golden", "schure.cooling_1.0Z")

# name, deck, overrides, switches ({setter: value}, applied before initialize), cycles
CONFIGS = [("hydro_vl2_plm_hllc", "synthetic_mhd", HYDRO_VL2, {}, 4)]
for ovl in (1, 0):
    for x1 in (1, 0):
        CONFIGS.append(("hydro_vl2_rehearsed_overlap%d_x1direct%d" % (ovl, x1), "synthetic_mhd", HYDRO_VL2 + REH,
                        {"set_overlap": ovl, "set_x1_direct": x1}, 4))
CONFIGS += [
    ("hydro_rk2_plm_hlle_rehearsed", "synthetic_mhd", B8 + _scheme("euler", "rk2", "plm", "hlle", 2) + REH, {}, 4),
    ("hydro_rk3_plm_hlle_rehearsed", "synthetic_mhd", B8 + _scheme("euler", "rk3", "plm", "hlle", 2) + REH, {}, 4),
    ("hydro_rk3_density_floor", "synthetic_mhd", B8 + _scheme("euler", "rk3", "plm", "hlle", 2) + ["hydro/dfloor=0.9"], {}, 4),
    ("mhd_vl2_ppm_hlld_extended_dedner", "synthetic_mhd", B8 + ["hydro/glmmhd_source=dedner_extended"], {}, 4),
    ("mhd_2d_64sq_4_blocks", "orszag_tang", ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=32",
                                            "parthenon/meshblock/nx2=32"], {}, 4),
    ("sod_1d", "sod", _mesh((256, 1, 1), (128, 1, 1)), {}, 4),
    # (strong enough that some trial stages are rejected within these cycles: fofc_fallback_stages > 0)
    ("blast_fofc_vl2", "blast", BLAST_FOFC + ["parthenon/time/integrator=vl2"], {}, 30),
    ("blast_fofc_rk2", "blast", BLAST_FOFC + ["parthenon/time/integrator=rk2"], {}, 30),
    ("scalars_rk2", "synthetic_mhd", B8 + ["hydro/nscalars=2", "parthenon/time/integrator=rk2"], {}, 4),
]
for pf in (1, 0):
    CONFIGS.append(("turbulence_vl2_prim_free%d" % pf, "turbulence", B8, {"set_prim_free": pf}, 4))
    CONFIGS.append(("turbulence_rk3_wenoz_rehearsed_prim_free%d" % pf, "turbulence",
                    B8 + REH + ["parthenon/mesh/nghost=3", "parthenon/time/integrator=rk3", "hydro/reconstruction=wenoz",
                                "hydro/riemann=hlld"], {"set_prim_free": pf}, 4))
CONFIGS += [
    ("sod_vl2_outflow_and_walls", "sod", WALLS + ["parthenon/time/integrator=vl2"], {}, 4),
    ("sod_rk2_outflow_and_walls", "sod", WALLS + ["parthenon/time/integrator=rk2"], {}, 4),
]
for pf in (1, 0):
    CONFIGS.append(("amr_static_prim_free%d" % pf, "blast", SMR, {"set_prim_free": pf}, 4))
    CONFIGS.append(("amr_adaptive_prim_free%d" % pf, "blast_3d_amr", AMR_BLAST + _bc("periodic"), {"set_prim_free": pf}, 4))
CONFIGS += [
    ("amr_static_full_exchange", "blast", SMR, {"set_amr_full_exchange": 1}, 4),
    ("amr_adaptive_full_exchange", "blast_3d_amr", AMR_BLAST + _bc("periodic"), {"set_amr_full_exchange": 1}, 4),
    ("amr_adaptive_outflow", "blast_3d_amr", AMR_BLAST + _bc("outflow"), {}, 4),
    ("diffusion_unsplit", "synthetic_mhd", DIFF3 + ["diffusion/integrator=unsplit"], {}, 4),
    ("diffusion_rkl2", "synthetic_mhd", DIFF3 + ["diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=20"], {}, 4),
    ("cooling_tabular", "cooling", ["cooling/table_filename=" + SCHURE, "parthenon/mesh/nx1=32", "parthenon/mesh/x1min=-2.0",
                                    "parthenon/mesh/x1max=2.0", "problem/sod/pres_l=15.0", "problem/sod/rho_r=30.0",
                                    "problem/sod/pres_r=0.2", "cooling/integrator=rk45"], {}, 4),
]


def fingerprint(name, deck, overrides, switches, cycles):
    from athenapk_amd import decks, driver
    print("== %s" % name)
    try:  # (a deck the driver refuses is part of the fingerprint; anything that goes wrong later is not caught)
        s = driver.Simulation(decks.load(deck), overrides, strict=True)
        for setter, value in sorted(switches.items()):
            getattr(s, setter)(value)
        s.initialize()
    except driver.L.ApkError as e:
        print("refused: %s" % e)
        return
    s.kernel_timing(True)
    s.read_kernel_timing()
    for _ in range(cycles):
        s.step()
    launches = {k: v[1] for k, v in s.read_kernel_timing().items() if v[1]}
    print("cycles %d blocks %d" % (s.ncycle, s.refresh_info().nblocks_total))
    print("counters overlapped=%d skipped_local=%d thin=%d x1_direct=%d turb_dt_kicks=%d amr_c2p_skipped=%d fofc_fallback=%d "
          "prim_is_stale=%d" % (s.overlapped_exchanges, s.skipped_local_exchanges(), s.thin_exchanges(), s.x1_direct_exchanges(),
                                s.turb_dt_kicks(), s.amr_c2p_passes_skipped(), s.fofc_fallback_stages, int(s.prim_is_stale)))
    print("launches " + " ".join("%s=%d" % kv for kv in sorted(launches.items())))
    print("time %s dt %s" % (float(s.time).hex(), float(s.dt).hex()))
    h = hashlib.sha256()
    if name.startswith("amr_"):   # (refined meshes are read block by block, ghost zones included: the accessor completes them)
        for lb in range(s.refresh_info().nblocks_local):
            h.update(np.ascontiguousarray(s.read_block(lb)).tobytes())
    else:
        h.update(np.ascontiguousarray(s.gather()).tobytes())
    print("cons sha256 %s" % h.hexdigest())
    sys.stdout.flush()
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib-dir", help="load libapk_amd_strict.so from this directory (a build of another commit)")
    ap.add_argument("--only", help="comma-separated configuration names")
    ap.add_argument("--out", help="write the fingerprint to this file instead of standard output")
    a = ap.parse_args()
    if a.lib_dir:
        from athenapk_amd import lib as L
        d = os.path.abspath(a.lib_dir)
        L.lib_path = lambda strict=False: os.path.join(d, "libapk_amd_strict.so" if strict else "libapk_amd.so")
    only = set(a.only.split(",")) if a.only else None
    if a.out:
        sys.stdout = open(a.out, "w")
    for cfg in CONFIGS:
        if only is None or cfg[0] in only:
            fingerprint(*cfg)


if __name__ == "__main__":
    main()
