# tools/cooling_prof.py -- the tabular cooling source term on 8 x 128^3 Euler blocks with the Schure table: temperatures
# spread smoothly over 1e4 - 1e8 K, density of the cooling deck, dt = the cooling-limited step (cooling/cfl = 0.1).
# Prints one JSON line per integrator: ms per call (median of >= 3 timed regions of >= 50 ms, the state restored
# before every call, outside the timed span), the memory floor, and the mean / per-wave maximum substeps of a sample of
# waves (restated on the host).
#   python tools/cooling_prof.py
#   rocprofv3 --kernel-trace --stats --output-format csv -d prof -o cool -- python tools/cooling_prof.py --quick
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cooling_reference as R  # noqa: E402
from athenapk_amd import hydro  # noqa: E402
from athenapk_amd import lib as L  # noqa: E402

QUICK = "--quick" in sys.argv
N, NB, NG = (64 if QUICK else 128), 8, 2
GAMMA, HE, RHO = 1.6666666666666667, 0.25, 147.7557589278723
U = R.CLUSTER_UNITS
MBAR_OVER_KB = R.composition(U, HE)[3]
MBAR_GM1 = MBAR_OVER_KB * (GAMMA - 1.0)
rows = R.read_table(os.path.join(ROOT, "tests", "golden", "schure.cooling_1.0Z"))

torch.cuda.set_device(0)
ctx = hydro.Context(strict=False)
nt = N + 2 * NG
x = (np.arange(nt) - NG + 0.5) / N
X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
cons = np.zeros((NB, 5, nt, nt, nt))
for b in range(NB):
    # log T from 4 to 8, smooth in space (a wave's 64 lanes see neighbouring temperatures)
    logT = 6.0 + 2.0 * np.sin(2 * np.pi * (X + 0.13 * b)) * np.cos(2 * np.pi * Y) * np.cos(np.pi * (Z - 0.5))
    logT = logT.transpose(2, 1, 0)  # [k, j, i] with i along x
    cons[b, 0] = RHO
    cons[b, 4] = RHO * 10 ** logT / MBAR_GM1
prim = cons.copy()
prim[:, 4] = cons[:, 4] * (GAMMA - 1.0)
md = hydro.MeshData(ctx, (N, N, N), NG, 5, dx=(1.0 / N,) * 3, nblocks=NB, cons=cons, prim=prim, with_flux=False)
saved = md.cons.clone()

dt_tab = hydro.TabularCooling(ctx, rows[0], rows[1], L.make_cooling_params(
    "rk12", cfl=0.1, lambda_units=U.lambda_units(), gamma=GAMMA, mbar_over_kb=MBAR_OVER_KB, He_mass_fraction=HE, mh=U.mh))
dt = dt_tab.EstimateTimeStep(md)


def timed(tab, region_ms=50.0, regions=3):
    st, sp = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    meds = []
    for _ in range(regions):
        tot, calls = 0.0, 0
        while tot < region_ms:
            md.cons.copy_(saved)
            st.record()
            tab.SrcTerm(md, "euler", dt)  # (synchronises: reads the failure flags)
            sp.record()
            torch.cuda.synchronize()
            tot += st.elapsed_time(sp)
            calls += 1
        meds.append(tot / calls)
    return float(np.median(meds)), meds


def substeps(integ, T, nwaves=48):
    """mean and per-wave maximum of the accepted substeps over a sample of waves (64 consecutive cells of a row)"""
    rng = np.random.default_rng(1)
    mean, wmax = [], []
    for _ in range(nwaves):
        b, k, j = rng.integers(NB), NG + rng.integers(N), NG + rng.integers(N)
        i0 = NG + 64 * rng.integers(max(1, N // 64))
        counts = []
        for i in range(i0, i0 + 64):
            e0 = cons[b, 4, k, j, i] / RHO
            R.subcycle_cell(T, integ, RHO, e0, dt, counts)
        mean.append(np.mean(counts))
        wmax.append(max(counts))
    return float(np.mean(mean)), float(np.mean(wmax))


for integ in ("rk12", "rk45", "townsend"):
    p = L.make_cooling_params(integ, d_e_tol=1e-8, lambda_units=U.lambda_units(), gamma=GAMMA,
                              mbar_over_kb=MBAR_OVER_KB, He_mass_fraction=HE, mh=U.mh)
    tab = hydro.TabularCooling(ctx, rows[0], rows[1], p)
    ms, regions = timed(tab, region_ms=10.0 if QUICK else 50.0)
    cells = NB * N ** 3
    out = dict(integrator=integ, cells=cells, dt=dt, ms_per_call=ms, regions_ms=regions,
               floor_bytes=48 * cells, floor_GBps=48 * cells / ms / 1e6)
    if integ != "townsend" and not QUICK:
        T = R.Table(rows[0], rows[1], U.lambda_units(), GAMMA, MBAR_OVER_KB, HE, U.mh, d_e_tol=1e-8, max_iter=100)
        out["substeps_mean"], out["substeps_wave_max_mean"] = substeps(integ, T)
    print(json.dumps(out), flush=True)
tab = None
dt_tab = None
md = None
ctx.close()
