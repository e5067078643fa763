"""What the cooling tests share, with and without a GPU: the gas constants, the two tables, the restated table object,
the random pack of blocks with its row of edge cases, and the adaptive-subcycling cases with their per-cell tolerance."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cooling_reference as R  # noqa: E402
from golden import make_cooling_tables as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHURE = os.path.join(ROOT, "tests", "golden", "schure.cooling_1.0Z")
GAMMA, HE = 1.6666666666666667, 0.25
U = R.CLUSTER_UNITS
MBAR_OVER_KB = R.composition(U, HE)[3]
MBAR_GM1_OVER_KB = MBAR_OVER_KB * (GAMMA - 1.0)
NG, NB = 2, 2
NX_ONE_WG = (8, 4, 3)   # 192 interior cells: one partial 256-lane workgroup
NX_TWO_WG = (12, 5, 3)  # 360: two workgroups, the second partial; block 1 starts at flat index 180, inside the first
T_FLOOR = 2e4


def rows(name):
    if name == "schure":
        return R.read_table(SCHURE)
    return M.power_law_table()


def restated(table_rows, integrator="rk12", **kw):
    lt, ll = table_rows
    return R.Table(lt, ll, U.lambda_units(1.0), GAMMA, MBAR_OVER_KB, HE, U.mh, townsend=integrator == "townsend", **kw)


def params(integrator="rk12", **kw):
    """lib.CoolingParams of the same gas"""
    from athenapk_amd import lib as L
    return L.make_cooling_params(integrator=integrator, lambda_units=U.lambda_units(1.0), gamma=GAMMA,
                                 mbar_over_kb=MBAR_OVER_KB, He_mass_fraction=HE, mh=U.mh, **kw)


def src(ctx, fluid, table_rows, cooling_params, u, prim, dt, nx):
    """TabularCooling::SrcTerm on the pack (u, prim) of `state`: the cooled cons on the host, the pack, the table"""
    from athenapk_amd import hydro
    md = hydro.MeshData(ctx, nx, NG, u.shape[1], dx=(0.1, 0.1, 0.1), nblocks=NB, cons=u, prim=prim)
    tab = hydro.TabularCooling(ctx, table_rows[0], table_rows[1], cooling_params)
    tab.SrcTerm(md, fluid, dt)
    return md.cons_host(), md, tab


def edge_temps(T, lt):
    """the edge rows: e < 0, NaN, below the table, below T_floor, above the table, and table nodes whose lookup the
    restatement's REQUIRE accepts"""
    e = [-1.0e-3, float("nan"), 10 ** 3.5 / MBAR_GM1_OVER_KB, 1.5e4 / MBAR_GM1_OVER_KB, 10 ** 9.2 / MBAR_GM1_OVER_KB]
    for k in range(3, len(lt) - 1, max(1, len(lt) // 7)):
        ek = 10 ** lt[k] / MBAR_GM1_OVER_KB
        x = math.log10(MBAR_GM1_OVER_KB * ek)
        i = min(int((x - T.log_temp_start) / T.d_log_temp), T.n - 2)
        lti = T.log_temp_start + T.d_log_temp * i
        if lti <= x <= lti + T.d_log_temp:
            e.append(ek)
    return e


def state(fluid, T, lt, seed, nx):
    """conserved and primitive arrays of NB blocks [NB, nvar, nk, nj, ni] and the interior mask of one block; row
    (k, j) = (0, 0) of block 0 holds the edge cases"""
    mhd = fluid == "glmmhd"
    nvar = 9 if mhd else 5
    ni, nj, nk = nx[0] + 2 * NG, nx[1] + 2 * NG, nx[2] + 2 * NG
    rng = np.random.default_rng(seed)
    shape = (NB, nk, nj, ni)
    rho = 147.7557589278723 * 10 ** rng.uniform(-1, 1, shape)
    e = 10 ** rng.uniform(3.5, 8.5, shape) / MBAR_GM1_OVER_KB
    v = [0.05 * rng.standard_normal(shape) for _ in range(3)]
    b = [0.02 * rng.standard_normal(shape) for _ in range(3)] if mhd else [np.zeros(shape)] * 3
    edge = edge_temps(T, lt)[: nx[0]]
    for i, ei in enumerate(edge):
        e[0, NG, NG, NG + i] = ei
    u = np.zeros((NB, nvar) + shape[1:])
    u[:, 0] = rho
    for d in range(3):
        u[:, 1 + d] = rho * v[d]
    kin = 0.5 * rho * (v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    mag = 0.5 * (b[0] ** 2 + b[1] ** 2 + b[2] ** 2)
    u[:, 4] = rho * e + kin + mag
    if mhd:
        for d in range(3):
            u[:, 5 + d] = b[d]
        u[:, 8] = 0.01 * rng.standard_normal(shape)
    # e < 0: the stored total energy below the kinetic + magnetic part
    u[0, 4, NG, NG, NG] = kin[0, NG, NG, NG] + mag[0, NG, NG, NG] - 1e-3 * rho[0, NG, NG, NG]
    prim = u.copy()
    for d in range(3):
        prim[:, 1 + d] = v[d]
    prim[:, 4] = (u[:, 4] - kin - mag) * (GAMMA - 1.0)
    mask = np.zeros(shape[1:], dtype=bool)
    mask[NG:NG + nx[2], NG:NG + nx[1], NG:NG + nx[0]] = True
    return u, prim, mask


# ---- adaptive subcycling (d_e_tol > 0) ---------------------------------------------------------------------------

# (d_e_tol, max_iter, dt): the default (rejections, clamps, growth, 1 to 100 substeps per cell); invalid stages, retries
# and jumps to the floor; nearly every cell collapsing to the floor
REGIMES = [(1e-8, 100, 2e-4), (1e-4, 16, 2e-2), (1e-6, 25, 1.0)]
ADAPTIVE_CASES = [(integ, fluid, table, regime) for integ in ("rk12", "rk45") for fluid in ("euler", "glmmhd")
                  for table in ("schure", "power_law") for regime in range(len(REGIMES))]
ADAPTIVE_SEED = 5
PROBE_DELTA, PROBE_SEEDS = 1e-13, (11, 12, 13, 14, 15, 16)


def cells(u, mhd, mask):
    """(rho, e, IEN) of the interior cells of one block, in flat order (k, j, i): the kernels' lane order"""
    rho, e = R.specific_internal_e(u, mhd)
    return rho[mask], e[mask], u[4][mask]


def adaptive_restated(integ, fluid, table, regime, probes=True):
    """the restatement of one adaptive case on the NX_TWO_WG pack: a dict with the table rows, the keywords of the
    cooling parameters, dt, the state (u, prim, mask), and over the interior cells of all blocks in flat order the
    initial IEN and the initial and final specific energy (ien, e0, a), the restated IEN (want: IEN + rho * (a - e0) as src_term does), the
    accepted substeps (counts), the event counters of the whole pack (events) and (probes) tol_cell:

        tol_cell = max(1e-12, 4 * max over six probes of |a_probe - a| / |a|)

    a_probe: a with every cooling rate multiplied by 1 + 1e-13 * xi, xi uniform in [-1, 1].  1e-13 is the difference
    the suite already allows between two log10 / pow implementations (one unit in the last place of log10 lambda near
    -145 is 6.5e-14 of lambda), 1e-12 is the fixed-substep test's bound, and 4 is headroom over the largest of six
    samples.  The tolerance is the restatement's own conditioning; nothing of the kernel enters it."""
    d_e_tol, max_iter, dt = REGIMES[regime]
    table_rows = rows(table)
    kw = dict(T_floor=T_FLOOR, d_e_tol=d_e_tol, max_iter=max_iter)
    T = restated(table_rows, integ, **kw)
    u, prim, mask = state(fluid, T, table_rows[0], ADAPTIVE_SEED, NX_TWO_WG)
    mhd = fluid == "glmmhd"
    rho, e0, ien = (np.concatenate(v) for v in zip(*(cells(u[b], mhd, mask) for b in range(NB))))
    counts, events = [], {}
    a = np.array([R.subcycle_cell(T, integ, float(r), float(e), dt, counts, events) for r, e in zip(rho, e0)])
    out = dict(rows=table_rows, kw=kw, dt=dt, u=u, prim=prim, mask=mask, T=T, rho=rho, e0=e0, ien=ien, a=a,
               want=ien + rho * (a - e0), counts=np.array(counts), events=events)
    if probes:
        dev = np.zeros(a.shape)
        for seed in PROBE_SEEDS:
            T.rate_noise(PROBE_DELTA, seed)
            p = np.array([R.subcycle_cell(T, integ, float(r), float(e), dt) for r, e in zip(rho, e0)])
            with np.errstate(invalid="ignore"):
                dev = np.fmax(dev, np.abs(p - a) / np.abs(a))
        T.rate_noise(0.0)
        out["tol"] = np.maximum(1e-12, 4.0 * dev)
    return out
