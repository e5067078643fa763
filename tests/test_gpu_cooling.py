"""Tabular cooling on the GPU: the kernels against the numpy restatement (tests/cooling_reference.py) in both builds,
the reference's cluster_tabular_cooling pins restated through the native driver (uniform gas, 1 Gyr, power-law table,
analytic e(t)), and the driver's time-step limit, temperature floor and decomposition invariance with cooling on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cooling_cases as C  # noqa: E402
import cooling_reference as R  # noqa: E402
from cooling_cases import GAMMA, HE, MBAR_GM1_OVER_KB, NB, NG, ROOT, SCHURE, T_FLOOR, U  # noqa: E402
from golden import make_cooling_tables as M  # noqa: E402

pytestmark = pytest.mark.gpu

NX = C.NX_ONE_WG
_rows, _restated, _edge_temps, _params, _src = C.rows, C.restated, C.edge_temps, C.params, C.src


def _loglam_tol(T, e):
    """relative tolerance of a cooling rate: 2e-14, or one unit in the last place of its log10 lambda (about -145 in
    these units: 6.5e-14 relative) -- log10 is not correctly rounded on either side, so a table lookup may land one
    ulp apart"""
    ll = T.log_lambda(e)
    return 2e-14 if ll is None else max(2e-14, 1.5 * math.log(10.0) * np.spacing(abs(ll)))


@pytest.mark.parametrize("build", ["strict", "fast"])
@pytest.mark.parametrize("table", ["schure", "power_law"])
def test_dedt_pointwise(gpu_ctx_strict, gpu_ctx_fast, build, table):
    from athenapk_amd import hydro
    ctx = gpu_ctx_strict if build == "strict" else gpu_ctx_fast
    rows = _rows(table)
    T = _restated(rows)
    rng = np.random.default_rng(7)
    e = list(10 ** rng.uniform(3.0, 9.0, 2000) / MBAR_GM1_OVER_KB) + _edge_temps(T, rows[0])
    rho = 147.7557589278723 * 10 ** rng.uniform(-2, 2, len(e))
    tab = hydro.TabularCooling(ctx, rows[0], rows[1], _params())
    got, valid = tab.DeDt(np.array(e), rho)
    for n, (ei, ri) in enumerate(zip(e, rho)):
        want, v = T.dedt(ei, ri)
        assert valid[n] == v, (n, ei)
        if want == 0.0:
            assert got[n] == 0.0, (n, ei, got[n])
        else:
            assert abs(got[n] - want) <= _loglam_tol(T, ei) * abs(want), (n, ei, got[n], want)
    assert (~valid).sum() == 2  # e < 0 and NaN


SRC_CASES = [(integ, fluid, table) for integ in ("rk12", "rk45", "townsend") for fluid in ("euler", "glmmhd")
             for table in ("schure", "power_law")]


def _check_src_term(ctx_strict, ctx_fast, integ, fluid, table, nx):
    rows = _rows(table)
    kw = dict(T_floor=T_FLOOR, d_e_tol=0.0, max_iter=8)
    T = _restated(rows, integ, **kw)
    u, prim, mask = C.state(fluid, T, rows[0], len(integ) + 3 * len(fluid) + len(table), nx)
    mhd = fluid == "glmmhd"
    dt = 2e-4
    got, _, _ = _src(ctx_strict, fluid, rows, _params(integ, **kw), u, prim, dt, nx)
    fast, _, _ = _src(ctx_fast, fluid, rows, _params(integ, **kw), u, prim, dt, nx)
    for b in range(NB):
        want = R.src_term(T, integ, u[b], mhd, dt, mask)
        assert np.array_equal(np.delete(got[b], 4, axis=0), np.delete(u[b], 4, axis=0), equal_nan=True)
        assert np.array_equal(np.delete(fast[b], 4, axis=0), np.delete(u[b], 4, axis=0), equal_nan=True)
        assert np.array_equal(got[b][4][~mask], u[b][4][~mask])  # ghost cells are not cooled
        g, w, f = got[b][4][mask], want[4][mask], fast[b][4][mask]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isnan(f), np.isnan(w))
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= 1e-12 * np.abs(w[ok])), np.max(np.abs(g[ok] - w[ok]) / np.abs(w[ok]))
        assert np.all(np.abs(f[ok] - g[ok]) <= 1e-12 * np.abs(g[ok])), np.max(np.abs(f[ok] - g[ok]) / np.abs(g[ok]))
        cooled = (w != u[b][4][mask]) & ok
        assert cooled.sum() >= mask.sum() // 2, "the source cooled too few cells to test anything"


@pytest.mark.parametrize("integ,fluid,table", SRC_CASES)
def test_src_term_against_restatement(gpu_ctx_strict, gpu_ctx_fast, integ, fluid, table):
    """rk12 / rk45 with d_e_tol = 0 (a fixed number of substeps) and Townsend: per cell within 1e-12 of the
    restatement (parity build), the product build within 1e-12 of the parity build; nothing but IEN changes"""
    _check_src_term(gpu_ctx_strict, gpu_ctx_fast, integ, fluid, table, NX)


@pytest.mark.parametrize("integ,fluid,table", [("townsend", "euler", "schure"), ("townsend", "glmmhd", "power_law"),
                                               ("rk45", "euler", "power_law"), ("rk45", "glmmhd", "schure")])
def test_src_term_two_workgroups(gpu_ctx_strict, gpu_ctx_fast, integ, fluid, table):
    """the same comparison on 360 interior cells: a second, partial workgroup, and the boundary between the blocks
    (flat index 180) inside the first"""
    _check_src_term(gpu_ctx_strict, gpu_ctx_fast, integ, fluid, table, C.NX_TWO_WG)


def _check_timestep(ctx, table, nx, fastest=None):
    """fastest: (block, k, j, i) of an interior cell that is given the shortest cooling time by far"""
    from athenapk_amd import hydro
    rows = _rows(table)
    T = _restated(rows, T_floor=T_FLOOR)
    u, prim, mask = C.state("euler", T, rows[0], 5, nx)
    prim[0, 4, NG, NG, NG] = 1.0  # (the e < 0 row holds a valid state in the primitives)
    prim[0, 4, NG, NG, NG + 1] = 1.0
    if fastest is not None:
        others = min(R.cooling_timestep(T, prim[b], mask) for b in range(NB))
        b, k, j, i = fastest
        assert mask[k, j, i]
        rho = 147.7557589278723e3  # (a hundred times the densest of the random cells, near the peak of the rates)
        prim[b, 0, k, j, i], prim[b, 4, k, j, i] = rho, rho * (10 ** 5.3 / MBAR_GM1_OVER_KB) * (GAMMA - 1.0)
        only = np.zeros_like(mask)
        only[k, j, i] = True
        assert R.cooling_timestep(T, prim[b], only) < 0.5 * others
    md = hydro.MeshData(ctx, nx, NG, 5, dx=(0.1, 0.1, 0.1), nblocks=NB, cons=u, prim=prim)
    want = min(R.cooling_timestep(T, prim[b], mask) for b in range(NB))
    tab = hydro.TabularCooling(ctx, rows[0], rows[1], _params(T_floor=T_FLOOR))
    got = tab.EstimateTimeStep(md)
    tol = 2e-14 + 1.5 * math.log(10.0) * np.spacing(max(abs(v) for v in T.log_lambdas))
    assert abs(got - want) <= tol * want, (got, want)
    return T, prim, mask, md, rows


@pytest.mark.parametrize("build", ["strict", "fast"])
@pytest.mark.parametrize("table", ["schure", "power_law"])
def test_cooling_timestep(gpu_ctx_strict, gpu_ctx_fast, build, table):
    from athenapk_amd import hydro
    ctx = gpu_ctx_strict if build == "strict" else gpu_ctx_fast
    T, prim, mask, md, rows = _check_timestep(ctx, table, NX)
    for cfl, expect in ((0.0, np.finfo(np.float64).max), (-1.0, np.finfo(np.float64).max), (float("nan"), math.inf),
                        (math.inf, math.inf)):
        t2 = hydro.TabularCooling(ctx, rows[0], rows[1], _params(T_floor=T_FLOOR, cfl=cfl))
        assert t2.EstimateTimeStep(md) == expect
        T.cfl = cfl
        assert R.cooling_timestep(T, prim[0], mask) == expect


@pytest.mark.parametrize("build", ["strict", "fast"])
@pytest.mark.parametrize("table", ["schure", "power_law"])
@pytest.mark.parametrize("where", ["random", "flat_359", "flat_180"])
def test_cooling_timestep_two_workgroups(gpu_ctx_strict, gpu_ctx_fast, build, table, where):
    """the minimum over 360 interior cells, wherever it falls, then in the last cell of block 1 (flat index 359, in
    the partial second workgroup) and in the first cell of block 1 (flat index 180, inside the first workgroup)"""
    nx = C.NX_TWO_WG
    cell = {"random": None, "flat_359": (1, NG + nx[2] - 1, NG + nx[1] - 1, NG + nx[0] - 1),
            "flat_180": (1, NG, NG, NG)}[where]
    _check_timestep(gpu_ctx_strict if build == "strict" else gpu_ctx_fast, table, nx, cell)


# ---- the native driver -------------------------------------------------------------------------------------------


def _sim(overrides, strict=True, deck="cooling"):
    from athenapk_amd import decks, driver
    s = driver.Simulation(decks.load(deck), ["cooling/table_filename=" + SCHURE] + list(overrides), strict=strict)
    return s.initialize()


def _e_of(prim):
    return prim[4] / (prim[0] * (GAMMA - 1.0))


def _run_uniform(table_path, integ, max_iter, d_e_tol, cfl=1e100):
    s = _sim(["cooling/table_filename=" + table_path, "cooling/integrator=%s" % integ, "cooling/max_iter=%d" % max_iter,
              "cooling/d_e_tol=%r" % d_e_tol, "cooling/cfl=%r" % cfl, "parthenon/time/tlim=1.0"])
    p0 = s.gather("prim")
    s.run()
    assert abs(s.time - 1.0) <= 1e-14
    return p0, s.gather("prim"), s.ncycle


def test_cluster_tabular_cooling_pins(tmp_path):
    """tst/regression/test_suites/cluster_tabular_cooling restated: 1 Gyr of a uniform gas on the power-law table"""
    path = M.write_power_law_table(str(tmp_path / "exponential.cooling"))
    rho0, p0 = 147.7557589278723, 1.5454368403867562
    e0 = p0 / (rho0 * (GAMMA - 1.0))
    analytic = R.analytic_e(U, HE, GAMMA, (M.LOG_TEMP0, M.LOG_TEMP1), (M.LOG_LAMBDA0, M.LOG_LAMBDA1), e0, 1.0)(rho0)
    assert analytic < 0.6 * e0  # (the gas does cool)

    def check(p_init, p_final):
        for v in range(4):  # density and velocity untouched, to machine precision
            want = rho0 if v == 0 else 0.0
            assert np.max(np.abs(p_init[v] - want)) <= 1e-14 * max(abs(want), 1.0)
            assert np.max(np.abs(p_final[v] - want)) <= 1e-14 * max(abs(want), 1.0)
        assert abs(np.mean(_e_of(p_init)) - e0) <= 1e-14 * e0
        return abs(np.mean(_e_of(p_final)) - analytic) / analytic

    iters = (4, 10, 25, 50)
    for integ, order in (("rk12", 2), ("rk45", 5)):
        errs = []
        for mi in iters:
            a, b, _ = _run_uniform(path, integ, mi, 0.0)
            errs.append(check(a, b))
        slope = np.polyfit(np.log(iters), np.log(errs), 1)[0]
        assert slope <= -order + 0.1, (integ, errs, slope)
    for integ, tol in (("rk12", 1e-4), ("rk45", 1e-10)):
        a, b, _ = _run_uniform(path, integ, 50, 1e-14)
        err = check(a, b)
        assert err < tol, (integ, err)
    a, b, _ = _run_uniform(path, "townsend", 1, 1e-14)
    err = check(a, b)
    assert err < 1e-14, err


def test_cooling_limits_the_time_step():
    s = _sim([])  # cooling/cfl = 0.1, Schure table
    rows = _rows("schure")
    T = _restated(rows, cfl=0.1)
    hyp = _sim(["cooling/enable_cooling=none"])
    for c in range(3):
        if c:
            s.step()
            hyp = None
        w = s.gather("prim")
        mask = np.ones(w.shape[1:], dtype=bool)
        want = R.cooling_timestep(T, w, mask)
        if hyp is not None:
            assert want < hyp.dt  # the cooling limit binds
        tol = 2e-14 + 1.5 * math.log(10.0) * np.spacing(max(abs(v) for v in T.log_lambdas))
        assert abs(s.dt - want) <= tol * want, (c, s.dt, want)


@pytest.mark.parametrize("integ", ["rk12", "rk45", "townsend"])
def test_gas_ends_at_the_temperature_floor(integ):
    s = _sim(["hydro/Tfloor=%r" % T_FLOOR, "cooling/integrator=" + integ, "cooling/cfl=0",
              "parthenon/time/tlim=0.01"])
    s.run()
    w = s.gather("prim")
    temp = _e_of(w) * MBAR_GM1_OVER_KB
    assert np.all(np.abs(temp - T_FLOOR) <= 1e-12 * T_FLOOR), (integ, temp.min(), temp.max())


SOD = ["parthenon/mesh/nx1=32", "parthenon/mesh/x1min=-2.0", "parthenon/mesh/x1max=2.0", "problem/sod/pres_l=15.0",
       "problem/sod/rho_r=30.0", "problem/sod/pres_r=0.2", "cooling/integrator=rk45"]
NCYC = 4


def _rank_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from athenapk_amd import decks, driver
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        s = driver.Simulation(decks.load("cooling"), ["cooling/table_filename=" + SCHURE] + SOD, rank=rank,
                              nranks=world, strict=True)
        s.initialize()
        dts = [s.dt]
        for _ in range(NCYC):
            s.step()
            dts.append(s.dt)
        blocks = {s.block_gid(lb)[0]: s.read_block(lb, "cons") for lb in range(s.info.nblocks_local)}
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), time=s.time, dts=np.array(dts),
                 **{"b%d" % g: a for g, a in blocks.items()})
        s.close()
    finally:
        dist.destroy_process_group()


def test_decomposition_invariance(tmp_path):
    from _spawn import spawn
    one = _sim(SOD)
    dts = [one.dt]
    u0 = one.gather()
    for _ in range(NCYC):
        one.step()
        dts.append(one.dt)
    assert not np.array_equal(one.gather()[4], u0[4])
    blocks = {one.block_gid(lb)[0]: one.read_block(lb, "cons") for lb in range(one.info.nblocks_local)}
    spawn(_rank_worker, lambda port: (2, port, str(tmp_path)), nprocs=2)
    ng = one.info.ng
    for r in range(2):
        z = np.load(tmp_path / ("rank%d.npz" % r))
        assert float(z["time"]) == one.time
        assert np.array_equal(z["dts"], np.array(dts)), (z["dts"], dts)
        for key in z.files:
            if key.startswith("b"):
                g = int(key[1:])
                a, b = z[key][:, ng:-ng, ng:-ng, ng:-ng], blocks[g][:, ng:-ng, ng:-ng, ng:-ng]
                assert np.array_equal(a, b), "block %d differs on 2 ranks" % g
