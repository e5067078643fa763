"""RKL2 super-time-stepping on the GPU: the array-path kernels and the fused sub-stage against the numpy restatement
(tests/sts_reference.py), and the native driver with diffusion/integrator = rkl2 -- fused against arrays, decomposition
invariance, the time step, conservation, zero coefficients, and the reference's regression pin (diffusion.py, rkl2 leg)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffusion_reference as R  # noqa: E402
import helpers as H  # noqa: E402
import sts_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {1: (40, 1, 1), 2: (18, 12, 1), 3: (12, 10, 8)}
DX = (0.1, 0.07, 0.13)
# (the table of tests/test_gpu_diffusion.py)
PROCESSES = {
    "cond_iso": dict(conduction="isotropic", kappa=0.7),
    "cond_aniso": dict(conduction="anisotropic", kappa=0.7),
    "visc": dict(viscosity="isotropic", nu=0.3),
    "ohm": dict(resistivity="ohmic", eta=0.45),
    "all": dict(conduction="anisotropic", kappa=0.7, viscosity="isotropic", nu=0.3, resistivity="ohmic", eta=0.45),
}
TAU, S_RKL = 0.013, 9


def _cfg(p):
    from athenapk_amd import lib as L
    return L.make_diff_cfg(conduction=p.get("conduction", "none"), kappa=p.get("kappa", 0.0), sat_phi=0.3,
                           viscosity=p.get("viscosity", "none"), nu=p.get("nu", 0.0),
                           resistivity=p.get("resistivity", "none"), eta=p.get("eta", 0.0))


def _ref_kw(p):
    kw = dict(p)
    kw["sat_prefac"] = 5.0 * 0.3
    return kw


def _fluid(p):
    return "glmmhd" if p.get("resistivity", "none") != "none" or p.get("conduction") == "anisotropic" else "euler"


class _Regs:
    """the four registers of a sub-stage with random contents, on the host and on the GPU; yjm1 carries prim and flux"""

    def __init__(self, ctx, fluid, nx, ng, seed, nblocks=2, row_pitch=None, prim=None, with_flux=True):
        import torch
        from athenapk_amd import hydro
        self.nx, self.ng = nx, ng
        self.ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
        if prim is None:
            prim = H.random_prim(fluid, nx, ng, seed=seed, kind="smooth", nblocks=nblocks)
        self.prim = prim
        rng = np.random.default_rng(seed + 1000)
        self.host = {k: rng.standard_normal(prim.shape) for k in ("y0", "yjm1", "yjm2", "my0")}
        nh = prim.shape[1]
        mk = lambda name, **kw: hydro.MeshData(ctx, nx, ng, nh, dx=DX, nblocks=nblocks, cons=self.host[name],
                                               row_pitch=row_pitch, **kw)
        self.yjm1 = mk("yjm1", prim=prim, with_flux=with_flux)
        self.y0, self.yjm2, self.my0 = (mk(n, with_flux=False) for n in ("y0", "yjm2", "my0"))
        self.flux = []
        for d in range(self.ndim if with_flux else 0):
            f = rng.standard_normal(prim.shape)
            self.yjm1.flux[d].copy_(torch.from_numpy(f).to(self.yjm1.flux[d].device))
            self.flux.append(f)

    def zero_flux(self):
        for d in range(self.ndim):
            self.yjm1.flux[d].zero_()

    def got(self):
        return {"yjm1": self.yjm1.cons_host(), "yjm2": self.yjm2.cons_host(), "my0": self.my0.cons_host()}

    def want(self):
        return {k: self.host[k].copy() for k in ("y0", "yjm1", "yjm2", "my0")}


def _interior(nx, ng):
    lo = [ng if n > 1 else 0 for n in nx]
    return (slice(None), slice(None)) + tuple(slice(lo[a], lo[a] + nx[a]) for a in (2, 1, 0))


def _compare(got, want, keys, exact, what):
    for k in keys:
        if exact:
            assert np.array_equal(got[k], want[k]), "%s %s: max |diff| %.3e" % (what, k, np.max(np.abs(got[k] - want[k])))
        else:
            scale = np.max(np.abs(want[k]))
            assert np.max(np.abs(got[k] - want[k])) <= 1e-12 * scale, (what, k, np.max(np.abs(got[k] - want[k])), scale)


@pytest.mark.parametrize("row_pitch", [None, "aligned"])
@pytest.mark.parametrize("fluid", ["euler", "glmmhd"])
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_array_path_kernels_strict_bitwise(gpu_ctx_strict, ndim, fluid, row_pitch):
    from athenapk_amd import hydro
    nx, ng = SHAPES[ndim], 2
    # FluxDivergence
    r = _Regs(gpu_ctx_strict, fluid, nx, ng, seed=7 * ndim + len(fluid), row_pitch=row_pitch)
    hydro.FluxDivergence(r.yjm1, r.my0)
    w = r.want()
    div = S.flux_divergence(r.flux + [None] * (3 - ndim), nx, ng, DX)
    w["my0"][_interior(nx, ng)] = div
    assert np.any(div != 0.0)
    _compare(r.got(), w, ("my0", "yjm1", "yjm2"), True, "FluxDivergence")
    # RKL2StepFirst
    r = _Regs(gpu_ctx_strict, fluid, nx, ng, seed=3 * ndim + 1, row_pitch=row_pitch)
    hydro.RKL2StepFirst(r.y0, r.yjm1, r.yjm2, r.my0, S_RKL, TAU)
    w = r.want()
    S.step_first(w["y0"], w["yjm1"], w["yjm2"], w["my0"], S_RKL, TAU, nx, ng)
    _compare(r.got(), w, ("yjm1", "yjm2", "my0"), True, "RKL2StepFirst")
    assert np.array_equal(r.y0.cons_host(), w["y0"])
    # RKL2StepOther
    r = _Regs(gpu_ctx_strict, fluid, nx, ng, seed=5 * ndim + 2, row_pitch=row_pitch)
    k = hydro.rkl2_coefficients(S_RKL, 4, strict=True)
    hydro.RKL2StepOther(r.y0, r.yjm1, r.yjm2, r.my0, k[0], k[1], k[2], k[3], TAU)
    w = r.want()
    S.step_other(w["y0"], w["yjm1"], w["yjm2"], w["my0"], S.flux_divergence(r.flux + [None] * (3 - ndim), nx, ng, DX),
                 S.coefficients(S_RKL, 4), TAU, nx, ng)
    _compare(r.got(), w, ("yjm1", "yjm2", "my0"), True, "RKL2StepOther")


def _array_substage(r, cfg, j):
    """the array path on the GPU: zeroed flux arrays, CalcDiffFluxes, FluxDivergence + RKL2StepFirst / RKL2StepOther"""
    from athenapk_amd import hydro
    r.zero_flux()
    hydro.CalcDiffFluxes(r.yjm1, cfg)
    if j == 1:
        hydro.FluxDivergence(r.yjm1, r.my0)
        hydro.RKL2StepFirst(r.y0, r.yjm1, r.yjm2, r.my0, S_RKL, TAU)
    else:
        k = hydro.rkl2_coefficients(S_RKL, j, strict=True)
        hydro.RKL2StepOther(r.y0, r.yjm1, r.yjm2, r.my0, k[0], k[1], k[2], k[3], TAU)


def _fused_case(ctx, name, ndim, j, exact, row_pitch=None, seed=0):
    from athenapk_amd import hydro
    p = PROCESSES[name]
    nx, ng = SHAPES[ndim], 2
    for fluid in sorted({_fluid(p), "glmmhd"}):
        sd = seed + 13 * ndim + len(name) + j
        fused = _Regs(ctx, fluid, nx, ng, seed=sd, row_pitch=row_pitch, with_flux=False)
        arrays = _Regs(ctx, fluid, nx, ng, seed=sd, row_pitch=row_pitch)
        hydro.RKL2SubstageFused(fused.y0, fused.yjm1, fused.yjm2, fused.my0, _cfg(p),
                                hydro.rkl2_coefficients(S_RKL, j, strict=True), TAU, first=(j == 1))
        _array_substage(arrays, _cfg(p), j)
        w = fused.want()
        S.substage(fused.prim, w["y0"], w["yjm1"], w["yjm2"], w["my0"], nx, ng, DX, S_RKL, j, TAU, **_ref_kw(p))
        assert not np.array_equal(w["yjm1"], fused.host["yjm1"])
        what = "%s %d-D %s j=%d" % (name, ndim, fluid, j)
        _compare(fused.got(), w, ("yjm1", "yjm2", "my0"), exact, what + " fused vs restatement")
        _compare(arrays.got(), w, ("yjm1", "yjm2", "my0"), exact, what + " arrays vs restatement")
        if exact:
            _compare(fused.got(), arrays.got(), ("yjm1", "yjm2", "my0"), True, what + " fused vs arrays")


CASES = [(name, ndim) for name in PROCESSES for ndim in (1, 2, 3)]


@pytest.mark.parametrize("j", [1, 4])
@pytest.mark.parametrize("name,ndim", CASES)
def test_fused_substage_strict_bitwise(gpu_ctx_strict, name, ndim, j):
    _fused_case(gpu_ctx_strict, name, ndim, j, exact=True)


@pytest.mark.parametrize("j", [1, 4])
def test_fused_substage_aligned_rows_bitwise(gpu_ctx_strict, j):
    _fused_case(gpu_ctx_strict, "all", 3, j, exact=True, row_pitch="aligned", seed=50)


@pytest.mark.parametrize("j", [1, 4])
@pytest.mark.parametrize("name,ndim", CASES)
def test_fused_substage_product_build_close(gpu_ctx_fast, name, ndim, j):
    _fused_case(gpu_ctx_fast, name, ndim, j, exact=False, seed=100)


@pytest.mark.parametrize("j", [1, 4])
def test_more_planes_than_one_launch_holds(gpu_ctx_strict, j):
    # 66 000 one-dimensional blocks: more (plane, block) pairs than a grid dimension holds (65 535)
    from athenapk_amd import hydro
    nb, nx, ng = 66000, (4, 1, 1), 1
    rng = np.random.default_rng(7)
    prim = rng.uniform(-1.0, 1.0, (nb, 9, 1, 1, nx[0] + 2 * ng))
    prim[:, 0] += 2.0
    prim[:, 4] += 2.0
    p = PROCESSES["all"]
    r = _Regs(gpu_ctx_strict, "glmmhd", nx, ng, seed=9, nblocks=nb, prim=prim, with_flux=False)
    hydro.RKL2SubstageFused(r.y0, r.yjm1, r.yjm2, r.my0, _cfg(p), hydro.rkl2_coefficients(S_RKL, j, strict=True), TAU,
                            first=(j == 1))
    w = r.want()
    S.substage(prim, w["y0"], w["yjm1"], w["yjm2"], w["my0"], nx, ng, DX, S_RKL, j, TAU, **_ref_kw(p))
    _compare(r.got(), w, ("yjm1", "yjm2", "my0"), True, "66000 blocks")
    a = _Regs(gpu_ctx_strict, "glmmhd", nx, ng, seed=9, nblocks=nb, prim=prim)
    _array_substage(a, _cfg(p), j)
    _compare(a.got(), w, ("yjm1", "yjm2", "my0"), True, "66000 blocks, arrays")


def test_fused_substage_refuses_what_the_fluxes_refuse(gpu_ctx_strict):
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    r = _Regs(gpu_ctx_strict, "euler", SHAPES[2], 2, seed=1, with_flux=False)
    with pytest.raises(L.ApkError) as e:
        hydro.RKL2SubstageFused(r.y0, r.yjm1, r.yjm2, r.my0, _cfg(PROCESSES["ohm"]), S.coefficients(S_RKL, 1), TAU, True)
    assert e.value.code == L.APK_ERR_INVALID
    with pytest.raises(L.ApkError):  # registers must be distinct arrays
        hydro.RKL2SubstageFused(r.y0, r.yjm1, r.y0, r.my0, _cfg(PROCESSES["visc"]), S.coefficients(S_RKL, 1), TAU, True)


# ---- the native driver with diffusion/integrator = rkl2 ---------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO = 200.0
ALL3 = ["diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=%g" % RATIO, "diffusion/conduction=anisotropic",
        "diffusion/conduction_coeff=fixed", "diffusion/thermal_diff_coeff_code=0.2", "diffusion/viscosity=isotropic",
        "diffusion/viscosity_coeff=fixed", "diffusion/mom_diff_coeff_code=0.01", "diffusion/resistivity=ohmic",
        "diffusion/resistivity_coeff=fixed", "diffusion/ohm_diff_coeff_code=0.015"]
MESH3 = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/time/integrator=rk2",
         "hydro/reconstruction=plm"]
ONE_BLOCK = ["parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"]
EIGHT_BLOCKS = ["parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8"]
NCYC = 6


def _sim(deck, overrides, strict=True):
    from athenapk_amd import decks, driver
    return driver.Simulation(decks.load(deck), overrides, strict=strict).initialize()


def test_fused_and_arrays_give_identical_states():
    a = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + ALL3 + ["apk_amd/sts_substage=fused"])
    b = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + ALL3 + ["apk_amd/sts_substage=arrays"])
    assert a.sts_info()[2] is True and b.sts_info()[2] is False and a.info.fused == 0
    u0 = a.gather()
    for _ in range(NCYC):
        a.step()
        b.step()
        assert a.dt == b.dt and a.sts_info()[:2] == b.sts_info()[:2]
    assert a.time == b.time
    assert np.array_equal(a.gather(), b.gather())
    assert np.array_equal(a.gather("prim"), b.gather("prim"))
    assert not np.array_equal(u0, a.gather())


def _rank_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from athenapk_amd import decks, driver
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        s = driver.Simulation(decks.load("synthetic_mhd"), MESH3 + EIGHT_BLOCKS + ALL3, rank=rank, nranks=world,
                              strict=True)
        s.initialize()
        for _ in range(NCYC):
            s.step()
        blocks = {s.block_gid(lb)[0]: s.read_block(lb, "cons") for lb in range(s.info.nblocks_local)}
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), time=s.time, dt=s.dt,
                 **{"b%d" % g: a for g, a in blocks.items()})
        s.close()
    finally:
        dist.destroy_process_group()


def _limits_periodic(sim, ctx):
    """(dt_hyp, dt_diff) of ALL3 on the whole periodic mesh of MESH3, from the state of a one-block simulation: the
    diffusive limit restated (tests/diffusion_reference.py) on the gathered primitives, the hyperbolic one by
    EstimateTimestep on a pack made of the block"""
    from athenapk_amd import hydro, lib as L
    w = sim.gather("prim")
    wp = np.pad(w, ((0, 0), (1, 1), (1, 1), (1, 1)), mode="wrap")[None]
    nx, dx = (32, 16, 16), (1.0 / 32, 1.0 / 16, 1.0 / 16)
    dt_diff = R.diffusion_timestep(wp, nx, 1, dx, 0.3, conduction="anisotropic", viscosity="isotropic", resistivity="ohmic",
                                   kappa=0.2, sat_prefac=1.5, nu=0.01, eta=0.015)
    md = hydro.MeshData(ctx, nx, sim.info.ng, 9, dx=dx, cons=sim.read_block(0, "cons")[None],
                        prim=sim.read_block(0, "prim")[None], with_flux=False, row_pitch="natural")
    return hydro.EstimateTimestep(md, "glmmhd", L.make_eos(sim.info.gamma), 0.3), dt_diff


def test_decomposition_invariance_time_step_and_conservation(tmp_path, gpu_ctx_strict):
    from _spawn import spawn
    one = _sim("synthetic_mhd", MESH3 + ONE_BLOCK + ALL3)
    eight = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + ALL3)
    u0 = one.gather()
    dt_taken = dt_diff = None
    for c in range(NCYC + 1):
        if c:
            dt_taken = one.dt
            one.step()
            eight.step()
            # both half steps of the cycle were sized with the limit estimated before it
            s_want = S.num_stages(0.5 * dt_taken, dt_diff)
            assert one.sts_info()[0] == s_want and eight.sts_info()[0] == s_want
            assert one.sts_info()[1] == 2.0 * (0.5 * dt_taken) / dt_diff
        # dt = min(dt_hyp, ratio dt_diff) where dt_hyp / dt_diff exceeds the ratio, dt_hyp otherwise (hydro.cpp:950-956)
        dt_hyp, dt_diff = _limits_periodic(one, gpu_ctx_strict)
        want = min(dt_hyp, RATIO * dt_diff) if dt_hyp / dt_diff > RATIO else dt_hyp
        print("cycle %d: dt %.17g dt_hyp %.17g dt_diff %.17g" % (c, one.dt, dt_hyp, dt_diff))
        if c == 0 or want <= 2.0 * dt_taken:  # (the driver lets the step grow by at most a factor of two per cycle)
            assert one.dt == want, (c, one.dt, want, dt_hyp, dt_diff)
        assert one.dt == eight.dt
    assert one.time == eight.time
    u1 = one.gather()
    assert np.array_equal(u1, eight.gather())
    assert not np.array_equal(u0, u1)
    # periodic box: mass, momentum and energy to round-off -- every update is a flux difference (the plain Dedner source
    # touches psi only)
    for v in range(5):
        s0, s1 = np.sum(u0[v]), np.sum(u1[v])
        assert abs(s1 - s0) <= 1e-13 * max(np.sum(np.abs(u0[v])), 1.0) * 10, (v, s0, s1)
    blocks = {eight.block_gid(lb)[0]: eight.read_block(lb, "cons") for lb in range(eight.info.nblocks_local)}
    spawn(_rank_worker, lambda port: (2, port, str(tmp_path)), nprocs=2)
    ng = eight.info.ng
    for r in range(2):
        z = np.load(tmp_path / ("rank%d.npz" % r))
        assert float(z["time"]) == one.time and float(z["dt"]) == one.dt
        for key in z.files:
            if key.startswith("b"):
                g = int(key[1:])
                a, b = z[key][:, ng:-ng, ng:-ng, ng:-ng], blocks[g][:, ng:-ng, ng:-ng, ng:-ng]
                assert np.array_equal(a, b), "block %d differs on 2 ranks" % g


def test_the_cap_sets_the_step_where_diffusion_is_stiff():
    # a large viscosity: dt_hyp / dt_diff > ratio, so the step is ratio * dt_diff (hydro.cpp:950-956)
    nu, ratio = 0.5, 20.0
    ov = [o.replace("0.01", str(nu)) if "mom_diff" in o else o for o in ALL3 if "rkl2_max_dt_ratio" not in o]
    s = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + ov + ["diffusion/conduction=none", "diffusion/resistivity=none",
                                                             "diffusion/cfl=0.25", "diffusion/rkl2_max_dt_ratio=%g" % ratio])
    dx = 1.0 / 32
    dt_diff = 0.25 * (1.0 / 6.0) * (dx * dx / (nu + 1e-20))
    assert s.dt == ratio * dt_diff
    s.step()
    assert s.sts_info()[0] == S.num_stages(0.5 * ratio * dt_diff, dt_diff) and s.sts_info()[1] == ratio
    assert s.dt == ratio * dt_diff


@pytest.mark.parametrize("substage", ["fused", "arrays"])
def test_zero_coefficient_leaves_the_restated_rounding_only(substage):
    # riemann = none, RK1: the hyperbolic stage adds zero fluxes, u <- 0 u + 1 u + dt 0 (and the Dedner source multiplies
    # psi = 0); what changes the state is the
    # rounding of mu Yjm1 + nu Yjm2 + (1 - mu - nu) Y0 in the two half steps -- bit for bit the restatement's
    # (iprob 10: a Gaussian in the internal energy whose width is set by thermal_diff_coeff_code, here only a parameter
    # of the profile -- conduction is off, the configured process is viscosity with a zero coefficient)
    n = 64
    ov = ["hydro/riemann=none", "hydro/reconstruction=dc", "parthenon/time/integrator=rk1",
          "parthenon/mesh/nx1=%d" % n, "parthenon/meshblock/nx1=32", "parthenon/time/tlim=0.5",
          "diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=200", "diffusion/mom_diff_coeff_code=0.0",
          "diffusion/thermal_diff_coeff_code=0.25", "problem/diffusion/iprob=10", "problem/diffusion/Bx=0.7",
          "problem/diffusion/amp=0.3", "apk_amd/sts_substage=%s" % substage]
    s = _sim("diffusion", ov)
    u = np.pad(s.gather()[None], ((0, 0), (0, 0), (0, 0), (0, 0), (1, 1)), mode="edge")
    assert np.ptp(u[0, 4]) > 0.01
    dx = (12.0 / n, 1.0, 1.0)
    dt_diff = 0.3 * 0.5 * (dx[0] * dx[0] / (0.0 + 1e-20))
    assert s.dt == 0.5  # the cap is far away: the step is what is left to tlim
    s.step()
    assert s.time == 0.5 and s.sts_info()[0] == 3
    # (zero fluxes whatever the primitives and the ghost cells are: the identity stands in for both)
    for _ in range(2):
        S.sts(u, 0.25, dt_diff, (n, 1, 1), 1, dx, lambda a: None, lambda a: a, viscosity="isotropic", nu=0.0)
    assert np.array_equal(s.gather(), u[0, ..., 1:-1])


def _gauss_l1(kind, n):
    """1-D Gaussian of the reference's diffusion suite at N cells with integrator = rkl2: L1 error of v2 (viscosity) or
    B2 (Ohmic) at t = 2"""
    D, tlim = 0.25, 2.0
    ov = ["parthenon/mesh/nx1=%d" % n, "parthenon/meshblock/nx1=64", "parthenon/time/tlim=%g" % tlim,
          "diffusion/viscosity=%s" % ("isotropic" if kind == "visc" else "none"),
          "diffusion/resistivity=%s" % ("ohmic" if kind == "ohm" else "none"),
          "problem/diffusion/iprob=%d" % (30 if kind == "visc" else 40)]
    if kind == "visc":
        ov += ["hydro/fluid=euler", "hydro/riemann=hllc"]
    s = _sim("diffusion_sts", ov, strict=False)
    s.run()
    assert abs(s.time - tlim) < 1e-12 and s.sts_info()[0] >= 3
    w = s.gather("prim")
    x = -6.0 + (np.arange(n) + 0.5) * 12.0 / n
    ref = 1e-6 / np.sqrt(4.0 * np.pi * D * (0.5 + tlim)) * np.exp(-(x ** 2) / (4.0 * D * (0.5 + tlim)))
    got = w[2, 0, 0, :] if kind == "visc" else w[6, 0, 0, :]
    return np.mean(np.abs(got - ref))


@pytest.mark.parametrize("kind", ["visc", "ohm"])
def test_gaussian_convergence_rkl2(kind):
    # tst/regression/test_suites/diffusion/diffusion.py, int_cfg = rkl2: N = 256, 512, 1024; fitted L1 rate <= -1.95
    res = [256, 512, 1024]
    err = [_gauss_l1(kind, n) for n in res]
    rate = np.polyfit(np.log(res), np.log(err), 1)[0]
    print(kind, "L1 errors", err, "rate", rate)
    assert rate <= -1.95, (err, rate)
