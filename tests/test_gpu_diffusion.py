"""Unsplit diffusion on the GPU: the kernels against the numpy restatement (tests/diffusion_reference.py), and the
native driver with a <diffusion> block -- zero coefficients, decomposition invariance, conservation, and the
reference's regression pins restated at sizes that keep the suite short."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffusion_reference as R  # noqa: E402
import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {1: (40, 1, 1), 2: (18, 12, 1), 3: (12, 10, 8)}
DX = (0.1, 0.07, 0.13)
PROCESSES = {
    "cond_iso": dict(conduction="isotropic", kappa=0.7),
    "cond_aniso": dict(conduction="anisotropic", kappa=0.7),
    "visc": dict(viscosity="isotropic", nu=0.3),
    "ohm": dict(resistivity="ohmic", eta=0.45),
    "all": dict(conduction="anisotropic", kappa=0.7, viscosity="isotropic", nu=0.3, resistivity="ohmic", eta=0.45),
}


def _cfg(p):
    from athenapk_amd import lib as L
    return L.make_diff_cfg(conduction=p.get("conduction", "none"), kappa=p.get("kappa", 0.0), sat_phi=0.3,
                           viscosity=p.get("viscosity", "none"), nu=p.get("nu", 0.0),
                           resistivity=p.get("resistivity", "none"), eta=p.get("eta", 0.0))


def _ref_kw(p):
    kw = dict(p)
    kw["sat_prefac"] = 5.0 * 0.3
    return kw


def _pack(ctx, fluid, ndim, seed, row_pitch=None):
    import torch
    from athenapk_amd import hydro
    nx, ng = SHAPES[ndim], 2
    prim = H.random_prim(fluid, nx, ng, seed=seed, kind="smooth", nblocks=2)
    md = hydro.MeshData(ctx, nx, ng, prim.shape[1], dx=DX, nblocks=2, prim=prim, cons=prim, row_pitch=row_pitch)
    rng = np.random.default_rng(seed + 100)
    flux = []
    for d in range(ndim):
        f = rng.standard_normal(prim.shape)
        md.flux[d].copy_(torch.from_numpy(f).to(md.flux[d].device))
        flux.append(f)
    return md, prim, flux, nx, ng


def _fluid(p):
    return "glmmhd" if p.get("resistivity", "none") != "none" or p.get("conduction") == "anisotropic" else "euler"


CASES = [(name, ndim) for name in PROCESSES for ndim in (1, 2, 3)]


@pytest.mark.parametrize("name,ndim", CASES)
def test_diff_fluxes_strict_bitwise(gpu_ctx_strict, name, ndim):
    from athenapk_amd import hydro
    p = PROCESSES[name]
    for fluid in sorted({_fluid(p), "glmmhd"}):
        md, prim, flux, nx, ng = _pack(gpu_ctx_strict, fluid, ndim, seed=11 * ndim + len(name))
        hydro.CalcDiffFluxes(md, _cfg(p))
        want = R.diff_fluxes(prim, flux + [None] * (3 - ndim), nx, ng, DX, **_ref_kw(p))
        for d in range(ndim):
            got = md.flux_host(d)
            assert not np.array_equal(want[d], flux[d]), "the process added nothing"
            assert np.array_equal(got, want[d]), "%s %d-D %s dir %d: max |diff| %.3e" % (
                name, ndim, fluid, d, np.max(np.abs(got - want[d])))


@pytest.mark.parametrize("name,ndim", CASES)
def test_diff_fluxes_product_build_close(gpu_ctx_fast, name, ndim):
    from athenapk_amd import hydro
    p = PROCESSES[name]
    md, prim, flux, nx, ng = _pack(gpu_ctx_fast, _fluid(p), ndim, seed=5 + ndim)
    hydro.CalcDiffFluxes(md, _cfg(p))
    want = R.diff_fluxes(prim, flux + [None] * (3 - ndim), nx, ng, DX, **_ref_kw(p))
    for d in range(ndim):
        got = md.flux_host(d)
        scale = np.max(np.abs(want[d]))
        assert np.max(np.abs(got - want[d])) <= 1e-12 * scale


def test_diff_fluxes_aligned_rows_bitwise(gpu_ctx_strict):
    from athenapk_amd import hydro
    p = PROCESSES["all"]
    md, prim, flux, nx, ng = _pack(gpu_ctx_strict, "glmmhd", 3, seed=21, row_pitch="aligned")
    assert md.pitch != md.shape[-1] or md.lead != 0
    hydro.CalcDiffFluxes(md, _cfg(p))
    want = R.diff_fluxes(prim, flux, nx, ng, DX, **_ref_kw(p))
    for d in range(3):
        assert np.array_equal(md.flux_host(d), want[d])


def test_more_planes_than_one_launch_holds(gpu_ctx_strict):
    # 66 000 one-dimensional blocks: more (plane, block) pairs than a grid dimension holds (65 535), so the flux passes
    # and the conduction time step are launched in chunks of blocks
    import torch
    from athenapk_amd import hydro
    nb, nx, ng = 66000, (4, 1, 1), 1
    rng = np.random.default_rng(7)
    prim = rng.uniform(-1.0, 1.0, (nb, 9, 1, 1, nx[0] + 2 * ng))
    prim[:, 0] += 2.0
    prim[:, 4] += 2.0
    md = hydro.MeshData(gpu_ctx_strict, nx, ng, 9, dx=DX, nblocks=nb, prim=prim, cons=prim)
    f = rng.standard_normal(prim.shape)
    md.flux[0].copy_(torch.from_numpy(f).to(md.flux[0].device))
    p = PROCESSES["all"]
    hydro.CalcDiffFluxes(md, _cfg(p))
    want = R.diff_fluxes(prim, [f, None, None], nx, ng, DX, **_ref_kw(p))
    assert np.array_equal(md.flux_host(0), want[0])
    got = hydro.EstimateDiffusionTimestep(md, _cfg(PROCESSES["cond_aniso"]), 0.35)
    assert got == R.diffusion_timestep(prim, nx, ng, DX, 0.35, **_ref_kw(PROCESSES["cond_aniso"]))


@pytest.mark.parametrize("name,ndim", [("cond_aniso", 1), ("cond_aniso", 2), ("cond_aniso", 3), ("all", 3),
                                       ("cond_iso", 2), ("visc", 3), ("ohm", 2)])
@pytest.mark.parametrize("strict", [True, False])
def test_diffusion_timestep(gpu_ctx_strict, gpu_ctx_fast, name, ndim, strict):
    from athenapk_amd import hydro
    p = PROCESSES[name]
    ctx = gpu_ctx_strict if strict else gpu_ctx_fast
    md, prim, _, nx, ng = _pack(ctx, _fluid(p), ndim, seed=3 + ndim, row_pitch="aligned" if ndim == 3 else None)
    got = hydro.EstimateDiffusionTimestep(md, _cfg(p), 0.35)
    want = R.diffusion_timestep(prim, nx, ng, DX, 0.35, **_ref_kw(p))
    assert 0.0 < want < 1e300
    if strict:
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= 1e-12 * want


def test_diffusion_refuses_without_mhd(gpu_ctx_strict):
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    md, *_ = _pack(gpu_ctx_strict, "euler", 2, seed=1)
    with pytest.raises(L.ApkError) as e:
        hydro.CalcDiffFluxes(md, _cfg(PROCESSES["ohm"]))
    assert e.value.code == L.APK_ERR_INVALID
    spitzer = _cfg(PROCESSES["cond_iso"])
    spitzer.conduction_coeff = L.DIFF_COEFF["spitzer"]
    with pytest.raises(L.ApkError) as e:
        hydro.CalcDiffFluxes(md, spitzer)
    assert e.value.code == L.APK_ERR_UNSUPPORTED


# ---- the native driver with a <diffusion> block -----------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL3 = ["diffusion/integrator=unsplit", "diffusion/conduction=anisotropic", "diffusion/conduction_coeff=fixed",
        "diffusion/thermal_diff_coeff_code=0.2", "diffusion/viscosity=isotropic", "diffusion/viscosity_coeff=fixed",
        "diffusion/mom_diff_coeff_code=0.01", "diffusion/resistivity=ohmic", "diffusion/resistivity_coeff=fixed",
        "diffusion/ohm_diff_coeff_code=0.015"]
MESH3 = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/time/integrator=rk2",
         "hydro/reconstruction=plm"]
ONE_BLOCK = ["parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"]
EIGHT_BLOCKS = ["parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8"]
NCYC = 6


def _sim(deck, overrides, strict=True, fused=None):
    from athenapk_amd import decks, driver
    s = driver.Simulation(decks.load(deck), overrides, strict=strict)
    if fused is not None:
        s.set_fused(fused)
    return s.initialize()


def test_zero_coefficients_equal_no_diffusion():
    zero = [o.split("=")[0] + "=0.0" if "coeff_code" in o else o for o in ALL3]
    a = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + zero)
    assert a.info.fused == 0
    b = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS, fused=False)
    for _ in range(NCYC):
        a.step()
        b.step()
    assert a.dt == b.dt and a.time == b.time
    assert np.array_equal(a.gather(), b.gather())


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


def _cond_dt_periodic(sim):
    """the diffusive limits of ALL3 (restated, tests/diffusion_reference.py) on the whole periodic mesh of MESH3:
    (anisotropic conduction alone, every process)"""
    w = np.pad(sim.gather("prim"), ((0, 0), (1, 1), (1, 1), (1, 1)), mode="wrap")[None]
    nx, dx = (32, 16, 16), (1.0 / 32, 1.0 / 16, 1.0 / 16)
    kw = dict(kappa=0.2, sat_prefac=1.5, nu=0.01, eta=0.015)
    cond = R.diffusion_timestep(w, nx, 1, dx, 0.3, conduction="anisotropic", **kw)
    every = R.diffusion_timestep(w, nx, 1, dx, 0.3, conduction="anisotropic", viscosity="isotropic",
                                 resistivity="ohmic", **kw)
    return cond, every


def test_decomposition_invariance_and_conservation(tmp_path):
    from _spawn import spawn
    one = _sim("synthetic_mhd", MESH3 + ONE_BLOCK + ALL3)
    eight = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + ALL3)
    u0 = one.gather()
    for c in range(NCYC + 1):
        if c:
            one.step()
            eight.step()
        # the step of every cycle is the anisotropic conduction limit (cond_dt_kernel, which reads the ghost zones of
        # every block), smaller than the hyperbolic one and the other processes' -- the same on one block and on eight
        cond, every = _cond_dt_periodic(one)
        assert cond == every
        assert one.dt == cond and eight.dt == cond, (c, one.dt, eight.dt, cond)
    assert one.time == eight.time
    u1 = one.gather()
    assert np.array_equal(u1, eight.gather())
    assert not np.array_equal(u0, u1)
    # periodic box: mass, momentum and energy to round-off (the plain Dedner source touches psi only)
    for v in range(5):
        s0, s1 = np.sum(u0[v]), np.sum(u1[v])
        assert abs(s1 - s0) <= 1e-13 * max(np.sum(np.abs(u0[v])), 1.0) * 10, (v, s0, s1)
    blocks = {eight.block_gid(lb)[0]: eight.read_block(lb, "cons") for lb in range(eight.info.nblocks_local)}
    spawn(_rank_worker, lambda port: (2, port, str(tmp_path)), nprocs=2)
    ng = eight.info.ng
    for r in range(2):
        z = np.load(tmp_path / ("rank%d.npz" % r))
        assert float(z["time"]) == one.time
        for key in z.files:
            if key.startswith("b"):
                g = int(key[1:])
                a, b = z[key][:, ng:-ng, ng:-ng, ng:-ng], blocks[g][:, ng:-ng, ng:-ng, ng:-ng]
                assert np.array_equal(a, b), "block %d differs on 2 ranks" % g


def test_diffusion_limits_the_time_step():
    # a large viscosity: the step is the diffusive limit cfl_diff / 6 * dx^2 / nu (hydro.cpp:935-963)
    nu = 0.5
    ov = [o.replace("0.01", str(nu)) if "mom_diff" in o else o for o in ALL3]
    s = _sim("synthetic_mhd", MESH3 + EIGHT_BLOCKS + ov + ["diffusion/conduction=none", "diffusion/resistivity=none",
                                                             "diffusion/cfl=0.25"])
    dx = 1.0 / 32
    want = 0.25 * (1.0 / 6.0) * (dx * dx / (nu + 1e-20))
    assert s.dt == want
    s.step()
    assert s.dt == want


def _gauss_l1(kind, n):
    """1-D Gaussian of the reference's diffusion suite at N cells: L1 error of v2 (viscosity) or B2 (Ohmic) at t = 2"""
    D, tlim = 0.25, 2.0
    ov = ["parthenon/mesh/nx1=%d" % n, "parthenon/meshblock/nx1=64", "parthenon/time/tlim=%g" % tlim,
          "diffusion/viscosity=%s" % ("isotropic" if kind == "visc" else "none"),
          "diffusion/resistivity=%s" % ("ohmic" if kind == "ohm" else "none"),
          "problem/diffusion/iprob=%d" % (30 if kind == "visc" else 40)]
    if kind == "visc":
        ov += ["hydro/fluid=euler", "hydro/riemann=hllc"]
    s = _sim("diffusion", ov, strict=False)
    s.run()
    assert abs(s.time - tlim) < 1e-12
    w = s.gather("prim")
    x = -6.0 + (np.arange(n) + 0.5) * 12.0 / n
    ref = 1e-6 / np.sqrt(4.0 * np.pi * D * (0.5 + tlim)) * np.exp(-(x ** 2) / (4.0 * D * (0.5 + tlim)))
    got = w[2, 0, 0, :] if kind == "visc" else w[6, 0, 0, :]
    return np.mean(np.abs(got - ref))


@pytest.mark.parametrize("kind", ["visc", "ohm"])
def test_gaussian_convergence(kind):
    # tst/regression/test_suites/diffusion/diffusion.py: N = 256, 512, 1024; fitted L1 rate <= -1.95 (unsplit)
    res = [256, 512, 1024]
    err = [_gauss_l1(kind, n) for n in res]
    rate = np.polyfit(np.log(res), np.log(err), 1)[0]
    assert rate <= -1.95, (err, rate)


def test_anisotropic_ring_stays_bounded_and_conserves_energy():
    # iprob 20: a hot arc on circular field lines, pure anisotropic conduction (riemann = none, as the reference's
    # ring decks); the reference's hard check is T >= 10 everywhere (aniso_therm_cond_ring_conv.py)
    ov = ["hydro/fluid=glmmhd", "hydro/riemann=none", "hydro/reconstruction=dc", "hydro/gamma=2.0",
          "parthenon/time/integrator=rk1", "parthenon/time/tlim=1.0", "parthenon/mesh/nx1=64",
          "parthenon/meshblock/nx1=32", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx2=32",
          "parthenon/mesh/x1min=-1.0", "parthenon/mesh/x1max=1.0", "parthenon/mesh/x2min=-1.0", "parthenon/mesh/x2max=1.0",
          "parthenon/mesh/ix1_bc=periodic", "parthenon/mesh/ox1_bc=periodic", "diffusion/viscosity=none",
          "diffusion/conduction=anisotropic", "diffusion/conduction_coeff=fixed", "diffusion/thermal_diff_coeff_code=0.01",
          "problem/diffusion/iprob=20"]
    s = _sim("diffusion", ov, strict=False)
    e0 = np.sum(s.gather()[4])
    w0 = s.gather("prim")
    s.run()
    assert s.ncycle > 10
    w = s.gather("prim")
    T = w[4] / w[0]
    assert np.min(T) >= 10.0
    assert np.max(T) <= 12.0
    assert not np.array_equal(w[4], w0[4])  # heat has moved
    assert abs(np.sum(s.gather()[4]) - e0) <= 1e-12 * e0


@pytest.mark.parametrize("res,tol", [(16, 0.22), (32, 0.05)])
def test_decaying_slow_wave(tmp_path, res, tol):
    # tst/regression/test_suites/diffusion_linwave3d/diffusion_linwave3d.py: a slow magnetosonic wave on 2N x N x N
    # decays under viscosity, conduction and resistivity; the decay rate fitted to the MaxAbsV2 history column
    # (column 13) is within 22 % (N = 16) / 5 % (N = 32) of the analytic rate
    from athenapk_amd import decks, driver
    nu = 0.01
    kappa = eta = 2.0 * nu
    ov = ["parthenon/mesh/nx1=%d" % (2 * res), "parthenon/meshblock/nx1=%d" % (2 * res), "parthenon/mesh/nx2=%d" % res,
          "parthenon/meshblock/nx2=%d" % res, "parthenon/mesh/nx3=%d" % res, "parthenon/meshblock/nx3=%d" % res,
          "parthenon/mesh/nghost=2", "parthenon/time/integrator=vl2", "parthenon/time/tlim=3.0",
          "hydro/reconstruction=plm", "hydro/fluid=glmmhd", "hydro/riemann=hlld", "parthenon/output2/file_type=hst",
          "parthenon/output2/dt=0.03", "problem/linear_wave/dump_max_v2=true", "parthenon/job/problem_id=lw%d" % res,
          "problem/linear_wave/amp=1e-4", "problem/linear_wave/wave_flag=2", "problem/linear_wave/compute_error=false",
          "problem/linear_wave/test=false",
          "diffusion/integrator=unsplit", "diffusion/conduction=isotropic", "diffusion/conduction_coeff=fixed",
          "diffusion/thermal_diff_coeff_code=%r" % kappa, "diffusion/viscosity=isotropic",
          "diffusion/viscosity_coeff=fixed", "diffusion/mom_diff_coeff_code=%r" % nu, "diffusion/resistivity=ohmic",
          "diffusion/resistivity_coeff=fixed", "diffusion/ohm_diff_coeff_code=%r" % eta]
    s = driver.Simulation(decks.load("linear_wave_mhd3d"), ov, strict=False)
    s.execute(str(tmp_path))
    s.close()
    hst = np.genfromtxt(str(tmp_path / ("lw%d.out2.hst" % res)), names=True, skip_header=1)
    tt, vy = hst["1time"], hst["13MaxAbsV2"]
    assert tt[-1] >= 3.0 - 1e-9 and len(tt) > 50
    ksqr = (2.0 * np.pi / 1.0) ** 2
    rate = (4.0 * nu + 3.0 * eta / 4.0 + kappa * 4.0 / 5.0) * (2.0 / 15.0) * ksqr
    p = np.polynomial.Polynomial.fit(tt, np.log(np.abs(vy)), 1, w=np.sqrt(vy))
    fit_rate = -p.convert(domain=(-1, 1)).coef[-1]
    assert abs(rate / fit_rate - 1.0) <= tol, (rate, fit_rate)


# tst/regression/test_suites/aniso_therm_cond_gauss_conv/aniso_therm_cond_gauss_conv.py: a Gaussian in temperature
# (iprob 10) on N x 32 cells of [-6, 6] x [-1, 1], gamma = 2 and rho = 1 so that T = p = e, pure conduction (riemann =
# none), kappa = 0.25, RK2 with the unsplit integrator, t = 2.  The field is absent (isotropic conduction), along x1,
# at 45 degrees, or along x2 (anisotropic).  Along the field the profile spreads with D = kappa Bx^2; the fitted L1 rate
# over N = 128, 256, 512 must be <= -1.98.  Across the field nothing is conducted: the profile stays as it started.
GAUSS_FIELDS = {"none": (0.0, 0.0), "aligned": (1.0, 0.0), "angle": (1.0 / np.sqrt(2.0), 1.0 / np.sqrt(2.0)),
                "perp": (0.0, 1.0)}


def _thermal_gauss(field, n):
    bx, by = GAUSS_FIELDS[field]
    ov = ["parthenon/mesh/nx1=%d" % n, "parthenon/meshblock/nx1=64", "parthenon/mesh/x1min=-6.0",
          "parthenon/mesh/x1max=6.0", "parthenon/mesh/ix1_bc=periodic", "parthenon/mesh/ox1_bc=periodic",
          "parthenon/mesh/nx2=32", "parthenon/meshblock/nx2=32", "parthenon/mesh/x2min=-1.0", "parthenon/mesh/x2max=1.0",
          "parthenon/time/integrator=rk2", "parthenon/time/tlim=2.0", "hydro/fluid=glmmhd", "hydro/riemann=none",
          "hydro/reconstruction=dc", "hydro/gamma=2.0", "problem/diffusion/iprob=10", "problem/diffusion/Bx=%.17g" % bx,
          "problem/diffusion/By=%.17g" % by, "diffusion/viscosity=none", "diffusion/resistivity=none",
          "diffusion/conduction=%s" % ("isotropic" if field == "none" else "anisotropic"),
          "diffusion/conduction_coeff=fixed", "diffusion/thermal_diff_coeff_code=0.25"]
    s = _sim("diffusion", ov, strict=False)
    t0 = s.gather("prim")[4, 0, 0, :]
    s.run()
    assert abs(s.time - 2.0) < 1e-12 and s.ncycle >= 1
    T = s.gather("prim")[4, 0, 0, :]  # one row, as the reference's analysis (p = T: gamma = 2, rho = 1)
    x = -6.0 + (np.arange(n) + 0.5) * 12.0 / n
    D = 0.25 if bx == 0.0 else 0.25 * bx * bx
    t = 0.0 if field == "perp" else 2.0
    ref = 1.0 + 1e-6 / (np.sqrt(4 * np.pi * D * (0.5 + t)) / np.exp(-(x ** 2) / (4.0 * D * (0.5 + t))))
    return np.mean(np.abs(T - ref)), T, t0


@pytest.mark.parametrize("field", ["none", "aligned", "angle"])
def test_thermal_gaussian_convergence(field):
    res = [128, 256, 512]
    err = [_thermal_gauss(field, n)[0] for n in res]
    rate = np.polyfit(np.log(res), np.log(err), 1)[0]
    assert rate <= -1.98, (field, err, rate)


def test_thermal_gaussian_across_the_field_is_not_conducted():
    for n in (128, 256, 512):
        l1, T, t0 = _thermal_gauss("perp", n)
        assert np.array_equal(T, t0)  # no flux across the field: not a bit has moved
        assert l1 < 1e-12  # ... and that is the initial profile (iprob 10 with Bx = 0: the unit-coefficient form)
