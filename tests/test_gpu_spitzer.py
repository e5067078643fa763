"""Spitzer thermal conduction on the GPU: the flux pass, the time-step reduction and the fused RKL2 sub-stage against the
numpy restatement (tests/spitzer_reference.py) on inputs that reach every branch (tests/spitzer_cases.py), the argument
handling of the _v2 entry points, and the native driver on inputs/diffusion_spitzer.in -- decomposition invariance,
fused against passes, the time step, conservation, and a linearisation that ties the unit conversion to a
fixed-coefficient run."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spitzer_cases as SC  # noqa: E402
import spitzer_reference as SP  # noqa: E402
import sts_reference as S  # noqa: E402
from test_gpu_sts import _Regs, _compare  # noqa: E402  (the four registers of a sub-stage; DX is the same)

pytestmark = pytest.mark.gpu

DX, NG = SC.DX, SC.NG
PROCESSES = {
    "iso": dict(conduction="isotropic"),
    "aniso": dict(conduction="anisotropic"),
    "iso_all": dict(conduction="isotropic", viscosity="isotropic", nu=0.3, resistivity="ohmic", eta=0.45),
    "aniso_all": dict(conduction="anisotropic", viscosity="isotropic", nu=0.3, resistivity="ohmic", eta=0.45),
}
CASES = [(name, ndim) for name in PROCESSES for ndim in (1, 2, 3)]
TAU, S_RKL = 0.013, 9


def _cfg(p):
    from athenapk_amd import lib as L
    cfg = L.make_diff_cfg(conduction=p["conduction"], kappa=0.0, viscosity=p.get("viscosity", "none"), nu=p.get("nu", 0.0),
                          resistivity=p.get("resistivity", "none"), eta=p.get("eta", 0.0))
    cfg.conduction_coeff = L.DIFF_COEFF["spitzer"]
    cfg.conduction_sat_prefac = SC.SAT_PREFAC
    return cfg


def _spitzer():
    from athenapk_amd import lib as L
    return L.make_spitzer_cfg(*SC.SPITZER)


def _ref_kw(p):
    return dict(p, sat_prefac=SC.SAT_PREFAC, spitzer=SC.SPITZER)


@functools.lru_cache(maxsize=None)
def _inputs(ndim):
    """(prim, flux) of a dimension, shared by the tests and never written to; the condition on the inputs -- every
    branch is taken -- is checked here, on the numpy side, before any device result is compared"""
    nx = SC.SHAPES[ndim]
    prim = SC.make_prim(nx, seed=40 + ndim)
    rng = np.random.default_rng(140 + ndim)
    flux = [rng.standard_normal(prim.shape) for _ in range(ndim)]
    for cond in ("anisotropic", "isotropic"):
        r = SC.branch_report(prim, nx, cond)
        assert r["pos"] > 0 and r["neg"] > 0 and r["zero"] > 0 and r["flat_cells"] > 0, r
        assert r["t_min"] < 2e5 and r["t_max"] > 5e7, r  # 1e5 K .. 1e8 K through the units
        if cond == "anisotropic":
            assert r["tiny_b"] > 0 and r["no_field_cells"] > 0 and r["ratio_below_1"] > 0 and r["ratio_above_100"] > 0, r
    return prim, flux


@functools.lru_cache(maxsize=None)
def _want_fluxes(name, ndim):
    prim, flux = _inputs(ndim)
    return SP.diff_fluxes(prim, flux + [None] * (3 - ndim), SC.SHAPES[ndim], NG, DX, **_ref_kw(PROCESSES[name]))


def _pack(ctx, ndim):
    import torch
    from athenapk_amd import hydro
    prim, flux = _inputs(ndim)
    md = hydro.MeshData(ctx, SC.SHAPES[ndim], NG, 9, dx=DX, nblocks=2, prim=prim, cons=prim)
    for d in range(ndim):
        md.flux[d].copy_(torch.from_numpy(flux[d]).to(md.flux[d].device))
    return md, prim, flux


@pytest.mark.parametrize("name,ndim", CASES)
def test_spitzer_fluxes_strict_bitwise(gpu_ctx_strict, name, ndim):
    from athenapk_amd import hydro
    md, prim, flux = _pack(gpu_ctx_strict, ndim)
    hydro.CalcDiffFluxes(md, _cfg(PROCESSES[name]), spitzer=_spitzer())
    want = _want_fluxes(name, ndim)
    for d in range(ndim):
        got = md.flux_host(d)
        assert not np.array_equal(want[d], flux[d]), "the process added nothing"
        assert np.array_equal(got, want[d]), "%s %d-D dir %d: max |diff| %.3e" % (name, ndim, d, np.max(np.abs(got - want[d])))


@pytest.mark.parametrize("name,ndim", CASES)
def test_spitzer_fluxes_product_build_close(gpu_ctx_fast, name, ndim):
    from athenapk_amd import hydro
    md, prim, flux = _pack(gpu_ctx_fast, ndim)
    hydro.CalcDiffFluxes(md, _cfg(PROCESSES[name]), spitzer=_spitzer())
    want = _want_fluxes(name, ndim)
    for d in range(ndim):
        got = md.flux_host(d)
        scale = np.max(np.abs(want[d]))
        err = np.max(np.abs(got - want[d]))
        print("%s %d-D dir %d: max |diff| %.3e of scale %.3e" % (name, ndim, d, err, scale))
        assert err <= 1e-12 * scale


@pytest.mark.parametrize("name,ndim", [(n, d) for n in ("iso", "aniso", "aniso_all") for d in (1, 2, 3)])
@pytest.mark.parametrize("strict", [True, False])
def test_spitzer_timestep(gpu_ctx_strict, gpu_ctx_fast, name, ndim, strict):
    from athenapk_amd import hydro
    p = PROCESSES[name]
    md, prim, _ = _pack(gpu_ctx_strict if strict else gpu_ctx_fast, ndim)
    got = hydro.EstimateDiffusionTimestep(md, _cfg(p), 0.35, spitzer=_spitzer())
    want = SP.diffusion_timestep(prim, SC.SHAPES[ndim], NG, DX, 0.35, **_ref_kw(p))
    assert 0.0 < want < 1e300
    print("%s %d-D: dt %.17g, restated %.17g" % (name, ndim, got, want))
    if strict:
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize("ndim", [1, 3])
@pytest.mark.parametrize("strict", [True, False])
def test_uniform_temperature_sets_no_limit(gpu_ctx_strict, gpu_ctx_fast, strict, ndim):
    # no cell has a gradient: the reduction returns its initial value DBL_MAX, and the limit is what the reference
    # returns for that (conduction.cpp:182-183), cfl_diff * fac * DBL_MAX -- DBL_MAX itself where cfl_diff * fac is 1
    from athenapk_amd import hydro
    nx = SC.SHAPES[ndim]
    prim = np.array(_inputs(ndim)[0])
    prim[:, 0] = 1.25
    prim[:, 4] = 2.5
    md = hydro.MeshData(gpu_ctx_strict if strict else gpu_ctx_fast, nx, NG, 9, dx=DX, nblocks=2, prim=prim, cons=prim)
    fac = 0.5 if ndim == 1 else 1.0 / 6.0
    for name in ("iso", "aniso"):
        for cfl in (0.35, 1.0 / fac):
            want = SP.diffusion_timestep(prim, nx, NG, DX, cfl, **_ref_kw(PROCESSES[name]))
            assert want == cfl * fac * sys.float_info.max
            if cfl != 0.35:
                assert want == sys.float_info.max
            assert hydro.EstimateDiffusionTimestep(md, _cfg(PROCESSES[name]), cfl, spitzer=_spitzer()) == want


def _restated_substage(w, prim, nx, j, p):
    """tests/sts_reference.py::substage with the fluxes of tests/spitzer_reference.py"""
    ndim = SC.ndim_of(nx)
    zero = [np.zeros_like(w["yjm1"]) if d < ndim else None for d in range(3)]
    m = S.flux_divergence(SP.diff_fluxes(prim, zero, nx, NG, DX, **_ref_kw(p)), nx, NG, DX)
    if j == 1:
        (sk, sj, si), _ = S._interior(nx, NG)
        w["my0"][(slice(None), slice(None), sk, sj, si)] = m
        S.step_first(w["y0"], w["yjm1"], w["yjm2"], w["my0"], S_RKL, TAU, nx, NG)
    else:
        S.step_other(w["y0"], w["yjm1"], w["yjm2"], w["my0"], m, S.coefficients(S_RKL, j), TAU, nx, NG)


def _fused_case(ctx, name, ndim, j, exact):
    """the fused sub-stage against the flux-array sequence on zeroed arrays (ResetFluxes, CalcDiffFluxes, FluxDivergence +
    RKL2StepFirst / RKL2StepOther), both on the device, and both against the restatement"""
    from athenapk_amd import hydro
    p, nx = PROCESSES[name], SC.SHAPES[ndim]
    prim = np.array(_inputs(ndim)[0])
    sd = 13 * ndim + len(name) + j
    fused = _Regs(ctx, "glmmhd", nx, NG, seed=sd, prim=prim, with_flux=False)
    arrays = _Regs(ctx, "glmmhd", nx, NG, seed=sd, prim=prim)
    k = hydro.rkl2_coefficients(S_RKL, j, strict=True)
    hydro.RKL2SubstageFused(fused.y0, fused.yjm1, fused.yjm2, fused.my0, _cfg(p), k, TAU, first=(j == 1), spitzer=_spitzer())
    arrays.zero_flux()
    hydro.CalcDiffFluxes(arrays.yjm1, _cfg(p), spitzer=_spitzer())
    if j == 1:
        hydro.FluxDivergence(arrays.yjm1, arrays.my0)
        hydro.RKL2StepFirst(arrays.y0, arrays.yjm1, arrays.yjm2, arrays.my0, S_RKL, TAU)
    else:
        hydro.RKL2StepOther(arrays.y0, arrays.yjm1, arrays.yjm2, arrays.my0, k[0], k[1], k[2], k[3], TAU)
    w = fused.want()
    _restated_substage(w, prim, nx, j, p)
    assert not np.array_equal(w["yjm1"], fused.host["yjm1"])
    what = "%s %d-D j=%d" % (name, ndim, j)
    regs = ("yjm1", "yjm2", "my0")
    if exact:
        _compare(fused.got(), arrays.got(), regs, True, what + " fused vs arrays")
    _compare(fused.got(), w, regs, exact, what + " fused vs restatement")
    _compare(arrays.got(), w, regs, exact, what + " arrays vs restatement")


@pytest.mark.parametrize("j", [1, 2])
@pytest.mark.parametrize("name,ndim", CASES)
def test_spitzer_fused_substage_strict_bitwise(gpu_ctx_strict, name, ndim, j):
    _fused_case(gpu_ctx_strict, name, ndim, j, exact=True)


@pytest.mark.parametrize("j", [1, 2])
@pytest.mark.parametrize("name,ndim", CASES)
def test_spitzer_fused_substage_product_build_close(gpu_ctx_fast, name, ndim, j):
    _fused_case(gpu_ctx_fast, name, ndim, j, exact=False)


def test_v2_argument_handling(gpu_ctx_strict):
    from athenapk_amd import hydro
    from athenapk_amd import lib as L
    md, *_ = _pack(gpu_ctx_strict, 2)
    for bad in ((0.0, SC.MBAR, SC.KB), (SC.COEFF, -SC.MBAR, SC.KB), (SC.COEFF, SC.MBAR, 0.0), (float("nan"), SC.MBAR, SC.KB)):
        with pytest.raises(L.ApkError) as e:
            hydro.CalcDiffFluxes(md, _cfg(PROCESSES["iso"]), spitzer=L.make_spitzer_cfg(*bad))
        assert e.value.code == L.APK_ERR_INVALID
        with pytest.raises(L.ApkError) as e:
            hydro.EstimateDiffusionTimestep(md, _cfg(PROCESSES["aniso"]), 0.3, spitzer=L.make_spitzer_cfg(*bad))
        assert e.value.code == L.APK_ERR_INVALID
    # without the Spitzer numbers: unsupported, as through the fixed-coefficient entry points
    for call in (lambda: hydro.CalcDiffFluxes(md, _cfg(PROCESSES["iso"])),
                 lambda: hydro.EstimateDiffusionTimestep(md, _cfg(PROCESSES["iso"]), 0.3)):
        with pytest.raises(L.ApkError) as e:
            call()
        assert e.value.code == L.APK_ERR_UNSUPPORTED
    # anisotropic Spitzer conduction on an Euler pack
    nx = SC.SHAPES[2]
    w = np.array(_inputs(2)[0][:, :5])
    euler = hydro.MeshData(gpu_ctx_strict, nx, NG, 5, dx=DX, nblocks=2, prim=w, cons=w)
    with pytest.raises(L.ApkError) as e:
        hydro.CalcDiffFluxes(euler, _cfg(PROCESSES["aniso"]), spitzer=_spitzer())
    assert e.value.code == L.APK_ERR_INVALID
    r = _Regs(gpu_ctx_strict, "euler", nx, NG, seed=1, prim=w, with_flux=False)
    with pytest.raises(L.ApkError) as e:
        hydro.RKL2SubstageFused(r.y0, r.yjm1, r.yjm2, r.my0, _cfg(PROCESSES["aniso"]), S.coefficients(S_RKL, 1), TAU, True,
                                spitzer=_spitzer())
    assert e.value.code == L.APK_ERR_INVALID
    # ... where isotropic Spitzer conduction runs
    before = euler.flux_host(0)
    hydro.CalcDiffFluxes(euler, _cfg(PROCESSES["iso"]), spitzer=_spitzer())
    assert not np.array_equal(euler.flux_host(0), before)
    # Spitzer resistivity stays refused
    cfg = _cfg(PROCESSES["aniso_all"])
    cfg.resistivity_coeff = L.DIFF_COEFF["spitzer"]
    with pytest.raises(L.ApkError) as e:
        hydro.CalcDiffFluxes(md, cfg, spitzer=_spitzer())
    assert e.value.code == L.APK_ERR_UNSUPPORTED


# ---- the native driver on inputs/diffusion_spitzer.in -------------------------------------------------------------------
# cut to 32 x 16 x 16 cells of width 0.375, periodic, with an oblique field.  The Spitzer coefficient is raised so that the
# diffusive limit is the one that matters: x 1e3 for unsplit (chi = 10 .. 16: dt_diff is a twelfth of dt_hyp), x 1e4 for
# rkl2 (dt_hyp / dt_diff near 180: some twenty sub-stages per half step).
MESH3 = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/mesh/x2min=-3.0",
         "parthenon/mesh/x2max=3.0", "parthenon/mesh/x3min=-3.0", "parthenon/mesh/x3max=3.0", "problem/diffusion/By=0.5"] + [
    "parthenon/mesh/%sx%d_bc=periodic" % (io, d) for d in (1, 2, 3) for io in "io"]
ONE_BLOCK = ["parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"]
EIGHT_BLOCKS = ["parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8"]
UNSPLIT = ["diffusion/spitzer_cond_in_erg_by_s_K_cm=4.6e-4"]
RATIO = 200.0
RKL2 = ["diffusion/spitzer_cond_in_erg_by_s_K_cm=4.6e-3", "diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=%g" % RATIO]
NCYC = 3


def _sim(overrides, strict=True, deck="diffusion_spitzer"):
    from athenapk_amd import decks, driver
    return driver.Simulation(decks.load(deck), overrides, strict=strict).initialize()


def _dt_diff_periodic(sim):
    """the diffusive limit restated on the gathered primitives of the whole periodic mesh of MESH3"""
    w = np.pad(sim.gather("prim"), ((0, 0), (1, 1), (1, 1), (1, 1)), mode="wrap")[None]
    sp = sim.spitzer_options()
    return SP.diffusion_timestep(w, (32, 16, 16), 1, (12.0 / 32, 6.0 / 16, 6.0 / 16), 0.3, conduction="anisotropic",
                                 sat_prefac=6.86 * np.sqrt(SC.MU) * 0.3, spitzer=(sp.coeff_code, sp.mbar, sp.k_boltzmann))


def _conserved_and_changed(u0, u1):
    assert not np.array_equal(u0, u1)
    e0, e1 = np.sum(u0[4]), np.sum(u1[4])
    print("total energy %.17g -> %.17g" % (e0, e1))
    assert abs(e1 - e0) <= 1e-12 * e0


def test_driver_unsplit():
    one = _sim(MESH3 + ONE_BLOCK + UNSPLIT)
    eight = _sim(MESH3 + EIGHT_BLOCKS + UNSPLIT)
    assert one.info.fused == 0 and one.spitzer_options() is not None
    u0 = one.gather()
    for c in range(NCYC + 1):
        if c:
            one.step()
            eight.step()
        want = _dt_diff_periodic(one)
        print("cycle %d: dt %.17g restated %.17g" % (c, one.dt, want))
        assert one.dt == want and eight.dt == want, (c, one.dt, eight.dt, want)
    assert one.time == eight.time
    u1 = one.gather()
    assert np.array_equal(u1, eight.gather())
    _conserved_and_changed(u0, u1)


def test_driver_rkl2():
    one = _sim(MESH3 + ONE_BLOCK + RKL2)
    eight = _sim(MESH3 + EIGHT_BLOCKS + RKL2)
    fused = _sim(MESH3 + EIGHT_BLOCKS + RKL2 + ["apk_amd/sts_substage=fused"])
    assert fused.sts_info()[2] is True and eight.sts_info()[2] is False
    u0 = one.gather()
    dt_diff = _dt_diff_periodic(one)
    for c in range(1, NCYC + 1):
        dt_taken = one.dt
        assert eight.dt == dt_taken and fused.dt == dt_taken
        for s in (one, eight, fused):
            s.step()
        # both half steps of the cycle were sized with the limit estimated before it, which is the restated one: with rkl2
        # the diffusive limit enters the step through the sub-stage count and the ratio 2 tau / dt_diff only
        s_want = S.num_stages(0.5 * dt_taken, dt_diff)
        print("cycle %d: dt %.17g dt_diff %.17g sub-stages %d" % (c, dt_taken, dt_diff, s_want))
        assert s_want >= 5
        for s in (one, eight, fused):
            assert s.sts_info()[0] == s_want and s.sts_info()[1] == 2.0 * (0.5 * dt_taken) / dt_diff, (c, s.sts_info())
        dt_diff = _dt_diff_periodic(one)
    assert one.time == eight.time == fused.time
    u1 = one.gather()
    assert np.array_equal(u1, eight.gather())
    assert np.array_equal(eight.gather(), fused.gather())
    assert np.array_equal(eight.gather("prim"), fused.gather("prim"))
    _conserved_and_changed(u0, u1)


# ---- linearisation ---------------------------------------------------------------------------------------------------
# The ratio ||T_A - T_B||_1 / (2.5 delta ||T_B - T0||_1) of tests/spitzer_cases.py, measured with the numpy restatements on
# this very setup (tests/test_spitzer_host.py repeats the measurement): 0.1227.  The bound is twice that.
LIN_K_MEASURED = 0.1227


def _lin_run(extra, tlim):
    u = SC.LIN_UNITS
    ov = ["parthenon/mesh/nx1=%d" % SC.LIN_N, "parthenon/meshblock/nx1=%d" % SC.LIN_N, "parthenon/mesh/x1min=%r" % SC.LIN_XMIN,
          "parthenon/mesh/x1max=%r" % SC.LIN_XMAX, "parthenon/mesh/ix1_bc=periodic", "parthenon/mesh/ox1_bc=periodic",
          "parthenon/time/cfl=%r" % SC.LIN_CFL, "parthenon/time/tlim=%r" % tlim, "hydro/gamma=2.0", "hydro/He_mass_fraction=%r" % u["he_mass_fraction"],
          "units/code_length_cgs=%r" % u["length"], "units/code_time_cgs=%r" % u["time"], "units/code_mass_cgs=%r" % u["mass"],
          "diffusion/conduction=anisotropic", "diffusion/conduction_sat_phi=%r" % SC.LIN_SAT_PHI, "problem/diffusion/Bx=1.0",
          "problem/diffusion/By=0.0"]
    s = _sim(ov + extra, strict=False)
    ng = s.info.ng
    u = np.zeros(s.block_shape)
    temp = np.pad(SC.lin_profile(), ng, mode="wrap")
    u[0] = 1.0
    u[5] = 1.0
    u[4, 0, 0] = temp + 0.5  # rho = 1, gamma = 2: E = p + B^2 / 2
    s.write_block(0, u)
    s.exchange_ghosts()
    s.fill_derived()
    s.reset_time_step()
    dt0 = s.dt
    s.run()
    assert abs(s.time - tlim) < 1e-12 and SC.LIN_CYCLES <= s.ncycle <= SC.LIN_CYCLES + 2, (s.time, s.ncycle)
    w = s.gather("prim")
    return w[4, 0, 0] / w[0, 0, 0], dt0


def test_linearisation_ties_the_units_to_a_fixed_coefficient():
    """Spitzer (run A) against anisotropic conduction with the fixed coefficient kappa0 = chi(T0, rho0) computed here from
    the cgs constants (run B), on T = T0 (1 + 1e-6 G(x)), 64 cells, the product build, both to the time of 300 diffusive
    limits of kappa0.  The two differ only through chi's relative variation 2.5 delta:
    ||T_A - T_B||_1 <= K 2.5 delta ||T_B - T0||_1 with K twice the ratio the numpy restatements give on this setup, 0.1227
    (so K = 0.2454).  A unit conversion off by 0.8 % (the hydrogen mass for the atomic mass unit) gives a ratio of 1166, one
    off by a factor of ten 2e5."""
    (coeff, mbar, kb), kappa0 = SC.lin_numbers()
    tlim = SC.lin_tlim(kappa0)
    t_a, dt_a = _lin_run(["diffusion/conduction_coeff=spitzer", "diffusion/spitzer_cond_in_erg_by_s_K_cm=%r" % SC.LIN_COND_CGS], tlim)
    t_b, dt_b = _lin_run(["diffusion/conduction_coeff=fixed", "diffusion/thermal_diff_coeff_code=%r" % kappa0], tlim)
    # both runs step at the diffusive limit, as the restated experiment does
    dx = (SC.LIN_XMAX - SC.LIN_XMIN) / SC.LIN_N
    assert abs(dt_b / (SC.LIN_CFL * 0.5 * dx * dx / kappa0) - 1.0) < 1e-9 and abs(dt_a / dt_b - 1.0) < 1e-4, (dt_a, dt_b)
    spread = np.sum(np.abs(t_b - SC.lin_profile()))
    assert spread > 0.1 * np.sum(np.abs(SC.lin_profile() - SC.LIN_T0))  # the pulse has spread
    ratio = SC.lin_ratio(t_a, t_b)
    print("linearisation ratio %.4f (restated on the CPU: %.4f)" % (ratio, LIN_K_MEASURED))
    assert ratio <= 2.0 * LIN_K_MEASURED
