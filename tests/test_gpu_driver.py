"""GPU driver-level parity: the native host driver (deck -> stages -> dt) on the device vs
the oracle's mini-driver on the CPU, on the BASELINE configurations scaled to sizes the
oracle finishes in seconds, plus size-independent properties at BASELINE's full sizes."""
import json
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GAMMA_DECK = 1.666666666666667  # the literal in the decks (inputs/*.in), not 5/3


def _sim(deck, overrides, strict=True, fused=True):
    from athenapk_amd import decks, driver
    s = driver.Simulation(decks.load(deck), overrides, strict=strict)
    s.set_fused(fused)
    return s


def _assert_same(got, want, strict, tol=1e-12):
    if strict:
        assert np.array_equal(got, want), "max abs diff %.3e" % np.max(np.abs(got - want))
    else:
        assert np.max(np.abs(got - want)) <= tol * (np.max(np.abs(want)) + 1e-300)


# ---- config 1: linear_wave3d, 64x32x32 single meshblock, PLM + HLLE, RK2 -----------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
def test_config1_linear_wave_matches_oracle(oracle, strict):
    s = _sim("linear_wave3d", [], strict=strict).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hlle", integrator="rk2", nx=(64, 32, 32), ng=2,
                   xmax=(3.0, 1.5, 1.5), cfl=0.3, gamma=GAMMA_DECK, nthreads=os.cpu_count())
    o.pgen("linear_wave", wave_flag=0, amp=1e-6)
    assert s.tlim == o.period  # "test = true": one wave period
    if strict:
        assert s.dt == o.dt
    n_gpu = s.run()
    n_cpu = o.run(o.period)
    assert n_gpu == n_cpu
    _assert_same(s.gather("cons"), o.gather_cons(), strict)
    rms, l1, _ = s.linear_wave_errors()
    rms_o, l1_o, _ = o.linear_wave_errors()
    # north_star: linear-wave L1 error within 1e-12 of the reference arithmetic.  The error itself is 7.9e-8, so the
    # bound that means something is relative to it: the product build (FMA contraction, reciprocal-based divides)
    # measures 8.8e-17 absolute = 1.1e-9 of the error norm; the test allows 1e-15 / 2e-8.
    assert abs(rms - rms_o) <= 1e-15 and abs(rms - rms_o) <= 2e-8 * rms_o and np.all(np.abs(l1 - l1_o) <= 1e-15)
    if strict:
        assert rms == rms_o


# ---- MHD linear waves (src/pgen/linear_wave_mhd.cpp): north_star's "linear-wave L1 error within 1e-12" on the MHD path ----
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("wave_flag,vflow", [(0, 0.0), (1, 0.0), (2, 0.0), (3, 1.0), (6, 0.0)],
                         ids=["fast", "alfven", "slow", "entropy", "fast_plus"])
def test_mhd_linear_wave_matches_oracle(oracle, wave_flag, vflow, strict):
    """inputs/linear_wave_mhd3d.in at 32 x 16 x 16 (two meshblocks), PPM + HLLD + Dedner, RK3, one wave period: problem
    generator (B = curl A), time step, every cycle and the error norms of d, M1..3, E, B1..3 -- bit for bit in the parity
    build; in the product build (FMA contraction, reciprocal-based divides) the L1 norms within north_star's 1e-12
    (1e-4 of the error of 1e-8 itself)."""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "problem/linear_wave/wave_flag=%d" % wave_flag,
          "problem/linear_wave/vflow=%g" % vflow]
    s = _sim("linear_wave_mhd3d", ov, strict=strict).initialize()
    o = oracle.Sim(fluid="glmmhd", recon="ppm", riemann="hlld", integrator="rk3", nx=(32, 16, 16), mb=(16, 16, 16), ng=3,
                   xmax=(3.0, 1.5, 1.5), cfl=0.3, gamma=GAMMA_DECK, nthreads=os.cpu_count())
    o.pgen("linear_wave_mhd", wave_flag=wave_flag, amp=1e-6, vflow=vflow)
    assert s.tlim == o.period  # "test = true": one wave period
    _assert_same(s.gather("cons"), o.gather_cons(), strict)      # the problem generator (host arithmetic; FMAs in the product build)
    if strict:
        assert s.dt == o.dt
    n_gpu = s.run()
    n_cpu = o.run(o.period)
    assert n_gpu == n_cpu
    # Product build (FMA contraction, reciprocal-based divides): a 1e-6 wave on an O(1) background puts PPM's extremum
    # tests within round-off of their thresholds in a few cells per cycle; a flipped limiter branch moves a cell by
    # ~1e-10 (1 % of the truncation error), so after a period the two builds sit up to ~1e-10 apart (measured: 1e-12
    # after one cycle, 1.2e-10 after the slow wave's 143).  Bound: 1e-3 of the wave amplitude.  What north_star bounds
    # -- the L1 error norm -- is compared to 1e-12 below.
    if strict:
        _assert_same(s.gather("cons"), o.gather_cons(), True)
    else:
        assert np.max(np.abs(s.gather("cons") - o.gather_cons())) <= 1e-9
    rms, l1, mx = s.linear_wave_mhd_errors()
    rms_o, l1_o, mx_o = o.linear_wave_errors()
    assert l1.shape == (8,) and rms_o > 1e-10
    assert abs(rms - rms_o) <= 1e-12 and np.all(np.abs(l1 - l1_o) <= 1e-12) and np.all(np.abs(mx - mx_o) <= 1e-9)
    if strict:
        assert rms == rms_o and np.array_equal(l1, l1_o) and np.array_equal(mx, mx_o)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("family", ["fast", "alfven", "slow", "entropy", "fast_plus"])
def test_mhd_linear_wave_reproduces_the_frozen_numbers(family, strict):
    """The same runs against tests/golden/mhd_linear_wave.json (made by tests/golden/make_mhd_linear_wave.py from the
    oracle): no live oracle involved.  Parity build: cycle count, time step, every error norm and the final conserved
    state bit for bit; product build: the L1 norms within north_star's 1e-12."""
    import hashlib
    with open(os.path.join(GOLD, "mhd_linear_wave.json")) as f:
        g = json.load(f)["cases"][family]
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "problem/linear_wave/wave_flag=%d" % g["wave_flag"],
          "problem/linear_wave/vflow=%g" % g["vflow"]]
    s = _sim("linear_wave_mhd3d", ov, strict=strict).initialize()
    assert s.run() == g["cycles"]
    rms, l1, mx = s.linear_wave_mhd_errors()
    want_l1 = np.array([float.fromhex(x) for x in g["l1"]])
    want_mx = np.array([float.fromhex(x) for x in g["max"]])
    if strict:
        assert s.dt == float.fromhex(g["dt"]) and rms == float.fromhex(g["rms_l1"])
        assert np.array_equal(l1, want_l1) and np.array_equal(mx, want_mx)
        assert hashlib.sha256(np.ascontiguousarray(s.gather("cons")).tobytes()).hexdigest() == g["cons_sha256"]
    else:
        assert abs(rms - float.fromhex(g["rms_l1"])) <= 1e-12 and np.all(np.abs(l1 - want_l1) <= 1e-12)
        assert np.all(np.abs(mx - want_mx) <= 1e-9)
        assert "%.3e" % rms == "%.3e" % float.fromhex(g["rms_l1"])   # the figure the reference's script reads, to 4 digits


def test_mhd_linear_wave_error_file(tmp_path):
    """the MHD problem's linearwave-errors.dat: 4 + (1 + 8) + (1 + 8) columns, read the way the reference's
    convergence scripts read the file (np.genfromtxt; column 4 = RMS-L1), one row appended per run"""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "parthenon/time/tlim=0.1"]
    path = tmp_path / "linearwave-errors.dat"
    for n in range(2):
        s = _sim("linear_wave_mhd3d", ov).initialize()
        s.run()
        s.write_linear_wave_errors(path)
        rms, l1, mx = s.linear_wave_mhd_errors()
    data = np.atleast_2d(np.genfromtxt(path))
    assert data.shape == (2, 22) and tuple(data[1, :3]) == (32, 16, 16)
    assert data[1, 4] == float("%e" % rms) and data[1, 10] == float("%e" % l1[5])
    with open(path) as f:
        head = f.readline()
    assert head.startswith("# Nx1  Nx2  Nx3  Ncycle  RMS-L1-Error  d_L1") and "B3c_L1" in head and "B3c_max" in head


def test_meshblock_decomposition_and_fused_path_do_not_change_a_bit(oracle):
    base = ["parthenon/time/integrator=vl2", "parthenon/time/tlim=0.1"]
    a = _sim("linear_wave3d", base, fused=True).initialize()
    b = _sim("linear_wave3d", base + ["parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=16",
                                      "parthenon/meshblock/nx3=16"], fused=True).initialize()
    c = _sim("linear_wave3d", base, fused=False).initialize()
    # a finite velocity ceiling that never binds: the cycle keeps its primitives and the stages take their non-lean forms
    d = _sim("linear_wave3d", base + ["hydro/vceil=1e301"], fused=True).initialize()
    assert b.info.nblocks_local == 8 and a.info.fused == 1 and c.info.fused == 0
    for sim in (a, b, c, d):
        sim.run()
    assert a.prim_is_stale and not d.prim_is_stale
    ua = a.gather()
    assert np.array_equal(ua, b.gather())
    assert np.array_equal(ua, c.gather())
    assert np.array_equal(ua, d.gather())


@pytest.mark.parametrize("integrator,recon,riemann,ng", [("rk3", "ppm", "hlle", 3), ("rk3", "wenoz", "hllc", 3),
                                                         ("rk1", "dc", "llf", 2), ("vl2", "weno3", "hlle", 2),
                                                         ("rk3", "limo3", "hlle", 2)])
def test_linear_wave_method_matrix_matches_oracle(oracle, integrator, recon, riemann, ng):
    """The method combinations of the reference's convergence suite (convergence.py:33-45)."""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16",
          "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=8",
          "parthenon/mesh/nghost=%d" % ng, "parthenon/time/integrator=%s" % integrator,
          "hydro/reconstruction=%s" % recon, "hydro/riemann=%s" % riemann, "parthenon/time/tlim=0.25"]
    s = _sim("linear_wave3d", ov).initialize()
    o = oracle.Sim(fluid="euler", recon=recon, riemann=riemann, integrator=integrator, nx=(32, 16, 16), ng=ng,
                   xmax=(3.0, 1.5, 1.5), cfl=0.3, gamma=GAMMA_DECK)
    o.pgen("linear_wave", wave_flag=0, amp=1e-6)
    assert s.run() == o.run(0.25 * o.period)
    assert np.array_equal(s.gather(), o.gather_cons())


# ---- config 2: Sod 3-D, PLM + HLLC, RK2, outflow in x1 -----------------------------------------------
def test_config2_sod_matches_oracle(oracle):
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=8", "parthenon/mesh/nx3=8",
          "parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=4",
          "parthenon/time/tlim=0.1"]
    s = _sim("sod", ov).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hllc", integrator="rk2", nx=(64, 8, 8), ng=2,
                   bc=("outflow", "periodic", "periodic"), xmin=(0.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5),
                   gamma=1.4, cfl=0.3).pgen("sod")
    assert s.run() == o.run(0.1)
    assert np.array_equal(s.gather(), o.gather_cons())


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
def test_vl2_with_walls_and_outflow_matches_oracle(oracle, strict):
    """3-D hydro VL2 (donor-cell predictor + two-kernel PLM corrector) in 32^3 meshblocks with outflow in x1 and
    reflecting walls in x2: the predictor stores its conserved result only in the shell the boundary conditions and
    the ghost copies read (apk_stage_args.cons_store = 1), the full-step primitives are never stored -- against the
    oracle, which stores everything."""
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=32",
          "parthenon/meshblock/nx2=32", "parthenon/meshblock/nx3=32", "parthenon/time/integrator=vl2",
          "parthenon/mesh/ix2_bc=reflecting", "parthenon/mesh/ox2_bc=reflecting", "parthenon/time/tlim=0.05"]
    s = _sim("sod", ov, strict=strict).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hllc", integrator="vl2", nx=(64, 32, 32), mb=(32, 32, 32), ng=2,
                   bc=("outflow", "reflecting", "periodic"), xmin=(0.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5),
                   gamma=1.4, cfl=0.3).pgen("sod")
    assert s.run() == o.run(0.05)
    assert s.prim_is_stale
    _assert_same(s.gather(), o.gather_cons(), strict)
    _assert_same(np.asarray(s.dt), np.asarray(o.dt), strict)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("scheme", [("rk2", "plm", 2), ("rk3", "ppm", 3)], ids=["rk2_plm", "rk3_ppm"])
def test_rk_with_walls_and_outflow_matches_oracle(oracle, strict, scheme):
    """3-D hydro RK2 / RK3 in 32^3 meshblocks with outflow in x1 and reflecting walls in x2, no primitives stored by any
    stage (the sweeps convert the conserved rows they load, ghost zones behind physical boundaries included; stages
    with gam0 != 0 write into a third buffer) -- against the oracle, which stores everything."""
    integ, recon, ng = scheme
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=32",
          "parthenon/meshblock/nx2=32", "parthenon/meshblock/nx3=32", "parthenon/time/integrator=%s" % integ,
          "hydro/reconstruction=%s" % recon, "parthenon/mesh/nghost=%d" % ng,
          "parthenon/mesh/ix2_bc=reflecting", "parthenon/mesh/ox2_bc=reflecting", "parthenon/time/tlim=0.05"]
    s = _sim("sod", ov, strict=strict).initialize()
    o = oracle.Sim(fluid="euler", recon=recon, riemann="hllc", integrator=integ, nx=(64, 32, 32), mb=(32, 32, 32), ng=ng,
                   bc=("outflow", "reflecting", "periodic"), xmin=(0.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5),
                   gamma=1.4, cfl=0.3).pgen("sod")
    assert s.run() == o.run(0.05)
    assert s.prim_is_stale
    _assert_same(s.gather(), o.gather_cons(), strict)
    _assert_same(np.asarray(s.dt), np.asarray(o.dt), strict)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("scheme", [("rk2", "plm", 2), ("rk3", "ppm", 3)], ids=["rk2_plm", "rk3_ppm"])
def test_rk_with_a_density_floor_that_fires_in_every_stage_matches_oracle(oracle, strict, scheme):
    """Round-4 advisor (high): a prim-free RK cycle stores the results of its stages without ConsToPrim, so a density
    floor would act on the register copy the next stage converts and never reach the stored conserved state, where the
    reference's FillDerived after EVERY stage writes the floored density back (adiabatic_hydro.hpp:81).  With
    hydro/dfloor the cycle must keep its primitives.  Two receding streams (u = -/+ 2.5) empty the middle of the tube
    below the floor in every stage of every cycle; against the oracle, whose ConsToPrim floors after every stage."""
    integ, recon, ng = scheme
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=32",
          "parthenon/meshblock/nx2=32", "parthenon/meshblock/nx3=32", "parthenon/time/integrator=%s" % integ,
          "hydro/reconstruction=%s" % recon, "parthenon/mesh/nghost=%d" % ng, "hydro/dfloor=0.3",
          "problem/sod/rho_l=1.0", "problem/sod/pres_l=0.4", "problem/sod/u_l=-2.5",
          "problem/sod/rho_r=1.0", "problem/sod/pres_r=0.4", "problem/sod/u_r=2.5", "parthenon/time/tlim=0.08"]
    s = _sim("sod", ov, strict=strict).initialize()
    o = oracle.Sim(fluid="euler", recon=recon, riemann="hllc", integrator=integ, nx=(64, 32, 32), mb=(32, 32, 32), ng=ng,
                   bc=("outflow", "periodic", "periodic"), xmin=(0.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5), cfl=0.3,
                   eos=oracle.make_eos(1.4, dfloor=0.3)).pgen("sod", rho_l=1.0, pres_l=0.4, u_l=-2.5, rho_r=1.0, pres_r=0.4,
                                                             u_r=2.5)
    assert s.run() == o.run(0.08)
    assert not s.prim_is_stale                      # (the cycle stores its primitives: every stage floors what it stores)
    u = s.gather()
    assert u[0].min() == 0.3 and (u[0] == 0.3).sum() > 32 * 32  # the floor is what holds the middle up
    if strict or recon != "ppm":
        _assert_same(u, o.gather_cons(), strict)
        _assert_same(np.asarray(s.dt), np.asarray(o.dt), strict)
    else:
        # product build (FMA contraction, reciprocal seeds) with PPM: a last-bit difference decides in single cells at the
        # edge of the evacuated region whether the floor fires or an extremum test flips, and the next stages carry that
        # on (measured: up to 2.8e-3 in a few of the tube's 64 x-positions after 0.08 time units, 6e-5 of the mean state
        # averaged over the tube; 1.1e-2 / 6e-4 after round 6 changed the last bits of the sound speed and of HLLC's
        # quotients -- another realisation of the same sensitivity: product and parity build agree to 2e-15 for the first
        # four cycles in every variant and part by 1e-3 .. 2e-2 within the next four to twelve, whichever quotient forms are
        # compiled; every pointwise comparison of the product build against the oracle is unchanged at a few ulp) -- the
        # parity build above is the bit-for-bit check
        uo = o.gather_cons()
        d = np.abs(u - uo)
        assert np.max(d) < 5e-2 and np.mean(d) < 2e-3 * np.mean(np.abs(uo))
        assert s.dt == pytest.approx(o.dt, rel=1e-4)


def test_config2_full_size_sod_stays_one_dimensional():
    """256^3, 8 meshblocks of 128^3 (BASELINE config 2).  Size-independent property: a
    planar problem keeps zero transverse momentum and no transverse structure, bitwise."""
    s = _sim("sod", [], strict=False).initialize()
    assert s.info.nblocks_local == 8 and s.info.zones_total == 256 ** 3
    m0 = s.history()[0]
    s.run(nlim=3)
    u = s.gather()
    assert np.all(u[2] == 0.0) and np.all(u[3] == 0.0)
    assert np.array_equal(u[:, :1, :1, :].repeat(256, 1).repeat(256, 2), u)
    # mass changes only through the outflow faces, which carry no flux yet
    assert s.history()[0] == pytest.approx(m0, rel=1e-13)
    assert u[0].min() >= 0.125 - 1e-12 and u[0].max() <= 1.0 + 1e-12


# ---- config 3: Orszag-Tang, PPM + HLLD + Dedner, VL2 --------------------------------------------------
@pytest.mark.parametrize("fofc", [False, True], ids=["plain", "fofc"])
def test_config3_orszag_tang_conserved_totals(oracle, fofc):
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=32",
          "parthenon/meshblock/nx2=32", "parthenon/time/tlim=0.1",
          "hydro/first_order_flux_correct=%s" % ("true" if fofc else "false")]
    s = _sim("orszag_tang", ov).initialize()
    o = oracle.Sim(fluid="glmmhd", recon="ppm", riemann="hlld", integrator="vl2", nx=(64, 64, 1), ng=3,
                   xmin=(-0.5, -0.5, -0.5), xmax=(0.5, 0.5, 0.5), cfl=0.4, gamma=GAMMA_DECK, fofc=fofc).pgen("orszag_tang")
    assert s.run() == o.run(0.1)
    assert s.c_h == o.c_h
    assert np.array_equal(s.gather(), o.gather_cons())
    assert s.fofc_count == o.fofc_count
    h, ho = s.history(), o.history()
    # north_star: Orszag-Tang conserved totals (mass, momenta, total energy; hydro.cpp:172-183)
    np.testing.assert_allclose(h[[0, 4, 5, 6]], ho[[0, 4, 5, 6]], rtol=1e-12)
    assert abs(h[1] - ho[1]) < 1e-13 and abs(h[2] - ho[2]) < 1e-13


def test_config3_fma_build_totals_within_tolerance(oracle):
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=64",
          "parthenon/meshblock/nx2=64", "parthenon/time/tlim=0.1"]
    s = _sim("orszag_tang", ov, strict=False).initialize()
    o = oracle.Sim(fluid="glmmhd", recon="ppm", riemann="hlld", integrator="vl2", nx=(64, 64, 1), ng=3,
                   xmin=(-0.5, -0.5, -0.5), xmax=(0.5, 0.5, 0.5), cfl=0.4, gamma=GAMMA_DECK).pgen("orszag_tang")
    s.run()
    o.run(0.1)
    h, ho = s.history(), o.history()
    np.testing.assert_allclose(h[[0, 4, 5, 6]], ho[[0, 4, 5, 6]], rtol=1e-12)
    u, uo = s.gather(), o.gather_cons()
    assert np.max(np.abs(u - uo)) <= 1e-13 * np.max(np.abs(uo))  # product-build deviation after 38 cycles (measured: 1.9e-15)


def test_config3_full_size_orszag_tang_symmetry_and_conservation():
    """512^2 (BASELINE config 3).  Properties: mass / energy conserved to round-off and the
    solution keeps the vortex' point symmetry u(x,y) -> u(-x,-y) with (m,B) odd/even."""
    s = _sim("orszag_tang", ["hydro/first_order_flux_correct=false"], strict=False).initialize()
    assert s.info.zones_total == 512 * 512
    h0 = s.history()
    s.run(nlim=20)
    h1 = s.history()
    assert h1[0] == pytest.approx(h0[0], rel=1e-13)
    assert h1[5] == pytest.approx(h0[5], rel=1e-12)
    assert abs(h1[1]) < 1e-12 and abs(h1[2]) < 1e-12
    u = s.gather()[:, 0]
    rot = u[:, ::-1, ::-1]
    assert np.max(np.abs(u[0] - rot[0])) < 1e-11   # density: even
    assert np.max(np.abs(u[1] + rot[1])) < 1e-11   # momentum: odd


# ---- the reference's own regression bounds, on the device -------------------------------------------
def test_reference_bound_hydro_linear_wave_on_gpu():
    """convergence.py:163-164 at the reference's resolution (128x64x64, VL2+PLM+HLLE)."""
    with open(os.path.join(GOLD, "oracle_pins.json")) as f:
        pin = json.load(f)["hydro_vl2_plm_hlle_128x64x64"]
    ov = ["parthenon/mesh/nx1=128", "parthenon/mesh/nx2=64", "parthenon/mesh/nx3=64",
          "parthenon/meshblock/nx1=128", "parthenon/meshblock/nx2=64", "parthenon/meshblock/nx3=64",
          "parthenon/time/integrator=vl2"]
    s = _sim("linear_wave3d", ov, strict=False).initialize()
    assert s.run() == pin["cycles"]
    rms, _, _ = s.linear_wave_errors()
    assert float("%e" % rms) <= pin["reference_bound"]
    assert abs(rms - pin["rms_l1"]) <= 1e-12


def test_reference_bound_mhd_linear_wave_on_gpu():
    """mhd_convergence.py:167-169 (256x128x128, RK3+WENOZ+HLLE through the GLM-MHD solver)."""
    with open(os.path.join(GOLD, "oracle_pins.json")) as f:
        pin = json.load(f)["glmmhd_rk3_wenoz_hlle_256x128x128"]
    ov = ["parthenon/mesh/nx1=256", "parthenon/mesh/nx2=128", "parthenon/mesh/nx3=128",
          "parthenon/meshblock/nx1=128", "parthenon/meshblock/nx2=128", "parthenon/meshblock/nx3=128",
          "parthenon/mesh/nghost=3", "parthenon/time/integrator=rk3", "hydro/reconstruction=wenoz",
          "hydro/fluid=glmmhd"]
    s = _sim("linear_wave3d", ov, strict=False).initialize()
    assert s.run() == pin["cycles"]
    rms, _, _ = s.linear_wave_errors()
    assert rms <= pin["reference_bound"]
    assert abs(rms - pin["rms_l1"]) <= 1e-12


# ---- north-star benchmark workload at full size: properties ------------------------------------------
def test_synthetic_mhd_256_cubed_conserves_and_matches_flux_array_path():
    a = _sim("synthetic_mhd", [], strict=False, fused=True).initialize()
    assert a.info.zones_total == 256 ** 3 and a.info.nblocks_local == 8
    h0 = a.history()
    a.run(nlim=2)
    h1 = a.history()
    for q in (0, 1, 2, 3, 5):  # mass, momenta, total energy on a periodic box
        assert abs(h1[q] - h0[q]) <= 1e-12 * max(abs(h0[q]), h0[0])
    ua = a.gather()
    a.close()
    # the fused path (sweeps + in-place ConsToPrim + dt in the finishing sweep) and the flux-array
    # path (separate tasks) are the same arithmetic: bit-identical in the parity build ...
    b = _sim("synthetic_mhd", [], strict=True, fused=True).initialize()
    c = _sim("synthetic_mhd", [], strict=True, fused=False).initialize()
    b.run(nlim=2)
    c.run(nlim=2)
    ub = b.gather()
    assert b.dt == c.dt
    assert np.array_equal(ub, c.gather())
    # ... and the FMA build stays within the stated tolerance of it
    assert np.max(np.abs(ua - ub)) <= 1e-12 * np.max(np.abs(ub))


# ---- one-GPU rehearsal of a rank of the 2 x 2 x 2 run --------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("scheme", [("vl2", "ppm", 3), ("rk3", "wenoz", 3)], ids=["vl2_ppm", "rk3_wenoz"])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlapped", "synchronous"])
@pytest.mark.parametrize("x1_direct", [True, False], ids=["x1_strips_in_buffers", "x1_strips_packed"])
def test_rehearsed_remote_faces_give_the_periodic_box(strict, scheme, overlap, x1_direct):
    """apk_amd/rehearse_remote_faces: the three outer faces of every block of a 2 x 2 x 2 brick (and its edges and corner)
    go through pack -> message on the halo stream -> unpack + ghost ConsToPrim, overlapped with the next stage's x3
    sweep windows, exactly as between the bricks of the 8-GPU run; the loopback transport delivers the rank's own
    messages, which for a periodic box ARE the neighbours' -- so the run must reproduce the plain one-rank run, which
    reads every neighbour directly and copies nothing: bit for bit in the parity build.  x1_direct (the default where it
    applies -- the VL2 cycle): the x1 strips of both exchanges bypass the pack / unpack kernels (apk_sim_set_x1_direct)."""
    integ, recon, ng = scheme
    ov = ["parthenon/mesh/nx%d=64" % d for d in (1, 2, 3)] + ["parthenon/meshblock/nx%d=32" % d for d in (1, 2, 3)] + [
        "parthenon/time/integrator=%s" % integ, "hydro/reconstruction=%s" % recon, "parthenon/mesh/nghost=%d" % ng]
    a = _sim("synthetic_mhd", ov, strict=strict).initialize()
    b = _sim("synthetic_mhd", ov + ["apk_amd/rehearse_remote_faces=true"], strict=strict)
    b.set_overlap(overlap)
    b.set_x1_direct(x1_direct)
    b.initialize()
    assert a.info.npeers == 0 and b.info.npeers == 7
    for _ in range(4):
        a.step()
        b.step()
    nstages = {"vl2": 2, "rk3": 3}[integ]
    # (VL2: both exchanges of every cycle; RK3: all three but the one after the very first stage, which still reads the
    # initial condition's stored primitives -- the stages from the conserved state are the ones that follow the table)
    assert b.x1_direct_exchanges() == ((8 if integ == "vl2" else 11) if x1_direct else 0)
    assert a.skipped_local_exchanges() == 4 * nstages and b.skipped_local_exchanges() == 4 * nstages  # (same-rank faces still direct)
    assert (b.overlapped_exchanges > 0) == overlap
    assert b.thin_exchanges() == (4 if integ == "vl2" else 0)
    _assert_same(np.asarray(b.dt), np.asarray(a.dt), strict)
    _assert_same(b.gather(), a.gather(), strict)
    _assert_same(b.gather("prim"), a.gather("prim"), strict)


def test_forced_turbulence_keeps_the_x1_strips_of_the_kicked_state_packed():
    """BASELINE config 4's scheme with its forcing on, rehearsed as a rank of the 8-GPU run: the stages that are not the last
    store their x1 strips into the messages (apk_sim_set_x1_direct), the exchange after the last one -- behind the kick,
    which changes the state the strips were taken from -- packs them as before; bit for bit the run with every strip
    packed (parity build)."""
    ov = ["parthenon/mesh/nx%d=64" % d for d in (1, 2, 3)] + ["parthenon/meshblock/nx%d=32" % d for d in (1, 2, 3)] + [
        "parthenon/mesh/nghost=3", "apk_amd/rehearse_remote_faces=true", "parthenon/time/integrator=rk3", "hydro/reconstruction=wenoz",
        "hydro/riemann=hlld"]
    runs = []
    for x1 in (True, False):
        s = _sim("turbulence", ov, strict=True)
        s.set_x1_direct(x1)
        s.initialize()
        for _ in range(3):
            s.step()
        runs.append((s.x1_direct_exchanges(), np.asarray(s.dt), s.gather()))
    assert runs[0][0] == 2 * 3 - 1 and runs[1][0] == 0   # (two of the three exchanges of a cycle; not after the very first stage)
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlapped", "synchronous"])
@pytest.mark.parametrize("prim_free", [True, False], ids=["prim_free", "stored_prims"])
def test_one_layer_exchange_before_the_predictor_and_its_completion(strict, overlap, prim_free):
    """VL2 on a periodic box with remote faces: the exchange at the end of a cycle delivers one layer of ghost cells
    (apk_sim_set_thin_exchange) -- all the donor-cell predictor reads.  Same bits as with full exchanges throughout, in
    the interior and -- after an accessor has completed them -- in every ghost zone, and the run carries on from there."""
    ov = ["parthenon/mesh/nx%d=64" % d for d in (1, 2, 3)] + ["parthenon/meshblock/nx%d=32" % d for d in (1, 2, 3)] + [
        "apk_amd/rehearse_remote_faces=true"]
    sims = []
    for thin in (True, False):
        s = _sim("synthetic_mhd", ov, strict=strict)
        s.set_overlap(overlap)
        s.set_thin_exchange(thin).set_prim_free(prim_free)
        sims.append(s.initialize())
    a, b = sims
    for rounds in range(2):
        for _ in range(3):
            a.step()
            b.step()
        assert a.thin_exchanges() == 3 * (rounds + 1) and b.thin_exchanges() == 0
        assert np.array_equal(np.asarray(a.dt), np.asarray(b.dt))
        for lb in range(8):
            for field in ("cons", "prim"):
                assert np.array_equal(a.read_block(lb, field), b.read_block(lb, field)), (rounds, lb, field)  # (ghost zones included)
    full, thin = a.messages("uniform"), a.messages("uniform_thin")
    assert all(t[1] * 3 <= f[1] for f, t in zip(full, thin))  # (nghost = 3: a third of a face, a ninth of an edge)


# ---- full-step primitives kept out of memory --------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("layout", [((64, 64, 64), (32, 32, 32), []), ((64, 32, 32), (32, 32, 16), []),
                                    ((64, 64, 64), (32, 32, 32), ["apk_amd/rehearse_remote_faces=true"]),
                                    ((64, 32, 34), (32, 16, 17), [])],
                         ids=["2x2x2", "2x1x2", "rehearsed_remote_faces", "odd_nx3_and_row_pairs"])
def test_cycle_without_stored_primitives_equals_the_cycle_with_them(strict, layout):
    """VL2 on a uniform 3-D mesh: the corrector computes the new primitives for the time-step estimate only and the
    predictor of the next cycle derives its input from the conserved state (apk_sim_set_prim_free; also the conserved
    half-step state is only stored where it is read).  Same bits as the cycle that stores and re-reads everything, at
    every accessor, which materialises the primitives on demand."""
    (n1, n2, n3), (m1, m2, m3), extra = layout
    ov = ["parthenon/mesh/nx1=%d" % n1, "parthenon/mesh/nx2=%d" % n2, "parthenon/mesh/nx3=%d" % n3,
          "parthenon/meshblock/nx1=%d" % m1, "parthenon/meshblock/nx2=%d" % m2, "parthenon/meshblock/nx3=%d" % m3] + extra
    a = _sim("synthetic_mhd", ov, strict=strict).initialize()
    b = _sim("synthetic_mhd", ov, strict=strict)
    b.set_prim_free(False)
    b.initialize()
    for _ in range(3):
        a.step()
        b.step()
    assert a.prim_is_stale and not b.prim_is_stale
    _assert_same(np.asarray(a.dt), np.asarray(b.dt), strict)
    _assert_same(a.gather(), b.gather(), strict)
    _assert_same(a.gather("prim"), b.gather("prim"), strict)   # (materialised by the accessor)
    assert not a.prim_is_stale
    a.step()                                                    # the predictor reads stored primitives again ...
    b.step()
    assert a.prim_is_stale                                      # ... and the cycle ends without them
    for lb in range(a.info.nblocks_local):
        for field in ("cons", "prim"):
            _assert_same(a.read_block(lb, field), b.read_block(lb, field), strict)   # ghost zones included
    # switching it off in mid-run
    a.step()
    a.set_prim_free(False)
    b.step()
    a.step()
    b.step()
    assert not a.prim_is_stale
    _assert_same(a.gather(), b.gather(), strict)
    _assert_same(np.asarray(a.dt), np.asarray(b.dt), strict)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("scheme", [("synthetic_mhd", "rk3", "wenoz", "hlld", 3), ("synthetic_mhd", "rk2", "ppm", "hlld", 3),
                                    ("synthetic_mhd", "rk1", "plm", "hlle", 2), ("linear_wave3d", "rk2", "plm", "hllc", 2),
                                    ("linear_wave3d", "rk3", "ppm", "hlle", 3)],
                         ids=["mhd_rk3_wenoz", "mhd_rk2_ppm", "mhd_rk1_plm", "hydro_rk2_plm_hllc", "hydro_rk3_ppm"])
@pytest.mark.parametrize("layout", [((64, 64, 64), (32, 32, 32), []), ((64, 32, 32), (32, 32, 16), []),
                                    ((64, 64, 64), (32, 32, 32), ["apk_amd/rehearse_remote_faces=true"])],
                         ids=["2x2x2", "2x1x2", "rehearsed_remote_faces"])
def test_rk_cycle_without_stored_primitives_equals_the_cycle_with_them(strict, scheme, layout):
    """RK1 / RK2 / RK3 on a uniform 3-D mesh whose stages are all two-kernel stages: every stage derives its input from
    the conserved state (apk_stage_args.prim_from_cons = 1 where gam0 = 0, = 2 with the result in a third buffer where
    the stage updates its own input) and stores no primitives; the last one computes them for the time-step estimate.
    Same bits as the cycle that stores and re-reads them, at every accessor, with same-rank and with remote faces."""
    deck, integ, recon, riemann, ng = scheme
    (n1, n2, n3), (m1, m2, m3), extra = layout
    ov = ["parthenon/mesh/nx1=%d" % n1, "parthenon/mesh/nx2=%d" % n2, "parthenon/mesh/nx3=%d" % n3,
          "parthenon/meshblock/nx1=%d" % m1, "parthenon/meshblock/nx2=%d" % m2, "parthenon/meshblock/nx3=%d" % m3,
          "parthenon/time/integrator=%s" % integ, "hydro/reconstruction=%s" % recon, "hydro/riemann=%s" % riemann,
          "parthenon/mesh/nghost=%d" % ng] + extra
    # (product build: the two cycles convert the same conserved values in different kernels, whose multiply-adds contract
    # differently -- last-bit differences, and a last bit can flip one of PPM's extremum tests: a limited instead of an
    # unlimited interface value somewhere, 5e-8 of the state after three cycles of RK2 PPM, as any perturbation of that size
    # does in either build.  The parity build, first parameter, is the test of the logic.)
    same = lambda x, y, st: _assert_same(x, y, st, tol=1e-6)
    a = _sim(deck, ov, strict=strict).initialize()
    b = _sim(deck, ov, strict=strict)
    b.set_prim_free(False)
    b.initialize()
    for _ in range(3):
        a.step()
        b.step()
    assert a.prim_is_stale and not b.prim_is_stale
    same(np.asarray(a.dt), np.asarray(b.dt), strict)
    same(a.gather(), b.gather(), strict)
    same(a.gather("prim"), b.gather("prim"), strict)   # (materialised by the accessor)
    assert not a.prim_is_stale
    a.step()                                                    # stage 1 reads stored primitives again ...
    b.step()
    assert a.prim_is_stale                                      # ... and the cycle ends without them
    for lb in range(a.info.nblocks_local):
        for field in ("cons", "prim"):
            same(a.read_block(lb, field), b.read_block(lb, field), strict)   # ghost zones included
    a.step()
    a.set_prim_free(False)                                      # switching it off in mid-run
    b.step()
    a.step()
    b.step()
    assert not a.prim_is_stale
    same(a.gather(), b.gather(), strict)
    same(np.asarray(a.dt), np.asarray(b.dt), strict)


# ---- direct neighbour addressing: the uniform-mesh cycle without same-rank ghost copies ------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("scheme", [("vl2", "ppm", 3), ("rk3", "wenoz", 3), ("rk2", "plm", 2)], ids=["vl2_ppm", "rk3_wenoz", "rk2_plm"])
@pytest.mark.parametrize("layout", [((64, 64, 64), (32, 32, 32)), ((64, 32, 16), (64, 16, 16)), ((96, 16, 16), (32, 16, 16))],
                         ids=["2x2x2", "1x2x1_self_periodic", "3x1x1"])
def test_direct_neighbor_cycle_equals_the_cycle_with_ghost_copies(strict, scheme, layout):
    """On uniform 3-D meshes the stage kernels read same-rank neighbours' interiors directly and the same-rank ghost
    copies are skipped (apk_sim_skipped_local_exchanges); the cycle with the copies (switched off at run time) gives
    the same bits everywhere -- interior, time step, and the ghost zones once an accessor has brought them up to date.
    Layouts include a block that is its own periodic neighbour in two directions."""
    integ, recon, ng = scheme
    (n1, n2, n3), (m1, m2, m3) = layout
    ov = ["parthenon/mesh/nx1=%d" % n1, "parthenon/mesh/nx2=%d" % n2, "parthenon/mesh/nx3=%d" % n3,
          "parthenon/meshblock/nx1=%d" % m1, "parthenon/meshblock/nx2=%d" % m2, "parthenon/meshblock/nx3=%d" % m3,
          "parthenon/time/integrator=%s" % integ, "hydro/reconstruction=%s" % recon, "parthenon/mesh/nghost=%d" % ng]
    a = _sim("synthetic_mhd", ov, strict=strict).initialize()
    b = _sim("synthetic_mhd", ov, strict=strict)
    b.set_direct_neighbors(False)
    b.initialize()
    for _ in range(3):
        a.step()
        b.step()
    nstages = {"vl2": 2, "rk2": 2, "rk3": 3}[integ]
    assert a.skipped_local_exchanges() == 3 * nstages and b.skipped_local_exchanges() == 0
    # (Product build: a ghost cell's primitives come from the ConsToPrim fused into the copy kernel, the neighbour's
    # interior primitives from the one in the finishing sweep -- the same expressions contracted into FMAs differently,
    # equal to the last bit only in the parity build; with direct addressing both sides of a face see the same values.)
    def same(x, y):
        _assert_same(np.asarray(x), np.asarray(y), strict)
    same(a.dt, b.dt)
    same(a.time, b.time)
    for lb in range(a.info.nblocks_local):
        for field in ("cons", "prim"):
            same(a.read_block(lb, field), b.read_block(lb, field))   # ghost zones included
    # switching it off in mid-run materialises the ghost zones first
    a.set_direct_neighbors(False)
    a.step()
    b.step()
    assert a.skipped_local_exchanges() == 3 * nstages
    same(a.gather(), b.gather())
    same(a.dt, b.dt)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("scheme", [("vl2", "ppm", 3), ("rk2", "plm", 2)], ids=["vl2_ppm", "rk2_plm"])
@pytest.mark.parametrize("floors", [["hydro/dfloor=0.9", "hydro/pfloor=1.0e-8"], ["hydro/dfloor=0.9"]], ids=["dfloor_pfloor", "dfloor"])
def test_direct_neighbor_cycle_with_floors_on_a_periodic_box(strict, scheme, floors):
    """With a floor or a ceiling set, ConsToPrim is not fused into the ghost fills and a separate pass converts the ghost
    zones -- which would read the zones a table-following exchange leaves unfilled.  On one rank with every direction
    periodic the table covers every face, nothing is left to fill or convert, and the direct cycle runs all the same
    (BASELINE config 3's deck sets a pressure floor).  A density floor that fires in a fifth of the cells every stage and
    a pressure floor that never does (and the density floor alone: the lean stage forms, and VL2 without stored full-step
    primitives): the same bits as the cycle with the copies, ghost zones included."""
    integ, recon, ng = scheme
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=16", "parthenon/meshblock/nx1=32",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "parthenon/time/integrator=%s" % integ,
          "hydro/reconstruction=%s" % recon, "parthenon/mesh/nghost=%d" % ng] + floors
    a = _sim("synthetic_mhd", ov, strict=strict).initialize()
    b = _sim("synthetic_mhd", ov, strict=strict)
    b.set_direct_neighbors(False)
    b.initialize()
    for _ in range(3):
        a.step()
        b.step()
    assert a.skipped_local_exchanges() == 6 and b.skipped_local_exchanges() == 0
    rho = np.asarray(a.gather())[0]
    assert 0.02 < np.mean(rho == 0.9) < 0.6          # the floor is at work
    _assert_same(np.asarray(a.dt), np.asarray(b.dt), strict)
    for lb in range(a.info.nblocks_local):
        for field in ("cons", "prim"):
            _assert_same(np.asarray(a.read_block(lb, field)), np.asarray(b.read_block(lb, field)), strict)


# ---- config 4 forcing: few-modes turbulence driver ---------------------------------------------------
def _turb_k_vec():
    from athenapk_amd import decks
    kv, block = {}, None
    for line in decks.load("turbulence").splitlines():
        line = line.split("#")[0].strip()
        if line.startswith("<"):
            block = line.strip("<>")
        elif "=" in line and block == "modes":
            k, v = [x.strip() for x in line.split("=")]
            kv[k] = int(v)
    n = len(kv) // 3
    return np.array([[kv["k_%d_%d" % (m + 1, d)] for m in range(n)] for d in range(3)], dtype=np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
@pytest.mark.parametrize("b_config", [0, 2])
@pytest.mark.parametrize("mb1", [16, 32], ids=["16cubed_blocks", "wide_blocks"])
def test_turbulence_driver_matches_oracle(oracle, strict, b_config, mb1):
    """32^3 in 8 (4) meshblocks, 12 driven cycles.  The spectral state is bit-identical (same host RNG);
    the fields agree to round-off (the Perturb sums are reduced in a different order).  With blocks at least 16 cells
    wide the stages are the two-kernel / single-march forms that read same-rank neighbours directly and no
    exchange copies same-rank ghost zones: the kick after the last stage converts the cells it touches to
    primitives and estimates the time step itself (apk_turb_apply_fill)."""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=%d" % mb1,
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "problem/turbulence/b_config=%d" % b_config]
    s = _sim("turbulence", ov, strict=strict).initialize()
    o = oracle.Sim(fluid="glmmhd", recon="plm", riemann="hlle", integrator="vl2", nx=(32, 32, 32), mb=(mb1, 16, 16),
                   ng=2, cfl=0.3, gamma=1.0001, nthreads=os.cpu_count())
    o.pgen("turbulence", k_vec=_turb_k_vec(), b_config=b_config)
    np.testing.assert_allclose(s.gather("cons"), o.gather_cons(), rtol=1e-14, atol=0)
    for _ in range(12):
        s.step()
        o.step()
    # (round 3: 16-cell-wide blocks take the two-kernel stage as well, so both layouts read their neighbours directly)
    assert s.skipped_local_exchanges() == 24
    assert np.array_equal(s.fmft_var_hat(), o.var_hat())
    assert abs(s.time - o.time) <= 1e-13 * o.time
    np.testing.assert_allclose(s.gather("cons"), o.gather_cons(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(s.turbulence_history(), o.turb_history(), rtol=1e-10)
    np.testing.assert_allclose(s.history(), o.history(), rtol=1e-11, atol=1e-14)


@pytest.mark.gpu
def test_turbulence_reference_regression_windows():
    """The reference's turbulence regression test (tst/regression/test_suites/turbulence/
    turbulence.py:44-52): 64^3 PLM + HLLE VL2 GLM-MHD driven to t = 5 must end with a sonic Mach
    number in (0.45, 0.50) and an Alfvenic Mach number in (12.8, 13.6).  Also compared with the
    oracle's run of the same deck (tests/golden/turbulence_pin.json)."""
    import json
    pin = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbulence_pin.json")))
    s = _sim("turbulence", [], strict=False).initialize()
    n = s.run()
    ms, ma, pb = s.turbulence_history()  # unit box: volume sums are the means
    assert 0.45 < ms < 0.50
    assert 12.8 < ma < 13.6
    assert n == pin["cycles"]
    assert abs(ms - pin["Ms"]) < 1e-6 * pin["Ms"] and abs(ma - pin["Ma"]) < 1e-6 * pin["Ma"]
    h = s.history()
    assert abs(h[0] - 1.0) < 1e-12 and np.abs(h[1:4]).max() < 1e-12


# ---- text outputs in the reference's formats -------------------------------------------------------------
@pytest.mark.gpu
def test_cli_history_file_is_readable_by_the_reference_analysis(tmp_path):
    """`python -m athenapk_amd -i turbulence ...` writes parthenon.out1.hst; read it the way the
    reference's turbulence.py:42-52 does (np.genfromtxt, Ms / Ma = third / second to last column)."""
    from athenapk_amd import __main__ as cli
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=32",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "parthenon/time/tlim=0.25",
          "parthenon/output1/data_format=%.14e"]
    assert cli.main(["-i", "turbulence", "-d", str(tmp_path)] + ov) == 0
    path = os.path.join(str(tmp_path), "parthenon.out1.hst")
    head = open(path).readlines()[:2]
    assert head[0].startswith("#  History data")
    names = head[1].lstrip("#").split()
    assert names[:4] == ["[1]=time", "[2]=dt", "[3]=cycle", "[4]=nbtotal"]
    assert [n.split("=")[1] for n in names[4:]] == ["mass", "1-mom", "2-mom", "3-mom", "KE", "tot-E", "ME", "relDivB",
                                                     "Ms", "Ma", "plasma_beta"]
    data = np.genfromtxt(path)
    assert data.shape[1] == 15
    assert data[0, 0] == 0.0 and data[-1, 0] == 0.25 and len(data) == 4   # t = 0, 0.1, 0.2, tlim
    assert np.all(data[:, 3] == 4)
    assert np.all(np.abs(data[:, 4] - 1.0) < 1e-13)                       # mass
    assert data[0, -3] == 0.0 and data[-1, -3] > 0.05                      # Ms grows from rest
    assert np.all(np.diff(data[:, 8]) > 0)                                 # KE is being injected
    named = np.genfromtxt(path, names=True, skip_header=1)                 # diffusion_linwave3d.py:118 style
    assert named["1time"][-1] == 0.25 and named["13Ms"][-1] == data[-1, -3]


@pytest.mark.gpu
def test_cli_linear_wave_error_file(tmp_path, oracle):
    """convergence.py:158-163 reads linearwave-errors.dat with np.genfromtxt and checks column 4
    (RMS-L1-Error); two runs append two rows."""
    from athenapk_amd import __main__ as cli
    for nx in (16, 32):
        ov = ["parthenon/mesh/nx1=%d" % (2 * nx), "parthenon/mesh/nx2=%d" % nx, "parthenon/mesh/nx3=%d" % nx,
              "parthenon/meshblock/nx1=%d" % nx, "parthenon/meshblock/nx2=%d" % nx, "parthenon/meshblock/nx3=%d" % nx]
        assert cli.main(["-i", "linear_wave3d", "-d", str(tmp_path), "--strict"] + ov) == 0
    path = os.path.join(str(tmp_path), "linearwave-errors.dat")
    assert open(path).readline().startswith("# Nx1  Nx2  Nx3  Ncycle  RMS-L1-Error  d_L1  M1_L1")
    data = np.genfromtxt(path)
    assert data.shape == (2, 16)
    assert list(data[:, 0]) == [32, 64] and list(data[:, 1]) == [16, 32] and list(data[:, 2]) == [16, 32]
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hlle", integrator="rk2", nx=(64, 32, 32), ng=2,
                   xmax=(3.0, 1.5, 1.5), cfl=0.3, gamma=GAMMA_DECK, nthreads=os.cpu_count())
    o.pgen("linear_wave", wave_flag=0, amp=1e-6)
    n = o.run(o.period)
    rms, l1, mx = o.linear_wave_errors()
    assert data[1, 3] == n
    want = [float("%e" % v) for v in [rms] + list(l1) + [np.max(mx / l1)] + list(mx)]
    assert list(data[1, 4:]) == want
    assert data[1, 4] < data[0, 4] / 2.5   # approaching second order (PLM, 16 -> 32 cells per wavelength)


# ---- config 5's problem (blast wave) on a uniform grid + the refinement criterion of its deck -------------
@pytest.mark.gpu
def test_blast_matches_oracle_and_tags_the_shock(oracle):
    """inputs/blast.in = the reference's blast_3d_amr.in without the refined mesh: 8^3 meshblocks,
    PLM + HLLE VL2, pressure ratio 1.6e8.  Bit for bit against the oracle, and the deck's
    pressure-gradient criterion (threshold 0.1) evaluated per block equals the oracle's: blocks
    around the blast would refine, the far field would derefine."""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=8",
          "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8", "problem/blast/radius_outer=0.1",
          "problem/blast/radius_inner=0.05"]
    s = _sim("blast", ov, strict=True).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hlle", integrator="vl2", nx=(32, 32, 32), mb=(8, 8, 8), ng=2,
                   xmin=(-0.5, -0.5, -0.5), xmax=(0.5, 0.5, 0.5), cfl=0.3, gamma=GAMMA_DECK, nthreads=os.cpu_count())
    o.pgen("blast", radius_outer=0.1, radius_inner=0.05, pressure_ambient=0.001, pressure_ratio=1.6e8)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    for _ in range(12):
        s.step()
        o.step()
    assert s.time == o.time and s.dt == o.dt
    got = s.gather("cons")
    assert np.array_equal(got, o.gather_cons())
    assert np.isfinite(got).all() and got[0].min() > 0
    # the blast is centred: the solution keeps the octant symmetry of the initial state
    assert np.allclose(got[0], got[0][::-1, :, :], rtol=1e-12) and np.allclose(got[0], got[0][:, :, ::-1], rtol=1e-12)
    tags, crit = s.check_refinement()
    g = H.geom("euler", (8, 8, 8), 2)
    want = [oracle.tag("pressure_gradient", g, o.prim(s.block_gid(lb)[0]), 0.1) for lb in range(s.info.nblocks_local)]
    assert list(tags) == [w[0] for w in want] and list(crit) == [w[1] for w in want]
    assert (tags == 1).sum() >= 8 and (tags == -1).sum() >= 8
    # refine tags sit at the centre of the box
    centre = [lb for lb in range(s.info.nblocks_local) if all(c in (1, 2) for c in s.block_gid(lb)[1])]
    assert all(tags[lb] == 1 for lb in centre)


# ---- the reference's lw_implode_symmetry regression test ----------------------------------------------------
def _symmetry_error(rho):
    return float(np.max(2 * np.abs(rho - rho.T) / (rho + rho.T)))   # lw_implode_symmetry.py:64


@pytest.mark.gpu
def test_lw_implode_matches_oracle(oracle):
    """64^2 Liska-Wendroff implosion to t = 2.5 (2378 cycles), reflecting walls, PLM + HLLC VL2:
    bit for bit against the oracle, and exactly symmetric about the diagonal."""
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=64", "parthenon/meshblock/nx2=64"]
    s = _sim("lw_implode", ov, strict=True).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hllc", integrator="vl2", nx=(64, 64, 1), ng=3,
                   bc=("reflecting", "reflecting", "periodic"), xmin=(0.0, 0.0, -0.5), xmax=(0.3, 0.3, 0.5), cfl=0.4,
                   gamma=1.4)
    o.pgen("lw_implode")
    assert s.run() == o.run(2.5)
    got = s.gather("cons")
    assert np.array_equal(got, o.gather_cons())
    assert _symmetry_error(got[0, 0]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fma"])
def test_lw_implode_reference_symmetry_criterion(strict):
    """tst/regression/test_suites/lw_implode_symmetry/lw_implode_symmetry.py:57-68 on the reference's
    deck (256^2, one meshblock, t = 2.5): max 2|rho - rho^T| / (rho + rho^T) <= 1e-11.  The parity
    build is exactly symmetric; the default build contracts FMAs differently in the x1 and x2
    sweeps and has to stay inside the reference's bound."""
    s = _sim("lw_implode", [], strict=strict).initialize()
    n = s.run()
    rho = s.gather("prim")[0, 0]
    err = _symmetry_error(rho)
    assert n > 8000 and np.isfinite(rho).all() and rho.min() > 0
    assert err <= 1e-11, err
    if strict:
        assert err == 0.0


# ---- the method x initial-condition matrix of the reference's riemann_hydro regression test -----------------
_RH_METHODS = [(1024, "vl2", "plm", "hllc"), (64, "rk1", "dc", "hlle"), (64, "rk1", "dc", "hllc"),
               (64, "vl2", "plm", "hlle"), (64, "vl2", "plm", "hllc"), (64, "rk3", "weno3", "hlle"),
               (64, "rk3", "weno3", "hllc"), (64, "rk3", "limo3", "hlle"), (64, "rk3", "limo3", "hllc"),
               (64, "rk3", "ppm", "hlle"), (64, "rk3", "ppm", "hllc"), (64, "rk3", "wenoz", "hlle"),
               (64, "rk3", "wenoz", "hllc")]   # riemann_hydro.py:22-36
# Toro Sec. 10.8 tests 1, 6, 7: rho_l, u_l, p_l, rho_r, u_r, p_r, x0, t_end   (riemann_hydro.py:40-55)
_RH_ICS = {"sod_sonic": (1.0, 0.75, 1.0, 0.125, 0.0, 0.1, 0.5, 0.2),
           "stationary_contact": (1.4, 0.0, 1.0, 1.0, 0.0, 1.0, 0.5, 2.0),
           "slow_contact": (1.4, 0.1, 1.0, 1.0, 0.1, 1.0, 0.5, 2.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("ic", sorted(_RH_ICS))
def test_riemann_hydro_matrix_matches_oracle(oracle, ic):
    """1-D shock tubes with every method of the reference's riemann_hydro suite: bit for bit against
    the oracle; HLLC keeps the isolated stationary contact exactly, HLLE smears it."""
    rl, ul, pl, rr, ur, pr, x0, tend = _RH_ICS[ic]
    for nx1, integ, recon, riemann in _RH_METHODS:
        ng = 3 if recon in ("ppm", "wenoz") else 2
        ov = ["parthenon/mesh/nx1=%d" % nx1, "parthenon/mesh/nx2=1", "parthenon/mesh/nx3=1",
              "parthenon/meshblock/nx1=%d" % nx1, "parthenon/meshblock/nx2=1", "parthenon/meshblock/nx3=1",
              "parthenon/mesh/nghost=%d" % ng, "parthenon/time/integrator=%s" % integ, "parthenon/time/tlim=%r" % tend,
              "hydro/reconstruction=%s" % recon, "hydro/riemann=%s" % riemann, "problem/sod/rho_l=%r" % rl,
              "problem/sod/u_l=%r" % ul, "problem/sod/pres_l=%r" % pl, "problem/sod/rho_r=%r" % rr,
              "problem/sod/u_r=%r" % ur, "problem/sod/pres_r=%r" % pr, "problem/sod/x_discont=%r" % x0]
        s = _sim("sod", ov, strict=True).initialize()
        o = oracle.Sim(fluid="euler", recon=recon, riemann=riemann, integrator=integ, nx=(nx1, 1, 1), ng=ng,
                       bc=("outflow", "periodic", "periodic"), xmin=(0.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5), gamma=1.4,
                       cfl=0.3)
        o.pgen("sod", rho_l=rl, u_l=ul, pres_l=pl, rho_r=rr, u_r=ur, pres_r=pr, x_discont=x0)
        label = "%s %s %s %d" % (integ, recon, riemann, nx1)
        assert s.run() == o.run(tend), label
        got = s.gather("cons")
        assert np.array_equal(got, o.gather_cons()), label
        if ic == "stationary_contact":
            rho0 = np.where((np.arange(nx1) + 0.5) / nx1 < x0, rl, rr)
            drift = np.abs(got[0, 0, 0] - rho0).max()
            if riemann == "hllc":
                assert drift < 1e-13, label
            else:
                assert drift > 1e-3, label


# ---- circularly polarised Alfven wave: an exact nonlinear MHD solution with B != 0 -------------------------
@pytest.mark.gpu
def test_cpaw_matches_oracle_and_converges(oracle, tmp_path):
    """The reference's inputs/cpaw.in (64x32x32, PLM + HLLD + Dedner, VL2, one period): bit for bit
    against the oracle incl. the L1 errors of cpaw.cpp:127-186; second-order convergence from the
    half-resolution run; the CLI writes cpaw-errors.dat in the reference's layout."""
    res = {}
    for n in (16, 32):
        ov = ["parthenon/mesh/nx1=%d" % (2 * n), "parthenon/mesh/nx2=%d" % n, "parthenon/mesh/nx3=%d" % n,
              "parthenon/meshblock/nx1=%d" % n, "parthenon/meshblock/nx2=%d" % n, "parthenon/meshblock/nx3=%d" % n]
        s = _sim("cpaw", ov, strict=True).initialize()
        o = oracle.Sim(fluid="glmmhd", recon="plm", riemann="hlld", integrator="vl2", nx=(2 * n, n, n), mb=(n, n, n),
                       ng=2, xmax=(3.0, 1.5, 1.5), cfl=0.3, gamma=GAMMA_DECK)
        o.pgen("cpaw")
        assert np.array_equal(s.gather("cons"), o.gather_cons())
        assert s.run() == o.run(1.0)
        assert np.array_equal(s.gather("cons"), o.gather_cons())
        rms, err = s.cpaw_errors()
        rms_o, err_o = o.cpaw_errors()
        assert rms == rms_o and np.array_equal(err, err_o)
        res[n] = rms
    assert 3.5 < res[16] / res[32] < 4.5          # second order
    from athenapk_amd import __main__ as cli
    assert cli.main(["-i", "cpaw", "-d", str(tmp_path), "--strict"]) == 0
    path = os.path.join(str(tmp_path), "cpaw-errors.dat")
    assert open(path).readline().startswith("# Nx1  Nx2  Nx3  Ncycle  RMS-Error  d  M1  M2  M3  E  B1c  B2c  B3c")
    row = np.genfromtxt(path)
    assert list(row[:3]) == [64, 32, 32] and row[4] == float("%e" % res[32])


# ---- extended Dedner source through the fused path (out-of-place FillDerived) ---------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["vl2", "rk3"])
def test_extended_dedner_source_matches_oracle(oracle, integrator):
    """hydro/glmmhd_source = dedner_extended (dedner_source.cpp:42-74 with the extra momentum /
    energy terms): the source reads neighbouring primitives, so the fused stage writes the new
    primitives out of place; 3-D, 8 meshblocks, bit for bit against the oracle."""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "hydro/glmmhd_source=dedner_extended",
          "parthenon/time/integrator=%s" % integrator]
    s = _sim("synthetic_mhd", ov, strict=True).initialize()
    o = oracle.Sim(fluid="glmmhd", recon="ppm", riemann="hlld", integrator=integrator, nx=(32, 32, 32), mb=(16, 16, 16),
                   ng=3, cfl=0.3, gamma=GAMMA_DECK, dedner_extended=True)
    o.pgen("synthetic")
    for _ in range(5):
        s.step()
        o.step()
    assert s.time == o.time and s.dt == o.dt
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert np.array_equal(s.gather("prim"), np.stack([_gather_prim(o)])[0])


def _gather_prim(o):
    nb = [o.params.nx[d] // o.params.mb[d] for d in range(3)]
    ng = o.params.ng
    out = np.zeros((o.geom.nvar, o.params.nx[2], o.params.nx[1], o.params.nx[0]))
    for b in range(o.nblocks):
        bi, bj, bk = b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])
        m = o.params.mb
        out[:, bk * m[2]:(bk + 1) * m[2], bj * m[1]:(bj + 1) * m[1], bi * m[0]:(bi + 1) * m[0]] = \
            o.prim(b)[:, ng:-ng, ng:-ng, ng:-ng]
    return out


# ---- passive scalars through the driver (fused path) ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("integrator,recon", [("vl2", "ppm"), ("rk3", "wenoz")])
def test_passive_scalars_fused_driver_matches_oracle(oracle, integrator, recon):
    """hydro/nscalars = 2 on 8 meshblocks: fused stages (incl. the single-march donor-cell predictor
    of VL2) carry the scalars; bit for bit against the oracle, and the scalar masses are conserved."""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "hydro/nscalars=2",
          "parthenon/time/integrator=%s" % integrator, "hydro/reconstruction=%s" % recon]
    s = _sim("synthetic_mhd", ov, strict=True).initialize()
    assert s.info.nscalars == 2
    o = oracle.Sim(fluid="glmmhd", recon=recon, riemann="hlld", integrator=integrator, nx=(32, 32, 32), mb=(16, 16, 16),
                   ng=3, cfl=0.3, gamma=GAMMA_DECK, nscalars=2)
    o.pgen("synthetic")
    c0 = s.gather("cons")
    assert np.array_equal(c0, o.gather_cons()) and np.abs(c0[9:]).min() > 0
    for _ in range(4):
        s.step()
        o.step()
    got = s.gather("cons")
    assert np.array_equal(got, o.gather_cons())
    assert np.allclose(got[9:].sum(axis=(1, 2, 3)), c0[9:].sum(axis=(1, 2, 3)), rtol=1e-13)


# ---- the reference's advection_3d.in on a uniform grid ----------------------------------------------------------
@pytest.mark.gpu
def test_advection_matches_oracle_and_tags_the_blob(oracle):
    """One crossing of the box diagonal (tlim = 1 -> sqrt(3)/|v|), 8^3 meshblocks, PLM + HLLE VL2:
    bit for bit against the oracle; mass conserved; the deck's max-density criterion tags the
    blocks that hold the blob."""
    s = _sim("advection_3d", ["parthenon/mesh/refinement=none"], strict=True).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hlle", integrator="vl2", nx=(32, 32, 32), mb=(8, 8, 8), ng=2,
                   xmin=(-0.5,) * 3, xmax=(0.5,) * 3, cfl=0.3, gamma=GAMMA_DECK)
    o.pgen("advection", vx=1.0, vy=1.0, vz=1.0, rho_ratio=1.01, rho_radius=0.0625, rho_fraction_edge=0.01)
    c0 = s.gather("cons")
    assert np.array_equal(c0, o.gather_cons())
    tags0, crit0 = s.check_refinement()
    assert (tags0 == 1).sum() == 8 and crit0.max() > 1.3      # the blob sits in the 8 central blocks
    assert s.tlim == pytest.approx(1.0, rel=1e-12)             # sqrt(3) / sqrt(3)
    assert s.run() == o.run(s.tlim)
    got = s.gather("cons")
    assert np.array_equal(got, o.gather_cons())
    assert abs(got[0].sum() - c0[0].sum()) < 1e-10 * c0[0].sum()
    tags, crit = s.check_refinement()
    g = H.geom("euler", (8, 8, 8), 2)
    want = [oracle.tag("maxdensity", g, o.prim(s.block_gid(lb)[0]), 1.0001, 1.00005) for lb in range(s.info.nblocks_local)]
    assert list(tags) == [w[0] for w in want] and list(crit) == [w[1] for w in want]


# ---- field loop advection (src/pgen/field_loop.cpp, tst/regression/test_suites/field_loop) ---------------
FIELD_LOOP_METHODS = [("rk1", "dc", 2), ("vl2", "plm", 2), ("rk3", "ppm", 3), ("rk3", "weno3", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("integrator,recon,ng", FIELD_LOOP_METHODS)
def test_field_loop_method_matrix_matches_oracle(oracle, integrator, recon, ng):
    """the four method configurations of field_loop.py:35-40 at its lowest resolution (64x32 in 32x32
    blocks, HLLE + plain Dedner, alpha 0.4): state, dt sequence, history row and UserRelDivB bit for bit"""
    ov = ["parthenon/mesh/nx1=64", "parthenon/meshblock/nx1=32", "parthenon/mesh/nx2=32", "parthenon/meshblock/nx2=32",
          "parthenon/time/integrator=%s" % integrator, "hydro/reconstruction=%s" % recon,
          "parthenon/mesh/nghost=%d" % ng, "parthenon/time/tlim=0.25"]
    s = _sim("field_loop", ov, strict=True).initialize()
    o = oracle.Sim(fluid="glmmhd", recon=recon, riemann="hlle", integrator=integrator, nx=(64, 32, 1), mb=(32, 32, 1),
                   ng=ng, xmin=(-1.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5), cfl=0.3, gamma=GAMMA_DECK, glmmhd_alpha=0.4)
    o.pgen("field_loop", rad=0.3, amp=1e-3, vflow=1.0, iprob=1)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert s.user_reldivb() < 1e-13
    assert s.run() == o.run(0.25)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert np.allclose(s.history(), o.history(), rtol=1e-13, atol=1e-300)
    assert abs(s.user_reldivb() - o.user_reldivb(1e-3)) <= 1e-12 * o.user_reldivb(1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("iprob", [1, 2, 3, 4, 5])
def test_field_loop_3d_variants_match_oracle(oracle, iprob):
    """iprob 1-5 in 3-D (cylinders along each axis, the rotated cylinder, the sphere)"""
    ov = ["parthenon/mesh/nx1=32", "parthenon/meshblock/nx1=16", "parthenon/mesh/nx2=16", "parthenon/meshblock/nx2=16",
          "parthenon/mesh/nx3=16", "parthenon/meshblock/nx3=8", "problem/field_loop/iprob=%d" % iprob,
          "parthenon/time/tlim=0.05"]
    s = _sim("field_loop", ov, strict=True).initialize()
    o = oracle.Sim(fluid="glmmhd", recon="plm", riemann="hlle", integrator="vl2", nx=(32, 16, 16), mb=(16, 16, 8),
                   ng=2, xmin=(-1.0, -0.5, -0.5), xmax=(1.0, 0.5, 0.5), cfl=0.3, gamma=GAMMA_DECK, glmmhd_alpha=0.4)
    o.pgen("field_loop", rad=0.3, amp=1e-3, vflow=1.0, iprob=iprob)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert np.abs(s.gather("cons")[5:8]).max() > 2e-4
    assert s.run() == o.run(0.05)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert abs(s.user_reldivb() - o.user_reldivb(1e-3)) <= 1e-12 * o.user_reldivb(1e-3)


@pytest.mark.gpu
def test_cli_field_loop_history_columns(tmp_path):
    """the reference's analysis reads Emag = column 10 and UserRelDivB = column 12 of <outname>.out1.hst
    (field_loop.py:139-143); product (FMA) build, the deck as shipped but a shorter run"""
    from athenapk_amd import __main__ as cli
    assert cli.main(["-i", "field_loop", "-d", str(tmp_path), "parthenon/job/problem_id=128_vl2_plm",
                     "parthenon/time/tlim=0.5"]) == 0
    path = os.path.join(str(tmp_path), "128_vl2_plm.out1.hst")
    names = [n.split("=")[1] for n in open(path).readlines()[1].lstrip("#").split()]
    assert names[10] == "ME" and names[11] == "relDivB" and names[12] == "UserRelDivB"
    data = np.genfromtxt(path)
    assert data.shape == (11, 13) and data[-1, 0] == 0.5
    assert np.all(data[:, 3] == 4)                                    # 128x64 in 64x32 blocks
    assert data[0, 12] < 1e-13 and np.all(data[1:, 12] > 0) and np.all(data[1:, 12] < 0.2)
    emag = data[:, 10] / data[0, 10]
    assert np.all(np.diff(emag) < 0) and emag[-1] > 0.8               # slow numerical decay only
    assert np.all(np.abs(data[:, 4] - 2.0) < 1e-12)                   # mass


# ---- Kelvin-Helmholtz (src/pgen/kh.cpp; inputs/kh-shear-lecoanet_2d.in) ------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("iprob", [2, 3, 4, 5])
def test_kh_matches_oracle(oracle, iprob):
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=32",
          "problem/kh/iprob=%d" % iprob, "problem/kh/a=0.01", "problem/kh/sigma=0.1", "problem/kh/drat=2.0",
          "parthenon/time/tlim=0.05"]
    s = _sim("kh-shear-lecoanet_2d", ov, strict=True).initialize()
    o = oracle.Sim(fluid="euler", recon="plm", riemann="hlle", integrator="vl2", nx=(32, 64, 1), mb=(16, 32, 1), ng=2,
                   xmin=(-0.5, -1.0, -0.5), xmax=(0.5, 1.0, 0.5), cfl=0.4, gamma=GAMMA_DECK)
    o.pgen("kh", iprob=iprob, vflow=1.0, amp=0.01, a=0.01, sigma=0.1, drat=2.0)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert s.run() == o.run(0.05)
    assert np.array_equal(s.gather("cons"), o.gather_cons())


@pytest.mark.gpu
def test_kh_lecoanet_keeps_its_shift_reflect_symmetry():
    """the reference builds the initial condition so that x1 -> x1 + 1/2, x2 -> -x2 maps the flow onto
    itself exactly (kh.cpp:152-188): the deck as shipped (128 x 256, PLM + HLLE, VL2) keeps it to
    round-off while the layers roll up"""
    s = _sim("kh-shear-lecoanet_2d", ["parthenon/time/tlim=0.5"], strict=True).initialize()
    s.run()
    u = s.gather("cons")[:, 0]
    shifted = np.roll(u[:, ::-1, :], 64, axis=2)
    assert np.abs(u[0] - shifted[0]).max() < 1e-12 and np.abs(u[2] + shifted[2]).max() < 1e-12
    assert np.abs(u[2]).max() > 0.01              # the perturbation is there (and growing)


# ---- first-order flux correction that actually corrects: optimistic fused stage + fallback ------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fluid,recon,riemann,integrator,pr,drat,rin", [("euler", "wenoz", "hllc", "vl2", 1e10, 100.0, 0.1),
                                                                        ("glmmhd", "ppm", "hlld", "vl2", 1e12, 1.0, 0.0),
                                                                        ("euler", "ppm", "hllc", "rk3", 1e10, 0.01, 0.0),
                                                                        ("euler", "wenoz", "hllc", "rk2", 1e10, 100.0, 0.1),
                                                                        ("glmmhd", "wenoz", "hlld", "rk3", 1e11, 1.0, 0.0)])
def test_first_order_flux_correction_with_fallback_matches_oracle(oracle, fluid, recon, riemann, integrator, pr, drat, rin):
    """a blast strong enough that the high-order update leaves cells with negative pressure: with
    hydro/first_order_flux_correct every stage runs fused first (a stage with gam0 != 0 -- the later
    stages of RK2 / RK3 -- writes its trial result into a third buffer so that the old u0 survives)
    and is redone through CalculateFluxes -> FirstOrderFluxCorrect -> update only when the finishing
    sweep's admissibility test finds a bad cell; both kinds of stages occur here, and the run equals
    the oracle's (which always takes the reference's sequence) bit for bit, corrected-cell count
    included"""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "hydro/first_order_flux_correct=true",
          "problem/blast/radius_outer=0.1", "problem/blast/radius_inner=%r" % rin, "problem/blast/pressure_ratio=%r" % pr,
          "problem/blast/density_ratio=%r" % drat,
          "hydro/fluid=%s" % fluid, "hydro/reconstruction=%s" % recon, "hydro/riemann=%s" % riemann,
          "parthenon/time/integrator=%s" % integrator, "parthenon/mesh/nghost=3", "parthenon/time/cfl=0.45"]
    s = _sim("blast", ov, strict=True).initialize()
    o = oracle.Sim(fluid=fluid, recon=recon, riemann=riemann, integrator=integrator, nx=(32, 32, 32), mb=(16, 16, 16), ng=3,
                   xmin=(-0.5, -0.5, -0.5), xmax=(0.5, 0.5, 0.5), cfl=0.45, gamma=GAMMA_DECK, fofc=True,
                   nthreads=os.cpu_count())
    o.pgen("blast", radius_outer=0.1, radius_inner=rin, pressure_ambient=0.001, pressure_ratio=pr, density_ratio=drat)
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    ncyc = 30
    for _ in range(ncyc):
        s.step()
        o.step()
    assert s.time == o.time and s.dt == o.dt
    assert np.array_equal(s.gather("cons"), o.gather_cons())
    assert s.fofc_count == o.fofc_count and s.fofc_count > 0
    nstages = {"vl2": 2, "rk2": 2, "rk3": 3}[integrator]
    assert 0 < s.fofc_fallback_stages < ncyc * nstages                   # some trial stages stood, some were redone
    # (one rank, periodic: the trial stages follow the face table, and a rejected one fills the ghost zones it left stale
    # before the flux arrays' sweeps read them)
    assert s.skipped_local_exchanges() == ncyc * nstages - s.fofc_fallback_stages


# ---- the product build's arithmetic on hard data ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fluid,riemann", [("glmmhd", "hlld"), ("glmmhd", "hlle"), ("euler", "hllc")])
@pytest.mark.parametrize("recon,ng", [("ppm", 3), ("wenoz", 3), ("plm", 2)])
def test_product_build_stays_finite_and_close_on_blasts(fluid, riemann, recon, ng):
    """A blast in a medium at rest with B = 0 exactly: fields that are identically zero and states
    that are exactly uniform put every guarded 0/0 of the limiters and of HLLD to work.  The product
    build (FMA contraction, reciprocal-based divides and roots) must stay finite and within 1e-9 of
    the parity build over 25 cycles.  (Regression test: reciprocal math together with
    -fno-honor-nans / -fno-honor-infinities turned guarded 0/0 into NaNs for GLM-MHD + PPM.)"""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=16",
          "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16", "problem/blast/radius_outer=0.1",
          "problem/blast/radius_inner=0.1", "problem/blast/pressure_ambient=1.0", "problem/blast/pressure_ratio=100",
          # off the mesh's symmetry planes: with mirror-symmetric data the limiters sit on exact ties and a
          # last-bit difference between the builds flips a branch (1e-6 in a cell pair, then in dt)
          "problem/blast/x1_0=0.013", "problem/blast/x2_0=-0.021", "problem/blast/x3_0=0.007",
          "hydro/fluid=%s" % fluid, "hydro/riemann=%s" % riemann, "hydro/reconstruction=%s" % recon,
          "parthenon/mesh/nghost=%d" % ng]
    runs = []
    for strict in (False, True):
        s = _sim("blast", ov, strict=strict).initialize()
        for _ in range(25):
            s.step()
        runs.append((s.time, s.gather("cons")))
    (tf, uf), (ts, us) = runs
    assert np.isfinite(uf).all() and uf[0].min() > 0
    assert abs(tf - ts) < 1e-12 * ts
    nh = 5
    for n in range(nh):
        assert np.abs(uf[n] - us[n]).max() < 1e-9 * max(np.abs(us[n]).max(), 1e-30)


PRODUCT_DECKS = {
    "linear_wave3d": ["parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"],
    "sod": ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/meshblock/nx1=32",
            "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"],
    "orszag_tang": ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=32"],
    "blast": ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32"],
    "lw_implode": ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=32"],
    "cpaw": [],
    "advection_3d": ["parthenon/mesh/refinement=none"],
    "field_loop": [],
    "kh-shear-lecoanet_2d": ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=128", "parthenon/meshblock/nx1=32",
                             "parthenon/meshblock/nx2=64"],
    "turbulence": ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=16",
                   "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"],
    "blast_3d_amr": [],
}


@pytest.mark.gpu
@pytest.mark.parametrize("deck", sorted(PRODUCT_DECKS))
def test_every_deck_runs_in_the_product_build_close_to_the_parity_build(deck):
    """20 cycles of every shipped deck (scaled down) in the product build: finite, positive, and within
    1e-6 of the parity build (problems with exact mirror symmetries sit on limiter ties, where last-bit
    differences show at 1e-7; everything else agrees to 1e-12)"""
    ov = PRODUCT_DECKS[deck]
    out = []
    for strict in (False, True):
        s = _sim(deck, ov, strict=strict).initialize()
        for _ in range(20):
            s.step()
        i = s.refresh_info()
        out.append((s.time, [s.read_block(lb) for lb in range(i.nblocks_total)]))
    (tf, bf), (ts, bs) = out
    assert len(bf) == len(bs) and abs(tf - ts) <= 1e-6 * ts
    nh = 5
    for a, b in zip(bf, bs):
        assert np.isfinite(a).all() and a[0].min() > 0
        for n in range(nh):
            assert np.abs(a[n] - b[n]).max() <= 1e-6 * max(np.abs(b[n]).max(), 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("deck,extra", [("orszag_tang", []), ("lw_implode", []), ("field_loop", []), ("cpaw", []),
                                        ("linear_wave3d", []), ("blast", []), ("blast_3d_amr", []),
                                        ("kh-shear-lecoanet_2d", ["parthenon/time/tlim=1.0"])])
def test_shipped_decks_run_to_their_time_limit(tmp_path, capsys, deck, extra):
    """`python -m athenapk_amd -i <deck>` as shipped, product build, all the way to tlim (thousands of
    cycles for some): no negative state, no NaN, the performance line at the end"""
    from athenapk_amd import __main__ as cli
    assert cli.main(["-i", deck, "-d", str(tmp_path)] + extra) == 0
    out = capsys.readouterr().out
    assert "zone-cycles/wallsecond" in out and "cycle=" in out
