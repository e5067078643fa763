"""CPU tests of the cluster problem's host side (no GPU): the options and their defaults, the constants rolled into the
gravity struct, the hydrostatic sphere's pressure profile against the numpy restatement (tests/cluster_reference.py)
and against the reference's own regression criterion, the initial state of every block from that block's own radial
mesh, the deck, and every refusal with its message."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402

EPS = np.finfo(np.float64).eps
MESH32 = ["parthenon/mesh/nx%d=32" % d for d in (1, 2, 3)] + ["parthenon/meshblock/nx%d=16" % d for d in (1, 2, 3)]
# the smallest cluster deck this path accepts without units: uniform gas in a box, every other key at its default
UNIFORM = """
<job>
problem_id = cluster
<parthenon/time>
tlim = 1.0
integrator = vl2
<parthenon/mesh>
nghost = 2
nx1 = 8
x1min = -1.0
x1max = 1.0
nx2 = 8
x2min = -1.0
x2max = 1.0
nx3 = 8
x3min = -1.0
x3max = 1.0
<parthenon/meshblock>
nx1 = 8
nx2 = 8
nx3 = 8
<hydro>
fluid = euler
gamma = 1.6666666666666667
eos = adiabatic
riemann = hlle
reconstruction = plm
<problem/cluster/gravity>
gravity_srcterm = false
<problem/cluster/uniform_gas>
init_uniform_gas = true
rho = 1.5
ux = 0.1
uy = -0.2
uz = 0.3
pres = 0.7
<problem/cluster/snia_feedback>
disabled = true
"""


def _plan(overrides=(), deck=None):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load("cluster_hse") if deck is None else deck, list(overrides))


def _refused(overrides=(), deck=None):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def _close(a, b, ulps):
    return abs(a - b) <= ulps * EPS * abs(b)


def _check_gravity(g, want):
    # r_nfw_s and g_const_nfw go through log and pow (1 ulp each side, the log's through a cancellation-free difference
    # of about 1.09 against 0.86 -- a factor 2 / 1.09 -- and a cube root that shrinks it by 3): 8 ulps cover them; the
    # other constants are products and quotients of the same numbers in the same order
    assert _close(g.r_nfw_s, want.r_nfw_s, 8) and _close(g.g_const_nfw, want.g_const_nfw, 8)
    assert g.r_bcg_s == want.r_bcg_s and g.g_const_bcg == want.g_const_bcg and g.g_const_smbh == want.g_const_smbh
    assert g.smoothing_r == want.smoothing_r


def test_the_deck_parses_with_its_parameters_converted_from_physical_units():
    p = _plan()
    o = p.cluster_options()
    u = R.DECK_UNITS
    assert o.enabled == 1 and o.gravity_srcterm == 1 and o.init_uniform_gas == 0 and o.init_uniform_b_field == 0
    assert (o.include_nfw_g, o.which_bcg_g, o.include_smbh_g) == (1, 1, 1) and o.test_he_sphere == 1
    # the constants of src/units.hpp this feature adds, in the deck's code units
    assert o.gravitational_constant == u.gravitational_constant() and o.msun == u.msun() and o.kpc == u.kpc()
    assert o.mpc == u.mpc() == 1.0 and o.km_s == u.km_s() and o.kev == u.kev()
    # the deck's numbers are the physical ones converted with those constants (decimal literals: one rounding each)
    for k, v in R.deck_parameters().items():
        assert _close(getattr(o, k), v, 2), (k, getattr(o, k), v)
    mu, mu_e = R.composition(R.DECK_HE)
    assert (o.mu, o.mu_e, o.mh, o.k_boltzmann) == (mu, mu_e, u.mh(), u.k_boltzmann())
    # defaults of the keys the deck leaves out
    assert (o.alpha_bcg_s, o.beta_bcg_s) == (0.1, 1.43)
    assert (o.test_he_sphere_r_start, o.test_he_sphere_r_end, o.test_he_sphere_n_r) == (1e-3 * u.kpc(), 4000 * u.kpc(), 4000)
    _check_gravity(o.gravity, R.deck_model()[0])
    info = p.info
    assert tuple(info.nx) == (64, 64, 64) and tuple(info.mb) == (32, 32, 32) and info.ng == 2 and info.nblocks_total == 8
    assert p.tlim == 1e-3


@pytest.mark.parametrize("units", ["deck", "cgs"])
def test_defaults_are_the_references_in_the_decks_units_and_in_cgs(units):
    if units == "deck":
        u = R.DECK_UNITS
        ov = ["units/code_length_cgs=3.0856775809623245e+24", "units/code_mass_cgs=1.98841586e+47",
              "units/code_time_cgs=3.15576e+16", "hydro/He_mass_fraction=0.25"]
    else:
        u, ov = R.Units(), []
    o = _plan(ov, UNIFORM).cluster_options()
    want = R.defaults(u)
    for k, v in want.items():
        assert getattr(o, k) == v, (k, getattr(o, k), v)
    assert (o.include_nfw_g, o.which_bcg_g, o.include_smbh_g, o.gravity_srcterm, o.test_he_sphere) == (0, 0, 0, 0, 0)
    assert (o.init_uniform_gas, o.uniform_gas_rho, o.uniform_gas_ux, o.uniform_gas_uy, o.uniform_gas_uz,
            o.uniform_gas_pres) == (1, 1.5, 0.1, -0.2, 0.3, 0.7)
    g = R.Gravity(u.gravitational_constant(), want["hubble_parameter"], False, "NONE", False, want["m_nfw_200"],
                  want["c_nfw"], want["m_bcg_s"], want["r_bcg_s"], want["m_smbh"], 0.0)
    _check_gravity(o.gravity, g)
    assert (o.gravity.include_nfw, o.gravity.which_bcg, o.gravity.include_smbh) == (0, 0, 0)
    assert o.gravity.g_const_bcg == 0.0  # BCG::NONE


def test_uniform_gas_and_uniform_field_initial_state():
    ov = ["hydro/fluid=glmmhd", "problem/cluster/uniform_b_field/init_uniform_b_field=true",
          "problem/cluster/uniform_b_field/bx=0.3", "problem/cluster/uniform_b_field/by=-0.1",
          "problem/cluster/uniform_b_field/bz=0.2"]
    got = _plan(ov, UNIFORM).pgen_block(0)
    want = R.pgen_uniform((8, 8, 8), 1.5, 0.1, -0.2, 0.3, 0.7, R.DECK_GAMMA, b=(0.3, -0.1, 0.2))
    assert got.shape == (9, 8, 8, 8) and np.array_equal(got[:8], want) and not got[8].any()
    # GLM-MHD without the block: zero field
    got = _plan(["hydro/fluid=glmmhd"], UNIFORM).pgen_block(0)
    assert np.array_equal(got[:5], R.pgen_uniform((8, 8, 8), 1.5, 0.1, -0.2, 0.3, 0.7, R.DECK_GAMMA)) and not got[5:].any()


@pytest.fixture(scope="module")
def test_profile():
    """the deck's sphere on the reference's test mesh (4000 radii, 1e-3 kpc to 4 Mpc): the code's and the restatement's"""
    u = R.DECK_UNITS
    got = _plan().he_sphere_profile(1e-3 * u.kpc(), 4000 * u.kpc(), 4000)
    grav, sph = R.deck_model()
    r, p = sph.profile(1e-3 * u.kpc(), 4000 * u.kpc(), 4000)
    return got, sph.columns(r, p), grav, sph


def test_he_sphere_profile_against_the_restatement(test_profile):
    """The two sides run the same IEEE operations in the same order and differ only where libm and numpy do: every pow
    and log is within 1 ulp of the true value on each side, so the two results of one call differ by at most 2 eps
    relative.  r has no such call: bit for bit.

    K = k_0 + k_100 pow(r / r_k, alpha_k): 2 eps from the pow, carried through one product and one sum that round
    again: 4 eps.

    g: the NFW term's log(1 + r / r_s) =: L enters as L - q, q = r / (r + r_s); a relative difference 2 eps of L is
    2 eps L / (L - q) of the term, so of g it is 2 eps A with A = [g_const_nfw L / r^2] / g, the term's share of g times
    its amplification.  A is evaluated below from the restatement (it peaks where the NFW term dominates, beyond the
    BCG).  The sums after it round again: 2 eps (A + 2).

    P: one RK4 step changes ln P by s_i = |ln P_{i+1} - ln P_i| through four evaluations of f = -rho g whose weights sum
    to one; f's relative difference is eps_f = 2 eps (1 + 3/5 + A): the pow in rho, the pow in K entering as K^(-3/5),
    and g.  A relative difference d of P itself obeys d' = -(2/5)(rho g / P) d, so it shrinks on the way in (P rises) and
    grows by at most (P_fix / P_end)^(2/5) =: amp on the way out.  Over the N = n_r - 1 steps of the recursion (1999
    inward, 2000 outward here) the differences add to at most amp * eps_f * sum_i s_i <= amp * eps_f * N * max s_i; the
    sum is what the test uses, plus 4 eps for the last step's own roundings.  rho = pow(mu P / K, 3/5) ...: 3/5 of P's and
    K's bounds plus its own pow, 2 eps, and two products."""
    got, want, grav, sph = test_profile
    r = want["r"]
    assert np.array_equal(got["r"], r)
    assert np.max(np.abs(got["K"] / want["K"] - 1)) <= 4 * EPS
    L, q = grav.nfw_terms(r)
    A = grav.g_const_nfw * L / (np.maximum(r, grav.smoothing_r) ** 2) / want["g"]
    err_g = np.abs(got["g"] / want["g"] - 1)
    assert np.all(err_g <= 2 * EPS * (A + 2)), np.max(err_g / (2 * EPS * (A + 2)))
    lnp = np.log(want["P"])
    steps = np.sum(np.abs(np.diff(lnp)))
    amp = max(1.0, float((sph.P_from_rho_K(sph.rho_fix, sph.K_from_r(sph.r_fix)) / want["P"][-1]) ** 0.4))
    bound_p = amp * 2 * EPS * (1.6 + np.max(A)) * steps + 4 * EPS
    err_p = np.max(np.abs(got["P"] / want["P"] - 1))
    print("P: max rel diff %.3e, bound %.3e (sum of |d ln P| %.2f, max A %.2f, amp %.2f)" % (err_p, bound_p, steps, np.max(A), amp))
    assert err_p <= bound_p
    bound_rho = 0.6 * (bound_p + 4 * EPS) + 4 * EPS
    assert np.max(np.abs(got["rho"] / want["rho"] - 1)) <= bound_rho
    for k in ("n", "ne", "T"):  # quotients of rho and P
        assert np.max(np.abs(got[k] / want[k] - 1)) <= bound_rho + bound_p + 4 * EPS, k
    assert np.max(np.abs(got["dP_dr"] / want["dP_dr"] - 1)) <= bound_rho + np.max(2 * EPS * (A + 2)) + 2 * EPS


def test_he_sphere_profile_against_an_rk4_on_a_geometric_mesh(test_profile):
    """the reference's own check (its cluster_hse regression): against an RK4 integration of dP/dr = -rho g on 4000
    geometrically spaced radii from 1e-3 kpc to 5 Mpc, starting at r_fix in both directions, norm(rel_err[1:-1]) / size
    <= 1e-3 for P, K, rho and g after interpolation to the profile's radii"""
    got, _, grav, sph = test_profile
    u = R.DECK_UNITS
    mesh = np.geomspace(1e-3 * u.kpc(), 5 * u.mpc(), 4000)
    r_in = np.concatenate((mesh[mesh < sph.r_fix], [sph.r_fix]))
    r_out = np.concatenate(([sph.r_fix], mesh[mesh > sph.r_fix]))
    p_fix = sph.P_from_rho_K(sph.rho_fix, sph.K_from_r(sph.r_fix))

    def rk4(radii):
        p = np.zeros(radii.size)
        p[0] = p_fix
        for i in range(radii.size - 1):
            p[i + 1] = sph.step_rk4(radii[i], radii[i + 1], p[i])
        return p

    p_in, p_out = rk4(r_in[::-1])[::-1], rk4(r_out)
    ar = np.concatenate((r_in, r_out[1:]))
    ap = np.concatenate((p_in, p_out[1:]))
    ak = sph.K_from_r(ar)
    analytic = {"P": ap, "K": ak, "rho": sph.rho_from_P_K(ap, ak), "g": grav.g_from_r(ar)}
    for k, a in analytic.items():
        interp = np.interp(got["r"], ar, a)
        rel_err = np.abs((interp - got[k]) / interp)
        norm = np.linalg.norm(rel_err[1:-1]) / rel_err.size
        print("%s: norm rel err %.3e" % (k, norm))
        assert norm <= 1e-3, (k, norm)


def test_every_block_starts_from_its_own_radial_mesh():
    """16^3 blocks: each block's initial state equals the restatement built from THAT block's radial mesh.  The
    meshes of two neighbouring blocks start at different radii, so their pressures at a shared radius differ in the last
    bits; a state built from the neighbour's mesh is not the block's.  The bound is the one of the profile test for the
    block's own recursion (2560-odd steps from r_fix = 2 Mpc inwards), with the interpolation's roundings: nothing but
    libm separates the two sides."""
    # (64 x 32 x 32 over [-0.2, 0.2] x [-0.1, 0.1]^2: the outer blocks along x1 do not touch the centre, so their meshes
    # start at another radius than their neighbours')
    p = _plan(MESH32 + ["parthenon/mesh/nx1=64", "parthenon/mesh/x1min=-0.2", "parthenon/mesh/x1max=0.2"])
    grav, sph = R.deck_model()
    info = p.info
    dx = np.array(list(info.dx))
    assert info.nblocks_local == 16
    blocks = {}
    for lb in range(16):
        gid, loc = p.block_gid(lb)
        xs = [R.cell_centres(info.xmin[d], dx[d], loc[d] * 16, 16) for d in range(3)]
        got = p.pgen_block(lb)
        r_mesh, p_mesh = p.block_he_profile(lb)
        want_mesh = sph.block_mesh(xs[0], xs[1], xs[2], dx)
        # the block's own mesh: same start, same length, same radii
        assert r_mesh.size == want_mesh[2] and r_mesh[0] == want_mesh[0]
        prof = sph.profile(*want_mesh)
        assert np.array_equal(prof[0], r_mesh)
        L, _ = grav.nfw_terms(prof[0])
        A = np.max(grav.g_const_nfw * L / (np.maximum(prof[0], grav.smoothing_r) ** 2) / grav.g_from_r(prof[0]))
        bound_p = 2 * EPS * (1.6 + A) * np.sum(np.abs(np.diff(np.log(prof[1])))) + 4 * EPS
        assert np.max(np.abs(p_mesh / prof[1] - 1)) <= bound_p
        want = R.pgen_sphere(sph, xs[0], xs[1], xs[2], dx, R.DECK_GAMMA)
        assert got.shape == want.shape and not got[1:4].any()
        assert np.max(np.abs(got[4] / want[4] - 1)) <= bound_p + 6 * EPS
        assert np.max(np.abs(got[0] / want[0] - 1)) <= 0.6 * (bound_p + 10 * EPS) + 4 * EPS
        blocks[tuple(loc)] = (xs, got, (r_mesh, p_mesh), bound_p)
    # two neighbours along x1: different meshes, and the wrong one is told apart.  The code's own mesh arrays are used
    # on both sides, so that libm does not enter the comparison: E of block a from a's mesh is bit for bit, from b's not.
    (xa, ga, ma, _), (_, _, mb, _) = blocks[(0, 0, 0)], blocks[(1, 0, 0)]
    assert ma[0][0] != mb[0][0] or ma[0].size != mb[0].size
    ra = R.radius(*xa)
    gm1 = R.DECK_GAMMA - 1.0
    assert np.array_equal(sph.P_from_r(ma, ra) / gm1, ga[4])
    assert not np.array_equal(sph.P_from_r(mb, ra) / gm1, ga[4])


def test_profile_errors_carry_the_references_wording():
    from athenapk_amd import lib as L
    p = _plan()
    with pytest.raises(L.ApkError, match=r"r\(i_fix\) to r_\(i_fix\+1\) does not contain r_fix_"):
        p.he_sphere_profile(1e-3, 1.0, 100)  # r_fix = 2 is outside
    # a block that does not reach r_fix cannot happen (the mesh is extended to it); r outside the profile is what the
    # generator raises when a cell's radius leaves the mesh: not reachable through a deck, so it is covered by the
    # stand-alone host program of tools/ (and its wording by the source)
    msg = _refused(["problem/cluster/hydrostatic_equilibrium/test_he_sphere_r_end=1.5"])
    assert "does not contain r_fix_" in msg


REFUSALS = [
    (["parthenon/mesh/refinement=static"], "parthenon/mesh/refinement"),
    (["parthenon/mesh/nx3=1", "parthenon/meshblock/nx3=1"], "parthenon/mesh/nx3"),
    (["parthenon/mesh/nx2=1", "parthenon/meshblock/nx2=1", "parthenon/mesh/nx3=1", "parthenon/meshblock/nx3=1"],
     "parthenon/mesh/nx3"),
    (["problem/cluster/agn_feedback/fixed_power=1.0"], "problem/cluster/agn_feedback/fixed_power"),
    (["problem/cluster/agn_triggering/triggering_mode=COLD_GAS"], "problem/cluster/agn_triggering/triggering_mode"),
    (["problem/cluster/magnetic_tower/alpha=20"], "problem/cluster/magnetic_tower"),
    (["problem/cluster/stellar_feedback/efficiency=1e-3"], "problem/cluster/stellar_feedback"),
    (["problem/cluster/snia_feedback/disabled=false"], "problem/cluster/snia_feedback/disabled"),
    (["problem/cluster/clips/clip_r=0.02"], "problem/cluster/clips/clip_r"),
    (["problem/cluster/clips/dfloor=1e-3"], "problem/cluster/clips/dfloor"),
    (["problem/cluster/clips/vceil=10"], "problem/cluster/clips/vceil"),
    (["problem/cluster/clips/vAceil=10"], "problem/cluster/clips/vAceil"),
    (["problem/cluster/clips/Tceil=1e9"], "problem/cluster/clips/Tceil"),
    (["problem/cluster/init_perturb/sigma_v=0.1"], "problem/cluster/init_perturb/sigma_v"),
    (["problem/cluster/init_perturb/sigma_b=0.1"], "problem/cluster/init_perturb/sigma_b"),
    (["problem/cluster/dipole_b_field/init_dipole_b_field=true"], "problem/cluster/dipole_b_field/init_dipole_b_field"),
    (["problem/cluster/reductions/cold_temp_thresh=1e5"], "problem/cluster/reductions"),
    (["problem/cluster/uniform_b_field/init_uniform_b_field=true", "problem/cluster/uniform_b_field/bx=1",
      "problem/cluster/uniform_b_field/by=0", "problem/cluster/uniform_b_field/bz=0"],
     "problem/cluster/uniform_b_field/init_uniform_b_field"),
    (["diffusion/integrator=rkl2", "diffusion/conduction=isotropic", "diffusion/conduction_coeff=fixed",
      "diffusion/thermal_diff_coeff_code=0.01", "diffusion/rkl2_max_dt_ratio=100"],
     "problem/cluster/gravity/gravity_srcterm"),
]


@pytest.mark.parametrize("overrides,key", REFUSALS, ids=[k for _, k in REFUSALS])
def test_what_is_not_built_is_refused_with_a_message_that_names_the_key(overrides, key):
    msg = _refused(overrides)
    assert key in msg, msg


def test_nx2_alone_collapsed_is_refused():
    # (a mesh with nx2 = 1 and nx3 > 1 is refused by the mesh itself or by this check: either way the run does not start)
    msg = _refused(["parthenon/mesh/nx2=1", "parthenon/meshblock/nx2=1"])
    assert "nx2" in msg or "nx3" in msg, msg


def test_snia_feedback_must_be_disabled_explicitly():
    from athenapk_amd import decks
    deck = decks.load("cluster_hse").replace("<problem/cluster/snia_feedback>\ndisabled = true\n", "")
    assert "snia_feedback" not in deck.split("# the reference enables")[1]
    assert "problem/cluster/snia_feedback/disabled" in _refused(deck=deck)


def test_unknown_bcg_type_and_missing_srcterm_key():
    assert "Unknown BCG type PLUMMER" in _refused(["problem/cluster/gravity/which_bcg_g=PLUMMER"])
    from athenapk_amd import decks
    deck = decks.load("cluster_hse").replace("gravity_srcterm    = true\n", "")
    assert "gravity_srcterm" in _refused(deck=deck)  # required, as in the reference


def test_the_sphere_needs_units_and_composition():
    """problem_id = cluster with neither the uniform-gas block nor units is refused"""
    deck = UNIFORM.replace("init_uniform_gas = true", "init_uniform_gas = false")
    msg = _refused(deck=deck)
    assert "requires units and gas composition" in msg and "problem/cluster/uniform_gas/init_uniform_gas" in msg
    from athenapk_amd import decks
    deck = decks.load("cluster_hse").replace("He_mass_fraction = 0.25\n", "")
    assert "requires units and gas composition" in _refused(deck=deck)


def test_gravity_runs_take_the_flux_array_stage_path():
    """an unsplit source acts between the update and ConsToPrim: no fused stage form"""
    assert _plan().info.fused == 0
    assert _plan(["problem/cluster/gravity/gravity_srcterm=false"]).info.fused == 1


def test_another_problems_deck_with_only_the_problem_id_switched():
    """cluster is known only together with its <problem/cluster/...> blocks: a deck that has none is told so"""
    from athenapk_amd import decks
    msg = _refused(["job/problem_id=cluster"], deck=decks.load("sod"))
    assert "unknown job/problem_id" in msg and "problem/cluster/gravity/gravity_srcterm" in msg
