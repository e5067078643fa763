"""CPU tests of Spitzer thermal conduction (no GPU): the diffusion_spitzer deck as Hydro::Initialize reads it
(src/hydro/hydro.cpp:567-593), the refusals, the numpy restatement (tests/spitzer_reference.py) against the older one
(tests/diffusion_reference.py) where the two overlap, and the size of the one deliberate deviation, T^(5/2) without pow."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffusion_reference as R  # noqa: E402
import helpers as H  # noqa: E402
import spitzer_cases as SC  # noqa: E402
import spitzer_reference as SP  # noqa: E402

# Units (src/units.hpp:15-54), cgs
ATOMIC_MASS_UNIT = 1.660538921e-24
K_BOLTZMANN = 1.3806488e-16


def _plan(overrides=(), deck="diffusion_spitzer"):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides))


def _refused(overrides, deck="diffusion_spitzer"):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def _deck_values(name="diffusion_spitzer"):
    """{block: {key: string}} of a deck file, read here without the driver"""
    from athenapk_amd import decks
    out, block = {}, None
    for line in decks.load(name).splitlines():
        line = line.split("#")[0].strip()
        if line.startswith("<"):
            block = line.strip("<>")
            out[block] = {}
        elif "=" in line:
            k, v = line.split("=", 1)
            out[block][k.strip()] = v.strip()
    return out


def test_deck_parses_and_converts_the_coefficient():
    from athenapk_amd import lib as L
    p = _plan()
    d = _deck_values()
    length, time, mass = (float(d["units"]["code_%s_cgs" % k]) for k in ("length", "time", "mass"))
    Y = float(d["hydro"]["He_mass_fraction"])
    # independently of the driver: 4.6e-7 erg / (s K cm) in code units, [T_code] = [T_phys] (hydro.cpp:575-581)
    energy = mass * length * length / (time * time)
    want_coeff = 4.6e-7 * (1.0 / energy) / ((1.0 / time) * (1.0 / length))
    mu = 1 / (Y * 3. / 4. + (1 - Y) * 2)
    sp = p.spitzer_options()
    assert isinstance(sp, L.SpitzerCfg)
    assert sp.coeff_code == want_coeff
    assert abs(sp.coeff_code / (4.6e-7 * time ** 3 / (mass * length)) - 1.0) < 1e-14  # (the same, as one power product)
    assert sp.mbar == mu * (ATOMIC_MASS_UNIT / mass)
    assert sp.k_boltzmann == K_BOLTZMANN / energy
    cfg, integ, cfl = p.diffusion_options()
    assert cfg.conduction == L.CONDUCTION["anisotropic"] and cfg.conduction_coeff == L.DIFF_COEFF["spitzer"]
    assert cfg.conduction_sat_prefac == 6.86 * math.sqrt(mu) * 0.3  # hydro.cpp:589-593
    assert cfg.thermal_diff_coeff == 0.0  # thermal_diff_coeff_code is not read
    assert integ == 1 and cfl == 0.3
    assert p.info.fused == 0  # the stages run through the flux arrays
    # what the deck's comment promises: the cold side (p / rho = 10) is at 1e7 K with chi about 0.01
    t_cold = sp.mbar / sp.k_boltzmann * 10.0
    chi_cold = float(SP.chi(np.float64(10.0), np.float64(1.0), spitzer=(sp.coeff_code, sp.mbar, sp.k_boltzmann)))
    assert abs(t_cold / 1.0e7 - 1.0) < 0.01 and abs(chi_cold / 0.01 - 1.0) < 0.05, (t_cold, chi_cold)


def test_other_coefficient_and_isotropic():
    p = _plan(["diffusion/spitzer_cond_in_erg_by_s_K_cm=9.2e-7", "diffusion/conduction=isotropic",
               "diffusion/conduction_sat_phi=0.2", "hydro/fluid=euler", "problem/diffusion/iprob=30",
               "diffusion/mom_diff_coeff_code=0.25"])
    q = _plan()
    assert p.spitzer_options().coeff_code == 2.0 * q.spitzer_options().coeff_code  # (a power of two: exact)
    assert p.diffusion_options()[0].conduction_sat_prefac == 6.86 * math.sqrt(p.units().mu) * 0.2
    # a deck without Spitzer has no Spitzer options
    assert _plan([], deck="diffusion").spitzer_options() is None
    assert _plan(["diffusion/conduction=none"]).spitzer_options() is None


NO_UNITS = ["diffusion/conduction=isotropic", "diffusion/conduction_coeff=spitzer"]


@pytest.mark.parametrize("overrides,deck,needle", [
    # no <units> block (the diffusion deck has none)
    (NO_UNITS, "diffusion", "Spitzer thermal conduction requires units and gas composition. Please set a 'units' block "
                            "and the 'hydro/He_mass_fraction' in the input file."),
    # <units> but no composition
    (NO_UNITS + ["units/code_length_cgs=3.0e21", "units/code_time_cgs=2.6e14", "units/code_mass_cgs=8.3e40"], "diffusion",
     "Spitzer thermal conduction requires units and gas composition"),
    (["diffusion/resistivity=ohmic", "diffusion/resistivity_coeff=spitzer"], "diffusion_spitzer", "Spitzer resistivity"),
    (["parthenon/mesh/refinement=adaptive"], "diffusion_spitzer", "refined meshes"),
    (["hydro/reconstruction=dc", "hydro/riemann=llf"], "diffusion_spitzer", "llf"),
    (["hydro/fluid=euler", "hydro/riemann=hllc", "problem/diffusion/iprob=30", "diffusion/mom_diff_coeff_code=0.25"],
     "diffusion_spitzer", "glmmhd"),  # (anisotropic conduction)
    (["diffusion/integrator=rkl2"], "diffusion_spitzer", "rkl2"),
])
def test_refusals(overrides, deck, needle):
    msg = _refused(overrides, deck)
    assert needle in msg, msg


def test_rkl2_with_a_ratio_is_accepted():
    p = _plan(["diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=200"])
    assert p.diffusion_options()[1] == 2 and p.spitzer_options() is not None


@pytest.mark.parametrize("nx", [(20, 1, 1), (9, 7, 1), (7, 6, 5)])
def test_new_restatement_equals_the_old_one_for_a_fixed_coefficient(nx):
    ng, dx = 2, (0.1, 0.07, 0.13)
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    prim = H.random_prim("glmmhd", nx, ng, seed=17 + ndim, kind="smooth", nblocks=2)
    prim[0, 5:8, ..., : nx[0] // 2] = 0.0  # some faces without a field: the TINY clamp
    rng = np.random.default_rng(5)
    flux = [rng.standard_normal(prim.shape) if d < ndim else None for d in range(3)]
    for kw in (dict(conduction="anisotropic", kappa=0.7, sat_prefac=1.5),
               dict(conduction="anisotropic", kappa=0.7, sat_prefac=1.5, viscosity="isotropic", nu=0.3, resistivity="ohmic",
                    eta=0.45),
               dict(conduction="isotropic", kappa=0.4), dict(viscosity="isotropic", nu=0.3)):
        old = R.diff_fluxes(prim, flux, nx, ng, dx, **kw)
        new = SP.diff_fluxes(prim, flux, nx, ng, dx, **kw)
        for d in range(ndim):
            assert not np.array_equal(old[d], flux[d])
            assert np.array_equal(old[d], new[d]), (kw, d)
        assert SP.diffusion_timestep(prim, nx, ng, dx, 0.35, **kw) == R.diffusion_timestep(prim, nx, ng, dx, 0.35, **kw)


def test_t_to_the_five_halves_is_within_3_ulp_of_pow():
    # three correctly rounded operations (1.5 ulp) against a good pow (1 ulp), rounded up: 3 ulp
    t = 10.0 ** np.random.default_rng(1).uniform(4.0, 9.0, 200000)
    got, ref = SP.t_pow_5_2(t), np.power(t, 2.5)
    err = np.abs(got - ref) / np.spacing(ref)
    print("max |T*T*sqrt(T) - pow(T, 2.5)|: %.2f ulp, %.3g relative" % (np.max(err), np.max(np.abs(got - ref) / ref)))
    assert np.max(err) <= 3.0
    assert np.any(got != ref)  # (the two are not the same function: hence the restatement spells it out)


def test_linearisation_ratio_of_the_restatements():
    # the measurement behind the bound of tests/test_gpu_spitzer.py::test_linearisation_ties_the_units_to_a_fixed_coefficient:
    # Spitzer against the fixed coefficient chi(T0, rho0) on a 1e-6 perturbation at the same time, both with the numpy
    # restatements
    spitzer, kappa0 = SC.lin_numbers()
    tlim = SC.lin_tlim(kappa0)
    t_a, t_b = SC.lin_cpu(tlim, spitzer=spitzer), SC.lin_cpu(tlim, kappa=kappa0)
    ratio = SC.lin_ratio(t_a, t_b)
    print("linearisation ratio %.4f, kappa0 %.6g" % (ratio, kappa0))
    assert abs(ratio / 0.1227 - 1.0) < 0.01
    # a coefficient built on the hydrogen mass instead of the atomic mass unit (0.8 % off) already shows
    t_c = SC.lin_cpu(tlim, kappa=kappa0 * 1.007947)
    assert SC.lin_ratio(t_a, t_c) > 1000.0 * ratio
