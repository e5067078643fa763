"""CPU tests of the <diffusion> block (no GPU): option defaults and requirements as Hydro::Initialize reads them
(src/hydro/hydro.cpp:538-702), the refusals of what this path does not implement, integrator = none as a no-op, and
the flux-array stage path (no fused stages) when diffusion is on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _plan(overrides, deck="diffusion"):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides))


def _refused(overrides, deck="diffusion"):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def test_deck_parses_with_viscosity_on():
    from athenapk_amd import lib as L
    p = _plan([])
    cfg, integ, cfl = p.diffusion_options()
    assert integ == 1 and cfl == 0.3  # diffusion/cfl defaults to parthenon/time/cfl (hydro.cpp:693-697)
    assert cfg.viscosity == L.VISCOSITY["isotropic"] and cfg.viscosity_coeff == L.DIFF_COEFF["fixed"]
    assert cfg.mom_diff_coeff == 0.25
    assert cfg.conduction == 0 and cfg.resistivity == 0
    assert p.info.fused == 0  # the stages run through the flux arrays


def test_conduction_defaults():
    p = _plan(["diffusion/conduction=anisotropic", "diffusion/conduction_coeff=fixed",
               "diffusion/thermal_diff_coeff_code=0.01", "diffusion/cfl=0.3"])
    cfg, integ, cfl = p.diffusion_options()
    assert cfg.conduction == 2 and cfg.thermal_diff_coeff == 0.01
    assert cfg.conduction_sat_prefac == 5.0 * 0.3  # conduction_sat_phi defaults to 0.3; 5 phi (hydro.cpp:595-604)
    assert cfl == 0.3
    p = _plan(["diffusion/conduction=isotropic", "diffusion/conduction_coeff=fixed",
               "diffusion/thermal_diff_coeff_code=0.01", "diffusion/conduction_sat_phi=0.2"])
    assert p.diffusion_options()[0].conduction_sat_prefac == 5.0 * 0.2


def test_integrator_none_is_a_no_op():
    p = _plan(["diffusion/integrator=none"])
    cfg, integ, cfl = p.diffusion_options()
    assert integ == 0 and cfl == 0.0
    assert p.info.fused == 1  # configured processes do nothing: the stages fuse as without <diffusion>
    # ... and a deck without the block at all
    q = _plan([], deck="linear_wave_mhd3d")
    assert q.diffusion_options()[1] == 0 and q.info.fused == 1


@pytest.mark.parametrize("overrides,needle", [
    (["diffusion/integrator=rkl2"], "rkl2"),
    (["diffusion/conduction=isotropic", "diffusion/conduction_coeff=spitzer"], "Spitzer"),
    (["diffusion/resistivity=ohmic", "diffusion/resistivity_coeff=spitzer"], "Spitzer"),
    (["parthenon/mesh/refinement=adaptive"], "refined meshes"),
    (["hydro/fluid=euler", "hydro/riemann=hllc", "diffusion/resistivity=ohmic"], "glmmhd"),
    (["hydro/fluid=euler", "hydro/riemann=hllc", "diffusion/conduction=anisotropic",
      "diffusion/conduction_coeff=fixed", "diffusion/thermal_diff_coeff_code=0.1"], "glmmhd"),
    (["hydro/reconstruction=dc", "hydro/riemann=llf"], "llf"),
    (["diffusion/conduction=isotropic"], "no coefficient is set"),
    (["diffusion/conduction=isotropic", "diffusion/conduction_coeff=fixed"], "thermal_diff_coeff_code"),
    (["diffusion/viscosity_coeff=none"], "no coefficient is set"),
    (["diffusion/conduction=spitzer"], "Unknown conduction method"),
    (["diffusion/integrator=explicit"], "unknown integration method"),
])
def test_refusals(overrides, needle):
    msg = _refused(overrides)
    assert needle in msg, msg


def test_refusals_wait_for_the_unsplit_integrator():
    # with integrator = none nothing acts, so nothing is refused for the combination (only unknown names are)
    p = _plan(["diffusion/integrator=none", "hydro/reconstruction=dc", "hydro/riemann=llf"])
    assert p.diffusion_options()[1] == 0


def test_diffusion_problem_generator_is_known():
    # every iprob that needs a field requires GLM-MHD (src/pgen/diffusion.cpp:34-36); the check runs at creation
    for ip in (0, 1, 2, 10, 20, 21, 22, 40):  # (21, 22: the rings in the other planes set field components too)
        msg = _refused(["hydro/fluid=euler", "hydro/riemann=hllc", "diffusion/viscosity=none",
                        "problem/diffusion/iprob=%d" % ip])
        assert "requires MHD" in msg
    _plan(["hydro/fluid=euler", "hydro/riemann=hllc"])  # iprob 30 with viscosity is a hydro setup
