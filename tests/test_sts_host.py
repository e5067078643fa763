"""CPU tests of RKL2 super-time-stepping (no GPU): the deck options, the stage count and the coefficients of the
library against the restatement (tests/sts_reference.py), the defining properties of the scheme with the library's
coefficients, and the restatement itself on the 1-D viscous Gaussian."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sts_reference as S  # noqa: E402

RKL2 = ["diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=200"]


def _plan(overrides, deck="diffusion"):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides))


def _refused(overrides, deck="diffusion"):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def test_rkl2_is_accepted_with_a_ratio():
    p = _plan(RKL2)
    cfg, integ, cfl = p.diffusion_options()
    assert integ == 2 and cfl == 0.3
    assert p.rkl2_max_dt_ratio() == 200.0
    assert p.info.fused == 0  # the hyperbolic stages run through the flux arrays
    assert p.sts_info() == (0, 0.0, False)  # nothing taken yet; sub-stages through the flux arrays by default
    assert _plan(RKL2 + ["apk_amd/sts_substage=fused"]).sts_info()[2] is True
    # the shipped deck
    q = _plan([], deck="diffusion_sts")
    assert q.diffusion_options()[1] == 2 and q.rkl2_max_dt_ratio() == 200.0
    # other integrators carry no ratio
    assert _plan([]).rkl2_max_dt_ratio() == -1.0


def test_bare_rkl2_is_refused():
    for ov in (["diffusion/integrator=rkl2"], ["diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=-1.0"],
               ["diffusion/integrator=rkl2", "diffusion/rkl2_max_dt_ratio=0"]):
        msg = _refused(ov)
        assert "rkl2" in msg and "rkl2_max_dt_ratio" in msg, msg
    assert "sts_substage" in _refused(RKL2 + ["apk_amd/sts_substage=both"])


@pytest.mark.parametrize("overrides,needle", [
    (["diffusion/conduction=isotropic", "diffusion/conduction_coeff=spitzer"], "Spitzer"),
    (["diffusion/resistivity=ohmic", "diffusion/resistivity_coeff=spitzer"], "Spitzer"),
    (["parthenon/mesh/refinement=adaptive"], "refined meshes"),
    (["parthenon/mesh/refinement=static"], "refined meshes"),
    (["hydro/fluid=euler", "hydro/riemann=hllc", "diffusion/resistivity=ohmic"], "glmmhd"),
    (["hydro/fluid=euler", "hydro/riemann=hllc", "diffusion/conduction=anisotropic",
      "diffusion/conduction_coeff=fixed", "diffusion/thermal_diff_coeff_code=0.1"], "glmmhd"),
    (["hydro/reconstruction=dc", "hydro/riemann=llf"], "llf"),
    (["diffusion/conduction=isotropic"], "no coefficient is set"),
])
def test_other_refusals_fire_with_rkl2(overrides, needle):
    msg = _refused(RKL2 + overrides)
    assert needle in msg, msg


@pytest.mark.parametrize("strict", [False, True])
def test_num_stages(strict):
    from athenapk_amd import hydro
    for r in np.concatenate([np.logspace(-3, 5, 801), [0.5, 1.0, 2.0, 2.5, 7.0, 100.0, 10.0 / 3.0]]):
        for tau, dt in ((r, 1.0), (r * 0.37, 0.37), (1.0, 1.0 / r)):
            s = hydro.rkl2_num_stages(tau, dt, strict=strict)
            assert s == S.num_stages(tau, dt), (tau, dt)
            assert s % 2 == 1
            # the RKL2 stability bound (Meyer+2014 eq. 21): an integer inequality once multiplied out
            assert (s * s + s - 2) / 4.0 >= tau / dt, (s, tau, dt)


@pytest.mark.parametrize("strict", [False, True])
def test_coefficients_bitwise(strict):
    from athenapk_amd import hydro
    for s in range(3, 100):
        for j in range(1, s + 1):
            assert hydro.rkl2_coefficients(s, j, strict=strict) == S.coefficients(s, j), (s, j)


def _lib_coeffs(s, j):
    from athenapk_amd import hydro
    return hydro.rkl2_coefficients(s, j)


@pytest.mark.parametrize("s", [3, 5, 9, 21])
def test_stability_on_the_negative_real_axis(s):
    z = np.linspace(-(s * s + s - 2) / 2.0, 0.0, 4001)
    r = S.stability_polynomial(s, z, coeffs=_lib_coeffs)
    print("s = %d: max |R| = %.17g" % (s, np.max(np.abs(r))))
    assert np.max(np.abs(r)) <= 1.0 + 1e-13


@pytest.mark.parametrize("s", [3, 5, 9, 21])
def test_second_order(s):
    # R(z) - (1 + z + z^2 / 2) = O(z^3): the scheme is second order
    z = -(2.0 ** -np.arange(4, 9))
    rem = np.abs(S.stability_polynomial(s, z, coeffs=_lib_coeffs) - (1.0 + z + 0.5 * z * z))
    order = np.polyfit(np.log(-z), np.log(rem), 1)[0]
    print("s = %d: fitted order of the remainder %.4f" % (s, order))
    assert order >= 2.99


def _gauss_l1(n):
    """the restatement on the reference's 1-D viscous Gaussian (diffusion.py: [-6, 6], outflow, D = 0.25, t = 2, the
    profile of t0 = 0.5, ratio 200): pure super-time-stepping, two half steps per cycle; L1 error of v2"""
    D, tlim, t0, amp, ratio, cfl = 0.25, 2.0, 0.5, 1e-6, 200.0, 0.3
    ng, nx = 1, (n, 1, 1)
    dx = (12.0 / n, 1.0, 1.0)
    x = -6.0 + (np.arange(-ng, n + ng) + 0.5) * dx[0]
    cons = np.zeros((1, 5, 1, 1, n + 2 * ng))
    cons[0, 0] = 1.0
    cons[0, 2, 0, 0] = amp / np.sqrt(4.0 * np.pi * D * t0) * np.exp(-(x ** 2) / (4.0 * D * t0))
    cons[0, 4] = 1.0 / 0.4 + 0.5 * cons[0, 2] ** 2

    def fill(u):
        u[..., :ng] = u[..., ng:ng + 1]
        u[..., -ng:] = u[..., -ng - 1:-ng]

    def c2p(u):
        w = u.copy()
        w[:, 1:4] = u[:, 1:4] / u[:, 0:1]
        w[:, 4] = 0.4 * (u[:, 4] - 0.5 * np.sum(u[:, 1:4] ** 2, axis=1) / u[:, 0])
        return w
    dt_diff = cfl * 0.5 * (dx[0] * dx[0] / (D + 1e-20))
    t = 0.0
    while t < tlim:
        dt = min(ratio * dt_diff, tlim - t)
        for _ in range(2):
            S.sts(cons, 0.5 * dt, dt_diff, nx, ng, dx, fill, c2p, viscosity="isotropic", nu=D)
        t += dt
    xi = x[ng:-ng]
    ref = amp / np.sqrt(4.0 * np.pi * D * (t0 + tlim)) * np.exp(-(xi ** 2) / (4.0 * D * (t0 + tlim)))
    return np.mean(np.abs(c2p(cons)[0, 2, 0, 0, ng:-ng] - ref))


def test_restatement_converges_at_second_order():
    res = [64, 128, 256]
    err = [_gauss_l1(n) for n in res]
    rate = np.polyfit(np.log(res), np.log(err), 1)[0]
    print("L1 errors", err, "rate", rate)
    assert rate <= -1.95, (err, rate)
