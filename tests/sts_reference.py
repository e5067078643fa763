"""numpy restatement of the reference's RKL2 super-time-stepping (test infrastructure, like diffusion_reference.py): the
reference of record for apk_rkl2_num_stages / apk_rkl2_coefficients / apk_flux_divergence / apk_rkl2_step_first /
apk_rkl2_step_other / apk_rkl2_substage_fused and for the driver's half steps.

Every expression follows the operation order of the reference's loops (src/hydro/hydro_driver.cpp):
  RKL2StepFirst   :93-126      RKL2StepOther   :128-166      AddSTSTasks   :168-344
and of this project's definition of Parthenon's FluxDivHelper (kernels_block.hip: flux_div).  The diffusive fluxes are
diffusion_reference.diff_fluxes on zeroed arrays.  Arrays are [nblocks][nvar][Nk][Nj][Ni].
"""
import math

import numpy as np

import diffusion_reference as R


def num_stages(tau, dt_diff):
    s = int(0.5 * (math.sqrt(9.0 + 16.0 * tau / dt_diff) - 1.0)) + 1
    if s % 2 == 0:
        s += 1
    return s


def mu_tilde_1(s):
    s = float(s)
    return 4. / 3. / (s * s + s - 2.)


def coefficients(s, j):
    """(mu_j, nu_j, mu_tilde_j, gamma_tilde_j); j = 1: (0, 0, mu_tilde_1, 0)"""
    if j == 1:
        return 0.0, 0.0, mu_tilde_1(s), 0.0
    sr = float(s)
    b_j = b_jm1 = b_jm2 = 1. / 3.
    w1 = 4. / (sr * sr + sr - 2.)
    out = None
    for jj in range(2, j + 1):
        q = float(jj)
        b_j = (q * q + q - 2.0) / (2 * q * (q + 1.0))
        mu = (2.0 * q - 1.0) / q * b_j / b_jm1
        nu = -(q - 1.0) / q * b_j / b_jm2
        mu_t = mu * w1
        gamma_t = -(1.0 - b_jm1) * mu_t
        out = (mu, nu, mu_t, gamma_t)
        b_jm2 = b_jm1
        b_jm1 = b_j
    return out


def stability_polynomial(s, z, coeffs=coefficients):
    """R(z) of the s-stage scheme on y' = lambda y, z = lambda tau (y0 = 1; M y = lambda y)"""
    z = np.asarray(z, dtype=np.float64)
    y0 = np.ones_like(z)
    my0 = z * y0  # tau * M Y0
    yjm2 = y0
    yjm1 = y0 + coeffs(s, 1)[2] * my0
    for j in range(2, s + 1):
        mu, nu, mu_t, gamma_t = coeffs(s, j)
        yj = mu * yjm1 + nu * yjm2 + (1.0 - mu - nu) * y0 + mu_t * (z * yjm1) + gamma_t * my0
        yjm2, yjm1 = yjm1, yj
    return yjm1


def _interior(nx, ng):
    lo = [ng if n > 1 else 0 for n in nx]
    return tuple(slice(lo[a], lo[a] + nx[a]) for a in (2, 1, 0)), lo


def flux_divergence(flux, nx, ng, dx):
    """-div F over the interior: [nblocks][nvar][nx3][nx2][nx1]"""
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    (sk, sj, si), lo = _interior(nx, ng)
    area = (dx[1] * dx[2], dx[0] * dx[2], dx[0] * dx[1])
    vol = dx[0] * dx[1] * dx[2]

    def up(sl, a):
        return slice(sl.start + a, sl.stop + a)
    f = flux[0]
    du = (area[0] * f[:, :, sk, sj, up(si, 1)] - area[0] * f[:, :, sk, sj, si])
    if ndim >= 2:
        f = flux[1]
        du = du + (area[1] * f[:, :, sk, up(sj, 1), si] - area[1] * f[:, :, sk, sj, si])
    if ndim == 3:
        f = flux[2]
        du = du + (area[2] * f[:, :, up(sk, 1), sj, si] - area[2] * f[:, :, sk, sj, si])
    return -du / vol


def step_first(y0, yjm1, yjm2, my0, s, tau, nx, ng):
    """in place on the interior of yjm1, yjm2"""
    (sk, sj, si), _ = _interior(nx, ng)
    I = (slice(None), slice(None), sk, sj, si)
    yjm1[I] = y0[I] + mu_tilde_1(s) * tau * my0[I]
    yjm2[I] = y0[I]


def step_other(y0, yjm1, yjm2, my0, myjm1, coeffs, tau, nx, ng):
    """in place on the interior of yjm1, yjm2; myjm1: flux_divergence of Yjm1's fluxes (interior extent)"""
    mu, nu, mu_t, gamma_t = coeffs
    (sk, sj, si), _ = _interior(nx, ng)
    I = (slice(None), slice(None), sk, sj, si)
    yj = mu * yjm1[I] + nu * yjm2[I] + (1.0 - mu - nu) * y0[I] + mu_t * tau * myjm1 + gamma_t * tau * my0[I]
    yjm2[I] = yjm1[I]
    yjm1[I] = yj


def substage(prim, y0, yjm1, yjm2, my0, nx, ng, dx, s, j, tau, **proc):
    """one sub-stage of AddSTSTasks without its exchange / FillDerived: ResetFluxes, CalcDiffFluxes(prim), then
    FluxDivergence + RKL2StepFirst (j = 1) or RKL2StepOther; in place on the interior of yjm1, yjm2 (and my0)"""
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    zero = [np.zeros_like(yjm1) if d < ndim else None for d in range(3)]
    flux = R.diff_fluxes(prim, zero, nx, ng, dx, **proc)
    m = flux_divergence(flux, nx, ng, dx)
    if j == 1:
        (sk, sj, si), _ = _interior(nx, ng)
        my0[(slice(None), slice(None), sk, sj, si)] = m
        step_first(y0, yjm1, yjm2, my0, s, tau, nx, ng)
    else:
        step_other(y0, yjm1, yjm2, my0, m, coefficients(s, j), tau, nx, ng)


def sts(cons, tau, dt_diff, nx, ng, dx, fill_ghosts, cons_to_prim, **proc):
    """AddSTSTasks(tau) on `cons` (updated in place, ghost zones included): fill_ghosts(cons) applies the boundary
    conditions in place, cons_to_prim(cons) returns the primitives of every cell.  cons and its primitives are in sync on
    entry and on exit.  Returns the number of sub-stages."""
    s = num_stages(tau, dt_diff)
    y0 = cons.copy()
    yjm2 = np.zeros_like(cons)
    my0 = np.zeros_like(cons)
    for j in range(1, s + 1):
        substage(cons_to_prim(cons), y0, cons, yjm2, my0, nx, ng, dx, s, j, tau, **proc)
        fill_ghosts(cons)
    return s
