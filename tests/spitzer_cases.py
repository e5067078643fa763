"""Shared inputs of the Spitzer conduction tests (tests/test_spitzer_host.py, tests/test_gpu_spitzer.py): a unit system,
seeded primitives that reach every branch of the general conduction flux and of its time step, and the linearisation
experiment that ties the unit conversion to a fixed-coefficient run."""
import math

import numpy as np

import helpers as H
import spitzer_reference as SP

# Units (src/units.hpp:15-54), cgs
ATOMIC_MASS_UNIT = 1.660538921e-24
K_BOLTZMANN = 1.3806488e-16


def spitzer_numbers(length, time, mass, he_mass_fraction, cond_cgs=4.6e-7):
    """(coeff_code, mbar, k_boltzmann, mu) in code units from the cgs constants and a unit system (hydro.cpp:482-503,
    575-586)"""
    energy = mass * length * length / (time * time)
    mu = 1 / (he_mass_fraction * 3. / 4. + (1 - he_mass_fraction) * 2)
    coeff = cond_cgs * (1.0 / energy) / ((1.0 / time) * (1.0 / length))
    return coeff, mu * (ATOMIC_MASS_UNIT / mass), K_BOLTZMANN / energy, mu


# The unit system of the kernel tests: 1 kpc, 8.2e13 s, 5.3e38 g.  mbar / k_B = 1.0e7 in code units, so p / rho between
# 0.01 and 10 is 1e5 K to 1e8 K, and chi(1e7 K, rho = 1) = 0.5: the temperatures span three decades through the units
# while every code-unit number stays of order one.
COEFF, MBAR, KB, MU = spitzer_numbers(3.085677580962325e21, 8.2e13, 5.3e38, 0.25)
SPITZER = (COEFF, MBAR, KB)
SAT_PHI = 0.3
SAT_PREFAC = 6.86 * math.sqrt(MU) * SAT_PHI  # hydro.cpp:589-593

NG = 2
# two blocks each: partial waves, an x1-face count (13 x 6) that is no multiple of 256, more than one wave per row in 1-D
SHAPES = {3: (12, 6, 5), 2: (12, 6, 1), 1: (70, 1, 1)}
DX = (0.1, 0.07, 0.13)


def ndim_of(nx):
    return 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)


def make_prim(nx, seed, nblocks=2):
    """GLM-MHD primitives [nblocks][9][Nk][Nj][Ni] incl. ghost zones: smooth random fields, log10(p / rho) between -2 and
    1, a slab of uniform temperature (cells and faces with no gradient) and a slab without a field (the TINY clamp)"""
    prim = H.random_prim("glmmhd", nx, NG, seed=seed, kind="smooth", nblocks=nblocks)
    rng = np.random.default_rng(seed + 7)
    _, _, nk, nj, ni = prim.shape
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    for b in range(nblocks):
        ph = rng.uniform(0, 2 * np.pi)
        log_t = -0.5 + 1.45 * np.sin(2 * np.pi * (1.3 * i / ni + 0.6 * j / max(nj, 2) + 0.3 * k / max(nk, 2)) + ph)
        log_t = np.clip(log_t + 0.05 * rng.standard_normal(log_t.shape), -2.0, 1.0)
        prim[b, 4] = prim[b, 0] * 10.0 ** log_t
    a = int(0.6 * ni)
    prim[:, 0, ..., a:a + 5] = 1.25
    prim[:, 4, ..., a:a + 5] = 2.5
    c = int(0.2 * ni)
    prim[:, 5:8, ..., c:c + 4] = 0.0
    return prim


def branch_report(prim, nx, conduction):
    """what the numpy side finds in `prim`: counts of faces with flux_classic > 0, < 0, == 0, of faces whose field is
    below TINY, and of time-step cells by saturation ratio and gradient"""
    out = {"pos": 0, "neg": 0, "zero": 0, "tiny_b": 0}
    for d in range(ndim_of(nx)):
        c = SP.conduction_faces(prim, nx, NG, DX, d, conduction, 0.0, SAT_PREFAC, SPITZER)
        out["pos"] += int(np.sum(c["fc"] > 0.0))
        out["neg"] += int(np.sum(c["fc"] < 0.0))
        out["zero"] += int(np.sum(c["fc"] == 0.0))
        if conduction == "anisotropic":
            out["tiny_b"] += int(np.sum(c["bmag"] < SP.TINY))
    t = SP.cond_dt_cells(prim, nx, NG, DX, conduction, 0.0, SAT_PREFAC, SPITZER)
    out["flat_cells"] = int(np.sum(t["gradTmag"] == 0.0))
    if conduction == "anisotropic":
        live = (t["gradTmag"] != 0.0) & (t["bmag"] != 0.0)
        out["ratio_below_1"] = int(np.sum(live & (t["ratio"] < 1.0)))
        out["ratio_above_100"] = int(np.sum(live & (t["ratio"] > 100.0)))
        out["no_field_cells"] = int(np.sum(t["bmag"] == 0.0))
    temp = MBAR / KB * prim[:, 4] / prim[:, 0]
    out["t_min"], out["t_max"] = float(np.min(temp)), float(np.max(temp))
    return out


# ---- linearisation: Spitzer against a fixed coefficient on a small perturbation ----------------------------------------
# 1-D, 64 cells on [-6, 6], periodic, rho = 1, v = 0, B = (1, 0, 0), gamma = 2 (so e = p), pure conduction with RK1:
# T = T0 (1 + delta G(x)), G a unit Gaussian.  With Spitzer chi varies by 2.5 delta around chi(T0); a fixed-coefficient
# run with kappa0 = chi(T0, rho0) differs from it only through that variation.  Both runs end at the same time,
# LIN_CYCLES diffusive limits of kappa0: after a fixed number of cycles instead, each of its own limit ~ dx^2 / kappa, a
# wrong coefficient would go unnoticed (kappa t stays the same).
LIN_N, LIN_XMIN, LIN_XMAX = 64, -6.0, 6.0
LIN_T0, LIN_DELTA, LIN_CYCLES, LIN_CFL = 10.0, 1e-6, 300, 0.3
LIN_SAT_PHI = 1e10  # saturation off: flux_sat / (flux_sat + |flux_classic|) = 1 to below 1e-15


def lin_profile():
    x = LIN_XMIN + (np.arange(LIN_N) + 0.5) * (LIN_XMAX - LIN_XMIN) / LIN_N
    return LIN_T0 * (1.0 + LIN_DELTA * np.exp(-0.5 * x * x))


def lin_ratio(t_a, t_b):
    """||T_A - T_B||_1 / (2.5 delta ||T_B - T0||_1)"""
    return float(np.sum(np.abs(t_a - t_b)) / (2.5 * LIN_DELTA * np.sum(np.abs(t_b - LIN_T0))))


def lin_tlim(kappa0):
    dx = (LIN_XMAX - LIN_XMIN) / LIN_N
    return LIN_CYCLES * (LIN_CFL * 0.5 * dx * dx / kappa0)


def lin_cpu(tlim, spitzer=None, kappa=0.0, sat_prefac=1.0):
    """the experiment with the numpy restatements: forward-Euler steps of dE/dt = -dF/dx, each of the diffusive limit of
    the current state (the last one of what is left to tlim); returns the temperatures"""
    nx, dx = (LIN_N, 1, 1), ((LIN_XMAX - LIN_XMIN) / LIN_N, 1.0, 1.0)
    w = np.zeros((1, 9, 1, 1, LIN_N + 2))
    w[0, 0] = 1.0
    w[0, 5] = 1.0
    w[0, 4, 0, 0, 1:-1] = lin_profile()  # p = rho T
    kw = dict(conduction="anisotropic", kappa=kappa, sat_prefac=sat_prefac, spitzer=spitzer)
    t = 0.0
    while t < tlim:
        w[..., 0] = w[..., -2]
        w[..., -1] = w[..., 1]
        dt = min(SP.diffusion_timestep(w, nx, 1, dx, LIN_CFL, **kw), tlim - t)
        t += dt
        f = SP.diff_fluxes(w, [np.zeros_like(w), None, None], nx, 1, dx, **kw)[0][0, 4, 0, 0]
        # e = p / (gamma - 1) = p; the lower face of cell i is f[i], the upper one f[i + 1]
        w[0, 4, 0, 0, 1:-1] += dt * (-(f[2:] - f[1:-1]) / dx[0])
    return w[0, 4, 0, 0, 1:-1] / w[0, 0, 0, 0, 1:-1]


# the units of the experiment (those of inputs/diffusion_spitzer.in) and its Spitzer coefficient in erg / (s K cm): large
# enough that the diffusive limit, not the hyperbolic one, is the time step
LIN_UNITS = dict(length=3.085677580962325e21, time=2.6e14, mass=8.3e40, he_mass_fraction=0.25)
LIN_COND_CGS = 4.6e-4


def lin_numbers():
    """((coeff_code, mbar, k_boltzmann), kappa0 = chi(T0, rho0 = 1)) of the experiment, from the cgs constants"""
    coeff, mbar, kb, _ = spitzer_numbers(cond_cgs=LIN_COND_CGS, **LIN_UNITS)
    return (coeff, mbar, kb), float(SP.chi(np.float64(LIN_T0), np.float64(1.0), spitzer=(coeff, mbar, kb)))
