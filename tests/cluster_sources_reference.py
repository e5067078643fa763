"""numpy restatement of the cluster problem's remaining sources, in the operation order of the code under test: SNIa
feedback (snia_feedback.cpp:87-118 with the Hernquist BCG's density of cluster_gravity.hpp:203-230), stellar feedback
(stellar_feedback.cpp:135-169), the clips (cluster_clips.cpp:93-155) and the five per-box sums in the device's order
(block_sum of tests/triggering_reference.py).  The yardstick of tests/test_cluster_sources_host.py and
tests/test_gpu_cluster_sources.py, written from the formulas in the manner of triggering_reference.py: host scalars go
through `math`, per-cell arithmetic is numpy float64, nothing fused or reassociated; squares and the cube are products.
Every per-cell operation is a product, quotient, sum or square root: stored values and sums are compared bit for bit.

All functions take a block's arrays [nvar][k][j][i] with the centres x1, x2, x3 of the same cells and a mask of the
cells a loop runs over (the interior ones); they return new arrays."""
import math
from types import SimpleNamespace

import numpy as np

import feedback_reference as FB
from triggering_reference import block_sum, block_sum_groups  # noqa: F401  (re-exported: the sums' order)

F = np.float64
INF = float("inf")
TOTALS = ("stellar_mass", "added_dfloor_mass", "removed_eceil_energy", "removed_vceil_energy", "added_vAceil_mass")


def rho_const_bcg(which_bcg, m_bcg_s, r_bcg_s):
    """calc_rho_const_bcg (cluster_gravity.hpp:89-102): 1 = HERNQUIST, 0 = NONE"""
    return m_bcg_s * r_bcg_s / (2 * math.pi) if which_bcg == 1 else 0.0


def eceil_of(Tceil, mbar_over_kb, gamma):
    """cluster.cpp:262-272"""
    return Tceil / mbar_over_kb / (gamma - 1.0) if Tceil < INF else Tceil


def snia_cfg(power, mass_rate, rho_const, r_bcg_s, smoothing_r=0.0):
    return SimpleNamespace(power_per_bcg_mass=F(power), mass_rate_per_bcg_mass=F(mass_rate), rho_const_bcg=F(rho_const),
                           r_bcg_s=F(r_bcg_s), smoothing_r=F(smoothing_r))


def stellar_cfg(stellar_radius, exclusion_radius, number_density_threshold, temperature_threshold, mbar, mbar_over_kb, mass_to_energy):
    return SimpleNamespace(stellar_radius=F(stellar_radius), exclusion_radius=F(exclusion_radius),
                           number_density_threshold=F(number_density_threshold), temperature_threshold=F(temperature_threshold),
                           mbar=F(mbar), mbar_over_kb=F(mbar_over_kb), mass_to_energy=F(mass_to_energy))


def clips_cfg(clip_r, dfloor=-1.0, vceil=INF, vAceil=INF, eceil=INF):
    return SimpleNamespace(clip_r=F(clip_r), dfloor=F(dfloor), vceil=F(vceil), vAceil=F(vAceil), eceil=F(eceil))


def _c2p(u, gamma):
    nh = 9 if u.shape[0] >= 9 else 5
    w = np.array(u, dtype=F)
    w[:nh] = FB.cons_to_prim(u[:nh], gamma)
    return w


def bcg_density(c, r_in):
    """ClusterGravity::rho_from_r with the BCG alone; the cube a product"""
    r = np.maximum(r_in, c.smoothing_r)
    ra = r + c.r_bcg_s
    return c.rho_const_bcg / (r * ((ra * ra) * ra))


def snia_feedback_src(u, w, x1, x2, x3, mask, c, beta_dt, gamma):
    """(u, w) after SNIAFeedback::FeedbackSrcTerm on the masked cells; the BCG density [k][j][i] as a third value"""
    u0, w0 = np.array(u, dtype=F), np.array(w, dtype=F)
    X, Y, Z = FB.grid(x1, x2, x3)
    with np.errstate(all="ignore"):
        r = np.sqrt(X * X + Y * Y + Z * Z)
        rho_bcg = bcg_density(c, r)
        energy = (c.power_per_bcg_mass * F(beta_dt)) * rho_bcg
        density = (c.mass_rate_per_bcg_mass * F(beta_dt)) * rho_bcg
        un = u0.copy()
        un[4] = un[4] + energy
        un[0] = un[0] + density
        un[1] = un[1] + density * w0[1]
        un[2] = un[2] + density * w0[2]
        un[3] = un[3] + density * w0[3]
        un[4] = un[4] + density * (0.5 * (w0[1] * w0[1] + w0[2] * w0[2] + w0[3] * w0[3]))
        wn = _c2p(un, gamma)
    return np.where(mask[None], un, u0), np.where(mask[None], wn, w0), rho_bcg


def _r2(x1, x2, x3):
    X, Y, Z = FB.grid(x1, x2, x3)
    return X * X + Y * Y + Z * Z


def _margin(q, threshold, where):
    """the least relative distance |q / threshold - 1| of the cells `where` from a threshold (inf: none, or no threshold)"""
    if not np.any(where) or not np.isfinite(threshold) or threshold == 0:
        return INF
    return float(np.min(np.abs(q[where] / threshold - 1.0)))


def stellar_shell(x1, x2, x3, c):
    """the cells the stellar loop does not leave at its first test: not (r > stellar_radius or r <= exclusion_radius)"""
    r = np.sqrt(_r2(x1, x2, x3))
    return ~((r > c.stellar_radius) | (r <= c.exclusion_radius))


def stellar_feedback_src(u, w, x1, x2, x3, mask, c, vol, gamma):
    """(u, w, terms, info): the state after StellarFeedback::FeedbackSrcTerm on the masked cells, the per-cell terms of
    stellar_mass [k][j][i] (zero where nothing converts), and the shell, the converting cells and whether the reference's
    sanity check would have failed"""
    u0, w0 = np.array(u, dtype=F), np.array(w, dtype=F)
    shell = stellar_shell(x1, x2, x3, c) & mask
    with np.errstate(all="ignore"):
        n = w0[0] / c.mbar
        temp = c.mbar_over_kb * w0[4] / w0[0]
        conv = shell & ~(n < c.number_density_threshold) & ~(temp > c.temperature_threshold)
        delta = c.number_density_threshold * c.mbar - w0[0]
        term = -(delta * F(vol))
        un = u0.copy()
        un[0] = un[0] + delta
        un[1] = un[1] + delta * w0[1]
        un[2] = un[2] + delta * w0[2]
        un[3] = un[3] + delta * w0[3]
        un[4] = un[4] + delta * (0.5 * (w0[1] * w0[1] + w0[2] * w0[2] + w0[3] * w0[3]) + 1 / (F(gamma) - 1.0) * w0[4] / w0[0])
        de = -c.mass_to_energy * delta
        un[4] = un[4] + de
        wn = _c2p(un, gamma)
    with np.errstate(all="ignore"):
        r = np.sqrt(_r2(x1, x2, x3))
        margin = min(_margin(r, c.stellar_radius, mask), _margin(r, c.exclusion_radius, mask),
                     _margin(n, c.number_density_threshold, shell), _margin(temp, c.temperature_threshold, shell))
    info = SimpleNamespace(shell=shell, converted=conv, failed=bool(np.any(conv & ~(de > 0.0))), margin=margin)
    return np.where(conv[None], un, u0), np.where(conv[None], wn, w0), np.where(conv, term, 0.0), info


def clip_sphere(x1, x2, x3, c):
    return _r2(x1, x2, x3) < c.clip_r * c.clip_r


def cluster_clips(u, w, x1, x2, x3, mask, c, vol, gamma, mhd):
    """(u, w, terms, info): the state after ApplyClusterClips on the masked cells -- ConsToPrim, dfloor, vceil, vAceil (with
    `mhd`), eceil, and no ConsToPrim afterwards --, terms[4][k][j][i] of added_dfloor_mass, removed_eceil_energy,
    removed_vceil_energy, added_vAceil_mass, and which cells each clip acted on"""
    u0, w0 = np.array(u, dtype=F), np.array(w, dtype=F)
    inside = clip_sphere(x1, x2, x3, c) & mask
    gm1 = F(gamma) - 1.0
    zero = np.zeros(u0.shape[1:])
    with np.errstate(all="ignore"):
        un = u0.copy()
        wn = _c2p(un, gamma)
        t_df = t_vc = t_va = t_ec = zero
        a_df = a_vc = a_va = a_ec = np.zeros(u0.shape[1:], bool)
        margin = _margin(_r2(x1, x2, x3), c.clip_r * c.clip_r, mask)
        if c.dfloor > 0:
            rho = wn[0].copy()
            margin = min(margin, _margin(rho, c.dfloor, inside))
            a_df = inside & (rho < c.dfloor)
            t_df = np.where(a_df, (c.dfloor - rho) * F(vol), 0.0)
            un[0] = np.where(a_df, c.dfloor, un[0])
            wn[0] = np.where(a_df, c.dfloor, wn[0])
        if c.vceil < INF:
            vceil2 = c.vceil * c.vceil
            v2 = wn[1] * wn[1] + wn[2] * wn[2] + wn[3] * wn[3]
            a_vc = inside & (v2 > vceil2)
            margin = min(margin, _margin(v2, vceil2, inside))
            v = np.sqrt(v2)
            for n in (1, 2, 3):
                un[n] = np.where(a_vc, un[n] * (c.vceil / v), un[n])
            for n in (1, 2, 3):
                wn[n] = np.where(a_vc, wn[n] * (c.vceil / v), wn[n])
            removed = 0.5 * wn[0] * (v2 - vceil2)
            t_vc = np.where(a_vc, removed * F(vol), 0.0)
            un[4] = np.where(a_vc, un[4] - removed, un[4])
        if mhd and c.vAceil * c.vAceil < INF:
            vAceil2 = c.vAceil * c.vAceil
            rho = wn[0].copy()
            B2 = wn[5] * wn[5] + wn[6] * wn[6] + wn[7] * wn[7]
            a_va = inside & (B2 / rho > vAceil2)
            margin = min(margin, _margin(B2 / rho, vAceil2, inside))
            rho_new = np.sqrt(B2 / vAceil2)
            t_va = np.where(a_va, (rho_new - rho) * F(vol), 0.0)
            un[0] = np.where(a_va, rho_new, un[0])
            wn[0] = np.where(a_va, rho_new, wn[0])
        if c.eceil < INF:
            e = wn[4] / (gm1 * wn[0])
            a_ec = inside & (e > c.eceil)
            margin = min(margin, _margin(e, c.eceil, inside))
            removed = wn[0] * (e - c.eceil)
            t_ec = np.where(a_ec, removed * F(vol), 0.0)
            un[4] = np.where(a_ec, un[4] - removed, un[4])
            wn[4] = np.where(a_ec, gm1 * wn[0] * c.eceil, wn[4])
    info = SimpleNamespace(inside=inside, dfloor=a_df, vceil=a_vc, vAceil=a_va, eceil=a_ec, margin=margin)
    return np.where(inside[None], un, u0), np.where(inside[None], wn, w0), np.array([t_df, t_ec, t_vc, t_va]), info


def split_src(u, w, x1, x2, x3, mask, stellar, clips, vol, gamma, mhd):
    """ClusterSplitSrcTerm: stellar feedback (if given), then the clips (if given); (u, w, terms[5][k][j][i] in the order
    of TOTALS, the two steps' infos)"""
    terms = np.zeros((5,) + np.asarray(u).shape[1:])
    infos = SimpleNamespace(stellar=None, clips=None)
    if stellar is not None:
        u, w, terms[0], infos.stellar = stellar_feedback_src(u, w, x1, x2, x3, mask, stellar, vol, gamma)
    if clips is not None:
        u, w, terms[1:], infos.clips = cluster_clips(u, w, x1, x2, x3, mask, clips, vol, gamma, mhd)
    return np.array(u, dtype=F), np.array(w, dtype=F), terms, infos


def box_sums(terms, lo, hi, P):
    """the five sums of one block in the device's order: terms[5][k][j][i] on the box [lo, hi) (i, j, k; hi exclusive), its
    cells in box order, i fastest, through block_sum with P workgroups"""
    t = terms[:, lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    return block_sum(t.reshape(t.shape[0], -1), P)


def brute_force_box(x, radius, first):
    """per direction the least [lo, hi) in extended indices (`first` = the first interior index) that holds every interior
    cell with |x| < radius; None if there is none"""
    inside = np.nonzero(np.abs(x) < radius)[0]
    return None if len(inside) == 0 else (first + int(inside[0]), first + int(inside[-1]) + 1)
