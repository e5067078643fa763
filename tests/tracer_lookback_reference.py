"""numpy restatement of the tracers' lookback histories and their correlations (test infrastructure):
src/pgen/turbulence.cpp:200-216 (state) and :513-647 (ProblemFillTracers), written from the description of what they
do.  Histories are arrays [n][12], level 0 the current cycle, level i the value of 2^(i-1) cycles' spacing."""
import math

import numpy as np

N_LOOKBACK = 12
N_SUMS = 26  # corr_s[12], corr_sdot[12], sum s[0], sum sdot[0]


def shifting_levels(cycle):
    """the levels that take the value of the level below them in cycle number `cycle`, highest first"""
    return [idx for idx in range(N_LOOKBACK - 1, 0, -1) if cycle % (1 << (idx - 1)) == 0]


def cascade(levels, cycle):
    """the shift of one update, in place on levels[..., 12]: highest level first, so that a level receives the OLD
    value of the level below it.  Level 0 is left for the caller to set."""
    for idx in shifting_levels(cycle):
        levels[..., idx] = levels[..., idx - 1]
    return levels


def held_cycle(level, cycle):
    """the cycle whose level-0 value level `level` holds after the update of cycle `cycle`, one update per cycle from
    cycle 0 on: level i >= 1 shifted last at the last multiple of d = 2^(i-1), and received what was d cycles old then.
    Negative: older than the run (-1 is the seed-time update, anything below is the empty history)."""
    if level == 0:
        return cycle
    d = 1 << (level - 1)
    return (cycle - cycle % d) - d


def update(s, sdot, rho, active, cycle, dt):
    """one update on copies of s, sdot [n][12]: active particles shift, then s[0] = ln rho, sdot[0] = (s[0] - s[1]) / dt"""
    s, sdot = s.copy(), sdot.copy()
    act = np.asarray(active) != 0
    s[act] = cascade(s[act], cycle)
    sdot[act] = cascade(sdot[act], cycle)
    s[act, 0] = np.log(rho[act])
    sdot[act, 0] = (s[act, 0] - s[act, 1]) / dt
    return s, sdot


def terms(s, sdot, active):
    """[26][n_active]: the terms of the 26 sums over the active particles, each product rounded once"""
    act = np.asarray(active) != 0
    s, sdot = s[act], sdot[act]
    return np.concatenate([(s[:, :1] * s).T, (sdot[:, :1] * sdot).T, s[:, :1].T, sdot[:, :1].T])


def sums_and_bounds(s, sdot, active):
    """(exactly rounded sums [26] by math.fsum, bounds [26]).  The bound is (n_active + 2) 2^-53 sum |term|: a sum of
    n terms in ANY order is off by at most (n - 1) u sum |term| to first order in u = 2^-53, each term carries one
    rounding of its product (u |term|), fsum itself rounds once more; n + 2 covers the second-order part for every n
    that fits in memory.  A contracted product (fma) rounds less, not more."""
    t = terms(s, sdot, active)
    exact = np.array([math.fsum(row.tolist()) for row in t])
    bound = (t.shape[1] + 2) * 2.0 ** -53 * np.abs(t).sum(axis=1)
    return exact, bound


def ulps(got, want):
    """|got - want| in units of the spacing of want"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))
