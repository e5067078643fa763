"""Writes the synthetic power-law cooling table of the reference's cluster_tabular_cooling regression test
(tst/regression/test_suites/cluster_tabular_cooling): log T from 4 to 6 and log Lambda from -30 to -25 (log10 erg cm^3/s),
100 evenly spaced rows each, i.e. Lambda ~ T^2.5.  The tests write it on the fly with power_law_table(); run this file
to keep a copy next to it:  python tests/golden/make_cooling_tables.py"""
import os

import numpy as np

LOG_TEMP0, LOG_TEMP1, N_LOG_TEMP = 4, 6, 100
LOG_LAMBDA0, LOG_LAMBDA1, N_LOG_LAMBDA = -30, -25, 100


def power_law_table():
    """(log_temps, log_lambdas) as the regression test builds them"""
    return (np.linspace(LOG_TEMP0, LOG_TEMP1, N_LOG_TEMP), np.linspace(LOG_LAMBDA0, LOG_LAMBDA1, N_LOG_LAMBDA))


def write_power_law_table(path):
    lt, ll = power_law_table()
    np.savetxt(path, np.vstack((lt, ll)).T, delimiter=" ")
    return path


if __name__ == "__main__":
    print(write_power_law_table(os.path.join(os.path.dirname(os.path.abspath(__file__)), "power_law.cooling")))
