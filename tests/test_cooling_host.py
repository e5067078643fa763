"""CPU tests of <units>, the gas composition and <cooling> (no GPU): the derived scales and mbar_over_kb
(src/units.hpp, hydro.cpp:482-503), the temperature floor and ceiling (hydro.cpp:509-536), the cooling options and
their defaults, the table checks with the reference's messages, the conversion of the rates to code units and the
Townsend coefficients (tabular_cooling.cpp:30-276), and the flux-array stage path when cooling is on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cooling_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHURE = os.path.join(ROOT, "tests", "golden", "schure.cooling_1.0Z")
GAMMA, HE = 1.6666666666666667, 0.25


def _plan(overrides, deck="cooling"):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), ["cooling/table_filename=" + SCHURE] + list(overrides))


def _refused(overrides, deck="cooling"):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def _table(tmp_path, rows, name="t.cooling"):
    p = tmp_path / name
    p.write_text(rows)
    return str(p)


def test_units_and_composition_of_the_deck():
    p = _plan([])
    u = p.units()
    want = R.CLUSTER_UNITS
    assert u.has_units == 1 and u.has_composition == 1
    assert (u.code_length_cgs, u.code_mass_cgs, u.code_time_cgs) == (want.length, want.mass, want.time)
    for k in ("mh", "k_boltzmann", "atomic_mass_unit", "erg", "cm", "s"):
        assert getattr(u, k) == getattr(want, k), k
    mu, mu_e, mbar, mbar_over_kb = R.composition(want, HE)
    assert (u.mu, u.mu_e, u.mbar, u.mbar_over_kb) == (mu, mu_e, mbar, mbar_over_kb)
    assert u.He_mass_fraction == HE
    # no floor, no ceiling: the EOS fields stay disabled
    assert u.efloor == -1.0 and u.eceil == math.inf


def test_units_default_to_one_and_composition_needs_units():
    p = _plan(["cooling/enable_cooling=none", "units/code_mass_cgs=1.0", "units/code_time_cgs=1.0",
               "units/code_length_cgs=1.0"])
    u = p.units()
    assert u.mh == R.MH_CGS and u.k_boltzmann == R.K_BOLTZMANN_CGS and u.erg == 1.0
    q = _plan([], deck="sod")
    assert q.units().has_units == 0 and q.units().has_composition == 0


def test_temperature_floor_and_ceiling_map_to_the_eos():
    p = _plan(["hydro/Tfloor=1e4", "hydro/Tceil=1e9"])
    u = p.units()
    mbar_over_kb = R.composition(R.CLUSTER_UNITS, HE)[3]
    assert u.efloor == 1e4 / mbar_over_kb / (GAMMA - 1.0)
    assert u.eceil == 1e9 / mbar_over_kb / (GAMMA - 1.0)


@pytest.mark.parametrize("key", ["Tfloor", "Tceil"])
def test_temperature_limits_without_units_are_refused(key):
    msg = _refused(["hydro/%s=1e4" % key], deck="sod")
    assert "requires units and gas composition" in msg


def test_cooling_defaults():
    from athenapk_amd import decks, driver
    from athenapk_amd import lib as L
    # a <cooling> block with the switch, the table and the units of its rates only
    head, tail = decks.load("cooling").split("<cooling>")
    tail = "\n".join(l for l in tail.splitlines()
                     if l.split("=")[0].strip() not in ("integrator", "max_iter", "cfl", "d_log_temp_tol", "d_e_tol"))
    q = driver.HostPlan(head + "<cooling>" + tail, ["cooling/table_filename=" + SCHURE])
    en, c, n = q.cooling_options()
    assert en and n == 100  # rows of the Schure table (comments skipped)
    assert c.integrator == L.COOL_INTEGRATOR["rk12"] and c.max_iter == 100 and c.cfl == 0.1
    assert c.d_log_temp_tol == 1e-8 and c.d_e_tol == 1e-8 and c.T_floor == -1.0
    assert c.gamma == GAMMA and c.He_mass_fraction == HE and c.mh == R.CLUSTER_UNITS.mh
    assert c.mbar_over_kb == R.composition(R.CLUSTER_UNITS, HE)[3]
    # T_floor comes from hydro/Tfloor
    assert _plan(["hydro/Tfloor=2e4"]).cooling_options()[1].T_floor == 2e4


def test_rates_in_code_units():
    p = _plan([])
    lt, ll = R.read_table(SCHURE)
    lam_u = R.CLUSTER_UNITS.lambda_units(1.0)
    assert p.cooling_options()[1].lambda_units == lam_u
    assert np.array_equal(p.cooling_table("log_temps"), lt)
    assert np.array_equal(p.cooling_table("log_lambdas"), ll - math.log10(lam_u))
    # lambda_units_cgs scales them
    q = _plan(["cooling/lambda_units_cgs=1e-23"])
    assert np.array_equal(q.cooling_table("log_lambdas"), ll - math.log10(R.CLUSTER_UNITS.lambda_units(1e-23)))


@pytest.mark.parametrize("table", ["schure", "power_law"])
def test_townsend_coefficients(tmp_path, table):
    import golden.make_cooling_tables as M
    path = SCHURE if table == "schure" else M.write_power_law_table(str(tmp_path / "pl.cooling"))
    p = _plan(["cooling/integrator=townsend", "cooling/table_filename=" + path])
    lt, ll = R.read_table(path)
    mbar_over_kb = R.composition(R.CLUSTER_UNITS, HE)[3]
    T = R.Table(lt, ll, R.CLUSTER_UNITS.lambda_units(), GAMMA, mbar_over_kb, HE, R.CLUSTER_UNITS.mh, townsend=True)
    a, y = p.cooling_table("alpha_k"), p.cooling_table("Y_k")
    assert len(a) == len(lt) - 1 and len(y) == len(lt) - 1
    np.testing.assert_allclose(a, T.alpha_k, rtol=1e-14, atol=0)
    np.testing.assert_allclose(y, T.Y_k, rtol=1e-14, atol=1e-14 * np.max(np.abs(T.Y_k)))
    assert y[-1] == 0.0 and np.all(np.diff(y) < 0)  # the temporal evolution function decreases with T


@pytest.mark.parametrize("rows,needle", [
    ("4.0 -22.0\n", "Not enough data to interpolate cooling"),
    ("4.0 -22.0\n3.9 -22.1\n4.0 -22.2\n", "second log_temp in table is descreasing"),
    ("4.0 -22.0\n4.1 -22.1\n4.0 -22.2\n", "log_temp in table is descreasing at i= 2"),
    ("4.0 -22.0\n4.1 -22.1\n4.3 -22.2\n", "d_log_temp in table is uneven at i=2"),
    ("4.0 -22.0 1.0\n4.1 -22.1\n", "Expected exactly two columns per line"),
    ("4.0\n4.1 -22.1\n", "Expected exactly two columns per line"),
    ("4.0 abc\n4.1 -22.1\n", "could not be parsed as double"),
])
def test_table_refusals(tmp_path, rows, needle):
    msg = _refused(["cooling/table_filename=" + _table(tmp_path, rows)])
    assert needle in msg, msg


def test_table_format_skips_comments_and_blank_lines(tmp_path):
    path = _table(tmp_path, "# a comment\n\n   \n  # indented comment\n4.0 -22.0\n4.1 -22.5\n4.2 -22.25\n")
    p = _plan(["cooling/table_filename=" + path])
    assert p.cooling_options()[2] == 3
    assert np.array_equal(p.cooling_table("log_temps"), [4.0, 4.1, 4.2])


def test_uneven_table_allowed_for_townsend_without_cfl(tmp_path):
    path = _table(tmp_path, "4.0 -22.0\n4.1 -22.1\n4.3 -22.4\n4.35 -22.3\n")
    assert "uneven" in _refused(["cooling/table_filename=" + path, "cooling/integrator=townsend"])
    assert "uneven" in _refused(["cooling/table_filename=" + path, "cooling/integrator=rk45", "cooling/cfl=0"])
    p = _plan(["cooling/table_filename=" + path, "cooling/integrator=townsend", "cooling/cfl=0"])
    assert p.cooling_options()[2] == 4 and len(p.cooling_table("alpha_k")) == 3
    # the tolerance is cooling/d_log_temp_tol
    q = _plan(["cooling/table_filename=" + path, "cooling/d_log_temp_tol=2.0"])
    assert q.cooling_options()[2] == 4


def test_townsend_power_law_index_one_is_refused(tmp_path):
    # (cgs code units: the rates need no conversion, and lambda ~ T on the first interval exactly)
    path = _table(tmp_path, "4.0 -22.0\n5.0 -21.0\n6.0 -20.5\n")
    cgs = ["units/code_length_cgs=1", "units/code_mass_cgs=1", "units/code_time_cgs=1"]
    assert "special case for Townsend" in _refused(cgs + ["cooling/table_filename=" + path, "cooling/integrator=townsend"])
    _plan(cgs + ["cooling/table_filename=" + path, "cooling/integrator=rk12"])  # (only Townsend needs the fits)


@pytest.mark.parametrize("overrides,needle", [
    (["cooling/enable_cooling=powerlaw"], "Unknown cooling string"),
    (["cooling/integrator=rk4"], "Unknown cooling integrator"),
    (["parthenon/mesh/refinement=static"], "refined meshes"),
    (["cooling/table_filename=/nonexistent/table"], "cannot open cooling table"),
])
def test_option_refusals(overrides, needle):
    msg = _refused(overrides)
    assert needle in msg, msg


def test_cooling_needs_units_and_composition():
    from athenapk_amd import decks, driver
    from athenapk_amd import lib as L
    deck = decks.load("cooling")
    no_units = deck.replace("<units>", "<unused_units>")
    for text in (no_units, deck.replace("He_mass_fraction = 0.25", "")):
        with pytest.raises(L.ApkError) as e:
            driver.HostPlan(text, ["cooling/table_filename=" + SCHURE])
        assert "requires units and gas composition" in str(e.value)


def test_lambda_units_are_required():
    from athenapk_amd import decks, driver
    from athenapk_amd import lib as L
    deck = decks.load("cooling").replace("lambda_units_cgs = 1", "")
    with pytest.raises(L.ApkError) as e:
        driver.HostPlan(deck, ["cooling/table_filename=" + SCHURE])
    assert "lambda_units_cgs" in str(e.value)


def test_cooling_selects_the_flux_array_stage_path():
    assert _plan([]).info.fused == 0
    off = _plan(["cooling/enable_cooling=none"])
    assert off.cooling_options()[0] is False and off.info.fused == 1
    # enable_cooling = none changes nothing: the same plan as a deck without the block
    assert _plan([], deck="sod").info.fused == 1 and _plan([], deck="sod").cooling_options()[0] is False


@pytest.mark.parametrize("integ", ["rk12", "rk45"])
def test_adaptive_cases_reach_every_branch(integ):
    """the cases of test_gpu_cooling_per_cell.py::test_adaptive_src_term_per_cell, in the restatement alone: every
    branch of the error control is taken at least 20 times in some case, and in some case the accepted substeps of
    the cooled cells of one wave (64 consecutive interior cells from a multiple of 64) differ by a factor 10 or more"""
    import cooling_cases as C
    most = dict.fromkeys(R.EVENTS, 0)
    span = 0.0
    for case in C.ADAPTIVE_CASES:
        if case[0] != integ:
            continue
        o = C.adaptive_restated(*case, probes=False)
        for k in R.EVENTS:
            most[k] = max(most[k], o["events"].get(k, 0))
        n = o["counts"]
        assert len(n) == C.NB * o["mask"].sum() and n.max() <= o["kw"]["max_iter"]
        for s in range(0, len(n), 64):
            w = n[s:s + 64]
            w = w[w > 0]
            if len(w):
                span = max(span, w.max() / w.min())
    assert min(most.values()) >= 20, most
    assert span >= 10.0, span


def test_rate_noise_is_off_by_default_and_seeded():
    import cooling_cases as C
    rows = C.rows("schure")
    T = C.restated(rows, "rk45", T_floor=C.T_FLOOR)
    rho, e = 147.7557589278723, 1e6 / C.MBAR_GM1_OVER_KB
    plain = T.dedt(e, rho)[0]
    a = [T.rate_noise(1e-13, 4).dedt(e, rho)[0] for _ in range(2)]
    b = [T.rate_noise(1e-13, 4).dedt(e, rho)[0] for _ in range(2)]
    assert a == b and a[0] != plain and abs(a[0] - plain) <= 1e-13 * abs(plain) * (1 + 1e-3)
    assert T.rate_noise(0.0).dedt(e, rho)[0] == plain
    assert T.rate_noise(1e-13, 4).dedt(1e3 / C.MBAR_GM1_OVER_KB, rho) == (0.0, True)  # (below the table: stays 0)
