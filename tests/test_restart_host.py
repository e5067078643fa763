"""Restart without a GPU: the state file round trip through athenapk_amd.restart (the writer is the C++ one, on a
host-only sim), the rst output blocks as parsed, and every refusal a host-only plan can see, with its key in the message."""
import math
import sys

import pytest

from athenapk_amd import decks, driver, restart
from athenapk_amd import lib as L

SMALL = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/meshblock/nx1=16",
         "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16"]


def _plan(deck, ov=(), text=None):
    return driver.HostPlan(text if text is not None else decks.load(deck), list(ov))


def _refused(deck, ov, *words, text=None):
    with pytest.raises(L.ApkError) as e:
        _plan(deck, ov, text)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.fixture(scope="module")
def turb_rst(tmp_path_factory):
    """the state file of a host-only turbulence sim (time 0, cycle 0, the driver freshly seeded): written once"""
    prefix = tmp_path_factory.mktemp("rst") / "turb"
    _plan("turbulence_restart", SMALL).write_restart(prefix)
    return str(prefix) + ".rst"


# ---- 1. the state block ------------------------------------------------------------------------------------------------
def test_state_of_a_host_only_sim(turb_rst):
    st = restart.state(turb_rst)
    assert st["format_version"] == 1 and st["cycle"] == 0 and st["time"] == 0.0
    # (unset mutable params hold the largest double: written with %.17g, read back exactly)
    big = sys.float_info.max
    assert st["dt"] == big and st["dt_hyp"] == big and st["mindx"] == big and st["dt_diff"] == big and st["c_h"] == 0.0
    assert (st["nranks"], st["nblocks"], st["fluid"], st["nvar"], st["nghost"]) == (1, 8, "glmmhd", 9, 2)
    assert st["mesh_nx"] == (32, 32, 32) and st["block_nx"] == (16, 16, 16) and st["refinement"] == "none"
    assert [b["gid"] for b in st["blocks"]] == list(range(8))
    assert sorted((b["lx1"], b["lx2"], b["lx3"]) for b in st["blocks"]) == [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    assert all(b["level"] == 0 and b["deref_count"] == 0 and b["rank"] == 0 for b in st["blocks"])
    assert sorted(b["index"] for b in st["blocks"]) == list(range(8))
    t = st["turbulence"]
    assert len(t["state_rng"].split()) == 625  # 624 words of std::mt19937 and its position
    assert [float(w) for w in t["state_dist"].split()] == [-1.0, 1.0]
    assert len(t["accel_hat"]) == 3 and len(t["accel_hat"][0]) == 30 and all(z == 0 for row in t["accel_hat"] for z in row)


def test_every_double_round_trips_exactly(tmp_path, turb_rst):
    """a state block with the doubles that are hard to print (17 digits, the largest, a denormal, inf for an unset dt_diff)
    through restart.state, and through the C++ reader: a plan built from that text re-writes it digit for digit"""
    vals = {"time": 0.1 + 0.2, "dt": 5e-324, "dt_hyp": sys.float_info.max, "mindx": 1.0 / 3.0, "c_h": 1.0 / 7.0,
            "dt_diff": math.inf}
    lines = []
    for line in restart.deck(turb_rst).splitlines():
        k = line.split("=")[0].strip()
        lines.append("%s = %s" % (k, "%.17g" % vals[k]) if k in vals else line)
    text = "\n".join(lines) + "\n"
    assert "dt_diff = inf" in text
    p = tmp_path / "edited.rst"
    p.write_text(text)
    st = restart.state(p)
    for k, v in vals.items():
        assert st[k] == v and math.copysign(1, st[k]) == math.copysign(1, v), k
    assert math.isinf(st["dt_diff"])
    # the C++ side: accepted as a deck (the state block agrees with the mesh), and the deck part is carried over
    again = tmp_path / "again"
    _plan(None, [], text).write_restart(again)
    st2 = restart.state(str(again) + ".rst")
    assert st2["turbulence"]["state_rng"] == st["turbulence"]["state_rng"]
    assert restart.parse(restart.deck(str(again) + ".rst"))["parthenon/mesh"]["nx1"] == "32"


def test_the_state_file_is_the_deck_with_overrides_applied(turb_rst):
    blocks = restart.parse(restart.deck(turb_rst))
    assert blocks["parthenon/mesh"]["nx1"] == "32" and blocks["parthenon/meshblock"]["nx3"] == "16"  # (the overrides)
    assert blocks["problem/turbulence"]["rseed"] == "20190729" and blocks["modes"]["k_30_2"] == "+2"
    assert blocks["parthenon/output3"] == {"file_type": "rst", "dt": "0.5"}  # (a default the reader adds, id, is not stored)
    assert "tracers" not in blocks and "problem/cluster/magnetic_tower" not in blocks  # (nor a block made of defaults alone)
    assert blocks["job"]["problem_id"] == "turbulence"


def test_a_plain_deck_is_not_a_state_file(tmp_path):
    p = tmp_path / "plain.rst"
    p.write_text(decks.load("sod"))
    with pytest.raises(ValueError, match="apk_amd/restart"):
        restart.deck(p)


# ---- 2. the rst output blocks ------------------------------------------------------------------------------------------
def test_restart_outputs_of_the_new_deck():
    assert _plan("turbulence_restart").restart_outputs() == [{"number": 3, "id": "out3", "dt": 0.5}]
    assert _plan("turbulence").restart_outputs() == []


def test_id_and_two_blocks():
    ov = ["parthenon/output7/file_type=rst", "parthenon/output7/dt=0.125", "parthenon/output7/id=checkpoint"]
    a, b = _plan("turbulence_restart", ov).restart_outputs()
    assert a == {"number": 3, "id": "out3", "dt": 0.5} and b == {"number": 7, "id": "checkpoint", "dt": 0.125}


def test_a_plan_without_tracers_and_with_an_rst_block_is_accepted():
    p = _plan("blast", ["parthenon/output4/file_type=rst", "parthenon/output4/dt=0.01", "tracers/enabled=false"])
    assert p.restart_outputs() == [{"number": 4, "id": "out4", "dt": 0.01}]
    assert p.snapshot_outputs() == []  # (an rst block is not a snapshot block)


# ---- 3. refused, never ignored -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["0", "-0.5"])
def test_dt_must_be_positive(dt):
    _refused("turbulence", ["parthenon/output3/file_type=rst", "parthenon/output3/dt=" + dt], "parthenon/output3", "dt")


def test_dt_must_be_there():
    _refused("turbulence", ["parthenon/output3/file_type=rst"], "parthenon/output3", "dt")


def test_an_rst_block_with_tracers_is_refused():
    _refused("turbulence_tracers", ["parthenon/output5/file_type=rst", "parthenon/output5/dt=0.5"], "parthenon/output5",
             "tracers/enabled")


def test_write_restart_with_tracers_is_refused(tmp_path):
    with pytest.raises(L.ApkError, match="tracers/enabled"):
        _plan("turbulence_tracers").write_restart(tmp_path / "x")
    assert not (tmp_path / "x.rst").exists()


def test_another_format_version_is_refused(turb_rst):
    text = restart.deck(turb_rst).replace("format_version = 1", "format_version = 2")
    _refused(None, [], "format_version", text=text)


@pytest.mark.parametrize("override,key", [
    ("parthenon/mesh/nx1=64", "parthenon/mesh/nx1"),
    ("parthenon/meshblock/nx2=8", "parthenon/meshblock/nx2"),
    ("parthenon/mesh/nghost=3", "parthenon/mesh/nghost"),
    ("hydro/nscalars=1", "hydro/nscalars"),
])
def test_overrides_on_a_state_file_that_change_the_layout_are_refused(turb_rst, override, key):
    extra = ["parthenon/mesh/nx2=64", "parthenon/mesh/nx3=64"] if key == "parthenon/mesh/nx1" else []  # (FMFT wants a cube)
    _refused(None, [override] + extra, key, "state file", text=restart.deck(turb_rst))


def test_overrides_that_change_the_fluid_or_the_refinement_mode_are_refused(tmp_path):
    prefix = tmp_path / "blast"
    _plan("blast", SMALL).write_restart(prefix)
    text, st = restart.deck(str(prefix) + ".rst"), restart.state(str(prefix) + ".rst")
    other = "euler" if st["fluid"] == "glmmhd" else "glmmhd"
    _refused(None, ["hydro/fluid=" + other], "hydro/fluid", "state file", text=text)
    assert st["refinement"] == "none"
    _refused(None, ["parthenon/mesh/refinement=static"], "parthenon/mesh/refinement", "state file", text=text)


def test_overrides_that_keep_the_layout_are_accepted(turb_rst):
    p = _plan(None, ["parthenon/time/tlim=2.0", "parthenon/output3/dt=0.25"], restart.deck(turb_rst))
    assert p.tlim == 2.0 and p.restart_outputs() == [{"number": 3, "id": "out3", "dt": 0.25}]
    # the driver of a plan built from a state file starts from the stored spectral state and RNG: here the fresh seed's
    fresh = _plan("turbulence_restart", SMALL)
    p.fmft_evolve(0.01)
    fresh.fmft_evolve(0.01)
    assert (p.fmft_var_hat() == fresh.fmft_var_hat()).all() and abs(p.fmft_var_hat()).max() > 0
