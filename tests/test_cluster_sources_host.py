"""CPU tests of SNIa feedback, stellar feedback and the clips of the cluster problem on the host (no GPU): the options and
their defaults, the exclusion radius' fallback, eceil, rho_const_bcg, every refusal with its key and wording, the split
sources' active list against a brute-force mask, and a deck without any of the three."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402
import cluster_sources_reference as CS  # noqa: E402
from cluster_cases import box as _box, mesh as _mesh  # noqa: E402

INF = float("inf")
SNIA = "problem/cluster/snia_feedback/"
STELLAR = "problem/cluster/stellar_feedback/"
CLIPS = "problem/cluster/clips/"
TRIG = "problem/cluster/agn_triggering/"
DECK = "cluster_sources"
RKL2 = ["diffusion/integrator=rkl2", "diffusion/conduction=isotropic", "diffusion/conduction_coeff=fixed",
        "diffusion/thermal_diff_coeff_code=0.01", "diffusion/rkl2_max_dt_ratio=100"]


def _plan(overrides=(), deck=DECK, **kw):
    from athenapk_amd import decks, driver
    return driver.HostPlan(decks.load(deck), list(overrides), strict=True, **kw)


def _refused(overrides=(), deck=DECK):
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan(overrides, deck)
    return str(e.value)


def _without(deck_name, *blocks):
    """the deck's text without the named blocks"""
    from athenapk_amd import decks
    out, keep = [], True
    for line in decks.load(deck_name).splitlines():
        if line.startswith("<"):
            keep = line.strip() not in ["<%s>" % b for b in blocks]
        if keep:
            out.append(line)
    return "\n".join(out) + "\n"


def _plan_text(text, overrides=()):
    from athenapk_amd import driver
    return driver.HostPlan(text, list(overrides), strict=True)


# ---- options and defaults ---------------------------------------------------------------------------------------------
def test_the_deck_parses_with_all_three_sources_active():
    p = _plan()
    o, u = p.cluster_source_options(), p.units()
    assert (o.snia_active, o.stellar_active, o.clips_active, o.flux_path_sources) == (1, 1, 1, 1)
    assert (o.power_per_bcg_mass, o.mass_rate_per_bcg_mass) == (0.0015780504379367209, 0.00315576)
    assert (o.stellar_radius, o.exclusion_radius, o.efficiency) == (0.03, 0.01, 5e-9)
    assert (o.number_density_threshold, o.temperature_threshold) == (1.4928506511614273e+75, 1e4)
    assert (o.clip_r, o.dfloor, o.vceil, o.vAceil, o.Tceil) == (0.04, 1e4, 0.0005, INF, 5000.0)
    # the derived numbers, in the reference's operation order
    assert o.mbar == u.mu * u.mh and o.mbar_over_kb == u.mbar_over_kb
    c = 2.99792458e10 / (u.code_length_cgs / u.code_time_cgs)  # Units::speed_of_light
    assert o.mass_to_energy == 5e-9 * (c * c) > 0
    assert o.eceil == CS.eceil_of(5000.0, u.mbar_over_kb, 1.6666666666666667) == 5000.0 / u.mbar_over_kb / (1.6666666666666667 - 1.0)
    assert o.rho_const_bcg == CS.rho_const_bcg(1, 7.5e-4, 0.004) == 7.5e-4 * 0.004 / (2 * math.pi)
    assert o.active_blocks == 8 and o.active_box_cells == 8 * 14 ** 3  # (|x| < 0.04: 13 cells per direction and one more)


def test_defaults_are_the_references_and_mean_inactive():
    """a deck with none of the three configured (SNIa disabled, as every deck must say): every key at the reference's
    default, nothing active, an empty list, and the stages do not leave the fused path for them"""
    p = _plan(deck="cluster_hse")
    o = p.cluster_source_options()
    assert (o.snia_active, o.stellar_active, o.clips_active) == (0, 0, 0)
    assert (o.power_per_bcg_mass, o.mass_rate_per_bcg_mass) == (0.0, 0.0)
    assert (o.stellar_radius, o.exclusion_radius, o.efficiency, o.number_density_threshold, o.temperature_threshold) == (0.0,) * 5
    assert (o.clip_r, o.dfloor, o.vceil, o.vAceil, o.Tceil, o.eceil) == (-1.0, -1.0, INF, INF, INF, INF)
    assert o.active_blocks == 0 and o.active_box_cells == 0 and p.cluster_split_active_list() == []
    assert o.flux_path_sources == 1  # (cluster_hse runs its gravity source: unchanged)
    # ... and a deck with no source at all keeps flux_path_sources() false
    text = _without(DECK, "problem/cluster/snia_feedback", "problem/cluster/stellar_feedback", "problem/cluster/clips")
    q = _plan_text(text, [SNIA + "disabled=true"]).cluster_source_options()
    assert (q.snia_active, q.stellar_active, q.clips_active, q.flux_path_sources) == (0, 0, 0, 0)
    # each source alone puts the stages on the flux-array path
    for ov in ([SNIA + "disabled=false", SNIA + "power_per_bcg_mass=1e-3"],
               [SNIA + "disabled=true", CLIPS + "clip_r=0.02", CLIPS + "dfloor=1.0"],
               [SNIA + "disabled=true", STELLAR + "stellar_radius=0.03", STELLAR + "exclusion_radius=0.01", STELLAR + "efficiency=1e-6",
                STELLAR + "number_density_threshold=1.0", STELLAR + "temperature_threshold=1.0"]):
        assert _plan_text(text, ov).cluster_source_options().flux_path_sources == 1


def test_exclusion_radius_falls_back_to_the_accretion_radius():
    text = _without(DECK, "problem/cluster/stellar_feedback")
    ov = [STELLAR + "stellar_radius=0.03", STELLAR + "efficiency=1e-6", STELLAR + "number_density_threshold=1.0",
          STELLAR + "temperature_threshold=1.0"]
    o = _plan_text(text, ov + [TRIG + "accretion_radius=0.015"]).cluster_source_options()
    assert o.stellar_active == 1 and o.exclusion_radius == 0.015
    # an explicit value wins
    o = _plan_text(text, ov + [TRIG + "accretion_radius=0.015", STELLAR + "exclusion_radius=0.005"]).cluster_source_options()
    assert o.exclusion_radius == 0.005
    # neither: the block is partly set
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan_text(text, ov)
    assert "problem/cluster/stellar_feedback" in str(e.value) and "Enabling stellar feedback requires setting all parameters." in str(e.value)


def test_eceil_and_rho_const_bcg():
    u = _plan().units()
    for tceil, gamma in ((1e7, 1.6666666666666667), (3.5e8, 1.4)):
        o = _plan([CLIPS + "Tceil=%r" % tceil, "hydro/gamma=%r" % gamma]).cluster_source_options()
        assert o.eceil == tceil / u.mbar_over_kb / (gamma - 1.0)
    # no ceiling: eceil stays infinite
    o = _plan_text(_without(DECK, "problem/cluster/clips"), [CLIPS + "clip_r=0.02", CLIPS + "vceil=1.0"]).cluster_source_options()
    assert o.Tceil == INF and o.eceil == INF
    # rho_const_bcg follows the deck's BCG; NONE gives 0 (SNIa then has to be off)
    o = _plan(["problem/cluster/gravity/m_bcg_s=1.25e-3", "problem/cluster/gravity/r_bcg_s=0.0075"]).cluster_source_options()
    assert o.rho_const_bcg == 1.25e-3 * 0.0075 / (2 * math.pi)
    o = _plan(["problem/cluster/gravity/which_bcg_g=NONE", SNIA + "disabled=true"]).cluster_source_options()
    assert o.rho_const_bcg == 0.0 and o.snia_active == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("snia_no_rates", [SNIA + "power_per_bcg_mass=0", SNIA + "mass_rate_per_bcg_mass=0"], SNIA + "disabled", "no-op"),
    ("snia_no_bcg", ["problem/cluster/gravity/which_bcg_g=NONE"], SNIA + "disabled", "BCG must be defined for SNIA Feedback to be enabled"),
    ("snia_rkl2", RKL2, SNIA + "disabled", "rkl2"),
    ("stellar_partly", [STELLAR + "efficiency=0"], "problem/cluster/stellar_feedback", "Enabling stellar feedback requires setting all parameters."),
    ("stellar_partly_threshold", [STELLAR + "temperature_threshold=0"], "problem/cluster/stellar_feedback",
     "Enabling stellar feedback requires setting all parameters."),
    ("clip_r_without_limit", [CLIPS + "dfloor=-1", CLIPS + "vceil=inf", CLIPS + "Tceil=inf"], CLIPS + "clip_r", "no limit"),
    ("dfloor_without_clip_r", [CLIPS + "clip_r=-1", CLIPS + "vceil=inf", CLIPS + "Tceil=inf"], CLIPS + "dfloor", "clip_r <= 0"),
    ("vceil_without_clip_r", [CLIPS + "clip_r=0", CLIPS + "dfloor=-1", CLIPS + "Tceil=inf"], CLIPS + "vceil", "clip_r <= 0"),
    ("Tceil_without_clip_r", [CLIPS + "clip_r=-1", CLIPS + "dfloor=-1", CLIPS + "vceil=inf"], CLIPS + "Tceil", "clip_r <= 0"),
    ("vAceil_without_clip_r", [CLIPS + "clip_r=-1", CLIPS + "dfloor=-1", CLIPS + "vceil=inf", CLIPS + "Tceil=inf", CLIPS + "vAceil=3",
                               "hydro/fluid=glmmhd"], CLIPS + "vAceil", "clip_r <= 0"),
    ("vAceil_without_mhd", [CLIPS + "vAceil=3"], CLIPS + "vAceil", "glmmhd"),
]


@pytest.mark.parametrize("overrides,key,wording", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_name_their_key(overrides, key, wording):
    msg = _refused(overrides)
    assert key in msg and wording in msg, msg


def test_refusals_that_need_another_deck():
    snia_off = [SNIA + "disabled=true"]
    # rkl2 with stellar feedback alone, and with the clips alone
    text = _without(DECK, "problem/cluster/clips")
    from athenapk_amd import lib as L
    with pytest.raises(L.ApkError) as e:
        _plan_text(text, snia_off + RKL2)
    assert "problem/cluster/stellar_feedback" in str(e.value) and "rkl2" in str(e.value)
    text = _without(DECK, "problem/cluster/stellar_feedback")
    with pytest.raises(L.ApkError) as e:
        _plan_text(text, snia_off + RKL2)
    assert CLIPS + "clip_r" in str(e.value) and "rkl2" in str(e.value)
    # without <units> and He_mass_fraction: stellar feedback, and the temperature ceiling with the reference's text
    no_units = "\n".join(ln for ln in _without(DECK, "units").splitlines() if not ln.startswith("He_mass_fraction")) + "\n"
    with pytest.raises(L.ApkError) as e:
        _plan_text(no_units, snia_off)
    assert "problem/cluster/stellar_feedback" in str(e.value) and "units" in str(e.value)
    no_units_no_stellar = "\n".join(ln for ln in _without(DECK, "units", "problem/cluster/stellar_feedback").splitlines()
                                    if not ln.startswith("He_mass_fraction")) + "\n"
    with pytest.raises(L.ApkError) as e:
        _plan_text(no_units_no_stellar, snia_off)
    assert CLIPS + "Tceil" in str(e.value) and "Temperature ceiling requires units and gas composition" in str(e.value)
    # ... and without the ceiling the clips need no units
    o = _plan_text(no_units_no_stellar, snia_off + [CLIPS + "Tceil=inf"]).cluster_source_options()
    assert o.clips_active == 1 and o.eceil == INF
    # everything else stays refused
    assert "problem/cluster/reductions" in _refused(["problem/cluster/reductions/cold_temp_thresh=1e5"])


# ---- the active list ------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_cluster_triggering.py with radii of two to four cells
MESHES = {
    "eight_blocks": _mesh(16, 8) + _box((-0.1,) * 3, (0.1,) * 3) + [STELLAR + "stellar_radius=0.05", STELLAR + "exclusion_radius=0.025",
                                                                    CLIPS + "clip_r=0.045"],
    "odd_block": _mesh((33, 5, 3), (33, 5, 3)) + _box((-0.3, -0.11, -0.07), (0.36, 0.14, 0.05)) + [
        STELLAR + "stellar_radius=0.08", STELLAR + "exclusion_radius=0.03", CLIPS + "clip_r=0.06"],
    "centre_at_zero": _mesh(8, 8) + _box((-0.4375,) * 3, (0.5625,) * 3) + [STELLAR + "stellar_radius=0.25", STELLAR + "exclusion_radius=0.125",
                                                                           CLIPS + "clip_r=0.25"],
}


def _interior_centres(p, lb):
    info = p.info
    loc = p.block_gid(lb)[1]
    return [R.cell_centres(info.xmin[d], info.dx[d], loc[d] * info.mb[d], info.mb[d]) for d in range(3)]


def _check_list(p, radius):
    info = p.info
    ng, mb = info.ng, tuple(info.mb)
    boxes = {lb: (lo, hi) for lb, lo, hi in p.cluster_split_active_list()}
    o = p.cluster_source_options()
    assert len(boxes) == o.active_blocks
    cells = inside_total = 0
    for lb in range(info.nblocks_local):
        xs = _interior_centres(p, lb)
        X, Y, Z = np.meshgrid(xs[0], xs[1], xs[2], indexing="ij")
        inside = X * X + Y * Y + Z * Z <= radius * radius  # [i][j][k], the edge included
        listed = np.zeros(inside.shape, bool)
        if lb in boxes:
            lo, hi = boxes[lb]
            for d in range(3):  # interior boxes, not empty
                assert ng <= lo[d] < hi[d] <= ng + mb[d]
                want = CS.brute_force_box(xs[d], radius, ng)
                assert want is not None and lo[d] <= want[0] and want[1] <= hi[d] and want[0] - lo[d] <= 1 and hi[d] - want[1] <= 1
            listed[lo[0] - ng:hi[0] - ng, lo[1] - ng:hi[1] - ng, lo[2] - ng:hi[2] - ng] = True
            cells += int(listed.sum())
        assert not np.any(inside & ~listed), "block %d: a cell within the radius is outside its box" % lb
        inside_total += int(inside.sum())
    assert cells == o.active_box_cells and inside_total > 0
    return boxes


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_active_list_holds_every_interior_cell_within_the_radius(mesh):
    """the list is built for max(stellar_radius, clip_r); with one of the two switched off, for the other"""
    p = _plan(MESHES[mesh])
    o = p.cluster_source_options()
    boxes = _check_list(p, max(o.stellar_radius, o.clip_r))
    assert len(boxes) == (8 if mesh == "eight_blocks" else 1)
    if mesh != "centre_at_zero":  # (there both radii are 0.25)
        assert o.stellar_radius > o.clip_r
        q = _plan_text(_without(DECK, "problem/cluster/stellar_feedback"), [ov for ov in MESHES[mesh] if not ov.startswith(STELLAR)])
        oq = q.cluster_source_options()
        assert oq.stellar_active == 0 and oq.active_box_cells <= o.active_box_cells
        _check_list(q, oq.clip_r)


def test_active_list_of_each_rank_of_two_and_a_block_out_of_reach():
    total = 0
    for rank in range(2):
        p = _plan(MESHES["eight_blocks"], rank=rank, nranks=2)
        boxes = _check_list(p, 0.05)
        assert sorted(boxes) == [0, 1, 2, 3]
        total += p.cluster_source_options().active_box_cells
    assert total == _plan(MESHES["eight_blocks"]).cluster_source_options().active_box_cells
    # 32 x 8 x 8 in 16 x 8 x 8 blocks, the origin well inside the first block: the second is not listed
    ov = _mesh((32, 8, 8), (16, 8, 8)) + _box((-0.2, -0.1, -0.1), (0.6, 0.1, 0.1)) + [
        STELLAR + "stellar_radius=0.06", STELLAR + "exclusion_radius=0.02", CLIPS + "clip_r=0.05"]
    p = _plan(ov)
    assert sorted(_check_list(p, 0.06)) == [0]
