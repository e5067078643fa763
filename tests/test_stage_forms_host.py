"""CPU test of the fused stage's decision table (no GPU): apk_stage_form on descriptors only -- which kernel form
apk_stage_fused takes for a scheme, a block shape and a set of arguments, or which rule refuses them (csrc/stage_form.hpp:
plan_stage).  The expectations are what the launch code did before the plan existed."""
import ctypes as C

import pytest

from athenapk_amd import hydro
from athenapk_amd import lib as L

OK, INVALID, UNSUPPORTED = L.APK_OK, L.APK_ERR_INVALID, L.APK_ERR_UNSUPPORTED
NGHOST = {"dc": 2, "plm": 2, "ppm": 3}
MHD_PPM, MHD_DC, MHD_PLM, HYDRO_PLM = ("glmmhd", "ppm", "hlld"), ("glmmhd", "dc", "hlld"), ("glmmhd", "plm", "hlld"), ("euler", "plm", "hllc")
_X1 = L.X1Halo(1, 0, 0, 0)  # (a block table that is only tested for NULL, no segments)


@pytest.fixture(scope="module")
def lib():
    return L.load(True)


def form(lib, scheme, nx, ng=None, nscalars=0, eos=None, x1_halo=False, window=False, face_table=False, **kw):
    fluid, recon, riemann = scheme
    desc = L.PackDesc()
    desc.nblocks, desc.nhydro, desc.nscalars = 2, (9 if fluid == "glmmhd" else 5), nscalars
    desc.ng = NGHOST[recon] if ng is None else ng
    desc.nx[:] = list(nx)
    a = L.StageArgs()
    a.cfg = L.FluxCfg(L.FLUID[fluid], L.RECON[recon], L.RIEMANN[riemann])
    a.eos = eos or L.make_eos(5.0 / 3.0)
    a.c_h, a.gam0, a.gam1, a.beta_dt, a.glmmhd_alpha, a.mindx = 1.5, 0.0, 1.0, 1.0e-3, 0.1, 0.1
    a.dedner = 1 if fluid == "glmmhd" else 0
    if window:  # (pointers are only tested for NULL)
        a.window, a.window_rl, a.window_rows = 8, desc.nx[0] + 2 * desc.ng, desc.nx[1]
    if face_table:
        a.face_neighbor = 8
    if x1_halo:
        a.x1_halo = C.addressof(_X1)
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return hydro.StageForm(lib, desc, a)


# scheme, shape, arguments, expected status, expected form [, lean, donor-cell rows per lane]
TABLE = [
    (MHD_PPM, (36, 9, 10), dict(fill_derived=2), OK, "TWO_KERNEL"),
    (MHD_PPM, (36, 9, 10), dict(fill_derived=1), OK, "THREE_SWEEP"),
    (MHD_PPM, (36, 9, 10), dict(fill_derived=3), INVALID, "NONE"),
    (MHD_PPM, (16, 16, 16), dict(ng=4), OK, "TWO_KERNEL"),
    (MHD_PPM, (16, 16, 8), dict(ng=4), OK, "THREE_SWEEP"),
    (MHD_PPM, (12, 16, 16), dict(ng=4), OK, "THREE_SWEEP"),
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=1, fill_derived=0), OK, "SINGLE_MARCH"),
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=1, fill_derived=3, estimate_dt=1), OK, "SINGLE_MARCH"),
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=1, fill_derived=2), OK, "TWO_KERNEL"),
    (HYDRO_PLM, (36, 9, 10), dict(prim_from_cons=1), OK, "TWO_KERNEL"),  # odd nx2
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=1, phase=1, window=True), OK, "TWO_KERNEL"),
    (MHD_PLM, (36, 10, 9), dict(prim_from_cons=1), OK, "TWO_KERNEL"),
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=1, x1_halo=True), UNSUPPORTED, "NONE"),
    (MHD_DC, (36, 8, 10), dict(fill_derived=2), OK, "DC_MARCH", 1, 2),
    (MHD_DC, (36, 9, 10), dict(fill_derived=2), OK, "DC_MARCH", 1, 1),
    (MHD_DC, (36, 8, 10), dict(fill_derived=2, eos=L.make_eos(5.0 / 3.0, pfloor=1e-6)), OK, "DC_MARCH", L.LEAN_PFLOOR, 2),
    (MHD_DC, (36, 8, 10), dict(fill_derived=0, eos=L.make_eos(5.0 / 3.0, pfloor=1e-6)), OK, "DC_MARCH", 0, 1),
    (MHD_DC, (36, 8, 10), dict(fill_derived=2, dedner=2), OK, "DC_MARCH", 0, 1),
    (MHD_DC, (36, 8, 10), dict(fill_derived=1), OK, "MARCH12_X3"),
    (MHD_DC, (36, 8, 10), dict(fill_derived=3, estimate_dt=1), UNSUPPORTED, "NONE"),
    (MHD_PPM, (64, 64, 1), dict(), OK, "X1_X2"),
    (MHD_DC, (64, 64, 1), dict(fill_derived=1), OK, "X1_X2"),
    (HYDRO_PLM, (64, 1, 1), dict(fill_derived=0), OK, "X1"),
    (HYDRO_PLM, (64, 1, 1), dict(fill_derived=1), UNSUPPORTED, "NONE"),
    (MHD_PPM, (36, 8, 10), dict(nscalars=2, face_table=True), UNSUPPORTED, "NONE"),
    (MHD_PPM, (36, 8, 10), dict(nscalars=2, cons_out_delta=4096), UNSUPPORTED, "NONE"),
    # beyond the forms themselves: the variants a plan carries, and split stages
    (MHD_PPM, (36, 8, 10), dict(fill_derived=2, count_unphysical=1), OK, "TWO_KERNEL", L.LEAN_PFLOOR),
    (MHD_PPM, (36, 8, 10), dict(fill_derived=0, count_unphysical=1), OK, "TWO_KERNEL", 0),
    (MHD_PPM, (36, 8, 10), dict(nscalars=2), OK, "TWO_KERNEL", 0),
    (MHD_PPM, (36, 8, 10), dict(fill_derived=2, x1_halo=True), OK, "TWO_KERNEL", 1),
    (MHD_PPM, (36, 8, 10), dict(fill_derived=2, x1_halo=True, eos=L.make_eos(5.0 / 3.0, pfloor=1e-6)), UNSUPPORTED, "NONE"),
    (MHD_PPM, (36, 8, 10), dict(phase=2, fill_derived=2, estimate_dt=1), OK, "TWO_KERNEL", 1),
    (MHD_PPM, (36, 9, 10), dict(phase=2, fill_derived=1), OK, "THREE_SWEEP", 0),
    (MHD_PPM, (36, 8, 10), dict(face_table=True), OK, "TWO_KERNEL", 1),
    (MHD_PPM, (36, 8, 10), dict(face_table=True, fill_derived=1), UNSUPPORTED, "NONE"),
    (MHD_DC, (36, 8, 10), dict(phase=1, window=True, fill_derived=2), OK, "DC_MARCH", 1, 1),
    (MHD_DC, (36, 8, 10), dict(phase=2, fill_derived=2), OK, "DC_MARCH"),
    (MHD_DC, (36, 8, 10), dict(phase=2, fill_derived=1), UNSUPPORTED, "NONE"),
    (MHD_DC, (36, 8, 10), dict(fill_derived=2, x1_halo=True), OK, "DC_MARCH", 1, 2),
    (MHD_DC, (36, 9, 10), dict(fill_derived=2, x1_halo=True), UNSUPPORTED, "NONE"),
    (MHD_DC, (36, 8, 10), dict(fill_derived=2, prim_from_cons=1), OK, "DC_MARCH", 1, 2),
    (MHD_DC, (36, 8, 10), dict(fill_derived=2, prim_from_cons=1, dedner=2), UNSUPPORTED, "NONE"),
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=2), INVALID, "NONE"),
    (HYDRO_PLM, (36, 10, 9), dict(prim_from_cons=2, cons_out_delta=4096), OK, "SINGLE_MARCH", 1),
    (HYDRO_PLM, (16, 16, 16), dict(prim_from_cons=1), OK, "TWO_KERNEL", 1),  # rows shorter than 32 cells keep the two kernels
    (HYDRO_PLM, (64, 64, 1), dict(phase=1, window=True), OK, "X1_X2"),
    (HYDRO_PLM, (64, 1, 1), dict(phase=2), UNSUPPORTED, "NONE"),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s-%s-%s" % ("_".join(r[0]), "x".join(map(str, r[1])), "-".join("%s=%s" % (
    k, v if isinstance(v, (int, bool)) else "set") for k, v in r[2].items()) or "plain"))
def test_form_of_a_stage(lib, row):
    scheme, nx, kw, status, name = row[:5]
    rc, info = form(lib, scheme, nx, **kw)
    assert (rc, info["form"]) == (status, name), info
    if len(row) > 5:
        assert info["lean"] == row[5], info
    if len(row) > 6:
        assert info["dc_rows"] == row[6], info
    assert (info["reason"] != "") == (rc != OK), info  # every refusal says why, an accepted stage says nothing


def test_variants_of_a_plan(lib):
    rc, info = form(lib, HYDRO_PLM, (36, 9, 10), prim_from_cons=2, cons_out_delta=4096, x1_halo=True)
    assert rc == OK and (info["form"], info["from_cons"], info["x1_halo"], info["lean"]) == ("TWO_KERNEL", 2, True, 1)
    # phase 1 of a split two-kernel stage is the x3 sweep, which ignores the x1 table
    rc, info = form(lib, MHD_PPM, (36, 8, 10), phase=1, window=True, x1_halo=True)
    assert rc == OK and (info["form"], info["x1_halo"]) == ("TWO_KERNEL", False)
    rc, info = form(lib, MHD_DC, (36, 8, 10))
    assert rc == OK and (info["from_cons"], info["x1_halo"], info["dc_rows"]) == (0, False, 2)


def test_refusals_by_different_rules_give_different_reasons(lib):
    refusals = [
        form(lib, HYDRO_PLM, (64, 1, 1), phase=2),                                   # a split 1-D stage
        form(lib, MHD_DC, (36, 8, 10), phase=2, fill_derived=1),                     # split donor cell, FillDerived in place
        form(lib, MHD_PPM, (36, 8, 10), nscalars=2, face_table=True),                # face table with scalars
        form(lib, MHD_DC, (36, 9, 10), fill_derived=2, x1_halo=True),                # x1 halo, one-row march
        form(lib, HYDRO_PLM, (36, 10, 9), prim_from_cons=1, x1_halo=True),           # x1 halo, single march
        form(lib, MHD_DC, (36, 8, 10), fill_derived=3, estimate_dt=1),               # fill_derived = 3 outside the two-kernel stage
        form(lib, MHD_DC, (36, 8, 10), fill_derived=2, prim_from_cons=1, dedner=2),  # prim_from_cons, not lean
        form(lib, MHD_PPM, (36, 8, 10), nscalars=2, cons_out_delta=4096),            # out of place with scalars
        form(lib, MHD_PPM, (36, 8, 10), nscalars=2, count_unphysical=1),             # trial count with scalars
        form(lib, HYDRO_PLM, (64, 1, 1), fill_derived=1),                            # FillDerived in 1-D
        form(lib, MHD_PPM, (36, 9, 10), fill_derived=3),                             # fill_derived = 3 without estimate_dt
        form(lib, MHD_PPM, (36, 9, 10), estimate_dt=1),                              # estimate_dt without fill_derived
        form(lib, MHD_PPM, (36, 9, 10), cons_store=3),
        form(lib, MHD_PPM, (36, 9, 10), ng=2),                                       # too few ghost zones
    ]
    assert all(rc != OK and info["form"] == "NONE" and info["reason"] for rc, info in refusals), refusals
    reasons = [info["reason"] for _, info in refusals]
    assert len(set(reasons)) == len(reasons), reasons
    assert refusals[-1][0] == L.APK_ERR_NGHOST


def test_bad_calls(lib):
    assert lib.apk_stage_form(None, None, None) == INVALID
    rc, info = form(lib, MHD_PPM, (36, 1, 10))  # nx2 == 1 requires nx3 == 1
    assert rc == INVALID and info["reason"]
