// stage_form.hpp -- which kernel form a fused stage takes (apk_stage_fused), decided ONCE, on the host, from the shape of
// the pack and the facts of the request: plan_stage() returns a StagePlan or a refusal with its reason.  The launchers
// (fused_kernel.hpp: launch_fused_stage) switch on the plan, the queries of the C API (apk_stage_form and the three older
// ones) read it.  Nothing here touches the device or a workspace pointer.
//
// The *_compiled() predicates say which template-argument tuples of a kernel family are instantiated: the plan asks them
// at run time (a tuple that is not compiled is a refusal), the launchers under `if constexpr` -- so neither can name a
// kernel the other does not know.
#pragma once

#include <type_traits>

#include "apk_internal.hpp"
#include "hydro_math.hpp"

namespace apk {

// what the finishing sweep does besides the RK update + Dedner source
enum { EXTRA_NONE = 0, EXTRA_C2P = 1, EXTRA_C2P_DT = 2 };

// ---- what is compiled ---------------------------------------------------------------------------
// (lean: 0 the general form, 1 lean, LEAN_PFLOOR lean but for a pressure floor / the trial count: fused_kernel.hpp, finish_cell)
// fused_dc3_kernel<FLUID, RS, EXTRA, LEAN, FROM_CONS>: from a conserved state in the lean form only; the pressure-floor
// form for stages with FillDerived; none that follows x1_halo
constexpr bool dc3_compiled(int extra, int lean, bool from_cons, bool x1h) {
  return !x1h && (from_cons ? lean == 1 : (lean != LEAN_PFLOOR || extra != EXTRA_NONE));
}
// fused_dc3r2_kernel<FLUID, RS, EXTRA, FROM_CONS, X1H, LEAN>: lean forms only; x1_halo for stages without the dt estimate
// (the predictor's place in a cycle); the pressure-floor form with FillDerived from stored primitives
constexpr bool dc3r2_compiled(int extra, bool from_cons, bool x1h, int lean) {
  return lean == 1 ? !(x1h && extra == EXTRA_C2P_DT) : (lean == LEAN_PFLOOR && !from_cons && !x1h && extra != EXTRA_NONE);
}
// fused_m12f_kernel<FLUID, RECON, RS, EXTRA, LEAN, FC, X1H>: from a conserved state / with x1_halo in the lean form only
constexpr bool m12f_compiled(int recon, int extra, int lean, bool from_cons, bool x1h) {
  return recon != APK_RC_DC && ((from_cons || x1h) ? lean == 1 : (lean != LEAN_PFLOOR || extra != EXTRA_NONE));
}
// fused_march_kernel<.., DIR = 3, FINAL = false, EXTRA_NONE, FC>: the x3 sweep of the two-kernel stage, both inputs
constexpr bool x3_sweep_compiled(int recon, bool /*from_cons*/) { return recon != APK_RC_DC; }
// fused_s3_kernel<FLUID, RECON, RS, EXTRA, SRC>: hydro with PLM for now -- 256 VGPRs, no scratch (WENO3 / LimO3 spill 44 - 98
// registers in this form, GLM-MHD would hold 2 x 9 x 7 doubles across a Riemann solve); no primitives stored
constexpr bool s3_compiled(int fluid, int recon, int extra, int src) {
  return fluid == APK_FLUID_EULER && recon == APK_RC_PLM && extra != EXTRA_C2P && (src == 1 || src == 2);
}

// ---- run-time value -> compile-time constant ----------------------------------------------------
// as_constants(f, among<0, 1, 2>{a}, among<0, 1>{b}) calls f(integral_constant<int, a>, integral_constant<int, b>) and
// returns what f returns (did it launch?); false if a value is not among those listed
template <int... Vs>
struct among {
  int v;
};
template <class F>
inline bool as_constants(F &&f) {
  return f();
}
template <class F, int... Vs, class... More>
inline bool as_constants(F &&f, among<Vs...> a, More... more) {
  return ((a.v == Vs && as_constants([&](auto... rest) { return f(std::integral_constant<int, Vs>{}, rest...); }, more...)) || ...);
}

// (the order of the arguments at the call sites and of the values listed decides where the kernels lie in the code object:
// the compiler emits the instantiations of one call in reverse)
using extra_among = among<EXTRA_NONE, EXTRA_C2P, EXTRA_C2P_DT>;

// ---- the request and the plan -------------------------------------------------------------------
struct StageRequest {
  int extra = EXTRA_NONE;
  int prim_to_u1 = 0, no_prim_store = 0;  // apk_stage_args.fill_derived >= 2 / == 3
  int prim_from_cons = 0;
  bool out_of_place = false;  // cons_out_delta != 0
  int phase = 0;
  bool window = false;  // phase 1 on index windows
  bool scalars = false, count_unphysical = false;
  int dedner = 0;
  apk_eos eos = {5.0 / 3.0, -1.0, -1.0, -1.0, __builtin_inf(), __builtin_inf()};  // (the reference's defaults: nothing acts)
  bool face_table = false;
  bool x1_halo = false;
  int x1_recv_depth = 0, x1_send_depth = 0, x1_send_field = 0;
};

struct StagePlan {
  int status = APK_OK;
  const char *reason = "";  // of a refusal: names the rule
  int form = APK_FORM_NONE;
  int extra = EXTRA_NONE;
  int lean = 0;       // 0 / 1 / LEAN_PFLOOR
  int dc_rows = 0;    // DC_MARCH: x2 rows per lane
  int from_cons = 0;  // 0, or apk_stage_args.prim_from_cons (the input the kernels convert)
  bool x1_halo = false;  // the kernels follow apk_stage_args.x1_halo
};

inline StagePlan refuse_stage(const char *reason, int status = APK_ERR_UNSUPPORTED) {
  StagePlan p;
  p.status = status;
  p.reason = reason;
  return p;
}

// A stage is LEAN when none of the finishing sweep's optional work is asked for: no passive scalars, no trial count
// (first-order flux correction), no extended Dedner source, and an equation of state whose velocity ceiling, pressure
// floor and energy ceiling are off (eos_is_lean).  The uniform-mesh cycles of the decks and of the benchmark are all of
// this kind.  1: lean; LEAN_PFLOOR: lean but for a pressure floor and / or the trial count -- the Orszag-Tang deck has
// both -- whose few instructions the forms <.., LEAN = 2> compile in; 0: the general form
inline int stage_lean_level(const StageRequest &r) {
  if (r.scalars || r.dedner == 2) return 0;
  if (!r.count_unphysical && eos_is_lean(r.eos)) return 1;
  return eos_is_lean_but_pfloor(r.eos) ? LEAN_PFLOOR : 0;
}

// can / should a stage take the two-kernel form?  3-D, a reconstruction with a stencil (ghost
// layers), FillDerived out of place or absent (K2's lanes read their x1 neighbours' primitives from
// memory), and rows long enough that the flattened (k, i) run keeps most lanes on interior cells
// (nx1 / (nx1 + 2 ng): 128 -> 96 %, 32 -> 84 %, 16 with nghost 4 -> 67 %).  Measured on the refined mesh of
// BASELINE config 5 (232 blocks of 16^3, MHD PPM+HLLD, nghost 4): 8.52e8 against 8.36e8 zone-cycles/s for the
// three-sweep schedule with several rows per wave, so 16-cell blocks take it too; narrower ones do not.
inline bool two_kernel_stage_applies(const PackView &u0, int recon, const StageRequest &r) {
  constexpr int min_nx1 = 16;
  // (blocks narrower than 32 cells only if they are deep enough along x3 for the plane windows of a split stage --
  // 4 nghost planes: the driver's overlap rule -- so that taking this form never costs an overlapped exchange)
  const bool wide_enough = u0.nx1 >= 32 || (u0.nx1 >= min_nx1 && u0.nx3 >= 4 * u0.ng);
  // (the marches address a block's cells as scalar row pointer + 32-bit byte offset of the lane: RowCellAt)
  const bool offsets_fit = (uint64_t)u0.sn * sizeof(double) < (1ull << 32);
  return u0.ndim == 3 && recon != APK_RC_DC && wide_enough && offsets_fit && (r.extra == EXTRA_NONE || r.prim_to_u1);
}

// does a stage take the single-march form?  A two-kernel stage with a three-point reconstruction, the lean form with its
// input derived from a conserved state (what a prim-free RK cycle asks of every stage), whole blocks (a split stage keeps
// the two kernels: its x3 sweep runs on plane windows while the halo messages fly), an even number of x2 rows, no
// primitives stored.
inline bool single_march_stage_applies(int fluid, const PackView &u0, int recon, const StageRequest &r) {
  // (rows of 32 cells and more: on the 16^3 blocks of a refined mesh the march's x1 halo lanes outnumber its cells and the
  // two-kernel form is faster -- refined hydro blast of BASELINE config 5, zone-cycles/s, same box: 16^3 blocks 2.02e9 with
  // this march against 2.32e9 with the two-kernel stage; 32^3: 4.55e9 against 4.17e9; 48^3: 5.85e9 against 5.23e9)
  return two_kernel_stage_applies(u0, recon, r) && s3_compiled(fluid, recon, r.extra, r.prim_from_cons) && u0.nx1 >= 32 &&
         r.phase == 0 && !r.window && stage_lean_level(r) == 1 && u0.nx2 % 2 == 0 && u0.nx2 >= 4 && u0.ng >= 2 &&
         (r.extra == EXTRA_NONE || r.no_prim_store) && (r.prim_from_cons == 1 || r.out_of_place);
}

// does a stage of this form follow apk_stage_args.x1_halo?  The lean two-row donor-cell march and the lean two-kernel
// stage's finishing march, from stored primitives or from a conserved state (plan_stage refuses the single march)
inline bool x1_halo_stage_ok(const PackView &u0, int recon, const StageRequest &r) {
  if (u0.ndim != 3 || stage_lean_level(r) != 1 || r.window) return false;
  const int deepest = r.x1_send_depth > r.x1_recv_depth ? r.x1_send_depth : r.x1_recv_depth;
  if (u0.nx1 < 2 * deepest || r.x1_send_depth < 0 || r.x1_recv_depth < 0 || r.x1_recv_depth > u0.ng) return false;
  if (r.x1_send_field == 1 && r.extra == EXTRA_NONE) return false;  // (primitives to send: a stage that computes them)
  if (recon == APK_RC_DC)  // the two-row march, which has no form with the time-step estimate for it
    return r.phase == 0 && (r.extra == EXTRA_NONE || (r.prim_to_u1 && r.extra == EXTRA_C2P)) && u0.nx2 % 2 == 0 && u0.nx2 >= 4;
  return two_kernel_stage_applies(u0, recon, r);
}

// The rules, in the order they are asked (DESIGN.md section 3.1 has them as a table)
inline StagePlan plan_stage(int fluid, int recon, const PackView &u0, const StageRequest &r) {
  const bool dc = recon == APK_RC_DC;
  const bool two_kernel = two_kernel_stage_applies(u0, recon, r);
  const bool single_march = single_march_stage_applies(fluid, u0, recon, r);
  const int level = stage_lean_level(r);
  const bool dc_out_of_place = r.extra == EXTRA_NONE || r.prim_to_u1;  // the single donor-cell march: no FillDerived in place
  StagePlan p;
  p.extra = r.extra;
  p.from_cons = r.prim_from_cons;
  // (the lean form with a pressure floor / the trial count: stages with FillDerived from stored primitives)
  p.lean = level == LEAN_PFLOOR ? ((r.extra != EXTRA_NONE && !r.prim_from_cons && !r.x1_halo) ? LEAN_PFLOOR : 0) : level;

  // split stage: where the x1 sweep is its own, non-finishing kernel, or the single-kernel
  // 3-D donor-cell stage with out-of-place (or no) FillDerived
  if (r.phase != 0 && u0.ndim == 1) return refuse_stage("a 1-D stage cannot be split (phase != 0)");
  if (r.phase != 0 && dc && u0.ndim == 3) {
    if (!(r.extra == EXTRA_NONE || (r.prim_to_u1 && r.extra == EXTRA_C2P)))
      return refuse_stage("a split 3-D donor-cell stage takes fill_derived = 0 or 2 without estimate_dt");
    if (r.phase == 2) {  // the cells were all retired in phase 1; only the scalars are left
      p.form = APK_FORM_DC_MARCH;
      p.dc_rows = 1;
      return p;
    }
  }
  // only the kernels that follow the table: the single-march donor-cell stage and the two-kernel
  // stage; nothing that reads neighbouring cells from memory by plain index arithmetic
  if (r.face_table && (u0.ndim != 3 || r.scalars || r.dedner == 2 || !(dc ? dc_out_of_place : two_kernel)))
    return refuse_stage("face_neighbor: 3-D single-march donor-cell or two-kernel stages only, without passive scalars or dedner = 2");
  // apk_stage_args.x1_halo: the lean two-row donor-cell march and the lean two-kernel stage's finishing march (phase 1 of
  // a split two-kernel stage is the x3 sweep, which reads no x1 ghost column and retires nothing: it ignores the table)
  p.x1_halo = r.x1_halo && !(!dc && r.phase == 1);
  if (p.x1_halo && !x1_halo_stage_ok(u0, recon, r))
    return refuse_stage("x1_halo: whole lean 3-D stages only -- the two-row donor-cell march or the two-kernel stage, segments that fit the block");
  if (p.x1_halo && single_march) return refuse_stage("x1_halo: the single march does not follow it");
  if (r.no_prim_store && !(u0.ndim == 3 && !dc && level == 1 && two_kernel))
    return refuse_stage("fill_derived = 3: the lean two-kernel stage only");
  if (r.prim_from_cons) {
    const bool dc_ok = dc && r.prim_from_cons == 1 && dc_out_of_place;
    // the two-kernel stage, whole or split (a stage that reads u0's conserved state writes its result elsewhere)
    const bool two_ok = two_kernel && !r.scalars && (r.prim_from_cons == 1 || r.out_of_place);
    if (!(u0.ndim == 3 && level == 1 && (dc_ok || two_ok)))
      return refuse_stage("prim_from_cons: the lean single-march donor-cell stage (1) or the lean two-kernel stage (1, or 2 out of place) only");
  }

  if (u0.ndim == 1) {
    p.form = APK_FORM_X1;
  } else if (u0.ndim == 2) {
    p.form = APK_FORM_X1_X2;
  } else if (dc && dc_out_of_place) {
    // whole donor-cell stage in one march; two rows per lane: whole blocks only -- a split stage's windows and odd row
    // counts keep the one-row kernel, in the SAME lean form (the product build's update expression is the form's, and a
    // split stage must reproduce the whole one bit for bit)
    p.form = APK_FORM_DC_MARCH;
    p.dc_rows = (p.lean != 0 && !r.window && u0.nx2 % 2 == 0 && u0.nx2 >= 4) ? 2 : 1;
    if (!(p.dc_rows == 2 ? dc3r2_compiled(p.extra, p.from_cons != 0, p.x1_halo, p.lean) : dc3_compiled(p.extra, p.lean, p.from_cons != 0, p.x1_halo)))
      return refuse_stage("donor-cell march: this combination of fill_derived / estimate_dt, lean level, prim_from_cons and x1_halo is not compiled");
  } else if (dc) {
    p.form = APK_FORM_MARCH12_X3;  // FillDerived in place: x1 + x2 in one march, then the finishing x3 march
  } else if (single_march) {
    p.form = APK_FORM_SINGLE_MARCH;
  } else if (two_kernel) {
    p.form = APK_FORM_TWO_KERNEL;
    if (!x3_sweep_compiled(recon, p.from_cons != 0) || !m12f_compiled(recon, p.extra, p.lean, p.from_cons != 0, p.x1_halo))
      return refuse_stage("two-kernel stage: this combination of fill_derived / estimate_dt, lean level, prim_from_cons and x1_halo is not compiled");
  } else {
    p.form = APK_FORM_THREE_SWEEP;
  }
  // (the forms built from the general kernels)
  if (p.form != APK_FORM_DC_MARCH && p.form != APK_FORM_TWO_KERNEL && p.form != APK_FORM_SINGLE_MARCH) p.lean = 0;
  return p;
}

// the same from apk_stage_args: checks what launch_stage_fused checks of them, then asks plan_stage (fused_dispatch.hip)
StagePlan plan_stage_args(const PackView &u0, const apk_stage_args &a);

}  // namespace apk
