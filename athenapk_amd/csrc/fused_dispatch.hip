// fused_dispatch.hip -- entry of the fused stage path: asks for the stage's plan (stage_form.hpp), sizes the
// workspaces of the handle and picks the (fluid, riemann) family.
#include "fused_kernel.hpp"

namespace apk {

// what the arguments ask for, checked and condensed to the facts plan_stage reads, and the plan for them (the ranges of
// fill_derived, prim_from_cons and phase: apk_stage_fused has checked)
StagePlan plan_stage_args(const PackView &u0, const apk_stage_args &a) {
  StageRequest r;
  r.scalars = u0.nvar != u0.nhydro;
  if (a.x1_halo) {
    if (!a.x1_halo->blocks || a.x1_halo->send_field < 0 || a.x1_halo->send_field > 1)
      return refuse_stage("x1_halo: no block table, or send_field not 0 or 1", APK_ERR_INVALID);
    r.x1_halo = true;
    r.x1_recv_depth = a.x1_halo->recv_depth;
    r.x1_send_depth = a.x1_halo->send_depth;
    r.x1_send_field = a.x1_halo->send_field;
  }
  if (a.cons_store < 0 || a.cons_store > 2) return refuse_stage("cons_store must be 0, 1 or 2", APK_ERR_INVALID);
  if (a.cons_out_delta != 0 && r.scalars) return refuse_stage("cons_out_delta: not with passive scalars (their kernels update in place)");
  if (a.count_unphysical && r.scalars) return refuse_stage("count_unphysical: not with passive scalars (they are updated by their own kernel)");
  if (a.fill_derived) {
    // in-place prim replacement is only safe when the finishing sweep is a march (x2/x3) and
    // the extended Dedner source does not read neighbouring primitives (out of place it may)
    if (u0.ndim == 1 || (a.dedner == 2 && a.fill_derived != 2))
      return refuse_stage("fill_derived: not in 1-D, and with dedner = 2 only out of place (fill_derived = 2)");
    r.extra = a.estimate_dt ? EXTRA_C2P_DT : EXTRA_C2P;
  } else if (a.estimate_dt) {
    return refuse_stage("estimate_dt needs fill_derived", APK_ERR_INVALID);
  }
  r.prim_to_u1 = (a.fill_derived >= 2) ? 1 : 0;
  r.no_prim_store = (a.fill_derived == 3) ? 1 : 0;
  r.prim_from_cons = a.prim_from_cons;
  r.out_of_place = a.cons_out_delta != 0;
  r.phase = a.phase;
  r.window = a.phase == 1 && a.window != nullptr;
  r.count_unphysical = a.count_unphysical != 0;
  r.dedner = a.dedner;
  r.eos = a.eos;
  r.face_table = a.face_neighbor != nullptr;
  return plan_stage(a.cfg.fluid, a.cfg.recon, u0, r);
}

int launch_stage_fused(apk_ctx *ctx, const PackView &u0, const PackView &u1,
                       const apk_stage_args &a, double dedner_coeff, hipStream_t s, const char *&why) {
  // (a refused stage enqueues nothing and sizes no workspace)
  const StagePlan plan = plan_stage_args(u0, a);
  if (plan.status != APK_OK) {
    why = plan.reason;
    return plan.status;
  }
  StageParams sp;
  sp.mflux = nullptr;
  if (u0.nvar != u0.nhydro) {
    // passive scalars: the sweeps leave the mass fluxes in a workspace of the handle
    if (ctx->d_mflux.reserve(ctx, 3 * (size_t)u0.nblocks * (size_t)u0.sn, s) != APK_OK) return APK_ERR_DEVICE;
    sp.mflux = ctx->d_mflux.p;
  }
  sp.gamma = a.eos.gamma;
  sp.c_h = a.c_h;
  sp.k = make_stage_consts(a.eos.gamma, a.c_h, a.eos);
  sp.gam0 = a.gam0;
  sp.gam1 = a.gam1;
  sp.beta_dt = a.beta_dt;
  sp.dedner = a.dedner;
  sp.dedner_coeff = dedner_coeff;
  sp.du = nullptr;
  sp.du_first = 0;
  sp.du_pitch = 0;
  sp.ctx = ctx;
#if APK_M12F_WAVE_ENDS
  sp.prio_off = wave_ends_env("APK_WAVE_PRIORITY_OFF", 0);
#endif
  sp.eos = a.eos;
  sp.flags = ctx->d_flags + (a.trial ? 1 : 0);
  sp.dt_bits = ctx->dt_word();  // min of the finishing sweep (apk_stage_dt_read)
  sp.bad_count = nullptr;
  sp.out_delta = a.cons_out_delta;
  sp.face_nbr = a.face_neighbor;
  sp.x1_blocks = nullptr;
  sp.x1_recv_depth = sp.x1_send_depth = sp.x1_send_field = 0;
  if (a.x1_halo) {
    sp.x1_blocks = a.x1_halo->blocks;
    sp.x1_recv_depth = a.x1_halo->recv_depth;
    sp.x1_send_depth = a.x1_halo->send_depth;
    sp.x1_send_field = a.x1_halo->send_field;
  }
  // (only the stage whose primitives go out of place may drop its conserved result; a windowed phase keeps everything)
  sp.cons_store = (a.fill_derived == 2 && !a.trial && a.cons_out_delta == 0) ? a.cons_store : 0;
  if (a.count_unphysical) {     // cells failing FirstOrderFluxCorrect's test (apk_stage_unphysical_read)
    sp.bad_count = ctx->bad_count_word();
    if (a.phase != 2 && hipMemsetAsync(sp.bad_count, 0, sizeof(unsigned long long), s) != hipSuccess) return APK_ERR_DEVICE;
  }
  sp.prim_to_u1 = (a.fill_derived >= 2) ? 1 : 0;
  sp.no_prim_store = (a.fill_derived == 3) ? 1 : 0;
  sp.prim_from_cons = a.prim_from_cons;
  sp.phase = a.phase;
  sp.window = (a.phase == 1) ? a.window : nullptr;
  sp.window_rl = a.window_rl;
  sp.window_rows = a.window_rows;
  if (plan.extra == EXTRA_C2P_DT && a.phase != 1) {  // (a split stage reduces dt in phase 2)
    if (prepare_dt_word(ctx, s) != APK_OK) return APK_ERR_DEVICE;
  }
  if (u0.ndim > 1) {
    // workspace owned by the handle, grown on demand
    if (ctx->d_du.reserve(ctx, (size_t)u0.nblocks * (size_t)u0.nvar * (size_t)u0.sn, s) != APK_OK) return APK_ERR_DEVICE;
    sp.du = ctx->d_du.p;
  }
  if (a.cfg.fluid == APK_FLUID_EULER) {
    if (a.cfg.riemann == APK_RS_HLLE) return launch_fused_euler_hlle(u0, u1, a.cfg.recon, sp, plan, s);
    if (a.cfg.riemann == APK_RS_HLLC) return launch_fused_euler_hllc(u0, u1, a.cfg.recon, sp, plan, s);
  } else if (a.cfg.fluid == APK_FLUID_GLMMHD) {
    if (a.cfg.riemann == APK_RS_HLLE) return launch_fused_mhd_hlle(u0, u1, a.cfg.recon, sp, plan, s);
    if (a.cfg.riemann == APK_RS_HLLD) return launch_fused_mhd_hlld(u0, u1, a.cfg.recon, sp, plan, s);
  }
  return APK_ERR_UNSUPPORTED;
}

}  // namespace apk
