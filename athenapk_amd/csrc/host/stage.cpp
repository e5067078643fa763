// stage.cpp -- the stage loop of the standalone host driver: the ghost exchange of uniform meshes, the predicates that
// say which form a cycle's stages and exchanges take, the completion of what those forms leave undone (sync_ghosts), and
// one stage of HydroDriver::MakeTaskCollection (do_stage).
#include "sim_internal.hpp"
#include "../hydro_math.hpp"

using namespace apk;

namespace apk {
namespace host {

// Ghost exchange in two halves.  begin: same-rank copies, message packing, post the transfers;
// end: wait for them, unpack, physical boundaries (x1, x2, x3).  With c2p the copies that fill
// ghost zones also convert them to primitives (apk_copy_plan_run_c2p), which replaces the separate
// ghost ConsToPrim pass -- and, around an exchange in flight, splits it by construction: the
// same-rank part in `begin`, the rest in `end`.
bool ghost_c2p_fusable(const apk_sim *s) {
  const apk_eos &e = s->pkg.eos;
  return !(e.dfloor > 0.0 || e.pfloor > 0.0 || e.efloor > 0.0 || e.vceil < 1.0e300 || e.eceil < 1.0e300);
}

// c2p: GHOST_COPY (plain), GHOST_C2P (cons and prim), GHOST_PRIM_ONLY (sim_internal.hpp)
int run_ghost_plan(apk_sim *s, int buf, int phase, int c2p, apk_stream_t stream) {
  if (!stream) stream = s->stream;
  if (!c2p) return apk_copy_plan_run(s->ctx, s->plans_of[buf][phase], stream);
  if (c2p == GHOST_PRIM_COPY) return apk_copy_plan_run(s->ctx, s->pplans_of[s->xchg_prim][phase], stream);
  const int64_t delta = s->d_prim2[s->pcur] - s->d_cons2[buf];
  // a boundary phase that is followed by another non-empty one copies corner cells from ghost
  // zones only that later phase fills: their (overwritten) primitives must not raise flags
  int latch = 1;
  for (int later = phase + 1; phase >= PH_BC1 && later <= PH_BC3; ++later)
    if (!s->mesh.plan[later].empty()) latch = 0;
  // direct neighbour addressing: the corner cells of a boundary phase are copied out of same-rank ghost
  // zones nobody fills (or reads); the other cells repeat interior cells, whose flags are latched there
  if (phase >= PH_BC1 && s->local_ghosts_stale) latch = 0;
  if (c2p == GHOST_PRIM_ONLY) return apk_copy_plan_run_c2p_prim_only(s->ctx, s->plans_of[buf][phase], s->pkg.fluid, &s->pkg.eos, delta, latch, stream);
  return apk_copy_plan_run_c2p(s->ctx, s->plans_of[buf][phase], s->pkg.fluid, &s->pkg.eos, delta, latch, stream);
}

// make the one-layer (or the full) message set the one the transports see (apk_sim_peer)
void select_thin_messages(apk_sim *s, bool thin) {
  if (s->thin_msgs == thin) return;
  s->thin_msgs = thin;
  s->msg_generation += 1;
}

int exchange_begin(apk_sim *s, bool async, int c2p, bool skip_local, bool thin) {
  const bool remote = !s->mesh.peers.empty();
  thin = thin && remote;
  s->xchg_thin = thin;
  // (x1 strips that never pass through a copy kernel: the stage just run has stored them into the send buffers, and the
  // stage that follows this exchange reads them from the receive buffers -- do_stage has checked that it will)
  const bool nox1 = remote && s->x1_out_direct;
  s->x1_out_direct = false;
  s->xchg_x1_direct = nox1;
  s->x1_in_recv = false;
  if (remote) {
    select_thin_messages(s, thin);
    s->remote_ghosts_thin = thin;  // (once this exchange is complete)
    if (thin) s->thin_exchanges += 1;
    if (nox1) s->x1_direct_exchanges += 1;
    if (c2p == GHOST_PRIM_COPY) {
      if (thin) return fail(s, APK_ERR_INVALID, "exchange_begin: a one-layer exchange carries the conserved state");
      s->xchg_prim = s->pcur;
      SIM_TRY(s, apk_copy_plan_run(s->ctx, s->pplans_of[s->pcur][nox1 ? PH_PACK_NOX1 : PH_PACK], s->stream));
    } else {
      SIM_TRY(s, apk_copy_plan_run(s->ctx, s->plan(thin ? (nox1 ? PH_PACK_THIN_NOX1 : PH_PACK_THIN) : (nox1 ? PH_PACK_NOX1 : PH_PACK)), s->stream));
    }
  } else if (c2p == GHOST_PRIM_COPY) {
    s->xchg_prim = s->pcur;
  }
  if (skip_local) {
    // direct neighbour addressing: the stages read their same-rank neighbours' interiors
    s->local_ghosts_stale = true;
    s->skipped_local_exchanges += 1;
  } else {
    SIM_TRY(s, run_ghost_plan(s, s->cur, PH_LOCAL, c2p));
  }
  if (remote) {
    if (!s->have_comm || !s->comm.exchange) return fail(s, APK_ERR_INVALID, "remote neighbours but no comm ops");
    if (async) {
      if (s->comm.exchange_begin(s->comm.user) != 0) return fail(s, APK_ERR_DEVICE, std::string("halo exchange (begin) failed ") + apk_sim_comm_error(s));
    } else if (s->comm.exchange(s->comm.user) != 0) {
      return fail(s, APK_ERR_DEVICE, "halo exchange failed");
    }
  }
  if (async) {
    s->exchange_pending = true;
    s->pending_cons = s->cur;
    s->pending_c2p = c2p;
  }
  return APK_OK;
}

int exchange_end(apk_sim *s, int c2p) {
  // an exchange left in flight targets the buffer that held the state when it was posted: the
  // first stage of the next cycle has swapped the buffer roles by the time it completes it
  const int buf = s->exchange_pending ? s->pending_cons : s->cur;
  if (s->exchange_pending) {
    if (!s->mesh.peers.empty() && s->comm.exchange_end(s->comm.user) != 0)
      return fail(s, APK_ERR_DEVICE, std::string("halo exchange (end) failed ") + apk_sim_comm_error(s));
    s->exchange_pending = false;
  }
  if (!s->mesh.peers.empty()) {
    const bool nox1 = s->xchg_x1_direct;
    SIM_TRY(s, run_ghost_plan(s, buf, s->xchg_thin ? (nox1 ? PH_UNPACK_THIN_NOX1 : PH_UNPACK_THIN) : (nox1 ? PH_UNPACK_NOX1 : PH_UNPACK), c2p));
    s->x1_in_recv = nox1;
  }
  for (int ph = PH_BC1; ph <= PH_BC3; ++ph) SIM_TRY(s, run_ghost_plan(s, buf, ph, c2p));
  return APK_OK;
}

int exchange_ghosts(apk_sim *s, int c2p, bool skip_local, bool thin) {
  if (s->amr) return amr_exchange(s, s->cur);
  if (!skip_local) s->local_ghosts_stale = false;  // (a full exchange of the current state)
  SIM_TRY(s, exchange_begin(s, false, c2p, skip_local, thin));
  return exchange_end(s, c2p);
}

// one rank, every active direction periodic: the face table covers every face of every block, so an exchange that
// follows it has no ghost zone left to fill (edges and corners are read by no stage that follows the table)
bool table_covers_all_faces(const apk_sim *s) { return s->mesh.peers.empty() && s->mesh.AllPeriodic(); }

// passive scalars or the extended Dedner source: their kernels read neighbouring cells by plain index arithmetic, so
// none of the leaner stage and exchange forms below takes them
static bool scalars_or_extended_dedner(const apk_sim *s) {
  return s->pkg.nscalars != 0 || (s->pkg.fluid == APK_FLUID_GLMMHD && s->pkg.glmmhd_source_extended);
}

// is every stage of the cycle that is not a donor-cell stage the two-kernel stage when it runs with this fill_derived?
static bool high_order_stages_are_two_kernel(const apk_sim *s, int fill_derived) {
  for (const apk_flux_cfg *cfg : {&s->pkg.flux_first_stage, &s->pkg.flux_other_stage})
    if (cfg->recon != APK_RC_DC && apk_stage_split_axis(s->mu0(), cfg, fill_derived) != 3) return false;
  return true;
}

// Can the stages of this simulation read same-rank neighbours directly (apk_stage_args.face_neighbor)
// so that the same-rank ghost copies can be skipped?  Every stage of the cycle must be one of the
// kernels that follow the table, and nothing else in the cycle may read ghost zones.  (do_stage skips
// the copies only after stages whose FillDerived was fused -- into the finishing sweep or, with the
// turbulence driver, into the kick; an exchange followed by a full-block ConsToPrim is a complete one.)
bool direct_neighbors(const apk_sim *s) {
  const HydroPackage &pkg = s->pkg;
  if (!s->direct_on || !s->d_face_nbr || s->amr || s->mesh.ndim != 3) return false;
  // first-order flux correction: every stage runs as the optimistic fused stage (do_stage) -- the same kernels with the
  // admissibility test in the finishing sweep; a stage that fails it is redone through the flux arrays, which read ghost
  // zones: do_stage fills them first (materialize_local_ghosts).  One-rank periodic boxes, no forcing.
  const bool optimistic = s->fused && pkg.first_order_flux_correct && !s->fmft && pkg.riemann != APK_RS_NONE && pkg.riemann != APK_RS_LLF &&
                          !pkg.flux_path_sources() && table_covers_all_faces(s);
  if (!stage_can_fuse(s) && !optimistic) return false;
  // (floors and ceilings: ConsToPrim is not fused into the ghost fills then, and the separate pass over the ghost zones
  // would convert the zones nobody filled -- unless no zone is left to fill at all.  What the stages read across a face
  // is the neighbour's floored interior state either way: the values the reference's ConsToPrim of a ghost cell produces
  // from the same conserved input.)
  if (scalars_or_extended_dedner(s) || (!ghost_c2p_fusable(s) && !table_covers_all_faces(s))) return false;
  return high_order_stages_are_two_kernel(s, 2);
}

// Refined meshes: may the stages read a same-rank neighbour of the SAME level through the face table (built in
// amr_rebuild) instead of the ghost zone behind that face?  Then the faces-only exchange of the stage loop skips
// those copies and their ConsToPrim (AMR_XCHG_DIRECT).  The stage forms that follow the table: the single-march
// donor-cell stage and the two-kernel stage (stage_form.hpp: plan_stage); refined-mesh stages run without FillDerived.
bool amr_direct(const apk_sim *s) {
  if (!s->direct_on || !s->amr || !s->d_face_nbr || s->mesh.ndim != 3 || !stage_can_fuse(s) || !amr_faces_only(s)) return false;
  return !scalars_or_extended_dedner(s) && high_order_stages_are_two_kernel(s, 0);
}

// does the cycle in progress end with a check of the refinement criteria?  Those read the full ring of ghost
// cells round a block -- edges and corners too (refinement/gradient.cpp:33-36 loops k, j, i over [s-1, e+1]
// and differences each of them) -- so the exchange after the last stage of such a cycle is a complete one, or at
// least two layers deep all round (amr_shell_before_check).
bool regrid_check_follows(const apk_sim *s) {
  return s->amr && s->amr_adaptive && s->amr_check_interval > 0 && (s->ncycle + 1) % s->amr_check_interval == 0;
}

// may the stage loop of a refined mesh skip the ghost zones behind edges and corners?  (apk_sim_set_amr_full_exchange(1):
// never)
bool amr_faces_only(const apk_sim *s) {
  return s->amr && !s->amr_full_exchange && s->mesh.ndim >= 2;
}

// Refined meshes, the exchange after the last stage of a cycle that ends with a refinement check (regrid_check_follows):
// may it fill the ghost zones AMR_SHELL_DEPTH layers deep only?  Tagging reads that far (refinement/gradient.cpp:33-36),
// and so must the first stage of the next cycle: a donor-cell stage (the VL2 predictor) reads one layer, PLM two.
// (Whoever needs more -- accessors, the data transfer of a regridding that does change the mesh -- calls sync_ghosts.)
bool amr_shell_before_check(const apk_sim *s) {
  const HydroPackage &pkg = s->pkg;
  if (!s->amr || !amr_faces_only(s) || !amr_has_shell(s) || !stage_can_fuse(s) || !pkg.calc_dt_hyp) return false;
  // the shell is AMR_SHELL_DEPTH layers deep: the first stage of the next cycle may read no deeper -- its stencil
  // half width plus the face it reconstructs for (DC 1 layer, PLM 2; PPM / WENO-Z 3 would read stale cells)
  const int recon = pkg.flux_first_stage.recon;
  const int reach = (recon == APK_RC_DC) ? 1 : ((recon == APK_RC_PPM || recon == APK_RC_WENOZ) ? 3 : 2);
  return reach <= AMR_SHELL_DEPTH && !(pkg.fluid == APK_FLUID_GLMMHD && pkg.glmmhd_source_extended && AMR_SHELL_DEPTH < 2);
}

// fill the ghost zones that direct neighbour addressing left stale: cons of buffer `buf` (default: the current state)
// and the stored primitives, which are that buffer's
int materialize_local_ghosts(apk_sim *s, int buf) {
  if (!s->local_ghosts_stale) return APK_OK;
  s->local_ghosts_stale = false;
  if (buf < 0) buf = s->cur;
  // (floors / ceilings: plain copies, then the pass over the ghost zones -- the order of a cycle without the table)
  const int mode = ghost_c2p_fusable(s) ? GHOST_C2P : GHOST_COPY;
  SIM_TRY(s, run_ghost_plan(s, buf, PH_LOCAL, mode));
  // (physical boundaries copy corner cells out of ghost zones the same-rank copies fill)
  for (int ph = PH_BC1; ph <= PH_BC3; ++ph) SIM_TRY(s, run_ghost_plan(s, buf, ph, mode));
  // (no stored primitives: the caller converts whole blocks, materialize_prim)
  if (mode == GHOST_COPY && !s->prim_stale)
    SIM_TRY(s, apk_cons_to_prim_ghosts(s->ctx, s->mu0_of[buf][s->pcur], s->pkg.fluid, &s->pkg.eos, s->stream));
  return APK_OK;
}

// Can stage 1 of a cycle take its input from the conserved state, so that the last stage of the cycle before it need
// not store primitives?  The single-march donor-cell stage in its lean form (uniform 3-D mesh, VL2), and a last stage
// that is the lean two-kernel stage with the time-step estimate fused in.
bool prim_free_cycle(const apk_sim *s) {
  const HydroPackage &pkg = s->pkg;
  if (!s->prim_free_on || s->amr || s->fmft || s->mesh.ndim != 3 || !stage_can_fuse(s)) return false;
  if (scalars_or_extended_dedner(s) || !pkg.calc_dt_hyp || !eos_is_lean(pkg.eos)) return false;
  if (pkg.flux_first_stage.recon != APK_RC_DC || pkg.flux_other_stage.recon == APK_RC_DC || s->nstages < 2) return false;
  return high_order_stages_are_two_kernel(s, 2);
}

// The same for integrators whose stages are all two-kernel stages (RK1 / RK2 / RK3 with PLM, PPM, WENO-Z ...): every
// stage derives its input from the conserved state (apk_stage_args.prim_from_cons: u1's in stages with gam0 = 0, u0's
// with an out-of-place result in the others -- a third buffer in rotation, as for the trial stages of first-order flux
// correction) and stores no primitives; the last one computes them for the time-step estimate (fill_derived = 3).
// apk_sim_set_prim_free(0) switches it off.
bool rk_prim_free_cycle(const apk_sim *s) {
  const HydroPackage &pkg = s->pkg;
  // (forced turbulence included: its kick after the last stage estimates the time step without storing primitives,
  // apk_turb_apply_dt)
  if (!s->prim_free_on || s->amr || s->mesh.ndim != 3 || !stage_can_fuse(s)) return false;
  if (scalars_or_extended_dedner(s) || !pkg.calc_dt_hyp) return false;
  const apk_eos &e = pkg.eos;
  if (!eos_is_lean(e)) return false;
  // Stages that are not the last store their result without ConsToPrim (fill_derived = 0): a density or internal-energy
  // floor would act on the register copy the next stage converts but never reach the stored conserved state, where the
  // reference's FillDerived after every stage writes the floored values back (adiabatic_hydro.hpp:81,129-136).  With
  // floors the cycle keeps its primitives (every stage fill_derived = 2).
  if (e.dfloor > 0.0 || e.efloor > 0.0) return false;
  if (pkg.flux_first_stage.recon == APK_RC_DC || pkg.flux_other_stage.recon == APK_RC_DC) return false;
  return high_order_stages_are_two_kernel(s, 0);
}

// Refined meshes, VL2 with a high-order corrector in the two-kernel form (BASELINE config 5): may the corrector derive
// its input from the half-step CONSERVED state (apk_stage_args.prim_from_cons = 2) -- so that no ConsToPrim pass runs
// between the two stages, 38 of 810 us per cycle on config 5's mesh -- and the flux correction's boundary planes likewise
// (apk_calculate_fluxes_boundary_list_from_cons)?  The corrector's result goes over the register u1, cell by cell the
// value the lane has just read, and the two buffers swap roles.  No floors or ceilings (the in-register ConsToPrim is
// the lean one and writes nothing back), no passive scalars, no forcing.  apk_sim_set_prim_free(0) switches it off.
bool amr_prim_free_cycle(const apk_sim *s) {
  const HydroPackage &pkg = s->pkg;
  if (!s->prim_free_on || !s->amr || s->fmft || s->mesh.ndim != 3 || !stage_can_fuse(s) || !amr_faces_only(s)) return false;
  const apk_eos &e = pkg.eos;
  if (scalars_or_extended_dedner(s) || !eos_is_lean(e) || e.dfloor > 0.0 || e.efloor > 0.0) return false;
  if (pkg.flux_first_stage.recon != APK_RC_DC || pkg.flux_other_stage.recon == APK_RC_DC || s->nstages != 2) return false;
  if (s->gam0[1] != 0.0) return false;  // (the corrector must not read the old u0: VL2)
  return high_order_stages_are_two_kernel(s, 0) && high_order_stages_are_two_kernel(s, 2);
}

// May the exchange at the end of a cycle deliver ONE layer of ghost cells (mesh.hpp PH_PACK_THIN)?  The first stage of the
// next cycle must be the single-march donor-cell stage (it reads one layer; the corrector's exchange stays a full one),
// nothing else in a cycle may read ghost zones (no forcing, no refinement), and the box must be periodic: a physical
// boundary phase copies corner cells out of ghost zones the messages fill.  Uniform 3-D meshes, exchanges left in
// flight (the path of N > 1 runs).  apk_sim_set_thin_exchange(0) switches it off.
bool thin_exchange_cycle(const apk_sim *s) {
  const HydroPackage &pkg = s->pkg;
  const Mesh &mm = s->mesh;
  if (!s->thin_on || s->amr || s->fmft || mm.ndim != 3 || mm.peers.empty() || !stage_can_fuse(s)) return false;
  if (mm.ng <= kThinDepth || scalars_or_extended_dedner(s)) return false;
  return pkg.flux_first_stage.recon == APK_RC_DC && s->nstages >= 2 && mm.AllPeriodic();
}

// May the x1 strips of this cycle's exchanges bypass the pack / unpack kernels (apk_stage_args.x1_halo)?  On a uniform
// periodic 3-D mesh with remote neighbours, in the leanest forms of a cycle:
//   1  VL2: the predictor reads the conserved state (prim_free_cycle) one layer deep (thin_exchange_cycle) and sends
//      primitives (GHOST_PRIM_COPY), the corrector reads those and sends one layer of the conserved state;
//   2  the RK integrators whose stages all derive their input from the conserved state (rk_prim_free_cycle) in the
//      two-kernel form: every exchange moves the conserved state nghost deep, and every finishing march stores its x1
//      strips into the messages and reads the ones of the stage before from them;
// both in stage forms that follow the table.  0: neither.  apk_sim_set_x1_direct(0) switches it off.
static int x1_kind_of(const apk_sim *s, bool direct, bool thin, bool prim_free, bool rk_free) {
  const HydroPackage &pkg = s->pkg;
  const Mesh &mm = s->mesh;
  if (!s->x1_on || !s->d_x1_tab[0] || mm.mb[0] < 2 * mm.ng || mm.peers.empty() || !mm.AllPeriodic()) return 0;
  if (!direct || !ghost_c2p_fusable(s)) return 0;
  const int ded = (pkg.fluid == APK_FLUID_GLMMHD) ? 1 : 0;
  if (s->nstages == 2 && thin && prim_free) {
    return (apk_stage_x1_halo(s->mu0(), &pkg.flux_first_stage, &pkg.eos, 2, ded, 1) == 1 &&
            apk_stage_x1_halo(s->mu0(), &pkg.flux_other_stage, &pkg.eos, 3, ded, 0) == 1) ? 1 : 0;
  }
  if (rk_free) {
    // (stage 1 reads u1's state, the others u0's with an out-of-place result; the last computes primitives for dt only)
    return (apk_stage_x1_halo(s->mu0(), &pkg.flux_first_stage, &pkg.eos, s->nstages == 1 ? 3 : 0, ded, 1) == 1 &&
            apk_stage_x1_halo(s->mu0(), &pkg.flux_other_stage, &pkg.eos, 0, ded, 2) == 1 &&
            apk_stage_x1_halo(s->mu0(), &pkg.flux_other_stage, &pkg.eos, 3, ded, 2) == 1) ? 2 : 0;
  }
  return 0;
}
int x1_direct_kind(const apk_sim *s) { return x1_kind_of(s, direct_neighbors(s), thin_exchange_cycle(s), prim_free_cycle(s), rk_prim_free_cycle(s)); }
bool x1_direct_cycle(const apk_sim *s) { return x1_direct_kind(s) != 0; }

// The predicates above for the cycle in progress, evaluated once per stage (CycleForm, sim_internal.hpp).  They read
// the configuration, the mesh, the switches (apk_sim_set_*), which device tables exist and -- through s->mu0() -- the
// pack geometry, which is the same for every buffer: nothing a stage writes.  The switches and a regridding may change
// the answer between two steps, so nothing is kept from one call of do_stage to the next.
static CycleForm cycle_form(const apk_sim *s) {
  CycleForm f;
  f.direct = direct_neighbors(s);
  f.amr_direct = amr_direct(s);
  f.prim_free = prim_free_cycle(s);
  f.rk_free = rk_prim_free_cycle(s);
  f.amr_pf = amr_prim_free_cycle(s);
  f.thin = thin_exchange_cycle(s);
  f.x1_kind = x1_kind_of(s, f.direct, f.thin, f.prim_free, f.rk_free);
  return f;
}

int materialize_prim(apk_sim *s) {
  if (!s->prim_stale) return APK_OK;
  s->prim_stale = false;
  return fill_derived(s);  // (every cell of every block: the ghost zones have been brought up to date by the caller)
}

// The last exchange was a one-layer one: repeat it in full (cons; and prim unless no primitives of this state are
// stored).  A collective over the ranks, like the completion of a refined mesh's ghost zones below: accessors that
// reach it are to be called on every rank.
int materialize_remote_ghosts(apk_sim *s) {
  if (!s->remote_ghosts_thin && !s->x1_in_recv) return APK_OK;  // (... or it left its x1 strips in the receive buffers)
  if (s->exchange_pending) return fail(s, APK_ERR_INVALID, "materialize_remote_ghosts: an exchange is in flight");
  if (!s->have_comm || !s->comm.exchange) return fail(s, APK_ERR_INVALID, "remote neighbours but no comm ops");
  // (the message half of exchange_begin / exchange_end: same-rank ghost zones are none of its business)
  const int mode = (!s->prim_stale && ghost_c2p_fusable(s)) ? GHOST_C2P : GHOST_COPY;
  select_thin_messages(s, false);
  s->xchg_thin = s->remote_ghosts_thin = false;
  s->xchg_x1_direct = s->x1_in_recv = s->x1_out_direct = false;
  SIM_TRY(s, apk_copy_plan_run(s->ctx, s->plan(PH_PACK), s->stream));
  if (s->comm.exchange(s->comm.user) != 0) return fail(s, APK_ERR_DEVICE, "halo exchange failed");
  SIM_TRY(s, run_ghost_plan(s, s->cur, PH_UNPACK, mode));
  for (int ph = PH_BC1; ph <= PH_BC3; ++ph) SIM_TRY(s, run_ghost_plan(s, s->cur, ph, mode));
  if (mode == GHOST_COPY && !s->prim_stale) SIM_TRY(s, apk_cons_to_prim_ghosts(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, s->stream));
  return APK_OK;
}

int sync_ghosts(apk_sim *s) {
  if (!s->amr && s->prim_stale) {
    SIM_TRY(s, finish_pending(s));
    SIM_TRY(s, materialize_remote_ghosts(s));
    SIM_TRY(s, materialize_local_ghosts(s));
    return materialize_prim(s);
  }
  if (s->amr) {
    if (s->amr_ghost_state == AMR_XCHG_FULL) return materialize_prim(s);  // (amr_prim_free_cycle may have left them stale)
    // the stage loop left the ghost zones behind edges and corners alone (or filled all of them a few layers deep):
    // complete exchange + ConsToPrim
    SIM_TRY(s, amr_exchange(s, s->cur, AMR_XCHG_FULL));
    s->prim_stale = false;
    return fill_derived(s);
  }
  SIM_TRY(s, finish_pending(s));
  SIM_TRY(s, materialize_remote_ghosts(s));
  return materialize_local_ghosts(s);
}

// is a stage with this flux configuration the two-kernel 3-D stage (its finishing march reads x1 neighbours from memory)?
static bool two_kernel_stage(const apk_sim *s, const apk_flux_cfg &cfg) {
  return s->mesh.ndim == 3 && cfg.recon != APK_RC_DC && apk_stage_split_axis(s->mu0(), &cfg, 2) == 3;
}

// can the exchange posted after a stage stay in flight while the stage `next` (1-based) starts?
bool can_overlap_next(const apk_sim *s, const CycleForm &f, int next) {
  const Mesh &m = s->mesh;
  // (messages to other ranks and / or same-rank copies on the copy stream)
  if (!(s->overlap && !s->amr && stage_can_fuse(s) && m.ndim >= 2 && s->x1win[0].d)) return false;
  if (!m.peers.empty() && !(s->have_comm && s->comm.exchange_begin && s->comm.exchange_end)) return false;
  if (m.peers.empty()) return false;
  const apk_flux_cfg &cfg = (next == 1) ? s->pkg.flux_first_stage : s->pkg.flux_other_stage;
  const bool ext_dedner = s->pkg.fluid == APK_FLUID_GLMMHD && s->pkg.glmmhd_source_extended;
  if (cfg.recon == APK_RC_DC) {
    // single-kernel donor-cell stage: 3-D, out-of-place FillDerived, no dt in the kernel
    return m.ndim == 3 && !ext_dedner && m.mb[0] >= 4 && m.mb[1] >= 4 && m.mb[2] >= 4 &&
           !(next == s->nstages && s->pkg.calc_dt_hyp) && !(s->fmft && next == s->nstages);
  }
  // A stage that runs as ONE march when left whole (hydro PLM in a prim-free RK cycle: 0.73 ms on 8 x 128^3 against 0.90
  // for the two kernels a split stage is made of) is left whole: the wire time the split could hide is 0.1 - 0.2 ms.
  if (f.rk_free && apk_stage_single_march(s->mu0(), &cfg)) return false;
  // x3 plane windows of the two-kernel schedule / x1 column windows of the three-sweep one
  return two_kernel_stage(s, cfg) ? m.mb[2] >= 4 * m.ng : m.mb[0] >= 4 * m.ng;
}

// complete an exchange left in flight (accessors, end of run): ghosts of cons and prim are valid after
int finish_pending(apk_sim *s) {
  if (!s->exchange_pending) return APK_OK;
  apk_pack *state = s->mu0_of[s->pending_cons][s->pcur];
  const int c2p = s->pending_c2p;
  SIM_TRY(s, exchange_end(s, c2p));
  if (c2p) return APK_OK;  // the ghost zones were converted as they were filled
  // (no primitives of this state are stored anywhere: whoever wants them runs materialize_prim over whole blocks)
  if (s->prim_stale) return APK_OK;
  return apk_cons_to_prim_ghosts(s->ctx, state, s->pkg.fluid, &s->pkg.eos, s->stream);
}

// turbulence::Driving = Generate + Perturb (src/pgen/turbulence.cpp:373-482), the first-order
// operator-split source run after the last stage (src/hydro/hydro_driver.cpp:559-560)
int turbulence_driving(apk_sim *s, double dt, bool fill, bool no_prim) {
  s->fmft->Evolve(dt);
  const auto &vh = s->fmft->var_hat();
  std::vector<double> flat(vh.size() * 2);
  for (size_t q = 0; q < vh.size(); ++q) {
    flat[2 * q] = vh[q].real();
    flat[2 * q + 1] = vh[q].imag();
  }
  SIM_TRY(s, apk_fmft_inverse(s->ctx, s->mu0(), s->fm_dev, flat.data(), s->stream));
  double sums[4];
  SIM_TRY(s, apk_turb_mean_momentum(s->ctx, s->mu0(), s->fm_dev, sums, s->stream));  // synchronises: flat is free
  const bool mpi = s->have_comm && s->nranks > 1;
  if (mpi && s->comm.allreduce_sum(s->comm.user, sums, 4) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  double ampl = 0.0;
  SIM_TRY(s, apk_turb_remove_mean(s->ctx, s->mu0(), s->fm_dev, sums, &ampl, s->stream));
  if (mpi && s->comm.allreduce_sum(s->comm.user, &ampl, 1) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  const double box = (s->xmax[0] - s->xmin[0]) * (s->xmax[1] - s->xmin[1]) * (s->xmax[2] - s->xmin[2]);
  const double norm = s->accel_rms / std::sqrt(ampl / box);
  // (fill: the kick also does FillDerived and the time-step estimate of the cells it touches -- the two tasks that
  // follow it, hydro_driver.cpp:559-577, 589-603 -- instead of a full ConsToPrim pass and a dt pass afterwards)
  // (no_prim: the stages of this cycle stored no primitives and the next one derives its input from the conserved state --
  // rk_prim_free_cycle --: the kick estimates the time step and leaves the primitives where they are, stale)
  if (fill && no_prim) {
    SIM_TRY(s, apk_turb_apply_dt(s->ctx, s->mu0(), s->fm_dev, norm, dt, s->pkg.fluid, &s->pkg.eos, s->stream));
    s->turb_dt_kicks += 1;
  }
  else if (fill) SIM_TRY(s, apk_turb_apply_fill(s->ctx, s->mu0(), s->fm_dev, norm, dt, s->pkg.fluid, &s->pkg.eos, s->pkg.calc_dt_hyp ? 1 : 0, s->stream));
  else SIM_TRY(s, apk_turb_apply(s->ctx, s->mu0(), s->fm_dev, norm, dt, s->stream));
  return APK_OK;
}


// ---- one stage of HydroDriver::MakeTaskCollection (hydro_driver.cpp:474-577) ----------------------------------------
// do_stage at the end of this file reads top to bottom; the steps it is made of follow in the order it takes them.

namespace {
// what a stage is given: its number, the flux configuration and the integrator's coefficients
struct Stage {
  int n;      // 1-based
  bool last;  // n == nstages
  apk_flux_cfg cfg;
  double g0, g1, beta_dt;
};

// What the fused stage of this call will be: decided in one place (plan_fused_stage), before anything is launched, and
// not changed after.
struct FusedStagePlan {
  int dedner;          // apk_stage_args.dedner: 0 / 1 / 2 (extended source)
  bool dc3;            // the single-march donor-cell stage (3-D)
  bool two_kernel;     // the two-kernel 3-D stage
  bool few_waves;      // a finishing march with too few waves to fill the GPU unless it is cut into segments
  bool fused_fill;     // the finishing sweep does FillDerived (and, in the last stage, the dt estimate)
  bool swap_prim;      // ... out of place: the two primitive buffers swap roles
  bool from_cons;      // the input is derived from the conserved state
  bool no_prim;        // no primitives are stored (fill_derived = 3: computed for the dt estimate only; 0: not at all)
  bool amr_fc;         // refined meshes: the corrector from the half-step conserved state, over u1 (amr_prim_free_cycle)
  int outbuf;          // the conserved buffer the result goes to: the current one unless the stage runs out of place
  int fill_derived, estimate_dt, prim_from_cons, cons_store;  // apk_stage_args
  bool ghost_cons_dead;  // the conserved values of this stage's result are read in no ghost zone
  bool x1_from_buffers;  // the exchange this stage follows left (or will leave) its x1 strips in the receive buffers
  bool x1_direct;        // the stage takes x1h (apk_stage_args.x1_halo)
  apk_x1_halo x1h;
};
}  // namespace

// The ghost-zone syncs the form of this stage demands, before anything is swapped or launched.  *from_cons: does the
// stage derive its input from the conserved state?  (Decided after the first sync and before the others: a later one
// that materialises the primitives does not take a prim-free stage form back.)
static int sync_for_stage_form(apk_sim *s, int stage, const CycleForm &f, bool *from_cons) {
  // (a stage form that reads ghost zones after stages that did not fill the same-rank ones)
  if (!f.direct && s->local_ghosts_stale) SIM_TRY(s, sync_ghosts(s));
  // (the full-step primitives were not stored: only the donor-cell predictor can do without them)
  // (refined meshes, amr_prim_free_cycle: both stages read the conserved state whether or not primitives are stored --
  // one set of kernels whatever happened between the cycles)
  *from_cons = f.amr_pf || (s->prim_stale && ((stage == 1 && f.prim_free) || f.rk_free));
  if (s->prim_stale && !*from_cons) SIM_TRY(s, sync_ghosts(s));
  if (f.amr_pf) s->amr_tag_vars_stored = s->amr_tags_posted = false;  // (the state they were taken from is about to be replaced)
  // (ghost zones one layer deep: enough for the donor-cell predictor they were left for, and for nothing else)
  if (s->remote_ghosts_thin && !(stage == 1 && f.thin)) SIM_TRY(s, sync_ghosts(s));
  // (... and their x1 strips still in the receive buffers: for a predictor that reads them there, x1_direct_cycle)
  if ((s->exchange_pending ? s->xchg_x1_direct : s->x1_in_recv) && f.x1_kind == 0) SIM_TRY(s, sync_ghosts(s));
  return APK_OK;
}

// "init u1" (hydro_driver.cpp:474-495) without the copy: the buffer holding u0 becomes the
// register u1 and the stage writes the new u0 into the other buffer.  Valid because
// gam0[0] == 0 for rk1/rk2/vl2/rk3, i.e. stage 1 never reads the old contents of its output.
static int swap_registers_for_stage_1(apk_sim *s) {
  if (s->gam0[0] != 0.0) {
    const size_t field_bytes = (size_t)s->nper * s->mesh.local_gids.size() * sizeof(double);
    SIM_HIP(s, hipMemcpyAsync(s->d_cons2[s->u1buf], s->d_cons2[s->cur], field_bytes, hipMemcpyDeviceToDevice, hs(s)));
  }
  const int was_u1 = s->u1buf;
  s->u1buf = s->cur;
  s->cur = was_u1;
  return APK_OK;
}

// the fields of apk_stage_args every fused stage sets, the trial stage of first-order flux correction included
static apk_stage_args stage_args_common(const apk_sim *s, const Stage &st, int dedner) {
  const HydroPackage &pkg = s->pkg;
  apk_stage_args a{};
  a.cfg = st.cfg;
  a.eos = pkg.eos;
  a.c_h = pkg.c_h;
  a.gam0 = st.g0;
  a.gam1 = st.g1;
  a.beta_dt = st.beta_dt;
  a.dedner = dedner;
  a.glmmhd_alpha = pkg.glmmhd_alpha;
  a.mindx = pkg.mindx;
  return a;
}

// refined meshes: the coarse-fine flux correction after a fused stage (amr_flux_fix), with the damping factor of psi the
// stage applied.  planes_ahead / cons_input: see amr_flux_fix.
static int amr_correct_after_stage(apk_sim *s, const Stage &st, int dedner, bool planes_ahead = false, int cons_input = -1) {
  if (!s->amr) return APK_OK;
  const HydroPackage &pkg = s->pkg;
  SIM_TRY(s, ensure_flux_arrays(s));
  const double psi_factor = dedner != 0 ? std::exp(-pkg.glmmhd_alpha * pkg.c_h * st.beta_dt / pkg.mindx) : 1.0;
  return amr_flux_fix(s, st.cfg, st.beta_dt, psi_factor, planes_ahead, cons_input);
}

// The plan of this stage.  No side effects beyond the buffers allocated on first use (ensure_spare_prim, ensure_trial_cons).
static int plan_fused_stage(apk_sim *s, const Stage &st, const CycleForm &f, bool from_cons, FusedStagePlan *out) {
  const HydroPackage &pkg = s->pkg;
  const Mesh &mm = s->mesh;
  const int stage = st.n;
  FusedStagePlan p{};
  p.from_cons = from_cons;
  p.dedner = (pkg.fluid == APK_FLUID_GLMMHD) ? (pkg.glmmhd_source_extended ? 2 : 1) : 0;
  // let the finishing sweep do FillDerived (and, in the last stage, the dt estimate) on the
  // cells it updates; only the ghost zones are converted after the exchange
  // (not when the turbulence driver kicks the state after this stage)
  // nor on refined meshes (the flux correction changes cells after the stage; the full pass after
  // the multilevel exchange converts everything)
  p.fused_fill = (mm.ndim >= 2) && !(s->fmft && st.last) && !s->amr;
  // A 3-D donor-cell stage (the VL2 predictor) runs as ONE march whose lanes read their
  // neighbours' primitives from memory, so it cannot replace prim in place: it writes the new
  // primitives into the spare buffer ("u1.prim") and the two prim buffers swap roles.
  p.dc3 = st.cfg.recon == APK_RC_DC && mm.ndim == 3;
  // waves of the finishing march if it cannot be cut into segments (an in-place ConsToPrim forbids
  // that): lanes along x1, one wave per transverse row (or 2 / 4 rows for narrow blocks)
  const int rpw_est = (mm.mb[0] <= 16) ? 4 : ((mm.mb[0] <= 32) ? 2 : 1);
  const int64_t final_waves = (int64_t)((mm.mb[0] + 64 / rpw_est - 1) / (64 / rpw_est)) *
                              ((mm.ndim == 3 ? mm.mb[1] : 1) + rpw_est - 1) / rpw_est * (int64_t)mm.local_gids.size();
  p.few_waves = mm.ndim >= 2 && final_waves < 2048;
  // (the two-kernel 3-D stage: its finishing march reads x1 neighbours from memory -- out of place)
  p.two_kernel = two_kernel_stage(s, st.cfg);
  if (p.fused_fill && (p.dc3 || p.dedner == 2 || p.few_waves || p.two_kernel)) {
    // (the extended Dedner source reads neighbouring primitives as well: out of place, too; and a
    // finishing march with too few waves to fill the GPU -- 2-D meshes, small packs -- runs out of
    // place so that it can be cut into segments)
    SIM_TRY(s, ensure_spare_prim(s));
    p.swap_prim = true;
  }
  p.fill_derived = p.fused_fill ? (p.swap_prim ? 2 : 1) : 0;
  p.estimate_dt = (p.fused_fill && st.last && pkg.calc_dt_hyp) ? 1 : 0;
  p.prim_from_cons = from_cons ? 1 : 0;
  // the last stage of a cycle whose successor's predictor reads the conserved state: primitives for the dt estimate only
  p.no_prim = (f.prim_free && st.last && p.two_kernel && p.swap_prim && p.estimate_dt) || (f.rk_free && p.two_kernel && p.fused_fill);
  if (p.no_prim) p.fill_derived = p.estimate_dt ? 3 : 0;  // (rk_free: stages that are not the last compute no primitives at all)
  p.outbuf = s->cur;
  if (f.rk_free && from_cons && st.g0 != 0.0) {
    // the input is the state this stage updates: its result goes to the free buffer, which becomes the current one
    SIM_TRY(s, ensure_trial_cons(s));
    p.outbuf = s->freebuf();
    p.prim_from_cons = 2;
  }
  // (refined meshes: the corrector from the half-step conserved state, over u1 -- amr_prim_free_cycle)
  p.amr_fc = f.amr_pf && stage == 2 && p.two_kernel && p.fill_derived == 0;
  if (f.amr_pf && stage == 2 && !p.amr_fc) return fail(s, APK_ERR_INVALID, "do_stage: the corrector of a refined mesh's prim-free cycle is not the two-kernel stage");
  if (p.amr_fc) {
    p.outbuf = s->u1buf;
    p.prim_from_cons = 2;
  }
  {
    // The predictor of VL2: the corrector has gam0 = 0 and takes its fluxes from the predictor's primitives, so the
    // half-step CONSERVED state is read by nobody but the ghost exchange -- the nghost-deep shell of every block --
    // and by nothing at all when every face is crossed through the face table (apk_stage_args.cons_store).
    const bool dead = p.dc3 && p.swap_prim && stage < s->nstages && s->gam0[stage] == 0.0 && !s->amr && !s->fmft && pkg.nscalars == 0;
    const bool all_periodic = mm.AllPeriodic();
    // (physical boundary phases copy conserved values out of ghost zones filled before them: periodic boxes only)
    // On a periodic box the exchange after this stage moves the stored primitives themselves (GHOST_PRIM_COPY in
    // post_stage_exchange; floors / ceilings keep the unfused order copy, then ConsToPrim of the ghost zones, which reads
    // the shell): then nothing reads any conserved value of this stage's result.
    if (dead) p.cons_store = (all_periodic && ((f.direct && mm.peers.empty()) || ghost_c2p_fusable(s))) ? 2 : 1;
    p.ghost_cons_dead = p.cons_store != 0 && all_periodic;
  }
  // x1 strips straight into / from the exchange buffers (x1_direct_cycle): the predictor sends its primitives nghost
  // deep and reads the one-layer conserved strips the corrector of the cycle before sent; the corrector the other way
  // round.  The receive side only when the exchange this stage follows left the strips in the buffers.
  // (Whether that exchange is still in flight or complete makes no difference: exchange_end hands xchg_x1_direct on to
  // x1_in_recv.)
  p.x1_from_buffers = s->exchange_pending ? s->xchg_x1_direct : s->x1_in_recv;
  if (f.x1_kind == 1) {
    const bool predictor = stage == 1 && p.dc3 && p.swap_prim && p.ghost_cons_dead && p.cons_store == 2;
    const bool corrector = st.last && stage > 1 && p.two_kernel && p.no_prim;
    if (predictor || corrector) {
      p.x1h.blocks = static_cast<const apk_x1_halo_block *>(s->d_x1_tab[predictor ? 0 : 1]);
      p.x1h.recv_depth = p.x1_from_buffers ? (predictor ? kThinDepth : mm.ng) : 0;
      p.x1h.send_depth = predictor ? mm.ng : kThinDepth;
      p.x1h.send_field = predictor ? 1 : 0;
      p.x1_direct = true;
    }
  } else if (f.x1_kind == 2 && p.two_kernel && f.rk_free && from_cons && (p.fill_derived == 0 || p.fill_derived == 3)) {
    // (an RK stage from the conserved state: the full messages both ways, the conserved state nghost deep)
    p.x1h.blocks = static_cast<const apk_x1_halo_block *>(s->d_x1_tab[2]);
    p.x1h.recv_depth = p.x1_from_buffers ? mm.ng : 0;
    // (forced turbulence: the kick after the last stage changes the state the strips were taken from -- that exchange
    // packs its x1 faces again)
    p.x1h.send_depth = (s->fmft && st.last) ? 0 : mm.ng;
    p.x1h.send_field = 0;
    p.x1_direct = p.x1h.recv_depth > 0 || p.x1h.send_depth > 0;
  }
  if (p.x1_from_buffers && !(p.x1_direct && p.x1h.recv_depth > 0))
    return fail(s, APK_ERR_INVALID, "do_stage: x1 ghost columns were left in the receive buffers for a stage that does not read them there");
  *out = p;
  return APK_OK;
}

// The previous stage's halo messages are still in flight.  Ghost zones filled by same-rank
// copies are ready: convert them, run whatever does not touch a late face (the x1 sweep of
// a high-order stage / the x3 sweep of the two-kernel stage, on index windows), then
// complete the exchange and do the thin slabs next to those faces; the caller launches the rest (phase 2).
static int run_overlapped_phase_1(apk_sim *s, const FusedStagePlan &p, apk_stage_args *a) {
  const HydroPackage &pkg = s->pkg;
  apk_pack *state = s->mu0_of[s->pending_cons][s->pcur];  // (stage 1 has swapped the cons roles already)
  const int c2p_in_copy = s->pending_c2p;  // then the ghost zones are converted as they are filled
  const bool convert_ghosts = !c2p_in_copy && !s->prim_stale;  // (stale: the predictor reads the conserved state)
  if (convert_ghosts)
    SIM_TRY(s, apk_cons_to_prim_ghosts_split(s->ctx, state, pkg.fluid, &pkg.eos, s->d_late_regions, 1, s->stream));
  // x3 plane windows of the two-kernel stage / x1 column windows of the three-sweep schedule (apk_stage_split_axis of
  // this stage's fill_derived: a two-kernel stage never fills in place).  A donor-cell stage does not get here.
  const apk_sim::WindowTable *tabs = p.two_kernel ? s->k3win : s->x1win;
  a->phase = 1;
  for (int q = 0; q < 3; ++q) {
    if (q == 1) {
      SIM_TRY(s, exchange_end(s, c2p_in_copy));
      if (convert_ghosts)
        SIM_TRY(s, apk_cons_to_prim_ghosts_split(s->ctx, state, pkg.fluid, &pkg.eos, s->d_late_regions, 2, s->stream));
    }
    if (!tabs[q].any) continue;
    a->window = tabs[q].d;
    a->window_rl = tabs[q].rl;
    a->window_rows = tabs[q].rows;
    SIM_TRY(s, apk_stage_fused(s->ctx, s->mu0(), s->mu1(), a, s->stream));
  }
  a->phase = 2;
  a->window = nullptr;
  a->window_rl = a->window_rows = 0;
  s->overlapped += 1;
  return APK_OK;
}

// the fused stage: finish or overlap the exchange in flight, launch, and book what the stage left where
static int run_fused_stage(apk_sim *s, const Stage &st, const CycleForm &f, const FusedStagePlan &p) {
  apk_stage_args a = stage_args_common(s, st, p.dedner);
  a.face_neighbor = (f.direct || f.amr_direct) ? s->d_face_nbr : nullptr;
  a.fill_derived = p.fill_derived;
  a.estimate_dt = p.estimate_dt;
  a.prim_from_cons = p.prim_from_cons;
  a.cons_out_delta = s->d_cons2[p.outbuf] - s->d_cons2[s->cur];
  a.cons_store = p.cons_store;
  if (p.x1_direct) a.x1_halo = &p.x1h;
  // An exchange in flight is always completed before a donor-cell stage, whichever form it takes.  The single-march
  // one (dc3 && swap_prim) split into windows (one main window + six slabs) runs one row per lane and
  // seven launches; whole, it runs two rows per lane (3.5 Riemann problems per cell instead of 4).  The one-GPU
  // rehearsal of an 8-GPU rank (bench.py) measures the split at +0.3 ms per cycle against 0.19 ms of wire time it
  // could hide: the exchange in flight at the start of a cycle is completed before the predictor instead
  // (round 3 split it: measured slower).  The other donor-cell forms have no windowed phase 1 at all.
  if (s->exchange_pending && st.cfg.recon == APK_RC_DC) SIM_TRY(s, finish_pending(s));
  if (s->exchange_pending) SIM_TRY(s, run_overlapped_phase_1(s, p, &a));
  // (refined meshes: the flux correction's boundary-plane fluxes beside the stage -- the stage stores no primitives there)
  // (amr_pf: the planes from the conserved state the stage reads -- u1's buffer in stage 1, the current one in stage 2)
  const int amr_cons_input = f.amr_pf ? (st.n == 1 ? s->u1buf : s->cur) : -1;
  bool planes_ahead = false;
  if (s->amr && a.fill_derived == 0) {
    SIM_TRY(s, ensure_flux_arrays(s));
    planes_ahead = amr_flux_planes_ahead(s, st.cfg, amr_cons_input);
  }
  {
    const int rc_stage = apk_stage_fused(s->ctx, s->mu0(), s->mu1(), &a, s->stream);
    // (the boundary-plane fluxes forked onto the side stream are joined on the error path too)
    if (rc_stage != APK_OK && planes_ahead) (void)hipStreamWaitEvent(hs(s), reinterpret_cast<hipEvent_t>(s->ev_join), 0);
    SIM_TRY(s, rc_stage);
  }
  s->stage_dt_pending = a.estimate_dt != 0;
  s->x1_in_recv = false;                                  // (read; the exchange below starts afresh)
  s->x1_out_direct = p.x1_direct && p.x1h.send_depth > 0;  // (consumed by exchange_begin)
  // (a stage that stored primitives -- the predictor's half-step ones -- makes the current buffer valid again; one that
  // stored none leaves them stale: the stages of a prim-free RK cycle, and its last stage under the turbulence driver,
  // whose kick then estimates the time step without storing them either)
  if (p.no_prim) s->prim_stale = true;
  else if (a.fill_derived == 1 || a.fill_derived == 2) {
    s->prim_stale = false;
    if (p.swap_prim) s->pcur = 1 - s->pcur;
  }
  const int inbuf = s->cur;
  s->cur = p.outbuf;                 // (its ghost zones are filled by the exchange below)
  if (p.amr_fc) s->u1buf = inbuf;  // (the half-step state: scratch from here on)
  // (boundary planes not computed beside the stage: from the state the stage read -- now the register's buffer)
  return amr_correct_after_stage(s, st, a.dedner, planes_ahead, amr_cons_input);
}

// first_order_flux_correct and a stage that does not read the old u0 (gam0 = 0: every VL2 stage,
// the first stage of the others): run the fused stage optimistically -- it leaves its inputs
// (prim, u1) intact -- and test the new state the way FirstOrderFluxCorrect tests its trial
// update.  No cell fails (the rule, away from strong shocks): done, with the result the
// flux-array sequence would have produced bit for bit.  Otherwise that sequence runs after all.
// The optimistic stage also does FillDerived (out of place: the old primitives are the fallback's
// input) and, in the last stage, the dt estimate, exactly like a stage without flux correction.
// (Refined meshes: the test sees the update before the coarse-fine flux correction, as
// FirstOrderFluxCorrect does in the reference's task order; the correction follows, and ConsToPrim
// stays the full pass after the exchange.)
// A stage that does read the old u0 (gam0 != 0: the later stages of RK2 / RK3) writes its trial
// result into a third buffer instead, so that u0 survives a rejected trial; an accepted one makes
// that buffer the current state.  (Not with passive scalars: their kernel updates in place; not on
// refined meshes: the flux correction after the stage addresses the current buffer.)
// (With the face table, so does a later stage that does not read it -- VL2's corrector: a rejected trial is redone
// through the flux arrays, whose sweeps read ghost primitives the table-following stages left stale, and those are
// regenerated from the conserved state they belong to -- which an in-place trial would have overwritten.)
// *accepted: the trial ran and stands (false: run_flux_array_stage does the stage); *filled: ... and did FillDerived.
static int run_trial_stage(apk_sim *s, const Stage &st, const CycleForm &f, bool *accepted, bool *filled) {
  const HydroPackage &pkg = s->pkg;
  *accepted = *filled = false;
  if (!(s->fused && pkg.first_order_flux_correct && (st.g0 == 0.0 || (pkg.nscalars == 0 && !s->amr)) &&
        !pkg.glmmhd_source_extended && s->mesh.ndim >= 2 && pkg.riemann != APK_RS_NONE && pkg.riemann != APK_RS_LLF &&
        !pkg.flux_path_sources()))
    return APK_OK;
  const bool trial_out_of_place = st.g0 != 0.0 || (f.direct && st.n > 1);
  if (trial_out_of_place) SIM_TRY(s, ensure_trial_cons(s));
  // FirstOrderFluxCorrect tests the UNfloored trial update (hydro.cpp:1283-1306; floors only act
  // in the ConsToPrim that follows the stage)
  // (the finishing sweep tests the update it holds in registers, before its own ConsToPrim floors
  // it; with passive scalars the stored state is tested after the stage, so nothing may floor it)
  const bool test_in_kernel = pkg.nscalars == 0;
  const bool fill = !(s->fmft && st.last) && !s->amr && (test_in_kernel || ghost_c2p_fusable(s));
  if (fill) SIM_TRY(s, ensure_spare_prim(s));
  // (plain Dedner source: the extended one does not get here)
  apk_stage_args a = stage_args_common(s, st, (pkg.fluid == APK_FLUID_GLMMHD) ? 1 : 0);
  a.fill_derived = fill ? 2 : 0;
  a.estimate_dt = (fill && st.last && pkg.calc_dt_hyp) ? 1 : 0;
  a.face_neighbor = f.direct ? s->d_face_nbr : nullptr;
  a.trial = 1;  // its ConsToPrim latches flags into the trial word: kept or dropped below
  // the finishing sweep applies FirstOrderFluxCorrect's test to the update it has in registers
  // (passive scalars ride a separate kernel: there the stored state is tested afterwards)
  a.count_unphysical = test_in_kernel ? 1 : 0;
  const int outbuf = trial_out_of_place ? s->freebuf() : s->cur;
  a.cons_out_delta = s->d_cons2[outbuf] - s->d_cons2[s->cur];
  SIM_TRY(s, apk_stage_fused(s->ctx, s->mu0(), s->mu1(), &a, s->stream));
  long long bad = 0;
  if (a.count_unphysical) SIM_TRY(s, apk_stage_unphysical_read(s->ctx, &bad, s->stream));
  else SIM_TRY(s, apk_count_unphysical(s->ctx, s->mu0(), pkg.fluid, &bad, s->stream));
  *accepted = bad == 0;
  if (fill) SIM_TRY(s, apk_trial_flags(s->ctx, *accepted ? 1 : 0, s->stream));
  if (!*accepted) {
    s->fofc_fallback_stages += 1;
    return APK_OK;
  }
  s->cur = outbuf;  // (its ghost zones are filled by the exchange below)
  if (fill) {
    s->pcur = 1 - s->pcur;
    *filled = true;
  }
  s->stage_dt_pending = a.estimate_dt != 0;
  return amr_correct_after_stage(s, st, a.dedner);
}

// the reference's task sequence through the flux arrays: the stage form of runs with unsplit sources or without a fused
// kernel for their solver, and the fallback of a rejected trial
static int run_flux_array_stage(apk_sim *s, const Stage &st) {
  const HydroPackage &pkg = s->pkg;
  // (the flux arrays' sweeps and FirstOrderFluxCorrect read the primitives of ghost cells: after stages that followed
  // the face table those are stale -- fill them, from the conserved buffer the stored primitives belong to: the
  // register u1 in stage 1, whose buffers have swapped roles above, the current state otherwise)
  if (s->local_ghosts_stale) SIM_TRY(s, materialize_local_ghosts(s, st.n == 1 ? s->u1buf : s->cur));
  SIM_TRY(s, ensure_flux_arrays(s));
  // (faces of interior cells only: nothing downstream reads the reference's extra transverse rows)
  SIM_TRY(s, apk_calculate_fluxes_tight(s->ctx, s->mu0(), st.cfg, &pkg.eos, pkg.c_h, s->stream));
  // the diffusive fluxes are added at the end of CalculateFluxes (hydro.cpp:1202-1205): FOFC's LLF fluxes, where it
  // corrects a cell, replace whole face fluxes after that
  if (pkg.diffusion_in_fluxes()) SIM_TRY(s, apk_calc_diff_fluxes_v2(s->ctx, s->mu0(), &pkg.diff, pkg.spitzer_cfg(), s->stream));
  if (pkg.first_order_flux_correct) {
    long long nfix = 0;
    SIM_TRY(s, apk_first_order_flux_correct(s->ctx, s->mu0(), s->mu1(), pkg.fluid, &pkg.eos, pkg.c_h, st.g0, st.g1,
                                            st.beta_dt, &nfix, s->stream));
    s->fofc_total += nfix;
  }
  if (s->amr) SIM_TRY(s, amr_flux_correction(s));
  SIM_TRY(s, apk_update_with_flux_divergence(s->ctx, s->mu0(), s->mu1(), st.g0, st.g1, st.beta_dt, s->stream));
  if (pkg.fluid == APK_FLUID_GLMMHD) {
    SIM_TRY(s, apk_dedner_source(s->ctx, s->mu0(), pkg.glmmhd_source_extended ? 1 : 0, pkg.glmmhd_alpha,
                                 pkg.c_h, pkg.mindx, st.beta_dt, s->stream));
  }
  // the other unsplit source (AddUnsplitSources, hydro.cpp:227-246): after the update and the Dedner source, before
  // the exchange and ConsToPrim of the stage (and before the turbulence kick of the last stage)
  if (pkg.cooling) SIM_TRY(s, apk_tabular_cooling_src(s->ctx, s->mu0(), s->cool_tab, pkg.fluid, st.beta_dt, s->stream));
  // ProblemSourceUnsplit comes last (hydro.cpp:241-243): the cluster's static gravity (cluster.cpp:63-74), with the
  // density and velocity of the stage's input -- the primitives this pack still holds
  if (pkg.gravity_srcterm)
    SIM_TRY(s, apk_gravity_src(s->ctx, s->mu0(), &s->cluster.gravity, s->d_block_xmin, st.beta_dt, s->stream));
  // ... then AGN feedback with the tower's power-scaled field, then the tower's fixed field rate (cluster.cpp:76-80)
  if (pkg.feedback_srcterm) SIM_TRY(s, cluster_feedback_sources(s, st.beta_dt));
  // ... then SNIa feedback (cluster.cpp:82-83)
  if (pkg.snia_srcterm) SIM_TRY(s, cluster_snia_source(s, st.beta_dt));
  // the first-order split sources after the unsplit ones of the last stage, with the full dt and the primitives the pack
  // then holds (hydro_driver.cpp:548-560): stellar feedback, then the clips (cluster.cpp:85-93)
  if (st.last && pkg.cluster_split_srcterm) SIM_TRY(s, cluster_split_sources(s, s->dt));
  return APK_OK;
}

// the forcing kick after the last stage (turbulence_driving).  *fused_fill: the stage did FillDerived -- or, on return,
// the kick did
static int forcing_kick(apk_sim *s, const CycleForm &f, bool *fused_fill) {
  const bool kick_fills = !*fused_fill && !s->amr;
  // (a cycle whose stages store no primitives: the kick leaves them stale too, the next stage 1 reads the conserved state)
  const bool kick_no_prim = kick_fills && s->prim_stale && f.rk_free;
  SIM_TRY(s, turbulence_driving(s, s->dt, kick_fills, kick_no_prim));
  if (kick_fills && !kick_no_prim) s->prim_stale = false;  // (the kick wrote the primitives of every cell it touched)
  if (kick_fills) {  // as after a stage whose finishing sweep did FillDerived and the dt estimate
    *fused_fill = true;
    s->stage_dt_pending = s->pkg.calc_dt_hyp;
  }
  return APK_OK;
}

// refined meshes: nothing in the stage loop reads a ghost cell behind an edge or a corner of a block -- the
// exchange skips those boxes (37 % of the ghost cells of a 16^3 block with nghost = 4) and ConsToPrim the cells
// (nor, with amr_direct, the ghost zones behind faces the stages cross by the face table)
static int amr_faces_exchange(apk_sim *s, const Stage &st, const CycleForm &f) {
  const HydroPackage &pkg = s->pkg;
  const bool dir = f.amr_direct;
  SIM_TRY(s, amr_exchange(s, s->cur, dir ? AMR_XCHG_DIRECT : AMR_XCHG_FACES));
  if (dir) s->skipped_local_exchanges += 1;
  if (st.last && pkg.calc_dt_hyp && f.amr_pf) {
    // (the next predictor reads the conserved state: the estimate alone, no primitive stored)
    SIM_TRY(s, apk_cons_to_prim_dt_select(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, 0, nullptr, 0u, s->stream));
    s->stage_dt_pending = true;
    s->prim_stale = true;
    s->amr_c2p_passes_skipped += 1;
  } else if (st.last && pkg.calc_dt_hyp) {  // (the time-step estimate on the way, as in post_stage_exchange)
    SIM_TRY(s, apk_cons_to_prim_faces_dt(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, dir ? s->d_face_nbr : nullptr, s->stream));
    s->stage_dt_pending = true;
  } else if (st.n == 1 && f.amr_pf) {
    // (the corrector converts what it loads: no pass over the blocks here)
    s->amr_c2p_passes_skipped += 1;
  } else if (dir) {
    SIM_TRY(s, apk_cons_to_prim_faces_skip(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, s->d_face_nbr, s->stream));
  } else {
    SIM_TRY(s, apk_cons_to_prim_faces(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, s->stream));
  }
  return APK_OK;
}

// refined meshes, the last exchange of a cycle that ends with a refinement check: every ghost zone, but only as deep as the tagging
// criteria and the first stage of the next cycle read; ConsToPrim of that shell with the time-step estimate
// (with the face table: nor the zones behind same-level same-rank faces, 59 % of the shell's cells -- the tag kernel,
// ConsToPrim and the next cycle's predictor all follow the table there)
// (periodic boxes only: a physical-boundary phase copies the edge cells next to the boundary out of ghost zones
// filled before it, and the tagging criteria read those edges)
static int amr_shell_exchange(apk_sim *s, const CycleForm &f) {
  const HydroPackage &pkg = s->pkg;
  const bool dir = f.amr_direct && s->mesh.AllPeriodic();
  SIM_TRY(s, amr_exchange(s, s->cur, dir ? AMR_XCHG_SHELL_DIRECT : AMR_XCHG_SHELL));
  if (dir) s->skipped_local_exchanges += 1;
  int crit = -1;
  double crit_p0 = 0.0, crit_p1 = 0.0;
  if (f.amr_pf && pkg.calc_dt_hyp) SIM_TRY(s, refinement_criterion(s, &crit, &crit_p0, &crit_p1));
  bool tags_done = false;
  if (crit == APK_TAG_PRESSURE_GRADIENT && s->mesh.ndim == 3) {
    // (... and for the pressure gradient not even that: the criterion is reduced in the same pass, its pressures in LDS)
    int pending = 0;
    const int rc_tag = apk_tag_blocks_dt_from_cons(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, dir ? s->d_face_nbr : nullptr, &pending, s->stream);
    if (rc_tag == APK_OK) {
      tags_done = true;
      s->amr_tags_posted = true;
      s->amr_posted_criterion = crit, s->amr_posted_pending = pending, s->amr_posted_p0 = crit_p0, s->amr_posted_p1 = crit_p1;
      s->prim_stale = true;
      s->amr_tag_vars_stored = false;
      s->amr_c2p_passes_skipped += 1;
    } else if (rc_tag != APK_ERR_UNSUPPORTED) {  // (blocks too wide for the pressure tile: the two passes below)
      return fail(s, rc_tag, std::string("apk_tag_blocks_dt_from_cons: ") + apk_last_error(s->ctx));
    }
  }
  if (tags_done) {
  } else if (crit >= 0) {
    // (the next predictor reads the conserved state: of the primitives only what the refinement criterion reads)
    // (the reference's order of the primitives: IDN = 0, IV1 .. IV3 = 1 .. 3, IPR = 4)
    const unsigned vars = crit == APK_TAG_PRESSURE_GRADIENT ? (1u << 4) : (crit == APK_TAG_VELOCITY_GRADIENT ? ((1u << 1) | (1u << 2)) : (1u << 0));
    SIM_TRY(s, apk_cons_to_prim_dt_select(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, AMR_SHELL_DEPTH, dir ? s->d_face_nbr : nullptr, vars, s->stream));
    s->prim_stale = true;
    s->amr_tag_vars_stored = true;
    s->amr_c2p_passes_skipped += 1;
  } else {
    SIM_TRY(s, apk_cons_to_prim_dt_skip(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, AMR_SHELL_DEPTH, dir ? s->d_face_nbr : nullptr, s->stream));
  }
  s->stage_dt_pending = true;
  return APK_OK;
}

// the ghost exchange after a stage and what is left of FillDerived (and of the time-step estimate) after it
static int post_stage_exchange(apk_sim *s, const Stage &st, const CycleForm &f, bool fused_fill, bool ghost_cons_dead) {
  const HydroPackage &pkg = s->pkg;
  // (a last stage that stored no primitives: the ghost zones get none either -- the next predictor reads the conserved
  // state there as everywhere)
  const bool ghost_prims = !s->prim_stale;
  const int c2p_in_copy = !(fused_fill && ghost_c2p_fusable(s) && ghost_prims)
                              ? GHOST_COPY
                              : (ghost_cons_dead ? GHOST_PRIM_COPY : GHOST_C2P);
  if (fused_fill && can_overlap_next(s, f, st.last ? 1 : st.n + 1)) {
    // post the messages and leave them in flight: the next stage (of this or of the next cycle)
    // completes the exchange
    return exchange_begin(s, true, c2p_in_copy, f.direct, st.last && f.thin);
  }
  if (s->amr && amr_faces_only(s) && !(st.last && regrid_check_follows(s))) return amr_faces_exchange(s, st, f);
  if (s->amr && st.last && amr_shell_before_check(s)) return amr_shell_exchange(s, f);
  // (without a fused FillDerived the full-block ConsToPrim below reads every ghost zone)
  SIM_TRY(s, exchange_ghosts(s, c2p_in_copy, f.direct && fused_fill, fused_fill && st.last && f.thin));
  if (fused_fill) {
    // (not after an exchange that filled nothing: direct addressing on a mesh whose faces the table covers)
    const bool filled_none = f.direct && table_covers_all_faces(s);
    if (!c2p_in_copy && ghost_prims && !filled_none) SIM_TRY(s, apk_cons_to_prim_ghosts(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, s->stream));
  } else if (st.last && pkg.calc_dt_hyp && !pkg.diffusion_sts()) {
    // (not with rkl2: the second super-time-step changes the state before the estimate)
    // the last FillDerived of the cycle and the time-step estimate that follows it (hydro_driver.cpp:571-603) in
    // one pass: the interior cells' primitives are in registers anyway (refined meshes, flux-array stages)
    SIM_TRY(s, apk_cons_to_prim_dt(s->ctx, s->mu0(), pkg.fluid, &pkg.eos, -1, s->stream));
    s->stage_dt_pending = true;
    s->prim_stale = false;  // (every cell of every block)
  } else {
    SIM_TRY(s, fill_derived(s));
    s->prim_stale = false;
  }
  return APK_OK;
}

int do_stage(apk_sim *s, int stage) {
  HydroPackage &pkg = s->pkg;
  const CycleForm form = cycle_form(s);
  bool from_cons = false;
  SIM_TRY(s, sync_for_stage_form(s, stage, form, &from_cons));
  if (stage == 1) SIM_TRY(s, swap_registers_for_stage_1(s));
  const Stage st{stage, stage == s->nstages, (stage == 1) ? pkg.flux_first_stage : pkg.flux_other_stage,
                 s->gam0[stage - 1], s->gam1[stage - 1], s->beta[stage - 1] * s->dt};
  s->stage_dt_pending = false;
  // an exchange left in flight is completed inside the fused stage below; anything else first
  if (s->exchange_pending && !can_overlap_next(s, form, stage)) SIM_TRY(s, finish_pending(s));
  bool fused_fill = false;       // FillDerived of the cells the stage updated is done (by its finishing sweep, or by the kick)
  bool ghost_cons_dead = false;  // the conserved values of this stage's result are read in no ghost zone
  if (stage_can_fuse(s)) {
    FusedStagePlan plan;
    SIM_TRY(s, plan_fused_stage(s, st, form, from_cons, &plan));
    SIM_TRY(s, run_fused_stage(s, st, form, plan));
    fused_fill = plan.fused_fill;
    ghost_cons_dead = plan.ghost_cons_dead;
  } else {
    bool accepted = false;
    SIM_TRY(s, run_trial_stage(s, st, form, &accepted, &fused_fill));
    if (!accepted) SIM_TRY(s, run_flux_array_stage(s, st));
  }
  if (s->fmft && st.last) SIM_TRY(s, forcing_kick(s, form, &fused_fill));
  SIM_TRY(s, post_stage_exchange(s, st, form, fused_fill, ghost_cons_dead));
  if (st.last && pkg.calc_c_h) {  // hydro_driver.cpp:589-603
    pkg.mindx = kHuge;
    pkg.dt_hyp = kHuge;
    s->dt_hyp_is_global = false;
  }
  return APK_OK;
}

}  // namespace host
}  // namespace apk
