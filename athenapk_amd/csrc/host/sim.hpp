// sim.hpp -- standalone host driver above the hot-path boundary: the "Hydro" package
// options (src/hydro/hydro.cpp:264-826), the per-cycle c_h update (hydro.cpp:102-143), the
// per-stage task order (src/hydro/hydro_driver.cpp:347-673) and Parthenon's dt control
// (SURVEY.md App. A.2-A.4).  All compute goes through the C-ABI of include/apk_amd.h.
#pragma once

#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/apk_amd.h"
#include "../../../include/apk_host.h"
#include "../cooling_table.hpp"
#include "amr.hpp"
#include "amr_forms.hpp"
#include "feedback.hpp"
#include "mesh.hpp"
#include "params.hpp"
#include "turbulence.hpp"

namespace apk {

// Units (src/units.hpp) and the gas composition (hydro.cpp:482-503)
struct UnitsState {
  bool has_units = false, has_composition = false;
  double code_length_cgs = 1, code_mass_cgs = 1, code_time_cgs = 1;
  double He_mass_fraction = 0, mu = 0, mu_e = 0, mbar = 0, mbar_over_kb = 0;
  double code_energy_cgs() const;
  // constants and scales in code units
  double k_boltzmann() const, mh() const, atomic_mass_unit() const, erg() const, cm() const, s() const;
  // (what the cluster problem converts its defaults with, host/cluster.cpp)
  double gravitational_constant() const, msun() const, kpc() const, mpc() const, km_s() const, kev() const, g() const;
  double speed_of_light() const;
};

// "Hydro" StateDescriptor params (names as in hydro.cpp)
struct HydroPackage {
  int fluid = APK_FLUID_EULER;
  int recon = APK_RC_UNDEFINED;
  int riemann = APK_RS_UNDEFINED;
  int integrator = APK_INT_UNDEFINED;
  int nhydro = 5, nscalars = 0;
  double cfl = 0.3;
  apk_eos eos{};
  bool glmmhd_source_extended = false;  // hydro/glmmhd_source
  double glmmhd_alpha = 0.1;
  bool calc_c_h = false, calc_dt_hyp = true;
  bool first_order_flux_correct = false;
  double max_dt = -1.0;
  // mutable params
  double c_h = 0.0;
  double mindx = std::numeric_limits<double>::max();
  double dt_hyp = std::numeric_limits<double>::max();
  // flux function keys (FluxFunKey_t) of the first and the other stages (hydro.cpp:449-467)
  apk_flux_cfg flux_first_stage{}, flux_other_stage{};
  // <diffusion> (hydro.cpp:538-702): the processes, diffint and cfl_diff
  apk_diff_cfg diff{};
  // conduction_coeff = spitzer (hydro.cpp:567-593): what ThermalDiffusivity::Get needs, next to `diff`; all 0 otherwise
  apk_spitzer_cfg spitzer{};
  const apk_spitzer_cfg *spitzer_cfg() const {
    return (diff.conduction != APK_COND_NONE && diff.conduction_coeff == APK_CONDC_SPITZER) ? &spitzer : nullptr;
  }
  int diffint = APK_DIFFINT_NONE;
  double cfl_diff = 0.0;
  // diffusion/rkl2_max_dt_ratio (hydro.cpp:686-689); rkl2 is accepted only with a positive ratio
  double rkl2_max_dt_ratio = -1.0;
  // the diffusive limit, minimum over all ranks, as estimated last (the "dt_diff" param, hydro.cpp:700-701, 961-962):
  // what both RKL2 half steps of the next cycle size their stage count with
  double dt_diff = std::numeric_limits<double>::max();
  bool diffusion_processes() const {
    return diff.conduction != APK_COND_NONE || diff.viscosity != APK_VISC_NONE || diff.resistivity != APK_RES_NONE;
  }
  // a process and an integrator are configured (with integrator = none the processes do nothing, as in the reference):
  // the diffusive time-step estimate, and stages on the flux-array path
  bool diffusion_configured() const { return diffint != APK_DIFFINT_NONE && diffusion_processes(); }
  // the diffusive fluxes are added at the end of CalculateFluxes (hydro.cpp:1202-1205): unsplit only -- with rkl2 the
  // hyperbolic stages carry none
  bool diffusion_in_fluxes() const { return diffint == APK_DIFFINT_UNSPLIT && diffusion_processes(); }
  // operator-split super-time-stepping around the hyperbolic stages (hydro_driver.cpp:455-458, 581-583)
  bool diffusion_sts() const { return diffint == APK_DIFFINT_RKL2 && diffusion_processes(); }
  UnitsState units;
  // <cooling> enable_cooling = tabular (hydro.cpp:723-738): the parameters, the table as parsed and its fingerprint
  bool cooling = false;
  apk_cooling_params cool{};
  CoolingTableHost cool_table;
  double cool_table_hash = 0.0;
  // the unsplit sources that run through the flux-array stage path (no fused stage forms with them)
  // problem/cluster/gravity/gravity_srcterm: the static field acts as the problem's unsplit source (host/cluster.cpp)
  bool gravity_srcterm = false;
  // problem/cluster/agn_feedback/fixed_power != 0 (and not disabled) or problem/cluster/magnetic_tower/fixed_field_rate
  // != 0: the feedback sources follow gravity in ProblemSourceUnsplit (cluster.cpp:63-84; host/cluster.cpp)
  bool feedback_srcterm = false;
  // problem/cluster/agn_triggering/triggering_mode != NONE: the cycle's reduction and removal update cons and prim in
  // place before stage 1 (hydro_driver.cpp:360-394)
  bool agn_triggering = false;
  // problem/cluster/snia_feedback with a rate (the third term of ClusterUnsplitSrcTerm, cluster.cpp:82-83), and
  // problem/cluster/stellar_feedback or problem/cluster/clips (ClusterSplitSrcTerm, cluster.cpp:85-93: once per cycle,
  // after the last stage's unsplit sources)
  bool snia_srcterm = false;
  bool cluster_split_srcterm = false;
  bool flux_path_sources() const {
    return diffusion_configured() || cooling || gravity_srcterm || feedback_srcterm || agn_triggering || snia_srcterm || cluster_split_srcterm;
  }
};

struct LinearWaveState {  // globals of src/pgen/linear_wave.cpp
  int wave_flag = 0;
  double amp = 0.0, vflow = 0.0;
  double sin_a2 = 0, cos_a2 = 1, sin_a3 = 0, cos_a3 = 1, k_par = 0, lambda = 1;
  double d0 = 1, p0 = 0, u0 = 0, gam = 0, gm1 = 0, ev[5] = {0}, rem[5][5] = {{0}};
  bool compute_error = false;
};

struct LinearWaveMhdState {  // what src/pgen/linear_wave_mhd.cpp keeps besides the hydro wave's geometry (LinearWaveState)
  double bx0 = 1.0, by0 = 0.0, bz0 = 0.0, dby = 0.0, dbz = 0.0, ev[7] = {0}, rem[7][7] = {{0}};
  bool dump_max_v2 = false;  // problem/linear_wave/dump_max_v2: the MaxAbsV2 history column (linear_wave_mhd.cpp:739-744)
};

struct CpawState {  // globals of src/pgen/cpaw.cpp
  double den = 1.0, pres = 0, gm1 = 0, b_par = 0, b_perp = 0, v_perp = 0, v_par = 0, fac = 1.0;
  double sin_a2 = 0, cos_a2 = 1, sin_a3 = 0, cos_a3 = 1, lambda = 1, k_par = 0;
  bool compute_error = false;
};

struct FieldLoopState {  // parameters of src/pgen/field_loop.cpp:129-170; B0 normalises UserRelDivB
  int iprob = 1;
  double rad = 0, amp = 0, vflow = 0, drat = 1.0, cos_a2 = 0, sin_a2 = 0, lambda = 0;
};

// <tracers> (src/tracers/tracers.cpp:43-93) and the rank-wide particle arrays (host/tracers.cpp)
struct TracerState {
  // the deck's options
  int seed_method = APK_TRACER_SEED_NONE;
  double per_cell = 0.0;
  long long rng_seed = 0;
  bool fused = true;  // apk_amd/tracer_step = fused | passes
  int nfields = 5;
  // particles seeded on the host and not yet on the device (random_per_block: drawn at creation, uploaded by
  // apk_sim_initialize; a host-only sim keeps them, which is what the CPU tests read)
  std::vector<double> hx, hy, hz;
  std::vector<int64_t> hid;
  std::vector<int32_t> hblock;
  int64_t next_id = 0;  // seed method user: ids run sequentially in call order
  // device: two sets of the arrays (the counting sort writes from one into the other), the block tables of the geometry,
  // the counters {lost, order changed} and the sort's buckets
  int64_t n = 0, cap = 0;
  double *set[2] = {nullptr, nullptr};
  int cur = 0;
  double *d_origin = nullptr, *d_table = nullptr, *d_counters = nullptr, *d_buckets = nullptr;
  int nbuckets = 0;
  apk_tracer_geom geom{};
  long long lost = 0;
  long long steps = 0, sorts = 0;  // tracer steps taken and counting sorts run since initialisation (apk_sim_tracers_stats)
  // apk_amd/tracer_lookback (src/pgen/turbulence.cpp:200-216, 513-647): s and sdot [12][cap] behind each set's arrays,
  // the 26 sums behind the two counters in d_counters (one readback per cycle), a row of partial sums per workgroup
  bool lookback = false;
  double *d_partials = nullptr;
  int64_t partials_cap = 0;
  double t_lookback[APK_TRACER_N_LOOKBACK] = {0};
  long long row_cycle = -1, row_active = 0;  // the last update: its cycle number, the particles it divided by,
  double row_time = 0.0;                     // its time and <s>, <sdot>, corr_s[12], corr_sdot[12]
  double row[2 + 2 * APK_TRACER_N_LOOKBACK] = {0};
  std::string csv_path;  // apk_sim_execute: <outdir>/correlations.csv, a row per cycle (empty: no file)
};

// one <parthenon/outputN> block with file_type = npy (host/snapshot.cpp): a field snapshot output
struct SnapshotOutput {
  std::string block, id;  // the deck block and the id of the file names (default out<N>)
  double dt = 0.0;
  bool single = false;             // single_precision_output
  std::vector<int> codes;          // apk_output_component, duplicates collapsed, deck order
  std::vector<std::string> names;  // their canonical names
};

// one <parthenon/outputN> block with file_type = rst (host/restart.cpp): a restart output
struct RestartOutputBlock {
  std::string block, number, id;  // the deck block, its N and the id of the file names (default out<N>)
  double dt = 0.0;
};

// where one output of apk_sim_execute stands: the block's N, the next output time and the files (rows, for hst) so far
struct OutputSchedule {
  std::string number;
  double next = 0.0;
  long long counter = 0;
};

}  // namespace apk

namespace apk {
namespace host {
struct RcclTransport;  // comm_rccl.cpp
void rccl_transport_destroy(RcclTransport *t);
// one-GPU rehearsal (mesh.hpp "rehearse"): the transport's streams and events without RCCL, every peer's message
// delivered by a device copy on the halo stream from this rank's own send buffer
int comm_loopback_attach(apk_sim *s);
}  // namespace host
}  // namespace apk

struct apk_sim {
  apk::host::RcclTransport *rccl = nullptr;  // native transport (apk_sim_comm_rccl); comm.* point into it
  apk::ParameterInput pin;
  apk::Mesh mesh;
  apk_cooling_table *cool_tab = nullptr;  // the device table of <cooling> (created with ctx)
  apk::HydroPackage pkg;
  std::string problem_id;
  apk::LinearWaveState lw;
  apk::LinearWaveMhdState lwm;
  apk::CpawState cpaw;
  apk::FieldLoopState floop;
  apk_cluster_options cluster{};     // problem_id = cluster as parsed (host/cluster.cpp)
  double *d_block_xmin = nullptr;    // [nblocks + 1][3]: what apk_gravity_src and the feedback sources take
  // AGN feedback and the magnetic tower of the cluster problem as parsed and derived (host/cluster.cpp,
  // host/feedback_model.cpp); the tower's power contributions of the cycle in flight (hydro_driver.cpp:409-449)
  apk_agn_feedback_options agn_opt{};
  apk::AgnFeedbackModel agn;
  apk_magnetic_tower_cfg tower{};
  double tower_linear_contrib = 0.0, tower_quadratic_contrib = 0.0;
  double *d_tower_contribs = nullptr;  // [nblocks][2] (allocated on first use)
  // AGN triggering (host/feedback_model.cpp, host/cluster.cpp): the model, the reduced quantities of the last cycle with
  // what follows from them, this rank's active list (built once at creation) and its device copy
  apk::AgnTriggeringModel trig;
  apk::AgnTriggeringModel::Reduced trig_q;
  double trig_rate = 0.0, trig_time = 0.0, trig_dt = 0.0;
  bool trig_write_to_file = false;
  std::string trig_filename, trig_path;  // trig_path: the file apk_sim_execute appends to (empty: none)
  std::vector<apk_trig_box> trig_boxes;
  long long trig_box_cells = 0, trig_max_box_cells = 0;
  apk_trig_box *d_trig_boxes = nullptr;
  double *d_trig_sums = nullptr;  // [nblocks][4]
  // SNIa feedback, stellar feedback and the clips (host/cluster.cpp): the options as parsed and derived, the split
  // sources' own active list with its device copy, and the five running totals since the last history row
  apk_cluster_source_options csrc{};
  apk_snia_cfg snia{};
  apk_stellar_cfg stellar{};
  apk_clips_cfg clips{};
  std::vector<apk_trig_box> split_boxes;
  long long split_box_cells = 0, split_max_box_cells = 0;
  apk_trig_box *d_split_boxes = nullptr;
  double *d_split_sums = nullptr;  // [nblocks][8]
  double split_totals[5] = {0, 0, 0, 0, 0};
  bool host_only = false;
  bool fused = true;
  int rank = 0, nranks = 1;
  double xmin[3] = {0, 0, 0}, xmax[3] = {1, 1, 1}, dx[3] = {1, 1, 1};
  // SimTime
  double time = 0.0, dt = std::numeric_limits<double>::max(), tlim = 1.0;
  int nlim = -1, ncycle = 0;
  long long fofc_total = 0;
  long long fofc_fallback_stages = 0;
  bool stage_dt_pending = false;  // the last fused stage already reduced the hyperbolic dt
  bool dt_hyp_is_global = false;  // pkg.dt_hyp holds the minimum over all ranks (no reduction needed in pre_step)
  // integrator (Parthenon LowStorageIntegrator)
  int nstages = 0;
  double beta[4] = {0}, gam0[4] = {0}, gam1[4] = {0};
  // device state
  apk_ctx *ctx = nullptr;
  apk_stream_t stream = nullptr;
  apk_allocator alloc{};
  bool have_alloc = false;
  apk_comm_ops comm{};
  bool have_comm = false;
  // doubles per field per block: nper = the slot a block has in a field's allocation (a multiple of 16 when rows are
  // padded), nblk = what is addressed from the block's pointer (nvar * sn), which sits mesh.lead doubles into the slot
  int64_t nper = 0, nblk = 0;
  double *blk(double *field, int64_t lb) const { return field + lb * nper + mesh.lead; }
  // Two conserved-variable buffers: the stage-1 "u1 <- u0" DeepCopy of the reference
  // (hydro_driver.cpp:474-495) is a buffer-role swap here -- stage 1 has gam0 = 0 for every
  // integrator, so it reads the old state as u1 and writes the new state into the other buffer.
  // (a third buffer of the same layout is allocated on first use as the output of trial stages with
  // gam0 != 0 -- first-order flux correction in the later stages of RK2 / RK3 -- whose input u0 must
  // survive a rejected trial; an accepted trial just makes it the current buffer)
  double *d_cons2[3] = {nullptr, nullptr, nullptr};
  int freebuf() const { return 3 - cur - u1buf; }  // the buffer that is neither u0 nor u1
  int cur = 0;    // buffer holding the current state u0 ("base")
  int u1buf = 1;  // buffer holding the register u1 of the step in flight
  // Two primitive-variable buffers as well (the second one is allocated on first use): a stage
  // whose finishing kernel cannot replace prim in place (3-D donor cell, see fused_dc3_kernel)
  // writes the new primitives into the other buffer and the roles swap.
  double *d_prim2[2] = {nullptr, nullptr};
  int pcur = 0;  // buffer holding the primitives of the current state
  double *d_flux[3] = {nullptr, nullptr, nullptr};
  std::vector<double *> send_buf, recv_buf;
  // per buffer: the pack presenting it as MeshData "base" (with prim/flux), the pack presenting it
  // as "u1" (cons, plus the spare prim buffer when there is one), and the ghost-exchange plans that target it
  // [cons buffer][prim buffer]; mu1 packs carry the OTHER prim buffer's arrays as "u1.prim"
  apk_pack *mu0_of[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}},
           *mu1_of[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  apk_copy_plan *plans_of[3][apk::PH_COUNT] = {};
  // the same plans over the two primitive buffers: exchanges that carry PRIMITIVES (GHOST_PRIM_COPY: VL2's half-step
  // state, whose conserved values nobody reads) -- the messages then hold what the face table shows a same-rank reader,
  // the neighbour's stored primitives, and neither side converts anything
  apk_copy_plan *pplans_of[2][apk::PH_COUNT] = {};
  int xchg_prim = 0;  // the primitive buffer such an exchange packs from and fills
  // refined meshes: the boundary-plane fluxes of a fused stage's flux correction run beside the stage kernels
  // (amr_flux_planes_ahead)
  void *side_stream = nullptr, *ev_fork = nullptr, *ev_join = nullptr;
  bool side_stream_failed = false;  // its creation failed once: not tried again
  apk_pack *mu0() const { return mu0_of[cur][pcur]; }
  apk_pack *mu1() const { return mu1_of[u1buf][pcur]; }
  double *d_prim() const { return d_prim2[pcur]; }
  apk_copy_plan *plan(int ph) const { return plans_of[cur][ph]; }
  double *d_cons() const { return d_cons2[cur]; }
  // few-modes turbulence driver (problem_id = turbulence; src/pgen/turbulence.cpp:103-200)
  std::unique_ptr<apk::FewModesFT> fmft;
  double accel_rms = 0.0;
  double *d_acc = nullptr;     // [nblocks][3][Nk][Nj][Ni]
  double *d_phases = nullptr;  // per block: phases_i | phases_j | phases_k
  apk_fmft *fm_dev = nullptr;
  // Overlap of the halo exchange between two stages with the x1 sweep of the next stage
  // (BASELINE north_star / SURVEY 8(e)): after a stage the messages are posted and left in flight
  // (exchange_pending); the next stage runs its x1 sweep on all cells farther than nghost from a
  // face with a remote neighbour, completes the exchange, then does the thin slabs and the rest.
  bool overlap = true;
  bool exchange_pending = false;
  // One-layer exchanges (mesh.hpp PH_PACK_THIN): the exchange at the end of a cycle whose first stage is the
  // donor-cell predictor.  thin_msgs: the message set apk_sim_peer reports is the one-layer one (transports read it at
  // every exchange); xchg_thin: the exchange begun last; remote_ghosts_thin: the ghost zones filled by messages are up
  // to date one layer deep only -- sync_ghosts completes them (a collective, like the one of refined meshes).
  bool thin_on = true, thin_msgs = false, xchg_thin = false, remote_ghosts_thin = false;
  long long thin_exchanges = 0;
  // x1 strips without pack / unpack kernels (apk_stage_args.x1_halo; x1_direct_cycle): the finishing kernels of a VL2
  // cycle store their x1 boundary columns straight into the send buffers (the predictor: primitives, nghost deep, into
  // the full messages; the corrector: the conserved state, one layer, into the one-layer messages) and read their x1
  // ghost columns straight from the receive buffers.  d_x1_tab[0]: the predictor's table (receive: one-layer segments,
  // send: full ones), [1]: the corrector's (receive: full, send: one-layer).
  //   x1_out_direct   the stage just run has stored its x1 strips: the exchange posted next packs without them
  //   xchg_x1_direct  the exchange begun last leaves the x1 ghost columns in the receive buffers (unpacks without them)
  //   x1_in_recv      ... and has completed: the next stage reads them there.  Always together with a one-layer exchange
  //                   (remote_ghosts_thin: whoever else reads ghost zones repeats the exchange in full) or inside a cycle.
  bool x1_on = true;  // apk_sim_set_x1_direct
  void *d_x1_tab[3] = {nullptr, nullptr, nullptr};  // ([2]: full messages both ways -- the RK integrators)
  bool x1_out_direct = false, xchg_x1_direct = false, x1_in_recv = false;
  long long x1_direct_exchanges = 0;
  long long turb_dt_kicks = 0;  // kicks that estimated the time step without storing primitives (apk_turb_apply_dt)
  int pending_c2p = 0;  // the exchange in flight converts ghost zones as it fills them (GHOST_C2P / GHOST_PRIM_ONLY)
  int pending_cons = 0;  // cons buffer whose ghost zones the exchange in flight fills (roles may swap meanwhile)
  // device window tables (apk_stage_args.window, 8 ints per block) of the split stages:
  // main / low slab / high slab
  struct WindowTable {
    int *d = nullptr;
    int rl = 0, rows = 0;
    bool any = false;  // some block has work in this table
  };
  WindowTable x1win[3];  // column windows of the x1 sweep
  WindowTable k3win[3];  // two-kernel stages: plane windows of the x3 sweep
  unsigned *d_late_regions = nullptr;  // per block: bit (sx+1)+3(sy+1)+9(sz+1) = that neighbour region is filled late
  // Direct neighbour addressing (apk_stage_args.face_neighbor; uniform 3-D meshes): per local block
  // and face the local index of the same-rank block behind it, or -1.  While every stage of the
  // cycle is one of the kernels that follow the table, the same-rank ghost copies are skipped
  // altogether and the ghost zones behind those faces go stale; whoever needs them (accessors, a
  // stage form that reads ghost zones) calls sync_ghosts() / materialize_local_ghosts() first.
  int *d_face_nbr = nullptr;
  bool local_ghosts_stale = false;
  bool direct_on = true;  // apk_sim_set_direct_neighbors
  // The primitives of the current (full-step) state are not in memory: the last stage of the cycle computed them for
  // the time-step estimate only (apk_stage_args.fill_derived = 3) because the first stage of the next cycle -- the
  // donor-cell predictor -- derives its input from the conserved state (prim_from_cons).  Whatever else reads
  // primitives goes through sync_ghosts(), which materialises them (ConsToPrim of every block).
  bool prim_stale = false;
  bool prim_free_on = true;  // apk_sim_set_prim_free
  long long skipped_local_exchanges = 0;
  // ... or the criterion itself was reduced with the time-step estimate at the end of the last stage
  // (apk_tag_blocks_dt_from_cons): amr_tags_begin hands this request on instead of launching one
  bool amr_tags_posted = false;
  int amr_posted_criterion = -1, amr_posted_pending = 0;
  double amr_posted_p0 = 0.0, amr_posted_p1 = 0.0;
  bool amr_tag_vars_stored = false;  // the primitives a refinement criterion reads are those of the current state (amr_prim_free_cycle)
  long long amr_c2p_passes_skipped = 0;  // ConsToPrim passes between the stages a refined mesh did without (amr_prim_free_cycle)
  // mesh refinement (parthenon/mesh/refinement = static | adaptive; one rank): the forest of
  // blocks, the index-box plans of the multilevel ghost exchange / flux correction and their device
  // forms, one set per cons buffer the exchange can target
  std::unique_ptr<apk::AmrTree> amr;
  apk::AmrGeom amr_geom;
  apk::AmrPlans amr_plans;
  bool amr_adaptive = false;
  int amr_derefine_count = 10, amr_check_interval = 1;
  long long amr_refined = 0, amr_derefined = 0;  // blocks refined / merged so far
  long long zone_cycles = 0;                     // sum over cycles of the interior cells updated
  long long perf_zone_mark = 0;                  // its value where the timed part of apk_sim_execute began
  double *d_coarse = nullptr;                    // [nblocks][amr_geom.coarse_doubles]
  // distribution over ranks: contiguous Z-order ranges; amr_plans is the global plan (every rank
  // builds the same one), amr_local this rank's share with local block numbers, copies that cross
  // ranks turned into packs / unpacks of one message per peer
  apk::AmrPartition amr_part;
  struct AmrLocalPlans {
    std::vector<apk::AmrRefOp> restrict_own, flux_restrict[3];
    std::vector<apk::BoxRegion> coarse_bc[3];
    // the ghost exchange in its forms (amr_forms.hpp): what a family shares, and every form's same-rank fill list
    struct Family {
      std::vector<apk::AmrRefOp> prolongate;
      std::vector<apk::BoxRegion> pack, unpack;
      std::vector<apk::BoxRegion> fine_bc[3];  // (empty where AMR_FAMILY[].bc names another family's)
    } family[apk::AMR_FAMILIES];
    std::vector<apk::BoxRegion> fill[apk::AMR_XCHG_FORMS];
    std::vector<apk::BoxRegion> flux_copy[3], flux_pack[3], flux_unpack[3];
    // the correction after a fused stage averages the fine fluxes of same-rank faces inside the fix kernel: the
    // restriction operators of flux_copy[d], entry for entry, and those whose coarse side lives on another rank (the
    // only ones that still run as operators there)
    std::vector<apk::AmrRefOp> flux_fused_ops[3], flux_restrict_remote[3];
  } amr_local;
  struct MsgSet {
    apk::AmrMessages plan;
    std::vector<double *> send, recv;
    std::vector<int64_t> send_cap, recv_cap;
  };
  MsgSet amr_halo[apk::AMR_FAMILIES], amr_fluxmsg, amr_move;
  // refined meshes: the form of the exchange run last, that is, which ghost zones of cons are current (amr_forms.hpp);
  // accessors and regridding complete them first (sync_ghosts)
  int amr_ghost_state = apk::AMR_XCHG_FULL;
  bool amr_full_exchange = false;  // apk_sim_set_amr_full_exchange
  const MsgSet *active_msgs = nullptr;  // the message set apk_sim_peer reports (null: the uniform mesh's)
  long long msg_generation = 0;         // bumped whenever that set, its sizes or its buffers change
  struct AmrDevice {
    std::vector<apk_refine_plan *> restrict_own[2], flux_restrict[3], flux_restrict_remote[3];
    apk_copy_plan *coarse_bc[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    // The device forms of AmrLocalPlans::family and ::fill, per cons buffer.  The launches of the exchange before / after
    // the message exchange take no per-cycle arguments: each half is captured once per mesh into a hipGraph and replayed
    // as ONE launch (void* = hipGraphExec_t; null = not captured, the plans are launched one by one) -- `post` belongs
    // to the family, `pre` to the form
    struct Family {
      std::vector<apk_refine_plan *> prolongate;
      apk_copy_plan *pack = nullptr, *unpack = nullptr, *fine_bc[3] = {nullptr, nullptr, nullptr};
      void *post = nullptr;
    } family[2][apk::AMR_FAMILIES];
    struct Form {
      apk_copy_plan *fill = nullptr;
      void *pre = nullptr;
    } form[2][apk::AMR_XCHG_FORMS];
    // no messages between the two halves (one rank): the `pre` graphs hold both halves -- one graph launch per exchange
    bool xchg_whole = false;
    apk_copy_plan *flux_copy[3] = {nullptr, nullptr, nullptr};
    apk_copy_plan *flux_pack[3] = {nullptr, nullptr, nullptr}, *flux_unpack[3] = {nullptr, nullptr, nullptr};
    // the correction applied after a fused stage instead (apk_flux_fix_plan): same-rank faces and
    // faces whose fine side arrived in a message, per cons buffer the stage wrote
    apk_flux_fix_plan *flux_fix[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    apk_flux_fix_plan *flux_fix_unpack[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    apk_flux_fix_plan *flux_fix_all[2] = {nullptr, nullptr}, *flux_fix_unpack_all[2] = {nullptr, nullptr};  // all directions in one launch
    // the faces (6 * local block + face) with a coarser or finer block behind them: the only boundary-plane
    // fluxes the correction after a fused stage reads (apk_calculate_fluxes_boundary_list)
    int *d_cf_faces = nullptr;
    int n_cf_faces = 0;
  } amr_dev;
  // RKL2 super-time-stepping (host/sts.cpp): the registers MY0 and Yjm2 (conserved-size buffers, allocated when rkl2 is
  // on) and the packs presenting them; Y0 is the u1 buffer.  sts_fused: apk_amd/sts_substage = fused | arrays (the default
  // until the fused kernel has been timed below the parent's kernels).
  double *d_my0 = nullptr, *d_yjm2 = nullptr;
  apk_pack *my0_pack = nullptr, *yjm2_pack = nullptr;
  bool sts_fused = false;
  // tracer particles (host/tracers.cpp): null unless tracers/enabled = true
  std::unique_ptr<apk::TracerState> tracers;
  // field snapshots (host/snapshot.cpp): the deck's npy outputs, the staging bound of apk_amd/snapshot_staging_mb in
  // bytes, and the two staging buffers (allocated on first use, grown when a component list needs more)
  std::vector<apk::SnapshotOutput> snap_outs;
  size_t snap_staging_bytes = 0;
  double *d_snap = nullptr;
  void *h_snap = nullptr;  // pinned (hipHostMalloc)
  size_t snap_dev_cap = 0, snap_host_cap = 0;
  // restart (host/restart.cpp): the deck's rst outputs; the schedules of apk_sim_execute's outputs while it runs (what a
  // dump stores) and those a state file brought; whether the state was set by apk_sim_initialize or apk_sim_restore
  std::vector<apk::RestartOutputBlock> rst_outs;
  std::vector<apk::OutputSchedule> out_sched, restored_sched;
  bool initialized = false, restored = false;
  int sts_last_s = 0;           // sub-stages of the last half step taken
  double sts_last_ratio = 0.0;  // its 2 tau / dt_diff
  long long overlapped = 0;
  int perf_cycles = 0;        // cycles inside loop_seconds (after parthenon/time/perf_cycle_offset)
  double loop_seconds = 0.0;  // wall time of the last apk_sim_execute main loop (device synchronised)
  std::string err;
};
