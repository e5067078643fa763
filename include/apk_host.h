/*
 * apk_host.h -- C-ABI of the host-side mini-driver that sits ABOVE the hot-path boundary
 * (include/apk_amd.h) in the standalone build.  It mirrors the reference's control flow
 * for this path only: input deck -> Hydro::Initialize options (src/hydro/hydro.cpp:264-826)
 * -> per-cycle PreStepMeshUserWorkInLoop (hydro.cpp:102-143) -> per-stage task order of
 * HydroDriver::MakeTaskCollection (src/hydro/hydro_driver.cpp:347-673) -> dt control.
 * In a real AthenaPK build Parthenon plays this role and only apk_amd.h is bound
 * (INTEGRATION.md).  Everything here is C++ compiled into libapk_amd.so; Python (tests,
 * bench.py) talks to it through ctypes and supplies device memory / torch.distributed.
 */
#ifndef APK_HOST_H_
#define APK_HOST_H_

#include <stddef.h>
#include <stdint.h>

#include "apk_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct apk_sim apk_sim;

/* Device-memory provider.  NULL => hipMalloc/hipFree.  bench.py / tests pass callbacks
 * that hand out torch CUDA tensors, so that message buffers can be given to
 * torch.distributed (RCCL) without copies.  `tag` names the buffer ("cons", "send:3", ...). */
typedef struct apk_allocator {
  void *user;
  void *(*alloc)(void *user, const char *tag, size_t bytes);
  void (*release)(void *user, void *ptr);
} apk_allocator;

/* Inter-rank operations (one process per GPU).  NULL => single rank.
 *  exchange: all per-peer send buffers are packed and the pack kernels are complete on the
 *            sim's stream when this is called; on return the per-peer receive buffers must
 *            be ready to be read by work enqueued on that stream.
 *  allreduce_min: in-place MIN over ranks of n doubles (dt; mindx/dt_hyp: hydro.cpp:122-128).
 *  allreduce_sum: in-place SUM over ranks (history output).
 *  exchange_begin / exchange_end (optional, both or neither): the same exchange in two halves so
 *            that it can overlap with compute: begin posts the sends/receives (same precondition
 *            as `exchange`) and returns without waiting; end makes work enqueued on the sim's
 *            stream afterwards wait for the receives.  Between the two calls the driver runs the
 *            x1 sweep of the next stage on every cell that does not need the data in flight
 *            (RCCL executes the transfers on its own stream). */
typedef struct apk_comm_ops {
  void *user;
  int (*exchange)(void *user);
  int (*allreduce_min)(void *user, double *vals, int n);
  int (*allreduce_sum)(void *user, double *vals, int n);
  int (*exchange_begin)(void *user);
  int (*exchange_end)(void *user);
} apk_comm_ops;

/* ---- creation from an Athena-style input deck ("<block>" / "key = value") -------------
 * `deck` is the deck TEXT; `overrides` are "block/key=value" strings exactly like the
 * reference's command line (README.md:113-119).  rank/nranks select this process' share
 * of the meshblocks (Morton-ordered contiguous ranges, like Parthenon).
 * On failure returns a negative apk_status and, if errbuf != NULL, a message. */
int apk_sim_create(const char *deck, const char *const *overrides, int noverrides, int rank,
                   int nranks, const apk_allocator *allocator, const apk_comm_ops *comm,
                   apk_stream_t stream, apk_sim **out, char *errbuf, size_t errlen);
void apk_sim_destroy(apk_sim *sim);
const char *apk_sim_last_error(const apk_sim *sim);

/* ---- native RCCL transport (csrc/host/comm_rccl.cpp) -------------------------------------
 * Instead of callbacks the driver can move its messages itself: grouped ncclSend / ncclRecv per
 * peer on a dedicated halo stream (overlapped with compute through events), ncclAllReduce on a second
 * communicator for the per-cycle reductions.  Create the sim with comm = NULL and nranks > 1, then:
 *   rank 0:    apk_rccl_unique_ids(ids, sizeof ids)      two ncclUniqueIds (2 x 128 bytes)
 *   launcher:  broadcast `ids` to all ranks (torch.distributed / MPI / a file)
 *   all ranks: apk_sim_comm_rccl(sim, ids, sizeof ids)    (collective: ncclCommInitRank)
 * before apk_sim_initialize.  One GPU per rank (RCCL refuses two ranks on one device).
 * Replaces Parthenon's boundary communication (hydro_driver.cpp:506, 567-568) and the
 * MPI_Allreduce calls of the package (hydro.cpp:127-128). */
#define APK_RCCL_ID_BYTES 128
int apk_rccl_unique_ids(char *ids, size_t len);
int apk_sim_comm_rccl(apk_sim *sim, const char *ids, size_t len);
/* exchanges posted / reductions done by the native transport so far */
int apk_sim_comm_stats(const apk_sim *sim, long long *exchanges, long long *reductions);
const char *apk_sim_comm_error(const apk_sim *sim);
/* one-rank exercise of the transport on the current device (n doubles sent to self, min / sum
 * reductions); writes "ok" or the failure into msg */
int apk_rccl_selftest(int n, char *msg, size_t len);

/* host-only mode: builds mesh / partition / ghost plans without touching a GPU (used by the
 * CPU tests of the host logic and the world_size-2 gloo tests). */
int apk_sim_create_host_only(const char *deck, const char *const *overrides, int noverrides,
                             int rank, int nranks, apk_sim **out, char *errbuf, size_t errlen);

/* ---- problem setup ------------------------------------------------------------------- */
/* Runs the problem generator selected by <job> problem_id (linear_wave, sod, orszag_tang,
 * synthetic), then ghost exchange -> FillDerived -> first EstimateTimestep (App. A.4). */
int apk_sim_initialize(apk_sim *sim);

/* ---- time integration ---------------------------------------------------------------- */
int apk_sim_step(apk_sim *sim);                      /* one cycle */
int apk_sim_run(apk_sim *sim, int nlim, int *ncycles); /* until tlim or nlim cycles (<0: none) */
double apk_sim_time(const apk_sim *sim);
double apk_sim_dt(const apk_sim *sim);
double apk_sim_tlim(const apk_sim *sim);
double apk_sim_c_h(const apk_sim *sim);
int apk_sim_ncycle(const apk_sim *sim);
long long apk_sim_fofc_count(const apk_sim *sim);
/* 0 = flux-array path (CalculateFluxes + Update + Dedner), 1 = fused stage path */
int apk_sim_set_fused(apk_sim *sim, int fused);
/* 1 (default) = overlap the halo exchange between two stages of a cycle with the x1 sweep of the
 * next stage where possible (remote neighbours, exchange_begin/end given, fused path, >= 2-D, next
 * stage not donor cell); 0 = always exchange synchronously.  Results are identical. */
int apk_sim_set_overlap(apk_sim *sim, int overlap);
/* number of stage boundaries so far at which the exchange was overlapped */
long long apk_sim_overlapped_exchanges(const apk_sim *sim);
/* Direct neighbour addressing (apk_stage_args.face_neighbor): on uniform 3-D meshes whose stages are
 * all single-march donor-cell or two-kernel stages (no passive scalars, floors, extended Dedner source
 * or flux correction) the stage kernels read the interiors of same-rank neighbour
 * blocks directly and the same-rank ghost-zone copies are skipped; ghost zones are brought up to date
 * on demand (every accessor does).  Results are identical.  apk_sim_set_direct_neighbors(sim, 0) switches it
 * off.  Returns the number of stage boundaries so far whose same-rank copies were skipped. */
long long apk_sim_skipped_local_exchanges(const apk_sim *sim);
int apk_sim_set_direct_neighbors(apk_sim *sim, int on); /* 1 (default) / 0 = always copy */
/* Refined meshes, VL2 with a high-order corrector in the two-kernel form, default equation-of-state limits, no passive
 * scalars: the corrector derives its input from the half-step conserved state (apk_stage_args.prim_from_cons = 2, its
 * result over the register u1) and the flux correction's boundary planes likewise
 * (apk_calculate_fluxes_boundary_list_from_cons), so that no ConsToPrim pass runs between the two stages.  Results are
 * identical.  apk_sim_set_prim_free(sim, 0) switches it off.  Returns the number of passes done without. */
long long apk_sim_amr_c2p_passes_skipped(const apk_sim *sim);
/* Full-step primitives kept out of memory (on by default where it applies: uniform 3-D meshes, VL2 -- a donor-cell
 * predictor followed by a two-kernel stage --, default equation-of-state limits, no passive scalars, no extended Dedner
 * source, no forcing): the last stage of a cycle computes the primitives of the new state for the time-step estimate
 * only (apk_stage_args.fill_derived = 3) and the predictor of the next cycle derives its input from the conserved state
 * (prim_from_cons) -- the reference stores them in FillDerived (hydro_driver.cpp:571-577) and reads them back in
 * CalculateFluxes.  Every accessor materialises them on demand; results are identical.  apk_sim_set_prim_free(sim, 0)
 * switches it off.  apk_sim_prim_is_stale: 1 while the primitives of the current state are not in memory.
 * The same switch governs the stage loop of refined meshes (apk_sim_amr_c2p_passes_skipped above). */
int apk_sim_set_prim_free(apk_sim *sim, int on);
/* One-layer exchanges (on by default where they apply: N > 1 ranks, uniform periodic 3-D meshes, VL2, no passive
 * scalars, no extended Dedner source, no forcing): the exchange at the end of a cycle delivers ONE layer of ghost
 * cells -- all the donor-cell predictor of the next cycle reads; the reference exchanges nghost layers after every
 * stage (hydro_driver.cpp:567-568) -- and the corrector's exchange stays a full one.  The messages are a prefix of
 * the same buffers; the transports find the current sizes in apk_sim_peer at every exchange
 * (apk_sim_message_generation tells when they changed).  Accessors that read ghost zones complete them with a full
 * exchange first: a COLLECTIVE then, to be called on every rank, like the accessors of a refined mesh.  Results are
 * identical.  apk_sim_set_thin_exchange(sim, 0) switches it off.  Returns (apk_sim_thin_exchanges) the number
 * of one-layer exchanges so far. */
int apk_sim_set_thin_exchange(apk_sim *sim, int on);
long long apk_sim_thin_exchanges(const apk_sim *sim);
/* x1 strips without pack / unpack kernels (on by default where it applies, uniform periodic 3-D meshes over N > 1 ranks:
 * the VL2 cycles that take one-layer exchanges and store no full-step primitives, and the RK integrators whose stages all
 * derive their input from the conserved state in the two-kernel form): the finishing kernel of a stage
 * stores its x1 boundary columns straight into the send buffers and the kernels of the next stage read their x1 ghost
 * columns straight from the receive buffers (apk_stage_args.x1_halo in apk_amd.h); the pack and unpack plans leave the
 * x1 faces out.  The messages are byte for byte what the pack kernel would have written, so a rank may use the path or
 * not independently of its peers; results are identical.  Accessors that read ghost zones repeat such an exchange in full
 * first (a COLLECTIVE, as after a one-layer exchange).  apk_sim_set_x1_direct(sim, 0) switches it off.
 * apk_sim_x1_direct_exchanges: the number of exchanges so far whose x1 strips went that way. */
int apk_sim_set_x1_direct(apk_sim *sim, int on);
long long apk_sim_x1_direct_exchanges(const apk_sim *sim);
int apk_sim_prim_is_stale(const apk_sim *sim);
/* forced turbulence in a cycle that stores no primitives: number of kicks that estimated the time step without storing
 * them (apk_turb_apply_dt) so far */
long long apk_sim_turb_dt_kicks(const apk_sim *sim);
/* Refined meshes: the stage loop's exchange leaves out the ghost zones behind block edges and corners
 * (no sweep or flux correction reads them; accessors, tagging and the last exchange of a cycle that
 * checks the refinement criteria complete them).  1 = always exchange in full: same results, for A/B timing and
 * for the tests of that statement. */
int apk_sim_set_amr_full_exchange(apk_sim *sim, int on);

/* ---- introspection ------------------------------------------------------------------- */
typedef struct apk_sim_info {
  int fluid, recon, riemann, integrator;
  int nx[3], mb[3], ng, nhydro, nscalars, ndim;
  int nblocks_total, nblocks_local, first_gid;
  int rank, nranks, npeers;
  int fofc, dedner_extended, fused;
  double cfl, gamma, glmmhd_alpha;
  double xmin[3], xmax[3], dx[3];
  int64_t cells_per_block; /* incl. ghosts */
  int64_t zones_local;     /* interior cells on this rank */
  int64_t zones_total;
} apk_sim_info;
int apk_sim_get_info(const apk_sim *sim, apk_sim_info *info);
/* the <diffusion> options as parsed (hydro.cpp:538-702): the processes and coefficients, diffusion/integrator
 * (apk_diffint) and diffusion/cfl (0 when the integrator is none) */
int apk_sim_diffusion_options(const apk_sim *sim, apk_diff_cfg *cfg, int *integrator, double *cfl_diff);
/* diffusion/conduction_coeff = spitzer as parsed (hydro.cpp:567-593): *enabled whether Spitzer conduction is on, and
 * then the converted coefficient (diffusion/spitzer_cond_in_erg_by_s_K_cm, default 4.6e-7, times erg / (s cm) in code
 * units), mbar and k_boltzmann -- what the driver hands to the *_v2 diffusion entry points; all 0 otherwise */
int apk_sim_spitzer_options(const apk_sim *sim, int *enabled, apk_spitzer_cfg *cfg);
/* diffusion/rkl2_max_dt_ratio as parsed (-1 unless diffusion/integrator = rkl2, which requires a positive one) */
double apk_sim_rkl2_max_dt_ratio(const apk_sim *sim);
/* super-time-stepping: what the last half step did -- its number of sub-stages and its ratio 2 tau / dt_diff (0 before
 * the first cycle) -- and which form a sub-stage takes: 1 the fused kernel (apk_rkl2_substage_fused), 0 the passes over
 * the flux arrays (apk_amd/sts_substage = fused | arrays) */
int apk_sim_sts_info(const apk_sim *sim, int *s_rkl, double *ratio, int *fused);
/* <units> (src/units.hpp) and the gas composition (hydro.cpp:482-503) as parsed.  has_units: a <units> block exists;
 * has_composition: so does hydro/He_mass_fraction (mu, mu_e, mbar, mbar_over_kb are 0 otherwise). */
typedef struct apk_units_info {
  int has_units, has_composition;
  double code_length_cgs, code_mass_cgs, code_time_cgs;
  double mh, k_boltzmann, atomic_mass_unit, erg, cm, s; /* in code units */
  double He_mass_fraction, mu, mu_e, mbar, mbar_over_kb;
  double efloor, eceil; /* the EOS fields hydro/Tfloor and hydro/Tceil map to */
} apk_units_info;
int apk_sim_units(const apk_sim *sim, apk_units_info *info);
/* <cooling> as parsed (tabular_cooling.cpp:30-276): *enabled = 1 for enable_cooling = tabular (then *params is filled,
 * else zeroed), *n_temp = rows of the table */
int apk_sim_cooling_options(const apk_sim *sim, int *enabled, apk_cooling_params *params, int *n_temp);
/* one array of the parsed table: which = 0 log_temps, 1 log_lambdas (code units), 2 Townsend alpha_k, 3 Townsend Y_k
 * (n_temp - 1 entries; townsend only); copies min(n, size) values into out, *size = the array's length */
int apk_sim_cooling_table(const apk_sim *sim, int which, double *out, int n, int *size);
/* ---- the cluster problem (job/problem_id = cluster; src/pgen/cluster.cpp, csrc/host/cluster.cpp) ------------------
 * The slice built here: static gravity (NFW + Hernquist BCG + SMBH) as an unsplit source, the ACCEPT-like entropy
 * profile and the hydrostatic-equilibrium sphere, or uniform gas; a uniform field with GLM-MHD.  Keys and defaults are
 * the reference's (<problem/cluster>, .../gravity, .../entropy_profile, .../hydrostatic_equilibrium, .../uniform_gas,
 * .../uniform_b_field; AGN feedback, the magnetic tower, AGN triggering, SNIa feedback, stellar feedback and the clips:
 * below).  Refused at creation, each with a message naming the
 * key: refined meshes, nx2 = 1 or nx3 = 1, init_perturb/sigma_v or sigma_b != 0, dipole_b_field, reductions, the
 * sphere without <units> and hydro/He_mass_fraction, uniform_b_field without GLM-MHD, gravity_srcterm with
 * diffusion/integrator = rkl2.  All entries below work on a host-only sim. */
typedef struct apk_cluster_options {
  int enabled; /* problem_id = cluster */
  int include_nfw_g, which_bcg_g, include_smbh_g, gravity_srcterm;
  int init_uniform_gas, init_uniform_b_field, test_he_sphere, test_he_sphere_n_r;
  double hubble_parameter;
  double m_nfw_200, c_nfw, alpha_bcg_s, beta_bcg_s, m_bcg_s, r_bcg_s, m_smbh, g_smoothing_radius;
  double k_0, k_100, r_k, alpha_k;
  double r_fix, rho_fix, r_sampling, test_he_sphere_r_start, test_he_sphere_r_end;
  double uniform_gas_rho, uniform_gas_ux, uniform_gas_uy, uniform_gas_uz, uniform_gas_pres;
  double uniform_b_field_bx, uniform_b_field_by, uniform_b_field_bz;
  double mh, k_boltzmann, mu, mu_e; /* what the sphere takes from Units and the composition (0 without them) */
  /* src/units.hpp in code units */
  double gravitational_constant, msun, kpc, mpc, km_s, kev;
  apk_cluster_gravity gravity; /* ClusterGravity's members */
} apk_cluster_options;
int apk_sim_cluster_options(const apk_sim *sim, apk_cluster_options *opt);
/* HydrostaticEquilibriumSphere::generate_P_rho_profile(r_start, r_end, n_r) and the columns PRhoProfile::
 * write_to_ostream derives from it: out[9][n_r] = r, P, K, rho, n, ne, T, g, dP_dr */
int apk_sim_he_sphere_profile(apk_sim *sim, double r_start, double r_end, int n_r, double *out);
/* the radial mesh local block lb integrates for itself (generate_P_rho_profile(ib, jb, kb, coords)): copies min(n,
 * size) values into r and p, *size = its length */
int apk_sim_block_he_profile(apk_sim *sim, int lb, double *r, double *p, int n, int *size);
/* the problem generator's conserved state of local block lb, interior cells only: out[nvar][nx3][nx2][nx1] of the
 * block (every generator that fills block by block; not turbulence) */
int apk_sim_pgen_block(apk_sim *sim, int lb, double *out);
/* apk_gravity_src once on the current state with the given beta_dt (conserved state and stored primitives of the
 * current buffers).  For tests. */
int apk_sim_gravity_src(apk_sim *sim, double beta_dt);

/* ---- fixed-power AGN feedback and the magnetic tower of the cluster problem (src/pgen/cluster/agn_feedback.cpp,
 * magnetic_tower.{hpp,cpp}, jet_coords.hpp; csrc/host/feedback_model.cpp, csrc/host/cluster.cpp) ---------------------
 * Keys and defaults are the reference's: <problem/cluster/precessing_jet> jet_theta, jet_phi_dot, jet_phi0;
 * <problem/cluster/agn_feedback> fixed_power, efficiency, thermal_fraction, kinetic_fraction, magnetic_fraction,
 * enable_magnetic_tower_mass_injection, thermal_radius, kinetic_jet_radius, kinetic_jet_thickness, kinetic_jet_offset,
 * kinetic_jet_velocity and / or kinetic_jet_temperature, vceil, Tceil, disabled; <problem/cluster/magnetic_tower>
 * potential_type = donut | li, li_alpha, l_scale, donut_offset, donut_thickness, initial_field, fixed_field_rate,
 * fixed_mass_rate, l_mass_scale.  A violated requirement of the reference is a deck error with its wording.  Refused at
 * creation, naming the key: fixed_power != 0 without <units> and hydro/He_mass_fraction, or with all three fractions zero
 * (the reference fails that at the first stage); magnetic_fraction != 0 or a non-zero tower field or rate without
 * hydro/fluid = glmmhd; a magnetic_tower block whose potential_type is neither donut nor li (stricter than the
 * reference, which fails inside a kernel); enable_tracer = true.  With AGN triggering (below) the power is fixed_power +
 * accretion_rate * efficiency * c^2, the source runs whenever that is not zero, and the history has an
 * agn_feedback_power column; without it the columns are the ones a run had before.  All entries but the three sources
 * work on a host-only sim. */
typedef struct apk_agn_feedback_options {
  int configured; /* a <problem/cluster/agn_feedback> block was read and its derived numbers are valid */
  int active;     /* not disabled and (fixed_power != 0 or a triggering mode): the source runs in every stage whose power != 0 */
  int disabled, enable_magnetic_tower_mass_injection, assumed_cold_jet;
  int tower_potential; /* apk_tower_potential */
  int tower_power_scaling; /* magnetic_fraction != 0 && (fixed_power != 0 || a triggering mode): the contributions are reduced every cycle */
  double fixed_power, efficiency;
  double thermal_fraction, kinetic_fraction, magnetic_fraction; /* normalised to sum 1 */
  double thermal_mass_fraction, kinetic_mass_fraction, magnetic_mass_fraction;
  double thermal_radius, kinetic_jet_radius, kinetic_jet_thickness, kinetic_jet_offset;
  double kinetic_jet_velocity, kinetic_jet_temperature, kinetic_jet_e; /* as given or derived */
  double vceil, Tceil, eceil;
  double jet_theta, jet_phi_dot, jet_phi0;
  double li_alpha, l_scale, donut_offset, donut_thickness, initial_field, fixed_field_rate, fixed_mass_rate, l_mass_scale;
  double speed_of_light, mbar_gm1_over_kb; /* what the derivations take from Units and the composition */
  double power, mass_rate;                 /* GetFeedbackPower / GetFeedbackMassRate with the current accretion rate */
} apk_agn_feedback_options;
int apk_sim_agn_feedback_options(const apk_sim *sim, apk_agn_feedback_options *opt);
/* the numbers of agn_feedback.cpp:263-303 for beta_dt, and the jet frame at `time` (what the kernels are passed) */
int apk_sim_agn_feedback_stage_numbers(const apk_sim *sim, double beta_dt, double time, apk_agn_feedback_cfg *cfg,
                                       apk_jet_coords *jet);
/* MagneticTower::PowerSrcTerm's field_to_add = (-lin + sqrt(lin^2 + 4 quad beta_dt P)) / (2 quad); fails with the
 * reference's two messages (both contributions zero; negative discriminant or quad = 0) */
int apk_sim_magnetic_tower_field_to_add(apk_sim *sim, double lin, double quad, double beta_dt, double power, double *field);
/* apk_agn_feedback_src once on the current state (thermal and kinetic channels; conserved state and stored primitives of
 * the current buffers), jet frame at `time`.  For tests. */
int apk_sim_agn_feedback_src(apk_sim *sim, double beta_dt, double time);
/* apk_magnetic_tower_src once on the current state with (field_to_add, mass_to_add), jet frame at `time`.  For tests. */
int apk_sim_magnetic_tower_src(apk_sim *sim, double field, double mass, double time);
/* apk_magnetic_tower_power_contribs on the current state, jet frame at `time`: out[0] = sum(prim_B . b1 dV), out[1] =
 * sum(0.5 b1^2 dV) over the whole mesh.  Each local block's pair goes into its slot of a zeroed array of 2 *
 * nblocks_global, allreduce_sum adds the arrays, and the host adds the slots in global block order: the result does not
 * depend on how the blocks are distributed over ranks (the reference sums per-rank partial sums).  A collective. */
int apk_sim_magnetic_tower_contribs(apk_sim *sim, double time, double out[2]);

/* ---- AGN triggering of the cluster problem (src/pgen/cluster/agn_triggering.{hpp,cpp}; csrc/host/feedback_model.cpp,
 * csrc/host/cluster.cpp, csrc/kernels_triggering.hip) -----------------------------------------------------------------
 * <problem/cluster/agn_triggering> with the reference's keys and defaults: triggering_mode = NONE | COLD_GAS |
 * BOOSTED_BONDI | BOOTH_SCHAYE, accretion_radius, cold_temp_thresh (K), cold_t_acc, bondi_alpha, bondi_n0, bondi_beta,
 * accretion_cfl (0.1), removed_accreted_mass (true), write_to_file, triggering_filename; bondi_M_smbh is
 * problem/cluster/gravity/m_smbh.  An unknown mode is a deck error ("Unrecognized AGNTriggeringMode").  Refused at
 * creation, naming the key: a mode with accretion_radius <= 0 or COLD_GAS with cold_t_acc <= 0 (both name
 * .../triggering_mode; stricter than the reference, where they give 0/0 and an infinite rate), BOOTH_SCHAYE with
 * bondi_n0 <= 0, accretion_cfl <= 0, a mode without <units> and hydro/He_mass_fraction, with diffusion/integrator = rkl2,
 * or with feedback enabled and all three fractions zero.
 * Once per cycle, before the tower's contributions (hydro_driver.cpp:360-394): reduce (COLD_GAS removes in the same
 * launch, with the cycle's dt), one sum over ranks with every block's sums in its own slot, the slots added in global
 * block order -- the result does not depend on the distribution of the blocks -- and, for the Bondi-like modes with
 * removed_accreted_mass, the removal.  A Bondi-like cycle whose reduced total_mass is zero fails the step.  The
 * triggering limit of the time step (agn_triggering.cpp:556-584) joins min_dt.  Not restarted; uniform meshes. */
typedef struct apk_agn_triggering_options {
  int mode; /* apk_agn_triggering_mode */
  int remove_accreted_mass, write_to_file;
  int active_blocks;          /* this rank's entries of the active list ... */
  long long active_box_cells; /* ... and the cells of their boxes */
  double accretion_radius, cold_temp_thresh, cold_t_acc, bondi_alpha, bondi_M_smbh, bondi_n0, bondi_beta, accretion_cfl;
  double mean_molecular_mass;       /* mu * atomic_mass_unit */
  double mean_molecular_mass_by_kb; /* mean_molecular_mass / k_boltzmann: what the kernel is passed */
  double gravitational_constant;
  char triggering_filename[256];
} apk_agn_triggering_options;
int apk_sim_agn_triggering_options(const apk_sim *sim, apk_agn_triggering_options *opt);
/* the last cycle's (or the last apk_sim_agn_triggering_reduce's) reduced quantities, all zero before the first */
typedef struct apk_agn_triggering_state {
  double cold_mass;                                                                /* COLD_GAS */
  double total_mass, mass_weighted_density, mass_weighted_velocity, mass_weighted_cs; /* Bondi-like: the four sums */
  double accretion_rate; /* GetAccretionRate of them (0 before the first reduction) */
  double power;          /* AGNFeedback::GetFeedbackPower with that rate (0 without an <agn_feedback> block) */
  double dt_limit;       /* EstimateTimeStep: DBL_MAX where the reference gives no limit */
  double time, dt;       /* of the cycle that reduced them */
} apk_agn_triggering_state;
int apk_sim_agn_triggering_state(const apk_sim *sim, apk_agn_triggering_state *st);
/* GetAccretionRate (agn_triggering.cpp:319-365) of the given reduced quantities with this sim's parameters: q[0] =
 * cold_mass (COLD_GAS), or q[0..3] = total_mass and the three mass-weighted sums.  Works on a host-only sim. */
int apk_sim_agn_triggering_accretion_rate(const apk_sim *sim, const double *q, double *rate);
/* EstimateTimeStep (agn_triggering.cpp:556-584) of the given reduced quantities */
int apk_sim_agn_triggering_timestep(const apk_sim *sim, const double *q, double *dt);
/* AGNFeedback::GetFeedbackPower and GetFeedbackMassRate (agn_feedback.cpp:187-212) for the given accretion rate:
 * fixed_power + rate * efficiency * c^2 and rate * (1 - efficiency) + fixed_power / (efficiency * c^2).  Needs a configured
 * feedback model (apk_agn_feedback_options.configured).  Works on a host-only sim. */
int apk_sim_agn_feedback_power_of(const apk_sim *sim, double accretion_rate, double *power, double *mass_rate);
/* this rank's active list: copies min(n, size) entries of 7 ints (local block, lo[3], hi[3]) into out, *size = the
 * number of entries.  Works on a host-only sim. */
int apk_sim_agn_triggering_active_list(const apk_sim *sim, int *out, int n, int *size);
/* One reduction (for COLD_GAS with the removal) on the current state with this dt, the sum over ranks, and the state
 * above updated: what a cycle does before the Bondi removal.  A collective.  For tests. */
int apk_sim_agn_triggering_reduce(apk_sim *sim, double dt);
/* RemoveBondiAccretedGas on the current state with the stored total_mass and accretion rate.  For tests. */
int apk_sim_agn_triggering_remove_bondi(apk_sim *sim, double dt);

/* ---- SNIa feedback, stellar feedback and the clips of the cluster problem (src/pgen/cluster/snia_feedback.cpp,
 * stellar_feedback.cpp, cluster_clips.cpp, cluster.cpp:240-313; csrc/host/cluster.cpp, csrc/kernels_cluster_sources.hip)
 * Keys and defaults are the reference's: <problem/cluster/snia_feedback> power_per_bcg_mass, mass_rate_per_bcg_mass,
 * disabled (false); <problem/cluster/stellar_feedback> stellar_radius, exclusion_radius (0: agn_triggering/
 * accretion_radius), efficiency, number_density_threshold, temperature_threshold (all zero: disabled);
 * <problem/cluster/clips> clip_r (-1), dfloor (-1), vceil, vAceil, Tceil (infinity), eceil = Tceil / mbar_over_kb /
 * (gamma - 1).  Refused at creation, naming the key ("refused, never ignored" extends to blocks that would be inert):
 * snia_feedback not disabled with both rates zero (the reference runs it as a no-op) or without a BCG; a partly set
 * stellar block; stellar feedback without <units> and hydro/He_mass_fraction; clip_r > 0 with no limit set; a limit off
 * its default with clip_r <= 0; vAceil without GLM-MHD; Tceil without units; any of the three with
 * diffusion/integrator = rkl2.
 * SNIa runs in every flux-array stage after the feedback sources, with the stage's beta_dt (cluster.cpp:82-83).  The
 * split sources run once per cycle after the unsplit sources of the last stage and before its exchange, with the full
 * dt (hydro_driver.cpp:548-560), over an active list of their own: per local block the interior index box of the cells
 * that can lie within max(stellar_radius, clip_r).  Their five sums go through the rank-order sum into running totals
 * that accumulate per cycle and are reset when a history row is written (cluster.cpp:300-313); runs with stellar
 * feedback or clips, and only those, carry them as five more history columns under the reference's names.  Not
 * restarted; uniform meshes; the reductions cold_mass and agn_extent are not built. */
typedef struct apk_cluster_source_options {
  int snia_active, stellar_active, clips_active;
  int flux_path_sources;      /* some source of this run (these three or any other) keeps its stages on the flux-array path */
  int active_blocks;          /* this rank's entries of the split sources' active list ... */
  long long active_box_cells; /* ... and the cells of their boxes */
  double power_per_bcg_mass, mass_rate_per_bcg_mass, rho_const_bcg; /* SNIa; rho_const_bcg as apk_snia_cfg's */
  double stellar_radius, exclusion_radius, efficiency, number_density_threshold, temperature_threshold;
  double mbar, mbar_over_kb, mass_to_energy; /* mu * mh, the package's mbar_over_kb, efficiency * c * c (0 without units) */
  double clip_r, dfloor, vceil, vAceil, Tceil, eceil;
} apk_cluster_source_options;
int apk_sim_cluster_source_options(const apk_sim *sim, apk_cluster_source_options *opt);
/* the split sources' active list, as apk_sim_agn_triggering_active_list.  Works on a host-only sim. */
int apk_sim_cluster_split_active_list(const apk_sim *sim, int *out, int n, int *size);
/* apk_snia_feedback_src once on the current state with the given beta_dt.  For tests. */
int apk_sim_snia_feedback_src(apk_sim *sim, double beta_dt);
/* apk_cluster_split_src once on the current state (stellar / clips: which of the configured steps run), the sum over
 * ranks into out[5] (stellar_mass, added_dfloor_mass, removed_eceil_energy, removed_vceil_energy, added_vAceil_mass) and
 * into the running totals.  dt is taken for symmetry with the reference's call; neither step depends on it.  A
 * collective.  For tests. */
int apk_sim_cluster_split_src(apk_sim *sim, double dt, int stellar, int clips, double out[5]);
/* the running totals since the last history row, in the order above */
int apk_sim_cluster_source_totals(const apk_sim *sim, double out[5]);

/* ---- tracer particles (<tracers>, src/tracers/tracers.cpp; csrc/host/tracers.cpp) ---------------------------------
 * Keys (tracers.cpp:43-93, 102-118): enabled (default false), initial_seed_method = none | random_per_block | user,
 * initial_num_tracers_per_cell, initial_rng_seed; and apk_amd/tracer_step = fused (default) | passes.  Refused at
 * creation: nx3 == 1, parthenon/mesh/refinement != none, more than one rank, nghost < 2, an unknown seed method,
 * random_per_block with a per-block count <= 0.  One rank, uniform meshes, no restart.
 * random_per_block draws its positions on the HOST from a stateless counter-based generator (splitmix64 keyed on
 * (initial_rng_seed + gid, n, component), 53-bit mantissas) where the reference uses Kokkos' pool: same layout of ids
 * (n_per_block * gid + n), other positions. */
enum apk_tracer_seed { APK_TRACER_SEED_NONE = 0, APK_TRACER_SEED_RANDOM_PER_BLOCK = 1, APK_TRACER_SEED_USER = 2 };
typedef struct apk_tracers_options {
  int enabled, seed_method, fused, nfields; /* nfields: 5, or 8 with GLM-MHD (B_x, B_y, B_z) */
  double num_tracers_per_cell;
  long long rng_seed, num_tracers_per_block;
} apk_tracers_options;
/* the options as parsed (valid on a host-only sim; all zero with tracers disabled) */
int apk_sim_tracers_options(const apk_sim *sim, apk_tracers_options *opt);
/* particles in the arrays, of which active, and lost so far through non-periodic boundaries (total = active + lost) */
int apk_sim_tracers_count(apk_sim *sim, long long *total, long long *active, long long *lost);
/* tracer steps taken since apk_sim_initialize and counting sorts run (one at seeding, then one after every step in
 * which a particle changed its block or was lost) */
int apk_sim_tracers_stats(const apk_sim *sim, long long *steps, long long *sorts);
/* one array in storage order (the driver keeps particles sorted by block and k-plane, not by id): field 0 x, 1 y, 2 z
 * (doubles), 3 id (int64), 4 local block index (int32), 5 active flag (int32), 6.. rho, pressure, vel_x, vel_y, vel_z,
 * B_x, B_y, B_z (doubles).  A host-only sim returns fields 0..4 of what the deck seeded. */
int apk_sim_tracers_read(apk_sim *sim, int field, void *out);
/* seed method user (ProblemSeedInitialTracers): n more particles at the given positions, ids sequential in call order;
 * owners from the block grid, fields filled at once (tracers.cpp:173-186).  Positions outside the domain are refused. */
int apk_sim_tracers_seed(apk_sim *sim, const double *x, const double *y, const double *z, long long n);
/* the tracer step alone on the current state (what apk_sim_step runs after the last stage with the cycle's dt):
 * completes primitives and ghost zones, advects, re-owns, fills, sorts when ownership changed.  For tests. */
int apk_sim_tracers_step(apk_sim *sim, double dt);
/* ---- tracer lookback histories and their correlations (src/pgen/turbulence.cpp:200-216, 513-647) --------------------
 * apk_amd/tracer_lookback = true | false (default false; anything else, and true without tracers/enabled = true, is
 * refused at creation).  Opt-in and independent of the problem generator, where the reference turns it on for
 * problem_id = turbulence whenever tracers are on.  Every particle then carries APK_TRACER_N_LOOKBACK levels of
 * s = ln rho and sdot; the update runs once when the deck's particles are seeded (cycle 0, the sim's dt;
 * tracers.cpp:183-186) and after the fill of every tracer step (hydro_driver.cpp:654-658) with the cycle number and the
 * time at the START of the cycle.  Particles of apk_sim_tracers_seed start with empty (zero) histories: no update runs
 * at user seeding.  apk_sim_execute writes <outdir>/correlations.csv: one '#' header line and one row per cycle,
 * cycle,time,s,sdot,corr_s[0..11],corr_sdot[0..11],t_lookback[0..11], %.17g. */
int apk_sim_tracer_lookback_options(const apk_sim *sim, int *enabled, int *n_lookback);
/* the histories in storage order like apk_sim_tracers_read: which = 0 s, 1 sdot; out[n_lookback][particles] */
int apk_sim_tracer_lookbacks_read(apk_sim *sim, int which, double *out);
/* the row of the last update (turbulence.cpp:603-641): the cycle number and time it ran with, the active particles it
 * divided by, and row[38] = <s>, <sdot>, corr_s[12], corr_sdot[12], t_lookback[12].  *cycle = -1 before any update. */
int apk_sim_tracer_correlations(const apk_sim *sim, long long *cycle, double *time, long long *n_active, double *row);

/* global block id and logical (bx,by,bz) of local block lb */
int apk_sim_block_location(const apk_sim *sim, int lb, int *gid, int loc[3]);
/* Mesh refinement (parthenon/mesh/refinement = static | adaptive, numlevel, derefine_count,
 * <parthenon/static_refinement#>, <refinement>): refinement level of a local block (0 on uniform
 * meshes); apk_sim_block_location then returns the logical location at that level.  Statistics:
 * blocks refined / sibling groups merged so far, deepest level allowed, zone-cycles done.
 * apk_sim_regrid runs one tag -> refine / derefine -> transfer pass on demand. */
/* hydro/first_order_flux_correct = true: stages with gam0 = 0 run fused and are only redone through
 * the flux-array sequence + FirstOrderFluxCorrect when a cell fails its admissibility test; this counts
 * those fallbacks */
long long apk_sim_fofc_fallback_stages(const apk_sim *s);
int apk_sim_block_level(const apk_sim *s, int lb);
int apk_sim_amr_stats(const apk_sim *s, long long *refined, long long *derefined, int *max_level,
                      long long *zone_cycles);
int apk_sim_regrid(apk_sim *s, int *changed);
/* a regridding pass for given per-block tags (+1 / 0 / -1, one per block of the whole forest, the
 * same array on every rank): forest update with 2:1 balance and derefine_count, new distribution,
 * new plans; on a device sim also the transfer of the state (copy / prolongate / restrict), ghost
 * exchange and ConsToPrim on the new mesh */
int apk_sim_amr_apply_tags(apk_sim *s, const int *tags, int ntags, int *changed);
/* device pointers of local block lb: field 0 = cons, 1 = prim, 2 = u1.cons */
void *apk_sim_block_ptr(const apk_sim *sim, int lb, int field);
/* copy the interior of every local block of `field` into a global-shaped host array
 * [nvar][nx3][nx2][nx1] (only this rank's cells are written) */
int apk_sim_gather(apk_sim *sim, int field, double *host_out);
/* copy one full block (incl. ghosts) host<->device.  Ghost zones are brought up to date first: the stage loop
 * leaves same-rank ghost zones of uniform meshes (direct neighbour addressing) and the ghost zones behind edges
 * and corners of refined meshes unfilled.  On a REFINED mesh distributed over several ranks that completion
 * is a halo exchange, i.e. collective: the first accessor after a cycle must be called on every rank (as the
 * outputs of apk_sim_execute are).  On uniform meshes it is local. */
int apk_sim_read_block(apk_sim *sim, int lb, int field, double *host_out);
int apk_sim_write_block(apk_sim *sim, int lb, int field, const double *host_in);
/* history sums over the whole mesh (allreduce'd): mass,1-mom,2-mom,3-mom,KE,tot-E,ME,relDivB.  GLM-MHD: relDivB
 * differences B across block faces, so the ghost zones are brought up to date first, as by the block accessors (and the
 * primitives stored, where the last cycle kept them out of memory): the column is that of the current state whatever the
 * stage loop left stale, and the call is collective where that completion is. */
int apk_sim_history(apk_sim *sim, double *out8);
/* linear-wave L1 errors vs the initial condition (src/pgen/linear_wave.cpp:183-335) */
/* few-modes turbulence driver (job/problem_id = turbulence).  History: volume sums of Ms, Ma,
 * plasma beta (src/pgen/turbulence.cpp:47-101; divide by the box volume for the means).  The
 * fmft_* calls expose the host spectral state (FewModesFT, src/utils/few_modes_ft.cpp) and also
 * work on a host-only sim: var_hat is [3][num_modes][2]; evolve advances the OU process by dt
 * (consuming RNG draws exactly as a driven step does); phases fills [2][num_modes][n] for cells
 * g0..g0+n-1 of `axis`.  read_acc copies block lb's acceleration field [3][Nk][Nj][Ni]. */
int apk_sim_turbulence_history(apk_sim *sim, double *out3);
/* field_loop's extra history column "UserRelDivB" (src/pgen/field_loop.cpp:60-103), summed over ranks */
int apk_sim_user_reldivb(apk_sim *s, double *out);
int apk_sim_fmft_num_modes(const apk_sim *sim);
int apk_sim_fmft_var_hat(const apk_sim *sim, double *out);
int apk_sim_fmft_evolve(apk_sim *sim, double dt);
int apk_sim_fmft_phases(const apk_sim *sim, int axis, int n, int g0, double *out);
int apk_sim_read_acc(apk_sim *sim, int lb, double *host_out);
/* The refinement criterion configured by the deck's <refinement> block (src/hydro/hydro.cpp:
 * 788-816: type = pressure_gradient | xyvelocity_gradient | maxdensity with their thresholds),
 * evaluated on every local block (pkg->CheckRefinementBlock): tags[lb] = +1 refine, 0 same,
 * -1 derefine; crit (may be NULL) receives the reduced criterion.  The mesh stays uniform. */
int apk_sim_check_refinement(apk_sim *sim, int *tags, double *crit);

/* ---- text outputs in the reference's formats ---------------------------------------------
 * History: one row per call, "time dt cycle nbtotal" followed by the package's history list
 * (src/hydro/hydro.cpp:422-441: mass 1-mom 2-mom 3-mom KE tot-E [ME relDivB]; turbulence adds
 * Ms [Ma plasma_beta], src/pgen/turbulence.cpp:104-116), under the two '#' header lines
 * Parthenon's history writer emits ("[n]=label" columns), so numpy.genfromtxt-based analysis
 * written for the reference reads it unchanged (e.g. tst/regression/test_suites/turbulence/
 * turbulence.py:42-52 takes Ms, Ma from the third- and second-to-last columns).  The header is
 * written when the file does not exist yet.  All ranks must call; rank 0 writes.
 * Error file: src/pgen/linear_wave.cpp:296-334 ("linearwave-errors.dat": header when new,
 * otherwise append; the Nx2-twice quirk of the reference's row is kept). */
int apk_sim_history_labels(const apk_sim *sim, char *buf, size_t len); /* space separated */
int apk_sim_write_history(apk_sim *sim, const char *path);
int apk_sim_write_linear_wave_errors(apk_sim *sim, const char *path);
/* main loop of a deck run (what `athenaPK -i deck` does for the scope here): initialize, step to
 * tlim / nlim, write every <parthenon/output*> block with file_type = hst to
 * <outdir>/<parthenon/job problem_id, default "parthenon">.out<N>.hst at its `dt` cadence (t = 0
 * and the final time included), every block with file_type = npy as field snapshots (below) at the same
 * cadence rule (a GLM-MHD history row completes the ghost zones first, see apk_sim_history), every block with
 * file_type = rst as restart dumps (below; none at t = 0), and, for linear_wave with
 * compute_error, the error file.  On a sim restored with apk_sim_restore it does not initialise, writes no row or dump for
 * the restored time, appends to the history files and the triggering file, takes every output's next time and counter
 * from the state file, and counts nlim from the run's cycle number. */
int apk_sim_execute(apk_sim *sim, const char *outdir, int *ncycles);

/* ---- field snapshots (csrc/host/snapshot.cpp, csrc/host/snapshot_format.cpp, csrc/kernels_output.hip) -----------------
 * A <parthenon/outputN> block with file_type = npy: dt (> 0), variables (comma separated, default cons),
 * single_precision_output (default false), id (default out<N>).  Entries of `variables`: the groups cons and prim; single
 * components cons.rho, cons.mom1..3, cons.etot, cons.B1..3, cons.psi, cons.s<n>, prim.rho, prim.vel1..3, prim.pressure,
 * prim.B1..3, prim.psi, prim.r<n>; the derived fields temperature, mach_sonic, B_mag, mach_alfven, plasma_beta
 * (apk_output_component in apk_amd.h; with every problem generator, where the reference has them for the cluster only).
 * Duplicates collapse, order is kept.  Refused at creation with a message naming block and key: an unknown entry, an MHD
 * component or MHD-only field with hydro/fluid = euler, temperature without <units> and hydro/He_mass_fraction, a scalar
 * index >= nscalars, dt <= 0, an empty list.  hdf5 blocks stay ignored; rst blocks are restart outputs (below).
 * A dump is <prefix>.rank<r>.npy on every rank -- NumPy format 1.0, shape (nblocks_local, ncomp, nx3, nx2, nx1) of the
 * meshblock, interior cells, '<f8' or '<f4', blocks in local order -- and <prefix>.json on rank 0: time, cycle, dt,
 * components, dtype, fluid, gamma, nscalars, xmin, xmax, mesh_nx, block_nx, nghost, nranks and blocks (gid, level, lx1,
 * lx2, lx3, rank, index = position in that rank's file), doubles as %.17g.  apk_sim_execute writes
 * <outdir>/<problem_id as for hst>.<id>.<NNNNN> from 00000: after initialisation, then when time >= next or on the last
 * cycle.  A dump packs the interior of the CURRENT conserved state on the sim's stream in chunks of whole blocks through a
 * device and a pinned host staging buffer of at most apk_amd/snapshot_staging_mb MB each (default 256; never less than
 * one block): no ghost zone is read, no stored primitive, nothing is exchanged and no driver state changes -- unlike
 * read_block / gather these are local calls, and a run that dumps takes the stage forms and exchanges of one that does
 * not.  `variables` below is such a comma-separated list. */
typedef struct apk_snapshot_output_info {
  int number;             /* N of <parthenon/outputN> */
  int single, ncomp;
  double dt;
  char id[64];
  char components[1024];  /* canonical names, comma separated */
} apk_snapshot_output_info;
/* the deck's snapshot outputs as parsed: copies min(n, size) entries, *size = their number.  Works on a host-only sim. */
int apk_sim_snapshot_outputs(const apk_sim *sim, apk_snapshot_output_info *out, int n, int *size);
/* what apk_sim_snapshot_read delivers for `variables`: local blocks, components, interior extents nx[3] = nx1, nx2, nx3 of
 * a block, bytes per item, and (names may be NULL) the canonical component names, comma separated.  Works on a host-only
 * sim. */
int apk_sim_snapshot_shape(apk_sim *sim, const char *variables, int single, int *nblocks, int *ncomp, int nx[3], int *itemsize,
                           char *names, size_t names_len);
/* packs the current state into out[nblocks][ncomp][nx3][nx2][nx1] (double or float); out_bytes must be that size */
int apk_sim_snapshot_read(apk_sim *sim, const char *variables, int single, void *out, size_t out_bytes);
/* one dump to <prefix>.rank<r>.npy (+ <prefix>.json on rank 0).  Every rank calls it; no rank waits for another. */
int apk_sim_write_snapshot(apk_sim *sim, const char *prefix, const char *variables, int single);
/* the JSON index alone, to `path`, with the sim's time, cycle and dt (a host-only sim: time 0, cycle 0) */
int apk_sim_write_snapshot_index(apk_sim *sim, const char *path, const char *variables, int single);
/* ---- restart (csrc/host/restart.cpp, csrc/host/restart_format.cpp, csrc/kernels_output.hip) ---------------------------
 * A <parthenon/outputN> block with file_type = rst: dt (> 0; missing or <= 0 is refused at creation naming block and key),
 * id (default out<N>).  apk_sim_execute writes <outdir>/<problem_id>.<id>.<NNNNN> at the cadence rule of the other
 * outputs and on the last cycle, not at t = 0.
 * A dump is the conserved state as a field snapshot of `cons` in double (<prefix>.rank<r>.npy on every rank,
 * <prefix>.json on rank 0: athenapk_amd.snapshots.load reads it) and the state file <prefix>.rst, which rank 0 writes
 * last -- to a temporary name, then renamed; with several ranks after a reduction all ranks take part in -- so that its
 * presence says the dump is complete.  The state file is text in the deck format: the deck as parsed with the overrides
 * applied, every block and key, plus the block <apk_amd/restart> -- format_version, time, cycle, dt, the package's dt_hyp,
 * mindx, c_h and dt_diff, the counters fofc_total, fofc_fallback_stages, zone_cycles, amr_refined and amr_derefined,
 * nranks, nblocks, fluid, nvar, nghost, refinement, mesh_nx, block_nx, one key block_<gid> = level lx1 lx2 lx3 deref_count
 * rank index per global block, the cluster problem's reduced quantities of AGN triggering with trig_rate, trig_time,
 * trig_dt and the five split_totals, and output<N>_next_time / output<N>_counter per hst, npy and rst block while
 * apk_sim_execute runs -- doubles as %.17g.  problem_id = turbulence adds accel_hat_<i>_<m>_r / _i, state_rng and
 * state_dist to <problem/turbulence> (the reference's restart parameters, src/pgen/turbulence.cpp:166-197); a deck that
 * carries them starts its driver from them.  Writing reads the interior of the current conserved state and changes
 * nothing: a run that writes dumps computes what one that does not computes, bit for bit.
 * apk_sim_restore takes the place of apk_sim_initialize on a sim created from the state file's text (which is a deck): it
 * checks mesh, meshblock, nghost, fluid, number of variables and refinement mode against the sim, installs the forest with
 * its derefinement counters on adaptive meshes (static forests are rebuilt from the deck and checked), moves the blocks
 * from whichever rank files hold them -- looked up by level and logical location, so a dump written on R ranks restores
 * on any number -- through the snapshots' pinned and device staging buffers (apk_amd/snapshot_staging_mb) into
 * apk_restart_unpack, sets the scalars and the turbulence driver, and runs the ghost exchange and FillDerived.  No time
 * step is estimated: dt, dt_hyp, mindx and c_h are the stored ones.  In the parity build the resumed run equals the
 * uninterrupted one bit for bit; in the product build it equals the uninterrupted run that calls apk_sim_exchange_ghosts
 * and apk_sim_fill_derived right after the dump (stage forms that derive primitives from the conserved state contract
 * differently from those that read stored ones).
 * Refused with a message naming the key: an rst block, apk_sim_write_restart or apk_sim_restore with tracers/enabled = true
 * (tracer arrays and lookback histories are not stored); a state file of another format_version; a deck that is a state
 * file with overrides that change mesh, meshblock, nghost, fluid, nscalars or refinement mode (at creation); restore on a
 * sim that has been initialised, stepped or restored.  A failed restore leaves a message and the process running.  Every
 * rank file the block table names is opened and checked (header, shape, size) on every rank before anything of the sim
 * changes: a restore refused for one of the reasons above, or for a missing, foreign or truncated file, leaves a sim that
 * may still be initialised or restored from another dump.  One that fails later (a block table that is no balanced
 * forest, a read error, a device error) leaves a sim to destroy.  apk_sim_write_restart reduces its status over the ranks:
 * if one rank cannot write its array, no state file is written and every rank reports the failure. */
typedef struct apk_restart_output_info {
  int number; /* N of <parthenon/outputN> */
  double dt;
  char id[64];
} apk_restart_output_info;
/* the deck's rst outputs as parsed: copies min(n, size) entries, *size = their number.  Works on a host-only sim. */
int apk_sim_restart_outputs(const apk_sim *sim, apk_restart_output_info *out, int n, int *size);
/* one dump to <prefix>.rank<r>.npy, <prefix>.json and <prefix>.rst.  Every rank calls it.  On a host-only sim: the state
 * file alone (time 0, cycle 0). */
int apk_sim_write_restart(apk_sim *sim, const char *prefix);
/* the state of the dump behind <prefix>.rst into a new sim, in place of apk_sim_initialize.  Every rank calls it. */
int apk_sim_restore(apk_sim *sim, const char *rst_path);
/* wall seconds of the main loop of the last apk_sim_execute (initialisation excluded, device
 * synchronised): zones * cycles / this = Parthenon's "zone-cycles/wallsecond" */
double apk_sim_loop_seconds(const apk_sim *sim);
/* cycles covered by apk_sim_loop_seconds: those after parthenon/time/perf_cycle_offset (default 0) */
int apk_sim_loop_cycles(const apk_sim *sim);
/* interior cells updated inside that timed loop, summed over its cycles (the block count of an
 * adaptive mesh changes from cycle to cycle): zone-cycles / wallsecond = this / loop_seconds */
long long apk_sim_loop_zone_cycles(const apk_sim *sim);
/* circularly polarised Alfven wave (job/problem_id = cpaw, 3-D): L1 errors against the initial state
 * and their RMS (src/pgen/cpaw.cpp:127-186; err8 = d, M1, M2, M3, E, B1, B2, B3), and the
 * reference's "cpaw-errors.dat" row (cpaw.cpp:188-220). */
int apk_sim_cpaw_errors(apk_sim *sim, double *rms, double *err8);
int apk_sim_write_cpaw_errors(apk_sim *sim, const char *path);
int apk_sim_linear_wave_errors(apk_sim *sim, double *rms, double *l1_5, double *max_5);
/* MHD linear waves (job/problem_id = linear_wave_mhd, src/pgen/linear_wave_mhd.cpp: the seven wave families of
 * adiabatic MHD on a magnetised background, wave_flag 0..6 = fast-, Alfven-, slow-, entropy, slow+, Alfven+, fast+;
 * B = curl A of the cell-centred potential :370-441): L1 / max errors of d, M1, M2, M3, E, B1, B2, B3 against the
 * analytic wave and their RMS (:177-276).  apk_sim_write_linear_wave_errors writes this problem's 8-column row. */
int apk_sim_linear_wave_mhd_errors(apk_sim *sim, double *rms, double *l1_8, double *max_8);
/* individual driver steps, exposed for tests */
int apk_sim_exchange_ghosts(apk_sim *sim);
int apk_sim_fill_derived(apk_sim *sim);
int apk_sim_estimate_timestep(apk_sim *sim, double *dt);
/* after replacing the state through apk_sim_write_block (+ exchange_ghosts + fill_derived): derive the time step
 * as apk_sim_initialize does after the problem generator (no growth limit from earlier steps) */
int apk_sim_reset_time_step(apk_sim *sim);

/* kernel timing of the sim's hot-path handle (apk_kernel_timing_* of apk_amd.h) */
int apk_sim_kernel_timing_enable(apk_sim *sim, int on);
int apk_sim_kernel_timing_read(apk_sim *sim, int slot, double *total_ms, long long *launches);

/* ---- ghost-exchange plan introspection (host logic; valid in host-only mode) ----------- */
typedef struct apk_peer_info {
  int rank;
  int64_t send_count, recv_count; /* doubles */
  void *send_buf, *recv_buf;      /* device pointers (NULL in host-only mode) */
} apk_peer_info;
int apk_sim_peer(const apk_sim *sim, int p, apk_peer_info *info);
/* The message set the next comm_ops.exchange moves.  On uniform meshes it never changes (the halo
 * buffers; apk_sim_info.npeers entries).  On refined meshes the driver makes the halo, the
 * flux-correction or the regridding messages current before it calls exchange, and regridding
 * changes peers, sizes and buffers: an exchange callback re-reads the set whenever
 * apk_sim_message_generation has changed since it last looked. */
int apk_sim_num_peers(const apk_sim *sim);
/* introspection: report the halo (1) / flux-correction (2) message set of a refined mesh through
 * apk_sim_peer (0 = the uniform mesh's set); 3 / 4: the halo sets of the faces-only and of the shell
 * exchange of the stage loop; 5 = the one-layer set of a uniform mesh (apk_sim_set_thin_exchange) */
int apk_sim_select_messages(apk_sim *sim, int which);
long long apk_sim_message_generation(const apk_sim *sim);
/* number of box copies in each phase: 0 local, 1 pack, 2 unpack, 3..5 physical BC x1..x3, 6 / 7 pack / unpack of the
 * one-layer exchange; on
 * refined meshes 10 = all copies of the multilevel exchange, 11..13 = coarse-buffer boundaries,
 * 14..16 = block boundaries, 17..19 = flux-correction copies x1..x3 (10..19: the global plan
 * every rank builds, global block numbers); this rank's share with local block numbers and message
 * buffers: 20 fill copies, 21 packs, 22 unpacks, 25..27 / 28..30 / 31..33 flux-correction copies /
 * packs / unpacks x1..x3, 34..36 coarse-buffer boundaries, 37..39 block boundaries; the exchanges of
 * the stage loop: 40..42 fill copies / packs / unpacks without the boxes behind edges and corners, 43
 * the copies of 40 without those between same-rank blocks of one level (the stages read these
 * neighbours through apk_stage_args.face_neighbor), 44..46 / 47..49 fill copies, packs, unpacks /
 * block boundaries of the exchange that fills every ghost zone two layers deep only (before a
 * refinement check), 50 the copies of 44 without those between same-rank blocks of one level */
int apk_sim_plan_size(const apk_sim *sim, int phase);
/* region r of a phase, with src/dst expressed as (kind, block, element offset):
 * kind 0 = local block cons, 1 = send buffer of peer `block`, 2 = recv buffer of peer `block`,
 * 3 = coarse buffer of the block, 4..6 = its x1..x3 flux array */
typedef struct apk_region_info {
  int src_kind, src_block, dst_kind, dst_block;
  int64_t src_off, dst_off;
  int ext[3], nvar, flip_var;
  int64_t src_stride[4], dst_stride[4];
} apk_region_info;
int apk_sim_plan_region(const apk_sim *sim, int phase, int r, apk_region_info *info);
/* operator lists of the multilevel exchange, in execution order restrict-own (which = 0) ->
 * phase 10 -> 11..13 -> prolongate (1) -> 14..16; flux correction: per direction d, which = 2 + d
 * then phase 17 + d.  which + 10 = this rank's share (local block numbers); 15 / 16: this rank's
 * prolongations of the faces-only and of the shell exchange.  kind is an APK_RO_* value; index boxes in
 * coarse-buffer indices. */
typedef struct apk_amr_op_info {
  int kind, level;
  int src_kind, src_block, dst_kind, dst_block;
  int lo[3], hi[3];
  double xmin[3], dx[3]; /* lower interior corner and cell widths of the block the operator works on */
  int cng;
  int64_t coarse_doubles; /* allocation of one coarse buffer */
} apk_amr_op_info;
int apk_sim_amr_ops_size(const apk_sim *sim, int which);
int apk_sim_amr_op(const apk_sim *sim, int which, int n, apk_amr_op_info *info);

#ifdef __cplusplus
}
#endif
#endif /* APK_HOST_H_ */
