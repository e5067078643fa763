/*
 * apk_amd.h -- C-ABI of the MI355X-native AthenaPK hot path (libapk_amd.so).
 *
 * Drop-in boundary: these entry points are what a Parthenon/AthenaPK build binds in place
 * of the Kokkos task functions of the flux-divergence update.  Every entry point cites
 * the reference interface (file:line under the AthenaPK tree) it replaces; the adapter a
 * maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; device memory is BORROWED for the duration of a call
 *    (Parthenon owns all field storage; src/hydro/hydro.cpp:777-786).
 *  - every call is asynchronous on the caller's HIP stream (`apk_stream_t` = hipStream_t
 *    cast to void*; NULL = default stream) unless it returns a host scalar.
 *  - return value: APK_OK (0) or a negative APK_ERR_* code.  Never throws, never aborts.
 *    Device-side "PARTHENON_REQUIRE" conditions (negative density / pressure in
 *    ConsToPrim, src/eos/adiabatic_hydro.hpp:77-79,111-113) are latched in a flag word
 *    read back with apk_poll_device_flags().
 *  - block field layout: [nvar][Nk][Nj][Ni] doubles, i fastest, Ni = nx1 + 2*ng (no
 *    ghosts in a collapsed dimension); flux(d, v, k, j, i) is the flux through the LOWER
 *    d-face of cell (k,j,i)  (SURVEY.md 8, App. A.5).
 *  - variable order: cons (rho, m1, m2, m3, E [,B1,B2,B3,psi], scalars...),
 *    prim (rho, v1, v2, v3, p [,B1,B2,B3,psi], scalars...)   src/main.hpp:19-33
 */
#ifndef APK_AMD_H_
#define APK_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APK_AMD_VERSION 1

/* ---- option enums: numeric values = position in the reference's enum classes,
 *      src/main.hpp:35-38 ---- */
enum apk_riemann { APK_RS_UNDEFINED = 0, APK_RS_NONE = 1, APK_RS_HLLE = 2, APK_RS_LLF = 3,
                   APK_RS_HLLC = 4, APK_RS_HLLD = 5 };
enum apk_recon { APK_RC_UNDEFINED = 0, APK_RC_DC = 1, APK_RC_PLM = 2, APK_RC_PPM = 3,
                 APK_RC_WENOZ = 4, APK_RC_WENO3 = 5, APK_RC_LIMO3 = 6 };
enum apk_integrator { APK_INT_UNDEFINED = 0, APK_INT_RK1 = 1, APK_INT_RK2 = 2,
                      APK_INT_VL2 = 3, APK_INT_RK3 = 4 };
enum apk_fluid { APK_FLUID_UNDEFINED = 0, APK_FLUID_EULER = 1, APK_FLUID_GLMMHD = 2 };

enum apk_status {
  APK_OK = 0,
  APK_ERR_INVALID = -1,      /* bad argument / inconsistent pack */
  APK_ERR_UNSUPPORTED = -2,  /* (fluid,recon,riemann) not in the registry, hydro.cpp:386-416 */
  APK_ERR_NGHOST = -3,       /* too few ghost zones for the reconstruction, hydro.cpp:444-447 */
  APK_ERR_DEVICE = -4,       /* HIP runtime error (see apk_last_error) */
  APK_ERR_NO_DEVICE = -5     /* no HIP device / extension not usable: fail loudly */
};

/* device flag bits latched by kernels (apk_poll_device_flags) */
#define APK_FLAG_NEG_DENSITY 1u
#define APK_FLAG_NEG_PRESSURE 2u
/* tabular cooling: the reference's device failures (PARTHENON_FAIL / REQUIRE), latched instead of trapping */
#define APK_FLAG_COOL_MAX_ITER 4u /* "Sub cycles exceed max_iter", tabular_cooling.cpp:375-380 */
#define APK_FLAG_COOL_TABLE 8u    /* "Failed to find log_temp", tabular_cooling.hpp:155-156 */
/* AGN feedback: "Kinetic injection leads to negative pressure" (agn_feedback.cpp:407-408), latched instead of trapping */
#define APK_FLAG_AGN_NEG_PRESSURE 16u

typedef void *apk_stream_t; /* hipStream_t */

/* AdiabaticHydroEOS / AdiabaticGLMMHDEOS parameters: src/eos/eos.hpp:33-61,
 * defaults src/hydro/hydro.cpp:507-537 (floors <= 0 disabled, ceilings +inf disabled) */
typedef struct apk_eos {
  double gamma;
  double pfloor, dfloor, efloor;
  double vceil, eceil;
} apk_eos;

/* what CalculateFluxes is templated on: src/hydro/hydro.hpp:43-46,53 (FluxFunKey_t) */
typedef struct apk_flux_cfg {
  int fluid;   /* apk_fluid */
  int recon;   /* apk_recon */
  int riemann; /* apk_riemann */
} apk_flux_cfg;

/* one meshblock of a MeshBlockPack: what `pack(b)(v,k,j,i)`, `pack(b).flux(d,v,k,j,i)`
 * and `pack.GetCoords(b).Dxc<d>()` resolve to (src/hydro/hydro.cpp:1041-1073).
 * All pointers are DEVICE pointers; flux[d] may be NULL if the caller only uses the fused
 * stage path (or for inactive dimensions). */
typedef struct apk_block_desc {
  double *cons;
  double *prim;
  double *flux[3];
  double dx[3];
} apk_block_desc;

/* MeshData / MeshBlockPack: src/hydro/hydro.cpp:1026-1063 */
typedef struct apk_pack_desc {
  int nblocks;  /* cons_in.GetDim(5) */
  int nhydro;   /* pkg->Param<int>("nhydro"): 5 or 9 */
  int nscalars; /* pkg->Param<int>("nscalars") */
  int nx[3];    /* block_size.nx(X1DIR..X3DIR); 1 = collapsed dimension */
  int ng;       /* parthenon/mesh/nghost */
  const apk_block_desc *blocks; /* HOST array [nblocks] */
  /* Element strides of the j, k and variable index of every array of the pack (cons, prim, flux): `pack(b)(v,k,j,i)` is
   * base[v * stride[2] + k * stride[1] + j * stride[0] + i] -- the reference's accessor is stride-agnostic
   * (src/hydro/hydro.cpp:1041-1073), Parthenon's allocations are LayoutRight.  0 = that natural layout:
   * Ni, Ni * Nj, Ni * Nj * Nk with Ni = nx[0] + 2 ng etc.  Anything else must satisfy stride[0] >= Ni,
   * stride[1] >= stride[0] * Nj, stride[2] >= stride[1] * Nk (and be the same for every block).  What it is for: rows
   * at a pitch that is a multiple of a cache line (16 doubles) from a base chosen so that the first INTERIOR cell of a
   * row sits on a line boundary -- the stage kernels then load and store the 128-cell rows of a 128^3 block as 8 whole
   * lines instead of 9 - 10 partial ones (the standalone driver: apk_amd/row_pitch = aligned). */
  int64_t stride[3];
} apk_pack_desc;

typedef struct apk_ctx apk_ctx;   /* workspace: flag words, reduction scratch */
typedef struct apk_pack apk_pack; /* device-resident copy of an apk_pack_desc */

/* ---- lifetime ---------------------------------------------------------------------- */
/* Creates the workspace on the CURRENT HIP device.  Fails with APK_ERR_NO_DEVICE when no
 * gfx950-capable device is visible: there is no CPU fallback. */
int apk_create(apk_ctx **out);
void apk_destroy(apk_ctx *ctx);
const char *apk_last_error(const apk_ctx *ctx);
int apk_version(void);
/* 1 if this library was built with -ffp-contract=off (bit-parity build), else 0 */
int apk_fp_strict(void);
/* Measurement aid of bench.py (no counterpart in the reference): the issue floor of the GLM-MHD PPM + HLLD scheme on this
 * device -- `steps` sweep steps (nine PPM reconstructions + one HLLD solve per lane, nothing else: no global memory, no
 * limiter block entered) in every lane of two waves per SIMD, `reps` launches timed with events on the null stream.
 * A cell-stage of the 3-D scheme is three such steps per cell. */
int apk_bench_scheme_floor(int steps, int reps, double *ms_per_launch, long long *lane_steps_per_launch);

/* Uploads the descriptors (tiny H2D copy, synchronous).  Rebuild after remeshing, like
 * Parthenon rebuilds its packs. */
int apk_pack_create(apk_ctx *ctx, const apk_pack_desc *desc, apk_pack **out);
void apk_pack_destroy(apk_pack *pack);

/* ---- the hot path ------------------------------------------------------------------- */

/* Replaces Hydro::CalculateFluxes<fluid,recon,rsolver>(std::shared_ptr<MeshData<Real>>&)
 * src/hydro/hydro.cpp:1025-1208 (type FluxFun_t, hydro.hpp:43-46; registry
 * hydro.cpp:386-416; (dc,llf) maps to CalculateFluxesTight hydro.cpp:980-1022).
 * Reads prim, writes flux[d] over the reference's loop extents. */
int apk_calculate_fluxes(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg,
                         const apk_eos *eos, double c_h, apk_stream_t stream);
/* The same fluxes on the faces of interior cells only (the loop limits of CalculateFluxesTight,
 * hydro.cpp:1006-1009).  The reference's sweeps also cover one transverse ghost row / plane
 * (hydro.cpp:1031-1039), which neither the flux divergence, the first-order flux correction nor
 * the coarse-fine flux correction consume: 27 % of the faces of a 16^3 meshblock, 56 % of an 8^3. */
int apk_calculate_fluxes_tight(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg,
                               const apk_eos *eos, double c_h, apk_stream_t stream);
/* Only the faces on the boundary of each meshblock (two planes per active direction, interior
 * transverse extent): what the coarse-fine flux correction needs when the stage itself ran fused
 * (apk_stage_fused never materialises face fluxes; see apk_flux_fix_plan below). */
int apk_calculate_fluxes_boundary(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg,
                                  const apk_eos *eos, double c_h, apk_stream_t stream);
/* The same for a DEVICE list of (block, face) pairs only, in ONE launch (the input of the coarse-fine flux
 * correction, hydro_driver.cpp:527-531, when the stage ran fused): faces[n] = 6 * block + face,
 * face = {x1 lower, x1 upper, x2 lower, x2 upper, x3 lower, x3 upper} -- on a refined mesh the faces
 * with a coarser or finer block behind them (the fine side's fluxes are averaged, the coarse side's own
 * flux is what the average replaces); the planes of unlisted faces are left untouched. */
int apk_calculate_fluxes_boundary_list(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                                       double c_h, const int *faces, int nfaces, apk_stream_t stream);
/* The same with the stencil cells taken from the CONSERVED state and converted in registers (the ConsToPrim the pass
 * over the blocks applies, adiabatic_hydro.hpp:61-169, without its floor / ceiling blocks: eos without dfloor, efloor,
 * pfloor, vceil, eceil only -- APK_ERR_UNSUPPORTED otherwise; no passive scalars): for cycles of a refined mesh whose
 * stages derive their input from the conserved state (apk_stage_args.prim_from_cons) and store no primitives.
 * cons_delta: offset in doubles from a block's `cons` array of the pack to the array that holds the input state (0: the
 * pack's own -- the stage's u0 --; the distance to u1's array for a stage whose input is u1). */
int apk_calculate_fluxes_boundary_list_from_cons(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                                                 double c_h, const int *faces, int nfaces, long long cons_delta,
                                                 apk_stream_t stream);

/* Replaces parthenon::Update::UpdateWithFluxDivergence<MeshData<Real>>(u0,u1,gam0,gam1,
 * beta_dt); call site src/hydro/hydro_driver.cpp:534-537.
 * u0.cons <- gam0*u0.cons + gam1*u1.cons + beta_dt * (-div F(u0.flux)) on interior cells. */
int apk_update_with_flux_divergence(apk_ctx *ctx, const apk_pack *u0, const apk_pack *u1,
                                    double gam0, double gam1, double beta_dt,
                                    apk_stream_t stream);

/* Replaces GLMMHD::DednerSource<extended>(MeshData<Real>*, Real beta_dt)
 * src/hydro/glmmhd/dedner_source.cpp:17-75 (called through Hydro::AddUnsplitSources,
 * src/hydro/hydro.cpp:227-246).  c_h, mindx, alpha are the package params of
 * dedner_source.cpp:27-29. */
int apk_dedner_source(apk_ctx *ctx, const apk_pack *md, int extended, double alpha,
                      double c_h, double mindx, double beta_dt, apk_stream_t stream);

/* Fused fast path for one RK stage of one pack = CalculateFluxes -> UpdateWithFlux-
 * Divergence -> DednerSource (hydro_driver.cpp:510-544) without materialising the flux
 * arrays in HBM.  Not usable when first-order flux correction or AMR flux correction needs
 * the face fluxes.  u1 may alias u0 only if gam1 == 0. */
/* x1 strips of a halo exchange that pass through no pack / unpack kernel (apk_stage_args.x1_halo).  The reference
 * fills every ghost zone through boundary buffers (hydro_driver.cpp:506-569 SendBoundBufs / ReceiveBoundBufs / SetBounds);
 * a row of an x1 strip is nghost doubles -- 24 of every 128-byte line a copy kernel fetches from, or writes into, a block.
 * Here the stage kernels go to the buffers themselves:
 *   recv[side]  the buffer segment holding the ghost columns behind the block's lower (0) / upper (1) x1 face: the stage
 *               reads those columns from there instead of the block's ghost zone.  NULL: the ghost zone (or the block
 *               face_neighbor names).
 *   send[side]  the buffer segment the stage ALSO stores the interior columns next to that face into, as it retires
 *               them.  NULL: nothing.
 * A segment is [nvar][nx3][nx2][depth] doubles, `depth` columns in x1 order over the interior extent in x2 and x3 (the
 * ghost columns is-depth..is-1 / ie+1..ie+depth, the interior columns is..is+depth-1 / ie-depth+1..ie): the layout of an
 * x1-face segment of the standalone driver's messages.  recv_depth < nghost: the deeper ghost columns are read from the
 * block as usual.  Needs nx1 >= 2 send_depth.  send_field: 0 = the updated conserved state, 1 = the new primitives
 * (needs fill_derived = 1 or 2).  Honoured by the stage forms apk_stage_x1_halo() reports; others refuse
 * (APK_ERR_UNSUPPORTED). */
typedef struct apk_x1_halo_block {
  const double *recv[2];
  double *send[2];
} apk_x1_halo_block;
typedef struct apk_x1_halo {
  const apk_x1_halo_block *blocks; /* DEVICE array, one entry per block of the pack */
  int recv_depth, send_depth;      /* columns per segment row (0: no segment of that kind is used) */
  int send_field;
} apk_x1_halo;

typedef struct apk_stage_args {
  apk_flux_cfg cfg;
  apk_eos eos;
  double c_h;
  double gam0, gam1, beta_dt; /* integrator->gam0/gam1/beta[stage-1]*dt */
  int dedner;                 /* 0 = off (euler), 1 = plain, 2 = extended */
  double glmmhd_alpha, mindx;
  /* Optional: let the finishing sweep also do the work of the NEXT two tasks on the cells it
   * updates, saving two passes over the interior:
   *  fill_derived = 1: apply ConsToPrim (floors included) and store prim in place
   *                    (Update::FillDerived, hydro_driver.cpp:571-577).  The caller then only
   *                    needs apk_cons_to_prim_ghosts() after the ghost exchange.  Not in 1-D,
   *                    not with dedner == 2 (APK_ERR_UNSUPPORTED).
   *  fill_derived = 2: the same (dedner == 2 allowed), but the new primitives are written into u1's prim arrays
   *                    ("u1.prim", which AthenaPK also carries: hydro_driver.cpp:484-493) and
   *                    u0's are left untouched; the caller swaps the roles of the two prim
   *                    arrays afterwards.  This is what lets a 3-D donor-cell stage (the VL2
   *                    predictor) run as a single march with no flux-difference array at all.
   *  estimate_dt  = 1: (needs fill_derived) also min-reduce dx_d/(|v_d|+c_d) over those cells
   *                    (EstimateHyperbolicTimestep, hydro.cpp:828-896); read it with
   *                    apk_stage_dt_read(). */
  int fill_derived;
  int estimate_dt;
  /* Optional: split the stage around a halo exchange that is still in flight (2-D / 3-D).  Work
   * that does not read the ghost zones still in flight runs first on per-block index windows:
   *  phase = 0   the whole stage (window must be NULL)
   *  phase = 1   partial work restricted per block by `window`, a DEVICE array of 8 ints per block
   *              {i0, rl, ilo, ihi, jlo, jhi, klo, khi}: rows jlo..jhi of planes klo..khi are
   *              flattened with rl columns starting at column i0 and only the cells ilo..ihi of a
   *              row are updated ({0, Ni, is, ie, js, je, ks, ke} is the whole block; rl = 0 skips
   *              the block).  May be called several times with disjoint windows whose union covers
   *              every interior cell exactly once.  An x1-sweep window must start two columns
   *              below ilo and end one above ihi (i0 <= ilo - 2, i0 + rl - 1 >= ihi + 1): the
   *              sweep hands states / PPM interface values from lane to lane.
   *                - stages whose x1 sweep is its own kernel (reconstruction other than dc): the
   *                  x1 sweep only (it reads x1 ghost zones only); j/k ranges must be the full
   *                  interior.  estimate_dt / fill_derived take effect in phase 2.
   *                - 3-D donor-cell stages (one kernel for the whole stage): the whole stage on the
   *                  window; estimate_dt is not available in this mode.
   *  phase = 2   the remaining sweeps (x2 [, x3], update, sources, fill_derived, dt); nothing for
   *              3-D donor-cell stages.
   * window_rl / window_rows: the largest rl and (jhi - jlo + 1) in `window` (size the launch). */
  int phase;
  const int *window;
  int window_rl, window_rows;
  /* trial = 1: the caller may discard this stage's result (the optimistic stage of first-order
   * flux correction): the negative-density / -pressure flags its FillDerived latches go to a
   * separate trial word, which apk_trial_flags() merges into the latched word (keep = 1) or drops
   * (keep = 0).  Flags latched by earlier kernels are never touched by a discarded stage. */
  int trial;
  /* count_unphysical = 1: the finishing sweep also applies FirstOrderFluxCorrect's admissibility
   * test (hydro.cpp:1297-1306: rho <= 0 or E - KE [- ME] <= 0) to every updated cell BEFORE any
   * floor acts (and, with fill_derived, counts cells whose ConsToPrim latched a flag); read the
   * number of failing cells with apk_stage_unphysical_read().  Not with passive scalars. */
  int count_unphysical;
  /* cons_out_delta != 0: the updated conserved state is written to cons + cons_out_delta (in
   * elements, the same offset for every block: a second allocation of identical layout) instead of
   * over u0, which stays intact -- the trial stage of first-order flux correction when gam0 != 0
   * (RK2 / RK3 later stages), whose fallback needs the old u0.  Interior cells only; not with
   * passive scalars. */
  int64_t cons_out_delta;
  /* face_neighbor != NULL: direct neighbour addressing.  A DEVICE array of 6 ints per block of the
   * pack {x1 lower, x1 upper, x2 lower, x2 upper, x3 lower, x3 upper}: the pack index of the block
   * of the same size behind that face whose INTERIOR stands in for this block's ghost zone there,
   * or -1 to read the ghost zone itself (a physical boundary, a neighbour on another rank).  With
   * it the same-rank ghost-zone copies of a uniform mesh -- 11 % of a VL2 cycle on 8 x 128^3 --
   * are not needed at all: the reference fills every ghost zone through boundary buffers
   * (hydro_driver.cpp:506-569 SendBoundBufs / SetBounds), the stage kernels here follow the table.
   * Only the face neighbours are read (the unsplit sweeps never touch edge or corner ghost cells);
   * the ghost zones behind faces with an entry >= 0 are neither read nor written.  3-D only, for the
   * stage forms whose kernels follow the table: donor cell (single march, fill_derived 0 or 2) and
   * the two-kernel stage (apk_stage_split_axis() == 3); not with passive scalars nor dedner = 2
   * (APK_ERR_UNSUPPORTED). */
  const int *face_neighbor;
  /* cons_store: which cells of the updated CONSERVED state the stage must leave in memory.
   *   0  every interior cell (the reference's semantics).
   *   1  only the cells within nghost layers of a face of their meshblock -- what ghost-zone copies, message packing
   *      and physical boundary conditions read.
   *   2  none.
   * For a stage whose conserved result nobody reads in full: the predictor of VL2, whose corrector has gam0 = 0 and
   * takes its fluxes from the predictor's PRIMITIVES (fill_derived = 2) -- the half-step conserved state is then
   * dead but for the strips the exchange reads (1), or altogether when every neighbour is read directly through
   * face_neighbor (2): 72 of the 288 bytes the donor-cell stage moves per cell, and that stage runs at the memory
   * system's rate.  Honoured by the 3-D single-march donor-cell stage in its lean form; every other stage form
   * stores all cells (always a valid reading of 1 and 2).  The cells not stored keep whatever they held. */
  int cons_store;
  /* prim_from_cons = 1: u0.prim does NOT hold the primitives of the stage's input state; the kernel derives them from
   * u1.cons, which must be that state (true in stage 1 of every integrator: u1 = u0 there, hydro_driver.cpp:474-495).
   * The single-march 3-D donor-cell stage and the two-kernel 3-D stage, in their lean forms only (else
   * APK_ERR_UNSUPPORTED).  Together with fill_derived = 3 in the last stage of the previous cycle it removes the
   * full-step primitives from memory altogether: 72 B per cell less to store there and 72 B less to load here, both on
   * kernels that run at the memory system's rate.
   * prim_from_cons = 2 (two-kernel stage): the input state is u0.cons itself -- the stages with gam0 != 0 of RK2 / RK3,
   * whose input is the state they update.  Neighbouring waves read the old values while a wave writes new ones, so the
   * result must go elsewhere: cons_out_delta != 0 is required.  With 1 / 2 in every stage and fill_derived = 0 (3 in the
   * last) an RK integrator keeps no primitives in memory at all.
   * fill_derived = 3 (listed here, with estimate_dt = 1): ConsToPrim of the updated cells for the time-step estimate
   * only; neither u0.prim nor u1.prim is written.  Two-kernel 3-D stage in its lean form only. */
  int prim_from_cons;
  /* x1 strips straight from / into exchange buffers (see apk_x1_halo above), or NULL.  Whole stages only (phase 0 or 2). */
  const apk_x1_halo *x1_halo;
} apk_stage_args;
int apk_stage_fused(apk_ctx *ctx, const apk_pack *u0, const apk_pack *u1,
                    const apk_stage_args *args, apk_stream_t stream);
/* Which ghost zones phase 1 of a split stage does NOT need, i.e. how its windows are laid out:
 *   1  the x1 sweep is its own kernel: column windows, late x1 faces matter (see `phase` above)
 *   3  two-kernel stage (3-D, reconstruction with a stencil, fill_derived 0 or 2, meshblocks at
 *      least 32 cells wide): phase 1 is the x3 sweep, which writes its flux difference and reads x3
 *      ghost zones only -- windows {0, Ni, is, ie, js, je, klo, khi} select whole planes klo..khi,
 *      late x3 faces matter; phase 2 is ONE march doing x1 + x2 and finishing the stage
 *   0  3-D donor-cell stage: one kernel for the whole stage, 3-D index windows
 * The two-kernel form moves 8.6 GB instead of 13.2 GB per PPM + HLLD stage of 8 x 128^3. */
/* number of cells that failed the test of the last apk_stage_fused(count_unphysical = 1);
 * synchronises the stream */
int apk_stage_unphysical_read(apk_ctx *ctx, long long *count, apk_stream_t stream);
int apk_stage_split_axis(const apk_pack *u0, const apk_flux_cfg *cfg, int fill_derived);
/* 1 if a whole-block stage of this scheme with these options follows apk_stage_args.x1_halo: the lean two-row donor-cell
 * march (3-D, fill_derived 0 / 2, nx2 even) and the lean two-kernel stage's finishing march -- from stored primitives or
 * (prim_from_cons != 0) from a conserved state, but not the stages that take the single march (apk_stage_single_march) --
 * without passive scalars (donor cell with prim_from_cons = 2, which apk_stage_fused refuses, answers 0).  A caller checks
 * BEFORE it leaves x1 strips out of its pack / unpack plans. */
int apk_stage_x1_halo(const apk_pack *u0, const apk_flux_cfg *cfg, const apk_eos *eos, int fill_derived, int dedner, int prim_from_cons);
/* 1 if a whole-block stage of this scheme in its lean form with prim_from_cons != 0 runs as ONE march (hydro with PLM:
 * x1 by wave shifts, two x2 rows per lane, x3 carried along the march -- no flux-difference array; the three tasks
 * hydro.cpp:1025-1208 + hydro_driver.cpp:534-544 in a single pass over the conserved state), 0 if it takes the two-kernel
 * form.  A split stage (phase != 0) always takes the two kernels: a caller that can choose leaves such a stage whole. */
int apk_stage_single_march(const apk_pack *u0, const apk_flux_cfg *cfg);
/* Which kernel form a stage takes, decided on the host from the pack's shape and the arguments alone: no context, no
 * device.  Returns what apk_stage_fused() would return for `args` on packs of this shape, as far as shape and arguments
 * decide it (APK_OK, or the code of the refusal), and fills `out`: the form, the lean level of its kernels (0 general,
 * 1 lean, 2 lean with the pressure floor / trial count), the x2 rows per lane of the donor-cell march (1 or 2, else 0),
 * the input its kernels convert (0, or prim_from_cons), whether they follow x1_halo, and -- of a refusal -- a short
 * sentence naming the rule that refused (a static string; "" otherwise).  shape->blocks is not read; of args->window,
 * face_neighbor and x1_halo->blocks only whether they are NULL. */
enum apk_stage_form_kind {
  APK_FORM_NONE = 0,         /* refused */
  APK_FORM_X1 = 1,           /* 1-D: the finishing x1 sweep */
  APK_FORM_X1_X2 = 2,        /* 2-D: x1 sweep, finishing x2 march */
  APK_FORM_THREE_SWEEP = 3,  /* 3-D: x1 sweep, x2 march, finishing x3 march */
  APK_FORM_MARCH12_X3 = 4,   /* 3-D donor cell with FillDerived in place: x1 + x2 in one march, finishing x3 march */
  APK_FORM_DC_MARCH = 5,     /* 3-D donor cell: the whole stage in one march, one or two x2 rows per lane */
  APK_FORM_TWO_KERNEL = 6,   /* 3-D: x3 sweep, then one finishing x1 + x2 march (apk_stage_split_axis() == 3) */
  APK_FORM_SINGLE_MARCH = 7  /* 3-D hydro PLM from a conserved state: the whole stage in one march (apk_stage_single_march) */
};
typedef struct apk_stage_form_info {
  int form; /* apk_stage_form_kind */
  int lean;
  int dc_rows;
  int from_cons;
  int x1_halo;
  const char *reason;
} apk_stage_form_info;
int apk_stage_form(const apk_pack_desc *shape, const apk_stage_args *args, apk_stage_form_info *out);

/* Replaces EquationOfState::ConservedToPrimitive(MeshData<Real>*) over the ENTIRE block
 * src/eos/adiabatic_hydro.cpp:33-55, adiabatic_glmmhd.cpp:33-56 (pkg->FillDerivedMesh,
 * src/hydro/hydro.cpp:705-713). */
int apk_cons_to_prim(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                     apk_stream_t stream);

/* apk_cons_to_prim() of every cell and, in the same pass, EstimateHyperbolicTimestep (hydro.cpp:828-896) of the
 * interior cells from the primitives it has just computed: the last FillDerived of a cycle and the time-step
 * estimate that follows it (hydro_driver.cpp:571-603) as one kernel.  The minimum goes to the context's stage
 * word: read it (times cfl) with apk_stage_dt_read() / apk_stage_dt_flags_read(), as after
 * apk_stage_fused(estimate_dt = 1).  ghost_depth < 0: every cell; >= 0: the interior and the ghost cells at
 * most that many layers outside it (edges and corners included) -- the shell a shallow ghost exchange has
 * filled; primitives further out are left as they were. */
int apk_cons_to_prim_dt(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, int ghost_depth, apk_stream_t stream);
/* ... leaving out the ghost cells straight behind a face whose entry in face_neighbor (device, [nblocks][6], or NULL) is
 * >= 0: zones an exchange that follows the face table has not filled and no reader of the table visits. */
int apk_cons_to_prim_dt_skip(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, int ghost_depth,
                             const int *face_neighbor, apk_stream_t stream);
/* ... storing only the primitives whose bit is set in store_vars (bit n = primitive n of the reference's order: IDN,
 * IV1, IV2, IV3, IPR [, IB1, IB2, IB3, IPS]; 0: none -- the time-step estimate alone; every bit: apk_cons_to_prim_dt_skip):
 * the end of a cycle whose successor derives its input from the conserved state (apk_stage_args.prim_from_cons) and
 * whose only reader of stored primitives is a refinement criterion -- the pressure for pressure_gradient, the two
 * velocities for xyvelocity_gradient, the density for maxdensity (apk_tag_blocks).  ghost_depth >= 0 (0: the interior).
 * Without floors and ceilings in eos (they write conserved values back that belong with all primitives of a cell:
 * APK_ERR_UNSUPPORTED), packs without passive scalars. */
int apk_cons_to_prim_dt_select(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, int ghost_depth,
                               const int *face_neighbor, unsigned store_vars, apk_stream_t stream);
/* ConsToPrim (Update::FillDerived, hydro_driver.cpp:571-577; src/eos/adiabatic_hydro.cpp:33) of the interior
 * and of the ghost cells straight behind a block FACE only (at most one ghost coordinate): what the unsplit
 * sweeps (hydro.cpp:1025-1199) and the flux correction read.  The refined-mesh stage loop of the standalone
 * driver fills and converts only those (edges and corners are 37 % of the ghost cells of a 16^3 block with
 * nghost = 4); primitives behind edges and corners are left as they were.  (The tagging criteria,
 * refinement/gradient.cpp:33-36, DO read behind edges and corners: a cycle that ends with a refinement check
 * exchanges and converts in full.) */
int apk_cons_to_prim_faces(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, apk_stream_t stream);
/* The same, leaving alone the ghost zone behind every face f of block b with face_neighbor[6 b + f] >= 0
 * (apk_stage_args.face_neighbor: the stages read that neighbour's interior instead, so nobody fills or
 * converts the zone).  face_neighbor: device pointer, [nblocks][6]. */
int apk_cons_to_prim_faces_skip(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const int *face_neighbor,
                                apk_stream_t stream);
/* apk_cons_to_prim_faces() / apk_cons_to_prim_faces_skip() (face_neighbor may be NULL) with the time-step
 * estimate of the interior cells reduced on the way, as apk_cons_to_prim_dt() does: the last stage of a
 * refined-mesh cycle that is not followed by a refinement check. */
int apk_cons_to_prim_faces_dt(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const int *face_neighbor,
                              apk_stream_t stream);
/* ConsToPrim restricted to the ghost zones of every block (interior cells untouched): the
 * companion of apk_stage_fused(fill_derived = 1). */
int apk_cons_to_prim_ghosts(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                            apk_stream_t stream);
/* The same in two parts around a halo exchange that is still in flight (see
 * apk_stage_args.phase).  late_regions: DEVICE array, one word per block; bit
 * (sx+1) + 3 (sy+1) + 9 (sz+1) set when the ghost region towards the neighbour at block offset
 * (sx, sy, sz) is only filled when the exchange completes (neighbour on another rank, physical
 * boundary).  part = 1 converts the ghost cells of the other regions (same-rank copies, ready
 * early), part = 2 those. */
int apk_cons_to_prim_ghosts_split(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                                  const unsigned *late_regions, int part, apk_stream_t stream);

/* Result of the last apk_stage_fused(estimate_dt = 1) on this context: *dt_out = cfl * min.
 * Synchronises `stream`. */
int apk_stage_dt_read(apk_ctx *ctx, double cfl, double *dt_out, apk_stream_t stream);
/* apk_stage_dt_read + apk_poll_device_flags with ONE synchronisation (the per-cycle host round
 * trip of a driver: new dt and the latched negative-density / -pressure flags).  CONSUMES the reduction: the device word
 * goes back to +max for the next one (on every platform); the handle remembers the minimum, and repeated calls -- or an
 * apk_stage_dt_read after it -- return the same value until the next stage / ConsToPrim with a time-step estimate starts
 * a new reduction. */
int apk_stage_dt_flags_read(apk_ctx *ctx, double cfl, double *dt_out, unsigned *flags,
                            apk_stream_t stream);

/* Replaces Hydro::EstimateHyperbolicTimestep<fluid>(MeshData<Real>*)
 * src/hydro/hydro.cpp:828-910.  Synchronises `stream`; *dt_out = cfl * min(...). */
int apk_estimate_timestep(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                          double cfl, double *dt_out, apk_stream_t stream);

/* ---- diffusion: fluxes and time step (diffusion/integrator = unsplit | rkl2) -----------------------------------------------------------
 * Option enums: numeric values = position in the reference's enum classes, src/main.hpp:40-46. */
enum apk_conduction { APK_COND_NONE = 0, APK_COND_ISOTROPIC = 1, APK_COND_ANISOTROPIC = 2 };
enum apk_conduction_coeff { APK_CONDC_NONE = 0, APK_CONDC_FIXED = 1, APK_CONDC_SPITZER = 2 };
enum apk_viscosity { APK_VISC_NONE = 0, APK_VISC_ISOTROPIC = 1 };
enum apk_viscosity_coeff { APK_VISCC_NONE = 0, APK_VISCC_FIXED = 1 };
enum apk_resistivity { APK_RES_NONE = 0, APK_RES_OHMIC = 1 };
enum apk_resistivity_coeff { APK_RESC_NONE = 0, APK_RESC_FIXED = 1, APK_RESC_SPITZER = 2 };
enum apk_diffint { APK_DIFFINT_NONE = 0, APK_DIFFINT_UNSPLIT = 1, APK_DIFFINT_RKL2 = 2 };

/* The "Hydro" params of the diffusive processes (hydro.cpp:538-702): the ThermalDiffusivity, MomentumDiffusivity and
 * OhmicDiffusivity objects with a fixed coefficient, and conduction_sat_prefac (5 * diffusion/conduction_sat_phi for a
 * fixed coefficient, 6.86 * sqrt(mu) * phi for Spitzer, hydro.cpp:589-604).  A process set to *_NONE is off.  The entry
 * points that take this struct alone are the fixed-coefficient ones: conduction_coeff = APK_CONDC_SPITZER is
 * APK_ERR_UNSUPPORTED there; the *_v2 entry points below take the Spitzer numbers next to it.  Spitzer resistivity is
 * refused everywhere, as in the reference (hydro.cpp:662-665). */
typedef struct apk_diff_cfg {
  int conduction, conduction_coeff; /* apk_conduction, apk_conduction_coeff */
  double thermal_diff_coeff;        /* diffusion/thermal_diff_coeff_code */
  double conduction_sat_prefac;     /* conduction_sat_prefac */
  int viscosity, viscosity_coeff;   /* apk_viscosity, apk_viscosity_coeff */
  double mom_diff_coeff;            /* diffusion/mom_diff_coeff_code */
  int resistivity, resistivity_coeff; /* apk_resistivity, apk_resistivity_coeff */
  double ohm_diff_coeff;            /* diffusion/ohm_diff_coeff_code */
} apk_diff_cfg;

/* Replaces CalcDiffFluxes(StateDescriptor*, MeshData<Real>*) src/hydro/diffusion/diffusion.cpp:18-53 (called at the end
 * of CalculateFluxes when diffusion/integrator = unsplit, hydro.cpp:1202-1205): ThermalFluxIsoFixed
 * (conduction.cpp:189-259), ThermalFluxGeneral for anisotropic conduction (conduction.cpp:265-471),
 * MomentumDiffFluxIsoFixed (viscosity.cpp:94-289), OhmicDiffFluxIsoFixed (resistivity.cpp:91-230).  ADDS the diffusive
 * fluxes of every enabled process into flux[d] on the faces of interior cells: one launch per active direction.  Reads
 * prim, including one layer of ghost cells (edges too).  Resistivity and anisotropic conduction need GLM-MHD.  The
 * transverse derivatives of the Ohmic current divide by 2 dx where the reference takes Xf(k+1) - Xf(k-1). */
int apk_calc_diff_fluxes(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg, apk_stream_t stream);

/* Replaces the diffusive part of Hydro::EstimateTimestep (hydro.cpp:935-949): the minimum of
 * EstimateConductionTimestep (conduction.cpp:44-184), EstimateViscosityTimestep (viscosity.cpp:34-89) and
 * EstimateResistivityTimestep (resistivity.cpp:33-86) over the enabled processes, each cfl_diff * fac * min(...) with
 * fac = 1/2, 1/4, 1/6 in 1, 2, 3 dimensions.  Fixed isotropic processes depend on the cell widths only and are
 * evaluated on the host; anisotropic conduction is a device min-reduction over the interior (synchronises `stream`).
 * No process enabled: *dt_out = DBL_MAX. */
int apk_estimate_diffusion_timestep(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg, double cfl_diff,
                                    double *dt_out, apk_stream_t stream);

/* What ThermalDiffusivity::Get (conduction.cpp:28-42) needs for conduction_coeff = APK_CONDC_SPITZER, in code units:
 *   T_cgs = mbar / k_boltzmann * p / rho;  kappa = coeff_code * T_cgs^(5/2);  chi = kappa * mbar / k_boltzmann / rho
 * each left to right.  T^(5/2) is evaluated as T * T * sqrt(T) (three correctly rounded operations) where the reference
 * calls std::pow: within 3 ulp of it, and the same bits in every build and in the tests' restatement. */
typedef struct apk_spitzer_cfg {
  double coeff_code;  /* diffusion/spitzer_cond_in_erg_by_s_K_cm * erg / (s * cm) in code units (hydro.cpp:577-581) */
  double mbar;        /* mu * atomic_mass_unit in code units (the "mbar" param, hydro.cpp:500) */
  double k_boltzmann; /* Units::k_boltzmann() in code units */
} apk_spitzer_cfg;

/* apk_calc_diff_fluxes with the whole dispatch of CalcDiffFluxes (diffusion.cpp:18-53): isotropic conduction with a
 * fixed coefficient is ThermalFluxIsoFixed; isotropic Spitzer and anisotropic conduction with either coefficient are
 * ThermalFluxGeneral (conduction.cpp:265-471; its isotropic branch :344-346 uses the lim4 transverse gradients too, and
 * a collapsed direction contributes 0 to |grad T|).  spitzer == NULL: exactly apk_calc_diff_fluxes (which forwards
 * here).  cfg->conduction_coeff = APK_CONDC_SPITZER reads `spitzer` instead of cfg->thermal_diff_coeff: NULL is
 * APK_ERR_UNSUPPORTED, a member that is not positive APK_ERR_INVALID.  `spitzer` is not read otherwise. */
int apk_calc_diff_fluxes_v2(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg, const apk_spitzer_cfg *spitzer,
                            apk_stream_t stream);
/* apk_estimate_diffusion_timestep with the general branch of EstimateConductionTimestep (conduction.cpp:93-181) for
 * Spitzer: per interior cell with a temperature gradient, dx_d^2 / chi(p, rho) (isotropic; no TINY_NUMBER there) or the
 * anisotropic expression with chi(p, rho) of the cell, the flux_classic / flux_sat > 100 early return included.  Both
 * are device min-reductions (synchronises `stream`).  `spitzer` as above. */
int apk_estimate_diffusion_timestep_v2(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg,
                                       const apk_spitzer_cfg *spitzer, double cfl_diff, double *dt_out, apk_stream_t stream);

/* ---- RKL2 super-time-stepping (diffusion/integrator = rkl2) ---------------------------------------------------------
 * Operator-split Runge-Kutta-Legendre super-time-stepping of the diffusive processes (Meyer, Balsara & Aslam 2014):
 * AddSTSTasks, src/hydro/hydro_driver.cpp:168-344.  A half step of length tau takes s sub-stages on four registers of
 * conserved variables: Y0 (the state on entry), Yjm1 (the pack that carries primitives and flux arrays, "base"), Yjm2
 * and MY0 = -div F_diff(Y0).  After every sub-stage the caller exchanges the ghost zones of Yjm1 and converts it to
 * primitives (hydro_driver.cpp:269-273, 334-338). */

/* Replaces the stage count of AddSTSTasks (hydro_driver.cpp:176-181; Meyer+2014 eq. 21):
 * s = int(0.5 * (sqrt(9 + 16 tau / dt_diff) - 1)) + 1, made odd.  Host only. */
int apk_rkl2_num_stages(double tau, double dt_diff, int *s_rkl);
/* Replaces the coefficients of sub-stage j of s (1 <= j <= s): j = 1 gives mu_tilde_1 = 4 / (3 (s^2 + s - 2))
 * (hydro_driver.cpp:101-104; the others 0), j >= 2 the recursion of hydro_driver.cpp:276-291, 341-342, in the
 * reference's operation order.  Host only. */
int apk_rkl2_coefficients(int s_rkl, int j, double *mu, double *nu, double *mu_tilde, double *gamma_tilde);
/* Replaces parthenon::Update::FluxDivergence<MeshData<Real>>(md, out), call site hydro_driver.cpp:254-255:
 * out.cons <- -div F(md.flux) on interior cells, every variable; the expression and term order of
 * apk_update_with_flux_divergence. */
int apk_flux_divergence(apk_ctx *ctx, const apk_pack *md, const apk_pack *out, apk_stream_t stream);
/* Replaces RKL2StepFirst(Y0, Yjm1, Yjm2, MY0, s_rkl, tau), hydro_driver.cpp:93-126:
 * Yjm1 <- Y0 + mu_tilde_1 tau MY0, Yjm2 <- Y0 on interior cells.  The four registers are distinct arrays. */
int apk_rkl2_step_first(apk_ctx *ctx, const apk_pack *y0, const apk_pack *yjm1, const apk_pack *yjm2, const apk_pack *my0,
                        int s_rkl, double tau, apk_stream_t stream);
/* Replaces RKL2StepOther(Y0, Yjm1, Yjm2, MY0, mu_j, nu_j, mu_tilde_j, gamma_tilde_j, tau), hydro_driver.cpp:128-166:
 * Yj = mu_j Yjm1 + nu_j Yjm2 + (1 - mu_j - nu_j) Y0 + mu_tilde_j tau (-div F(Yjm1.flux)) + gamma_tilde_j tau MY0;
 * Yjm2 <- Yjm1, Yjm1 <- Yj.  Yjm1 carries the flux arrays (zeroed, then apk_calc_diff_fluxes). */
int apk_rkl2_step_other(apk_ctx *ctx, const apk_pack *y0, const apk_pack *yjm1, const apk_pack *yjm2, const apk_pack *my0,
                        double mu_j, double nu_j, double mu_tilde_j, double gamma_tilde_j, double tau, apk_stream_t stream);

typedef struct apk_rkl2_regs {
  const apk_pack *y0, *yjm2, *my0; /* conserved arrays only; the shape of the pack they go with */
} apk_rkl2_regs;
typedef struct apk_rkl2_coeffs {
  double mu, nu, mu_tilde, gamma_tilde; /* apk_rkl2_coefficients; the first sub-stage reads mu_tilde (= mu_tilde_1) only */
} apk_rkl2_coeffs;
/* One whole sub-stage in ONE kernel: replaces ResetFluxes + CalcDiffFluxes + FluxDivergence + RKL2StepFirst (first != 0;
 * hydro_driver.cpp:234-260) or ResetFluxes + CalcDiffFluxes + RKL2StepOther (hydro_driver.cpp:306-326).  A lane owns an
 * interior cell of md (= Yjm1), forms the diffusive fluxes through its 2 ndim faces from md.prim (one layer of ghost
 * cells, edges too) with the arithmetic of apk_calc_diff_fluxes on zeroed arrays, takes their divergence and applies the
 * step: in the parity build bit for bit what the sequence above leaves in Yjm1, Yjm2 (and MY0 when first).  Reads
 * primitives, writes conserved arrays: in place, no flux arrays needed. */
int apk_rkl2_substage_fused(apk_ctx *ctx, const apk_pack *md, const apk_rkl2_regs *regs, const apk_diff_cfg *cfg,
                            const apk_rkl2_coeffs *coeffs, double tau, int first, apk_stream_t stream);
/* The same with the fluxes of apk_calc_diff_fluxes_v2; `spitzer` as there (NULL: exactly apk_rkl2_substage_fused, which
 * forwards here).  The diffusivity of the lane's cell and of each of its 2 ndim neighbours is formed once. */
int apk_rkl2_substage_fused_v2(apk_ctx *ctx, const apk_pack *md, const apk_rkl2_regs *regs, const apk_diff_cfg *cfg,
                               const apk_spitzer_cfg *spitzer, const apk_rkl2_coeffs *coeffs, double tau, int first,
                               apk_stream_t stream);

/* ---- tabular radiative cooling (<cooling> enable_cooling = tabular) -------------------------------------------------
 * Integrator enum: numeric values = position in cooling::CoolIntegrator, tabular_cooling.hpp:96. */
enum apk_cool_integrator { APK_COOL_UNDEFINED = 0, APK_COOL_RK12 = 1, APK_COOL_RK45 = 2, APK_COOL_TOWNSEND = 3 };

/* The parameters TabularCooling::TabularCooling reads (tabular_cooling.cpp:30-276) and the "Hydro" params it takes from
 * the package (AdiabaticIndex, mbar_over_kb, He_mass_fraction, units.mh()), all in code units. */
typedef struct apk_cooling_params {
  int integrator;         /* apk_cool_integrator */
  int max_iter;           /* cooling/max_iter */
  double cfl;             /* cooling/cfl (<= 0: no time-step limit) */
  double d_log_temp_tol;  /* cooling/d_log_temp_tol: allowed relative unevenness of the log T spacing */
  double d_e_tol;         /* cooling/d_e_tol (0: fixed sub steps dt / max_iter) */
  double T_floor;         /* hydro/Tfloor in K (negative: none) */
  double lambda_units;    /* cooling/lambda_units_cgs / (erg cm^3 / s in code units) */
  double gamma;           /* hydro/gamma */
  double mbar_over_kb;    /* mu mh / kB */
  double He_mass_fraction;
  double mh;              /* hydrogen mass in code units (Units::mh) */
} apk_cooling_params;

typedef struct apk_cooling_table apk_cooling_table;

/* Replaces the table part of TabularCooling::TabularCooling (tabular_cooling.cpp:103-276): checks the table (>= 2
 * rows, increasing log T, even spacing within d_log_temp_tol unless townsend with cfl <= 0), converts log_lambdas to code
 * units (log_lambda - log10(lambda_units)), precomputes the Townsend coefficients alpha_k, Y_k (:230-265; alpha_k == 1 is
 * refused) and uploads the arrays.  log_temps / log_lambdas: host arrays of n rows as read from the file.  A refusal
 * returns APK_ERR_INVALID with the reference's message in apk_last_error. */
int apk_cooling_table_create(apk_ctx *ctx, const double *log_temps, const double *log_lambdas, int n,
                             const apk_cooling_params *params, apk_cooling_table **out);
void apk_cooling_table_destroy(apk_cooling_table *table);

/* CoolingTableObj::DeDt (tabular_cooling.hpp:129-173) at n points: device arrays e (specific internal energy), rho ->
 * dedt; valid[i] = 0 where DeDt cleared is_valid (e < 0 or NaN), else 1.  For testing. */
int apk_cooling_dedt(apk_ctx *ctx, const apk_cooling_table *table, const double *e, const double *rho, double *dedt,
                     int *valid, int64_t n, apk_stream_t stream);

/* Replaces TabularCooling::SrcTerm (tabular_cooling.cpp:278-288), called with beta_dt by AddUnsplitSources
 * (hydro.cpp:227-246): SubcyclingFixedIntSrcTerm<RK12Stepper | RK45Stepper> (:290-487) or TownsendSrcTerm (:489-604) on
 * the interior cells of every block.  Changes cons(IEN) only.  Deviations: ghost cells are not cooled (the reference
 * loops over IndexDomain::entire; the stage's ghost exchange refills them before anything reads them) and prim(IPR) is
 * not written (ConsToPrim recomputes it after the stage).  The reference's device failures latch APK_FLAG_COOL_* into the
 * flag word (apk_poll_device_flags). */
int apk_tabular_cooling_src(apk_ctx *ctx, const apk_pack *md, const apk_cooling_table *table, int fluid, double dt,
                            apk_stream_t stream);

/* Replaces TabularCooling::EstimateTimeStep (tabular_cooling.cpp:606-665), joined to min_dt by Hydro::EstimateTimestep
 * (hydro.cpp:926-933): cfl * min over interior cells of |e / DeDt(e)| from the stored primitives (+inf where DeDt is 0
 * or e is below the floor).  cfl <= 0: DBL_MAX; cfl NaN or infinite: +inf (no launch).  Synchronises `stream`. */
int apk_estimate_cooling_timestep(apk_ctx *ctx, const apk_pack *md, const apk_cooling_table *table, double *dt_out,
                                  apk_stream_t stream);

/* Replaces Hydro::FirstOrderFluxCorrect<fluid>(u0,u1,gam0,gam1,beta_dt)
 * src/hydro/hydro.cpp:1223-1342.  Iterates <= 4 attempts, one host sync per attempt like
 * the reference's parallel_reduce.  *num_corrected (optional) = cells corrected. */
int apk_first_order_flux_correct(apk_ctx *ctx, const apk_pack *u0, const apk_pack *u1,
                                 int fluid, const apk_eos *eos, double c_h, double gam0,
                                 double gam1, double beta_dt, long long *num_corrected,
                                 apk_stream_t stream);
/* The admissibility test of FirstOrderFluxCorrect (hydro.cpp:1297-1306: density > 0 and
 * E - kinetic [- magnetic] energy > 0) on the conserved state of the pack's interior cells; count =
 * cells that fail it.  Lets a caller run apk_stage_fused optimistically where the reference enables
 * first_order_flux_correct and fall back to the flux-array sequence only when a cell needs it
 * (stages with gam0 = 0, whose inputs the fused stage leaves intact).  Synchronises. */
int apk_count_unphysical(apk_ctx *ctx, const apk_pack *md, int fluid, long long *count,
                         apk_stream_t stream);

/* Replaces the HydroHst<...> reductions src/hydro/hydro.cpp:145-208:
 * out[8] = mass, 1-mom, 2-mom, 3-mom, KE, tot-E, ME, relDivB.  Synchronises `stream`. */
int apk_history(apk_ctx *ctx, const apk_pack *md, int fluid, double *out8,
                apk_stream_t stream);

/* Reads-and-clears the device flag word (APK_FLAG_*).  Synchronises `stream`. */
int apk_poll_device_flags(apk_ctx *ctx, unsigned *flags, apk_stream_t stream);
/* commit (keep = 1) or drop (keep = 0) the flags of stages run with apk_stage_args.trial = 1;
 * asynchronous on `stream`.  Mirrors the reference, where the FOFC trial update
 * (hydro.cpp:1283-1306) never reaches ConservedToPrimitive unless it is accepted. */
int apk_trial_flags(apk_ctx *ctx, int keep, apk_stream_t stream);

/* ---- ghost zones (the step either side of the path; Parthenon bvals, call sites
 *      src/hydro/hydro_driver.cpp:506,567-568) ------------------------------------------ */
/* One strided box copy: dst(v, k, j, i) = sign_v * src(v, k', j', i').  With a zero source
 * stride it broadcasts (outflow); with a negative stride it mirrors (reflecting,
 * src/bvals/boundary_conditions_apk.hpp:38-85).  Used for same-rank neighbour copies,
 * packing into / unpacking from contiguous message buffers, and physical boundaries. */
typedef struct apk_copy_region {
  const double *src;
  double *dst;
  int ext[3];             /* box extent (ni, nj, nk) */
  int nvar;
  int64_t src_stride[4];  /* element strides for (i, j, k, v) */
  int64_t dst_stride[4];
  int flip_var;           /* variable index whose sign is flipped, or -1 */
} apk_copy_region;
typedef struct apk_copy_plan apk_copy_plan;
int apk_copy_plan_create(apk_ctx *ctx, const apk_copy_region *regions, int n,
                         apk_copy_plan **out);
void apk_copy_plan_destroy(apk_copy_plan *plan);
int apk_copy_plan_run(apk_ctx *ctx, const apk_copy_plan *plan, apk_stream_t stream);
/* The same copy for plans whose destinations are ghost zones of cons arrays, with
 * ConservedToPrimitive of every destination cell fused in: the primitives are written at
 * dst + prim_delta (in doubles; the distance from a block's cons array to its prim array, the
 * same for all regions of the plan).  Saves the separate ghost-zone ConsToPrim pass.  Refused
 * (APK_ERR_UNSUPPORTED) when a floor or ceiling of the EOS is active: those write cons back and
 * must keep acting after all boundary phases, as in the reference.  latch_flags = 0 keeps the
 * negative-density / -pressure flags quiet: a physical-boundary phase that is followed by
 * another one copies corner cells whose sources are only filled by that later phase. */
int apk_copy_plan_run_c2p(apk_ctx *ctx, const apk_copy_plan *plan, int fluid, const apk_eos *eos,
                          int64_t prim_delta, int latch_flags, apk_stream_t stream);
/* The same, storing the primitives ONLY: for ghost zones whose conserved values nothing reads -- the half-step
 * state of VL2, whose corrector (gam0 = 0) takes its fluxes from the primitives and updates the full-step state
 * (apk_stage_args.cons_store).  `dst` still names the cons array of the destination block (the primitives go to
 * dst + prim_delta); nothing is written at dst itself. */
int apk_copy_plan_run_c2p_prim_only(apk_ctx *ctx, const apk_copy_plan *plan, int fluid, const apk_eos *eos,
                                    int64_t prim_delta, int latch_flags, apk_stream_t stream);

/* ---- few-modes turbulence driver (BASELINE config 4 forcing; "next" row of SURVEY 8(f)) -------
 * The device side of turbulence::Driving (src/pgen/turbulence.cpp:373-482), which AthenaPK
 * enrols as Hydro::ProblemSourceFirstOrder (src/main.cpp:115, run after the last stage,
 * src/hydro/hydro_driver.cpp:559-560), and of FewModesFT::Generate's inverse transform
 * (src/utils/few_modes_ft.cpp:322-347).  The spectral state (3 x num_modes complex numbers),
 * its host RNG and the Ornstein-Uhlenbeck update stay on the host, as in the reference. */
typedef struct apk_fmft_block {
  double *acc;            /* [3][Nk][Nj][Ni] acceleration field ("acc", turbulence.cpp:119-127) */
  const double *phases_i; /* [2][num_modes][nx1]: (re|im, mode, cell), the shape of the reference's
                             "<prefix>_phases_i" variable (few_modes_ft.cpp:60-62, 143-160) */
  const double *phases_j; /* [2][num_modes][nx2] */
  const double *phases_k; /* [2][num_modes][nx3] */
} apk_fmft_block;
typedef struct apk_fmft apk_fmft;
int apk_fmft_create(apk_ctx *ctx, const apk_fmft_block *blocks /* host array */, int nblocks,
                    int num_modes, apk_fmft **out);
void apk_fmft_destroy(apk_fmft *f);
/* acc(b, n, k, j, i) = sum_m 2 (Re var_hat(n,m) Re phase - Im var_hat(n,m) Im phase) on the
 * interior; var_hat_host is [3][num_modes][2], copied to the device on `stream`: keep it valid
 * until the stream has been synchronised (apk_turb_mean_momentum, the next step, does) */
int apk_fmft_inverse(apk_ctx *ctx, const apk_pack *md, apk_fmft *f, const double *var_hat_host,
                     apk_stream_t stream);
/* turbulence::Perturb in three device steps around the reference's two MPI_Allreduce's
 * (turbulence.cpp:395-436): sums4 = (mass, rho*acc_1..3) * cell volume  [synchronises];
 * subtract sums4[n+1]/sums4[0] from acc_n and return sum acc^2 * volume    [synchronises];
 * scale acc by norm and kick momentum / energy with dt (turbulence.cpp:446-469). */
int apk_turb_mean_momentum(apk_ctx *ctx, const apk_pack *md, const apk_fmft *f, double *sums4,
                           apk_stream_t stream);
int apk_turb_remove_mean(apk_ctx *ctx, const apk_pack *md, apk_fmft *f, const double *sums4,
                         double *ampl_sum, apk_stream_t stream);
int apk_turb_apply(apk_ctx *ctx, const apk_pack *md, apk_fmft *f, double norm, double dt,
                   apk_stream_t stream);
/* apk_turb_apply plus the two tasks that follow the kick on the same cells (hydro_driver.cpp:559-577, 589-603):
 * FillDerived -- ConsToPrim with the floors of `eos`, prim replaced in place -- and, with estimate_dt, the
 * min-reduction of dx_d / (|v_d| + c_d) into the stage's word (read it with apk_stage_dt_read); the caller
 * then converts ghost zones only (apk_copy_plan_run_c2p / apk_cons_to_prim_ghosts).  One pass over cons
 * instead of three. */
int apk_turb_apply_fill(apk_ctx *ctx, const apk_pack *md, apk_fmft *f, double norm, double dt, int fluid,
                        const apk_eos *eos, int estimate_dt, apk_stream_t stream);
/* The same with the time-step estimate and WITHOUT storing the primitives: for cycles whose next stage derives its
 * input from the conserved state (apk_stage_args.prim_from_cons).  No passive scalars. */
int apk_turb_apply_dt(apk_ctx *ctx, const apk_pack *md, apk_fmft *f, double norm, double dt, int fluid,
                      const apk_eos *eos, apk_stream_t stream);
/* TurbulenceHst<Ms|Ma|pb> (turbulence.cpp:47-101): out3 = volume sums of sonic Mach number,
 * Alfvenic Mach number, plasma beta.  Synchronises. */
int apk_turbulence_history(apk_ctx *ctx, const apk_pack *md, int fluid, double gamma, double *out3,
                           apk_stream_t stream);

/* ---- mesh-refinement operators and block tagging (SURVEY 8(f) rank 3 building blocks) -------
 * The operators AthenaPK registers for `cons` (src/hydro/hydro.cpp:780-781):
 * Hydro::refinement_ops::ProlongateCellMinModMultiD (src/hydro/prolongation/custom_ops.hpp:49-186)
 * and Parthenon's RestrictAverage for cells and, for the coarse-fine flux correction
 * (src/hydro/hydro_driver.cpp:527-531), for face fluxes.  A plan is a list of index boxes over
 * many meshblocks of one shape, executed in ONE launch (AMR meshes have many 16^3 blocks: a launch
 * per block and per buffer would be latency bound).  Fine arrays are [nvar][Nk][Nj][Ni] with `ng`
 * ghosts, coarse buffers [nvar][cNk][cNj][cNi] with nx/2 interior cells and `cng` ghosts per active
 * dimension; face arrays have one more entry along their own direction.  Index boxes are inclusive
 * and given in COARSE indices; prolongation reads one coarse cell beyond the box. */
typedef struct apk_refine_geom {
  int nx[3];    /* fine interior cells of a meshblock (1 in a collapsed dimension) */
  int ng;       /* fine ghost cells */
  int cng;      /* coarse-buffer ghost cells */
  double dx[3]; /* fine cell widths */
} apk_refine_geom;
enum {
  APK_RO_PROLONGATE = 0,    /* src = coarse buffer, dst = fine array */
  APK_RO_RESTRICT_CELL = 1, /* src = fine array,   dst = coarse buffer */
  APK_RO_RESTRICT_FACE1 = 2,
  APK_RO_RESTRICT_FACE2 = 3,
  APK_RO_RESTRICT_FACE3 = 4,
  /* the same area average for fluxes stored the way apk_block_desc.flux stores them (cell-shaped
   * arrays, face i = lower face of cell i), into a cell-shaped coarse buffer: the coarse-fine flux
   * correction of the standalone driver */
  APK_RO_RESTRICT_FLUX1 = 5,
  APK_RO_RESTRICT_FLUX2 = 6,
  APK_RO_RESTRICT_FLUX3 = 7
};
typedef struct apk_refine_op {
  int kind;
  const double *src; /* device */
  double *dst;       /* device */
  int lo[3], hi[3];
  double xmin[3]; /* lower interior corner of the block (enters the slope spacings as in the
                     reference, which differences cell-centre coordinates) */
  double dx[3];   /* fine cell widths of THIS box; all zero = the plan's apk_refine_geom.dx.  Lets one
                     plan (one launch) hold boxes of several refinement levels */
} apk_refine_op;
typedef struct apk_refine_plan apk_refine_plan;
int apk_refine_plan_create(apk_ctx *ctx, const apk_refine_geom *geom, int nvar,
                           const apk_refine_op *ops /* host */, int nops, apk_refine_plan **out);
void apk_refine_plan_destroy(apk_refine_plan *p);
int apk_refine_plan_run(apk_ctx *ctx, const apk_refine_plan *p, apk_stream_t stream);

/* Coarse-fine flux correction AFTER a fused stage (hydro_driver.cpp:527-537 puts it before the flux
 * divergence; the fused stage has already applied the coarse block's own face flux F, so the cells
 * next to a coarse-fine face are corrected by the difference): for every element of a region
 *   cons += beta_dt * scale * (fine_avg - coarse_flux)   [times psi_factor for variable psi_var]
 * with scale = +1/dx for the lower face of the cell, -1/dx for its upper face; fine_avg is the
 * area average of the fine blocks' fluxes (an APK_RO_RESTRICT_FLUX* result or a message buffer),
 * coarse_flux the coarse block's flux on the same face (apk_calculate_fluxes_boundary).  psi_factor
 * is the Dedner damping exp(-alpha c_h beta_dt / mindx) the stage applied after its update.
 * average = 0: fine_avg holds the averages, one per element.  average = d + 1 (1..3): fine_avg is the
 * fine block's own cell-shaped x_d flux array at the first fine face under the region (src_stride =
 * twice that array's strides), and each element averages the 2 (2-D) or 4 (3-D) fine faces under its
 * coarse face at fine_stride[], weighted with fine_area -- the arithmetic of APK_RO_RESTRICT_FLUX1 + d,
 * bit for bit, without the restricted plane in between (same-rank faces). */
typedef struct apk_flux_fix_region {
  const double *fine_avg;    /* strides src_stride */
  const double *coarse_flux; /* strides dst_stride */
  double *cons;              /* strides dst_stride */
  int ext[3];
  int nvar;
  int64_t src_stride[4], dst_stride[4];
  double scale;
  int average, ndim;
  int64_t fine_stride[3];
  double fine_area;
} apk_flux_fix_region;
typedef struct apk_flux_fix_plan apk_flux_fix_plan;
int apk_flux_fix_plan_create(apk_ctx *ctx, const apk_flux_fix_region *regions /* host */, int n,
                             apk_flux_fix_plan **out);
/* The regions of up to three directions as ONE plan that runs in ONE launch: regions = direction 0's, then 1's, then
 * 2's (n_by_dir).  A coarse cell on an edge of its block may lie next to two or three coarse-fine faces; the plans per
 * direction correct it direction by direction, and so does this one: the region of the lowest direction that holds a
 * cell applies the terms of all of them in that order (same additions, same order: bit-identical to the three plans
 * run one after the other).  field_base / block_elems: the cell-shaped field [block][var][k][j][i] the regions' cons
 * pointers point into and its elements per block.  APK_ERR_UNSUPPORTED if a region shares cells with more than 8
 * others or is not laid out that way (the caller keeps one plan per direction). */
int apk_flux_fix_plan_create_merged(apk_ctx *ctx, const apk_flux_fix_region *regions /* host */, const int n_by_dir[3],
                                    const double *field_base, int64_t block_elems, apk_flux_fix_plan **out);
void apk_flux_fix_plan_destroy(apk_flux_fix_plan *p);
int apk_flux_fix_plan_run(apk_ctx *ctx, const apk_flux_fix_plan *p, double beta_dt, int psi_var,
                          double psi_factor, apk_stream_t stream);

/* Block tagging, one launch for the whole pack: refinement::gradient::PressureGradient
 * (src/refinement/gradient.cpp:18-61: refine above p0, derefine below 0.25 p0),
 * VelocityGradient (:64-96: p0, 0.5 p0), refinement::other::MaxDensity (src/refinement/other.cpp:
 * 18-44: refine above p0, derefine below p1).  tags[b] = +1 refine / 0 same / -1 derefine,
 * crit[b] (may be NULL) = the reduced criterion.  Synchronises. */
enum { APK_TAG_PRESSURE_GRADIENT = 0, APK_TAG_VELOCITY_GRADIENT = 1, APK_TAG_MAX_DENSITY = 2 };
int apk_tag_blocks(apk_ctx *ctx, const apk_pack *md, int criterion, double p0, double p1, int *tags,
                   double *crit, apk_stream_t stream);
/* The same in two halves, so that the tags share a host round trip with whatever else the caller
 * reads back at the end of a cycle (the driver enqueues the time-step reduction between the two):
 * _begin launches the reduction and the read-back into pinned memory without waiting; _end waits
 * for the stream and converts (pending = what _begin returned). */
int apk_tag_blocks_begin(apk_ctx *ctx, const apk_pack *md, int criterion, int *pending, apk_stream_t stream);
/* ... with apk_stage_args.face_neighbor's table (device, [nblocks][6]): ghost cells straight behind a face whose entry is
 * >= 0 are read from that block's interior, so the exchange in front of the check may leave those zones out (edges and
 * corners are read from the block's own ghost zones as before).  Same criteria, bit for bit. */
int apk_tag_blocks_begin_skip(apk_ctx *ctx, const apk_pack *md, int criterion, const int *face_neighbor, int *pending,
                              apk_stream_t stream);
/* The pressure-gradient criterion (gradient.cpp:18-61) AND the hyperbolic time-step estimate (hydro.cpp:845-895) in one
 * pass over the CONSERVED state: the end of a cycle whose stage loop stores no primitives (apk_stage_args.prim_from_cons).
 * What apk_cons_to_prim_dt_select(pressure, two layers) followed by apk_tag_blocks_begin_skip(APK_TAG_PRESSURE_GRADIENT)
 * computes, bit for bit, with no pressure array written and read back: the minimum goes to the stage's time-step word
 * (apk_stage_dt_read / apk_stage_dt_flags_read), the maxima are read by apk_tag_blocks_end(APK_TAG_PRESSURE_GRADIENT,
 * pending).  3-D packs with at least two ghost layers whose blocks are narrow enough for a few pressure planes in LDS
 * (16^3 .. 64^3), no passive scalars, eos without floors and ceilings: APK_ERR_UNSUPPORTED otherwise. */
int apk_tag_blocks_dt_from_cons(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const int *face_neighbor,
                                int *pending, apk_stream_t stream);
int apk_tag_blocks_end(apk_ctx *ctx, int nblocks, int criterion, int pending, double p0, double p1, int *tags,
                       double *crit, apk_stream_t stream);

/* field_loop::RelDivBHst (src/pgen/field_loop.cpp:60-95), the "UserRelDivB" history column of the
 * field-loop problem: sum of 0.5 |dx| |div B| / B0 * volume, B0 fixed.  Synchronises. */
int apk_history_user_reldivb(apk_ctx *ctx, const apk_pack *md, double B0, double *out,
                             apk_stream_t stream);

/* ---- tracer particles (src/tracers/tracers.cpp; uniform meshes, 3-D) ----------------------------------------------
 * One rank-wide structure of arrays in DEVICE memory: positions, id, the index of the owning block in the pack, an
 * active flag (0 once the particle has left through a non-periodic boundary) and the fields FillTracers interpolates
 * (tracers.cpp:64-85), in this order: rho, pressure, vel_x, vel_y, vel_z and, with GLM-MHD (nfields = 8), B_x, B_y,
 * B_z.  s, sdot: the lookback histories of s = ln rho and ds/dt (src/pgen/turbulence.cpp:200-216), structure of arrays
 * [n_lookback][lookback_stride] with the level outermost, level i holding the value of 2^(i-1) cycles' spacing (level 0:
 * the current cycle); s == NULL means "no histories", and every entry point then does what it does without them. */
#define APK_TRACER_N_LOOKBACK 12 /* turbulence.cpp:204: 0, 1, 2, 4, ... 1024 cycles */
#define APK_TRACER_N_SUMS 26     /* corr_s[12], corr_sdot[12], sum s, sum sdot */
typedef struct apk_tracer_arrays {
  int64_t n;
  double *x, *y, *z;
  int64_t *id;
  int32_t *block;
  int32_t *active;
  double *field[8];
  int nfields; /* 5 or 8 */
  double *s, *sdot;
  int64_t lookback_stride; /* >= n */
  int n_lookback;          /* APK_TRACER_N_LOOKBACK when s != NULL */
} apk_tracer_arrays;
/* The uniform block grid the particles live on.  block_origin: DEVICE array [nblocks][3], the lower interior face of
 * every block of the pack; block_table: DEVICE array [nb[2]][nb[1]][nb[0]], block coordinates to index in the pack;
 * block_size = cells per block times dx; periodic_lo / periodic_hi: that boundary of the domain wraps positions (every
 * other kind of boundary loses the particle). */
typedef struct apk_tracer_geom {
  double xmin[3], xmax[3], dx[3], block_size[3];
  int nb[3], periodic_lo[3], periodic_hi[3];
  const double *block_origin;
  const int32_t *block_table;
} apk_tracer_geom;
/* Replaces Tracers::AdvectTracers (tracers.cpp:189-242): Heun's method with the velocities the last fill stored on the
 * particle, x* = x + dt v_p, v* = the primitives' velocity interpolated at x* in the particle's block, x += dt / 2
 * (v_p + v*).  Trilinear on cell centres like interpolation::cent::linear, NOT clamped to the interior: reads prim two
 * ghost layers deep, edges and corners included (APK_ERR_NGHOST with fewer).  Positions are left unwrapped. */
int apk_tracers_advect(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *tracers, const apk_tracer_geom *geom,
                       double dt, apk_stream_t stream);
/* Replaces what the swarm's transport does on one rank after the advection (hydro_driver.cpp:615-660): positions beyond
 * a periodic boundary wrap, particles beyond any other boundary become inactive, and every other particle gets the block
 * that contains its position.  counters: two DEVICE words, [0] += particles lost, [1] = 1 when any particle changed its
 * block or was lost. */
int apk_tracers_reown(apk_ctx *ctx, const apk_tracer_arrays *tracers, const apk_tracer_geom *geom,
                      unsigned long long *counters, apk_stream_t stream);
/* Replaces Tracers::FillTracers (tracers.cpp:249-308): all fields interpolated at the particle's position in its
 * block. */
int apk_tracers_fill(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *tracers, const apk_tracer_geom *geom,
                     apk_stream_t stream);
/* The three of them in ONE launch (one lane per particle, both gathers; tracers.cpp:189-308 and
 * hydro_driver.cpp:615-660).  Bit for bit what the three calls give in the -ffp-contract=off build. */
int apk_tracers_step_fused(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *tracers, const apk_tracer_geom *geom,
                           double dt, unsigned long long *counters, apk_stream_t stream);
/* Counting sort of the particles by (block, interior k-plane), inactive ones last, into a second set of arrays `out`
 * (no equivalent in the reference, whose swarms are per block).  buckets: DEVICE scratch of nbuckets = blocks x nx3 + 1
 * words.  The order inside a bucket is arbitrary. */
int apk_tracers_sort(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *tracers, const apk_tracer_arrays *out,
                     const apk_tracer_geom *geom, unsigned long long *buckets, int nbuckets, apk_stream_t stream);
/* Replaces the device part of turbulence::ProblemFillTracers (src/pgen/turbulence.cpp:557-584) for cycle number
 * `cycle` >= 0: per active particle, level idx = 11 ... 1 of s and sdot takes the value of level idx - 1 when
 * cycle % 2^(idx-1) == 0 (a level that does not shift is read, not written), then s[0] = log(rho) of field[0] and
 * sdot[0] = (s[0] - s[1]) / dt; and the sums over active particles, without atomics: every workgroup of 256 particles
 * writes its 26 partial sums to partials[workgroup][26] (DEVICE scratch of npartials_cap rows >= (n + 255) / 256), and a
 * second kernel adds the rows into sums26 (DEVICE): [0..11] sum s[0] s[i], [12..23] sum sdot[0] sdot[i], [24] sum s[0],
 * [25] sum sdot[0].  NOT divided by the number of active particles (turbulence.cpp:605-608 is the caller's).  Reads of
 * `tracers` only n, active, field[0] and the histories.  Does not synchronise. */
int apk_tracers_lookback(apk_ctx *ctx, const apk_tracer_arrays *tracers, long long cycle, double dt, double *partials,
                         long long npartials_cap, double *sums26, apk_stream_t stream);
/* apk_tracers_step_fused and apk_tracers_lookback in ONE launch plus the small summing kernel (tracers.cpp:189-308,
 * hydro_driver.cpp:615-660 and turbulence.cpp:557-584): the update uses the rho the fill just computed.  tracers->s
 * must not be NULL.  Bit for bit what the separate calls leave in the particle arrays in the -ffp-contract=off build. */
int apk_tracers_step_fused_lookback(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *tracers,
                                    const apk_tracer_geom *geom, double dt, unsigned long long *counters, long long cycle,
                                    double *partials, long long npartials_cap, double *sums26, apk_stream_t stream);

/* ---- static gravity of the cluster problem (src/pgen/cluster/cluster_gravity.hpp) -----------------------------------
 * ClusterGravity's members in code units: which components act, and their constants with G and the masses rolled in
 * (the constructor's arithmetic is done by the host, csrc/host/cluster.cpp). */
enum apk_cluster_bcg { APK_BCG_NONE = 0, APK_BCG_HERNQUIST = 1 };
typedef struct apk_cluster_gravity {
  int include_nfw, which_bcg, include_smbh;
  double r_nfw_s, g_const_nfw, r_bcg_s, g_const_bcg, g_const_smbh, smoothing_r;
} apk_cluster_gravity;

/* Replaces GravitationalFieldSrcTerm<ClusterGravity> (src/hydro/srcterms/gravitational_field.hpp:25-64), called with
 * beta_dt by ProblemSourceUnsplit, the last of AddUnsplitSources (hydro.cpp:227-246).  Interior cells of every block:
 *   r = sqrt(x^2 + y^2 + z^2), src = (r == 0) ? 0 : beta_dt * prim.rho * g_from_r(r) / r,
 *   cons.M_d -= src * x_d, cons.E -= src * (x vx + y vy + z vz)      (rho, v: md's stored primitives)
 * block_xmin: device, [nblocks + 1][3] -- rows 0 .. nblocks-1 the lower interior corner of each block, the last row the
 * lower corner of the whole mesh.  The centre of interior cell i_d of a block is the number the host's generators use,
 *   x_d = xmin_d + ((g_d + i_d) + 1/2) dx_d,   g_d = rint((corner_d - xmin_d) / dx_d) the block's first global cell,
 * which is corner_d + (i_d + 1/2) dx_d up to rounding (and exactly that for the blocks at the mesh's lower corner). */
int apk_gravity_src(apk_ctx *ctx, const apk_pack *md, const apk_cluster_gravity *gravity, const double *block_xmin,
                    double beta_dt, apk_stream_t stream);
/* ClusterGravity::g_from_r (cluster_gravity.hpp:173-201) at n radii: device arrays r -> g.  For tests. */
int apk_gravity_g_from_r(apk_ctx *ctx, const apk_cluster_gravity *gravity, const double *r, double *g, int64_t n,
                         apk_stream_t stream);

/* ---- AGN feedback and the magnetic tower of the cluster problem (src/pgen/cluster/agn_feedback.{hpp,cpp},
 * magnetic_tower.{hpp,cpp}, jet_coords.hpp, cluster_utils.hpp) --------------------------------------------------------
 * The jet frame (JetCoords, jet_coords.hpp:25-37): cos and sin of the axis' angle off z and of its angle around z,
 * phi0 + time * phi_dot, computed by the host (csrc/host/feedback_model.cpp) and passed by value. */
typedef struct apk_jet_coords {
  double cos_theta, sin_theta, cos_phi, sin_phi;
} apk_jet_coords;
/* The numbers AGNFeedback::FeedbackSrcTerm computes before its loop (agn_feedback.cpp:263-303), for one stage's beta_dt,
 * in the reference's operation order (host: agn_feedback_stage_numbers).  vceil / eceil = +inf: no ceiling. */
typedef struct apk_agn_feedback_cfg {
  double thermal_feedback, thermal_density, thermal_radius;
  double jet_density, jet_momentum, jet_feedback;
  double kinetic_jet_radius, kinetic_jet_thickness, kinetic_jet_offset;
  double vceil, eceil;
} apk_agn_feedback_cfg;
enum apk_tower_potential { APK_TOWER_UNDEFINED = 0, APK_TOWER_LI = 1, APK_TOWER_DONUT = 2 };
/* MagneticTower's members that MagneticTowerObj takes (magnetic_tower.hpp:45-58, 167-176) */
typedef struct apk_magnetic_tower_cfg {
  int potential; /* apk_tower_potential, uniform over a launch */
  double li_alpha, l_scale, donut_offset, donut_thickness, l_mass_scale;
} apk_magnetic_tower_cfg;

/* Replaces the loop of AGNFeedback::FeedbackSrcTerm (agn_feedback.cpp:314-409) on the interior cells of every block,
 * operation for operation: the thermal sphere (r2 <= R^2; AddDensityToConsAtFixedVel, cluster_utils.hpp:22-34, on the
 * stored primitives), the jet cylinders (r < radius, offset <= |h| <= offset + thickness; ConsToPrim before and after
 * the deposit), the velocity and internal-energy ceilings on every cell while jet_density > 0 (outside the cylinders
 * they see the stored primitives), and the closing ConsToPrim, which writes the stored primitives of every interior
 * cell.  Where the reference aborts on the device ("Kinetic injection leads to negative pressure") the kernel latches
 * APK_FLAG_AGN_NEG_PRESSURE in the flag word (apk_poll_device_flags) and goes on.  Squares are products (x * x) where
 * the reference writes pow(x, 2).  block_xmin as for apk_gravity_src. */
int apk_agn_feedback_src(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_agn_feedback_cfg *cfg,
                         const apk_jet_coords *jet, const double *block_xmin, apk_stream_t stream);
/* Replaces MagneticTower::AddSrcTerm (magnetic_tower.cpp:29-140), GLM-MHD only, in ONE kernel and without the
 * reference's potential array: a cell evaluates PotentialInSimCart (magnetic_tower.hpp:60-102) at its six neighbours'
 * centres -- the same centre function of the same index a stored array would have been filled with -- forms the
 * central-difference curl in the reference's association (/ dx / 2.0), adds b to cons B, prim_B . b + 0.5 b^2 to E (the
 * stored primitive field) and, with mass_to_add > 0, the Gaussian density (DensityFromSimCart) scaled by
 * mass_to_add / (l_mass_scale^3 pi^(3/2)).  field_to_add = mass_to_add = 0 launches nothing. */
int apk_magnetic_tower_src(apk_ctx *ctx, const apk_pack *md, const apk_magnetic_tower_cfg *tower, const apk_jet_coords *jet,
                           const double *block_xmin, double field_to_add, double mass_to_add, apk_stream_t stream);
/* Replaces MagneticTower::ReducePowerContribs (magnetic_tower.cpp:146-202): per block, sum(prim_B . b1 dV) and
 * sum(0.5 b1^2 dV) over its interior cells, b1 = FieldInSimCart at unit field, into contribs[nblocks][2] (device).  A
 * fixed reduction tree per block, no atomics: a block's pair is a function of the block alone, bit for bit. */
int apk_magnetic_tower_power_contribs(apk_ctx *ctx, const apk_pack *md, const apk_magnetic_tower_cfg *tower,
                                      const apk_jet_coords *jet, const double *block_xmin, double *contribs,
                                      apk_stream_t stream);

/* ---- AGN triggering of the cluster problem (src/pgen/cluster/agn_triggering.{hpp,cpp}, cluster_utils.hpp:40-52) -------
 * The accretion sphere is a few cells across at the centre of a large mesh, and neither the mesh nor the radius changes
 * during a run: the host builds an ACTIVE LIST once (csrc/host/cluster.cpp: triggering_active_list) -- per local block
 * the index box, in the block's extended index space (ghost cells included, 0 .. ni-1), of the cells whose centre can
 * satisfy |x_d| < accretion_radius in all three directions, widened by one cell per side; blocks with an empty box are
 * not listed -- and the kernels launch over the list only.  A kernel clips every box to the block's arrays. */
enum apk_agn_triggering_mode { APK_TRIG_NONE = 0, APK_TRIG_COLD_GAS = 1, APK_TRIG_BOOSTED_BONDI = 2, APK_TRIG_BOOTH_SCHAYE = 3 };
typedef struct apk_trig_box {
  int block;        /* index into the pack */
  int lo[3], hi[3]; /* i, j, k: lo inclusive, hi exclusive, in the extended index space */
} apk_trig_box;
typedef struct apk_agn_triggering_cfg {
  int mode;                    /* apk_agn_triggering_mode, not NONE */
  int remove_accreted_mass;    /* COLD_GAS: remove in the reduction's launch */
  double accretion_radius;
  double cold_temp_thresh, cold_t_acc;
  double mean_molecular_mass_by_kb; /* mean_molecular_mass / k_boltzmann, the host's number */
} apk_agn_triggering_cfg;
/* Replaces AGNTriggering::ReduceBondiTriggeringQuantities (agn_triggering.cpp:202-264) and ReduceColdMass
 * (agn_triggering.cpp:124-198).  sums: device, [nblocks][4]; blocks outside the list report zeros.
 * Bondi-like modes: per block the sums over its interior cells with r2 < R^2 (strict) of m = rho dV, m rho, m |v| and
 * m sqrt(gamma p / rho), from the stored primitives.  COLD_GAS: sums[b][0] = the interior mass of cells with r2 < R^2 and
 * T = mean_molecular_mass_by_kb * p / rho <= cold_temp_thresh (inclusive), the other three 0; and with
 * remove_accreted_mass every such cell of the box, ghost cells included, gets delta = -rho / cold_t_acc * dt through
 * AddDensityToConsAtFixedVelTemp (cluster_utils.hpp:40-52) and its primitives from ConsToPrim, whose flags go into the
 * flag word.  r2 = x * x + y * y + z * z (products where the reference writes pow(x, 2)).
 * Grid (P, nboxes): each workgroup of 256 takes a fixed contiguous share of its box's cells, i fastest; a lane adds its
 * cells in index order, the workgroup reduces through a fixed LDS tree, a second kernel adds a block's P partials in
 * order.  No atomics: a block's sums depend on nothing but the block and its box.  boxes: device, nboxes entries, at
 * most one per block; max_box_cells: the largest box.  block_xmin as for apk_gravity_src. */
int apk_agn_triggering_reduce(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_agn_triggering_cfg *cfg,
                              const apk_trig_box *boxes, int nboxes, int64_t max_box_cells, const double *block_xmin, double dt,
                              double *sums, apk_stream_t stream);
/* Replaces AGNTriggering::RemoveBondiAccretedGas (agn_triggering.cpp:269-315) over the same list: every cell of a box
 * with r2 < R^2, ghost cells included, gets delta = -rho / total_mass * accretion_rate * dt (that association) through
 * AddDensityToConsAtFixedVelTemp, then ConsToPrim. */
int apk_agn_triggering_remove_bondi(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, double accretion_radius,
                                    const apk_trig_box *boxes, int nboxes, int64_t max_box_cells, const double *block_xmin,
                                    double total_mass, double accretion_rate, double dt, apk_stream_t stream);

/* ---- SNIa feedback, stellar feedback and the clips of the cluster problem (src/pgen/cluster/snia_feedback.cpp,
 * stellar_feedback.cpp, cluster_clips.cpp, cluster_utils.hpp; csrc/kernels_cluster_sources.hip) ------------------------
 * SNIAFeedback's numbers and the Hernquist BCG's density (ClusterGravity::rho_from_r with NFW and SMBH off,
 * cluster_gravity.hpp:203-230).  rho_const_bcg = m_bcg_s * r_bcg_s / (2 pi) for HERNQUIST and 0 for NONE: what the
 * reference's calc_rho_const_bcg returns.  The reference never calls that function and reads its member uninitialised
 * (cluster_gravity.hpp:46, 220): this is the evident intent, not the behaviour. */
typedef struct apk_snia_cfg {
  double power_per_bcg_mass, mass_rate_per_bcg_mass;
  double rho_const_bcg, r_bcg_s, smoothing_r;
} apk_snia_cfg;
/* Replaces the loop of SNIAFeedback::FeedbackSrcTerm (snia_feedback.cpp:87-118) on the interior cells of every block:
 *   r = sqrt(x * x + y * y + z * z), r' = max(r, smoothing_r), rho_bcg = rho_const_bcg / (r' * ((r' + a) * (r' + a) * (r' + a)))
 *   cons.E += power_per_bcg_mass * beta_dt * rho_bcg; AddDensityToConsAtFixedVel(mass_rate_per_bcg_mass * beta_dt * rho_bcg)
 * on the stored primitives (cluster_utils.hpp:24-34), then ConsToPrim, whose flags go into the flag word; cons and prim
 * are stored.  The cube is a product where the reference writes pow(r + a, 3).  block_xmin as for apk_gravity_src. */
int apk_snia_feedback_src(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_snia_cfg *cfg,
                          const double *block_xmin, double beta_dt, apk_stream_t stream);
/* StellarFeedback's numbers (stellar_feedback.cpp:105-114): mass_to_energy = efficiency * c * c */
typedef struct apk_stellar_cfg {
  double stellar_radius, exclusion_radius;
  double number_density_threshold, temperature_threshold;
  double mbar, mbar_over_kb, mass_to_energy;
} apk_stellar_cfg;
/* the "cluster_*" params of cluster.cpp:250-277; a clip at its disabled value (dfloor <= 0, a ceiling +inf) is skipped */
typedef struct apk_clips_cfg {
  double clip_r, dfloor, vceil, vAceil, eceil;
} apk_clips_cfg;
/* Replaces ClusterSplitSrcTerm (cluster.cpp:85-93) in ONE launch over an active list (apk_trig_box, clipped to the
 * blocks' interior: both reference loops run over IndexDomain::interior).  A lane owns its cell and applies in order
 *   1. stellar != NULL: StellarFeedback::FeedbackSrcTerm's lambda (stellar_feedback.cpp:135-169) -- out when
 *      r > stellar_radius || r <= exclusion_radius (r = sqrt(r2)), when rho / mbar < number_density_threshold, when
 *      mbar_over_kb * p / rho > temperature_threshold (stored primitives); delta = threshold * mbar - rho;
 *      AddDensityToConsAtFixedVelTemp(delta), E += -mass_to_energy * delta, ConsToPrim.  Where the reference aborts
 *      ("Added thermal energy should be positive") APK_FLAG_STELLAR_ENERGY is latched and the kernel goes on.
 *   2. clips != NULL and r2 < clip_r * clip_r: ApplyClusterClips' lambda (cluster_clips.cpp:93-155) statement for
 *      statement -- ConsToPrim first, dfloor, vceil, vAceil (GLM-MHD only), eceil -- and NO ConsToPrim afterwards: the
 *      primitives are stored as the reference leaves them (a stale velocity after dfloor included).
 * sums: device, [nblocks][8], cleared first: stellar_mass (the sum of -(delta * dV)), added_dfloor_mass,
 * removed_eceil_energy, removed_vceil_energy, added_vAceil_mass, three zeros; the deterministic block sum of
 * apk_agn_triggering_reduce.  One call with both configurations equals stellar alone followed by clips alone. */
#define APK_FLAG_STELLAR_ENERGY 32u
int apk_cluster_split_src(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_stellar_cfg *stellar,
                          const apk_clips_cfg *clips, const apk_trig_box *boxes, int nboxes, int64_t max_box_cells,
                          const double *block_xmin, double *sums, apk_stream_t stream);

/* ---- field snapshots: one fused pass from the conserved state to a dense staging buffer (csrc/kernels_output.hip) ----
 * Component codes.  APK_OUT_CONS + n: conserved variable n as stored (n < nhydro + nscalars); APK_OUT_PRIM + n: primitive
 * n as ConsToPrim would give it (passive scalars: r_n = s_n / rho); the derived fields of the reference's
 * Cluster::UserWorkBeforeOutput (src/pgen/cluster.cpp:866-924), with SQR(x) = x * x and sums left to right:
 *   temperature = mbar_over_kb * P / rho           mach_sonic = sqrt(v1^2 + v2^2 + v3^2) / sqrt(gamma * P / rho)
 *   B_mag = sqrt(B^2)    mach_alfven = mach_sonic * c_s / sqrt(B^2 / rho)    plasma_beta = (B^2 != 0) ? P / (0.5 B^2) : NaN
 * (the last three: GLM-MHD packs only). */
enum apk_output_component {
  APK_OUT_CONS = 0,
  APK_OUT_PRIM = 64,
  APK_OUT_TEMPERATURE = 128,
  APK_OUT_MACH_SONIC = 129,
  APK_OUT_B_MAG = 130,
  APK_OUT_MACH_ALFVEN = 131,
  APK_OUT_PLASMA_BETA = 132
};
#define APK_OUT_MAX_COMPONENTS 48
typedef struct apk_output_desc {
  int ncomp;                        /* 1 .. APK_OUT_MAX_COMPONENTS */
  int single;                       /* 0 = double, 1 = float (round to nearest even) */
  double gamma;                     /* of mach_sonic / mach_alfven */
  double mbar_over_kb;              /* of temperature */
  int comp[APK_OUT_MAX_COMPONENTS]; /* apk_output_component codes, in output order */
} apk_output_desc;
/* Blocks [first, first + n) of md: out[block - first][component][k][j][i] over INTERIOR cells only, C order, double or
 * float; out is DEVICE memory of n * ncomp * nx3 * nx2 * nx1 items.  Every lane owns one interior cell, reads its
 * nhydro + nscalars conserved values once, runs ConsToPrim on a register copy and stores the components asked for.  The
 * pack is never written: a floor that fires changes the primitives that come out, not the state in memory, and no flag
 * is latched.  Needs no ghost zone and no stored primitive (md's prim pointers are not read).  Honours
 * apk_pack_desc.stride; 1-D, 2-D and 3-D blocks.  Does not synchronise. */
int apk_output_pack(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_output_desc *desc, int first,
                    int n, void *out, apk_stream_t stream);

/* The inverse of apk_output_pack for the conserved variables (restart files, csrc/host/restart.cpp).  `in`: DEVICE memory
 * [n][nhydro + nscalars][nx3][nx2][nx1], dense, interior cells, double; it goes into the interior of `cons` of blocks
 * [first, first + n).  One lane per interior cell, the variable loop inside the lane.  Ghost zones, row padding and prim
 * are never written.  Honours apk_pack_desc.stride; 1-D, 2-D and 3-D blocks.  Does not synchronise. */
int apk_restart_unpack(apk_ctx *ctx, const apk_pack *md, int first, int n, const double *in, apk_stream_t stream);

/* ---- in-library kernel timing (HIP events on the caller's stream) ------------------------
 * bench.py needs the average duration of individual kernels measured live on the stream
 * they are launched on.  When enabled, every kernel launch of the listed groups is
 * bracketed by hipEventRecord; apk_kernel_timing_read() synchronises, accumulates and
 * resets.  Off by default (zero overhead). */
enum apk_timing_slot {
  APK_T_FUSED_X1 = 0, /* fused x1 sweep            */
  APK_T_FUSED_X2 = 1, /* fused x2 march            */
  APK_T_FUSED_X3 = 2, /* fused x3 march            */
  APK_T_FLUXES = 3,   /* flux-array sweeps (all directions of one call) */
  APK_T_UPDATE = 4,   /* UpdateWithFluxDivergence  */
  APK_T_DEDNER = 5,   /* DednerSource              */
  APK_T_C2P = 6,      /* ConservedToPrimitive      */
  APK_T_MIN_DT = 7,   /* EstimateHyperbolicTimestep */
  APK_T_COPY = 8,     /* strided box copies (ghost zones) */
  APK_T_FUSED_DC_X1 = 9,  /* the three fused sweeps when the stage reconstructs with donor */
  APK_T_FUSED_DC_X2 = 10, /* cell (VL2 predictor, hydro.cpp:457-463); slots 0-2 then hold   */
  APK_T_FUSED_DC_X3 = 11, /* only the high-order stages                                    */
  APK_T_TRACERS = 12,     /* tracer particles: advect, re-own, fill (or the fused step), lookbacks */
  APK_T_TRACER_SORT = 13, /* ... and their counting sort (memset, histogram, scan, scatter) */
  APK_T_GRAVITY = 14,     /* the static gravity source (apk_gravity_src) */
  APK_T_AGN_FEEDBACK = 15,   /* apk_agn_feedback_src */
  APK_T_TOWER = 16,          /* apk_magnetic_tower_src */
  APK_T_TOWER_CONTRIBS = 17, /* apk_magnetic_tower_power_contribs */
  APK_T_TRIGGERING = 18,     /* apk_agn_triggering_reduce, apk_agn_triggering_remove_bondi */
  APK_T_CLUSTER_SOURCES = 19, /* apk_snia_feedback_src, apk_cluster_split_src */
  APK_T_COUNT = 20
};
int apk_kernel_timing_enable(apk_ctx *ctx, int on);
/* total_ms / launches may be NULL */
int apk_kernel_timing_read(apk_ctx *ctx, int slot, double *total_ms, long long *launches);

#ifdef __cplusplus
}
#endif
#endif /* APK_AMD_H_ */
