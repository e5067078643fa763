// kernels_cluster_sources.hip -- the remaining sources of the cluster problem:
//   SNIAFeedback::FeedbackSrcTerm       src/pgen/cluster/snia_feedback.cpp:87-118     third term of ClusterUnsplitSrcTerm
//   ClusterGravity::rho_from_r          src/pgen/cluster/cluster_gravity.hpp:203-230  (the Hernquist BCG alone)
//   StellarFeedback::FeedbackSrcTerm    src/pgen/cluster/stellar_feedback.cpp:135-169 first term of ClusterSplitSrcTerm
//   ApplyClusterClips                   src/pgen/cluster/cluster_clips.cpp:93-155     second term of ClusterSplitSrcTerm
//   AddDensityToConsAtFixedVel[Temp]    src/pgen/cluster/cluster_utils.hpp:22-52
// and the C-ABI entries of include/apk_amd.h (apk_snia_feedback_src, apk_cluster_split_src).
//
// apk_snia_feedback_src.  One lane per interior cell of every block (cell_of, as in kernels_gravity.hip).  A lane reads
// its conserved values and the stored velocity, adds the energy and the mass at fixed velocity, runs ConsToPrim and stores
// cons and prim.  Bytes per cell: cons read and written, the velocity read, prim written: 144 B (hydro), 240 B (GLM-MHD).
// Two deliberate deviations from the reference:
//   * the cube is a product, (r + a) * (r + a) * (r + a), where the reference writes pow(r + a, 3) -- the project's rule
//     for squares, extended to cubes;
//   * rho_const_bcg = m_bcg_s * r_bcg_s / (2 pi) for HERNQUIST and 0 for NONE, what the reference's calc_rho_const_bcg
//     (cluster_gravity.hpp:89-102) returns.  The reference never calls that function, so its rho_const_bcg_ is read
//     uninitialised (cluster_gravity.hpp:46, 220): this is the evident intent, not the behaviour.
//
// apk_cluster_split_src.  Stellar feedback and the clips act within a few cells of the centre: the host hands over an
// active list (apk_trig_box, here the interior index box of the cells that can lie within max(stellar_radius, clip_r)),
// and the grid is (P, entries) as in kernels_triggering.hip, rows of a box coalescing with i fastest (active_box.hpp).
// A lane owns its cell: it holds cons and prim in registers, applies the stellar step and then the clips -- both are
// cell-local, so one call with both equals two calls, the store and reload between them being the identity -- and stores
// what it changed.  Only interior cells are touched (both reference loops run over IndexDomain::interior); the stage's
// exchange follows.  The five running totals are the deterministic block sums of block_sum.hpp, 8 slots per block:
// stellar_mass, added_dfloor_mass, removed_eceil_energy, removed_vceil_energy, added_vAceil_mass and three zeros.
// Where the reference's PARTHENON_REQUIRE(cell_delta_energy_density > 0) would abort the kernel latches
// APK_FLAG_STELLAR_ENERGY and goes on, as apk_agn_feedback_src does with APK_FLAG_AGN_NEG_PRESSURE.  The clips store the
// primitives exactly as the reference leaves them: no ConsToPrim afterwards, so after dfloor the velocity is the stale one.
//
// Measured (product build, GLM-MHD packs, one MI355X, device events, medians of 5 windows of 100 launches;
// tools/cluster_sources_cost.py, profiles/cluster_sources_cost.jsonl; the engineer's own
// measurements, not predictions), 8 x 128^3 | one 64^3 block:
//   apk_snia_feedback_src    0.764 ms = 0.92 x a device copy of its 240 B per cell (0.827 ms; 5.3 TB/s) | 11.8 us = 1.20 x    memory bound
//   apk_cluster_split_src    10.3 us = 1.04 x apk_agn_triggering_reduce (Bondi sums, 9.95 us), 2.8 x a copy of the boxes'
//                            bytes (3.7 us) | 15.0 us = 1.45 x the reduction (10.3 us), 4.1 x the copy
// with stellar radius and clip radius of four cells (1000 box cells) and all four clips: a clear and two dependent launches
// of a few workgroups, latency and not bandwidth, as for the triggering reduction.  Not measured: hydro packs, larger
// radii, either step alone, the kernels inside a cycle.
//
// Build forms.  The parity build (APK_FP_STRICT, -ffp-contract=off) agrees with a numpy restatement bit for bit on every
// stored value and sum (products, quotients, sums and square roots only).  The product build compiles the same source.
#include <cmath>
#include <cstdint>

#include "active_box.hpp"
#include "apk_internal.hpp"
#include "block_sum.hpp"
#include "cell_centre.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

// SNIAFeedback::FeedbackSrcTerm's lambda (snia_feedback.cpp:98-118), one interior cell per lane
template <int FLUID>
__global__ void __launch_bounds__(256) snia_feedback_kernel(PackView pv, apk_eos eos, apk_snia_cfg c, const double *__restrict__ block_xmin,
                                                            double beta_dt, unsigned *d_flags) {
  constexpr int NV = nvars<FLUID>();
  int b, i, j, k;
  int64_t off;
  if (!cell_of(pv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, b, i, j, k, off)) return;
  const apk_block_desc &bd = pv.blocks[b];
  double x, y, z;
  cell_xyz(bd, block_xmin, b, pv.nblocks, i, j, k, x, y, z);
  const int64_t sn = pv.sn;
  double *__restrict__ wp = bd.prim + off;
  double *__restrict__ up = bd.cons + off;
  double u[NV], w[NV], di;
#pragma unroll
  for (int n = 0; n < NV; ++n) u[n] = up[n * sn];
  const double v1 = wp[IV1 * sn], v2 = wp[IV2 * sn], v3 = wp[IV3 * sn];

  const double energy_per_bcg_mass = c.power_per_bcg_mass * beta_dt;
  const double mass_per_bcg_mass = c.mass_rate_per_bcg_mass * beta_dt;
  const double r_in = sqrt(x * x + y * y + z * z);
  const double r = (r_in < c.smoothing_r) ? c.smoothing_r : r_in;  // std::max(r_in, smoothing_r_)
  const double ra = r + c.r_bcg_s;
  const double bcg_density = c.rho_const_bcg / (r * ((ra * ra) * ra));
  const double snia_energy_density = energy_per_bcg_mass * bcg_density;
  const double density = mass_per_bcg_mass * bcg_density;
  u[IEN] += snia_energy_density;
  u[IDN] += density;  // AddDensityToConsAtFixedVel: the stored velocity
  u[IM1] += density * v1;
  u[IM2] += density * v2;
  u[IM3] += density * v3;
  u[IEN] += density * (0.5 * (sqr(v1) + sqr(v2) + sqr(v3)));
  const unsigned flags = cons_to_prim_cell<FLUID>(eos, u, w, di);
  if (flags) atomicOr(d_flags, flags);
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    up[n * sn] = u[n];
    wp[n * sn] = w[n];
  }
}

// ClusterSplitSrcTerm (cluster.cpp:85-93) on the cells of the active list: grid (P, entries)
template <int FLUID>
__global__ void __launch_bounds__(256) cluster_split_kernel(PackView pv, apk_eos eos, apk_stellar_cfg st, int have_stellar, apk_clips_cfg cl,
                                                            int have_clips, const apk_trig_box *__restrict__ boxes,
                                                            const double *__restrict__ block_xmin, double *__restrict__ partial,
                                                            unsigned *d_flags) {
  constexpr int NV = nvars<FLUID>();
  constexpr bool mhd = (FLUID == APK_FLUID_GLMMHD);
  __shared__ double red[8][256];
  const int e = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned flags = 0;
  BoxShare s;
  if (box_share(pv, boxes, e, p, P, s, true)) {
    const apk_block_desc &bd = pv.blocks[s.b];
    const double vol = bd.dx[0] * bd.dx[1] * bd.dx[2];
    const double inf = __builtin_inf();
    const double gm1 = eos.gamma - 1.0;
    const double clip_r2 = cl.clip_r * cl.clip_r, vceil2 = cl.vceil * cl.vceil, vAceil2 = cl.vAceil * cl.vAceil;
    const int64_t sn = pv.sn;
    for (int64_t q = s.first + threadIdx.x; q < s.last; q += 256) {
      const TrigCell cell = trig_cell(pv, s, bd, block_xmin, q);
      if (!cell.interior) continue;  // (box_share clipped the box already)
      const double r = sqrt(cell.r2);
      const bool in_shell = have_stellar && !(r > st.stellar_radius || r <= st.exclusion_radius);
      const bool in_clip = have_clips && cell.r2 < clip_r2;
      if (!in_shell && !in_clip) continue;
      double *__restrict__ up = bd.cons + cell.off;
      double *__restrict__ wp = bd.prim + cell.off;
      double u[NV], w[NV], di;
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        u[n] = up[n * sn];
        w[n] = wp[n * sn];
      }
      bool changed = false;

      // stellar feedback (stellar_feedback.cpp:144-169), on the stored primitives
      if (in_shell) {
        const double number_density = w[IDN] / st.mbar;
        const double temp = st.mbar_over_kb * w[IPR] / w[IDN];
        if (!(number_density < st.number_density_threshold) && !(temp > st.temperature_threshold)) {
          const double cell_delta_rho = st.number_density_threshold * st.mbar - w[IDN];
          acc[0] += -(cell_delta_rho * vol);
          add_density_fixed_vel_temp_regs<NV>(eos, cell_delta_rho, u, w);
          const double cell_delta_energy_density = -st.mass_to_energy * cell_delta_rho;
          if (!(cell_delta_energy_density > 0.0)) flags |= APK_FLAG_STELLAR_ENERGY;
          u[IEN] += cell_delta_energy_density;
          flags |= cons_to_prim_cell<FLUID>(eos, u, w, di);
          changed = true;
        }
      }

      // the clips (cluster_clips.cpp:93-155)
      if (in_clip) {
        flags |= cons_to_prim_cell<FLUID>(eos, u, w, di);
        changed = true;
        if (cl.dfloor > 0) {
          const double rho = w[IDN];
          if (rho < cl.dfloor) {
            acc[1] += (cl.dfloor - rho) * vol;
            u[IDN] = cl.dfloor;
            w[IDN] = cl.dfloor;
          }
        }
        if (cl.vceil < inf) {
          const double v2 = sqr(w[IV1]) + sqr(w[IV2]) + sqr(w[IV3]);
          if (v2 > vceil2) {
            const double v = sqrt(v2);
            u[IM1] *= cl.vceil / v;
            u[IM2] *= cl.vceil / v;
            u[IM3] *= cl.vceil / v;
            w[IV1] *= cl.vceil / v;
            w[IV2] *= cl.vceil / v;
            w[IV3] *= cl.vceil / v;
            const double removed_energy = 0.5 * w[IDN] * (v2 - vceil2);
            acc[3] += removed_energy * vol;
            u[IEN] -= removed_energy;
          }
        }
        if constexpr (mhd) {
          if (vAceil2 < inf) {
            const double rho = w[IDN];
            const double B2 = sqr(w[IB1]) + sqr(w[IB2]) + sqr(w[IB3]);
            const double va2 = B2 / rho;
            if (va2 > vAceil2) {
              const double rho_new = sqrt(B2 / vAceil2);
              acc[4] += (rho_new - rho) * vol;
              u[IDN] = rho_new;
              w[IDN] = rho_new;
            }
          }
        }
        if (cl.eceil < inf) {
          const double internal_e = w[IPR] / (gm1 * w[IDN]);
          if (internal_e > cl.eceil) {
            const double removed_energy = w[IDN] * (internal_e - cl.eceil);
            acc[2] += removed_energy * vol;
            u[IEN] -= removed_energy;
            w[IPR] = gm1 * w[IDN] * cl.eceil;
          }
        }
      }

      if (changed) {
#pragma unroll
        for (int n = 0; n < NV; ++n) {
          up[n * sn] = u[n];
          wp[n * sn] = w[n];
        }
      }
    }
  }
  if (flags) atomicOr(d_flags, flags);
  block_sum_store<5, 8>(red, acc, e, p, P, partial);
}

}  // namespace
}  // namespace apk

using namespace apk;

extern "C" {

int apk_snia_feedback_src(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_snia_cfg *cfg,
                          const double *block_xmin, double beta_dt, apk_stream_t stream) {
  if (!ctx || !md || !eos || !cfg || !block_xmin) return set_err(ctx, APK_ERR_INVALID, "apk_snia_feedback_src: bad argument");
  if (!(cfg->r_bcg_s > 0.0) && cfg->rho_const_bcg != 0.0)
    return set_err(ctx, APK_ERR_INVALID, "apk_snia_feedback_src: a scale radius that is not positive");
  if (const char *why = pack_problem(md, PACK_FLUID, fluid)) return pack_refused(ctx, "apk_snia_feedback_src", why);
  const PackView &v = md->view;
  const int64_t ncell = (int64_t)v.nx1 * v.nx2 * v.nx3 * v.nblocks;
  if (ncell == 0) return APK_OK;
  if (const char *why = pack_problem(md, PACK_STORED)) return pack_refused(ctx, "apk_snia_feedback_src", why);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_CLUSTER_SOURCES, s);
  const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
  if (fluid == APK_FLUID_GLMMHD)
    hipLaunchKernelGGL((snia_feedback_kernel<APK_FLUID_GLMMHD>), grid, block, 0, s, v, *eos, *cfg, block_xmin, beta_dt, ctx->d_flags);
  else
    hipLaunchKernelGGL((snia_feedback_kernel<APK_FLUID_EULER>), grid, block, 0, s, v, *eos, *cfg, block_xmin, beta_dt, ctx->d_flags);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "SNIa feedback source launch failed");
  return APK_OK;
}

int apk_cluster_split_src(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_stellar_cfg *stellar,
                          const apk_clips_cfg *clips, const apk_trig_box *boxes, int nboxes, int64_t max_box_cells,
                          const double *block_xmin, double *sums, apk_stream_t stream) {
  if (!ctx || !md || !eos || !block_xmin || !sums || nboxes < 0 || (nboxes > 0 && !boxes))
    return set_err(ctx, APK_ERR_INVALID, "apk_cluster_split_src: bad argument");
  if (const char *why = pack_problem(md, PACK_FLUID | PACK_3D | PACK_STORED, fluid)) return pack_refused(ctx, "apk_cluster_split_src", why);
  const PackView &v = md->view;
  if (v.nblocks == 0) return APK_OK;
  if (nboxes > v.nblocks || nboxes > 65535) return set_err(ctx, APK_ERR_INVALID, "apk_cluster_split_src: more entries than blocks, or than 65535");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_CLUSTER_SOURCES, s);
  APK_HIP_TRY(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 8 * (size_t)v.nblocks, s));
  if (nboxes == 0 || (!stellar && !clips)) return APK_OK;
  const int P = block_sum_groups(max_box_cells);
  const int rc = ctx->d_partial.reserve(ctx, (size_t)nboxes * P * 8, s);
  if (rc != APK_OK) return rc;
  const apk_stellar_cfg st = stellar ? *stellar : apk_stellar_cfg{};
  const apk_clips_cfg cl = clips ? *clips : apk_clips_cfg{};
  const dim3 grid((unsigned)P, (unsigned)nboxes), block(256);
  if (fluid == APK_FLUID_GLMMHD)
    hipLaunchKernelGGL((cluster_split_kernel<APK_FLUID_GLMMHD>), grid, block, 0, s, v, *eos, st, stellar ? 1 : 0, cl, clips ? 1 : 0, boxes,
                       block_xmin, ctx->d_partial.p, ctx->d_flags);
  else
    hipLaunchKernelGGL((cluster_split_kernel<APK_FLUID_EULER>), grid, block, 0, s, v, *eos, st, stellar ? 1 : 0, cl, clips ? 1 : 0, boxes,
                       block_xmin, ctx->d_partial.p, ctx->d_flags);
  block_sum_final_by_box<8>(ctx->d_partial.p, P, nboxes, v.nblocks, boxes, sums, s);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "cluster split source launch failed");
  return APK_OK;
}

}  // extern "C"
