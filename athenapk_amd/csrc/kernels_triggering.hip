// kernels_triggering.hip -- AGN triggering of the cluster problem: the reductions and removals over the accretion sphere
//   AGNTriggering::ReduceColdMass                    src/pgen/cluster/agn_triggering.cpp:124-198
//   AGNTriggering::ReduceBondiTriggeringQuantities   agn_triggering.cpp:202-264
//   AGNTriggering::RemoveBondiAccretedGas            agn_triggering.cpp:269-315
//   AddDensityToConsAtFixedVelTemp                   src/pgen/cluster/cluster_utils.hpp:40-52
// and the C-ABI entries of include/apk_amd.h (apk_agn_triggering_reduce, apk_agn_triggering_remove_bondi).
//
// Kernel structure.  The sphere is a few cells across at the centre of a large mesh, so no kernel here walks the mesh:
// the host hands over an active list (apk_trig_box: a block and an index box in its extended index space, ghost cells
// included, that holds every cell whose centre can lie inside the sphere) and the grid is (P, entries of the list).
// Each workgroup of 256 takes a fixed contiguous share of its box's cells, i fastest so that loads coalesce along a row
// of the box; a box is clipped to the block's arrays before it is used (active_box.hpp, shared with kernels_cluster_sources.hip).  The cell centre is cell_centre of
// cell_centre.hpp with the index counted from the first interior cell (negative in the lower ghost zone), the number the
// host's generators and a neighbouring block form for that cell; r2 = x * x + y * y + z * z and the test is the strict
// r2 < R^2.
//
// Reductions.  The deterministic block sum of block_sum.hpp with a box as the entry: P, a workgroup's share and the order
// of every addition are defined there (the tower's power contributions of kernels_feedback.hip add in the same order, in
// kernels of their own); no atomics, a block's sums are a function of the block and its box alone.  The kernels here
// supply the terms of a cell (four Bondi sums, or one cold mass and three zeros); the final kernel writes the four to the
// slots of the block an entry names.  Only interior cells enter
// the sums.  Blocks outside the list report zeros (the output is cleared first).
//
// In-place updates (COLD_GAS with removal in the reduction's launch, and the Bondi removal).  A lane owns its cell: it
// reads cons and prim of that cell only, applies AddDensityToConsAtFixedVelTemp on the stored primitives, re-derives the
// primitives with cons_to_prim_cell and stores both.  Ghost cells of the box are updated by position like interior ones
// (the reference's loops run over IndexDomain::entire): after the call a ghost cell inside the sphere holds what the
// neighbour's interior cell holds, and no exchange has to follow.  ConsToPrim's flags go into the device flag word.
//
// Measured (product build, GLM-MHD packs, one MI355X, device events, accretion radius of four cells; tools/triggering_cost.py,
// profiles/triggering_cost.jsonl; the engineer's own measurements, not predictions), each next to
// apk_magnetic_tower_power_contribs (a 24 B per cell walk over every cell) and a device copy of the boxes' bytes timed in the
// same run, 8 x 128^3 (8 boxes, 2744 cells) | one 64^3 block (1000 cells):
//   reduce, Bondi sums            12.6 us = 0.085 x the walk (147.8 us), 3.1 x the copy | 12.7 us = 0.68 x the walk (18.6 us), 2.9 x
//   reduce, cold gas + removal    12.8 us = 0.087 x the walk,            3.1 x the copy | 13.6 us = 0.73 x,                    3.2 x
//   Bondi removal                  5.8 us = 0.039 x the walk,            1.4 x the copy |  7.2 us = 0.39 x,                    1.7 x
// The copies take 4.1 - 4.4 us, launch latency themselves; the reduction is a clear and two dependent launches of a few
// workgroups: latency, not bandwidth.  Not measured: hydro packs, larger radii, one launch instead of three.
//
// Build forms.  The parity build (APK_FP_STRICT, -ffp-contract=off) agrees with a numpy restatement bit for bit on every
// stored value (products, quotients, sums and square roots only).  The product build compiles the same source.
#include <cmath>
#include <cstdint>

#include "active_box.hpp"
#include "apk_internal.hpp"
#include "block_sum.hpp"
#include "cell_centre.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

// ReduceBondiTriggeringQuantities (agn_triggering.cpp:234-256): grid (P, entries)
__global__ void __launch_bounds__(256) trig_reduce_bondi_kernel(PackView pv, double gamma, double accretion_radius,
                                                                const apk_trig_box *__restrict__ boxes,
                                                                const double *__restrict__ block_xmin, double *__restrict__ partial) {
  __shared__ double red[4][256];
  const int e = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  BoxShare s;
  if (box_share(pv, boxes, e, p, P, s)) {
    const apk_block_desc &bd = pv.blocks[s.b];
    const double vol = bd.dx[0] * bd.dx[1] * bd.dx[2];
    const double r2max = accretion_radius * accretion_radius;
    const int64_t sn = pv.sn;
    for (int64_t q = s.first + threadIdx.x; q < s.last; q += 256) {
      const TrigCell c = trig_cell(pv, s, bd, block_xmin, q);
      if (!c.interior || !(c.r2 < r2max)) continue;
      const double *__restrict__ w = bd.prim + c.off;
      const double rho = w[IDN * sn], v1 = w[IV1 * sn], v2 = w[IV2 * sn], v3 = w[IV3 * sn], pr = w[IPR * sn];
      const double cell_mass = rho * vol;
      acc[0] += cell_mass;
      acc[1] += cell_mass * rho;
      acc[2] += cell_mass * sqrt(v1 * v1 + v2 * v2 + v3 * v3);
      acc[3] += cell_mass * sqrt(gamma * pr / rho);
    }
  }
  block_sum_store<4, 4>(red, acc, e, p, P, partial);
}

// ReduceColdMass (agn_triggering.cpp:162-195): grid (P, entries)
template <int FLUID>
__global__ void __launch_bounds__(256) trig_reduce_cold_kernel(PackView pv, apk_eos eos, apk_agn_triggering_cfg c, double dt,
                                                               const apk_trig_box *__restrict__ boxes,
                                                               const double *__restrict__ block_xmin, double *__restrict__ partial,
                                                               unsigned *d_flags) {
  __shared__ double red[4][256];
  const int e = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned flags = 0;
  BoxShare s;
  if (box_share(pv, boxes, e, p, P, s)) {
    const apk_block_desc &bd = pv.blocks[s.b];
    const double vol = bd.dx[0] * bd.dx[1] * bd.dx[2];
    const double r2max = c.accretion_radius * c.accretion_radius;
    const int64_t sn = pv.sn;
    for (int64_t q = s.first + threadIdx.x; q < s.last; q += 256) {
      const TrigCell cell = trig_cell(pv, s, bd, block_xmin, q);
      if (!(cell.r2 < r2max)) continue;
      const double *__restrict__ w = bd.prim + cell.off;
      const double rho = w[IDN * sn];
      const double temp = c.mean_molecular_mass_by_kb * w[IPR * sn] / rho;
      if (!(temp <= c.cold_temp_thresh)) continue;
      if (cell.interior) acc[0] += rho * vol;
      if (c.remove_accreted_mass)
        flags |= add_density_fixed_vel_temp<FLUID>(eos, bd, cell.off, sn, [&](double rho_c) { return -rho_c / c.cold_t_acc * dt; });
    }
  }
  if (flags) atomicOr(d_flags, flags);
  block_sum_store<1, 4>(red, acc, e, p, P, partial);
}

// RemoveBondiAccretedGas (agn_triggering.cpp:296-314): grid (P, entries)
template <int FLUID>
__global__ void __launch_bounds__(256) trig_remove_bondi_kernel(PackView pv, apk_eos eos, double accretion_radius, double total_mass,
                                                                double accretion_rate, double dt,
                                                                const apk_trig_box *__restrict__ boxes,
                                                                const double *__restrict__ block_xmin, unsigned *d_flags) {
  const int e = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  unsigned flags = 0;
  BoxShare s;
  if (box_share(pv, boxes, e, p, P, s)) {
    const apk_block_desc &bd = pv.blocks[s.b];
    const double r2max = accretion_radius * accretion_radius;
    for (int64_t q = s.first + threadIdx.x; q < s.last; q += 256) {
      const TrigCell cell = trig_cell(pv, s, bd, block_xmin, q);
      if (!(cell.r2 < r2max)) continue;
      flags |= add_density_fixed_vel_temp<FLUID>(eos, bd, cell.off, pv.sn,
                                                 [&](double rho) { return -rho / total_mass * accretion_rate * dt; });
    }
  }
  if (flags) atomicOr(d_flags, flags);
}

}  // namespace
}  // namespace apk

using namespace apk;

extern "C" {

int apk_agn_triggering_reduce(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_agn_triggering_cfg *cfg,
                              const apk_trig_box *boxes, int nboxes, int64_t max_box_cells, const double *block_xmin, double dt,
                              double *sums, apk_stream_t stream) {
  if (!ctx || !md || !eos || !cfg || !block_xmin || !sums || nboxes < 0 || (nboxes > 0 && !boxes))
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_reduce: bad argument");
  if (const char *why = pack_problem(md, PACK_FLUID | PACK_3D | PACK_STORED, fluid)) return pack_refused(ctx, "apk_agn_triggering_reduce", why);
  if (cfg->mode != APK_TRIG_COLD_GAS && cfg->mode != APK_TRIG_BOOSTED_BONDI && cfg->mode != APK_TRIG_BOOTH_SCHAYE)
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_reduce: Unrecognized AGNTriggeringMode");
  const PackView &v = md->view;
  if (v.nblocks == 0) return APK_OK;
  if (nboxes > v.nblocks || nboxes > 65535) return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_reduce: more entries than blocks, or than 65535");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_TRIGGERING, s);
  APK_HIP_TRY(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 4 * (size_t)v.nblocks, s));
  if (nboxes == 0) return APK_OK;
  const int P = block_sum_groups(max_box_cells);
  const int rc = ctx->d_partial.reserve(ctx, (size_t)nboxes * P * 4, s);
  if (rc != APK_OK) return rc;
  const dim3 grid((unsigned)P, (unsigned)nboxes), block(256);
  if (cfg->mode == APK_TRIG_COLD_GAS) {  // (one sum; the other three slots are written as zeros)
    if (fluid == APK_FLUID_GLMMHD)
      hipLaunchKernelGGL((trig_reduce_cold_kernel<APK_FLUID_GLMMHD>), grid, block, 0, s, v, *eos, *cfg, dt, boxes, block_xmin, ctx->d_partial.p, ctx->d_flags);
    else
      hipLaunchKernelGGL((trig_reduce_cold_kernel<APK_FLUID_EULER>), grid, block, 0, s, v, *eos, *cfg, dt, boxes, block_xmin, ctx->d_partial.p, ctx->d_flags);
  } else {
    hipLaunchKernelGGL(trig_reduce_bondi_kernel, grid, block, 0, s, v, eos->gamma, cfg->accretion_radius, boxes, block_xmin, ctx->d_partial.p);
  }
  block_sum_final_by_box<4>(ctx->d_partial.p, P, nboxes, v.nblocks, boxes, sums, s);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "AGN triggering reduction launch failed");
  return APK_OK;
}

int apk_agn_triggering_remove_bondi(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, double accretion_radius,
                                    const apk_trig_box *boxes, int nboxes, int64_t max_box_cells, const double *block_xmin,
                                    double total_mass, double accretion_rate, double dt, apk_stream_t stream) {
  if (!ctx || !md || !eos || !block_xmin || nboxes < 0 || (nboxes > 0 && !boxes))
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_remove_bondi: bad argument");
  if (const char *why = pack_problem(md, PACK_FLUID | PACK_3D | PACK_STORED, fluid))
    return pack_refused(ctx, "apk_agn_triggering_remove_bondi", why);
  const PackView &v = md->view;
  if (v.nblocks == 0 || nboxes == 0) return APK_OK;
  if (nboxes > v.nblocks || nboxes > 65535)
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_remove_bondi: more entries than blocks, or than 65535");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_TRIGGERING, s);
  const dim3 grid((unsigned)block_sum_groups(max_box_cells), (unsigned)nboxes), block(256);
  if (fluid == APK_FLUID_GLMMHD)
    hipLaunchKernelGGL((trig_remove_bondi_kernel<APK_FLUID_GLMMHD>), grid, block, 0, s, v, *eos, accretion_radius, total_mass, accretion_rate,
                       dt, boxes, block_xmin, ctx->d_flags);
  else
    hipLaunchKernelGGL((trig_remove_bondi_kernel<APK_FLUID_EULER>), grid, block, 0, s, v, *eos, accretion_radius, total_mass, accretion_rate,
                       dt, boxes, block_xmin, ctx->d_flags);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "Bondi removal launch failed");
  return APK_OK;
}

}  // extern "C"
