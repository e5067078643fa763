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
// of the box; a box is clipped to the block's arrays before it is used.  The cell centre is centre() of cell_centre.hpp
// with the index counted from the first interior cell (negative in the lower ghost zone), the number the host's
// generators and a neighbouring block form for that cell; r2 = x * x + y * y + z * z and the test is the strict r2 < R^2.
//
// Reductions.  A lane adds its cells in index order, the workgroup reduces through a fixed LDS tree, and a second small
// kernel adds a block's P partials in order: no atomics, a block's sums are a function of the block and its box alone
// (the pattern of tower_contribs_kernel).  Only interior cells enter the sums.  Blocks outside the list report zeros (the
// output is cleared first).
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

#include "apk_internal.hpp"
#include "cell_centre.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

constexpr int kTrigCellsPerGroup = 4096, kTrigMaxGroups = 64;
inline int trig_groups(int64_t max_box_cells) {
  const int64_t p = (max_box_cells + kTrigCellsPerGroup - 1) / kTrigCellsPerGroup;
  return (int)(p < 1 ? 1 : (p > kTrigMaxGroups ? kTrigMaxGroups : p));
}

// the box of entry `e`, clipped to the block's arrays, and this workgroup's share [first, last) of its cells
struct BoxShare {
  int b, lo[3], n[3];
  int64_t first, last;
};
APK_DEV bool box_share(const PackView &pv, const apk_trig_box *__restrict__ boxes, int e, int p, int P, BoxShare &s) {
  const apk_trig_box bx = boxes[e];
  s.b = bx.block;
  if (s.b < 0 || s.b >= pv.nblocks) return false;
  const int ext[3] = {pv.ni, pv.nj, pv.nk};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int lo = bx.lo[d] < 0 ? 0 : bx.lo[d];
    const int hi = bx.hi[d] > ext[d] ? ext[d] : bx.hi[d];
    s.lo[d] = lo;
    s.n[d] = hi > lo ? hi - lo : 0;
  }
  const int64_t ncell = (int64_t)s.n[0] * s.n[1] * s.n[2];
  // a whole number of 256-cell rounds, the same for every workgroup of the box
  const int64_t share = ((ncell + P - 1) / P + 255) / 256 * 256;
  s.first = (int64_t)p * share;
  s.last = (s.first + share < ncell) ? s.first + share : ncell;
  return true;
}

// cell q of the share: its extended indices, offset, centre and whether it is an interior cell
struct TrigCell {
  int64_t off;
  double r2;
  bool interior;
};
APK_DEV TrigCell trig_cell(const PackView &pv, const BoxShare &s, const apk_block_desc &bd, const double *__restrict__ block_xmin,
                           int64_t q) {
  const int64_t nrow = s.n[0], nplane = nrow * s.n[1];
  const int kk = (int)(q / nplane);
  const int64_t r = q - (int64_t)kk * nplane;
  const int jj = (int)(r / nrow);
  const int ii = (int)(r - (int64_t)jj * nrow);
  const int i = s.lo[0] + ii, j = s.lo[1] + jj, k = s.lo[2] + kk;
  const double *corner = block_xmin + 3 * (int64_t)s.b;
  const double *mesh = block_xmin + 3 * (int64_t)pv.nblocks;
  const double x = centre(corner[0], mesh[0], bd.dx[0], i - pv.is);
  const double y = centre(corner[1], mesh[1], bd.dx[1], j - pv.js);
  const double z = centre(corner[2], mesh[2], bd.dx[2], k - pv.ks);
  TrigCell c;
  c.off = (int64_t)k * pv.sk + (int64_t)j * pv.sj + i;
  c.r2 = x * x + y * y + z * z;
  c.interior = i >= pv.is && i <= pv.ie && j >= pv.js && j <= pv.je && k >= pv.ks && k <= pv.ke;
  return c;
}

// AddDensityToConsAtFixedVelTemp (cluster_utils.hpp:40-52) on the stored primitives, then ConsToPrim, for one cell;
// density_of(rho): the density to add, from the stored density
template <int FLUID, typename F>
APK_DEV unsigned add_density_fixed_vel_temp(const apk_eos &eos, const apk_block_desc &bd, int64_t off, int64_t sn, F density_of) {
  constexpr int NV = nvars<FLUID>();
  double *__restrict__ up = bd.cons + off;
  double *__restrict__ wp = bd.prim + off;
  double u[NV], w[NV], di;
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    u[n] = up[n * sn];
    w[n] = wp[n * sn];
  }
  const double density = density_of(w[IDN]);
  u[IDN] += density;
  u[IM1] += density * w[IV1];
  u[IM2] += density * w[IV2];
  u[IM3] += density * w[IV3];
  u[IEN] += density * (0.5 * (sqr(w[IV1]) + sqr(w[IV2]) + sqr(w[IV3])) + 1 / (eos.gamma - 1.0) * w[IPR] / w[IDN]);
  const unsigned flags = cons_to_prim_cell<FLUID>(eos, u, w, di);
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    up[n * sn] = u[n];
    wp[n * sn] = w[n];
  }
  return flags;
}

// the workgroup's NS sums through a fixed LDS tree into partial[(e * P + p) * 4 + n]
template <int NS>
APK_DEV void reduce_store(double (&red)[4][256], const double (&acc)[4], int e, int p, int P, double *__restrict__ partial) {
#pragma unroll
  for (int n = 0; n < NS; ++n) red[n][threadIdx.x] = acc[n];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int n = 0; n < NS; ++n) red[n][threadIdx.x] += red[n][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int n = 0; n < 4; ++n) partial[((int64_t)e * P + p) * 4 + n] = n < NS ? red[n][0] : 0.0;
  }
}

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
  reduce_store<4>(red, acc, e, p, P, partial);
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
  reduce_store<1>(red, acc, e, p, P, partial);
}

// the P partials of every listed block, added in order: one lane per (entry, sum)
__global__ void __launch_bounds__(64) trig_reduce_final_kernel(const double *__restrict__ partial, int P, int nboxes, int nblocks,
                                                               const apk_trig_box *__restrict__ boxes, double *__restrict__ sums) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 4 * nboxes) return;
  const int e = q >> 2, n = q & 3;
  const int b = boxes[e].block;
  if (b < 0 || b >= nblocks) return;
  double sum = 0.0;
  for (int p = 0; p < P; ++p) sum += partial[((int64_t)e * P + p) * 4 + n];
  sums[4 * (int64_t)b + n] = sum;
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

const char *trig_pack_problem(const apk_pack *md, int fluid) {
  const PackView &v = md->view;
  if (v.nhydro != 5 && v.nhydro != 9) return "the pack is neither hydro nor GLM-MHD";
  if ((fluid == APK_FLUID_GLMMHD) != (v.nhydro == 9) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD))
    return "fluid does not match the pack";
  if (v.ndim != 3) return "the pack is not three-dimensional";
  for (int b = 0; b < v.nblocks; ++b)
    if (!md->h_blocks[b].prim || !md->h_blocks[b].cons) return "the pack needs cons and prim";
  return nullptr;
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
  if (const char *why = trig_pack_problem(md, fluid)) return set_err(ctx, APK_ERR_INVALID, (std::string("apk_agn_triggering_reduce: ") + why).c_str());
  if (cfg->mode != APK_TRIG_COLD_GAS && cfg->mode != APK_TRIG_BOOSTED_BONDI && cfg->mode != APK_TRIG_BOOTH_SCHAYE)
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_reduce: Unrecognized AGNTriggeringMode");
  const PackView &v = md->view;
  if (v.nblocks == 0) return APK_OK;
  if (nboxes > v.nblocks || nboxes > 65535) return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_reduce: more entries than blocks, or than 65535");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_TRIGGERING, s);
  APK_HIP_TRY(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 4 * (size_t)v.nblocks, s));
  if (nboxes == 0) return APK_OK;
  const int P = trig_groups(max_box_cells);
  const int rc = ensure_partial_doubles(ctx, (size_t)nboxes * P * 4);
  if (rc != APK_OK) return rc;
  const dim3 grid((unsigned)P, (unsigned)nboxes), block(256);
  if (cfg->mode == APK_TRIG_COLD_GAS) {
    if (fluid == APK_FLUID_GLMMHD)
      hipLaunchKernelGGL((trig_reduce_cold_kernel<APK_FLUID_GLMMHD>), grid, block, 0, s, v, *eos, *cfg, dt, boxes, block_xmin, ctx->d_partial, ctx->d_flags);
    else
      hipLaunchKernelGGL((trig_reduce_cold_kernel<APK_FLUID_EULER>), grid, block, 0, s, v, *eos, *cfg, dt, boxes, block_xmin, ctx->d_partial, ctx->d_flags);
  } else {
    hipLaunchKernelGGL(trig_reduce_bondi_kernel, grid, block, 0, s, v, eos->gamma, cfg->accretion_radius, boxes, block_xmin, ctx->d_partial);
  }
  hipLaunchKernelGGL(trig_reduce_final_kernel, dim3((unsigned)((4 * nboxes + 63) / 64)), dim3(64), 0, s, ctx->d_partial, P, nboxes,
                     v.nblocks, boxes, sums);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "AGN triggering reduction launch failed");
  return APK_OK;
}

int apk_agn_triggering_remove_bondi(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, double accretion_radius,
                                    const apk_trig_box *boxes, int nboxes, int64_t max_box_cells, const double *block_xmin,
                                    double total_mass, double accretion_rate, double dt, apk_stream_t stream) {
  if (!ctx || !md || !eos || !block_xmin || nboxes < 0 || (nboxes > 0 && !boxes))
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_remove_bondi: bad argument");
  if (const char *why = trig_pack_problem(md, fluid))
    return set_err(ctx, APK_ERR_INVALID, (std::string("apk_agn_triggering_remove_bondi: ") + why).c_str());
  const PackView &v = md->view;
  if (v.nblocks == 0 || nboxes == 0) return APK_OK;
  if (nboxes > v.nblocks || nboxes > 65535)
    return set_err(ctx, APK_ERR_INVALID, "apk_agn_triggering_remove_bondi: more entries than blocks, or than 65535");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_TRIGGERING, s);
  const dim3 grid((unsigned)trig_groups(max_box_cells), (unsigned)nboxes), block(256);
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
