// active_box.hpp -- what the kernels that launch over an active list share (kernels_triggering.hip,
// kernels_cluster_sources.hip): the box of an entry and a workgroup's share of it, the view of a cell of that share, and
// AddDensityToConsAtFixedVelTemp (src/pgen/cluster/cluster_utils.hpp:40-52).  The grid is (P, entries of the list), see
// block_sum.hpp.
#pragma once

#include <cstdint>

#include "apk_internal.hpp"
#include "block_sum.hpp"
#include "cell_centre.hpp"
#include "hydro_math.hpp"

namespace apk {

// the box of entry `e`, clipped to the block's arrays (interior_only: to its interior cells), and this workgroup's share
// [first, last) of its cells
struct BoxShare {
  int b, lo[3], n[3];
  int64_t first, last;
};
APK_DEV bool box_share(const PackView &pv, const apk_trig_box *__restrict__ boxes, int e, int p, int P, BoxShare &s,
                       bool interior_only = false) {
  const apk_trig_box bx = boxes[e];
  s.b = bx.block;
  if (s.b < 0 || s.b >= pv.nblocks) return false;
  const int first[3] = {interior_only ? pv.is : 0, interior_only ? pv.js : 0, interior_only ? pv.ks : 0};
  const int end[3] = {interior_only ? pv.ie + 1 : pv.ni, interior_only ? pv.je + 1 : pv.nj, interior_only ? pv.ke + 1 : pv.nk};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int lo = bx.lo[d] < first[d] ? first[d] : bx.lo[d];
    const int hi = bx.hi[d] > end[d] ? end[d] : bx.hi[d];
    s.lo[d] = lo;
    s.n[d] = hi > lo ? hi - lo : 0;
  }
  block_sum_share((int64_t)s.n[0] * s.n[1] * s.n[2], p, P, s.first, s.last);
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
  const int64_t nrow = s.n[0];
  int ii, jj, kk;
  box_ijk(q, nrow, nrow * s.n[1], ii, jj, kk);
  const int i = s.lo[0] + ii, j = s.lo[1] + jj, k = s.lo[2] + kk;
  double x, y, z;
  cell_xyz(bd, block_xmin, s.b, pv.nblocks, i - pv.is, j - pv.js, k - pv.ks, x, y, z);
  TrigCell c;
  c.off = (int64_t)k * pv.sk + (int64_t)j * pv.sj + i;
  c.r2 = x * x + y * y + z * z;
  c.interior = i >= pv.is && i <= pv.ie && j >= pv.js && j <= pv.je && k >= pv.ks && k <= pv.ke;
  return c;
}

// AddDensityToConsAtFixedVelTemp (cluster_utils.hpp:40-52): `density` added to the cell's conserved values u at the
// velocity and temperature of its primitives w
template <int NV>
APK_DEV void add_density_fixed_vel_temp_regs(const apk_eos &eos, double density, double (&u)[NV], const double (&w)[NV]) {
  u[IDN] += density;
  u[IM1] += density * w[IV1];
  u[IM2] += density * w[IV2];
  u[IM3] += density * w[IV3];
  u[IEN] += density * (0.5 * (sqr(w[IV1]) + sqr(w[IV2]) + sqr(w[IV3])) + 1 / (eos.gamma - 1.0) * w[IPR] / w[IDN]);
}

// ... on the stored primitives, then ConsToPrim, for one cell in memory; density_of(rho): the density to add, from the
// stored density
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
  add_density_fixed_vel_temp_regs<NV>(eos, density_of(w[IDN]), u, w);
  const unsigned flags = cons_to_prim_cell<FLUID>(eos, u, w, di);
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    up[n * sn] = u[n];
    wp[n * sn] = w[n];
  }
  return flags;
}

}  // namespace apk
