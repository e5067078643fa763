// kernels_feedback.hip -- fixed-power AGN feedback of the cluster problem as unsplit sources:
//   AGNFeedback::FeedbackSrcTerm      src/pgen/cluster/agn_feedback.cpp:314-409   thermal dump, kinetic jet, ceilings
//   AddDensityToConsAtFixedVel        src/pgen/cluster/cluster_utils.hpp:22-34
//   JetCoords                         src/pgen/cluster/jet_coords.hpp:39-84       (feedback_math.hpp)
//   MagneticTower::AddSrcTerm         src/pgen/cluster/magnetic_tower.cpp:29-140  potential, curl, field, energy, density
//   MagneticTower::ReducePowerContribs  magnetic_tower.cpp:146-202                the two sums of the power scaling
// and the C-ABI entries of include/apk_amd.h (apk_agn_feedback_src, apk_magnetic_tower_src,
// apk_magnetic_tower_power_contribs).
//
// Kernel structure.  One lane per interior cell.  The view of a cell is cell_centre.hpp's, shared with kernels_gravity.hip
// and kernels_triggering.hip: cell_of names the lane's cell, cell_centre / cell_xyz give its centre (the host's number),
// pack_problem says what an entry asks of its pack.
// Which channels act (thermal_feedback > 0, thermal_density > 0, jet_density > 0, density_to_add > 0, the potential) are
// kernel arguments: uniform over the launch, scalar compares.  Lane-dependent are the sphere, the cylinders and the
// ceilings.  Ceilings that are +inf are not compiled into the launch (template flag CEIL, as LEAN in cons_to_prim_core).
//
// apk_agn_feedback_src.  The reference's lambda keeps cons and prim in memory and converts in place; here a lane holds
// both in registers, walks the same sequence -- sphere on the stored primitives, ConsToPrim / deposit / ConsToPrim in
// the cylinders, ceilings on whatever the primitives then are (outside the cylinders: the stored, stage-input ones),
// closing ConsToPrim -- and stores both once.  The reference traps when the closing pressure is not positive; the kernel
// latches APK_FLAG_AGN_NEG_PRESSURE (with the flags of its ConsToPrim calls) and the driver fails the step at the
// end-of-cycle read.  Bytes per cell: cons read and written, prim read and written: 160 B (hydro), 288 B (GLM-MHD).
//
// apk_magnetic_tower_src.  The reference fills a three-component potential one ghost layer deep and differences it in a
// second kernel (48 B per cell written and read again, plus the array).  Here there is no potential array: a cell
// evaluates the potential at its six neighbours' centres, cell_centre of the neighbour's index, so in the parity build every
// value is the number the array would have held and the curl (/ dx / 2.0, the reference's association) is the same.
// Six exponentials per cell and one more with mass injection.  Bytes per cell: prim B read (24 B), cons B, E and rho read
// and written (80 B): 104 B.  An LDS tile (one evaluation per cell plus halo) was not tried.
//
// apk_magnetic_tower_power_contribs.  Per block P = min(64, ceil(cells / 4096)) workgroups, each over a fixed contiguous
// share of the block's cells: a lane adds its cells in index order, the workgroup reduces through a fixed LDS tree, a
// second small kernel adds the block's P partial pairs in order.  No atomics: the pair of a block depends on nothing but
// the block.  The order is the one block_sum.hpp defines for the triggering reductions; this pair of kernels keeps its own
// statement of it and of the cell centre (see the note above tower_contribs_kernel).  Bytes per cell: prim B read, 24 B;
// one exponential.
//
// Measured (product build, GLM-MHD packs, one MI355X, device events, each next to a device copy of the kernel's bytes timed
// in the same run; profiles/feedback_cost.jsonl, tools/feedback_cost.py), 8 x 128^3 | one 64^3 block:
//   apk_agn_feedback_src               0.946 ms = 1.02 x its copy (5.1 TB/s of 288 B) | 11.4 us = 1.00 x    memory bound
//   apk_magnetic_tower_src             0.568 ms = 1.80 x its copy (3.1 TB/s of 104 B) | 12.9 us = 3.17 x    exp and memory about even
//   apk_magnetic_tower_power_contribs  0.147 ms = 1.98 x its copy (2.7 TB/s of 24 B)  | 18.9 us = 4.61 x    once per cycle
// Not measured: hydro packs, the donut potential, an LDS tile for the tower (at best the copy's 0.315 ms).
//
// Build forms.  The parity build (APK_FP_STRICT, -ffp-contract=off) agrees with a numpy restatement operation for
// operation, except for exp.  The product build compiles the same source with FMA contraction and reciprocal-based
// divides but without -fapprox-func (Makefile): the curl subtracts potentials that agree in their leading digits.
#include <cmath>
#include <cstdint>

#include "apk_internal.hpp"
#include "cell_centre.hpp"
#include "feedback_math.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

// AGNFeedback::FeedbackSrcTerm's lambda (agn_feedback.cpp:317-409), one interior cell per lane
template <int FLUID, bool CEIL>
__global__ void __launch_bounds__(256) agn_feedback_kernel(PackView pv, apk_eos eos, apk_agn_feedback_cfg c, apk_jet_coords jc,
                                                           const double *__restrict__ block_xmin, unsigned *d_flags) {
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
  for (int n = 0; n < NV; ++n) {
    u[n] = up[n * sn];
    w[n] = wp[n * sn];
  }
  unsigned flags = 0;

  // thermal feedback: the sphere r <= thermal_radius
  if (c.thermal_feedback > 0 || c.thermal_density > 0) {
    const double r2 = x * x + y * y + z * z;
    if (r2 <= c.thermal_radius * c.thermal_radius) {
      if (c.thermal_feedback > 0) u[IEN] += c.thermal_feedback;
      if (c.thermal_density > 0) {  // AddDensityToConsAtFixedVel: the stored velocity
        u[IDN] += c.thermal_density;
        u[IM1] += c.thermal_density * w[IV1];
        u[IM2] += c.thermal_density * w[IV2];
        u[IM3] += c.thermal_density * w[IV3];
        u[IEN] += c.thermal_density * (0.5 * (sqr(w[IV1]) + sqr(w[IV2]) + sqr(w[IV3])));
      }
    }
  }

  if (c.jet_density > 0) {
    double r, cos_t, sin_t, h;
    sim_cart_to_jet_cyl(jc, x, y, z, r, cos_t, sin_t, h);
    if (r < c.kinetic_jet_radius && fabs(h) >= c.kinetic_jet_offset && fabs(h) <= c.kinetic_jet_offset + c.kinetic_jet_thickness) {
      double ax, ay, az;
      jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, 0.0, 0.0, 1.0, ax, ay, az);
      const double sign_jet = (h > 0) ? 1 : -1;
      flags |= cons_to_prim_cell<FLUID>(eos, u, w, di);
      u[IDN] += c.jet_density;
      u[IM1] += c.jet_momentum * sign_jet * ax;
      u[IM2] += c.jet_momentum * sign_jet * ay;
      u[IM3] += c.jet_momentum * sign_jet * az;
      u[IEN] += c.jet_feedback;
      flags |= cons_to_prim_cell<FLUID>(eos, u, w, di);
    }
    if constexpr (CEIL) {
      const double gm1 = eos.gamma - 1.0;
      const double vceil2 = c.vceil * c.vceil;
      const double v2 = sqr(w[IV1]) + sqr(w[IV2]) + sqr(w[IV3]);
      if (vceil2 > 0 && v2 > vceil2) {
        const double v = sqrt(v2);
        u[IM1] *= c.vceil / v;
        u[IM2] *= c.vceil / v;
        u[IM3] *= c.vceil / v;
        w[IV1] *= c.vceil / v;
        w[IV2] *= c.vceil / v;
        w[IV3] *= c.vceil / v;
        u[IEN] -= 0.5 * w[IDN] * (v2 - vceil2);
      }
      const double internal_e = w[IPR] / (gm1 * w[IDN]);
      if (c.eceil > 0 && internal_e > c.eceil) {
        u[IEN] -= w[IDN] * (internal_e - c.eceil);
        w[IPR] = gm1 * w[IDN] * c.eceil;
      }
    }
  }

  flags |= cons_to_prim_cell<FLUID>(eos, u, w, di);
  if (!(w[IPR] > 0)) flags |= APK_FLAG_AGN_NEG_PRESSURE;
  if (flags) atomicOr(d_flags, flags);
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    up[n * sn] = u[n];
    wp[n * sn] = w[n];
  }
}

// MagneticTower::AddSrcTerm's two loops (magnetic_tower.cpp:83-139) in one, one interior cell per lane, GLM-MHD
__global__ void __launch_bounds__(256) magnetic_tower_kernel(PackView pv, apk_magnetic_tower_cfg t, apk_jet_coords jc,
                                                             const double *__restrict__ block_xmin, double field,
                                                             double density_to_add) {
  int b, i, j, k;
  int64_t off;
  if (!cell_of(pv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, b, i, j, k, off)) return;
  const apk_block_desc &bd = pv.blocks[b];
  const double dx1 = cell_width(bd, 0), dx2 = cell_width(bd, 1), dx3 = cell_width(bd, 2);
  const auto at = [&](int d, int n) { return cell_centre(bd, block_xmin, b, pv.nblocks, d, n); };
  const double x = at(0, i), xm = at(0, i - 1), xp = at(0, i + 1);
  const double y = at(1, j), ym = at(1, j - 1), yp = at(1, j + 1);
  const double z = at(2, k), zm = at(2, k - 1), zp = at(2, k + 1);
  const int64_t sn = pv.sn;
  const double *__restrict__ w = bd.prim + off;
  double *__restrict__ u = bd.cons + off;

  // A(n, k, j, i +- 1), A(n, k, j +- 1, i), A(n, k +- 1, j, i): what the stored array would hold there
  double a_im[3], a_ip[3], a_jm[3], a_jp[3], a_km[3], a_kp[3];
  tower_potential(t, jc, field, xm, y, z, a_im[0], a_im[1], a_im[2]);
  tower_potential(t, jc, field, xp, y, z, a_ip[0], a_ip[1], a_ip[2]);
  tower_potential(t, jc, field, x, ym, z, a_jm[0], a_jm[1], a_jm[2]);
  tower_potential(t, jc, field, x, yp, z, a_jp[0], a_jp[1], a_jp[2]);
  tower_potential(t, jc, field, x, y, zm, a_km[0], a_km[1], a_km[2]);
  tower_potential(t, jc, field, x, y, zp, a_kp[0], a_kp[1], a_kp[2]);
  const double b_x = (a_jp[2] - a_jm[2]) / dx2 / 2.0 - (a_kp[1] - a_km[1]) / dx3 / 2.0;
  const double b_y = (a_kp[0] - a_km[0]) / dx3 / 2.0 - (a_ip[2] - a_im[2]) / dx1 / 2.0;
  const double b_z = (a_ip[1] - a_im[1]) / dx1 / 2.0 - (a_jp[0] - a_jm[0]) / dx2 / 2.0;

  u[IB1 * sn] += b_x;
  u[IB2 * sn] += b_y;
  u[IB3 * sn] += b_z;
  // dE_B = B_old . b + 1/2 b^2, B_old the stored primitive field
  u[IEN * sn] += w[IB1 * sn] * b_x + w[IB2 * sn] * b_y + w[IB3 * sn] * b_z + 0.5 * (b_x * b_x + b_y * b_y + b_z * b_z);
  const double cell_delta_rho = density_to_add > 0.0 ? tower_density(t, jc, density_to_add, x, y, z) : 0.0;
  u[IDN * sn] += cell_delta_rho;
}

// The power contributions keep their own statement of the block sum of block_sum.hpp and of the cell centre (centre() on
// block_xmin's rows, as cell_xyz does), in the same order of additions: written with the shared helpers the kernel
// compiles to other code than it had (same instruction count within two, another register allocation), and a timing on one
// 64^3 block (18.6 us) does not repeat from process to process within the spread of its windows, so it cannot show the
// two equal.
constexpr int kContribCellsPerGroup = 4096, kContribMaxGroups = 64;
inline int contrib_groups(int64_t ncell_block) {
  const int64_t p = (ncell_block + kContribCellsPerGroup - 1) / kContribCellsPerGroup;
  return (int)(p < 1 ? 1 : (p > kContribMaxGroups ? kContribMaxGroups : p));
}

// MagneticTower::ReducePowerContribs (magnetic_tower.cpp:173-198): grid (P, nblocks); partial[(b * P + p) * 2 + {0, 1}]
__global__ void __launch_bounds__(256) tower_contribs_kernel(PackView pv, apk_magnetic_tower_cfg t, apk_jet_coords jc,
                                                             const double *__restrict__ block_xmin, double *__restrict__ partial) {
  __shared__ double red[2][256];
  const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  const apk_block_desc &bd = pv.blocks[b];
  const double *corner = block_xmin + 3 * (int64_t)b;
  const double *mesh = block_xmin + 3 * (int64_t)pv.nblocks;
  const int64_t nrow = pv.nx1, nplane = nrow * pv.nx2, nblk = nplane * pv.nx3;
  // this workgroup's share: a whole number of 256-cell rounds, the same for every workgroup of the block
  const int64_t share = ((nblk + P - 1) / P + 255) / 256 * 256;
  const int64_t first = (int64_t)p * share, last = (first + share < nblk) ? first + share : nblk;
  const double vol = bd.dx[0] * bd.dx[1] * bd.dx[2];
  const int64_t sn = pv.sn;
  double lin = 0.0, quad = 0.0;
  for (int64_t q = first + threadIdx.x; q < last; q += 256) {
    const int k = (int)(q / nplane);
    int64_t r = q - (int64_t)k * nplane;
    const int j = (int)(r / nrow);
    const int i = (int)(r - (int64_t)j * nrow);
    const double *__restrict__ w = bd.prim + (pv.ks + k) * pv.sk + (pv.js + j) * pv.sj + (pv.is + i);
    double b_x, b_y, b_z;
    tower_field(t, jc, 1.0, centre(corner[0], mesh[0], bd.dx[0], i), centre(corner[1], mesh[1], bd.dx[1], j),
                centre(corner[2], mesh[2], bd.dx[2], k), b_x, b_y, b_z);
    lin += (w[IB1 * sn] * b_x + w[IB2 * sn] * b_y + w[IB3 * sn] * b_z) * vol;
    quad += 0.5 * (b_x * b_x + b_y * b_y + b_z * b_z) * vol;
  }
  red[0][threadIdx.x] = lin;
  red[1][threadIdx.x] = quad;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[((int64_t)b * P + p) * 2 + 0] = red[0][0];
    partial[((int64_t)b * P + p) * 2 + 1] = red[1][0];
  }
}

// the block's P partial pairs, added in order: one lane per (block, sum)
__global__ void __launch_bounds__(64) tower_contribs_final_kernel(const double *__restrict__ partial, int P, int nblocks,
                                                                  double *__restrict__ contribs) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2 * nblocks) return;
  const int b = q >> 1, c = q & 1;
  double sum = 0.0;
  for (int p = 0; p < P; ++p) sum += partial[((int64_t)b * P + p) * 2 + c];
  contribs[q] = sum;
}

bool tower_ok(const apk_magnetic_tower_cfg &t) {
  if (t.potential != APK_TOWER_LI && t.potential != APK_TOWER_DONUT) return false;
  return t.l_scale > 0.0 && t.l_mass_scale >= 0.0;
}

}  // namespace
}  // namespace apk

using namespace apk;

extern "C" {

int apk_agn_feedback_src(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_agn_feedback_cfg *cfg,
                         const apk_jet_coords *jet, const double *block_xmin, apk_stream_t stream) {
  if (!ctx || !md || !eos || !cfg || !jet || !block_xmin) return set_err(ctx, APK_ERR_INVALID, "apk_agn_feedback_src: bad argument");
  const char *why = pack_problem(md, PACK_3D | PACK_STORED);
  if (!why) why = pack_problem(md, PACK_FLUID, fluid);  // (asked last here)
  if (why) return pack_refused(ctx, "apk_agn_feedback_src", why);
  const PackView &v = md->view;
  const int64_t ncell = (int64_t)v.nx1 * v.nx2 * v.nx3 * v.nblocks;
  if (ncell == 0) return APK_OK;
  // (nothing acts: the reference's loop would still run its closing ConsToPrim; so does this)
  const bool ceil = cfg->vceil != __builtin_inf() || cfg->eceil != __builtin_inf();
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
  ScopedTiming span(ctx, APK_T_AGN_FEEDBACK, s);
  if (fluid == APK_FLUID_GLMMHD) {
    if (ceil) hipLaunchKernelGGL((agn_feedback_kernel<APK_FLUID_GLMMHD, true>), grid, block, 0, s, v, *eos, *cfg, *jet, block_xmin, ctx->d_flags);
    else hipLaunchKernelGGL((agn_feedback_kernel<APK_FLUID_GLMMHD, false>), grid, block, 0, s, v, *eos, *cfg, *jet, block_xmin, ctx->d_flags);
  } else {
    if (ceil) hipLaunchKernelGGL((agn_feedback_kernel<APK_FLUID_EULER, true>), grid, block, 0, s, v, *eos, *cfg, *jet, block_xmin, ctx->d_flags);
    else hipLaunchKernelGGL((agn_feedback_kernel<APK_FLUID_EULER, false>), grid, block, 0, s, v, *eos, *cfg, *jet, block_xmin, ctx->d_flags);
  }
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "AGN feedback source launch failed");
  return APK_OK;
}

int apk_magnetic_tower_src(apk_ctx *ctx, const apk_pack *md, const apk_magnetic_tower_cfg *tower, const apk_jet_coords *jet,
                           const double *block_xmin, double field_to_add, double mass_to_add, apk_stream_t stream) {
  if (!ctx || !md || !tower || !jet || !block_xmin) return set_err(ctx, APK_ERR_INVALID, "apk_magnetic_tower_src: bad argument");
  if (field_to_add == 0 && mass_to_add == 0) return APK_OK;  // (magnetic_tower.cpp:36-38)
  if (const char *why = pack_problem(md, PACK_MHD | PACK_3D | PACK_STORED)) return pack_refused(ctx, "apk_magnetic_tower_src", why);
  if (!tower_ok(*tower))
    return set_err(ctx, APK_ERR_INVALID, "apk_magnetic_tower_src: Unknown magnetic tower potential, or a length scale that is not positive");
  if (!(mass_to_add == 0.0 || tower->l_mass_scale > 0.0))
    return set_err(ctx, APK_ERR_INVALID, "Trying to inject mass with the tower model but 0 mass lengthscale. Either disable tower mass "
                                          "injection or set positive lengthscale.");
  // (magnetic_tower.cpp:59-61; std::pow and M_PI as there)
  const double density_to_add = mass_to_add > 0.0 ? mass_to_add / (std::pow(tower->l_mass_scale, 3) * std::pow(M_PI, 3. / 2.)) : 0.0;
  const PackView &v = md->view;
  const int64_t ncell = (int64_t)v.nx1 * v.nx2 * v.nx3 * v.nblocks;
  if (ncell == 0) return APK_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_TOWER, s);
  hipLaunchKernelGGL(magnetic_tower_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, s, v, *tower, *jet, block_xmin,
                     field_to_add, density_to_add);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "magnetic tower source launch failed");
  return APK_OK;
}

int apk_magnetic_tower_power_contribs(apk_ctx *ctx, const apk_pack *md, const apk_magnetic_tower_cfg *tower,
                                      const apk_jet_coords *jet, const double *block_xmin, double *contribs,
                                      apk_stream_t stream) {
  if (!ctx || !md || !tower || !jet || !block_xmin || !contribs)
    return set_err(ctx, APK_ERR_INVALID, "apk_magnetic_tower_power_contribs: bad argument");
  if (const char *why = pack_problem(md, PACK_MHD | PACK_3D | PACK_STORED)) return pack_refused(ctx, "apk_magnetic_tower_power_contribs", why);
  if (!tower_ok(*tower))
    return set_err(ctx, APK_ERR_INVALID, "apk_magnetic_tower_power_contribs: Unknown magnetic tower potential, or a length scale that is not positive");
  const PackView &v = md->view;
  if (v.nblocks == 0) return APK_OK;
  if (v.nblocks > 65535) return set_err(ctx, APK_ERR_UNSUPPORTED, "apk_magnetic_tower_power_contribs: more than 65535 blocks in a pack");
  const int P = contrib_groups((int64_t)v.nx1 * v.nx2 * v.nx3);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ctx->d_partial.reserve(ctx, (size_t)v.nblocks * P * 2, s);
  if (rc != APK_OK) return rc;
  ScopedTiming span(ctx, APK_T_TOWER_CONTRIBS, s);
  hipLaunchKernelGGL(tower_contribs_kernel, dim3((unsigned)P, (unsigned)v.nblocks), dim3(256), 0, s, v, *tower, *jet, block_xmin,
                     ctx->d_partial.p);
  hipLaunchKernelGGL(tower_contribs_final_kernel, dim3((unsigned)((2 * v.nblocks + 63) / 64)), dim3(64), 0, s, ctx->d_partial.p, P,
                     v.nblocks, contribs);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "magnetic tower power contributions launch failed");
  return APK_OK;
}

}  // extern "C"
