// kernels_gravity.hip -- the static gravitational field of the cluster problem as an unsplit source:
//   ClusterGravity::g_from_r        src/pgen/cluster/cluster_gravity.hpp:173-201   NFW + Hernquist BCG + point-mass SMBH
//   GravitationalFieldSrcTerm       src/hydro/srcterms/gravitational_field.hpp:25-64
// and the C-ABI entries of include/apk_amd.h (apk_gravity_src, apk_gravity_g_from_r).
//
// Kernel structure.  One lane per interior cell, lanes laid along x1 and rows flattened one after the other (cell_of, as
// in kernels_cooling.hip), so that a wave reads and writes whole stretches of rows and a short or odd row leaves no lane
// idle but those past the last cell of the pack.  Which of the three components act is a kernel argument: the branches
// are uniform over the launch (scalar compares), no lane diverges on them.  The only lane-dependent select is r == 0.
//
// Bytes per cell (what the launch must move; the floor, not a measurement): the stored primitives rho, v1, v2, v3 are
// read (32 B), the conserved M1, M2, M3, E are read and written (64 B): 96 B per cell, 201 MB on 8 x 128^3.  Memory
// bound: per cell one sqrt, one log (NFW), five divides and about 40 other fp64 operations.  The per-block corner and
// cell widths (9 doubles per block) are read through the cached path: a wave touches at most two blocks.
// Measured (product build, one MI355X, device events; profiles/gravity_cost.jsonl): 7.5 us on one
// 64^3 block (0.029 ns per cell), 0.308 ms on 8 x 128^3 (0.018 ns per cell, 5.2 TB/s of the 96 B: 83 % of the 6.29 TB/s
// stream rate of DESIGN.md section 7.0).  Not measured: GLM-MHD packs (same bytes, a longer variable stride).
//
// Cell centres.  The centre is the number the problem generator used on the host, xc() of host/sim_pgen.cpp, rebuilt
// from the blocks' lower interior corners: cell_of and cell_xyz of cell_centre.hpp, the view of a cell that
// kernels_feedback.hip and kernels_triggering.hip share; pack_problem of the same header is the entry's pack check.
//
// Build forms.  The parity build (APK_FP_STRICT, -ffp-contract=off) keeps the reference's association order with IEEE
// divides and roots: it agrees with a numpy restatement operation for operation, except for log, the one step that is
// not correctly rounded.  The product build compiles the same source with FMA contraction and reciprocal-based divides
// (-freciprocal-math) but, like kernels_cooling.hip, without -fapprox-func: log(1 + r / r_s) - r / (r + r_s) cancels
// to r / r_s of its terms at small radii, and an approximate log would leave the product build's 1e-12.
#include <cmath>
#include <cstdint>

#include "apk_internal.hpp"
#include "cell_centre.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

// ClusterGravity::g_from_r (cluster_gravity.hpp:173-201)
APK_DEV double g_from_r(const apk_cluster_gravity &c, double r_in) {
  const double r = (r_in < c.smoothing_r) ? c.smoothing_r : r_in;  // std::max(r_in, smoothing_r_)
  const double r2 = r * r;
  double g_r = 0;
  if (c.include_nfw) g_r += c.g_const_nfw * (log(1 + r / c.r_nfw_s) - r / (r + c.r_nfw_s)) / r2;
  if (c.which_bcg == APK_BCG_HERNQUIST) g_r += c.g_const_bcg / ((1 + r / c.r_bcg_s) * (1 + r / c.r_bcg_s));
  if (c.include_smbh) g_r += c.g_const_smbh / r2;
  return g_r;
}

// GravitationalFieldSrcTerm (gravitational_field.hpp:40-63), one interior cell per lane
__global__ void __launch_bounds__(256) gravity_src_kernel(PackView pv, apk_cluster_gravity c, const double *__restrict__ block_xmin,
                                                          double beta_dt) {
  int b, i, j, k;
  int64_t off;
  if (!cell_of(pv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, b, i, j, k, off)) return;
  const apk_block_desc &bd = pv.blocks[b];
  double x, y, z;
  cell_xyz(bd, block_xmin, b, pv.nblocks, i, j, k, x, y, z);
  const int64_t sn = pv.sn;
  const double *__restrict__ w = bd.prim + off;
  double *__restrict__ u = bd.cons + off;

  const double r = sqrt(x * x + y * y + z * z);
  const double g_r = g_from_r(c, r);
  const double den = w[IDN * sn];
  const double src = (r == 0) ? 0 : beta_dt * den * g_r / r;
  u[IM1 * sn] -= src * x;
  u[IM2 * sn] -= src * y;
  u[IM3 * sn] -= src * z;
  u[IEN * sn] -= src * (x * w[IV1 * sn] + y * w[IV2 * sn] + z * w[IV3 * sn]);
}

__global__ void __launch_bounds__(256) gravity_g_kernel(apk_cluster_gravity c, const double *__restrict__ r, double *__restrict__ g,
                                                        int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g[i] = g_from_r(c, r[i]);
}

bool gravity_ok(const apk_cluster_gravity &c) {
  if (c.which_bcg != APK_BCG_NONE && c.which_bcg != APK_BCG_HERNQUIST) return false;
  if (c.include_nfw && !(c.r_nfw_s > 0.0)) return false;
  if (c.which_bcg == APK_BCG_HERNQUIST && !(c.r_bcg_s > 0.0)) return false;
  return true;
}

}  // namespace
}  // namespace apk

using namespace apk;

extern "C" {

int apk_gravity_src(apk_ctx *ctx, const apk_pack *md, const apk_cluster_gravity *gravity, const double *block_xmin,
                    double beta_dt, apk_stream_t stream) {
  if (!ctx || !md || !gravity || !block_xmin) return set_err(ctx, APK_ERR_INVALID, "apk_gravity_src: bad argument");
  if (!gravity_ok(*gravity)) return set_err(ctx, APK_ERR_INVALID, "apk_gravity_src: Unknown BCG type or a scale radius that is not positive");
  if (const char *why = pack_problem(md, 0)) return pack_refused(ctx, "apk_gravity_src", why);
  const PackView &v = md->view;
  const int64_t ncell = (int64_t)v.nx1 * v.nx2 * v.nx3 * v.nblocks;
  if (ncell == 0) return APK_OK;  // (an empty pack is not asked for its arrays, nor any pack for three dimensions)
  if (const char *why = pack_problem(md, PACK_STORED)) return pack_refused(ctx, "apk_gravity_src", why);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScopedTiming span(ctx, APK_T_GRAVITY, s);
  hipLaunchKernelGGL(gravity_src_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, s, v, *gravity, block_xmin, beta_dt);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "gravity source launch failed");
  return APK_OK;
}

int apk_gravity_g_from_r(apk_ctx *ctx, const apk_cluster_gravity *gravity, const double *r, double *g, int64_t n,
                         apk_stream_t stream) {
  if (!ctx || !gravity || n < 0 || (n > 0 && (!r || !g))) return set_err(ctx, APK_ERR_INVALID, "apk_gravity_g_from_r: bad argument");
  if (!gravity_ok(*gravity)) return set_err(ctx, APK_ERR_INVALID, "apk_gravity_g_from_r: Unknown BCG type or a scale radius that is not positive");
  if (n == 0) return APK_OK;
  hipLaunchKernelGGL(gravity_g_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *gravity, r,
                     g, n);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "gravity g_from_r launch failed");
  return APK_OK;
}

}  // extern "C"
