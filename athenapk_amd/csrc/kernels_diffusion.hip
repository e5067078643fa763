// kernels_diffusion.hip -- the unsplit diffusive face fluxes of CalcDiffFluxes (src/hydro/diffusion/diffusion.cpp:18-53)
// and the diffusive time-step limit (src/hydro/hydro.cpp:935-949):
//   ThermalFluxIsoFixed      conduction.cpp:189-259   isotropic conduction with a fixed coefficient, no saturation
//   ThermalFluxGeneral       conduction.cpp:265-471   anisotropic conduction (fixed or Spitzer) and isotropic Spitzer:
//                                                     lim4 (MC) transverse gradients (diffusion.hpp:20-68), upwinded
//                                                     saturated flux, ThermalDiffusivity::Get (conduction.cpp:28-42)
//   MomentumDiffFluxIsoFixed viscosity.cpp:94-289     isotropic viscosity
//   OhmicDiffFluxIsoFixed    resistivity.cpp:91-230   Ohmic resistivity
//   EstimateConductionTimestep (general branch)  conduction.cpp:44-184, early returns included
//
// One launch per active direction adds every enabled process into flux[d] (never overwrites it) on the faces of
// interior cells, the reference's loop extents.  One lane owns one face: all primitives of the stencil are loaded
// first and shared by the processes, then the lane reads, updates and writes back its face's flux components -- no
// atomics.  Each process adds its contribution in the reference's order (conduction, viscosity, resistivity), so the
// strict (-ffp-contract=off) build is bit for bit the reference's arithmetic.
//
// Deviations, both at the last bit or below the reference's own definition:
//  - Ohmic resistivity's transverse derivatives divide by Xf(k+1) - Xf(k-1); a block descriptor carries no block
//    origin, so this uses 2 dx (the same number up to the rounding of the two face coordinates).
//  - ThermalFluxGeneral's x1 sweep reads the j +- 1 rows unconditionally, which a 1-D block does not have: here a
//    transverse gradient of an inactive direction is 0 (as the reference already does for dT/dz in 2-D).
//
// Bytes per face pass (what the launch must move; the floor, not a measurement): reads nprim primitives of the cell
// row it sweeps (neighbour rows hit the L2 / MALL) and reads + writes the touched flux components.  GLM-MHD with all
// three processes: 8 primitives (rho, v, p, B) + 6 flux components read and written = 64 + 96 = 160 B per cell and
// direction.
#include "apk_internal.hpp"
#include "diff_flux_face.hpp"
#include "hydro_math.hpp"
#include "wg_reduce.hpp"

namespace apk {

namespace {

// Face of direction DIR between cell L = (k,j,i) - e_DIR and R = (k,j,i): the arithmetic is diff_face
// (diff_flux_face.hpp), shared with the fused RKL2 sub-stage.
template <int DIR, int COND, bool VISC, bool RES, int COEFF>
__global__ void __launch_bounds__(256) diff_flux_kernel(PackView pv, DiffCoeffs c, int b0) {
  // faces of this direction: nx + 1 along DIR
  const int nfi = pv.nx1 + (DIR == 0), nfj = pv.nx2 + (DIR == 1), nfk = pv.nx3 + (DIR == 2);
  int io, jo;
  if (DIR == 0) {
    // x1 faces: nx1 + 1 per row -- rows laid end to end (along grid x, which has no 64 K limit) so that no workgroup
    // runs a 1-lane column
    const int64_t fl64 = (int64_t)blockIdx.x * 256 + threadIdx.y * 64 + threadIdx.x;
    if (fl64 >= (int64_t)nfi * nfj) return;
    const int f = (int)fl64;
    jo = f / nfi;
    io = f - jo * nfi;
  } else if (!rect_ij(nfi, nfj, io, jo)) {
    return;
  }
  const int b = b0 + (int)(blockIdx.z / nfk);  // (blocks b0 .. of this launch: grid z holds at most 65535)
  const int k = pv.ks + (int)(blockIdx.z % nfk), j = pv.js + jo, i = pv.is + io;
  const apk_block_desc blk = pv.blocks[b];
  const int64_t cell = k * pv.sk + j * pv.sj + i;
  const double *__restrict__ w = blk.prim + cell;
  const int64_t sn = pv.sn;
  double *__restrict__ fl = blk.flux[DIR] + cell;
  constexpr int b0v = (DIR == 0) ? IB2 : IB1, b1v = (DIR == 2) ? IB2 : IB3;
  // the lane reads its face's flux components, adds the processes (diff_face) and writes them back
  DiffFaceFlux f{{0.0, 0.0, 0.0}, {0.0, 0.0}, 0.0};
  if constexpr (VISC) {
    f.m[0] = fl[IM1 * sn];
    f.m[1] = fl[IM2 * sn];
    f.m[2] = fl[IM3 * sn];
  }
  if constexpr (RES) {
    f.b[0] = fl[b0v * sn];
    f.b[1] = fl[b1v * sn];
  }
  if constexpr (COND != COND_NONE || VISC || RES) f.e = fl[IEN * sn];
  double chiR = c.kappa, chiL = c.kappa;
  if constexpr (COEFF == COEFF_SPITZER) {
    const int64_t on = DIR == 0 ? 1 : (DIR == 1 ? pv.sj : pv.sk);  // R - L
    chiR = diff_chi<COEFF>(c, w[IPR * sn], w[IDN * sn]);
    chiL = diff_chi<COEFF>(c, w[IPR * sn - on], w[IDN * sn - on]);
  }
  diff_face<DIR, COND, VISC, RES>(w, sn, pv.sj, pv.sk, blk.dx, pv.ndim, c, chiR, chiL, f);
  if constexpr (VISC) {
    fl[IM1 * sn] = f.m[0];
    fl[IM2 * sn] = f.m[1];
    fl[IM3 * sn] = f.m[2];
  }
  if constexpr (RES) {
    fl[b0v * sn] = f.b[0];
    fl[b1v * sn] = f.b[1];
  }
  if constexpr (COND != COND_NONE || VISC || RES) fl[IEN * sn] = f.e;
}

// EstimateConductionTimestep, general branch (conduction.cpp:96-180), with chi = ThermalDiffusivity::Get of the cell:
// the minimum over interior cells of dx_d^2 / chi (COND_ISO_GEN: isotropic Spitzer, no TINY) or of
// dx_d^2 / (chi |B_d| / |B| cos(theta) + TINY) (COND_ANISO) into min_bits (positive doubles order like their bit
// patterns).  Grid = rect_grid(nx1, nx2, nx3 * nblocks).
template <int COND, int COEFF>
__global__ void __launch_bounds__(256) cond_dt_kernel(PackView pv, DiffCoeffs c, unsigned long long *min_bits, int b0) {
  int io, jo;
  const bool inside = rect_ij(pv.nx1, pv.nx2, io, jo);
  double m = 1.7976931348623157e308;
  if (inside) {
    const int b = b0 + (int)(blockIdx.z / pv.nx3), k = pv.ks + (int)(blockIdx.z % pv.nx3), j = pv.js + jo, i = pv.is + io;
    const apk_block_desc blk = pv.blocks[b];
    const double *__restrict__ w = blk.prim + (k * pv.sk + j * pv.sj + i);
    const int64_t sn = pv.sn, sj = pv.sj, sk = pv.sk;
    const int ndim = pv.ndim;
    auto T = [&](int64_t o) { return w[IPR * sn + o] / w[IDN * sn + o]; };
    const double rho = w[IDN * sn], p = w[IPR * sn];
    const double dTdx = 0.5 * (T(1) - T(-1)) / blk.dx[0];
    const double dTdy = ndim >= 2 ? 0.5 * (T(sj) - T(-sj)) / blk.dx[1] : 0.0;
    const double dTdz = ndim >= 3 ? 0.5 * (T(sk) - T(-sk)) / blk.dx[2] : 0.0;
    const double gradTmag = sqrt(dTdx * dTdx + dTdy * dTdy + dTdz * dTdz);
    const double chi = diff_chi<COEFF>(c, p, rho);
    if constexpr (COND == COND_ISO_GEN) {
      // no gradient: no constraint
      if (gradTmag != 0.0) {
        m = fmin(m, blk.dx[0] * blk.dx[0] / chi);
        if (ndim >= 2) m = fmin(m, blk.dx[1] * blk.dx[1] / chi);
        if (ndim >= 3) m = fmin(m, blk.dx[2] * blk.dx[2] / chi);
      }
    } else {
      const double bx = w[IB1 * sn], by = w[IB2 * sn], bz = w[IB3 * sn];
      const double bmag = sqrt(bx * bx + by * by + bz * bz);
      const double flux_sat = c.sat_prefac * sqrt(p / rho) * p;
      const double flux_classic = chi * rho * gradTmag;
      // no gradient, no field, or saturated (the hyperbolic limit covers it): no constraint
      if (gradTmag != 0.0 && bmag != 0.0 && !(flux_classic / flux_sat > 100.)) {
        const double costheta = fabs(bx * dTdx + by * dTdy + bz * dTdz) / (bmag * gradTmag);
        m = fmin(m, blk.dx[0] * blk.dx[0] / (chi * fabs(bx) / bmag * costheta + kTiny));
        if (ndim >= 2) m = fmin(m, blk.dx[1] * blk.dx[1] / (chi * fabs(by) / bmag * costheta + kTiny));
        if (ndim >= 3) m = fmin(m, blk.dx[2] * blk.dx[2] / (chi * fabs(bz) / bmag * costheta + kTiny));
      }
    }
  }
  wg_min_to_word(m, min_bits);
}

using DiffKernel = void (*)(PackView, DiffCoeffs, int);

template <int DIR, int COND, bool VISC, bool RES, int COEFF>
DiffKernel pick() {
  return diff_flux_kernel<DIR, COND, VISC, RES, COEFF>;
}

// the (mode, coefficient) pairs CalcDiffFluxes can dispatch to (diffusion.cpp:18-53)
template <int DIR>
DiffKernel pick_dir(int cond, int coeff, bool visc, bool res) {
#define APK_DIFF_PICK(C, K)                                               \
  if (cond == C && coeff == K) {                                          \
    if (visc && res) return pick<DIR, C, true, true, K>();                \
    if (visc) return pick<DIR, C, true, false, K>();                      \
    if (res) return pick<DIR, C, false, true, K>();                       \
    return pick<DIR, C, false, false, K>();                               \
  }
  APK_DIFF_PICK(COND_NONE, COEFF_FIXED)
  APK_DIFF_PICK(COND_ISO, COEFF_FIXED)
  APK_DIFF_PICK(COND_ANISO, COEFF_FIXED)
  APK_DIFF_PICK(COND_ISO_GEN, COEFF_SPITZER)
  APK_DIFF_PICK(COND_ANISO, COEFF_SPITZER)
#undef APK_DIFF_PICK
  return nullptr;
}

}  // namespace

// cond: apk_conduction; spitzer: NULL for a fixed coefficient kappa, else the Spitzer numbers (kappa is not read)
int launch_diff_fluxes(const PackView &pv, int cond, bool visc, bool res, double kappa, double sat_prefac, double nu,
                       double eta, const apk_spitzer_cfg *spitzer, hipStream_t s) {
  const DiffCoeffs c = diff_coeffs(cond, kappa, sat_prefac, nu, eta, spitzer);
  const int coeff = diff_coeff_kind(cond, spitzer);
  cond = diff_cond_mode(cond, spitzer);
  if (cond == COND_NONE && !visc && !res) return APK_OK;
  for (int d = 0; d < pv.ndim; ++d) {
    const DiffKernel k = d == 0 ? pick_dir<0>(cond, coeff, visc, res)
                                : (d == 1 ? pick_dir<1>(cond, coeff, visc, res) : pick_dir<2>(cond, coeff, visc, res));
    if (!k) return APK_ERR_INVALID;
    const int nfi = pv.nx1 + (d == 0), nfj = pv.nx2 + (d == 1), nfk = pv.nx3 + (d == 2);
    const int per = blocks_per_launch(nfk);
    for (int b0 = 0; b0 < pv.nblocks; b0 += per) {
      const int nb = pv.nblocks - b0 < per ? pv.nblocks - b0 : per;
      const dim3 grid = d == 0 ? dim3((unsigned)(((int64_t)nfi * nfj + 255) / 256), 1, (unsigned)(nfk * nb))
                               : rect_grid(nfi, nfj, nfk * nb);
      hipLaunchKernelGGL(k, grid, dim3(64, 4, 1), 0, s, pv, c, b0);
      if (hipGetLastError() != hipSuccess) return APK_ERR_DEVICE;
    }
  }
  return APK_OK;
}

// the general branch of EstimateConductionTimestep: anisotropic conduction (either coefficient) or isotropic Spitzer
int launch_cond_dt(const PackView &pv, int cond, double kappa, double sat_prefac, const apk_spitzer_cfg *spitzer,
                   unsigned long long *d_min_bits, hipStream_t s) {
  const DiffCoeffs c = diff_coeffs(cond, kappa, sat_prefac, 0.0, 0.0, spitzer);
  const int coeff = diff_coeff_kind(cond, spitzer);
  cond = diff_cond_mode(cond, spitzer);
  void (*k)(PackView, DiffCoeffs, unsigned long long *, int) = nullptr;
  if (cond == COND_ANISO) k = coeff == COEFF_SPITZER ? cond_dt_kernel<COND_ANISO, COEFF_SPITZER> : cond_dt_kernel<COND_ANISO, COEFF_FIXED>;
  if (cond == COND_ISO_GEN && coeff == COEFF_SPITZER) k = cond_dt_kernel<COND_ISO_GEN, COEFF_SPITZER>;
  if (!k) return APK_ERR_INVALID;
  const int per = blocks_per_launch(pv.nx3);
  for (int b0 = 0; b0 < pv.nblocks; b0 += per) {
    const int nb = pv.nblocks - b0 < per ? pv.nblocks - b0 : per;
    hipLaunchKernelGGL(k, rect_grid(pv.nx1, pv.nx2, pv.nx3 * nb), dim3(64, 4, 1), 0, s, pv, c, d_min_bits, b0);
    if (hipGetLastError() != hipSuccess) return APK_ERR_DEVICE;
  }
  return APK_OK;
}

}  // namespace apk
