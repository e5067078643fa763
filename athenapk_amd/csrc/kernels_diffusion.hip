// kernels_diffusion.hip -- the unsplit diffusive face fluxes of CalcDiffFluxes (src/hydro/diffusion/diffusion.cpp:18-53)
// and the diffusive time-step limit (src/hydro/hydro.cpp:935-949), fixed coefficients only:
//   ThermalFluxIsoFixed      conduction.cpp:189-259   isotropic conduction, no saturation
//   ThermalFluxGeneral       conduction.cpp:265-471   anisotropic conduction: lim4 (MC) transverse gradients
//                                                     (diffusion.hpp:20-68), upwinded saturated flux
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
#include "hydro_math.hpp"

namespace apk {

namespace {

enum { COND_NONE = 0, COND_ISO = 1, COND_ANISO = 2 };

struct DiffCoeffs {
  double kappa;       // thermal_diff_coeff_code
  double sat_prefac;  // conduction_sat_prefac (5 phi for a fixed coefficient, hydro.cpp:595-604)
  double nu;          // mom_diff_coeff_code
  double eta;         // ohm_diff_coeff_code
};

// limiters::minmod / mc / lim2 / lim4 (diffusion.hpp:20-68), std::min / std::max spelled out
APK_DEV double minmod(double a, double b) {
  if (a * b > 0.0) return (a > 0.0) ? ((b < a) ? b : a) : ((a < b) ? b : a);
  return 0.0;
}
APK_DEV double mc_lim(double a, double b) { return minmod(2.0 * minmod(a, b), (a + b) / 2.0); }
APK_DEV double lim4(double a, double b, double c, double d) { return mc_lim(mc_lim(a, b), mc_lim(c, d)); }

// Face of direction DIR between cell L = (k,j,i) - e_DIR and R = (k,j,i).  All loads go through `w` (the primitives,
// const restrict): the compiler shares identical loads between the processes since no store precedes them.
template <int DIR, int COND, bool VISC, bool RES>
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
  const int64_t off[3] = {1, pv.sj, pv.sk};
  const int64_t on = off[DIR];  // R - L
  const double dxn = blk.dx[DIR];
  const int ndim = pv.ndim;
  // transverse axes in increasing order (the order the reference adds their terms in)
  constexpr int ta = (DIR == 0) ? 1 : 0;
  constexpr int tb = (DIR == 2) ? 1 : 2;
  const bool act_a = ta < ndim, act_b = tb < ndim;
  const int64_t oa = act_a ? off[ta] : 0, ob = act_b ? off[tb] : 0;
  auto P = [&](int v, int64_t o) { return w[v * sn + o]; };  // o relative to R

  double *__restrict__ fl = blk.flux[DIR] + cell;
  // ---- conduction ------------------------------------------------------------------------------------------------
  double q_cond = 0.0;
  if constexpr (COND == COND_ISO) {
    const double tR = P(IPR, 0) / P(IDN, 0), tL = P(IPR, -on) / P(IDN, -on);
    const double dTdn = (tR - tL) / dxn;
    const double denf = 0.5 * (P(IDN, 0) + P(IDN, -on));
    q_cond = c.kappa * denf * dTdn;  // flux -= q
  } else if constexpr (COND == COND_ANISO) {
    auto T = [&](int64_t o) { return P(IPR, o) / P(IDN, o); };
    double g[3];
    g[DIR] = (T(0) - T(-on)) / dxn;
    g[ta] = act_a ? lim4(T(oa) - T(0), T(0) - T(-oa), T(-on + oa) - T(-on), T(-on) - T(-on - oa)) / blk.dx[ta] : 0.0;
    g[tb] = act_b ? lim4(T(ob) - T(0), T(0) - T(-ob), T(-on + ob) - T(-on), T(-on) - T(-on - ob)) / blk.dx[tb] : 0.0;
    const double denf = 0.5 * (P(IDN, 0) + P(IDN, -on));
    const double tdf = 0.5 * (c.kappa + c.kappa);
    const double bx = 0.5 * (P(IB1, -on) + P(IB1, 0));
    const double by = 0.5 * (P(IB2, -on) + P(IB2, 0));
    const double bz = ndim >= 3 ? 0.5 * (P(IB3, -on) + P(IB3, 0)) : 0.0;
    double bmag = sqrt(bx * bx + by * by + bz * bz);
    bmag = (bmag < kTiny) ? kTiny : bmag;
    const double bn = (DIR == 0 ? bx : (DIR == 1 ? by : bz)) / bmag;
    const double bdg = (bx * g[0] + by * g[1] + bz * g[2]) / bmag;
    const double fc = -tdf * denf * bdg * bn;
    const double fcm = fabs(tdf * denf * bdg);
    const double pL = P(IPR, -on), pR = P(IPR, 0);
    double fsat;
    if (fc > 0.0) {
      fsat = c.sat_prefac * sqrt(pL / denf) * pL;
    } else if (fc < 0.0) {
      fsat = c.sat_prefac * sqrt(pR / denf) * pR;
    } else {
      const double presf = 0.5 * (pR + pL);
      fsat = c.sat_prefac * sqrt(presf / denf) * presf;
    }
    q_cond = (fsat / (fsat + fcm)) * fc;  // flux += q
  }
  // ---- viscosity -------------------------------------------------------------------------------------------------
  double fv[3] = {0.0, 0.0, 0.0}, nud = 0.0, q_visc = 0.0;
  if constexpr (VISC) {
    constexpr int vn = IV1 + DIR, va = IV1 + ta, vb = IV1 + tb;
    // normal component: 4/3 d vn/dn - 2/3 (d va/da + d vb/db); transverse: d vt/dn + d vn/dt
    auto tsum = [&](int v, int64_t o) { return (P(v, o) + P(v, o - on)) - (P(v, -o) + P(v, -o - on)); };
    fv[DIR] = 4.0 * (P(vn, 0) - P(vn, -on)) / (3.0 * dxn);
    fv[ta] = (P(va, 0) - P(va, -on)) / dxn;
    fv[tb] = (P(vb, 0) - P(vb, -on)) / dxn;
    if (act_a) {
      fv[DIR] -= tsum(va, oa) / (6.0 * blk.dx[ta]);
      fv[ta] += tsum(vn, oa) / (4.0 * blk.dx[ta]);
    }
    if (act_b) {
      fv[DIR] -= tsum(vb, ob) / (6.0 * blk.dx[tb]);
      fv[tb] += tsum(vn, ob) / (4.0 * blk.dx[tb]);
    }
    nud = 0.5 * c.nu * (P(IDN, 0) + P(IDN, -on));
    q_visc = 0.5 * nud *
             ((P(IV1, -on) + P(IV1, 0)) * fv[0] + (P(IV2, -on) + P(IV2, 0)) * fv[1] + (P(IV3, -on) + P(IV3, 0)) * fv[2]);
  }
  // ---- Ohmic resistivity -----------------------------------------------------------------------------------------
  double fb[2] = {0.0, 0.0}, q_res = 0.0;  // the two transverse field fluxes, in increasing component order
  if constexpr (RES) {
    const double eta = c.eta;
    auto dn = [&](int v) { return (P(v, 0) - P(v, -on)) / dxn; };
    auto dt = [&](int v, int t, bool act, int64_t o) {
      return act ? (0.5 * (P(v, o - on) + P(v, o)) - 0.5 * (P(v, -o - on) + P(v, -o))) / (2.0 * blk.dx[t]) : 0.0;
    };
    auto bs = [&](int v) { return P(v, -on) + P(v, 0); };
    if constexpr (DIR == 0) {
      const double j2 = dt(IB1, 2, act_b, ob) - dn(IB3);  // d3B1 - d1B3
      const double j3 = dn(IB2) - dt(IB1, 1, act_a, oa);  // d1B2 - d2B1
      fb[0] = -eta * j3;                                  // IB2
      fb[1] = eta * j2;                                   // IB3
      q_res = 0.5 * eta * (bs(IB3) * j2 - bs(IB2) * j3);
    } else if constexpr (DIR == 1) {
      const double j3 = dt(IB2, 0, act_a, oa) - dn(IB1);  // d1B2 - d2B1
      const double j1 = dn(IB3) - dt(IB2, 2, act_b, ob);  // d2B3 - d3B2
      fb[0] = eta * j3;                                   // IB1
      fb[1] = -eta * j1;                                  // IB3
      q_res = 0.5 * eta * (bs(IB1) * j3 - bs(IB3) * j1);
    } else {
      const double j1 = dt(IB3, 1, act_b, ob) - dn(IB2);  // d2B3 - d3B2
      const double j2 = dn(IB1) - dt(IB3, 0, act_a, oa);  // d3B1 - d1B3
      fb[0] = -eta * j2;                                  // IB1
      fb[1] = eta * j1;                                   // IB2
      q_res = 0.5 * eta * (bs(IB2) * j1 - bs(IB1) * j2);
    }
  }
  // ---- accumulate into the face flux in the reference's order ---------------------------------------------------
  if constexpr (VISC) {
    fl[IM1 * sn] -= nud * fv[0];
    fl[IM2 * sn] -= nud * fv[1];
    fl[IM3 * sn] -= nud * fv[2];
  }
  if constexpr (RES) {
    constexpr int b0 = (DIR == 0) ? IB2 : IB1, b1 = (DIR == 2) ? IB2 : IB3;
    fl[b0 * sn] += fb[0];
    fl[b1 * sn] += fb[1];
  }
  if constexpr (COND != COND_NONE || VISC || RES) {
    double e = fl[IEN * sn];
    if constexpr (COND == COND_ISO) e -= q_cond;
    if constexpr (COND == COND_ANISO) e += q_cond;
    if constexpr (VISC) e -= q_visc;
    if constexpr (RES) e += q_res;
    fl[IEN * sn] = e;
  }
}

APK_DEV double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
  return v;
}

// EstimateConductionTimestep, general branch (conduction.cpp:96-180), anisotropic with a fixed coefficient: the
// minimum over interior cells of dx_d^2 / (kappa |B_d| / |B| cos(theta) + TINY) into min_bits (positive doubles order
// like their bit patterns).  Grid = rect_grid(nx1, nx2, nx3 * nblocks).
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
    const double bx = w[IB1 * sn], by = w[IB2 * sn], bz = w[IB3 * sn];
    const double bmag = sqrt(bx * bx + by * by + bz * bz);
    const double flux_sat = c.sat_prefac * sqrt(p / rho) * p;
    const double flux_classic = c.kappa * rho * gradTmag;
    // no gradient, no field, or saturated (the hyperbolic limit covers it): no constraint
    if (gradTmag != 0.0 && bmag != 0.0 && !(flux_classic / flux_sat > 100.)) {
      const double costheta = fabs(bx * dTdx + by * dTdy + bz * dTdz) / (bmag * gradTmag);
      m = fmin(m, blk.dx[0] * blk.dx[0] / (c.kappa * fabs(bx) / bmag * costheta + kTiny));
      if (ndim >= 2) m = fmin(m, blk.dx[1] * blk.dx[1] / (c.kappa * fabs(by) / bmag * costheta + kTiny));
      if (ndim >= 3) m = fmin(m, blk.dx[2] * blk.dx[2] / (c.kappa * fabs(bz) / bmag * costheta + kTiny));
    }
  }
  m = wave_min_d(m);
  __shared__ double part[4];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if ((tid & 63) == 0) part[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    const double r = fmin(fmin(part[0], part[1]), fmin(part[2], part[3]));
    atomicMin(min_bits, (unsigned long long)__double_as_longlong(r));
  }
}

using DiffKernel = void (*)(PackView, DiffCoeffs, int);

// blocks per launch: grid z = (planes per block) x (blocks) stays within the 65535 a grid dimension may hold
inline int blocks_per_launch(int planes) { return planes > 0 ? (65535 / planes > 0 ? 65535 / planes : 1) : 1; }

template <int DIR, int COND, bool VISC, bool RES>
DiffKernel pick() {
  return diff_flux_kernel<DIR, COND, VISC, RES>;
}

template <int DIR>
DiffKernel pick_dir(int cond, bool visc, bool res) {
#define APK_DIFF_PICK(C)                                                  \
  if (cond == C) {                                                        \
    if (visc && res) return pick<DIR, C, true, true>();                   \
    if (visc) return pick<DIR, C, true, false>();                         \
    if (res) return pick<DIR, C, false, true>();                          \
    return pick<DIR, C, false, false>();                                  \
  }
  APK_DIFF_PICK(COND_NONE)
  APK_DIFF_PICK(COND_ISO)
  APK_DIFF_PICK(COND_ANISO)
#undef APK_DIFF_PICK
  return nullptr;
}

}  // namespace

// cond: 0 none, 1 isotropic (fixed), 2 anisotropic (fixed); coefficients as in DiffCoeffs
int launch_diff_fluxes(const PackView &pv, int cond, bool visc, bool res, double kappa, double sat_prefac, double nu,
                       double eta, hipStream_t s) {
  const DiffCoeffs c{kappa, sat_prefac, nu, eta};
  if (cond == COND_NONE && !visc && !res) return APK_OK;
  for (int d = 0; d < pv.ndim; ++d) {
    const DiffKernel k = d == 0 ? pick_dir<0>(cond, visc, res) : (d == 1 ? pick_dir<1>(cond, visc, res) : pick_dir<2>(cond, visc, res));
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

int launch_cond_dt(const PackView &pv, double kappa, double sat_prefac, unsigned long long *d_min_bits, hipStream_t s) {
  const DiffCoeffs c{kappa, sat_prefac, 0.0, 0.0};
  const int per = blocks_per_launch(pv.nx3);
  for (int b0 = 0; b0 < pv.nblocks; b0 += per) {
    const int nb = pv.nblocks - b0 < per ? pv.nblocks - b0 : per;
    hipLaunchKernelGGL(cond_dt_kernel, rect_grid(pv.nx1, pv.nx2, pv.nx3 * nb), dim3(64, 4, 1), 0, s, pv, c, d_min_bits, b0);
    if (hipGetLastError() != hipSuccess) return APK_ERR_DEVICE;
  }
  return APK_OK;
}

}  // namespace apk
