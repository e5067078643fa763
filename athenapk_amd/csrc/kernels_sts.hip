// kernels_sts.hip -- RKL2 super-time-stepping of the diffusive processes (diffusion/integrator = rkl2; Meyer, Balsara &
// Aslam 2014), one sub-stage of AddSTSTasks (src/hydro/hydro_driver.cpp:170-344).
//
// The array path, kernel for kernel what the reference runs on zeroed flux arrays after CalcDiffFluxes:
//   flux_divergence_kernel   Update::FluxDivergence            out = -div F           (hydro_driver.cpp:254)
//   rkl2_step_first_kernel   RKL2StepFirst                     hydro_driver.cpp:93-126
//   rkl2_step_other_kernel   RKL2StepOther                     hydro_driver.cpp:128-166
// and the fused sub-stage, which replaces { zero three flux arrays, three read-modify-write flux passes, the update }
// by ONE kernel: a lane owns an interior cell, forms the diffusive fluxes through its 2 ndim faces in registers
// (diff_face, the arithmetic of the flux-array pass, each face accumulated onto 0), takes their divergence in the
// term order of flux_div and applies RKL2StepFirst / RKL2StepOther.  It reads primitives and its own cell of the
// conserved registers and writes conserved registers only, so it runs in place.  Every face is formed twice (by the
// cells on either side): no flux array, no atomics, no LDS.
//
// Bytes per cell and sub-stage (what the launches must move; a model, not a measurement), GLM-MHD, all processes, 3-D:
//   array path   3 memsets 3 x 72 + 3 flux passes 3 x 160 (kernels_diffusion.hip) + update: 3 x 72 flux reads (the
//                upper faces hit the cache), 4 registers read, 2 written 6 x 72                          = 1344 B
//   fused        8 primitives read (neighbours hit the L2 / MALL) 64 + 4 registers read, 2 written 432   =  496 B
#include "apk_internal.hpp"
#include "diff_flux_face.hpp"
#include "flux_div.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

struct Rkl2Coeffs {
  double mu, nu, mu_tilde, gamma_tilde;  // (first sub-stage: mu_tilde = mu_tilde_1, the others unused)
};

// interior cell of this lane; grid = rect_grid(nx1, nx2, nx3 * (blocks of this launch)), block (64, 4)
APK_DEV bool sts_cell(const PackView &pv, int b0, int &b, int64_t &cell) {
  int io, jo;
  if (!rect_ij(pv.nx1, pv.nx2, io, jo)) return false;
  b = b0 + (int)(blockIdx.z / pv.nx3);  // (blocks b0 .. of this launch: grid z holds at most 65535)
  const int k = pv.ks + (int)(blockIdx.z % pv.nx3);
  cell = k * pv.sk + (pv.js + jo) * pv.sj + (pv.is + io);
  return true;
}

__global__ void __launch_bounds__(256) flux_divergence_kernel(PackView pv, const apk_block_desc *out, int b0) {
  int b;
  int64_t cell;
  if (!sts_cell(pv, b0, b, cell)) return;
  const apk_block_desc blk = pv.blocks[b];
  double *__restrict__ o = out[b].cons;
  double area[3], vol;
  block_areas(blk, area, vol);
  for (int n = 0; n < pv.nvar; ++n) {
    const int64_t idx = n * pv.sn + cell;
    o[idx] = flux_div(pv, blk, idx, area, vol);
  }
}

__global__ void __launch_bounds__(256) rkl2_step_first_kernel(PackView pv, const apk_block_desc *y0b, const apk_block_desc *yjm2b,
                                                              const apk_block_desc *my0b, double mu_tilde_1, double tau, int b0) {
  int b;
  int64_t cell;
  if (!sts_cell(pv, b0, b, cell)) return;
  const double *y0 = y0b[b].cons, *my0 = my0b[b].cons;
  double *yjm1 = pv.blocks[b].cons, *yjm2 = yjm2b[b].cons;
  for (int n = 0; n < pv.nvar; ++n) {
    const int64_t idx = n * pv.sn + cell;
    const double y = y0[idx];
    yjm1[idx] = y + mu_tilde_1 * tau * my0[idx];  // Y_1
    yjm2[idx] = y;                                // Y_0
  }
}

// pv: Yjm1 (its flux arrays hold the diffusive fluxes of Yjm1)
__global__ void __launch_bounds__(256) rkl2_step_other_kernel(PackView pv, const apk_block_desc *y0b, const apk_block_desc *yjm2b,
                                                              const apk_block_desc *my0b, Rkl2Coeffs k, double tau, int b0) {
  int b;
  int64_t cell;
  if (!sts_cell(pv, b0, b, cell)) return;
  const apk_block_desc blk = pv.blocks[b];
  const double *y0 = y0b[b].cons, *my0 = my0b[b].cons;
  double *yjm1 = blk.cons, *yjm2 = yjm2b[b].cons;
  double area[3], vol;
  block_areas(blk, area, vol);
  for (int n = 0; n < pv.nvar; ++n) {
    const int64_t idx = n * pv.sn + cell;
    const double myjm1 = flux_div(pv, blk, idx, area, vol);
    const double was = yjm1[idx];
    const double yj = k.mu * was + k.nu * yjm2[idx] + (1.0 - k.mu - k.nu) * y0[idx] + k.mu_tilde * tau * myjm1 +
                      k.gamma_tilde * tau * my0[idx];
    yjm2[idx] = was;
    yjm1[idx] = yj;
  }
}

// The fused sub-stage.  pv: Yjm1 (prim: its primitives, ghost zones in sync; cons: updated in place).
template <int NDIM, int COND, bool VISC, bool RES, int COEFF>
__global__ void __launch_bounds__(256) rkl2_substage_fused_kernel(PackView pv, const apk_block_desc *y0b, const apk_block_desc *yjm2b,
                                                                  const apk_block_desc *my0b, DiffCoeffs c, Rkl2Coeffs k, double tau,
                                                                  int first, int b0) {
  int b;
  int64_t cell;
  if (!sts_cell(pv, b0, b, cell)) return;
  const apk_block_desc blk = pv.blocks[b];
  const double *__restrict__ w = blk.prim + cell;
  const int64_t sn = pv.sn, sj = pv.sj, sk = pv.sk;
  // the faces of this cell, each accumulated onto 0 as the flux-array pass does onto a zeroed array: lo[d] the lower
  // d-face (R = this cell), hi[d] the upper one (R = the next cell)
  // (forming one direction at a time between scheduling barriers was tried to shorten the live ranges of the 3-D kernel
  // with every process: it spilled 156 B per lane where this form uses 488 registers and no scratch)
  DiffFaceFlux lo[3] = {}, hi[3] = {};
  // the diffusivity of this cell and of its 2 ndim neighbours, each formed once (7 evaluations for 6 faces; chi of a cell
  // is one value wherever it is formed, so the faces are those of the flux-array pass); a fixed coefficient: c.kappa
  auto chi = [&](int64_t o) { return diff_chi<COEFF>(c, w[IPR * sn + o], w[IDN * sn + o]); };
  const double chi0 = chi(0);
  diff_face<0, COND, VISC, RES>(w, sn, sj, sk, blk.dx, NDIM, c, chi0, chi(-1), lo[0]);
  diff_face<0, COND, VISC, RES>(w + 1, sn, sj, sk, blk.dx, NDIM, c, chi(1), chi0, hi[0]);
  if constexpr (NDIM >= 2) {
    diff_face<1, COND, VISC, RES>(w, sn, sj, sk, blk.dx, NDIM, c, chi0, chi(-sj), lo[1]);
    diff_face<1, COND, VISC, RES>(w + sj, sn, sj, sk, blk.dx, NDIM, c, chi(sj), chi0, hi[1]);
  }
  if constexpr (NDIM == 3) {
    diff_face<2, COND, VISC, RES>(w, sn, sj, sk, blk.dx, NDIM, c, chi0, chi(-sk), lo[2]);
    diff_face<2, COND, VISC, RES>(w + sk, sn, sj, sk, blk.dx, NDIM, c, chi(sk), chi0, hi[2]);
  }
  double area[3], vol;
  block_areas(blk, area, vol);
  // flux_div on register values: (x1, x0) the upper and lower x1-face flux of one variable, and so on
  auto div = [&](double x1, double x0, double y1, double y0, double z1, double z0) {
    double du = (area[0] * x1 - area[0] * x0);
    if constexpr (NDIM >= 2) du += (area[1] * y1 - area[1] * y0);
    if constexpr (NDIM == 3) du += (area[2] * z1 - area[2] * z0);
    return -du / vol;
  };
  // -div F per hydro variable (a variable no enabled process touches has zero flux, as in the zeroed arrays)
  double m[9];
  m[IDN] = div(0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
  m[IM1] = div(hi[0].m[0], lo[0].m[0], hi[1].m[0], lo[1].m[0], hi[2].m[0], lo[2].m[0]);
  m[IM2] = div(hi[0].m[1], lo[0].m[1], hi[1].m[1], lo[1].m[1], hi[2].m[1], lo[2].m[1]);
  m[IM3] = div(hi[0].m[2], lo[0].m[2], hi[1].m[2], lo[1].m[2], hi[2].m[2], lo[2].m[2]);
  m[IEN] = div(hi[0].e, lo[0].e, hi[1].e, lo[1].e, hi[2].e, lo[2].e);
  // field components: DIR 0 carries (IB2, IB3), DIR 1 (IB1, IB3), DIR 2 (IB1, IB2)
  m[IB1] = div(0.0, 0.0, hi[1].b[0], lo[1].b[0], hi[2].b[0], lo[2].b[0]);
  m[IB2] = div(hi[0].b[0], lo[0].b[0], 0.0, 0.0, hi[2].b[1], lo[2].b[1]);
  m[IB3] = div(hi[0].b[1], lo[0].b[1], hi[1].b[1], lo[1].b[1], 0.0, 0.0);
  m[IPS] = m[IDN];

  const double *y0 = y0b[b].cons + cell;
  double *my0 = my0b[b].cons + cell, *yjm1 = blk.cons + cell, *yjm2 = yjm2b[b].cons + cell;
  auto apply = [&](int n, double mn) {
    const int64_t idx = n * sn;
    if (first) {
      const double y = y0[idx];
      my0[idx] = mn;
      yjm1[idx] = y + k.mu_tilde * tau * mn;  // Y_1
      yjm2[idx] = y;                          // Y_0
    } else {
      const double was = yjm1[idx];
      const double yj = k.mu * was + k.nu * yjm2[idx] + (1.0 - k.mu - k.nu) * y0[idx] + k.mu_tilde * tau * mn +
                        k.gamma_tilde * tau * my0[idx];
      yjm2[idx] = was;
      yjm1[idx] = yj;
    }
  };
#pragma unroll
  for (int n = 0; n < 9; ++n)
    if (n < pv.nhydro) apply(n, m[n]);
  for (int n = pv.nhydro; n < pv.nvar; ++n) apply(n, m[IDN]);  // passive scalars: no diffusive flux
}

using FusedKernel = void (*)(PackView, const apk_block_desc *, const apk_block_desc *, const apk_block_desc *, DiffCoeffs,
                             Rkl2Coeffs, double, int, int);

template <int NDIM>
FusedKernel pick_fused(int cond, int coeff, bool visc, bool res) {
#define APK_STS_PICK(C, K)                                                            \
  if (cond == C && coeff == K) {                                                      \
    if (visc && res) return rkl2_substage_fused_kernel<NDIM, C, true, true, K>;       \
    if (visc) return rkl2_substage_fused_kernel<NDIM, C, true, false, K>;             \
    if (res) return rkl2_substage_fused_kernel<NDIM, C, false, true, K>;              \
    return rkl2_substage_fused_kernel<NDIM, C, false, false, K>;                      \
  }
  APK_STS_PICK(COND_NONE, COEFF_FIXED)
  APK_STS_PICK(COND_ISO, COEFF_FIXED)
  APK_STS_PICK(COND_ANISO, COEFF_FIXED)
  APK_STS_PICK(COND_ISO_GEN, COEFF_SPITZER)
  APK_STS_PICK(COND_ANISO, COEFF_SPITZER)
#undef APK_STS_PICK
  return nullptr;
}

// one launch per chunk of blocks: grid z = nx3 x (blocks) within 65535
template <class Launch>
int for_block_chunks(const PackView &pv, Launch launch) {
  const int per = blocks_per_launch(pv.nx3);
  for (int b0 = 0; b0 < pv.nblocks; b0 += per) {
    const int nb = pv.nblocks - b0 < per ? pv.nblocks - b0 : per;
    launch(rect_grid(pv.nx1, pv.nx2, pv.nx3 * nb), b0);
    if (hipGetLastError() != hipSuccess) return APK_ERR_DEVICE;
  }
  return APK_OK;
}

}  // namespace

int launch_flux_divergence(const PackView &pv, const apk_block_desc *out, hipStream_t s) {
  return for_block_chunks(pv, [&](dim3 grid, int b0) {
    hipLaunchKernelGGL(flux_divergence_kernel, grid, dim3(64, 4, 1), 0, s, pv, out, b0);
  });
}

int launch_rkl2_step_first(const PackView &yjm1, const apk_block_desc *y0, const apk_block_desc *yjm2, const apk_block_desc *my0,
                           double mu_tilde_1, double tau, hipStream_t s) {
  return for_block_chunks(yjm1, [&](dim3 grid, int b0) {
    hipLaunchKernelGGL(rkl2_step_first_kernel, grid, dim3(64, 4, 1), 0, s, yjm1, y0, yjm2, my0, mu_tilde_1, tau, b0);
  });
}

int launch_rkl2_step_other(const PackView &yjm1, const apk_block_desc *y0, const apk_block_desc *yjm2, const apk_block_desc *my0,
                           double mu, double nu, double mu_tilde, double gamma_tilde, double tau, hipStream_t s) {
  const Rkl2Coeffs k{mu, nu, mu_tilde, gamma_tilde};
  return for_block_chunks(yjm1, [&](dim3 grid, int b0) {
    hipLaunchKernelGGL(rkl2_step_other_kernel, grid, dim3(64, 4, 1), 0, s, yjm1, y0, yjm2, my0, k, tau, b0);
  });
}

// cond, spitzer: as launch_diff_fluxes
int launch_rkl2_substage_fused(const PackView &yjm1, const apk_block_desc *y0, const apk_block_desc *yjm2, const apk_block_desc *my0,
                               int cond, bool visc, bool res, double kappa, double sat_prefac, double nu_visc, double eta,
                               const apk_spitzer_cfg *spitzer, double mu, double nu, double mu_tilde, double gamma_tilde,
                               double tau, bool first, hipStream_t s) {
  const DiffCoeffs c = diff_coeffs(cond, kappa, sat_prefac, nu_visc, eta, spitzer);
  const int coeff = diff_coeff_kind(cond, spitzer);
  cond = diff_cond_mode(cond, spitzer);
  const Rkl2Coeffs k{mu, nu, mu_tilde, gamma_tilde};
  const FusedKernel kern = yjm1.ndim == 1 ? pick_fused<1>(cond, coeff, visc, res)
                                          : (yjm1.ndim == 2 ? pick_fused<2>(cond, coeff, visc, res)
                                                            : pick_fused<3>(cond, coeff, visc, res));
  if (!kern) return APK_ERR_INVALID;
  return for_block_chunks(yjm1, [&](dim3 grid, int b0) {
    hipLaunchKernelGGL(kern, grid, dim3(64, 4, 1), 0, s, yjm1, y0, yjm2, my0, c, k, tau, first ? 1 : 0, b0);
  });
}

}  // namespace apk
