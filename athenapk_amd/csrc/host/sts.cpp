// sts.cpp -- operator-split RKL2 super-time-stepping of the diffusive processes (diffusion/integrator = rkl2; Meyer,
// Balsara & Aslam 2014): AddSTSTasks of src/hydro/hydro_driver.cpp:168-344 on the standalone driver's buffers, and the
// host-only pieces of its C-ABI (stage count and coefficients; here rather than next to the kernels so that they are
// compiled without the kernels' reciprocal-math flags: the recursion is the reference's to the bit in both builds).
//
// Registers: "base" is the current state (s->cur, with the stored primitives), Y0 the u1 buffer -- free between the
// cycles' hyperbolic stages --, MY0 and Yjm2 two conserved-size buffers of their own.
#include <iostream>

#include "sim_internal.hpp"

namespace apk {
namespace host {

static int ensure_sts_registers(apk_sim *s) {
  if (s->my0_pack && s->yjm2_pack) return APK_OK;
  const int nlb = (int)s->mesh.local_gids.size();
  const size_t bytes = (size_t)s->nper * nlb * sizeof(double);
  double **bufs[2] = {&s->d_my0, &s->d_yjm2};
  apk_pack **packs[2] = {&s->my0_pack, &s->yjm2_pack};
  const char *tags[2] = {"sts_my0", "sts_yjm2"};
  for (int q = 0; q < 2; ++q) {
    if (!*bufs[q]) {
      SIM_TRY(s, dev_alloc(s, tags[q], bytes, bufs[q]));
      SIM_HIP(s, hipMemsetAsync(*bufs[q], 0, bytes, hs(s)));
    }
    std::vector<apk_block_desc> b(nlb);
    for (int lb = 0; lb < nlb; ++lb) {
      b[lb] = apk_block_desc{};
      b[lb].cons = s->blk(*bufs[q], lb);
      for (int d = 0; d < 3; ++d) b[lb].dx[d] = level_dx(s, block_level(s, lb), d);
    }
    apk_pack_desc d{};
    d.nblocks = nlb;
    d.nhydro = s->pkg.nhydro;
    d.nscalars = s->pkg.nscalars;
    for (int a = 0; a < 3; ++a) d.nx[a] = s->mesh.mb[a];
    d.ng = s->mesh.ng;
    if (s->mesh.pitch > 0) {
      d.stride[0] = s->mesh.sj;
      d.stride[1] = s->mesh.sk;
      d.stride[2] = s->mesh.sn;
    }
    d.blocks = b.data();
    SIM_TRY(s, apk_pack_create(s->ctx, &d, packs[q]));
  }
  return APK_OK;
}

void sts_free(apk_sim *s) {
  apk_pack_destroy(s->my0_pack);
  apk_pack_destroy(s->yjm2_pack);
  s->my0_pack = s->yjm2_pack = nullptr;
  dev_free(s, s->d_my0);
  dev_free(s, s->d_yjm2);
  s->d_my0 = s->d_yjm2 = nullptr;
}

// AddSTSTasks(tau).  Assumes that the ghost zones and the stored primitives of the current state are in sync, and
// guarantees it at the end: every sub-stage ends with a full ghost exchange (physical boundaries included) and
// ConsToPrim of whole blocks, the pair the flux-array stages run.
int sts_half_step(apk_sim *s, double tau) {
  HydroPackage &pkg = s->pkg;
  if (s->amr) return fail(s, APK_ERR_UNSUPPORTED, "super-time-stepping on refined meshes is not supported");
  // (the stages around it run through the flux arrays and leave a complete state; this completes what an accessor or a
  // switch of options may have left)
  SIM_TRY(s, sync_ghosts(s));
  if (s->exchange_pending || s->prim_stale || s->local_ghosts_stale || s->remote_ghosts_thin || s->x1_in_recv)
    return fail(s, APK_ERR_INVALID, "sts_half_step: ghost zones and primitives of the current state are not in sync");
  if (!(pkg.dt_diff > 0.0) || !(pkg.dt_diff < kHuge))
    return fail(s, APK_ERR_INVALID, "sts_half_step: no diffusive time-step estimate");
  int s_rkl = 0;
  if (apk_rkl2_num_stages(tau, pkg.dt_diff, &s_rkl) != APK_OK) return fail(s, APK_ERR_INVALID, "sts_half_step: bad tau / dt_diff");
  const double ratio = 2.0 * tau / pkg.dt_diff;
  if (s->rank == 0) {
    std::cout << "STS ratio: " << ratio << " Taking " << s_rkl << " steps." << std::endl;
    if (ratio > 400.1) std::cout << "WARNING: ratio is > 400. Proceed at own risk." << std::endl;
  }
  s->sts_last_s = s_rkl;
  s->sts_last_ratio = ratio;
  SIM_TRY(s, ensure_sts_registers(s));
  if (!s->sts_fused) SIM_TRY(s, ensure_flux_arrays(s));
  const size_t field_bytes = (size_t)s->nper * s->mesh.local_gids.size() * sizeof(double);
  // Y0 <- base (hydro_driver.cpp:193-208).  The conserved state only: no sub-stage reads the primitives of Y0 (every
  // flux is formed from those of base), which the reference copies along.
  SIM_HIP(s, hipMemcpyAsync(s->d_cons2[s->u1buf], s->d_cons2[s->cur], field_bytes, hipMemcpyDeviceToDevice, hs(s)));
  const apk_pack *base = s->mu0(), *y0 = s->mu1();
  for (int j = 1; j <= s_rkl; ++j) {
    apk_rkl2_coeffs k{};
    if (apk_rkl2_coefficients(s_rkl, j, &k.mu, &k.nu, &k.mu_tilde, &k.gamma_tilde) != APK_OK)
      return fail(s, APK_ERR_INVALID, "sts_half_step: coefficients");
    if (s->sts_fused) {
      const apk_rkl2_regs regs{y0, s->yjm2_pack, s->my0_pack};
      SIM_TRY(s, apk_rkl2_substage_fused_v2(s->ctx, base, &regs, &pkg.diff, pkg.spitzer_cfg(), &k, tau, j == 1 ? 1 : 0, s->stream));
    } else {
      // ResetFluxes, CalcDiffFluxes, then FluxDivergence + RKL2StepFirst or RKL2StepOther (hydro_driver.cpp:234-260, 306-326)
      for (int d = 0; d < s->mesh.ndim; ++d) SIM_HIP(s, hipMemsetAsync(s->d_flux[d], 0, field_bytes, hs(s)));
      SIM_TRY(s, apk_calc_diff_fluxes_v2(s->ctx, base, &pkg.diff, pkg.spitzer_cfg(), s->stream));
      if (j == 1) {
        SIM_TRY(s, apk_flux_divergence(s->ctx, base, s->my0_pack, s->stream));
        SIM_TRY(s, apk_rkl2_step_first(s->ctx, y0, base, s->yjm2_pack, s->my0_pack, s_rkl, tau, s->stream));
      } else {
        SIM_TRY(s, apk_rkl2_step_other(s->ctx, y0, base, s->yjm2_pack, s->my0_pack, k.mu, k.nu, k.mu_tilde, k.gamma_tilde, tau, s->stream));
      }
    }
    SIM_TRY(s, exchange_ghosts(s));
    SIM_TRY(s, fill_derived(s));
  }
  // (a time-step reduction the last hyperbolic stage may have started -- the turbulence kick -- is of a state that no
  // longer exists: the estimate at the end of the cycle measures the current one)
  s->stage_dt_pending = false;
  return APK_OK;
}

}  // namespace host
}  // namespace apk

extern "C" {

// ---- RKL2 super-time-stepping: stage count and coefficients (hydro_driver.cpp:176-181, 101-104, 276-291) -------------
int apk_rkl2_num_stages(double tau, double dt_diff, int *s_rkl) {
  if (!s_rkl || !(tau > 0.0) || !(dt_diff > 0.0) || !(tau / dt_diff < 1.0e15)) return APK_ERR_INVALID;
  // eq (21) of Meyer+2014 (hydro_driver.cpp:178-181)
  int s = static_cast<int>(0.5 * (std::sqrt(9.0 + 16.0 * tau / dt_diff) - 1.0)) + 1;
  if (s % 2 == 0) s += 1;  // ensure odd number of stages
  *s_rkl = s;
  return APK_OK;
}

int apk_rkl2_coefficients(int s_rkl, int j, double *mu, double *nu, double *mu_tilde, double *gamma_tilde) {
  if (s_rkl < 2 || j < 1 || j > s_rkl || !mu || !nu || !mu_tilde || !gamma_tilde) return APK_ERR_INVALID;
  const double sr = static_cast<double>(s_rkl);
  if (j == 1) {  // Meyer+2014 eq. (18) (hydro_driver.cpp:102-104)
    *mu = *nu = *gamma_tilde = 0.0;
    *mu_tilde = 4. / 3. / (sr * sr + sr - 2.);
    return APK_OK;
  }
  // Meyer+2012 eq. (16) (hydro_driver.cpp:277-291, 341-342)
  double b_j = 1. / 3., b_jm1 = 1. / 3., b_jm2 = 1. / 3.;
  const double w1 = 4. / (sr * sr + sr - 2.);
  for (int jj = 2; jj <= j; jj++) {
    const double q = static_cast<double>(jj);
    b_j = (q * q + q - 2.0) / (2 * q * (q + 1.0));
    *mu = (2.0 * q - 1.0) / q * b_j / b_jm1;
    *nu = -(q - 1.0) / q * b_j / b_jm2;
    *mu_tilde = *mu * w1;
    *gamma_tilde = -(1.0 - b_jm1) * *mu_tilde;  // -a_jm1*mu_tilde_j
    b_jm2 = b_jm1;
    b_jm1 = b_j;
  }
  return APK_OK;
}

int apk_sim_sts_info(const apk_sim *s, int *s_rkl, double *ratio, int *fused) {
  if (!s || !s_rkl || !ratio || !fused) return APK_ERR_INVALID;
  *s_rkl = s->sts_last_s;
  *ratio = s->sts_last_ratio;
  *fused = s->sts_fused ? 1 : 0;
  return APK_OK;
}

double apk_sim_rkl2_max_dt_ratio(const apk_sim *s) { return s ? s->pkg.rkl2_max_dt_ratio : -1.0; }

}  // extern "C"
