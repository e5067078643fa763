// hse_check.cpp -- stand-alone host program for the cluster problem's model (csrc/host/cluster_model.cpp): builds the
// hydrostatic sphere of inputs/cluster_hse.in on the reference's test mesh, one 32^3 block's own radial mesh and that
// block's initial state, and exercises the two failures the model raises.  No GPU, no Python; meant to be compiled with
// sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/cluster/hse_check.cpp athenapk_amd/csrc/host/cluster_model.cpp -o /tmp/hse_check && /tmp/hse_check
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../athenapk_amd/csrc/host/cluster.hpp"

using namespace apk;

int main() {
  // src/units.hpp in the deck's code units (1 Mpc, 1e14 Msun, 1 Gyr)
  const double L = 3.0856775809623245e+24, M = 1.98841586e+47, T = 3.15576e+16;
  const double E = M * L * L / (T * T);
  const double kpc = 3.0856775809623245e+21 / L, mpc = 3.0856775809623245e+24 / L, msun = 1.98841586e+33 / M;
  const double km_s = 1e5 / (L / T), kev = 1.60218e-9 / E, cm = 1.0 / L, g = 1.0 / M;
  const double He = 0.25;

  ClusterGravityInput gi;
  gi.include_nfw_g = gi.include_smbh_g = true;
  gi.which_bcg_g = APK_BCG_HERNQUIST;
  gi.gravitational_constant = 6.67408e-08 / (std::pow(L, 3) / (M * std::pow(T, 2)));
  gi.hubble_parameter = 70 * km_s / mpc;
  gi.m_nfw_200 = 1e15 * msun, gi.c_nfw = 6.0;
  gi.m_bcg_s = 1e11 * msun, gi.r_bcg_s = 4 * kpc, gi.m_smbh = 1e8 * msun, gi.g_smoothing_radius = 1e-6;

  HeSphere sp;
  sp.gravity = cluster_gravity_constants(gi);
  sp.k_0 = 10 * kev * cm * cm, sp.k_100 = 150 * kev * cm * cm, sp.r_k = 100 * kpc, sp.alpha_k = 1.1;
  sp.mh = 1.007947 * 1.660538921e-24 / M, sp.k_boltzmann = 1.3806488e-16 / E;
  sp.mu = 1 / (He * 3. / 4. + (1 - He) * 2), sp.mu_e = 1 / (He * 2. / 4. + (1 - He));
  sp.r_fix = 2 * mpc, sp.rho_fix = 1e-28 * g / (cm * cm * cm), sp.r_sampling = 4.0;

  // the deck's profile on the reference's test mesh, with its derived columns
  const HeProfile test = he_generate_profile(sp, 1e-3 * kpc, 4000 * kpc, 4000);
  std::vector<double> col(9 * (size_t)test.n_r);
  test.columns(col.data());
  std::printf("test profile: %d radii, P(r_start) = %.6e, P(r_end) = %.6e, T(100 kpc) = %.4e K\n", test.n_r, test.p.front(),
              test.p.back(), sp.T_from_rho_P(test.rho_from_r(0.1), test.P_from_r(0.1)));

  // block (0, 0, 0) of the deck's 64^3 mesh in 32^3 blocks over [-0.1, 0.1]^3: its radial mesh and initial state
  const int mb = 32;
  const double xmin = -0.1, dx[3] = {0.2 / 64, 0.2 / 64, 0.2 / 64};
  std::vector<double> x(mb);
  for (int i = 0; i < mb; ++i) x[i] = xmin + ((0.0 + (double)i) + 0.5) * dx[0];
  const HeProfile prof = he_generate_block_profile(sp, x.data(), mb, x.data(), mb, x.data(), mb, dx);
  const double gm1 = 5.0 / 3.0 - 1.0;
  std::vector<double> rho((size_t)mb * mb * mb), en(rho.size());
  double mass = 0.0, rho_min = 1e300, rho_max = 0.0;
  for (int k = 0; k < mb; ++k)
    for (int j = 0; j < mb; ++j)
      for (int i = 0; i < mb; ++i) {
        const double r = std::sqrt(x[i] * x[i] + x[j] * x[j] + x[k] * x[k]);
        const size_t q = ((size_t)k * mb + j) * mb + i;
        rho[q] = prof.rho_from_r(r);
        en[q] = prof.P_from_r(r) / gm1;
        mass += rho[q] * dx[0] * dx[1] * dx[2];
        rho_min = std::fmin(rho_min, rho[q]);
        rho_max = std::fmax(rho_max, rho[q]);
      }
  std::printf("block profile: %d radii from %.6e to %.6e; block mass %.6e, rho in [%.6e, %.6e]\n", prof.n_r, prof.r_start,
              prof.r_end, mass, rho_min, rho_max);
  if (!(rho_min > 0.0) || !std::isfinite(mass)) return 1;

  // the two failures, with the reference's wording
  int caught = 0;
  try {
    (void)he_generate_profile(sp, 1e-3 * kpc, 1500 * kpc, 100);  // r_fix = 2 Mpc is outside
  } catch (const std::runtime_error &e) {
    caught += std::string(e.what()).find("does not contain r_fix_") != std::string::npos;
  }
  for (const double r : {prof.r_end + 1.0, -1.0, std::nan("")}) {
    try {
      (void)prof.P_from_r(r);
    } catch (const std::runtime_error &e) {
      caught += std::string(e.what()).find("PRhoProfile::P_from_r R(i_r) to R_(i_r+1) does not contain r") != std::string::npos;
    }
  }
  std::printf("failures raised: %d of 4\n", caught);
  return caught == 4 ? 0 : 1;
}
