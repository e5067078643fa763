// cluster.hpp -- the host-side model of the cluster problem, free of the driver: ClusterGravity's constants and
// g_from_r (src/pgen/cluster/cluster_gravity.hpp), the ACCEPT-like entropy profile (cluster/entropy_profiles.hpp) and
// the hydrostatic-equilibrium sphere with its RK4 pressure profile (cluster/hydrostatic_equilibrium_sphere.{hpp,cpp}),
// restated in the reference's operation order.  Plain C++ (host/cluster_model.cpp): a stand-alone program can link it.
#pragma once

#include <string>
#include <vector>

#include "../../../include/apk_amd.h"

namespace apk {

// what ClusterGravity's constructor reads (code units)
struct ClusterGravityInput {
  bool include_nfw_g = false, include_smbh_g = false;
  int which_bcg_g = APK_BCG_NONE;
  double gravitational_constant = 0, hubble_parameter = 0;
  double m_nfw_200 = 0, c_nfw = 0, alpha_bcg_s = 0, beta_bcg_s = 0, m_bcg_s = 0, r_bcg_s = 0, m_smbh = 0;
  double g_smoothing_radius = 0;
};
// the constants rolled together in ClusterGravity's constructor (cluster_gravity.hpp:56-107, 137-164)
apk_cluster_gravity cluster_gravity_constants(const ClusterGravityInput &in);
// ClusterGravity::g_from_r (cluster_gravity.hpp:173-201)
double cluster_g_from_r(const apk_cluster_gravity &c, double r_in);

// HydrostaticEquilibriumSphere<ClusterGravity, ACCEPTEntropyProfile> and its members
struct HeSphere {
  apk_cluster_gravity gravity{};
  double k_0 = 0, k_100 = 0, r_k = 0, alpha_k = 0;  // ACCEPTEntropyProfile
  double mh = 0, k_boltzmann = 0, mu = 0, mu_e = 0;
  double r_fix = 0, rho_fix = 0, r_sampling = 4.0;

  double K_from_r(double r) const;
  double P_from_rho_K(double rho, double k) const;
  double rho_from_P_K(double p, double k) const;
  double n_from_rho(double rho) const;
  double ne_from_rho(double rho) const;
  double T_from_rho_P(double rho, double p) const;
  double dP_dr(double r, double p) const;  // dP_dr_from_r_P_functor
  double step_rk4(double t0, double t1, double y0) const;
};

// PRhoProfile: the radial mesh, the pressures on it, and the interpolation.  The reference's PARTHENON_FAIL and
// Kokkos::abort conditions throw std::runtime_error with the reference's wording.
struct HeProfile {
  HeSphere sphere;
  std::vector<double> r, p;
  int n_r = 0;
  double r_start = 0, r_end = 0;
  double P_from_r(double r) const;
  double rho_from_r(double r) const;
  // PRhoProfile::write_to_ostream's columns: out[9][n_r] = r, P, K, rho, n, ne, T, g, dP_dr
  void columns(double *out) const;
};

// generate_P_rho_profile(r_start, r_end, n_r) (hydrostatic_equilibrium_sphere.cpp:185-253)
HeProfile he_generate_profile(const HeSphere &sphere, double r_start, double r_end, unsigned int n_r);
// generate_P_rho_profile(ib, jb, kb, coords) (hydrostatic_equilibrium_sphere.cpp:124-180): the block's own radial mesh
// from its interior cell centres x1[n1], x2[n2], x3[n3] and cell widths, extended to include r_fix
HeProfile he_generate_block_profile(const HeSphere &sphere, const double *x1, int n1, const double *x2, int n2,
                                    const double *x3, int n3, const double dx[3]);

}  // namespace apk
