// cluster_model.cpp -- see cluster.hpp.  Every expression keeps the reference's association order, so that a restatement
// in another language (tests/cluster_reference.py) differs only where its libm does (pow, log).
#include <algorithm>
#include <cmath>
#include <limits>
#include <sstream>
#include <stdexcept>

#include "cluster.hpp"

namespace apk {

apk_cluster_gravity cluster_gravity_constants(const ClusterGravityInput &in) {
  apk_cluster_gravity c{};
  c.include_nfw = in.include_nfw_g ? 1 : 0;
  c.which_bcg = in.which_bcg_g;
  c.include_smbh = in.include_smbh_g ? 1 : 0;
  const double G = in.gravitational_constant;
  const double rho_crit = 3 * in.hubble_parameter * in.hubble_parameter / (8 * M_PI * G);
  const double c_nfw = in.c_nfw, m_nfw_200 = in.m_nfw_200;
  // calc_R_nfw_s
  const double rho_nfw_0 = 200 / 3. * rho_crit * std::pow(c_nfw, 3.) / (std::log(1 + c_nfw) - c_nfw / (1 + c_nfw));
  c.r_nfw_s = std::pow(m_nfw_200 / (4 * M_PI * rho_nfw_0 * (std::log(1 + c_nfw) - c_nfw / (1 + c_nfw))), 1. / 3.);
  // calc_g_const_nfw
  c.g_const_nfw = G * m_nfw_200 / (std::log(1 + c_nfw) - c_nfw / (1 + c_nfw));
  c.r_bcg_s = in.r_bcg_s;
  // calc_g_const_bcg
  c.g_const_bcg = (in.which_bcg_g == APK_BCG_HERNQUIST) ? G * in.m_bcg_s / (in.r_bcg_s * in.r_bcg_s) : 0.0;
  c.g_const_smbh = G * in.m_smbh;  // calc_g_const_smbh
  c.smoothing_r = in.g_smoothing_radius;
  return c;
}

double cluster_g_from_r(const apk_cluster_gravity &c, double r_in) {
  const double r = std::max(r_in, c.smoothing_r);
  const double r2 = r * r;
  double g_r = 0;
  if (c.include_nfw) g_r += c.g_const_nfw * (std::log(1 + r / c.r_nfw_s) - r / (r + c.r_nfw_s)) / r2;
  if (c.which_bcg == APK_BCG_HERNQUIST) g_r += c.g_const_bcg / ((1 + r / c.r_bcg_s) * (1 + r / c.r_bcg_s));
  if (c.include_smbh) g_r += c.g_const_smbh / r2;
  return g_r;
}

double HeSphere::K_from_r(double r) const { return k_0 + k_100 * std::pow(r / r_k, alpha_k); }
double HeSphere::P_from_rho_K(double rho, double k) const {
  return k * std::pow(rho / mh, 5. / 3.) / (mu * std::pow(mu_e, 2. / 3.));
}
double HeSphere::rho_from_P_K(double p, double k) const { return std::pow(mu * p / k, 3. / 5.) * mh * std::pow(mu_e, 2. / 5); }
double HeSphere::n_from_rho(double rho) const { return rho / (mu * mh); }
double HeSphere::ne_from_rho(double rho) const { return mu / mu_e * n_from_rho(rho); }
double HeSphere::T_from_rho_P(double rho, double p) const { return p / (n_from_rho(rho) * k_boltzmann); }
double HeSphere::dP_dr(double r, double p) const {
  const double g = cluster_g_from_r(gravity, r);
  const double k = K_from_r(r);
  const double rho = rho_from_P_K(p, k);
  return -rho * g;
}
double HeSphere::step_rk4(double t0, double t1, double y0) const {
  const double h = t1 - t0;
  const double k1 = dP_dr(t0, y0);
  const double k2 = dP_dr(t0 + h / 2., y0 + h / 2. * k1);
  const double k3 = dP_dr(t0 + h / 2., y0 + h / 2. * k2);
  const double k4 = dP_dr(t0 + h, y0 + h * k3);
  return y0 + h / 6. * (k1 + 2 * k2 + 2 * k3 + k4);
}

namespace {
constexpr double kRTol = 1e-15;
}

double HeProfile::P_from_r(double rr) const {
  // the indices in r bounding rr
  const double f = std::floor((n_r - 1) / (r_end - r_start) * (rr - r_start));
  // (outside the array the reference reads past it before it aborts; here the abort comes first)
  if (!(f >= 0.0 && f <= (double)(n_r - 2)))
    throw std::runtime_error("PRhoProfile::P_from_r R(i_r) to R_(i_r+1) does not contain r");
  const int i_r = static_cast<int>(f);
  if (rr < r[i_r] - kRTol || rr > r[i_r + 1] + kRTol)
    throw std::runtime_error("PRhoProfile::P_from_r R(i_r) to R_(i_r+1) does not contain r");
  // linear interpolation of the pressure
  return (p[i_r] * (r[i_r + 1] - rr) + p[i_r + 1] * (rr - r[i_r])) / (r[i_r + 1] - r[i_r]);
}

double HeProfile::rho_from_r(double rr) const {
  const double p_r = P_from_r(rr);
  const double k_r = sphere.K_from_r(rr);
  return sphere.rho_from_P_K(p_r, k_r);
}

void HeProfile::columns(double *out) const {
  const size_t n = (size_t)n_r;
  for (size_t i = 0; i < n; ++i) {
    const double ri = r[i], pi = p[i];
    const double k = sphere.K_from_r(ri);
    const double rho = sphere.rho_from_P_K(pi, k);
    out[0 * n + i] = ri;
    out[1 * n + i] = pi;
    out[2 * n + i] = k;
    out[3 * n + i] = rho;
    out[4 * n + i] = sphere.n_from_rho(rho);
    out[5 * n + i] = sphere.ne_from_rho(rho);
    out[6 * n + i] = sphere.T_from_rho_P(rho, pi);
    out[7 * n + i] = cluster_g_from_r(sphere.gravity, ri);
    out[8 * n + i] = sphere.dP_dr(ri, pi);
  }
}

HeProfile he_generate_profile(const HeSphere &sphere, double r_start, double r_end, unsigned int n_r) {
  if (n_r < 2 || n_r > (1u << 28)) throw std::runtime_error("HydrostaticEquilibriumSphere::generate_P_rho_profile: n_r must be at least 2");
  HeProfile prof;
  prof.sphere = sphere;
  prof.n_r = (int)n_r;
  prof.r.resize(n_r);
  prof.p.resize(n_r);
  std::vector<double> &r = prof.r, &p = prof.p;
  const double dr = (r_end - r_start) / (n_r - 1.0);
  for (int i = 0; i < (int)n_r; i++) r[i] = r_start + i * dr;  // a linear r

  const double r_fix = sphere.r_fix;
  const double k_fix = sphere.K_from_r(r_fix);
  const double p_fix = sphere.P_from_rho_K(sphere.rho_fix, k_fix);

  // the index in r right before r_fix
  const double f_fix = std::floor((n_r - 1) / (r_end - r_start) * (r_fix - r_start));
  const bool inside = f_fix >= 0.0 && f_fix <= (double)(n_r - 2);
  const int i_fix = inside ? static_cast<int>(f_fix) : 0;
  if (!inside || r_fix < r[i_fix] - kRTol || r_fix > r[i_fix + 1] + kRTol) {
    std::stringstream msg;
    msg.precision(17);
    msg << "### FATAL ERROR in function [HydrostaticEquilibriumSphere::generate_P_rho_profile]" << std::endl
        << "r(i_fix) to r_(i_fix+1) does not contain r_fix_" << std::endl;
    if (inside) msg << "r(i_fix) r_fix_ r(i_fix+1):" << r[i_fix] << " " << r_fix << " " << r[i_fix + 1] << std::endl;
    else msg << "r_start r_fix_ r_end:" << r_start << " " << r_fix << " " << r_end << std::endl;
    throw std::runtime_error(msg.str());
  }

  // integrate P inward from r_fix ...
  double r_i = r_fix, p_i = p_fix;
  for (int i = i_fix + 1; i > 0; i--) {
    p[i - 1] = sphere.step_rk4(r_i, r[i - 1], p_i);
    r_i = r[i - 1];
    p_i = p[i - 1];
  }
  // ... and outward
  r_i = r_fix;
  p_i = p_fix;
  for (int i = i_fix; i < (int)n_r - 1; i++) {
    p[i + 1] = sphere.step_rk4(r_i, r[i + 1], p_i);
    r_i = r[i + 1];
    p_i = p[i + 1];
  }
  prof.r_start = r[0];
  prof.r_end = r[n_r - 1];
  return prof;
}

HeProfile he_generate_block_profile(const HeSphere &sphere, const double *x1, int n1, const double *x2, int n2,
                                    const double *x3, int n3, const double dx[3]) {
  // 1 / r_sampling of the resolution or of r_k, whichever is smaller
  const double r_sampling = sphere.r_sampling;
  const double dr = std::min(std::min(dx[0], std::min(dx[1], dx[2])) / r_sampling, sphere.r_k / r_sampling);
  // the block's range of radii, r_fix included
  double r_start = sphere.r_fix, r_end = sphere.r_fix;
  for (int k = 0; k < n3; k++)
    for (int j = 0; j < n2; j++)
      for (int i = 0; i < n1; i++) {
        const double r = std::sqrt(x1[i] * x1[i] + x2[j] * x2[j] + x3[k] * x3[k]);
        r_start = std::min(r, r_start);
        r_end = std::max(r, r_end);
      }
  // some room at both ends
  r_start = std::max(0.0, r_start - r_sampling * dr);
  r_end += r_sampling * dr;
  const double cells = std::ceil((r_end - r_start) / dr);
  if (!(cells >= 2.0 && cells <= (double)(1u << 28)))
    throw std::runtime_error("HydrostaticEquilibriumSphere::generate_P_rho_profile: the block's radial mesh needs between 2 and "
                             "2^28 points (problem/cluster/hydrostatic_equilibrium/r_sampling, r_fix)");
  const auto n_r = static_cast<unsigned int>(cells);
  r_end = r_start + dr * (n_r - 1);  // make r_end consistent
  return he_generate_profile(sphere, r_start, r_end, n_r);
}

}  // namespace apk
