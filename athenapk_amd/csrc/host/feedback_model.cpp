// feedback_model.cpp -- the host-side model of the cluster problem's fixed-power AGN feedback (host/feedback.hpp): the
// jet frame, AGNFeedback's derived jet numbers with its five consistency requirements, the per-stage numbers, the
// magnetic tower's power scaling and its initial field; AGN triggering's accretion rate, time-step rule and the index
// range of its active list.  Plain C++, no driver, no GPU: tools/cluster/feedback_check.cpp
// links it alone.  std::pow and M_PI stand where the reference has them; squares of positions are products
// (feedback_math.hpp).
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../feedback_math.hpp"
#include "feedback.hpp"

namespace apk {

namespace {
double sqr(double x) { return x * x; }
}  // namespace

apk_jet_coords jet_coords_at(double jet_theta, double jet_phi_dot, double jet_phi0, double time) {
  const double phi = jet_phi0 + time * jet_phi_dot;
  return apk_jet_coords{std::cos(jet_theta), std::sin(jet_theta), std::cos(phi), std::sin(phi)};
}

double AgnFeedbackModel::power() const { return in.fixed_power + accretion_rate * in.efficiency * std::pow(in.speed_of_light, 2); }
double AgnFeedbackModel::mass_rate() const {
  return accretion_rate * (1 - in.efficiency) + in.fixed_power / (in.efficiency * std::pow(in.speed_of_light, 2));
}

// AGNFeedback::AGNFeedback (agn_feedback.cpp:34-160)
AgnFeedbackModel agn_feedback_model(const AgnFeedbackInput &in) {
  AgnFeedbackModel m;
  m.in = in;
  m.thermal_fraction = in.thermal_fraction, m.kinetic_fraction = in.kinetic_fraction, m.magnetic_fraction = in.magnetic_fraction;
  const double total_frac = m.thermal_fraction + m.kinetic_fraction + m.magnetic_fraction;
  if (total_frac > 0) {
    m.thermal_fraction = m.thermal_fraction / total_frac;
    m.kinetic_fraction = m.kinetic_fraction / total_frac;
    m.magnetic_fraction = m.magnetic_fraction / total_frac;
  }
  if (!(m.thermal_fraction >= 0 && m.kinetic_fraction >= 0 && m.magnetic_fraction >= 0))
    throw std::runtime_error("AGN feedback energy fractions must be non-negative.");
  if (in.enable_magnetic_tower_mass_injection) {
    m.thermal_mass_fraction = m.thermal_fraction;
    m.kinetic_mass_fraction = m.kinetic_fraction;
    m.magnetic_mass_fraction = m.magnetic_fraction;
  } else {
    const double total_mass_frac = m.thermal_fraction + m.kinetic_fraction;
    m.thermal_mass_fraction = m.thermal_fraction / total_mass_frac;
    m.kinetic_mass_fraction = m.kinetic_fraction / total_mass_frac;
    m.magnetic_mass_fraction = 0.0;
  }

  // v_jet = sqrt(2 (eps c^2 - (1 - eps) e_jet)): either of velocity and temperature, both or neither
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double c = in.speed_of_light, eff = in.efficiency;
  double v = in.has_velocity ? in.kinetic_jet_velocity : nan;
  double T = in.has_temperature ? in.kinetic_jet_temperature : nan;
  double e = in.has_temperature ? T / in.mbar_gm1_over_kb : nan;
  if (std::isnan(v) && std::isnan(T)) {  // neither: a jet at 0 K
    v = c * std::sqrt(2 * (eff));
    T = 0;
    e = 0;
    m.assumed_cold_jet = true;
  } else if (std::isnan(v)) {
    v = std::sqrt(2 * (eff * sqr(c) - (1.0 - eff) * e));
  } else if (std::isnan(T)) {
    e = (eff * sqr(c) - 0.5 * sqr(v)) / (1 - eff);
    T = in.mbar_gm1_over_kb * e;
  }
  if (!(std::fabs(v - std::sqrt(2 * (eff * sqr(c) - (1 - eff) * e))) < 10 * std::numeric_limits<double>::epsilon()))
    throw std::runtime_error("Specified kinetic jet velocity and temperature are incompatible with mass to energy conversion "
                             "efficiency. Either the specified velocity, temperature, or efficiency are incompatible");
  if (!(v <= c * std::sqrt(2 * eff))) throw std::runtime_error("Kinetic jet velocity implies negative temperature of the jet");
  if (!(e <= sqr(c) * eff / (1 - eff))) throw std::runtime_error("Kinetic jet temperature implies negative kinetic energy of the jet");
  if (!(v >= 0)) throw std::runtime_error("Kinetic jet velocity must be non-negative");
  if (!(T >= 0)) throw std::runtime_error("Kinetic jet temperature must be non-negative");
  m.kinetic_jet_velocity = v, m.kinetic_jet_temperature = T, m.kinetic_jet_e = e;
  m.eceil = in.Tceil / in.mbar_gm1_over_kb;
  return m;
}

// agn_feedback.cpp:263-303
apk_agn_feedback_cfg agn_feedback_stage_numbers(const AgnFeedbackModel &m, double beta_dt) {
  const AgnFeedbackInput &in = m.in;
  const double power = m.power(), mass_rate = m.mass_rate();
  apk_agn_feedback_cfg c{};
  const double thermal_scaling_factor = 1 / (4. / 3. * M_PI * std::pow(in.thermal_radius, 3));
  c.thermal_feedback = m.thermal_fraction * power * thermal_scaling_factor * beta_dt;
  c.thermal_density = m.thermal_mass_fraction * mass_rate * thermal_scaling_factor * beta_dt;
  c.thermal_radius = in.thermal_radius;
  const double kinetic_scaling_factor = 1 / (2 * in.kinetic_jet_thickness * M_PI * std::pow(in.kinetic_jet_radius, 2));
  c.jet_density = m.kinetic_mass_fraction * mass_rate * kinetic_scaling_factor * beta_dt;
  c.jet_momentum = c.jet_density * m.kinetic_jet_velocity;
  c.jet_feedback = m.kinetic_fraction * power * kinetic_scaling_factor * beta_dt;
  c.kinetic_jet_radius = in.kinetic_jet_radius, c.kinetic_jet_thickness = in.kinetic_jet_thickness;
  c.kinetic_jet_offset = in.kinetic_jet_offset;
  c.vceil = in.vceil, c.eceil = m.eceil;
  return c;
}

double tower_field_to_add(double linear_contrib, double quadratic_contrib, double beta_dt, double power) {
  if (linear_contrib == 0 && quadratic_contrib == 0)
    throw std::runtime_error("MagneticTowerModel::PowerSrcTerm mt_linear_contrib and mt_quadratic_contrib are both zero. "
                             "(Has MagneticTowerReducePowerContribs been called?)");
  const double disc = linear_contrib * linear_contrib + 4 * quadratic_contrib * beta_dt * power;
  if (disc < 0 || quadratic_contrib == 0)
    throw std::runtime_error("MagneticTowerModel::PowerSrcTerm No field rate is viable linear_contrib: " +
                             std::to_string(linear_contrib) + " quadratic_contrib: " + std::to_string(quadratic_contrib));
  return (-linear_contrib + std::sqrt(disc)) / (2 * quadratic_contrib);
}

double tower_density_to_add(double mass_to_add, double l_mass_scale) {
  if (!(mass_to_add == 0.0 || l_mass_scale > 0.0))
    throw std::runtime_error("Trying to inject mass with the tower model but 0 mass lengthscale. Either disable tower mass "
                             "injection or set positive lengthscale.");
  return mass_to_add > 0.0 ? mass_to_add / (std::pow(l_mass_scale, 3) * std::pow(M_PI, 3. / 2.)) : 0.0;
}

void tower_check_combination(const apk_magnetic_tower_cfg &t) {
  if (t.potential == APK_TOWER_DONUT) {
    if (!(t.donut_offset >= 0.0 && t.donut_thickness > 0.0))
      throw std::runtime_error("Incompatible combination of donut_offset and donut_thickness for magnetic donut feedback.");
    if (!(t.li_alpha == 0.0)) throw std::runtime_error("Please disable (set to zero) tower li_alpha for the donut model");
  } else if (t.potential == APK_TOWER_LI) {
    if (!(t.donut_offset <= 0.0 && t.donut_thickness <= 0.0))
      throw std::runtime_error("Please disable (set to zero) tower offset and thickness for the Li tower model");
  }
}

void tower_check_scales(const apk_magnetic_tower_cfg &t) {
  if (!(t.l_scale > 0)) throw std::runtime_error("Magnetic Tower Length scale must be strictly postitive");
  if (!(t.l_mass_scale >= 0)) throw std::runtime_error("Magnetic Tower Mass Length scale must be zero (disabled) or postitive");
}

void tower_initial_field_block(const apk_magnetic_tower_cfg &t, const apk_jet_coords &jc, double field, const double *x1, int n1,
                               const double *x2, int n2, const double *x3, int n3, const double dx[3], double *b) {
  tower_check_scales(t);
  if (t.potential != APK_TOWER_LI && t.potential != APK_TOWER_DONUT) throw std::runtime_error("Unknown magnetic tower potential.");
  const size_t m1 = (size_t)n1 + 2, m2 = (size_t)n2 + 2, m3 = (size_t)n3 + 2, na = m1 * m2 * m3;
  std::vector<double> A(3 * na, 0.0);
  auto a = [&](int n, int k, int j, int i) -> double & { return A[n * na + ((size_t)k * m2 + j) * m1 + i]; };
  for (int k = 0; k < (int)m3; ++k)
    for (int j = 0; j < (int)m2; ++j)
      for (int i = 0; i < (int)m1; ++i) {
        double a_x, a_y, a_z;
        tower_potential(t, jc, field, x1[i], x2[j], x3[k], a_x, a_y, a_z);
        a(0, k, j, i) += a_x;
        a(1, k, j, i) += a_y;
        a(2, k, j, i) += a_z;
      }
  const size_t nb = (size_t)n1 * n2 * n3;
  for (int k = 1; k <= n3; ++k)
    for (int j = 1; j <= n2; ++j)
      for (int i = 1; i <= n1; ++i) {
        const size_t q = ((size_t)(k - 1) * n2 + (j - 1)) * n1 + (i - 1);
        b[0 * nb + q] = (a(2, k, j + 1, i) - a(2, k, j - 1, i)) / dx[1] / 2.0 - (a(1, k + 1, j, i) - a(1, k - 1, j, i)) / dx[2] / 2.0;
        b[1 * nb + q] = (a(0, k + 1, j, i) - a(0, k - 1, j, i)) / dx[2] / 2.0 - (a(2, k, j, i + 1) - a(2, k, j, i - 1)) / dx[0] / 2.0;
        b[2 * nb + q] = (a(1, k, j, i + 1) - a(1, k, j, i - 1)) / dx[0] / 2.0 - (a(0, k, j + 1, i) - a(0, k, j - 1, i)) / dx[1] / 2.0;
      }
}

int parse_agn_triggering_mode(const std::string &mode_str) {
  if (mode_str == "COLD_GAS") return APK_TRIG_COLD_GAS;
  if (mode_str == "BOOSTED_BONDI") return APK_TRIG_BOOSTED_BONDI;
  if (mode_str == "BOOTH_SCHAYE") return APK_TRIG_BOOTH_SCHAYE;
  if (mode_str == "NONE") return APK_TRIG_NONE;
  throw std::runtime_error("### FATAL ERROR in function [ParseAGNTriggeringMode]\nUnrecognized AGNTriggeringMode: \"" + mode_str + "\"");
}

// agn_triggering.cpp:319-365
double AgnTriggeringModel::accretion_rate(const Reduced &q) const {
  switch (mode) {
  case APK_TRIG_COLD_GAS:
    return q.cold_mass / cold_t_acc;
  case APK_TRIG_BOOSTED_BONDI:
  case APK_TRIG_BOOTH_SCHAYE: {
    const double mean_mass_weighted_density = q.mass_weighted_density / q.total_mass;
    const double mean_mass_weighted_velocity = q.mass_weighted_velocity / q.total_mass;
    const double mean_mass_weighted_cs = q.mass_weighted_cs / q.total_mass;
    double alpha = 0;
    if (mode == APK_TRIG_BOOSTED_BONDI) {
      alpha = bondi_alpha;
    } else {
      const double mean_mass_weighted_n = mean_mass_weighted_density / mean_molecular_mass;
      alpha = (mean_mass_weighted_n <= bondi_n0) ? 1 : std::pow(mean_mass_weighted_n / bondi_n0, bondi_beta);
    }
    return alpha * 2 * M_PI * std::pow(gravitational_constant, 2) * std::pow(bondi_M_smbh, 2) * mean_mass_weighted_density /
           (std::pow(std::pow(mean_mass_weighted_velocity, 2) + std::pow(mean_mass_weighted_cs, 2), 3. / 2.));
  }
  default:
    return 0;
  }
}

// agn_triggering.cpp:556-584
double AgnTriggeringModel::estimate_timestep(const Reduced &q) const {
  switch (mode) {
  case APK_TRIG_COLD_GAS:
    return accretion_cfl * cold_t_acc;
  case APK_TRIG_BOOSTED_BONDI:
  case APK_TRIG_BOOTH_SCHAYE: {
    // (before the first reduction: the reference ignores the constraint during the first time step)
    if (q.total_mass == 0) return std::numeric_limits<double>::max();
    const double mdot = accretion_rate(q);
    return accretion_cfl * q.total_mass / mdot;
  }
  default:
    return std::numeric_limits<double>::max();
  }
}

void triggering_index_range(const double *x, int n_ext, double radius, int *lo, int *hi) {
  int first = n_ext, last = -1;
  for (int i = 0; i < n_ext; ++i)
    if (std::fabs(x[i]) < radius) {
      if (first == n_ext) first = i;
      last = i;
    }
  if (last < 0) {
    *lo = *hi = 0;
    return;
  }
  *lo = first - 1 < 0 ? 0 : first - 1;
  *hi = last + 2 > n_ext ? n_ext : last + 2;
}

}  // namespace apk
