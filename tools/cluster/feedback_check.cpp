// feedback_check.cpp -- stand-alone host program for the cluster problem's AGN feedback model
// (csrc/host/feedback_model.cpp): the derived jet numbers in the four ways of giving velocity and temperature, the per-stage
// numbers, the power scaling with its two failures, the requirement messages, and one 8^3 block's initial tower field for
// both potentials with its discrete divergence; AGN triggering's accretion rate in its three modes, its time-step rule, power
// and mass rate with accretion, and the active list's index range.  No GPU, no Python; meant to be compiled with sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/cluster/feedback_check.cpp athenapk_amd/csrc/host/feedback_model.cpp -o /tmp/feedback_check && /tmp/feedback_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../athenapk_amd/csrc/host/feedback.hpp"

using namespace apk;

namespace {
int raised(const char *what, const std::string &want, void (*f)()) {
  try {
    f();
  } catch (const std::runtime_error &e) {
    if (std::string(e.what()).find(want) != std::string::npos) return 1;
    std::printf("%s: wrong message: %s\n", what, e.what());
    return 0;
  }
  std::printf("%s: nothing raised\n", what);
  return 0;
}

AgnFeedbackInput deck_input() {
  // src/units.hpp in the decks' code units (1 Mpc, 1e14 Msun, 1 Gyr), He_mass_fraction = 0.25, gamma = 5 / 3
  const double L = 3.0856775809623245e+24, M = 1.98841586e+47, T = 3.15576e+16;
  const double E = M * L * L / (T * T);
  const double mu = 1 / (0.25 * 3. / 4. + (1 - 0.25) * 2), mh = 1.007947 * 1.660538921e-24 / M, kb = 1.3806488e-16 / E;
  AgnFeedbackInput in;
  in.fixed_power = 0.3319965633348794, in.efficiency = 1e-3, in.thermal_fraction = 0.5, in.kinetic_fraction = 0.5;
  in.thermal_radius = 0.1, in.kinetic_jet_radius = 0.05, in.kinetic_jet_thickness = 0.05, in.kinetic_jet_offset = 0.01;
  in.vceil = in.Tceil = std::numeric_limits<double>::infinity();
  in.speed_of_light = 2.99792458e10 / (L / T);
  in.mbar_gm1_over_kb = mu * mh / kb * (1.6666666666666667 - 1.0);
  return in;
}
}  // namespace

int main() {
  int ok = 1;
  // the four ways
  AgnFeedbackInput in = deck_input();
  const AgnFeedbackModel cold = agn_feedback_model(in);
  in.has_temperature = true, in.kinetic_jet_temperature = 1e7;
  const AgnFeedbackModel hot = agn_feedback_model(in);
  AgnFeedbackInput both = in;
  both.has_velocity = true, both.kinetic_jet_velocity = hot.kinetic_jet_velocity;
  const AgnFeedbackModel given = agn_feedback_model(both);
  AgnFeedbackInput vel = deck_input();
  vel.has_velocity = true, vel.kinetic_jet_velocity = 8.0;
  const AgnFeedbackModel from_v = agn_feedback_model(vel);
  std::printf("v_jet: cold %.17g, T = 1e7 K %.17g (e_jet %.17g), both %.17g, v = 8: T %.17g\n", cold.kinetic_jet_velocity,
              hot.kinetic_jet_velocity, hot.kinetic_jet_e, given.kinetic_jet_velocity, from_v.kinetic_jet_temperature);
  ok &= cold.assumed_cold_jet && cold.kinetic_jet_e == 0.0 && given.kinetic_jet_velocity == hot.kinetic_jet_velocity;
  const apk_agn_feedback_cfg c = agn_feedback_stage_numbers(hot, 1e-4);
  std::printf("stage numbers: thermal %.6e %.6e, jet %.6e %.6e %.6e\n", c.thermal_feedback, c.thermal_density, c.jet_density,
              c.jet_momentum, c.jet_feedback);
  ok &= c.jet_momentum == c.jet_density * hot.kinetic_jet_velocity && std::isinf(c.eceil);

  // requirement messages
  int caught = 0;
  caught += raised("incompatible", "are incompatible with mass to energy conversion", [] {
    AgnFeedbackInput i = deck_input();
    i.has_velocity = i.has_temperature = true, i.kinetic_jet_velocity = 5.0, i.kinetic_jet_temperature = 1e7;
    (void)agn_feedback_model(i);
  });
  caught += raised("negative temperature", "Kinetic jet velocity implies negative temperature of the jet", [] {
    AgnFeedbackInput i = deck_input();
    i.has_velocity = true, i.kinetic_jet_velocity = 1.001 * i.speed_of_light * std::sqrt(2e-3);
    (void)agn_feedback_model(i);
  });
  caught += raised("temperature sign", "Kinetic jet temperature must be non-negative", [] {
    AgnFeedbackInput i = deck_input();
    i.has_temperature = true, i.kinetic_jet_temperature = -1e-20;
    (void)agn_feedback_model(i);
  });
  caught += raised("fractions", "AGN feedback energy fractions must be non-negative.", [] {
    AgnFeedbackInput i = deck_input();
    i.thermal_fraction = -0.5;
    (void)agn_feedback_model(i);
  });

  // the power scaling and its two failures
  const double f = tower_field_to_add(-0.37, 0.0213, 1.7e-4, 1.66e-3);
  std::printf("field_to_add %.17g, residual %.3e\n", f, -0.37 * f + 0.0213 * f * f - 1.7e-4 * 1.66e-3);
  caught += raised("both zero", "mt_linear_contrib and mt_quadratic_contrib are both zero", [] { (void)tower_field_to_add(0, 0, 1, 1); });
  caught += raised("negative discriminant", "No field rate is viable", [] { (void)tower_field_to_add(1, -1, 1, 1); });
  caught += raised("quad zero", "No field rate is viable", [] { (void)tower_field_to_add(1, 0, 1, 1); });
  caught += raised("mass scale", "0 mass lengthscale", [] { (void)tower_density_to_add(1.0, 0.0); });
  ok &= tower_density_to_add(0.0, 0.0) == 0.0 && tower_density_to_add(1.0, 0.005) > 0.0;

  // one block's initial field, both potentials, tilted axis: block (1, 0, 1) of a 16^3 mesh over [-0.1, 0.1]^3 in 8^3 blocks
  const apk_jet_coords jc = jet_coords_at(0.2, 0.0, 1.0, 0.0);
  const int n = 8;
  const double dx[3] = {0.2 / 16, 0.2 / 16, 0.2 / 16};
  const int g0[3] = {8, 0, 8};
  std::vector<double> x[3];
  for (int d = 0; d < 3; ++d)
    for (int i = -1; i <= n; ++i) x[d].push_back(-0.1 + (((double)g0[d] + (double)i) + 0.5) * dx[d]);
  for (int pot : {APK_TOWER_LI, APK_TOWER_DONUT}) {
    apk_magnetic_tower_cfg t{};
    t.potential = pot, t.l_scale = 0.04, t.l_mass_scale = 0.005;
    if (pot == APK_TOWER_LI) t.li_alpha = 20;
    else t.donut_offset = 0.01, t.donut_thickness = 0.05;
    tower_check_combination(t);
    std::vector<double> b(3 * (size_t)n * n * n);
    tower_initial_field_block(t, jc, 0.1243156000020414, x[0].data(), n, x[1].data(), n, x[2].data(), n, dx, b.data());
    auto at = [&](int c, int k, int j, int i) { return b[(size_t)c * n * n * n + ((size_t)k * n + j) * n + i]; };
    double bmax = 0.0, divmax = 0.0;
    for (double v : b) bmax = std::fmax(bmax, std::fabs(v));
    for (int k = 1; k < n - 1; ++k)
      for (int j = 1; j < n - 1; ++j)
        for (int i = 1; i < n - 1; ++i) {
          const double div = (at(0, k, j, i + 1) - at(0, k, j, i - 1)) / dx[0] / 2.0 + (at(1, k, j + 1, i) - at(1, k, j - 1, i)) / dx[1] / 2.0 +
                             (at(2, k + 1, j, i) - at(2, k - 1, j, i)) / dx[2] / 2.0;
          divmax = std::fmax(divmax, std::fabs(div));
        }
    std::printf("%s: max |B| %.6e, max |div B| %.3e\n", pot == APK_TOWER_LI ? "li" : "donut", bmax, divmax);
    ok &= bmax > 0.0 && std::isfinite(bmax) && divmax < 1e-10 * bmax / dx[0];
  }
  caught += raised("length scale", "Magnetic Tower Length scale must be strictly postitive", [] {
    apk_magnetic_tower_cfg t{};
    t.potential = APK_TOWER_LI;
    const double x3[3] = {0, 1, 2}, d[3] = {1, 1, 1};
    double b[3];
    tower_initial_field_block(t, jet_coords_at(0, 0, 0, 0), 1.0, x3, 1, x3, 1, x3, 1, d, b);
  });

  // AGN triggering: the suite's uniform gas in the deck's units, a sphere of 20 kpc
  {
    const double L = 3.0856775809623245e+24, M = 1.98841586e+47, T = 3.15576e+16;
    const double mu = 1 / (0.25 * 3. / 4. + (1 - 0.25) * 2);
    AgnTriggeringModel t;
    t.accretion_radius = 0.02, t.cold_temp_thresh = 7198.523584993223, t.cold_t_acc = 0.1, t.bondi_alpha = 100, t.bondi_beta = 2;
    t.bondi_M_smbh = 1e-6, t.mean_molecular_mass = mu * (1.660538921e-24 / M);
    t.mean_molecular_mass_by_kb = t.mean_molecular_mass / (1.3806488e-16 / (M * L * L / (T * T)));
    t.gravitational_constant = 6.67408e-08 / (std::pow(L, 3) / (M * std::pow(T, 2)));
    const double rho = 14775.575892787225, vol = 4. / 3. * M_PI * std::pow(0.02, 3), v = 8.97e-4, cs = 1.32e-2;
    t.bondi_n0 = 0.05 * rho / t.mean_molecular_mass;
    AgnTriggeringModel::Reduced q;
    q.cold_mass = q.total_mass = rho * vol;
    q.mass_weighted_density = q.total_mass * rho, q.mass_weighted_velocity = q.total_mass * v, q.mass_weighted_cs = q.total_mass * cs;
    const AgnTriggeringModel::Reduced none;
    double rate[4], dt[4], dt0[4];
    for (int mode : {APK_TRIG_NONE, APK_TRIG_COLD_GAS, APK_TRIG_BOOSTED_BONDI, APK_TRIG_BOOTH_SCHAYE}) {
      t.mode = mode;
      rate[mode] = t.accretion_rate(q), dt[mode] = t.estimate_timestep(q), dt0[mode] = t.estimate_timestep(none);
      std::printf("triggering mode %d: rate %.17g, dt %.6e, dt before the first reduction %.6e\n", mode, rate[mode], dt[mode], dt0[mode]);
    }
    const double huge = std::numeric_limits<double>::max();
    ok &= rate[APK_TRIG_NONE] == 0 && dt[APK_TRIG_NONE] == huge && rate[APK_TRIG_COLD_GAS] == q.cold_mass / 0.1;
    ok &= dt[APK_TRIG_COLD_GAS] == 0.1 * 0.1 && dt0[APK_TRIG_COLD_GAS] == 0.1 * 0.1;
    ok &= dt0[APK_TRIG_BOOSTED_BONDI] == huge && dt0[APK_TRIG_BOOTH_SCHAYE] == huge;
    ok &= std::fabs(rate[APK_TRIG_BOOTH_SCHAYE] / (rate[APK_TRIG_BOOSTED_BONDI] / 100 * 400) - 1) < 1e-13;  // (n / n0)^2 = 400
    ok &= std::fabs(dt[APK_TRIG_BOOSTED_BONDI] - 0.1 * q.total_mass / rate[APK_TRIG_BOOSTED_BONDI]) <= 1e-15 * dt[APK_TRIG_BOOSTED_BONDI];
    t.mode = APK_TRIG_BOOTH_SCHAYE, t.bondi_n0 = q.mass_weighted_density / q.total_mass / t.mean_molecular_mass;  // n == n0: alpha = 1
    const double at_n0 = t.accretion_rate(q);
    t.mode = APK_TRIG_BOOSTED_BONDI, t.bondi_alpha = 1;
    ok &= at_n0 == t.accretion_rate(q);
    // power and mass rate with that accretion
    AgnFeedbackModel fb = agn_feedback_model(deck_input());
    const double p0 = fb.power(), m0 = fb.mass_rate();
    fb.accretion_rate = rate[APK_TRIG_COLD_GAS];
    const double c2 = std::pow(fb.in.speed_of_light, 2);
    std::printf("power %.17g -> %.17g, mass rate %.17g -> %.17g\n", p0, fb.power(), m0, fb.mass_rate());
    ok &= p0 == fb.in.fixed_power && fb.power() == fb.in.fixed_power + fb.accretion_rate * 1e-3 * c2;
    ok &= fb.mass_rate() == fb.accretion_rate * (1 - 1e-3) + fb.in.fixed_power / (1e-3 * c2);
    // the active list's range: 12 extended cells of a block whose interior starts at the origin, radius 2.4 cells
    double xc[12];
    for (int i = 0; i < 12; ++i) xc[i] = ((double)(i - 2) + 0.5) * 0.0125;
    int lo = -1, hi = -1;
    triggering_index_range(xc, 12, 0.03, &lo, &hi);
    ok &= lo == 0 && hi == 5;  // cells 0 .. 3 lie inside, one more on the upper side, clipped below
    triggering_index_range(xc + 6, 6, 0.03, &lo, &hi);
    ok &= lo >= hi;
    triggering_index_range(xc, 12, 0.03, &lo, &hi);
    std::printf("index range of the block at the origin: [%d, %d)\n", lo, hi);
  }
  caught += raised("triggering mode", "Unrecognized AGNTriggeringMode", [] { (void)parse_agn_triggering_mode("EDDINGTON"); });
  ok &= parse_agn_triggering_mode("BOOTH_SCHAYE") == APK_TRIG_BOOTH_SCHAYE && parse_agn_triggering_mode("NONE") == APK_TRIG_NONE;
  std::printf("failures raised: %d of 10\n", caught);
  return (ok && caught == 10) ? 0 : 1;
}
