// feedback_check.cpp -- stand-alone host program for the cluster problem's AGN feedback model
// (csrc/host/feedback_model.cpp): the derived jet numbers in the four ways of giving velocity and temperature, the per-stage
// numbers, the power scaling with its two failures, the requirement messages, and one 8^3 block's initial tower field for
// both potentials with its discrete divergence.  No GPU, no Python; meant to be compiled with sanitizers:
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
  std::printf("failures raised: %d of 9\n", caught);
  return (ok && caught == 9) ? 0 : 1;
}
