// sources_check.cpp -- stand-alone host program for the cluster problem's SNIa feedback, stellar feedback and clips
// (csrc/host/cluster_sources_model.cpp): the options as parsed with their defaults, the exclusion radius' fallback, eceil and
// rho_const_bcg, every refusal with its key and wording, and the split sources' active list of a direction against a
// brute-force search on even, odd and one-cell rows.  No GPU, no Python; meant to be compiled with sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/cluster/sources_check.cpp \
//       athenapk_amd/csrc/host/cluster_sources_model.cpp athenapk_amd/csrc/host/feedback_model.cpp -o /tmp/sources_check && /tmp/sources_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../athenapk_amd/csrc/host/cluster_sources.hpp"

using namespace apk;

namespace {
const double kInf = std::numeric_limits<double>::infinity();

// inputs/cluster_sources.in in its code units (1 Mpc, 1e14 Msun, 1 Gyr), He_mass_fraction = 0.25, gamma = 5 / 3
ClusterSourcesInput deck_input() {
  const double L = 3.0856775809623245e+24, M = 1.98841586e+47, T = 3.15576e+16;
  const double E = M * L * L / (T * T);
  ClusterSourcesInput in;
  in.power_per_bcg_mass = 0.0015780504379367209, in.mass_rate_per_bcg_mass = 0.00315576;
  in.stellar_radius = 0.03, in.exclusion_radius = 0.01, in.efficiency = 5e-9;
  in.number_density_threshold = 1.4928506511614273e+75, in.temperature_threshold = 1e4;
  in.clip_r = 0.04, in.dfloor = 1e4, in.vceil = 0.0005, in.vAceil = kInf, in.Tceil = 5000;
  in.which_bcg_g = APK_BCG_HERNQUIST, in.m_bcg_s = 7.5e-4, in.r_bcg_s = 0.004;
  in.has_composition = true, in.gamma = 1.6666666666666667;
  in.mu = 1 / (0.25 * 3. / 4. + (1 - 0.25) * 2), in.mh = 1.007947 * 1.660538921e-24 / M;
  in.mbar_over_kb = in.mu * in.mh / (1.3806488e-16 / E);
  in.speed_of_light = 2.99792458e10 / (L / T);
  return in;
}

ClusterSourcesInput no_sources() {
  ClusterSourcesInput in = deck_input();
  in.power_per_bcg_mass = in.mass_rate_per_bcg_mass = 0.0, in.snia_disabled = true;
  in.stellar_radius = in.exclusion_radius = in.efficiency = in.number_density_threshold = in.temperature_threshold = 0.0;
  in.clip_r = in.dfloor = -1.0, in.vceil = in.vAceil = in.Tceil = kInf;
  return in;
}

int refused(const char *what, const ClusterSourcesInput &in, const std::string &key, const std::string &wording) {
  try {
    (void)cluster_source_options(in);
  } catch (const std::runtime_error &e) {
    const std::string msg = e.what();
    if (msg.find(key) != std::string::npos && msg.find(wording) != std::string::npos) return 1;
    std::printf("%s: wrong message: %s\n", what, e.what());
    return 0;
  }
  std::printf("%s: nothing raised\n", what);
  return 0;
}

// the active list's range against a search over every cell
int check_range(int n, int first, double xmin, double dx, double radius) {
  std::vector<double> x((size_t)n);
  for (int i = 0; i < n; ++i) x[(size_t)i] = xmin + (i + 0.5) * dx;
  int lo = -7, hi = -7;
  split_index_range(x.data(), n, first, radius, &lo, &hi);
  int in_lo = n, in_hi = -1;
  for (int i = 0; i < n; ++i)
    if (std::fabs(x[(size_t)i]) < radius) in_lo = std::min(in_lo, i), in_hi = std::max(in_hi, i);
  if (in_hi < 0) {
    if (hi > lo) std::printf("range: n %d radius %g: [%d, %d) for no cell\n", n, radius, lo, hi);
    return hi <= lo;
  }
  const int ok = lo >= first && hi <= first + n && lo <= first + in_lo && hi >= first + in_hi + 1 && first + in_lo - lo <= 1 &&
                 hi - (first + in_hi + 1) <= 1;
  if (!ok) std::printf("range: n %d first %d radius %g: [%d, %d) for cells %d .. %d\n", n, first, radius, lo, hi, in_lo, in_hi);
  return ok;
}
}  // namespace

int main() {
  int ok = 1;
  // the deck
  const ClusterSourcesInput deck = deck_input();
  const apk_cluster_source_options o = cluster_source_options(deck);
  std::printf("active: snia %d stellar %d clips %d; rho_const_bcg %.17g mbar %.17g mass_to_energy %.17g eceil %.17g\n", o.snia_active,
              o.stellar_active, o.clips_active, o.rho_const_bcg, o.mbar, o.mass_to_energy, o.eceil);
  ok &= o.snia_active == 1 && o.stellar_active == 1 && o.clips_active == 1;
  ok &= o.rho_const_bcg == 7.5e-4 * 0.004 / (2 * M_PI) && rho_const_bcg(APK_BCG_NONE, 7.5e-4, 0.004) == 0.0;
  ok &= o.eceil == 5000 / deck.mbar_over_kb / (deck.gamma - 1.0) && o.mbar == deck.mu * deck.mh;
  ok &= o.mass_to_energy == 5e-9 * (deck.speed_of_light * deck.speed_of_light) && o.exclusion_radius == 0.01;
  // defaults: nothing active, no ceiling
  const apk_cluster_source_options none = cluster_source_options(no_sources());
  ok &= none.snia_active == 0 && none.stellar_active == 0 && none.clips_active == 0 && none.eceil == kInf && none.clip_r == -1.0;
  // the exclusion radius' fallback
  ClusterSourcesInput in = deck;
  in.exclusion_radius = 0.0, in.accretion_radius = 0.015;
  ok &= cluster_source_options(in).exclusion_radius == 0.015;
  in.accretion_radius = 0.0;
  ok &= refused("stellar without an exclusion radius", in, "problem/cluster/stellar_feedback", "Enabling stellar feedback requires setting all parameters.");
  // the clips need no units without a temperature ceiling
  in = deck;
  in.has_composition = false, in.stellar_radius = in.exclusion_radius = in.efficiency = in.number_density_threshold = in.temperature_threshold = 0.0;
  ok &= refused("Tceil without units", in, "problem/cluster/clips/Tceil", "Temperature ceiling requires units and gas composition");
  in.Tceil = kInf;
  ok &= cluster_source_options(in).clips_active == 1 && cluster_source_options(in).eceil == kInf;

  // refusals
  in = deck, in.power_per_bcg_mass = in.mass_rate_per_bcg_mass = 0.0;
  ok &= refused("snia without rates", in, "problem/cluster/snia_feedback/disabled", "no-op");
  in = deck, in.which_bcg_g = APK_BCG_NONE;
  ok &= refused("snia without a BCG", in, "problem/cluster/snia_feedback/disabled", "BCG must be defined for SNIA Feedback to be enabled");
  in = deck, in.rkl2 = true;
  ok &= refused("snia with rkl2", in, "problem/cluster/snia_feedback/disabled", "rkl2");
  in = deck, in.snia_disabled = true, in.rkl2 = true;
  ok &= refused("stellar with rkl2", in, "problem/cluster/stellar_feedback", "rkl2");
  in = deck, in.efficiency = 0.0;
  ok &= refused("stellar partly set", in, "problem/cluster/stellar_feedback", "Enabling stellar feedback requires setting all parameters.");
  in = deck, in.has_composition = false;
  ok &= refused("stellar without units", in, "problem/cluster/stellar_feedback", "units");
  in = deck, in.dfloor = -1.0, in.vceil = in.Tceil = kInf;
  ok &= refused("clip_r without a limit", in, "problem/cluster/clips/clip_r", "no limit");
  const struct {
    const char *key;
    double ClusterSourcesInput::*member;
    double value;
  } limits[] = {{"dfloor", &ClusterSourcesInput::dfloor, 1.0}, {"vceil", &ClusterSourcesInput::vceil, 1.0},
                {"vAceil", &ClusterSourcesInput::vAceil, 1.0}, {"Tceil", &ClusterSourcesInput::Tceil, 1e7}};
  for (const auto &l : limits) {
    in = no_sources(), in.mhd = true;
    in.*(l.member) = l.value;
    ok &= refused(l.key, in, std::string("problem/cluster/clips/") + l.key, "clip_r <= 0");
  }
  in = deck, in.vAceil = 3.0;
  ok &= refused("vAceil without MHD", in, "problem/cluster/clips/vAceil", "glmmhd");
  in.mhd = true;
  ok &= cluster_source_options(in).vAceil == 3.0;
  in = deck, in.snia_disabled = true, in.rkl2 = true;
  in.stellar_radius = in.exclusion_radius = in.efficiency = in.number_density_threshold = in.temperature_threshold = 0.0;
  ok &= refused("clips with rkl2", in, "problem/cluster/clips/clip_r", "rkl2");

  // the active list of a direction: blocks left of, across and right of the origin, odd and one-cell rows, radii from
  // less than half a cell to more than the block
  for (int n : {1, 3, 8, 33})
    for (int first : {0, 2, 4})
      for (double xmin : {-1.0, -0.4375, -0.26, 0.0, 0.31})
        for (double radius : {0.01, 0.0624, 0.125, 0.25, 0.3, 5.0}) ok &= check_range(n, first, xmin, 0.125, radius);
  std::printf(ok ? "sources_check ok\n" : "sources_check FAILED\n");
  return ok ? 0 : 1;
}
