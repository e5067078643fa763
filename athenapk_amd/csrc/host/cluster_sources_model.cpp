// cluster_sources_model.cpp -- see cluster_sources.hpp
#include "cluster_sources.hpp"

#include <cmath>
#include <limits>
#include <stdexcept>

#include "feedback.hpp"

namespace apk {

namespace {
const char *kSnia = "problem/cluster/snia_feedback";
const char *kStellar = "problem/cluster/stellar_feedback";
const char *kClips = "problem/cluster/clips";

[[noreturn]] void refuse(const std::string &key, const std::string &why) {
  throw std::runtime_error("problem_id = cluster: " + key + " " + why);
}
}  // namespace

double rho_const_bcg(int which_bcg_g, double m_bcg_s, double r_bcg_s) {
  // (the evident intent: the reference never calls calc_rho_const_bcg and reads the member uninitialised,
  // cluster_gravity.hpp:46, 220)
  return which_bcg_g == APK_BCG_HERNQUIST ? m_bcg_s * r_bcg_s / (2 * M_PI) : 0.0;
}

// "refused, never ignored" extends to blocks that would be inert
apk_cluster_source_options cluster_source_options(const ClusterSourcesInput &in) {
  const double inf = std::numeric_limits<double>::infinity();
  apk_cluster_source_options o{};

  // SNIa feedback (the reference's default is ENABLED: a deck that runs without has to say so)
  o.power_per_bcg_mass = in.power_per_bcg_mass, o.mass_rate_per_bcg_mass = in.mass_rate_per_bcg_mass;
  o.rho_const_bcg = rho_const_bcg(in.which_bcg_g, in.m_bcg_s, in.r_bcg_s);
  if (!in.snia_disabled) {
    if (o.power_per_bcg_mass == 0.0 && o.mass_rate_per_bcg_mass == 0.0)
      refuse(std::string(kSnia) + "/disabled", "must be true when power_per_bcg_mass and mass_rate_per_bcg_mass are both zero: the "
             "reference enables SNIa feedback by default and runs it as a no-op");
    if (in.which_bcg_g == APK_BCG_NONE)
      refuse(std::string(kSnia) + "/disabled", "= false with problem/cluster/gravity/which_bcg_g = NONE: BCG must be defined for SNIA "
             "Feedback to be enabled");
    if (!(in.r_bcg_s > 0.0)) refuse("problem/cluster/gravity/r_bcg_s", "must be positive");
    if (in.rkl2) refuse(std::string(kSnia) + "/disabled", "= false is not supported with diffusion/integrator = rkl2");
    o.snia_active = 1;
  }

  // stellar feedback
  o.stellar_radius = in.stellar_radius, o.exclusion_radius = in.exclusion_radius, o.efficiency = in.efficiency;
  o.number_density_threshold = in.number_density_threshold, o.temperature_threshold = in.temperature_threshold;
  const bool stellar_disabled = o.stellar_radius == 0.0 && o.exclusion_radius == 0.0 && o.efficiency == 0.0 &&
                                o.number_density_threshold == 0.0 && o.temperature_threshold == 0.0;
  // (if exclusion_radius is not specified, the AGN triggering accretion radius)
  if (!stellar_disabled && o.exclusion_radius == 0.0) o.exclusion_radius = in.accretion_radius;
  if (in.has_composition) {
    o.mbar = in.mu * in.mh;
    o.mbar_over_kb = in.mbar_over_kb;
    o.mass_to_energy = o.efficiency * (in.speed_of_light * in.speed_of_light);
  }
  if (!stellar_disabled) {
    if (!(o.stellar_radius != 0.0 && o.exclusion_radius != 0.0 && o.efficiency != 0.0 && o.number_density_threshold != 0.0 &&
          o.temperature_threshold != 0.0))
      refuse(kStellar, "is partly set: Enabling stellar feedback requires setting all parameters.");
    if (!in.has_composition)
      refuse(kStellar, "requires units and gas composition. Set a 'units' block and 'hydro/He_mass_fraction' in the input file.");
    if (in.rkl2) refuse(kStellar, "is not supported with diffusion/integrator = rkl2");
    o.stellar_active = 1;
  }

  // the clips
  o.clip_r = in.clip_r, o.dfloor = in.dfloor, o.vceil = in.vceil, o.vAceil = in.vAceil, o.Tceil = in.Tceil;
  o.eceil = o.Tceil;
  const struct {
    const char *key;
    double v, def;
  } limits[] = {{"dfloor", o.dfloor, -1.0}, {"vceil", o.vceil, inf}, {"vAceil", o.vAceil, inf}, {"Tceil", o.Tceil, inf}};
  if (!(o.clip_r > 0.0))
    for (const auto &l : limits)
      if (l.v != l.def) refuse(std::string(kClips) + "/" + l.key, "is set with problem/cluster/clips/clip_r <= 0: the clip would never act");
  if (o.vAceil < inf && !in.mhd) refuse(std::string(kClips) + "/vAceil", "needs hydro/fluid = glmmhd");
  if (o.eceil < inf) {
    if (!in.has_composition)
      refuse(std::string(kClips) + "/Tceil", "Temperature ceiling requires units and gas composition. Either set a 'units' block and the "
             "'hydro/He_mass_fraction' in input file or use a pressure floor (defined code units) instead.");
    o.eceil = o.Tceil / in.mbar_over_kb / (in.gamma - 1.0);
  }
  if (o.clip_r > 0.0) {
    // (the reference's condition to run at all, cluster_clips.cpp:56-58)
    if (!(o.dfloor > 0 || o.eceil < inf || o.vceil < inf || o.vAceil < inf))
      refuse(std::string(kClips) + "/clip_r", "> 0 with no limit set (dfloor, vceil, vAceil, Tceil): the clips would never act");
    if (in.rkl2) refuse(std::string(kClips) + "/clip_r", "> 0 is not supported with diffusion/integrator = rkl2");
    o.clips_active = 1;
  }
  return o;
}

void split_index_range(const double *x, int n, int first, double radius, int *lo, int *hi) {
  int l = 0, h = 0;
  triggering_index_range(x, n, radius, &l, &h);
  *lo = first + l, *hi = first + h;
}

}  // namespace apk
