// cluster_sources.hpp -- the host-side model of the cluster problem's SNIa feedback, stellar feedback and clips, free of
// the driver: what the reference's constructors derive from the deck's keys (src/pgen/cluster/snia_feedback.cpp:31-48,
// stellar_feedback.cpp:32-65, cluster.cpp:250-277), what this path refuses of them, and the split sources' active list of
// one block and direction.  Plain C++ (host/cluster_sources_model.cpp): a stand-alone program can link it together with
// host/feedback_model.cpp.
#pragma once

#include <string>

#include "../../../include/apk_host.h"

namespace apk {

// the keys as read (code units; defaults: the reference's) and what the rest of the deck says
struct ClusterSourcesInput {
  double power_per_bcg_mass = 0.0, mass_rate_per_bcg_mass = 0.0;
  bool snia_disabled = false;
  double stellar_radius = 0.0, exclusion_radius = 0.0, efficiency = 0.0, number_density_threshold = 0.0, temperature_threshold = 0.0;
  double accretion_radius = 0.0;  // problem/cluster/agn_triggering/accretion_radius: the exclusion radius' fallback
  double clip_r = -1.0, dfloor = -1.0;
  double vceil = 0.0, vAceil = 0.0, Tceil = 0.0;  // (+inf: none)
  int which_bcg_g = APK_BCG_NONE;
  double m_bcg_s = 0.0, r_bcg_s = 0.0;
  bool mhd = false, rkl2 = false, has_composition = false;
  double gamma = 0.0, mu = 0.0, mh = 0.0, mbar_over_kb = 0.0, speed_of_light = 0.0;  // (the last four: with a composition)
};

// calc_rho_const_bcg (cluster_gravity.hpp:89-102)
double rho_const_bcg(int which_bcg_g, double m_bcg_s, double r_bcg_s);
// the options with everything derived; active_blocks and active_box_cells are left 0.  Throws std::runtime_error
// "problem_id = cluster: <key> <why>" for what is refused
apk_cluster_source_options cluster_source_options(const ClusterSourcesInput &in);
// The split sources' active list of one block and one direction: the range [lo, hi) of extended indices whose INTERIOR
// cells can satisfy |x| < radius, widened by one cell per side and clipped to the interior.  x[n]: the centres of the
// block's n interior cells, `first` the extended index of the first one.  lo >= hi: no cell.
void split_index_range(const double *x, int n, int first, double radius, int *lo, int *hi);

}  // namespace apk
