// restart_format.hpp -- the state file of a restart dump (host/restart.cpp), plain C++ without HIP: text in the deck
// format -- the deck as parsed, plus the block <apk_amd/restart> with the driver's mutable state and, for problem_id =
// turbulence, the driver's spectral state and RNG in <problem/turbulence> under the reference's own names
// (src/pgen/turbulence.cpp:166-197).  Doubles are written as %.17g, which strtod reads back exactly (inf included).
// tools/restart/format_check.cpp builds against this header, params.hpp and restart_format.cpp alone.
#pragma once

#include <string>
#include <vector>

#include "params.hpp"

namespace apk {

constexpr int kRestartFormatVersion = 1;
constexpr const char *kRestartBlock = "apk_amd/restart";

struct RestartBlock {  // one global block: key block_<gid> = level lx1 lx2 lx3 deref_count rank index
  int level = 0;
  int lx[3] = {0, 0, 0};    // logical location at its level
  int deref_count = 0;      // adaptive meshes: consecutive derefinement requests
  int rank = 0, index = 0;  // the rank whose .npy file holds it, and its position there
};

struct RestartOutput {  // one <parthenon/outputN> block (hst, npy, rst): keys output<N>_next_time, output<N>_counter
  std::string number;   // N as in the block's name
  double next_time = 0.0;
  long long counter = 0;  // files (rows, for hst) written so far
};

struct RestartState {
  int format_version = kRestartFormatVersion;
  double time = 0.0, dt = 0.0;
  long long cycle = 0;
  double dt_hyp = 0.0, mindx = 0.0, c_h = 0.0, dt_diff = 0.0;  // the package's mutable params
  long long fofc_total = 0, fofc_fallback_stages = 0, zone_cycles = 0, amr_refined = 0, amr_derefined = 0;
  int nranks = 1;
  std::string fluid;       // "euler" | "glmmhd"
  std::string refinement;  // "none" | "static" | "adaptive"
  int nvar = 0, nghost = 0;
  int mesh_nx[3] = {1, 1, 1}, block_nx[3] = {1, 1, 1};
  std::vector<RestartBlock> blocks;  // gid order (key nblocks = their number)
  // the cluster problem's scalars
  bool has_triggering = false;
  double trig_reduced[5] = {0, 0, 0, 0, 0};  // cold_mass, total_mass, mass_weighted_density, _velocity, _cs
  double trig_rate = 0.0, trig_time = 0.0, trig_dt = 0.0;
  bool has_split_totals = false;
  double split_totals[5] = {0, 0, 0, 0, 0};
  std::vector<RestartOutput> outputs;
  // problem_id = turbulence (FewModesFT::SaveState): [3][M][re, im]
  bool has_turbulence = false;
  std::vector<double> accel_hat;
  std::string state_rng, state_dist;
};

// a double as %.17g
std::string restart_real(double v);
// the state into `pin`: <apk_amd/restart> (whatever it held before is dropped) and the turbulence keys
void restart_state_store(const RestartState &st, ParameterInput &pin);
// the text of the state file: `deck` with the state stored into it
std::string restart_file_text(const ParameterInput &deck, const RestartState &st);
// the state out of a parsed state file; throws std::runtime_error naming the key that is missing or malformed, or
// format_version if it is not kRestartFormatVersion.  The turbulence state is read where state_rng exists.
void restart_state_load(const ParameterInput &pin, RestartState &st);

}  // namespace apk
