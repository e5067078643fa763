// format_check.cpp -- stand-alone host program for the state file of a restart dump (csrc/host/restart_format.cpp):
// writes a state with a forest of mixed levels, the turbulence driver's spectral state and the operator<< text of a
// std::mt19937 (625 words) through those functions into a deck, reads the file back with the deck reader and checks every
// field -- doubles through %.17g (a value that needs all 17 digits, the largest double, inf, a denormal, -0.0), 64-bit
// counters, the block table, the output schedules, the turbulence keys under the reference's names -- then that the RNG
// restored from the text draws what the original draws, that a second store drops what the first left, and that another
// format_version, a missing key and a malformed block row are refused with a message naming the key.  No GPU, no Python;
// meant to be compiled with sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/restart/format_check.cpp athenapk_amd/csrc/host/restart_format.cpp athenapk_amd/csrc/host/snapshot_format.cpp \
//       -o /tmp/restart_format_check && /tmp/restart_format_check /tmp
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../athenapk_amd/csrc/host/restart_format.hpp"
#include "../../athenapk_amd/csrc/host/snapshot_format.hpp"
#include "../../athenapk_amd/csrc/host/turbulence.hpp"

using namespace apk;

namespace {
int check(bool ok, const char *what) {
  if (!ok) std::printf("FAILED: %s\n", what);
  return ok ? 1 : 0;
}

std::string slurp(const std::string &path) {
  std::string s;
  FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return s;
  char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  std::fclose(f);
  return s;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the message of restart_state_load on `pin`, empty if it passes
std::string refusal(const ParameterInput &pin) {
  RestartState st;
  try {
    restart_state_load(pin, st);
  } catch (const std::exception &e) {
    return e.what();
  }
  return "";
}
}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  int ok = 1;

  // a deck with comments, an empty block and a key that an override added
  ParameterInput deck;
  deck.LoadFromString("<job>\nproblem_id = turbulence  # comment\n\n<parthenon/mesh>\nnx1 = 32\nrefinement = adaptive\n\n<empty/block>\n\n"
                      "<problem/turbulence>\nnum_modes = 2\nrseed = 7\naccel_hat_0_9_r = 1.0\n");
  deck.ApplyOverride("parthenon/time/tlim=2.0");

  // a turbulence driver that has drawn numbers: its state is what the file must carry
  const int gnx[3] = {32, 32, 32};
  FewModesFT fm(2, {1, 0, 0, 1, 1, -1}, 2.0, 1.0, 1.0, 7u, gnx);
  fm.Evolve(0.01);
  fm.Evolve(0.02);

  RestartState st;
  st.time = 0.1 + 0.2;  // 0.30000000000000004: needs all 17 digits
  st.dt = 4.9406564584124654e-324;
  st.cycle = 123456789012LL;
  st.dt_hyp = DBL_MAX;
  st.mindx = 1.0 / 3.0;
  st.c_h = -0.0;
  st.dt_diff = std::numeric_limits<double>::infinity();
  st.fofc_total = 9007199254740993LL;  // (not a double)
  st.fofc_fallback_stages = 3, st.zone_cycles = 1LL << 40, st.amr_refined = 17, st.amr_derefined = 2;
  st.nranks = 2;
  st.fluid = "glmmhd";
  st.refinement = "adaptive";
  st.nvar = 11, st.nghost = 3;
  const int mesh[3] = {32, 16, 1}, blk[3] = {8, 8, 1};
  for (int d = 0; d < 3; ++d) st.mesh_nx[d] = mesh[d], st.block_nx[d] = blk[d];
  // a forest of mixed levels: root block 0 split into four (one of them split again), the other seven roots whole
  auto add = [&](int level, int x, int y, int deref) {
    RestartBlock b;
    b.level = level, b.lx[0] = x, b.lx[1] = y, b.deref_count = deref;
    b.rank = (int)st.blocks.size() % 2, b.index = (int)st.blocks.size() / 2;
    st.blocks.push_back(b);
  };
  for (int c = 0; c < 4; ++c) add(2, c % 2, c / 2, 9 - c);
  for (int c = 1; c < 4; ++c) add(1, c % 2, c / 2, c);
  for (int r = 1; r < 8; ++r) add(0, r % 4, r / 4, 0);
  st.has_triggering = true;
  for (int q = 0; q < 5; ++q) st.trig_reduced[q] = std::ldexp(1.0 / 7.0, 10 * q);
  st.trig_rate = 1e-300, st.trig_time = 0.25, st.trig_dt = 1.0 / 1024.0;
  st.has_split_totals = true;
  for (int q = 0; q < 5; ++q) st.split_totals[q] = -std::ldexp(1.0 / 11.0, -q);
  st.outputs = {{"1", 0.1 * 3, 4}, {"2", 0.5, 1}, {"13", 1.5, 123456}};
  st.has_turbulence = true;
  fm.SaveState(st.accel_hat, st.state_rng, st.state_dist);
  {
    std::istringstream words(st.state_rng);
    std::string w;
    int n = 0;
    while (words >> w) ++n;
    ok &= check(n == 625, "the mt19937 text has 625 words");
  }

  const std::string path = dir + "/restart_format_check.rst";
  const std::string text = restart_file_text(deck, st);
  ok &= check(write_text_file(path, text), "state file written");
  const std::string back_text = slurp(path);
  ok &= check(back_text == text, "state file read back");
  ParameterInput pin;
  pin.LoadFromString(back_text);

  // the deck itself survives: every block and key, overrides included, comments gone, the stale turbulence key dropped
  ok &= check(pin.GetString("job", "problem_id") == "turbulence", "deck key");
  ok &= check(pin.GetReal("parthenon/time", "tlim") == 2.0, "override kept");
  ok &= check(pin.DoesBlockExist("empty/block"), "a block without keys keeps its header");
  ok &= check(!pin.DoesParameterExist("problem/turbulence", "accel_hat_0_9_r"), "a stale accel_hat key is dropped");
  ok &= check(pin.GetInteger("problem/turbulence", "rseed") == 7, "the block's own keys stay");

  RestartState rd;
  try {
    restart_state_load(pin, rd);
  } catch (const std::exception &e) {
    std::printf("FAILED: load: %s\n", e.what());
    return 1;
  }
  ok &= check(rd.format_version == kRestartFormatVersion, "format_version");
  ok &= check(same_bits(rd.time, st.time) && same_bits(rd.dt, st.dt) && same_bits(rd.dt_hyp, DBL_MAX) && same_bits(rd.mindx, st.mindx), "doubles round-trip");
  ok &= check(same_bits(rd.c_h, -0.0), "-0.0 round-trips");
  ok &= check(std::isinf(rd.dt_diff) && rd.dt_diff > 0, "inf round-trips");
  ok &= check(rd.cycle == st.cycle && rd.fofc_total == st.fofc_total && rd.zone_cycles == st.zone_cycles, "64-bit counters");
  ok &= check(rd.fofc_fallback_stages == 3 && rd.amr_refined == 17 && rd.amr_derefined == 2, "counters");
  ok &= check(rd.nranks == 2 && rd.fluid == "glmmhd" && rd.refinement == "adaptive" && rd.nvar == 11 && rd.nghost == 3, "layout keys");
  ok &= check(std::memcmp(rd.mesh_nx, mesh, sizeof mesh) == 0 && std::memcmp(rd.block_nx, blk, sizeof blk) == 0, "extents");
  ok &= check(rd.blocks.size() == st.blocks.size() && rd.blocks.size() == 14, "block count");
  for (size_t g = 0; ok && g < st.blocks.size(); ++g) {
    const RestartBlock &a = st.blocks[g], &b = rd.blocks[g];
    ok &= check(a.level == b.level && std::memcmp(a.lx, b.lx, sizeof a.lx) == 0 && a.deref_count == b.deref_count && a.rank == b.rank && a.index == b.index, "block row");
  }
  ok &= check(pin.GetString(kRestartBlock, "block_0") == "2 0 0 0 9 0 0" && pin.GetString(kRestartBlock, "block_13") == "0 3 1 0 0 1 6", "block row text");
  ok &= check(rd.has_triggering && rd.has_split_totals, "cluster scalars present");
  for (int q = 0; q < 5; ++q) ok &= check(same_bits(rd.trig_reduced[q], st.trig_reduced[q]) && same_bits(rd.split_totals[q], st.split_totals[q]), "cluster scalars");
  ok &= check(same_bits(rd.trig_rate, 1e-300) && rd.trig_time == 0.25 && rd.trig_dt == 1.0 / 1024.0, "triggering scalars");
  ok &= check(rd.outputs.size() == 3, "output schedules");
  for (const RestartOutput &o : rd.outputs)
    for (const RestartOutput &w : st.outputs)
      if (o.number == w.number) ok &= check(same_bits(o.next_time, w.next_time) && o.counter == w.counter, "output schedule");
  ok &= check(rd.has_turbulence && rd.accel_hat.size() == 12 && rd.state_rng == st.state_rng && rd.state_dist == st.state_dist, "turbulence state");
  for (size_t q = 0; q < st.accel_hat.size() && q < rd.accel_hat.size(); ++q) ok &= check(same_bits(rd.accel_hat[q], st.accel_hat[q]), "accel_hat");
  ok &= check(pin.DoesParameterExist("problem/turbulence", "accel_hat_2_1_i") && pin.DoesParameterExist("problem/turbulence", "state_dist"),
              "the reference's key names");

  // the restored driver goes on as the original does
  FewModesFT fresh(2, {1, 0, 0, 1, 1, -1}, 2.0, 1.0, 1.0, 7u, gnx);
  ok &= check(fresh.RestoreState(rd.accel_hat, rd.state_rng, rd.state_dist), "RestoreState");
  FewModesFT seeded(2, {1, 0, 0, 1, 1, -1}, 2.0, 1.0, 1.0, 7u, gnx);
  fm.Evolve(0.03), fresh.Evolve(0.03), seeded.Evolve(0.03);
  bool same = true, differs = false;
  for (size_t q = 0; q < fm.var_hat().size(); ++q) {
    same = same && fm.var_hat()[q] == fresh.var_hat()[q];
    differs = differs || fm.var_hat()[q] != seeded.var_hat()[q];
  }
  ok &= check(same, "the restored driver draws what the original draws");
  ok &= check(differs, "a freshly seeded driver does not");
  ok &= check(!fresh.RestoreState(rd.accel_hat, "not a generator", rd.state_dist), "a text that does not parse is refused");
  ok &= check(!fresh.RestoreState(std::vector<double>(6), rd.state_rng, rd.state_dist), "another number of modes is refused");

  // a second store into the parsed file: a smaller forest and no cluster or turbulence state leave nothing stale behind
  RestartState small = st;
  small.blocks.resize(3);
  small.has_triggering = small.has_split_totals = small.has_turbulence = false;
  small.outputs.clear();
  restart_state_store(small, pin);
  ok &= check(!pin.DoesParameterExist(kRestartBlock, "block_3") && !pin.DoesParameterExist(kRestartBlock, "trig_rate") &&
                  !pin.DoesParameterExist(kRestartBlock, "output13_counter") && !pin.DoesParameterExist("problem/turbulence", "state_rng"),
              "a second store drops what the first left");
  ok &= check(refusal(pin).empty(), "the second state loads");

  // refusals name the key
  ParameterInput bad = pin;
  bad.Set(kRestartBlock, "format_version", "2");
  ok &= check(refusal(bad).find("format_version") != std::string::npos, "another format_version is refused");
  bad = pin;
  bad.Erase(kRestartBlock, "c_h");
  ok &= check(refusal(bad).find("c_h") != std::string::npos, "a missing key is named");
  bad = pin;
  bad.Set(kRestartBlock, "block_1", "1 0 0");
  ok &= check(refusal(bad).find("block_1") != std::string::npos, "a short block row is named");
  bad = pin;
  bad.Set(kRestartBlock, "block_2", "0 0 0 0 0 5 0");
  ok &= check(refusal(bad).find("block_2") != std::string::npos, "a rank beyond nranks is named");
  bad = pin;
  bad.Set(kRestartBlock, "time", "soon");
  ok &= check(refusal(bad).find("time") != std::string::npos, "a malformed double is named");
  ParameterInput none;
  none.LoadFromString("<job>\nproblem_id = sod\n");
  ok &= check(refusal(none).find("format_version") != std::string::npos, "a plain deck is not a state file");

  std::remove(path.c_str());
  std::printf(ok ? "format_check: ok\n" : "format_check: FAILED\n");
  return ok ? 0 : 1;
}
