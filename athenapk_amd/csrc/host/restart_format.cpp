// restart_format.cpp -- writing and parsing the state file of a restart dump (restart_format.hpp).  No HIP, no driver state.
#include "restart_format.hpp"

#include <cstdio>
#include <cstdlib>
#include <sstream>

namespace apk {

std::string restart_real(double v) {
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}

namespace {

const char *kTrigKeys[5] = {"trig_cold_mass", "trig_total_mass", "trig_mass_weighted_density", "trig_mass_weighted_velocity",
                            "trig_mass_weighted_cs"};
const char *kTurb = "problem/turbulence";

std::string hat_key(int i, int m, bool imag) {
  return "accel_hat_" + std::to_string(i) + "_" + std::to_string(m) + (imag ? "_i" : "_r");
}

long long get_ll(const ParameterInput &pin, const std::string &key) {
  const std::string v = pin.GetString(kRestartBlock, key);
  char *end = nullptr;
  const long long x = std::strtoll(v.c_str(), &end, 10);
  if (end == v.c_str() || *end != '\0') throw std::runtime_error(std::string("restart: <") + kRestartBlock + "> " + key + " is not an integer: " + v);
  return x;
}

double get_real(const ParameterInput &pin, const std::string &block, const std::string &key) {
  const std::string v = pin.GetString(block, key);
  char *end = nullptr;
  const double x = std::strtod(v.c_str(), &end);
  if (end == v.c_str() || *end != '\0') throw std::runtime_error("restart: <" + block + "> " + key + " is not a number: " + v);
  return x;
}

void get_ints(const ParameterInput &pin, const std::string &key, int *out, int n) {
  std::istringstream in(pin.GetString(kRestartBlock, key));
  for (int q = 0; q < n; ++q)
    if (!(in >> out[q])) throw std::runtime_error(std::string("restart: <") + kRestartBlock + "> " + key + " needs " + std::to_string(n) + " integers");
  std::string rest;
  if (in >> rest) throw std::runtime_error(std::string("restart: <") + kRestartBlock + "> " + key + " has more than " + std::to_string(n) + " integers");
}

std::string ints(const int *v, int n) {
  std::string s;
  for (int q = 0; q < n; ++q) s += (q ? " " : "") + std::to_string(v[q]);
  return s;
}

}  // namespace

void restart_state_store(const RestartState &st, ParameterInput &pin) {
  const std::string B = kRestartBlock;
  for (const std::string &k : pin.KeysOf(B)) pin.Erase(B, k);
  auto real = [&](const char *k, double v) { pin.Set(B, k, restart_real(v)); };
  auto integer = [&](const char *k, long long v) { pin.Set(B, k, std::to_string(v)); };
  integer("format_version", st.format_version);
  real("time", st.time);
  integer("cycle", st.cycle);
  real("dt", st.dt);
  real("dt_hyp", st.dt_hyp);
  real("mindx", st.mindx);
  real("c_h", st.c_h);
  real("dt_diff", st.dt_diff);
  integer("fofc_total", st.fofc_total);
  integer("fofc_fallback_stages", st.fofc_fallback_stages);
  integer("zone_cycles", st.zone_cycles);
  integer("amr_refined", st.amr_refined);
  integer("amr_derefined", st.amr_derefined);
  integer("nranks", st.nranks);
  integer("nblocks", (long long)st.blocks.size());
  pin.Set(B, "fluid", st.fluid);
  pin.Set(B, "refinement", st.refinement);
  integer("nvar", st.nvar);
  integer("nghost", st.nghost);
  pin.Set(B, "mesh_nx", ints(st.mesh_nx, 3));
  pin.Set(B, "block_nx", ints(st.block_nx, 3));
  for (size_t g = 0; g < st.blocks.size(); ++g) {
    const RestartBlock &b = st.blocks[g];
    const int row[7] = {b.level, b.lx[0], b.lx[1], b.lx[2], b.deref_count, b.rank, b.index};
    pin.Set(B, "block_" + std::to_string(g), ints(row, 7));
  }
  if (st.has_triggering) {
    for (int q = 0; q < 5; ++q) real(kTrigKeys[q], st.trig_reduced[q]);
    real("trig_rate", st.trig_rate);
    real("trig_time", st.trig_time);
    real("trig_dt", st.trig_dt);
  }
  if (st.has_split_totals)
    for (int q = 0; q < 5; ++q) pin.Set(B, "split_totals_" + std::to_string(q), restart_real(st.split_totals[q]));
  for (const RestartOutput &o : st.outputs) {
    pin.Set(B, "output" + o.number + "_next_time", restart_real(o.next_time));
    pin.Set(B, "output" + o.number + "_counter", std::to_string(o.counter));
  }
  // the turbulence driver: whatever an earlier dump left goes first (the number of modes is the deck's)
  for (const std::string &k : pin.KeysOf(kTurb))
    if (k.compare(0, 10, "accel_hat_") == 0 || k == "state_rng" || k == "state_dist") pin.Erase(kTurb, k);
  if (st.has_turbulence) {
    const int M = (int)(st.accel_hat.size() / 6);
    for (int i = 0; i < 3; ++i)
      for (int m = 0; m < M; ++m) {
        pin.Set(kTurb, hat_key(i, m, false), restart_real(st.accel_hat[((size_t)i * M + m) * 2]));
        pin.Set(kTurb, hat_key(i, m, true), restart_real(st.accel_hat[((size_t)i * M + m) * 2 + 1]));
      }
    pin.Set(kTurb, "state_rng", st.state_rng);
    pin.Set(kTurb, "state_dist", st.state_dist);
  }
}

std::string restart_file_text(const ParameterInput &deck, const RestartState &st) {
  ParameterInput pin = deck;
  restart_state_store(st, pin);
  return pin.Dump();
}

void restart_state_load(const ParameterInput &pin, RestartState &st) {
  const std::string B = kRestartBlock;
  if (!pin.DoesParameterExist(B, "format_version"))
    throw std::runtime_error("restart: not a state file: <" + B + "> format_version is missing");
  st = RestartState();
  st.format_version = (int)get_ll(pin, "format_version");
  if (st.format_version != kRestartFormatVersion)
    throw std::runtime_error("restart: <" + B + "> format_version = " + std::to_string(st.format_version) + ", this build reads " +
                             std::to_string(kRestartFormatVersion));
  st.time = get_real(pin, B, "time");
  st.cycle = get_ll(pin, "cycle");
  st.dt = get_real(pin, B, "dt");
  st.dt_hyp = get_real(pin, B, "dt_hyp");
  st.mindx = get_real(pin, B, "mindx");
  st.c_h = get_real(pin, B, "c_h");
  st.dt_diff = get_real(pin, B, "dt_diff");
  st.fofc_total = get_ll(pin, "fofc_total");
  st.fofc_fallback_stages = get_ll(pin, "fofc_fallback_stages");
  st.zone_cycles = get_ll(pin, "zone_cycles");
  st.amr_refined = get_ll(pin, "amr_refined");
  st.amr_derefined = get_ll(pin, "amr_derefined");
  st.nranks = (int)get_ll(pin, "nranks");
  st.fluid = pin.GetString(B, "fluid");
  st.refinement = pin.GetString(B, "refinement");
  st.nvar = (int)get_ll(pin, "nvar");
  st.nghost = (int)get_ll(pin, "nghost");
  get_ints(pin, "mesh_nx", st.mesh_nx, 3);
  get_ints(pin, "block_nx", st.block_nx, 3);
  const long long nb = get_ll(pin, "nblocks");
  if (nb < 1 || nb > (1LL << 30) || st.nranks < 1) throw std::runtime_error("restart: <" + B + "> nblocks / nranks out of range");
  st.blocks.resize((size_t)nb);
  std::vector<long long> per_rank((size_t)st.nranks, 0);
  for (long long g = 0; g < nb; ++g) {
    int row[7];
    get_ints(pin, "block_" + std::to_string(g), row, 7);
    RestartBlock &b = st.blocks[(size_t)g];
    b.level = row[0], b.lx[0] = row[1], b.lx[1] = row[2], b.lx[2] = row[3], b.deref_count = row[4], b.rank = row[5], b.index = row[6];
    if (b.level < 0 || b.level > 30 || b.lx[0] < 0 || b.lx[1] < 0 || b.lx[2] < 0 || b.rank < 0 || b.rank >= st.nranks || b.index < 0 || b.index >= nb)
      throw std::runtime_error("restart: <" + B + "> block_" + std::to_string(g) + " is out of range");
    per_rank[(size_t)b.rank] += 1;
  }
  for (const RestartBlock &b : st.blocks)
    if (b.index >= per_rank[(size_t)b.rank]) throw std::runtime_error("restart: <" + B + "> block table: an index beyond its rank's block count");
  st.has_triggering = pin.DoesParameterExist(B, "trig_rate");
  if (st.has_triggering) {
    for (int q = 0; q < 5; ++q) st.trig_reduced[q] = get_real(pin, B, kTrigKeys[q]);
    st.trig_rate = get_real(pin, B, "trig_rate");
    st.trig_time = get_real(pin, B, "trig_time");
    st.trig_dt = get_real(pin, B, "trig_dt");
  }
  st.has_split_totals = pin.DoesParameterExist(B, "split_totals_0");
  if (st.has_split_totals)
    for (int q = 0; q < 5; ++q) st.split_totals[q] = get_real(pin, B, "split_totals_" + std::to_string(q));
  for (const std::string &k : pin.KeysOf(B)) {
    const std::string tail = "_next_time";
    if (k.compare(0, 6, "output") != 0 || k.size() <= 6 + tail.size() || k.compare(k.size() - tail.size(), tail.size(), tail) != 0) continue;
    RestartOutput o;
    o.number = k.substr(6, k.size() - 6 - tail.size());
    o.next_time = get_real(pin, B, k);
    o.counter = get_ll(pin, "output" + o.number + "_counter");
    st.outputs.push_back(o);
  }
  st.has_turbulence = pin.DoesParameterExist(kTurb, "state_rng");
  if (st.has_turbulence) {
    const int M = pin.GetInteger(kTurb, "num_modes");
    if (M < 1 || M > (1 << 20)) throw std::runtime_error("restart: <problem/turbulence> num_modes out of range");
    st.accel_hat.resize((size_t)M * 6);
    for (int i = 0; i < 3; ++i)
      for (int m = 0; m < M; ++m) {
        st.accel_hat[((size_t)i * M + m) * 2] = get_real(pin, kTurb, hat_key(i, m, false));
        st.accel_hat[((size_t)i * M + m) * 2 + 1] = get_real(pin, kTurb, hat_key(i, m, true));
      }
    st.state_rng = pin.GetString(kTurb, "state_rng");
    st.state_dist = pin.GetString(kTurb, "state_dist");
  }
}

}  // namespace apk
