// restart.cpp -- restart dumps of the standalone driver and resuming from one: the deck's rst output blocks, the dump (a
// field snapshot of `cons` in double through host/snapshot.cpp, then the state file of restart_format.cpp), the chunked
// way back through the pinned and the device staging buffer into the unpack kernel (apk_restart_unpack,
// csrc/kernels_output.hip), and the C API of include/apk_host.h.
//
// Writing reads the interior of the current conserved buffer and the driver's scalars and changes nothing: the writing
// run takes the stage forms and exchanges of one that does not write.  Restoring takes the place of apk_sim_initialize:
// it ends with complete ghost zones and stored primitives, and with the stored dt, dt_hyp, mindx and c_h -- no time step
// is estimated, because set_global_dt's growth limit and the next cycle's c_h depend on the stored ones.
#include "restart_format.hpp"
#include "sim_internal.hpp"

#include <algorithm>
#include <map>

namespace apk {
namespace host {

namespace {

const char *refinement_mode(const apk_sim *s) { return s->amr ? (s->amr_adaptive ? "adaptive" : "static") : "none"; }

std::string triple(const int v[3]) { return std::to_string(v[0]) + " " + std::to_string(v[1]) + " " + std::to_string(v[2]); }

// what of a state file must equal the sim it is restored into; empty, or the message naming the deck key that differs
std::string mismatch(const apk_sim *s, const RestartState &st) {
  const Mesh &m = s->mesh;
  static const char *ax[3] = {"nx1", "nx2", "nx3"};
  for (int d = 0; d < 3; ++d)
    if (st.mesh_nx[d] != m.nx[d])
      return std::string("restart: parthenon/mesh/") + ax[d] + " = " + std::to_string(m.nx[d]) + ", the state file has mesh_nx = " + triple(st.mesh_nx);
  for (int d = 0; d < 3; ++d)
    if (st.block_nx[d] != m.mb[d])
      return std::string("restart: parthenon/meshblock/") + ax[d] + " = " + std::to_string(m.mb[d]) + ", the state file has block_nx = " + triple(st.block_nx);
  if (st.nghost != m.ng) return "restart: parthenon/mesh/nghost = " + std::to_string(m.ng) + ", the state file has nghost = " + std::to_string(st.nghost);
  const std::string fluid = s->pkg.fluid == APK_FLUID_GLMMHD ? "glmmhd" : "euler";
  if (st.fluid != fluid) return "restart: hydro/fluid = " + fluid + ", the state file has fluid = " + st.fluid;
  if (st.nvar != s->pkg.nhydro + s->pkg.nscalars)
    return "restart: hydro/nscalars = " + std::to_string(s->pkg.nscalars) + " makes " + std::to_string(s->pkg.nhydro + s->pkg.nscalars) +
           " variables, the state file has nvar = " + std::to_string(st.nvar);
  if (st.refinement != refinement_mode(s))
    return std::string("restart: parthenon/mesh/refinement = ") + refinement_mode(s) + ", the state file has refinement = " + st.refinement;
  return "";
}

void collect_state(const apk_sim *s, RestartState &st) {
  const Mesh &m = s->mesh;
  st.time = s->host_only ? 0.0 : s->time;
  st.cycle = s->host_only ? 0 : s->ncycle;
  st.dt = s->dt;
  st.dt_hyp = s->pkg.dt_hyp, st.mindx = s->pkg.mindx, st.c_h = s->pkg.c_h, st.dt_diff = s->pkg.dt_diff;
  st.fofc_total = s->fofc_total, st.fofc_fallback_stages = s->fofc_fallback_stages, st.zone_cycles = s->zone_cycles;
  st.amr_refined = s->amr_refined, st.amr_derefined = s->amr_derefined;
  st.nranks = s->nranks;
  st.fluid = s->pkg.fluid == APK_FLUID_GLMMHD ? "glmmhd" : "euler";
  st.refinement = refinement_mode(s);
  st.nvar = s->pkg.nhydro + s->pkg.nscalars;
  st.nghost = m.ng;
  for (int d = 0; d < 3; ++d) st.mesh_nx[d] = m.nx[d], st.block_nx[d] = m.mb[d];
  std::vector<SnapshotBlock> table;
  snapshot_block_table(s, table);
  st.blocks.resize(table.size());
  for (size_t g = 0; g < table.size(); ++g) {
    RestartBlock &b = st.blocks[g];
    b.level = table[g].level;
    for (int d = 0; d < 3; ++d) b.lx[d] = table[g].lx[d];
    b.deref_count = s->amr ? s->amr->leaves[g].deref_count : 0;
    b.rank = table[g].rank, b.index = table[g].index;
  }
  st.has_triggering = s->pkg.agn_triggering;
  if (st.has_triggering) {
    const auto &q = s->trig_q;
    const double r[5] = {q.cold_mass, q.total_mass, q.mass_weighted_density, q.mass_weighted_velocity, q.mass_weighted_cs};
    for (int n = 0; n < 5; ++n) st.trig_reduced[n] = r[n];
    st.trig_rate = s->trig_rate, st.trig_time = s->trig_time, st.trig_dt = s->trig_dt;
  }
  st.has_split_totals = s->cluster.enabled != 0;
  for (int n = 0; n < 5; ++n) st.split_totals[n] = s->split_totals[n];
  for (const OutputSchedule &o : s->out_sched) {
    RestartOutput r;
    r.number = o.number, r.next_time = o.next, r.counter = o.counter;
    st.outputs.push_back(r);
  }
  st.has_turbulence = (bool)s->fmft;
  if (s->fmft) s->fmft->SaveState(st.accel_hat, st.state_rng, st.state_dist);
}

int write_state_file(apk_sim *s, const std::string &prefix) {
  RestartState st;
  collect_state(s, st);
  const std::string path = prefix + ".rst", tmp = path + ".tmp";
  if (!write_text_file(tmp, restart_file_text(s->pin, st))) return fail(s, APK_ERR_INVALID, "cannot write " + tmp);
  if (std::rename(tmp.c_str(), path.c_str()) != 0) return fail(s, APK_ERR_INVALID, "cannot rename " + tmp + " to " + path);
  return APK_OK;
}

bool read_text_file(const std::string &path, std::string &text) {
  FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  text.clear();
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}

// one rank's array file of a dump, opened and checked against what the block table says it holds
struct RankFile {
  FILE *f = nullptr;
  long long data = 0;  // offset of the first block
  ~RankFile() {
    if (f) std::fclose(f);
  }
};

int open_rank_file(apk_sim *s, const std::string &path, long long nblocks, int nvar, const int nx[3], size_t per_block, RankFile &rf) {
  rf.f = std::fopen(path.c_str(), "rb");
  if (!rf.f) return fail(s, APK_ERR_INVALID, "restore: cannot open " + path);
  unsigned char head[10];
  if (std::fread(head, 1, 10, rf.f) != 10 || std::memcmp(head, "\x93NUMPY\x01\x00", 8) != 0)
    return fail(s, APK_ERR_INVALID, "restore: " + path + " is not a NumPy 1.0 file");
  const size_t hlen = head[8] | ((size_t)head[9] << 8);
  std::string dict(hlen, '\0');
  if (std::fread(&dict[0], 1, hlen, rf.f) != hlen) return fail(s, APK_ERR_INVALID, "restore: " + path + " ends inside its header");
  const std::string shape = "'shape': (" + std::to_string(nblocks) + ", " + std::to_string(nvar) + ", " + std::to_string(nx[2]) + ", " +
                            std::to_string(nx[1]) + ", " + std::to_string(nx[0]) + ")";
  if (dict.find("'descr': '<f8'") == std::string::npos || dict.find("'fortran_order': False") == std::string::npos ||
      dict.find(shape) == std::string::npos)
    return fail(s, APK_ERR_INVALID, "restore: " + path + " does not hold '<f8' with " + shape + ": " + dict.substr(0, dict.find('}') + 1));
  rf.data = 10 + (long long)hlen;
  if (fseeko(rf.f, 0, SEEK_END) != 0) return fail(s, APK_ERR_INVALID, "restore: cannot seek in " + path);
  const long long size = (long long)ftello(rf.f);
  if (size < rf.data + nblocks * (long long)per_block)
    return fail(s, APK_ERR_INVALID, "restore: " + path + " is truncated: " + std::to_string(size) + " bytes, " +
                                        std::to_string(rf.data + nblocks * (long long)per_block) + " expected");
  return APK_OK;
}

// every rank file the block table names, opened and checked (header, shape, size) before anything of the sim changes
int check_rank_files(apk_sim *s, const std::string &prefix, const RestartState &st) {
  const Mesh &m = s->mesh;
  const size_t per_block = (size_t)st.nvar * (size_t)m.mb[0] * m.mb[1] * m.mb[2] * sizeof(double);
  std::vector<long long> per_rank((size_t)st.nranks, 0);
  for (const RestartBlock &b : st.blocks) per_rank[(size_t)b.rank] += 1;
  for (int r = 0; r < st.nranks; ++r) {
    if (per_rank[(size_t)r] == 0) continue;
    RankFile rf;
    SIM_TRY(s, open_rank_file(s, prefix + ".rank" + std::to_string(r) + ".npy", per_rank[(size_t)r], st.nvar, m.mb, per_block, rf));
  }
  return APK_OK;
}

// the forest of an adaptive mesh as the state file has it, derefinement counters included; fresh arrays for it
int install_forest(apk_sim *s, const RestartState &st) {
  AmrTree &t = *s->amr;
  std::unordered_map<uint64_t, AmrLeaf> leafmap;
  std::unordered_set<uint64_t> internal;
  for (const RestartBlock &b : st.blocks) {
    if (b.level > t.max_level) return fail(s, APK_ERR_INVALID, "restore: a block of level " + std::to_string(b.level) + ", the deck allows " + std::to_string(t.max_level));
    for (int d = 0; d < 3; ++d)
      if (b.lx[d] >= (t.act[d] ? (t.nrb[d] << b.level) : 1)) return fail(s, APK_ERR_INVALID, "restore: a block outside the mesh in the block table");
    AmrLeaf l;
    l.level = b.level, l.deref_count = b.deref_count;
    for (int d = 0; d < 3; ++d) l.lx[d] = b.lx[d];
    leafmap[AmrTree::Key(l.level, l.lx)] = l;
    int p[3] = {l.lx[0], l.lx[1], l.lx[2]};
    for (int lev = l.level; lev > 0; --lev) {
      for (int d = 0; d < 3; ++d) p[d] >>= 1;
      internal.insert(AmrTree::Key(lev - 1, p));
    }
  }
  if (leafmap.size() != st.blocks.size()) return fail(s, APK_ERR_INVALID, "restore: the block table names a block twice");
  t.leafmap.swap(leafmap);
  t.internal.swap(internal);
  t.modifications += 1;
  t.Reindex();
  for (size_t g = 0; g < st.blocks.size(); ++g) {
    const AmrLeaf &l = t.leaves[g];
    const RestartBlock &b = st.blocks[g];
    if (l.level != b.level || l.lx[0] != b.lx[0] || l.lx[1] != b.lx[1] || l.lx[2] != b.lx[2])
      return fail(s, APK_ERR_INVALID, "restore: the block table is not in the forest's Z-order");
  }
  if ((int)t.leaves.size() < s->nranks) return fail(s, APK_ERR_INVALID, "fewer meshblocks than ranks");
  return amr_reallocate(s);
}

// every local block's interior from the rank files of the dump, chunk by chunk: file -> pinned buffer -> one
// host-to-device copy -> unpack kernel -> sync (the two buffers are reused by the next chunk)
int unpack_blocks(apk_sim *s, const std::string &prefix, const RestartState &st) {
  const Mesh &m = s->mesh;
  apk_pack *md = s->mu0();
  if (!md) return fail(s, APK_ERR_INVALID, "restore: no pack presents the current state");
  const int nlb = (int)m.local_gids.size();
  const size_t per_block = (size_t)st.nvar * (size_t)m.mb[0] * m.mb[1] * m.mb[2] * sizeof(double);
  std::map<uint64_t, const RestartBlock *> by_loc;
  std::vector<long long> per_rank((size_t)st.nranks, 0);
  for (const RestartBlock &b : st.blocks) {
    by_loc[AmrTree::Key(b.level, b.lx)] = &b;
    per_rank[(size_t)b.rank] += 1;
  }
  std::vector<const RestartBlock *> src(nlb);
  for (int lb = 0; lb < nlb; ++lb) {
    int level = 0, lx[3];
    if (s->amr) {
      const AmrLeaf &l = amr_leaf(s, lb);
      level = l.level;
      for (int d = 0; d < 3; ++d) lx[d] = l.lx[d];
    } else {
      m.Loc(m.local_gids[lb], lx);
    }
    auto it = by_loc.find(AmrTree::Key(level, lx));
    if (it == by_loc.end())
      return fail(s, APK_ERR_INVALID, "restore: the block table has no block of level " + std::to_string(level) + " at " + triple(lx));
    src[lb] = it->second;
  }
  if (nlb == 0) return APK_OK;
  const size_t bound = std::max(per_block, std::min(s->snap_staging_bytes, per_block * (size_t)nlb));
  const int chunk_blocks = (int)std::min<size_t>(bound / per_block, (size_t)nlb);
  SIM_TRY(s, snapshot_staging(s, per_block * (size_t)chunk_blocks));
  std::map<int, RankFile> files;
  for (int first = 0; first < nlb; first += chunk_blocks) {
    const int n = std::min(chunk_blocks, nlb - first);
    for (int q = 0; q < n; ++q) {
      const RestartBlock &b = *src[first + q];
      RankFile &rf = files[b.rank];
      const std::string path = prefix + ".rank" + std::to_string(b.rank) + ".npy";
      if (!rf.f) SIM_TRY(s, open_rank_file(s, path, per_rank[(size_t)b.rank], st.nvar, m.mb, per_block, rf));
      if (fseeko(rf.f, (off_t)(rf.data + (long long)b.index * (long long)per_block), SEEK_SET) != 0 ||
          std::fread(static_cast<char *>(s->h_snap) + per_block * (size_t)q, 1, per_block, rf.f) != per_block)
        return fail(s, APK_ERR_INVALID, "restore: cannot read block " + std::to_string(b.index) + " of " + path);
    }
    SIM_HIP(s, hipMemcpyAsync(s->d_snap, s->h_snap, per_block * (size_t)n, hipMemcpyHostToDevice, hs(s)));
    SIM_TRY(s, apk_restart_unpack(s->ctx, md, first, n, s->d_snap, s->stream));
    SIM_HIP(s, hipStreamSynchronize(hs(s)));
  }
  return APK_OK;
}

}  // namespace

void restart_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  s->rst_outs.clear();
  for (const std::string &blk : pin.BlocksWithPrefix("parthenon/output")) {
    if (blk == "parthenon/output_defaults" || !pin.DoesParameterExist(blk, "file_type")) continue;
    if (pin.GetString(blk, "file_type") != "rst") continue;
    RestartOutputBlock o;
    o.block = blk;
    o.number = blk.substr(std::string("parthenon/output").size());
    if (!pin.DoesParameterExist(blk, "dt")) throw std::runtime_error("<" + blk + "> dt is missing: rst outputs need dt > 0");
    o.dt = pin.GetReal(blk, "dt");
    if (!(o.dt > 0.0)) throw std::runtime_error("<" + blk + "> dt must be positive for rst outputs");
    o.id = pin.GetOrAddString(blk, "id", "out" + o.number);
    if (s->tracers)
      throw std::runtime_error("<" + blk + "> file_type = rst with tracers/enabled = true: restart files do not hold tracers or their lookback histories");
    s->rst_outs.push_back(o);
  }
  // a deck that is a state file (python -m athenapk_amd -r, restart.deck): what the overrides on top of it must not change
  if (pin.DoesParameterExist(kRestartBlock, "format_version")) {
    RestartState st;
    restart_state_load(pin, st);
    const std::string why = mismatch(s, st);
    if (!why.empty()) throw std::runtime_error(why + " (a restart keeps mesh, meshblock, nghost, fluid, nscalars and refinement mode)");
    if (s->tracers) throw std::runtime_error("restart: tracers/enabled = true: restart files do not hold tracers or their lookback histories");
  }
}

int restart_write(apk_sim *s, const std::string &prefix) {
  if (s->tracers) return fail(s, APK_ERR_INVALID, "write_restart: tracers/enabled = true: restart files do not hold tracers or their lookback histories");
  if (s->host_only) return write_state_file(s, prefix);  // (no state: the state file alone, time 0, cycle 0)
  const int rc = apk_sim_write_snapshot(s, prefix.c_str(), "cons", 0);
  // the state file says the dump is complete: rank 0 writes it once every rank has written its array, and no rank writes
  // or reports one if a rank could not -- the ranks reduce their status (the one collective of a dump; a rank that failed
  // takes part in it, so nobody waits for it)
  if (s->have_comm && s->nranks > 1) {
    double ok = rc == APK_OK ? 1.0 : 0.0;
    if (s->comm.allreduce_min(s->comm.user, &ok, 1) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_min failed");
    if (rc == APK_OK && ok != 1.0) return fail(s, APK_ERR_INVALID, "write_restart: another rank could not write its array file " + prefix + ".rank<r>.npy");
  }
  if (rc != APK_OK) return rc;
  if (s->rank != 0) return APK_OK;
  return write_state_file(s, prefix);
}

}  // namespace host
}  // namespace apk

using namespace apk;
using namespace apk::host;

extern "C" {

int apk_sim_restart_outputs(const apk_sim *s, apk_restart_output_info *out, int n, int *size) {
  if (!s || !size || (n > 0 && !out)) return APK_ERR_INVALID;
  *size = (int)s->rst_outs.size();
  for (int q = 0; q < std::min(n, *size); ++q) {
    const RestartOutputBlock &o = s->rst_outs[q];
    std::memset(&out[q], 0, sizeof(out[q]));
    out[q].number = std::atoi(o.number.c_str());
    out[q].dt = o.dt;
    std::snprintf(out[q].id, sizeof(out[q].id), "%s", o.id.c_str());
  }
  return APK_OK;
}

int apk_sim_write_restart(apk_sim *s, const char *prefix) {
  if (!s || !prefix) return APK_ERR_INVALID;
  s->err.clear();
  return restart_write(s, prefix);
}

int apk_sim_restore(apk_sim *s, const char *rst_path) {
  if (!s || s->host_only || !rst_path) return APK_ERR_INVALID;
  s->err.clear();
  if (s->initialized || s->restored)
    return fail(s, APK_ERR_INVALID, "restore: the sim has been initialised, stepped or restored already; restore takes the place of initialize on a new sim");
  if (s->tracers) return fail(s, APK_ERR_INVALID, "restore: tracers/enabled = true: restart files do not hold tracers or their lookback histories");
  if (s->nranks > 1 && !(s->have_comm && s->comm.exchange && s->comm.allreduce_min && s->comm.allreduce_sum))
    return fail(s, APK_ERR_INVALID, "nranks > 1 requires comm ops (apk_sim_create) or the native transport (apk_sim_comm_rccl)");
  const std::string path = rst_path;
  if (path.size() < 5 || path.compare(path.size() - 4, 4, ".rst") != 0) return fail(s, APK_ERR_INVALID, "restore: " + path + " is not a .rst state file");
  const std::string prefix = path.substr(0, path.size() - 4);
  std::string text;
  if (!read_text_file(path, text)) return fail(s, APK_ERR_INVALID, "restore: cannot read " + path);
  RestartState st;
  try {
    ParameterInput rp;
    rp.LoadFromString(text);
    restart_state_load(rp, st);
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, std::string(e.what()) + " (" + path + ")");
  }
  const std::string why = mismatch(s, st);
  if (!why.empty()) return fail(s, APK_ERR_INVALID, why + " (" + path + ")");
  if (st.has_turbulence != (bool)s->fmft) return fail(s, APK_ERR_INVALID, "restore: job/problem_id: the state file and the sim differ in the turbulence driver (" + path + ")");
  // up to here nothing of the sim has changed, and a restore that fails leaves a sim that may still be initialised or
  // restored from another dump: the files are checked first, the turbulence driver takes its state or none of it
  SIM_TRY(s, check_rank_files(s, prefix, st));
  if (s->fmft && !s->fmft->RestoreState(st.accel_hat, st.state_rng, st.state_dist))
    return fail(s, APK_ERR_INVALID, "restore: problem/turbulence/state_rng or state_dist does not parse, or num_modes differs (" + path + ")");
  // (from here on a failure -- a block table that is no balanced forest, a read error, the device -- leaves a sim to discard)
  SIM_TRY(s, sync_ghosts(s));
  if (s->amr && s->amr_adaptive) {
    SIM_TRY(s, install_forest(s, st));
  } else if (s->amr) {  // a static forest is rebuilt from the deck: checked only
    if (st.blocks.size() != s->amr->leaves.size()) return fail(s, APK_ERR_INVALID, "restore: the state file has " + std::to_string(st.blocks.size()) + " blocks, the deck's static refinement makes " + std::to_string(s->amr->leaves.size()));
    for (size_t g = 0; g < st.blocks.size(); ++g) {
      const AmrLeaf &l = s->amr->leaves[g];
      const RestartBlock &b = st.blocks[g];
      if (l.level != b.level || l.lx[0] != b.lx[0] || l.lx[1] != b.lx[1] || l.lx[2] != b.lx[2])
        return fail(s, APK_ERR_INVALID, "restore: block " + std::to_string(g) + " of the state file is not that of the deck's static refinement");
    }
  } else if ((int)st.blocks.size() != s->mesh.nblocks_total) {
    return fail(s, APK_ERR_INVALID, "restore: the state file has " + std::to_string(st.blocks.size()) + " blocks, the mesh " + std::to_string(s->mesh.nblocks_total));
  }
  SIM_TRY(s, unpack_blocks(s, prefix, st));
  s->time = st.time;
  s->ncycle = (int)st.cycle;
  s->dt = st.dt;
  s->pkg.dt_hyp = st.dt_hyp, s->pkg.mindx = st.mindx, s->pkg.c_h = st.c_h, s->pkg.dt_diff = st.dt_diff;
  s->fofc_total = st.fofc_total, s->fofc_fallback_stages = st.fofc_fallback_stages, s->zone_cycles = st.zone_cycles;
  s->amr_refined = st.amr_refined, s->amr_derefined = st.amr_derefined;
  if (s->cluster.enabled) cluster_triggering_reset(s);
  if (st.has_triggering && s->pkg.agn_triggering) {
    auto &q = s->trig_q;
    q.cold_mass = st.trig_reduced[0], q.total_mass = st.trig_reduced[1], q.mass_weighted_density = st.trig_reduced[2];
    q.mass_weighted_velocity = st.trig_reduced[3], q.mass_weighted_cs = st.trig_reduced[4];
    s->trig_rate = st.trig_rate, s->trig_time = st.trig_time, s->trig_dt = st.trig_dt;
    s->agn.accretion_rate = s->trig_rate;  // (as the reduction leaves it: the feedback power follows the rate)
    if (s->agn_opt.configured) s->agn_opt.power = s->agn.power(), s->agn_opt.mass_rate = s->agn.mass_rate();
  }
  for (int n = 0; n < 5; ++n) s->split_totals[n] = st.has_split_totals ? st.split_totals[n] : 0.0;
  s->restored_sched.clear();
  for (const RestartOutput &o : st.outputs) s->restored_sched.push_back({o.number, o.next_time, o.counter});
  // as apk_sim_initialize after the problem generator: complete ghost zones, stored primitives
  SIM_TRY(s, exchange_ghosts(s));
  SIM_TRY(s, fill_derived(s));
  s->prim_stale = false;
  s->stage_dt_pending = false;
  s->dt_hyp_is_global = true;  // (the stored dt_hyp is the minimum over all ranks: estimate_timestep_commit reduced it)
  s->initialized = s->restored = true;
  return APK_OK;
}

}  // extern "C"
