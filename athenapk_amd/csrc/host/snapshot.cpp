// snapshot.cpp -- field snapshot outputs of the standalone driver: the deck's npy output blocks, the chunked transfer of
// the pack kernel's output (apk_output_pack, csrc/kernels_output.hip) through a device and a pinned host staging buffer,
// the files of a dump (formats: snapshot_format.cpp) and the C API of include/apk_host.h.
//
// A dump reads the interior of the current conserved buffer and nothing else: no sync_ghosts, no ConsToPrim pass, no
// collective, no driver flag touched.  The kernel is ordered after the cycle's kernels by the sim's stream; an exchange
// still in flight writes ghost zones (or message buffers) only, which the kernel does not read.
#include "sim_internal.hpp"
#include "snapshot_format.hpp"

#include <algorithm>

namespace apk {
namespace host {

// position of every global block in its rank's file: Morton order within a rank on uniform meshes (mesh.hpp: Build), the
// Z-ordered leaf list itself on refined ones
void snapshot_block_table(const apk_sim *s, std::vector<SnapshotBlock> &blocks) {
  const Mesh &m = s->mesh;
  const int nb = m.nblocks_total;
  blocks.assign(nb, SnapshotBlock());
  std::vector<int> order(nb);
  for (int g = 0; g < nb; ++g) order[g] = g;
  if (!s->amr) {
    std::vector<uint64_t> key(nb);
    for (int g = 0; g < nb; ++g) {
      int bc[3];
      m.Loc(g, bc);
      key[g] = Mesh::Morton(bc[0], bc[1], bc[2]);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  }
  std::vector<int> count(s->nranks, 0);
  for (int p = 0; p < nb; ++p) {
    const int g = order[p];
    SnapshotBlock &b = blocks[g];
    b.gid = g;
    b.rank = m.gid_rank[g];
    b.index = count[b.rank]++;
    if (s->amr) {
      const AmrLeaf &leaf = s->amr->leaves[g];
      b.level = leaf.level;
      for (int d = 0; d < 3; ++d) b.lx[d] = leaf.lx[d];
    } else {
      m.Loc(g, b.lx);
    }
  }
}

namespace {

const char *kConsNames[9] = {"rho", "mom1", "mom2", "mom3", "etot", "B1", "B2", "B3", "psi"};
const char *kPrimNames[9] = {"rho", "vel1", "vel2", "vel3", "pressure", "B1", "B2", "B3", "psi"};

std::string trim(const std::string &s) {
  const auto a = s.find_first_not_of(" \t");
  if (a == std::string::npos) return "";
  return s.substr(a, s.find_last_not_of(" \t") - a + 1);
}

std::string code_name(const apk_sim *s, int code) {
  const int nh = s->pkg.nhydro;
  if (code >= APK_OUT_TEMPERATURE) {
    const char *d[5] = {"temperature", "mach_sonic", "B_mag", "mach_alfven", "plasma_beta"};
    return d[code - APK_OUT_TEMPERATURE];
  }
  const bool prim = code >= APK_OUT_PRIM;
  const int n = prim ? code - APK_OUT_PRIM : code;
  if (n < nh) return std::string(prim ? "prim." : "cons.") + (prim ? kPrimNames[n] : kConsNames[n]);
  return std::string(prim ? "prim.r" : "cons.s") + std::to_string(n - nh);
}

// A `variables` list -> component codes and canonical names.  `where` prefixes every message ("<block> variables: ").
void parse_variables(const apk_sim *s, const std::string &list, const std::string &where, std::vector<int> &codes,
                     std::vector<std::string> &names) {
  codes.clear();
  names.clear();
  const int nh = s->pkg.nhydro, nvar = nh + s->pkg.nscalars;
  const bool mhd = s->pkg.fluid == APK_FLUID_GLMMHD;
  auto add = [&](int code) {
    if (std::find(codes.begin(), codes.end(), code) != codes.end()) return;
    codes.push_back(code);
  };
  size_t pos = 0;
  while (pos <= list.size()) {
    const size_t comma = std::min(list.find(',', pos), list.size());
    const std::string e = trim(list.substr(pos, comma - pos));
    pos = comma + 1;
    if (e.empty()) {
      if (trim(list).empty()) break;
      throw std::runtime_error(where + "empty entry in '" + list + "'");
    }
    if (e == "cons" || e == "prim") {
      for (int n = 0; n < nvar; ++n) add((e == "cons" ? APK_OUT_CONS : APK_OUT_PRIM) + n);
      continue;
    }
    const char *derived[5] = {"temperature", "mach_sonic", "B_mag", "mach_alfven", "plasma_beta"};
    int code = -1;
    for (int q = 0; q < 5; ++q)
      if (e == derived[q]) code = APK_OUT_TEMPERATURE + q;
    if (code >= APK_OUT_B_MAG && !mhd) throw std::runtime_error(where + e + " needs hydro/fluid = glmmhd");
    if (code == APK_OUT_TEMPERATURE && !(s->pkg.units.has_units && s->pkg.units.has_composition))
      throw std::runtime_error(where + "temperature needs a <units> block and hydro/He_mass_fraction");
    if (code < 0 && (e.compare(0, 5, "cons.") == 0 || e.compare(0, 5, "prim.") == 0)) {
      const bool prim = e[0] == 'p';
      const std::string v = e.substr(5);
      for (int n = 0; n < 9; ++n)
        if (v == (prim ? kPrimNames[n] : kConsNames[n])) {
          if (n >= nh) throw std::runtime_error(where + e + " needs hydro/fluid = glmmhd");
          code = (prim ? APK_OUT_PRIM : APK_OUT_CONS) + n;
        }
      if (code < 0 && v.size() > 1 && v[0] == (prim ? 'r' : 's') && v.find_first_not_of("0123456789", 1) == std::string::npos &&
          v.size() < 8) {
        const int n = std::atoi(v.c_str() + 1);
        if (n >= s->pkg.nscalars)
          throw std::runtime_error(where + e + ": scalar index " + std::to_string(n) + " >= hydro/nscalars = " + std::to_string(s->pkg.nscalars));
        code = (prim ? APK_OUT_PRIM : APK_OUT_CONS) + nh + n;
      }
    }
    if (code < 0) throw std::runtime_error(where + "unknown entry '" + e + "'");
    add(code);
  }
  if (codes.empty()) throw std::runtime_error(where + "the list is empty");
  if ((int)codes.size() > APK_OUT_MAX_COMPONENTS)
    throw std::runtime_error(where + "more than " + std::to_string(APK_OUT_MAX_COMPONENTS) + " components");
  for (int c : codes) names.push_back(code_name(s, c));
}

// the C API's form: failures into s->err
int parse_api(apk_sim *s, const char *variables, std::vector<int> &codes, std::vector<std::string> &names) {
  if (!variables) return fail(s, APK_ERR_INVALID, "snapshot: variables is NULL");
  try {
    parse_variables(s, variables, "snapshot variables: ", codes, names);
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

std::string joined(const std::vector<std::string> &names) {
  std::string j;
  for (size_t c = 0; c < names.size(); ++c) j += (c ? "," : "") + names[c];
  return j;
}

int64_t block_cells(const apk_sim *s) { return (int64_t)s->mesh.mb[0] * s->mesh.mb[1] * s->mesh.mb[2]; }

// staging buffers of at least `bytes` (one chunk): grown by free + allocate once the stream has drained
int ensure_staging(apk_sim *s, size_t bytes) {
  if (s->snap_dev_cap < bytes) {
    SIM_HIP(s, hipStreamSynchronize(hs(s)));
    dev_free(s, s->d_snap);
    s->d_snap = nullptr;
    s->snap_dev_cap = 0;
    SIM_TRY(s, dev_alloc(s, "snapshot", bytes, &s->d_snap));
    s->snap_dev_cap = bytes;
  }
  if (s->snap_host_cap < bytes) {
    if (s->h_snap) (void)hipHostFree(s->h_snap);
    s->h_snap = nullptr;
    s->snap_host_cap = 0;
    SIM_HIP(s, hipHostMalloc(&s->h_snap, bytes, hipHostMallocDefault));
    s->snap_host_cap = bytes;
  }
  return APK_OK;
}

// The current state, chunk by chunk: pack kernel -> one device-to-host copy -> sync -> sink(bytes of whole blocks).  One
// pinned buffer: a second one, to overlap the sink of chunk c with the pack and copy of chunk c + 1, is for
// tools/snapshot_cost.py to justify first.
template <class Sink>
int snapshot_chunks(apk_sim *s, const std::vector<int> &codes, bool single, Sink &&sink) {
  if (s->host_only) return fail(s, APK_ERR_INVALID, "snapshot: a host-only sim has no state");
  apk_pack *md = s->mu0();
  if (!md) return fail(s, APK_ERR_INVALID, "snapshot: no pack presents the current state");
  const int nlb = (int)s->mesh.local_gids.size();
  const size_t per_block = (size_t)codes.size() * (size_t)block_cells(s) * (single ? 4 : 8);
  if (nlb == 0 || per_block == 0) return APK_OK;
  const size_t bound = std::max(per_block, std::min(s->snap_staging_bytes, per_block * (size_t)nlb));
  const int chunk_blocks = (int)std::min<size_t>(bound / per_block, (size_t)nlb);
  SIM_TRY(s, ensure_staging(s, per_block * (size_t)chunk_blocks));
  apk_output_desc d{};
  d.ncomp = (int)codes.size();
  d.single = single ? 1 : 0;
  d.gamma = s->pkg.eos.gamma;
  d.mbar_over_kb = s->pkg.units.mbar_over_kb;
  for (size_t c = 0; c < codes.size(); ++c) d.comp[c] = codes[c];
  for (int first = 0; first < nlb; first += chunk_blocks) {
    const int n = std::min(chunk_blocks, nlb - first);
    const size_t bytes = per_block * (size_t)n;
    SIM_TRY(s, apk_output_pack(s->ctx, md, s->pkg.fluid, &s->pkg.eos, &d, first, n, s->d_snap, s->stream));
    SIM_HIP(s, hipMemcpyAsync(s->h_snap, s->d_snap, bytes, hipMemcpyDeviceToHost, hs(s)));
    SIM_HIP(s, hipStreamSynchronize(hs(s)));
    const int rc = sink(s->h_snap, bytes);
    if (rc != APK_OK) return rc;
  }
  return APK_OK;
}

void build_index(const apk_sim *s, const std::vector<std::string> &names, bool single, SnapshotIndex &ix) {
  const Mesh &m = s->mesh;
  ix.time = s->host_only ? 0.0 : s->time;
  ix.cycle = s->host_only ? 0 : s->ncycle;
  ix.dt = s->dt;
  ix.components = names;
  ix.dtype = single ? "<f4" : "<f8";
  ix.fluid = s->pkg.fluid == APK_FLUID_GLMMHD ? "glmmhd" : "euler";
  ix.gamma = s->pkg.eos.gamma;
  ix.nscalars = s->pkg.nscalars;
  for (int d = 0; d < 3; ++d) {
    ix.xmin[d] = s->xmin[d];
    ix.xmax[d] = s->xmax[d];
    ix.mesh_nx[d] = m.nx[d];
    ix.block_nx[d] = m.mb[d];
  }
  ix.nghost = m.ng;
  ix.nranks = s->nranks;
  snapshot_block_table(s, ix.blocks);
}

}  // namespace

int snapshot_staging(apk_sim *s, size_t bytes) { return ensure_staging(s, bytes); }

void snapshot_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  const double mb = pin.GetOrAddReal("apk_amd", "snapshot_staging_mb", 256.0);
  if (!(mb > 0.0)) throw std::runtime_error("apk_amd/snapshot_staging_mb must be positive");
  s->snap_staging_bytes = (size_t)(mb * 1048576.0);
  s->snap_outs.clear();
  for (const std::string &blk : pin.BlocksWithPrefix("parthenon/output")) {
    if (blk == "parthenon/output_defaults" || !pin.DoesParameterExist(blk, "file_type")) continue;
    if (pin.GetString(blk, "file_type") != "npy") continue;  // hst: apk_sim_execute; rst: host/restart.cpp; hdf5: ignored
    SnapshotOutput o;
    o.block = blk;
    const std::string num = blk.substr(std::string("parthenon/output").size());
    o.dt = pin.GetReal(blk, "dt");
    if (!(o.dt > 0.0)) throw std::runtime_error("<" + blk + "> dt must be positive for npy outputs");
    o.single = pin.GetOrAddBoolean(blk, "single_precision_output", false);
    o.id = pin.GetOrAddString(blk, "id", "out" + num);
    parse_variables(s, pin.GetOrAddString(blk, "variables", "cons"), "<" + blk + "> variables: ", o.codes, o.names);
    s->snap_outs.push_back(o);
  }
}

int snapshot_write(apk_sim *s, const std::string &prefix, const std::vector<int> &codes, const std::vector<std::string> &names,
                   bool single) {
  const Mesh &m = s->mesh;
  const std::string path = prefix + ".rank" + std::to_string(s->rank) + ".npy";
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return fail(s, APK_ERR_INVALID, "cannot open " + path);
  const std::string head = npy_header(single ? "<f4" : "<f8", {m.local_gids.size(), codes.size(), (size_t)m.mb[2], (size_t)m.mb[1], (size_t)m.mb[0]});
  bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
  const int rc = snapshot_chunks(s, codes, single, [&](const void *p, size_t bytes) {
    ok = ok && std::fwrite(p, 1, bytes, f) == bytes;
    return APK_OK;
  });
  ok = (std::fclose(f) == 0) && ok;
  if (rc != APK_OK) return rc;
  if (!ok) return fail(s, APK_ERR_INVALID, "cannot write " + path);
  if (s->rank != 0) return APK_OK;
  SnapshotIndex ix;
  build_index(s, names, single, ix);
  if (!write_text_file(prefix + ".json", snapshot_index_json(ix))) return fail(s, APK_ERR_INVALID, "cannot write " + prefix + ".json");
  return APK_OK;
}

void snapshot_free(apk_sim *s) {
  dev_free(s, s->d_snap);
  s->d_snap = nullptr;
  if (s->h_snap) (void)hipHostFree(s->h_snap);
  s->h_snap = nullptr;
  s->snap_dev_cap = s->snap_host_cap = 0;
}

}  // namespace host
}  // namespace apk

using namespace apk;
using namespace apk::host;

extern "C" {

int apk_sim_snapshot_outputs(const apk_sim *s, apk_snapshot_output_info *out, int n, int *size) {
  if (!s || !size || (n > 0 && !out)) return APK_ERR_INVALID;
  *size = (int)s->snap_outs.size();
  for (int q = 0; q < std::min(n, *size); ++q) {
    const SnapshotOutput &o = s->snap_outs[q];
    std::memset(&out[q], 0, sizeof(out[q]));
    out[q].number = std::atoi(o.block.c_str() + std::string("parthenon/output").size());
    out[q].single = o.single ? 1 : 0;
    out[q].ncomp = (int)o.codes.size();
    out[q].dt = o.dt;
    std::snprintf(out[q].id, sizeof(out[q].id), "%s", o.id.c_str());
    std::snprintf(out[q].components, sizeof(out[q].components), "%s", joined(o.names).c_str());
  }
  return APK_OK;
}

int apk_sim_snapshot_shape(apk_sim *s, const char *variables, int single, int *nblocks, int *ncomp, int nx[3], int *itemsize,
                           char *names, size_t names_len) {
  if (!s) return APK_ERR_INVALID;
  std::vector<int> codes;
  std::vector<std::string> nm;
  SIM_TRY(s, parse_api(s, variables, codes, nm));
  if (nblocks) *nblocks = (int)s->mesh.local_gids.size();
  if (ncomp) *ncomp = (int)codes.size();
  if (nx)
    for (int d = 0; d < 3; ++d) nx[d] = s->mesh.mb[d];
  if (itemsize) *itemsize = single ? 4 : 8;
  if (names && names_len) std::snprintf(names, names_len, "%s", joined(nm).c_str());
  return APK_OK;
}

int apk_sim_snapshot_read(apk_sim *s, const char *variables, int single, void *out, size_t out_bytes) {
  if (!s || !out) return APK_ERR_INVALID;
  std::vector<int> codes;
  std::vector<std::string> nm;
  SIM_TRY(s, parse_api(s, variables, codes, nm));
  const size_t need = s->mesh.local_gids.size() * codes.size() * (size_t)block_cells(s) * (single ? 4 : 8);
  if (out_bytes != need) return fail(s, APK_ERR_INVALID, "apk_sim_snapshot_read: out_bytes is " + std::to_string(out_bytes) + ", the snapshot has " + std::to_string(need));
  char *dst = static_cast<char *>(out);
  return snapshot_chunks(s, codes, single != 0, [&](const void *p, size_t bytes) {
    std::memcpy(dst, p, bytes);
    dst += bytes;
    return APK_OK;
  });
}

int apk_sim_write_snapshot(apk_sim *s, const char *prefix, const char *variables, int single) {
  if (!s || !prefix) return APK_ERR_INVALID;
  std::vector<int> codes;
  std::vector<std::string> nm;
  SIM_TRY(s, parse_api(s, variables, codes, nm));
  return snapshot_write(s, prefix, codes, nm, single != 0);
}

int apk_sim_write_snapshot_index(apk_sim *s, const char *path, const char *variables, int single) {
  if (!s || !path) return APK_ERR_INVALID;
  std::vector<int> codes;
  std::vector<std::string> nm;
  SIM_TRY(s, parse_api(s, variables, codes, nm));
  SnapshotIndex ix;
  build_index(s, nm, single != 0, ix);
  if (!write_text_file(path, snapshot_index_json(ix))) return fail(s, APK_ERR_INVALID, std::string("cannot write ") + path);
  return APK_OK;
}

}  // extern "C"
