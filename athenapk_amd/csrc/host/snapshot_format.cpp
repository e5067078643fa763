// snapshot_format.cpp -- NumPy header and JSON index of a field snapshot (snapshot_format.hpp).  No HIP, no driver state.
#include "snapshot_format.hpp"

#include <cmath>
#include <cstdio>

namespace apk {

std::string npy_header(const std::string &descr, const std::vector<size_t> &shape) {
  std::string dict = "{'descr': '" + descr + "', 'fortran_order': False, 'shape': (";
  for (size_t d = 0; d < shape.size(); ++d) dict += std::to_string(shape[d]) + (shape.size() == 1 || d + 1 < shape.size() ? "," : "") +
                                                    (d + 1 < shape.size() ? " " : "");
  dict += "), }";
  while ((10 + dict.size() + 1) % 64 != 0) dict += ' ';
  dict += '\n';
  std::string h("\x93NUMPY", 6);
  h += (char)1;
  h += (char)0;
  h += (char)(dict.size() & 0xff);
  h += (char)((dict.size() >> 8) & 0xff);
  return h + dict;
}

namespace {
std::string num(double v) {
  if (!std::isfinite(v)) return "null";
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}
std::string quoted(const std::string &s) {
  std::string q = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') q += '\\';
    q += c;
  }
  return q + "\"";
}
std::string triple(const double v[3]) { return "[" + num(v[0]) + ", " + num(v[1]) + ", " + num(v[2]) + "]"; }
std::string triple(const int v[3]) { return "[" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + ", " + std::to_string(v[2]) + "]"; }
}  // namespace

std::string snapshot_index_json(const SnapshotIndex &ix) {
  std::string j = "{\n";
  j += "  \"time\": " + num(ix.time) + ",\n";
  j += "  \"cycle\": " + std::to_string(ix.cycle) + ",\n";
  j += "  \"dt\": " + num(ix.dt) + ",\n";
  j += "  \"components\": [";
  for (size_t c = 0; c < ix.components.size(); ++c) j += (c ? ", " : "") + quoted(ix.components[c]);
  j += "],\n";
  j += "  \"dtype\": " + quoted(ix.dtype) + ",\n";
  j += "  \"fluid\": " + quoted(ix.fluid) + ",\n";
  j += "  \"gamma\": " + num(ix.gamma) + ",\n";
  j += "  \"nscalars\": " + std::to_string(ix.nscalars) + ",\n";
  j += "  \"xmin\": " + triple(ix.xmin) + ",\n";
  j += "  \"xmax\": " + triple(ix.xmax) + ",\n";
  j += "  \"mesh_nx\": " + triple(ix.mesh_nx) + ",\n";
  j += "  \"block_nx\": " + triple(ix.block_nx) + ",\n";
  j += "  \"nghost\": " + std::to_string(ix.nghost) + ",\n";
  j += "  \"nranks\": " + std::to_string(ix.nranks) + ",\n";
  j += "  \"blocks\": [";
  for (size_t b = 0; b < ix.blocks.size(); ++b) {
    const SnapshotBlock &k = ix.blocks[b];
    j += std::string(b ? ",\n    " : "\n    ") + "{\"gid\": " + std::to_string(k.gid) + ", \"level\": " + std::to_string(k.level) +
         ", \"lx1\": " + std::to_string(k.lx[0]) + ", \"lx2\": " + std::to_string(k.lx[1]) + ", \"lx3\": " + std::to_string(k.lx[2]) +
         ", \"rank\": " + std::to_string(k.rank) + ", \"index\": " + std::to_string(k.index) + "}";
  }
  j += ix.blocks.empty() ? "]\n" : "\n  ]\n";
  j += "}\n";
  return j;
}

bool write_text_file(const std::string &path, const std::string &text) {
  FILE *f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
  return std::fclose(f) == 0 && ok;
}

}  // namespace apk
