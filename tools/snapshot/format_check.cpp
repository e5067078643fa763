// format_check.cpp -- stand-alone host program for the two file formats of a field snapshot
// (csrc/host/snapshot_format.cpp): writes a small array under an N-dimensional NumPy header and a small JSON index
// through those functions, reads both back and checks them byte by byte -- the header's magic, version, length field,
// 64-byte alignment and dict for one to five dimensions, the data behind it, the index's doubles through %.17g (a value
// that needs all 17 digits, the largest double, a non-finite one) and its block table.  No GPU, no Python; meant to be
// compiled with sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/snapshot/format_check.cpp athenapk_amd/csrc/host/snapshot_format.cpp -o /tmp/format_check && /tmp/format_check /tmp
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../athenapk_amd/csrc/host/snapshot_format.hpp"

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

// the number behind "key": in the JSON text
double number_after(const std::string &json, const std::string &key) {
  const size_t at = json.find("\"" + key + "\": ");
  if (at == std::string::npos) return -1.0;
  return std::strtod(json.c_str() + at + key.size() + 4, nullptr);
}
}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  int ok = 1;

  // ---- the header, one to five dimensions
  const std::vector<std::vector<size_t>> shapes = {{7}, {3, 5}, {2, 3, 4}, {1, 2, 3, 4}, {2, 3, 4, 2, 6}, {123456, 48, 128, 128, 128}};
  const char *dicts[] = {"(7,), }", "(3, 5), }", "(2, 3, 4), }", "(1, 2, 3, 4), }", "(2, 3, 4, 2, 6), }", "(123456, 48, 128, 128, 128), }"};
  for (size_t q = 0; q < shapes.size(); ++q) {
    const std::string h = npy_header(q % 2 ? "<f4" : "<f8", shapes[q]);
    ok &= check(h.size() % 64 == 0 && h.size() >= 64, "header length is a multiple of 64");
    ok &= check(std::memcmp(h.data(), "\x93NUMPY\x01\x00", 8) == 0, "magic and version 1.0");
    const size_t len = (unsigned char)h[8] | ((size_t)(unsigned char)h[9] << 8);
    ok &= check(len + 10 == h.size(), "little-endian length field");
    ok &= check(h.back() == '\n', "the dict ends with a newline");
    const std::string want = std::string("{'descr': '") + (q % 2 ? "<f4" : "<f8") + "', 'fortran_order': False, 'shape': " + dicts[q];
    ok &= check(h.compare(10, want.size(), want) == 0, "the dict");
    ok &= check(h.find_first_not_of(' ', 10 + want.size()) == h.size() - 1, "space padding");
  }

  // ---- an array behind it
  const std::vector<size_t> shape = {2, 3, 4, 2, 6};
  std::vector<float> data(2 * 3 * 4 * 2 * 6);
  for (size_t q = 0; q < data.size(); ++q) data[q] = 0.25f * (float)q - 7.0f;
  const std::string npy = dir + "/format_check.rank0.npy";
  {
    const std::string h = npy_header("<f4", shape);
    FILE *f = std::fopen(npy.c_str(), "wb");
    ok &= check(f != nullptr, "array file opens");
    if (f) {
      ok &= check(std::fwrite(h.data(), 1, h.size(), f) == h.size(), "header written");
      ok &= check(std::fwrite(data.data(), sizeof(float), data.size(), f) == data.size(), "data written");
      std::fclose(f);
    }
    const std::string back = slurp(npy);
    ok &= check(back.size() == h.size() + data.size() * sizeof(float), "array file size");
    ok &= check(back.size() >= h.size() && std::memcmp(back.data() + h.size(), data.data(), data.size() * sizeof(float)) == 0, "array bytes");
  }

  // ---- the index
  SnapshotIndex ix;
  ix.time = 0.1 + 0.2;  // 0.30000000000000004: needs all 17 digits
  ix.dt = DBL_MAX;
  ix.cycle = 123456789012LL;
  ix.components = {"cons.rho", "prim.pressure", "plasma_beta"};
  ix.dtype = "<f4";
  ix.fluid = "glmmhd";
  ix.gamma = 5.0 / 3.0;
  ix.nscalars = 2;
  const double lo[3] = {-1.0 / 3.0, 0.0, -0.5}, hi[3] = {2.0 / 3.0, 1e-300, 0.5};
  const int mesh[3] = {24, 4, 8}, blk[3] = {6, 2, 4};
  for (int d = 0; d < 3; ++d) ix.xmin[d] = lo[d], ix.xmax[d] = hi[d], ix.mesh_nx[d] = mesh[d], ix.block_nx[d] = blk[d];
  ix.nghost = 2;
  ix.nranks = 2;
  for (int g = 0; g < 9; ++g) {
    SnapshotBlock b;
    b.gid = g, b.level = g ? 1 : 0, b.lx[0] = g % 2, b.lx[1] = (g / 2) % 2, b.lx[2] = g / 4, b.rank = g % 2, b.index = g / 2;
    ix.blocks.push_back(b);
  }
  const std::string json = snapshot_index_json(ix);
  const std::string jpath = dir + "/format_check.json";
  ok &= check(write_text_file(jpath, json), "index written");
  ok &= check(slurp(jpath) == json, "index read back");
  ok &= check(number_after(json, "time") == ix.time, "time round-trips");
  ok &= check(number_after(json, "dt") == DBL_MAX, "the largest double round-trips");
  ok &= check(number_after(json, "gamma") == ix.gamma, "gamma round-trips");
  ok &= check(json.find("\"cycle\": 123456789012,") != std::string::npos, "cycle");
  ok &= check(json.find("\"components\": [\"cons.rho\", \"prim.pressure\", \"plasma_beta\"]") != std::string::npos, "components");
  ok &= check(json.find("{\"gid\": 8, \"level\": 1, \"lx1\": 0, \"lx2\": 0, \"lx3\": 2, \"rank\": 0, \"index\": 4}") != std::string::npos, "last block");
  ok &= check(json.find("\"mesh_nx\": [24, 4, 8]") != std::string::npos && json.find("\"block_nx\": [6, 2, 4]") != std::string::npos, "extents");
  size_t braces = 0;
  for (char c : json) braces += c == '{', braces -= c == '}';
  ok &= check(braces == 0, "balanced braces");
  // what JSON cannot hold, and an empty table
  SnapshotIndex empty;
  empty.time = std::strtod("nan", nullptr);
  const std::string ej = snapshot_index_json(empty);
  ok &= check(ej.find("\"time\": null") != std::string::npos && ej.find("\"blocks\": []") != std::string::npos, "non-finite and empty");
  ok &= check(!write_text_file(dir + "/no/such/directory/x.json", json), "an unwritable path is reported");

  std::remove(npy.c_str());
  std::remove(jpath.c_str());
  std::printf(ok ? "format_check: ok\n" : "format_check: FAILED\n");
  return ok ? 0 : 1;
}
