// snapshot_format.hpp -- the two file formats of a field snapshot (host/snapshot.cpp), plain C++ without HIP: the NumPy
// format 1.0 header of an N-dimensional array and the JSON index.  tools/snapshot/format_check.cpp builds against this
// header and snapshot_format.cpp alone.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

namespace apk {

// The header of a .npy file, format 1.0 (magic, version, little-endian length, the dict, padded with spaces and closed
// with '\n' so that the data begin on a multiple of 64 bytes): descr e.g. "<f8", C order.  The data follow as they lie in
// memory.
std::string npy_header(const std::string &descr, const std::vector<size_t> &shape);

struct SnapshotBlock {
  int gid = 0, level = 0;
  int lx[3] = {0, 0, 0};  // logical location at its level
  int rank = 0, index = 0;  // the rank whose file holds it, and its position there
};

struct SnapshotIndex {
  double time = 0.0, dt = 0.0;
  long long cycle = 0;
  std::vector<std::string> components;
  std::string dtype;  // "<f8" | "<f4"
  std::string fluid;  // "euler" | "glmmhd"
  double gamma = 0.0;
  int nscalars = 0;
  double xmin[3] = {0, 0, 0}, xmax[3] = {0, 0, 0};
  int mesh_nx[3] = {1, 1, 1}, block_nx[3] = {1, 1, 1};
  int nghost = 0, nranks = 1;
  std::vector<SnapshotBlock> blocks;  // one per global block, gid order
};

// the index as JSON text; doubles as %.17g (non-finite ones, which JSON cannot hold, as null)
std::string snapshot_index_json(const SnapshotIndex &ix);
// text -> file; false if it could not be written in full
bool write_text_file(const std::string &path, const std::string &text);

}  // namespace apk
