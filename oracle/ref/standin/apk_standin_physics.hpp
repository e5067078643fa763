// apk_standin_physics.hpp -- the further stand-in names that the reference's physics headers touch: src/units.hpp,
// src/pgen/cluster/{cluster_gravity,entropy_profiles,jet_coords,magnetic_tower,cluster_utils}.hpp,
// src/hydro/srcterms/tabular_cooling.hpp and src/hydro/diffusion/diffusion.hpp (oracle/ref/ref_physics.cpp).
//
// TEST INFRASTRUCTURE.  Written for this project: it is not Parthenon and holds no line of it or of the reference.
// It adds to apk_standin.hpp and changes none of its names' meaning for ref_vectors.cpp, which never includes it:
//   - ParameterInput: a map "block/key" -> string with GetOrAddReal / GetOrAddBoolean / GetOrAddString (a key that is
//     absent is ADDED with the default, as the name says) and Set(), which the driver fills from its command line
//   - StateDescriptor: AddParam / Param over std::any, AddField that only records the name
//   - Metadata (three flags and a shape), IndexRange, ParArray1D (an owning handle with operator())
//   - Kokkos::abort
//   - PARTHENON_FAIL for a C string or a std::stringstream (still a braced block), PARTHENON_REQUIRE_THROWS, which
//     throws std::runtime_error and, as the reference writes it once without one, carries its own semicolon
#ifndef APK_STANDIN_PHYSICS_HPP_
#define APK_STANDIN_PHYSICS_HPP_

#include "apk_standin.hpp"

#include <any>
#include <sstream>
#include <stdexcept>

namespace apk_standin {
[[noreturn]] inline void fail(const char *file, const int line, const char *msg) {
  std::fprintf(stderr, "PARTHENON_FAIL %s:%d: %s\n", file, line, msg);
  std::abort();
}
[[noreturn]] inline void fail(const char *file, const int line, const std::stringstream &msg) {
  fail(file, line, msg.str().c_str());
}
} // namespace apk_standin

#undef PARTHENON_FAIL
#define PARTHENON_FAIL(msg)                                                                                       \
  { apk_standin::fail(__FILE__, __LINE__, msg); }
#define PARTHENON_REQUIRE_THROWS(cond, msg)                                                                       \
  if (!(cond)) throw std::runtime_error(msg);

namespace Kokkos {
[[noreturn]] inline void abort(const char *msg) {
  std::fprintf(stderr, "Kokkos::abort: %s\n", msg);
  std::abort();
}
} // namespace Kokkos

namespace parthenon {

class ParameterInput {
 public:
  void Set(const std::string &block, const std::string &name, const std::string &value) { kv_[block + "/" + name] = value; }
  bool DoesParameterExist(const std::string &block, const std::string &name) const { return kv_.count(block + "/" + name) != 0; }
  Real GetOrAddReal(const std::string &block, const std::string &name, const Real def) {
    const std::string *s = find(block, name);
    if (s != nullptr) return std::strtod(s->c_str(), nullptr);
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", def);
    Set(block, name, buf);
    return def;
  }
  bool GetOrAddBoolean(const std::string &block, const std::string &name, const bool def) {
    const std::string *s = find(block, name);
    if (s != nullptr) return *s == "true" || *s == "1";
    Set(block, name, def ? "true" : "false");
    return def;
  }
  std::string GetOrAddString(const std::string &block, const std::string &name, const std::string &def) {
    const std::string *s = find(block, name);
    if (s != nullptr) return *s;
    Set(block, name, def);
    return def;
  }
  const std::map<std::string, std::string> &all() const { return kv_; }

 private:
  const std::string *find(const std::string &block, const std::string &name) const {
    const auto it = kv_.find(block + "/" + name);
    return it == kv_.end() ? nullptr : &it->second;
  }
  std::map<std::string, std::string> kv_;
};

struct Metadata {
  enum Flag { Cell, Derived, OneCopy };
  Metadata() = default;
  Metadata(const std::vector<Flag> &f, const std::vector<int> &s) : flags(f), shape(s) {}
  std::vector<Flag> flags;
  std::vector<int> shape;
};

struct IndexRange {
  int s = 0, e = 0;
};

class StateDescriptor {
 public:
  template <class T>
  void AddParam(const std::string &name, const T &value, const bool = false) {
    params_.insert_or_assign(name, std::any(value));
  }
  template <class T>
  const T &Param(const std::string &name) const {
    return *std::any_cast<T>(&params_.at(name));
  }
  void AddField(const std::string &name, const Metadata &) { fields_.push_back(name); }

 private:
  std::map<std::string, std::any> params_;
  std::vector<std::string> fields_;
};

template <class T>
class ParArray1D {
 public:
  ParArray1D() = default;
  // one zero element more than asked for: CoolingTableObj::DeDt reads log_lambdas_(n_temp_) when log T sits exactly on
  // the last node (and multiplies what it read by an exact zero); here that read stays inside the allocation
  ParArray1D(const std::string &, const std::size_t n) : store_(std::make_shared<std::vector<T>>(n + 1)) {}
  T &operator()(const std::size_t i) const { return (*store_)[i]; }
  std::size_t size() const { return store_ ? store_->size() - 1 : 0; }

 private:
  std::shared_ptr<std::vector<T>> store_;
};

namespace package {
namespace prelude {
using ::parthenon::ParArray1D;
} // namespace prelude
} // namespace package
} // namespace parthenon

#endif // APK_STANDIN_PHYSICS_HPP_
