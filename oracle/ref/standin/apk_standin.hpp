// apk_standin.hpp -- stand-in for the Kokkos/Parthenon names that the reference's header-only arithmetic
// (src/recon/*_simple.hpp, src/hydro/rsolvers/*.hpp, src/eos/adiabatic_*.hpp, src/hydro/hydro.hpp) touches.
//
// TEST INFRASTRUCTURE.  Written for this project from the list in SURVEY.md 8(c): it is not Parthenon and holds
// no line of it or of the reference.  Everything is serial, host-only and as small as those headers allow:
//   - Real, X1DIR..X3DIR, team_mbr_t, par_for_inner (INCLUSIVE bounds)
//   - ScratchPad2D, VariablePack, VariableFluxPack, ParArray4D: small owning arrays with operator() / flux()
//   - Coords::Dxc<D>
//   - empty declarations of the framework types that hydro.hpp / eos.hpp / main.hpp only name
//   - the macros.  SQR, SIGN and TINY_NUMBER are Parthenon's; Parthenon is not vendored in the reference tree, so
//     their definitions are RECALLED, not read: SQR(x) = x*x, SIGN(0) = +1, TINY_NUMBER = 1e-20.
//     PARTHENON_REQUIRE / PARTHENON_FAIL abort; PARTHENON_FAIL is a braced block because the reference writes it
//     without a trailing semicolon.
#ifndef APK_STANDIN_HPP_
#define APK_STANDIN_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#define KOKKOS_INLINE_FUNCTION inline
#define KOKKOS_FORCEINLINE_FUNCTION inline
#define KOKKOS_LAMBDA [=]

#define SQR(x) ((x) * (x))
#define SIGN(x) (((x) < 0.0) ? -1.0 : 1.0)
#define TINY_NUMBER 1.0e-20

#define PARTHENON_FAIL(msg)                                                                                       \
  {                                                                                                               \
    std::fprintf(stderr, "PARTHENON_FAIL %s:%d: %s\n", __FILE__, __LINE__, msg);                                  \
    std::abort();                                                                                                 \
  }
#define PARTHENON_REQUIRE(cond, msg)                                                                              \
  if (!(cond)) PARTHENON_FAIL(msg)

namespace parthenon {

using Real = double;
constexpr int X1DIR = 1, X2DIR = 2, X3DIR = 3;

struct team_mbr_t {};

template <class F>
inline void par_for_inner(const team_mbr_t &, const int il, const int iu, const F &f) {
  for (int i = il; i <= iu; ++i) f(i);
}

struct Coords {
  Real dx[3] = {1.0, 1.0, 1.0};
  template <int D>
  Real Dxc(const int, const int, const int) const {
    return dx[D - 1];
  }
};

// Views are handles: operator() of a const view yields a writable element, as with the framework's arrays.
template <class T>
class ScratchPad2D {
 public:
  ScratchPad2D() = default;
  ScratchPad2D(const int n, const int m) : m_(m), store_(std::make_shared<std::vector<T>>(std::size_t(n) * m)) {
    p_ = store_->data();
  }
  static std::size_t shmem_size(const int n, const int m) { return std::size_t(n) * m * sizeof(T); }
  T &operator()(const int n, const int i) const { return p_[std::size_t(n) * m_ + i]; }
  T *data() const { return p_; }
  void assign_data(T *p) { p_ = p; }

 private:
  int m_ = 0;
  std::shared_ptr<std::vector<T>> store_;
  T *p_ = nullptr;
};

template <class T>
class ParArray4D {
 public:
  ParArray4D() = default;
  ParArray4D(const int nv, const int nk, const int nj, const int ni)
      : nv_(nv), nk_(nk), nj_(nj), ni_(ni), store_(std::make_shared<std::vector<T>>(std::size_t(nv) * nk * nj * ni)) {}
  T &operator()(const int n, const int k, const int j, const int i) const {
    return (*store_)[((std::size_t(n) * nk_ + k) * nj_ + j) * ni_ + i];
  }
  int GetDim(const int d) const { return d == 4 ? nv_ : d == 3 ? nk_ : d == 2 ? nj_ : d == 1 ? ni_ : 1; }
  T *data() const { return store_->data(); }
  std::size_t size() const { return store_->size(); }

 private:
  int nv_ = 0, nk_ = 0, nj_ = 0, ni_ = 0;
  std::shared_ptr<std::vector<T>> store_;
};

template <class T>
class VariablePack : public ParArray4D<T> {
 public:
  VariablePack() = default;
  VariablePack(const int nv, const int nk, const int nj, const int ni) : ParArray4D<T>(nv, nk, nj, ni) {}
  const Coords &GetCoords() const { return coords; }
  Coords coords;
};

template <class T>
class VariableFluxPack : public VariablePack<T> {
 public:
  VariableFluxPack() = default;
  VariableFluxPack(const int nv, const int nk, const int nj, const int ni) : VariablePack<T>(nv, nk, nj, ni) {
    for (auto &f : f_) f = ParArray4D<T>(nv, nk, nj, ni);
  }
  T &flux(const int dir, const int n, const int k, const int j, const int i) const { return f_[dir - 1](n, k, j, i); }

 private:
  ParArray4D<T> f_[3];
};

// names that the reference headers mention in declarations only
class ParameterInput;
class StateDescriptor;
class Mesh;
class MeshBlock;
struct SimTime;
template <class T>
class MeshData;
template <class T>
class MeshBlockData;
template <class T>
class MeshBlockVarPack;
using Packages_t = std::map<std::string, std::shared_ptr<StateDescriptor>>;
enum class TaskStatus { fail, complete, incomplete, iterate };
enum class AmrTag : int { derefine = -1, same = 0, refine = 1 };

namespace package {
namespace prelude {
using ::parthenon::AmrTag;
using ::parthenon::Mesh;
using ::parthenon::MeshBlock;
using ::parthenon::MeshBlockData;
using ::parthenon::MeshBlockVarPack;
using ::parthenon::MeshData;
using ::parthenon::Packages_t;
using ::parthenon::ParameterInput;
using ::parthenon::ParArray4D;
using ::parthenon::Real;
using ::parthenon::ScratchPad2D;
using ::parthenon::StateDescriptor;
using ::parthenon::TaskStatus;
using ::parthenon::VariableFluxPack;
using ::parthenon::VariablePack;
using ::parthenon::X1DIR;
using ::parthenon::X2DIR;
using ::parthenon::X3DIR;
} // namespace prelude
} // namespace package
} // namespace parthenon

#endif // APK_STANDIN_HPP_
