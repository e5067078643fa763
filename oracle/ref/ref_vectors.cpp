// ref_vectors.cpp -- runs the REFERENCE's own header-only arithmetic on raw fp64 vectors.
//
// TEST INFRASTRUCTURE.  This file is this project's; it holds no reference code.  It includes the reference's
// headers by include path only (the tree is given to the Makefile as APK_REFERENCE_SRC), against the stand-in
// names of standin/apk_standin.hpp, and the binary it builds into oracle/_ref/ is never committed.
//
// A filter: little-endian fp64 from stdin, little-endian fp64 to stdout, arrays row-major.
//   recon   <method> <n> <dx> <positivity>        in q[n][5] (i-2..i+2)          out ql_ip1[n], qr_i[n]
//   riemann <fluid> <solver> <n> <ivx> <gamma> <c_h>
//                                                  in wl[n][nv], wr[n][nv]        out flux[n][nv]
//   c2p     <fluid> <n> <gamma> <pfloor> <dfloor> <efloor> <vceil> <eceil> <nscalars>
//                                                  in u[n][nv+ns]                 out u_after[n][nv+ns], w[n][nv+ns]
//   speeds  <n> <gamma>                            in (d,p,bx,by,bz)[n]           out SoundSpeed[n], FastMagnetosonicSpeed[n]
//   pencil  <fluid> <recon> <solver> <dir> <n> <gamma> <c_h> <dx>
//                                                  in w[n][nv] along <dir>        out flux[n][nv]; face i is the lower
//                                                  face of cell i; faces the stencil does not reach are 0
// States are in natural variable order (rho, v1, v2, v3, p[, B1, B2, B3, psi]); fluxes in natural conserved order.
// weno3 and limo3 take the cell width dx (weno3 squares it, as its wrapper does).
//
// NEVER feed inputs on which PARTHENON_REQUIRE fires (non-positive density or pressure with the matching floor
// off in c2p): they abort, as in the reference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hydro/hydro.hpp" // first: brings Real, the enums and the prelude names into scope for the headers below
#include "eos/adiabatic_glmmhd.hpp"
#include "eos/adiabatic_hydro.hpp"
#include "hydro/rsolvers/rsolvers.hpp"
#include "recon/dc_simple.hpp"
#include "recon/limo3_simple.hpp"
#include "recon/plm_simple.hpp"
#include "recon/ppm_simple.hpp"
#include "recon/weno3_simple.hpp"
#include "recon/wenoz_simple.hpp"

// the block-level ConservedToPrimitive(MeshData*) live in .cpp files that need the framework; they are never called
void AdiabaticHydroEOS::ConservedToPrimitive(MeshData<Real> *) const {}
void AdiabaticGLMMHDEOS::ConservedToPrimitive(MeshData<Real> *) const {}

namespace {

[[noreturn]] void die(const char *msg) {
  std::fprintf(stderr, "ref_vectors: %s\n", msg);
  std::exit(2);
}

std::vector<double> read_doubles(const std::size_t n) {
  std::vector<double> v(n);
  if (n && std::fread(v.data(), sizeof(double), n, stdin) != n) die("short read on stdin");
  return v;
}

void write_doubles(const std::vector<double> &v) {
  if (!v.empty() && std::fwrite(v.data(), sizeof(double), v.size(), stdout) != v.size()) die("short write");
}

Reconstruction recon_of(const std::string &s) {
  if (s == "dc") return Reconstruction::dc;
  if (s == "plm") return Reconstruction::plm;
  if (s == "ppm") return Reconstruction::ppm;
  if (s == "wenoz") return Reconstruction::wenoz;
  if (s == "weno3") return Reconstruction::weno3;
  if (s == "limo3") return Reconstruction::limo3;
  die("unknown reconstruction");
}

RiemannSolver solver_of(const std::string &s) {
  if (s == "none") return RiemannSolver::none;
  if (s == "hlle") return RiemannSolver::hlle;
  if (s == "llf") return RiemannSolver::llf;
  if (s == "hllc") return RiemannSolver::hllc;
  if (s == "hlld") return RiemannSolver::hlld;
  die("unknown Riemann solver");
}

Fluid fluid_of(const std::string &s) {
  if (s == "euler") return Fluid::euler;
  if (s == "glmmhd") return Fluid::glmmhd;
  die("unknown fluid");
}

template <Fluid F>
using eos_t = typename std::conditional<F == Fluid::euler, AdiabaticHydroEOS, AdiabaticGLMMHDEOS>::type;

template <Fluid F>
eos_t<F> plain_eos(const double gamma) {
  const double inf = std::numeric_limits<double>::infinity();
  return eos_t<F>(-1.0, -1.0, -1.0, inf, inf, gamma);
}

// ---- recon: the pointwise functions --------------------------------------------------------------------------
void cmd_recon(const Reconstruction rc, const long n, const double dx, const bool positivity) {
  const auto q = read_doubles(5 * n);
  std::vector<double> out(2 * n);
  for (long s = 0; s < n; ++s) {
    const double *p = &q[5 * s];
    double &ql = out[s], &qr = out[n + s];
    switch (rc) {
    case Reconstruction::dc: ql = qr = p[2]; break;
    case Reconstruction::plm: PLM(p[1], p[2], p[3], ql, qr); break;
    case Reconstruction::ppm: PPM(p[0], p[1], p[2], p[3], p[4], ql, qr); break;
    case Reconstruction::wenoz: WENOZ(p[0], p[1], p[2], p[3], p[4], ql, qr); break;
    case Reconstruction::weno3: {
      double dx2 = dx;
      dx2 = dx2 * dx2;
      WENO3(p[1], p[2], p[3], ql, qr, dx2);
      break;
    }
    case Reconstruction::limo3: LimO3(p[1], p[2], p[3], ql, qr, dx, positivity); break;
    default: die("recon");
    }
  }
  write_doubles(out);
}

// ---- riemann -------------------------------------------------------------------------------------------------
template <Fluid F, RiemannSolver S>
void riemann_pads(const long n, const int ivx, const double gamma, const double c_h) {
  const int nv = int(Hydro::GetNVars<F>());
  const auto in = read_doubles(2 * std::size_t(nv) * n);
  parthenon::ScratchPad2D<Real> wl(nv, int(n)), wr(nv, int(n));
  parthenon::VariableFluxPack<Real> cons(nv, 1, 1, int(n));
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < nv; ++v) {
      wl(v, int(s)) = in[s * nv + v];
      wr(v, int(s)) = in[(n + s) * nv + v];
    }
  const auto eos = plain_eos<F>(gamma);
  Riemann<F, S>::Solve(parthenon::team_mbr_t(), 0, 0, 0, int(n) - 1, ivx, wl, wr, cons, eos, c_h);
  std::vector<double> out(std::size_t(nv) * n);
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < nv; ++v) out[s * nv + v] = cons.flux(ivx, v, 0, 0, int(s));
  write_doubles(out);
}

// the LLF solvers read a donor-cell pair straight from the primitive array: cells 2s, 2s+1 along ivx hold (wl, wr)
template <Fluid F>
void riemann_llf(const long n, const int ivx, const double gamma, const double c_h) {
  const int nv = int(Hydro::GetNVars<F>());
  const auto in = read_doubles(2 * std::size_t(nv) * n);
  int dim[3] = {1, 1, 1}; // nk, nj, ni
  dim[3 - ivx] = int(2 * n);
  parthenon::VariablePack<Real> prim(nv, dim[0], dim[1], dim[2]);
  parthenon::VariableFluxPack<Real> cons(nv, dim[0], dim[1], dim[2]);
  auto at = [&](const long c, int &k, int &j, int &i) {
    k = j = i = 0;
    (ivx == 1 ? i : ivx == 2 ? j : k) = int(c);
  };
  int k, j, i;
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < nv; ++v) {
      at(2 * s, k, j, i);
      prim(v, k, j, i) = in[s * nv + v];
      at(2 * s + 1, k, j, i);
      prim(v, k, j, i) = in[(n + s) * nv + v];
    }
  const auto eos = plain_eos<F>(gamma);
  std::vector<double> out(std::size_t(nv) * n);
  for (long s = 0; s < n; ++s) {
    at(2 * s + 1, k, j, i);
    Riemann<F, RiemannSolver::llf>::Solve(eos, k, j, i, ivx, prim, cons, c_h);
    for (int v = 0; v < nv; ++v) out[s * nv + v] = cons.flux(ivx, v, k, j, i);
  }
  write_doubles(out);
}

void cmd_riemann(const Fluid f, const RiemannSolver s, const long n, const int ivx, const double gamma, const double c_h) {
  if (ivx < 1 || ivx > 3) die("ivx");
  if (f == Fluid::euler) {
    switch (s) {
    case RiemannSolver::none: return riemann_pads<Fluid::euler, RiemannSolver::none>(n, ivx, gamma, c_h);
    case RiemannSolver::hlle: return riemann_pads<Fluid::euler, RiemannSolver::hlle>(n, ivx, gamma, c_h);
    case RiemannSolver::hllc: return riemann_pads<Fluid::euler, RiemannSolver::hllc>(n, ivx, gamma, c_h);
    case RiemannSolver::llf: return riemann_llf<Fluid::euler>(n, ivx, gamma, c_h);
    default: die("no such euler solver");
    }
  }
  switch (s) {
  case RiemannSolver::none: return riemann_pads<Fluid::glmmhd, RiemannSolver::none>(n, ivx, gamma, c_h);
  case RiemannSolver::hlle: return riemann_pads<Fluid::glmmhd, RiemannSolver::hlle>(n, ivx, gamma, c_h);
  case RiemannSolver::hlld: return riemann_pads<Fluid::glmmhd, RiemannSolver::hlld>(n, ivx, gamma, c_h);
  case RiemannSolver::llf: return riemann_llf<Fluid::glmmhd>(n, ivx, gamma, c_h);
  default: die("no such glmmhd solver");
  }
}

// ---- c2p: the templated ConsToPrim(View4D ...) ------------------------------------------------------------------
template <Fluid F>
void cmd_c2p(const long n, const double gamma, const double pfloor, const double dfloor, const double efloor,
             const double vceil, const double eceil, const int nscalars) {
  const int nh = int(Hydro::GetNVars<F>()), nv = nh + nscalars;
  const auto in = read_doubles(std::size_t(nv) * n);
  parthenon::ParArray4D<Real> cons(nv, 1, 1, int(n)), prim(nv, 1, 1, int(n));
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < nv; ++v) cons(v, 0, 0, int(s)) = in[s * nv + v];
  const eos_t<F> eos(pfloor, dfloor, efloor, vceil, eceil, gamma);
  for (long s = 0; s < n; ++s) eos.ConsToPrim(cons, prim, nh, nscalars, 0, 0, int(s));
  std::vector<double> out(2 * std::size_t(nv) * n);
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < nv; ++v) {
      out[s * nv + v] = cons(v, 0, 0, int(s));
      out[(n + s) * nv + v] = prim(v, 0, 0, int(s));
    }
  write_doubles(out);
}

void cmd_speeds(const long n, const double gamma) {
  const auto in = read_doubles(5 * n);
  const auto eos = plain_eos<Fluid::glmmhd>(gamma);
  const auto eos_h = plain_eos<Fluid::euler>(gamma);
  std::vector<double> out(2 * n);
  for (long s = 0; s < n; ++s) {
    const double *p = &in[5 * s];
    Real w[NHYDRO] = {p[0], 0.0, 0.0, 0.0, p[1]};
    out[s] = eos_h.SoundSpeed(w);
    if (eos.SoundSpeed(w) != out[s] && out[s] == out[s]) die("the two SoundSpeed differ");
    out[n + s] = eos.FastMagnetosonicSpeed(p[0], p[1], p[2], p[3], p[4]);
  }
  write_doubles(out);
}

// ---- pencil: Reconstruct<recon, DIR> then Solve along one line of cells -----------------------------------------
// The only orchestration restated here is that of CalculateFluxes, src/hydro/hydro.cpp:1100-1199: in x1 the
// wrapper writes ql at i+1, so one call gives both sides of every face; in x2 / x3 the wrapper of row j writes the
// upper state of row j (the left state of face j+1) and the lower state qr of row j, so the left state of row j-1
// is kept and the two pads swap after every row.
template <Fluid F, Reconstruction RC, RiemannSolver S, int DIR>
void pencil(const long n, const double gamma, const double c_h, const double dx) {
  const int nv = int(Hydro::GetNVars<F>());
  const int N = int(n);
  const int g = (RC == Reconstruction::dc) ? 0 : (RC == Reconstruction::ppm || RC == Reconstruction::wenoz) ? 2 : 1;
  const auto in = read_doubles(std::size_t(nv) * n);
  int dim[3] = {1, 1, 1};
  dim[3 - DIR] = N;
  parthenon::VariablePack<Real> prim(nv, dim[0], dim[1], dim[2]);
  prim.coords.dx[0] = prim.coords.dx[1] = prim.coords.dx[2] = dx;
  parthenon::VariableFluxPack<Real> cons(nv, dim[0], dim[1], dim[2]);
  auto at = [&](const int c, int &k, int &j, int &i) {
    k = j = i = 0;
    (DIR == 1 ? i : DIR == 2 ? j : k) = c;
  };
  int k, j, i;
  for (int c = 0; c < N; ++c)
    for (int v = 0; v < nv; ++v) {
      at(c, k, j, i);
      prim(v, k, j, i) = in[std::size_t(c) * nv + v];
      cons.flux(DIR, v, k, j, i) = 0.0;
    }
  const auto eos = plain_eos<F>(gamma);
  const parthenon::team_mbr_t member;
  const int width = (DIR == 1) ? N + 1 : 1;
  parthenon::ScratchPad2D<Real> wl(nv, width), wr(nv, width), wlb(nv, width);
  if (DIR == 1) {
    Reconstruct<RC, DIR>(member, 0, 0, g, N - 1 - g, prim, wl, wr);
    Riemann<F, S>::Solve(member, 0, 0, g + 1, N - 1 - g, IV1, wl, wr, cons, eos, c_h);
  } else {
    for (int c = g; c <= N - 1 - g; ++c) {
      at(c, k, j, i);
      Reconstruct<RC, DIR>(member, k, j, 0, 0, prim, wlb, wr);
      if (c > g) Riemann<F, S>::Solve(member, k, j, 0, 0, DIR, wl, wr, cons, eos, c_h);
      auto *tmp = wl.data();
      wl.assign_data(wlb.data());
      wlb.assign_data(tmp);
    }
  }
  std::vector<double> out(std::size_t(nv) * n);
  for (int c = 0; c < N; ++c)
    for (int v = 0; v < nv; ++v) {
      at(c, k, j, i);
      out[std::size_t(c) * nv + v] = cons.flux(DIR, v, k, j, i);
    }
  write_doubles(out);
}

template <Fluid F, Reconstruction RC, RiemannSolver S>
void pencil_dir(const int dir, const long n, const double gamma, const double c_h, const double dx) {
  switch (dir) {
  case 1: return pencil<F, RC, S, 1>(n, gamma, c_h, dx);
  case 2: return pencil<F, RC, S, 2>(n, gamma, c_h, dx);
  case 3: return pencil<F, RC, S, 3>(n, gamma, c_h, dx);
  default: die("dir");
  }
}

template <Fluid F, RiemannSolver S>
void pencil_recon(const Reconstruction rc, const int dir, const long n, const double gamma, const double c_h,
                  const double dx) {
  switch (rc) {
  case Reconstruction::dc: return pencil_dir<F, Reconstruction::dc, S>(dir, n, gamma, c_h, dx);
  case Reconstruction::plm: return pencil_dir<F, Reconstruction::plm, S>(dir, n, gamma, c_h, dx);
  case Reconstruction::ppm: return pencil_dir<F, Reconstruction::ppm, S>(dir, n, gamma, c_h, dx);
  case Reconstruction::wenoz: return pencil_dir<F, Reconstruction::wenoz, S>(dir, n, gamma, c_h, dx);
  case Reconstruction::weno3: return pencil_dir<F, Reconstruction::weno3, S>(dir, n, gamma, c_h, dx);
  case Reconstruction::limo3: return pencil_dir<F, Reconstruction::limo3, S>(dir, n, gamma, c_h, dx);
  default: die("recon");
  }
}

void cmd_pencil(const Fluid f, const Reconstruction rc, const RiemannSolver s, const int dir, const long n,
                const double gamma, const double c_h, const double dx) {
  if (f == Fluid::euler && s == RiemannSolver::hlle) return pencil_recon<Fluid::euler, RiemannSolver::hlle>(rc, dir, n, gamma, c_h, dx);
  if (f == Fluid::euler && s == RiemannSolver::hllc) return pencil_recon<Fluid::euler, RiemannSolver::hllc>(rc, dir, n, gamma, c_h, dx);
  if (f == Fluid::glmmhd && s == RiemannSolver::hlle) return pencil_recon<Fluid::glmmhd, RiemannSolver::hlle>(rc, dir, n, gamma, c_h, dx);
  if (f == Fluid::glmmhd && s == RiemannSolver::hlld) return pencil_recon<Fluid::glmmhd, RiemannSolver::hlld>(rc, dir, n, gamma, c_h, dx);
  die("no such pencil combination");
}

} // namespace

int main(int argc, char **argv) {
  const uint16_t one = 1;
  if (*reinterpret_cast<const unsigned char *>(&one) != 1) die("little-endian hosts only");
  if (argc < 2) die("usage: ref_vectors recon|riemann|c2p|speeds|pencil ... (see the head of ref_vectors.cpp)");
  const std::string cmd = argv[1];
  auto need = [&](const int n) {
    if (argc != n + 2) die("wrong number of arguments");
  };
  auto D = [&](const int a) { return std::strtod(argv[a], nullptr); }; // strtod reads "inf"
  auto L = [&](const int a) { return std::strtol(argv[a], nullptr, 10); };
  if (cmd == "recon") {
    need(4);
    cmd_recon(recon_of(argv[2]), L(3), D(4), L(5) != 0);
  } else if (cmd == "riemann") {
    need(6);
    cmd_riemann(fluid_of(argv[2]), solver_of(argv[3]), L(4), int(L(5)), D(6), D(7));
  } else if (cmd == "c2p") {
    need(9);
    if (fluid_of(argv[2]) == Fluid::euler)
      cmd_c2p<Fluid::euler>(L(3), D(4), D(5), D(6), D(7), D(8), D(9), int(L(10)));
    else
      cmd_c2p<Fluid::glmmhd>(L(3), D(4), D(5), D(6), D(7), D(8), D(9), int(L(10)));
  } else if (cmd == "speeds") {
    need(2);
    cmd_speeds(L(2), D(3));
  } else if (cmd == "pencil") {
    need(8);
    cmd_pencil(fluid_of(argv[2]), recon_of(argv[3]), solver_of(argv[4]), int(L(5)), L(6), D(7), D(8), D(9));
  } else {
    die("unknown subcommand");
  }
  return std::fflush(stdout) == 0 ? 0 : 2;
}
