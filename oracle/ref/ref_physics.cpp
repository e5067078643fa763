// ref_physics.cpp -- runs the REFERENCE's own header-inline physics on raw fp64 vectors: units, the cluster's gravity
// and entropy profile, the jet frame, the magnetic tower, the add-density helpers, the cooling table's DeDt with the
// two Runge-Kutta steppers, and the diffusion limiters.
//
// TEST INFRASTRUCTURE.  This file is this project's; it holds no reference code.  It includes the reference's
// headers by include path only (the tree is given to the Makefile as APK_REFERENCE_SRC), against the stand-in
// names of standin/apk_standin.hpp + standin/apk_standin_physics.hpp, and the binary it builds into oracle/_ref/ is
// never committed.
//
// Conventions of ref_vectors.cpp: little-endian fp64 from stdin, little-endian fp64 to stdout, arrays row-major,
// 17 digits wherever text is written.  Every argument that holds a '=' is a deck entry block/key=value (the block is
// what precedes the LAST '/' before the '='); the entries fill the stand-in ParameterInput, so that the reference's own
// constructors run with their key names, their defaults and their Units(pin).  The other arguments are positional:
//   units                                out: text, one "name value" line per public accessor of Units
//   gravity <n>                          in r[n]                        out g_from_r[n]
//   entropy <n>                          in r[n]                        out K_from_r[n]
//   jet <theta> <phi0> <phidot> <time> <n>
//                                        in p[n][3], (cos, sin, v_r, v_theta, v_h)[n][5]
//                                        out (r, cos_theta, sin_theta, h)[n][4], v_sim[n][3]
//                                        through JetCoordsFactory(pin).CreateJetCoords(time)
//   tower <field> <density> <time> <n>   in p[n][3]                     out A[n][3], B[n][3], density[n]
//                                        MagneticTower(pin)'s members, JetCoordsFactory(pin), then MagneticTowerObj
//                                        with the argument list of magnetic_tower.cpp:65-67; the density is 0 unless
//                                        <density> > 0, as magnetic_tower.cpp:134-137
//   dedt <table file> <n>                in (e, rho)[n][2]              out de_dt[n], valid[n]
//   rkstep rk12|rk45 <table file> <n>    in (e0, rho, h)[n][3], (h, err, tol)[n][3]
//                                        out y1_h[n], y1_l[n], valid[n], OptimalStep[n]
//                                        f = [&](t, e, valid) { return table.DeDt(e, rho, valid); }, valid = true before
//                                        the step, as tabular_cooling.cpp:350-352 and :395
//   limiters <n>                         in (A, B, C, D)[n][4]          out vanleer(A,B)[n], minmod(A,B)[n], mc(A,B)[n],
//                                                                           lim2(A,B)[n], lim4(A,B,C,D)[n]
//   adddensity fixedvel|fixedveltemp <gamma> <n>
//                                        in (delta, cons[5], prim[5])[n][11]   out cons[n][5]
//
// The CoolingTableObj is built with the arguments TabularCooling's constructor passes.  Only that list is restated here
// (make_table below), from tabular_cooling.cpp: lambda_units :48-51, the rows' log_lambda - log10(lambda_units) :134,
// log_temp_start, d_log_temp :155-156, n_temp, log_temp_final :194-197, and the call :269-275 with
// mbar_over_kb = mu mh / k_B of hydro.cpp:495, :503.  Keys: cooling/lambda_units_cgs (required), hydro/gamma,
// hydro/He_mass_fraction, units/*.
//
// rho_from_r is NOT offered: it reads rho_const_nfw_ and rho_const_bcg_, which the reference never initialises.
//
// NEVER feed inputs on which PARTHENON_REQUIRE or Kokkos::abort fires: they abort, as in the reference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "hydro/hydro.hpp" // first: brings Real, the enums and the prelude names into scope for the headers below
#include "parameter_input.hpp"
#include "units.hpp"
#include "hydro/diffusion/diffusion.hpp"
#include "hydro/srcterms/tabular_cooling.hpp"
#include "pgen/cluster/cluster_gravity.hpp"
#include "pgen/cluster/cluster_utils.hpp"
#include "pgen/cluster/entropy_profiles.hpp"
#include "pgen/cluster/jet_coords.hpp"
#include "pgen/cluster/magnetic_tower.hpp"

// the block-level ConservedToPrimitive(MeshData*) live in .cpp files that need the framework; they are never called
void AdiabaticHydroEOS::ConservedToPrimitive(MeshData<Real> *) const {}
void AdiabaticGLMMHDEOS::ConservedToPrimitive(MeshData<Real> *) const {}

namespace {

[[noreturn]] void die(const char *msg) {
  std::fprintf(stderr, "ref_physics: %s\n", msg);
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

void cmd_units(parthenon::ParameterInput *pin) {
  const Units u(pin);
#define SHOW(name) std::printf(#name " %.17g\n", u.name())
  SHOW(code_length_cgs);
  SHOW(code_mass_cgs);
  SHOW(code_time_cgs);
  SHOW(code_energy_cgs);
  SHOW(code_density_cgs);
  SHOW(code_pressure_cgs);
  SHOW(code_entropy_kev_cm2);
  SHOW(code_magnetic_cgs);
  SHOW(k_boltzmann);
  SHOW(gravitational_constant);
  SHOW(speed_of_light);
  SHOW(kev);
  SHOW(g);
  SHOW(cm);
  SHOW(cm_s);
  SHOW(km_s);
  SHOW(kpc);
  SHOW(mpc);
  SHOW(s);
  SHOW(yr);
  SHOW(myr);
  SHOW(dyne_cm2);
  SHOW(g_cm3);
  SHOW(msun);
  SHOW(atomic_mass_unit);
  SHOW(electron_mass);
  SHOW(mh);
  SHOW(erg);
  SHOW(gauss);
  SHOW(microgauss);
#undef SHOW
}

void cmd_gravity(parthenon::ParameterInput *pin, const long n) {
  const cluster::ClusterGravity grav(pin);
  const auto r = read_doubles(n);
  std::vector<double> out(n);
  for (long s = 0; s < n; ++s) out[s] = grav.g_from_r(r[s]);
  write_doubles(out);
}

void cmd_entropy(parthenon::ParameterInput *pin, const long n) {
  const cluster::ACCEPTEntropyProfile prof(pin);
  const auto r = read_doubles(n);
  std::vector<double> out(n);
  for (long s = 0; s < n; ++s) out[s] = prof.K_from_r(r[s]);
  write_doubles(out);
}

void cmd_jet(parthenon::ParameterInput *pin, const double time, const long n) {
  parthenon::StateDescriptor pkg;
  const cluster::JetCoordsFactory factory(pin, &pkg);
  const cluster::JetCoords jc = factory.CreateJetCoords(time);
  const auto p = read_doubles(3 * n);
  const auto v = read_doubles(5 * n);
  std::vector<double> cyl(4 * n), sim(3 * n);
  for (long s = 0; s < n; ++s) {
    jc.SimCartToJetCylCoords(p[3 * s], p[3 * s + 1], p[3 * s + 2], cyl[4 * s], cyl[4 * s + 1], cyl[4 * s + 2], cyl[4 * s + 3]);
    jc.JetCylToSimCartVector(v[5 * s], v[5 * s + 1], v[5 * s + 2], v[5 * s + 3], v[5 * s + 4], sim[3 * s], sim[3 * s + 1],
                             sim[3 * s + 2]);
  }
  write_doubles(cyl);
  write_doubles(sim);
}

void cmd_tower(parthenon::ParameterInput *pin, const double field, const double density, const double time, const long n) {
  parthenon::StateDescriptor pkg;
  const cluster::JetCoordsFactory factory(pin, &pkg);
  const cluster::MagneticTower t(pin, &pkg);
  const cluster::MagneticTowerObj mt(field, t.alpha_, t.l_scale_, t.offset_, t.thickness_, density, t.l_mass_scale_,
                                     factory.CreateJetCoords(time), t.potential_);
  const auto p = read_doubles(3 * n);
  std::vector<double> a(3 * n), b(3 * n), rho(n);
  for (long s = 0; s < n; ++s) {
    const double x = p[3 * s], y = p[3 * s + 1], z = p[3 * s + 2];
    mt.PotentialInSimCart(x, y, z, a[3 * s], a[3 * s + 1], a[3 * s + 2]);
    mt.FieldInSimCart(x, y, z, b[3 * s], b[3 * s + 1], b[3 * s + 2]);
    rho[s] = density > 0.0 ? mt.DensityFromSimCart(x, y, z) : 0.0;
  }
  write_doubles(a);
  write_doubles(b);
  write_doubles(rho);
}

cooling::CoolingTableObj make_table(parthenon::ParameterInput *pin, const char *path) {
  const Units units(pin);
  if (!pin->DoesParameterExist("cooling", "lambda_units_cgs")) die("cooling/lambda_units_cgs is required");
  const Real lambda_units_cgs = pin->GetOrAddReal("cooling", "lambda_units_cgs", 0.0);
  const Real lambda_units = lambda_units_cgs / (units.erg() * pow(units.cm(), 3) / units.s());
  std::ifstream f(path);
  if (!f) die("cannot open the cooling table");
  std::vector<Real> log_temps, log_lambdas;
  std::string line;
  while (std::getline(f, line)) {
    const std::size_t c = line.find_first_not_of(" \t\r");
    if (c == std::string::npos || line[c] == '#') continue;
    std::istringstream iss(line);
    double lt, ll;
    if (!(iss >> lt >> ll)) die("a table row is not two numbers");
    log_temps.push_back(lt);
    log_lambdas.push_back(ll - std::log10(lambda_units));
  }
  if (log_temps.size() < 2) die("the table has fewer than two rows");
  const unsigned int n_temp = log_temps.size();
  const Real log_temp_start = log_temps[0];
  const Real d_log_temp = log_temps[1] - log_temp_start;
  const Real log_temp_final = log_temps[n_temp - 1];
  parthenon::ParArray1D<Real> view("log_lambdas_", n_temp);
  for (unsigned int i = 0; i < n_temp; ++i) view(i) = log_lambdas[i];
  const Real He = pin->GetOrAddReal("hydro", "He_mass_fraction", 0.25);
  const Real gamma = pin->GetOrAddReal("hydro", "gamma", 5. / 3.);
  const Real mu = 1 / (He * 3. / 4. + (1 - He) * 2);
  const Real mbar_over_kb = mu * units.mh() / units.k_boltzmann();
  return cooling::CoolingTableObj(view, log_temp_start, log_temp_final, d_log_temp, n_temp, mbar_over_kb, gamma, 1.0 - He,
                                  units);
}

void cmd_dedt(parthenon::ParameterInput *pin, const char *path, const long n) {
  const auto table = make_table(pin, path);
  const auto in = read_doubles(2 * n);
  std::vector<double> out(2 * n);
  for (long s = 0; s < n; ++s) {
    bool valid = true;
    out[s] = table.DeDt(in[2 * s], in[2 * s + 1], valid);
    out[n + s] = valid ? 1.0 : 0.0;
  }
  write_doubles(out);
}

template <class Stepper>
void cmd_rkstep(parthenon::ParameterInput *pin, const char *path, const long n) {
  const auto table = make_table(pin, path);
  const auto in = read_doubles(3 * n);
  const auto opt = read_doubles(3 * n);
  std::vector<double> out(4 * n);
  for (long s = 0; s < n; ++s) {
    const Real e0 = in[3 * s], rho = in[3 * s + 1], h = in[3 * s + 2];
    auto f = [&](const Real, const Real e, bool &valid) { return table.DeDt(e, rho, valid); };
    bool valid = true;
    Real y1_h, y1_l;
    Stepper::Step(0.0, h, e0, f, y1_h, y1_l, valid);
    out[s] = y1_h;
    out[n + s] = y1_l;
    out[2 * n + s] = valid ? 1.0 : 0.0;
    out[3 * n + s] = Stepper::OptimalStep(opt[3 * s], opt[3 * s + 1], opt[3 * s + 2]);
  }
  write_doubles(out);
}

void cmd_limiters(const long n) {
  const auto q = read_doubles(4 * n);
  std::vector<double> out(5 * n);
  for (long s = 0; s < n; ++s) {
    const double a = q[4 * s], b = q[4 * s + 1], c = q[4 * s + 2], d = q[4 * s + 3];
    out[s] = limiters::vanleer(a, b);
    out[n + s] = limiters::minmod(a, b);
    out[2 * n + s] = limiters::mc(a, b);
    out[3 * n + s] = limiters::lim2(a, b);
    out[4 * n + s] = limiters::lim4(a, b, c, d);
  }
  write_doubles(out);
}

void cmd_adddensity(const bool temp, const double gamma, const long n) {
  const auto in = read_doubles(11 * n);
  parthenon::ParArray4D<Real> cons(5, 1, 1, int(n)), prim(5, 1, 1, int(n));
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < 5; ++v) {
      cons(v, 0, 0, int(s)) = in[11 * s + 1 + v];
      prim(v, 0, 0, int(s)) = in[11 * s + 6 + v];
    }
  for (long s = 0; s < n; ++s) {
    if (temp)
      cluster::AddDensityToConsAtFixedVelTemp(in[11 * s], cons, prim, gamma, 0, 0, int(s));
    else
      cluster::AddDensityToConsAtFixedVel(in[11 * s], cons, prim, 0, 0, int(s));
  }
  std::vector<double> out(5 * n);
  for (long s = 0; s < n; ++s)
    for (int v = 0; v < 5; ++v) out[5 * s + v] = cons(v, 0, 0, int(s));
  write_doubles(out);
}

} // namespace

int main(int argc, char **argv) {
  const uint16_t one = 1;
  if (*reinterpret_cast<const unsigned char *>(&one) != 1) die("little-endian hosts only");
  parthenon::ParameterInput pin;
  std::vector<std::string> a; // the positional arguments
  for (int i = 1; i < argc; ++i) {
    const std::string s = argv[i];
    const std::size_t eq = s.find('=');
    if (eq == std::string::npos) {
      a.push_back(s);
      continue;
    }
    const std::size_t slash = s.rfind('/', eq);
    if (slash == std::string::npos || slash == 0 || slash + 1 == eq) die("a deck entry is block/key=value");
    pin.Set(s.substr(0, slash), s.substr(slash + 1, eq - slash - 1), s.substr(eq + 1));
  }
  if (a.empty()) die("usage: ref_physics units|gravity|entropy|jet|tower|dedt|rkstep|limiters|adddensity ... (see the head of ref_physics.cpp)");
  const std::string cmd = a[0];
  auto need = [&](const std::size_t n) {
    if (a.size() != n + 1) die("wrong number of positional arguments");
  };
  auto D = [&](const int i) { return std::strtod(a[i].c_str(), nullptr); };
  auto L = [&](const int i) { return std::strtol(a[i].c_str(), nullptr, 10); };
  auto set_real = [&](const char *name, const double v) {
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    pin.Set("problem/cluster/precessing_jet", name, buf);
  };
  try {
    if (cmd == "units") {
      need(0);
      cmd_units(&pin);
    } else if (cmd == "gravity") {
      need(1);
      cmd_gravity(&pin, L(1));
    } else if (cmd == "entropy") {
      need(1);
      cmd_entropy(&pin, L(1));
    } else if (cmd == "jet") {
      need(5);
      set_real("jet_theta", D(1));
      set_real("jet_phi0", D(2));
      set_real("jet_phi_dot", D(3));
      cmd_jet(&pin, D(4), L(5));
    } else if (cmd == "tower") {
      need(4);
      cmd_tower(&pin, D(1), D(2), D(3), L(4));
    } else if (cmd == "dedt") {
      need(2);
      cmd_dedt(&pin, a[1].c_str(), L(2));
    } else if (cmd == "rkstep") {
      need(3);
      if (a[1] == "rk12")
        cmd_rkstep<cooling::RK12Stepper>(&pin, a[2].c_str(), L(3));
      else if (a[1] == "rk45")
        cmd_rkstep<cooling::RK45Stepper>(&pin, a[2].c_str(), L(3));
      else
        die("rkstep rk12|rk45");
    } else if (cmd == "limiters") {
      need(1);
      cmd_limiters(L(1));
    } else if (cmd == "adddensity") {
      need(3);
      if (a[1] != "fixedvel" && a[1] != "fixedveltemp") die("adddensity fixedvel|fixedveltemp");
      cmd_adddensity(a[1] == "fixedveltemp", D(2), L(3));
    } else {
      die("unknown subcommand");
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "ref_physics: the reference threw: %s\n", e.what());
    return 3;
  }
  return std::fflush(stdout) == 0 ? 0 : 2;
}
