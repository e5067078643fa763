// cooling.cpp -- <units>, the gas composition and <cooling> on the host: Units (src/units.hpp), the composition and
// temperature floor / ceiling of Hydro::Initialize (src/hydro/hydro.cpp:482-536) and the table part of
// TabularCooling::TabularCooling (src/hydro/srcterms/tabular_cooling.cpp:30-276).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>

#include "../cooling_table.hpp"
#include "sim_internal.hpp"

namespace apk {

std::string cooling_table_read(const std::string &filename, std::vector<double> *log_temps,
                               std::vector<double> *log_lambdas) {
  std::ifstream f(filename);
  if (!f) return "### FATAL ERROR in function [TabularCooling::TabularCooling]\ncannot open cooling table \"" + filename + "\"";
  std::stringstream tab_ss;
  tab_ss << f.rdbuf();
  log_temps->clear();
  log_lambdas->clear();
  std::string line;
  while (tab_ss.good()) {
    std::getline(tab_ss, line);
    if (line.empty()) continue;                                   // skip blank line
    const std::size_t first_char = line.find_first_not_of(" ");  // skip white space
    if (first_char == std::string::npos) continue;                // line is all white space
    if (line.compare(first_char, 1, "#") == 0) continue;          // skip comments
    std::istringstream iss(line);
    std::vector<std::string> line_data{std::istream_iterator<std::string>{iss}, std::istream_iterator<std::string>{}};
    if (line_data.size() != 2)
      return "### FATAL ERROR in function [TabularCooling::TabularCooling]\nExpected exactly two columns per line but got: \"" +
             line + "\"";
    try {
      const double lt = std::stod(line_data[0]);
      const double ll = std::stod(line_data[1]);
      log_temps->push_back(lt);
      log_lambdas->push_back(ll);
    } catch (const std::exception &ia) {  // (invalid_argument; out_of_range alike)
      return std::string("### FATAL ERROR in function [TabularCooling::TabularCooling]\nNumber: \"") + ia.what() +
             "\" could not be parsed as double";
    }
  }
  return "";
}

std::string cooling_table_build(const double *log_temps, const double *log_lambdas_in, int n, const apk_cooling_params &p,
                                 CoolingTableHost *out) {
  const std::string head = "### FATAL ERROR in function [TabularCooling::TabularCooling]\n";
  char buf[512];
  if (p.integrator < APK_COOL_RK12 || p.integrator > APK_COOL_TOWNSEND)
    return "Unknown cooling integrator. Options are: rk12, rk45, townsend";
  if (!(p.lambda_units > 0.0)) return "cooling: lambda_units must be positive";
  if (n < 2 || !log_temps || !log_lambdas_in) return head + "Not enough data to interpolate cooling";
  const double log_temp_start = log_temps[0];
  const double d_log_temp = log_temps[1] - log_temp_start;
  if (d_log_temp <= 0) return head + "second log_temp in table is descreasing";
  for (int i = 1; i < n; i++) {
    const double d_log_temp_i = log_temps[i] - log_temps[i - 1];
    if (d_log_temp_i < 0) {
      std::snprintf(buf, sizeof(buf), "log_temp in table is descreasing at i= %d log_temp= %g", i, log_temps[i]);
      return head + buf;
    }
    // (DeDt indexes the table directly: even spacing, unless only Townsend's search reads it)
    if (((p.integrator != APK_COOL_TOWNSEND) || (p.cfl > 0.0)) &&
        (std::fabs(d_log_temp_i - d_log_temp) / d_log_temp > p.d_log_temp_tol)) {
      std::snprintf(buf, sizeof(buf),
                    "d_log_temp in table is uneven at i=%d log_temp=%g d_log_temp= %g d_log_temp_i= %g diff= %g "
                    "rel_diff= %g tol= %g",
                    i, log_temps[i], d_log_temp, d_log_temp_i, d_log_temp_i - d_log_temp,
                    std::fabs(d_log_temp_i - d_log_temp) / d_log_temp, p.d_log_temp_tol);
      return head + buf;
    }
  }
  CoolingTableHost t;
  t.n = n;
  t.log_temps.assign(log_temps, log_temps + n);
  t.log_lambdas.resize(n);
  const double shift = std::log10(p.lambda_units);
  for (int i = 0; i < n; i++) t.log_lambdas[i] = log_lambdas_in[i] - shift;  // (tabular_cooling.cpp:134)
  t.log_temp_start = log_temps[0];
  t.log_temp_final = log_temps[n - 1];
  t.d_log_temp = d_log_temp;
  t.lambda_final = std::pow(10.0, t.log_lambdas[n - 1]);
  if (p.integrator == APK_COOL_TOWNSEND) {  // piecewise power laws (tabular_cooling.cpp:216-266)
    t.lambdas.resize(n);
    t.temps.resize(n);
    for (int i = 0; i < n; i++) {
      t.lambdas[i] = std::pow(10.0, t.log_lambdas[i]);
      t.temps[i] = std::pow(10.0, log_temps[i]);
    }
    const int n_bins = n - 1;
    t.alpha_k.resize(n_bins);
    t.Y_k.resize(n_bins);
    for (int i = 0; i < n_bins; i++) {
      t.alpha_k[i] = (std::log10(t.lambdas[i + 1]) - std::log10(t.lambdas[i])) / (log_temps[i + 1] - log_temps[i]);
      if (t.alpha_k[i] == 1.0) return "Need to implement special case for Townsend piecewise fits.";
    }
    t.Y_k[n_bins - 1] = 0.0;  // Y_N = Y(T_ref) = 0
    for (int i = n_bins - 2; i >= 0; i--) {
      const double alpha_k_m1 = t.alpha_k[i] - 1.0;
      const double step = (t.lambdas[n_bins] / t.lambdas[i]) * (t.temps[i] / t.temps[n_bins]) *
                          (std::pow(t.temps[i] / t.temps[i + 1], alpha_k_m1) - 1.0) / alpha_k_m1;
      t.Y_k[i] = t.Y_k[i + 1] - step;
    }
  }
  *out = std::move(t);
  return "";
}

namespace host {

// Units (src/units.hpp:15-54, 62-126): the constants, in cgs
namespace cgs {
constexpr double atomic_mass_unit = 1.660538921e-24;  // g
constexpr double mh = 1.007947 * atomic_mass_unit;    // g (as yt defines it)
constexpr double k_boltzmann = 1.3806488e-16;         // erg / K
}  // namespace cgs

// <units> and hydro/He_mass_fraction (hydro.cpp:482-503); called by hydro_initialize before the EOS floors
void units_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  UnitsState &u = s->pkg.units;
  u = UnitsState{};
  u.has_units = pin.DoesBlockExist("units");
  if (u.has_units) {
    u.code_length_cgs = pin.GetOrAddReal("units", "code_length_cgs", 1);
    u.code_mass_cgs = pin.GetOrAddReal("units", "code_mass_cgs", 1);
    u.code_time_cgs = pin.GetOrAddReal("units", "code_time_cgs", 1);
  }
  if (u.has_units && pin.DoesParameterExist("hydro", "He_mass_fraction")) {
    u.has_composition = true;
    const double He_mass_fraction = pin.GetReal("hydro", "He_mass_fraction");
    u.He_mass_fraction = He_mass_fraction;
    u.mu = 1 / (He_mass_fraction * 3. / 4. + (1 - He_mass_fraction) * 2);
    u.mu_e = 1 / (He_mass_fraction * 2. / 4. + (1 - He_mass_fraction));
    u.mbar = u.mu * u.atomic_mass_unit();
    // (the mean molecular weight in units of mh, as the astro community does)
    u.mbar_over_kb = u.mu * u.mh() / u.k_boltzmann();
  }
}

// <cooling> (hydro.cpp:723-738, tabular_cooling.cpp:30-276).  Unlike the reference, an unknown integrator is refused
// here rather than at the first source-term call, and what this path does not implement is refused too.
void cooling_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  HydroPackage &pkg = s->pkg;
  pkg.cooling = false;
  pkg.cool = apk_cooling_params{};
  pkg.cool_table = CoolingTableHost{};
  const std::string enable = pin.GetOrAddString("cooling", "enable_cooling", "none");
  if (enable == "tabular") pkg.cooling = true;
  else if (enable != "none")
    throw std::runtime_error("AthenaPK hydro: Unknown cooling string. Supported options are 'none' and 'tabular'");
  if (!pkg.cooling) return;
  const UnitsState &u = pkg.units;
  if (!u.has_composition)
    throw std::runtime_error("Tabular cooling requires units and gas composition. Set a 'units' block and "
                             "'hydro/He_mass_fraction' in the input file.");
  if (pin.GetOrAddString("parthenon/mesh", "refinement", "none") != "none")
    throw std::runtime_error("Tabular cooling on refined meshes is not supported: parthenon/mesh/refinement must be none.");
  apk_cooling_params &c = pkg.cool;
  const std::string table_filename = pin.GetString("cooling", "table_filename");
  const double lambda_units_cgs = pin.GetReal("cooling", "lambda_units_cgs");
  // erg cm^3 / s in code units (tabular_cooling.cpp:48-51)
  c.lambda_units = lambda_units_cgs / (u.erg() * std::pow(u.cm(), 3) / u.s());
  const std::string integrator = pin.GetOrAddString("cooling", "integrator", "rk12");
  if (integrator == "rk12") c.integrator = APK_COOL_RK12;
  else if (integrator == "rk45") c.integrator = APK_COOL_RK45;
  else if (integrator == "townsend") c.integrator = APK_COOL_TOWNSEND;
  else throw std::runtime_error("Unknown cooling integrator '" + integrator + "'. Options are: rk12, rk45, townsend");
  c.max_iter = pin.GetOrAddInteger("cooling", "max_iter", 100);
  if (c.max_iter < 1) throw std::runtime_error("cooling/max_iter must be >= 1");
  c.cfl = pin.GetOrAddReal("cooling", "cfl", 0.1);
  c.d_log_temp_tol = pin.GetOrAddReal("cooling", "d_log_temp_tol", 1e-8);
  c.d_e_tol = pin.GetOrAddReal("cooling", "d_e_tol", 1e-8);
  c.T_floor = pin.GetOrAddReal("hydro", "Tfloor", -1.0);  // (negative: none)
  c.gamma = pkg.eos.gamma;
  c.mbar_over_kb = u.mbar_over_kb;
  c.He_mass_fraction = u.He_mass_fraction;
  c.mh = u.mh();
  std::vector<double> lt, ll;
  std::string err = cooling_table_read(table_filename, &lt, &ll);
  if (err.empty()) err = cooling_table_build(lt.data(), ll.data(), (int)lt.size(), c, &pkg.cool_table);
  if (!err.empty()) throw std::runtime_error(err);
  // a fingerprint of the table as this rank read it: every rank must hold the same one (estimate_timestep_commit)
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < pkg.cool_table.n; ++i)
    for (double v : {pkg.cool_table.log_temps[i], pkg.cool_table.log_lambdas[i]}) {
      uint64_t b;
      std::memcpy(&b, &v, sizeof(b));
      h = (h ^ b) * 1099511628211ull;
    }
  pkg.cool_table_hash = (double)(h >> 11);  // (53 bits: exact as a double)
}

}  // namespace host

double UnitsState::code_energy_cgs() const {
  return code_mass_cgs * code_length_cgs * code_length_cgs / (code_time_cgs * code_time_cgs);
}
double UnitsState::k_boltzmann() const { return host::cgs::k_boltzmann / code_energy_cgs(); }
double UnitsState::mh() const { return host::cgs::mh / code_mass_cgs; }
double UnitsState::atomic_mass_unit() const { return host::cgs::atomic_mass_unit / code_mass_cgs; }
double UnitsState::erg() const { return 1.0 / code_energy_cgs(); }
double UnitsState::cm() const { return 1.0 / code_length_cgs; }
double UnitsState::s() const { return 1.0 / code_time_cgs; }

}  // namespace apk
