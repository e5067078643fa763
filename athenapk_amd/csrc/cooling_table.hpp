// cooling_table.hpp -- the host half of TabularCooling::TabularCooling (src/hydro/srcterms/tabular_cooling.cpp:30-276):
// reading the two-column table file, its checks, the conversion to code units and the Townsend coefficients.  Shared by
// the deck parser (host/cooling.cpp, no GPU) and apk_cooling_table_create (kernels_cooling.hip), so that both refuse the
// same tables with the same messages.
#pragma once

#include <string>
#include <vector>

#include "../../include/apk_amd.h"

namespace apk {

struct CoolingTableHost {
  int n = 0;  // rows (n_temp_)
  double log_temp_start = 0, log_temp_final = 0, d_log_temp = 0, lambda_final = 0;
  std::vector<double> log_temps, log_lambdas;   // log_lambdas in code units
  std::vector<double> lambdas, temps;           // Townsend only (n)
  std::vector<double> alpha_k, Y_k;             // Townsend only (n - 1)
};

// The rows of a cooling table file, parsed as tabular_cooling.cpp:103-141 does (blank, all-space and '#' lines skipped,
// exactly two numbers per line).  Returns "" or the reference's message.
std::string cooling_table_read(const std::string &filename, std::vector<double> *log_temps,
                               std::vector<double> *log_lambdas);

// The checks and precomputation of tabular_cooling.cpp:143-266 on n rows as read (log_lambdas in cgs units of
// lambda_units_cgs).  Returns "" or the reference's message.
std::string cooling_table_build(const double *log_temps, const double *log_lambdas, int n, const apk_cooling_params &p,
                                CoolingTableHost *out);

}  // namespace apk
