// kernels_cooling.hip -- tabular radiative cooling (src/hydro/srcterms/tabular_cooling.{hpp,cpp}):
//   CoolingTableObj::DeDt                 tabular_cooling.hpp:129-173
//   SubcyclingFixedIntSrcTerm<RK12|RK45>  tabular_cooling.cpp:290-487   adaptive dual-order RK subcycling
//   TownsendSrcTerm                       tabular_cooling.cpp:489-604   exact integration (Townsend 2009)
//   EstimateTimeStep                      tabular_cooling.cpp:606-665   min-reduction of |e / DeDt|
// and the C-ABI entries of include/apk_amd.h (apk_cooling_table_*, apk_cooling_dedt, apk_tabular_cooling_src,
// apk_estimate_cooling_timestep).
//
// Kernel structure.  One lane per interior cell, lanes laid along x1 (a wave is 64 consecutive cells of a row, and
// neighbouring cells have similar temperatures, so similar substep counts).  The subcycle loop is lane-divergent: a wave
// runs as long as its slowest lane, and the cost of a wave is (max substeps over its lanes) x (one RK step).  The RK
// stepper is a template parameter, so each kernel carries only its own stages.  Each cell reads 5 (Euler) or 8 (GLM-MHD)
// conserved variables and writes one (IEN): 48 B resp. 72 B per cell; the rest is arithmetic: each DeDt is one log10 and
// one pow(10, x) in fp64 plus ~15 other fp64 operations, and an RK45 step makes six of them.  The table (log_lambdas, a
// few hundred doubles) is read through the cached global path: a wave's lanes read at most a few neighbouring entries.
//
// Build forms.  The parity build (APK_FP_STRICT) keeps the reference's expression order and libm calls: log10,
// pow(10., x), pow(tol / err, 2 | 5).  The product build uses exp10 for pow(10., x) and multiplies for the integer powers.
// (This file is compiled without -fapprox-func in the product build too -- see the Makefile -- so the libm calls stay
// the accurate ones.)
//
// Deviations from the reference, documented in include/apk_amd.h:
//  - only interior cells are cooled (the reference: IndexDomain::entire); the stage's ghost exchange refills the ghosts
//  - prim(IPR) is not written (ConsToPrim recomputes it after the stage)
//  - the reference's device failures (PARTHENON_FAIL "Sub cycles exceed max_iter", PARTHENON_REQUIRE "Failed to find
//    log_temp") latch APK_FLAG_COOL_* in the flag word instead of trapping; the host fails the call
//  - DeDt clamps its table index to n - 2 (log T exactly at the top node would read one entry past the table in the
//    reference); a cell whose substep attempts would never end (a NaN error estimate at the minimum substep, where the
//    reference spins forever) stops after max_iter + 4 attempts with APK_FLAG_COOL_MAX_ITER.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "apk_internal.hpp"
#include "cooling_table.hpp"
#include "hydro_math.hpp"
#include "wg_reduce.hpp"

namespace apk {

namespace {

// what the kernels read: the device arrays and the scalars of TabularCooling / CoolingTableObj
struct CoolDev {
  const double *log_lambdas;                       // n (code units)
  const double *lambdas, *temps, *alpha_k, *Y_k;   // Townsend: n, n, n - 1, n - 1
  int n;
  double log_temp_start, log_temp_final, d_log_temp;
  double mbar_gm1_over_kb;  // mbar_over_kb * (gamma - 1)
  double x_H_over_m_h2;     // SQR((1 - He) / mh) (CoolingTableObj)
  double X_by_mh2;          // pow((1 - He) / mh, 2) (TownsendSrcTerm)
  double lambda_final, temp_final, temp_cool_floor;
  double e_floor_sub;       // max(T_floor, 10^log_temp_start) / mbar_gm1_over_kb (subcycling, time step)
  double e_floor_town;      // T_floor / mbar_gm1_over_kb (Townsend: T_floor as given)
  double d_e_tol;
  unsigned max_iter;
  int bsearch;              // Townsend: the index searches may bisect (temps increasing, Y_k decreasing)
};

APK_DEV double cool_pow10(double x) {
#ifdef APK_FP_STRICT
  return pow(10., x);
#else
  return exp10(x);
#endif
}

// CoolingTableObj::DeDt (tabular_cooling.hpp:129-173); ll: log_lambdas
APK_DEV double dedt(const CoolDev &c, const double *ll, double e, double rho, bool &is_valid, unsigned &flags) {
  if (e < 0 || isnan(e)) {
    is_valid = false;
    return 0;
  }
  const double temp = c.mbar_gm1_over_kb * e;
  const double log_temp = log10(temp);
  double log_lambda;
  if (log_temp < c.log_temp_start) {
    return 0;
  } else if (log_temp > c.log_temp_final) {
    // above the table: free-free cooling, lambda ~ T^(1/2)
    log_lambda = 0.5 * log_temp - 0.5 * c.log_temp_final + ll[c.n - 1];
  } else {
    unsigned int i_temp = static_cast<unsigned int>((log_temp - c.log_temp_start) / c.d_log_temp);
    if (i_temp > (unsigned)(c.n - 2)) i_temp = (unsigned)(c.n - 2);  // (log T at the top node: the last interval)
    const double log_temp_i = c.log_temp_start + c.d_log_temp * i_temp;
    if (!(log_temp >= log_temp_i && log_temp <= log_temp_i + c.d_log_temp)) flags |= APK_FLAG_COOL_TABLE;
    const double log_lambda_i = ll[i_temp];
    const double log_lambda_ip1 = ll[i_temp + 1];
    log_lambda = log_lambda_i + (log_temp - log_temp_i) * (log_lambda_ip1 - log_lambda_i) / c.d_log_temp;
  }
  const double lambda = cool_pow10(log_lambda);
  const double de_dt = -lambda * c.x_H_over_m_h2 * rho;
  return de_dt;
}

// RK12Stepper / RK45Stepper (tabular_cooling.hpp:36-93)
struct RK12 {
  template <typename F>
  static APK_DEV void Step(double h, double y0, F f, double &y1_h, double &y1_l, bool &valid) {
    const double f_t0_y0 = f(y0, valid);
    y1_l = y0 + h * f_t0_y0;                             // 1st order
    y1_h = y0 + h / 2. * (f_t0_y0 + f(y1_l, valid));     // 2nd order
  }
  static APK_DEV double OptimalStep(double h, double err, double tol) {
#ifdef APK_FP_STRICT
    return 0.95 * h * pow(tol / err, 2);
#else
    const double r = tol / err;
    return 0.95 * h * (r * r);
#endif
  }
};

struct RK45 {
  template <typename F>
  static APK_DEV void Step(double h, double y0, F f, double &y1_h, double &y1_l, bool &valid) {
    const double k1 = h * f(y0, valid);
    const double k2 = h * f(y0 + 1. / 4. * k1, valid);
    const double k3 = h * f(y0 + 3. / 32. * k1 + 9. / 32. * k2, valid);
    const double k4 = h * f(y0 + 1932. / 2197. * k1 - 7200. / 2197. * k2 + 7296. / 2197. * k3, valid);
    const double k5 = h * f(y0 + 439. / 216. * k1 - 8. * k2 + 3680. / 513. * k3 - 845. / 4104. * k4, valid);
    const double k6 =
        h * f(y0 - 8. / 27. * k1 + 2. * k2 - 3544. / 2565. * k3 + 1859. / 4104. * k4 - 11. / 40. * k5, valid);
    y1_l = y0 + 25. / 216. * k1 + 1408. / 2565. * k3 + 2197. / 4104. * k4 - 1. / 5. * k5;  // 4th order
    y1_h = y0 + 16. / 135. * k1 + 6656. / 12825. * k3 + 28561. / 56430. * k4 - 9. / 50. * k5 +
           2. / 55. * k6;  // 5th order
  }
  static APK_DEV double OptimalStep(double h, double err, double tol) {
#ifdef APK_FP_STRICT
    return 0.95 * h * pow(tol / err, 5);
#else
    const double r = tol / err, r2 = r * r;
    return 0.95 * h * (r2 * r2 * r);
#endif
  }
};

constexpr double kEpsilon = 1e-12;  // TabularCooling::KEpsilon_

// (b, k, j, i) of interior cell `idx` of the pack; false past the last one
APK_DEV bool cell_of(const PackView &pv, int64_t idx, int &b, int64_t &off) {
  const int64_t nrow = pv.nx1, nplane = nrow * pv.nx2, nblk = nplane * pv.nx3;
  if (idx >= nblk * pv.nblocks) return false;
  b = (int)(idx / nblk);
  int64_t r = idx - (int64_t)b * nblk;
  const int k = (int)(r / nplane);
  r -= (int64_t)k * nplane;
  const int j = (int)(r / nrow);
  const int i = (int)(r - (int64_t)j * nrow);
  off = (pv.ks + k) * pv.sk + (pv.js + j) * pv.sj + (pv.is + i);
  return true;
}

APK_DEV void latch(unsigned *d_flags, unsigned flags) {
  if (flags) atomicOr(d_flags, flags);
}

// SubcyclingFixedIntSrcTerm<RKStepper> (tabular_cooling.cpp:290-487), one interior cell per lane
template <typename RK, bool MHD>
__global__ void __launch_bounds__(256) cool_subcycle_kernel(PackView pv, CoolDev c, double dt, unsigned *d_flags) {
  const double *ll = c.log_lambdas;
  int b;
  int64_t off;
  if (!cell_of(pv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, b, off)) return;
  double *__restrict__ u = pv.blocks[b].cons + off;
  const int64_t sn = pv.sn;
  unsigned flags = 0;
  const double min_sub_dt = dt / c.max_iter;
  const double d_e_tol = c.d_e_tol;
  const double internal_e_floor = c.e_floor_sub;

  const double rho = u[IDN * sn];
  double internal_e = u[IEN * sn] - 0.5 * (sqr(u[IM1 * sn]) + sqr(u[IM2 * sn]) + sqr(u[IM3 * sn])) / rho;
  if constexpr (MHD) internal_e -= 0.5 * (sqr(u[IB1 * sn]) + sqr(u[IB2 * sn]) + sqr(u[IB3 * sn]));
  internal_e /= rho;
  const double internal_e_initial = internal_e;

  bool dedt_valid = true;
  auto f = [&](double e, bool &valid) { return dedt(c, ll, e, rho, valid, flags); };

  double sub_t = 0;
  double sub_dt = dt;  // try the full dt; the error control shrinks it
  const double dedt_initial = f(internal_e_initial, dedt_valid);
  if (dedt_initial == 0.0 || internal_e_initial <= internal_e_floor) {
    latch(d_flags, flags);
    return;
  }
  if (d_e_tol == 0) sub_dt = min_sub_dt;

  unsigned int sub_iter = 0;
  // (dedt != 0 in case the cooling floor is hit during subcycling)
  while ((sub_t * (1 + kEpsilon) < dt) && (f(internal_e, dedt_valid) != 0.0)) {
    if (sub_iter > c.max_iter) {  // "Sub cycles exceed max_iter (This should be impossible)"
      flags |= APK_FLAG_COOL_MAX_ITER;
      break;
    }
    double internal_e_next_h;
    double d_e_err = 0;
    unsigned int sub_attempt = 0;
    bool reattempt_sub = true;
    do {
      double internal_e_next_l;
      dedt_valid = true;
      RK::Step(sub_dt, internal_e, f, internal_e_next_h, internal_e_next_l, dedt_valid);
      sub_attempt++;
      if (!dedt_valid) {
        if (sub_dt == min_sub_dt) {
          // cooling so fast that even the minimum substep gives a negative energy: to the floor
          sub_dt = (dt - sub_t);
          internal_e_next_h = internal_e_floor;
          reattempt_sub = false;
        } else {
          reattempt_sub = true;
          sub_dt = min_sub_dt;
        }
      } else {
        d_e_err = fabs((internal_e_next_h - internal_e_next_l) / internal_e_next_h);
        reattempt_sub = false;
        if (isnan(d_e_err)) {
          reattempt_sub = true;
          sub_dt = min_sub_dt;
        } else if (d_e_err >= d_e_tol && sub_dt > min_sub_dt) {
          reattempt_sub = true;
          if (d_e_tol == 0) {
            sub_dt = min_sub_dt;
          } else {
            sub_dt = RK::OptimalStep(sub_dt, d_e_err, d_e_tol);
          }
          if (sub_dt < min_sub_dt || sub_attempt >= c.max_iter) sub_dt = min_sub_dt;
        }
      }
      if (reattempt_sub && sub_attempt > c.max_iter + 4) {  // (the reference would spin here forever)
        flags |= APK_FLAG_COOL_MAX_ITER;
        reattempt_sub = false;
      }
    } while (reattempt_sub);
    if (flags & APK_FLAG_COOL_MAX_ITER) break;
    sub_t += sub_dt;
    internal_e = internal_e_next_h;
    if (d_e_err == 0) {
      sub_dt = dt - sub_t;  // (error 0: to the end)
    } else {
      sub_dt = RK::OptimalStep(sub_dt, d_e_err, d_e_tol);  // grow (or shrink, at the minimum substep)
    }
    if (d_e_tol == 0) sub_dt = min_sub_dt;
    sub_dt = (sub_dt < min_sub_dt) ? min_sub_dt : sub_dt;  // std::max(sub_dt, min_sub_dt)
    sub_dt = ((dt - sub_t) < sub_dt) ? (dt - sub_t) : sub_dt;  // std::min(sub_dt, dt - sub_t)
    sub_iter++;
  }
  internal_e = (internal_e > internal_e_floor) ? internal_e : internal_e_floor;
  u[IEN * sn] += rho * (internal_e - internal_e_initial);
  latch(d_flags, flags);
}

// the reference's linear scans, or bisections returning the same index when the arrays are monotonic
APK_DEV int townsend_bin_up(const CoolDev &c, int nbins, double temp) {
  // first: while ((idx < nbins - 1) && (temps(idx + 1) < temp)) idx += 1;
  if (!c.bsearch) {
    int idx = 0;
    while ((idx < nbins - 1) && (c.temps[idx + 1] < temp)) idx += 1;
    return idx;
  }
  int lo = 1, hi = nbins;  // first k in [1, nbins - 1] with temps[k] >= temp (nbins: none)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c.temps[mid] < temp) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

APK_DEV int townsend_bin_down(const CoolDev &c, int idx, double tef_adj) {
  // while ((idx > 0) && (tef_adj > Y_k(idx))) idx -= 1;
  if (!c.bsearch) {
    while ((idx > 0) && (tef_adj > c.Y_k[idx])) idx -= 1;
    return idx;
  }
  if (!(tef_adj > c.Y_k[idx])) return idx;
  int lo = 0, hi = idx;  // largest j in [0, idx) with !(tef_adj > Y_k[j]); 0 if none
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (!(tef_adj > c.Y_k[mid])) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// TownsendSrcTerm (tabular_cooling.cpp:489-604)
template <bool MHD>
__global__ void __launch_bounds__(256) cool_townsend_kernel(PackView pv, CoolDev c, double dt) {
  int b;
  int64_t off;
  if (!cell_of(pv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, b, off)) return;
  double *__restrict__ u = pv.blocks[b].cons + off;
  const int64_t sn = pv.sn;
  const double rho = u[IDN * sn];
  double internal_e = u[IEN * sn] - 0.5 * (sqr(u[IM1 * sn]) + sqr(u[IM2 * sn]) + sqr(u[IM3 * sn])) / rho;
  if constexpr (MHD) internal_e -= 0.5 * (sqr(u[IB1 * sn]) + sqr(u[IB2 * sn]) + sqr(u[IB3 * sn]));
  internal_e /= rho;
  const double internal_e_floor = c.e_floor_town;
  if (internal_e <= internal_e_floor) {  // below the floor: reset
    u[IEN * sn] += rho * (internal_e_floor - internal_e);
    return;
  }
  const double temp = c.mbar_gm1_over_kb * internal_e;
  if (temp < c.temp_cool_floor) return;  // above the floor, below the table: no cooling
  const double n_h2_by_rho = rho * c.X_by_mh2;
  const int nbins = c.n - 1;
  int idx = townsend_bin_up(c, nbins, temp);
  // the temporal evolution function Y(T) (Eq. A5)
  const double alpha_k_m1 = c.alpha_k[idx] - 1.0;
  const double tef = c.Y_k[idx] + (c.lambda_final / c.lambdas[idx]) * (c.temps[idx] / c.temp_final) *
                                      (pow(c.temps[idx] / temp, alpha_k_m1) - 1.0) / alpha_k_m1;
  // the adjusted TEF for the new time step (Eq. 26)
  const double tef_adj = tef + c.lambda_final * dt / c.temp_final * c.mbar_gm1_over_kb * n_h2_by_rho;
  idx = townsend_bin_down(c, idx, tef_adj);
  // the inverse Y^{-1}(Y) (Eq. A7)
  const double temp_new = c.temps[idx] * pow(1 - (1.0 - c.alpha_k[idx]) * (c.lambdas[idx] / c.lambda_final) *
                                                     (c.temp_final / c.temps[idx]) * (tef_adj - c.Y_k[idx]),
                                                 1.0 / (1.0 - c.alpha_k[idx]));
  const double internal_e_new =
      temp_new > c.temp_cool_floor ? temp_new / c.mbar_gm1_over_kb : c.temp_cool_floor / c.mbar_gm1_over_kb;
  u[IEN * sn] += rho * (internal_e_new - internal_e);
}

// EstimateTimeStep (tabular_cooling.cpp:606-665): min over interior cells of the cooling time into min_bits (positive
// doubles and +inf order like their bit patterns)
__global__ void __launch_bounds__(256) cool_dt_kernel(PackView pv, CoolDev c, double gm1, unsigned long long *min_bits,
                                                      unsigned *d_flags) {
  const double *ll = c.log_lambdas;
  int b;
  int64_t off;
  unsigned flags = 0;
  double m = INFINITY;
  if (cell_of(pv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, b, off)) {
    const double *__restrict__ w = pv.blocks[b].prim + off;
    const double rho = w[IDN * pv.sn];
    const double pres = w[IPR * pv.sn];
    const double internal_e = pres / (rho * gm1);
    bool valid = true;
    const double de_dt = dedt(c, ll, internal_e, rho, valid, flags);
    // DeDt 0 (below the table) or below the floor: no limit
    const double cooling_time = ((de_dt == 0) || (internal_e < c.e_floor_sub)) ? INFINITY : fabs(internal_e / de_dt);
    m = cooling_time < m ? cooling_time : m;  // std::min(cooling_time, m)
  }
  latch(d_flags, flags);
  wg_min_to_word(m, min_bits);
}

__global__ void __launch_bounds__(256) cool_dedt_kernel(CoolDev c, const double *e, const double *rho, double *out,
                                                        int *valid, int64_t n, unsigned *d_flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned flags = 0;
  bool v = true;
  out[i] = dedt(c, c.log_lambdas, e[i], rho[i], v, flags);
  valid[i] = v ? 1 : 0;
  latch(d_flags, flags);
}

int64_t interior_cells(const PackView &pv) { return (int64_t)pv.nx1 * pv.nx2 * pv.nx3 * pv.nblocks; }

}  // namespace
}  // namespace apk

struct apk_cooling_table {
  apk::CoolDev dev{};
  double *d_buf = nullptr;
  apk_cooling_params p{};
};

using namespace apk;

extern "C" {

int apk_cooling_table_create(apk_ctx *ctx, const double *log_temps, const double *log_lambdas, int n,
                             const apk_cooling_params *params, apk_cooling_table **out) {
  if (!ctx || !params || !out) return set_err(ctx, APK_ERR_INVALID, "apk_cooling_table_create: bad argument");
  *out = nullptr;
  const apk_cooling_params &p = *params;
  if (p.max_iter < 1) return set_err(ctx, APK_ERR_INVALID, "cooling: max_iter must be >= 1");
  if (!(p.mbar_over_kb > 0.0) || !(p.mh > 0.0) || !(p.gamma > 1.0))
    return set_err(ctx, APK_ERR_INVALID, "cooling: needs units and gas composition (mbar_over_kb, mh) and gamma > 1");
  CoolingTableHost t;
  const std::string err = cooling_table_build(log_temps, log_lambdas, n, p, &t);
  if (!err.empty()) return set_err(ctx, APK_ERR_INVALID, err.c_str());
  auto *tab = new (std::nothrow) apk_cooling_table();
  if (!tab) return set_err(ctx, APK_ERR_INVALID, "apk_cooling_table_create: out of host memory");
  tab->p = p;
  const bool town = p.integrator == APK_COOL_TOWNSEND;
  // one buffer: log_lambdas | lambdas | temps | alpha_k | Y_k
  const size_t nd = (size_t)n + (town ? 2 * (size_t)n + 2 * (size_t)(n - 1) : 0);
  std::vector<double> h(nd);
  std::copy(t.log_lambdas.begin(), t.log_lambdas.end(), h.begin());
  if (town) {
    std::copy(t.lambdas.begin(), t.lambdas.end(), h.begin() + n);
    std::copy(t.temps.begin(), t.temps.end(), h.begin() + 2 * n);
    std::copy(t.alpha_k.begin(), t.alpha_k.end(), h.begin() + 3 * n);
    std::copy(t.Y_k.begin(), t.Y_k.end(), h.begin() + 4 * n - 1);
  }
  if (hipMalloc(&tab->d_buf, nd * sizeof(double)) != hipSuccess ||
      hipMemcpy(tab->d_buf, h.data(), nd * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    apk_cooling_table_destroy(tab);
    return set_err(ctx, APK_ERR_DEVICE, "apk_cooling_table_create: upload failed", hipGetLastError());
  }
  CoolDev &c = tab->dev;
  c.log_lambdas = tab->d_buf;
  if (town) {
    c.lambdas = tab->d_buf + n;
    c.temps = tab->d_buf + 2 * n;
    c.alpha_k = tab->d_buf + 3 * n;
    c.Y_k = tab->d_buf + 4 * n - 1;
    bool mono = true;  // (then bisection returns the linear scans' indices)
    for (int i = 1; i < n; ++i) mono = mono && t.temps[i] > t.temps[i - 1];
    for (int i = 1; i < n - 1; ++i) mono = mono && t.Y_k[i] < t.Y_k[i - 1];
    c.bsearch = mono ? 1 : 0;
  }
  c.n = n;
  c.log_temp_start = t.log_temp_start;
  c.log_temp_final = t.log_temp_final;
  c.d_log_temp = t.d_log_temp;
  const double gm1 = p.gamma - 1.0;
  c.mbar_gm1_over_kb = p.mbar_over_kb * gm1;
  const double x_H = 1.0 - p.He_mass_fraction;
  c.x_H_over_m_h2 = (x_H / p.mh) * (x_H / p.mh);
  c.X_by_mh2 = std::pow((1 - p.He_mass_fraction) / p.mh, 2);
  c.lambda_final = t.lambda_final;
  c.temp_final = std::pow(10.0, t.log_temp_final);
  c.temp_cool_floor = std::pow(10.0, t.log_temp_start);  // low end of the table
  const double temp_floor = (p.T_floor > c.temp_cool_floor) ? p.T_floor : c.temp_cool_floor;
  c.e_floor_sub = temp_floor / c.mbar_gm1_over_kb;
  c.e_floor_town = p.T_floor / c.mbar_gm1_over_kb;
  c.d_e_tol = p.d_e_tol;
  c.max_iter = (unsigned)p.max_iter;
  *out = tab;
  return APK_OK;
}

void apk_cooling_table_destroy(apk_cooling_table *table) {
  if (!table) return;
  if (table->d_buf) (void)hipFree(table->d_buf);
  delete table;
}

int apk_cooling_dedt(apk_ctx *ctx, const apk_cooling_table *table, const double *e, const double *rho, double *dedt_out,
                     int *valid, int64_t n, apk_stream_t stream) {
  if (!ctx || !table || n < 0 || (n > 0 && (!e || !rho || !dedt_out || !valid)))
    return set_err(ctx, APK_ERR_INVALID, "apk_cooling_dedt: bad argument");
  if (n == 0) return APK_OK;
  hipLaunchKernelGGL(cool_dedt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), table->dev, e,
                     rho, dedt_out, valid, n, ctx->d_flags);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "cooling DeDt launch failed");
  return APK_OK;
}

int apk_tabular_cooling_src(apk_ctx *ctx, const apk_pack *md, const apk_cooling_table *table, int fluid, double dt,
                            apk_stream_t stream) {
  if (!ctx || !md || !table) return set_err(ctx, APK_ERR_INVALID, "apk_tabular_cooling_src: bad argument");
  const PackView &v = md->view;
  if ((fluid == APK_FLUID_EULER && v.nhydro != 5) || (fluid == APK_FLUID_GLMMHD && v.nhydro != 9) ||
      (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD))
    return set_err(ctx, APK_ERR_INVALID, "apk_tabular_cooling_src: fluid does not match the pack");
  const int64_t ncell = interior_cells(v);
  if (ncell == 0) return APK_OK;
  const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool mhd = fluid == APK_FLUID_GLMMHD;
  const CoolDev &c = table->dev;
  switch (table->p.integrator) {
    case APK_COOL_RK12:
      if (mhd) hipLaunchKernelGGL((cool_subcycle_kernel<RK12, true>), grid, block, 0, s, v, c, dt, ctx->d_flags);
      else hipLaunchKernelGGL((cool_subcycle_kernel<RK12, false>), grid, block, 0, s, v, c, dt, ctx->d_flags);
      break;
    case APK_COOL_RK45:
      if (mhd) hipLaunchKernelGGL((cool_subcycle_kernel<RK45, true>), grid, block, 0, s, v, c, dt, ctx->d_flags);
      else hipLaunchKernelGGL((cool_subcycle_kernel<RK45, false>), grid, block, 0, s, v, c, dt, ctx->d_flags);
      break;
    case APK_COOL_TOWNSEND:
      if (mhd) hipLaunchKernelGGL(cool_townsend_kernel<true>, grid, block, 0, s, v, c, dt);
      else hipLaunchKernelGGL(cool_townsend_kernel<false>, grid, block, 0, s, v, c, dt);
      break;
    default:
      return set_err(ctx, APK_ERR_INVALID, "Unknown cooling integrator.");
  }
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "cooling source launch failed");
  return APK_OK;
}

int apk_estimate_cooling_timestep(apk_ctx *ctx, const apk_pack *md, const apk_cooling_table *table, double *dt_out,
                                  apk_stream_t stream) {
  if (!ctx || !md || !table || !dt_out) return set_err(ctx, APK_ERR_INVALID, "apk_estimate_cooling_timestep: bad argument");
  const double cfl = table->p.cfl;
  if (cfl <= 0.0) {
    *dt_out = DBL_MAX;
    return APK_OK;
  }
  if (std::isnan(cfl) || std::isinf(cfl)) {
    *dt_out = INFINITY;
    return APK_OK;
  }
  const PackView &v = md->view;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = min_seed(ctx, INFINITY, s);
  if (rc != APK_OK) return rc;
  const int64_t ncell = interior_cells(v);
  if (ncell > 0) {
    const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
    const double gm1 = table->p.gamma - 1.0;
    hipLaunchKernelGGL(cool_dt_kernel, grid, block, 0, s, v, table->dev, gm1, ctx->min_word(), ctx->d_flags);
    if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "cooling time-step launch failed");
  }
  double m;
  if ((rc = min_fetch(ctx, &m, s)) != APK_OK) return rc;
  *dt_out = cfl * m;
  return APK_OK;
}

}  // extern "C"
