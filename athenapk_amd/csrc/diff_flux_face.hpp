// diff_flux_face.hpp -- the diffusive flux through ONE face (the loop bodies of
//   ThermalFluxIsoFixed      conduction.cpp:189-259
//   ThermalFluxGeneral       conduction.cpp:265-471   (lim4 of diffusion.hpp:20-68, upwinded saturated flux; both of its
//                                                     branches, with ThermalDiffusivity::Get of conduction.cpp:28-42)
//   MomentumDiffFluxIsoFixed viscosity.cpp:94-289
//   OhmicDiffFluxIsoFixed    resistivity.cpp:91-230)
// shared by the flux-array pass (kernels_diffusion.hip: one lane per face, read-modify-write of flux[d]) and the fused
// RKL2 sub-stage (kernels_sts.hip: one lane per cell, its 2 ndim faces in registers).  Both callers hand in what the
// face holds so far and get it back with every enabled process added in the reference's order (conduction, viscosity,
// resistivity), so the two paths are the same arithmetic.
#pragma once

#include "apk_internal.hpp"
#include "hydro_math.hpp"

namespace apk {

// conduction modes as CalcDiffFluxes dispatches them (diffusion.cpp:18-53): COND_ISO is ThermalFluxIsoFixed (isotropic
// with a fixed coefficient, no saturation); everything else is ThermalFluxGeneral -- COND_ANISO its anisotropic branch
// (either coefficient), COND_ISO_GEN its isotropic branch (isotropic Spitzer)
enum { COND_NONE = 0, COND_ISO = 1, COND_ANISO = 2, COND_ISO_GEN = 3 };
// ConductionCoeff: what ThermalDiffusivity::Get returns
enum { COEFF_FIXED = 0, COEFF_SPITZER = 1 };

struct DiffCoeffs {
  double kappa;       // thermal_diff_coeff_code; Spitzer: spitzer_cond_in_erg_by_s_K_cm in code units (hydro.cpp:577-581)
  double sat_prefac;  // conduction_sat_prefac (5 phi for a fixed coefficient, 6.86 sqrt(mu) phi for Spitzer, hydro.cpp:589-604)
  double nu;          // mom_diff_coeff_code
  double eta;         // ohm_diff_coeff_code
  double mbar, kb;    // Spitzer only: mu * atomic_mass_unit and k_boltzmann in code units
};

// ThermalDiffusivity::Get (conduction.cpp:28-42): the diffusivity chi of a cell.  T^(5/2) is T * T * sqrt(T), three
// correctly rounded operations, where the reference calls std::pow (whose last bit differs between libraries).
template <int COEFF>
APK_DEV double diff_chi(const DiffCoeffs &c, double pres, double rho) {
  if constexpr (COEFF == COEFF_SPITZER) {
    const double t_cgs = c.mbar / c.kb * pres / rho;
    const double kappa_spitzer = c.kappa * (t_cgs * t_cgs * sqrt(t_cgs));
    return kappa_spitzer * c.mbar / c.kb / rho;
  } else {
    return c.kappa;
  }
}

// the flux components the diffusive processes touch: momenta, the two transverse field components (in increasing
// component order: DIR 0 -> IB2, IB3; DIR 1 -> IB1, IB3; DIR 2 -> IB1, IB2) and the energy
struct DiffFaceFlux {
  double m[3];
  double b[2];
  double e;
};

// limiters::minmod / mc / lim2 / lim4 (diffusion.hpp:20-68), std::min / std::max spelled out
APK_DEV double diff_minmod(double a, double b) {
  if (a * b > 0.0) return (a > 0.0) ? ((b < a) ? b : a) : ((a < b) ? b : a);
  return 0.0;
}
APK_DEV double diff_mc(double a, double b) { return diff_minmod(2.0 * diff_minmod(a, b), (a + b) / 2.0); }
APK_DEV double diff_lim4(double a, double b, double c, double d) { return diff_mc(diff_mc(a, b), diff_mc(c, d)); }

// Face of direction DIR between cell L = R - e_DIR and R; `w` points at the primitives of R (const restrict: the
// compiler shares identical loads between the processes, and between the faces of one cell, since no store precedes
// them).  chiR, chiL: diff_chi of R and of L, read by the general conduction modes only (the caller forms them, so that the
// fused sub-stage evaluates each cell's once; a fixed coefficient hands in c.kappa twice).  f: in, what the face holds;
// out, with the processes added.
template <int DIR, int COND, bool VISC, bool RES>
APK_DEV void diff_face(const double *__restrict__ w, int64_t sn, int64_t sj, int64_t sk, const double (&dx)[3], int ndim,
                       const DiffCoeffs &c, double chiR, double chiL, DiffFaceFlux &f) {
  const int64_t off[3] = {1, sj, sk};
  const int64_t on = off[DIR];  // R - L
  const double dxn = dx[DIR];
  // transverse axes in increasing order (the order the reference adds their terms in)
  constexpr int ta = (DIR == 0) ? 1 : 0;
  constexpr int tb = (DIR == 2) ? 1 : 2;
  const bool act_a = ta < ndim, act_b = tb < ndim;
  const int64_t oa = act_a ? off[ta] : 0, ob = act_b ? off[tb] : 0;
  auto P = [&](int v, int64_t o) { return w[v * sn + o]; };  // o relative to R

  // ---- conduction ------------------------------------------------------------------------------------------------
  double q_cond = 0.0;
  if constexpr (COND == COND_ISO) {
    const double tR = P(IPR, 0) / P(IDN, 0), tL = P(IPR, -on) / P(IDN, -on);
    const double dTdn = (tR - tL) / dxn;
    const double denf = 0.5 * (P(IDN, 0) + P(IDN, -on));
    q_cond = c.kappa * denf * dTdn;  // flux -= q
  } else if constexpr (COND == COND_ANISO || COND == COND_ISO_GEN) {
    auto T = [&](int64_t o) { return P(IPR, o) / P(IDN, o); };
    double g[3];
    g[DIR] = (T(0) - T(-on)) / dxn;
    g[ta] = act_a ? diff_lim4(T(oa) - T(0), T(0) - T(-oa), T(-on + oa) - T(-on), T(-on) - T(-on - oa)) / dx[ta] : 0.0;
    g[tb] = act_b ? diff_lim4(T(ob) - T(0), T(0) - T(-ob), T(-on + ob) - T(-on), T(-on) - T(-on - ob)) / dx[tb] : 0.0;
    const double denf = 0.5 * (P(IDN, 0) + P(IDN, -on));
    const double tdf = 0.5 * (chiR + chiL);
    double fc, fcm;  // flux_classic, flux_classic_mag
    if constexpr (COND == COND_ANISO) {
      const double bx = 0.5 * (P(IB1, -on) + P(IB1, 0));
      const double by = 0.5 * (P(IB2, -on) + P(IB2, 0));
      const double bz = ndim >= 3 ? 0.5 * (P(IB3, -on) + P(IB3, 0)) : 0.0;
      double bmag = sqrt(bx * bx + by * by + bz * bz);
      bmag = (bmag < kTiny) ? kTiny : bmag;
      const double bn = (DIR == 0 ? bx : (DIR == 1 ? by : bz)) / bmag;
      const double bdg = (bx * g[0] + by * g[1] + bz * g[2]) / bmag;
      fc = -tdf * denf * bdg * bn;
      fcm = fabs(tdf * denf * bdg);
    } else {
      const double gmag = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
      fc = -tdf * denf * g[DIR];
      fcm = tdf * denf * gmag;
    }
    const double pL = P(IPR, -on), pR = P(IPR, 0);
    double fsat;
    if (fc > 0.0) {
      fsat = c.sat_prefac * sqrt(pL / denf) * pL;
    } else if (fc < 0.0) {
      fsat = c.sat_prefac * sqrt(pR / denf) * pR;
    } else {
      const double presf = 0.5 * (pR + pL);
      fsat = c.sat_prefac * sqrt(presf / denf) * presf;
    }
    q_cond = (fsat / (fsat + fcm)) * fc;  // flux += q
  }
  // ---- viscosity -------------------------------------------------------------------------------------------------
  double fv[3] = {0.0, 0.0, 0.0}, nud = 0.0, q_visc = 0.0;
  if constexpr (VISC) {
    constexpr int vn = IV1 + DIR, va = IV1 + ta, vb = IV1 + tb;
    // normal component: 4/3 d vn/dn - 2/3 (d va/da + d vb/db); transverse: d vt/dn + d vn/dt
    auto tsum = [&](int v, int64_t o) { return (P(v, o) + P(v, o - on)) - (P(v, -o) + P(v, -o - on)); };
    fv[DIR] = 4.0 * (P(vn, 0) - P(vn, -on)) / (3.0 * dxn);
    fv[ta] = (P(va, 0) - P(va, -on)) / dxn;
    fv[tb] = (P(vb, 0) - P(vb, -on)) / dxn;
    if (act_a) {
      fv[DIR] -= tsum(va, oa) / (6.0 * dx[ta]);
      fv[ta] += tsum(vn, oa) / (4.0 * dx[ta]);
    }
    if (act_b) {
      fv[DIR] -= tsum(vb, ob) / (6.0 * dx[tb]);
      fv[tb] += tsum(vn, ob) / (4.0 * dx[tb]);
    }
    nud = 0.5 * c.nu * (P(IDN, 0) + P(IDN, -on));
    q_visc = 0.5 * nud *
             ((P(IV1, -on) + P(IV1, 0)) * fv[0] + (P(IV2, -on) + P(IV2, 0)) * fv[1] + (P(IV3, -on) + P(IV3, 0)) * fv[2]);
  }
  // ---- Ohmic resistivity -----------------------------------------------------------------------------------------
  double fb[2] = {0.0, 0.0}, q_res = 0.0;  // the two transverse field fluxes, in increasing component order
  if constexpr (RES) {
    const double eta = c.eta;
    auto dn = [&](int v) { return (P(v, 0) - P(v, -on)) / dxn; };
    auto dt = [&](int v, int t, bool act, int64_t o) {
      return act ? (0.5 * (P(v, o - on) + P(v, o)) - 0.5 * (P(v, -o - on) + P(v, -o))) / (2.0 * dx[t]) : 0.0;
    };
    auto bs = [&](int v) { return P(v, -on) + P(v, 0); };
    if constexpr (DIR == 0) {
      const double j2 = dt(IB1, 2, act_b, ob) - dn(IB3);  // d3B1 - d1B3
      const double j3 = dn(IB2) - dt(IB1, 1, act_a, oa);  // d1B2 - d2B1
      fb[0] = -eta * j3;                                  // IB2
      fb[1] = eta * j2;                                   // IB3
      q_res = 0.5 * eta * (bs(IB3) * j2 - bs(IB2) * j3);
    } else if constexpr (DIR == 1) {
      const double j3 = dt(IB2, 0, act_a, oa) - dn(IB1);  // d1B2 - d2B1
      const double j1 = dn(IB3) - dt(IB2, 2, act_b, ob);  // d2B3 - d3B2
      fb[0] = eta * j3;                                   // IB1
      fb[1] = -eta * j1;                                  // IB3
      q_res = 0.5 * eta * (bs(IB1) * j3 - bs(IB3) * j1);
    } else {
      const double j1 = dt(IB3, 1, act_b, ob) - dn(IB2);  // d2B3 - d3B2
      const double j2 = dn(IB1) - dt(IB3, 0, act_a, oa);  // d3B1 - d1B3
      fb[0] = -eta * j2;                                  // IB1
      fb[1] = eta * j1;                                   // IB2
      q_res = 0.5 * eta * (bs(IB2) * j1 - bs(IB1) * j2);
    }
  }
  // ---- accumulate into the face flux in the reference's order ---------------------------------------------------
  if constexpr (VISC) {
    f.m[0] -= nud * fv[0];
    f.m[1] -= nud * fv[1];
    f.m[2] -= nud * fv[2];
  }
  if constexpr (RES) {
    f.b[0] += fb[0];
    f.b[1] += fb[1];
  }
  if constexpr (COND != COND_NONE || VISC || RES) {
    double e = f.e;
    if constexpr (COND == COND_ISO) e -= q_cond;
    if constexpr (COND == COND_ANISO || COND == COND_ISO_GEN) e += q_cond;
    if constexpr (VISC) e -= q_visc;
    if constexpr (RES) e += q_res;
    f.e = e;
  }
}

// What the launchers make of (apk_conduction, fixed coefficient | apk_spitzer_cfg): the coefficients, the coefficient kind
// and the kernels' conduction mode.  Isotropic conduction takes the general path only with Spitzer (diffusion.cpp:18-53).
inline int diff_coeff_kind(int cond, const apk_spitzer_cfg *spitzer) {
  return (cond != COND_NONE && spitzer) ? COEFF_SPITZER : COEFF_FIXED;
}
inline int diff_cond_mode(int cond, const apk_spitzer_cfg *spitzer) {
  return (cond == COND_ISO && spitzer) ? COND_ISO_GEN : cond;
}
inline DiffCoeffs diff_coeffs(int cond, double kappa, double sat_prefac, double nu, double eta, const apk_spitzer_cfg *spitzer) {
  if (diff_coeff_kind(cond, spitzer) == COEFF_SPITZER)
    return DiffCoeffs{spitzer->coeff_code, sat_prefac, nu, eta, spitzer->mbar, spitzer->k_boltzmann};
  return DiffCoeffs{kappa, sat_prefac, nu, eta, 0.0, 0.0};
}

// blocks per launch: grid z = (planes per block) x (blocks) stays within the 65535 a grid dimension may hold
inline int blocks_per_launch(int planes) { return planes > 0 ? (65535 / planes > 0 ? 65535 / planes : 1) : 1; }

}  // namespace apk
