// feedback_math.hpp -- the pointwise geometry of the cluster problem's AGN feedback, shared by the host model
// (host/feedback_model.cpp, plain C++) and the kernels (kernels_feedback.hip): one text, so that the host's initial
// field, the tower source and a numpy restatement run the same IEEE operations in the same order.
//   JetCoords::SimCartToJetCylCoords, JetCylToSimCartVector     src/pgen/cluster/jet_coords.hpp:39-84
//   MagneticTowerObj::PotentialInJetCyl / PotentialInSimCart      src/pgen/cluster/magnetic_tower.hpp:60-102
//   MagneticTowerObj::FieldInJetCyl / FieldInSimCart              magnetic_tower.hpp:104-146
//   MagneticTowerObj::DensityFromSimCart                          magnetic_tower.hpp:148-158
// Deliberate deviation: where the reference writes pow(x, 2) (jet_coords.hpp:56, the tower's pow(r / l, 2)) this writes
// x * x, so that host, device and numpy agree operation for operation; exp is the one step that is not correctly rounded.
#pragma once

#include <cmath>

#include "../../include/apk_amd.h"

#if defined(__HIPCC__)
#define APK_HD __host__ __device__ inline
#else
#define APK_HD inline
#endif

namespace apk {

// position (x, y, z) of the simulation frame in the jet's cylindrical coordinates
APK_HD void sim_cart_to_jet_cyl(const apk_jet_coords &jc, double x, double y, double z, double &r, double &cos_t, double &sin_t,
                                double &h) {
  const double x_jet = x * jc.cos_phi * jc.cos_theta + y * jc.sin_phi * jc.cos_theta - z * jc.sin_theta;
  const double y_jet = -x * jc.sin_phi + y * jc.cos_phi;
  const double z_jet = x * jc.sin_theta * jc.cos_phi + y * jc.sin_phi * jc.sin_theta + z * jc.cos_theta;
  r = sqrt(fabs(x_jet) * fabs(x_jet) + fabs(y_jet) * fabs(y_jet));
  // (on the axis both are 0: every user multiplies them with a component that vanishes there)
  cos_t = (r != 0) ? x_jet / r : 0;
  sin_t = (r != 0) ? y_jet / r : 0;
  h = z_jet;
}

// vector (v_r, v_theta, v_h) of the jet's cylindrical frame in the simulation frame
APK_HD void jet_cyl_to_sim_cart_vector(const apk_jet_coords &jc, double cos_t, double sin_t, double v_r, double v_theta, double v_h,
                                       double &v_x, double &v_y, double &v_z) {
  const double v_x_jet = v_r * cos_t - v_theta * sin_t;
  const double v_y_jet = v_r * sin_t + v_theta * cos_t;
  const double v_z_jet = v_h;
  v_x = v_x_jet * jc.cos_phi * jc.cos_theta - v_y_jet * jc.sin_phi + v_z_jet * jc.sin_theta * jc.cos_phi;
  v_y = v_x_jet * jc.sin_phi * jc.cos_theta + v_y_jet * jc.cos_phi + v_z_jet * jc.sin_phi * jc.sin_theta;
  v_z = -v_x_jet * jc.sin_theta + v_z_jet * jc.cos_theta;
}

// the tower's vector potential at field strength `field`
APK_HD void tower_potential(const apk_magnetic_tower_cfg &t, const apk_jet_coords &jc, double field, double x, double y, double z,
                            double &a_x, double &a_y, double &a_z) {
  double r, cos_t, sin_t, h;
  sim_cart_to_jet_cyl(jc, x, y, z, r, cos_t, sin_t, h);
  double a_theta = 0.0, a_h = 0.0;
  if (t.potential == APK_TOWER_DONUT) {
    const double rl = r / t.l_scale;
    const double e = exp(-(rl * rl));
    if (fabs(h) >= t.donut_offset && fabs(h) <= t.donut_offset + t.donut_thickness) a_h = field * t.l_scale * e;
  } else {  // APK_TOWER_LI
    const double rl = r / t.l_scale, hl = h / t.l_scale;
    const double e = exp(-(rl * rl) - hl * hl);
    a_theta = field * t.l_scale * (r / t.l_scale) * e;
    a_h = field * t.l_scale * t.li_alpha / 2.0 * e;
  }
  jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, 0.0, a_theta, a_h, a_x, a_y, a_z);
}

// the tower's analytic field at field strength `field`
APK_HD void tower_field(const apk_magnetic_tower_cfg &t, const apk_jet_coords &jc, double field, double x, double y, double z,
                        double &b_x, double &b_y, double &b_z) {
  double r, cos_t, sin_t, h;
  sim_cart_to_jet_cyl(jc, x, y, z, r, cos_t, sin_t, h);
  double b_r = 0.0, b_theta = 0.0, b_h = 0.0;
  if (t.potential == APK_TOWER_DONUT) {
    const double rl = r / t.l_scale;
    const double e = exp(-(rl * rl));
    if (fabs(h) >= t.donut_offset && fabs(h) <= t.donut_offset + t.donut_thickness) b_theta = 2.0 * field * r / t.l_scale * e;
  } else {
    const double rl = r / t.l_scale, hl = h / t.l_scale;
    const double e = exp(-(rl * rl) - hl * hl);
    b_r = field * 2 * (h / t.l_scale) * (r / t.l_scale) * e;
    b_theta = field * t.li_alpha * (r / t.l_scale) * e;
    b_h = field * 2 * (1 - rl * rl) * e;
  }
  jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, b_r, b_theta, b_h, b_x, b_y, b_z);
}

// the Gaussian density the tower injects with its field
APK_HD double tower_density(const apk_magnetic_tower_cfg &t, const apk_jet_coords &jc, double density, double x, double y,
                            double z) {
  double r, cos_t, sin_t, h;
  sim_cart_to_jet_cyl(jc, x, y, z, r, cos_t, sin_t, h);
  return density * exp(-(r * r + h * h) / (t.l_mass_scale * t.l_mass_scale));
}

}  // namespace apk
