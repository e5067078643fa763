// feedback.hpp -- the host-side model of the cluster problem's fixed-power AGN feedback, free of the driver: the
// precessing jet frame (src/pgen/cluster/jet_coords.hpp), AGNFeedback's constructor and the numbers its source term
// computes per stage (cluster/agn_feedback.cpp:34-185, 187-212, 263-303), the magnetic tower's power scaling
// (cluster/magnetic_tower.cpp:258-292) and its initial field (magnetic_tower.cpp:206-235, cluster.cpp:556-625),
// restated in the reference's operation order.  Plain C++ (host/feedback_model.cpp): a stand-alone program can link it.
#pragma once

#include <string>

#include "../../../include/apk_amd.h"

namespace apk {

// JetCoordsFactory::CreateJetCoords(time) (jet_coords.hpp:109-111)
apk_jet_coords jet_coords_at(double jet_theta, double jet_phi_dot, double jet_phi0, double time);

// what AGNFeedback's constructor reads (code units; has_* = the key is in the deck)
struct AgnFeedbackInput {
  double fixed_power = 0.0, efficiency = 1e-3;
  double thermal_fraction = 0.0, kinetic_fraction = 0.0, magnetic_fraction = 0.0;
  bool enable_magnetic_tower_mass_injection = true;
  double thermal_radius = 0.01, kinetic_jet_radius = 0.01, kinetic_jet_thickness = 0.02, kinetic_jet_offset = 0.02;
  bool has_velocity = false, has_temperature = false;
  double kinetic_jet_velocity = 0.0, kinetic_jet_temperature = 0.0;
  double vceil = 0.0, Tceil = 0.0;  // (+inf: none)
  double speed_of_light = 0.0, mbar_gm1_over_kb = 0.0;  // Units::speed_of_light(), mbar_over_kb * (gamma - 1)
};
// ... and what it derives.  A violated PARTHENON_REQUIRE throws std::runtime_error with the reference's wording.
struct AgnFeedbackModel {
  AgnFeedbackInput in;
  double thermal_fraction = 0, kinetic_fraction = 0, magnetic_fraction = 0;  // normalised to sum 1
  double thermal_mass_fraction = 0, kinetic_mass_fraction = 0, magnetic_mass_fraction = 0;
  double kinetic_jet_velocity = 0, kinetic_jet_temperature = 0, kinetic_jet_e = 0, eceil = 0;
  bool assumed_cold_jet = false;  // neither velocity nor temperature given (the reference prints a warning)
  // GetFeedbackPower / GetFeedbackMassRate (agn_feedback.cpp:187-212) with the accretion rate of AGN triggering (0
  // without it): fixed_power + mdot * efficiency * c^2 and mdot * (1 - efficiency) + fixed_power / (efficiency * c^2)
  double accretion_rate = 0;
  double power() const;
  double mass_rate() const;
};
AgnFeedbackModel agn_feedback_model(const AgnFeedbackInput &in);
// the numbers of agn_feedback.cpp:263-303 for one stage
apk_agn_feedback_cfg agn_feedback_stage_numbers(const AgnFeedbackModel &m, double beta_dt);

// MagneticTower::PowerSrcTerm's field_to_add (magnetic_tower.cpp:270-288); its two PARTHENON_FAILs throw
double tower_field_to_add(double linear_contrib, double quadratic_contrib, double beta_dt, double power);
// AddSrcTerm's density_to_add (magnetic_tower.cpp:55-61); the PARTHENON_REQUIRE_THROWS throws
double tower_density_to_add(double mass_to_add, double l_mass_scale);
// MagneticTower's constructor checks (magnetic_tower.hpp:194-207) and MagneticTowerObj's (magnetic_tower.hpp:53-57); throw
void tower_check_combination(const apk_magnetic_tower_cfg &t);
void tower_check_scales(const apk_magnetic_tower_cfg &t);

// The initial field of one block (cluster.cpp:556-625 with magnetic_tower.cpp:206-235): the potential at field strength
// `field` on the cell centres x1[n1 + 2], x2[n2 + 2], x3[n3 + 2] (the interior plus one cell each side) and its
// central-difference curl on the interior, b[3][n3][n2][n1]
void tower_initial_field_block(const apk_magnetic_tower_cfg &t, const apk_jet_coords &jc, double field, const double *x1, int n1,
                               const double *x2, int n2, const double *x3, int n3, const double dx[3], double *b);

// AGNTriggering (agn_triggering.{hpp,cpp}) on already reduced quantities, in the reference's operation order
struct AgnTriggeringModel {
  int mode = APK_TRIG_NONE;
  double accretion_radius = 0, cold_temp_thresh = 0, cold_t_acc = 0, bondi_alpha = 0, bondi_M_smbh = 0, bondi_n0 = 0, bondi_beta = 0;
  double accretion_cfl = 1e-1;
  bool remove_accreted_mass = true;
  double mean_molecular_mass = 0;        // mu * atomic_mass_unit (agn_triggering.cpp:75-78)
  double mean_molecular_mass_by_kb = 0;  // mean_molecular_mass / k_boltzmann (agn_triggering.cpp:149)
  double gravitational_constant = 0;     // Units::gravitational_constant()
  // the reduced quantities (the "agn_triggering_*" params): COLD_GAS reads cold_mass, the Bondi-like modes the four sums
  struct Reduced {
    double cold_mass = 0, total_mass = 0, mass_weighted_density = 0, mass_weighted_velocity = 0, mass_weighted_cs = 0;
  };
  // GetAccretionRate (agn_triggering.cpp:319-365)
  double accretion_rate(const Reduced &q) const;
  // EstimateTimeStep (agn_triggering.cpp:556-584); numeric_limits<double>::max() where there is no limit
  double estimate_timestep(const Reduced &q) const;
};
// ParseAGNTriggeringMode (agn_triggering.cpp:34-51); throws with the reference's wording
int parse_agn_triggering_mode(const std::string &mode_str);

// The active list of one block and one direction: the range [lo, hi) of extended indices (0 .. n_ext - 1; the first
// interior cell is `first`) whose centres x[i] can satisfy |x| < radius, widened by one cell per side and clipped to the
// block's arrays.  x[n_ext]: the centres of the extended cells.  lo >= hi: no cell.
void triggering_index_range(const double *x, int n_ext, double radius, int *lo, int *hi);

}  // namespace apk
