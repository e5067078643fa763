// cluster.cpp -- problem_id = cluster in the standalone host driver: the options of ProblemInitPackageData
// (src/pgen/cluster.cpp:114-250) for the slice built here, what is refused of the rest, the problem generator
// (cluster.cpp:469-653), the per-block origins of the gravity and feedback sources, the feedback sources of a stage
// (cluster.cpp:76-80), AGN triggering's options, active list and cycle (agn_triggering.cpp, hydro_driver.cpp:360-394) and the C entries of include/apk_host.h.  The model itself is host/cluster_model.cpp (ClusterGravity,
// ACCEPTEntropyProfile, HydrostaticEquilibriumSphere) and host/feedback_model.cpp (the jet frame, AGNFeedback's derived
// numbers, the magnetic tower's scaling and initial field).
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <limits>

#include "cluster.hpp"
#include "cluster_sources.hpp"
#include "sim_internal.hpp"

namespace apk {

// Units (src/units.hpp:20-47, 99-133): the constants the cluster problem converts its defaults with
namespace {
namespace cgs {
constexpr double kev = 1.60218e-9;                     // erg
constexpr double km_s = 1e5;                           // cm / s
constexpr double kpc = 3.0856775809623245e+21;         // cm
constexpr double mpc = 3.0856775809623245e+24;         // cm
constexpr double msun = 1.98841586e+33;                // g
constexpr double gravitational_constant = 6.67408e-08;  // cm^3 / (g s^2)
}  // namespace cgs
}  // namespace
double UnitsState::gravitational_constant() const {
  return cgs::gravitational_constant / (std::pow(code_length_cgs, 3) / (code_mass_cgs * std::pow(code_time_cgs, 2)));
}
double UnitsState::msun() const { return cgs::msun / code_mass_cgs; }
double UnitsState::kpc() const { return cgs::kpc / code_length_cgs; }
double UnitsState::mpc() const { return cgs::mpc / code_length_cgs; }
double UnitsState::km_s() const { return cgs::km_s / (code_length_cgs / code_time_cgs); }
double UnitsState::kev() const { return cgs::kev / code_energy_cgs(); }
double UnitsState::g() const { return 1.0 / code_mass_cgs; }
double UnitsState::speed_of_light() const { return 2.99792458e10 / (code_length_cgs / code_time_cgs); }

namespace host {

namespace {

const char *kGrav = "problem/cluster/gravity";
const char *kHse = "problem/cluster/hydrostatic_equilibrium";
const char *kAgn = "problem/cluster/agn_feedback";
const char *kTower = "problem/cluster/magnetic_tower";
const char *kJet = "problem/cluster/precessing_jet";
const char *kTrig = "problem/cluster/agn_triggering";
const char *kSnia = "problem/cluster/snia_feedback";
const char *kStellar = "problem/cluster/stellar_feedback";
const char *kClips = "problem/cluster/clips";

[[noreturn]] void refuse(const std::string &key, const std::string &why) {
  throw std::runtime_error("problem_id = cluster: " + key + " " + why);
}

// what the cluster generator would do and this path does not: refused, never ignored
void refuse_unbuilt(apk_sim *s) {
  ParameterInput &pin = s->pin;
  if (pin.GetOrAddString("parthenon/mesh", "refinement", "none") != "none")
    refuse("parthenon/mesh/refinement", "must be none: the cluster problem runs on uniform meshes only (static refinement included)");
  if (s->mesh.nx[2] == 1) refuse("parthenon/mesh/nx3", "= 1: the cluster problem is three-dimensional");
  if (s->mesh.nx[1] == 1) refuse("parthenon/mesh/nx2", "= 1: the cluster problem is three-dimensional");
  if (pin.GetOrAddBoolean(kAgn, "enable_tracer", false))
    refuse("problem/cluster/agn_feedback/enable_tracer", "must be false: the AGN passive-scalar tag is not implemented");
  if (pin.GetOrAddReal("problem/cluster/init_perturb", "sigma_v", 0.0) != 0.0)
    refuse("problem/cluster/init_perturb/sigma_v", "must be 0: initial velocity perturbations are not implemented");
  if (pin.GetOrAddReal("problem/cluster/init_perturb", "sigma_b", 0.0) != 0.0)
    refuse("problem/cluster/init_perturb/sigma_b", "must be 0: initial field perturbations are not implemented");
  if (pin.GetOrAddBoolean("problem/cluster/dipole_b_field", "init_dipole_b_field", false))
    refuse("problem/cluster/dipole_b_field/init_dipole_b_field", "must be false: the dipole field is not implemented");
  if (pin.DoesBlockExist("problem/cluster/reductions"))
    refuse("problem/cluster/reductions", "is not implemented: remove the block");
}

HeSphere sphere_of(const apk_cluster_options &o) {
  HeSphere sp;
  sp.gravity = o.gravity;
  sp.k_0 = o.k_0, sp.k_100 = o.k_100, sp.r_k = o.r_k, sp.alpha_k = o.alpha_k;
  sp.mh = o.mh, sp.k_boltzmann = o.k_boltzmann, sp.mu = o.mu, sp.mu_e = o.mu_e;
  sp.r_fix = o.r_fix, sp.rho_fix = o.rho_fix, sp.r_sampling = o.r_sampling;
  return sp;
}

// the block's own radial mesh (generate_P_rho_profile(ib, jb, kb, coords)), cell centres from xc()
HeProfile block_profile(apk_sim *s, int lb) {
  LevelDxScope level_dx_scope(s, lb);
  const Mesh &m = s->mesh;
  double x0[3];
  block_origin(s, lb, x0);
  std::vector<double> x1, x2, x3;
  for (int i = m.is; i <= m.ie; ++i) x1.push_back(xc(s, x0, 0, i));
  for (int j = m.js; j <= m.je; ++j) x2.push_back(xc(s, x0, 1, j));
  for (int k = m.ks; k <= m.ke; ++k) x3.push_back(xc(s, x0, 2, k));
  return he_generate_block_profile(sphere_of(s->cluster), x1.data(), (int)x1.size(), x2.data(), (int)x2.size(), x3.data(),
                                   (int)x3.size(), s->dx);
}

bool sphere_available(const apk_sim *s) { return s->cluster.enabled && s->pkg.units.has_composition; }

// AGNTriggering as the reference's constructor reads it (agn_triggering.cpp:53-119), what this path refuses of it, and
// the active list of this rank's blocks (include/apk_amd.h: apk_trig_box)
void triggering_active_list(apk_sim *s) {
  const Mesh &m = s->mesh;
  s->trig_boxes.clear();
  s->trig_box_cells = s->trig_max_box_cells = 0;
  const int next[3] = {m.ni, m.nj, m.nk};
  for (int lb = 0; lb < (int)m.local_gids.size(); ++lb) {
    double x0[3];
    block_origin(s, lb, x0);
    apk_trig_box box{};
    box.block = lb;
    long long cells = 1;
    for (int d = 0; d < 3; ++d) {
      std::vector<double> x((size_t)next[d]);
      for (int i = 0; i < next[d]; ++i) x[(size_t)i] = xc(s, x0, d, i);
      triggering_index_range(x.data(), next[d], s->trig.accretion_radius, &box.lo[d], &box.hi[d]);
      cells *= std::max(box.hi[d] - box.lo[d], 0);
    }
    if (cells == 0) continue;
    s->trig_boxes.push_back(box);
    s->trig_box_cells += cells;
    s->trig_max_box_cells = std::max(s->trig_max_box_cells, cells);
  }
}

void triggering_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  const UnitsState &u = s->pkg.units;
  AgnTriggeringModel &t = s->trig;
  t = AgnTriggeringModel{};
  s->trig_q = AgnTriggeringModel::Reduced{};
  s->trig_rate = s->trig_time = s->trig_dt = 0.0;
  const std::string mode_key = std::string(kTrig) + "/triggering_mode";
  t.mode = parse_agn_triggering_mode(pin.GetOrAddString(kTrig, "triggering_mode", "NONE"));
  t.accretion_radius = pin.GetOrAddReal(kTrig, "accretion_radius", 0);
  t.cold_temp_thresh = pin.GetOrAddReal(kTrig, "cold_temp_thresh", 0);
  t.cold_t_acc = pin.GetOrAddReal(kTrig, "cold_t_acc", 0);
  t.bondi_alpha = pin.GetOrAddReal(kTrig, "bondi_alpha", 0);
  t.bondi_M_smbh = pin.GetOrAddReal(kGrav, "m_smbh", 0);
  t.bondi_n0 = pin.GetOrAddReal(kTrig, "bondi_n0", 0);
  t.bondi_beta = pin.GetOrAddReal(kTrig, "bondi_beta", 0);
  t.accretion_cfl = pin.GetOrAddReal(kTrig, "accretion_cfl", 1e-1);
  t.remove_accreted_mass = pin.GetOrAddBoolean(kTrig, "removed_accreted_mass", true);
  s->trig_write_to_file = pin.GetOrAddBoolean(kTrig, "write_to_file", false);
  s->trig_filename = pin.GetOrAddString(kTrig, "triggering_filename", "agn_triggering.dat");
  t.gravitational_constant = u.gravitational_constant();
  if (u.has_composition) {
    t.mean_molecular_mass = u.mu * u.atomic_mass_unit();
    t.mean_molecular_mass_by_kb = t.mean_molecular_mass / u.k_boltzmann();
  }
  if (!(t.accretion_cfl > 0.0)) refuse(std::string(kTrig) + "/accretion_cfl", "must be positive");
  s->pkg.agn_triggering = t.mode != APK_TRIG_NONE;
  if (t.mode == APK_TRIG_NONE) return;
  // (stricter than the reference, where an empty sphere gives 0 / 0 and a zero accretion time a zero time step and an
  // infinite rate)
  if (!(t.accretion_radius > 0.0)) refuse(mode_key, "other than NONE needs " + std::string(kTrig) + "/accretion_radius > 0");
  if (t.mode == APK_TRIG_COLD_GAS && !(t.cold_t_acc > 0.0)) refuse(mode_key, "= COLD_GAS needs " + std::string(kTrig) + "/cold_t_acc > 0");
  if (t.mode == APK_TRIG_BOOTH_SCHAYE && !(t.bondi_n0 > 0.0)) refuse(std::string(kTrig) + "/bondi_n0", "must be positive with triggering_mode = BOOTH_SCHAYE");
  if (!u.has_composition)
    refuse(mode_key, "other than NONE requires units and gas composition. Set a 'units' block and 'hydro/He_mass_fraction' in the "
           "input file.");
  if (s->pkg.diffint == APK_DIFFINT_RKL2) refuse(mode_key, "other than NONE is not supported with diffusion/integrator = rkl2");
  triggering_active_list(s);
}

// the interior index box, in the block's extended index space, of the cells of every local block that can lie within
// `radius` of the origin: the active list of the split sources (include/apk_amd.h: apk_trig_box)
void split_active_list(apk_sim *s, double radius) {
  const Mesh &m = s->mesh;
  s->split_boxes.clear();
  s->split_box_cells = s->split_max_box_cells = 0;
  const int first[3] = {m.is, m.js, m.ks}, nint[3] = {m.ie - m.is + 1, m.je - m.js + 1, m.ke - m.ks + 1};
  for (int lb = 0; lb < (int)m.local_gids.size(); ++lb) {
    double x0[3];
    block_origin(s, lb, x0);
    apk_trig_box box{};
    box.block = lb;
    long long cells = 1;
    for (int d = 0; d < 3; ++d) {
      std::vector<double> x((size_t)nint[d]);
      for (int i = 0; i < nint[d]; ++i) x[(size_t)i] = xc(s, x0, d, first[d] + i);
      split_index_range(x.data(), nint[d], first[d], radius, &box.lo[d], &box.hi[d]);
      cells *= std::max(box.hi[d] - box.lo[d], 0);
    }
    if (cells == 0) continue;
    s->split_boxes.push_back(box);
    s->split_box_cells += cells;
    s->split_max_box_cells = std::max(s->split_max_box_cells, cells);
  }
}

// SNIAFeedback, StellarFeedback and the clips as the reference reads them (snia_feedback.cpp:31-48,
// stellar_feedback.cpp:32-65, cluster.cpp:250-277); the derivations and refusals are host/cluster_sources_model.cpp's
void sources_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  const UnitsState &u = s->pkg.units;
  const double inf = std::numeric_limits<double>::infinity();
  ClusterSourcesInput in;
  in.power_per_bcg_mass = pin.GetOrAddReal(kSnia, "power_per_bcg_mass", 0.0);
  in.mass_rate_per_bcg_mass = pin.GetOrAddReal(kSnia, "mass_rate_per_bcg_mass", 0.0);
  in.snia_disabled = pin.GetOrAddBoolean(kSnia, "disabled", false);
  in.stellar_radius = pin.GetOrAddReal(kStellar, "stellar_radius", 0.0);
  in.exclusion_radius = pin.GetOrAddReal(kStellar, "exclusion_radius", 0.0);
  in.efficiency = pin.GetOrAddReal(kStellar, "efficiency", 0.0);
  in.number_density_threshold = pin.GetOrAddReal(kStellar, "number_density_threshold", 0.0);
  in.temperature_threshold = pin.GetOrAddReal(kStellar, "temperature_threshold", 0.0);
  in.accretion_radius = pin.GetOrAddReal(kTrig, "accretion_radius", 0);
  in.clip_r = pin.GetOrAddReal(kClips, "clip_r", -1.0);
  in.dfloor = pin.GetOrAddReal(kClips, "dfloor", -1.0);
  in.vceil = pin.GetOrAddReal(kClips, "vceil", inf);
  in.vAceil = pin.GetOrAddReal(kClips, "vAceil", inf);
  in.Tceil = pin.GetOrAddReal(kClips, "Tceil", inf);
  in.which_bcg_g = s->cluster.which_bcg_g, in.m_bcg_s = s->cluster.m_bcg_s, in.r_bcg_s = s->cluster.r_bcg_s;
  in.mhd = s->pkg.fluid == APK_FLUID_GLMMHD, in.rkl2 = s->pkg.diffint == APK_DIFFINT_RKL2, in.has_composition = u.has_composition;
  in.gamma = s->pkg.eos.gamma;
  if (u.has_composition) in.mu = u.mu, in.mh = u.mh(), in.mbar_over_kb = u.mbar_over_kb, in.speed_of_light = u.speed_of_light();
  s->snia = apk_snia_cfg{}, s->stellar = apk_stellar_cfg{}, s->clips = apk_clips_cfg{};
  for (double &t : s->split_totals) t = 0.0;
  apk_cluster_source_options &o = s->csrc;
  o = cluster_source_options(in);  // (throws what is refused)
  if (o.snia_active) {
    s->snia.power_per_bcg_mass = o.power_per_bcg_mass, s->snia.mass_rate_per_bcg_mass = o.mass_rate_per_bcg_mass;
    s->snia.rho_const_bcg = o.rho_const_bcg, s->snia.r_bcg_s = s->cluster.r_bcg_s, s->snia.smoothing_r = s->cluster.g_smoothing_radius;
  }
  if (o.stellar_active) {
    s->stellar.stellar_radius = o.stellar_radius, s->stellar.exclusion_radius = o.exclusion_radius;
    s->stellar.number_density_threshold = o.number_density_threshold, s->stellar.temperature_threshold = o.temperature_threshold;
    s->stellar.mbar = o.mbar, s->stellar.mbar_over_kb = o.mbar_over_kb, s->stellar.mass_to_energy = o.mass_to_energy;
  }
  if (o.clips_active)
    s->clips.clip_r = o.clip_r, s->clips.dfloor = o.dfloor, s->clips.vceil = o.vceil, s->clips.vAceil = o.vAceil, s->clips.eceil = o.eceil;
  s->pkg.snia_srcterm = o.snia_active != 0;
  s->pkg.cluster_split_srcterm = o.stellar_active || o.clips_active;
  s->split_boxes.clear();
  s->split_box_cells = s->split_max_box_cells = 0;
  if (s->pkg.cluster_split_srcterm)
    split_active_list(s, std::max(o.stellar_active ? o.stellar_radius : 0.0, o.clips_active ? o.clip_r : 0.0));
  o.active_blocks = (int)s->split_boxes.size(), o.active_box_cells = s->split_box_cells;
}

// AGNFeedback, MagneticTower and JetCoordsFactory as the reference's constructors read them (agn_feedback.cpp:34-185,
// magnetic_tower.hpp:178-219, jet_coords.hpp:100-107), and what this path refuses of them
void feedback_initialize(apk_sim *s, bool agn_block, bool tower_block) {
  ParameterInput &pin = s->pin;
  const UnitsState &u = s->pkg.units;
  const double inf = std::numeric_limits<double>::infinity();
  apk_agn_feedback_options &o = s->agn_opt;
  o = apk_agn_feedback_options{};
  const bool mhd = s->pkg.fluid == APK_FLUID_GLMMHD;

  o.jet_theta = pin.GetOrAddReal(kJet, "jet_theta", 0.0);
  o.jet_phi_dot = pin.GetOrAddReal(kJet, "jet_phi_dot", 0.0);
  o.jet_phi0 = pin.GetOrAddReal(kJet, "jet_phi0", 0.0);

  // the tower first: AGN feedback's refusals look at it
  apk_magnetic_tower_cfg &t = s->tower;
  t = apk_magnetic_tower_cfg{};
  t.li_alpha = pin.GetOrAddReal(kTower, "li_alpha", 0.0);
  t.l_scale = pin.GetOrAddReal(kTower, "l_scale", 0.0);
  t.donut_offset = pin.GetOrAddReal(kTower, "donut_offset", 0.0);
  t.donut_thickness = pin.GetOrAddReal(kTower, "donut_thickness", 0.0);
  o.initial_field = pin.GetOrAddReal(kTower, "initial_field", 0.0);
  o.fixed_field_rate = pin.GetOrAddReal(kTower, "fixed_field_rate", 0.0);
  o.fixed_mass_rate = pin.GetOrAddReal(kTower, "fixed_mass_rate", 0.0);
  t.l_mass_scale = pin.GetOrAddReal(kTower, "l_mass_scale", 0.0);
  const std::string potential_str = pin.GetOrAddString(kTower, "potential_type", "undefined");
  t.potential = potential_str == "donut" ? APK_TOWER_DONUT : (potential_str == "li" ? APK_TOWER_LI : APK_TOWER_UNDEFINED);
  // (stricter than the reference, which meets an undefined potential inside a kernel)
  if (tower_block && t.potential == APK_TOWER_UNDEFINED)
    refuse("problem/cluster/magnetic_tower/potential_type", "= " + potential_str + ": must be donut or li (Unknown magnetic tower potential.)");
  tower_check_combination(t);
  o.li_alpha = t.li_alpha, o.l_scale = t.l_scale, o.donut_offset = t.donut_offset, o.donut_thickness = t.donut_thickness;
  o.l_mass_scale = t.l_mass_scale, o.tower_potential = t.potential;
  const struct {
    const char *key;
    double v;
  } tower_rates[] = {{"initial_field", o.initial_field}, {"fixed_field_rate", o.fixed_field_rate}, {"fixed_mass_rate", o.fixed_mass_rate}};
  for (const auto &r : tower_rates)
    if (r.v != 0.0 && !mhd) refuse(std::string(kTower) + "/" + r.key, "!= 0 needs hydro/fluid = glmmhd");

  // AGN feedback
  AgnFeedbackInput in;
  in.fixed_power = pin.GetOrAddReal(kAgn, "fixed_power", 0.0);
  in.vceil = pin.GetOrAddReal(kAgn, "vceil", inf);
  in.efficiency = pin.GetOrAddReal(kAgn, "efficiency", 1e-3);
  in.thermal_fraction = pin.GetOrAddReal(kAgn, "thermal_fraction", 0.0);
  in.kinetic_fraction = pin.GetOrAddReal(kAgn, "kinetic_fraction", 0.0);
  in.magnetic_fraction = pin.GetOrAddReal(kAgn, "magnetic_fraction", 0.0);
  in.thermal_radius = pin.GetOrAddReal(kAgn, "thermal_radius", 0.01);
  in.kinetic_jet_radius = pin.GetOrAddReal(kAgn, "kinetic_jet_radius", 0.01);
  in.kinetic_jet_thickness = pin.GetOrAddReal(kAgn, "kinetic_jet_thickness", 0.02);
  in.kinetic_jet_offset = pin.GetOrAddReal(kAgn, "kinetic_jet_offset", 0.02);
  o.disabled = pin.GetOrAddBoolean(kAgn, "disabled", false) ? 1 : 0;
  in.enable_magnetic_tower_mass_injection = pin.GetOrAddBoolean(kAgn, "enable_magnetic_tower_mass_injection", true);
  in.has_velocity = pin.DoesParameterExist(kAgn, "kinetic_jet_velocity");
  if (in.has_velocity) in.kinetic_jet_velocity = pin.GetReal(kAgn, "kinetic_jet_velocity");
  in.has_temperature = pin.DoesParameterExist(kAgn, "kinetic_jet_temperature");
  if (in.has_temperature) in.kinetic_jet_temperature = pin.GetReal(kAgn, "kinetic_jet_temperature");
  in.Tceil = pin.GetOrAddReal(kAgn, "Tceil", inf);
  o.fixed_power = in.fixed_power, o.efficiency = in.efficiency, o.vceil = in.vceil, o.Tceil = in.Tceil;
  o.enable_magnetic_tower_mass_injection = in.enable_magnetic_tower_mass_injection ? 1 : 0;
  o.thermal_radius = in.thermal_radius, o.kinetic_jet_radius = in.kinetic_jet_radius;
  o.kinetic_jet_thickness = in.kinetic_jet_thickness, o.kinetic_jet_offset = in.kinetic_jet_offset;
  o.thermal_fraction = in.thermal_fraction, o.kinetic_fraction = in.kinetic_fraction, o.magnetic_fraction = in.magnetic_fraction;

  if (in.fixed_power != 0.0 && !u.has_composition)
    refuse("problem/cluster/agn_feedback/fixed_power", "!= 0 requires units and gas composition. Set a 'units' block and "
           "'hydro/He_mass_fraction' in the input file.");
  // (the reference meets this in the first stage: "AGNFeedback::FeedbackSrcTerm Magnetic, Thermal, and Kinetic fractions
  // are all zero")
  if (in.fixed_power != 0.0 && in.thermal_fraction == 0.0 && in.kinetic_fraction == 0.0 && in.magnetic_fraction == 0.0)
    refuse("problem/cluster/agn_feedback/fixed_power", "!= 0 with thermal_fraction, kinetic_fraction and magnetic_fraction all zero "
           "(AGNFeedback::FeedbackSrcTerm Magnetic, Thermal, and Kinetic fractions are all zero)");
  const bool triggered = s->trig.mode != APK_TRIG_NONE;
  if (triggered && !o.disabled && in.thermal_fraction == 0.0 && in.kinetic_fraction == 0.0 && in.magnetic_fraction == 0.0)
    refuse("problem/cluster/agn_triggering/triggering_mode", "other than NONE with problem/cluster/agn_feedback/disabled = false and "
           "thermal_fraction, kinetic_fraction and magnetic_fraction all zero (AGNFeedback::FeedbackSrcTerm Magnetic, Thermal, and "
           "Kinetic fractions are all zero)");
  if (in.magnetic_fraction != 0.0 && !mhd) refuse("problem/cluster/agn_feedback/magnetic_fraction", "!= 0 needs hydro/fluid = glmmhd");

  // the derived jet numbers need the units: with them the constructor's requirements hold for every deck, as in the
  // reference; without them (no feedback possible, see above) the keys are kept as read
  if (u.has_composition && (agn_block || triggered)) {
    in.speed_of_light = u.speed_of_light();
    in.mbar_gm1_over_kb = u.mbar_over_kb * (s->pkg.eos.gamma - 1.0);
    s->agn = agn_feedback_model(in);
    const AgnFeedbackModel &m = s->agn;
    o.configured = 1;
    o.assumed_cold_jet = m.assumed_cold_jet ? 1 : 0;
    o.thermal_fraction = m.thermal_fraction, o.kinetic_fraction = m.kinetic_fraction, o.magnetic_fraction = m.magnetic_fraction;
    o.thermal_mass_fraction = m.thermal_mass_fraction, o.kinetic_mass_fraction = m.kinetic_mass_fraction;
    o.magnetic_mass_fraction = m.magnetic_mass_fraction;
    o.kinetic_jet_velocity = m.kinetic_jet_velocity, o.kinetic_jet_temperature = m.kinetic_jet_temperature;
    o.kinetic_jet_e = m.kinetic_jet_e, o.eceil = m.eceil;
    o.speed_of_light = in.speed_of_light, o.mbar_gm1_over_kb = in.mbar_gm1_over_kb;
    o.power = m.power(), o.mass_rate = m.mass_rate();
  }
  o.active = (o.configured && (in.fixed_power != 0.0 || triggered) && !o.disabled) ? 1 : 0;
  // (cluster.cpp:225-231: magnetic_fraction != 0 && (fixed_power != 0 || triggering_mode != NONE))
  o.tower_power_scaling = (o.active && o.magnetic_fraction != 0.0) ? 1 : 0;
  // whatever evaluates the tower needs its potential and its length scales (MagneticTowerObj's constructor)
  const bool tower_used = o.tower_power_scaling || o.initial_field != 0.0 || o.fixed_field_rate != 0.0;
  if (tower_used && t.potential == APK_TOWER_UNDEFINED)
    refuse("problem/cluster/magnetic_tower/potential_type", "must be donut or li (Unknown magnetic tower potential.)");
  if (tower_used) tower_check_scales(t);
  if ((o.active || o.fixed_field_rate != 0.0) && s->pkg.diffint == APK_DIFFINT_RKL2)
    refuse((o.active && in.fixed_power != 0.0) ? "problem/cluster/agn_feedback/fixed_power" : "problem/cluster/magnetic_tower/fixed_field_rate",
           "!= 0 is not supported with diffusion/integrator = rkl2");
  s->pkg.feedback_srcterm = o.active || o.fixed_field_rate != 0.0;
}

apk_jet_coords jet_at(const apk_sim *s, double time) {
  return jet_coords_at(s->agn_opt.jet_theta, s->agn_opt.jet_phi_dot, s->agn_opt.jet_phi0, time);
}

}  // namespace

void cluster_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  const UnitsState &u = s->pkg.units;
  apk_cluster_options &o = s->cluster;
  o = apk_cluster_options{};
  // a deck of another problem with only its problem_id switched: the generator is known only together with its blocks
  // (the reference would abort on the first required key, problem/cluster/gravity/gravity_srcterm)
  if (pin.BlocksWithPrefix("problem/cluster").empty())
    throw std::runtime_error("unknown job/problem_id: cluster is known only together with its <problem/cluster/...> blocks, and "
                             "this deck has none (problem/cluster/gravity/gravity_srcterm is required)");
  // (reading a key with its default enters it: which blocks the deck itself has is asked first)
  const bool agn_block = pin.DoesBlockExist(kAgn), tower_block = pin.DoesBlockExist(kTower);
  refuse_unbuilt(s);
  o.enabled = 1;
  o.gravitational_constant = u.gravitational_constant();
  o.msun = u.msun(), o.kpc = u.kpc(), o.mpc = u.mpc(), o.km_s = u.km_s(), o.kev = u.kev();

  // uniform gas (cluster.cpp:120-136) and uniform field (cluster.cpp:142-154)
  o.init_uniform_gas = pin.GetOrAddBoolean("problem/cluster/uniform_gas", "init_uniform_gas", false) ? 1 : 0;
  if (o.init_uniform_gas) {
    o.uniform_gas_rho = pin.GetReal("problem/cluster/uniform_gas", "rho");
    o.uniform_gas_ux = pin.GetReal("problem/cluster/uniform_gas", "ux");
    o.uniform_gas_uy = pin.GetReal("problem/cluster/uniform_gas", "uy");
    o.uniform_gas_uz = pin.GetReal("problem/cluster/uniform_gas", "uz");
    o.uniform_gas_pres = pin.GetReal("problem/cluster/uniform_gas", "pres");
  }
  o.init_uniform_b_field = pin.GetOrAddBoolean("problem/cluster/uniform_b_field", "init_uniform_b_field", false) ? 1 : 0;
  if (o.init_uniform_b_field) {
    if (s->pkg.fluid != APK_FLUID_GLMMHD)
      refuse("problem/cluster/uniform_b_field/init_uniform_b_field", "needs hydro/fluid = glmmhd");
    o.uniform_b_field_bx = pin.GetReal("problem/cluster/uniform_b_field", "bx");
    o.uniform_b_field_by = pin.GetReal("problem/cluster/uniform_b_field", "by");
    o.uniform_b_field_bz = pin.GetReal("problem/cluster/uniform_b_field", "bz");
  }

  // ClusterGravity::ClusterGravity (cluster_gravity.hpp:115-165)
  ClusterGravityInput gi;
  gi.include_nfw_g = pin.GetOrAddBoolean(kGrav, "include_nfw_g", false);
  const std::string which_bcg_g_str = pin.GetOrAddString(kGrav, "which_bcg_g", "NONE");
  if (which_bcg_g_str == "NONE") gi.which_bcg_g = APK_BCG_NONE;
  else if (which_bcg_g_str == "HERNQUIST") gi.which_bcg_g = APK_BCG_HERNQUIST;
  else throw std::runtime_error("### FATAL ERROR in function [InitUserMeshData]\nUnknown BCG type " + which_bcg_g_str +
                                " (problem/cluster/gravity/which_bcg_g)");
  gi.include_smbh_g = pin.GetOrAddBoolean(kGrav, "include_smbh_g", false);
  gi.gravitational_constant = o.gravitational_constant;
  gi.hubble_parameter = pin.GetOrAddReal("problem/cluster", "hubble_parameter", 70 * u.km_s() / u.mpc());
  gi.m_nfw_200 = pin.GetOrAddReal(kGrav, "m_nfw_200", 8.5e14 * u.msun());
  gi.c_nfw = pin.GetOrAddReal(kGrav, "c_nfw", 6.81);
  gi.alpha_bcg_s = pin.GetOrAddReal(kGrav, "alpha_bcg_s", 0.1);
  gi.beta_bcg_s = pin.GetOrAddReal(kGrav, "beta_bcg_s", 1.43);
  gi.m_bcg_s = pin.GetOrAddReal(kGrav, "m_bcg_s", 7.5e10 * u.msun());
  gi.r_bcg_s = pin.GetOrAddReal(kGrav, "r_bcg_s", 4 * u.kpc());
  gi.m_smbh = pin.GetOrAddReal(kGrav, "m_smbh", 3.4e8 * u.msun());
  gi.g_smoothing_radius = pin.GetOrAddReal(kGrav, "g_smoothing_radius", 0.0);
  o.gravity = cluster_gravity_constants(gi);
  o.include_nfw_g = gi.include_nfw_g, o.which_bcg_g = gi.which_bcg_g, o.include_smbh_g = gi.include_smbh_g;
  o.hubble_parameter = gi.hubble_parameter;
  o.m_nfw_200 = gi.m_nfw_200, o.c_nfw = gi.c_nfw, o.alpha_bcg_s = gi.alpha_bcg_s, o.beta_bcg_s = gi.beta_bcg_s;
  o.m_bcg_s = gi.m_bcg_s, o.r_bcg_s = gi.r_bcg_s, o.m_smbh = gi.m_smbh, o.g_smoothing_radius = gi.g_smoothing_radius;
  o.gravity_srcterm = pin.GetBoolean(kGrav, "gravity_srcterm") ? 1 : 0;  // (required, cluster.cpp:183-184)
  if (o.gravity_srcterm && s->pkg.diffint == APK_DIFFINT_RKL2)
    refuse("problem/cluster/gravity/gravity_srcterm", "= true is not supported with diffusion/integrator = rkl2");
  if (o.gravity_srcterm && gi.include_nfw_g && !(o.gravity.r_nfw_s > 0.0))
    refuse("problem/cluster/gravity/m_nfw_200", "and c_nfw must give a positive NFW scale radius");
  if (o.gravity_srcterm && gi.which_bcg_g == APK_BCG_HERNQUIST && !(gi.r_bcg_s > 0.0))
    refuse("problem/cluster/gravity/r_bcg_s", "must be positive");
  s->pkg.gravity_srcterm = o.gravity_srcterm != 0;
  triggering_initialize(s);
  feedback_initialize(s, agn_block, tower_block);
  sources_initialize(s);

  // ACCEPTEntropyProfile (entropy_profiles.hpp:25-34)
  o.k_0 = pin.GetOrAddReal("problem/cluster/entropy_profile", "k_0", 20 * u.kev() * u.cm() * u.cm());
  o.k_100 = pin.GetOrAddReal("problem/cluster/entropy_profile", "k_100", 120 * u.kev() * u.cm() * u.cm());
  o.r_k = pin.GetOrAddReal("problem/cluster/entropy_profile", "r_k", 100 * u.kpc());
  o.alpha_k = pin.GetOrAddReal("problem/cluster/entropy_profile", "alpha_k", 1.75);

  // HydrostaticEquilibriumSphere (hydrostatic_equilibrium_sphere.cpp:38-87)
  o.mh = u.mh();
  o.k_boltzmann = u.k_boltzmann();
  o.mu = u.mu, o.mu_e = u.mu_e;  // (0 without a composition)
  o.r_fix = pin.GetOrAddReal(kHse, "r_fix", 1953.9724519818478 * u.kpc());
  o.rho_fix = pin.GetOrAddReal(kHse, "rho_fix", 8.607065015897638e-30 * u.g() / std::pow(u.kpc(), 3));
  o.r_sampling = pin.GetOrAddReal(kHse, "r_sampling", 4.0);
  o.test_he_sphere = pin.GetOrAddBoolean(kHse, "test_he_sphere", false) ? 1 : 0;
  if (o.test_he_sphere) {
    o.test_he_sphere_r_start = pin.GetOrAddReal(kHse, "test_he_sphere_r_start", 1e-3 * u.kpc());
    o.test_he_sphere_r_end = pin.GetOrAddReal(kHse, "test_he_sphere_r_end", 4000 * u.kpc());
    o.test_he_sphere_n_r = pin.GetOrAddInteger(kHse, "test_he_sphere_n_r", 4000);
  }
  if (!o.init_uniform_gas || o.test_he_sphere) {
    // (the reference reads mu and mu_e from the package and aborts when they are missing, hydrostatic_equilibrium_sphere.cpp:49-50)
    if (!u.has_composition)
      refuse("problem/cluster/uniform_gas/init_uniform_gas", "= false: the hydrostatic sphere requires units and gas composition. "
             "Set a 'units' block and 'hydro/He_mass_fraction' in the input file.");
    if (!(o.r_sampling > 0.0)) refuse("problem/cluster/hydrostatic_equilibrium/r_sampling", "must be positive");
    if (!(o.r_k > 0.0)) refuse("problem/cluster/entropy_profile/r_k", "must be positive");
    if (o.test_he_sphere) {
      if (o.test_he_sphere_n_r < 2) refuse("problem/cluster/hydrostatic_equilibrium/test_he_sphere_n_r", "must be at least 2");
      // (as in the reference the profile is generated when the package is built: a deck whose r_fix the test mesh does
      // not bracket fails here)
      (void)he_generate_profile(sphere_of(o), o.test_he_sphere_r_start, o.test_he_sphere_r_end, (unsigned)o.test_he_sphere_n_r);
    }
  }
}

// cluster::ProblemGenerator (cluster.cpp:469-550) and, with GLM-MHD, the uniform field (cluster.cpp:630-653; the
// vector potential of the tower and the dipole is zero here, so its curl adds exact zeros)
void cluster_pgen_block(apk_sim *s, int lb, std::vector<double> &u) {
  const Mesh &m = s->mesh;
  const apk_cluster_options &o = s->cluster;
  const bool mhd = s->pkg.fluid == APK_FLUID_GLMMHD;
  const double gm1 = s->pkg.eos.gamma - 1.0;
  auto at = [&](int n, int k, int j, int i) -> double & { return u[n * m.sn + k * m.sk + j * m.sj + i]; };
  double x0[3];
  block_origin(s, lb, x0);
  if (o.init_uniform_gas) {
    const double rho = o.uniform_gas_rho, ux = o.uniform_gas_ux, uy = o.uniform_gas_uy, uz = o.uniform_gas_uz;
    const double pres = o.uniform_gas_pres;
    const double Mx = rho * ux, My = rho * uy, Mz = rho * uz;
    const double E = rho * (0.5 * (ux * ux + uy * uy + uz * uz) + pres / (gm1 * rho));
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) {
          at(0, k, j, i) = rho;
          at(1, k, j, i) = Mx;
          at(2, k, j, i) = My;
          at(3, k, j, i) = Mz;
          at(4, k, j, i) = E;
        }
  } else {
    const HeProfile prof = block_profile(s, lb);
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) {
          const double x1 = xc(s, x0, 0, i), x2 = xc(s, x0, 1, j), x3 = xc(s, x0, 2, k);
          const double r = std::sqrt(x1 * x1 + x2 * x2 + x3 * x3);
          const double P_r = prof.P_from_r(r);
          const double rho_r = prof.rho_from_r(r);
          at(0, k, j, i) = rho_r;  // zero initial velocity
          at(4, k, j, i) = P_r / gm1;
        }
  }
  if (mhd && s->agn_opt.initial_field != 0.0) {
    // the initial magnetic tower: the potential on the interior plus one cell, jet frame at time 0, B its
    // central-difference curl and 0.5 B^2 added to the energy (cluster.cpp:556-625, magnetic_tower.cpp:206-235)
    const int n1 = m.ie - m.is + 1, n2 = m.je - m.js + 1, n3 = m.ke - m.ks + 1;
    std::vector<double> x1, x2, x3;
    for (int i = m.is - 1; i <= m.ie + 1; ++i) x1.push_back(xc(s, x0, 0, i));
    for (int j = m.js - 1; j <= m.je + 1; ++j) x2.push_back(xc(s, x0, 1, j));
    for (int k = m.ks - 1; k <= m.ke + 1; ++k) x3.push_back(xc(s, x0, 2, k));
    const size_t nb = (size_t)n1 * n2 * n3;
    std::vector<double> b(3 * nb);
    tower_initial_field_block(s->tower, jet_at(s, 0.0), s->agn_opt.initial_field, x1.data(), n1, x2.data(), n2, x3.data(), n3, s->dx,
                              b.data());
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) {
          const size_t q = ((size_t)(k - m.ks) * n2 + (j - m.js)) * n1 + (i - m.is);
          const double bx = b[q], by = b[nb + q], bz = b[2 * nb + q];
          at(5, k, j, i) = bx;
          at(6, k, j, i) = by;
          at(7, k, j, i) = bz;
          at(4, k, j, i) += 0.5 * (bx * bx + by * by + bz * bz);
        }
  }
  if (mhd && o.init_uniform_b_field) {
    // (cluster.cpp:630-653: added to whatever the potential left)
    const double bx = o.uniform_b_field_bx, by = o.uniform_b_field_by, bz = o.uniform_b_field_bz;
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) {
          const double bx_i = at(5, k, j, i), by_i = at(6, k, j, i), bz_i = at(7, k, j, i);
          at(5, k, j, i) += bx;
          at(6, k, j, i) += by;
          at(7, k, j, i) += bz;
          at(4, k, j, i) += bx_i * bx + by_i * by + bz_i * bz + 0.5 * (bx * bx + by * by + bz * bz);
        }
  }
}

bool cluster_needs_block_origins(const apk_sim *s) {
  return s->pkg.gravity_srcterm || s->pkg.agn_triggering || s->pkg.snia_srcterm || s->pkg.cluster_split_srcterm ||
         (s->cluster.enabled && (s->agn_opt.configured || s->tower.potential != APK_TOWER_UNDEFINED));
}

// The sum over all blocks of all ranks of nq per-block sums, out[nq]: d_local holds this rank's, nq per local block
// (nullptr: zeros, nothing is read back).  Every local block's sums go into its slot of a zeroed array over all blocks,
// one allreduce_sum, the slots added in global block order.  Adding zeros is exact: the result does not depend on the
// distribution of the blocks, which is what makes two ranks reproduce one bit for bit.
static int sum_blocks_in_global_order(apk_sim *s, const double *d_local, int nq, double *out) {
  const Mesh &m = s->mesh;
  const size_t nlb = m.local_gids.size();
  std::vector<double> local(nq * nlb, 0.0), all((size_t)nq * m.nblocks_total, 0.0);
  if (d_local) {
    SIM_HIP(s, hipMemcpyAsync(local.data(), d_local, sizeof(double) * local.size(), hipMemcpyDeviceToHost, hs(s)));
    SIM_HIP(s, hipStreamSynchronize(hs(s)));
  }
  for (size_t lb = 0; lb < nlb; ++lb)
    for (int q = 0; q < nq; ++q) all[(size_t)nq * m.local_gids[lb] + q] = local[nq * lb + q];
  if (s->have_comm && s->nranks > 1 && s->comm.allreduce_sum(s->comm.user, all.data(), (int)all.size()) != 0)
    return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  for (int q = 0; q < nq; ++q) out[q] = 0.0;
  for (size_t g = 0; g < (size_t)m.nblocks_total; ++g)
    for (int q = 0; q < nq; ++q) out[q] += all[nq * g + q];
  return APK_OK;
}

static AgnTriggeringModel::Reduced reduced_of(const AgnTriggeringModel &t, const double *q) {
  AgnTriggeringModel::Reduced r;
  if (t.mode == APK_TRIG_COLD_GAS) r.cold_mass = q[0];
  else r.total_mass = q[0], r.mass_weighted_density = q[1], r.mass_weighted_velocity = q[2], r.mass_weighted_cs = q[3];
  return r;
}

// MagneticTowerReducePowerContribs with its reduction over ranks (magnetic_tower.cpp:301-317, hydro_driver.cpp:409-449)
int cluster_tower_contribs(apk_sim *s, double time, double out[2]) {
  const int nlb = (int)s->mesh.local_gids.size();
  if (!s->d_block_xmin) return fail(s, APK_ERR_INVALID, "magnetic_tower_contribs needs problem_id = cluster with a magnetic tower");
  SIM_TRY(s, sync_ghosts(s));  // (materialises the stored primitives when the cycle kept them out of memory)
  if (!s->d_tower_contribs) SIM_TRY(s, dev_alloc(s, "tower_contribs", sizeof(double) * 2 * (size_t)std::max(nlb, 1), &s->d_tower_contribs));
  const apk_jet_coords jet = jet_at(s, time);
  SIM_TRY(s, apk_magnetic_tower_power_contribs(s->ctx, s->mu0(), &s->tower, &jet, s->d_block_xmin, s->d_tower_contribs, s->stream));
  return sum_blocks_in_global_order(s, s->d_tower_contribs, 2, out);
}

// the feedback part of ClusterUnsplitSrcTerm (cluster.cpp:76-80): AGNFeedback::FeedbackSrcTerm -- the thermal and kinetic
// channels, then MagneticTower::PowerSrcTerm with the power-scaled field (agn_feedback.cpp:411-416) -- and
// MagneticTower::FixedFieldSrcTerm.  The jet frame is the one of the cycle's start time in every stage (tm.time).
int cluster_feedback_sources(apk_sim *s, double beta_dt) {
  const apk_agn_feedback_options &o = s->agn_opt;
  const apk_jet_coords jet = jet_at(s, s->time);
  try {
    if (o.active && s->agn.power() != 0) {  // (agn_feedback.cpp:241: "No AGN feedback, return")
      const apk_agn_feedback_cfg cfg = agn_feedback_stage_numbers(s->agn, beta_dt);
      SIM_TRY(s, apk_agn_feedback_src(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, &cfg, &jet, s->d_block_xmin, s->stream));
      const double magnetic_power = s->agn.power() * s->agn.magnetic_fraction;
      const double magnetic_mass_rate = s->agn.mass_rate() * s->agn.magnetic_mass_fraction;
      if (magnetic_power != 0) {
        const double field_to_add = tower_field_to_add(s->tower_linear_contrib, s->tower_quadratic_contrib, beta_dt, magnetic_power);
        (void)tower_density_to_add(magnetic_mass_rate * beta_dt, s->tower.l_mass_scale);  // (its requirement, as a step error)
        SIM_TRY(s, apk_magnetic_tower_src(s->ctx, s->mu0(), &s->tower, &jet, s->d_block_xmin, field_to_add,
                                          magnetic_mass_rate * beta_dt, s->stream));
      }
    }
    if (o.fixed_field_rate != 0) {
      (void)tower_density_to_add(o.fixed_mass_rate * beta_dt, s->tower.l_mass_scale);
      SIM_TRY(s, apk_magnetic_tower_src(s->ctx, s->mu0(), &s->tower, &jet, s->d_block_xmin, o.fixed_field_rate * beta_dt,
                                        o.fixed_mass_rate * beta_dt, s->stream));
    }
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

// SNIAFeedback::FeedbackSrcTerm, the third term of ClusterUnsplitSrcTerm (cluster.cpp:82-83)
int cluster_snia_source(apk_sim *s, double beta_dt) {
  return apk_snia_feedback_src(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, &s->snia, s->d_block_xmin, beta_dt, s->stream);
}

// ClusterSplitSrcTerm (cluster.cpp:85-93) over this rank's active list, the five sums over blocks and ranks
// (sum_blocks_in_global_order) added to the running totals; out[5]: this call's sums (may be null)
static int split_sources(apk_sim *s, bool stellar, bool clips, double *out) {
  const bool listed = !s->split_boxes.empty();  // (a rank with no block in the list launches nothing and contributes zeros)
  if (listed)
    SIM_TRY(s, apk_cluster_split_src(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, stellar ? &s->stellar : nullptr, clips ? &s->clips : nullptr,
                                     s->d_split_boxes, (int)s->split_boxes.size(), s->split_max_box_cells, s->d_block_xmin,
                                     s->d_split_sums, s->stream));
  double sum[8];
  SIM_TRY(s, sum_blocks_in_global_order(s, listed ? s->d_split_sums : nullptr, 8, sum));
  for (int q = 0; q < 5; ++q) {
    s->split_totals[q] += sum[q];
    if (out) out[q] = sum[q];
  }
  return APK_OK;
}

int cluster_split_sources(apk_sim *s, double dt) {
  (void)dt;  // (the reference passes it; neither stellar feedback nor the clips reads it)
  return split_sources(s, s->csrc.stellar_active != 0, s->csrc.clips_active != 0, nullptr);
}

// AGN triggering of one cycle (hydro_driver.cpp:360-394): AGNTriggeringResetTriggering, ReduceTriggering over this rank's
// active list (COLD_GAS removes in the same launch), the sum over blocks and ranks (sum_blocks_in_global_order), and what
// follows from the sums.
static int triggering_reduce(apk_sim *s, double dt) {
  const AgnTriggeringModel &t = s->trig;
  SIM_TRY(s, sync_ghosts(s));  // (ghost cells of the boxes are read and written; materialises the stored primitives)
  const bool listed = !s->trig_boxes.empty();  // (a rank with no block in the list launches nothing and contributes zeros)
  if (listed) {
    apk_agn_triggering_cfg cfg{};
    cfg.mode = t.mode, cfg.remove_accreted_mass = t.remove_accreted_mass ? 1 : 0;
    cfg.accretion_radius = t.accretion_radius, cfg.cold_temp_thresh = t.cold_temp_thresh, cfg.cold_t_acc = t.cold_t_acc;
    cfg.mean_molecular_mass_by_kb = t.mean_molecular_mass_by_kb;
    SIM_TRY(s, apk_agn_triggering_reduce(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, &cfg, s->d_trig_boxes, (int)s->trig_boxes.size(),
                                         s->trig_max_box_cells, s->d_block_xmin, dt, s->d_trig_sums, s->stream));
  }
  double sum[4];
  SIM_TRY(s, sum_blocks_in_global_order(s, listed ? s->d_trig_sums : nullptr, 4, sum));
  AgnTriggeringModel::Reduced &r = s->trig_q;
  r = reduced_of(t, sum);
  s->trig_time = s->time, s->trig_dt = dt;
  if (t.mode != APK_TRIG_COLD_GAS && r.total_mass == 0) {
    s->trig_rate = s->agn.accretion_rate = 0.0;
    return fail(s, APK_ERR_INVALID, "AGN triggering: no gas inside problem/cluster/agn_triggering/accretion_radius (the reduced total_mass "
                                    "is zero): the Bondi accretion rate is undefined");
  }
  s->trig_rate = t.accretion_rate(r);
  s->agn.accretion_rate = s->trig_rate;
  if (s->agn_opt.configured) s->agn_opt.power = s->agn.power(), s->agn_opt.mass_rate = s->agn.mass_rate();
  return APK_OK;
}

static int triggering_remove_bondi(apk_sim *s, double dt) {
  if (s->trig_boxes.empty()) return APK_OK;
  return apk_agn_triggering_remove_bondi(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, s->trig.accretion_radius, s->d_trig_boxes,
                                         (int)s->trig_boxes.size(), s->trig_max_box_cells, s->d_block_xmin, s->trig_q.total_mass,
                                         s->trig_rate, dt, s->stream);
}

// AGNTriggeringFinalizeTriggering's row (agn_triggering.cpp:491-524), every number with %.17g (the reference prints six
// digits): time dt accretion_rate, then cold_mass or total_mass avg_density avg_velocity avg_cs
static int triggering_write_row(apk_sim *s) {
  if (s->trig_path.empty() || s->rank != 0) return APK_OK;
  FILE *f = std::fopen(s->trig_path.c_str(), "a");
  if (!f) return fail(s, APK_ERR_INVALID, "cannot open " + s->trig_path);
  const AgnTriggeringModel::Reduced &r = s->trig_q;
  std::fprintf(f, "%.17g %.17g %.17g ", s->trig_time, s->trig_dt, s->trig_rate);
  if (s->trig.mode == APK_TRIG_COLD_GAS)
    std::fprintf(f, "%.17g", r.cold_mass);
  else
    std::fprintf(f, "%.17g %.17g %.17g %.17g", r.total_mass, r.mass_weighted_density / r.total_mass, r.mass_weighted_velocity / r.total_mass,
                 r.mass_weighted_cs / r.total_mass);
  std::fprintf(f, "\n");
  std::fclose(f);
  return APK_OK;
}

int cluster_agn_triggering(apk_sim *s, double dt) {
  SIM_TRY(s, triggering_reduce(s, dt));
  SIM_TRY(s, triggering_write_row(s));  // (AGNTriggeringFinalizeTriggering writes before it removes)
  if (s->trig.mode != APK_TRIG_COLD_GAS && s->trig.remove_accreted_mass) SIM_TRY(s, triggering_remove_bondi(s, dt));
  return APK_OK;
}

void cluster_triggering_reset(apk_sim *s) {
  s->trig_q = AgnTriggeringModel::Reduced{};
  s->trig_rate = s->trig_time = s->trig_dt = 0.0;
  s->agn.accretion_rate = 0.0;
  if (s->agn_opt.configured) s->agn_opt.power = s->agn.power(), s->agn_opt.mass_rate = s->agn.mass_rate();
}

// the origins apk_gravity_src takes: every local block's lower interior corner, then the mesh's lower corner
int cluster_device_setup(apk_sim *s) {
  const Mesh &m = s->mesh;
  const int nlb = (int)m.local_gids.size();
  std::vector<double> h(3 * ((size_t)nlb + 1));
  for (int lb = 0; lb < nlb; ++lb) {
    double x0[3];
    block_origin(s, lb, x0);
    for (int d = 0; d < 3; ++d) h[3 * (size_t)lb + d] = s->xmin[d] + x0[d] * s->dx[d];
    // the kernel rebuilds the block's first global index from the corner: the cell centres it then forms must be xc()'s
    for (int d = 0; d < 3; ++d)
      if (std::rint((h[3 * (size_t)lb + d] - s->xmin[d]) / s->dx[d]) != x0[d])
        return fail(s, APK_ERR_INVALID, "cluster sources: a block's corner does not give back its global cell index");
  }
  for (int d = 0; d < 3; ++d) h[3 * (size_t)nlb + d] = s->xmin[d];
  SIM_TRY(s, dev_alloc(s, "block_xmin", h.size() * sizeof(double), &s->d_block_xmin));
  SIM_HIP(s, hipMemcpy(s->d_block_xmin, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  if (s->pkg.agn_triggering && !s->trig_boxes.empty()) {
    SIM_TRY(s, dev_alloc(s, "trig_boxes", s->trig_boxes.size() * sizeof(apk_trig_box), reinterpret_cast<double **>(&s->d_trig_boxes)));
    SIM_HIP(s, hipMemcpy(s->d_trig_boxes, s->trig_boxes.data(), s->trig_boxes.size() * sizeof(apk_trig_box), hipMemcpyHostToDevice));
    SIM_TRY(s, dev_alloc(s, "trig_sums", sizeof(double) * 4 * (size_t)std::max(nlb, 1), &s->d_trig_sums));
  }
  if (s->pkg.cluster_split_srcterm && !s->split_boxes.empty()) {
    SIM_TRY(s, dev_alloc(s, "split_boxes", s->split_boxes.size() * sizeof(apk_trig_box), reinterpret_cast<double **>(&s->d_split_boxes)));
    SIM_HIP(s, hipMemcpy(s->d_split_boxes, s->split_boxes.data(), s->split_boxes.size() * sizeof(apk_trig_box), hipMemcpyHostToDevice));
    SIM_TRY(s, dev_alloc(s, "split_sums", sizeof(double) * 8 * (size_t)std::max(nlb, 1), &s->d_split_sums));
  }
  return APK_OK;
}

// PRhoProfile::write_to_ostream (hydrostatic_equilibrium_sphere.cpp:92-119), every number with %.17g
int cluster_write_test_profile(apk_sim *s, const std::string &path) {
  const apk_cluster_options &o = s->cluster;
  if (!o.enabled || !o.test_he_sphere || s->rank != 0) return APK_OK;
  try {
    const HeProfile prof = he_generate_profile(sphere_of(o), o.test_he_sphere_r_start, o.test_he_sphere_r_end, (unsigned)o.test_he_sphere_n_r);
    const size_t n = (size_t)prof.n_r;
    std::vector<double> col(9 * n);
    prof.columns(col.data());
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail(s, APK_ERR_INVALID, "cannot open " + path);
    for (size_t i = 0; i < n; ++i) {
      for (int c = 0; c < 9; ++c) std::fprintf(f, c ? " %.17g" : "%.17g", col[c * n + i]);
      std::fprintf(f, "\n");
    }
    std::fclose(f);
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

}  // namespace host
}  // namespace apk

using namespace apk;
using namespace apk::host;

extern "C" {

int apk_sim_cluster_options(const apk_sim *s, apk_cluster_options *opt) {
  if (!s || !opt) return APK_ERR_INVALID;
  *opt = s->cluster;
  return APK_OK;
}

int apk_sim_he_sphere_profile(apk_sim *s, double r_start, double r_end, int n_r, double *out) {
  if (!s || !out) return APK_ERR_INVALID;
  if (!sphere_available(s)) return fail(s, APK_ERR_INVALID, "he_sphere_profile needs problem_id = cluster with units and gas composition");
  if (n_r < 2) return fail(s, APK_ERR_INVALID, "he_sphere_profile: n_r must be at least 2");
  try {
    he_generate_profile(sphere_of(s->cluster), r_start, r_end, (unsigned)n_r).columns(out);
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

int apk_sim_block_he_profile(apk_sim *s, int lb, double *r, double *p, int n, int *size) {
  if (!s || !size || lb < 0 || lb >= (int)s->mesh.local_gids.size()) return APK_ERR_INVALID;
  if (!sphere_available(s)) return fail(s, APK_ERR_INVALID, "block_he_profile needs problem_id = cluster with units and gas composition");
  try {
    const HeProfile prof = block_profile(s, lb);
    *size = prof.n_r;
    for (int i = 0; i < n && i < prof.n_r; ++i) {
      if (r) r[i] = prof.r[i];
      if (p) p[i] = prof.p[i];
    }
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

int apk_sim_pgen_block(apk_sim *s, int lb, double *out) {
  if (!s || !out || lb < 0 || lb >= (int)s->mesh.local_gids.size()) return APK_ERR_INVALID;
  if (s->problem_id == "turbulence") return fail(s, APK_ERR_INVALID, "the turbulence generator fills all blocks at once");
  const Mesh &m = s->mesh;
  try {
    std::vector<double> u((size_t)m.nvar * m.sn);
    pgen_block(s, lb, u);
    size_t q = 0;
    for (int n = 0; n < m.nvar; ++n)
      for (int k = m.ks; k <= m.ke; ++k)
        for (int j = m.js; j <= m.je; ++j)
          for (int i = m.is; i <= m.ie; ++i) out[q++] = u[n * m.sn + k * m.sk + j * m.sj + i];
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

int apk_sim_gravity_src(apk_sim *s, double beta_dt) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->cluster.enabled || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "gravity_src needs problem_id = cluster with problem/cluster/gravity/gravity_srcterm = true");
  SIM_TRY(s, sync_ghosts(s));  // (materialises the stored primitives when the cycle kept them out of memory)
  SIM_TRY(s, apk_gravity_src(s->ctx, s->mu0(), &s->cluster.gravity, s->d_block_xmin, beta_dt, s->stream));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

int apk_sim_agn_feedback_options(const apk_sim *s, apk_agn_feedback_options *opt) {
  if (!s || !opt) return APK_ERR_INVALID;
  *opt = s->agn_opt;
  return APK_OK;
}

int apk_sim_agn_feedback_stage_numbers(const apk_sim *s, double beta_dt, double time, apk_agn_feedback_cfg *cfg, apk_jet_coords *jet) {
  if (!s || !cfg || !jet || !s->cluster.enabled || !s->agn_opt.configured) return APK_ERR_INVALID;
  *cfg = agn_feedback_stage_numbers(s->agn, beta_dt);
  *jet = jet_at(s, time);
  return APK_OK;
}

int apk_sim_magnetic_tower_field_to_add(apk_sim *s, double lin, double quad, double beta_dt, double power, double *field) {
  if (!s || !field) return APK_ERR_INVALID;
  try {
    *field = tower_field_to_add(lin, quad, beta_dt, power);
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  return APK_OK;
}

int apk_sim_agn_feedback_src(apk_sim *s, double beta_dt, double time) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->cluster.enabled || !s->agn_opt.configured || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "agn_feedback_src needs problem_id = cluster with a <problem/cluster/agn_feedback> block, units and gas composition");
  SIM_TRY(s, sync_ghosts(s));  // (materialises the stored primitives when the cycle kept them out of memory)
  const apk_agn_feedback_cfg cfg = agn_feedback_stage_numbers(s->agn, beta_dt);
  const apk_jet_coords jet = jet_at(s, time);
  SIM_TRY(s, apk_agn_feedback_src(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, &cfg, &jet, s->d_block_xmin, s->stream));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

int apk_sim_magnetic_tower_src(apk_sim *s, double field, double mass, double time) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->cluster.enabled || s->tower.potential == APK_TOWER_UNDEFINED || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "magnetic_tower_src needs problem_id = cluster with a <problem/cluster/magnetic_tower> block");
  SIM_TRY(s, sync_ghosts(s));
  const apk_jet_coords jet = jet_at(s, time);
  SIM_TRY(s, apk_magnetic_tower_src(s->ctx, s->mu0(), &s->tower, &jet, s->d_block_xmin, field, mass, s->stream));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

int apk_sim_magnetic_tower_contribs(apk_sim *s, double time, double out[2]) {
  if (!s || s->host_only || !out) return APK_ERR_INVALID;
  if (!s->cluster.enabled || s->tower.potential == APK_TOWER_UNDEFINED)
    return fail(s, APK_ERR_INVALID, "magnetic_tower_contribs needs problem_id = cluster with a <problem/cluster/magnetic_tower> block");
  return cluster_tower_contribs(s, time, out);
}

int apk_sim_agn_triggering_options(const apk_sim *s, apk_agn_triggering_options *o) {
  if (!s || !o || !s->cluster.enabled) return APK_ERR_INVALID;
  const AgnTriggeringModel &t = s->trig;
  *o = apk_agn_triggering_options{};
  o->mode = t.mode, o->remove_accreted_mass = t.remove_accreted_mass ? 1 : 0, o->write_to_file = s->trig_write_to_file ? 1 : 0;
  o->active_blocks = (int)s->trig_boxes.size(), o->active_box_cells = s->trig_box_cells;
  o->accretion_radius = t.accretion_radius, o->cold_temp_thresh = t.cold_temp_thresh, o->cold_t_acc = t.cold_t_acc;
  o->bondi_alpha = t.bondi_alpha, o->bondi_M_smbh = t.bondi_M_smbh, o->bondi_n0 = t.bondi_n0, o->bondi_beta = t.bondi_beta;
  o->accretion_cfl = t.accretion_cfl;
  o->mean_molecular_mass = t.mean_molecular_mass, o->mean_molecular_mass_by_kb = t.mean_molecular_mass_by_kb;
  o->gravitational_constant = t.gravitational_constant;
  std::snprintf(o->triggering_filename, sizeof(o->triggering_filename), "%s", s->trig_filename.c_str());
  return APK_OK;
}

int apk_sim_agn_triggering_state(const apk_sim *s, apk_agn_triggering_state *st) {
  if (!s || !st || !s->cluster.enabled) return APK_ERR_INVALID;
  const AgnTriggeringModel::Reduced &r = s->trig_q;
  *st = apk_agn_triggering_state{};
  st->cold_mass = r.cold_mass, st->total_mass = r.total_mass, st->mass_weighted_density = r.mass_weighted_density;
  st->mass_weighted_velocity = r.mass_weighted_velocity, st->mass_weighted_cs = r.mass_weighted_cs;
  st->accretion_rate = s->trig_rate;
  st->power = s->agn_opt.configured ? s->agn.power() : 0.0;
  st->dt_limit = s->trig.estimate_timestep(r);
  st->time = s->trig_time, st->dt = s->trig_dt;
  return APK_OK;
}

int apk_sim_agn_triggering_accretion_rate(const apk_sim *s, const double *q, double *rate) {
  if (!s || !q || !rate || !s->cluster.enabled) return APK_ERR_INVALID;
  *rate = s->trig.accretion_rate(reduced_of(s->trig, q));
  return APK_OK;
}

int apk_sim_agn_triggering_timestep(const apk_sim *s, const double *q, double *dt) {
  if (!s || !q || !dt || !s->cluster.enabled) return APK_ERR_INVALID;
  *dt = s->trig.estimate_timestep(reduced_of(s->trig, q));
  return APK_OK;
}

int apk_sim_agn_feedback_power_of(const apk_sim *s, double accretion_rate, double *power, double *mass_rate) {
  if (!s || !power || !mass_rate || !s->cluster.enabled || !s->agn_opt.configured) return APK_ERR_INVALID;
  AgnFeedbackModel m = s->agn;
  m.accretion_rate = accretion_rate;
  *power = m.power(), *mass_rate = m.mass_rate();
  return APK_OK;
}

int apk_sim_agn_triggering_active_list(const apk_sim *s, int *out, int n, int *size) {
  if (!s || !size || !s->cluster.enabled) return APK_ERR_INVALID;
  *size = (int)s->trig_boxes.size();
  for (int e = 0; out && e < n && e < *size; ++e) {
    const apk_trig_box &b = s->trig_boxes[(size_t)e];
    out[7 * e] = b.block;
    for (int d = 0; d < 3; ++d) out[7 * e + 1 + d] = b.lo[d], out[7 * e + 4 + d] = b.hi[d];
  }
  return APK_OK;
}

int apk_sim_cluster_source_options(const apk_sim *s, apk_cluster_source_options *o) {
  if (!s || !o || !s->cluster.enabled) return APK_ERR_INVALID;
  *o = s->csrc;
  o->flux_path_sources = s->pkg.flux_path_sources() ? 1 : 0;
  return APK_OK;
}

int apk_sim_cluster_split_active_list(const apk_sim *s, int *out, int n, int *size) {
  if (!s || !size || !s->cluster.enabled) return APK_ERR_INVALID;
  *size = (int)s->split_boxes.size();
  for (int e = 0; out && e < n && e < *size; ++e) {
    const apk_trig_box &b = s->split_boxes[(size_t)e];
    out[7 * e] = b.block;
    for (int d = 0; d < 3; ++d) out[7 * e + 1 + d] = b.lo[d], out[7 * e + 4 + d] = b.hi[d];
  }
  return APK_OK;
}

int apk_sim_snia_feedback_src(apk_sim *s, double beta_dt) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->cluster.enabled || !s->pkg.snia_srcterm || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "snia_feedback_src needs problem_id = cluster with problem/cluster/snia_feedback/disabled = false");
  SIM_TRY(s, sync_ghosts(s));  // (materialises the stored primitives when the cycle kept them out of memory)
  SIM_TRY(s, cluster_snia_source(s, beta_dt));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

int apk_sim_cluster_split_src(apk_sim *s, double dt, int stellar, int clips, double out[5]) {
  if (!s || s->host_only || !out) return APK_ERR_INVALID;
  (void)dt;
  if (!s->cluster.enabled || !s->pkg.cluster_split_srcterm || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "cluster_split_src needs problem_id = cluster with problem/cluster/stellar_feedback or problem/cluster/clips");
  SIM_TRY(s, sync_ghosts(s));
  SIM_TRY(s, split_sources(s, stellar && s->csrc.stellar_active, clips && s->csrc.clips_active, out));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

int apk_sim_cluster_source_totals(const apk_sim *s, double out[5]) {
  if (!s || !out || !s->cluster.enabled) return APK_ERR_INVALID;
  for (int q = 0; q < 5; ++q) out[q] = s->split_totals[q];
  return APK_OK;
}

int apk_sim_agn_triggering_reduce(apk_sim *s, double dt) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->cluster.enabled || !s->pkg.agn_triggering || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "agn_triggering_reduce needs problem_id = cluster with problem/cluster/agn_triggering/triggering_mode other than NONE");
  SIM_TRY(s, triggering_reduce(s, dt));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

int apk_sim_agn_triggering_remove_bondi(apk_sim *s, double dt) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->cluster.enabled || s->trig.mode == APK_TRIG_NONE || s->trig.mode == APK_TRIG_COLD_GAS || !s->d_block_xmin)
    return fail(s, APK_ERR_INVALID, "agn_triggering_remove_bondi needs problem_id = cluster with triggering_mode = BOOSTED_BONDI or BOOTH_SCHAYE");
  SIM_TRY(s, sync_ghosts(s));
  SIM_TRY(s, triggering_remove_bondi(s, dt));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

}  // extern "C"
