"""ctypes binding of libapk_amd.so (include/apk_amd.h + include/apk_host.h).

The shared library is the product; this module only loads it and declares the C
signatures.  There is no Python/CPU fallback: if the library is missing, or no gfx950
device is visible when a context is created, the call fails loudly.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")

# enums of include/apk_amd.h (positions in the reference's enum classes, src/main.hpp:35-38)
FLUID = {"euler": 1, "glmmhd": 2}
RECON = {"dc": 1, "plm": 2, "ppm": 3, "wenoz": 4, "weno3": 5, "limo3": 6}
RIEMANN = {"none": 1, "hlle": 2, "llf": 3, "hllc": 4, "hlld": 5}
INTEGRATOR = {"rk1": 1, "rk2": 2, "vl2": 3, "rk3": 4}
# diffusion enums of include/apk_amd.h (src/main.hpp:40-46)
CONDUCTION = {"none": 0, "isotropic": 1, "anisotropic": 2}
VISCOSITY = {"none": 0, "isotropic": 1}
RESISTIVITY = {"none": 0, "ohmic": 1}
DIFF_COEFF = {"none": 0, "fixed": 1, "spitzer": 2}
# cooling integrators (apk_cool_integrator; cooling::CoolIntegrator) and the flag bits of its device failures
COOL_INTEGRATOR = {"rk12": 1, "rk45": 2, "townsend": 3}
APK_FLAG_COOL_MAX_ITER = 4
APK_FLAG_COOL_TABLE = 8
APK_FLAG_AGN_NEG_PRESSURE = 16
APK_FLAG_STELLAR_ENERGY = 32  # stellar feedback's "Added thermal energy should be positive"

TIMING_SLOTS = ("fused_x1", "fused_x2", "fused_x3", "fluxes", "update", "dedner", "cons_to_prim",
                "min_dt", "copy_regions", "fused_dc_x1", "fused_dc_x2", "fused_dc_x3", "tracers", "tracer_sort", "gravity",
                "agn_feedback", "tower", "tower_contribs", "triggering", "cluster_sources")

APK_OK = 0
APK_RCCL_ID_BYTES = 128
APK_ERR_INVALID, APK_ERR_UNSUPPORTED, APK_ERR_NGHOST, APK_ERR_DEVICE, APK_ERR_NO_DEVICE = -1, -2, -3, -4, -5
FLAG_NEG_DENSITY, FLAG_NEG_PRESSURE = 1, 2

c_dp = C.POINTER(C.c_double)


class Eos(C.Structure):
    _fields_ = [("gamma", C.c_double), ("pfloor", C.c_double), ("dfloor", C.c_double),
                ("efloor", C.c_double), ("vceil", C.c_double), ("eceil", C.c_double)]


def make_eos(gamma, pfloor=-1.0, dfloor=-1.0, efloor=-1.0, vceil=float("inf"),
             eceil=float("inf")):
    return Eos(gamma, pfloor, dfloor, efloor, vceil, eceil)


class FluxCfg(C.Structure):
    _fields_ = [("fluid", C.c_int), ("recon", C.c_int), ("riemann", C.c_int)]


class DiffCfg(C.Structure):
    _fields_ = [("conduction", C.c_int), ("conduction_coeff", C.c_int), ("thermal_diff_coeff", C.c_double),
                ("conduction_sat_prefac", C.c_double), ("viscosity", C.c_int), ("viscosity_coeff", C.c_int),
                ("mom_diff_coeff", C.c_double), ("resistivity", C.c_int), ("resistivity_coeff", C.c_int),
                ("ohm_diff_coeff", C.c_double)]


def make_diff_cfg(conduction="none", kappa=0.0, sat_phi=0.3, viscosity="none", nu=0.0, resistivity="none", eta=0.0):
    """apk_diff_cfg with fixed coefficients; conduction_sat_prefac = 5 phi (hydro.cpp:595-604)"""
    fixed = DIFF_COEFF["fixed"]
    return DiffCfg(CONDUCTION[conduction], fixed, kappa, 5.0 * sat_phi, VISCOSITY[viscosity], fixed, nu,
                   RESISTIVITY[resistivity], fixed, eta)


class SpitzerCfg(C.Structure):
    _fields_ = [("coeff_code", C.c_double), ("mbar", C.c_double), ("k_boltzmann", C.c_double)]


def make_spitzer_cfg(coeff_code, mbar, k_boltzmann):
    """apk_spitzer_cfg, all in code units: the Spitzer coefficient (spitzer_cond_in_erg_by_s_K_cm * erg / (s cm)), mbar
    = mu * atomic_mass_unit and k_boltzmann (hydro.cpp:577-586).  Goes with a lib.DiffCfg whose conduction_coeff is
    DIFF_COEFF["spitzer"] and whose conduction_sat_prefac is 6.86 sqrt(mu) phi (hydro.cpp:589-593)."""
    return SpitzerCfg(float(coeff_code), float(mbar), float(k_boltzmann))


class Rkl2Regs(C.Structure):
    _fields_ = [("y0", C.c_void_p), ("yjm2", C.c_void_p), ("my0", C.c_void_p)]


class Rkl2Coeffs(C.Structure):
    _fields_ = [("mu", C.c_double), ("nu", C.c_double), ("mu_tilde", C.c_double), ("gamma_tilde", C.c_double)]


class CoolingParams(C.Structure):
    _fields_ = [("integrator", C.c_int), ("max_iter", C.c_int), ("cfl", C.c_double), ("d_log_temp_tol", C.c_double),
                ("d_e_tol", C.c_double), ("T_floor", C.c_double), ("lambda_units", C.c_double), ("gamma", C.c_double),
                ("mbar_over_kb", C.c_double), ("He_mass_fraction", C.c_double), ("mh", C.c_double)]


def make_cooling_params(integrator="rk12", max_iter=100, cfl=0.1, d_log_temp_tol=1e-8, d_e_tol=1e-8, T_floor=-1.0,
                        lambda_units=1.0, gamma=5.0 / 3.0, mbar_over_kb=1.0, He_mass_fraction=0.25, mh=1.0):
    """apk_cooling_params with the reference's defaults (tabular_cooling.cpp:53-68)"""
    return CoolingParams(COOL_INTEGRATOR[integrator], int(max_iter), float(cfl), float(d_log_temp_tol), float(d_e_tol),
                         float(T_floor), float(lambda_units), float(gamma), float(mbar_over_kb), float(He_mass_fraction),
                         float(mh))


# which_bcg_g of the cluster problem (apk_cluster_bcg; cluster::BCG)
CLUSTER_BCG = {"NONE": 0, "HERNQUIST": 1}


class ClusterGravity(C.Structure):
    """apk_cluster_gravity: ClusterGravity's members in code units (cluster_gravity.hpp:29-53)"""
    _fields_ = [("include_nfw", C.c_int), ("which_bcg", C.c_int), ("include_smbh", C.c_int), ("r_nfw_s", C.c_double),
                ("g_const_nfw", C.c_double), ("r_bcg_s", C.c_double), ("g_const_bcg", C.c_double),
                ("g_const_smbh", C.c_double), ("smoothing_r", C.c_double)]


class ClusterOptions(C.Structure):
    """apk_cluster_options: problem_id = cluster as parsed (include/apk_host.h)"""
    _fields_ = ([(n, C.c_int) for n in ("enabled", "include_nfw_g", "which_bcg_g", "include_smbh_g", "gravity_srcterm",
                                        "init_uniform_gas", "init_uniform_b_field", "test_he_sphere",
                                        "test_he_sphere_n_r")] +
                [(n, C.c_double) for n in ("hubble_parameter", "m_nfw_200", "c_nfw", "alpha_bcg_s", "beta_bcg_s", "m_bcg_s",
                                           "r_bcg_s", "m_smbh", "g_smoothing_radius", "k_0", "k_100", "r_k", "alpha_k",
                                           "r_fix", "rho_fix", "r_sampling", "test_he_sphere_r_start",
                                           "test_he_sphere_r_end", "uniform_gas_rho", "uniform_gas_ux", "uniform_gas_uy",
                                           "uniform_gas_uz", "uniform_gas_pres", "uniform_b_field_bx",
                                           "uniform_b_field_by", "uniform_b_field_bz", "mh", "k_boltzmann", "mu", "mu_e",
                                           "gravitational_constant", "msun", "kpc", "mpc", "km_s", "kev")] +
                [("gravity", ClusterGravity)])


# potential_type of the magnetic tower (apk_tower_potential; cluster::MagneticTowerPotential)
TOWER_POTENTIAL = {"undefined": 0, "li": 1, "donut": 2}


class JetCoords(C.Structure):
    """apk_jet_coords: cos and sin of the jet axis' angle off z and around z (jet_coords.hpp:25-37)"""
    _fields_ = [(n, C.c_double) for n in ("cos_theta", "sin_theta", "cos_phi", "sin_phi")]


class AgnFeedbackCfg(C.Structure):
    """apk_agn_feedback_cfg: what AGNFeedback::FeedbackSrcTerm computes for one stage (agn_feedback.cpp:263-303)"""
    _fields_ = [(n, C.c_double) for n in ("thermal_feedback", "thermal_density", "thermal_radius", "jet_density",
                                          "jet_momentum", "jet_feedback", "kinetic_jet_radius", "kinetic_jet_thickness",
                                          "kinetic_jet_offset", "vceil", "eceil")]


class MagneticTowerCfg(C.Structure):
    """apk_magnetic_tower_cfg: MagneticTowerObj's members (magnetic_tower.hpp:45-58)"""
    _fields_ = [("potential", C.c_int)] + [(n, C.c_double) for n in ("li_alpha", "l_scale", "donut_offset",
                                                                    "donut_thickness", "l_mass_scale")]


class AgnFeedbackOptions(C.Structure):
    """apk_agn_feedback_options: <problem/cluster/agn_feedback>, .../magnetic_tower and .../precessing_jet as parsed, and
    the derived jet numbers (include/apk_host.h)"""
    _fields_ = ([(n, C.c_int) for n in ("configured", "active", "disabled", "enable_magnetic_tower_mass_injection",
                                        "assumed_cold_jet", "tower_potential", "tower_power_scaling")] +
                [(n, C.c_double) for n in ("fixed_power", "efficiency", "thermal_fraction", "kinetic_fraction",
                                           "magnetic_fraction", "thermal_mass_fraction", "kinetic_mass_fraction",
                                           "magnetic_mass_fraction", "thermal_radius", "kinetic_jet_radius",
                                           "kinetic_jet_thickness", "kinetic_jet_offset", "kinetic_jet_velocity",
                                           "kinetic_jet_temperature", "kinetic_jet_e", "vceil", "Tceil", "eceil",
                                           "jet_theta", "jet_phi_dot", "jet_phi0", "li_alpha", "l_scale", "donut_offset",
                                           "donut_thickness", "initial_field", "fixed_field_rate", "fixed_mass_rate",
                                           "l_mass_scale", "speed_of_light", "mbar_gm1_over_kb", "power", "mass_rate")])


# triggering_mode of AGN triggering (apk_agn_triggering_mode; cluster::AGNTriggeringMode)
TRIGGERING_MODE = {"NONE": 0, "COLD_GAS": 1, "BOOSTED_BONDI": 2, "BOOTH_SCHAYE": 3}


class TrigBox(C.Structure):
    """apk_trig_box: an entry of the active list -- a block of the pack and its index box [lo, hi) in the block's
    extended index space (i, j, k)"""
    _fields_ = [("block", C.c_int), ("lo", C.c_int * 3), ("hi", C.c_int * 3)]


class AgnTriggeringCfg(C.Structure):
    """apk_agn_triggering_cfg: what apk_agn_triggering_reduce takes by value"""
    _fields_ = ([("mode", C.c_int), ("remove_accreted_mass", C.c_int)] +
                [(n, C.c_double) for n in ("accretion_radius", "cold_temp_thresh", "cold_t_acc", "mean_molecular_mass_by_kb")])


class SniaCfg(C.Structure):
    """apk_snia_cfg: what apk_snia_feedback_src takes by value"""
    _fields_ = [(n, C.c_double) for n in ("power_per_bcg_mass", "mass_rate_per_bcg_mass", "rho_const_bcg", "r_bcg_s", "smoothing_r")]


class StellarCfg(C.Structure):
    """apk_stellar_cfg: stellar feedback's numbers as apk_cluster_split_src takes them"""
    _fields_ = [(n, C.c_double) for n in ("stellar_radius", "exclusion_radius", "number_density_threshold", "temperature_threshold",
                                          "mbar", "mbar_over_kb", "mass_to_energy")]


class ClipsCfg(C.Structure):
    """apk_clips_cfg: the clips as apk_cluster_split_src takes them (a clip at its disabled value is skipped)"""
    _fields_ = [(n, C.c_double) for n in ("clip_r", "dfloor", "vceil", "vAceil", "eceil")]


class ClusterSourceOptions(C.Structure):
    """apk_cluster_source_options: <problem/cluster/snia_feedback>, <problem/cluster/stellar_feedback> and
    <problem/cluster/clips> as parsed and derived, and the size of this rank's active list (include/apk_host.h)"""
    _fields_ = ([(n, C.c_int) for n in ("snia_active", "stellar_active", "clips_active", "flux_path_sources", "active_blocks")] +
                [("active_box_cells", C.c_longlong)] +
                [(n, C.c_double) for n in ("power_per_bcg_mass", "mass_rate_per_bcg_mass", "rho_const_bcg", "stellar_radius",
                                           "exclusion_radius", "efficiency", "number_density_threshold", "temperature_threshold",
                                           "mbar", "mbar_over_kb", "mass_to_energy", "clip_r", "dfloor", "vceil", "vAceil", "Tceil",
                                           "eceil")])


class AgnTriggeringOptions(C.Structure):
    """apk_agn_triggering_options: <problem/cluster/agn_triggering> as parsed, the derived mean molecular mass and
    temperature factor, and the size of this rank's active list (include/apk_host.h)"""
    _fields_ = ([(n, C.c_int) for n in ("mode", "remove_accreted_mass", "write_to_file", "active_blocks")] +
                [("active_box_cells", C.c_longlong)] +
                [(n, C.c_double) for n in ("accretion_radius", "cold_temp_thresh", "cold_t_acc", "bondi_alpha", "bondi_M_smbh",
                                           "bondi_n0", "bondi_beta", "accretion_cfl", "mean_molecular_mass",
                                           "mean_molecular_mass_by_kb", "gravitational_constant")] +
                [("triggering_filename", C.c_char * 256)])


class AgnTriggeringState(C.Structure):
    """apk_agn_triggering_state: the last cycle's reduced quantities and what follows from them"""
    _fields_ = [(n, C.c_double) for n in ("cold_mass", "total_mass", "mass_weighted_density", "mass_weighted_velocity",
                                          "mass_weighted_cs", "accretion_rate", "power", "dt_limit", "time", "dt")]


class UnitsInfo(C.Structure):
    _fields_ = [("has_units", C.c_int), ("has_composition", C.c_int), ("code_length_cgs", C.c_double),
                ("code_mass_cgs", C.c_double), ("code_time_cgs", C.c_double), ("mh", C.c_double),
                ("k_boltzmann", C.c_double), ("atomic_mass_unit", C.c_double), ("erg", C.c_double), ("cm", C.c_double),
                ("s", C.c_double), ("He_mass_fraction", C.c_double), ("mu", C.c_double), ("mu_e", C.c_double),
                ("mbar", C.c_double), ("mbar_over_kb", C.c_double), ("efloor", C.c_double), ("eceil", C.c_double)]


class BlockDesc(C.Structure):
    _fields_ = [("cons", C.c_void_p), ("prim", C.c_void_p), ("flux", C.c_void_p * 3),
                ("dx", C.c_double * 3)]


class PackDesc(C.Structure):
    _fields_ = [("nblocks", C.c_int), ("nhydro", C.c_int), ("nscalars", C.c_int),
                ("nx", C.c_int * 3), ("ng", C.c_int), ("blocks", C.POINTER(BlockDesc)), ("stride", C.c_int64 * 3)]


class StageArgs(C.Structure):
    _fields_ = [("cfg", FluxCfg), ("eos", Eos), ("c_h", C.c_double), ("gam0", C.c_double),
                ("gam1", C.c_double), ("beta_dt", C.c_double), ("dedner", C.c_int),
                ("glmmhd_alpha", C.c_double), ("mindx", C.c_double), ("fill_derived", C.c_int),
                ("estimate_dt", C.c_int), ("phase", C.c_int), ("window", C.c_void_p),
                ("window_rl", C.c_int), ("window_rows", C.c_int), ("trial", C.c_int), ("count_unphysical", C.c_int), ("cons_out_delta", C.c_int64),
                ("face_neighbor", C.c_void_p), ("cons_store", C.c_int), ("prim_from_cons", C.c_int), ("x1_halo", C.c_void_p)]


# apk_stage_form_kind, and what apk_stage_form fills in
STAGE_FORMS = ("NONE", "X1", "X1_X2", "THREE_SWEEP", "MARCH12_X3", "DC_MARCH", "TWO_KERNEL", "SINGLE_MARCH")
LEAN_PFLOOR = 2


class StageFormInfo(C.Structure):
    _fields_ = [("form", C.c_int), ("lean", C.c_int), ("dc_rows", C.c_int), ("from_cons", C.c_int), ("x1_halo", C.c_int),
                ("reason", C.c_char_p)]


class X1HaloBlock(C.Structure):
    _fields_ = [("recv", C.c_void_p * 2), ("send", C.c_void_p * 2)]


class X1Halo(C.Structure):
    _fields_ = [("blocks", C.c_void_p), ("recv_depth", C.c_int), ("send_depth", C.c_int), ("send_field", C.c_int)]


class FmftBlock(C.Structure):
    _fields_ = [("acc", C.c_void_p), ("phases_i", C.c_void_p), ("phases_j", C.c_void_p),
                ("phases_k", C.c_void_p)]


class RefineGeom(C.Structure):
    _fields_ = [("nx", C.c_int * 3), ("ng", C.c_int), ("cng", C.c_int), ("dx", C.c_double * 3)]


class RefineOp(C.Structure):
    _fields_ = [("kind", C.c_int), ("src", C.c_void_p), ("dst", C.c_void_p), ("lo", C.c_int * 3),
                ("hi", C.c_int * 3), ("xmin", C.c_double * 3), ("dx", C.c_double * 3)]


REFINE_OPS = {"prolongate": 0, "restrict_cell": 1, "restrict_face1": 2, "restrict_face2": 3, "restrict_face3": 4,
              "restrict_flux1": 5, "restrict_flux2": 6, "restrict_flux3": 7}
TAG_CRITERIA = {"pressure_gradient": 0, "xyvelocity_gradient": 1, "maxdensity": 2}


class FluxFixRegion(C.Structure):
    _fields_ = [("fine_avg", C.c_void_p), ("coarse_flux", C.c_void_p), ("cons", C.c_void_p), ("ext", C.c_int * 3),
                ("nvar", C.c_int), ("src_stride", C.c_int64 * 4), ("dst_stride", C.c_int64 * 4), ("scale", C.c_double),
                ("average", C.c_int), ("ndim", C.c_int), ("fine_stride", C.c_int64 * 3), ("fine_area", C.c_double)]


class CopyRegion(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("ext", C.c_int * 3),
                ("nvar", C.c_int), ("src_stride", C.c_int64 * 4),
                ("dst_stride", C.c_int64 * 4), ("flip_var", C.c_int)]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t)
RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, c_dp, C.c_int)


class Allocator(C.Structure):
    _fields_ = [("user", C.c_void_p), ("alloc", ALLOC_FN), ("release", RELEASE_FN)]


class CommOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("exchange", EXCHANGE_FN), ("allreduce_min", ALLREDUCE_FN),
                ("allreduce_sum", ALLREDUCE_FN), ("exchange_begin", EXCHANGE_FN), ("exchange_end", EXCHANGE_FN)]


class SimInfo(C.Structure):
    _fields_ = [("fluid", C.c_int), ("recon", C.c_int), ("riemann", C.c_int), ("integrator", C.c_int),
                ("nx", C.c_int * 3), ("mb", C.c_int * 3), ("ng", C.c_int), ("nhydro", C.c_int),
                ("nscalars", C.c_int), ("ndim", C.c_int), ("nblocks_total", C.c_int),
                ("nblocks_local", C.c_int), ("first_gid", C.c_int), ("rank", C.c_int),
                ("nranks", C.c_int), ("npeers", C.c_int), ("fofc", C.c_int),
                ("dedner_extended", C.c_int), ("fused", C.c_int), ("cfl", C.c_double),
                ("gamma", C.c_double), ("glmmhd_alpha", C.c_double), ("xmin", C.c_double * 3),
                ("xmax", C.c_double * 3), ("dx", C.c_double * 3), ("cells_per_block", C.c_int64),
                ("zones_local", C.c_int64), ("zones_total", C.c_int64)]


class PeerInfo(C.Structure):
    _fields_ = [("rank", C.c_int), ("send_count", C.c_int64), ("recv_count", C.c_int64),
                ("send_buf", C.c_void_p), ("recv_buf", C.c_void_p)]


class RegionInfo(C.Structure):
    _fields_ = [("src_kind", C.c_int), ("src_block", C.c_int), ("dst_kind", C.c_int),
                ("dst_block", C.c_int), ("src_off", C.c_int64), ("dst_off", C.c_int64),
                ("ext", C.c_int * 3), ("nvar", C.c_int), ("flip_var", C.c_int),
                ("src_stride", C.c_int64 * 4), ("dst_stride", C.c_int64 * 4)]


class TracerArrays(C.Structure):
    _fields_ = [("n", C.c_int64), ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("id", C.c_void_p),
                ("block", C.c_void_p), ("active", C.c_void_p), ("field", C.c_void_p * 8), ("nfields", C.c_int),
                ("s", C.c_void_p), ("sdot", C.c_void_p), ("lookback_stride", C.c_int64), ("n_lookback", C.c_int)]


class TracerGeom(C.Structure):
    _fields_ = [("xmin", C.c_double * 3), ("xmax", C.c_double * 3), ("dx", C.c_double * 3), ("block_size", C.c_double * 3),
                ("nb", C.c_int * 3), ("periodic_lo", C.c_int * 3), ("periodic_hi", C.c_int * 3),
                ("block_origin", C.c_void_p), ("block_table", C.c_void_p)]


TRACER_N_LOOKBACK = 12  # APK_TRACER_N_LOOKBACK
TRACER_N_SUMS = 26      # APK_TRACER_N_SUMS: corr_s[12], corr_sdot[12], sum s, sum sdot
TRACER_SEED = {"none": 0, "random_per_block": 1, "user": 2}
# apk_sim_tracers_read: field number and numpy dtype of every array
TRACER_FIELDS = (("x", "f8"), ("y", "f8"), ("z", "f8"), ("id", "i8"), ("block", "i4"), ("active", "i4"), ("rho", "f8"),
                 ("pressure", "f8"), ("vel_x", "f8"), ("vel_y", "f8"), ("vel_z", "f8"), ("B_x", "f8"), ("B_y", "f8"),
                 ("B_z", "f8"))


class TracersOptions(C.Structure):
    _fields_ = [("enabled", C.c_int), ("seed_method", C.c_int), ("fused", C.c_int), ("nfields", C.c_int),
                ("num_tracers_per_cell", C.c_double), ("rng_seed", C.c_longlong), ("num_tracers_per_block", C.c_longlong)]


# apk_output_component: APK_OUT_CONS + n, APK_OUT_PRIM + n, and the derived fields
OUT_CONS, OUT_PRIM = 0, 64
OUT_DERIVED = {"temperature": 128, "mach_sonic": 129, "B_mag": 130, "mach_alfven": 131, "plasma_beta": 132}
OUT_MAX_COMPONENTS = 48


class OutputDesc(C.Structure):
    """apk_output_desc: what apk_output_pack stores per interior cell"""
    _fields_ = [("ncomp", C.c_int), ("single", C.c_int), ("gamma", C.c_double), ("mbar_over_kb", C.c_double),
                ("comp", C.c_int * OUT_MAX_COMPONENTS)]


def make_output_desc(codes, single=False, gamma=5.0 / 3.0, mbar_over_kb=1.0):
    d = OutputDesc(len(codes), int(bool(single)), float(gamma), float(mbar_over_kb))
    for q, c in enumerate(codes):
        d.comp[q] = int(c)
    return d


class SnapshotOutputInfo(C.Structure):
    """apk_snapshot_output_info: one npy output block of the deck as parsed"""
    _fields_ = [("number", C.c_int), ("single", C.c_int), ("ncomp", C.c_int), ("dt", C.c_double), ("id", C.c_char * 64),
                ("components", C.c_char * 1024)]


class RestartOutputInfo(C.Structure):
    """apk_restart_output_info: one rst output block of the deck as parsed"""
    _fields_ = [("number", C.c_int), ("dt", C.c_double), ("id", C.c_char * 64)]


class AmrOpInfo(C.Structure):
    _fields_ = [("kind", C.c_int), ("level", C.c_int), ("src_kind", C.c_int), ("src_block", C.c_int),
                ("dst_kind", C.c_int), ("dst_block", C.c_int), ("lo", C.c_int * 3), ("hi", C.c_int * 3),
                ("xmin", C.c_double * 3), ("dx", C.c_double * 3), ("cng", C.c_int), ("coarse_doubles", C.c_int64)]


# every symbol include/apk_amd.h and include/apk_host.h declare: name -> (restype, argtypes)
def _signatures():
    i, d, vp, ll = C.c_int, C.c_double, C.c_void_p, C.c_longlong
    E = C.POINTER(Eos)
    pp = C.POINTER(C.c_void_p)
    strs = C.POINTER(C.c_char_p)
    return {
        # apk_amd.h
        "apk_version": (i, []),
        "apk_fp_strict": (i, []),
        "apk_create": (i, [pp]),
        "apk_destroy": (None, [vp]),
        "apk_last_error": (C.c_char_p, [vp]),
        "apk_pack_create": (i, [vp, C.POINTER(PackDesc), pp]),
        "apk_pack_destroy": (None, [vp]),
        "apk_calculate_fluxes": (i, [vp, vp, FluxCfg, E, d, vp]),
        "apk_calculate_fluxes_tight": (i, [vp, vp, FluxCfg, E, d, vp]),
        "apk_calculate_fluxes_boundary": (i, [vp, vp, FluxCfg, E, d, vp]),
        "apk_calculate_fluxes_boundary_list": (i, [vp, vp, FluxCfg, E, d, vp, C.c_int, vp]),
        "apk_calculate_fluxes_boundary_list_from_cons": (i, [vp, vp, FluxCfg, E, d, vp, C.c_int, C.c_longlong, vp]),
        "apk_flux_fix_plan_create": (i, [vp, C.POINTER(FluxFixRegion), i, pp]),
        "apk_flux_fix_plan_create_merged": (i, [vp, C.POINTER(FluxFixRegion), C.POINTER(C.c_int), vp, C.c_int64, pp]),
        "apk_flux_fix_plan_destroy": (None, [vp]),
        "apk_flux_fix_plan_run": (i, [vp, vp, d, i, d, vp]),
        "apk_update_with_flux_divergence": (i, [vp, vp, vp, d, d, d, vp]),
        "apk_dedner_source": (i, [vp, vp, i, d, d, d, d, vp]),
        "apk_stage_fused": (i, [vp, vp, vp, C.POINTER(StageArgs), vp]),
        "apk_cons_to_prim": (i, [vp, vp, i, E, vp]),
        "apk_cons_to_prim_ghosts": (i, [vp, vp, i, E, vp]),
        "apk_cons_to_prim_faces": (i, [vp, vp, i, E, vp]),
        "apk_cons_to_prim_dt": (i, [vp, vp, i, E, i, vp]),
        "apk_cons_to_prim_dt_skip": (i, [vp, vp, i, E, i, vp, vp]),
        "apk_cons_to_prim_dt_select": (i, [vp, vp, i, E, i, vp, C.c_uint, vp]),
        "apk_cons_to_prim_faces_skip": (i, [vp, vp, i, E, vp, vp]),
        "apk_cons_to_prim_faces_dt": (i, [vp, vp, i, E, vp, vp]),
        "apk_cons_to_prim_ghosts_split": (i, [vp, vp, i, E, vp, i, vp]),
        "apk_stage_dt_read": (i, [vp, d, c_dp, vp]),
        "apk_stage_dt_flags_read": (i, [vp, d, c_dp, C.POINTER(C.c_uint), vp]),
        "apk_estimate_timestep": (i, [vp, vp, i, E, d, c_dp, vp]),
        "apk_calc_diff_fluxes": (i, [vp, vp, C.POINTER(DiffCfg), vp]),
        "apk_estimate_diffusion_timestep": (i, [vp, vp, C.POINTER(DiffCfg), d, c_dp, vp]),
        "apk_calc_diff_fluxes_v2": (i, [vp, vp, C.POINTER(DiffCfg), C.POINTER(SpitzerCfg), vp]),
        "apk_estimate_diffusion_timestep_v2": (i, [vp, vp, C.POINTER(DiffCfg), C.POINTER(SpitzerCfg), d, c_dp, vp]),
        "apk_rkl2_num_stages": (i, [d, d, C.POINTER(C.c_int)]),
        "apk_rkl2_coefficients": (i, [i, i, c_dp, c_dp, c_dp, c_dp]),
        "apk_flux_divergence": (i, [vp, vp, vp, vp]),
        "apk_rkl2_step_first": (i, [vp, vp, vp, vp, vp, i, d, vp]),
        "apk_rkl2_step_other": (i, [vp, vp, vp, vp, vp, d, d, d, d, d, vp]),
        "apk_rkl2_substage_fused": (i, [vp, vp, C.POINTER(Rkl2Regs), C.POINTER(DiffCfg), C.POINTER(Rkl2Coeffs), d, i, vp]),
        "apk_rkl2_substage_fused_v2": (i, [vp, vp, C.POINTER(Rkl2Regs), C.POINTER(DiffCfg), C.POINTER(SpitzerCfg),
                                           C.POINTER(Rkl2Coeffs), d, i, vp]),
        "apk_cooling_table_create": (i, [vp, c_dp, c_dp, i, C.POINTER(CoolingParams), pp]),
        "apk_cooling_table_destroy": (None, [vp]),
        "apk_cooling_dedt": (i, [vp, vp, vp, vp, vp, vp, C.c_int64, vp]),
        "apk_tabular_cooling_src": (i, [vp, vp, vp, i, d, vp]),
        "apk_estimate_cooling_timestep": (i, [vp, vp, vp, c_dp, vp]),
        "apk_gravity_src": (i, [vp, vp, C.POINTER(ClusterGravity), vp, d, vp]),
        "apk_gravity_g_from_r": (i, [vp, C.POINTER(ClusterGravity), vp, vp, C.c_int64, vp]),
        "apk_agn_feedback_src": (i, [vp, vp, i, C.POINTER(Eos), C.POINTER(AgnFeedbackCfg), C.POINTER(JetCoords), vp, vp]),
        "apk_magnetic_tower_src": (i, [vp, vp, C.POINTER(MagneticTowerCfg), C.POINTER(JetCoords), vp, d, d, vp]),
        "apk_magnetic_tower_power_contribs": (i, [vp, vp, C.POINTER(MagneticTowerCfg), C.POINTER(JetCoords), vp, vp, vp]),
        "apk_agn_triggering_reduce": (i, [vp, vp, i, C.POINTER(Eos), C.POINTER(AgnTriggeringCfg), vp, i, C.c_int64, vp, d, vp, vp]),
        "apk_agn_triggering_remove_bondi": (i, [vp, vp, i, C.POINTER(Eos), d, vp, i, C.c_int64, vp, d, d, d, vp]),
        "apk_snia_feedback_src": (i, [vp, vp, i, C.POINTER(Eos), C.POINTER(SniaCfg), vp, d, vp]),
        "apk_cluster_split_src": (i, [vp, vp, i, C.POINTER(Eos), C.POINTER(StellarCfg), C.POINTER(ClipsCfg), vp, i, C.c_int64, vp, vp, vp]),
        "apk_first_order_flux_correct": (i, [vp, vp, vp, i, E, d, d, d, d, C.POINTER(ll), vp]),
        "apk_count_unphysical": (i, [vp, vp, i, C.POINTER(ll), vp]),
        "apk_history": (i, [vp, vp, i, c_dp, vp]),
        "apk_fmft_create": (i, [vp, C.POINTER(FmftBlock), i, i, pp]),
        "apk_fmft_destroy": (None, [vp]),
        "apk_fmft_inverse": (i, [vp, vp, vp, c_dp, vp]),
        "apk_turb_mean_momentum": (i, [vp, vp, vp, c_dp, vp]),
        "apk_turb_remove_mean": (i, [vp, vp, vp, c_dp, c_dp, vp]),
        "apk_turb_apply": (i, [vp, vp, vp, d, d, vp]),
        "apk_turb_apply_fill": (i, [vp, vp, vp, d, d, i, E, i, vp]),
        "apk_turb_apply_dt": (i, [vp, vp, vp, d, d, i, E, vp]),
        "apk_turbulence_history": (i, [vp, vp, i, d, c_dp, vp]),
        "apk_history_user_reldivb": (i, [vp, vp, d, c_dp, vp]),
        "apk_refine_plan_create": (i, [vp, C.POINTER(RefineGeom), i, C.POINTER(RefineOp), i, pp]),
        "apk_refine_plan_destroy": (None, [vp]),
        "apk_refine_plan_run": (i, [vp, vp, vp]),
        "apk_tag_blocks": (i, [vp, vp, i, d, d, C.POINTER(C.c_int), c_dp, vp]),
        "apk_tag_blocks_begin": (i, [vp, vp, i, C.POINTER(C.c_int), vp]),
        "apk_tag_blocks_begin_skip": (i, [vp, vp, i, vp, C.POINTER(C.c_int), vp]),
        "apk_tag_blocks_dt_from_cons": (i, [vp, vp, i, E, vp, C.POINTER(C.c_int), vp]),
        "apk_tag_blocks_end": (i, [vp, i, i, i, d, d, C.POINTER(C.c_int), c_dp, vp]),
        "apk_poll_device_flags": (i, [vp, C.POINTER(C.c_uint), vp]),
        "apk_trial_flags": (i, [vp, i, vp]),
        "apk_stage_split_axis": (i, [vp, vp, i]),
        "apk_stage_single_march": (i, [vp, vp]),
        "apk_stage_form": (i, [C.POINTER(PackDesc), C.POINTER(StageArgs), C.POINTER(StageFormInfo)]),
        "apk_bench_scheme_floor": (i, [i, i, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
        "apk_stage_x1_halo": (i, [vp, vp, E, i, i, i]),
        "apk_stage_unphysical_read": (i, [vp, C.POINTER(C.c_longlong), vp]),
        "apk_copy_plan_create": (i, [vp, C.POINTER(CopyRegion), i, pp]),
        "apk_copy_plan_destroy": (None, [vp]),
        "apk_copy_plan_run": (i, [vp, vp, vp]),
        "apk_copy_plan_run_c2p": (i, [vp, vp, i, E, C.c_int64, i, vp]),
        "apk_copy_plan_run_c2p_prim_only": (i, [vp, vp, i, E, C.c_int64, i, vp]),
        "apk_tracers_advect": (i, [vp, vp, C.POINTER(TracerArrays), C.POINTER(TracerGeom), d, vp]),
        "apk_tracers_reown": (i, [vp, C.POINTER(TracerArrays), C.POINTER(TracerGeom), vp, vp]),
        "apk_tracers_fill": (i, [vp, vp, C.POINTER(TracerArrays), C.POINTER(TracerGeom), vp]),
        "apk_tracers_step_fused": (i, [vp, vp, C.POINTER(TracerArrays), C.POINTER(TracerGeom), d, vp, vp]),
        "apk_tracers_sort": (i, [vp, vp, C.POINTER(TracerArrays), C.POINTER(TracerArrays), C.POINTER(TracerGeom), vp, i, vp]),
        "apk_tracers_lookback": (i, [vp, C.POINTER(TracerArrays), ll, d, vp, ll, vp, vp]),
        "apk_tracers_step_fused_lookback": (i, [vp, vp, C.POINTER(TracerArrays), C.POINTER(TracerGeom), d, vp, ll, vp, ll, vp, vp]),
        "apk_output_pack": (i, [vp, vp, i, E, C.POINTER(OutputDesc), i, i, vp, vp]),
        "apk_restart_unpack": (i, [vp, vp, i, i, vp, vp]),
        "apk_kernel_timing_enable": (i, [vp, i]),
        "apk_kernel_timing_read": (i, [vp, i, c_dp, C.POINTER(ll)]),
        # apk_host.h
        "apk_sim_create": (i, [C.c_char_p, strs, i, i, i, C.POINTER(Allocator), C.POINTER(CommOps),
                               vp, pp, C.c_char_p, C.c_size_t]),
        "apk_sim_create_host_only": (i, [C.c_char_p, strs, i, i, i, pp, C.c_char_p, C.c_size_t]),
        "apk_sim_destroy": (None, [vp]),
        "apk_sim_last_error": (C.c_char_p, [vp]),
        "apk_sim_initialize": (i, [vp]),
        "apk_sim_step": (i, [vp]),
        "apk_sim_run": (i, [vp, i, C.POINTER(C.c_int)]),
        "apk_sim_time": (d, [vp]),
        "apk_sim_dt": (d, [vp]),
        "apk_sim_tlim": (d, [vp]),
        "apk_sim_c_h": (d, [vp]),
        "apk_sim_ncycle": (i, [vp]),
        "apk_sim_fofc_count": (ll, [vp]),
        "apk_sim_set_fused": (i, [vp, i]),
        "apk_sim_set_overlap": (i, [vp, i]),
        "apk_sim_overlapped_exchanges": (ll, [vp]),
        "apk_sim_skipped_local_exchanges": (ll, [vp]),
        "apk_sim_amr_c2p_passes_skipped": (ll, [vp]),
        "apk_sim_set_thin_exchange": (i, [vp, i]),
        "apk_sim_thin_exchanges": (ll, [vp]),
        "apk_sim_set_x1_direct": (i, [vp, i]),
        "apk_sim_x1_direct_exchanges": (ll, [vp]),
        "apk_sim_set_direct_neighbors": (C.c_int, [vp, C.c_int]),
        "apk_sim_set_amr_full_exchange": (C.c_int, [vp, C.c_int]),
        "apk_sim_set_prim_free": (C.c_int, [vp, C.c_int]),
        "apk_sim_prim_is_stale": (C.c_int, [vp]),
        "apk_sim_turb_dt_kicks": (ll, [vp]),
        "apk_sim_loop_seconds": (d, [vp]),
        "apk_sim_loop_cycles": (i, [vp]),
        "apk_sim_get_info": (i, [vp, C.POINTER(SimInfo)]),
        "apk_sim_diffusion_options": (i, [vp, C.POINTER(DiffCfg), C.POINTER(C.c_int), c_dp]),
        "apk_sim_spitzer_options": (i, [vp, C.POINTER(C.c_int), C.POINTER(SpitzerCfg)]),
        "apk_sim_rkl2_max_dt_ratio": (d, [vp]),
        "apk_sim_sts_info": (i, [vp, C.POINTER(C.c_int), c_dp, C.POINTER(C.c_int)]),
        "apk_sim_units": (i, [vp, C.POINTER(UnitsInfo)]),
        "apk_sim_cooling_options": (i, [vp, C.POINTER(C.c_int), C.POINTER(CoolingParams), C.POINTER(C.c_int)]),
        "apk_sim_cooling_table": (i, [vp, i, c_dp, i, C.POINTER(C.c_int)]),
        "apk_sim_cluster_options": (i, [vp, C.POINTER(ClusterOptions)]),
        "apk_sim_he_sphere_profile": (i, [vp, d, d, i, c_dp]),
        "apk_sim_block_he_profile": (i, [vp, i, c_dp, c_dp, i, C.POINTER(C.c_int)]),
        "apk_sim_pgen_block": (i, [vp, i, c_dp]),
        "apk_sim_gravity_src": (i, [vp, d]),
        "apk_sim_agn_feedback_options": (i, [vp, C.POINTER(AgnFeedbackOptions)]),
        "apk_sim_agn_feedback_stage_numbers": (i, [vp, d, d, C.POINTER(AgnFeedbackCfg), C.POINTER(JetCoords)]),
        "apk_sim_magnetic_tower_field_to_add": (i, [vp, d, d, d, d, c_dp]),
        "apk_sim_agn_feedback_src": (i, [vp, d, d]),
        "apk_sim_magnetic_tower_src": (i, [vp, d, d, d]),
        "apk_sim_magnetic_tower_contribs": (i, [vp, d, c_dp]),
        "apk_sim_agn_triggering_options": (i, [vp, C.POINTER(AgnTriggeringOptions)]),
        "apk_sim_agn_triggering_state": (i, [vp, C.POINTER(AgnTriggeringState)]),
        "apk_sim_agn_triggering_accretion_rate": (i, [vp, c_dp, c_dp]),
        "apk_sim_agn_triggering_timestep": (i, [vp, c_dp, c_dp]),
        "apk_sim_agn_feedback_power_of": (i, [vp, d, c_dp, c_dp]),
        "apk_sim_agn_triggering_active_list": (i, [vp, C.POINTER(C.c_int), i, C.POINTER(C.c_int)]),
        "apk_sim_cluster_source_options": (i, [vp, C.POINTER(ClusterSourceOptions)]),
        "apk_sim_cluster_split_active_list": (i, [vp, C.POINTER(C.c_int), i, C.POINTER(C.c_int)]),
        "apk_sim_snia_feedback_src": (i, [vp, d]),
        "apk_sim_cluster_split_src": (i, [vp, d, i, i, c_dp]),
        "apk_sim_cluster_source_totals": (i, [vp, c_dp]),
        "apk_sim_agn_triggering_reduce": (i, [vp, d]),
        "apk_sim_agn_triggering_remove_bondi": (i, [vp, d]),
        "apk_sim_tracers_options": (i, [vp, C.POINTER(TracersOptions)]),
        "apk_sim_tracers_count": (i, [vp, C.POINTER(ll), C.POINTER(ll), C.POINTER(ll)]),
        "apk_sim_tracers_stats": (i, [vp, C.POINTER(ll), C.POINTER(ll)]),
        "apk_sim_tracers_read": (i, [vp, i, vp]),
        "apk_sim_tracers_seed": (i, [vp, c_dp, c_dp, c_dp, ll]),
        "apk_sim_tracers_step": (i, [vp, d]),
        "apk_sim_tracer_lookback_options": (i, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "apk_sim_tracer_lookbacks_read": (i, [vp, i, c_dp]),
        "apk_sim_tracer_correlations": (i, [vp, C.POINTER(ll), c_dp, C.POINTER(ll), c_dp]),
        "apk_sim_block_location": (i, [vp, i, C.POINTER(C.c_int), C.POINTER(C.c_int * 3)]),
        "apk_sim_block_ptr": (vp, [vp, i, i]),
        "apk_sim_gather": (i, [vp, i, c_dp]),
        "apk_sim_read_block": (i, [vp, i, i, c_dp]),
        "apk_sim_write_block": (i, [vp, i, i, c_dp]),
        "apk_sim_history": (i, [vp, c_dp]),
        "apk_sim_linear_wave_errors": (i, [vp, c_dp, c_dp, c_dp]),
        "apk_sim_linear_wave_mhd_errors": (i, [vp, c_dp, c_dp, c_dp]),
        "apk_sim_cpaw_errors": (i, [vp, c_dp, c_dp]),
        "apk_sim_write_cpaw_errors": (i, [vp, C.c_char_p]),
        "apk_sim_check_refinement": (i, [vp, C.POINTER(C.c_int), c_dp]),
        "apk_sim_history_labels": (i, [vp, C.c_char_p, C.c_size_t]),
        "apk_sim_write_history": (i, [vp, C.c_char_p]),
        "apk_sim_write_linear_wave_errors": (i, [vp, C.c_char_p]),
        "apk_sim_execute": (i, [vp, C.c_char_p, C.POINTER(C.c_int)]),
        "apk_sim_turbulence_history": (i, [vp, c_dp]),
        "apk_sim_user_reldivb": (i, [vp, c_dp]),
        "apk_sim_fmft_num_modes": (i, [vp]),
        "apk_sim_fmft_var_hat": (i, [vp, c_dp]),
        "apk_sim_fmft_evolve": (i, [vp, d]),
        "apk_sim_fmft_phases": (i, [vp, i, i, i, c_dp]),
        "apk_sim_read_acc": (i, [vp, i, c_dp]),
        "apk_sim_exchange_ghosts": (i, [vp]),
        "apk_sim_fill_derived": (i, [vp]),
        "apk_sim_estimate_timestep": (i, [vp, c_dp]),
        "apk_sim_reset_time_step": (C.c_int, [vp]),
        "apk_sim_kernel_timing_enable": (i, [vp, i]),
        "apk_sim_kernel_timing_read": (i, [vp, i, c_dp, C.POINTER(ll)]),
        "apk_sim_peer": (i, [vp, i, C.POINTER(PeerInfo)]),
        "apk_sim_plan_size": (i, [vp, i]),
        "apk_sim_plan_region": (i, [vp, i, i, C.POINTER(RegionInfo)]),
        "apk_sim_num_peers": (i, [vp]),
        "apk_sim_select_messages": (i, [vp, i]),
        "apk_sim_message_generation": (ll, [vp]),
        "apk_sim_amr_ops_size": (i, [vp, i]),
        "apk_sim_amr_op": (i, [vp, i, i, C.POINTER(AmrOpInfo)]),
        "apk_sim_loop_zone_cycles": (ll, [vp]),
        "apk_sim_fofc_fallback_stages": (ll, [vp]),
        "apk_sim_block_level": (i, [vp, i]),
        "apk_sim_amr_stats": (i, [vp, C.POINTER(ll), C.POINTER(ll), C.POINTER(i), C.POINTER(ll)]),
        "apk_sim_regrid": (i, [vp, C.POINTER(i)]),
        "apk_rccl_unique_ids": (i, [C.c_char_p, C.c_size_t]),
        "apk_sim_comm_rccl": (i, [vp, C.c_char_p, C.c_size_t]),
        "apk_sim_comm_stats": (i, [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
        "apk_sim_comm_error": (C.c_char_p, [vp]),
        "apk_rccl_selftest": (i, [i, C.c_char_p, C.c_size_t]),
        "apk_sim_amr_apply_tags": (i, [vp, C.POINTER(i), i, C.POINTER(i)]),
        "apk_sim_snapshot_outputs": (i, [vp, C.POINTER(SnapshotOutputInfo), i, C.POINTER(i)]),
        "apk_sim_snapshot_shape": (i, [vp, C.c_char_p, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_int * 3), C.POINTER(i),
                                       C.c_char_p, C.c_size_t]),
        "apk_sim_snapshot_read": (i, [vp, C.c_char_p, i, vp, C.c_size_t]),
        "apk_sim_write_snapshot": (i, [vp, C.c_char_p, C.c_char_p, i]),
        "apk_sim_write_snapshot_index": (i, [vp, C.c_char_p, C.c_char_p, i]),
        "apk_sim_restart_outputs": (i, [vp, C.POINTER(RestartOutputInfo), i, C.POINTER(i)]),
        "apk_sim_write_restart": (i, [vp, C.c_char_p]),
        "apk_sim_restore": (i, [vp, C.c_char_p]),
    }


SYMBOLS = tuple(_signatures().keys())


def lib_path(strict=False):
    # APK_LIB_PATH: profiling aid, an A/B variant of the product build (csrc/Makefile `variant`)
    if not strict and os.environ.get("APK_LIB_PATH"):
        return os.path.abspath(os.environ["APK_LIB_PATH"])
    return os.path.join(_HERE, "libapk_amd_strict.so" if strict else "libapk_amd.so")


def build(strict=None, jobs=8):
    """Compile the gfx950 libraries in-tree with hipcc (strict=None builds both)."""
    targets = []
    if strict in (None, False):
        targets.append("../libapk_amd.so")
    if strict in (None, True):
        targets.append("../libapk_amd_strict.so")
    subprocess.run(["make", "-C", _CSRC, "-j%d" % jobs] + targets, check=True,
                   stdout=subprocess.DEVNULL)
    return [os.path.normpath(os.path.join(_CSRC, t)) for t in targets]


_LIBS = {}


def load(strict=False):
    """Load libapk_amd[_strict].so.  Raises if it has not been built."""
    key = bool(strict)
    if key not in _LIBS:
        path = lib_path(strict)
        if not os.path.exists(path):
            raise RuntimeError(
                "%s not found: run athenapk_amd.lib.build() / __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
        lib = C.CDLL(path)
        # (APK_LIB_PATH, or a library from another directory: a profiling variant or a build of an older commit for a
        # same-box comparison -- entry points it lacks are left unbound; the product library must export every declared symbol)
        variant = (bool(os.environ.get("APK_LIB_PATH")) and not strict) or os.path.dirname(path) != _HERE
        skipped = []
        for name, (res, args) in _signatures().items():
            if variant and not hasattr(lib, name):
                skipped.append(name)
                continue
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if skipped:  # (said aloud: a call through an unbound entry point would go out with default int argtypes)
            import warnings
            warnings.warn("%s lacks %d declared entry point(s), left unbound: %s"
                          % (path, len(skipped), ", ".join(skipped)))
        _LIBS[key] = lib
    return _LIBS[key]


class ApkError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("apk error %d: %s" % (code, msg))
        self.code = code
