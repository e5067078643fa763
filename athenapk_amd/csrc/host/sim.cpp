// sim.cpp -- the standalone host driver (include/apk_host.h): deck -> packages and mesh, device
// resources, plans and tables, the step and run loop, outputs and the C API (the stage loop: stage.cpp).
#include "sim_internal.hpp"
#include "../hydro_math.hpp"

using namespace apk;

namespace apk {
namespace host {

int parse_bc(const std::string &v) {
  if (v == "periodic") return BC_PERIODIC;
  if (v == "outflow") return BC_OUTFLOW;
  if (v == "reflecting") return BC_REFLECT;
  throw std::runtime_error("unknown boundary condition: " + v);
}

// ---- Hydro::Initialize (src/hydro/hydro.cpp:264-826), options of this path only ---------
void hydro_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  HydroPackage &pkg = s->pkg;
  pkg.cfl = pin.GetOrAddReal("parthenon/time", "cfl", 0.3);
  const std::string fluid = pin.GetOrAddString("hydro", "fluid", "euler");
  if (fluid == "euler") {
    pkg.fluid = APK_FLUID_EULER;
    pkg.nhydro = 5;
  } else if (fluid == "glmmhd") {
    pkg.fluid = APK_FLUID_GLMMHD;
    pkg.nhydro = 9;
    const std::string src = pin.GetOrAddString("hydro", "glmmhd_source", "dedner_plain");
    if (src == "dedner_plain") pkg.glmmhd_source_extended = false;
    else if (src == "dedner_extended") pkg.glmmhd_source_extended = true;
    else throw std::runtime_error("AthenaPK hydro: Unknown glmmhd_source");
    pkg.glmmhd_alpha = pin.GetOrAddReal("hydro", "glmmhd_alpha", 0.1);
    pkg.calc_c_h = true;
  } else {
    throw std::runtime_error("AthenaPK hydro: Unknown fluid method.");
  }
  pkg.max_dt = pin.GetOrAddReal("hydro", "max_dt", -1.0);

  const std::string recon = pin.GetString("hydro", "reconstruction");
  int need_ng = 3;
  if (recon == "dc") pkg.recon = APK_RC_DC, need_ng = 1;
  else if (recon == "plm") pkg.recon = APK_RC_PLM, need_ng = 2;
  else if (recon == "ppm") pkg.recon = APK_RC_PPM, need_ng = 3;
  else if (recon == "limo3") pkg.recon = APK_RC_LIMO3, need_ng = 2;
  else if (recon == "weno3") pkg.recon = APK_RC_WENO3, need_ng = 2;
  else if (recon == "wenoz") pkg.recon = APK_RC_WENOZ, need_ng = 3;
  else throw std::runtime_error("AthenaPK hydro: Unknown reconstruction method.");

  pkg.calc_dt_hyp = true;
  const std::string riemann = pin.GetString("hydro", "riemann");
  if (riemann == "llf") {
    pkg.riemann = APK_RS_LLF;
    if (pkg.recon != APK_RC_DC) throw std::runtime_error("LLF Riemann solver only implemented with DC reconstruction.");
  } else if (riemann == "hlle") {
    pkg.riemann = APK_RS_HLLE;
  } else if (riemann == "hllc") {
    pkg.riemann = APK_RS_HLLC;
  } else if (riemann == "hlld") {
    pkg.riemann = APK_RS_HLLD;
  } else if (riemann == "none") {
    pkg.riemann = APK_RS_NONE;
    pkg.calc_dt_hyp = false;
    if (pkg.recon != APK_RC_DC) throw std::runtime_error("'none' Riemann solver only supported with DC reconstruction.");
  } else {
    throw std::runtime_error("AthenaPK hydro: Unknown riemann solver.");
  }
  if (pin.DoesParameterExist("hydro", "calc_dt_hyp")) pkg.calc_dt_hyp = pin.GetBoolean("hydro", "calc_dt_hyp");
  // registry check (flux_functions.at(...) throws in the reference, hydro.cpp:420)
  const bool hydro_ok = pkg.fluid == APK_FLUID_EULER && (pkg.riemann == APK_RS_HLLE || pkg.riemann == APK_RS_HLLC);
  const bool mhd_ok = pkg.fluid == APK_FLUID_GLMMHD && (pkg.riemann == APK_RS_HLLE || pkg.riemann == APK_RS_HLLD);
  if (!(hydro_ok || mhd_ok || pkg.riemann == APK_RS_LLF || pkg.riemann == APK_RS_NONE))
    throw std::runtime_error("AthenaPK hydro: no flux function for this fluid/riemann combination");

  const int nghost = pin.GetInteger("parthenon/mesh", "nghost");
  if (nghost < need_ng) throw std::runtime_error("AthenaPK hydro: Need more ghost zones for chosen reconstruction.");

  const std::string integ = pin.GetString("parthenon/time", "integrator");
  pkg.flux_other_stage = {pkg.fluid, pkg.recon, pkg.riemann};
  pkg.flux_first_stage = pkg.flux_other_stage;
  // Parthenon low-storage integrator coefficients
  if (integ == "rk1") {
    pkg.integrator = APK_INT_RK1;
    s->nstages = 1;
    s->beta[0] = 1.0, s->gam0[0] = 0.0, s->gam1[0] = 1.0;
  } else if (integ == "rk2") {
    pkg.integrator = APK_INT_RK2;
    s->nstages = 2;
    s->beta[0] = 1.0, s->gam0[0] = 0.0, s->gam1[0] = 1.0;
    s->beta[1] = 0.5, s->gam0[1] = 0.5, s->gam1[1] = 0.5;
  } else if (integ == "rk3") {
    pkg.integrator = APK_INT_RK3;
    s->nstages = 3;
    s->beta[0] = 1.0, s->gam0[0] = 0.0, s->gam1[0] = 1.0;
    s->beta[1] = 0.25, s->gam0[1] = 0.25, s->gam1[1] = 0.75;
    s->beta[2] = 2.0 / 3.0, s->gam0[2] = 2.0 / 3.0, s->gam1[2] = 1.0 / 3.0;
  } else if (integ == "vl2") {
    pkg.integrator = APK_INT_VL2;
    s->nstages = 2;
    s->beta[0] = 0.5, s->gam0[0] = 0.0, s->gam1[0] = 1.0;
    s->beta[1] = 1.0, s->gam0[1] = 0.0, s->gam1[1] = 1.0;
    // override first stage (predictor) to first order (hydro.cpp:457-463)
    pkg.flux_first_stage = {pkg.fluid, APK_RC_DC, pkg.riemann};
  } else {
    throw std::runtime_error("unknown integrator: " + integ);
  }
  pkg.first_order_flux_correct = pin.GetOrAddBoolean("hydro", "first_order_flux_correct", false);

  const std::string eos = pin.GetString("hydro", "eos");
  if (eos != "adiabatic") throw std::runtime_error("AthenaPK hydro: Unknown EOS");
  pkg.eos.gamma = pin.GetReal("hydro", "gamma");
  pkg.eos.dfloor = pin.GetOrAddReal("hydro", "dfloor", -1.0);
  pkg.eos.pfloor = pin.GetOrAddReal("hydro", "pfloor", -1.0);
  units_initialize(s);
  // temperature floor and ceiling as specific internal energies (hydro.cpp:509-536)
  const double Tfloor = pin.GetOrAddReal("hydro", "Tfloor", -1.0);
  double efloor = Tfloor;
  if (efloor > 0.0) {
    if (!pkg.units.has_composition)
      throw std::runtime_error("Temperature floor requires units and gas composition. Either set a 'units' block and the "
                               "'hydro/He_mass_fraction' in input file or use a pressure floor (defined code units) instead.");
    efloor = Tfloor / pkg.units.mbar_over_kb / (pkg.eos.gamma - 1.0);
  }
  pkg.eos.efloor = efloor;
  pkg.eos.vceil = pin.GetOrAddReal("hydro", "vceil", std::numeric_limits<double>::infinity());
  const double Tceil = pin.GetOrAddReal("hydro", "Tceil", std::numeric_limits<double>::infinity());
  double eceil = Tceil;
  if (eceil < std::numeric_limits<double>::infinity()) {
    if (!pkg.units.has_composition)
      throw std::runtime_error("Temperature ceiling requires units and gas composition. Either set a 'units' block and the "
                               "'hydro/He_mass_fraction' in input file or use a pressure floor (defined code units) instead.");
    eceil = Tceil / pkg.units.mbar_over_kb / (pkg.eos.gamma - 1.0);
  }
  pkg.eos.eceil = eceil;
  pkg.nscalars = pin.GetOrAddInteger("hydro", "nscalars", 0);
  if (pkg.nscalars < 0) throw std::runtime_error("hydro/nscalars must be >= 0");
  diffusion_initialize(s);
  cooling_initialize(s);
}

// <diffusion> (src/hydro/hydro.cpp:538-702): the fixed-coefficient processes and Spitzer conduction.  What this
// path does not implement is refused instead of being ignored: a deck that asks for diffusion must not run inviscid.
void diffusion_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  HydroPackage &pkg = s->pkg;
  apk_diff_cfg &c = pkg.diff;
  c = apk_diff_cfg{};
  pkg.spitzer = apk_spitzer_cfg{};
  const std::string conduction = pin.GetOrAddString("diffusion", "conduction", "none");
  if (conduction == "isotropic") c.conduction = APK_COND_ISOTROPIC;
  else if (conduction == "anisotropic") c.conduction = APK_COND_ANISOTROPIC;
  else if (conduction != "none") throw std::runtime_error("Unknown conduction method. Options are: none, isotropic, anisotropic");
  if (c.conduction != APK_COND_NONE) {
    const std::string coeff = pin.GetOrAddString("diffusion", "conduction_coeff", "none");
    const double sat_phi = pin.GetOrAddReal("diffusion", "conduction_sat_phi", 0.3);
    if (coeff == "spitzer") {
      const UnitsState &u = pkg.units;
      if (!u.has_composition)
        throw std::runtime_error("Spitzer thermal conduction requires units and gas composition. Please set a 'units' "
                                 "block and the 'hydro/He_mass_fraction' in the input file.");
      c.conduction_coeff = APK_CONDC_SPITZER;
      // default: a fully ionized hydrogen plasma with a Coulomb logarithm of 40, 1.84e-5 / ln Lambda = 4.6e-7; to code
      // units with no temperature conversion, [T_phys] = [T_code] (hydro.cpp:575-581)
      double spitzer_coeff = pin.GetOrAddReal("diffusion", "spitzer_cond_in_erg_by_s_K_cm", 4.6e-7);
      spitzer_coeff *= u.erg() / (u.s() * u.cm());
      pkg.spitzer = apk_spitzer_cfg{spitzer_coeff, u.mbar, u.k_boltzmann()};
      c.conduction_sat_prefac = 6.86 * std::sqrt(u.mu) * sat_phi;  // eq (7) of Cowie & McKee 1977, T_e = T_i (hydro.cpp:589-593)
    } else if (coeff == "fixed") {
      c.conduction_coeff = APK_CONDC_FIXED;
      c.thermal_diff_coeff = pin.GetReal("diffusion", "thermal_diff_coeff_code");
      c.conduction_sat_prefac = 5.0 * sat_phi;  // eq (8) of Cowie & McKee 1977 (hydro.cpp:595-604)
    } else {
      throw std::runtime_error("Thermal conduction is enabled but no coefficient is set. Please set "
                               "diffusion/conduction_coeff to either 'spitzer' or 'fixed'");
    }
    if (c.conduction_sat_prefac == 0.0) throw std::runtime_error("Saturated thermal conduction prefactor uninitialized.");
  }
  const std::string viscosity = pin.GetOrAddString("diffusion", "viscosity", "none");
  if (viscosity == "isotropic") c.viscosity = APK_VISC_ISOTROPIC;
  else if (viscosity != "none") throw std::runtime_error("Unknown viscosity method. Options are: none, isotropic");
  if (c.viscosity != APK_VISC_NONE) {
    if (pin.GetOrAddString("diffusion", "viscosity_coeff", "none") != "fixed")
      throw std::runtime_error("Viscosity is enabled but no coefficient is set. Please set diffusion/viscosity_coeff to "
                               "'fixed' and diffusion/mom_diff_coeff_code to the desired value.");
    c.viscosity_coeff = APK_VISCC_FIXED;
    c.mom_diff_coeff = pin.GetReal("diffusion", "mom_diff_coeff_code");
  }
  const std::string resistivity = pin.GetOrAddString("diffusion", "resistivity", "none");
  if (resistivity == "ohmic") c.resistivity = APK_RES_OHMIC;
  else if (resistivity != "none") throw std::runtime_error("Unknown resistivity method. Options are: none, ohmic");
  if (c.resistivity != APK_RES_NONE) {
    const std::string coeff = pin.GetOrAddString("diffusion", "resistivity_coeff", "none");
    if (coeff == "spitzer") throw std::runtime_error("Spitzer resistivity is not implemented (in the reference neither).");
    if (coeff != "fixed")
      throw std::runtime_error("Resistivity is enabled but no coefficient is set. Please set diffusion/resistivity_coeff "
                               "to 'fixed' and diffusion/ohm_diff_coeff_code to the desired value.");
    c.resistivity_coeff = APK_RESC_FIXED;
    c.ohm_diff_coeff = pin.GetReal("diffusion", "ohm_diff_coeff_code");
  }
  const std::string integrator = pin.GetOrAddString("diffusion", "integrator", "none");
  if (integrator == "unsplit") pkg.diffint = APK_DIFFINT_UNSPLIT;
  else if (integrator == "rkl2") {
    pkg.diffint = APK_DIFFINT_RKL2;
    pkg.rkl2_max_dt_ratio = pin.GetOrAddReal("diffusion", "rkl2_max_dt_ratio", -1.0);
    // (a deviation: the reference runs rkl2 without a ratio too, one uncapped step under Parthenon's dt_ceil, which this
    // driver does not have -- the mode its own documentation warns about)
    if (!(pkg.rkl2_max_dt_ratio > 0.0))
      throw std::runtime_error("diffusion/integrator = rkl2 (super-time-stepping) is not supported without a positive "
                               "diffusion/rkl2_max_dt_ratio; set it (the reference's tests use 200) or use unsplit.");
  }
  else if (integrator == "none") pkg.diffint = APK_DIFFINT_NONE;
  else throw std::runtime_error("AthenaPK unknown integration method for diffusion processes. Options are: none, unsplit, rkl2");
  // as in Athena++ a cfl safety factor is applied to the theoretical limit, by default the hyperbolic cfl
  if (pkg.diffint != APK_DIFFINT_NONE) pkg.cfl_diff = pin.GetOrAddReal("diffusion", "cfl", pkg.cfl);
  if (!pkg.diffusion_configured()) return;
  if (pkg.fluid == APK_FLUID_EULER && (c.resistivity != APK_RES_NONE || c.conduction == APK_COND_ANISOTROPIC))
    throw std::runtime_error("Ohmic resistivity and anisotropic conduction need hydro/fluid = glmmhd.");
  if (pkg.riemann == APK_RS_LLF)
    throw std::runtime_error("Diffusion with hydro/riemann = llf is not supported: the reference's (dc, llf) flux "
                             "function (CalculateFluxesTight) adds no diffusive fluxes.");
  if (pin.GetOrAddString("parthenon/mesh", "refinement", "none") != "none")
    throw std::runtime_error("Diffusion on refined meshes is not supported: parthenon/mesh/refinement must be none.");
  // (not a reference parameter: which form an RKL2 sub-stage takes -- the fused kernel, or the reference's sequence of
  // passes over the flux arrays, the default until the fused kernel has been timed below them)
  const std::string substage = pin.GetOrAddString("apk_amd", "sts_substage", "arrays");
  if (substage != "fused" && substage != "arrays") throw std::runtime_error("apk_amd/sts_substage must be fused or arrays");
  s->sts_fused = substage == "fused";
}

void mesh_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  Mesh &m = s->mesh;
  const char *nxk[3] = {"nx1", "nx2", "nx3"};
  const char *mink[3] = {"x1min", "x2min", "x3min"}, *maxk[3] = {"x1max", "x2max", "x3max"};
  const char *ibc[3] = {"ix1_bc", "ix2_bc", "ix3_bc"}, *obc[3] = {"ox1_bc", "ox2_bc", "ox3_bc"};
  for (int d = 0; d < 3; ++d) {
    m.nx[d] = pin.GetOrAddInteger("parthenon/mesh", nxk[d], 1);
    m.mb[d] = pin.GetOrAddInteger("parthenon/meshblock", nxk[d], m.nx[d]);
    s->xmin[d] = pin.GetOrAddReal("parthenon/mesh", mink[d], -0.5);
    s->xmax[d] = pin.GetOrAddReal("parthenon/mesh", maxk[d], 0.5);
    s->dx[d] = (s->xmax[d] - s->xmin[d]) / (double)m.nx[d];
    m.bc_in[d] = parse_bc(pin.GetOrAddString("parthenon/mesh", ibc[d], "periodic"));
    m.bc_out[d] = parse_bc(pin.GetOrAddString("parthenon/mesh", obc[d], "periodic"));
  }
  const std::string refinement = pin.GetOrAddString("parthenon/mesh", "refinement", "none");
  if (refinement != "none" && refinement != "static" && refinement != "adaptive")
    throw std::runtime_error("parthenon/mesh/refinement must be none, static or adaptive");
  m.ng = pin.GetInteger("parthenon/mesh", "nghost");
  m.nvar = s->pkg.nhydro + s->pkg.nscalars;
  m.rank = s->rank;
  m.nranks = s->nranks;
  // (not a reference parameter: the one-GPU rehearsal of a rank of the 2 x 2 x 2 run, mesh.hpp "rehearse")
  m.rehearse = pin.GetOrAddBoolean("apk_amd", "rehearse_remote_faces", false) ? 1 : 0;
  if (m.rehearse && refinement != "none") throw std::runtime_error("apk_amd/rehearse_remote_faces needs a uniform mesh");
  // (not a reference parameter either: rows of the block arrays at a cache-line pitch, interior cells line-aligned --
  // uniform meshes without the turbulence driver, whose acceleration field has its own layout)
  // natural | aligned | auto (default).  auto = aligned where it was measured to pay (profiles/r06_row_pitch_ab.txt: the
  // nine-variable GLM-MHD marches on 128-cell rows, -0.7 .. -1.4 % per cycle; hydro PLM+HLLC with its outflow boundary
  // copies +0.8 %): 3-D GLM-MHD on blocks whose rows are whole lines.
  const std::string row_pitch = pin.GetOrAddString("apk_amd", "row_pitch", std::getenv("APK_ROW_PITCH") ? std::getenv("APK_ROW_PITCH") : "auto");
  if (row_pitch != "natural" && row_pitch != "aligned" && row_pitch != "auto") throw std::runtime_error("apk_amd/row_pitch must be natural, aligned or auto");
  const bool can_pad = refinement == "none" && s->problem_id != "turbulence";
  const bool pays = s->pkg.fluid == APK_FLUID_GLMMHD && m.mb[2] > 1 && m.mb[0] % 16 == 0 && m.mb[0] >= 64;
  if (can_pad && (row_pitch == "aligned" || (row_pitch == "auto" && pays))) {
    m.pitch = (m.mb[0] + 2 * m.ng + 15) / 16 * 16;
    m.lead = (16 - m.ng % 16) % 16;
  }
  m.Build();
  s->nblk = m.sn * m.nvar;
  s->nper = m.lead == 0 && m.pitch == 0 ? s->nblk : (s->nblk + m.lead + 15) / 16 * 16;
  if (refinement != "none") amr_initialize(s, refinement == "adaptive");
  s->tlim = pin.GetOrAddReal("parthenon/time", "tlim", 1.0);
  s->nlim = pin.GetOrAddInteger("parthenon/time", "nlim", -1);
}

// ---- device resources -----------------------------------------------------------------------
int dev_alloc(apk_sim *s, const char *tag, size_t bytes, double **out) {
  *out = nullptr;
  if (bytes == 0) return APK_OK;
  if (s->have_alloc) {
    *out = static_cast<double *>(s->alloc.alloc(s->alloc.user, tag, bytes));
    if (!*out) return fail(s, APK_ERR_DEVICE, std::string("allocator returned NULL for ") + tag);
    return APK_OK;
  }
  SIM_HIP(s, hipMalloc(out, bytes));
  return APK_OK;
}
void dev_free(apk_sim *s, double *p) {
  if (!p) return;
  if (s->have_alloc) {
    if (s->alloc.release) s->alloc.release(s->alloc.user, p);
  } else {
    (void)hipFree(p);
  }
}

int build_packs(apk_sim *s) {
  const int nlb = (int)s->mesh.local_gids.size();
  for (int p = 0; p < 3; ++p)
    for (int w = 0; w < 2; ++w) {
      if (s->mu0_of[p][w]) apk_pack_destroy(s->mu0_of[p][w]);
      if (s->mu1_of[p][w]) apk_pack_destroy(s->mu1_of[p][w]);
      s->mu0_of[p][w] = s->mu1_of[p][w] = nullptr;
      if (!s->d_prim2[w] || !s->d_cons2[p]) continue;
      double *spare = s->d_prim2[1 - w];  // may be null: then u1 carries no prim
      std::vector<apk_block_desc> b0(nlb), b1(nlb);
      for (int lb = 0; lb < nlb; ++lb) {
        b0[lb].cons = s->blk(s->d_cons2[p], lb);
        b0[lb].prim = s->blk(s->d_prim2[w], lb);
        b1[lb].cons = s->blk(s->d_cons2[p], lb);
        b1[lb].prim = spare ? s->blk(spare, lb) : nullptr;
        for (int d = 0; d < 3; ++d) {
          b0[lb].flux[d] = s->d_flux[d] ? s->blk(s->d_flux[d], lb) : nullptr;
          b1[lb].flux[d] = nullptr;
          b0[lb].dx[d] = b1[lb].dx[d] = level_dx(s, block_level(s, lb), d);
        }
      }
      apk_pack_desc d{};
      d.nblocks = nlb;
      d.nhydro = s->pkg.nhydro;
      d.nscalars = s->pkg.nscalars;
      for (int q = 0; q < 3; ++q) d.nx[q] = s->mesh.mb[q];
      d.ng = s->mesh.ng;
      if (s->mesh.pitch > 0) {
        d.stride[0] = s->mesh.sj;
        d.stride[1] = s->mesh.sk;
        d.stride[2] = s->mesh.sn;
      }
      d.blocks = b0.data();
      SIM_TRY(s, apk_pack_create(s->ctx, &d, &s->mu0_of[p][w]));
      d.blocks = b1.data();
      SIM_TRY(s, apk_pack_create(s->ctx, &d, &s->mu1_of[p][w]));
    }
  return APK_OK;
}

// third conserved buffer (output of trial stages that must keep their input), on first use
int ensure_trial_cons(apk_sim *s) {
  if (s->d_cons2[2]) return APK_OK;
  const size_t bytes = (size_t)s->nper * s->mesh.local_gids.size() * sizeof(double);
  SIM_TRY(s, dev_alloc(s, "cons3", bytes, &s->d_cons2[2]));
  SIM_HIP(s, hipMemsetAsync(s->d_cons2[2], 0, bytes, hs(s)));
  SIM_TRY(s, build_packs(s));
  return build_copy_plans(s);
}

// second primitive buffer, on first use
int ensure_spare_prim(apk_sim *s) {
  if (s->d_prim2[1 - s->pcur]) return APK_OK;
  const size_t bytes = (size_t)s->nper * s->mesh.local_gids.size() * sizeof(double);
  SIM_TRY(s, dev_alloc(s, "prim2", bytes, &s->d_prim2[1 - s->pcur]));
  SIM_HIP(s, hipMemsetAsync(s->d_prim2[1 - s->pcur], 0, bytes, hs(s)));
  SIM_TRY(s, build_packs(s));
  return build_prim_plans(s);
}

int ensure_flux_arrays(apk_sim *s) {
  bool changed = false;
  const size_t bytes = (size_t)s->nper * s->mesh.local_gids.size() * sizeof(double);
  const char *tags[3] = {"flux1", "flux2", "flux3"};
  for (int d = 0; d < s->mesh.ndim; ++d) {
    if (!s->d_flux[d]) {
      SIM_TRY(s, dev_alloc(s, tags[d], bytes, &s->d_flux[d]));
      SIM_HIP(s, hipMemsetAsync(s->d_flux[d], 0, bytes, hs(s)));
      changed = true;
    }
  }
  if (changed || !s->mu0()) return build_packs(s);
  return APK_OK;
}

bool stage_can_fuse(const apk_sim *s) {
  // (refined meshes included: the coarse-fine flux correction is applied after the fused stage from
  // boundary-plane fluxes, see amr_flux_fix)
  // (diffusion: the stages run through the flux arrays, whose face fluxes the diffusive ones are added to; cooling and
  // the cluster's gravity: the source acts between the update and ConsToPrim, which the fused stages do in one sweep)
  return s->fused && !s->pkg.first_order_flux_correct && s->pkg.riemann != APK_RS_NONE &&
         s->pkg.riemann != APK_RS_LLF && !s->pkg.flux_path_sources();
}

// the plans of one field buffer (`field`: the first block's array; blocks follow at nper doubles)
static int make_plans(apk_sim *s, double *field, apk_copy_plan *(&out)[PH_COUNT]) {
  for (int ph = 0; ph < PH_COUNT; ++ph) {
    if (out[ph]) {
      apk_copy_plan_destroy(out[ph]);
      out[ph] = nullptr;
    }
    if (!field) continue;
    std::vector<apk_copy_region> regs;
    auto base = [&](int kind, int block) -> double * {
      if (kind == RK_BLOCK) return s->blk(field, block);
      return kind == RK_SEND ? s->send_buf[block] : s->recv_buf[block];
    };
    for (const BoxRegion &r : s->mesh.plan[ph]) {
      apk_copy_region c{};
      c.src = base(r.src_kind, r.src_block) + r.src_off;
      c.dst = base(r.dst_kind, r.dst_block) + r.dst_off;
      for (int q = 0; q < 3; ++q) c.ext[q] = r.ext[q];
      c.nvar = r.nvar;
      for (int q = 0; q < 4; ++q) {
        c.src_stride[q] = r.src_stride[q];
        c.dst_stride[q] = r.dst_stride[q];
      }
      c.flip_var = r.flip_var;
      regs.push_back(c);
    }
    SIM_TRY(s, apk_copy_plan_create(s->ctx, regs.data(), (int)regs.size(), &out[ph]));
  }
  return APK_OK;
}

int build_copy_plans(apk_sim *s) {
  for (int par = 0; par < 3; ++par) SIM_TRY(s, make_plans(s, s->d_cons2[par], s->plans_of[par]));
  return build_prim_plans(s);
}

// (exchanges of stored primitives -- GHOST_PRIM_COPY -- only happen on uniform meshes with remote neighbours or
// same-rank copies: nothing to build where no plan has a region)
int build_prim_plans(apk_sim *s) {
  for (int w = 0; w < 2; ++w) SIM_TRY(s, make_plans(s, s->amr ? nullptr : s->d_prim2[w], s->pplans_of[w]));
  return APK_OK;
}

// EvolutionDriver::SetGlobalTimeStep
void set_global_dt(apk_sim *s, double dt_est) {
  double dt = s->dt;
  if (dt < 0.1 * kHuge) dt *= 2.0;
  if (dt_est < dt) dt = dt_est;
  if (s->time < s->tlim && (s->tlim - s->time) < dt) dt = s->tlim - s->time;
  s->dt = dt;
}

// Hydro::EstimateTimestep<fluid> over this rank's pack + global min (hydro.cpp:913-977)
// The time-step estimate in two halves (round-2 advisor finding: a regridding pass between "measure" and
// "use" must not inherit side effects of an estimate made on the old mesh).
//   _read    device work + ONE host round trip: the local minimum and the device flag word.  Consumes the
//            finishing sweep's pending reduction; touches nothing of the package.
//   _commit  the reference's reaction to the flags (PARTHENON_REQUIRE in ConsToPrim), the reduction over
//            ranks, and the hyperbolic estimate the next cycle's c_h needs (hydro.cpp:102-143, 903-908).
int estimate_timestep_read(apk_sim *s, DtEstimate *e) {
  double dt = kHuge;
  unsigned flags = 0;
  bool have_flags = false;
  if (s->pkg.calc_dt_hyp) {
    if (s->stage_dt_pending) {  // already reduced by the finishing sweep of the last stage
      SIM_TRY(s, apk_stage_dt_flags_read(s->ctx, s->pkg.cfl, &dt, &flags, s->stream));  // one host round trip
      have_flags = true;
      s->stage_dt_pending = false;
    } else {
      if (s->prim_stale) SIM_TRY(s, sync_ghosts(s));  // (the estimate reads stored primitives)
      SIM_TRY(s, apk_estimate_timestep(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, s->pkg.cfl, &dt, s->stream));
    }
  }
  if (!have_flags) SIM_TRY(s, apk_poll_device_flags(s->ctx, &flags, s->stream));
  e->dt_hyp_local = dt;
  // the diffusive limit (hydro.cpp:935-963; unsplit: min_dt = min(dt_hyp, dt_diff); rkl2: see estimate_timestep_commit)
  if (s->pkg.diffusion_configured()) {
    if (s->prim_stale) SIM_TRY(s, sync_ghosts(s));  // (the estimate reads stored primitives)
    SIM_TRY(s, apk_estimate_diffusion_timestep_v2(s->ctx, s->mu0(), &s->pkg.diff, s->pkg.spitzer_cfg(), s->pkg.cfl_diff,
                                                  &e->dt_diff_local, s->stream));
  }
  // the cooling limit (hydro.cpp:926-933): joins min_dt, not dt_hyp (so c_h is untouched)
  if (s->pkg.cooling) {
    if (s->prim_stale) SIM_TRY(s, sync_ghosts(s));  // (the estimate reads stored primitives)
    SIM_TRY(s, apk_estimate_cooling_timestep(s->ctx, s->mu0(), s->cool_tab, &e->dt_cool_local, s->stream));
    unsigned more = 0;  // (what the source term latched since the stage's read)
    SIM_TRY(s, apk_poll_device_flags(s->ctx, &more, s->stream));
    flags |= more;
  }
  e->flags |= flags;  // (flags latched before an earlier read of the same cycle stay raised)
  return APK_OK;
}

int estimate_timestep_commit(apk_sim *s, const DtEstimate &e, double *dt_out) {
  const bool sts = s->pkg.diffusion_sts();
  // (rkl2: dt_diff does not join min_dt directly, hydro.cpp:950-956)
  double dt = std::min(std::min(e.dt_hyp_local, sts ? kHuge : e.dt_diff_local), e.dt_cool_local);
  // the triggering limit (cluster.cpp:95-107 through ProblemEstimateTimestep): joins min_dt, not dt_hyp.  It follows from
  // the globally reduced quantities: the same number on every rank
  if (s->pkg.agn_triggering) dt = std::min(dt, s->trig.estimate_timestep(s->trig_q));
  if (s->pkg.max_dt > 0.0 && s->pkg.max_dt < dt) dt = s->pkg.max_dt;
  // one reduction for both minima: the time step, and the hyperbolic estimate that the next cycle's
  // c_h needs (hydro.cpp:102-143 reduces it in PreStepMeshUserWorkInLoop; same value, one message less).
  // The negative-state flags travel with them (two more slots, MIN of -1 / 0): a rank that latched a flag must not
  // leave the collective to its peers -- every rank takes part, then every rank fails.
  // With cooling two more: the flags of its device failures, and the table's fingerprint (as x and -x) -- every rank
  // must integrate with the same table.
  const bool cool = s->pkg.cooling;
  const double h = s->pkg.cool_table_hash;
  // With rkl2 one more, last: the diffusive limit itself, which sizes the next cycle's super-time-steps.
  // (the AGN feedback source's own pressure check and stellar feedback's energy check share the pressure slot: -3 and -2
  // below -1, so that every rank sees which; the reference meets the AGN one first)
  double mins[8] = {dt, e.dt_hyp_local, (e.flags & APK_FLAG_NEG_DENSITY) ? -1.0 : 0.0,
                    (e.flags & APK_FLAG_AGN_NEG_PRESSURE) ? -3.0 : ((e.flags & APK_FLAG_STELLAR_ENERGY) ? -2.0 : ((e.flags & APK_FLAG_NEG_PRESSURE) ? -1.0 : 0.0)),
                    (e.flags & (APK_FLAG_COOL_MAX_ITER | APK_FLAG_COOL_TABLE)) ? -1.0 : 0.0, h, -h, e.dt_diff_local};
  if (s->have_comm && s->nranks > 1) {
    if (s->comm.allreduce_min(s->comm.user, mins, sts ? 8 : (cool ? 7 : 4)) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_min failed");
  }
  if (cool && mins[5] != -mins[6]) return fail(s, APK_ERR_INVALID, "cooling: the ranks read different cooling tables");
  if (cool && mins[4] < 0.0) {
    if (e.flags & APK_FLAG_COOL_MAX_ITER)
      return fail(s, APK_ERR_INVALID, "FATAL ERROR in [TabularCooling::SubcyclingFixedIntSrcTerm]: Sub cycles exceed max_iter (This should be impossible)");
    if (e.flags & APK_FLAG_COOL_TABLE) return fail(s, APK_ERR_INVALID, "FATAL ERROR in [CoolingTable::DeDt]: Failed to find log_temp");
    return fail(s, APK_ERR_INVALID, "cooling failed on another rank");
  }
  // agn_feedback.cpp:407-408: the reference aborts inside the source's loop, before any later ConsToPrim can complain
  if (mins[3] <= -3.0) return fail(s, APK_ERR_INVALID, "Kinetic injection leads to negative pressure");
  // stellar_feedback.cpp:163-165
  if (mins[3] <= -2.0) return fail(s, APK_ERR_INVALID, "Sanity check failed. Added thermal energy should be positive.");
  if (mins[2] < 0.0)
    return fail(s, APK_ERR_INVALID, "Got negative density. Consider enabling first-order flux correction or setting a reasonble density floor.");
  if (mins[3] < 0.0)
    return fail(s, APK_ERR_INVALID, "Got negative pressure. Consider enabling first-order flux correction or setting a reasonble pressure or temperature floor.");
  if (s->pkg.calc_dt_hyp && s->pkg.fluid == APK_FLUID_GLMMHD && mins[1] < s->pkg.dt_hyp) s->pkg.dt_hyp = mins[1];  // hydro.cpp:903-908
  s->dt_hyp_is_global = true;
  if (sts) {
    // hydro.cpp:950-962.  The reference evaluates this condition per partition, on that partition's dt_hyp and dt_diff;
    // here it is evaluated once on the globally reduced pair, so that the step does not depend on the decomposition
    // (identical for one partition).  Without a hyperbolic estimate (riemann = none) dt_hyp is huge and the cap alone
    // sets the step.
    s->pkg.dt_diff = mins[7];
    const double ratio = s->pkg.rkl2_max_dt_ratio;
    if (mins[1] / mins[7] > ratio) mins[0] = std::min(mins[0], ratio * mins[7]);
  }
  *dt_out = mins[0];
  return APK_OK;
}

int estimate_timestep(apk_sim *s, double *dt_out) {
  DtEstimate e;
  SIM_TRY(s, estimate_timestep_read(s, &e));
  return estimate_timestep_commit(s, e, dt_out);
}

// the per-block segment tables of apk_stage_args.x1_halo (apk_sim::d_x1_tab), from Mesh::x1_send / x1_recv
int build_x1_tables(apk_sim *s) {
  const Mesh &m = s->mesh;
  if (m.peers.empty() || m.ndim != 3) return APK_OK;
  const size_t nlb = m.local_gids.size();
  std::vector<apk_x1_halo_block> pred(nlb), corr(nlb), full(nlb);
  for (size_t lb = 0; lb < nlb; ++lb)
    for (int side = 0; side < 2; ++side) {
      const X1Segment &sd = m.x1_send[lb][side], &rv = m.x1_recv[lb][side];
      pred[lb].send[side] = sd.peer >= 0 ? s->send_buf[sd.peer] + sd.off : nullptr;
      corr[lb].send[side] = sd.peer >= 0 ? s->send_buf[sd.peer] + sd.off_thin : nullptr;
      pred[lb].recv[side] = rv.peer >= 0 ? s->recv_buf[rv.peer] + rv.off_thin : nullptr;
      corr[lb].recv[side] = rv.peer >= 0 ? s->recv_buf[rv.peer] + rv.off : nullptr;
      full[lb].send[side] = pred[lb].send[side];  // (the RK integrators: full messages both ways)
      full[lb].recv[side] = corr[lb].recv[side];
    }
  const char *tags[3] = {"x1_halo_predictor", "x1_halo_corrector", "x1_halo_full"};
  const std::vector<apk_x1_halo_block> *tabs[3] = {&pred, &corr, &full};
  for (int q = 0; q < 3; ++q) {
    double *p = nullptr;
    SIM_TRY(s, dev_alloc(s, tags[q], sizeof(apk_x1_halo_block) * nlb, &p));
    s->d_x1_tab[q] = p;
    SIM_HIP(s, hipMemcpy(p, tabs[q]->data(), sizeof(apk_x1_halo_block) * nlb, hipMemcpyHostToDevice));
  }
  return APK_OK;
}


// index windows of the split stages, per local block (see apk_stage_args.window)
int upload_window(apk_sim *s, const char *tag, const std::vector<int> &w, apk_sim::WindowTable &t) {
  const size_t nlb = w.size() / 8;
  t.rl = t.rows = 0;
  t.any = false;
  for (size_t lb = 0; lb < nlb; ++lb) {
    const int *q = &w[8 * lb];
    if (q[1] <= 0 || q[3] < q[2] || q[5] < q[4] || q[7] < q[6]) continue;
    t.any = true;
    t.rl = std::max(t.rl, q[1]);
    t.rows = std::max(t.rows, q[5] - q[4] + 1);
  }
  double *p = nullptr;
  SIM_TRY(s, dev_alloc(s, tag, sizeof(int) * w.size(), &p));
  t.d = reinterpret_cast<int *>(p);
  SIM_HIP(s, hipMemcpy(t.d, w.data(), sizeof(int) * w.size(), hipMemcpyHostToDevice));
  return APK_OK;
}

int build_windows(apk_sim *s) {
  const Mesh &m = s->mesh;
  const int nlb = (int)m.local_gids.size();
  const int W = m.ng;
  auto put = [](std::vector<int> &t, int lb, int i0, int rl, int ilo, int ihi, int jlo, int jhi, int klo, int khi) {
    int *q = &t[8 * (size_t)lb];
    q[0] = i0, q[1] = rl, q[2] = ilo, q[3] = ihi, q[4] = jlo, q[5] = jhi, q[6] = klo, q[7] = khi;
  };
  std::vector<int> x1[3], k3[3];
  for (auto &t : x1) t.assign(8 * (size_t)nlb, 0);
  for (auto &t : k3) t.assign(8 * (size_t)nlb, 0);
  std::vector<unsigned> late(nlb, 0u);
  // (two-kernel stage: when no block has BOTH its x3 faces late -- the 2 x 2 x 2 brick: every block is a corner -- the
  // low and the high slabs are one table, one launch with twice the waves: a slab launch of half the blocks fills half
  // the GPU for the length of a whole march prologue)
  bool k3_one_slab = true;
  for (int lb = 0; lb < nlb; ++lb)
    if (m.Active(2) && m.LateFace(lb, 2, -1) && m.LateFace(lb, 2, +1)) k3_one_slab = false;
  for (int lb = 0; lb < nlb; ++lb) {
    // "late" faces: ghost zones filled by messages of other ranks (physical boundaries are applied after them)
    int L[3][2];
    for (int d = 0; d < 3; ++d) L[d][0] = (m.Active(d) && m.LateFace(lb, d, -1)) ? 1 : 0;
    for (int d = 0; d < 3; ++d) L[d][1] = m.LateFace(lb, d, +1) ? 1 : 0;
    // x1 sweep of a high-order stage: everything farther than nghost from a late x1 face, then the slabs
    put(x1[0], lb, 0, m.ni, m.is + W * L[0][0], m.ie - W * L[0][1], m.js, m.je, m.ks, m.ke);
    // (two columns of margin on the left: the L state of the cell below the first retired one needs, with
    // PPM's shared interface values, the lane below it as well -- x1_first_lane in fused_kernel.hpp)
    put(x1[1], lb, m.is - 2, L[0][0] ? W + 3 : 0, m.is, m.is + W - 1, m.js, m.je, m.ks, m.ke);
    put(x1[2], lb, m.ie - W - 1, L[0][1] ? W + 3 : 0, m.ie - W + 1, m.ie, m.js, m.je, m.ks, m.ke);
    // two-kernel stage (3-D): its first kernel is the x3 sweep, which reads x3 ghost zones only --
    // every plane farther than nghost from a late x3 face, then the slabs next to those faces
    put(k3[0], lb, 0, m.ni, m.is, m.ie, m.js, m.je, m.ks + W * L[2][0], m.ke - W * L[2][1]);
    if (k3_one_slab) {
      const bool hi = L[2][1] != 0;
      put(k3[1], lb, 0, (L[2][0] || L[2][1]) ? m.ni : 0, m.is, m.ie, m.js, m.je, hi ? m.ke - W + 1 : m.ks, hi ? m.ke : m.ks + W - 1);
      put(k3[2], lb, 0, 0, m.is, m.ie, m.js, m.je, m.ke - W + 1, m.ke);
    } else {
      put(k3[1], lb, 0, L[2][0] ? m.ni : 0, m.is, m.ie, m.js, m.je, m.ks, m.ks + W - 1);
      put(k3[2], lb, 0, L[2][1] ? m.ni : 0, m.is, m.ie, m.js, m.je, m.ke - W + 1, m.ke);
    }
    // (the single-kernel donor-cell stage of 3-D meshes is never split: an exchange in flight is completed before it)
    // lateness per neighbour region for the split ghost ConsToPrim
    int bc[3], nbc[3];
    m.Loc(m.local_gids[lb], bc);
    for (int sz = -1; sz <= 1; ++sz)
      for (int sy = -1; sy <= 1; ++sy)
        for (int sx = -1; sx <= 1; ++sx) {
          if (!sx && !sy && !sz) continue;
          if ((sx && !m.Active(0)) || (sy && !m.Active(1)) || (sz && !m.Active(2))) continue;
          const int o[3] = {sx, sy, sz};
          const bool is_late = !m.Neighbor(bc, o, nbc) || m.NeighborRank(bc, o, nbc) != m.rank;
          if (is_late) late[lb] |= 1u << ((sx + 1) + 3 * (sy + 1) + 9 * (sz + 1));
        }
  }
  {
    double *p = nullptr;
    SIM_TRY(s, dev_alloc(s, "late_regions", sizeof(unsigned) * (size_t)nlb, &p));
    s->d_late_regions = reinterpret_cast<unsigned *>(p);
    SIM_HIP(s, hipMemcpy(s->d_late_regions, late.data(), sizeof(unsigned) * (size_t)nlb, hipMemcpyHostToDevice));
  }
  const char *x1tags[3] = {"win_x1_main", "win_x1_lo", "win_x1_hi"};
  for (int q = 0; q < 3; ++q) SIM_TRY(s, upload_window(s, x1tags[q], x1[q], s->x1win[q]));
  if (m.ndim == 3) {
    const char *k3tags[3] = {"win_k3_main", "win_k3_lo", "win_k3_hi"};
    for (int q = 0; q < 3; ++q) SIM_TRY(s, upload_window(s, k3tags[q], k3[q], s->k3win[q]));
  }
  return APK_OK;
}

// apk_stage_args.face_neighbor of this rank's pack: the same-rank block behind every face, or -1
// (a physical boundary, a block of another rank: those ghost zones are filled by the exchange)
int build_face_table(apk_sim *s) {
  const Mesh &m = s->mesh;
  const int nlb = (int)m.local_gids.size();
  std::vector<int> tab(6 * (size_t)nlb, -1);
  for (int lb = 0; lb < nlb; ++lb) {
    int bc[3], nbc[3];
    m.Loc(m.local_gids[lb], bc);
    for (int d = 0; d < 3; ++d)
      for (int side = 0; side < 2; ++side) {
        int o[3] = {0, 0, 0};
        o[d] = side ? 1 : -1;
        if (!m.Active(d) || !m.Neighbor(bc, o, nbc)) continue;
        const int ngid = m.Gid(nbc);
        if (m.NeighborRank(bc, o, nbc) == m.rank) tab[6 * (size_t)lb + 2 * d + side] = m.gid_local.at(ngid);
      }
  }
  double *p = nullptr;
  SIM_TRY(s, dev_alloc(s, "face_neighbors", sizeof(int) * tab.size(), &p));
  s->d_face_nbr = reinterpret_cast<int *>(p);
  SIM_HIP(s, hipMemcpy(s->d_face_nbr, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
  return APK_OK;
}

int fill_derived(apk_sim *s) {
  return apk_cons_to_prim(s->ctx, s->mu0(), s->pkg.fluid, &s->pkg.eos, s->stream);
}

// Hydro::PreStepMeshUserWorkInLoop (hydro.cpp:102-143)
int pre_step(apk_sim *s) {
  if (!s->pkg.calc_c_h) return APK_OK;
  // CalculateGlobalMinDx (hydro.cpp:65-95): over the blocks that exist, i.e. the finest level present
  int finest = 0;
  if (s->amr)
    for (const AmrLeaf &l : s->amr->leaves) finest = std::max(finest, l.level);
  double mindx = level_dx(s, finest, 0);
  if (s->mesh.Active(1)) mindx = std::fmin(mindx, level_dx(s, finest, 1));
  if (s->mesh.Active(2)) mindx = std::fmin(mindx, level_dx(s, finest, 2));
  double mins[3] = {mindx, s->pkg.dt_hyp, kHuge};
  // (the cell widths are the same on every rank -- the forest is replicated -- and estimate_timestep
  // has reduced dt_hyp already)
  if (s->have_comm && s->nranks > 1 && !s->dt_hyp_is_global) {
    if (s->comm.allreduce_min(s->comm.user, mins, 3) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_min failed");
  }
  s->pkg.mindx = mins[0];
  s->pkg.dt_hyp = mins[1];
  s->pkg.c_h = s->pkg.cfl * s->pkg.mindx / s->pkg.dt_hyp;
  return APK_OK;
}

// acc field, per-block phase tables (FewModesFT::SetPhases, few_modes_ft.cpp:142-195) and the
// device descriptor of the driver
int turbulence_device_setup(apk_sim *s) {
  const Mesh &m = s->mesh;
  const int nlb = (int)m.local_gids.size();
  const int M = s->fmft->num_modes();
  const size_t acc_per = 3 * (size_t)m.sn;
  const size_t ph_per = (size_t)(m.mb[0] + m.mb[1] + m.mb[2]) * M * 2;
  SIM_TRY(s, dev_alloc(s, "acc", acc_per * nlb * sizeof(double), &s->d_acc));
  SIM_TRY(s, dev_alloc(s, "turbulence_phases", ph_per * nlb * sizeof(double), &s->d_phases));
  SIM_HIP(s, hipMemset(s->d_acc, 0, acc_per * nlb * sizeof(double)));
  std::vector<double> ph(ph_per * nlb);
  std::vector<apk_fmft_block> desc(nlb);
  for (int lb = 0; lb < nlb; ++lb) {
    int bc[3];
    m.Loc(m.local_gids[lb], bc);
    double *h = ph.data() + ph_per * lb;
    double *d = s->d_phases + ph_per * lb;
    size_t off = 0;
    const double *dptr[3];
    for (int ax = 0; ax < 3; ++ax) {
      s->fmft->Phases(ax, m.mb[ax], bc[ax] * m.mb[ax], m.nx[ax], h + off);
      dptr[ax] = d + off;
      off += (size_t)m.mb[ax] * M * 2;
    }
    desc[lb].acc = s->d_acc + acc_per * lb;
    desc[lb].phases_i = dptr[0];
    desc[lb].phases_j = dptr[1];
    desc[lb].phases_k = dptr[2];
  }
  SIM_HIP(s, hipMemcpy(s->d_phases, ph.data(), ph.size() * sizeof(double), hipMemcpyHostToDevice));
  SIM_TRY(s, apk_fmft_create(s->ctx, desc.data(), nlb, M, &s->fm_dev));
  return APK_OK;
}

int create_common(const char *deck, const char *const *overrides, int noverrides, int rank, int nranks,
                  apk_sim **out, char *errbuf, size_t errlen) {
  if (!out || !deck) return APK_ERR_INVALID;
  *out = nullptr;
  apk_sim *s = new (std::nothrow) apk_sim();
  if (!s) return APK_ERR_INVALID;
  s->rank = rank;
  s->nranks = nranks;
  try {
    s->pin.LoadFromString(deck);
    for (int i = 0; i < noverrides; ++i) s->pin.ApplyOverride(overrides[i]);
    s->problem_id = s->pin.GetString("job", "problem_id");
    hydro_initialize(s);
    mesh_initialize(s);
    if (s->problem_id == "linear_wave") lw_setup(s);
    else if (s->problem_id == "linear_wave_mhd") lwm_setup(s);
    else if (s->problem_id == "cpaw") cpaw_setup(s);
    else if (s->problem_id == "field_loop") field_loop_setup(s);
    else if (s->problem_id == "kh") kh_setup(s);
    else if (s->problem_id == "advection") {
      // advection::InitUserMeshData (src/pgen/advection.cpp:34-59): tlim counts box diagonals / |v|
      const double vx = s->pin.GetOrAddReal("problem/advection", "vx", 0.0), vy = s->pin.GetOrAddReal("problem/advection", "vy", 0.0),
                   vz = s->pin.GetOrAddReal("problem/advection", "vz", 0.0);
      const double L[3] = {s->xmax[0] - s->xmin[0], s->xmax[1] - s->xmin[1], s->xmax[2] - s->xmin[2]};
      const double vmag = std::sqrt(vx * vx + vy * vy + vz * vz) + 1.0e-20;  // TINY_NUMBER
      const double diag = std::sqrt(L[0] * L[0] + L[1] * L[1] + L[2] * L[2]);
      s->tlim = diag / vmag * s->tlim;
    }
    else if (s->problem_id == "lw_implode" && s->pkg.fluid == APK_FLUID_GLMMHD)
      throw std::runtime_error("Only hydro runs are supported for LW implosion problem generator.");
    else if (s->problem_id == "turbulence") turbulence_setup(s);
    else if (s->problem_id == "diffusion") diffusion_check(s);
    else if (s->problem_id == "cluster") cluster_initialize(s);
    else if (s->problem_id != "sod" && s->problem_id != "orszag_tang" && s->problem_id != "synthetic" &&
             s->problem_id != "blast" && s->problem_id != "lw_implode" && s->problem_id != "cpaw" &&
             s->problem_id != "advection" && s->problem_id != "field_loop" && s->problem_id != "kh" &&
             s->problem_id != "linear_wave" && s->problem_id != "linear_wave_mhd" && s->problem_id != "diffusion")
      throw std::runtime_error("unknown job/problem_id: " + s->problem_id);
    // src/bvals/boundary_conditions_apk.hpp:47-50 (raised when the wall is first applied, i.e. after
    // the problem generator's own checks): the wall only mirrors the normal momentum
    for (int d = 0; d < 3; ++d)
      if ((s->mesh.bc_in[d] == BC_REFLECT || s->mesh.bc_out[d] == BC_REFLECT) && s->pkg.fluid != APK_FLUID_EULER)
        throw std::runtime_error("Reflecting boundary conditions for MHD need special treatment.");
    tracers_initialize(s);  // <tracers> (after the hydro package, as the reference's Initialize order)
    snapshot_initialize(s);  // the npy output blocks (host/snapshot.cpp)
    restart_initialize(s);   // the rst output blocks and what a restart refuses (host/restart.cpp)
  } catch (const std::exception &e) {
    if (errbuf && errlen) std::snprintf(errbuf, errlen, "%s", e.what());
    delete s;
    return APK_ERR_INVALID;
  }
  *out = s;
  return APK_OK;
}


}  // namespace host
}  // namespace apk

using namespace apk::host;

extern "C" {

int apk_sim_create_host_only(const char *deck, const char *const *overrides, int noverrides, int rank,
                             int nranks, apk_sim **out, char *errbuf, size_t errlen) {
  int rc = create_common(deck, overrides, noverrides, rank, nranks, out, errbuf, errlen);
  if (rc == APK_OK) (*out)->host_only = true;
  return rc;
}

int apk_sim_create(const char *deck, const char *const *overrides, int noverrides, int rank, int nranks,
                   const apk_allocator *allocator, const apk_comm_ops *comm, apk_stream_t stream,
                   apk_sim **out, char *errbuf, size_t errlen) {
  int rc = create_common(deck, overrides, noverrides, rank, nranks, out, errbuf, errlen);
  if (rc != APK_OK) return rc;
  apk_sim *s = *out;
  auto bail = [&](int code) {
    if (errbuf && errlen) std::snprintf(errbuf, errlen, "%s", s->err.c_str());
    apk_sim_destroy(s);
    *out = nullptr;
    return code;
  };
  s->stream = stream;
  if (allocator && allocator->alloc) {
    s->alloc = *allocator;
    s->have_alloc = true;
  }
  if (comm) {
    s->comm = *comm;
    s->have_comm = true;
  }
  // (comm == NULL with nranks > 1: the native RCCL transport is attached by apk_sim_comm_rccl
  // before apk_sim_initialize, which checks)
  if (nranks > 1 && comm && !(comm->exchange && comm->allreduce_min && comm->allreduce_sum)) {
    s->err = "nranks > 1 requires comm ops";
    return bail(APK_ERR_INVALID);
  }
  if (s->mesh.rehearse && comm) {
    s->err = "apk_amd/rehearse_remote_faces brings its own (loopback) transport";
    return bail(APK_ERR_INVALID);
  }
  rc = apk_create(&s->ctx);
  if (rc != APK_OK) {
    s->err = "apk_create failed: no usable gfx950 device (there is no CPU fallback)";
    return bail(rc);
  }
  if (s->pkg.cooling) {
    const CoolingTableHost &ct = s->pkg.cool_table;
    // (the rows as read: the table handle converts and checks them itself)
    std::vector<double> ll(ct.n);
    const double shift = std::log10(s->pkg.cool.lambda_units);
    for (int i = 0; i < ct.n; ++i) ll[i] = ct.log_lambdas[i] + shift;
    rc = apk_cooling_table_create(s->ctx, ct.log_temps.data(), ll.data(), ct.n, &s->pkg.cool, &s->cool_tab);
    if (rc != APK_OK) {
      s->err = apk_last_error(s->ctx);
      return bail(rc);
    }
  }
  if (s->amr) {
    if ((rc = amr_allocate(s, s->mesh.local_gids.size(), s->d_cons2, &s->d_prim2[0], s->d_flux, &s->d_coarse)) != APK_OK) return bail(rc);
    if ((rc = amr_rebuild(s)) != APK_OK) return bail(rc);
    if ((rc = build_copy_plans(s)) != APK_OK) return bail(rc);  // (empty: the uniform-mesh plans are unused)
    return APK_OK;
  }
  const size_t nlb = s->mesh.local_gids.size();
  const size_t bytes = (size_t)s->nper * nlb * sizeof(double);
  if ((rc = dev_alloc(s, "cons", bytes, &s->d_cons2[0])) != APK_OK) return bail(rc);
  if ((rc = dev_alloc(s, "prim", bytes, &s->d_prim2[0])) != APK_OK) return bail(rc);
  if ((rc = dev_alloc(s, "u1", bytes, &s->d_cons2[1])) != APK_OK) return bail(rc);
  if (hipMemset(s->d_cons2[0], 0, bytes) != hipSuccess || hipMemset(s->d_prim2[0], 0, bytes) != hipSuccess ||
      hipMemset(s->d_cons2[1], 0, bytes) != hipSuccess) {
    s->err = "hipMemset failed";
    return bail(APK_ERR_DEVICE);
  }
  for (size_t p = 0; p < s->mesh.peers.size(); ++p) {
    double *sb = nullptr, *rb = nullptr;
    const std::string st = "send:" + std::to_string(s->mesh.peers[p].rank);
    const std::string rt = "recv:" + std::to_string(s->mesh.peers[p].rank);
    if ((rc = dev_alloc(s, st.c_str(), s->mesh.peers[p].send_count * sizeof(double), &sb)) != APK_OK) return bail(rc);
    if ((rc = dev_alloc(s, rt.c_str(), s->mesh.peers[p].recv_count * sizeof(double), &rb)) != APK_OK) return bail(rc);
    s->send_buf.push_back(sb);
    s->recv_buf.push_back(rb);
  }
  if (!stage_can_fuse(s)) {
    if ((rc = ensure_flux_arrays(s)) != APK_OK) return bail(rc);
  } else if ((rc = build_packs(s)) != APK_OK) {
    return bail(rc);
  }
  if ((rc = build_copy_plans(s)) != APK_OK) return bail(rc);
  // (Same-rank ghost copies on a second stream, overlapped with the part of the next stage that needs no ghost zone, were
  // measured in round 2 on 8 x 128^3 PPM+HLLD VL2: 5.73 ms per cycle against 5.24 -- the thin slab launches next to every
  // face and the copy kernel's share of the memory system cost more than the overlap hid; direct neighbour addressing
  // then removed the copies altogether.)
  if (s->mesh.rehearse && (rc = comm_loopback_attach(s)) != APK_OK) return bail(rc);
  if (!s->mesh.peers.empty() && (rc = build_windows(s)) != APK_OK) return bail(rc);
  if ((rc = build_x1_tables(s)) != APK_OK) return bail(rc);
  if (s->mesh.ndim == 3 && (rc = build_face_table(s)) != APK_OK) return bail(rc);
  if (s->fmft && (rc = turbulence_device_setup(s)) != APK_OK) return bail(rc);
  if (s->tracers && (rc = tracers_device_setup(s)) != APK_OK) return bail(rc);
  if (cluster_needs_block_origins(s) && (rc = cluster_device_setup(s)) != APK_OK) return bail(rc);
  return APK_OK;
}

void apk_sim_destroy(apk_sim *s) {
  if (!s) return;
  if (!s->host_only) {
    if (s->exchange_pending && s->comm.exchange_end) (void)s->comm.exchange_end(s->comm.user);  // drain
    (void)hipDeviceSynchronize();
    rccl_transport_destroy(s->rccl);
    s->rccl = nullptr;
    for (auto &pp : s->pplans_of)
      for (auto &pl : pp)
        if (pl) apk_copy_plan_destroy(pl);
    for (auto &pp : s->plans_of)
      for (auto &p : pp) apk_copy_plan_destroy(p);
    for (int p = 0; p < 3; ++p)
      for (int w = 0; w < 2; ++w) {
        apk_pack_destroy(s->mu0_of[p][w]);
        apk_pack_destroy(s->mu1_of[p][w]);
      }
    apk_fmft_destroy(s->fm_dev);
    if (s->side_stream) (void)hipStreamDestroy(reinterpret_cast<hipStream_t>(s->side_stream));
    if (s->ev_fork) (void)hipEventDestroy(reinterpret_cast<hipEvent_t>(s->ev_fork));
    if (s->ev_join) (void)hipEventDestroy(reinterpret_cast<hipEvent_t>(s->ev_join));
    if (s->amr) amr_destroy_device_plans(s);
    for (auto &m : s->amr_halo) amr_free_buffers(s, m);
    amr_free_buffers(s, s->amr_fluxmsg);
    amr_free_buffers(s, s->amr_move);
    dev_free(s, s->d_coarse);
    for (auto &t : s->x1win) dev_free(s, reinterpret_cast<double *>(t.d));
    for (auto &t : s->k3win) dev_free(s, reinterpret_cast<double *>(t.d));
    dev_free(s, reinterpret_cast<double *>(s->d_late_regions));
    dev_free(s, reinterpret_cast<double *>(s->d_face_nbr));
    for (auto &t : s->d_x1_tab) dev_free(s, static_cast<double *>(t));
    sts_free(s);
    tracers_free(s);
    snapshot_free(s);
    dev_free(s, s->d_acc);
    dev_free(s, s->d_phases);
    dev_free(s, s->d_block_xmin);
    dev_free(s, s->d_tower_contribs);
    dev_free(s, reinterpret_cast<double *>(s->d_trig_boxes));
    dev_free(s, s->d_trig_sums);
    dev_free(s, reinterpret_cast<double *>(s->d_split_boxes));
    dev_free(s, s->d_split_sums);
    dev_free(s, s->d_cons2[0]);
    dev_free(s, s->d_prim2[0]);
    dev_free(s, s->d_prim2[1]);
    dev_free(s, s->d_cons2[1]);
    dev_free(s, s->d_cons2[2]);
    for (auto *f : s->d_flux) dev_free(s, f);
    for (auto *b : s->send_buf) dev_free(s, b);
    for (auto *b : s->recv_buf) dev_free(s, b);
    apk_cooling_table_destroy(s->cool_tab);
    apk_destroy(s->ctx);
  }
  delete s;
}

const char *apk_sim_last_error(const apk_sim *s) { return s ? s->err.c_str() : "null sim"; }

int apk_sim_set_fused(apk_sim *s, int fused) {
  if (!s) return APK_ERR_INVALID;
  if (!s->host_only) SIM_TRY(s, sync_ghosts(s));
  s->fused = fused != 0;
  if (!s->host_only && !stage_can_fuse(s)) return ensure_flux_arrays(s);
  return APK_OK;
}

int apk_sim_set_overlap(apk_sim *s, int overlap) {
  if (!s) return APK_ERR_INVALID;
  if (!s->host_only) SIM_TRY(s, sync_ghosts(s));
  s->overlap = overlap != 0;
  return APK_OK;
}

long long apk_sim_overlapped_exchanges(const apk_sim *s) { return s ? s->overlapped : 0; }
long long apk_sim_skipped_local_exchanges(const apk_sim *s) { return s ? s->skipped_local_exchanges : 0; }
long long apk_sim_amr_c2p_passes_skipped(const apk_sim *s) { return s ? s->amr_c2p_passes_skipped : 0; }
int apk_sim_set_direct_neighbors(apk_sim *s, int on) {
  if (!s) return APK_ERR_INVALID;
  if (!s->host_only) SIM_TRY(s, sync_ghosts(s));
  s->direct_on = on != 0;
  return APK_OK;
}
int apk_sim_set_prim_free(apk_sim *s, int on) {
  if (!s) return APK_ERR_INVALID;
  if (!s->host_only) SIM_TRY(s, sync_ghosts(s));
  s->prim_free_on = on != 0;
  return APK_OK;
}
int apk_sim_set_thin_exchange(apk_sim *s, int on) {
  if (!s) return APK_ERR_INVALID;
  s->thin_on = on != 0;
  return APK_OK;
}
long long apk_sim_thin_exchanges(const apk_sim *s) { return s ? s->thin_exchanges : 0; }
int apk_sim_set_x1_direct(apk_sim *s, int on) {
  if (!s) return APK_ERR_INVALID;
  s->x1_on = on != 0;
  return APK_OK;
}
long long apk_sim_x1_direct_exchanges(const apk_sim *s) { return s ? s->x1_direct_exchanges : 0; }
int apk_sim_prim_is_stale(const apk_sim *s) { return (s && s->prim_stale) ? 1 : 0; }
long long apk_sim_turb_dt_kicks(const apk_sim *s) { return s ? s->turb_dt_kicks : 0; }
int apk_sim_set_amr_full_exchange(apk_sim *s, int on) {
  if (!s) return APK_ERR_INVALID;
  if (!s->host_only) SIM_TRY(s, sync_ghosts(s));
  s->amr_full_exchange = on != 0;
  return APK_OK;
}
double apk_sim_loop_seconds(const apk_sim *s) { return s ? s->loop_seconds : 0.0; }
int apk_sim_loop_cycles(const apk_sim *s) { return s ? s->perf_cycles : 0; }
long long apk_sim_loop_zone_cycles(const apk_sim *s) { return s ? s->zone_cycles - s->perf_zone_mark : 0; }

int apk_sim_initialize(apk_sim *s) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  s->err.clear();
  if (s->nranks > 1 && !(s->have_comm && s->comm.exchange && s->comm.allreduce_min && s->comm.allreduce_sum))
    return fail(s, APK_ERR_INVALID, "nranks > 1 requires comm ops (apk_sim_create) or the native transport (apk_sim_comm_rccl)");
  SIM_TRY(s, sync_ghosts(s));
  const int nlb = (int)s->mesh.local_gids.size();
  std::vector<double> host((size_t)s->nper);
  try {
    if (s->problem_id == "turbulence") {
      std::vector<std::vector<double>> blocks;
      SIM_TRY(s, pgen_turbulence(s, blocks));
      for (int lb = 0; lb < nlb; ++lb)
        SIM_HIP(s, hipMemcpy(s->blk(s->d_cons(), lb), blocks[lb].data(), sizeof(double) * s->nblk, hipMemcpyHostToDevice));
    } else {
      for (int lb = 0; lb < nlb; ++lb) {
        pgen_block(s, lb, host);
        SIM_HIP(s, hipMemcpy(s->blk(s->d_cons(), lb), host.data(), sizeof(double) * s->nblk, hipMemcpyHostToDevice));
      }
    }
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  s->time = 0.0;
  s->ncycle = 0;
  s->dt = kHuge;
  s->fofc_total = 0;
  s->fofc_fallback_stages = 0;
  s->zone_cycles = 0;
  s->pkg.mindx = kHuge;
  s->pkg.dt_hyp = kHuge;
  if (s->cluster.enabled) cluster_triggering_reset(s);
  for (double &t : s->split_totals) t = 0.0;
  SIM_TRY(s, exchange_ghosts(s));
  SIM_TRY(s, fill_derived(s));
  // adaptive meshes: tag the initial condition, refine, and evaluate the problem generator again on
  // the new blocks (not a prolongation), level by level
  for (int pass = 0; s->amr && s->amr_adaptive && pass < s->amr->max_level; ++pass) {
    std::vector<int> tags;
    SIM_TRY(s, amr_global_tags(s, tags));
    try {
      if (!amr_update_tree(s, tags, false)) break;
    } catch (const std::exception &e) {
      return fail(s, APK_ERR_INVALID, e.what());
    }
    SIM_TRY(s, amr_reallocate(s));
    try {
      for (int lb = 0; lb < (int)s->mesh.local_gids.size(); ++lb) {
        pgen_block(s, lb, host);
        SIM_HIP(s, hipMemcpy(s->blk(s->d_cons(), lb), host.data(), sizeof(double) * s->nblk, hipMemcpyHostToDevice));
      }
    } catch (const std::exception &e) {
      return fail(s, APK_ERR_INVALID, e.what());
    }
    SIM_TRY(s, exchange_ghosts(s));
    SIM_TRY(s, fill_derived(s));
  }
  double est = kHuge;
  SIM_TRY(s, estimate_timestep(s, &est));
  set_global_dt(s, est);
  SIM_TRY(s, tracers_seed_initial(s));  // SeedInitialTracers (UserWorkBeforeLoopMesh, tracers.cpp:87, 95-186)
  s->initialized = true;
  s->restored = false;
  return APK_OK;
}

int apk_sim_step(apk_sim *s) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  s->err.clear();
  s->initialized = true;
  if (s->time < s->tlim && (s->tlim - s->time) < s->dt) s->dt = s->tlim - s->time;
  SIM_TRY(s, pre_step(s));
  // diffusion/integrator = rkl2: a parabolic half step before and after the hyperbolic stages (hydro_driver.cpp:455-458,
  // 581-583), both sized with the diffusive limit estimated at the end of the previous cycle
  const bool sts = s->pkg.diffusion_sts();
  if (sts) SIM_TRY(s, sts_half_step(s, 0.5 * s->dt));
  // AGN triggering: the accretion rate of the cycle and the removal of the accreted gas, with the cycle's dt, before
  // the tower's contributions (hydro_driver.cpp:360-394)
  if (s->pkg.agn_triggering) SIM_TRY(s, cluster_agn_triggering(s, s->dt));
  // the magnetic tower's power scaling: its two sums once per cycle, before stage 1 (hydro_driver.cpp:409-449)
  if (s->agn_opt.tower_power_scaling) {
    double contribs[2];
    SIM_TRY(s, cluster_tower_contribs(s, s->time, contribs));
    s->tower_linear_contrib = contribs[0], s->tower_quadratic_contrib = contribs[1];
  }
  for (int stage = 1; stage <= s->nstages; ++stage) SIM_TRY(s, do_stage(s, stage));
  if (sts) SIM_TRY(s, sts_half_step(s, 0.5 * s->dt));
  // the tracer step: after the last stage (and the turbulence kick inside it), with the cycle's dt
  // (hydro_driver.cpp:615-660)
  if (s->tracers) SIM_TRY(s, tracers_cycle(s, s->dt));
  s->time += s->dt;
  s->ncycle += 1;
  s->zone_cycles += (long long)s->mesh.mb[0] * s->mesh.mb[1] * s->mesh.mb[2] * (long long)s->mesh.nblocks_total;
  double est = kHuge;
  if (s->amr && s->amr_adaptive && s->amr_check_interval > 0 && s->ncycle % s->amr_check_interval == 0) {
    // Mesh::LoadBalancingAndAdaptiveMeshRefinement, then the new time step (the reference's order).  The tag
    // reduction and the time-step reduction are enqueued back to back and read in ONE host round trip; the
    // estimate is only kept if the mesh stays as it is (every cycle but a few), else it is redone on the new one.
    AmrTagRequest req;
    SIM_TRY(s, amr_tags_begin(s, &req));
    DtEstimate e;
    SIM_TRY(s, estimate_timestep_read(s, &e));
    bool changed = false;
    SIM_TRY(s, amr_regrid(s, &changed, &req));
    if (changed) {  // measure again on the new mesh; flags raised during the cycle stay raised
      e.dt_hyp_local = kHuge;
      SIM_TRY(s, estimate_timestep_read(s, &e));
    }
    SIM_TRY(s, estimate_timestep_commit(s, e, &est));
  } else {
    SIM_TRY(s, estimate_timestep(s, &est));
  }
  set_global_dt(s, est);
  return APK_OK;
}

int apk_sim_run(apk_sim *s, int nlim, int *ncycles) {
  if (!s) return APK_ERR_INVALID;
  int n = 0;
  while (s->time < s->tlim && (nlim < 0 || n < nlim)) {
    int rc = apk_sim_step(s);
    if (rc != APK_OK) return rc;
    ++n;
  }
  if (ncycles) *ncycles = n;
  return APK_OK;
}

double apk_sim_time(const apk_sim *s) { return s->time; }
double apk_sim_dt(const apk_sim *s) { return s->dt; }
double apk_sim_tlim(const apk_sim *s) { return s->tlim; }
double apk_sim_c_h(const apk_sim *s) { return s->pkg.c_h; }
int apk_sim_ncycle(const apk_sim *s) { return s->ncycle; }
long long apk_sim_fofc_count(const apk_sim *s) { return s->fofc_total; }

int apk_sim_diffusion_options(const apk_sim *s, apk_diff_cfg *cfg, int *integrator, double *cfl_diff) {
  if (!s || !cfg || !integrator || !cfl_diff) return APK_ERR_INVALID;
  *cfg = s->pkg.diff;
  *integrator = s->pkg.diffint;
  *cfl_diff = s->pkg.cfl_diff;
  return APK_OK;
}

int apk_sim_spitzer_options(const apk_sim *s, int *enabled, apk_spitzer_cfg *cfg) {
  if (!s || !enabled || !cfg) return APK_ERR_INVALID;
  *enabled = s->pkg.spitzer_cfg() ? 1 : 0;
  *cfg = s->pkg.spitzer;
  return APK_OK;
}

int apk_sim_units(const apk_sim *s, apk_units_info *o) {
  if (!s || !o) return APK_ERR_INVALID;
  std::memset(o, 0, sizeof(*o));
  const UnitsState &u = s->pkg.units;
  o->has_units = u.has_units;
  o->has_composition = u.has_composition;
  o->code_length_cgs = u.code_length_cgs, o->code_mass_cgs = u.code_mass_cgs, o->code_time_cgs = u.code_time_cgs;
  o->mh = u.mh(), o->k_boltzmann = u.k_boltzmann(), o->atomic_mass_unit = u.atomic_mass_unit();
  o->erg = u.erg(), o->cm = u.cm(), o->s = u.s();
  o->He_mass_fraction = u.He_mass_fraction, o->mu = u.mu, o->mu_e = u.mu_e, o->mbar = u.mbar;
  o->mbar_over_kb = u.mbar_over_kb;
  o->efloor = s->pkg.eos.efloor, o->eceil = s->pkg.eos.eceil;
  return APK_OK;
}

int apk_sim_cooling_options(const apk_sim *s, int *enabled, apk_cooling_params *p, int *n_temp) {
  if (!s || !enabled || !p || !n_temp) return APK_ERR_INVALID;
  *enabled = s->pkg.cooling ? 1 : 0;
  *p = s->pkg.cool;
  *n_temp = s->pkg.cool_table.n;
  return APK_OK;
}

int apk_sim_cooling_table(const apk_sim *s, int which, double *out, int n, int *size) {
  if (!s || !size || (n > 0 && !out)) return APK_ERR_INVALID;
  const CoolingTableHost &t = s->pkg.cool_table;
  const std::vector<double> *v = which == 0 ? &t.log_temps : which == 1 ? &t.log_lambdas : which == 2 ? &t.alpha_k
                                 : which == 3 ? &t.Y_k : nullptr;
  if (!v) return APK_ERR_INVALID;
  *size = (int)v->size();
  for (int i = 0; i < n && i < (int)v->size(); ++i) out[i] = (*v)[i];
  return APK_OK;
}

int apk_sim_get_info(const apk_sim *s, apk_sim_info *o) {
  if (!s || !o) return APK_ERR_INVALID;
  std::memset(o, 0, sizeof(*o));
  o->fluid = s->pkg.fluid;
  o->recon = s->pkg.recon;
  o->riemann = s->pkg.riemann;
  o->integrator = s->pkg.integrator;
  for (int d = 0; d < 3; ++d) {
    o->nx[d] = s->mesh.nx[d];
    o->mb[d] = s->mesh.mb[d];
    o->xmin[d] = s->xmin[d];
    o->xmax[d] = s->xmax[d];
    o->dx[d] = s->dx[d];
  }
  o->ng = s->mesh.ng;
  o->nhydro = s->pkg.nhydro;
  o->nscalars = s->pkg.nscalars;
  o->ndim = s->mesh.ndim;
  o->nblocks_total = s->mesh.nblocks_total;
  o->nblocks_local = (int)s->mesh.local_gids.size();
  o->first_gid = s->mesh.local_gids.empty() ? -1 : s->mesh.local_gids[0];
  o->rank = s->rank;
  o->nranks = s->nranks;
  o->npeers = (int)s->mesh.peers.size();
  o->fofc = s->pkg.first_order_flux_correct;
  o->dedner_extended = s->pkg.glmmhd_source_extended;
  o->fused = stage_can_fuse(s);
  o->cfl = s->pkg.cfl;
  o->gamma = s->pkg.eos.gamma;
  o->glmmhd_alpha = s->pkg.glmmhd_alpha;
  o->cells_per_block = s->mesh.sn;
  o->zones_local = (int64_t)s->mesh.mb[0] * s->mesh.mb[1] * s->mesh.mb[2] * (int64_t)s->mesh.local_gids.size();
  o->zones_total = s->amr ? o->zones_local : (int64_t)s->mesh.nx[0] * s->mesh.nx[1] * s->mesh.nx[2];
  return APK_OK;
}

int apk_sim_block_location(const apk_sim *s, int lb, int *gid, int loc[3]) {
  if (!s || lb < 0 || lb >= (int)s->mesh.local_gids.size()) return APK_ERR_INVALID;
  if (gid) *gid = s->mesh.local_gids[lb];
  if (loc && s->amr) {
    for (int d = 0; d < 3; ++d) loc[d] = amr_leaf(s, lb).lx[d];
  } else if (loc) {
    s->mesh.Loc(s->mesh.local_gids[lb], loc);
  }
  return APK_OK;
}

// refinement level of a local block (0 on uniform meshes); with apk_sim_block_location's logical
// location at that level this places the block: x_min = mesh x_min + loc * nx_block * dx / 2^level
int apk_sim_block_level(const apk_sim *s, int lb) {
  if (!s || lb < 0 || lb >= (int)s->mesh.local_gids.size()) return -1;
  return block_level(s, lb);
}

// stages with first_order_flux_correct that had to fall back from the optimistic fused stage to the
// flux-array sequence because a cell failed the admissibility test
long long apk_sim_fofc_fallback_stages(const apk_sim *s) { return s ? s->fofc_fallback_stages : 0; }

int apk_sim_amr_stats(const apk_sim *s, long long *refined, long long *derefined, int *max_level, long long *zone_cycles) {
  if (!s) return APK_ERR_INVALID;
  if (refined) *refined = s->amr_refined;
  if (derefined) *derefined = s->amr_derefined;
  if (max_level) *max_level = s->amr ? s->amr->max_level : 0;
  if (zone_cycles) *zone_cycles = s->zone_cycles;
  return APK_OK;
}

// A regridding pass for GIVEN tags (+1 refine / -1 derefine / 0 per block of the forest, global
// numbering; every rank passes the same array): forest update, new distribution, new plans and --
// on a device sim -- the transfer of the state, ghost exchange and ConsToPrim on the new mesh
int apk_sim_amr_apply_tags(apk_sim *s, const int *tags, int ntags, int *changed) {
  if (!s || !s->amr || !tags || ntags != (int)s->amr->leaves.size()) return APK_ERR_INVALID;
  const std::vector<AmrLeaf> old = s->amr->leaves;
  const AmrPartition old_part = s->amr_part;
  bool ch = false;
  try {
    ch = amr_update_tree(s, std::vector<int>(tags, tags + ntags), true);
    if (s->host_only) {
      amr_sync_mesh(s);
      amr_localize(s);
    }
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  if (!s->host_only && ch) {  // move the state as a regridding pass of the run does
    SIM_TRY(s, amr_transfer(s, old, old_part));
    SIM_TRY(s, exchange_ghosts(s));
    SIM_TRY(s, fill_derived(s));
  }
  if (changed) *changed = ch ? 1 : 0;
  return APK_OK;
}

// one regridding pass on demand (adaptive meshes do this every check_refine_interval cycles)
int apk_sim_regrid(apk_sim *s, int *changed) {
  if (!s || s->host_only || !s->amr) return APK_ERR_INVALID;
  bool ch = false;
  SIM_TRY(s, amr_regrid(s, &ch));
  if (changed) *changed = ch ? 1 : 0;
  return APK_OK;
}

void *apk_sim_block_ptr(const apk_sim *s, int lb, int field) {
  if (!s || s->host_only || lb < 0 || lb >= (int)s->mesh.local_gids.size()) return nullptr;
  double *base = field == 0 ? s->d_cons() : (field == 1 ? s->d_prim() : (field == 2 ? s->d_cons2[s->u1buf] : nullptr));
  return base ? s->blk(base, lb) : nullptr;
}

// The accessors hand blocks over in the natural layout, [nvar][Nk][Nj][Ni], whatever the row pitch on the device
namespace {
void unpad_block(const apk_sim *s, const double *padded, double *natural) {
  const Mesh &m = s->mesh;
  for (int n = 0; n < m.nvar; ++n)
    for (int k = 0; k < m.nk; ++k)
      for (int j = 0; j < m.nj; ++j)
        std::memcpy(natural + (((int64_t)n * m.nk + k) * m.nj + j) * m.ni, padded + n * m.sn + k * m.sk + j * m.sj, sizeof(double) * m.ni);
}
void pad_block(const apk_sim *s, const double *natural, double *padded) {
  const Mesh &m = s->mesh;
  for (int n = 0; n < m.nvar; ++n)
    for (int k = 0; k < m.nk; ++k)
      for (int j = 0; j < m.nj; ++j)
        std::memcpy(padded + n * m.sn + k * m.sk + j * m.sj, natural + (((int64_t)n * m.nk + k) * m.nj + j) * m.ni, sizeof(double) * m.ni);
}
}  // namespace

// a block as it lies on the device (rows at the mesh's pitch; the block's nblk doubles): the host-side readers of this
// file index it through mesh.sj / sk / sn
static int read_block_device_layout(apk_sim *s, int lb, int field, double *host_out) {
  if (s && !s->host_only) SIM_TRY(s, sync_ghosts(s));
  void *p = apk_sim_block_ptr(s, lb, field);
  if (!p || !host_out) return APK_ERR_INVALID;
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  SIM_HIP(s, hipMemcpy(host_out, p, sizeof(double) * s->nblk, hipMemcpyDeviceToHost));
  return APK_OK;
}

int apk_sim_read_block(apk_sim *s, int lb, int field, double *host_out) {
  if (!s || s->host_only || s->mesh.pitch == 0) return read_block_device_layout(s, lb, field, host_out);
  std::vector<double> tmp((size_t)s->nblk);
  SIM_TRY(s, read_block_device_layout(s, lb, field, tmp.data()));
  unpad_block(s, tmp.data(), host_out);
  return APK_OK;
}

int apk_sim_write_block(apk_sim *s, int lb, int field, const double *host_in) {
  if (s && !s->host_only) SIM_TRY(s, sync_ghosts(s));
  void *p = apk_sim_block_ptr(s, lb, field);
  if (!p || !host_in) return APK_ERR_INVALID;
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  if (s->mesh.pitch > 0) {
    std::vector<double> tmp((size_t)s->nblk);
    SIM_HIP(s, hipMemcpy(tmp.data(), p, sizeof(double) * s->nblk, hipMemcpyDeviceToHost));  // (the padding keeps what it held)
    pad_block(s, host_in, tmp.data());
    SIM_HIP(s, hipMemcpy(p, tmp.data(), sizeof(double) * s->nblk, hipMemcpyHostToDevice));
    return APK_OK;
  }
  SIM_HIP(s, hipMemcpy(p, host_in, sizeof(double) * s->nblk, hipMemcpyHostToDevice));
  return APK_OK;
}

int apk_sim_gather(apk_sim *s, int field, double *out) {
  if (!s || s->host_only || !out) return APK_ERR_INVALID;
  if (s->amr) return fail(s, APK_ERR_UNSUPPORTED, "apk_sim_gather needs a uniform mesh: read refined meshes block by block");
  const Mesh &m = s->mesh;
  std::vector<double> host((size_t)s->nper);
  const int64_t NX = m.nx[0], NY = m.nx[1], NZ = m.nx[2];
  for (int lb = 0; lb < (int)m.local_gids.size(); ++lb) {
    int rc = read_block_device_layout(s, lb, field, host.data());
    if (rc != APK_OK) return rc;
    int bc[3];
    m.Loc(m.local_gids[lb], bc);
    for (int n = 0; n < m.nvar; ++n)
      for (int k = m.ks; k <= m.ke; ++k)
        for (int j = m.js; j <= m.je; ++j)
          for (int i = m.is; i <= m.ie; ++i) {
            const int64_t gi = (int64_t)bc[0] * m.mb[0] + (i - m.is), gj = (int64_t)bc[1] * m.mb[1] + (j - m.js),
                          gk = (int64_t)bc[2] * m.mb[2] + (k - m.ks);
            out[((n * NZ + gk) * NY + gj) * NX + gi] = host[n * m.sn + k * m.sk + j * m.sj + i];
          }
  }
  return APK_OK;
}

int apk_sim_history(apk_sim *s, double *out8) {
  if (!s || s->host_only || !out8) return APK_ERR_INVALID;
  // (relDivB differences B across the faces of a block: the ghost zones behind them must be those of the current state,
  // which the stage loop does not keep where it reads neighbours directly -- else the column depends on when they were
  // last filled, and a resumed run, whose ghost zones were filled at the dump, would not repeat it)
  if (s->pkg.fluid == APK_FLUID_GLMMHD) SIM_TRY(s, sync_ghosts(s));
  SIM_TRY(s, apk_history(s->ctx, s->mu0(), s->pkg.fluid, out8, s->stream));
  if (s->have_comm && s->nranks > 1) {
    if (s->comm.allreduce_sum(s->comm.user, out8, 8) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  }
  return APK_OK;
}

// TurbulenceHst<Ms|Ma|pb> (src/pgen/turbulence.cpp:47-101), summed over ranks like Parthenon's
// UserHistoryOperation::sum
int apk_sim_turbulence_history(apk_sim *s, double *out3) {
  if (!s || s->host_only || !out3) return APK_ERR_INVALID;
  if (s->prim_stale) SIM_TRY(s, sync_ghosts(s));  // (the Mach numbers are sums over the PRIMITIVES of the interior)
  SIM_TRY(s, apk_turbulence_history(s->ctx, s->mu0(), s->pkg.fluid, s->pkg.eos.gamma, out3, s->stream));
  if (s->have_comm && s->nranks > 1) {
    if (s->comm.allreduce_sum(s->comm.user, out3, 3) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  }
  return APK_OK;
}

// field_loop::RelDivBHst (src/pgen/field_loop.cpp:60-95), registered as "UserRelDivB" (:97-103)
int apk_sim_user_reldivb(apk_sim *s, double *out) {
  if (!s || s->host_only || !out || s->problem_id != "field_loop") return APK_ERR_INVALID;
  SIM_TRY(s, sync_ghosts(s));  // (div B differences reach into the ghost zones)
  SIM_TRY(s, apk_history_user_reldivb(s->ctx, s->mu0(), s->floop.amp, out, s->stream));
  if (s->have_comm && s->nranks > 1) {
    if (s->comm.allreduce_sum(s->comm.user, out, 1) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  }
  return APK_OK;
}

int apk_sim_fmft_num_modes(const apk_sim *s) { return (s && s->fmft) ? s->fmft->num_modes() : 0; }

int apk_sim_fmft_var_hat(const apk_sim *s, double *out) {
  if (!s || !s->fmft || !out) return APK_ERR_INVALID;
  const auto &vh = s->fmft->var_hat();
  for (size_t q = 0; q < vh.size(); ++q) {
    out[2 * q] = vh[q].real();
    out[2 * q + 1] = vh[q].imag();
  }
  return APK_OK;
}

int apk_sim_fmft_evolve(apk_sim *s, double dt) {
  if (!s || !s->fmft) return APK_ERR_INVALID;
  s->fmft->Evolve(dt);
  return APK_OK;
}

int apk_sim_fmft_phases(const apk_sim *s, int axis, int n, int g0, double *out) {
  if (!s || !s->fmft || !out || axis < 0 || axis > 2 || n <= 0) return APK_ERR_INVALID;
  s->fmft->Phases(axis, n, g0, s->mesh.nx[axis], out);
  return APK_OK;
}

int apk_sim_read_acc(apk_sim *s, int lb, double *host_out) {
  if (!s || s->host_only || !s->d_acc || !host_out || lb < 0 || lb >= (int)s->mesh.local_gids.size()) return APK_ERR_INVALID;
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  SIM_HIP(s, hipMemcpy(host_out, s->d_acc + 3 * (int64_t)s->mesh.sn * lb, sizeof(double) * 3 * s->mesh.sn, hipMemcpyDeviceToHost));
  return APK_OK;
}

// pkg->CheckRefinementBlock as configured by <refinement> (src/hydro/hydro.cpp:788-816), evaluated
// for every local block: tags[lb] = +1 refine / 0 same / -1 derefine.  The mesh itself stays uniform
// here; this is the tagging half of the AMR loop.
int apk_sim_check_refinement(apk_sim *s, int *tags, double *crit) {
  if (!s || s->host_only || !tags) return APK_ERR_INVALID;
  SIM_TRY(s, sync_ghosts(s));
  int criterion;
  double p0, p1;
  SIM_TRY(s, refinement_criterion(s, &criterion, &p0, &p1));
  SIM_TRY(s, apk_tag_blocks(s->ctx, s->mu0(), criterion, p0, p1, tags, crit, s->stream));
  return APK_OK;
}

int apk_sim_history_labels(const apk_sim *s, char *buf, size_t len) {
  if (!s || !buf || !len) return APK_ERR_INVALID;
  std::string l = "mass 1-mom 2-mom 3-mom KE tot-E";
  const bool mhd = s->pkg.fluid == APK_FLUID_GLMMHD;
  if (mhd) l += " ME relDivB";
  if (s->fmft) l += mhd ? " Ms Ma plasma_beta" : " Ms";
  if (s->problem_id == "field_loop") l += " UserRelDivB";
  if (s->problem_id == "linear_wave_mhd" && s->lwm.dump_max_v2) l += " MaxAbsV2";
  // (agn_feedback.cpp:162-177 adds the column whenever feedback is enabled; here only runs with triggering have it, so
  // that the others keep their columns)
  if (s->pkg.agn_triggering) l += " agn_feedback_power";
  // (cluster.cpp:292-313 adds these to every cluster run; here only runs with stellar feedback or clips have them)
  if (s->pkg.cluster_split_srcterm) l += " stellar_mass added_dfloor_mass removed_eceil_energy removed_vceil_energy added_vAceil_mass";
  std::snprintf(buf, len, "%s", l.c_str());
  return APK_OK;
}

// HstMaxV2 (src/pgen/linear_wave_mhd.cpp:713-737): max |v2| over the interior cells of every block, max over ranks.  For
// history outputs only: each block's v2 comes to the host (one plane of the primitives per block).
static int max_abs_v2(apk_sim *s, double *out) {
  if (s->prim_stale) SIM_TRY(s, sync_ghosts(s));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  const Mesh &m = s->mesh;
  std::vector<double> v((size_t)m.sn);
  double mx = 0.0;
  for (int lb = 0; lb < (int)m.local_gids.size(); ++lb) {
    SIM_HIP(s, hipMemcpy(v.data(), s->blk(s->d_prim(), lb) + 2 * m.sn /* IV2 */, sizeof(double) * m.sn, hipMemcpyDeviceToHost));
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) mx = std::fmax(mx, std::fabs(v[k * m.sk + j * m.sj + i]));
  }
  double neg = -mx;  // (max over ranks as the min of the negatives)
  if (s->have_comm && s->nranks > 1 && s->comm.allreduce_min(s->comm.user, &neg, 1) != 0)
    return fail(s, APK_ERR_DEVICE, "allreduce_min failed");
  *out = -neg;
  return APK_OK;
}

int apk_sim_write_history(apk_sim *s, const char *path) {
  if (!s || s->host_only || !path) return APK_ERR_INVALID;
  const bool mhd = s->pkg.fluid == APK_FLUID_GLMMHD;
  double h[8], t3[3] = {0, 0, 0};
  int rc = apk_sim_history(s, h);
  if (rc != APK_OK) return rc;
  if (s->fmft && (rc = apk_sim_turbulence_history(s, t3)) != APK_OK) return rc;
  const bool floop = s->problem_id == "field_loop";
  double urdb = 0.0;
  if (floop && (rc = apk_sim_user_reldivb(s, &urdb)) != APK_OK) return rc;
  const bool maxv2 = s->problem_id == "linear_wave_mhd" && s->lwm.dump_max_v2;
  double mv2 = 0.0;
  if (maxv2 && (rc = max_abs_v2(s, &mv2)) != APK_OK) return rc;
  // the running totals of the split cluster sources: reported, then reset on every rank (cluster.cpp:300-313)
  double totals[5];
  for (int q = 0; q < 5; ++q) totals[q] = s->split_totals[q], s->split_totals[q] = 0.0;
  if (s->rank != 0) return APK_OK;
  std::vector<double> row(h, h + (mhd ? 8 : 6));
  if (s->fmft) row.insert(row.end(), t3, t3 + (mhd ? 3 : 1));
  if (floop) row.push_back(urdb);
  if (maxv2) row.push_back(mv2);
  if (s->pkg.agn_triggering) row.push_back(s->agn_opt.configured ? s->agn.power() : 0.0);
  if (s->pkg.cluster_split_srcterm) row.insert(row.end(), totals, totals + 5);
  FILE *f = std::fopen(path, "r");
  const bool fresh = (f == nullptr);
  if (f) std::fclose(f);
  f = std::fopen(path, "a");
  if (!f) return fail(s, APK_ERR_INVALID, std::string("history file could not be opened: ") + path);
  if (fresh) {
    char labels[512];
    apk_sim_history_labels(s, labels, sizeof(labels));
    int col = 1;
    std::fprintf(f, "#  History data\n");
    std::fprintf(f, "# [%d]=time     ", col++);
    std::fprintf(f, "[%d]=dt       ", col++);
    std::fprintf(f, "[%d]=cycle    ", col++);
    std::fprintf(f, "[%d]=nbtotal  ", col++);
    std::istringstream iss(labels);
    std::string lab;
    while (iss >> lab) std::fprintf(f, "[%d]=%-8s", col++, lab.c_str());
    std::fprintf(f, "\n");
  }
  const std::string fmt = " " + s->pin.GetOrAddString("parthenon/output_defaults", "data_format", "%12.5e");
  std::fprintf(f, fmt.c_str(), s->time);
  std::fprintf(f, fmt.c_str(), s->dt);
  std::fprintf(f, " %d %d", s->ncycle, s->mesh.nblocks_total);
  for (double v : row) std::fprintf(f, fmt.c_str(), v);
  std::fprintf(f, "\n");
  std::fclose(f);
  return APK_OK;
}

int apk_sim_write_linear_wave_errors(apk_sim *s, const char *path) {
  if (!s || !path) return APK_ERR_INVALID;
  const bool mhd_wave = s->problem_id == "linear_wave_mhd";
  const int ncol = mhd_wave ? 8 : 5;
  double rms = 0.0, l1[8], mx[8];
  int rc = mhd_wave ? apk_sim_linear_wave_mhd_errors(s, &rms, l1, mx) : apk_sim_linear_wave_errors(s, &rms, l1, mx);
  if (rc != APK_OK) return rc;
  if (s->rank != 0) return APK_OK;
  double max_max_over_l1 = 0.0;
  for (int n = 0; n < ncol; ++n) max_max_over_l1 = std::fmax(max_max_over_l1, mx[n] / l1[n]);
  FILE *f = std::fopen(path, "r");
  const bool fresh = (f == nullptr);
  if (f) std::fclose(f);
  f = std::fopen(path, "a");
  if (!f) return fail(s, APK_ERR_INVALID, "Error output file could not be opened");
  if (fresh) {  // linear_wave.cpp:315-320 / linear_wave_mhd.cpp:318-326
    std::fprintf(f, "# Nx1  Nx2  Nx3  Ncycle  ");
    std::fprintf(f, "RMS-L1-Error  d_L1  M1_L1  M2_L1  M3_L1  E_L1 ");
    if (mhd_wave) std::fprintf(f, "  B1c_L1  B2c_L1  B3c_L1");
    std::fprintf(f, "  Largest-Max/L1  d_max  M1_max  M2_max  M3_max  E_max ");
    if (mhd_wave) std::fprintf(f, "  B1c_max  B2c_max  B3c_max");
    std::fprintf(f, "\n");
  }
  // the hydro file's column 3 repeats Nx2 (that is what linear_wave.cpp:323-324 prints); the MHD file's holds Nx3
  std::fprintf(f, "%d  %d", s->mesh.nx[0], s->mesh.nx[1]);
  std::fprintf(f, "  %d  %d", mhd_wave ? s->mesh.nx[2] : s->mesh.nx[1], s->ncycle);
  std::fprintf(f, "  %e  %e", rms, l1[0]);
  std::fprintf(f, "  %e  %e  %e", l1[1], l1[2], l1[3]);
  std::fprintf(f, "  %e", l1[4]);
  for (int n = 5; n < ncol; ++n) std::fprintf(f, "  %e", l1[n]);
  std::fprintf(f, "  %e  %e  ", max_max_over_l1, mx[0]);
  std::fprintf(f, "%e  %e  %e", mx[1], mx[2], mx[3]);
  std::fprintf(f, "  %e", mx[4]);
  for (int n = 5; n < ncol; ++n) std::fprintf(f, "  %e", mx[n]);
  std::fprintf(f, "\n");
  std::fclose(f);
  return APK_OK;
}

int apk_sim_execute(apk_sim *s, const char *outdir, int *ncycles) {
  if (!s || s->host_only || !outdir) return APK_ERR_INVALID;
  struct HstOut {
    std::string path;
    double dt, next;
    int rows = 0;  // history rows written so far
    std::string number;  // N of <parthenon/outputN>
  };
  // a restored sim (apk_sim_restore) goes on where the dump was written: no initialisation, no row or dump for the restored
  // time, files appended to, every output's next time and counter as the state file has them
  const bool resumed = s->restored;
  auto stored = [&](const std::string &number) -> const apk::OutputSchedule * {
    for (const auto &o : s->restored_sched)
      if (o.number == number) return &o;
    return nullptr;
  };
  // (an output block the state file does not know, e.g. one an override added: from the next multiple of its dt on)
  auto next_after = [&](double dt) { return dt * (std::floor(s->time / dt) + 1.0); };
  std::vector<HstOut> outs;
  try {
    const std::string base = s->pin.GetOrAddString("parthenon/job", "problem_id", "parthenon");
    for (const std::string &blk : s->pin.BlocksWithPrefix("parthenon/output")) {
      if (blk == "parthenon/output_defaults" || !s->pin.DoesParameterExist(blk, "file_type")) continue;
      // npy: field snapshots, rst: restart dumps, both parsed at creation (host/snapshot.cpp: s->snap_outs, host/restart.cpp:
      // s->rst_outs); hdf5 outputs are out of scope
      if (s->pin.GetString(blk, "file_type") != "hst") continue;
      const std::string num = blk.substr(std::string("parthenon/output").size());
      const double out_dt = s->pin.GetReal(blk, "dt");
      if (!(out_dt > 0.0)) throw std::runtime_error("<" + blk + ">: dt must be positive for hst outputs");
      outs.push_back({std::string(outdir) + "/" + base + ".out" + num + ".hst", out_dt, 0.0, 0, num});
      if (s->pin.DoesParameterExist(blk, "data_format"))
        s->pin.ApplyOverride("parthenon/output_defaults/data_format=" + s->pin.GetString(blk, "data_format"));
    }
  } catch (const std::exception &e) {
    return fail(s, APK_ERR_INVALID, e.what());
  }
  // the lookback correlations (turbulence.cpp:610-643): truncated by the initialisation, a row per cycle while this
  // call runs
  struct CsvScope {
    apk_sim *s;
    ~CsvScope() {
      if (s->tracers) s->tracers->csv_path.clear();
    }
  } csv_scope{s};
  if (s->tracers && s->tracers->lookback) s->tracers->csv_path = std::string(outdir) + "/correlations.csv";
  // problem/cluster/agn_triggering/write_to_file: truncated here, a row per cycle while this call runs
  struct TrigScope {
    apk_sim *s;
    ~TrigScope() { s->trig_path.clear(); }
  } trig_scope{s};
  if (s->pkg.agn_triggering && s->trig_write_to_file) {
    s->trig_path = std::string(outdir) + "/" + s->trig_filename;
    if (s->rank == 0) {
      FILE *f = std::fopen(s->trig_path.c_str(), resumed ? "a" : "w");
      if (!f) return fail(s, APK_ERR_INVALID, "cannot open " + s->trig_path);
      std::fclose(f);
    }
  }
  if (!resumed) SIM_TRY(s, apk_sim_initialize(s));
  // problem/cluster/hydrostatic_equilibrium/test_he_sphere: the reference writes the file when it builds the package
  if (!resumed) SIM_TRY(s, cluster_write_test_profile(s, std::string(outdir) + "/test_he_sphere.dat"));
  // the tracers next to every history row: <history file without .hst>.<row, 5 digits>.tracers.<field>.npy
  auto write_tracers = [&](HstOut &o) -> int {
    if (!s->tracers) return APK_OK;
    char num[16];
    std::snprintf(num, sizeof num, "%05d", o.rows++);
    return tracers_write_outputs(s, o.path.substr(0, o.path.size() - 4) + "." + num + ".tracers");
  };
  for (auto &o : outs) {
    if (resumed) {
      const apk::OutputSchedule *st = stored(o.number);
      o.next = st ? st->next : next_after(o.dt);
      o.rows = st ? (int)st->counter : 0;
      continue;
    }
    if (s->rank == 0) std::remove(o.path.c_str());
    SIM_TRY(s, apk_sim_write_history(s, o.path.c_str()));
    SIM_TRY(s, write_tracers(o));
    if (!s->tracers) o.rows += 1;  // (write_tracers counts them otherwise)
    o.next = o.dt;
  }
  // the field snapshots: <outdir>/<problem_id>.<id>.<NNNNN>, the cadence rule of the history outputs
  struct SnapOut {
    const apk::SnapshotOutput *o;
    double next;
    int dumps;
  };
  std::vector<SnapOut> snaps;
  for (const auto &o : s->snap_outs) {
    const apk::OutputSchedule *st = resumed ? stored(o.block.substr(std::string("parthenon/output").size())) : nullptr;
    snaps.push_back({&o, st ? st->next : (resumed ? next_after(o.dt) : o.dt), st ? (int)st->counter : 0});
  }
  auto write_snapshot = [&](SnapOut &so) -> int {
    char num[16];
    std::snprintf(num, sizeof num, "%05d", so.dumps++);
    const std::string base = s->pin.GetOrAddString("parthenon/job", "problem_id", "parthenon");
    return snapshot_write(s, std::string(outdir) + "/" + base + "." + so.o->id + "." + num, so.o->codes, so.o->names, so.o->single);
  };
  if (!resumed)
    for (auto &so : snaps) SIM_TRY(s, write_snapshot(so));
  // the restart dumps: <outdir>/<problem_id>.<id>.<NNNNN>.{rank<r>.npy, json, rst}, the same cadence rule; none at t = 0
  struct RstOut {
    const apk::RestartOutputBlock *o;
    double next;
    int dumps;
  };
  std::vector<RstOut> rsts;
  for (const auto &o : s->rst_outs) {
    const apk::OutputSchedule *st = resumed ? stored(o.number) : nullptr;
    rsts.push_back({&o, st ? st->next : (resumed ? next_after(o.dt) : o.dt), st ? (int)st->counter : 0});
  }
  // what a dump stores of the outputs: where each of them stands once the cycle's outputs are written
  struct SchedScope {
    apk_sim *s;
    ~SchedScope() { s->out_sched.clear(); }
  } sched_scope{s};
  auto publish_schedules = [&]() {
    s->out_sched.clear();
    for (const auto &o : outs) s->out_sched.push_back({o.number, o.next, (long long)o.rows});
    for (const auto &so : snaps) s->out_sched.push_back({so.o->block.substr(std::string("parthenon/output").size()), so.next, (long long)so.dumps});
    for (const auto &ro : rsts) s->out_sched.push_back({ro.o->number, ro.next, (long long)ro.dumps});
  };
  int n = 0;
  // parthenon/time/perf_cycle_offset: cycles left out of the performance figure (first-touch
  // allocations, e.g. the flux-difference workspace and the spare prim buffer, happen there)
  const int perf_offset = s->pin.GetOrAddInteger("parthenon/time", "perf_cycle_offset", 0);
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  auto t0 = std::chrono::steady_clock::now();
  s->perf_cycles = 0;
  s->perf_zone_mark = s->zone_cycles;
  const int done_before = resumed ? s->ncycle : 0;  // (nlim bounds the run's cycle number, as Parthenon's does)
  while (s->time < s->tlim && (s->nlim < 0 || done_before + n < s->nlim)) {
    if (n == perf_offset && n > 0) {
      SIM_HIP(s, hipStreamSynchronize(hs(s)));
      t0 = std::chrono::steady_clock::now();
      s->perf_zone_mark = s->zone_cycles;
    }
    SIM_TRY(s, apk_sim_step(s));
    ++n;
    if (n > perf_offset) s->perf_cycles += 1;
    const bool last = !(s->time < s->tlim && (s->nlim < 0 || done_before + n < s->nlim));
    for (auto &o : outs)
      if (s->time >= o.next || last) {
        SIM_TRY(s, apk_sim_write_history(s, o.path.c_str()));
        SIM_TRY(s, write_tracers(o));
        if (!s->tracers) o.rows += 1;
        while (o.next <= s->time) o.next += o.dt;
      }
    for (auto &so : snaps)
      if (s->time >= so.next || last) {
        SIM_TRY(s, write_snapshot(so));
        while (so.next <= s->time) so.next += so.o->dt;
      }
    // every rst output that fires this cycle is counted and advanced before any of them is written: each dump then says
    // where ALL outputs stand after this cycle, and a run resumed from either numbers the next dumps as this one does
    std::vector<std::pair<const RstOut *, int>> firing;
    for (auto &ro : rsts)
      if (s->time >= ro.next || last) {
        firing.emplace_back(&ro, ro.dumps++);
        while (ro.next <= s->time) ro.next += ro.o->dt;
      }
    if (!firing.empty()) publish_schedules();
    for (const auto &fr : firing) {
      char num[16];
      std::snprintf(num, sizeof num, "%05d", fr.second);
      const std::string base = s->pin.GetOrAddString("parthenon/job", "problem_id", "parthenon");
      SIM_TRY(s, restart_write(s, std::string(outdir) + "/" + base + "." + fr.first->o->id + "." + num));
    }
  }
  SIM_TRY(s, sync_ghosts(s));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  s->loop_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if ((s->problem_id == "linear_wave" || s->problem_id == "linear_wave_mhd") && s->lw.compute_error)
    SIM_TRY(s, apk_sim_write_linear_wave_errors(s, (std::string(outdir) + "/linearwave-errors.dat").c_str()));
  if (s->problem_id == "cpaw" && s->cpaw.compute_error)
    SIM_TRY(s, apk_sim_write_cpaw_errors(s, (std::string(outdir) + "/cpaw-errors.dat").c_str()));
  if (ncycles) *ncycles = n;
  return APK_OK;
}

// src/pgen/linear_wave.cpp:183-335 (5 columns: d, M1, M2, M3, E) and src/pgen/linear_wave_mhd.cpp:177-276 (8 columns:
// + B1, B2, B3 against the ANALYTIC field; psi is not part of the norm): volume-weighted L1 and max errors of the
// interior cells against the wave at the initial phase, L1 normalised by the domain volume, RMS over the columns
static int linear_wave_errors_n(apk_sim *s, int ncol, double *rms, double *l1, double *mx) {
  const Mesh &m = s->mesh;
  const bool mhd_wave = ncol == 8;
  std::vector<double> host((size_t)s->nper);
  double acc[16] = {0};
  for (int lb = 0; lb < (int)m.local_gids.size(); ++lb) {
    int rc = read_block_device_layout(s, lb, 0, host.data());
    if (rc != APK_OK) return rc;
    LevelDxScope level_dx_scope(s, lb);
    const double cellvol = s->dx[0] * s->dx[1] * s->dx[2];
    double x0[3];
    block_origin(s, lb, x0);
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) {
          double u[8];
          if (mhd_wave) lwm_state(s, xc(s, x0, 0, i), xc(s, x0, 1, j), xc(s, x0, 2, k), u);
          else lw_state(s->lw, xc(s, x0, 0, i), xc(s, x0, 1, j), xc(s, x0, 2, k), u);
          for (int n = 0; n < ncol; ++n) {
            const double e = std::abs(u[n] - host[n * m.sn + k * m.sk + j * m.sj + i]);
            acc[n] += e * cellvol;
            if (e > acc[8 + n]) acc[8 + n] = e;
          }
        }
  }
  if (s->have_comm && s->nranks > 1) {
    if (s->comm.allreduce_sum(s->comm.user, acc, ncol) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
    // MAX of non-negative values through the MIN callback
    double neg[8];
    for (int n = 0; n < ncol; ++n) neg[n] = -acc[8 + n];
    if (s->comm.allreduce_min(s->comm.user, neg, ncol) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_min failed");
    for (int n = 0; n < ncol; ++n) acc[8 + n] = -neg[n];
  }
  const double vol = (s->xmax[0] - s->xmin[0]) * (s->xmax[1] - s->xmin[1]) * (s->xmax[2] - s->xmin[2]);
  double r = 0.0;
  for (int n = 0; n < ncol; ++n) {
    l1[n] = acc[n] / vol;
    mx[n] = acc[8 + n];
    r += l1[n] * l1[n];
  }
  *rms = std::sqrt(r);
  return APK_OK;
}

int apk_sim_linear_wave_errors(apk_sim *s, double *rms, double *l1, double *mx) {
  if (!s || s->host_only || s->problem_id != "linear_wave" || !rms || !l1 || !mx) return APK_ERR_INVALID;
  return linear_wave_errors_n(s, 5, rms, l1, mx);
}

int apk_sim_linear_wave_mhd_errors(apk_sim *s, double *rms, double *l1, double *mx) {
  if (!s || s->host_only || s->problem_id != "linear_wave_mhd" || !rms || !l1 || !mx) return APK_ERR_INVALID;
  return linear_wave_errors_n(s, 8, rms, l1, mx);
}

// cpaw::UserWorkAfterLoop (src/pgen/cpaw.cpp:127-221): L1 errors against the initial state, err8 in
// the order d, M1, M2, M3, E, B1, B2, B3
int apk_sim_cpaw_errors(apk_sim *s, double *rms, double *err8) {
  if (!s || s->host_only || s->problem_id != "cpaw" || !rms || !err8) return APK_ERR_INVALID;
  const Mesh &m = s->mesh;
  const CpawState &c = s->cpaw;
  std::vector<double> host((size_t)s->nper);
  double err[8] = {0};
  for (int lb = 0; lb < (int)m.local_gids.size(); ++lb) {
    int rc = read_block_device_layout(s, lb, 0, host.data());
    if (rc != APK_OK) return rc;
    double x0[3];
    block_origin(s, lb, x0);
    auto at = [&](int n, int k, int j, int i) { return host[n * m.sn + k * m.sk + j * m.sj + i]; };
    for (int k = m.ks; k <= m.ke; ++k)
      for (int j = m.js; j <= m.je; ++j)
        for (int i = m.is; i <= m.ie; ++i) {
          double mom[3], b[3];
          cpaw_state(c, xc(s, x0, 0, i), xc(s, x0, 1, j), xc(s, x0, 2, k), mom, b);
          err[0] += std::abs(c.den - at(0, k, j, i));
          for (int d = 0; d < 3; ++d) err[1 + d] += std::abs(mom[d] - at(1 + d, k, j, i));
          for (int d = 0; d < 3; ++d) err[5 + d] += std::abs(b[d] - at(5 + d, k, j, i));
          const double e0 = c.pres / c.gm1 + 0.5 * (mom[0] * mom[0] + mom[1] * mom[1] + mom[2] * mom[2]) / c.den +
                            0.5 * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
          err[4] += std::abs(e0 - at(4, k, j, i));
        }
  }
  if (s->have_comm && s->nranks > 1) {
    if (s->comm.allreduce_sum(s->comm.user, err, 8) != 0) return fail(s, APK_ERR_DEVICE, "allreduce_sum failed");
  }
  const double ncells = (double)m.nx[0] * m.nx[1] * m.nx[2];
  double r = 0.0;
  for (int n = 0; n < 8; ++n) {
    err8[n] = err[n] / ncells;
    r += err8[n] * err8[n];
  }
  *rms = std::sqrt(r);
  return APK_OK;
}

// "cpaw-errors.dat" (cpaw.cpp:188-220): header when the file is new, otherwise append
int apk_sim_write_cpaw_errors(apk_sim *s, const char *path) {
  if (!s || !path) return APK_ERR_INVALID;
  double rms = 0.0, err[8];
  int rc = apk_sim_cpaw_errors(s, &rms, err);
  if (rc != APK_OK) return rc;
  if (s->rank != 0) return APK_OK;
  FILE *f = std::fopen(path, "r");
  const bool fresh = (f == nullptr);
  if (f) std::fclose(f);
  f = std::fopen(path, "a");
  if (!f) return fail(s, APK_ERR_INVALID, "Error output file could not be opened");
  if (fresh) {
    std::fprintf(f, "# Nx1  Nx2  Nx3  Ncycle  RMS-Error  d  M1  M2  M3");
    std::fprintf(f, "  E");
    std::fprintf(f, "  B1c  B2c  B3c");
    std::fprintf(f, "\n");
  }
  std::fprintf(f, "%d  %d", s->mesh.nx[0], s->mesh.nx[1]);
  std::fprintf(f, "  %d  %d  %e", s->mesh.nx[2], s->ncycle, rms);
  std::fprintf(f, "  %e  %e  %e  %e", err[0], err[1], err[2], err[3]);
  std::fprintf(f, "  %e", err[4]);
  std::fprintf(f, "  %e  %e  %e", err[5], err[6], err[7]);
  std::fprintf(f, "\n");
  std::fclose(f);
  return APK_OK;
}

int apk_sim_exchange_ghosts(apk_sim *s) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  SIM_TRY(s, sync_ghosts(s));
  return exchange_ghosts(s);
}
int apk_sim_fill_derived(apk_sim *s) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  SIM_TRY(s, sync_ghosts(s));
  return fill_derived(s);
}
int apk_sim_estimate_timestep(apk_sim *s, double *dt) {
  if (!s || s->host_only || !dt) return APK_ERR_INVALID;
  return estimate_timestep(s, dt);
}

// after the caller replaced the state (apk_sim_write_block + apk_sim_exchange_ghosts + apk_sim_fill_derived): the time
// step as apk_sim_initialize derives it from a problem generator's state -- no growth limit from an earlier step
int apk_sim_reset_time_step(apk_sim *s) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  s->err.clear();
  SIM_TRY(s, sync_ghosts(s));
  s->dt = kHuge;
  s->pkg.mindx = kHuge;
  s->pkg.dt_hyp = kHuge;
  s->dt_hyp_is_global = false;
  s->stage_dt_pending = false;
  double est = kHuge;
  SIM_TRY(s, estimate_timestep(s, &est));
  set_global_dt(s, est);
  return APK_OK;
}

int apk_sim_kernel_timing_enable(apk_sim *s, int on) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  return apk_kernel_timing_enable(s->ctx, on);
}
int apk_sim_kernel_timing_read(apk_sim *s, int slot, double *total_ms, long long *launches) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  return apk_kernel_timing_read(s->ctx, slot, total_ms, launches);
}

// the message set the next comm.exchange moves: the uniform mesh's halo buffers, or -- on refined
// meshes -- whichever of halo / flux-correction / regridding messages the driver has made current
int apk_sim_num_peers(const apk_sim *s) {
  if (!s) return APK_ERR_INVALID;
  return s->active_msgs ? (int)s->active_msgs->plan.peers.size() : (int)s->mesh.peers.size();
}
long long apk_sim_message_generation(const apk_sim *s) { return s ? s->msg_generation : 0; }
// plan introspection: make the halo (1) or flux-correction (2) message set of a refined mesh the one
// apk_sim_peer reports (0: back to the uniform mesh's)
int apk_sim_select_messages(apk_sim *s, int which) {
  if (!s || which < 0 || which > 5 || (which > 0 && which < 5 && !s->amr) || (which == 5 && s->amr)) return APK_ERR_INVALID;
  const apk_sim::MsgSet *sets[6] = {nullptr, &s->amr_halo[AMR_FAMILY_FULL], &s->amr_fluxmsg, &s->amr_halo[AMR_FAMILY_FACES],
                                    &s->amr_halo[AMR_FAMILY_SHELL], nullptr};
  s->active_msgs = sets[which];
  s->thin_msgs = which == 5;  // (the one-layer set of a uniform mesh; every exchange selects the set it moves anyway)
  s->msg_generation += 1;
  return APK_OK;
}

int apk_sim_peer(const apk_sim *s, int p, apk_peer_info *o) {
  if (!s || !o || p < 0 || p >= apk_sim_num_peers(s)) return APK_ERR_INVALID;
  if (s->active_msgs) {
    const apk_sim::MsgSet &m = *s->active_msgs;
    o->rank = m.plan.peers[p].rank;
    o->send_count = m.plan.peers[p].send_count;
    o->recv_count = m.plan.peers[p].recv_count;
    o->send_buf = (p < (int)m.send.size()) ? m.send[p] : nullptr;
    o->recv_buf = (p < (int)m.recv.size()) ? m.recv[p] : nullptr;
    return APK_OK;
  }
  o->rank = s->mesh.peers[p].rank;
  o->send_count = s->thin_msgs ? s->mesh.peers[p].send_count_thin : s->mesh.peers[p].send_count;
  o->recv_count = s->thin_msgs ? s->mesh.peers[p].recv_count_thin : s->mesh.peers[p].recv_count;
  o->send_buf = (p < (int)s->send_buf.size()) ? s->send_buf[p] : nullptr;
  o->recv_buf = (p < (int)s->recv_buf.size()) ? s->recv_buf[p] : nullptr;
  return APK_OK;
}

// phases 0..5: the uniform-mesh plan; 10: multilevel fill copies, 11..13: coarse-buffer boundaries
// x1..x3, 14..16: block boundaries x1..x3, 17..19: flux-correction copies x1..x3
const std::vector<BoxRegion> *plan_of_phase(const apk_sim *s, int phase) {
  // (0..7: the uniform mesh's plans PH_LOCAL .. PH_UNPACK_THIN; 60..63: the same pack / unpack plans without the x1 faces,
  // PH_PACK_NOX1 .. PH_UNPACK_THIN_NOX1 -- the numbers 10..50 below belong to refined meshes)
  if (phase >= 0 && phase < PH_PACK_NOX1) return &s->mesh.plan[phase];
  if (phase >= 60 && phase < 60 + (PH_COUNT - PH_PACK_NOX1)) return &s->mesh.plan[PH_PACK_NOX1 + (phase - 60)];
  if (!s->amr) return nullptr;
  // this rank's share (local block numbers; kinds 1 / 2 = message buffers of the halo set for 20..24,
  // of the flux-correction set for 25..33)
  const auto &l = s->amr_local;
  if (phase >= 25 && phase <= 27) return &l.flux_copy[phase - 25];
  if (phase >= 28 && phase <= 30) return &l.flux_pack[phase - 28];
  if (phase >= 31 && phase <= 33) return &l.flux_unpack[phase - 31];
  if (phase >= 34 && phase <= 36) return &l.coarse_bc[phase - 34];
  // the ghost exchange in its forms (amr_forms.hpp): a family's whole fill copies, packs and unpacks at 20..22 (full),
  // 40..42 (faces: the stage loop's) and 44..46 (shell); the full and the shell family's block boundaries at 37..39 and
  // 47..49; the fill copies of 40 and 44 without the same-level same-rank ones (direct neighbour addressing) at 43 and 50
  const int first[AMR_FAMILIES] = {20, 40, 44}, bc[AMR_FAMILIES] = {37, -1, 47};
  for (int fam = 0; fam < AMR_FAMILIES; ++fam) {
    if (phase == first[fam]) return &l.fill[AMR_FAMILY[fam].whole];
    if (phase == first[fam] + 1) return &l.family[fam].pack;
    if (phase == first[fam] + 2) return &l.family[fam].unpack;
    if (bc[fam] >= 0 && phase >= bc[fam] && phase < bc[fam] + 3) return &l.family[fam].fine_bc[phase - bc[fam]];
  }
  if (phase == 43) return &l.fill[AMR_XCHG_DIRECT];
  if (phase == 50) return &l.fill[AMR_XCHG_SHELL_DIRECT];
  if (phase == 10) return &s->amr_plans.fill;
  if (phase >= 11 && phase <= 13) return &s->amr_plans.coarse_bc[phase - 11];
  if (phase >= 14 && phase <= 16) return &s->amr_plans.fine_bc[phase - 14];
  if (phase >= 17 && phase <= 19) return &s->amr_plans.flux_copy[phase - 17];
  return nullptr;
}

int apk_sim_plan_size(const apk_sim *s, int phase) {
  const std::vector<BoxRegion> *p = s ? plan_of_phase(s, phase) : nullptr;
  return p ? (int)p->size() : APK_ERR_INVALID;
}

int apk_sim_plan_region(const apk_sim *s, int phase, int r, apk_region_info *o) {
  const std::vector<BoxRegion> *p = (s && o) ? plan_of_phase(s, phase) : nullptr;
  if (!p || r < 0 || r >= (int)p->size()) return APK_ERR_INVALID;
  const BoxRegion &b = (*p)[r];
  o->src_kind = b.src_kind;
  o->src_block = b.src_block;
  o->dst_kind = b.dst_kind;
  o->dst_block = b.dst_block;
  o->src_off = b.src_off;
  o->dst_off = b.dst_off;
  o->nvar = b.nvar;
  o->flip_var = b.flip_var;
  for (int q = 0; q < 3; ++q) o->ext[q] = b.ext[q];
  for (int q = 0; q < 4; ++q) {
    o->src_stride[q] = b.src_stride[q];
    o->dst_stride[q] = b.dst_stride[q];
  }
  return APK_OK;
}

// operator lists of the multilevel plans: 0 restrict-own, 1 prolongate, 2..4 flux restriction x1..x3
const std::vector<AmrRefOp> *ops_of(const apk_sim *s, int which) {
  if (!s->amr) return nullptr;
  // 10..14: this rank's share of 0..4 (local block numbers)
  if (which == 10) return &s->amr_local.restrict_own;
  if (which == 11) return &s->amr_local.family[AMR_FAMILY_FULL].prolongate;
  if (which >= 12 && which <= 14) return &s->amr_local.flux_restrict[which - 12];
  if (which == 15 || which == 16) return &s->amr_local.family[AMR_FAMILY_FACES + (which - 15)].prolongate;  // (faces, shell)
  if (which == 0) return &s->amr_plans.restrict_own;
  if (which == 1) return &s->amr_plans.prolongate;
  if (which >= 2 && which <= 4) return &s->amr_plans.flux_restrict[which - 2];
  return nullptr;
}

int apk_sim_amr_ops_size(const apk_sim *s, int which) {
  const std::vector<AmrRefOp> *p = s ? ops_of(s, which) : nullptr;
  return p ? (int)p->size() : APK_ERR_INVALID;
}

int apk_sim_amr_op(const apk_sim *s, int which, int n, apk_amr_op_info *o) {
  const std::vector<AmrRefOp> *p = (s && o) ? ops_of(s, which) : nullptr;
  if (!p || n < 0 || n >= (int)p->size()) return APK_ERR_INVALID;
  const AmrRefOp &a = (*p)[n];
  o->kind = a.kind;
  o->level = a.level;
  o->src_kind = a.src_kind;
  o->src_block = a.src_block;
  o->dst_kind = a.dst_kind;
  o->dst_block = a.dst_block;
  for (int q = 0; q < 3; ++q) {
    o->lo[q] = a.lo[q];
    o->hi[q] = a.hi[q];
    o->dx[q] = level_dx(s, a.level, q);
    o->xmin[q] = s->xmin[q] + (double)s->amr->leaves[a.geom_block].lx[q] * s->mesh.mb[q] * o->dx[q];
  }
  o->cng = s->amr_geom.cng;
  o->coarse_doubles = s->amr_geom.coarse_doubles;
  return APK_OK;
}

}  // extern "C"
