// capi.hip -- the extern "C" boundary (include/apk_amd.h).  Validates arguments on the host
// (the reference aborts with PARTHENON_FAIL on unknown options, src/hydro/hydro.cpp:299,338,
// 366; here they become error codes), then enqueues kernels on the caller's stream.
#include <cmath>
#include <cstring>
#include <limits>
#include <new>

#include "apk_internal.hpp"
#include "hydro_math.hpp"
#include "stage_form.hpp"

using namespace apk;

namespace {

hipStream_t as_stream(apk_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

bool valid_eos(const apk_eos *e) { return e && e->gamma > 1.0; }

// what is wrong with the shape of a pack, or NULL
const char *bad_pack_geometry(const apk_pack_desc &d) {
  if (d.nblocks <= 0) return "empty pack";
  if (d.nhydro != 5 && d.nhydro != 9) return "nhydro must be 5 or 9";
  if (d.nscalars < 0 || d.ng < 1 || d.nx[0] < 1 || d.nx[1] < 1 || d.nx[2] < 1) return "bad pack geometry";
  if (d.nx[1] == 1 && d.nx[2] > 1) return "nx2 == 1 requires nx3 == 1";
  const PackView t = make_view(d, nullptr);  // (explicit strides: no array may overlap the next one)
  if (d.stride[0] < 0 || d.stride[1] < 0 || d.stride[2] < 0 || t.sj < t.ni || t.sk < t.sj * t.nj || t.sn < t.sk * t.nk)
    return "pack strides smaller than the extents they step over";
  return nullptr;
}

// registry of compiled-in flux functions: src/hydro/hydro.cpp:386-416
bool in_registry(const apk_flux_cfg &c) {
  const bool recon_ok = c.recon >= APK_RC_DC && c.recon <= APK_RC_LIMO3;
  if (!recon_ok) return false;
  if (c.riemann == APK_RS_NONE || c.riemann == APK_RS_LLF) return c.recon == APK_RC_DC;
  if (c.fluid == APK_FLUID_EULER) return c.riemann == APK_RS_HLLE || c.riemann == APK_RS_HLLC;
  if (c.fluid == APK_FLUID_GLMMHD) return c.riemann == APK_RS_HLLE || c.riemann == APK_RS_HLLD;
  return false;
}

int need_nghost(int recon) {  // src/hydro/hydro.cpp:316-339
  switch (recon) {
  case APK_RC_DC: return 1;
  case APK_RC_PPM:
  case APK_RC_WENOZ: return 3;
  default: return 2;
  }
}

int cfg_status(const PackView &v, const apk_flux_cfg &cfg, const char *&why) {
  const int nh = (cfg.fluid == APK_FLUID_EULER) ? 5 : 9;
  if (!in_registry(cfg)) return why = "flux function not in registry", APK_ERR_UNSUPPORTED;
  if (v.nhydro != nh) return why = "pack nhydro does not match fluid", APK_ERR_INVALID;
  if (v.ng < need_nghost(cfg.recon)) return why = "need more ghost zones for chosen reconstruction", APK_ERR_NGHOST;
  return APK_OK;
}
int check_cfg(apk_ctx *ctx, const apk_pack *md, const apk_flux_cfg &cfg) {
  const char *why = "";
  const int rc = cfg_status(md->view, cfg, why);
  return rc == APK_OK ? rc : set_err(ctx, rc, why);
}

// apk_stage_fused's checks of its arguments against the shape of the pack (what needs the blocks' pointers stays there)
int stage_args_status(const PackView &v, const apk_stage_args &a, const char *&why) {
  if (!valid_eos(&a.eos)) return why = "apk_stage_fused: bad argument", APK_ERR_INVALID;
  const int rc = cfg_status(v, a.cfg, why);
  if (rc != APK_OK) return rc;
  if (a.cfg.riemann == APK_RS_NONE || a.cfg.riemann == APK_RS_LLF)
    return why = "fused stage: none/llf solvers use the flux-array path", APK_ERR_UNSUPPORTED;
  if (a.dedner != 0 && (a.cfg.fluid != APK_FLUID_GLMMHD || !(a.mindx > 0.0)))
    return why = "fused stage: Dedner source needs glmmhd and mindx > 0", APK_ERR_INVALID;
  if (a.phase < 0 || a.phase > 2 || (a.phase == 1) != (a.window != nullptr) ||
      (a.phase == 1 && (a.window_rl < 3 || a.window_rl > v.ni || a.window_rows < 1 || a.window_rows > v.nx2)))
    return why = "fused stage: phase / window mismatch", APK_ERR_INVALID;
  if (a.phase == 1 && a.estimate_dt && a.cfg.recon == APK_RC_DC && v.ndim == 3)
    return why = "fused stage: estimate_dt is not available in a split 3-D donor-cell stage", APK_ERR_UNSUPPORTED;
  if (a.fill_derived < 0 || a.fill_derived > 3) return why = "fused stage: fill_derived must be 0, 1, 2 or 3", APK_ERR_INVALID;
  if (a.fill_derived == 3 && !a.estimate_dt)
    return why = "fused stage: fill_derived = 3 (primitives for the time-step estimate only) needs estimate_dt", APK_ERR_INVALID;
  if (a.prim_from_cons < 0 || a.prim_from_cons > 2) return why = "fused stage: prim_from_cons must be 0, 1 or 2", APK_ERR_INVALID;
  if (a.prim_from_cons == 2 && a.cons_out_delta == 0)
    return why = "fused stage: prim_from_cons = 2 (input = u0.cons) needs an out-of-place result (cons_out_delta)", APK_ERR_INVALID;
  return APK_OK;
}

// the pack of a hypothetical stage for the legacy queries, and what of a request they fix
StagePlan plan_hypothetical(const apk_pack *u0, const apk_flux_cfg *cfg, int fill_derived, StageRequest r) {
  r.extra = fill_derived ? (fill_derived == 3 ? EXTRA_C2P_DT : EXTRA_C2P) : EXTRA_NONE;
  r.prim_to_u1 = (fill_derived >= 2) ? 1 : 0;
  r.no_prim_store = (fill_derived == 3) ? 1 : 0;
  return plan_stage(cfg->fluid, cfg->recon, u0->view, r);
}

bool same_shape(const apk_pack *a, const apk_pack *b) {
  const PackView &x = a->view, &y = b->view;
  return x.nblocks == y.nblocks && x.nvar == y.nvar && x.ni == y.ni && x.nj == y.nj &&
         x.nk == y.nk && x.ng == y.ng && x.sj == y.sj && x.sk == y.sk && x.sn == y.sn;
}

}  // namespace

namespace apk {
namespace {
// u64 = the context's device words, h = its pinned host block (device address): apk_internal.hpp names the layout
__global__ void cycle_gather_kernel(unsigned long long *u64, unsigned long long *h, const unsigned long long *tag_words, double *h_tags,
                                    int ntags) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < ntags) {
    h_tags[t] = __longlong_as_double((long long)tag_words[t]);
    const_cast<unsigned long long *>(tag_words)[t] = 0ull;
  }
  if (t == 0) {
    h[kWordStageDt] = u64[kWordStageDt];
    h[kWordFlags] = u64[kWordFlags];
    u64[kWordStageDt] = u64[kWordPlusMax];                  // +max: ready for the next reduction
    reinterpret_cast<unsigned *>(u64 + kWordFlags)[0] = 0u;  // latched flags handed over ([1], the trial stage's, stays)
  }
}
}  // namespace

int prepare_dt_word(apk_ctx *ctx, hipStream_t s) {
  if (!ctx->dt_word_clean || ctx->clean_stream != s) {
    // +max (neutral element of the min), device to device so the launch path never blocks the host
    if (hipMemcpyAsync(ctx->dt_word(), ctx->word(kWordPlusMax), sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return APK_ERR_DEVICE;
  }
  ctx->dt_word_clean = false;  // (about to be reduced into)
  ctx->last_stage_min_valid = false;
  return APK_OK;
}

int launch_cycle_gather(apk_ctx *ctx, hipStream_t s) {
  const int ntags = (ctx->tags_pending > 0 && ctx->h_partial_dev) ? ctx->tags_pending : 0;
  const int blocks = ntags > 0 ? (ntags + 255) / 256 : 1;
  hipLaunchKernelGGL(cycle_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ctx->d_u64, ctx->h_pinned_dev,
                     ctx->d_tagmax.p, ctx->h_partial_dev, ntags);
  if (hipGetLastError() != hipSuccess) return APK_ERR_DEVICE;
  ctx->dt_word_clean = true;
  ctx->clean_stream = s;
  if (ntags > 0) {
    ctx->tag_words_clean = ntags;
    ctx->tags_pending = 0;
  }
  return APK_OK;
}
}  // namespace apk

extern "C" {

int apk_version(void) { return APK_AMD_VERSION; }

int apk_fp_strict(void) {
#ifdef APK_FP_STRICT
  return 1;
#else
  return 0;
#endif
}

int apk_create(apk_ctx **out) {
  if (!out) return APK_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return APK_ERR_NO_DEVICE;
  apk_ctx *ctx = new (std::nothrow) apk_ctx();
  if (!ctx) return APK_ERR_INVALID;
  if (hipGetDevice(&ctx->device) != hipSuccess) {
    delete ctx;
    return APK_ERR_NO_DEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess ||
      std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    // kernels are compiled for gfx950 only; anything else cannot run them
    delete ctx;
    return APK_ERR_NO_DEVICE;
  }
  if (hipMalloc(&ctx->d_u64, kNumWords * sizeof(unsigned long long)) != hipSuccess ||
      hipHostMalloc(&ctx->h_pinned, kPinnedBytes, hipHostMallocDefault) != hipSuccess) {
    apk_destroy(ctx);
    return APK_ERR_DEVICE;
  }
  // the flag words ([0] latched, [1] trial stage) follow the stage's time-step word: one 16-byte read-back fetches
  // both at the end of a cycle (apk_stage_dt_flags_read)
  ctx->d_flags = reinterpret_cast<unsigned *>(ctx->word(kWordFlags));
  (void)hipMemset(ctx->d_u64, 0, kNumWords * sizeof(unsigned long long));
  {
    const double huge = 1.7976931348623157e308;  // the neutral element of the dt min
    (void)hipMemcpy(ctx->word(kWordPlusMax), &huge, sizeof(double), hipMemcpyHostToDevice);
  }
  {
    void *dev = nullptr;  // (pinned host memory is mapped into the device's address space by default; if not: copies)
    if (hipHostGetDevicePointer(&dev, ctx->h_pinned, 0) == hipSuccess) ctx->h_pinned_dev = static_cast<unsigned long long *>(dev);
    else (void)hipGetLastError();
  }
  *out = ctx;
  return APK_OK;
}

void apk_destroy(apk_ctx *ctx) {
  if (!ctx) return;
  if (ctx->d_u64) (void)hipFree(ctx->d_u64);  // (d_flags points into it)
  ctx->d_mflux.release();
  ctx->d_partial.release();
  ctx->d_tagmax.release();
  ctx->d_mark.release();
  ctx->d_du.release();
  if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
  if (ctx->h_partial) (void)hipHostFree(ctx->h_partial);
  for (auto &sp : ctx->spans) {
    (void)hipEventDestroy(sp.start);
    (void)hipEventDestroy(sp.stop);
  }
  for (auto e : ctx->free_events) (void)hipEventDestroy(e);
  delete ctx;
}

const char *apk_last_error(const apk_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int apk_pack_create(apk_ctx *ctx, const apk_pack_desc *desc, apk_pack **out) {
  if (!ctx || !desc || !out) return APK_ERR_INVALID;
  *out = nullptr;
  if (!desc->blocks) return set_err(ctx, APK_ERR_INVALID, "empty pack");
  if (const char *why = bad_pack_geometry(*desc)) return set_err(ctx, APK_ERR_INVALID, why);
  apk_pack *p = new (std::nothrow) apk_pack();
  if (!p) return APK_ERR_INVALID;
  p->h_blocks.assign(desc->blocks, desc->blocks + desc->nblocks);
  p->desc = *desc;
  p->desc.blocks = p->h_blocks.data();
  for (int d = 0; d < 3; ++d) {
    p->have_flux[d] = true;
    for (const auto &b : p->h_blocks) p->have_flux[d] = p->have_flux[d] && (b.flux[d] != nullptr);
  }
  for (const auto &b : p->h_blocks) {
    if (!b.cons) {
      delete p;
      return set_err(ctx, APK_ERR_INVALID, "block without cons pointer");
    }
  }
  const size_t bytes = sizeof(apk_block_desc) * desc->nblocks;
  hipError_t e = hipMalloc(&p->d_blocks, bytes);
  if (e == hipSuccess) e = hipMemcpy(p->d_blocks, p->h_blocks.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (p->d_blocks) (void)hipFree(p->d_blocks);
    delete p;
    return set_err(ctx, APK_ERR_DEVICE, "apk_pack_create", e);
  }
  p->view = make_view(p->desc, p->d_blocks);
  *out = p;
  return APK_OK;
}

void apk_pack_destroy(apk_pack *pack) {
  if (!pack) return;
  if (pack->d_blocks) (void)hipFree(pack->d_blocks);
  delete pack;
}

namespace {
int calculate_fluxes(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos, double c_h, int faces,
                     apk_stream_t stream, const int *face_list = nullptr, int nlist = 0, const FluxConsInput *from_cons = nullptr) {
  if (!ctx || !md || !valid_eos(eos)) return set_err(ctx, APK_ERR_INVALID, "apk_calculate_fluxes: bad argument");
  int rc = check_cfg(ctx, md, cfg);
  if (rc != APK_OK) return rc;
  for (int d = 0; d < md->view.ndim; ++d)
    if (!md->have_flux[d]) return set_err(ctx, APK_ERR_INVALID, "pack has no flux arrays");
  if (!from_cons)
    for (const auto &b : md->h_blocks)
      if (!b.prim) return set_err(ctx, APK_ERR_INVALID, "block without prim pointer");
  hipStream_t s = as_stream(stream);
  const PackView &pv = md->view;
  ScopedTiming timing(ctx, APK_T_FLUXES, s);
  if ((cfg.riemann == APK_RS_NONE || cfg.riemann == APK_RS_LLF) && faces == 2)
    return set_err(ctx, APK_ERR_UNSUPPORTED, "boundary-plane fluxes are not offered for the none / llf entries");
  if (cfg.riemann == APK_RS_NONE || cfg.riemann == APK_RS_LLF)
    rc = launch_fluxes_misc(pv, cfg.fluid, cfg.riemann, eos->gamma, c_h, s);
  else if (cfg.fluid == APK_FLUID_EULER)
    rc = (cfg.riemann == APK_RS_HLLE) ? launch_fluxes_euler_hlle(pv, cfg.recon, eos->gamma, c_h, s, faces, face_list, nlist, from_cons)
                                      : launch_fluxes_euler_hllc(pv, cfg.recon, eos->gamma, c_h, s, faces, face_list, nlist, from_cons);
  else
    rc = (cfg.riemann == APK_RS_HLLE) ? launch_fluxes_mhd_hlle(pv, cfg.recon, eos->gamma, c_h, s, faces, face_list, nlist, from_cons)
                                      : launch_fluxes_mhd_hlld(pv, cfg.recon, eos->gamma, c_h, s, faces, face_list, nlist, from_cons);
  if (rc != APK_OK) return set_err(ctx, rc, "flux kernel launch failed", hipGetLastError());
  return APK_OK;
}
}  // namespace

int apk_calculate_fluxes(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                         double c_h, apk_stream_t stream) {
  return calculate_fluxes(ctx, md, cfg, eos, c_h, 0, stream);
}

int apk_calculate_fluxes_tight(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                               double c_h, apk_stream_t stream) {
  return calculate_fluxes(ctx, md, cfg, eos, c_h, 1, stream);
}

int apk_calculate_fluxes_boundary(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                                  double c_h, apk_stream_t stream) {
  return calculate_fluxes(ctx, md, cfg, eos, c_h, 2, stream);
}

int apk_calculate_fluxes_boundary_list(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                                       double c_h, const int *faces, int nfaces, apk_stream_t stream) {
  if (!faces || nfaces < 0) return set_err(ctx, APK_ERR_INVALID, "apk_calculate_fluxes_boundary_list: bad argument");
  return calculate_fluxes(ctx, md, cfg, eos, c_h, 2, stream, faces, nfaces);
}

int apk_calculate_fluxes_boundary_list_from_cons(apk_ctx *ctx, const apk_pack *md, apk_flux_cfg cfg, const apk_eos *eos,
                                                 double c_h, const int *faces, int nfaces, long long cons_delta,
                                                 apk_stream_t stream) {
  if (!faces || nfaces < 0 || !valid_eos(eos))
    return set_err(ctx, APK_ERR_INVALID, "apk_calculate_fluxes_boundary_list_from_cons: bad argument");
  // (the stencil cells are converted by the lean ConsToPrim, and nothing writes a floored value back)
  if (!eos_is_lean(*eos) || eos->dfloor > 0.0 || eos->efloor > 0.0)
    return set_err(ctx, APK_ERR_UNSUPPORTED, "apk_calculate_fluxes_boundary_list_from_cons: floors / ceilings need the stored primitives");
  if (cfg.riemann == APK_RS_NONE || cfg.riemann == APK_RS_LLF)
    return set_err(ctx, APK_ERR_UNSUPPORTED, "boundary-plane fluxes are not offered for the none / llf entries");
  const StageConsts k = make_stage_consts(eos->gamma, c_h, *eos);
  const FluxConsInput ci{(int64_t)cons_delta, *eos, k.eos_gm1, k.vceil_sq, k.pfloor_over_gm1};
  const int rc = calculate_fluxes(ctx, md, cfg, eos, c_h, 2, stream, faces, nfaces, &ci);
  return rc;
}

int apk_update_with_flux_divergence(apk_ctx *ctx, const apk_pack *u0, const apk_pack *u1,
                                    double gam0, double gam1, double beta_dt,
                                    apk_stream_t stream) {
  if (!ctx || !u0 || !u1 || !same_shape(u0, u1))
    return set_err(ctx, APK_ERR_INVALID, "apk_update_with_flux_divergence: bad argument");
  for (int d = 0; d < u0->view.ndim; ++d)
    if (!u0->have_flux[d]) return set_err(ctx, APK_ERR_INVALID, "u0 pack has no flux arrays");
  ScopedTiming timing(ctx, APK_T_UPDATE, as_stream(stream));
  int rc = launch_update_flux_div(u0->view, u1->view, gam0, gam1, beta_dt, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "update kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_dedner_source(apk_ctx *ctx, const apk_pack *md, int extended, double alpha, double c_h,
                      double mindx, double beta_dt, apk_stream_t stream) {
  if (!ctx || !md || md->view.nhydro != 9 || !(mindx > 0.0))
    return set_err(ctx, APK_ERR_INVALID, "apk_dedner_source: bad argument");
  // Mignone & Tzeferacos 2010 (27): dedner_source.cpp:32
  const double coeff = std::exp(-alpha * c_h * beta_dt / mindx);
  ScopedTiming timing(ctx, APK_T_DEDNER, as_stream(stream));
  int rc = launch_dedner(md->view, extended, coeff, beta_dt, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "dedner kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_stage_fused(apk_ctx *ctx, const apk_pack *u0, const apk_pack *u1,
                    const apk_stage_args *a, apk_stream_t stream) {
  if (!ctx || !u0 || !u1 || !a || !same_shape(u0, u1))
    return set_err(ctx, APK_ERR_INVALID, "apk_stage_fused: bad argument");
  const char *why = "fused stage: not supported";
  int rc = stage_args_status(u0->view, *a, why);
  if (rc != APK_OK) return set_err(ctx, rc, why);
  if (a->prim_from_cons) {
    for (const apk_block_desc &b : u1->h_blocks)
      if (!b.cons) return set_err(ctx, APK_ERR_INVALID, "fused stage: prim_from_cons needs u1.cons");
  }
  if (a->fill_derived == 2) {
    for (const apk_block_desc &b : u1->h_blocks)
      if (!b.prim) return set_err(ctx, APK_ERR_INVALID, "fused stage: fill_derived = 2 needs prim arrays in u1");
    for (size_t b = 0; b < u0->h_blocks.size(); ++b)
      if (u0->h_blocks[b].prim == u1->h_blocks[b].prim)
        return set_err(ctx, APK_ERR_INVALID, "fused stage: fill_derived = 2 needs u1.prim distinct from u0.prim");
  }
  double coeff = 1.0;
  if (a->dedner != 0) coeff = std::exp(-a->glmmhd_alpha * a->c_h * a->beta_dt / a->mindx);
  rc = launch_stage_fused(ctx, u0->view, u1->view, *a, coeff, as_stream(stream), why);
  if (rc == APK_ERR_DEVICE) return set_err(ctx, rc, "fused stage kernel launch failed", hipGetLastError());
  return rc == APK_OK ? rc : set_err(ctx, rc, why);
}

int apk_stage_form(const apk_pack_desc *shape, const apk_stage_args *args, apk_stage_form_info *out) {
  if (!shape || !args || !out) return APK_ERR_INVALID;
  *out = apk_stage_form_info{APK_FORM_NONE, 0, 0, 0, 0, ""};
  if ((out->reason = bad_pack_geometry(*shape))) return APK_ERR_INVALID;
  out->reason = "";
  const PackView v = make_view(*shape, nullptr);
  const int rc = stage_args_status(v, *args, out->reason);
  if (rc != APK_OK) return rc;
  const StagePlan p = plan_stage_args(v, *args);
  *out = apk_stage_form_info{p.form, p.lean, p.dc_rows, p.from_cons, p.x1_halo ? 1 : 0, p.reason};
  return p.status;
}

int apk_stage_unphysical_read(apk_ctx *ctx, long long *count, apk_stream_t stream) {
  if (!ctx || !count) return APK_ERR_INVALID;
  unsigned long long n = 0;
  const int rc = counter_fetch(ctx, kWordStageBad, &n, as_stream(stream));
  *count = (long long)n;
  return rc;
}

// The three older queries: each describes a hypothetical whole stage on this pack, asks the plan and reads the form.
int apk_stage_split_axis(const apk_pack *u0, const apk_flux_cfg *cfg, int fill_derived) {
  if (!u0 || !cfg) return 0;
  // (of fill_derived only "in place, out of place or none": the layout of the windows does not depend on the rest)
  switch (plan_hypothetical(u0, cfg, fill_derived > 2 ? 2 : fill_derived, StageRequest{}).form) {
  case APK_FORM_DC_MARCH:
  case APK_FORM_MARCH12_X3: return 0;  // single-kernel stage: 3-D index windows
  case APK_FORM_TWO_KERNEL: return 3;
  default: return 1;
  }
}

int apk_stage_x1_halo(const apk_pack *u0, const apk_flux_cfg *cfg, const apk_eos *eos, int fill_derived, int dedner, int prim_from_cons) {
  if (!u0 || !cfg || !eos) return 0;
  if (cfg->riemann == APK_RS_NONE || cfg->riemann == APK_RS_LLF) return 0;
  // (asked of the scheme's plain prim-free stage whatever fill_derived is: on the safe side for the stages with FillDerived,
  // which keep the two kernels)
  if (cfg->recon != APK_RC_DC && prim_from_cons && apk_stage_single_march(u0, cfg)) return 0;
  StageRequest r;
  r.scalars = u0->view.nvar != u0->view.nhydro;
  r.eos = *eos;
  r.dedner = dedner;
  r.prim_from_cons = prim_from_cons;
  r.out_of_place = prim_from_cons == 2;  // (such a stage writes its result elsewhere: the caller's business)
  r.x1_halo = true;
  return plan_hypothetical(u0, cfg, fill_derived, r).status == APK_OK ? 1 : 0;
}

int apk_stage_single_march(const apk_pack *u0, const apk_flux_cfg *cfg) {
  if (!u0 || !cfg) return 0;
  StageRequest r;  // a whole-block lean stage whose input is a conserved state
  r.prim_from_cons = 1;
  return plan_hypothetical(u0, cfg, 0, r).form == APK_FORM_SINGLE_MARCH ? 1 : 0;
}

int apk_cons_to_prim(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                     apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim: bad argument");
  ScopedTiming timing(ctx, APK_T_C2P, as_stream(stream));
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_dt(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, int ghost_depth, apk_stream_t stream) {
  return apk_cons_to_prim_dt_skip(ctx, md, fluid, eos, ghost_depth, nullptr, stream);
}

int apk_cons_to_prim_dt_skip(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, int ghost_depth, const int *face_neighbor,
                             apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_dt: bad argument");
  hipStream_t s = as_stream(stream);
  unsigned long long *dt_bits = ctx->dt_word();  // the stage's word: apk_stage_dt_read / apk_stage_dt_flags_read
  if (apk::prepare_dt_word(ctx, s) != APK_OK) return set_err(ctx, APK_ERR_DEVICE, "time-step word reset", hipGetLastError());
  ScopedTiming timing(ctx, APK_T_C2P, s);
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, s, false, nullptr, 0, false, face_neighbor, dt_bits, ghost_depth);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_dt_select(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, int ghost_depth, const int *face_neighbor,
                               unsigned store_vars, apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9) || ghost_depth < 0 || ghost_depth > md->view.ng)
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_dt_select: bad argument");
  if (md->view.nvar != md->view.nhydro || (store_vars >> md->view.nhydro) != 0u)
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_dt_select: store_vars names the hydro primitives of a pack without passive scalars");
  // (a floor or ceiling writes conserved values back that belong with ALL primitives of the cell)
  if (!eos_is_lean(*eos) || eos->dfloor > 0.0 || eos->efloor > 0.0)
    return set_err(ctx, APK_ERR_UNSUPPORTED, "apk_cons_to_prim_dt_select: floors / ceilings need the full ConsToPrim");
  hipStream_t s = as_stream(stream);
  unsigned long long *dt_bits = ctx->dt_word();  // the stage's word: apk_stage_dt_read / apk_stage_dt_flags_read
  if (apk::prepare_dt_word(ctx, s) != APK_OK) return set_err(ctx, APK_ERR_DEVICE, "time-step word reset", hipGetLastError());
  ScopedTiming timing(ctx, APK_T_C2P, s);
  // (store_vars = every primitive is the pass apk_cons_to_prim_dt_skip runs; ~0u is the kernels' word for it)
  const unsigned all = (1u << md->view.nhydro) - 1u;
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, s, false, nullptr, 0, false, face_neighbor, dt_bits, ghost_depth,
                               store_vars == all ? ~0u : store_vars);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_faces(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_faces: bad argument");
  ScopedTiming timing(ctx, APK_T_C2P, as_stream(stream));
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, as_stream(stream), false, nullptr, 0, true);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_faces_skip(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const int *face_neighbor,
                                apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9) || !face_neighbor)
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_faces_skip: bad argument");
  ScopedTiming timing(ctx, APK_T_C2P, as_stream(stream));
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, as_stream(stream), false, nullptr, 0, true, face_neighbor);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_faces_dt(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const int *face_neighbor,
                              apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_faces_dt: bad argument");
  hipStream_t s = as_stream(stream);
  unsigned long long *dt_bits = ctx->dt_word();  // the stage's word: apk_stage_dt_read / apk_stage_dt_flags_read
  if (apk::prepare_dt_word(ctx, s) != APK_OK) return set_err(ctx, APK_ERR_DEVICE, "time-step word reset", hipGetLastError());
  ScopedTiming timing(ctx, APK_T_C2P, s);
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, s, false, nullptr, 0, true, face_neighbor, dt_bits);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_ghosts(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                            apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_ghosts: bad argument");
  ScopedTiming timing(ctx, APK_T_C2P, as_stream(stream));
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, as_stream(stream), true);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_cons_to_prim_ghosts_split(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                                  const unsigned *late_regions, int part, apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD) ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9) || !late_regions || (part != 1 && part != 2))
    return set_err(ctx, APK_ERR_INVALID, "apk_cons_to_prim_ghosts_split: bad argument");
  ScopedTiming timing(ctx, APK_T_C2P, as_stream(stream));
  int rc = launch_cons_to_prim(md->view, fluid, *eos, ctx->d_flags, as_stream(stream), true, late_regions, part);
  if (rc != APK_OK) return set_err(ctx, rc, "cons_to_prim kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_stage_dt_read(apk_ctx *ctx, double cfl, double *dt_out, apk_stream_t stream) {
  if (!ctx || !dt_out) return APK_ERR_INVALID;
  if (ctx->last_stage_min_valid) {  // (apk_stage_dt_flags_read has taken the minimum out of the device word)
    *dt_out = cfl * ctx->last_stage_min;
    return APK_OK;
  }
  hipStream_t s = as_stream(stream);
  unsigned long long *h = ctx->pinned_u64() + kWordStageDt;
  APK_HIP_TRY(ctx, hipMemcpyAsync(h, ctx->dt_word(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  APK_HIP_TRY(ctx, hipStreamSynchronize(s));
  double m;
  std::memcpy(&m, h, sizeof(m));
  *dt_out = cfl * m;  // hydro.cpp:909
  return APK_OK;
}

int apk_estimate_timestep(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos,
                          double cfl, double *dt_out, apk_stream_t stream) {
  if (!ctx || !md || !valid_eos(eos) || !dt_out ||
      md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_estimate_timestep: bad argument");
  hipStream_t s = as_stream(stream);
  int rc = min_seed(ctx, std::numeric_limits<double>::max(), s);
  if (rc != APK_OK) return rc;
  {
    ScopedTiming timing(ctx, APK_T_MIN_DT, s);
    rc = launch_min_dt(md->view, fluid, eos->gamma, ctx->min_word(), s);
  }
  if (rc != APK_OK) return set_err(ctx, rc, "min_dt kernel launch failed", hipGetLastError());
  double m;
  if ((rc = min_fetch(ctx, &m, s)) != APK_OK) return rc;
  *dt_out = cfl * m;  // hydro.cpp:909
  return APK_OK;
}

namespace {
// the subset of CalcDiffFluxes this library implements (diffusion.cpp:18-53): fixed coefficients, and Spitzer conduction
// where the caller hands in its numbers.  *sp: what the launchers get -- `spitzer` where the configuration reads it
int check_diff_cfg(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *c, const apk_spitzer_cfg *spitzer,
                   const apk_spitzer_cfg **sp) {
  *sp = nullptr;
  if (!c) return set_err(ctx, APK_ERR_INVALID, "diffusion: cfg is NULL");
  if (c->conduction < APK_COND_NONE || c->conduction > APK_COND_ANISOTROPIC || c->viscosity < APK_VISC_NONE ||
      c->viscosity > APK_VISC_ISOTROPIC || c->resistivity < APK_RES_NONE || c->resistivity > APK_RES_OHMIC)
    return set_err(ctx, APK_ERR_INVALID, "diffusion: unknown process");
  if (c->conduction != APK_COND_NONE && c->conduction_coeff == APK_CONDC_SPITZER) {
    if (!spitzer)
      return set_err(ctx, APK_ERR_UNSUPPORTED, "diffusion: Spitzer conduction needs its units (an apk_spitzer_cfg, the _v2 entry points)");
    if (!(spitzer->coeff_code > 0.0) || !(spitzer->mbar > 0.0) || !(spitzer->k_boltzmann > 0.0))
      return set_err(ctx, APK_ERR_INVALID, "diffusion: apk_spitzer_cfg members must be positive");
    *sp = spitzer;
  } else if (c->conduction != APK_COND_NONE && c->conduction_coeff != APK_CONDC_FIXED) {
    return set_err(ctx, APK_ERR_UNSUPPORTED, "diffusion: unknown conduction coefficient");
  }
  if ((c->viscosity != APK_VISC_NONE && c->viscosity_coeff != APK_VISCC_FIXED) ||
      (c->resistivity != APK_RES_NONE && c->resistivity_coeff != APK_RESC_FIXED))
    return set_err(ctx, APK_ERR_UNSUPPORTED, "diffusion: viscosity and resistivity support fixed coefficients only");
  if ((c->resistivity != APK_RES_NONE || c->conduction == APK_COND_ANISOTROPIC) && md->view.nhydro != 9)
    return set_err(ctx, APK_ERR_INVALID, "diffusion: resistivity and anisotropic conduction need a GLM-MHD pack");
  if (md->view.ng < 1) return set_err(ctx, APK_ERR_NGHOST, "diffusion: needs one ghost layer");
  return APK_OK;
}
}  // namespace

int apk_calc_diff_fluxes(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg, apk_stream_t stream) {
  return apk_calc_diff_fluxes_v2(ctx, md, cfg, nullptr, stream);
}

int apk_calc_diff_fluxes_v2(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg, const apk_spitzer_cfg *spitzer,
                            apk_stream_t stream) {
  if (!ctx || !md) return set_err(ctx, APK_ERR_INVALID, "apk_calc_diff_fluxes: bad argument");
  const apk_spitzer_cfg *sp;
  int rc = check_diff_cfg(ctx, md, cfg, spitzer, &sp);
  if (rc != APK_OK) return rc;
  for (int d = 0; d < md->view.ndim; ++d)
    if (!md->have_flux[d]) return set_err(ctx, APK_ERR_INVALID, "apk_calc_diff_fluxes: pack has no flux arrays");
  rc = launch_diff_fluxes(md->view, cfg->conduction, cfg->viscosity != APK_VISC_NONE, cfg->resistivity != APK_RES_NONE,
                          cfg->thermal_diff_coeff, cfg->conduction_sat_prefac, cfg->mom_diff_coeff, cfg->ohm_diff_coeff, sp,
                          as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "diffusion flux kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_estimate_diffusion_timestep(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg, double cfl_diff,
                                    double *dt_out, apk_stream_t stream) {
  return apk_estimate_diffusion_timestep_v2(ctx, md, cfg, nullptr, cfl_diff, dt_out, stream);
}

int apk_estimate_diffusion_timestep_v2(apk_ctx *ctx, const apk_pack *md, const apk_diff_cfg *cfg,
                                       const apk_spitzer_cfg *spitzer, double cfl_diff, double *dt_out, apk_stream_t stream) {
  if (!ctx || !md || !dt_out) return set_err(ctx, APK_ERR_INVALID, "apk_estimate_diffusion_timestep: bad argument");
  const apk_spitzer_cfg *sp;
  int rc = check_diff_cfg(ctx, md, cfg, spitzer, &sp);
  if (rc != APK_OK) return rc;
  const double huge = std::numeric_limits<double>::max();
  const PackView &v = md->view;
  const double fac = v.ndim == 1 ? 0.5 : (v.ndim == 2 ? 0.25 : 1.0 / 6.0);
  // a fixed isotropic coefficient: min over cells of Dxc_d^2 / (coeff + TINY), the same for every cell of a block
  auto iso_fixed = [&](double coeff) {
    double m = huge;
    for (const apk_block_desc &b : md->h_blocks)
      for (int d = 0; d < v.ndim; ++d) m = std::fmin(m, b.dx[d] * b.dx[d] / (coeff + 1.0e-20));
    return cfl_diff * fac * m;
  };
  double dt = huge;
  if (cfg->conduction == APK_COND_ISOTROPIC && !sp) {
    dt = std::fmin(dt, iso_fixed(cfg->thermal_diff_coeff));
  } else if (cfg->conduction != APK_COND_NONE) {  // the general branch: anisotropic, or Spitzer
    hipStream_t s = as_stream(stream);
    if ((rc = min_seed(ctx, huge, s)) != APK_OK) return rc;
    rc = launch_cond_dt(v, cfg->conduction, cfg->thermal_diff_coeff, cfg->conduction_sat_prefac, sp, ctx->min_word(), s);
    if (rc != APK_OK) return set_err(ctx, rc, "conduction dt kernel launch failed", hipGetLastError());
    double m;
    if ((rc = min_fetch(ctx, &m, s)) != APK_OK) return rc;
    dt = std::fmin(dt, cfl_diff * fac * m);
  }
  if (cfg->viscosity != APK_VISC_NONE) dt = std::fmin(dt, iso_fixed(cfg->mom_diff_coeff));
  if (cfg->resistivity != APK_RES_NONE) dt = std::fmin(dt, iso_fixed(cfg->ohm_diff_coeff));
  *dt_out = dt;
  return APK_OK;
}

// ---- RKL2 super-time-stepping (hydro_driver.cpp:93-344) -----------------------------------------------------------
// (apk_rkl2_num_stages / apk_rkl2_coefficients: host/sts.cpp, compiled without the kernels' fast-math flags)
int apk_flux_divergence(apk_ctx *ctx, const apk_pack *md, const apk_pack *out, apk_stream_t stream) {
  if (!ctx || !md || !out || !same_shape(md, out)) return set_err(ctx, APK_ERR_INVALID, "apk_flux_divergence: bad argument");
  for (int d = 0; d < md->view.ndim; ++d)
    if (!md->have_flux[d]) return set_err(ctx, APK_ERR_INVALID, "apk_flux_divergence: pack has no flux arrays");
  int rc = launch_flux_divergence(md->view, out->d_blocks, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "flux divergence kernel launch failed", hipGetLastError());
  return APK_OK;
}

namespace {
// the four registers of a sub-stage: same shape, and the ones written distinct from each other and from Y0
int check_rkl2_regs(apk_ctx *ctx, const char *who, const apk_pack *y0, const apk_pack *yjm1, const apk_pack *yjm2, const apk_pack *my0) {
  if (!ctx || !y0 || !yjm1 || !yjm2 || !my0 || !same_shape(yjm1, y0) || !same_shape(yjm1, yjm2) || !same_shape(yjm1, my0))
    return set_err(ctx, APK_ERR_INVALID, who);
  for (size_t b = 0; b < yjm1->h_blocks.size(); ++b) {
    const double *p[4] = {y0->h_blocks[b].cons, yjm1->h_blocks[b].cons, yjm2->h_blocks[b].cons, my0->h_blocks[b].cons};
    for (int i = 0; i < 4; ++i)
      for (int q = i + 1; q < 4; ++q)
        if (!p[i] || p[i] == p[q]) return set_err(ctx, APK_ERR_INVALID, who);
  }
  return APK_OK;
}
}  // namespace

int apk_rkl2_step_first(apk_ctx *ctx, const apk_pack *y0, const apk_pack *yjm1, const apk_pack *yjm2, const apk_pack *my0,
                        int s_rkl, double tau, apk_stream_t stream) {
  int rc = check_rkl2_regs(ctx, "apk_rkl2_step_first: bad argument", y0, yjm1, yjm2, my0);
  if (rc != APK_OK) return rc;
  double mu, nu, mu_tilde_1, gamma_tilde;
  if (apk_rkl2_coefficients(s_rkl, 1, &mu, &nu, &mu_tilde_1, &gamma_tilde) != APK_OK)
    return set_err(ctx, APK_ERR_INVALID, "apk_rkl2_step_first: s_rkl must be >= 2");
  rc = launch_rkl2_step_first(yjm1->view, y0->d_blocks, yjm2->d_blocks, my0->d_blocks, mu_tilde_1, tau, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "RKL2 first step kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_rkl2_step_other(apk_ctx *ctx, const apk_pack *y0, const apk_pack *yjm1, const apk_pack *yjm2, const apk_pack *my0,
                        double mu_j, double nu_j, double mu_tilde_j, double gamma_tilde_j, double tau, apk_stream_t stream) {
  int rc = check_rkl2_regs(ctx, "apk_rkl2_step_other: bad argument", y0, yjm1, yjm2, my0);
  if (rc != APK_OK) return rc;
  for (int d = 0; d < yjm1->view.ndim; ++d)
    if (!yjm1->have_flux[d]) return set_err(ctx, APK_ERR_INVALID, "apk_rkl2_step_other: Yjm1 has no flux arrays");
  rc = launch_rkl2_step_other(yjm1->view, y0->d_blocks, yjm2->d_blocks, my0->d_blocks, mu_j, nu_j, mu_tilde_j, gamma_tilde_j, tau,
                              as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "RKL2 step kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_rkl2_substage_fused(apk_ctx *ctx, const apk_pack *md, const apk_rkl2_regs *regs, const apk_diff_cfg *cfg,
                            const apk_rkl2_coeffs *coeffs, double tau, int first, apk_stream_t stream) {
  return apk_rkl2_substage_fused_v2(ctx, md, regs, cfg, nullptr, coeffs, tau, first, stream);
}

int apk_rkl2_substage_fused_v2(apk_ctx *ctx, const apk_pack *md, const apk_rkl2_regs *regs, const apk_diff_cfg *cfg,
                               const apk_spitzer_cfg *spitzer, const apk_rkl2_coeffs *coeffs, double tau, int first,
                               apk_stream_t stream) {
  if (!regs || !coeffs) return set_err(ctx, APK_ERR_INVALID, "apk_rkl2_substage_fused: bad argument");
  int rc = check_rkl2_regs(ctx, "apk_rkl2_substage_fused: bad argument", regs->y0, md, regs->yjm2, regs->my0);
  if (rc != APK_OK) return rc;
  const apk_spitzer_cfg *sp;
  if ((rc = check_diff_cfg(ctx, md, cfg, spitzer, &sp)) != APK_OK) return rc;
  for (const apk_block_desc &b : md->h_blocks)
    if (!b.prim) return set_err(ctx, APK_ERR_INVALID, "apk_rkl2_substage_fused: the pack has no primitives");
  rc = launch_rkl2_substage_fused(md->view, regs->y0->d_blocks, regs->yjm2->d_blocks, regs->my0->d_blocks, cfg->conduction,
                                  cfg->viscosity != APK_VISC_NONE, cfg->resistivity != APK_RES_NONE, cfg->thermal_diff_coeff,
                                  cfg->conduction_sat_prefac, cfg->mom_diff_coeff, cfg->ohm_diff_coeff, sp, coeffs->mu, coeffs->nu,
                                  coeffs->mu_tilde, coeffs->gamma_tilde, tau, first != 0, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "fused RKL2 sub-stage kernel launch failed", hipGetLastError());
  return APK_OK;
}

int apk_first_order_flux_correct(apk_ctx *ctx, const apk_pack *u0, const apk_pack *u1, int fluid,
                                 const apk_eos *eos, double c_h, double gam0, double gam1,
                                 double beta_dt, long long *num_corrected, apk_stream_t stream) {
  if (!ctx || !u0 || !u1 || !same_shape(u0, u1) || !valid_eos(eos) ||
      u0->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_first_order_flux_correct: bad argument");
  for (int d = 0; d < u0->view.ndim; ++d)
    if (!u0->have_flux[d]) return set_err(ctx, APK_ERR_INVALID, "u0 pack has no flux arrays");
  hipStream_t s = as_stream(stream);
  int rc = ctx->d_mark.reserve(ctx, (size_t)u0->view.nblocks * (size_t)u0->view.sn, s);
  if (rc != APK_OK) return rc;
  long long total = 0;
  unsigned long long corrected = 0;
  int attempts = 0;
  do {  // hydro.cpp:1265-1339: <= 4 attempts, one host sync per attempt
    APK_HIP_TRY(ctx, hipMemsetAsync(ctx->counter_word(), 0, sizeof(unsigned long long), s));
    rc = launch_fofc_mark(u0->view, u1->view, fluid, gam0, gam1, beta_dt, attempts, ctx->d_mark.p,
                          ctx->counter_word(), s);
    if (rc != APK_OK) return set_err(ctx, rc, "fofc mark kernel launch failed", hipGetLastError());
    if ((rc = counter_fetch(ctx, kWordCounter, &corrected, s)) != APK_OK) return rc;
    if (corrected > 0) {
      rc = launch_fofc_fix(u0->view, fluid, eos->gamma, c_h, ctx->d_mark.p, s);
      if (rc != APK_OK) return set_err(ctx, rc, "fofc fix kernel launch failed", hipGetLastError());
    }
    total += (long long)corrected;
    attempts += 1;
  } while (corrected > 0 && attempts < 4);
  if (num_corrected) *num_corrected = total;
  return APK_OK;
}

int apk_count_unphysical(apk_ctx *ctx, const apk_pack *md, int fluid, long long *count, apk_stream_t stream) {
  if (!ctx || !md || !count || md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_count_unphysical: bad argument");
  hipStream_t s = as_stream(stream);
  APK_HIP_TRY(ctx, hipMemsetAsync(ctx->counter_word(), 0, sizeof(unsigned long long), s));
  int rc = launch_count_unphysical(md->view, fluid, ctx->counter_word(), s);
  if (rc != APK_OK) return set_err(ctx, rc, "count_unphysical launch failed", hipGetLastError());
  unsigned long long n = 0;
  rc = counter_fetch(ctx, kWordCounter, &n, s);
  *count = (long long)n;
  return rc;
}

int apk_history(apk_ctx *ctx, const apk_pack *md, int fluid, double *out8, apk_stream_t stream) {
  if (!ctx || !md || !out8 || md->view.nhydro != ((fluid == APK_FLUID_EULER) ? 5 : 9))
    return set_err(ctx, APK_ERR_INVALID, "apk_history: bad argument");
  hipStream_t s = as_stream(stream);
  int nwg = 0;
  launch_history(md->view, fluid, nullptr, &nwg, nullptr, s);
  int rc = ctx->d_partial.reserve(ctx, (size_t)nwg * 8 + 8, s);
  if (rc != APK_OK) return rc;
  double *d_out = ctx->d_partial.p + (size_t)nwg * 8;
  rc = launch_history(md->view, fluid, ctx->d_partial.p, &nwg, d_out, s);
  if (rc != APK_OK) return set_err(ctx, rc, "history kernel launch failed", hipGetLastError());
  double *h = ctx->pinned_history();
  APK_HIP_TRY(ctx, hipMemcpyAsync(h, d_out, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
  APK_HIP_TRY(ctx, hipStreamSynchronize(s));
  std::memcpy(out8, h, 8 * sizeof(double));
  return APK_OK;
}

int apk_stage_dt_flags_read(apk_ctx *ctx, double cfl, double *dt_out, unsigned *flags, apk_stream_t stream) {
  if (!ctx || !dt_out || !flags) return APK_ERR_INVALID;
  hipStream_t s = as_stream(stream);
  const unsigned long long *h = ctx->pinned_u64();
  if (ctx->last_stage_min_valid) {  // (already consumed: the word on the device has been reset)
    *dt_out = cfl * ctx->last_stage_min;
    return apk_poll_device_flags(ctx, flags, stream);
  }
  if (ctx->h_pinned_dev) {
    // one small kernel hands the time-step and flag words (and the tag criteria an apk_tag_blocks_begin left pending) to
    // the host and leaves the device words ready for the next cycle
    if (apk::launch_cycle_gather(ctx, s) != APK_OK) return set_err(ctx, APK_ERR_DEVICE, "cycle gather launch", hipGetLastError());
  } else {
    // the stage's minimum and the flag words that follow it in one copy
    APK_HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned_u64() + kWordStageDt, ctx->dt_word(), 2 * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, s));
    APK_HIP_TRY(ctx, hipMemsetAsync(ctx->d_flags, 0, sizeof(unsigned), s));
    // (the same consume-on-read semantics as the gather kernel's: the word back to +max, ready for the next reduction)
    APK_HIP_TRY(ctx, hipMemcpyAsync(ctx->dt_word(), ctx->word(kWordPlusMax), sizeof(double), hipMemcpyDeviceToDevice, s));
    ctx->dt_word_clean = true;
    ctx->clean_stream = s;
  }
  APK_HIP_TRY(ctx, hipStreamSynchronize(s));
  double m;
  std::memcpy(&m, h + kWordStageDt, sizeof(m));
  ctx->last_stage_min = m;
  ctx->last_stage_min_valid = true;
  *dt_out = cfl * m;  // hydro.cpp:909
  unsigned f[2];
  std::memcpy(f, h + kWordFlags, sizeof(f));
  *flags = f[0];
  return APK_OK;
}

namespace {
__global__ void commit_trial_flags_kernel(unsigned *f) {
  if (f[1]) atomicOr(f, f[1]);
  f[1] = 0u;
}
}  // namespace

int apk_trial_flags(apk_ctx *ctx, int keep, apk_stream_t stream) {
  if (!ctx) return APK_ERR_INVALID;
  hipStream_t s = as_stream(stream);
  if (keep) {
    hipLaunchKernelGGL(commit_trial_flags_kernel, dim3(1), dim3(1), 0, s, ctx->d_flags);
    if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "apk_trial_flags: launch failed");
  } else {
    APK_HIP_TRY(ctx, hipMemsetAsync(ctx->d_flags + 1, 0, sizeof(unsigned), s));
  }
  return APK_OK;
}

int apk_poll_device_flags(apk_ctx *ctx, unsigned *flags, apk_stream_t stream) {
  if (!ctx || !flags) return APK_ERR_INVALID;
  hipStream_t s = as_stream(stream);
  unsigned *h = ctx->pinned_polled_flags();
  APK_HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  APK_HIP_TRY(ctx, hipMemsetAsync(ctx->d_flags, 0, sizeof(unsigned), s));
  APK_HIP_TRY(ctx, hipStreamSynchronize(s));
  *flags = *h;
  return APK_OK;
}

int apk_copy_plan_create(apk_ctx *ctx, const apk_copy_region *regions, int n,
                         apk_copy_plan **out) {
  if (!ctx || !out || n < 0 || (n > 0 && !regions)) return APK_ERR_INVALID;
  apk_copy_plan *p = new (std::nothrow) apk_copy_plan();
  if (!p) return APK_ERR_INVALID;
  p->n = n;
  for (int r = 0; r < n; ++r) {
    const int64_t c = (int64_t)regions[r].ext[0] * regions[r].ext[1] * regions[r].ext[2];
    if (c > p->max_cells) p->max_cells = c;
    if (c * regions[r].nvar > p->max_items) p->max_items = c * regions[r].nvar;
  }
  if (n > 0) {
    std::vector<apk_copy_chunk> by_items, by_cells;
    for (int r = 0; r < n; ++r) {
      const int64_t c = (int64_t)regions[r].ext[0] * regions[r].ext[1] * regions[r].ext[2];
      const int64_t items = c * regions[r].nvar;
      if (items >= (int64_t)1 << 31) {
        delete p;
        return set_err(ctx, APK_ERR_INVALID, "apk_copy_plan_create: box too large");
      }
      for (int64_t f = 0; f < items; f += kCopyChunkItems) by_items.push_back({r, (int)f});
      for (int64_t f = 0; f < c; f += kCopyChunkCells) by_cells.push_back({r, (int)f});
    }
    p->nchunks_items = (int)by_items.size();
    p->nchunks_cells = (int)by_cells.size();
    hipError_t e = hipMalloc(&p->d_regions, sizeof(apk_copy_region) * n);
    if (e == hipSuccess)
      e = hipMemcpy(p->d_regions, regions, sizeof(apk_copy_region) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && !by_items.empty()) {
      e = hipMalloc(&p->d_chunks_items, sizeof(apk_copy_chunk) * by_items.size());
      if (e == hipSuccess)
        e = hipMemcpy(p->d_chunks_items, by_items.data(), sizeof(apk_copy_chunk) * by_items.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !by_cells.empty()) {
      e = hipMalloc(&p->d_chunks_cells, sizeof(apk_copy_chunk) * by_cells.size());
      if (e == hipSuccess)
        e = hipMemcpy(p->d_chunks_cells, by_cells.data(), sizeof(apk_copy_chunk) * by_cells.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      apk_copy_plan_destroy(p);
      return set_err(ctx, APK_ERR_DEVICE, "apk_copy_plan_create", e);
    }
  }
  *out = p;
  return APK_OK;
}

void apk_copy_plan_destroy(apk_copy_plan *plan) {
  if (!plan) return;
  if (plan->d_regions) (void)hipFree(plan->d_regions);
  if (plan->d_chunks_items) (void)hipFree(plan->d_chunks_items);
  if (plan->d_chunks_cells) (void)hipFree(plan->d_chunks_cells);
  delete plan;
}

int apk_copy_plan_run(apk_ctx *ctx, const apk_copy_plan *plan, apk_stream_t stream) {
  if (!ctx || !plan) return APK_ERR_INVALID;
  if (plan->n <= 0) return APK_OK;
  ScopedTiming timing(ctx, APK_T_COPY, as_stream(stream));
  int rc = launch_copy_regions(*plan, as_stream(stream));
  if (rc != APK_OK) return set_err(ctx, rc, "copy kernel launch failed", hipGetLastError());
  return APK_OK;
}

namespace {
int copy_plan_run_c2p(apk_ctx *ctx, const apk_copy_plan *plan, int fluid, const apk_eos *eos, int64_t prim_delta, int latch_flags,
                      bool prim_only, apk_stream_t stream) {
  if (!ctx || !plan || !valid_eos(eos) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD))
    return set_err(ctx, APK_ERR_INVALID, "apk_copy_plan_run_c2p: bad argument");
  if (eos->dfloor > 0.0 || eos->pfloor > 0.0 || eos->efloor > 0.0 || eos->vceil < 1.0e300 || eos->eceil < 1.0e300)
    return set_err(ctx, APK_ERR_UNSUPPORTED, "apk_copy_plan_run_c2p: floors / ceilings are active; copy, then apk_cons_to_prim_ghosts");
  if (plan->n <= 0) return APK_OK;
  ScopedTiming timing(ctx, APK_T_COPY, as_stream(stream));
  int rc = launch_copy_regions(*plan, as_stream(stream), fluid, eos, latch_flags ? ctx->d_flags : nullptr, prim_delta, prim_only);
  if (rc != APK_OK) return set_err(ctx, rc, "copy kernel launch failed", hipGetLastError());
  return APK_OK;
}
}  // namespace

int apk_copy_plan_run_c2p(apk_ctx *ctx, const apk_copy_plan *plan, int fluid, const apk_eos *eos, int64_t prim_delta,
                          int latch_flags, apk_stream_t stream) {
  return copy_plan_run_c2p(ctx, plan, fluid, eos, prim_delta, latch_flags, false, stream);
}

int apk_copy_plan_run_c2p_prim_only(apk_ctx *ctx, const apk_copy_plan *plan, int fluid, const apk_eos *eos, int64_t prim_delta,
                                    int latch_flags, apk_stream_t stream) {
  return copy_plan_run_c2p(ctx, plan, fluid, eos, prim_delta, latch_flags, true, stream);
}

int apk_kernel_timing_enable(apk_ctx *ctx, int on) {
  if (!ctx) return APK_ERR_INVALID;
  ctx->timing_on = on != 0;
  return APK_OK;
}

int apk_kernel_timing_read(apk_ctx *ctx, int slot, double *total_ms, long long *launches) {
  if (!ctx || slot < 0 || slot >= APK_T_COUNT) return APK_ERR_INVALID;
  // fold every completed span into the per-slot totals, then hand the events back
  for (auto &sp : ctx->spans) {
    float ms = 0.0f;
    hipError_t e = hipEventSynchronize(sp.stop);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, sp.start, sp.stop);
    if (e != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "apk_kernel_timing_read", e);
    ctx->timing_ms[sp.slot] += (double)ms;
    ctx->timing_n[sp.slot] += 1;
    ctx->free_events.push_back(sp.start);
    ctx->free_events.push_back(sp.stop);
  }
  ctx->spans.clear();
  if (total_ms) *total_ms = ctx->timing_ms[slot];
  if (launches) *launches = ctx->timing_n[slot];
  ctx->timing_ms[slot] = 0.0;
  ctx->timing_n[slot] = 0;
  return APK_OK;
}

}  // extern "C"
