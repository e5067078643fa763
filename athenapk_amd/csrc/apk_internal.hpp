// apk_internal.hpp -- internal types shared by the kernels and the C-ABI layer.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/apk_amd.h"

namespace apk {

// What a kernel sees of a MeshBlockPack: a device array of per-block descriptors plus the
// (uniform) block geometry.  Interior index bounds follow Parthenon's IndexDomain::interior
// (SURVEY.md App. A.5): [ng, ng+nx-1] in active dimensions, {0} in collapsed ones.
struct PackView {
  const apk_block_desc *blocks;  // device
  int nblocks, nvar, nhydro;
  int ng, ndim;
  int nx1, nx2, nx3;
  int ni, nj, nk;  // extents including ghosts
  int is, ie, js, je, ks, ke;
  int64_t sj, sk, sn;  // element strides of j, k and variable index
};

inline PackView make_view(const apk_pack_desc &d, const apk_block_desc *dev_blocks) {
  PackView v{};
  v.blocks = dev_blocks;
  v.nblocks = d.nblocks;
  v.nhydro = d.nhydro;
  v.nvar = d.nhydro + d.nscalars;
  v.ng = d.ng;
  v.nx1 = d.nx[0];
  v.nx2 = d.nx[1];
  v.nx3 = d.nx[2];
  v.ndim = (d.nx[2] > 1) ? 3 : ((d.nx[1] > 1) ? 2 : 1);
  v.ni = d.nx[0] + 2 * d.ng;
  v.nj = (d.nx[1] > 1) ? d.nx[1] + 2 * d.ng : 1;
  v.nk = (d.nx[2] > 1) ? d.nx[2] + 2 * d.ng : 1;
  v.is = d.ng;
  v.ie = d.ng + d.nx[0] - 1;
  v.js = (d.nx[1] > 1) ? d.ng : 0;
  v.je = (d.nx[1] > 1) ? d.ng + d.nx[1] - 1 : 0;
  v.ks = (d.nx[2] > 1) ? d.ng : 0;
  v.ke = (d.nx[2] > 1) ? d.ng + d.nx[2] - 1 : 0;
  v.sj = d.stride[0] > 0 ? d.stride[0] : v.ni;
  v.sk = d.stride[1] > 0 ? d.stride[1] : v.sj * v.nj;
  v.sn = d.stride[2] > 0 ? d.stride[2] : v.sk * v.nk;
  return v;
}

// ---- the context's scratch: 16 device words (apk_ctx::d_u64) and 256 bytes of pinned host memory (apk_ctx::h_pinned) --
// Device words.  kWordFlags follows kWordStageDt: the end-of-cycle read-back fetches both with one 16-byte copy.
enum : int {
  kWordMin = 0,       // one-shot seeded minimum of the stand-alone time-step estimators (min_seed / min_fetch)
  kWordCounter = 2,   // cells counted by FirstOrderFluxCorrect / apk_count_unphysical
  kWordStageDt = 4,   // the stage's time-step minimum (prepare_dt_word; apk_stage_dt_read / apk_stage_dt_flags_read)
  kWordFlags = 5,     // two 32-bit flag words, apk_ctx::d_flags: [0] latched, [1] trial stage
  kWordStageBad = 6,  // the fused stage's count of unphysical cells (apk_stage_unphysical_read)
  kWordMarchTickets = 7,  // piece tickets of the finishing march's dynamic phase (zeroed in stream order by launch_m12f
                          // before the launch that draws them; never read back)
  kWordPlusMax = 15,  // constant +max, the neutral element the time-step word is reset from
  kNumWords = 16
};
// Pinned block.  Its first 8 u64 slots receive device words -- slot w word w, except that the one-shot minimum comes
// back into kPinMin beside its seed --, then three regions of their own (byte offsets).
enum : int {
  kPinSeed = 0,  // u64 slot: the seed on its way to kWordMin
  kPinMin = 1,   // u64 slot: kWordMin read back
  kPinU64Slots = 8,
  kPinHistory = 64,       // 8 doubles: apk_history
  kPinSums = 128,         // kPinSumsMax doubles: the turbulence driver's sums (finish_sums)
  kPinSumsMax = 4,
  kPinPolledFlags = 192,  // one unsigned: apk_poll_device_flags
  kPinnedBytes = 256
};
static_assert(kWordFlags == kWordStageDt + 1, "time-step word and flag words are read back with one 16-byte copy");
static_assert(kWordStageBad < kWordMarchTickets && kWordMarchTickets < kWordPlusMax, "the march's ticket word is a spare one");
static_assert(kPinSeed != kPinMin && kPinMin < kWordCounter && kWordStageBad < kPinU64Slots && kWordPlusMax < kNumWords,
              "u64 slots: seed, minimum and the mirrored words are distinct");
static_assert(kPinU64Slots * 8 <= kPinHistory && kPinHistory + 8 * 8 <= kPinSums &&
                  kPinSums + kPinSumsMax * 8 <= kPinPolledFlags && kPinPolledFlags + 4 <= kPinnedBytes,
              "pinned regions are disjoint and fit the block");

}  // namespace apk

struct apk_ctx;
namespace apk {
// A device buffer of an apk_ctx that grows on demand.
template <class T>
struct DeviceBuf {
  T *p = nullptr;
  size_t cap = 0;  // in elements
  // At least n elements; grows by free + allocate of exactly n, contents are not kept.  A live buffer is freed only
  // after `s` has drained (the kernels that use these buffers run on the caller's stream); the wait is paid only when
  // a buffer grows, where hipFree waits for the device in any case.  A failure is APK_ERR_DEVICE, worded by APK_HIP_TRY.
  int reserve(apk_ctx *ctx, size_t n, hipStream_t s);
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
}  // namespace apk

struct apk_pack {
  apk::PackView view;
  apk_pack_desc desc;  // desc.blocks points into h_blocks
  std::vector<apk_block_desc> h_blocks;
  apk_block_desc *d_blocks = nullptr;
  bool have_flux[3] = {false, false, false};
};

struct apk_ctx {
  int device = -1;
  unsigned *d_flags = nullptr;       // latched APK_FLAG_* bits: the two halves of word kWordFlags
  unsigned long long *d_u64 = nullptr;  // [kNumWords] scratch words, laid out by the kWord* names above
  unsigned long long *word(int w) const { return d_u64 + w; }
  unsigned long long *min_word() const { return word(apk::kWordMin); }
  unsigned long long *counter_word() const { return word(apk::kWordCounter); }
  unsigned long long *dt_word() const { return word(apk::kWordStageDt); }
  unsigned long long *bad_count_word() const { return word(apk::kWordStageBad); }
  apk::DeviceBuf<double> d_partial;       // reduction partials
  apk::DeviceBuf<unsigned char> d_mark;   // FOFC cell marks
  void *h_pinned = nullptr;          // kPinnedBytes of pinned host staging, laid out by the kPin* names above
  unsigned long long *pinned_u64() const { return static_cast<unsigned long long *>(h_pinned); }
  double *pinned_history() const { return reinterpret_cast<double *>(static_cast<char *>(h_pinned) + apk::kPinHistory); }
  double *pinned_sums() const { return reinterpret_cast<double *>(static_cast<char *>(h_pinned) + apk::kPinSums); }
  unsigned *pinned_polled_flags() const { return reinterpret_cast<unsigned *>(static_cast<char *>(h_pinned) + apk::kPinPolledFlags); }
  // End-of-cycle gather (capi.hip: cycle_gather_kernel): ONE small kernel writes the stage's time-step word, the flag
  // words and the per-block tag criteria straight into pinned host memory and leaves the device words ready for the
  // next cycle (+max / 0) -- instead of two device-to-host copies, two fills and the next cycle's device-to-device reset
  // (5 - 7 us of stream time each; 0.9 ms cycles on refined meshes).  The *_clean flags say what the stream already
  // holds; everything that reduces into those words goes through prepare_dt_word / the tag launch, which clear them.
  unsigned long long *h_pinned_dev = nullptr;  // device address of h_pinned (null: no mapping, copies as before)
  double *h_partial_dev = nullptr;             // device address of h_partial
  apk::DeviceBuf<unsigned long long> d_tagmax;  // per-block criterion maxima of apk_tag_blocks (bit patterns), own buffer
  // the minimum apk_stage_dt_flags_read last took out of the time-step word (the read resets the word): repeated reads,
  // and a following apk_stage_dt_read, return it until the next reduction into the word starts (prepare_dt_word)
  double last_stage_min = 0.0;
  bool last_stage_min_valid = false;
  bool dt_word_clean = false;                  // the time-step word holds +max ...
  hipStream_t clean_stream = nullptr;          // ... as of the gather enqueued on this stream (another stream: reset again)
  int tag_words_clean = 0;                     // the first n words of d_tagmax hold 0
  int tags_pending = 0;                        // criteria of this many blocks reduced, not yet in h_partial
  double *h_partial = nullptr;       // pinned host mirror of d_tagmax (the per-block criteria, read back every cycle)
  size_t h_partial_cap = 0;
  apk::DeviceBuf<double> d_du;       // fused path: flux-difference accumulator
  apk::DeviceBuf<double> d_mflux;    // fused path with passive scalars: mass flux per face, [3][nblocks][sn]
  // optional kernel timing (apk_kernel_timing_*)
  bool timing_on = false;
  struct TimedSpan {
    int slot;
    hipEvent_t start, stop;
  };
  std::vector<TimedSpan> spans;       // recorded, not yet read
  std::vector<hipEvent_t> free_events;
  double timing_ms[APK_T_COUNT] = {0};
  long long timing_n[APK_T_COUNT] = {0};
  char err[512] = {0};
};

// A copy plan's work list: the regions cut into chunks of at most kCopyChunkItems (cell, variable)
// items / kCopyChunkCells cells, one workgroup per chunk -- the boxes of a plan range from 64-cell
// corners to whole faces, and a (largest box) x (regions) grid leaves most workgroups empty.
constexpr int kCopyChunkItems = 1024, kCopyChunkCells = 256;
struct apk_copy_chunk {
  int region, first;  // first item (plain copy) / first cell (ConsToPrim variant) of the chunk
};
struct apk_copy_plan {
  apk_copy_region *d_regions = nullptr;
  int n = 0;
  int64_t max_cells = 0, max_items = 0;  // largest box in cells / in cells x variables
  apk_copy_chunk *d_chunks_items = nullptr, *d_chunks_cells = nullptr;
  int nchunks_items = 0, nchunks_cells = 0;
};

namespace apk {

inline int set_err(apk_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess) {
  if (ctx) {
    if (e != hipSuccess)
      std::snprintf(ctx->err, sizeof(ctx->err), "%s: %s", what, hipGetErrorString(e));
    else
      std::snprintf(ctx->err, sizeof(ctx->err), "%s", what);
  }
  return code;
}

#define APK_HIP_TRY(ctx, expr)                                              \
  do {                                                                      \
    hipError_t e__ = (expr);                                                \
    if (e__ != hipSuccess) return apk::set_err((ctx), APK_ERR_DEVICE, #expr, e__); \
  } while (0)

template <class T>
int DeviceBuf<T>::reserve(apk_ctx *ctx, size_t n, hipStream_t s) {
  if (cap >= n) return APK_OK;
  if (p) (void)hipStreamSynchronize(s);
  release();
  APK_HIP_TRY(ctx, hipMalloc(&p, n * sizeof(T)));
  cap = n;
  return APK_OK;
}

// One-shot minimum: min_seed puts the neutral element into the word, the caller's kernel reduces into ctx->min_word(),
// min_fetch waits for it and returns the minimum.
inline int min_seed(apk_ctx *ctx, double seed, hipStream_t s) {
  unsigned long long *h = ctx->pinned_u64() + kPinSeed;
  std::memcpy(h, &seed, sizeof(seed));
  APK_HIP_TRY(ctx, hipMemcpyAsync(ctx->min_word(), h, sizeof(seed), hipMemcpyHostToDevice, s));
  return APK_OK;
}
inline int min_fetch(apk_ctx *ctx, double *m, hipStream_t s) {
  unsigned long long *h = ctx->pinned_u64() + kPinMin;
  APK_HIP_TRY(ctx, hipMemcpyAsync(h, ctx->min_word(), sizeof(*m), hipMemcpyDeviceToHost, s));
  APK_HIP_TRY(ctx, hipStreamSynchronize(s));
  std::memcpy(m, h, sizeof(*m));
  return APK_OK;
}
// A counter word (kWordCounter, kWordStageBad), zeroed before the kernel that counted in it was launched: read back.
inline int counter_fetch(apk_ctx *ctx, int w, unsigned long long *n, hipStream_t s) {
  unsigned long long *h = ctx->pinned_u64() + w;
  APK_HIP_TRY(ctx, hipMemcpyAsync(h, ctx->word(w), sizeof(*n), hipMemcpyDeviceToHost, s));
  APK_HIP_TRY(ctx, hipStreamSynchronize(s));
  *n = *h;
  return APK_OK;
}

// ---- kernel launchers implemented in the .hip translation units ---------------------
// input of the boundary-plane fluxes taken from the conserved state (flux_kernel.hpp: face_states_from_cons)
struct FluxConsInput {
  int64_t delta;  // from a block's cons array to the array holding the input state (doubles)
  apk_eos eos;
  double eos_gm1, vceil_sq, pfloor_over_gm1;
};
// flux arrays path (one TU per (fluid, riemann) family to keep compile times parallel)
int launch_fluxes_euler_hlle(const PackView &pv, int recon, double gamma, double c_h,
                             hipStream_t s, int faces = 0, const int *face_list = nullptr, int nlist = 0,
                             const FluxConsInput *from_cons = nullptr);
int launch_fluxes_euler_hllc(const PackView &pv, int recon, double gamma, double c_h,
                             hipStream_t s, int faces = 0, const int *face_list = nullptr, int nlist = 0,
                             const FluxConsInput *from_cons = nullptr);
int launch_fluxes_mhd_hlle(const PackView &pv, int recon, double gamma, double c_h,
                           hipStream_t s, int faces = 0, const int *face_list = nullptr, int nlist = 0,
                             const FluxConsInput *from_cons = nullptr);
int launch_fluxes_mhd_hlld(const PackView &pv, int recon, double gamma, double c_h,
                           hipStream_t s, int faces = 0, const int *face_list = nullptr, int nlist = 0,
                             const FluxConsInput *from_cons = nullptr);
// (dc,none) and (dc,llf = CalculateFluxesTight) for both fluids
int launch_fluxes_misc(const PackView &pv, int fluid, int riemann, double gamma, double c_h,
                       hipStream_t s);

int launch_update_flux_div(const PackView &u0, const PackView &u1, double gam0, double gam1,
                           double beta_dt, hipStream_t s);
int launch_dedner(const PackView &pv, int extended, double coeff, double beta_dt,
                  hipStream_t s);
int launch_cons_to_prim(const PackView &pv, int fluid, const apk_eos &eos, unsigned *d_flags,
                        hipStream_t s, bool ghosts_only = false, const unsigned *late_regions = nullptr,
                        int part = 0, bool faces_only = false, const int *face_nbr = nullptr,
                        unsigned long long *dt_bits = nullptr, int depth = -1, unsigned store_vars = ~0u);
int tag_from_cons_kchunks(const PackView &pv);
int launch_tag_pgrad_from_cons(const PackView &pv, int fluid, const apk_eos &eos, unsigned *d_flags, unsigned long long *dt_bits,
                               unsigned long long *block_max, const int *face_nbr, hipStream_t s);
int launch_min_dt(const PackView &pv, int fluid, double gamma, unsigned long long *d_min_bits,
                  hipStream_t s);
int launch_history(const PackView &pv, int fluid, double *d_partial, int *nblocks_out,
                   double *d_out8, hipStream_t s);
int launch_fofc_mark(const PackView &u0, const PackView &u1, int fluid, double gam0,
                     double gam1, double beta_dt, int attempt, unsigned char *d_mark,
                     unsigned long long *d_count, hipStream_t s);
int launch_count_unphysical(const PackView &u0, int fluid, unsigned long long *d_count, hipStream_t s);
// unsplit diffusion (kernels_diffusion.hip); cond: apk_conduction; spitzer: NULL for the fixed coefficient kappa, else
// the Spitzer numbers (kappa is then not read)
int launch_diff_fluxes(const PackView &pv, int cond, bool visc, bool res, double kappa, double sat_prefac, double nu,
                       double eta, const apk_spitzer_cfg *spitzer, hipStream_t s);
int launch_cond_dt(const PackView &pv, int cond, double kappa, double sat_prefac, const apk_spitzer_cfg *spitzer,
                   unsigned long long *d_min_bits, hipStream_t s);
// RKL2 super-time-stepping (kernels_sts.hip); the registers are DEVICE arrays of block descriptors of the shape of `yjm1`
int launch_flux_divergence(const PackView &pv, const apk_block_desc *out, hipStream_t s);
int launch_rkl2_step_first(const PackView &yjm1, const apk_block_desc *y0, const apk_block_desc *yjm2, const apk_block_desc *my0,
                           double mu_tilde_1, double tau, hipStream_t s);
int launch_rkl2_step_other(const PackView &yjm1, const apk_block_desc *y0, const apk_block_desc *yjm2, const apk_block_desc *my0,
                           double mu, double nu, double mu_tilde, double gamma_tilde, double tau, hipStream_t s);
int launch_rkl2_substage_fused(const PackView &yjm1, const apk_block_desc *y0, const apk_block_desc *yjm2, const apk_block_desc *my0,
                               int cond, bool visc, bool res, double kappa, double sat_prefac, double nu_visc, double eta,
                               const apk_spitzer_cfg *spitzer, double mu, double nu, double mu_tilde, double gamma_tilde,
                               double tau, bool first, hipStream_t s);
int launch_fofc_fix(const PackView &u0, int fluid, double gamma, double c_h,
                    const unsigned char *d_mark, hipStream_t s);
int launch_copy_regions(const apk_copy_plan &plan, hipStream_t s, int c2p_fluid = 0, const apk_eos *eos = nullptr,
                        unsigned *d_flags = nullptr, int64_t prim_delta = 0, bool prim_only = false);
// fused stage path (fused_dispatch.hip)
int launch_stage_fused(apk_ctx *ctx, const PackView &u0, const PackView &u1,
                       const apk_stage_args &a, double dedner_coeff, hipStream_t s, const char *&why);

// +max into the stage's time-step word (kWordStageDt) before a kernel reduces into it -- unless the stream already holds it
int prepare_dt_word(apk_ctx *ctx, hipStream_t s);
// the gather described at apk_ctx::h_pinned_dev: time-step word + flag words (+ pending tag criteria) to the host
int launch_cycle_gather(apk_ctx *ctx, hipStream_t s);

// RAII span: records start/stop events around the launches issued in its scope
struct ScopedTiming {
  apk_ctx *ctx;
  hipStream_t s;
  int idx = -1;
  ScopedTiming(apk_ctx *c, int slot, hipStream_t st) : ctx(c), s(st) {
    if (!ctx || !ctx->timing_on) return;
    auto grab = [&]() {
      hipEvent_t e = nullptr;
      if (!ctx->free_events.empty()) {
        e = ctx->free_events.back();
        ctx->free_events.pop_back();
      } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
      }
      return e;
    };
    apk_ctx::TimedSpan sp{slot, grab(), grab()};
    if (!sp.start || !sp.stop) return;
    (void)hipEventRecord(sp.start, s);
    ctx->spans.push_back(sp);
    idx = (int)ctx->spans.size() - 1;
  }
  ~ScopedTiming() {
    if (idx >= 0) (void)hipEventRecord(ctx->spans[idx].stop, s);
  }
};

// Thread -> (i, j) offset inside an ni x nj index rectangle for the (64, 4) workgroups of the
// per-cell kernels.  Rows of at least 48 cells: 64 lanes along i, 4 rows per workgroup (every load
// a full 512-B segment).  Shorter rows -- the 8^3 / 16^3 meshblocks of refined meshes -- are
// flattened row after row, so that the lanes stay busy; launch with rect_grid().
#ifdef __HIPCC__
__device__ __forceinline__ bool rect_ij(int ni, int nj, int &io, int &jo) {
  if (ni >= 48) {
    io = blockIdx.x * 64 + threadIdx.x;
    jo = blockIdx.y * 4 + threadIdx.y;
  } else {
    const int f = blockIdx.y * 256 + threadIdx.y * 64 + threadIdx.x;
    jo = f / ni;
    io = f - jo * ni;
  }
  return io < ni && jo < nj;
}
inline dim3 rect_grid(int ni, int nj, int nz) {
  return ni >= 48 ? dim3((ni + 63) / 64, (nj + 3) / 4, nz) : dim3(1, (ni * nj + 255) / 256, nz);
}
#endif

}  // namespace apk
