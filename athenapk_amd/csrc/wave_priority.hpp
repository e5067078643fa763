// wave_priority.hpp -- a march wave's issue priority follows the share of its march it still has in front of it.
//
// The stage marches run two waves per SIMD (242 - 256 VGPRs, an 18.4 KB LDS ring), and the SIMD arbitrates VALU issue
// between the two by priority, then by age: with both at priority 0 the wave dispatched first runs nearly unimpeded and
// its partner gets the slots that are left, so the partners of a pair end a third of a launch apart and the SIMD spends
// that third with one wave (profiles/m12f_wave_ends_before.json).  A wave that sets its priority from the
// work it has LEFT hands the slots to whichever partner is behind: no work moves, no wave waits for another, nothing is
// read or written -- the scalar s_setprio, at most four times per march.  The scale is geometric (halves of the
// remaining share), so the lag two partners can keep to the very end is an eighth of a march.
// Used by the x3 sweep and the finishing march of the two-kernel stage (fused_march_kernel<.., 3, false>,
// fused_m12f_kernel: -4 % and -3.5 %, occupied share of the wave slots 85 -> 93 % and 90 -> 95.5 %); measured without
// effect in the donor-cell predictor, which does not set it.
#pragma once

#include <hip/hip_runtime.h>

#ifndef APK_WAVE_PRIORITY
// 0 (diagnostic builds only): no march sets a priority -- the schedule before DESIGN 7.R8.
#define APK_WAVE_PRIORITY 1
#endif
#ifndef APK_M12F_WAVE_ENDS
// 1: the diagnostic variant build of fused2_kernel.hpp / wave_ends.hpp
#define APK_M12F_WAVE_ENDS 0
#endif

namespace apk {

// priority of a wave with `remaining` of the `total` steps of its march still to do:
// 3 above a half, 2 above a quarter, 1 above an eighth, 0 below (and always 0 with nothing left)
constexpr int wave_priority_level(int remaining, int total) {
  return 2 * (long long)remaining > total ? 3 : (4 * (long long)remaining > total ? 2 : (8 * (long long)remaining > total ? 1 : 0));
}

constexpr bool wave_priority_scale_holds(int total) {
  if (wave_priority_level(0, total) != 0 || wave_priority_level(total, total) != 3) return false;
  for (int r = total; r > 0; --r)
    if (wave_priority_level(r - 1, total) > wave_priority_level(r, total)) return false;  // (never rises as the work shrinks)
  return true;
}
static_assert(wave_priority_scale_holds(1) && wave_priority_scale_holds(2) && wave_priority_scale_holds(3) &&
              wave_priority_scale_holds(7) && wave_priority_scale_holds(8) && wave_priority_scale_holds(16) &&
              wave_priority_scale_holds(64) && wave_priority_scale_holds(128), "priority scale");
static_assert(wave_priority_level(65, 128) == 3 && wave_priority_level(64, 128) == 2 && wave_priority_level(33, 128) == 2 &&
              wave_priority_level(32, 128) == 1 && wave_priority_level(17, 128) == 1 && wave_priority_level(16, 128) == 0,
              "thresholds at a half, a quarter and an eighth");
static_assert(wave_priority_level(1, 7) == 1 && wave_priority_level(1, 8) == 0 && wave_priority_level(1, 3) == 2 &&
              wave_priority_level(1, 2) == 2 && wave_priority_level(1, 1) == 3, "short marches");

// The priority a wave last set.  Levels are computed from wave-uniform values (loop counters through v_readfirstlane):
// s_setprio is a scalar instruction that ignores the execution mask, so a condition the compiler takes for divergent
// would lower to an unconditional s_setprio; a uniform one lowers to s_cmp / s_cbranch_scc around it.
struct WavePriority {
  int level = 0;
#if APK_M12F_WAVE_ENDS
  bool off = false;  // (variant build: StageParams.prio_off, so that before and after come from one library)
#endif

  __device__ __forceinline__ void set(int lv) {
#if APK_WAVE_PRIORITY
#if APK_M12F_WAVE_ENDS
    if (off) return;
#endif
    if (lv == level) return;
    switch (lv) {  // (the instruction takes a literal)
      case 3: __builtin_amdgcn_s_setprio(3); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      default: __builtin_amdgcn_s_setprio(0); break;
    }
    level = lv;
#else
    (void)lv;
#endif
  }
  // at the top of a step of the march: `remaining` steps follow this one, of `total`
  __device__ __forceinline__ void step(int remaining, int total) {
    set(wave_priority_level(__builtin_amdgcn_readfirstlane(remaining), __builtin_amdgcn_readfirstlane(total)));
  }
  // the march's loop has ended
  __device__ __forceinline__ void done() { set(0); }
};

}  // namespace apk
