// wave_ends.hpp -- diagnostic variant build (`make variant VAR=we VARFLAGS=-DAPK_M12F_WAVE_ENDS=1`): when does every
// wave of ONE launch of the three headline kernels start and end?  Empty in every other build.
//
// Every wave records four words by vector stores of lane 0 into a table nothing else reads: its start, a mark in
// between (the finishing march: the end of its whole columns; the others: its start again), its end -- ticks of the
// constant-rate wall clock (100 MHz) -- and where it ran (the hardware's id word, the XCC number above it).  The launcher
// writes the table of launch number APK_M12F_WAVE_ENDS_CALL to the file its environment variable names:
//   finishing march  APK_M12F_WAVE_ENDS_OUT      x3 sweep  APK_X3_WAVE_ENDS_OUT      donor-cell predictor  APK_DC_WAVE_ENDS_OUT
// (tools/m12f_wave_ends.py turns the tables into end-time distributions, per SIMD pair).  Switches that exist in this
// build only, so that the before / after pairs and the launch-shape sweeps come from one library:
//   APK_M12F_STATIC=1        the finishing march keeps the static leftover split
//   APK_M12F_PIECE_ROWS=n    piece length of its dynamic phase
//   APK_X3_NSEG=n            segments per column of the x3 sweep (march_segments otherwise)
//   APK_DC_KSEG=n            planes per wave of the donor-cell predictor (launch_dc_march's choice otherwise)
//   APK_WAVE_PRIORITY_OFF=m  bit 0 / 1: the finishing march / the x3 sweep set no priority (wave_priority.hpp)
#pragma once

#include "wave_priority.hpp"

#if APK_M12F_WAVE_ENDS
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace apk {

constexpr int kWaveEndsMax = 16384;
enum { WE_M12F = 0, WE_X3 = 1, WE_DC = 2 };
static __device__ unsigned long long g_wave_ends[3][4 * kWaveEndsMax];

inline int wave_ends_env(const char *name, int dflt) {
  const char *e = std::getenv(name);
  return (e && std::atoi(e) > 0) ? std::atoi(e) : dflt;
}

struct WaveEndsMark {
  unsigned long long start, mid;
};
__device__ __forceinline__ WaveEndsMark wave_ends_begin() {
  const unsigned long long t = wall_clock64();
  return {t, t};
}
__device__ __forceinline__ void wave_ends_finish(int kind, int w, const WaveEndsMark &m) {
  if (threadIdx.x == 0 && w < kWaveEndsMax) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the last row's stores have left the wave)
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID: wave 3:0, SIMD 5:4, pipe 7:6, CU 11:8, SH 12, SE 15:13
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // XCC_ID 3:0
    unsigned long long *row = g_wave_ends[kind] + 4 * (size_t)w;
    row[0] = m.start;
    row[1] = m.mid;
    row[2] = wall_clock64();
    row[3] = ((unsigned long long)(xcc & 0xfu) << 16) | (hw & 0xffffu);
  }
}

// host side, after a launch: write the table of this launcher's launch number APK_M12F_WAVE_ENDS_CALL
// (static like the table: every translation unit reads the copy its own kernels wrote)
static inline void wave_ends_dump(int kind, const char *env_out, int &calls, int nwaves, int per_xcd, const char *head, hipStream_t s) {
  static const int want = wave_ends_env("APK_M12F_WAVE_ENDS_CALL", 20);
  const char *out = std::getenv(env_out);
  if (++calls != want || !out) return;
  (void)hipStreamSynchronize(s);
  std::vector<unsigned long long> h(4 * (size_t)kWaveEndsMax);
  (void)hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_wave_ends), h.size() * sizeof(unsigned long long),
                            (size_t)kind * h.size() * sizeof(unsigned long long));
  if (FILE *f = std::fopen(out, "w")) {
    std::fprintf(f, "# %s\n", head);
    std::fprintf(f, "# wave xcd start mid end where (ticks of the 100 MHz wall clock; where = XCC << 16 | HW_ID[15:0])\n");
    for (int w = 0; w < nwaves && w < kWaveEndsMax; ++w)
      std::fprintf(f, "%d %d %llu %llu %llu %llu\n", w, per_xcd > 0 ? w / per_xcd : 0, h[4 * w], h[4 * w + 1], h[4 * w + 2], h[4 * w + 3]);
    std::fclose(f);
  }
}

}  // namespace apk
#endif
