// block_sum.hpp -- the deterministic sum over the cells of an entry (a box of a block): the AGN triggering reductions
// (kernels_triggering.hip).
//
// The grid is (P, entries): P = block_sum_groups(cells) workgroups of 256 lanes per entry, each over a fixed contiguous
// share of the entry's cells, a whole number of 256-cell rounds (block_sum_share).  The order of every addition is fixed:
//   1. a lane adds the terms of its cells first + lane, first + lane + 256, ... in that order (the caller's loop);
//   2. the workgroup halves its 256 lane sums through LDS, 128 -> 1: lane l adds lane l + s to itself (block_sum_store);
//   3. a second small kernel adds the entry's P partials in order, p = 0 first (block_sum_final_by_box).
// No atomics: an entry's sums are a function of its cells alone, whatever else the launch holds.  The restatement is
// block_sum of tests/triggering_reference.py.
#pragma once

#include <cstdint>

#include "apk_internal.hpp"
#include "hydro_math.hpp"

namespace apk {

constexpr int kBlockSumCellsPerGroup = 4096, kBlockSumMaxGroups = 64;

// P: one workgroup per 4096 cells of the largest entry, at most 64
inline int block_sum_groups(int64_t ncell) {
  const int64_t p = (ncell + kBlockSumCellsPerGroup - 1) / kBlockSumCellsPerGroup;
  return (int)(p < 1 ? 1 : (p > kBlockSumMaxGroups ? kBlockSumMaxGroups : p));
}

// the share [first, last) of workgroup p of P of an entry's ncell cells: a whole number of 256-cell rounds, the same for
// every workgroup of the entry
APK_DEV void block_sum_share(int64_t ncell, int p, int P, int64_t &first, int64_t &last) {
  const int64_t share = ((ncell + P - 1) / P + 255) / 256 * 256;
  first = (int64_t)p * share;
  last = (first + share < ncell) ? first + share : ncell;
}

// the workgroup's first NS lane sums through the LDS tree into partial[(e * P + p) * NSLOT + n], the slots past them
// cleared; every lane of the workgroup calls
template <int NS, int NSLOT>
APK_DEV void block_sum_store(double (&red)[NSLOT][256], const double (&acc)[NSLOT], int e, int p, int P, double *__restrict__ partial) {
#pragma unroll
  for (int n = 0; n < NS; ++n) red[n][threadIdx.x] = acc[n];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int n = 0; n < NS; ++n) red[n][threadIdx.x] += red[n][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int n = 0; n < NSLOT; ++n) partial[((int64_t)e * P + p) * NSLOT + n] = n < NS ? red[n][0] : 0.0;
  }
}

namespace {  // (a kernel of its own in each translation unit that includes this: they are built with different flags)

// the P partials of every entry, added in order: one lane per (entry, slot).  The entry's sums go to the block boxes[e]
// names, out[NSLOT * block + n]; an entry whose block is none of the nblocks is dropped.  NSLOT is a power of two.
template <int NSLOT>
__global__ void __launch_bounds__(64) block_sum_final_by_box_kernel(const double *__restrict__ partial, int P, int nentries, int nblocks,
                                                                    const apk_trig_box *__restrict__ boxes, double *__restrict__ out) {
  static_assert(NSLOT > 0 && (NSLOT & (NSLOT - 1)) == 0, "a power of two");
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= NSLOT * nentries) return;
  const int e = q >> __builtin_ctz(NSLOT), n = q & (NSLOT - 1);
  const int b = boxes[e].block;
  if (b < 0 || b >= nblocks) return;
  double sum = 0.0;
  for (int p = 0; p < P; ++p) sum += partial[((int64_t)e * P + p) * NSLOT + n];
  out[NSLOT * (int64_t)b + n] = sum;
}

}  // namespace

// launch it (the caller checks hipGetLastError)
template <int NSLOT>
inline void block_sum_final_by_box(const double *partial, int P, int nentries, int nblocks, const apk_trig_box *boxes, double *out,
                                   hipStream_t s) {
  hipLaunchKernelGGL(block_sum_final_by_box_kernel<NSLOT>, dim3((unsigned)((NSLOT * nentries + 63) / 64)), dim3(64), 0, s,
                     partial, P, nentries, nblocks, boxes, out);
}

}  // namespace apk
