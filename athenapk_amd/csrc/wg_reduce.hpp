// wg_reduce.hpp -- a value of every lane reduced over a workgroup of 256 lanes: the minimum (time-step estimates), the
// maximum (refinement tags) and sums (history, turbulence) of the streaming kernels.
//
// One shape throughout: a __shfl_down tree over the 64 lanes of a wave, lane 0 of the four waves leaves its result in
// LDS, one lane combines the four and issues the atomic or the store.  Both launch shapes of the callers work, (64, 4, 1)
// and flat 256: the wave of a lane is (threadIdx.y * 64 + threadIdx.x) >> 6.  Every lane of the workgroup calls, and a
// kernel calls each function once (its four LDS words are not fenced against a second round).
//
// Order of additions (the contract of the sums; tests/helpers.py restates it,
// test_gpu_parity.py::test_history_sums_in_the_stated_order holds history_kernel to it bit for bit and
// test_gpu_turbulence_shapes.py the turbulence sums and the user history of kernels_turb.hip):
//   1. wave_sum: lane l adds lane l + off to itself, off = 32, 16, 8, 4, 2, 1;
//   2. wg_sums_to_row: (w0 + w1) + (w2 + w3) over the four waves' results;
//   2a. mid_sum_kernel (kernels_turb.hip; only where a launch leaves more than 2048 rows): with chunk = ceil(rows / 256),
//      workgroup g of 256 owns the rows [g * chunk, min((g + 1) * chunk, rows)); its thread t of 256 adds the rows
//      lo + t, lo + t + 256, ... to 0.0 in that order, then steps 1 and 2 over the 256 threads.  A workgroup whose share
//      is empty leaves 0.0, and step 3 runs over these 256 rows instead;
//   3. final_sum_kernel: lane l of 32 adds the rows l, l + 32, l + 64, ... to 0.0 in that order, then the same tree at
//      width 32, off = 16 .. 1.
// Minima and maxima do not depend on an order.
//
// Not included by the fused marches (fused*_kernel.hpp), which keep their inline trees and one atomic per wave: the
// benchmark times them, and a helper with the same body re-rolls their register allocation.  block_sum.hpp (a fixed
// LDS tree over cells of a box) and the tracers' LDS combine, ((w0 + w1) + w2) + w3, are orders of their own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace apk {

// the trees: the result is valid in lane 0
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The workgroup's minimum into *word (positive doubles order like their bit patterns): one candidate per workgroup, and
// an atomic only if it beats the word's current value.  The word only ever decreases, so a stale read is larger and
// merely costs an atomic that changes nothing; fmin drops a NaN before the compare.  Tens of thousands of workgroups
// would otherwise queue on one address for milliseconds.
__device__ __forceinline__ void wg_min_to_word(double lane_min, unsigned long long *word) {
  __shared__ double wmin[4];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const double m = wave_min(lane_min);
  if ((tid & 63) == 0) wmin[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    const double g = fmin(fmin(wmin[0], wmin[1]), fmin(wmin[2], wmin[3]));
    const double cur = __longlong_as_double((long long)__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (g < cur) atomicMin(word, (unsigned long long)__double_as_longlong(g));
  }
}

// The workgroup's maximum (of non-negative values) into *word, always by the atomic; store: uniform over the workgroup,
// false leaves the word alone.
__device__ __forceinline__ void wg_max_to_word(double lane_max, unsigned long long *word, bool store) {
  __shared__ double wmax[4];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const double m = wave_max(lane_max);
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0 && store) {
    const double g = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    atomicMax(word, (unsigned long long)__double_as_longlong(g));
  }
}

// this workgroup's place in its grid: its row of a [workgroups][NQ] array of partials
__device__ __forceinline__ int64_t wg_index() { return (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// NQ sums of the workgroup into row[NQ], in the order stated above
template <int NQ>
__device__ __forceinline__ void wg_sums_to_row(const double (&h)[NQ], double *row) {
  __shared__ double part[4][NQ];
  const int tid = threadIdx.y * 64 + threadIdx.x;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double s = wave_sum(h[q]);
    if ((tid & 63) == 0) part[tid >> 6][q] = s;
  }
  __syncthreads();
  if (tid < NQ) row[tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

namespace {  // (a kernel of its own in each translation unit that launches it)

// out[q] = the sum over the rows of partial[nwg][NQ]: NQ <= 8 quantities x 32 lanes each, in the order stated above --
// the same from run to run
template <int NQ>
__global__ void __launch_bounds__(256) final_sum_kernel(const double *partial, int nwg, double *out) {
  const int q = threadIdx.x / 32, lane = threadIdx.x % 32;
  if (q >= NQ) return;
  double s = 0.0;
  for (int w = lane; w < nwg; w += 32) s += partial[(int64_t)w * NQ + q];
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) s += __shfl_down(s, off, 32);
  if (lane == 0) out[q] = s;
}

}  // namespace

}  // namespace apk
