// flux_div.hpp -- Parthenon Update::FluxDivHelper (un-vendored) as the per-cell kernels use it:
// UpdateWithFluxDivergence (kernels_block.hip) and FluxDivergence / RKL2StepOther (kernels_sts.hip).  One definition,
// so that the term order cannot drift between them.
#pragma once

#include "apk_internal.hpp"
#include "hydro_math.hpp"

namespace apk {

// du = A1 F1(i+1) - A1 F1(i) [+ A2 ..][+ A3 ..];  return -du / V
APK_DEV double flux_div(const PackView &pv, const apk_block_desc &blk, int64_t idx,
                        const double (&area)[3], double vol) {
  const double *f1 = blk.flux[0] + idx;
  double du = (area[0] * f1[1] - area[0] * f1[0]);
  if (pv.ndim >= 2) {
    const double *f2 = blk.flux[1] + idx;
    du += (area[1] * f2[pv.sj] - area[1] * f2[0]);
  }
  if (pv.ndim == 3) {
    const double *f3 = blk.flux[2] + idx;
    du += (area[2] * f3[pv.sk] - area[2] * f3[0]);
  }
  return -du / vol;
}

APK_DEV void block_areas(const apk_block_desc &blk, double (&area)[3], double &vol) {
  area[0] = blk.dx[1] * blk.dx[2];
  area[1] = blk.dx[0] * blk.dx[2];
  area[2] = blk.dx[0] * blk.dx[1];
  vol = blk.dx[0] * blk.dx[1] * blk.dx[2];
}

}  // namespace apk
