// cell_centre.hpp -- what the per-cell source kernels of the cluster problem share (kernels_gravity.hip,
// kernels_feedback.hip): one lane per interior cell of the pack, and the cell centre the host's generators use.
//
// Cell centres.  The centre must be the number the problem generator used on the host, xc() of host/sim_pgen.cpp:
//   x_d = xmin_d + ((g_d + i_d) + 1/2) dx_d
// with g_d the global index of the block's first interior cell and xmin_d the mesh's lower corner.  The kernels take the
// blocks' lower interior corners (and, in one more row, the mesh's) and rebuild g_d = rint((corner_d - xmin_d) / dx_d),
// exact for any mesh whose index fits a double's mantissa; product and sum are spelled __dmul_rn / __dadd_rn so that the
// product build does not contract them into an FMA, which would be another number than the host's.  i_d may lie outside
// the block (-1, nx_d): the centre is then the one the neighbouring block forms for that cell, (g + nx) + 0 = g + nx.
#pragma once

#include <cstdint>

#include "apk_internal.hpp"
#include "hydro_math.hpp"

namespace apk {

// (b, i, j, k) of interior cell `idx` of the pack, indices counted from the first interior cell, and its offset in the
// block's arrays; false past the last one
APK_DEV bool cell_of(const PackView &pv, int64_t idx, int &b, int &i, int &j, int &k, int64_t &off) {
  const int64_t nrow = pv.nx1, nplane = nrow * pv.nx2, nblk = nplane * pv.nx3;
  if (idx >= nblk * pv.nblocks) return false;
  b = (int)(idx / nblk);
  int64_t r = idx - (int64_t)b * nblk;
  k = (int)(r / nplane);
  r -= (int64_t)k * nplane;
  j = (int)(r / nrow);
  i = (int)(r - (int64_t)j * nrow);
  off = (pv.ks + k) * pv.sk + (pv.js + j) * pv.sj + (pv.is + i);
  return true;
}

// xc() of host/sim_pgen.cpp from the block's corner, the mesh's corner and the cell width (see the header comment)
APK_DEV double centre(double corner, double xmin, double dx, int i) {
  const double g = rint((corner - xmin) / dx);
  return __dadd_rn(xmin, __dmul_rn((g + (double)i) + 0.5, dx));
}

}  // namespace apk
