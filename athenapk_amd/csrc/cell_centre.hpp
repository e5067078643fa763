// cell_centre.hpp -- the view of a cell that the source kernels of the cluster problem share (kernels_gravity.hip,
// kernels_feedback.hip, kernels_triggering.hip): which cell a lane owns, where its centre lies, and what an entry asks of
// its pack.
//
// Cell centres.  The centre must be the number the problem generator used on the host, xc() of host/sim_pgen.cpp:
//   x_d = xmin_d + ((g_d + i_d) + 1/2) dx_d
// with g_d the global index of the block's first interior cell and xmin_d the mesh's lower corner.  The kernels take the
// blocks' lower interior corners (and, in one more row, the mesh's) as block_xmin; cell_centre reads that layout (so does
// tower_contribs_kernel of kernels_feedback.hip, which calls centre() itself).  It rebuilds
// g_d = rint((corner_d - xmin_d) / dx_d), exact for any mesh whose index fits a double's mantissa; product and sum are
// spelled __dmul_rn / __dadd_rn so that the product build does not contract them into an FMA, which would be another
// number than the host's.  i_d may lie outside the block (-1, nx_d, or a ghost index): the centre is then the one the
// neighbouring block forms for that cell, (g + nx) + 0 = g + nx.
#pragma once

#include <cstdint>

#include "apk_internal.hpp"
#include "hydro_math.hpp"

namespace apk {

// (i, j, k) of cell `q` of an nrow x (nplane / nrow) x ... box, i fastest
APK_DEV void box_ijk(int64_t q, int64_t nrow, int64_t nplane, int &i, int &j, int &k) {
  k = (int)(q / nplane);
  const int64_t r = q - (int64_t)k * nplane;
  j = (int)(r / nrow);
  i = (int)(r - (int64_t)j * nrow);
}

// (b, i, j, k) of interior cell `idx` of the pack, indices counted from the first interior cell, and its offset in the
// block's arrays; false past the last one
APK_DEV bool cell_of(const PackView &pv, int64_t idx, int &b, int &i, int &j, int &k, int64_t &off) {
  const int64_t nrow = pv.nx1, nplane = nrow * pv.nx2, nblk = nplane * pv.nx3;
  if (idx >= nblk * pv.nblocks) return false;
  b = (int)(idx / nblk);
  box_ijk(idx - (int64_t)b * nblk, nrow, nplane, i, j, k);
  off = (pv.ks + k) * pv.sk + (pv.js + j) * pv.sj + (pv.is + i);
  return true;
}

// xc() of host/sim_pgen.cpp from the block's corner, the mesh's corner and the cell width (see the header comment)
APK_DEV double centre(double corner, double xmin, double dx, int i) {
  const double g = rint((corner - xmin) / dx);
  return __dadd_rn(xmin, __dmul_rn((g + (double)i) + 0.5, dx));
}

// The cells of block b of nblocks, bd = pv.blocks[b] its descriptor; row b of block_xmin holds the block's lower interior
// corner, row nblocks the mesh's.  Plain functions on the caller's own reference to the descriptor: the kernels that call
// them compile to the code they had with the lookup written out.
APK_DEV double cell_width(const apk_block_desc &bd, int d) { return bd.dx[d]; }
// the centre of index i of direction d, counted from the first interior cell; i may lie outside the block
APK_DEV double cell_centre(const apk_block_desc &bd, const double *block_xmin, int b, int nblocks, int d, int i) {
  return centre(block_xmin[3 * (int64_t)b + d], block_xmin[3 * (int64_t)nblocks + d], bd.dx[d], i);
}
APK_DEV void cell_xyz(const apk_block_desc &bd, const double *block_xmin, int b, int nblocks, int i, int j, int k, double &x, double &y,
                      double &z) {
  x = cell_centre(bd, block_xmin, b, nblocks, 0, i);
  y = cell_centre(bd, block_xmin, b, nblocks, 1, j);
  z = cell_centre(bd, block_xmin, b, nblocks, 2, k);
}

// What a source entry asks of its pack, checked in this order; nullptr when the pack will do.  Every pack must be hydro
// or GLM-MHD (PACK_MHD: GLM-MHD).
enum : unsigned {
  PACK_MHD = 1u,     // nine variables
  PACK_FLUID = 2u,   // `fluid` names the pack's fluid
  PACK_3D = 4u,      // three-dimensional
  PACK_STORED = 8u,  // every block has cons and prim
};
inline const char *pack_problem(const apk_pack *md, unsigned need, int fluid = APK_FLUID_EULER) {
  const PackView &v = md->view;
  if (need & PACK_MHD) {
    if (v.nhydro != 9) return "the pack is not GLM-MHD";
  } else if (v.nhydro != 5 && v.nhydro != 9) {
    return "the pack is neither hydro nor GLM-MHD";
  }
  if ((need & PACK_FLUID) && ((fluid == APK_FLUID_GLMMHD) != (v.nhydro == 9) || (fluid != APK_FLUID_EULER && fluid != APK_FLUID_GLMMHD)))
    return "fluid does not match the pack";
  if ((need & PACK_3D) && v.ndim != 3) return "the pack is not three-dimensional";
  if (need & PACK_STORED)
    for (int b = 0; b < v.nblocks; ++b)
      if (!md->h_blocks[b].prim || !md->h_blocks[b].cons) return "the pack needs cons and prim";
  return nullptr;
}
// the refusal of entry `entry`: "<entry>: <why>"
inline int pack_refused(apk_ctx *ctx, const char *entry, const char *why) {
  return set_err(ctx, APK_ERR_INVALID, (std::string(entry) + ": " + why).c_str());
}

}  // namespace apk
