// kernels_output.hip -- field snapshots: one fused pass from the conserved state to a dense staging buffer, and the C-ABI
// entry of include/apk_amd.h (apk_output_pack); restart: the way back for the conserved variables (apk_restart_unpack, a
// copy kernel with the same lane mapping, further down).
//
// What it replaces.  Without it a field leaves the device block by block through the accessors: ghost zones are brought up
// to date, ConsToPrim runs over every block (ghost zones included), each block is copied with its ghost zones and the host
// unpads it.  This kernel reads the interior of the conserved state once and produces every requested component in
// registers -- conserved variables as stored, primitives as ConsToPrim would give them (cons_to_prim_cell of
// hydro_math.hpp on a register copy; passive scalars r_n = s_n / rho as in kernels_block.hip), the derived fields of the
// reference's Cluster::UserWorkBeforeOutput (src/pgen/cluster.cpp:866-924), optionally rounded to float.  It needs no ghost
// zone and no stored primitive, and it never writes to the pack: a floor that fires changes the primitives that come out,
// not the state in memory, and no flag is latched.
//
// Kernel structure.  One lane per interior cell; lanes run over the DENSE interior index of the block range, i fastest,
// rows flattened one after the other (the mapping of cell_centre.hpp: cell_of), so a wave on the 16-cell rows of a 16^3
// block covers four rows and no lane idles but those past the last cell.  A 1-D grid with a grid-stride loop: no grid
// dimension grows with a row or plane count.  The loads of one variable are contiguous over the lanes of a row (row-padded
// layouts: interior rows begin on a line boundary, the padding is never touched).  The stores of one component are
// contiguous over ALL lanes -- out[block][component][cell] with cell the dense index -- so a wave stores whole 128-byte
// lines wherever a block's cell count is a multiple of 16 (double) / 32 (float), as that of every 8^3 and larger cubic
// block is; partly covered lines on the store side halve what the memory system delivers.  Which
// components are stored is uniform over the launch: the selects below compare scalars.
//
// Bytes per cell (what the launch must move): nvar * 8 read, ncomp * itemsize written.  GLM-MHD `prim` in float: 72 + 36;
// `cons` in double: 72 + 72.  Memory bound: ConsToPrim is one reciprocal and ~25 fp64 operations, the derived fields add
// three roots and four quotients.
// Measured (product build, one MI355X, device events; profiles/snapshot_cost.jsonl): on 8 x 128^3
// 0.436 ms for `prim` in float (4.16 TB/s of the 108 B; 1.26 x a device copy of the same bytes), 0.490 ms for `cons` in
// double (4.93 TB/s; 1.07 x), 0.827 ms for 21 components in double (4.87 TB/s; 1.05 x); on 512 x 16^3 0.065 / 0.069 /
// 0.116 ms.  Not measured: hydro packs, packs with passive scalars.
//
// Build forms.  The parity build (APK_FP_STRICT, -ffp-contract=off) evaluates the formulas of include/apk_amd.h with IEEE
// sqrt and /, sums left to right: it agrees with a numpy restatement bit for bit.  The product build compiles the same
// source with FMA contraction and -freciprocal-math, but without -fapprox-func (csrc/Makefile says why): its quotients and
// roots stay IEEE, so a zero field gives mach_alfven = inf and not the NaN of a refined reciprocal of zero.
#include <cmath>
#include <cstdint>

#include "apk_internal.hpp"
#include "cell_centre.hpp"
#include "hydro_math.hpp"

namespace apk {

namespace {

constexpr int kOutThreads = 256;

template <int FLUID, class T>
__global__ void __launch_bounds__(kOutThreads) output_pack_kernel(PackView pv, apk_eos eos, apk_output_desc d, int first, int nblocks,
                                                                  T *__restrict__ out) {
  constexpr int NV = nvars<FLUID>();
  constexpr bool mhd = (FLUID == APK_FLUID_GLMMHD);
  const int64_t nrow = pv.nx1, nplane = nrow * pv.nx2, nblk = nplane * pv.nx3;
  const int64_t total = nblk * nblocks, step = (int64_t)gridDim.x * kOutThreads;
  const int64_t sn = pv.sn;
  for (int64_t idx = (int64_t)blockIdx.x * kOutThreads + threadIdx.x; idx < total; idx += step) {
    const int b = (int)(idx / nblk);
    const int64_t cell = idx - (int64_t)b * nblk;
    int i, j, k;
    box_ijk(cell, nrow, nplane, i, j, k);
    const double *__restrict__ cons = pv.blocks[first + b].cons + ((pv.ks + k) * pv.sk + (pv.js + j) * pv.sj + (pv.is + i));
    double raw[NV], u[NV], w[NV], di;
#pragma unroll
    for (int n = 0; n < NV; ++n) raw[n] = u[n] = cons[n * sn];
    (void)cons_to_prim_cell<FLUID>(eos, u, w, di);  // (u takes the floors; raw is what is stored)

    // the derived fields, in the reference's operation order (cluster.cpp:870-876, 914-924)
    const double rho = w[IDN], P = w[IPR];
    const double v_mag = sqrt(w[IV1] * w[IV1] + w[IV2] * w[IV2] + w[IV3] * w[IV3]);
    const double c_s = sqrt(d.gamma * P / rho);
    const double M_s = v_mag / c_s;
    const double temperature = d.mbar_over_kb * P / rho;
    double B_mag = 0.0, M_a = 0.0, beta = 0.0;
    if constexpr (mhd) {
      const double B2 = w[IB1] * w[IB1] + w[IB2] * w[IB2] + w[IB3] * w[IB3];
      B_mag = sqrt(B2);
      const double v_A = sqrt(B2 / rho);
      M_a = M_s * c_s / v_A;
      beta = (B2 != 0) ? P / (0.5 * B2) : __builtin_nan("");
    }

    T *__restrict__ o = out + (int64_t)b * d.ncomp * nblk + cell;
    for (int c = 0; c < d.ncomp; ++c) {
      const int code = d.comp[c];  // uniform over the launch
      double v = 0.0;
      if (code >= APK_OUT_TEMPERATURE) {
        v = code == APK_OUT_TEMPERATURE   ? temperature
            : code == APK_OUT_MACH_SONIC  ? M_s
            : code == APK_OUT_B_MAG       ? B_mag
            : code == APK_OUT_MACH_ALFVEN ? M_a
                                          : beta;
      } else {
        const bool prim = code >= APK_OUT_PRIM;
        const int n = prim ? code - APK_OUT_PRIM : code;
        if (n >= NV) continue;  // passive scalars: below, one load each
#pragma unroll
        for (int m = 0; m < NV; ++m)
          if (n == m) v = prim ? w[m] : raw[m];
      }
      o[c * nblk] = static_cast<T>(v);
    }
    // passive scalars (adiabatic_hydro.hpp:139-141: r_n = s_n * (1 / rho)): each one loaded once, whoever asks for it
    for (int n = NV; n < pv.nvar; ++n) {
      bool wanted = false;
      for (int c = 0; c < d.ncomp; ++c) wanted = wanted || d.comp[c] == APK_OUT_CONS + n || d.comp[c] == APK_OUT_PRIM + n;
      if (!wanted) continue;
      const double s = cons[n * sn];
      for (int c = 0; c < d.ncomp; ++c) {
        if (d.comp[c] == APK_OUT_CONS + n) o[c * nblk] = static_cast<T>(s);
        else if (d.comp[c] == APK_OUT_PRIM + n) o[c * nblk] = static_cast<T>(s * di);
      }
    }
  }
}

template <int FLUID, class T>
void launch_output(const PackView &v, const apk_eos &eos, const apk_output_desc &d, int first, int n, void *out, hipStream_t s) {
  const int64_t total = (int64_t)v.nx1 * v.nx2 * v.nx3 * n;
  // enough workgroups to fill the device several times over, the grid-stride loop takes the rest
  const int64_t want = (total + kOutThreads - 1) / kOutThreads;
  const unsigned grid = (unsigned)(want < 16384 ? want : 16384);
  hipLaunchKernelGGL((output_pack_kernel<FLUID, T>), dim3(grid), dim3(kOutThreads), 0, s, v, eos, d, first, n, static_cast<T *>(out));
}

// The inverse of output_pack_kernel for the conserved variables (restart files): in[block][variable][cell], dense, into
// the interior of cons.  The same lane mapping -- one lane per interior cell over the dense index of the block range, i
// fastest -- with the variable loop inside the lane: the loads of one variable are contiguous over ALL lanes, the stores
// contiguous over the lanes of a row, which begins on a line boundary in row-padded layouts.  A copy: nvar * 8 bytes
// read and nvar * 8 written per cell, no arithmetic.  The variable count is uniform over the launch; all loads of a cell
// are issued before its first store (NV of them in flight per lane, the passive scalars one by one after them).
// Only interior cells are addressed: ghost zones, the row padding and prim are never written.
// Measured (product build, one MI355X, device events; profiles/restart_cost.jsonl): 0.584 ms on
// 8 x 128^3 GLM-MHD (4.14 TB/s of the 144 B per cell; 1.27 x a device copy of the same bytes), 0.099 ms on 512 x 16^3
// (1.52 x): the partly covered lines at the row ends are on the store side here.  Not measured: hydro packs, row-padded packs.
template <int NV>
__global__ void __launch_bounds__(kOutThreads) restart_unpack_kernel(PackView pv, int first, int nblocks, const double *__restrict__ in) {
  const int64_t nrow = pv.nx1, nplane = nrow * pv.nx2, nblk = nplane * pv.nx3;
  const int64_t total = nblk * nblocks, step = (int64_t)gridDim.x * kOutThreads;
  const int64_t sn = pv.sn;
  for (int64_t idx = (int64_t)blockIdx.x * kOutThreads + threadIdx.x; idx < total; idx += step) {
    const int b = (int)(idx / nblk);
    const int64_t cell = idx - (int64_t)b * nblk;
    int i, j, k;
    box_ijk(cell, nrow, nplane, i, j, k);
    double *__restrict__ cons = pv.blocks[first + b].cons + ((pv.ks + k) * pv.sk + (pv.js + j) * pv.sj + (pv.is + i));
    const double *__restrict__ src = in + (int64_t)b * pv.nvar * nblk + cell;
    double u[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) u[n] = src[n * nblk];
#pragma unroll
    for (int n = 0; n < NV; ++n) cons[n * sn] = u[n];
    for (int n = NV; n < pv.nvar; ++n) cons[n * sn] = src[n * nblk];  // passive scalars
  }
}

}  // namespace
}  // namespace apk

using namespace apk;

extern "C" {

int apk_restart_unpack(apk_ctx *ctx, const apk_pack *md, int first, int n, const double *in, apk_stream_t stream) {
  if (!ctx || !md) return set_err(ctx, APK_ERR_INVALID, "apk_restart_unpack: bad argument");
  if (const char *why = pack_problem(md, 0)) return pack_refused(ctx, "apk_restart_unpack", why);
  const PackView &v = md->view;
  if (first < 0 || n < 0 || first + n > v.nblocks) return set_err(ctx, APK_ERR_INVALID, "apk_restart_unpack: block range outside the pack");
  if (n == 0) return APK_OK;
  if (!in) return set_err(ctx, APK_ERR_INVALID, "apk_restart_unpack: in is NULL");
  for (int b = first; b < first + n; ++b)
    if (!md->h_blocks[b].cons) return set_err(ctx, APK_ERR_INVALID, "apk_restart_unpack: the pack needs cons");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = (int64_t)v.nx1 * v.nx2 * v.nx3 * n;
  const int64_t want = (total + kOutThreads - 1) / kOutThreads;
  const unsigned grid = (unsigned)(want < 16384 ? want : 16384);  // (as launch_output: the grid-stride loop takes the rest)
  if (v.nhydro == 9) hipLaunchKernelGGL((restart_unpack_kernel<9>), dim3(grid), dim3(kOutThreads), 0, s, v, first, n, in);
  else hipLaunchKernelGGL((restart_unpack_kernel<5>), dim3(grid), dim3(kOutThreads), 0, s, v, first, n, in);
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "restart unpack launch failed");
  return APK_OK;
}

int apk_output_pack(apk_ctx *ctx, const apk_pack *md, int fluid, const apk_eos *eos, const apk_output_desc *desc, int first,
                    int n, void *out, apk_stream_t stream) {
  if (!ctx || !md || !eos || !desc || !(eos->gamma > 1.0)) return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: bad argument");
  if (const char *why = pack_problem(md, PACK_FLUID, fluid)) return pack_refused(ctx, "apk_output_pack", why);
  const PackView &v = md->view;
  if (first < 0 || n < 0 || first + n > v.nblocks) return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: block range outside the pack");
  if (desc->ncomp < 1 || desc->ncomp > APK_OUT_MAX_COMPONENTS || (desc->single != 0 && desc->single != 1))
    return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: bad descriptor");
  const bool mhd = fluid == APK_FLUID_GLMMHD;
  for (int c = 0; c < desc->ncomp; ++c) {
    const int code = desc->comp[c];
    const bool var = (code >= APK_OUT_CONS && code < APK_OUT_CONS + v.nvar) || (code >= APK_OUT_PRIM && code < APK_OUT_PRIM + v.nvar);
    const bool derived = code == APK_OUT_TEMPERATURE || code == APK_OUT_MACH_SONIC;
    const bool derived_mhd = code == APK_OUT_B_MAG || code == APK_OUT_MACH_ALFVEN || code == APK_OUT_PLASMA_BETA;
    if (derived_mhd && !mhd) return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: B_mag, mach_alfven and plasma_beta need a GLM-MHD pack");
    if (!var && !derived && !derived_mhd) return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: unknown component code");
  }
  if (n == 0) return APK_OK;
  if (!out) return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: out is NULL");
  for (int b = first; b < first + n; ++b)
    if (!md->h_blocks[b].cons) return set_err(ctx, APK_ERR_INVALID, "apk_output_pack: the pack needs cons");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (mhd) {
    if (desc->single) launch_output<APK_FLUID_GLMMHD, float>(v, *eos, *desc, first, n, out, s);
    else launch_output<APK_FLUID_GLMMHD, double>(v, *eos, *desc, first, n, out, s);
  } else {
    if (desc->single) launch_output<APK_FLUID_EULER, float>(v, *eos, *desc, first, n, out, s);
    else launch_output<APK_FLUID_EULER, double>(v, *eos, *desc, first, n, out, s);
  }
  if (hipGetLastError() != hipSuccess) return set_err(ctx, APK_ERR_DEVICE, "output pack launch failed");
  return APK_OK;
}

}  // extern "C"
