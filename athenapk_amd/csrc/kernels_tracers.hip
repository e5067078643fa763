// kernels_tracers.hip -- tracer particles on uniform meshes: the reference's three tasks per cycle
//   Tracers::AdvectTracers      src/tracers/tracers.cpp:189-242   Heun's method with the velocities stored on the particle
//   (swarm transport / re-own)  src/hydro/hydro_driver.cpp:615-660 periodic wrap, loss through other boundaries, new owner
//   Tracers::FillTracers        src/tracers/tracers.cpp:249-308   rho, v, p (and B) interpolated at the new position
// as three kernels (apk_tracers_advect, apk_tracers_reown, apk_tracers_fill) and as ONE (apk_tracers_step_fused): one lane
// owns one particle and does both gathers in the same launch.  All four call the same device functions, so that the two
// forms agree bit for bit in the strict (-ffp-contract=off) build.  With lookback histories a fourth task,
//   turbulence::ProblemFillTracers  src/pgen/turbulence.cpp:557-584  s = ln rho and sdot at 12 lookback levels, 26 sums
// as a kernel of its own (apk_tracers_lookback) and inside the fused step (apk_tracers_step_fused_lookback), again
// through one device function.
//
// Interpolation: trilinear on cell centres (Parthenon's interpolation::cent::linear).  Per direction, with x0 the lower
// interior face of the block and il counted from the first interior cell,
//   il = floor((x - x0) / dx - 1/2)                  the cell whose centre is <= x
//   w_lo = ((x0 + ((il + 1) + 1/2) dx) - x) / dx     w_hi = 1 - w_lo
// and the value is summed x first, then y, then z.  il is NOT clamped to the interior: a predictor position up to one
// cell outside the block reads two layers of ghost cells.  It IS clamped to the allocated extent [-ng, nx + ng - 2], which
// a particle that respects |v| dt < dx never reaches: a guard against reading outside the block's arrays, not physics.
//
// Bytes per particle and cycle (what the launch must move; the floor, not a measurement), GLM-MHD, fused form:
//   particle arrays   read x, y, z, block, active, vel_x, vel_y, vel_z = 56 B; written x, y, z, block, active + 8 fields
//                     = 96 B                                                                                   152 B
//   mesh              3 + 8 variables x 8 cells x 8 B = 704 B requested per particle, but particles sorted by (block,
//                     k-plane) share their cells: at one particle per cell every primitive of the block is read about
//                     once, 8 variables x 8 B = 64 B per particle (1/8 per cell: 512 B), the rest are L2 hits
// so 216 B per particle at one per cell (hydro: 5 fields, 40 B of mesh, 168 B).  The three-kernel form reads and writes
// x, y, z, block and active once more in each of its extra kernels: + 28 + 24 (advect) + 32 (re-own) = 84 B.
//
// Lookback histories (apk_amd/tracer_lookback; src/pgen/turbulence.cpp:513-647), the floor again and not a measurement:
//   histories         read s[12] and sdot[12] = 24 loads                                                      192 B
//                     written: level 0 and the levels that shift this cycle.  Level i >= 1 shifts when the cycle number
//                     is a multiple of 2^(i-1): on average 1 + 1/2 + 1/4 + ... ~ 2 of them, so about 3 levels x 2 arrays
//                     x 8 B                                                                                   ~48-64 B
//                     (192 B if every level were stored; a level that does not shift is read, never written)
//   partial sums      26 doubles per workgroup of 256 particles                                                 0.8 B
// so about 250 B on top of the step; the standalone kernel (the passes, and the seed-time call) reads rho and active
// again, + 12 B.  The counting sort carries all 24 values: + 192 B read and 192 B written per sort.
// The sums use no atomic: every lane forms a term (exact zeros for inactive and out-of-range lanes), the wave adds it
// with wave_sum (wg_reduce.hpp), lane 0 of the four waves leaves it in LDS, and 26 lanes add the four in wave order
// and store the workgroup's row of partials[nworkgroups][26] with ordinary vector stores;
// tracers_lookback_sum_kernel (26 workgroups, one per sum, a stride loop over the rows) adds the rows.
//
// Locality: apk_tracers_sort is a counting sort by (block, interior k-plane) -- histogram, one-workgroup scan, scatter
// through atomics on the bucket cursors (the order inside a bucket is arbitrary: no result depends on it, the accessors
// sort by id).  Inactive particles go to a bucket of their own at the end.
#include "apk_internal.hpp"
#include "hydro_math.hpp"
#include "wg_reduce.hpp"

namespace apk {

namespace {

struct TracerInterp {
  int64_t cell;      // offset of the lower cell (k0, j0, i0) in a variable's array
  double w[3][2];    // [direction][lower, upper]
};

// cell and weights of one direction (see the header comment)
APK_DEV void tracer_axis(double x, double x0, double dx, int nx, int ng, int &il, double &wlo) {
  const double t = (x - x0) / dx - 0.5;
  il = (int)floor(t);
  il = il < -ng ? -ng : (il > nx + ng - 2 ? nx + ng - 2 : il);
  wlo = ((x0 + ((double)(il + 1) + 0.5) * dx) - x) / dx;
}

APK_DEV TracerInterp tracer_locate(const PackView &pv, const apk_tracer_geom &g, int b, double x, double y, double z) {
  const double *o = g.block_origin + 3 * (int64_t)b;
  int il, jl, kl;
  TracerInterp t;
  tracer_axis(x, o[0], g.dx[0], pv.nx1, pv.ng, il, t.w[0][0]);
  tracer_axis(y, o[1], g.dx[1], pv.nx2, pv.ng, jl, t.w[1][0]);
  tracer_axis(z, o[2], g.dx[2], pv.nx3, pv.ng, kl, t.w[2][0]);
  for (int d = 0; d < 3; ++d) t.w[d][1] = 1.0 - t.w[d][0];
  t.cell = (int64_t)(pv.ks + kl) * pv.sk + (int64_t)(pv.js + jl) * pv.sj + (pv.is + il);
  return t;
}

APK_DEV double tracer_gather(const double *__restrict__ f, const TracerInterp &t, int64_t sj, int64_t sk) {
  const double *p = f + t.cell;
  const double c00 = t.w[0][0] * p[0] + t.w[0][1] * p[1];
  const double c01 = t.w[0][0] * p[sj] + t.w[0][1] * p[sj + 1];
  const double c10 = t.w[0][0] * p[sk] + t.w[0][1] * p[sk + 1];
  const double c11 = t.w[0][0] * p[sk + sj] + t.w[0][1] * p[sk + sj + 1];
  const double c0 = t.w[1][0] * c00 + t.w[1][1] * c01;
  const double c1 = t.w[1][0] * c10 + t.w[1][1] * c11;
  return t.w[2][0] * c0 + t.w[2][1] * c1;
}

// Heun: x* = x + dt v_p, v* = interp(prim, x*) in the particle's block, x += dt/2 (v_p + v*)
APK_DEV void tracer_advect(const PackView &pv, const apk_tracer_geom &g, int b, double dt, const double vp[3], double x[3]) {
  const double xs[3] = {x[0] + dt * vp[0], x[1] + dt * vp[1], x[2] + dt * vp[2]};
  const TracerInterp t = tracer_locate(pv, g, b, xs[0], xs[1], xs[2]);
  const double *__restrict__ w = pv.blocks[b].prim;
  const double hdt = 0.5 * dt;
  for (int d = 0; d < 3; ++d) {
    const double vs = tracer_gather(w + (IV1 + d) * pv.sn, t, pv.sj, pv.sk);
    x[d] = x[d] + hdt * (vp[d] + vs);
  }
}

// periodic wrap / loss, then the owner from the uniform block grid; returns false when the particle left the domain
APK_DEV bool tracer_reown(const apk_tracer_geom &g, double x[3], int &b) {
  int bc[3];
  for (int d = 0; d < 3; ++d) {
    if (x[d] < g.xmin[d]) {
      if (!g.periodic_lo[d]) return false;
      x[d] = x[d] + (g.xmax[d] - g.xmin[d]);
    } else if (x[d] >= g.xmax[d]) {
      if (!g.periodic_hi[d]) return false;
      x[d] = x[d] - (g.xmax[d] - g.xmin[d]);
    }
    int c = (int)floor((x[d] - g.xmin[d]) / g.block_size[d]);
    bc[d] = c < 0 ? 0 : (c > g.nb[d] - 1 ? g.nb[d] - 1 : c);
  }
  b = g.block_table[bc[0] + g.nb[0] * (bc[1] + g.nb[1] * bc[2])];
  return true;
}

// returns the density it stored (the lookback update of the fused step takes it from the register)
APK_DEV double tracer_fill(const PackView &pv, const apk_tracer_geom &g, const apk_tracer_arrays &a, int64_t n, int b, const double x[3]) {
  const TracerInterp t = tracer_locate(pv, g, b, x[0], x[1], x[2]);
  const double *__restrict__ w = pv.blocks[b].prim;
  // field order: rho, pressure, vel_x, vel_y, vel_z, B_x, B_y, B_z
  const double rho = tracer_gather(w + IDN * pv.sn, t, pv.sj, pv.sk);
  a.field[0][n] = rho;
  a.field[1][n] = tracer_gather(w + IPR * pv.sn, t, pv.sj, pv.sk);
  for (int d = 0; d < 3; ++d) a.field[2 + d][n] = tracer_gather(w + (IV1 + d) * pv.sn, t, pv.sj, pv.sk);
  if (a.nfields == 8)
    for (int d = 0; d < 3; ++d) a.field[5 + d][n] = tracer_gather(w + (IB1 + d) * pv.sn, t, pv.sj, pv.sk);
  return rho;
}

// ---- lookback histories (turbulence.cpp:557-584) ---------------------------------------------------------------------
constexpr int NLB = APK_TRACER_N_LOOKBACK, NSUMS = APK_TRACER_N_SUMS;

// The update of one active particle: s and sd come back holding the particle's new levels.  shift: bit idx set = level
// idx takes level idx - 1 this cycle -- a kernel argument, so the branches are scalar; a level that does not shift is
// read and not written.
APK_DEV void tracer_lookback_update(const apk_tracer_arrays &a, int64_t n, unsigned shift, double rho, double dt,
                                    double (&s)[NLB], double (&sd)[NLB]) {
  double *__restrict__ ps = a.s + n;
  double *__restrict__ pd = a.sdot + n;
  const int64_t L = a.lookback_stride;
#pragma unroll
  for (int i = 0; i < NLB; ++i) s[i] = ps[i * L], sd[i] = pd[i * L];
#pragma unroll
  for (int i = NLB - 1; i >= 1; --i)  // highest level first: a level receives the OLD value of the level below it
    if ((shift >> i) & 1u) {
      s[i] = s[i - 1], sd[i] = sd[i - 1];
      ps[i * L] = s[i], pd[i * L] = sd[i];
    }
  s[0] = log(rho);
  sd[0] = (s[0] - s[1]) / dt;
  ps[0] = s[0], pd[0] = sd[0];
}

// The workgroup's 26 partial sums of s[0] s[i], sd[0] sd[i], s[0], sd[0] into row[26]; a lane without an active particle
// passes zeros.  Every lane of the workgroup must call it.
APK_DEV void tracer_lookback_partials(const double (&s)[NLB], const double (&sd)[NLB], double *__restrict__ row) {
  __shared__ double part[4][NSUMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NSUMS; ++q) {
    const double term = q < NLB ? s[0] * s[q] : q < 2 * NLB ? sd[0] * sd[q - NLB] : q == 2 * NLB ? s[0] : sd[0];
    const double v = wave_sum(term);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < NSUMS) {
    const int q = threadIdx.x;
    // (wave order, here and in tracers_lookback_sum_kernel: not wg_sums_to_row's pairs -- the correlations keep their bits)
    row[q] = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
  }
}

// the 12-bit shift mask of a cycle number (turbulence.cpp:562-571): level idx shifts when cycle % 2^(idx-1) == 0
unsigned tracer_shift_mask(long long cycle) {
  unsigned m = 0;
  for (int idx = 1; idx < NLB; ++idx)
    if (cycle % (1ll << (idx - 1)) == 0) m |= 1u << idx;
  return m;
}

// particle of this lane: grid x, 64-bit (more particles than 65535 x 256 must survive)
APK_DEV int64_t tracer_index() { return (int64_t)blockIdx.x * 256 + threadIdx.x; }

// counters: [0] particles lost so far, [1] set when a particle changed its block or was lost (the sort is due)
APK_DEV void tracer_count(unsigned long long *counters, bool lost, bool moved) {
  if (lost) atomicAdd(&counters[0], 1ull);
  if ((lost || moved) && counters[1] == 0ull) atomicExch(&counters[1], 1ull);
}

__global__ void __launch_bounds__(256) tracers_advect_kernel(PackView pv, apk_tracer_geom g, apk_tracer_arrays a, double dt) {
  const int64_t n = tracer_index();
  if (n >= a.n || !a.active[n]) return;
  double x[3] = {a.x[n], a.y[n], a.z[n]};
  const double vp[3] = {a.field[2][n], a.field[3][n], a.field[4][n]};
  tracer_advect(pv, g, a.block[n], dt, vp, x);
  a.x[n] = x[0], a.y[n] = x[1], a.z[n] = x[2];
}

__global__ void __launch_bounds__(256) tracers_reown_kernel(apk_tracer_geom g, apk_tracer_arrays a, unsigned long long *counters) {
  const int64_t n = tracer_index();
  if (n >= a.n || !a.active[n]) return;
  double x[3] = {a.x[n], a.y[n], a.z[n]};
  const int b0 = a.block[n];
  int b = b0;
  const bool kept = tracer_reown(g, x, b);
  tracer_count(counters, !kept, b != b0);
  if (!kept) {
    a.active[n] = 0;
    return;
  }
  a.x[n] = x[0], a.y[n] = x[1], a.z[n] = x[2];
  a.block[n] = b;
}

__global__ void __launch_bounds__(256) tracers_fill_kernel(PackView pv, apk_tracer_geom g, apk_tracer_arrays a) {
  const int64_t n = tracer_index();
  if (n >= a.n || !a.active[n]) return;
  const double x[3] = {a.x[n], a.y[n], a.z[n]};
  tracer_fill(pv, g, a, n, a.block[n], x);
}

// one particle through advect, re-own and fill; false when the lane has no particle, an inactive one or one lost in this
// step; rho: the density the fill stored
APK_DEV bool tracer_step_fused(const PackView &pv, const apk_tracer_geom &g, const apk_tracer_arrays &a, double dt,
                               unsigned long long *counters, int64_t n, double &rho) {
  if (n >= a.n || !a.active[n]) return false;
  double x[3] = {a.x[n], a.y[n], a.z[n]};
  const double vp[3] = {a.field[2][n], a.field[3][n], a.field[4][n]};
  const int b0 = a.block[n];
  tracer_advect(pv, g, b0, dt, vp, x);
  int b = b0;
  const double xa[3] = {x[0], x[1], x[2]};
  const bool kept = tracer_reown(g, x, b);
  tracer_count(counters, !kept, b != b0);
  if (!kept) {  // (a lost particle keeps the position it left with, unwrapped, as the passes leave it)
    a.x[n] = xa[0], a.y[n] = xa[1], a.z[n] = xa[2];
    a.active[n] = 0;
    return false;
  }
  a.x[n] = x[0], a.y[n] = x[1], a.z[n] = x[2];
  a.block[n] = b;
  rho = tracer_fill(pv, g, a, n, b, x);
  return true;
}

// LOOKBACK: the histories' update and the workgroup's partial sums in the same launch (every lane stays to the end)
template <bool LOOKBACK>
__global__ void __launch_bounds__(256) tracers_step_fused_kernel(PackView pv, apk_tracer_geom g, apk_tracer_arrays a, double dt,
                                                                 unsigned long long *counters, unsigned shift, double *partials) {
  const int64_t n = tracer_index();
  double rho = 1.0;
  const bool live = tracer_step_fused(pv, g, a, dt, counters, n, rho);
  if constexpr (LOOKBACK) {
    double s[NLB] = {0}, sd[NLB] = {0};
    if (live) tracer_lookback_update(a, n, shift, rho, dt, s, sd);
    tracer_lookback_partials(s, sd, partials + (int64_t)blockIdx.x * NSUMS);
  }
}

// the update alone, on the rho the fill stored (the passes' fourth kernel, and the seed-time call)
__global__ void __launch_bounds__(256) tracers_lookback_kernel(apk_tracer_arrays a, double dt, unsigned shift, double *partials) {
  const int64_t n = tracer_index();
  double s[NLB] = {0}, sd[NLB] = {0};
  if (n < a.n && a.active[n]) tracer_lookback_update(a, n, shift, a.field[0][n], dt, s, sd);
  tracer_lookback_partials(s, sd, partials + (int64_t)blockIdx.x * NSUMS);
}

// sums26[q] = sum over the rows of partials[nrows][26]: workgroup q, lanes stride over the rows, then wave and LDS
__global__ void __launch_bounds__(256) tracers_lookback_sum_kernel(const double *__restrict__ partials, int64_t nrows, double *sums26) {
  __shared__ double part[4];
  const int q = blockIdx.x;
  double v = 0.0;
  for (int64_t r = threadIdx.x; r < nrows; r += 256) v += partials[r * NSUMS + q];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) sums26[q] = ((part[0] + part[1]) + part[2]) + part[3];
}

// ---- counting sort by (block, interior k-plane) ----------------------------------------------------------------------
APK_DEV int tracer_bucket(const PackView &pv, const apk_tracer_geom &g, const apk_tracer_arrays &a, int64_t n, int nbuckets) {
  if (!a.active[n]) return nbuckets - 1;
  const int b = a.block[n];
  int k = (int)floor((a.z[n] - g.block_origin[3 * (int64_t)b + 2]) / g.dx[2]);
  k = k < 0 ? 0 : (k > pv.nx3 - 1 ? pv.nx3 - 1 : k);
  return b * pv.nx3 + k;
}

__global__ void __launch_bounds__(256) tracers_hist_kernel(PackView pv, apk_tracer_geom g, apk_tracer_arrays a, int nbuckets,
                                                           unsigned long long *hist) {
  const int64_t n = tracer_index();
  if (n >= a.n) return;
  atomicAdd(&hist[tracer_bucket(pv, g, a, n, nbuckets)], 1ull);
}

// exclusive scan of the histogram in place, one workgroup (nbuckets = blocks x planes + 1: thousands)
__global__ void __launch_bounds__(256) tracers_scan_kernel(unsigned long long *hist, int nbuckets) {
  __shared__ unsigned long long part[256];
  const int t = threadIdx.x;
  const int per = (nbuckets + 255) / 256;
  const int lo = t * per, hi = lo + per < nbuckets ? lo + per : nbuckets;
  unsigned long long sum = 0;
  for (int q = lo; q < hi; ++q) sum += hist[q];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0;
    for (int q = 0; q < 256; ++q) {
      const unsigned long long v = part[q];
      part[q] = run;
      run += v;
    }
  }
  __syncthreads();
  unsigned long long run = part[t];
  for (int q = lo; q < hi; ++q) {
    const unsigned long long v = hist[q];
    hist[q] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(256) tracers_scatter_kernel(PackView pv, apk_tracer_geom g, apk_tracer_arrays a, apk_tracer_arrays out,
                                                              int nbuckets, unsigned long long *cursor) {
  const int64_t n = tracer_index();
  if (n >= a.n) return;
  const int64_t m = (int64_t)atomicAdd(&cursor[tracer_bucket(pv, g, a, n, nbuckets)], 1ull);
  if (m < 0 || m >= a.n) return;  // (cannot happen: the cursors partition [0, n))
  out.x[m] = a.x[n], out.y[m] = a.y[n], out.z[m] = a.z[n];
  out.id[m] = a.id[n];
  out.block[m] = a.block[n];
  out.active[m] = a.active[n];
  for (int f = 0; f < a.nfields; ++f) out.field[f][m] = a.field[f][n];
  if (a.s)
    for (int i = 0; i < NLB; ++i) {
      out.s[i * out.lookback_stride + m] = a.s[i * a.lookback_stride + n];
      out.sdot[i * out.lookback_stride + m] = a.sdot[i * a.lookback_stride + n];
    }
}

hipStream_t tr_stream(apk_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

int tracer_check(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *a, const apk_tracer_geom *g) {
  if (!ctx || !a || !g) return set_err(ctx, APK_ERR_INVALID, "tracers: bad argument");
  if (a->n < 0 || (a->nfields != 5 && a->nfields != 8)) return set_err(ctx, APK_ERR_INVALID, "tracers: 5 or 8 fields");
  if (a->n > 0) {
    if (!a->x || !a->y || !a->z || !a->id || !a->block || !a->active) return set_err(ctx, APK_ERR_INVALID, "tracers: null particle array");
    for (int f = 0; f < a->nfields; ++f)
      if (!a->field[f]) return set_err(ctx, APK_ERR_INVALID, "tracers: null field array");
  }
  if (a->s && (!a->sdot || a->n_lookback != NLB || a->lookback_stride < a->n))
    return set_err(ctx, APK_ERR_INVALID, "tracers: lookback histories need sdot, 12 levels and a stride >= n");
  if (!g->block_origin || !g->block_table) return set_err(ctx, APK_ERR_INVALID, "tracers: geometry without its tables");
  if (md) {
    const PackView &v = md->view;
    if (v.ndim != 3) return set_err(ctx, APK_ERR_UNSUPPORTED, "tracers: 3-D blocks only");
    if (v.ng < 2) return set_err(ctx, APK_ERR_NGHOST, "tracers: the predictor position reads two ghost layers");
    if (a->nfields == 8 && v.nhydro != 9) return set_err(ctx, APK_ERR_INVALID, "tracers: B fields need a GLM-MHD pack");
    if ((int64_t)g->nb[0] * g->nb[1] * g->nb[2] != v.nblocks) return set_err(ctx, APK_ERR_INVALID, "tracers: block grid and pack differ");
    for (const apk_block_desc &b : md->h_blocks)
      if (!b.prim) return set_err(ctx, APK_ERR_INVALID, "tracers: pack without primitives");
  }
  return APK_OK;
}

// what the lookback update reads of the arrays, and its scratch: one row of partials per workgroup of 256 particles
int lookback_check(apk_ctx *ctx, const apk_tracer_arrays *a, long long cycle, const double *partials, long long npartials_cap,
                   const double *sums26) {
  if (!ctx || !a || a->n < 0 || cycle < 0 || !sums26) return set_err(ctx, APK_ERR_INVALID, "tracers lookback: bad argument");
  if (!a->s || !a->sdot || a->n_lookback != NLB || a->lookback_stride < a->n)
    return set_err(ctx, APK_ERR_INVALID, "tracers lookback: histories need s, sdot, 12 levels and a stride >= n");
  if (a->n > 0 && (!a->active || !a->field[0])) return set_err(ctx, APK_ERR_INVALID, "tracers lookback: null particle array");
  if (a->n > 0 && (!partials || npartials_cap < (a->n + 255) / 256))
    return set_err(ctx, APK_ERR_INVALID, "tracers lookback: partials must hold a row per 256 particles");
  return APK_OK;
}

// one lane per particle, 256 per workgroup along grid x (2^31 - 1 workgroups)
bool tracer_grid(int64_t n, dim3 &grid) {
  const int64_t wg = (n + 255) / 256;
  if (wg > 2147483647ll) return false;
  grid = dim3((unsigned)wg, 1, 1);
  return true;
}

#define APK_TRACER_LAUNCH_SLOT(slot, ctx, kernel, n, stream, ...)                                       \
  do {                                                                                                  \
    dim3 grid__;                                                                                        \
    if (!tracer_grid((n), grid__)) return set_err((ctx), APK_ERR_INVALID, "tracers: too many particles"); \
    ScopedTiming span__((ctx), (slot), tr_stream(stream));                                           \
    hipLaunchKernelGGL(kernel, grid__, dim3(256, 1, 1), 0, tr_stream(stream), __VA_ARGS__);              \
    const hipError_t e__ = hipGetLastError();                                                           \
    if (e__ != hipSuccess) return set_err((ctx), APK_ERR_DEVICE, #kernel, e__);                         \
  } while (0)

#define APK_TRACER_LAUNCH(ctx, kernel, n, stream, ...) APK_TRACER_LAUNCH_SLOT(APK_T_TRACERS, ctx, kernel, n, stream, __VA_ARGS__)

}  // namespace

}  // namespace apk

using namespace apk;

extern "C" {

int apk_tracers_advect(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *a, const apk_tracer_geom *g, double dt,
                       apk_stream_t stream) {
  if (!md) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_advect: bad argument");
  const int rc = tracer_check(ctx, md, a, g);
  if (rc != APK_OK || a->n == 0) return rc;
  APK_TRACER_LAUNCH(ctx, tracers_advect_kernel, a->n, stream, md->view, *g, *a, dt);
  return APK_OK;
}

int apk_tracers_reown(apk_ctx *ctx, const apk_tracer_arrays *a, const apk_tracer_geom *g, unsigned long long *counters,
                      apk_stream_t stream) {
  const int rc = tracer_check(ctx, nullptr, a, g);
  if (rc != APK_OK) return rc;
  if (!counters) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_reown: no counters");
  if (a->n == 0) return APK_OK;
  APK_TRACER_LAUNCH(ctx, tracers_reown_kernel, a->n, stream, *g, *a, counters);
  return APK_OK;
}

int apk_tracers_fill(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *a, const apk_tracer_geom *g, apk_stream_t stream) {
  if (!md) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_fill: bad argument");
  const int rc = tracer_check(ctx, md, a, g);
  if (rc != APK_OK || a->n == 0) return rc;
  APK_TRACER_LAUNCH(ctx, tracers_fill_kernel, a->n, stream, md->view, *g, *a);
  return APK_OK;
}

int apk_tracers_step_fused(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *a, const apk_tracer_geom *g, double dt,
                           unsigned long long *counters, apk_stream_t stream) {
  if (!md) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_step_fused: bad argument");
  const int rc = tracer_check(ctx, md, a, g);
  if (rc != APK_OK) return rc;
  if (!counters) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_step_fused: no counters");
  if (a->n == 0) return APK_OK;
  APK_TRACER_LAUNCH(ctx, tracers_step_fused_kernel<false>, a->n, stream, md->view, *g, *a, dt, counters, 0u, (double *)nullptr);
  return APK_OK;
}

int apk_tracers_lookback(apk_ctx *ctx, const apk_tracer_arrays *a, long long cycle, double dt, double *partials,
                         long long npartials_cap, double *sums26, apk_stream_t stream) {
  const int rc = lookback_check(ctx, a, cycle, partials, npartials_cap, sums26);
  if (rc != APK_OK) return rc;
  if (a->n > 0) APK_TRACER_LAUNCH(ctx, tracers_lookback_kernel, a->n, stream, *a, dt, tracer_shift_mask(cycle), partials);
  APK_TRACER_LAUNCH(ctx, tracers_lookback_sum_kernel, (int64_t)256 * NSUMS, stream, partials, (a->n + 255) / 256, sums26);
  return APK_OK;
}

int apk_tracers_step_fused_lookback(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *a, const apk_tracer_geom *g,
                                    double dt, unsigned long long *counters, long long cycle, double *partials,
                                    long long npartials_cap, double *sums26, apk_stream_t stream) {
  if (!md) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_step_fused_lookback: bad argument");
  int rc = tracer_check(ctx, md, a, g);
  if (rc != APK_OK) return rc;
  if (!counters) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_step_fused_lookback: no counters");
  if ((rc = lookback_check(ctx, a, cycle, partials, npartials_cap, sums26)) != APK_OK) return rc;
  if (a->n > 0)
    APK_TRACER_LAUNCH(ctx, tracers_step_fused_kernel<true>, a->n, stream, md->view, *g, *a, dt, counters, tracer_shift_mask(cycle),
                      partials);
  APK_TRACER_LAUNCH(ctx, tracers_lookback_sum_kernel, (int64_t)256 * NSUMS, stream, partials, (a->n + 255) / 256, sums26);
  return APK_OK;
}

int apk_tracers_sort(apk_ctx *ctx, const apk_pack *md, const apk_tracer_arrays *a, const apk_tracer_arrays *out,
                     const apk_tracer_geom *g, unsigned long long *buckets, int nbuckets, apk_stream_t stream) {
  if (!md) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_sort: bad argument");
  int rc = tracer_check(ctx, md, a, g);
  if (rc != APK_OK) return rc;
  if ((rc = tracer_check(ctx, md, out, g)) != APK_OK) return rc;
  if (out->n != a->n || out->nfields != a->nfields || out->x == a->x) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_sort: the output arrays must be a second set of the same size");
  if (!buckets || nbuckets != md->view.nblocks * md->view.nx3 + 1) return set_err(ctx, APK_ERR_INVALID, "apk_tracers_sort: nbuckets must be blocks x planes + 1");
  if (a->n == 0) return APK_OK;
  {
    ScopedTiming span(ctx, APK_T_TRACER_SORT, tr_stream(stream));
    APK_HIP_TRY(ctx, hipMemsetAsync(buckets, 0, sizeof(unsigned long long) * (size_t)nbuckets, tr_stream(stream)));
  }
  APK_TRACER_LAUNCH_SLOT(APK_T_TRACER_SORT, ctx, tracers_hist_kernel, a->n, stream, md->view, *g, *a, nbuckets, buckets);
  APK_TRACER_LAUNCH_SLOT(APK_T_TRACER_SORT, ctx, tracers_scan_kernel, (int64_t)256, stream, buckets, nbuckets);
  APK_TRACER_LAUNCH_SLOT(APK_T_TRACER_SORT, ctx, tracers_scatter_kernel, a->n, stream, md->view, *g, *a, *out, nbuckets, buckets);
  return APK_OK;
}

}  // extern "C"
