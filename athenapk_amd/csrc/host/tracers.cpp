// tracers.cpp -- tracer particles above the hot-path boundary: the <tracers> options and what is refused
// (src/tracers/tracers.cpp:43-93), seeding (tracers.cpp:95-186), the tracer step after the last stage of a cycle
// (src/hydro/hydro_driver.cpp:615-660) and the accessors.  One rank, uniform meshes; the kernels are
// csrc/kernels_tracers.hip.
//
// Storage: ONE rank-wide structure of arrays (the reference keeps a swarm per block) -- x, y, z, id, fields, block,
// active -- in a single allocation from the driver's allocator, twice: the counting sort by (block, k-plane) that keeps
// the gathers of a wave in few cache lines writes from one set into the other.
//
// Seeding deviates from the reference, which draws from Kokkos' RNG pool: random_per_block evaluates a stateless
// counter-based generator on the host, r(gid, n, c) = splitmix64 chained over (initial_rng_seed + gid, n, c), top 53 bits,
// and places particle n of block gid at origin + r * block size.  Positions depend on neither the distribution of blocks
// nor a launch shape; ids are the reference's, n_per_block * gid + n.
//
// Lookback histories (apk_amd/tracer_lookback; src/pgen/turbulence.cpp:200-216, 513-647): s and sdot, [12][cap] each,
// behind the arrays of each set, allocated only with the switch on (96 B per particle without, 288 B with, GLM-MHD).
// The host keeps t_lookback[12] and the last row; the 26 sums come back with the two counters in one copy.
#include "sim_internal.hpp"

#include <fstream>

namespace apk {
namespace host {

namespace {

uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double tracer_uniform(uint64_t key, uint64_t n, uint64_t c) {
  const uint64_t u = splitmix64(splitmix64(splitmix64(key) ^ n) ^ c);
  return (double)(u >> 11) * (1.0 / 9007199254740992.0);
}

constexpr int kLookback = APK_TRACER_N_LOOKBACK, kSums = APK_TRACER_N_SUMS;

size_t bytes_per_particle(const TracerState &t) {
  return sizeof(double) * (3 + t.nfields) + sizeof(int64_t) + 2 * sizeof(int32_t) + (t.lookback ? sizeof(double) * 2 * kLookback : 0);
}

// the arrays of set `which` for n particles (layout: x | y | z | id | fields | block | active, each cap long, then
// with lookbacks s | sdot, each [12][cap])
apk_tracer_arrays arrays_of(const TracerState &t, int which, int64_t n) {
  apk_tracer_arrays a{};
  a.n = n;
  a.nfields = t.nfields;
  double *p = t.set[which];
  if (!p) return a;
  a.x = p;
  a.y = p + t.cap;
  a.z = p + 2 * t.cap;
  a.id = reinterpret_cast<int64_t *>(p + 3 * t.cap);
  for (int f = 0; f < t.nfields; ++f) a.field[f] = p + (4 + f) * t.cap;
  a.block = reinterpret_cast<int32_t *>(p + (4 + t.nfields) * t.cap);
  a.active = a.block + t.cap;
  if (t.lookback) {
    a.s = p + (5 + t.nfields) * t.cap;
    a.sdot = a.s + kLookback * t.cap;
    a.lookback_stride = t.cap;
    a.n_lookback = kLookback;
  }
  return a;
}

// room for `want` particles in both sets; what set `cur` holds survives
int reserve(apk_sim *s, int64_t want) {
  TracerState &t = *s->tracers;
  if (want <= t.cap) return APK_OK;
  const int64_t cap = (std::max(want, t.cap + t.cap / 2) + 1) / 2 * 2;  // (even: the int32 arrays end on 8 bytes)
  TracerState old;  // (pointers and sizes only: what arrays_of reads)
  old.nfields = t.nfields, old.n = t.n, old.cap = t.cap, old.cur = t.cur, old.set[0] = t.set[0], old.set[1] = t.set[1];
  old.lookback = t.lookback;
  double *fresh[2] = {nullptr, nullptr};
  SIM_TRY(s, dev_alloc(s, "tracers", bytes_per_particle(t) * (size_t)cap, &fresh[0]));
  const int rc = dev_alloc(s, "tracers_sorted", bytes_per_particle(t) * (size_t)cap, &fresh[1]);
  if (rc != APK_OK) {
    dev_free(s, fresh[0]);
    return rc;
  }
  if (t.lookback) {  // a row of partial sums per workgroup of 256 particles (no kernel is in flight: see the sync below)
    SIM_HIP(s, hipStreamSynchronize(hs(s)));
    dev_free(s, t.d_partials);
    t.d_partials = nullptr;
    t.partials_cap = (cap + 255) / 256;
    SIM_TRY(s, dev_alloc(s, "tracer_lookback_partials", sizeof(double) * kSums * (size_t)t.partials_cap, &t.d_partials));
  }
  t.cap = cap;
  t.set[0] = fresh[0], t.set[1] = fresh[1];
  t.cur = 0;
  if (old.n > 0) {
    const apk_tracer_arrays from = arrays_of(old, old.cur, old.n), to = arrays_of(t, 0, old.n);
    const size_t nd = sizeof(double) * (size_t)old.n;
    // (on the sim's stream, whatever kind it is, and complete before the old sets go back to the allocator)
    const hipStream_t st = hs(s);
    SIM_HIP(s, hipMemcpyAsync(to.x, from.x, nd, hipMemcpyDeviceToDevice, st));
    SIM_HIP(s, hipMemcpyAsync(to.y, from.y, nd, hipMemcpyDeviceToDevice, st));
    SIM_HIP(s, hipMemcpyAsync(to.z, from.z, nd, hipMemcpyDeviceToDevice, st));
    SIM_HIP(s, hipMemcpyAsync(to.id, from.id, nd, hipMemcpyDeviceToDevice, st));
    for (int f = 0; f < t.nfields; ++f) SIM_HIP(s, hipMemcpyAsync(to.field[f], from.field[f], nd, hipMemcpyDeviceToDevice, st));
    SIM_HIP(s, hipMemcpyAsync(to.block, from.block, nd / 2, hipMemcpyDeviceToDevice, st));
    SIM_HIP(s, hipMemcpyAsync(to.active, from.active, nd / 2, hipMemcpyDeviceToDevice, st));
    for (int i = 0; t.lookback && i < kLookback; ++i) {
      SIM_HIP(s, hipMemcpyAsync(to.s + i * to.lookback_stride, from.s + i * from.lookback_stride, nd, hipMemcpyDeviceToDevice, st));
      SIM_HIP(s, hipMemcpyAsync(to.sdot + i * to.lookback_stride, from.sdot + i * from.lookback_stride, nd, hipMemcpyDeviceToDevice, st));
    }
  }
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  dev_free(s, old.set[0]);
  dev_free(s, old.set[1]);
  return APK_OK;
}

// owner of a position inside the domain: the kernels' arithmetic (tracer_reown)
int owner_of(const apk_sim *s, const double x[3]) {
  const Mesh &m = s->mesh;
  int bc[3];
  for (int d = 0; d < 3; ++d) {
    const int c = (int)std::floor((x[d] - s->xmin[d]) / ((double)m.mb[d] * s->dx[d]));
    bc[d] = std::min(std::max(c, 0), m.nb[d] - 1);
  }
  return m.gid_local.at(m.Gid(bc));
}

// append particles to the device arrays (ids given), active, fields zero until the fill, histories empty (zero)
int append(apk_sim *s, const double *x, const double *y, const double *z, const int64_t *id, const int32_t *block, int64_t n) {
  TracerState &t = *s->tracers;
  if (n <= 0) return APK_OK;
  SIM_TRY(s, reserve(s, t.n + n));
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n + n);
  const size_t nd = sizeof(double) * (size_t)n;
  // (on the sim's stream; the host arrays are the caller's: complete before returning)
  const hipStream_t st = hs(s);
  const std::vector<int32_t> ones((size_t)n, 1);
  SIM_HIP(s, hipMemcpyAsync(a.x + t.n, x, nd, hipMemcpyHostToDevice, st));
  SIM_HIP(s, hipMemcpyAsync(a.y + t.n, y, nd, hipMemcpyHostToDevice, st));
  SIM_HIP(s, hipMemcpyAsync(a.z + t.n, z, nd, hipMemcpyHostToDevice, st));
  SIM_HIP(s, hipMemcpyAsync(a.id + t.n, id, nd, hipMemcpyHostToDevice, st));
  SIM_HIP(s, hipMemcpyAsync(a.block + t.n, block, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
  SIM_HIP(s, hipMemcpyAsync(a.active + t.n, ones.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
  for (int f = 0; f < t.nfields; ++f) SIM_HIP(s, hipMemsetAsync(a.field[f] + t.n, 0, nd, st));
  for (int i = 0; t.lookback && i < kLookback; ++i) {
    SIM_HIP(s, hipMemsetAsync(a.s + i * a.lookback_stride + t.n, 0, nd, st));
    SIM_HIP(s, hipMemsetAsync(a.sdot + i * a.lookback_stride + t.n, 0, nd, st));
  }
  SIM_HIP(s, hipStreamSynchronize(st));
  t.n += n;
  return APK_OK;
}

// counting sort by (block, k-plane) from the current set into the other one; the roles swap
int sort_particles(apk_sim *s) {
  TracerState &t = *s->tracers;
  if (t.n == 0) return APK_OK;
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n), out = arrays_of(t, 1 - t.cur, t.n);
  SIM_TRY(s, apk_tracers_sort(s->ctx, s->mu0(), &a, &out, &t.geom, reinterpret_cast<unsigned long long *>(t.d_buckets), t.nbuckets, s->stream));
  t.cur = 1 - t.cur;
  t.sorts += 1;
  return APK_OK;
}

// The stored primitives of the current state with every ghost zone complete, for the duration of a gather: the driver's
// own completion path (what the accessors use).  On scope exit a cycle that stored no primitives is told again that it has
// none to rely on: the next first stage then derives its input from the conserved state exactly as it does without
// tracers.  (It could read the primitives just stored instead -- the same numbers in the strict build, but in the product
// build the ConsToPrim kernel and the stage's in-register conversion contract differently, and the last-bit differences
// would make the tracers act on the flow.)  prim_stale = true errs on the safe side: whoever needs stored primitives
// converts again; the ghost-zone flags stay as the completion left them, i.e. complete.
struct CompletedState {
  apk_sim *s;
  bool was_stale;
  explicit CompletedState(apk_sim *sim) : s(sim), was_stale(sim->prim_stale) {}
  int complete() { return sync_ghosts(s); }
  ~CompletedState() {
    if (was_stale) s->prim_stale = true;
  }
};

int fill_particles(apk_sim *s) {
  TracerState &t = *s->tracers;
  if (t.n == 0) return APK_OK;
  CompletedState state(s);
  SIM_TRY(s, state.complete());
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n);
  return apk_tracers_fill(s->ctx, s->mu0(), &a, &t.geom, s->stream);
}

// the two counters and, with lookbacks, the 26 sums behind them: one copy, one synchronisation
int read_counters(apk_sim *s, unsigned long long out[2 + kSums]) {
  const size_t words = s->tracers->lookback ? 2 + kSums : 2;
  SIM_HIP(s, hipMemcpyAsync(out, s->tracers->d_counters, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, hs(s)));
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  return APK_OK;
}

double *lookback_sums(const TracerState &t) { return t.d_counters + 2; }

// The host's part of ProblemFillTracers for the update that ran with cycle number c at time `time`
// (turbulence.cpp:523-534, 603-641): the t_lookback cascade, highest level first, the means, and the row of the file
int lookback_row(apk_sim *s, long long c, double time, const unsigned long long words[2 + kSums]) {
  TracerState &t = *s->tracers;
  for (int idx = kLookback - 1; idx >= 1; --idx)
    if (c % (1ll << (idx - 1)) == 0) t.t_lookback[idx] = t.t_lookback[idx - 1];
  t.t_lookback[0] = time;
  double sums[kSums];
  std::memcpy(sums, words + 2, sizeof sums);
  t.row_cycle = c;
  t.row_time = time;
  t.row_active = (long long)t.n - t.lost;
  const double n_active = (double)t.row_active;
  t.row[0] = sums[2 * kLookback] / n_active;
  t.row[1] = sums[2 * kLookback + 1] / n_active;
  for (int q = 0; q < 2 * kLookback; ++q) t.row[2 + q] = sums[q] / n_active;
  return APK_OK;
}

// <outdir>/correlations.csv: truncated with its header (one line; the reference's is broken over three by a misplaced
// endl, turbulence.cpp:617-622), then a row per cycle that round-trips (the reference prints six digits)
int lookback_csv(apk_sim *s, bool header) {
  const TracerState &t = *s->tracers;
  if (t.csv_path.empty() || s->rank != 0) return APK_OK;
  FILE *f = std::fopen(t.csv_path.c_str(), header ? "w" : "a");
  if (!f) return fail(s, APK_ERR_INVALID, "cannot write " + t.csv_path);
  if (header) {
    std::fprintf(f, "# cycle,time,s,sdot");
    for (const char *var : {"corr_s", "corr_sdot", "t_lookback"})
      for (int i = 0; i < kLookback; ++i) std::fprintf(f, ",%s[%d]", var, i);
  } else {
    std::fprintf(f, "%lld,%.17g", t.row_cycle, t.row_time);
    for (double v : t.row) std::fprintf(f, ",%.17g", v);
    for (double v : t.t_lookback) std::fprintf(f, ",%.17g", v);
  }
  std::fprintf(f, "\n");
  std::fclose(f);
  return APK_OK;
}

// NumPy .npy, format 1.0 (little endian, C order, one dimension)
bool write_npy(const std::string &path, const char *descr, const void *data, size_t n, size_t item) {
  std::string h = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" + std::to_string(n) + ",), }";
  while ((10 + h.size() + 1) % 64 != 0) h += ' ';
  h += '\n';
  std::ofstream f(path, std::ios::binary);
  if (!f) return false;
  const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
  const unsigned char len[2] = {(unsigned char)(h.size() & 0xff), (unsigned char)(h.size() >> 8)};
  f.write(reinterpret_cast<const char *>(magic), 8);
  f.write(reinterpret_cast<const char *>(len), 2);
  f.write(h.data(), (std::streamsize)h.size());
  f.write(static_cast<const char *>(data), (std::streamsize)(n * item));
  return (bool)f;
}

const char *kFieldNames[8] = {"rho", "pressure", "vel_x", "vel_y", "vel_z", "B_x", "B_y", "B_z"};

}  // namespace

void tracers_initialize(apk_sim *s) {
  ParameterInput &pin = s->pin;
  // apk_amd/tracer_lookback: opt-in, with any problem generator (the reference: always, for problem_id = turbulence)
  bool lookback = false;
  if (pin.DoesParameterExist("apk_amd", "tracer_lookback")) {
    const std::string v = pin.GetString("apk_amd", "tracer_lookback");
    if (v != "true" && v != "false") throw std::runtime_error("apk_amd/tracer_lookback must be true or false");
    lookback = v == "true";
  }
  if (!pin.GetOrAddBoolean("tracers", "enabled", false)) {
    if (lookback) throw std::runtime_error("apk_amd/tracer_lookback = true needs tracers/enabled = true");
    return;
  }
  const Mesh &m = s->mesh;
  // tracers.cpp:70-71
  if (m.nx[2] <= 1) throw std::runtime_error("Tracers/swarms currently only supported/tested in 3D.");
  // tracers.cpp:77-79 refuses adaptive meshes; static ones too here: interpolation across levels is not defined there
  if (pin.GetOrAddString("parthenon/mesh", "refinement", "none") != "none")
    throw std::runtime_error("Tracers/swarms currently only supported on uniform meshes (parthenon/mesh/refinement = none).");
  if (s->nranks > 1) throw std::runtime_error("tracers need a single rank for now");
  // the predictor position of Heun's method lies up to one cell outside the block: its stencil reaches two ghost layers
  if (m.ng < 2) throw std::runtime_error("tracers need parthenon/mesh/nghost >= 2: the advection reads two ghost layers");
  auto t = std::make_unique<TracerState>();
  t->nfields = s->pkg.fluid == APK_FLUID_GLMMHD ? 8 : 5;
  const std::string form = pin.GetOrAddString("apk_amd", "tracer_step", "fused");
  if (form != "fused" && form != "passes") throw std::runtime_error("apk_amd/tracer_step must be fused or passes");
  t->fused = form == "fused";
  t->lookback = lookback;
  const std::string method = pin.GetOrAddString("tracers", "initial_seed_method", "none");
  t->per_cell = pin.GetOrAddReal("tracers", "initial_num_tracers_per_cell", 0.0);
  t->rng_seed = pin.GetOrAddInteger("tracers", "initial_rng_seed", 0);
  if (method == "none") t->seed_method = APK_TRACER_SEED_NONE;
  else if (method == "user") t->seed_method = APK_TRACER_SEED_USER;
  else if (method == "random_per_block") t->seed_method = APK_TRACER_SEED_RANDOM_PER_BLOCK;
  else throw std::runtime_error("Unknown tracer initial_seed_method");  // tracers.cpp:170
  if (t->seed_method == APK_TRACER_SEED_RANDOM_PER_BLOCK) {
    // tracers.cpp:108-115
    if (!(t->per_cell > 0.0)) throw std::runtime_error("You should seed at least some tracers.");
    const long long cells = (long long)m.mb[0] * m.mb[1] * m.mb[2];
    const int per_block = static_cast<int>((double)cells * t->per_cell);
    if (per_block <= 0) throw std::runtime_error("Resulting number of particles per block is invalid.");
    // tracers.cpp:120-168 over this rank's blocks in local order
    const size_t nlb = m.local_gids.size();
    const size_t total = nlb * (size_t)per_block;
    t->hx.resize(total), t->hy.resize(total), t->hz.resize(total), t->hid.resize(total), t->hblock.resize(total);
    for (size_t lb = 0; lb < nlb; ++lb) {
      const int gid = m.local_gids[lb];
      int bc[3];
      m.Loc(gid, bc);
      double o[3], size[3];
      for (int d = 0; d < 3; ++d) {
        size[d] = (double)m.mb[d] * s->dx[d];
        o[d] = s->xmin[d] + (double)(bc[d] * m.mb[d]) * s->dx[d];
      }
      const uint64_t key = (uint64_t)(t->rng_seed + (long long)gid);
      for (int n = 0; n < per_block; ++n) {
        const size_t q = lb * (size_t)per_block + n;
        t->hx[q] = o[0] + tracer_uniform(key, (uint64_t)n, 0) * size[0];
        t->hy[q] = o[1] + tracer_uniform(key, (uint64_t)n, 1) * size[1];
        t->hz[q] = o[2] + tracer_uniform(key, (uint64_t)n, 2) * size[2];
        t->hid[q] = (int64_t)per_block * gid + n;
        t->hblock[q] = (int32_t)lb;
      }
    }
  }
  s->tracers = std::move(t);
}

int tracers_device_setup(apk_sim *s) {
  if (!s->tracers) return APK_OK;
  TracerState &t = *s->tracers;
  const Mesh &m = s->mesh;
  const size_t nlb = m.local_gids.size();
  apk_tracer_geom &g = t.geom;
  std::vector<double> origin(3 * nlb);
  std::vector<int32_t> table((size_t)m.nblocks_total + 1, 0);  // (+1: an even number of words)
  for (int d = 0; d < 3; ++d) {
    g.xmin[d] = s->xmin[d], g.xmax[d] = s->xmax[d], g.dx[d] = s->dx[d];
    g.block_size[d] = (double)m.mb[d] * s->dx[d];
    g.nb[d] = m.nb[d];
    g.periodic_lo[d] = m.bc_in[d] == BC_PERIODIC ? 1 : 0;
    g.periodic_hi[d] = m.bc_out[d] == BC_PERIODIC ? 1 : 0;
  }
  for (size_t lb = 0; lb < nlb; ++lb) {
    int bc[3];
    m.Loc(m.local_gids[lb], bc);
    for (int d = 0; d < 3; ++d) origin[3 * lb + d] = s->xmin[d] + (double)(bc[d] * m.mb[d]) * s->dx[d];
    table[m.local_gids[lb]] = (int32_t)lb;  // (Gid is x-fastest: the table's [nb2][nb1][nb0])
  }
  t.nbuckets = (int)nlb * m.mb[2] + 1;
  SIM_TRY(s, dev_alloc(s, "tracer_block_origin", sizeof(double) * origin.size(), &t.d_origin));
  SIM_TRY(s, dev_alloc(s, "tracer_block_table", sizeof(int32_t) * table.size(), &t.d_table));
  const size_t counter_words = t.lookback ? 2 + kSums : 2;  // (the 26 sums of the lookbacks behind the counters)
  SIM_TRY(s, dev_alloc(s, "tracer_counters", counter_words * sizeof(unsigned long long), &t.d_counters));
  SIM_TRY(s, dev_alloc(s, "tracer_buckets", sizeof(unsigned long long) * (size_t)t.nbuckets, &t.d_buckets));
  SIM_HIP(s, hipMemcpy(t.d_origin, origin.data(), sizeof(double) * origin.size(), hipMemcpyHostToDevice));
  SIM_HIP(s, hipMemcpy(t.d_table, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice));
  SIM_HIP(s, hipMemset(t.d_counters, 0, counter_words * sizeof(unsigned long long)));
  g.block_origin = t.d_origin;
  g.block_table = reinterpret_cast<const int32_t *>(t.d_table);
  return APK_OK;
}

// SeedInitialTracers (tracers.cpp:95-186), called by apk_sim_initialize once the initial state, its ghost zones and its
// primitives are in place: particles of an earlier initialisation are dropped
int tracers_seed_initial(apk_sim *s) {
  if (!s->tracers) return APK_OK;
  TracerState &t = *s->tracers;
  t.n = 0;
  t.lost = 0;
  t.next_id = 0;
  t.steps = t.sorts = 0;
  SIM_HIP(s, hipMemsetAsync(t.d_counters, 0, 2 * sizeof(unsigned long long), hs(s)));
  if (t.lookback) {  // empty histories (append zeroes what it adds), no row yet, a fresh file
    for (double &v : t.t_lookback) v = 0.0;
    for (double &v : t.row) v = 0.0;
    t.row_cycle = -1, t.row_active = 0, t.row_time = 0.0;
    SIM_TRY(s, lookback_csv(s, true));
  }
  if (t.seed_method != APK_TRACER_SEED_RANDOM_PER_BLOCK) return APK_OK;
  SIM_TRY(s, append(s, t.hx.data(), t.hy.data(), t.hz.data(), t.hid.data(), t.hblock.data(), (int64_t)t.hx.size()));
  SIM_TRY(s, sort_particles(s));
  SIM_TRY(s, fill_particles(s));  // tracers.cpp:173-186
  if (!t.lookback || t.n == 0) return APK_OK;
  // ... which end with ProblemFillTracers at cycle 0 with the sim's dt: every level shifts, s[0] = ln rho of the seeded
  // state.  The first cycle runs with cycle number 0 again and truncates the file, so this call writes no row; what it
  // leaves is s[1] (and t_lookback[1]) of the first row.
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n);
  SIM_TRY(s, apk_tracers_lookback(s->ctx, &a, 0, s->dt, t.d_partials, t.partials_cap, lookback_sums(t), s->stream));
  unsigned long long c[2 + kSums] = {0};
  SIM_TRY(s, read_counters(s, c));
  return lookback_row(s, 0, s->time, c);
}

int tracers_cycle(apk_sim *s, double dt) {
  if (!s->tracers || s->tracers->n == 0) return APK_OK;
  TracerState &t = *s->tracers;
  // Many cycles store no primitives and copy no same-rank ghost zones: both gathers need the primitives of the new time
  // with edges and corners filled
  CompletedState state(s);
  SIM_TRY(s, state.complete());
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n);
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(t.d_counters);
  // the lookbacks run with the cycle being executed and the time at its start (tm.ncycle, tm.time of the task):
  // apk_sim_step increments both after this call
  const long long cycle = s->ncycle;
  if (t.fused && t.lookback) {
    SIM_TRY(s, apk_tracers_step_fused_lookback(s->ctx, s->mu0(), &a, &t.geom, dt, counters, cycle, t.d_partials, t.partials_cap,
                                               lookback_sums(t), s->stream));
  } else if (t.fused) {
    SIM_TRY(s, apk_tracers_step_fused(s->ctx, s->mu0(), &a, &t.geom, dt, counters, s->stream));
  } else {
    SIM_TRY(s, apk_tracers_advect(s->ctx, s->mu0(), &a, &t.geom, dt, s->stream));
    SIM_TRY(s, apk_tracers_reown(s->ctx, &a, &t.geom, counters, s->stream));
    SIM_TRY(s, apk_tracers_fill(s->ctx, s->mu0(), &a, &t.geom, s->stream));
    if (t.lookback)  // the reference's task order: ProblemFillTracers after FillTracers (hydro_driver.cpp:654-658)
      SIM_TRY(s, apk_tracers_lookback(s->ctx, &a, cycle, dt, t.d_partials, t.partials_cap, lookback_sums(t), s->stream));
  }
  t.steps += 1;
  unsigned long long c[2 + kSums] = {0};
  SIM_TRY(s, read_counters(s, c));
  t.lost = (long long)c[0];
  if (t.lookback) {
    SIM_TRY(s, lookback_row(s, cycle, s->time, c));
    SIM_TRY(s, lookback_csv(s, false));
  }
  if (c[1] != 0ull) {  // ownership changed: restore the order by (block, k-plane)
    SIM_HIP(s, hipMemsetAsync(counters + 1, 0, sizeof(unsigned long long), hs(s)));
    SIM_TRY(s, sort_particles(s));
  }
  return APK_OK;
}

// one array per field, sorted by id: <prefix>.<name>.npy
int tracers_write_outputs(apk_sim *s, const std::string &prefix) {
  if (!s->tracers) return APK_OK;
  TracerState &t = *s->tracers;
  const size_t n = (size_t)t.n;
  std::vector<int64_t> id(n);
  std::vector<int32_t> i32(n), tmp32(n);
  std::vector<double> buf(n), sorted(n);
  SIM_TRY(s, apk_sim_tracers_read(s, 3, id.data()));
  std::vector<size_t> order(n);
  for (size_t q = 0; q < n; ++q) order[q] = q;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return id[a] < id[b]; });
  std::vector<int64_t> id_sorted(n);
  for (size_t q = 0; q < n; ++q) id_sorted[q] = id[order[q]];
  if (!write_npy(prefix + ".id.npy", "<i8", id_sorted.data(), n, 8)) return fail(s, APK_ERR_INVALID, "cannot write " + prefix + ".id.npy");
  const char *names[3] = {"x", "y", "z"};
  for (int f = 0; f < 3 + t.nfields; ++f) {
    SIM_TRY(s, apk_sim_tracers_read(s, f < 3 ? f : 3 + f, buf.data()));
    for (size_t q = 0; q < n; ++q) sorted[q] = buf[order[q]];
    const std::string path = prefix + "." + (f < 3 ? names[f] : kFieldNames[f - 3]) + ".npy";
    if (!write_npy(path, "<f8", sorted.data(), n, 8)) return fail(s, APK_ERR_INVALID, "cannot write " + path);
  }
  SIM_TRY(s, apk_sim_tracers_read(s, 5, tmp32.data()));
  for (size_t q = 0; q < n; ++q) i32[q] = tmp32[order[q]];
  if (!write_npy(prefix + ".active.npy", "<i4", i32.data(), n, 4)) return fail(s, APK_ERR_INVALID, "cannot write " + prefix + ".active.npy");
  return APK_OK;
}

void tracers_free(apk_sim *s) {
  if (!s->tracers) return;
  TracerState &t = *s->tracers;
  dev_free(s, t.set[0]);
  dev_free(s, t.set[1]);
  dev_free(s, t.d_origin);
  dev_free(s, t.d_table);
  dev_free(s, t.d_counters);
  dev_free(s, t.d_buckets);
  dev_free(s, t.d_partials);
  t.d_partials = nullptr;
  t.set[0] = t.set[1] = t.d_origin = t.d_table = t.d_counters = t.d_buckets = nullptr;
}

}  // namespace host
}  // namespace apk

using namespace apk;
using namespace apk::host;

extern "C" {

int apk_sim_tracers_options(const apk_sim *s, apk_tracers_options *o) {
  if (!s || !o) return APK_ERR_INVALID;
  *o = apk_tracers_options{};
  if (!s->tracers) return APK_OK;
  const TracerState &t = *s->tracers;
  o->enabled = 1;
  o->seed_method = t.seed_method;
  o->fused = t.fused ? 1 : 0;
  o->nfields = t.nfields;
  o->num_tracers_per_cell = t.per_cell;
  o->rng_seed = t.rng_seed;
  if (t.seed_method == APK_TRACER_SEED_RANDOM_PER_BLOCK)
    o->num_tracers_per_block = static_cast<int>((double)((long long)s->mesh.mb[0] * s->mesh.mb[1] * s->mesh.mb[2]) * t.per_cell);
  return APK_OK;
}

int apk_sim_tracers_count(apk_sim *s, long long *total, long long *active, long long *lost) {
  if (!s) return APK_ERR_INVALID;
  if (!s->tracers) return fail(s, APK_ERR_INVALID, "tracers are not enabled (tracers/enabled = true)");
  const TracerState &t = *s->tracers;
  const long long n = s->host_only ? (long long)t.hx.size() : (long long)t.n;
  if (total) *total = n;
  if (active) *active = n - t.lost;
  if (lost) *lost = t.lost;
  return APK_OK;
}

int apk_sim_tracers_stats(const apk_sim *s, long long *steps, long long *sorts) {
  if (!s || !s->tracers) return APK_ERR_INVALID;
  if (steps) *steps = s->tracers->steps;
  if (sorts) *sorts = s->tracers->sorts;
  return APK_OK;
}

int apk_sim_tracers_read(apk_sim *s, int field, void *out) {
  if (!s || !out) return APK_ERR_INVALID;
  if (!s->tracers) return fail(s, APK_ERR_INVALID, "tracers are not enabled (tracers/enabled = true)");
  TracerState &t = *s->tracers;
  if (field < 0 || field >= 6 + t.nfields) return fail(s, APK_ERR_INVALID, "apk_sim_tracers_read: no such field");
  if (s->host_only) {
    const size_t n = t.hx.size();
    if (field == 0) std::memcpy(out, t.hx.data(), n * 8);
    else if (field == 1) std::memcpy(out, t.hy.data(), n * 8);
    else if (field == 2) std::memcpy(out, t.hz.data(), n * 8);
    else if (field == 3) std::memcpy(out, t.hid.data(), n * 8);
    else if (field == 4) std::memcpy(out, t.hblock.data(), n * 4);
    else return fail(s, APK_ERR_INVALID, "apk_sim_tracers_read: a host-only sim holds positions, ids and blocks only");
    return APK_OK;
  }
  if (t.n == 0) return APK_OK;
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n);
  const void *src = field == 0 ? (const void *)a.x : field == 1 ? (const void *)a.y : field == 2 ? (const void *)a.z
                    : field == 3 ? (const void *)a.id : field == 4 ? (const void *)a.block : field == 5 ? (const void *)a.active
                    : (const void *)a.field[field - 6];
  const size_t item = (field == 4 || field == 5) ? 4 : 8;
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  SIM_HIP(s, hipMemcpy(out, src, item * (size_t)t.n, hipMemcpyDeviceToHost));
  return APK_OK;
}

int apk_sim_tracers_seed(apk_sim *s, const double *x, const double *y, const double *z, long long n) {
  if (!s || s->host_only || n < 0 || (n > 0 && (!x || !y || !z))) return APK_ERR_INVALID;
  if (!s->tracers) return fail(s, APK_ERR_INVALID, "tracers are not enabled (tracers/enabled = true)");
  TracerState &t = *s->tracers;
  if (t.seed_method != APK_TRACER_SEED_USER) return fail(s, APK_ERR_INVALID, "apk_sim_tracers_seed needs tracers/initial_seed_method = user");
  if (n == 0) return APK_OK;
  std::vector<int64_t> id((size_t)n);
  std::vector<int32_t> block((size_t)n);
  for (long long q = 0; q < n; ++q) {
    const double p[3] = {x[q], y[q], z[q]};
    for (int d = 0; d < 3; ++d)
      if (!(p[d] >= s->xmin[d] && p[d] < s->xmax[d])) return fail(s, APK_ERR_INVALID, "apk_sim_tracers_seed: position outside the domain");
    id[(size_t)q] = t.next_id + q;
    block[(size_t)q] = (int32_t)owner_of(s, p);
  }
  SIM_TRY(s, append(s, x, y, z, id.data(), block.data(), (int64_t)n));
  t.next_id += n;
  SIM_TRY(s, sort_particles(s));
  return fill_particles(s);
}

int apk_sim_tracer_lookback_options(const apk_sim *s, int *enabled, int *n_lookback) {
  if (!s) return APK_ERR_INVALID;
  if (enabled) *enabled = s->tracers && s->tracers->lookback ? 1 : 0;
  if (n_lookback) *n_lookback = kLookback;
  return APK_OK;
}

int apk_sim_tracer_lookbacks_read(apk_sim *s, int which, double *out) {
  if (!s || s->host_only || !out || which < 0 || which > 1) return APK_ERR_INVALID;
  if (!s->tracers || !s->tracers->lookback) return fail(s, APK_ERR_INVALID, "tracer lookbacks are not enabled (apk_amd/tracer_lookback = true)");
  TracerState &t = *s->tracers;
  if (t.n == 0) return APK_OK;
  const apk_tracer_arrays a = arrays_of(t, t.cur, t.n);
  SIM_HIP(s, hipStreamSynchronize(hs(s)));
  SIM_HIP(s, hipMemcpy2D(out, sizeof(double) * (size_t)t.n, which == 0 ? a.s : a.sdot, sizeof(double) * (size_t)a.lookback_stride,
                         sizeof(double) * (size_t)t.n, kLookback, hipMemcpyDeviceToHost));
  return APK_OK;
}

int apk_sim_tracer_correlations(const apk_sim *s, long long *cycle, double *time, long long *n_active, double *row) {
  if (!s || !s->tracers || !s->tracers->lookback) return APK_ERR_INVALID;
  const TracerState &t = *s->tracers;
  if (cycle) *cycle = t.row_cycle;
  if (time) *time = t.row_time;
  if (n_active) *n_active = t.row_active;
  if (row) {
    std::memcpy(row, t.row, sizeof t.row);
    std::memcpy(row + 2 + 2 * kLookback, t.t_lookback, sizeof t.t_lookback);
  }
  return APK_OK;
}

int apk_sim_tracers_step(apk_sim *s, double dt) {
  if (!s || s->host_only) return APK_ERR_INVALID;
  if (!s->tracers) return fail(s, APK_ERR_INVALID, "tracers are not enabled (tracers/enabled = true)");
  s->err.clear();
  return tracers_cycle(s, dt);
}

}  // extern "C"
