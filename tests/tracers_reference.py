"""numpy restatement of the tracer particles (test infrastructure): seeding, trilinear interpolation on cell centres,
Heun's method, periodic wrap / loss, ownership on the uniform block grid, and the fill.  Written from the description of
the scheme, operation by operation in IEEE double without contraction, so that the strict
(-ffp-contract=off) build can be compared bit for bit.

Conventions
  * a block's arrays are [nvar][Nk][Nj][Ni] including `ng` ghost cells; primitives are rho, v1, v2, v3, p [, B1, B2, B3, psi]
  * origin = lower interior face of the block, xmin + (block coordinate * cells per block) * dx
  * per direction: il = floor((x - origin) / dx - 1/2) counted from the first interior cell (the cell whose centre is
    <= x), w_lo = ((origin + ((il + 1) + 1/2) dx) - x) / dx, w_hi = 1 - w_lo; summed x first, then y, then z
  * fields: rho, pressure, vel_x, vel_y, vel_z [, B_x, B_y, B_z] = primitives 0, 4, 1, 2, 3 [, 5, 6, 7]
"""
import numpy as np

FIELD_VARS = (0, 4, 1, 2, 3, 5, 6, 7)
FIELD_NAMES = ("rho", "pressure", "vel_x", "vel_y", "vel_z", "B_x", "B_y", "B_z")
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform(key, n, c):
    """r in [0, 1) with a 53-bit mantissa from the chained hash of (key, n, c)"""
    key = np.uint64(int(key) & 0xFFFFFFFFFFFFFFFF)
    u = splitmix64(splitmix64(splitmix64(key) ^ np.asarray(n, dtype=np.uint64)) ^ np.uint64(c))
    return (u >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


class Grid:
    """the uniform block grid: domain, cells, cells per block, ghost depth, periodicity per side"""

    def __init__(self, xmin, xmax, nx, mb, ng, periodic_lo=(True, True, True), periodic_hi=(True, True, True)):
        self.xmin = np.array(xmin, dtype=np.float64)
        self.xmax = np.array(xmax, dtype=np.float64)
        self.nx, self.mb, self.ng = tuple(nx), tuple(mb), ng
        self.dx = (self.xmax - self.xmin) / np.array(nx, dtype=np.float64)
        self.nb = tuple(n // m for n, m in zip(nx, mb))
        self.block_size = np.array(mb, dtype=np.float64) * self.dx
        self.periodic_lo, self.periodic_hi = tuple(periodic_lo), tuple(periodic_hi)

    def gid(self, bc):
        return bc[0] + self.nb[0] * (bc[1] + self.nb[1] * bc[2])

    def loc(self, gid):
        return (gid % self.nb[0], (gid // self.nb[0]) % self.nb[1], gid // (self.nb[0] * self.nb[1]))

    def origin(self, gid):
        bc = self.loc(gid)
        return np.array([self.xmin[d] + float(bc[d] * self.mb[d]) * self.dx[d] for d in range(3)])


def seed_random_per_block(grid, per_cell, rng_seed):
    """ids, positions and gids of tracers/initial_seed_method = random_per_block over the whole mesh, sorted by id"""
    cells = grid.mb[0] * grid.mb[1] * grid.mb[2]
    per_block = int(cells * per_cell)
    n = np.arange(per_block, dtype=np.uint64)
    out = {k: [] for k in ("x", "y", "z", "id", "gid")}
    for gid in range(grid.nb[0] * grid.nb[1] * grid.nb[2]):
        o = grid.origin(gid)
        for d, name in enumerate("xyz"):
            out[name].append(o[d] + uniform(rng_seed + gid, n, d) * grid.block_size[d])
        out["id"].append(per_block * gid + np.arange(per_block, dtype=np.int64))
        out["gid"].append(np.full(per_block, gid, dtype=np.int64))
    return {k: np.concatenate(v) for k, v in out.items()}


def _axis(x, origin, dx, nx, ng):
    t = (x - origin) / dx - 0.5
    il = np.floor(t).astype(np.int64)
    il = np.clip(il, -ng, nx + ng - 2)  # (the guard of the allocated extent; never active for |v| dt < dx)
    wlo = ((origin + ((il + 1).astype(np.float64) + 0.5) * dx) - x) / dx
    return il, wlo


def interpolate(grid, prim_blocks, gids, x, y, z, variables):
    """prim_blocks: {gid: [nvar][Nk][Nj][Ni]}; gids: owning block per particle; returns [len(variables)][n]"""
    n = len(x)
    out = np.zeros((len(variables), n))
    ng = grid.ng
    for gid in np.unique(gids):
        sel = np.nonzero(gids == gid)[0]
        o = grid.origin(int(gid))
        il, wx0 = _axis(x[sel], o[0], grid.dx[0], grid.mb[0], ng)
        jl, wy0 = _axis(y[sel], o[1], grid.dx[1], grid.mb[1], ng)
        kl, wz0 = _axis(z[sel], o[2], grid.dx[2], grid.mb[2], ng)
        wx1, wy1, wz1 = 1.0 - wx0, 1.0 - wy0, 1.0 - wz0
        i0, j0, k0 = il + ng, jl + ng, kl + ng
        w = prim_blocks[int(gid)]
        for q, v in enumerate(variables):
            f = w[v]
            c00 = wx0 * f[k0, j0, i0] + wx1 * f[k0, j0, i0 + 1]
            c01 = wx0 * f[k0, j0 + 1, i0] + wx1 * f[k0, j0 + 1, i0 + 1]
            c10 = wx0 * f[k0 + 1, j0, i0] + wx1 * f[k0 + 1, j0, i0 + 1]
            c11 = wx0 * f[k0 + 1, j0 + 1, i0] + wx1 * f[k0 + 1, j0 + 1, i0 + 1]
            c0 = wy0 * c00 + wy1 * c01
            c1 = wy0 * c10 + wy1 * c11
            out[q, sel] = wz0 * c0 + wz1 * c1
    return out


def owner(grid, x, y, z):
    """gid of the block containing each (in-domain) position"""
    bc = []
    for d, p in enumerate((x, y, z)):
        c = np.floor((p - grid.xmin[d]) / grid.block_size[d]).astype(np.int64)
        bc.append(np.clip(c, 0, grid.nb[d] - 1))
    return bc[0] + grid.nb[0] * (bc[1] + grid.nb[1] * bc[2])


def step(grid, prim_blocks, state, dt, nfields):
    """one tracer step in place on state = {x, y, z, gid, active, <fields>}: Heun, wrap / loss, owner, fill.
    Inactive particles are left alone; a particle lost in this step keeps its unwrapped position and its old fields."""
    act = np.nonzero(state["active"] != 0)[0]
    x, y, z = state["x"][act], state["y"][act], state["z"][act]
    gids = state["gid"][act]
    vp = [state[n][act] for n in ("vel_x", "vel_y", "vel_z")]
    xs, ys, zs = x + dt * vp[0], y + dt * vp[1], z + dt * vp[2]
    vs = interpolate(grid, prim_blocks, gids, xs, ys, zs, (1, 2, 3))
    hdt = 0.5 * dt
    new = [x + hdt * (vp[0] + vs[0]), y + hdt * (vp[1] + vs[1]), z + hdt * (vp[2] + vs[2])]
    adv = [p.copy() for p in new]
    kept = np.ones(len(act), dtype=bool)
    for d in range(3):
        L = grid.xmax[d] - grid.xmin[d]
        # (direction by direction, a particle already lost is not looked at again)
        lo = kept & (new[d] < grid.xmin[d])
        hi = kept & ~lo & (new[d] >= grid.xmax[d])
        if grid.periodic_lo[d]:
            new[d] = np.where(lo, new[d] + L, new[d])
        else:
            kept &= ~lo
        if grid.periodic_hi[d]:
            new[d] = np.where(hi, new[d] - L, new[d])
        else:
            kept &= ~hi
    for d, name in enumerate("xyz"):
        state[name][act] = np.where(kept, new[d], adv[d])
    k = act[kept]
    state["active"][act[~kept]] = 0
    state["gid"][k] = owner(grid, state["x"][k], state["y"][k], state["z"][k])
    fill(grid, prim_blocks, state, nfields, k)
    return state


def fill(grid, prim_blocks, state, nfields, which=None):
    if which is None:
        which = np.nonzero(state["active"] != 0)[0]
    vals = interpolate(grid, prim_blocks, state["gid"][which], state["x"][which], state["y"][which], state["z"][which],
                       FIELD_VARS[:nfields])
    for q in range(nfields):
        state[FIELD_NAMES[q]][which] = vals[q]
    return state
