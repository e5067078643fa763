"""Reader of field snapshots (include/apk_host.h "field snapshots"): <prefix>.json, the index rank 0 writes, and
<prefix>.rank<r>.npy, one array of shape (nblocks_local, ncomp, nx3, nx2, nx1) per rank with the interior cells of its
blocks in local order.  numpy only; no library, no GPU.

    snap = snapshots.load("out/blast.out2.00003.json")
    rho = snap.component("prim.rho")          # uniform meshes: [NX3][NX2][NX1]
    for b in snap.blocks:                     # refined meshes: block by block
        lo, hi = snap.block_bounds(b["gid"])
        data = snap.block(b["gid"])           # [ncomp][nx3][nx2][nx1]
"""
import json

import numpy as np


class Snapshot:
    def __init__(self, json_path):
        self.path = str(json_path)
        if not self.path.endswith(".json"):
            raise ValueError("%s: a snapshot is loaded from its .json index" % self.path)
        self.prefix = self.path[:-len(".json")]
        with open(self.path) as f:
            self.index = json.load(f)
        ix = self.index
        self.time, self.cycle, self.dt = ix["time"], ix["cycle"], ix["dt"]
        self.components = list(ix["components"])
        self.dtype = np.dtype(ix["dtype"])
        self.blocks = list(ix["blocks"])
        self.block_nx = tuple(ix["block_nx"])
        self.mesh_nx = tuple(ix["mesh_nx"])
        self.xmin, self.xmax = tuple(ix["xmin"]), tuple(ix["xmax"])
        self._by_gid = {b["gid"]: b for b in self.blocks}
        self._rank_files = {}

    @property
    def refined(self):
        return any(b["level"] != 0 for b in self.blocks)

    def _rank_array(self, rank):
        if rank not in self._rank_files:
            a = np.load("%s.rank%d.npy" % (self.prefix, rank), mmap_mode="r")
            want = (len(self.components),) + tuple(reversed(self.block_nx))
            if a.ndim != 5 or a.shape[1:] != want or a.dtype != self.dtype:
                raise ValueError("%s.rank%d.npy holds %s %s, the index says (n,) + %s %s"
                                 % (self.prefix, rank, a.shape, a.dtype, want, self.dtype))
            self._rank_files[rank] = a
        return self._rank_files[rank]

    def block(self, gid):
        """[ncomp][nx3][nx2][nx1] of global block gid (a view into the memory-mapped rank file)"""
        b = self._by_gid[gid]
        return self._rank_array(b["rank"])[b["index"]]

    def block_bounds(self, gid):
        """(min corner, max corner) of global block gid, from its level and logical location: a block of level l spans
        block_nx cells of width (xmax - xmin) / mesh_nx / 2^l in every active direction"""
        b = self._by_gid[gid]
        lo, hi = [], []
        for d, lx in enumerate((b["lx1"], b["lx2"], b["lx3"])):
            if self.mesh_nx[d] == 1:  # a collapsed direction is not refined
                lo.append(self.xmin[d])
                hi.append(self.xmax[d])
                continue
            w = (self.xmax[d] - self.xmin[d]) * self.block_nx[d] / (self.mesh_nx[d] << b["level"])
            lo.append(self.xmin[d] + lx * w)
            hi.append(self.xmin[d] + (lx + 1) * w)
        return tuple(lo), tuple(hi)

    def component(self, name):
        """the assembled [NX3][NX2][NX1] array of one component on a uniform mesh"""
        if self.refined:
            raise ValueError("component() assembles uniform meshes only: this snapshot has refined blocks, iterate over "
                             "snapshot.blocks with block(gid) and block_bounds(gid)")
        c = self.components.index(name)
        nx1, nx2, nx3 = self.block_nx
        out = np.empty(tuple(reversed(self.mesh_nx)), dtype=self.dtype)
        for b in self.blocks:
            i, j, k = b["lx1"] * nx1, b["lx2"] * nx2, b["lx3"] * nx3
            out[k:k + nx3, j:j + nx2, i:i + nx1] = self.block(b["gid"])[c]
        return out


def load(json_path):
    """the Snapshot behind a dump's .json index"""
    return Snapshot(json_path)
