"""Reader of restart state files (include/apk_host.h "restart"): <prefix>.rst, text in the deck format -- the deck as
parsed plus the block <apk_amd/restart> with the driver's mutable state.  The conserved state of the dump lies next to it
as a field snapshot (<prefix>.json, <prefix>.rank<r>.npy: athenapk_amd.snapshots.load(prefix + ".json") reads it).

    text = restart.deck("out/turbulence.out3.00002.rst")      # a deck: what the resumed Simulation is built from
    sim = driver.Simulation(text, ["parthenon/time/tlim=2.0"]).restore("out/turbulence.out3.00002.rst")
    st = restart.state("out/turbulence.out3.00002.rst")       # {"time": ..., "cycle": ..., "blocks": [...], ...}

No library, no GPU.
"""

BLOCK = "apk_amd/restart"
FORMAT_VERSION = 1
_INTS = ("format_version", "cycle", "fofc_total", "fofc_fallback_stages", "zone_cycles", "amr_refined", "amr_derefined",
         "nranks", "nblocks", "nvar", "nghost")
_STRINGS = ("fluid", "refinement")
_TRIPLES = ("mesh_nx", "block_nx")


def parse(text):
    """deck text -> {block: {key: value string}}, as the driver's reader does: '#' starts a comment, '<block>' a block"""
    out, block = {}, None
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if line.startswith("<"):
            if ">" not in line:
                raise ValueError("unterminated block header: " + line)
            block = line[1:line.index(">")].strip()
            out.setdefault(block, {})
            continue
        if "=" not in line or block is None:
            raise ValueError("expected key = value inside a block: " + line)
        k, v = line.split("=", 1)
        out[block][k.strip()] = v.strip()
    return out


def deck(path):
    """the text of the state file `path`, which is a deck: the writing run's deck with its overrides applied, the state
    block, and for problem_id = turbulence the driver's spectral state and RNG in <problem/turbulence>"""
    with open(str(path)) as f:
        text = f.read()
    if BLOCK not in parse(text):
        raise ValueError("%s: not a restart state file (no <%s> block)" % (path, BLOCK))
    return text


def state(path):
    """the mutable state of the dump: the keys of <apk_amd/restart> with their types -- doubles exactly as written
    (%.17g; inf stays inf), integers, "blocks": [{"gid", "level", "lx1", "lx2", "lx3", "deref_count", "rank", "index"}],
    "outputs": {N: {"next_time", "counter"}} -- and "turbulence": {"accel_hat": [3][M] complex, "state_rng", "state_dist"}
    where the state file has them"""
    blocks = parse(deck(path))
    raw = blocks[BLOCK]
    version = int(raw["format_version"])
    if version != FORMAT_VERSION:
        raise ValueError("%s: format_version = %d, this reader knows %d" % (path, version, FORMAT_VERSION))
    out, table, outputs = {}, {}, {}
    for k, v in raw.items():
        if k in _INTS:
            out[k] = int(v)
        elif k in _STRINGS:
            out[k] = v
        elif k in _TRIPLES:
            out[k] = tuple(int(x) for x in v.split())
        elif k.startswith("block_") and k[6:].isdigit():
            w = [int(x) for x in v.split()]
            table[int(k[6:])] = dict(zip(("level", "lx1", "lx2", "lx3", "deref_count", "rank", "index"), w), gid=int(k[6:]))
        elif k.startswith("output") and k.endswith("_next_time"):
            outputs.setdefault(k[6:-len("_next_time")], {})["next_time"] = float(v)
        elif k.startswith("output") and k.endswith("_counter"):
            outputs.setdefault(k[6:-len("_counter")], {})["counter"] = int(v)
        else:
            out[k] = float(v)
    out["blocks"] = [table[g] for g in sorted(table)]
    out["outputs"] = outputs
    if len(out["blocks"]) != out["nblocks"] or sorted(table) != list(range(out["nblocks"])):
        raise ValueError("%s: the block table does not hold nblocks = %d blocks" % (path, out["nblocks"]))
    turb = blocks.get("problem/turbulence", {})
    if "state_rng" in turb:
        M = int(turb["num_modes"])
        out["turbulence"] = {
            "accel_hat": [[complex(float(turb["accel_hat_%d_%d_r" % (i, m)]), float(turb["accel_hat_%d_%d_i" % (i, m)]))
                           for m in range(M)] for i in range(3)],
            "state_rng": turb["state_rng"], "state_dist": turb["state_dist"]}
    return out
