"""CPU restatement of the host's choice of path for a structural hspf_graph_patch (graph_patch_impl in
holo_amd/csrc/spf_capi.hip) and the generators of the cases at its limits (tests/test_host_patch_model.py checks that every
case sits where it claims, tests/test_gpu_patch_limits.py runs them on the device).  Plain numpy, no GPU import.

The constants are READ from the sources (the `constexpr` lines and the expressions of graph_patch_impl), not typed in again:
a changed constant moves the cases with it, an expression this file no longer recognises fails the import loudly."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np

from holo_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "holo_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(name, pattern, what):
    m = re.search(pattern, _text(name))
    if not m:
        raise RuntimeError(f"tests/_patch_model.py: {what} not found in holo_amd/csrc/{name} (pattern {pattern!r})")
    return tuple(int(x) for x in m.groups())


def _constexpr(name, const):
    return _find(name, r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)u?\s*;" % const, "constexpr " + const)[0]


PA_MAX_ROWS = _constexpr("graph_patch.hip.h", "PA_MAX_ROWS")
PA_LDS_ROWS = _constexpr("graph_patch.hip.h", "PA_LDS_ROWS")
PA_IN_STRIDE = _constexpr("graph_patch.hip.h", "PA_IN_STRIDE")
PA_OUT_STRIDE = _constexpr("graph_patch.hip.h", "PA_OUT_STRIDE")
GIANT_DEG = _constexpr("spf_kernels.hip.h", "GIANT_DEG")
HUB_DEG = _constexpr("graph_build.hip.h", "HUB_DEG")
GB_UNITS_MAX_CHUNKS = _constexpr("graph_build.hip.h", "GB_UNITS_MAX_CHUNKS")
# the list of affected rows is looked at (deduplicated) whenever it holds more than AFF_FACTOR * PA_MAX_ROWS entries
AFF_FACTOR, = _find("spf_capi.hip", r"aff\.size\(\)\s*>\s*(\d+)u\s*\*\s*PA_MAX_ROWS", "the size bound of the affected list")
# tw_bound = max(TW_MIN, e_new / TW_DIV)
TW_MIN, TW_DIV = _find("spf_capi.hip", r"std::max<uint64_t>\((\d+)u,\s*e_new\s*/\s*(\d+)u\)", "the default two-way work bound")
# link capacity of the arena: e + max(e / a, b) at upload, e_new + max(e_new / c, d) when a patch grows it
CAP_UP_DIV, CAP_UP_MIN = _find("spf_capi.hip", r"alloc_arena\(ctx, g, n, e \+ std::max\(e / (\d+), (\d+)u\)\)", "the upload's spare capacity")
CAP_GROW_DIV, CAP_GROW_MIN = _find("spf_capi.hip", r"cap = e_new \+ std::max\(e_new / (\d+), (\d+)u\)", "the grown capacity")
AFF_LIMIT = AFF_FACTOR * PA_MAX_ROWS

VF_NETWORK, VF_NO_TRANSIT, VF_NO_EXPAND = synth.VF_NETWORK, synth.VF_NO_TRANSIT, synth.VF_NO_EXPAND
RF_GIANT = _constexpr("spf_kernels.hip.h", "RF_GIANT")
# what hspf_graph_export(HSPF_GX_BUILD_MODE) reports, from the expression that computes it
MODE_COST, MODE_INCREMENTAL, MODE_HUB, MODE_REBUILD = _find(
    "spf_capi.hip", r"g->costs_only \? (\d+)u : g->patched_in_place \? (\d+)u : g->hub_built \? (\d+)u : (\d+)u", "the build-mode expression")


def kept_in_degree(row_ptr, col, vflags):
    """Kept in-links per vertex, vectorised: the entry u -> t is kept when row t lists u (the two-way check) and u is
    expanded (no VF_NO_EXPAND); parallel entries count each."""
    rp = np.asarray(row_ptr, np.int64)
    c = np.asarray(col, np.int64)
    n = len(rp) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    two = np.isin(c * n + src, src * n + c)
    keep = two & ((np.asarray(vflags)[src] & VF_NO_EXPAND) == 0)
    return np.bincount(c[keep], minlength=n).astype(np.int64)


def splice(row_ptr, col, metric, vs, rows):
    """The CSR with the rows of `vs` (ascending) replaced by `rows` = [(col, metric)]."""
    rp = np.asarray(row_ptr, np.int64)
    lens = np.diff(rp)
    nl = lens.copy()
    vs = np.asarray(vs, np.int64)
    nl[vs] = [len(c) for c, _ in rows]
    nrp = np.zeros(len(rp), np.int64)
    nrp[1:] = np.cumsum(nl)
    old_keep = np.ones(int(rp[-1]), bool)
    new_keep = np.ones(int(nrp[-1]), bool)
    for v in vs.tolist():
        old_keep[rp[v]:rp[v + 1]] = False
        new_keep[nrp[v]:nrp[v + 1]] = False
    ncol = np.empty(int(nrp[-1]), np.uint32)
    nmet = np.empty(int(nrp[-1]), np.uint32)
    ncol[new_keep] = np.asarray(col)[old_keep]
    nmet[new_keep] = np.asarray(metric)[old_keep]
    for v, (c, m) in zip(vs.tolist(), rows):
        ncol[nrp[v]:nrp[v + 1]] = c
        nmet[nrp[v]:nrp[v + 1]] = m
    return nrp.astype(np.uint32), ncol, nmet


@dataclass
class Patch:
    vs: np.ndarray                 # replaced rows, ascending
    rows: list                     # [(col u32, metric u32)]
    flags: np.ndarray              # u8 per replaced row

    def __post_init__(self):
        self.vs = np.asarray(self.vs, np.uint32)
        self.rows = [(np.asarray(c, np.uint32), np.asarray(m, np.uint32)) for c, m in self.rows]
        self.flags = np.asarray(self.flags, np.uint8)
        assert len(self.vs) == len(self.rows) == len(self.flags) and (np.diff(self.vs.astype(np.int64)) > 0).all()


@dataclass
class Decision:
    path: str                      # the HOST's choice: "cost", "incremental" or "rebuild"
    device_fallback: bool          # the host chose "incremental" and an affected row outgrows the staging area on the device
    build_mode: int                # what hspf_graph_export(BUILD_MODE) reports afterwards
    affected: np.ndarray           # the complete affected set: replaced rows, all their old targets, all their new targets
    pre_dedup: int                 # m + de + sum of the old lengths
    tw_work: int
    tw_bound: int
    e_new: int
    max_old_len: int
    max_new_len: int
    grown: bool
    max_in_deg_before: int
    max_in_deg_after: int
    why: str = ""                  # the first condition that sent the patch to the rebuild

    @property
    def na(self):
        return len(self.affected)


def legacy_affected(row_ptr, col, patch):
    """What the collection loop gathered before it was completed (it stopped adding old rows once the list held more than
    AFF_LIMIT entries, and the path was chosen from the deduplicated remainder): (the set, the row at which it stopped or None)."""
    rp = np.asarray(row_ptr, np.int64)
    parts = [patch.vs.astype(np.int64)] + [c.astype(np.int64) for c, _ in patch.rows]
    size = sum(len(p) for p in parts)
    stop = None
    for j, v in enumerate(patch.vs.tolist()):
        if size > AFF_LIMIT:
            stop = j
            break
        parts.append(np.asarray(col[rp[v]:rp[v + 1]], np.int64))
        size += int(rp[v + 1] - rp[v])
    return np.unique(np.concatenate(parts)), stop


class GraphModel:
    """The state graph_patch_impl decides from, kept alongside a CSR: link capacity, hub mode of the last build, kept
    in-degrees (from the CSR itself: every path leaves them as a fresh build has them)."""

    def __init__(self, row_ptr, col, metric, vflags, *, hub_deg=HUB_DEG, tw_host_max=None, patch_full=False):
        self.row_ptr = np.asarray(row_ptr, np.uint32)
        self.col = np.asarray(col, np.uint32)
        self.metric = np.asarray(metric, np.uint32)
        self.vflags = np.asarray(vflags, np.uint8).copy()
        self.hub_deg, self.tw_host_max, self.patch_full = hub_deg, tw_host_max, patch_full
        e = len(self.col)
        self.cap_e = e + max(e // CAP_UP_DIV, CAP_UP_MIN)
        self.kin = kept_in_degree(self.row_ptr, self.col, self.vflags)
        self.hub_built = self.max_out > hub_deg or self.max_in_deg > hub_deg

    n = property(lambda self: len(self.row_ptr) - 1)
    max_out = property(lambda self: int(np.diff(self.row_ptr.astype(np.int64)).max(initial=0)))
    max_in_deg = property(lambda self: int(self.kin.max(initial=0)))
    n_giant = property(lambda self: int((self.kin > GIANT_DEG).sum()))
    e_kept = property(lambda self: int(self.kin.sum()))

    def step(self, patch: Patch, commit=True) -> Decision:
        rp = self.row_ptr.astype(np.int64)
        rlen = np.diff(rp)
        vs = patch.vs.astype(np.int64)
        m = len(vs)
        old_cols = [self.col[rp[v]:rp[v + 1]] for v in vs.tolist()]
        new_cols = [c for c, _ in patch.rows]
        cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)      # noqa: E731
        oc, nc = cat(old_cols), cat(new_cols)
        de = len(nc)
        assert de == 0 or int(nc.max()) < self.n
        e_new = len(self.col) + de - len(oc)
        max_old_len = max((len(c) for c in old_cols), default=0)
        max_new_len = max((len(c) for c in new_cols), default=0)
        affected = np.unique(np.concatenate([vs, oc, nc]))
        pre_dedup = m + de + len(oc)
        tw_work = int((rlen[nc] + 1).sum() + (rlen[oc] + 1).sum() + 2 * de)
        tw_bound = max(TW_MIN, e_new // TW_DIV) if self.tw_host_max is None else self.tw_host_max
        clean = self.max_in_deg <= GIANT_DEG and self.n_giant == 0
        same = clean and all(len(o) == len(c) and np.array_equal(o, c) for o, c in zip(old_cols, new_cols)) and \
            np.array_equal(self.vflags[vs], patch.flags)
        nrp, ncol, nmet = splice(self.row_ptr, self.col, self.metric, vs, patch.rows)
        nvf = self.vflags.copy()
        nvf[vs] = patch.flags
        kin_new = self.kin if same else kept_in_degree(nrp, ncol, nvf)
        max_out_new = int(np.diff(nrp.astype(np.int64)).max(initial=0))
        grown = e_new > self.cap_e
        why = ""
        if same:
            path = "cost"
        else:
            conds = [(not self.patch_full, "HSPF_PATCH_FULL"), (tw_work <= tw_bound, "tw_work > bound"), (not grown, "arena growth"),
                     (self.max_in_deg <= PA_IN_STRIDE, "max_in_deg > PA_IN_STRIDE"), (self.n_giant == 0, "giant rows"),
                     (not self.hub_built, "hub build"), (max(self.max_out, max_new_len) <= min(self.hub_deg, PA_OUT_STRIDE), "row > PA_OUT_STRIDE"),
                     ((self.n + 15) // 16 <= GB_UNITS_MAX_CHUNKS, "too many chunks"), (self.e_kept != 0, "no kept links"),
                     (len(affected) <= PA_MAX_ROWS, "affected rows > PA_MAX_ROWS")]
            why = next((w for ok, w in conds if not ok), "")
            path = "rebuild" if why else "incremental"
        fallback = path == "incremental" and int(kin_new[affected].max(initial=0)) > PA_IN_STRIDE
        if path == "cost":
            mode = MODE_COST
        elif path == "incremental" and not fallback:
            mode = MODE_INCREMENTAL
        else:
            mode = MODE_HUB if (max_out_new > self.hub_deg or int(kin_new.max(initial=0)) > self.hub_deg) else MODE_REBUILD
        d = Decision(path, fallback, mode, affected, pre_dedup, tw_work, tw_bound, e_new, max_old_len, max_new_len, grown,
                     self.max_in_deg, int(kin_new.max(initial=0)), why)
        if commit:
            if grown:
                self.cap_e = e_new + max(e_new // CAP_GROW_DIV, CAP_GROW_MIN)
            if mode == MODE_INCREMENTAL:
                self.hub_built = False
            elif mode != MODE_COST:
                self.hub_built = mode == MODE_HUB
            self.row_ptr, self.col, self.metric, self.vflags, self.kin = nrp, ncol, nmet, nvf, kin_new
        return d


# ---------------------------------------------------------------------------------------------------------------- cases

@dataclass
class Step:
    tag: str
    patch: Patch
    claim: dict                    # what the generator was built to hit (checked against the model by the CPU suite)
    model: Decision = None         # the model's word in the default configuration


@dataclass
class Case:
    name: str
    graph: synth.CsrGraph
    steps: list
    roots: np.ndarray
    returns: bool                  # the last step restores the graph the case started from
    small: bool                    # small enough for tests/_layout_ref.layout
    notes: dict = field(default_factory=dict)


def replay(case, **kw):
    """The model's decisions for the steps of a case, in another configuration if asked (patch_full=True, tw_host_max=..)."""
    g = case.graph
    mdl = GraphModel(g.row_ptr, g.col, g.metric, g.vflags, **kw)
    return [mdl.step(s.patch) for s in case.steps]


def _finish(case):
    for s, d in zip(case.steps, replay(case)):
        s.model = d
    return case


def _row(g, v):
    a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
    return g.col[a:b].copy(), g.metric[a:b].copy()


_EMPTY = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
_isis = None


def isis_100k():
    global _isis
    if _isis is None:
        _isis = synth.isis_100k()
    return _isis


# ---- (a) the ladder of affected rows at full size

LADDER = (PA_LDS_ROWS, PA_LDS_ROWS + 1, PA_LDS_ROWS + 2, PA_MAX_ROWS - 1, PA_MAX_ROWS, PA_MAX_ROWS + 1)


def ladder_case(na):
    """isis-100k: routers purged (rows emptied) and returned, chosen so that the purged routers and their neighbours are
    exactly `na` vertices: far-apart routers first (each brings its whole neighbourhood), then routers next to the ones
    already taken, whose neighbourhoods overlap, for the remainder."""
    g = isis_100k()
    rp, col, n = g.row_ptr.astype(np.int64), g.col.astype(np.int64), g.n
    nb = lambda v: col[rp[v]:rp[v + 1]].tolist()      # noqa: E731
    # candidates spread over the graph, (1009 + 523 i) mod n, whose closed neighbourhoods share no vertex: each brings its
    # degree + 1 vertices whichever of the others are taken
    reserved, cands = set(), []
    i = 0
    while sum(sz for _, sz in cands) < na + 1200:
        v = (1009 + 523 * i) % n
        i += 1
        hood = {v} | set(nb(v))
        if not (hood & reserved):
            reserved |= hood
            cands.append((v, len(hood)))
    purged, have, k = [], 0, 0
    while na - have - cands[k][1] >= 60:                 # the bulk in order ..
        purged.append(cands[k][0])
        have += cands[k][1]
        k += 1
    reach = {0: []}                                      # .. and the remainder trimmed: a subset of the next ones that adds up exactly
    for v, sz in cands[k:]:
        for tot, sub in sorted(reach.items(), reverse=True):
            if tot + sz <= na - have and tot + sz not in reach:
                reach[tot + sz] = sub + [v]
    if na - have not in reach:
        raise RuntimeError(f"ladder_case({na}): no subset of the candidates adds exactly {na - have} vertices")
    purged += reach[na - have]
    vs = np.array(sorted(purged), np.uint32)
    flags = g.vflags[vs].copy()
    expect = "incremental" if na <= PA_MAX_ROWS else "rebuild"
    claim = {"na": na, "path": expect, "pre_dedup_side": "le"}
    steps = [Step("purge", Patch(vs, [_EMPTY] * len(vs), flags), dict(claim)),
             Step("return", Patch(vs, [_row(g, int(v)) for v in vs], flags), dict(claim))]
    purged.sort()
    left = purged[0]
    roots = np.array([purged[0], purged[-1], nb(left)[0], nb(purged[-1])[-1], 0, 31250, 62500, n - 1], np.uint32)
    return _finish(Case(f"ladder-{na}", g, steps, np.unique(roots), True, False, {"purged": len(purged)}))


# ---- (b) more old targets than the list holds before it is deduplicated

CLUSTERS = {
    # name: routers, links per router, dead stubs, live stubs, routers into the live stubs (the LAST ones), extra links of the last router
    "purge-1000x18": dict(R=1000, deg=18, n_dead=500, n_live=150, RL=145, extra=0),
    "exact-limit": dict(R=862, deg=18, n_dead=500, n_live=150, RL=145, extra=AFF_LIMIT - 862 * 19),
    "limit-plus-1": dict(R=862, deg=18, n_dead=500, n_live=150, RL=145, extra=AFF_LIMIT + 1 - 862 * 19),
    "also-new-target": dict(R=1000, deg=18, n_dead=500, n_live=150, RL=145, extra=0, new_first=10),
    "duplicates-100x200": dict(R=100, deg=200, n_dead=200, n_live=20, RL=10, extra=0),
}


def cluster_case(name):
    """isis-100k with a cluster beside it: R routers of `deg` links each; the first R - RL list one-way dead stubs (empty
    rows), the last RL list live stubs, each of which lists one of them back (two-way links, kept in both directions).  The
    patch empties all R routers: every stub is an old target; the live ones are old targets of the LAST rows only."""
    p = dict(CLUSTERS[name])
    R, deg, n_dead, n_live, RL, extra, new_first = p["R"], p["deg"], p["n_dead"], p["n_live"], p["RL"], p["extra"], p.get("new_first", 0)
    g0 = isis_100k()
    n0 = g0.n
    r0, d0, l0 = n0, n0 + R, n0 + R + n_dead
    n = l0 + n_live
    src, dst, met = [], [], []
    for i in range(R - RL):
        for k in range(deg):
            src.append(r0 + i); dst.append(d0 + (i * deg + k) % n_dead); met.append(1 + (i + k) % 7)
    lists = {}                                             # live stub -> the first router that lists it
    for q in range(RL):
        i = R - RL + q
        for k in range(deg + (extra if q == RL - 1 else 0)):
            s = l0 + (q * deg + k) % n_live
            src.append(r0 + i); dst.append(s); met.append(1 + (i + k) % 7)
            lists.setdefault(s, r0 + i)
    assert len(lists) == n_live
    for s in sorted(lists):
        src.append(s); dst.append(lists[s]); met.append(3)
    rp2, col2, met2 = synth._csr_from_links(n, np.array(src, np.int64), np.array(dst, np.int64), np.array(met, np.int64))
    row_ptr = np.concatenate([g0.row_ptr[:-1], (rp2[n0:].astype(np.int64) + g0.e).astype(np.uint32)])
    g = synth.CsrGraph(row_ptr, np.concatenate([g0.col, col2]), np.concatenate([g0.metric, met2]), np.zeros(n, np.uint8),
                       g0.max_path_metric, "isis-100k+" + name, {})
    vs = np.arange(r0, r0 + R, dtype=np.uint32)
    purge = [_EMPTY] * R
    if new_first:                                          # the first router's new row lists live stubs (one-way): new targets
        purge = [(np.arange(l0, l0 + new_first, dtype=np.uint32), np.full(new_first, 5, np.uint32))] + purge[1:]
    flags = np.zeros(R, np.uint8)
    total = R + new_first + R * deg + extra
    na = R + n_dead + n_live
    claim = {"na": na, "path": "incremental", "pre_dedup": total, "pre_dedup_side": "le" if total <= AFF_LIMIT else "gt"}
    steps = [Step("purge", Patch(vs, purge, flags), claim),
             Step("return", Patch(vs, [_row(g, int(v)) for v in vs], flags), {"pre_dedup": R + R * deg + extra + new_first})]
    live = sorted(lists)
    roots = np.array([live[0], live[-1], lists[live[0]], lists[live[-1]], r0 + R - 1, r0, d0, 0, 50000], np.uint32)
    return _finish(Case("cluster-" + name, g, steps, np.unique(roots), True, False,
                        {"live_stubs": np.array(live, np.int64), "live_routers": np.array(sorted(set(lists.values())), np.int64)}))


# ---- (c), (d) the staging strides and a chain of path changes, on one small graph

def stride_graph():
    """200 routers and 6 LANs (synth.random_lsdb) and, appended: a router H with 520 spokes that all list it (it lists a
    few of them; the spokes from 250 on are not expanded, so H keeps at most 250 of them as in-links however many it lists),
    and a LAN P of 260 members in a ring: P lists all of them, the first PA_IN_STRIDE - 1 list it back."""
    b = synth.random_lsdb(200, 6, 3.0, 909, metric_hi=6)
    nb_ = b.n
    src = np.repeat(np.arange(nb_, dtype=np.int64), np.diff(b.row_ptr.astype(np.int64))).tolist()
    dst, met = b.col.astype(np.int64).tolist(), b.metric.astype(np.int64).tolist()
    H, S0, n_sp = nb_, nb_ + 1, 520
    P, M0, n_mem = S0 + n_sp, S0 + n_sp + 1, 260
    n = M0 + n_mem
    b0, b1 = 20, 40                                        # routers of the base graph the two parts hang on

    def add(u, v, w):
        src.append(u); dst.append(v); met.append(w)

    add(H, b0, 4); add(b0, H, 4)
    for k in range(n_sp):
        add(S0 + k, H, 2)
        if k < 5:
            add(H, S0 + k, 1 + k % 5)
    for k in range(n_mem):
        add(P, M0 + k, 0)
        add(M0 + k, M0 + (k + 1) % n_mem, 3); add(M0 + k, M0 + (k - 1) % n_mem, 3)
        if k < PA_IN_STRIDE - 1:
            add(M0 + k, P, 10)
    add(M0, b1, 5); add(b1, M0, 5)
    row_ptr, col, metric = synth._csr_from_links(n, np.array(src, np.int64), np.array(dst, np.int64), np.array(met, np.int64))
    vflags = np.concatenate([b.vflags, np.zeros(n - nb_, np.uint8)])
    vflags[S0 + 250:S0 + n_sp] |= VF_NO_EXPAND
    vflags[P] |= VF_NETWORK
    meta = {"H": H, "S0": S0, "P": P, "M0": M0, "b0": b0, "b1": b1, "n_networks": 6, "n_base": nb_}
    return synth.CsrGraph(row_ptr, col, metric, vflags, b.max_path_metric, "strides", meta)


def _stride_roots(g):
    m = g.meta
    return np.unique(np.array([m["b0"], m["b1"], m["H"], m["S0"], m["S0"] + 3, m["S0"] + 300, m["S0"] + 519, m["M0"], m["M0"] + 1,
                               m["M0"] + 100, m["M0"] + PA_IN_STRIDE - 1, m["M0"] + PA_IN_STRIDE, m["M0"] + PA_IN_STRIDE + 1] +
                              list(range(6, 30)), np.uint32))


def _hub_row(g, k):
    """H's row with exactly k links: the base router and the first k - 1 spokes."""
    m = g.meta
    c = np.concatenate([[m["b0"]], np.arange(m["S0"], m["S0"] + k - 1)]).astype(np.uint32)
    return c, (1 + np.arange(k) % 5).astype(np.uint32)


def _member_row(g, k, joined):
    m = g.meta
    M0, n_mem = m["M0"], 260
    c = [M0 + (k + 1) % n_mem, M0 + (k - 1) % n_mem] + ([m["P"]] if joined else [])
    return np.array(c, np.uint32), np.array([3, 3, 10][:len(c)], np.uint32)


def row_stride_case(k):
    """H's row replaced by one of k links (PA_OUT_STRIDE - 1, PA_OUT_STRIDE: incremental, 512 kept out-links staged by 256
    threads; PA_OUT_STRIDE + 1: the host rebuilds, in hub mode), and back."""
    g = stride_graph()
    H = g.meta["H"]
    fits = k <= min(PA_OUT_STRIDE, HUB_DEG)
    fl = g.vflags[[H]]
    steps = [Step(f"row of {k}", Patch([H], [_hub_row(g, k)], fl), {"path": "incremental" if fits else "rebuild", "max_new_len": k, "na": k + 1}),
             Step("back", Patch([H], [_row(g, H)], fl), {"path": "incremental" if fits else "rebuild", "max_old_len": k})]
    return _finish(Case(f"row-{k}", g, steps, _stride_roots(g), True, True))


def lan_stride_case():
    """P's kept in-row 255 -> 256 (incremental: the staging area exactly full), 256 -> 257 (the host still says incremental,
    kb_pa_rows raises GB_ERR_PATCH and the host rebuilds from the raw CSR), 257 -> 256 (a giant row: the host rebuilds), 256 -> 255."""
    g = stride_graph()
    M0 = g.meta["M0"]
    a, b = M0 + PA_IN_STRIDE - 1, M0 + PA_IN_STRIDE
    z = np.zeros(1, np.uint8)
    steps = [Step("in-row 255 -> 256", Patch([a], [_member_row(g, a - M0, True)], z), {"path": "incremental", "fallback": False, "in_after": PA_IN_STRIDE}),
             Step("in-row 256 -> 257", Patch([b], [_member_row(g, b - M0, True)], z), {"path": "incremental", "fallback": True, "in_after": PA_IN_STRIDE + 1}),
             Step("in-row 257 -> 256", Patch([b], [_member_row(g, b - M0, False)], z), {"path": "rebuild", "in_after": PA_IN_STRIDE}),
             Step("in-row 256 -> 255", Patch([a], [_member_row(g, a - M0, False)], z), {"path": "incremental", "fallback": False, "in_after": PA_IN_STRIDE - 1})]
    return _finish(Case("lan-in-row", g, steps, _stride_roots(g), True, True))


def chain_case():
    """Path changes in a chain on one graph.  Between the device fallback and the next incremental patch stands one more
    step than the bare sequence "incremental, fallback, incremental, .." names: the fallback leaves a giant row (257 kept
    in-links), and while the graph has one the host takes the rebuild — so the row shrinks first, through the rebuild."""
    g = stride_graph()
    m = g.meta
    M0, H, S0, nb_ = m["M0"], m["H"], m["S0"], m["n_base"]
    a, b = M0 + PA_IN_STRIDE - 1, M0 + PA_IN_STRIDE
    z = np.zeros(1, np.uint8)
    steps = [Step("incremental: in-row 255 -> 256", Patch([a], [_member_row(g, a - M0, True)], z), {"path": "incremental", "fallback": False}),
             Step("device fallback: in-row 256 -> 257", Patch([b], [_member_row(g, b - M0, True)], z), {"path": "incremental", "fallback": True}),
             Step("host rebuild: the giant row shrinks", Patch([b], [_member_row(g, b - M0, False)], z), {"path": "rebuild"}),
             Step("incremental: in-row 256 -> 255", Patch([a], [_member_row(g, a - M0, False)], z), {"path": "incremental", "fallback": False})]
    vs = np.arange(30, 36)
    steps.append(Step("cost-only", Patch(vs, [(_row(g, v)[0], _row(g, v)[1] + 2) for v in vs], g.vflags[vs]), {"path": "cost"}))
    vs = np.arange(6, nb_)                                 # every router of the base graph lists its links in reverse order
    steps.append(Step("host rebuild: work bound", Patch(vs, [tuple(x[::-1].copy() for x in _row(g, v)) for v in vs], g.vflags[vs]), {"path": "rebuild"}))
    steps.append(Step("incremental: row of 512", Patch([H], [_hub_row(g, PA_OUT_STRIDE)], g.vflags[[H]]), {"path": "incremental", "fallback": False}))
    # two members that never joined the LAN list 270 spokes each besides their ring neighbours, one-way: more links than the
    # arena has room for, and few enough row entries that arena growth is the ONLY reason for the rebuild
    vs = np.array([M0 + 257, M0 + 258])
    grow = [(np.concatenate([_member_row(g, int(v) - M0, False)[0], np.arange(S0 + 100 * i, S0 + 100 * i + 270)]).astype(np.uint32),
             np.full(272, 2, np.uint32)) for i, v in enumerate(vs)]
    steps.append(Step("arena growth", Patch(vs, grow, g.vflags[vs]), {"path": "rebuild", "grown": True}))
    steps.append(Step("incremental: the row returns", Patch([H], [_row(g, H)], g.vflags[[H]]), {"path": "incremental", "fallback": False}))
    return _finish(Case("chain", g, steps, _stride_roots(g), False, True))


# ---- (e) seeded random multi-row patches at full size

RANDOM_SEED = 5
RANDOM_ROUNDS = 8


def random_case(seed=RANDOM_SEED):
    """Eight rounds of 10 to 150 replaced rows on isis-100k (links dropped, added, re-costed, re-ordered, rows emptied, flags
    flipped), each on top of the last, and a ninth patch that returns every touched row."""
    g = isis_100k()
    rng = np.random.default_rng(seed)
    mdl = GraphModel(g.row_ptr, g.col, g.metric, g.vflags)
    steps, touched = [], set()
    for rnd in range(RANDOM_ROUNDS):
        k = int(rng.integers(10, 151))
        vs = np.sort(rng.choice(g.n, size=k, replace=False))
        rows, flags = [], []
        rp = mdl.row_ptr.astype(np.int64)
        for v in vs.tolist():
            c, w = mdl.col[rp[v]:rp[v + 1]].copy(), mdl.metric[rp[v]:rp[v + 1]].copy()
            if rng.random() < 0.1:
                c, w = c[:0], w[:0]
            keep = rng.random(len(c)) > 0.3
            c, w = c[keep], w[keep]
            w = np.where(rng.random(len(w)) < 0.5, rng.integers(1, 101, len(w)), w).astype(np.uint32)
            extra = int(rng.integers(0, 4))
            c = np.concatenate([c, rng.integers(0, g.n, extra).astype(np.uint32)])
            w = np.concatenate([w, rng.integers(1, 101, extra).astype(np.uint32)])
            p = rng.permutation(len(c))
            rows.append((c[p], w[p]))
            f = int(mdl.vflags[v])
            if rng.random() < 0.3:
                f ^= VF_NO_TRANSIT
            if rng.random() < 0.2:
                f ^= VF_NO_EXPAND
            flags.append(f)
        patch = Patch(vs, rows, np.array(flags, np.uint8))
        mdl.step(patch)
        touched.update(vs.tolist())
        steps.append(Step(f"round {rnd}: {k} rows", patch, {}))
    vs = np.array(sorted(touched), np.uint32)
    steps.append(Step("all rows return", Patch(vs, [_row(g, int(v)) for v in vs], g.vflags[vs]), {}))
    first, last = steps[0].patch, steps[RANDOM_ROUNDS - 1].patch
    roots = np.array([first.vs[0], first.vs[-1], last.vs[0], last.vs[-1], first.rows[1][0][0] if len(first.rows[1][0]) else 1, 0, 50000, g.n - 1], np.uint32)
    return _finish(Case(f"random-{seed}", g, steps, np.unique(roots), True, False))


def all_cases():
    for na in LADDER:
        yield ladder_case(na)
    for name in CLUSTERS:
        yield cluster_case(name)
    for k in (PA_OUT_STRIDE - 1, PA_OUT_STRIDE, PA_OUT_STRIDE + 1):
        yield row_stride_case(k)
    yield lan_stride_case()
    yield chain_case()
    yield random_case()
