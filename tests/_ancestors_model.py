"""Plain reference of hspf_ancestors_device (include/holo_spf_hip.h): the parent DAG as the reference builds `Vertex.parents`
(holo-isis/src/spf.rs:637-706), the level-L routers, and Spt::is_on_path (spf.rs:261-286) as a stack DFS over every parent.
TEST INFRASTRUCTURE ONLY.

The parent DAG is defined from the oracle's tables (oracle.graph_oracle.run: dist, hops, in-SPT flags and the TRUE pop order),
not the way the kernel shortcuts it.  Link u -> v (position k of row u) is a parent link iff
  - the library keeps it (header "The LSDB graph ..."): the two-way check passes (row v lists u), u is not VF_NO_EXPAND, and u is
    not an overloaded router other than the root unless the run ignores the overload bit (spf.rs:557-574; the reference gates on
    `hops != 0`, and the root is the only router with hops == 0);
  - both ends are in the SPT;
  - it is tight under the graph's add: min(dist[u] + w, 2^32 - 1) == dist[v] (a sum beyond max_path_metric was never relaxed and
    cannot equal a distance of the SPT);
  - pop_rank[u] < pop_rank[v]: u was expanded while v was still a candidate.
Every such link is one entry of `parents` (parallel links count once each), so len(parents[v]) == OracleResult.n_parents.
Nothing here knows about "w > 0 or u < v" or the one-parent rule of hop-count graphs: k_anc_sweep's shortcuts are what the tests
test."""
from dataclasses import dataclass, field

import numpy as np

from oracle import graph_oracle as go

VF_NETWORK, VF_NO_TRANSIT, VF_NO_EXPAND = 1, 2, 4
RUN_IGNORE_OVERLOAD = 2
INF = 0xFFFFFFFF
NO_ROOT = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF


def two_way(row_ptr, col):
    """[e] bool: the target's row lists the source (holo-isis/src/spf.rs:616-627)."""
    n = len(row_ptr) - 1
    rows = [set(col[row_ptr[u]:row_ptr[u + 1]].tolist()) for u in range(n)]
    tw = np.zeros(len(col), bool)
    for u in range(n):
        for k in range(int(row_ptr[u]), int(row_ptr[u + 1])):
            tw[k] = u in rows[int(col[k])]
    return tw


def parent_lists(row_ptr, col, metric, vflags, root, run_flags, dist, flags, pop_rank, tw=None):
    """parents[v] = sources of the parent links into v, one entry per link, for one root's oracle row."""
    n = len(row_ptr) - 1
    if tw is None:
        tw = two_way(row_ptr, col)
    parents = [[] for _ in range(n)]
    if root == NO_ROOT:
        return parents
    for u in range(n):
        if not (flags[u] & 1):
            continue
        f = int(vflags[u])
        if f & VF_NO_EXPAND:
            continue
        if (f & VF_NO_TRANSIT) and not (f & VF_NETWORK) and u != root and not (run_flags & RUN_IGNORE_OVERLOAD):
            continue
        du, pu = int(dist[u]), int(pop_rank[u])
        for k in range(int(row_ptr[u]), int(row_ptr[u + 1])):
            v = int(col[k])
            if not tw[k] or not (flags[v] & 1):
                continue
            if min(du + int(metric[k]), U32_MAX) != int(dist[v]):
                continue
            if pu < int(pop_rank[v]):
                parents[v].append(u)
    return parents


def ancestors_of(parents, v):
    """Every vertex a stack DFS from v over all parents reaches, v included (the walk of Spt::is_on_path without its early exit)."""
    seen, stack = set(), [v]
    while stack:
        cur = stack.pop()
        if cur in seen:
            continue
        seen.add(cur)
        stack.extend(parents[cur])
    return seen


@dataclass
class Model:
    level_rank: np.ndarray     # [R, n] u32, INF where the vertex is no level-L router of that root
    level_count: np.ndarray    # [R] u32
    anc: list                  # [R][n] Python ints: bit level_rank[a] set iff a is an ancestor of v, or v itself
    parents: list              # [R][n] lists (shared by every level of one (graph, roots, run_flags))
    ref: go.OracleResult
    _words: dict = field(default_factory=dict)

    def words(self, W):
        """anc as [R, n, W] u64; raises when a set does not fit."""
        if W not in self._words:
            self._words[W] = self._to_words(W)
        return self._words[W]

    def _to_words(self, W):
        R, n = self.level_rank.shape
        out = np.zeros((R, n, W), np.uint64)
        for r in range(R):
            for v in range(n):
                x = self.anc[r][v]
                assert x >> (64 * W) == 0
                q = 0
                while x:
                    out[r, v, q] = x & 0xFFFFFFFFFFFFFFFF
                    x >>= 64
                    q += 1
        return out

    def is_on_path(self, r, a, d):
        """Spt::is_on_path(a, d) in the SPT of root r, for a level-L router a."""
        return bool((self.anc[r][d] >> int(self.level_rank[r, a])) & 1)


class Tables:
    """The oracle's rows, the parent lists and the full ancestor sets of one (graph, roots, run_flags): every level is read off them."""

    def __init__(self, row_ptr, col, metric, vflags, max_path_metric, roots, run_flags):
        self.row_ptr = np.ascontiguousarray(row_ptr, np.uint32)
        self.col = np.ascontiguousarray(col, np.uint32)
        self.metric = np.ascontiguousarray(metric, np.uint32)
        self.vflags = np.ascontiguousarray(vflags, np.uint8)
        self.roots = [int(r) for r in roots]
        self.n = len(self.row_ptr) - 1
        self.ref = go.run(self.row_ptr, self.col, self.metric, self.vflags, max_path_metric, np.asarray(self.roots, np.uint32), run_flags,
                          go.MAP)
        tw = two_way(self.row_ptr, self.col)
        self.parents = [parent_lists(self.row_ptr, self.col, self.metric, self.vflags, root, run_flags, self.ref.dist[r], self.ref.flags[r],
                                     self.ref.pop_rank[r], tw) for r, root in enumerate(self.roots)]
        self._above, self._levels = {}, {}

    def above(self, r):
        """[n] sets: the DFS of every vertex of root r's SPT (empty outside it)."""
        if r not in self._above:
            fl = self.ref.flags[r]
            self._above[r] = [ancestors_of(self.parents[r], v) if fl[v] & 1 else set() for v in range(self.n)]
        return self._above[r]

    def level(self, L) -> Model:
        if L not in self._levels:
            self._levels[L] = self._level(L)
        return self._levels[L]

    def _level(self, L) -> Model:
        R, n = len(self.roots), self.n
        rank = np.full((R, n), INF, np.uint32)
        count = np.zeros(R, np.uint32)
        anc = []
        for r, root in enumerate(self.roots):
            if root == NO_ROOT:
                anc.append([0] * n)
                continue
            fl, hp = self.ref.flags[r], self.ref.hops[r]
            members = [v for v in range(n) if (fl[v] & 1) and not (self.vflags[v] & VF_NETWORK) and int(hp[v]) == L]
            for i, v in enumerate(members):          # ascending vertex index
                rank[r, v] = i
            count[r] = len(members)
            ms = set(members)
            anc.append([sum(1 << int(rank[r, a]) for a in s & ms) for s in self.above(r)])
        return Model(rank, count, anc, self.parents, self.ref)


def model(row_ptr, col, metric, vflags, max_path_metric, roots, run_flags, level) -> Model:
    return Tables(row_ptr, col, metric, vflags, max_path_metric, roots, run_flags).level(level)
