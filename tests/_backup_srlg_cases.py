"""The graphs, group tables, prefix tables and model-side plumbing the per-prefix SRLG backup tests share
(tests/test_host_backup_srlg.py, tests/test_gpu_backup_srlg.py, tests/test_gpu_backup_srlg_random.py, tests/test_cpp_backup_srlg.py).
Plain numpy over the CPU oracle, no GPU import.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_cases as C
import _backup_model as B
import _backup_srlg_model as BS
import _lfa_model as M
import _rlfa_model as R
import _srlg_model as SM
import _tilfa_model as T

MAXP = 0xFFFFFFFF


class Model:
    """The model's side of some protected roots over ONE table set — the rows of the batch of hspf_lfa_srlg_device: per protected
    root [S] ++ neighbour routers ++ member endpoints, joined in order of first appearance — and ONE prefix table."""

    def __init__(self, graph, prot, gp, gr, table: B.Table, maxp=MAXP, run_flags=0, w_min=1, no_members=False):
        from oracle import graph_oracle as go
        self.graph, self.prot, self.gp, self.gr, self.table = graph, tuple(int(r) for r in prot), gp, gr, table
        self.maxp, self.run_flags = maxp, run_flags
        per, rows = [], []
        for s in self.prot:
            c, rs, _, mem = SM.protect_one(*graph, s, gp, gr)
            per.append((c, mem))
            rows += [int(x) for x in rs if int(x) not in rows]
        row_of = {v: i for i, v in enumerate(rows)}
        self.roots = np.array(rows, np.uint32)
        self.cands = [c for c, _ in per]
        self.root_row = [row_of[c.root] for c in self.cands]
        self.nbr_row = [np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32) for c in self.cands]
        self.mems = []
        for c, mem in per:
            if no_members:
                mem = SM.empty_members(len(c.nbr))
            else:
                mem.tail_row = np.array([row_of[int(x)] for x in mem.tail], np.uint32)
                mem.head_row = np.array([row_of[int(x)] for x in mem.head], np.uint32)
            self.mems.append(mem)
        self.W = max(go.mask_words(*graph, self.roots), max((len(c.nbr) + 63) // 64 for c in self.cands), w_min)
        self.fwd, self.rdist = R.tables(graph, maxp, self.roots, run_flags, self.W)
        self._frr, self._want = {}, {}

    def routes(self, i=0, table=None):
        f = self.fwd
        return B.routes(f.dist, f.flags, f.mask, self.root_row[i], table or self.table)

    def frr(self, lfa_flags=0):
        """[(SRLG LFA, SRLG RLFA, TI-LFA on the safe tables)] of the protected roots."""
        lf_ = lfa_flags & ~BS.SAFE_REPAIRS
        if lf_ not in self._frr:
            f, out = self.fwd, []
            for c, rr, nr, mem in zip(self.cands, self.root_row, self.nbr_row, self.mems):
                lf = SM.lfa(f.dist, f.flags, f.mask, c, rr, nr, mem, lf_)
                r = SM.rlfa(f.dist, f.flags, f.mask, self.rdist, self.graph[3], c, rr, nr, mem, lf_, lf.alt_flags)
                out.append((lf, r, T.tilfa(f.dist, f.flags, f.mask, self.rdist, self.graph, c, rr, nr, r.space_flags, r.space_via, lf.alt_flags)))
            self._frr[lf_] = out
        return self._frr[lf_]

    def want(self, lfa_flags=0, remote=True, table=None, tilfa=None):
        """[SRLG backup model] of the protected roots; tilfa: [TI-LFA tables per root] in place of the chain's."""
        key = (lfa_flags, remote, id(table), id(tilfa))
        if key not in self._want:
            f, t = self.fwd, table or self.table
            ti = tilfa if tilfa is not None else [x[2] for x in self.frr(lfa_flags)] if remote else [None] * len(self.prot)
            self._want[key] = [BS.backup(f.dist, f.flags, f.mask, c, rr, nr, mem, t, self.routes(i, t), lfa_flags, ti[i])
                               for i, (c, rr, nr, mem) in enumerate(zip(self.cands, self.root_row, self.nbr_row, self.mems))]
        return self._want[key]

    def slot(self, v, i=0):
        return int(np.flatnonzero(self.cands[i].nbr == v)[0])


def group(graph, *links, gid=5):
    """(grp_ptr, grp) with the given (u, v[, nth]) links in ONE group."""
    return SM.groups_csr(len(graph[1]), {SM.link_pos(graph, *l): [gid] for l in links})


# ---------------------------------------------------------------------------------------------------- the hand-checked case

def ring_graph():
    """The 6-ring of unit costs with the chords 0 - 3 (cost 2) and 1 - 4 (cost 1) of tests/test_gpu_srlg.py; S = 0."""
    ring = [(v, (v + 1) % 6, 1) for v in range(6)]
    return M.csr(6, M.both(ring + [(0, 3, 2), (1, 4, 1)]))


def ring():
    """(graph, S, (grp_ptr, grp), Table).  Link 3 -> 2 shares the group of 0 -> 1.
    prefix v (v = 0 .. 5): router v alone at metric 0 — the per-vertex answers of hspf_lfa_srlg_device.
    prefix 6: routers 2 (metric 0) and 3 (metric 3).  S reaches it through 1 at cost 2; the chord's neighbour 3 has
              d_3(p) = min(1 + 0, 0 + 3) = 1 < d(3, 0) + 2, by 3 -> 2: the member.  Refused, nothing else: BK_NONE / the repair.
    prefix 7: routers 2 (metric 5) and 3 (metric 0).  S uses the chord (cost 2): the primary has no member."""
    g = ring_graph()
    gp, gr = group(g, (0, 1), (3, 2))
    return g, 0, (gp, gr), B.table([[(v, 0)] for v in range(6)] + [[(2, 0), (3, 3)], [(2, 5), (3, 0)]])


# ------------------------------------------------------------------------------------------------------------ random inputs

def random_groups(graph, seed, n_groups=(1, 7), per_group=(2, 6), root=None):
    """1 .. 6 groups of 2 .. 5 links each drawn anywhere in the graph; with `root`, every group holds one link of the root's row."""
    r = np.random.default_rng(seed)
    rp, col = graph[0], graph[1]
    of = {}
    for gid in range(int(r.integers(*n_groups))):
        links = [int(x) for x in r.choice(len(col), size=min(len(col), int(r.integers(*per_group))), replace=False)]
        if root is not None and rp[root + 1] > rp[root]:
            links.append(int(r.integers(int(rp[root]), int(rp[root + 1]))))
        for l in links:
            if gid + 100 not in of.setdefault(l, []):
                of[l].append(gid + 100)
    return SM.groups_csr(len(col), of)


RANDOM_SEED, GPU_GRAPHS = 9100, 40


def random_case(seed):
    """(graph, S, (grp_ptr, grp), Table): the sweep graphs of tests/_backup_cases.py (8 - 40 routers, up to two LANs, overloaded
    routers, 1 - 3 advertisers per prefix — a fourth is added to every fifth prefix) with 1 - 6 random groups, each through S's row."""
    g, S, t = C.sweep_case(seed)
    r = np.random.default_rng(seed + 1)
    nr = int(np.count_nonzero(~(g[3] & M.VF_NETWORK).astype(bool)))
    lists = []
    for p in range(min(t.n, 80)):
        e = [(v, m) for v, m, _ in t.entries(p)]
        if p % 5 == 4:
            more = [int(v) for v in range(nr) if v not in {x for x, _ in e}]
            e += [(int(v), int(r.integers(0, 16))) for v in r.choice(more, size=min(len(more), 4 - len(e)), replace=False)]
        lists.append(e)
    return g, S, random_groups(g, seed, root=S), B.table(lists)


def tally(wants):
    """How many prefixes of each class the non-vacuity conditions name, over a list of model results."""
    keys = ("refused_other", "refused_none", "pair_refused", "ecmp_one_sided", "flag_matters")
    return {k: sum(len(getattr(w, k)) for w in wants) for k in keys}
