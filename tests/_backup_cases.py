"""The graphs, prefix tables and model-side plumbing the per-prefix backup tests share (tests/test_host_backup.py,
tests/test_gpu_backup.py, tests/test_cpp_backup.py): the two hand-checked cases, the seeded sweep, the augmented graph of the
independent oracle.  Plain numpy over the CPU oracle, no GPU import.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_model as B
import _lfa_model as M
import _rlfa_model as R
import _tilfa_model as T

MAXP = 0xFFFFFFFF


class Model:
    """The model's side of some protected roots over ONE table set (the rows of tests/_frr_chains.py's Protected: the protected
    roots, then the other neighbour routers in ascending order) and ONE prefix table."""

    def __init__(self, graph, prot, table: B.Table, maxp=MAXP, run_flags=0, w_min=1):
        from oracle import graph_oracle as go
        self.graph, self.prot, self.table, self.maxp, self.run_flags = graph, tuple(int(r) for r in prot), table, maxp, run_flags
        self.cands = [M.candidates(*graph, r) for r in self.prot]
        rows = list(self.prot) + sorted({int(x) for c in self.cands for x in c.nbr if x != M.NONE} - set(self.prot))
        self.roots = np.array(rows, np.uint32)
        row_of = {v: i for i, v in enumerate(rows)}
        self.root_row = [row_of[r] for r in self.prot]
        self.nbr_row = [np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32) for c in self.cands]
        self.W = max(go.mask_words(*graph, self.roots), max((len(c.nbr) + 63) // 64 for c in self.cands), w_min)
        self.fwd, self.rdist = R.tables(graph, maxp, self.roots, run_flags, self.W)
        self._frr, self._want = {}, {}

    def routes(self, i=0, table=None):
        f = self.fwd
        return B.routes(f.dist, f.flags, f.mask, self.root_row[i], table or self.table)

    def frr(self, lfa_flags=0):
        """[(LFA, RLFA, TI-LFA model)] of the protected roots (the per-vertex chain of tests/_frr_chains.py)."""
        if lfa_flags not in self._frr:
            f, out = self.fwd, []
            for c, rr, nr in zip(self.cands, self.root_row, self.nbr_row):
                lf = M.lfa(f.dist, f.flags, f.mask, c, rr, nr, lfa_flags)
                r = R.rlfa(f.dist, f.flags, f.mask, self.rdist, self.graph[3], c, rr, nr, lfa_flags, lf.alt_flags)
                out.append((lf, r, T.tilfa(f.dist, f.flags, f.mask, self.rdist, self.graph, c, rr, nr, r.space_flags, r.space_via, lf.alt_flags)))
            self._frr[lfa_flags] = out
        return self._frr[lfa_flags]

    def want(self, lfa_flags=0, remote=True, table=None):
        """[Backup model] of the protected roots."""
        key = (lfa_flags, remote, id(table))
        if key not in self._want:
            f, t = self.fwd, table or self.table
            self._want[key] = [B.backup(f.dist, f.flags, f.mask, c, rr, nr, t, self.routes(i, t), lfa_flags, self.frr(lfa_flags)[i][2] if remote else None)
                               for i, (c, rr, nr) in enumerate(zip(self.cands, self.root_row, self.nbr_row))]
        return self._want[key]

    def slot(self, v, i=0):
        return int(np.flatnonzero(self.cands[i].nbr == v)[0])


# ---------------------------------------------------------------------------------------------------- the hand-checked cases

def square():
    """S = 0; 0-1 costs 2, 0-3 costs 1, 3-2 costs 1, 1-2 costs 5, the diagonal 0-2 costs 3 (row 0: slot 0 -> 1, slot 1 -> 3,
    slot 2 -> 2).  Prefix 0 is advertised by router 1 at metric 1 and by router 2 at metric 2; prefix 1 by router 1 alone at 1."""
    g = M.csr(4, M.both([(0, 1, 2), (0, 3, 1), (3, 2, 1), (1, 2, 5), (0, 2, 3)]))
    return g, 0, B.table([[(1, 1), (2, 2)], [(1, 1)]])


def five_ring_graph():
    """0-1-2-3-4-0 with costs 1, 1, 1, 1 and 4 on 4-0 (the five-ring of tests/test_host_tilfa.py)."""
    return M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]))


def five_ring():
    """S = 2.  Prefix v (v = 0 .. 4) is advertised by router v alone at metric 10; prefix 5 by router 1 at 2 and router 3 at 1."""
    return five_ring_graph(), 2, B.table([[(v, 10)] for v in range(5)] + [[(1, 2), (3, 1)]])


def triangle():
    """S = 0, router 1 overloaded, every link costs 1.  Prefix 0 = {router 1 at 2, router 2 at 1}, prefix 1 = {router 1 at 3,
    router 2 at 1}."""
    return M.csr(3, M.both([(0, 1, 1), (0, 2, 1), (1, 2, 1)]), no_transit=[1]), 0, B.table([[(1, 2), (2, 1)], [(1, 3), (2, 1)]])


# ------------------------------------------------------------------------------------------------------------ the seeded sweep

SWEEP_SEED = 7000                         # first seed of the sweep; the range was chosen on the CPU (tests/test_host_backup.py, test 5)
HOST_GRAPHS, GPU_GRAPHS = 500, 40


def sweep_case(seed):
    """(graph, S, Table): 8-40 routers on a sparse mesh with asymmetric costs, up to two LANs (pseudonodes appended after the
    routers), some overloaded routers; 1-3 router advertisers per prefix at metrics >= 1, flags 0."""
    r = np.random.default_rng(seed)
    nr = int(r.integers(8, 41))
    n_lan = int(r.integers(0, 3))
    n = nr + n_lan
    und = {(v, int(r.integers(0, v))) for v in range(1, nr)}                       # a random tree: connected
    for _ in range(int(r.integers(nr // 2, nr + nr // 2))):
        a, b = (int(x) for x in r.integers(0, nr, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        c1 = int(r.integers(1, 12))
        c2 = c1 if r.random() < 0.6 else int(r.integers(1, 12))
        links += [(a, b, c1), (b, a, c2)]
    for i in range(n_lan):
        for m in r.choice(nr, size=int(r.integers(2, 5)), replace=False):
            links += [(int(m), nr + i, int(r.integers(1, 8))), (nr + i, int(m), 0)]
    overloaded = [int(v) for v in range(nr) if r.random() < 0.12]
    S = int(r.integers(0, nr))
    g = M.csr(n, links, net=range(nr, n), no_transit=[v for v in overloaded if v != S])
    lists = []
    for _ in range(int(r.integers(nr // 2, 2 * nr))):
        k = int(r.choice([1, 1, 2, 2, 3]))
        adv = r.choice(nr, size=k, replace=False)
        # metrics drawn near the spread of the distances, so that a second advertiser is often the better one for a neighbour
        lists.append([(int(v), int(r.integers(1, 16))) for v in adv])
    return g, S, B.table(lists)


def qualifies(t: B.Table, S, vflags, p):
    """Every advertiser of p is a router other than S that is not overloaded (and there is one): what a vertex X_p behind the
    advertisers can stand for (nothing reaches X_p THROUGH an overloaded router, whose own prefixes stay reachable)."""
    e = t.entries(p)
    return bool(e) and all(v != S and not (vflags[v] & (M.VF_NETWORK | M.VF_NO_TRANSIT)) for v, _, _ in e)


def augmented(graph, S, t: B.Table):
    """(graph', {p: X_p}): every qualifying prefix p gets a router vertex X_p with HSPF_VF_NO_TRANSIT appended after all existing
    vertices and linked two-way to each advertiser v at cost m_v; the links are appended at the END of v's row, so that S's slot
    numbering is unchanged (S advertises no qualifying prefix)."""
    rp, col, met, vf = graph
    n = len(vf)
    links = [(u, int(col[k]), int(met[k])) for u in range(n) for k in range(int(rp[u]), int(rp[u + 1]))]
    xs = {}
    for p in range(t.n):
        if qualifies(t, S, vf, p):
            xs[p] = n + len(xs)
            for v, m, _ in t.entries(p):
                links += [(v, xs[p], m), (xs[p], v, m)]
    g = M.csr(n + len(xs), links)
    g[3][:n] = vf
    g[3][n:] = M.VF_NO_TRANSIT
    return g, xs
