"""Chains of hspf_graph_patch steps under the three fast-reroute calls, model side only: the graphs, the patches, what each
step is meant to change (asserted on the MODEL) and the path the patch model (tests/_patch_model.py) predicts per engine
configuration.  tests/test_gpu_frr_patched.py runs the chains on the device against these models, tests/test_host_tilfa.py
runs the same splices and the same assertions without one.  Also the seeded graphs of the TI-LFA sweep of
tests/test_gpu_tilfa.py.  Plain numpy over the CPU oracle, no GPU import.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _lfa_model as M
import _patch_model as pm
import _rlfa_model as R
import _tilfa_model as T

MAXP = 0xFFFFFFFF
# the patch model's view of the engine configurations of tests/conftest.py (tests/_engines.py: hub_engines)
ENGINES = {"default": {}, "hubsort": {"hub_deg": 0, "tw_host_max": 0}, "patchfull": {"patch_full": True}}


class Protected:
    """The model's side of some protected roots over ONE table set: the rows are the protected roots, then the other
    neighbour routers in ascending order (one root: exactly the rows of tests/test_gpu_rlfa.py's Case)."""

    def __init__(self, graph, prot, maxp=MAXP):
        from oracle import graph_oracle as go
        self.graph, self.prot, self.maxp = graph, tuple(int(r) for r in prot), maxp
        self.cands = [M.candidates(*graph, r) for r in self.prot]
        rows = list(self.prot) + sorted({int(x) for c in self.cands for x in c.nbr if x != M.NONE} - set(self.prot))
        self.roots = np.array(rows, np.uint32)
        row_of = {v: i for i, v in enumerate(rows)}
        self.root_row = [row_of[r] for r in self.prot]
        self.nbr_row = [np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32) for c in self.cands]
        self.W = max(go.mask_words(*graph, self.roots), max((len(c.nbr) + 63) // 64 for c in self.cands), 1)
        self.fwd, self.rdist = R.tables(graph, maxp, self.roots, 0, self.W)
        self._want = {}

    def want(self, lfa_flags=0):
        """[(LFA, RLFA, TI-LFA model)] of the protected roots, the later ones fed by the alt_flags of the first."""
        if lfa_flags not in self._want:
            out = []
            f = self.fwd
            for c, rr, nr in zip(self.cands, self.root_row, self.nbr_row):
                lf = M.lfa(f.dist, f.flags, f.mask, c, rr, nr, lfa_flags)
                r = R.rlfa(f.dist, f.flags, f.mask, self.rdist, self.graph[3], c, rr, nr, lfa_flags, lf.alt_flags)
                t = T.tilfa(f.dist, f.flags, f.mask, self.rdist, self.graph, c, rr, nr, r.space_flags, r.space_via, lf.alt_flags)
                out.append((lf, r, t))
            self._want[lfa_flags] = out
        return self._want[lfa_flags]

    def slot(self, v, i=0):
        return int(np.flatnonzero(self.cands[i].nbr == v)[0])

    def slots(self, i=0):
        return np.flatnonzero(self.cands[i].nbr != M.NONE)

    def repairs(self, e, i=0, lfa_flags=0):
        r = self.want(lfa_flags)[i][1]
        return T.repairs(self.fwd.dist, self.rdist, self.graph, self.cands[i], self.root_row[i], self.nbr_row[i], e, r.space_flags[e], r.space_via[e])

    def pairs(self, e, i=0, lfa_flags=0):
        return {(p, q) for _, kind, p, q, _ in self.repairs(e, i, lfa_flags) if kind == T.KIND_PAIR}

    def winner(self, e, i=0, lfa_flags=0):
        t = self.want(lfa_flags)[i][2]
        return int(t.ti_kind[e]), int(t.ti_p[e]), int(t.ti_q[e])

    def winners(self, i=0):
        return [self.winner(int(e), i) for e in self.slots(i)]


def same_tilfa(a, b, i=0, lfa_flags=0):
    """Every TI-LFA field of the two models agrees (the slot arrays over the root's slots: the stride may differ)."""
    K = len(a.cands[i].nbr)
    ta, tb = a.want(lfa_flags)[i][2], b.want(lfa_flags)[i][2]
    return len(b.cands[i].nbr) == K and all(np.array_equal(getattr(ta, f)[:K] if f.startswith("ti_") else getattr(ta, f),
                                                            getattr(tb, f)[:K] if f.startswith("ti_") else getattr(tb, f)) for f in T.FIELDS)


@dataclass
class Step:
    tag: str
    patch: pm.Patch = None         # None: the upload
    prot: tuple = ()               # the protected roots of this step (one table set)
    lfa_flags: tuple = (0,)
    parity: bool = False           # the device also compares the patched handle with a fresh upload of the spliced CSR
    convenience: bool = False      # the device also runs SpfContext.tilfa() on the patched handle
    need: object = None            # need(chain, i): what the step is meant to change, asserted on the MODEL
    graph: tuple = None            # the spliced CSR after the step


@dataclass
class Path:
    """One step in one engine configuration, by the patch model."""
    decision: pm.Decision          # None for the upload
    build_mode: int
    pool_compact: bool             # the host mirror's rows lie back to back after the step (hspf_tilfa_device copies it as it is)
    flags_fetched: bool            # the patch fetched the mirror's two-way flags from the device instead of scanning rows


class Chain:
    def __init__(self, name, graph, prot, maxp=MAXP, **kw):
        self.name, self.maxp = name, maxp
        self._mdl = pm.GraphModel(*graph)
        self.steps = [Step("upload", None, tuple(prot), graph=tuple(graph), **kw)]
        self._models = {}

    @property
    def graph(self):
        """The CSR after the last step added so far."""
        return self.steps[-1].graph

    def row(self, v):
        rp, col, met, _ = self.graph
        a, b = int(rp[v]), int(rp[v + 1])
        return col[a:b].copy(), met[a:b].copy()

    def plus(self, v, t, c):
        col, met = self.row(v)
        return np.append(col, np.uint32(t)), np.append(met, np.uint32(c))

    def minus(self, v, t):
        col, met = self.row(v)
        return col[col != t], met[col != t]

    def recost(self, v, t, c):
        col, met = self.row(v)
        met[col == t] = c
        return col, met

    def add(self, tag, rows, flags=None, prot=None, **kw):
        """One patch: rows = {vertex: (col, metric)}, flags = {vertex: new flags} (default: unchanged)."""
        vs = sorted(rows)
        vf = self.graph[3]
        patch = pm.Patch(vs, [rows[v] for v in vs], [int((flags or {}).get(v, vf[v])) for v in vs])
        self._mdl.step(patch)
        m = self._mdl
        self.steps.append(Step(tag, patch, tuple(prot or self.steps[-1].prot), graph=(m.row_ptr, m.col, m.metric, m.vflags), **kw))
        return self.steps[-1]

    def model(self, i) -> Protected:
        i = i % len(self.steps)
        if i not in self._models:
            self._models[i] = Protected(self.steps[i].graph, self.steps[i].prot, self.maxp)
        return self._models[i]

    def paths(self, engine):
        """The model's word per step for an engine configuration of tests/conftest.py."""
        mdl = pm.GraphModel(*self.steps[0].graph, **ENGINES[engine])
        out = [Path(None, pm.MODE_HUB if mdl.hub_built else pm.MODE_REBUILD, True, False)]
        packed = True
        for s in self.steps[1:]:
            old_len = np.diff(mdl.row_ptr.astype(np.int64))[s.patch.vs]
            d = mdl.step(s.patch)
            fetched = d.path != "cost" and d.tw_work > d.tw_bound
            if d.path != "cost":
                if not np.array_equal(old_len, [len(c) for c, _ in s.patch.rows]):
                    packed = False
                if fetched:
                    packed = True                               # the device's flags are in row order: the mirror is compacted first
            out.append(Path(d, d.build_mode, packed, fetched))
        return out

    def check(self, i):
        """The non-vacuity assertions of step i."""
        if self.steps[i].need is not None:
            self.steps[i].need(self, i)


def twoway_byte(graph, u, t):
    """The flag the host mirror keeps for the (first) link u -> t: row t lists u."""
    rp, col, _, _ = graph
    assert t in col[rp[u]:rp[u + 1]]
    return int(u in col[rp[t]:rp[t + 1]])


def cut_distance(graph, S, E, maxp=MAXP):
    """The oracle's distance S -> E on the graph without the links S -> E and E -> S."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    n = len(vf)
    links = [(u, int(col[k]), int(met[k])) for u in range(n) for k in range(int(rp[u]), int(rp[u + 1])) if {u, int(col[k])} != {S, E}]
    g = M.csr(n, links)
    return int(go.run(g[0], g[1], g[2], vf, maxp, np.array([S], np.uint32), 0, go.MAP, mask_words_=1).dist[0, E])


def property_applies(graph):
    """Routers only, no overload, every cost >= 1 and every two-way link costs the same both ways (one-way links are ignored
    by SPF and by the repairs alike): then the best repair's total is the distance S -> E without the protected link."""
    rp, col, met, vf = graph
    if vf.any() or (met == 0).any():
        return False
    cost = {}
    for u in range(len(vf)):
        for k in range(int(rp[u]), int(rp[u + 1])):
            if (u, int(col[k])) in cost:
                return False                                    # parallel links: not used by the chains
            cost[(u, int(col[k]))] = int(met[k])
    return all(cost.get((t, u), c) == c for (u, t), c in cost.items())


def check_best_is_the_way_round(model: Protected):
    """The independent property of tests/test_host_tilfa.py on every candidate slot of every protected root; returns the slots checked."""
    assert property_applies(model.graph)
    checked = 0
    for i, S in enumerate(model.prot):
        t = model.want()[i][2]
        for e in model.slots(i):
            E = int(model.cands[i].nbr[e])
            d = cut_distance(model.graph, S, E, model.maxp)
            if d == R.INF:
                assert t.ti_kind[e] == T.KIND_NONE and t.ti_metric[e] == 0, (S, E)
            else:
                assert t.ti_kind[e] != T.KIND_NONE and t.ti_metric[e] == d, (S, E, d, int(t.ti_metric[e]))
            checked += 1
    return checked


# ---------------------------------------------------------------------------------------------------------------- chains

def _slot_tuple(model, e, lfa_flags=0):
    t = model.want(lfa_flags)[0][2]
    return int(t.ti_kind[e]), int(t.ti_p[e]), int(t.ti_q[e]), int(t.ti_metric[e]), t.ti_counts[e].tolist()


def chain_a():
    """One-way, then two-way, then one-way again, then costs only: the five-ring of tests/test_gpu_tilfa.py, S = 2, the slot of
    E = 3.  Steps 2 and 3 also go through SpfContext.tilfa() (the pending numpy splices of SpfGraph)."""
    from test_gpu_tilfa import five_ring
    c = Chain("a", five_ring(), (2,))

    def need0(ch, i):
        m = ch.model(i)
        assert _slot_tuple(m, m.slot(3)) == (T.KIND_PAIR, 0, 4, 7, [0, 1])
    c.steps[0].need = need0

    def need1(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        e = m.slot(3)
        old, new = ch.steps[i - 1].graph, ch.steps[i].graph
        assert np.diff(new[0])[1] == np.diff(old[0])[1] + 1                      # the row grows: the pool is no longer compact
        assert twoway_byte(new, 1, 4) == 0
        sf = m.want()[0][1].space_flags[e]
        assert sf[1] & R.IN_P and sf[1] & R.ELIGIBLE and sf[4] & R.IN_Q and sf[4] & R.ELIGIBLE      # only the two-way check keeps it out
        assert (1, 4) not in m.pairs(e) and same_tilfa(m, before)
        assert _slot_tuple(m, e) == (T.KIND_PAIR, 0, 4, 7, [0, 1])
    c.add("row 1 gains the one-way link 1 -> 4", {1: c.plus(1, 4, 1)}, need=need1, parity=True)

    def need2(ch, i):
        m = ch.model(i)
        e = m.slot(3)
        assert 1 not in ch.steps[i].patch.vs.tolist()                             # the byte that flips sits in a row the patch does not replace
        assert twoway_byte(ch.steps[i - 1].graph, 1, 4) == 0 and twoway_byte(ch.steps[i].graph, 1, 4) == 1
        assert _slot_tuple(m, e) == (T.KIND_NODE, 4, 4, 3, [1, 3])
        assert m.want()[0][2].td_coverage.tolist() == [3, 0, 3, 0, 0]
        assert (1, 4) in m.pairs(e)
        assert np.array_equal(m.rdist, m.fwd.dist)                                 # symmetric=True of the convenience path is entitled
    c.add("row 4 gains 4 -> 1: the link 1 -> 4 is two-way", {4: c.plus(4, 1, 1)}, need=need2, convenience=True)

    def need3(ch, i):
        m = ch.model(i)
        old, new = ch.steps[i - 1].graph, ch.steps[i].graph
        assert np.diff(new[0])[4] == np.diff(old[0])[4] - 1                      # the row shrinks: a hole in the pool
        assert twoway_byte(new, 1, 4) == 0 and 1 not in ch.steps[i].patch.vs.tolist()
        assert (1, 4) not in m.pairs(m.slot(3)) and same_tilfa(m, ch.model(1))
        assert all(np.array_equal(x, y) for x, y in zip(new, ch.steps[1].graph))
        assert np.array_equal(m.rdist, m.fwd.dist)
    c.add("row 4 loses 4 -> 1 again", {4: c.minus(4, 1)}, need=need3, convenience=True)

    def need4(ch, i):
        m = ch.model(i)
        assert all(ch.paths(eng)[i].decision.path == "cost" for eng in ENGINES)
        assert _slot_tuple(m, m.slot(3)) == (T.KIND_PAIR, 0, 4, 9, [0, 1])
    c.add("costs only: 4 - 0 from 4 to 6", {0: c.recost(0, 4, 6), 4: c.recost(4, 0, 6)}, need=need4)
    return c


def chain_b():
    """Overload set and cleared through a patch that leaves every link as it is (d_vflags rewritten in place): ring8, S = 0, the
    slot of E = 1; every step with and without HSPF_LFA_IGNORE_OVERLOAD."""
    from test_gpu_rlfa import ring8
    both = (0, M.IGNORE_OVERLOAD)
    c = Chain("b", ring8(), (0,), lfa_flags=both)

    def need0(ch, i):
        m = ch.model(i)
        e = m.slot(1)
        assert all(m.winner(e, lfa_flags=lf) == (T.KIND_NODE, 4, 4) for lf in both)
    c.steps[0].need = need0

    def need1(ch, i):
        m = ch.model(i)
        e = m.slot(1)
        p = ch.steps[i].patch
        assert all(np.array_equal(x, y) for x, y in zip(ch.steps[i].graph[:3], ch.steps[i - 1].graph[:3]))      # identical links
        assert p.flags.tolist() == [M.VF_NO_TRANSIT] and ch.steps[i - 1].graph[3][4] == 0
        assert m.winner(e) == (T.KIND_NONE, T.NONE, T.NONE) and m.winner(e, lfa_flags=M.IGNORE_OVERLOAD) == (T.KIND_NODE, 4, 4)
        sp0, sp1 = (m.want(lf)[0][1].space_flags[e] for lf in both)
        assert not sp0[4] & R.ELIGIBLE and sp1[4] & R.ELIGIBLE                     # the space tables differ in the flag's vertex
    c.add("row 4: the same links, overload set", {4: c.row(4)}, flags={4: M.VF_NO_TRANSIT}, need=need1, lfa_flags=both, parity=True)

    def need2(ch, i):
        m = ch.model(i)
        assert ch.steps[i].graph[3][4] == 0 and all(same_tilfa(m, ch.model(0), lfa_flags=lf) for lf in both)
        assert m.winner(m.slot(1)) == (T.KIND_NODE, 4, 4)
    c.add("row 4: overload cleared", {4: c.row(4)}, flags={4: 0}, need=need2, lfa_flags=both)
    return c


CHAIN_C = dict(chord=(60, 257, 3), removed=(44, 145), second_root=258)      # chosen on the CPU: see chain_c


def chain_c():
    """Shifted rows and a second tile: the 300-ring with six chords of tests/test_gpu_tilfa.py (E2E).  The chord 60 - 257 (the
    first of a handful tried whose winners differ AND lie behind both splices: rows 259 and 260) shifts every later row of the
    raw CSR; removing the chord 44 - 145 shifts them back by one and is run with a second protected root beyond vertex 256
    on the same table set; the last patch replaces two rows at once: a winner's row in reverse order (the forced link's
    position moves) and a row before it that grows by a one-way link."""
    from test_gpu_rlfa import ring_chords
    from test_gpu_tilfa import E2E
    seed, root = E2E
    a, b, cost = CHAIN_C["chord"]
    c = Chain("c", ring_chords(300, seed, 1, 9, chords=6), (root,))

    def need1(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        assert a < 256 < b and all(int(x) > b for w in m.winners() for x in w[1:])        # the winners' rows lie behind both splices
        assert all(x != y for x, y in zip(m.winners(), before.winners()))                  # (ti_kind, ti_p, ti_q) of every slot differs
        assert m.want()[0][2].td_coverage[1] > 0 and m.want()[0][2].td_coverage[3] > 0
    c.add(f"chord {a} - {b}", {a: c.plus(a, b, cost), b: c.plus(b, a, cost)}, need=need1, parity=True)

    x, y = CHAIN_C["removed"]
    second = CHAIN_C["second_root"]

    def need2(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        assert m.prot == (root, second) and second > 256 and len(m.roots) == 6
        t0, t1 = m.want()[0][2], m.want()[1][2]
        assert not np.array_equal(t0.ti_counts, before.want()[0][2].ti_counts)             # the removed chord was part of some repair
        assert {w[0] for w in m.winners(0)} == {T.KIND_PAIR} and {w[0] for w in m.winners(1)} == {T.KIND_NODE}
        assert not np.array_equal(t0.td_kind, t1.td_kind)
    c.add(f"chord {x} - {y} removed", {x: c.minus(x, y), y: c.minus(y, x)}, prot=(root, second), need=need2)

    p = c.model(1).winners()[0][1]
    col, met = c.row(p)

    def need3(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        e = int(m.slots()[0])
        assert len(ch.steps[i].patch.vs) == 2 and m.winner(e) == before.winner(e) == (T.KIND_PAIR, p, p - 1)
        l0, l1 = int(before.want()[0][2].ti_link[e]), int(m.want()[0][2].ti_link[e])
        assert (l0, l1) == (0, 1)                                                          # the same link at another position of the row
        assert twoway_byte(ch.steps[i].graph, 99, 270) == 0 and np.array_equal(m.want()[0][2].ti_counts, before.want()[0][2].ti_counts)
    c.add(f"row {p} in reverse order, row 99 gains a one-way link", {p: (col[::-1].copy(), met[::-1].copy()), 99: c.plus(99, 270, 1)},
          prot=(root,), need=need3)
    return c


def chain_d():
    """Arena growth: a ring of 24 routers with two chords and 40 vertices with empty rows; three routers — p and q of the pair
    that wins two slots of S = 4 (19 is also a neighbour of S: its table row has 349 slots, six mask words) and the node that
    wins the third — gain 344 one-way links each into the empty rows: more links than the upload's spare capacity holds (the
    patch model: `grown`; 1024 spare links at the least, so no smaller patch grows any graph), few enough row entries that
    the host still keeps the two-way flags itself, so the mirror's pool stays out of order across the growth.  Then a
    structural step from the arena's reset state, a chord away from the long rows that changes a winner, and a chord between
    two of the long rows: replacing them is more scanning than the host does, in every configuration."""
    from test_gpu_rlfa import ring_chords
    rp, col, met, vf = ring_chords(24, 3, 1, 9, chords=2)
    n, n_sink = 24, 40
    g = (np.concatenate([rp, np.full(n_sink, rp[-1], np.uint32)]), col, met, np.zeros(n + n_sink, np.uint8))
    root = 4
    c = Chain("d", g, (root,))
    sinks = n + np.arange(344) % n_sink
    fat = (2, 11, 19)

    def need1(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        for eng in ENGINES:
            path = ch.paths(eng)[i]
            assert path.decision.grown and path.decision.path == "rebuild"
        assert not ch.paths("default")[i].flags_fetched and not ch.paths("default")[i].pool_compact
        assert same_tilfa(m, before) and (m.want()[0][2].ti_kind != 0).any()               # one-way links: the answer must not move
        assert {x for win in m.winners() for x in win[1:]} == set(fat)                     # every winner's row is one of the long rows
        assert {win[0] for win in m.winners()} == {T.KIND_NODE, T.KIND_PAIR} and m.W == 6 and before.W == 1
    rows = {v: (np.concatenate([c.row(v)[0], sinks]).astype(np.uint32), np.concatenate([c.row(v)[1], np.full(344, 2)]).astype(np.uint32)) for v in fat}
    c.add("three rows gain 344 one-way links each: the arena grows", rows, need=need1, parity=True)

    def need2(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        path = ch.paths("default")[i]
        assert path.build_mode == pm.MODE_INCREMENTAL and not path.decision.grown and not path.pool_compact      # still out of order
        assert m.winners() != before.winners()
    c.add("a chord 14 - 17 after the growth", {14: c.plus(14, 17, 1), 17: c.plus(17, 14, 1)}, need=need2)

    def need3(ch, i):
        m, before = ch.model(i), ch.model(i - 1)
        assert all(ch.paths(eng)[i].flags_fetched for eng in ENGINES)            # two long rows replaced: too many entries to scan
        assert m.winners() != before.winners()
    c.add("a chord 2 - 11 between two of the long rows", {2: c.plus(2, 11, 1), 11: c.plus(11, 2, 1)}, need=need3)
    return c


_chains = {}


def chain(name):
    """The chains are built (and their models computed) once per process."""
    if name not in _chains:
        _chains[name] = {"a": chain_a, "b": chain_b, "c": chain_c, "d": chain_d}[name]()
    return _chains[name]


# ------------------------------------------------------------------------------------- the TI-LFA sweep of the GPU suite

SWEEP_SEED = 20240614                      # of four tried on the CPU the one whose MODEL has the most slots of its rarest kind (11, 93, 11)
SWEEP_GRAPHS = 40


def sweep_graphs(seed=None):
    """[(graph, protected root, what)]: 40 graphs of the generator of tests/test_host_tilfa.py with 12 to 60 routers.  Odd graphs
    get a cost of their own per direction; graphs 0, 4, 8 .. get a share of zero-cost links, graphs 1, 5, 9 .. one overloaded
    router (never the root).  One seeded root each."""
    from test_host_tilfa import _random_graph
    r = np.random.default_rng(SWEEP_SEED if seed is None else seed)
    out = []
    for i in range(SWEEP_GRAPHS):
        n, und = _random_graph(r, 12, 60)
        root = int(r.integers(0, n))
        asym, zero, overload = i % 2 == 1, i % 4 == 0, i % 4 == 1
        links = []
        for a, b, c in und:
            c2 = int(r.integers(1, 10)) if asym else c
            if zero and r.random() < 0.15:
                c = c2 = 0
            links += [(a, b, c), (b, a, c2)]
        ovl = [int((root + 1 + r.integers(0, n - 1)) % n)] if overload else []
        out.append((M.csr(n, links, no_transit=ovl), root, dict(n=n, asym=asym, zero=zero, overload=overload)))
    return out


def sweep_classes(models):
    """(slots per ti_kind over the candidate slots, destinations per td_kind class) over [(candidate slots, TI-LFA model)]."""
    kinds, dests = np.zeros(3, np.int64), np.zeros(5, np.int64)
    for slots, t in models:
        kinds += np.bincount(t.ti_kind[slots], minlength=3)
        dests += np.bincount(t.td_kind, minlength=5)
    return kinds, dests


def check_sweep_classes(models):
    kinds, dests = sweep_classes(models)
    assert (kinds >= 5).all(), ("fewer than five slots of a kind (none, node, pair)", kinds.tolist())
    assert (dests[1:] >= 1).all(), ("a td_kind class without a destination (LFA, node, pair, none)", dests.tolist())
    return kinds, dests
