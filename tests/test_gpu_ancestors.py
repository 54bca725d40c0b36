"""hspf_ancestors_device against the plain parent-DAG model (tests/_ancestors_model.py), word for word: level counts, level ranks
and every word of the ancestor sets, on graphs that need more than one wave, one block, one set word and one chunk of sweeps, on
weighted, hop-count, zero-cost and saturating graphs, with overload flags both ways, padding roots, surplus words, the error
returns and the scratch the call shares with graph patches and runs.  tests/test_host_ancestors_model.py pins the model and
proves on the CPU that every case of CASES reaches what it is here for."""
import functools
from dataclasses import dataclass, field

import numpy as np
import pytest

from holo_amd import synth
import _ancestors_model as M
from _failure_cases import CASES as FAILURE_CASES, csr

pytestmark = [pytest.mark.gpu,
              pytest.mark.parametrize("spf_ctx", ["default", "sweeps", "kfused", "twophase", "widemask", "lanevertex", "xcd", "hubsort",
                                                  "patchfull"], indirect=True)]

INF = 0xFFFFFFFF
NO_ROOT = 0xFFFFFFFF
NET_NEXTHOPS, IGNORE_OVERLOAD = 1, 2
RF_EXACT = 2
E_INVAL, E_TOO_MANY_SLOTS = -1, -5
GUARD = 64                        # guard words before and after every output table
FILL = 0xA5


# ---- the case table -------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    graph: tuple                  # (row_ptr, col, metric, vflags)
    maxp: int
    roots: list
    levels: tuple
    run_flags: tuple = (0,)
    # what the case exists for, asserted on the oracle's tables by tests/test_host_ancestors_model.py
    count: dict = field(default_factory=dict)     # {level: exact largest level_count}
    min_count: dict = field(default_factory=dict)  # {level: the largest level_count is at least this}
    min_depth: dict = field(default_factory=dict)  # {level: depth of the parent DAG below the level is at least this}
    static: tuple = (0, 0)        # (at least this many roots in static (dist, index) pop order, at least this many not)
    blocks: dict = field(default_factory=dict)     # {level: its routers of the first root lie in at least this many 256-vertex blocks}
    hubs: tuple = ()              # star-W: (hub, k)
    one_parent_rule: bool = False  # hop-count: a network with two tight zero-cost in-links from routers at equal distance
    saturates: bool = False       # a vertex sits in an SPT at a saturated distance
    min_compared: float = 0.0     # share of the roots that must not be flagged HSPF_RF_EXACT on the device


def _rows_to_csr(rows, vf=None):
    return csr(rows, vf)


def star(k, seed=0):
    """One hub with k p2p neighbours of cost 1 to 5 at the odd indices, a ring of cost 5 through the neighbours (never shorter than
    a direct link, so the hub's level 1 is exactly its neighbours), and the even indices filled with routers behind one or two
    neighbours (the hub's level 2), often at equal total cost.  k = 130: n = 268, the neighbours run past vertex 256."""
    rng = np.random.default_rng(1000 + k + seed)
    n = 2 * k + 8
    hub = 2
    nbrs = list(range(1, 2 * k, 2))
    fill = [v for v in range(n) if v != hub and v not in set(nbrs)]
    rows = [[] for _ in range(n)]

    def link(a, b, c):
        rows[a].append((b, int(c)))
        rows[b].append((a, int(c)))
    hc = {}
    for v in nbrs:
        hc[v] = int(rng.integers(1, 6))
        link(hub, v, hc[v])
    for i, v in enumerate(nbrs):
        link(v, nbrs[(i + 1) % k], 5)
    for f in fill:
        i = min(range(k), key=lambda j: abs(nbrs[j] - f))
        p, q = nbrs[i], nbrs[(i + 1) % k]
        link(f, p, 7 - hc[p])
        if rng.random() < 0.7:
            link(f, q, 7 - hc[q] if rng.random() < 0.7 else int(rng.integers(1, 6)))
    return _rows_to_csr(rows), hub, nbrs


def star_case(k):
    g, hub, nbrs = star(k)
    return Case(f"star-{k}", g, INF, [hub, nbrs[0], nbrs[-1]], (1, 2), count={1: k}, hubs=(hub, k),
                blocks={1: 2} if k == 130 else {}, static=(3, 0), min_compared=1.0)


def wide_level_2():
    """A weighted tree (root, 20 routers, 160 below them, 420 below those) on shuffled indices, n = 601, with chords between
    adjacent depths at the cost that makes them tight (several parents) and a few at other costs."""
    rng = np.random.default_rng(77)
    n = 601
    perm = rng.permutation(n).tolist()
    dist, parent = {perm[0]: 0}, {}
    layers = [[perm[0]], perm[1:21], perm[21:181], perm[181:]]
    rows = [[] for _ in range(n)]

    def link(a, b, c):
        rows[a].append((b, int(c)))
        rows[b].append((a, int(c)))
    for d in (1, 2, 3):
        for v in layers[d]:
            p = layers[d - 1][int(rng.integers(0, len(layers[d - 1])))]
            c = int(rng.integers(1, 4))
            link(p, v, c)
            dist[v], parent[v] = dist[p] + c, p
    for _ in range(260):                                  # tight chords: a second (third) parent one layer up
        d = int(rng.integers(2, 4))
        v = layers[d][int(rng.integers(0, len(layers[d])))]
        p = layers[d - 1][int(rng.integers(0, len(layers[d - 1])))]
        if p != parent[v] and dist[v] > dist[p]:
            link(p, v, dist[v] - dist[p])
    for _ in range(40):                                   # and some that are not tight, or shorten a path
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            link(a, b, int(rng.integers(2, 5)))
    roots = [perm[0], perm[1], perm[2], perm[30]]
    return Case("wide-level-2", _rows_to_csr(rows), INF, roots, (1, 2, 3), min_count={2: 129}, blocks={2: 3}, static=(4, 0), min_compared=1.0)


def deep(mixed):
    """A chain of 40 routers from the root at vertex 0, with unit costs or costs 1 to 4, four bypass routers (40 .. 43) that close an
    equal-cost two-link way round one chain router each, and one direct equal-cost link over a chain router near the far end."""
    rng = np.random.default_rng(5)
    n = 44
    c = [int(rng.integers(1, 5)) if mixed else 1 for _ in range(39)]
    rows = [[] for _ in range(n)]

    def link(a, b, w):
        rows[a].append((b, w))
        rows[b].append((a, w))
    for i in range(39):
        link(i, i + 1, c[i])
    for b, i in zip(range(40, 44), (3, 11, 19, 30)):
        tot = c[i] + c[i + 1]
        w = 1 if tot == 2 else int(rng.integers(1, tot))
        link(i, b, w)
        link(b, i + 2, tot - w)
    link(35, 37, c[35] + c[36])
    return Case("deep-mixed" if mixed else "deep-unit", _rows_to_csr(rows), INF, [0], (1, 2, 20), min_depth={1: 33}, static=(1, 0), min_compared=1.0)


ROOTS64 = list(range(15, 79))
ALL_FLAGS = (0, IGNORE_OVERLOAD, NET_NEXTHOPS, IGNORE_OVERLOAD | NET_NEXTHOPS)


def _lsdb_graph(g):
    return (g.row_ptr, g.col, g.metric, g.vflags)


def weighted_random(seed):
    g = synth.random_lsdb(150, 15, 3.0, seed, metric_hi=6)
    return Case(f"weighted-random-{seed}", _lsdb_graph(g), g.max_path_metric, ROOTS64, (1, 2, 3), ALL_FLAGS, static=(64, 0), min_compared=1.0)


def hopcount_random(seed):
    g = synth.random_lsdb(150, 15, 3.0, seed, metric_hi=6, hopcount=True, lan_size=8)
    return Case(f"hopcount-random-{seed}", _lsdb_graph(g), g.max_path_metric, ROOTS64, (1, 2, 3), ALL_FLAGS, one_parent_rule=True, min_compared=0.25)


ZERO_COST_SEED = 9       # chosen on the CPU: tests/test_host_ancestors_model.py asserts the shares of static and dynamic roots


def zero_cost_mixed():
    g = synth.random_lsdb(150, 15, 3.0, ZERO_COST_SEED, metric_hi=40, zero_cost_router_links=True)
    return Case("zero-cost-mixed", _lsdb_graph(g), g.max_path_metric, ROOTS64, (1, 2), (0,), static=(32, 4), min_compared=0.25)


def saturating(cut):
    """The saturating_detour graph of tests/_failure_cases.py (0 - 1 at 1, 0 - 2 at 0xFFFFFFF0, 2 - 1 at 0x20, OSPF's max path metric);
    cut: without the link 0 - 1, so that root 0 reaches router 1 at a sum that saturates u32 (in the SPT at 0xFFFFFFFF)."""
    c = FAILURE_CASES["saturating_detour"]
    rows = [[(t, w) for t, w in row if cut and {v, t} != {0, 1} or not cut] for v, row in enumerate(c.rows)]
    return Case("saturating-cut" if cut else "saturating", csr(rows, c.vf), c.maxp, [0, 1, 2], (1, 2), saturates=cut)


CASES = ([star_case(k) for k in (63, 64, 65, 130)] + [wide_level_2(), deep(False), deep(True)] +
         [weighted_random(s) for s in range(4)] + [hopcount_random(s) for s in range(2)] + [zero_cost_mixed(), saturating(False), saturating(True)])
CASE_BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def tables(name, run_flags) -> M.Tables:
    """The model's tables of one case and run-flag word: built once, shared by every test and engine configuration, never changed."""
    c = CASE_BY_NAME[name]
    return M.Tables(*c.graph, c.maxp, c.roots, run_flags)


# ---- the device side ------------------------------------------------------------------------------------------------------

class Guarded:
    """A device table with GUARD words before and after it, all of it filled with 0xA5 bytes."""

    def __init__(self, shape, np_dtype):
        import torch
        self.shape, self.dt = shape, np.dtype(np_dtype)
        self.words = int(np.prod(shape))
        self.buf = torch.full(((self.words + 2 * GUARD) * self.dt.itemsize,), FILL, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.buf.data_ptr() + GUARD * self.dt.itemsize

    def fetch(self):
        """The table as numpy, after asserting that the guards are untouched."""
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        g = GUARD * self.dt.itemsize
        assert (raw[:g] == FILL).all() and (raw[-g:] == FILL).all(), "guard words overwritten"
        return raw[g:len(raw) - g].view(self.dt).reshape(self.shape)


FILL_WORD = {4: np.uint32(0xA5A5A5A5), 8: np.uint64(0xA5A5A5A5A5A5A5A5)}


class Run:
    """run_device of `roots` on an uploaded graph: the tables stay on the device for ancestors()."""

    def __init__(self, ctx, G, roots, run_flags):
        import torch
        self.ctx, self.G, self.roots, self.run_flags = ctx, G, np.asarray(roots, np.uint32), run_flags
        R, n = len(roots), G.n
        dev = torch.device("cuda:0")
        self.dist = torch.empty((R, n), dtype=torch.int32, device=dev)
        self.hops = torch.empty((R, n), dtype=torch.int16, device=dev)
        self.flags = torch.empty((R, n), dtype=torch.int16, device=dev)
        ctx.run_device(G, self.roots, run_flags, dist_ptr=self.dist.data_ptr(), hops_ptr=self.hops.data_ptr(), flags_ptr=self.flags.data_ptr())

    def host(self):
        return (self.dist.cpu().numpy().view(np.uint32), self.hops.cpu().numpy().view(np.uint16), self.flags.cpu().numpy().view(np.uint16))

    def check_against(self, ref):
        d, h, f = self.host()
        assert np.array_equal(d, ref.dist) and np.array_equal(h, ref.hops) and np.array_equal(f & 1, ref.flags)

    def exact_roots(self):
        """[R] bool: the root's own flags entry carries HSPF_RF_EXACT."""
        f = self.host()[2]
        return np.array([r != NO_ROOT and bool(f[i, r] & RF_EXACT) for i, r in enumerate(self.roots.tolist())])

    def ancestors(self, level, W, want_rank=True, roots=None):
        """-> (rc, level_count [R], level_rank [R, n] or None, anc [R, n, W]); guards checked."""
        R, n = len(self.roots), self.G.n
        rank = Guarded((R, n), np.uint32) if want_rank else None
        cnt = Guarded((R,), np.uint32)
        anc = Guarded((R, n, W), np.uint64)
        rc = self.ctx.ancestors_device(self.G, self.roots if roots is None else roots, self.run_flags, dist_ptr=self.dist.data_ptr(),
                                       hops_ptr=self.hops.data_ptr(), flags_ptr=self.flags.data_ptr(), level=level, n_words=W,
                                       level_rank_ptr=rank.ptr if want_rank else 0, level_count_ptr=cnt.ptr, anc_ptr=anc.ptr)
        return rc, cnt.fetch(), rank.fetch() if want_rank else None, anc.fetch()


def words_needed(model, skip=None):
    c = [int(x) for i, x in enumerate(model.level_count) if skip is None or not skip[i]]
    return max(1, (max(c, default=0) + 63) // 64)


def compare(run: Run, model: M.Model, level, W=None, min_compared=0.0):
    """One ancestors call at exactly the words the compared roots need (or W), against the model: counts, ranks, every set word.
    Roots the device flags HSPF_RF_EXACT report 0xFFFFFFFF and are skipped.  Returns (compared, skipped)."""
    skip = run.exact_roots()
    if W is None:
        W = words_needed(model, skip)
    rc, cnt, rank, anc = run.ancestors(level, W)
    assert rc == 0, run.ctx.last_error()
    want_cnt = np.where(skip, np.uint32(INF), model.level_count)
    assert np.array_equal(cnt, want_cnt), (cnt.tolist(), want_cnt.tolist())
    keep = np.flatnonzero(~skip)
    assert len(keep) >= min_compared * len(skip), f"{int(skip.sum())} of {len(skip)} roots flagged HSPF_RF_EXACT"
    assert not (rank[keep] == FILL_WORD[4]).any() and not (anc[keep] == FILL_WORD[8]).any(), "table words left unwritten"
    assert np.array_equal(rank[keep], model.level_rank[keep])
    want = model.words(W)
    bad = np.argwhere(anc[keep] != want[keep])
    assert len(bad) == 0, [(int(keep[r]), int(v), int(q), hex(int(anc[keep[r], v, q])), hex(int(want[keep[r], v, q]))) for r, v, q in bad[:8]]
    return len(keep), int(skip.sum())


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_ancestor_sets_match_parent_dag_model(spf_ctx, name):
    c = CASE_BY_NAME[name]
    G = spf_ctx.upload(*c.graph, c.maxp)
    try:
        for rf in c.run_flags:
            t = tables(name, rf)
            run = Run(spf_ctx, G, c.roots, rf)
            run.check_against(t.ref)
            for L in c.levels:
                compared, skipped = compare(run, t.level(L), L, min_compared=c.min_compared)
                print(f"{name} flags={rf} level={L}: count<={int(t.level(L).level_count.max())} compared={compared} skipped={skipped}")
    finally:
        G.free()


@functools.lru_cache(maxsize=None)
def _padding_tables(a, b):
    c = CASE_BY_NAME["weighted-random-0"]
    return M.Tables(*c.graph, c.maxp, [a, NO_ROOT, b, a], 0)


def test_padding_roots_null_rank_high_level_and_surplus_words(spf_ctx):
    c = CASE_BY_NAME["weighted-random-0"]
    t = _padding_tables(20, 47)
    G = spf_ctx.upload(*c.graph, c.maxp)
    try:
        run = Run(spf_ctx, G, t.roots, 0)
        run.check_against(t.ref)
        for L in (1, 2):
            m = t.level(L)
            W = words_needed(m)
            compare(run, m, L, min_compared=1.0)
            rc, cnt, rank, anc = run.ancestors(L, W)
            assert rc == 0
            # the pad row: count 0, all ranks 0xFFFFFFFF, all sets zero; the duplicate rows are identical
            assert cnt[1] == 0 and (rank[1] == INF).all() and not anc[1].any()
            assert cnt[0] == cnt[3] and np.array_equal(rank[0], rank[3]) and np.array_equal(anc[0], anc[3])
            # level_rank == NULL: the same counts and sets
            rc, cnt0, _, anc0 = run.ancestors(L, W, want_rank=False)
            assert rc == 0 and np.array_equal(cnt0, cnt) and np.array_equal(anc0, anc)
            # more words than needed: the surplus words are zero, the others the same
            compare(run, m, L, W=W + 2, min_compared=1.0)
            rc, _, _, wide = run.ancestors(L, W + 2)
            assert rc == 0 and np.array_equal(wide[:, :, :W], anc) and not wide[:, :, W:].any()
        # a level above the deepest hop: count 0, every rank 0xFFFFFFFF, every set zero
        assert not t.level(1000).level_count.any()
        compare(run, t.level(1000), 1000, min_compared=1.0)
        rc, cnt, rank, anc = run.ancestors(1000, 1)
        assert rc == 0 and not cnt.any() and (rank == INF).all() and not anc.any()
    finally:
        G.free()


def test_argument_errors_and_too_many_level_routers(spf_ctx):
    from holo_amd.engine import HspfError
    for k, short in ((65, 1), (130, 2)):
        c = CASE_BY_NAME[f"star-{k}"]
        m = tables(c.name, 0).level(1)
        G = spf_ctx.upload(*c.graph, c.maxp)
        try:
            run = Run(spf_ctx, G, c.roots, 0)
            assert not run.exact_roots().any()
            if k == 65:
                n = G.n
                for level, W, roots in ((0, 2, c.roots), (0x10000, 2, c.roots), (1, 0, c.roots), (1, 2, []), (1, 2, [c.roots[0], n, c.roots[2]])):
                    with pytest.raises(HspfError) as ei:
                        run.ancestors(level, W, roots=np.asarray(roots, np.uint32))
                    assert ei.value.code == E_INVAL, (level, W, roots)
            # one word short: HSPF_E_TOO_MANY_SLOTS, the counts are filled in all the same, the text names the words needed
            assert words_needed(m) == short + 1
            rc, cnt, _, _ = run.ancestors(1, short)
            assert rc == E_TOO_MANY_SLOTS
            assert np.array_equal(cnt, m.level_count)
            assert f"need {short + 1} words" in spf_ctx.last_error(), spf_ctx.last_error()
            # and the next call with enough words is right
            compare(run, m, 1, min_compared=1.0)
        finally:
            G.free()


_PATCHED = {}


def test_scratch_shared_with_patch_and_run(spf_ctx):
    """The call takes the graph-patch staging area and the run's flag scratch, and drops the run prefill: run, ancestors, a
    structural patch of two rows, run, ancestors, the same run again, on one context; every run against the oracle, every
    ancestors call against the model of the CSR of that moment."""
    c = CASE_BY_NAME["weighted-random-1"]
    rp, col, met, vf = c.graph
    t = tables(c.name, 0)
    G = spf_ctx.upload(*c.graph, c.maxp)
    try:
        run = Run(spf_ctx, G, c.roots, 0)
        run.check_against(t.ref)
        compare(run, t.level(2), 2, min_compared=1.0)
        # two routers without a link between them get one each way: both rows grow by an entry
        a, b = 30, 31
        while b in col[rp[a]:rp[a + 1]].tolist() or a in col[rp[b]:rp[b + 1]].tolist():
            b += 1
        G.patch([a, b], [(np.append(col[rp[a]:rp[a + 1]], b), np.append(met[rp[a]:rp[a + 1]], 2)),
                         (np.append(col[rp[b]:rp[b + 1]], a), np.append(met[rp[b]:rp[b + 1]], 3))], [vf[a], vf[b]])
        assert len(G.col) == len(col) + 2
        if c.name not in _PATCHED:
            _PATCHED[c.name] = M.Tables(G.row_ptr.copy(), G.col.copy(), G.metric.copy(), G.vflags.copy(), c.maxp, c.roots, 0)
        t2 = _PATCHED[c.name]
        assert not np.array_equal(t2.ref.dist, t.ref.dist)              # the patch changed shortest paths
        run2 = Run(spf_ctx, G, c.roots, 0)
        run2.check_against(t2.ref)
        compare(run2, t2.level(2), 2, min_compared=1.0)
        compare(run2, t2.level(1), 1, min_compared=1.0)
        Run(spf_ctx, G, c.roots, 0).check_against(t2.ref)
    finally:
        G.free()


