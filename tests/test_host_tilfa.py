"""Two-segment repair paths on the CPU side: the new symbol in header, ctypes table and library; the model
(tests/_tilfa_model.py) pinned on hand-checked cases; and the property the feature rests on, on seeded random graphs: with
routers only, symmetric costs >= 1 and no overload, the best repair's total is the SPF distance S -> E on the graph WITHOUT
the protected link, and there is no repair exactly when E is unreachable there.  The distances of the cut graph come from the
CPU oracle; nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _tilfa_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXP = 0xFFFFFFFF


def one_root(graph, root, lfa_flags=0, with_lfa=True):
    """(cand, nbr_row, forward tables, rdist, RLFA model, TI-LFA model) of one protected root, rows = [root] + its neighbour routers."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64)
    fwd, rdist = R.tables(graph, MAXP, roots, 0, W)
    alt = M.lfa(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, lfa_flags).alt_flags if with_lfa else None
    r = R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, vf, c, 0, nbr_row, lfa_flags, alt)
    t = T.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, 0, nbr_row, r.space_flags, r.space_via, alt)
    return c, nbr_row, fwd, rdist, r, t


def slot_of(c, v):
    return int(np.flatnonzero(c.nbr == v)[0])


def test_header_ctypes_and_library_agree_on_the_new_symbol():
    from holo_amd import build, _lib
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"\bint hspf_tilfa_device\(([^;]*?)\);", hdr, re.S)
    assert m, "hspf_tilfa_device is not declared"
    assert len(m.group(1).split(",")) == 16
    assert hasattr(lib, "hspf_tilfa_device")
    assert table["hspf_tilfa_device"][0] is ctypes.c_int and len(table["hspf_tilfa_device"][1]) == 16
    assert lib.hspf_abi_version() == 8                                   # additions only
    from holo_amd import engine as E
    for c_name, py in (("HSPF_TILFA_NONE", E.TILFA_NONE), ("HSPF_TILFA_NODE", E.TILFA_NODE), ("HSPF_TILFA_PAIR", E.TILFA_PAIR),
                       ("HSPF_TILFA_D_LFA", E.TILFA_D_LFA), ("HSPF_TILFA_D_NODE", E.TILFA_D_NODE), ("HSPF_TILFA_D_PAIR", E.TILFA_D_PAIR),
                       ("HSPF_TILFA_D_NONE", E.TILFA_D_NONE), ("HSPF_TILFA_COUNT_WORDS", E.TILFA_COUNT_WORDS),
                       ("HSPF_TILFA_COVERAGE_WORDS", E.TILFA_COVERAGE_WORDS)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py, c_name
    assert (T.KIND_NONE, T.KIND_NODE, T.KIND_PAIR) == (E.TILFA_NONE, E.TILFA_NODE, E.TILFA_PAIR)
    assert (T.D_LFA, T.D_NODE, T.D_PAIR, T.D_NONE) == (E.TILFA_D_LFA, E.TILFA_D_NODE, E.TILFA_D_PAIR, E.TILFA_D_NONE)
    assert len(_lib.HspfTilfaOut._fields_) == 9 and ctypes.sizeof(_lib.HspfTilfaOut) == 9 * ctypes.sizeof(ctypes.c_void_p)


def test_six_ring_unit_costs_single_node():
    """0-1-2-3-4-5-0, S = 0, protected link 0-1.  P = {5, 4}, extended P through neighbour 5 = {5, 4, 3}, Q = {1, 2, 3}: the
    PQ node is 3, released by neighbour 5 at 1 + 2, and 3 reaches 1 at 2: total 5 = the way round.  The pairs 4 -> 3 and
    3 -> 2 cost 5 too; the single node comes first."""
    g = M.csr(6, M.both([(v, (v + 1) % 6, 1) for v in range(6)]))
    c, _, _, _, r, t = one_root(g, 0)
    e, k5 = slot_of(c, 1), slot_of(c, 5)
    assert r.pq_node[e] == 3
    assert (t.ti_kind[e], t.ti_p[e], t.ti_q[e], t.ti_via[e], t.ti_link[e], t.ti_metric[e]) == (T.KIND_NODE, 3, 3, k5, T.NONE, 5)
    assert t.ti_counts[e].tolist() == [1, 2]                             # node 3 | 4 -> 3 and 3 -> 2 (5 -> 4: 4 is not in Q)
    # by symmetry the other link: PQ node 3 again, released by neighbour 1
    e5 = slot_of(c, 5)
    assert (t.ti_kind[e5], t.ti_p[e5], t.ti_via[e5], t.ti_metric[e5]) == (T.KIND_NODE, 3, slot_of(c, 1), 5)
    # 2 and 3 have one primary (through 1; 3 is at equal cost both ways: two), no LFA on a ring: repaired by the node
    assert t.td_kind[1] == T.D_NODE and t.td_kind[2] == T.D_NODE and t.td_kind[3] == 0 and t.td_kind[0] == 0
    assert t.td_coverage.tolist() == [4, 0, 4, 0, 0]
    assert not t.ti_kind[2:].any() and (t.ti_p[2:] == T.NONE).all() and (t.ti_link[2:] == T.NONE).all() and not t.ti_metric[2:].any()


def test_five_ring_uneven_costs_needs_the_pair():
    """0-1-2-3-4-0 with costs 1, 1, 1, 1 and 4 on 4-0.  S = 2, protected link 2-3: extended P = {1, 0} (4 is nearer through 3),
    Q = {3, 4} (0 reaches 3 through 2 at the same cost as through 4): no PQ node.  The pair is p = 0, q = 4 over the cost-4
    link: 2 + 4 + 1 = 7 = 2-1-0-4-3."""
    g = M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]))
    c, _, _, _, r, t = one_root(g, 2)
    e = slot_of(c, 3)
    assert r.pq_node[e] == R.NONE and r.pq_counts[e, 3] == 0
    assert (t.ti_kind[e], t.ti_p[e], t.ti_q[e], t.ti_metric[e]) == (T.KIND_PAIR, 0, 4, 7)
    assert t.ti_via[e] == T.VIA_SELF                                     # 0 is in P: S releases it itself at d(2, 0) = 2
    rp, col = g[0], g[1]
    assert col[rp[0] + t.ti_link[e]] == 4
    assert t.ti_counts[e].tolist() == [0, 1]
    # the other link, 2-1, mirrors it: P = {3, 4}, Q = {0, 1}, the pair 4 -> 0 at 2 + 4 + 1 = 7
    e1 = slot_of(c, 1)
    assert (t.ti_kind[e1], t.ti_p[e1], t.ti_q[e1], t.ti_metric[e1]) == (T.KIND_PAIR, 4, 0, 7)
    # every destination has one primary, RLFA left all four uncovered, the pairs cover them
    assert r.rl_coverage.tolist() == [4, 0, 0, 4] and t.td_kind.tolist() == [T.D_PAIR, T.D_PAIR, 0, T.D_PAIR, T.D_PAIR]
    assert t.td_coverage.tolist() == [4, 0, 0, 4, 0]


def test_pendant_bridge_has_no_repair():
    """A triangle 0-2-3 and a pendant 0-1: the link 0-1 is a bridge."""
    g = M.csr(4, M.both([(0, 1, 1), (0, 2, 1), (2, 3, 1), (3, 0, 1)]))
    c, _, _, _, _, t = one_root(g, 0)
    e = slot_of(c, 1)
    assert (t.ti_kind[e], t.ti_p[e], t.ti_q[e], t.ti_via[e], t.ti_link[e], t.ti_metric[e]) == (T.KIND_NONE, T.NONE, T.NONE, T.NONE, T.NONE, 0)
    assert t.ti_counts[e].tolist() == [0, 0] and t.td_kind[1] == T.D_NONE and t.td_coverage[4] == 1
    assert t.ti_kind[slot_of(c, 2)] == T.KIND_NODE                       # the triangle's links are repaired by the third corner


N_GRAPHS = 2000


def _random_graph(r, n_lo=4, n_hi=14):
    """A ring of n_lo .. n_hi routers, unit costs or random costs 1-9, zero to n random chords, parallel links allowed.  Returns
    the undirected links; link i is the two directed entries that M.both makes of und[i]."""
    n = int(r.integers(n_lo, n_hi + 1))
    unit = bool(r.integers(0, 2))
    cost = lambda: 1 if unit else int(r.integers(1, 10))      # noqa: E731
    und = [(v, (v + 1) % n, cost()) for v in range(n)]
    for _ in range(int(r.integers(0, n + 1))):
        a, b = (int(x) for x in r.integers(0, n, 2))
        if a != b:
            und.append((a, b, cost()))
    return n, und


def test_best_repair_is_the_shortest_path_without_the_link():
    from oracle import graph_oracle as go
    go.build()
    r = np.random.default_rng(20240611)
    slots = skipped = pairs = singles = none = 0
    for _ in range(N_GRAPHS):
        n, und = _random_graph(r)
        S = int(r.integers(0, n))
        g = M.csr(n, M.both(und))
        # position j of S's row is link ids[j]: M.csr keeps the order in which a vertex's links appear
        ids = [i for i, (a, b, _) in enumerate(und) for end in (a, b) if end == S]
        c, _, _, _, rl, t = one_root(g, S)
        assert len(c.nbr) == len(ids) and (c.nbr != M.NONE).all()        # routers only: every slot is a candidate, slot = row position
        for e in range(len(ids)):
            slots += 1
            if c.cost[e] == 0:
                skipped += 1
                continue
            a, b, w = und[ids[e]]
            E = b if a == S else a
            assert c.nbr[e] == E and c.cost[e] == w
            cut = M.csr(n, M.both(und[:ids[e]] + und[ids[e] + 1:]))
            d = int(go.run(*cut, MAXP, np.array([S], np.uint32), 0, go.MAP, mask_words_=1).dist[0, E])
            if d == R.INF:
                assert t.ti_kind[e] == T.KIND_NONE and t.ti_metric[e] == 0, (und, S, e)
                none += 1
            else:
                assert t.ti_kind[e] != T.KIND_NONE and t.ti_metric[e] == d, (und, S, e, d, int(t.ti_metric[e]))
                pairs += t.ti_kind[e] == T.KIND_PAIR
                singles += t.ti_kind[e] == T.KIND_NODE
            assert t.ti_counts[e, 0] == rl.pq_counts[e, 3]
    assert skipped == 0 and slots >= 2 * N_GRAPHS                         # the property was applied to every generated slot
    # both kinds of repair occurred; a ring with chords has no bridge, so "unreachable" is test_pendant_bridge_has_no_repair's
    assert pairs > 0 and singles > 0 and none == 0, (pairs, singles, none)


# ---- the model-only halves of tests/test_gpu_frr_patched.py and of the sweep of tests/test_gpu_tilfa.py: the same splices, the
# same assertions on what each step changes, and the property above after every step it applies to — the inputs of the GPU
# tests are proven meaningful without one.

@pytest.mark.parametrize("name,applies", [("a", [0, 1, 2, 3, 4]), ("b", [0, 2]), ("c", [0, 1, 2, 3]), ("d", [0])])
def test_patch_chains_on_the_model(name, applies):
    """Every step of a chain: what it is meant to change, on the model; on the steps with routers only, symmetric costs >= 1 and
    no overload (`applies`: chain b's middle step sets the overload, chain d's long rows hold parallel links) the best total of
    every candidate slot is the SPF distance S -> E without the link."""
    import _frr_chains as F
    from test_gpu_rlfa import Case
    chain = F.chain(name)
    slots = 0
    for i, step in enumerate(chain.steps):
        chain.check(i)
        m = chain.model(i)
        assert F.property_applies(step.graph) == (i in applies), (name, i)
        if i in applies:
            slots += F.check_best_is_the_way_round(m)
        if len(m.prot) == 1:                                             # one root: the rows, and so every table, are Case's
            case = Case(step.graph, m.prot[0])
            assert np.array_equal(case.roots, m.roots) and np.array_equal(case.nbr_row, m.nbr_row[0]) and case.W == m.W
            assert np.array_equal(case.fwd.dist, m.fwd.dist) and np.array_equal(case.rdist, m.rdist)
    assert slots >= 2 * len(applies)
    # the patch model's word on the paths the device is to take: per engine configuration of tests/conftest.py
    paths = {e: chain.paths(e) for e in F.ENGINES}
    assert all(p.build_mode == F.pm.MODE_HUB or p.decision.path == "cost" for p in paths["hubsort"][1:])
    assert all(p.build_mode == F.pm.MODE_REBUILD or p.decision.path == "cost" for p in paths["patchfull"][1:])
    structural = [i for i, p in enumerate(paths["default"]) if i and p.decision.path != "cost"]
    assert all(paths["hubsort"][i].flags_fetched and paths["hubsort"][i].pool_compact for i in structural)
    if name != "b":                                                      # a row's length changes: the pool is out of order afterwards
        assert any(not paths[e][i].pool_compact for e in ("default", "patchfull") for i in structural)
    else:
        assert all(p.pool_compact for e in F.ENGINES for p in paths[e])


def test_patch_chains_reach_every_way_of_keeping_the_flags():
    """Over the four chains, by the patch model: the incremental path, the rebuild, the cost-only path and an arena growth; the
    two-way flags kept by the host's row scan with the pool left out of order, and fetched from the device — in the default
    configuration too (chain d's last step)."""
    import _frr_chains as F
    steps = [(e, p) for name in "abcd" for e in F.ENGINES for p in F.chain(name).paths(e)[1:]]
    modes = {(e, p.build_mode) for e, p in steps}
    assert {("default", F.pm.MODE_INCREMENTAL), ("default", F.pm.MODE_REBUILD), ("default", F.pm.MODE_COST), ("hubsort", F.pm.MODE_HUB),
            ("patchfull", F.pm.MODE_REBUILD)} <= modes
    assert any(p.decision.grown for _, p in steps)
    assert any(e == "default" and p.flags_fetched for e, p in steps) and any(e == "default" and not p.pool_compact for e, p in steps)


def test_sweep_of_the_gpu_suite_shows_every_class():
    """The 40 graphs of tests/test_gpu_tilfa.py's sweep, on the model: n between 12 and 60, the shares of asymmetric, zero-cost
    and overloaded graphs, at least five slots of every ti_kind and a destination in every td_kind class; and the property above
    on the graphs it applies to."""
    import _frr_chains as F
    graphs = F.sweep_graphs()
    assert len(graphs) == 40 and all(12 <= w["n"] <= 60 for _, _, w in graphs)
    assert sum(w["asym"] for _, _, w in graphs) == 20 and sum(w["zero"] for _, _, w in graphs) == 10 and sum(w["overload"] for _, _, w in graphs) == 10
    models, checked = [], 0
    for g, root, w in graphs:
        assert (g[2] == 0).any() == w["zero"] and int((g[3] & M.VF_NO_TRANSIT != 0).sum()) == int(w["overload"]) and not g[3][root]
        m = F.Protected(g, (root,))
        models.append((m.slots(), m.want()[0][2]))
        if not (w["asym"] or w["zero"] or w["overload"]):
            d = {}
            for u in range(w["n"]):
                for k in range(int(g[0][u]), int(g[0][u + 1])):
                    d.setdefault((u, int(g[1][k])), []).append(int(g[2][k]))
            if all(len(v) == 1 for v in d.values()):                     # (no parallel links: cut_distance removes every S - E link)
                checked += F.check_best_is_the_way_round(m)
    kinds, dests = F.check_sweep_classes(models)
    assert checked > 0
