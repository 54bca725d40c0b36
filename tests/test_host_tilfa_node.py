"""The two-segment node-protecting model (tests/_tilfa_node_model.py) against a definition that uses no inequality, on router-only
graphs with symmetric costs >= 1, no GPU: for every destination the model repairs with a pair, the shortest-path DAGs are ENUMERATED
(a Dijkstra of this file, then a walk back from the target over the links that lie on a shortest path) —
  * no shortest path of the tunnel's first leg, from the router the via starts at (S itself, or the neighbour of slot tn_via, which
    is not E) to p, touches E;
  * no shortest path q -> D touches E;
  * the forced link p - q is a link of the graph and is not incident to E;
  * tn_metric is at least the SPF distance S -> D in the graph with E removed (the repair is a path there).
Over the six-ring of the header with its exact values, seeded rings with one heavy link and chords, and grids.  At most a fifth
of the random cases may lack a pair destination (the seeds were chosen on the CPU so that the model alone meets that); the fixed
cases may not lack one at all."""
import heapq

import numpy as np
import pytest

import _rlfa_node_model as N
import _tilfa_node_model as TN
from test_gpu_rlfa import Case
from test_gpu_tilfa import grid, slot_of
from test_gpu_tilfa_node import Want, heavy_ring, six_ring

RING_SEEDS = range(12)                     # rings of 12 + 3 * seed routers, two chords, the root opposite the heavy link
GRID_SEEDS = range(1, 13)                  # 5 x 5 grids with symmetric seeded costs (of seeds 0 .. 15, three have no pair destination; one is in here)


def _adj(graph, without=None):
    rp, col, met, _ = graph
    return [[] if u == without else [(int(col[k]), int(met[k])) for k in range(int(rp[u]), int(rp[u + 1])) if int(col[k]) != without]
            for u in range(len(rp) - 1)]


def _dijkstra(adj, s):
    d = {s: 0}
    heap = [(0, s)]
    while heap:
        du, u = heapq.heappop(heap)
        if du != d[u]:
            continue
        for v, c in adj[u]:
            if v not in d or du + c < d[v]:
                d[v] = du + c
                heapq.heappush(heap, (du + c, v))
    return d


def _on_shortest_paths(adj, s, t):
    """Every vertex on some shortest path s -> t: the DAG of s walked back from t."""
    d = _dijkstra(adj, s)
    assert t in d
    seen, todo = {t}, [t]
    while todo:
        v = todo.pop()
        for u in range(len(adj)):
            if u in d and u not in seen and any(x == v and d[u] + c == d[v] for x, c in adj[u]):
                seen.add(u)
                todo.append(u)
    return seen


def check(case, w):
    """The four properties on every pair destination of the model; returns how many there are."""
    adj = _adj(case.graph)
    rp, col, _, _ = case.graph
    S, pairs = case.root, 0
    for D in np.flatnonzero(w.d.tn_kind == TN.D_PAIR):
        D = int(D)
        e = [k for k in range(len(case.cand.nbr)) if (int(case.fwd.mask[0, D, k // 64]) >> (k % 64)) & 1]
        assert len(e) == 1
        E = int(case.cand.nbr[e[0]])
        p, q, link, via = int(w.d.tn_p[D]), int(w.d.tn_q[D]), int(w.d.tn_link[D]), int(w.d.tn_via[D])
        start = S if via == TN.VIA_SELF else int(case.cand.nbr[via])
        assert start != E and E not in _on_shortest_paths(adj, start, p), (S, D, "the first leg touches E")
        assert E not in _on_shortest_paths(adj, q, D), (S, D, "q's path touches E")
        assert int(col[int(rp[p]) + link]) == q and E not in (p, q), (S, D, "the forced link")
        cut = _dijkstra(_adj(case.graph, without=E), S)
        assert D in cut and int(w.d.tn_metric[D]) >= cut[D], (S, D, int(w.d.tn_metric[D]), cut.get(D))
        pairs += 1
    return pairs


def test_six_ring_exact():
    case = Case(six_ring(), 0)
    w = Want(case)
    e = slot_of(case, 1)
    assert w.nd_kind.tolist() == [0, N.D_LAST_HOP, N.D_NONE, N.D_NONE, N.D_NONE, N.D_LAST_HOP]
    assert [hex(int(x)) for x in w.r.space_flags[e]] == ["0x0", "0xc", "0xc", "0xc", "0xb", "0xb"]           # extended P = {4, 5}, Q = {1, 2, 3}
    assert (w.sel.tq_q[e, 0], w.sel.tq_p[e, 0], w.sel.tq_link[e, 0], w.sel.tq_via[e, 0], w.sel.tq_metric[e, 0], w.sel.tq_count[e]) == (3, 4, 0, TN.VIA_SELF, 12, 1)
    assert w.d.tn_kind.tolist() == [0, TN.D_LAST_HOP, TN.D_PAIR, TN.D_PAIR, TN.D_PAIR, TN.D_LAST_HOP]
    assert w.d.tn_metric.tolist() == [0, 0, 13, 12, 13, 0] and w.d.tn_set.tolist() == [0, 0, 1, 1, 1, 0]
    assert w.d.tn_coverage.tolist() == [5, 0, 0, 2, 0, 3]
    assert check(case, w) == 3
    assert check(case, Want(case, with_nd=False, with_lfa=False)) == 3


def test_fixed_cases_have_pairs_and_hold_the_properties():
    for case in (Case(heavy_ring(60, 0, 6, heavy_at=40, heavy=40), 10), Case(heavy_ring(255, 1, 2), 121)):
        assert check(case, Want(case)) > 0


def test_random_rings_with_a_heavy_link_and_chords():
    without = 0
    for seed in RING_SEEDS:
        n = 12 + 3 * seed
        root = int(np.random.default_rng(seed).integers(0, n))
        case = Case(heavy_ring(n, seed, 2, heavy_at=(root + n // 2) % n, heavy=n), root)
        for kw in ({}, dict(with_nd=False)):
            without += check(case, Want(case, **kw)) == 0
    assert without * 5 <= 2 * len(RING_SEEDS), without


def test_random_grids():
    without = 0
    for seed in GRID_SEEDS:
        root = int(np.random.default_rng(seed).integers(0, 25))
        case = Case(grid(5, 5, seed), root)
        assert np.array_equal(case.rdist, case.fwd.dist)                    # symmetric costs
        without += check(case, Want(case, with_nd=False)) == 0             # (nd_kind_in NULL: on a grid PQ nodes cover most destinations)
    assert without * 5 <= len(GRID_SEEDS), without
