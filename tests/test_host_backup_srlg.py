"""The model of hspf_routes_backup_srlg_device (tests/_backup_srlg_model.py) on the CPU: its crossing test against an independent
walk of the shortest-path DAG on graphs with a sink vertex per prefix, its agreement with the per-vertex SRLG model for single-homed
prefixes and with the plain per-prefix model for empty member tables, and the non-vacuity of the inputs the GPU tests use.  The
constants the model is run with (the flag of lfa_flags, the three bk_flags bits, the width of bk_coverage) are the PRODUCT's, taken
from holo_amd.engine next to the library's symbol by the module's fixture below, and held to the model's: without the call nothing
here runs."""
import heapq

import numpy as np
import pytest

import _backup_cases as C
import _backup_model as B
import _backup_srlg_cases as SC
import _backup_srlg_model as BS
import _lfa_model as M
import _srlg_model as SM

NONE = M.NONE


@pytest.fixture(scope="module", autouse=True)
def product():
    """The library's symbol and the engine's constants; the model's copies of the constants are held to them once, here."""
    from holo_amd import _lib as L
    from holo_amd import engine as E
    assert hasattr(L.load(), "hspf_routes_backup_srlg_device")
    assert (E.LFA_SRLG_SAFE_REPAIRS, E.BK_SRLG_PRIMARY, E.BK_SRLG_PAIR_REFUSED, E.LFA_SRLG_REFUSED, E.BK_SRLG_COVERAGE_WORDS) == \
        (BS.SAFE_REPAIRS, BS.SRLG_PRIMARY, BS.PAIR_REFUSED, BS.SRLG_REFUSED, BS.COVERAGE_WORDS)
    return E


def test_the_product_exports_the_call_and_its_constants(product):
    assert product.SpfContext.routes_backup_srlg_device and "srlg_repairs" in product.SpfContext.backup_routes.__code__.co_varnames


# ---- the crossing test against a walk of the shortest-path DAG ----------------------------------------------------------------

def dijkstra(n, adj, src):
    d = [None] * n
    d[src] = 0
    heap = [(0, src)]
    while heap:
        x, u = heapq.heappop(heap)
        if x > d[u]:
            continue
        for v, c, _ in adj[u]:
            if d[v] is None or x + c < d[v]:
                d[v] = x + c
                heapq.heappush(heap, (d[v], v))
    return d


def links_on_shortest_paths(n, adj, radj, src, dst):
    """The ids of the links some shortest path src -> dst runs over: walk forward from src along links that are tight from src
    and whose head still lies on a shortest path into dst."""
    ds, dt = dijkstra(n, adj, src), dijkstra(n, radj, dst)
    if ds[dst] is None:
        return set()
    seen, todo, out = {src}, [src], set()
    while todo:
        u = todo.pop()
        for v, c, lid in adj[u]:
            if dt[v] is not None and ds[u] + c + dt[v] == ds[dst]:
                out.add(lid)
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
    return out


def router_case(seed):
    """(graph, S, groups, Table) of routers only, no overload: 6 - 14 routers, asymmetric costs, multi-homed prefixes, 1 - 4 groups."""
    r = np.random.default_rng(seed)
    n = int(r.integers(6, 15))
    und = {(v, int(r.integers(0, v))) for v in range(1, n)}
    for _ in range(int(r.integers(n // 2, n + 2))):
        a, b = (int(x) for x in r.integers(0, n, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        links += [(a, b, int(r.integers(1, 6))), (b, a, int(r.integers(1, 6)))]
    g = M.csr(n, links)
    S = int(r.integers(0, n))
    t = B.table([[(int(v), int(r.integers(0, 6))) for v in r.choice(n, size=int(r.integers(1, 4)), replace=False)] for _ in range(2 * n)])
    return g, S, SC.random_groups(g, seed, n_groups=(1, 5), per_group=(2, 5), root=S), t


@pytest.mark.parametrize("seed", range(24))
def test_model_refuses_exactly_when_a_shortest_path_to_the_sink_crosses_the_member(seed):
    g, S, (gp, gr), t = router_case(500 + seed)
    m = SC.Model(g, [S], gp, gr, t)
    rp, col, met, _ = g
    n = len(rp) - 1
    adj = [[(int(col[k]), int(met[k]), k) for k in range(int(rp[u]), int(rp[u + 1]))] for u in range(n)] + [[] for _ in range(t.n)]
    for p in range(t.n):                                              # the sink of prefix p: vertex n + p
        for v, mm, e in t.entries(p):
            adj[v].append((n + p, mm, len(col) + e))
    radj = [[] for _ in adj]
    for u, row in enumerate(adj):
        for v, c, lid in row:
            radj[v].append((u, c, lid))
    c, mem, f = m.cands[0], m.mems[0], m.fwd
    checked = crossed = 0
    for k in range(len(c.nbr)):
        N = int(c.nbr[k])
        if N == NONE:
            continue
        for p in range(t.n):
            on_path = links_on_shortest_paths(len(adj), adj, radj, N, n + p)
            d_np = B.dist_to_prefix(f.dist, f.flags, m.nbr_row[0][k], t, p)[0]
            for i in range(len(mem.tail)):
                lid = int(rp[int(mem.tail[i])]) + int(mem.pos[i])
                want = lid in on_path
                got = d_np is not None and BS.crosses(f.dist, f.flags, t, p, d_np, int(f.dist[m.nbr_row[0][k], int(mem.tail[i])]), mem.cost[i],
                                                      int(mem.head_row[i]))
                assert got == want, (seed, k, p, i)
                checked += 1
                crossed += want
    assert checked and (crossed or seed % 4)                          # (most graphs cross something; none is required to)


# ---- agreement with the existing models ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(SC.RANDOM_SEED, SC.RANDOM_SEED + 12))
def test_single_homed_metric_0_prefixes_are_the_per_vertex_srlg_answer(seed):
    g, S, (gp, gr), _ = SC.random_case(seed)
    routers = [v for v in range(len(g[3])) if not (g[3][v] & M.VF_NETWORK)]
    m = SC.Model(g, [S], gp, gr, B.table([[(v, 0)] for v in routers]))
    for lf in (0, M.IGNORE_OVERLOAD):
        w, a = m.want(lf, remote=False)[0], m.frr(lf)[0][0]
        for p, v in enumerate(routers):
            fl = int(a.alt_flags[v])
            if not (fl & M.HAS_PRIMARY):
                assert w.bk_kind[p] in (B.NO_ROUTE, B.LOCAL)
                continue
            assert np.array_equal(w.bk_cand_mask[p], a.cand_mask[v]) and np.array_equal(w.bk_node_mask[p], a.node_mask[v]), (seed, v)
            assert bool(w.bk_flags[p] & BS.SRLG_REFUSED) == bool(fl & SM.SRLG_REFUSED)
            if fl & M.ECMP:
                assert w.bk_kind[p] == B.ECMP
                continue
            assert (w.bk_kind[p] == B.LFA) == bool(fl & M.LINK_PROTECT)
            assert w.bk_slot[p] == a.alt_slot[v] and w.bk_metric[p] == a.alt_metric[v]
            assert (int(w.bk_flags[p]) ^ fl) & (M.NODE_PROTECT | M.DOWNSTREAM) == 0


@pytest.mark.parametrize("seed", range(SC.RANDOM_SEED, SC.RANDOM_SEED + 12))
def test_empty_member_tables_are_the_plain_model(seed):
    g, S, (gp, gr), t = SC.random_case(seed)
    m = SC.Model(g, [S], gp, gr, t, no_members=True)
    plain = C.Model(g, [S], t)
    assert np.array_equal(m.roots[:len(plain.roots)], plain.roots) or set(plain.roots) <= set(m.roots)
    for lf in (0, BS.SAFE_REPAIRS):
        w = m.want(lf)[0]
        f, c, rr, nr = m.fwd, m.cands[0], m.root_row[0], m.nbr_row[0]
        x = B.backup(f.dist, f.flags, f.mask, c, rr, nr, t, m.routes(0), 0, m.frr(0)[0][2])
        for name in B.FIELDS[:-1]:
            assert np.array_equal(getattr(w, name), getattr(x, name)), name
        assert np.array_equal(w.bk_coverage[:7], x.bk_coverage) and not w.bk_coverage[7:].any()


# ---- non-vacuity of what the GPU tests feed the kernel ------------------------------------------------------------------------

def differs_from_the_attaining_vertex(m, w, a):
    """Multi-homed prefixes with one primary whose per-prefix answer is not the per-vertex answer at S's attaining vertex."""
    t, r, out = m.table, m.routes(0), []
    for p in range(t.n):
        if int(t.ptr[p + 1]) - int(t.ptr[p]) < 2 or w.bk_kind[p] not in (B.LFA, B.NOTHING, B.NODE, B.PAIR):
            continue
        v = int(t.vertex[int(r.best_entry[p])])
        if (a.alt_slot[v] if a.alt_flags[v] & M.LINK_PROTECT else NONE) != (w.bk_slot[p] if w.bk_kind[p] == B.LFA else NONE):
            out.append(p)
    return out


def test_every_class_occurs_in_the_hand_and_random_inputs_of_the_gpu_tests():
    cases = [SC.ring()] + [SC.random_case(s) for s in range(SC.RANDOM_SEED, SC.RANDOM_SEED + SC.GPU_GRAPHS)]
    total = dict(differs=0)
    for g, S, (gp, gr), t in cases:
        m = SC.Model(g, [S], gp, gr, t)
        off, on = m.want(0)[0], m.want(BS.SAFE_REPAIRS)[0]
        for k, v in SC.tally([off, on]).items():
            total[k] = total.get(k, 0) + v
        total["differs"] += len(differs_from_the_attaining_vertex(m, off, m.frr(0)[0][0]))
        total["node_under_flag"] = total.get("node_under_flag", 0) + sum(1 for p in off.flag_matters if off.bk_kind[p] == B.NOTHING and on.bk_kind[p] == B.NODE)
    for k in ("refused_other", "refused_none", "differs", "node_under_flag", "pair_refused", "ecmp_one_sided"):
        assert total[k] > 0, (k, total)


def test_the_hand_case_is_what_its_docstring_says():
    g, S, (gp, gr), t = SC.ring()
    m = SC.Model(g, [S], gp, gr, t)
    off, on = m.want(0)[0], m.want(BS.SAFE_REPAIRS)[0]
    e, k3 = m.slot(1), m.slot(3)
    assert off.bk_kind[6] == B.NOTHING and off.bk_primary[6] == e and off.bk_flags[6] == BS.SRLG_PRIMARY | BS.SRLG_REFUSED
    assert on.bk_kind[6] == B.NODE and on.bk_flags[6] == off.bk_flags[6]
    plain = C.Model(g, [S], t).want(0)[0]
    assert plain.bk_kind[6] == B.LFA and plain.bk_slot[6] == k3                  # what hspf_routes_backup_device installs: the chord
    assert off.bk_primary[7] == k3 and off.bk_flags[7] & BS.SRLG_PRIMARY == 0
