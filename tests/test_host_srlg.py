"""SRLG-safe alternates and remote-LFA spaces without a GPU: hspf_srlg_members (host arithmetic of the library) against the
plain-Python restatement of tests/_srlg_model.py, and the model itself against ground truth — on router-only graphs a vertex is in
a safe space, and a slot in the safe cand, exactly when the full shortest-path DAG (walked back over the CPU oracle's distances)
holds neither the protected link nor a member.  The generator is held to making members matter: the shares are asserted."""
import ctypes

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _srlg_model as SM
import _tilfa_model as T

NONE = M.NONE


def _rng(seed):
    return np.random.default_rng(seed)


# ---- hspf_srlg_members ---------------------------------------------------------------------------------------------------

def product_members(graph, root, grp_ptr, grp, cap_slots=None, cap_members=None):
    from holo_amd import engine as E
    return E.srlg_members(*graph, root, grp_ptr, grp, cap_slots, cap_members)


def assert_members(graph, root, grp_ptr, grp):
    want = SM.members(*graph, root, grp_ptr, grp)
    got = product_members(graph, root, grp_ptr, grp)
    for name in ("mem_ptr", "tail", "pos", "head", "cost"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (root, name)
    assert got.total_slots == len(want.mem_ptr) - 1 and got.total_members == len(want.tail)
    return want


def random_lsdb(seed):
    """Routers and LANs, parallel links, links in several groups; the root may have a LAN."""
    r = _rng(seed)
    n_r, n_l = int(r.integers(4, 12)), int(r.integers(0, 3))
    n = n_r + n_l
    links = []
    for v in range(n_r):
        links += M.both([(v, (v + 1) % n_r, int(r.integers(1, 9)))])
    for _ in range(int(r.integers(0, n_r))):
        a, b = (int(x) for x in r.integers(0, n_r, 2))
        if a != b:
            links += M.both([(a, b, int(r.integers(1, 9)))])        # (parallel links happen)
    for l in range(n_r, n):
        for v in sorted(set(int(x) for x in r.integers(0, n_r, 3))):
            links += [(v, l, int(r.integers(1, 9))), (l, v, 0)]
    graph = M.csr(n, links, net=range(n_r, n))
    E = len(graph[1])
    of = {}
    for l in range(E):
        k = int(r.integers(0, 4))
        if k:
            of[l] = sorted(set(int(x) for x in r.integers(0, 6, k)))
    return graph, SM.groups_csr(E, of), int(r.integers(0, n_r))


def test_members_hand_graph_groups_parallel_links_and_self_exclusion():
    # 0 -> 1 twice (parallel), 0 -> 2; link 0->1 (first) shares group 7 with 2->3 and group 9 with the second 0->1 and with 2->3
    g = M.csr(4, M.both([(0, 1, 1)]) + M.both([(0, 1, 5), (0, 2, 1), (2, 3, 1), (1, 3, 1)]))
    p01a, p01b, p23 = SM.link_pos(g, 0, 1, 0), SM.link_pos(g, 0, 1, 1), SM.link_pos(g, 2, 3)
    gp, gr = SM.groups_csr(len(g[1]), {p01a: [7, 9], p01b: [9], p23: [9, 7]})
    want = assert_members(g, 0, gp, gr)
    k_a = 0                                                        # slot 0 = the first link of the root's row
    mem = [(int(want.tail[i]), int(want.pos[i]), int(want.head[i]), int(want.cost[i])) for i in want.of(k_a)]
    assert mem == [(0, 1, 1, 5), (2, int(p23 - g[0][2]), 3, 1)]      # ascending (tail, pos), 2->3 once though it shares two groups, itself left out
    assert [len(want.of(k)) for k in range(3)] == [2, 2, 0]


@pytest.mark.parametrize("seed", range(200))
def test_members_random_graphs_against_the_restatement(seed):
    graph, (gp, gr), root = random_lsdb(seed)
    assert_members(graph, root, gp, gr)


def test_members_root_with_more_than_64_slots_and_caps():
    r = _rng(5)
    g = M.csr(71, M.both([(0, v, int(r.integers(1, 9))) for v in range(1, 71)] + [(v, v + 1, 2) for v in range(1, 70)]))
    E = len(g[1])
    gp, gr = SM.groups_csr(E, {l: [int(x) for x in r.integers(0, 40, 2)] for l in range(E)})
    want = assert_members(g, 0, gp, gr)
    K, Mt = len(want.mem_ptr) - 1, len(want.tail)
    assert K == 70 and Mt > 70
    got = product_members(g, 0, gp, gr, cap_slots=10, cap_members=7)
    assert got.total_slots == K and got.total_members == Mt
    assert np.array_equal(got.mem_ptr, want.mem_ptr[:11])
    for name in ("tail", "pos", "head", "cost"):
        assert np.array_equal(getattr(got, name), getattr(want, name)[:7])


def test_members_caps_on_the_raw_symbol_write_every_entry_the_header_promises():
    """mem_ptr holds the true offsets for k <= min(slots, cap_slots): cap_slots + 1 entries, the last one closing slot
    cap_slots - 1; the columns are written below cap_members and nowhere else."""
    from holo_amd import _lib as L
    lib = L.load()
    r = _rng(5)
    g = M.csr(71, M.both([(0, v, int(r.integers(1, 9))) for v in range(1, 71)] + [(v, v + 1, 2) for v in range(1, 70)]))
    rp, col, met, vf = (np.ascontiguousarray(x) for x in g)
    gp, gr = SM.groups_csr(len(col), {l: [int(x) for x in r.integers(0, 40, 2)] for l in range(len(col))})
    want = SM.members(*g, 0, gp, gr)
    K, Mt = len(want.mem_ptr) - 1, len(want.tail)
    u32 = lambda a: a.ctypes.data_as(L.u32p)      # noqa: E731
    csr = L.HspfCsr(71, len(col), u32(rp), u32(col), u32(met), vf.ctypes.data_as(L.u8p), 0xFFFFFFFF)
    SENT = 0xABCDABCD
    for cap_slots, cap_members in ((0, 0), (1, 3), (10, 7), (K - 1, Mt - 1), (K, Mt), (K + 5, Mt + 5)):
        mp = np.full(cap_slots + 2, SENT, np.uint32)
        cols = [np.full(cap_members + 1, SENT, np.uint32) for _ in range(4)]
        ts, tm = ctypes.c_uint32(), ctypes.c_uint32()
        k = lib.hspf_srlg_members(ctypes.byref(csr), 0, u32(gp), u32(gr), cap_slots, cap_members, u32(mp), *(u32(c) for c in cols),
                                  ctypes.byref(ts), ctypes.byref(tm))
        assert k == K == ts.value and tm.value == Mt
        filled = min(K, cap_slots) + 1
        assert np.array_equal(mp[:filled], want.mem_ptr[:filled]) and (mp[filled:] == SENT).all(), (cap_slots, mp[:12])
        m = min(Mt, cap_members)
        for got, name in zip(cols, ("tail", "pos", "head", "cost")):
            assert np.array_equal(got[:m], getattr(want, name)[:m]) and (got[m:] == SENT).all(), (cap_members, name)


def test_members_inval_cases():
    from holo_amd import _lib as L
    lib = L.load()
    g = M.csr(3, M.both([(0, 1, 1), (1, 2, 1)]))
    rp, col, met, vf = (np.ascontiguousarray(x) for x in g)
    u32 = lambda a: a.ctypes.data_as(L.u32p)      # noqa: E731
    csr = L.HspfCsr(3, len(col), u32(rp), u32(col), u32(met), vf.ctypes.data_as(L.u8p), 0xFFFFFFFF)
    gp = np.zeros(len(col) + 1, np.uint32)
    call = lambda c, root, ptr: lib.hspf_srlg_members(c, root, ptr, None, 0, 0, None, None, None, None, None, None, None)      # noqa: E731
    assert call(ctypes.byref(csr), 1, u32(gp)) == 2                                 # the slot count, as hspf_lfa_candidates
    assert call(ctypes.byref(csr), 3, u32(gp)) == -1                                 # root out of range
    assert call(None, 0, u32(gp)) == -1 and call(ctypes.byref(csr), 0, None) == -1
    bad = gp.copy(); bad[1] = 2; bad[2] = 1                                           # not monotone
    gr = np.zeros(4, np.uint32)
    assert lib.hspf_srlg_members(ctypes.byref(csr), 0, u32(bad), u32(gr), 0, 0, None, None, None, None, None, None, None) == -1
    col2 = col.copy(); col2[0] = 9                                                    # what hspf_lfa_candidates rejects: a target out of range
    csr2 = L.HspfCsr(3, len(col), u32(rp), u32(col2), u32(met), vf.ctypes.data_as(L.u8p), 0xFFFFFFFF)
    assert call(ctypes.byref(csr2), 0, u32(gp)) == -1


# ---- the model against ground truth --------------------------------------------------------------------------------------

TRUTH_SEEDS = range(24)


def truth_graph(seed):
    """A simple router-only graph (no parallel links), one cost per direction >= 1, 12 .. 40 vertices; every link of the root's
    row is in a group of its own with 1 .. 4 links drawn near the root, so that they lie on shortest paths, and now and then with
    the link before it in the root's row: 1 .. 6 members per protected link, links in two groups, local members."""
    r = _rng(1000 + seed)
    n = int(r.integers(12, 41))
    und = {(v, (v + 1) % n) if v + 1 < n else (0, v) for v in range(n)}
    while len(und) < int(n * 1.6):
        a, b = sorted(int(x) for x in r.integers(0, n, 2))
        if a != b:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        links += [(a, b, int(r.integers(1, 7))), (b, a, int(r.integers(1, 7)))]
    graph = M.csr(n, links)
    rp, col = graph[0], graph[1]
    root = int(r.integers(0, n))
    E = len(col)
    of = {}
    hood = {root} | {int(x) for x in col[rp[root]:rp[root + 1]]}
    hood |= {int(x) for u in sorted(hood) for x in col[rp[u]:rp[u + 1]]}
    near = np.array([l for u in sorted(hood - {root}) for l in range(int(rp[u]), int(rp[u + 1]))])
    for j in range(int(rp[root + 1] - rp[root])):
        prot = int(rp[root]) + j
        for l in r.choice(near, int(r.integers(1, 5)), replace=False):
            of.setdefault(int(l), []).append(100 + j)
        of.setdefault(prot, []).append(100 + j)
        if j and r.random() < 0.5:                                  # a group of two with the link before it in the root's row: local members
            of[prot - 1].append(200 + j)
            of[prot].append(200 + j)
    return graph, SM.groups_csr(E, of), root


def all_pairs(graph):
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    roots = np.arange(len(vf), dtype=np.uint32)
    return go.run(rp, col, met, vf, 0xFFFFFFFF, roots, 0, go.MAP, mask_words_=max(1, go.mask_words(rp, col, met, vf, roots))).dist


def dag_edges(graph, d_x, v, in_links):
    """The links (by position in col) of the full shortest-path DAG X -> v: a predecessor walk back from v over d(X, .)."""
    seen, stack, edges = {v}, [v], set()
    while stack:
        y = stack.pop()
        for x, w, l in in_links[y]:
            if d_x[x] != M.INF and int(d_x[x]) + w == int(d_x[y]):
                edges.add(l)
                if x not in seen:
                    seen.add(x)
                    stack.append(x)
    return edges


def check_truth(seed):
    """Returns (some destination has SRLG_REFUSED, the fifth count word is non-zero somewhere, the sixth coverage word is)."""
    graph, (gp, gr), root = truth_graph(seed)
    rp, col, met, vf = graph
    n = len(vf)
    m = SM.one_root(graph, root, gp, gr)
    cand, mem, lfa, rl = m["cand"], m["mem"], m["lfa"], m["rl"]
    assert all(1 <= len(mem.of(k)) <= 6 for k in range(len(cand.nbr)))
    d = all_pairs(graph)
    in_links = [[] for _ in range(n)]
    for u in range(n):
        for l in range(int(rp[u]), int(rp[u + 1])):
            in_links[int(col[l])].append((u, int(met[l]), l))
    pos_of = lambda a, p: int(rp[a]) + p      # noqa: E731
    bad = {e: {pos_of(root, int(cand.root_link[e]))} | {pos_of(int(mem.tail[i]), int(mem.pos[i])) for i in mem.of(e)} for e in range(len(cand.nbr))}
    dags = {}

    def dag(x, v):
        if (x, v) not in dags:
            dags[(x, v)] = dag_edges(graph, d[x], v, in_links)
        return dags[(x, v)]

    for e in range(len(cand.nbr)):
        E = int(cand.nbr[e])
        for v in range(n):
            if v == root:
                continue
            sf = int(rl.space_flags[e, v])
            assert sf & R.ELIGIBLE
            assert bool(sf & R.IN_P) == (not (dag(root, v) & bad[e])), (seed, "P", e, v)
            assert bool(sf & R.IN_Q) == (not (dag(v, E) & bad[e])), (seed, "Q", e, v)
            xp = False
            for k in range(len(cand.nbr)):
                if cand.root_link[k] == cand.root_link[e]:
                    continue
                first_is_member = pos_of(root, int(cand.root_link[k])) in bad[e]
                xp = xp or (not first_is_member and not (dag(int(cand.nbr[k]), v) & bad[e]))
            assert bool(sf & R.IN_XP) == xp, (seed, "XP", e, v)
    # cand of the LFA call: slot k protects D when N_k's DAG to D holds S nowhere on it (loop-free), and neither k's first link nor
    # that DAG holds the protected link of a primary or one of its members
    for D in range(n):
        if D == root:
            continue
        prim = [p for p in range(len(cand.nbr)) if (int(m["fwd"].mask[0, D, p // 64]) >> (p % 64)) & 1]
        for k in range(len(cand.nbr)):
            N = int(cand.nbr[k])
            loop_free = int(d[N, D]) < int(d[N, root]) + int(d[root, D])
            avoid = set().union(*(bad[p] for p in prim))
            want = loop_free and pos_of(root, int(cand.root_link[k])) not in avoid and not (dag(N, D) & avoid)
            assert bool((int(lfa.cand_mask[D, k // 64]) >> (k % 64)) & 1) == want, (seed, "cand", D, k)
    return bool((lfa.alt_flags & SM.SRLG_REFUSED).any()), bool(rl.pq_counts[:, 4].any()), bool(rl.rl_coverage[5])


def test_model_against_the_shortest_path_dags_and_members_matter():
    hits = np.array([check_truth(seed) for seed in TRUTH_SEEDS])
    share = hits.mean(axis=0)
    assert (share >= 0.1).all(), share.tolist()                       # SRLG_REFUSED | a fifth count word | a sixth coverage word


def test_six_ring_with_one_chord_no_group_refuses_the_chord_and_leaves_a_pq_node():
    """Why the hand case of tests/test_gpu_srlg.py has a second chord.  On a 6-ring with ONE chord at S = 0, for every chord
    (0 - 2, 0 - 3, 0 - 4), every chord cost 1 .. 5 and every group of the primary 0 -> 1 with one or two links that do not leave S
    (the chord's ONWARD path, not the chord itself: a member local to the chord's slot is another hand case): whenever the chord
    is the alternate the plain call chose for some destination and the group refuses it, leaving none, the slot's safe spaces
    hold no PQ node.  (Every path into the far end of the ring ends on the same link.)"""
    import itertools
    ring = [(v, (v + 1) % 6, 1) for v in range(6)]
    refused = 0
    for far in (2, 3, 4):
        for cost in range(1, 6):
            g = M.csr(6, M.both(ring + [(0, far, cost)]))
            E = len(g[1])
            p01 = SM.link_pos(g, 0, 1)
            others = [l for l in range(E) if l >= int(g[0][1])]      # the links of rows 1 .. 5
            for grp_links in itertools.chain(((l,) for l in others), itertools.combinations(others, 2)):
                gp, gr = SM.groups_csr(E, {p01: [1], **{l: [1] for l in grp_links}})
                m = SM.one_root(g, 0, gp, gr)
                c, lfa, rl = m["cand"], m["lfa"], m["rl"]
                e = [k for k in range(len(c.nbr)) if c.nbr[k] == 1][0]
                kc = [k for k in range(len(c.nbr)) if c.nbr[k] == far][0]
                hit = [D for D in range(6) if lfa.plain.alt_slot[D] == kc and (lfa.alt_flags[D] & SM.SRLG_REFUSED) and not (lfa.alt_flags[D] & M.LINK_PROTECT)
                       and (int(m["fwd"].mask[0, D, 0]) >> e) & 1]
                if hit:
                    refused += 1
                    assert rl.pq_node[e] == NONE, (far, cost, grp_links, hit, int(rl.pq_node[e]))
    assert refused > 20                                       # the premise occurs: the search is not vacuous


# ---- identities -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_empty_member_lists_give_the_plain_models(seed):
    graph, (gp, gr), root = truth_graph(seed)
    m = SM.one_root(graph, root, gp, gr, no_members=True)
    for name in SM.LFA_FIELDS[:-1]:
        assert np.array_equal(getattr(m["lfa"], name), getattr(m["lfa"].plain, name)), name
    assert np.array_equal(m["lfa"].coverage[:5], m["lfa"].plain.coverage) and not m["lfa"].coverage[5:].any()
    for name in R.FIELDS:
        g, w = getattr(m["rl"], name), getattr(m["rl"].plain, name)
        if name == "pq_counts":
            assert np.array_equal(g[:, :4], w) and not g[:, 4].any()
        elif name == "rl_coverage":
            assert np.array_equal(g[:4], w) and not g[4:].any()
        else:
            assert np.array_equal(g, w), name


@pytest.mark.parametrize("seed", range(4))
def test_tilfa_on_the_safe_tables_takes_single_nodes_from_the_safe_pq_set(seed):
    graph, (gp, gr), root = truth_graph(seed)
    m = SM.one_root(graph, root, gp, gr)
    rl, c = m["rl"], m["cand"]
    t = T.tilfa(m["fwd"].dist, m["fwd"].flags, m["fwd"].mask, m["rdist"], graph, c, 0, m["nbr_row"], rl.space_flags, rl.space_via, m["lfa"].alt_flags)
    assert np.array_equal(t.ti_counts[:, 0], rl.pq_counts[:, 3])
    for e in np.flatnonzero(t.ti_kind == 1):
        sf = int(rl.space_flags[e, int(t.ti_p[e])])
        assert (sf & (R.IN_P | R.IN_XP)) and (sf & R.IN_Q)
