"""Per-prefix node-protecting backups on the CPU side: the new symbol in header, ctypes table and library; the model
(tests/_backup_node_model.py) pinned on hand-checked cases; then two independent checks on seeded graphs
(tests/_backup_node_cases.py) — the chosen node's distance to the prefix recomputed by the oracle on the graph WITHOUT the
neighbour, and the gather of the per-vertex models for single-homed prefixes — and the counts that show the sweeps are not vacuous.
Nothing here touches a GPU."""
import ctypes
import os
import re
from collections import Counter

import numpy as np

import _backup_cases as C
import _backup_model as B
import _backup_node_cases as BC
import _backup_node_model as BN
import _rlfa_node_model as N
import _tilfa_node_model as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "hspf_routes_backup_node_device"


def test_header_ctypes_and_library_agree_on_the_new_symbol():
    from holo_amd import build, _lib
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"\bint " + FN + r"\(([^;]*?)\);", hdr, re.S)
    assert m, FN + " is not declared"
    assert len(m.group(1).split(",")) == 20
    assert hasattr(lib, FN)
    assert table[FN][0] is ctypes.c_int and len(table[FN][1]) == 20
    assert lib.hspf_abi_version() == 8                                   # additions only
    from holo_amd import engine as E
    for c_name, py, mdl in (("HSPF_BN_LFA", E.BN_LFA, BN.BN_LFA), ("HSPF_BN_PQ", E.BN_PQ, BN.BN_PQ), ("HSPF_BN_LAST_HOP", E.BN_LAST_HOP, BN.BN_LAST_HOP),
                            ("HSPF_BN_NONE", E.BN_NONE, BN.BN_NONE), ("HSPF_BN_PAIR", E.BN_PAIR, BN.BN_PAIR),
                            ("HSPF_BN_COVERAGE_WORDS", E.BN_COVERAGE_WORDS, 6)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py == mdl, c_name
    assert (BN.BN_LFA, BN.BN_PQ, BN.BN_LAST_HOP, BN.BN_NONE, BN.BN_PAIR) == (TN.D_LFA, TN.D_PQ, TN.D_LAST_HOP, TN.D_NONE, TN.D_PAIR)   # the numbering of HSPF_TN_D_*
    assert len(_lib.HspfBackupNodeOut._fields_) == 10 and ctypes.sizeof(_lib.HspfBackupNodeOut) == 10 * ctypes.sizeof(ctypes.c_void_p)
    names = re.search(r"typedef struct \{([^}]*)\} hspf_backup_node_out;", hdr, re.S).group(1)
    assert re.findall(r"\*(bn_\w+);", names) == [f for f, _ in _lib.HspfBackupNodeOut._fields_] == list(BN.FIELDS)
    assert all(f in E.BackupRoutes.__dataclass_fields__ and E.BackupRoutes.__dataclass_fields__[f].default is None for f in BN.FIELDS)


def test_six_ring_an_anycast_prefix_on_the_neighbour_is_protected():
    """0-1-2-3-4-5-0 at cost 1, S = 0, slot 0 -> E = 1, slot 1 -> router 5.
    The link 0-1: P = {0, 5, 4, 3} (3 at a tie, extended through neighbour 5: d(5,3) = 2 < d(5,0) + d(0,3) = 4), Q = {1, 2, 3}
    (3 at a tie: d(3,1) = 2 < d(3,0) + d(0,1) = 4): the only PQ node is 3, released by neighbour 5 (slot 1) at 1 + 2 = 3, and its
    release path 0-5-4-3 avoids router 1.
    Prefix 0 = {1 at 0, 3 at 0}: d_S(p) = 1 through slot 0 alone.  d_E(p) = 0 (E's own entry).  d_3(p) = min(d(3,1) + 0, 0 + 0) = 0
    < d(3,1) + d_E(p) = 2: node 3 protects, metric 3 + 0 = 3 — although per vertex the destination is E itself (HSPF_NP_D_LAST_HOP).
    Prefix 1 = {1}: d_3(p) = 2 is not < 2 + 0: nothing protects, E's entry attains d_E(p): HSPF_BN_LAST_HOP.
    Prefix 2 = {2}: d_E(p) = 1, d_3(p) = 1 < d(3,1) + 1 = 3: HSPF_BN_PQ at 3 + 1 = 4.
    Prefix 3 = {3 at 0, 5 at 2}: 3 + 0 = 1 + 2: both slots are primaries: 0."""
    g, S, t = BC.six_ring()
    m = C.Model(g, [S], t)
    assert m.cands[0].nbr.tolist() == [1, 5]
    w = BN.Want(m)
    e = m.slot(1)
    assert (w.rn.nq_node[e, 0], w.rn.nq_via[e, 0], w.rn.nq_metric[e, 0], w.rn.nq_count[e]) == (3, m.slot(5), 3, 1)
    assert w.bk.bk_kind.tolist()[:3] == [B.NODE, B.NODE, B.NODE] and w.bk.bk_kind[3] == B.ECMP      # the plain call: link repairs, no word on the node
    nd, tn = w.per_vertex()
    assert nd.nd_kind[1] == N.D_LAST_HOP and tn.tn_kind[1] == TN.D_LAST_HOP
    bn = w.bn
    assert bn.bn_kind.tolist() == [BN.BN_PQ, BN.BN_LAST_HOP, BN.BN_PQ, 0]
    assert bn.bn_primary.tolist() == [0, 0, 0, BN.NONE] and bn.bn_p.tolist() == bn.bn_q.tolist() == [3, BN.NONE, 3, BN.NONE]
    assert bn.bn_via.tolist() == [1, BN.NONE, 1, BN.NONE] and bn.bn_metric.tolist() == [3, 0, 4, 0] and (bn.bn_link == BN.NONE).all()
    assert bn.bn_set_pq.tolist() == [1, 0, 1, 0] and bn.bn_coverage.tolist() == [3, 0, 2, 1, 0, 0]
    # without the one-segment list the pairs take over: 4 -> 3 (tunnel to 4 at 2, the link at 1) reaches router 3 itself
    wt = BN.Want(m, with_rn=False)
    assert wt.bn.bn_kind.tolist() == [BN.BN_PAIR, BN.BN_LAST_HOP, BN.BN_PAIR, 0] and wt.bn.bn_q[0] == 3 and wt.bn.bn_p[0] == 4 and wt.bn.bn_metric[0] == 3


def test_five_ring_where_p_and_q_do_not_meet_the_prefix_gets_a_pair():
    """0-1-2-3-4-0 with costs 1, 1, 1, 1, 4; S = 2, slot 0 -> router 1, slot 1 -> router 3 (tests/test_host_backup.py).  Neither link
    has a PQ node; the pairs 4 -> 0 (behind slot 0) and 0 -> 4 (behind slot 1) cross the cost-4 link: tunnel at 2, the link at 4.
    Prefix 0 = {0 at 10}: primary slot 0, E = 1, d_E(p) = 1 + 10; q = 0: d_0(p) = 10 < d(0,1) + 11: HSPF_BN_PAIR (4, 0) at 6 + 10.
    Prefix 1 = {1 at 10}: nothing protects, E's own entry: HSPF_BN_LAST_HOP.  Prefix 2 is S's own: 0.  Prefixes 3, 4 mirror 1, 0.
    Prefix 5 = {1 at 2, 3 at 1}: the plain call's alternate is node-protecting: HSPF_BN_LFA; without bk_in the entries decide: router 3
    is E and the listed q = 4 reaches router 1 only through ... 0: d_4(p) = min(5 + 2, 1 + 1) = 2 is not < d(4,3) + d_3(p) = 1 + 1:
    HSPF_BN_LAST_HOP (E's own entry attains d_E(p) = 1)."""
    g, S, t = BC.five_ring()
    m = C.Model(g, [S], t)
    w = BN.Want(m)
    assert (w.rn.nq_count == 0).all() and w.tn.tq_count[:2].tolist() == [1, 1]
    bn = w.bn
    assert bn.bn_kind.tolist() == [BN.BN_PAIR, BN.BN_LAST_HOP, 0, BN.BN_LAST_HOP, BN.BN_PAIR, BN.BN_LFA]
    assert (bn.bn_p[0], bn.bn_q[0], bn.bn_link[0], bn.bn_via[0], bn.bn_metric[0]) == (4, 0, 1, TN.VIA_SELF, 16)
    assert (bn.bn_p[4], bn.bn_q[4], bn.bn_metric[4]) == (0, 4, 16) and bn.bn_set_pair.tolist() == [1, 0, 0, 0, 1, 0]
    assert bn.bn_coverage.tolist() == [5, 1, 0, 2, 0, 2]
    wo = BN.Want(m, with_bk=False).bn
    assert wo.bn_kind.tolist() == [BN.BN_PAIR, BN.BN_LAST_HOP, 0, BN.BN_LAST_HOP, BN.BN_PAIR, BN.BN_LAST_HOP]
    for f in BN.FIELDS[1:-1]:
        assert np.array_equal(getattr(wo, f)[:5], getattr(bn, f)[:5]), f


def _wants(models):
    return [(m, BN.Want(m, max_pq=BC.SWEEP_MAX, max_pairs=BC.SWEEP_MAX)) for m in models]


_W = {}


def wants():
    """[(Model, Want)] of both sweeps, computed once and left unchanged."""
    if not _W:
        _W["all"] = _wants(BC.sweep_models()) + _wants(BC.host_models())
    return _W["all"]


def test_the_chosen_node_reaches_the_prefix_at_the_same_distance_without_the_neighbour():
    """The independent oracle.  For every prefix of kind PQ or PAIR the forward SPT of the chosen node (bn_q) on the graph with
    every link of E removed gives the same distance to the prefix as d_Y(p) on the full graph: the path really avoids E."""
    checked = 0
    for gi, (m, w) in enumerate(wants()):
        c, bn, t = m.cands[0], w.bn, m.table
        need = {}
        for p in np.flatnonzero((bn.bn_kind == BN.BN_PQ) | (bn.bn_kind == BN.BN_PAIR)):
            need.setdefault(int(c.nbr[int(bn.bn_primary[p])]), []).append(int(p))
        for E, ps in need.items():
            cut = BC.without_node(m.graph, E)
            rows = N.y_rows(cut, m.maxp, {int(bn.bn_q[p]) for p in ps}, m.run_flags)
            for p in ps:
                Y = int(bn.bn_q[p])
                d_full, d_cut = BN.node_dist_to_prefix(w.yrows[Y], t, p), BN.node_dist_to_prefix(rows[Y], t, p)
                assert d_full is not None and d_full == d_cut, (gi, p, Y, E, d_full, d_cut)
                e = int(bn.bn_primary[p])
                lst = (w.rn.nq_node[e], w.rn.nq_metric[e]) if bn.bn_kind[p] == BN.BN_PQ else (w.tn.tq_q[e], w.tn.tq_metric[e])
                j = [int(x) for x in lst[0]].index(Y)
                assert int(bn.bn_metric[p]) <= int(lst[1][j]) + d_full, (gi, p)
                checked += 1
    assert checked > 1000, checked


def test_single_homed_prefixes_equal_the_gather_of_the_per_vertex_models():
    """A prefix with one advertiser v != S is the vertex v seen from further away: tn_kind[v] (fed by alt_flags and nd_kind) is
    bn_kind one to one — the LFA class through bk_kind / bk_flags of the per-prefix call — and the chosen entry is nd_* / tn_* of v
    with the metric plus m.  Every such prefix of both sweeps."""
    checked = 0
    for gi, (m, w) in enumerate(wants()):
        S, t, bn = m.prot[0], m.table, w.bn
        nd, tn = w.per_vertex()
        for p in range(t.n):
            ent = t.entries(p)
            if len(ent) != 1 or ent[0][0] == S:
                continue
            v, metric, _ = ent[0]
            tag = (gi, p, v)
            assert int(bn.bn_kind[p]) == int(tn.tn_kind[v]), tag
            if bn.bn_kind[p] == BN.BN_PQ:
                assert (int(bn.bn_p[p]), int(bn.bn_q[p]), int(bn.bn_via[p])) == (int(nd.nd_node[v]),) * 2 + (int(nd.nd_via[v]),), tag
                assert int(bn.bn_metric[p]) == min(int(nd.nd_metric[v]) + metric, BN.SAT) and bn.bn_set_pq[p] == nd.nd_set[v], tag
            elif bn.bn_kind[p] == BN.BN_PAIR:
                assert (int(bn.bn_p[p]), int(bn.bn_q[p]), int(bn.bn_link[p]), int(bn.bn_via[p])) == \
                       (int(tn.tn_p[v]), int(tn.tn_q[v]), int(tn.tn_link[v]), int(tn.tn_via[v])), tag
                assert int(bn.bn_metric[p]) == min(int(tn.tn_metric[v]) + metric, BN.SAT) and bn.bn_set_pair[p] == tn.tn_set[v], tag
            else:
                assert (int(bn.bn_p[p]), int(bn.bn_q[p]), int(bn.bn_link[p]), int(bn.bn_via[p]), int(bn.bn_metric[p])) == (BN.NONE,) * 4 + (0,), tag
            checked += 1
    assert checked > 1500, checked


def test_the_sweeps_show_every_kind_and_the_divergence_from_the_per_vertex_class():
    """Counts on the MODEL alone (the seeds were chosen for them on the CPU: tests/_backup_node_cases.py): every kind 1 .. 5 in the 40
    graphs the GPU test runs, and multi-homed prefixes whose kind is not the per-vertex class of S's attaining advertiser — among them
    prefixes protected although that advertiser is the neighbour itself."""
    n_gpu = len(BC.sweep_models())
    kinds, divergent, anycast = Counter(), 0, 0
    for m, w in wants()[:n_gpu]:
        kinds.update(int(k) for k in w.bn.bn_kind)
    for m, w in wants():
        _, tn = w.per_vertex()
        for p in range(m.table.n):
            if len(m.table.entries(p)) > 1 and w.bn.bn_kind[p]:
                v = int(m.table.vertex[int(w.routes.best_entry[p])])
                divergent += int(tn.tn_kind[v]) != int(w.bn.bn_kind[p])
                anycast += int(tn.tn_kind[v]) == TN.D_LAST_HOP and int(w.bn.bn_kind[p]) in (BN.BN_PQ, BN.BN_PAIR)
    print("kinds", sorted(kinds.items()), "divergent", divergent, "anycast", anycast)
    assert all(kinds[k] >= 50 for k in range(1, 6)), kinds
    assert divergent >= 100 and anycast >= 5, (divergent, anycast)
