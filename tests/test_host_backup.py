"""Per-prefix backup routes on the CPU side: the new symbol in header, ctypes table and library; the model
(tests/_backup_model.py) pinned on two hand-checked cases; then two independent checks on 500 seeded graphs
(tests/_backup_cases.py) — the per-vertex LFA model, verified on its own, on a graph in which every multi-homed prefix has become a
vertex, and the gather of the per-vertex tables for single-homed prefixes — and the counts that show the sweep is not vacuous.
Nothing here touches a GPU."""
import ctypes
import os
import re
from collections import Counter

import numpy as np
import pytest

import _backup_cases as C
import _backup_model as B
import _lfa_model as M
import _tilfa_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(C.SWEEP_SEED, C.SWEEP_SEED + C.HOST_GRAPHS)


def test_header_ctypes_and_library_agree_on_the_new_symbol():
    from holo_amd import build, _lib
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"\bint hspf_routes_backup_device\(([^;]*?)\);", hdr, re.S)
    assert m, "hspf_routes_backup_device is not declared"
    assert len(m.group(1).split(",")) == 14
    assert hasattr(lib, "hspf_routes_backup_device")
    assert table["hspf_routes_backup_device"][0] is ctypes.c_int and len(table["hspf_routes_backup_device"][1]) == 14
    assert lib.hspf_abi_version() == 8                                   # additions only
    from holo_amd import engine as E
    for c_name, py, mdl in (("HSPF_BK_NO_ROUTE", E.BK_NO_ROUTE, B.NO_ROUTE), ("HSPF_BK_LOCAL", E.BK_LOCAL, B.LOCAL), ("HSPF_BK_ECMP", E.BK_ECMP, B.ECMP),
                            ("HSPF_BK_LFA", E.BK_LFA, B.LFA), ("HSPF_BK_NODE", E.BK_NODE, B.NODE), ("HSPF_BK_PAIR", E.BK_PAIR, B.PAIR),
                            ("HSPF_BK_NONE", E.BK_NONE, B.NOTHING), ("HSPF_BK_COVERAGE_WORDS", E.BK_COVERAGE_WORDS, 7)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py == mdl, c_name
    assert (B.NODE_PROTECT, B.DOWNSTREAM) == (E.LFA_NODE_PROTECT, E.LFA_DOWNSTREAM) == (M.NODE_PROTECT, M.DOWNSTREAM)
    assert len(_lib.HspfBackupOut._fields_) == 8 and ctypes.sizeof(_lib.HspfBackupOut) == 8 * ctypes.sizeof(ctypes.c_void_p)
    names = re.search(r"typedef struct \{([^}]*)\} hspf_backup_out;", hdr, re.S).group(1)
    assert re.findall(r"\*(bk_\w+);", names) == [f for f, _ in _lib.HspfBackupOut._fields_] == list(B.FIELDS)


def test_square_with_a_diagonal_prefix_alternate_that_is_no_vertex_alternate():
    """S = 0; links 0-1: 2, 0-3: 1, 3-2: 1, 1-2: 5, 0-2: 3; slots of S: 0 -> router 1, 1 -> router 3, 2 -> router 2.
    Prefix 0 = {router 1 at metric 1, router 2 at metric 2}.
      d_S(p) = min(d(0,1) + 1, d(0,2) + 2) = min(2 + 1, 2 + 2) = 3, attained by router 1 alone: P = {slot 0}, E = 1.
      Per vertex, D = 1: d(3,1) = 3 (through S) is not < d(3,0) + d(0,1) = 1 + 2; d(2,1) = 4 (2-3-0-1) is not < d(2,0) + d(0,1) =
      2 + 2: router 1 has NO alternate — alt_flags[1] = HAS_PRIMARY alone.
      Per prefix: N = 3: d_3(p) = min(3 + 1, 1 + 2) = 3 < d(3,0) + d_S(p) = 1 + 3: a candidate (it delivers to router 2).
                  N = 2: d_2(p) = min(4 + 1, 0 + 2) = 2 < d(2,0) + d_S(p) = 2 + 3: a candidate.
      Node protection, d_E(p) = d_1(p) = min(0 + 1, 4 + 2) = 1: N = 3: 3 < d(3,1) + 1 = 4; N = 2: 2 < d(2,1) + 1 = 5: both.
      Choice: both in node; cost + d_N(p) = 1 + 3 = 4 for slot 1, 3 + 2 = 5 for slot 2: slot 1 at 4.  Downstream: 3 < 3 is false.
    Prefix 1 = {router 1 at 1}: the per-vertex result of router 1 — no alternate; the repair of the link 0-1."""
    g, S, t = C.square()
    m = C.Model(g, [S], t)
    assert m.cands[0].nbr.tolist() == [1, 3, 2] and m.cands[0].cost.tolist() == [2, 1, 3]
    r, w, (lf, _, ti) = m.routes(), m.want()[0], m.frr()[0]
    assert r.best_metric.tolist() == [3, 3] and r.best_entry.tolist() == [0, 2] and r.nexthop_mask[:, 0].tolist() == [1, 1]
    assert lf.alt_flags[1] == M.HAS_PRIMARY and not (lf.alt_flags[1] & M.LINK_PROTECT)
    assert (w.bk_kind[0], w.bk_primary[0], w.bk_slot[0], w.bk_metric[0], w.bk_flags[0]) == (B.LFA, 0, 1, 4, B.NODE_PROTECT)
    assert w.bk_cand_mask[0, 0] == 0b110 and w.bk_node_mask[0, 0] == 0b110
    assert ti.ti_kind[0] != T.KIND_NONE and w.bk_kind[1] == B.NODE + int(ti.ti_kind[0]) - 1
    assert (w.bk_primary[1], w.bk_slot[1], w.bk_metric[1], w.bk_flags[1]) == (0, ti.ti_via[0], ti.ti_metric[0], 0)
    assert m.want(0, remote=False)[0].bk_kind.tolist() == [B.LFA, B.NOTHING]


def test_five_ring_remote_repairs_back_up_the_far_side():
    """0-1-2-3-4-0 with costs 1, 1, 1, 1, 4; S = 2, slot 0 -> router 1, slot 1 -> router 3.  No neighbour is loop-free for anything
    (d(1, v) = 1 + d(2, v) for v = 3, 4; the mirror image for 3) and neither link has a PQ node: the pairs 0 -> 4 / 4 -> 0 at 7 are
    the repairs (tests/test_host_tilfa.py).  Prefixes 0, 1 (behind slot 0) and 3, 4 (behind slot 1), single-homed at metric 10: PAIR
    with the repairs, NONE without; prefix 2 is S's own: LOCAL.  Prefix 5 = {router 1 at 2, router 3 at 1}: d_S(p) = min(1 + 2, 1 + 1)
    = 2 through slot 1; N = 1: d_1(p) = min(0 + 2, 2 + 1) = 2 < d(1,2) + 2 = 3: an alternate, its own entry; node: 2 < d(1,3) +
    d_3(p) = 2 + 1; metric 1 + 2 = 3; downstream 2 < 2 is false."""
    g, S, t = C.five_ring()
    m = C.Model(g, [S], t)
    w, wo = m.want(0, True)[0], m.want(0, False)[0]
    assert w.bk_kind.tolist() == [B.PAIR, B.PAIR, B.LOCAL, B.PAIR, B.PAIR, B.LFA]
    assert wo.bk_kind.tolist() == [B.NOTHING, B.NOTHING, B.LOCAL, B.NOTHING, B.NOTHING, B.LFA]
    assert w.bk_primary.tolist() == [0, 0, B.NONE, 1, 1, 1] and w.bk_metric.tolist() == [7, 7, 0, 7, 7, 3]
    assert w.bk_slot.tolist() == [T.VIA_SELF, T.VIA_SELF, B.NONE, T.VIA_SELF, T.VIA_SELF, 0] and w.bk_flags.tolist() == [0, 0, 0, 0, 0, B.NODE_PROTECT]
    assert w.bk_coverage.tolist() == [0, 1, 0, 1, 0, 4, 0] and wo.bk_coverage.tolist() == [0, 1, 0, 1, 0, 0, 4]
    for f in ("bk_primary", "bk_flags", "bk_cand_mask", "bk_node_mask"):
        assert np.array_equal(getattr(w, f), getattr(wo, f)), f


def test_triangle_overloaded_neighbour_is_admitted_through_its_own_entry_only():
    """S = 0, N = 1 overloaded, E = 2; every link costs 1; slot 0 -> router 1, slot 1 -> router 2.
    Prefix 0 = {router 1 at 2, router 2 at 1}: d_S(p) = min(1 + 2, 1 + 1) = 2 through slot 1.  d_1(p) = min(0 + 2, 1 + 1) = 2, a
    tie that N's OWN entry attains: N delivers without transiting, and 2 < d(1,0) + 2 = 3: the alternate, at 1 + 2 = 3.  Node:
    d_2(p) = 1, 2 < d(1,2) + 1 = 2 is false; downstream 2 < 2 is false: flags 0.
    Prefix 1 = {router 1 at 3, router 2 at 1}: d_1(p) = min(3, 2) = 2 through router 2 alone: transit through an overloaded
    router — no candidate, unless the call passes HSPF_LFA_IGNORE_OVERLOAD."""
    g, S, t = C.triangle()
    m = C.Model(g, [S], t)
    assert m.cands[0].nbr.tolist() == [1, 2] and m.cands[0].cflags.tolist() == [M.C_NO_TRANSIT, 0]
    w, wi = m.want(0, remote=False)[0], m.want(M.IGNORE_OVERLOAD, remote=False)[0]
    assert w.bk_kind.tolist() == [B.LFA, B.NOTHING] and w.bk_primary.tolist() == [1, 1] and w.own_exception == 1
    assert (w.bk_slot[0], w.bk_metric[0], w.bk_flags[0], w.bk_cand_mask[0, 0], w.bk_node_mask[0, 0]) == (0, 3, 0, 1, 0)
    assert w.bk_cand_mask[1, 0] == 0 and wi.bk_kind.tolist() == [B.LFA, B.LFA] and wi.bk_cand_mask[:, 0].tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------------------------ the sweep

_SWEEP = {}


def sweep():
    """[(seed, Model)] of the 500 graphs, computed once and left unchanged."""
    if not _SWEEP:
        _SWEEP["models"] = [(s, C.Model(*(lambda g, S, t: (g, [S], t))(*C.sweep_case(s)))) for s in SEEDS]
    return _SWEEP["models"]


def test_every_multi_homed_prefix_equals_the_per_vertex_model_on_the_augmented_graph():
    """The independent oracle.  Every qualifying prefix becomes a router vertex X_p with HSPF_VF_NO_TRANSIT behind its advertisers
    at their metrics (tests/_backup_cases.py: augmented); d(X, X_p) is then d_X(p), the first-hop mask of X_p the route's, and
    tests/_lfa_model.py at D = X_p — pinned by tests/test_host_lfa.py — must give the model's (bk_slot, bk_metric, flags, cand_mask,
    node_mask) without the remote fallback, with and without HSPF_LFA_IGNORE_OVERLOAD.  A prefix qualifies when its advertisers
    are all routers other than S AND none of them is overloaded: SPF expands no overloaded router, so nothing reaches a vertex
    X_p THROUGH one, while the router's own prefixes stay reachable — the augmented graph cannot say that.  Prefixes with an
    overloaded advertiser are covered by the gather test below when single-homed and by the hand-checked triangle.  No qualifying
    prefix is skipped."""
    compared = 0
    for seed, m in sweep():
        S, t = m.prot[0], m.table
        g2, xs = C.augmented(m.graph, S, t)
        if not xs:                                               # (a small graph whose S advertises into every prefix)
            continue
        aug = C.Model(g2, [S], B.table([]), w_min=m.W)
        c = aug.cands[0]
        assert np.array_equal(c.nbr, m.cands[0].nbr) and np.array_equal(c.cost, m.cands[0].cost) and np.array_equal(aug.roots, m.roots)
        for lf in (0, M.IGNORE_OVERLOAD):
            w, v = m.want(lf, remote=False)[0], M.lfa(aug.fwd.dist, aug.fwd.flags, aug.fwd.mask, c, 0, aug.nbr_row[0], lf)
            for p, X in xs.items():
                tag = (seed, lf, p)
                assert np.array_equal(w.bk_cand_mask[p], v.cand_mask[X]) and np.array_equal(w.bk_node_mask[p], v.node_mask[X]), tag
                assert (int(w.bk_slot[p]), int(w.bk_metric[p]), int(w.bk_flags[p])) == \
                       (int(v.alt_slot[X]), int(v.alt_metric[X]), int(v.alt_flags[X]) & (M.NODE_PROTECT | M.DOWNSTREAM)), tag
                assert (w.bk_kind[p] == B.LFA) == bool(int(v.alt_flags[X]) & M.LINK_PROTECT), tag
                assert (w.bk_kind[p] == B.NO_ROUTE) == (not int(v.alt_flags[X]) & M.HAS_PRIMARY) and (w.bk_kind[p] == B.ECMP) == bool(int(v.alt_flags[X]) & M.ECMP), tag
                compared += 1
    assert compared > 10000, compared


def test_single_homed_prefixes_equal_the_gather_of_the_per_vertex_tables():
    """A prefix with one advertiser v != S is the vertex v seen from further away: td_kind[v] maps to bk_kind, alt_* to bk_*
    (alt_metric + the advertised metric), the repair of the one primary to bk_slot / bk_metric.  Every such prefix of the sweep."""
    kind_of = {T.D_LFA: B.LFA, T.D_NODE: B.NODE, T.D_PAIR: B.PAIR, T.D_NONE: B.NOTHING}
    checked = 0
    for seed, m in sweep():
        S, t, K = m.prot[0], m.table, len(m.cands[0].nbr)
        w, (lf, _, ti), f = m.want()[0], m.frr()[0], m.fwd
        for p in range(t.n):
            e = t.entries(p)
            if len(e) != 1 or e[0][0] == S:
                continue
            v, metric, _ = e[0]
            tag = (seed, p, v)
            prim = [k for k in range(K) if (int(f.mask[0, v, k // 64]) >> (k % 64)) & 1]
            if not int(f.flags[0, v]) & 1:
                want = (B.NO_ROUTE, B.NONE, B.NONE, 0, 0)
            elif len(prim) != 1:
                want = (B.ECMP if prim else B.LOCAL, B.NONE, B.NONE, 0, 0)
            elif int(lf.alt_flags[v]) & M.LINK_PROTECT:
                want = (B.LFA, prim[0], int(lf.alt_slot[v]), min(int(lf.alt_metric[v]) + metric, 0xFFFFFFFE), int(lf.alt_flags[v]) & (M.NODE_PROTECT | M.DOWNSTREAM))
            elif ti.ti_kind[prim[0]] != T.KIND_NONE:
                want = (B.NODE + int(ti.ti_kind[prim[0]]) - 1, prim[0], int(ti.ti_via[prim[0]]), int(ti.ti_metric[prim[0]]), 0)
            else:
                want = (B.NOTHING, prim[0], B.NONE, 0, 0)
            assert (int(w.bk_kind[p]), int(w.bk_primary[p]), int(w.bk_slot[p]), int(w.bk_metric[p]), int(w.bk_flags[p])) == want, tag
            if len(prim) == 1:
                assert want[0] == kind_of[int(ti.td_kind[v])], tag
            if prim:
                assert np.array_equal(w.bk_cand_mask[p], lf.cand_mask[v]) and np.array_equal(w.bk_node_mask[p], lf.node_mask[v]), tag
            checked += 1
    assert checked > 5000, checked


def test_the_sweep_shows_every_kind_the_divergence_and_the_own_entry_exception():
    """Counts on the MODEL alone (the seed range was chosen for them on the CPU): every kind 0-6; prefixes whose alternate serves the
    prefix although the attaining vertex has none (test 1's divergence); prefixes with an overloaded neighbour admitted through its
    own entry."""
    kinds, divergent, own = Counter(), 0, 0
    for _, m in sweep():
        w, lf, r, t = m.want()[0], m.frr()[0][0], m.routes(), m.table
        kinds.update(int(k) for k in w.bk_kind)
        own += w.own_exception
        for p in np.flatnonzero(w.bk_kind == B.LFA):
            v = int(t.vertex[int(r.best_entry[p])])
            divergent += v != m.prot[0] and not int(lf.alt_flags[v]) & M.LINK_PROTECT
    print("kinds", sorted(kinds.items()), "divergent", divergent, "own-entry", own)
    assert all(kinds[k] >= 100 for k in range(7)), kinds
    assert divergent >= 100 and own >= 20, (divergent, own)
