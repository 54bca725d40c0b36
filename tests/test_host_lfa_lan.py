"""Broadcast-link protection on the CPU side: the LAN models (tests/_lfa_lan_model.py) pinned on hand-checked graphs and on a
property that does not use their inequality at all (the oracle on the graph WITHOUT the LAN), their equivalence with the plain
models when no slot crosses a LAN, and hspf_lfa_lan_candidates (pure host arithmetic, no context) against the model's table."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest

import _backup_model as B
import _lfa_lan_model as LM
import _lfa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MAXP = 0xFFFFFFFF
L_, S_, E_, A_, C_, D_, F_, T_ = range(8)


def trap():
    """Pseudonode L with S, E, A attached (router -> L costs 10, 10, 1; L -> router 0); p2p S-C 10, C-A 1, E-D 1, S-F 10, F-E 14,
    D-T 1.  S reaches D and T across L through E; C's own shortest path to them crosses L (C-A-L-E), F's does not."""
    links = [(S_, L_, 10), (L_, S_, 0)] + M.both([(S_, C_, 10), (S_, F_, 10)])
    links += [(E_, L_, 10), (L_, E_, 0), (A_, L_, 1), (L_, A_, 0)] + M.both([(C_, A_, 1), (E_, D_, 1), (F_, E_, 14), (D_, T_, 1)])
    return M.csr(8, links, net=[L_]), S_


def two_lans():
    """S = 2 on LANs 0 and 1 (cost 5 each), E1 = 3 on LAN 0, E2 = 4 on LAN 1, both 5 from D = 5: ECMP across both LANs.  X = 6 (p2p
    S-X 10, X on LAN 0 at cost 1, X-D 6) is safe for LAN 1 and not for LAN 0; Y = 7 (p2p S-Y 10, Y-D 3) is safe for both."""
    links = [(2, 0, 5), (0, 2, 0), (2, 1, 5), (1, 2, 0)] + M.both([(2, 6, 10), (2, 7, 10)])
    links += [(3, 0, 5), (0, 3, 0), (4, 1, 5), (1, 4, 0), (6, 0, 1), (0, 6, 0)] + M.both([(3, 5, 5), (4, 5, 5), (6, 5, 6), (7, 5, 3)])
    return M.csr(8, links, net=[0, 1]), 2


def lone_candidate():
    """The trap without F, plus two stub chains S - Q1 - G1 and S - Q2 - G2 (all costs 1): C is the only alternate towards D and is
    refused, so D has none; G1 and G2 hang behind point-to-point primaries that no neighbour protects."""
    links = [(1, 0, 10), (0, 1, 0)] + M.both([(1, 4, 10), (1, 6, 1), (1, 7, 1)])
    links += [(2, 0, 10), (0, 2, 0), (3, 0, 1), (0, 3, 0)] + M.both([(4, 3, 1), (2, 5, 1), (6, 8, 1), (7, 9, 1)])
    return M.csr(10, links, net=[0]), 1


def two_lans_prefix():
    """two_lans() plus V1 = 8 behind E1 and V2 = 9 behind E2 (5 each) and W = 10: p2p S-W 10, W on LAN 1 at cost 1, p2p W-V1 7.  A
    prefix on V1 and V2 is ECMP across both LANs; S's attaining entry is V1's.  For the VERTEX V1 (one primary, across LAN 0) W is
    safe: 7 < d(W, LAN 0) + 5 = 11.  For the PREFIX W's nearest advertiser is V2, across LAN 1: 6 = d(W, LAN 1) + d_LAN1(p) = 1 + 5."""
    (rp, col, met, vf), root = two_lans()
    links = [(u, int(col[k]), int(met[k])) for u in range(8) for k in range(rp[u], rp[u + 1])]
    links += M.both([(3, 8, 5), (4, 9, 5), (2, 10, 10), (10, 8, 7)]) + [(10, 1, 1), (1, 10, 0)]
    return M.csr(11, links, net=[0, 1]), root


def models(graph, root, run_flags=0, maxp=MAXP, lfa_flags=0):
    """(candidates, lan, plain LFA model, LAN LFA model, the oracle's tables, roots, nbr_row, lan_row) of one root."""
    from oracle import graph_oracle as go
    c, roots, nbr_row, lan, lan_row = LM.protect_one(*graph, root)
    W = max(go.mask_words(*graph, roots), (len(c.nbr) + 63) // 64)
    t = go.run(*graph, maxp, roots, run_flags, go.MAP, mask_words_=W)
    plain = M.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row, lfa_flags)
    lanm = LM.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row, lan, lan_row, lfa_flags)
    return c, lan, plain, lanm, t, roots, nbr_row, lan_row


def members(mask_row):
    return [k for k in range(64 * len(mask_row)) if (int(mask_row[k // 64]) >> (k % 64)) & 1]


def test_header_ctypes_and_library_agree_on_the_new_symbols():
    from holo_amd import build, _lib, engine as E
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, n_args in (("hspf_lfa_lan_candidates", 5), ("hspf_lfa_lan_device", 12), ("hspf_routes_backup_lan_device", 15)):
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert table[name][0] is ctypes.c_int and len(table[name][1]) == n_args
    assert lib.hspf_abi_version() == 8                                   # additions only
    for c_name, py in (("HSPF_LFA_LAN_PRIMARY", E.LFA_LAN_PRIMARY), ("HSPF_LFA_LAN_REFUSED", E.LFA_LAN_REFUSED),
                       ("HSPF_LFA_LAN_COVERAGE_WORDS", E.LFA_LAN_COVERAGE_WORDS), ("HSPF_BK_LAN_COVERAGE_WORDS", E.BK_LAN_COVERAGE_WORDS)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py, c_name
    assert (LM.LAN_PRIMARY, LM.LAN_REFUSED) == (E.LFA_LAN_PRIMARY, E.LFA_LAN_REFUSED) == (0x20, 0x40)
    assert ctypes.sizeof(_lib.HspfLfaProtect) == 56                      # hspf_lfa_protect did not grow


@pytest.mark.parametrize("run_flags", [0, 1])                # HSPF_RUN_NET_NEXTHOPS off / on
def test_trap_the_cheapest_alternate_crosses_the_primarys_lan(run_flags):
    graph, root = trap()
    c, lan, plain, lanm, t, _, nbr_row, lan_row = models(graph, root, run_flags)
    kC, kF = (int(np.flatnonzero((c.nbr == v) & (lan == M.NONE))[0]) for v in (C_, F_))
    for D in (D_, T_):
        P = members(t.mask[0, D])
        assert len(P) == 1 and lan[P[0]] == L_                              # one primary, across L
        assert c.nbr[P[0]] in (E_, M.NONE)
        assert members(plain.cand_mask[D]) == sorted((kC, kF)) and plain.alt_slot[D] == kC and not plain.node_mask[D].any()
        extra = int(t.dist[0, D]) - 11                                       # T lies one behind D
        assert plain.alt_metric[D] == 13 + extra and int(c.cost[kF]) + int(t.dist[nbr_row[kF], D]) == 25 + extra
        # C is refused: d(C, D) = 3 = d(C, L) + d(L, D) = 2 + 1
        assert int(t.dist[nbr_row[kC], D]) == 3 + extra and int(t.dist[nbr_row[kC], L_]) == 2 and int(t.dist[lan_row[P[0]], D]) == 1 + extra
        assert members(lanm.cand_mask[D]) == [kF] and lanm.alt_slot[D] == kF and lanm.alt_metric[D] == 25 + extra
        assert lanm.alt_flags[D] & LM.LAN_PRIMARY and lanm.alt_flags[D] & LM.LAN_REFUSED and lanm.alt_flags[D] & M.LINK_PROTECT
        assert not lanm.alt_flags[D] & M.NODE_PROTECT
    if lanm.alt_flags[L_] & M.HAS_PRIMARY:                                              # (with HSPF_RUN_NET_NEXTHOPS the LAN has a next hop)
        assert lanm.alt_flags[L_] & LM.LAN_PRIMARY and lanm.alt_slot[L_] == M.NONE       # nothing protects the LAN's own vertex
    assert not lanm.alt_flags[C_] & LM.LAN_PRIMARY
    assert lanm.coverage[5] >= 2 and lanm.coverage[6] >= 2


@pytest.mark.parametrize("run_flags", [0, 1])
def test_root_on_two_lans_safe_for_one_is_refused(run_flags):
    graph, root = two_lans()
    c, lan, plain, lanm, t, *_ = models(graph, root, run_flags)
    kX, kY = (int(np.flatnonzero((c.nbr == v) & (lan == M.NONE))[0]) for v in (6, 7))
    P = members(t.mask[0, 5])
    assert len(P) == 2 and sorted(int(lan[p]) for p in P) == [0, 1]      # ECMP across both LANs
    assert members(plain.cand_mask[5]) == sorted((kX, kY))
    assert members(lanm.cand_mask[5]) == [kY]
    assert lanm.alt_flags[5] == M.HAS_PRIMARY | M.ECMP | LM.LAN_PRIMARY | LM.LAN_REFUSED and lanm.alt_slot[5] == M.NONE
    assert (5, kX) in lanm.refused


def _strip(g):
    """The CSR of a recorded topology for the property: its links and network vertices as recorded; router-link costs >= 1, no
    overload / no-expand flags."""
    rp, col, met, vf = (np.array(x) for x in (g.row_ptr, g.col, g.metric, g.vflags))
    vf = (vf & M.VF_NETWORK).astype(np.uint8)
    src = np.repeat(np.arange(len(vf)), np.diff(rp.astype(np.int64)))
    met = np.where((vf[src] & M.VF_NETWORK) == 0, np.maximum(met, 1), met).astype(np.uint32)
    return rp.astype(np.uint32), col.astype(np.uint32), met, vf


def golden_graphs():
    from holo_amd import isis, ospf
    out = {}
    for p in sorted(glob.glob(os.path.join(GOLD, "isis", "*.json"))):
        inst = isis.Instance.from_vector(json.load(open(p)))
        for level in inst.config.levels():
            out[os.path.basename(p)[:-5].rsplit("_", 1)[0] + "_l%d" % level] = _strip(isis.LevelGraph(inst, level, None))
    for p in sorted(glob.glob(os.path.join(GOLD, "ospfv2", "*.json"))):
        for i, a in enumerate(json.load(open(p))["areas"]):
            out[os.path.basename(p)[:-5] + "_a%d" % i] = _strip(ospf.AreaGraph(ospf.Area.from_vector(a)))
    uniq = {}
    for name, g in out.items():                                             # one LSDB is recorded once per router: keep each once
        uniq.setdefault(tuple(x.tobytes() for x in g), (name, g))
    return dict(uniq.values())


def random_graph(seed):
    from holo_amd import synth
    g = synth.random_lsdb(40, 8, 3.0, seed, metric_hi=6, max_path=MAXP, p_overload=0.0, p_noexpand=0.0, lan_size=4)
    return g.row_ptr, g.col, g.metric, g.vflags


SEEDS = list(range(1, 7))


def without_vertices(graph, gone):
    """The graph with every link from or to a vertex of `gone` removed."""
    rp, col, met, vf = graph
    n = len(vf)
    links = [(u, int(col[k]), int(met[k])) for u in range(n) for k in range(rp[u], rp[u + 1]) if u not in gone and int(col[k]) not in gone]
    g = M.csr(n, links)
    g[3][:] = vf
    return g


def check_property(graph):
    """Returns (refused triples, LAN-primary destinations that keep an alternate) over every router root of the graph."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    n_refused = n_kept = 0
    for root in range(len(vf)):
        if vf[root] & M.VF_NETWORK:
            continue
        lan0 = LM.lan_candidates(*graph, root)
        if not (lan0 != M.NONE).any():
            continue
        c, lan, plain, lanm, t, roots, nbr_row, lan_row = models(graph, root)
        cut = {}                                                               # LAN set -> d(N_k, .) without those LANs
        refused = set(lanm.refused)
        for D in np.flatnonzero(lanm.alt_flags & LM.LAN_PRIMARY):
            D = int(D)
            P = members(t.mask[0, D])
            lans = frozenset(int(lan[p]) for p in P if lan[p] != M.NONE)
            ks = members(lanm.cand_mask[D])
            n_kept += bool(lanm.alt_flags[D] & M.LINK_PROTECT)
            if ks and lans not in cut:
                cut[lans] = go.run(*without_vertices(graph, lans), MAXP, roots, 0, go.MAP, mask_words_=t.mask.shape[2]).dist
            for k in ks:
                assert cut[lans][nbr_row[k], D] == t.dist[nbr_row[k], D], (root, D, k)
            for k in members(plain.cand_mask[D]):
                if k not in ks:
                    assert (D, k) in refused
                    n_refused += 1
                    assert any(int(t.dist[nbr_row[k], L]) + int(t.dist[lan_row[p], D]) == int(t.dist[nbr_row[k], D])
                               for p in P for L in [int(lan[p])] if L != M.NONE), (root, D, k)
    return n_refused, n_kept


def test_property_lan_safe_alternates_do_not_need_the_lan_seeded_random_lsdbs():
    totals = np.zeros(2, np.int64)
    for seed in SEEDS:
        totals += check_property(random_graph(seed))
    assert totals[0] >= 50 and totals[1] >= 50, totals


def test_property_lan_safe_alternates_do_not_need_the_lan_recorded_topologies():
    graphs = golden_graphs()                                 # (parsed here, not at import: tests/test_gpu_lfa_lan.py imports this module)
    assert len(graphs) >= 10
    attached = 0
    for name in sorted(graphs):
        g = graphs[name]
        attached += sum(1 for r in range(len(g[3])) if not g[3][r] & M.VF_NETWORK and (LM.lan_candidates(*g, r) != M.NONE).any())
        check_property(g)
    assert attached >= 20                                    # routers attached to a network vertex were there to check


def prefix_table(n, seed, flags=0):
    r = np.random.default_rng(seed)
    lists = [[(int(v), int(r.integers(0, 9))) for v in r.choice(n, int(r.integers(1, 4)), replace=False)] for _ in range(2 * n)]
    return B.table(lists, flags)


@pytest.mark.parametrize("which", ["trap", "two_lans", "random"])
def test_without_lans_the_lan_models_are_the_plain_models(which):
    graph, root = trap() if which == "trap" else two_lans() if which == "two_lans" else (random_graph(3), 20)
    c, lan, plain, _, t, roots, nbr_row, lan_row = models(graph, root)
    none = np.full(len(lan), M.NONE, np.uint32)
    lanm = LM.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row, none, lan_row)
    for f in ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask"):
        assert np.array_equal(getattr(lanm, f), getattr(plain, f)), f
    assert np.array_equal(lanm.coverage[:5], plain.coverage) and not lanm.coverage[5:].any()
    pt = prefix_table(len(graph[3]), 5)
    r = B.routes(t.dist, t.flags, t.mask, 0, pt)
    bp = B.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, pt, r)
    bl = LM.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, none, lan_row, pt, r)
    for f in B.FIELDS[:-1]:
        assert np.array_equal(getattr(bl, f), getattr(bp, f)), f
    assert np.array_equal(bl.bk_coverage[:7], bp.bk_coverage) and not bl.bk_coverage[7:].any()


def test_backup_model_on_the_trap_refuses_per_prefix():
    """Prefix 0 is D's; prefix 1 is advertised by T (at 0) and by A (at 20): S and C both use T's entry, across L; prefix 2 is E's.
    For all three C is refused through the LAN and F takes over."""
    graph, root = trap()
    c, lan, _, _, t, roots, nbr_row, lan_row = models(graph, root)
    pt = B.table([[(D_, 0)], [(T_, 0), (A_, 20)], [(E_, 0)]])
    r = B.routes(t.dist, t.flags, t.mask, 0, pt)
    bl = LM.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, lan, lan_row, pt, r)
    kC, kF = (int(np.flatnonzero((c.nbr == v) & (lan == M.NONE))[0]) for v in (C_, F_))
    assert bl.bk_kind.tolist() == [B.LFA] * 3 and bl.bk_slot.tolist() == [kF, kF, kF]
    assert all(f & LM.LAN_PRIMARY and f & LM.LAN_REFUSED for f in bl.bk_flags)
    assert bl.bk_coverage.tolist() == [0, 0, 0, 3, 0, 0, 0, 3, 3]


def test_backup_model_refuses_per_prefix_where_the_vertex_rule_passes():
    """With ONE primary the prefix rule cannot refuse a neighbour that the vertex rule admits for S's attaining vertex V: S prefers
    V across L, so d_L(p) = d(L, V) + m_V, and d_N(p) <= d(N, V) + m_V < d(N, L) + d_L(p).  It can with ECMP over two LANs."""
    graph, root = two_lans_prefix()
    c, lan, _, lanm, t, roots, nbr_row, lan_row = models(graph, root)
    kW = int(np.flatnonzero((c.nbr == 10) & (lan == M.NONE))[0])
    assert members(t.mask[0, 8]) and [int(lan[p]) for p in members(t.mask[0, 8])] == [0]          # the vertex V1: one primary, across LAN 0
    assert kW in members(lanm.cand_mask[8]) and (8, kW) not in lanm.refused                           # the vertex rule admits W
    pt = B.table([[(8, 0), (9, 0)]])
    r = B.routes(t.dist, t.flags, t.mask, 0, pt)
    assert pt.vertex[int(r.best_entry[0])] == 8 and sorted(int(lan[p]) for p in members(r.nexthop_mask[0])) == [0, 1]
    assert B.dist_to_prefix(t.dist, t.flags, nbr_row[kW], pt, 0)[0] == 6 and int(t.dist[nbr_row[kW], 1]) == 1
    plain = B.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, pt, r)
    bl = LM.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, lan, lan_row, pt, r)
    assert kW in members(plain.bk_cand_mask[0]) and kW not in members(bl.bk_cand_mask[0]) and (0, kW) in bl.refused
    assert bl.bk_kind[0] == B.ECMP and bl.bk_flags[0] == LM.LAN_PRIMARY | LM.LAN_REFUSED


def mixed_repairs(n_slots):
    """A per-slot repair table with something on offer everywhere: HSPF_TILFA_NODE on even slots, HSPF_TILFA_PAIR on odd ones."""
    import types
    k = np.arange(n_slots, dtype=np.uint32)
    return types.SimpleNamespace(ti_kind=(1 + (k & 1)).astype(np.uint8), ti_via=k, ti_metric=np.full(n_slots, 7, np.uint32))


def test_backup_model_a_lan_primary_never_takes_the_per_link_repair():
    graph, root = lone_candidate()
    c, lan, _, lanm, t, roots, nbr_row, lan_row = models(graph, root)
    pt = B.table([[(5, 0)], [(8, 0)], [(9, 0)]])
    r = B.routes(t.dist, t.flags, t.mask, 0, pt)
    ti = mixed_repairs(64)
    plain = B.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, pt, r, 0, ti)
    bl = LM.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, lan, lan_row, pt, r, 0, ti)
    kC = int(np.flatnonzero((c.nbr == 4) & (lan == M.NONE))[0])
    assert plain.bk_kind.tolist() == [B.LFA, B.NODE, B.PAIR] and plain.bk_slot[0] == kC
    assert bl.bk_kind.tolist() == [B.NOTHING, B.NODE, B.PAIR]                 # D: C refused, a repair on offer, not taken
    assert lan[bl.bk_primary[0]] == 0 and ti.ti_kind[bl.bk_primary[0]] != 0 and bl.bk_flags[0] == LM.LAN_PRIMARY | LM.LAN_REFUSED
    assert lan[bl.bk_primary[1]] == M.NONE and lan[bl.bk_primary[2]] == M.NONE and not bl.bk_flags[1:].any()
    assert bl.bk_coverage.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]


CAND_CASES = {"trap": trap, "two_lans": two_lans, "random": lambda: (random_graph(2), 25)}


@pytest.mark.parametrize("name", sorted(CAND_CASES))
def test_lan_candidates_equal_the_model(name):
    from holo_amd import engine as E
    graph, root = CAND_CASES[name]()
    want = LM.lan_candidates(*graph, root)
    got = E.lfa_lan_candidates(*graph, root)
    assert np.array_equal(got, want), (got, want)
    c = M.candidates(*graph, root)
    for k in range(len(want)):                                                 # all slots behind one link of S agree
        assert want[k] == want[int(c.root_link[k])]
    if name == "trap":                                                        # S's row: L, C, F; then L's row: S, E, A
        assert want.tolist() == [L_, M.NONE, M.NONE, L_, L_, L_]
    cut = E.lfa_lan_candidates(*graph, root, cap=2)
    assert np.array_equal(cut, want[:2])


def test_lan_candidates_raw_call_cap_and_bad_arguments():
    from holo_amd import _lib
    (rp, col, met, vf), root = trap()
    want = LM.lan_candidates(rp, col, met, vf, root)
    lib = _lib.load()
    csr = _lib.HspfCsr(8, len(col), rp.ctypes.data_as(_lib.u32p), col.ctypes.data_as(_lib.u32p), met.ctypes.data_as(_lib.u32p),
                       vf.ctypes.data_as(_lib.u8p), MAXP)
    lan = np.full(8, 0xABCD, np.uint32)
    total = ctypes.c_uint32()
    assert lib.hspf_lfa_lan_candidates(ctypes.byref(csr), root, 4, lan.ctypes.data_as(_lib.u32p), ctypes.byref(total)) == 6 and total.value == 6
    assert np.array_equal(lan[:4], want[:4]) and (lan[4:] == 0xABCD).all()
    assert lib.hspf_lfa_lan_candidates(ctypes.byref(csr), root, 0, None, None) == 6
    assert lib.hspf_lfa_lan_candidates(ctypes.byref(csr), 8, 0, None, None) == -1          # root out of range
    assert lib.hspf_lfa_lan_candidates(None, 0, 0, None, None) == -1
