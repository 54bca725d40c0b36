"""TI-LFA repairs along the post-convergence path on the CPU side.  The product code under test is the sequential host twin
(hspf::host::tilfa_pc_sequential in include/holo_spf_host.hpp, through the `host` leg of tests/cpp/tilfa_pc_driver.cpp): on the hand
cases against expectations worked out by hand and against the model (tests/_tilfa_pc_model.py), on 40 instances of the IS-IS / OSPF
generators and on the asymmetric sweep against the model; every repair it returns is checked independently, with the oracle and
without any walk; the promise towards hspf_tilfa_device on symmetric graphs; the symbol in header, ctypes table and library."""
import ctypes
import os
import re

import numpy as np
import pytest

import _failure_cases as F
import _lfa_model as M
import _rlfa_model as R
import _tilfa_model as T
import _tilfa_pc_cases as C
import _tilfa_pc_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXP = 0xFFFFFFFF


def test_header_ctypes_and_library_agree_on_the_new_symbol():
    from holo_amd import build, _lib
    from holo_amd import engine as E
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    m = re.search(r"\bint hspf_tilfa_pc_device\(([^;]*?)\);", hdr, re.S)
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert m and len(m.group(1).split(",")) == 21 and hasattr(lib, "hspf_tilfa_pc_device")
    assert table["hspf_tilfa_pc_device"][0] is ctypes.c_int and len(table["hspf_tilfa_pc_device"][1]) == 21
    assert lib.hspf_abi_version() == 8                                   # an addition only
    s = re.search(r"typedef struct \{([^}]*)\} hspf_tilfa_pc_out;", hdr, re.S).group(1)
    assert tuple(re.findall(r"\*(\w+);", s)) == tuple(n for n, _ in _lib.HspfTilfaPcOut._fields_) == P.FIELDS == E.TILFA_PC_FIELDS
    for k, v in (("MAX_ADJ", P.MAX_ADJ), ("D_LFA", P.D_LFA), ("D_REPAIR", P.D_REPAIR), ("D_NONE", P.D_NONE), ("D_LONG", P.D_LONG), ("D_LAN", P.D_LAN),
                 ("D_WALK", P.D_WALK), ("ON_PC", P.ON_PC), ("P_IS_ROOT", P.P_IS_ROOT), ("Q_IS_DEST", P.Q_IS_DEST), ("COVERAGE_WORDS", 12)):
        assert int(re.search(r"#define HSPF_TIPC_" + k + r"\s+(\w+)u", hdr).group(1), 0) == v == getattr(E, "TIPC_" + k), k
    assert lib.hspf_tilfa_pc_device(None, None, 0, 0, 0, None, None, None, None, None, 0, 0, None, None, None, None, 0, None, 0, 1, None) == -1      # a NULL context


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_twin_and_model_give_the_hand_written_repairs(name, tmp_path):
    from oracle import graph_oracle as go
    go.build()
    c = C.CASES[name]
    assert len(c.graph[3]) <= 12
    wants = [c.want(w_min) for w_min in (1, 2)]
    for w, got in zip(wants, C.twin(tmp_path, [(w, c.lfa_flags, False, c.max_walk) for w in wants], name)):
        C.check_expect(w.tp, c.expect, name)
        C.check_expect(got, c.expect, name + " (twin)")
        C.same(got, w.tp, name)
        assert got.tp_coverage.tolist() == P.recount(got.tp_kind, got.tp_n_adj)
        check_repairs(w, got)


def test_hand_cases_show_every_class_and_every_length():
    kinds, lens, flags = set(), set(), set()
    for c in C.CASES.values():
        tp = c.want().tp
        kinds |= set(tp.tp_kind.tolist())
        rep = tp.tp_kind == P.D_REPAIR
        lens |= set(tp.tp_n_adj[rep].tolist())
        flags |= set(tp.tp_flags[rep].tolist())
    assert kinds == {0, P.D_REPAIR, P.D_NONE, P.D_LONG, P.D_LAN, P.D_WALK} and lens == {0, 1, 2, 3, 4}      # (_D_LFA: the sweeps, which pass alt_flags)
    assert any(f & P.P_IS_ROOT for f in flags) and any(f & P.Q_IS_DEST for f in flags) and any(not f & P.ON_PC for f in flags)


# ---- every repair checked without the walk --------------------------------------------------------------------------------------

def dist_from(graph, maxp, v, run_flags=0):
    from oracle import graph_oracle as go
    return go.run(*graph, maxp, np.array([v], np.uint32), run_flags, go.MAP, mask_words_=4).dist[0]


def check_repairs(w: P.Want, tp=None):
    """Each _D_REPAIR of one root (tp: the twin's result; None: the model's): the hops exist in the CSR, chain up from p to q and are not the failed link; q's distance to D
    is the same with and without the link; the release path to p avoids the link (hspf_rlfa_device's P / XP inequality, from the
    oracle's rows); with _ON_PC the metric is the failure row's distance."""
    rp, col, met, vf = w.graph
    S, tp, c = w.root, w.tp if tp is None else tp, w.cand
    checked = 0
    cut = {}
    for D in np.flatnonzero(tp.tp_kind == P.D_REPAIR):
        D = int(D)
        e = [k for k in range(len(c.nbr)) if (int(w.fwd.mask[0, D, k // 64]) >> (k % 64)) & 1]
        assert len(e) == 1
        e = e[0]
        E, cst, fpos = int(c.nbr[e]), int(c.cost[e]), int(c.root_link[e])
        p, q, via, na = int(tp.tp_p[D]), int(tp.tp_q[D]), int(tp.tp_via[D]), int(tp.tp_n_adj[D])
        tail, walked = p, 0
        for h in range(na):
            j, head = int(tp.tp_hop_pos[D, h]), int(tp.tp_hop_head[D, h])
            assert j < rp[tail + 1] - rp[tail] and col[rp[tail] + j] == head and not (tail == S and j == fpos), (D, h)
            assert tail in col[rp[head]:rp[head + 1]]                                           # two-way
            walked += int(met[rp[tail] + j])
            tail = head
        assert tail == q
        # q -> D does not cross the link
        if e not in cut:
            g2 = F.retarget(w.graph, S, F.ROOT_LINK, fpos)
            cut[e] = (g2, {})
        g2, memo = cut[e]
        if q != D:
            if q not in memo:
                memo[q] = (dist_from(w.graph, w.maxp, q, w.run_flags), dist_from(g2, w.maxp, q, w.run_flags)[:len(vf)])
            assert memo[q][0][D] == memo[q][1][D] != P.INF, (D, q)
        # S -> p: the release inequality, from rows the walk never read
        dE = w.fwd.dist[w.nbr_row[e]]
        if p == S:
            assert via == P.NONE and tp.tp_flags[D] & P.P_IS_ROOT
            rel = 0
        elif via == P.VIA_SELF:
            rel = int(w.fwd.dist[0, p])
            assert rel < cst + int(dE[p])
        else:
            dN = w.fwd.dist[w.nbr_row[via]]
            assert c.nbr[via] != P.NONE and c.root_link[via] != fpos and int(dN[p]) < int(dN[S]) + cst + int(dE[p])
            rel = int(c.cost[via]) + int(dN[p])
        row = w.pc[e]
        total = rel + walked
        if tp.tp_flags[D] & P.ON_PC:
            assert tp.tp_metric[D] == row[D], (D, int(tp.tp_metric[D]), int(row[D]))
        assert tp.tp_metric[D] == min(rel + int(row[D]) - (0 if p == S else int(row[p])), P.SAT)
        if not vf[col[rp[S] + fpos]] & 1:                      # a point-to-point slot: the release path is a path of the failure run, never shorter than its row
            assert tp.tp_metric[D] >= min(int(row[D]), P.SAT)  # (behind a pseudonode the plain P / XP sets are relative to E, not to the link: out of scope)
        assert total + (0 if q == D else int(row[D]) - int(row[q])) == rel + int(row[D]) - (0 if p == S else int(row[p]))      # the hops are tight
        checked += 1
    return checked


def test_every_repair_of_the_hand_cases_holds(tmp_path):
    wants = [c.want() for c in C.CASES.values()]
    outs = C.twin(tmp_path, [(w, c.lfa_flags, False, c.max_walk) for w, c in zip(wants, C.CASES.values())])
    assert sum(check_repairs(w, got) for w, got in zip(wants, outs)) >= 25


def test_twin_on_forty_protocol_instances(tmp_path):
    """40 instances of the IS-IS / OSPF generators, every router as the root: the twin equals the model, and every repair holds."""
    wants = []
    for seed in range(40):
        graph, maxp, run_flags = F.protocol_graph(seed)
        lf = M.IGNORE_OVERLOAD if run_flags & 2 else 0
        for root in np.flatnonzero((graph[3] & 1) == 0):
            wants.append((P.one_root(graph, int(root), maxp, run_flags, lf, with_lfa=bool(seed % 2)), lf, bool(seed % 2), 256))
    checked, kinds = 0, set()
    for (w, *_), got in zip(wants, C.twin(tmp_path, wants)):
        C.same(got, w.tp, (w.root, len(w.graph[3])))
        checked += check_repairs(w, got)
        kinds |= set(got.tp_kind.tolist())
    assert checked >= 300 and {P.D_LFA, P.D_REPAIR, P.D_NONE, P.D_LAN} <= kinds, (checked, kinds)


def test_twin_on_the_asymmetric_sweep(tmp_path):
    """The 40 graphs of the GPU sweep (30 to 60 routers, a cost per direction), one root each, no alt_flags: every length 0 .. 4."""
    wants = []
    for seed in range(40):
        g = C.sweep_graph(seed)
        wants.append((P.one_root(g, (seed * 11) % len(g[3]), with_lfa=False), 0, False, 256))
    checked, lens = 0, set()
    for (w, *_), got in zip(wants, C.twin(tmp_path, wants)):
        C.same(got, w.tp, w.root)
        checked += check_repairs(w, got)
        lens |= set(got.tp_n_adj[got.tp_kind == P.D_REPAIR].tolist())
    assert checked >= 1000 and lens == {0, 1, 2, 3, 4}, (checked, lens)


# ---- towards hspf_tilfa_device ---------------------------------------------------------------------------------------------------

def test_on_symmetric_graphs_the_repair_of_e_is_the_two_segment_repair(tmp_path):
    """The sweep graphs of tests/test_host_tilfa.py (routers only, symmetric costs >= 1, no overload), D = E of every candidate
    slot whose link is E's one primary, on the TWIN's result: at most one adjacency, a repair wherever hspf_tilfa_device has one and
    never a cheaper one; with _ON_PC exactly its metric.  (Without _ON_PC — p released by a neighbour off the post-convergence path
    — the metric is larger: hspf_tilfa_device picks the cheapest p, the walk the p the path meets first.  So tp_metric ==
    ti_metric does not hold for every such D and is not asserted.)"""
    from test_host_tilfa import N_GRAPHS, _random_graph
    r = np.random.default_rng(20240611)
    wants = []
    for _ in range(N_GRAPHS):
        n, und = _random_graph(r)
        S = int(r.integers(0, n))
        wants.append((P.one_root(M.csr(n, M.both(und)), S, with_lfa=False), 0, False, 256))
    applied = with_adj = on_pc = 0
    for (w, *_), tp in zip(wants, C.twin(tmp_path, wants)):
        C.same(tp, w.tp, w.root)
        t = T.tilfa(w.fwd.dist, w.fwd.flags, w.fwd.mask, w.rdist, w.graph, w.cand, 0, w.nbr_row, w.rl.space_flags, w.rl.space_via, None)
        for e in np.flatnonzero(w.cand.nbr != M.NONE):
            E = int(w.cand.nbr[e])
            if tp.tp_kind[E] == 0 or int(w.fwd.mask[0, E, e // 64]) >> (e % 64) & 1 == 0:
                continue                                                # E has other primaries: not in the population
            assert tp.tp_kind[E] == P.D_REPAIR and t.ti_kind[e] != T.KIND_NONE, (w.root, e)
            assert tp.tp_n_adj[E] <= 1 and tp.tp_metric[E] >= t.ti_metric[e], (w.root, e, int(tp.tp_n_adj[E]), int(tp.tp_metric[E]), int(t.ti_metric[e]))
            if tp.tp_flags[E] & P.ON_PC:
                assert tp.tp_metric[E] == t.ti_metric[e], (w.root, e)
                on_pc += 1
            applied += 1
            with_adj += int(tp.tp_n_adj[E])
    assert applied >= N_GRAPHS and with_adj > 0 and on_pc > 0, (applied, with_adj, on_pc)


def test_the_python_layer_has_the_calls():
    import inspect
    from holo_amd import engine as E
    assert "pc_row" in inspect.signature(E.SpfContext.tilfa_pc_device).parameters
    assert "max_walk" in inspect.signature(E.SpfContext.tilfa_pc).parameters
    tp = E.TilfaPcResult(*(np.zeros((1, 2) + ((4,) if "hop" in k else ()), np.uint32) for k in E.TILFA_PC_FIELDS))
    assert tp.segments(1) is None
