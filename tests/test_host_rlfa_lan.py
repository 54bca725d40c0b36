"""Remote LFA with LAN-safe spaces on the CPU side: the model (tests/_rlfa_lan_model.py) pinned on hand-checked graphs and on a
property that does not use its inequalities at all (the oracle on the graph WITHOUT the LAN), its equivalence with the plain
model when no slot crosses a LAN, the backup model with and without HSPF_LFA_LAN_SAFE_REPAIRS, and header / ctypes / library
agreeing on the new symbol and constants."""
import ctypes
import os
import re

import numpy as np
import pytest

import _backup_model as B
import _lfa_model as M
import _rlfa_lan_model as RL
import _rlfa_model as R
import _tilfa_model as T
import test_host_lfa_lan as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXP = 0xFFFFFFFF
NONE, SELF = M.NONE, R.VIA_SELF
P_, XP_, Q_, EL_ = R.IN_P, R.IN_XP, R.IN_Q, R.ELIGIBLE
L_, S_, E_, A_, C_, D_, F_, T_, X_ = range(9)


def trap_x():
    """test_host_lfa_lan.trap() plus a stub X behind A (cost 1).  For the slot S -> L -> E the cheapest plain PQ nodes are A, C
    and X: S tunnels to A and X ACROSS L, and C reaches E across L (C - A - L - E).  F (S - F 10, F - E 14) needs L for neither."""
    (rp, col, met, vf), root = HL.trap()
    links = [(u, int(col[k]), int(met[k])) for u in range(8) for k in range(rp[u], rp[u + 1])] + M.both([(A_, X_, 1)])
    return M.csr(9, links, net=[L_]), root


def q_only():
    """S = 1, E = 2 and V = 3 on LAN 0 (router -> LAN 10, 10, 1); p2p S - V 5, S - F 10 (F = 4), F - E 14.  V is released by S
    without the LAN (5 < 10) but reaches E across it (V - L - E = 1): only Q fails."""
    links = [(1, 0, 10), (0, 1, 0), (2, 0, 10), (0, 2, 0), (3, 0, 1), (0, 3, 0)] + M.both([(1, 3, 5), (1, 4, 10), (4, 2, 14)])
    return M.csr(5, links, net=[0]), 1


def via_only():
    """S = 1, E = 2 and A = 3 on LAN 0 (10, 10, 1); p2p S - A 10, E - W 1 (W = 5), S - F 12 (F = 4), F - E 14.  W is in no P-space;
    its cheapest release is by the neighbour A, which sits on the LAN and reaches W across it (A - L - E - W = 2 = d(A, L) +
    d(L, W)): that via-slot fails, F's (12 + 15) does not."""
    links = [(1, 0, 10), (0, 1, 0), (2, 0, 10), (0, 2, 0), (3, 0, 1), (0, 3, 0)] + M.both([(1, 3, 10), (2, 5, 1), (1, 4, 12), (4, 2, 14)])
    return M.csr(6, links, net=[0]), 1


def slot_of(m, E, across):
    """The candidate slot whose neighbour is E and whose LAN is `across` (NONE: the point-to-point slot)."""
    return int(np.flatnonzero((m["cand"].nbr == E) & (m["lan"] == across))[0])


def triple(rl, e):
    return int(rl.pq_node[e]), int(rl.pq_via[e]), int(rl.pq_metric[e])


def test_header_ctypes_and_library_agree_on_the_new_symbols():
    from holo_amd import build, _lib, engine as E
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"\bint hspf_rlfa_lan_device\(([^;]*?)\);", hdr, re.S)
    assert m, "hspf_rlfa_lan_device is not declared"
    assert len(m.group(1).split(",")) == 15
    assert hasattr(lib, "hspf_rlfa_lan_device")
    assert table["hspf_rlfa_lan_device"][0] is ctypes.c_int and len(table["hspf_rlfa_lan_device"][1]) == 15
    assert lib.hspf_abi_version() == 8                                   # additions only
    for c_name, py in (("HSPF_RLFA_LAN_COUNT_WORDS", E.RLFA_LAN_COUNT_WORDS), ("HSPF_RLFA_LAN_COVERAGE_WORDS", E.RLFA_LAN_COVERAGE_WORDS),
                       ("HSPF_LFA_LAN_SAFE_REPAIRS", E.LFA_LAN_SAFE_REPAIRS), ("HSPF_LFA_IGNORE_OVERLOAD", E.LFA_IGNORE_OVERLOAD)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py, c_name
    assert (RL.COUNT_WORDS, RL.COVERAGE_WORDS, RL.LAN_SAFE_REPAIRS) == (E.RLFA_LAN_COUNT_WORDS, E.RLFA_LAN_COVERAGE_WORDS, E.LFA_LAN_SAFE_REPAIRS) == (5, 6, 2)
    assert ctypes.sizeof(_lib.HspfRlfaOut) == 72                         # hspf_rlfa_out did not grow


def test_trap_the_plain_pq_nodes_tunnel_crosses_the_lan():
    m = RL.one_root(*trap_x())
    rl, e = m["rl"], slot_of(m, E_, L_)
    assert triple(rl.plain, e) == (A_, SELF, 10)                         # d(S, A) = 10 is S - L - A
    assert triple(rl, e) == (F_, SELF, 10)
    assert rl.plain.pq_counts[e].tolist() == [4, 7, 7, 7] and rl.pq_counts[e].tolist() == [2, 7, 4, 4, 3]
    # A and X: S's own path crosses L (10 = d(S, L) + 0), C releases them (1 < 2 + 0), none of the three reaches E without L
    assert [int(rl.plain.space_flags[e][v]) for v in (A_, C_, X_)] == [P_ | XP_ | Q_ | EL_] * 3
    assert [int(rl.space_flags[e][v]) for v in (A_, C_, X_)] == [XP_ | EL_, P_ | XP_ | EL_, XP_ | EL_]
    kC = slot_of(m, C_, NONE)
    assert rl.space_via[e][A_] == kC and rl.plain.space_via[e][A_] == SELF
    assert int(rl.space_flags[e][F_]) == P_ | XP_ | Q_ | EL_ and int(rl.space_flags[e][D_]) == int(rl.plain.space_flags[e][D_]) == XP_ | Q_ | EL_
    for k in (kC, slot_of(m, F_, NONE)):                                  # the point-to-point slots: the plain answer
        assert triple(rl, k) == triple(rl.plain, k) and rl.pq_counts[k].tolist() == rl.plain.pq_counts[k].tolist() + [0]
        assert np.array_equal(rl.space_flags[k], rl.plain.space_flags[k]) and np.array_equal(rl.space_via[k], rl.plain.space_via[k])
    assert rl.rl_coverage.tolist()[:4] == rl.plain.rl_coverage.tolist() and rl.rl_coverage[4] == 5


def test_only_q_fails_the_node_reaches_e_through_the_lan():
    m = RL.one_root(*q_only())
    rl, e = m["rl"], slot_of(m, 2, 0)
    assert triple(rl.plain, e) == (3, SELF, 5) and triple(rl, e) == (4, SELF, 10)
    assert int(rl.plain.space_flags[e][3]) == P_ | XP_ | Q_ | EL_ and int(rl.space_flags[e][3]) == P_ | XP_ | EL_
    assert rl.space_via[e][3] == SELF and rl.pq_counts[e].tolist() == [2, 3, 2, 2, 1]


def test_only_the_via_slot_fails_the_neighbour_sits_on_the_lan():
    m = RL.one_root(*via_only())
    rl, e = m["rl"], slot_of(m, 2, 0)
    kA, kF, W = slot_of(m, 3, NONE), slot_of(m, 4, NONE), 5
    assert int(rl.plain.space_flags[e][W]) == int(rl.space_flags[e][W]) == XP_ | Q_ | EL_      # W stays in XP and Q ...
    assert rl.plain.space_via[e][W] == kA and rl.space_via[e][W] == kF                          # ... released by F instead of A
    assert int(m["cand"].cost[kA]) + int(m["fwd"].dist[m["nbr_row"][kA], W]) == 12 and int(m["cand"].cost[kF]) + int(m["fwd"].dist[m["nbr_row"][kF], W]) == 27
    assert triple(rl.plain, e) == (3, SELF, 10) and triple(rl, e) == (4, SELF, 12)
    # the slot that protects S - L - A: A itself is released by its point-to-point slot
    assert triple(rl, slot_of(m, 3, 0)) == (3, kA, 10)


def test_root_on_two_lans_in_one_chunk():
    m = RL.one_root(*HL.two_lans())
    rl, lan = m["rl"], m["lan"]
    cands = np.flatnonzero(m["cand"].nbr != NONE)
    assert len(cands) <= 8 and sorted({int(x) for x in lan[cands] if x != NONE}) == [0, 1]      # both LANs in the first chunk
    e1, ex, e2 = slot_of(m, 3, 0), slot_of(m, 6, 0), slot_of(m, 4, 1)
    # X = 6 and E1 = 3 are reached across LAN 0; D = 5 is released by E2 behind LAN 1 (5 + 5) and reaches both without LAN 0
    assert triple(rl.plain, e1) == (6, SELF, 5) and triple(rl, e1) == (5, e2, 10)
    assert triple(rl.plain, ex) == (3, SELF, 5) and triple(rl, ex) == (5, e2, 10)
    assert triple(rl, e2) == triple(rl.plain, e2) and rl.pq_counts[e2][4] == 0                  # LAN 1: nothing crosses it
    assert rl.pq_counts[e1][4] == 1 and rl.pq_counts[ex][4] == 1


def _check_graph(graph):
    """The property on one graph, every router root: returns (slots whose PQ node changes, slots that lose it, lost slots that a
    TI-LFA pair repairs, LAN slots)."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    n_changed = n_lost = n_pair = n_slots = 0
    for root in range(len(vf)):
        if vf[root] & M.VF_NETWORK or not (HL.LM.lan_candidates(*graph, root) != NONE).any():
            continue
        m = RL.one_root(graph, root)
        c, lan, nbr_row, rl, fwd, rdist = m["cand"], m["lan"], m["nbr_row"], m["rl"], m["fwd"], m["rdist"]
        ti = RL.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, 0, nbr_row, rl, m["lfa"].alt_flags)
        cut = {}
        for e in np.flatnonzero((c.nbr != NONE) & (lan != NONE)):
            e = int(e)
            n_slots += 1
            Lv = int(lan[e])
            if Lv not in cut:
                cut[Lv] = R.tables(HL.without_vertices(graph, {Lv}), MAXP, m["roots"], 0, m["W"])
            cfwd, crdist = cut[Lv]
            lf, pf = rl.space_flags[e], rl.plain.space_flags[e]
            assert not ((lf & 7) & ~(pf & 7)).any() and np.array_equal(lf & EL_, pf & EL_), (root, e)      # subsets, bit by bit
            for v in np.flatnonzero(((lf & (P_ | XP_)) != 0) & ((lf & Q_) != 0)):
                via = int(rl.space_via[e][v])
                row = 0 if via == SELF else int(nbr_row[via])
                assert cfwd.dist[row, v] == fwd.dist[row, v], (root, e, v, "release path")
                assert crdist[nbr_row[e], v] == rdist[nbr_row[e], v], (root, e, v, "path on to E")
            d_cut = int(cfwd.dist[0, int(c.nbr[e])])                                           # d(S, E) without L
            if ti.ti_kind[e] != T.KIND_NONE:
                assert d_cut != M.NONE and int(ti.ti_metric[e]) >= d_cut, (root, e)
            had, has = rl.plain.pq_node[e] != NONE, rl.pq_node[e] != NONE
            n_changed += bool(had and has and rl.plain.pq_node[e] != rl.pq_node[e])
            n_lost += bool(had and not has)
            n_pair += bool(had and not has and ti.ti_kind[e] == T.KIND_PAIR)
    return n_changed, n_lost, n_pair, n_slots


def test_property_lan_safe_tunnels_do_not_need_the_lan():
    totals = np.zeros(4, np.int64)
    for seed in range(12):
        totals += _check_graph(HL.random_graph(seed))
    print("changed / lost / lost and repaired by a pair / LAN slots:", totals.tolist())
    assert totals[0] >= 1 and totals[1] >= 1 and totals[2] >= 1, totals
    assert totals[:2].tolist() == [576, 128] and totals[3] == 1134, totals          # the figures of the issue


@pytest.mark.parametrize("which", ["trap_x", "two_lans", "random"])
def test_without_lans_the_model_is_the_plain_model(which):
    graph, root = trap_x() if which == "trap_x" else HL.two_lans() if which == "two_lans" else (HL.random_graph(3), 20)
    m = RL.one_root(graph, root, no_lans=True)
    rl = m["rl"]
    for f in R.FIELDS:
        got, want = getattr(rl, f), getattr(rl.plain, f)
        if f == "pq_counts":
            assert np.array_equal(got[:, :4], want) and not got[:, 4].any()
        elif f == "rl_coverage":
            assert np.array_equal(got[:4], want) and not got[4:].any()
        else:
            assert np.array_equal(got, want), f


def test_backup_model_with_and_without_lan_safe_repairs():
    graph, root = HL.lone_candidate()
    c, lan, _, lanm, t, roots, nbr_row, lan_row = HL.models(graph, root)
    pt = B.table([[(5, 0)], [(8, 0)], [(9, 0)]])
    r = B.routes(t.dist, t.flags, t.mask, 0, pt)
    ti = HL.mixed_repairs(64)
    args = (t.dist, t.flags, t.mask, c, 0, nbr_row, lan, lan_row, pt, r)
    off, today = RL.backup(*args, 0, ti), HL.LM.backup(*args, 0, ti)
    for f in B.FIELDS:
        assert np.array_equal(getattr(off, f), getattr(today, f)), f
    assert off.bk_kind.tolist() == [B.NOTHING, B.NODE, B.PAIR]
    on = RL.backup(*args, RL.LAN_SAFE_REPAIRS, ti)
    e = int(on.bk_primary[0])
    assert lan[e] == 0 and e == int(off.bk_primary[0])
    assert on.bk_kind[0] == (B.NODE if ti.ti_kind[e] == 1 else B.PAIR) and on.bk_slot[0] == ti.ti_via[e] and on.bk_metric[0] == 7
    assert on.bk_kind.tolist()[1:] == [B.NODE, B.PAIR] and on.bk_flags.tolist() == off.bk_flags.tolist()
    assert int(on.bk_coverage[:7].sum()) == 3 and on.bk_coverage[B.NOTHING] == 0 and on.bk_coverage[7:].tolist() == [1, 1]
    assert RL.backup(*args, RL.LAN_SAFE_REPAIRS, None).bk_kind.tolist() == [B.NOTHING] * 3                  # no repairs given: nothing to take
