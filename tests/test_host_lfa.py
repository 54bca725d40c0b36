"""Loop-free alternates on the CPU side: the two new symbols in header, ctypes table and library; hspf_lfa_candidates (pure host
arithmetic, no context) against the model's restatement of the candidate table; and the model itself pinned on hand-checked
RFC 5286 textbook cases, so that what the GPU tests compare against is checked independently of the engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lfa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXP = 0xFFFFFFFF


def test_header_ctypes_and_library_agree_on_the_two_symbols():
    from holo_amd import build, _lib
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, n_args in (("hspf_lfa_candidates", 8), ("hspf_lfa_device", 11)):
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert table[name][0] is ctypes.c_int and len(table[name][1]) == n_args
    assert lib.hspf_abi_version() == 8                                   # additions only
    from holo_amd import engine as E
    for c_name, py in (("HSPF_LFA_C_NO_TRANSIT", E.LFA_C_NO_TRANSIT), ("HSPF_LFA_IGNORE_OVERLOAD", E.LFA_IGNORE_OVERLOAD),
                       ("HSPF_LFA_HAS_PRIMARY", E.LFA_HAS_PRIMARY), ("HSPF_LFA_ECMP", E.LFA_ECMP), ("HSPF_LFA_LINK_PROTECT", E.LFA_LINK_PROTECT),
                       ("HSPF_LFA_NODE_PROTECT", E.LFA_NODE_PROTECT), ("HSPF_LFA_DOWNSTREAM", E.LFA_DOWNSTREAM), ("HSPF_LFA_NO_SLOT", E.LFA_NO_SLOT),
                       ("HSPF_LFA_COVERAGE_WORDS", E.LFA_COVERAGE_WORDS)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py, c_name
    assert (M.HAS_PRIMARY, M.ECMP, M.LINK_PROTECT, M.NODE_PROTECT, M.DOWNSTREAM) == (E.LFA_HAS_PRIMARY, E.LFA_ECMP, E.LFA_LINK_PROTECT,
                                                                                   E.LFA_NODE_PROTECT, E.LFA_DOWNSTREAM)


def _square_parallel():
    # routers 0..3 in a ring, a second (parallel, dearer) link 0 - 1
    return M.csr(4, M.both([(0, 1, 1), (0, 1, 5), (1, 2, 1), (2, 3, 1), (3, 0, 1)])), 0


def _lan():
    # vertex 0 = pseudonode of a LAN with routers 1, 2, 3 (router -> LAN costs 10, LAN -> router 0), plus a p2p link 1 - 3
    links = []
    for r in (1, 2, 3):
        links += [(r, 0, 10), (0, r, 0)]
    links += M.both([(1, 3, 7)])
    return M.csr(4, links, net=[0]), 1


def _net_chain():
    # root 2 -> network 0 -> network 1 -> router 3; router 4 on network 0
    links = [(2, 0, 3), (0, 2, 0), (0, 1, 2), (1, 0, 2), (1, 3, 0), (3, 1, 4), (0, 4, 0), (4, 0, 9)]
    return M.csr(5, links, net=[0, 1]), 2


def _one_way():
    # 0 lists 1, 2 and 3; 2 does not list 0
    return M.csr(4, [(0, 1, 1), (1, 0, 1), (0, 2, 1), (0, 3, 2), (3, 0, 2), (2, 3, 1), (3, 2, 1)], no_transit=[3]), 0


def _hub70():
    links = []
    for k in range(1, 71):
        links += [(0, k, k), (k, 0, k)]
    return M.csr(71, links, no_transit=[5, 69]), 0


CASES = {"square_parallel": _square_parallel, "lan": _lan, "net_chain": _net_chain, "one_way": _one_way, "hub70": _hub70}


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_equal_the_model(name):
    from holo_amd import engine as E
    (rp, col, met, vf), root = CASES[name]()
    want = M.candidates(rp, col, met, vf, root)
    got = E.lfa_candidates(rp, col, met, vf, root)
    assert got.total_slots == len(want.nbr) == got.n_slots
    assert np.array_equal(got.nbr, want.nbr), (got.nbr, want.nbr)
    assert np.array_equal(got.cost, want.cost)
    assert np.array_equal(got.root_link, want.root_link)
    assert np.array_equal(got.cflags, want.cflags)
    # what the cases are there for
    if name == "square_parallel":
        assert want.nbr.tolist() == [1, 1, 3] and want.root_link.tolist() == [0, 1, 2] and want.cost.tolist() == [1, 5, 1]
    if name == "lan":          # slot 0: the LAN (no candidate), slot 1: p2p to 3, slots 2..4: the LAN's links to 1 (the root), 2, 3
        assert want.nbr.tolist() == [M.NONE, 3, M.NONE, 2, 3] and want.root_link.tolist() == [0, 1, 0, 0, 0] and want.cost.tolist() == [10, 7, 10, 10, 10]
    if name == "net_chain":    # root row | network 0's row | network 1's row
        assert want.nbr.tolist() == [M.NONE, M.NONE, M.NONE, 4, M.NONE, 3] and want.cost.tolist() == [3, 3, 5, 3, 7, 5]
    if name == "one_way":
        assert want.nbr.tolist() == [1, M.NONE, 3] and want.cflags.tolist() == [0, 0, M.C_NO_TRANSIT]
    if name == "hub70":
        assert len(want.nbr) == 70 and want.cflags[4] == M.C_NO_TRANSIT and want.cflags[68] == M.C_NO_TRANSIT and want.cflags.sum() == 2


def test_candidates_cap_smaller_than_the_slot_count_and_bad_arguments():
    from holo_amd import _lib, engine as E
    (rp, col, met, vf), root = _hub70()
    want = M.candidates(rp, col, met, vf, root)
    got = E.lfa_candidates(rp, col, met, vf, root, cap=10)
    assert got.total_slots == 70 and got.n_slots == 10
    assert np.array_equal(got.nbr, want.nbr[:10]) and np.array_equal(got.cost, want.cost[:10])
    # the raw call: nothing behind `cap` is written, NULL arrays are skipped, the count comes back either way
    lib = _lib.load()
    csr = _lib.HspfCsr(71, len(col), rp.ctypes.data_as(_lib.u32p), col.ctypes.data_as(_lib.u32p), met.ctypes.data_as(_lib.u32p),
                       vf.ctypes.data_as(_lib.u8p), MAXP)
    nbr = np.full(12, 0xABCD, np.uint32)
    assert lib.hspf_lfa_candidates(ctypes.byref(csr), 0, 10, nbr.ctypes.data_as(_lib.u32p), None, None, None, None) == 70
    assert np.array_equal(nbr[:10], want.nbr[:10]) and nbr[10] == 0xABCD and nbr[11] == 0xABCD
    assert lib.hspf_lfa_candidates(ctypes.byref(csr), 71, 0, None, None, None, None, None) == -1      # root out of range
    assert lib.hspf_lfa_candidates(None, 0, 0, None, None, None, None, None) == -1


# ---- the model on hand-checked textbook cases (RFC 5286 section 3: inequalities 1, 2 and 3) ------------------------------------

def _model(graph, root, run_flags=0, lfa_flags=0):
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64)
    t = go.run(rp, col, met, vf, MAXP, roots, run_flags, go.MAP, mask_words_=W)
    return c, M.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row, lfa_flags)


def test_model_triangle_equal_costs():
    """S = 0, neighbours 1 and 2, every link 1.  D = 1: the other neighbour is loop-free (1 < 1 + 1) and not on the failed link;
    the primary next hop IS the destination, so there is no node to protect; d(2, 1) = 1 is not below d(0, 1) = 1."""
    c, r = _model(M.csr(3, M.both([(0, 1, 1), (0, 2, 1), (1, 2, 1)])), 0)
    assert c.nbr.tolist() == [1, 2]
    assert r.alt_flags.tolist() == [0, M.HAS_PRIMARY | M.LINK_PROTECT, M.HAS_PRIMARY | M.LINK_PROTECT]
    assert r.alt_slot.tolist() == [M.NONE, 1, 0] and r.alt_metric.tolist() == [0, 2, 2]
    assert r.cand_mask[:, 0].tolist() == [0, 2, 1] and r.node_mask[:, 0].tolist() == [0, 0, 0]
    assert r.coverage.tolist() == [2, 0, 2, 0, 0]


def test_model_square_ring_unit_costs():
    """0 - 1 - 2 - 3 - 0, S = 0.  The far corner 2 is ECMP (no alternate chosen; each primary shares its link with itself only,
    the other primary is not a candidate because it is a primary).  For the adjacent corner 1 the only other neighbour, 3,
    reaches 1 at cost 2 = d(3, 0) + d(0, 1): not loop-free."""
    c, r = _model(M.csr(4, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1)])), 0)
    assert c.nbr.tolist() == [1, 3]
    assert r.alt_flags.tolist() == [0, M.HAS_PRIMARY, M.HAS_PRIMARY | M.ECMP, M.HAS_PRIMARY]
    assert r.alt_slot.tolist() == [M.NONE] * 4 and r.alt_metric.tolist() == [0] * 4
    assert not r.cand_mask.any() and not r.node_mask.any()
    assert r.coverage.tolist() == [3, 1, 0, 0, 0]


def test_model_triangle_with_a_long_third_side():
    """0 - 1 and 0 - 2 cost 1, 1 - 2 costs 3 > 1 + 1: each neighbour reaches the other THROUGH S (2 = 1 + 1, not less)."""
    _c, r = _model(M.csr(3, M.both([(0, 1, 1), (0, 2, 1), (1, 2, 3)])), 0)
    assert r.alt_flags.tolist() == [0, M.HAS_PRIMARY, M.HAS_PRIMARY]
    assert r.alt_slot.tolist() == [M.NONE] * 3 and not r.cand_mask.any()
    assert r.coverage.tolist() == [2, 0, 0, 0, 0]


def test_model_node_protection_and_downstream():
    """S = 0; 0 - 1 (1), 1 - 3 (1), 0 - 2 (1), 2 - 3 (2), 3 - 4 (1).  D = 3 and D = 4 go through 1; neighbour 2 is loop-free
    (2 < 1 + 2) and avoids node 1 (2 < d(2, 1) + d(1, 3) = 2 + 1): node-protecting, alternate metric 1 + 2 = 3 (4 for D = 4);
    d(2, 3) = 2 is not below d(0, 3) = 2: not downstream.  With 2 - 3 at cost 1, D = 3 becomes ECMP instead.  For D = 2 the
    neighbour 1 gives 3 < 1 + 1? no: no alternate."""
    g = M.csr(5, M.both([(0, 1, 1), (1, 3, 1), (0, 2, 1), (2, 3, 2), (3, 4, 1)]))
    _c, r = _model(g, 0)
    HP, LP, NP = M.HAS_PRIMARY, M.LINK_PROTECT, M.NODE_PROTECT
    assert r.alt_flags.tolist() == [0, HP, HP, HP | LP | NP, HP | LP | NP]
    assert r.alt_slot.tolist() == [M.NONE, M.NONE, M.NONE, 1, 1] and r.alt_metric.tolist() == [0, 0, 0, 3, 4]
    assert r.node_mask[:, 0].tolist() == [0, 0, 0, 2, 2]
    assert r.coverage.tolist() == [4, 0, 2, 2, 0]
    # a downstream alternate: make 2 strictly closer to 3 than S is (0 - 1 costs 2 now: d(0, 3) = 3 via either, so lengthen 0 - 2 too)
    g = M.csr(5, M.both([(0, 1, 2), (1, 3, 2), (0, 2, 3), (2, 3, 2), (3, 4, 1)]))
    _c, r = _model(g, 0)
    assert r.alt_flags[3] == HP | LP | NP | M.DOWNSTREAM and r.alt_metric[3] == 5 and r.coverage[4] == 2


def test_model_overloaded_neighbour_and_sums_beyond_32_bits():
    """A neighbour with NO_TRANSIT is an alternate only for itself, unless the call ignores the overload bit; and with wide
    metrics d(N, S) + d(S, D) passes 2^32: in 32 bits the sum would wrap and the inequality flip."""
    g = M.csr(4, M.both([(0, 1, 1), (0, 2, 1), (1, 2, 1), (2, 3, 1), (1, 3, 5)]), no_transit=[2])
    # (the SPTs ignore the overload bit, as a flooding-topology run does, so that 3 stays reachable through 2)
    _c, r = _model(g, 0, run_flags=2)
    assert r.alt_flags[1] == M.HAS_PRIMARY          # D = 1: 2 would do (1 < 1 + 1) but carries no transit traffic
    _c, r2 = _model(g, 0, run_flags=2, lfa_flags=M.IGNORE_OVERLOAD)
    assert r2.alt_flags[1] == M.HAS_PRIMARY | M.LINK_PROTECT and r2.alt_slot[1] == 1
    big = 0x7F000000
    g = M.csr(4, M.both([(0, 1, big), (1, 2, big), (0, 3, big), (3, 2, big + 5)]))
    from oracle import graph_oracle as go
    rp, col, met, vf = g
    c, roots, nbr_row = M.protect_one(rp, col, met, vf, 0)
    t = go.run(rp, col, met, vf, 0xFE000000, roots, 0, go.MAP, mask_words_=1)
    r = M.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row)
    # D = 2 via 1 (0xFE000000); neighbour 3: d(3, 2) = big + 5 < d(3, 0) + d(0, 2) = big + 2 big = 0x17D000000 (wraps to 0x7D000000 in u32)
    assert r.alt_flags[2] == M.HAS_PRIMARY | M.LINK_PROTECT | M.NODE_PROTECT | M.DOWNSTREAM
    assert r.alt_metric[2] == 0xFE000005 and r.alt_slot[2] == 1


def test_model_overloaded_neighbour_protects_only_itself():
    """S = 0; 0 - 1 (1), 1 - 2 (1), 0 - 2 (5), 1 - 3 (3), 2 - 3 (1); router 2 is overloaded (SPTs WITH the overload bit: 2 is a leaf of
    every tree but its own).  S reaches 2 through 1 (2 < 5), so slot 1 (the dear 0 - 2 link) is no primary of D = 2 but a candidate:
    d(2, 2) = 0 < d(2, 0) + d(0, 2) = 2 + 2, another first link, and N == D lifts the overload rule; it avoids node 1
    (0 < d(2, 1) + d(1, 2) = 2) and is downstream (0 < 2); metric 5 + 0.  For D = 1 (1 < 2 + 1) and D = 3 (d(2, 3) = 1 < 2 + d(0, 3) = 4)
    neighbour 2 is loop-free too, but overloaded and not the destination: offered only when the call ignores the overload bit."""
    g = M.csr(4, M.both([(0, 1, 1), (1, 2, 1), (0, 2, 5), (1, 3, 3), (2, 3, 1)]), no_transit=[2])
    c, r = _model(g, 0)
    assert c.nbr.tolist() == [1, 2] and c.cflags.tolist() == [0, M.C_NO_TRANSIT]
    HP, LP, NP, DS = M.HAS_PRIMARY, M.LINK_PROTECT, M.NODE_PROTECT, M.DOWNSTREAM
    assert r.cand_mask[:, 0].tolist() == [0, 0, 2, 0]                       # bit 1 exactly at D == N
    assert r.alt_flags.tolist() == [0, HP, HP | LP | NP | DS, HP]
    assert r.alt_slot.tolist() == [M.NONE, M.NONE, 1, M.NONE] and r.alt_metric.tolist() == [0, 0, 5, 0]
    assert r.coverage.tolist() == [3, 0, 1, 1, 1]
    _c, r = _model(g, 0, lfa_flags=M.IGNORE_OVERLOAD)
    assert r.cand_mask[:, 0].tolist() == [0, 2, 2, 2]
    # D = 1: the primary's router is the destination (no node to protect), d(2, 1) = 1 is not below d(0, 1) = 1;
    # D = 3: 1 < d(2, 1) + d(1, 3) = 1 + 3 and 1 < d(0, 3) = 4; metric 5 + 1
    assert r.alt_flags.tolist() == [0, HP | LP, HP | LP | NP | DS, HP | LP | NP | DS] and r.alt_metric.tolist() == [0, 6, 5, 6]
