"""Remote loop-free alternates on the CPU side: the new symbols in header, ctypes table and library; hspf_csr_transpose (pure host
arithmetic, no context) against the model's independent transpose; the property the feature rests on — dist of a run on the
transposed graph is the distance TO the root — on the oracle; and the model itself (tests/_rlfa_model.py) pinned on hand-checked
RFC 7490 cases, so that what the GPU tests compare against is checked independently of the engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXP = 0xFFFFFFFF


def test_header_ctypes_and_library_agree_on_the_new_symbols():
    from holo_amd import build, _lib
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, n_args in (("hspf_csr_transpose", 4), ("hspf_rlfa_device", 14)):
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert table[name][0] is ctypes.c_int and len(table[name][1]) == n_args
    assert lib.hspf_abi_version() == 8                                   # additions only
    from holo_amd import engine as E
    for c_name, py in (("HSPF_RLFA_VIA_SELF", E.RLFA_VIA_SELF), ("HSPF_RLFA_IN_P", E.RLFA_IN_P), ("HSPF_RLFA_IN_XP", E.RLFA_IN_XP),
                       ("HSPF_RLFA_IN_Q", E.RLFA_IN_Q), ("HSPF_RLFA_ELIGIBLE", E.RLFA_ELIGIBLE), ("HSPF_RLFA_COUNT_WORDS", E.RLFA_COUNT_WORDS),
                       ("HSPF_RLFA_COVERAGE_WORDS", E.RLFA_COVERAGE_WORDS)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py, c_name
    assert (R.VIA_SELF, R.IN_P, R.IN_XP, R.IN_Q, R.ELIGIBLE) == (E.RLFA_VIA_SELF, E.RLFA_IN_P, E.RLFA_IN_XP, E.RLFA_IN_Q, E.RLFA_ELIGIBLE)
    assert len(_lib.HspfRlfaOut._fields_) == 9 and ctypes.sizeof(_lib.HspfRlfaOut) == 9 * ctypes.sizeof(ctypes.c_void_p)


# ---- hspf_csr_transpose ------------------------------------------------------------------------------------------------------

def _raw_transpose(rp, col, met, vf):
    """The C symbol itself (the Python wrapper is compared too)."""
    from holo_amd import _lib as L
    lib = L.load()
    rp, col, met, vf = (np.ascontiguousarray(a, dt) for a, dt in ((rp, np.uint32), (col, np.uint32), (met, np.uint32), (vf, np.uint8)))
    csr = L.HspfCsr(len(vf), len(col), rp.ctypes.data_as(L.u32p), col.ctypes.data_as(L.u32p), met.ctypes.data_as(L.u32p), vf.ctypes.data_as(L.u8p), MAXP)
    o = np.full(len(rp), 0x5A5A5A5A, np.uint32), np.full(len(col), 0x5A5A5A5A, np.uint32), np.full(len(col), 0x5A5A5A5A, np.uint32)
    rc = lib.hspf_csr_transpose(ctypes.byref(csr), *(a.ctypes.data_as(L.u32p) for a in o))
    return rc, o


def _transpose_graphs():
    from holo_amd import synth
    par = M.csr(4, [(0, 1, 5), (2, 1, 9), (0, 1, 3), (1, 0, 7), (0, 1, 4), (3, 1, 1), (0, 3, 2), (2, 1, 8)])      # parallel links: row order matters
    empty = M.csr(6, [(0, 2, 1), (2, 0, 1), (4, 2, 3), (2, 5, 6)])                                                  # rows 1, 3, 5 empty; 1 and 3 isolated
    net = M.csr(5, [(1, 0, 10), (0, 1, 0), (2, 0, 10), (0, 2, 0), (1, 3, 4), (3, 1, 6), (4, 0, 2)], net=[0])        # a pseudonode, a one-way link into it
    g = synth.random_lsdb(40, 6, 3.0, 3)
    return [par, empty, net, (g.row_ptr, g.col, g.metric, g.vflags)]


def _row_multiset(rp, col, met, v):
    return sorted(zip(col[rp[v]:rp[v + 1]].tolist(), met[rp[v]:rp[v + 1]].tolist()))


@pytest.mark.parametrize("gi", range(4))
def test_transpose_symbol_and_wrapper_equal_the_models(gi):
    from holo_amd import engine as E
    rp, col, met, vf = _transpose_graphs()[gi]
    want = R.transpose(rp, col, met)
    rc, got = _raw_transpose(rp, col, met, vf)
    assert rc == 0
    for g, w, py in zip(got, want, E.csr_transpose(rp, col, met, vf)):
        assert np.array_equal(g, w) and np.array_equal(py, w)
    if gi == 0:                                                          # the parallel links 0 -> 1 keep the order of 0's row: 5, 3, 4
        trp, tcol, tmet = want
        assert tcol[trp[1]:trp[2]].tolist() == [0, 0, 0, 2, 2, 3] and tmet[trp[1]:trp[2]].tolist() == [5, 3, 4, 9, 8, 1]
    if gi == 1:
        assert np.diff(want[0].astype(np.int64)).tolist() == [1, 0, 2, 0, 0, 1]
    # twice: every row holds the same multiset of (target, cost) as at the start
    back = E.csr_transpose(*want, vf)
    assert np.array_equal(back[0], np.asarray(rp, np.uint32))
    for v in range(len(vf)):
        assert _row_multiset(*back, v) == _row_multiset(rp, col, met, v)


def test_transpose_rejects_what_the_upload_rejects():
    rp, col, met, vf = _transpose_graphs()[0]
    bad_rp = rp.copy(); bad_rp[-1] += 1
    assert _raw_transpose(bad_rp, col, met, vf)[0] == -1                 # row_ptr[n] != n_edges
    dec = rp.copy(); dec[1], dec[2] = dec[2], dec[1]
    if dec[1] > dec[2]:
        assert _raw_transpose(dec, col, met, vf)[0] == -1                # not monotone
    far = col.copy(); far[0] = 99
    rc, out = _raw_transpose(rp, far, met, vf)
    assert rc == -1 and all((a == 0x5A5A5A5A).all() for a in out)        # a target out of range: nothing written
    from holo_amd import _lib as L
    assert L.load().hspf_csr_transpose(None, None, None, None) == -1


# ---- the reverse-distance property, on the oracle ---------------------------------------------------------------------------

def _asym_lsdb(seed):
    from holo_amd import synth
    g = synth.random_lsdb(60, 8, 3.0, seed)
    r = np.random.default_rng(1000 + seed)
    met = r.integers(1, 400, len(g.col)).astype(np.uint32)               # every direction drawn on its own
    vf = g.vflags.copy()
    vf[8 + r.choice(60, 4, replace=False)] |= M.VF_NO_TRANSIT
    return g.row_ptr, g.col, met, vf


@pytest.mark.parametrize("seed", range(1, 7))
@pytest.mark.parametrize("run_flags", [0, 2])                            # HSPF_RUN_IGNORE_OVERLOAD
def test_oracle_on_the_transposed_graph_gives_distances_to_the_root(seed, run_flags):
    from oracle import graph_oracle as go
    rp, col, met, vf = _asym_lsdb(seed)
    n = len(vf)
    roots = np.arange(n, dtype=np.uint32)
    fwd = go.run(rp, col, met, vf, 1023, roots, run_flags, go.MAP).dist                 # fwd[u][v] = d(u, v)
    rev = go.run(*R.transpose(rp, col, met), vf, 1023, roots, run_flags, go.MAP).dist   # rev[x][v] must be d(v, x)
    ok = (vf & R.VF_NO_EXPAND) == 0
    pair = ok[:, None] & ok[None, :]
    assert np.array_equal(rev[pair], fwd.T[pair])
    off = pair & ~np.eye(n, dtype=bool)
    unreach = (fwd[off] == R.INF).mean()
    assert 0.01 < unreach < 0.5                                          # max_path_metric 1023 prunes, and not everything
    both = off & (fwd != R.INF) & (fwd.T != R.INF)
    assert (fwd[both] != fwd.T[both]).mean() >= 0.5                      # the forward distances are no substitute


# ---- the model, pinned on hand-checked cases ---------------------------------------------------------------------------------

def _ring(n, cost=lambda a, b: 1, no_transit=()):
    links = []
    for v in range(n):
        w = (v + 1) % n
        links += [(v, w, cost(v, w)), (w, v, cost(w, v))]
    return M.csr(n, links, no_transit=no_transit)


def _members(r, e, bit):
    return np.flatnonzero(r.space_flags[e] & bit).tolist()


def _slot_of(c, v):
    return int(np.flatnonzero(c.nbr == v)[0])


def test_model_ring_of_eight_unit_costs():
    c, roots, nbr_row, W, lfa, r = R.one_root(_ring(8), 0)
    e, k7 = _slot_of(c, 1), _slot_of(c, 7)
    assert _members(r, e, R.IN_P) == [5, 6, 7]
    assert _members(r, e, R.IN_P | R.IN_XP) == [4, 5, 6, 7]
    assert _members(r, e, R.IN_Q) == [1, 2, 3, 4]
    assert _members(r, e, R.ELIGIBLE) == [1, 2, 3, 4, 5, 6, 7]
    assert r.pq_counts[e].tolist() == [3, 4, 4, 1]
    assert (r.pq_node[e], r.pq_via[e], r.pq_metric[e]) == (4, k7, 4)
    assert r.space_via[e, 4] == k7 and r.space_via[e, 5] == R.VIA_SELF and r.space_via[e, 2] == R.NONE
    assert not (lfa.alt_flags[[1, 2, 3]] & M.LINK_PROTECT).any()         # LFA alone covers none of them
    assert r.rl_node[[1, 2, 3]].tolist() == [4, 4, 4] and r.rl_via[[1, 2, 3]].tolist() == [k7] * 3
    assert r.rl_node[4] == R.NONE and lfa.alt_flags[4] & M.ECMP          # two primaries: no remote alternate is chosen
    assert r.rl_node[[5, 6, 7]].tolist() == [4, 4, 4]                    # the mirror image: the PQ node of slot k7 is 4 as well
    assert r.rl_coverage.tolist() == [6, 0, 6, 0]
    assert (r.pq_node[2:] == R.NONE).all() and (r.pq_via[2:] == R.NONE).all() and not r.pq_metric[2:].any()      # slots that do not exist


def test_model_triangle_lfa_covers_everything():
    c, roots, nbr_row, W, lfa, r = R.one_root(M.csr(3, M.both([(0, 1, 1), (1, 2, 1), (2, 0, 1)])), 0)
    assert r.rl_coverage.tolist() == [2, 2, 0, 0] and (r.rl_node == R.NONE).all()
    # without the LFA flags the same destinations are handed to the PQ nodes
    r2 = R.one_root(M.csr(3, M.both([(0, 1, 1), (1, 2, 1), (2, 0, 1)])), 0, with_lfa=False)[5]
    assert r2.rl_coverage[1] == 0 and r2.rl_coverage[0] == 2


def test_model_two_parallel_links_pq_is_the_far_end():
    c, roots, nbr_row, W, lfa, r = R.one_root(M.csr(2, M.both([(0, 1, 1), (0, 1, 5)])), 0)
    assert c.nbr.tolist() == [1, 1] and c.cost.tolist() == [1, 5]
    assert (r.pq_node[0], r.pq_via[0], r.pq_metric[0]) == (1, 1, 5)      # E itself, released over the other link
    assert r.space_flags[0, 1] == R.IN_XP | R.IN_Q | R.ELIGIBLE


def test_model_overloaded_pq_candidate_and_via_neighbour():
    # the would-be PQ node 4 is overloaded: skipped, unless the call ignores overload
    g = _ring(8, no_transit=[4])
    c, _, _, _, _, r = R.one_root(g, 0)
    e, k7 = _slot_of(c, 1), _slot_of(c, 7)
    assert r.pq_node[e] == R.NONE and not (r.space_flags[e, 4] & R.ELIGIBLE) and r.pq_counts[e, 3] == 0
    r = R.one_root(g, 0, lfa_flags=M.IGNORE_OVERLOAD)[5]
    assert (r.pq_node[e], r.pq_via[e], r.pq_metric[e]) == (4, k7, 4)
    # the via-neighbour 7 is overloaded: not admissible, the extended P-space is empty; admissible when overload is ignored
    g = _ring(8, no_transit=[7])
    c, _, _, _, _, r = R.one_root(g, 0)
    assert c.cflags[k7] & M.C_NO_TRANSIT
    assert r.pq_counts[e].tolist()[:2] == [0, 0] and r.pq_node[e] == R.NONE
    r = R.one_root(g, 0, lfa_flags=M.IGNORE_OVERLOAD)[5]
    assert _members(r, e, R.IN_XP) == [4, 5, 6, 7] and _members(r, e, R.IN_Q) == [1, 2, 3, 4, 5, 6] and (r.pq_node[e], r.pq_via[e], r.pq_metric[e]) == (6, k7, 2)


def asym_ring():
    """Ring of 8 with each direction of each link at its own cost (found by search on the model; asserted below): going round
    clockwise and counter-clockwise cost different sums, so the distances TO the far end are not the distances FROM it."""
    cw = [3, 3, 4, 5, 1, 1, 5, 5]          # v -> v + 1
    ccw = [2, 2, 5, 3, 2, 5, 2, 3]         # v + 1 -> v
    return _ring(8, cost=lambda a, b: cw[a] if b == (a + 1) % 8 else ccw[b])


def test_model_asymmetric_ring_needs_the_reverse_run():
    g = asym_ring()
    c, roots, nbr_row, W, lfa, true = R.one_root(g, 0)
    wrong = R.one_root(g, 0, rdist_is_forward=True)[5]
    e = _slot_of(c, 1)
    assert _members(true, e, R.IN_Q) == [1, 2, 3, 4, 5] and _members(wrong, e, R.IN_Q) == [1, 2, 3, 4, 5, 6, 7]
    assert (true.pq_node[e], true.pq_metric[e]) == (5, 10)               # 0 -> 7 -> 6 -> 5 costs 3 + 2 + 5
    assert wrong.pq_node[e] == 7                                         # d(1, 7) = 5 < d(0, 7) + 3, but d(7, 1) = 8 is not < d(7, 0) + 3 = 8
    assert np.array_equal(true.space_flags[e] & 3, wrong.space_flags[e] & 3)      # P and XP do not read rdist
