"""hspf_tilfa_node_select_device and hspf_tilfa_node_device on the GPU against the plain-Python model (tests/_tilfa_node_model.py)
over the CPU oracle's SPTs: every output array of both calls, bit for bit, into buffers pre-filled with a non-zero byte.  The
tables the kernels read are the engine's own — hspf_run_device on the forward and the transposed upload, the space_flags
hspf_rlfa_device wrote (compared with the RLFA model first), one more hspf_run_device for the q rows; alt_flags and nd_kind are the
models' — the expected values never touch the engine.  Each case is the smallest shape at which one thing can go wrong; the class
a case exists for is asserted on the MODEL before anything is compared.  Every seed below was chosen on the CPU."""
import ctypes
import functools

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _rlfa_node_model as N
import _tilfa_model as T
import _tilfa_node_model as TN
from test_gpu_frr_mixed_k import EDGE, HUB, LEAF, hub_on_grid
from test_gpu_rlfa import Case, Tables, lan, ring8, ring_chords
from test_gpu_tilfa import BIG, grid, slot_of

pytestmark = pytest.mark.gpu

SEL, DST = TN.SEL_FIELDS, TN.DEST_FIELDS
TILE_EDGE = {255: (1, 121), 256: (1, 122), 257: (1, 122)}      # n: (seed, protected root) of a heavy ring with two chords: vertex n - 1 is listed and chosen
MESH = (0, 100)                                           # (seed, protected root) of a unit-cost 600-ring with 600 chords
PICK = (0, 10)                                            # (seed, protected root) of a heavy 60-ring with six chords: several listed q's are chosen
GRID_SEED, GRID_ROOT = 5, 20                              # the asymmetric 6 x 6 grid of tests/test_gpu_rlfa_node.py
WRAP_N = 64 * 256 + 40                                    # k_tn_sel_final deals the tiles' lists to 64 lanes: the 65th tile is the first wrap


def six_ring(no_transit=()):
    """The smallest example: 0-1-2-3-4-5-0, link 3-4 at 10, every other at 1."""
    return M.csr(6, M.both([(v, (v + 1) % 6, 10 if v == 3 else 1) for v in range(6)]), no_transit=no_transit)


def heavy_ring(n, seed, chords, heavy_at=None, heavy=None, lo=1, hi=3, no_transit=()):
    """A ring of n routers with seeded costs lo .. hi, ONE heavy link (`heavy_at`, `heavy_at` + 1; default n - 2, cost default 2 n)
    and `chords` seeded chords that cost as much as the ring between their ends (they shorten nothing: the spaces stay apart)."""
    r = np.random.default_rng(seed)
    h = n - 2 if heavy_at is None else heavy_at
    und = [(v, (v + 1) % n, (2 * n if heavy is None else heavy) if v == h else int(r.integers(lo, hi + 1))) for v in range(n)]
    have = {(v, (v + 1) % n) for v in range(n)}
    while len(und) < n + chords:
        a, b = sorted(int(x) for x in r.integers(0, n, 2))
        if b - a < 2 or (a, b) in have or (a == 0 and b == n - 1) or a <= h < b:
            continue
        have.add((a, b))
        und.append((a, b, sum(c for u, _, c in und[:n] if a <= u < b)))
    return M.csr(n, M.both(und), no_transit=no_transit)


def q_is_e():
    """S = 0, E = 1.  Router 2 is in P, the Q-space is {1, 3}: hspf_tilfa_device's best pair is (2, 1) at 11 — q == E — before (2, 3) at
    12.  Router 4 hangs off E alone: every q reaches it through E."""
    return M.csr(5, M.both([(0, 1, 1), (0, 2, 1), (2, 1, 10), (1, 3, 1), (2, 3, 10), (1, 4, 1)]))


def parallel_pq():
    """The six-ring with three links 4 -> 3 in row 4 at 12, 10, 10 (and three back): the entry of q = 3 is the first link at 10."""
    links = []
    for v in range(6):
        if v == 3:
            links += [(3, 4, 12), (4, 3, 12), (3, 4, 10), (4, 3, 10), (3, 4, 10), (4, 3, 10)]
        else:
            links += M.both([(v, (v + 1) % 6, 1)])
    return M.csr(6, links)


class Want:
    """The model's side of one protected root of a Case: RLFA, the RLFA-node result (nd_kind), the lists, the q roots, the
    per-destination result."""

    def __init__(self, case, lfa_flags=0, with_lfa=True, with_nd=True, max_pairs=16, y_pick=None):
        f = case.fwd
        self.alt = case.lfa(lfa_flags).alt_flags if with_lfa else None
        self.r = case.want(lfa_flags, with_lfa)
        self.nd_kind = None
        if with_nd:
            ns = N.select(f.dist, case.cand, 0, case.nbr_row, self.r.space_flags, lfa_flags, 16)
            yn = N.y_rows(case.graph, case.maxp, N.union(ns), case.run_flags)
            self.nd_kind = N.dest(f.dist, f.flags, f.mask, case.cand, 0, case.nbr_row, ns, yn, self.alt).nd_kind
        self.sel = TN.select(f.dist, case.graph, case.cand, 0, case.nbr_row, self.r.space_flags, lfa_flags, max_pairs)
        self.y_roots = np.array((y_pick(self.sel) if y_pick else TN.union(self.sel)) or [TN.NONE], np.uint32)
        self.yrows = TN.y_rows(case.graph, case.maxp, [v for v in self.y_roots if v != TN.NONE], case.run_flags)
        self.d = TN.dest(f.dist, f.flags, f.mask, case.cand, 0, case.nbr_row, self.sel, self.yrows, self.alt, self.nd_kind)


def run_tn(ctx, tab, protect, y_roots, run_flags=0, lfa_flags=0, alt_flags=None, nd_kind=None, max_pairs=16, want_set=True, fill=7):
    """hspf_rlfa_device with space_flags, the select call on them, hspf_run_device of y_roots, the per-destination call; nothing
    leaves the device in between.  Returns ({space_flags}, {tq_*}, {tn_*}) as host arrays ([P, ...]; tn_set None when skipped)."""
    import torch
    dev = torch.device("cuda:0")
    P, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dev)      # noqa: E731
    r = dict(pq_node=full((P, S), torch.int32), pq_via=full((P, S), torch.int32), pq_metric=full((P, S), torch.int32), pq_counts=full((P, S, 4), torch.int32),
             space_flags=full((P, S, n), torch.uint8), rl_node=full((P, n), torch.int32), rl_via=full((P, n), torch.int32), rl_coverage=full((P, 4), torch.int32))
    s = {k: full((P, S, max_pairs), torch.int32) for k in SEL[:-1]}
    s["tq_count"] = full((P, S), torch.int32)
    d = dict(tn_kind=full((P, n), torch.uint8), **{k: full((P, n), torch.int32) for k in DST[1:-2]}, tn_set=full((P, n), torch.int32) if want_set else None,
             tn_coverage=full((P, 6), torch.int32))
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    alt, ndk = up(alt_flags), up(nd_kind)
    ptr = lambda x: 0 if x is None else x.data_ptr()      # noqa: E731
    fwd = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr())
    ydist = full((len(y_roots), n), torch.int32)
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the calls on the context's
    ctx.rlfa_device(tab.G, tab.R, tab.W, *fwd, tab.rdist.data_ptr(), protect, alt_flags_in_ptr=ptr(alt), lfa_flags=lfa_flags,
                    **{k + "_ptr": x.data_ptr() for k, x in r.items()})
    ctx.tilfa_node_select_device(tab.G, tab.R, tab.W, *fwd, protect, space_flags_ptr=r["space_flags"].data_ptr(), max_pairs=max_pairs, lfa_flags=lfa_flags,
                                 **{k + "_ptr": x.data_ptr() for k, x in s.items()})
    ctx.run_device(tab.G, y_roots, run_flags, dist_ptr=ydist.data_ptr())
    ctx.tilfa_node_device(n, tab.R, tab.W, *fwd, protect, ydist_ptr=ydist.data_ptr(), y_roots=y_roots, sel=tuple(s[k].data_ptr() for k in SEL),
                          max_pairs=max_pairs, alt_flags_in_ptr=ptr(alt), nd_kind_in_ptr=ptr(ndk), **{k + "_ptr": ptr(x) for k, x in d.items()})
    host = lambda t: {k: None if x is None else x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in t.items()}      # noqa: E731
    return host(r), host(s), host(d)


def assert_equal(got, want_r, want_sel, want_d, i=0, want_set=True, tag=""):
    got_r, got_s, got_d = got
    assert np.array_equal(got_r["space_flags"][i], want_r.space_flags), (tag, "space_flags")      # the input the select call read is the model's
    for name, g, w in [(k, got_s[k], getattr(want_sel, k)) for k in SEL] + [(k, got_d[k], getattr(want_d, k)) for k in DST]:
        if name == "tn_set" and not want_set:
            assert g is None
            continue
        g = g[i]
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:8].tolist(), g[g != w][:8], w[g != w][:8])


def check_one(ctx, case, lfa_flags=(0,), need=None, with_lfa=True, with_nd=True, max_pairs=16, y_pick=None, want_set=True):
    """One protected root on the device against the model, for every lfa_flags; returns the model of the first."""
    from holo_amd import engine as E
    pc = E.lfa_candidates(*case.graph, case.root)
    assert np.array_equal(pc.nbr, case.cand.nbr) and np.array_equal(pc.cost, case.cand.cost)
    wants = [Want(case, lf, with_lfa, with_nd, max_pairs, y_pick) for lf in lfa_flags]
    if need is not None:
        need(wants[0])
    tab = Tables(ctx, case.graph, case.maxp, case.roots, case.run_flags, case.W)
    try:
        for lf, w in zip(lfa_flags, wants):
            one = lambda a: None if a is None else a[None, :]      # noqa: E731
            got = run_tn(ctx, tab, [(0, pc, case.nbr_row)], w.y_roots, case.run_flags, lf, one(w.alt), one(w.nd_kind), max_pairs, want_set)
            assert_equal(got, w.r, w.sel, w.d, want_set=want_set, tag=lf)
    finally:
        tab.free()
    return wants[0]


def cands(case):
    return np.flatnonzero(case.cand.nbr != M.NONE)


def six_ring_need(case):
    def need(w):
        e = slot_of(case, 1)
        assert w.nd_kind.tolist() == [0, N.D_LAST_HOP, N.D_NONE, N.D_NONE, N.D_NONE, N.D_LAST_HOP]      # no PQ node: RFC 8102 has nothing
        assert (w.sel.tq_q[e, 0], w.sel.tq_p[e, 0], w.sel.tq_link[e, 0], w.sel.tq_via[e, 0], w.sel.tq_metric[e, 0], w.sel.tq_count[e]) == (3, 4, 0, TN.VIA_SELF, 12, 1)
        assert w.d.tn_kind.tolist() == [0, TN.D_LAST_HOP, TN.D_PAIR, TN.D_PAIR, TN.D_PAIR, TN.D_LAST_HOP]
        assert w.d.tn_metric.tolist() == [0, 0, 13, 12, 13, 0] and w.d.tn_p[2:4].tolist() == [4, 4] and w.d.tn_q[2:4].tolist() == [3, 3]
        assert w.d.tn_coverage.tolist() == [5, 0, 0, 2, 0, 3]
    return need


def test_six_ring(spf_ctx):
    case = Case(six_ring(), 0)
    check_one(spf_ctx, case, need=six_ring_need(case))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_heavy_rings_with_chords_at_the_tile_edge(spf_ctx, n):
    """The heavy link joins n - 2 and n - 1: vertex n - 1 is a listed q of one slot and a listed p of the other — the last valid lane
    of the one partial tile (255), the last lane of a full tile (256), the only valid lane of the second tile (257)."""
    seed, root = TILE_EDGE[n]
    case = Case(heavy_ring(n, seed, 2), root)

    def need(w):
        ks = cands(case)
        assert (w.sel.tq_q[ks] == n - 1).any() and (w.sel.tq_p[ks] == n - 1).any()
        assert (w.d.tn_q == n - 1).any() and (w.d.tn_p == n - 1).any() and w.d.tn_coverage[5] > 0
    check_one(spf_ctx, case, need=need)


@pytest.mark.parametrize("max_pairs", [1, 4, 32])
def test_unit_cost_mesh_truncation_and_ties(spf_ctx, max_pairs):
    """A unit-cost ring of 600 with 600 chords: slots with more than 32 q's, in all three tiles, many at one entry metric — every
    stage (wave, workgroup, the merge of the tiles' lists) cuts a list short, inside a tie.  nd_kind_in is NULL: the pairs are
    judged although PQ nodes exist."""
    seed, root = MESH
    case = Case(ring_chords(600, seed, 1, 1, chords=600), root)

    def need(w):
        ks = cands(case)
        assert (w.sel.tq_count[ks] > 32).any()
        ent = [TN.entries(case.fwd.dist, case.graph, case.cand, 0, case.nbr_row, w.r.space_flags, e) for e in ks]
        big = [x for x in ent if len(x) > 32]
        assert any(max(np.bincount([q // 64 for _, q, *_ in x])) > max_pairs for x in big)           # one wave holds more than max_pairs of them
        assert any(len({q // 256 for _, q, *_ in x}) == 3 for x in big)                              # all three tiles hold some
        assert any(x[max_pairs - 1][0] == x[max_pairs][0] for x in big)                              # the cut falls inside a tie
        assert w.d.tn_coverage[5] > 0
    check_one(spf_ctx, case, need=need, with_nd=False, max_pairs=max_pairs)


def test_asymmetric_grid_6x6(spf_ctx):
    case = Case(grid(6, 6, GRID_SEED, asym=True), GRID_ROOT)

    def need(w):
        assert not np.array_equal(case.rdist, case.fwd.dist)                          # a real transposed rdist behind the Q bits
        assert w.d.tn_coverage[1] > 0 and w.d.tn_coverage[2] > 0 and (w.sel.tq_count[cands(case)] > 1).any()
    check_one(spf_ctx, case, need=need)
    check_one(spf_ctx, case, with_nd=False, with_lfa=False)


def test_parallel_p_q_links_the_first_at_the_entry_metric(spf_ctx):
    case = Case(parallel_pq(), 0)

    def need(w):
        e = slot_of(case, 1)
        rp, col, met, _ = case.graph
        row4 = [(int(col[k]), int(met[k])) for k in range(rp[4], rp[5])]
        assert row4[:3] == [(3, 12), (3, 10), (3, 10)]
        assert (w.sel.tq_q[e, 0], w.sel.tq_p[e, 0], w.sel.tq_link[e, 0], w.sel.tq_metric[e, 0], w.sel.tq_count[e]) == (3, 4, 1, 12, 1)
        assert w.d.tn_link[2] == 1 and w.d.tn_kind[2] == TN.D_PAIR
    check_one(spf_ctx, case, need=need)


def test_q_equal_to_the_neighbour_is_not_listed_and_a_stub_behind_it_has_none(spf_ctx):
    """hspf_tilfa_device's own best pair enters E itself; the list holds the next one.  Router 4 hangs off E: pairs exist for the
    link, none protects it — HSPF_TN_D_NONE with an empty set."""
    case = Case(q_is_e(), 0)

    def need(w):
        e = slot_of(case, 1)
        t = T.tilfa(case.fwd.dist, case.fwd.flags, case.fwd.mask, case.rdist, case.graph, case.cand, 0, case.nbr_row, w.r.space_flags, w.r.space_via, w.alt)
        assert (t.ti_kind[e], t.ti_p[e], t.ti_q[e], t.ti_metric[e]) == (T.KIND_PAIR, 2, 1, 11)
        assert w.sel.tq_count[e] == 1 and (w.sel.tq_q[e, 0], w.sel.tq_p[e, 0], w.sel.tq_metric[e, 0]) == (3, 2, 11) and not (w.sel.tq_q == 1).any()
        assert (w.d.tn_kind[3], w.d.tn_metric[3], w.d.tn_set[3]) == (TN.D_PAIR, 11, 1)
        assert (w.d.tn_kind[4], w.d.tn_set[4], w.d.tn_q[4]) == (TN.D_NONE, 0, TN.NONE)
    check_one(spf_ctx, case, need=need)
    check_one(spf_ctx, case, with_lfa=False, with_nd=False)


def test_overloaded_via_neighbour_with_and_without_ignore(spf_ctx):
    """The six-ring with router 5 overloaded: S's own paths do not cross 5, so router 4 is in no P-space; asked to ignore the
    overload, neighbour 5 releases it and the pair (4, 3) is listed (nd_kind_in is NULL: with it, router 4 is a PQ node and stands)."""
    case = Case(six_ring(no_transit=[5]), 0)
    e, k5 = slot_of(case, 1), slot_of(case, 5)
    plain, ign = Want(case, 0, with_nd=False), Want(case, M.IGNORE_OVERLOAD, with_nd=False)
    assert plain.sel.tq_count[e] == 0 and ign.sel.tq_count[e] == 2
    assert (ign.sel.tq_q[e, 1], ign.sel.tq_p[e, 1], ign.sel.tq_via[e, 1], ign.sel.tq_metric[e, 1]) == (3, 4, k5, 12)
    assert plain.d.tn_coverage[5] == 0 and ign.d.tn_coverage[5] > 0
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD), with_nd=False)
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD))


def test_lan_primary_slot_is_no_candidate(spf_ctx):
    case = Case(lan(), 1, run_flags=1)

    def need(w):
        assert case.cand.nbr[0] == M.NONE and int(case.fwd.mask[0, 0, 0]) == 1 and w.d.tn_kind[0] == TN.D_NONE and w.sel.tq_count[0] == 0
        assert (w.sel.tq_q[0] == TN.NONE).all()
    check_one(spf_ctx, case, need=need, with_lfa=False)
    check_one(spf_ctx, case)


def big_ring():
    """A six-ring with 0x7FFFFFF0 and 0x80000001 on two links: relN(4) + w and tq_metric + d(q, D) pass 32 bits, and the heavier of the
    two keeps router 3 out of the extended P-space."""
    return M.csr(6, M.both([(0, 1, 1), (1, 2, 16), (2, 3, 16), (3, 4, BIG + 17), (4, 5, 16), (5, 0, BIG)]))


def test_costs_near_2_to_the_31_sums_and_saturation(spf_ctx):
    case = Case(big_ring(), 0)

    def need(w):
        e = slot_of(case, 1)
        assert (w.sel.tq_q[e, 0], w.sel.tq_p[e, 0], w.sel.tq_metric[e, 0]) == (3, 4, 0xFFFFFFFE)
        assert int(case.fwd.dist[0, 4]) + BIG + 17 > 0xFFFFFFFF                       # the entry metric is a saturated 64-bit sum
        assert (w.d.tn_kind[2], w.d.tn_metric[2]) == (TN.D_PAIR, 0xFFFFFFFE) and int(w.sel.tq_metric[e, 0]) + int(w.yrows[3][2]) > 0xFFFFFFFF
    check_one(spf_ctx, case, need=need)


def pick_case():
    seed, root = PICK
    return Case(heavy_ring(60, seed, 6, heavy_at=(root + 30) % 60, heavy=40), root)


def test_y_roots_padding_duplicate_and_a_listed_q_left_out(spf_ctx):
    case = pick_case()
    full = Want(case, max_pairs=4)
    chosen = sorted({int(v) for v in full.d.tn_q if v != TN.NONE})
    drop = chosen[0]

    def y_pick(sel):
        u = [v for v in TN.union(sel) if v != drop]
        return [TN.NONE, u[1]] + u + [TN.NONE, u[0]]         # padding in front and inside, two duplicates

    def need(w):
        was = full.d.tn_q == drop
        assert was.any() and not (w.d.tn_q == drop).any()
        assert (w.d.tn_kind[was] == TN.D_PAIR).any()         # the choice moved on to another entry of the list
        assert len(w.y_roots) == len(TN.union(w.sel)) + 3 and (w.y_roots == TN.NONE).sum() == 2
    check_one(spf_ctx, case, need=need, max_pairs=4, y_pick=y_pick)


def test_tn_set_null(spf_ctx):
    check_one(spf_ctx, Case(six_ring(), 0), want_set=False)


def test_nd_kind_in_null_and_given(spf_ctx):
    """The eight-ring has PQ nodes: given nd_kind, its destinations stay HSPF_TN_D_PQ; without it the pairs are judged."""
    case = Case(ring8(), 0)

    def need_given(w):
        assert (w.d.tn_kind == TN.D_PQ).sum() == 4 and w.d.tn_coverage[2] == 4 and w.d.tn_coverage[5] == 0 and (w.sel.tq_count[cands(case)] > 0).all()

    def need_null(w):
        assert w.d.tn_coverage[2] == 0 and w.d.tn_coverage[5] > 0
    check_one(spf_ctx, case, need=need_given)
    check_one(spf_ctx, case, need=need_null, with_nd=False)


@functools.lru_cache(maxsize=None)
def mixed_wants(max_pairs=8):
    """The model's side of three protected roots of 65, 3 and 1 slots over ONE table set."""
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph = hub_on_grid()
    prot_roots = [HUB, EDGE, LEAF]
    cs = [M.candidates(*graph, r) for r in prot_roots]
    rows = prot_roots + sorted({int(x) for c in cs for x in c.nbr if x != M.NONE} - set(prot_roots))
    roots, row_of = np.array(rows, np.uint32), {v: i for i, v in enumerate(rows)}
    W = max(go.mask_words(*graph, roots), 2)
    fwd, rdist = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
    protect, alts, sels = [], [], []
    for r, mc in zip(prot_roots, cs):
        nbr_row = np.array([row_of.get(int(x), 0) for x in mc.nbr], np.uint32)
        protect.append((row_of[r], E.lfa_candidates(*graph, r), nbr_row))
        alts.append(M.lfa(fwd.dist, fwd.flags, fwd.mask, mc, row_of[r], nbr_row).alt_flags)
        wr = R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], mc, row_of[r], nbr_row, 0, alts[-1])
        sels.append((wr, TN.select(fwd.dist, graph, mc, row_of[r], nbr_row, wr.space_flags, 0, max_pairs), nbr_row))
    y_roots = np.array(sorted({v for _, s, _ in sels for v in TN.union(s)}), np.uint32)
    yrows = TN.y_rows(graph, 0xFFFFFFFF, y_roots)
    wants = [(wr, s, TN.dest(fwd.dist, fwd.flags, fwd.mask, mc, row_of[r], nbr_row, s, yrows, alt))
             for r, mc, (wr, s, nbr_row), alt in zip(prot_roots, cs, sels, alts)]
    return graph, roots, W, cs, protect, alts, y_roots, wants


def test_roots_of_65_3_and_1_slots_in_one_call(spf_ctx):
    graph, roots, W, cs, protect, alts, y_roots, wants = mixed_wants()
    assert [len(c.nbr) for c in cs] == [65, 3, 1] and W == 2
    assert wants[0][1].tq_count[64] > 0 and wants[0][2].tn_coverage[5] > 0 and wants[1][2].tn_coverage[5] > 0      # a slot of the second word; two roots with repairs
    assert not wants[2][1].tq_count.any() and wants[2][2].tn_coverage[5] == 0                                       # a leaf has none
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        got = run_tn(spf_ctx, tab, protect, y_roots, alt_flags=np.stack(alts), max_pairs=8)
        for i, (wr, s, d) in enumerate(wants):
            assert_equal(got, wr, s, d, i, tag=i)
    finally:
        tab.free()


def test_a_ring_past_the_first_wrap_of_the_tile_lists(spf_ctx):
    """65 tiles: lane 0 of k_tn_sel_final holds the lists of tiles 0 and 64.  The heavy link joins the last two vertices, so the
    listed q of one slot and the listed p of the other lie in tile 64."""
    n = WRAP_N
    case = Case(heavy_ring(n, 0, 2), n // 2 - 1)

    def need(w):
        ks = cands(case)
        assert (w.sel.tq_q[ks] >= 64 * 256).any() and (w.sel.tq_p[ks] >= 64 * 256).any() and (w.sel.tq_q[ks] < 64 * 256).any()
        assert (w.d.tn_q >= 64 * 256).any() and w.d.tn_coverage[5] > 0
    check_one(spf_ctx, case, need=need)


def test_every_class_occurs_on_the_models_side():
    """Every tn_kind class is compared somewhere above (this test needs no device; it lives here to stand next to the cases)."""
    seen = set()
    for case in (Case(six_ring(), 0), Case(ring8(), 0), Case(q_is_e(), 0), Case(grid(6, 6, GRID_SEED, asym=True), GRID_ROOT)):
        seen |= set(Want(case).d.tn_kind.tolist())
    assert seen >= {TN.D_LFA, TN.D_PQ, TN.D_LAST_HOP, TN.D_NONE, TN.D_PAIR}, seen


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import torch
    case = pick_case()
    n, S, MP = 60, 64, 4
    w = Want(case, max_pairs=MP)
    tab = Tables(spf_ctx, case.graph, case.maxp, case.roots, 0, 1)
    other = spf_ctx.upload(*six_ring(), 0xFFFFFFFF)
    try:
        pc = E.lfa_candidates(*case.graph, case.root)
        protect = [(0, pc, case.nbr_row)]
        good = run_tn(spf_ctx, tab, protect, w.y_roots, alt_flags=w.alt[None, :], nd_kind=w.nd_kind[None, :], max_pairs=MP)
        assert_equal(good, w.r, w.sel, w.d)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda:0")      # noqa: E731
        sp_f = dev(good[0]["space_flags"], np.uint8)
        sel_in = {k: dev(good[1][k], np.int32) for k in SEL}
        ydist = torch.zeros((len(w.y_roots), n), dtype=torch.int32, device="cuda:0")
        sizes = {k: S * MP * 4 for k in SEL[:-1]}
        sizes.update(tq_count=S * 4, tn_kind=64, **{k: n * 4 for k in DST[1:-1]}, tn_coverage=24)
        out = torch.full((sum(sizes.values()),), 0x5A, dtype=torch.uint8, device="cuda:0")
        ptrs, off = {}, 0
        for k, b in sizes.items():
            ptrs[k + "_ptr"] = out.data_ptr() + off
            off += b
        fwd = dict(dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr())
        untouched = lambda: bool((out.cpu().numpy() == 0x5A).all())      # noqa: E731

        def inval_select(protect_=None, max_pairs=MP, space_flags_ptr=None, graph=None, **kw):
            t, p = dict(fwd), {k: v for k, v in ptrs.items() if k.startswith("tq_")}
            for k, v in kw.items():
                (t if k in t else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.tilfa_node_select_device(graph or tab.G, tab.R, 1, t["dist"], t["flags"], t["mask"], protect_ or protect,
                                                 space_flags_ptr=sp_f.data_ptr() if space_flags_ptr is None else space_flags_ptr, max_pairs=max_pairs, **p)
            assert e.value.code == -1 and "hspf_tilfa_node_select_device" in str(e.value) and untouched()

        def inval_dest(protect_=None, max_pairs=MP, y_roots=None, ydist_ptr=None, sel=None, **kw):
            t, p = dict(fwd), {k: v for k, v in ptrs.items() if k.startswith("tn_")}
            for k, v in kw.items():
                (t if k in t else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.tilfa_node_device(n, tab.R, 1, t["dist"], t["flags"], t["mask"], protect_ or protect,
                                          ydist_ptr=ydist.data_ptr() if ydist_ptr is None else ydist_ptr, y_roots=w.y_roots if y_roots is None else y_roots,
                                          sel=sel or tuple(sel_in[k].data_ptr() for k in SEL), max_pairs=max_pairs, **p)
            assert e.value.code == -1 and "hspf_tilfa_node_device" in str(e.value) and untouched()

        bad_row = case.nbr_row.copy()
        bad_row[np.flatnonzero(case.cand.nbr != M.NONE)[0]] = tab.R
        many = E.LfaCandidates(case.root, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        bad_prot = ([(0, pc, bad_row)], [(tab.R, pc, case.nbr_row)], [(0, many, np.zeros(65, np.uint32))])      # nbr_row, root_row, n_slots out of range
        for f in (inval_select, inval_dest):
            for k in fwd:                                    # NULL required pointers: the tables
                f(**{k: 0})
            for pr in bad_prot:                              # what hspf_lfa_device rejects in `prot`
                f(protect_=pr)
            f(max_pairs=0)
            f(max_pairs=33)
        inval_select(space_flags_ptr=0)                      # a NULL space table
        for k in SEL:                                        # every output of the select call
            inval_select(**{k + "_ptr": 0})
        for k in ("tn_kind", "tn_p", "tn_q", "tn_link", "tn_via", "tn_metric", "tn_coverage"):      # every required output of the second call
            inval_dest(**{k + "_ptr": 0})
        inval_dest(ydist_ptr=0)
        for i in range(len(SEL)):                            # a NULL list of the select result
            inval_dest(sel=tuple(0 if j == i else sel_in[k].data_ptr() for j, k in enumerate(SEL)))
        inval_dest(y_roots=np.zeros(0, np.uint32))           # n_yrows == 0
        inval_dest(y_roots=np.array([3, n, TN.NONE], np.uint32))      # an entry >= n_vertices that is not HSPF_NO_ROOT
        # the raw calls with NULL graph / prot / out, a graph of another size, and zero protected roots
        lib = L.load()
        arr, keep = spf_ctx._protect_array(protect, "test")
        so = L.HspfTilfaNodeSel(*(ptrs[k + "_ptr"] for k in SEL))
        do = L.HspfTilfaNodeOut(*(ptrs[k + "_ptr"] for k in DST))
        si = L.HspfTilfaNodeSel(*(sel_in[k].data_ptr() for k in SEL))
        yr = np.ascontiguousarray(w.y_roots)
        yp = yr.ctypes.data_as(L.u32p)
        t3 = tuple(fwd.values())
        gh = tab.G.handle
        for g_, prot_, np_, o in ((gh, None, 1, ctypes.byref(so)), (gh, arr, 1, None), (gh, arr, 0, ctypes.byref(so)), (None, arr, 1, ctypes.byref(so)),
                                  (other.handle, arr, 1, ctypes.byref(so))):
            assert lib.hspf_tilfa_node_select_device(spf_ctx.handle, g_, n, tab.R, 1, *t3, prot_, np_, 0, sp_f.data_ptr(), MP, o) == -1
            assert "hspf_tilfa_node_select_device" in spf_ctx.last_error() and untouched()
        for prot_, np_, yp_, s_, o in ((None, 1, yp, ctypes.byref(si), ctypes.byref(do)), (arr, 1, None, ctypes.byref(si), ctypes.byref(do)),
                                       (arr, 1, yp, None, ctypes.byref(do)), (arr, 1, yp, ctypes.byref(si), None), (arr, 0, yp, ctypes.byref(si), ctypes.byref(do))):
            assert lib.hspf_tilfa_node_device(spf_ctx.handle, n, tab.R, 1, *t3, prot_, np_, ydist.data_ptr(), yp_, len(yr), s_, MP, None, None, o) == -1
            assert "hspf_tilfa_node_device" in spf_ctx.last_error() and untouched()
        del keep
        # and the context still works
        again = run_tn(spf_ctx, tab, protect, w.y_roots, alt_flags=w.alt[None, :], nd_kind=w.nd_kind[None, :], max_pairs=MP)
        assert_equal(again, w.r, w.sel, w.d)
    finally:
        other.free()
        tab.free()


def test_tilfa_node_convenience_end_to_end(spf_ctx):
    """SpfContext.tilfa_node(): the chain of rlfa_node(), the select call, the run over the union of the lists, the per-destination
    call with alt_flags and nd_kind, results on the host; symmetric=True gives the same on these graphs."""
    for case in (Case(six_ring(), 0), pick_case()):
        w = Want(case, max_pairs=16)
        assert w.d.tn_coverage[5] > 0
        G = spf_ctx.upload(*case.graph, 0xFFFFFFFF)
        try:
            res = spf_ctx.tilfa_node(G, case.root)
            res2 = spf_ctx.tilfa_node(G, case.root, symmetric=True)
        finally:
            G.free()
        assert np.array_equal(res.rlfa_node.candidates.nbr, case.cand.nbr) and np.array_equal(res.rlfa_node.lfa.alt_flags[0], w.alt)
        assert np.array_equal(res.rlfa_node.nd_kind[0], w.nd_kind) and np.array_equal(res.y_roots, w.y_roots)
        for name in SEL + DST:
            want = getattr(w.sel if name in SEL else w.d, name)
            assert np.array_equal(getattr(res, name)[0], want), name
            assert np.array_equal(getattr(res2, name), getattr(res, name)), name
