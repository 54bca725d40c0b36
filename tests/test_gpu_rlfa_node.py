"""hspf_rlfa_node_select_device and hspf_rlfa_node_device on the GPU against the plain-Python model (tests/_rlfa_node_model.py)
over the CPU oracle's SPTs: every output array of both calls, bit for bit, into buffers pre-filled with a non-zero byte.  The
tables the kernels read are the engine's own — hspf_run_device on the forward and the transposed upload, the space_flags
hspf_rlfa_device wrote (compared with the RLFA model first), one more hspf_run_device for the PQ-node rows — the expected values
never touch the engine.  Each case is the smallest shape at which one thing can go wrong; the class a case exists for is
asserted on the MODEL before anything is compared.  Every seed below was chosen on the CPU."""
import ctypes

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _rlfa_node_model as N
from test_gpu_frr_mixed_k import EDGE, HUB, LEAF, hub_on_grid
from test_gpu_rlfa import Case, Tables, lan, ring8, ring_chords
from test_gpu_tilfa import BIG, five_ring, grid, slot_of

pytestmark = pytest.mark.gpu

TILE_EDGE = {255: (2, 215), 256: (2, 216), 257: (16, 217)}      # n: (seed, protected root) of a ring with four chords: vertex n - 1 is listed and chosen
RING300 = (59, 3, 200)                                    # (seed, chords, protected root) of a unit-cost 300-ring: two slots with 4 qualifying vertices each
GRID_SEED, GRID_ROOT = 5, 20                              # the asymmetric 6 x 6 grid
DENSE = (0, 100)                                        # (seed, protected root) of a unit-cost 600-ring with 600 chords
SEL, DST = N.SEL_FIELDS, N.DEST_FIELDS


class Want:
    """The model's side of one protected root of a Case: RLFA, the lists, the PQ-node roots, the per-destination result."""

    def __init__(self, case, lfa_flags=0, with_lfa=True, max_pq=16, y_pick=None):
        self.alt = case.lfa(lfa_flags).alt_flags if with_lfa else None
        self.r = case.want(lfa_flags, with_lfa)
        self.sel = N.select(case.fwd.dist, case.cand, 0, case.nbr_row, self.r.space_flags, lfa_flags, max_pq)
        self.y_roots = np.array((y_pick(self.sel) if y_pick else N.union(self.sel)) or [N.NONE], np.uint32)
        self.yrows = N.y_rows(case.graph, case.maxp, [v for v in self.y_roots if v != N.NONE], case.run_flags)
        self.d = N.dest(case.fwd.dist, case.fwd.flags, case.fwd.mask, case.cand, 0, case.nbr_row, self.sel, self.yrows, self.alt)


def run_node(ctx, tab, protect, y_roots, run_flags=0, lfa_flags=0, alt_flags=None, max_pq=16, want_set=True, fill=7):
    """hspf_rlfa_device with space_flags, the select call on them, hspf_run_device of y_roots, the per-destination call; nothing
    leaves the device in between.  Returns ({space_flags}, {nq_*}, {nd_*}) as host arrays ([P, ...]; nd_set None when skipped)."""
    import torch
    dev = torch.device("cuda:0")
    P, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dev)      # noqa: E731
    r = dict(pq_node=full((P, S), torch.int32), pq_via=full((P, S), torch.int32), pq_metric=full((P, S), torch.int32), pq_counts=full((P, S, 4), torch.int32),
             space_flags=full((P, S, n), torch.uint8), rl_node=full((P, n), torch.int32), rl_via=full((P, n), torch.int32), rl_coverage=full((P, 4), torch.int32))
    s = dict(nq_node=full((P, S, max_pq), torch.int32), nq_via=full((P, S, max_pq), torch.int32), nq_metric=full((P, S, max_pq), torch.int32),
             nq_count=full((P, S), torch.int32))
    d = dict(nd_kind=full((P, n), torch.uint8), nd_node=full((P, n), torch.int32), nd_via=full((P, n), torch.int32), nd_metric=full((P, n), torch.int32),
             nd_set=full((P, n), torch.int32) if want_set else None, nd_coverage=full((P, 5), torch.int32))
    alt = torch.from_numpy(np.ascontiguousarray(alt_flags)).to(dev) if alt_flags is not None else None
    ap = 0 if alt is None else alt.data_ptr()
    fwd = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr())
    ydist = full((len(y_roots), n), torch.int32)
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the calls on the context's
    ctx.rlfa_device(tab.G, tab.R, tab.W, *fwd, tab.rdist.data_ptr(), protect, alt_flags_in_ptr=ap, lfa_flags=lfa_flags,
                    **{k + "_ptr": x.data_ptr() for k, x in r.items()})
    ctx.rlfa_node_select_device(n, tab.R, tab.W, *fwd, protect, space_flags_ptr=r["space_flags"].data_ptr(), max_pq=max_pq, lfa_flags=lfa_flags,
                                **{k + "_ptr": x.data_ptr() for k, x in s.items()})
    ctx.run_device(tab.G, y_roots, run_flags, dist_ptr=ydist.data_ptr())
    ctx.rlfa_node_device(n, tab.R, tab.W, *fwd, protect, ydist_ptr=ydist.data_ptr(), y_roots=y_roots, sel=tuple(s[k].data_ptr() for k in SEL),
                         max_pq=max_pq, alt_flags_in_ptr=ap, **{k + "_ptr": 0 if x is None else x.data_ptr() for k, x in d.items()})
    host = lambda t: {k: None if x is None else x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in t.items()}      # noqa: E731
    return host(r), host(s), host(d)


def assert_equal(got, want_r, want_sel, want_d, i=0, want_set=True, tag=""):
    got_r, got_s, got_d = got
    assert np.array_equal(got_r["space_flags"][i], want_r.space_flags), (tag, "space_flags")      # the input the select call read is the model's
    for name, g, w in [(k, got_s[k], getattr(want_sel, k)) for k in SEL] + [(k, got_d[k], getattr(want_d, k)) for k in DST]:
        if name == "nd_set" and not want_set:
            assert g is None
            continue
        g = g[i]
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:8].tolist(), g[g != w][:8], w[g != w][:8])


def check_one(ctx, case, lfa_flags=(0,), need=None, with_lfa=True, max_pq=16, y_pick=None, want_set=True):
    """One protected root on the device against the model, for every lfa_flags; returns the model of the first."""
    from holo_amd import engine as E
    pc = E.lfa_candidates(*case.graph, case.root)
    assert np.array_equal(pc.nbr, case.cand.nbr) and np.array_equal(pc.cost, case.cand.cost)
    wants = [Want(case, lf, with_lfa, max_pq, y_pick) for lf in lfa_flags]
    if need is not None:
        need(wants[0])
    tab = Tables(ctx, case.graph, case.maxp, case.roots, case.run_flags, case.W)
    try:
        for lf, w in zip(lfa_flags, wants):
            got = run_node(ctx, tab, [(0, pc, case.nbr_row)], w.y_roots, case.run_flags, lf, None if w.alt is None else w.alt[None, :], max_pq, want_set)
            assert_equal(got, w.r, w.sel, w.d, want_set=want_set, tag=lf)
    finally:
        tab.free()
    return wants[0]


def cands(case):
    return np.flatnonzero(case.cand.nbr != M.NONE)


def test_eight_ring_and_five_ring(spf_ctx):
    c8 = Case(ring8(), 0)

    def need8(w):
        e, k7 = slot_of(c8, 1), slot_of(c8, 7)
        assert (w.sel.nq_node[e, 0], w.sel.nq_via[e, 0], w.sel.nq_metric[e, 0], w.sel.nq_count[e]) == (4, k7, 4, 1)
        assert w.d.nd_kind.tolist() == [0, N.D_LAST_HOP, N.D_PQ, N.D_PQ, 0, N.D_PQ, N.D_PQ, N.D_LAST_HOP] and w.d.nd_coverage.tolist() == [6, 0, 4, 2, 0]
    check_one(spf_ctx, c8, need=need8)
    check_one(spf_ctx, c8, with_lfa=False)
    c5 = Case(five_ring(), 2)

    def need5(w):                                            # no PQ node at all (tests/test_host_tilfa.py): every list is empty
        assert not w.sel.nq_count.any() and w.y_roots.tolist() == [N.NONE] and w.d.nd_coverage.tolist() == [4, 0, 0, 2, 2]
    check_one(spf_ctx, c5, need=need5)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_rings_with_chords_at_the_tile_edge(spf_ctx, n):
    """A listed node is vertex n - 1: the last valid lane of the one partial tile (255), the last lane of a full tile (256), the
    only valid lane of the second tile (257)."""
    seed, root = TILE_EDGE[n]
    case = Case(ring_chords(n, seed, 1, 9, chords=4), root)

    def need(w):
        ks = cands(case)
        assert (w.sel.nq_node[ks] == n - 1).any() and (w.d.nd_node == n - 1).any() and w.d.nd_coverage[2] > 0
    check_one(spf_ctx, case, need=need)


@pytest.mark.parametrize("max_pq", [1, 4, 32])
def test_unit_cost_ring_of_300_ties_and_list_lengths(spf_ctx, max_pq):
    """Unit costs: many qualifying vertices share a release metric and the vertex index decides; they lie in both tiles.  Over the
    three max_pq the counts of the slots fall below, at and above the limit."""
    seed, chords, root = RING300
    case = Case(ring_chords(300, seed, 1, 1, chords=chords), root)
    rel = set()
    for m in (1, 4, 32):
        cnt = Want(case, max_pq=m).sel.nq_count[cands(case)]
        rel |= {int(np.sign(int(c) - m)) for c in cnt if c}
    assert rel == {-1, 0, 1}

    def need(w):
        ks = cands(case)
        q = [N.qualifying(case.fwd.dist, case.cand, 0, case.nbr_row, w.r.space_flags, e) for e in ks]
        assert any(len(x) > 1 and x[0][0] == x[1][0] for x in q)                      # a tie in the release metric at the head of a list
        assert any(any(v < 256 for _, v, _ in x) and any(v >= 256 for _, v, _ in x) for x in q)
        assert w.d.nd_coverage[2] > 0
    check_one(spf_ctx, case, need=need, max_pq=max_pq)


@pytest.mark.parametrize("max_pq", [4, 16])
def test_dense_unit_cost_mesh_truncates_long_lists(spf_ctx, max_pq):
    """A unit-cost ring of 600 with 600 chords: slots with far more qualifying vertices than max_pq, many of them in one wave and
    in each of the three tiles — every stage (wave, workgroup, the merge of the tiles' lists) cuts a list short, on ties."""
    seed, root = DENSE
    case = Case(ring_chords(600, seed, 1, 1, chords=600), root)

    def need(w):
        ks = cands(case)
        assert (w.sel.nq_count[ks] > 4 * max_pq).any()
        q = [N.qualifying(case.fwd.dist, case.cand, 0, case.nbr_row, w.r.space_flags, e) for e in ks]
        big = [x for x in q if len(x) > 4 * max_pq]
        assert any(max(np.bincount([v // 64 for _, v, _ in x])) > max_pq for x in big)             # one wave holds more than max_pq of them
        assert any(len({v // 256 for _, v, _ in x}) == 3 for x in big)                                # all three tiles hold some
        assert any(len({v // 256 for _, v, _ in x[:max_pq]}) > 1 for x in big)                        # the winners come from several tiles
        assert any(x[max_pq - 1][0] == x[max_pq][0] for x in big)                                     # the cut falls inside a tie
        assert w.d.nd_coverage[2] > 0
    check_one(spf_ctx, case, need=need, max_pq=max_pq)


def test_asymmetric_grid_6x6(spf_ctx):
    case = Case(grid(6, 6, GRID_SEED, asym=True), GRID_ROOT)

    def need(w):
        assert not np.array_equal(case.rdist, case.fwd.dist)                          # a real transposed rdist behind the Q bits
        assert w.d.nd_coverage[2] > 0 and (w.sel.nq_count[cands(case)] > 1).any()
    check_one(spf_ctx, case, need=need)


def test_parallel_links_root_to_neighbour(spf_ctx):
    """Two links 0-1 at 3 and 5: with the first protected, the link repair releases 1 and 2 over the parallel link (slot 1).  For
    the NODE 1 that slot is no way round: 1 is not listed, and 2 is listed as released by neighbour 5."""
    case = Case(M.csr(6, M.both([(0, 1, 3), (0, 1, 5)] + [(v, (v + 1) % 6, 2) for v in range(1, 6)])), 0)

    def need(w):
        e0, e1 = (int(k) for k in np.flatnonzero(case.cand.nbr == 1))
        k5 = slot_of(case, 5)
        assert w.r.space_via[e0][1] == e1 and w.r.space_via[e0][2] == e1               # the link repair: over the parallel link
        for e, other in ((e0, e1), (e1, e0)):
            L = int(w.sel.nq_count[e])
            assert L > 0 and not np.isin(w.sel.nq_via[e, :L], [other]).any() and not (w.sel.nq_node[e, :L] == 1).any()
        j = w.sel.nq_node[e0].tolist().index(2)
        assert w.sel.nq_via[e0, j] == k5
        assert w.d.nd_coverage[2] > 0
    check_one(spf_ctx, case, need=need, with_lfa=False)
    check_one(spf_ctx, case)


def test_overloaded_via_neighbour_with_and_without_ignore(spf_ctx):
    case = Case(ring8(no_transit=[7]), 0)
    e, k7 = slot_of(case, 1), slot_of(case, 7)
    plain, ign = Want(case, 0), Want(case, M.IGNORE_OVERLOAD)
    assert plain.sel.nq_count[e] == 0 and ign.sel.nq_count[e] == 3 and (ign.sel.nq_via[e, :3] == k7).all()      # every release is the overloaded neighbour's
    assert plain.d.nd_coverage[2] < ign.d.nd_coverage[2]
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD))


def test_lan_primary_slot_is_no_candidate(spf_ctx):
    """The LAN of tests/test_gpu_rlfa.py with HSPF_RUN_NET_NEXTHOPS: the pseudonode's one primary is S's slot onto the LAN, whose
    target is a network vertex — no candidate, no list; the routers behind the LAN are reached over candidate slots."""
    case = Case(lan(), 1, run_flags=1)

    def need(w):
        assert case.cand.nbr[0] == M.NONE and int(case.fwd.mask[0, 0, 0]) == 1 and w.d.nd_kind[0] == N.D_NONE and w.sel.nq_count[0] == 0
        assert w.d.nd_coverage[2] > 0
    check_one(spf_ctx, case, need=need, with_lfa=False)
    check_one(spf_ctx, case)


def test_costs_near_2_to_the_31_sums_and_saturation(spf_ctx):
    """A six-ring with 0x7FFFFFF0 on every link but the protected one: d(N, E) + d(E, v) and nq_metric + d(Y, D) pass 32 bits."""
    case = Case(M.csr(6, M.both([(0, 1, 1), (1, 2, 16), (2, 3, BIG), (3, 4, 16), (4, 5, 16), (5, 0, BIG)])), 0)

    def need(w):
        ks = cands(case)
        assert (w.sel.nq_metric[ks] >= 0x7FFFFFF0).any() and (w.d.nd_metric == 0xFFFFFFFE).any() and w.d.nd_coverage[2] > 0
        D = int(np.flatnonzero(w.d.nd_metric == 0xFFFFFFFE)[0])
        e = [k for k in ks if (int(case.fwd.mask[0, D, 0]) >> k) & 1][0]
        j = w.sel.nq_node[e].tolist().index(int(w.d.nd_node[D]))
        assert int(w.sel.nq_metric[e, j]) + int(w.yrows[int(w.d.nd_node[D])][D]) > 0xFFFFFFFF
    check_one(spf_ctx, case, need=need)


def test_y_roots_padding_duplicate_and_a_listed_node_left_out(spf_ctx):
    seed, chords, root = RING300
    case = Case(ring_chords(300, seed, 1, 1, chords=chords), root)
    full = Want(case, max_pq=4)
    chosen = sorted({int(v) for v in full.d.nd_node if v != N.NONE})
    drop = chosen[0]

    def y_pick(sel):
        u = [v for v in N.union(sel) if v != drop]
        return [N.NONE, u[1]] + u + [N.NONE, u[0]]           # padding in front and inside, two duplicates

    def need(w):
        was = full.d.nd_node == drop
        assert was.any() and not (w.d.nd_node == drop).any()
        assert (w.d.nd_kind[was] == N.D_PQ).any()            # the choice moved on to another entry of the list
        assert len(w.y_roots) == len(N.union(w.sel)) + 3 and (w.y_roots == N.NONE).sum() == 2
    check_one(spf_ctx, case, need=need, max_pq=4, y_pick=y_pick)


def test_nd_set_null(spf_ctx):
    check_one(spf_ctx, Case(ring8(), 0), want_set=False)


def test_roots_of_65_3_and_1_slots_in_one_call(spf_ctx):
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph = hub_on_grid()
    prot_roots = [HUB, EDGE, LEAF]
    cs = [M.candidates(*graph, r) for r in prot_roots]
    rows = prot_roots + sorted({int(x) for c in cs for x in c.nbr if x != M.NONE} - set(prot_roots))
    roots, row_of = np.array(rows, np.uint32), {v: i for i, v in enumerate(rows)}
    W = max(go.mask_words(*graph, roots), 2)
    fwd, rdist = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
    protect, wants, alts, sels = [], [], [], []
    for r, mc in zip(prot_roots, cs):
        nbr_row = np.array([row_of.get(int(x), 0) for x in mc.nbr], np.uint32)
        protect.append((row_of[r], E.lfa_candidates(*graph, r), nbr_row))
        alts.append(M.lfa(fwd.dist, fwd.flags, fwd.mask, mc, row_of[r], nbr_row).alt_flags)
        wr = R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], mc, row_of[r], nbr_row, 0, alts[-1])
        sels.append((wr, N.select(fwd.dist, mc, row_of[r], nbr_row, wr.space_flags, 0, 8), nbr_row))
    y_roots = np.array(sorted({v for _, s, _ in sels for v in N.union(s)}), np.uint32)
    yrows = N.y_rows(graph, 0xFFFFFFFF, y_roots)
    for r, mc, (wr, s, nbr_row), alt in zip(prot_roots, cs, sels, alts):
        wants.append((wr, s, N.dest(fwd.dist, fwd.flags, fwd.mask, mc, row_of[r], nbr_row, s, yrows, alt)))
    assert [len(c.nbr) for c in cs] == [65, 3, 1] and W == 2
    assert wants[0][1].nq_count[64] > 0 and wants[0][2].nd_coverage[2] > 0 and wants[1][2].nd_coverage[2] > 0      # a slot of the second word; two roots with repairs
    assert not wants[2][1].nq_count.any() and wants[2][2].nd_coverage[2] == 0                                       # a leaf has none
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        got = run_node(spf_ctx, tab, protect, y_roots, alt_flags=np.stack(alts), max_pq=8)
        for i, (wr, s, d) in enumerate(wants):
            assert_equal(got, wr, s, d, i, tag=i)
    finally:
        tab.free()


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import torch
    case = Case(ring_chords(30, 1, chords=4), 8)
    n, S, MQ = 30, 64, 4
    w = Want(case, max_pq=MQ)
    tab = Tables(spf_ctx, case.graph, case.maxp, case.roots, 0, 1)
    try:
        pc = E.lfa_candidates(*case.graph, 8)
        protect = [(0, pc, case.nbr_row)]
        good = run_node(spf_ctx, tab, protect, w.y_roots, alt_flags=w.alt[None, :], max_pq=MQ)
        assert_equal(good, w.r, w.sel, w.d)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda:0")      # noqa: E731
        sp_f = dev(good[0]["space_flags"], np.uint8)
        sel_in = {k: dev(good[1][k], np.int32) for k in SEL}
        ydist = torch.zeros((len(w.y_roots), n), dtype=torch.int32, device="cuda:0")
        sizes = dict(nq_node=S * MQ * 4, nq_via=S * MQ * 4, nq_metric=S * MQ * 4, nq_count=S * 4, nd_kind=32, nd_node=n * 4, nd_via=n * 4, nd_metric=n * 4,
                     nd_set=n * 4, nd_coverage=20)
        out = torch.full((sum(sizes.values()),), 0x5A, dtype=torch.uint8, device="cuda:0")
        ptrs, off = {}, 0
        for k, b in sizes.items():
            ptrs[k + "_ptr"] = out.data_ptr() + off
            off += b
        fwd = dict(dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr())
        untouched = lambda: bool((out.cpu().numpy() == 0x5A).all())      # noqa: E731

        def inval_select(protect_=None, max_pq=MQ, space_flags_ptr=None, **kw):
            t, p = dict(fwd), {k: v for k, v in ptrs.items() if k.startswith("nq_")}
            for k, v in kw.items():
                (t if k in t else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.rlfa_node_select_device(n, tab.R, 1, t["dist"], t["flags"], t["mask"], protect_ or protect,
                                                space_flags_ptr=sp_f.data_ptr() if space_flags_ptr is None else space_flags_ptr, max_pq=max_pq, **p)
            assert e.value.code == -1 and "hspf_rlfa_node_select_device" in str(e.value) and untouched()

        def inval_dest(protect_=None, max_pq=MQ, y_roots=None, ydist_ptr=None, sel=None, **kw):
            t, p = dict(fwd), {k: v for k, v in ptrs.items() if k.startswith("nd_")}
            for k, v in kw.items():
                (t if k in t else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.rlfa_node_device(n, tab.R, 1, t["dist"], t["flags"], t["mask"], protect_ or protect,
                                         ydist_ptr=ydist.data_ptr() if ydist_ptr is None else ydist_ptr, y_roots=w.y_roots if y_roots is None else y_roots,
                                         sel=sel or tuple(sel_in[k].data_ptr() for k in SEL), max_pq=max_pq, **p)
            assert e.value.code == -1 and "hspf_rlfa_node_device" in str(e.value) and untouched()

        bad_row = case.nbr_row.copy()
        bad_row[np.flatnonzero(case.cand.nbr != M.NONE)[0]] = tab.R
        many = E.LfaCandidates(8, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        bad_prot = ([(0, pc, bad_row)], [(tab.R, pc, case.nbr_row)], [(0, many, np.zeros(65, np.uint32))])      # nbr_row, root_row, n_slots out of range
        for f in (inval_select, inval_dest):
            for k in fwd:                                    # NULL required pointers: the tables
                f(**{k: 0})
            for pr in bad_prot:                              # what hspf_lfa_device rejects in `prot`
                f(protect_=pr)
            f(max_pq=0)
            f(max_pq=33)
        inval_select(space_flags_ptr=0)
        for k in SEL:                                        # every output of the select call
            inval_select(**{k + "_ptr": 0})
        for k in ("nd_kind", "nd_node", "nd_via", "nd_metric", "nd_coverage"):      # every required output of the second call
            inval_dest(**{k + "_ptr": 0})
        inval_dest(ydist_ptr=0)
        for i in range(4):                                   # a NULL list of the select result
            inval_dest(sel=tuple(0 if j == i else sel_in[k].data_ptr() for j, k in enumerate(SEL)))
        inval_dest(y_roots=np.zeros(0, np.uint32))           # n_yrows == 0
        inval_dest(y_roots=np.array([3, n, N.NONE], np.uint32))      # an entry >= n_vertices that is not HSPF_NO_ROOT
        # the raw calls with NULL prot / out, and zero protected roots
        lib = L.load()
        arr, keep = spf_ctx._protect_array(protect, "test")
        so = L.HspfRlfaNodeSel(*(ptrs[k + "_ptr"] for k in SEL))
        do = L.HspfRlfaNodeOut(*(ptrs[k + "_ptr"] for k in DST))
        si = L.HspfRlfaNodeSel(*(sel_in[k].data_ptr() for k in SEL))
        yr = np.ascontiguousarray(w.y_roots)
        yp = yr.ctypes.data_as(L.u32p)
        t3 = tuple(fwd.values())
        for prot_, np_, o in ((None, 1, ctypes.byref(so)), (arr, 1, None), (arr, 0, ctypes.byref(so))):
            assert lib.hspf_rlfa_node_select_device(spf_ctx.handle, n, tab.R, 1, *t3, prot_, np_, 0, sp_f.data_ptr(), MQ, o) == -1
            assert "hspf_rlfa_node_select_device" in spf_ctx.last_error() and untouched()
        for prot_, np_, yp_, s_, o in ((None, 1, yp, ctypes.byref(si), ctypes.byref(do)), (arr, 1, None, ctypes.byref(si), ctypes.byref(do)),
                                       (arr, 1, yp, None, ctypes.byref(do)), (arr, 1, yp, ctypes.byref(si), None), (arr, 0, yp, ctypes.byref(si), ctypes.byref(do))):
            assert lib.hspf_rlfa_node_device(spf_ctx.handle, n, tab.R, 1, *t3, prot_, np_, ydist.data_ptr(), yp_, len(yr), s_, MQ, None, o) == -1
            assert "hspf_rlfa_node_device" in spf_ctx.last_error() and untouched()
        del keep
        # and the context still works
        again = run_node(spf_ctx, tab, protect, w.y_roots, alt_flags=w.alt[None, :], max_pq=MQ)
        assert_equal(again, w.r, w.sel, w.d)
    finally:
        tab.free()


def test_rlfa_node_convenience_end_to_end(spf_ctx):
    """SpfContext.rlfa_node(): candidates, both runs, lfa_device, rlfa_device with the space tables, the select call, the run over
    the union of the lists, the per-destination call, results on the host; symmetric=True gives the same on this graph."""
    seed, root = TILE_EDGE[256]
    case = Case(ring_chords(256, seed, 1, 9, chords=4), root)
    w = Want(case, max_pq=16)
    assert w.d.nd_coverage[2] > 0
    G = spf_ctx.upload(*case.graph, 0xFFFFFFFF)
    try:
        res = spf_ctx.rlfa_node(G, root)
        res2 = spf_ctx.rlfa_node(G, root, symmetric=True)
    finally:
        G.free()
    assert np.array_equal(res.candidates.nbr, case.cand.nbr) and np.array_equal(res.lfa.alt_flags[0], case.lfa().alt_flags)
    assert np.array_equal(res.y_roots, w.y_roots)
    for name in SEL + DST:
        want = getattr(w.sel if name in SEL else w.d, name)
        assert np.array_equal(getattr(res, name)[0], want), name
        assert np.array_equal(getattr(res2, name), getattr(res, name)), name
