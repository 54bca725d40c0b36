"""hspf_tilfa_device on the GPU against the plain-Python model (tests/_tilfa_model.py) over the CPU oracle's SPTs: every output
array, bit for bit.  The tables the kernels read are the engine's own — hspf_run_device on the forward and the transposed upload,
the space tables hspf_rlfa_device wrote (compared with the RLFA model first) — the expected values never touch the engine.  Each
case is the smallest shape at which one thing can go wrong; where a case is for a class of result, that class is asserted on the
MODEL before anything is compared."""
import ctypes

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _tilfa_model as T
from test_gpu_rlfa import PRUNE_SEED, Case, Tables, lan, ring8, ring_chords, with_island

pytestmark = pytest.mark.gpu

RING300 = (3, 110)            # (seed, protected root): the equal-cost repairs of a slot lie on both sides of vertex 256, the winner is 255
E2E = (11, 100)               # (seed, protected root) of a 300-ring with six chords on which RLFA covers nothing and the pairs everything
TILE_EDGE = {255: (1, 109), 256: (10, 152), 257: (53, 152)}      # n: (seed, protected root) of a ring with four chords whose winner is vertex n - 1
BIG = 0x7FFFFFF0              # two such costs fit 32 bits, two and anything more than 14 do not


def want_of(case, lfa_flags=0, with_lfa=True, rdist=None):
    """(RLFA model, TI-LFA model) of the case's one protected root."""
    alt = case.lfa(lfa_flags).alt_flags if with_lfa else None
    r = case.want(lfa_flags, with_lfa, rdist)
    t = T.tilfa(case.fwd.dist, case.fwd.flags, case.fwd.mask, case.rdist if rdist is None else rdist, case.graph, case.cand, 0, case.nbr_row,
                r.space_flags, r.space_via, alt)
    return r, t


def run_tilfa(ctx, tab, protect, lfa_flags=0, alt_flags=None, fill=7):
    """hspf_rlfa_device with the space tables, then hspf_tilfa_device on them, nothing leaving the device in between.
    Returns ({field: host array} of the RLFA call's space tables and counts, {field: host array} of the TI-LFA call)."""
    import torch
    dev = torch.device("cuda:0")
    P, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dev)      # noqa: E731
    r = dict(pq_node=full((P, S), torch.int32), pq_via=full((P, S), torch.int32), pq_metric=full((P, S), torch.int32), pq_counts=full((P, S, 4), torch.int32),
             space_flags=full((P, S, n), torch.uint8), space_via=full((P, S, n), torch.int32), rl_node=full((P, n), torch.int32),
             rl_via=full((P, n), torch.int32), rl_coverage=full((P, 4), torch.int32))
    t = dict(ti_kind=full((P, S), torch.uint8), ti_p=full((P, S), torch.int32), ti_q=full((P, S), torch.int32), ti_via=full((P, S), torch.int32),
             ti_link=full((P, S), torch.int32), ti_metric=full((P, S), torch.int32), ti_counts=full((P, S, 2), torch.int32),
             td_kind=full((P, n), torch.uint8), td_coverage=full((P, 5), torch.int32))
    alt = torch.from_numpy(np.ascontiguousarray(alt_flags)).to(dev) if alt_flags is not None else None
    ap = 0 if alt is None else alt.data_ptr()
    tables = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr())
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.rlfa_device(tab.G, tab.R, tab.W, *tables, protect, alt_flags_in_ptr=ap, lfa_flags=lfa_flags, **{k + "_ptr": x.data_ptr() for k, x in r.items()})
    ctx.tilfa_device(tab.G, tab.R, tab.W, *tables, protect, space_flags_ptr=r["space_flags"].data_ptr(), space_via_ptr=r["space_via"].data_ptr(),
                     alt_flags_in_ptr=ap, lfa_flags=lfa_flags, **{k + "_ptr": x.data_ptr() for k, x in t.items()})
    host = lambda d: {k: x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in d.items()}      # noqa: E731
    return host(r), host(t)


def assert_equal(got_r, got_t, want_r, want_t, i=0, tag=""):
    for name in ("space_flags", "space_via", "pq_counts"):                     # the input the second call read is the model's
        assert np.array_equal(got_r[name][i], getattr(want_r, name)), (tag, name)
    for name in T.FIELDS:
        g, w = got_t[name][i], getattr(want_t, name)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:8].tolist(), g[g != w][:8], w[g != w][:8])
    assert np.array_equal(got_t["ti_counts"][i][:, 0], got_r["pq_counts"][i][:, 3])


def check_one(ctx, case, lfa_flags=(0,), need=None, with_lfa=True):
    """One protected root on the device against the model, for every lfa_flags; returns the models of the first."""
    from holo_amd import engine as E
    pc = E.lfa_candidates(*case.graph, case.root)
    assert np.array_equal(pc.nbr, case.cand.nbr) and np.array_equal(pc.cost, case.cand.cost)
    wants = [want_of(case, lf, with_lfa) for lf in lfa_flags]
    if need is not None:
        need(*wants[0])
    tab = Tables(ctx, case.graph, case.maxp, case.roots, case.run_flags, case.W)
    try:
        for lf, (wr, wt) in zip(lfa_flags, wants):
            alt = case.lfa(lf).alt_flags[None, :] if with_lfa else None
            assert_equal(*run_tilfa(ctx, tab, [(0, pc, case.nbr_row)], lf, alt), wr, wt, tag=lf)
    finally:
        tab.free()
    return wants[0]


def slot_of(case, v):
    return int(np.flatnonzero(case.cand.nbr == v)[0])


def five_ring(extra=()):
    """0-1-2-3-4-0 with costs 1, 1, 1, 1 and 4 on 4-0 (tests/test_host_tilfa.py): S = 2 needs the pair 0 -> 4 for the link 2-3."""
    return M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]) + list(extra))


def grid(rows, cols, seed, asym=False):
    r = np.random.default_rng(seed)
    links = []
    for y in range(rows):
        for x in range(cols):
            for a, b in (((y, x), (y, x + 1)), ((y, x), (y + 1, x))):
                if b[0] < rows and b[1] < cols:
                    c1 = int(r.integers(1, 10))
                    c2 = int(r.integers(1, 10)) if asym else c1
                    links += [(a[0] * cols + a[1], b[0] * cols + b[1], c1), (b[0] * cols + b[1], a[0] * cols + a[1], c2)]
    return M.csr(rows * cols, links)


def hub_on_ring(k, seed):
    """Vertex 0 linked to every router of a ring 1 .. k; seeded costs, the hub's links dearer than the ring's."""
    r = np.random.default_rng(seed)
    und = [(0, v, int(r.integers(5, 12))) for v in range(1, k + 1)] + [(v, v % k + 1, int(r.integers(1, 6))) for v in range(1, k + 1)]
    return M.csr(k + 1, M.both(und))


def test_five_and_six_ring(spf_ctx):
    c5 = Case(five_ring(), 2)

    def need5(wr, wt):
        e = slot_of(c5, 3)
        assert wr.pq_node[e] == R.NONE and (wt.ti_kind[e], wt.ti_p[e], wt.ti_q[e], wt.ti_metric[e]) == (T.KIND_PAIR, 0, 4, 7)
        assert wt.td_coverage.tolist() == [4, 0, 0, 4, 0]
    check_one(spf_ctx, c5, need=need5)
    c6 = Case(M.csr(6, M.both([(v, (v + 1) % 6, 1) for v in range(6)])), 0)

    def need6(wr, wt):
        e = slot_of(c6, 1)
        assert (wt.ti_kind[e], wt.ti_p[e], wt.ti_metric[e]) == (T.KIND_NODE, 3, 5) and wt.ti_counts[e].tolist() == [1, 2]
    check_one(spf_ctx, c6, need=need6)
    check_one(spf_ctx, c6, with_lfa=False)


def test_ring_of_300_winner_and_tie_in_different_tiles(spf_ctx):
    seed, root = RING300
    case = Case(ring_chords(300, seed, 1, 9, chords=0), root)

    def need(wr, wt):
        both_sides = 0
        for e in np.flatnonzero(case.cand.nbr != M.NONE):
            reps = T.repairs(case.fwd.dist, case.rdist, case.graph, case.cand, 0, case.nbr_row, e, wr.space_flags[e], wr.space_via[e])
            best = [x for x in reps if x[0] == min(reps)[0]]
            both_sides += any(x[2] < 256 for x in best) and any(x[2] >= 256 for x in best)
        assert both_sides and (wt.ti_kind != 0).sum() == 2 and (wt.ti_p[:2] == 255).all()
    check_one(spf_ctx, case, need=need)


@pytest.mark.parametrize("asym", [False, True])
def test_grid_4x4(spf_ctx, asym):
    case = Case(grid(4, 4, 11, asym), 5)

    def need(wr, wt):
        assert (wt.ti_kind[:4] != 0).all() and len(case.cand.nbr) == 4
        if asym:
            assert not np.array_equal(case.rdist, case.fwd.dist)               # a real transposed rdist
    check_one(spf_ctx, case, need=need)


def test_parallel_links_root_to_neighbour(spf_ctx):
    """Two links 0-1: with one of them protected E = 1 itself is in P and Q — the repair is the other link."""
    case = Case(M.csr(6, M.both([(0, 1, 3), (0, 1, 5)] + [(v, (v + 1) % 6, 2) for v in range(1, 6)])), 0)

    def need(wr, wt):
        e0, e1 = (int(k) for k in np.flatnonzero(case.cand.nbr == 1))
        assert (wt.ti_kind[e0], wt.ti_p[e0], wt.ti_metric[e0]) == (T.KIND_NODE, 1, 5)
        assert (wt.ti_kind[e1], wt.ti_p[e1], wt.ti_metric[e1]) == (T.KIND_NODE, 1, 3)
    check_one(spf_ctx, case, need=need)


@pytest.mark.parametrize("costs,link", [((6, 4), 2), ((4, 4), 1)])
def test_parallel_links_p_to_q(spf_ctx, costs, link):
    """The 4-0 link of the five-ring doubled: the cheaper one is forced; at equal cost (two pairs with equal totals, equal p and
    q) the earlier position."""
    g = M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, costs[0]), (4, 0, costs[1])]))
    case = Case(g, 2)

    def need(wr, wt):
        e = slot_of(case, 3)
        assert (wt.ti_kind[e], wt.ti_p[e], wt.ti_q[e], wt.ti_link[e], wt.ti_metric[e]) == (T.KIND_PAIR, 0, 4, link, 7)
        assert wt.ti_counts[e].tolist() == [0, 2]
    check_one(spf_ctx, case, need=need)


def test_one_way_link_is_not_forced(spf_ctx):
    """1 -> 4 at cost 1 with nothing back: it would repair 2-3 at 1 + 1 + 1; it fails the two-way check."""
    case = Case(five_ring(extra=[(1, 4, 1)]), 2)

    def need(wr, wt):
        e = slot_of(case, 3)
        assert wr.space_flags[e][1] & R.IN_P and wr.space_flags[e][4] & R.IN_Q
        assert (wt.ti_kind[e], wt.ti_p[e], wt.ti_q[e], wt.ti_metric[e]) == (T.KIND_PAIR, 0, 4, 7) and wt.ti_counts[e].tolist() == [0, 1]
    check_one(spf_ctx, case, need=need)


def test_overloaded_router_on_the_repair_path(spf_ctx):
    case = Case(ring8(no_transit=[4]), 0)
    e = slot_of(case, 1)
    assert want_of(case, 0)[1].ti_kind[e] == T.KIND_NONE and want_of(case, M.IGNORE_OVERLOAD)[1].ti_kind[e] != T.KIND_NONE
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD))


def test_lan_pseudonode_between_p_and_q_is_not_offered(spf_ctx):
    """S = 1 and E = 2 on a p2p link; 3 (in P) and 4 (in Q) share a LAN whose pseudonode is 0 (cost 10 onto it, so that
    4 is in no extended P-space); the only way round is 1-3-LAN-4-2."""
    links = M.both([(1, 2, 1), (1, 3, 1), (4, 2, 1)])
    for r_ in (3, 4):
        links += [(r_, 0, 10), (0, r_, 0)]
    case = Case(M.csr(5, links, net=[0]), 1)

    def need(wr, wt):
        e = slot_of(case, 2)
        assert wr.space_flags[e][3] & R.IN_P and wr.space_flags[e][4] & R.IN_Q and not wr.space_flags[e][0] & R.ELIGIBLE
        assert wt.ti_kind[e] == T.KIND_NONE and wt.ti_counts[e].tolist() == [0, 0]
    check_one(spf_ctx, case, need=need)
    check_one(spf_ctx, Case(lan(), 1))


def test_hub_root_with_70_neighbours_two_mask_words(spf_ctx):
    case = Case(hub_on_ring(70, 2), 0)

    def need(wr, wt):
        assert case.W == 2 and len(case.cand.nbr) == 70
        assert (wt.ti_kind[64:70] != 0).all() and not wt.ti_kind[70:].any() and (wt.ti_p[70:] == T.NONE).all()
    check_one(spf_ctx, case, need=need)


def test_degree_70_p_long_row(spf_ctx):
    case = Case(hub_on_ring(70, 3), 35)

    def need(wr, wt):
        ks = np.flatnonzero(case.cand.nbr != M.NONE)
        assert any(wr.space_flags[e][0] & (R.IN_P | R.IN_XP) for e in ks)        # the hub's 70-link row is walked
        assert wt.ti_counts[ks, 1].max() >= 30
    check_one(spf_ctx, case, need=need)


def test_two_protected_roots_share_one_table_set(spf_ctx):
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph = ring_chords(40, 9, 1, 9, chords=3)
    prot_roots = [0, 20]
    cands = [M.candidates(*graph, r) for r in prot_roots]
    rows = prot_roots + sorted({int(x) for c in cands for x in c.nbr if x != M.NONE} - set(prot_roots))
    roots, row_of = np.array(rows, np.uint32), {v: i for i, v in enumerate(rows)}
    W = go.mask_words(*graph, roots)
    fwd, rdist = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
    protect, wants, alts = [], [], []
    for r, mc in zip(prot_roots, cands):
        nbr_row = np.array([row_of.get(int(x), 0) for x in mc.nbr], np.uint32)
        protect.append((row_of[r], E.lfa_candidates(*graph, r), nbr_row))
        alts.append(M.lfa(fwd.dist, fwd.flags, fwd.mask, mc, row_of[r], nbr_row).alt_flags)
        wr = R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], mc, row_of[r], nbr_row, 0, alts[-1])
        wants.append((wr, T.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, mc, row_of[r], nbr_row, wr.space_flags, wr.space_via, alts[-1])))
    assert all((wt.ti_kind != 0).any() for _, wt in wants) and not np.array_equal(wants[0][1].ti_p, wants[1][1].ti_p)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        got_r, got_t = run_tilfa(spf_ctx, tab, protect, 0, np.stack(alts))
        for i, (wr, wt) in enumerate(wants):
            assert_equal(got_r, got_t, wr, wt, i, tag=i)
    finally:
        tab.free()


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import torch
    case = Case(ring_chords(30, 1, chords=4), 8)
    n, S = 30, 64
    tab = Tables(spf_ctx, case.graph, case.maxp, case.roots, 0, 1)
    try:
        pc = E.lfa_candidates(*case.graph, 8)
        protect = [(0, pc, case.nbr_row)]
        good_r, good_t = run_tilfa(spf_ctx, tab, protect)
        sp_f = torch.from_numpy(good_r["space_flags"]).to("cuda:0")
        sp_v = torch.from_numpy(good_r["space_via"].view(np.int32)).to("cuda:0")
        sizes = dict(ti_kind=S, ti_p=S * 4, ti_q=S * 4, ti_via=S * 4, ti_link=S * 4, ti_metric=S * 4, ti_counts=S * 8, td_kind=32, td_coverage=20)
        out = torch.full((sum(sizes.values()),), 0x5A, dtype=torch.uint8, device="cuda:0")
        ptrs, off = {}, 0
        for k, b in sizes.items():
            ptrs[k + "_ptr"] = out.data_ptr() + off
            off += b
        ptrs.update(space_flags_ptr=sp_f.data_ptr(), space_via_ptr=sp_v.data_ptr())

        def expect_inval(protect_=None, **kw):
            tables = dict(dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr(), rdist=tab.rdist.data_ptr())
            p = dict(ptrs)
            for k, v in kw.items():
                (tables if k in tables else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.tilfa_device(tab.G, tab.R, 1, tables["dist"], tables["flags"], tables["mask"], tables["rdist"], protect_ or protect, **p)
            assert e.value.code == -1 and "hspf_tilfa_device" in str(e.value)
            assert (out.cpu().numpy() == 0x5A).all()         # nothing was written: nothing was launched

        for k in ("dist", "flags", "mask", "rdist"):        # NULL required pointers: the tables,
            expect_inval(**{k: 0})
        expect_inval(space_flags_ptr=0)                      # the space tables (required here, optional for RLFA),
        expect_inval(space_via_ptr=0)
        for k in sizes:                                      # and every output
            expect_inval(**{k + "_ptr": 0})
        bad_row = case.nbr_row.copy()
        bad_row[np.flatnonzero(case.cand.nbr != M.NONE)[0]] = tab.R
        expect_inval(protect_=[(0, pc, bad_row)])            # nbr_row >= n_rows
        expect_inval(protect_=[(tab.R, pc, case.nbr_row)])   # root_row out of range
        many = E.LfaCandidates(8, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        expect_inval(protect_=[(0, many, np.zeros(65, np.uint32))])      # n_slots > 64 * n_mask_words
        lib = L.load()
        arr, keep = spf_ctx._protect_array(protect, "test")
        o = L.HspfTilfaOut(*(ptrs[k + "_ptr"] for k in sizes))
        tb = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr())
        other = spf_ctx.upload(*ring8(), 0xFFFFFFFF)         # a graph of another size than n_vertices
        try:
            assert lib.hspf_tilfa_device(spf_ctx.handle, other.handle, n, tab.R, 1, *tb, arr, 1, 0, None, sp_f.data_ptr(), sp_v.data_ptr(), ctypes.byref(o)) == -1
            assert "hspf_tilfa_device" in spf_ctx.last_error() and (out.cpu().numpy() == 0x5A).all()
        finally:
            other.free()
        # the raw call with NULL graph / prot / out, and zero protected roots
        assert lib.hspf_tilfa_device(spf_ctx.handle, None, n, tab.R, 1, *tb, arr, 1, 0, None, sp_f.data_ptr(), sp_v.data_ptr(), ctypes.byref(o)) == -1
        assert lib.hspf_tilfa_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, *tb, None, 1, 0, None, sp_f.data_ptr(), sp_v.data_ptr(), ctypes.byref(o)) == -1
        assert lib.hspf_tilfa_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, *tb, arr, 1, 0, None, sp_f.data_ptr(), sp_v.data_ptr(), None) == -1
        assert lib.hspf_tilfa_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, *tb, arr, 0, 0, None, sp_f.data_ptr(), sp_v.data_ptr(), ctypes.byref(o)) == -1
        assert "hspf_tilfa_device" in spf_ctx.last_error() and (out.cpu().numpy() == 0x5A).all()
        del keep
        # and the context still works
        again_r, again_t = run_tilfa(spf_ctx, tab, protect)
        assert all(np.array_equal(good_t[k], again_t[k]) for k in good_t)
        assert_equal(again_r, again_t, *want_of(case, with_lfa=False))
    finally:
        tab.free()


def test_tilfa_convenience_end_to_end(spf_ctx):
    """SpfContext.tilfa(): candidates, both runs, lfa_device, rlfa_device with the space tables, tilfa_device, results on the
    host; td_coverage says how much of RLFA's remainder the pairs close."""
    seed, root = E2E
    case = Case(ring_chords(300, seed, 1, 9, chords=6), root)
    wr, wt = want_of(case)
    assert wr.rl_coverage[3] > 0 and wt.td_coverage[3] > 0 and wt.td_coverage[4] == 0        # on the MODEL: RLFA leaves some, the pairs close them
    G = spf_ctx.upload(*case.graph, 0xFFFFFFFF)
    try:
        cand, lfa, rl, ti = spf_ctx.tilfa(G, root)
        cand2, lfa2, rl2, ti2 = spf_ctx.tilfa(G, root, symmetric=True)
    finally:
        G.free()
    assert np.array_equal(cand.nbr, case.cand.nbr) and np.array_equal(lfa.alt_flags[0], case.lfa().alt_flags)
    for name in R.FIELDS:
        assert np.array_equal(getattr(rl, name)[0], getattr(wr, name)), name
    for name in T.FIELDS:
        assert np.array_equal(getattr(ti, name)[0], getattr(wt, name)), name
        assert np.array_equal(getattr(ti2, name), getattr(ti, name)), name
    assert ti.td_coverage[0].tolist() == wt.td_coverage.tolist() and ti.td_coverage[0, 0] == rl.rl_coverage[0, 0]
    assert ti.td_coverage[0, 1] == rl.rl_coverage[0, 1] and ti.td_coverage[0, 2] == rl.rl_coverage[0, 2]


# ---- the edges hspf_rlfa_device's suite has: tile edge, totals beyond 32 bits, zero-cost links, unreachable and pruned vertices,
# overload, self-loops, and a seeded sweep.  Every seed was chosen on the CPU so that the MODEL shows the class (asserted first).

def all_repairs(case, wr):
    return {int(e): T.repairs(case.fwd.dist, case.rdist, case.graph, case.cand, 0, case.nbr_row, e, wr.space_flags[e], wr.space_via[e])
            for e in np.flatnonzero(case.cand.nbr != M.NONE)}


@pytest.mark.parametrize("n", [255, 256, 257])
def test_rings_with_chords_at_the_tile_edge(spf_ctx, n):
    """The winner of both slots is vertex n - 1: the last valid lane of the one partial tile (255), the last lane of a full
    tile (256), the only valid lane of the second tile (257)."""
    seed, root = TILE_EDGE[n]
    case = Case(ring_chords(n, seed, 1, 9, chords=4), root)

    def need(wr, wt):
        ks = np.flatnonzero(case.cand.nbr != M.NONE)
        assert any(n - 1 in (int(wt.ti_p[e]), int(wt.ti_q[e])) for e in ks) and wt.td_coverage[2] > 0
    check_one(spf_ctx, case, need=need)


def test_totals_beyond_32_bits_saturate_and_tie(spf_ctx):
    """The five-ring with 0x7FFFFFF0 on every link but 2-3: every repair of the link 2-3 adds three of them.  Six repairs
    saturate at 0xFFFFFFFE and tie: the single node with the smallest p wins."""
    case = Case(M.csr(5, M.both([(0, 1, BIG), (1, 2, BIG), (2, 3, 1), (3, 4, BIG), (4, 0, BIG)])), 2)

    def need(wr, wt):
        e = slot_of(case, 3)
        reps = all_repairs(case, wr)[e]
        assert sum(1 for r in reps if r[0] == T.SAT) >= 2 and len({r[1] for r in reps if r[0] == T.SAT}) == 2      # nodes and pairs tie
        assert (wt.ti_kind[e], wt.ti_p[e], wt.ti_metric[e]) == (T.KIND_NODE, 0, 0xFFFFFFFE) and wt.ti_counts[e].tolist() == [2, 4]
    check_one(spf_ctx, case, need=need)


def test_saturated_pair_with_two_q_at_different_true_totals(spf_ctx):
    """S = 0 - N = 2 - p = 3, E = 1; p reaches E through q = 4 at 0x60000000 + 0x60000000 and through q = 5 at 0x50000000 +
    0x50000000; both totals are beyond 32 bits, so both are 0xFFFFFFFE and the order is (total, q, position): q = 4, the dearer
    one before the clamp.  No single node: 4 and 5 are in no extended P-space, 3 is not in Q."""
    B1, B2 = 0x60000000, 0x50000000
    case = Case(M.csr(6, M.both([(0, 1, 1), (0, 2, 1), (2, 3, BIG), (3, 4, B1), (3, 5, B2), (4, 1, B1), (5, 1, B2)])), 0)

    def need(wr, wt):
        e = slot_of(case, 1)
        reps = all_repairs(case, wr)[e]
        assert sorted((r[1], r[2], r[3]) for r in reps) == [(T.KIND_PAIR, 3, 4), (T.KIND_PAIR, 3, 5)] and all(r[0] == T.SAT for r in reps)
        rel = 1 + BIG                                                        # d(S, p); 3 is in P, released by S itself
        assert case.fwd.dist[0, 3] == rel and wt.ti_via[e] == T.VIA_SELF
        assert rel + 2 * B1 > rel + 2 * B2 > T.SAT                           # different totals before the clamp, the larger q the cheaper
        assert (wt.ti_kind[e], wt.ti_p[e], wt.ti_q[e], wt.ti_link[e], wt.ti_metric[e]) == (T.KIND_PAIR, 3, 4, 1, 0xFFFFFFFE)
        assert wt.ti_counts[e].tolist() == [0, 2]
    check_one(spf_ctx, case, need=need)


def test_zero_cost_links(spf_ctx):
    case = Case(ring_chords(300, 8, 1, 6, chords=300, zero_share=0.01), 17)

    def need(wr, wt):
        rp, _, met, _ = case.graph
        ks = np.flatnonzero(case.cand.nbr != M.NONE)
        assert (wt.ti_kind[ks] != 0).all() and wt.ti_counts[ks, 1].min() > 0
        assert any(r[1] == T.KIND_PAIR and met[rp[r[2]] + r[4]] == 0 for reps in all_repairs(case, wr).values() for r in reps)      # a forced link at cost 0
    check_one(spf_ctx, case, need=need)


def test_unreachable_island_is_in_no_repair(spf_ctx):
    case = Case(with_island(ring_chords(100, 3)), 44)

    def need(wr, wt):
        ks = np.flatnonzero(case.cand.nbr != M.NONE)
        assert (wt.ti_kind[ks] != 0).all() and not wt.td_kind[100:].any() and wt.td_coverage[0] == 99
        assert all(r[2] < 100 and r[3] < 100 for reps in all_repairs(case, wr).values() for r in reps)
    check_one(spf_ctx, case, need=need)


def test_pruned_vertices_are_in_no_repair(spf_ctx):
    case = Case(ring_chords(120, PRUNE_SEED, 1, 400), 7, maxp=1023)

    def need(wr, wt):
        pruned = case.fwd.dist[0] == R.INF
        ks = np.flatnonzero(case.cand.nbr != M.NONE)
        assert pruned.any() and not pruned.all() and (case.fwd.dist[1:][:, pruned] != R.INF).any()      # a neighbour still reaches some of them
        assert (wt.ti_kind[ks] != 0).any() and wt.ti_counts[ks, 1].min() > 0 and not wt.td_kind[pruned].any()
        assert all(not pruned[r[2]] and not pruned[r[3]] for reps in all_repairs(case, wr).values() for r in reps)
    check_one(spf_ctx, case, need=need)


def test_protected_link_to_an_overloaded_neighbour(spf_ctx):
    """ring8, S = 0, the neighbour E = 1 overloaded: its own slot is repaired by the node 4 either way; the slot of 7 would be
    repaired through 1 and is not, unless the overload is ignored."""
    case = Case(ring8(no_transit=[1]), 0)
    e1, e7 = slot_of(case, 1), slot_of(case, 7)
    assert case.cand.cflags[e1] & M.C_NO_TRANSIT
    plain, ign = want_of(case, 0)[1], want_of(case, M.IGNORE_OVERLOAD)[1]
    assert (plain.ti_kind[e1], plain.ti_p[e1]) == (T.KIND_NODE, 4) and plain.ti_kind[e7] == T.KIND_NONE and plain.td_coverage[4] > 0
    assert (ign.ti_kind[e7], ign.ti_p[e7]) == (T.KIND_NODE, 2) and ign.td_coverage[4] == 0
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD))


def test_self_loop_in_the_row_of_a_pq_node(spf_ctx):
    """The six-ring with a link 3 -> 3: 3 is in the extended P-space and in Q, so the link would count as a pair (3, 3) if a
    vertex's links to itself were not skipped: two pairs, not three."""
    case = Case(M.csr(6, M.both([(v, (v + 1) % 6, 1) for v in range(6)]) + [(3, 3, 1)]), 0)

    def need(wr, wt):
        e = slot_of(case, 1)
        rp, col, _, _ = case.graph
        assert 3 in col[rp[3]:rp[4]] and wr.space_flags[e][3] & (R.IN_P | R.IN_XP) and wr.space_flags[e][3] & R.IN_Q
        assert (wt.ti_kind[e], wt.ti_p[e], wt.ti_metric[e]) == (T.KIND_NODE, 3, 5) and wt.ti_counts[e].tolist() == [1, 2]
    check_one(spf_ctx, case, need=need)


def test_seeded_sweep_of_forty_graphs(spf_ctx):
    """40 graphs of the generator of tests/test_host_tilfa.py with 12 to 60 routers (tests/_frr_chains.py: sweep_graphs), half of
    them with a cost per direction, a quarter with zero-cost links, a quarter with an overloaded router; one seeded root each,
    none skipped.  Over the sweep the MODEL shows at least five slots of every ti_kind and a destination in every td_kind
    class (tests/test_host_tilfa.py holds the seed to that on the CPU)."""
    import _frr_chains as F
    cases = [Case(g, root) for g, root, _ in F.sweep_graphs()]
    assert len(cases) == 40 and all(12 <= len(c.graph[3]) <= 60 for c in cases)
    F.check_sweep_classes([(np.flatnonzero(c.cand.nbr != M.NONE), want_of(c)[1]) for c in cases])
    for c in cases:
        check_one(spf_ctx, c)
