"""hspf_lfa_ecmp_device on the GPU against the numpy model (tests/_lfa_ecmp_model.py) over the CPU oracle's SPTs: ea_ptr, the four
entry arrays, the coverage and the total, bit for bit.  Shapes: the hand cases, the 256-destination tile edge, one / two mask words
(the LDS and the cache instantiation, the r-th-set-bit walk across a word boundary), three protected roots over one table set with
an empty segment in the middle, no ECMP at all, more tiles than one pass of the scan consumes, the capacity convention, seeded
random graphs through SpfContext.lfa_ecmp, a patched graph, the argument errors, and hspf_lfa_device around the call."""
import ctypes

import numpy as np
import pytest

import _lfa_ecmp_cases as C
import _lfa_ecmp_model as EM
import _lfa_model as M
from test_gpu_lfa import Tables, run_lfa

pytestmark = pytest.mark.gpu

SENTINEL = 0x07070707


def run_ecmp(ctx, tab, protect, lfa_flags=0, cap=None):
    """The call on the rows of `tab`.  cap None: the two sizing calls, every array checked to be untouched beyond the total.
    Returns (total, ea_ptr, ea_primary, ea_slot, ea_metric, ea_flags, ea_coverage) on the host."""
    import torch
    dev = torch.device("cuda:0")
    P, n = len(protect), tab.n
    args = (n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect)
    ptr = torch.full((P * n + 1,), 7, dtype=torch.int32, device=dev)
    if cap is None:
        cap = ctx.lfa_ecmp_device(*args, ea_ptr_ptr=ptr.data_ptr(), lfa_flags=lfa_flags)
        assert int(ptr[-1].item()) == cap
        ptr.fill_(7)
    pri, slot, met = (torch.full((cap + 3,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3))
    fl = torch.full((cap + 3,), 7, dtype=torch.uint8, device=dev)
    cov = torch.full((P, EM.COVERAGE_WORDS), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    total = ctx.lfa_ecmp_device(*args, ea_ptr_ptr=ptr.data_ptr(), cap_entries=cap, ea_primary_ptr=pri.data_ptr(), ea_slot_ptr=slot.data_ptr(),
                                ea_metric_ptr=met.data_ptr(), ea_flags_ptr=fl.data_ptr(), ea_coverage_ptr=cov.data_ptr(), lfa_flags=lfa_flags)
    h = lambda t, dt: t.cpu().numpy().view(dt)      # noqa: E731
    for t in (pri, slot, met):
        assert (h(t, np.uint32)[cap:] == SENTINEL).all()                 # nothing is written beyond the capacity
    assert (h(fl, np.uint8)[cap:] == 7).all()
    k = min(total, cap)
    return total, h(ptr, np.uint32), h(pri, np.uint32)[:k], h(slot, np.uint32)[:k], h(met, np.uint32)[:k], h(fl, np.uint8)[:k], h(cov, np.uint32)


def same(got, want: EM.Ecmp, P=1):
    total, ptr, pri, slot, met, fl, cov = got
    assert total == want.total
    assert np.array_equal(ptr, want.ea_ptr), np.flatnonzero(ptr != want.ea_ptr)[:8]
    for name, g in (("ea_primary", pri), ("ea_slot", slot), ("ea_metric", met), ("ea_flags", fl)):
        assert np.array_equal(g, getattr(want, name)), (name, np.flatnonzero(g != getattr(want, name))[:8])
    assert np.array_equal(cov, want.ea_coverage.reshape(P, EM.COVERAGE_WORDS)), (cov, want.ea_coverage)


def plan(graph, root):
    """(model candidates, product candidates, roots, nbr_row, W) of one protected root; the two candidate tables agree."""
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    mc, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    pc = E.lfa_candidates(rp, col, met, vf, root)
    for a, b in ((pc.nbr, mc.nbr), (pc.cost, mc.cost), (pc.root_link, mc.root_link), (pc.cflags, mc.cflags)):
        assert np.array_equal(a, b)
    return mc, pc, roots, nbr_row, max(go.mask_words(rp, col, met, vf, roots), (len(mc.nbr) + 63) // 64)


def check_one(ctx, graph, root, run_flags=0, lfa_flags=0, need=None):
    mc, pc, roots, nbr_row, W = plan(graph, root)
    tab = Tables(ctx, graph, 0xFFFFFFFF, roots, run_flags, W)
    try:
        want = EM.lfa_ecmp(tab.ref.dist, tab.ref.flags, tab.ref.mask, mc, 0, nbr_row, lfa_flags)
        if need is not None:
            need(want)                                   # non-vacuity: a condition on the MODEL, before anything is compared
        same(run_ecmp(ctx, tab, [(0, pc, nbr_row)], lfa_flags), want)
    finally:
        tab.free()
    return want


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_cases(spf_ctx, name):
    case = C.HAND[name]()
    want = check_one(spf_ctx, case[0], case[1], C.RUN_FLAGS.get(name, 0), case[2])
    for f, w in zip(EM.FIELDS, C.expected(case)):        # the model's arrays are the hand-written ones
        assert np.array_equal(getattr(want, f), w), f


@pytest.mark.parametrize("n", [5, 255, 256, 257])
def test_ring_with_chords_at_the_tile_edge(spf_ctx, n):
    """n = 1 + K, and one vertex below / at / above the 256-destination tile."""
    def need(want):
        assert want.total > 0 and want.ea_coverage[2] > 0
        assert want.ea_dest.max() >= n - 4                                        # ECMP destinations up to the end (n = 257: vertex 256, alone in its tile)
    check_one(spf_ctx, *C.ring_chords(n, 4), need=need)


@pytest.mark.parametrize("K", [64, 65])
def test_star_centre_one_and_two_mask_words(spf_ctx, K):
    """64 slots: one mask word, tables in LDS; 65: two words, tables through the caches, and the r-th set bit of P is found across
    the word boundary (popcount(P) of the far vertex is K)."""
    def need(want):
        far = K + 1
        assert want.ea_ptr[far + 1] - want.ea_ptr[far] == K and want.ea_primary.max() == K - 1
        assert (want.ea_flags[want.ea_dest == far] == C.L | C.N | C.D | C.P).all()
    check_one(spf_ctx, *C.star(K), need=need)


def test_three_protected_roots_share_one_table_set_the_middle_one_without_ecmp(spf_ctx):
    """The diamond 0 - {1, 2} - 3 with the tail 3 - 4 - 5, every vertex a row.  Root 0 and root 3 have ECMP destinations, root 5 (one
    slot) has none: its segment of the stream is empty, and the stream crosses two root boundaries."""
    from holo_amd import engine as E
    graph = M.csr(6, M.both([(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1)]))
    roots = np.arange(6, dtype=np.uint32)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, 1)
    try:
        parts, protect = [], []
        for S in (0, 5, 3):
            mc = M.candidates(*graph, S)
            nbr_row = np.where(mc.nbr == M.NONE, 0, mc.nbr).astype(np.uint32)        # row v holds the SPT rooted at v
            parts.append(EM.lfa_ecmp(tab.ref.dist, tab.ref.flags, tab.ref.mask, mc, S, nbr_row))
            protect.append((S, E.lfa_candidates(*graph, S), nbr_row))
        assert parts[0].total == 6 and parts[1].total == 0 and parts[2].total == 2
        same(run_ecmp(spf_ctx, tab, protect), EM.stack(parts, 6), P=3)
    finally:
        tab.free()


def test_no_ecmp_anywhere(spf_ctx):
    want = check_one(spf_ctx, *C.chain(40))
    assert want.total == 0 and not want.ea_ptr.any() and not want.ea_coverage.any()


def test_more_tiles_than_one_pass_of_the_scan(spf_ctx):
    """k_events_scan, the one workgroup that scans the tile totals, consumes 1024 tiles per pass (EA_SCAN_PASS in
    spf_lfa_ecmp.hip.h).  A 515 x 515 unit-cost grid rooted in a corner has 265 225 vertices = 1 037 tiles of 256 destinations, so
    the scan carries over one pass boundary; nearly every vertex has both of the root's links as primaries."""
    import torch
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph, root = C.grid(515, 515)
    roots = np.array([0, 1, 515], np.uint32)                 # the corner and its two neighbours
    pc = E.lfa_candidates(*graph, root)
    assert pc.nbr.tolist() == [1, 515] and pc.root_link.tolist() == [0, 1] and pc.cost.tolist() == [1, 1] and not pc.cflags.any()
    mc, nbr_row = M.Cand(0, pc.nbr.copy(), pc.cost.copy(), pc.root_link.copy(), pc.cflags.copy()), np.array([1, 2], np.uint32)
    ref = go.run(*graph, 0xFFFFFFFF, roots, 0, go.HEAP, mask_words_=1)      # (the other two variants run out of memory on this grid)
    want = EM.lfa_ecmp(ref.dist, ref.flags, ref.mask, mc, 0, nbr_row)
    assert (len(want.ea_ptr) - 1 + 255) // 256 > 1024 and want.total > 500000
    assert want.ea_ptr[1024 * 256] > 0 and want.ea_ptr[-1] > want.ea_ptr[1024 * 256]           # entries on both sides of the boundary
    tab = Tables.__new__(Tables)
    tab.n, tab.R, tab.W, tab.ref = len(graph[3]), 3, 1, ref
    tab.G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        dev = torch.device("cuda:0")
        tab.dist = torch.empty((3, tab.n), dtype=torch.int32, device=dev)
        tab.flags = torch.empty((3, tab.n), dtype=torch.int16, device=dev)
        tab.mask = torch.empty((3, tab.n, 1), dtype=torch.int64, device=dev)
        spf_ctx.run_device(tab.G, roots, 0, dist_ptr=tab.dist.data_ptr(), flags_ptr=tab.flags.data_ptr(), mask_ptr=tab.mask.data_ptr(), mask_words=1)
        same(run_ecmp(spf_ctx, tab, [(0, pc, nbr_row)]), want)
    finally:
        tab.free()


def test_capacity_convention(spf_ctx):
    """cap_entries = 0 with NULL arrays; total - 1: returns 0 with ea_ptr and the total right; total: everything."""
    graph, root = C.ring_chords(257, 4)
    mc, pc, roots, nbr_row, W = plan(graph, root)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        import torch
        want = EM.lfa_ecmp(tab.ref.dist, tab.ref.flags, tab.ref.mask, mc, 0, nbr_row)
        assert want.total > 2
        ptr = torch.full((tab.n + 1,), 7, dtype=torch.int32, device="cuda:0")
        total = spf_ctx.lfa_ecmp_device(tab.n, tab.R, W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), [(0, pc, nbr_row)],
                                        ea_ptr_ptr=ptr.data_ptr())
        assert total == want.total and np.array_equal(ptr.cpu().numpy().view(np.uint32), want.ea_ptr)
        got = run_ecmp(spf_ctx, tab, [(0, pc, nbr_row)], cap=want.total - 1)
        assert got[0] == want.total and np.array_equal(got[1], want.ea_ptr)
        same(run_ecmp(spf_ctx, tab, [(0, pc, nbr_row)], cap=want.total), want)
    finally:
        tab.free()


@pytest.mark.parametrize("seed", C.GPU_SEEDS)
def test_random_graphs_through_the_context(spf_ctx, seed):
    """Pseudonodes, overloaded routers, zero-cost links and asymmetric costs, through SpfContext.lfa_ecmp (plan, run, both calls)."""
    graph, root = C.random_isis_like(seed)
    lf = M.IGNORE_OVERLOAD if seed % 4 == 3 else 0
    G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        cand, got = spf_ctx.lfa_ecmp(G, root, lfa_flags=lf)
    finally:
        G.free()
    mc, want = EM.model(graph, root, 0, lf)
    assert np.array_equal(cand.nbr, mc.nbr)
    same((got.total, got.ea_ptr, got.ea_primary, got.ea_slot, got.ea_metric, got.ea_flags, got.ea_coverage), want)


def test_the_random_graphs_show_every_class():
    """On the MODEL (no GPU work): the 40 graphs hold entries of every kind."""
    cov = np.zeros(EM.COVERAGE_WORDS, np.int64)
    for seed in C.GPU_SEEDS:
        graph, root = C.random_isis_like(seed)
        cov += EM.model(graph, root, 0, M.IGNORE_OVERLOAD if seed % 4 == 3 else 0)[1].ea_coverage
    dests, entries, alt, node, down, prim, full = cov
    assert dests > 100 and entries - alt > 0 and alt - node > 0 and node > 0 and down > 0 and alt - down > 0 and prim > 0 and alt - prim > 0 and 0 < full < dests, cov


def test_patched_graph(spf_ctx):
    """S = 0 reaches D = 3 through A = 1 alone while B - D costs 3; one hspf_graph_patch of the rows of B and D makes it 1 and D an
    ECMP destination.  The call on the patched graph equals the model, and a fresh upload."""
    before = M.csr(4, M.both([(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 3)]))
    after = M.csr(4, M.both([(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)]))
    assert EM.model(before, 0)[1].total == 0
    _, want = EM.model(after, 0)
    assert want.total == 2
    rp, col, met, vf = after
    G = spf_ctx.upload(*before, 0xFFFFFFFF)
    F = spf_ctx.upload(*after, 0xFFFFFFFF)
    try:
        _, empty = spf_ctx.lfa_ecmp(G, 0)
        assert empty.total == 0
        G.patch([2, 3], [(col[rp[v]:rp[v + 1]], met[rp[v]:rp[v + 1]]) for v in (2, 3)], [0, 0])
        for g in (G, F):
            _, got = spf_ctx.lfa_ecmp(g, 0)
            same((got.total, got.ea_ptr, got.ea_primary, got.ea_slot, got.ea_metric, got.ea_flags, got.ea_coverage), want)
    finally:
        G.free()
        F.free()


def test_argument_errors_leave_the_outputs_untouched(spf_ctx):
    import torch
    from holo_amd import _lib as L
    from holo_amd import engine as E
    graph, root, _, _ = C.diamond()
    mc, pc, roots, nbr_row, W = plan(graph, root)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        dev = torch.device("cuda:0")
        n = tab.n
        ptr = torch.full((n + 1,), 7, dtype=torch.int32, device=dev)
        ent = [torch.full((8,), 7, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.full((8,), 7, dtype=torch.uint8, device=dev)]
        cov = torch.full((1, EM.COVERAGE_WORDS), 7, dtype=torch.int32, device=dev)
        arr, keep = spf_ctx._protect_array([(0, pc, nbr_row)], "test")
        lib, hd = spf_ctx.lib, spf_ctx.handle
        good = dict(n=n, R=tab.R, W=W, dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr(), prot=arr, n_prot=1, cap=8,
                    out=[ptr.data_ptr()] + [t.data_ptr() for t in ent] + [cov.data_ptr()], total=True)

        def call(**kw):
            a = dict(good, **kw)
            out = L.HspfLfaEcmpOut(*[p or None for p in a["out"]])
            total = ctypes.c_uint64(77)
            rc = lib.hspf_lfa_ecmp_device(hd, a["n"], a["R"], a["W"], a["dist"] or None, a["flags"] or None, a["mask"] or None, a["prot"], a["n_prot"], 0,
                                          a["cap"], ctypes.byref(out), ctypes.byref(total) if a["total"] else None)
            return rc, total.value

        def null_out(i):
            o = list(good["out"])
            o[i] = 0
            return o
        bad_row, _k1 = spf_ctx._protect_array([(tab.R, pc, nbr_row)], "test")
        bad_nbr_row, _k2 = spf_ctx._protect_array([(0, pc, nbr_row + tab.R)], "test")
        wide = E.LfaCandidates(0, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        too_many, _k3 = spf_ctx._protect_array([(0, wide, np.zeros(65, np.uint32))], "test")
        # the host-side bound: n_vertices * n_slots summed over the protected roots reaches 2^32 (nothing that large is allocated:
        # the check comes before any table is read)
        errors = [dict(dist=0), dict(flags=0), dict(mask=0), dict(out=null_out(0)), dict(total=False)] + [dict(out=null_out(i)) for i in range(1, 6)] + \
                 [dict(n=0), dict(R=0), dict(W=0), dict(n_prot=0), dict(prot=bad_row), dict(prot=bad_nbr_row), dict(prot=too_many),
                  dict(n=1 << 31, W=1 << 10, prot=too_many)]
        for kw in errors:
            rc, total = call(**kw)
            assert rc == -1, kw                                                 # HSPF_E_INVAL
            assert b"hspf_lfa_ecmp_device" in lib.hspf_last_error(hd), (kw, lib.hspf_last_error(hd))
            assert total == 77 or not kw.get("total", True)
        for t in [ptr] + ent + [cov]:
            assert (t.cpu().numpy() == 7).all()
        rc, total = call()                                                      # and the good call goes through
        assert rc == 0 and total == 2
    finally:
        tab.free()


def test_lfa_device_before_and_after_the_call_is_unchanged(spf_ctx):
    """The two calls share the staged tables and the scalars on the context."""
    graph, root = C.ring_chords(257, 4)
    mc, pc, roots, nbr_row, W = plan(graph, root)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        before = run_lfa(spf_ctx, tab, [(0, pc, nbr_row)])
        assert run_ecmp(spf_ctx, tab, [(0, pc, nbr_row)])[0] > 0
        after = run_lfa(spf_ctx, tab, [(0, pc, nbr_row)])
        for b, a in zip(before, after):
            assert np.array_equal(b, a)
        want = M.lfa(tab.ref.dist, tab.ref.flags, tab.ref.mask, mc, 0, nbr_row)
        assert np.array_equal(after[2][0], want.alt_flags) and np.array_equal(after[0][0], want.alt_slot)
    finally:
        tab.free()
