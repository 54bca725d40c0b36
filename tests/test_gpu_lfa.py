"""hspf_lfa_device on the GPU against the numpy model (tests/_lfa_model.py) over the CPU oracle's SPTs: every output array and the
coverage, bit for bit.  The tables the kernel reads come from hspf_run_device on each engine configuration; the expected values
never touch the engine.  Shapes: the smallest at which the kernel can go wrong — the 256-destination tile edge, one / two mask
words and the edge of the one-word instantiation (63, 64, 65, 128 slots), LAN pseudonodes, overload, unreachable vertices,
sums beyond 32 bits, zero-cost links, several protected roots over one table set."""
import ctypes

import numpy as np
import pytest

import _lfa_model as M
from _engines import both_engines

pytestmark = pytest.mark.gpu

WIDE = 0xFE000000
# seeds of the random grids, chosen on the CPU so that the MODEL shows every class (asserted below before anything is compared)
GRID_SEEDS = {255: 2, 256: 1, 257: 1}


def _rng(seed):
    return np.random.default_rng(seed)


def grid(n, seed, lo=1, hi=20, width=16):
    """4-neighbour grid of `n` vertices, `width` per row (the last row may be short), one seeded cost per link."""
    r = _rng(seed)
    und = [(v, v + 1) for v in range(n) if (v + 1) % width and v + 1 < n] + [(v, v + width) for v in range(n) if v + width < n]
    return M.csr(n, M.both([(a, b, int(r.integers(lo, hi + 1))) for a, b in und]))


def torus(side=16):
    und = []
    for y in range(side):
        for x in range(side):
            v = y * side + x
            und += [(v, y * side + (x + 1) % side), (v, ((y + 1) % side) * side + x)]
    return M.csr(side * side, M.both([(a, b, 1) for a, b in und]))


def hub(k, seed):
    """Vertex 0 with `k` router neighbours and a sparse random mesh among them."""
    r = _rng(seed)
    und = [(0, v, int(r.integers(1, 21))) for v in range(1, k + 1)]
    seen = set()
    for _ in range(2 * k):
        a, b = (int(x) for x in r.integers(1, k + 1, 2))
        if a != b and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
            und.append((a, b, int(r.integers(1, 21))))
    return M.csr(k + 1, M.both(und))


def lan():
    """0 = pseudonode of a LAN with S = 1, E = 2, A = 3, B = 4; C = 5 on a p2p link of S; D = 6 behind all of them, nearest
    through E: A and B sit behind the primary's first link (never offered), C is."""
    links = []
    for r_ in (1, 2, 3, 4):
        links += [(r_, 0, 10), (0, r_, 0)]
    links += M.both([(1, 5, 10), (2, 6, 1), (3, 6, 5), (4, 6, 5), (5, 6, 5), (6, 7, 1)])
    return M.csr(8, links, net=[0])


def mesh(n, seed, lo, hi, extra=2.0, zero_share=0.0, no_transit=()):
    """A ring (connected) plus random chords; `zero_share` of the links cost 0."""
    r = _rng(seed)
    und = {(v, (v + 1) % n) for v in range(n)}
    while len(und) < int(n * extra):
        a, b = (int(x) for x in r.integers(0, n, 2))
        if a != b and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        c = int(r.integers(lo, hi + 1))
        if zero_share and r.random() < zero_share:
            c = 0
        links.append((a, b, c))
    return M.csr(n, M.both(links), no_transit=no_transit)


def with_island(graph, n_island=5):
    """The graph plus a ring of `n_island` vertices nothing leads to."""
    rp, col, met, vf = graph
    n = len(vf)
    links = [(u, int(col[k]), int(met[k])) for u in range(n) for k in range(rp[u], rp[u + 1])]
    links += M.both([(n + i, n + (i + 1) % n_island, 1) for i in range(n_island)])
    g = M.csr(n + n_island, links)
    g[3][:n] = vf
    return g


class Tables:
    """The SPT rows of `roots` twice: on the device from the engine (hspf_run_device), on the host from the oracle."""

    def __init__(self, ctx, graph, maxp, roots, run_flags, W):
        import torch
        from oracle import graph_oracle as go
        rp, col, met, vf = graph
        self.n, self.R, self.W = len(vf), len(roots), W
        self.ref = go.run(rp, col, met, vf, maxp, roots, run_flags, go.MAP, mask_words_=W)
        dev = torch.device("cuda:0")
        self.G = ctx.upload(rp, col, met, vf, maxp)
        assert self.G.mask_words(roots) <= W
        self.dist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
        self.flags = torch.empty((self.R, self.n), dtype=torch.int16, device=dev)
        self.mask = torch.empty((self.R, self.n, W), dtype=torch.int64, device=dev)
        ctx.run_device(self.G, roots, run_flags, dist_ptr=self.dist.data_ptr(), flags_ptr=self.flags.data_ptr(), mask_ptr=self.mask.data_ptr(),
                       mask_words=W)

    def free(self):
        self.G.free()


def run_lfa(ctx, tab, protect, lfa_flags=0, masks=True):
    """protect: [(root_row, product candidates, nbr_row)].  Returns the six host arrays ([P, n] ...; masks None when skipped)."""
    import torch
    dev = torch.device("cuda:0")
    P, n, W = len(protect), tab.n, tab.W
    slot = torch.full((P, n), 7, dtype=torch.int32, device=dev)
    metric = torch.full((P, n), 7, dtype=torch.int32, device=dev)
    fl = torch.full((P, n), 7, dtype=torch.uint8, device=dev)
    cov = torch.full((P, 5), 7, dtype=torch.int32, device=dev)
    cm = torch.full((P, n, W), 7, dtype=torch.int64, device=dev) if masks else None
    nm = torch.full((P, n, W), 7, dtype=torch.int64, device=dev) if masks else None
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.lfa_device(n, tab.R, W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect, alt_slot_ptr=slot.data_ptr(),
                   alt_metric_ptr=metric.data_ptr(), alt_flags_ptr=fl.data_ptr(), coverage_ptr=cov.data_ptr(),
                   cand_mask_ptr=cm.data_ptr() if masks else 0, node_mask_ptr=nm.data_ptr() if masks else 0, lfa_flags=lfa_flags)
    h = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)      # noqa: E731
    return h(slot, np.uint32), h(metric, np.uint32), h(fl, np.uint8), h(cm, np.uint64), h(nm, np.uint64), h(cov, np.uint32)


def check_one(ctx, graph, root, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=(0,), need=None, w_min=1, need_exact_row=False):
    """One protected root with [root] + its neighbour routers as the rows; returns the model's result of the first lfa_flags."""
    from holo_amd import engine as E
    rp, col, met, vf = graph
    mc, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    pc = E.lfa_candidates(rp, col, met, vf, root)
    for a, b in ((pc.nbr, mc.nbr), (pc.cost, mc.cost), (pc.root_link, mc.root_link), (pc.cflags, mc.cflags)):
        assert np.array_equal(a, b)
    from oracle import graph_oracle as go
    W = max(go.mask_words(rp, col, met, vf, roots), (len(mc.nbr) + 63) // 64, w_min)
    tab = Tables(ctx, graph, maxp, roots, run_flags, W)
    first = None
    try:
        if need_exact_row:                                   # a row of the table set comes from the dynamic-pop-order path (HSPF_RF_EXACT)
            assert ((tab.flags.cpu().numpy().view(np.uint16) & 2) != 0).any(axis=1).any()
        for lf in lfa_flags:
            want = M.lfa(tab.ref.dist, tab.ref.flags, tab.ref.mask, mc, 0, nbr_row, lf)
            if need is not None and first is None:
                need(want)                                   # non-vacuity: a condition on the MODEL, before anything is compared
            got = run_lfa(ctx, tab, [(0, pc, nbr_row)], lf)
            for name, g, w in zip(("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask", "coverage"), got,
                                  (want.alt_slot, want.alt_metric, want.alt_flags, want.cand_mask, want.node_mask, want.coverage)):
                assert np.array_equal(g[0], w), (name, lf, np.flatnonzero((g[0] != w).reshape(len(w), -1).any(axis=1))[:8])
            first = first or want
    finally:
        tab.free()
    return first


def every_class(want):
    has, ecmp, alt, node, down = (int(x) for x in want.coverage)
    assert has - ecmp - alt > 0, "no destination without an alternate"
    assert alt - node > 0, "no link-only destination"
    assert node > 0 and ecmp > 0 and down > 0, want.coverage


@both_engines
@pytest.mark.parametrize("n", [255, 256, 257])
def test_random_grids_at_the_tile_edge(spf_ctx, n):
    check_one(spf_ctx, grid(n, GRID_SEEDS[n]), n // 2 + 3, need=every_class)


@both_engines
def test_torus_unit_costs_maximal_ecmp(spf_ctx):
    want = check_one(spf_ctx, torus(16), 37)
    assert want.coverage[1] > 200                            # nearly every destination is ECMP


@both_engines
@pytest.mark.parametrize("k", [63, 64, 65, 128])
def test_hub_root_one_and_two_mask_words(spf_ctx, k):
    want = check_one(spf_ctx, hub(k, 100 + k), 0)
    assert want.cand_mask.shape[1] == (1 if k <= 64 else 2)
    assert want.coverage[2] > 0 and want.coverage[3] > 0
    if k > 64:
        assert want.cand_mask[:, 1].any() and (want.alt_slot[want.alt_slot != M.NONE] >= 64).any()      # the second word is in use


@both_engines
@pytest.mark.parametrize("run_flags", [0, 1])                # HSPF_RUN_NET_NEXTHOPS off / on
def test_lan_candidates_behind_the_primarys_pseudonode(spf_ctx, run_flags):
    want = check_one(spf_ctx, lan(), 1, run_flags=run_flags)
    c = M.candidates(*lan(), 1)
    k_c = int(np.flatnonzero(c.nbr == 5)[0])
    ks = [int(np.flatnonzero(c.nbr == v)[0]) for v in (3, 4)]
    for D in (6, 7):                                         # primary: through the LAN to E = 2
        assert want.alt_slot[D] == k_c and want.cand_mask[D, 0] == 1 << k_c
        assert not any(int(want.cand_mask[D, 0]) >> k & 1 for k in ks)


def overloaded_detour():
    """mesh(40) with the first neighbour N of root 0 overloaded and the direct 0 - N link made dear, so that 0 reaches N over a
    detour: the 0 - N slot is then no primary of D = N but a candidate for it — the one destination an overloaded neighbour may
    protect (`N == D`)."""
    g = mesh(40, 5, 1, 9, extra=2.5)
    rp, col, met, vf = g
    c = M.candidates(*g, 0)
    k = int(np.flatnonzero(c.nbr != M.NONE)[0])
    ovl = int(c.nbr[k])
    for u, v in ((0, ovl), (ovl, 0)):
        for e in range(rp[u], rp[u + 1]):
            if col[e] == v:
                met[e] = 60
    vf[ovl] |= M.VF_NO_TRANSIT
    return g, k, ovl


@both_engines
def test_overloaded_neighbour_with_and_without_ignore(spf_ctx):
    g, k, ovl = overloaded_detour()
    seen = []

    def need(want):                                          # on the MODEL, before anything is compared
        hit = ((want.cand_mask[:, k // 64] >> np.uint64(k % 64)) & np.uint64(1)) != 0
        seen.append(hit)
        assert np.flatnonzero(hit).tolist() == [ovl]         # without the flag: an alternate for itself, and for nothing else
        assert want.alt_flags[ovl] & M.LINK_PROTECT

    check_one(spf_ctx, g, 0, lfa_flags=(0, M.IGNORE_OVERLOAD), need=need)
    from oracle import graph_oracle as go
    mc, roots, nbr_row = M.protect_one(*g, 0)
    t = go.run(*g, 0xFFFFFFFF, roots, 0, go.MAP, mask_words_=1)
    ign = M.lfa(t.dist, t.flags, t.mask, mc, 0, nbr_row, M.IGNORE_OVERLOAD)
    hit = ((ign.cand_mask[:, 0] >> np.uint64(k)) & np.uint64(1)) != 0
    assert hit[ovl] and hit.sum() > 1                        # with it: for other destinations too (compared above)


@both_engines
@pytest.mark.parametrize("run_flags", [0, 1])
def test_random_lsdb_with_networks(spf_ctx, run_flags):
    from holo_amd import synth
    g = synth.random_lsdb(120, 15, 3.0, 11, metric_hi=9)
    graph = (g.row_ptr, g.col, g.metric, g.vflags)
    roots = [r for r in range(15, 135) if not (g.vflags[r] & 0x06) and (M.candidates(*graph, r).nbr != M.NONE).sum() >= 3][:2]
    assert len(roots) == 2
    for r in roots:
        check_one(spf_ctx, graph, r, maxp=g.max_path_metric, run_flags=run_flags)


@both_engines
def test_unreachable_island(spf_ctx):
    want = check_one(spf_ctx, with_island(grid(100, 9, width=10)), 44)
    assert not want.alt_flags[100:].any() and (want.alt_slot[100:] == M.NONE).all()


@both_engines
def test_wide_metrics_sums_beyond_32_bits(spf_ctx):
    g = mesh(14, 21, 0x7E000000, 0x7F000000, extra=1.6)
    want = check_one(spf_ctx, g, 0, maxp=WIDE)
    assert want.coverage[2] > 0 and (want.alt_metric > 0x7FFFFFFF).any()


@both_engines
def test_zero_cost_links(spf_ctx):
    want = check_one(spf_ctx, mesh(300, 8, 1, 6, extra=2.0, zero_share=0.01), 17, need_exact_row=True)
    assert want.coverage[2] > 0


@both_engines
def test_one_word_of_slots_in_a_two_word_table_set(spf_ctx):
    """At most 64 slots (the one-word instantiation) over tables made with two mask words: the second word of both sets is zero."""
    want = check_one(spf_ctx, grid(257, GRID_SEEDS[257]), 257 // 2 + 3, w_min=2)
    assert want.cand_mask.shape[1] == 2 and want.cand_mask[:, 0].any() and not want.cand_mask[:, 1].any()


@both_engines
@pytest.mark.parametrize("masks", [True, False])
def test_eight_protected_roots_share_one_64_row_table(spf_ctx, masks):
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph = mesh(300, 31, 1, 20, extra=1.7)
    prot_roots, rows = [], []
    for r in range(0, 300, 37):                              # 9 spread-out routers; take those whose neighbours still fit
        nb = sorted({int(x) for x in M.candidates(*graph, r).nbr if x != M.NONE})
        new = [v for v in [r] + nb if v not in rows]
        if len(rows) + len(new) <= 64 and len(prot_roots) < 8:
            rows += new
            prot_roots.append(r)
    assert len(prot_roots) == 8
    rows += [v for v in range(300) if v not in rows][:64 - len(rows)]
    roots = np.array(rows, np.uint32)
    row_of = {v: i for i, v in enumerate(rows)}
    W = go.mask_words(*graph, roots)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        protect, wants = [], []
        for r in prot_roots:
            mc = M.candidates(*graph, r)
            nbr_row = np.array([row_of.get(int(x), 0) for x in mc.nbr], np.uint32)
            protect.append((row_of[r], E.lfa_candidates(*graph, r), nbr_row))
            wants.append(M.lfa(tab.ref.dist, tab.ref.flags, tab.ref.mask, mc, row_of[r], nbr_row))
        got = run_lfa(spf_ctx, tab, protect, 0, masks)
        for i, w in enumerate(wants):
            assert np.array_equal(got[0][i], w.alt_slot) and np.array_equal(got[1][i], w.alt_metric) and np.array_equal(got[2][i], w.alt_flags)
            assert np.array_equal(got[5][i], w.coverage)
            if masks:
                assert np.array_equal(got[3][i], w.cand_mask) and np.array_equal(got[4][i], w.node_mask)
        assert got[3] is not None or not masks
    finally:
        tab.free()


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    graph = grid(30, 1, width=6)
    mc, roots, nbr_row = M.protect_one(*graph, 8)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, 1)
    try:
        pc = E.lfa_candidates(*graph, 8)
        good = run_lfa(spf_ctx, tab, [(0, pc, nbr_row)])
        import torch
        out = torch.full((30 * 4 + 30 * 4 + 30 + 5 * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
        base = out.data_ptr()
        ptrs = dict(alt_slot_ptr=base, alt_metric_ptr=base + 120, alt_flags_ptr=base + 240, coverage_ptr=base + 272)

        def expect_inval(protect=None, dist=None, **kw):
            p = dict(ptrs)
            p.update(kw)
            with pytest.raises(E.HspfError) as e:
                spf_ctx.lfa_device(30, tab.R, 1, tab.dist.data_ptr() if dist is None else dist, tab.flags.data_ptr(), tab.mask.data_ptr(),
                                   protect or [(0, pc, nbr_row)], **p)
            assert e.value.code == -1 and "hspf_lfa_device" in str(e.value)
            assert (out.cpu().numpy() == 0x5A).all()         # nothing was written: nothing was launched

        expect_inval(dist=0)                                 # a NULL required pointer (table)
        expect_inval(alt_slot_ptr=0)                         # ... (output)
        expect_inval(coverage_ptr=0)
        bad_row = nbr_row.copy()
        bad_row[np.flatnonzero(mc.nbr != M.NONE)[0]] = tab.R
        expect_inval(protect=[(0, pc, bad_row)])             # nbr_row >= n_rows
        expect_inval(protect=[(tab.R, pc, nbr_row)])         # root_row out of range
        many = E.LfaCandidates(8, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        expect_inval(protect=[(0, many, np.zeros(65, np.uint32))])      # n_slots > 64 * n_mask_words
        # the raw call with NULL prot / out
        lib = L.load()
        assert lib.hspf_lfa_device(spf_ctx.handle, 30, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), None, 1, 0, None) == -1
        # and the context still works
        again = run_lfa(spf_ctx, tab, [(0, pc, nbr_row)])
        assert all(np.array_equal(a, b) for a, b in zip(good, again))
    finally:
        tab.free()


def test_lfa_convenience_end_to_end(spf_ctx):
    """SpfContext.lfa(): candidates + one run_device for [root] + neighbours + lfa_device, results on the host."""
    graph = grid(256, GRID_SEEDS[256])
    root = 256 // 2 + 3
    G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        cand, res = spf_ctx.lfa(G, root)
    finally:
        G.free()
    from oracle import graph_oracle as go
    mc, roots, nbr_row = M.protect_one(*graph, root)
    t = go.run(*graph, 0xFFFFFFFF, roots, 0, go.MAP, mask_words_=res.cand_mask.shape[2])
    want = M.lfa(t.dist, t.flags, t.mask, mc, 0, nbr_row)
    assert np.array_equal(cand.nbr, mc.nbr)
    assert np.array_equal(res.alt_slot[0], want.alt_slot) and np.array_equal(res.alt_metric[0], want.alt_metric)
    assert np.array_equal(res.alt_flags[0], want.alt_flags) and np.array_equal(res.coverage[0], want.coverage)
    assert np.array_equal(res.cand_mask[0], want.cand_mask) and np.array_equal(res.node_mask[0], want.node_mask)
