"""hspf_rlfa_device on the GPU against the numpy model (tests/_rlfa_model.py) over the CPU oracle's SPTs: every output array and
every count, bit for bit, the optional space tables included.  Both table sets the kernel reads come from hspf_run_device — the
forward upload and the upload of hspf_csr_transpose's result — on each engine configuration; the expected values never touch the
engine.  Shapes: the smallest at which the kernels can go wrong — the 256-vertex tile edge, the 8-slot chunk edge (7, 8, 9, 17
candidates), one / two mask words (63, 64, 65, 128), LAN pseudonodes, asymmetric costs, overload, unreachable and pruned vertices,
sums beyond 32 bits, zero-cost links, several protected roots over one table set.  Every seed below was chosen on the CPU so that
the MODEL shows the class its case is for; each test asserts that on the model before anything is compared."""
import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
from _engines import both_engines

pytestmark = pytest.mark.gpu

WIDE = 0xFE000000
RINGS = {255: (3, 10), 256: (21, 254), 257: (18, 212)}      # n: (seed, protected root)
HUB_SEEDS = {7: 1, 8: 0, 9: 1, 17: 0, 63: 0, 64: 0, 65: 43, 128: 0}
ASYM_SEED = 0
PRUNE_SEED = 0
WIDE_SEED = 0


def _rng(seed):
    return np.random.default_rng(seed)


def ring_chords(n, seed, lo=1, hi=20, chords=None, asym=False, zero_share=0.0):
    """A ring of n routers plus about n / 8 chords; one seeded cost per link, or one per direction (`asym`)."""
    r = _rng(seed)
    und = {(v, (v + 1) % n) for v in range(n)}
    while len(und) < n + (n // 8 if chords is None else chords):
        a, b = (int(x) for x in r.integers(0, n, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        c1 = int(r.integers(lo, hi + 1))
        c2 = int(r.integers(lo, hi + 1)) if asym else c1
        if zero_share and r.random() < zero_share:
            c1 = c2 = 0
        links += [(a, b, c1), (b, a, c2)]
    return M.csr(n, links)


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
    """The graph of tests/test_gpu_lfa.py: 0 = pseudonode of a LAN with S = 1, E = 2, A = 3, B = 4; C = 5 on a p2p link of S;
    D = 6 behind all of them, nearest through E; 7 behind D."""
    links = []
    for r_ in (1, 2, 3, 4):
        links += [(r_, 0, 10), (0, r_, 0)]
    links += M.both([(1, 5, 10), (2, 6, 1), (3, 6, 5), (4, 6, 5), (5, 6, 5), (6, 7, 1)])
    return M.csr(8, links, net=[0])


def ring8(no_transit=()):
    return M.csr(8, M.both([(v, (v + 1) % 8, 1) for v in range(8)]), no_transit=no_transit)


def with_island(graph, n_island=5):
    """The graph plus a ring of `n_island` vertices nothing leads to."""
    rp, col, met, vf = graph
    n = len(vf)
    links = [(u, int(col[k]), int(met[k])) for u in range(n) for k in range(rp[u], rp[u + 1])]
    links += M.both([(n + i, n + (i + 1) % n_island, 1) for i in range(n_island)])
    g = M.csr(n + n_island, links)
    g[3][:n] = vf
    return g


class Case:
    """The model's side of one protected root with [root] + its neighbour routers as the rows (no device involved)."""

    def __init__(self, graph, root, maxp=0xFFFFFFFF, run_flags=0, w_min=1):
        from oracle import graph_oracle as go
        self.graph, self.root, self.maxp, self.run_flags = graph, root, maxp, run_flags
        rp, col, met, vf = graph
        self.cand, self.roots, self.nbr_row = M.protect_one(rp, col, met, vf, root)
        self.W = max(go.mask_words(rp, col, met, vf, self.roots), (len(self.cand.nbr) + 63) // 64, w_min)
        self.fwd, self.rdist = R.tables(graph, maxp, self.roots, run_flags, self.W)

    def lfa(self, lfa_flags=0):
        return M.lfa(self.fwd.dist, self.fwd.flags, self.fwd.mask, self.cand, 0, self.nbr_row, lfa_flags)

    def want(self, lfa_flags=0, with_lfa=True, rdist=None):
        alt = self.lfa(lfa_flags).alt_flags if with_lfa else None
        return R.rlfa(self.fwd.dist, self.fwd.flags, self.fwd.mask, self.rdist if rdist is None else rdist, self.graph[3], self.cand, 0,
                      self.nbr_row, lfa_flags, alt)


class Tables:
    """The rows of `roots` on the device from the engine: the forward set from the uploaded graph, rdist from the upload of the
    product's transpose of it."""

    def __init__(self, ctx, graph, maxp, roots, run_flags, W):
        import torch
        from holo_amd import engine as E
        rp, col, met, vf = graph
        dev = torch.device("cuda:0")
        self.n, self.R, self.W = len(vf), len(roots), W
        self.G = ctx.upload(rp, col, met, vf, maxp)
        self.GT = None
        try:
            assert self.G.mask_words(roots) <= W
            self.dist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
            self.flags = torch.empty((self.R, self.n), dtype=torch.int16, device=dev)
            self.mask = torch.empty((self.R, self.n, W), dtype=torch.int64, device=dev)
            self.rdist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
            ctx.run_device(self.G, roots, run_flags, dist_ptr=self.dist.data_ptr(), flags_ptr=self.flags.data_ptr(), mask_ptr=self.mask.data_ptr(),
                           mask_words=W)
            self.GT = ctx.upload(*E.csr_transpose(rp, col, met, vf), vf, maxp)
            ctx.run_device(self.GT, roots, run_flags, dist_ptr=self.rdist.data_ptr())
        except BaseException:
            self.free()
            raise

    def free(self):
        self.G.free()
        if self.GT is not None:
            self.GT.free()


def run_rlfa(ctx, tab, protect, lfa_flags=0, spaces=True, alt_flags=None, rdist=None):
    """protect: [(root_row, product candidates, nbr_row)]; alt_flags: [P, n] u8 host array or None.  Returns {field: host array}
    ([P, S] ..., the space tables None when skipped)."""
    import torch
    dev = torch.device("cuda:0")
    P, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, 7, dtype=dt, device=dev)      # noqa: E731
    t = dict(pq_node=full((P, S), torch.int32), pq_via=full((P, S), torch.int32), pq_metric=full((P, S), torch.int32),
             pq_counts=full((P, S, 4), torch.int32), space_flags=full((P, S, n), torch.uint8) if spaces else None,
             space_via=full((P, S, n), torch.int32) if spaces else None, rl_node=full((P, n), torch.int32), rl_via=full((P, n), torch.int32),
             rl_coverage=full((P, 4), torch.int32))
    alt = torch.from_numpy(np.ascontiguousarray(alt_flags)).to(dev) if alt_flags is not None else None
    ptr = lambda x: 0 if x is None else x.data_ptr()      # noqa: E731
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.rlfa_device(tab.G, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(),
                    (tab.rdist if rdist is None else rdist).data_ptr(), protect, pq_node_ptr=ptr(t["pq_node"]), pq_via_ptr=ptr(t["pq_via"]),
                    pq_metric_ptr=ptr(t["pq_metric"]), pq_counts_ptr=ptr(t["pq_counts"]), rl_node_ptr=ptr(t["rl_node"]), rl_via_ptr=ptr(t["rl_via"]),
                    rl_coverage_ptr=ptr(t["rl_coverage"]), space_flags_ptr=ptr(t["space_flags"]), space_via_ptr=ptr(t["space_via"]),
                    alt_flags_in_ptr=ptr(alt), lfa_flags=lfa_flags)
    return {k: None if x is None else x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in t.items()}


def assert_equal(got, want, i=0, spaces=True, tag=""):
    for name in R.FIELDS:
        if not spaces and name.startswith("space_"):
            assert got[name] is None
            continue
        g, w = got[name][i], getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:8].tolist())


def check_one(ctx, case, lfa_flags=(0,), need=None, need_exact_row=False, with_lfa=True):
    """One protected root on the device against the model, for every lfa_flags; returns the model's result of the first."""
    from holo_amd import engine as E
    pc = E.lfa_candidates(*case.graph, case.root)
    for a, b in ((pc.nbr, case.cand.nbr), (pc.cost, case.cand.cost), (pc.root_link, case.cand.root_link), (pc.cflags, case.cand.cflags)):
        assert np.array_equal(a, b)
    wants = [case.want(lf, with_lfa) for lf in lfa_flags]
    if need is not None:
        need(wants[0])                                       # non-vacuity: a condition on the MODEL, before anything is compared
    tab = Tables(ctx, case.graph, case.maxp, case.roots, case.run_flags, case.W)
    try:
        if need_exact_row:                                   # a row of the table set comes from the dynamic-pop-order path (HSPF_RF_EXACT)
            assert ((tab.flags.cpu().numpy().view(np.uint16) & 2) != 0).any(axis=1).any()
        assert np.array_equal(tab.rdist.cpu().numpy().view(np.uint32), case.rdist)      # the reverse run itself
        for lf, want in zip(lfa_flags, wants):
            alt = case.lfa(lf).alt_flags[None, :] if with_lfa else None
            assert_equal(run_rlfa(ctx, tab, [(0, pc, case.nbr_row)], lf, alt_flags=alt), want, tag=lf)
    finally:
        tab.free()
    return wants[0]


def cand_slots(case):
    return np.flatnonzero(case.cand.nbr != M.NONE)


def every_class(case):
    def need(want):
        ks = cand_slots(case)
        via = want.pq_via[ks]
        assert (via == R.VIA_SELF).any(), "no PQ node released by the root itself"
        assert ((via != R.VIA_SELF) & (via != R.NONE)).any(), "no PQ node released by a neighbour"
        assert (want.pq_node[ks] == R.NONE).any(), "no slot without a PQ node"
        assert want.rl_coverage[2] > 0 and want.rl_coverage[3] > 0, want.rl_coverage
    return need


@both_engines
@pytest.mark.parametrize("n", [255, 256, 257])
def test_rings_with_chords_at_the_tile_edge(spf_ctx, n):
    case = Case(ring_chords(n, RINGS[n][0]), RINGS[n][1])
    check_one(spf_ctx, case, need=every_class(case))


@both_engines
@pytest.mark.parametrize("k", [7, 8, 9, 17, 63, 64, 65, 128])
def test_hub_root_chunk_edge_and_mask_words(spf_ctx, k):
    case = Case(hub(k, HUB_SEEDS[k]), 0)

    def need(want):
        assert len(cand_slots(case)) == k and case.W == (1 if k <= 64 else 2)
        via = want.pq_via[:k]
        assert ((via != R.VIA_SELF) & (via != R.NONE)).any() and want.pq_counts[:k, 3].any()
        if k > 8:
            assert (via[8:] != R.NONE).any()                 # a PQ node beyond the first chunk
        if k > 64:
            assert ((via >= 64) & (via < k)).any()           # a via-slot of the second mask word
    check_one(spf_ctx, case, need=need)


@both_engines
@pytest.mark.parametrize("run_flags", [0, 1])                # HSPF_RUN_NET_NEXTHOPS off / on
def test_lan_slots_behind_the_primarys_pseudonode(spf_ctx, run_flags):
    case = Case(lan(), 1, run_flags=run_flags)
    c = case.cand
    e, k_c = (int(np.flatnonzero(c.nbr == v)[0]) for v in (2, 5))
    behind = [int(np.flatnonzero(c.nbr == v)[0]) for v in (3, 4)]

    def need(want):
        assert c.root_link[e] == c.root_link[behind[0]] == c.root_link[behind[1]] != c.root_link[k_c]
        assert want.pq_node[e] != R.NONE and want.pq_node[k_c] != R.NONE
        assert not np.isin(want.space_via[e], behind).any()                  # never a via: they share the protected first link
        assert not (want.space_flags[:, 0] & R.ELIGIBLE).any() and (want.pq_node != 0).all()      # the pseudonode is no PQ node
    check_one(spf_ctx, case, need=need)
    check_one(spf_ctx, case, with_lfa=False)


@both_engines
def test_asymmetric_costs_need_the_reverse_tables(spf_ctx):
    case = Case(ring_chords(40, ASYM_SEED, 1, 30, chords=4, asym=True), 0)
    true, wrong = case.want(), case.want(rdist=case.fwd.dist)
    ks = cand_slots(case)
    assert (true.pq_node[ks] != wrong.pq_node[ks]).any() and (true.pq_node[ks] != R.NONE).any()      # on the MODEL
    check_one(spf_ctx, case)
    # and the device, handed the forward table as rdist, gives the other answer too: the argument is really read
    from holo_amd import engine as E
    tab = Tables(spf_ctx, case.graph, case.maxp, case.roots, 0, case.W)
    try:
        got = run_rlfa(spf_ctx, tab, [(0, E.lfa_candidates(*case.graph, 0), case.nbr_row)], alt_flags=case.lfa().alt_flags[None, :], rdist=tab.dist)
        assert_equal(got, wrong)
    finally:
        tab.free()


@both_engines
def test_overloaded_pq_candidate_with_and_without_ignore(spf_ctx):
    case = Case(ring8(no_transit=[4]), 0)
    e = int(np.flatnonzero(case.cand.nbr == 1)[0])
    assert case.want(0).pq_node[e] == R.NONE and case.want(M.IGNORE_OVERLOAD).pq_node[e] == 4
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD))


@both_engines
def test_overloaded_via_neighbour_with_and_without_ignore(spf_ctx):
    case = Case(ring8(no_transit=[7]), 0)
    e, k7 = (int(np.flatnonzero(case.cand.nbr == v)[0]) for v in (1, 7))
    assert case.want(0).pq_counts[e, 1] == 0 and case.want(M.IGNORE_OVERLOAD).pq_via[e] == k7
    check_one(spf_ctx, case, lfa_flags=(0, M.IGNORE_OVERLOAD))


@both_engines
def test_unreachable_island_is_in_no_set(spf_ctx):
    case = Case(with_island(ring_chords(100, 3)), 44)
    want = check_one(spf_ctx, case)
    assert not want.space_flags[:, 100:].any() and (want.space_via[:, 100:] == R.NONE).all() and (want.rl_node[100:] == R.NONE).all()
    assert (want.pq_node != R.NONE).any()


@both_engines
def test_pruned_vertices_are_in_no_set(spf_ctx):
    case = Case(ring_chords(120, PRUNE_SEED, 1, 400), 7, maxp=1023)

    def need(want):
        pruned = case.fwd.dist[0] == R.INF
        assert pruned.any() and not pruned.all()
        assert not want.space_flags[:, pruned].any()
        assert (case.fwd.dist[1:][:, pruned] != R.INF).any()                 # a neighbour still reaches some of them: eligibility cut them
        assert (want.pq_node != R.NONE).any()
    check_one(spf_ctx, case, need=need)


@both_engines
def test_wide_metrics_sums_beyond_32_bits(spf_ctx):
    case = Case(ring_chords(14, WIDE_SEED, 0x7E000000, 0x7F000000, chords=3), 0, maxp=WIDE)

    def need(want):
        ks = cand_slots(case)
        d = case.fwd.dist[case.nbr_row[ks]].astype(np.uint64)
        d = np.where(d == R.INF, 0, d) + case.cand.cost[ks].astype(np.uint64)[:, None]
        assert (d > 0xFFFFFFFF).any()                                        # c + d(E, v) does not fit 32 bits
        assert (want.pq_metric >= 0x7FFFFFFF).any() and (want.pq_node[ks] != R.NONE).any()
    check_one(spf_ctx, case, need=need)


@both_engines
def test_zero_cost_links(spf_ctx):
    case = Case(ring_chords(300, 8, 1, 6, chords=300, zero_share=0.01), 17)
    want = check_one(spf_ctx, case, need_exact_row=True)
    assert (want.pq_node != R.NONE).any()


@both_engines
@pytest.mark.parametrize("spaces", [True, False])
@pytest.mark.parametrize("with_alt", [True, False])
def test_eight_protected_roots_share_one_64_row_table(spf_ctx, spaces, with_alt):
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph = ring_chords(300, 31, chords=210)
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
    fwd, rdist = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
    protect, wants, alts = [], [], []
    for r in prot_roots:
        mc = M.candidates(*graph, r)
        nbr_row = np.array([row_of.get(int(x), 0) for x in mc.nbr], np.uint32)
        protect.append((row_of[r], E.lfa_candidates(*graph, r), nbr_row))
        alts.append(M.lfa(fwd.dist, fwd.flags, fwd.mask, mc, row_of[r], nbr_row).alt_flags)
        wants.append(R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], mc, row_of[r], nbr_row, 0, alts[-1] if with_alt else None))
    assert sum(int(w.rl_coverage[2]) for w in wants) > 0
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        got = run_rlfa(spf_ctx, tab, protect, 0, spaces, np.stack(alts) if with_alt else None)
        for i, w in enumerate(wants):
            assert_equal(got, w, i, spaces, tag=i)
    finally:
        tab.free()


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import ctypes
    import torch
    case = Case(ring_chords(30, 1, chords=4), 8)
    n, S = 30, 64
    tab = Tables(spf_ctx, case.graph, case.maxp, case.roots, 0, 1)
    try:
        pc = E.lfa_candidates(*case.graph, 8)
        good = run_rlfa(spf_ctx, tab, [(0, pc, case.nbr_row)])
        sizes = dict(pq_node=S * 4, pq_via=S * 4, pq_metric=S * 4, pq_counts=S * 16, rl_node=n * 4, rl_via=n * 4, rl_coverage=16)
        out = torch.full((sum(sizes.values()),), 0x5A, dtype=torch.uint8, device="cuda:0")
        ptrs, off = {}, 0
        for k, b in sizes.items():
            ptrs[k + "_ptr"] = out.data_ptr() + off
            off += b

        def expect_inval(protect=None, **kw):
            tables = dict(dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr(), rdist=tab.rdist.data_ptr())
            p = dict(ptrs)
            for k, v in kw.items():
                (tables if k in tables else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.rlfa_device(tab.G, tab.R, 1, tables["dist"], tables["flags"], tables["mask"], tables["rdist"],
                                    protect or [(0, pc, case.nbr_row)], **p)
            assert e.value.code == -1 and "hspf_rlfa_device" in str(e.value)
            assert (out.cpu().numpy() == 0x5A).all()         # nothing was written: nothing was launched

        expect_inval(dist=0)                                 # NULL required pointers: the tables ...
        expect_inval(rdist=0)
        expect_inval(pq_node_ptr=0)                          # ... and the outputs
        expect_inval(pq_counts_ptr=0)
        expect_inval(rl_coverage_ptr=0)
        bad_row = case.nbr_row.copy()
        bad_row[np.flatnonzero(case.cand.nbr != M.NONE)[0]] = tab.R
        expect_inval(protect=[(0, pc, bad_row)])             # nbr_row >= n_rows
        expect_inval(protect=[(tab.R, pc, case.nbr_row)])    # root_row out of range
        many = E.LfaCandidates(8, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        expect_inval(protect=[(0, many, np.zeros(65, np.uint32))])      # n_slots > 64 * n_mask_words
        lib = L.load()
        arr, keep = spf_ctx._protect_array([(0, pc, case.nbr_row)], "test")
        o = L.HspfRlfaOut(*(ptrs[k + "_ptr"] for k in ("pq_node", "pq_via", "pq_metric", "pq_counts")), None, None,
                          *(ptrs[k + "_ptr"] for k in ("rl_node", "rl_via", "rl_coverage")))
        other = spf_ctx.upload(*ring8(), 0xFFFFFFFF)         # a graph of another size than n_vertices
        try:
            assert lib.hspf_rlfa_device(spf_ctx.handle, other.handle, n, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(),
                                        tab.rdist.data_ptr(), arr, 1, 0, None, ctypes.byref(o)) == -1
            assert "hspf_rlfa_device" in spf_ctx.last_error() and (out.cpu().numpy() == 0x5A).all()
        finally:
            other.free()
        # the raw call with NULL graph / prot / out
        assert lib.hspf_rlfa_device(spf_ctx.handle, None, n, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr(),
                                    None, 1, 0, None, None) == -1
        assert lib.hspf_rlfa_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(),
                                    tab.rdist.data_ptr(), None, 1, 0, None, ctypes.byref(L.HspfRlfaOut())) == -1
        # and the context still works
        again = run_rlfa(spf_ctx, tab, [(0, pc, case.nbr_row)])
        assert all(np.array_equal(good[k], again[k]) for k in good)
        assert_equal(again, case.want(with_lfa=False))
    finally:
        tab.free()


def test_rlfa_convenience_end_to_end(spf_ctx):
    """SpfContext.rlfa(): candidates, the forward and the transposed run, lfa_device, rlfa_device, results on the host; and
    symmetric=True — no transposed run — gives the same on a graph whose costs are symmetric."""
    n = 256
    case = Case(ring_chords(n, RINGS[n][0]), n - 2)
    want_lfa, want = case.lfa(), case.want()
    G = spf_ctx.upload(*case.graph, 0xFFFFFFFF)
    try:
        cand, lfa, res = spf_ctx.rlfa(G, n - 2, want_spaces=True)
        cand2, lfa2, res2 = spf_ctx.rlfa(G, n - 2, want_spaces=True, symmetric=True)
    finally:
        G.free()
    assert np.array_equal(cand.nbr, case.cand.nbr)
    assert np.array_equal(lfa.alt_flags[0], want_lfa.alt_flags) and np.array_equal(lfa.alt_slot[0], want_lfa.alt_slot)
    assert np.array_equal(lfa.coverage[0], want_lfa.coverage)
    for name in R.FIELDS:
        assert np.array_equal(getattr(res, name)[0], getattr(want, name)), name
        assert np.array_equal(getattr(res2, name), getattr(res, name)), name
