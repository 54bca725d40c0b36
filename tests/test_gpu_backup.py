"""hspf_routes_backup_device on the GPU against the plain-Python model (tests/_backup_model.py) over the CPU oracle's SPTs: every
output array and the coverage, bit for bit.  The tables the kernel reads are the engine's own — hspf_run_device for the rows,
hspf_routes_device for the routes (compared with the model's first); the per-slot repairs it falls back on are the TI-LFA
MODEL's, uploaded (tests/test_gpu_tilfa.py checks the call that writes them; the end-to-end test below runs the whole chain on
the device).  Each case is the smallest shape at which one thing can go wrong: the 256-prefix tile edge, the 8-slot chunk edge,
one / two mask words, empty, long, unreachable and local advertiser lists, the table flags, several protected roots."""
import ctypes

import numpy as np
import pytest

import _backup_cases as C
import _backup_model as B
import _lfa_model as M
from test_gpu_rlfa import Tables, hub, lan, with_island

pytestmark = pytest.mark.gpu

WIDE = 0xFE000000
HUB_SEEDS = {7: 3, 8: 3, 9: 0, 17: 3, 65: 3}      # k: seed of tests/test_gpu_rlfa.py's hub on which the MODEL makes the last slot a candidate
OUT = dict(bk_kind=np.uint8, bk_primary=np.uint32, bk_slot=np.uint32, bk_metric=np.uint32, bk_flags=np.uint8, bk_cand_mask=np.uint64,
           bk_node_mask=np.uint64, bk_coverage=np.uint32)


def _torch_dt(dt):
    import torch
    return {np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64}[dt]


def protect_of(model):
    from holo_amd import engine as E
    out = []
    for r, mc, rr, nr in zip(model.prot, model.cands, model.root_row, model.nbr_row):
        pc = E.lfa_candidates(*model.graph, r)
        for a, b in ((pc.nbr, mc.nbr), (pc.cost, mc.cost), (pc.root_link, mc.root_link), (pc.cflags, mc.cflags)):
            assert np.array_equal(a, b)
        out.append((rr, pc, nr))
    return out


class Device:
    """The rows of the model's roots on the device, from the engine."""

    def __init__(self, ctx, model):
        self.ctx, self.model = ctx, model
        self.tab = Tables(ctx, model.graph, model.maxp, model.roots, model.run_flags, model.W)
        self.protect = protect_of(model)

    def free(self):
        self.tab.free()

    def routes(self, t: B.Table, flags=None, arrays=None):
        """hspf_routes_device for every row; {name: device tensor}, checked against the model for the protected roots."""
        import torch
        tab, NP = self.tab, t.n
        r = dict(best_metric=torch.full((tab.R, NP), 7, dtype=torch.int32, device="cuda:0"), best_entry=torch.full((tab.R, NP), 7, dtype=torch.int32, device="cuda:0"),
                 nexthop_mask=torch.full((tab.R, NP, tab.W), 7, dtype=torch.int64, device="cuda:0"))
        a = arrays or (t.ptr, t.vertex, t.metric)
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        self.ctx.routes_device(tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), *a, flags=t.flags if flags is None else flags,
                               **{k + "_ptr": x.data_ptr() for k, x in r.items()})
        for i, rr in enumerate(self.model.root_row):
            w = self.model.routes(i, t)
            for k, x in r.items():
                assert np.array_equal(x[rr].cpu().numpy().view(getattr(w, k).dtype), getattr(w, k)), ("routes", i, k)
        return r

    def backup(self, t: B.Table, lfa_flags=0, remote=True, masks=True, flags=None, routes=None, arrays=None, protect=None):
        """routes_device, then routes_backup_device; {field: host array [n_prot, ...]} (the masks None when skipped)."""
        import torch
        tab, P, NP = self.tab, len(self.model.prot), t.n
        r = routes or self.routes(t, None if flags is None else flags & ~B.PFX_RESIDENT, arrays)
        shapes = dict(bk_kind=(P, NP), bk_primary=(P, NP), bk_slot=(P, NP), bk_metric=(P, NP), bk_flags=(P, NP), bk_cand_mask=(P, NP, tab.W),
                      bk_node_mask=(P, NP, tab.W), bk_coverage=(P, 7))
        out = {k: torch.full(sh, 7, dtype=_torch_dt(OUT[k]), device="cuda:0") for k, sh in shapes.items() if masks or not k.endswith("_mask")}
        ti = None
        if remote:
            S = 64 * tab.W
            tm = [f[2] for f in self.model.frr(lfa_flags)]
            ti = [torch.from_numpy(np.stack([getattr(x, k) for x in tm]).view(np.uint8 if k == "ti_kind" else np.int32)).to("cuda:0") for k in ("ti_kind", "ti_via", "ti_metric")]
            assert ti[0].shape == (P, S)
        a = arrays or (t.ptr, t.vertex, t.metric)
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        self.ctx.routes_backup_device(tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect or self.protect, *a,
                                      routes=tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")),
                                      tilfa=None if ti is None else tuple(x.data_ptr() for x in ti), flags=t.flags if flags is None else flags, lfa_flags=lfa_flags,
                                      **{k + "_ptr": x.data_ptr() for k, x in out.items()})
        return {k: (out[k].cpu().numpy().view(OUT[k]) if k in out else None) for k in shapes}


def assert_equal(got, wants, masks=True, tag=""):
    for i, w in enumerate(wants):
        for name in B.FIELDS:
            if not masks and name.endswith("_mask"):
                assert got[name] is None
                continue
            g, x = got[name][i], getattr(w, name)
            assert g.shape == x.shape and g.dtype == x.dtype and np.array_equal(g, x), (tag, i, name, np.argwhere(g != x)[:8].tolist(), g[g != x][:8], x[g != x][:8])


def check(ctx, model, lfa_flags=(0,), remotes=(True, False), need=None):
    """The model's protected roots and table on the device, for every lfa_flags with and without the repairs."""
    if need is not None:
        need(model.want(lfa_flags[0], remotes[0]))              # non-vacuity: on the MODEL, before anything is compared
    d = Device(ctx, model)
    try:
        r = d.routes(model.table)
        for lf in lfa_flags:
            for rem in remotes:
                assert_equal(d.backup(model.table, lf, rem, routes=r), model.want(lf, rem), tag=(lf, rem))
    finally:
        d.free()


def kinds_of(wants):
    return {int(k) for w in wants for k in w.bk_kind}


def random_table(r, nr, n_pfx, lo=1, hi=16):
    return B.table([[(int(v), int(r.integers(lo, hi))) for v in r.choice(nr, size=int(r.choice([1, 2, 2, 3])), replace=False)] for _ in range(n_pfx)])


def test_the_hand_checked_cases(spf_ctx):
    for case in (C.square, C.five_ring, C.triangle):
        g, S, t = case()
        check(spf_ctx, C.Model(g, [S], t), lfa_flags=(0, M.IGNORE_OVERLOAD))


@pytest.mark.parametrize("n_pfx", [1, 63, 64, 65, 257])
def test_prefix_counts_at_the_tile_edge(spf_ctx, n_pfx):
    r = np.random.default_rng(100 + n_pfx)
    g = M.csr(12, M.both([(v, (v + 1) % 12, int(r.integers(1, 9))) for v in range(12)] + [(0, 5, 4), (2, 9, 3), (3, 7, 6)]))
    model = C.Model(g, [4], random_table(r, 12, n_pfx))

    def need(w):
        assert n_pfx < 63 or {B.LFA, B.LOCAL} <= kinds_of(w)
    check(spf_ctx, model, need=need)
    assert model.want()[0].bk_kind[-1] != B.NO_ROUTE                     # the last lane of the last tile has something to say


@pytest.mark.parametrize("k", [7, 8, 9, 17, 65])
def test_hub_root_chunk_edge_and_mask_words(spf_ctx, k):
    """A root with k candidate slots (chunks of 8; 65: two mask words, the last slot and its root_link in the second)."""
    r = np.random.default_rng(200 + k)
    model = C.Model(hub(k, HUB_SEEDS[k]), [0], random_table(r, k + 1, 48))

    def need(w):
        assert len(model.cands[0].nbr) == k and (model.cands[0].nbr != M.NONE).all() and model.W == (k + 63) // 64
        assert (w[0].bk_cand_mask[:, -1] & np.uint64(1 << ((k - 1) % 64))).any(), "the last slot is never a candidate"
        assert B.LFA in kinds_of(w)
    check(spf_ctx, model, need=need)


def advertiser_lists():
    """A 40-router mesh (seed chosen on the CPU) plus an island of five routers nothing leads to; S = 3."""
    r = np.random.default_rng(5)
    und = {(v, int(r.integers(0, v))) for v in range(1, 40)} | {(int(a), int(b)) for a, b in r.integers(0, 40, (30, 2)) if a > b}
    g = with_island(M.csr(40, M.both([(a, b, int(r.integers(1, 9))) for a, b in sorted(und)])))
    S = 3
    d = C.Model(g, [S], B.table([])).fwd.dist[0]
    better = int(np.argmin(np.where(np.arange(45) == S, M.INF, d)))             # the router nearest to S
    lists = [[], [(17, 4)], [(v, 1 + (v * 7) % 13) for v in range(4, 37)], [(40, 1), (42, 2), (44, 3)], [(S, 5)],
             [(S, int(d[better]) + 9), (better, 2)], [(S, 1), (better, 2)]]
    return g, S, B.table(lists)


def test_advertiser_lists_empty_long_unreachable_and_local(spf_ctx):
    g, S, t = advertiser_lists()
    model = C.Model(g, [S], t)

    def need(w):
        k, ptr = w[0].bk_kind, np.diff(t.ptr)
        assert ptr.tolist()[:5] == [0, 1, 33, 3, 1]
        assert k[0] == B.NO_ROUTE and k[3] == B.NO_ROUTE and k[4] == B.LOCAL and k[6] == B.LOCAL
        assert k[5] >= B.ECMP and t.vertex[model.routes().best_entry[5]] != S    # advertised by S and, better, by another router
        assert k[1] >= B.ECMP and k[2] >= B.ECMP
    check(spf_ctx, model, need=need)


def saturating_case():
    """A four-ring with costs of 0x7F000000 under max_path_metric 0xFE000000; S = 0, the far router 2 at 0xFE000000 both ways round.
    Prefix 0: every term saturates (a tie at 0xFFFFFFFF over both first hops); prefix 1: only the far advertiser's does; prefix 2:
    0x7F000000 + 0x80FFFFFF = 0xFFFFFFFF exactly against a saturated term — equal only with HSPF_PFX_SATURATING; 3: small metrics."""
    c = 0x7F000000
    g = M.csr(4, M.both([(0, 1, c), (1, 2, c), (2, 3, c), (3, 0, c)]))
    return g, 0, [[(1, 0x90000000), (3, 0x90000000)], [(1, 0x10000000), (2, 0x20000000)], [(1, 0x80FFFFFF), (2, 0x05000000)], [(2, 1), (3, 5)]]


@pytest.mark.parametrize("flags", [0, B.PFX_SATURATING])
def test_metrics_that_saturate_and_sums_beyond_32_bits(spf_ctx, flags):
    g, S, lists = saturating_case()
    model = C.Model(g, [S], B.table(lists, flags), maxp=WIDE)

    def need(w):
        r = model.routes()
        if flags:
            assert r.best_metric[0] == 0xFFFFFFFF and w[0].bk_kind[0] == B.ECMP and r.best_metric[2] == 0xFFFFFFFF
            assert bin(int(r.nexthop_mask[2, 0])).count("1") == 2                  # the tie at the saturated value merges both entries
        else:
            assert r.best_metric[0] == (0x7F000000 + 0x90000000) & 0xFFFFFFFF     # the plain add of hspf_routes_device wraps
    check(spf_ctx, model, need=need)


def last_min_case():
    """The LAN of tests/test_gpu_rlfa.py (S = 1 on pseudonode 0) plus pseudonode 8 between routers 6 and 7 and pseudonode 9 between
    routers 5 and 7: d(1, 8) = 14 through the LAN's router 2, d(1, 9) = 14 through the p2p link to router 5.  Prefix 0 sits on both
    at metric 0: a tie whose two entries have different first hops."""
    rp, col, met, vf = lan()
    links = [(u, int(col[k]), int(met[k])) for u in range(8) for k in range(rp[u], rp[u + 1])]
    links += [(6, 8, 3), (8, 6, 0), (7, 8, 3), (8, 7, 0), (5, 9, 4), (9, 5, 0), (7, 9, 4), (9, 7, 0)]
    return M.csr(10, links, net=[0, 8, 9]), 1, [[(8, 0), (9, 0)], [(0, 6), (8, 0)], [(9, 0)], [(0, 0)], [(8, 2), (9, 0)]]


def test_last_min_on_network_vertex_prefixes(spf_ctx):
    """Network-LSA prefixes: HSPF_PFX_LAST_MIN keeps the later entry's mask alone where hspf_routes_device would merge a tie — one
    primary instead of ECMP — and the mask is read as given; d_X(p) is the same with and without the flag."""
    g, S, lists = last_min_case()
    wants = {}
    for flags in (B.PFX_LAST_MIN | B.PFX_SATURATING, B.PFX_SATURATING, B.PFX_LAST_MIN):
        model = C.Model(g, [S], B.table(lists, flags))
        wants[flags] = model.want()[0]
        check(spf_ctx, model)
    last, merged = wants[B.PFX_LAST_MIN | B.PFX_SATURATING], wants[B.PFX_SATURATING]
    assert merged.bk_kind[0] == B.ECMP and last.bk_kind[0] >= B.LFA and np.array_equal(last.bk_kind[1:], merged.bk_kind[1:])


def test_resident_table_then_a_changed_one(spf_ctx):
    r = np.random.default_rng(9)
    g, S, _ = C.sweep_case(C.SWEEP_SEED + 3)
    nr = int((g[3] & M.VF_NETWORK == 0).sum())
    t1, t2 = random_table(r, nr, 70), random_table(r, nr, 70)
    model = C.Model(g, [S], t1)
    d = Device(spf_ctx, model)
    try:
        first = d.backup(t1)
        assert_equal(first, model.want(table=t1), tag="uploaded")
        again = d.backup(t1, flags=B.PFX_RESIDENT)                                  # the same arrays, held by the context
        assert all(np.array_equal(first[k], again[k]) for k in first)
        r1 = d.routes(t1)
        assert len(t2.vertex) != len(t1.vertex) or not np.array_equal(t2.vertex, t1.vertex)
        assert_equal(d.backup(t2), model.want(table=t2), tag="changed, uploaded")   # another table without the flag
        r2 = d.routes(t2)
        assert_equal(d.backup(t1, routes=r1), model.want(table=t1), tag="back: the backup call itself uploads")
        # the flag on arrays the context does not hold (it holds t1's): uploaded as usual
        assert_equal(d.backup(t2, flags=B.PFX_RESIDENT, routes=r2), model.want(table=t2), tag="resident flag, other arrays")
    finally:
        d.free()


def test_three_protected_roots_share_one_table_set(spf_ctx):
    g, S, t = C.sweep_case(C.SWEEP_SEED + 8)
    nbrs = [int(x) for x in M.candidates(*g, S).nbr if x != M.NONE]
    model = C.Model(g, [nbrs[0], S, nbrs[-1]], t)

    def need(w):
        assert model.root_row == [0, 1, 2] and len({tuple(x.bk_kind.tolist()) for x in w}) == 3
    check(spf_ctx, model, lfa_flags=(0, M.IGNORE_OVERLOAD), need=need)


def test_without_repairs_kinds_4_and_5_become_6_and_without_masks_nothing_else_changes(spf_ctx):
    g, S, t = C.five_ring()
    model = C.Model(g, [S], t)
    d = Device(spf_ctx, model)
    try:
        full, local, bare = d.backup(t), d.backup(t, remote=False), d.backup(t, masks=False)
    finally:
        d.free()
    assert_equal(full, model.want())
    assert_equal(local, model.want(0, False))
    assert_equal(bare, model.want(), masks=False)
    remote = np.isin(full["bk_kind"], (B.NODE, B.PAIR))
    assert remote.any() and (local["bk_kind"][remote] == B.NOTHING).all() and np.array_equal(local["bk_kind"][~remote], full["bk_kind"][~remote])
    for f in ("bk_primary", "bk_flags", "bk_cand_mask", "bk_node_mask"):
        assert np.array_equal(full[f], local[f]), f
    assert all(np.array_equal(full[f], bare[f]) for f in B.FIELDS if not f.endswith("_mask"))


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import torch
    g, S, t = C.square()
    model = C.Model(g, [S], t)
    d = Device(spf_ctx, model)
    try:
        tab, pc, nr = d.tab, d.protect[0][1], model.nbr_row[0]
        r = d.routes(t)
        good = d.backup(t, remote=False, routes=r)
        sizes = dict(bk_kind=2, bk_primary=8, bk_slot=8, bk_metric=8, bk_flags=2, bk_cand_mask=16, bk_node_mask=16, bk_coverage=28)
        out = torch.full((sum(sizes.values()) + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        ptrs, off = {}, 0
        for k, b in sizes.items():
            ptrs[k + "_ptr"] = out.data_ptr() + off
            off += (b + 7) // 8 * 8

        def expect_inval(protect=None, table=None, tflags=0, routes=None, tilfa=None, **kw):
            tables = dict(dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr())
            p = dict(ptrs)
            for k, v in kw.items():
                (tables if k in tables else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.routes_backup_device(tab.n, tab.R, 1, tables["dist"], tables["flags"], tables["mask"], protect or d.protect,
                                             *(table or (t.ptr, t.vertex, t.metric)), flags=tflags, tilfa=tilfa,
                                             routes=routes or tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")), **p)
            assert e.value.code == -1 and "hspf_routes_backup_device" in str(e.value), str(e.value)
            assert (out.cpu().numpy() == 0x5A).all()         # nothing was written: nothing was launched

        for k in ("dist", "flags", "mask"):                  # NULL required pointers: the tables ...
            expect_inval(**{k: 0})
        for k in ("bk_kind", "bk_primary", "bk_slot", "bk_metric", "bk_flags", "bk_coverage"):      # ... the outputs ...
            expect_inval(**{k + "_ptr": 0})
        expect_inval(routes=(0, r["best_entry"].data_ptr(), r["nexthop_mask"].data_ptr()))           # ... the routes ...
        expect_inval(routes=(r["best_metric"].data_ptr(), r["best_entry"].data_ptr(), 0))
        expect_inval(tilfa=(0, 8, 8))                        # ... and a repair set without ti_kind
        bad_row = nr.copy()
        bad_row[0] = tab.R
        expect_inval(protect=[(0, pc, bad_row)])             # what hspf_lfa_device rejects in prot
        expect_inval(protect=[(tab.R, pc, nr)])
        many = E.LfaCandidates(0, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        expect_inval(protect=[(0, many, np.zeros(65, np.uint32))])
        expect_inval(tflags=B.PFX_ORDERED)                    # out of scope
        expect_inval(tflags=0x10)                            # what the table checks of hspf_routes_device reject
        expect_inval(table=(np.array([1, 2, 3], np.uint32), t.vertex, t.metric))
        expect_inval(table=(np.array([0, 3, 2, 3], np.uint32), t.vertex, t.metric))
        expect_inval(table=(t.ptr, np.array([1, 2, 4], np.uint32), t.metric))
        lib = L.load()
        assert lib.hspf_routes_backup_device(spf_ctx.handle, tab.n, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(),
                                             None, 1, 0, None, None, None, None) == -1
        assert "hspf_routes_backup_device" in spf_ctx.last_error()
        assert_equal(d.backup(t, remote=False, routes=r), model.want(0, False))      # and the context still works
        assert all(np.array_equal(good[k], v) for k, v in d.backup(t, remote=False, routes=r).items())
    finally:
        d.free()


def test_seeded_sweep(spf_ctx):
    kinds = set()
    for seed in range(C.SWEEP_SEED, C.SWEEP_SEED + C.GPU_GRAPHS):
        g, S, t = C.sweep_case(seed)
        model = C.Model(g, [S], t)
        kinds |= kinds_of(model.want())
        check(spf_ctx, model, remotes=(True,))
    assert kinds == set(range(7)), kinds


def _same_backup(res, w, wr, tag):
    for name in ("best_metric", "best_entry", "nexthop_mask"):
        assert np.array_equal(getattr(res, name)[0], getattr(wr, name)), (tag, name)
    for name in B.FIELDS:
        assert np.array_equal(getattr(res, name)[0], getattr(w, name)), (tag, name)


def test_backup_routes_end_to_end_on_the_five_ring_and_on_a_patched_graph(spf_ctx):
    """SpfContext.backup_routes(): run, routes, lfa, rlfa + tilfa, backup — all on the device.  Then one step of chain (a) of
    tests/_frr_chains.py on the same handle: row 4 gains 4 -> 1 after row 1 gained 1 -> 4, and the single node 4 repairs 2-3."""
    import _frr_chains as F
    g, S, t = C.five_ring()
    model = C.Model(g, [S], t)
    chain = F.chain("a")
    assert all(np.array_equal(x, y) for x, y in zip(chain.steps[0].graph, g)) and chain.steps[0].prot == (S,)
    G = spf_ctx.upload(*g, C.MAXP)
    try:
        for remote in (True, False):
            for symmetric in (False, True):
                res = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), symmetric=symmetric, remote=remote)
                _same_backup(res, model.want(0, remote)[0], model.routes(), (remote, symmetric))
                assert np.array_equal(res.candidates.nbr, model.cands[0].nbr) and (res.tilfa is not None) == remote
        for step in chain.steps[1:3]:
            G.patch(step.patch.vs, step.patch.rows, step.patch.flags)
        patched = C.Model(chain.steps[2].graph, [S], t)
        w = patched.want()[0]
        assert w.bk_kind.tolist() != model.want()[0].bk_kind.tolist() and B.NODE in w.bk_kind
        _same_backup(spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric)), w, patched.routes(), "patched")
    finally:
        G.free()
