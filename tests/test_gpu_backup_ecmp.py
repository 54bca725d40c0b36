"""hspf_routes_backup_ecmp_device on the GPU against the plain-Python model (tests/_backup_ecmp_model.py) over the CPU oracle's SPTs:
eb_ptr, the five entry arrays, the coverage and the total, bit for bit.  The tables the kernel reads are the engine's own —
hspf_run_device for the rows, hspf_routes_device for the routes (compared with the model's first); the per-slot repairs are the
TI-LFA MODEL's, uploaded, as in tests/test_gpu_backup.py.  Each case is the smallest shape at which one thing can go wrong: see the
tests' names."""
import ctypes

import numpy as np
import pytest

import _backup_ecmp_cases as C
import _backup_ecmp_model as BE
import _backup_model as B
import _lfa_model as M
from test_gpu_backup import Device, assert_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0x07070707
WIDE = 0xFE000000


def run_ecmp(d: Device, t: B.Table, lfa_flags=0, remote=True, cap=None, routes=None, protect=None, flags=None):
    """routes_device, then the call.  cap None: the sizing call first, then arrays of that size (three elements more, checked to be
    untouched).  Returns (total, eb_ptr, eb_primary, eb_kind, eb_slot, eb_metric, eb_flags, eb_coverage) on the host."""
    import torch
    tab, model = d.tab, d.model
    protect = protect or d.protect
    P, NP = len(protect), t.n
    r = routes or d.routes(t)
    ti = None
    if remote:
        tm = [f[2] for f in model.frr(lfa_flags)]
        ti = [torch.from_numpy(np.stack([getattr(x, k) for x in tm]).view(np.uint8 if k == "ti_kind" else np.int32)).to("cuda:0") for k in ("ti_kind", "ti_via", "ti_metric")]
    args = (tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect, t.ptr, t.vertex, t.metric)
    kw = dict(routes=tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")), tilfa=None if ti is None else tuple(x.data_ptr() for x in ti),
              flags=t.flags if flags is None else flags, lfa_flags=lfa_flags)
    ptr = torch.full((P * NP + 1,), 7, dtype=torch.int32, device="cuda:0")
    if cap is None:
        cap = d.ctx.routes_backup_ecmp_device(*args, eb_ptr_ptr=ptr.data_ptr(), **kw)
        assert int(ptr[-1].item()) == cap
        ptr.fill_(7)
    pri, slot, met = (torch.full((cap + 3,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(3))
    kind, fl = (torch.full((cap + 3,), 7, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    cov = torch.full((P, BE.COVERAGE_WORDS), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    total = d.ctx.routes_backup_ecmp_device(*args, eb_ptr_ptr=ptr.data_ptr(), cap_entries=cap, eb_primary_ptr=pri.data_ptr(), eb_kind_ptr=kind.data_ptr(),
                                            eb_slot_ptr=slot.data_ptr(), eb_metric_ptr=met.data_ptr(), eb_flags_ptr=fl.data_ptr(), eb_coverage_ptr=cov.data_ptr(), **kw)
    h = lambda x, dt: x.cpu().numpy().view(dt)      # noqa: E731
    for x in (pri, slot, met):
        assert (h(x, np.uint32)[cap:] == SENTINEL).all()                 # nothing is written beyond the capacity
    assert (h(kind, np.uint8)[cap:] == 7).all() and (h(fl, np.uint8)[cap:] == 7).all()
    k = min(total, cap)
    return total, h(ptr, np.uint32), h(pri, np.uint32)[:k], h(kind, np.uint8)[:k], h(slot, np.uint32)[:k], h(met, np.uint32)[:k], h(fl, np.uint8)[:k], h(cov, np.uint32)


def same(got, wants, tag=""):
    want = BE.stack(wants)
    total, ptr, *ent, cov = got
    assert total == want.total, (tag, total, want.total)
    assert np.array_equal(ptr, want.eb_ptr), (tag, np.flatnonzero(ptr != want.eb_ptr)[:8])
    for name, g in zip(BE.FIELDS[1:6], ent):
        w = getattr(want, name)
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
    assert np.array_equal(cov, want.eb_coverage), (tag, cov, want.eb_coverage)


class OracleRows:
    """The rows of the model's roots uploaded from the CPU oracle: for roots with more first-hop slots than hspf_run_device takes
    (1 024), which the call itself accepts — its tables may come from anywhere."""

    def __init__(self, model):
        import torch
        f = model.fwd
        self.n, self.R, self.W = f.dist.shape[1], f.dist.shape[0], f.mask.shape[2]
        self.dist = torch.from_numpy(f.dist.view(np.int32)).to("cuda:0")
        self.flags = torch.from_numpy(f.flags.view(np.int16)).to("cuda:0")
        self.mask = torch.from_numpy(f.mask.view(np.int64)).to("cuda:0")

    def free(self):
        pass


class OracleDevice(Device):
    def __init__(self, ctx, model):
        from test_gpu_backup import protect_of
        self.ctx, self.model = ctx, model
        self.tab = OracleRows(model)
        self.protect = protect_of(model)


def check(ctx, model, lfa_flags=(0,), remotes=(True, False), need=None, device=Device):
    """The model's protected roots and table on the device, for every lfa_flags with and without the repairs."""
    if need is not None:
        need(BE.want(model, lfa_flags[0], remotes[0]))           # non-vacuity: on the MODEL, before anything is compared
    d = device(ctx, model)
    try:
        r = d.routes(model.table)
        for lf in lfa_flags:
            for rem in remotes:
                same(run_ecmp(d, model.table, lf, rem, routes=r), BE.want(model, lf, rem), tag=(lf, rem))
    finally:
        d.free()


def kinds_of(wants):
    return {int(k) for w in wants for k in w.eb_kind}


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_cases(spf_ctx, name):
    """Among them: a prefix that is ECMP only per prefix (two advertisers, each vertex with one primary), a neighbour that is an
    alternate for the prefix and none for S's attaining vertex, two parallel links (the link, not the node), two primaries behind
    one LAN without a repair."""
    case = C.HAND[name]()
    model = C.Model(case[0], [case[1]], case[2])
    for f, w in zip(BE.FIELDS, C.expected(case)):                # the model's arrays are the hand-written ones
        assert np.array_equal(getattr(BE.want(model, case[3], False)[0], f), w), f
    check(spf_ctx, model, lfa_flags=(case[3],))


def test_two_primaries_behind_one_lan_take_the_repair_of_each_primary(spf_ctx):
    g, S, t = C.lan_ring()
    model = C.Model(g, [S], t)

    def need(w):
        ti = model.frr(0)[0][2]
        assert w[0].eb_primary.tolist() == [3, 4] and set(w[0].eb_kind.tolist()) <= {BE.NODE, BE.PAIR}
        assert w[0].eb_slot.tolist() == [int(ti.ti_via[3]), int(ti.ti_via[4])] and w[0].eb_metric.tolist() == [int(ti.ti_metric[3]), int(ti.ti_metric[4])]
        assert w[0].eb_coverage.tolist() == [1, 2, 0, 0, 0, 0, 2, 1]
        assert BE.want(model, 0, False)[0].eb_kind.tolist() == [BE.NOTHING, BE.NOTHING]           # without tilfa_dev
    check(spf_ctx, model, need=need)


def test_a_primary_whose_target_is_a_network_vertex(spf_ctx):
    g, S, t = C.network_primary()
    model = C.Model(g, [S], t, run_flags=0x01)

    def need(w):
        assert model.cands[0].nbr.tolist() == [M.NONE, 1, M.NONE, 1]
        assert w[0].entries(0) == [(0, BE.LFA, 1, 6, BE.DOWNSTREAM | BE.EA_PRIMARY), (1, BE.LFA, 3, 7, BE.DOWNSTREAM)]     # never node-protecting: E is no router
    check(spf_ctx, model, need=need)


def test_an_overloaded_neighbour_whose_own_entry_attains_the_distance(spf_ctx):
    g, S, t = C.overload_own_entry()
    model = C.Model(g, [S], t)
    plain, ign = (BE.want(model, lf, False, sets=True)[0] for lf in (0, M.IGNORE_OVERLOAD))
    assert plain.cand == [{1, 2}, {0, 2}, {1}, {0}] and ign.cand == [{1, 2}, {0, 2}, {1, 2}, {0, 2}]
    check(spf_ctx, model, lfa_flags=(0, M.IGNORE_OVERLOAD))


def test_the_overload_bit_decides_the_choice(spf_ctx):
    """A and B share a LAN, so the overloaded C = 5 behind S's second link is the only candidate of both primaries: taken where its
    own entry attains d_C(p), refused where another advertiser does — unless the call ignores the overload bit."""
    links = [(0, 1, 1), (1, 0, 0), (2, 1, 1), (1, 2, 0), (3, 1, 1), (1, 3, 0)] + M.both([(2, 4, 1), (3, 4, 1), (0, 5, 2), (5, 4, 1), (5, 6, 1)])
    g = M.csr(7, links, net=[1], no_transit=[5])
    # prefix 0: vertex 4 at 3 and C = 5 itself at 4 (d_C(p) = 4 by its own entry and through 4); prefix 1: vertex 4 at 3 and vertex 6 at 1 (d_C(p) = 2 through 6)
    model = C.Model(g, [0], B.table([[(4, 3), (5, 4)], [(4, 3), (6, 1)]]))

    def need(w):
        assert [e[1] for e in w[0].entries(0)] == [BE.LFA, BE.LFA] and [e[1] for e in w[0].entries(1)] == [BE.NOTHING, BE.NOTHING]
        assert [e[1] for e in BE.want(model, M.IGNORE_OVERLOAD, False)[0].entries(1)] == [BE.LFA, BE.LFA]
    check(spf_ctx, model, lfa_flags=(0, M.IGNORE_OVERLOAD), remotes=(False,), need=need)


@pytest.mark.parametrize("flags", [0, B.PFX_SATURATING, B.PFX_SATURATING | B.PFX_LAST_MIN])
def test_terms_that_saturate_and_sums_beyond_32_bits(spf_ctx, flags):
    g, S, lists = C.saturating()
    model = C.Model(g, [S], B.table(lists, flags), maxp=WIDE)

    def need(w):
        if flags == B.PFX_SATURATING:
            assert model.routes().best_metric[0] == 0xFFFFFFFF and w[0].entries(0)[0][1:4] == (BE.LFA, 1, 0xFFFFFFFE)
        if flags == 0:
            assert w[0].eb_ptr.tolist() == [0, 2, 4, 6, 6] and 2399141888 in w[0].eb_metric.tolist()
    check(spf_ctx, model, remotes=(False,), need=need)


@pytest.mark.parametrize("K", [64, 65])
def test_a_root_with_one_and_two_mask_words(spf_ctx, K):
    """65 spokes: W = 2, the r-th-set-bit walk and the primary test cross the word boundary; B = 2048 / K prefixes per batch."""
    g, S, lists = C.spokes(K, 40, 300 + K, far=2, ring=True, far_share=0.4)
    lists.append([(K - 1, 0), (K, 0)])                                    # the last two spokes: each is the other's backup
    model = C.Model(g, [S], B.table(lists))

    def need(w):
        assert model.W == (K + 63) // 64 and w[0].eb_primary.max() == K - 1 and w[0].eb_slot[w[0].eb_kind == BE.LFA].max() == K - 1
        assert np.diff(w[0].eb_ptr.astype(np.int64)).max() == K and w[0].eb_coverage[3] > 0
    check(spf_ctx, model, remotes=(False,), need=need)


def test_more_candidates_than_one_lds_chunk_and_more_primaries_than_one_round(spf_ctx):
    g, S, lists = C.many_slots()
    model = C.Model(g, [S], B.table(lists))

    def need(w):
        cnt = np.diff(w[0].eb_ptr.astype(np.int64)).tolist()
        assert len(model.cands[0].nbr) == 2057 and (model.cands[0].nbr != M.NONE).all() and cnt == [257, 3]
        assert w[0].eb_slot.max() >= 2048 and w[0].eb_coverage[3] > 0 and (w[0].eb_kind == BE.LFA).all()       # a choice out of the second chunk
    check(spf_ctx, model, remotes=(False,), need=need, device=OracleDevice)


def test_two_protected_roots_on_one_table_set(spf_ctx):
    g, _, lists = C.grid_table(6, 5, 70, 11)
    model = C.Model(g, [0, 29], B.table(lists))

    def need(w):
        assert w[0].total > 0 and w[1].total > 0 and not np.array_equal(w[0].eb_ptr, w[1].eb_ptr)
    check(spf_ctx, model, need=need)


@pytest.mark.parametrize("n_pfx", [255, 256, 257])
def test_prefix_counts_at_the_tile_edge(spf_ctx, n_pfx):
    g, S, lists = C.grid_table(5, 4, n_pfx, 400 + n_pfx)
    lists[-1] = [(19, 1)]                                                 # the far corner: both of the root's links
    lists[254] = [(18, 0), (14, 1)]
    model = C.Model(g, [S], B.table(lists))

    def need(w):
        cnt = np.diff(w[0].eb_ptr.astype(np.int64))
        assert cnt[254] == 2 and cnt[-1] == 2 and (cnt[:250] > 0).sum() > 100          # ECMP prefixes on both sides of the tile edge
    check(spf_ctx, model, remotes=(False,), need=need)


def test_more_ecmp_prefixes_in_a_tile_than_one_batch_holds(spf_ctx):
    """K = 40 spokes: 2048 / 40 = 51 prefixes per batch; 240 prefixes, most of them ECMP: the batch loop runs several times with a
    partial last batch, and the entries of one batch (up to 51 x 40) are dealt to the lanes in several rounds."""
    g, S, lists = C.spokes(40, 240, 77, far=3, far_share=0.7)
    model = C.Model(g, [S], B.table(lists))

    def need(w):
        n_ecmp = int(w[0].eb_coverage[0])
        assert n_ecmp > 2 * 51 and n_ecmp % 51 != 0 and w[0].total > 51 * 40
    check(spf_ctx, model, remotes=(False,), need=need)


def test_a_prefix_with_forty_advertisers(spf_ctx):
    g, S, lists = C.grid_table(8, 8, 30, 5, wide=(7, 40))
    model = C.Model(g, [S], B.table(lists))

    def need(w):
        assert len(lists[7]) == 40 and len(w[0].entries(7)) == 2
    check(spf_ctx, model, remotes=(False,), need=need)


def test_a_table_without_an_ecmp_prefix(spf_ctx):
    g, S, lists = C.chain_table(30)
    model = C.Model(g, [S], B.table(lists))
    d = Device(spf_ctx, model)
    try:
        total, ptr, *ent, cov = run_ecmp(d, model.table, remote=False)
        assert total == 0 and not ptr.any() and not cov.any() and all(len(x) == 0 for x in ent)
    finally:
        d.free()


def test_capacity_convention(spf_ctx):
    g, _, lists = C.grid_table(6, 5, 70, 11)
    model = C.Model(g, [0], B.table(lists))
    want = BE.want(model, 0, False)
    T = want[0].total
    assert T > 4
    d = Device(spf_ctx, model)
    try:
        r = d.routes(model.table)
        import torch
        ptr = torch.full((model.table.n + 1,), 7, dtype=torch.int32, device="cuda:0")
        args = (d.tab.n, d.tab.R, d.tab.W, d.tab.dist.data_ptr(), d.tab.flags.data_ptr(), d.tab.mask.data_ptr(), d.protect, model.table.ptr, model.table.vertex, model.table.metric)
        rt = tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask"))
        assert spf_ctx.routes_backup_ecmp_device(*args, routes=rt, eb_ptr_ptr=ptr.data_ptr()) == T            # cap 0 sizes the stream
        assert np.array_equal(ptr.cpu().numpy().view(np.uint32), want[0].eb_ptr)
        short = run_ecmp(d, model.table, remote=False, cap=T - 1, routes=r)                                     # one below: eb_ptr and the total
        assert short[0] == T and np.array_equal(short[1], want[0].eb_ptr)
        same(run_ecmp(d, model.table, remote=False, cap=T, routes=r), want)                                     # the exact cap fills everything
        same(run_ecmp(d, model.table, remote=False, cap=T + 5, routes=r), want)
    finally:
        d.free()


@pytest.mark.parametrize("seed", C.GPU_SEEDS)
def test_seeded_graphs_with_multihomed_prefixes(spf_ctx, seed):
    g, S, t = C.random_multihomed(seed)
    check(spf_ctx, C.Model(g, [S], t), lfa_flags=(0, M.IGNORE_OVERLOAD))


def test_the_seeds_reach_every_kind_and_every_flag_bit():
    """(the seeds were chosen on the CPU; BK_NONE comes from the runs without the repairs)"""
    kinds, bits = set(), 0
    for seed in C.GPU_SEEDS:
        g, S, t = C.random_multihomed(seed)
        model = C.Model(g, [S], t)
        for rem in (True, False):
            w = BE.want(model, 0, rem)
            assert w[0].total > 0
            kinds |= kinds_of(w)
            bits |= int(np.bitwise_or.reduce(w[0].eb_flags))
    assert kinds == {BE.LFA, BE.NODE, BE.PAIR, BE.NOTHING} and bits == BE.NODE_PROTECT | BE.DOWNSTREAM | BE.EA_PRIMARY


def test_argument_errors_are_inval_and_name_the_call(spf_ctx):
    import torch
    from holo_amd import _lib as L
    from holo_amd import engine as E
    case = C.two_homes()
    model = C.Model(case[0], [case[1]], case[2])
    d = Device(spf_ctx, model)
    try:
        t, tab = model.table, d.tab
        r = d.routes(t)
        rt = tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask"))
        buf = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        p = buf.data_ptr()
        good = dict(routes=rt, eb_ptr_ptr=p, cap_entries=2, eb_primary_ptr=p, eb_kind_ptr=p, eb_slot_ptr=p, eb_metric_ptr=p, eb_flags_ptr=p, eb_coverage_ptr=p)
        args = [tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), d.protect, t.ptr, t.vertex, t.metric]

        def bad(a=None, **kw):
            with pytest.raises(E.HspfError) as ei:
                spf_ctx.routes_backup_ecmp_device(*(a or args), **dict(good, **kw))
            assert ei.value.code == -1 and "hspf_routes_backup_ecmp_device" in str(ei.value), str(ei.value)
        for k in ("eb_ptr_ptr", "eb_primary_ptr", "eb_kind_ptr", "eb_slot_ptr", "eb_metric_ptr", "eb_flags_ptr", "eb_coverage_ptr"):
            bad(**{k: 0})
        bad(routes=(0, rt[1], rt[2]))
        bad(tilfa=(p, 0, p))
        bad(flags=B.PFX_ORDERED, pfx_origin=np.zeros(len(t.vertex), np.uint32))
        bad(flags=0x100)
        for i in (3, 4, 5):
            bad(args[:i] + [0] + args[i + 1:])
        bad([tab.n, tab.R, 0] + args[3:])
        pc = d.protect[0]
        bad(args[:6] + [[(tab.R, pc[1], pc[2])]] + args[7:])                     # root_row >= n_rows
        bad(args[:7] + [np.array([0, 3], np.uint32)] + args[8:])                 # pfx_ptr malformed
        bad(args[:8] + [np.array([1, 99], np.uint32)] + args[9:])                # pfx_vertex out of range
        # out_total NULL, and the 32-bit bound, through the raw symbol
        arr, keep = spf_ctx._protect_array(d.protect, "test")
        ht = L.HspfPrefixTable(t.n, len(t.vertex), t.ptr.ctypes.data_as(L.u32p), t.vertex.ctypes.data_as(L.u32p), t.metric.ctypes.data_as(L.u32p), 0, None, None, None, None)
        hr = L.HspfRoutes(*rt)
        out = L.HspfBackupEcmpOut(p, None, None, None, None, None, None)
        head = (spf_ctx.handle, tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr, 1, 0)
        assert spf_ctx.lib.hspf_routes_backup_ecmp_device(*head, ctypes.byref(ht), ctypes.byref(hr), None, 0, ctypes.byref(out), None) == -1
        assert b"hspf_routes_backup_ecmp_device" in spf_ctx.lib.hspf_last_error(spf_ctx.handle)
        big = L.HspfPrefixTable(0xFFFFFFFF, len(t.vertex), t.ptr.ctypes.data_as(L.u32p), t.vertex.ctypes.data_as(L.u32p), t.metric.ctypes.data_as(L.u32p), 0, None, None, None, None)
        total = ctypes.c_uint64(7)
        assert spf_ctx.lib.hspf_routes_backup_ecmp_device(*head, ctypes.byref(big), ctypes.byref(hr), None, 0, ctypes.byref(out), ctypes.byref(total)) == -1
        assert b"2^32" in spf_ctx.lib.hspf_last_error(spf_ctx.handle) and total.value == 7
        del keep
        assert not buf.any()                                                     # nothing was launched
        same(run_ecmp(d, t, remote=False, routes=r), BE.want(model, 0, False))   # and the context still works
    finally:
        d.free()


def test_backup_routes_with_ecmp_agrees_with_the_raw_call_and_without_it_nothing_changes(spf_ctx):
    from holo_amd import engine as E
    g, _, lists = C.grid_table(6, 5, 70, 11)
    t = B.table(lists)
    model = C.Model(g, [0], t)
    G = spf_ctx.upload(*g, 0xFFFFFFFF)
    try:
        plain = spf_ctx.backup_routes(G, 0, (t.ptr, t.vertex, t.metric))
        both = spf_ctx.backup_routes(G, 0, (t.ptr, t.vertex, t.metric), ecmp=True)
    finally:
        G.free()
    assert plain.ecmp is None and isinstance(both.ecmp, E.BackupEcmpResult)
    for f in ("best_metric", "best_entry", "nexthop_mask") + B.FIELDS:
        assert np.array_equal(getattr(plain, f), getattr(both, f)), f
    assert_equal({k: getattr(plain, k) for k in B.FIELDS}, model.want(0, True))              # today's arrays, unchanged
    w = BE.want(model, 0, True)[0]
    assert w.total > 0
    for f in BE.FIELDS:
        assert np.array_equal(np.asarray(getattr(both.ecmp, f)).ravel(), getattr(w, f).ravel()), f
    p = int(w.eb_prefix[0])
    assert both.ecmp.entries(0, p) == w.entries(p) and both.ecmp.total == w.total
    assert (plain.bk_kind[0] == B.ECMP).sum() == w.eb_coverage[0]                              # the stream speaks about exactly the BK_ECMP prefixes
    with pytest.raises(ValueError):
        spf_ctx.backup_routes(None, 0, (t.ptr, t.vertex, t.metric), ecmp=True, lan_protect=True)
