"""hspf_routes_backup_ecmp_srlg_device on the GPU against the model (tests/_backup_ecmp_srlg_model.py) over the CPU oracle's SPTs:
eb_ptr, the five entry arrays, the eleven coverage words and the total, bit for bit, every output pre-filled.  The rows are the
engine's own (hspf_run_device of [S] ++ neighbour routers ++ member endpoints), the routes hspf_routes_device's (compared with the
model's first); the per-slot repairs are the TI-LFA MODEL's on the SRLG-safe tables, uploaded, as in tests/test_gpu_backup_ecmp.py.
Each case is the smallest shape at which one thing can go wrong: see the tests' names."""
import ctypes

import numpy as np
import pytest

import _backup_ecmp_cases as EC
import _backup_ecmp_srlg_cases as C
import _backup_ecmp_srlg_model as BES
import _backup_model as B
import _backup_srlg_cases as SC
import _lfa_model as M
import _srlg_model as SM
from test_gpu_backup_ecmp import OracleRows, SENTINEL, WIDE
from test_gpu_backup_ecmp import run_ecmp as run_plain
from test_gpu_backup_ecmp import same
from test_gpu_backup_srlg import Device
from test_gpu_srlg import product_members

pytestmark = pytest.mark.gpu

TI = ("ti_kind", "ti_via", "ti_metric", "ti_p", "ti_link")
SAFE = BES.SAFE_REPAIRS


class OracleDevice(Device):
    """The rows uploaded from the CPU oracle: for a root with more first-hop slots than hspf_run_device takes."""

    def __init__(self, ctx, model):
        from test_gpu_backup import protect_of
        self.ctx, self.model = ctx, model
        self.tab = OracleRows(model)
        self.protect = protect_of(model)
        self.srlgs = [product_members(m) for m in model.mems]


def run(d, t, lfa_flags=0, tilfa=None, cap=None, routes=None, srlgs=None, flags=None):
    """routes_device, then the call.  tilfa: None, or [object with ti_* per root].  cap None: the sizing call first, then arrays of
    that size (three elements more, checked to be untouched).  Returns (total, eb_ptr, eb_primary, eb_kind, eb_slot, eb_metric,
    eb_flags, eb_coverage) on the host."""
    import torch
    tab = d.tab
    P, NP, S = len(d.protect), t.n, 64 * tab.W
    r = routes or d.routes(t)
    ti = None
    if tilfa is not None:
        pad = lambda a: np.concatenate([np.asarray(a), np.zeros(S - len(a), np.asarray(a).dtype)])      # noqa: E731
        ti = [torch.from_numpy(np.stack([pad(getattr(x, k)) for x in tilfa]).view(np.uint8 if k == "ti_kind" else np.int32)).to("cuda:0") for k in TI]
    args = (tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), d.protect, srlgs or d.srlgs, t.ptr, t.vertex, t.metric)
    kw = dict(routes=tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")), tilfa=None if ti is None else tuple(x.data_ptr() for x in ti),
              flags=t.flags if flags is None else flags, lfa_flags=lfa_flags)
    ptr = torch.full((P * NP + 1,), 7, dtype=torch.int32, device="cuda:0")
    if cap is None:
        cap = d.ctx.routes_backup_ecmp_srlg_device(*args, eb_ptr_ptr=ptr.data_ptr(), **kw)
        assert int(ptr[-1].item()) == cap
        ptr.fill_(7)
    pri, slot, met = (torch.full((cap + 3,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(3))
    kind, fl = (torch.full((cap + 3,), 7, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    cov = torch.full((P, BES.COVERAGE_WORDS), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    total = d.ctx.routes_backup_ecmp_srlg_device(*args, eb_ptr_ptr=ptr.data_ptr(), cap_entries=cap, eb_primary_ptr=pri.data_ptr(), eb_kind_ptr=kind.data_ptr(),
                                                 eb_slot_ptr=slot.data_ptr(), eb_metric_ptr=met.data_ptr(), eb_flags_ptr=fl.data_ptr(),
                                                 eb_coverage_ptr=cov.data_ptr(), **kw)
    h = lambda x, dt: x.cpu().numpy().view(dt)      # noqa: E731
    for x in (pri, slot, met):
        assert (h(x, np.uint32)[cap:] == SENTINEL).all()                 # nothing is written beyond the capacity
    assert (h(kind, np.uint8)[cap:] == 7).all() and (h(fl, np.uint8)[cap:] == 7).all()
    k = min(total, cap)
    return total, h(ptr, np.uint32), h(pri, np.uint32)[:k], h(kind, np.uint8)[:k], h(slot, np.uint32)[:k], h(met, np.uint32)[:k], h(fl, np.uint8)[:k], h(cov, np.uint32)


def repairs_of(model, lf, rem):
    return [x[2] for x in model.frr(lf)] if rem else None


def check(ctx, model, lfa_flags=(0, SAFE), remotes=(True, False), need=None, device=Device):
    """The model's protected roots and table on the device, for every lfa_flags with and without the repairs."""
    if need is not None:
        need(BES.want(model, lfa_flags[0], remotes[0]))          # non-vacuity: on the MODEL, before anything is compared
    d = device(ctx, model)
    try:
        r = d.routes(model.table)
        for lf in lfa_flags:
            for rem in remotes:
                same(run(d, model.table, lf, repairs_of(model, lf, rem), routes=r), BES.want(model, lf, rem), tag=(lf, rem))
    finally:
        d.free()


def with_members(w):
    assert sum(int(x.eb_coverage[8]) for x in w) > 0 and sum(int(x.eb_coverage[9]) for x in w) > 0


def test_conduit_pair_takes_the_third_uplink_and_not_the_other_primary(spf_ctx):
    """The test that fails without the feature: the plain ECMP call hands each of the two uplinks in one conduit the other."""
    case = C.conduit_pair()
    model = C.model_of(case)
    d = Device(spf_ctx, model)
    try:
        total, ptr, pri, kind, slot, met, fl, cov = run(d, model.table)
        assert total == 2 and pri.tolist() == [0, 1] and kind.tolist() == [BES.LFA, BES.LFA]
        assert slot.tolist() == [2, 2] and met.tolist() == [3, 3]
        assert fl.tolist() == [BES.NODE_PROTECT | BES.SRLG_REFUSED | BES.SRLG_PRIMARY] * 2
        assert cov.tolist() == [[1, 2, 2, 2, 0, 0, 0, 1, 2, 2, 0]]
        plain = run_plain(d, model.table, remote=False)
        assert plain[4].tolist() == [1, 0] and plain[7][0, 7] == 1      # the plain call on the same tables: each other, "every primary covered"
    finally:
        d.free()


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_cases(spf_ctx, name):
    case = C.HAND[name]()
    model = C.model_of(case)
    d = Device(spf_ctx, model)
    try:
        r = d.routes(model.table)
        for exp in case["expect"]:
            lf, ti = exp[0], exp[1]
            total, *got = run(d, model.table, lf, None if ti is None else [ti], routes=r)
            for f, g, w in zip(BES.FIELDS, got, C.expected(exp)):
                assert np.array_equal(np.asarray(g).ravel(), w), (name, lf, f, g, w)
            assert total == len(exp[3])
    finally:
        d.free()


@pytest.mark.parametrize("seed", EC.GPU_SEEDS[:2])
def test_without_members_every_shared_output_is_the_plain_calls(spf_ctx, seed):
    g, S, t = EC.random_multihomed(seed)
    model = C.Model(g, [S], *SC.group(g), t, no_members=True)
    d = Device(spf_ctx, model)
    try:
        r = d.routes(t)
        for lf in (0, SAFE, M.IGNORE_OVERLOAD):
            for rem in (True, False):
                got = run(d, t, lf, repairs_of(model, lf, rem), routes=r)
                same(got, BES.want(model, lf, rem), tag=(lf, rem))
                plain = run_plain(d, t, lf & ~SAFE, rem, routes=r)
                assert got[0] == plain[0] and got[0] > 0
                for a, b in zip(got[1:7], plain[1:7]):
                    assert np.array_equal(a, b), (lf, rem)
                assert np.array_equal(got[7][:, :8], plain[7]) and not got[7][:, 8:].any()
    finally:
        d.free()


def spokes_with_groups(K, n_pfx, seed, sizes, **kw):
    """EC.spokes() with one group per entry of `sizes`: the link S -> spoke i + 1 and sizes[i] links drawn among the others."""
    g, S, lists = EC.spokes(K, n_pfx, seed, **kw)
    rp = g[0]
    r = np.random.default_rng(seed)
    far = np.arange(int(rp[1]), len(g[1]))
    of = {}
    for i, sz in enumerate(sizes):
        of.setdefault(int(rp[0]) + i, []).append(i + 1)
        for l in r.choice(far, sz, replace=False):
            of.setdefault(int(l), []).append(i + 1)
    return g, S, SM.groups_csr(len(g[1]), of), lists


def test_sixteen_members_nine_members_and_a_primary_without_any(spf_ctx):
    """Slot 0 has 16 members (both streams of the prefix's entries, every register of the packed array), slot 1 has 9 (the second
    stream for ONE member), slot 2 one, the others none: most ECMP prefixes have primaries with and without members."""
    g, S, (gp, gr), lists = spokes_with_groups(6, 60, 31, [16, 9, 1], far=2, ring=True, far_share=0.6)
    model = C.Model(g, [S], gp, gr, B.table(lists))

    def need(w):
        assert np.diff(model.mems[0].mem_ptr).tolist() == [16, 9, 1, 0, 0, 0]
        fl, pri = w[0].eb_flags, w[0].eb_primary
        for h in (0, 1):
            assert ((pri == h) & (fl & BES.SRLG_REFUSED != 0)).any(), h
        assert ((pri == 3) & (fl & BES.SRLG_PRIMARY == 0)).any() and 0 < w[0].eb_coverage[8] < w[0].eb_coverage[1]
    check(spf_ctx, model, need=need)


@pytest.mark.parametrize("K", [64, 65])
def test_a_root_with_one_and_two_mask_words(spf_ctx, K):
    g, S, (gp, gr), lists = spokes_with_groups(K, 40, 300 + K, [3, 2] + [0] * (K - 4) + [4, 2], far=2, ring=True, far_share=0.4)
    lists.append([(K - 1, 0), (K, 0)])                                    # the last two spokes: each is the other's backup
    model = C.Model(g, [S], gp, gr, B.table(lists))

    def need(w):
        assert model.W == (K + 63) // 64 and w[0].eb_primary.max() == K - 1 and np.diff(model.mems[0].mem_ptr)[K - 1] == 2
        with_members(w)
        assert (w[0].eb_flags[w[0].eb_primary == K - 1] & BES.SRLG_PRIMARY).all()
    check(spf_ctx, model, lfa_flags=(0,), remotes=(False,), need=need)


@pytest.mark.parametrize("n_pfx", [255, 256, 257])
def test_prefix_counts_at_the_tile_edge(spf_ctx, n_pfx):
    g, S, lists = EC.grid_table(5, 4, n_pfx, 400 + n_pfx)
    lists[-1] = [(19, 1)]                                                 # the far corner: both of the root's links
    lists[254] = [(18, 0), (14, 1)]
    gp, gr = SC.random_groups(g, 5, n_groups=(2, 3), per_group=(3, 5), root=S)
    model = C.Model(g, [S], gp, gr, B.table(lists))

    def need(w):
        cnt = np.diff(w[0].eb_ptr.astype(np.int64))
        assert cnt[254] == 2 and cnt[-1] == 2 and (cnt[:250] > 0).sum() > 100
        with_members(w)
    check(spf_ctx, model, lfa_flags=(0,), remotes=(False,), need=need)


def test_more_ecmp_prefixes_in_a_tile_than_one_batch_holds(spf_ctx):
    g, S, (gp, gr), lists = spokes_with_groups(40, 240, 77, [5, 0, 12, 3], far=3, far_share=0.7)
    model = C.Model(g, [S], gp, gr, B.table(lists))

    def need(w):
        n_ecmp = int(w[0].eb_coverage[0])
        assert n_ecmp > 2 * 51 and n_ecmp % 51 != 0 and w[0].total > 51 * 40
        with_members(w)
    check(spf_ctx, model, lfa_flags=(0,), remotes=(False,), need=need)


def test_more_candidates_than_one_lds_chunk_with_members_on_some_primaries(spf_ctx):
    """many_slots() of tests/_backup_ecmp_cases.py (2 057 candidates, a prefix with 257 primaries): the first link to B — slot
    2 054, what every link to A takes in the plain call — shares a group with the first three links to A, and a link to A with
    the link 3 -> 4.  The rows are uploaded from the CPU oracle, because hspf_run_device stops at 1 024 slots."""
    g, S, lists = EC.many_slots()
    rp = g[0]
    of = {int(rp[0]) + 2054: [1], int(rp[0]) + 1800: [1, 2], int(rp[0]) + 1801: [1], int(rp[0]) + 1802: [1], SM.link_pos(g, 3, 4): [2]}
    gp, gr = SM.groups_csr(len(g[1]), of)
    model = C.Model(g, [S], gp, gr, B.table(lists))

    def need(w):
        cnt = np.diff(w[0].eb_ptr.astype(np.int64)).tolist()
        assert len(model.cands[0].nbr) == 2057 and cnt == [257, 3]
        e = w[0].entries(0)
        assert e[0][0] == 1800 and e[0][2] == 2055 and e[0][4] & BES.SRLG_REFUSED      # the second link to B, out of the second chunk
        assert e[5][2] == 2054 and not e[5][4] & BES.SRLG_PRIMARY and 0 < w[0].eb_coverage[9] < 10
    check(spf_ctx, model, lfa_flags=(0,), remotes=(False,), need=need, device=OracleDevice)


def test_a_prefix_with_forty_advertisers(spf_ctx):
    g, S, lists = EC.grid_table(8, 8, 30, 5, wide=(7, 40))
    gp, gr = SC.random_groups(g, 9, n_groups=(3, 4), per_group=(4, 7), root=S)
    model = C.Model(g, [S], gp, gr, B.table(lists))

    def need(w):
        e = w[0].entries(7)
        assert len(lists[7]) == 40 and len(e) == 2 and any(x[4] & BES.SRLG_PRIMARY for x in e)
    check(spf_ctx, model, lfa_flags=(0,), remotes=(False,), need=need)


@pytest.mark.parametrize("flags", [B.PFX_SATURATING, B.PFX_SATURATING | B.PFX_LAST_MIN])
def test_terms_that_saturate_and_member_sums_beyond_32_bits(spf_ctx, flags):
    """The four-ring with costs of 0x7F000000: 0 -> 1 shares a group with 3 -> 2, 0 -> 3 with 1 -> 2.  For the candidate 3 of the
    primary 1, d(3, 3) + w + d_2(p) = 0x7F000000 + (a saturated 0xFFFFFFFF) lies beyond 32 bits (with HSPF_PFX_LAST_MIN prefix 0 is
    not ECMP; prefix 2 is, and its slot 1 is refused for slot 0)."""
    g, S, lists = EC.saturating()
    of = {SM.link_pos(g, 0, 1): [1], SM.link_pos(g, 3, 2): [1], SM.link_pos(g, 0, 3): [2], SM.link_pos(g, 1, 2): [2]}
    t = B.table(lists, flags)
    model = C.Model(g, [S], *SM.groups_csr(len(g[1]), of), t, maxp=WIDE)

    def need(w):
        f = model.fwd
        row2 = int(np.flatnonzero(model.roots == 2)[0])
        d2p = B.dist_to_prefix(f.dist, f.flags, row2, t, 0)[0]
        assert d2p == 0xFFFFFFFF and 0x7F000000 + d2p > 0xFFFFFFFF and w[0].eb_coverage[8] == w[0].eb_coverage[1] > 0
        assert model.routes().best_metric[0] == 0xFFFFFFFF and len(w[0].entries(2)) == 2 and w[0].eb_coverage[9] == 1
        if flags == B.PFX_SATURATING:                                     # in 32 bits the sum would wrap below d_3(p) = 0x90000000 and refuse slot 1
            assert w[0].entries(0)[0][1:3] == (BES.LFA, 1) and not w[0].entries(0)[0][4] & BES.SRLG_REFUSED
    check(spf_ctx, model, lfa_flags=(0,), remotes=(False,), need=need)


def test_two_protected_roots_with_different_slot_and_member_counts(spf_ctx):
    g, _, lists = EC.grid_table(6, 5, 70, 11)
    gp, gr = SC.random_groups(g, 4, n_groups=(4, 5), per_group=(3, 6), root=0)
    model = C.Model(g, [0, 14], gp, gr, B.table(lists))

    def need(w):
        assert w[0].total > 0 and w[1].total > 0 and len(model.cands[0].nbr) != len(model.cands[1].nbr)
        assert len(model.mems[0].tail) != len(model.mems[1].tail) and w[0].eb_coverage[8] > 0
    check(spf_ctx, model, need=need)


def test_capacity_convention(spf_ctx):
    g, S, (gp, gr), t = C.seeded(7152)
    model = C.Model(g, [S], gp, gr, t)
    want = BES.want(model, 0, False)
    T = want[0].total
    assert T > 4
    d = Device(spf_ctx, model)
    try:
        r = d.routes(t)
        import torch
        ptr = torch.full((t.n + 1,), 7, dtype=torch.int32, device="cuda:0")
        args = (d.tab.n, d.tab.R, d.tab.W, d.tab.dist.data_ptr(), d.tab.flags.data_ptr(), d.tab.mask.data_ptr(), d.protect, d.srlgs, t.ptr, t.vertex, t.metric)
        rt = tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask"))
        assert spf_ctx.routes_backup_ecmp_srlg_device(*args, routes=rt, eb_ptr_ptr=ptr.data_ptr()) == T      # cap 0 sizes the stream
        assert np.array_equal(ptr.cpu().numpy().view(np.uint32), want[0].eb_ptr)
        short = run(d, t, cap=T - 1, routes=r)                                                                 # one below: eb_ptr and the total
        assert short[0] == T and np.array_equal(short[1], want[0].eb_ptr)
        same(run(d, t, cap=T, routes=r), want)                                                                 # the exact cap fills everything
        same(run(d, t, cap=T + 5, routes=r), want)
    finally:
        d.free()


@pytest.mark.parametrize("seed", C.GPU_SEEDS)
def test_seeded_graphs_with_groups(spf_ctx, seed):
    g, S, (gp, gr), t = C.seeded(seed)
    model = C.Model(g, [S], gp, gr, t)
    d = Device(spf_ctx, model)
    try:
        r = d.routes(t)
        for lf in (0, SAFE, SAFE | M.IGNORE_OVERLOAD):
            for rem in (True, False):
                same(run(d, t, lf, repairs_of(model, lf, rem), routes=r), BES.want(model, lf, rem), tag=(seed, lf, rem))
        forged = C.forged_pair(model)                                     # every member primary's repair forces its first member
        same(run(d, t, SAFE, forged, routes=r), BES.want(model, SAFE, True, tilfa=forged), tag=(seed, "forged"))
    finally:
        d.free()


def test_argument_errors_are_inval_and_name_the_call(spf_ctx):
    import torch
    from holo_amd import engine as E
    case = C.conduit_pair()
    model = C.model_of(case)
    d = Device(spf_ctx, model)
    try:
        t, tab = model.table, d.tab
        r = d.routes(t)
        rt = tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask"))
        buf = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        p = buf.data_ptr()
        good = dict(routes=rt, eb_ptr_ptr=p, cap_entries=2, eb_primary_ptr=p, eb_kind_ptr=p, eb_slot_ptr=p, eb_metric_ptr=p, eb_flags_ptr=p, eb_coverage_ptr=p)
        args = [tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), d.protect, d.srlgs, t.ptr, t.vertex, t.metric]

        def bad(a=None, **kw):
            with pytest.raises(E.HspfError) as ei:
                spf_ctx.routes_backup_ecmp_srlg_device(*(a or args), **dict(good, **kw))
            assert ei.value.code == -1 and "hspf_routes_backup_ecmp_srlg_device" in str(ei.value), str(ei.value)
        for k in ("eb_ptr_ptr", "eb_primary_ptr", "eb_kind_ptr", "eb_slot_ptr", "eb_metric_ptr", "eb_flags_ptr", "eb_coverage_ptr"):
            bad(**{k: 0})
        bad(routes=(0, rt[1], rt[2]))
        bad(tilfa=(p, 0, p, p, p))
        bad(tilfa=(p, p, p, 0, p))                                               # ti_p missing
        bad(tilfa=(p, p, p, p, 0))                                               # ti_link missing
        bad(flags=B.PFX_ORDERED, pfx_origin=np.zeros(len(t.vertex), np.uint32))
        for i in (3, 4, 5):
            bad(args[:i] + [0] + args[i + 1:])
        mem = model.mems[0]
        K = len(model.cands[0].nbr)
        z17 = np.zeros(17, np.uint32)
        many = E.SrlgMembers(np.array([0] + [17] * K, np.uint32), z17, z17, z17, z17, z17, z17)
        bad(args[:7] + [[many]] + args[8:])                                      # 17 members on slot 0
        far = E.SrlgMembers(mem.mem_ptr, mem.tail, mem.pos, mem.head, mem.cost, mem.tail_row, np.full(len(mem.tail), tab.R, np.uint32))
        bad(args[:7] + [[far]] + args[8:])                                       # head_row >= n_rows
        out = np.full(len(mem.tail), tab.n, np.uint32)
        bad(args[:7] + [[E.SrlgMembers(mem.mem_ptr, out, mem.pos, mem.head, mem.cost, mem.tail_row, mem.head_row)]] + args[8:])      # tail >= n_vertices
        bad(args[:9] + [np.array([0, 3], np.uint32)] + args[10:])               # pfx_ptr malformed
        # a NULL srlg pointer, through the raw symbol
        from holo_amd import _lib as L
        arr, keep = spf_ctx._protect_array(d.protect, "test")
        ht = L.HspfPrefixTable(t.n, len(t.vertex), t.ptr.ctypes.data_as(L.u32p), t.vertex.ctypes.data_as(L.u32p), t.metric.ctypes.data_as(L.u32p), 0, None, None, None, None)
        hr = L.HspfRoutes(*rt)
        o = L.HspfBackupEcmpOut(p, None, None, None, None, None, None)
        total = ctypes.c_uint64(7)
        rc = spf_ctx.lib.hspf_routes_backup_ecmp_srlg_device(spf_ctx.handle, tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr,
                                                             None, 1, 0, ctypes.byref(ht), ctypes.byref(hr), None, 0, ctypes.byref(o), ctypes.byref(total))
        assert rc == -1 and b"hspf_routes_backup_ecmp_srlg_device" in spf_ctx.lib.hspf_last_error(spf_ctx.handle) and total.value == 7
        del keep
        assert not buf.any()                                                     # nothing was launched
        same(run(d, t, routes=r), BES.want(model, 0, False))                     # and the context still works
    finally:
        d.free()


def test_backup_routes_with_ecmp_and_groups_and_the_two_older_switches_unchanged(spf_ctx):
    from holo_amd import engine as E
    import _backup_ecmp_model as BE
    import _backup_srlg_model as BS
    case = C.conduit_pair()
    g, (gp, gr), t = case["graph"], case["groups"], case["table"]
    G = spf_ctx.upload(*g, 0xFFFFFFFF)
    try:
        res = spf_ctx.backup_routes(G, 0, (t.ptr, t.vertex, t.metric), ecmp=True, srlg=(gp, gr))
        assert isinstance(res.ecmp, E.BackupEcmpResult) and res.srlg is not None and res.ecmp.eb_coverage.shape == (1, 11)
        assert [e[:4] for e in res.ecmp.entries(0, 0)] == [(0, E.BK_LFA, 2, 3), (1, E.BK_LFA, 2, 3)]      # the hand case
        g2, S2, (gp2, gr2), t2 = C.seeded(7224)
        model = C.Model(g2, [S2], gp2, gr2, t2)
        G2 = spf_ctx.upload(*g2, 0xFFFFFFFF)
        try:
            tab = (t2.ptr, t2.vertex, t2.metric)
            for repairs in (False, True):
                lf = SAFE if repairs else 0
                both = spf_ctx.backup_routes(G2, S2, tab, ecmp=True, srlg=(gp2, gr2), srlg_repairs=repairs)
                w = BES.want(model, lf, True)[0]
                assert w.total > 0 and w.eb_coverage[8] > 0
                for f in BES.FIELDS:
                    assert np.array_equal(np.asarray(getattr(both.ecmp, f)).ravel(), getattr(w, f).ravel()), (f, repairs)
                only = spf_ctx.backup_routes(G2, S2, tab, srlg=(gp2, gr2), srlg_repairs=repairs)           # srlg alone: what it returned before
                assert only.ecmp is None
                ws = model.want(lf)[0]
                for f in BS.FIELDS:
                    assert np.array_equal(getattr(only, f)[0], getattr(ws, f)) and np.array_equal(getattr(both, f)[0], getattr(ws, f)), (f, repairs)
            plain = EC.Model(g2, [S2], t2)                                                                 # ecmp alone: what it returned before
            pe = spf_ctx.backup_routes(G2, S2, tab, ecmp=True)
            wp = BE.want(plain, 0, True)[0]
            assert pe.srlg is None and pe.ecmp.eb_coverage.shape == (1, 8)
            for f in BE.FIELDS:
                assert np.array_equal(np.asarray(getattr(pe.ecmp, f)).ravel(), getattr(wp, f).ravel()), f
        finally:
            G2.free()
        for kw in (dict(lan_protect=True), dict(node_protect=True)):
            with pytest.raises(ValueError):
                spf_ctx.backup_routes(G, 0, (t.ptr, t.vertex, t.metric), ecmp=True, **kw)
    finally:
        G.free()
