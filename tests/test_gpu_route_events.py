"""hspf_routes_events on the GPU: the stream against an independent numpy restatement of the action rule, the follow property
(old tables + stream == new tables), consistency with hspf_routes_diff_device + hspf_routes_pack, capacity / _rest / staging
growth, real tables of an isis-100k run before and after a cost change, argument errors."""
import ctypes
import types

import numpy as np
import pytest

import _route_events as RE
from holo_amd import _lib as L
from holo_amd import engine as E
from holo_amd import routes as RT
from holo_amd import synth

# (seed, roots, prefixes, mask words, share of re-drawn pairs, all four actions expected)
CASES = [
    (11, 1, 120_000, 1, 1e-4, True), (12, 1, 120_000, 1, 1e-2, True), (13, 1, 120_000, 1, 0.5, True),
    (14, 64, 120_000, 1, 1e-4, True), (15, 64, 120_000, 1, 1e-2, True), (16, 64, 120_000, 1, 0.5, True),
    (17, 3, 5_000, 2, 1e-4, False), (18, 3, 5_000, 2, 1e-2, True), (19, 3, 5_000, 2, 0.5, True),
    (20, 1, 1, 1, 0.0, False), (21, 1, 1, 1, 1.0, False),
    (22, 7, 333, 1, 0.5, True),                      # 2331 pairs: no multiple of 64, 256 or 1024
    (23, 5, 1_025, 3, 1e-2, False),                   # a tile boundary inside a root, three mask words
    (24, 1, 120_000, 1, 0.0, False),                  # all SAME: no event
    (25, 1, 120_000, 1, 1.0, False), (26, 3, 5_000, 2, 1.0, False),     # every pair an event
]
E_INVAL = -1            # HSPF_E_INVAL
IDS = [f"{r}x{p}-W{w}-d{d:g}" for _, r, p, w, d, _ in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generator_covers_the_actions(case):
    """(CPU) the inputs of the GPU test hold what they are meant to hold — checked with the numpy rule alone."""
    seed, R, P, W, density, all_four = case
    old, new = RE.table_pair(seed, R, P, W, density)
    act = RE.actions(old, new)
    if all_four:
        assert set(np.unique(act).tolist()) == {RE.SAME, RE.INSTALL, RE.WITHDRAW, RE.SILENT}
    if density == 0.0:
        assert not act.any()
    if density == 1.0:
        assert act.all()
    assert len(RE.want_stream(old, new, True)) == np.count_nonzero(act)
    got = RT.apply_route_events(tuple(a.copy() for a in old), RE.want_stream(old, new, True))
    assert all(np.array_equal(a, b) for a, b in zip(got, new))


def _upload(tables):
    import torch
    dev = torch.device("cuda:0")
    bm, be, nm = tables
    return (torch.from_numpy(bm.view(np.int32)).to(dev), torch.from_numpy(be.view(np.int32)).to(dev), torch.from_numpy(nm.view(np.int64)).to(dev))


def _ptrs(t):
    return tuple(x.data_ptr() for x in t)


def _pack_path(ctx, R, P, W, d_old, d_new):
    """Today's calls: diff, then the pack of the new set and of the old set."""
    import torch
    dev = torch.device("cuda:0")
    act = torch.empty((R, P), dtype=torch.uint8, device=dev)
    chg = torch.empty((max(R * P, 1),), dtype=torch.int32, device=dev)
    cptr = torch.empty((R + 1,), dtype=torch.int32, device=dev)
    ctx.routes_diff_device(R, P, W, _ptrs(d_old), _ptrs(d_new), action_ptr=act.data_ptr(), changed_ptr=chg.data_ptr(), changed_ptr_ptr=cptr.data_ptr())
    kw = dict(action_ptr=act.data_ptr(), changed_ptr=chg.data_ptr(), changed_ptr_ptr=cptr.data_ptr())
    return ctx.routes_pack(R, P, W, _ptrs(d_new), **kw), ctx.routes_pack(R, P, W, _ptrs(d_old), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stream_equals_the_numpy_restatement(spf_ctx, case):
    seed, R, P, W, density, _ = case
    old, new = RE.table_pair(seed, R, P, W, density)
    d_old, d_new = _upload(old), _upload(new)
    for with_silent in (True, False):
        want = RE.want_stream(old, new, with_silent)
        got = spf_ctx.routes_events(R, P, W, _ptrs(d_old), _ptrs(d_new), with_silent=with_silent)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got, want)
        if with_silent:                                       # the follow property: a caller's tables follow every event
            mine = RT.apply_route_events(tuple(a.copy() for a in old), got)
            assert all(np.array_equal(a, b) for a, b in zip(mine, new))
    # the INSTALL / WITHDRAW subset is what hspf_routes_diff_device + hspf_routes_pack hand over, old half = pack of the old set
    new_pack, old_pack = _pack_path(spf_ctx, R, P, W, d_old, d_new)
    assert np.array_equal(RT.events_as_pack_records(got), new_pack)
    oh, op = RT.events_as_pack_records(got, old_half=True), old_pack
    assert np.array_equal(oh[:, [0, 1, 3, 4]], op[:, [0, 1, 3, 4]]) and np.array_equal(oh[:, 6:], op[:, 6:])


def _raw_events(ctx, R, P, W, d_old, d_new, flags, cap, buf):
    o, n = L.HspfRoutes(*_ptrs(d_old)), L.HspfRoutes(*_ptrs(d_new))
    total = ctypes.c_uint32(0xDEAD)
    rc = ctx.lib.hspf_routes_events(ctx.handle, R, P, W, ctypes.byref(o), ctypes.byref(n), flags, cap,
                                    buf.ctypes.data_as(L.u32p) if buf is not None else None, ctypes.byref(total))
    return rc, int(total.value)


@pytest.mark.gpu
def test_capacity_rest_and_staging_growth():
    ctx = E.SpfContext(0)                                     # a context of its own: its staging starts small
    try:
        R, P, W = 2, 40_000, 1
        rw = E.EVENT_REC_WORDS + 4 * W
        small, big = RE.table_pair(31, R, P, W, 1e-3), RE.table_pair(32, R, P, W, 0.6)
        for old, new in (small, big):                         # the second pair has many more events than the first: the staging grows
            want = RE.want_stream(old, new, True)
            total = len(want)
            assert total > 2
            d_old, d_new = _upload(old), _upload(new)
            for cap in (0, 1, total - 1, total, total + 7):
                buf = np.full((max(cap, 1), rw), 0xABABABAB, np.uint32) if cap else None
                rc, n = _raw_events(ctx, R, P, W, d_old, d_new, E.EV_SILENT, cap, buf)
                assert rc == 0, ctx.last_error()
                assert n == total
                head = min(cap, total)
                if head:
                    assert np.array_equal(buf[:head], want[:head])
                if head < total:
                    tail = np.zeros((total - head, rw), np.uint32)
                    assert ctx.lib.hspf_routes_events_rest(ctx.handle, head, total - head, tail.ctypes.data_as(L.u32p)) == 0, ctx.last_error()
                    assert np.array_equal(tail, want[head:])
                mid = np.zeros((2, rw), np.uint32)            # any range, more than once
                assert ctx.lib.hspf_routes_events_rest(ctx.handle, total // 2, 2, mid.ctypes.data_as(L.u32p)) == 0
                assert np.array_equal(mid, want[total // 2:total // 2 + 2])
                assert ctx.lib.hspf_routes_events_rest(ctx.handle, total, 0, None) == 0
                assert ctx.lib.hspf_routes_events_rest(ctx.handle, total - 1, 2, mid.ctypes.data_as(L.u32p)) == E_INVAL
                assert "beyond" in ctx.last_error()
                assert ctx.lib.hspf_routes_events_rest(ctx.handle, 0xFFFFFFFF, 2, mid.ctypes.data_as(L.u32p)) == E_INVAL
            assert np.array_equal(ctx.routes_events(R, P, W, _ptrs(d_old), _ptrs(d_new)), want)
        # back to few events after many: still exact
        old, new = small
        assert np.array_equal(ctx.routes_events(R, P, W, _ptrs(_upload(old)), _ptrs(_upload(new))), RE.want_stream(old, new, True))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_argument_errors_are_inval_with_a_message():
    ctx = E.SpfContext(0)
    try:
        old, new = RE.table_pair(41, 1, 100, 1, 0.5)
        d_old, d_new = _upload(old), _upload(new)
        rw = E.EVENT_REC_WORDS + 4
        buf = np.zeros((100, rw), np.uint32)
        total = ctypes.c_uint32(0)
        o, n = L.HspfRoutes(*_ptrs(d_old)), L.HspfRoutes(*_ptrs(d_new))
        lib, h = ctx.lib, ctx.handle
        u = buf.ctypes.data_as(L.u32p)
        assert lib.hspf_routes_events_rest(h, 0, 1, u) == E_INVAL and ctx.last_error()        # no stream yet
        assert lib.hspf_routes_events(None, 1, 100, 1, ctypes.byref(o), ctypes.byref(n), 1, 100, u, ctypes.byref(total)) == E_INVAL
        bad = [
            (0, 100, 1, ctypes.byref(o), ctypes.byref(n), 1, 100, u, ctypes.byref(total)),          # no roots
            (1, 100, 0, ctypes.byref(o), ctypes.byref(n), 1, 100, u, ctypes.byref(total)),          # no mask words
            (1, 100, 1, None, ctypes.byref(n), 1, 100, u, ctypes.byref(total)),
            (1, 100, 1, ctypes.byref(o), None, 1, 100, u, ctypes.byref(total)),
            (1, 100, 1, ctypes.byref(o), ctypes.byref(n), 1, 100, None, ctypes.byref(total)),      # capacity without a buffer
            (1, 100, 1, ctypes.byref(o), ctypes.byref(n), 1, 100, u, None),                         # nowhere to put the count
            (1, 100, 1, ctypes.byref(o), ctypes.byref(n), 0x10, 100, u, ctypes.byref(total)),       # unknown flag
            (70_000, 70_000, 1, ctypes.byref(o), ctypes.byref(n), 1, 100, u, ctypes.byref(total)),  # more than 2^32 pairs
            (1, 100, 1, ctypes.byref(L.HspfRoutes(0, d_old[1].data_ptr(), d_old[2].data_ptr())), ctypes.byref(n), 1, 100, u, ctypes.byref(total)),
            (1, 100, 1, ctypes.byref(o), ctypes.byref(L.HspfRoutes(d_new[0].data_ptr(), d_new[1].data_ptr(), 0)), 1, 100, u, ctypes.byref(total)),
        ]
        for args in bad:
            assert lib.hspf_routes_events(h, *args) == E_INVAL, args[:3]
            assert "hspf_routes_events" in ctx.last_error()
            assert lib.hspf_routes_events_rest(h, 0, 1, u) == E_INVAL                        # a failed call leaves no stream behind
        # the context still works
        assert np.array_equal(ctx.routes_events(1, 100, 1, _ptrs(d_old), _ptrs(d_new)), RE.want_stream(old, new, True))
        # no prefixes: nothing to compare, no event
        assert lib.hspf_routes_events(h, 3, 0, 1, ctypes.byref(o), ctypes.byref(n), 1, 100, u, ctypes.byref(total)) == 0 and total.value == 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_real_tables_before_and_after_a_cost_change(spf_ctx):
    """BASELINE's isis-100k graph, one root, 120 000 prefixes: SPF + hspf_routes_device before and after a handful of link
    costs rose.  The stream passes the follow property, and its INSTALL / WITHDRAW subset expands to the same messages as the
    records of today's diff + pack."""
    import torch
    rng = np.random.default_rng(77)
    g = synth.isis_100k()
    n = g.n
    roots = np.array([n // 3], np.uint32)
    P = 120_000
    extra = rng.integers(0, P, 30_000)                         # a quarter of the prefixes has a second advertiser
    pfx = np.sort(np.concatenate([np.arange(P), extra]))
    vtx = rng.integers(0, n, len(pfx)).astype(np.uint32)
    met = rng.integers(0, 64, len(pfx)).astype(np.uint32)
    ptr = np.zeros(P + 1, np.uint32)
    np.add.at(ptr, pfx + 1, 1)
    ptr = np.cumsum(ptr, dtype=np.uint64).astype(np.uint32)
    m2 = g.metric.copy()
    rp = g.row_ptr.astype(np.int64)
    src = np.repeat(np.arange(n), np.diff(rp))
    root_nb = set(g.col[rp[roots[0]]:rp[roots[0] + 1]].tolist()) | {int(roots[0])}
    cand = np.nonzero(~np.isin(src, list(root_nb)))[0]          # the root's own row and its neighbours' keep their costs: slots mean the same
    pick = rng.choice(cand, size=40, replace=False)
    m2[pick] = m2[pick] + rng.integers(1, 50, 40).astype(np.uint32)
    dev = torch.device("cuda:0")
    sets, host = [], []
    Wn = None
    for metric in (g.metric, m2):
        G = spf_ctx.upload(g.row_ptr, g.col, metric, g.vflags, g.max_path_metric)
        W = G.mask_words(roots)
        assert Wn in (None, W)
        Wn = W
        dist = torch.empty((1, n), dtype=torch.int32, device=dev); hops = torch.empty((1, n), dtype=torch.int16, device=dev)
        flags = torch.empty((1, n), dtype=torch.int16, device=dev); mask = torch.empty((1, n, W), dtype=torch.int64, device=dev)
        spf_ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), hops_ptr=hops.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        bm = torch.empty((1, P), dtype=torch.int32, device=dev); be = torch.empty((1, P), dtype=torch.int32, device=dev)
        nm = torch.empty((1, P, W), dtype=torch.int64, device=dev)
        spf_ctx.routes_device(n, 1, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), ptr, vtx, met,
                              best_metric_ptr=bm.data_ptr(), best_entry_ptr=be.data_ptr(), nexthop_mask_ptr=nm.data_ptr())
        G.free()
        sets.append((bm, be, nm))
        host.append((bm.cpu().numpy().view(np.uint32), be.cpu().numpy().view(np.uint32), nm.cpu().numpy().view(np.uint64)))
    W = Wn
    stream = spf_ctx.routes_events(1, P, W, _ptrs(sets[0]), _ptrs(sets[1]))
    assert 0 < len(stream) < P
    assert np.array_equal(stream, RE.want_stream(host[0], host[1], True))
    mine = RT.apply_route_events(tuple(a.copy() for a in host[0]), stream)
    assert all(np.array_equal(a, b) for a, b in zip(mine, host[1]))
    new_pack, _ = _pack_path(spf_ctx, 1, P, W, sets[0], sets[1])
    prefixes = [f"10.{p >> 16}.{(p >> 8) & 255}.{p & 255}/32" for p in range(P)]
    slot_nh = {s: types.SimpleNamespace(ipv4=f"192.0.{s >> 8}.{s & 255}", ipv6=None, iface_name=f"eth{s % 7}") for s in range(64 * W)}
    ifindex = {f"eth{i}": i + 1 for i in range(7)}
    msgs_today = RT.expand_route_records(new_pack, prefixes, slot_nh, {}, ifindex, 16)
    msgs_events = RT.expand_route_records(RT.events_as_pack_records(stream), prefixes, slot_nh, {}, ifindex, 16)
    assert msgs_events == msgs_today and len(msgs_today) > 0
