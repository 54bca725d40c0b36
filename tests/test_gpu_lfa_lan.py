"""hspf_lfa_lan_device and hspf_routes_backup_lan_device on the GPU against the LAN models (tests/_lfa_lan_model.py) over the CPU
oracle's SPTs: every output array and the coverage, bit for bit, masks on and off.  The tables the kernels read come from
hspf_run_device on each engine configuration; the expected values never touch the engine.  Shapes: the hand-checked graphs of
tests/test_host_lfa_lan.py, the 256-destination tile edge, 64 / 65 slots (the LDS instantiation and the two-word one), several
protected roots over one table set, zero-cost links, sums beyond 32 bits, an unreachable island."""
import types

import numpy as np
import pytest

import _backup_model as B
import _lfa_lan_model as LM
import _lfa_model as M
from _engines import both_engines
from test_gpu_lfa import Tables, mesh, with_island
from test_host_lfa_lan import trap, two_lans, lone_candidate, two_lans_prefix, prefix_table, L_, S_, E_, A_, C_, D_, F_, T_

pytestmark = pytest.mark.gpu

WIDE = 0xFE000000
LFA_FIELDS = ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask", "coverage")


def _dev():
    import torch
    return torch, torch.device("cuda:0")


def run_lfa(ctx, tab, protect, lans, lfa_flags=0, masks=True, plain=False):
    torch, dev = _dev()
    P, n, W = len(protect), tab.n, tab.W
    slot = torch.full((P, n), 7, dtype=torch.int32, device=dev)
    metric = torch.full((P, n), 7, dtype=torch.int32, device=dev)
    fl = torch.full((P, n), 7, dtype=torch.uint8, device=dev)
    cov = torch.full((P, 5 if plain else 7), 7, dtype=torch.int32, device=dev)
    cm = torch.full((P, n, W), 7, dtype=torch.int64, device=dev) if masks else None
    nm = torch.full((P, n, W), 7, dtype=torch.int64, device=dev) if masks else None
    kw = dict(alt_slot_ptr=slot.data_ptr(), alt_metric_ptr=metric.data_ptr(), alt_flags_ptr=fl.data_ptr(), coverage_ptr=cov.data_ptr(),
              cand_mask_ptr=cm.data_ptr() if masks else 0, node_mask_ptr=nm.data_ptr() if masks else 0, lfa_flags=lfa_flags)
    args = (n, tab.R, W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect)
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    if plain:
        ctx.lfa_device(*args, **kw)
    else:
        ctx.lfa_lan_device(*args, lans, **kw)
    h = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)      # noqa: E731
    return dict(zip(LFA_FIELDS, (h(slot, np.uint32), h(metric, np.uint32), h(fl, np.uint8), h(cm, np.uint64), h(nm, np.uint64), h(cov, np.uint32))))


def run_backup(ctx, tab, protect, lans, pt, lfa_flags=0, masks=True, plain=False, tilfa=None, resident=False):
    """routes_device on every row, then the backup call.  Returns (the eight bk_* host arrays, the routes on the host)."""
    torch, dev = _dev()
    P, n, W, NP = len(protect), tab.n, tab.W, pt.n
    bm = torch.empty((tab.R, NP), dtype=torch.int32, device=dev)
    be = torch.empty((tab.R, NP), dtype=torch.int32, device=dev)
    nh = torch.empty((tab.R, NP, W), dtype=torch.int64, device=dev)
    tabs = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr())
    ctx.routes_device(n, tab.R, W, *tabs, pt.ptr, pt.vertex, pt.metric, flags=pt.flags, best_metric_ptr=bm.data_ptr(), best_entry_ptr=be.data_ptr(),
                      nexthop_mask_ptr=nh.data_ptr())
    out = dict(bk_kind=torch.full((P, NP), 7, dtype=torch.uint8, device=dev), bk_primary=torch.full((P, NP), 7, dtype=torch.int32, device=dev),
               bk_slot=torch.full((P, NP), 7, dtype=torch.int32, device=dev), bk_metric=torch.full((P, NP), 7, dtype=torch.int32, device=dev),
               bk_flags=torch.full((P, NP), 7, dtype=torch.uint8, device=dev),
               bk_cand_mask=torch.full((P, NP, W), 7, dtype=torch.int64, device=dev) if masks else None,
               bk_node_mask=torch.full((P, NP, W), 7, dtype=torch.int64, device=dev) if masks else None,
               bk_coverage=torch.full((P, 7 if plain else 9), 7, dtype=torch.int32, device=dev))
    ti = None
    if tilfa is not None:
        ti_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in tilfa]
        ti = tuple(t.data_ptr() for t in ti_dev)
    kw = {k + "_ptr": (0 if v is None else v.data_ptr()) for k, v in out.items()}
    call = ctx.routes_backup_device if plain else ctx.routes_backup_lan_device
    args = (n, tab.R, W, *tabs, protect) + (() if plain else (lans,)) + (pt.ptr, pt.vertex, pt.metric)
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    call(*args, routes=(bm.data_ptr(), be.data_ptr(), nh.data_ptr()), tilfa=ti, flags=pt.flags | (8 if resident else 0), lfa_flags=lfa_flags, **kw)
    dt = dict(bk_kind=np.uint8, bk_primary=np.uint32, bk_slot=np.uint32, bk_metric=np.uint32, bk_flags=np.uint8, bk_cand_mask=np.uint64,
              bk_node_mask=np.uint64, bk_coverage=np.uint32)
    return {k: None if v is None else v.cpu().numpy().view(dt[k]) for k, v in out.items()}


def plan(graph, roots_to_protect):
    """One table set for all protected roots: the union of [S] + neighbours + LANs; per root (model candidates, nbr_row, lan, lan_row)."""
    per, rows = [], []
    for S in roots_to_protect:
        c, r, _, lan, _ = LM.protect_one(*graph, S)
        per.append((c, lan))
        rows += [int(x) for x in r]
    roots = np.array(sorted(set(rows)), np.uint32)
    row_of = {int(v): i for i, v in enumerate(roots)}
    out = []
    for c, lan in per:
        nbr_row = np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32)
        lan_row = np.array([row_of.get(int(x), 0) for x in lan], np.uint32)
        out.append((row_of[c.root], c, nbr_row, lan, lan_row))
    return roots, out


def check(ctx, graph, roots_to_protect, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=0, need=None, pt=None, w_min=1, need_exact_row=False, tilfa=False,
          no_lans=False):
    """Device against model for every protected root: LFA (masks on and off) and, with `pt`, the backups.  Returns the LFA models."""
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    roots, per = plan(graph, roots_to_protect)
    for _, c, _, lan, _ in per:
        pc = E.lfa_candidates(*graph, c.root)
        assert np.array_equal(pc.nbr, c.nbr) and np.array_equal(pc.root_link, c.root_link)
        assert np.array_equal(E.lfa_lan_candidates(*graph, c.root), lan)
    if no_lans:
        per = [(r, c, nr, np.full(len(lan), M.NONE, np.uint32), lr) for r, c, nr, lan, lr in per]
    W = max(go.mask_words(*graph, roots), max((len(c.nbr) + 63) // 64 for _, c, _, _, _ in per), w_min)
    tab = Tables(ctx, graph, maxp, roots, run_flags, W)
    try:
        if need_exact_row:
            assert ((tab.flags.cpu().numpy().view(np.uint16)[per[0][0]] & 2) != 0).any()      # the protected root's own row is HSPF_RF_EXACT
        t = tab.ref
        want = [LM.lfa(t.dist, t.flags, t.mask, c, r, nr, lan, lr, lfa_flags) for r, c, nr, lan, lr in per]
        if need is not None:
            need(want)                                       # non-vacuity: a condition on the MODEL, before anything is compared
        protect = [(r, c, nr) for r, c, nr, _, _ in per]
        lans = [(lan, lr) for _, _, _, lan, lr in per]
        for masks in (True, False):
            got = run_lfa(ctx, tab, protect, lans, lfa_flags, masks)
            for i, w in enumerate(want):
                for f in LFA_FIELDS:
                    if got[f] is not None:
                        assert np.array_equal(got[f][i], getattr(w, f)), (f, i, masks)
        if no_lans:
            plain = run_lfa(ctx, tab, protect, None, lfa_flags, True, plain=True)
            got = run_lfa(ctx, tab, protect, lans, lfa_flags, True)
            for f in LFA_FIELDS[:-1]:
                assert np.array_equal(got[f], plain[f]), f
            assert np.array_equal(got["coverage"][:, :5], plain["coverage"]) and not got["coverage"][:, 5:].any()
        if pt is not None:
            ti = None
            if tilfa:                                        # a repair for every slot: only the LAN rule decides who may take it
                S = 64 * W
                k = np.tile(np.arange(S, dtype=np.uint32), (len(per), 1))      # HSPF_TILFA_NODE on even slots, HSPF_TILFA_PAIR on odd ones
                ti = ((1 + (k & 1)).astype(np.uint8), k, np.full((len(per), S), 7, np.uint32))
            bwant = []
            for i, (r, c, nr, lan, lr) in enumerate(per):
                rt = B.routes(t.dist, t.flags, t.mask, r, pt)
                tm = None if ti is None else types.SimpleNamespace(ti_kind=ti[0][i], ti_via=ti[1][i], ti_metric=ti[2][i])
                bwant.append(LM.backup(t.dist, t.flags, t.mask, c, r, nr, lan, lr, pt, rt, lfa_flags, tm))
            for masks in (True, False):
                got = run_backup(ctx, tab, protect, lans, pt, lfa_flags, masks, tilfa=ti, resident=not masks)      # second call: resident
                for i, w in enumerate(bwant):
                    for f in B.FIELDS:
                        if got[f] is not None:
                            assert np.array_equal(got[f][i], getattr(w, f)), (f, i, masks)
            if no_lans:
                plain = run_backup(ctx, tab, protect, None, pt, lfa_flags, True, plain=True, tilfa=ti)
                got = run_backup(ctx, tab, protect, lans, pt, lfa_flags, True, tilfa=ti)
                for f in B.FIELDS[:-1]:
                    assert np.array_equal(got[f], plain[f]), f
                assert np.array_equal(got["bk_coverage"][:, :7], plain["bk_coverage"]) and not got["bk_coverage"][:, 7:].any()
            return want, bwant
    finally:
        tab.free()
    return want


def slot_of(c, lan, v):
    return int(np.flatnonzero((c.nbr == v) & (lan == M.NONE))[0])


@both_engines
@pytest.mark.parametrize("run_flags", [0, 1])
def test_trap_the_cheapest_alternate_crosses_the_primarys_lan(spf_ctx, run_flags):
    graph, root = trap()
    pt = B.table([[(D_, 0)], [(T_, 0), (A_, 20)], [(E_, 0)], [(S_, 3)], [(C_, 1), (F_, 1)]])
    (want,), (bw,) = check(spf_ctx, graph, [root], run_flags=run_flags, pt=pt, tilfa=True)
    c, _, _, lan, _ = LM.protect_one(*graph, root)
    kC, kF = slot_of(c, lan, C_), slot_of(c, lan, F_)
    for D in (D_, T_):                                       # fails on the plain call: it offers C
        assert want.alt_slot[D] == kF and want.cand_mask[D, 0] == 1 << kF and want.alt_flags[D] & LM.LAN_REFUSED
    assert bw.bk_slot[:3].tolist() == [kF] * 3 and bw.bk_kind[3] == B.LOCAL


@both_engines
@pytest.mark.parametrize("run_flags", [0, 1])
def test_a_lan_primary_never_takes_the_per_link_repair(spf_ctx, run_flags):
    graph, root = lone_candidate()
    _, (bw,) = check(spf_ctx, graph, [root], run_flags=run_flags, pt=B.table([[(5, 0)], [(8, 0)], [(9, 0)]]), tilfa=True)
    assert bw.bk_kind.tolist() == [B.NOTHING, B.NODE, B.PAIR] and bw.bk_flags[0] == LM.LAN_PRIMARY | LM.LAN_REFUSED      # (on the model)


@both_engines
def test_prefix_rule_refuses_where_the_vertex_rule_passes(spf_ctx):
    graph, root = two_lans_prefix()
    (want,), (bw,) = check(spf_ctx, graph, [root], pt=B.table([[(8, 0), (9, 0)], [(8, 0)], [(9, 3)]]))
    c, _, _, lan, _ = LM.protect_one(*graph, root)
    kW = slot_of(c, lan, 10)
    assert (int(want.cand_mask[8, 0]) >> kW) & 1 and not (int(bw.bk_cand_mask[0, 0]) >> kW) & 1 and bw.bk_flags[0] & LM.LAN_REFUSED


@both_engines
@pytest.mark.parametrize("run_flags", [0, 1])
def test_root_on_two_lans(spf_ctx, run_flags):
    graph, root = two_lans()
    (want,), _ = check(spf_ctx, graph, [root], run_flags=run_flags, pt=B.table([[(5, 0)], [(5, 1), (6, 0)], [(3, 0), (4, 0)]]))
    assert want.alt_flags[5] == M.HAS_PRIMARY | M.ECMP | LM.LAN_PRIMARY | LM.LAN_REFUSED


def lsdb(n_routers, n_networks, seed, **kw):
    from holo_amd import synth
    g = synth.random_lsdb(n_routers, n_networks, 3.0, seed, metric_hi=6, **kw)
    return (g.row_ptr, g.col, g.metric, g.vflags), g.max_path_metric


def roots_on_lans(graph, count, min_cands=2):
    out = []
    for r in range(len(graph[3])):
        if graph[3][r] & 0x07:
            continue
        if (LM.lan_candidates(*graph, r) != M.NONE).any() and (M.candidates(*graph, r).nbr != M.NONE).sum() >= min_cands:
            out.append(r)
        if len(out) == count:
            break
    assert len(out) == count
    return out


def some_of_each(want):
    cov = sum(w.coverage.astype(np.int64) for w in want)
    assert cov[5] > 0 and cov[2] > 0, cov       # LAN primaries, and alternates (refusals are rare at random: the hand-made graphs pin them)


@both_engines
@pytest.mark.parametrize("n", [255, 256, 257])
def test_random_lsdbs_at_the_tile_edge(spf_ctx, n):
    graph, maxp = lsdb(n - 30, 30, 40 + n)
    assert len(graph[3]) == n
    check(spf_ctx, graph, roots_on_lans(graph, 2, 3), maxp=maxp, need=some_of_each, pt=prefix_table(n, n, B.PFX_LAST_MIN))


def hub_with_lans(n_p2p, seed):
    """Root 0 with `n_p2p` point-to-point neighbours and two LANs of six members each (the root among them): n_p2p + 2 + 12 slots."""
    r = np.random.default_rng(seed)
    k = n_p2p + 10
    l1, l2 = k + 1, k + 2
    links = M.both([(0, v, int(r.integers(5, 21))) for v in range(1, n_p2p + 1)])
    for lan, mem in ((l1, [0] + list(range(n_p2p + 1, n_p2p + 6))), (l2, [0] + list(range(n_p2p + 6, n_p2p + 11)))):
        for v in mem:
            links += [(v, lan, int(r.integers(1, 9))), (lan, v, 0)]
    seen = set()
    for _ in range(3 * k):
        a, b = (int(x) for x in r.integers(1, k + 1, 2))
        if a != b and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
            links += M.both([(a, b, int(r.integers(1, 9)))])
    return M.csr(k + 3, links, net=[l1, l2])


@both_engines
@pytest.mark.parametrize("slots", [64, 65])
def test_hub_root_one_and_two_mask_words(spf_ctx, slots):
    graph = hub_with_lans(slots - 14, 7)
    assert len(M.candidates(*graph, 0).nbr) == slots
    (want,), _ = check(spf_ctx, graph, [0], need=some_of_each, pt=prefix_table(len(graph[3]), 3))
    assert want.cand_mask.shape[1] == (1 if slots <= 64 else 2)


@both_engines
def test_eight_protected_roots_share_one_table_set(spf_ctx):
    graph, maxp = lsdb(90, 12, 5)
    check(spf_ctx, graph, roots_on_lans(graph, 8), maxp=maxp, need=some_of_each, pt=prefix_table(102, 9, B.PFX_SATURATING))


@both_engines
def test_zero_cost_links_an_exact_row(spf_ctx):
    rp, col, met, vf = mesh(300, 8, 1, 6, extra=2.0, zero_share=0.01)      # (the graph of test_gpu_lfa's zero-cost case) plus a LAN at the root
    links = [(u, int(col[k]), int(met[k])) for u in range(300) for k in range(rp[u], rp[u + 1])]
    for v, c in ((17, 2), (40, 1), (90, 3), (200, 1)):
        links += [(v, 300, c), (300, v, 0)]
    check(spf_ctx, M.csr(301, links, net=[300]), [17], need=some_of_each, need_exact_row=True)


@both_engines
def test_wide_metrics_sums_beyond_32_bits(spf_ctx):
    graph, root = trap()
    graph[2][graph[2] > 0] += 0x7E000000 // 2

    def need(want):
        assert (want[0].alt_metric > 0x7FFFFFFF).any() and want[0].coverage[6] > 0
    check(spf_ctx, graph, [root], maxp=WIDE, need=need, pt=B.table([[(D_, 0x7F000000)], [(T_, 5)]], B.PFX_SATURATING))


@both_engines
def test_unreachable_island(spf_ctx):
    graph, root = trap()
    (want,) = check(spf_ctx, with_island_keeping_flags(graph), [root])
    assert not want.alt_flags[8:].any() and (want.alt_slot[8:] == M.NONE).all()


def with_island_keeping_flags(graph):
    g = with_island(graph)
    g[3][:len(graph[3])] = graph[3]
    return g


@both_engines
@pytest.mark.parametrize("which", ["trap", "lsdb"])
def test_without_lans_the_outputs_are_those_of_the_plain_calls(spf_ctx, which):
    if which == "trap":
        (graph, root), maxp = trap(), 0xFFFFFFFF
        roots = [root]
    else:
        graph, maxp = lsdb(100, 12, 6)
        roots = roots_on_lans(graph, 3)
    check(spf_ctx, graph, roots, maxp=maxp, pt=prefix_table(len(graph[3]), 4), tilfa=True, no_lans=True)


@both_engines
def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    graph, root = trap()
    roots, ((r, c, nr, lan, lr),) = plan(graph, [root])
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, 1)
    pt = B.table([[(D_, 0)]])
    try:
        bad = [([(np.where(lan == L_, 99, lan), lr)], "lan of slot"), ([(lan, np.where(lan == L_, 99, lr))], "lan_row of slot")]
        for lans, text in bad:
            for call, name in ((run_lfa, "hspf_lfa_lan_device"), (lambda *a: run_backup(*a[:4], pt), "hspf_routes_backup_lan_device")):
                with pytest.raises(E.HspfError) as e:
                    call(spf_ctx, tab, [(r, c, nr)], lans)
                assert e.value.code == -1 and name in str(e.value) and text in str(e.value), str(e.value)
        # the raw call with lan == NULL, outputs pre-filled: nothing is written
        import ctypes
        import torch
        from holo_amd import _lib as L
        dev = torch.device("cuda:0")
        arr, keep = spf_ctx._protect_array([(r, c, nr)], "test")
        bufs = [torch.full((1, 8), 7, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.uint8, torch.int32)]
        out = L.HspfLfaOut(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), None, None, bufs[3].data_ptr())
        rc = spf_ctx.lib.hspf_lfa_lan_device(spf_ctx.handle, 8, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr, None, 1, 0,
                                             ctypes.byref(out))
        assert rc == -1 and "hspf_lfa_lan_device" in spf_ctx.last_error() and "NULL lan" in spf_ctx.last_error()
        empty = (L.HspfLfaLan * 1)()
        rc = spf_ctx.lib.hspf_lfa_lan_device(spf_ctx.handle, 8, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr, empty, 1, 0,
                                             ctypes.byref(out))
        assert rc == -1 and "NULL lan / lan_row array" in spf_ctx.last_error()
        rc = spf_ctx.lib.hspf_lfa_lan_device(spf_ctx.handle, 8, tab.R + 1, 0, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr, empty, 1, 0,
                                             ctypes.byref(out))
        assert rc == -1 and "hspf_lfa_lan_device" in spf_ctx.last_error()          # what hspf_lfa_device rejects, under the new name
        # the same three on the raw hspf_routes_backup_lan_device, and its lan / lan_row range errors
        rt = [torch.zeros((tab.R, 1) + sh, dtype=dt, device=dev) for sh, dt in (((), torch.int32), ((), torch.int32), ((1,), torch.int64))]
        ptab = L.HspfPrefixTable(1, 1, pt.ptr.ctypes.data_as(L.u32p), pt.vertex.ctypes.data_as(L.u32p), pt.metric.ctypes.data_as(L.u32p), 0, None, None, None, None)
        routes = L.HspfRoutes(*(x.data_ptr() for x in rt))
        bb = [torch.full((1, 1), 7, dtype=dt, device=dev) for dt in (torch.uint8, torch.int32, torch.int32, torch.int32, torch.uint8)]
        bcov = torch.full((1, 9), 7, dtype=torch.int32, device=dev)
        bout = L.HspfBackupOut(*(b.data_ptr() for b in bb), None, None, bcov.data_ptr())
        bad_lan, bad_row = np.where(lan == L_, 99, lan).astype(np.uint32), np.where(lan == L_, 99, lr).astype(np.uint32)
        one = lambda a, b: (L.HspfLfaLan * 1)(L.HspfLfaLan(a.ctypes.data_as(L.u32p), b.ctypes.data_as(L.u32p)))      # noqa: E731
        for larr, W_, text in ((None, 1, "NULL lan"), (empty, 1, "NULL lan / lan_row array"), (one(bad_lan, lr), 1, "lan of slot"),
                               (one(lan, bad_row), 1, "lan_row of slot"), (empty, 0, "out of range")):
            rc = spf_ctx.lib.hspf_routes_backup_lan_device(spf_ctx.handle, 8, tab.R, W_, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr,
                                                           larr, 1, 0, ctypes.byref(ptab), ctypes.byref(routes), None, ctypes.byref(bout))
            assert rc == -1 and "hspf_routes_backup_lan_device" in spf_ctx.last_error() and text in spf_ctx.last_error(), spf_ctx.last_error()
        torch.cuda.synchronize()
        assert all(bool((b == 7).all()) for b in bufs + bb + [bcov])
    finally:
        tab.free()


@both_engines
def test_lfa_and_backup_routes_end_to_end_with_lan_protect(spf_ctx):
    from holo_amd import engine as E
    graph, root = trap()
    G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        cand, plain = spf_ctx.lfa(G, root)
        cand2, res = spf_ctx.lfa(G, root, lan_protect=True)
        kC, kF = slot_of(cand, res.lan, C_), slot_of(cand, res.lan, F_)
        assert plain.alt_slot[0, D_] == kC and plain.coverage.shape == (1, 5) and plain.lan is None
        assert res.alt_slot[0, D_] == kF and res.alt_slot[0, T_] == kF and res.alt_flags[0, D_] & E.LFA_LAN_REFUSED and res.coverage.shape == (1, 7)
        pt = (np.array([0, 1, 2], np.uint32), np.array([D_, C_], np.uint32), np.array([0, 0], np.uint32))
        bp = spf_ctx.backup_routes(G, root, pt)
        bl = spf_ctx.backup_routes(G, root, pt, lan_protect=True)
        assert bp.bk_slot[0, 0] == kC and bp.bk_coverage.shape == (1, 7)
        assert bl.bk_slot[0, 0] == kF and bl.bk_kind[0, 0] == E.BK_LFA and bl.bk_flags[0, 0] & E.LFA_LAN_REFUSED and bl.bk_coverage.shape == (1, 9)
        assert bl.bk_kind[0, 1] == bp.bk_kind[0, 1] and not bl.bk_flags[0, 1] & E.LFA_LAN_PRIMARY      # C is reached over a p2p link
    finally:
        G.free()
