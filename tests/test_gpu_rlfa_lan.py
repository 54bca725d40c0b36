"""hspf_rlfa_lan_device on the GPU against the model (tests/_rlfa_lan_model.py) over the CPU oracle's SPTs: every output array and
both count arrays, bit for bit; hspf_tilfa_device on the tables it wrote; hspf_routes_backup_lan_device with and without
HSPF_LFA_LAN_SAFE_REPAIRS.  Both table sets come from hspf_run_device on each engine configuration (the forward graph and the
product's transpose of it, root list [S] + neighbour routers + LANs); the expected values never touch the engine.  Shapes: the
hand-checked graphs of tests/test_host_rlfa_lan.py, the 256-vertex tile edge, 7 / 8 / 9 / 17 LAN slots (the chunk of 8), 64 / 65
slots, eight protected roots over one table set, asymmetric, wide and zero costs, an island, a pruned LAN, overloaded routers."""
import types

import numpy as np
import pytest

import _backup_model as B
import _lfa_lan_model as LM
import _lfa_model as M
import _rlfa_lan_model as RL
import _rlfa_model as R
import _tilfa_model as T
from _engines import both_engines
from test_gpu_lfa import mesh
from test_gpu_lfa_lan import hub_with_lans, lsdb, plan, roots_on_lans, run_backup, with_island_keeping_flags
from test_gpu_rlfa import Tables, run_rlfa
from test_host_lfa_lan import lone_candidate, two_lans
from test_host_rlfa_lan import q_only, trap_x, via_only, A_, C_, E_, F_, L_

pytestmark = pytest.mark.gpu

WIDE = 0xFE000000
NONE = M.NONE
TI_NAMES = ("ti_kind", "ti_p", "ti_q", "ti_via", "ti_link", "ti_metric", "ti_counts", "td_kind", "td_coverage")


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def run_rlfa_lan(ctx, tab, protect, lans, lfa_flags=0, spaces=True, alt_flags=None, keep=False):
    """hspf_rlfa_lan_device, every output pre-filled with 7.  Returns {field: host array}; with `keep` also the device tensors."""
    torch, dev = _torch()
    P, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, 7, dtype=dt, device=dev)      # noqa: E731
    t = dict(pq_node=full((P, S), torch.int32), pq_via=full((P, S), torch.int32), pq_metric=full((P, S), torch.int32),
             pq_counts=full((P, S, 5), torch.int32), space_flags=full((P, S, n), torch.uint8) if spaces else None,
             space_via=full((P, S, n), torch.int32) if spaces else None, rl_node=full((P, n), torch.int32), rl_via=full((P, n), torch.int32),
             rl_coverage=full((P, 6), torch.int32))
    alt = torch.from_numpy(np.ascontiguousarray(alt_flags)).to(dev) if alt_flags is not None else None
    ptr = lambda x: 0 if x is None else x.data_ptr()      # noqa: E731
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.rlfa_lan_device(tab.G, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr(), protect, lans,
                        pq_node_ptr=ptr(t["pq_node"]), pq_via_ptr=ptr(t["pq_via"]), pq_metric_ptr=ptr(t["pq_metric"]), pq_counts_ptr=ptr(t["pq_counts"]),
                        rl_node_ptr=ptr(t["rl_node"]), rl_via_ptr=ptr(t["rl_via"]), rl_coverage_ptr=ptr(t["rl_coverage"]),
                        space_flags_ptr=ptr(t["space_flags"]), space_via_ptr=ptr(t["space_via"]), alt_flags_in_ptr=ptr(alt), lfa_flags=lfa_flags)
    host = {k: None if x is None else x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in t.items()}
    return (host, t, alt) if keep else host


def run_tilfa_on(ctx, tab, protect, dev_tables, alt, lfa_flags=0):
    """hspf_tilfa_device on the space tables another call left on the device."""
    torch, dev = _torch()
    P, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, 7, dtype=dt, device=dev)      # noqa: E731
    t = dict(ti_kind=full((P, S), torch.uint8), ti_p=full((P, S), torch.int32), ti_q=full((P, S), torch.int32), ti_via=full((P, S), torch.int32),
             ti_link=full((P, S), torch.int32), ti_metric=full((P, S), torch.int32), ti_counts=full((P, S, 2), torch.int32),
             td_kind=full((P, n), torch.uint8), td_coverage=full((P, 5), torch.int32))
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.tilfa_device(tab.G, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr(), protect,
                     space_flags_ptr=dev_tables["space_flags"].data_ptr(), space_via_ptr=dev_tables["space_via"].data_ptr(),
                     alt_flags_in_ptr=0 if alt is None else alt.data_ptr(), lfa_flags=lfa_flags, **{k + "_ptr": v.data_ptr() for k, v in t.items()})
    return {k: x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in t.items()}


def assert_rlfa(got, want, i, spaces=True, tag=""):
    for name in R.FIELDS:
        if not spaces and name.startswith("space_"):
            assert got[name] is None
            continue
        g, w = got[name][i], getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, i, name, np.argwhere(g != w)[:8].tolist())


def models(graph, roots_to_protect, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=0, w_min=1, with_alt=True, no_lans=False):
    """The model's side of a case (no device): (roots, per-root tuples, W, oracle tables, rdist, LFA models, RLFA models)."""
    from oracle import graph_oracle as go
    roots, per = plan(graph, roots_to_protect)
    if no_lans:
        per = [(r, c, nr, np.full(len(lan), NONE, np.uint32), lr) for r, c, nr, lan, lr in per]
    W = max(go.mask_words(*graph, roots), max((len(c.nbr) + 63) // 64 for _, c, _, _, _ in per), w_min)
    fwd, rdist = R.tables(graph, maxp, roots, run_flags, W)
    lfa = [LM.lfa(fwd.dist, fwd.flags, fwd.mask, c, r, nr, lan, lr, lfa_flags) for r, c, nr, lan, lr in per]
    rl = [RL.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], c, r, nr, lan, lr, lfa_flags, a.alt_flags if with_alt else None)
          for (r, c, nr, lan, lr), a in zip(per, lfa)]
    return roots, per, W, fwd, rdist, lfa, rl


def some_lost(rl):
    """Non-vacuity on the MODEL: LAN slots are there, the LAN conditions removed members, and a PQ node changed or went."""
    c4 = sum(int(w.pq_counts[:, 4].sum()) for w in rl)
    moved = sum(int(((w.plain.pq_node != w.pq_node) & (w.plain.pq_node != NONE)).sum()) for w in rl)
    assert c4 > 0 and moved > 0, (c4, moved)


def check(ctx, graph, roots_to_protect, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=(0,), need=some_lost, w_min=1, need_exact_row=False, tilfa=True,
          variants=((True, True),), no_lans=False):
    """Device against model for every protected root and every lfa_flags; `variants`: (space tables, alt_flags_in) pairs.  TI-LFA is
    run on the tables of the first variant when it has them.  Returns the RLFA models of the first lfa_flags."""
    first = None
    tab = None
    try:
        for lf in lfa_flags:
            roots, per, W, fwd, rdist, lfa, rl = models(graph, roots_to_protect, maxp, run_flags, lf, w_min, no_lans=no_lans)
            if first is None:
                first = rl
                if need is not None:
                    need(rl)                                     # before anything is compared
                tab = Tables(ctx, graph, maxp, roots, run_flags, W)
                assert np.array_equal(tab.rdist.cpu().numpy().view(np.uint32), rdist)      # the reverse run itself
                if need_exact_row:
                    assert ((tab.flags.cpu().numpy().view(np.uint16) & 2) != 0).any()
            protect = [(r, c, nr) for r, c, nr, _, _ in per]
            lans = [(lan, lr) for _, _, _, lan, lr in per]
            alt_flags = np.stack([a.alt_flags for a in lfa])
            for spaces, with_alt in variants:
                want = rl if with_alt else models(graph, roots_to_protect, maxp, run_flags, lf, w_min, with_alt=False, no_lans=no_lans)[6]
                got, dev_t, alt = run_rlfa_lan(ctx, tab, protect, lans, lf, spaces, alt_flags if with_alt else None, keep=True)
                for i, w in enumerate(want):
                    assert_rlfa(got, w, i, spaces, (lf, spaces, with_alt))
                if no_lans:                                      # the plain call on the same tables
                    plain = run_rlfa(ctx, tab, protect, lf, spaces, alt_flags if with_alt else None)
                    for name in R.FIELDS:
                        if got[name] is None:
                            continue
                        if name == "pq_counts":
                            assert np.array_equal(got[name][:, :, :4], plain[name]) and not got[name][:, :, 4].any()
                        elif name == "rl_coverage":
                            assert np.array_equal(got[name][:, :4], plain[name]) and not got[name][:, 4:].any()
                        else:
                            assert np.array_equal(got[name], plain[name]), name
                if tilfa and spaces and with_alt:
                    got_t = run_tilfa_on(ctx, tab, protect, dev_t, alt, lf)
                    for i, ((r, c, nr, _, _), w) in enumerate(zip(per, want)):
                        wt = RL.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, r, nr, w, alt_flags[i])
                        for name in T.FIELDS:
                            assert np.array_equal(got_t[name][i], getattr(wt, name)), ("tilfa", lf, i, name)
                        assert np.array_equal(wt.ti_counts[:, 0], w.pq_counts[:, 3])
    finally:
        if tab is not None:
            tab.free()
    return first


def hub_lans(m1, m2, seed, n_p2p=3):
    """Root 0 with `n_p2p` point-to-point neighbours and two LANs with m1 and m2 OTHER members: m1 + m2 candidate slots cross a LAN."""
    r = np.random.default_rng(seed)
    k = n_p2p + m1 + m2
    l1, l2 = k + 1, k + 2
    links = M.both([(0, v, int(r.integers(5, 21))) for v in range(1, n_p2p + 1)])
    for lan, mem in ((l1, [0] + list(range(n_p2p + 1, n_p2p + 1 + m1))), (l2, [0] + list(range(n_p2p + 1 + m1, k + 1)))):
        for v in mem:
            links += [(v, lan, int(r.integers(1, 9))), (lan, v, 0)]
    seen = set()
    for _ in range(3 * k):
        a, b = (int(x) for x in r.integers(1, k + 1, 2))
        if a != b and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
            links += M.both([(a, b, int(r.integers(1, 9)))])
    return M.csr(k + 3, links, net=[l1, l2])


def overloaded(which):
    """trap_x with HSPF_VF_NO_TRANSIT on C (the via-neighbour that releases A and X) or on F (the LAN-safe PQ node)."""
    graph, root = trap_x()
    graph[3][C_ if which == "via" else F_] |= 0x02
    return graph, root


def asym(graph):
    rp, col, met, vf = (np.array(x) for x in graph)
    src = np.repeat(np.arange(len(vf)), np.diff(rp.astype(np.int64)))
    up = ((vf[src] & 1) == 0) & ((vf[col] & 1) == 0) & (src < col)
    return rp, col, np.where(up, met + 3, met).astype(np.uint32), vf


def zero_cost():
    rp, col, met, vf = mesh(300, 8, 1, 6, extra=2.0, zero_share=0.01)
    links = [(u, int(col[k]), int(met[k])) for u in range(300) for k in range(rp[u], rp[u + 1])]
    for v, c in ((17, 2), (40, 1), (90, 3), (200, 1)):
        links += [(v, 300, c), (300, v, 0)]
    return M.csr(301, links, net=[300])


def wide():
    graph, root = trap_x()
    graph[2][graph[2] > 0] += 0x7E000000                      # two links fit under WIDE, three do not; sums of two rows pass 2^32
    return graph, root


def need_wide(rl):
    some_lost(rl)
    assert (rl[0].pq_metric >= 0x7E000000).any()


def pruned():
    """S = 1 and E = 2 on LAN 0 whose links back to its routers are dear (S -> L 5, L -> S 9, E -> L 5, L -> E 5); p2p S - V 4 and
    E - V 10 (V = 3).  With max_path_metric 12 S reaches L (5) and V (4), E reaches V (10), and L's own row does not reach V
    (9 + 4 = 13, 5 + 10 = 15): d(S, L) is finite and d(L, V) is HSPF_DIST_INF.  V is the plain PQ node of the slot S - L - E
    (4 < 10 + 10; 10 < 4 + 10) and falls out of P_lan on the INF term alone."""
    links = [(1, 0, 5), (0, 1, 9), (2, 0, 5), (0, 2, 5)] + M.both([(1, 3, 4), (2, 3, 10)])
    return M.csr(4, links, net=[0]), 1


# name -> (graph, protected roots, keyword arguments of check()); evaluated lazily, the models need no device
CASES = {
    "trap_x": lambda: (trap_x()[0], [trap_x()[1]], {}),
    "trap_x_net_nexthops": lambda: (trap_x()[0], [trap_x()[1]], dict(run_flags=1)),
    "q_only": lambda: (q_only()[0], [q_only()[1]], {}),
    "via_only": lambda: (via_only()[0], [via_only()[1]], {}),
    "two_lans_one_chunk": lambda: (two_lans()[0], [two_lans()[1]], {}),
    "tile_255": lambda: _tile(255), "tile_256": lambda: _tile(256), "tile_257": lambda: _tile(257),
    "lan_slots_7": lambda: (hub_lans(3, 4, 1), [0], {}), "lan_slots_8": lambda: (hub_lans(4, 4, 2), [0], {}),
    "lan_slots_9": lambda: (hub_lans(4, 5, 3), [0], {}), "lan_slots_17": lambda: (hub_lans(8, 9, 4), [0], {}),
    "slots_64": lambda: (hub_with_lans(50, 7), [0], dict(tilfa=False)), "slots_65": lambda: (hub_with_lans(51, 7), [0], dict(tilfa=False)),
    "eight_roots": lambda: _eight(),
    "asymmetric": lambda: _asym(),
    "wide": lambda: (wide()[0], [wide()[1]], dict(maxp=WIDE, need=need_wide)),
    "zero_cost_exact_row": lambda: (zero_cost(), [17], dict(need_exact_row=True, tilfa=False)),
    "island": lambda: (with_island_keeping_flags(trap_x()[0]), [trap_x()[1]], {}),
    "pruned_lan": lambda: (pruned()[0], [pruned()[1]], dict(maxp=12)),
    "overloaded_via": lambda: (overloaded("via")[0], [1], dict(lfa_flags=(0, 1), need=None)),
    "overloaded_pq": lambda: (overloaded("pq")[0], [1], dict(lfa_flags=(0, 1), need=None)),
    "no_lans_trap": lambda: (trap_x()[0], [trap_x()[1]], dict(no_lans=True, need=None)),
    "no_lans_lsdb": lambda: _no_lans(),
}


def _tile(n):
    graph, maxp = lsdb(n - 30, 30, 40 + n)
    assert len(graph[3]) == n
    return graph, roots_on_lans(graph, 2, 3), dict(maxp=maxp)


def _eight():
    graph, maxp = lsdb(90, 12, 5)
    return graph, roots_on_lans(graph, 8), dict(maxp=maxp, variants=((True, True), (False, True), (True, False), (False, False)))


def _asym():
    graph, maxp = lsdb(70, 10, 8)
    graph = asym(graph)
    return graph, roots_on_lans(graph, 2, 3), dict(maxp=maxp)


def _no_lans():
    graph, maxp = lsdb(100, 12, 6)
    return graph, roots_on_lans(graph, 3), dict(maxp=maxp, no_lans=True, need=None)


@both_engines
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(spf_ctx, name):
    graph, roots, kw = CASES[name]()
    rl = check(spf_ctx, graph, roots, **kw)
    if name == "trap_x":                                      # fails with hspf_rlfa_device in its place: that offers A
        e = int(np.flatnonzero((rl[0].plain.pq_node == A_) & (rl[0].pq_node == F_))[0])
        assert rl[0].pq_counts[e].tolist() == [2, 7, 4, 4, 3]
    if name == "two_lans_one_chunk":
        _, per, *_ = models(graph, roots)
        lan = per[0][3]
        assert len(np.flatnonzero(per[0][1].nbr != NONE)) <= 8 and {0, 1} <= {int(x) for x in lan}
    if name.startswith("lan_slots_"):
        _, per, *_ = models(graph, roots)
        assert int(((per[0][1].nbr != NONE) & (per[0][3] != NONE)).sum()) == int(name.rsplit("_", 1)[1])
    if name.startswith("slots_"):                            # one and two mask words
        _, per, W, *_ = models(graph, roots)
        n_slots = int(name.rsplit("_", 1)[1])
        assert len(per[0][1].nbr) == n_slots and W == (1 if n_slots <= 64 else 2) and rl[0].pq_node.shape == (64 * W,)
    if name == "pruned_lan":                                  # a LAN S reaches whose own row does not reach a member of the plain P-space
        _, per, _, fwd, *_ = models(graph, roots, maxp=kw["maxp"])
        r, c, _, lan, lr = per[0]
        hit = [(e, v) for e in np.flatnonzero((c.nbr != NONE) & (lan != NONE)) for v in np.flatnonzero(rl[0].plain.space_flags[e] & R.IN_P)
               if fwd.dist[r, lan[e]] != NONE and fwd.dist[lr[e], v] == NONE]
        assert hit and all(not rl[0].space_flags[e][v] & R.IN_P for e, v in hit)
    if name.startswith("overloaded"):                         # the overloaded router counts only with HSPF_LFA_IGNORE_OVERLOAD
        on = models(graph, roots, lfa_flags=1)[6][0]
        assert not np.array_equal(on.space_flags, rl[0].space_flags)


@both_engines
def test_backups_with_and_without_lan_safe_repairs(spf_ctx):
    graph, root = lone_candidate()
    roots, per, W, fwd, rdist, lfa, rl = models(graph, [root])
    (r, c, nr, lan, lr), = per
    pt = B.table([[(5, 0)], [(8, 0)], [(9, 0)]])
    S = 64 * W
    k = np.arange(S, dtype=np.uint32)[None, :]
    ti = ((1 + (k & 1)).astype(np.uint8), k, np.full((1, S), 7, np.uint32))
    tm = types.SimpleNamespace(ti_kind=ti[0][0], ti_via=ti[1][0], ti_metric=ti[2][0])
    rt = B.routes(fwd.dist, fwd.flags, fwd.mask, r, pt)
    args = (fwd.dist, fwd.flags, fwd.mask, c, r, nr, lan, lr, pt, rt)
    today, on = LM.backup(*args, 0, tm), RL.backup(*args, RL.LAN_SAFE_REPAIRS, tm)
    assert today.bk_kind.tolist() == [B.NOTHING, B.NODE, B.PAIR] and on.bk_kind[0] in (B.NODE, B.PAIR)      # (on the models)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        for lf, want in ((0, today), (RL.LAN_SAFE_REPAIRS, on), (1, LM.backup(*args, 1, tm)), (3, RL.backup(*args, 3, tm))):
            got = run_backup(spf_ctx, tab, [(r, c, nr)], [(lan, lr)], pt, lf, True, tilfa=ti)
            for f in B.FIELDS:
                assert np.array_equal(got[f][0], getattr(want, f)), (lf, f)
        plain = run_backup(spf_ctx, tab, [(r, c, nr)], None, pt, RL.LAN_SAFE_REPAIRS, True, plain=True, tilfa=ti)      # the plain call ignores the bit
        plain0 = run_backup(spf_ctx, tab, [(r, c, nr)], None, pt, 0, True, plain=True, tilfa=ti)
        assert all(np.array_equal(plain[f], plain0[f]) for f in B.FIELDS)
    finally:
        tab.free()


@both_engines
def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    import ctypes
    from holo_amd import engine as E, _lib as Lb
    torch, dev = _torch()
    graph, root = trap_x()
    roots, per, W, *_ = models(graph, [root])
    (r, c, nr, lan, lr), = per
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        for lans, text in (([(np.where(lan == L_, 99, lan), lr)], "lan of slot"), ([(lan, np.where(lan == L_, 99, lr))], "lan_row of slot")):
            with pytest.raises(E.HspfError) as e:
                run_rlfa_lan(spf_ctx, tab, [(r, c, nr)], lans)
            assert e.value.code == -1 and "hspf_rlfa_lan_device" in str(e.value) and text in str(e.value), str(e.value)
        bad_c = types.SimpleNamespace(root=c.root, nbr=np.where(c.nbr == E_, 99, c.nbr), cost=c.cost, root_link=c.root_link, cflags=c.cflags)
        with pytest.raises(E.HspfError) as e:                 # what hspf_rlfa_device rejects, under the new name
            run_rlfa_lan(spf_ctx, tab, [(r, bad_c, nr)], [(lan, lr)])
        assert e.value.code == -1 and "hspf_rlfa_lan_device" in str(e.value) and "nbr of slot" in str(e.value)
        # the raw call, outputs pre-filled: nothing is written
        arr, keep = spf_ctx._protect_array([(r, c, nr)], "test")
        larr, lkeep = spf_ctx._lan_array([(lan, lr)], [(r, c, nr)], "test")
        n, S = tab.n, 64 * W
        bufs = [torch.full(sh, 7, dtype=torch.int32, device=dev) for sh in ((1, S), (1, S), (1, S), (1, S, 5), (1, n), (1, n), (1, 6))]
        out = Lb.HspfRlfaOut(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), None, None, bufs[4].data_ptr(),
                             bufs[5].data_ptr(), bufs[6].data_ptr())
        head = (spf_ctx.handle, tab.G.handle, n, tab.R)
        tabs = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr())
        empty = (Lb.HspfLfaLan * 1)()
        call = spf_ctx.lib.hspf_rlfa_lan_device
        for args, text in (((*head, W, *tabs, arr, None, 1, 0, None, ctypes.byref(out)), "NULL lan"),
                           ((*head, W, *tabs, arr, empty, 1, 0, None, ctypes.byref(out)), "NULL lan / lan_row array"),
                           ((*head, 0, *tabs, arr, larr, 1, 0, None, ctypes.byref(out)), "out of range"),
                           ((*head, W, *tabs[:3], None, arr, larr, 1, 0, None, ctypes.byref(out)), "NULL graph, table"),
                           ((spf_ctx.handle, tab.G.handle, n + 1, tab.R, W, *tabs, arr, larr, 1, 0, None, ctypes.byref(out)), "n_vertices is not the graph's")):
            assert call(*args) == -1 and "hspf_rlfa_lan_device" in spf_ctx.last_error() and text in spf_ctx.last_error(), spf_ctx.last_error()
        torch.cuda.synchronize()
        assert all(bool((b == 7).all()) for b in bufs)
        del keep, lkeep
    finally:
        tab.free()


@both_engines
def test_engine_chain_end_to_end_with_lan_protect_and_lan_repairs(spf_ctx):
    from holo_amd import engine as E
    graph, root = trap_x()
    roots, per, W, fwd, rdist, lfa, rl = models(graph, [root])
    (r, c, nr, lan, lr), = per
    wt = RL.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, r, nr, rl[0], lfa[0].alt_flags)
    G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        cand, plain_lfa, plain_rl = spf_ctx.rlfa(G, root)
        cand2, res_lfa, res_rl, res_ti = spf_ctx.tilfa(G, root, lan_protect=True)
        e = int(np.flatnonzero((cand.nbr == E_) & (res_lfa.lan == L_))[0])
        assert plain_rl.pq_node[0, e] == A_ and plain_rl.pq_counts.shape[2] == 4 and plain_rl.rl_coverage.shape == (1, 4)
        assert res_rl.pq_node[0, e] == F_ and res_rl.pq_counts.shape[2] == 5 and res_rl.rl_coverage.shape == (1, 6)
        for name in R.FIELDS:
            assert np.array_equal(getattr(res_rl, name)[0], getattr(rl[0], name)), name
        for name in T.FIELDS:
            assert np.array_equal(getattr(res_ti, name)[0], getattr(wt, name)), name
        with pytest.raises(ValueError):
            spf_ctx.rlfa(G, root, lan_protect=True, symmetric=True)
    finally:
        G.free()
    # the backups: D = 5 of lone_candidate() sits behind a LAN primary without an alternate
    graph, root = lone_candidate()
    pt = (np.array([0, 1, 2, 3], np.uint32), np.array([5, 8, 9], np.uint32), np.zeros(3, np.uint32))
    G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        off = spf_ctx.backup_routes(G, root, pt, lan_protect=True)
        on = spf_ctx.backup_routes(G, root, pt, lan_protect=True, lan_repairs=True)
        roots, per, W, fwd, rdist, lfa, rl = models(graph, [root])
        (r, c, nr, lan, lr), = per
        wt = RL.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, r, nr, rl[0], lfa[0].alt_flags)
        tbl = B.table([[(5, 0)], [(8, 0)], [(9, 0)]])
        want = RL.backup(fwd.dist, fwd.flags, fwd.mask, c, r, nr, lan, lr, tbl, B.routes(fwd.dist, fwd.flags, fwd.mask, r, tbl), RL.LAN_SAFE_REPAIRS, wt)
        assert off.bk_kind[0, 0] == E.BK_NONE and off.bk_coverage.shape == (1, 9)
        for f in B.FIELDS:
            assert np.array_equal(getattr(on, f)[0], getattr(want, f)), f
        with pytest.raises(ValueError):
            spf_ctx.backup_routes(G, root, pt, lan_repairs=True)
    finally:
        G.free()
