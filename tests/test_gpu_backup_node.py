"""hspf_routes_backup_node_device on the GPU against the plain-Python model (tests/_backup_node_model.py) over the CPU oracle's SPTs:
every output array and the coverage, bit for bit, into buffers pre-filled with a non-zero byte.  The tables the kernel reads are
the engine's own — hspf_run_device for the rows of the roots and of the listed nodes, hspf_routes_device for the routes (compared
with the model's first); the two lists and bk_kind / bk_flags are the MODELS', uploaded (tests/test_gpu_rlfa_node.py,
tests/test_gpu_tilfa_node.py and tests/test_gpu_backup.py check the calls that write them; the end-to-end tests below run the whole
chain on the device).  Each case is the smallest shape at which one thing can go wrong; what a case exists for is asserted on the
MODEL before anything is compared.  Every seed below was chosen on the CPU."""
import numpy as np
import pytest

import _backup_cases as C
import _backup_model as B
import _backup_node_cases as BC
import _backup_node_model as BN
import _lfa_model as M
from test_gpu_backup import HUB_SEEDS, WIDE, Device, advertiser_lists, random_table, saturating_case
from test_gpu_rlfa import hub, ring_chords

pytestmark = pytest.mark.gpu

FN = "hspf_routes_backup_node_device"
NONE = BN.NONE
OUT = dict(bn_kind=np.uint8, **{k: np.uint32 for k in BN.FIELDS[1:]})
RN, TQ = ("nq_node", "nq_via", "nq_metric", "nq_count"), ("tq_q", "tq_p", "tq_link", "tq_via", "tq_metric", "tq_count")
MESH = (120, 0, 7)                                        # (n, seed, protected root) of a unit-cost ring with as many chords: lists longer than 9


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).to("cuda:0")


class NodeDevice(Device):
    """tests/test_gpu_backup.py's Device plus the rows of the listed nodes and the new call."""

    def ydist(self, y_roots, run_flags=0):
        """[len(y_roots), n] device tensor: the engine's forward dist of every vertex of y_roots in its place(s), 7s in the rows of
        NO_ROOT entries."""
        import torch
        tab = self.tab
        out = torch.full((len(y_roots), tab.n), 7, dtype=torch.int32, device="cuda:0")
        real = sorted({int(v) for v in y_roots if v != NONE})
        if real:
            rows = torch.full((len(real), tab.n), 7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
            self.ctx.run_device(tab.G, np.array(real, np.uint32), run_flags, dist_ptr=rows.data_ptr())
            for i, v in enumerate(y_roots):
                if v != NONE:
                    out[i] = rows[real.index(int(v))]
        return out

    def backup_node(self, wants, t=None, y_roots=None, with_rn=True, with_tn=True, with_bk=True, sets=True, flags=None, routes=None, arrays=None,
                    protect=None, fill=7):
        """routes_device, then routes_backup_node_device on the uploaded lists of `wants` (one Want per protected root);
        {field: host array [n_prot, ...]} (the sets None when skipped)."""
        import torch
        tab, P = self.tab, len(wants)
        t = t or wants[0].table
        r = routes or self.routes(t, None if flags is None else flags & ~B.PFX_RESIDENT, arrays)
        if y_roots is None:
            y_roots = np.array(sorted({int(v) for w in wants for v in w.y_roots if v != NONE}) or [NONE], np.uint32)
        yd = self.ydist(y_roots, self.model.run_flags)
        shapes = {k: (P, t.n) for k in BN.FIELDS[:-1]}
        shapes["bn_coverage"] = (P, 6)
        out = {k: torch.full(sh, fill, dtype=torch.uint8 if OUT[k] == np.uint8 else torch.int32, device="cuda:0") for k, sh in shapes.items()
               if sets or not k.startswith("bn_set")}
        rn = [_dev(np.stack([getattr(w.rn, k) for w in wants])) for k in RN] if with_rn else None
        tn = [_dev(np.stack([getattr(w.tn, k) for w in wants])) for k in TQ] if with_tn else None
        bk = [_dev(np.stack([getattr(w.bk, k) for w in wants])) for k in ("bk_kind", "bk_flags")] if with_bk else None
        a = arrays or (t.ptr, t.vertex, t.metric)
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        self.ctx.routes_backup_node_device(tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect or self.protect, *a,
                                           routes=tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")), ydist_ptr=yd.data_ptr(),
                                           y_roots=y_roots, rn_sel=None if rn is None else tuple(x.data_ptr() for x in rn),
                                           max_pq=wants[0].rn.nq_node.shape[1] if with_rn else 0,
                                           tn_sel=None if tn is None else tuple(x.data_ptr() for x in tn),
                                           max_pairs=wants[0].tn.tq_q.shape[1] if with_tn else 0,
                                           bk_in=None if bk is None else tuple(x.data_ptr() for x in bk), flags=t.flags if flags is None else flags,
                                           **{k + "_ptr": x.data_ptr() for k, x in out.items()})
        return {k: (out[k].cpu().numpy().view(OUT[k]) if k in out else None) for k in shapes}


def assert_equal(got, wants, sets=True, tag=""):
    for i, w in enumerate(wants):
        for name in BN.FIELDS:
            if not sets and name.startswith("bn_set"):
                assert got[name] is None
                continue
            g, x = got[name][i], getattr(w.bn, name)
            assert g.shape == x.shape and g.dtype == x.dtype and np.array_equal(g, x), (tag, i, name, np.argwhere(g != x)[:8].tolist(), g[g != x][:8], x[g != x][:8])


def check(ctx, model, wants, **kw):
    """The model's protected roots on the device against `wants` (one Want per root, made with the same with_* as `kw`)."""
    d = NodeDevice(ctx, model)
    try:
        assert_equal(d.backup_node(wants, **kw), wants, tag=sorted(kw))
    finally:
        d.free()


def kinds_of(w):
    return {int(k) for k in w.bn.bn_kind}


def mesh_model(n_pfx=60):
    n, seed, root = MESH
    r = np.random.default_rng(300)
    return C.Model(ring_chords(n, seed, 1, 1, chords=n), [root], random_table(r, n, n_pfx))


def test_the_restated_table_recipe_is_the_original():
    """tests/_backup_node_cases.py restates random_table (its module must not import the GPU helpers); the seed notes there hold only
    while the two agree."""
    a, b = random_table(np.random.default_rng(11), 30, 40), BC.random_table(np.random.default_rng(11), 30, 40)
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("ptr", "vertex", "metric")) and a.flags == b.flags


def test_the_hand_checked_cases(spf_ctx):
    for case, kinds in ((BC.six_ring, {0, BN.BN_PQ, BN.BN_LAST_HOP}), (BC.five_ring, {0, BN.BN_LFA, BN.BN_LAST_HOP, BN.BN_PAIR})):
        g, S, t = case()
        model = C.Model(g, [S], t)
        w = BN.Want(model)
        assert kinds_of(w) == kinds
        check(spf_ctx, model, [w])


@pytest.mark.parametrize("n_pfx", [255, 256, 257])
def test_prefix_counts_at_the_tile_edge(spf_ctx, n_pfx):
    """The last valid lane of the one partial tile (255), the last lane of a full tile (256), the only valid lane of the second."""
    g, S, _ = BC.six_ring()
    lists = [[(1 + p % 5, p % 3)] + ([(3, 0)] if p % 2 else []) for p in range(n_pfx - 1)] + [[(1, 0), (3, 0)]]
    model = C.Model(g, [S], B.table(lists))
    w = BN.Want(model)
    assert w.bn.bn_kind[-1] == BN.BN_PQ and w.bn.bn_metric[-1] == 3 and {BN.BN_PQ, BN.BN_LAST_HOP} <= kinds_of(w)
    check(spf_ctx, model, [w])


@pytest.mark.parametrize("m", [1, 8, 9, 32])
def test_list_lengths_at_the_chunk_edge(spf_ctx, m):
    """max_pq = max_pairs = 1, the chunk (8), the chunk + 1, the most: lists that are cut short, and entries chosen from the second
    chunk."""
    model = mesh_model()
    w = BN.Want(model, max_pq=m, max_pairs=m, with_bk=False)
    assert w.rn.nq_count.max() > 9 and w.tn.tq_count.max() > 9
    assert m < 9 or (w.bn.bn_set_pq >> np.uint32(8)).any() and (w.bn.bn_set_pair >> np.uint32(8)).any()     # an entry of the second chunk protects
    assert BN.BN_PQ in kinds_of(w)
    check(spf_ctx, model, [w], with_bk=False)


def test_hub_root_with_65_slots_two_mask_words(spf_ctx):
    """The table seed (267; 260 .. 267 tried on the CPU) is the first with a one-primary prefix behind slot 64, the only slot of the
    second mask word.  Every alternate of the hub is node-protecting, so class 1 takes all with bk_in; without it the lists decide."""
    r = np.random.default_rng(267)
    model = C.Model(hub(65, HUB_SEEDS[65]), [0], random_table(r, 66, 48))
    w, wo = BN.Want(model), BN.Want(model, with_bk=False)
    assert model.W == 2 and len(model.cands[0].nbr) == 65
    assert (w.bn.bn_primary[w.bn.bn_kind > 0] == 64).any(), "no prefix behind the slot of the second word"
    assert BN.BN_LFA in kinds_of(w) and {BN.BN_PQ, BN.BN_LAST_HOP} <= kinds_of(wo) and wo.rn.nq_count.max() > 32
    check(spf_ctx, model, [w])
    check(spf_ctx, model, [wo], with_bk=False)


def test_advertiser_lists_empty_long_unreachable_and_local(spf_ctx):
    g, S, t = advertiser_lists()
    model = C.Model(g, [S], t)
    w = BN.Want(model, with_bk=False)
    k, ptr = w.bn.bn_kind, np.diff(t.ptr)
    assert ptr.tolist()[:5] == [0, 1, 33, 3, 1]
    assert k[0] == 0 and k[3] == 0 and k[4] == 0 and k[6] == 0                     # no entry | an island nothing reaches | S's own
    assert k[1] > 0 and k[2] > 0 and k[5] > 0 and (w.bn.bn_set_pq[[1, 2, 5]] != 0).any()
    check(spf_ctx, model, [w], with_bk=False)
    # the same lists behind a prefix with 71 entries: every vertex but S, the island's included, 27 of them twice
    many = [(v, 3 + v % 11) for v in range(45) if v != S] + [(v, 2 + v % 7) for v in range(4, 31)]
    long = B.table([many] + [[(x, m) for x, m, _ in t.entries(p)] for p in range(t.n)])
    m2 = C.Model(g, [S], long)
    w2 = BN.Want(m2, with_bk=False)
    assert np.diff(long.ptr)[0] == 71 and w2.bn.bn_kind[0] > 0
    check(spf_ctx, m2, [w2], with_bk=False)


@pytest.mark.parametrize("flags", [0, B.PFX_SATURATING])
def test_metrics_that_saturate_and_sums_beyond_32_bits(spf_ctx, flags):
    """The four-ring of tests/test_gpu_backup.py at costs of 0x7F000000: the listed node's d_Y(p) and d(Y, E) + d_E(p) pass 2^32."""
    g, S, lists = saturating_case()
    lists = lists + [[(2, 0xF0000000)], [(2, 0xF0000000), (1, 0xFFFFFFFF)], [(2, 5)]]
    model = C.Model(g, [S], B.table(lists, flags), maxp=WIDE)
    w = BN.Want(model, with_bk=False)
    assert {BN.BN_PQ} <= kinds_of(w) or {BN.BN_PAIR} <= kinds_of(w)
    assert (w.bn.bn_metric == BN.SAT).any()                                          # a chosen sum beyond 32 bits is saturated
    check(spf_ctx, model, [w], with_bk=False)


def test_y_rows_missing_duplicated_and_no_root_entries(spf_ctx):
    model = mesh_model(40)
    full = BN.Want(model, with_bk=False)
    listed = [int(v) for v in full.y_roots]
    assert len(listed) > 6
    drop = lambda ys: ys[::2]      # noqa: E731
    half = BN.Want(model, with_bk=False, y_pick=drop)
    assert not np.array_equal(half.bn.bn_set_pq, full.bn.bn_set_pq)                 # a listed node without a row is skipped
    d = NodeDevice(spf_ctx, model)
    try:
        assert_equal(d.backup_node([half], with_bk=False), [half], tag="missing")
        ys = np.array([NONE] + listed[:3] + [NONE] + listed + listed[-2:] + [NONE], np.uint32)
        assert_equal(d.backup_node([full], with_bk=False, y_roots=ys), [full], tag="duplicated, NO_ROOT")
        none = BN.Want(model, with_bk=False, y_pick=lambda ys: [])
        assert set(kinds_of(none)) <= {0, BN.BN_LAST_HOP, BN.BN_NONE}
        assert_equal(d.backup_node([none], with_bk=False, y_roots=np.array([NONE], np.uint32)), [none], tag="no rows at all")
    finally:
        d.free()


def test_only_one_list_both_lists_bk_in_and_the_set_tables(spf_ctx):
    """rn_sel alone, tn_sel alone, both; bk_in NULL against given: only the prefixes of class 1 move, to what the entries say;
    without the set tables nothing else changes."""
    m = BC.sweep_models()[4]
    both, rn, tn, nobk = BN.Want(m), BN.Want(m, with_tn=False), BN.Want(m, with_rn=False), BN.Want(m, with_bk=False)
    assert BN.BN_LFA in kinds_of(both) and BN.BN_PQ in kinds_of(both) and not np.array_equal(rn.bn.bn_kind, tn.bn.bn_kind)
    d = NodeDevice(spf_ctx, m)
    try:
        ys = both.y_roots
        g_both, g_rn, g_tn = d.backup_node([both]), d.backup_node([rn], with_tn=False, y_roots=ys), d.backup_node([tn], with_rn=False, y_roots=ys)
        g_nobk, g_bare = d.backup_node([nobk], with_bk=False), d.backup_node([both], sets=False)
    finally:
        d.free()
    assert_equal(g_both, [both]); assert_equal(g_rn, [rn]); assert_equal(g_tn, [tn]); assert_equal(g_nobk, [nobk]); assert_equal(g_bare, [both], sets=False)
    lfa = g_both["bn_kind"][0] == BN.BN_LFA
    assert lfa.any() and (g_nobk["bn_kind"][0][lfa] != BN.BN_LFA).all()
    for f in BN.FIELDS[:-1]:
        assert np.array_equal(g_both[f][0][~lfa], g_nobk[f][0][~lfa]), f
    assert all(np.array_equal(g_both[f], g_bare[f]) for f in BN.FIELDS if not f.startswith("bn_set"))


def test_three_protected_roots_share_one_table_set(spf_ctx):
    g, S, t = C.sweep_case(C.SWEEP_SEED + 8)
    nbrs = [int(x) for x in M.candidates(*g, S).nbr if x != M.NONE]
    model = C.Model(g, [nbrs[0], S, nbrs[-1]], t)
    wants = [BN.Want(model, i) for i in range(3)]
    assert model.root_row == [0, 1, 2] and len({tuple(w.bn.bn_kind.tolist()) for w in wants}) == 3
    check(spf_ctx, model, wants)


def test_resident_table_then_a_changed_one(spf_ctx):
    r = np.random.default_rng(9)
    g, S, _ = C.sweep_case(C.SWEEP_SEED + 3)
    nr = int((g[3] & M.VF_NETWORK == 0).sum())
    t1, t2 = random_table(r, nr, 70), random_table(r, nr, 70)
    model = C.Model(g, [S], t1)
    w1, w2 = BN.Want(model, table=t1), BN.Want(model, table=t2)
    assert not np.array_equal(w1.bn.bn_kind, w2.bn.bn_kind)
    d = NodeDevice(spf_ctx, model)
    try:
        r1 = d.routes(t1)                                                           # hspf_routes_device uploads t1 ...
        first = d.backup_node([w1], routes=r1, flags=B.PFX_RESIDENT)                # ... and this call finds it resident
        assert_equal(first, [w1], tag="resident")
        assert_equal(d.backup_node([w2]), [w2], tag="changed, uploaded")
        r2 = d.routes(t2)
        assert_equal(d.backup_node([w1], routes=r1), [w1], tag="back: the call itself uploads")
        assert_equal(d.backup_node([w2], routes=r2, flags=B.PFX_RESIDENT), [w2], tag="resident flag, other arrays")
    finally:
        d.free()


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import torch
    g, S, t = BC.six_ring()
    model = C.Model(g, [S], t)
    w = BN.Want(model)
    d = NodeDevice(spf_ctx, model)
    try:
        tab, pc, nr = d.tab, d.protect[0][1], model.nbr_row[0]
        r = d.routes(t)
        good = d.backup_node([w], routes=r)
        assert_equal(good, [w])
        NP = t.n
        sizes = {k: NP * (1 if k == "bn_kind" else 4) for k in BN.FIELDS[:-1]}
        sizes["bn_coverage"] = 24
        out = torch.full((sum((b + 7) // 8 * 8 for b in sizes.values()) + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        ptrs, off = {}, 0
        for k, b in sizes.items():
            ptrs[k + "_ptr"] = out.data_ptr() + off
            off += (b + 7) // 8 * 8
        yd = d.ydist(w.y_roots)
        rn = [_dev(getattr(w.rn, k)[None]) for k in RN]
        tn = [_dev(getattr(w.tn, k)[None]) for k in TQ]
        bk = [_dev(getattr(w.bk, k)[None]) for k in ("bk_kind", "bk_flags")]
        ok = dict(routes=tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")), ydist_ptr=yd.data_ptr(), y_roots=w.y_roots,
                  rn_sel=tuple(x.data_ptr() for x in rn), max_pq=16, tn_sel=tuple(x.data_ptr() for x in tn), max_pairs=16,
                  bk_in=tuple(x.data_ptr() for x in bk), flags=0)

        def expect_inval(protect=None, table=None, **kw):
            tables = dict(dist=tab.dist.data_ptr(), flags_=tab.flags.data_ptr(), mask=tab.mask.data_ptr())
            p = dict(ptrs, **ok)
            for k, v in kw.items():
                (tables if k in tables else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.routes_backup_node_device(tab.n, tab.R, 1, tables["dist"], tables["flags_"], tables["mask"], protect or d.protect,
                                                  *(table or (t.ptr, t.vertex, t.metric)), **p)
            assert e.value.code == -1 and FN in str(e.value), str(e.value)
            assert (out.cpu().numpy() == 0x5A).all()         # nothing was written: nothing was launched

        for k in ("dist", "flags_", "mask"):                 # NULL required pointers: the tables ...
            expect_inval(**{k: 0})
        for k in ("bn_kind", "bn_primary", "bn_p", "bn_q", "bn_link", "bn_via", "bn_metric", "bn_coverage"):      # ... the outputs ...
            expect_inval(**{k + "_ptr": 0})
        expect_inval(routes=(0,) + ok["routes"][1:])          # ... the routes ...
        expect_inval(routes=ok["routes"][:2] + (0,))
        bad_row = nr.copy()
        bad_row[0] = tab.R
        expect_inval(protect=[(0, pc, bad_row)])             # what hspf_lfa_device rejects in prot
        expect_inval(protect=[(tab.R, pc, nr)])
        many = E.LfaCandidates(0, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        expect_inval(protect=[(0, many, np.zeros(65, np.uint32))])
        expect_inval(flags=B.PFX_ORDERED)                     # out of scope
        expect_inval(flags=0x10)                             # what the table checks of hspf_routes_device reject
        expect_inval(table=(np.array([1, 2, 3, 4, 5], np.uint32), t.vertex, t.metric))
        expect_inval(table=(np.array([0, 3, 2, 3, 6], np.uint32), t.vertex, t.metric))
        bad_v = t.vertex.copy()
        bad_v[0] = 6
        expect_inval(table=(t.ptr, bad_v, t.metric))
        expect_inval(ydist_ptr=0)                            # what hspf_rlfa_node_device rejects about the y rows
        expect_inval(y_roots=np.zeros(0, np.uint32))
        expect_inval(y_roots=np.array([3, 6], np.uint32))
        expect_inval(rn_sel=None, tn_sel=None)               # no list at all
        expect_inval(rn_sel=(0,) + ok["rn_sel"][1:])         # a NULL array in a given sel / bk_in
        expect_inval(tn_sel=ok["tn_sel"][:5] + (0,))
        expect_inval(bk_in=(0, ok["bk_in"][1]))
        expect_inval(bk_in=(ok["bk_in"][0], 0))
        for bad in (0, 33):                                  # the limits of a given sel
            expect_inval(max_pq=bad)
            expect_inval(max_pairs=bad)
        lib = L.load()
        assert lib.hspf_routes_backup_node_device(spf_ctx.handle, tab.n, tab.R, 1, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(),
                                                  None, 1, None, None, None, None, 0, None, 0, None, 0, None, None) == -1
        assert FN in spf_ctx.last_error()
        # the limit of a sel that is NULL is not read; and the context still works
        again = d.backup_node([BN.Want(model, with_tn=False)], with_tn=False, routes=r)
        assert_equal(again, [BN.Want(model, with_tn=False)])
        assert all(np.array_equal(good[k], v) for k, v in d.backup_node([w], routes=r).items())
    finally:
        d.free()


def _same(res, w, tag):
    for name in ("best_metric", "best_entry", "nexthop_mask"):
        assert np.array_equal(getattr(res, name)[0], getattr(w.routes, name)), (tag, name)
    for name in B.FIELDS:
        assert np.array_equal(getattr(res, name)[0], getattr(w.bk, name)), (tag, name)
    for name in BN.FIELDS:
        g, x = getattr(res, name)[0], getattr(w.bn, name)
        assert g.dtype == x.dtype and np.array_equal(g, x), (tag, name, g, x)


def test_backup_routes_node_protect_end_to_end_and_the_default_path(spf_ctx):
    """SpfContext.backup_routes(node_protect=True): run, routes, lfa, rlfa + tilfa, backup, the two select calls, the run over the
    listed nodes, the new call — all on the device — on the six-ring, and on the patched handle of chain (a) of
    tests/_frr_chains.py.  Without the flag the result is what it was: every bn_* field None, everything else equal."""
    import dataclasses
    import _frr_chains as F
    g, S, t = BC.six_ring()
    model = C.Model(g, [S], t)
    w = BN.Want(model)
    G = spf_ctx.upload(*g, C.MAXP)
    try:
        for symmetric in (False, True):
            res = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), symmetric=symmetric, node_protect=True)
            _same(res, w, ("six-ring", symmetric))
        plain = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric))
        assert all(getattr(plain, f) is None for f in BN.FIELDS)
        for f in dataclasses.fields(plain):
            a, b = getattr(plain, f.name), getattr(res, f.name)
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and np.array_equal(a, b), f.name
        for name in B.FIELDS:
            assert np.array_equal(getattr(plain, name)[0], getattr(w.bk, name)), name
        small = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), node_protect=True, max_pq=1, max_pairs=1)
        _same(small, BN.Want(model, max_pq=1, max_pairs=1), "max 1")
        with pytest.raises(ValueError):
            spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), node_protect=True, remote=False)
    finally:
        G.free()
    chain = F.chain("a")
    g5, S5, t5 = BC.five_ring()
    assert all(np.array_equal(x, y) for x, y in zip(chain.steps[0].graph, g5)) and chain.steps[0].prot == (S5,)
    G = spf_ctx.upload(*g5, C.MAXP)
    try:
        _same(spf_ctx.backup_routes(G, S5, (t5.ptr, t5.vertex, t5.metric), node_protect=True), BN.Want(C.Model(g5, [S5], t5)), "five-ring")
        G.patch(chain.steps[1].patch.vs, chain.steps[1].patch.rows, chain.steps[1].patch.flags)
        patched = C.Model(chain.steps[1].graph, [S5], t5)
        _same(spf_ctx.backup_routes(G, S5, (t5.ptr, t5.vertex, t5.metric), node_protect=True), BN.Want(patched), "patched")
    finally:
        G.free()
