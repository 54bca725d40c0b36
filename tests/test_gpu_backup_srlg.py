"""hspf_routes_backup_srlg_device on the GPU against the model (tests/_backup_srlg_model.py) over the CPU oracle's SPTs: every output
array and the coverage, bit for bit, every output pre-filled with 7.  The tables the kernel reads are the engine's own:
hspf_run_device for the rows ([S] + neighbour routers + member endpoints), hspf_routes_device for the routes, hspf_lfa_srlg_device +
hspf_rlfa_srlg_device + hspf_tilfa_device for the repairs.  Each case is the smallest shape at which one thing can go wrong: the
chunk of 8 candidate slots, 16 members and 1, the 256-prefix tile, empty / long / own-entry advertiser lists, two mask words,
several protected roots, the table flags, no repairs, a forced link that is a member, no masks, empty member tables."""
import ctypes

import numpy as np
import pytest

import _backup_cases as C
import _backup_model as B
import _backup_srlg_cases as SC
import _backup_srlg_model as BS
import _lfa_model as M
import _srlg_model as SM
from test_gpu_backup import HUB_SEEDS, OUT, _torch_dt
from test_gpu_rlfa import Tables, hub, ring_chords
from test_gpu_rlfa_lan import run_tilfa_on
from test_gpu_srlg import product_members, run_lfa_srlg, run_rlfa_srlg

pytestmark = pytest.mark.gpu

TI = ("ti_kind", "ti_via", "ti_metric", "ti_p", "ti_link")


class Device:
    """The rows of the model's roots on the device, from the engine."""

    def __init__(self, ctx, model):
        from holo_amd import engine as E
        self.ctx, self.model = ctx, model
        self.tab = Tables(ctx, model.graph, model.maxp, model.roots, model.run_flags, model.W)
        self.protect = [(rr, E.lfa_candidates(*model.graph, r), nr) for r, rr, nr in zip(model.prot, model.root_row, model.nbr_row)]
        self.srlgs = [product_members(m) for m in model.mems]
        self._ti = {}

    def free(self):
        self.tab.free()

    def routes(self, t: B.Table):
        import torch
        tab, NP = self.tab, t.n
        r = dict(best_metric=torch.full((tab.R, NP), 7, dtype=torch.int32, device="cuda:0"), best_entry=torch.full((tab.R, NP), 7, dtype=torch.int32, device="cuda:0"),
                 nexthop_mask=torch.full((tab.R, NP, tab.W), 7, dtype=torch.int64, device="cuda:0"))
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        self.ctx.routes_device(tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), t.ptr, t.vertex, t.metric, flags=t.flags,
                               **{k + "_ptr": x.data_ptr() for k, x in r.items()})
        for i, rr in enumerate(self.model.root_row):
            w = self.model.routes(i, t)
            for k, x in r.items():
                assert np.array_equal(x[rr].cpu().numpy().view(getattr(w, k).dtype), getattr(w, k)), ("routes", i, k)
        return r

    def repairs(self, lfa_flags=0):
        """hspf_lfa_srlg_device, hspf_rlfa_srlg_device and hspf_tilfa_device on the device; {ti_*: host array [n_prot, S]}."""
        lf = lfa_flags & ~BS.SAFE_REPAIRS
        if lf not in self._ti:
            alt = run_lfa_srlg(self.ctx, self.tab, self.protect, self.srlgs, lf, masks=False)["alt_flags"]
            _, dev_t, dev_alt = run_rlfa_srlg(self.ctx, self.tab, self.protect, self.srlgs, lf, True, alt, keep=True)
            self._ti[lf] = run_tilfa_on(self.ctx, self.tab, self.protect, dev_t, dev_alt, lf)
        return self._ti[lf]

    def backup(self, t: B.Table, lfa_flags=0, remote=True, masks=True, routes=None, tilfa=None, srlgs=None, plain=False):
        """routes_device, then routes_backup_srlg_device (plain: routes_backup_device); {field: host array [n_prot, ...]}."""
        import torch
        tab, P, NP = self.tab, len(self.model.prot), t.n
        r = routes or self.routes(t)
        shapes = dict(bk_kind=(P, NP), bk_primary=(P, NP), bk_slot=(P, NP), bk_metric=(P, NP), bk_flags=(P, NP), bk_cand_mask=(P, NP, tab.W),
                      bk_node_mask=(P, NP, tab.W), bk_coverage=(P, 7 if plain else 10))
        out = {k: torch.full(sh, 7, dtype=_torch_dt(OUT[k]), device="cuda:0") for k, sh in shapes.items() if masks or not k.endswith("_mask")}
        ti = None
        if remote:
            src = tilfa if tilfa is not None else self.repairs(lfa_flags)
            ti = [torch.from_numpy(np.ascontiguousarray(src[k]).view(np.uint8 if k == "ti_kind" else np.int32)).to("cuda:0") for k in TI]
        args = (tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), self.protect)
        kw = dict(routes=tuple(r[k].data_ptr() for k in ("best_metric", "best_entry", "nexthop_mask")), flags=t.flags, lfa_flags=lfa_flags,
                  **{k + "_ptr": x.data_ptr() for k, x in out.items()})
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        if plain:
            self.ctx.routes_backup_device(*args, t.ptr, t.vertex, t.metric, tilfa=None if ti is None else tuple(x.data_ptr() for x in ti[:3]), **kw)
        else:
            self.ctx.routes_backup_srlg_device(*args, srlgs or self.srlgs, t.ptr, t.vertex, t.metric, tilfa=None if ti is None else tuple(x.data_ptr() for x in ti), **kw)
        return {k: (out[k].cpu().numpy().view(OUT[k]) if k in out else None) for k in shapes}


def assert_equal(got, wants, masks=True, tag=""):
    for i, w in enumerate(wants):
        for name in BS.FIELDS:
            if not masks and name.endswith("_mask"):
                assert got[name] is None
                continue
            g, x = got[name][i], getattr(w, name)
            assert g.shape == x.shape and g.dtype == x.dtype and np.array_equal(g, x), (tag, i, name, np.argwhere(g != x)[:8].tolist(), g[g != x][:8], x[g != x][:8])


def check(ctx, model, lfa_flags=(0, BS.SAFE_REPAIRS), remotes=(True, False), need=None):
    """The model's protected roots and table on the device, for every lfa_flags with and without the repairs."""
    if need is not None:
        need(model.want(lfa_flags[0], remotes[0]))              # non-vacuity: on the MODEL, before anything is compared
    d = Device(ctx, model)
    try:
        r = d.routes(model.table)
        for lf in lfa_flags:
            for rem in remotes:
                if rem:                                          # the repairs the kernel reads are the model's
                    for i, x in enumerate(model.frr(lf)):
                        for k in TI:
                            assert np.array_equal(d.repairs(lf)[k][i], getattr(x[2], k)), ("tilfa", k)
                assert_equal(d.backup(model.table, lf, rem, routes=r), model.want(lf, rem), tag=(lf, rem))
    finally:
        d.free()


def random_table(r, nr, n_pfx, lo=0, hi=16):
    return B.table([[(int(v), int(r.integers(lo, hi))) for v in r.choice(nr, size=int(r.choice([1, 2, 2, 3])), replace=False)] for _ in range(n_pfx)])


def some_refused(wants):
    assert sum(int(w.bk_coverage[8]) for w in wants) > 0 and sum(int(w.bk_coverage[7]) for w in wants) > 0


def test_ring_with_chords_a_prefix_on_two_routers(spf_ctx):
    g, S, (gp, gr), t = SC.ring()
    m = SC.Model(g, [S], gp, gr, t)
    check(spf_ctx, m, lfa_flags=(0, BS.SAFE_REPAIRS, M.IGNORE_OVERLOAD), need=some_refused)
    assert m.want(0)[0].bk_kind[6] == B.NOTHING and m.want(BS.SAFE_REPAIRS)[0].bk_kind[6] == B.NODE


def hub_case(k, seed=1):
    g = hub(k, HUB_SEEDS[k])
    r = np.random.default_rng(seed)
    return g, SC.random_groups(g, 0, n_groups=(3, 7), per_group=(2, 6), root=0), random_table(r, k + 1, 60)      # (group seed 0: chosen on the CPU)


@pytest.mark.parametrize("k", [8, 9, 17, 65])
def test_hub_root_chunk_edge_and_mask_words(spf_ctx, k):
    g, (gp, gr), t = hub_case(k)
    m = SC.Model(g, [0], gp, gr, t)

    def need(w):
        assert int(np.count_nonzero(m.cands[0].nbr != M.NONE)) == k and m.W == (1 if k <= 64 else 2)
        some_refused(w)
        assert any(int(x) >> ((k - 1) % 64) & 1 for x in w[0].bk_cand_mask[:, (k - 1) // 64])            # the last slot of the last chunk is a candidate
    check(spf_ctx, m, need=need)


def test_a_primary_with_16_members_and_one_with_1(spf_ctx):
    """The hub of 17: slot 8 (the primary of most prefixes of the table) shares a group with 16 links among the neighbours, slot 15
    with one.  The draw (seed 0) was chosen on the CPU so that the 16-member primary refuses something."""
    g = hub(17, 3)
    rp, col = g[0], g[1]
    far = [l for u in range(1, 18) for l in range(int(rp[u]), int(rp[u + 1])) if int(col[l]) != 0]
    pick = [int(x) for x in np.random.default_rng(0).choice(far, 17, replace=False)]
    of = {int(rp[0]) + 8: [1], int(rp[0]) + 15: [2], pick[16]: [2]}
    for l in pick[:16]:
        of.setdefault(l, []).append(1)
    gp, gr = SM.groups_csr(len(col), of)
    m = SC.Model(g, [0], gp, gr, random_table(np.random.default_rng(5), 18, 70))

    def need(w):
        sizes = np.diff(m.mems[0].mem_ptr)
        assert sizes[8] == SM.MAX_MEMBERS == 16 and sizes[15] == 1
        prim = w[0].bk_primary
        assert ((prim == 8) & (w[0].bk_flags & BS.SRLG_REFUSED != 0)).any() and (prim == 15).any()
    check(spf_ctx, m, need=need)


def test_a_primary_with_9_members_takes_the_second_member_stream(spf_ctx):
    """The hub of 17 again: slot 8 shares a group with 9 links among the neighbours — one more than a stream of the prefix's entries
    carries, so members 8 .. 15 take their own.  The draw (seed 0) was chosen on the CPU so that the primary refuses something."""
    g = hub(17, 3)
    rp, col = g[0], g[1]
    far = [l for u in range(1, 18) for l in range(int(rp[u]), int(rp[u + 1])) if int(col[l]) != 0]
    of = {int(rp[0]) + 8: [1]}
    for l in np.random.default_rng(0).choice(far, 9, replace=False):
        of.setdefault(int(l), []).append(1)
    gp, gr = SM.groups_csr(len(col), of)
    m = SC.Model(g, [0], gp, gr, random_table(np.random.default_rng(5), 18, 70))

    def need(w):
        assert np.diff(m.mems[0].mem_ptr)[8] == 9
        assert ((w[0].bk_primary == 8) & (w[0].bk_flags & BS.SRLG_REFUSED != 0)).any() and (w[0].bk_kind == B.ECMP).any()
    check(spf_ctx, m, need=need)


@pytest.mark.parametrize("n_pfx", [255, 256, 300])
def test_prefix_counts_at_the_tile_edge(spf_ctx, n_pfx):
    g = ring_chords(24, 11, 1, 6, chords=6)
    gp, gr = SC.random_groups(g, 77, n_groups=(4, 5), per_group=(3, 6), root=0)
    m = SC.Model(g, [0], gp, gr, random_table(np.random.default_rng(n_pfx), 24, n_pfx))

    def need(w):
        some_refused(w)
        assert w[0].bk_kind[n_pfx - 1] >= B.ECMP                                                   # the last lane of the last tile has sets
    check(spf_ctx, m, remotes=(True,), need=need)


def test_advertiser_lists_empty_long_and_an_overloaded_neighbours_own_entry(spf_ctx):
    ring = [(v, (v + 1) % 6, 1) for v in range(6)]
    links = M.both(ring + [(0, 3, 2), (1, 4, 1)] + [(6 + i, 6 + i + 1, 1) for i in range(39)] + [(2, 6, 1)])
    g = M.csr(46, links, no_transit=[3])
    gp, gr = SC.group(g, (0, 1), (3, 2))
    t = B.table([[], [(v, 1 + v % 3) for v in range(6, 46)], [(3, 0), (2, 9)], [(2, 0), (3, 1)], [(5, 0), (3, 2)], [(3, 1)]])
    m = SC.Model(g, [0], gp, gr, t)

    def need(w):
        assert w[0].bk_kind[0] == B.NO_ROUTE and w[0].bk_kind[1] >= B.ECMP
        k3 = m.slot(3)
        plain = C.Model(g, [0], t).want(0)[0]
        # N = 3 itself advertises, on an overloaded N: admitted through its own entry — for prefix 3 one of its shortest paths is
        # 3 -> 2, the member (refused); prefix 4's primary has no member (kept)
        assert plain.own_exception == 2 and all(int(plain.bk_cand_mask[p, 0]) >> k3 & 1 for p in (3, 4))
        assert not int(w[0].bk_cand_mask[3, 0]) >> k3 & 1 and w[0].bk_flags[3] & BS.SRLG_REFUSED and int(w[0].bk_cand_mask[4, 0]) >> k3 & 1
    check(spf_ctx, m, lfa_flags=(0, M.IGNORE_OVERLOAD, BS.SAFE_REPAIRS), need=need)


def test_three_protected_roots_share_one_table_set(spf_ctx):
    g = ring_chords(20, 4, 1, 5, chords=6)
    gp, gr = SC.random_groups(g, 3, n_groups=(5, 7), per_group=(3, 6))
    m = SC.Model(g, [0, 7, 13], gp, gr, random_table(np.random.default_rng(2), 20, 50))

    def need(w):
        assert all(int(x.bk_coverage[7]) for x in w) and sum(int(x.bk_coverage[8]) for x in w)
    check(spf_ctx, m, need=need)


@pytest.mark.parametrize("flags", [B.PFX_SATURATING, B.PFX_LAST_MIN, B.PFX_SATURATING | B.PFX_LAST_MIN])
def test_saturating_and_last_min_tables(spf_ctx, flags):
    g, S, (gp, gr), t = SC.ring()
    big = 0xFFFFFFFE
    lists = [[(v, big)] for v in range(6)] + [[(2, big), (3, big + 1)], [(2, 2), (3, 3)], [(1, 1), (5, 1)], [(2, 0), (3, 3)]]
    m = SC.Model(g, [S], gp, gr, B.table(lists, flags))

    def need(w):
        some_refused(w)
        if flags & B.PFX_SATURATING:                                                              # a saturated sum is a number: the route exists
            assert m.routes(0).best_metric[3] == 0xFFFFFFFF and m.routes(0).best_entry[3] != M.NONE and w[0].bk_kind[3] >= B.ECMP
    check(spf_ctx, m, need=need)


def test_a_pair_whose_forced_link_is_a_member_is_refused(spf_ctx):
    g, S, (gp, gr), t = SC.ring()
    m = SC.Model(g, [S], gp, gr, t)
    e = m.slot(1)
    ti = m.frr(0)[0][2]
    forged = {k: np.array(getattr(ti, k))[None].copy() for k in TI}
    forged["ti_kind"][0, e], forged["ti_p"][0, e], forged["ti_link"][0, e] = 2, 3, SM.link_pos(g, 3, 2) - int(g[0][3])

    class Forged:
        pass
    f = Forged()
    for k in TI:
        setattr(f, k, forged[k][0])
    d = Device(spf_ctx, m)
    try:
        for lf in (0, BS.SAFE_REPAIRS):
            want = m.want(lf, tilfa=[f])
            assert (want[0].bk_coverage[9] > 0) == bool(lf) and (not lf or want[0].bk_kind[6] == B.NOTHING)
            assert_equal(d.backup(t, lf, True, tilfa=forged), want, tag=lf)
        forged["ti_link"][0, e] += 1                                                                # the other link of 3's row: accepted
        f.ti_link = forged["ti_link"][0]
        want = m.want(BS.SAFE_REPAIRS, tilfa=[f], table=B.table([[(2, 0), (3, 3)]]))
        assert want[0].bk_kind[0] == B.PAIR and not want[0].bk_coverage[9]
        assert_equal(d.backup(B.table([[(2, 0), (3, 3)]]), BS.SAFE_REPAIRS, True, tilfa=forged), want)
    finally:
        d.free()


def test_masks_null_changes_nothing_else(spf_ctx):
    g, S, (gp, gr), t = SC.random_case(SC.RANDOM_SEED + 3)
    m = SC.Model(g, [S], gp, gr, t)
    d = Device(spf_ctx, m)
    try:
        assert_equal(d.backup(t, BS.SAFE_REPAIRS, True, masks=False), m.want(BS.SAFE_REPAIRS), masks=False)
    finally:
        d.free()


@pytest.mark.parametrize("seed", [SC.RANDOM_SEED, SC.RANDOM_SEED + 1])
def test_empty_member_tables_equal_the_plain_call_on_the_device(spf_ctx, seed):
    g, S, (gp, gr), t = SC.random_case(seed)
    m = SC.Model(g, [S], gp, gr, t, no_members=True)
    d = Device(spf_ctx, m)
    try:
        r = d.routes(t)
        for lf in (0, BS.SAFE_REPAIRS, M.IGNORE_OVERLOAD):
            for rem in (True, False):
                got = d.backup(t, lf, rem, routes=r)
                plain = d.backup(t, lf & ~BS.SAFE_REPAIRS, rem, routes=r, plain=True)
                for name in BS.FIELDS[:-1]:
                    assert np.array_equal(got[name], plain[name]), (name, lf, rem)
                assert np.array_equal(got["bk_coverage"][:, :7], plain["bk_coverage"]) and not got["bk_coverage"][:, 7:].any()
                assert_equal(got, m.want(lf, rem))
    finally:
        d.free()


def test_backup_routes_end_to_end_with_groups(spf_ctx):
    from holo_amd import engine as E
    g, S, (gp, gr), t = SC.ring()
    m = SC.Model(g, [S], gp, gr, t)
    G = spf_ctx.upload(*g, 0xFFFFFFFF)
    try:
        for repairs in (False, True):
            res = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), srlg=(gp, gr), srlg_repairs=repairs)
            w = m.want(BS.SAFE_REPAIRS if repairs else 0)[0]
            for name in BS.FIELDS:
                assert np.array_equal(getattr(res, name)[0], getattr(w, name)), (name, repairs)
            assert np.array_equal(res.srlg.mem_ptr, m.mems[0].mem_ptr) and res.tilfa is not None
        res = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), srlg=(gp, gr), remote=False)
        assert_equal({k: getattr(res, k) for k in BS.FIELDS}, m.want(0, False))
        plain = spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric))                             # the default path: the chord, unchanged
        assert plain.bk_kind[0, 6] == E.BK_LFA and plain.bk_coverage.shape == (1, 7) and plain.srlg is None
        for kw in (dict(lan_protect=True), dict(node_protect=True)):
            with pytest.raises(ValueError, match="srlg excludes"):
                spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), srlg=(gp, gr), **kw)
        with pytest.raises(ValueError, match="srlg_repairs needs"):
            spf_ctx.backup_routes(G, S, (t.ptr, t.vertex, t.metric), srlg_repairs=True)
    finally:
        G.free()


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    import torch
    from holo_amd import _lib as L
    from holo_amd import engine as E
    g, S, (gp, gr), t = SC.ring()
    m = SC.Model(g, [S], gp, gr, t)
    d = Device(spf_ctx, m)
    try:
        r = d.routes(t)
        tab, NP = d.tab, t.n
        out = {k: torch.full((1, NP) + ((tab.W,) if k.endswith("_mask") else ()), 7, dtype=_torch_dt(OUT[k]), device="cuda:0") for k in OUT if k != "bk_coverage"}
        out["bk_coverage"] = torch.full((1, 10), 7, dtype=torch.int32, device="cuda:0")
        lib = L.load()
        parr, pkeep = spf_ctx._protect_array(d.protect, "t")
        u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))      # noqa: E731
        mem = m.mems[0]
        cols = {k: np.ascontiguousarray(getattr(mem, k), np.uint32) for k in ("mem_ptr", "tail", "pos", "head", "cost", "tail_row", "head_row")}

        def call(srlg_cols=cols, srlg_null=False, pt=None, routes=r, ti=None, bk=out, dist=tab.dist.data_ptr(), n_rows=tab.R):
            s = (L.HspfSrlg * 1)()
            s[0] = L.HspfSrlg(*(None if srlg_cols[k] is None else u32(srlg_cols[k]) for k in cols))
            pt = pt or L.HspfPrefixTable(t.n, len(t.vertex), u32(t.ptr), u32(t.vertex), u32(t.metric), 0, None, None, None, None)
            rr = L.HspfRoutes(*(routes[k].data_ptr() if routes[k] is not None else None for k in ("best_metric", "best_entry", "nexthop_mask")))
            o = L.HspfBackupOut(*(bk[k].data_ptr() if bk[k] is not None else None for k in ("bk_kind", "bk_primary", "bk_slot", "bk_metric", "bk_flags",
                                                                                           "bk_cand_mask", "bk_node_mask", "bk_coverage")))
            rc = lib.hspf_routes_backup_srlg_device(spf_ctx.handle, tab.n, n_rows, tab.W, dist or None, tab.flags.data_ptr(), tab.mask.data_ptr(), parr,
                                                    None if srlg_null else s, 1, 0, ctypes.byref(pt), ctypes.byref(rr), None if ti is None else ctypes.byref(ti),
                                                    ctypes.byref(o))
            return rc, spf_ctx.last_error()

        def bad_col(name, fn):
            c = dict(cols)
            c[name] = None if fn is None else fn(cols[name].copy())
            return call(srlg_cols=c)

        def edit(a, i, v):
            a[i] = v
            return a
        K = len(m.cands[0].nbr)
        e_slot = int(np.flatnonzero(np.diff(mem.mem_ptr))[0])
        many = dict(cols, mem_ptr=np.array([0] + [17] * K, np.uint32), **{k: np.zeros(17, np.uint32) for k in list(cols)[1:]})
        ti_bad = L.HspfTilfaOut(out["bk_kind"].data_ptr(), None, None, out["bk_slot"].data_ptr(), None, out["bk_metric"].data_ptr(), None, None, None)
        cases = [
            call(srlg_null=True), bad_col("mem_ptr", None), bad_col("head_row", None),
            bad_col("mem_ptr", lambda a: edit(a, e_slot + 1, 0) if e_slot else edit(a, 0, 5)),
            call(srlg_cols=many),
            bad_col("tail", lambda a: edit(a, 0, tab.n)), bad_col("head", lambda a: edit(a, 0, tab.n)),
            bad_col("tail_row", lambda a: edit(a, 0, tab.R)), bad_col("head_row", lambda a: edit(a, 0, tab.R)),
            call(dist=0), call(routes=dict(r, best_entry=None)), call(bk=dict(out, bk_flags=None)), call(bk=dict(out, bk_coverage=None)),
            call(ti=ti_bad), call(n_rows=0),
            call(pt=L.HspfPrefixTable(t.n, len(t.vertex), u32(t.ptr), u32(t.vertex), u32(t.metric), B.PFX_ORDERED, None, None, None, None)),
            call(pt=L.HspfPrefixTable(t.n, len(t.vertex), None, u32(t.vertex), u32(t.metric), 0, None, None, None, None)),
            call(pt=L.HspfPrefixTable(t.n, len(t.vertex), u32(t.ptr), u32(np.full(len(t.vertex), tab.n, np.uint32)), u32(t.metric), 0, None, None, None, None)),
        ]
        for i, (rc, err) in enumerate(cases):
            assert rc == -1 and "hspf_routes_backup_srlg_device" in err, (i, rc, err)
        for x in out.values():                                                                       # nothing was launched: every 7 is still there
            assert bool((x == 7).all())
        rc, _ = call()
        assert rc == 0 and not bool((out["bk_kind"] == 7).any())
        del pkeep
        assert E.BK_SRLG_COVERAGE_WORDS == 10
    finally:
        d.free()
