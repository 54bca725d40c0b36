"""hspf_tilfa_pc_device on the GPU against the plain-Python model (tests/_tilfa_pc_model.py) over the CPU oracle's tables: every
output array, bit for bit.  The tables the kernels read are the engine's own — hspf_run_device on the forward and the transposed
upload, the space tables of hspf_rlfa_device, the rows of hspf_run_failures_device — and each of them is compared with its model
first; the expected values never touch the engine."""
import ctypes

import numpy as np
import pytest

import _failure_cases as F
import _lfa_model as M
import _tilfa_pc_cases as C
import _tilfa_pc_model as P
from _tilfa_pc_cases import ring_chords, sweep_graph
from test_gpu_rlfa import Tables

pytestmark = pytest.mark.gpu

SHAPES = dict(tp_kind=(1, "uint8"), tp_p=(1, "int32"), tp_via=(1, "int32"), tp_q=(1, "int32"), tp_n_adj=(1, "uint8"), tp_hop_pos=(4, "int32"),
              tp_hop_head=(4, "int32"), tp_metric=(1, "int32"), tp_flags=(1, "uint8"))


def host(d):
    import torch
    return {k: x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in d.items()}


def out_buffers(P_, n, fill=7):
    """The output arrays with every BYTE set to `fill`."""
    import torch
    dev = torch.device("cuda:0")
    val = lambda dt: fill if dt == "uint8" else fill * 0x01010101      # noqa: E731
    t = {k: torch.full((P_, n) if w == 1 else (P_, n, w), val(dt), dtype=getattr(torch, dt), device=dev) for k, (w, dt) in SHAPES.items()}
    t["tp_coverage"] = torch.full((P_, 12), val("int32"), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    return t


def run_pc(ctx, tab, protect, wants, run_flags=0, lfa_flags=0, alt_flags=None, max_walk=256, drops=None):
    """rlfa_device with the space tables, ONE run_failures_device for the candidate slots of every protected root, tilfa_pc_device.
    wants: the model of each protected root (the inputs are held to it).  Returns {field: host array [P, ...]}."""
    import torch
    dev = torch.device("cuda:0")
    NP, n, S = len(protect), tab.n, 64 * tab.W
    full = lambda shape, dt: torch.full(shape, 7, dtype=dt, device=dev)      # noqa: E731
    r = dict(pq_node=full((NP, S), torch.int32), pq_via=full((NP, S), torch.int32), pq_metric=full((NP, S), torch.int32), pq_counts=full((NP, S, 4), torch.int32),
             space_flags=full((NP, S, n), torch.uint8), space_via=full((NP, S, n), torch.int32), rl_node=full((NP, n), torch.int32),
             rl_via=full((NP, n), torch.int32), rl_coverage=full((NP, 4), torch.int32))
    alt = torch.from_numpy(np.ascontiguousarray(alt_flags)).to(dev) if alt_flags is not None else None
    ap = 0 if alt is None else alt.data_ptr()
    tables = (tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr())
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.rlfa_device(tab.G, tab.R, tab.W, *tables, protect, alt_flags_in_ptr=ap, lfa_flags=lfa_flags, **{k + "_ptr": x.data_ptr() for k, x in r.items()})
    hr = host(r)
    roots, fails, pc_row = [], [], np.full((NP, S), 0xFFFFFFFF, np.uint32)
    for i, (_, pc, _) in enumerate(protect):
        for e in np.flatnonzero(pc.nbr != 0xFFFFFFFF):
            if drops and int(e) in drops[i]:
                continue
            pc_row[i, e] = len(roots)
            roots.append(pc.root)
            fails.append((F.ROOT_LINK, int(pc.root_link[e])))
    pcd = full((max(len(roots), 1), n), torch.int32)
    if roots:
        ctx.run_failures_device(tab.G, roots, fails, run_flags, dist_ptr=pcd.data_ptr())
    hp = pcd.cpu().numpy().view(np.uint32)
    for i, w in enumerate(wants):
        assert np.array_equal(hr["space_flags"][i], w.rl.space_flags) and np.array_equal(hr["space_via"][i], w.rl.space_via), ("spaces", i)
        for e, row in w.pc.items():
            assert np.array_equal(hp[pc_row[i, e]], row), ("post-convergence row", i, e)
    t = out_buffers(NP, n)
    ctx.tilfa_pc_device(tab.G, tab.R, tab.W, *tables, protect, space_flags_ptr=r["space_flags"].data_ptr(), space_via_ptr=r["space_via"].data_ptr(),
                        pc_dist_ptr=pcd.data_ptr(), n_pc_rows=len(roots), pc_row=pc_row, max_walk=max_walk, run_flags=run_flags, alt_flags_in_ptr=ap,
                        lfa_flags=lfa_flags, **{k + "_ptr": x.data_ptr() for k, x in t.items()})
    return host(t)


def assert_equal(got, want: P.TilfaPc, i=0, tag=""):
    for name in P.FIELDS:
        g, w = got[name][i], getattr(want, name)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:8].tolist(), g[g != w][:8], w[g != w][:8])
    assert got["tp_coverage"][i].tolist() == P.recount(got["tp_kind"][i], got["tp_n_adj"][i]), tag      # the device's counts are its own arrays'


def check_want(ctx, w: P.Want, lfa_flags=0, with_lfa=False, max_walk=256, drop=(), tag=""):
    from holo_amd import engine as E
    pc = E.lfa_candidates(*w.graph, w.root)
    assert np.array_equal(pc.nbr, w.cand.nbr) and np.array_equal(pc.root_link, w.cand.root_link)
    tab = Tables(ctx, w.graph, w.maxp, w.roots, w.run_flags, w.W)
    try:
        got = run_pc(ctx, tab, [(0, pc, w.nbr_row)], [w], w.run_flags, lfa_flags, w.lfa.alt_flags[None, :] if with_lfa else None, max_walk, [set(drop)])
    finally:
        tab.free()
    assert_equal(got, w.tp, tag=tag)
    return got


@pytest.mark.parametrize("w_min", [1, 2])
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_hand_case(spf_ctx, name, w_min):
    c = C.CASES[name]
    w = c.want(w_min)
    assert w.W == w_min
    C.check_expect(w.tp, c.expect, name)                       # the model shows what the case is for
    got = check_want(spf_ctx, w, c.lfa_flags, False, c.max_walk, c.drop, tag=name)

    class One:
        pass
    one = One()
    for k in P.FIELDS:
        setattr(one, k, got[k][0])
    C.check_expect(one, c.expect, name)


@pytest.mark.parametrize("seed", range(40))
def test_random_graphs(spf_ctx, seed):
    """Three roots per graph; odd (seed + root) pass the alt_flags of the LFA model, the others none (every destination is walked)."""
    g = sweep_graph(seed)
    n = len(g[3])
    assert 30 <= n <= 60
    for pick in range(3):
        root = (seed * 11 + pick * 17) % n
        with_lfa = bool((seed + pick) % 2)
        check_want(spf_ctx, P.one_root(g, root, with_lfa=with_lfa), 0, with_lfa, tag=(seed, pick))


def test_protocol_instances(spf_ctx):
    """40 instances of the IS-IS / OSPF generators of the failure-row tests (LANs, overload bits, zero metrics, the run flags of the
    protocol), one root each."""
    kinds = set()
    for seed in range(40):
        graph, maxp, run_flags = F.protocol_graph(seed)
        routers = np.flatnonzero((graph[3] & 1) == 0)
        lf = M.IGNORE_OVERLOAD if run_flags & 2 else 0
        w = P.one_root(graph, int(routers[(seed * 7) % len(routers)]), maxp, run_flags, lf, with_lfa=bool(seed % 2))
        kinds |= set(w.tp.tp_kind.tolist())
        check_want(spf_ctx, w, lf, bool(seed % 2), tag=seed)
    assert {P.D_LFA, P.D_REPAIR, P.D_NONE, P.D_LAN} <= kinds


def test_ring_of_300_two_workgroups(spf_ctx):
    """Destinations, parents and p / q on both sides of vertex 256; costs per direction, so that adjacencies are needed."""
    w = P.one_root(ring_chords(300, 5, 1, 9, chords=6, asym=True), 150, max_walk=512)
    k = w.tp.tp_kind
    assert (k[:256] == P.D_REPAIR).any() and (k[256:] == P.D_REPAIR).any() and (w.tp.tp_n_adj > 0).any()
    rep = np.flatnonzero(k == P.D_REPAIR)
    assert ((rep < 256) != (w.tp.tp_p[rep] < 256)).any()                          # a walk crosses the tile edge
    check_want(spf_ctx, w, with_lfa=True, max_walk=512)


def test_walk_cap_on_a_long_path(spf_ctx):
    """A 300-ring, S = 0: the post-convergence path of the far neighbour visits 150 vertices before it meets P; max_walk 100 cuts
    those walks (_D_WALK) and leaves the short ones."""
    g = ring_chords(300, 1, 1, 1, chords=0)
    w = P.one_root(g, 0, max_walk=100, with_lfa=False)
    assert (w.tp.tp_kind == P.D_WALK).any() and (w.tp.tp_kind == P.D_REPAIR).any()
    check_want(spf_ctx, w, max_walk=100)
    w = P.one_root(g, 0, max_walk=400, with_lfa=False)
    assert not (w.tp.tp_kind == P.D_WALK).any()
    check_want(spf_ctx, w, max_walk=400)


class PatchedTables(Tables):
    """Tables of a graph that was uploaded as `graph` and then lost a link through ONE structural hspf_graph_patch."""

    def __init__(self, ctx, graph, root):
        import torch
        from holo_amd import engine as E
        dev = torch.device("cuda:0")
        self.G = ctx.upload(*graph, 0xFFFFFFFF)
        self.GT = None
        try:
            self.g2, did = F.drop_last_link(self.G, graph)
            assert did and self.G.export("build_mode")[0] == 3             # the incremental path: the link arrays are the other set now
            self.want = w = P.one_root(self.g2, root)
            self.n, self.R, self.W = len(graph[3]), len(w.roots), w.W
            self.dist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
            self.flags = torch.empty((self.R, self.n), dtype=torch.int16, device=dev)
            self.mask = torch.empty((self.R, self.n, self.W), dtype=torch.int64, device=dev)
            self.rdist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
            ctx.run_device(self.G, w.roots, 0, dist_ptr=self.dist.data_ptr(), flags_ptr=self.flags.data_ptr(), mask_ptr=self.mask.data_ptr(), mask_words=self.W)
            self.GT = ctx.upload(*E.csr_transpose(*self.g2), self.g2[3], 0xFFFFFFFF)
            ctx.run_device(self.GT, w.roots, 0, dist_ptr=self.rdist.data_ptr())
        except BaseException:
            self.free()
            raise


def test_after_structural_patch(spf_ctx):
    """One structural hspf_graph_patch between the upload and the calls: the in-link arrays the parents are read from are the
    swapped set."""
    from holo_amd import engine as E
    tab = PatchedTables(spf_ctx, ring_chords(60, 4, 1, 9, chords=8, asym=True), 30)
    try:
        w = tab.want
        assert (w.tp.tp_kind == P.D_REPAIR).any() and (w.tp.tp_n_adj > 0).any()
        got = run_pc(spf_ctx, tab, [(0, E.lfa_candidates(*tab.g2, 30), w.nbr_row)], [w], alt_flags=w.lfa.alt_flags[None, :])
    finally:
        tab.free()
    assert_equal(got, w.tp, tag="patched")


def test_two_protected_roots_and_a_missing_row(spf_ctx):
    """n_prot = 2 over one table set; the second root's first candidate slot gets no row: its destinations are _D_NONE."""
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    import _rlfa_model as R
    graph = ring_chords(40, 9, 1, 9, chords=3, asym=True)
    prot_roots = [0, 20]
    cands = [M.candidates(*graph, r) for r in prot_roots]
    rows = prot_roots + sorted({int(x) for c in cands for x in c.nbr if x != M.NONE} - set(prot_roots))
    roots, row_of = np.array(rows, np.uint32), {v: i for i, v in enumerate(rows)}
    W = go.mask_words(*graph, roots)
    fwd, rdist = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
    protect, wants, drops = [], [], [set(), {0}]
    for r, mc, drop in zip(prot_roots, cands, drops):
        nbr_row = np.array([row_of.get(int(x), 0) for x in mc.nbr], np.uint32)
        protect.append((row_of[r], E.lfa_candidates(*graph, r), nbr_row))
        rl = R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], mc, row_of[r], nbr_row, 0, None)
        pc = {e: x for e, x in P.pc_rows(graph, 0xFFFFFFFF, mc).items() if e not in drop}
        tp = P.tilfa_pc(fwd.dist, fwd.flags, fwd.mask, graph, mc, row_of[r], nbr_row, rl.space_flags, rl.space_via, pc)
        wants.append(P.Want(graph, r, 0xFFFFFFFF, 0, mc, roots, nbr_row, W, fwd, rdist, None, rl, pc, tp))
    assert all((w.tp.tp_kind == P.D_REPAIR).any() for w in wants) and (wants[1].tp.tp_kind == P.D_NONE).any()
    assert not np.array_equal(wants[0].tp.tp_p, wants[1].tp.tp_p)
    tab = Tables(spf_ctx, graph, 0xFFFFFFFF, roots, 0, W)
    try:
        got = run_pc(spf_ctx, tab, protect, wants, drops=drops)
    finally:
        tab.free()
    for i, w in enumerate(wants):
        assert_equal(got, w.tp, i, tag=i)


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import _lib as L, engine as E
    import torch
    c = C.CASES["b_ring_one_adj"]
    w = c.want()
    n, S = 5, 64
    pc = E.lfa_candidates(*w.graph, w.root)
    protect = [(0, pc, w.nbr_row)]
    tab = Tables(spf_ctx, w.graph, w.maxp, w.roots, 0, 1)
    try:
        good = run_pc(spf_ctx, tab, protect, [w])
        assert_equal(good, w.tp)
        dev = torch.device("cuda:0")
        sp_f = torch.from_numpy(w.rl.space_flags[None]).to(dev)
        sp_v = torch.from_numpy(w.rl.space_via[None].view(np.int32)).to(dev)
        slots = sorted(w.pc)
        pcd = torch.from_numpy(np.stack([w.pc[e] for e in slots]).view(np.int32)).to(dev)
        pc_row = np.full((1, S), 0xFFFFFFFF, np.uint32)
        pc_row[0, slots] = np.arange(len(slots))
        out = out_buffers(1, n, fill=0x5A)
        tables = dict(dist=tab.dist.data_ptr(), flags=tab.flags.data_ptr(), mask=tab.mask.data_ptr(), rdist=tab.rdist.data_ptr())
        base = dict(space_flags_ptr=sp_f.data_ptr(), space_via_ptr=sp_v.data_ptr(), pc_dist_ptr=pcd.data_ptr(), n_pc_rows=len(slots), pc_row=pc_row,
                    max_walk=16, **{k + "_ptr": x.data_ptr() for k, x in out.items()})

        def untouched():
            return all((x.cpu().numpy().view(np.uint8) == 0x5A).all() for x in out.values())

        def expect_inval(protect_=None, **kw):
            t, p = dict(tables), dict(base)
            for k, v in kw.items():
                (t if k in t else p)[k] = v
            with pytest.raises(E.HspfError) as e:
                spf_ctx.tilfa_pc_device(tab.G, tab.R, 1, t["dist"], t["flags"], t["mask"], t["rdist"], protect_ or protect, **p)
            assert e.value.code == -1 and "hspf_tilfa_pc_device" in str(e.value), str(e.value)
            assert untouched()                                   # nothing was written: nothing was launched

        for k in tables:                                         # what hspf_tilfa_device rejects: NULL tables,
            expect_inval(**{k: 0})
        expect_inval(space_flags_ptr=0)
        expect_inval(space_via_ptr=0)
        for k in out:                                            # every output,
            expect_inval(**{k + "_ptr": 0})
        bad_row = w.nbr_row.copy()
        bad_row[slots[0]] = tab.R
        expect_inval(protect_=[(0, pc, bad_row)])                # nbr_row >= n_rows, root_row out of range, too many slots,
        expect_inval(protect_=[(tab.R, pc, w.nbr_row)])
        many = E.LfaCandidates(2, np.full(65, E.NO_ROOT, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint32), np.zeros(65, np.uint8))
        expect_inval(protect_=[(0, many, np.zeros(65, np.uint32))])
        expect_inval(pc_dist_ptr=0)                              # the new ones: NULL pc_dist / pc_row,
        expect_inval(pc_row=None)
        r2 = pc_row.copy()
        r2[0, len(pc.nbr)] = 0                                   # a row for a slot >= n_slots,
        expect_inval(pc_row=r2)
        nc = E.LfaCandidates(pc.root, pc.nbr.copy(), pc.cost, pc.root_link, pc.cflags)
        nc.nbr[slots[0]] = E.NO_ROOT                             # for a slot that is no candidate,
        expect_inval(protect_=[(0, nc, w.nbr_row)])
        r3 = pc_row.copy()
        r3[0, slots[0]] = len(slots)                             # a row >= n_pc_rows,
        expect_inval(pc_row=r3)
        expect_inval(max_walk=0)                                 # max_walk outside 1 .. 65535
        expect_inval(max_walk=65536)
        lib = L.load()
        arr, keep = spf_ctx._protect_array(protect, "test")
        o = L.HspfTilfaPcOut(*(out[k].data_ptr() for k in P.FIELDS))
        tb = tuple(tables.values())
        rest = (sp_f.data_ptr(), sp_v.data_ptr(), pcd.data_ptr(), len(slots), pc_row.ctypes.data_as(L.u32p), 0, 16)
        assert lib.hspf_tilfa_pc_device(spf_ctx.handle, None, n, tab.R, 1, *tb, arr, 1, 0, None, *rest, ctypes.byref(o)) == -1
        assert lib.hspf_tilfa_pc_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, *tb, None, 1, 0, None, *rest, ctypes.byref(o)) == -1
        assert lib.hspf_tilfa_pc_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, *tb, arr, 1, 0, None, *rest, None) == -1
        assert lib.hspf_tilfa_pc_device(spf_ctx.handle, tab.G.handle, n, tab.R, 1, *tb, arr, 0, 0, None, *rest, ctypes.byref(o)) == -1
        assert "hspf_tilfa_pc_device" in spf_ctx.last_error() and untouched()
        other = spf_ctx.upload(*C.CASES["a_p_in_q"].graph, 0xFFFFFFFF)      # a graph of another size than n_vertices
        try:
            assert lib.hspf_tilfa_pc_device(spf_ctx.handle, other.handle, n, tab.R, 1, *tb, arr, 1, 0, None, *rest, ctypes.byref(o)) == -1
            assert "hspf_tilfa_pc_device" in spf_ctx.last_error() and untouched()
        finally:
            other.free()
        del keep
        # and the context still works, on the buffers the refused calls left alone
        spf_ctx.tilfa_pc_device(tab.G, tab.R, 1, *tb, protect, **base)
        assert_equal(host(out), w.tp, tag="after the errors")
    finally:
        tab.free()


def test_tilfa_pc_convenience_end_to_end(spf_ctx):
    """SpfContext.tilfa_pc(): the chain of tilfa(), one run_failures_device() over the candidate slots, tilfa_pc_device(); equal to
    the step-by-step calls (which the tests above hold to the model) and to the model itself; segments() reads a repair."""
    graph = ring_chords(60, 4, 1, 9, chords=8, asym=True)
    root = 30
    w = P.one_root(graph, root)
    assert (w.tp.tp_kind == P.D_REPAIR).any() and (w.tp.tp_kind == P.D_LFA).any() and (w.tp.tp_n_adj > 0).any()
    steps = check_want(spf_ctx, w, with_lfa=True)
    G = spf_ctx.upload(*graph, 0xFFFFFFFF)
    try:
        cand, lfa, rl, ti, tp = spf_ctx.tilfa_pc(G, root)
        ti_only = spf_ctx.tilfa(G, root)[3]
    finally:
        G.free()
    assert np.array_equal(cand.nbr, w.cand.nbr) and np.array_equal(lfa.alt_flags[0], w.lfa.alt_flags)
    assert np.array_equal(ti.ti_kind, ti_only.ti_kind) and np.array_equal(ti.ti_metric, ti_only.ti_metric)
    for name in P.FIELDS:
        assert np.array_equal(getattr(tp, name), steps[name]), name
    D = int(np.flatnonzero((w.tp.tp_kind == P.D_REPAIR) & (w.tp.tp_n_adj > 0))[0])
    via, p, hops, q = tp.segments(D)
    rp, col = graph[0], graph[1]
    assert (via, p, q) == (int(w.tp.tp_via[D]), int(w.tp.tp_p[D]), int(w.tp.tp_q[D])) and hops[0][0] == p and hops[-1][2] == q
    assert all(int(col[rp[t] + j]) == h for t, j, h in hops) and all(a[2] == b[0] for a, b in zip(hops, hops[1:]))
    assert tp.segments(root) is None
