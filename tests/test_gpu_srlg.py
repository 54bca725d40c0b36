"""hspf_lfa_srlg_device and hspf_rlfa_srlg_device on the GPU against the model (tests/_srlg_model.py) over the CPU oracle's SPTs:
every output array, bit for bit; hspf_tilfa_device on the safe tables; with empty member lists every shared output against the
plain calls on the device.  Both table sets come from hspf_run_device (the forward graph and the product's transpose of it, root
list [S] + neighbour routers + member endpoints); the expected values never touch the engine.  Shapes: hand graphs, 8 / 9 / 17
candidate slots (the chunk of 8), a slot with 16 members, slots sharing members behind one link, 255 / 256 / 300 vertices (the
workgroup of 256), two mask words, three protected roots over one table set, a LAN with an overloaded router."""
import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _srlg_model as SM
import _tilfa_model as T
from test_gpu_lfa import mesh, run_lfa
from test_gpu_rlfa import Tables, ring_chords, run_rlfa
from test_gpu_rlfa_lan import run_tilfa_on

pytestmark = pytest.mark.gpu

NONE = M.NONE


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def product_members(mem):
    from holo_amd import engine as E
    return E.SrlgMembers(mem.mem_ptr, mem.tail, mem.pos, mem.head, mem.cost, mem.tail_row, mem.head_row)


def run_lfa_srlg(ctx, tab, protect, srlgs, lfa_flags=0, masks=True):
    """hspf_lfa_srlg_device, every output pre-filled with 7.  Returns {field: host array}."""
    torch, dev = _torch()
    P, n, W = len(protect), tab.n, tab.W
    full = lambda shape, dt: torch.full(shape, 7, dtype=dt, device=dev)      # noqa: E731
    t = dict(alt_slot=full((P, n), torch.int32), alt_metric=full((P, n), torch.int32), alt_flags=full((P, n), torch.uint8),
             cand_mask=full((P, n, W), torch.int64) if masks else None, node_mask=full((P, n, W), torch.int64) if masks else None,
             coverage=full((P, 7), torch.int32))
    ptr = lambda x: 0 if x is None else x.data_ptr()      # noqa: E731
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.lfa_srlg_device(n, tab.R, W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), protect, srlgs, alt_slot_ptr=ptr(t["alt_slot"]),
                        alt_metric_ptr=ptr(t["alt_metric"]), alt_flags_ptr=ptr(t["alt_flags"]), coverage_ptr=ptr(t["coverage"]),
                        cand_mask_ptr=ptr(t["cand_mask"]), node_mask_ptr=ptr(t["node_mask"]), lfa_flags=lfa_flags)
    view = {torch.uint8: np.uint8, torch.int32: np.uint32, torch.int64: np.uint64}
    return {k: None if x is None else x.cpu().numpy().view(view[x.dtype]) for k, x in t.items()}


def run_rlfa_srlg(ctx, tab, protect, srlgs, lfa_flags=0, spaces=True, alt_flags=None, keep=False, rdist=None):
    """hspf_rlfa_srlg_device, every output pre-filled with 7.  Returns {field: host array}; with `keep` also the device tensors."""
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
    ctx.rlfa_srlg_device(tab.G, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(),
                         (tab.rdist if rdist is None else rdist).data_ptr(), protect, srlgs,
                         pq_node_ptr=ptr(t["pq_node"]), pq_via_ptr=ptr(t["pq_via"]), pq_metric_ptr=ptr(t["pq_metric"]), pq_counts_ptr=ptr(t["pq_counts"]),
                         rl_node_ptr=ptr(t["rl_node"]), rl_via_ptr=ptr(t["rl_via"]), rl_coverage_ptr=ptr(t["rl_coverage"]),
                         space_flags_ptr=ptr(t["space_flags"]), space_via_ptr=ptr(t["space_via"]), alt_flags_in_ptr=ptr(alt), lfa_flags=lfa_flags)
    host = {k: None if x is None else x.cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in t.items()}
    return (host, t, alt) if keep else host


def plan(graph, protect_roots, gp, gr, no_members=False):
    """One table set for all protected roots: (roots of the run, per root (root_row, cand, nbr_row, members with rows))."""
    per, roots = [], []
    for s in protect_roots:
        c, rs, _, mem = SM.protect_one(*graph, s, gp, gr)
        per.append((c, mem))
        roots += [int(x) for x in rs if int(x) not in roots]
    row_of = {v: i for i, v in enumerate(roots)}
    out = []
    for c, mem in per:
        nbr_row = np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32)
        if no_members:
            mem = SM.empty_members(len(c.nbr))
        else:
            mem.tail_row = np.array([row_of[int(x)] for x in mem.tail], np.uint32)
            mem.head_row = np.array([row_of[int(x)] for x in mem.head], np.uint32)
        out.append((row_of[c.root], c, nbr_row, mem))
    return np.array(roots, np.uint32), out


def assert_fields(got, want, i, fields, tag):
    for name in fields:
        if got[name] is None:
            continue
        g, w = got[name][i], getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, i, name, np.argwhere(g != w)[:8].tolist())


def some_refused_and_lost(lfa, rl):
    assert sum(int(a.coverage[6]) for a in lfa) > 0 and sum(int(w.pq_counts[:, 4].sum()) for w in rl) > 0


def check(ctx, graph, protect_roots, gp, gr, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=(0,), need=some_refused_and_lost, w_min=1,
          variants=((True, True),), no_members=False, tilfa=True):
    """Device against model for every protected root and every lfa_flags; `variants`: (space tables and masks, alt_flags_in) pairs.
    Returns (LFA models, RLFA models) of the first lfa_flags."""
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    roots, per = plan(graph, protect_roots, gp, gr, no_members)
    W = max(go.mask_words(*graph, roots), max((len(c.nbr) + 63) // 64 for _, c, _, _ in per), w_min)
    fwd, rdist = R.tables(graph, maxp, roots, run_flags, W)
    if not no_members:                                       # the product's member lists are the model's
        for _, c, _, mem in per:
            pm = E.srlg_members(*graph, c.root, gp, gr)
            for name in ("mem_ptr", "tail", "pos", "head", "cost"):
                assert np.array_equal(getattr(pm, name), getattr(mem, name)), name
    first = None
    tab = Tables(ctx, graph, maxp, roots, run_flags, W)
    try:
        assert np.array_equal(tab.rdist.cpu().numpy().view(np.uint32), rdist)      # the reverse run itself
        protect = [(r, E.lfa_candidates(*graph, c.root), nr) for r, c, nr, _ in per]
        srlgs = [product_members(mem) for _, _, _, mem in per]
        for lf in lfa_flags:
            lfa = [SM.lfa(fwd.dist, fwd.flags, fwd.mask, c, r, nr, mem, lf) for r, c, nr, mem in per]
            if first is None and need is not None:
                need(lfa, [SM.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], c, r, nr, mem, lf, a.alt_flags) for (r, c, nr, mem), a in zip(per, lfa)])
            alt_flags = np.stack([a.alt_flags for a in lfa])
            for spaces, with_alt in variants:
                rl = [SM.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph[3], c, r, nr, mem, lf, a.alt_flags if with_alt else None)
                      for (r, c, nr, mem), a in zip(per, lfa)]
                if first is None:
                    first = (lfa, rl)
                got_l = run_lfa_srlg(ctx, tab, protect, srlgs, lf, masks=spaces)
                got, dev_t, alt = run_rlfa_srlg(ctx, tab, protect, srlgs, lf, spaces, alt_flags if with_alt else None, keep=True)
                for i in range(len(per)):
                    assert_fields(got_l, lfa[i], i, SM.LFA_FIELDS, ("lfa", lf, spaces))
                    assert_fields(got, rl[i], i, R.FIELDS, ("rlfa", lf, spaces, with_alt))
                if no_members:                                   # the plain calls on the same tables
                    pl = run_lfa(ctx, tab, protect, lf, masks=spaces)
                    for name, p in zip(SM.LFA_FIELDS, pl):
                        if name == "coverage":
                            assert np.array_equal(got_l[name][:, :5], p) and not got_l[name][:, 5:].any()
                        elif p is not None:
                            assert np.array_equal(got_l[name], p), name
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
                    for i, ((r, c, nr, _), w) in enumerate(zip(per, rl)):
                        wt = T.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, r, nr, w.space_flags, w.space_via, alt_flags[i])
                        for name in T.FIELDS:
                            assert np.array_equal(got_t[name][i], getattr(wt, name)), ("tilfa", lf, i, name)
                        assert np.array_equal(wt.ti_counts[:, 0], w.pq_counts[:, 3])
    finally:
        tab.free()
    return first


def slot_to(c, v, nth=0):
    return [k for k in range(len(c.nbr)) if c.nbr[k] == v][nth]


def group(graph, *links):
    """(grp_ptr, grp) with the given (u, v[, nth]) links in ONE group."""
    return SM.groups_csr(len(graph[1]), {SM.link_pos(graph, *l): [5] for l in links})


def random_groups(graph, root, seed, per_link=(1, 5), hops=2):
    """Every link of the root's row in a group of its own with `per_link` links drawn within `hops` of the root."""
    r = np.random.default_rng(seed)
    rp, col = graph[0], graph[1]
    hood = {root}
    for _ in range(hops):
        hood |= {int(x) for u in sorted(hood) for x in col[rp[u]:rp[u + 1]]}
    near = np.array([l for u in sorted(hood - {root}) for l in range(int(rp[u]), int(rp[u + 1]))])
    of = {}
    for j in range(int(rp[root + 1] - rp[root])):
        for l in r.choice(near, min(len(near), int(r.integers(*per_link))), replace=False):
            of.setdefault(int(l), []).append(100 + j)
        of.setdefault(int(rp[root]) + j, []).append(100 + j)
    return SM.groups_csr(len(col), of)


# ---- hand cases -----------------------------------------------------------------------------------------------------------

def test_ring_with_chords_the_only_lfa_shares_the_primarys_group(spf_ctx):
    """A 6-ring of unit costs, S = 0 with the chord 0 - 3 (cost 2), and 1 - 4 (cost 1).  For D = 1 and D = 2 the chord is the
    only alternate; link 3 -> 2, on its onward path to 2, shares the group of the primary 0 -> 1.  (On a 6-ring with the one
    chord alone every path into the far end ends on the same link, so no group on the chord's onward path refuses the chord and
    leaves a PQ node — tests/test_host_srlg.py searches it; the second chord is what gives the safe spaces a node.)"""
    ring = [(v, (v + 1) % 6, 1) for v in range(6)]
    g = M.csr(6, M.both(ring + [(0, 3, 2), (1, 4, 1)]))
    gp, gr = group(g, (0, 1), (3, 2))
    lfa, rl = check(spf_ctx, g, [0], gp, gr)
    c = M.candidates(*g, 0)
    e, k3 = slot_to(c, 1), slot_to(c, 3)
    assert lfa[0].plain.alt_slot[2] == k3 and lfa[0].alt_slot[2] == NONE
    assert (lfa[0].alt_flags[2] & SM.SRLG_REFUSED) and not (lfa[0].alt_flags[2] & M.LINK_PROTECT)
    assert rl[0].plain.pq_node[e] == 3 and rl[0].pq_node[e] == 4 and rl[0].rl_node[2] == 4


def test_local_member_refuses_the_neighbours_own_link(spf_ctx):
    g = M.csr(4, M.both([(0, 1, 1), (0, 2, 2), (1, 3, 1), (2, 3, 1), (1, 2, 5)]))
    gp, gr = group(g, (0, 1), (0, 2))                      # S's two links share a conduit
    lfa, rl = check(spf_ctx, g, [0], gp, gr, need=None)
    c = M.candidates(*g, 0)
    assert lfa[0].plain.alt_slot[1] == slot_to(c, 2) and lfa[0].alt_slot[1] == NONE and lfa[0].alt_flags[1] & SM.SRLG_REFUSED
    assert not (rl[0].space_flags[slot_to(c, 1)] & R.IN_XP).any()


def test_parallel_links_only_the_costlier_is_a_member_nothing_refused(spf_ctx):
    g = M.csr(4, M.both([(0, 1, 1), (0, 2, 1), (2, 3, 1)]) + M.both([(2, 3, 9), (1, 3, 3)]))
    gp, gr = group(g, (0, 1), (2, 3, 1))                   # the second, costlier 2 -> 3
    lfa, rl = check(spf_ctx, g, [0], gp, gr, need=None)
    assert not lfa[0].coverage[6] and lfa[0].coverage[5] and not rl[0].pq_counts[:, 4].any()
    assert np.array_equal(lfa[0].alt_slot, lfa[0].plain.alt_slot)


def test_member_no_row_reaches_refuses_nothing(spf_ctx):
    links = M.both([(0, 1, 1), (0, 2, 2), (1, 3, 1), (2, 3, 1)]) + [(4, 5, 1), (5, 4, 1)]      # 4 - 5: an island
    g = M.csr(6, links)
    gp, gr = group(g, (0, 1), (4, 5))
    lfa, rl = check(spf_ctx, g, [0], gp, gr, need=None)
    assert not lfa[0].coverage[6] and lfa[0].coverage[5] and not rl[0].pq_counts[:, 4].any()
    assert np.array_equal(lfa[0].alt_slot, lfa[0].plain.alt_slot) and np.array_equal(rl[0].pq_node, rl[0].plain.pq_node)


def test_member_with_head_s_and_member_with_tail_e(spf_ctx):
    g = ring_chords(10, 3, 1, 4, chords=3, asym=True)
    E = int(g[1][g[0][0]])                                  # the neighbour behind S's first link
    other = [int(x) for x in g[1][g[0][E]:g[0][E + 1]] if int(x) != 0][0]
    gp, gr = group(g, (0, E), (E, 0), (E, other))
    check(spf_ctx, g, [0], gp, gr, need=None)


# ---- shape limits -----------------------------------------------------------------------------------------------------------

def hub_mesh(k, seed):
    """Root 0 with k router neighbours on a sparse mesh (no parallel links)."""
    r = np.random.default_rng(seed)
    und = {(0, v): int(r.integers(1, 9)) for v in range(1, k + 1)}
    for v in range(1, k + 1):
        und.setdefault((v, v % k + 1) if v < v % k + 1 else (v % k + 1, v), int(r.integers(1, 9)))
    for _ in range(k):
        a, b = sorted(int(x) for x in r.integers(1, k + 1, 2))
        if a != b:
            und.setdefault((a, b), int(r.integers(1, 9)))
    return M.csr(k + 1, M.both([(a, b, c) for (a, b), c in sorted(und.items())]))


CHUNK_SEEDS = {8: 1, 9: 1, 17: 16}                       # seeds whose groups refuse an alternate and remove a PQ candidate (the check asserts it)


@pytest.mark.parametrize("k", [8, 9, 17])
def test_candidate_slots_at_the_chunk_edges(spf_ctx, k):
    g = hub_mesh(k, CHUNK_SEEDS[k])
    gp, gr = random_groups(g, 0, CHUNK_SEEDS[k])
    check(spf_ctx, g, [0], gp, gr, variants=((True, True), (False, False)))


def test_more_than_64_slots_take_the_word_by_word_kernel(spf_ctx):
    g = hub_mesh(70, 3)
    gp, gr = random_groups(g, 0, 3)
    check(spf_ctx, g, [0], gp, gr, variants=((True, True), (False, False)))


def test_a_slot_with_exactly_sixteen_members(spf_ctx):
    g = hub_mesh(12, 1)
    rp, col = g[0], g[1]
    others = [l for u in range(1, 13) for l in range(int(rp[u]), int(rp[u + 1])) if int(col[l]) != 0][:16]
    gp, gr = SM.groups_csr(len(col), {int(rp[0]): [1], **{l: [1] for l in others}})
    lfa, rl = check(spf_ctx, g, [0], gp, gr)
    assert len(SM.members(*g, 0, gp, gr).of(0)) == 16


def test_two_slots_behind_one_link_share_their_members(spf_ctx):
    # S = 0 on a LAN (vertex 5) with routers 1 and 2, and a p2p link to 3; 4 behind all of them
    links = [(0, 5, 3), (5, 0, 0), (1, 5, 3), (5, 1, 0), (2, 5, 3), (5, 2, 0)] + M.both([(0, 3, 4), (1, 4, 2), (2, 4, 6), (3, 4, 2), (1, 3, 3)])
    g = M.csr(6, links, net=[5])
    gp, gr = group(g, (0, 5), (3, 4), (1, 4))
    lfa, rl = check(spf_ctx, g, [0], gp, gr, need=None)
    mem = SM.members(*g, 0, gp, gr)
    c = M.candidates(*g, 0)
    k1, k2 = slot_to(c, 1), slot_to(c, 2)
    assert c.root_link[k1] == c.root_link[k2] and len(mem.of(k1)) == len(mem.of(k2)) == 2
    assert lfa[0].coverage[6] or rl[0].pq_counts[:, 4].any()


@pytest.mark.parametrize("n", [255, 256, 300])
def test_vertices_at_the_workgroup_edges(spf_ctx, n):
    g = ring_chords(n, n, 1, 9, asym=True)
    gp, gr = random_groups(g, n // 3, n, hops=4)
    check(spf_ctx, g, [n // 3], gp, gr, need=None)


def test_two_mask_words_three_roots_one_table_set(spf_ctx):
    g = mesh(60, 7, 1, 9)
    rp, col = g[0], g[1]
    of = {}
    for s in (3, 20, 41):
        for j in range(int(rp[s + 1] - rp[s])):
            of.setdefault(int(rp[s]) + j, []).append(1000 * s + j)
            hood = [int(x) for x in col[rp[s]:rp[s + 1]]]
            u = hood[(j + 1) % len(hood)]
            of.setdefault(int(rp[u]), []).append(1000 * s + j)
            of.setdefault(int(rp[u + 1]) - 1, []).append(1000 * s + j)
    gp, gr = SM.groups_csr(len(col), of)
    check(spf_ctx, g, [3, 20, 41], gp, gr, w_min=2, variants=((True, True), (True, False), (False, True)))


def test_lan_and_overloaded_router_with_and_without_ignore(spf_ctx):
    links = [(0, 7, 2), (7, 0, 0), (1, 7, 2), (7, 1, 0), (2, 7, 2), (7, 2, 0)]
    links += M.both([(0, 3, 3), (1, 4, 1), (2, 4, 4), (3, 4, 2), (3, 5, 1), (5, 6, 1), (4, 6, 2), (1, 3, 2)])
    g = M.csr(8, links, net=[7], no_transit=[3])
    gp, gr = group(g, (0, 7), (4, 6), (0, 3))
    check(spf_ctx, g, [0], gp, gr, lfa_flags=(0, M.IGNORE_OVERLOAD), need=None)


@pytest.mark.parametrize("seed", range(30))
def test_random_graphs(spf_ctx, seed):
    r = np.random.default_rng(seed)
    n = int(r.integers(40, 201))
    g = ring_chords(n, 100 + seed, 1, 7, chords=n // 3, asym=bool(seed % 2))
    root = int(r.integers(0, n))
    gp, gr = random_groups(g, root, seed, per_link=(1, 7), hops=3)
    check(spf_ctx, g, [root], gp, gr, need=None, tilfa=seed % 3 == 0)


def test_empty_member_lists_equal_the_plain_calls(spf_ctx):
    g = mesh(70, 2, 1, 9)
    gp, gr = random_groups(g, 5, 2)
    check(spf_ctx, g, [5, 30], gp, gr, need=None, no_members=True, variants=((True, True), (False, False)))


def test_argument_errors_are_inval_and_launch_nothing(spf_ctx):
    from holo_amd import engine as E
    g = hub_mesh(8, 8)
    gp, gr = random_groups(g, 0, 8)
    roots, per = plan(g, [0], gp, gr)
    r, c, nr, mem = per[0]
    W = 1
    tab = Tables(spf_ctx, g, 0xFFFFFFFF, roots, 0, W)
    try:
        protect = [(r, E.lfa_candidates(*g, 0), nr)]
        good = product_members(mem)

        def broken(**kw):
            m = product_members(mem)
            for k, v in kw.items():
                a = np.array(getattr(m, k), np.uint32).copy()
                v(a)
                setattr(m, k, a)
            return m

        def setter(i, val):
            def f(a):
                a[i] = val
            return f

        many = np.zeros(len(mem.mem_ptr), np.uint32)
        many[1:] = 17
        # a true monotonicity violation: mem_ptr[2] < mem_ptr[1] with every difference that is looked at before it <= 16
        assert int(mem.mem_ptr[1]) >= 1 and int(mem.mem_ptr[1]) <= 16
        cases = [broken(mem_ptr=setter(2, int(mem.mem_ptr[1]) - 1)), broken(tail=setter(0, tab.n)), broken(head=setter(0, tab.n)),
                 broken(tail_row=setter(0, tab.R)), broken(head_row=setter(0, tab.R)),
                 E.SrlgMembers(many, *(np.zeros(17, np.uint32) for _ in range(6)))]
        for m in cases:
            for call, name in ((run_lfa_srlg, "hspf_lfa_srlg_device"), (run_rlfa_srlg, "hspf_rlfa_srlg_device")):
                with pytest.raises(E.HspfError) as ei:
                    call(spf_ctx, tab, protect, [m])
                assert ei.value.code == -1 and name in str(ei.value)
        for call in (run_lfa_srlg, run_rlfa_srlg):
            with pytest.raises(E.HspfError) as ei:
                call(spf_ctx, tab, protect, [cases[0]])
            assert "not monotone" in str(ei.value)
        # NULL srlg / NULL columns, through the raw binding
        from holo_amd import _lib as L
        import ctypes
        arr, keep = spf_ctx._protect_array(protect, "t")
        out = L.HspfLfaOut(*(tab.dist.data_ptr(),) * 3, None, None, tab.dist.data_ptr())
        head = (spf_ctx.handle, tab.n, tab.R, W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), arr)
        d = tab.dist.data_ptr()
        rout = L.HspfRlfaOut(d, d, d, d, None, None, d, d, d)      # (never written: every call below returns before a launch)
        rhead = (spf_ctx.handle, tab.G.handle, tab.n, tab.R, W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), tab.rdist.data_ptr(), arr)
        mp = np.ascontiguousarray(mem.mem_ptr, np.uint32)
        null_cols = (L.HspfSrlg * 1)(L.HspfSrlg(mp.ctypes.data_as(L.u32p), None, None, None, None, None, None))
        null_ptr = (L.HspfSrlg * 1)(L.HspfSrlg(None, None, None, None, None, None, None))
        for bad_srlg, text in ((None, "NULL srlg"), (null_cols, "NULL member column"), (null_ptr, "NULL mem_ptr")):
            assert spf_ctx.lib.hspf_lfa_srlg_device(*head, bad_srlg, 1, 0, ctypes.byref(out)) == -1
            assert "hspf_lfa_srlg_device" in spf_ctx.last_error() and text in spf_ctx.last_error()
            assert spf_ctx.lib.hspf_rlfa_srlg_device(*rhead, bad_srlg, 1, 0, None, ctypes.byref(rout)) == -1
            assert "hspf_rlfa_srlg_device" in spf_ctx.last_error() and text in spf_ctx.last_error()
        # the context is usable afterwards
        want = SM.lfa(*(lambda f: (f.dist, f.flags, f.mask))(R.tables(g, 0xFFFFFFFF, roots, 0, W)[0]), c, r, nr, mem)
        assert_fields(run_lfa_srlg(spf_ctx, tab, protect, [good]), want, 0, SM.LFA_FIELDS, "after")
        fwd, rdist = R.tables(g, 0xFFFFFFFF, roots, 0, W)
        want_r = SM.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, g[3], c, r, nr, mem)
        assert_fields(run_rlfa_srlg(spf_ctx, tab, protect, [good]), want_r, 0, R.FIELDS, "after")
    finally:
        tab.free()


def test_conveniences_end_to_end(spf_ctx):
    g = hub_mesh(9, 9)
    gp, gr = random_groups(g, 0, 9)
    m = SM.one_root(g, 0, gp, gr)
    G = spf_ctx.upload(*g, 0xFFFFFFFF)
    try:
        cand, mem, lfa = spf_ctx.lfa_srlg(G, 0, gp, gr)
        assert np.array_equal(lfa.alt_slot[0], m["lfa"].alt_slot) and np.array_equal(lfa.coverage[0], m["lfa"].coverage)
        cand, mem, lfa, rl, ti = spf_ctx.tilfa_srlg(G, 0, gp, gr)
        assert np.array_equal(rl.pq_node[0], m["rl"].pq_node) and np.array_equal(rl.rl_coverage[0], m["rl"].rl_coverage)
        assert np.array_equal(ti.ti_counts[0][:, 0], m["rl"].pq_counts[:, 3])
    finally:
        G.free()
