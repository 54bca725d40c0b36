"""hspf_run_failures* on the GPU against the unmodified CPU oracle on the retargeted CSR (tests/_failure_cases.py), bit for bit in
dist, hops, HSPF_RF_IN_SPT and every mask word: the shared case list through both engine widths (n_mask_words 1, and 2 through a root
with more than 64 slots), 130 rows over three batches with repeated roots and padding, the argument errors, seeded random LSDBs with a
structural patch in between, the fast-reroute family's distance promise, and the compiled driver."""
import os
import subprocess

import numpy as np
import pytest

import _failure_cases as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = F.INF


def _upload(ctx, graph, maxp):
    return ctx.upload(graph[0], graph[1], graph[2], graph[3], maxp)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_case_matches_the_oracle(spf_ctx, name, wide):
    c = F.CASES[name]
    graph, ref = F.run_check(c, wide)
    G = _upload(spf_ctx, graph, c.maxp)
    try:
        res = spf_ctx.run_failures(G, c.roots, c.fails, c.flags)
    finally:
        G.free()
    assert res.first_hop_mask.shape[2] == (2 if wide else 1)
    F.same(res, ref)
    if c.exact:
        assert res.stats["n_exact_roots"] >= 1 and res.stats["n_repaired_roots"] == 0        # the sequential kernel, not the repair kernels
    for r, (kind, arg) in enumerate(c.fails):
        if kind == F.ROOT_LINK:                                                              # the slot bit of the failed link is never set
            assert not ((res.first_hop_mask[r, :, arg // 64] >> np.uint64(arg % 64)) & np.uint64(1)).any()


def test_130_rows_repeated_roots_and_padding(spf_ctx):
    import torch
    graph, maxp, S, roots, fails = F.batch130()
    n = len(graph[3])
    ref = F.reference(graph, maxp, roots, fails)
    G = _upload(spf_ctx, graph, maxp)
    try:
        W = G.mask_words(roots)
        assert W == ref.mask.shape[2]
        res = spf_ctx.run_failures(G, roots, fails)
        assert res.stats["n_batches"] == 3 and res.stats["n_roots"] == 130
        F.same(res, ref)
        # the device form, and the HSPF_FAIL_NONE rows against hspf_run_device's rows of the same roots
        dev = torch.device("cuda:0")
        t = [dict(dist=torch.empty((130, n), dtype=torch.int32, device=dev), hops=torch.empty((130, n), dtype=torch.int16, device=dev),
                  flags=torch.empty((130, n), dtype=torch.int16, device=dev), mask=torch.empty((130, n, W), dtype=torch.int64, device=dev)) for _ in range(2)]
        spf_ctx.run_failures_device(G, roots, fails, 0, dist_ptr=t[0]["dist"].data_ptr(), hops_ptr=t[0]["hops"].data_ptr(), flags_ptr=t[0]["flags"].data_ptr(),
                                    mask_ptr=t[0]["mask"].data_ptr(), mask_words=W)
        spf_ctx.run_device(G, roots, 0, dist_ptr=t[1]["dist"].data_ptr(), hops_ptr=t[1]["hops"].data_ptr(), flags_ptr=t[1]["flags"].data_ptr(),
                           mask_ptr=t[1]["mask"].data_ptr(), mask_words=W)
    finally:
        G.free()
    a, b = ({k: v.cpu().numpy() for k, v in x.items()} for x in t)
    assert np.array_equal(a["dist"].view(np.uint32), res.dist) and np.array_equal(a["mask"].view(np.uint64), res.first_hop_mask)
    none = np.array([k == F.NONE or int(r) == F.NO_ROOT for r, (k, _) in zip(roots, fails)])
    assert none.sum() > 40
    for k in ("dist", "hops", "mask"):
        assert np.array_equal(a[k][none], b[k][none]), k
    assert np.array_equal(a["flags"][none] & ~2, b["flags"][none] & ~2)                    # (HSPF_RF_EXACT: the two calls take different paths)


def test_argument_errors_launch_nothing_and_name_the_call(spf_ctx):
    from holo_amd.engine import HspfError, RUN_POP_RANK, RUN_COUNT_ROWS
    c = F.CASES["ring"]
    G = _upload(spf_ctx, c.graph(), c.maxp)
    try:
        spf_ctx.run(G, [0, 1, 2])
        before = spf_ctx.stats()
        for roots, fails, flags in (([0], [(F.ROOT_LINK, 2)], 0), ([0], [(F.VERTEX, 0)], 0), ([0], [(F.VERTEX, 6)], 0), ([0], [(3, 0)], 0),
                                    ([0], [(F.NONE, 0)], RUN_POP_RANK), ([0], [(F.NONE, 0)], RUN_COUNT_ROWS), ([6], [(F.NONE, 0)], 0)):
            with pytest.raises(HspfError) as e:
                spf_ctx.run_failures(G, roots, fails, flags)
            assert e.value.code == -1 and "hspf_run_failures: " in str(e.value)
            assert spf_ctx.stats() == before
        # HSPF_NO_ROOT: the failure is not looked at
        res = spf_ctx.run_failures(G, [F.NO_ROOT, 0], [(F.VERTEX, 99), (F.NONE, 7)])
        assert (res.dist[0] == INF).all() and res.dist[1].tolist() == [0, 1, 2, 3, 2, 1]
    finally:
        G.free()


@pytest.mark.parametrize("seed", range(40))
def test_random_isis_and_ospf_instances_every_link_and_neighbour_of_three_roots(spf_ctx, seed):
    """40 seeded random graphs of tests/_random_isis.py / tests/_random_ospf.py: every link and every neighbour of three roots (all
    routers where there are fewer), with one hspf_graph_patch applied in between for half of them (seeds 2, 3 mod 4)."""
    graph, maxp, flags = F.protocol_graph(seed)
    r = np.random.default_rng(9100 + seed)
    G = _upload(spf_ctx, graph, maxp)
    try:
        if seed % 4 >= 2:
            graph, _ = F.drop_last_link(G, graph)
        routers = np.flatnonzero((graph[3] & 1) == 0)
        roots, fails = [], []
        for S in r.choice(routers, min(3, len(routers)), replace=False):
            sc = F.all_scenarios(graph, int(S))
            roots += [int(S)] * len(sc)
            fails += sc
        if not roots:                                                    # (an instance whose routers list nobody)
            roots, fails = [int(routers[0])], [(F.NONE, 0)]
        ref = F.reference(graph, maxp, roots, fails, flags)
        res = spf_ctx.run_failures(G, roots, fails, flags)
    finally:
        G.free()
    F.same(res, ref)


@pytest.mark.parametrize("seed", range(40))
def test_random_lsdbs_every_link_and_neighbour_of_three_roots(spf_ctx, seed):
    """Seeded random LSDBs (routers and LANs, overload bits, zero-cost links on every fourth): every link and every neighbour of three
    roots; on odd seeds one structural hspf_graph_patch is applied first (a router's row loses its last link)."""
    from holo_amd import synth
    from holo_amd.engine import splice_rows
    r = np.random.default_rng(9000 + seed)
    g = synth.random_lsdb(int(r.integers(20, 90)), int(r.integers(2, 9)), 3.0, 100 + seed, metric_hi=int(r.integers(1, 12)), zero_cost_router_links=(seed % 4 == 3))
    graph = (g.row_ptr, g.col, g.metric, g.vflags)
    flags = (0, F.NET_NEXTHOPS, F.IGNORE_OVERLOAD)[seed % 3]
    G = _upload(spf_ctx, graph, int(g.max_path_metric))
    try:
        if seed % 2:
            deg = np.diff(g.row_ptr.astype(np.int64))
            u = int(np.flatnonzero((g.vflags == 0) & (deg >= 2))[0])
            a, b = int(g.row_ptr[u]), int(g.row_ptr[u + 1]) - 1
            G.patch([u], [(g.col[a:b], g.metric[a:b])], [int(g.vflags[u])])
            graph = splice_rows(g.row_ptr, g.col, g.metric, g.vflags, [u], [g.col[a:b]], [g.metric[a:b]], [int(g.vflags[u])])
        n = len(graph[3])
        routers = np.flatnonzero((graph[3] & 1) == 0)
        roots, fails = [], []
        for S in r.choice(routers, 3, replace=False):
            sc = F.all_scenarios(graph, int(S))
            roots += [int(S)] * len(sc)
            fails += sc
        ref = F.reference(graph, int(g.max_path_metric), roots, fails, flags)
        res = spf_ctx.run_failures(G, roots, fails, flags)
    finally:
        G.free()
    assert len(roots) >= 3 and n == res.dist.shape[1]
    F.same(res, ref)


def _promise(spf_ctx, graph, maxp, S):
    """ti_metric of every candidate slot of S == dist[E] of that slot's HSPF_FAIL_ROOT_LINK row; HSPF_TILFA_NONE exactly where the row
    leaves E unreachable.  Returns (slots checked, slots without a repair)."""
    from holo_amd import engine as E
    G = _upload(spf_ctx, graph, maxp)
    try:
        cand, _, _, ti = spf_ctx.tilfa(G, S)
        c2, sl, rows = spf_ctx.post_convergence(G, S)
    finally:
        G.free()
    assert np.array_equal(c2.nbr, cand.nbr) and len(sl) == int((cand.nbr != E.NO_ROOT).sum())
    none = 0
    for i, e in enumerate(sl):
        d = int(rows.dist[i, int(cand.nbr[e])])
        if d == INF:
            assert ti.ti_kind[0, e] == E.TILFA_NONE, (S, int(e))
            none += 1
        else:
            assert ti.ti_kind[0, e] != E.TILFA_NONE and int(ti.ti_metric[0, e]) == d, (S, int(e), d, int(ti.ti_metric[0, e]))
    return len(sl), none


@pytest.mark.parametrize("name,applies", [("a", [0, 1, 2, 3, 4]), ("b", [0, 2]), ("c", [0, 1, 2, 3]), ("d", [0])])
def test_tilfa_promise_on_the_patch_chains(spf_ctx, name, applies):
    """The graphs of tests/test_host_tilfa.py's distance property, first half: the steps of the four patch chains it applies to
    (routers only, symmetric costs >= 1, no overload, no parallel links), every protected root of the step."""
    import _frr_chains as FC
    chain = FC.chain(name)
    slots = 0
    for i, step in enumerate(chain.steps):
        assert FC.property_applies(step.graph) == (i in applies), (name, i)
        if i in applies:
            for S in step.prot:
                slots += _promise(spf_ctx, step.graph, chain.maxp, int(S))[0]
    assert slots >= 2 * len(applies)


def test_tilfa_promise_on_the_sweep_graphs(spf_ctx):
    """... second half: the graphs of _frr_chains.sweep_graphs() that qualify (neither asymmetric nor zero-cost nor overloaded, no
    parallel links), their seeded root."""
    import _frr_chains as FC
    checked = graphs = 0
    for g, root, w in FC.sweep_graphs():
        if w["asym"] or w["zero"] or w["overload"] or not FC.property_applies(g):
            continue
        checked += _promise(spf_ctx, g, FC.MAXP, int(root))[0]
        graphs += 1
    assert graphs >= 1 and checked >= 2 * graphs


def test_tilfa_metric_is_the_distance_of_the_root_link_row(spf_ctx):
    """The same on 20 more graphs of this file's own, with a bridge at the root on every third so that HSPF_TILFA_NONE occurs.
    The family's promise on the device: on router-only graphs with symmetric costs >= 1 and no overload, ti_metric of every candidate
    slot equals dist[E] of that slot's HSPF_FAIL_ROOT_LINK row, and HSPF_TILFA_NONE occurs exactly where the row leaves E unreachable."""
    from holo_amd import engine as E
    import _frr_chains as FC
    r = np.random.default_rng(20240611)
    slots = none = 0
    for _ in range(20):
        n = int(r.integers(4, 15))
        unit = bool(r.integers(0, 2))
        und = [(v, (v + 1) % n, 1 if unit else int(r.integers(1, 10))) for v in range(n)]
        seen = {frozenset((a, b)) for a, b, _ in und}
        for _ in range(int(r.integers(0, n + 1))):
            a, b = (int(x) for x in r.integers(0, n, 2))
            if a != b and frozenset((a, b)) not in seen:
                seen.add(frozenset((a, b)))
                und.append((a, b, 1 if unit else int(r.integers(1, 10))))
        S = int(r.integers(0, n))
        if n % 3 == 0:
            und.append((0, n, 1))                                      # a bridge at the root: its far side has no repair
            n += 1
            S = 0
        graph = F.csr(F.both(n, und))
        assert FC.property_applies(graph)
        G = _upload(spf_ctx, graph, INF)
        try:
            cand, _, _, ti = spf_ctx.tilfa(G, S)
            c2, sl, rows = spf_ctx.post_convergence(G, S)
        finally:
            G.free()
        assert np.array_equal(c2.nbr, cand.nbr) and len(sl) == int((cand.nbr != E.NO_ROOT).sum())
        for i, e in enumerate(sl):
            d = int(rows.dist[i, int(cand.nbr[e])])
            if d == INF:
                assert ti.ti_kind[0, e] == E.TILFA_NONE
                none += 1
            else:
                assert ti.ti_kind[0, e] != E.TILFA_NONE and int(ti.ti_metric[0, e]) == d, (S, int(e), d, int(ti.ti_metric[0, e]))
            slots += 1
    assert slots >= 40 and none >= 1            # every root sits on the ring: at least two candidate slots per graph


def test_post_convergence_node_rows(spf_ctx):
    c = F.CASES["cut_vertex"]
    graph = c.graph()
    G = _upload(spf_ctx, graph, c.maxp)
    try:
        cand, sl, rows = spf_ctx.post_convergence(G, 0, node=True)
    finally:
        G.free()
    ref = F.reference(graph, c.maxp, [0] * len(sl), [(F.VERTEX, int(cand.nbr[e])) for e in sl])
    F.same(rows, ref)
    assert rows.dist[list(cand.nbr[sl]).index(1)].tolist() == [0, INF, INF, INF, 1]


def test_compiled_driver_on_the_gpu_engine(tmp_path):
    import test_host_failures as H
    H._build_driver()
    files = H._files(tmp_path)
    out = subprocess.run([H.DRIVER, "--engine", "hip"] + files, capture_output=True, text=True, timeout=300)
    m = H.LINE.search(out.stdout)
    assert out.returncode == 0 and m, out.stdout + out.stderr
    assert int(m.group(1)) == len(files) and int(m.group(3)) == 0
