"""hspf_run_failures* at every mask width and on hop-count-like graphs, against the unmodified CPU oracle on the retargeted CSR
(tests/_failure_cases.py), bit for bit in dist, hops, HSPF_RF_IN_SPT and every mask word (F.same).

Scenario runs always take k_relax<.., FAIL> and k_dag<W, GS, FAIL>, and tests/test_gpu_failures.py reaches kernel widths 1 and 2 only.
Here: every case with 130, 300, 520 and 960 spokes at its root (3, 5, 9, 16 words needed: k_dag<4>, <8>, <16>, <16>, and k_emit writing
fewer words than the kernel holds in the first three), the failed link and the detour in the top word, failures in the later 64-link
chunks of an in-row, the hop-count-like branch of k_dag with a failure in the lane, three batches at width through both forms of the
call, the 16-word limit, and SpfContext.post_convergence sizing the masks itself."""
import numpy as np
import pytest

import _failure_cases as F

pytestmark = pytest.mark.gpu
INF = F.INF


def _upload(ctx, graph, maxp):
    return ctx.upload(graph[0], graph[1], graph[2], graph[3], maxp)


def _run(spf_ctx, base, extra, flags=None, hopcount=None):
    """One case (at(extra) where extra is given) through hspf_run_failures against F.run_check's rows, with the per-case extras of
    tests/test_gpu_failures.py; returns the result."""
    if flags is not None:
        from dataclasses import replace
        base = replace(base, flags=flags)
    graph, ref = F.run_check(base, extra=extra)
    c = base.at(extra) if extra is not None else base
    G = _upload(spf_ctx, graph, c.maxp)
    try:
        if hopcount is not None:
            assert bool(G.export("summary")[1]) == hopcount               # the engine's own verdict: hc != 0 in k_dag
        res = spf_ctx.run_failures(G, c.roots, c.fails, c.flags)
    finally:
        G.free()
    assert res.first_hop_mask.shape[2] == ref.mask.shape[2] == res.stats["n_mask_words"]
    F.same(res, ref)
    if c.exact:
        assert res.stats["n_exact_roots"] >= 1 and res.stats["n_repaired_roots"] == 0        # the sequential kernel, not the repair kernels
    for r, (kind, arg) in enumerate(c.fails):
        if kind == F.ROOT_LINK:                                                              # the slot bit of the failed link is never set
            assert not ((res.first_hop_mask[r, :, arg // 64] >> np.uint64(arg % 64)) & np.uint64(1)).any()
    return res


@pytest.mark.parametrize("extra", F.EXTRAS)
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_case_matches_the_oracle_at_every_width(spf_ctx, name, extra):
    """Every case of the shared list at 3, 5, 9 and 16 mask words.  Among them the sequential kernel at width: zero_cost_plateau and
    saturating_detour (`exact`) must report n_exact_roots >= 1 and n_repaired_roots == 0 at each width; high_slot_detour has the
    failed link and the detour in the top word; giant_row_far and hub_far_link fail links and vertices in the later chunks of an
    in-row."""
    c = F.CASES[name]
    res = _run(spf_ctx, c, extra, hopcount=c.hopcount)
    assert res.first_hop_mask.shape[2] == F.WORDS[extra]


@pytest.mark.parametrize("name,extra", [(n, e) for n, c in sorted(F.WIDE_CASES.items()) for e in sorted(c.words)])
def test_wide_only_case_matches_the_oracle(spf_ctx, name, extra):
    """giant_row_member: a root that is a router of the 301-router LAN (303 slots of its own: 5, 7, 10 and 13 words), its failed link
    into the LAN in the fifth 64-link chunk of the LAN's in-row and looking tight."""
    c = F.WIDE_CASES[name]
    res = _run(spf_ctx, c, extra or None)
    assert res.first_hop_mask.shape[2] == c.words[extra]


@pytest.mark.parametrize("flags", [0, F.NET_NEXTHOPS])
@pytest.mark.parametrize("extra", [None, 300])
def test_hopcount_first_parent_with_a_failure_in_the_lane(spf_ctx, extra, flags):
    """hopcount_lan_first_parent at one word (k_dag<1, GS = true, FAIL>) and at five, with and without HSPF_RUN_NET_NEXTHOPS."""
    _run(spf_ctx, F.CASES["hopcount_lan_first_parent"], extra, flags=flags, hopcount=True)


@pytest.mark.parametrize("flags", [0, F.NET_NEXTHOPS])
@pytest.mark.parametrize("extra", [None, 280])
@pytest.mark.parametrize("seed", F.HOPCOUNT_SEEDS)
def test_hopcount_random_every_link_and_neighbour_of_three_roots(spf_ctx, seed, extra, flags):
    """20 seeded hop-count-like graphs, every link and every neighbour (mostly LANs) of three router roots, at one word and at five."""
    _run(spf_ctx, F.hopcount_random(seed), extra, flags=flags, hopcount=True)


def _wide_batch130():
    """F.batch130() with 130 spokes at the root S: three words."""
    graph, maxp, S, roots, fails = F.batch130()
    rp, col, met, vf = graph
    rows = [[(int(col[k]), int(met[k])) for k in range(int(rp[v]), int(rp[v + 1]))] for v in range(len(vf))]
    graph = F.csr(*F.widen(rows, vf.tolist(), S, 130))
    return graph, maxp, roots, fails, F.reference(graph, maxp, roots, fails)


def test_130_rows_at_three_words_host_and_device_forms(spf_ctx):
    """Three batches (the last ragged) at three words needed, kernel width 4: the host form; the device form into filled tensors; and
    the HSPF_FAIL_NONE / HSPF_NO_ROOT rows against hspf_run_device's rows of the same roots, which at this width come from k_fw."""
    import torch
    graph, maxp, roots, fails, ref = _wide_batch130()
    n = len(graph[3])
    assert ref.mask.shape[2] == 3
    G = _upload(spf_ctx, graph, maxp)
    try:
        W = G.mask_words(roots)
        assert W == 3
        res = spf_ctx.run_failures(G, roots, fails)
        assert res.stats["n_batches"] == 3 and res.stats["n_roots"] == 130
        F.same(res, ref)
        dev = torch.device("cuda:0")
        t = [dict(dist=torch.full((130, n), 0x07070707, dtype=torch.int32, device=dev), hops=torch.full((130, n), 0x0707, dtype=torch.int16, device=dev),
                  flags=torch.full((130, n), 0x0707, dtype=torch.int16, device=dev),
                  mask=torch.full((130, n, W), 0x0707070707070707, dtype=torch.int64, device=dev)) for _ in range(2)]
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        spf_ctx.run_failures_device(G, roots, fails, 0, dist_ptr=t[0]["dist"].data_ptr(), hops_ptr=t[0]["hops"].data_ptr(), flags_ptr=t[0]["flags"].data_ptr(),
                                    mask_ptr=t[0]["mask"].data_ptr(), mask_words=W)
        spf_ctx.run_device(G, roots, 0, dist_ptr=t[1]["dist"].data_ptr(), hops_ptr=t[1]["hops"].data_ptr(), flags_ptr=t[1]["flags"].data_ptr(),
                           mask_ptr=t[1]["mask"].data_ptr(), mask_words=W)
    finally:
        G.free()
    a, b = ({k: v.cpu().numpy() for k, v in x.items()} for x in t)
    # the device form wrote every element: bit for bit the oracle's rows, nothing of the fill left
    assert np.array_equal(a["dist"].view(np.uint32), ref.dist) and np.array_equal(a["hops"].view(np.uint16), ref.hops)
    assert np.array_equal(a["flags"].view(np.uint16) & ~F.RF_EXACT, ref.flags) and np.array_equal(a["mask"].view(np.uint64), ref.mask)
    none = np.array([k == F.NONE or int(r) == F.NO_ROOT for r, (k, _) in zip(roots, fails)])
    assert none.sum() > 40
    for k in ("dist", "hops", "mask"):
        assert np.array_equal(a[k][none], b[k][none]), k
    assert np.array_equal(a["flags"][none] & ~2, b["flags"][none] & ~2)                    # (HSPF_RF_EXACT: the two calls take different paths)


def test_seventeen_words_are_refused_by_both_forms(spf_ctx):
    """A root with 1 032 slots needs 17 mask words: HSPF_E_TOO_MANY_SLOTS from both forms, nothing launched (the statistics of the
    last run stay), and the context goes on working."""
    import torch
    from holo_amd.engine import HspfError
    c = F.CASES["ring"]
    big = c.at(1030)
    small = c.at(130)
    n = len(big.vf)
    G, G2 = _upload(spf_ctx, big.graph(), big.maxp), _upload(spf_ctx, small.graph(), small.maxp)
    try:
        assert G.mask_words(big.roots) == 17
        spf_ctx.run_failures(G2, small.roots, small.fails)
        before = spf_ctx.stats()
        with pytest.raises(HspfError) as e:
            spf_ctx.run_failures(G, big.roots, big.fails)
        assert e.value.code == -5 and spf_ctx.stats() == before
        dev = torch.device("cuda:0")
        dist = torch.full((1, n), 7, dtype=torch.int32, device=dev)
        mask = torch.full((1, n, 17), 7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
        with pytest.raises(HspfError) as e:
            spf_ctx.run_failures_device(G, big.roots, big.fails, 0, dist_ptr=dist.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=17)
        assert e.value.code == -5 and spf_ctx.stats() == before
        torch.cuda.synchronize()
        assert bool((dist == 7).all()) and bool((mask == 7).all())                           # nothing was written
        _, ref = F.run_check(c, extra=130)
        F.same(spf_ctx.run_failures(G2, small.roots, small.fails), ref)
    finally:
        G.free()
        G2.free()


@pytest.mark.parametrize("node", [False, True])
def test_post_convergence_sizes_the_masks_itself(spf_ctx, node):
    """SpfContext.post_convergence on the two_lans root with 130 spokes (three words): one row per candidate slot, against the oracle."""
    c = F.CASES["two_lans"].at(130)
    graph = c.graph()
    G = _upload(spf_ctx, graph, c.maxp)
    try:
        cand, sl, rows = spf_ctx.post_convergence(G, 0, node=node)
    finally:
        G.free()
    assert len(sl) >= 130 and rows.first_hop_mask.shape[2] == 3
    fails = [(F.VERTEX, int(cand.nbr[e])) if node else (F.ROOT_LINK, int(cand.root_link[e])) for e in sl]
    ref = F.reference(graph, c.maxp, [0] * len(sl), fails)
    assert ref.mask.shape[2] == 3
    F.same(rows, ref)
    assert (rows.dist[:, 1] == INF).any() and (rows.dist[:, 1] == 10).any()                 # the row that loses router 1, and the spokes' rows that do not
