"""k_fused_lean has two instantiations per launch mode: one for graphs with rows that take a zero-cost link from a higher- or
equal-numbered source (RF_ZERO rows, not hop-count-like: the pop order of some roots may be dynamic) and a clean one without
the zero-cost row path and the LF_DYN bookkeeping.  The host picks it from the graph's count of RF_ZERO rows and its
hop-count shape (hspf_graph_export HSPF_GX_SUMMARY: [1] hop-count-like, [4] RF_ZERO rows), which every patch path keeps
current, and reports it in hspf_stats::dbg[0] (bit 0: the lean sweep ran, bit 1: its zero-cost row instantiation).  Every
run below equals the CPU oracle bit for bit, on both sides of every switch."""
import os

import numpy as np
import pytest

from holo_amd import synth
from holo_amd import engine as E
from oracle import graph_oracle as go

from _engines import sweeps_engine  # noqa: E402

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(64, os.cpu_count() or 1)


def _zero_rows(G):
    s = G.export("summary")
    return int(s[4]), int(s[1])


def _check(ctx, G, max_path_metric, roots, flags=0):
    res = ctx.run(G, roots, flags)
    ref = go.run(G.row_ptr, G.col, G.metric, G.vflags, max_path_metric, roots, flags & 3, go.HEAP,
                 mask_words_=res.first_hop_mask.shape[2], threads=ORACLE_THREADS)
    assert np.array_equal(res.dist, ref.dist), "dist"
    assert np.array_equal(res.hops, ref.hops), "hops"
    assert np.array_equal(res.flags & 1, ref.flags), "flags"
    assert np.array_equal(res.first_hop_mask, ref.mask), "first-hop mask"
    return res.stats


def _row(G, u):
    a, b = int(G.row_ptr[u]), int(G.row_ptr[u + 1])
    return G.col[a:b].copy(), G.metric[a:b].copy()


def _lower_neighbour(G, u):
    """Position in u's row of a link to a lower-numbered router with a link back (a zero cost on it makes that row RF_ZERO)."""
    cols, _ = _row(G, u)
    for k, v in enumerate(cols):
        v = int(v)
        if v < u and not (G.vflags[v] & synth.VF_NETWORK) and u in set(int(x) for x in _row(G, v)[0]):
            return k
    raise AssertionError(f"router {u} has no lower-numbered two-way neighbour")


@sweeps_engine
def test_isis_100k_clean_then_cost_patch_to_zero_and_back(spf_ctx):
    g = synth.isis_100k()
    roots = (np.arange(64, dtype=np.int64) * g.n // 64).astype(np.uint32)
    G = spf_ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
    try:
        assert _zero_rows(G) == (0, 0)                               # clean: the instantiation without the zero-cost row path
        st = _check(spf_ctx, G, g.max_path_metric, roots)
        assert st["state_bytes"] == 4 and (st["dbg"][0] & 3) == 1 and st["n_repaired_roots"] == 0
        # a cost-only patch puts one router link at 0: the next run takes the other instantiation, dynamic roots included
        u = int(roots[5]) + 1
        k = _lower_neighbour(G, u)
        cols, mets = _row(G, u)
        old = int(mets[k])
        mets[k] = 0
        G.patch([u], [(cols, mets)], [G.vflags[u]])
        assert int(G.export("build_mode")[0]) == 2                   # costs only
        assert _zero_rows(G)[0] >= 1
        st = _check(spf_ctx, G, g.max_path_metric, roots)
        assert (st["dbg"][0] & 3) == 3 and st["n_repaired_roots"] > 0, st
        # and back: clean again
        mets[k] = old
        G.patch([u], [(cols, mets)], [G.vflags[u]])
        assert _zero_rows(G) == (0, 0)
        st = _check(spf_ctx, G, g.max_path_metric, roots)
        assert (st["dbg"][0] & 3) == 1 and st["n_repaired_roots"] == 0
    finally:
        G.free()


@sweeps_engine
def test_isis_100k_structural_patch_adds_and_removes_a_zero_cost_link(spf_ctx):
    g = synth.isis_100k()
    roots = (np.arange(64, dtype=np.int64) * g.n // 64 + 7).astype(np.uint32)
    G = spf_ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
    try:
        assert _zero_rows(G) == (0, 0)
        _check(spf_ctx, G, g.max_path_metric, roots)
        # a new two-way link u - v, v < u, cost 0 from u to v (row v becomes RF_ZERO), 5 back
        u = int(roots[9]) + 3
        nb = set(int(x) for x in _row(G, u)[0])
        v = next(x for x in range(u - 2, 0, -1) if x not in nb and not (G.vflags[x] & synth.VF_NETWORK))
        cu, mu = _row(G, u)
        cv, mv = _row(G, v)
        G.patch([u, v], [(np.append(cu, v), np.append(mu, 0)), (np.append(cv, u), np.append(mv, 5))], [G.vflags[u], G.vflags[v]])
        assert int(G.export("build_mode")[0]) != 2                   # structural
        assert _zero_rows(G)[0] >= 1
        st = _check(spf_ctx, G, g.max_path_metric, roots)
        assert (st["dbg"][0] & 3) == 3 and st["n_repaired_roots"] > 0, st
        # the link goes away again: clean
        G.patch([u, v], [(cu, mu), (cv, mv)], [G.vflags[u], G.vflags[v]])
        assert _zero_rows(G) == (0, 0)
        st = _check(spf_ctx, G, g.max_path_metric, roots)
        assert (st["dbg"][0] & 3) == 1 and st["n_repaired_roots"] == 0
    finally:
        G.free()


@sweeps_engine
@pytest.mark.parametrize("seed", range(3))
def test_hopcount_graph_takes_the_clean_instantiation(spf_ctx, seed):
    """Hop-count graphs (cost 0 into pseudonodes) have zero-cost rows but their own rule, which never reports LF_DYN:
    the clean instantiation runs them, through the general row routine for the RF_ZERO rows.  The roots are routers with at
    most 12 first-hop slots: the lean sweep's 4-byte word then keeps 7 hop bits and a 10-bit distance field (a run whose
    roots need more mask bits leaves too few for the other fields and goes to k_fused)."""
    g = synth.random_lsdb(3000, 400, 3.0, 900 + seed, hopcount=True)
    G = spf_ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
    try:
        cand = [r for r in range(400, 3000) if not (g.vflags[r] & synth.VF_NETWORK) and G.slot_table(r)[2] <= 12]
        assert len(cand) >= 128
        roots = np.array(cand[:128], dtype=np.uint32)
        nz, hc = _zero_rows(G)
        assert hc == 1 and nz >= 1
        st = _check(spf_ctx, G, g.max_path_metric, roots, E.RUN_IGNORE_OVERLOAD)
        assert (st["dbg"][0] & 3) == 1 and st["n_repaired_roots"] == 0, st     # the lean sweep, clean instantiation
    finally:
        G.free()
