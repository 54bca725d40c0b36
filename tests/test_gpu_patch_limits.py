"""Structural hspf_graph_patch at every limit of the incremental path (holo_amd/csrc/graph_patch.hip.h) and across the
changes between it, the device-side fallback, the cost-only path, the rebuild and the arena growth.  The cases come from
tests/_patch_model.py, which also says which path the host takes (tests/test_host_patch_model.py holds each case to its edge
on the CPU); here, after EVERY patch: every exported array and the number of kept links equal a fresh upload of the patched
CSR, the build mode is the one the model predicts, the layout is the CPU restatement's on the small graphs, SPF (distances,
hops, in-SPT flags, first-hop masks) equals the oracle's from affected, left-out and ordinary roots, and after the
reverse patch every export equals the first one bit for bit.

Each step prints one line of figures (`pytest -s`): the model's affected rows, list size before deduplication, two-way work
and its bound, and the mode the device reported."""
import numpy as np
import pytest

from holo_amd import synth
from holo_amd import engine as E
from oracle import graph_oracle as go
import _patch_model as pm
from test_gpu_graph_build import BUILT, RAW, DERIVED, assert_layout
from _engines import patch_engines

pytestmark = pytest.mark.gpu

EXPORTS = BUILT + RAW + DERIVED + ("zcyc", "host_row_ptr", "host_col")


def snapshot(G):
    out = {name: G.export(name) for name in EXPORTS}
    out["n_edges_kept"] = np.array([G.n_edges_kept])
    return out


def differing(a, b):
    return [name for name in a if not np.array_equal(a[name], b[name])]


def spf_problems(ctx, G, g, roots, run_flags):
    res = ctx.run(G, roots, run_flags)
    ref = go.run(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric, np.asarray(roots, np.uint32), run_flags & 3, go.MAP,
                 mask_words_=res.first_hop_mask.shape[2])
    bad = []
    for name, got, want in (("dist", res.dist, ref.dist), ("hops", res.hops, ref.hops), ("in_spt", res.flags & 1, ref.flags),
                            ("first_hop_mask", res.first_hop_mask, ref.mask)):
        if not np.array_equal(got, want):
            rows = np.unique(np.nonzero(np.asarray(got) != np.asarray(want))[0])
            bad.append(f"spf {name} differs from the oracle for roots {np.asarray(roots)[rows].tolist()}")
    return bad


def run_case(ctx, case, decisions):
    g = case.graph
    run_flags = E.RUN_NET_NEXTHOPS if case.small else 0
    G = ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
    try:
        first = snapshot(G)
        got = first
        for s, d in zip(case.steps, decisions):
            G.patch(s.patch.vs, s.patch.rows, s.patch.flags)
            mode = int(G.export("build_mode")[0])
            print(f"\nPATCHLIMITS {case.name} | {s.tag} | engine={ctx.mode} na={d.na} pre_dedup={d.pre_dedup} tw_work={d.tw_work} "
                  f"bound={d.tw_bound} host={d.path} fallback={d.device_fallback} model_mode={d.build_mode} gpu_mode={mode}", flush=True)
            cur = synth.CsrGraph(G.row_ptr, G.col, G.metric, G.vflags, g.max_path_metric, g.name, g.meta)
            got = snapshot(G)                                     # exported once per step, compared twice
            F = ctx.upload(cur.row_ptr, cur.col, cur.metric, cur.vflags, cur.max_path_metric)
            try:
                fresh = snapshot(F)
            finally:
                F.free()
            problems = [f"{name} differs from a fresh upload" for name in differing(got, fresh)]
            if mode != d.build_mode:
                problems.append(f"build_mode {mode}, the model says {d.build_mode} ({d.path}, {d.why or 'fits'})")
            problems += spf_problems(ctx, G, cur, case.roots, run_flags)
            assert not problems, (case.name, s.tag, f"build_mode == {mode}", problems)
            if case.small:
                assert_layout(G, cur)
            if d.device_fallback:                                 # the rebuild that followed saw the row the staging area could not hold
                summary = got["summary"]
                assert summary[6] == d.max_in_deg_after > pm.PA_IN_STRIDE and summary[3] & pm.RF_GIANT, (case.name, s.tag, summary)
                assert int((got["rowflags"] & pm.RF_GIANT != 0).sum()) == 1
        if case.returns:
            assert differing(got, first) == [], (case.name, "after the reverse patch")
    finally:
        G.free()


_cases = {}


def case_of(make, *args):
    key = (make.__name__,) + args
    if key not in _cases:
        _cases[key] = make(*args)
    return _cases[key]


@patch_engines
@pytest.mark.parametrize("na", pm.LADDER)
def test_affected_row_ladder_at_full_size(spf_ctx, na):
    """(a) isis-100k, routers purged and returned: exactly PA_LDS_ROWS, +1, +2 affected rows (kb_pa_shift's searches move from
    LDS to global memory), PA_MAX_ROWS - 1 and PA_MAX_ROWS (pa_scan_body with eight rows per thread), all incremental, and
    PA_MAX_ROWS + 1: the rebuild.  With HSPF_PATCH_FULL every one rebuilds."""
    case = case_of(pm.ladder_case, na)
    full = spf_ctx.mode == "patchfull"
    decisions = pm.replay(case, patch_full=True) if full else [s.model for s in case.steps]
    assert all(d.na == na for d in decisions)
    assert all(d.build_mode == (pm.MODE_INCREMENTAL if na <= pm.PA_MAX_ROWS and not full else pm.MODE_REBUILD) for d in decisions)
    run_case(spf_ctx, case, decisions)


@pytest.mark.parametrize("name", list(pm.CLUSTERS))
def test_more_old_targets_than_the_list_holds(spf_ctx, name):
    """(b) The replaced rows' old targets are more than 8 x PA_MAX_ROWS list entries while the unique affected rows fit: the
    incremental path is taken (mode 3) and must hand the device the COMPLETE set.  The collection loop used to stop at the
    bound and choose the path from the remainder: the stubs listed only by the last rows kept their stale in- and out-rows,
    the layout differed from a fresh upload's and SPF from a purged router still reached them — with no switch set
    ("purge-1000x18", "also-new-target", "duplicates-100x200"; the two cases at the bound itself were complete before too)."""
    case = case_of(pm.cluster_case, name)
    d = case.steps[0].model
    assert d.path == "incremental" and d.build_mode == pm.MODE_INCREMENTAL and not d.device_fallback
    run_case(spf_ctx, case, [s.model for s in case.steps])


@pytest.mark.parametrize("links", (pm.PA_OUT_STRIDE - 1, pm.PA_OUT_STRIDE, pm.PA_OUT_STRIDE + 1))
def test_row_at_the_out_stride(spf_ctx, links):
    """(c) A row replaced by one of PA_OUT_STRIDE - 1 and PA_OUT_STRIDE links, all kept (incremental: kb_pa_rows gives links
    2 tid and 2 tid + 1 to 256 threads), and of PA_OUT_STRIDE + 1 (the host rebuilds, in hub mode); and back."""
    case = case_of(pm.row_stride_case, links)
    assert case.steps[0].model.build_mode == (pm.MODE_INCREMENTAL if links <= pm.PA_OUT_STRIDE else pm.MODE_HUB)
    run_case(spf_ctx, case, [s.model for s in case.steps])


def test_in_row_at_the_in_stride_and_the_device_fallback(spf_ctx):
    """(c) A LAN's kept in-row 255 -> 256 (incremental, the staging area exactly full), 256 -> 257 (the one place where host
    and device disagree by design: the host cannot know the kept in-degree a patch will produce, sends it down the
    incremental path, kb_pa_rows raises GB_ERR_PATCH after rewriting the rows' records in place, and the host rebuilds:
    mode 0, the summary reports the giant row), 257 -> 256 (a giant row: host rebuild), 256 -> 255 (incremental)."""
    case = case_of(pm.lan_stride_case)
    assert [(s.model.path, s.model.device_fallback) for s in case.steps] == [("incremental", False), ("incremental", True), ("rebuild", False), ("incremental", False)]
    run_case(spf_ctx, case, [s.model for s in case.steps])


def test_path_changes_in_a_chain(spf_ctx):
    """(d) incremental, device fallback, (host rebuild: the giant row the fallback left must shrink first), incremental,
    cost-only, host rebuild, incremental, arena growth, incremental — on one graph, compared in full after every step."""
    case = case_of(pm.chain_case)
    assert [s.model.build_mode for s in case.steps] == [3, 0, 0, 3, 2, 0, 3, 0, 3] and case.steps[7].model.grown
    run_case(spf_ctx, case, [s.model for s in case.steps])


def test_random_multi_row_patches_at_full_size(spf_ctx):
    """(e) Eight seeded rounds of 10 to 150 replaced rows on isis-100k, at least six of them incremental by the model, each run
    once on the device with the path the model gives it, and everything returned at the end."""
    case = case_of(pm.random_case)
    rounds = case.steps[:pm.RANDOM_ROUNDS]
    assert sum(s.model.build_mode == pm.MODE_INCREMENTAL for s in rounds) >= 6
    run_case(spf_ctx, case, [s.model for s in case.steps])
