"""The cases of tests/test_gpu_patch_limits.py sit where they claim (tests/_patch_model.py: a CPU restatement of the host's
choice between the incremental structural patch and the rebuild).  A generator that drifts off its edge fails HERE; it must
not quietly turn a GPU test of the incremental path into a test of the rebuild."""
import numpy as np
import pytest

from holo_amd import synth
import _patch_model as pm
from _layout_ref import layout


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in pm.all_cases()}


def test_constants_come_from_the_sources():
    assert pm.PA_LDS_ROWS < pm.PA_MAX_ROWS and pm.PA_IN_STRIDE <= pm.GIANT_DEG and pm.PA_OUT_STRIDE <= pm.HUB_DEG
    assert pm.AFF_LIMIT == pm.AFF_FACTOR * pm.PA_MAX_ROWS and pm.AFF_FACTOR > 1
    assert pm.LADDER == (pm.PA_LDS_ROWS, pm.PA_LDS_ROWS + 1, pm.PA_LDS_ROWS + 2, pm.PA_MAX_ROWS - 1, pm.PA_MAX_ROWS, pm.PA_MAX_ROWS + 1)


def check_claims(case):
    for s in case.steps:
        d, c = s.model, s.claim
        where = (case.name, s.tag)
        if "path" in c:
            assert d.path == c["path"], (where, d.path, d.why)
        if c.get("na") is not None:
            assert d.na == c["na"], where
        if "pre_dedup" in c:
            assert d.pre_dedup == c["pre_dedup"], where
        if "pre_dedup_side" in c:
            assert (d.pre_dedup <= pm.AFF_LIMIT) == (c["pre_dedup_side"] == "le"), (where, d.pre_dedup)
        if "fallback" in c:
            assert d.device_fallback == c["fallback"], where
        if "grown" in c:
            assert d.grown == c["grown"], where
        if "max_new_len" in c:
            assert d.max_new_len == c["max_new_len"], where
        if "max_old_len" in c:
            assert d.max_old_len == c["max_old_len"], where
        if "in_after" in c:
            assert d.max_in_deg_after == c["in_after"], where
        if d.path == "incremental":
            assert d.tw_work <= d.tw_bound and d.na <= pm.PA_MAX_ROWS and max(d.max_old_len, d.max_new_len) <= pm.PA_OUT_STRIDE, where
            assert d.max_in_deg_before <= pm.PA_IN_STRIDE, where
            assert d.build_mode == (pm.MODE_REBUILD if d.device_fallback else pm.MODE_INCREMENTAL), where
        assert d.tw_bound == max(pm.TW_MIN, d.e_new // pm.TW_DIV), where           # no switch: the product's bound


def test_every_case_sits_where_it_claims(cases):
    assert len(cases) == len(pm.LADDER) + len(pm.CLUSTERS) + 3 + 3
    for case in cases.values():
        check_claims(case)
        if case.returns:                                                         # the last step restores the first graph
            g, mdl = case.graph, pm.GraphModel(case.graph.row_ptr, case.graph.col, case.graph.metric, case.graph.vflags)
            for s in case.steps:
                mdl.step(s.patch)
            assert np.array_equal(mdl.row_ptr, g.row_ptr) and np.array_equal(mdl.col, g.col) and np.array_equal(mdl.metric, g.metric)
            assert np.array_equal(mdl.vflags, g.vflags)


def test_ladder_hits_each_count_exactly(cases):
    for na in pm.LADDER:
        case = cases[f"ladder-{na}"]
        for s in case.steps:
            assert s.model.na == na
            assert s.model.path == ("incremental" if na <= pm.PA_MAX_ROWS else "rebuild"), (na, s.tag, s.model.why)
            if na > pm.PA_MAX_ROWS:
                assert s.model.why == "affected rows > PA_MAX_ROWS"                # and nothing else sends it to the rebuild
        assert all(len(c) == 0 for c, _ in case.steps[0].patch.rows)
        # with the old and the new links in one patch the work does not fit: purge and return stay two patches
        both = case.steps[0].model.tw_work + case.steps[1].model.tw_work
        if na >= pm.PA_MAX_ROWS - 1:
            assert both > case.steps[0].model.tw_bound
    # in another configuration every one of them rebuilds
    assert all(d.path == "rebuild" and d.build_mode == pm.MODE_REBUILD for d in pm.replay(cases[f"ladder-{pm.PA_LDS_ROWS}"], patch_full=True))


def test_cluster_cases_cross_the_list_bound_as_stated(cases):
    """The list of a cluster patch passes AFF_LIMIT entries while its unique rows fit, and the loop that stopped there
    (pm.legacy_affected) leaves live two-way stubs out — except for the two cases at the bound itself, which it completes."""
    for name in pm.CLUSTERS:
        case = cases["cluster-" + name]
        g, s = case.graph, case.steps[0]
        d = s.model
        old, stop = pm.legacy_affected(g.row_ptr, g.col, s.patch)
        live = case.notes["live_stubs"]
        assert np.isin(live, d.affected).all() and np.isin(case.notes["live_routers"], d.affected).all()
        kin = pm.kept_in_degree(g.row_ptr, g.col, g.vflags)
        assert (kin[live] >= 1).all() and kin.max() <= pm.PA_IN_STRIDE and d.max_old_len <= pm.PA_OUT_STRIDE
        left_out = np.setdiff1d(d.affected, old)
        if name in ("exact-limit", "limit-plus-1"):
            assert d.pre_dedup == pm.AFF_LIMIT + (name == "limit-plus-1") and stop is None and len(left_out) == 0
        else:
            assert d.pre_dedup > pm.AFF_LIMIT and stop is not None and len(old) <= pm.PA_MAX_ROWS
            assert len(left_out) and np.isin(left_out, live).all()
            assert stop <= int(case.notes["live_routers"].min() - s.patch.vs[0])   # the rows behind the stop are the live ones
            assert np.isin(case.roots, left_out).any() and np.isin(case.roots, old).any()
        if name == "also-new-target":
            assert np.isin(s.patch.rows[0][0], live).all() and np.isin(s.patch.rows[0][0], old).all() and len(left_out) == len(live) - len(s.patch.rows[0][0])
    d = cases["cluster-purge-1000x18"].steps[0].model
    assert (d.pre_dedup, d.na, d.tw_work, d.tw_bound) == (19000, 1650, 20610, 31254)
    assert pm.legacy_affected(cases["cluster-purge-1000x18"].graph.row_ptr, cases["cluster-purge-1000x18"].graph.col,
                              cases["cluster-purge-1000x18"].steps[0].patch)[1] == 855


def test_stride_cases_stand_on_their_edges(cases):
    g = pm.stride_graph()
    want = layout(g.row_ptr, g.col, g.metric, g.vflags)
    kin = np.diff(want["in_ptr"].astype(np.int64))
    assert np.array_equal(kin, pm.kept_in_degree(g.row_ptr, g.col, g.vflags))      # the vectorised count is the restatement's
    assert kin[g.meta["P"]] == pm.PA_IN_STRIDE - 1 and kin.max() == pm.PA_IN_STRIDE - 1
    for name in ("lan-in-row", "chain", "row-511", "row-512", "row-513"):
        case = cases[name.replace("511", str(pm.PA_OUT_STRIDE - 1)).replace("512", str(pm.PA_OUT_STRIDE)).replace("513", str(pm.PA_OUT_STRIDE + 1))]
        mdl = pm.GraphModel(g.row_ptr, g.col, g.metric, g.vflags)
        for s in case.steps:
            mdl.step(s.patch)
            w = layout(mdl.row_ptr, mdl.col, mdl.metric, mdl.vflags)
            k2 = np.diff(w["in_ptr"].astype(np.int64))
            assert np.array_equal(k2, mdl.kin), (name, s.tag)
            assert s.model.max_in_deg_after == k2.max(), (name, s.tag)
    lan = cases["lan-in-row"]
    assert [s.model.max_in_deg_after for s in lan.steps] == [pm.PA_IN_STRIDE, pm.PA_IN_STRIDE + 1, pm.PA_IN_STRIDE, pm.PA_IN_STRIDE - 1]
    assert [(s.model.path, s.model.device_fallback, s.model.build_mode) for s in lan.steps] == \
        [("incremental", False, 3), ("incremental", True, 0), ("rebuild", False, 0), ("incremental", False, 3)]
    assert lan.steps[2].model.why == "max_in_deg > PA_IN_STRIDE"
    row = cases[f"row-{pm.PA_OUT_STRIDE}"]
    H = g.meta["H"]
    mdl = pm.GraphModel(g.row_ptr, g.col, g.metric, g.vflags)
    mdl.step(row.steps[0].patch)
    w = layout(mdl.row_ptr, mdl.col, mdl.metric, mdl.vflags)
    assert int(np.diff(w["out_ptr"].astype(np.int64))[H]) == pm.PA_OUT_STRIDE        # all 512 links kept: the staged out-row is full
    over = cases[f"row-{pm.PA_OUT_STRIDE + 1}"]
    assert [s.model.build_mode for s in over.steps] == [pm.MODE_HUB, pm.MODE_REBUILD] and over.steps[0].model.why == "row > PA_OUT_STRIDE"


def test_chain_changes_path_at_every_step(cases):
    got = [(s.model.path, s.model.device_fallback, s.model.build_mode, s.model.grown) for s in cases["chain"].steps]
    assert got == [("incremental", False, 3, False), ("incremental", True, 0, False), ("rebuild", False, 0, False), ("incremental", False, 3, False),
                   ("cost", False, 2, False), ("rebuild", False, 0, False), ("incremental", False, 3, False), ("rebuild", False, 0, True),
                   ("incremental", False, 3, False)]
    assert cases["chain"].steps[5].model.why == "tw_work > bound" and cases["chain"].steps[7].model.why == "arena growth"


def test_random_rounds_are_mostly_incremental(cases):
    case = cases[f"random-{pm.RANDOM_SEED}"]
    rounds = case.steps[:pm.RANDOM_ROUNDS]
    assert all(10 <= len(s.patch.vs) <= 150 for s in rounds)
    assert sum(s.model.path == "incremental" for s in rounds) >= 6, [(s.tag, s.model.path, s.model.why) for s in rounds]
    assert not any(s.model.device_fallback for s in rounds)


def affected_by_sets(row_ptr, col, vs, rows):
    a = set()
    for v, (c, _) in zip(vs, rows):
        a.add(int(v))
        a.update(int(t) for t in col[row_ptr[v]:row_ptr[v + 1]])
        a.update(int(t) for t in c)
    return a


@pytest.mark.parametrize("seed", range(5))
def test_vectorised_model_equals_the_obvious_restatement(seed):
    g = synth.random_lsdb(60 + 20 * seed, 5, 3.0, 3100 + seed, metric_hi=5, p_oneway=0.2, p_parallel=0.3, p_noexpand=0.1)
    rng = np.random.default_rng(seed)
    mdl = pm.GraphModel(g.row_ptr, g.col, g.metric, g.vflags)
    for rnd in range(6):
        k = int(rng.integers(1, 12))
        vs = np.sort(rng.choice(g.n, size=k, replace=False))
        rows = []
        for v in vs.tolist():
            c = mdl.col[mdl.row_ptr[v]:mdl.row_ptr[v + 1]]
            c = np.concatenate([c[rng.random(len(c)) > 0.4], rng.integers(0, g.n, int(rng.integers(0, 3))).astype(np.uint32)])
            rows.append((c, rng.integers(1, 6, len(c)).astype(np.uint32)))
        rp, col = mdl.row_ptr.astype(np.int64), mdl.col
        rlen = np.diff(rp)
        want = affected_by_sets(rp, col, vs.tolist(), rows)
        work = sum(int(rlen[t]) + 1 for v, (c, _) in zip(vs.tolist(), rows) for t in list(c) + list(col[rp[v]:rp[v + 1]])) + 2 * sum(len(c) for c, _ in rows)
        pre = k + sum(len(c) for c, _ in rows) + sum(int(rlen[v]) for v in vs.tolist())
        patch = pm.Patch(vs, rows, mdl.vflags[vs])
        legacy, stop = pm.legacy_affected(rp, col, patch)
        d = mdl.step(patch)
        assert set(d.affected.tolist()) == want and d.na == len(want) and stop is None and set(legacy.tolist()) == want
        assert d.tw_work == work and d.pre_dedup == pre and d.e_new == len(mdl.col)
        w = layout(mdl.row_ptr, mdl.col, mdl.metric, mdl.vflags)
        assert np.array_equal(np.diff(w["in_ptr"].astype(np.int64)), mdl.kin)
