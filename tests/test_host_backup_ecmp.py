"""Per-primary backups of ECMP prefixes on the CPU side: the new symbol in header, ctypes table and library; the plain-Python model
(tests/_backup_ecmp_model.py) pinned on hand cases with the expected arrays written out, against shortest-path walks on seeded
graphs with multi-homed prefixes, against the per-vertex model on single-homed prefixes, and against the plain per-prefix model's
sets — so that what the GPU tests compare against is checked independently of the engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import _backup_cases as BC
import _backup_ecmp_cases as C
import _backup_ecmp_model as BE
import _backup_model as B
import _lfa_ecmp_model as EM
import _lfa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_ctypes_and_library_agree_on_the_symbol():
    from holo_amd import build, _lib
    from holo_amd import engine as E
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"\bint hspf_routes_backup_ecmp_device\(([^;]*?)\);", hdr, re.S)
    assert m, "hspf_routes_backup_ecmp_device is not declared"
    assert len(m.group(1).split(",")) == 16 and hasattr(lib, "hspf_routes_backup_ecmp_device")
    assert table["hspf_routes_backup_ecmp_device"][0] is ctypes.c_int and len(table["hspf_routes_backup_ecmp_device"][1]) == 16
    assert lib.hspf_abi_version() == 8                                   # additions only
    assert int(re.search(r"#define HSPF_BK_ECMP_COVERAGE_WORDS\s+(\d+)u", hdr).group(1)) == E.BK_ECMP_COVERAGE_WORDS == BE.COVERAGE_WORDS
    assert (BE.LFA, BE.NODE, BE.PAIR, BE.NOTHING) == (E.BK_LFA, E.BK_NODE, E.BK_PAIR, E.BK_NONE)
    assert (BE.NODE_PROTECT, BE.DOWNSTREAM, BE.EA_PRIMARY) == (E.LFA_NODE_PROTECT, E.LFA_DOWNSTREAM, E.LFA_EA_PRIMARY)
    fields = [f for f, _ in _lib.HspfBackupEcmpOut._fields_]
    assert fields == re.findall(r"\*(eb_[a-z]+);", re.search(r"typedef struct \{([^}]*)\} hspf_backup_ecmp_out;", hdr).group(1)) == list(BE.FIELDS)
    assert "not yet" not in hdr                                           # the six "per prefix: not yet" sentences point to the call now


def test_a_null_context_is_an_argument_error_as_for_the_other_frr_calls():
    from holo_amd import _lib
    lib = _lib.load()
    total = ctypes.c_uint64(7)
    out = _lib.HspfBackupEcmpOut()
    prot = (_lib.HspfLfaProtect * 1)()
    rc = lib.hspf_routes_backup_ecmp_device(None, 4, 1, 1, None, None, None, prot, 1, 0, None, None, None, 0, ctypes.byref(out), ctypes.byref(total))
    assert rc == -1 and total.value == 7                                  # HSPF_E_INVAL


def test_the_python_layer_has_the_call_the_result_and_the_switch():
    import inspect
    from holo_amd import engine as E
    assert "cap_entries" in inspect.signature(E.SpfContext.routes_backup_ecmp_device).parameters
    assert inspect.signature(E.SpfContext.backup_routes).parameters["ecmp"].default is False
    r = E.BackupEcmpResult(np.array([0, 0, 2], np.uint32), np.array([0, 1], np.uint32), np.array([3, 6], np.uint8), np.array([1, 0xFFFFFFFF], np.uint32),
                           np.array([6, 0], np.uint32), np.array([0x38, 0], np.uint8), np.zeros((1, 8), np.uint32), n_prefixes=2)
    assert r.total == 2 and r.entries(0, 0) == [] and r.entries(0, 1) == [(0, 3, 1, 6, 0x38), (1, 6, 0xFFFFFFFF, 0, 0)]


# ---- hand cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.HAND))
def test_model_on_the_hand_cases(name):
    case = C.HAND[name]()
    model = C.Model(case[0], [case[1]], case[2])
    got = BE.want(model, case[3], False)[0]
    for f, w in zip(BE.FIELDS, C.expected(case)):
        assert np.array_equal(getattr(got, f), w), (f, getattr(got, f), w)


def test_model_ecmp_only_per_prefix_where_the_per_vertex_call_is_silent():
    g, S, t, _, _ = C.two_homes()
    model = C.Model(g, [S], t)
    f = model.fwd
    per_vertex = EM.lfa_ecmp(f.dist, f.flags, f.mask, model.cands[0], 0, model.nbr_row[0])
    assert per_vertex.total == 0 and BE.want(model, 0, False)[0].total == 2


def test_model_an_alternate_for_the_prefix_that_is_none_for_the_attaining_vertex_and_node_protection_the_other_way():
    g, S, t, _, _ = C.prefix_not_vertex()
    model = C.Model(g, [S], t)
    f, c = model.fwd, model.cands[0]
    got = BE.want(model, 0, False, sets=True)[0]
    per_vertex = EM.lfa_ecmp(f.dist, f.flags, f.mask, c, 0, model.nbr_row[0], sets=True)
    assert got.cand == [{1, 2}, {0, 2}]                                            # C (slot 2) for the prefix ...
    e = np.flatnonzero(per_vertex.ea_dest == 4)
    assert len(e) == 2 and not per_vertex.cand[e, 2].any()                        # ... and not for X = 4, the vertex S's route uses
    # the converse, over the seeded graphs: a slot that protects the NODE E on the way to the attaining vertex and not on the way to
    # the prefix (E itself is nearer to another advertiser), and a member of the per-vertex cand is always a member here
    converse = 0
    for seed in C.GPU_SEEDS:
        g, S, t = C.random_multihomed(seed)
        model = C.Model(g, [S], t)
        f, c, nr, r = model.fwd, model.cands[0], model.nbr_row[0], model.routes()
        w = BE.want(model, 0, False, sets=True)[0]
        for e in range(w.total):
            p, h = int(w.eb_prefix[e]), int(w.eb_primary[e])
            X, E = int(t.vertex[r.best_entry[p]]), int(c.nbr[h])
            if E == M.NONE:
                continue
            for k in w.cand[e] - w.node[e]:
                dN = f.dist[nr[k]]
                converse += int(dN[X]) < int(dN[E]) + int(f.dist[nr[h]][X])
    assert converse > 0


# ---- shortest-path walks ------------------------------------------------------------------------------------------------------

def test_model_equals_shortest_path_walks_on_seeded_graphs_with_multihomed_prefixes():
    """The method of tests/test_host_lfa_ecmp.py on the augmented graph of tests/_backup_cases.py, whose distances come from the CPU
    oracle: a prefix whose advertisers are plain routers becomes a vertex X_p behind them.  EVERY shortest path N -> X_p avoids a
    vertex V exactly when the way through V is longer than the distance: d(N, X_p) < d(N, V) + d(V, X_p).  A chosen alternate's
    shortest paths to the prefix avoid S — and so the first link of h, which starts at S, unless the alternate starts on that
    link itself — and a node-protecting one's avoid E."""
    from oracle import graph_oracle as go
    checked = 0
    for seed in C.GPU_SEEDS[:16]:
        g, S, t = C.random_multihomed(seed)
        model = C.Model(g, [S], t)
        c = model.cands[0]
        w = BE.want(model, 0, False, sets=True)[0]
        ga, xs = BC.augmented(g, S, t)
        n = len(g[3])
        d = go.run(*ga, 0xFFFFFFFF, np.arange(n, dtype=np.uint32), 0, go.MAP).dist.astype(np.int64)      # d[v][u], every original vertex a root
        d[d == M.INF] = 1 << 60
        for e in range(w.total):
            p, h = int(w.eb_prefix[e]), int(w.eb_primary[e])
            if p not in xs:
                continue
            X, E = xs[p], int(c.nbr[h])
            for k in range(len(c.nbr)):
                N = int(c.nbr[k])
                if N == M.NONE or k == h or g[3][N] & M.VF_NO_TRANSIT:
                    continue
                avoids_s = d[N, X] < (1 << 60) and d[N, X] < d[N, S] + d[S, X]
                is_cand = bool(avoids_s) and c.root_link[k] != c.root_link[h]
                assert (k in w.cand[e]) == is_cand, (seed, e, k)
                if E != M.NONE:
                    assert (k in w.node[e]) == (is_cand and bool(d[N, X] < d[N, E] + d[E, X])), (seed, e, k)
                checked += 1
            if w.eb_kind[e] == BE.LFA:
                assert int(w.eb_slot[e]) in w.cand[e] and bool(w.eb_flags[e] & BE.NODE_PROTECT) == (int(w.eb_slot[e]) in w.node[e])
    assert checked > 300, checked


# ---- single-homed reduction ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", C.SMALL_SEEDS[:12])
def test_single_homed_prefixes_of_metric_zero_reduce_to_the_per_vertex_entries(seed):
    import _lfa_ecmp_cases as LC
    g, root = LC.small_graph(seed)
    n = len(g[3])
    model = C.Model(g, [root], B.table([[(v, 0)] for v in range(n)]))
    f = model.fwd
    pv = EM.lfa_ecmp(f.dist, f.flags, f.mask, model.cands[0], 0, model.nbr_row[0])
    got = BE.want(model, 0, False)[0]
    assert np.array_equal(got.eb_ptr, pv.ea_ptr) and np.array_equal(got.eb_primary, pv.ea_primary)
    assert np.array_equal(got.eb_slot, pv.ea_slot) and np.array_equal(got.eb_metric, pv.ea_metric)
    assert np.array_equal(got.eb_kind, np.where(pv.ea_flags & M.LINK_PROTECT, BE.LFA, BE.NOTHING).astype(np.uint8))      # the kind mapped
    assert np.array_equal(got.eb_flags, pv.ea_flags & ~np.uint8(M.LINK_PROTECT))
    assert got.eb_coverage[:6].tolist() == pv.ea_coverage[:6].tolist() and got.eb_coverage[6] == 0 and got.eb_coverage[7] == pv.ea_coverage[6]


# ---- the plain call's set -----------------------------------------------------------------------------------------------------

def test_the_plain_models_cand_mask_is_a_subset_of_every_cand_h_and_where_it_is_not_empty_every_entry_has_an_alternate():
    nonempty = 0
    for seed in C.GPU_SEEDS:
        g, S, t = C.random_multihomed(seed)
        model = C.Model(g, [S], t)
        plain = model.want(0, False)[0]
        w = BE.want(model, 0, False, sets=True)[0]
        assert np.array_equal(np.diff(w.eb_ptr.astype(np.int64)) > 0, plain.bk_kind == B.ECMP)          # the stream speaks about the BK_ECMP prefixes
        for e in range(w.total):
            p = int(w.eb_prefix[e])
            both = {k for k in range(len(model.cands[0].nbr)) if (int(plain.bk_cand_mask[p, k // 64]) >> (k % 64)) & 1}
            assert both <= w.cand[e], (seed, e)
            if both:
                nonempty += 1
                assert w.eb_kind[e] == BE.LFA
    assert nonempty > 0


def test_one_primary_prefixes_under_the_same_rule_are_the_plain_models_choice():
    for seed in C.GPU_SEEDS[:12]:
        g, S, t = C.random_multihomed(seed)
        model = C.Model(g, [S], t)
        f = model.fwd
        plain = model.want(0, True)[0]
        one = BE.backup_ecmp(f.dist, f.flags, f.mask, model.cands[0], 0, model.nbr_row[0], t, model.routes(), 0, model.frr(0)[0][2], min_primaries=1)
        single = np.flatnonzero(np.diff(one.eb_ptr.astype(np.int64)) == 1)
        e = one.eb_ptr[single]
        assert len(single) and np.array_equal(single, np.flatnonzero(plain.bk_kind >= B.LFA))
        for name in ("kind", "primary", "slot", "metric", "flags"):
            assert np.array_equal(getattr(one, "eb_" + name)[e], getattr(plain, "bk_" + name)[single]), (seed, name)
