"""The host side of the randomised fast-reroute run (tools/gpu_fuzz.py: frr_case, frr_compare), without a GPU: for exactly the seed
ranges tests/test_gpu_frr_fuzz.py runs, the MODELS must show every class the run exists for (a range that shows none of a class
proves nothing about it), and a deliberately wrong expected side must fail with a line that names the call.

Model time per range, measured on one CPU core of the build machine (expected outputs of every step plus the chains' own models;
frr_case is cached per seed, so the engine parametrisations of the GPU tests pay it once) and the counters of each range
(LAN primaries / refused for the LAN; slots whose LAN conditions removed PQ members / whose PQ node moved; TI-LFA node / pair
winners; destinations with a node-protecting PQ node; backups LFA, NODE, PAIR, NOTHING; roots with a second mask word;
steps whose roots' K differ):

    first step only   40..51   1.9 s   909 / 247   272 / 83    497 / 35   946   802, 175,   7, 210   1   6
                      70..81   2.6 s   716 / 358   403 / 181   890 / 16   708   746, 242,  27, 467   5   9
                      96..107  2.2 s   634 / 215   218 / 69    467 / 33   352   488,  58,  20, 320   2   5
    with patches     166..177  2.5 s, 28 steps;    232..243  2.9 s, 19 steps (both: structural and cost-only patches, and a patch
                                                   that changed an expected output)

A root with several hundred slots costs the models seconds to minutes (the node-protecting lists are a triple loop), hence
FRR_MAX_SLOTS and LANs of at most 62 routers; the ranges were chosen on the CPU among 300 seeds (147 s in all, 19 s the dearest)."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gpu_fuzz  # noqa: E402

PLAIN = {40: 12, 70: 12, 96: 12}              # first seed: seeds (tests/test_gpu_frr_fuzz.py: patches=False)
PATCHED = {166: 12, 232: 12}                  # (patches=True)


def counters(first, count, patches):
    m = gpu_fuzz._m()
    c = dict(lan_primary=0, lan_refused=0, pq_lost=0, pq_moved=0, ti_node=0, ti_pair=0, np_pq=0, bk=np.zeros(7, np.int64), two_words=0, mixed_k=0,
             structural=0, cost_only=0, patch_changed=0, steps=0, no_cand=0, one_slot=0, one_lan=0, two_lans=0)
    for seed in range(first, first + count):
        steps = gpu_fuzz.frr_case(seed)
        prev = None
        for s in steps if patches else steps[:1]:
            w = s.models
            per = s.plan[1]
            Ks = [len(c_.nbr) for _, c_, *_ in per]
            c["steps"] += 1
            c["two_words"] += sum(k > 64 for k in Ks)
            c["mixed_k"] += len(set(Ks)) > 1
            c["no_cand"] += sum(not (c_.nbr != m.M.NONE).any() for _, c_, *_ in per)
            c["one_slot"] += sum(k == 1 for k in Ks)
            for _, _, _, lan, _ in per:
                lans = len({int(x) for x in lan if x != m.M.NONE})
                c["one_lan"] += lans == 1
                c["two_lans"] += lans >= 2
            for a in w["lfa_lan"]:
                c["lan_primary"] += int(a.coverage[5]); c["lan_refused"] += int(a.coverage[6])
            for r in w["rlfa_lan"]:
                c["pq_lost"] += int((r.pq_counts[:, 4] > 0).sum())
                c["pq_moved"] += int(((r.plain.pq_node != r.pq_node) & (r.plain.pq_node != m.M.NONE) & (r.pq_node != m.M.NONE)).sum())
            for t in w["tilfa"] + w["tilfa_lan"]:
                c["ti_node"] += int((t.ti_kind == m.T.KIND_NODE).sum()); c["ti_pair"] += int((t.ti_kind == m.T.KIND_PAIR).sum())
            c["np_pq"] += sum(int(d.nd_coverage[m.N.D_PQ]) for d in w["dest"])
            for b in w["backup"] + w["backup_lan"]:
                c["bk"] += b.bk_coverage[:7]
            if s.patch is not None:
                c["cost_only" if s.costs_only else "structural"] += 1
                now, was = s.want, prev.want
                c["patch_changed"] += any(now[k][f].shape != was[k][f].shape or not np.array_equal(now[k][f], was[k][f])
                                          for k in ("lfa_lan_device", "rlfa_lan_device", "tilfa_device", "routes_backup_lan_device", "rlfa_node_device") for f in now[k])
            prev = s
    return c


def check_classes(c):
    m = gpu_fuzz._m()
    assert c["lan_primary"] > 0 and c["lan_refused"] > 0, c
    assert c["pq_lost"] > 0 and c["pq_moved"] > 0, c
    assert c["ti_node"] > 0 and c["ti_pair"] > 0 and c["np_pq"] > 0, c
    assert all(c["bk"][k] > 0 for k in (m.B.NOTHING, m.B.LFA, m.B.NODE, m.B.PAIR)), c
    assert c["two_words"] > 0 and c["mixed_k"] > 0, c


@pytest.mark.parametrize("first", sorted(PLAIN))
def test_each_unpatched_range_shows_every_class_on_the_models(first):
    c = counters(first, PLAIN[first], False)
    print(first, c)
    check_classes(c)
    assert c["steps"] == PLAIN[first]


@pytest.mark.parametrize("first", sorted(PATCHED))
def test_each_patched_range_shows_every_class_and_patches_that_matter(first):
    c = counters(first, PATCHED[first], True)
    print(first, c)
    check_classes(c)
    assert c["structural"] > 0 and c["cost_only"] > 0 and c["patch_changed"] > 0 and c["steps"] > PATCHED[first], c


def test_the_root_shapes_occur_over_the_ranges():
    tot = {}
    for ranges, patches in ((PLAIN, False), (PATCHED, True)):
        for first, count in ranges.items():
            for k, v in counters(first, count, patches).items():
                tot[k] = tot.get(k, 0) + v
    print(tot)
    assert tot["no_cand"] > 0 and tot["one_slot"] > 0 and tot["one_lan"] > 0 and tot["two_lans"] > 0 and tot["two_words"] > 0, tot


def test_frr_case_is_deterministic_and_its_patches_are_the_splices():
    from holo_amd import engine as E
    gpu_fuzz.frr_case.cache_clear()
    a = gpu_fuzz.frr_case(166)
    gpu_fuzz.frr_case.cache_clear()
    b = gpu_fuzz.frr_case(166)
    assert len(a) == len(b) > 1
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x.graph, y.graph)) and x.prot == y.prot and vars(x.opt).keys() == vars(y.opt).keys()
        assert all(np.array_equal(x.want[k][f], y.want[k][f]) for k in x.want for f in x.want[k])
    for prev, s in zip(a, a[1:]):
        g = E.splice_rows(*prev.graph, s.patch.vs, [c for c, _ in s.patch.rows], [m for _, m in s.patch.rows], s.patch.flags)
        assert all(np.array_equal(p, q) for p, q in zip(g, s.graph))


def _step_with_two_different_roots():
    for first, count in PLAIN.items():
        for seed in range(first, first + count):
            s = gpu_fuzz.frr_case(seed)[0]
            w = s.want
            if len(s.prot) >= 2 and all(any(not np.array_equal(w[k][f][0], w[k][f][1]) for f in w[k]) for k in w):
                return s
    raise AssertionError("no step whose first two roots differ in every call")


def test_a_wrong_expected_side_fails_with_a_line_that_names_the_call():
    """The comparison of fuzz_frr driven without a device: the model's arrays as `got`; the expected side with the first two
    protected roots' models swapped (the chains have one root: a coverage word is changed instead).  Every call is named."""
    s = _step_with_two_different_roots()
    got = copy.deepcopy(s.want)
    lines = []
    assert gpu_fuzz.frr_compare(s.want, got, gpu_fuzz.frr_reporter(s.seed, 0, "none", lines)) == 0 and not lines
    for call in s.want:
        bad = dict(s.want)
        bad[call] = {f: np.concatenate([a[1:2], a[0:1], a[2:]]) for f, a in s.want[call].items()}
        lines = []
        assert gpu_fuzz.frr_compare(bad, got, gpu_fuzz.frr_reporter(s.seed, 0, "none", lines)) > 0
        assert lines and all(f"seed={s.seed} step=0 engine=none call={call} root=" in x for x in lines), (call, lines[:2])
        assert {x.split(" root=")[1].split()[0] for x in lines} <= {"0", "1"}
    got = copy.deepcopy(s.chain)
    for call in s.chain:
        bad = copy.deepcopy(s.chain)
        f = [k for k in bad[call] if k.endswith("coverage")][0]
        bad[call][f][0, 0] += 1
        lines = []
        assert gpu_fuzz.frr_compare(bad, got, gpu_fuzz.frr_reporter(s.seed, 0, "none", lines)) == 1
        assert f"call={call} root=0 field={f} idx=[[0]]" in lines[0], lines
