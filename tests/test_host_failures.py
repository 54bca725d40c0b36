"""Failure-scenario rows on the CPU side: the reference construction pinned on three hand graphs whose post-failure trees are written
out by hand, the symbol in header / ctypes table / library, the argument errors that need no GPU, and the compiled driver's two CPU
legs over the shared case list (tests/_failure_cases.py): the host twin (hspf::host::run_failures_sequential) and the oracle engine
standing in for the GPU engine, both against the oracle's rows."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _failure_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "failures_driver")
LINE = re.compile(r"(\d+) cases, (\d+) rows compared, (\d+) entries differ")
INF = F.INF


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    from oracle import graph_oracle as go
    go.build()
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("failures_driver")


def test_header_ctypes_and_library_agree_on_the_symbols():
    from holo_amd import build, _lib
    from holo_amd import engine as E
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in ("hspf_run_failures", "hspf_run_failures_device"):
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == 7 and hasattr(lib, name)
        assert table[name][0] is ctypes.c_int and len(table[name][1]) == 7
    assert lib.hspf_abi_version() == 8                                   # additions only
    for k, v in (("NONE", E.FAIL_NONE), ("ROOT_LINK", E.FAIL_ROOT_LINK), ("VERTEX", E.FAIL_VERTEX)):
        assert int(re.search(r"#define HSPF_FAIL_" + k + r"\s+(\d+)u", hdr).group(1)) == v
    assert (F.NONE, F.ROOT_LINK, F.VERTEX) == (E.FAIL_NONE, E.FAIL_ROOT_LINK, E.FAIL_VERTEX)
    assert ctypes.sizeof(_lib.HspfFailure) == 8


def test_a_null_context_is_an_argument_error():
    from holo_amd import _lib
    lib = _lib.load()
    res = _lib.HspfResult()
    roots = (ctypes.c_uint32 * 1)(0)
    fail = (_lib.HspfFailure * 1)()
    assert lib.hspf_run_failures(None, None, roots, fail, 1, 0, ctypes.byref(res)) == -1
    assert lib.hspf_run_failures_device(None, None, roots, fail, 1, 0, ctypes.byref(res)) == -1


def test_the_python_layer_has_the_calls():
    import inspect
    from holo_amd import engine as E
    assert "failures" in inspect.signature(E.SpfContext.run_failures).parameters
    assert "dist_ptr" in inspect.signature(E.SpfContext.run_failures_device).parameters
    assert "node" in inspect.signature(E.SpfContext.post_convergence).parameters


# ---- the construction itself, on three hand graphs ---------------------------------------------------------------------------------

def test_construction_square_link_failure():
    """Square 0 - 1 - 2 - 3 - 0, unit costs, rows [1, 3], [0, 2], [1, 3], [2, 0].  Root 0 loses link 0 (to 1): 1 is reached the way
    round at 3 through slot 1, 2 at 2 and 3 at 1 through slot 1 too."""
    g = F.csr(F.both(4, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1)]))
    ref = F.reference(g, INF, [0], [(F.ROOT_LINK, 0)])
    assert ref.dist[0].tolist() == [0, 3, 2, 1] and ref.hops[0].tolist() == [0, 3, 2, 1] and ref.flags[0].tolist() == [1, 1, 1, 1]
    assert ref.mask[0, :, 0].tolist() == [0, 2, 2, 2]


def test_construction_vertex_failure_on_a_chain_with_a_chord():
    """0 - 1 - 2 - 3 with the chord 0 - 2 at 5.  Without 1: 2 at 5 and 3 at 6 through slot 1 (the chord), 1 not in the tree."""
    g = F.csr(F.both(4, [(0, 1, 1), (0, 2, 5), (1, 2, 1), (2, 3, 1)]))
    ref = F.reference(g, INF, [0], [(F.VERTEX, 1)])
    assert ref.dist[0].tolist() == [0, INF, 5, 6] and ref.hops[0].tolist() == [0, 0, 1, 2] and ref.flags[0].tolist() == [1, 0, 1, 1]
    assert ref.mask[0, :, 0].tolist() == [0, 0, 2, 2]


def test_construction_lan_failure_keeps_the_slot_numbering():
    """Routers 0, 1 on the LAN 2 (router -> LAN 10, LAN -> router 0) and 0 - 1 at 50, rows [2, 1], [2, 0], [0, 1].  Root 0 has slots
    0, 1 of its own row and 2, 3 of the pseudonode's.  Plain: 1 at 10 through slot 3 (the LAN's link to 1).  Without the LAN: 1 at 50
    through slot 1 — the positions did not move."""
    g = F.csr([[(2, 10), (1, 50)], [(2, 10), (0, 50)], [(0, 0), (1, 0)]], [0, 0, 1])
    plain = F.reference(g, INF, [0], [(F.NONE, 0)])
    assert plain.dist[0].tolist() == [0, 10, 10] and plain.mask[0, :, 0].tolist() == [0, 8, 0]
    ref = F.reference(g, INF, [0], [(F.VERTEX, 2)])
    assert ref.dist[0].tolist() == [0, 50, INF] and ref.mask[0, :, 0].tolist() == [0, 2, 0] and ref.flags[0].tolist() == [1, 1, 0]
    link = F.reference(g, INF, [0], [(F.ROOT_LINK, 0)], F.NET_NEXTHOPS)
    assert link.dist[0].tolist() == [0, 50, 60] and link.mask[0, :, 0].tolist() == [0, 2, 2]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_every_case_takes_the_branch_it_names(name, wide):
    from oracle import graph_oracle as go
    go.build()
    F.run_check(F.CASES[name], wide)


@pytest.mark.parametrize("extra", F.EXTRAS)
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_every_case_takes_its_branch_at_every_width(name, extra):
    """130, 300, 520 and 960 spokes at the case's first root: the oracle needs 3, 5, 9 and 16 mask words (run_check asserts it) and
    every case's own check still holds."""
    from oracle import graph_oracle as go
    go.build()
    F.run_check(F.CASES[name], extra=extra)


@pytest.mark.parametrize("name,extra", [(n, e) for n, c in sorted(F.WIDE_CASES.items()) for e in sorted(c.words)])
def test_the_wide_only_cases_take_their_branch(name, extra):
    from oracle import graph_oracle as go
    go.build()
    c = F.WIDE_CASES[name]
    g, ref = F.run_check(c, extra=extra or None)
    assert ref.mask.shape[2] == c.words[extra] > 1


def test_the_case_list_has_the_new_branches_and_one_word_bases():
    """The cases the wide GPU tests lean on are there; every case of CASES fits one mask word unwidened with at most 20 slots (what
    the table F.WORDS assumes), the hop-count-like ones are hop-count-like and the others are not (run_check asserts both)."""
    assert {"high_slot_detour", "giant_row_far", "hub_far_link", "hopcount_lan_first_parent"} <= set(F.CASES) and "giant_row_member" in F.WIDE_CASES
    assert F.CASES["high_slot_detour"].front and F.CASES["hopcount_lan_first_parent"].hopcount
    for name, c in F.CASES.items():
        g = c.graph()
        assert max(F.slot_bases(g, int(r))[1] for r in c.roots) <= 20, name
        assert F.is_hopcount_like(g) == c.hopcount and F.is_hopcount_like(c.at(130).graph()) == c.hopcount, name
    top = F.CASES["high_slot_detour"].at(960)
    assert top.fails == [(F.ROOT_LINK, 960)] and top.graph()[1][960:962].tolist() == [1, 5]


def test_the_hopcount_sweep_is_hopcount_like_and_sees_failures_bite():
    """Non-vacuity of the seeded hop-count-like graphs of tests/test_gpu_failures_wide.py, on the CPU oracle: all 20 have the shape,
    20 to 60 vertices and three router roots; failures of network vertices occur in every graph, and nearly every row differs from
    the plain row of its root."""
    from oracle import graph_oracle as go
    go.build()
    rows = nets = bite = 0
    for seed in F.HOPCOUNT_SEEDS:
        c = F.hopcount_random(seed)
        g = c.graph()
        assert F.is_hopcount_like(g) and 20 <= len(c.vf) <= 60 and len(set(c.roots)) == 3 and not any(c.vf[r] & F.NET for r in c.roots)
        ref = F.reference(g, c.maxp, c.roots, c.fails)
        plain = F.reference(g, c.maxp, c.roots, [(F.NONE, 0)] * len(c.roots))
        assert ref.mask.shape[2] == 1
        k = sum(1 for kind, a in c.fails if kind == F.VERTEX and c.vf[a] & F.NET)
        assert k >= 3
        nets += k
        rows += len(c.roots)
        bite += sum(F._differs(ref, plain, r) for r in range(len(c.roots)))
    assert rows >= 200 and nets >= 100 and bite >= rows * 9 // 10, (rows, nets, bite)


def test_the_protocol_sweep_patches_half_and_sees_failures_bite():
    """Non-vacuity of the protocol sweep of tests/test_gpu_failures.py, on the CPU oracle: about half of its 40 graphs really lose
    a link to the patch, and in most graphs a failure row differs from the plain row of its root."""
    class Mirror:                                                          # the patch applied to nothing: only the spliced CSR is wanted
        def patch(self, *a):
            pass
    patched = bite = 0
    for seed in range(40):
        graph, maxp, flags = F.protocol_graph(seed)
        if seed % 4 >= 2:
            graph, did = F.drop_last_link(Mirror(), graph)
            patched += did
        routers = np.flatnonzero((graph[3] & 1) == 0)
        S = int(routers[np.argmax(np.diff(graph[0].astype(np.int64))[routers])])
        sc = F.all_scenarios(graph, S)
        if not sc:
            continue
        ref = F.reference(graph, maxp, [S] * len(sc), sc, flags)
        plain = F.reference(graph, maxp, [S], [(F.NONE, 0)], flags)
        bite += any(not np.array_equal(ref.dist[i], plain.dist[0]) or not np.array_equal(ref.mask[i], plain.mask[0]) for i in range(len(sc)))
    assert patched >= 18 and bite >= 30, (patched, bite)


# ---- the compiled driver's CPU legs ------------------------------------------------------------------------------------------------

def _files(tmp_path):
    files = F.driver_files(tmp_path, names=sorted(F.CASES))
    graph, maxp, S, roots, fails = F.batch130()
    ref = F.reference(graph, maxp, roots, fails)
    p = tmp_path / "failures_batch130.txt"
    F.write_case_file(p, graph, maxp, roots, fails, 0, ref)
    return files + [str(p)]


@pytest.mark.parametrize("engine", ["host", "oracle"])
def test_driver_cpu_legs_reproduce_the_oracle_rows(tmp_path, engine):
    _build_driver()
    files = _files(tmp_path)
    out = subprocess.run([DRIVER, "--engine", engine, "--oracle-so", os.path.join(ROOT, "oracle", "liboracle_spf.so")] + files,
                         capture_output=True, text=True, timeout=300)
    m = LINE.search(out.stdout)
    assert out.returncode == 0 and m, out.stdout + out.stderr
    assert int(m.group(1)) == len(files) and int(m.group(2)) >= len(files) + 129 and int(m.group(3)) == 0


@pytest.mark.parametrize("engine", ["host", "oracle"])
def test_driver_cpu_legs_at_every_width_and_on_hopcount_graphs(tmp_path, engine):
    """The host twin and the model on F.wide_runs(): every case at 3, 5, 9 and 16 mask words, the wide-only cases, the seeded
    hop-count-like graphs at one word and at five."""
    _build_driver()
    files = F.driver_files_wide(tmp_path)
    assert len(files) == 4 * len(F.CASES) + 4 + 2 * len(F.HOPCOUNT_SEEDS)
    out = subprocess.run([DRIVER, "--engine", engine, "--oracle-so", os.path.join(ROOT, "oracle", "liboracle_spf.so")] + files,
                         capture_output=True, text=True, timeout=300)
    m = LINE.search(out.stdout)
    assert out.returncode == 0 and m, out.stdout[-2000:] + out.stderr[-2000:]
    assert int(m.group(1)) == len(files) and int(m.group(2)) >= 2 * len(files) and int(m.group(3)) == 0
