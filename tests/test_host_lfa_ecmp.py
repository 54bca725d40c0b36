"""Per-primary alternates of ECMP destinations on the CPU side: the new symbol in header, ctypes table and library; the numpy model
(tests/_lfa_ecmp_model.py) pinned on hand cases with the expected arrays written out, against shortest-path DAG walks on 24 small
graphs, and against the existing LFA model — so that what the GPU tests compare against is checked independently of the engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lfa_ecmp_cases as C
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
    m = re.search(r"\bint hspf_lfa_ecmp_device\(([^;]*?)\);", hdr, re.S)
    assert m, "hspf_lfa_ecmp_device is not declared"
    assert len(m.group(1).split(",")) == 13 and hasattr(lib, "hspf_lfa_ecmp_device")
    assert table["hspf_lfa_ecmp_device"][0] is ctypes.c_int and len(table["hspf_lfa_ecmp_device"][1]) == 13
    assert lib.hspf_abi_version() == 8                                   # additions only
    for c_name, py in (("HSPF_LFA_EA_PRIMARY", E.LFA_EA_PRIMARY), ("HSPF_LFA_ECMP_COVERAGE_WORDS", E.LFA_ECMP_COVERAGE_WORDS)):
        assert int(re.search(r"#define " + c_name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr).group(1), 0) == py, c_name
    assert (EM.EA_PRIMARY, EM.COVERAGE_WORDS) == (E.LFA_EA_PRIMARY, E.LFA_ECMP_COVERAGE_WORDS)
    fields = [f for f, _ in _lib.HspfLfaEcmpOut._fields_]
    assert fields == re.findall(r"\*(ea_[a-z]+);", re.search(r"typedef struct \{([^}]*)\} hspf_lfa_ecmp_out;", hdr).group(1))


def test_a_null_context_is_an_argument_error_as_for_the_other_frr_calls():
    from holo_amd import _lib
    lib = _lib.load()
    total = ctypes.c_uint64(7)
    out = _lib.HspfLfaEcmpOut()
    prot = (_lib.HspfLfaProtect * 1)()
    rc = lib.hspf_lfa_ecmp_device(None, 4, 1, 1, None, None, None, prot, 1, 0, 0, ctypes.byref(out), ctypes.byref(total))
    lout = _lib.HspfLfaOut()
    assert rc == lib.hspf_lfa_device(None, 4, 1, 1, None, None, None, prot, 1, 0, ctypes.byref(lout)) == -1      # HSPF_E_INVAL
    assert total.value == 7


def _same(got: EM.Ecmp, want):
    for name, w in zip(EM.FIELDS, want):
        assert np.array_equal(getattr(got, name), w), (name, getattr(got, name), w)


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_model_on_the_hand_cases(name):
    case = C.HAND[name]()
    _, got = EM.model(case[0], case[1], C.RUN_FLAGS.get(name, 0), case[2])
    _same(got, C.expected(case))
    if name == "lan":                     # both entries without an alternate: the destination is not counted as fully protected
        assert got.ea_slot.tolist() == [M.NONE, M.NONE] and got.ea_coverage[6] == 0 and got.ea_coverage[0] == 1


def test_model_a_primary_towards_a_network_vertex_is_protected_and_never_offered():
    g, root, lf, _ = C.network_primary()
    c, got = EM.model(g, root, C.RUN_FLAGS["network_primary"], lf, sets=True)
    assert c.nbr.tolist() == [M.NONE, 1, M.NONE, 1] and c.root_link.tolist() == [0, 1, 0, 0] and c.cost.tolist() == [2, 1, 2, 2]
    assert got.ea_dest.tolist() == [2, 2] and got.ea_primary.tolist() == [0, 1]                       # both of the LAN's primaries are protected
    assert not got.cand[:, c.nbr == M.NONE].any() and not got.node.any()                             # ... slot 0 is offered to nobody


# ---- the model against walks over the shortest-path DAG -------------------------------------------------------------------------

def _on_shortest_paths(adj, src, dst):
    """The vertices that lie on at least one shortest path src -> dst, by enumerating every such path (Dijkstra for the distances,
    then a depth-first walk of the tight links)."""
    import heapq
    dist = {src: 0}
    pq = [(0, src)]
    while pq:
        d, v = heapq.heappop(pq)
        if d > dist[v]:
            continue
        for t, c in adj[v]:
            if d + c < dist.get(t, 1 << 62):
                dist[t] = d + c
                heapq.heappush(pq, (d + c, t))
    if dst not in dist:
        return None
    seen = set()

    def walk(v, path):
        if v == dst:
            seen.update(path)
            return
        for t, c in adj[v]:
            if dist[v] + c == dist.get(t):
                walk(t, path + [t])
    walk(src, [src])
    return seen


def test_model_equals_shortest_path_dag_walks_on_24_graphs():
    with_ecmp = 0
    for seed in C.SMALL_SEEDS:
        g, root = C.small_graph(seed)
        rp, col, met, _ = g
        adj = [[(int(col[k]), int(met[k])) for k in range(rp[v], rp[v + 1])] for v in range(len(rp) - 1)]
        c, got = EM.model(g, root, sets=True)
        with_ecmp += got.total > 0
        for e in range(got.total):
            h, Dv = int(got.ea_primary[e]), int(got.ea_dest[e])
            for k in range(len(c.nbr)):
                on = _on_shortest_paths(adj, int(c.nbr[k]), Dv)
                is_cand = k != h and root not in on and c.root_link[k] != c.root_link[h]
                assert bool(got.cand[e, k]) == is_cand, (seed, e, k)
                assert bool(got.node[e, k]) == (is_cand and int(c.nbr[h]) not in on), (seed, e, k)
    assert with_ecmp >= 12, with_ecmp


# ---- against the existing LFA model ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", C.SMALL_SEEDS[:12])
def test_model_against_the_lfa_model(seed):
    g, root = C.small_graph(seed)
    c, _, nbr_row, _, t = EM.tables(g, root)
    old = M.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row)
    got = EM.lfa_ecmp(t.dist, t.flags, t.mask, c, 0, nbr_row, sets=True)
    _, inP = EM.primaries(t.dist, t.flags, t.mask, c, 0)
    K = len(c.nbr)
    bit = lambda m, d, k: bool((int(m[d, k // 64]) >> (k % 64)) & 1)
    for Dv in np.unique(got.ea_dest):
        ent = np.flatnonzero(got.ea_dest == Dv)
        for k in range(K):
            if inP[k, Dv]:
                continue                   # the old sets never hold a primary
            assert bit(old.cand_mask, Dv, k) == bool(got.cand[ent, k].all()), (seed, Dv, k)
            assert bit(old.node_mask, Dv, k) == bool(got.node[ent, k].all()), (seed, Dv, k)
    # the per-primary rule on destinations with ONE primary is hspf_lfa_device's choice
    one = EM.lfa_ecmp(t.dist, t.flags, t.mask, c, 0, nbr_row, min_primaries=1)
    single = np.flatnonzero(inP.sum(0) == 1)
    e = one.ea_ptr[single]
    assert len(single) and np.array_equal(one.ea_ptr[single + 1] - e, np.ones(len(single), np.uint32))
    assert np.array_equal(one.ea_slot[e], old.alt_slot[single]) and np.array_equal(one.ea_metric[e], old.alt_metric[single])
    three = M.LINK_PROTECT | M.NODE_PROTECT | M.DOWNSTREAM
    assert np.array_equal(one.ea_flags[e] & three, old.alt_flags[single] & three) and not (one.ea_flags[e] & EM.EA_PRIMARY).any()


@pytest.mark.parametrize("seed", C.SMALL_SEEDS[:12])
def test_model_ptr_total_and_entry_order(seed):
    g, root = C.small_graph(seed)
    c, _, nbr_row, _, t = EM.tables(g, root)
    got = EM.lfa_ecmp(t.dist, t.flags, t.mask, c, 0, nbr_row)
    _, inP = EM.primaries(t.dist, t.flags, t.mask, c, 0)
    npri = inP.sum(0)
    assert got.ea_ptr[0] == 0 and got.ea_ptr[-1] == got.total
    assert np.array_equal(np.diff(got.ea_ptr.astype(np.int64)), np.where(npri >= 2, npri, 0))
    assert np.all(np.diff(got.ea_dest.astype(np.int64)) >= 0)                                  # D ascending
    for Dv in np.unique(got.ea_dest):
        assert got.ea_primary[got.ea_ptr[Dv]:got.ea_ptr[Dv + 1]].tolist() == np.flatnonzero(inP[:, Dv]).tolist()       # h ascending


def test_no_device_is_an_error_code_from_the_python_layer():
    """Without a GPU the context cannot be made: the call is reachable only through a context, as every FRR call."""
    from holo_amd import engine as E
    import inspect
    assert "cap_entries" in inspect.signature(E.SpfContext.lfa_ecmp_device).parameters
    assert "lfa_flags" in inspect.signature(E.SpfContext.lfa_ecmp).parameters
