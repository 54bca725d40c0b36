"""Hand cases of hspf_tilfa_pc_device, at most 12 vertices each, with what the rule of include/holo_spf_hip.h ("repairs along the
post-convergence path") gives for them worked out BY HAND: tests/test_host_tilfa_pc.py holds the model to these, the GPU and C++
tests hold the engine to the model.  None of them passes alt_flags (LFA would cover some of the destinations and hide the walk).

A case: graph, protected root S, run_flags, max_walk, and expect = {D: {field: value}}; "hops" stands for the list of
(position, head) in the order p -> q."""
import os
import re
import subprocess
from dataclasses import dataclass, field

import numpy as np

import _lfa_model as M
import _tilfa_pc_model as P

IGN_RUN, IGN_LFA = 2, 1


@dataclass
class Case:
    graph: tuple
    root: int
    expect: dict
    run_flags: int = 0
    lfa_flags: int = 0
    max_walk: int = 256
    drop: tuple = field(default_factory=tuple)

    def want(self, w_min=1):
        return P.one_root(self.graph, self.root, run_flags=self.run_flags, lfa_flags=self.lfa_flags, w_min=w_min, with_lfa=False,
                          max_walk=self.max_walk, drop=self.drop)


def one_way_ring(n):
    """0 -> 1 -> ... -> n-1 -> 0 at cost 1, the other direction at cost 10."""
    return M.csr(n, [x for v in range(n) for x in ((v, (v + 1) % n, 1), ((v + 1) % n, v, 10))])


def pos(graph, u, v, nth=0):
    """Position of the nth link u -> v in u's row."""
    rp, col = graph[0], graph[1]
    return [j for j, t in enumerate(col[rp[u]:rp[u + 1]]) if t == v][nth]


def _cases():
    C = {}
    R, F = P.D_REPAIR, (P.ON_PC, P.P_IS_ROOT, P.Q_IS_DEST)
    # (a) unit ring of six, S = 0, link 0-1: 3 is released through 5 (XP) and is in Q — p == q, no adjacency, for D = 1 and D = 2
    g = M.csr(6, M.both([(v, (v + 1) % 6, 1) for v in range(6)]))
    C["a_p_in_q"] = Case(g, 0, {1: dict(kind=R, p=3, q=3, n_adj=0, hops=[], metric=5, flags=F[0]),
                                2: dict(kind=R, p=3, q=3, n_adj=0, hops=[], metric=4, flags=F[0])})
    # (b) the five-ring of tests/test_host_tilfa.py (4-0 costs 4), S = 2, link 2-3: p = 0 in P, q = 4 in Q, one adjacency 0 -> 4
    g = M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]))
    C["b_ring_one_adj"] = Case(g, 2, {3: dict(kind=R, p=0, via=P.VIA_SELF, q=4, n_adj=1, hops=[(pos(g, 0, 4), 4)], metric=7, flags=F[0]),
                                      4: dict(kind=R, p=0, q=4, n_adj=1, hops=[(pos(g, 0, 4), 4)], metric=6, flags=F[0] | F[2])})
    # (c) five-ring with a cost per direction, S = 0, link 0-1: 4 is in P, 2 in Q, 3 in neither and 4's row has no link into Q
    #     (hspf_tilfa_device: HSPF_TILFA_NONE); the post-convergence path 0 -> 4 -> 3 -> 2 -> 1 gives 4, then 4 -> 3, 3 -> 2
    g = M.csr(5, [(0, 1, 1), (1, 0, 1), (0, 4, 1), (4, 0, 1), (4, 3, 10), (3, 4, 1), (3, 2, 10), (2, 3, 1), (2, 1, 1), (1, 2, 1)])
    C["c_two_adj"] = Case(g, 0, {1: dict(kind=R, p=4, via=P.VIA_SELF, q=2, n_adj=2, hops=[(pos(g, 4, 3), 3), (pos(g, 3, 2), 2)], metric=22, flags=F[0])})
    # (d) one-way ring of six, S = 0, link 0-1: only 5 is released (through its own slot), nothing on the way is in Q:
    #     5 -> 4 -> 3 -> 2 -> 1 for D = 1, four adjacencies;  (h) D = 2 is not in Q itself: q is the destination, three adjacencies
    g = one_way_ring(6)
    C["d_four_adj"] = Case(g, 0, {1: dict(kind=R, p=5, via=1, q=1, n_adj=4, hops=[(pos(g, 5, 4), 4), (pos(g, 4, 3), 3), (pos(g, 3, 2), 2), (pos(g, 2, 1), 1)],
                                          metric=50, flags=F[0] | F[2]),
                                  2: dict(kind=R, p=5, q=2, n_adj=3, hops=[(pos(g, 5, 4), 4), (pos(g, 4, 3), 3), (pos(g, 3, 2), 2)], metric=40, flags=F[0] | F[2])})
    # (e) one-way ring of seven: five adjacencies for D = 1
    g = one_way_ring(7)
    C["e_long"] = Case(g, 0, {1: dict(kind=P.D_LONG, p=P.NONE, q=P.NONE, n_adj=0, hops=[], metric=0, flags=0),
                              2: dict(kind=R, p=6, q=2, n_adj=4)})
    # (f) S = 1, E = 2 on a point-to-point link; 3 (in P) and 4 (in Q) share the LAN of pseudonode 0: the gap 3 -> 0 -> 4 crosses it
    links = M.both([(1, 2, 1), (1, 3, 1), (4, 2, 1)])
    for r_ in (3, 4):
        links += [(r_, 0, 10), (0, r_, 0)]
    C["f_lan_in_gap"] = Case(M.csr(5, links, net=[0]), 1, {2: dict(kind=P.D_LAN, p=P.NONE, n_adj=0, hops=[]), 4: dict(kind=P.D_LAN)})
    #     ... and the five-ring of (b) with D = 6 behind a stub LAN (pseudonode 5) of E = 3: the pseudonode is below q, not in the gap
    g = M.csr(7, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]) + [(3, 5, 1), (5, 3, 0), (6, 5, 1), (5, 6, 0)], net=[5])
    C["f_lan_below_q"] = Case(g, 2, {6: dict(kind=R, p=0, q=4, n_adj=1, hops=[(pos(g, 0, 4), 4)], metric=8, flags=F[0])})
    # (g) D = 2 is an overloaded neighbour of S = 0 whose primary is the link to 1: after the failure it hangs on S's own link, and
    #     it is not eligible: no P node on the path, p is the root and the one adjacency is S's link
    g = M.csr(3, M.both([(0, 1, 1), (1, 2, 1), (0, 2, 5)]), no_transit=[2])
    C["g_p_is_root"] = Case(g, 0, {2: dict(kind=R, p=0, via=P.NONE, q=2, n_adj=1, hops=[(pos(g, 0, 2), 2)], metric=5, flags=F[0] | F[1] | F[2])})
    # (i) S = 0, E = 1; 4 hangs on 2 (post-convergence 0 -> 2 -> 4 = 6) but 2 does not release it (5 < 1 + 1 + 3 fails); 3 does, at
    #     10 + 1 = 11: p = q = 4, the repair costs 5 more than the post-convergence path
    g = M.csr(5, M.both([(0, 1, 1), (0, 2, 1), (2, 4, 5), (0, 3, 10), (3, 4, 1), (1, 4, 3)]))
    C["i_off_pc"] = Case(g, 0, {4: dict(kind=R, p=4, via=2, q=4, n_adj=0, hops=[], metric=11, flags=F[2])})
    # (j) 2 <-> 3 at cost 0, entered from 5: parent(3) = 2, parent(2) = 3 (3 < 5): the walk circles until max_walk
    g = M.csr(6, M.both([(0, 1, 1), (1, 3, 1), (0, 5, 2), (5, 2, 4), (2, 3, 0)]))
    C["j_zero_cycle"] = Case(g, 0, {3: dict(kind=P.D_WALK, p=P.NONE, n_adj=0, hops=[]), 2: dict(kind=P.D_WALK)}, max_walk=8)
    # (k) a chain: nothing behind the link is reachable after the failure
    g = M.csr(3, M.both([(0, 1, 1), (1, 2, 1)]))
    C["k_unreachable"] = Case(g, 0, {1: dict(kind=P.D_NONE, p=P.NONE, metric=0), 2: dict(kind=P.D_NONE)})
    # (l) S = 0, E = 1; 4 is reached at 6 through 2 (two parallel links 2 -> 4 at 4) and through 3: parent(4) = (2, first of the two)
    g = M.csr(5, M.both([(0, 1, 1), (1, 4, 1), (0, 2, 2), (0, 3, 2), (3, 4, 4), (2, 4, 4), (2, 4, 4)]))
    C["l_tie_break"] = Case(g, 0, {4: dict(kind=R, p=2, q=4, n_adj=1, hops=[(pos(g, 2, 4, 0), 4)], metric=6, flags=F[0] | F[2])})
    # (n) the same with 2 overloaded: it is no parent (and no via); 3 is.  With the overload ignored by both runs it is (l) again
    g = M.csr(5, M.both([(0, 1, 1), (1, 4, 1), (0, 2, 2), (0, 3, 2), (3, 4, 4), (2, 4, 4), (2, 4, 4)]), no_transit=[2])
    C["n_overloaded_parent"] = Case(g, 0, {4: dict(kind=R, p=3, q=4, n_adj=1, hops=[(pos(g, 3, 4), 4)], metric=6, flags=F[0] | F[2])})
    C["n_overload_ignored"] = Case(g, 0, {4: dict(kind=R, p=2, q=4, n_adj=1, hops=[(pos(g, 2, 4, 0), 4)], metric=6, flags=F[0] | F[2])},
                                   run_flags=IGN_RUN, lfa_flags=IGN_LFA)
    # (m) two links 0 -> 1, at 1 (protected) and at 3: E = 1 is released through the other link's slot, p == q == E (and 2 likewise: p == q == 2) ...
    g = M.csr(3, M.both([(0, 1, 1), (0, 1, 3), (1, 2, 1)]))
    C["m_parallel"] = Case(g, 0, {1: dict(kind=R, p=1, via=1, q=1, n_adj=0, hops=[], metric=3, flags=F[0] | F[2]),
                                  2: dict(kind=R, p=2, via=1, q=2, n_adj=0, metric=4, flags=F[0] | F[2])})
    #     ... and with E overloaded (not eligible) the walk reaches S over the parallel link, position 1 of S's row; 2 is then in no SPT of S
    g = M.csr(3, M.both([(0, 1, 1), (0, 1, 3), (1, 2, 1)]), no_transit=[1])
    C["m_parallel_walked"] = Case(g, 0, {1: dict(kind=R, p=0, via=P.NONE, q=1, n_adj=1, hops=[(1, 1)], metric=3, flags=F[0] | F[1] | F[2]),
                                         2: dict(kind=0)})
    # a candidate slot without a row: its destinations are _D_NONE
    g = M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]))
    C["no_row"] = Case(g, 2, {3: dict(kind=P.D_NONE), 4: dict(kind=P.D_NONE), 1: dict(kind=R)}, drop=(1,))
    return C


CASES = _cases()


def check_expect(tp, expect, tag=""):
    """The hand-written expectations against a result (model, host twin or device): tp has the FIELDS of the model, one root."""
    for D, want in expect.items():
        for k, v in want.items():
            if k == "hops":
                got = [(int(tp.tp_hop_pos[D, h]), int(tp.tp_hop_head[D, h])) for h in range(int(tp.tp_n_adj[D]))]
                assert got == v, (tag, D, "hops", got, v)
                assert (tp.tp_hop_pos[D, len(v):] == P.NONE).all() and (tp.tp_hop_head[D, len(v):] == P.NONE).all(), (tag, D)
            else:
                got = int(getattr(tp, "tp_" + k)[D])
                assert got == v, (tag, D, k, got, v)


# ---- the sweep graphs of the host and GPU tests ------------------------------------------------------------------------------------

def ring_chords(n, seed, lo=1, hi=20, chords=None, asym=False, zero_share=0.0):
    """A ring of n routers plus about n / 8 chords; one seeded cost per link, or one per direction (`asym`).  (The generator of
    tests/test_gpu_rlfa.py, restated so that the CPU tests import no GPU test module; same seeds, same graphs.)"""
    r = np.random.default_rng(seed)
    und = {(v, (v + 1) % n) for v in range(n)}
    while len(und) < n + (n // 8 if chords is None else chords):
        a, b = (int(x) for x in r.integers(0, n, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        c1 = int(r.integers(lo, hi + 1))
        c2 = int(r.integers(lo, hi + 1)) if asym else c1
        if zero_share and r.random() < zero_share:
            c1 = c2 = 0
        links += [(a, b, c1), (b, a, c2)]
    return M.csr(n, links)


def sweep_graph(seed):
    """30 to 60 routers on a ring with chords and a cost per direction; every fourth seed with zero-cost links, every fourth with
    an overloaded router."""
    n = 30 + (seed * 7) % 31
    g = ring_chords(n, 100 + seed, 1, 9, chords=n // 6, asym=True, zero_share=0.08 if seed % 4 == 3 else 0.0)
    if seed % 4 == 2:
        g[3][(seed * 5) % n] |= M.VF_NO_TRANSIT
    return g


# ---- case files of tests/cpp/tilfa_pc_driver.cpp, and its host-twin leg --------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "tilfa_pc_driver")
LINE = re.compile(r"(\d+) cases, (\d+) destinations compared, (\d+) differ, (\d+) answered not supported")


def build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    from oracle import graph_oracle as go
    go.build()
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("tilfa_pc_driver")


def write_case_file(path, w: P.Want, lfa_flags=0, with_lfa=False, max_walk=256):
    """The model's side of one protected root (tests/_tilfa_pc_model.py: Want) in the driver's format."""
    rp, col, met, vf = w.graph
    n, S = len(vf), 64 * w.W
    slots = sorted(w.pc)
    pc_row = np.full(S, P.NONE, np.uint32)
    pc_row[slots] = np.arange(len(slots))
    pcd = np.stack([w.pc[e] for e in slots]).ravel() if slots else []
    tp = w.tp
    parts = [[n, len(col), w.maxp, w.root, w.run_flags, lfa_flags, max_walk], rp, col, met, vf, [len(w.cand.nbr)], w.cand.nbr, w.cand.cost, w.cand.root_link,
             w.cand.cflags, [len(w.roots)], w.roots, w.nbr_row, [w.W], w.fwd.dist.ravel(), w.fwd.flags.ravel(), w.fwd.mask.ravel(), [int(with_lfa)],
             w.lfa.alt_flags, w.rl.space_flags.ravel(), w.rl.space_via.ravel(), [len(slots)], pc_row, pcd, tp.tp_kind, tp.tp_p, tp.tp_via, tp.tp_q, tp.tp_n_adj,
             tp.tp_hop_pos.ravel(), tp.tp_hop_head.ravel(), tp.tp_metric, tp.tp_flags, tp.tp_coverage]
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")


def run_driver(engine, files, out_dir=None):
    cmd = [DRIVER, "--engine", engine]
    if engine == "oracle":
        cmd += ["--oracle-so", os.path.join(ROOT, "oracle", "liboracle_spf.so")]
    if out_dir is not None:
        cmd += ["--out-dir", str(out_dir)]
    r = subprocess.run(cmd + [str(f) for f in files], capture_output=True, text=True, timeout=300)
    m = LINE.search(r.stdout)
    assert r.returncode == 0 and m, r.stdout[-4000:] + r.stderr[-4000:]
    return [int(x) for x in m.groups()]


def twin(tmp_path, wants, tag="case"):
    """The host twin (hspf::host::tilfa_pc_sequential through the driver's `host` leg, ONE process) on the model's inputs of every
    entry of wants = [(Want, lfa_flags, with_lfa, max_walk)]: the driver compares every array with the model's; what the twin
    returned comes back as a TilfaPc per entry."""
    build_driver()
    files = []
    for i, (w, lfa_flags, with_lfa, max_walk) in enumerate(wants):
        files.append(tmp_path / f"{tag}_{i}.txt")
        write_case_file(files[-1], w, lfa_flags, with_lfa, max_walk)
    cases, compared, bad, _ = run_driver("host", files, tmp_path)
    assert cases == len(wants) and bad == 0 and compared == sum(len(w.graph[3]) for w, *_ in wants)
    outs = []
    for f, (w, *_) in zip(files, wants):
        n = len(w.graph[3])
        rows = [np.array(line.split(), np.uint64) for line in open(str(f) + ".out")]
        dts = (np.uint8, np.uint32, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint8, np.uint32)
        arrs = [r.astype(dt) for r, dt in zip(rows, dts)]
        arrs[5], arrs[6] = arrs[5].reshape(n, P.MAX_ADJ), arrs[6].reshape(n, P.MAX_ADJ)
        outs.append(P.TilfaPc(*arrs))
    return outs


def same(got: P.TilfaPc, want: P.TilfaPc, tag=""):
    for name in P.FIELDS:
        g, x = getattr(got, name), getattr(want, name)
        assert g.shape == x.shape and g.dtype == x.dtype and np.array_equal(g, x), (tag, name, np.argwhere(g != x)[:8].tolist())
