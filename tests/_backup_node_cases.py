"""The graphs, prefix tables and model-side plumbing the per-prefix node-protection tests share (tests/test_host_backup_node.py,
tests/test_gpu_backup_node.py, tests/test_gpu_backup_node_random.py): the hand-checked cases and the
two seeded sweeps.  Plain numpy over the CPU oracle, no GPU import.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_cases as C
import _backup_model as B
import _lfa_model as M

# The random tables of the 40 graphs of tests/_frr_chains.py: sweep_graphs.  Seeds 1 .. 4 were tried on the CPU with the model
# (max_pq = max_pairs = 8); all four show every kind 1 .. 5 at least 73 times and at least 188 multi-homed prefixes whose kind differs
# from the per-vertex class of S's attaining advertiser; 1 is the first of them (kinds 1 .. 5: 596, 353, 117, 174, 84; 193 differ).
TABLE_SEED = 1
# The host-only sweep over tests/_backup_cases.py: sweep_case.  Pairs are rare on those sparse meshes: of the 40-seed windows at
# 7000, 7040, 7080, 7120 each has 2 to 14 prefixes of kind 5; the test takes all four (160 graphs, 29 of kind 5).
HOST_SEEDS = range(C.SWEEP_SEED, C.SWEEP_SEED + 160)
SWEEP_MAX = 8                             # max_pq = max_pairs of both sweeps: lists are cut short on the larger graphs


def six_ring():
    """0-1-2-3-4-5-0, every link at 1; S = 0, slot 0 -> router 1, slot 1 -> router 5.  Prefix 0 = {1, 3} (anycast on the neighbour
    and behind it), prefix 1 = {1}, prefix 2 = {2}, prefix 3 = {3 at 0, 5 at 1} (two primaries), all metrics 0 but the last."""
    g = M.csr(6, M.both([(v, (v + 1) % 6, 1) for v in range(6)]))
    return g, 0, B.table([[(1, 0), (3, 0)], [(1, 0)], [(2, 0)], [(3, 0), (5, 2)]])


def five_ring():
    """The five-ring of tests/_backup_cases.py (costs 1, 1, 1, 1 and 4 on 4-0), S = 2: P and Q of either link do not meet."""
    return C.five_ring()


_SWEEP = {}


def sweep_models():
    """[Model] of the 40 graphs of tests/_frr_chains.py with seeded multi-homed tables (test_gpu_backup.random_table's recipe),
    computed once and left unchanged."""
    if "fc" not in _SWEEP:
        import _frr_chains as FC
        r = np.random.default_rng(TABLE_SEED)
        _SWEEP["fc"] = [C.Model(g, [root], random_table(r, len(g[3]), int(r.integers(20, 60)))) for g, root, _ in FC.sweep_graphs()]
    return _SWEEP["fc"]


def random_table(r, nr, n_pfx, lo=1, hi=16):
    """The recipe of tests/test_gpu_backup.py: random_table (restated: that module imports the GPU helpers)."""
    return B.table([[(int(v), int(r.integers(lo, hi))) for v in r.choice(nr, size=int(r.choice([1, 2, 2, 3])), replace=False)] for _ in range(n_pfx)])


def host_models():
    if "host" not in _SWEEP:
        _SWEEP["host"] = [C.Model(*(lambda g, S, t: (g, [S], t))(*C.sweep_case(s))) for s in HOST_SEEDS]
    return _SWEEP["host"]


def without_node(graph, E):
    """The graph with every link of E, in both directions, removed."""
    rp, col, met, vf = graph
    links = [(u, int(col[k]), int(met[k])) for u in range(len(vf)) for k in range(int(rp[u]), int(rp[u + 1])) if u != E and int(col[k]) != E]
    g = M.csr(len(vf), links)
    g[3][:] = vf
    return g
