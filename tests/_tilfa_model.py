"""Two-segment repair paths (TI-LFA, link protection) restated in plain Python over SPTs of the CPU oracle: the expected values of
tests/test_host_tilfa.py, tests/test_gpu_tilfa.py and tests/test_cpp_tilfa.py.  Shares no code with holo_amd/ and none with the
selection of tests/_rlfa_model.py: the space tables are INPUTS here (what hspf_rlfa_device wrote, or what the RLFA model says it
writes); every repair is enumerated as a tuple (total, kind, p, q, position) and the smallest tuple wins — the order of
include/holo_spf_hip.h ("two-segment repair paths on device") is the order of Python tuples.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NONE = 0xFFFFFFFF
VIA_SELF = 0xFFFFFFFE
SAT = 0xFFFFFFFE
IN_P, IN_XP, IN_Q, ELIGIBLE = 0x01, 0x02, 0x04, 0x08
LINK_PROTECT = 0x04
KIND_NONE, KIND_NODE, KIND_PAIR = 0, 1, 2
D_LFA, D_NODE, D_PAIR, D_NONE = 1, 2, 3, 4


@dataclass
class Tilfa:
    ti_kind: np.ndarray       # [S] u8             (S = 64 * W)
    ti_p: np.ndarray          # [S] u32
    ti_q: np.ndarray          # [S] u32
    ti_via: np.ndarray        # [S] u32
    ti_link: np.ndarray       # [S] u32
    ti_metric: np.ndarray     # [S] u32
    ti_counts: np.ndarray     # [S, 2] u32
    td_kind: np.ndarray       # [n] u8
    td_coverage: np.ndarray   # [5] u32


FIELDS = ("ti_kind", "ti_p", "ti_q", "ti_via", "ti_link", "ti_metric", "ti_counts", "td_kind", "td_coverage")


def repairs(dist, rdist, graph, cand, root_row, nbr_row, e, sflags_e, svia_e):
    """Every repair of slot e as (saturated total, kind, p, q, position); position is 0 for a single node."""
    rp, col, met, _ = graph
    n = dist.shape[1]
    rows = [[int(t) for t in col[rp[v]:rp[v + 1]]] for v in range(n)]
    rdE = rdist[nbr_row[e]]

    def rel(v):
        via = int(svia_e[v])
        if via == VIA_SELF:
            return int(dist[root_row, v])
        return int(cand.cost[via]) + int(dist[nbr_row[via], v])

    out = []
    for p in range(n):
        f = int(sflags_e[p])
        if not (f & ELIGIBLE) or not (f & (IN_P | IN_XP)):
            continue
        r = rel(p)
        if f & IN_Q:
            out.append((min(r + int(rdE[p]), SAT), KIND_NODE, p, p, 0))
        for j, q in enumerate(rows[p]):
            fq = int(sflags_e[q])
            if q == p or not (fq & ELIGIBLE) or not (fq & IN_Q) or p not in rows[q]:
                continue
            out.append((min(r + int(met[rp[p] + j]) + int(rdE[q]), SAT), KIND_PAIR, p, q, j))
    return out


def tilfa(dist, flags, mask, rdist, graph, cand, root_row, nbr_row, space_flags, space_via, alt_flags_in=None) -> Tilfa:
    """Every output of ONE protected root.  dist / flags / mask / rdist: the oracle's tables; graph: the forward CSR
    (row_ptr, col, metric, vflags); space_flags / space_via: [stride, n] of the RLFA step; alt_flags_in: [n] or None."""
    n, W = dist.shape[1], mask.shape[2]
    S, K, stride = cand.root, len(cand.nbr), 64 * W
    out = Tilfa(np.zeros(stride, np.uint8), np.full(stride, NONE, np.uint32), np.full(stride, NONE, np.uint32), np.full(stride, NONE, np.uint32),
                np.full(stride, NONE, np.uint32), np.zeros(stride, np.uint32), np.zeros((stride, 2), np.uint32), np.zeros(n, np.uint8),
                np.zeros(5, np.uint32))
    for e in range(K):
        if cand.nbr[e] == NONE:
            continue
        reps = repairs(dist, rdist, graph, cand, root_row, nbr_row, e, space_flags[e], space_via[e])
        out.ti_counts[e] = [sum(1 for r in reps if r[1] == KIND_NODE), sum(1 for r in reps if r[1] == KIND_PAIR)]
        if reps:
            total, kind, p, q, j = min(reps)
            out.ti_kind[e], out.ti_p[e], out.ti_q[e], out.ti_via[e], out.ti_metric[e] = kind, p, q, space_via[e][p], total
            if kind == KIND_PAIR:
                out.ti_link[e] = j
    dS = dist[root_row]
    for D in range(n):
        if D == S or not (int(flags[root_row, D]) & 1) or dS[D] == NONE:
            continue
        prim = [k for k in range(K) if (int(mask[root_row, D, k // 64]) >> (k % 64)) & 1]
        if len(prim) != 1:
            continue
        if alt_flags_in is not None and (int(alt_flags_in[D]) & LINK_PROTECT):
            cls = D_LFA
        else:
            cls = {KIND_NODE: D_NODE, KIND_PAIR: D_PAIR, KIND_NONE: D_NONE}[int(out.ti_kind[prim[0]])]
        out.td_kind[D] = cls
        out.td_coverage[0] += 1
        out.td_coverage[cls] += 1
    return out
