"""Node-protecting remote loop-free alternates (RFC 8102) restated in plain Python over SPTs of the CPU oracle: the expected
values of tests/test_host_rlfa_node.py, tests/test_gpu_rlfa_node.py and tests/test_cpp_rlfa_node.py.  Shares no code with
holo_amd/: both steps are loops over vertices and Python integers after the rules of include/holo_spf_hip.h ("node-protecting
remote loop-free alternates on device"); a list is a sorted list of tuples, a choice is `min` of tuples.  The space table the
first step reads is the RLFA model's (tests/_rlfa_model.py).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _lfa_model as M
import _rlfa_model as R

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
VIA_SELF = 0xFFFFFFFE
SAT = 0xFFFFFFFE
D_LFA, D_PQ, D_LAST_HOP, D_NONE = 1, 2, 3, 4
MAX_PQ = 32


def less(a, b, c):
    """a < b + c over Python integers; a term that is INF makes it false."""
    return a != INF and b != INF and c != INF and a < b + c


@dataclass
class Sel:
    nq_node: np.ndarray       # [S, max_pq] u32       (S = 64 * W)
    nq_via: np.ndarray        # [S, max_pq] u32
    nq_metric: np.ndarray     # [S, max_pq] u32
    nq_count: np.ndarray      # [S] u32


SEL_FIELDS = ("nq_node", "nq_via", "nq_metric", "nq_count")


def qualifying(dist, cand: M.Cand, root_row, nbr_row, space_flags, e, lfa_flags=0):
    """The sorted list [(saturated release metric, v, via)] of ALL vertices that qualify under candidate slot e."""
    n = dist.shape[1]
    S, K = cand.root, len(cand.nbr)
    E = int(cand.nbr[e])
    ign = bool(lfa_flags & M.IGNORE_OVERLOAD)
    d = lambda row, v: int(dist[row, v])      # noqa: E731
    out = []
    for v in range(n):
        sf = int(space_flags[e, v])
        if not (sf & R.ELIGIBLE and sf & R.IN_Q and sf & (R.IN_P | R.IN_XP)) or v == E:
            continue
        dEv = d(nbr_row[e], v)
        rel = []                                                   # (release metric, order of preference, via)
        if less(d(root_row, v), d(root_row, E), dEv):
            rel.append((d(root_row, v), -1, VIA_SELF))
        for k in range(K):
            if cand.nbr[k] == NONE or cand.root_link[k] == cand.root_link[e] or int(cand.nbr[k]) == E:
                continue
            if (cand.cflags[k] & M.C_NO_TRANSIT) and not ign:
                continue
            if less(d(nbr_row[k], v), d(nbr_row[k], E), dEv):
                rel.append((int(cand.cost[k]) + d(nbr_row[k], v), k, k))
        if rel:
            m, _, via = min(rel)
            out.append((min(m, SAT), v, via))
    return sorted(out)


def select(dist, cand: M.Cand, root_row, nbr_row, space_flags, lfa_flags=0, max_pq=16) -> Sel:
    """Every output of hspf_rlfa_node_select_device for ONE protected root; space_flags: [S, n] of the RLFA model."""
    stride = space_flags.shape[0]
    out = Sel(np.full((stride, max_pq), NONE, np.uint32), np.full((stride, max_pq), NONE, np.uint32), np.zeros((stride, max_pq), np.uint32),
              np.zeros(stride, np.uint32))
    for e in range(len(cand.nbr)):
        if cand.nbr[e] == NONE:
            continue
        q = qualifying(dist, cand, root_row, nbr_row, space_flags, e, lfa_flags)
        out.nq_count[e] = len(q)
        for j, (m, v, via) in enumerate(q[:max_pq]):
            out.nq_node[e, j], out.nq_via[e, j], out.nq_metric[e, j] = v, via, m
    return out


@dataclass
class Dest:
    nd_kind: np.ndarray       # [n] u8
    nd_node: np.ndarray       # [n] u32
    nd_via: np.ndarray        # [n] u32
    nd_metric: np.ndarray     # [n] u32
    nd_set: np.ndarray        # [n] u32
    nd_coverage: np.ndarray   # [5] u32


DEST_FIELDS = ("nd_kind", "nd_node", "nd_via", "nd_metric", "nd_set", "nd_coverage")


def dest(dist, flags, mask, cand: M.Cand, root_row, nbr_row, sel: Sel, yrows: dict, alt_flags_in=None) -> Dest:
    """Every output of hspf_rlfa_node_device for ONE protected root.  yrows: {vertex Y: its forward dist row [n]} — a listed node
    that is no key has no row and is skipped."""
    n = dist.shape[1]
    S, K = cand.root, len(cand.nbr)
    max_pq = sel.nq_node.shape[1]
    out = Dest(np.zeros(n, np.uint8), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
               np.zeros(5, np.uint32))
    for D in range(n):
        if D == S or not (int(flags[root_row, D]) & 1) or int(dist[root_row, D]) == INF:
            continue
        prim = [k for k in range(K) if (int(mask[root_row, D, k // 64]) >> (k % 64)) & 1]
        if len(prim) != 1:
            continue
        e = prim[0]
        E = int(cand.nbr[e])
        if alt_flags_in is not None and int(alt_flags_in[D]) & M.NODE_PROTECT:
            kind = D_LFA
        elif E == NONE:
            kind = D_NONE
        elif D == E:
            kind = D_LAST_HOP
        else:
            dED = int(dist[nbr_row[e], D])
            ok = []                                                # (total, j)
            for j in range(min(int(sel.nq_count[e]), max_pq)):
                Y = int(sel.nq_node[e, j])
                if Y not in yrows:
                    continue
                dY = yrows[Y]
                if less(int(dY[D]), int(dY[E]), dED):
                    ok.append((int(sel.nq_metric[e, j]) + int(dY[D]), j))
                    out.nd_set[D] |= np.uint32(1 << j)
            if ok:
                tot, j = min(ok)
                kind = D_PQ
                out.nd_node[D], out.nd_via[D], out.nd_metric[D] = sel.nq_node[e, j], sel.nq_via[e, j], min(tot, SAT)
            else:
                kind = D_NONE
        out.nd_kind[D] = kind
        out.nd_coverage[0] += 1
        out.nd_coverage[kind] += 1
    return out


def union(sel: Sel):
    """The ascending union of the listed nodes."""
    return sorted({int(v) for v in sel.nq_node.ravel() if v != NONE})


def y_rows(graph, maxp, verts, run_flags=0):
    """{Y: forward oracle dist row} of the given vertices."""
    from oracle import graph_oracle as go
    verts = sorted({int(v) for v in verts})
    if not verts:
        return {}
    rp, col, met, vf = graph
    roots = np.array(verts, np.uint32)
    res = go.run(rp, col, met, vf, maxp, roots, run_flags, go.MAP, mask_words_=go.mask_words(rp, col, met, vf, roots))
    return {v: res.dist[i] for i, v in enumerate(verts)}
