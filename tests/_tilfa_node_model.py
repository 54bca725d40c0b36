"""Two-segment node-protecting repairs (TI-LFA node protection) restated in plain Python over SPTs of the CPU oracle: the expected
values of tests/test_host_tilfa_node.py, tests/test_gpu_tilfa_node.py and tests/test_cpp_tilfa_node.py.  Shares no code with
holo_amd/: both steps are loops over vertices, links and Python integers after the rules of include/holo_spf_hip.h ("two-segment
node-protecting repairs on device"); a list is a sorted list of tuples, a choice is `min` of tuples.  The space table the first
step reads is the RLFA model's (tests/_rlfa_model.py); the candidate table is the LFA model's (tests/_lfa_model.py); the
inequality and the row helper are the RLFA-node model's (tests/_rlfa_node_model.py).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _lfa_model as M
import _rlfa_model as R
import _rlfa_node_model as N

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
VIA_SELF = 0xFFFFFFFE
SAT = 0xFFFFFFFE
D_LFA, D_PQ, D_LAST_HOP, D_NONE, D_PAIR = 1, 2, 3, 4, 5
MAX_PAIRS = 32
less = N.less
y_rows = N.y_rows


@dataclass
class Sel:
    tq_q: np.ndarray          # [S, max_pairs] u32       (S = 64 * W)
    tq_p: np.ndarray          # [S, max_pairs] u32
    tq_link: np.ndarray       # [S, max_pairs] u32
    tq_via: np.ndarray        # [S, max_pairs] u32
    tq_metric: np.ndarray     # [S, max_pairs] u32
    tq_count: np.ndarray      # [S] u32


SEL_FIELDS = ("tq_q", "tq_p", "tq_link", "tq_via", "tq_metric", "tq_count")


def release(dist, cand: M.Cand, root_row, nbr_row, e, v, lfa_flags=0):
    """(unsaturated release sum, via) of v when the NODE behind slot e is to be avoided, or None."""
    K = len(cand.nbr)
    E = int(cand.nbr[e])
    ign = bool(lfa_flags & M.IGNORE_OVERLOAD)
    d = lambda row, x: int(dist[row, x])      # noqa: E731
    dEv = d(nbr_row[e], v)
    rel = []                                                       # (release sum, order of preference, via)
    if less(d(root_row, v), d(root_row, E), dEv):
        rel.append((d(root_row, v), -1, VIA_SELF))
    for k in range(K):
        if cand.nbr[k] == NONE or cand.root_link[k] == cand.root_link[e] or int(cand.nbr[k]) == E:
            continue
        if (cand.cflags[k] & M.C_NO_TRANSIT) and not ign:
            continue
        if less(d(nbr_row[k], v), d(nbr_row[k], E), dEv):
            rel.append((int(cand.cost[k]) + d(nbr_row[k], v), k, k))
    if not rel:
        return None
    m, _, via = min(rel)
    return m, via


def links(dist, graph, cand: M.Cand, root_row, nbr_row, space_flags, e, lfa_flags=0):
    """Every qualifying link of candidate slot e as (saturated relN(p) + w, p, j, q, via)."""
    rp, col, met, _ = graph
    n = dist.shape[1]
    E = int(cand.nbr[e])
    rows = [[int(t) for t in col[rp[v]:rp[v + 1]]] for v in range(n)]
    sf = space_flags[e]
    out = []
    for p in range(n):
        f = int(sf[p])
        if not (f & R.ELIGIBLE) or not (f & (R.IN_P | R.IN_XP)) or p == E:
            continue
        rel = release(dist, cand, root_row, nbr_row, e, p, lfa_flags)
        if rel is None:
            continue
        for j, q in enumerate(rows[p]):
            fq = int(sf[q])
            if q == p or q == E or not (fq & R.ELIGIBLE) or not (fq & R.IN_Q) or p not in rows[q]:
                continue
            out.append((min(rel[0] + int(met[rp[p] + j]), SAT), p, j, q, rel[1]))
    return out


def entries(dist, graph, cand: M.Cand, root_row, nbr_row, space_flags, e, lfa_flags=0):
    """The sorted list [(saturated entry metric, q, p, j, via)] of ALL q with a qualifying link under candidate slot e."""
    best = {}
    for t in links(dist, graph, cand, root_row, nbr_row, space_flags, e, lfa_flags):
        q = t[3]
        best[q] = min(best.get(q, t), t)                           # (metric, p, j, ...): the smaller p, then the smaller j
    return sorted((m, q, p, j, via) for q, (m, p, j, _, via) in best.items())


def select(dist, graph, cand: M.Cand, root_row, nbr_row, space_flags, lfa_flags=0, max_pairs=16) -> Sel:
    """Every output of hspf_tilfa_node_select_device for ONE protected root; space_flags: [S, n] of the RLFA model."""
    stride = space_flags.shape[0]
    pad = lambda v: np.full((stride, max_pairs), v, np.uint32)      # noqa: E731
    out = Sel(pad(NONE), pad(NONE), pad(NONE), pad(NONE), pad(0), np.zeros(stride, np.uint32))
    for e in range(len(cand.nbr)):
        if cand.nbr[e] == NONE:
            continue
        ent = entries(dist, graph, cand, root_row, nbr_row, space_flags, e, lfa_flags)
        out.tq_count[e] = len(ent)
        for i, (m, q, p, j, via) in enumerate(ent[:max_pairs]):
            out.tq_q[e, i], out.tq_p[e, i], out.tq_link[e, i], out.tq_via[e, i], out.tq_metric[e, i] = q, p, j, via, m
    return out


@dataclass
class Dest:
    tn_kind: np.ndarray       # [n] u8
    tn_p: np.ndarray          # [n] u32
    tn_q: np.ndarray          # [n] u32
    tn_link: np.ndarray       # [n] u32
    tn_via: np.ndarray        # [n] u32
    tn_metric: np.ndarray     # [n] u32
    tn_set: np.ndarray        # [n] u32
    tn_coverage: np.ndarray   # [6] u32


DEST_FIELDS = ("tn_kind", "tn_p", "tn_q", "tn_link", "tn_via", "tn_metric", "tn_set", "tn_coverage")


def dest(dist, flags, mask, cand: M.Cand, root_row, nbr_row, sel: Sel, yrows: dict, alt_flags_in=None, nd_kind_in=None) -> Dest:
    """Every output of hspf_tilfa_node_device for ONE protected root.  yrows: {vertex q: its forward dist row [n]} — a listed q that
    is no key has no row and is skipped."""
    n = dist.shape[1]
    S, K = cand.root, len(cand.nbr)
    max_pairs = sel.tq_q.shape[1]
    pad = lambda v: np.full(n, v, np.uint32)      # noqa: E731
    out = Dest(np.zeros(n, np.uint8), pad(NONE), pad(NONE), pad(NONE), pad(NONE), pad(0), pad(0), np.zeros(6, np.uint32))
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
        elif nd_kind_in is not None and int(nd_kind_in[D]) == N.D_PQ:
            kind = D_PQ
        else:
            dED = int(dist[nbr_row[e], D])
            ok = []                                                # (total, j)
            for j in range(min(int(sel.tq_count[e]), max_pairs)):
                q = int(sel.tq_q[e, j])
                if q not in yrows:
                    continue
                dq = yrows[q]
                if less(int(dq[D]), int(dq[E]), dED):
                    ok.append((int(sel.tq_metric[e, j]) + int(dq[D]), j))
                    out.tn_set[D] |= np.uint32(1 << j)
            if ok:
                tot, j = min(ok)
                kind = D_PAIR
                out.tn_p[D], out.tn_q[D], out.tn_link[D], out.tn_via[D] = sel.tq_p[e, j], sel.tq_q[e, j], sel.tq_link[e, j], sel.tq_via[e, j]
                out.tn_metric[D] = min(tot, SAT)
            else:
                kind = D_NONE
        out.tn_kind[D] = kind
        out.tn_coverage[0] += 1
        out.tn_coverage[kind] += 1
    return out


def union(sel: Sel):
    """The ascending union of the listed q's."""
    return sorted({int(v) for v in sel.tq_q.ravel() if v != NONE})
