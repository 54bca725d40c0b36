"""TI-LFA repairs along the post-convergence path (hspf_tilfa_pc_device) restated in plain Python over the CPU oracle's tables: the
expected values of tests/test_host_tilfa_pc.py, tests/test_gpu_tilfa_pc.py and tests/test_cpp_tilfa_pc.py.  Shares no code with
holo_amd/: the post-convergence rows come from the unmodified oracle on a CSR whose failed link is retargeted
(tests/_failure_cases.py), the space tables from tests/_rlfa_model.py, the parents and the walk from the rules of
include/holo_spf_hip.h ("repairs along the post-convergence path").  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _failure_cases as F
import _lfa_model as M
import _rlfa_model as R

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
VIA_SELF = 0xFFFFFFFE
SAT = 0xFFFFFFFE
MAX_ADJ = 4
D_LFA, D_REPAIR, D_NONE, D_LONG, D_LAN, D_WALK = 1, 2, 3, 4, 5, 6
ON_PC, P_IS_ROOT, Q_IS_DEST = 1, 2, 4
VF_NETWORK, VF_NO_TRANSIT, VF_NO_EXPAND = 1, 2, 4
RUN_IGNORE_OVERLOAD = 2
FIELDS = ("tp_kind", "tp_p", "tp_via", "tp_q", "tp_n_adj", "tp_hop_pos", "tp_hop_head", "tp_metric", "tp_flags", "tp_coverage")


@dataclass
class TilfaPc:
    tp_kind: np.ndarray       # [n] u8
    tp_p: np.ndarray          # [n] u32
    tp_via: np.ndarray        # [n] u32
    tp_q: np.ndarray          # [n] u32
    tp_n_adj: np.ndarray      # [n] u8
    tp_hop_pos: np.ndarray    # [n, 4] u32
    tp_hop_head: np.ndarray   # [n, 4] u32
    tp_metric: np.ndarray     # [n] u32
    tp_flags: np.ndarray      # [n] u8
    tp_coverage: np.ndarray   # [12] u32


def pc_rows(graph, maxp, cand: M.Cand, run_flags=0):
    """{slot: dist row of the root's SPT with link root_link[slot] failed} for every candidate slot, from the oracle."""
    slots = [int(e) for e in np.flatnonzero(cand.nbr != NONE)]
    if not slots:
        return {}
    ref = F.reference(graph, maxp, [cand.root] * len(slots), [(F.ROOT_LINK, int(cand.root_link[e])) for e in slots], run_flags)
    return {e: ref.dist[i] for i, e in enumerate(slots)}


def in_links(graph):
    """Per vertex v the links (u, j, w) into it that a run uses whatever its root: two-way, u without HSPF_VF_NO_EXPAND."""
    rp, col, met, vf = graph
    n = len(vf)
    rows = [[int(t) for t in col[rp[u]:rp[u + 1]]] for u in range(n)]
    into = [[] for _ in range(n)]
    for u in range(n):
        if vf[u] & VF_NO_EXPAND:
            continue
        for j, v in enumerate(rows[u]):
            if v < n and u in rows[v]:
                into[v].append((u, j, int(met[rp[u] + j])))
    return into


def parent(into, vf, pc, S, fpos, ignore_ovl, v):
    """The smallest (u, j) among the tight usable links into v, or None."""
    best = None
    for u, j, w in into[v]:
        if not ignore_ovl and (vf[u] & VF_NO_TRANSIT) and not (vf[u] & VF_NETWORK) and u != S:
            continue
        if u == S and j == fpos:
            continue
        if pc[u] == INF or int(pc[u]) + w != int(pc[v]):
            continue
        if best is None or (u, j) < best:
            best = (u, j)
    return best


def rel_of(dist, cand, root_row, nbr_row, via, v):
    """The release metric of v from its via (unsaturated), or None."""
    if via == VIA_SELF:
        return int(dist[root_row, v])
    if via >= len(cand.nbr):
        return None
    return int(cand.cost[via]) + int(dist[nbr_row[via], v])


def tilfa_pc(dist, flags, mask, graph, cand: M.Cand, root_row, nbr_row, space_flags, space_via, pc, run_flags=0, max_walk=256, alt_flags_in=None) -> TilfaPc:
    """Every output of ONE protected root.  pc: {slot: post-convergence dist row}; a slot that is missing has no row."""
    vf = np.asarray(graph[3])
    n, S, K = dist.shape[1], cand.root, len(cand.nbr)
    ign = bool(run_flags & RUN_IGNORE_OVERLOAD)
    into = in_links(graph)
    out = TilfaPc(np.zeros(n, np.uint8), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32), np.zeros(n, np.uint8),
                  np.full((n, MAX_ADJ), NONE, np.uint32), np.full((n, MAX_ADJ), NONE, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8),
                  np.zeros(12, np.uint32))
    for D in range(n):
        if D == S or not (flags[root_row, D] & 1) or dist[root_row, D] == INF:
            continue
        prim = [k for k in range(K) if (int(mask[root_row, D, k // 64]) >> (k % 64)) & 1]
        if len(prim) != 1:
            continue
        e = prim[0]
        if alt_flags_in is not None and (alt_flags_in[D] & M.LINK_PROTECT):
            out.tp_kind[D] = D_LFA
            continue
        if cand.nbr[e] == NONE or e not in pc or pc[e][D] == INF:
            out.tp_kind[D] = D_NONE
            continue
        row, sf, sv, fpos = pc[e], space_flags[e], space_via[e], int(cand.root_link[e])
        cur, q, gap, p, via, rel, kind = D, D, [], None, NONE, 0, D_WALK
        for _ in range(max_walk):
            f = int(sf[cur])
            if (f & R.ELIGIBLE) and (f & R.IN_Q):
                q, gap = cur, []
            if (f & R.ELIGIBLE) and (f & (R.IN_P | R.IN_XP)) and sv[cur] != NONE:
                r = rel_of(dist, cand, root_row, nbr_row, int(sv[cur]), cur)
                if r is not None:
                    p, via, rel, kind = cur, int(sv[cur]), r, D_REPAIR
                    break
            if cur == S:
                p, via, rel, kind = S, NONE, 0, D_REPAIR
                break
            par = parent(into, vf, row, S, fpos, ign, cur)
            if par is None:
                kind = D_NONE
                break
            gap.insert(0, (par[1], cur))
            cur = par[0]
        if kind == D_REPAIR:
            if len(gap) > MAX_ADJ:
                kind = D_LONG
            elif any(vf[h] & VF_NETWORK for _, h in gap[:-1]):
                kind = D_LAN
        out.tp_kind[D] = kind
        if kind != D_REPAIR:
            continue
        pcp = 0 if p == S else int(row[p])
        out.tp_p[D], out.tp_via[D], out.tp_q[D], out.tp_n_adj[D] = p, via, q, len(gap)
        for h, (pos, head) in enumerate(gap):
            out.tp_hop_pos[D, h], out.tp_hop_head[D, h] = pos, head
        out.tp_metric[D] = min(rel + int(row[D]) - pcp, SAT)
        out.tp_flags[D] = (ON_PC if rel == pcp else 0) | (P_IS_ROOT if p == S else 0) | (Q_IS_DEST if q == D else 0)
    out.tp_coverage[:] = recount(out.tp_kind, out.tp_n_adj)
    return out


def recount(tp_kind, tp_n_adj):
    """tp_coverage from the per-destination arrays."""
    cov = [int((tp_kind != 0).sum())] + [int((tp_kind == c).sum()) for c in range(1, 7)]
    return cov + [int(((tp_kind == D_REPAIR) & (tp_n_adj == a)).sum()) for a in range(5)]


@dataclass
class Want:
    """The whole model of one protected root with [root] + its neighbour routers as the rows."""
    graph: tuple
    root: int
    maxp: int
    run_flags: int
    cand: M.Cand
    roots: np.ndarray
    nbr_row: np.ndarray
    W: int
    fwd: object
    rdist: np.ndarray
    lfa: M.Lfa
    rl: R.Rlfa
    pc: dict
    tp: TilfaPc


def one_root(graph, root, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=0, w_min=1, with_lfa=True, max_walk=256, drop=()) -> Want:
    """lfa_flags follows run_flags' overload bit unless given.  drop: candidate slots that get no row."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64, w_min)
    fwd, rdist = R.tables(graph, maxp, roots, run_flags, W)
    lfa = M.lfa(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, lfa_flags)
    rl = R.rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, vf, c, 0, nbr_row, lfa_flags, lfa.alt_flags if with_lfa else None)
    pc = {e: r for e, r in pc_rows(graph, maxp, c, run_flags).items() if e not in drop}
    tp = tilfa_pc(fwd.dist, fwd.flags, fwd.mask, graph, c, 0, nbr_row, rl.space_flags, rl.space_via, pc, run_flags, max_walk,
                  lfa.alt_flags if with_lfa else None)
    return Want(graph, root, maxp, run_flags, c, roots, nbr_row, W, fwd, rdist, lfa, rl, pc, tp)
