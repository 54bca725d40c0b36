"""Remote loop-free alternates (RFC 7490) restated in numpy over SPTs of the CPU oracle: the expected values of
tests/test_host_rlfa.py, tests/test_gpu_rlfa.py and tests/test_cpp_rlfa.py.  Shares no code with holo_amd/: the transpose is
written here, the candidate table comes from tests/_lfa_model.py, the sets and the selection from the rules of
include/holo_spf_hip.h ("remote loop-free alternates on device").  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _lfa_model as M

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
VIA_SELF = 0xFFFFFFFE
VF_NETWORK, VF_NO_TRANSIT, VF_NO_EXPAND = 0x01, 0x02, 0x04
IN_P, IN_XP, IN_Q, ELIGIBLE = 0x01, 0x02, 0x04, 0x08
SAT = 0xFFFFFFFE


def transpose(row_ptr, col, metric):
    """(row_ptr, col, metric) of the reversed graph: row t lists (u, cost) of every link u -> t by ascending u, then by position
    in u's row.  Written with a sort of explicit (target, source, position) triples — not the product's counting sort."""
    n = len(row_ptr) - 1
    trip = sorted((int(col[k]), u, k - int(row_ptr[u]), int(metric[k])) for u in range(n) for k in range(int(row_ptr[u]), int(row_ptr[u + 1])))
    trp = np.zeros(n + 1, np.uint32)
    for t, _, _, _ in trip:
        trp[t + 1] += 1
    trp = np.cumsum(trp).astype(np.uint32)
    return trp, np.array([u for _, u, _, _ in trip], np.uint32), np.array([c for _, _, _, c in trip], np.uint32)


@dataclass
class Rlfa:
    pq_node: np.ndarray       # [S] u32            (S = 64 * W)
    pq_via: np.ndarray        # [S] u32
    pq_metric: np.ndarray     # [S] u32
    pq_counts: np.ndarray     # [S, 4] u32
    space_flags: np.ndarray   # [S, n] u8
    space_via: np.ndarray     # [S, n] u32
    rl_node: np.ndarray       # [n] u32
    rl_via: np.ndarray        # [n] u32
    rl_coverage: np.ndarray   # [4] u32


def _lt(a, b):
    """a < b where a holds uint32 values with INF = not reached and b is a uint64 sum, or None where a term of it was INF."""
    return (a != INF) & b[1] & (a.astype(np.uint64) < b[0])


def _sum(*terms):
    """(64-bit sum, all terms finite) of uint32 arrays / scalars."""
    tot, ok = np.uint64(0), True
    for t in terms:
        t = np.asarray(t)
        ok = ok & (t != INF)
        tot = tot + t.astype(np.uint64)
    return tot, ok


def rlfa(dist, flags, mask, rdist, vflags, cand: M.Cand, root_row: int, nbr_row, lfa_flags: int = 0, alt_flags_in=None) -> Rlfa:
    """Every output of ONE protected root.  dist / flags / mask: the forward oracle tables; rdist: [rows, n] dist of the same roots
    on the transposed graph; vflags: the graph's; alt_flags_in: [n] alt_flags of the LFA model, or None."""
    n, W = dist.shape[1], mask.shape[2]
    S, K, stride = cand.root, len(cand.nbr), 64 * mask.shape[2]
    assert K <= stride
    ign = bool(lfa_flags & M.IGNORE_OVERLOAD)
    V = np.arange(n)
    dS, rS = dist[root_row], rdist[root_row]
    vflags = np.asarray(vflags)
    elig = ((flags[root_row] & 1) != 0) & (dS != INF) & (V != S) & ((vflags & (VF_NETWORK | VF_NO_EXPAND)) == 0)
    if not ign:
        elig &= (vflags & VF_NO_TRANSIT) == 0
    out = Rlfa(np.full(stride, NONE, np.uint32), np.full(stride, NONE, np.uint32), np.zeros(stride, np.uint32), np.zeros((stride, 4), np.uint32),
               np.zeros((stride, n), np.uint8), np.full((stride, n), NONE, np.uint32), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32),
               np.zeros(4, np.uint32))
    for e in range(K):
        if cand.nbr[e] == NONE:
            continue
        c = np.uint32(cand.cost[e])
        dE, rE = dist[nbr_row[e]], rdist[nbr_row[e]]
        P = elig & _lt(dS, _sum(c, dE))
        Q = elig & _lt(rE, _sum(rS, c))
        best = np.where(P, dS.astype(np.uint64), np.uint64(0xFFFFFFFFFFFFFFFF))
        via = np.where(P, np.uint32(VIA_SELF), np.uint32(NONE))
        XP = np.zeros(n, bool)
        for k in range(K):
            if cand.nbr[k] == NONE or cand.root_link[k] == cand.root_link[e]:
                continue
            if (cand.cflags[k] & M.C_NO_TRANSIT) and not ign:
                continue
            dN = dist[nbr_row[k]]
            x = elig & _lt(dN, _sum(np.uint32(dN[S]), c, dE))
            XP |= x
            rel = dN.astype(np.uint64) + np.uint64(int(cand.cost[k]))
            better = x & (rel < best)                                  # ascending k after S: a tie keeps the earlier one
            best[better] = rel[better]
            via[better] = k
        ext = P | XP
        pq = ext & Q
        out.space_flags[e] = P * IN_P + XP * IN_XP + Q * IN_Q + elig * ELIGIBLE
        out.space_via[e] = via
        out.pq_counts[e] = [P.sum(), ext.sum(), Q.sum(), pq.sum()]
        if pq.any():
            met = np.minimum(best, np.uint64(SAT))
            key = np.where(pq, (met << np.uint64(32)) | V.astype(np.uint64), np.uint64(0xFFFFFFFFFFFFFFFF))
            v = int(np.argmin(key))
            out.pq_node[e], out.pq_via[e], out.pq_metric[e] = v, via[v], met[v]
    # per destination: the PQ node of its one primary slot
    live = ((flags[root_row] & 1) != 0) & (V != S) & (dS != INF)
    inP = np.zeros((K, n), bool)
    for k in range(K):
        inP[k] = live & (((mask[root_row, :, k // 64] >> np.uint64(k % 64)) & np.uint64(1)) != 0)
    one = inP.sum(axis=0) == 1
    cov = [int(one.sum()), 0, 0, 0]
    for D in np.flatnonzero(one):
        e = int(np.flatnonzero(inP[:, D])[0])
        if alt_flags_in is not None and (alt_flags_in[D] & M.LINK_PROTECT):
            cov[1] += 1
        elif cand.nbr[e] != NONE and out.pq_node[e] != NONE:
            out.rl_node[D], out.rl_via[D] = out.pq_node[e], out.pq_via[e]
            cov[2] += 1
        else:
            cov[3] += 1
    out.rl_coverage[:] = cov
    return out


FIELDS = ("pq_node", "pq_via", "pq_metric", "pq_counts", "space_flags", "space_via", "rl_node", "rl_via", "rl_coverage")


def tables(graph, maxp, roots, run_flags, W):
    """Forward oracle tables of `roots` and the dist of the same roots on the transposed graph."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    fwd = go.run(rp, col, met, vf, maxp, roots, run_flags, go.MAP, mask_words_=W)
    trp, tcol, tmet = transpose(rp, col, met)
    rev = go.run(trp, tcol, tmet, vf, maxp, roots, run_flags, go.MAP, mask_words_=max(W, go.mask_words(trp, tcol, tmet, vf, roots)))
    return fwd, rev.dist


def one_root(graph, root, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=0, w_min=1, with_lfa=True, rdist_is_forward=False):
    """The whole model for one protected root with [root] + its neighbour routers as the rows: (cand, roots, nbr_row, W, lfa, rlfa)."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64, w_min)
    fwd, rdist = tables(graph, maxp, roots, run_flags, W)
    lfa = M.lfa(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, lfa_flags)
    r = rlfa(fwd.dist, fwd.flags, fwd.mask, fwd.dist if rdist_is_forward else rdist, vf, c, 0, nbr_row, lfa_flags,
             lfa.alt_flags if with_lfa else None)
    return c, roots, nbr_row, W, lfa, r
