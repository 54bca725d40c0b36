"""SRLG-safe loop-free alternates and remote-LFA spaces restated in numpy ON TOP of tests/_lfa_model.py and tests/_rlfa_model.py: the
expected values of tests/test_host_srlg.py, tests/test_gpu_srlg.py and tests/test_cpp_srlg.py.  The plain models say what cand, P,
XP and Q are; this file adds the member conditions of include/holo_spf_hip.h ("SRLG-safe alternates and remote-LFA spaces") as
literal conjunctions, repeats the selection over what is left and counts the new words against the plain answer.  members() is a
plain-Python restatement of hspf_srlg_members.  TI-LFA on the safe tables is tests/_tilfa_model.py fed with them.  Shares no code
with holo_amd/.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _lfa_model as M
import _rlfa_model as R

INF = NONE = 0xFFFFFFFF
MAX_MEMBERS = 16
SRLG_REFUSED = 0x80
LFA_COVERAGE_WORDS, COUNT_WORDS, COVERAGE_WORDS = 7, 5, 6
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


@dataclass
class Members:
    mem_ptr: np.ndarray       # [K + 1]
    tail: np.ndarray
    pos: np.ndarray
    head: np.ndarray
    cost: np.ndarray
    tail_row: np.ndarray = None
    head_row: np.ndarray = None

    def of(self, k):
        return range(int(self.mem_ptr[k]), int(self.mem_ptr[k + 1]))


def empty_members(K):
    z = np.zeros(0, np.uint32)
    return Members(np.zeros(K + 1, np.uint32), z, z, z, z, z, z)


def members(row_ptr, col, metric, vflags, root, grp_ptr, grp) -> Members:
    """Per first-hop slot of `root` (the numbering of _lfa_model.candidates): every OTHER directed link — by ascending position
    in `col`, which is ascending (tail, pos) — that shares a group id with the link at root_link[k] of the root's own row."""
    c = M.candidates(row_ptr, col, metric, vflags, root)
    E = len(col)
    groups = [set(int(x) for x in grp[int(grp_ptr[l]):int(grp_ptr[l + 1])]) for l in range(E)]
    tail_of = [u for u in range(len(row_ptr) - 1) for _ in range(int(row_ptr[u]), int(row_ptr[u + 1]))]
    ptr, cols = [0], [[], [], [], []]
    for k in range(len(c.nbr)):
        prot = int(row_ptr[root]) + int(c.root_link[k])
        for l in range(E):
            if l != prot and groups[l] & groups[prot]:
                a = tail_of[l]
                for lst, x in zip(cols, (a, l - int(row_ptr[a]), int(col[l]), int(metric[l]))):
                    lst.append(x)
        ptr.append(len(cols[0]))
    return Members(np.array(ptr, np.uint32), *(np.array(x, np.uint32) for x in cols))


def protect_one(row_ptr, col, metric, vflags, root, grp_ptr, grp):
    """What a caller prepares for one root: (candidates, SPF roots = [root] + neighbour routers + the members' endpoints that are
    not yet in the list, nbr_row, members with their rows filled)."""
    c, roots, nbr_row = M.protect_one(row_ptr, col, metric, vflags, root)
    mem = members(row_ptr, col, metric, vflags, root, grp_ptr, grp)
    have = [int(x) for x in roots]
    more = sorted({int(x) for x in list(mem.tail) + list(mem.head)} - set(have))
    roots = np.array(have + more, np.uint32)
    row_of = {v: i for i, v in enumerate(roots.tolist())}
    mem.tail_row = np.array([row_of[int(x)] for x in mem.tail], np.uint32)
    mem.head_row = np.array([row_of[int(x)] for x in mem.head], np.uint32)
    return c, roots, nbr_row, mem


def _cross(dxv, dxa, w, dbv):
    """crosses: d(X, a) and d(b, v) both finite and d(X, v) >= d(X, a) + w + d(b, v) in 64 bits."""
    dxv, dxa, dbv = (np.asarray(x).astype(np.uint64) for x in (dxv, dxa, dbv))
    return (dxa != INF) & (dbv != INF) & (dxv >= dxa + np.uint64(int(w)) + dbv)


def _local(cand, mem, i, k):
    return int(mem.tail[i]) == cand.root and int(mem.pos[i]) == int(cand.root_link[k])


def lfa(dist, flags, mask, cand: M.Cand, root_row, nbr_row, mem: Members, lfa_flags=0) -> M.Lfa:
    """hspf_lfa_srlg_device for ONE protected root; coverage has seven words.  `plain` (an extra attribute) is the plain model."""
    plain = M.lfa(dist, flags, mask, cand, root_row, nbr_row, lfa_flags)
    n, W = dist.shape[1], mask.shape[2]
    S, K = cand.root, len(cand.nbr)
    D = np.arange(n)
    dS = dist[root_row]
    live = ((flags[root_row] & 1) != 0) & (D != S) & (dS != INF)
    inP = [live & (((mask[root_row, :, k // 64] >> np.uint64(k % 64)) & np.uint64(1)) != 0) for k in range(K)]
    npri = sum(x.astype(np.int64) for x in inP) if K else np.zeros(n, np.int64)
    prim = [p for p in range(K) if inP[p].any()]
    hasm = np.zeros(n, bool)
    for p in prim:
        if len(mem.of(p)):
            hasm |= inP[p]
    has_router_primary = np.zeros(n, bool)
    for p in prim:
        if cand.nbr[p] != NONE:
            has_router_primary |= inP[p]
    cand_mask = np.zeros((n, W), np.uint64)
    node_mask = np.zeros((n, W), np.uint64)
    alt_slot = np.full(n, NONE, np.uint32)
    best_sum = np.zeros(n, np.uint64)
    best_node, best_down, have, refused = (np.zeros(n, bool) for _ in range(4))
    for k in range(K):
        if cand.nbr[k] == NONE:
            continue
        dN = dist[nbr_row[k]]
        bit = np.uint64(1) << np.uint64(k % 64)
        c = (plain.cand_mask[:, k // 64] & bit) != 0                  # every condition of the plain cand
        safe = c.copy()
        for p in prim:
            for i in mem.of(p):
                ok_i = np.full(n, not _local(cand, mem, i, k)) & ~_cross(dN, dN[int(mem.tail[i])], mem.cost[i], dist[int(mem.head_row[i])])
                safe &= ~inP[p] | ok_i
        refused |= c & ~safe
        nd = safe & has_router_primary
        for p in prim:
            E = int(cand.nbr[p])
            if E != NONE:
                nd &= ~inP[p] | M._less(dN, np.full(n, dN[E], np.uint32), dist[nbr_row[p]])
        cand_mask[safe, k // 64] |= bit
        node_mask[nd, k // 64] |= bit
        s = dN.astype(np.uint64) + np.uint64(int(cand.cost[k]))
        better = safe & (npri == 1) & (~have | (nd & ~best_node) | ((nd == best_node) & (s < best_sum)))
        alt_slot[better] = k
        best_sum[better] = s[better]
        best_node[better] = nd[better]
        best_down[better] = (dN.astype(np.uint64) < dS.astype(np.uint64))[better]
        have |= better
    fl = np.zeros(n, np.uint8)
    fl[npri >= 1] |= M.HAS_PRIMARY
    fl[npri >= 2] |= M.ECMP
    fl[have] |= M.LINK_PROTECT
    fl[have & best_node] |= M.NODE_PROTECT
    fl[have & best_down] |= M.DOWNSTREAM
    fl[refused] |= SRLG_REFUSED
    alt_metric = np.where(have, np.minimum(best_sum, np.uint64(0xFFFFFFFE)), np.uint64(0)).astype(np.uint32)
    cov = [int(((fl & b) != 0).sum()) for b in (M.HAS_PRIMARY, M.ECMP, M.LINK_PROTECT, M.NODE_PROTECT, M.DOWNSTREAM)]
    cov += [int(hasm.sum()), int(refused.sum())]
    out = M.Lfa(alt_slot, alt_metric, fl, cand_mask, node_mask, np.array(cov, np.uint32))
    out.plain = plain
    return out


def rlfa(dist, flags, mask, rdist, vflags, cand: M.Cand, root_row, nbr_row, mem: Members, lfa_flags=0, alt_flags_in=None) -> R.Rlfa:
    """hspf_rlfa_srlg_device for ONE protected root.  pq_counts has five words per slot, rl_coverage six.  `plain` (an extra
    attribute) is the plain model's answer on the same tables."""
    plain = R.rlfa(dist, flags, mask, rdist, vflags, cand, root_row, nbr_row, lfa_flags, alt_flags_in)
    n, K, stride = dist.shape[1], len(cand.nbr), 64 * mask.shape[2]
    S = cand.root
    ign = bool(lfa_flags & M.IGNORE_OVERLOAD)
    V = np.arange(n)
    dS = dist[root_row]
    out = R.Rlfa(plain.pq_node.copy(), plain.pq_via.copy(), plain.pq_metric.copy(), np.zeros((stride, COUNT_WORDS), np.uint32),
                 plain.space_flags.copy(), plain.space_via.copy(), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32),
                 np.zeros(COVERAGE_WORDS, np.uint32))
    out.pq_counts[:, :4] = plain.pq_counts
    out.plain = plain
    for e in range(K):
        if cand.nbr[e] == NONE or not len(mem.of(e)):
            continue                                                   # no members: the plain answer
        E, c = int(cand.nbr[e]), np.uint32(cand.cost[e])
        dE, rE = dist[nbr_row[e]], rdist[nbr_row[e]]
        pf = plain.space_flags[e]
        elig = (pf & R.ELIGIBLE) != 0
        P = (pf & R.IN_P) != 0
        Q = (pf & R.IN_Q) != 0
        for i in mem.of(e):
            a, w, hr, tr = int(mem.tail[i]), mem.cost[i], int(mem.head_row[i]), int(mem.tail_row[i])
            P = P & ~_cross(dS, dS[a], w, dist[hr])
            Q = Q & ~_cross(rE, rdist[tr], w, dist[hr][E])
        best = np.where(P, dS.astype(np.uint64), U64_MAX)
        via = np.where(P, np.uint32(R.VIA_SELF), np.uint32(NONE))
        XP = np.zeros(n, bool)
        for k in range(K):
            if cand.nbr[k] == NONE or cand.root_link[k] == cand.root_link[e]:
                continue
            if (cand.cflags[k] & M.C_NO_TRANSIT) and not ign:
                continue
            dN = dist[nbr_row[k]]
            x = elig & R._lt(dN, R._sum(np.uint32(dN[S]), c, dE))
            for i in mem.of(e):
                x = x & (not _local(cand, mem, i, k)) & ~_cross(dN, dN[int(mem.tail[i])], mem.cost[i], dist[int(mem.head_row[i])])
            XP |= x
            rel = dN.astype(np.uint64) + np.uint64(int(cand.cost[k]))
            better = x & (rel < best)
            best[better] = rel[better]
            via[better] = k
        ext = P | XP
        pq = ext & Q
        plain_pq = ((pf & (R.IN_P | R.IN_XP)) != 0) & ((pf & R.IN_Q) != 0)
        out.space_flags[e] = P * R.IN_P + XP * R.IN_XP + Q * R.IN_Q + elig * R.ELIGIBLE
        out.space_via[e] = via
        out.pq_counts[e] = [P.sum(), ext.sum(), Q.sum(), pq.sum(), (plain_pq & ~pq).sum()]
        out.pq_node[e], out.pq_via[e], out.pq_metric[e] = NONE, NONE, 0
        if pq.any():
            met = np.minimum(best, np.uint64(R.SAT))
            key = np.where(pq, (met << np.uint64(32)) | V.astype(np.uint64), U64_MAX)
            v = int(np.argmin(key))
            out.pq_node[e], out.pq_via[e], out.pq_metric[e] = v, via[v], met[v]
    cov = [0] * COVERAGE_WORDS
    for D in range(n):
        if D == S or not (int(flags[root_row, D]) & 1) or dS[D] == INF:
            continue
        prim = [k for k in range(K) if (int(mask[root_row, D, k // 64]) >> (k % 64)) & 1]
        if len(prim) != 1:
            continue
        e = prim[0]
        hasm = len(mem.of(e)) > 0
        cov[0] += 1
        cov[4] += hasm
        if alt_flags_in is not None and (int(alt_flags_in[D]) & M.LINK_PROTECT):
            cov[1] += 1
        elif cand.nbr[e] != NONE and out.pq_node[e] != NONE:
            out.rl_node[D], out.rl_via[D] = out.pq_node[e], out.pq_via[e]
            cov[2] += 1
        else:
            cov[3] += 1
            cov[5] += bool(hasm and cand.nbr[e] != NONE and plain.pq_node[e] != NONE)
    out.rl_coverage[:] = cov
    return out


FIELDS = R.FIELDS
LFA_FIELDS = ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask", "coverage")


def one_root(graph, root, grp_ptr, grp, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=0, w_min=1, with_lfa=True, no_members=False):
    """The whole model for one protected root with [root] + neighbour routers + member endpoints as the rows of BOTH table sets:
    dict(cand, roots, nbr_row, mem, W, fwd, rdist, lfa, rl)."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row, mem = protect_one(rp, col, met, vf, root, grp_ptr, grp)
    if no_members:
        mem = empty_members(len(c.nbr))
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64, w_min)
    fwd, rdist = R.tables(graph, maxp, roots, run_flags, W)
    a = lfa(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, mem, lfa_flags)
    rl = rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, vf, c, 0, nbr_row, mem, lfa_flags, a.alt_flags if with_lfa else None)
    return dict(cand=c, roots=roots, nbr_row=nbr_row, mem=mem, W=W, fwd=fwd, rdist=rdist, lfa=a, rl=rl)


def groups_csr(n_links, of_link):
    """(grp_ptr, grp) from {link position: [group ids]}."""
    ptr, g = [0], []
    for l in range(n_links):
        g += list(of_link.get(l, []))
        ptr.append(len(g))
    return np.array(ptr, np.uint32), np.array(g, np.uint32)


def link_pos(graph, u, v, nth=0):
    """Position in `col` of the nth link u -> v."""
    rp, col = graph[0], graph[1]
    hits = [k for k in range(int(rp[u]), int(rp[u + 1])) if int(col[k]) == v]
    return hits[nth]
