"""Remote LFA with LAN-safe spaces restated in numpy ON TOP of tests/_rlfa_model.py and tests/_lfa_lan_model.py: the expected
values of tests/test_host_rlfa_lan.py, tests/test_gpu_rlfa_lan.py and tests/test_cpp_rlfa_lan.py.  The plain model says what
P, XP and Q are; this file adds the three LAN inequalities of include/holo_spf_hip.h ("remote loop-free alternates with LAN-safe
spaces") as literal conjunctions, repeats the release point and the choice over what is left, and counts the two new words
against the plain model's answer.  TI-LFA on the LAN tables is tests/_tilfa_model.py fed with them; the per-prefix backups are
_lfa_lan_model.backup plus the HSPF_LFA_LAN_SAFE_REPAIRS bit.  Shares no code with holo_amd/.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_model as B
import _lfa_lan_model as LM
import _lfa_model as M
import _rlfa_model as R
import _tilfa_model as T

INF = NONE = 0xFFFFFFFF
LAN_SAFE_REPAIRS = 0x02
COUNT_WORDS, COVERAGE_WORDS = 5, 6
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def rlfa(dist, flags, mask, rdist, vflags, cand: M.Cand, root_row, nbr_row, lan, lan_row, lfa_flags=0, alt_flags_in=None) -> R.Rlfa:
    """hspf_rlfa_lan_device for ONE protected root.  pq_counts has five words per slot, rl_coverage six.  `plain` (an extra
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
        if cand.nbr[e] == NONE or lan[e] == NONE:
            continue                                                   # a point-to-point slot: the plain answer
        E, lr, c = int(cand.nbr[e]), int(lan_row[e]), np.uint32(cand.cost[e])
        Lv = int(lan[e])
        dE, rE, dL, rL = dist[nbr_row[e]], rdist[nbr_row[e]], dist[lr], rdist[lr]
        pf = plain.space_flags[e]
        elig = (pf & R.ELIGIBLE) != 0
        P = ((pf & R.IN_P) != 0) & R._lt(dS, R._sum(np.uint32(dS[Lv]), dL))
        Q = ((pf & R.IN_Q) != 0) & R._lt(rE, R._sum(rL, np.uint32(dL[E])))
        best = np.where(P, dS.astype(np.uint64), U64_MAX)
        via = np.where(P, np.uint32(R.VIA_SELF), np.uint32(NONE))
        XP = np.zeros(n, bool)
        for k in range(K):
            if cand.nbr[k] == NONE or cand.root_link[k] == cand.root_link[e]:
                continue
            if (cand.cflags[k] & M.C_NO_TRANSIT) and not ign:
                continue
            dN = dist[nbr_row[k]]
            x = elig & R._lt(dN, R._sum(np.uint32(dN[S]), c, dE)) & R._lt(dN, R._sum(np.uint32(dN[Lv]), dL))
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
    # per destination: the PQ node of its one primary slot; the LAN words against the plain model's PQ node
    cov = [0] * COVERAGE_WORDS
    for D in range(n):
        if D == S or not (int(flags[root_row, D]) & 1) or dS[D] == INF:
            continue
        prim = [k for k in range(K) if (int(mask[root_row, D, k // 64]) >> (k % 64)) & 1]
        if len(prim) != 1:
            continue
        e = prim[0]
        cov[0] += 1
        cov[4] += bool(lan[e] != NONE)
        if alt_flags_in is not None and (int(alt_flags_in[D]) & M.LINK_PROTECT):
            cov[1] += 1
        elif cand.nbr[e] != NONE and out.pq_node[e] != NONE:
            out.rl_node[D], out.rl_via[D] = out.pq_node[e], out.pq_via[e]
            cov[2] += 1
        else:
            cov[3] += 1
            cov[5] += bool(lan[e] != NONE and cand.nbr[e] != NONE and plain.pq_node[e] != NONE)
    out.rl_coverage[:] = cov
    return out


def tilfa(dist, flags, mask, rdist, graph, cand, root_row, nbr_row, rl: R.Rlfa, alt_flags_in=None) -> T.Tilfa:
    """hspf_tilfa_device fed with the tables of `rl`."""
    return T.tilfa(dist, flags, mask, rdist, graph, cand, root_row, nbr_row, rl.space_flags, rl.space_via, alt_flags_in)


def backup(dist, flags, mask, cand, root_row, nbr_row, lan, lan_row, t: B.Table, r: B.Routes, lfa_flags=0, tilfa=None) -> B.Backup:
    """hspf_routes_backup_lan_device with HSPF_LFA_LAN_SAFE_REPAIRS honoured: without the bit _lfa_lan_model.backup as it is; with
    it a LAN primary that was left with nothing takes the per-link repair on offer."""
    out = LM.backup(dist, flags, mask, cand, root_row, nbr_row, lan, lan_row, t, r, lfa_flags & ~LAN_SAFE_REPAIRS, tilfa)
    if not (lfa_flags & LAN_SAFE_REPAIRS) or tilfa is None:
        return out
    for p in range(t.n):
        if out.bk_kind[p] != B.NOTHING:
            continue
        e = int(out.bk_primary[p])
        if lan[e] != NONE and int(tilfa.ti_kind[e]) != 0:
            kind = B.NODE if int(tilfa.ti_kind[e]) == 1 else B.PAIR
            out.bk_coverage[B.NOTHING] -= 1
            out.bk_coverage[kind] += 1
            out.bk_kind[p], out.bk_slot[p], out.bk_metric[p] = kind, tilfa.ti_via[e], tilfa.ti_metric[e]
    return out


FIELDS = R.FIELDS


def one_root(graph, root, maxp=0xFFFFFFFF, run_flags=0, lfa_flags=0, w_min=1, with_lfa=True, no_lans=False):
    """The whole model for one protected root with [root] + neighbour routers + LANs as the rows of BOTH table sets:
    dict(cand, roots, nbr_row, lan, lan_row, W, fwd, rdist, lfa, rl)."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row, lan, lan_row = LM.protect_one(rp, col, met, vf, root)
    if no_lans:
        lan = np.full(len(lan), NONE, np.uint32)
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64, w_min)
    fwd, rdist = R.tables(graph, maxp, roots, run_flags, W)
    lfa = LM.lfa(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, lan, lan_row, lfa_flags)
    rl = rlfa(fwd.dist, fwd.flags, fwd.mask, rdist, vf, c, 0, nbr_row, lan, lan_row, lfa_flags, lfa.alt_flags if with_lfa else None)
    return dict(cand=c, roots=roots, nbr_row=nbr_row, lan=lan, lan_row=lan_row, W=W, fwd=fwd, rdist=rdist, lfa=lfa, rl=rl)
