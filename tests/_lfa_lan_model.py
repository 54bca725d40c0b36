"""Broadcast-link protection (RFC 5286 section 3.3) restated in plain Python ON TOP of tests/_lfa_model.py and
tests/_backup_model.py: the expected values of tests/test_host_lfa_lan.py and tests/test_gpu_lfa_lan.py.
The plain models say which slots are in `cand` / `node`; this file removes the members that fail the LAN inequality of
include/holo_spf_hip.h ("broadcast-link protection") and repeats the choice over what is left.  Shares no code with holo_amd/.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_model as B
import _lfa_model as M

INF = NONE = 0xFFFFFFFF
LAN_PRIMARY, LAN_REFUSED = 0x20, 0x40
BITS = (M.HAS_PRIMARY, M.ECMP, M.LINK_PROTECT, M.NODE_PROTECT, M.DOWNSTREAM, LAN_PRIMARY, LAN_REFUSED)


def lan_candidates(row_ptr, col, metric, vflags, root) -> np.ndarray:
    """lan[k]: the network vertex that link root_link[k] of the root's own row leads to over a two-way link, NONE otherwise."""
    c = M.candidates(row_ptr, col, metric, vflags, root)
    row_ptr = np.asarray(row_ptr, np.int64)
    row = lambda v: [int(x) for x in col[row_ptr[v]:row_ptr[v + 1]]]      # noqa: E731
    of_link = [t if (vflags[t] & M.VF_NETWORK) and root in row(t) else NONE for t in row(root)]
    return np.array([of_link[int(j)] for j in c.root_link], np.uint32)


def protect_one(row_ptr, col, metric, vflags, root):
    """M.protect_one plus the LANs: (candidates, SPF roots = [root] + neighbour routers + distinct LANs, nbr_row, lan, lan_row)."""
    c, roots, nbr_row = M.protect_one(row_ptr, col, metric, vflags, root)
    lan = lan_candidates(row_ptr, col, metric, vflags, root)
    lans = sorted({int(x) for x in lan if x != NONE})
    row_of = {v: len(roots) + i for i, v in enumerate(lans)}
    lan_row = np.array([row_of.get(int(x), 0) for x in lan], np.uint32)
    return c, np.concatenate([roots, np.array(lans, np.uint32)]).astype(np.uint32), nbr_row, lan, lan_row


def _bits(mask_row, K):
    return [k for k in range(K) if (int(mask_row[k // 64]) >> (k % 64)) & 1]


def _lan_ok(d_nd, d_nl, d_ld):
    """d(N, D) < d(N, L) + d(L, D) with Python integers; an INF (or missing) term makes it false."""
    return None not in (d_nd, d_nl, d_ld) and INF not in (d_nd, d_nl, d_ld) and d_nd < d_nl + d_ld


def lfa(dist, flags, mask, cand: M.Cand, root_row, nbr_row, lan, lan_row, lfa_flags=0) -> M.Lfa:
    """hspf_lfa_lan_device for ONE protected root: M.lfa, then per destination the members of cand held against the LANs of the
    primaries, the choice repeated over the survivors.  coverage has seven words.  `refused` (an extra attribute) lists the
    (D, k) pairs that failed only the LAN inequality."""
    plain = M.lfa(dist, flags, mask, cand, root_row, nbr_row, lfa_flags)
    n, W = dist.shape[1], mask.shape[2]
    K = len(cand.nbr)
    out = M.Lfa(np.full(n, NONE, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), plain.cand_mask.copy(), plain.node_mask.copy(),
                np.zeros(7, np.uint32))
    out.refused = []
    for D in range(n):
        fl = int(plain.alt_flags[D]) & (M.HAS_PRIMARY | M.ECMP)
        if fl:
            P = _bits(mask[root_row, D], K)
            lans = [(int(lan[p]), int(lan_row[p])) for p in P if lan[p] != NONE]
            if lans:
                fl |= LAN_PRIMARY
            members = []
            for k in _bits(plain.cand_mask[D], K):
                d_nd = int(dist[nbr_row[k], D])
                if all(_lan_ok(d_nd, int(dist[nbr_row[k], L]), int(dist[r, D])) for L, r in lans):
                    members.append(k)
                else:
                    fl |= LAN_REFUSED
                    out.refused.append((D, k))
                    out.cand_mask[D, k // 64] &= ~np.uint64(1 << (k % 64))
                    out.node_mask[D, k // 64] &= ~np.uint64(1 << (k % 64))
            if not (fl & M.ECMP) and members:
                node = lambda k: bool((int(out.node_mask[D, k // 64]) >> (k % 64)) & 1)      # noqa: E731
                k = min(members, key=lambda k: (not node(k), int(cand.cost[k]) + int(dist[nbr_row[k], D]), k))
                out.alt_slot[D] = k
                out.alt_metric[D] = min(int(cand.cost[k]) + int(dist[nbr_row[k], D]), 0xFFFFFFFE)
                fl |= M.LINK_PROTECT | (M.NODE_PROTECT if node(k) else 0) | (M.DOWNSTREAM if int(dist[nbr_row[k], D]) < int(dist[root_row, D]) else 0)
        out.alt_flags[D] = fl
    out.coverage[:] = [int(((out.alt_flags & b) != 0).sum()) for b in BITS]
    return out


def backup(dist, flags, mask, cand: M.Cand, root_row, nbr_row, lan, lan_row, t: B.Table, r: B.Routes, lfa_flags=0, tilfa=None) -> B.Backup:
    """hspf_routes_backup_lan_device for ONE protected root: the members B.sets_of finds, held against d(N, L) + d_L(p) of the
    primaries' LANs; the per-link repair only for a point-to-point primary.  bk_coverage has nine words."""
    W, K = mask.shape[2], len(cand.nbr)
    out = B.Backup(np.zeros(t.n, np.uint8), np.full(t.n, NONE, np.uint32), np.full(t.n, NONE, np.uint32), np.zeros(t.n, np.uint32),
                   np.zeros(t.n, np.uint8), np.zeros((t.n, W), np.uint64), np.zeros((t.n, W), np.uint64), np.zeros(9, np.uint32))
    out.refused = []
    for p in range(t.n):
        fl = 0
        if int(r.best_entry[p]) == INF:
            kind = B.NO_ROUTE
        else:
            P = _bits(r.nexthop_mask[p], K)
            kind = B.LOCAL if not P else B.ECMP if len(P) >= 2 else B.NOTHING
        if kind >= B.ECMP:
            lans = [(int(lan[e]), B.dist_to_prefix(dist, flags, int(lan_row[e]), t, p)[0]) for e in P if lan[e] != NONE]
            if lans:
                fl |= LAN_PRIMARY
            members = []
            for m in B.sets_of(dist, flags, cand, root_row, nbr_row, t, p, P, int(r.best_metric[p]), lfa_flags):
                k = m[0]
                d_np = m[2] - int(cand.cost[k])
                # (d_N(p) and d_L(p) are numbers even when saturated at 0xFFFFFFFF; only "no advertiser reached" and d(N, L) can be INF)
                if all(d_lp is not None and int(dist[nbr_row[k], L]) != INF and d_np < int(dist[nbr_row[k], L]) + d_lp for L, d_lp in lans):
                    members.append(m)
                    out.bk_cand_mask[p, k // 64] |= np.uint64(1 << (k % 64))
                    if m[1]:
                        out.bk_node_mask[p, k // 64] |= np.uint64(1 << (k % 64))
                else:
                    fl |= LAN_REFUSED
                    out.refused.append((p, k))
            if kind == B.NOTHING:
                e = P[0]
                out.bk_primary[p] = e
                if members:
                    k, node, total, down, _ = min(members, key=lambda m: (not m[1], m[2], m[0]))
                    kind = B.LFA
                    out.bk_slot[p], out.bk_metric[p] = k, min(total, 0xFFFFFFFE)
                    fl |= (B.NODE_PROTECT if node else 0) | (B.DOWNSTREAM if down else 0)
                elif tilfa is not None and int(tilfa.ti_kind[e]) != 0 and lan[e] == NONE:
                    kind = B.NODE if int(tilfa.ti_kind[e]) == 1 else B.PAIR
                    out.bk_slot[p], out.bk_metric[p] = tilfa.ti_via[e], tilfa.ti_metric[e]
        out.bk_kind[p], out.bk_flags[p] = kind, fl
        out.bk_coverage[kind] += 1
        out.bk_coverage[7] += bool(fl & LAN_PRIMARY)
        out.bk_coverage[8] += bool(fl & LAN_REFUSED)
    return out
