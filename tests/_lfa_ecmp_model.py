"""Per-primary alternates of ECMP destinations (hspf_lfa_ecmp_device) restated in numpy over SPTs of the CPU oracle: the expected
values of tests/test_host_lfa_ecmp.py, tests/test_gpu_lfa_ecmp.py and tests/test_cpp_lfa_ecmp.py.  Shares no code with holo_amd/:
the candidate table is that of tests/_lfa_model.py, the rule is the one of include/holo_spf_hip.h ("per-primary alternates for
ECMP destinations").
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

import _lfa_model as M

INF, NONE = M.INF, M.NONE
LINK_PROTECT, NODE_PROTECT, DOWNSTREAM, EA_PRIMARY = M.LINK_PROTECT, M.NODE_PROTECT, M.DOWNSTREAM, 0x20
COVERAGE_WORDS = 7
FIELDS = ("ea_ptr", "ea_primary", "ea_slot", "ea_metric", "ea_flags", "ea_coverage")


@dataclass
class Ecmp:
    ea_ptr: np.ndarray        # [n + 1] u32
    ea_primary: np.ndarray    # [T] u32
    ea_slot: np.ndarray       # [T] u32
    ea_metric: np.ndarray     # [T] u32
    ea_flags: np.ndarray      # [T] u8
    ea_coverage: np.ndarray   # [7] u32
    ea_dest: np.ndarray       # [T] the destination of every entry (not an output of the call)
    cand: Optional[np.ndarray] = None     # [T, K] bool: cand(h) of every entry (sets=True)
    node: Optional[np.ndarray] = None     # [T, K] bool: node(h)

    @property
    def total(self) -> int:
        return len(self.ea_primary)


def primaries(dist, flags, mask, cand: M.Cand, root_row: int):
    """(live [n], inP [K, n]): the destinations the call speaks about at all, and bit k of mask_S[D] for the K slots that exist."""
    n, K, S = dist.shape[1], len(cand.nbr), cand.root
    D = np.arange(n)
    live = ((flags[root_row] & 1) != 0) & (D != S) & (dist[root_row] != INF)
    inP = np.zeros((K, n), bool)
    for k in range(K):
        inP[k] = live & (((mask[root_row, :, k // 64] >> np.uint64(k % 64)) & np.uint64(1)) != 0)
    return live, inP


def lfa_ecmp(dist, flags, mask, cand: M.Cand, root_row: int, nbr_row, lfa_flags: int = 0, *, min_primaries: int = 2, sets: bool = False) -> Ecmp:
    """The stream of ONE protected root.  min_primaries = 1 applies the same per-primary rule to single-primary destinations as
    well (the cross-check against _lfa_model.lfa); the call itself is min_primaries = 2."""
    n, K, S = dist.shape[1], len(cand.nbr), cand.root
    assert K <= 64 * mask.shape[2]
    dS = dist[root_row]
    _, inP = primaries(dist, flags, mask, cand, root_row)
    npri = inP.sum(0)
    spoken = npri >= min_primaries
    ptr = np.zeros(n + 1, np.uint64)
    ptr[1:] = np.cumsum(np.where(spoken, npri, 0))
    T = int(ptr[-1])
    e_primary, e_dest = np.zeros(T, np.uint32), np.zeros(T, np.uint32)
    e_slot, e_sum = np.full(T, NONE, np.uint32), np.zeros(T, np.uint64)
    e_have, e_node, e_prim, e_down = (np.zeros(T, bool) for _ in range(4))
    s_cand = np.zeros((T, K), bool) if sets else None
    s_node = np.zeros((T, K), bool) if sets else None
    rank = np.zeros(n, np.uint64)                  # primaries of D below h
    for h in range(K):
        Dh = np.flatnonzero(inP[h] & spoken)
        pos = (ptr[Dh] + rank[Dh]).astype(np.int64)
        rank += inP[h]
        if not len(Dh):
            continue
        e_primary[pos], e_dest[pos] = h, Dh
        E = int(cand.nbr[h])
        dED = dist[nbr_row[h]][Dh] if E != NONE else None
        for k in range(K):                         # ascending k: ties keep the smaller slot
            N = int(cand.nbr[k])
            if k == h or N == NONE or cand.root_link[k] == cand.root_link[h]:
                continue
            dN = dist[nbr_row[k]]
            dND = dN[Dh]
            c = M._less(dND, np.full(len(Dh), dN[S], np.uint32), dS[Dh])
            if (cand.cflags[k] & M.C_NO_TRANSIT) and not (lfa_flags & M.IGNORE_OVERLOAD):
                c &= Dh == N
            nd = c & M._less(dND, np.full(len(Dh), dN[E], np.uint32), dED) if E != NONE else np.zeros(len(Dh), bool)
            pr = inP[k][Dh]
            s = dND.astype(np.uint64) + np.uint64(int(cand.cost[k]))
            if sets:
                s_cand[pos, k], s_node[pos, k] = c, nd
            have, bn, bp, bs = e_have[pos], e_node[pos], e_prim[pos], e_sum[pos]
            better = c & (~have | (nd & ~bn) | ((nd == bn) & ((pr & ~bp) | ((pr == bp) & (s < bs)))))
            w = pos[better]
            e_slot[w], e_sum[w], e_node[w], e_prim[w], e_have[w] = k, s[better], nd[better], pr[better], True
            e_down[w] = (dND.astype(np.uint64) < dS[Dh].astype(np.uint64))[better]
    fl = np.zeros(T, np.uint8)
    fl[e_have] |= LINK_PROTECT
    fl[e_have & e_node] |= NODE_PROTECT
    fl[e_have & e_down] |= DOWNSTREAM
    fl[e_have & e_prim] |= EA_PRIMARY
    metric = np.where(e_have, np.minimum(e_sum, np.uint64(0xFFFFFFFE)), np.uint64(0)).astype(np.uint32)
    missing = np.zeros(n, np.int64)
    np.add.at(missing, e_dest[~e_have], 1)
    cov = np.array([int(spoken.sum()), T, int(e_have.sum()), int((e_have & e_node).sum()), int((e_have & e_down).sum()),
                    int((e_have & e_prim).sum()), int((spoken & (missing == 0)).sum())], np.uint32)
    return Ecmp(ptr.astype(np.uint32), e_primary, e_slot, metric, fl, cov, e_dest, s_cand, s_node)


def stack(parts, n):
    """The stream of several protected roots sharing one table set, in the order of the protect list."""
    ptr, off = [np.zeros(1, np.uint32)], 0
    for p in parts:
        ptr.append((p.ea_ptr[1:].astype(np.uint64) + np.uint64(off)).astype(np.uint32))
        off += p.total
    cat = lambda f, dt: np.concatenate([getattr(p, f) for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    return Ecmp(np.concatenate(ptr), cat("ea_primary", np.uint32), cat("ea_slot", np.uint32), cat("ea_metric", np.uint32), cat("ea_flags", np.uint8),
                np.stack([p.ea_coverage for p in parts]), cat("ea_dest", np.uint32))


def tables(graph, root, run_flags=0, variant=None):
    """(candidates, roots, nbr_row, W, oracle tables) of one protected root on `graph` = (row_ptr, col, metric, vflags).  variant: the
    oracle's (default MAP; HEAP for large unit-cost grids, on which the other two run out of memory)."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    c, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
    W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64)
    return c, roots, nbr_row, W, go.run(rp, col, met, vf, 0xFFFFFFFF, roots, run_flags, go.MAP if variant is None else variant, mask_words_=W)


def model(graph, root, run_flags=0, lfa_flags=0, **kw):
    c, _, nbr_row, _, t = tables(graph, root, run_flags)
    return c, lfa_ecmp(t.dist, t.flags, t.mask, c, 0, nbr_row, lfa_flags, **kw)
