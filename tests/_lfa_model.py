"""Loop-free alternates (RFC 5286) restated in numpy over SPTs of the CPU oracle: the expected values of tests/test_host_lfa.py,
tests/test_gpu_lfa.py and tests/test_cpp_lfa.py.  Shares no code with holo_amd/: the candidate table is derived from the CSR
here, the sets and the selection from the rules of include/holo_spf_hip.h ("loop-free alternates on device").
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
VF_NETWORK, VF_NO_TRANSIT = 0x01, 0x02
C_NO_TRANSIT = 0x01
IGNORE_OVERLOAD = 0x01
HAS_PRIMARY, ECMP, LINK_PROTECT, NODE_PROTECT, DOWNSTREAM = 0x01, 0x02, 0x04, 0x08, 0x10


@dataclass
class Cand:
    root: int
    nbr: np.ndarray
    cost: np.ndarray
    root_link: np.ndarray
    cflags: np.ndarray


def candidates(row_ptr, col, metric, vflags, root) -> Cand:
    """One entry per first-hop slot of `root`: H = [root] ++ networks reached through networks only (breadth-first, links in
    row order, two-way links only, each vertex once); slot(p, j) = sum of the row lengths of H before p, plus j."""
    row_ptr = np.asarray(row_ptr, np.int64)
    rows = [list(map(int, col[row_ptr[v]:row_ptr[v + 1]])) for v in range(len(row_ptr) - 1)]
    H = [(int(root), 0, None)]                 # vertex, cost of the path that discovered it, first link of that path
    in_h = {int(root)}
    nbr, cost, rl, cf = [], [], [], []
    qi = 0
    while qi < len(H):
        p, pc, first = H[qi]
        for j, t in enumerate(rows[p]):
            c = min(pc + int(metric[row_ptr[p] + j]), 0xFFFFFFFF)
            f = j if qi == 0 else first
            net = bool(vflags[t] & VF_NETWORK)
            two = p in rows[t]
            is_c = (not net) and t != root and two
            nbr.append(t if is_c else NONE)
            cost.append(c)
            rl.append(f)
            cf.append(C_NO_TRANSIT if is_c and (vflags[t] & VF_NO_TRANSIT) else 0)
            if net and two and t not in in_h:
                in_h.add(t)
                H.append((t, c, f))
        qi += 1
    return Cand(int(root), np.array(nbr, np.uint32), np.array(cost, np.uint32), np.array(rl, np.uint32), np.array(cf, np.uint8))


@dataclass
class Lfa:
    alt_slot: np.ndarray      # [n] u32
    alt_metric: np.ndarray    # [n] u32
    alt_flags: np.ndarray     # [n] u8
    cand_mask: np.ndarray     # [n, W] u64
    node_mask: np.ndarray     # [n, W] u64
    coverage: np.ndarray      # [5] u32


def _less(a, b, c):
    """a < b + c in 64 bits, false when a term is INF (arrays or scalars of uint32 values)."""
    a64, b64, c64 = (np.asarray(x).astype(np.uint64) for x in (a, b, c))
    return (a64 != INF) & (b64 != INF) & (c64 != INF) & (a64 < b64 + c64)


def lfa(dist, flags, mask, cand: Cand, root_row: int, nbr_row, lfa_flags: int = 0) -> Lfa:
    """The five outputs and the coverage of ONE protected root.  dist / flags / mask: [rows, n] / [rows, n] / [rows, n, W] tables
    (oracle.graph_oracle.run); nbr_row[k]: row of the SPT rooted at cand.nbr[k]."""
    n, W = dist.shape[1], mask.shape[2]
    S, K = cand.root, len(cand.nbr)
    assert K <= 64 * W
    D = np.arange(n)
    dS = dist[root_row]
    live = ((flags[root_row] & 1) != 0) & (D != S) & (dS != INF)
    inP = [live & (((mask[root_row, :, k // 64] >> np.uint64(k % 64)) & np.uint64(1)) != 0) for k in range(K)]
    npri = np.zeros(n, np.int64)
    for k in range(K):
        npri += inP[k]
    prim = [p for p in range(K) if inP[p].any()]
    has_router_primary = np.zeros(n, bool)
    for p in prim:
        if cand.nbr[p] != NONE:
            has_router_primary |= inP[p]
    cand_mask = np.zeros((n, W), np.uint64)
    node_mask = np.zeros((n, W), np.uint64)
    alt_slot = np.full(n, NONE, np.uint32)
    best_sum = np.zeros(n, np.uint64)
    best_node = np.zeros(n, bool)
    best_down = np.zeros(n, bool)
    have = np.zeros(n, bool)
    for k in range(K):
        N = int(cand.nbr[k])
        if N == NONE:
            continue
        dN = dist[nbr_row[k]]
        c = live & _less(dN, np.full(n, dN[S], np.uint32), dS)
        if (cand.cflags[k] & C_NO_TRANSIT) and not (lfa_flags & IGNORE_OVERLOAD):
            c &= D == N
        nd = c & has_router_primary
        for p in prim:
            if cand.root_link[p] == cand.root_link[k] or p == k:
                c &= ~inP[p]
            E = int(cand.nbr[p])
            if E != NONE:
                nd &= ~inP[p] | _less(dN, np.full(n, dN[E], np.uint32), dist[nbr_row[p]])
        nd &= c
        bit = np.uint64(1) << np.uint64(k % 64)
        cand_mask[c, k // 64] |= bit
        node_mask[nd, k // 64] |= bit
        s = dN.astype(np.uint64) + np.uint64(int(cand.cost[k]))
        better = c & (npri == 1) & (~have | (nd & ~best_node) | ((nd == best_node) & (s < best_sum)))      # ascending k: ties keep the smaller slot
        alt_slot[better] = k
        best_sum[better] = s[better]
        best_node[better] = nd[better]
        best_down[better] = (dN.astype(np.uint64) < dS.astype(np.uint64))[better]
        have |= better
    fl = np.zeros(n, np.uint8)
    fl[npri >= 1] |= HAS_PRIMARY
    fl[npri >= 2] |= ECMP
    fl[have] |= LINK_PROTECT
    fl[have & best_node] |= NODE_PROTECT
    fl[have & best_down] |= DOWNSTREAM
    alt_metric = np.where(have, np.minimum(best_sum, np.uint64(0xFFFFFFFE)), np.uint64(0)).astype(np.uint32)
    cov = np.array([int(((fl & b) != 0).sum()) for b in (HAS_PRIMARY, ECMP, LINK_PROTECT, NODE_PROTECT, DOWNSTREAM)], np.uint32)
    return Lfa(alt_slot, alt_metric, fl, cand_mask, node_mask, cov)


def protect_one(row_ptr, col, metric, vflags, root):
    """What a caller prepares for one root: (candidates, SPF roots = [root] + its distinct neighbour routers, nbr_row)."""
    c = candidates(row_ptr, col, metric, vflags, root)
    nbrs = sorted({int(x) for x in c.nbr if x != NONE})
    roots = np.array([root] + nbrs, np.uint32)
    row_of = {v: i + 1 for i, v in enumerate(nbrs)}
    nbr_row = np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32)
    return c, roots, nbr_row


def csr(n, links, net=(), no_transit=()):
    """CSR from directed (u, v, cost) links in the given order (rows keep the order in which a vertex's links appear)."""
    rows = [[] for _ in range(n)]
    for u, v, c in links:
        rows[u].append((v, c))
    row_ptr = np.zeros(n + 1, np.uint32)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([v for r in rows for v, _ in r], np.uint32)
    met = np.array([c for r in rows for _, c in r], np.uint32)
    vf = np.zeros(n, np.uint8)
    vf[list(net)] |= VF_NETWORK
    vf[list(no_transit)] |= VF_NO_TRANSIT
    return row_ptr, col, met, vf


def both(links):
    return [x for u, v, c in links for x in ((u, v, c), (v, u, c))]
