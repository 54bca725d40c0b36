"""Per-prefix backup routes restated in plain Python over SPTs of the CPU oracle: the expected values of tests/test_host_backup.py,
tests/test_gpu_backup.py and tests/test_cpp_backup.py.  Shares no code with holo_amd/: the route reduction of hspf_routes_device
is restated here (`routes`: holo_amd/routes.py has no host-side reduction of its own to borrow), the candidate table comes from
tests/_lfa_model.py, the per-slot repairs from tests/_rlfa_model.py and tests/_tilfa_model.py, the sets and the selection from
the rules of include/holo_spf_hip.h ("per-prefix backup routes on device"), one prefix and one candidate at a time with Python
integers.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _lfa_model as M

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
PFX_SATURATING, PFX_LAST_MIN, PFX_ORDERED, PFX_RESIDENT = 1, 2, 4, 8
NO_ROUTE, LOCAL, ECMP, LFA, NODE, PAIR, NOTHING = 0, 1, 2, 3, 4, 5, 6
NODE_PROTECT, DOWNSTREAM = 0x08, 0x10
FIELDS = ("bk_kind", "bk_primary", "bk_slot", "bk_metric", "bk_flags", "bk_cand_mask", "bk_node_mask", "bk_coverage")


@dataclass
class Table:
    ptr: np.ndarray
    vertex: np.ndarray
    metric: np.ndarray
    flags: int = 0

    @property
    def n(self):
        return len(self.ptr) - 1

    def entries(self, p):
        return [(int(self.vertex[e]), int(self.metric[e]), e) for e in range(int(self.ptr[p]), int(self.ptr[p + 1]))]


def table(lists, flags=0) -> Table:
    """Table from [[(vertex, metric), ...] per prefix]; the entries of a prefix are sorted by vertex (stable)."""
    lists = [sorted(x, key=lambda t: t[0]) for x in lists]
    ptr = np.zeros(len(lists) + 1, np.uint32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return Table(ptr, np.array([v for x in lists for v, _ in x], np.uint32), np.array([m for x in lists for _, m in x], np.uint32), flags)


@dataclass
class Routes:
    best_metric: np.ndarray   # [P] u32
    best_entry: np.ndarray    # [P] u32
    nexthop_mask: np.ndarray  # [P, W] u64


def routes(dist, flags, mask, row, t: Table) -> Routes:
    """What hspf_routes_device leaves for the row (include/holo_spf_hip.h "route derivation on device"): a plain u32 add,
    saturating with PFX_SATURATING; the first smallest entry, with PFX_LAST_MIN the last; the masks of the attaining entries."""
    W = mask.shape[2]
    sat, last = bool(t.flags & PFX_SATURATING), bool(t.flags & PFX_LAST_MIN)
    out = Routes(np.full(t.n, INF, np.uint32), np.full(t.n, INF, np.uint32), np.zeros((t.n, W), np.uint64))
    for p in range(t.n):
        bm, be, vals = INF, INF, []
        for v, m, e in t.entries(p):
            if not (int(flags[row, v]) & 1):
                continue
            s = int(dist[row, v]) + m
            s = min(s, INF) if sat else s & 0xFFFFFFFF
            vals.append((s, v, e))
            if be == INF or s < bm or (last and s == bm):
                bm, be = s, e
        out.best_metric[p], out.best_entry[p] = bm, be
        if be != INF:
            for s, v, e in vals:
                if (e == be) if last else (s == bm):
                    out.nexthop_mask[p] |= mask[row, v]
    return out


def dist_to_prefix(dist, flags, row, t: Table, p, own=None):
    """(d_X(p), X's own entry attains it) for the row of X = `own`'s row; d_X(p) is None when no advertiser is reached."""
    best, mine = None, False
    for v, m, _ in t.entries(p):
        if not (int(flags[row, v]) & 1) or int(dist[row, v]) == INF:
            continue
        s = int(dist[row, v]) + m
        if t.flags & PFX_SATURATING:
            s = min(s, 0xFFFFFFFF)
        if best is None or s < best:
            best, mine = s, v == own
        elif s == best and v == own:
            mine = True
    return best, mine


@dataclass
class Backup:
    bk_kind: np.ndarray        # [P] u8
    bk_primary: np.ndarray     # [P] u32
    bk_slot: np.ndarray        # [P] u32
    bk_metric: np.ndarray      # [P] u32
    bk_flags: np.ndarray       # [P] u8
    bk_cand_mask: np.ndarray   # [P, W] u64
    bk_node_mask: np.ndarray   # [P, W] u64
    bk_coverage: np.ndarray    # [7] u32
    own_exception: int = 0     # prefixes with a NO_TRANSIT candidate admitted through its own entry (the model's book-keeping)


def sets_of(dist, flags, cand: M.Cand, root_row, nbr_row, t: Table, p, P, d_sp, lfa_flags=0):
    """[(k, in node, cost[k] + d_N(p), downstream, admitted through the own-entry exception)] for the members of cand(p)."""
    S = cand.root
    routers = [e for e in P if cand.nbr[e] != NONE]
    d_ep = {e: dist_to_prefix(dist, flags, nbr_row[e], t, p)[0] for e in routers}
    out = []
    for k in range(len(cand.nbr)):
        N = int(cand.nbr[k])
        if N == NONE or k in P or any(cand.root_link[k] == cand.root_link[e] for e in P):
            continue
        d_np, mine = dist_to_prefix(dist, flags, nbr_row[k], t, p, own=N)
        d_ns = int(dist[nbr_row[k], S])
        if d_np is None or d_ns == INF or not d_np < d_ns + d_sp:
            continue
        exception = False
        if (cand.cflags[k] & M.C_NO_TRANSIT) and not (lfa_flags & M.IGNORE_OVERLOAD):
            if not mine:
                continue
            exception = True
        node = bool(routers)
        for e in routers:
            d_ne = int(dist[nbr_row[k], int(cand.nbr[e])])
            node = node and d_ep[e] is not None and d_ne != INF and d_np < d_ne + d_ep[e]
        out.append((k, node, int(cand.cost[k]) + d_np, d_np < d_sp, exception))
    return out


def backup(dist, flags, mask, cand: M.Cand, root_row, nbr_row, t: Table, r: Routes, lfa_flags=0, tilfa=None) -> Backup:
    """Every output of ONE protected root.  r: the routes of the root's row; tilfa: the TI-LFA model of the root (ti_kind, ti_via,
    ti_metric are read) or None."""
    W, K = mask.shape[2], len(cand.nbr)
    assert not (t.flags & PFX_ORDERED) and K <= 64 * W
    out = Backup(np.zeros(t.n, np.uint8), np.full(t.n, NONE, np.uint32), np.full(t.n, NONE, np.uint32), np.zeros(t.n, np.uint32),
                 np.zeros(t.n, np.uint8), np.zeros((t.n, W), np.uint64), np.zeros((t.n, W), np.uint64), np.zeros(7, np.uint32))
    for p in range(t.n):
        if int(r.best_entry[p]) == INF:
            kind = NO_ROUTE
        else:
            P = [k for k in range(K) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
            kind = LOCAL if not P else ECMP if len(P) >= 2 else NOTHING
        if kind >= ECMP:
            members = sets_of(dist, flags, cand, root_row, nbr_row, t, p, P, int(r.best_metric[p]), lfa_flags)
            out.own_exception += any(m[4] for m in members)
            for k, node, _, _, _ in members:
                out.bk_cand_mask[p, k // 64] |= np.uint64(1 << (k % 64))
                if node:
                    out.bk_node_mask[p, k // 64] |= np.uint64(1 << (k % 64))
        if kind == NOTHING:
            e = P[0]
            out.bk_primary[p] = e
            if members:
                k, node, total, down, _ = min(members, key=lambda m: (not m[1], m[2], m[0]))
                kind = LFA
                out.bk_slot[p], out.bk_metric[p] = k, min(total, 0xFFFFFFFE)
                out.bk_flags[p] = (NODE_PROTECT if node else 0) | (DOWNSTREAM if down else 0)
            elif tilfa is not None and int(tilfa.ti_kind[e]) != 0:
                kind = NODE if int(tilfa.ti_kind[e]) == 1 else PAIR
                out.bk_slot[p], out.bk_metric[p] = tilfa.ti_via[e], tilfa.ti_metric[e]
        out.bk_kind[p] = kind
        out.bk_coverage[kind] += 1
    return out
