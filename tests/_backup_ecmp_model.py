"""Per-primary backups of ECMP prefixes (hspf_routes_backup_ecmp_device) restated in plain Python over SPTs of the CPU oracle: the
expected values of tests/test_host_backup_ecmp.py, tests/test_gpu_backup_ecmp.py and tests/test_cpp_backup_ecmp.py.  Shares no code
with holo_amd/: d_X(p), the routes and the table come from tests/_backup_model.py, the flag values and the order of the choice
(node, primary, sum, slot) from tests/_lfa_ecmp_model.py, the rule itself from include/holo_spf_hip.h ("per-primary backups for
ECMP prefixes"), one prefix, one primary and one candidate at a time with Python integers.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

import _backup_model as B
import _lfa_ecmp_model as EM
import _lfa_model as M

INF, NONE = B.INF, B.NONE
LFA, NODE, PAIR, NOTHING = B.LFA, B.NODE, B.PAIR, B.NOTHING
NODE_PROTECT, DOWNSTREAM, EA_PRIMARY = EM.NODE_PROTECT, EM.DOWNSTREAM, EM.EA_PRIMARY
COVERAGE_WORDS = 8
FIELDS = ("eb_ptr", "eb_primary", "eb_kind", "eb_slot", "eb_metric", "eb_flags", "eb_coverage")
DTYPES = dict(eb_ptr=np.uint32, eb_primary=np.uint32, eb_kind=np.uint8, eb_slot=np.uint32, eb_metric=np.uint32, eb_flags=np.uint8, eb_coverage=np.uint32)


@dataclass
class BackupEcmp:
    eb_ptr: np.ndarray        # [n_prefixes + 1] u32
    eb_primary: np.ndarray    # [T] u32
    eb_kind: np.ndarray       # [T] u8
    eb_slot: np.ndarray       # [T] u32
    eb_metric: np.ndarray     # [T] u32
    eb_flags: np.ndarray      # [T] u8
    eb_coverage: np.ndarray   # [8] u32
    eb_prefix: np.ndarray     # [T] the prefix of every entry (not an output of the call)
    cand: Optional[list] = None     # [T] the set cand(h) of every entry
    node: Optional[list] = None     # [T] the set node(h)

    @property
    def total(self) -> int:
        return len(self.eb_primary)

    def entries(self, p):
        return [(int(self.eb_primary[e]), int(self.eb_kind[e]), int(self.eb_slot[e]), int(self.eb_metric[e]), int(self.eb_flags[e]))
                for e in range(int(self.eb_ptr[p]), int(self.eb_ptr[p + 1]))]


def members_of(dist, flags, cand: M.Cand, nbr_row, t: B.Table, p, P, h, d_sp, lfa_flags=0, memo=None):
    """[(k, in node(h), k in P, cost[k] + d_N(p), downstream)] for the members of cand(h) of prefix p, ascending k.  memo: a dict
    that keeps, between the primaries of this prefix, what does not depend on h: d_N(p) of every slot, and the slots that pass the
    loop-free inequality and the overload rule."""
    S, K = cand.root, len(cand.nbr)
    E = int(cand.nbr[h])
    memo = {} if memo is None else memo
    if "base" not in memo:
        base, in_p = [], set(P)
        for k in range(K):
            N = int(cand.nbr[k])
            if N == NONE:
                continue
            d_np, mine = memo[k] = B.dist_to_prefix(dist, flags, nbr_row[k], t, p, own=N)
            d_ns = int(dist[nbr_row[k], S])
            if d_np is None or d_ns == INF or not d_np < d_ns + d_sp:
                continue
            if (cand.cflags[k] & M.C_NO_TRANSIT) and not (lfa_flags & M.IGNORE_OVERLOAD) and not mine:
                continue
            base.append((k, d_np, k in in_p, int(cand.cost[k]) + d_np, d_np < d_sp, int(cand.root_link[k])))
        memo["base"] = base
    d_ep = memo[h][0] if E != NONE else None
    d_e = dist[:, E] if E != NONE and d_ep is not None else None            # d(., E) of every row
    rlh = int(cand.root_link[h])
    out = []
    for k, d_np, prim, total, down, rl in memo["base"]:
        if k == h or rl == rlh:
            continue
        node = False
        if d_e is not None:
            d_ne = int(d_e[nbr_row[k]])
            node = d_ne != INF and d_np < d_ne + d_ep
        out.append((k, node, prim, total, down))
    return out


def backup_ecmp(dist, flags, mask, cand: M.Cand, root_row, nbr_row, t: B.Table, r: B.Routes, lfa_flags=0, tilfa=None, *, min_primaries=2,
                sets=False) -> BackupEcmp:
    """The stream of ONE protected root.  r: the routes of the root's row; tilfa: the TI-LFA model of the root (ti_kind, ti_via,
    ti_metric are read) or None.  min_primaries = 1 applies the same per-primary rule to one-primary prefixes as well (the
    cross-check against _backup_model.backup); the call itself is min_primaries = 2."""
    K = len(cand.nbr)
    assert not (t.flags & B.PFX_ORDERED) and K <= 64 * mask.shape[2]
    ptr = [0]
    ent, pfx, s_cand, s_node = [], [], [], []
    cov = [0] * COVERAGE_WORDS
    for p in range(t.n):
        P = []
        if int(r.best_entry[p]) != INF:
            P = [k for k in range(K) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
        if len(P) < min_primaries:
            ptr.append(ptr[-1])
            continue
        cov[0] += 1
        backed, memo = True, {}
        for h in P:
            mem = members_of(dist, flags, cand, nbr_row, t, p, P, h, int(r.best_metric[p]), lfa_flags, memo)
            kind, slot, metric, fl = NOTHING, NONE, 0, 0
            if mem:
                k, node, prim, total, down = min(mem, key=lambda m: (not m[1], not m[2], m[3], m[0]))
                kind, slot, metric = LFA, k, min(total, 0xFFFFFFFE)
                fl = (NODE_PROTECT if node else 0) | (DOWNSTREAM if down else 0) | (EA_PRIMARY if prim else 0)
            elif tilfa is not None and int(tilfa.ti_kind[h]) != 0:
                kind = NODE if int(tilfa.ti_kind[h]) == 1 else PAIR
                slot, metric = int(tilfa.ti_via[h]), int(tilfa.ti_metric[h])
            ent.append((h, kind, slot, metric, fl))
            pfx.append(p)
            if sets:
                s_cand.append({m[0] for m in mem})
                s_node.append({m[0] for m in mem if m[1]})
            cov[1] += 1
            cov[2] += kind == LFA
            cov[3] += bool(fl & NODE_PROTECT)
            cov[4] += bool(fl & DOWNSTREAM)
            cov[5] += bool(fl & EA_PRIMARY)
            cov[6] += kind in (NODE, PAIR)
            backed = backed and kind != NOTHING
        cov[7] += backed
        ptr.append(ptr[-1] + len(P))
    col = lambda i, dt: np.array([e[i] for e in ent], dt)      # noqa: E731
    return BackupEcmp(np.array(ptr, np.uint32), col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint8),
                      np.array(cov, np.uint32), np.array(pfx, np.uint32), s_cand if sets else None, s_node if sets else None)


def stack(parts):
    """The stream of several protected roots sharing one table set and table, in the order of the protect list."""
    ptr, off = [np.zeros(1, np.uint32)], 0
    for p in parts:
        ptr.append((p.eb_ptr[1:].astype(np.uint64) + np.uint64(off)).astype(np.uint32))
        off += p.total
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts]).astype(DTYPES.get(f, np.uint32))      # noqa: E731
    return BackupEcmp(np.concatenate(ptr), cat("eb_primary"), cat("eb_kind"), cat("eb_slot"), cat("eb_metric"), cat("eb_flags"),
                      np.stack([p.eb_coverage for p in parts]), cat("eb_prefix"))


def want(model, lfa_flags=0, remote=True, table=None, **kw):
    """[BackupEcmp] of the protected roots of a tests/_backup_cases.py Model."""
    f, t = model.fwd, table or model.table
    return [backup_ecmp(f.dist, f.flags, f.mask, c, rr, nr, t, model.routes(i, t), lfa_flags, model.frr(lfa_flags)[i][2] if remote else None, **kw)
            for i, (c, rr, nr) in enumerate(zip(model.cands, model.root_row, model.nbr_row))]
