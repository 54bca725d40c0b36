"""Per-prefix node-protecting backups restated in plain Python over SPTs of the CPU oracle: the expected values of
tests/test_host_backup_node.py, tests/test_gpu_backup_node.py and tests/test_gpu_backup_node_random.py.  Shares no code with
holo_amd/: one prefix and one list entry at a time with Python integers after the rules of include/holo_spf_hip.h ("per-prefix node-protecting backups on device").  The route reduction, the table and d_E(p)
are the backup model's (tests/_backup_model.py), the lists are the RLFA-node and TI-LFA-node models' (tests/_rlfa_node_model.py,
tests/_tilfa_node_model.py).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _backup_model as B
import _lfa_model as M
import _rlfa_node_model as N
import _tilfa_node_model as TN

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
SAT = 0xFFFFFFFE
BN_LFA, BN_PQ, BN_LAST_HOP, BN_NONE, BN_PAIR = 1, 2, 3, 4, 5
FIELDS = ("bn_kind", "bn_primary", "bn_p", "bn_q", "bn_link", "bn_via", "bn_metric", "bn_set_pq", "bn_set_pair", "bn_coverage")


@dataclass
class BackupNode:
    bn_kind: np.ndarray        # [P] u8
    bn_primary: np.ndarray     # [P] u32
    bn_p: np.ndarray           # [P] u32
    bn_q: np.ndarray           # [P] u32
    bn_link: np.ndarray        # [P] u32
    bn_via: np.ndarray         # [P] u32
    bn_metric: np.ndarray      # [P] u32
    bn_set_pq: np.ndarray      # [P] u32
    bn_set_pair: np.ndarray    # [P] u32
    bn_coverage: np.ndarray    # [6] u32


def node_dist_to_prefix(yrow, t: B.Table, p):
    """d_Y(p) from Y's forward dist row, or None: an INF entry contributes nothing, no flags are read."""
    best = None
    for v, m, _ in t.entries(p):
        if int(yrow[v]) == INF:
            continue
        s = int(yrow[v]) + m
        if t.flags & B.PFX_SATURATING:
            s = min(s, 0xFFFFFFFF)
        best = s if best is None or s < best else best
    return best


def protecting(t: B.Table, p, nodes, metrics, count, yrows, E, d_ep):
    """[(metric[j] + d_Y(p), j)] of the list entries j < count that protect p."""
    out = []
    if d_ep is None:
        return out
    for j in range(count):
        Y = int(nodes[j])
        if Y not in yrows:
            continue
        d_yp = node_dist_to_prefix(yrows[Y], t, p)
        d_ye = int(yrows[Y][E])
        if d_yp is None or d_ye == INF or not d_yp < d_ye + d_ep:
            continue
        out.append((int(metrics[j]) + d_yp, j))
    return out


def backup_node(dist, flags, mask, cand: M.Cand, root_row, nbr_row, t: B.Table, r: B.Routes, yrows: dict, rn_sel=None, tn_sel=None,
                bk: B.Backup = None) -> BackupNode:
    """Every output of hspf_routes_backup_node_device for ONE protected root.  r: the routes of the root's row; yrows: {vertex:
    its forward dist row [n]} — a listed node that is no key has no row and is skipped; rn_sel / tn_sel: the Sel of the RLFA-node /
    TI-LFA-node model or None (at least one); bk: the Backup model of the root or None."""
    assert rn_sel is not None or tn_sel is not None
    K = len(cand.nbr)
    pad = lambda v: np.full(t.n, v, np.uint32)      # noqa: E731
    out = BackupNode(np.zeros(t.n, np.uint8), pad(NONE), pad(NONE), pad(NONE), pad(NONE), pad(NONE), pad(0), pad(0), pad(0), np.zeros(6, np.uint32))
    for p in range(t.n):
        if int(r.best_entry[p]) == INF:
            continue
        P = [k for k in range(K) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
        if len(P) != 1:
            continue
        e = P[0]
        E = int(cand.nbr[e])
        out.bn_primary[p] = e
        if bk is not None and int(bk.bk_kind[p]) == B.LFA and int(bk.bk_flags[p]) & B.NODE_PROTECT:
            kind = BN_LFA
        elif E == NONE:
            kind = BN_NONE
        else:
            d_ep, own = B.dist_to_prefix(dist, flags, nbr_row[e], t, p, own=E)
            pq, pair = [], []
            if rn_sel is not None:
                M_ = rn_sel.nq_node.shape[1]
                pq = protecting(t, p, rn_sel.nq_node[e], rn_sel.nq_metric[e], min(int(rn_sel.nq_count[e]), M_), yrows, E, d_ep)
            if tn_sel is not None:
                M_ = tn_sel.tq_q.shape[1]
                pair = protecting(t, p, tn_sel.tq_q[e], tn_sel.tq_metric[e], min(int(tn_sel.tq_count[e]), M_), yrows, E, d_ep)
            for _, j in pq:
                out.bn_set_pq[p] |= np.uint32(1 << j)
            for _, j in pair:
                out.bn_set_pair[p] |= np.uint32(1 << j)
            if pq:
                tot, j = min(pq)
                kind = BN_PQ
                out.bn_p[p] = out.bn_q[p] = rn_sel.nq_node[e, j]
                out.bn_via[p], out.bn_metric[p] = rn_sel.nq_via[e, j], min(tot, SAT)
            elif pair:
                tot, j = min(pair)
                kind = BN_PAIR
                out.bn_p[p], out.bn_q[p], out.bn_link[p], out.bn_via[p] = tn_sel.tq_p[e, j], tn_sel.tq_q[e, j], tn_sel.tq_link[e, j], tn_sel.tq_via[e, j]
                out.bn_metric[p] = min(tot, SAT)
            else:
                kind = BN_LAST_HOP if d_ep is not None and own else BN_NONE
        out.bn_kind[p] = kind
        out.bn_coverage[0] += 1
        out.bn_coverage[kind] += 1
    return out


class Want:
    """The model's side of protected root i of a tests/_backup_cases.py Model: the two lists, the union of the listed nodes with
    their rows, the per-vertex results nd_* / tn_* and the per-prefix result."""

    def __init__(self, model, i=0, lfa_flags=0, max_pq=16, max_pairs=16, with_rn=True, with_tn=True, with_bk=True, remote=True, table=None,
                 y_pick=None):
        f, c, rr, nr = model.fwd, model.cands[i], model.root_row[i], model.nbr_row[i]
        self.table = t = table or model.table
        lf, rl, _ = model.frr(lfa_flags)[i]
        self.alt = lf.alt_flags
        self.rn = N.select(f.dist, c, rr, nr, rl.space_flags, lfa_flags, max_pq)
        self.tn = TN.select(f.dist, model.graph, c, rr, nr, rl.space_flags, lfa_flags, max_pairs)
        listed = sorted(set((N.union(self.rn) if with_rn else []) + (TN.union(self.tn) if with_tn else [])))
        self.y_roots = np.array((y_pick(listed) if y_pick else listed) or [NONE], np.uint32)
        self.yrows = N.y_rows(model.graph, model.maxp, [v for v in self.y_roots if v != NONE], model.run_flags)
        self.routes = model.routes(i, t)
        self.bk = model.want(lfa_flags, remote, table)[i] if with_bk else None
        self.bn = backup_node(f.dist, f.flags, f.mask, c, rr, nr, t, self.routes, self.yrows, self.rn if with_rn else None,
                              self.tn if with_tn else None, self.bk)
        self._model, self._i = model, i

    def per_vertex(self):
        """(nd, tn) of the per-vertex models on the same lists and rows, with the alt_flags of the LFA model."""
        m, i = self._model, self._i
        f, c, rr, nr = m.fwd, m.cands[i], m.root_row[i], m.nbr_row[i]
        nd = N.dest(f.dist, f.flags, f.mask, c, rr, nr, self.rn, self.yrows, self.alt)
        tn = TN.dest(f.dist, f.flags, f.mask, c, rr, nr, self.tn, self.yrows, self.alt, nd.nd_kind)
        return nd, tn
