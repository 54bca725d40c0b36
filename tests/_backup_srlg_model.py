"""Per-prefix SRLG-safe backup routes restated in numpy / plain Python ON TOP of tests/_backup_model.py and tests/_srlg_model.py: the
expected values of tests/test_host_backup_srlg.py, tests/test_gpu_backup_srlg.py, tests/test_gpu_backup_srlg_random.py and
tests/test_cpp_backup_srlg.py.  The plain model says what cand(p), node(p) and the choice are; this file adds the member conditions
of include/holo_spf_hip.h ("per-prefix SRLG-safe backups") as literal conjunctions over given SPT rows, repeats the choice over what
is left, and applies the fallback rule.  It never touches the engine.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_model as B
import _lfa_model as M
import _srlg_model as SM

INF = NONE = 0xFFFFFFFF
SAFE_REPAIRS = 0x04
SRLG_PRIMARY, PAIR_REFUSED, SRLG_REFUSED = 0x01, 0x02, 0x80
COVERAGE_WORDS = 10
FIELDS = B.FIELDS


def crosses(dist, flags, t: B.Table, p, d_np, d_na, w, head_row):
    """crosses_p(N, i): d(N, a_i) finite, d_{b_i}(p) exists, d_N(p) >= d(N, a_i) + w_i + d_{b_i}(p) (Python integers)."""
    if d_na == INF:
        return False
    d_bp = B.dist_to_prefix(dist, flags, head_row, t, p)[0]
    return d_bp is not None and d_np >= d_na + int(w) + d_bp


def backup(dist, flags, mask, cand: M.Cand, root_row, nbr_row, mem: SM.Members, t: B.Table, r: B.Routes, lfa_flags=0, tilfa=None) -> B.Backup:
    """Every output of ONE protected root; bk_coverage has ten words.  tilfa: the TI-LFA model of the root (ti_kind, ti_via,
    ti_metric, ti_p, ti_link are read) or None.  `refused_other` / `refused_none` / `pair_refused` / `ecmp_one_sided` / `flag_matters`
    (extra attributes) list the prefixes of the classes the tests must not be vacuous about."""
    W, K = mask.shape[2], len(cand.nbr)
    assert not (t.flags & B.PFX_ORDERED) and K <= 64 * W
    out = B.Backup(np.zeros(t.n, np.uint8), np.full(t.n, NONE, np.uint32), np.full(t.n, NONE, np.uint32), np.zeros(t.n, np.uint32),
                   np.zeros(t.n, np.uint8), np.zeros((t.n, W), np.uint64), np.zeros((t.n, W), np.uint64), np.zeros(COVERAGE_WORDS, np.uint32))
    out.refused_other, out.refused_none, out.pair_refused, out.ecmp_one_sided, out.flag_matters = [], [], [], [], []
    for p in range(t.n):
        fl = 0
        if int(r.best_entry[p]) == INF:
            kind = B.NO_ROUTE
        else:
            P = [k for k in range(K) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
            kind = B.LOCAL if not P else B.ECMP if len(P) >= 2 else B.NOTHING
        if kind >= B.ECMP:
            with_members = [e for e in P if len(mem.of(e))]
            if with_members:
                fl |= SRLG_PRIMARY
                if kind == B.ECMP and len(with_members) < len(P):
                    out.ecmp_one_sided.append(p)
            plain = B.sets_of(dist, flags, cand, root_row, nbr_row, t, p, P, int(r.best_metric[p]), lfa_flags)
            members = []
            for m in plain:
                k = m[0]
                d_np = m[2] - int(cand.cost[k])
                safe = True
                for e in with_members:
                    for i in mem.of(e):
                        local = int(mem.tail[i]) == cand.root and int(mem.pos[i]) == int(cand.root_link[k])
                        d_na = int(dist[nbr_row[k], int(mem.tail[i])])
                        safe = safe and not local and not crosses(dist, flags, t, p, d_np, d_na, mem.cost[i], int(mem.head_row[i]))
                if safe:
                    members.append(m)
                else:
                    fl |= SRLG_REFUSED
            for k, node, _, _, _ in members:
                out.bk_cand_mask[p, k // 64] |= np.uint64(1 << (k % 64))
                if node:
                    out.bk_node_mask[p, k // 64] |= np.uint64(1 << (k % 64))
        if kind == B.NOTHING:
            e = P[0]
            out.bk_primary[p] = e
            hasm = len(mem.of(e)) > 0
            if members:
                k, node, total, down, _ = min(members, key=lambda m: (not m[1], m[2], m[0]))
                kind = B.LFA
                out.bk_slot[p], out.bk_metric[p] = k, min(total, 0xFFFFFFFE)
                fl |= (B.NODE_PROTECT if node else 0) | (B.DOWNSTREAM if down else 0)
                if fl & SRLG_REFUSED:
                    out.refused_other.append(p)
            elif tilfa is not None and int(tilfa.ti_kind[e]) != 0:
                if hasm and not (lfa_flags & SAFE_REPAIRS):
                    out.flag_matters.append(p)
                else:
                    forced = int(tilfa.ti_kind[e]) == 2 and any(
                        int(mem.tail[i]) == int(tilfa.ti_p[e]) and int(mem.pos[i]) == int(tilfa.ti_link[e]) for i in mem.of(e))
                    if forced:
                        fl |= PAIR_REFUSED
                        out.pair_refused.append(p)
                    else:
                        kind = B.NODE if int(tilfa.ti_kind[e]) == 1 else B.PAIR
                        out.bk_slot[p], out.bk_metric[p] = tilfa.ti_via[e], tilfa.ti_metric[e]
            if kind == B.NOTHING and (fl & SRLG_REFUSED):
                out.refused_none.append(p)
        out.bk_kind[p], out.bk_flags[p] = kind, fl
        out.bk_coverage[kind] += 1
        out.bk_coverage[7] += bool(fl & SRLG_PRIMARY)
        out.bk_coverage[8] += bool(fl & SRLG_REFUSED)
        out.bk_coverage[9] += bool(fl & PAIR_REFUSED)
    return out
