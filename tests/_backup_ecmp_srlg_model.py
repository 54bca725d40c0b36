"""Per-primary SRLG-safe backups of ECMP prefixes (hspf_routes_backup_ecmp_srlg_device) in plain Python ON TOP of
tests/_backup_ecmp_model.py and tests/_backup_srlg_model.py: the expected values of tests/test_host_backup_ecmp_srlg.py,
tests/test_gpu_backup_ecmp_srlg.py and tests/test_cpp_backup_ecmp_srlg.py.  The plain cand(h), node(h) and the order of the choice
are _backup_ecmp_model.members_of and its key; crosses_p is _backup_srlg_model.crosses; this file joins them per ENTRY (p, h) over
the members of h alone, as include/holo_spf_hip.h ("per-primary SRLG-safe backups for ECMP prefixes") says, and applies the
fallback rule of the per-prefix SRLG call to h.  It never touches the engine.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import _backup_ecmp_model as BE
import _backup_srlg_model as BS
import _lfa_model as M
import _srlg_model as SM

INF = NONE = 0xFFFFFFFF
LFA, NODE, PAIR, NOTHING = BE.LFA, BE.NODE, BE.PAIR, BE.NOTHING
NODE_PROTECT, DOWNSTREAM, EA_PRIMARY = BE.NODE_PROTECT, BE.DOWNSTREAM, BE.EA_PRIMARY
SAFE_REPAIRS = BS.SAFE_REPAIRS
SRLG_PRIMARY, PAIR_REFUSED, SRLG_REFUSED = BS.SRLG_PRIMARY, BS.PAIR_REFUSED, BS.SRLG_REFUSED
COVERAGE_WORDS = 11
FIELDS = BE.FIELDS


def safe_for(dist, flags, cand: M.Cand, nbr_row, mem: SM.Members, t, p, h, k, d_np):
    """Candidate k with d_{N_k}(p) = d_np against the members of h: none is local to k, none is crossed."""
    for i in mem.of(h):
        if int(mem.tail[i]) == cand.root and int(mem.pos[i]) == int(cand.root_link[k]):
            return False
        if BS.crosses(dist, flags, t, p, d_np, int(dist[nbr_row[k], int(mem.tail[i])]), mem.cost[i], int(mem.head_row[i])):
            return False
    return True


def backup_ecmp_srlg(dist, flags, mask, cand: M.Cand, root_row, nbr_row, mem: SM.Members, t, r, lfa_flags=0, tilfa=None, *, sets=False) -> BE.BackupEcmp:
    """The stream of ONE protected root; eb_coverage has eleven words.  tilfa: the TI-LFA model of the root (ti_kind, ti_via,
    ti_metric, ti_p, ti_link are read) or None."""
    K = len(cand.nbr)
    assert not (t.flags & BE.B.PFX_ORDERED) and K <= 64 * mask.shape[2]
    ptr = [0]
    ent, pfx, s_cand, s_node = [], [], [], []
    cov = [0] * COVERAGE_WORDS
    for p in range(t.n):
        P = []
        if int(r.best_entry[p]) != INF:
            P = [k for k in range(K) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
        if len(P) < 2:
            ptr.append(ptr[-1])
            continue
        cov[0] += 1
        backed, memo = True, {}
        for h in P:
            plain = BE.members_of(dist, flags, cand, nbr_row, t, p, P, h, int(r.best_metric[p]), lfa_flags, memo)
            hasm = len(mem.of(h)) > 0
            fl = SRLG_PRIMARY if hasm else 0
            kept = [m for m in plain if safe_for(dist, flags, cand, nbr_row, mem, t, p, h, m[0], m[3] - int(cand.cost[m[0]]))]
            if len(kept) < len(plain):
                fl |= SRLG_REFUSED
            kind, slot, metric = NOTHING, NONE, 0
            if kept:
                k, node, prim, total, down = min(kept, key=lambda m: (not m[1], not m[2], m[3], m[0]))
                kind, slot, metric = LFA, k, min(total, 0xFFFFFFFE)
                fl |= (NODE_PROTECT if node else 0) | (DOWNSTREAM if down else 0) | (EA_PRIMARY if prim else 0)
            elif tilfa is not None and int(tilfa.ti_kind[h]) != 0 and (not hasm or lfa_flags & SAFE_REPAIRS):
                forced = hasm and int(tilfa.ti_kind[h]) == 2 and any(
                    int(mem.tail[i]) == int(tilfa.ti_p[h]) and int(mem.pos[i]) == int(tilfa.ti_link[h]) for i in mem.of(h))
                if forced:
                    fl |= PAIR_REFUSED
                else:
                    kind = NODE if int(tilfa.ti_kind[h]) == 1 else PAIR
                    slot, metric = int(tilfa.ti_via[h]), int(tilfa.ti_metric[h])
            ent.append((h, kind, slot, metric, fl))
            pfx.append(p)
            if sets:
                s_cand.append({m[0] for m in kept})
                s_node.append({m[0] for m in kept if m[1]})
            cov[1] += 1
            cov[2] += kind == LFA
            cov[3] += bool(fl & NODE_PROTECT)
            cov[4] += bool(fl & DOWNSTREAM)
            cov[5] += bool(fl & EA_PRIMARY)
            cov[6] += kind in (NODE, PAIR)
            cov[8] += bool(fl & SRLG_PRIMARY)
            cov[9] += bool(fl & SRLG_REFUSED)
            cov[10] += bool(fl & PAIR_REFUSED)
            backed = backed and kind != NOTHING
        cov[7] += backed
        ptr.append(ptr[-1] + len(P))
    col = lambda i, dt: np.array([e[i] for e in ent], dt)      # noqa: E731
    return BE.BackupEcmp(np.array(ptr, np.uint32), col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint8),
                         np.array(cov, np.uint32), np.array(pfx, np.uint32), s_cand if sets else None, s_node if sets else None)


stack = BE.stack


def want(model, lfa_flags=0, remote=True, table=None, tilfa=None, mems=None, **kw):
    """[BackupEcmp] of the protected roots of a tests/_backup_srlg_cases.py Model (its rows hold the member endpoints); the repairs
    are the model's chain on the SRLG-safe tables, or `tilfa` ([TI-LFA tables per root])."""
    f, t = model.fwd, table or model.table
    ti = tilfa if tilfa is not None else [x[2] for x in model.frr(lfa_flags)] if remote else [None] * len(model.prot)
    return [backup_ecmp_srlg(f.dist, f.flags, f.mask, c, rr, nr, mem, t, model.routes(i, t), lfa_flags, ti[i], **kw)
            for i, (c, rr, nr, mem) in enumerate(zip(model.cands, model.root_row, model.nbr_row, mems or model.mems))]


def want_plain(model, lfa_flags=0, tilfa=None, table=None, **kw):
    """[BackupEcmp] of the PLAIN ECMP model on the same rows and routes (tilfa: [TI-LFA tables per root] or None)."""
    f, t = model.fwd, table or model.table
    ti = tilfa if tilfa is not None else [None] * len(model.prot)
    return [BE.backup_ecmp(f.dist, f.flags, f.mask, c, rr, nr, t, model.routes(i, t), lfa_flags & ~SAFE_REPAIRS, ti[i], **kw)
            for i, (c, rr, nr) in enumerate(zip(model.cands, model.root_row, model.nbr_row))]
