"""The seams of the member lane that hspf_routes_backup_srlg_device and hspf_routes_backup_ecmp_srlg_device share (BkMembers,
holo_amd/csrc/spf_backup_srlg.hip.h), on the GPU, bit for bit against the models: a pseudonode primary with members (no d_E(p) next
to the first member stream), a member-free primary next to one with 16 members, an ECMP prefix whose primaries have 8 and 9
members on a hub of 65, the one-primary choice of the per-prefix call against the per-primary model's rule, and the repairs absent
/ given without HSPF_LFA_SRLG_SAFE_REPAIRS.  Every draw was chosen on the CPU; each case asserts on the MODEL that the branch it
is about is taken before anything runs on the device."""
import numpy as np
import pytest

import _backup_ecmp_model as BE
import _backup_ecmp_srlg_model as BES
import _backup_model as B
import _backup_srlg_cases as SC
import _backup_srlg_model as BS
import _lfa_model as M
import _srlg_model as SM
from test_gpu_backup import HUB_SEEDS
from test_gpu_backup_srlg import Device, assert_equal, check, random_table
from test_gpu_rlfa import hub, lan

pytestmark = pytest.mark.gpu

RUN_NET_NEXTHOPS = 0x01          # HSPF_RUN_NET_NEXTHOPS: a network next to the root gets its own first-hop slot
SRLG_BITS = BS.SRLG_PRIMARY | BS.PAIR_REFUSED | BS.SRLG_REFUSED
ONE_PRIMARY_FIELDS = ("bk_kind", "bk_primary", "bk_slot", "bk_metric", "bk_flags", "bk_cand_mask", "bk_node_mask")


def group_of(graph, first, others, gid=1):
    """(grp_ptr, grp): link `first` and the links `others` (positions in the graph's column array) in one group."""
    return SM.groups_csr(len(graph[1]), {int(l): [gid] for l in [first] + list(others)})


# ------------------------------------------------------------------------------------------ 1, 5: a pseudonode primary with 9 members

def pseudonode_case():
    """tests/test_gpu_rlfa.py's LAN, S = 1, run with HSPF_RUN_NET_NEXTHOPS.  Prefix 0 sits on the
    pseudonode 0: its one primary is the pseudonode's slot (nbr == NONE:
    no d_E(p)), and S's link to the LAN shares a group with the nine links 5 <-> 6, 2 <-> 6, 3 <-> 6, 4 <-> 6 and 6 -> 7.  The only
    candidate of another root_link is C = 5: d_5(p) = 16 = w(5 -> 6) + d_6(p), crossed."""
    g = lan()
    far = [SM.link_pos(g, u, v) for u, v in ((5, 6), (6, 5), (2, 6), (6, 2), (3, 6), (6, 3), (4, 6), (6, 4), (6, 7))]
    gp, gr = group_of(g, SM.link_pos(g, 1, 0), far)
    t = B.table([[(0, 0)], [(0, 3), (7, 30)], [(5, 0)], [(7, 0)], [(0, 0), (5, 0)]])
    return SC.Model(g, [1], gp, gr, t, run_flags=RUN_NET_NEXTHOPS)


def test_a_pseudonode_primary_with_nine_members_with_and_without_the_repairs(spf_ctx):
    """Cases 1 and 5: flags 0 and HSPF_LFA_SRLG_SAFE_REPAIRS, tilfa given and NULL."""
    m = pseudonode_case()

    def need(w):
        e = int(w[0].bk_primary[0])
        assert w[0].bk_kind[0] != B.ECMP and m.cands[0].nbr[e] == M.NONE and np.diff(m.mems[0].mem_ptr)[e] == 9
        assert w[0].bk_flags[0] & BS.SRLG_PRIMARY and w[0].bk_flags[0] & BS.SRLG_REFUSED and w[0].bk_coverage[8] > 0
        assert w[0].bk_kind[0] == B.NOTHING          # no slot was left: the epilogue's repair branch is reached (no slot of this graph has a repair)
    check(spf_ctx, m, lfa_flags=(0, BS.SAFE_REPAIRS), remotes=(True, False), need=need)


# ------------------------------------------------------------------- 2: a router primary with no members next to one with 16, 257 prefixes

def sixteen_case():
    """The hub of 17 of tests/test_gpu_backup_srlg.py: slot 8 shares a group with 16 links among the neighbours, no other slot has a
    member; 257 prefixes, one more than a tile."""
    g = hub(17, 3)
    rp, col = g[0], g[1]
    far = [l for u in range(1, 18) for l in range(int(rp[u]), int(rp[u + 1])) if int(col[l]) != 0]
    gp, gr = group_of(g, int(rp[0]) + 8, np.random.default_rng(0).choice(far, 16, replace=False))
    return SC.Model(g, [0], gp, gr, random_table(np.random.default_rng(5), 18, 257))


def test_a_member_free_primary_next_to_one_with_16_members_equals_the_plain_call(spf_ctx):
    m = sixteen_case()
    w = m.want(BS.SAFE_REPAIRS)[0]
    sizes = np.diff(m.mems[0].mem_ptr)
    one = (w.bk_kind != B.ECMP) & (w.bk_primary != M.NONE)
    free = one & (sizes[np.where(one, w.bk_primary, 0)] == 0)
    assert sizes[8] == SM.MAX_MEMBERS == 16 and sizes.sum() == 16 and m.table.n == 257
    assert free.sum() > 20 and free[256] and ((w.bk_primary == 8) & (w.bk_flags & BS.SRLG_REFUSED != 0)).any() and w.bk_coverage[8] > 0
    d = Device(spf_ctx, m)
    try:
        r = d.routes(m.table)
        for lf in (0, BS.SAFE_REPAIRS):
            for rem in (True, False):
                got = d.backup(m.table, lf, rem, routes=r)
                assert_equal(got, m.want(lf, rem), tag=(lf, rem))
                plain = d.backup(m.table, 0, rem, routes=r, plain=True)
                for name in ONE_PRIMARY_FIELDS:
                    assert np.array_equal(got[name][0][free], plain[name][0][free]), (name, lf, rem)
                assert not (got["bk_flags"][0][free] & SRLG_BITS).any()
    finally:
        d.free()


# ------------------------------------------------------------- 3: an ECMP prefix on a hub of 65 whose primaries have 8 and 9 members

ECMP_SEED = 4          # chosen on the CPU (ecmp_case's assertions hold for it)


def refusals(m, p):
    """(primaries, slots refused for a member local to them, slots refused for a crossed member alone, the plain candidates) of
    prefix p, from the model's pieces."""
    f, c, nr, mem, t = m.fwd, m.cands[0], m.nbr_row[0], m.mems[0], m.table
    r = m.routes(0)
    P = [k for k in range(len(c.nbr)) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
    local, crossed = [], []
    plain = B.sets_of(f.dist, f.flags, c, m.root_row[0], nr, t, p, P, int(r.best_metric[p]), 0)
    for k, _, total, _, _ in plain:
        d_np = total - int(c.cost[k])
        ms = [i for e in P for i in mem.of(e)]
        if any(int(mem.tail[i]) == c.root and int(mem.pos[i]) == int(c.root_link[k]) for i in ms):
            local.append(k)
        elif any(BS.crosses(f.dist, f.flags, t, p, d_np, int(f.dist[nr[k], int(mem.tail[i])]), mem.cost[i], int(mem.head_row[i])) for i in ms):
            crossed.append(k)
    return P, local, crossed, [k for k, *_ in plain]


def ecmp_case(seed=ECMP_SEED):
    """The hub of 65 (two mask words).  Prefix 0 is advertised by two neighbours a, b at metrics that make S's two direct links tie.
    S -> a shares group 1 with 8 links (one of them the link of S's row behind a plain candidate of the prefix: local to it), S -> b group 2 with 9 links among
    the neighbours.  The other prefixes are random."""
    g = hub(65, HUB_SEEDS[65])
    rp, col, met = g[0], g[1], g[2]
    r = np.random.default_rng(seed)
    f = SC.Model(g, [0], *SM.groups_csr(len(col), {}), B.table([[(1, 0)]])).fwd
    direct = [v for v in range(1, 66) if int(f.dist[0, v]) == int(met[int(rp[0]) + v - 1]) and bin(int(f.mask[0, v, 0]) | int(f.mask[0, v, 1]) << 64).count("1") == 1]
    a, b = (int(x) for x in r.choice(direct, 2, replace=False))
    top = max(int(f.dist[0, a]), int(f.dist[0, b]))
    far = [l for u in range(1, 66) for l in range(int(rp[u]), int(rp[u + 1])) if int(col[l]) != 0]
    pick = [int(x) for x in r.choice(far, 16, replace=False)]
    first = [(a, top - int(f.dist[0, a])), (b, top - int(f.dist[0, b]))]
    m0 = SC.Model(g, [0], *SM.groups_csr(len(col), {}), B.table([first]))                     # no groups: the plain candidates of prefix 0
    local = refusals(m0, 0)[3][0]
    of = {int(rp[0]) + a - 1: [1], int(rp[0]) + b - 1: [2], int(rp[0]) + int(m0.cands[0].root_link[local]): [1]}
    for i, l in enumerate(pick):
        of.setdefault(l, []).append(1 if i < 7 else 2)
    gp, gr = SM.groups_csr(len(col), of)
    lists = [first]
    t = random_table(r, 66, 40)
    lists += [[(v, mm) for v, mm, _ in t.entries(p)] for p in range(t.n)]
    return SC.Model(g, [0], gp, gr, B.table(lists))


def test_an_ecmp_prefix_whose_primaries_have_8_and_9_members_on_a_hub_of_65(spf_ctx):
    m = ecmp_case()

    def need(w):
        P, local, crossed, _ = refusals(m, 0)
        sizes = np.diff(m.mems[0].mem_ptr)
        assert m.W == 2 and w[0].bk_kind[0] == B.ECMP and len(P) == 2 and sorted(int(sizes[e]) for e in P) == [8, 9]
        assert len(local) >= 1 and len(crossed) >= 1 and w[0].bk_flags[0] & BS.SRLG_REFUSED
        cand = [k for k in range(65) if int(w[0].bk_cand_mask[0, k // 64]) >> (k % 64) & 1]
        assert cand and not set(cand) & set(local + crossed)                                # (W == 2: every walk over the primaries takes two words)
    check(spf_ctx, m, need=need)


# ----------------------------------------------------------------- 4: the per-prefix call's one-primary choice is the per-primary rule's

def per_primary_rule(m, lfa_flags, ti):
    """What tests/_backup_ecmp_srlg_model.py's rule gives for the ONE primary h of every prefix that has exactly one: cand(h) of
    _backup_ecmp_model.members_of over P = [h], held against the members of h by safe_for, the choice by (node, sum, slot) — the
    per-primary key without its "is a primary" term, which no slot of cand(h) has when h is the only primary — and the fallback of
    backup_ecmp_srlg.  {p: (kind, slot, metric, flags)}; flags: NODE_PROTECT, DOWNSTREAM and the three SRLG bits."""
    f, c, nr, mem, t = m.fwd, m.cands[0], m.nbr_row[0], m.mems[0], m.table
    r, out = m.routes(0), {}
    for p in range(t.n):
        if int(r.best_entry[p]) == M.NONE:
            continue
        P = [k for k in range(len(c.nbr)) if (int(r.nexthop_mask[p, k // 64]) >> (k % 64)) & 1]
        if len(P) != 1:
            continue
        h = P[0]
        plain = BE.members_of(f.dist, f.flags, c, nr, t, p, P, h, int(r.best_metric[p]), lfa_flags & ~BS.SAFE_REPAIRS)
        kept = [x for x in plain if BES.safe_for(f.dist, f.flags, c, nr, mem, t, p, h, x[0], x[3] - int(c.cost[x[0]]))]
        hasm = len(mem.of(h)) > 0
        fl = (BS.SRLG_PRIMARY if hasm else 0) | (BS.SRLG_REFUSED if len(kept) < len(plain) else 0)
        kind, slot, metric = B.NOTHING, M.NONE, 0
        if kept:
            k, node, _, total, down = min(kept, key=lambda x: (not x[1], x[3], x[0]))
            kind, slot, metric = B.LFA, k, min(total, 0xFFFFFFFE)
            fl |= (B.NODE_PROTECT if node else 0) | (B.DOWNSTREAM if down else 0)
        elif ti is not None and int(ti.ti_kind[h]) != 0 and (not hasm or lfa_flags & BS.SAFE_REPAIRS):
            if hasm and int(ti.ti_kind[h]) == 2 and any(int(mem.tail[i]) == int(ti.ti_p[h]) and int(mem.pos[i]) == int(ti.ti_link[h]) for i in mem.of(h)):
                fl |= BS.PAIR_REFUSED
            else:
                kind, slot, metric = (B.NODE if int(ti.ti_kind[h]) == 1 else B.PAIR), int(ti.ti_via[h]), int(ti.ti_metric[h])
        out[p] = (kind, slot, metric, fl)
    return out


@pytest.mark.parametrize("seed", [SC.RANDOM_SEED + 2])
def test_the_one_primary_choice_is_the_per_primary_rule(spf_ctx, seed):
    """The comparison, exactly: for every prefix with exactly one primary h, bk_kind, bk_slot, bk_metric and bk_flags (all eight bits:
    the per-prefix call sets no bit outside NODE_PROTECT, DOWNSTREAM and the three SRLG bits) of the per-prefix call are those of
    per_primary_rule, and bk_primary is h."""
    g, S, (gp, gr), t = SC.random_case(seed)
    m = SC.Model(g, [S], gp, gr, t)
    lf = BS.SAFE_REPAIRS
    rule = per_primary_rule(m, lf, m.frr(lf)[0][2])
    w = m.want(lf)[0]
    assert len(rule) >= 10 and any(v[3] & BS.SRLG_REFUSED for v in rule.values()) and any(v[0] == B.LFA and v[3] & BS.SRLG_PRIMARY for v in rule.values())
    assert any(v[0] in (B.NODE, B.PAIR) for v in rule.values())
    for p, v in rule.items():                                      # the two models agree: the device is held against both
        assert (int(w.bk_kind[p]), int(w.bk_slot[p]), int(w.bk_metric[p]), int(w.bk_flags[p])) == v, p
    d = Device(spf_ctx, m)
    try:
        got = d.backup(t, lf, True)
        assert_equal(got, m.want(lf))
        for p, v in rule.items():
            assert (int(got["bk_kind"][0][p]), int(got["bk_slot"][0][p]), int(got["bk_metric"][0][p]), int(got["bk_flags"][0][p])) == v, p
            assert int(got["bk_primary"][0][p]) == int(w.bk_primary[p])
    finally:
        d.free()
