"""The hand cases and generators of the hspf_routes_backup_ecmp_srlg_device tests (CPU: tests/test_host_backup_ecmp_srlg.py, GPU:
tests/test_gpu_backup_ecmp_srlg.py, tests/test_cpp_backup_ecmp_srlg.py).  A hand case is a dict: graph, root, groups (grp_ptr, grp),
table, and `expect`, a list of (lfa_flags, tilfa or None, eb_ptr, entries as (primary, kind, slot, metric, flags), the eleven
coverage words) with every array written out by hand; `mem` (optional) replaces the members derived from the groups with
hand-written ones.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _backup_ecmp_cases as EC
import _backup_ecmp_srlg_model as BES
import _backup_model as B
import _backup_srlg_cases as SC
import _lfa_model as M
import _srlg_model as SM

N, D, P = BES.NODE_PROTECT, BES.DOWNSTREAM, BES.EA_PRIMARY
SP, PR, SR = BES.SRLG_PRIMARY, BES.PAIR_REFUSED, BES.SRLG_REFUSED
LFA, NODE, PAIR, NOTHING = BES.LFA, BES.NODE, BES.PAIR, BES.NOTHING
SAFE = BES.SAFE_REPAIRS
NO = 0xFFFFFFFF
Model = SC.Model


def conduit_pair():
    """S = 0; A = 1, B = 2 and C = 3 at cost 1 (slots 0, 1, 2); X = 4 behind A and B at cost 1 and behind C at cost 2; the prefix is
    on X at metric 0.  S -> A and S -> B share a group.  The plain ECMP call gives each of slots 0 / 1 the other (node | downstream
    | primary, metric 2).  Here the other primary's own first link is a member of h (local): refused.  C is left: cost 1 +
    d_C(p) = 2, node-protecting (2 < d(C, A) + d_A(p) = 2 + 1), not downstream (d_C(p) = 2 is not below d_S(p) = 2)."""
    g = M.csr(5, M.both([(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 4, 1), (3, 4, 2)]))
    ent = [(0, LFA, 2, 3, N | SR | SP), (1, LFA, 2, 3, N | SR | SP)]
    return dict(graph=g, root=0, groups=SC.group(g, (0, 1), (0, 2)), table=B.table([[(4, 0)]]),
                plain=[(0, LFA, 1, 2, N | D | P), (1, LFA, 0, 2, N | D | P)],
                expect=[(0, None, [0, 2], ent, [1, 2, 2, 2, 0, 0, 0, 1, 2, 2, 0])])


def multihomed():
    """conduit_pair with Y = 5 one hop behind C (cost 1); the prefix is on X at metric 0 and on Y at metric 1; C -> Y is in the
    conduit's group too.  d_S(p) = 2 over A and B.  C's shortest path to X, S's attaining vertex, is its own link (2 < d(C, C) + 1 +
    d(Y, X) = 4: the per-vertex reasoning admits C), but d_C(p) = 2 is also attained through Y over the member: 2 >= 0 + 1 + 1.
    Refused per prefix; the other primary is local: both entries are HSPF_BK_NONE."""
    g = M.csr(6, M.both([(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 4, 1), (3, 4, 2), (3, 5, 1)]))
    ent = [(0, NOTHING, NO, 0, SR | SP), (1, NOTHING, NO, 0, SR | SP)]
    return dict(graph=g, root=0, groups=SC.group(g, (0, 1), (0, 2), (3, 5)), table=B.table([[(4, 0), (5, 1)]]),
                expect=[(0, None, [0, 2], ent, [1, 2, 0, 0, 0, 0, 0, 0, 2, 2, 0])])


def unreachable():
    """S = 0; A = 1, B = 2 at cost 1, X = 4 behind both, the prefix on X.  S -> A shares a group with 5 -> 6, whose tail nothing
    reaches (5 has no incoming link); S -> B with 4 -> 7, whose head 7 reaches nothing.  Neither member refuses anything: the plain
    answers, with HSPF_BK_SRLG_PRIMARY on both entries."""
    g = M.csr(8, M.both([(0, 1, 1), (0, 2, 1), (1, 4, 1), (2, 4, 1)]) + [(5, 6, 1), (6, 4, 1), (4, 7, 1)])
    of = {SM.link_pos(g, 0, 1): [5], SM.link_pos(g, 5, 6): [5], SM.link_pos(g, 0, 2): [6], SM.link_pos(g, 4, 7): [6]}
    ent = [(0, LFA, 1, 2, N | D | P | SP), (1, LFA, 0, 2, N | D | P | SP)]
    return dict(graph=g, root=0, groups=SM.groups_csr(len(g[1]), of), table=B.table([[(4, 0)]]),
                expect=[(0, None, [0, 2], ent, [1, 2, 2, 2, 2, 2, 0, 1, 2, 0, 0])])


class Repairs:
    """Hand-written per-slot repairs of one root (64 slots): {slot: (kind, via, metric, p, link)}."""

    def __init__(self, of):
        self.ti_kind = np.zeros(64, np.uint8)
        self.ti_via, self.ti_p, self.ti_link = (np.full(64, NO, np.uint32) for _ in range(3))
        self.ti_metric = np.zeros(64, np.uint32)
        for s, (k, via, met, p, link) in of.items():
            self.ti_kind[s], self.ti_via[s], self.ti_metric[s], self.ti_p[s], self.ti_link[s] = k, via, met, p, link


def fallback():
    """lan_ring() of tests/_backup_ecmp_cases.py: S = 0 on LAN 1 with A = 2 (slot 3) and B = 3 (slot 4), both one hop from 4, which
    advertises the prefix; the long way round over C = 5 (slot 1) is no alternate, and the two primaries share their first link:
    neither has an alternate.  The members are written by hand: slot 3 has ONE member, the link 2 -> 4 (position 1 of A's row);
    slot 4 has none.  The repairs are written by hand too: one segment through slot 1 at 4 for both, and in the third run a pair
    for slot 3 whose forced adjacency (2, 1) is that member."""
    g, S, t = EC.lan_ring()
    mem = SM.Members(np.array([0, 0, 0, 0, 1, 1], np.uint32), *(np.array([x], np.uint32) for x in (2, 1, 4, 1)))
    node = Repairs({3: (1, 1, 4, NO, NO), 4: (1, 1, 4, NO, NO)})
    pair = Repairs({3: (2, 1, 4, 2, 1), 4: (1, 1, 4, NO, NO)})
    return dict(graph=g, root=S, groups=SC.group(g, (0, 1), (2, 4)), table=t, mem=mem,
                expect=[(0, node, [0, 2], [(3, NOTHING, NO, 0, SP), (4, NODE, 1, 4, 0)], [1, 2, 0, 0, 0, 0, 1, 0, 1, 0, 0]),
                        (SAFE, node, [0, 2], [(3, NODE, 1, 4, SP), (4, NODE, 1, 4, 0)], [1, 2, 0, 0, 0, 0, 2, 1, 1, 0, 0]),
                        (SAFE, pair, [0, 2], [(3, NOTHING, NO, 0, SP | PR), (4, NODE, 1, 4, 0)], [1, 2, 0, 0, 0, 0, 1, 0, 1, 0, 1])])


HAND = {"conduit_pair": conduit_pair, "multihomed": multihomed, "unreachable": unreachable, "fallback": fallback}


def model_of(case):
    """The Model of a hand case: the rows are those of the groups ([S] ++ neighbour routers ++ member endpoints); hand-written
    members take the place of the derived ones, their rows looked up in that list."""
    m = Model(case["graph"], [case["root"]], *case["groups"], case["table"])
    if "mem" in case:
        mem = case["mem"]
        row_of = {int(v): i for i, v in enumerate(m.roots)}
        mem.tail_row = np.array([row_of[int(x)] for x in mem.tail], np.uint32)
        mem.head_row = np.array([row_of[int(x)] for x in mem.head], np.uint32)
        m.mems = [mem]
    return m


def expected(exp):
    """The hand-written arrays of one `expect` row in the order of BES.FIELDS."""
    _, _, ptr, ent, cov = exp
    col = lambda i, dt: np.array([e[i] for e in ent], dt)      # noqa: E731
    return (np.array(ptr, np.uint32), col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint8), np.array(cov, np.uint32))


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------

def seeded(seed):
    """(graph, S, (grp_ptr, grp), Table): random_multihomed() of tests/_backup_ecmp_cases.py — tie-heavy, so ECMP prefixes are
    common — with one to four groups of two to five links, each through S's row."""
    g, S, t = EC.random_multihomed(seed)
    return g, S, SC.random_groups(g, seed, n_groups=(1, 5), per_group=(2, 6), root=S), t


def symmetric(seed):
    """(graph, S, (grp_ptr, grp), Table) with symmetric costs from [1, 3], no LAN and no overloaded router: 10 - 20 routers on a
    tree plus chords; prefixes with one to three advertisers other than S at metrics 0 .. 3; groups as in seeded()."""
    r = np.random.default_rng(seed)
    nr = int(r.integers(10, 21))
    und = {(v, int(r.integers(0, v))) for v in range(1, nr)}
    for _ in range(nr):
        a, b = (int(x) for x in r.integers(0, nr, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    g = M.csr(nr, M.both([(a, b, int(r.integers(1, 4))) for a, b in sorted(und)]))
    S = int(r.integers(0, nr))
    others = np.array([v for v in range(nr) if v != S])
    lists = [[(int(v), int(r.integers(0, 4))) for v in r.choice(others, size=int(r.choice([1, 2, 2, 3])), replace=False)] for _ in range(2 * nr)]
    return g, S, SC.random_groups(g, seed, n_groups=(2, 5), per_group=(2, 5), root=S), B.table(lists)


def forged_pair(model, lfa_flags=0):
    """The model's repairs with every member primary's repair turned into a pair whose forced adjacency is the primary's first
    member: [object with ti_* per root].  What HSPF_BK_SRLG_PAIR_REFUSED needs and random graphs almost never give."""
    out = []
    for x, mem, c in zip(model.frr(lfa_flags), model.mems, model.cands):
        ti = x[2]
        f = Repairs({})
        for k in ("ti_kind", "ti_via", "ti_metric", "ti_p", "ti_link"):
            a = np.array(getattr(ti, k)).copy()
            setattr(f, k, a)
        for h in range(len(c.nbr)):
            if len(mem.of(h)) and f.ti_kind[h]:
                i = mem.of(h)[0]
                f.ti_kind[h], f.ti_p[h], f.ti_link[h] = 2, mem.tail[i], mem.pos[i]
        out.append(f)
    return out


# chosen on the CPU (tests/test_host_backup_ecmp_srlg.py holds what they reach): every graph has ECMP prefixes whose primaries have members
GPU_SEEDS = [7106, 7108, 7109, 7117, 7122, 7127, 7132, 7145, 7152, 7163, 7183, 7224]
SYM_SEEDS = list(range(8200, 8216))
