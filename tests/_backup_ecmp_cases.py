"""The hand cases and generators of the hspf_routes_backup_ecmp_device tests (CPU: tests/test_host_backup_ecmp.py, GPU:
tests/test_gpu_backup_ecmp.py, tests/test_cpp_backup_ecmp.py).  A hand case is (graph, root, table, lfa_flags, expected) with
`expected` written out by hand: eb_ptr, the entries as (primary, kind, slot, metric, flags) and the eight coverage words, all
WITHOUT the repairs (remote=False) unless the case says otherwise.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _backup_cases as BC
import _backup_ecmp_model as BE
import _backup_model as B
import _lfa_model as M

N, D, P = BE.NODE_PROTECT, BE.DOWNSTREAM, BE.EA_PRIMARY
LFA, NOTHING = BE.LFA, BE.NOTHING
NO = 0xFFFFFFFF
Model = BC.Model


def two_homes():
    """ECMP only per PREFIX.  S = 0 with A = 1 and B = 2 at cost 1; the prefix is advertised by A and by B at metric 5.  Each of the
    two vertices has one primary, so the per-vertex call is silent; the prefix has both: d_S(p) = 6 over slot 0 and over slot 1, and
    each is the other's node-protecting downstream backup (d_B(p) = 5 by B's own entry; 5 < d(B, A) + d_A(p) = 2 + 5)."""
    g = M.csr(3, M.both([(0, 1, 1), (0, 2, 1)]))
    return g, 0, B.table([[(1, 5), (2, 5)]]), 0, ([0, 2], [(0, LFA, 1, 6, N | D | P), (1, LFA, 0, 6, N | D | P)], [1, 2, 2, 2, 2, 2, 0, 1])


def prefix_not_vertex():
    """An alternate for the PREFIX that is none for S's attaining vertex.  S = 0; A = 1, B = 2, C = 3 at cost 1; X = 4 behind A and
    B at cost 1 (two primaries); Y = 5 behind C at cost 11.  The prefix: X at metric 10, Y at metric 1.  d_S(p) = 12 through X alone
    (through Y: 13).  C: d_C(p) = 11 + 1 = 12 < d(C, S) + 12 = 13 — a member of cand(h) for both primaries, although
    d(C, X) = 3 is not below d(C, S) + d(S, X) = 3.  The choice still takes the other primary: both are node-protecting
    (d_B(p) = 11 < d(B, A) + d_A(p) = 2 + 11), a primary goes first."""
    g = M.csr(6, M.both([(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 4, 1), (3, 5, 11)]))
    return g, 0, B.table([[(4, 10), (5, 1)]]), 0, ([0, 2], [(0, LFA, 1, 12, N | D | P), (1, LFA, 0, 12, N | D | P)], [1, 2, 2, 2, 2, 2, 0, 1])


def parallel():
    """S = 0 with two links to E = 1, E - 2.  Prefix 0 sits on E at metric 0, prefix 1 on vertex 2 at metric 3: each parallel link
    backs up the other — the link, not the node (N == E)."""
    g = M.csr(3, [(0, 1, 1), (1, 0, 1), (0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 1, 1)])
    ent = [(0, LFA, 1, 1, D | P), (1, LFA, 0, 1, D | P), (0, LFA, 1, 5, D | P), (1, LFA, 0, 5, D | P)]
    return g, 0, B.table([[(1, 0)], [(2, 3)]]), 0, ([0, 2, 4], ent, [2, 4, 4, 0, 4, 4, 0, 2])


def lan_pair():
    """S = 0 on LAN 1 with A = 2 and B = 3, both one hop from 4, which advertises the prefix at 7: the two primaries (slots 2 and 3)
    share root_link 0 and protect nothing of each other; S has no other link, so there is no repair either."""
    links = [(0, 1, 1), (1, 0, 0), (2, 1, 1), (1, 2, 0), (3, 1, 1), (1, 3, 0)] + M.both([(2, 4, 1), (3, 4, 1)])
    return M.csr(5, links, net=[1]), 0, B.table([[(4, 7)]]), 0, ([0, 2], [(2, NOTHING, NO, 0, 0), (3, NOTHING, NO, 0, 0)], [1, 2, 0, 0, 0, 0, 0, 0])


HAND = {"two_homes": two_homes, "prefix_not_vertex": prefix_not_vertex, "parallel": parallel, "lan_pair": lan_pair}


def expected(case):
    """The hand-written arrays of a case in the order of BE.FIELDS."""
    ptr, ent, cov = case[4]
    col = lambda i, dt: np.array([e[i] for e in ent], dt)      # noqa: E731
    return (np.array(ptr, np.uint32), col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint8), np.array(cov, np.uint32))


# ---- shapes without hand-written arrays: the model is the expectation, a `need` on the model says what the shape is for -------------

def lan_ring():
    """lan_pair() with a long way round: S - C = 5 - F = 6 - G = 7 - 4 at cost 1 each.  C is no alternate for the prefix
    (d_C(p) = 3 + 7 is not below d(C, S) + d_S(p) = 1 + 9), so without the repairs both LAN primaries get HSPF_BK_NONE, and with them
    the per-link repair of each primary."""
    links = [(0, 1, 1), (1, 0, 0), (2, 1, 1), (1, 2, 0), (3, 1, 1), (1, 3, 0)] + M.both([(2, 4, 1), (3, 4, 1), (0, 5, 1), (5, 6, 1), (6, 7, 1), (7, 4, 1)])
    return M.csr(8, links, net=[1]), 0, B.table([[(4, 7)]])


def network_primary():
    """The graph of tests/_lfa_ecmp_cases.py's network_primary (run with HSPF_RUN_NET_NEXTHOPS): S = 0 reaches the LAN 2 over its own
    attachment (2) and through A = 1 (1 + 1).  The prefix sits on the LAN vertex: one primary's target is a network vertex."""
    links = [(0, 2, 2), (2, 0, 0), (0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 1, 0)]
    return M.csr(3, links, net=[2]), 0, B.table([[(2, 4)]])


def overload_own_entry():
    """S = 0; A = 1, B = 2 at cost 1 towards X = 4 (two primaries); C = 3 at cost 1, overloaded, advertises the prefix itself at
    metric 4 and X advertises it at metric 2: d_S(p) = 4, d_C(p) = 4 by C's OWN entry (through X it would be 3 + 2 = 5 with transit
    over S, or C - X direct at 9: 11).  C delivers without transiting: a member of cand(h) with and without HSPF_LFA_IGNORE_OVERLOAD.
    Prefix 1 (X at 2, and vertex 5 behind C at metric 1, C - 5 cost 2): d_C(p) = 3 through 5, not C's own entry: refused unless the
    overload bit is ignored."""
    g = M.csr(6, M.both([(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 4, 1), (3, 4, 9), (3, 5, 2)]), no_transit=[3])
    return g, 0, B.table([[(3, 4), (4, 2)], [(4, 2), (5, 1)]])


def saturating():
    """The four-ring of tests/test_gpu_backup.py with costs of 0x7F000000 (max_path_metric 0xFE000000), S = 0: with
    HSPF_PFX_SATURATING every term of prefix 0 saturates — a tie at 0xFFFFFFFF over both first hops."""
    c = 0x7F000000
    g = M.csr(4, M.both([(0, 1, c), (1, 2, c), (2, 3, c), (3, 0, c)]))
    lists = [[(1, 0x90000000), (3, 0x90000000)], [(1, 0x10000000), (2, 0x20000000)], [(1, 0x80FFFFFF), (2, 0x05000000)], [(2, 1), (3, 5)]]
    return g, 0, lists


def spokes(K, n_pfx, seed, far=1, ring=False, far_share=0.0):
    """Root 0 with K equal-cost spokes 1 .. K; `far` far vertices K + 1 .. K + far, each one hop from every spoke (ring: the spokes
    also form a unit-cost ring).  n_pfx prefixes: seeded, one to three advertisers among the far vertices and the spokes, small
    metrics; far_share: the share of prefixes advertised by far vertices alone, which are ECMP over all K spokes."""
    r = np.random.default_rng(seed)
    links = [(0, k, 1) for k in range(1, K + 1)] + [(k, K + 1 + f, 1) for k in range(1, K + 1) for f in range(far)]
    if ring:
        links += [(k, k % K + 1, 1) for k in range(1, K + 1)]
    n = K + 1 + far
    lists = []
    for _ in range(n_pfx):
        pool = np.arange(K + 1, n) if r.random() < far_share else np.arange(1, n)
        adv = r.choice(pool, size=min(len(pool), int(r.choice([1, 2, 3]))), replace=False)
        lists.append([(int(v), int(r.integers(0, 4))) for v in adv])
    return M.csr(n, M.both(links)), 0, lists


def grid_table(w, h, n_pfx, seed, wide=None):
    """A unit-cost w x h grid, root in a corner (almost every vertex has both of the root's links as primaries); n_pfx seeded
    prefixes with one or two advertisers at metrics 0 .. 2.  wide = (p, count): prefix p gets `count` advertisers instead, inner
    vertices at metrics that make every one of them attain the route."""
    r = np.random.default_rng(seed)
    idx = lambda x, y: y * w + x      # noqa: E731
    links = [(idx(x, y), idx(x + 1, y), 1) for y in range(h) for x in range(w - 1)] + [(idx(x, y), idx(x, y + 1), 1) for y in range(h - 1) for x in range(w)]
    n = w * h
    lists = [[(int(v), int(r.integers(0, 3))) for v in r.choice(np.arange(1, n), size=int(r.choice([1, 2])), replace=False)] for _ in range(n_pfx)]
    if wide is not None:
        inner = [idx(x, y) for y in range(1, h) for x in range(1, w)]
        lists[wide[0]] = [(int(v), 40 - int(v) % w - int(v) // w) for v in r.choice(inner, size=wide[1], replace=False)]
    return M.csr(n, M.both(links)), 0, lists


def many_slots():
    """More candidate slots than one LDS chunk of the fill kernel holds (2 048): S = 0 with 1 800 parallel links to C = 3 at cost 2,
    then 254 to A = 1 and 3 to B = 2 at cost 1; X = 4 one hop behind each of them.  Prefix 0 sits on X: 257 primaries (more than the
    256 entries one round of the walk takes) judged against 2 057 candidates in two chunks — a link to A takes the first link to B,
    slot 2 054, out of the second chunk; prefix 1 on B: its three links."""
    links = []
    for v, count, c in ((3, 1800, 2), (1, 254, 1), (2, 3, 1)):
        for _ in range(count):
            links += [(0, v, c), (v, 0, c)]
    links += M.both([(1, 4, 1), (2, 4, 1), (3, 4, 1)])
    return M.csr(5, links), 0, [[(4, 0)], [(2, 0)]]


def chain_table(n):
    """A path with the root in the middle: no ECMP anywhere."""
    g = M.csr(n, M.both([(v, v + 1, 1 + v % 3) for v in range(n - 1)]))
    return g, n // 2, [[(v, 1)] for v in range(n)]


def random_multihomed(seed):
    """8 - 24 routers on a tree plus a few chords (rings: repairs are needed) with tie-heavy, partly asymmetric costs from [1, 3], up
    to two LANs — the root S is on the first — some overloaded routers; prefixes with one to three advertisers at metrics 0 .. 3,
    so that per-prefix ties are common."""
    r = np.random.default_rng(seed)
    nr = int(r.integers(8, 25))
    n_lan = int(r.integers(0, 3))
    S = int(r.integers(0, nr))
    und = {(v, int(r.integers(0, v))) for v in range(1, nr)}
    for _ in range(int(r.integers(1, max(2, nr // 2)))):
        a, b = (int(x) for x in r.integers(0, nr, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        c1 = int(r.integers(1, 4))
        c2 = c1 if r.random() < 0.8 else int(r.integers(1, 4))
        links += [(a, b, c1), (b, a, c2)]
    for i in range(n_lan):
        members = {int(m) for m in r.choice(nr, size=int(r.integers(2, 5)), replace=False)} | ({S} if i == 0 else set())
        for m in sorted(members):
            links += [(m, nr + i, int(r.integers(1, 3))), (nr + i, m, 0)]
    overloaded = [int(v) for v in range(nr) if r.random() < 0.12 and v != S]
    g = M.csr(nr + n_lan, links, net=range(nr, nr + n_lan), no_transit=overloaded)
    lists = []
    for _ in range(int(r.integers(nr, 3 * nr))):
        adv = r.choice(nr, size=int(r.choice([1, 2, 2, 3])), replace=False)
        lists.append([(int(v), int(r.integers(0, 4))) for v in adv])
    return g, S, B.table(lists)


SMALL_SEEDS = list(range(24))
# chosen on the CPU: every graph has ECMP prefixes, together they show every kind and every flag bit (14 of them need a repair)
GPU_SEEDS = [7101, 7104, 7105, 7106, 7107, 7108, 7109, 7110, 7111, 7114, 7117, 7118, 7119, 7120, 7121, 7122, 7123, 7124, 7125, 7126, 7127, 7128,
             7130, 7132, 7134, 7135, 7137, 7145, 7152, 7156, 7163, 7179, 7183, 7204, 7222, 7224]
