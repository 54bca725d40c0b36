"""The hand cases and generators of the hspf_lfa_ecmp_device tests (CPU: tests/test_host_lfa_ecmp.py, GPU: tests/test_gpu_lfa_ecmp.py,
tests/test_cpp_lfa_ecmp.py).  A hand case is (graph, root, lfa_flags, expected) with `expected` written out by hand: ea_ptr, the
entries as (primary, slot, metric, flags) and the seven coverage words.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _lfa_model as M

L, N, D, P = 0x04, 0x08, 0x10, 0x20          # LINK_PROTECT, NODE_PROTECT, DOWNSTREAM, EA_PRIMARY
NO = 0xFFFFFFFF


def diamond():
    """S = 0, A = 1, B = 2, D = 3, all costs 1: each primary is the other's node-protecting downstream alternate."""
    g = M.csr(4, M.both([(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)]))
    return g, 0, 0, ([0, 0, 0, 0, 2], [(0, 1, 2, L | N | D | P), (1, 0, 2, L | N | D | P)], [1, 2, 2, 2, 2, 2, 1])


def parallel(with_c=True):
    """S = 0 with two links to E = 1, E - D = 2; C = 3 on the detour S - C - D (2, 2) protects the node E for D and is no primary.
    With C each parallel link gets C (node before primary); without C each gets the other link: the link, not the node."""
    links = [(0, 1, 1), (1, 0, 1), (0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 1, 1)]
    if not with_c:
        return M.csr(3, links), 0, 0, ([0, 0, 2, 4], [(0, 1, 1, L | D | P), (1, 0, 1, L | D | P), (0, 1, 2, L | D | P), (1, 0, 2, L | D | P)],
                                       [2, 4, 4, 0, 4, 4, 2])
    links += M.both([(0, 3, 2), (3, 2, 2)])
    return M.csr(4, links), 0, 0, ([0, 0, 2, 4, 4], [(0, 1, 1, L | D | P), (1, 0, 1, L | D | P), (0, 2, 4, L | N), (1, 2, 4, L | N)],
                                   [2, 4, 4, 2, 2, 2, 2])


def lan(third=False):
    """S = 0 on LAN 1 with A = 2 and B = 3, both one hop from D = 4: the two primaries share root_link 0 and protect nothing of each
    other.  third: C = 5 behind S's second link (S - C 2, C - D 1) is taken by both."""
    links = [(0, 1, 1), (1, 0, 0), (2, 1, 1), (1, 2, 0), (3, 1, 1), (1, 3, 0)] + M.both([(2, 4, 1), (3, 4, 1)])
    if not third:
        # slots: 0 S -> LAN | 1 LAN -> S | 2 LAN -> A | 3 LAN -> B
        return M.csr(5, links, net=[1]), 0, 0, ([0, 0, 0, 0, 0, 2], [(2, NO, 0, 0), (3, NO, 0, 0)], [1, 2, 0, 0, 0, 0, 0])
    links += M.both([(0, 5, 2), (5, 4, 1)])
    # slots: 0 S -> LAN | 1 S -> C | 2 LAN -> S | 3 LAN -> A | 4 LAN -> B
    return M.csr(6, links, net=[1]), 0, 0, ([0, 0, 0, 0, 0, 2, 2], [(3, 1, 3, L | N | D), (4, 1, 3, L | N | D)], [1, 2, 2, 2, 2, 0, 1])


def overload(ignore=False):
    """parallel() with C overloaded: C carries no transit traffic and is refused unless the call ignores the bit."""
    links = [(0, 1, 1), (1, 0, 1), (0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 1, 1)] + M.both([(0, 3, 2), (3, 2, 2)])
    g = M.csr(4, links, no_transit=[3])
    if ignore:
        return g, 0, M.IGNORE_OVERLOAD, ([0, 0, 2, 4, 4], [(0, 1, 1, L | D | P), (1, 0, 1, L | D | P), (0, 2, 4, L | N), (1, 2, 4, L | N)], [2, 4, 4, 2, 2, 2, 2])
    return g, 0, 0, ([0, 0, 2, 4, 4], [(0, 1, 1, L | D | P), (1, 0, 1, L | D | P), (0, 1, 2, L | D | P), (1, 0, 2, L | D | P)], [2, 4, 4, 0, 4, 4, 2])


def network_primary():
    """S = 0 reaches the LAN 2 over its own attachment (cost 2) and through A = 1 (1 + 1); run with HSPF_RUN_NET_NEXTHOPS.  Slots: 0 S -> LAN (a network vertex: no
    candidate) | 1 S -> A | 2 LAN -> S | 3 LAN -> A (root_link 0, cost 2).  For D = the LAN, primary 0 is protected by A and protects
    no node; primary 1 is never offered slot 0, although that is a primary too, and gets A across the LAN: the link, not the node."""
    links = [(0, 2, 2), (2, 0, 0), (0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 1, 0)]
    return M.csr(3, links, net=[2]), 0, 0, ([0, 0, 0, 2], [(0, 1, 2, L | D | P), (1, 3, 3, L | D)], [1, 2, 2, 0, 2, 1, 1])


RUN_FLAGS = {"network_primary": 0x01}      # HSPF_RUN_NET_NEXTHOPS: a directly attached network has its own attachment as a primary slot
HAND = {"diamond": diamond, "network_primary": network_primary, "parallel_c": parallel, "parallel": lambda: parallel(False), "lan": lan, "lan_third": lambda: lan(True),
        "overload": overload, "overload_ignored": lambda: overload(True)}


def expected(case):
    """The hand-written arrays of a case as an (ea_ptr, ea_primary, ea_slot, ea_metric, ea_flags, ea_coverage) tuple."""
    ptr, ent, cov = case[3]
    col = lambda i, dt: np.array([e[i] for e in ent], dt)
    return (np.array(ptr, np.uint32), col(0, np.uint32), col(1, np.uint32), col(2, np.uint32), col(3, np.uint8), np.array(cov, np.uint32))


def small_graph(seed):
    """Routers only, symmetric costs from [1, 3], 8 - 20 vertices, connected: tie-heavy, so that ECMP is common."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(8, 21))
    links = [(v, int(rng.integers(0, v)), int(rng.integers(1, 4))) for v in range(1, n)]
    have = {(min(a, b), max(a, b)) for a, b, _ in links}
    for _ in range(n):
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b and (min(a, b), max(a, b)) not in have:
            have.add((min(a, b), max(a, b)))
            links.append((a, b, int(rng.integers(1, 4))))
    return M.csr(n, M.both(links)), int(rng.integers(0, n))


SMALL_SEEDS = list(range(24))
GPU_SEEDS = list(range(7000, 7040))


def random_isis_like(seed):
    """8 - 40 routers on a sparse mesh with tie-heavy, partly asymmetric costs from [0, 3] (zero-cost router links included), up to
    two LANs (pseudonodes after the routers, LAN -> router cost 0), some overloaded routers; the root is a router."""
    r = np.random.default_rng(seed)
    nr = int(r.integers(8, 41))
    n_lan = int(r.integers(0, 3))
    und = {(v, int(r.integers(0, v))) for v in range(1, nr)}
    for _ in range(int(r.integers(nr // 2, nr + nr // 2))):
        a, b = (int(x) for x in r.integers(0, nr, 2))
        if a != b and (a, b) not in und and (b, a) not in und:
            und.add((a, b))
    links = []
    for a, b in sorted(und):
        c1 = int(r.integers(0, 4)) if r.random() < 0.15 else int(r.integers(1, 4))
        c2 = c1 if r.random() < 0.8 else int(r.integers(1, 4))
        links += [(a, b, c1), (b, a, c2)]
    for i in range(n_lan):
        for m in r.choice(nr, size=int(r.integers(2, 5)), replace=False):
            links += [(int(m), nr + i, int(r.integers(1, 4))), (nr + i, int(m), 0)]
    S = int(r.integers(0, nr))
    overloaded = [int(v) for v in range(nr) if r.random() < 0.12 and v != S]
    return M.csr(nr + n_lan, links, net=range(nr, nr + n_lan), no_transit=overloaded), S


def ring_chords(n, K):
    """Root 0 with K neighbours 1 .. K (n >= 1 + K) at cost 1 (odd) and 2 (even), which form a unit-cost ring 1 - 2 - ... - K - 1: an
    even neighbour is reached directly and through both odd ones next to it.  Every further vertex v hangs on the chords v - (v - K)
    and v - (v - K + 1) at cost 1, so ties reach every destination up to the last."""
    links = [(0, k, 2 - k % 2) for k in range(1, K + 1)] + [(k, k % K + 1, 1) for k in range(1, K + 1)]
    links += [(v, v - K, 1) for v in range(K + 1, n)] + [(v, v - K + 1, 1) for v in range(K + 1, n)]
    return M.csr(n, M.both(links)), 0


def star(K):
    """Root 0 with K equal-cost spokes 1 .. K, every spoke one hop from the one far vertex K + 1: popcount(P) of it is K."""
    links = [(0, k, 1) for k in range(1, K + 1)] + [(k, K + 1, 1) for k in range(1, K + 1)]
    return M.csr(K + 2, M.both(links)), 0


def chain(n):
    """A path 0 - 1 - ... - (n - 1): no ECMP anywhere."""
    return M.csr(n, M.both([(v, v + 1, 1 + v % 3) for v in range(n - 1)])), n // 2


def grid(w, h):
    """A unit-cost w x h grid, root in a corner: almost every vertex has both of the root's links as primaries."""
    idx = lambda x, y: y * w + x
    links = [(idx(x, y), idx(x + 1, y), 1) for y in range(h) for x in range(w - 1)] + [(idx(x, y), idx(x, y + 1), 1) for y in range(h - 1) for x in range(w)]
    u, v, c = (np.array(a, np.uint32) for a in zip(*links))
    src, dst, cost = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([c, c])
    order = np.argsort(src, kind="stable")
    rp = np.zeros(w * h + 1, np.uint32)
    rp[1:] = np.cumsum(np.bincount(src, minlength=w * h))
    return (rp, dst[order], cost[order], np.zeros(w * h, np.uint8)), 0
