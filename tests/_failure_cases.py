"""Failure-scenario SPF rows (hspf_run_failures*): the reference construction on the unmodified CPU oracle, and the shared case list.

Reference: one extra vertex n with an empty row; a failed root link `col[row_ptr[S] + j]` is retargeted to n, a failed vertex X has
every link of its row retargeted to n.  The retargeted links fail the two-way check, no position moves, slot numbering is preserved;
columns 0 .. n-1 of the oracle's row are what the engine must deliver bit for bit.

A case is (graph, max_path_metric, roots, failures, run_flags, check): `check(ref, plain)` asserts on the ORACLE's rows that the branch
the case names is taken (ref: the failure rows, plain: the same roots without failures).  `widen` gives the root more than 64 slots;
`Case.at(extra)` is the case with `extra` spokes at its first root (WORDS: 130, 300, 520, 960 spokes -> 3, 5, 9, 16 mask words, the
engine's kernel widths 4, 8, 16, 16), and Ref.extra / Ref.front tell a check how many spokes the root has and where they stand."""
from dataclasses import dataclass, replace
from typing import Callable

import numpy as np

NONE, ROOT_LINK, VERTEX = 0, 1, 2
INF = 0xFFFFFFFF
NO_ROOT = 0xFFFFFFFF
NET, OVL = 1, 2
NET_NEXTHOPS, IGNORE_OVERLOAD = 1, 2
RF_EXACT = np.uint16(2)


def csr(rows, vf=None):
    """rows[v] = [(target, cost), ...] -> (row_ptr, col, metric, vflags)."""
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    col = np.array([t for r in rows for t, _ in r], np.uint32)
    met = np.array([c for r in rows for _, c in r], np.uint32)
    return rp, col, met, np.array(vf if vf is not None else [0] * len(rows), np.uint8)


def both(n, und):
    """Undirected (a, b, cost) -> rows, each link appended to both rows in list order."""
    rows = [[] for _ in range(n)]
    for a, b, c in und:
        rows[a].append((b, c))
        rows[b].append((a, c))
    return rows


WORDS = {130: 3, 300: 5, 520: 9, 960: 16}     # spokes of Case.at() -> mask words needed (the roots of the case list have 1 .. 20 slots of their own)


def widen(rows, vf, S, extra=66, cost=9, front=False):
    """`extra` single-homed routers behind S, their links appended to S's row: S gets more than 64 slots, nothing else moves.
    front: the spokes' links stand BEFORE S's own links instead, whose positions (and slots) move up by `extra`."""
    rows = [list(r) for r in rows]
    vf = list(vf)
    spokes = []
    for _ in range(extra):
        v = len(rows)
        rows.append([(S, cost)])
        spokes.append((v, cost))
        vf.append(0)
    rows[S] = spokes + rows[S] if front else rows[S] + spokes
    return rows, vf


def retarget(graph, root, kind, arg):
    rp, col, met, vf = graph
    n = len(vf)
    rp2 = np.append(rp, rp[-1]).astype(np.uint32)
    col2 = col.copy()
    if kind == ROOT_LINK:
        col2[int(rp[root]) + int(arg)] = n
    elif kind == VERTEX:
        col2[int(rp[arg]):int(rp[arg + 1])] = n
    return rp2, col2, met, np.append(vf, 0).astype(np.uint8)


def slot_bases(graph, root):
    """{H vertex: slot base} of a root (include/holo_spf_hip.h "first-hop slots"), restated: H = [root] ++ the network vertices reached
    through network vertices only over two-way links, in row order."""
    rp, col, _, vf = graph
    base, total, q = {root: 0}, int(rp[root + 1] - rp[root]), [root]
    for p in q:
        for k in range(int(rp[p]), int(rp[p + 1])):
            t = int(col[k])
            if t in base or not (vf[t] & 1) or p not in col[rp[t]:rp[t + 1]]:
                continue
            base[t] = total
            total += int(rp[t + 1] - rp[t])
            q.append(t)
    return base, total


def renumber(mask, W, old, new, graph):
    """Mask words in the numbering `old` ({vertex: base}) rewritten in the numbering `new`: slot (p, j) keeps its identity."""
    rp = graph[0]
    bits = np.zeros(mask.shape[0], object)
    for v in range(mask.shape[0]):
        bits[v] = sum(int(mask[v, w]) << (64 * w) for w in range(mask.shape[1]))
    out = np.zeros((mask.shape[0], W), np.uint64)
    for v in range(mask.shape[0]):
        x, y = bits[v], 0
        if x:
            for p, b in old.items():
                ln = int(rp[p + 1] - rp[p])
                y |= ((x >> b) & ((1 << ln) - 1)) << new[p]
        for w in range(W):
            out[v, w] = (y >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


@dataclass
class Ref:
    dist: np.ndarray
    hops: np.ndarray
    flags: np.ndarray
    mask: np.ndarray
    pop_rank: np.ndarray
    extra: int = 0               # spokes at the case's first root (run_check sets both)
    front: bool = False          # ... standing before the root's own links


def reference(graph, maxp, roots, fails, run_flags=0, W=None) -> Ref:
    """The oracle's rows, one plain oracle run per row on the retargeted CSR."""
    from oracle import graph_oracle as go
    rp, col, met, vf = graph
    n, R = len(vf), len(roots)
    if W is None:
        W = go.mask_words(rp, col, met, vf, np.asarray(roots, np.uint32))
    out = Ref(np.full((R, n), INF, np.uint32), np.zeros((R, n), np.uint16), np.zeros((R, n), np.uint16), np.zeros((R, n, W), np.uint64),
              np.full((R, n), INF, np.uint32))
    for r, (root, (kind, arg)) in enumerate(zip(roots, fails)):
        if int(root) == NO_ROOT:
            continue
        g2 = retarget(graph, int(root), int(kind), int(arg))
        o = go.run(g2[0], g2[1], g2[2], g2[3], maxp, np.array([root], np.uint32), run_flags, go.MAP, mask_words_=W)
        assert o.flags[0, n] == 0                                          # the extra vertex is never reached
        m = o.mask[0, :n]
        # A retargeted link into a network vertex of the root's slot table H (the root's own LAN link failed, or the LAN excluded)
        # takes that vertex out of H ON THE RETARGETED GRAPH, and the bases of the networks behind it move down.  The call keeps
        # the numbering of the intact graph ("no slot moves"), so the oracle's bits are carried over slot by slot: (H vertex,
        # position) is the identity of a slot in both numberings.  Where H is unchanged this is the identity map.
        b1, _ = slot_bases(graph, int(root))
        b2, _ = slot_bases(g2, int(root))
        if b1 != b2:
            assert set(b2) <= set(b1)
            m = renumber(m, W, b2, b1, graph)
        out.dist[r], out.hops[r], out.flags[r], out.mask[r], out.pop_rank[r] = o.dist[0, :n], o.hops[0, :n], o.flags[0, :n], m, o.pop_rank[0, :n]
    return out


def same(res, ref: Ref):
    """Bit for bit: dist, hops, every mask word, and every flag bit but HSPF_RF_EXACT (the oracle does not set it: it only says that the
    sequential kernel wrote the row)."""
    assert np.array_equal(res.dist, ref.dist), ("dist", np.argwhere(res.dist != ref.dist)[:4].tolist())
    assert np.array_equal(res.hops, ref.hops), ("hops", np.argwhere(res.hops != ref.hops)[:4].tolist())
    assert np.array_equal(res.flags & ~RF_EXACT, ref.flags), ("flags", np.argwhere((res.flags & ~RF_EXACT) != ref.flags)[:4].tolist())
    assert np.array_equal(res.first_hop_mask, ref.mask), ("mask", np.argwhere(res.first_hop_mask != ref.mask)[:4].tolist())


@dataclass
class Case:
    rows: list
    vf: list
    maxp: int
    roots: list
    fails: list
    flags: int
    check: Callable
    exact: bool = False          # the rows must come from the sequential kernel (stats n_exact_roots > 0)
    spoke_cost: int = 9          # cost of the widening spokes (1 on hop-count-like graphs, which they must not leave)
    front: bool = False          # at(): the spokes stand before the root's own links
    extra: int = 0               # spokes already added by at()
    hopcount: bool = False       # the graph is hop-count-like, spokes included
    words: dict = None           # {spokes: mask words needed} of a case that does not start at one word (default: WORDS)

    def graph(self, wide=False):
        rows, vf = (widen(self.rows, self.vf, self.roots[0], cost=self.spoke_cost) if wide else (self.rows, self.vf))
        return csr(rows, vf)

    def at(self, extra):
        """The case with `extra` spokes at its first root.  With `front` they come first in the root's row, and the HSPF_FAIL_ROOT_LINK
        positions of that root move up with its own links."""
        assert self.extra == 0
        S = self.roots[0]
        rows, vf = widen(self.rows, self.vf, S, extra, self.spoke_cost, self.front)
        fails = [(k, a + extra) if (self.front and k == ROOT_LINK and r == S) else (k, a) for r, (k, a) in zip(self.roots, self.fails)]
        return replace(self, rows=rows, vf=vf, fails=fails, extra=extra)


def bit(ref, r, v, slot):
    return bool(int(ref.mask[r, v, slot // 64]) >> (slot % 64) & 1)


def _differs(ref, plain, r=0):
    return not (np.array_equal(ref.dist[r], plain.dist[r]) and np.array_equal(ref.mask[r], plain.mask[r]))


def _cases():
    C = {}
    # 1: unit ring of six, link 0 -> 1 (position 0) fails: the detour is the whole ring
    ring = both(6, [(v, (v + 1) % 6, 1) for v in range(6)])
    C["ring"] = Case(ring, [0] * 6, INF, [0], [(ROOT_LINK, 0)], 0,
                     lambda f, p: (p.dist[0, 1] == 1 and f.dist[0, 1] == 5 and not bit(f, 0, 1, 0) and bit(f, 0, 1, 1)) or _fail())
    # 2: two parallel links S - E, equal and unequal cost, each failed in turn
    for name, c0, c1 in (("parallel_equal", 1, 1), ("parallel_unequal", 1, 3)):
        rows = [[(1, c0), (1, c1)], [(0, c0), (0, c1), (2, 1)], [(1, 1)]]

        def chk(f, p, c0=c0, c1=c1):
            assert bit(p, 0, 1, 0) and (bit(p, 0, 1, 1) == (c0 == c1))           # the failed link was on the plain SPT (row 0)
            assert f.dist[0, 1] == c1 and not bit(f, 0, 1, 0) and bit(f, 0, 1, 1)   # link 0 failed: link 1 carries, its own bit set
            assert f.dist[1, 1] == c0 and bit(f, 1, 1, 0) and not bit(f, 1, 1, 1)   # link 1 failed: link 0 carries
            assert f.dist[0, 2] == c1 + 1
        C[name] = Case(rows, [0] * 3, INF, [0, 0], [(ROOT_LINK, 0), (ROOT_LINK, 1)], 0, chk)
    # 3: the failed link did not survive the two-way check (2 does not list 0): the row equals the plain row
    rows = [[(1, 1), (2, 1)], [(0, 1), (2, 1)], [(1, 1)]]
    C["one_way_link"] = Case(rows, [0] * 3, INF, [0], [(ROOT_LINK, 1)], 0,
                             lambda f, p: (not _differs(f, p) and p.dist[0, 2] == 2) or _fail())
    # 4: a leaf (router 1, single-homed) behind the failed link; 5 / 6: a leaf behind the excluded vertex, the excluded vertex a leaf
    rows = both(4, [(0, 1, 1), (0, 2, 1), (2, 3, 1), (3, 0, 1)])
    C["leaf_behind_link"] = Case(rows, [0] * 4, INF, [0], [(ROOT_LINK, 0)], 0,
                                 lambda f, p: (p.dist[0, 1] == 1 and f.dist[0, 1] == INF and f.flags[0, 1] == 0 and f.dist[0, 3] == 1) or _fail())
    rows = both(4, [(0, 1, 1), (1, 2, 1), (0, 3, 1), (3, 1, 1)])
    C["leaf_behind_vertex"] = Case(rows, [0] * 4, INF, [0], [(VERTEX, 1)], 0,
                                   lambda f, p: (p.dist[0, 2] == 2 and f.dist[0, 2] == INF and f.dist[0, 1] == INF and f.dist[0, 3] == 1) or _fail())
    C["leaf_excluded"] = Case(rows, [0] * 4, INF, [0], [(VERTEX, 2)], 0,
                              lambda f, p: (f.dist[0, 2] == INF and f.dist[0, 1] == 1 and (f.dist[0] != p.dist[0]).sum() == 1) or _fail())
    # 7: S = 0 on a LAN (pseudonode 3) with routers 1 and 2, and a point-to-point link 0 - 1 at 50: the S -> pseudonode link fails
    lan = [[(3, 10), (1, 50)], [(3, 10), (0, 50)], [(3, 10)], [(0, 0), (1, 0), (2, 0)]]
    C["lan_link"] = Case(lan, [0, 0, 0, NET], INF, [0], [(ROOT_LINK, 0)], 0,
                         lambda f, p: (p.dist[0, 2] == 10 and f.dist[0, 1] == 50 and f.dist[0, 3] == 60 and f.dist[0, 2] == 60 and not bit(f, 0, 2, 0)) or _fail())
    # 8: the pseudonode excluded (a LAN failure), with HSPF_RUN_NET_NEXTHOPS and without
    for name, fl in (("lan_excluded_net_nexthops", NET_NEXTHOPS), ("lan_excluded", 0)):
        C[name] = Case(lan, [0, 0, 0, NET], INF, [0], [(VERTEX, 3)], fl,
                       lambda f, p: (p.dist[0, 2] == 10 and f.dist[0, 3] == INF and f.dist[0, 2] == INF and f.dist[0, 1] == 50) or _fail())
    # 9: the only detour runs through an overloaded router (2): unreachable unless HSPF_RUN_IGNORE_OVERLOAD
    rows = both(3, [(0, 1, 1), (0, 2, 1), (2, 1, 1)])
    C["overloaded_detour"] = Case(rows, [0, 0, OVL], INF, [0], [(ROOT_LINK, 0)], 0,
                                  lambda f, p: (p.dist[0, 1] == 1 and f.dist[0, 1] == INF and f.dist[0, 2] == 1) or _fail())
    C["overloaded_detour_ignored"] = Case(rows, [0, 0, OVL], INF, [0], [(ROOT_LINK, 0)], IGNORE_OVERLOAD,
                                          lambda f, p: (f.dist[0, 1] == 2 and bit(f, 0, 1, 1) and not bit(f, 0, 1, 0)) or _fail())
    # 10: a cut vertex excluded: the far side is unreachable
    rows = both(5, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 4, 1)])
    C["cut_vertex"] = Case(rows, [0] * 5, INF, [0], [(VERTEX, 1)], 0,
                           lambda f, p: (p.dist[0, 3] == 3 and list(f.dist[0, :5]) == [0, INF, INF, INF, 1]) or _fail())
    # 11: max_path_metric 1023 with a detour of 1024 (and of 1023, which stays)
    for name, a, want in (("maxpath_1024", 512, INF), ("maxpath_1023", 511, 1023)):
        rows = both(3, [(0, 1, 1), (0, 2, a), (2, 1, 512)])
        C[name] = Case(rows, [0] * 3, 1023, [0], [(ROOT_LINK, 0)], 0,
                       lambda f, p, want=want: (p.dist[0, 1] == 1 and f.dist[0, 1] == want and (f.flags[0, 1] == 1) == (want != INF)) or _fail())
    # 12: max_path_metric 0xFFFFFFFF and a detour whose sum saturates u32: the sequential kernel
    rows = both(3, [(0, 1, 1), (0, 2, 0xFFFFFFF0), (2, 1, 0x20)])
    C["saturating_detour"] = Case(rows, [0] * 3, INF, [0], [(ROOT_LINK, 0)], 0,
                                  lambda f, p: (p.dist[0, 1] == 1 and f.dist[0, 1] == INF and f.flags[0, 1] == 1 and f.hops[0, 1] == 2) or _fail(), exact=True)
    # 13: a zero-cost plateau 3 <-> 1 whose way in is through the HIGHER-numbered 3: the pop order is dynamic.  Row 0 fails 0 -> 2 (off
    # the plateau, where it was one of two equal-cost ways to 2: still dynamic), row 1 fails 0 -> 3 (on it: 1 is now reached first, from 2, and the order is static again)
    rows = both(4, [(0, 3, 1), (3, 1, 0), (1, 2, 1), (0, 2, 2)])

    def chk13(f, p):
        assert p.pop_rank[0, 3] < p.pop_rank[0, 1] and p.dist[0, 1] == p.dist[0, 3] == 1              # dynamic: 3 pops before 1 at equal distance
        assert f.pop_rank[0, 3] < f.pop_rank[0, 1] and f.dist[0, 2] == 2 and p.dist[0, 2] == 2 and _differs(f, p, 0)
        assert f.dist[1, 1] == 3 and f.dist[1, 3] == 3 and f.pop_rank[1, 1] < f.pop_rank[1, 3] and not bit(f, 1, 3, 0)
    C["zero_cost_plateau"] = Case(rows, [0] * 4, INF, [0, 0], [(ROOT_LINK, 1), (ROOT_LINK, 0)], 0, chk13, exact=True)
    # 14: a giant row (a pseudonode with 300 routers, more than 256 in-links) next to the failure: S = 301 hangs on routers 1 (at 5)
    # and 2 (at 30) of the LAN; its link to 1 fails, then router 1 (a source of the giant row) is excluded, then the LAN itself
    n_r = 300
    rows = [[(r, 0) for r in range(1, n_r + 1)]] + [[(0, 10)] for _ in range(n_r)] + [[(1, 5), (2, 30)]]
    rows[1].append((301, 5))
    rows[2].append((301, 30))

    def chk14(f, p):
        assert p.dist[0, 0] == 15 and p.dist[0, 300] == 15 and bit(p, 0, 300, 0)
        assert f.dist[0, 2] == 30 and f.dist[0, 0] == 40 and f.dist[0, 1] == 40 and f.dist[0, 300] == 40 and bit(f, 0, 300, 1) and not bit(f, 0, 300, 0)
        assert f.dist[1, 1] == INF and f.dist[1, 0] == 40 and f.dist[1, 300] == 40
        assert f.dist[2, 0] == INF and f.dist[2, 1] == 5 and f.dist[2, 2] == 30 and (f.dist[2, :302] != INF).sum() == 3
    C["giant_row"] = Case(rows, [NET] + [0] * (n_r + 1), INF, [301, 301, 301], [(ROOT_LINK, 0), (VERTEX, 1), (VERTEX, 0)], 0, chk14)
    # 15: the root on two LANs (3 with router 1, 4 with router 2): its link to the first fails, then that LAN is excluded.  The second
    # LAN's slots come behind the first's in the root's slot table and must keep their numbers: router 2 is reached through the LAN's
    # link to it, slot (own links) + 2 + 1
    rows = [[(3, 10), (4, 10)], [(3, 10)], [(4, 10)], [(0, 0), (1, 0)], [(0, 0), (2, 0)]]

    def chk15(f, p):
        own = 2 + f.extra
        for r in (0, 1):
            assert p.dist[r, 1] == 10 and f.dist[r, 1] == INF and f.dist[r, 2] == 10 and f.dist[r, 4] == 10
            assert bit(f, r, 2, own + 3) and not bit(f, r, 2, own + 1) and bit(p, r, 2, own + 3) and bit(p, r, 1, own + 1)
        assert f.dist[0, 3] == INF and f.dist[1, 3] == INF
    C["two_lans"] = Case(rows, [0, 0, 0, NET, NET], INF, [0, 0], [(ROOT_LINK, 0), (VERTEX, 3)], 0, chk15)
    # 16: the ring of case 1 with the spokes of at() standing FIRST in the root's row: the failed link 0 -> 1 and the detour 0 -> 5 then
    # have the two highest slots of the root, both in the top mask word (960 spokes: slots 960 and 961, word 15)
    def chk16(f, p):
        fs = f.extra if f.front else 0
        ds = fs + 1
        if f.front:
            assert f.extra >= 64 and fs // 64 == ds // 64 == f.mask.shape[2] - 1
        assert p.dist[0, 1] == 1 and bit(p, 0, 1, fs) and f.dist[0, 1] == 5
        assert any(bit(f, 0, v, ds) for v in range(1, 6)) and not any(bit(f, 0, v, fs) for v in range(f.dist.shape[1]))
    C["high_slot_detour"] = Case(ring, [0] * 6, INF, [0], [(ROOT_LINK, 0)], 0, chk16, front=True)
    # 17: the giant row of case 14 with the failures far down it: S = 301 hangs on routers 130 (at 5) and 290 (at 30), whose links into
    # the pseudonode stand at in-row positions 129 and 289 (the third and the fifth 64-link chunk).  (Router 302 belongs to case 20.)
    g17 = _giant_far()
    C["giant_row_far"] = Case(g17[0], g17[1], INF, [301, 301, 301], [(ROOT_LINK, 0), (VERTEX, 130), (VERTEX, 0)], 0, lambda f, p: _chk_far(f, p, 0))
    # 18: a root's failed link far down a ROUTER's in-row (no pseudonode: the root keeps two slots).  Hub 0 with routers 1 .. 70 at 5;
    # S = 70 also reaches the hub through 71 (2 + 3): with S's own link to the hub failed (position 1 of its row, position 69 of the
    # hub's in-row, the second chunk) the hub is still 5 away and the failed link looks tight; the link 64 places before it in the
    # in-row (router 6's) has position 0 in ITS row
    rows = [[(r, 5) for r in range(1, 71)] + [(71, 3)]] + [[(0, 5)] for _ in range(70)] + [[(70, 2), (0, 3)]]
    rows[70] = [(71, 2), (0, 5)]

    def chk18(f, p):
        assert p.dist[0, 0] == 5 and bit(p, 0, 0, 0) and bit(p, 0, 0, 1)
        assert f.dist[0, 0] == 5 and bit(f, 0, 0, 0) and not bit(f, 0, 0, 1) and f.dist[0, 1] == 10 and not bit(f, 0, 1, 1)
    C["hub_far_link"] = Case(rows, [0] * 72, INF, [70], [(ROOT_LINK, 1)], 0, chk18)
    assert in_row(csr(rows), 0)[69] == (70, 1) and in_row(csr(rows), 0)[5] == (6, 0)
    # 19: a hop-count-like graph (LANs 0, 1, 2 numbered below their routers 3 .. 8; router -> LAN 0, LAN -> router 1).  S = 3 and R = 4
    # share the LANs 0 and 1, router 6 is on LAN 0 only; 5 and 8 (LANs 1 and 2) are both one hop away, so both their links are tight
    # zero-cost in-links of LAN 2 from higher-numbered sources, and the first, 5's, is its only parent (7 is behind LAN 2).
    # Rows: nothing failed; S's link into LAN 0 (its parent becomes R's link); R excluded; LAN 0 excluded; 5 excluded (8's link takes over)
    rows = [[(3, 1), (4, 1), (6, 1)], [(3, 1), (4, 1), (5, 1), (8, 1)], [(5, 1), (8, 1), (7, 1)],
            [(0, 0), (1, 0)], [(0, 0), (1, 0)], [(1, 0), (2, 0)], [(0, 0)], [(2, 0)], [(1, 0), (2, 0)]]

    def chk19(f, p):
        a, b, c, d, e = range(5)
        own = 2 + f.extra
        s5, s8 = own + 3 + 2, own + 3 + 3                                 # slots of LAN 1's links to 5 and to 8 (LAN 0's three come first)
        assert f.dist[a].tolist()[:9] == [0, 0, 1, 0, 1, 1, 1, 2, 1] and np.array_equal(f.dist[a], p.dist[a]) and np.array_equal(f.mask[a], p.mask[a])
        assert f.dist[b, 0] == 1 and f.flags[b, 0] == 1 and f.hops[a, 0] == 0 and f.hops[b, 0] == 1 and f.dist[b, 6] == 2
        assert bit(f, b, 6, own + 3 + 1) and not bit(f, b, 6, own + 2) and bit(f, a, 6, own + 2)   # 6: through LAN 1's link to R, not LAN 0's to 6
        assert f.dist[c, 4] == INF and f.dist[c, 0] == 0 and f.dist[d, 0] == INF and f.dist[d, 6] == INF and f.dist[d, 4] == 1
        assert bit(f, a, 7, s5) and not bit(f, a, 7, s8) and bit(f, a, 2, s5) and not bit(f, a, 2, s8)   # LAN 2 and 7: the first parent only
        assert f.dist[e, 5] == INF and f.dist[e, 2] == 1 and f.dist[e, 7] == 2 and bit(f, e, 7, s8) and not bit(f, e, 7, s5)
    C["hopcount_lan_first_parent"] = Case(rows, [NET] * 3 + [0] * 6, INF, [3] * 5, [(NONE, 0), (ROOT_LINK, 0), (VERTEX, 4), (VERTEX, 0), (VERTEX, 5)], 0,
                                          chk19, spoke_cost=1, hopcount=True)
    return C


def in_row(graph, t):
    """[(source, position in the source's row)] of the links into t in the engine's in-row order: cost descending, source ascending,
    position ascending (two-way links only)."""
    rp, col, met, _ = graph
    out = []
    for u in range(len(rp) - 1):
        for k in range(int(rp[u]), int(rp[u + 1])):
            if int(col[k]) == t and u in col[rp[t]:rp[t + 1]]:
                out.append((-int(met[k]), u, k - int(rp[u])))
    return [(u, j) for _, u, j in sorted(out)]


def _giant_far():
    n_r = 300
    rows = [[(r, 0) for r in range(1, n_r + 1)]] + [[(0, 10)] for _ in range(n_r)] + [[(130, 5), (290, 30)]]
    rows[130].append((301, 5))
    rows[290].append((301, 30))
    # router 302 behind 280 (at 3) and on the LAN (at 7): 280 reaches the LAN at 10 both ways
    rows.append([(280, 3), (0, 7)])
    rows[280] = [(302, 3), (0, 10)]
    rows[0].append((302, 0))
    g = csr(rows)
    pos = in_row(g, 0)
    assert pos[129] == (130, 0) and pos[289] == (290, 0) and pos[279] == (280, 1) and pos[279 - 256] == (24, 0) and len(pos) == 301
    return rows, [NET] + [0] * 302


def _chk_far(f, p, r0):
    a, b, c = r0, r0 + 1, r0 + 2
    assert p.dist[a, 0] == 15 and p.dist[a, 300] == 15 and bit(p, a, 300, 0)
    assert f.dist[a, 290] == 30 and f.dist[a, 0] == 40 and f.dist[a, 130] == 40 and f.dist[a, 300] == 40 and bit(f, a, 300, 1) and not bit(f, a, 300, 0)
    assert f.dist[b, 130] == INF and f.dist[b, 0] == 40 and f.dist[b, 300] == 40
    assert f.dist[c, 0] == INF and f.dist[c, 130] == 5 and f.dist[c, 290] == 30 and (f.dist[c, :303] != INF).sum() == 3


def _wide_cases():
    """Cases whose first root needs more than one mask word before any widening: not part of CASES, whose every case runs at one word."""
    # 20: case 17's graph with a root that is itself a router of the 301-router LAN: M = 280, in-row position 279 (the fifth chunk), its
    # link into the LAN at position 1 of its row while the in-link 256 places earlier (router 24's) has position 0.  M reaches the
    # LAN at 10 directly and through 302 (3 + 7): with its own link failed the LAN keeps its distance, the failed link looks tight,
    # and everything behind the LAN moves from the LAN's own slots to slot 0 (M -> 302).  Then 302 excluded, and case 17's three rows.
    rows, vf = _giant_far()

    def chk20(f, p):
        own = 2 + f.extra
        assert p.dist[0, 0] == 10 and p.hops[0, 0] == 0 and bit(p, 0, 1, own + 0) and not bit(p, 0, 1, 0)
        assert f.dist[0, 0] == 10 and f.hops[0, 0] == 1 and bit(f, 0, 1, 0) and not bit(f, 0, 1, own + 0) and f.dist[0, 1] == 10
        assert not any(bit(f, 0, v, 1) for v in range(f.dist.shape[1]))
        assert f.dist[1, 302] == INF and f.dist[1, 0] == 10 and f.hops[1, 0] == 0
        _chk_far(f, p, 2)
    fails = [(ROOT_LINK, 1), (VERTEX, 302), (ROOT_LINK, 0), (VERTEX, 130), (VERTEX, 0)]
    return {"giant_row_member": Case(rows, vf, INF, [280, 280, 301, 301, 301], fails, 0, chk20, words={0: 5, 130: 7, 300: 10, 520: 13})}


def _fail():
    raise AssertionError("the case does not take the branch it names")


CASES = _cases()
WIDE_CASES = _wide_cases()


def hopcount_random(seed) -> Case:
    """A seeded hop-count-like graph of 20 to 60 vertices — LANs first, so that each is numbered below its routers; every router on one
    to three of them, on odd seeds with some point-to-point links at 1 — with every link and every neighbour (mostly LANs) of three
    router roots.  Every root has at most 40 slots: 280 spokes at the first bring the run to five mask words."""
    r = np.random.default_rng(7700 + seed)
    n = int(r.integers(20, 61))
    k = max(3, n // 4)
    rows = [[] for _ in range(n)]
    for v in range(k, n):
        for l in r.choice(k, int(r.integers(1, 4)), replace=False).tolist():
            rows[v].append((l, 0))
            rows[l].append((v, 1))
    if seed % 2:
        for _ in range(n // 4):
            a, b = (int(x) for x in r.integers(k, n, 2))
            if a != b and all(t != b for t, _ in rows[a]):
                rows[a].append((b, 1))
                rows[b].append((a, 1))
    vf = [NET] * k + [0] * (n - k)
    graph = csr(rows, vf)
    roots, fails = [], []
    for S in r.choice(np.arange(k, n), 3, replace=False).tolist():
        sc = all_scenarios(graph, S)
        roots += [S] * len(sc)
        fails += sc
    return Case(rows, vf, INF, roots, fails, 0, lambda f, p: None, spoke_cost=1, hopcount=True, words={0: 1, 280: 5})


def is_hopcount_like(graph):
    """The engine's hop-count shape, restated on the CSR: every link that survives the two-way check costs 0 into a network — and
    then comes from a higher-numbered router — and 1 into a router; some network has such a link."""
    rp, col, met, vf = graph
    net_in = False
    for u in range(len(vf)):
        for k in range(int(rp[u]), int(rp[u + 1])):
            t = int(col[k])
            if u not in col[rp[t]:rp[t + 1]]:
                continue
            if vf[t] & NET:
                if met[k] != 0 or (vf[u] & NET) or u <= t:
                    return False
                net_in = True
            elif met[k] != 1:
                return False
    return net_in


def run_check(case: Case, wide: bool = False, extra=None):
    """The oracle's rows of a case, after asserting that its branch is taken; returns (graph, ref).  extra: the case at(extra), whose
    roots and failures the caller takes from at(extra) too; the oracle must need WORDS[extra] mask words."""
    from oracle import graph_oracle as go
    assert not (wide and extra is not None)
    if extra is not None:
        case = case.at(extra)
    g = case.graph(wide)
    ref = reference(g, case.maxp, case.roots, case.fails, case.flags)
    plain = reference(g, case.maxp, case.roots, [(NONE, 0)] * len(case.roots), case.flags)
    need = go.mask_words(g[0], g[1], g[2], g[3], np.asarray(case.roots, np.uint32))
    want = (2 if wide else (case.words or {0: 1})[0]) if extra is None else (case.words or WORDS)[extra]
    assert need == ref.mask.shape[2] == want, (need, ref.mask.shape, want)
    assert is_hopcount_like(g) == case.hopcount
    for x in (ref, plain):
        x.extra, x.front = (66 if wide else 0) if extra is None else extra, extra is not None and case.front
    case.check(ref, plain)
    return g, ref


def all_scenarios(graph, S):
    """Every link of S failed, then every distinct neighbour excluded."""
    rp, col, _, _ = graph
    links = [(ROOT_LINK, j) for j in range(int(rp[S + 1] - rp[S]))]
    nbrs = [(VERTEX, int(x)) for x in dict.fromkeys(col[rp[S]:rp[S + 1]].tolist()) if int(x) != S]
    return links + nbrs


def batch130(seed=5):
    """130 rows = three batches, the last one ragged: root S with every link failed and every neighbour excluded, interleaved with
    HSPF_FAIL_NONE rows of S and of other roots and with HSPF_NO_ROOT padding."""
    from holo_amd import synth
    g = synth.random_lsdb(120, 10, 3.0, seed, metric_hi=9)
    graph = (g.row_ptr, g.col, g.metric, g.vflags)
    deg = np.diff(g.row_ptr.astype(np.int64))
    S = int(np.argmax(np.where(g.vflags == 0, deg, -1)))
    sc = all_scenarios(graph, S)
    assert len(sc) <= 44                                                   # rows 0, 3, 6 .. 129 walk the list once: links first, then neighbours
    roots, fails = [], []
    for i in range(130):
        if i % 3 == 0:
            roots.append(S); fails.append(sc[(i // 3) % len(sc)])
        elif i % 3 == 1:
            roots.append(S if i % 2 else (i * 7) % g.n); fails.append((NONE, 99))
        else:
            roots.append(NO_ROOT if i % 4 == 2 else (i * 11) % g.n); fails.append((VERTEX, 5) if i % 4 == 2 else (NONE, 0))
    return graph, int(g.max_path_metric), S, np.array(roots, np.uint32), fails


def write_case_file(path, graph, maxp, roots, fails, flags, ref: Ref):
    rp, col, met, vf = graph
    parts = [[len(vf), len(col), maxp, flags], rp, col, met, vf, [len(roots)], roots, [k for k, _ in fails], [a for _, a in fails],
             [ref.mask.shape[2]], ref.dist.ravel(), ref.hops.ravel(), ref.flags.ravel(), ref.mask.ravel()]
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")


def driver_files(tmp_path, names=("ring", "parallel_unequal", "lan_link", "lan_excluded_net_nexthops", "overloaded_detour", "maxpath_1024", "zero_cost_plateau")):
    files = []
    for name in names:
        for wide in (False, True):
            c = CASES[name]
            g, ref = run_check(c, wide)
            p = tmp_path / f"failures_{name}_{int(wide)}.txt"
            write_case_file(p, g, c.maxp, c.roots, c.fails, c.flags, ref)
            files.append(str(p))
    return files


EXTRAS = sorted(WORDS)
HOPCOUNT_SEEDS = range(20)


def wide_runs():
    """(id, base case, spokes or None) of everything beyond the two legacy widths: every case of CASES at the four widths of WORDS,
    the cases of WIDE_CASES as they are and at the widths that keep them within 16 words, the seeded hop-count-like graphs at one
    word and at five."""
    runs = [(f"{name}-{e}", CASES[name], e) for name in sorted(CASES) for e in EXTRAS]
    runs += [(f"{name}-{e}", c, e or None) for name, c in sorted(WIDE_CASES.items()) for e in sorted(c.words)]
    runs += [(f"hopcount_random{seed}-{e}", hopcount_random(seed), e or None) for seed in HOPCOUNT_SEEDS for e in (0, 280)]
    return runs


def driver_files_wide(tmp_path):
    files = []
    for rid, c, e in wide_runs():
        g, ref = run_check(c, extra=e)
        cw = c.at(e) if e is not None else c
        p = tmp_path / f"failures_{rid}.txt"
        write_case_file(p, g, cw.maxp, cw.roots, cw.fails, cw.flags, ref)
        files.append(str(p))
    return files


def protocol_graph(seed):
    """Even seeds: a random IS-IS instance of tests/_random_isis.py (every fourth with zero metrics), its first non-empty level as the
    standard topology; odd seeds: the first area of a random OSPFv2 instance of tests/_random_ospf.py.  Returns (CSR, max-path, flags)."""
    if seed % 2 == 0:
        from _random_isis import make
        from holo_amd import isis as HI
        inst = HI.Instance.from_vector(make(3000 + seed, zero=(seed % 8 == 6)))
        for level in inst.config.levels():
            g = HI.LevelGraph(inst, level, 0, False)
            if g.n:
                return (g.row_ptr, g.col, g.metric, g.vflags), int(g.max_path_metric), int(g.run_flags)
        raise AssertionError("an instance without a level")
    from _random_ospf import make
    from holo_amd import ospf as HO
    g = HO.AreaGraph(HO.Area.from_vector(make(3000 + seed, zero=(seed % 8 == 7))["areas"][0]))
    return (g.row_ptr, g.col, g.metric, g.vflags), HO.MAX_PATH_METRIC_OSPF, NET_NEXTHOPS


def drop_last_link(G, graph):
    """One structural hspf_graph_patch: the first router with two or more links loses its last one.  Returns the spliced CSR."""
    from holo_amd.engine import splice_rows
    rp, col, met, vf = graph
    deg = np.diff(rp.astype(np.int64))
    cand = np.flatnonzero(((vf & 1) == 0) & (deg >= 2))
    if len(cand) == 0:
        return graph, False
    u = int(cand[0])
    a, b = int(rp[u]), int(rp[u + 1]) - 1
    G.patch([u], [(col[a:b], met[a:b])], [int(vf[u])])
    return splice_rows(rp, col, met, vf, [u], [col[a:b]], [met[a:b]], [int(vf[u])]), True
