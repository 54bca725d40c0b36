"""k_fused_lean fetches the link records of a wave's four rows with one load per array (lane 16 i + j = entry j of row i; rows past
the end of the graph read the pad row n, lane by lane).  The lean sweep is forced on small graphs (HSPF_SINGLE_MAX_N=0,
HSPF_XCD_MAX_ROOTS=0, HSPF_LV_MAX_ROOTS=0) under four plans, so that the stamped (0), dense (1), all-due (2) and HEAD instantiations
all run; every table of every run equals the CPU oracle (HEAP) bit for bit.  The switches are read at hspf_init: one fresh child
process per plan runs all the cases and reports them on one JSON line; the tests below read that line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SWEEPS = {"HSPF_SINGLE_MAX_N": "0", "HSPF_XCD_MAX_ROOTS": "0", "HSPF_LV_MAX_ROOTS": "0"}
PLANS = {
    "default": {},
    "stamped": {"HSPF_VARIANT": str(1 << 19)},                       # stamped sweeps only: mode 0
    "nohead": {"HSPF_LEAN_HEAD": "0", "HSPF_DENSE_PASSES": "1"},     # the dense stretch first, one pass per launch
    "dense16": {"HSPF_DENSE_PASSES": "16"},
}
SIZES = (5, 17, 18, 19, 64, 1021, 1022, 1023)        # the last wave's group of four rows ends 1, 2 and 3 rows short, or full
ROOT_COUNTS = (1, 63, 64, 65)                        # 65: two batches, the second slab's pad row
CASES = ([f"n{n}" for n in SIZES] + [f"degrees-roots{r}" for r in ROOT_COUNTS] +
         ["degrees33", "zero-cost", "patch-cost", "patch-structural"])
INF = 0xFFFFFFFF


def _csr(n, links):
    """{(u, v): cost} -> CSR arrays; row order = insertion order."""
    src = np.array([u for u, _ in links], np.int64)
    order = np.argsort(src, kind="stable")
    col = np.array([v for _, v in links], np.uint32)[order]
    met = np.array(list(links.values()), np.uint32)[order]
    row_ptr = np.zeros(n + 1, np.uint32)
    row_ptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return row_ptr, col, met


def _two_way(links, rng, u, v):
    if u != v and (u, v) not in links:
        links[(u, v)] = int(rng.integers(1, 10))
        links[(v, u)] = int(rng.integers(1, 10))


def _ring_with_chords(n, seed):
    """Routers only: a ring and one random chord per vertex, every link two-way with its own costs (a few hops across)."""
    rng = np.random.default_rng(seed)
    links = {}
    for v in range(n):
        _two_way(links, rng, v, (v + 1) % n)
    for v in range(n):
        _two_way(links, rng, v, int(rng.integers(n)))
    return links


def _degree_graph(big):
    """In-degrees 0, 1, 2, 15, 16, 17 and `big`: both edges of the 16-entry record form, rows of the general routine, rows of more
    than 16 out-links (their wake-ups are walked), with and without an in-degree of at most 16."""
    rng = np.random.default_rng(77)
    n, ring = 104, 100
    links = {}
    for v in range(ring):
        _two_way(links, rng, v, (v + 1) % ring)
    hubs = {20: 15, 40: 16, 60: 17, 80: big}
    for h, deg in hubs.items():
        t = h + 3
        while sum(1 for (u, _) in links if u == h) < deg:
            if t % ring not in hubs:
                _two_way(links, rng, h, t % ring)
            t += 2
    links[(100, 0)] = 3                               # in-degree 0 (a one-way link out)
    _two_way(links, rng, 101, 1)                      # in-degree 1
    links[(20, 102)] = 2                              # 15 links in, 17 out
    links[(20, 103)] = 2
    row_ptr, col, met = _csr(n, links)
    indeg = np.bincount(col, minlength=n)
    assert set((0, 1, 2, 15, 16, 17, big)) <= set(indeg.tolist()) and indeg.max() == big
    outdeg = np.diff(row_ptr.astype(np.int64))
    assert outdeg[20] == 17 and indeg[20] == 15
    cand = [v for v in range(ring) if v not in hubs and outdeg[v] <= 6]       # roots: few first-hop slots, some next to a hub
    assert len(cand) >= 65
    return (row_ptr, col, met), np.array(cand, np.uint32)


def _spread_roots(n, count):
    count = min(n, count)
    return (np.arange(count, dtype=np.int64) * n // count).astype(np.uint32)


def _child(plan):
    sys.path.insert(0, ROOT)
    from holo_amd import engine as E
    from oracle import graph_oracle as go
    ctx = E.SpfContext(0)
    out = {}

    def check(G, roots, want_dbg):
        res = ctx.run(G, roots, 0)
        ref = go.run(G.row_ptr, G.col, G.metric, G.vflags, INF, roots, 0, go.HEAP, mask_words_=res.first_hop_mask.shape[2],
                     threads=min(16, os.cpu_count() or 1))
        for name, got, want in (("dist", res.dist, ref.dist), ("hops", res.hops, ref.hops), ("flags", res.flags & 1, ref.flags),
                                ("first-hop mask", res.first_hop_mask, ref.mask)):
            assert np.array_equal(got, want), f"{name}: {int(np.count_nonzero(got != want))} words differ"
        if want_dbg is not None:
            assert (res.stats["dbg"][0] & 3) == want_dbg, f"dbg[0] = {res.stats['dbg'][0]}: not the lean sweep's expected instantiation"
            check_plan(res.stats["dbg"][1])

    def check_plan(d1):
        """hspf_stats::dbg[1] of a lean run: dense passes that did work | head sweeps that ran << 8 | passes planned << 16 | head sweeps
        planned << 24, all zero without a plan.  The host launches what it planned: head sweeps are mode 0 with HEAD, the passes mode 1,
        the sweep behind them mode 2 (it always runs: a dense launch always reports a change), the tail mode 0."""
        used, planned, heads = d1 & 0xFF, (d1 >> 16) & 0xFF, (d1 >> 24) & 0x7F
        if plan == "stamped":
            assert d1 == 0, f"dbg[1] = {d1:#x}: a plan under stamped sweeps only"
        elif plan == "nohead":
            # no head sweep: pass 0 starts from the roots alone, and rows 0 .. 3 (a counting wave) hold a root or a root's neighbour
            assert heads == 0 and planned >= 2 and used >= 1, f"dbg[1] = {d1:#x}: the dense stretch did not start the run"
        else:
            assert heads >= 1 and planned >= 2, f"dbg[1] = {d1:#x}: no head sweeps or no dense passes planned"

    def case(name, fn):
        try:
            fn()
            out[name] = "ok"
        except Exception as e:      # noqa: BLE001  (reported to the parent, case by case)
            out[name] = f"{type(e).__name__}: {e}"

    def with_graph(csr, fn):
        G = ctx.upload(csr[0], csr[1], csr[2], np.zeros(len(csr[0]) - 1, np.uint8), INF)
        try:
            fn(G)
        finally:
            G.free()

    try:
        for n in SIZES:
            case(f"n{n}", lambda n=n: with_graph(_csr(n, _ring_with_chords(n, 100 + n)), lambda G: check(G, _spread_roots(n, 65), 1)))
        csr32, cand = _degree_graph(32)
        for r in ROOT_COUNTS:
            case(f"degrees-roots{r}", lambda r=r: with_graph(csr32, lambda G: check(G, cand[:r], 1)))
        # a row of 33 in-links makes a heavy work unit, and a graph with one is not eligible for the lean sweep: this case never
        # runs k_fused_lean (the in-degree-32 graph above is the largest that does); it pins the tables of the sweep that takes over
        csr33, cand33 = _degree_graph(33)
        case("degrees33", lambda: with_graph(csr33, lambda G: check(G, cand33[:65], None)))

        def zero_cost():
            links = _ring_with_chords(200, 5)
            rng = np.random.default_rng(6)
            keys = [k for k in links if k[0] > k[1] + 1]
            for k in rng.choice(len(keys), 6, replace=False):
                links[keys[k]] = 0                    # a zero-cost link from a higher-numbered source: the row of its target is RF_ZERO
            u, v = keys[int(rng.integers(len(keys)))]
            links[(u, v)] = links[(v, u)] = 0         # and a zero-cost cycle
            with_graph(_csr(200, links), lambda G: check(G, _spread_roots(200, 65), 3))       # dbg[0] bit 1: the ZROWS instantiation
        case("zero-cost", zero_cost)

        def patched(structural):
            def run(G):
                roots = _spread_roots(1023, 65)
                check(G, roots, 1)
                u = 517
                a, b = int(G.row_ptr[u]), int(G.row_ptr[u + 1])
                cols, mets = G.col[a:b].copy(), G.metric[a:b].copy()
                if structural:
                    cols, mets = cols[:-1], mets[:-1]     # one row loses a link (the link back stays: it fails the two-way check now)
                else:
                    mets[0] = mets[0] % 9 + 1
                G.patch([u], [(cols, mets)], [G.vflags[u]])
                assert (int(G.export("build_mode")[0]) == 2) == (not structural)
                check(G, roots, 1)
            with_graph(_csr(1023, _ring_with_chords(1023, 100 + 1023)), run)
        case("patch-cost", lambda: patched(False))
        case("patch-structural", lambda: patched(True))
    finally:
        ctx.close()
    print("RESULT " + json.dumps(out))


@functools.lru_cache(maxsize=None)
def _plan_results(plan):
    env = dict(os.environ)
    for k in ("HSPF_VARIANT", "HSPF_LEAN_HEAD", "HSPF_DENSE_PASSES"):
        env.pop(k, None)
    env.update(SWEEPS)
    env.update(PLANS[plan])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), plan], env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and lines, f"child of plan {plan}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    return json.loads(lines[-1][len("RESULT "):])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_lean_record_fetch_matches_oracle(plan, case):
    assert _plan_results(plan)[case] == "ok"


if __name__ == "__main__":
    _child(sys.argv[1])
