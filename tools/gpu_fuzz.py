"""Randomised differential run on the GPU box: many small adversarial LSDBs (LANs of every size, one-way / parallel /
zero-cost links, overloaded and non-expandable vertices, hop-count mode, tight max-path metrics, ragged root lists with
padding entries, network vertices as roots), every run flag combination, optional row patches in between — the HIP
engine against the CPU oracle, bit for bit.  Not part of the pytest suite (minutes, not seconds):

    python tools/gpu_fuzz.py [first_seed] [n_graphs]
    FUZZ_WIDE=n python tools/gpu_fuzz.py [first_seed]      (n graphs with LANs of 150-900 routers: up to 15 mask words)
    FUZZ_MID=n python tools/gpu_fuzz.py [first_seed]       (n graphs of 2 000-19 500 vertices, 1-8 roots per run: k_xcd's range)
    FUZZ_FRR=n python tools/gpu_fuzz.py [first_seed]       (n seeds of the fast-reroute family: every device call of
                                                            holo_amd/csrc/spf_frr.hip.h and the SpfContext chains, on patched
                                                            handles too, against the plain-Python models of tests/)

frr_case(seed) is the host half of FUZZ_FRR (graph, protected roots, options, patches and every expected output, no device);
tests/test_host_frr_fuzz.py checks it without a GPU.
"""
import functools
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from holo_amd import _lib                      # noqa: E402
if os.environ.get("HSPF_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["HSPF_LIB"])
from holo_amd import synth                     # noqa: E402
from holo_amd import engine as E               # noqa: E402
from oracle import graph_oracle as go          # noqa: E402


PATHS = {"k_xcd": 0, "other": 0, "repaired": 0, "exact": 0}   # which kernel took the runs (fuzz_mid reports it: a k_xcd run that gave up shows here);
                                                                # roots put right by k_repair / re-run by the sequential kernel


def compare(ctx, G, g, roots, flags, tag):
    try:
        res = ctx.run(G, roots, flags)
        PATHS["k_xcd" if res.stats.get("single_wg") == 2 else "other"] += 1
        PATHS["repaired"] += res.stats.get("n_repaired_roots", 0); PATHS["exact"] += res.stats.get("n_exact_roots", 0)
    except E.HspfError as e:
        if e.code == -5:                       # documented limit: more than 1024 first-hop slots (16 mask words)
            return True
        raise
    ref = go.run(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric, roots, flags & 3, go.MAP,
                 mask_words_=res.first_hop_mask.shape[2])
    bad = []
    if not np.array_equal(res.dist, ref.dist): bad.append("dist")
    if not np.array_equal(res.hops, ref.hops): bad.append("hops")
    if not np.array_equal(res.flags & 1, ref.flags): bad.append("flags")
    if not np.array_equal(res.first_hop_mask, ref.mask): bad.append("mask")
    if res.pop_rank is not None and not np.array_equal(res.pop_rank, ref.pop_rank): bad.append("pop_rank")
    # round 5: the same run through the packed hand-off (hspf_run_packed); a run whose results do not fit packed words must
    # say so (HSPF_E_NO_PACKED), never deliver something else
    if not (flags & E.RUN_POP_RANK) and os.environ.get("FUZZ_PACKED", "1") != "0":
        try:
            pr = ctx.run_packed(G, roots, flags)
            if not np.array_equal(pr.dist, ref.dist): bad.append("packed dist")
            if not np.array_equal(pr.hops, ref.hops): bad.append("packed hops")
            if not np.array_equal(pr.in_spt, ref.flags.astype(bool)): bad.append("packed in-SPT")
            if res.first_hop_mask.shape[2] != 1 or not np.array_equal(pr.first_hop_mask[..., 0], ref.mask[..., 0]): bad.append("packed mask")
        except E.HspfError as e:
            if e.code != E.E_NO_PACKED:
                raise
            slots = max((G.slot_table(int(r))[2] for r in np.unique(roots) if r != E.NO_ROOT), default=0)
            fused_off = (int(os.environ.get("HSPF_VARIANT", "0") or "0", 0) & 1) or getattr(ctx, "mode", "") == "widemask"   # the A/B switch that turns
            # the fused path off (tests/conftest.py "widemask"): every packed request is refused then, as the header says (include/holo_spf_hip.h)
            if slots <= 16 and not fused_off:  # (17-24 slots: refused once the graph has seen a hop-field overflow)
                bad.append("packed refused a run whose roots have at most 16 first-hop slots")
    if bad:
        print("MISMATCH", tag, bad, "stats", res.stats, flush=True)
        if os.environ.get("FUZZ_DUMP"):
            dump_mismatch(ctx, G, g, roots, flags, res, ref)
    return not bad


def dump_mismatch(ctx, G, g, roots, flags, res, ref):
    """Where the tables differ, and whether the same run differs again (FUZZ_DUMP=1: an intermittent mismatch of round 6)."""
    for name, got, want in (("dist", res.dist, ref.dist), ("hops", res.hops, ref.hops), ("mask", res.first_hop_mask[..., 0], ref.mask[..., 0])):
        d = np.argwhere(got != want)
        if not len(d):
            continue
        rr, vv = int(d[0][0]), int(d[0][1])
        print("  ", name, "differs at", len(d), "places; roots", sorted(set(d[:, 0].tolist()))[:10], "first: slot", rr, "root", int(roots[rr]), "vertex", vv,
              "got", int(got[rr, vv]), "want", int(want[rr, vv]), "dist", int(ref.dist[rr, vv]), "exact flag", int(res.flags[rr, vv] & 2), flush=True)
        print("   vertices of that root:", d[d[:, 0] == rr][:12, 1].tolist(), "vflags", int(g.vflags[vv]))
        ins = [(int(u), int(g.metric[kx])) for u in range(g.n) for kx in range(int(g.row_ptr[u]), int(g.row_ptr[u + 1])) if g.col[kx] == vv]
        print("   links into it (source, cost, ref dist, ref hops, got hops, ref rank):",
              [(u, c, int(ref.dist[rr, u]), int(ref.hops[rr, u]), int(res.hops[rr, u]), int(ref.pop_rank[rr, u]) if ref.pop_rank is not None else None) for u, c in ins][:20], flush=True)
        break
    for again in range(3):
        r2 = ctx.run(G, roots, flags)
        print("   again:", {"dist": int((r2.dist != ref.dist).sum()), "hops": int((r2.hops != ref.hops).sum()), "mask": int((r2.first_hop_mask != ref.mask).sum())},
              "repaired", r2.stats.get("n_repaired_roots"), "sweeps", r2.stats.get("repair_sweeps"), flush=True)


def fuzz(ctx, first, count, verbose=True):
    ok = runs = 0
    t0 = time.time()
    for seed in range(first, first + count):
        rng = np.random.default_rng(10_000 + seed)
        nr = int(rng.integers(5, 260)) if rng.random() > 0.04 else int(rng.integers(800, 3000))
        nn = int(rng.integers(0, 14))
        hop = rng.random() < 0.2
        zero = os.environ.get("FUZZ_ZERO") is not None              # round 6: every graph with zero-cost router links and tie-heavy costs (dynamic pop orders)
        g = synth.random_lsdb(nr, nn, float(rng.uniform(1.2, 4.5)), 50_000 + seed,
                              metric_lo=1, metric_hi=int(rng.integers(1, 5 if zero else 40)),
                              max_path=(1023 if rng.random() < 0.15 else (0xFFFFFFFF if rng.random() < 0.3 else synth.MAX_PATH_METRIC_WIDE)),
                              p_oneway=float(rng.choice([0.0, 0.03, 0.3])), p_parallel=float(rng.choice([0.0, 0.05, 0.4])),
                              p_overload=float(rng.choice([0.0, 0.03, 0.3])), p_noexpand=float(rng.choice([0.0, 0.02, 0.2])),
                              zero_cost_router_links=bool(rng.random() < 0.15) or zero, lan_size=int(rng.choice([2, 3, 5, 8, 14, 20, 30, 45, 70, 140])), hopcount=hop)
        if rng.random() < 0.15 and not hop:                       # large costs: 8-byte state, max-path pruning, u32 saturation
            g.metric = (g.metric.astype(np.uint64) << int(rng.integers(8, 25))).clip(0, 0xFFFFFFFE).astype(np.uint32)
        G = ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
        for rep in range(3):
            k = int(rng.integers(1, min(g.n, 200 if g.n < 800 else 700) + 1))
            if os.environ.get("FUZZ_MAX_ROOTS"):                     # (the one-XCD-per-root kernel takes runs of at most eight roots)
                k = min(k, int(rng.integers(1, int(os.environ["FUZZ_MAX_ROOTS"]) + 1)))
            roots = rng.choice(g.n, size=k, replace=rng.random() < 0.2).astype(np.uint32)
            if k > 3 and rng.random() < 0.3:
                roots[int(rng.integers(0, k))] = E.NO_ROOT
            flags = int(rng.choice([0, E.RUN_NET_NEXTHOPS, E.RUN_IGNORE_OVERLOAD, E.RUN_NET_NEXTHOPS | E.RUN_IGNORE_OVERLOAD]))
            if hop:
                flags |= E.RUN_IGNORE_OVERLOAD
            if rng.random() < (0.3 if zero else 0.08):
                flags |= E.RUN_POP_RANK
            runs += 1
            t_run = time.time()
            ok += compare(ctx, G, g, roots, flags, (seed, rep, flags, k))
            if rng.random() < 0.12:                                  # an instance repeating its run: the lean sweep learns its mode schedule
                for again in range(4):                                # (plain, learning, scheduled, scheduled)
                    runs += 1
                    ok += compare(ctx, G, g, roots, flags, (seed, rep, flags, k, "repeat", again))
            if os.environ.get("FUZZ_TIMING") and time.time() - t_run > float(os.environ["FUZZ_TIMING"]):
                print(f"SLOW seed {seed} rep {rep} n {g.n} roots {k} flags {flags} hop {hop} maxpath {g.max_path_metric:#x}: {time.time() - t_run:.2f} s, stats {ctx.stats()}", flush=True)
            if rep < 2 and rng.random() < 0.5:                      # re-originate a few rows in between
                vs = np.sort(rng.choice(g.n, size=int(rng.integers(1, 6)), replace=False))
                rows, fl = [], []
                costs_only = rng.random() < 0.5                     # a metric change: applied in place (build mode 2)
                for v in vs.tolist():
                    c = g.col[g.row_ptr[v]:g.row_ptr[v + 1]]; m = g.metric[g.row_ptr[v]:g.row_ptr[v + 1]]
                    keep = rng.random(len(c)) > (-1.0 if costs_only else 0.25)
                    c, m = c[keep], m[keep].copy()
                    if len(m) and (v >= nn or costs_only):
                        m[rng.random(len(m)) < 0.5] = int(rng.integers(0 if costs_only else 1, 9)) if not hop else int(rng.integers(0, 2))
                    rows.append((c, m)); fl.append(int(g.vflags[v]) ^ (synth.VF_NO_TRANSIT if (v >= nn and not costs_only and rng.random() < 0.3) else 0))
                G.patch(vs, rows, fl)
                if costs_only and int(G.export("build_mode")[0]) != 2 and int(np.diff(G.export("in_ptr")).max(initial=0)) <= 256:
                    print("COST PATCH NOT IN PLACE", seed, rep, flush=True); ok -= 1
                g = synth.CsrGraph(G.row_ptr, G.col, G.metric, G.vflags, g.max_path_metric, g.name, g.meta)
        G.free()
    if verbose:
        print(f"fuzz: {ok}/{runs} runs bit-exact over {count} graphs in {time.time() - t0:.1f} s (roots put right by k_repair: {PATHS['repaired']}, by the sequential kernel: {PATHS['exact']})", flush=True)
    return ok, runs


def fuzz_mid(ctx, first, count, verbose=True):
    """Mid-size LSDBs (2 000 - 19 500 vertices: beyond the one-workgroup kernel, inside k_xcd's 20 000), one to eight roots per
    run — what k_xcd and the choice between it and the sweep engine see in production —, the adversarial ingredients of
    fuzz() and row patches in between."""
    ok = runs = 0
    t0 = time.time()
    for seed in range(first, first + count):
        rng = np.random.default_rng(170_000 + seed)
        nr = int(rng.integers(2000, 19000))
        nn = int(rng.integers(0, 500))
        hop = rng.random() < 0.2
        g = synth.random_lsdb(nr, nn, float(rng.uniform(1.5, 4.0)), 180_000 + seed, metric_lo=1, metric_hi=int(rng.integers(1, 60)),
                              max_path=(4095 if rng.random() < 0.1 else (0xFFFFFFFF if rng.random() < 0.3 else synth.MAX_PATH_METRIC_WIDE)),
                              p_oneway=float(rng.choice([0.0, 0.03])), p_parallel=float(rng.choice([0.0, 0.05])),
                              p_overload=float(rng.choice([0.0, 0.03, 0.2])), p_noexpand=float(rng.choice([0.0, 0.02])),
                              zero_cost_router_links=bool(rng.random() < 0.1), lan_size=int(rng.choice([2, 4, 8, 20, 40])), hopcount=hop)
        G = ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
        for rep in range(4):
            k = int(rng.integers(1, 9))
            roots = rng.choice(g.n, size=k, replace=False).astype(np.uint32)
            if k > 2 and rng.random() < 0.3:
                roots[int(rng.integers(0, k))] = E.NO_ROOT
            flags = int(rng.choice([0, E.RUN_NET_NEXTHOPS, E.RUN_IGNORE_OVERLOAD, E.RUN_NET_NEXTHOPS | E.RUN_IGNORE_OVERLOAD]))
            if hop:
                flags |= E.RUN_IGNORE_OVERLOAD
            for again in range(1 if rep else 7):                       # the first root set seven times: the product context tries both kernels, then chooses
                runs += 1
                ok += compare(ctx, G, g, roots, flags, ("mid", seed, rep, flags, k, again))
            if rep < 3:
                vs = np.sort(rng.choice(g.n, size=int(rng.integers(1, 5)), replace=False))
                rows, fl = [], []
                costs_only = rng.random() < 0.5
                for v in vs.tolist():
                    c = g.col[g.row_ptr[v]:g.row_ptr[v + 1]]; m = g.metric[g.row_ptr[v]:g.row_ptr[v + 1]]
                    keep = rng.random(len(c)) > (-1.0 if costs_only else 0.25)
                    c, m = c[keep], m[keep].copy()
                    if len(m) and (v >= nn or costs_only):
                        m[rng.random(len(m)) < 0.5] = int(rng.integers(0 if costs_only else 1, 9)) if not hop else int(rng.integers(0, 2))
                    rows.append((c, m)); fl.append(int(g.vflags[v]))
                G.patch(vs, rows, fl)
                g = synth.CsrGraph(G.row_ptr, G.col, G.metric, G.vflags, g.max_path_metric, g.name, g.meta)
        G.free()
    if verbose:
        print(f"fuzz_mid: {ok}/{runs} runs bit-exact over {count} graphs in {time.time() - t0:.1f} s (k_xcd took {PATHS['k_xcd']} of them)", flush=True)
    return ok, runs


def fuzz_wide(ctx, first, count, verbose=True):
    """Many first-hop slots: one to three LANs of 150-900 routers (up to 15 mask words, k_fw<W> for every W, rows far beyond
    32 in-links = work units; 1 000+ members = hub-mode graph build), roots on and off the LANs, LAN vertices as roots."""
    ok = runs = 0
    t0 = time.time()
    for seed in range(first, first + count):
        rng = np.random.default_rng(130_000 + seed)
        lan = int(rng.choice([150, 260, 400, 640, 900]))
        nr = lan + int(rng.integers(0, 300)) if rng.random() < 0.5 else lan * int(rng.integers(2, 5))   # most routers off the LAN:
                                                                  # one mask word, the LAN's row is a giant row of k_fused
        nn = int(rng.integers(1, 4))
        hop = rng.random() < 0.15
        g = synth.random_lsdb(nr, nn, float(rng.uniform(1.0, 3.0)), 140_000 + seed, metric_lo=1, metric_hi=int(rng.integers(1, 12)),
                              p_oneway=float(rng.choice([0.0, 0.05])), p_parallel=float(rng.choice([0.0, 0.1])),
                              p_overload=float(rng.choice([0.0, 0.05])), p_noexpand=float(rng.choice([0.0, 0.02])),
                              zero_cost_router_links=bool(rng.random() < 0.1), lan_size=lan, hopcount=hop)
        G = ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
        for rep in range(2):
            k = int(rng.integers(1, 90))
            roots = rng.choice(g.n, size=k, replace=False).astype(np.uint32)
            if rep == 0:
                roots[0] = int(rng.integers(0, nn))                       # a LAN vertex itself
            flags = int(rng.choice([0, E.RUN_NET_NEXTHOPS, E.RUN_IGNORE_OVERLOAD, 3]))
            if hop:
                flags |= E.RUN_IGNORE_OVERLOAD
            runs += 1
            ok += compare(ctx, G, g, roots, flags, ("wide", seed, rep, flags, k))
        G.free()
    if verbose:
        print(f"fuzz_wide: {ok}/{runs} runs bit-exact over {count} graphs in {time.time() - t0:.1f} s", flush=True)
    return ok, runs


def fuzz_layout(ctx, first, count, verbose=True, spf=False):
    """Device graph construction and row patches: every exported array against the numpy restatement
    (tests/_layout_ref.py), and a patched graph against a fresh upload of the patched CSR."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from _layout_ref import layout
    built = ("twoway", "in_ptr", "in_src", "in_cost", "in_pos", "out_ptr", "out_dst", "out_cost", "out_pos", "rowflags", "leaf")
    derived = ("ell_src", "ell_cost", "ell_out", "summary")
    ok = runs = 0
    t0 = time.time()
    for seed in range(first, first + count):
        rng = np.random.default_rng(70_000 + seed)
        g = synth.random_lsdb(int(rng.integers(3, 150)), int(rng.integers(0, 10)), float(rng.uniform(1.0, 5.0)), 90_000 + seed,
                              metric_hi=int(rng.integers(1, 10)), p_oneway=float(rng.choice([0.0, 0.1, 0.5])),
                              p_parallel=float(rng.choice([0.0, 0.2, 0.6])), p_overload=float(rng.choice([0.0, 0.3])),
                              p_noexpand=float(rng.choice([0.0, 0.3])), zero_cost_router_links=bool(rng.random() < 0.3),
                              lan_size=int(rng.choice([2, 6, 20, 50])), hopcount=bool(rng.random() < 0.2))
        G = ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
        for rep in range(3):
            want = layout(G.row_ptr, G.col, G.metric, G.vflags)
            good = all(np.array_equal(G.export(k), want[k]) for k in built) and G.n_edges_kept == len(want["in_src"])
            good = good and all(np.array_equal(G.export(k), getattr(G, k)) for k in ("row_ptr", "col", "metric", "vflags"))
            good = good and np.array_equal(G.export("host_row_ptr"), G.row_ptr) and np.array_equal(G.export("host_col"), G.col)   # the library's host mirrors
            runs += 1
            ok += good
            if not good:
                print("LAYOUT MISMATCH", seed, rep, flush=True)
            n = G.n
            vs = np.sort(rng.choice(n, size=int(rng.integers(1, min(n, 12) + 1)), replace=False))
            rows, fl = [], []
            for v in vs.tolist():
                deg = int(rng.integers(0, 9))
                rows.append((rng.integers(0, n, deg).astype(np.uint32), rng.integers(0, 6, deg).astype(np.uint32)))
                fl.append(int(rng.integers(0, 8)))
            G.patch(vs, rows, fl)
            if rng.random() < 0.6:                             # ... then new costs on some rows, in place; arrays and summary as a fresh upload's
                vs2 = np.sort(rng.choice(n, size=int(rng.integers(1, min(n, 12) + 1)), replace=False))
                rows2 = []
                for v in vs2.tolist():
                    c = G.col[G.row_ptr[v]:G.row_ptr[v + 1]].copy()
                    rows2.append((c, rng.integers(0, 6, len(c)).astype(np.uint32)))
                G.patch(vs2, rows2, G.vflags[vs2].copy())
                F = ctx.upload(G.row_ptr, G.col, G.metric, G.vflags, g.max_path_metric)
                good = all(np.array_equal(G.export(k), F.export(k)) for k in built + derived)
                good = good and (int(G.export("build_mode")[0]) == 2 or int(np.diff(G.export("in_ptr")).max(initial=0)) > 256)
                F.free()
                runs += 1
                ok += good
                if not good:
                    print("COST PATCH MISMATCH", seed, rep, flush=True)
            if spf:                                            # SPF on whatever graph the arbitrary rows made
                gg = synth.CsrGraph(G.row_ptr, G.col, G.metric, G.vflags, g.max_path_metric)
                roots = rng.choice(n, size=int(rng.integers(1, min(n, 70) + 1)), replace=False).astype(np.uint32)
                flags = int(rng.choice([0, E.RUN_NET_NEXTHOPS, E.RUN_IGNORE_OVERLOAD, 3]))
                runs += 1
                ok += compare(ctx, G, gg, roots, flags, ("arbitrary", seed, rep, flags))
        G.free()
    if verbose:
        print(f"fuzz_layout: {ok}/{runs} layouts identical over {count} graphs in {time.time() - t0:.1f} s", flush=True)
    return ok, runs


def fuzz_routes(ctx, first, count, verbose=True):
    """hspf_routes_device (IS-IS rule, OSPF saturating add, OSPF last-min-replaces) on random prefix tables against a
    per-prefix restatement over the oracle's SPT tables."""
    import torch
    dev = torch.device("cuda:0")
    ok = runs = 0
    t0 = time.time()
    for seed in range(first, first + count):
        rng = np.random.default_rng(130_000 + seed)
        g = synth.random_lsdb(int(rng.integers(5, 120)), int(rng.integers(0, 8)), float(rng.uniform(1.5, 4.0)), 140_000 + seed,
                              metric_hi=int(rng.integers(1, 8)), lan_size=int(rng.choice([2, 5, 12])), max_path=0xFFFFFFFF)
        n = g.n
        R = int(rng.integers(1, min(n, 70) + 1))
        roots = rng.choice(n, size=R, replace=False).astype(np.uint32)
        rflags = int(rng.choice([0, E.RUN_NET_NEXTHOPS]))
        ref = go.run(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric, roots, rflags, go.MAP)
        W = ref.mask.shape[2]
        G = ctx.upload(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric)
        dist = torch.empty((R, n), dtype=torch.int32, device=dev); hops = torch.empty((R, n), dtype=torch.int16, device=dev)
        fl = torch.empty((R, n), dtype=torch.int16, device=dev); mask = torch.empty((R, n, W), dtype=torch.int64, device=dev)
        ctx.run_device(G, roots, rflags, dist_ptr=dist.data_ptr(), hops_ptr=hops.data_ptr(), flags_ptr=fl.data_ptr(),
                       mask_ptr=mask.data_ptr(), mask_words=W)
        G.free()
        P = int(rng.integers(1, 60)); ne = int(rng.integers(0, 200))
        pfx = np.sort(rng.integers(0, P, ne)); vtx = rng.integers(0, n, ne)
        order = np.lexsort((vtx, pfx)); pfx, vtx = pfx[order], vtx[order].astype(np.uint32)
        met = rng.integers(0, 4, ne).astype(np.uint32)
        big = rng.random(ne) < 0.08
        met[big] = (0xFFFFFFFF - rng.integers(0, 6, int(big.sum()))).astype(np.uint32)
        ptr = np.zeros(P + 1, np.uint32); np.add.at(ptr, pfx + 1, 1); ptr = np.cumsum(ptr, dtype=np.uint64).astype(np.uint32)
        for mode in (0, E.PFX_SATURATING, E.PFX_LAST_MIN, E.PFX_SATURATING | E.PFX_LAST_MIN):
            bm = torch.empty((R, P), dtype=torch.int32, device=dev); be = torch.empty((R, P), dtype=torch.int32, device=dev)
            nm = torch.empty((R, P, W), dtype=torch.int64, device=dev)
            ctx.routes_device(n, R, W, dist.data_ptr(), fl.data_ptr(), mask.data_ptr(), ptr, vtx, met, best_metric_ptr=bm.data_ptr(),
                              best_entry_ptr=be.data_ptr(), nexthop_mask_ptr=nm.data_ptr(), flags=mode)
            torch.cuda.synchronize()
            hbm = bm.cpu().numpy().view(np.uint32); hbe = be.cpu().numpy().view(np.uint32); hnm = nm.cpu().numpy().view(np.uint64)
            sat, last = bool(mode & E.PFX_SATURATING), bool(mode & E.PFX_LAST_MIN)
            good = True
            for r in range(R):
                for p in range(P):
                    best, ent, acc = 0xFFFFFFFF, 0xFFFFFFFF, np.zeros(W, np.uint64)
                    for e in range(int(ptr[p]), int(ptr[p + 1])):
                        v = int(vtx[e])
                        if not ref.flags[r, v]:
                            continue
                        m = int(ref.dist[r, v]) + int(met[e])
                        m = min(m, 0xFFFFFFFF) if sat else m & 0xFFFFFFFF
                        if ent == 0xFFFFFFFF or m < best or (last and m == best):
                            best, ent, acc = m, e, ref.mask[r, v].copy()
                        elif m == best:
                            acc |= ref.mask[r, v]
                    good = good and hbm[r, p] == best and hbe[r, p] == ent and np.array_equal(hnm[r, p], acc)
            runs += 1
            ok += good
            if not good:
                print("ROUTES MISMATCH", seed, mode, flush=True)
    if verbose:
        print(f"fuzz_routes: {ok}/{runs} tables identical over {count} graphs in {time.time() - t0:.1f} s", flush=True)
    return ok, runs


# ------------------------------------------------------------------------------------------------- the fast-reroute family

_MODELS = None
FRR_ENGINES = {"default": {}, "hubsort": {"hub_deg": 0, "tw_host_max": 0}, "patchfull": {"patch_full": True}}      # tests/_frr_chains.py
LFA_FIELDS = ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask", "coverage")
ROUTE_FIELDS = ("best_metric", "best_entry", "nexthop_mask")
CAND_FIELDS = ("nbr", "cost", "root_link", "cflags")
FRR_MAX_SLOTS = 130                           # the models cost seconds per root beyond this (several mask words of slots)
FRR_LAN_SIZES = ([2, 3, 5, 8, 14, 20, 30, 62], [0.12, 0.12, 0.16, 0.16, 0.14, 0.1, 0.1, 0.1])      # 62: a member has a second mask word of slots


def _m():
    """The plain-Python models of tests/ (numpy over the CPU oracle, no GPU import)."""
    global _MODELS
    if _MODELS is None:
        import types
        tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
        if tests not in sys.path:
            sys.path.insert(0, tests)
        import _backup_model as B, _lfa_lan_model as LM, _lfa_model as M, _patch_model as pm, _rlfa_lan_model as RL      # noqa: E401
        import _rlfa_model as R, _rlfa_node_model as N, _tilfa_model as T      # noqa: E401
        _MODELS = types.SimpleNamespace(B=B, LM=LM, M=M, pm=pm, RL=RL, R=R, N=N, T=T)
    return _MODELS


def _stack(objs, fields):
    return {f: np.stack([np.asarray(getattr(o, f)) for o in objs]) for f in fields}


def _pad(a, words):
    """[P, ..., k] -> [P, ..., words] with zeros: what a LAN call writes where no slot crosses a LAN."""
    out = np.zeros(a.shape[:-1] + (words,), a.dtype)
    out[..., :a.shape[-1]] = a
    return out


class FrrStep:
    """One (seed, step) of frr_case: the spliced CSR, the protected roots, the drawn options, the patch that led here, and —
    computed on first use, on the host alone — the plan and every expected output."""

    def __init__(self, seed, index, graph, maxp, prot, opt, patch=None, costs_only=None):
        self.seed, self.index, self.graph, self.maxp, self.prot, self.opt = seed, index, graph, maxp, tuple(prot), opt
        self.patch, self.costs_only = patch, costs_only
        self._plan = self._models = self._want = self._chain = None

    @property
    def plan(self):
        """(roots, [(root_row, candidates, nbr_row, lan, lan_row)], W): one table set for all protected roots, the ascending union
        of [S] + neighbour routers + LANs (plan() of tests/test_gpu_lfa_lan.py), W with the drawn extra mask words."""
        if self._plan is None:
            from oracle import graph_oracle as go
            m = _m()
            per, rows = [], []
            for S in self.prot:
                c, r, _, lan, _ = m.LM.protect_one(*self.graph, S)
                per.append((c, lan))
                rows += [int(x) for x in r]
            roots = np.array(sorted(set(rows)), np.uint32)
            row_of = {int(v): i for i, v in enumerate(roots)}
            out = [(row_of[c.root], c, np.array([row_of.get(int(x), 0) for x in c.nbr], np.uint32), lan,
                    np.array([row_of.get(int(x), 0) for x in lan], np.uint32)) for c, lan in per]
            W = max(go.mask_words(*self.graph, roots), max((len(c.nbr) + 63) // 64 for c, _ in per), 1) + self.opt.w_extra
            self._plan = (roots, out, W)
        return self._plan

    @property
    def models(self):
        """Per protected root the model objects, by name; plus the oracle tables (`fwd`, `rdist`) and `y_roots`."""
        if self._models is None:
            m, o, g = _m(), self.opt, self.graph
            roots, per, W = self.plan
            fwd, rdist = m.R.tables(g, self.maxp, roots, o.run_flags, W)
            t3 = (fwd.dist, fwd.flags, fwd.mask)
            lf = o.lfa_flags
            w = {k: [] for k in ("lfa", "lfa_lan", "rlfa", "rlfa_lan", "tilfa", "tilfa_lan", "routes", "backup", "backup_noti", "backup_lan",
                                 "backup_lan_noti", "sel", "dest")}
            for r, c, nr, lan, lr in per:
                a = m.M.lfa(*t3, c, r, nr, lf)
                al = m.LM.lfa(*t3, c, r, nr, lan, lr, lf)
                alt, alt_l = (a.alt_flags, al.alt_flags) if o.with_alt else (None, None)
                rl = m.R.rlfa(*t3, rdist, g[3], c, r, nr, lf, alt)
                rll = m.RL.rlfa(*t3, rdist, g[3], c, r, nr, lan, lr, lf, alt_l)
                ti = m.T.tilfa(*t3, rdist, g, c, r, nr, rl.space_flags, rl.space_via, alt)
                til = m.RL.tilfa(*t3, rdist, g, c, r, nr, rll, alt_l)
                rt = m.B.routes(*t3, r, o.pt)
                safe = m.RL.LAN_SAFE_REPAIRS if o.safe else 0
                w["lfa"].append(a); w["lfa_lan"].append(al); w["rlfa"].append(rl); w["rlfa_lan"].append(rll)
                w["tilfa"].append(ti); w["tilfa_lan"].append(til); w["routes"].append(rt)
                w["backup"].append(m.B.backup(*t3, c, r, nr, o.pt, rt, lf, ti))
                w["backup_noti"].append(m.B.backup(*t3, c, r, nr, o.pt, rt, lf, None))
                w["backup_lan"].append(m.RL.backup(*t3, c, r, nr, lan, lr, o.pt, rt, lf | safe, til if o.safe else ti))
                w["backup_lan_noti"].append(m.RL.backup(*t3, c, r, nr, lan, lr, o.pt, rt, lf | safe, None))
                w["sel"].append(m.N.select(fwd.dist, c, r, nr, rl.space_flags, lf, o.max_pq))
            y = sorted({v for s in w["sel"] for v in m.N.union(s)})
            yrows = m.N.y_rows(g, self.maxp, y, o.run_flags)
            for (r, c, nr, _, _), s, a in zip(per, w["sel"], w["lfa"]):
                w["dest"].append(m.N.dest(*t3, c, r, nr, s, yrows, a.alt_flags if o.with_alt else None))
            w.update(fwd=fwd, rdist=rdist, y_roots=np.array(y or [m.N.NONE], np.uint32))
            self._models = w
        return self._models

    @property
    def want(self):
        """{call: {field: [P, ...] array}}: the expected side of every comparison of the device calls."""
        if self._want is None:
            m, w = _m(), self.models
            rows = [r for r, *_ in self.plan[1]]
            f = w["fwd"]
            out = {"run_device": dict(dist=f.dist, flags=f.flags, mask=f.mask, rdist=w["rdist"]),
                   "lfa_device": _stack(w["lfa"], LFA_FIELDS), "lfa_lan_device": _stack(w["lfa_lan"], LFA_FIELDS),
                   "rlfa_device": _stack(w["rlfa"], m.R.FIELDS), "rlfa_lan_device": _stack(w["rlfa_lan"], m.R.FIELDS),
                   "tilfa_device": _stack(w["tilfa"], m.T.FIELDS), "tilfa_device(lan tables)": _stack(w["tilfa_lan"], m.T.FIELDS),
                   "routes_device": _stack(w["routes"], ROUTE_FIELDS),
                   "routes_backup_device": _stack(w["backup"], m.B.FIELDS), "routes_backup_device(no tilfa)": _stack(w["backup_noti"], m.B.FIELDS),
                   "routes_backup_lan_device": _stack(w["backup_lan"], m.B.FIELDS),
                   "routes_backup_lan_device(no tilfa)": _stack(w["backup_lan_noti"], m.B.FIELDS),
                   "rlfa_node_select_device": _stack(w["sel"], m.N.SEL_FIELDS), "rlfa_node_device": _stack(w["dest"], m.N.DEST_FIELDS)}
            out["rlfa_node_select_device"]["y_roots"] = w["y_roots"][None, :]
            out["rlfa_device(no spaces)"], out["rlfa_lan_device(no spaces)"] = out["rlfa_device"], out["rlfa_lan_device"]
            # all LAN columns NONE: the outputs of the plain calls, the LAN words zero (the no_lans checks of tests/test_gpu_*_lan.py)
            nl = dict(out["lfa_device"]); nl["coverage"] = _pad(nl["coverage"], 7)
            nr_ = dict(out["rlfa_device"]); nr_["pq_counts"] = _pad(nr_["pq_counts"], m.RL.COUNT_WORDS); nr_["rl_coverage"] = _pad(nr_["rl_coverage"], m.RL.COVERAGE_WORDS)
            nb = dict(out["routes_backup_device"]); nb["bk_coverage"] = _pad(nb["bk_coverage"], 9)
            out.update({"lfa_lan_device(no lans)": nl, "rlfa_lan_device(no lans)": nr_, "routes_backup_lan_device(no lans)": nb})
            del rows
            self._want = out
        return self._want

    @property
    def chain(self):
        """{call: {field: [1, ...] array}} of the SpfContext chains for the drawn protected root, from the same models over the
        chain's own rows ([root] + neighbour routers (+ LANs)); rdist is the forward dist where `symmetric` says so."""
        if self._chain is None:
            from oracle import graph_oracle as go
            m, o, g = _m(), self.opt, self.graph
            root, lf = self.prot[o.chain_root], o.lfa_flags
            cache = {}

            def mdl(lp, sym, lan_spaces):
                if (lp, sym, lan_spaces) not in cache:
                    import types
                    if lp:
                        c, roots, nr, lan, lr = m.LM.protect_one(*g, root)
                    else:
                        (c, roots, nr), lan, lr = m.M.protect_one(*g, root), None, None
                    W = max(go.mask_words(*g, roots), (len(c.nbr) + 63) // 64, 1)
                    fwd, rdist = m.R.tables(g, self.maxp, roots, o.run_flags, W)
                    t3, rd = (fwd.dist, fwd.flags, fwd.mask), fwd.dist if sym else rdist
                    a = m.LM.lfa(*t3, c, 0, nr, lan, lr, lf) if lp else m.M.lfa(*t3, c, 0, nr, lf)
                    rl = m.RL.rlfa(*t3, rd, g[3], c, 0, nr, lan, lr, lf, a.alt_flags) if lan_spaces else m.R.rlfa(*t3, rd, g[3], c, 0, nr, lf, a.alt_flags)
                    ti = m.T.tilfa(*t3, rd, g, c, 0, nr, rl.space_flags, rl.space_via, a.alt_flags)
                    cache[(lp, sym, lan_spaces)] = types.SimpleNamespace(c=c, nr=nr, lan=lan, lr=lr, t3=t3, lfa=a, rl=rl, ti=ti)
                return cache[(lp, sym, lan_spaces)]

            lp, sym = o.lan_protect, o.symmetric and not o.lan_protect
            x = mdl(lp, sym, lp)
            out = {"SpfContext.lfa": dict(_stack([x.lfa], LFA_FIELDS), **_stack([x.c], CAND_FIELDS)),
                   "SpfContext.rlfa": _stack([x.rl], m.R.FIELDS), "SpfContext.tilfa": dict(_stack([x.rl], m.R.FIELDS), **_stack([x.ti], m.T.FIELDS))}
            if lp:
                out["SpfContext.lfa"]["lan"] = x.lan[None, :]
            p = mdl(False, o.symmetric, False)
            sel = m.N.select(p.t3[0], p.c, 0, p.nr, p.rl.space_flags, lf, o.max_pq)
            y = m.N.union(sel)
            d = m.N.dest(*p.t3, p.c, 0, p.nr, sel, m.N.y_rows(g, self.maxp, y, o.run_flags), p.lfa.alt_flags)
            out["SpfContext.rlfa_node"] = dict(_stack([sel], m.N.SEL_FIELDS), **_stack([d], m.N.DEST_FIELDS), y_roots=np.array(y or [m.N.NONE], np.uint32)[None, :])
            b = mdl(lp, sym, o.lan_repairs)
            rt = m.B.routes(*b.t3, 0, o.pt)
            ti = b.ti if o.remote else None
            if lp:
                bk = m.RL.backup(*b.t3, b.c, 0, b.nr, b.lan, b.lr, o.pt, rt, lf | (m.RL.LAN_SAFE_REPAIRS if o.lan_repairs else 0), ti)
            else:
                bk = m.B.backup(*b.t3, b.c, 0, b.nr, o.pt, rt, lf, ti)
            out["SpfContext.backup_routes"] = dict(_stack([rt], ROUTE_FIELDS), **_stack([bk], m.B.FIELDS), **(_stack([ti], m.T.FIELDS) if o.remote else {}))
            self._chain = out
        return self._chain


def _frr_options(rng, n):
    """The drawn options of one step."""
    import types
    m = _m()
    n_pfx = int(rng.choice([1, int(rng.integers(2, 40)), int(rng.integers(40, 90))]))
    lists = []
    for _ in range(n_pfx):
        adv = rng.choice(n, size=min(int(rng.choice([1, 2, 2, 3])), n), replace=False)
        lists.append([(int(v), int(0xFFFFFFFF - rng.integers(0, 6)) if rng.random() < 0.04 else int(rng.integers(0, 16))) for v in adv])
    pt = m.B.table(lists, int(rng.choice([0, m.B.PFX_SATURATING, m.B.PFX_LAST_MIN, m.B.PFX_SATURATING | m.B.PFX_LAST_MIN])))
    lan_protect = bool(rng.random() < 0.6)
    lan_repairs = lan_protect and bool(rng.random() < 0.5)
    return types.SimpleNamespace(
        run_flags=int(rng.choice([0, E.RUN_NET_NEXTHOPS, E.RUN_IGNORE_OVERLOAD, E.RUN_NET_NEXTHOPS | E.RUN_IGNORE_OVERLOAD])),
        lfa_flags=int(rng.random() < 0.35), safe=bool(rng.random() < 0.5), w_extra=int(rng.choice([0, 0, 1, 2])), masks=bool(rng.random() < 0.6),
        masks_lan=bool(rng.random() < 0.6), spaces=bool(rng.random() < 0.6), with_alt=bool(rng.random() < 0.7), max_pq=int(rng.integers(1, 33)), pt=pt,
        resident=bool(rng.random() < 0.5), order=rng.permutation(7).tolist(), chain_root=0, symmetric=bool(rng.random() < 0.4), lan_protect=lan_protect,
        lan_repairs=lan_repairs, remote=lan_repairs or bool(rng.random() < 0.7))


@functools.lru_cache(maxsize=None)
def frr_case(seed):
    """The host side of fuzz_frr for one seed, deterministic in it: [FrrStep] — an adversarial LSDB with the ingredients of fuzz()
    (5 to 300 vertices, LANs of 2 to 62 routers), one to four protected routers of at most FRR_MAX_SLOTS first-hop slots over one
    table set, drawn options per step, and zero to two row patches as fuzz() draws them, applied with engine.splice_rows.  Every
    expected output comes from the models of tests/ over the CPU oracle's SPTs of the spliced CSR; nothing touches the device."""
    m = _m()
    rng = np.random.default_rng(310_000 + seed)
    n = int([rng.integers(5, 60), rng.integers(60, 257), rng.integers(257, 301)][int(rng.choice(3, p=[0.55, 0.3, 0.15]))])
    lan_size = int(rng.choice(FRR_LAN_SIZES[0], p=FRR_LAN_SIZES[1]))
    nn = int(rng.integers(0, min(8 if lan_size < 30 else 2, n // 3) + 1))      # (a router on three big LANs has too many slots for the models)
    nr = n - nn
    g = synth.random_lsdb(nr, nn, float(rng.uniform(1.2, 4.5)), 320_000 + seed, metric_lo=1, metric_hi=int(rng.integers(1, 40)),
                          max_path=(1023 if rng.random() < 0.15 else (0xFFFFFFFF if rng.random() < 0.3 else synth.MAX_PATH_METRIC_WIDE)),
                          p_oneway=float(rng.choice([0.0, 0.03, 0.3])), p_parallel=float(rng.choice([0.0, 0.05, 0.4])),
                          p_overload=float(rng.choice([0.0, 0.03, 0.3])), p_noexpand=float(rng.choice([0.0, 0.02, 0.2])),
                          zero_cost_router_links=bool(rng.random() < 0.15), lan_size=lan_size)
    if rng.random() < 0.15:                                        # large costs: sums beyond 32 bits, max-path pruning, saturation
        g.metric = (g.metric.astype(np.uint64) << int(rng.integers(8, 25))).clip(0, 0xFFFFFFFE).astype(np.uint32)
    graph, maxp = (g.row_ptr, g.col, g.metric, g.vflags), int(g.max_path_metric)
    # protected roots: plain routers; more often than not one that sits on a LAN; never more than FRR_MAX_SLOTS slots
    plain = [v for v in range(nn, n) if not graph[3][v] & 0x07]
    on_lan = [v for v in plain if (graph[1][graph[0][v]:graph[0][v + 1]] < nn).any()]
    prot = []
    for _ in range(int(rng.integers(1, 5))):
        pool = on_lan if on_lan and rng.random() < 0.6 else plain
        for v in rng.permutation(pool).tolist()[:6]:
            if v not in prot and len(m.M.candidates(*graph, v).nbr) <= FRR_MAX_SLOTS:
                prot.append(int(v))
                break
    if not prot:                                                    # (every router overloaded / non-expandable, or all too wide)
        prot = [int(v) for v in range(nn, n) if len(m.M.candidates(*graph, v).nbr) <= FRR_MAX_SLOTS][:1]
    assert prot, seed
    steps = []
    for i in range(3):
        opt = _frr_options(rng, n)
        opt.chain_root = int(rng.integers(0, len(prot)))
        if i == 0:
            steps.append(FrrStep(seed, 0, graph, maxp, prot, opt))
            continue
        if rng.random() >= 0.6:
            break
        vs = np.sort(rng.choice(n, size=int(rng.integers(1, min(n, 5) + 1)), replace=False))
        rows, fl = [], []
        costs_only = bool(rng.random() < 0.5)
        for v in vs.tolist():
            c = graph[1][graph[0][v]:graph[0][v + 1]]; mm = graph[2][graph[0][v]:graph[0][v + 1]]
            keep = rng.random(len(c)) > (-1.0 if costs_only else 0.25)
            c, mm = c[keep].copy(), mm[keep].copy()
            if len(mm) and (v >= nn or costs_only):
                mm[rng.random(len(mm)) < 0.5] = int(rng.integers(0 if costs_only else 1, 9))
            rows.append((c, mm))
            toggle = v >= nn and v not in prot and not costs_only and rng.random() < 0.3
            fl.append(int(graph[3][v]) ^ (synth.VF_NO_TRANSIT if toggle else 0))
        graph = E.splice_rows(*graph, vs, [c for c, _ in rows], [x for _, x in rows], np.array(fl, np.uint8))
        wide = [r for r in prot if len(m.M.candidates(*graph, r).nbr) > FRR_MAX_SLOTS]
        assert not wide, (seed, i, wide)                             # (a patch only removes links)
        steps.append(FrrStep(seed, i, graph, maxp, prot, opt, m.pm.Patch(vs, rows, fl), costs_only))
    return steps


def frr_compare(want, outs, report):
    """{call: {field: [P, ...]}} of the device (or of anything else) against the expected side; a field that is None was not asked
    for.  report(call, root index, field, first eight differing indices, got there, want there) per difference; returns their count."""
    bad = 0
    for call, fields in outs.items():
        for f, got in fields.items():
            if got is None:
                continue
            w = want[call][f]
            if got.shape != w.shape:
                report(call, -1, f + " (shape)", [], list(got.shape), list(w.shape)); bad += 1
                continue
            for i in range(len(w)):
                if not np.array_equal(got[i], w[i]):
                    idx = np.argwhere(got[i] != w[i])[:8]
                    at = tuple(idx.T)
                    report(call, i, f, idx.tolist(), got[i][at].tolist(), np.asarray(w[i])[at].tolist()); bad += 1
    return bad


def frr_reporter(seed, step, engine, sink=None):
    """report() of frr_compare: one reproducer line per difference."""
    def report(call, root, field, idx, got, want):
        line = f"FRR MISMATCH seed={seed} step={step} engine={engine} call={call} root={root} field={field} idx={idx} got={got} want={want}"
        print(line, flush=True)
        if sink is not None:
            sink.append(line)
    return report


_NP_OF = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}


def _frr_alloc(spec):
    """{name: (shape, 'u8' | 'u16' | 'u32' | 'u64') or None} -> device tensors pre-filled with 7 (None stays None)."""
    import torch
    dt = {"u8": torch.uint8, "u16": torch.int16, "u32": torch.int32, "u64": torch.int64}
    return {k: None if v is None else torch.full(v[0], 7, dtype=dt[v[1]], device="cuda:0") for k, v in spec.items()}, \
           {k: None if v is None else _NP_OF[v[1]] for k, v in spec.items()}


def _frr_host(tensors, dts):
    return {k: None if x is None else x.cpu().numpy().view(dts[k]) for k, x in tensors.items()}


def _ptrs(tensors):
    return {k + "_ptr": 0 if x is None else x.data_ptr() for k, x in tensors.items()}


def frr_device_step(ctx, G, step, report):
    """Every device call of the family on the (patched) handle G, all protected roots in one call, the groups in the drawn order;
    then the chains for the drawn root.  Returns {call: {field: host array}} for frr_compare, or None when the candidate tables
    already differ (reported)."""
    import torch
    m, o, g = _m(), step.opt, step.graph
    roots, per, W = step.plan
    n, R, P, S, NP = len(g[3]), len(roots), len(per), 64 * W, o.pt.n
    protect, lans, no_lans = [], [], []
    for i, (r, c, nr, lan, lr) in enumerate(per):
        pc, pl = E.lfa_candidates(*g, c.root), E.lfa_lan_candidates(*g, c.root)
        same = True
        for f in CAND_FIELDS:
            if not np.array_equal(getattr(pc, f), getattr(c, f)):
                report("lfa_candidates", i, f, [], getattr(pc, f)[:8].tolist(), getattr(c, f)[:8].tolist()); same = False
        if not np.array_equal(pl, lan):
            report("lfa_lan_candidates", i, "lan", [], pl[:8].tolist(), lan[:8].tolist()); same = False
        if not same:
            return None
        protect.append((r, pc, nr)); lans.append((lan, lr)); no_lans.append((np.full(len(lan), m.M.NONE, np.uint32), lr))
    tab, tdt = _frr_alloc(dict(dist=((R, n), "u32"), flags=((R, n), "u16"), mask=((R, n, W), "u64"), rdist=((R, n), "u32")))
    assert G.mask_words(roots) <= W
    ctx.run_device(G, roots, o.run_flags, dist_ptr=tab["dist"].data_ptr(), flags_ptr=tab["flags"].data_ptr(), mask_ptr=tab["mask"].data_ptr(), mask_words=W)
    GT = ctx.upload(*E.csr_transpose(*g), g[3], step.maxp)       # the reverse graph is not under test: a fresh upload per step
    try:
        ctx.run_device(GT, roots, o.run_flags, dist_ptr=tab["rdist"].data_ptr())
    finally:
        GT.free()
    outs = {"run_device": _frr_host(tab, tdt)}
    outs["run_device"]["flags"] = outs["run_device"]["flags"] & 1
    t3 = (tab["dist"].data_ptr(), tab["flags"].data_ptr(), tab["mask"].data_ptr())
    w = step.models
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    alt = up(np.stack([x.alt_flags for x in w["lfa"]])) if o.with_alt else None
    alt_l = up(np.stack([x.alt_flags for x in w["lfa_lan"]])) if o.with_alt else None
    ap = lambda x: 0 if x is None else x.data_ptr()      # noqa: E731
    lf = o.lfa_flags
    safe = m.RL.LAN_SAFE_REPAIRS if o.safe else 0

    def lfa_spec(words, masks):
        mk = ((P, n, W), "u64") if masks else None
        return dict(alt_slot=((P, n), "u32"), alt_metric=((P, n), "u32"), alt_flags=((P, n), "u8"), cand_mask=mk, node_mask=mk, coverage=((P, words), "u32"))

    def rlfa_spec(cw, vw, spaces):
        return dict(pq_node=((P, S), "u32"), pq_via=((P, S), "u32"), pq_metric=((P, S), "u32"), pq_counts=((P, S, cw), "u32"),
                    space_flags=((P, S, n), "u8") if spaces else None, space_via=((P, S, n), "u32") if spaces else None, rl_node=((P, n), "u32"),
                    rl_via=((P, n), "u32"), rl_coverage=((P, vw), "u32"))

    ti_spec = dict(ti_kind=((P, S), "u8"), ti_p=((P, S), "u32"), ti_q=((P, S), "u32"), ti_via=((P, S), "u32"), ti_link=((P, S), "u32"),
                   ti_metric=((P, S), "u32"), ti_counts=((P, S, 2), "u32"), td_kind=((P, n), "u8"), td_coverage=((P, 5), "u32"))

    def lfa_calls(name, lan_cols, masks):
        t, dt = _frr_alloc(lfa_spec(5 if lan_cols is None else 7, masks))
        if lan_cols is None:
            ctx.lfa_device(n, R, W, *t3, protect, lfa_flags=lf, **_ptrs(t))
        else:
            ctx.lfa_lan_device(n, R, W, *t3, protect, lan_cols, lfa_flags=lf, **_ptrs(t))
        outs[name] = _frr_host(t, dt)

    def rlfa_calls(name, lan_cols, alt_in, spaces=True):
        t, dt = _frr_alloc(rlfa_spec(4 if lan_cols is None else 5, 4 if lan_cols is None else 6, spaces))
        head = (G, R, W, *t3, tab["rdist"].data_ptr(), protect)
        if lan_cols is None:
            ctx.rlfa_device(*head, alt_flags_in_ptr=ap(alt_in), lfa_flags=lf, **_ptrs(t))
        else:
            ctx.rlfa_lan_device(*head, lan_cols, alt_flags_in_ptr=ap(alt_in), lfa_flags=lf, **_ptrs(t))
        outs[name] = _frr_host(t, dt)
        return t

    def tilfa_call(name, spaces, alt_in):
        t, dt = _frr_alloc(ti_spec)
        ctx.tilfa_device(G, R, W, *t3, tab["rdist"].data_ptr(), protect, space_flags_ptr=spaces["space_flags"].data_ptr(),
                         space_via_ptr=spaces["space_via"].data_ptr(), alt_flags_in_ptr=ap(alt_in), lfa_flags=lf, **_ptrs(t))
        outs[name] = _frr_host(t, dt)

    def plain_remote():                                             # rlfa, TI-LFA on its tables, the node-protecting pair on its space_flags
        sp = rlfa_calls("rlfa_device", None, alt)
        if not o.spaces:
            rlfa_calls("rlfa_device(no spaces)", None, alt, False)
        after = [lambda: tilfa_call("tilfa_device", sp, alt), lambda: node_calls(sp)]
        for k in ([0, 1] if o.order[0] < o.order[1] else [1, 0]):
            after[k]()

    def node_calls(sp):
        MQ = o.max_pq
        s, sdt = _frr_alloc(dict(nq_node=((P, S, MQ), "u32"), nq_via=((P, S, MQ), "u32"), nq_metric=((P, S, MQ), "u32"), nq_count=((P, S), "u32")))
        ctx.rlfa_node_select_device(n, R, W, *t3, protect, space_flags_ptr=sp["space_flags"].data_ptr(), max_pq=MQ, lfa_flags=lf, **_ptrs(s))
        hs = _frr_host(s, sdt)
        listed = np.unique(hs["nq_node"][hs["nq_node"] != m.N.NONE]).astype(np.uint32)
        y_roots = listed if len(listed) else np.array([m.N.NONE], np.uint32)
        outs["rlfa_node_select_device"] = dict(hs, y_roots=y_roots[None, :])
        if not np.array_equal(y_roots, w["y_roots"]) or (listed >= n).any():
            return                                                  # (reported by the comparison; the second call needs the model's rows)
        ydist = torch.full((len(y_roots), n), 7, dtype=torch.int32, device="cuda:0")
        if len(listed):
            ctx.run_device(G, y_roots, o.run_flags, dist_ptr=ydist.data_ptr())
        d, ddt = _frr_alloc(dict(nd_kind=((P, n), "u8"), nd_node=((P, n), "u32"), nd_via=((P, n), "u32"), nd_metric=((P, n), "u32"),
                                 nd_set=((P, n), "u32"), nd_coverage=((P, 5), "u32")))
        ctx.rlfa_node_device(n, R, W, *t3, protect, ydist_ptr=ydist.data_ptr(), y_roots=y_roots, sel=tuple(s[k].data_ptr() for k in m.N.SEL_FIELDS),
                             max_pq=MQ, alt_flags_in_ptr=ap(alt), **_ptrs(d))
        outs["rlfa_node_device"] = _frr_host(d, ddt)

    def lan_remote():
        sp = rlfa_calls("rlfa_lan_device", lans, alt_l)
        if not o.spaces:
            rlfa_calls("rlfa_lan_device(no spaces)", lans, alt_l, False)
        tilfa_call("tilfa_device(lan tables)", sp, alt_l)

    def backups():
        r, rdt = _frr_alloc(dict(best_metric=((R, NP), "u32"), best_entry=((R, NP), "u32"), nexthop_mask=((R, NP, W), "u64")))
        pt = o.pt
        ctx.routes_device(n, R, W, *t3, pt.ptr, pt.vertex, pt.metric, flags=pt.flags, **_ptrs(r))
        rows = [x for x, *_ in per]
        outs["routes_device"] = {k: v[rows] for k, v in _frr_host(r, rdt).items()}
        routes = tuple(r[k].data_ptr() for k in ROUTE_FIELDS)
        ti_of = lambda key: [up(np.stack([getattr(x, f) for x in w[key]])) for f in ("ti_kind", "ti_via", "ti_metric")]      # noqa: E731
        ti, til = ti_of("tilfa"), ti_of("tilfa_lan" if o.safe else "tilfa")
        calls = [("routes_backup_device", None, ti, o.masks, lf), ("routes_backup_device(no tilfa)", None, None, not o.masks, lf),
                 ("routes_backup_lan_device", lans, til, o.masks_lan, lf | safe), ("routes_backup_lan_device(no tilfa)", lans, None, not o.masks_lan, lf | safe),
                 ("routes_backup_lan_device(no lans)", no_lans, ti, o.masks, lf | safe)]
        for j, k in enumerate(np.argsort(o.order[:5]).tolist()):
            name, lan_cols, tis, masks, flags = calls[k]
            mk = ((P, NP, W), "u64") if masks else None
            b, bdt = _frr_alloc(dict(bk_kind=((P, NP), "u8"), bk_primary=((P, NP), "u32"), bk_slot=((P, NP), "u32"), bk_metric=((P, NP), "u32"),
                                     bk_flags=((P, NP), "u8"), bk_cand_mask=mk, bk_node_mask=mk, bk_coverage=((P, 7 if lan_cols is None else 9), "u32")))
            kw = dict(routes=routes, tilfa=None if tis is None else tuple(x.data_ptr() for x in tis),
                      flags=pt.flags | (m.B.PFX_RESIDENT if o.resident and j else 0), lfa_flags=flags, **_ptrs(b))
            if lan_cols is None:
                ctx.routes_backup_device(n, R, W, *t3, protect, pt.ptr, pt.vertex, pt.metric, **kw)
            else:
                ctx.routes_backup_lan_device(n, R, W, *t3, protect, lan_cols, pt.ptr, pt.vertex, pt.metric, **kw)
            outs[name] = _frr_host(b, bdt)

    def lan_free():
        lfa_calls("lfa_lan_device(no lans)", no_lans, True)
        rlfa_calls("rlfa_lan_device(no lans)", no_lans, alt)

    def chains():
        outs.update(frr_chain_calls(ctx, G, step))

    groups = [lambda: lfa_calls("lfa_device", None, o.masks), lambda: lfa_calls("lfa_lan_device", lans, o.masks_lan), plain_remote, lan_remote, backups,
              lan_free, chains]
    for k in o.order:
        groups[k]()
    torch.cuda.synchronize()
    return outs


def frr_chain_calls(ctx, G, step):
    """SpfContext.lfa / rlfa / tilfa / rlfa_node / backup_routes on the handle for the drawn root: {call: {field: [1, ...]}}."""
    m, o = _m(), step.opt
    root, lf, lp = step.prot[o.chain_root], o.lfa_flags, o.lan_protect
    sym = o.symmetric and not lp
    of = lambda obj, fields: {f: getattr(obj, f) for f in fields}      # noqa: E731
    cand, res = ctx.lfa(G, root, o.run_flags, lfa_flags=lf, want_masks=o.masks, lan_protect=lp)
    out = {"SpfContext.lfa": dict(of(res, LFA_FIELDS), **{f: getattr(cand, f)[None, :] for f in CAND_FIELDS})}
    if lp:
        out["SpfContext.lfa"]["lan"] = res.lan[None, :]
    _, _, rl = ctx.rlfa(G, root, o.run_flags, lfa_flags=lf, want_spaces=True, symmetric=sym, lan_protect=lp)
    out["SpfContext.rlfa"] = of(rl, m.R.FIELDS)
    _, _, rl, ti = ctx.tilfa(G, root, o.run_flags, lfa_flags=lf, symmetric=sym, lan_protect=lp)
    out["SpfContext.tilfa"] = dict(of(rl, m.R.FIELDS), **of(ti, m.T.FIELDS))
    nd = ctx.rlfa_node(G, root, o.run_flags, lfa_flags=lf, max_pq=o.max_pq, symmetric=o.symmetric)
    out["SpfContext.rlfa_node"] = dict(of(nd, m.N.SEL_FIELDS + m.N.DEST_FIELDS), y_roots=nd.y_roots[None, :])
    bk = ctx.backup_routes(G, root, (o.pt.ptr, o.pt.vertex, o.pt.metric, o.pt.flags), o.run_flags, lfa_flags=lf, symmetric=sym, remote=o.remote,
                           lan_protect=lp, lan_repairs=o.lan_repairs)
    out["SpfContext.backup_routes"] = dict(of(bk, ROUTE_FIELDS + m.B.FIELDS), **(of(bk.tilfa, m.T.FIELDS) if o.remote else {}))
    return out


def fuzz_frr(ctx, first, count, verbose=True, patches=True):
    """The fast-reroute family against its models: per seed ONE upload, per step of frr_case(seed) every device call of the family
    with all protected roots in one call (outputs pre-filled with 7, the calls in a drawn order on the one context), the LAN
    calls with every LAN column NONE against the plain calls' answers, and the SpfContext chains for one root — every array
    bit for bit.  patches=False: the first step only.  After a patch the handle's build mode must be the one tests/_patch_model.py
    predicts for the engine configuration.  One run = one (seed, step); a mismatch prints one line per difference and ends the seed."""
    m = _m()
    engine = getattr(ctx, "mode", "default")
    ok = runs = 0
    t0 = time.time()
    for seed in range(first, first + count):
        steps = frr_case(seed)
        steps = steps if patches else steps[:1]
        mdl = m.pm.GraphModel(*steps[0].graph, **FRR_ENGINES.get(engine, {}))
        G = ctx.upload(*steps[0].graph, steps[0].maxp)
        try:
            for step in steps:
                runs += 1
                report = frr_reporter(seed, step.index, engine)
                bad = 0
                if step.patch is not None:
                    want_mode = mdl.step(step.patch).build_mode
                    G.patch(step.patch.vs, step.patch.rows, step.patch.flags)
                    mode = int(G.export("build_mode")[0])
                    if mode != want_mode:
                        report("hspf_graph_patch", -1, "build_mode", [], mode, want_mode); bad += 1
                outs = frr_device_step(ctx, G, step, report)
                if outs is None:
                    break
                for call in set(step.want) | set(step.chain):         # every call ran (the per-destination call needs the model's lists)
                    if call not in outs and not (call.endswith("(no spaces)") and step.opt.spaces):
                        report(call, -1, "not run", [], [], []); bad += 1
                chain = {k: v for k, v in outs.items() if k.startswith("SpfContext.")}
                bad += frr_compare(step.want, {k: v for k, v in outs.items() if k not in chain}, report) + frr_compare(step.chain, chain, report)
                if bad:
                    break
                ok += 1
        finally:
            G.free()
    if verbose:
        print(f"fuzz_frr: {ok}/{runs} (seed, step) runs bit-exact over {count} seeds in {time.time() - t0:.1f} s", flush=True)
    return ok, runs


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    ctx = E.SpfContext(0)
    if os.environ.get("FUZZ_MID"):                                  # only the mid-size graphs (k_xcd's range)
        ok, runs = fuzz_mid(ctx, first, int(os.environ["FUZZ_MID"]))
        sys.exit(0 if ok == runs else 1)
    if os.environ.get("FUZZ_WIDE"):                                 # only the wide-mask graphs
        ok, runs = fuzz_wide(ctx, first, int(os.environ["FUZZ_WIDE"]))
        sys.exit(0 if ok == runs else 1)
    if os.environ.get("FUZZ_FRR"):                                  # only the fast-reroute family against its models
        ok, runs = fuzz_frr(ctx, first, int(os.environ["FUZZ_FRR"]))
        sys.exit(0 if ok == runs else 1)
    ok, runs = fuzz(ctx, first, count)
    ok2, runs2 = fuzz_layout(ctx, first, max(count // 4, 20), spf=bool(os.environ.get("FUZZ_ARBITRARY")))
    ok3, runs3 = fuzz_routes(ctx, first, max(count // 20, 5))
    sys.exit(0 if (ok == runs and ok2 == runs2 and ok3 == runs3) else 1)


if __name__ == "__main__":
    main()
