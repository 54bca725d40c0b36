"""Times hspf_routes_backup_ecmp_device against hspf_routes_backup_device on the SAME resident tables, routes and prefix table.  A
sample is one wall-clock window around `--inner` consecutive C calls with prebuilt arguments, host staging and the call's own
synchronisation included (the figure is the window over `--inner`); the calls are ALTERNATED sample by sample, `--repeats` samples
each after one warm-up call each, so a difference can be held against the plain call's own spread.  The ECMP call is timed as its
second, filling call (cap_entries = the total); the sizing call (cap_entries = 0: count and scan, the fill writes eb_ptr alone) is
timed separately.  tilfa_dev is NULL in both calls; the prefix table is resident after the first call; the plain call writes both
set tables.
    python tools/backup_ecmp_measure.py [--inner 10] [--repeats 9]
Workloads (graphs of holo_amd/synth.py, tables of tools/backup_node_measure.py: one prefix per vertex, then n2 on two vertices):
  mesh     isis-100k, root 50200, 120 000 prefixes — twelve slots, few ECMP prefixes;
  ring     a ring of 20 000 routers, 24 000 prefixes — two slots, next to no ECMP;
  fattree  the k = 16 fat-tree, the first edge switch, one prefix per vertex and 1 000 on two — 8 uplinks, maximal ECMP.
One JSON line per workload: the samples, the medians, the ratio ECMP / plain, each call's spread, the coverage, entries per second."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backup_node_measure import table_of      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")

    def timed(calls):
        samples = {k: [] for k in calls}
        for call in calls.values():
            call()
        for _ in range(args.repeats):
            for k, call in calls.items():
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    call()                                   # (every call synchronises the context's stream itself)
                samples[k].append(round((time.perf_counter() - t0) * 1e3 / args.inner, 4))
        return samples

    def one(name, g, root, n2):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        G = ctx.upload(*graph, g.max_path_metric)
        plan = ctx._frr_plan(G, root)
        cand, roots, W = plan.cand, plan.roots, plan.mask_words
        R, n = len(roots), g.n
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        i64 = lambda *sh: torch.empty(sh, dtype=torch.int64, device=dev)      # noqa: E731
        u8 = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=dev)       # noqa: E731
        dist, flags, mask = i32(R, n), torch.empty((R, n), dtype=torch.int16, device=dev), i64(R, n, W)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        tabs = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        ptr, vtx, met = table_of(n, n2=n2)
        NP = len(ptr) - 1
        bm, be, nh = i32(R, NP), i32(R, NP), i64(R, NP, W)
        ctx.routes_device(n, R, W, *tabs, ptr, vtx, met, best_metric_ptr=bm.data_ptr(), best_entry_ptr=be.data_ptr(), nexthop_mask_ptr=nh.data_ptr())
        arr, keep = ctx._protect_array([(0, cand, plan.nbr_row)], "backup_ecmp_measure")
        u32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))      # noqa: E731
        t = L.HspfPrefixTable(NP, len(vtx), u32p(ptr), u32p(vtx), u32p(met), E.PFX_RESIDENT, None, None, None, None)
        r = L.HspfRoutes(bm.data_ptr(), be.data_ptr(), nh.data_ptr())
        o = [u8(1, NP), i32(1, NP), i32(1, NP), i32(1, NP), u8(1, NP), i64(1, NP, W), i64(1, NP, W), i32(1, E.BK_COVERAGE_WORDS)]
        bo = L.HspfBackupOut(*(x.data_ptr() for x in o))
        eptr = i32(NP + 1)
        total = ctypes.c_uint64()
        ok = lambda rc: rc == 0 or sys.exit(ctx.last_error())      # noqa: E731
        head = (ctx.handle, n, R, W, *tabs, arr, 1, 0, ctypes.byref(t), ctypes.byref(r), None)
        so = L.HspfBackupEcmpOut(eptr.data_ptr(), None, None, None, None, None, None)
        ok(ctx.lib.hspf_routes_backup_ecmp_device(*head, 0, ctypes.byref(so), ctypes.byref(total)))
        T = int(total.value)
        c = max(T, 1)
        e = [i32(c), u8(c), i32(c), i32(c), u8(c), i32(1, E.BK_ECMP_COVERAGE_WORDS)]
        eo = L.HspfBackupEcmpOut(eptr.data_ptr(), *[x.data_ptr() for x in e])
        calls = dict(
            backup_ms=lambda: ok(ctx.lib.hspf_routes_backup_device(*head, ctypes.byref(bo))),
            ecmp_ms=lambda: ok(ctx.lib.hspf_routes_backup_ecmp_device(*head, c, ctypes.byref(eo), ctypes.byref(total))),
            ecmp_size_ms=lambda: ok(ctx.lib.hspf_routes_backup_ecmp_device(*head, 0, ctypes.byref(so), ctypes.byref(total))))
        out = dict(workload=name, n_vertices=n, rows=R, slots=cand.n_slots, n_prefixes=NP, entries=T, inner=args.inner,
                   fill="d_N(p) per (prefix, candidate) into LDS, then lane = (p, h); 2 048 values per batch")
        out.update(timed(calls))
        out["bk_coverage"] = o[7].cpu().numpy().view(np.uint32).ravel().tolist()
        calls["ecmp_ms"]()
        out["eb_coverage"] = e[5].cpu().numpy().view(np.uint32).ravel().tolist()
        for k in calls:
            out[k + "_median"] = round(float(np.median(out[k])), 4)
            out[k + "_spread"] = round(float((max(out[k]) - min(out[k])) / np.median(out[k])), 4)
        out["ecmp_over_plain"] = round(out["ecmp_ms_median"] / out["backup_ms_median"], 4)
        out["entries_per_s"] = round(T / (out["ecmp_ms_median"] * 1e-3)) if T else 0
        print(json.dumps(out), flush=True)
        del keep
        G.free()

    one("mesh: isis-100k, root 50200, 120 000 prefixes", synth.isis_100k(), 50200, 20000)
    nr = 20000
    ring = np.stack([np.arange(nr, dtype=np.int64), (np.arange(nr, dtype=np.int64) + 1) % nr], axis=1)
    one("ring: 20 000 routers, 24 000 prefixes", synth._routers_only(nr, ring, synth.SEED, 1, 100, synth.MAX_PATH_METRIC_WIDE, "ring-20k", {}), 0, 4000)
    ft = synth.isis_fattree(16)
    one("fattree: k = 16, first edge switch, multi-homed prefixes", ft, ft.meta["roots"][0], 1000)
    ctx.close()


if __name__ == "__main__":
    main()
