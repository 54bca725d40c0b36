"""Times hspf_routes_backup_ecmp_srlg_device against hspf_routes_backup_ecmp_device on the SAME resident tables, routes and prefix
table, in the manner of tools/backup_ecmp_measure.py: a sample is one wall-clock window around `--inner` consecutive C calls with
prebuilt arguments, host staging and the call's own synchronisation included (the figure is the window over `--inner`); the two
calls are ALTERNATED sample by sample, `--repeats` samples each after one warm-up call each.  Both are timed as the filling call
(cap_entries = the total); tilfa_dev is NULL; the prefix table is resident after the first call.
    python tools/backup_ecmp_srlg_measure.py [--inner 10] [--repeats 9]
Workloads: the three of tools/backup_ecmp_measure.py (mesh isis-100k root 50200, the ring of 20 000 routers, the k = 16 fat-tree's
first edge switch), each with 0 and with 16 members per first link of the root (groups and rows as tools/srlg_measure.py: the table
set also holds the member endpoints' rows, in both calls), and the fat-tree once more with its uplinks grouped two by two (links
2i and 2i + 1 of the root's row in group i: the coverage line of profiles/r28_notes.md).
One JSON line per workload and member table: the samples, the medians, the ratio SRLG / plain, each call's spread, both coverages."""
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
from srlg_measure import groups              # noqa: E402


def uplink_pairs(g, root):
    """(grp_ptr, grp): links 2i and 2i + 1 of the root's row carry group i."""
    rp = g.row_ptr
    per = np.zeros(len(g.col), np.uint32)
    lo, hi = int(rp[root]), int(rp[root + 1])
    per[lo:lo + (hi - lo) // 2 * 2] = 1
    gp = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    return gp, (np.arange((hi - lo) // 2 * 2, dtype=np.uint32) // 2)


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

    def one(name, g, root, n2, pairs=False):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cand = E.lfa_candidates(*graph, root)
        mems = {"uplinks two by two": E.srlg_members(*graph, root, *uplink_pairs(g, root))} if pairs else \
               {str(m) + " per link": E.srlg_members(*graph, root, *groups(g, root, m)) for m in (0, 16)}
        ends = {int(v) for mem in mems.values() for v in np.concatenate([mem.tail, mem.head])}
        rows = [root] + sorted(({int(v) for v in cand.nbr if v != E.NO_ROOT} | ends) - {root})
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        W = max(G.mask_words(roots), (cand.n_slots + 63) // 64)
        R, n = len(rows), g.n
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
        protect = [(0, cand, np.array([row_of.get(int(v), 0) for v in cand.nbr], np.uint32))]
        arr, keep = ctx._protect_array(protect, "backup_ecmp_srlg_measure")
        u32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))      # noqa: E731
        t = L.HspfPrefixTable(NP, len(vtx), u32p(ptr), u32p(vtx), u32p(met), E.PFX_RESIDENT, None, None, None, None)
        r = L.HspfRoutes(bm.data_ptr(), be.data_ptr(), nh.data_ptr())
        eptr = i32(NP + 1)
        total = ctypes.c_uint64()
        ok = lambda rc: rc == 0 or sys.exit(ctx.last_error())      # noqa: E731
        head = (ctx.handle, n, R, W, *tabs, arr)
        tail = (1, 0, ctypes.byref(t), ctypes.byref(r), None)
        so = L.HspfBackupEcmpOut(eptr.data_ptr(), None, None, None, None, None, None)
        ok(ctx.lib.hspf_routes_backup_ecmp_device(*head, *tail, 0, ctypes.byref(so), ctypes.byref(total)))
        T = int(total.value)
        c = max(T, 1)
        ep, es = ([i32(c), u8(c), i32(c), i32(c), u8(c), i32(1, w)] for w in (E.BK_ECMP_COVERAGE_WORDS, E.BK_ECMP_SRLG_COVERAGE_WORDS))
        eo_p = L.HspfBackupEcmpOut(eptr.data_ptr(), *[x.data_ptr() for x in ep])
        eo_s = L.HspfBackupEcmpOut(eptr.data_ptr(), *[x.data_ptr() for x in es])
        for label, mem in mems.items():
            mem.tail_row = np.array([row_of[int(v)] for v in mem.tail], np.uint32)
            mem.head_row = np.array([row_of[int(v)] for v in mem.head], np.uint32)
            sarr, skeep = ctx._srlg_array([mem], protect, "backup_ecmp_srlg_measure")
            calls = dict(
                ecmp_ms=lambda: ok(ctx.lib.hspf_routes_backup_ecmp_device(*head, *tail, c, ctypes.byref(eo_p), ctypes.byref(total))),
                ecmp_srlg_ms=lambda: ok(ctx.lib.hspf_routes_backup_ecmp_srlg_device(*head, sarr, *tail, c, ctypes.byref(eo_s), ctypes.byref(total))))
            out = dict(workload=name, members=label, n_members=int(mem.mem_ptr[-1]), n_vertices=n, rows=R, slots=cand.n_slots, n_prefixes=NP, entries=T,
                       inner=args.inner)
            out.update(timed(calls))
            out["eb_coverage"] = ep[5].cpu().numpy().view(np.uint32).ravel().tolist()
            out["eb_coverage_srlg"] = es[5].cpu().numpy().view(np.uint32).ravel().tolist()
            for k in calls:
                out[k + "_median"] = round(float(np.median(out[k])), 4)
                out[k + "_spread"] = round(float((max(out[k]) - min(out[k])) / np.median(out[k])), 4)
            out["srlg_over_plain"] = round(out["ecmp_srlg_ms_median"] / out["ecmp_ms_median"], 4)
            print(json.dumps(out), flush=True)
            del skeep
        del keep
        G.free()

    one("mesh: isis-100k, root 50200, 120 000 prefixes", synth.isis_100k(), 50200, 20000)
    nr = 20000
    ring = np.stack([np.arange(nr, dtype=np.int64), (np.arange(nr, dtype=np.int64) + 1) % nr], axis=1)
    one("ring: 20 000 routers, 24 000 prefixes", synth._routers_only(nr, ring, synth.SEED, 1, 100, synth.MAX_PATH_METRIC_WIDE, "ring-20k", {}), 0, 4000)
    ft = synth.isis_fattree(16)
    one("fattree: k = 16, first edge switch, multi-homed prefixes", ft, ft.meta["roots"][0], 1000)
    one("fattree: k = 16, first edge switch, multi-homed prefixes", ft, ft.meta["roots"][0], 1000, pairs=True)
    ctx.close()


if __name__ == "__main__":
    main()
