"""Times hspf_routes_backup_srlg_device against hspf_routes_backup_device on the same resident tables, routes and prefix table.
A sample is one HIP-event window on the context's stream around `--inner` consecutive C calls with prebuilt arguments (the figure
is the window over `--inner`); the plain call and the SRLG call are ALTERNATED sample by sample, `--repeats` samples each after one
warm-up call each, so a difference can be held against the plain call's own spread.
    python tools/backup_srlg_measure.py [--inner 10] [--repeats 9]
Workloads (graphs of holo_amd/synth.py; groups and rows as tools/srlg_measure.py), each at 0, 4 and 16 members per first link of
the root:
  ring  a ring of 20 000 routers, 20 000 single-homed prefixes and 4 000 on two routers;
  mesh  isis-100k, root 50200, with the 120 000-prefix table of bench.py's pipeline_1root (100 000 single-homed, 20 000 on two).
Both calls write both set tables; tilfa_dev is NULL (no per-link repairs: the fallback reads three words per prefix and is the
same in both calls); the prefix table is resident after the first call.
One JSON line per workload and member count: the samples, the medians, the ratio SRLG / plain, each call's spread, the coverage."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from backup_node_measure import table_of      # noqa: E402
from srlg_measure import groups              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))

    def timed(calls):
        samples = {k: [] for k in calls}
        for call in calls.values():
            call()
        for _ in range(args.repeats):
            for k, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.inner):
                    call()
                e1.record(stream); e1.synchronize()
                samples[k].append(round(e0.elapsed_time(e1) / args.inner, 4))
        return samples

    def one(name, g, root, n2):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cand = E.lfa_candidates(*graph, root)
        mems = {m: E.srlg_members(*graph, root, *groups(g, root, m)) for m in (0, 4, 16)}
        ends = {int(v) for v in np.concatenate([mems[16].tail, mems[16].head])}
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
        ftabs = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        ptr, vtx, met = table_of(n, n2=n2)
        NP = len(ptr) - 1
        bm, be, nh = i32(R, NP), i32(R, NP), i64(R, NP, W)
        ctx.routes_device(n, R, W, *ftabs, ptr, vtx, met, best_metric_ptr=bm.data_ptr(), best_entry_ptr=be.data_ptr(), nexthop_mask_ptr=nh.data_ptr())
        protect = [(0, cand, np.array([row_of.get(int(v), 0) for v in cand.nbr], np.uint32))]
        arr, keep = ctx._protect_array(protect, "backup_srlg_measure")
        u32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))      # noqa: E731
        t = L.HspfPrefixTable(NP, len(vtx), u32p(ptr), u32p(vtx), u32p(met), E.PFX_RESIDENT, None, None, None, None)
        r = L.HspfRoutes(bm.data_ptr(), be.data_ptr(), nh.data_ptr())
        o = [u8(1, NP), i32(1, NP), i32(1, NP), i32(1, NP), u8(1, NP), i64(1, NP, W), i64(1, NP, W), i32(1, E.BK_SRLG_COVERAGE_WORDS)]
        out_dev = L.HspfBackupOut(*(x.data_ptr() for x in o))
        ok = lambda rc: rc == 0 or sys.exit(ctx.last_error())      # noqa: E731
        for m, mem in mems.items():
            mem.tail_row = np.array([row_of[int(v)] for v in mem.tail], np.uint32)
            mem.head_row = np.array([row_of[int(v)] for v in mem.head], np.uint32)
            sarr, skeep = ctx._srlg_array([mem], protect, "backup_srlg_measure")
            calls = dict(
                backup_ms=lambda: ok(ctx.lib.hspf_routes_backup_device(ctx.handle, n, R, W, *ftabs, arr, 1, 0, ctypes.byref(t), ctypes.byref(r), None,
                                                                        ctypes.byref(out_dev))),
                backup_srlg_ms=lambda: ok(ctx.lib.hspf_routes_backup_srlg_device(ctx.handle, n, R, W, *ftabs, arr, sarr, 1, 0, ctypes.byref(t), ctypes.byref(r),
                                                                                  None, ctypes.byref(out_dev))))
            out = dict(workload=name, members_per_link=m, n_vertices=n, rows=R, slots=cand.n_slots, n_prefixes=NP, members=int(mem.mem_ptr[-1]),
                       inner=args.inner)
            out.update(timed(calls))                         # (the SRLG call is the last to run: the coverage below is its)
            out["bk_coverage_srlg"] = o[7].cpu().numpy().view(np.uint32).ravel().tolist()
            for k in calls:
                out[k + "_median"] = round(float(np.median(out[k])), 4)
                out[k + "_spread"] = round(float((max(out[k]) - min(out[k])) / np.median(out[k])), 4)
            out["srlg_over_plain"] = round(out["backup_srlg_ms_median"] / out["backup_ms_median"], 4)
            print(json.dumps(out), flush=True)
            del skeep
        del keep
        G.free()

    nr = 20000
    ring = np.stack([np.arange(nr, dtype=np.int64), (np.arange(nr, dtype=np.int64) + 1) % nr], axis=1)
    one("ring: 20 000 routers, 24 000 prefixes", synth._routers_only(nr, ring, synth.SEED, 1, 100, synth.MAX_PATH_METRIC_WIDE, "ring-20k", {}), 0, 4000)
    one("mesh: isis-100k, root 50200, 120 000 prefixes", synth.isis_100k(), 50200, 20000)
    ctx.close()


if __name__ == "__main__":
    main()
