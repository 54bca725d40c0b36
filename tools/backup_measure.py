"""Times hspf_routes_backup_device alone (HIP events on the context's stream around the C call with prebuilt arguments and a
resident prefix table, median after one warm-up; the kernels themselves: run it under `rocprofv3 --kernel-trace --stats`) against
its byte floor: the route and the table read once, one distance and one flag gather per (candidate slot, entry), the outputs
written once.  No remote fallback (tilfa_dev = NULL: it adds three loads per prefix with one primary).
    python tools/backup_measure.py [--reps 7] [--prefixes 120000] [--dual 0.05]
Workloads: (a) isis-100k, root 50200 + its neighbours, 120 000 prefixes of which 5 % are dual-homed; (b) the same table, eight
protected roots (a 2 x 4 block of the grid) over one table set; (c) fat-tree k=100, one edge switch, 100 slots, W = 2."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def prefix_table(n_vertices, vflags, n_prefixes, dual_share, seed=1):
    """CSR-by-prefix table: every prefix on one router, a share of them on a second one too; entries sorted by vertex."""
    r = np.random.default_rng(seed)
    routers = np.flatnonzero((np.asarray(vflags) & 1) == 0).astype(np.uint32)
    first = r.choice(routers, n_prefixes)
    dual = r.random(n_prefixes) < dual_share
    second = r.choice(routers, n_prefixes)
    dual &= second != first
    ptr = np.zeros(n_prefixes + 1, np.uint32)
    ptr[1:] = np.cumsum(1 + dual.astype(np.uint32))
    vertex = np.empty(int(ptr[-1]), np.uint32)
    lo, hi = np.minimum(first, second), np.maximum(first, second)
    vertex[ptr[:-1]] = np.where(dual, lo, first)
    vertex[ptr[:-1][dual] + 1] = hi[dual]
    metric = r.integers(1, 64, len(vertex)).astype(np.uint32)
    return ptr, vertex, metric, int(dual.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prefixes", type=int, default=120000)
    ap.add_argument("--dual", type=float, default=0.05)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))

    def one(name, g, prot_roots):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cands = [E.lfa_candidates(*graph, r) for r in prot_roots]
        rows = list(prot_roots) + sorted({int(v) for c in cands for v in c.nbr if v != E.NO_ROOT} - set(prot_roots))
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        W = max(G.mask_words(roots), max((c.n_slots + 63) // 64 for c in cands))
        R, n, P = len(rows), g.n, len(prot_roots)
        dist = torch.empty((R, n), dtype=torch.int32, device=dev); flags = torch.empty((R, n), dtype=torch.int16, device=dev)
        mask = torch.empty((R, n, W), dtype=torch.int64, device=dev)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        ptr, vertex, metric, n_dual = prefix_table(n, g.vflags, args.prefixes, args.dual)
        NP = len(ptr) - 1
        bm = torch.empty((R, NP), dtype=torch.int32, device=dev); be = torch.empty((R, NP), dtype=torch.int32, device=dev)
        nm = torch.empty((R, NP, W), dtype=torch.int64, device=dev)
        ctx.routes_device(n, R, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), ptr, vertex, metric, best_metric_ptr=bm.data_ptr(),
                          best_entry_ptr=be.data_ptr(), nexthop_mask_ptr=nm.data_ptr())
        protect = [(row_of[r], c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32)) for r, c in zip(prot_roots, cands)]
        u = {k: torch.empty((P, NP), dtype=torch.int32, device=dev) for k in ("bk_primary", "bk_slot", "bk_metric")}
        u.update(bk_kind=torch.empty((P, NP), dtype=torch.uint8, device=dev), bk_flags=torch.empty((P, NP), dtype=torch.uint8, device=dev),
                 bk_cand_mask=torch.empty((P, NP, W), dtype=torch.int64, device=dev), bk_node_mask=torch.empty((P, NP, W), dtype=torch.int64, device=dev),
                 bk_coverage=torch.empty((P, 7), dtype=torch.int32, device=dev))
        # the ctypes structures are built once: what is timed is the C call (validation, staging of the slot tables, three kernels, one synchronisation)
        arr, keep = ctx._protect_array(protect, "backup_measure")
        t = L.HspfPrefixTable(NP, len(vertex), ptr.ctypes.data_as(L.u32p), vertex.ctypes.data_as(L.u32p), metric.ctypes.data_as(L.u32p), E.PFX_RESIDENT,
                              None, None, None, None)
        ro = L.HspfRoutes(bm.data_ptr(), be.data_ptr(), nm.data_ptr())
        o = L.HspfBackupOut(*(u[k].data_ptr() for k in ("bk_kind", "bk_primary", "bk_slot", "bk_metric", "bk_flags", "bk_cand_mask", "bk_node_mask", "bk_coverage")))

        def call():
            rc = ctx.lib.hspf_routes_backup_device(ctx.handle, n, R, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), arr, P, 0, ctypes.byref(t),
                                                   ctypes.byref(ro), None, ctypes.byref(o))
            assert rc == 0, ctx.last_error()
        call()
        ev_ms, wall_ms = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record(stream); call(); e1.record(stream); e1.synchronize()
            wall_ms.append((time.perf_counter() - w0) * 1e3); ev_ms.append(e0.elapsed_time(e1))
        kinds = u["bk_kind"].cpu().numpy()
        # the floor: per protected root the route (8 + 8 W bytes per prefix) and the table (4 per prefix, 8 per entry), 6 bytes per
        # (candidate slot, entry) of every prefix whose sets are evaluated, the outputs (14 + 16 W bytes per prefix)
        n_cand = [int((c.nbr != E.NO_ROOT).sum()) for c in cands]
        evaluated = [int(np.diff(ptr)[kinds[i] >= 2].sum()) for i in range(P)]
        read = sum(NP * (8 + 8 * W + 4) + len(vertex) * 8 + k * e * 6 for k, e in zip(n_cand, evaluated))
        write = P * (NP * (14 + 16 * W) + 28)
        floor_ms = (read + write) / 8e12 * 1e3
        print(json.dumps(dict(case=name, n=n, rows=R, protected=P, W=W, prefixes=NP, dual_homed=n_dual, slots=[c.n_slots for c in cands][:4],
                              event_ms_median=float(np.median(ev_ms)), event_ms_all=[round(x, 4) for x in ev_ms], wall_ms_median=float(np.median(wall_ms)),
                              floor_bytes=read + write, floor_ms=floor_ms, fraction_of_floor=floor_ms / float(np.median(ev_ms)),
                              coverage_first=u["bk_coverage"].cpu().numpy()[0].tolist(), coverage_sum=u["bk_coverage"].cpu().numpy().sum(axis=0).tolist())), flush=True)
        del keep
        G.free()

    g = synth.isis_100k()
    one("a_isis100k_one_root", g, [50200])
    one("b_isis100k_8_roots", g, [r * 400 + c for r in range(100, 102) for c in range(200, 204)])
    one("c_fattree_edge_switch", synth.isis_fattree(100), [7500])
    ctx.close()


if __name__ == "__main__":
    main()
