"""Times the node-protecting remote LFA chain step by step (HIP events on the context's stream around each C call with prebuilt
arguments, median after one warm-up): hspf_rlfa_node_select_device, the hspf_run_device over the union of the listed nodes (the
Y rows), hspf_rlfa_node_device — and, on the same tables, hspf_rlfa_device itself: the yardstick of the select step, which
evaluates the same family of inequalities over the same rows.  Each step against its byte floor at 8 TB/s.
    python tools/rlfa_node_measure.py [--reps 7] [--max-pq 16]
Workloads (those of tools/tilfa_measure.py): (a) isis-100k, root 50200 + its neighbours; (b) isis-100k, the 64 routers of an
8 x 8 block of the grid, rows = the block and every neighbour of it; (c) fat-tree k=100, one edge switch, 100 slots, W = 2."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-pq", type=int, default=16)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))
    M = args.max_pq

    def timed(call):
        call()
        ev = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream); e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        return float(np.median(ev)), [round(x, 4) for x in ev]

    def one(name, g, prot_roots):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cands = [E.lfa_candidates(*graph, r) for r in prot_roots]
        rows = list(prot_roots) + sorted({int(v) for c in cands for v in c.nbr if v != E.NO_ROOT} - set(prot_roots))
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        W = max(G.mask_words(roots), max((c.n_slots + 63) // 64 for c in cands))
        R, n, P, S = len(rows), g.n, len(prot_roots), 64 * W
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        u8 = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=dev)      # noqa: E731
        dist, rdist = i32(R, n), i32(R, n)
        flags = torch.empty((R, n), dtype=torch.int16, device=dev); mask = torch.empty((R, n, W), dtype=torch.int64, device=dev)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        GT = ctx.upload(*E.csr_transpose(*graph), g.vflags, g.max_path_metric)
        ctx.run_device(GT, roots, 0, dist_ptr=rdist.data_ptr())
        protect = [(row_of[r], c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32)) for r, c in zip(prot_roots, cands)]
        slot, met, fl, cov = i32(P, n), i32(P, n), u8(P, n), i32(P, 5)
        fwd = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        ctx.lfa_device(n, R, W, *fwd, protect, alt_slot_ptr=slot.data_ptr(), alt_metric_ptr=met.data_ptr(), alt_flags_ptr=fl.data_ptr(),
                       coverage_ptr=cov.data_ptr())
        arr, keep = ctx._protect_array(protect, "rlfa_node_measure")
        # the yardstick: hspf_rlfa_device with the space_flags table (space_via is not needed here)
        t = dict(pq_node=i32(P, S), pq_via=i32(P, S), pq_metric=i32(P, S), pq_counts=i32(P, S, 4))
        sp_flags, rl_node, rl_via, rl_cov = u8(P, S, n), i32(P, n), i32(P, n), i32(P, 4)
        ro = L.HspfRlfaOut(*(t[k].data_ptr() for k in t), sp_flags.data_ptr(), None, rl_node.data_ptr(), rl_via.data_ptr(), rl_cov.data_ptr())

        def call_rlfa():
            rc = ctx.lib.hspf_rlfa_device(ctx.handle, G.handle, n, R, W, *fwd, rdist.data_ptr(), arr, P, 0, fl.data_ptr(), ctypes.byref(ro))
            assert rc == 0, ctx.last_error()
        rlfa_ms, rlfa_all = timed(call_rlfa)
        # step 1: the lists
        s = dict(nq_node=i32(P, S, M), nq_via=i32(P, S, M), nq_metric=i32(P, S, M), nq_count=i32(P, S))
        so = L.HspfRlfaNodeSel(*(s[k].data_ptr() for k in s))

        def call_sel():
            rc = ctx.lib.hspf_rlfa_node_select_device(ctx.handle, n, R, W, *fwd, arr, P, 0, sp_flags.data_ptr(), M, ctypes.byref(so))
            assert rc == 0, ctx.last_error()
        sel_ms, sel_all = timed(call_sel)
        nodes = s["nq_node"].cpu().numpy().view(np.uint32)
        counts = s["nq_count"].cpu().numpy().view(np.uint32)
        y_roots = np.unique(nodes[nodes != E.NO_ROOT]).astype(np.uint32)
        if len(y_roots) == 0:
            y_roots = np.array([E.NO_ROOT], np.uint32)
        Y = len(y_roots)
        # step 2: the Y rows (dist only)
        ydist = i32(Y, n)
        yr = L.HspfResult(ydist.data_ptr(), None, None, None, 1, None)
        yp = y_roots.ctypes.data_as(L.u32p)

        def call_y():
            rc = ctx.lib.hspf_run_device(ctx.handle, G.handle, yp, Y, 0, ctypes.byref(yr))
            assert rc == 0, ctx.last_error()
        y_ms, y_all = timed(call_y)
        # step 3: the per-destination test
        d = dict(nd_kind=u8(P, n), nd_node=i32(P, n), nd_via=i32(P, n), nd_metric=i32(P, n), nd_set=i32(P, n), nd_coverage=i32(P, 5))
        do = L.HspfRlfaNodeOut(*(d[k].data_ptr() for k in d))

        def call_dest():
            rc = ctx.lib.hspf_rlfa_node_device(ctx.handle, n, R, W, *fwd, arr, P, ydist.data_ptr(), yp, Y, ctypes.byref(so), M, fl.data_ptr(),
                                               ctypes.byref(do))
            assert rc == 0, ctx.last_error()
        dest_ms, dest_all = timed(call_dest)
        # byte floors.  select: per candidate slot its space_flags row (1 byte per vertex); per protected root every distinct dist row
        # once (S, and each neighbour router as E or as a via); the lists and counts written once.  dest: the root's dist / flags /
        # mask rows and alt_flags, the map, per root the rows of E it reads (at most its distinct neighbours) and of the listed
        # nodes (at most min(Y, slots * max_pq)); the five outputs.  rlfa: as tools/rlfa_measure.py counts it — the same rows of both
        # table sets, the vertex flags, and the space_flags table written.
        n_cand = [int((c.nbr != E.NO_ROOT).sum()) for c in cands]
        n_nbr = [len({int(v) for v in c.nbr if v != E.NO_ROOT}) for c in cands]
        sel_bytes = sum(k * n + (1 + nb) * n * 4 for k, nb in zip(n_cand, n_nbr)) + P * S * (M * 12 + 4)
        dest_bytes = sum(n * (4 + 2 + 8 * W + 1) + nb * n * 4 + min(Y, k * M) * n * 4 for k, nb in zip(n_cand, n_nbr)) + n * 4 + P * n * 17
        rlfa_bytes = sum((1 + nb) * n * 8 + n * (1 + 2 + 8 * W + 1) + k * n + n * 8 for k, nb in zip(n_cand, n_nbr)) + P * S * 28
        fl_ms = lambda b: b / 8e12 * 1e3      # noqa: E731
        out = dict(case=name, n=n, rows=R, protected=P, W=W, max_pq=M, slots=[c.n_slots for c in cands][:4], candidates=sum(n_cand),
                   select_event_ms_median=sel_ms, select_event_ms_all=sel_all, select_floor_bytes=sel_bytes, select_fraction_of_floor=fl_ms(sel_bytes) / sel_ms,
                   y_roots=Y, y_run_event_ms_median=y_ms, y_run_event_ms_all=y_all,
                   dest_event_ms_median=dest_ms, dest_event_ms_all=dest_all, dest_floor_bytes=dest_bytes, dest_fraction_of_floor=fl_ms(dest_bytes) / dest_ms,
                   rlfa_event_ms_median=rlfa_ms, rlfa_event_ms_all=rlfa_all, rlfa_floor_bytes=rlfa_bytes, select_over_rlfa=sel_ms / rlfa_ms,
                   nq_count_max=int(counts.max()), nq_count_sum=int(counts.sum()),
                   rl_coverage_sum=rl_cov.cpu().numpy().sum(axis=0).tolist(), nd_coverage_sum=d["nd_coverage"].cpu().numpy().sum(axis=0).tolist())
        print(json.dumps(out), flush=True)
        del keep
        G.free(); GT.free()

    t0 = time.perf_counter()
    g = synth.isis_100k()
    one("a_isis100k_one_root", g, [50200])
    one("b_isis100k_64_roots", g, [r * 400 + c for r in range(100, 108) for c in range(200, 208)])
    one("c_fattree_edge_switch", synth.isis_fattree(100), [7500])
    print(json.dumps(dict(total_s=time.perf_counter() - t0)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
