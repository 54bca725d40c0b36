"""Times the two-segment node-protecting chain step by step, wall clock and HIP events on the context's stream around each C call
with prebuilt arguments (median after one warm-up): hspf_tilfa_node_select_device, the hspf_run_device over the union of the listed
q's, hspf_tilfa_node_device — and, in the SAME run on the same tables, hspf_tilfa_device and the two RLFA-node calls, the
yardsticks: the first walks the same rows of the raw CSR, the other two have the same select / evaluate shape.
    python tools/tilfa_node_measure.py [--reps 7] [--max-pairs 16] [--max-pq 16]
Workloads (those of tools/rlfa_node_measure.py): (a) isis-100k, root 50200 + its neighbours; (b) isis-100k, the 64 routers of an
8 x 8 block of the grid, rows = the block and every neighbour of it; (c) fat-tree k=100, one edge switch, 100 slots, W = 2.
`cells_bytes` is the select call's scratch: 8 bytes x (largest n_slots) x n per protected root — it is not tiled."""
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
    ap.add_argument("--max-pairs", type=int, default=16)
    ap.add_argument("--max-pq", type=int, default=16)
    ap.add_argument("--cases", default="abc")
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))
    M, MQ = args.max_pairs, args.max_pq

    def timed(call):
        call()
        ev, wall = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream); call(); e1.record(stream); e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        return dict(event_ms=round(float(np.median(ev)), 4), wall_ms=round(float(np.median(wall)), 4), event_ms_all=[round(x, 4) for x in ev])

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
        arr, keep = ctx._protect_array(protect, "tilfa_node_measure")
        t = dict(pq_node=i32(P, S), pq_via=i32(P, S), pq_metric=i32(P, S), pq_counts=i32(P, S, 4))
        sp_flags, sp_via, rl_node, rl_via, rl_cov = u8(P, S, n), i32(P, S, n), i32(P, n), i32(P, n), i32(P, 4)
        ro = L.HspfRlfaOut(*(t[k].data_ptr() for k in t), sp_flags.data_ptr(), sp_via.data_ptr(), rl_node.data_ptr(), rl_via.data_ptr(), rl_cov.data_ptr())
        rc = ctx.lib.hspf_rlfa_device(ctx.handle, G.handle, n, R, W, *fwd, rdist.data_ptr(), arr, P, 0, fl.data_ptr(), ctypes.byref(ro))
        assert rc == 0, ctx.last_error()
        out = dict(case=name, n=n, rows=R, protected=P, W=W, max_pairs=M, max_pq=MQ, candidates=int(sum((c.nbr != E.NO_ROOT).sum() for c in cands)),
                   cells_bytes=8 * max(c.n_slots for c in cands) * n * P)
        # yardstick 1: hspf_tilfa_device
        ti = dict(ti_kind=u8(P, S), ti_p=i32(P, S), ti_q=i32(P, S), ti_via=i32(P, S), ti_link=i32(P, S), ti_metric=i32(P, S), ti_counts=i32(P, S, 2),
                  td_kind=u8(P, n), td_coverage=i32(P, 5))
        to = L.HspfTilfaOut(*(ti[k].data_ptr() for k in ti))

        def call_tilfa():
            rc = ctx.lib.hspf_tilfa_device(ctx.handle, G.handle, n, R, W, *fwd, rdist.data_ptr(), arr, P, 0, fl.data_ptr(), sp_flags.data_ptr(),
                                           sp_via.data_ptr(), ctypes.byref(to))
            assert rc == 0, ctx.last_error()
        out["tilfa"] = timed(call_tilfa)
        # yardsticks 2 and 3: the RLFA-node pair
        s = dict(nq_node=i32(P, S, MQ), nq_via=i32(P, S, MQ), nq_metric=i32(P, S, MQ), nq_count=i32(P, S))
        so = L.HspfRlfaNodeSel(*(s[k].data_ptr() for k in s))

        def call_nsel():
            rc = ctx.lib.hspf_rlfa_node_select_device(ctx.handle, n, R, W, *fwd, arr, P, 0, sp_flags.data_ptr(), MQ, ctypes.byref(so))
            assert rc == 0, ctx.last_error()
        out["rlfa_node_select"] = timed(call_nsel)

        def y_of(lists):
            y = np.unique(lists[lists != E.NO_ROOT]).astype(np.uint32)
            return y if len(y) else np.array([E.NO_ROOT], np.uint32)
        yn = y_of(s["nq_node"].cpu().numpy().view(np.uint32))
        yndist = i32(len(yn), n)
        ctx.run_device(G, yn, 0, dist_ptr=yndist.data_ptr())
        d = dict(nd_kind=u8(P, n), nd_node=i32(P, n), nd_via=i32(P, n), nd_metric=i32(P, n), nd_set=i32(P, n), nd_coverage=i32(P, 5))
        do = L.HspfRlfaNodeOut(*(d[k].data_ptr() for k in d))
        ynp = yn.ctypes.data_as(L.u32p)

        def call_ndest():
            rc = ctx.lib.hspf_rlfa_node_device(ctx.handle, n, R, W, *fwd, arr, P, yndist.data_ptr(), ynp, len(yn), ctypes.byref(so), MQ, fl.data_ptr(),
                                               ctypes.byref(do))
            assert rc == 0, ctx.last_error()
        out["rlfa_node_dest"] = timed(call_ndest)
        # the new pair
        q = {k: i32(P, S, M) for k in ("tq_q", "tq_p", "tq_link", "tq_via", "tq_metric")}
        q["tq_count"] = i32(P, S)
        qo = L.HspfTilfaNodeSel(*(q[k].data_ptr() for k in q))

        def call_tsel():
            rc = ctx.lib.hspf_tilfa_node_select_device(ctx.handle, G.handle, n, R, W, *fwd, arr, P, 0, sp_flags.data_ptr(), M, ctypes.byref(qo))
            assert rc == 0, ctx.last_error()
        out["tilfa_node_select"] = timed(call_tsel)
        yq = y_of(q["tq_q"].cpu().numpy().view(np.uint32))
        counts = q["tq_count"].cpu().numpy().view(np.uint32)
        yqdist = i32(len(yq), n)
        yr = L.HspfResult(yqdist.data_ptr(), None, None, None, 1, None)
        yqp = yq.ctypes.data_as(L.u32p)

        def call_y():
            rc = ctx.lib.hspf_run_device(ctx.handle, G.handle, yqp, len(yq), 0, ctypes.byref(yr))
            assert rc == 0, ctx.last_error()
        out["q_rows_run"] = timed(call_y)
        tn = dict(tn_kind=u8(P, n), **{k: i32(P, n) for k in ("tn_p", "tn_q", "tn_link", "tn_via", "tn_metric", "tn_set")}, tn_coverage=i32(P, 6))
        tno = L.HspfTilfaNodeOut(*(tn[k].data_ptr() for k in tn))

        def call_tdest():
            rc = ctx.lib.hspf_tilfa_node_device(ctx.handle, n, R, W, *fwd, arr, P, yqdist.data_ptr(), yqp, len(yq), ctypes.byref(qo), M, fl.data_ptr(),
                                                d["nd_kind"].data_ptr(), ctypes.byref(tno))
            assert rc == 0, ctx.last_error()
        out["tilfa_node_dest"] = timed(call_tdest)
        out.update(y_roots_pq=len(yn), y_roots_q=len(yq), tq_count_max=int(counts.max()), tq_count_sum=int(counts.sum()),
                   select_over_tilfa=round(out["tilfa_node_select"]["event_ms"] / out["tilfa"]["event_ms"], 3),
                   select_over_rlfa_node_select=round(out["tilfa_node_select"]["event_ms"] / out["rlfa_node_select"]["event_ms"], 3),
                   dest_over_rlfa_node_dest=round(out["tilfa_node_dest"]["event_ms"] / out["rlfa_node_dest"]["event_ms"], 3),
                   nd_coverage_sum=d["nd_coverage"].cpu().numpy().sum(axis=0).tolist(), tn_coverage_sum=tn["tn_coverage"].cpu().numpy().sum(axis=0).tolist())
        print(json.dumps(out), flush=True)
        del keep
        G.free(); GT.free()

    t0 = time.perf_counter()
    g = synth.isis_100k()
    if "a" in args.cases:
        one("a_isis100k_one_root", g, [50200])
    if "b" in args.cases:
        one("b_isis100k_64_roots", g, [r * 400 + c for r in range(100, 108) for c in range(200, 208)])
    if "c" in args.cases:
        one("c_fattree_edge_switch", synth.isis_fattree(100), [7500])
    print(json.dumps(dict(total_s=time.perf_counter() - t0)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
