"""Times hspf_routes_backup_node_device against hspf_routes_backup_device on the same tables, wall clock and HIP events on the
context's stream around each C call with prebuilt arguments (median after one warm-up), and — separately — the hspf_run_device
over the union of the listed nodes that the new call needs.
    python tools/backup_node_measure.py [--reps 7] [--max-pq 16] [--max-pairs 16]
Workloads: (a) isis-100k, root 50200, with the 120 000-prefix table of bench.py's pipeline_1root (100 000 single-homed prefixes,
20 000 with two owners; the same seed); (c) fat-tree k=100, one edge switch (100 slots, W = 2), a table of that recipe over its
vertices.  `gathers_ratio` is the number of ydist / dist gathers per advertiser of the new call (the listed entries of the lane's
primary slot, both lists, + 1 for d_E(p)) over the plain call's (the candidate slots + 1), averaged over the prefixes with one
primary."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table_of(n, seed=12, n2=20000):
    """bench.py pipeline_1root's table: prefixes 0 .. n-1 with one owner each, then n2 with two owners."""
    rng = np.random.default_rng(seed)
    two = np.sort(rng.integers(0, n, (n2, 2)), axis=1)
    two[:, 1] = np.where(two[:, 1] == two[:, 0], (two[:, 0] + 1) % n, two[:, 1]); two.sort(axis=1)
    vtx = np.concatenate([np.arange(n), two.reshape(-1)]).astype(np.uint32)
    ptr = np.concatenate([np.arange(n), n + 2 * np.arange(n2 + 1)]).astype(np.uint32)
    met = np.concatenate([np.arange(n) % 7, rng.integers(0, 10, 2 * n2)]).astype(np.uint32)
    return ptr, vtx, met


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-pairs", type=int, default=16)
    ap.add_argument("--max-pq", type=int, default=16)
    ap.add_argument("--cases", default="ac")
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

    def one(name, g, root):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        c = E.lfa_candidates(*graph, root)
        rows = [root] + sorted({int(v) for v in c.nbr if v != E.NO_ROOT} - {root})
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        W = max(G.mask_words(roots), (c.n_slots + 63) // 64)
        R, n, S = len(rows), g.n, 64 * W
        ptr, vtx, met = table_of(n)
        NP = len(ptr) - 1
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        u8 = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=dev)      # noqa: E731
        dist, rdist = i32(R, n), i32(R, n)
        flags = torch.empty((R, n), dtype=torch.int16, device=dev); mask = torch.empty((R, n, W), dtype=torch.int64, device=dev)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        GT = ctx.upload(*E.csr_transpose(*graph), g.vflags, g.max_path_metric)
        ctx.run_device(GT, roots, 0, dist_ptr=rdist.data_ptr())
        protect = [(0, c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32))]
        fwd = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        slot, ame, fl, cov = i32(1, n), i32(1, n), u8(1, n), i32(1, 5)
        ctx.lfa_device(n, R, W, *fwd, protect, alt_slot_ptr=slot.data_ptr(), alt_metric_ptr=ame.data_ptr(), alt_flags_ptr=fl.data_ptr(), coverage_ptr=cov.data_ptr())
        rl = dict(pq_node=i32(1, S), pq_via=i32(1, S), pq_metric=i32(1, S), pq_counts=i32(1, S, 4), space_flags=u8(1, S, n), space_via=i32(1, S, n),
                  rl_node=i32(1, n), rl_via=i32(1, n), rl_coverage=i32(1, 4))
        ctx.rlfa_device(G, R, W, *fwd, rdist.data_ptr(), protect, alt_flags_in_ptr=fl.data_ptr(), **{k + "_ptr": x.data_ptr() for k, x in rl.items()})
        ti = dict(ti_kind=u8(1, S), ti_p=i32(1, S), ti_q=i32(1, S), ti_via=i32(1, S), ti_link=i32(1, S), ti_metric=i32(1, S), ti_counts=i32(1, S, 2),
                  td_kind=u8(1, n), td_coverage=i32(1, 5))
        ctx.tilfa_device(G, R, W, *fwd, rdist.data_ptr(), protect, space_flags_ptr=rl["space_flags"].data_ptr(), space_via_ptr=rl["space_via"].data_ptr(),
                         alt_flags_in_ptr=fl.data_ptr(), **{k + "_ptr": x.data_ptr() for k, x in ti.items()})
        ro = dict(best_metric=i32(1, NP), best_entry=i32(1, NP), nexthop_mask=torch.empty((1, NP, W), dtype=torch.int64, device=dev))
        ctx.routes_device(n, 1, W, *fwd, ptr, vtx, met, **{k + "_ptr": x.data_ptr() for k, x in ro.items()})
        rn = dict(nq_node=i32(1, S, MQ), nq_via=i32(1, S, MQ), nq_metric=i32(1, S, MQ), nq_count=i32(1, S))
        ctx.rlfa_node_select_device(n, R, W, *fwd, protect, space_flags_ptr=rl["space_flags"].data_ptr(), max_pq=MQ, **{k + "_ptr": x.data_ptr() for k, x in rn.items()})
        tq = {k: i32(1, S, M) for k in ("tq_q", "tq_p", "tq_link", "tq_via", "tq_metric")}
        tq["tq_count"] = i32(1, S)
        ctx.tilfa_node_select_device(G, R, W, *fwd, protect, space_flags_ptr=rl["space_flags"].data_ptr(), max_pairs=M, **{k + "_ptr": x.data_ptr() for k, x in tq.items()})
        listed = np.concatenate([rn["nq_node"].cpu().numpy().view(np.uint32).ravel(), tq["tq_q"].cpu().numpy().view(np.uint32).ravel()])
        y = np.unique(listed[listed != E.NO_ROOT]).astype(np.uint32)
        y = y if len(y) else np.array([E.NO_ROOT], np.uint32)
        ydist = i32(len(y), n)
        yr, yp = L.HspfResult(ydist.data_ptr(), None, None, None, 1, None), y.ctypes.data_as(L.u32p)

        def call_y():
            rc = ctx.lib.hspf_run_device(ctx.handle, G.handle, yp, len(y), 0, ctypes.byref(yr))
            assert rc == 0, ctx.last_error()
        out = dict(case=name, n=n, rows=R, W=W, n_prefixes=NP, max_pq=MQ, max_pairs=M, candidates=int((c.nbr != E.NO_ROOT).sum()), y_rows=len(y))
        if y[0] != E.NO_ROOT:
            out["listed_rows_run"] = timed(call_y)
        arr, keep = ctx._protect_array(protect, "backup_node_measure")
        t = L.HspfPrefixTable(NP, len(vtx), ptr.ctypes.data_as(L.u32p), vtx.ctypes.data_as(L.u32p), met.ctypes.data_as(L.u32p), E.PFX_RESIDENT, None, None, None, None)
        r = L.HspfRoutes(*(ro[k].data_ptr() for k in ro))
        bk = dict(bk_kind=u8(1, NP), bk_primary=i32(1, NP), bk_slot=i32(1, NP), bk_metric=i32(1, NP), bk_flags=u8(1, NP),
                  bk_cand_mask=torch.empty((1, NP, W), dtype=torch.int64, device=dev), bk_node_mask=torch.empty((1, NP, W), dtype=torch.int64, device=dev),
                  bk_coverage=i32(1, 7))
        bo = L.HspfBackupOut(*(bk[k].data_ptr() for k in bk))
        tio = L.HspfTilfaOut(ti["ti_kind"].data_ptr(), None, None, ti["ti_via"].data_ptr(), None, ti["ti_metric"].data_ptr(), None, None, None)

        def call_bk():
            rc = ctx.lib.hspf_routes_backup_device(ctx.handle, n, R, W, *fwd, arr, 1, 0, ctypes.byref(t), ctypes.byref(r), ctypes.byref(tio), ctypes.byref(bo))
            assert rc == 0, ctx.last_error()
        out["routes_backup"] = timed(call_bk)
        bn = dict(bn_kind=u8(1, NP), **{k: i32(1, NP) for k in ("bn_primary", "bn_p", "bn_q", "bn_link", "bn_via", "bn_metric", "bn_set_pq", "bn_set_pair")},
                  bn_coverage=i32(1, 6))
        bno = L.HspfBackupNodeOut(*(bn[k].data_ptr() for k in bn))
        rno, tqo = L.HspfRlfaNodeSel(*(rn[k].data_ptr() for k in rn)), L.HspfTilfaNodeSel(*(tq[k].data_ptr() for k in tq))

        def call_bn(with_bk):
            def f():
                rc = ctx.lib.hspf_routes_backup_node_device(ctx.handle, n, R, W, *fwd, arr, 1, ctypes.byref(t), ctypes.byref(r), ydist.data_ptr(), yp, len(y),
                                                            ctypes.byref(rno), MQ, ctypes.byref(tqo), M, ctypes.byref(bo) if with_bk else None, ctypes.byref(bno))
                assert rc == 0, ctx.last_error()
            return f
        bno_bare = L.HspfBackupNodeOut(*(None if k.startswith("bn_set") else bn[k].data_ptr() for k in bn))

        def call_bare():                                # bk_in NULL, both set tables NULL: a chosen PQ entry ends the prefix's work
            rc = ctx.lib.hspf_routes_backup_node_device(ctx.handle, n, R, W, *fwd, arr, 1, ctypes.byref(t), ctypes.byref(r), ydist.data_ptr(), yp, len(y),
                                                        ctypes.byref(rno), MQ, ctypes.byref(tqo), M, None, ctypes.byref(bno_bare))
            assert rc == 0, ctx.last_error()
        out["routes_backup_node_no_bk_in_no_sets"] = timed(call_bare)
        out["routes_backup_node_no_bk_in"] = timed(call_bn(False))
        cov_no_bk = bn["bn_coverage"].cpu().numpy()[0].tolist()
        out["routes_backup_node"] = timed(call_bn(True))
        prim = bn["bn_primary"].cpu().numpy().view(np.uint32)[0]
        one_p = prim != E.LFA_NO_SLOT
        nqc = np.minimum(rn["nq_count"].cpu().numpy().view(np.uint32)[0], MQ).astype(np.int64)
        tqc = np.minimum(tq["tq_count"].cpu().numpy().view(np.uint32)[0], M).astype(np.int64)
        per = (nqc + tqc)[prim[one_p]] + 1            # with the set tables given: both lists are walked whatever the first one finds
        out.update(bn_coverage=bn["bn_coverage"].cpu().numpy()[0].tolist(), bn_coverage_no_bk_in=cov_no_bk, bk_coverage=bk["bk_coverage"].cpu().numpy()[0].tolist(),
                   gathers_per_advertiser_no_bk_in=round(float(per.mean()), 2) if one_p.any() else 0.0, gathers_per_advertiser_plain=out["candidates"] + 1,
                   node_over_plain=round(out["routes_backup_node"]["event_ms"] / out["routes_backup"]["event_ms"], 3),
                   node_no_bk_in_no_sets_over_plain=round(out["routes_backup_node_no_bk_in_no_sets"]["event_ms"] / out["routes_backup"]["event_ms"], 3),
                   node_no_bk_in_over_plain=round(out["routes_backup_node_no_bk_in"]["event_ms"] / out["routes_backup"]["event_ms"], 3))
        print(json.dumps(out), flush=True)
        del keep
        G.free(); GT.free()

    t0 = time.perf_counter()
    if "a" in args.cases:
        one("a_isis100k_one_root", synth.isis_100k(), 50200)
    if "c" in args.cases:
        one("c_fattree_edge_switch", synth.isis_fattree(100), 7500)
    print(json.dumps(dict(total_s=time.perf_counter() - t0)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
