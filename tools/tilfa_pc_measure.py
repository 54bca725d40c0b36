"""Times hspf_tilfa_pc_device next to hspf_tilfa_device on the same inputs (wall clock around the engine call, which synchronises
once at its end; median after one warm-up) and prints the class and adjacency histograms (tp_coverage) of the root.
    python tools/tilfa_pc_measure.py [--reps 7] [--root 50200] [--max-walk 4096]
Workload: isis-100k, one protected root, [root] + its neighbours as the rows, one failure row per candidate slot."""
import argparse
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
    ap.add_argument("--root", type=int, default=50200)
    ap.add_argument("--max-walk", type=int, default=4096)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    g = synth.isis_100k()
    graph = (g.row_ptr, g.col, g.metric, g.vflags)
    G = ctx.upload(*graph, g.max_path_metric)
    cand = E.lfa_candidates(*graph, args.root)
    nbrs = np.unique(cand.nbr[cand.nbr != E.NO_ROOT])
    roots = np.concatenate([[args.root], nbrs]).astype(np.uint32)
    nbr_row = np.zeros(cand.n_slots, np.uint32)
    nbr_row[cand.nbr != E.NO_ROOT] = 1 + np.searchsorted(nbrs, cand.nbr[cand.nbr != E.NO_ROOT])
    W = max(G.mask_words(roots), (cand.n_slots + 63) // 64)
    R, n, S = len(roots), g.n, 64 * W
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
    u8 = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=dev)       # noqa: E731
    dist, rdist, flags, mask = i32(R, n), i32(R, n), torch.empty((R, n), dtype=torch.int16, device=dev), torch.empty((R, n, W), dtype=torch.int64, device=dev)
    ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
    GT = ctx.upload(*E.csr_transpose(*graph), g.vflags, g.max_path_metric)
    ctx.run_device(GT, roots, 0, dist_ptr=rdist.data_ptr())
    protect = [(0, cand, nbr_row)]
    tabs = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), rdist.data_ptr())
    slot, met, fl, cov = i32(1, n), i32(1, n), u8(1, n), i32(1, 5)
    ctx.lfa_device(n, R, W, *tabs[:3], protect, alt_slot_ptr=slot.data_ptr(), alt_metric_ptr=met.data_ptr(), alt_flags_ptr=fl.data_ptr(), coverage_ptr=cov.data_ptr())
    r = dict(pq_node=i32(1, S), pq_via=i32(1, S), pq_metric=i32(1, S), pq_counts=i32(1, S, 4), rl_node=i32(1, n), rl_via=i32(1, n), rl_coverage=i32(1, 4),
             space_flags=u8(1, S, n), space_via=i32(1, S, n))
    ctx.rlfa_device(G, R, W, *tabs, protect, alt_flags_in_ptr=fl.data_ptr(), **{k + "_ptr": x.data_ptr() for k, x in r.items()})
    slots = np.flatnonzero(cand.nbr != E.NO_ROOT)
    pcd = i32(len(slots), n)
    fails = np.stack([np.full(len(slots), E.FAIL_ROOT_LINK, np.uint32), cand.root_link[slots].astype(np.uint32)], axis=1)
    t0 = time.perf_counter()
    ctx.run_failures_device(G, np.full(len(slots), args.root, np.uint32), fails, 0, dist_ptr=pcd.data_ptr())
    fail_ms = (time.perf_counter() - t0) * 1e3
    pc_row = np.full((1, S), E.NO_ROOT, np.uint32)
    pc_row[0, slots] = np.arange(len(slots))
    ti = dict(ti_kind=u8(1, S), ti_p=i32(1, S), ti_q=i32(1, S), ti_via=i32(1, S), ti_link=i32(1, S), ti_metric=i32(1, S), ti_counts=i32(1, S, 2),
              td_kind=u8(1, n), td_coverage=i32(1, 5))
    tp = dict(tp_kind=u8(1, n), tp_p=i32(1, n), tp_via=i32(1, n), tp_q=i32(1, n), tp_n_adj=u8(1, n), tp_hop_pos=i32(1, n, 4), tp_hop_head=i32(1, n, 4),
              tp_metric=i32(1, n), tp_flags=u8(1, n), tp_coverage=i32(1, 12))
    sp = dict(space_flags_ptr=r["space_flags"].data_ptr(), space_via_ptr=r["space_via"].data_ptr(), alt_flags_in_ptr=fl.data_ptr())

    def tilfa():
        ctx.tilfa_device(G, R, W, *tabs, protect, **sp, **{k + "_ptr": x.data_ptr() for k, x in ti.items()})

    def tilfa_pc():
        ctx.tilfa_pc_device(G, R, W, *tabs, protect, **sp, pc_dist_ptr=pcd.data_ptr(), n_pc_rows=len(slots), pc_row=pc_row, max_walk=args.max_walk,
                            **{k + "_ptr": x.data_ptr() for k, x in tp.items()})

    def timed(f):
        f()
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            f()
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms)), [round(x, 3) for x in ms]
    a, b = timed(tilfa), timed(tilfa_pc)
    covp = tp["tp_coverage"].cpu().numpy().view(np.uint32)[0].tolist()
    print(json.dumps(dict(case="isis100k_one_root", root=args.root, n=n, links=len(g.col), candidate_slots=len(slots), max_walk=args.max_walk,
                          run_failures_ms_first_call=fail_ms, tilfa_ms_median=a[0], tilfa_ms_all=a[1], tilfa_pc_ms_median=b[0], tilfa_pc_ms_all=b[1],
                          parent_scratch_bytes=len(slots) * n * 8, td_coverage=ti["td_coverage"].cpu().numpy().view(np.uint32)[0].tolist(),
                          tp_population=covp[0], tp_classes=dict(zip(("lfa", "repair", "none", "long", "lan", "walk"), covp[1:7])),
                          tp_repairs_by_n_adj=covp[7:], on_pc=int(((tp["tp_flags"].cpu().numpy()[0] & E.TIPC_ON_PC) != 0).sum()))), flush=True)
    G.free(); GT.free()
    ctx.close()


if __name__ == "__main__":
    main()
