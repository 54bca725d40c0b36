"""Times hspf_tilfa_device alone (HIP events on the context's stream around the C call with prebuilt arguments, median after one
warm-up; the kernels themselves: run it under `rocprofv3 --kernel-trace --stats`) against its byte floor, and the path a caller has
without it: the tables and the space tables copied to the host (hspf_device_to_host) plus the Python model of
tests/_tilfa_model.py, results compared equal.  Reports td_coverage next to rl_coverage: how much of RLFA's remainder closes.
    python tools/tilfa_measure.py [--reps 7] [--skip-host]
Workloads: (a) isis-100k, root 50200 + its 12 neighbours; (b) isis-100k, the 64 routers of an 8 x 8 block of the grid, rows = the
block and every neighbour of it; (c) fat-tree k=100, one edge switch, 100 slots, W = 2."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    import _lfa_model as M
    import _rlfa_model as RM
    import _tilfa_model as TM
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
        R, n, P, S = len(rows), g.n, len(prot_roots), 64 * W
        dist = torch.empty((R, n), dtype=torch.int32, device=dev); flags = torch.empty((R, n), dtype=torch.int16, device=dev)
        mask = torch.empty((R, n, W), dtype=torch.int64, device=dev); rdist = torch.empty((R, n), dtype=torch.int32, device=dev)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        tr = E.csr_transpose(*graph)
        GT = ctx.upload(*tr, g.vflags, g.max_path_metric)
        ctx.run_device(GT, roots, 0, dist_ptr=rdist.data_ptr())
        protect = [(row_of[r], c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32)) for r, c in zip(prot_roots, cands)]
        slot = torch.empty((P, n), dtype=torch.int32, device=dev); met = torch.empty((P, n), dtype=torch.int32, device=dev)
        fl = torch.empty((P, n), dtype=torch.uint8, device=dev); cov = torch.empty((P, 5), dtype=torch.int32, device=dev)
        ctx.lfa_device(n, R, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), protect, alt_slot_ptr=slot.data_ptr(), alt_metric_ptr=met.data_ptr(),
                       alt_flags_ptr=fl.data_ptr(), coverage_ptr=cov.data_ptr())
        t = {k: torch.empty(sh, dtype=torch.int32, device=dev) for k, sh in dict(pq_node=(P, S), pq_via=(P, S), pq_metric=(P, S), pq_counts=(P, S, 4),
                                                                                rl_node=(P, n), rl_via=(P, n), rl_cov=(P, 4), sp_via=(P, S, n)).items()}
        sp_flags = torch.empty((P, S, n), dtype=torch.uint8, device=dev)
        ctx.rlfa_device(G, R, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), rdist.data_ptr(), protect, pq_node_ptr=t["pq_node"].data_ptr(),
                        pq_via_ptr=t["pq_via"].data_ptr(), pq_metric_ptr=t["pq_metric"].data_ptr(), pq_counts_ptr=t["pq_counts"].data_ptr(),
                        rl_node_ptr=t["rl_node"].data_ptr(), rl_via_ptr=t["rl_via"].data_ptr(), rl_coverage_ptr=t["rl_cov"].data_ptr(),
                        space_flags_ptr=sp_flags.data_ptr(), space_via_ptr=t["sp_via"].data_ptr(), alt_flags_in_ptr=fl.data_ptr())
        u = {k: torch.empty(sh, dtype=torch.int32, device=dev) for k, sh in dict(ti_p=(P, S), ti_q=(P, S), ti_via=(P, S), ti_link=(P, S), ti_metric=(P, S),
                                                                                ti_counts=(P, S, 2), td_coverage=(P, 5)).items()}
        u.update(ti_kind=torch.empty((P, S), dtype=torch.uint8, device=dev), td_kind=torch.empty((P, n), dtype=torch.uint8, device=dev))
        # the ctypes structures are built once: what is timed is the C call (validation, staging, three kernels, one synchronisation)
        arr, keep = ctx._protect_array(protect, "tilfa_measure")
        o = L.HspfTilfaOut(*(u[k].data_ptr() for k in TM.FIELDS))

        def call():
            rc = ctx.lib.hspf_tilfa_device(ctx.handle, G.handle, n, R, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), rdist.data_ptr(), arr, P, 0,
                                           fl.data_ptr(), sp_flags.data_ptr(), t["sp_via"].data_ptr(), ctypes.byref(o))
            assert rc == 0, ctx.last_error()
        call()
        ev_ms, wall_ms = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record(stream); call(); e1.record(stream); e1.synchronize()
            wall_ms.append((time.perf_counter() - w0) * 1e3); ev_ms.append(e0.elapsed_time(e1))
        # the floor: per protected root and candidate slot the two space rows (5 bytes per vertex), once the raw CSR with its two-way
        # bytes (9 bytes per link + 4 per vertex), one dist row per distinct via and one rdist row per slot, the root's own dist /
        # flags / mask rows and the given alt_flags for the destination pass; the outputs written once
        n_cand = [int((c.nbr != E.NO_ROOT).sum()) for c in cands]
        e_links = len(g.col)
        read = sum(k * n * 5 + k * n * 4 + len({int(v) for v in c.nbr if v != E.NO_ROOT}) * n * 4 + n * (4 + 2 + 8 * W + 1) for k, c in zip(n_cand, cands)) + \
            e_links * 9 + (n + 1) * 4
        write = P * (n + S * (1 + 20 + 8) + 20)
        floor_ms = (read + write) / 8e12 * 1e3
        out = dict(case=name, n=n, links=e_links, rows=R, protected=P, W=W, slots=[c.n_slots for c in cands][:4], event_ms_median=float(np.median(ev_ms)),
                   event_ms_all=[round(x, 4) for x in ev_ms], wall_ms_median=float(np.median(wall_ms)), floor_bytes=read + write, floor_ms=floor_ms,
                   fraction_of_floor=floor_ms / float(np.median(ev_ms)), rl_coverage_first=t["rl_cov"].cpu().numpy()[0].tolist(),
                   td_coverage_first=u["td_coverage"].cpu().numpy()[0].tolist(), rl_coverage_sum=t["rl_cov"].cpu().numpy().sum(axis=0).tolist(),
                   td_coverage_sum=u["td_coverage"].cpu().numpy().sum(axis=0).tolist(),
                   max_pairs_per_slot=int(u["ti_counts"].cpu().numpy()[:, :, 1].max()))
        if not args.skip_host:
            h0 = time.perf_counter()
            hd, hr, hf, hm = np.empty((R, n), np.uint32), np.empty((R, n), np.uint32), np.empty((R, n), np.uint16), np.empty((R, n, W), np.uint64)
            hsf, hsv = np.empty((P, S, n), np.uint8), np.empty((P, S, n), np.uint32)
            for a, x in ((hd, dist), (hr, rdist), (hf, flags), (hm, mask), (hsf, sp_flags), (hsv, t["sp_via"])):
                ctx.lib.hspf_device_to_host(ctx.handle, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(x.data_ptr()), a.nbytes)
            h1 = time.perf_counter()
            nbytes = sum(a.nbytes for a in (hd, hr, hf, hm, hsf, hsv))
            rr, c, nbr_row = protect[0]                       # the model is timed for ONE protected root and scaled
            if c.n_slots * n > 1e6:                           # a Python loop over slots x vertices x links: minutes; the copy alone is reported
                out.update(host_copy_ms=(h1 - h0) * 1e3, host_copy_bytes=nbytes, host_model_skipped=True)
                print(json.dumps(out), flush=True)
                G.free(); GT.free()
                return
            mc = M.Cand(c.root, c.nbr, c.cost, c.root_link, c.cflags)
            alt = fl.cpu().numpy()[0]
            m0 = time.perf_counter()
            w = TM.tilfa(hd, hf, hm, hr, graph, mc, rr, nbr_row, hsf[0], hsv[0], alt)
            m1 = time.perf_counter()
            got = {k: x[0].cpu().numpy().view(np.uint8 if x.dtype == torch.uint8 else np.uint32) for k, x in u.items()}
            ok = all(np.array_equal(got[k], getattr(w, k)) for k in TM.FIELDS)
            out.update(host_copy_ms=(h1 - h0) * 1e3, host_copy_bytes=nbytes, host_model_ms_one_root=(m1 - m0) * 1e3,
                       host_model_ms_scaled=(m1 - m0) * 1e3 * P, host_equals_device=bool(ok))
        print(json.dumps(out), flush=True)
        del keep
        G.free(); GT.free()

    g = synth.isis_100k()
    one("a_isis100k_one_root", g, [50200])
    block = [r * 400 + c for r in range(100, 108) for c in range(200, 208)]
    one("b_isis100k_64_roots", g, block)
    ft = synth.isis_fattree(100)
    one("c_fattree_edge_switch", ft, [7500])
    ctx.close()


if __name__ == "__main__":
    main()
