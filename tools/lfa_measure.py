"""Times hspf_lfa_device alone (HIP events on the context's stream around the C call, median; the kernels themselves:
run it under `rocprofv3 --kernel-trace --stats`) against its byte floor, and the path a caller had
before it: the SPT tables copied to the host (hspf_device_to_host) plus the numpy model of tests/_lfa_model.py.
    python tools/lfa_measure.py [--reps 7] [--skip-host]
Workloads: (a) fat-tree k=100, one edge switch, 100 candidates, W = 2, both masks; (b) isis-100k, one root + its neighbours;
(c) isis-100k, the 64 routers of an 8 x 8 block of the grid, rows = the block and every neighbour of it."""
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
    from holo_amd import engine as E, synth
    import _lfa_model as M
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))

    def one(name, g, prot_roots, masks):
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
        protect = [(row_of[r], c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32)) for r, c in zip(prot_roots, cands)]
        slot = torch.empty((P, n), dtype=torch.int32, device=dev); met = torch.empty((P, n), dtype=torch.int32, device=dev)
        fl = torch.empty((P, n), dtype=torch.uint8, device=dev); cov = torch.empty((P, 5), dtype=torch.int32, device=dev)
        cm = torch.empty((P, n, W), dtype=torch.int64, device=dev) if masks else None
        nm = torch.empty((P, n, W), dtype=torch.int64, device=dev) if masks else None

        # the ctypes structures are built once: what is timed is the C call (validation, staging, two kernels, one synchronisation)
        from holo_amd import _lib as L
        keep = [[np.ascontiguousarray(x, dt) for x, dt in ((c.nbr, np.uint32), (nr, np.uint32), (c.cost, np.uint32), (c.root_link, np.uint32), (c.cflags, np.uint8))]
                for _rr, c, nr in protect]
        arr = (L.HspfLfaProtect * P)()
        for i, ((rr, c, _nr), cols) in enumerate(zip(protect, keep)):
            arr[i] = L.HspfLfaProtect(int(c.root), int(rr), len(cols[0]), *(x.ctypes.data_as(L.u32p) for x in cols[:4]), cols[4].ctypes.data_as(L.u8p))
        o = L.HspfLfaOut(slot.data_ptr(), met.data_ptr(), fl.data_ptr(), cm.data_ptr() if masks else None, nm.data_ptr() if masks else None, cov.data_ptr())

        def call():
            rc = ctx.lib.hspf_lfa_device(ctx.handle, n, R, W, dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), arr, P, 0, ctypes.byref(o))
            assert rc == 0, ctx.last_error()
        call()
        ev_ms, wall_ms = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream); call(); e1.record(stream); e1.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3); ev_ms.append(e0.elapsed_time(e1))
        # the floor: every row a protected root needs read once (its own: dist, flags, masks; one dist row per distinct neighbour), outputs written once
        read = sum(n * (4 + 2 + 8 * W) + len({int(v) for v in c.nbr if v != E.NO_ROOT}) * n * 4 for c in cands)
        write = P * n * (4 + 4 + 1 + (16 * W if masks else 0))
        floor_ms = (read + write) / 8e12 * 1e3
        out = dict(case=name, n=n, rows=R, protected=P, W=W, slots=[c.n_slots for c in cands][:4], masks=masks, event_ms_median=float(np.median(ev_ms)),
                   wall_ms_median=float(np.median(wall_ms)), floor_bytes=read + write, floor_ms=floor_ms, fraction_of_floor=floor_ms / float(np.median(ev_ms)),
                   coverage_first=cov.cpu().numpy()[0].tolist())
        if not args.skip_host:
            t0 = time.perf_counter()
            hd, hf, hm = np.empty((R, n), np.uint32), np.empty((R, n), np.uint16), np.empty((R, n, W), np.uint64)
            for a, t in ((hd, dist), (hf, flags), (hm, mask)):
                ctx.lib.hspf_device_to_host(ctx.handle, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(t.data_ptr()), a.nbytes)
            t1 = time.perf_counter()
            ok = True
            for i, (rr, c, nbr_row) in enumerate(protect):
                w = M.lfa(hd, hf, hm, M.Cand(c.root, c.nbr, c.cost, c.root_link, c.cflags), rr, nbr_row)
                if i == 0:
                    ok = bool(np.array_equal(w.alt_slot, slot[0].cpu().numpy().view(np.uint32)) and np.array_equal(w.coverage, cov[0].cpu().numpy().view(np.uint32)))
            t2 = time.perf_counter()
            out.update(host_copy_ms=(t1 - t0) * 1e3, host_copy_bytes=hd.nbytes + hf.nbytes + hm.nbytes, host_model_ms=(t2 - t1) * 1e3, host_equals_device=ok)
        print(json.dumps(out), flush=True)
        G.free()

    ft = synth.isis_fattree(100)
    one("a_fattree_edge_switch", ft, [7500], True)
    g = synth.isis_100k()
    one("b_isis100k_one_root", g, [50200], True)
    block = [r * 400 + c for r in range(100, 108) for c in range(200, 208)]
    one("c_isis100k_64_roots", g, block, False)
    ctx.close()


if __name__ == "__main__":
    main()
