"""Times hspf_lfa_ecmp_device against hspf_lfa_device on the SAME resident tables.  A sample is one wall-clock window around
`--inner` consecutive C calls with prebuilt arguments, host staging and the call's own synchronisation included (the figure is the
window over `--inner`); the two calls are ALTERNATED sample by sample, `--repeats` samples each after one warm-up call each, so a
difference can be held against the plain call's own spread.  The ECMP call is timed as its second, filling call (cap_entries =
the total); the sizing call (cap_entries = 0: count and scan, the fill returns at once) is timed separately.
    python tools/lfa_ecmp_measure.py [--inner 10] [--repeats 9]
Workloads (graphs of holo_amd/synth.py):
  mesh     isis-100k, the 8-neighbour grid with chords, root 50200 — twelve slots, few ECMP destinations;
  ring     a ring of 20 000 routers — two slots, one ECMP destination at most;
  fattree  the k = 16 fat-tree, the first edge switch — 8 uplinks, maximal ECMP.
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

    def one(name, g, root):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        G = ctx.upload(*graph, g.max_path_metric)
        plan = ctx._frr_plan(G, root)
        cand, roots, W = plan.cand, plan.roots, plan.mask_words
        R, n = len(roots), g.n
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        dist, flags, mask = i32(R, n), torch.empty((R, n), dtype=torch.int16, device=dev), torch.empty((R, n, W), dtype=torch.int64, device=dev)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        tabs = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        arr, keep = ctx._protect_array([(0, cand, plan.nbr_row)], "lfa_ecmp_measure")
        a = [i32(1, n), i32(1, n), torch.empty((1, n), dtype=torch.uint8, device=dev), i32(1, 5)]
        lo = L.HspfLfaOut(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), None, None, a[3].data_ptr())
        ptr = i32(n + 1)
        total = ctypes.c_uint64()
        ok = lambda rc: rc == 0 or sys.exit(ctx.last_error())      # noqa: E731
        so = L.HspfLfaEcmpOut(ptr.data_ptr(), None, None, None, None, None)
        ok(ctx.lib.hspf_lfa_ecmp_device(ctx.handle, n, R, W, *tabs, arr, 1, 0, 0, ctypes.byref(so), ctypes.byref(total)))
        T = int(total.value)
        e = [i32(max(T, 1)), i32(max(T, 1)), i32(max(T, 1)), torch.empty((max(T, 1),), dtype=torch.uint8, device=dev), i32(1, 7)]
        eo = L.HspfLfaEcmpOut(ptr.data_ptr(), *[t.data_ptr() for t in e])
        calls = dict(
            lfa_ms=lambda: ok(ctx.lib.hspf_lfa_device(ctx.handle, n, R, W, *tabs, arr, 1, 0, ctypes.byref(lo))),
            ecmp_ms=lambda: ok(ctx.lib.hspf_lfa_ecmp_device(ctx.handle, n, R, W, *tabs, arr, 1, 0, max(T, 1), ctypes.byref(eo), ctypes.byref(total))),
            ecmp_size_ms=lambda: ok(ctx.lib.hspf_lfa_ecmp_device(ctx.handle, n, R, W, *tabs, arr, 1, 0, 0, ctypes.byref(so), ctypes.byref(total))))
        out = dict(workload=name, n_vertices=n, rows=R, slots=cand.n_slots, entries=T, inner=args.inner, fill="lane = (D, h), stride 256 per tile")
        out.update(timed(calls))
        out["lfa_coverage"] = a[3].cpu().numpy().view(np.uint32).tolist()
        calls["ecmp_ms"]()
        out["ea_coverage"] = e[4].cpu().numpy().view(np.uint32).tolist()
        for k in calls:
            out[k + "_median"] = round(float(np.median(out[k])), 4)
            out[k + "_spread"] = round(float((max(out[k]) - min(out[k])) / np.median(out[k])), 4)
        out["ecmp_over_lfa"] = round(out["ecmp_ms_median"] / out["lfa_ms_median"], 4)
        out["entries_per_s"] = round(T / (out["ecmp_ms_median"] * 1e-3)) if T else 0
        print(json.dumps(out), flush=True)
        del keep
        G.free()

    one("mesh: isis-100k, root 50200", synth.isis_100k(), 50200)
    nr = 20000
    ring = np.stack([np.arange(nr, dtype=np.int64), (np.arange(nr, dtype=np.int64) + 1) % nr], axis=1)
    one("ring: 20 000 routers", synth._routers_only(nr, ring, synth.SEED, 1, 100, synth.MAX_PATH_METRIC_WIDE, "ring-20k", {}), 0)
    ft = synth.isis_fattree(16)
    one("fattree: k = 16, first edge switch", ft, ft.meta["roots"][0])
    ctx.close()


if __name__ == "__main__":
    main()
