"""Times hspf_rlfa_srlg_device against hspf_rlfa_device, and hspf_lfa_srlg_device against hspf_lfa_device, on the same resident
tables.  A sample is one HIP-event window on the context's stream around `--inner` consecutive C calls with prebuilt arguments
(the figure is the window over `--inner`); the plain call and the SRLG call are ALTERNATED sample by sample, `--repeats` samples
each after one warm-up call each, so a difference can be held against the plain call's own spread.
    python tools/srlg_measure.py [--inner 10] [--repeats 9]
Workloads (graphs of holo_amd/synth.py), each at 0, 4 and 16 members per first link of the root:
  ring  a ring of 20 000 routers (synth's router-only costs) — two slots, sparse Q-spaces;
  mesh  isis-100k, the 8-neighbour grid with chords, root 50200 — eight or more slots, dense Q-spaces.
The members of a link are the first links, in row order, of the routers found breadth-first from the root (the root itself left
out): near the root, so that they lie on shortest paths.  The rows of every variant are [root] + neighbours + the endpoints of
the 16-member variant, so the three variants and the plain call read the same table set.
One JSON line per workload and member count: the samples, the medians, the ratios SRLG / plain and each call's spread."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def near_links(g, root, count):
    """`count` link positions near `root`: the rows of the routers in breadth-first order from the root, the root's own row left out."""
    seen, order, out = {root}, [root], []
    for u in order:
        for l in range(int(g.row_ptr[u]), int(g.row_ptr[u + 1])):
            v = int(g.col[l])
            if u != root:
                out.append(l)
                if len(out) == count:
                    return out
            if v not in seen:
                seen.add(v)
                order.append(v)
    return out


def groups(g, root, per_link):
    """(grp_ptr, grp): link j of the root's row is in group j with `per_link` links of its own near the root."""
    own = int(g.row_ptr[root + 1] - g.row_ptr[root])
    pool = near_links(g, root, own * per_link) if per_link else []
    of = {int(g.row_ptr[root]) + j: [j] for j in range(own)} if per_link else {}
    for i, l in enumerate(pool):
        of.setdefault(l, []).append(i // per_link)
    ptr, ids = [0], []
    for l in range(len(g.col)):
        ids += of.get(l, [])
        ptr.append(len(ids))
    return np.array(ptr, np.uint32), np.array(ids, np.uint32)


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

    def one(name, g, root):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cand = E.lfa_candidates(*graph, root)
        mems = {m: E.srlg_members(*graph, root, *groups(g, root, m)) for m in (0, 4, 16)}
        ends = {int(v) for v in np.concatenate([mems[16].tail, mems[16].head])}
        rows = [root] + sorted(({int(v) for v in cand.nbr if v != E.NO_ROOT} | ends) - {root})
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        GT = ctx.upload(*E.csr_transpose(*graph), g.vflags, g.max_path_metric)
        W = max(G.mask_words(roots), (cand.n_slots + 63) // 64)
        R, n, S = len(rows), g.n, 64 * W
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        dist, flags, mask, rdist = i32(R, n), torch.empty((R, n), dtype=torch.int16, device=dev), torch.empty((R, n, W), dtype=torch.int64, device=dev), i32(R, n)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        ctx.run_device(GT, roots, 0, dist_ptr=rdist.data_ptr())
        ftabs = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        protect = [(0, cand, np.array([row_of.get(int(v), 0) for v in cand.nbr], np.uint32))]
        arr, keep = ctx._protect_array(protect, "srlg_measure")
        sf, sv = torch.empty((1, S, n), dtype=torch.uint8, device=dev), i32(1, S, n)
        b = [i32(1, S), i32(1, S), i32(1, S), i32(1, S, 5), i32(1, n), i32(1, n), i32(1, 6)]
        ro = L.HspfRlfaOut(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), sf.data_ptr(), sv.data_ptr(), b[4].data_ptr(),
                           b[5].data_ptr(), b[6].data_ptr())
        a = [i32(1, n), i32(1, n), torch.empty((1, n), dtype=torch.uint8, device=dev), i32(1, 7)]
        lo = L.HspfLfaOut(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), None, None, a[3].data_ptr())
        for m, mem in mems.items():
            mem.tail_row = np.array([row_of[int(v)] for v in mem.tail], np.uint32)
            mem.head_row = np.array([row_of[int(v)] for v in mem.head], np.uint32)
            sarr, skeep = ctx._srlg_array([mem], protect, "srlg_measure")
            ok = lambda rc: rc == 0 or sys.exit(ctx.last_error())      # noqa: E731
            calls = dict(
                rlfa_ms=lambda: ok(ctx.lib.hspf_rlfa_device(ctx.handle, G.handle, n, R, W, *ftabs, rdist.data_ptr(), arr, 1, 0, None, ctypes.byref(ro))),
                rlfa_srlg_ms=lambda: ok(ctx.lib.hspf_rlfa_srlg_device(ctx.handle, G.handle, n, R, W, *ftabs, rdist.data_ptr(), arr, sarr, 1, 0, None, ctypes.byref(ro))),
                lfa_ms=lambda: ok(ctx.lib.hspf_lfa_device(ctx.handle, n, R, W, *ftabs, arr, 1, 0, ctypes.byref(lo))),
                lfa_srlg_ms=lambda: ok(ctx.lib.hspf_lfa_srlg_device(ctx.handle, n, R, W, *ftabs, arr, sarr, 1, 0, ctypes.byref(lo))))
            out = dict(workload=name, members_per_link=m, n_vertices=n, rows=R, slots=cand.n_slots, members=int(mem.mem_ptr[-1]), inner=args.inner)
            out.update(timed(calls))
            out["lfa_coverage_srlg"] = a[3].cpu().numpy().view(np.uint32).tolist()
            out["rl_coverage_srlg"] = b[6].cpu().numpy().view(np.uint32).tolist()
            for k in calls:
                out[k + "_median"] = round(float(np.median(out[k])), 4)
                out[k + "_spread"] = round(float((max(out[k]) - min(out[k])) / np.median(out[k])), 4)
            out["rlfa_srlg_over_plain"] = round(out["rlfa_srlg_ms_median"] / out["rlfa_ms_median"], 4)
            out["lfa_srlg_over_plain"] = round(out["lfa_srlg_ms_median"] / out["lfa_ms_median"], 4)
            print(json.dumps(out), flush=True)
            del skeep
        del keep
        G.free()
        GT.free()

    nr = 20000
    ring = np.stack([np.arange(nr, dtype=np.int64), (np.arange(nr, dtype=np.int64) + 1) % nr], axis=1)
    one("ring: 20 000 routers", synth._routers_only(nr, ring, synth.SEED, 1, 100, synth.MAX_PATH_METRIC_WIDE, "ring-20k", {}), 0)
    one("mesh: isis-100k, root 50200", synth.isis_100k(), 50200)
    ctx.close()


if __name__ == "__main__":
    main()
