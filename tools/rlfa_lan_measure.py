"""Times hspf_rlfa_lan_device against hspf_rlfa_device on the same resident tables.  A sample is one HIP-event window on the
context's stream around `--inner` consecutive C calls with prebuilt arguments (about a millisecond of work; the figure is the
window over `--inner`); the two calls are ALTERNATED sample by sample, `--repeats` samples each after one warm-up call each, so a
difference can be held against the plain call's own spread.
    python tools/rlfa_lan_measure.py [--inner 10] [--repeats 9] [--plain-only]
--plain-only times hspf_rlfa_device alone and needs nothing this call added: it runs unchanged on a checkout that has no
hspf_rlfa_lan_device (the same happens by itself where the library lacks the symbol).  That is how the plain call of an earlier
commit is compared with this tree's: both checkouts, the same job, alternating processes.
Workloads:
  (a) isis-100k (no network vertex): root 50200 + its neighbours.  Every lan[k] is HSPF_NO_ROOT: no LAN term is ever evaluated;
      what the LAN call adds is the second staged table, the wider gather, the fifth count word and the wider chunk state.
  (b) an LSDB with networks (synth.random_lsdb, 20 000 routers, 2 000 LANs): one protected root on a LAN, then eight sharing one
      table set (rows: the roots, their neighbour routers, their LANs; both the forward and the transposed run).
One JSON line per workload: the samples, the median of each call, the ratio LAN / plain and each call's spread."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))

    with_lan = not args.plain_only and hasattr(ctx.lib, "hspf_rlfa_lan_device")

    def timed(calls):
        """{name: samples}: the calls taken in turn, sample by sample; a sample is ms per call over a window of `inner` calls."""
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

    def one(name, g, prot_roots, spaces):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cands = [E.lfa_candidates(*graph, r) for r in prot_roots]
        lans = [E.lfa_lan_candidates(*graph, r) for r in prot_roots]
        extra = {int(v) for c in cands for v in c.nbr if v != E.NO_ROOT} | {int(v) for l in lans for v in l if v != E.NO_ROOT}
        rows = list(prot_roots) + sorted(extra - set(prot_roots))
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        GT = ctx.upload(*E.csr_transpose(*graph), g.vflags, g.max_path_metric)
        W = max(G.mask_words(roots), max((c.n_slots + 63) // 64 for c in cands))
        R, n, P, S = len(rows), g.n, len(prot_roots), 64 * W
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        u8 = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=dev)      # noqa: E731
        dist, flags, mask, rdist = i32(R, n), torch.empty((R, n), dtype=torch.int16, device=dev), torch.empty((R, n, W), dtype=torch.int64, device=dev), i32(R, n)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        ctx.run_device(GT, roots, 0, dist_ptr=rdist.data_ptr())
        tabs = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr(), rdist.data_ptr())
        protect = [(row_of[r], c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32)) for r, c in zip(prot_roots, cands)]
        lan_cols = [(l, np.array([row_of.get(int(v), 0) for v in l], np.uint32)) for l in lans]
        arr, keep = ctx._protect_array(protect, "rlfa_lan_measure")
        larr, lkeep = ctx._lan_array(lan_cols, protect, "rlfa_lan_measure") if with_lan else (None, None)
        sf, sv = (u8(P, S, n), i32(P, S, n)) if spaces else (None, None)
        bufs = [i32(P, S), i32(P, S), i32(P, S), i32(P, S, 5), i32(P, n), i32(P, n), i32(P, 6)]
        ro = L.HspfRlfaOut(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), sf.data_ptr() if spaces else None,
                           sv.data_ptr() if spaces else None, bufs[4].data_ptr(), bufs[5].data_ptr(), bufs[6].data_ptr())

        def plain():
            assert ctx.lib.hspf_rlfa_device(ctx.handle, G.handle, n, R, W, *tabs, arr, P, 0, None, ctypes.byref(ro)) == 0, ctx.last_error()

        def lan():
            assert ctx.lib.hspf_rlfa_lan_device(ctx.handle, G.handle, n, R, W, *tabs, arr, larr, P, 0, None, ctypes.byref(ro)) == 0, ctx.last_error()
        out = dict(workload=name, n_vertices=n, rows=R, protected=P, mask_words=W, spaces=spaces, slots=[c.n_slots for c in cands],
                   lan_slots=[int(((l != E.NO_ROOT) & (c.nbr != E.NO_ROOT)).sum()) for l, c in zip(lans, cands)], inner=args.inner)
        out.update(timed(dict(rlfa_ms=plain, rlfa_lan_ms=lan) if with_lan else dict(rlfa_ms=plain)))
        if with_lan:
            out["rl_coverage_lan"] = bufs[6].cpu().numpy().view(np.uint32).tolist()
            out["rlfa_lan_over_plain"] = round(float(np.median(out["rlfa_lan_ms"]) / np.median(out["rlfa_ms"])), 4)
        for k in [k for k in ("rlfa_ms", "rlfa_lan_ms") if k in out]:
            out[k + "_median"] = round(float(np.median(out[k])), 4)
            out[k + "_spread"] = round(float((max(out[k]) - min(out[k])) / np.median(out[k])), 4)
        print(json.dumps(out), flush=True)
        del keep, lkeep
        G.free()
        GT.free()

    one("a: isis-100k, no LAN, root 50200", synth.isis_100k(), [50200], True)
    g = synth.random_lsdb(20000, 2000, 4.0, 3, metric_hi=50, p_overload=0.0, p_noexpand=0.0)
    on_lan = [r for r in range(2000, 22000) if (E.lfa_lan_candidates(g.row_ptr, g.col, g.metric, g.vflags, r) != E.NO_ROOT).any()
              and E.lfa_candidates(g.row_ptr, g.col, g.metric, g.vflags, r).n_slots <= 64][:8]
    one("b1: LSDB with networks, one root", g, on_lan[:1], True)
    one("b8: LSDB with networks, eight roots, no space tables", g, on_lan, False)
    ctx.close()


if __name__ == "__main__":
    main()
