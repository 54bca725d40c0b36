"""Times hspf_lfa_lan_device against hspf_lfa_device, and hspf_routes_backup_lan_device against hspf_routes_backup_device, on the
same resident tables (HIP events on the context's stream around each C call with prebuilt arguments; `--repeats` samples of the
median of `--reps` calls after one warm-up, so that a difference can be held against the plain call's own spread).
    python tools/lfa_lan_measure.py [--reps 7] [--repeats 3] [--prefixes 200000]
Workloads:
  (a) isis-100k (no network vertex): root 50200 + its neighbours.  Every lan[k] is HSPF_NO_ROOT: no LAN term is ever evaluated;
      what the LAN call adds is the second staged table and the wider gather.
  (b) an LSDB with networks (synth.random_lsdb, 20 000 routers, 2 000 LANs): one protected root on a LAN, then eight sharing one
      table set (rows: the roots, their neighbour routers, their LANs).
Both halves run on THIS tree.  The plain calls' kernels k_lfa<ONE> report the parent commit's resource figures
(profiles/r17_notes.md), k_backup does not quite; a comparison against the parent commit itself means running the plain half
(tools/backup_measure.py, or this tool's lfa_ms / backup_ms columns) on a checkout of the parent.
One JSON line per workload: the samples, the median of each call and the ratio LAN / plain."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prefixes", type=int, default=200000)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth, _lib as L
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.lib.hspf_get_stream(ctx.handle))

    def timed(call):
        samples = []
        for _ in range(args.repeats):
            call()
            ev = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); call(); e1.record(stream); e1.synchronize()
                ev.append(e0.elapsed_time(e1))
            samples.append(round(float(np.median(ev)), 4))
        return samples

    def one(name, g, prot_roots):
        graph = (g.row_ptr, g.col, g.metric, g.vflags)
        cands = [E.lfa_candidates(*graph, r) for r in prot_roots]
        lans = [E.lfa_lan_candidates(*graph, r) for r in prot_roots]
        extra = {int(v) for c in cands for v in c.nbr if v != E.NO_ROOT} | {int(v) for l in lans for v in l if v != E.NO_ROOT}
        rows = list(prot_roots) + sorted(extra - set(prot_roots))
        row_of = {v: i for i, v in enumerate(rows)}
        roots = np.array(rows, np.uint32)
        G = ctx.upload(*graph, g.max_path_metric)
        W = max(G.mask_words(roots), max((c.n_slots + 63) // 64 for c in cands))
        R, n, P = len(rows), g.n, len(prot_roots)
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
        u8 = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=dev)      # noqa: E731
        i64 = lambda *sh: torch.empty(sh, dtype=torch.int64, device=dev)      # noqa: E731
        dist, flags, mask = i32(R, n), torch.empty((R, n), dtype=torch.int16, device=dev), i64(R, n, W)
        ctx.run_device(G, roots, 0, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr(), mask_ptr=mask.data_ptr(), mask_words=W)
        fwd = (dist.data_ptr(), flags.data_ptr(), mask.data_ptr())
        protect = [(row_of[r], c, np.array([row_of.get(int(v), 0) for v in c.nbr], np.uint32)) for r, c in zip(prot_roots, cands)]
        lan_cols = [(l, np.array([row_of.get(int(v), 0) for v in l], np.uint32)) for l in lans]
        arr, keep = ctx._protect_array(protect, "lfa_lan_measure")
        larr, lkeep = ctx._lan_array(lan_cols, protect, "lfa_lan_measure")
        slot, met, fl, cm, nm, cov = i32(P, n), i32(P, n), u8(P, n), i64(P, n, W), i64(P, n, W), i32(P, 7)
        lo = L.HspfLfaOut(slot.data_ptr(), met.data_ptr(), fl.data_ptr(), cm.data_ptr(), nm.data_ptr(), cov.data_ptr())

        def lfa_plain():
            assert ctx.lib.hspf_lfa_device(ctx.handle, n, R, W, *fwd, arr, P, 0, ctypes.byref(lo)) == 0, ctx.last_error()

        def lfa_lan():
            assert ctx.lib.hspf_lfa_lan_device(ctx.handle, n, R, W, *fwd, arr, larr, P, 0, ctypes.byref(lo)) == 0, ctx.last_error()
        out = dict(workload=name, n_vertices=n, rows=R, protected=P, mask_words=W, slots=[c.n_slots for c in cands],
                   lan_slots=[int((l != E.NO_ROOT).sum()) for l in lans], lfa_ms=timed(lfa_plain), lfa_lan_ms=timed(lfa_lan))
        out["lfa_coverage_lan"] = cov.cpu().numpy().view(np.uint32).tolist()
        # the per-prefix calls: every router advertises, a share of the prefixes on two routers
        rng = np.random.default_rng(7)
        NP = min(args.prefixes, 4 * n)
        routers = np.flatnonzero((g.vflags & 1) == 0).astype(np.uint32)
        first = rng.choice(routers, NP)
        second = rng.choice(routers, NP)
        two = rng.random(NP) < 0.2
        pfx_ptr = np.concatenate([[0], np.cumsum(1 + two)]).astype(np.uint32)
        pv = np.empty(int(pfx_ptr[-1]), np.uint32)
        pv[pfx_ptr[:-1]] = first
        pv[pfx_ptr[:-1][two] + 1] = second[two]
        pm = rng.integers(0, 20, len(pv)).astype(np.uint32)
        bm, be, nh = i32(R, NP), i32(R, NP), i64(R, NP, W)
        ctx.routes_device(n, R, W, *fwd, pfx_ptr, pv, pm, best_metric_ptr=bm.data_ptr(), best_entry_ptr=be.data_ptr(), nexthop_mask_ptr=nh.data_ptr())
        tab = L.HspfPrefixTable(NP, len(pv), pfx_ptr.ctypes.data_as(L.u32p), pv.ctypes.data_as(L.u32p), pm.ctypes.data_as(L.u32p), E.PFX_RESIDENT,
                                None, None, None, None)
        ro = L.HspfRoutes(bm.data_ptr(), be.data_ptr(), nh.data_ptr())
        bk = [u8(P, NP), i32(P, NP), i32(P, NP), i32(P, NP), u8(P, NP), i64(P, NP, W), i64(P, NP, W), i32(P, 9)]
        bo = L.HspfBackupOut(*(x.data_ptr() for x in bk))

        def bk_plain():
            rc = ctx.lib.hspf_routes_backup_device(ctx.handle, n, R, W, *fwd, arr, P, 0, ctypes.byref(tab), ctypes.byref(ro), None, ctypes.byref(bo))
            assert rc == 0, ctx.last_error()

        def bk_lan():
            rc = ctx.lib.hspf_routes_backup_lan_device(ctx.handle, n, R, W, *fwd, arr, larr, P, 0, ctypes.byref(tab), ctypes.byref(ro), None, ctypes.byref(bo))
            assert rc == 0, ctx.last_error()
        out.update(prefixes=NP, backup_ms=timed(bk_plain), backup_lan_ms=timed(bk_lan))
        out["backup_coverage_lan"] = bk[7].cpu().numpy().view(np.uint32).tolist()
        for a, b in (("lfa_ms", "lfa_lan_ms"), ("backup_ms", "backup_lan_ms")):
            out[b + "_over_plain"] = round(float(np.median(out[b]) / np.median(out[a])), 4)
            out[a + "_spread"] = round(float((max(out[a]) - min(out[a])) / np.median(out[a])), 4)
        print(json.dumps(out), flush=True)
        del keep, lkeep
        G.free()

    one("a: isis-100k, no LAN, root 50200", synth.isis_100k(), [50200])
    g = synth.random_lsdb(20000, 2000, 4.0, 3, metric_hi=50, p_overload=0.0, p_noexpand=0.0)
    on_lan = [r for r in range(2000, 22000) if (E.lfa_lan_candidates(g.row_ptr, g.col, g.metric, g.vflags, r) != E.NO_ROOT).any()
              and E.lfa_candidates(g.row_ptr, g.col, g.metric, g.vflags, r).n_slots <= 64][:8]
    one("b1: LSDB with networks, one root", g, on_lan[:1])
    one("b8: LSDB with networks, eight roots", g, on_lan)
    ctx.close()


if __name__ == "__main__":
    main()
