#!/usr/bin/env python3
"""A/B of the route hand-off on one GPU, one process, identical device tables:

  (A) the sequence HipEngine::routes_changed issues: hspf_routes_diff_device, hspf_routes_diff_count, hspf_routes_pack of the
      new set, hspf_routes_pack of the old set — into freshly sized pageable host arrays, as the std::vectors there are;
  (B) ONE hspf_routes_events call with HSPF_EV_SILENT into a page-locked buffer the caller keeps (what HipEngine::routes_events
      does).

Shapes: 1 root x 120 000 prefixes with ~10 changed pairs (one LSP change), the same with every pair changed (cold start),
64 x 120 000 with about 1 % changed.  Every shape is warmed up on both sides, then the two sides alternate; host clock around
calls that end synchronised.  One JSON line per shape: median and 10th / 90th percentile of each side in milliseconds, and
whether median(B) <= median(A) + (p90(A) - p10(A)).

    python tools/route_events_ab.py [--reps 200] [--warmup 20]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from holo_amd import _lib as L          # noqa: E402
from holo_amd import engine as E        # noqa: E402

NONE = 0xFFFFFFFF


def tables(rng, R, P, W):
    n = R * P
    bm = rng.integers(1, 1000, n, dtype=np.uint32)
    be = rng.integers(0, 1 << 20, n, dtype=np.uint32)
    nm = np.zeros((n, W), np.uint64)
    nm[:, 0] = np.uint64(1) << rng.integers(0, 24, n, dtype=np.uint64)
    nm[rng.random(n) < 0.1] = 0                                # CONNECTED-like routes: no next hops
    gone = rng.random(n) < 0.05
    bm[gone], be[gone], nm[gone] = NONE, NONE, 0
    return bm, be, nm


def changed(rng, old, k):
    """k pairs change: metric up (INSTALL, or SILENT for a route without next hops), some routes vanish (WITHDRAW / SILENT)."""
    bm, be, nm = (a.copy() for a in old)
    idx = rng.choice(len(bm), size=k, replace=False) if k < len(bm) else np.arange(len(bm))
    has = be[idx] != NONE
    bm[idx[has]] += 1
    drop = idx[has][:: 7]
    bm[drop], be[drop], nm[drop] = NONE, NONE, 0
    new_route = idx[~has]
    bm[new_route], be[new_route] = 5, 1
    nm[new_route, 0] = 1
    return bm, be, nm


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    ctx = E.SpfContext(0)
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(2026)
    shapes = [("1x120000_10_changed", 1, 120_000, 10), ("1x120000_all_changed", 1, 120_000, 120_000), ("64x120000_1pct", 64, 120_000, 76_800)]
    W = 1
    ok_all = True
    for name, R, P, k in shapes:
        old = tables(rng, R, P, W)
        new = changed(rng, old, k)
        up = lambda t: (torch.from_numpy(t[0].view(np.int32)).to(dev), torch.from_numpy(t[1].view(np.int32)).to(dev),      # noqa: E731
                        torch.from_numpy(t[2].view(np.int64).reshape(R, P, W)).to(dev))
        d_old, d_new = up(old), up(new)
        o, n = L.HspfRoutes(*(x.data_ptr() for x in d_old)), L.HspfRoutes(*(x.data_ptr() for x in d_new))
        act = torch.empty((R * P,), dtype=torch.uint8, device=dev)
        chg = torch.empty((R * P,), dtype=torch.int32, device=dev)
        cptr = torch.empty((R + 1,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rw_a, rw_b = 6 + 2 * W, E.EVENT_REC_WORDS + 4 * W
        pin = {"buf": None, "cap": 0}

        def side_a():
            rc = lib.hspf_routes_diff_device(h, R, P, W, ctypes.byref(o), ctypes.byref(n), act.data_ptr(), chg.data_ptr(), cptr.data_ptr())
            assert rc == 0, ctx.last_error()
            cnt = lib.hspf_routes_diff_count(h)
            words = np.zeros((cnt, rw_a), np.uint32)
            if cnt:
                assert lib.hspf_routes_pack(h, R, P, W, ctypes.byref(n), act.data_ptr(), chg.data_ptr(), cptr.data_ptr(), cnt, words.ctypes.data_as(L.u32p)) == 0
                old_words = np.zeros((cnt, rw_a), np.uint32)
                assert lib.hspf_routes_pack(h, R, P, W, ctypes.byref(o), act.data_ptr(), chg.data_ptr(), cptr.data_ptr(), cnt, old_words.ctypes.data_as(L.u32p)) == 0
            return cnt

        def side_b():
            if pin["buf"] is None:
                pin["cap"] = 1024
                pin["buf"] = E.PinnedBuffer(ctx, pin["cap"] * rw_b * 4)
            total = ctypes.c_uint32(0)
            rc = lib.hspf_routes_events(h, R, P, W, ctypes.byref(o), ctypes.byref(n), E.EV_SILENT, pin["cap"],
                                        ctypes.cast(pin["buf"].ptr, L.u32p), ctypes.byref(total))
            assert rc == 0, ctx.last_error()
            if total.value > pin["cap"]:                       # the kept buffer grows, the tail comes with the second call
                head, cap = pin["cap"], total.value + total.value // 4
                grown = E.PinnedBuffer(ctx, cap * rw_b * 4)
                grown.array[:head * rw_b * 4] = pin["buf"].array[:head * rw_b * 4]
                assert lib.hspf_routes_events_rest(h, head, total.value - head, ctypes.cast(grown.ptr + head * rw_b * 4, L.u32p)) == 0
                pin["buf"].free()
                pin["buf"], pin["cap"] = grown, cap
            return total.value

        na = nb = 0
        for _ in range(args.warmup):
            na, nb = side_a(), side_b()
        ta, tb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); side_a(); t1 = time.perf_counter(); side_b(); t2 = time.perf_counter()
            ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
        pa, pb = np.percentile(ta, [10, 50, 90]), np.percentile(tb, [10, 50, 90])
        ok = bool(pb[1] <= pa[1] + (pa[2] - pa[0]))
        ok_all &= ok
        print(json.dumps({"shape": name, "roots": R, "prefixes": P, "mask_words": W, "reps": args.reps,
                          "records_a": int(na), "events_b": int(nb),
                          "a_ms": {"p10": round(float(pa[0]), 4), "median": round(float(pa[1]), 4), "p90": round(float(pa[2]), 4)},
                          "b_ms": {"p10": round(float(pb[0]), 4), "median": round(float(pb[1]), 4), "p90": round(float(pb[2]), 4)},
                          "b_within_a_band": ok}), flush=True)
        pin["buf"].free()
        del d_old, d_new, act, chg, cptr
    ctx.close()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
