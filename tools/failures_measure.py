"""Times hspf_run_failures_device against the route it replaces: per scenario a structural hspf_graph_patch, a one-root
hspf_run_device and the patch back.  Scenarios: every link of the root failed, then every distinct neighbour excluded.
  (a) failures  ONE hspf_run_failures_device call for all scenarios, on the untouched graph;
  (b) patched   per scenario: patch (the root's row with the failed link retargeted to a spare isolated vertex, or the excluded
                vertex's row emptied), hspf_run_device of the one root, patch back.  The graph is uploaded with one spare vertex.
A sample is one wall-clock window around the whole series, host staging and the calls' own synchronisation included; (a) and (b)
alternate sample by sample, `--repeats` samples each after one warm-up each.
    python tools/failures_measure.py [--repeats 9]
Workloads (holo_amd/synth.py): isis-100k root 50200; a ring of 20 000 routers; the first edge switch of the k = 16 fat-tree.
One JSON line per workload: both series, the medians, their spreads, (a) / (b)."""
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
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    import torch
    from holo_amd import engine as E, synth
    ctx = E.SpfContext(0)
    dev = torch.device("cuda:0")

    def one(name, g, root):
        # one spare vertex with an empty row: the target of a retargeted link (it fails the two-way check)
        n = g.n + 1
        rp = np.append(g.row_ptr, g.row_ptr[-1]).astype(np.uint32)
        vf = np.append(g.vflags, 0).astype(np.uint8)
        col, met = g.col, g.metric
        G = ctx.upload(rp, col, met, vf, g.max_path_metric)
        a, b = int(rp[root]), int(rp[root + 1])
        links = [(E.FAIL_ROOT_LINK, j) for j in range(b - a)]
        nbrs = [(E.FAIL_VERTEX, int(x)) for x in dict.fromkeys(col[a:b].tolist()) if int(x) != root]
        fails = np.array(links + nbrs, np.uint32)
        R = len(fails)
        roots = np.full(R, root, np.uint32)
        W = G.mask_words(roots)
        t = dict(dist=torch.empty((R, n), dtype=torch.int32, device=dev), hops=torch.empty((R, n), dtype=torch.int16, device=dev),
                 flags=torch.empty((R, n), dtype=torch.int16, device=dev), mask=torch.empty((R, n, W), dtype=torch.int64, device=dev))
        ptrs = dict(dist_ptr=t["dist"].data_ptr(), hops_ptr=t["hops"].data_ptr(), flags_ptr=t["flags"].data_ptr(), mask_ptr=t["mask"].data_ptr(), mask_words=W)
        one_ptrs = dict(ptrs)

        def failures():
            ctx.run_failures_device(G, roots, fails, 0, **ptrs)

        def patched():
            for kind, arg in fails.tolist():
                v = root if kind == E.FAIL_ROOT_LINK else arg
                va, vb = int(rp[v]), int(rp[v + 1])
                c = col[va:vb].copy()
                if kind == E.FAIL_ROOT_LINK:
                    c[arg] = n - 1
                else:
                    c[:] = n - 1
                G.patch([v], [(c, met[va:vb])], [int(vf[v])])
                ctx.run_device(G, roots[:1], 0, **one_ptrs)
                G.patch([v], [(col[va:vb], met[va:vb])], [int(vf[v])])

        calls = {"failures_ms": failures, "patched_ms": patched}
        samples = {k: [] for k in calls}
        for call in calls.values():
            call()
        for _ in range(args.repeats):
            for k, call in calls.items():
                t0 = time.perf_counter()
                call()
                samples[k].append(round((time.perf_counter() - t0) * 1e3, 4))
        out = {"workload": name, "n": g.n, "scenarios": R, "links": len(links), "neighbours": len(nbrs), "mask_words": W}
        failures()
        out["stats"] = {k: ctx.stats()[k] for k in ("n_exact_roots", "n_relax_launches", "n_dag_launches")}
        for k, v in samples.items():
            out[k] = v
            out[k + "_median"] = round(float(np.median(v)), 4)
            out[k + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 4)
        out["failures_over_patched"] = round(out["failures_ms_median"] / out["patched_ms_median"], 4)
        print(json.dumps(out), flush=True)
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
