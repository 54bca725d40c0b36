"""bench.py's multi-rank code at world size 2 on CPU (gloo), the engine stubbed FROM tests/ (tests/_bench_stub_engine.py):
first-contact insurance for the driver's N > 1 runs, which no session of this build could execute on hardware.  What runs
is the real file: launcher re-exec (`--gpus 2` without WORLD_SIZE), RANK / WORLD_SIZE handling, the communicator-id
broadcast, the C ABI's own hspf_shard_bounds, the in-flight step loop with `run_async` / `run_wait`, the in-place gather of
the distance table, the oracle check of the GATHERED table on rank 0, the `exchange` block and the one JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(port):
    env = dict(os.environ)
    env["HSPF_BENCH_STUB"] = "_bench_stub_engine"
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT, env.get("PYTHONPATH", "")])
    env["MASTER_PORT"] = str(port)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def _line(stdout):
    lines = [ln for ln in stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_two_ranks_through_the_launcher_reexec():
    """`python bench.py --gpus 2` started by hand becomes the launcher (torch.distributed.run, rendezvous on 127.0.0.1)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
                        "--no-cpu-baseline"], env=_env(29641), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    d = _line(p.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0 and d["steps"] == 2
    assert d["verified_roots"] == 64 and d["verified_gathered_dist_roots"] == 128, "rank 0 checks the gathered table of all 2 x 64 roots"
    assert "STUB" in d["data"]
    assert "hspf_multi_run" in d["config"]["gather"]
    ex = d["exchange"]
    assert [r["rank"] for r in ex["per_rank"]] == [0, 1] and all(r["bytes_sent"] == 64 * d["config"]["n_vertices"] * 4 for r in ex["per_rank"])
    assert "cpu_baseline" not in d and "roofline" in d and d["roofline"]["frac"] > 0


def test_two_ranks_as_the_driver_launches_them_without_the_library_gather():
    """The driver's command line (`python -m torch.distributed.run ... bench.py --gpus 2 ...`), here with `--gather none`:
    each rank keeps its own rows (a one-rank engine per process)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29643",
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--gather", "none"]
    p = subprocess.run(cmd, env=_env(29643), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    d = _line(p.stdout)
    assert d["n_gpus"] == 2 and d["verified_roots"] == 64 and d["verified_gathered_dist_roots"] == 64 and d["config"]["gather"] == "none"
    assert "exchange" not in d


def test_plain_run_prints_the_headline_only_and_dumps_the_last_timed_step(tmp_path):
    """A plain run (no --full) at world size 1: exactly --steps timed steps, the headline keys and nothing beside them;
    --dump-outputs writes the last timed step's tables (float32 / float64, below 64 MB) and they are the oracle's."""
    import numpy as np
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=_env(29645), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    d = _line(p.stdout)
    assert set(d) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "timed_steps", "timed_ms",
                      "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
    assert d["steps"] == d["timed_steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["value"] > 0
    assert abs(d["ms_per_step"] * d["timed_steps"] - d["timed_ms"]) < 0.01 * d["timed_ms"] + 0.01
    names = {"dist", "hops", "flags", "first_hop_mask_lo", "first_hop_mask_hi", "vertex_index", "dist_roots", "roots"}
    assert {f.name for f in out.iterdir()} == {n + ".npy" for n in names}
    a = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum((out / (n + ".npy")).stat().st_size for n in names) < 64 * 2 ** 20
    from oracle import graph_oracle as go
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _bench_stub_engine
    g = _bench_stub_engine.bench_graph()
    roots, vidx = a["roots"].astype(np.uint32), a["vertex_index"].astype(np.int64)
    W = d["config"]["mask_words"]
    ref = go.run(g.row_ptr, g.col, g.metric, g.vflags, g.max_path_metric, roots, 0, go.HEAP, mask_words_=W)
    mask = (a["first_hop_mask_hi"].astype(np.uint64) << np.uint64(32)) | a["first_hop_mask_lo"].astype(np.uint64)
    assert np.array_equal(a["dist_roots"], a["roots"]) and a["dist"].shape == (64, len(vidx))
    assert np.array_equal(a["dist"].astype(np.uint64), ref.dist[:, vidx].astype(np.uint64))
    assert np.array_equal(a["hops"], ref.hops[:, vidx].astype(np.float32))
    assert np.array_equal(a["flags"], (ref.flags[:, vidx] & 3).astype(np.float32))
    assert np.array_equal(mask, ref.mask[:, vidx])
