"""RibPipeline on an engine with the route event stream (Engine::routes_events -> hspf_routes_events): tests/cpp/route_events_driver.cpp
replays the recorded IS-IS step sequences and random chains of LSP-level changes; the messages of every step equal the literal
restatement's, and after EVERY step the pipeline's RIB (RibPipeline::full_rib(): prefix, metric, resolved next hops, rows without
next hops included) equals the RIB the restatement holds.  CPU leg: OracleEngine plus a restatement of the event stream; GPU leg:
the product engine."""
import glob
import os
import re
import subprocess

import pytest

from test_cpp_driver import _random_step_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "route_events_driver")
GOLD = os.path.join(ROOT, "tests", "golden")
RECORDED = sorted(p for p in glob.glob(os.path.join(GOLD, "isis_steps", "*.json")))
LINE = re.compile(r"(\d+) pipelines \((\d+) steps\) followed through the event stream, (\d+) differ, (\d+) not applicable; (\d+) RIB rows compared, "
                  r"(\d+) of them without next hops; (\d+) chains in which a route lost all its next hops and regained them")


def _build_driver():
    deps = [DRIVER + ".cpp"] + [os.path.join(ROOT, "tests", "cpp", f) for f in ("host_parity.cpp", "mini_json.hpp", "oracle_engine.hpp")] + \
        glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        subprocess.check_call([hb.hipcc_path(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-pthread", "-w", "-I" + os.path.join(ROOT, "include"),
                               DRIVER + ".cpp", "-L" + os.path.join(ROOT, "holo_amd"), "-lholo_spf_hip",
                               "-Wl,-rpath,$ORIGIN/../../holo_amd", "-ldl", "-o", DRIVER])


def _run(engine, golden, files):
    cmd = [DRIVER, "--engine", engine, "--golden", golden]
    if engine == "oracle":
        cmd += ["--oracle-so", os.path.join(ROOT, "oracle", "liboracle_spf.so")]
    r = subprocess.run(cmd + files, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout
    return [int(x) for x in m.groups()], r.stdout


def test_recorded_sequences_rib_follows_every_event_cpu():
    from oracle import graph_oracle
    graph_oracle.build()
    _build_driver()
    assert len(RECORDED) >= 17
    (pipes, steps, bad, _skipped, rows, no_nh, _), out = _run("oracle", GOLD, RECORDED)
    assert bad == 0 and pipes == 3 and steps == 2 * pipes, out      # (the three recorded steps that keep interfaces and configuration, as in host_parity)
    assert rows > 0 and no_nh > 0, out
    assert "routes_events calls" in out and int(re.search(r"(\d+) routes_events calls", out).group(1)) == steps


def test_random_chains_rib_follows_every_event_cpu(tmp_path):
    """200 random chains (seeds of this test's own): five steps each on one pipeline."""
    from oracle import graph_oracle
    graph_oracle.build()
    _build_driver()
    gdir, files = _random_step_files(tmp_path, range(17000, 17200))
    (pipes, steps, bad, skipped, rows, no_nh, regained), out = _run("oracle", gdir, files)
    assert bad == 0 and skipped == 0 and pipes == 200 and steps == 5 * pipes, out
    assert no_nh > 0 and int(re.search(r"(\d+) SILENT records", out).group(1)) > 0, out
    assert regained > 0, out                                          # a route lost all its next hops and got some back later


@pytest.mark.gpu
def test_recorded_sequences_and_random_chains_rib_follows_every_event_gpu(tmp_path):
    """The same with the product engine: hspf_routes_events behind HipEngine::routes_events (page-locked record buffer)."""
    _build_driver()
    (pipes, _steps, bad, _s, _rows, no_nh, _), out = _run("hip", GOLD, RECORDED)
    assert bad == 0 and pipes == 3 and no_nh > 0, out
    gdir, files = _random_step_files(tmp_path, range(17000, 17200))
    (pipes, steps, bad, skipped, _rows, no_nh, regained), out = _run("hip", gdir, files)
    assert bad == 0 and skipped == 0 and pipes == 200 and steps == 5 * pipes, out
    assert no_nh > 0 and regained > 0, out
