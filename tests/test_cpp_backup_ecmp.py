"""Per-primary backups of ECMP prefixes through the compiled layers: tests/cpp/backup_ecmp_driver.cpp reads a case the Python model
wrote (graph, candidate table, rows, prefix table, expected arrays with and without the repairs) and compares what the RAII layer
(hspf::Engine::backup_routes(..., ecmp = true): the whole chain and both calls) and the host interface
(hspf::host::HipEngine::backup_routes_ecmp on a DeviceRun and its DeviceRoutes) deliver, every array.
CPU leg: an engine without the call answers supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _backup_ecmp_cases as C
import _backup_ecmp_model as BE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "backup_ecmp_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("backup_ecmp_driver")


def _write_cases(tmp_path):
    """The prefix that is ECMP only per prefix, the LAN pair with a repair, and one seeded graph that needs repairs."""
    files, sizes = [], 0
    two = C.two_homes()
    for i, (graph, root, t) in enumerate([two[:3], C.lan_ring(), C.random_multihomed(C.GPU_SEEDS[11])]):
        rp, col, met, vf = graph
        model = C.Model(graph, [root], t)
        c, wants = model.cands[0], [BE.want(model, 0, rem)[0] for rem in (True, False)]
        assert wants[0].total > 0 and model.root_row[0] == 0
        n = len(vf)
        parts = [[n, len(col), 0xFFFFFFFF, root, 0, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(model.roots)], model.roots, model.nbr_row[0], [t.n, len(t.vertex), t.flags], t.ptr, t.vertex, t.metric]
        for w in wants:
            parts += [[w.total]] + [np.asarray(getattr(w, k)).ravel() for k in BE.FIELDS]
            sizes += t.n + 1 + 5 * w.total + BE.COVERAGE_WORDS                                      # each leg compares every array of one block
        p = tmp_path / f"backup_ecmp_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    return files, sizes


def _run(engine, files):
    cmd = [DRIVER, "--engine", engine]
    if engine == "oracle":
        cmd += ["--oracle-so", os.path.join(ROOT, "oracle", "liboracle_spf.so")]
    r = subprocess.run(cmd + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout
    return [int(x) for x in m.groups()], r.stdout


def test_host_interface_default_is_not_supported_cpu(tmp_path):
    from oracle import graph_oracle
    graph_oracle.build()
    _build_driver()
    files, _ = _write_cases(tmp_path)
    (cases, compared, bad, unsupported), out = _run("oracle", files)
    assert cases == len(files) == unsupported and compared == 0 and bad == 0, out


@pytest.mark.gpu
def test_raii_layer_and_host_interface_equal_the_model_gpu(tmp_path):
    _build_driver()
    files, sizes = _write_cases(tmp_path)
    (cases, compared, bad, unsupported), out = _run("hip", files)
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == sizes, out
