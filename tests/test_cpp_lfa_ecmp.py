"""Per-primary alternates of ECMP destinations through the compiled layers: tests/cpp/lfa_ecmp_driver.cpp reads a case the Python
model wrote (graph, candidate table, rows, expected arrays) and compares what the RAII layer (hspf::Engine::lfa_ecmp: candidates,
run and both sizing calls) and the host interface (hspf::host::HipEngine::lfa_ecmp on a DeviceRun) deliver, every array.
CPU leg: an engine without the call answers supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _lfa_ecmp_cases as C
import _lfa_ecmp_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "lfa_ecmp_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("lfa_ecmp_driver")


def _write_cases(tmp_path):
    """The diamond and one seeded graph with pseudonodes."""
    files, sizes = [], 0
    for i, (graph, root) in enumerate([C.diamond()[:2], C.random_isis_like(C.GPU_SEEDS[1])]):
        rp, col, met, vf = graph
        c, roots, nbr_row, _, t = EM.tables(graph, root)
        w = EM.lfa_ecmp(t.dist, t.flags, t.mask, c, 0, nbr_row)
        assert w.total > 0
        n = len(vf)
        sizes += len(c.nbr) + len(roots) + 2 * (n + 1 + 4 * w.total + EM.COVERAGE_WORDS)          # both legs compare every array
        parts = [[n, len(col), 0xFFFFFFFF, root, 0, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(roots)], roots, nbr_row, [w.total]] + [np.asarray(getattr(w, k)).ravel() for k in EM.FIELDS]
        p = tmp_path / f"lfa_ecmp_case_{i}.txt"
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
