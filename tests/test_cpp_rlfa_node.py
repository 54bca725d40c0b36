"""Node-protecting remote LFA through the compiled layers: tests/cpp/rlfa_node_driver.cpp reads a case the Python model wrote
(graph, candidate table, expected arrays) and compares what the RAII layer (hspf::Engine::rlfa_node_select_device /
rlfa_node_device on device buffers) and hspf::host::HipEngine::rlfa_node (the host interface) deliver, every array.  CPU leg: an
engine without the call answers RlfaNodeOut::supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _rlfa_node_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "rlfa_node_driver")
LINE = re.compile(r"(\d+) cases, (\d+) destinations compared, (\d+) differ, (\d+) answered not supported")
MAX_PQ = 4


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("rlfa_node_driver")


def _ring(n, seed):
    """A ring with one seeded cost per DIRECTION (the reverse run matters) and one chord."""
    r = np.random.default_rng(seed)
    links = []
    for a, b in [(v, (v + 1) % n) for v in range(n)] + [(5, n - 4)]:
        links += [(a, b, int(r.integers(1, 10))), (b, a, int(r.integers(1, 10)))]
    return M.csr(n, links)


def _ring8():
    return M.csr(8, M.both([(v, (v + 1) % 8, 1) for v in range(8)]))


def _write_cases(tmp_path):
    files, kinds = [], set()
    for i, (graph, root) in enumerate([(_ring(24, 5), 2), (_ring8(), 0)]):
        rp, col, met, vf = graph
        c, roots, nbr_row, W, lfa, rl = R.one_root(graph, root)
        fwd, _ = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
        sel = N.select(fwd.dist, c, 0, nbr_row, rl.space_flags, 0, MAX_PQ)
        y = N.union(sel) or [N.NONE]
        d = N.dest(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, sel, N.y_rows(graph, 0xFFFFFFFF, [v for v in y if v != N.NONE]), lfa.alt_flags)
        kinds |= set(d.nd_kind.tolist())
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(roots)], roots, nbr_row, [W, MAX_PQ], sel.nq_node.ravel(), sel.nq_via.ravel(), sel.nq_metric.ravel(), sel.nq_count, [len(y)], y,
                 d.nd_kind, d.nd_node, d.nd_via, d.nd_metric, d.nd_set, d.nd_coverage]
        p = tmp_path / f"rlfa_node_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert {N.D_PQ, N.D_LAST_HOP} <= kinds                               # repairs by a PQ node go through the layers
    return files


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
    files = _write_cases(tmp_path)
    (cases, compared, bad, unsupported), out = _run("oracle", files)
    assert cases == len(files) == unsupported and compared == 0 and bad == 0, out


@pytest.mark.gpu
def test_raii_layer_and_host_interface_equal_the_model_gpu(tmp_path):
    _build_driver()
    files = _write_cases(tmp_path)
    (cases, compared, bad, unsupported), out = _run("hip", files)
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == 2 * (24 + 8), out
