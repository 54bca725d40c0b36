"""Two-segment node-protecting repairs through the compiled layers: tests/cpp/tilfa_node_driver.cpp reads a case the Python model
wrote (graph, candidate table, expected arrays) and compares what the RAII layer (hspf::Engine::tilfa_node_select_device /
tilfa_node_device on device buffers), its one-root convenience (hspf::Engine::tilfa_node) and hspf::host::HipEngine::tilfa_node (the host interface, fed by its own rlfa_node) deliver,
every array.  CPU leg: an engine without the call answers TilfaNodeOut::supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _rlfa_node_model as N
import _tilfa_node_model as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "tilfa_node_driver")
LINE = re.compile(r"(\d+) cases, (\d+) destinations compared, (\d+) differ, (\d+) answered not supported")
MAX_PAIRS = 4


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("tilfa_node_driver")


def _heavy_ring(n, seed, heavy_at):
    """A ring with one seeded cost per DIRECTION (the reverse run matters) and one link at 4 n."""
    r = np.random.default_rng(seed)
    links = []
    for a, b in [(v, (v + 1) % n) for v in range(n)]:
        c1, c2 = (4 * n, 4 * n) if a == heavy_at else (int(r.integers(1, 4)), int(r.integers(1, 4)))
        links += [(a, b, c1), (b, a, c2)]
    return M.csr(n, links)


def _six_ring():
    return M.csr(6, M.both([(v, (v + 1) % 6, 10 if v == 3 else 1) for v in range(6)]))


def _ring8():
    return M.csr(8, M.both([(v, (v + 1) % 8, 1) for v in range(8)]))


def _write_cases(tmp_path):
    files, kinds = [], set()
    for i, (graph, root) in enumerate([(_heavy_ring(24, 5, 14), 2), (_six_ring(), 0), (_ring8(), 0)]):
        rp, col, met, vf = graph
        c, roots, nbr_row, W, lfa, rl = R.one_root(graph, root)
        fwd, _ = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
        ns = N.select(fwd.dist, c, 0, nbr_row, rl.space_flags, 0, 16)
        nd = N.dest(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, ns, N.y_rows(graph, 0xFFFFFFFF, N.union(ns)), lfa.alt_flags)
        sel = TN.select(fwd.dist, graph, c, 0, nbr_row, rl.space_flags, 0, MAX_PAIRS)
        y = TN.union(sel) or [TN.NONE]
        d = TN.dest(fwd.dist, fwd.flags, fwd.mask, c, 0, nbr_row, sel, TN.y_rows(graph, 0xFFFFFFFF, [v for v in y if v != TN.NONE]), lfa.alt_flags, nd.nd_kind)
        kinds |= set(d.tn_kind.tolist())
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(roots)], roots, nbr_row, [W, MAX_PAIRS], sel.tq_q.ravel(), sel.tq_p.ravel(), sel.tq_link.ravel(), sel.tq_via.ravel(),
                 sel.tq_metric.ravel(), sel.tq_count, [len(y)], y, nd.nd_kind,
                 d.tn_kind, d.tn_p, d.tn_q, d.tn_link, d.tn_via, d.tn_metric, d.tn_set, d.tn_coverage]
        p = tmp_path / f"tilfa_node_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert {TN.D_PAIR, TN.D_PQ, TN.D_LAST_HOP} <= kinds                   # two-segment repairs, and one-segment ones that stand, go through the layers
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
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == 3 * (24 + 6 + 8), out
