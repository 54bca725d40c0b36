"""Two-segment repair paths through the compiled layers: tests/cpp/tilfa_driver.cpp reads a case the Python model wrote (graph,
candidate table, expected arrays) and compares what hspf::Engine::tilfa (the RAII layer) and hspf::host::HipEngine::tilfa (the host
interface) deliver, every array.  CPU leg: an engine without the call answers TilfaOut::supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _tilfa_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "tilfa_driver")
LINE = re.compile(r"(\d+) cases, (\d+) destinations compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("tilfa_driver")


def _ring(n, seed):
    """A ring with one seeded cost per DIRECTION (the reverse run matters) and one chord."""
    r = np.random.default_rng(seed)
    links = []
    for a, b in [(v, (v + 1) % n) for v in range(n)] + [(5, n - 4)]:
        links += [(a, b, int(r.integers(1, 10))), (b, a, int(r.integers(1, 10)))]
    return M.csr(n, links)


def _five_ring():
    return M.csr(5, M.both([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 4)]))


def _write_cases(tmp_path):
    files = []
    kinds = set()
    for i, (graph, root) in enumerate([(_ring(24, 5), 2), (_five_ring(), 2)]):
        rp, col, met, vf = graph
        c, roots, nbr_row, W, lfa, rl = R.one_root(graph, root)
        fwd, rdist = R.tables(graph, 0xFFFFFFFF, roots, 0, W)
        want = T.tilfa(fwd.dist, fwd.flags, fwd.mask, rdist, graph, c, 0, nbr_row, rl.space_flags, rl.space_via, lfa.alt_flags)
        kinds |= set(want.ti_kind.tolist())
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(roots)], roots, nbr_row, [W], want.ti_kind, want.ti_p, want.ti_q, want.ti_via, want.ti_link, want.ti_metric,
                 want.ti_counts.ravel(), want.td_kind, want.td_coverage]
        p = tmp_path / f"tilfa_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert {T.KIND_NODE, T.KIND_PAIR} <= kinds                           # both kinds of repair go through the layers
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
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == 2 * (24 + 5), out
