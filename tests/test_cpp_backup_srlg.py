"""Per-prefix SRLG-safe backups through the compiled layers: tests/cpp/backup_srlg_driver.cpp reads a case the Python model wrote
(graph, candidate table, member lists with their rows, prefix table, the model's per-slot repairs, expected arrays) and compares
what the RAII layer (hspf::Engine::routes_backup_srlg_device on device buffers) and the host interface
(hspf::host::HipEngine::routes_device -> backup_routes_srlg) deliver, every array.  CPU leg: an engine without the call answers
supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _backup_srlg_cases as SC
import _backup_srlg_model as BS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "backup_srlg_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")
TI = ("ti_kind", "ti_via", "ti_metric", "ti_p", "ti_link")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("backup_srlg_driver")


def _write_cases(tmp_path):
    """The ring with two chords with and without HSPF_LFA_SRLG_SAFE_REPAIRS, and two random graphs under the flag."""
    files, sizes, refused, repaired = [], 0, 0, 0
    inputs = [(SC.ring(), 0), (SC.ring(), BS.SAFE_REPAIRS), (SC.random_case(SC.RANDOM_SEED), BS.SAFE_REPAIRS), (SC.random_case(SC.RANDOM_SEED + 2), BS.SAFE_REPAIRS)]
    for i, ((graph, root, (gp, gr), t), lf) in enumerate(inputs):
        rp, col, met, vf = graph
        m = SC.Model(graph, [root], gp, gr, t)
        c, mem, ti, w = m.cands[0], m.mems[0], m.frr(lf)[0][2], m.want(lf)[0]
        refused += int(w.bk_coverage[8])
        repaired += int(w.bk_coverage[4]) + int(w.bk_coverage[5])
        sizes += 2 * (5 * t.n + 2 * t.n * m.W + BS.COVERAGE_WORDS)              # both legs compare every array
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0, lf], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(mem.tail)], mem.mem_ptr, mem.tail, mem.pos, mem.head, mem.cost, mem.tail_row, mem.head_row, [len(m.roots)], m.roots, m.nbr_row[0],
                 [m.W, t.n, len(t.vertex), t.flags], t.ptr, t.vertex, t.metric]
        parts += [np.asarray(getattr(ti, k)).ravel() for k in TI] + [np.asarray(getattr(w, k)).ravel() for k in BS.FIELDS]
        p = tmp_path / f"backup_srlg_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert refused >= 3 and repaired >= 1                                   # refusals and accepted repairs go through the layers
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
