"""Broadcast-link protection through the compiled layers: tests/cpp/lfa_lan_driver.cpp reads a case the Python model wrote (graph,
candidate table with its LAN columns, prefix table, expected arrays) and compares what the RAII layer
(hspf::Engine::lfa_lan_candidates / lfa_lan_device / routes_backup_lan_device on device buffers) and
hspf::host::HipEngine::lfa_lan (the host interface) deliver, every array.  CPU leg: an engine without the calls answers
supported == false for lfa_lan and backup_routes_lan."""
import os
import re
import subprocess

import numpy as np
import pytest

import _backup_model as B
import _lfa_lan_model as LM
import _lfa_model as M
from test_host_lfa_lan import trap, two_lans, models, A_, C_, D_, E_, F_, T_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "lfa_lan_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("lfa_lan_driver")


def _write_cases(tmp_path):
    files, refused = [], 0
    tables = [B.table([[(D_, 0)], [(T_, 0), (A_, 20)], [(E_, 0)], [(C_, 1), (F_, 1)]]), B.table([[(5, 0)], [(5, 1), (6, 0)], [(3, 0), (4, 0)]])]
    for i, ((graph, root), pt) in enumerate(zip((trap(), two_lans()), tables)):
        rp, col, met, vf = graph
        c, lan, _, want, t, roots, nbr_row, lan_row = models(graph, root)
        bk = LM.backup(t.dist, t.flags, t.mask, c, 0, nbr_row, lan, lan_row, pt, B.routes(t.dist, t.flags, t.mask, 0, pt))
        refused += int(want.coverage[6]) + int(bk.bk_coverage[8])
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags, lan,
                 [len(roots)], roots, nbr_row, lan_row, [t.mask.shape[2]], want.alt_slot, want.alt_metric, want.alt_flags, want.cand_mask.ravel(),
                 want.node_mask.ravel(), want.coverage, [pt.n, len(pt.vertex), pt.flags], pt.ptr, pt.vertex, pt.metric,
                 bk.bk_kind, bk.bk_primary, bk.bk_slot, bk.bk_metric, bk.bk_flags, bk.bk_cand_mask.ravel(), bk.bk_node_mask.ravel(), bk.bk_coverage]
        p = tmp_path / f"lfa_lan_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert refused >= 4                                                   # refusals go through the layers
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


def test_host_interface_defaults_are_not_supported_cpu(tmp_path):
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
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == (2 * 8 + 4) + (2 * 8 + 3), out
