"""Remote LFA with LAN-safe spaces through the compiled layers: tests/cpp/rlfa_lan_driver.cpp reads a case the Python model wrote
(graph, candidate table with its LAN columns, expected arrays) and compares what the RAII layer (hspf::Engine::lfa_lan_device ->
rlfa_lan_device -> tilfa_device on device buffers) and the host interface (hspf::host::HipEngine::lfa_lan -> rlfa_lan -> tilfa)
deliver, every array.  CPU leg: an engine without the call answers supported == false for rlfa_lan."""
import os
import re
import subprocess

import numpy as np
import pytest

import _rlfa_lan_model as RL
import _rlfa_model as R
import _tilfa_model as T
from test_host_lfa_lan import two_lans
from test_host_rlfa_lan import trap_x, via_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "rlfa_lan_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("rlfa_lan_driver")


def _write_cases(tmp_path):
    files, lost, sizes = [], 0, 0
    for i, (graph, root) in enumerate((trap_x(), via_only(), two_lans())):
        rp, col, met, vf = graph
        m = RL.one_root(graph, root)
        c, rl, fwd = m["cand"], m["rl"], m["fwd"]
        ti = RL.tilfa(fwd.dist, fwd.flags, fwd.mask, m["rdist"], graph, c, 0, m["nbr_row"], rl, m["lfa"].alt_flags)
        lost += int(rl.pq_counts[:, 4].sum())
        S, n = 64 * m["W"], len(vf)              # both legs compare every RLFA and every TI-LFA array: per leg
        sizes += 2 * ((3 * S + RL.COUNT_WORDS * S + 2 * S * n + 2 * n + RL.COVERAGE_WORDS) + (6 * S + 2 * S + n + 5))
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags, m["lan"],
                 [len(m["roots"])], m["roots"], m["nbr_row"], m["lan_row"], [m["W"]]]
        parts += [np.asarray(getattr(rl, f)).ravel() for f in R.FIELDS] + [np.asarray(getattr(ti, f)).ravel() for f in T.FIELDS]
        p = tmp_path / f"rlfa_lan_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert lost >= 6                                                      # nodes removed by the LAN rule go through the layers
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
