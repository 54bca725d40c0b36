"""Per-primary SRLG-safe backups of ECMP prefixes through the compiled layers: tests/cpp/backup_ecmp_srlg_driver.cpp reads a case
the Python model wrote (graph, candidate table, member lists with their rows, prefix table, the model's per-slot repairs, expected
arrays) and compares what the RAII layer (hspf::Engine::routes_backup_ecmp_srlg_device on device buffers, both calls) and the host
interface (hspf::host::HipEngine::routes_device -> backup_routes_ecmp_srlg) deliver, every array.  CPU leg: an engine without the
call answers supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _backup_ecmp_srlg_cases as C
import _backup_ecmp_srlg_model as BES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "backup_ecmp_srlg_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")
TI = ("ti_kind", "ti_via", "ti_metric", "ti_p", "ti_link")
SEEDS = (7224, 7152)


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("backup_ecmp_srlg_driver")


def _write_cases(tmp_path):
    """Two seeded graphs under HSPF_LFA_SRLG_SAFE_REPAIRS: refusals, accepted repairs and a refused pair go through the layers."""
    files, sizes, cov = [], 0, np.zeros(BES.COVERAGE_WORDS, np.int64)
    for i, seed in enumerate(SEEDS):
        graph, root, (gp, gr), t = C.seeded(seed)
        rp, col, met, vf = graph
        m = C.Model(graph, [root], gp, gr, t)
        lf = BES.SAFE_REPAIRS
        c, mem, ti, w = m.cands[0], m.mems[0], m.frr(lf)[0][2], BES.want(m, lf, True)[0]
        assert m.root_row[0] == 0 and w.total > 0
        cov += w.eb_coverage
        sizes += 2 * (t.n + 1 + 5 * w.total + BES.COVERAGE_WORDS)              # both legs compare every array
        pad = lambda a: np.concatenate([np.asarray(a).ravel(), np.zeros(64 * m.W - np.asarray(a).size, np.uint32)])      # noqa: E731
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, 0, lf], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(mem.tail)], mem.mem_ptr, mem.tail, mem.pos, mem.head, mem.cost, mem.tail_row, mem.head_row, [len(m.roots)], m.roots, m.nbr_row[0],
                 [m.W, t.n, len(t.vertex), t.flags], t.ptr, t.vertex, t.metric]
        parts += [pad(getattr(ti, k)) for k in TI] + [[w.total]] + [np.asarray(getattr(w, k)).ravel() for k in BES.FIELDS]
        p = tmp_path / f"backup_ecmp_srlg_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert cov[6] > 0 and (cov[8:] > 0).all(), cov
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
