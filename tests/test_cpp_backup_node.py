"""Per-prefix node-protecting backups through the compiled layers: tests/cpp/backup_node_driver.cpp reads a case the Python model
wrote (graph, candidate table, prefix table, the plain call's bk_kind / bk_flags, expected arrays) and compares every output array
of hspf::Engine::routes_backup_node_device (the RAII layer) and of hspf::host::HipEngine::backup_routes_node (the host interface).
CPU leg: an engine without the call answers BackupNodeOut::supported == false through the host interface's default."""
import os
import re
import subprocess

import pytest

import _backup_cases as C
import _backup_node_cases as BC
import _backup_node_model as BN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "backup_node_driver")
LINE = re.compile(r"(\d+) cases, (\d+) prefixes compared, (\d+) differ, (\d+) answered not supported")
MQ, MP = 16, 8                                            # max_pq and max_pairs of the cases: two different list lengths


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("backup_node_driver")


def _write_cases(tmp_path):
    files, kinds, total = [], set(), 0
    for i, case in enumerate([BC.six_ring(), BC.five_ring(), C.sweep_case(C.SWEEP_SEED + 1)]):
        g, S, t = case
        m = C.Model(g, [S], t)
        rp, col, met, vf = g
        w = BN.Want(m, max_pq=MQ, max_pairs=MP)
        c, bn = m.cands[0], w.bn
        kinds |= set(bn.bn_kind.tolist())
        total += t.n
        parts = [[len(vf), len(col), C.MAXP, S, 0], rp, col, met, vf, [len(c.nbr)], c.nbr, m.nbr_row[0], c.cost, c.root_link, c.cflags, [len(m.roots)], m.roots,
                 [m.W, MQ, MP, t.n, len(t.vertex), t.flags], t.ptr, t.vertex, t.metric, [len(w.y_roots)], w.y_roots, w.bk.bk_kind, w.bk.bk_flags,
                 *(getattr(bn, f) for f in BN.FIELDS)]
        p = tmp_path / f"backup_node_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert {BN.BN_LFA, BN.BN_PQ, BN.BN_LAST_HOP, BN.BN_PAIR} <= kinds, kinds      # an alternate, both repairs and a last hop go through
    return files, total


def _run(engine, files):
    cmd = [DRIVER, "--engine", engine]
    if engine == "oracle":
        cmd += ["--oracle-so", os.path.join(ROOT, "oracle", "liboracle_spf.so")]
    r = subprocess.run(cmd + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
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
def test_both_cpp_layers_equal_the_model_gpu(tmp_path):
    _build_driver()
    files, total = _write_cases(tmp_path)
    (cases, compared, bad, unsupported), out = _run("hip", files)
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == 2 * total, out
