"""SRLG-safe alternates and remote-LFA spaces through the compiled layers: tests/cpp/srlg_driver.cpp reads a case the Python model
wrote (graph, candidate table, group table, member lists with their rows, expected arrays) and compares what the RAII layer
(hspf::Engine::srlg_members -> lfa_srlg_device -> rlfa_srlg_device -> tilfa_device on device buffers) and the host interface
(hspf::host::HipEngine::lfa_srlg -> rlfa_srlg -> tilfa) deliver, every array.  CPU leg: an engine without the calls answers
supported == false for lfa_srlg and rlfa_srlg."""
import os
import re
import subprocess

import numpy as np
import pytest

import _lfa_model as M
import _rlfa_model as R
import _srlg_model as SM
import _tilfa_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "srlg_driver")
LINE = re.compile(r"(\d+) cases, (\d+) entries compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("srlg_driver")


def _cases():
    """(graph, root, groups): the ring with two chords whose one alternate is refused; S's two links in one conduit (a local
    member); a hub whose every link has members near the root."""
    ring = [(v, (v + 1) % 6, 1) for v in range(6)]
    g1 = M.csr(6, M.both(ring + [(0, 3, 2), (1, 4, 1)]))
    g2 = M.csr(4, M.both([(0, 1, 1), (0, 2, 2), (1, 3, 1), (2, 3, 1), (1, 2, 5)]))
    r = np.random.default_rng(1)
    und = {(0, v): int(r.integers(1, 9)) for v in range(1, 9)}
    for v in range(1, 9):
        und.setdefault(tuple(sorted((v, v % 8 + 1))), int(r.integers(1, 9)))
    g3 = M.csr(9, M.both([(a, b, c) for (a, b), c in sorted(und.items())]))
    of = {}
    for j in range(8):
        of.setdefault(int(g3[0][0]) + j, []).append(j)
        for l in (int(g3[0][1 + (j + 2) % 8]), int(g3[0][1 + (j + 3) % 8]) + 1):
            of.setdefault(l, []).append(j)
    one = lambda g, *links: SM.groups_csr(len(g[1]), {SM.link_pos(g, *l): [5] for l in links})      # noqa: E731
    return [(g1, 0, one(g1, (0, 1), (3, 2))), (g2, 0, one(g2, (0, 1), (0, 2))), (g3, 0, SM.groups_csr(len(g3[1]), of))]


def _write_cases(tmp_path):
    files, refused, lost, sizes = [], 0, 0, 0
    for i, (graph, root, (gp, gr)) in enumerate(_cases()):
        rp, col, met, vf = graph
        m = SM.one_root(graph, root, gp, gr)
        c, mem, lfa, rl, fwd = m["cand"], m["mem"], m["lfa"], m["rl"], m["fwd"]
        ti = T.tilfa(fwd.dist, fwd.flags, fwd.mask, m["rdist"], graph, c, 0, m["nbr_row"], rl.space_flags, rl.space_via, lfa.alt_flags)
        refused += int(lfa.coverage[6])
        lost += int(rl.pq_counts[:, 4].sum())
        S, n, K, Mt = 64 * m["W"], len(vf), len(c.nbr), len(mem.tail)
        per_leg = (3 * n + SM.LFA_COVERAGE_WORDS) + (3 * S + SM.COUNT_WORDS * S + 2 * S * n + 2 * n + SM.COVERAGE_WORDS) + (6 * S + 2 * S + n + 5)
        sizes += 2 * per_leg + (K + 1 + 4 * Mt)              # both legs compare every array; the RAII leg also the member lists
        parts = [[n, len(col), 0xFFFFFFFF, root, 0], rp, col, met, vf, [K], c.nbr, c.cost, c.root_link, c.cflags, gp, [len(gr)], gr,
                 [Mt], mem.mem_ptr, mem.tail, mem.pos, mem.head, mem.cost, [len(m["roots"])], m["roots"], m["nbr_row"], mem.tail_row, mem.head_row,
                 [m["W"]], lfa.alt_slot, lfa.alt_metric, lfa.alt_flags, lfa.coverage]
        parts += [np.asarray(getattr(rl, f)).ravel() for f in R.FIELDS] + [np.asarray(getattr(ti, f)).ravel() for f in T.FIELDS]
        p = tmp_path / f"srlg_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
    assert refused >= 3 and lost >= 3                                     # refused alternates and removed PQ candidates go through the layers
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
