"""Loop-free alternates through the compiled layers: tests/cpp/lfa_driver.cpp reads cases the numpy model wrote (graph, candidate
table, expected arrays) and compares what hspf::Engine::lfa (the RAII layer) and hspf::host::HipEngine::lfa (the host interface)
deliver, every array, every destination.  CPU leg: an engine without the call answers LfaOut::supported == false."""
import os
import re
import subprocess

import numpy as np
import pytest

import _lfa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "lfa_driver")
LINE = re.compile(r"(\d+) cases, (\d+) destinations compared, (\d+) differ, (\d+) answered not supported")


def _build_driver():
    import glob
    deps = [DRIVER + ".cpp", os.path.join(ROOT, "tests", "cpp", "oracle_engine.hpp")] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    from holo_amd import build as hb
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        subprocess.check_call([hb.hipcc_path(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-pthread", "-w", "-I" + os.path.join(ROOT, "include"),
                               DRIVER + ".cpp", "-L" + os.path.join(ROOT, "holo_amd"), "-lholo_spf_hip",
                               "-Wl,-rpath,$ORIGIN/../../holo_amd", "-ldl", "-o", DRIVER])


def _grid(n, seed, width):
    r = np.random.default_rng(seed)
    und = [(v, v + 1) for v in range(n) if (v + 1) % width and v + 1 < n] + [(v, v + width) for v in range(n) if v + width < n]
    return M.csr(n, M.both([(a, b, int(r.integers(1, 10))) for a, b in und]))


def _lan():
    links = []
    for r_ in (1, 2, 3, 4):
        links += [(r_, 0, 10), (0, r_, 0)]
    links += M.both([(1, 5, 10), (2, 6, 1), (3, 6, 5), (4, 6, 5), (5, 6, 5), (6, 7, 1)])
    return M.csr(8, links, net=[0])


def _hub(k):
    r = np.random.default_rng(k)
    und = [(0, v, int(r.integers(1, 21))) for v in range(1, k + 1)] + [(v, v % k + 1, int(r.integers(1, 21))) for v in range(1, k + 1)]
    return M.csr(k + 1, M.both(und))


def _write_cases(tmp_path):
    from oracle import graph_oracle as go
    files = []
    for i, (graph, root, run_flags) in enumerate([(_grid(70, 4, 8), 27, 0), (_lan(), 1, 0), (_lan(), 1, 1), (_hub(66), 0, 0)]):
        rp, col, met, vf = graph
        c, roots, nbr_row = M.protect_one(rp, col, met, vf, root)
        W = max(go.mask_words(rp, col, met, vf, roots), (len(c.nbr) + 63) // 64)
        t = go.run(rp, col, met, vf, 0xFFFFFFFF, roots, run_flags, go.MAP, mask_words_=W)
        want = M.lfa(t.dist, t.flags, t.mask, c, 0, nbr_row)
        assert want.coverage[2] > 0
        parts = [[len(vf), len(col), 0xFFFFFFFF, root, run_flags], rp, col, met, vf, [len(c.nbr)], c.nbr, c.cost, c.root_link, c.cflags,
                 [len(roots)], roots, nbr_row, [W], want.alt_slot, want.alt_metric, want.alt_flags, want.cand_mask.ravel(), want.node_mask.ravel(),
                 want.coverage]
        p = tmp_path / f"lfa_case_{i}.txt"
        p.write_text("\n".join(" ".join(str(int(x)) for x in part) for part in parts) + "\n")
        files.append(str(p))
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
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == 2 * (70 + 8 + 8 + 67), out
