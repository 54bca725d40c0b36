"""TI-LFA repairs along the post-convergence path through the compiled layers: tests/cpp/tilfa_pc_driver.cpp reads a case the Python
model wrote (graph, candidate table, tables, space tables, failure rows, expected arrays) and compares every array.  CPU legs: the
sequential host twin (hspf::host::tilfa_pc_sequential), and an engine without the call, which answers TilfaPcOut::supported ==
false.  GPU leg: hspf::Engine::tilfa_pc_device (the RAII layer) and hspf::host::HipEngine::tilfa_pc (the host interface, on its own
runs, space tables and failure rows)."""
import pytest

import _tilfa_pc_cases as C
import _tilfa_pc_model as P

NAMES = ("b_ring_one_adj", "c_two_adj", "d_four_adj", "e_long", "f_lan_in_gap", "g_p_is_root", "j_zero_cycle", "n_overload_ignored", "no_row")


def _write_cases(tmp_path):
    """Nine hand cases (every class but _D_LFA), and two sweep graphs with the alt_flags of the LFA model (one with two mask words)."""
    files, kinds, lens = [], set(), set()
    wants = [(C.CASES[k].want(), C.CASES[k].lfa_flags, False, C.CASES[k].max_walk) for k in NAMES]
    wants += [(P.one_root(C.sweep_graph(s), r, with_lfa=True, w_min=wm), 0, True, 256) for s, r, wm in ((5, 7, 1), (12, 3, 2))]
    for i, (w, lfa_flags, with_lfa, max_walk) in enumerate(wants):
        files.append(str(tmp_path / f"tilfa_pc_case_{i}.txt"))
        C.write_case_file(files[-1], w, lfa_flags, with_lfa, max_walk)
        kinds |= set(w.tp.tp_kind.tolist())
        lens |= set(w.tp.tp_n_adj[w.tp.tp_kind == P.D_REPAIR].tolist())
    assert {P.D_LFA, P.D_REPAIR, P.D_NONE, P.D_LONG, P.D_LAN, P.D_WALK} <= kinds and {0, 1, 2, 4} <= lens
    return files, sum(len(w.graph[3]) for w, *_ in wants)


def test_host_twin_equals_the_model_cpu(tmp_path):
    C.build_driver()
    files, n_dest = _write_cases(tmp_path)
    cases, compared, bad, unsupported = C.run_driver("host", files)
    assert cases == len(files) and compared == n_dest and bad == 0 and unsupported == 0


def test_host_interface_default_is_not_supported_cpu(tmp_path):
    C.build_driver()
    files, _ = _write_cases(tmp_path)
    cases, compared, bad, unsupported = C.run_driver("oracle", files)
    assert cases == len(files) == unsupported and compared == 0 and bad == 0


@pytest.mark.gpu
def test_raii_layer_and_host_interface_equal_the_model_gpu(tmp_path):
    C.build_driver()
    files, n_dest = _write_cases(tmp_path)
    cases, compared, bad, unsupported = C.run_driver("hip", files)
    assert cases == len(files) and bad == 0 and unsupported == 0 and compared == 2 * n_dest
