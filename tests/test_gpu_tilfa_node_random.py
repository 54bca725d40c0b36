"""A randomised differential run of hspf_tilfa_node_select_device and hspf_tilfa_node_device: the 40 seeded graphs of the TI-LFA
sweep (tests/_frr_chains.py: 12 to 60 routers, asymmetric costs, zero-cost links, an overloaded router) and ONE patched handle — the
five-ring of chain (a) after hspf_graph_patch gave row 1 a one-way link, so the host mirror's pool is out of order when the call
stages the two-way bytes.  One protected root each; every output of both calls against the plain-Python model
(tests/_tilfa_node_model.py), with the model's alt_flags, and the model's nd_kind on every other graph."""
import numpy as np
import pytest

import _frr_chains as FC
import _tilfa_node_model as TN
from test_gpu_rlfa import Case, Tables
from test_gpu_tilfa_node import Want, assert_equal, run_tn

pytestmark = pytest.mark.gpu


def test_forty_random_graphs_and_a_patched_handle(spf_ctx):
    from holo_amd import engine as E
    from test_gpu_frr_patched import PatchedTables
    kinds, listed = np.zeros(6, np.int64), 0
    jobs = [(Case(graph, root), i % 2 == 0, None) for i, (graph, root, _) in enumerate(FC.sweep_graphs())]
    ch = FC.chain("a")
    assert not ch.paths(spf_ctx.mode)[1].pool_compact                         # the patched handle's mirror is out of order
    jobs.append((Case(ch.steps[1].graph, ch.steps[1].prot[0]), True, ch))
    for i, (case, with_nd, chain) in enumerate(jobs):
        w = Want(case, with_nd=with_nd, max_pairs=8)
        kinds += np.bincount(w.d.tn_kind, minlength=6)
        listed += int(w.sel.tq_count.sum())
        pc = E.lfa_candidates(*case.graph, case.root)
        G = None
        if chain is None:
            tab = Tables(spf_ctx, case.graph, case.maxp, case.roots, 0, case.W)
        else:
            G = spf_ctx.upload(*chain.steps[0].graph, chain.maxp)
            G.patch(chain.steps[1].patch.vs, chain.steps[1].patch.rows, chain.steps[1].patch.flags)
            tab = PatchedTables(spf_ctx, G, chain.model(1))
            assert tab.W == case.W and np.array_equal(chain.model(1).roots, case.roots)
        try:
            one = lambda a: None if a is None else a[None, :]      # noqa: E731
            got = run_tn(spf_ctx, tab, [(0, pc, case.nbr_row)], w.y_roots, 0, 0, one(w.alt), one(w.nd_kind), 8)
            assert_equal(got, w.r, w.sel, w.d, tag=i)
        finally:
            if G is not None:
                G.free()
            else:
                tab.free()
    assert listed > 100 and (kinds[1:] > 0).all(), (listed, kinds.tolist())  # every class occurs, and the lists are not empty
