"""A randomised differential run of hspf_routes_backup_node_device: the 40 seeded graphs of the TI-LFA sweep (tests/_frr_chains.py:
12 to 60 routers, asymmetric costs, zero-cost links, an overloaded router) with seeded multi-homed prefix tables
(tests/_backup_node_cases.py) and ONE patched handle — the five-ring of chain (a) after hspf_graph_patch gave row 1 a one-way link.
One protected root each, lists of 8; every output against the plain-Python model (tests/_backup_node_model.py), bk_in on every
other graph."""
import numpy as np
import pytest

import _backup_cases as C
import _backup_node_cases as BC
import _backup_node_model as BN
import _frr_chains as FC
from test_gpu_backup_node import NodeDevice, assert_equal

pytestmark = pytest.mark.gpu


def test_forty_random_graphs_and_a_patched_handle(spf_ctx):
    from test_gpu_frr_patched import PatchedTables
    from test_gpu_backup import protect_of
    kinds = np.zeros(6, np.int64)
    jobs = [(m, i % 2 == 0) for i, m in enumerate(BC.sweep_models())]
    wants = [BN.Want(m, max_pq=BC.SWEEP_MAX, max_pairs=BC.SWEEP_MAX, with_bk=bk) for m, bk in jobs]
    for w in wants:
        kinds += np.bincount(w.bn.bn_kind, minlength=6)
    assert (kinds[1:] > 0).all(), kinds.tolist()                                  # a condition on the inputs: every kind occurs
    for i, ((m, bk), w) in enumerate(zip(jobs, wants)):
        d = NodeDevice(spf_ctx, m)
        try:
            assert_equal(d.backup_node([w], with_bk=bk), [w], tag=i)
        finally:
            d.free()
    ch = FC.chain("a")
    assert not ch.paths(spf_ctx.mode)[1].pool_compact                             # the patched handle's mirror is out of order
    g5, S5, t5 = BC.five_ring()
    pm = C.Model(ch.steps[1].graph, ch.steps[1].prot, t5)
    assert np.array_equal(ch.model(1).roots, pm.roots) and ch.model(1).W == pm.W
    w = BN.Want(pm)
    G = spf_ctx.upload(*ch.steps[0].graph, ch.maxp)
    try:
        G.patch(ch.steps[1].patch.vs, ch.steps[1].patch.rows, ch.steps[1].patch.flags)
        d = NodeDevice.__new__(NodeDevice)
        d.ctx, d.model, d.tab, d.protect = spf_ctx, pm, PatchedTables(spf_ctx, G, ch.model(1)), protect_of(pm)
        assert_equal(d.backup_node([w]), [w], tag="patched")
    finally:
        G.free()
