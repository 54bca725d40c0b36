"""The protection modes of one kernel family against each other on the GPU: with an empty member table the SRLG call, and with no
LAN slot the LAN call, write what the plain call writes — every alt_* / bk_* array and both sets bit for bit, and the plain call's
coverage words (5 for the alternates, 7 for the backups) with zeros behind them.  One body per family is what guarantees it.
Shapes: a hub of 9 neighbours (two chunks of 8 candidates, one mask word) and one of 65 (two mask words, the kernels without the
LDS tables), 257 prefixes (a second, partial tile), tilfa_dev NULL; each with one-primary and ECMP destinations."""
import numpy as np
import pytest

import _lfa_model as M
import _srlg_model as SM
from test_gpu_backup import HUB_SEEDS, OUT, _torch_dt
from test_gpu_backup_srlg import random_table
from test_gpu_lfa_lan import run_backup, run_lfa
from test_gpu_rlfa import Tables, hub
from test_gpu_srlg import plan, product_members, run_lfa_srlg

pytestmark = pytest.mark.gpu

N_PFX = 257


class Hub:
    """Root 0 of the hub of k on the device, with an empty member table and no LAN slot."""

    def __init__(self, ctx, k):
        from holo_amd import engine as E
        self.graph = hub(k, HUB_SEEDS[k])
        gp, gr = SM.groups_csr(len(self.graph[1]), {})
        roots, ((r, c, nbr_row, mem),) = plan(self.graph, [0], gp, gr, no_members=True)
        K = len(c.nbr)
        assert int(np.count_nonzero(c.nbr != M.NONE)) == k and not np.diff(mem.mem_ptr).any()
        self.W = (K + 63) // 64
        self.tab = Tables(ctx, self.graph, 0xFFFFFFFF, roots, 0, self.W)
        self.protect = [(r, E.lfa_candidates(*self.graph, 0), nbr_row)]
        self.srlgs = [product_members(mem)]
        self.lans = [(np.full(K, M.NONE, np.uint32), np.zeros(K, np.uint32))]


def same(got, plain, fields, words, tag):
    for name in fields:
        assert got[name].dtype == plain[name].dtype and np.array_equal(got[name], plain[name]), (tag, name)
    cov = "bk_coverage" if "bk_coverage" in plain else "coverage"
    assert plain[cov].shape[1] == words and np.array_equal(got[cov][:, :words], plain[cov]) and not got[cov][:, words:].any(), (tag, cov)


@pytest.mark.parametrize("k", [9, 65])
@pytest.mark.parametrize("lfa_flags", [0, M.IGNORE_OVERLOAD])
def test_alternates_of_the_srlg_and_lan_calls_with_nothing_to_avoid_are_the_plain_ones(spf_ctx, k, lfa_flags):
    h = Hub(spf_ctx, k)
    try:
        plain = run_lfa(spf_ctx, h.tab, h.protect, None, lfa_flags, plain=True)
        fl = plain["alt_flags"][0]
        assert (fl & 0x02).any() and ((fl & 0x03) == 0x01).any() and (fl & 0x04).any() and h.W == (1 if k <= 64 else 2)      # ECMP, one primary, an alternate
        fields = ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask")
        same(run_lfa_srlg(spf_ctx, h.tab, h.protect, h.srlgs, lfa_flags), plain, fields, 5, "srlg")
        same(run_lfa(spf_ctx, h.tab, h.protect, h.lans, lfa_flags), plain, fields, 5, "lan")
    finally:
        h.tab.free()


def run_backup_srlg(ctx, h, t, routes, lfa_flags):
    """hspf_routes_backup_srlg_device without repairs (tilfa_dev NULL), every output pre-filled with 7."""
    import torch
    tab, NP = h.tab, t.n
    shapes = dict(bk_kind=(1, NP), bk_primary=(1, NP), bk_slot=(1, NP), bk_metric=(1, NP), bk_flags=(1, NP), bk_cand_mask=(1, NP, tab.W),
                  bk_node_mask=(1, NP, tab.W), bk_coverage=(1, 10))
    out = {k: torch.full(sh, 7, dtype=_torch_dt(OUT[k]), device="cuda:0") for k, sh in shapes.items()}
    torch.cuda.synchronize()                                   # the fills run on torch's stream, the call on the context's
    ctx.routes_backup_srlg_device(tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), h.protect, h.srlgs, t.ptr, t.vertex,
                                  t.metric, tilfa=None, routes=routes, flags=t.flags, lfa_flags=lfa_flags, **{k + "_ptr": x.data_ptr() for k, x in out.items()})
    return {k: x.cpu().numpy().view(OUT[k]) for k, x in out.items()}


@pytest.mark.parametrize("k", [9, 65])
@pytest.mark.parametrize("lfa_flags", [0, M.IGNORE_OVERLOAD])
def test_backups_of_the_srlg_and_lan_calls_with_nothing_to_avoid_are_the_plain_ones(spf_ctx, k, lfa_flags):
    import torch
    h = Hub(spf_ctx, k)
    try:
        tab, t = h.tab, random_table(np.random.default_rng(k), k + 1, N_PFX)
        plain = run_backup(spf_ctx, tab, h.protect, None, t, lfa_flags, plain=True)
        kinds = plain["bk_kind"][0]
        assert (kinds == 2).any() and (kinds == 3).any() and kinds[N_PFX - 1] >= 2              # ECMP, an alternate; the last lane of the partial tile has sets
        fields = ("bk_kind", "bk_primary", "bk_slot", "bk_metric", "bk_flags", "bk_cand_mask", "bk_node_mask")
        same(run_backup(spf_ctx, tab, h.protect, h.lans, t, lfa_flags), plain, fields, 7, "lan")
        r = [torch.empty((tab.R, t.n) + sh, dtype=dt, device="cuda:0") for sh, dt in (((), torch.int32), ((), torch.int32), ((tab.W,), torch.int64))]
        spf_ctx.routes_device(tab.n, tab.R, tab.W, tab.dist.data_ptr(), tab.flags.data_ptr(), tab.mask.data_ptr(), t.ptr, t.vertex, t.metric, flags=t.flags,
                              best_metric_ptr=r[0].data_ptr(), best_entry_ptr=r[1].data_ptr(), nexthop_mask_ptr=r[2].data_ptr())
        same(run_backup_srlg(spf_ctx, h, t, tuple(x.data_ptr() for x in r), lfa_flags), plain, fields, 7, "srlg")
    finally:
        h.tab.free()
