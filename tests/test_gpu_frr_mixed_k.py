"""Three protected roots with 65, 3 and 1 first-hop slots in ONE call of hspf_lfa_device, hspf_rlfa_device, hspf_tilfa_device and
hspf_routes_backup_device.  The staged candidate tables of the roots lie back to back (holo_amd/csrc/spf_frr_common.hip.h): with
these K the slot arrays of the second and third root start at words 24 + 6 * 65 and 24 + 6 * 68 of the block, their scalars at
words 65 * 66 and 65 * 66 + 12 — a kernel that takes a root's table from the wrong header word reads another root's columns.
The hub has 64 spokes and one link into the grid, not 70 spokes: its 65 slots are what the case is about (asserted on the model).
65 slots make two mask words, so hspf_lfa_device runs its any-K instantiation over all three roots.  Every output array of the
four calls against the plain-Python models over the CPU oracle's SPTs, bit for bit, with the helpers of the four per-call files."""
import numpy as np
import pytest

import _backup_cases as C
import _lfa_model as M
from test_gpu_backup import Device, assert_equal as assert_backup, random_table
from test_gpu_lfa import run_lfa
from test_gpu_rlfa import assert_equal as assert_rlfa
from test_gpu_tilfa import assert_equal as assert_tilfa, run_tilfa

pytestmark = pytest.mark.gpu

LFA_FIELDS = ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask", "coverage")
SPOKES, LEAVES, COLS, ROWS = 64, 4, 16, 15
HUB, LEAF, EDGE = 0, SPOKES, SPOKES + 1 + 5                  # the hub | its last spoke | the sixth vertex of the grid's first row
N_PFX = 65


def hub_on_grid(seed=7):
    """Vertex 0 with 64 spokes — the first 60 on a ring among themselves, the last 4 leaves — and one link into a 16 x 15 grid
    (vertices 65 ..), seeded costs: 305 vertices, two tiles."""
    r = np.random.default_rng(seed)
    cost = lambda lo, hi: int(r.integers(lo, hi))      # noqa: E731
    ring = SPOKES - LEAVES
    und = [(HUB, v, cost(5, 12)) for v in range(1, SPOKES + 1)] + [(v, v % ring + 1, cost(1, 6)) for v in range(1, ring + 1)]
    g0 = SPOKES + 1
    at = lambda y, x: g0 + y * COLS + x      # noqa: E731
    for y in range(ROWS):
        for x in range(COLS):
            if x + 1 < COLS:
                und.append((at(y, x), at(y, x + 1), cost(1, 10)))
            if y + 1 < ROWS:
                und.append((at(y, x), at(y + 1, x), cost(1, 10)))
    und += [(HUB, at(7, 8), cost(5, 12)), (1, at(0, 0), cost(5, 12))]      # the hub's 65th slot; a second way into the grid
    return M.csr(g0 + ROWS * COLS, M.both(und))


def test_roots_of_65_3_and_1_slots_in_one_call(spf_ctx):
    g = hub_on_grid()
    model = C.Model(g, [HUB, EDGE, LEAF], random_table(np.random.default_rng(11), len(g[3]), N_PFX))
    frr, want_bk = model.frr(0), model.want(0, True)
    # non-vacuity, on the MODEL: the three K, two mask words, slots of the second word in use, every root has something to say
    assert [len(c.nbr) for c in model.cands] == [65, 3, 1] and model.W == 2 and model.table.n == N_PFX
    assert frr[0][0].cand_mask[:, 1].any() and all(f[0].coverage[0] > 0 for f in frr)
    assert frr[0][0].coverage[2] > 0 and frr[1][0].coverage[2] > 0 and frr[2][0].coverage[2] == 0      # a leaf has no alternate
    assert len({tuple(w.bk_kind.tolist()) for w in want_bk}) == 3
    d = Device(spf_ctx, model)
    try:
        lfa = dict(zip(LFA_FIELDS, run_lfa(spf_ctx, d.tab, d.protect)))
        rl, ti = run_tilfa(spf_ctx, d.tab, d.protect, 0, np.stack([f[0].alt_flags for f in frr]))
        for i, (wl, wr, wt) in enumerate(frr):
            for name in LFA_FIELDS:
                got, want = lfa[name][i], getattr(wl, name)
                assert got.shape == want.shape and np.array_equal(got, want), (i, name, np.argwhere(got != want)[:8].tolist())
            assert_rlfa(rl, wr, i, tag=i)
            assert_tilfa(rl, ti, wr, wt, i, tag=i)
        assert_backup(d.backup(model.table, 0, True), want_bk)
    finally:
        d.free()
