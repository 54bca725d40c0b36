"""hspf_lfa_device, hspf_rlfa_device and hspf_tilfa_device on a graph handle that has been through hspf_graph_patch: ONE uploaded
forward graph per chain, patched step by step (tests/_frr_chains.py), the three calls after every step against the plain-Python
models over the CPU oracle's SPTs of the SPLICED CSR — every output array, bit for bit, with the assert_equal helpers of the
three fresh-upload files.  hspf_tilfa_device reads the raw CSR through the ping-pong copy a structural patch swaps (and an arena
growth resets) and stages the two-way byte per link from the host mirror, which a patch keeps by a row scan, by a fetch from the
device or by the full rebuild, and repacks into vertex order when a patch changed a row's length; hspf_rlfa_device reads the
vertex flags a patch rewrites in place.  A stale byte or a wrong row order offers a forced adjacency that should not be: counts
and winners change, nothing faults.

After every step the build mode the handle reports is the one the patch model predicts for the engine configuration: the
intended path ran.  What a step is meant to change is asserted on the MODEL before anything is compared.  The reverse graph is
not under test: the transpose of the spliced CSR is uploaded fresh for every step.  One step per chain is also compared with the
same calls on a fresh upload of the spliced CSR in the same context, so that a difference the models report too can be told
from one the patch made.  Each step prints one line (`pytest -s`): engine, build mode, whether the mirror's pool was compact
and whether its flags were fetched."""
import numpy as np
import pytest

import _frr_chains as F
import _rlfa_model as R
import _tilfa_model as T
from _engines import hub_engines
from test_gpu_lfa import run_lfa
from test_gpu_rlfa import Tables, assert_equal as assert_rlfa
from test_gpu_tilfa import assert_equal as assert_tilfa, run_tilfa

pytestmark = pytest.mark.gpu

LFA_FIELDS = ("alt_slot", "alt_metric", "alt_flags", "cand_mask", "node_mask", "coverage")


class PatchedTables:
    """The rows of `roots` on the device: the forward set from the PATCHED handle, rdist from a fresh upload of the product's
    transpose of the spliced CSR (the attributes run_lfa / run_rlfa / run_tilfa read)."""

    def __init__(self, ctx, G, model):
        import torch
        from holo_amd import engine as E
        rp, col, met, vf = model.graph
        dev = torch.device("cuda:0")
        self.G, self.n, self.R, self.W = G, len(vf), len(model.roots), model.W
        assert G.mask_words(model.roots) <= self.W                               # (walks the patched host mirror)
        self.dist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
        self.flags = torch.empty((self.R, self.n), dtype=torch.int16, device=dev)
        self.mask = torch.empty((self.R, self.n, self.W), dtype=torch.int64, device=dev)
        self.rdist = torch.empty((self.R, self.n), dtype=torch.int32, device=dev)
        ctx.run_device(G, model.roots, 0, dist_ptr=self.dist.data_ptr(), flags_ptr=self.flags.data_ptr(), mask_ptr=self.mask.data_ptr(),
                       mask_words=self.W)
        GT = ctx.upload(*E.csr_transpose(rp, col, met, vf), vf, model.maxp)
        try:
            ctx.run_device(GT, model.roots, 0, dist_ptr=self.rdist.data_ptr())
        finally:
            GT.free()


def protect_of(model):
    """[(root_row, product candidates, nbr_row)] from the spliced CSR; the product's table is the model's."""
    from holo_amd import engine as E
    out = []
    for r, mc, rr, nr in zip(model.prot, model.cands, model.root_row, model.nbr_row):
        pc = E.lfa_candidates(*model.graph, r)
        for a, b in ((pc.nbr, mc.nbr), (pc.cost, mc.cost), (pc.root_link, mc.root_link), (pc.cflags, mc.cflags)):
            assert np.array_equal(a, b)
        out.append((rr, pc, nr))
    return out


def three_calls(ctx, tab, model, lfa_flags):
    """(LFA's six arrays by name, RLFA's fields with the space tables, TI-LFA's fields) of every protected root of the model."""
    protect = protect_of(model)
    alts = np.stack([w[0].alt_flags for w in model.want(lfa_flags)])
    lfa = dict(zip(LFA_FIELDS, run_lfa(ctx, tab, protect, lfa_flags)))
    rl, ti = run_tilfa(ctx, tab, protect, lfa_flags, alts)
    return lfa, rl, ti


def compare(got, model, lfa_flags, tag):
    lfa, rl, ti = got
    for i, (wl, wr, wt) in enumerate(model.want(lfa_flags)):
        for name in LFA_FIELDS:
            g, w = lfa[name][i], getattr(wl, name)
            assert g.shape == w.shape and np.array_equal(g, w), (tag, i, name, np.argwhere(g != w)[:8].tolist())
        assert_rlfa(rl, wr, i, tag=(tag, i))
        assert_tilfa(rl, ti, wr, wt, i, tag=(tag, i))


def same_outputs(a, b, tag):
    for da, db in zip(a, b):
        for name in da:
            assert np.array_equal(da[name], db[name]), (tag, "patched handle and fresh upload differ", name, np.argwhere(da[name] != db[name])[:8].tolist())


def convenience(ctx, G, model, tag):
    """SpfContext.tilfa() on the patched handle, with and without the transposed run: candidates and CSR come from SpfGraph's
    pending numpy splices; every field of all four results."""
    (wl, wr, wt), mc = model.want()[0], model.cands[0]
    for symmetric in (False, True):
        cand, lfa, rl, ti = ctx.tilfa(G, model.prot[0], symmetric=symmetric)
        for name in ("nbr", "cost", "root_link", "cflags"):
            assert np.array_equal(getattr(cand, name), getattr(mc, name)), (tag, symmetric, name)
        assert cand.root == mc.root and lfa.cand_mask is None and lfa.node_mask is None
        for name in ("alt_slot", "alt_metric", "alt_flags", "coverage"):
            assert np.array_equal(getattr(lfa, name)[0], getattr(wl, name)), (tag, symmetric, name)
        for name in R.FIELDS:
            assert np.array_equal(getattr(rl, name)[0], getattr(wr, name)), (tag, symmetric, name)
        for name in T.FIELDS:
            assert np.array_equal(getattr(ti, name)[0], getattr(wt, name)), (tag, symmetric, name)


def run_chain(ctx, chain):
    paths = chain.paths(ctx.mode)
    G = None
    try:
        for i, (step, path) in enumerate(zip(chain.steps, paths)):
            model = chain.model(i)
            chain.check(i)                                       # non-vacuity: on the MODEL, before anything is compared
            tag = (chain.name, i, step.tag, ctx.mode)
            if step.patch is None:
                G = ctx.upload(*model.graph, chain.maxp)
            else:
                G.patch(step.patch.vs, step.patch.rows, step.patch.flags)
            mode = int(G.export("build_mode")[0])
            print(f"\nFRRPATCHED chain {chain.name} | step {i}: {step.tag} | engine={ctx.mode} model_mode={path.build_mode} gpu_mode={mode} "
                  f"pool_compact={path.pool_compact} flags_fetched={path.flags_fetched}", flush=True)
            assert mode == path.build_mode, (tag, f"build_mode {mode}, the model says {path.build_mode}")
            tab = PatchedTables(ctx, G, model)
            first = None
            for lf in step.lfa_flags:
                got = three_calls(ctx, tab, model, lf)
                first = first or got
                compare(got, model, lf, tag + (lf,))
            if step.parity:
                fresh = Tables(ctx, model.graph, chain.maxp, model.roots, 0, model.W)
                try:
                    same_outputs(first, three_calls(ctx, fresh, model, step.lfa_flags[0]), tag)
                finally:
                    fresh.free()
            if step.convenience:
                convenience(ctx, G, model, tag)
    finally:
        if G is not None:
            G.free()


@hub_engines
def test_one_way_then_two_way_then_one_way_again(spf_ctx):
    """(a) and (e).  The five-ring, S = 2, the slot of E = 3.  Row 1 gains the one-way link 1 -> 4 (the row grows: the mirror's pool
    is out of order from here on, hspf_tilfa_device repacks it): nothing may change, 1 -> 4 is not offered.  Row 4 ALONE gains
    4 -> 1: the byte of 1 -> 4 sits in row 1, which the patch does not replace — the single node 4 at 3, three pairs, (1, 4) among
    them.  Row 4 loses the link again (a hole in the pool): back to step 1's.  Then costs only: the pair at 9.  Steps 2 and 3
    also through SpfContext.tilfa(), with and without the transposed run."""
    chain = F.chain("a")
    default = chain.paths("default")
    assert [p.build_mode for p in default[1:]] == [F.pm.MODE_INCREMENTAL] * 3 + [F.pm.MODE_COST] and not any(p.pool_compact for p in default[1:])
    assert all(p.flags_fetched for p in chain.paths("hubsort")[1:4])
    run_chain(spf_ctx, chain)


@hub_engines
def test_overload_set_and_cleared_through_a_patch(spf_ctx):
    """(b) ring8, S = 0, the slot of E = 1: row 4 replaced by itself with HSPF_VF_NO_TRANSIT set (the vertex flags are rewritten in
    place): the single node 4 goes, with HSPF_LFA_IGNORE_OVERLOAD it stays; cleared again: back.  The space tables at every
    step, under both flags."""
    run_chain(spf_ctx, F.chain("b"))


@hub_engines
def test_shifted_rows_and_a_second_tile(spf_ctx):
    """(c) The 300-ring with six chords: a chord between a vertex below and one beyond 256 shifts every later row of the raw CSR,
    the winners' rows lie behind both splices; another chord is removed, with two protected roots on one table set; two rows
    are replaced in one patch, one of them the winner's in reverse order: the forced link's position moves."""
    run_chain(spf_ctx, F.chain("c"))


@hub_engines
def test_arena_growth_then_structural_steps(spf_ctx):
    """(d) A patch the model reports as `grown` (the raw CSR and the vertex flags move to a new arena, the ping-pong index is
    reset), with the pool out of order across it in the default configuration; an incremental step from the reset state; a
    step whose flags come back from the device in every configuration."""
    chain = F.chain("d")
    assert all(chain.paths(e)[1].decision.grown for e in F.ENGINES) and chain.paths("default")[2].build_mode == F.pm.MODE_INCREMENTAL
    run_chain(spf_ctx, chain)
