"""Per-primary SRLG-safe backups of ECMP prefixes on the CPU side: the new symbol in header, ctypes table and library; the model
(tests/_backup_ecmp_srlg_model.py) pinned on hand cases with every array written out, against the plain ECMP model where no slot
has members, and against the CPU oracle's distances on the graph without S and without the protected primary's member links — so
that what the GPU tests compare against is checked independently of the engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import _backup_cases as BC
import _backup_ecmp_cases as EC
import _backup_ecmp_srlg_cases as C
import _backup_ecmp_srlg_model as BES
import _lfa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hspf_routes_backup_ecmp_srlg_device"
FAR = 1 << 24


def test_header_ctypes_and_library_agree_on_the_symbol():
    from holo_amd import build, _lib
    from holo_amd import engine as E
    build.build_lib()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"\bint " + NAME + r"\(([^;]*?)\);", hdr, re.S)
    assert m, NAME + " is not declared"
    assert len(m.group(1).split(",")) == 17 and hasattr(lib, NAME)
    assert table[NAME][0] is ctypes.c_int and len(table[NAME][1]) == 17
    assert lib.hspf_abi_version() == 8                                   # additions only
    assert int(re.search(r"#define HSPF_BK_ECMP_SRLG_COVERAGE_WORDS\s+(\d+)u", hdr).group(1)) == E.BK_ECMP_SRLG_COVERAGE_WORDS == BES.COVERAGE_WORDS
    assert (BES.SRLG_PRIMARY, BES.PAIR_REFUSED, BES.SRLG_REFUSED, BES.SAFE_REPAIRS) == (E.BK_SRLG_PRIMARY, E.BK_SRLG_PAIR_REFUSED, E.LFA_SRLG_REFUSED, E.LFA_SRLG_SAFE_REPAIRS)


def test_a_null_context_is_an_argument_error_as_for_the_other_frr_calls():
    from holo_amd import _lib
    lib = _lib.load()
    total = ctypes.c_uint64(7)
    out = _lib.HspfBackupEcmpOut()
    prot = (_lib.HspfLfaProtect * 1)()
    srlg = (_lib.HspfSrlg * 1)()
    rc = getattr(lib, NAME)(None, 4, 1, 1, None, None, None, prot, srlg, 1, 0, None, None, None, 0, ctypes.byref(out), ctypes.byref(total))
    assert rc == -1 and total.value == 7                                  # HSPF_E_INVAL


def test_the_python_layer_has_the_call_and_the_switch_accepts_groups():
    import inspect
    from holo_amd import engine as E
    assert "srlgs" in inspect.signature(E.SpfContext.routes_backup_ecmp_srlg_device).parameters
    assert "srlgs" in inspect.signature(E.SpfContext._backup_ecmp_tail).parameters and "ecmp" in inspect.signature(E.SpfContext._backup_srlg).parameters


# ---- hand cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.HAND))
def test_model_on_the_hand_cases(name):
    case = C.HAND[name]()
    model = C.model_of(case)
    for exp in case["expect"]:
        lf, ti = exp[0], exp[1]
        got = BES.want(model, lf, ti is not None, tilfa=None if ti is None else [ti])[0]
        for f, w in zip(BES.FIELDS, C.expected(exp)):
            assert np.array_equal(getattr(got, f), w), (name, lf, f, getattr(got, f), w)


def test_conduit_pair_is_where_the_plain_ecmp_call_hands_each_link_the_other():
    case = C.conduit_pair()
    model = C.model_of(case)
    assert BES.want_plain(model)[0].entries(0) == case["plain"]
    assert [e[2] for e in BES.want(model, 0, False)[0].entries(0)] == [2, 2]
    assert model.mems[0].mem_ptr.tolist() == [0, 1, 2, 2]                # each uplink has the other as its one member, C has none


def test_multihomed_is_admitted_by_the_per_vertex_reasoning():
    """d(C, X) = 2 < d(C, a) + w + d(Y, X) = 0 + 1 + 3: C's shortest path to the attaining VERTEX avoids the member C -> Y."""
    model = C.model_of(C.multihomed())
    d = model.fwd.dist
    row = {int(v): i for i, v in enumerate(model.roots)}
    assert int(d[row[3], 4]) == 2 and int(d[row[5], 4]) == 3 and int(d[row[3], 5]) == 1


# ---- no members ---------------------------------------------------------------------------------------------------------------

def test_without_members_the_model_is_the_plain_ecmp_model_on_every_array():
    for seed in EC.GPU_SEEDS:
        g, S, t = EC.random_multihomed(seed)
        model = C.Model(g, [S], *C.SC.group(g), t, no_members=True)
        for lf in (0, BES.SAFE_REPAIRS, M.IGNORE_OVERLOAD):
            for rem in (True, False):
                ti = [x[2] for x in model.frr(lf)] if rem else None
                got, plain = BES.want(model, lf, rem)[0], BES.want_plain(model, lf, ti)[0]
                for f in BES.FIELDS[:-1]:
                    assert np.array_equal(getattr(got, f), getattr(plain, f)), (seed, lf, rem, f)
                assert np.array_equal(got.eb_coverage[:8], plain.eb_coverage) and not got.eb_coverage[8:].any()


# ---- the independent check ----------------------------------------------------------------------------------------------------

def test_a_chosen_alternates_distance_to_the_prefix_survives_the_loss_of_s_and_of_the_primarys_member_links():
    """Symmetric costs >= 1, no overloaded router.  The prefix becomes a vertex X_p behind its advertisers
    (tests/_backup_cases.py).  For every HSPF_BK_LFA entry whose primary h has members: on the graph WITHOUT S and without the
    member links of h the CPU oracle's distance from N_k to X_p equals d_{N_k}(p) — no shortest path of the alternate needs S or
    a link of h's group."""
    from oracle import graph_oracle as go
    checked = 0
    for seed in C.SYM_SEEDS:
        g, S, (gp, gr), t = C.symmetric(seed)
        model = C.Model(g, [S], gp, gr, t)
        c, mem = model.cands[0], model.mems[0]
        w = BES.want(model, 0, False)[0]
        (rp, col, met, vf), xs = BC.augmented(g, S, t)
        for e in range(w.total):
            p, h, k = int(w.eb_prefix[e]), int(w.eb_primary[e]), int(w.eb_slot[e])
            if w.eb_kind[e] != BES.LFA or not len(mem.of(h)) or p not in xs:
                continue
            gone = {(int(mem.tail[i]), int(mem.pos[i])) for i in mem.of(h)}
            # (a member is ONE directed link: it is priced out of every path, at 2^24, instead of deleted, so that its reverse
            # link keeps passing the oracle's two-way check)
            links = [(u, int(col[x]), FAR if (u, x - int(rp[u])) in gone else int(met[x])) for u in range(len(vf)) for x in range(int(rp[u]), int(rp[u + 1]))
                     if u != S and int(col[x]) != S]
            g2 = M.csr(len(vf), links)
            g2[3][:] = vf
            d = go.run(*g2, 0xFFFFFFFF, np.array([int(c.nbr[k])], np.uint32), 0, go.MAP).dist[0]
            assert int(d[xs[p]]) == int(w.eb_metric[e]) - int(c.cost[k]), (seed, e, p, h, k)
            checked += 1
    assert checked > 40, checked


def test_the_seeds_reach_every_kind_every_new_flag_bit_and_every_new_coverage_word():
    """(the seeds were chosen on the CPU; HSPF_BK_SRLG_PAIR_REFUSED also comes from forged pairs)"""
    kinds, bits, cov = set(), 0, np.zeros(BES.COVERAGE_WORDS, np.int64)
    for seed in C.GPU_SEEDS:
        g, S, (gp, gr), t = C.seeded(seed)
        model = C.Model(g, [S], gp, gr, t)
        for lf, rem in ((0, True), (BES.SAFE_REPAIRS, True), (0, False)):
            w = BES.want(model, lf, rem)[0]
            assert w.total > 0 and w.eb_coverage[8] > 0
            kinds |= {int(k) for k in w.eb_kind}
            bits |= int(np.bitwise_or.reduce(w.eb_flags))
            cov += w.eb_coverage
    assert kinds == {BES.LFA, BES.NODE, BES.PAIR, BES.NOTHING}
    assert bits == BES.NODE_PROTECT | BES.DOWNSTREAM | BES.EA_PRIMARY | BES.SRLG_PRIMARY | BES.SRLG_REFUSED | BES.PAIR_REFUSED
    assert (cov[8:] > 0).all(), cov
