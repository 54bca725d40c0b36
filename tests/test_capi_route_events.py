"""hspf_routes_events on the CPU side: the symbols, the unchanged ABI number, the constants, and apply_route_events — the
documented meaning of the stream — on hand-made tables."""
import ctypes
import os
import re

import numpy as np
import pytest

from holo_amd import _lib as L
from holo_amd import engine as E
from holo_amd import routes as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
INF = 0xFFFFFFFF


def test_library_exports_the_event_calls_and_keeps_abi_8():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ("hspf_routes_events", "hspf_routes_events_rest"):
        assert getattr(raw, name) is not None
        assert name in [s[0] for s in L.SYMBOLS]
    assert lib.hspf_abi_version() == 8


def test_header_constants_equal_the_python_ones():
    text = open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read()
    words = int(re.search(r"#define\s+HSPF_EVENT_REC_WORDS\s+(\d+)u", text).group(1))
    silent = int(re.search(r"#define\s+HSPF_EV_SILENT\s+0x([0-9a-fA-F]+)u", text).group(1), 16)
    assert words == E.EVENT_REC_WORDS == 8
    assert silent == E.EV_SILENT
    assert int(re.search(r"#define\s+HSPF_ABI_VERSION\s+(\d+)", text).group(1)) == 8


def _record(root, prefix, action, new, old, W):
    """One record from (metric, entry, [mask words]) halves."""
    rec = [root, prefix, action, new[0], new[1], old[0], old[1], 0]
    for half in (new, old):
        for w in range(W):
            rec += [half[2][w] & 0xFFFFFFFF, half[2][w] >> 32]
    return rec


@pytest.mark.parametrize("W", [1, 2])
def test_apply_route_events_on_hand_made_tables(W):
    R, P = 2, 6
    hi = (1 << 63) | 5                                     # a mask word that needs its high half
    z = [0] * W
    m1 = [3] + [0] * (W - 1)
    m2 = [hi] + ([1 << 40] if W == 2 else [])
    bm = np.full((R, P), INF, np.uint32); be = np.full((R, P), NONE, np.uint32); nm = np.zeros((R, P, W), np.uint64)

    def put(r, p, metric, entry, mask):
        bm[r, p], be[r, p] = metric, entry
        nm[r, p] = np.array(mask, np.uint64)
    put(0, 1, 10, 4, m1)        # -> changed next hops: INSTALL
    put(0, 2, 20, 5, m1)        # -> gone: WITHDRAW
    put(0, 3, 30, 6, m1)        # -> loses all next hops: SILENT (route stays, mask empty)
    put(1, 0, 40, 7, z)         # had no next hops and vanishes: SILENT
    put(1, 5, 50, 8, m2)        # untouched
    #                           (0, 0): no route -> new route with next hops: INSTALL
    old = (bm.copy(), be.copy(), nm.copy())
    recs = np.array([
        _record(0, 0, E.DIFF_INSTALL, (11, 1, m2), (INF, NONE, z), W),
        _record(0, 1, E.DIFF_INSTALL, (10, 4, m2), (10, 4, m1), W),
        _record(0, 2, E.DIFF_WITHDRAW, (INF, NONE, z), (20, 5, m1), W),
        _record(0, 3, E.DIFF_SILENT, (31, 6, z), (30, 6, m1), W),
        _record(1, 0, E.DIFF_SILENT, (INF, NONE, z), (40, 7, z), W),
    ], np.uint64).astype(np.uint32)
    assert recs.shape == (5, E.EVENT_REC_WORDS + 4 * W)
    got = RT.apply_route_events((bm, be, nm), recs)
    assert got[0] is bm
    assert (bm[0, 0], be[0, 0]) == (11, 1) and nm[0, 0].tolist() == m2
    assert (bm[0, 1], be[0, 1]) == (10, 4) and nm[0, 1].tolist() == m2
    assert (bm[0, 2], be[0, 2]) == (INF, NONE) and nm[0, 2].tolist() == z
    assert (bm[0, 3], be[0, 3]) == (31, 6) and nm[0, 3].tolist() == z
    assert (bm[1, 0], be[1, 0]) == (INF, NONE) and nm[1, 0].tolist() == z
    touched = np.zeros((R, P), bool)
    touched[recs[:, 0], recs[:, 1]] = True
    for a, b in zip(old, (bm, be, nm)):
        assert np.array_equal(a[~touched], b[~touched])
    # the pack-layout view keeps INSTALL / WITHDRAW only, new half or old half
    new_pack = RT.events_as_pack_records(recs)
    old_pack = RT.events_as_pack_records(recs, old_half=True)
    assert new_pack.shape == old_pack.shape == (3, 6 + 2 * W)
    assert new_pack[:, :5].tolist() == [[0, 0, 1, 11, 1], [0, 1, 1, 10, 4], [0, 2, 2, INF, NONE]]
    assert old_pack[:, :5].tolist() == [[0, 0, 1, INF, NONE], [0, 1, 1, 10, 4], [0, 2, 2, 20, 5]]
    assert new_pack[0, 6:].tolist() == recs[0, 8:8 + 2 * W].tolist() and old_pack[2, 6:].tolist() == recs[2, 8 + 2 * W:].tolist()
    # an empty stream changes nothing; a stream for other tables is refused
    before = bm.copy()
    RT.apply_route_events((bm, be, nm), np.zeros((0, E.EVENT_REC_WORDS + 4 * W), np.uint32))
    assert np.array_equal(before, bm)
    with pytest.raises(ValueError):
        RT.apply_route_events((bm, be, nm), recs[:1])      # its old half says "no route", the table holds one now
    with pytest.raises(ValueError):
        RT.apply_route_events((bm, be, nm), np.zeros((1, E.EVENT_REC_WORDS + 4 * W + 1), np.uint32))
