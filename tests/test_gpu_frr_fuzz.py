"""A slice of the randomised differential run of the fast-reroute family (tools/gpu_fuzz.py, fuzz_frr) inside the GPU suite: per
seed one uploaded adversarial LSDB, one to four protected roots of different slot counts in ONE call of every device call of the
family (outputs pre-filled, the calls in a drawn order on one context, drawn flags / masks / space tables / alt_flags_in / max_pq /
prefix table), the LAN calls without LANs against the plain calls, the SpfContext chains for one root — and, on the patched
ranges, the same again after every hspf_graph_patch, with the build mode the patch model predicts.  Every array against the
plain-Python models over the CPU oracle's SPTs, bit for bit.  The seed ranges, their non-vacuity counters and the cost of their
model side are pinned by tests/test_host_frr_fuzz.py, which needs no GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from _engines import both_engines, hub_engines  # noqa: E402
from test_host_frr_fuzz import PATCHED, PLAIN  # noqa: E402

pytestmark = pytest.mark.gpu


@both_engines
@pytest.mark.parametrize("first", sorted(PLAIN))
def test_random_frr_against_the_models(spf_ctx, first):
    import gpu_fuzz
    ok, runs = gpu_fuzz.fuzz_frr(spf_ctx, first, PLAIN[first], verbose=False, patches=False)
    assert ok == runs and runs >= PLAIN[first]


@hub_engines
@pytest.mark.parametrize("first", sorted(PATCHED))
def test_random_frr_on_patched_handles(spf_ctx, first):
    """(a build mode other than the patch model's is a mismatch of the run: fuzz_frr reports it as call=hspf_graph_patch)"""
    import gpu_fuzz
    ok, runs = gpu_fuzz.fuzz_frr(spf_ctx, first, PATCHED[first], verbose=False, patches=True)
    assert ok == runs and runs >= PATCHED[first]
