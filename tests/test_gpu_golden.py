"""GPU parity against the reference's own recorded answers: holo_amd.isis on the HIP engine
(through the C ABI) must reproduce the `local-rib` of every IS-IS conformance fixture, and its
batched multi-root SPTs must equal the literal restatement of compute_spt vertex by vertex."""
import glob
import json
import os

import pytest

from holo_amd import isis as H
from oracle import isis_ref as R
from test_host_isis import check_spts_against_ref

from _engines import both_engines  # noqa: E402

pytestmark = [pytest.mark.gpu, both_engines]

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ISIS = sorted(glob.glob(os.path.join(GOLD, "isis", "*.json"))) + sorted(glob.glob(os.path.join(GOLD, "isis_steps", "*.json")))


@pytest.mark.parametrize("path", ISIS, ids=[os.path.basename(p)[:-5] for p in ISIS])
def test_isis_compute_spf_on_gpu_reproduces_reference_local_rib(spf_ctx, path):
    vec = json.load(open(path))
    inst = H.Instance.from_vector(vec)
    want = sorted(vec["rib"], key=lambda r: R._net_key(r["prefix"]))
    assert H.compute_spf(inst, spf_ctx) == want


@pytest.mark.parametrize("path", ISIS, ids=[os.path.basename(p)[:-5] for p in ISIS])
def test_isis_batched_roots_on_gpu_match_literal_restatement(spf_ctx, path):
    vec = json.load(open(path))
    check_spts_against_ref(vec, H.Instance.from_vector(vec), spf_ctx)


# ---- OSPFv2 -----------------------------------------------------------------------------------------
from test_host_ospf import OSPF, check_ospf_vector      # noqa: E402


@pytest.mark.parametrize("path", OSPF, ids=[os.path.basename(p)[:-5] for p in OSPF])
def test_ospfv2_run_area_on_gpu_reproduces_reference_intra_area_rib(spf_ctx, path):
    check_ospf_vector(json.load(open(path)), spf_ctx)


# ---- OSPFv3 -----------------------------------------------------------------------------------------
from test_host_ospf import OSPF3, check_ospfv3_vector      # noqa: E402


@pytest.mark.parametrize("path", OSPF3, ids=[os.path.basename(p)[:-5] for p in OSPF3])
def test_ospfv3_run_area_on_gpu_reproduces_reference_intra_area_rib(spf_ctx, path):
    check_ospfv3_vector(json.load(open(path)), spf_ctx)


# ---- incremental LSDB -> CSR: step tests replayed through device-resident, patched graphs ---------
from test_host_isis_incremental import STEPS as ISIS_STEP_FILES, replay_isis_step      # noqa: E402
from test_host_ospf_incremental import STEPS as OSPF_STEP_FILES, replay_ospf_step      # noqa: E402


@pytest.mark.parametrize("path", ISIS_STEP_FILES, ids=[os.path.basename(p)[:-5] for p in ISIS_STEP_FILES])
def test_isis_step_on_gpu_through_patched_graphs(spf_ctx, path):
    replay_isis_step(json.load(open(path)), spf_ctx)


@pytest.mark.parametrize("path", OSPF_STEP_FILES, ids=[os.path.basename(p)[:-5] for p in OSPF_STEP_FILES])
def test_ospfv2_step_on_gpu_through_patched_graphs(spf_ctx, path):
    replay_ospf_step(json.load(open(path)), spf_ctx)


# ---- flooding::manet: one batched hop-count run per level, reflood lists answered from it ----------------------------
from test_host_manet import check_reflood_lists      # noqa: E402

MANET_FILES = sorted(glob.glob(os.path.join(GOLD, "isis", "*.json")))[::2]


@pytest.mark.parametrize("path", MANET_FILES, ids=[os.path.basename(p)[:-5] for p in MANET_FILES])
def test_manet_reflood_lists_on_gpu_match_literal_restatement(spf_ctx, path):
    assert check_reflood_lists(json.load(open(path)), spf_ctx) > 0


# ---- the same lists with the is_on_path queries answered from device-built ancestor sets (hspf_ancestors_device) ------
from holo_amd import isis as H                       # noqa: E402
from oracle import isis_ref as R                     # noqa: E402
from test_host_manet import ALGOS                    # noqa: E402


def check_reflood_lists_device(vec, engine, reflood_ref=R.reflood_list):
    inst = H.Instance.from_vector(vec)
    local = inst.config.system_id
    n_lists = 0
    for level in inst.config.levels():
        if level not in inst.lsdb:
            continue
        systems = sorted({l.system_id for l in inst.lsdb[level].iter()})
        lsp_ids = [(s, 0, 0) for s in systems] + [(systems[0], 3, 9), (systems[-1], 0, 17)]
        for name, algo_of in ALGOS.items():
            cache = H.manet_init_cache_device(level, inst, engine, algo_of)
            for tn in cache:
                for lsp_id in lsp_ids:
                    got = H.reflood_list_device(cache, local, tn, lsp_id)
                    want = reflood_ref(vec, level, local, tn, lsp_id, algo_of)
                    assert got == want, (level, name, tn.hex(), lsp_id)
                    n_lists += 1
    return n_lists


@pytest.mark.parametrize("path", MANET_FILES, ids=[os.path.basename(p)[:-5] for p in MANET_FILES])
def test_manet_reflood_lists_from_device_ancestor_sets(spf_ctx, path):
    assert check_reflood_lists_device(json.load(open(path)), spf_ctx) > 0


@pytest.mark.parametrize("block", range(2))
def test_manet_reflood_lists_from_device_ancestor_sets_random_instances(spf_ctx, block):
    from _random_isis import make
    total = 0
    for seed in range(2000 + block * 15, 2000 + block * 15 + 15):
        total += check_reflood_lists_device(make(seed), spf_ctx)
    assert total > 50


def wide_first_hop_instance():
    """An instance in the schema of _random_isis.make whose neighbour 2 has 70 p2p neighbours of its own: the local router 1, the
    local router's other neighbour 3, and 4 .. 71.  Routers 72 .. 79 sit behind two of those each, 80 and 81 behind the local router
    alone (the second hops it has to reflood to), 82 behind the local router and 3; the local router's adjacencies are 2 and 3.
    Root 2 has 70 first hops, root 3 has 70 second hops: both levels need a second set word."""
    from _random_isis import sid
    links = [(2, x) for x in [1] + list(range(3, 72))] + [(1, 3), (1, 80), (1, 81), (1, 82), (3, 82)]
    links += [(72 + i, 4 + 7 * i) for i in range(8)] + [(72 + i, 50 + 3 * i) for i in range(8)]
    n = 82
    lsps = []
    for r in range(1, n + 1):
        nbrs = [[f"{sid(b if a == r else a)}.00", 10] for a, b in links if r in (a, b)]
        lsps.append({"id": f"{sid(r)}.00-00", "flags": [], "protocols": [204, 142], "is_reach": [], "ext_is_reach": nbrs,
                     "mt": [], "mt_is_reach": [], "mt_ipv6": [], "ipv4_int": [], "ipv4_ext": [],
                     "ext_ipv4": [[f"10.0.{r}.0/24", 1, False]], "ipv6": []})
    ifaces = [{"name": f"eth{k}", "type": "point-to-point", "metric": {"1": 10, "2": 10},
               "adjacencies": [{"system_id": sid(other), "usage": "level-2", "state": "up", "ipv4": [f"10.1.{k}.{other}"],
                                "ipv6": [f"fe80::1:{k:x}:{other:x}"], "topologies": [0], "area_addrs": ["49.0000"]}]}
              for k, other in enumerate((2, 3), 1)]
    ifaces.append({"name": "lo", "type": "broadcast", "metric": {"1": 10, "2": 10}, "adjacencies": []})
    return {"proto": "isis", "source": "a neighbour with 70 first hops",
            "config": {"system_id": sid(1), "level_type": "level-2", "metric_type": {"1": "wide", "2": "wide"},
                       "afs": {"ipv4": True, "ipv6": False}, "mt_ipv6_unicast": False, "max_paths": 16, "att_ignore": False,
                       "area_addrs": ["49.0000"]},
            "interfaces": ifaces, "lsdb": {"2": lsps}, "rib": []}


_WIDE_REF = {}


def _wide_reflood_ref(vec, level, local, tn, lsp_id, algo_of):
    """R.reflood_list on the one instance above, computed once for all engine configurations."""
    key = (level, tn, lsp_id, algo_of)
    if key not in _WIDE_REF:
        _WIDE_REF[key] = R.reflood_list(vec, level, local, tn, lsp_id, algo_of)
    return _WIDE_REF[key]


def test_manet_reflood_lists_from_device_ancestor_sets_of_two_words(spf_ctx):
    """manet_init_cache_device's retry: the first hspf_ancestors_device call of either level returns HSPF_E_TOO_MANY_SLOTS at one
    word, the loop reads the level counts and calls again with two."""
    from oracle.isis_ref import parse_lan_id
    vec = wide_first_hop_instance()
    inst = H.Instance.from_vector(vec)
    cache = H.manet_init_cache_device(2, inst, spf_ctx)
    c2 = cache[parse_lan_id("0000.0000.0002.00")[0]]
    assert c2.fallback is None and len(c2.rnl_bit) == 70 and sorted(c2.rnl_bit.values()) == list(range(70))     # W == 2 for level 1
    c3 = cache[parse_lan_id("0000.0000.0003.00")[0]]
    assert c3.fallback is None and len(c3.second) > 64                                                          # ... and for level 2
    assert any(a1 >> 64 for _, _, a1 in c2.second)                       # a second hop behind a first hop of the second word
    assert check_reflood_lists_device(vec, spf_ctx, _wide_reflood_ref) > 0
    local = inst.config.system_id
    lists = [H.reflood_list_device(cache, local, tn, (tn, 0, 0)) for tn in cache]
    assert any(lists), "no reflood list of the instance has an entry"
