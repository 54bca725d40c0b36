"""The argument checks of the fast-reroute calls of both compiled layers, word for word: tests/cpp/frr_args_driver.cpp makes one call
per check of hspf::host::HipEngine (include/holo_spf_host.hpp) and of hspf::Engine (include/holo_spf_hip.hpp), each with exactly one
defect, on a 4-router ring, and prints what came back.  Every check stands in front of the first device call of its method.

EXPECTED is the driver's output against the headers of commit dd36015 (the parent of the commit that folded the two headers'
fast-reroute parts), run on an MI355X and pasted here: the texts a caller may have matched on did not move.  Not covered, because
they need a failed hipMemcpy or a failed C call to fire: the "hspf_<call>: " / "hspf_<call> (" texts behind a non-zero return code,
"hipMemcpy of the repairs: ", "hipMemcpy of the lists: ", and Error(k, "hspf_lfa_candidates" / "hspf_lfa_lan_candidates" /
"hspf_srlg_members" / "hspf_csr_transpose")."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "frr_args_driver")

EXPECTED = """\
raii.lfa.csr throws code=-1 Engine::lfa: the CSR is not the one the graph was uploaded from: invalid argument
raii.lfa_ecmp.csr throws code=-1 Engine::lfa_ecmp: the CSR is not the one the graph was uploaded from: invalid argument
raii.rlfa.csr throws code=-1 Engine::rlfa: the CSR is not the one the graph was uploaded from: invalid argument
raii.tilfa.csr throws code=-1 Engine::rlfa: the CSR is not the one the graph was uploaded from: invalid argument
raii.tilfa_node.csr throws code=-1 Engine::rlfa: the CSR is not the one the graph was uploaded from: invalid argument
raii.backup_routes.csr throws code=-1 Engine::rlfa: the CSR is not the one the graph was uploaded from: invalid argument
raii.tilfa_node.max_pq_0 throws code=-1 Engine::tilfa_node: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ: invalid argument
raii.tilfa_node.max_pq_over throws code=-1 Engine::tilfa_node: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ: invalid argument
raii.tilfa_node.max_pairs_0 throws code=-1 Engine::tilfa_node: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS: invalid argument
raii.tilfa_node.max_pairs_over throws code=-1 Engine::tilfa_node: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS: invalid argument
raii.backup_routes.no_pfx_ptr throws code=-1 Engine::backup_routes: malformed prefix table: invalid argument
raii.backup_routes.pfx_metric_short throws code=-1 Engine::backup_routes: malformed prefix table: invalid argument
raii.srlg_members.grp_ptr_short throws code=-1 srlg_members: grp_ptr needs one entry per link and one more: invalid argument
raii.lfa_lan_device.lans throws code=-1 lfa_lan_device: one hspf_lfa_lan per protected root: invalid argument
raii.rlfa_lan_device.lans throws code=-1 rlfa_lan_device: one hspf_lfa_lan per protected root: invalid argument
raii.routes_backup_lan_device.lans throws code=-1 routes_backup_lan_device: one hspf_lfa_lan per protected root: invalid argument
raii.lfa_srlg_device.srlgs throws code=-1 lfa_srlg_device: one hspf_srlg per protected root: invalid argument
raii.rlfa_srlg_device.srlgs throws code=-1 rlfa_srlg_device: one hspf_srlg per protected root: invalid argument
raii.routes_backup_srlg_device.srlgs throws code=-1 routes_backup_srlg_device: one hspf_srlg per protected root: invalid argument
raii.routes_backup_ecmp_srlg_device.srlgs throws code=-1 routes_backup_ecmp_srlg_device: one hspf_srlg per protected root: invalid argument
raii.tilfa_pc_device.pc_row throws code=-1 tilfa_pc_device: pc_row holds 64 * n_mask_words entries per protected root: invalid argument
host.lfa.empty ok supported=1 n_protected=0
host.lfa.cost throws lfa: the slot arrays of a protected root differ in length
host.lfa_ecmp.empty ok supported=1 n_protected=0
host.lfa_ecmp.cost throws lfa_ecmp: the slot arrays of a protected root differ in length
host.lfa_lan.empty ok supported=1 n_protected=0
host.lfa_lan.lans throws lfa_lan: one LfaLan per protected root
host.lfa_lan.cost throws lfa: the slot arrays of a protected root differ in length
host.lfa_lan.lan_row throws lfa_lan: lan / lan_row differ in length from the slot arrays
host.lfa_srlg.empty ok supported=1 n_protected=0
host.lfa_srlg.cost throws lfa: the slot arrays of a protected root differ in length
host.lfa_srlg.srlgs throws lfa_srlg: one Srlg per protected root
host.lfa_srlg.mem_ptr throws lfa_srlg: mem_ptr needs one entry per slot and one more
host.lfa_srlg.member throws lfa_srlg: a member column is shorter than mem_ptr says
host.rlfa.empty ok supported=1 n_protected=0
host.rlfa.reverse_run throws rlfa: the two runs differ in shape
host.rlfa.cost throws rlfa: the slot arrays of a protected root differ in length
host.rlfa_lan.empty ok supported=1 n_protected=0
host.rlfa_lan.lans throws rlfa_lan: one LfaLan per protected root
host.rlfa_lan.reverse_run throws rlfa_lan: the two runs differ in shape
host.rlfa_lan.cost throws rlfa_lan: the slot arrays of a protected root differ in length
host.rlfa_lan.lan_row throws rlfa_lan: lan / lan_row differ in length from the slot arrays
host.rlfa_srlg.empty ok supported=1 n_protected=0
host.rlfa_srlg.reverse_run throws rlfa_srlg: the two runs differ in shape
host.rlfa_srlg.cost throws rlfa_srlg: the slot arrays of a protected root differ in length
host.rlfa_srlg.srlgs throws rlfa_srlg: one Srlg per protected root
host.rlfa_srlg.mem_ptr throws rlfa_srlg: mem_ptr needs one entry per slot and one more
host.rlfa_srlg.member throws rlfa_srlg: a member column is shorter than mem_ptr says
host.tilfa.empty ok supported=1 n_protected=0
host.tilfa.reverse_run throws tilfa: the two runs differ in shape
host.tilfa.no_spaces throws tilfa: the RLFA result holds no space tables of this protect list
host.tilfa.cost throws tilfa: the slot arrays of a protected root differ in length
host.tilfa_pc.empty ok supported=1 n_protected=0
host.tilfa_pc.reverse_run throws tilfa_pc: the two runs differ in shape
host.tilfa_pc.no_spaces throws tilfa_pc: the RLFA result holds no space tables of this protect list
host.tilfa_pc.pc_row throws tilfa_pc: pc_row or pc_dist is not of this protect list
host.tilfa_pc.pc_dist throws tilfa_pc: pc_row or pc_dist is not of this protect list
host.tilfa_pc.cost throws tilfa_pc: the slot arrays of a protected root differ in length
host.rlfa_node.empty ok supported=1 n_protected=0
host.rlfa_node.max_pq_0 throws rlfa_node: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ
host.rlfa_node.max_pq_over throws rlfa_node: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ
host.rlfa_node.no_spaces throws rlfa_node: the RLFA result holds no space tables of this protect list
host.rlfa_node.cost throws rlfa_node: the slot arrays of a protected root differ in length
host.tilfa_node.empty ok supported=1 n_protected=0
host.tilfa_node.max_pairs_0 throws tilfa_node: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS
host.tilfa_node.max_pairs_over throws tilfa_node: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS
host.tilfa_node.no_spaces throws tilfa_node: the RLFA result holds no space tables of this protect list
host.tilfa_node.cost throws tilfa_node: the slot arrays of a protected root differ in length
host.backup_routes_srlg.empty ok supported=1 n_protected=0
host.backup_routes_srlg.routes throws backup_routes_srlg: the routes are not of this run and prefix table
host.backup_routes_srlg.cost throws backup_routes_srlg: the slot arrays of a protected root differ in length
host.backup_routes_srlg.srlgs throws backup_routes_srlg: one Srlg per protected root
host.backup_routes_srlg.mem_ptr throws backup_routes_srlg: mem_ptr needs one entry per slot and one more
host.backup_routes_srlg.member throws backup_routes_srlg: a member column is shorter than mem_ptr says
host.backup_routes_srlg.tilfa throws backup_routes_srlg: the TI-LFA result is not of this protect list
host.backup_routes_ecmp.empty ok supported=1 n_protected=0
host.backup_routes_ecmp.routes throws backup_routes_ecmp: the routes are not of this run and prefix table
host.backup_routes_ecmp.cost throws backup_routes_ecmp: the slot arrays of a protected root differ in length
host.backup_routes_ecmp.tilfa throws backup_routes_ecmp: the TI-LFA result is not of this protect list
host.backup_routes_ecmp_srlg.empty ok supported=1 n_protected=0
host.backup_routes_ecmp_srlg.routes throws backup_routes_ecmp: the routes are not of this run and prefix table
host.backup_routes_ecmp_srlg.cost throws backup_routes_ecmp: the slot arrays of a protected root differ in length
host.backup_routes_ecmp_srlg.srlgs throws backup_routes_ecmp_srlg: one Srlg per protected root
host.backup_routes_ecmp_srlg.mem_ptr throws backup_routes_ecmp_srlg: mem_ptr needs one entry per slot and one more
host.backup_routes_ecmp_srlg.member throws backup_routes_ecmp_srlg: a member column is shorter than mem_ptr says
host.backup_routes_ecmp_srlg.tilfa throws backup_routes_ecmp: the TI-LFA result is not of this protect list
host.backup_routes_node.empty ok supported=1 n_protected=0
host.backup_routes_node.routes throws backup_routes_node: the routes are not of this run and prefix table
host.backup_routes_node.no_list throws backup_routes_node: at least one of the two lists is required
host.backup_routes_node.node throws backup_routes_node: the RLFA-node result is not of this protect list
host.backup_routes_node.pairs throws backup_routes_node: the TI-LFA-node result is not of this protect list
host.backup_routes_node.backup throws backup_routes_node: the backup result is not of this protect list and table
host.backup_routes_node.cost throws backup_routes_node: the slot arrays of a protected root differ in length
"""


def _build_driver():
    import glob
    from holo_amd import build as hb
    deps = [DRIVER + ".cpp"] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps):
        hb.build_lib()
        hb.build_driver("frr_args_driver")


@pytest.mark.gpu
def test_every_argument_check_throws_what_it_threw_gpu():
    _build_driver()
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got, want = r.stdout.splitlines(), EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
