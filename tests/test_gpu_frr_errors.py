"""The argument checks of the 18 fast-reroute device calls, pinned: for every call one single-defect variant of a valid call per
check it makes, with the return code and the FULL text of hspf_last_error written out below.  No row reaches a launch: every output
pointer leads into one arena of 0x5A bytes, which is compared after every row.  After the rows a valid hspf_lfa_device call on the
same context returns what it returned before them.

The graph (8 vertices, vertex 0 a LAN, one mask word) gives the protected root S = 1 the slots
    0: the LAN itself   1: router 4, point-to-point, one SRLG member (link 2 -> 5)   2: router 6, point-to-point
    3: S across the LAN   4, 5: routers 2 and 3 across the LAN
over the rows [1, 4, 6, 2, 3, 0, 5]; two prefixes with one entry each; router 4 is the listed node of the node calls."""
import ctypes

import numpy as np
import pytest

from test_gpu_rlfa import Tables

pytestmark = pytest.mark.gpu

LINKS = [(1, 0, 10), (0, 1, 0), (1, 4, 10), (4, 1, 10), (1, 6, 10), (6, 1, 10), (2, 0, 10), (0, 2, 0), (3, 0, 1), (0, 3, 0),
         (4, 3, 1), (3, 4, 1), (2, 5, 1), (5, 2, 1), (6, 2, 14), (2, 6, 14), (5, 7, 1), (7, 5, 1)]
S, ROOTS = 1, [1, 4, 6, 2, 3, 0, 5]
N, R, W, K = 8, 7, 1, 6
SLOT = 4096                                             # bytes of the arena behind every output pointer

# name -> the arguments behind the context, in order.  `out`, `sel`, `rn_sel`, `tn_sel`, `bk_in`, `table`, `routes`, `tilfa` are
# structs passed by reference, `total` a u64 by reference; the rest are values.
HEAD = "n R W dist flags mask prot"
GHEAD = "g n R W dist flags mask"
BK = "n_prot lfa_flags table routes tilfa"
SIG = {
    "hspf_lfa_device": (HEAD + " n_prot lfa_flags out", "HspfLfaOut"),
    "hspf_lfa_lan_device": (HEAD + " lan n_prot lfa_flags out", "HspfLfaOut"),
    "hspf_lfa_srlg_device": (HEAD + " srlg n_prot lfa_flags out", "HspfLfaOut"),
    "hspf_lfa_ecmp_device": (HEAD + " n_prot lfa_flags cap out total", "HspfLfaEcmpOut"),
    "hspf_rlfa_device": (GHEAD + " rdist prot n_prot lfa_flags alt_in out", "HspfRlfaOut"),
    "hspf_rlfa_lan_device": (GHEAD + " rdist prot lan n_prot lfa_flags alt_in out", "HspfRlfaOut"),
    "hspf_rlfa_srlg_device": (GHEAD + " rdist prot srlg n_prot lfa_flags alt_in out", "HspfRlfaOut"),
    "hspf_tilfa_device": (GHEAD + " rdist prot n_prot lfa_flags alt_in space_flags space_via out", "HspfTilfaOut"),
    "hspf_routes_backup_device": (HEAD + " " + BK + " out", "HspfBackupOut"),
    "hspf_routes_backup_lan_device": (HEAD + " lan " + BK + " out", "HspfBackupOut"),
    "hspf_routes_backup_srlg_device": (HEAD + " srlg " + BK + " out", "HspfBackupOut"),
    "hspf_routes_backup_ecmp_device": (HEAD + " " + BK + " cap out total", "HspfBackupEcmpOut"),
    "hspf_routes_backup_ecmp_srlg_device": (HEAD + " srlg " + BK + " cap out total", "HspfBackupEcmpOut"),
    "hspf_rlfa_node_select_device": (HEAD + " n_prot lfa_flags space_flags max_pq out", "HspfRlfaNodeSel"),
    "hspf_rlfa_node_device": (HEAD + " n_prot ydist y_roots n_yrows sel max_pq alt_in out", "HspfRlfaNodeOut"),
    "hspf_tilfa_node_select_device": (GHEAD + " prot n_prot lfa_flags space_flags max_pairs out", "HspfTilfaNodeSel"),
    "hspf_tilfa_node_device": (HEAD + " n_prot ydist y_roots n_yrows tsel max_pairs alt_in nd_in out", "HspfTilfaNodeOut"),
    "hspf_routes_backup_node_device": (HEAD + " n_prot table routes ydist y_roots n_yrows rn_sel max_pq tn_sel max_pairs bk_in out", "HspfBackupNodeOut"),
}

# The defects.  A plain key replaces the argument (None: a NULL pointer); "struct.field" replaces one field of a struct argument;
# nbr_row / lan_row / tail_row / mem_ptr / n_slots / y_roots are (index, value) edits of the caller's arrays.
NULL_TABLE, NULL_OUT = dict(dist=None), dict(out=None)
DIMS = dict(W=0)
NBR_ROW, LAN_ROW, TAIL_ROW, MEM_PTR = dict(nbr_row=(1, R)), dict(lan_row=(0, R)), dict(tail_row=(0, R)), dict(mem_ptr=(3, 0))
ORDERED = {"table.flags": 0x4}
HUGE = dict(n_slots=0xFFFFFFFF)


INVAL = -1
ROWS = [
    # ---- loop-free alternates
    ("hspf_lfa_device", NULL_TABLE, INVAL, "hspf_lfa_device: NULL table, prot or out pointer"),
    ("hspf_lfa_device", dict(prot=None), INVAL, "hspf_lfa_device: NULL table, prot or out pointer"),
    ("hspf_lfa_device", NULL_OUT, INVAL, "hspf_lfa_device: NULL table, prot or out pointer"),
    ("hspf_lfa_device", {"out.alt_slot": None}, INVAL, "hspf_lfa_device: NULL alt_slot / alt_metric / alt_flags / coverage"),
    ("hspf_lfa_device", {"out.coverage": None}, INVAL, "hspf_lfa_device: NULL alt_slot / alt_metric / alt_flags / coverage"),
    ("hspf_lfa_device", DIMS, INVAL, "hspf_lfa_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_lfa_device", dict(n_prot=0), INVAL, "hspf_lfa_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_lfa_device", NBR_ROW, INVAL, "hspf_lfa_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_lfa_device", dict(n_slots=65), INVAL, "hspf_lfa_device: protected root 0: n_slots > 64 * n_mask_words"),
    ("hspf_lfa_lan_device", NULL_TABLE, INVAL, "hspf_lfa_lan_device: NULL table, prot or out pointer"),
    ("hspf_lfa_lan_device", {"out.alt_flags": None}, INVAL, "hspf_lfa_lan_device: NULL alt_slot / alt_metric / alt_flags / coverage"),
    ("hspf_lfa_lan_device", DIMS, INVAL, "hspf_lfa_lan_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_lfa_lan_device", dict(lan=None), INVAL, "hspf_lfa_lan_device: NULL lan pointer"),
    ("hspf_lfa_lan_device", dict(n_slots=65), INVAL, "hspf_lfa_lan_device: protected root 0: n_slots > 64 * n_mask_words"),
    ("hspf_lfa_lan_device", LAN_ROW, INVAL, "hspf_lfa_lan_device: protected root 0: lan_row of slot 0 >= n_rows"),
    ("hspf_lfa_lan_device", NBR_ROW, INVAL, "hspf_lfa_lan_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_lfa_srlg_device", NULL_TABLE, INVAL, "hspf_lfa_srlg_device: NULL table, prot or out pointer"),
    ("hspf_lfa_srlg_device", {"out.alt_metric": None}, INVAL, "hspf_lfa_srlg_device: NULL alt_slot / alt_metric / alt_flags / coverage"),
    ("hspf_lfa_srlg_device", DIMS, INVAL, "hspf_lfa_srlg_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_lfa_srlg_device", dict(srlg=None), INVAL, "hspf_lfa_srlg_device: NULL srlg pointer"),
    ("hspf_lfa_srlg_device", dict(n_slots=65), INVAL, "hspf_lfa_srlg_device: protected root 0: n_slots > 64 * n_mask_words"),
    ("hspf_lfa_srlg_device", MEM_PTR, INVAL, "hspf_lfa_srlg_device: protected root 0: mem_ptr is not monotone at slot 2"),
    ("hspf_lfa_srlg_device", TAIL_ROW, INVAL, "hspf_lfa_srlg_device: protected root 0: tail_row or head_row of member 0 >= n_rows"),
    ("hspf_lfa_srlg_device", NBR_ROW, INVAL, "hspf_lfa_srlg_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_lfa_ecmp_device", NULL_TABLE, INVAL, "hspf_lfa_ecmp_device: NULL table, prot or out pointer"),
    ("hspf_lfa_ecmp_device", {"out.ea_ptr": None}, INVAL, "hspf_lfa_ecmp_device: NULL ea_ptr or out_total"),
    ("hspf_lfa_ecmp_device", dict(total=None), INVAL, "hspf_lfa_ecmp_device: NULL ea_ptr or out_total"),
    ("hspf_lfa_ecmp_device", {"out.ea_slot": None}, INVAL,
     "hspf_lfa_ecmp_device: NULL ea_primary / ea_slot / ea_metric / ea_flags / ea_coverage with cap_entries > 0"),
    ("hspf_lfa_ecmp_device", DIMS, INVAL, "hspf_lfa_ecmp_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_lfa_ecmp_device", HUGE, INVAL,
     "hspf_lfa_ecmp_device: n_vertices * max(n_slots, 1), summed over the protected roots, reaches 2^32: split the protect list"),
    ("hspf_lfa_ecmp_device", NBR_ROW, INVAL, "hspf_lfa_ecmp_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    # ---- remote loop-free alternates
    ("hspf_rlfa_device", dict(g=None), INVAL, "hspf_rlfa_device: NULL graph, table, prot or out pointer"),
    ("hspf_rlfa_device", dict(rdist=None), INVAL, "hspf_rlfa_device: NULL graph, table, prot or out pointer"),
    ("hspf_rlfa_device", {"out.pq_counts": None}, INVAL,
     "hspf_rlfa_device: NULL pq_node / pq_via / pq_metric / pq_counts / rl_node / rl_via / rl_coverage"),
    ("hspf_rlfa_device", DIMS, INVAL, "hspf_rlfa_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_rlfa_device", dict(g="other"), INVAL, "hspf_rlfa_device: n_vertices is not the graph's"),
    ("hspf_rlfa_device", NBR_ROW, INVAL, "hspf_rlfa_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_rlfa_lan_device", dict(g=None), INVAL, "hspf_rlfa_lan_device: NULL graph, table, prot or out pointer"),
    ("hspf_rlfa_lan_device", {"out.rl_node": None}, INVAL,
     "hspf_rlfa_lan_device: NULL pq_node / pq_via / pq_metric / pq_counts / rl_node / rl_via / rl_coverage"),
    ("hspf_rlfa_lan_device", DIMS, INVAL, "hspf_rlfa_lan_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_rlfa_lan_device", dict(g="other"), INVAL, "hspf_rlfa_lan_device: n_vertices is not the graph's"),
    ("hspf_rlfa_lan_device", dict(lan=None), INVAL, "hspf_rlfa_lan_device: NULL lan pointer"),
    ("hspf_rlfa_lan_device", LAN_ROW, INVAL, "hspf_rlfa_lan_device: protected root 0: lan_row of slot 0 >= n_rows"),
    ("hspf_rlfa_lan_device", NBR_ROW, INVAL, "hspf_rlfa_lan_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_rlfa_srlg_device", dict(g=None), INVAL, "hspf_rlfa_srlg_device: NULL graph, table, prot or out pointer"),
    ("hspf_rlfa_srlg_device", {"out.rl_coverage": None}, INVAL,
     "hspf_rlfa_srlg_device: NULL pq_node / pq_via / pq_metric / pq_counts / rl_node / rl_via / rl_coverage"),
    ("hspf_rlfa_srlg_device", DIMS, INVAL, "hspf_rlfa_srlg_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_rlfa_srlg_device", dict(g="other"), INVAL, "hspf_rlfa_srlg_device: n_vertices is not the graph's"),
    ("hspf_rlfa_srlg_device", dict(srlg=None), INVAL, "hspf_rlfa_srlg_device: NULL srlg pointer"),
    ("hspf_rlfa_srlg_device", MEM_PTR, INVAL, "hspf_rlfa_srlg_device: protected root 0: mem_ptr is not monotone at slot 2"),
    ("hspf_rlfa_srlg_device", TAIL_ROW, INVAL, "hspf_rlfa_srlg_device: protected root 0: tail_row or head_row of member 0 >= n_rows"),
    ("hspf_rlfa_srlg_device", NBR_ROW, INVAL, "hspf_rlfa_srlg_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    # ---- two-segment repair paths
    ("hspf_tilfa_device", dict(g=None), INVAL, "hspf_tilfa_device: NULL graph, table, prot or out pointer"),
    ("hspf_tilfa_device", dict(space_via=None), INVAL,
     "hspf_tilfa_device: NULL space_flags / space_via (the tables of hspf_rlfa_device are required)"),
    ("hspf_tilfa_device", {"out.td_kind": None}, INVAL,
     "hspf_tilfa_device: NULL ti_kind / ti_p / ti_q / ti_via / ti_link / ti_metric / ti_counts / td_kind / td_coverage"),
    ("hspf_tilfa_device", DIMS, INVAL, "hspf_tilfa_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_tilfa_device", dict(g="other"), INVAL, "hspf_tilfa_device: n_vertices is not the graph's"),
    ("hspf_tilfa_device", NBR_ROW, INVAL, "hspf_tilfa_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    # ---- per-prefix backups
    ("hspf_routes_backup_device", NULL_TABLE, INVAL, "hspf_routes_backup_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_device", dict(table=None), INVAL, "hspf_routes_backup_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_device", dict(routes=None), INVAL, "hspf_routes_backup_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_device", {"routes.best_entry": None}, INVAL, "hspf_routes_backup_device: NULL best_metric / best_entry / nexthop_mask"),
    ("hspf_routes_backup_device", {"out.bk_slot": None}, INVAL,
     "hspf_routes_backup_device: NULL bk_kind / bk_primary / bk_slot / bk_metric / bk_flags / bk_coverage"),
    ("hspf_routes_backup_device", {"tilfa.ti_via": None}, INVAL, "hspf_routes_backup_device: NULL ti_kind / ti_via / ti_metric in tilfa_dev"),
    ("hspf_routes_backup_device", DIMS, INVAL, "hspf_routes_backup_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_routes_backup_device", {"table.pfx_ptr": None}, INVAL, "hspf_routes_backup_device: NULL pfx_ptr / pfx_vertex / pfx_metric"),
    ("hspf_routes_backup_device", ORDERED, INVAL, "hspf_routes_backup_device: HSPF_PFX_ORDERED tables are out of scope"),
    ("hspf_routes_backup_device", NBR_ROW, INVAL, "hspf_routes_backup_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_routes_backup_lan_device", NULL_TABLE, INVAL, "hspf_routes_backup_lan_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_lan_device", {"routes.nexthop_mask": None}, INVAL, "hspf_routes_backup_lan_device: NULL best_metric / best_entry / nexthop_mask"),
    ("hspf_routes_backup_lan_device", {"out.bk_coverage": None}, INVAL,
     "hspf_routes_backup_lan_device: NULL bk_kind / bk_primary / bk_slot / bk_metric / bk_flags / bk_coverage"),
    ("hspf_routes_backup_lan_device", {"tilfa.ti_kind": None}, INVAL, "hspf_routes_backup_lan_device: NULL ti_kind / ti_via / ti_metric in tilfa_dev"),
    ("hspf_routes_backup_lan_device", DIMS, INVAL, "hspf_routes_backup_lan_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_routes_backup_lan_device", {"table.pfx_vertex": None}, INVAL, "hspf_routes_backup_lan_device: NULL pfx_ptr / pfx_vertex / pfx_metric"),
    ("hspf_routes_backup_lan_device", ORDERED, INVAL, "hspf_routes_backup_lan_device: HSPF_PFX_ORDERED tables are out of scope"),
    ("hspf_routes_backup_lan_device", dict(lan=None), INVAL, "hspf_routes_backup_lan_device: NULL lan pointer"),
    ("hspf_routes_backup_lan_device", LAN_ROW, INVAL, "hspf_routes_backup_lan_device: protected root 0: lan_row of slot 0 >= n_rows"),
    ("hspf_routes_backup_lan_device", NBR_ROW, INVAL, "hspf_routes_backup_lan_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_routes_backup_srlg_device", NULL_TABLE, INVAL, "hspf_routes_backup_srlg_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_srlg_device", {"routes.best_metric": None}, INVAL, "hspf_routes_backup_srlg_device: NULL best_metric / best_entry / nexthop_mask"),
    ("hspf_routes_backup_srlg_device", {"out.bk_kind": None}, INVAL,
     "hspf_routes_backup_srlg_device: NULL bk_kind / bk_primary / bk_slot / bk_metric / bk_flags / bk_coverage"),
    ("hspf_routes_backup_srlg_device", {"tilfa.ti_p": None}, INVAL,
     "hspf_routes_backup_srlg_device: NULL ti_kind / ti_via / ti_metric / ti_p / ti_link in tilfa_dev"),
    ("hspf_routes_backup_srlg_device", {"tilfa.ti_link": None}, INVAL,
     "hspf_routes_backup_srlg_device: NULL ti_kind / ti_via / ti_metric / ti_p / ti_link in tilfa_dev"),
    ("hspf_routes_backup_srlg_device", DIMS, INVAL, "hspf_routes_backup_srlg_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_routes_backup_srlg_device", {"table.pfx_metric": None}, INVAL, "hspf_routes_backup_srlg_device: NULL pfx_ptr / pfx_vertex / pfx_metric"),
    ("hspf_routes_backup_srlg_device", ORDERED, INVAL, "hspf_routes_backup_srlg_device: HSPF_PFX_ORDERED tables are out of scope"),
    ("hspf_routes_backup_srlg_device", dict(srlg=None), INVAL, "hspf_routes_backup_srlg_device: NULL srlg pointer"),
    ("hspf_routes_backup_srlg_device", MEM_PTR, INVAL, "hspf_routes_backup_srlg_device: protected root 0: mem_ptr is not monotone at slot 2"),
    ("hspf_routes_backup_srlg_device", TAIL_ROW, INVAL,
     "hspf_routes_backup_srlg_device: protected root 0: tail_row or head_row of member 0 >= n_rows"),
    ("hspf_routes_backup_srlg_device", NBR_ROW, INVAL, "hspf_routes_backup_srlg_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_routes_backup_ecmp_device", NULL_TABLE, INVAL, "hspf_routes_backup_ecmp_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_ecmp_device", {"routes.best_entry": None}, INVAL, "hspf_routes_backup_ecmp_device: NULL best_metric / best_entry / nexthop_mask"),
    ("hspf_routes_backup_ecmp_device", {"out.eb_ptr": None}, INVAL, "hspf_routes_backup_ecmp_device: NULL eb_ptr or out_total"),
    ("hspf_routes_backup_ecmp_device", dict(total=None), INVAL, "hspf_routes_backup_ecmp_device: NULL eb_ptr or out_total"),
    ("hspf_routes_backup_ecmp_device", {"out.eb_kind": None}, INVAL,
     "hspf_routes_backup_ecmp_device: NULL eb_primary / eb_kind / eb_slot / eb_metric / eb_flags / eb_coverage with cap_entries > 0"),
    ("hspf_routes_backup_ecmp_device", {"tilfa.ti_metric": None}, INVAL, "hspf_routes_backup_ecmp_device: NULL ti_kind / ti_via / ti_metric in tilfa_dev"),
    ("hspf_routes_backup_ecmp_device", DIMS, INVAL, "hspf_routes_backup_ecmp_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_routes_backup_ecmp_device", {"table.pfx_ptr": None}, INVAL, "hspf_routes_backup_ecmp_device: NULL pfx_ptr / pfx_vertex / pfx_metric"),
    ("hspf_routes_backup_ecmp_device", ORDERED, INVAL, "hspf_routes_backup_ecmp_device: HSPF_PFX_ORDERED tables are out of scope"),
    ("hspf_routes_backup_ecmp_device", HUGE, INVAL,
     "hspf_routes_backup_ecmp_device: n_prefixes * max(n_slots, 1), summed over the protected roots, reaches 2^32: split the protect list"),
    ("hspf_routes_backup_ecmp_device", NBR_ROW, INVAL, "hspf_routes_backup_ecmp_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_routes_backup_ecmp_srlg_device", NULL_TABLE, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_ecmp_srlg_device", {"routes.best_metric": None}, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: NULL best_metric / best_entry / nexthop_mask"),
    ("hspf_routes_backup_ecmp_srlg_device", {"out.eb_ptr": None}, INVAL, "hspf_routes_backup_ecmp_srlg_device: NULL eb_ptr or out_total"),
    ("hspf_routes_backup_ecmp_srlg_device", {"out.eb_coverage": None}, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: NULL eb_primary / eb_kind / eb_slot / eb_metric / eb_flags / eb_coverage with cap_entries > 0"),
    ("hspf_routes_backup_ecmp_srlg_device", {"tilfa.ti_p": None}, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: NULL ti_kind / ti_via / ti_metric / ti_p / ti_link in tilfa_dev"),
    ("hspf_routes_backup_ecmp_srlg_device", {"tilfa.ti_link": None}, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: NULL ti_kind / ti_via / ti_metric / ti_p / ti_link in tilfa_dev"),
    ("hspf_routes_backup_ecmp_srlg_device", DIMS, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_routes_backup_ecmp_srlg_device", {"table.pfx_ptr": None}, INVAL, "hspf_routes_backup_ecmp_srlg_device: NULL pfx_ptr / pfx_vertex / pfx_metric"),
    ("hspf_routes_backup_ecmp_srlg_device", ORDERED, INVAL, "hspf_routes_backup_ecmp_srlg_device: HSPF_PFX_ORDERED tables are out of scope"),
    ("hspf_routes_backup_ecmp_srlg_device", HUGE, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: n_prefixes * max(n_slots, 1), summed over the protected roots, reaches 2^32: split the protect list"),
    ("hspf_routes_backup_ecmp_srlg_device", dict(srlg=None), INVAL, "hspf_routes_backup_ecmp_srlg_device: NULL srlg pointer"),
    ("hspf_routes_backup_ecmp_srlg_device", MEM_PTR, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: protected root 0: mem_ptr is not monotone at slot 2"),
    ("hspf_routes_backup_ecmp_srlg_device", TAIL_ROW, INVAL,
     "hspf_routes_backup_ecmp_srlg_device: protected root 0: tail_row or head_row of member 0 >= n_rows"),
    ("hspf_routes_backup_ecmp_srlg_device", NBR_ROW, INVAL, "hspf_routes_backup_ecmp_srlg_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    # ---- node protection
    ("hspf_rlfa_node_select_device", NULL_TABLE, INVAL, "hspf_rlfa_node_select_device: NULL table, prot or out pointer"),
    ("hspf_rlfa_node_select_device", dict(space_flags=None), INVAL,
     "hspf_rlfa_node_select_device: NULL space_flags (the table of hspf_rlfa_device is required)"),
    ("hspf_rlfa_node_select_device", {"out.nq_via": None}, INVAL, "hspf_rlfa_node_select_device: NULL nq_node / nq_via / nq_metric / nq_count"),
    ("hspf_rlfa_node_select_device", dict(max_pq=0), INVAL, "hspf_rlfa_node_select_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ"),
    ("hspf_rlfa_node_select_device", dict(max_pq=33), INVAL, "hspf_rlfa_node_select_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ"),
    ("hspf_rlfa_node_select_device", DIMS, INVAL, "hspf_rlfa_node_select_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_rlfa_node_select_device", NBR_ROW, INVAL, "hspf_rlfa_node_select_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_rlfa_node_device", NULL_TABLE, INVAL, "hspf_rlfa_node_device: NULL table, prot or out pointer"),
    ("hspf_rlfa_node_device", dict(ydist=None), INVAL, "hspf_rlfa_node_device: NULL ydist, y_roots or sel pointer"),
    ("hspf_rlfa_node_device", dict(y_roots=None), INVAL, "hspf_rlfa_node_device: NULL ydist, y_roots or sel pointer"),
    ("hspf_rlfa_node_device", dict(sel=None), INVAL, "hspf_rlfa_node_device: NULL ydist, y_roots or sel pointer"),
    ("hspf_rlfa_node_device", {"sel.nq_count": None}, INVAL, "hspf_rlfa_node_device: NULL nq_node / nq_via / nq_metric / nq_count in sel_dev"),
    ("hspf_rlfa_node_device", {"out.nd_node": None}, INVAL, "hspf_rlfa_node_device: NULL nd_kind / nd_node / nd_via / nd_metric / nd_coverage"),
    ("hspf_rlfa_node_device", dict(max_pq=0), INVAL, "hspf_rlfa_node_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ"),
    ("hspf_rlfa_node_device", dict(max_pq=33), INVAL, "hspf_rlfa_node_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ"),
    ("hspf_rlfa_node_device", dict(n_yrows=0), INVAL, "hspf_rlfa_node_device: n_yrows is 0"),
    ("hspf_rlfa_node_device", DIMS, INVAL, "hspf_rlfa_node_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_rlfa_node_device", dict(y_roots=(0, N)), INVAL, "hspf_rlfa_node_device: y_roots entry 0 >= n_vertices"),
    ("hspf_rlfa_node_device", NBR_ROW, INVAL, "hspf_rlfa_node_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_tilfa_node_select_device", dict(g=None), INVAL, "hspf_tilfa_node_select_device: NULL graph, table, prot or out pointer"),
    ("hspf_tilfa_node_select_device", dict(space_flags=None), INVAL,
     "hspf_tilfa_node_select_device: NULL space_flags (the table of hspf_rlfa_device is required)"),
    ("hspf_tilfa_node_select_device", {"out.tq_link": None}, INVAL,
     "hspf_tilfa_node_select_device: NULL tq_q / tq_p / tq_link / tq_via / tq_metric / tq_count"),
    ("hspf_tilfa_node_select_device", dict(max_pairs=0), INVAL, "hspf_tilfa_node_select_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS"),
    ("hspf_tilfa_node_select_device", dict(max_pairs=33), INVAL, "hspf_tilfa_node_select_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS"),
    ("hspf_tilfa_node_select_device", DIMS, INVAL, "hspf_tilfa_node_select_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_tilfa_node_select_device", dict(g="other"), INVAL, "hspf_tilfa_node_select_device: n_vertices is not the graph's"),
    ("hspf_tilfa_node_select_device", NBR_ROW, INVAL, "hspf_tilfa_node_select_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_tilfa_node_device", NULL_TABLE, INVAL, "hspf_tilfa_node_device: NULL table, prot or out pointer"),
    ("hspf_tilfa_node_device", dict(ydist=None), INVAL, "hspf_tilfa_node_device: NULL ydist, y_roots or sel pointer"),
    ("hspf_tilfa_node_device", dict(tsel=None), INVAL, "hspf_tilfa_node_device: NULL ydist, y_roots or sel pointer"),
    ("hspf_tilfa_node_device", {"tsel.tq_p": None}, INVAL, "hspf_tilfa_node_device: NULL tq_q / tq_p / tq_link / tq_via / tq_metric / tq_count in sel_dev"),
    ("hspf_tilfa_node_device", {"out.tn_q": None}, INVAL,
     "hspf_tilfa_node_device: NULL tn_kind / tn_p / tn_q / tn_link / tn_via / tn_metric / tn_coverage"),
    ("hspf_tilfa_node_device", dict(max_pairs=0), INVAL, "hspf_tilfa_node_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS"),
    ("hspf_tilfa_node_device", dict(max_pairs=33), INVAL, "hspf_tilfa_node_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS"),
    ("hspf_tilfa_node_device", dict(n_yrows=0), INVAL, "hspf_tilfa_node_device: n_yrows is 0"),
    ("hspf_tilfa_node_device", DIMS, INVAL, "hspf_tilfa_node_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_tilfa_node_device", dict(y_roots=(0, N)), INVAL, "hspf_tilfa_node_device: y_roots entry 0 >= n_vertices"),
    ("hspf_tilfa_node_device", NBR_ROW, INVAL, "hspf_tilfa_node_device: protected root 0: nbr_row of slot 1 >= n_rows"),
    ("hspf_routes_backup_node_device", NULL_TABLE, INVAL, "hspf_routes_backup_node_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_node_device", dict(table=None), INVAL, "hspf_routes_backup_node_device: NULL table, prot, prefix table, routes or out pointer"),
    ("hspf_routes_backup_node_device", {"routes.nexthop_mask": None}, INVAL, "hspf_routes_backup_node_device: NULL best_metric / best_entry / nexthop_mask"),
    ("hspf_routes_backup_node_device", {"out.bn_via": None}, INVAL,
     "hspf_routes_backup_node_device: NULL bn_kind / bn_primary / bn_p / bn_q / bn_link / bn_via / bn_metric / bn_coverage"),
    ("hspf_routes_backup_node_device", dict(ydist=None), INVAL, "hspf_routes_backup_node_device: NULL ydist or y_roots pointer"),
    ("hspf_routes_backup_node_device", dict(y_roots=None), INVAL, "hspf_routes_backup_node_device: NULL ydist or y_roots pointer"),
    ("hspf_routes_backup_node_device", dict(rn_sel=None, tn_sel=None), INVAL,
     "hspf_routes_backup_node_device: NULL rn_sel_dev and tn_sel_dev (at least one list is required)"),
    ("hspf_routes_backup_node_device", {"rn_sel.nq_node": None}, INVAL,
     "hspf_routes_backup_node_device: NULL nq_node / nq_via / nq_metric / nq_count in rn_sel_dev"),
    ("hspf_routes_backup_node_device", dict(max_pq=0), INVAL, "hspf_routes_backup_node_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ"),
    ("hspf_routes_backup_node_device", dict(max_pq=33), INVAL, "hspf_routes_backup_node_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ"),
    ("hspf_routes_backup_node_device", {"tn_sel.tq_count": None}, INVAL,
     "hspf_routes_backup_node_device: NULL tq_q / tq_p / tq_link / tq_via / tq_metric / tq_count in tn_sel_dev"),
    ("hspf_routes_backup_node_device", dict(max_pairs=0), INVAL, "hspf_routes_backup_node_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS"),
    ("hspf_routes_backup_node_device", dict(max_pairs=33), INVAL, "hspf_routes_backup_node_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS"),
    ("hspf_routes_backup_node_device", {"bk_in.bk_flags": None}, INVAL, "hspf_routes_backup_node_device: NULL bk_kind / bk_flags in bk_in_dev"),
    ("hspf_routes_backup_node_device", dict(n_yrows=0), INVAL, "hspf_routes_backup_node_device: n_yrows is 0"),
    ("hspf_routes_backup_node_device", DIMS, INVAL, "hspf_routes_backup_node_device: n_vertices, n_rows, n_mask_words or n_prot out of range"),
    ("hspf_routes_backup_node_device", {"table.pfx_ptr": None}, INVAL, "hspf_routes_backup_node_device: NULL pfx_ptr / pfx_vertex / pfx_metric"),
    ("hspf_routes_backup_node_device", ORDERED, INVAL, "hspf_routes_backup_node_device: HSPF_PFX_ORDERED tables are out of scope"),
    ("hspf_routes_backup_node_device", dict(y_roots=(0, N)), INVAL, "hspf_routes_backup_node_device: y_roots entry 0 >= n_vertices"),
    ("hspf_routes_backup_node_device", NBR_ROW, INVAL, "hspf_routes_backup_node_device: protected root 0: nbr_row of slot 1 >= n_rows"),
]


def graph():
    rows = [[(b, c) for a, b, c in LINKS if a == v] for v in range(N)]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    vf = np.zeros(N, np.uint8)
    vf[0] = 1                                            # HSPF_VF_NETWORK
    return rp, np.array([t for r in rows for t, _ in r], np.uint32), np.array([c for r in rows for _, c in r], np.uint32), vf


class Caller:
    """Builds the arguments of a valid call of every entry point, applies one defect, calls."""

    def __init__(self, ctx, tab, other, arena):
        from holo_amd import _lib as L
        from holo_amd import engine as E
        self.ctx, self.tab, self.other, self.L = ctx, tab, other, L
        self.base, self.next = arena.data_ptr(), 0
        g = graph()
        row_of = {v: i for i, v in enumerate(ROOTS)}
        c = E.lfa_candidates(*g, S)
        lan = E.lfa_lan_candidates(*g, S)
        grp_ptr = np.zeros(len(g[1]) + 1, np.uint32)     # links 4 (1 -> 4) and 7 (2 -> 5) share group 5
        grp_ptr[5:8] = 1
        grp_ptr[8:] = 2
        mem = E.srlg_members(*g, S, grp_ptr, np.array([5, 5], np.uint32))
        none = int(E.NO_ROOT)
        assert c.nbr.tolist() == [none, 4, 6, none, 2, 3] and lan.tolist() == [0, none, none, 0, 0, 0]
        assert mem.mem_ptr.tolist() == [0, 0, 1, 1, 1, 1, 1] and (int(mem.tail[0]), int(mem.head[0])) == (2, 5)
        u32 = lambda x: np.array(x, np.uint32)      # noqa: E731
        self.cols = dict(nbr=c.nbr.copy(), nbr_row=u32([row_of.get(int(x), 0) for x in c.nbr]), cost=c.cost.copy(), root_link=c.root_link.copy(),
                         cflags=c.cflags.copy(), lan=lan.copy(), lan_row=u32([row_of.get(int(x), 0) for x in lan]), mem_ptr=mem.mem_ptr.copy(),
                         tail=mem.tail.copy(), pos=mem.pos.copy(), head=mem.head.copy(), mcost=mem.cost.copy(), tail_row=u32([row_of[2]]),
                         head_row=u32([row_of[5]]), y_roots=u32([4]), pfx_ptr=u32([0, 1, 2]), pfx_vertex=u32([5, 7]), pfx_metric=u32([0, 3]))
        assert len(c.nbr) == K and self.cols["nbr_row"][1] == 1 and self.cols["lan_row"][0] == 5

    def slot(self):
        p = self.base + self.next * SLOT
        self.next += 1
        return p

    def struct(self, name):
        cls = getattr(self.L, name)
        return cls(*(self.slot() for _ in cls._fields_))

    def args(self, fn, defect):
        L, t = self.L, self.tab
        self.next = 0
        cols = {k: v.copy() for k, v in self.cols.items()}
        n_slots = K
        for key in ("nbr_row", "lan_row", "tail_row", "mem_ptr", "y_roots"):
            if isinstance(defect.get(key), tuple):
                i, v = defect[key]
                cols[key][i] = v
        if "n_slots" in defect:
            n_slots = defect["n_slots"]
        p32 = lambda k: cols[k].ctypes.data_as(L.u32p)      # noqa: E731
        names, out_cls = SIG[fn]
        out = self.struct(out_cls)                      # (first: the valid call's arena is a few slots long)
        self.total = ctypes.c_uint64(7)
        v = dict(
            g=t.G.handle, n=t.n, R=t.R, W=W, dist=t.dist.data_ptr(), flags=t.flags.data_ptr(), mask=t.mask.data_ptr(), rdist=t.rdist.data_ptr(),
            prot=(L.HspfLfaProtect * 1)(L.HspfLfaProtect(S, 0, n_slots, p32("nbr"), p32("nbr_row"), p32("cost"), p32("root_link"),
                                                        cols["cflags"].ctypes.data_as(L.u8p))),
            lan=(L.HspfLfaLan * 1)(L.HspfLfaLan(p32("lan"), p32("lan_row"))),
            srlg=(L.HspfSrlg * 1)(L.HspfSrlg(p32("mem_ptr"), p32("tail"), p32("pos"), p32("head"), p32("mcost"), p32("tail_row"), p32("head_row"))),
            n_prot=1, lfa_flags=0, alt_in=None, nd_in=None, cap=16, total=self.total, max_pq=2, max_pairs=2,
            space_flags=self.slot(), space_via=self.slot(), ydist=t.dist.data_ptr(), y_roots=p32("y_roots"), n_yrows=1,
            table=L.HspfPrefixTable(2, 2, p32("pfx_ptr"), p32("pfx_vertex"), p32("pfx_metric"), 0, None, None, None, None),
            routes=self.struct("HspfRoutes"), tilfa=self.struct("HspfTilfaOut"), sel=self.struct("HspfRlfaNodeSel"), rn_sel=self.struct("HspfRlfaNodeSel"),
            tsel=self.struct("HspfTilfaNodeSel"), tn_sel=self.struct("HspfTilfaNodeSel"), bk_in=self.struct("HspfBackupOut"), out=out)
        for key, val in defect.items():
            if "." in key:
                s, f = key.split(".")
                setattr(v[s], f, val)
            elif key == "g" and val == "other":
                v["g"] = self.other.handle
            elif not isinstance(val, tuple) and key != "n_slots":
                v[key] = val
        self.keep = (cols, v)
        return [v[k] if v[k] is None or not isinstance(v[k], (ctypes.Structure, ctypes.c_uint64)) else ctypes.byref(v[k]) for k in names.split()], v

    def call(self, fn, defect):
        a, v = self.args(fn, defect)
        rc = getattr(self.ctx.lib, fn)(self.ctx.handle, *a)
        return rc, self.ctx.lib.hspf_last_error(self.ctx.handle).decode()


def test_the_table_names_every_entry_point_and_every_listed_check():
    assert {r[0] for r in ROWS} == set(SIG) and len(SIG) == 18
    for fn in SIG:
        texts = " | ".join(r[3] for r in ROWS if r[0] == fn)
        assert all(r[3].startswith(fn + ": ") for r in ROWS if r[0] == fn)
        assert "NULL" in texts and "out of range" in texts and "nbr_row" in texts, fn
        names = SIG[fn][0].split()
        for arg, text in (("g", "not the graph's"), ("table", "HSPF_PFX_ORDERED"), ("max_pq", "max_pq outside"), ("max_pairs", "max_pairs outside"),
                          ("n_yrows", "n_yrows is 0"), ("y_roots", "y_roots entry 0"), ("lan", "lan_row"), ("srlg", "mem_ptr is not monotone"),
                          ("srlg", "tail_row")):
            assert (arg not in names) or text in texts, (fn, arg)
        if "srlg" in names and "tilfa" in names:
            assert "ti_p / ti_link" in texts, fn


def test_every_row_fails_with_its_code_and_text_and_writes_nothing(spf_ctx):
    import torch
    dev = torch.device("cuda:0")
    g = graph()
    tab = Tables(spf_ctx, g, 0xFFFFFFFF, np.array(ROOTS, np.uint32), 0, W)
    other = spf_ctx.upload(np.array([0, 1, 2], np.uint32), np.array([1, 0], np.uint32), np.ones(2, np.uint32), np.zeros(2, np.uint8), 0xFFFFFFFF)
    try:
        arena = torch.full((64 * SLOT,), 0x5A, dtype=torch.uint8, device=dev)
        real = torch.full((8 * SLOT,), 0x33, dtype=torch.uint8, device=dev)      # the outputs of the valid call before and after
        cl, ok = Caller(spf_ctx, tab, other, arena), Caller(spf_ctx, tab, other, real)

        def valid_lfa():
            real.fill_(0x33)
            torch.cuda.synchronize()                    # (the fill is on torch's stream, the call on the context's)
            a, _ = ok.args("hspf_lfa_device", {})
            assert spf_ctx.lib.hspf_lfa_device(spf_ctx.handle, *a) == 0, spf_ctx.last_error()
            return real.cpu().numpy().copy()

        before = valid_lfa()
        assert (before != 0x33).any()
        wrong = []
        for fn, defect, code, text in ROWS:
            rc, msg = cl.call(fn, defect)
            assert cl.next <= 64
            if (rc, msg) != (code, text):
                wrong.append((fn, defect, rc, msg))
            assert bool((arena == 0x5A).all()), (fn, defect)
            assert cl.total.value == 7, (fn, defect)
        assert not wrong, wrong
        assert np.array_equal(valid_lfa(), before)
    finally:
        other.free()
        tab.free()
