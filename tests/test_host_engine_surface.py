"""The Python surface of the fast-reroute layer of holo_amd.engine.SpfContext, pinned: the signature of every public method from
lfa_device() to tilfa_node(), and of the private helpers that tests and tools/*_measure.py call or inspect.  The tables were
generated with str(inspect.signature(...)) before the layer was folded onto one call path (_frr_call); a change here is a change
of the API, not of its implementation."""
import inspect

PUBLIC = {
    'lfa_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, *, alt_slot_ptr: 'int', alt_metric_ptr: 'int', alt_flags_ptr: 'int', coverage_ptr: 'int', cand_mask_ptr: 'int' = 0, node_mask_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'lfa_lan_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, lans, *, alt_slot_ptr: 'int', alt_metric_ptr: 'int', alt_flags_ptr: 'int', coverage_ptr: 'int', cand_mask_ptr: 'int' = 0, node_mask_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'lfa':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, want_masks: 'bool' = True, lan_protect: 'bool' = False)",
    'lfa_ecmp_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, *, ea_ptr_ptr: 'int', cap_entries: 'int' = 0, ea_primary_ptr: 'int' = 0, ea_slot_ptr: 'int' = 0, ea_metric_ptr: 'int' = 0, ea_flags_ptr: 'int' = 0, ea_coverage_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'int'",
    'lfa_ecmp':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0)",
    'rlfa_device':
        "(self, graph: 'SpfGraph', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', rdist_ptr: 'int', protect, *, pq_node_ptr: 'int', pq_via_ptr: 'int', pq_metric_ptr: 'int', pq_counts_ptr: 'int', rl_node_ptr: 'int', rl_via_ptr: 'int', rl_coverage_ptr: 'int', space_flags_ptr: 'int' = 0, space_via_ptr: 'int' = 0, alt_flags_in_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'rlfa_lan_device':
        "(self, graph: 'SpfGraph', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', rdist_ptr: 'int', protect, lans, *, pq_node_ptr: 'int', pq_via_ptr: 'int', pq_metric_ptr: 'int', pq_counts_ptr: 'int', rl_node_ptr: 'int', rl_via_ptr: 'int', rl_coverage_ptr: 'int', space_flags_ptr: 'int' = 0, space_via_ptr: 'int' = 0, alt_flags_in_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'lfa_srlg_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, srlgs, *, alt_slot_ptr: 'int', alt_metric_ptr: 'int', alt_flags_ptr: 'int', coverage_ptr: 'int', cand_mask_ptr: 'int' = 0, node_mask_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'rlfa_srlg_device':
        "(self, graph: 'SpfGraph', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', rdist_ptr: 'int', protect, srlgs, *, pq_node_ptr: 'int', pq_via_ptr: 'int', pq_metric_ptr: 'int', pq_counts_ptr: 'int', rl_node_ptr: 'int', rl_via_ptr: 'int', rl_coverage_ptr: 'int', space_flags_ptr: 'int' = 0, space_via_ptr: 'int' = 0, alt_flags_in_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'lfa_srlg':
        "(self, graph: 'SpfGraph', root: 'int', grp_ptr, grp, run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, want_masks: 'bool' = True)",
    'rlfa_srlg':
        "(self, graph: 'SpfGraph', root: 'int', grp_ptr, grp, run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, want_spaces: 'bool' = False, symmetric: 'bool' = False)",
    'tilfa_srlg':
        "(self, graph: 'SpfGraph', root: 'int', grp_ptr, grp, run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, symmetric: 'bool' = False)",
    'tilfa_device':
        "(self, graph: 'SpfGraph', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', rdist_ptr: 'int', protect, *, space_flags_ptr: 'int', space_via_ptr: 'int', ti_kind_ptr: 'int', ti_p_ptr: 'int', ti_q_ptr: 'int', ti_via_ptr: 'int', ti_link_ptr: 'int', ti_metric_ptr: 'int', ti_counts_ptr: 'int', td_kind_ptr: 'int', td_coverage_ptr: 'int', alt_flags_in_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'tilfa_pc_device':
        "(self, graph: 'SpfGraph', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', rdist_ptr: 'int', protect, *, space_flags_ptr: 'int', space_via_ptr: 'int', pc_dist_ptr: 'int', n_pc_rows: 'int', pc_row, max_walk: 'int' = 256, run_flags: 'int' = 0, tp_kind_ptr: 'int', tp_p_ptr: 'int', tp_via_ptr: 'int', tp_q_ptr: 'int', tp_n_adj_ptr: 'int', tp_hop_pos_ptr: 'int', tp_hop_head_ptr: 'int', tp_metric_ptr: 'int', tp_flags_ptr: 'int', tp_coverage_ptr: 'int', alt_flags_in_ptr: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'routes_backup_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, pfx_ptr, pfx_vertex, pfx_metric, *, routes: 'tuple', bk_kind_ptr: 'int', bk_primary_ptr: 'int', bk_slot_ptr: 'int', bk_metric_ptr: 'int', bk_flags_ptr: 'int', bk_coverage_ptr: 'int', bk_cand_mask_ptr: 'int' = 0, bk_node_mask_ptr: 'int' = 0, tilfa: 'Optional[tuple]' = None, flags: 'int' = 0, lfa_flags: 'int' = 0, pfx_origin=None) -> 'None'",
    'routes_backup_ecmp_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, pfx_ptr, pfx_vertex, pfx_metric, *, routes: 'tuple', eb_ptr_ptr: 'int', cap_entries: 'int' = 0, eb_primary_ptr: 'int' = 0, eb_kind_ptr: 'int' = 0, eb_slot_ptr: 'int' = 0, eb_metric_ptr: 'int' = 0, eb_flags_ptr: 'int' = 0, eb_coverage_ptr: 'int' = 0, tilfa: 'Optional[tuple]' = None, flags: 'int' = 0, lfa_flags: 'int' = 0, pfx_origin=None) -> 'int'",
    'routes_backup_ecmp_srlg_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, srlgs, pfx_ptr, pfx_vertex, pfx_metric, *, routes: 'tuple', eb_ptr_ptr: 'int', cap_entries: 'int' = 0, eb_primary_ptr: 'int' = 0, eb_kind_ptr: 'int' = 0, eb_slot_ptr: 'int' = 0, eb_metric_ptr: 'int' = 0, eb_flags_ptr: 'int' = 0, eb_coverage_ptr: 'int' = 0, tilfa: 'Optional[tuple]' = None, flags: 'int' = 0, lfa_flags: 'int' = 0, pfx_origin=None) -> 'int'",
    'routes_backup_lan_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, lans, pfx_ptr, pfx_vertex, pfx_metric, **kw) -> 'None'",
    'routes_backup_srlg_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, srlgs, pfx_ptr, pfx_vertex, pfx_metric, *, routes: 'tuple', bk_kind_ptr: 'int', bk_primary_ptr: 'int', bk_slot_ptr: 'int', bk_metric_ptr: 'int', bk_flags_ptr: 'int', bk_coverage_ptr: 'int', bk_cand_mask_ptr: 'int' = 0, bk_node_mask_ptr: 'int' = 0, tilfa: 'Optional[tuple]' = None, flags: 'int' = 0, lfa_flags: 'int' = 0) -> 'None'",
    'routes_backup_node_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, pfx_ptr, pfx_vertex, pfx_metric, *, routes: 'tuple', ydist_ptr: 'int', y_roots, bn_kind_ptr: 'int', bn_primary_ptr: 'int', bn_p_ptr: 'int', bn_q_ptr: 'int', bn_link_ptr: 'int', bn_via_ptr: 'int', bn_metric_ptr: 'int', bn_coverage_ptr: 'int', bn_set_pq_ptr: 'int' = 0, bn_set_pair_ptr: 'int' = 0, rn_sel: 'Optional[tuple]' = None, max_pq: 'int' = 0, tn_sel: 'Optional[tuple]' = None, max_pairs: 'int' = 0, bk_in: 'Optional[tuple]' = None, flags: 'int' = 0) -> 'None'",
    'backup_routes':
        "(self, graph: 'SpfGraph', root: 'int', prefix_table, run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, symmetric: 'bool' = False, remote: 'bool' = True, lan_protect: 'bool' = False, lan_repairs: 'bool' = False, node_protect: 'bool' = False, max_pq: 'int' = 16, max_pairs: 'int' = 16, srlg: 'Optional[tuple]' = None, srlg_repairs: 'bool' = False, ecmp: 'bool' = False) -> 'BackupRoutes'",
    'rlfa':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, want_spaces: 'bool' = False, symmetric: 'bool' = False, lan_protect: 'bool' = False)",
    'tilfa':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, symmetric: 'bool' = False, lan_protect: 'bool' = False)",
    'tilfa_pc':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, symmetric: 'bool' = False, max_walk: 'int' = 256)",
    'rlfa_node_select_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, *, space_flags_ptr: 'int', max_pq: 'int', nq_node_ptr: 'int', nq_via_ptr: 'int', nq_metric_ptr: 'int', nq_count_ptr: 'int', lfa_flags: 'int' = 0) -> 'None'",
    'rlfa_node_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, *, ydist_ptr: 'int', y_roots, sel: 'tuple', max_pq: 'int', nd_kind_ptr: 'int', nd_node_ptr: 'int', nd_via_ptr: 'int', nd_metric_ptr: 'int', nd_coverage_ptr: 'int', nd_set_ptr: 'int' = 0, alt_flags_in_ptr: 'int' = 0) -> 'None'",
    'rlfa_node':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, max_pq: 'int' = 16, symmetric: 'bool' = False)",
    'tilfa_node_select_device':
        "(self, graph: 'SpfGraph', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, *, space_flags_ptr: 'int', max_pairs: 'int', tq_q_ptr: 'int', tq_p_ptr: 'int', tq_link_ptr: 'int', tq_via_ptr: 'int', tq_metric_ptr: 'int', tq_count_ptr: 'int', lfa_flags: 'int' = 0) -> 'None'",
    'tilfa_node_device':
        "(self, n_vertices: 'int', n_rows: 'int', mask_words: 'int', dist_ptr: 'int', flags_ptr: 'int', mask_ptr: 'int', protect, *, ydist_ptr: 'int', y_roots, sel: 'tuple', max_pairs: 'int', tn_kind_ptr: 'int', tn_p_ptr: 'int', tn_q_ptr: 'int', tn_link_ptr: 'int', tn_via_ptr: 'int', tn_metric_ptr: 'int', tn_coverage_ptr: 'int', tn_set_ptr: 'int' = 0, alt_flags_in_ptr: 'int' = 0, nd_kind_in_ptr: 'int' = 0) -> 'None'",
    'tilfa_node':
        "(self, graph: 'SpfGraph', root: 'int', run_flags: 'int' = 0, *, lfa_flags: 'int' = 0, max_pq: 'int' = 16, max_pairs: 'int' = 16, symmetric: 'bool' = False)",
}

PRIVATE = {
    '_protect_array':
        "(protect, who: 'str')",
    '_lan_array':
        "(lans, protect, who: 'str')",
    '_srlg_array':
        "(srlgs, protect, who: 'str')",
    '_frr_plan':
        "(self, graph: 'SpfGraph', root: 'int', lan_protect: 'bool' = False)",
    '_srlg_plan':
        "(self, graph: 'SpfGraph', root: 'int', grp_ptr, grp)",
    '_dev_buffers':
        "(self, sizes: 'dict')",
    '_fetch':
        "(self, host_arrays: 'dict', dev: 'dict') -> 'None'",
    '_check_rc':
        "(self, name: 'str', rc: 'int') -> 'None'",
    '_backup_ecmp_tail':
        "(self, n: 'int', R: 'int', W: 'int', dev: 'dict', protect, backup, tilfa: 'bool', lfa_flags: 'int', srlgs=None) -> 'BackupEcmpResult'",
    '_backup_srlg':
        "(self, graph: 'SpfGraph', root: 'int', tab, grp_ptr, grp, run_flags: 'int', lfa_flags: 'int', symmetric: 'bool', remote: 'bool', srlg_repairs: 'bool', ecmp: 'bool' = False) -> 'BackupRoutes'",
}


def _public_frr_methods():
    """The public callables of SpfContext from lfa_device to tilfa_node, in definition order."""
    from holo_amd.engine import SpfContext
    names = [k for k, v in vars(SpfContext).items() if callable(getattr(SpfContext, k))]
    return [k for k in names[names.index("lfa_device"):names.index("tilfa_node") + 1] if not k.startswith("_")]


def test_the_public_frr_methods_are_the_pinned_ones_in_their_order():
    assert _public_frr_methods() == list(PUBLIC)


def test_every_pinned_signature_holds():
    from holo_amd.engine import SpfContext
    wrong = {k: str(inspect.signature(getattr(SpfContext, k))) for k, s in {**PUBLIC, **PRIVATE}.items()
             if str(inspect.signature(getattr(SpfContext, k))) != s}
    assert not wrong, wrong


def test_the_three_array_helpers_are_static_and_the_buffers_a_context_manager():
    from holo_amd.engine import SpfContext
    for k in ("_protect_array", "_lan_array", "_srlg_array"):
        assert isinstance(vars(SpfContext)[k], staticmethod), k
    assert hasattr(SpfContext._dev_buffers, "__wrapped__")          # contextlib.contextmanager
