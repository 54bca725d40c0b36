// frr_args_driver.cpp — the argument checks of the fast-reroute calls of both compiled layers: what they throw, word for word.
//   frr_args_driver          one line per call: `<case> ok supported=<0|1> n_protected=<count>` or `<case> throws <what()>`
//                            (an hspf::Error: `<case> throws code=<code> <what()>`)
// One 4-router ring with unit metrics, root 0, one mask word; one valid run, one reverse run (the ring's costs are symmetric: the
// forward graph serves), a routes set and a two-prefix table.  Every call carries exactly ONE defect, and every check it trips
// stands in front of the first device call of its method: no kernel sees a bad argument.  The results handed from one call to the
// next (RlfaOut, TilfaOut, ...) are sized by hand, as a caller's of the right shape would be; their contents are never read.
// tests/test_cpp_frr_args.py holds the expected lines.  Built by holo_amd/build.py (build_driver).  TEST INFRASTRUCTURE.
#include <cstdio>
#include <string>
#include <vector>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"

namespace {

namespace H = hspf::host;

template <typename F>
void probe(const char *name, F &&call) {          // a host-interface call: every result struct has supported / n_protected
  try {
    const auto o = call();
    printf("%s ok supported=%d n_protected=%u\n", name, o.supported ? 1 : 0, o.n_protected);
  } catch (const hspf::Error &e) {
    printf("%s throws code=%d %s\n", name, e.code, e.what());
  } catch (const std::exception &e) {
    printf("%s throws %s\n", name, e.what());
  }
}

template <typename F>
void refuse(const char *name, F &&call) {         // a call of the RAII layer that must not get as far as the device
  try {
    call();
    printf("%s ok\n", name);
  } catch (const hspf::Error &e) {
    printf("%s throws code=%d %s\n", name, e.code, e.what());
  } catch (const std::exception &e) {
    printf("%s throws %s\n", name, e.what());
  }
}

}  // namespace

int main() {
  const std::vector<uint32_t> row_ptr{0, 2, 4, 6, 8}, col{1, 3, 0, 2, 1, 3, 0, 2}, metric(8, 1u);
  const std::vector<uint8_t> vflags(4, 0);
  const uint32_t maxp = 0xFFFFFFFFu, root = 0, n = 4, S = 64;
  const std::vector<uint32_t> roots{0, 1, 3};
  const std::vector<uint32_t> pfx_ptr{0, 1, 2}, pfx_vertex{2, 3}, pfx_metric{0, 0};
  try {
    const hspf::LfaCandidates c = hspf::Engine::lfa_candidates(row_ptr, col, metric, vflags, root);      // nbr 1 and 3: rows 1 and 2
    std::vector<uint32_t> nbr_row;
    for (uint32_t v : c.nbr) nbr_row.push_back(v == 1 ? 1u : 2u);
    {
      // ---- the RAII layer -----------------------------------------------------------------------------------------------
      hspf::Engine eng(0);
      hspf::Graph g = eng.upload(row_ptr, col, metric, vflags, maxp);
      const std::vector<uint8_t> vf5(5, 0);                 // one vertex more than the graph has
      refuse("raii.lfa.csr", [&] { eng.lfa(g, row_ptr, col, metric, vf5, root); });
      refuse("raii.lfa_ecmp.csr", [&] { eng.lfa_ecmp(g, row_ptr, col, metric, vf5, root); });
      refuse("raii.rlfa.csr", [&] { eng.rlfa(g, row_ptr, col, metric, vf5, maxp, root); });
      refuse("raii.tilfa.csr", [&] { eng.tilfa(g, row_ptr, col, metric, vf5, maxp, root); });
      refuse("raii.tilfa_node.csr", [&] { eng.tilfa_node(g, row_ptr, col, metric, vf5, maxp, root); });
      refuse("raii.backup_routes.csr", [&] { eng.backup_routes(g, row_ptr, col, metric, vf5, maxp, root, pfx_ptr, pfx_vertex, pfx_metric); });
      refuse("raii.tilfa_node.max_pq_0", [&] { eng.tilfa_node(g, row_ptr, col, metric, vflags, maxp, root, 0, 0, false, 0, 16); });
      refuse("raii.tilfa_node.max_pq_over", [&] { eng.tilfa_node(g, row_ptr, col, metric, vflags, maxp, root, 0, 0, false, HSPF_RLFA_NODE_MAX_PQ + 1, 16); });
      refuse("raii.tilfa_node.max_pairs_0", [&] { eng.tilfa_node(g, row_ptr, col, metric, vflags, maxp, root, 0, 0, false, 16, 0); });
      refuse("raii.tilfa_node.max_pairs_over", [&] { eng.tilfa_node(g, row_ptr, col, metric, vflags, maxp, root, 0, 0, false, 16, HSPF_TILFA_NODE_MAX_PAIRS + 1); });
      refuse("raii.backup_routes.no_pfx_ptr", [&] { eng.backup_routes(g, row_ptr, col, metric, vflags, maxp, root, {}, pfx_vertex, pfx_metric); });
      refuse("raii.backup_routes.pfx_metric_short", [&] { eng.backup_routes(g, row_ptr, col, metric, vflags, maxp, root, pfx_ptr, pfx_vertex, {0}); });
      refuse("raii.srlg_members.grp_ptr_short", [&] { hspf::Engine::srlg_members(row_ptr, col, metric, vflags, root, std::vector<uint32_t>(8, 0u), {}); });
      // the *_device wrappers: one protected root, a list one short; the device pointers are never looked at
      const std::vector<hspf_lfa_protect> p{{root, 0u, (uint32_t)c.nbr.size(), c.nbr.data(), nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()}};
      const hspf_prefix_table tab{2, 2, pfx_ptr.data(), pfx_vertex.data(), pfx_metric.data(), 0, nullptr, nullptr, nullptr, nullptr};
      const hspf_routes ro{};
      refuse("raii.lfa_lan_device.lans", [&] { eng.lfa_lan_device(n, 3, 1, nullptr, nullptr, nullptr, p, {}, 0, hspf_lfa_out{}); });
      refuse("raii.rlfa_lan_device.lans", [&] { eng.rlfa_lan_device(g, 3, 1, nullptr, nullptr, nullptr, nullptr, p, {}, 0, nullptr, hspf_rlfa_out{}); });
      refuse("raii.routes_backup_lan_device.lans", [&] { eng.routes_backup_lan_device(n, 3, 1, nullptr, nullptr, nullptr, p, {}, 0, tab, ro, nullptr, hspf_backup_out{}); });
      refuse("raii.lfa_srlg_device.srlgs", [&] { eng.lfa_srlg_device(n, 3, 1, nullptr, nullptr, nullptr, p, {}, 0, hspf_lfa_out{}); });
      refuse("raii.rlfa_srlg_device.srlgs", [&] { eng.rlfa_srlg_device(g, 3, 1, nullptr, nullptr, nullptr, nullptr, p, {}, 0, nullptr, hspf_rlfa_out{}); });
      refuse("raii.routes_backup_srlg_device.srlgs", [&] { eng.routes_backup_srlg_device(n, 3, 1, nullptr, nullptr, nullptr, p, {}, 0, tab, ro, nullptr, hspf_backup_out{}); });
      refuse("raii.routes_backup_ecmp_srlg_device.srlgs",
             [&] { eng.routes_backup_ecmp_srlg_device(n, 3, 1, nullptr, nullptr, nullptr, p, {}, 0, tab, ro, nullptr, 0, hspf_backup_ecmp_out{}); });
      refuse("raii.tilfa_pc_device.pc_row", [&] {
        eng.tilfa_pc_device(g, 3, 1, nullptr, nullptr, nullptr, nullptr, p, 0, nullptr, nullptr, nullptr, nullptr, 1, std::vector<uint32_t>(S - 1, HSPF_NO_ROOT), 0, 256,
                            hspf_tilfa_pc_out{});
      });
    }
    // ---- the host interface on the product engine ---------------------------------------------------------------------------
    H::HipEngine heng(0);
    auto hg = heng.upload(row_ptr, col, metric, vflags, maxp);
    auto run = heng.run_device(*hg, roots, 0);
    auto rrun = heng.run_device(*hg, roots, 0);
    auto rrun2 = heng.run_device(*hg, {0, 1}, 0);           // another root count
    auto routes = heng.routes_device(*run, pfx_ptr, pfx_vertex, pfx_metric, 0);
    auto routes1 = heng.routes_device(*run, {0, 1}, {2}, {0}, 0);      // another prefix count
    H::LfaProtect hp;
    hp.root_vertex = root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
    H::LfaProtect hp_short = hp;
    hp_short.cost.pop_back();
    const std::vector<H::LfaProtect> none, good{hp}, bad{hp_short};
    const size_t K = hp.nbr.size(), sp = (size_t)S * n, P = 2;
    // LAN and SRLG lists: no LAN behind a slot, no member of a group
    const H::LfaLan lan{std::vector<uint32_t>(K, HSPF_NO_ROOT), std::vector<uint32_t>(K, 0u)};
    H::LfaLan lan_short = lan;
    lan_short.lan_row.pop_back();
    H::Srlg sg;
    sg.mem_ptr.assign(K + 1, 0u);
    H::Srlg sg_ptr_short = sg, sg_col_short = sg;
    sg_ptr_short.mem_ptr.pop_back();
    sg_col_short.mem_ptr.back() = 1;                        // one member, and no column holds it
    const std::vector<H::LfaLan> no_lans, lans{lan}, lans_short{lan_short};
    const std::vector<H::Srlg> no_srlgs, srlgs{sg}, srlgs_ptr{sg_ptr_short}, srlgs_col{sg_col_short};
    // results of the calls in front, of this protect list's shape
    H::RlfaOut rl, rl_bare;
    rl.supported = rl_bare.supported = true; rl.n_protected = rl_bare.n_protected = 1; rl.n_vertices = rl_bare.n_vertices = n;
    rl.space_flags.assign(sp, 0); rl.space_via.assign(sp, 0u);
    auto tilfa_of = [&](size_t stride) {
      H::TilfaOut t;
      t.supported = true; t.n_protected = 1; t.n_vertices = n; t.slot_stride = (uint32_t)stride;
      t.ti_kind.assign(stride, 0); t.ti_p.assign(stride, 0u); t.ti_q.assign(stride, 0u); t.ti_via.assign(stride, 0u); t.ti_link.assign(stride, 0u);
      t.ti_metric.assign(stride, 0u);
      return t;
    };
    const H::TilfaOut ti = tilfa_of(S), ti_wide = tilfa_of(2 * S);
    H::RlfaNodeOut rn;
    rn.supported = true; rn.n_protected = 1; rn.n_vertices = n; rn.max_pq = 2;
    rn.nq_node.assign(2 * S, HSPF_NO_ROOT); rn.nq_via.assign(2 * S, 0u); rn.nq_metric.assign(2 * S, 0u); rn.nq_count.assign(S, 0u);
    H::RlfaNodeOut rn_short = rn;
    rn_short.nq_count.pop_back();
    H::TilfaNodeOut tn;
    tn.supported = true; tn.n_protected = 1; tn.n_vertices = n; tn.max_pairs = 2;
    tn.tq_q.assign(2 * S, HSPF_NO_ROOT); tn.tq_p.assign(2 * S, 0u); tn.tq_link.assign(2 * S, 0u); tn.tq_via.assign(2 * S, 0u); tn.tq_metric.assign(2 * S, 0u);
    tn.tq_count.assign(S, 0u);
    H::TilfaNodeOut tn_short = tn;
    tn_short.tq_count.pop_back();
    H::BackupOut bo;
    bo.supported = true; bo.n_protected = 1; bo.n_prefixes = (uint32_t)P; bo.bk_kind.assign(P, 0); bo.bk_flags.assign(P, 0);
    H::BackupOut bo_short = bo;
    bo_short.bk_flags.pop_back();
    const std::vector<uint32_t> pc_dist(n, 0u), pc_row(S, HSPF_NO_ROOT), pc_row_short(S - 1, HSPF_NO_ROOT), pc_dist_short(n - 1, 0u);

    probe("host.lfa.empty", [&] { return heng.lfa(*run, none, 0, false); });
    probe("host.lfa.cost", [&] { return heng.lfa(*run, bad, 0, false); });
    probe("host.lfa_ecmp.empty", [&] { return heng.lfa_ecmp(*run, none, 0); });
    probe("host.lfa_ecmp.cost", [&] { return heng.lfa_ecmp(*run, bad, 0); });
    probe("host.lfa_lan.empty", [&] { return heng.lfa_lan(*run, none, no_lans, 0, false); });
    probe("host.lfa_lan.lans", [&] { return heng.lfa_lan(*run, good, no_lans, 0, false); });
    probe("host.lfa_lan.cost", [&] { return heng.lfa_lan(*run, bad, lans, 0, false); });
    probe("host.lfa_lan.lan_row", [&] { return heng.lfa_lan(*run, good, lans_short, 0, false); });
    probe("host.lfa_srlg.empty", [&] { return heng.lfa_srlg(*run, none, no_srlgs, 0, false); });
    probe("host.lfa_srlg.cost", [&] { return heng.lfa_srlg(*run, bad, srlgs, 0, false); });
    probe("host.lfa_srlg.srlgs", [&] { return heng.lfa_srlg(*run, good, no_srlgs, 0, false); });
    probe("host.lfa_srlg.mem_ptr", [&] { return heng.lfa_srlg(*run, good, srlgs_ptr, 0, false); });
    probe("host.lfa_srlg.member", [&] { return heng.lfa_srlg(*run, good, srlgs_col, 0, false); });

    probe("host.rlfa.empty", [&] { return heng.rlfa(*hg, *run, *rrun, none, 0, nullptr, false); });
    probe("host.rlfa.reverse_run", [&] { return heng.rlfa(*hg, *run, *rrun2, good, 0, nullptr, false); });
    probe("host.rlfa.cost", [&] { return heng.rlfa(*hg, *run, *rrun, bad, 0, nullptr, false); });
    probe("host.rlfa_lan.empty", [&] { return heng.rlfa_lan(*hg, *run, *rrun, none, no_lans, 0, nullptr, false); });
    probe("host.rlfa_lan.lans", [&] { return heng.rlfa_lan(*hg, *run, *rrun, good, no_lans, 0, nullptr, false); });
    probe("host.rlfa_lan.reverse_run", [&] { return heng.rlfa_lan(*hg, *run, *rrun2, good, lans, 0, nullptr, false); });
    probe("host.rlfa_lan.cost", [&] { return heng.rlfa_lan(*hg, *run, *rrun, bad, lans, 0, nullptr, false); });
    probe("host.rlfa_lan.lan_row", [&] { return heng.rlfa_lan(*hg, *run, *rrun, good, lans_short, 0, nullptr, false); });
    probe("host.rlfa_srlg.empty", [&] { return heng.rlfa_srlg(*hg, *run, *rrun, none, no_srlgs, 0, nullptr, false); });
    probe("host.rlfa_srlg.reverse_run", [&] { return heng.rlfa_srlg(*hg, *run, *rrun2, good, srlgs, 0, nullptr, false); });
    probe("host.rlfa_srlg.cost", [&] { return heng.rlfa_srlg(*hg, *run, *rrun, bad, srlgs, 0, nullptr, false); });
    probe("host.rlfa_srlg.srlgs", [&] { return heng.rlfa_srlg(*hg, *run, *rrun, good, no_srlgs, 0, nullptr, false); });
    probe("host.rlfa_srlg.mem_ptr", [&] { return heng.rlfa_srlg(*hg, *run, *rrun, good, srlgs_ptr, 0, nullptr, false); });
    probe("host.rlfa_srlg.member", [&] { return heng.rlfa_srlg(*hg, *run, *rrun, good, srlgs_col, 0, nullptr, false); });

    probe("host.tilfa.empty", [&] { return heng.tilfa(*hg, *run, *rrun, none, 0, nullptr, rl); });
    probe("host.tilfa.reverse_run", [&] { return heng.tilfa(*hg, *run, *rrun2, good, 0, nullptr, rl); });
    probe("host.tilfa.no_spaces", [&] { return heng.tilfa(*hg, *run, *rrun, good, 0, nullptr, rl_bare); });
    probe("host.tilfa.cost", [&] { return heng.tilfa(*hg, *run, *rrun, bad, 0, nullptr, rl); });
    probe("host.tilfa_pc.empty", [&] { return heng.tilfa_pc(*hg, *run, *rrun, none, 0, nullptr, rl, pc_dist, 1, pc_row, 0, 256); });
    probe("host.tilfa_pc.reverse_run", [&] { return heng.tilfa_pc(*hg, *run, *rrun2, good, 0, nullptr, rl, pc_dist, 1, pc_row, 0, 256); });
    probe("host.tilfa_pc.no_spaces", [&] { return heng.tilfa_pc(*hg, *run, *rrun, good, 0, nullptr, rl_bare, pc_dist, 1, pc_row, 0, 256); });
    probe("host.tilfa_pc.pc_row", [&] { return heng.tilfa_pc(*hg, *run, *rrun, good, 0, nullptr, rl, pc_dist, 1, pc_row_short, 0, 256); });
    probe("host.tilfa_pc.pc_dist", [&] { return heng.tilfa_pc(*hg, *run, *rrun, good, 0, nullptr, rl, pc_dist_short, 1, pc_row, 0, 256); });
    probe("host.tilfa_pc.cost", [&] { return heng.tilfa_pc(*hg, *run, *rrun, bad, 0, nullptr, rl, pc_dist, 1, pc_row, 0, 256); });

    probe("host.rlfa_node.empty", [&] { return heng.rlfa_node(*hg, *run, none, 0, 0, nullptr, rl, 2); });
    probe("host.rlfa_node.max_pq_0", [&] { return heng.rlfa_node(*hg, *run, good, 0, 0, nullptr, rl, 0); });
    probe("host.rlfa_node.max_pq_over", [&] { return heng.rlfa_node(*hg, *run, good, 0, 0, nullptr, rl, HSPF_RLFA_NODE_MAX_PQ + 1); });
    probe("host.rlfa_node.no_spaces", [&] { return heng.rlfa_node(*hg, *run, good, 0, 0, nullptr, rl_bare, 2); });
    probe("host.rlfa_node.cost", [&] { return heng.rlfa_node(*hg, *run, bad, 0, 0, nullptr, rl, 2); });
    probe("host.tilfa_node.empty", [&] { return heng.tilfa_node(*hg, *run, none, 0, 0, nullptr, rl, nullptr, 2); });
    probe("host.tilfa_node.max_pairs_0", [&] { return heng.tilfa_node(*hg, *run, good, 0, 0, nullptr, rl, nullptr, 0); });
    probe("host.tilfa_node.max_pairs_over", [&] { return heng.tilfa_node(*hg, *run, good, 0, 0, nullptr, rl, nullptr, HSPF_TILFA_NODE_MAX_PAIRS + 1); });
    probe("host.tilfa_node.no_spaces", [&] { return heng.tilfa_node(*hg, *run, good, 0, 0, nullptr, rl_bare, nullptr, 2); });
    probe("host.tilfa_node.cost", [&] { return heng.tilfa_node(*hg, *run, bad, 0, 0, nullptr, rl, nullptr, 2); });

    probe("host.backup_routes_srlg.empty", [&] { return heng.backup_routes_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, none, no_srlgs, 0, nullptr); });
    probe("host.backup_routes_srlg.routes", [&] { return heng.backup_routes_srlg(*run, *routes1, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs, 0, nullptr); });
    probe("host.backup_routes_srlg.cost", [&] { return heng.backup_routes_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, bad, srlgs, 0, nullptr); });
    probe("host.backup_routes_srlg.srlgs", [&] { return heng.backup_routes_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, no_srlgs, 0, nullptr); });
    probe("host.backup_routes_srlg.mem_ptr", [&] { return heng.backup_routes_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs_ptr, 0, nullptr); });
    probe("host.backup_routes_srlg.member", [&] { return heng.backup_routes_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs_col, 0, nullptr); });
    probe("host.backup_routes_srlg.tilfa", [&] { return heng.backup_routes_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs, 0, &ti_wide); });
    probe("host.backup_routes_ecmp.empty", [&] { return heng.backup_routes_ecmp(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, none, 0, nullptr); });
    probe("host.backup_routes_ecmp.routes", [&] { return heng.backup_routes_ecmp(*run, *routes1, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, nullptr); });
    probe("host.backup_routes_ecmp.cost", [&] { return heng.backup_routes_ecmp(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, bad, 0, nullptr); });
    probe("host.backup_routes_ecmp.tilfa", [&] { return heng.backup_routes_ecmp(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, &ti_wide); });
    probe("host.backup_routes_ecmp_srlg.empty", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, none, no_srlgs, 0, nullptr); });
    probe("host.backup_routes_ecmp_srlg.routes", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes1, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs, 0, nullptr); });
    probe("host.backup_routes_ecmp_srlg.cost", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, bad, srlgs, 0, nullptr); });
    probe("host.backup_routes_ecmp_srlg.srlgs", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, no_srlgs, 0, nullptr); });
    probe("host.backup_routes_ecmp_srlg.mem_ptr", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs_ptr, 0, nullptr); });
    probe("host.backup_routes_ecmp_srlg.member", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs_col, 0, nullptr); });
    probe("host.backup_routes_ecmp_srlg.tilfa", [&] { return heng.backup_routes_ecmp_srlg(*run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, srlgs, 0, &ti_wide); });
    (void)ti;

    probe("host.backup_routes_node.empty", [&] { return heng.backup_routes_node(*hg, *run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, none, 0, &rn, &tn, &bo); });
    probe("host.backup_routes_node.routes", [&] { return heng.backup_routes_node(*hg, *run, *routes1, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, &rn, &tn, &bo); });
    probe("host.backup_routes_node.no_list", [&] { return heng.backup_routes_node(*hg, *run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, nullptr, nullptr, &bo); });
    probe("host.backup_routes_node.node", [&] { return heng.backup_routes_node(*hg, *run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, &rn_short, &tn, &bo); });
    probe("host.backup_routes_node.pairs", [&] { return heng.backup_routes_node(*hg, *run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, &rn, &tn_short, &bo); });
    probe("host.backup_routes_node.backup", [&] { return heng.backup_routes_node(*hg, *run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, good, 0, &rn, &tn, &bo_short); });
    probe("host.backup_routes_node.cost", [&] { return heng.backup_routes_node(*hg, *run, *routes, pfx_ptr, pfx_vertex, pfx_metric, 0, bad, 0, &rn, &tn, &bo); });
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "frr_args_driver: %s\n", e.what());
    return 2;
  }
}
