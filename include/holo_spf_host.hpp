// holo_spf_host.hpp — what the C++ host-side twins (holo_spf_isis.hpp, holo_spf_ospf.hpp) share: the three engine calls
// they need, the product implementation of those calls on the C ABI, and IP prefix / address keys in the order of the
// reference's BTreeMap<IpNetwork, _> / BTreeMap<IpAddr, _>.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "holo_spf_hip.h"

namespace hspf {
namespace host {

// ---- engine seen from the host side ------------------------------------------------------------------------------
struct Tables {                       // row-major [root][vertex] results of one run
  uint32_t n_roots = 0, n_vertices = 0, mask_words = 1;
  std::vector<uint32_t> dist, pop_rank;
  std::vector<uint16_t> hops, flags;
  std::vector<uint64_t> mask;
};
struct SlotTable { std::vector<uint32_t> vertex, base; uint32_t total = 0; };
struct Failure { uint32_t kind = HSPF_FAIL_NONE, arg = 0; };   // one row of run_failures(): hspf_failure

class Graph {                         // one uploaded graph (device resident for the product engine)
 public:
  virtual ~Graph() = default;
};
// Results of one run left where the engine produced them (HBM for the product engine): input of routes().
// The same tables as plain pointers into memory the run object keeps (valid while it lives): what a caller needs that
// reads a handful of entries (the first-hop slot replay) and must not pay for four std::vector copies per step.
struct TablesView { const uint32_t *dist = nullptr; const uint16_t *hops = nullptr, *flags = nullptr; const uint64_t *mask = nullptr;
                    uint32_t n_roots = 0, n_vertices = 0, mask_words = 1; };
class DeviceRun {
 public:
  virtual ~DeviceRun() = default;
  virtual Tables host_tables() = 0;   // the copy the host side still needs for next-hop resolution
  // distance / hops / flags (and the masks when asked for) on the host, zero-copy for the caller; the default keeps a Tables
  virtual TablesView host_view(bool with_mask) {
    (void)with_mask;
    if (!view_cache_) view_cache_ = std::make_unique<Tables>(host_tables());
    return TablesView{view_cache_->dist.data(), view_cache_->hops.data(), view_cache_->flags.data(), view_cache_->mask.data(), n_roots, n_vertices, mask_words};
  }
  uint32_t n_roots = 0, n_vertices = 0, mask_words = 1;
 private:
  std::unique_ptr<Tables> view_cache_;
};
struct RoutesOut {                    // per (root, prefix), row-major: see hspf_routes in holo_spf_hip.h
  std::vector<uint32_t> best_metric, best_entry;
  std::vector<uint64_t> nexthop_mask;
};
// Route tables of one routes_device() call (or an uploaded set) left where the engine keeps them (HBM for the product
// engine): operands of the RIB comparison (hspf_routes_diff_device).
class DeviceRoutes {
 public:
  virtual ~DeviceRoutes() = default;
  virtual RoutesOut host() = 0;
  uint32_t n_roots = 0, n_prefixes = 0, mask_words = 1;
};
// The record stream of hspf_routes_pack: [count][HSPF_ROUTE_REC_WORDS + 2 mask_words] u32 (root, prefix, action, metric, entry, 0, mask words lo/hi)
struct RouteRecords {
  uint32_t mask_words = 1;
  std::vector<uint32_t> words;
  std::vector<uint32_t> old_words;     // the same records packed from the OLD set (metric, entry, masks of the route held before)
  const uint32_t *old_rec(size_t k) const { return old_words.data() + k * stride(); }
  size_t stride() const { return HSPF_ROUTE_REC_WORDS + 2u * mask_words; }
  size_t count() const { return words.size() / stride(); }
  const uint32_t *rec(size_t k) const { return words.data() + k * stride(); }
};
// The event stream of hspf_routes_events: every pair that is not SAME as ONE record with the new and the old half of the
// route (HSPF_EVENT_REC_WORDS + 4 * mask_words words).  supported == false: the engine has no such call (the caller keeps
// routes_changed).  `data` points into a buffer the engine keeps: valid until its next routes_events.
struct RouteEvents {
  bool supported = false;
  uint32_t mask_words = 1;
  size_t n = 0;
  const uint32_t *data = nullptr;
  std::vector<uint32_t> own;           // (engines without a kept buffer put the stream here and point `data` at it)
  size_t stride() const { return HSPF_EVENT_REC_WORDS + 4u * mask_words; }
  size_t count() const { return n; }
  const uint32_t *rec(size_t k) const { return (own.empty() ? data : own.data()) + k * stride(); }
  uint32_t root(size_t k) const { return rec(k)[0]; }
  uint32_t prefix(size_t k) const { return rec(k)[1]; }
  uint32_t action(size_t k) const { return rec(k)[2]; }
  uint32_t new_metric(size_t k) const { return rec(k)[3]; }
  uint32_t new_entry(size_t k) const { return rec(k)[4]; }
  uint32_t old_metric(size_t k) const { return rec(k)[5]; }
  uint32_t old_entry(size_t k) const { return rec(k)[6]; }
  const uint32_t *new_mask(size_t k) const { return rec(k) + HSPF_EVENT_REC_WORDS; }                       // 2 * mask_words words, low half first
  const uint32_t *old_mask(size_t k) const { return rec(k) + HSPF_EVENT_REC_WORDS + 2u * mask_words; }
};
// Loop-free alternates (hspf_lfa_device) of protected roots whose SPTs — and their neighbour routers' — are rows of one
// DeviceRun: what the caller passes per protected root, and what comes back on the host.  supported == false: the engine has
// no such call (the caller evaluates RFC 5286's inequalities on host_tables() itself).
struct LfaProtect {
  uint32_t root_vertex = 0, root_row = 0;
  std::vector<uint32_t> nbr, nbr_row, cost, root_link;      // one entry per first-hop slot (hspf_lfa_candidates)
  std::vector<uint8_t> cflags;
};
// Broadcast-link protection (hspf_lfa_lan_device / hspf_routes_backup_lan_device): parallel to LfaProtect, one entry per slot —
// the LAN behind the slot's first link (hspf_lfa_lan_candidates, HSPF_NO_ROOT: point-to-point) and the row of the SPT rooted at it.
// The outputs are LfaOut / BackupOut with HSPF_LFA_LAN_COVERAGE_WORDS / HSPF_BK_LAN_COVERAGE_WORDS coverage words per root.
struct LfaLan {
  std::vector<uint32_t> lan, lan_row;
};
// Shared-risk link groups (hspf_lfa_srlg_device / hspf_rlfa_srlg_device): parallel to LfaProtect — the members of every slot
// (hspf_srlg_members: slot k's are entries mem_ptr[k] .. mem_ptr[k + 1] of the columns) and the rows of the SPTs rooted at their
// endpoints.  The outputs are LfaOut / RlfaOut with HSPF_LFA_SRLG_COVERAGE_WORDS / HSPF_RLFA_SRLG_COUNT_WORDS /
// HSPF_RLFA_SRLG_COVERAGE_WORDS words.
struct Srlg {
  std::vector<uint32_t> mem_ptr, tail, pos, head, cost, tail_row, head_row;
};
struct LfaOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0, mask_words = 1;
  std::vector<uint32_t> alt_slot, alt_metric;               // [n_protected][n_vertices]
  std::vector<uint8_t> alt_flags;
  std::vector<uint64_t> cand_mask, node_mask;               // [n_protected][n_vertices][mask_words] (empty without with_masks)
  std::vector<uint32_t> coverage;                           // [n_protected][HSPF_LFA_COVERAGE_WORDS] (lfa_lan: HSPF_LFA_LAN_COVERAGE_WORDS)
};
// Per-primary alternates of the ECMP destinations (hspf_lfa_ecmp_device) of the same protected roots: a stream in CSR form over
// (protected root, destination), the entries of one destination in ascending primary slot order.  supported == false: no such call.
struct LfaEcmpOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0;
  std::vector<uint32_t> ea_ptr;                             // [n_protected * n_vertices + 1]
  std::vector<uint32_t> ea_primary, ea_slot, ea_metric;     // [ea_ptr.back()]
  std::vector<uint8_t> ea_flags;
  std::vector<uint32_t> ea_coverage;                        // [n_protected][HSPF_LFA_ECMP_COVERAGE_WORDS]
};
// Remote loop-free alternates (hspf_rlfa_device) of the same protected roots: PQ nodes per (protected root, slot) and the remote
// alternate per destination, from the forward DeviceRun and the DeviceRun of the SAME roots on the transposed graph
// (hspf_csr_transpose).  supported == false: the engine has no such call.
struct RlfaOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0, slot_stride = 64;
  std::vector<uint32_t> pq_node, pq_via, pq_metric;         // [n_protected][slot_stride]
  std::vector<uint32_t> pq_counts;                          // [n_protected][slot_stride][HSPF_RLFA_COUNT_WORDS] (rlfa_lan: HSPF_RLFA_LAN_COUNT_WORDS)
  std::vector<uint8_t> space_flags;                         // [n_protected][slot_stride][n_vertices] (empty without with_spaces)
  std::vector<uint32_t> space_via;
  std::vector<uint32_t> rl_node, rl_via;                    // [n_protected][n_vertices]
  std::vector<uint32_t> rl_coverage;                        // [n_protected][HSPF_RLFA_COVERAGE_WORDS] (rlfa_lan: HSPF_RLFA_LAN_COVERAGE_WORDS)
};
// Two-segment repair paths (hspf_tilfa_device) of the same protected roots: per (protected root, slot) the cheapest repair that is
// one PQ node or a node of the extended P-space plus one forced adjacency into the Q-space, and the class of every destination,
// from the same two DeviceRuns and the space tables of rlfa(..., with_spaces = true).  supported == false: no such call.
struct TilfaOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0, slot_stride = 64;
  std::vector<uint8_t> ti_kind;                             // [n_protected][slot_stride] HSPF_TILFA_*
  std::vector<uint32_t> ti_p, ti_q, ti_via, ti_link, ti_metric;
  std::vector<uint32_t> ti_counts;                          // [n_protected][slot_stride][HSPF_TILFA_COUNT_WORDS]
  std::vector<uint8_t> td_kind;                             // [n_protected][n_vertices] HSPF_TILFA_D_*
  std::vector<uint32_t> td_coverage;                        // [n_protected][HSPF_TILFA_COVERAGE_WORDS]
};
// TI-LFA repairs along the post-convergence path (hspf_tilfa_pc_device) of the same protected roots: per destination with one
// primary slot the Node-SID, the adjacencies and the class, from the forward DeviceRun, the space tables of rlfa(..., with_spaces =
// true) and the dist rows of run_failures() for the slots' links.  supported == false: no such call.
struct TilfaPcOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0;
  std::vector<uint8_t> tp_kind, tp_n_adj, tp_flags;         // [n_protected][n_vertices] HSPF_TIPC_D_* | 0 .. HSPF_TIPC_MAX_ADJ | HSPF_TIPC_*
  std::vector<uint32_t> tp_p, tp_via, tp_q, tp_metric;      // [n_protected][n_vertices]
  std::vector<uint32_t> tp_hop_pos, tp_hop_head;            // [n_protected][n_vertices][HSPF_TIPC_MAX_ADJ], in the order p -> q
  std::vector<uint32_t> tp_coverage;                        // [n_protected][HSPF_TIPC_COVERAGE_WORDS]
  struct Hop { uint32_t tail, pos, head; };
  // the repair of destination d of protected root i: false unless HSPF_TIPC_D_REPAIR; via == HSPF_LFA_NO_SLOT: p is the root
  bool segments(uint32_t i, uint32_t d, uint32_t &via, uint32_t &p, std::vector<Hop> &hops, uint32_t &q) const {
    const size_t c = (size_t)i * n_vertices + d;
    hops.clear();
    if (i >= n_protected || d >= n_vertices || tp_kind[c] != HSPF_TIPC_D_REPAIR) return false;
    via = tp_via[c]; p = tp_p[c]; q = tp_q[c];
    uint32_t tail = p;
    for (uint32_t h = 0; h < tp_n_adj[c] && h < HSPF_TIPC_MAX_ADJ; ++h) {
      hops.push_back(Hop{tail, tp_hop_pos[c * HSPF_TIPC_MAX_ADJ + h], tp_hop_head[c * HSPF_TIPC_MAX_ADJ + h]});
      tail = hops.back().head;
    }
    return true;
  }
};
// Node-protecting remote loop-free alternates (RFC 8102: hspf_rlfa_node_select_device, one run over the listed nodes,
// hspf_rlfa_node_device) of the same protected roots: per (protected root, slot) the cheapest max_pq PQ nodes whose release path
// avoids the neighbour behind the slot, and per destination the cheapest of them whose own path avoids it too, from the forward
// DeviceRun and the space_flags of rlfa(..., with_spaces = true).  supported == false: no such call.
struct RlfaNodeOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0, slot_stride = 64, max_pq = 0;
  std::vector<uint32_t> nq_node, nq_via, nq_metric;         // [n_protected][slot_stride][max_pq]
  std::vector<uint32_t> nq_count;                           // [n_protected][slot_stride]
  std::vector<uint32_t> y_roots;                            // the roots of the PQ-node rows: the ascending union of the lists
  std::vector<uint8_t> nd_kind;                             // [n_protected][n_vertices] HSPF_NP_D_*
  std::vector<uint32_t> nd_node, nd_via, nd_metric, nd_set; // [n_protected][n_vertices]
  std::vector<uint32_t> nd_coverage;                        // [n_protected][HSPF_NP_COVERAGE_WORDS]
};
// Two-segment node-protecting repairs (hspf_tilfa_node_select_device, one run over the listed q's, hspf_tilfa_node_device) of the
// same protected roots: per (protected root, slot) the cheapest max_pairs routers q of the Q-space a forced adjacency p -> q enters
// from a node p whose release path avoids the neighbour behind the slot, and per destination the cheapest of them whose q reaches it
// without that neighbour, from the forward DeviceRun and the space_flags of rlfa(..., with_spaces = true).  supported == false: no
// such call.
struct TilfaNodeOut {
  bool supported = false;
  uint32_t n_protected = 0, n_vertices = 0, slot_stride = 64, max_pairs = 0;
  std::vector<uint32_t> tq_q, tq_p, tq_link, tq_via, tq_metric;   // [n_protected][slot_stride][max_pairs]
  std::vector<uint32_t> tq_count;                           // [n_protected][slot_stride]
  std::vector<uint32_t> y_roots;                            // the roots of the q rows: the ascending union of the lists
  std::vector<uint8_t> tn_kind;                             // [n_protected][n_vertices] HSPF_TN_D_*
  std::vector<uint32_t> tn_p, tn_q, tn_link, tn_via, tn_metric, tn_set;   // [n_protected][n_vertices]
  std::vector<uint32_t> tn_coverage;                        // [n_protected][HSPF_TN_COVERAGE_WORDS]
};
// Per-prefix backup routes (hspf_routes_backup_device) of the same protected roots over the prefix table of a DeviceRoutes: per
// (protected root, prefix) the kind of backup (HSPF_BK_*), the primary slot, the backup slot / metric / flags.  `tilfa`: nullptr, or
// what tilfa() returned for the same protect list (the fallback to the primary link's repair).  supported == false: no such call.
struct BackupOut {
  bool supported = false;
  uint32_t n_protected = 0, n_prefixes = 0, mask_words = 1;
  std::vector<uint8_t> bk_kind, bk_flags;                   // [n_protected][n_prefixes]
  std::vector<uint32_t> bk_primary, bk_slot, bk_metric;
  std::vector<uint64_t> bk_cand_mask, bk_node_mask;         // [n_protected][n_prefixes][mask_words]
  std::vector<uint32_t> bk_coverage;                        // [n_protected][HSPF_BK_COVERAGE_WORDS] (backup_routes_srlg: HSPF_BK_SRLG_COVERAGE_WORDS)
};
// Per-primary backups of the ECMP prefixes (hspf_routes_backup_ecmp_device) of the same protected roots: a stream in CSR form over
// (protected root, prefix), the entries of one prefix in ascending primary slot order.  supported == false: no such call.
struct BackupEcmpOut {
  bool supported = false;
  uint32_t n_protected = 0, n_prefixes = 0;
  std::vector<uint32_t> eb_ptr;                             // [n_protected * n_prefixes + 1]
  std::vector<uint32_t> eb_primary, eb_slot, eb_metric;     // [eb_ptr.back()]
  std::vector<uint8_t> eb_kind, eb_flags;
  std::vector<uint32_t> eb_coverage;                        // [n_protected][HSPF_BK_ECMP_COVERAGE_WORDS]
};
// Per-prefix node-protecting backups (hspf_routes_backup_node_device) of the same protected roots over the prefix table of a
// DeviceRoutes: per (protected root, prefix) with one primary the kind (HSPF_BN_*), the primary slot and the chosen repair.
// supported == false: no such call.
struct BackupNodeOut {
  bool supported = false;
  uint32_t n_protected = 0, n_prefixes = 0;
  std::vector<uint32_t> y_roots;                            // the roots of the rows: the ascending union of both lists
  std::vector<uint8_t> bn_kind;                             // [n_protected][n_prefixes] HSPF_BN_*
  std::vector<uint32_t> bn_primary, bn_p, bn_q, bn_link, bn_via, bn_metric, bn_set_pq, bn_set_pair;
  std::vector<uint32_t> bn_coverage;                        // [n_protected][HSPF_BN_COVERAGE_WORDS]
};
class Engine {
 public:
  virtual ~Engine() = default;
  // `routes`: what routes_device() wrote for `run` and the prefix table given here again (pfx_* / table_flags: the call reads the
  // advertisers); `node` / `pairs`: what rlfa_node() / tilfa_node() returned for the same protect list (nullptr: no such entries; at
  // least one); `backup`: what backup_routes() returned (only bk_kind and bk_flags are read), or nullptr.  The rows of the listed
  // nodes are run on `gr` with `run_flags`.  The default: not supported.
  virtual BackupNodeOut backup_routes_node(Graph &, DeviceRun & /*run*/, DeviceRoutes & /*routes*/, const std::vector<uint32_t> & /*pfx_ptr*/,
                                           const std::vector<uint32_t> & /*pfx_vertex*/, const std::vector<uint32_t> & /*pfx_metric*/,
                                           uint32_t /*table_flags*/, const std::vector<LfaProtect> &, uint32_t /*run_flags*/,
                                           const RlfaNodeOut * /*node*/, const TilfaNodeOut * /*pairs*/, const BackupOut * /*backup*/) {
    return BackupNodeOut{};
  }
  // `routes`: what routes_device() wrote for `run` and the prefix table.  The default: not supported.
  virtual BackupOut backup_routes(DeviceRun & /*run*/, DeviceRoutes & /*routes*/, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/,
                                  const TilfaOut * /*tilfa*/) { return BackupOut{}; }
  // `rlfa`: what rlfa() returned for the same protect list WITH its space tables; `gr` is the forward graph `run` was made on, the
  // PQ-node rows are run on it with `run_flags`.  The default: not supported.
  virtual RlfaNodeOut rlfa_node(Graph &, DeviceRun & /*run*/, const std::vector<LfaProtect> &, uint32_t /*run_flags*/, uint32_t /*lfa_flags*/,
                                const LfaOut * /*lfa*/, const RlfaOut & /*rlfa*/, uint32_t /*max_pq*/) { return RlfaNodeOut{}; }
  // As rlfa_node(); `node`: what rlfa_node() returned for the same protect list (its one-segment repairs stand: HSPF_TN_D_PQ), or
  // nullptr.  The default: not supported.
  virtual TilfaNodeOut tilfa_node(Graph &, DeviceRun & /*run*/, const std::vector<LfaProtect> &, uint32_t /*run_flags*/, uint32_t /*lfa_flags*/,
                                  const LfaOut * /*lfa*/, const RlfaOut & /*rlfa*/, const RlfaNodeOut * /*node*/, uint32_t /*max_pairs*/) { return TilfaNodeOut{}; }
  // `rlfa`: what rlfa() returned for the same protect list WITH its space tables; `gr` is the forward graph.  The default: not supported.
  virtual TilfaOut tilfa(Graph &, DeviceRun & /*run*/, DeviceRun & /*reverse_run*/, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/,
                         const LfaOut * /*lfa*/, const RlfaOut & /*rlfa*/) { return TilfaOut{}; }
  // tilfa()'s inputs, and `pc_dist` [n_pc_rows][n_vertices]: the dist rows of run_failures() on `gr`; pc_row [n_protected][64 *
  // mask_words]: per slot the row of its {HSPF_FAIL_ROOT_LINK, root_link} scenario, HSPF_NO_ROOT for none; run_flags: that run's.
  // The default: not supported (tilfa_pc_sequential() below is the loop an engine that holds its CSR can answer with).
  virtual TilfaPcOut tilfa_pc(Graph &, DeviceRun & /*run*/, DeviceRun & /*reverse_run*/, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/,
                              const LfaOut * /*lfa*/, const RlfaOut & /*rlfa*/, const std::vector<uint32_t> & /*pc_dist*/, uint32_t /*n_pc_rows*/,
                              const std::vector<uint32_t> & /*pc_row*/, uint32_t /*run_flags*/, uint32_t /*max_walk*/) { return TilfaPcOut{}; }
  // lfa() / backup_routes() with loop-freeness towards the pseudonodes of the primaries' LANs; lans[i] belongs to protect[i], the
  // run holds the SPTs rooted at the LANs too.  The defaults: not supported.
  virtual LfaOut lfa_lan(DeviceRun &, const std::vector<LfaProtect> &, const std::vector<LfaLan> &, uint32_t /*lfa_flags*/, bool /*with_masks*/) {
    return LfaOut{};
  }
  virtual BackupOut backup_routes_lan(DeviceRun & /*run*/, DeviceRoutes & /*routes*/, const std::vector<LfaProtect> &, const std::vector<LfaLan> &,
                                      uint32_t /*lfa_flags*/, const TilfaOut * /*tilfa*/) { return BackupOut{}; }
  // The default: not supported (LfaOut::supported == false).
  virtual LfaOut lfa(DeviceRun &, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/, bool /*with_masks*/) { return LfaOut{}; }
  // Per primary slot of every destination with two or more of them: its alternate and what that protects (hspf_lfa_ecmp_device).
  // The default: not supported.
  virtual LfaEcmpOut lfa_ecmp(DeviceRun &, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/) { return LfaEcmpOut{}; }
  // `reverse_run`: the run of the same roots on the upload of the transposed CSR (the forward run itself on a graph whose
  // costs are symmetric); `lfa`: nullptr, or what lfa() returned for the same protect list.  The default: not supported.
  virtual RlfaOut rlfa(Graph &, DeviceRun & /*run*/, DeviceRun & /*reverse_run*/, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/,
                       const LfaOut * /*lfa*/, bool /*with_spaces*/) { return RlfaOut{}; }
  // rlfa() with P, extended P and Q loop-free towards the pseudonode of every slot's LAN (hspf_rlfa_lan_device); lans[i] belongs to
  // protect[i]; both runs hold the SPTs rooted at the LANs too and `reverse_run` is ALWAYS the run on the transposed graph; `lfa`:
  // nullptr, or what lfa_lan() returned.  The result feeds tilfa() unchanged.  The default: not supported.
  virtual RlfaOut rlfa_lan(Graph &, DeviceRun & /*run*/, DeviceRun & /*reverse_run*/, const std::vector<LfaProtect> &, const std::vector<LfaLan> &,
                           uint32_t /*lfa_flags*/, const LfaOut * /*lfa*/, bool /*with_spaces*/) { return RlfaOut{}; }
  // lfa() / rlfa() against shared-risk link groups (hspf_lfa_srlg_device / hspf_rlfa_srlg_device); srlgs[i] belongs to protect[i];
  // both runs hold the SPTs rooted at the members' endpoints too; `lfa`: nullptr, or what lfa_srlg() returned.  The result of
  // rlfa_srlg() feeds tilfa() unchanged.  The defaults: not supported.
  virtual LfaOut lfa_srlg(DeviceRun &, const std::vector<LfaProtect> &, const std::vector<Srlg> &, uint32_t /*lfa_flags*/, bool /*with_masks*/) {
    return LfaOut{};
  }
  virtual RlfaOut rlfa_srlg(Graph &, DeviceRun & /*run*/, DeviceRun & /*reverse_run*/, const std::vector<LfaProtect> &, const std::vector<Srlg> &,
                            uint32_t /*lfa_flags*/, const LfaOut * /*lfa*/, bool /*with_spaces*/) { return RlfaOut{}; }
  // backup_routes() against shared-risk link groups (hspf_routes_backup_srlg_device): srlgs[i] belongs to protect[i], the run holds
  // the SPTs rooted at the members' endpoints too; the prefix table is given again (pfx_* / table_flags: the call reads the
  // advertisers); HSPF_LFA_SRLG_SAFE_REPAIRS in lfa_flags vouches that `tilfa` comes from rlfa_srlg()'s tables.  bk_coverage has
  // HSPF_BK_SRLG_COVERAGE_WORDS words per root.  The default: not supported.
  virtual BackupOut backup_routes_srlg(DeviceRun & /*run*/, DeviceRoutes & /*routes*/, const std::vector<uint32_t> & /*pfx_ptr*/,
                                       const std::vector<uint32_t> & /*pfx_vertex*/, const std::vector<uint32_t> & /*pfx_metric*/,
                                       uint32_t /*table_flags*/, const std::vector<LfaProtect> &, const std::vector<Srlg> &, uint32_t /*lfa_flags*/,
                                       const TilfaOut * /*tilfa*/) { return BackupOut{}; }
  // Per primary slot of every prefix whose route has two or more of them: its backup (hspf_routes_backup_ecmp_device).  `routes`:
  // what routes_device() wrote for `run` and the prefix table given here again (pfx_* / table_flags: the call reads the
  // advertisers); `tilfa`: nullptr, or what tilfa() returned for the same protect list.  The default: not supported.
  virtual BackupEcmpOut backup_routes_ecmp(DeviceRun & /*run*/, DeviceRoutes & /*routes*/, const std::vector<uint32_t> & /*pfx_ptr*/,
                                           const std::vector<uint32_t> & /*pfx_vertex*/, const std::vector<uint32_t> & /*pfx_metric*/,
                                           uint32_t /*table_flags*/, const std::vector<LfaProtect> &, uint32_t /*lfa_flags*/,
                                           const TilfaOut * /*tilfa*/) { return BackupEcmpOut{}; }
  // backup_routes_ecmp() against shared-risk link groups (hspf_routes_backup_ecmp_srlg_device): per primary h an alternate that
  // avoids h's own groups; srlgs[i] belongs to protect[i] and the run holds the members' endpoints' rows, as for backup_routes_srlg();
  // HSPF_LFA_SRLG_SAFE_REPAIRS in lfa_flags vouches for `tilfa`, whose ti_p / ti_link are read too.  eb_coverage has
  // HSPF_BK_ECMP_SRLG_COVERAGE_WORDS words per root.  The default: not supported.
  virtual BackupEcmpOut backup_routes_ecmp_srlg(DeviceRun & /*run*/, DeviceRoutes & /*routes*/, const std::vector<uint32_t> & /*pfx_ptr*/,
                                                const std::vector<uint32_t> & /*pfx_vertex*/, const std::vector<uint32_t> & /*pfx_metric*/,
                                                uint32_t /*table_flags*/, const std::vector<LfaProtect> &, const std::vector<Srlg> &,
                                                uint32_t /*lfa_flags*/, const TilfaOut * /*tilfa*/) { return BackupEcmpOut{}; }
  virtual std::unique_ptr<Graph> upload(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col,
                                        const std::vector<uint32_t> &metric, const std::vector<uint8_t> &vflags,
                                        uint32_t max_path_metric) = 0;
  // LSDB records -> CSR on the engine (hspf_graph_upload_keyed): vertices by 64-bit key in any order, links as
  // (target key, cost), targets unresolved.  nullptr: the engine has no such path (the caller derives the CSR itself and calls
  // upload).  On success csr_* hold the CSR the engine built (vertex index = rank of the key; links to absent keys dropped) and
  // rank[i] the index of input vertex i.
  virtual std::unique_ptr<Graph> upload_keyed(const std::vector<uint64_t> &, const std::vector<uint32_t> &, const std::vector<uint64_t> &,
                                              const std::vector<uint32_t> &, const std::vector<uint8_t> &, uint32_t, std::vector<uint32_t> &,
                                              std::vector<uint32_t> &, std::vector<uint32_t> &, std::vector<uint32_t> &, std::vector<uint8_t> &) { return nullptr; }
  virtual Tables run(Graph &g, const std::vector<uint32_t> &roots, uint32_t run_flags) = 0;
  // Failure scenarios (hspf_run_failures): row r = the run of roots[r] with failures[r] applied, the graph untouched; mask_words as
  // for run() on `roots`.  The default: not supported (an engine without the call; run_failures_sequential() below is the loop
  // itself for a caller that holds the CSR).
  virtual Tables run_failures(Graph &, const std::vector<uint32_t> & /*roots*/, const std::vector<Failure> & /*failures*/, uint32_t /*run_flags*/) {
    throw std::runtime_error("run_failures: not supported by this engine");
  }
  virtual SlotTable slot_table(Graph &g, uint32_t root) = 0;
  // whole rows replaced (hspf_graph_patch): vertices strictly ascending, rows[i] = (col, metric) of vertices[i]
  virtual void patch(Graph &g, const std::vector<uint32_t> &vertices,
                     const std::vector<std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> &rows,
                     const std::vector<uint8_t> &vflags) = 0;
  // device-resident variant (hspf_run_device) + prefix attachment on the device (hspf_routes_device; table CSR by
  // prefix, flags = HSPF_PFX_*)
  virtual std::unique_ptr<DeviceRun> run_device(Graph &g, const std::vector<uint32_t> &roots, uint32_t run_flags) = 0;
  virtual RoutesOut routes(DeviceRun &run, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                           const std::vector<uint32_t> &pfx_metric, uint32_t flags) = 0;
  // The wire step on the device: the same attachment with the tables LEFT on the device, a host table set
  // brought there (the RIB held before), and the comparison + ordered compaction + ONE packed copy of what changed
  // (hspf_routes_diff_device + hspf_routes_pack).  flags may carry HSPF_PFX_RESIDENT (same vectors as the previous call).
  virtual std::unique_ptr<DeviceRoutes> routes_device(DeviceRun &run, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                                                      const std::vector<uint32_t> &pfx_metric, uint32_t flags) = 0;
  virtual std::unique_ptr<DeviceRoutes> routes_upload(const RoutesOut &t, uint32_t n_roots, uint32_t n_prefixes, uint32_t mask_words) = 0;
  virtual RouteRecords routes_changed(DeviceRoutes &old_set, DeviceRoutes &new_set) = 0;
  // routes_changed with the old half in the same record and, with_silent, the HSPF_DIFF_SILENT pairs too: one device call.
  // The default: not supported (RouteEvents::supported == false) — the caller uses routes_changed.
  virtual RouteEvents routes_events(DeviceRoutes &, DeviceRoutes &, bool /*with_silent*/) { return RouteEvents{}; }
  // Several areas, ONE RIB (hspf_rib_clear_device / hspf_rib_fold_device): an empty instance-wide state over `n_prefixes`
  // prefixes and `mask_words` words of instance-wide first-hop slots, and the ordered fold (HSPF_PFX_ORDERED rules) of one
  // area's table into it — `prefix_map`: area prefix -> instance prefix, the area's slots start at word `word_offset`.
  virtual std::unique_ptr<DeviceRoutes> rib_new(uint32_t n_prefixes, uint32_t mask_words) = 0;
  virtual void rib_fold(DeviceRoutes &rib, DeviceRun &run, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                        const std::vector<uint32_t> &pfx_metric, const std::vector<uint32_t> &pfx_origin, const std::vector<uint32_t> &prefix_map,
                        uint32_t area_index, uint32_t word_offset) = 0;
};

// CSR with the rows of `vertices` (strictly ascending) replaced — the host-side twin of hspf_graph_patch.
inline void splice_rows(std::vector<uint32_t> &row_ptr, std::vector<uint32_t> &col, std::vector<uint32_t> &metric,
                        std::vector<uint8_t> &vflags, const std::vector<uint32_t> &vertices,
                        const std::vector<std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> &rows,
                        const std::vector<uint8_t> &new_flags) {
  const uint32_t n = (uint32_t)row_ptr.size() - 1;
  if (!vertices.empty() && vertices.size() <= 16) {
    // a handful of rows (the everyday LSP change): IN PLACE, last row first so that the offsets in front stay valid — the tail
    // behind a row moves once by its change in length, nothing is allocated; then one pass over the row starts behind the first
    std::vector<long> d(vertices.size());
    for (size_t j = vertices.size(); j-- > 0;) {
      const uint32_t u = vertices[j];
      const size_t a = row_ptr[u], old_len = row_ptr[u + 1] - a, new_len = rows[j].first.size();
      d[j] = (long)new_len - (long)old_len;
      if (new_len > old_len) {
        col.insert(col.begin() + a + old_len, new_len - old_len, 0u);
        metric.insert(metric.begin() + a + old_len, new_len - old_len, 0u);
      } else if (new_len < old_len) {
        col.erase(col.begin() + a + new_len, col.begin() + a + old_len);
        metric.erase(metric.begin() + a + new_len, metric.begin() + a + old_len);
      }
      std::copy(rows[j].first.begin(), rows[j].first.end(), col.begin() + a);
      std::copy(rows[j].second.begin(), rows[j].second.end(), metric.begin() + a);
      vflags[u] = new_flags[j];
    }
    long shift = 0;
    size_t j = 0;
    for (uint32_t u = vertices[0]; u <= n; ++u) {                        // row u starts behind every replaced row with a lower index
      while (j < vertices.size() && vertices[j] < u) shift += d[j++];
      row_ptr[u] = (uint32_t)((long)row_ptr[u] + shift);
    }
    return;
  }
  // many rows: the stretches BETWEEN the replaced rows move as blocks into exactly sized arrays (not a million appends)
  long delta = 0;
  for (size_t j = 0; j < vertices.size(); ++j) delta += (long)rows[j].first.size() - (long)(row_ptr[vertices[j] + 1] - row_ptr[vertices[j]]);
  const size_t new_len = (size_t)((long)col.size() + delta);
  std::vector<uint32_t> ncol(new_len), nmet(new_len), nrp(n + 1);
  size_t out = 0;                      // write position in the new arrays
  uint32_t from = 0;                   // first vertex of the pending untouched stretch
  auto copy_stretch = [&](uint32_t to) {                                   // rows [from, to) unchanged: one block, offsets shifted
    if (to <= from) return;
    const uint32_t a = row_ptr[from], b = row_ptr[to];
    std::copy(col.begin() + a, col.begin() + b, ncol.begin() + out);
    std::copy(metric.begin() + a, metric.begin() + b, nmet.begin() + out);
    const long shift = (long)out - (long)a;
    for (uint32_t u = from; u < to; ++u) nrp[u] = (uint32_t)((long)row_ptr[u] + shift);
    out += b - a;
  };
  for (size_t j = 0; j < vertices.size(); ++j) {
    const uint32_t u = vertices[j];
    copy_stretch(u);
    nrp[u] = (uint32_t)out;
    std::copy(rows[j].first.begin(), rows[j].first.end(), ncol.begin() + out);
    std::copy(rows[j].second.begin(), rows[j].second.end(), nmet.begin() + out);
    out += rows[j].first.size();
    vflags[u] = new_flags[j];
    from = u + 1;
  }
  copy_stretch(n);
  nrp[n] = (uint32_t)out;
  row_ptr.swap(nrp); col.swap(ncol); metric.swap(nmet);
}

// The host twin of hspf_tilfa_pc_device: the rule of include/holo_spf_hip.h ("repairs along the post-convergence path") as a
// sequential loop on the caller's CSR.  `fwd`: the forward tables of the run the protect list indexes (dist, flags, mask); space_flags /
// space_via [n_protected][64 * mask_words][n]; alt_flags: nullptr or [n_protected][n]; pc_dist / pc_row / run_flags / max_walk as
// the call's.  Parents are found per visited vertex with a scan of the whole CSR's in-links built once: O(links) memory, no device.
inline TilfaPcOut tilfa_pc_sequential(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                                      const std::vector<uint8_t> &vflags, const Tables &fwd, const std::vector<LfaProtect> &protect,
                                      const std::vector<uint8_t> &space_flags, const std::vector<uint32_t> &space_via, const std::vector<uint8_t> *alt_flags,
                                      const std::vector<uint32_t> &pc_dist, uint32_t n_pc_rows, const std::vector<uint32_t> &pc_row, uint32_t run_flags,
                                      uint32_t max_walk) {
  const uint32_t n = fwd.n_vertices, W = fwd.mask_words, A = HSPF_TIPC_MAX_ADJ;
  const size_t stride = (size_t)64 * W, np = protect.size();
  if (row_ptr.size() != (size_t)n + 1 || vflags.size() != n) throw std::invalid_argument("tilfa_pc: the CSR is not of the tables' size");
  if (max_walk == 0 || max_walk > 65535u) throw std::invalid_argument("tilfa_pc: max_walk outside 1 .. 65535");
  if (space_flags.size() != np * stride * n || space_via.size() != np * stride * n || pc_row.size() != np * stride || pc_dist.size() != (size_t)n_pc_rows * n ||
      (alt_flags && alt_flags->size() != np * n))
    throw std::invalid_argument("tilfa_pc: an input array is not of this protect list");
  for (size_t i = 0; i < np; ++i)
    for (size_t e = 0; e < stride; ++e) {
      const uint32_t r = pc_row[i * stride + e];
      if (r == HSPF_NO_ROOT) continue;
      if (e >= protect[i].nbr.size() || protect[i].nbr[e] == HSPF_NO_ROOT) throw std::invalid_argument("tilfa_pc: pc_row given for a slot that is no candidate");
      if (r >= n_pc_rows) throw std::invalid_argument("tilfa_pc: pc_row >= n_pc_rows");
    }
  // the links a run uses whatever its root: two-way, the source without HSPF_VF_NO_EXPAND; per target (source, position, cost)
  struct In { uint32_t u, j, w; };
  std::vector<std::vector<In>> into(n);
  auto lists = [&](uint32_t t, uint32_t u) { for (uint32_t k = row_ptr[t]; k < row_ptr[t + 1]; ++k) if (col[k] == u) return true; return false; };
  for (uint32_t u = 0; u < n; ++u) {
    if (vflags[u] & HSPF_VF_NO_EXPAND) continue;
    for (uint32_t k = row_ptr[u]; k < row_ptr[u + 1]; ++k)
      if (col[k] < n && lists(col[k], u)) into[col[k]].push_back(In{u, k - row_ptr[u], metric[k]});
  }
  const bool ign = (run_flags & HSPF_RUN_IGNORE_OVERLOAD) != 0;
  TilfaPcOut o;
  o.supported = true; o.n_protected = (uint32_t)np; o.n_vertices = n;
  o.tp_kind.assign(np * n, 0); o.tp_n_adj.assign(np * n, 0); o.tp_flags.assign(np * n, 0);
  o.tp_p.assign(np * n, HSPF_NO_ROOT); o.tp_via.assign(np * n, HSPF_LFA_NO_SLOT); o.tp_q.assign(np * n, HSPF_NO_ROOT); o.tp_metric.assign(np * n, 0);
  o.tp_hop_pos.assign(np * n * A, HSPF_LFA_NO_SLOT); o.tp_hop_head.assign(np * n * A, HSPF_NO_ROOT);
  o.tp_coverage.assign(np * HSPF_TIPC_COVERAGE_WORDS, 0);
  for (size_t i = 0; i < np; ++i) {
    const LfaProtect &pr = protect[i];
    const uint32_t S = pr.root_vertex, K = (uint32_t)pr.nbr.size();
    const uint32_t *dS = fwd.dist.data() + (size_t)pr.root_row * n;
    uint32_t *cov = o.tp_coverage.data() + i * HSPF_TIPC_COVERAGE_WORDS;
    for (uint32_t D = 0; D < n; ++D) {
      const size_t sd = (size_t)pr.root_row * n + D, od = i * n + D;
      if (D == S || !(fwd.flags[sd] & 1u) || dS[D] == HSPF_DIST_INF) continue;
      uint32_t nprim = 0, e = 0;
      for (uint32_t k = 0; k < K; ++k)
        if ((fwd.mask[sd * W + k / 64] >> (k % 64)) & 1u) { if (!nprim) e = k; ++nprim; }
      if (nprim != 1) continue;
      uint32_t cls;
      std::vector<std::pair<uint32_t, uint32_t>> gap;              // (position, head) in the order of recording: q first
      uint32_t p = HSPF_NO_ROOT, q = D, via = HSPF_LFA_NO_SLOT;
      uint64_t rel = 0;
      const size_t si = i * stride + e;
      const uint32_t *pc = pc_row[si] != HSPF_NO_ROOT ? pc_dist.data() + (size_t)pc_row[si] * n : nullptr;
      if (alt_flags && ((*alt_flags)[od] & HSPF_LFA_LINK_PROTECT)) cls = HSPF_TIPC_D_LFA;
      else if (pr.nbr[e] == HSPF_NO_ROOT || !pc || pc[D] == HSPF_DIST_INF) cls = HSPF_TIPC_D_NONE;
      else {
        const uint8_t *sf = space_flags.data() + si * n;
        const uint32_t *sv = space_via.data() + si * n;
        const uint32_t fpos = pr.root_link[e];
        bool lan = false;
        uint32_t cur = D;
        cls = HSPF_TIPC_D_WALK;
        for (uint32_t step = 0; step < max_walk; ++step) {
          const uint8_t f = sf[cur];
          if ((f & HSPF_RLFA_ELIGIBLE) && (f & HSPF_RLFA_IN_Q)) { q = cur; gap.clear(); lan = false; }
          if ((f & HSPF_RLFA_ELIGIBLE) && (f & (HSPF_RLFA_IN_P | HSPF_RLFA_IN_XP)) && (sv[cur] == HSPF_RLFA_VIA_SELF || sv[cur] < K)) {
            p = cur; via = sv[cur];
            rel = via == HSPF_RLFA_VIA_SELF ? (uint64_t)dS[cur] : (uint64_t)pr.cost[via] + fwd.dist[(size_t)pr.nbr_row[via] * n + cur];
            cls = HSPF_TIPC_D_REPAIR;
            break;
          }
          if (cur == S) { p = S; rel = 0; cls = HSPF_TIPC_D_REPAIR; break; }
          uint32_t bu = HSPF_NO_ROOT, bj = HSPF_NO_ROOT;
          for (const In &l : into[cur]) {
            if (!ign && (vflags[l.u] & HSPF_VF_NO_TRANSIT) && !(vflags[l.u] & HSPF_VF_NETWORK) && l.u != S) continue;
            if (l.u == S && l.j == fpos) continue;
            if (pc[l.u] == HSPF_DIST_INF || (uint64_t)pc[l.u] + l.w != pc[cur]) continue;
            if (l.u < bu || (l.u == bu && l.j < bj)) { bu = l.u; bj = l.j; }
          }
          if (bu == HSPF_NO_ROOT) { cls = HSPF_TIPC_D_NONE; break; }
          if (!gap.empty() && (vflags[cur] & HSPF_VF_NETWORK)) lan = true;
          gap.emplace_back(bj, cur);
          cur = bu;
        }
        if (cls == HSPF_TIPC_D_REPAIR) cls = gap.size() > A ? HSPF_TIPC_D_LONG : lan ? HSPF_TIPC_D_LAN : HSPF_TIPC_D_REPAIR;
        if (cls == HSPF_TIPC_D_REPAIR) {
          const uint32_t pcp = p == S ? 0u : pc[p];
          const uint64_t t = rel + pc[D] - pcp;
          o.tp_p[od] = p; o.tp_via[od] = via; o.tp_q[od] = q; o.tp_n_adj[od] = (uint8_t)gap.size();
          o.tp_metric[od] = (uint32_t)std::min<uint64_t>(t, 0xFFFFFFFEull);
          o.tp_flags[od] = (uint8_t)((rel == pcp ? HSPF_TIPC_ON_PC : 0u) | (p == S ? HSPF_TIPC_P_IS_ROOT : 0u) | (q == D ? HSPF_TIPC_Q_IS_DEST : 0u));
          for (size_t h = 0; h < gap.size(); ++h) {
            o.tp_hop_pos[od * A + h] = gap[gap.size() - 1 - h].first; o.tp_hop_head[od * A + h] = gap[gap.size() - 1 - h].second;
          }
          ++cov[7 + gap.size()];
        }
      }
      o.tp_kind[od] = (uint8_t)cls;
      ++cov[0]; ++cov[cls];
    }
  }
  return o;
}

// The host twin of hspf_run_failures: the sequential SPF loop on the caller's CSR with the two skips — the
// root's failed link, and every link into the excluded vertex (which is then never labelled, never popped, never expanded).  Pops in
// (distance, vertex) order; flags are HSPF_RF_IN_SPT alone.  Throws std::invalid_argument where the C call returns HSPF_E_INVAL.
inline Tables run_failures_sequential(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                                      const std::vector<uint8_t> &vflags, uint32_t max_path_metric, const std::vector<uint32_t> &roots,
                                      const std::vector<Failure> &failures, uint32_t run_flags) {
  const uint32_t n = (uint32_t)vflags.size(), R = (uint32_t)roots.size();
  if (failures.size() != roots.size()) throw std::invalid_argument("run_failures: one failure per root");
  if (run_flags & (HSPF_RUN_POP_RANK | HSPF_RUN_COUNT_ROWS)) throw std::invalid_argument("run_failures: HSPF_RUN_POP_RANK / HSPF_RUN_COUNT_ROWS are not accepted");
  for (uint32_t r = 0; r < R; ++r) {
    if (roots[r] == HSPF_NO_ROOT) continue;
    if (roots[r] >= n) throw std::invalid_argument("run_failures: root out of range");
    const Failure &f = failures[r];
    if (f.kind == HSPF_FAIL_ROOT_LINK) { if (f.arg >= row_ptr[roots[r] + 1] - row_ptr[roots[r]]) throw std::invalid_argument("run_failures: link position beyond the root's row"); }
    else if (f.kind == HSPF_FAIL_VERTEX) { if (f.arg >= n || f.arg == roots[r]) throw std::invalid_argument("run_failures: excluded vertex out of range or the root"); }
    else if (f.kind != HSPF_FAIL_NONE) throw std::invalid_argument("run_failures: unknown failure kind");
  }
  // the two-way check, once: link k of u's row is kept when its target lists u
  std::vector<uint8_t> twoway(col.size(), 0);
  for (uint32_t u = 0; u < n; ++u)
    for (uint32_t k = row_ptr[u]; k < row_ptr[u + 1]; ++k) {
      const uint32_t t = col[k];
      for (uint32_t k2 = row_ptr[t]; k2 < row_ptr[t + 1] && !twoway[k]; ++k2) twoway[k] = col[k2] == u;
    }
  // slot bases of a root: H = [root] ++ networks reached through networks only, over kept links in row order
  std::vector<uint32_t> base(n);
  auto slots_of = [&](uint32_t root) {
    std::fill(base.begin(), base.end(), 0xFFFFFFFFu);
    std::vector<uint32_t> q{root};
    base[root] = 0;
    uint32_t total = row_ptr[root + 1] - row_ptr[root];
    for (size_t qi = 0; qi < q.size(); ++qi)
      for (uint32_t k = row_ptr[q[qi]]; k < row_ptr[q[qi] + 1]; ++k) {
        const uint32_t t = col[k];
        if (!twoway[k] || !(vflags[t] & HSPF_VF_NETWORK) || base[t] != 0xFFFFFFFFu) continue;
        base[t] = total; total += row_ptr[t + 1] - row_ptr[t];
        q.push_back(t);
      }
    return total;
  };
  Tables t;
  t.n_roots = R; t.n_vertices = n; t.mask_words = 1;
  for (uint32_t r = 0; r < R; ++r) if (roots[r] != HSPF_NO_ROOT) t.mask_words = std::max(t.mask_words, (slots_of(roots[r]) + 63u) / 64u);
  const uint32_t W = t.mask_words;
  const size_t rn = (size_t)R * n;
  t.dist.assign(rn, HSPF_DIST_INF); t.hops.assign(rn, 0); t.flags.assign(rn, 0); t.mask.assign(rn * W, 0);
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t root = roots[r];
    if (root == HSPF_NO_ROOT) continue;
    const uint32_t fpos = failures[r].kind == HSPF_FAIL_ROOT_LINK ? failures[r].arg : 0xFFFFFFFFu;
    const uint32_t fvtx = failures[r].kind == HSPF_FAIL_VERTEX ? failures[r].arg : 0xFFFFFFFFu;
    slots_of(root);
    uint32_t *dist = t.dist.data() + (size_t)r * n;
    uint16_t *hops = t.hops.data() + (size_t)r * n, *flags = t.flags.data() + (size_t)r * n;
    uint64_t *mask = t.mask.data() + (size_t)r * n * W;
    std::map<std::pair<uint32_t, uint32_t>, char> cand;            // (distance, vertex): the reference's ordered candidate list
    dist[root] = 0; cand[{0u, root}] = 1;
    while (!cand.empty()) {
      const uint32_t v = cand.begin()->first.second;
      cand.erase(cand.begin());
      flags[v] = HSPF_RF_IN_SPT;
      const uint8_t vf = vflags[v];
      const uint16_t vh = hops[v];
      if (vf & HSPF_VF_NO_EXPAND) continue;
      if (vh != 0 && !(vf & HSPF_VF_NETWORK) && !(run_flags & HSPF_RUN_IGNORE_OVERLOAD) && (vf & HSPF_VF_NO_TRANSIT)) continue;
      for (uint32_t k = row_ptr[v]; k < row_ptr[v + 1]; ++k) {
        if (!twoway[k]) continue;
        const uint32_t tv = col[k];
        if (flags[tv] & HSPF_RF_IN_SPT) continue;
        if (tv == fvtx || (v == root && k - row_ptr[v] == fpos)) continue;      // the two skips
        const uint64_t s64 = (uint64_t)dist[v] + metric[k];
        const uint32_t d = s64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s64;
        if (d > max_path_metric) continue;
        const bool on_cand = cand.count({dist[tv], tv}) != 0;
        if (on_cand && d > dist[tv]) continue;
        if (!on_cand || d < dist[tv]) {
          if (on_cand) cand.erase({dist[tv], tv});
          dist[tv] = d;
          hops[tv] = (vflags[tv] & HSPF_VF_NETWORK) ? vh : (uint16_t)(vh == 0xFFFFu ? 0xFFFFu : vh + 1u);
          std::fill(mask + (size_t)tv * W, mask + (size_t)(tv + 1) * W, 0ull);
          cand[{d, tv}] = 1;
        }
        if (vh == 0) {
          if (!(vflags[tv] & HSPF_VF_NETWORK) || (run_flags & HSPF_RUN_NET_NEXTHOPS)) {
            const uint32_t sl = base[v] + (k - row_ptr[v]);
            mask[(size_t)tv * W + sl / 64u] |= 1ull << (sl % 64u);
          }
        } else {
          for (uint32_t w = 0; w < W; ++w) mask[(size_t)tv * W + w] |= mask[(size_t)v * W + w];
        }
      }
    }
  }
  return t;
}

// ---- addresses and prefixes (BTreeMap<IpNetwork, _> / BTreeMap<IpAddr, _> order) -----------------------------------
struct IpKey {                        // (version, 128-bit address, prefix length)
  int version = 4;
  std::array<uint8_t, 16> addr{};
  int len = 0;
  bool operator<(const IpKey &o) const { return std::tie(version, addr, len) < std::tie(o.version, o.addr, o.len); }
  bool operator==(const IpKey &o) const { return version == o.version && addr == o.addr && len == o.len; }
};
// "a.b.c.d[/len]" without a heap allocation (the general routine below makes six strings per address: a quarter of the compiled
// twin's route computation at 120 000 prefixes was this).  false: not plain dotted-quad text — the caller takes the general routine.
inline bool parse_ip4_fast(const std::string &text, IpKey &k) {
  const char *p = text.data(), *end = p + text.size();
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) {
    uint32_t o = 0; int nd = 0;
    while (p != end && *p >= '0' && *p <= '9' && nd < 3) { o = o * 10u + (uint32_t)(*p - '0'); ++p; ++nd; }
    if (nd == 0 || o > 255u) return false;
    v = (v << 8) | o;
    if (i < 3) { if (p == end || *p != '.') return false; ++p; }
  }
  int len = 32;
  if (p != end) {
    if (*p != '/') return false;
    ++p;
    int nd = 0; len = 0;
    while (p != end && *p >= '0' && *p <= '9' && nd < 2) { len = len * 10 + (*p - '0'); ++p; ++nd; }
    if (nd == 0 || p != end || len > 32) return false;
  }
  if (len < 32) v = len == 0 ? 0u : (v & (0xFFFFFFFFu << (32 - len)));       // network address: host bits cleared (strict = false)
  k.version = 4; k.addr.fill(0); k.len = len;
  k.addr[12] = (uint8_t)(v >> 24); k.addr[13] = (uint8_t)(v >> 16); k.addr[14] = (uint8_t)(v >> 8); k.addr[15] = (uint8_t)v;
  return true;
}
inline IpKey parse_ip(const std::string &text) {             // "a.b.c.d[/len]" or IPv6 text form (with "::")
  IpKey k;
  if (parse_ip4_fast(text, k)) return k;
  k = IpKey{};
  std::string a = text;
  const size_t slash = a.find('/');
  int len = -1;
  if (slash != std::string::npos) { len = std::stoi(a.substr(slash + 1)); a = a.substr(0, slash); }
  if (a.find(':') == std::string::npos) {
    k.version = 4;
    size_t pos = 0;
    for (int i = 0; i < 4; ++i) {
      const size_t dot = a.find('.', pos);
      k.addr[12 + i] = (uint8_t)std::stoi(a.substr(pos, dot == std::string::npos ? std::string::npos : dot - pos));
      pos = dot == std::string::npos ? a.size() : dot + 1;
    }
    k.len = len < 0 ? 32 : len;
    if (k.len < 32) {                                        // network address: host bits cleared (strict = false)
      uint32_t v = ((uint32_t)k.addr[12] << 24) | ((uint32_t)k.addr[13] << 16) | ((uint32_t)k.addr[14] << 8) | k.addr[15];
      v = k.len == 0 ? 0 : (v & (0xFFFFFFFFu << (32 - k.len)));
      k.addr[12] = v >> 24; k.addr[13] = v >> 16; k.addr[14] = v >> 8; k.addr[15] = v;
    }
    return k;
  }
  k.version = 6;
  std::vector<uint16_t> head, tail;
  bool in_tail = false;
  size_t pos = 0;
  if (a.rfind("::", 0) == 0) { in_tail = true; pos = 2; }
  while (pos < a.size()) {
    size_t c = a.find(':', pos);
    std::string grp = a.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    if (grp.empty()) { in_tail = true; pos = c + 1; continue; }
    (in_tail ? tail : head).push_back((uint16_t)std::stoul(grp, nullptr, 16));
    if (c == std::string::npos) break;
    if (c + 1 < a.size() && a[c + 1] == ':') { in_tail = true; pos = c + 2; } else pos = c + 1;
  }
  std::vector<uint16_t> g(8, 0);
  for (size_t i = 0; i < head.size() && i < 8; ++i) g[i] = head[i];
  for (size_t i = 0; i < tail.size() && i < 8; ++i) g[8 - tail.size() + i] = tail[i];
  for (int i = 0; i < 8; ++i) { k.addr[2 * i] = g[i] >> 8; k.addr[2 * i + 1] = g[i] & 0xFF; }
  k.len = len < 0 ? 128 : len;
  for (int bit = k.len; bit < 128; ++bit) k.addr[bit / 8] &= ~(uint8_t)(0x80u >> (bit % 8));
  return k;
}


// ---- the wire step's message (what goes on the ibus per route: RouteIpAdd / RouteIpDel) --------------------------------
struct IbusMsg {
  bool add = true;
  std::string prefix;
  uint32_t metric = 0;
  std::vector<std::pair<int, std::string>> nexthops;       // (ifindex, address), as the reference's BTreeSet<Nexthop> orders them
  bool operator==(const IbusMsg &o) const { return add == o.add && prefix == o.prefix && (!add || (metric == o.metric && nexthops == o.nexthops)); }
};

// ---- the product engine: libholo_spf_hip.so through the C ABI ---------------------------------------------------------
class HipGraph : public Graph {
 public:
  HipGraph(hspf_ctx *c, hspf_graph *g) : ctx(c), g(g) {}
  ~HipGraph() override { if (g) hspf_graph_free(ctx, g); }
  hspf_ctx *ctx;
  hspf_graph *g;
};
// Device and page-locked host blocks of the objects below, kept for reuse: a running instance makes the same few allocations
// every SPF event (run tables, route tables, staging), and hipMalloc / hipFree cost 10-50 us each and synchronise the device
// (the LSP-change pipeline of RibPipeline: 0.94 -> ~0.7 ms, profiles/r05_notes.md).  Blocks are handed out by exact size class
// (rounded up to 64 KB); every engine call that reads or writes them is synchronous, so a returned block is idle.  Like the
// engine and its context the pool belongs to ONE thread (the protocol instance's): no locking.
class HipPool {
 public:
  ~HipPool() {
    for (auto &kv : dev_) for (void *p : kv.second) (void)hipFree(p);
    for (auto &kv : pin_) for (void *p : kv.second) (void)hipHostFree(p);
  }
  static size_t cls(size_t bytes) { return (std::max<size_t>(bytes, 1) + 65535) & ~size_t(65535); }
  void *dev(size_t bytes) {
    auto &fl = dev_[cls(bytes)];
    if (!fl.empty()) { void *p = fl.back(); fl.pop_back(); return p; }
    void *p = nullptr;
    if (hipMalloc(&p, cls(bytes)) != hipSuccess) throw std::runtime_error("hipMalloc failed");
    return p;
  }
  void dev_free(void *p, size_t bytes) { if (p) dev_[cls(bytes)].push_back(p); }
  void *pinned(size_t bytes) {
    auto &fl = pin_[cls(bytes)];
    if (!fl.empty()) { void *p = fl.back(); fl.pop_back(); return p; }
    void *p = nullptr;
    if (hipHostMalloc(&p, cls(bytes), hipHostMallocDefault) != hipSuccess) throw std::runtime_error("hipHostMalloc failed");
    return p;
  }
  void pinned_free(void *p, size_t bytes) { if (p) pin_[cls(bytes)].push_back(p); }
 private:
  std::map<size_t, std::vector<void *>> dev_, pin_;
};
// One device request from the pool, handed back when the scope ends — the way out an exception takes included.
class HipLease {
 public:
  HipLease(HipPool &pool, size_t bytes, bool wanted = true) : pool_(pool), bytes_(bytes), p_(wanted ? pool.dev(bytes) : nullptr) {}
  HipLease(const HipLease &) = delete;
  HipLease &operator=(const HipLease &) = delete;
  ~HipLease() { pool_.dev_free(p_, bytes_); }
  template <typename T> T *as() const { return static_cast<T *>(p_); }
 private:
  HipPool &pool_;
  size_t bytes_;
  void *p_;
};
// A cursor over one device block: arrays in the order they are asked for (64-bit arrays first, then words, then bytes: every
// array stays aligned), host vectors copied in and out, and in `ok` whether every copy went through (after the first that did
// not, the rest are skipped).  Without a block it is the copies and their flag alone.
class DevCursor {
 public:
  DevCursor() = default;
  explicit DevCursor(const HipLease &block) : at_(block.as<uint8_t>()) {}
  explicit DevCursor(void *block) : at_(static_cast<uint8_t *>(block)) {}
  template <typename T> T *take(size_t count) { T *p = reinterpret_cast<T *>(at_); at_ += count * sizeof(T); return p; }
  template <typename T> void upload(T *dst, const std::vector<T> &src) {
    ok = ok && (src.empty() || hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  }
  template <typename T> T *put(const std::vector<T> &src) { T *dst = take<T>(src.size()); upload(dst, src); return dst; }
  template <typename T> void fetch(std::vector<T> &vec, const T *src, size_t count) {
    vec.resize(count);
    ok = ok && (count == 0 || hipMemcpy(vec.data(), src, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
  }
  bool ok = true;
 private:
  uint8_t *at_ = nullptr;
};
class HipDeviceRun : public DeviceRun {             // dist / hops / flags / masks of one run in device buffers of the engine's pool
 public:
  explicit HipDeviceRun(std::shared_ptr<HipPool> pool) : pool_(std::move(pool)) {}
  ~HipDeviceRun() override {
    pool_->dev_free(dist, rn() * 4); pool_->dev_free(hops, rn() * 2); pool_->dev_free(flags, rn() * 2); pool_->dev_free(mask, rn() * 8 * mask_words);
    pool_->pinned_free(stage_, stage_bytes_);
  }
  void alloc() {
    dist = (uint32_t *)pool_->dev(rn() * 4); hops = (uint16_t *)pool_->dev(rn() * 2); flags = (uint16_t *)pool_->dev(rn() * 2);
    mask = (uint64_t *)pool_->dev(rn() * 8 * mask_words);
  }
  Tables host_tables() override {
    Tables t;
    t.n_roots = n_roots; t.n_vertices = n_vertices; t.mask_words = mask_words;
    t.dist.resize(rn()); t.hops.resize(rn()); t.flags.resize(rn()); t.mask.resize(rn() * mask_words);
    if (hipMemcpy(t.dist.data(), dist, rn() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(t.hops.data(), hops, rn() * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(t.flags.data(), flags, rn() * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(t.mask.data(), mask, rn() * 8 * mask_words, hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("hipMemcpy of the run tables failed");
    return t;
  }
  // into ONE page-locked block of the pool (bus speed, no std::vector to size and fill): [mask (when asked for) | dist | hops | flags]
  TablesView host_view(bool with_mask) override {
    const size_t mb = with_mask ? rn() * 8 * mask_words : 0, need = mb + rn() * 8;
    if (!stage_ || stage_bytes_ < need || (with_mask && !stage_mask_)) {
      pool_->pinned_free(stage_, stage_bytes_);
      stage_ = (char *)pool_->pinned(need); stage_bytes_ = need; stage_mask_ = with_mask; staged_ = false;
    }
    char *pm = stage_, *pd = stage_ + (stage_mask_ ? rn() * 8 * mask_words : 0), *ph = pd + rn() * 4, *pf = ph + rn() * 2;
    if (!staged_) {
      bool ok = hipMemcpy(pd, dist, rn() * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(ph, hops, rn() * 2, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(pf, flags, rn() * 2, hipMemcpyDeviceToHost) == hipSuccess;
      if (ok && stage_mask_) ok = hipMemcpy(pm, mask, rn() * 8 * mask_words, hipMemcpyDeviceToHost) == hipSuccess;
      if (!ok) throw std::runtime_error("hipMemcpy of the run tables failed");
      staged_ = true;
    }
    return TablesView{(const uint32_t *)pd, (const uint16_t *)ph, (const uint16_t *)pf, stage_mask_ ? (const uint64_t *)pm : nullptr, n_roots, n_vertices, mask_words};
  }
  uint32_t *dist = nullptr; uint16_t *hops = nullptr, *flags = nullptr; uint64_t *mask = nullptr;
 private:
  size_t rn() const { return (size_t)n_roots * n_vertices; }
  std::shared_ptr<HipPool> pool_;
  char *stage_ = nullptr; size_t stage_bytes_ = 0; bool stage_mask_ = false, staged_ = false;
};
class HipDeviceRoutes : public DeviceRoutes {       // best_metric / best_entry / nexthop_mask of one table set in device buffers of the engine's pool
 public:
  explicit HipDeviceRoutes(std::shared_ptr<HipPool> pool) : pool_(std::move(pool)) {}
  ~HipDeviceRoutes() override {
    pool_->dev_free(bm, rp() * 4); pool_->dev_free(be, rp() * 4); pool_->dev_free(nm, rp() * 8 * mask_words); pool_->dev_free(org, std::max<size_t>(n_prefixes, 1) * 4);
  }
  RoutesOut host() override {
    RoutesOut o;
    const size_t n = (size_t)n_roots * n_prefixes;
    o.best_metric.resize(n); o.best_entry.resize(n); o.nexthop_mask.resize(n * mask_words);
    if (n && (hipMemcpy(o.best_metric.data(), bm, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(o.best_entry.data(), be, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(o.nexthop_mask.data(), nm, n * 8 * mask_words, hipMemcpyDeviceToHost) != hipSuccess))
      throw std::runtime_error("hipMemcpy of the route tables failed");
    return o;
  }
  bool alloc() {
    bm = (uint32_t *)pool_->dev(rp() * 4); be = (uint32_t *)pool_->dev(rp() * 4); nm = (uint64_t *)pool_->dev(rp() * 8 * mask_words);
    return true;
  }
  void alloc_origin() { org = (uint32_t *)pool_->dev(std::max<size_t>(n_prefixes, 1) * 4); }
  hspf_routes raw() const { return hspf_routes{bm, be, nm}; }
  uint32_t *bm = nullptr, *be = nullptr; uint64_t *nm = nullptr;
  uint32_t *org = nullptr;             // rib_new only: the owners' origins (hspf_rib_device.origin)
 private:
  size_t rp() const { return std::max<size_t>((size_t)n_roots * n_prefixes, 1); }
  std::shared_ptr<HipPool> pool_;
};
class HipEngine : public Engine {
 public:
  explicit HipEngine(int device = 0) {
    const int rc = hspf_init(device, &ctx_);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_init: ") + hspf_strerror(rc));   // no CPU fallback
  }
  ~HipEngine() override { if (diff_) (void)hipFree(diff_); if (ev_pin_) hspf_host_free(ctx_, ev_pin_); if (pin_) hspf_host_free(ctx_, pin_); if (ctx_) hspf_shutdown(ctx_); }
  hspf_ctx *raw() const { return ctx_; }
  std::unique_ptr<Graph> upload(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col,
                                const std::vector<uint32_t> &metric, const std::vector<uint8_t> &vflags,
                                uint32_t max_path_metric) override {
    hspf_csr csr{(uint32_t)vflags.size(), (uint32_t)col.size(), row_ptr.data(), col.data(), metric.data(), vflags.data(), max_path_metric};
    hspf_graph *g = nullptr;
    const int rc = hspf_graph_upload(ctx_, &csr, &g);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_graph_upload: ") + hspf_last_error(ctx_));
    return std::make_unique<HipGraph>(ctx_, g);
  }
  std::unique_ptr<Graph> upload_keyed(const std::vector<uint64_t> &vkey, const std::vector<uint32_t> &vrow, const std::vector<uint64_t> &tkey,
                                      const std::vector<uint32_t> &tmet, const std::vector<uint8_t> &vfl, uint32_t max_path_metric, std::vector<uint32_t> &rank,
                                      std::vector<uint32_t> &row_ptr, std::vector<uint32_t> &col, std::vector<uint32_t> &metric, std::vector<uint8_t> &vflags) override {
    const uint32_t n = (uint32_t)vkey.size();
    hspf_keyed_lsdb k{n, (uint32_t)tkey.size(), vkey.data(), vrow.data(), tkey.data(), tmet.data(), vfl.data(), max_path_metric};
    hspf_graph *g = nullptr;
    rank.resize(n);
    const int rc = hspf_graph_upload_keyed(ctx_, &k, &g, rank.data());
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_graph_upload_keyed: ") + hspf_last_error(ctx_));
    auto out = std::make_unique<HipGraph>(ctx_, g);
    // the CSR as the engine built it: the twins' slot replay, refresh and Spt queries walk it on the host
    auto fetch = [&](uint32_t which, void *dst, size_t bytes) {
      size_t got = 0;
      if (hspf_graph_export(ctx_, g, which, dst, bytes, &got) != HSPF_OK || got != bytes) throw std::runtime_error(std::string("hspf_graph_export: ") + hspf_last_error(ctx_));
    };
    const uint32_t e = hspf_graph_n_edges(g);
    row_ptr.resize((size_t)n + 1); col.resize(e); metric.resize(e); vflags.resize(n);
    fetch(HSPF_GX_ROW_PTR, row_ptr.data(), ((size_t)n + 1) * 4);
    if (e) { fetch(HSPF_GX_COL, col.data(), (size_t)e * 4); fetch(HSPF_GX_METRIC, metric.data(), (size_t)e * 4); }
    fetch(HSPF_GX_VFLAGS, vflags.data(), n);
    return out;
  }
  // One run, tables on the host.  Since ABI 7 through the PACKED hand-off (hspf_run_packed: one word per (root, vertex) into a
  // page-locked buffer the engine keeps, a quarter of hspf_run's bytes over the bus) and decoded into the twins' tables
  // here; runs whose results do not fit packed words (more than 24 first-hop slots), and runs that ask for the pop order,
  // take hspf_run as before.  `last_handoff` says which way the last run went and what it cost.
  struct Handoff { bool packed = false; uint32_t word_bytes = 0; double run_ms = 0, alloc_ms = 0, decode_ms = 0; };   // alloc: the twins' own table vectors
  Handoff last_handoff;
  Tables run(Graph &gr, const std::vector<uint32_t> &roots, uint32_t run_flags) override {
    hspf_graph *g = static_cast<HipGraph &>(gr).g;
    Tables t;
    t.n_roots = (uint32_t)roots.size();
    t.n_vertices = hspf_graph_n_vertices(g);
    const size_t rn = (size_t)t.n_roots * t.n_vertices;
    last_handoff = Handoff{};
    const auto t0 = std::chrono::steady_clock::now();
    if (!(run_flags & HSPF_RUN_POP_RANK) && use_packed) {
      if (pin_cap_ < rn * 8) {
        if (pin_) hspf_host_free(ctx_, pin_);
        pin_ = nullptr; pin_cap_ = 0;
        if (hspf_host_alloc(ctx_, rn * 8, &pin_) != HSPF_OK) throw std::runtime_error(std::string("hspf_host_alloc: ") + hspf_last_error(ctx_));
        pin_cap_ = rn * 8;
      }
      hspf_packed_layout ly{};
      std::vector<uint8_t> status(t.n_roots, 0);
      const int rc = hspf_run_packed(ctx_, g, roots.data(), t.n_roots, run_flags, pin_, pin_cap_, &ly, status.data());
      if (rc == HSPF_OK) {
        const auto t1 = std::chrono::steady_clock::now();
        t.mask_words = 1;
        t.dist.resize(rn); t.hops.resize(rn); t.flags.resize(rn); t.mask.resize(rn);
        const auto t1b = std::chrono::steady_clock::now();
        for (uint32_t r = 0; r < t.n_roots; ++r) {
          const uint16_t ex = (status[r] & HSPF_ROOT_EXACT) ? (uint16_t)HSPF_RF_EXACT : (uint16_t)0;
          const size_t o = (size_t)r * t.n_vertices;
          if (ly.word_bytes == 4) decode_row<uint32_t>((const uint32_t *)pin_ + o, ly, ex, t, o);
          else decode_row<uint64_t>((const uint64_t *)pin_ + o, ly, ex, t, o);
        }
        const auto t2 = std::chrono::steady_clock::now();
        last_handoff = Handoff{true, ly.word_bytes, std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t1b - t1).count(),
                               std::chrono::duration<double, std::milli>(t2 - t1b).count()};
        return t;
      }
      if (rc != HSPF_E_NO_PACKED) throw std::runtime_error(std::string("hspf_run_packed: ") + hspf_last_error(ctx_));
    }
    int rc = hspf_mask_words(ctx_, g, roots.data(), t.n_roots, &t.mask_words);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_mask_words: ") + hspf_last_error(ctx_));
    t.dist.resize(rn); t.hops.resize(rn); t.flags.resize(rn); t.mask.resize(rn * t.mask_words);
    if (run_flags & HSPF_RUN_POP_RANK) t.pop_rank.resize(rn);
    hspf_result out{t.dist.data(), t.hops.data(), t.flags.data(), t.mask.data(), t.mask_words,
                    (run_flags & HSPF_RUN_POP_RANK) ? t.pop_rank.data() : nullptr};
    rc = hspf_run(ctx_, g, roots.data(), t.n_roots, run_flags, &out);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_run: ") + hspf_last_error(ctx_));
    last_handoff.run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return t;
  }
  bool use_packed = true;              // false: hspf_run for every run (the A/B of tests and of the end-to-end timing)
  Tables run_failures(Graph &gr, const std::vector<uint32_t> &roots, const std::vector<Failure> &failures, uint32_t run_flags) override {
    hspf_graph *g = static_cast<HipGraph &>(gr).g;
    if (failures.size() != roots.size()) throw std::runtime_error("run_failures: one failure per root");
    Tables t;
    t.n_roots = (uint32_t)roots.size();
    t.n_vertices = hspf_graph_n_vertices(g);
    int rc = hspf_mask_words(ctx_, g, roots.data(), t.n_roots, &t.mask_words);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_mask_words: ") + hspf_last_error(ctx_));
    const size_t rn = (size_t)t.n_roots * t.n_vertices;
    t.dist.resize(rn); t.hops.resize(rn); t.flags.resize(rn); t.mask.resize(rn * t.mask_words);
    std::vector<hspf_failure> ff;
    for (const Failure &f : failures) ff.push_back(hspf_failure{f.kind, f.arg});
    hspf_result out{t.dist.data(), t.hops.data(), t.flags.data(), t.mask.data(), t.mask_words, nullptr};
    rc = hspf_run_failures(ctx_, g, roots.data(), ff.data(), t.n_roots, run_flags, &out);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_run_failures: ") + hspf_last_error(ctx_));
    return t;
  }
  SlotTable slot_table(Graph &gr, uint32_t root) override {
    hspf_graph *g = static_cast<HipGraph &>(gr).g;
    SlotTable st;
    const int cnt = hspf_slot_table(ctx_, g, root, nullptr, nullptr, 0, &st.total);
    if (cnt < 0) throw std::runtime_error(std::string("hspf_slot_table: ") + hspf_last_error(ctx_));
    st.vertex.resize(cnt); st.base.resize(cnt);
    hspf_slot_table(ctx_, g, root, st.vertex.data(), st.base.data(), (uint32_t)cnt, &st.total);
    return st;
  }
  void patch(Graph &gr, const std::vector<uint32_t> &vertices,
             const std::vector<std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> &rows, const std::vector<uint8_t> &vflags) override {
    std::vector<uint32_t> rp{0}, c, m;
    for (auto &r : rows) { c.insert(c.end(), r.first.begin(), r.first.end()); m.insert(m.end(), r.second.begin(), r.second.end()); rp.push_back((uint32_t)c.size()); }
    if (c.empty()) { c.push_back(0); m.push_back(0); }              // non-NULL pointers for an all-empty delta
    hspf_rows d{(uint32_t)vertices.size(), vertices.data(), rp.data(), c.data(), m.data(), vflags.data()};
    const int rc = hspf_graph_patch(ctx_, static_cast<HipGraph &>(gr).g, &d);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_graph_patch: ") + hspf_last_error(ctx_));
  }
  std::unique_ptr<DeviceRun> run_device(Graph &gr, const std::vector<uint32_t> &roots, uint32_t run_flags) override {
    hspf_graph *g = static_cast<HipGraph &>(gr).g;
    auto r = std::make_unique<HipDeviceRun>(pool_);
    r->n_roots = (uint32_t)roots.size(); r->n_vertices = hspf_graph_n_vertices(g);
    int rc = hspf_mask_words(ctx_, g, roots.data(), r->n_roots, &r->mask_words);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_mask_words: ") + hspf_last_error(ctx_));
    r->alloc();
    hspf_result out{r->dist, r->hops, r->flags, r->mask, r->mask_words, nullptr};
    rc = hspf_run_device(ctx_, g, roots.data(), r->n_roots, run_flags, &out);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_run_device: ") + hspf_last_error(ctx_));
    return r;
  }
  RoutesOut routes(DeviceRun &run, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                   const std::vector<uint32_t> &pfx_metric, uint32_t flags) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    const uint32_t P = (uint32_t)pfx_ptr.size() - 1;
    RoutesOut o;
    const size_t rp = (size_t)r.n_roots * P;
    o.best_metric.assign(rp, 0xFFFFFFFFu); o.best_entry.assign(rp, 0xFFFFFFFFu); o.nexthop_mask.assign(rp * r.mask_words, 0);
    if (P == 0) return o;
    uint32_t *bm = (uint32_t *)pool_->dev(rp * 4), *be = (uint32_t *)pool_->dev(rp * 4);
    uint64_t *nm = (uint64_t *)pool_->dev(rp * 8 * r.mask_words);
    const hspf_prefix_table tab = prefix_table(pfx_ptr, pfx_vertex, pfx_metric, flags);
    hspf_routes ro{bm, be, nm};
    const int rc = hspf_routes_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, &tab, &ro);
    bool ok = rc == HSPF_OK && hipMemcpy(o.best_metric.data(), bm, rp * 4, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(o.best_entry.data(), be, rp * 4, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(o.nexthop_mask.data(), nm, rp * 8 * r.mask_words, hipMemcpyDeviceToHost) == hipSuccess;
    pool_->dev_free(bm, rp * 4); pool_->dev_free(be, rp * 4); pool_->dev_free(nm, rp * 8 * r.mask_words);
    if (!ok) throw std::runtime_error(std::string("hspf_routes_device: ") + hspf_last_error(ctx_));
    return o;
  }
  std::unique_ptr<DeviceRoutes> routes_device(DeviceRun &run, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                                              const std::vector<uint32_t> &pfx_metric, uint32_t flags) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    auto o = std::make_unique<HipDeviceRoutes>(pool_);
    o->n_roots = r.n_roots; o->n_prefixes = (uint32_t)pfx_ptr.size() - 1; o->mask_words = r.mask_words;
    if (!o->alloc()) throw std::runtime_error("hipMalloc of the route tables failed");
    if (o->n_prefixes == 0) return o;
    const hspf_prefix_table tab = prefix_table(pfx_ptr, pfx_vertex, pfx_metric, flags);
    hspf_routes ro = o->raw();
    const int rc = hspf_routes_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, &tab, &ro);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_routes_device: ") + hspf_last_error(ctx_));
    return o;
  }
  std::unique_ptr<DeviceRoutes> routes_upload(const RoutesOut &t, uint32_t n_roots, uint32_t n_prefixes, uint32_t mask_words) override {
    auto o = std::make_unique<HipDeviceRoutes>(pool_);
    o->n_roots = n_roots; o->n_prefixes = n_prefixes; o->mask_words = mask_words;
    const size_t rp = (size_t)n_roots * n_prefixes;
    if (t.best_metric.size() != rp || t.best_entry.size() != rp || t.nexthop_mask.size() != rp * mask_words) throw std::runtime_error("routes_upload: table sizes");
    if (!o->alloc()) throw std::runtime_error("hipMalloc of the route tables failed");
    if (rp && (hipMemcpy(o->bm, t.best_metric.data(), rp * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(o->be, t.best_entry.data(), rp * 4, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(o->nm, t.nexthop_mask.data(), rp * 8 * mask_words, hipMemcpyHostToDevice) != hipSuccess))
      throw std::runtime_error("hipMemcpy of the route tables failed");
    return o;
  }
  std::unique_ptr<DeviceRoutes> rib_new(uint32_t n_prefixes, uint32_t mask_words) override {
    auto o = std::make_unique<HipDeviceRoutes>(pool_);
    o->n_roots = 1; o->n_prefixes = n_prefixes; o->mask_words = mask_words;
    o->alloc(); o->alloc_origin();
    const hspf_rib_device rib{n_prefixes, mask_words, o->bm, o->be, o->nm, o->org};
    const int rc = hspf_rib_clear_device(ctx_, &rib);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_rib_clear_device: ") + hspf_last_error(ctx_));
    return o;
  }
  void rib_fold(DeviceRoutes &rib_set, DeviceRun &run, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                const std::vector<uint32_t> &pfx_metric, const std::vector<uint32_t> &pfx_origin, const std::vector<uint32_t> &prefix_map,
                uint32_t area_index, uint32_t word_offset) override {
    auto &o = static_cast<HipDeviceRoutes &>(rib_set);
    auto &r = static_cast<HipDeviceRun &>(run);
    if (pfx_ptr.size() <= 1) return;
    const hspf_prefix_table tab = prefix_table(pfx_ptr, pfx_vertex, pfx_metric, HSPF_PFX_SATURATING | HSPF_PFX_ORDERED, &pfx_origin);
    const hspf_rib_device rib{o.n_prefixes, o.mask_words, o.bm, o.be, o.nm, o.org};
    const int rc = hspf_rib_fold_device(ctx_, r.n_vertices, r.mask_words, r.dist, r.flags, r.mask, &tab, prefix_map.data(), area_index, word_offset, &rib);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_rib_fold_device: ") + hspf_last_error(ctx_));
  }
  RouteRecords routes_changed(DeviceRoutes &old_set, DeviceRoutes &new_set) override {
    auto &a = static_cast<HipDeviceRoutes &>(old_set);
    auto &b = static_cast<HipDeviceRoutes &>(new_set);
    if (a.n_roots != b.n_roots || a.n_prefixes != b.n_prefixes || a.mask_words != b.mask_words) throw std::runtime_error("routes_changed: the two sets differ in shape");
    RouteRecords out;
    out.mask_words = b.mask_words;
    const size_t rp = (size_t)b.n_roots * b.n_prefixes;
    if (rp == 0) return out;
    // scratch of the comparison (action bytes, changed list, per-root bounds): kept by the engine, grown on demand
    const size_t need = rp + rp * 4 + ((size_t)b.n_roots + 1) * 4 + 64;
    if (diff_cap_ < need) {
      if (diff_) (void)hipFree(diff_);
      diff_ = nullptr; diff_cap_ = 0;
      if (hipMalloc(&diff_, need) != hipSuccess) throw std::runtime_error("hipMalloc of the diff scratch failed");
      diff_cap_ = need;
    }
    DevCursor c(diff_);
    uint32_t *changed = c.take<uint32_t>(rp), *cptr = c.take<uint32_t>((size_t)b.n_roots + 1);
    uint8_t *action = c.take<uint8_t>(rp);
    hspf_routes ro = a.raw(), rn = b.raw();
    int rc = hspf_routes_diff_device(ctx_, b.n_roots, b.n_prefixes, b.mask_words, &ro, &rn, action, changed, cptr);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_routes_diff_device: ") + hspf_last_error(ctx_));
    const uint32_t k = hspf_routes_diff_count(ctx_);
    out.words.assign((size_t)k * out.stride(), 0u);
    if (k) {
      rc = hspf_routes_pack(ctx_, b.n_roots, b.n_prefixes, b.mask_words, &rn, action, changed, cptr, k, out.words.data());
      if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_routes_pack: ") + hspf_last_error(ctx_));
      out.old_words.assign(out.words.size(), 0u);                    // the same list packed from the old set: what the route was
      rc = hspf_routes_pack(ctx_, b.n_roots, b.n_prefixes, b.mask_words, &ro, action, changed, cptr, k, out.old_words.data());
      if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_routes_pack (old set): ") + hspf_last_error(ctx_));
    }
    return out;
  }
 private:
  // ---- what the fast-reroute calls below share ---------------------------------------------------------------------------
  [[noreturn]] void fail(const char *what) const { throw std::runtime_error(std::string(what) + hspf_last_error(ctx_)); }
  // the head of a result: per protected root over the vertices of a run, or over the prefixes of a routes set
  template <typename Out> static Out head(const std::vector<LfaProtect> &protect, const HipDeviceRun &r) {
    Out o;
    o.supported = true;
    o.n_protected = (uint32_t)protect.size(); o.n_vertices = r.n_vertices;
    return o;
  }
  template <typename Out> static Out head(const std::vector<LfaProtect> &protect, const HipDeviceRoutes &rt) {
    Out o;
    o.supported = true;
    o.n_protected = (uint32_t)protect.size(); o.n_prefixes = rt.n_prefixes;
    return o;
  }
  static void same_shape(const std::string &who, const HipDeviceRun &r, const HipDeviceRun &rr) {
    if (rr.n_vertices != r.n_vertices || rr.n_roots != r.n_roots) throw std::runtime_error(who + "the two runs differ in shape");
  }
  static void routes_of_run(const std::string &who, const HipDeviceRun &r, const HipDeviceRoutes &rt, const std::vector<uint32_t> &pfx_ptr,
                            const std::vector<uint32_t> &pfx_vertex, const std::vector<uint32_t> &pfx_metric) {
    if (pfx_ptr.size() != (size_t)rt.n_prefixes + 1 || pfx_vertex.size() != pfx_metric.size() || rt.mask_words != r.mask_words)
      throw std::runtime_error(who + "the routes are not of this run and prefix table");
  }
  // the hspf_lfa_protect / hspf_lfa_lan array of a call (and srlg_raw, below: the hspf_srlg array), the lengths held to the slot
  // arrays; lans: one per protected root, which the caller has checked
  static std::vector<hspf_lfa_protect> protect_raw(const std::string &who, const std::vector<LfaProtect> &protect) {
    std::vector<hspf_lfa_protect> out;
    for (const LfaProtect &p : protect) {
      if (p.nbr_row.size() != p.nbr.size() || p.cost.size() != p.nbr.size() || p.root_link.size() != p.nbr.size() || p.cflags.size() != p.nbr.size())
        throw std::runtime_error(who + "the slot arrays of a protected root differ in length");
      out.push_back(hspf_lfa_protect{p.root_vertex, p.root_row, (uint32_t)p.nbr.size(), p.nbr.data(), p.nbr_row.data(), p.cost.data(), p.root_link.data(), p.cflags.data()});
    }
    return out;
  }
  static std::vector<hspf_lfa_lan> lan_raw(const std::string &who, const std::vector<LfaProtect> &protect, const std::vector<LfaLan> &lans) {
    std::vector<hspf_lfa_lan> out;
    for (size_t i = 0; i < lans.size(); ++i) {
      const LfaLan &l = lans[i];
      if (l.lan.size() != protect[i].nbr.size() || l.lan_row.size() != protect[i].nbr.size()) throw std::runtime_error(who + "lan / lan_row differ in length from the slot arrays");
      out.push_back(hspf_lfa_lan{l.lan.data(), l.lan_row.data()});
    }
    return out;
  }
  // a prefix table from the caller's vectors; an empty one is stood in for by one zero, the C call wants non-NULL pointers
  static hspf_prefix_table prefix_table(const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex, const std::vector<uint32_t> &pfx_metric,
                                        uint32_t flags, const std::vector<uint32_t> *pfx_origin = nullptr) {
    static const uint32_t zero = 0;
    auto data = [](const std::vector<uint32_t> &v) { return v.empty() ? &zero : v.data(); };
    return hspf_prefix_table{(uint32_t)pfx_ptr.size() - 1, (uint32_t)pfx_vertex.size(), pfx_ptr.data(), data(pfx_vertex), data(pfx_metric), flags,
                             pfx_origin ? data(*pfx_origin) : nullptr, nullptr, nullptr, nullptr};
  }
  // ... given AGAIN to a backup call, which reads the advertisers from it: nothing of it is resident for that call
  static hspf_prefix_table given_table(const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex, const std::vector<uint32_t> &pfx_metric,
                                       uint32_t table_flags) {
    return prefix_table(pfx_ptr, pfx_vertex, pfx_metric, table_flags & ~HSPF_PFX_RESIDENT);
  }
  // the alt_flags of lfa() for the same protect list, where given: pn bytes at the end of the call's block
  static bool has_alt(const LfaOut *lfa, size_t pn) { return lfa && lfa->supported && lfa->alt_flags.size() == pn; }
  static uint8_t *put_alt(DevCursor &c, const LfaOut *lfa, size_t pn) { return has_alt(lfa, pn) ? c.put(lfa->alt_flags) : nullptr; }
  // the per-slot repairs of tilfa() a backup call falls back on (with_links: ti_p and ti_link are read too), where given — those
  // of another protect list are an error: 9 bytes per slot of the call's block, 17 with the links, ti_kind behind the words
  static bool has_tilfa(const std::string &who, const TilfaOut *t, size_t ps, bool with_links) {
    if (!t || !t->supported) return false;
    if (t->ti_kind.size() != ps || t->ti_via.size() != ps || t->ti_metric.size() != ps || (with_links && (t->ti_p.size() != ps || t->ti_link.size() != ps)))
      throw std::runtime_error(who + "the TI-LFA result is not of this protect list");
    return true;
  }
  static hspf_tilfa_out put_tilfa(DevCursor &c, const TilfaOut &t, bool with_links) {
    hspf_tilfa_out ti{};
    ti.ti_via = c.put(t.ti_via); ti.ti_metric = c.put(t.ti_metric);
    if (with_links) { ti.ti_p = c.put(t.ti_p); ti.ti_link = c.put(t.ti_link); }
    ti.ti_kind = c.put(t.ti_kind);
    return ti;
  }
  // the rows a node-protecting call reads: the ascending union of the vertices the lists name — where they name none, one padding
  // row keeps the arguments of that call valid (true: it is padding) — and their dist on the forward graph
  static bool y_union(std::vector<uint32_t> &y, const std::vector<uint32_t> *a, const std::vector<uint32_t> *b = nullptr) {
    for (const std::vector<uint32_t> *l : {a, b})
      if (l) for (uint32_t v : *l) if (v != HSPF_NO_ROOT) y.push_back(v);
    std::sort(y.begin(), y.end());
    y.erase(std::unique(y.begin(), y.end()), y.end());
    const bool none = y.empty();
    if (none) y.push_back(HSPF_NO_ROOT);
    return none;
  }
  void y_run(Graph &gr, const std::vector<uint32_t> &y, bool none, uint32_t run_flags, uint32_t *ydist, const char *what) {
    if (none) return;
    hspf_result yres{ydist, nullptr, nullptr, nullptr, 1, nullptr};
    if (hspf_run_device(ctx_, static_cast<HipGraph &>(gr).g, y.data(), (uint32_t)y.size(), run_flags, &yres) != HSPF_OK) fail(what);
  }
  // the frame of rlfa() (lans == srlgs == nullptr: hspf_rlfa_device), rlfa_lan() (hspf_rlfa_lan_device) and rlfa_srlg()
  // (hspf_rlfa_srlg_device)
  RlfaOut rlfa_with(Graph &gr, DeviceRun &run, DeviceRun &reverse_run, const std::vector<LfaProtect> &protect, const std::vector<LfaLan> *lans,
                    const std::vector<Srlg> *srlgs, uint32_t lfa_flags, const LfaOut *lfa, bool with_spaces) {
    const uint32_t nw = lans ? HSPF_RLFA_LAN_COUNT_WORDS : srlgs ? HSPF_RLFA_SRLG_COUNT_WORDS : HSPF_RLFA_COUNT_WORDS;
    const uint32_t cw = lans ? HSPF_RLFA_LAN_COVERAGE_WORDS : srlgs ? HSPF_RLFA_SRLG_COVERAGE_WORDS : HSPF_RLFA_COVERAGE_WORDS;
    const char *fn = lans ? "hspf_rlfa_lan_device: " : srlgs ? "hspf_rlfa_srlg_device: " : "hspf_rlfa_device: ";
    const std::string who = lans ? "rlfa_lan: " : srlgs ? "rlfa_srlg: " : "rlfa: ";
    auto &r = static_cast<HipDeviceRun &>(run);
    auto &rr = static_cast<HipDeviceRun &>(reverse_run);
    same_shape(who, r, rr);
    RlfaOut o = head<RlfaOut>(protect, r);
    o.slot_stride = 64u * r.mask_words;
    if (protect.empty()) return o;
    const std::vector<hspf_lfa_protect> pr = protect_raw(who, protect);
    std::vector<hspf_lfa_lan> ls;
    if (lans) ls = lan_raw(who, protect, *lans);
    std::vector<hspf_srlg> ss;
    if (srlgs) ss = srlg_raw(who, protect, *srlgs);
    const size_t pn = (size_t)o.n_protected * o.n_vertices, ps = (size_t)o.n_protected * o.slot_stride, sp = with_spaces ? ps * o.n_vertices : 0;
    const size_t cb = (size_t)o.n_protected * cw;
    // one block: pq_node | pq_via | pq_metric | pq_counts | rl_node | rl_via | rl_coverage | space_via | space_flags | alt_flags
    HipLease blk(*pool_, (ps * (3 + nw) + pn * 2 + cb + sp) * 4 + sp + (has_alt(lfa, pn) ? pn : 0));
    DevCursor c(blk);
    hspf_rlfa_out out{};
    out.pq_node = c.take<uint32_t>(ps); out.pq_via = c.take<uint32_t>(ps); out.pq_metric = c.take<uint32_t>(ps); out.pq_counts = c.take<uint32_t>(ps * nw);
    out.rl_node = c.take<uint32_t>(pn); out.rl_via = c.take<uint32_t>(pn); out.rl_coverage = c.take<uint32_t>(cb);
    if (with_spaces) { out.space_via = c.take<uint32_t>(sp); out.space_flags = c.take<uint8_t>(sp); }
    const uint8_t *alt = put_alt(c, lfa, pn);
    hspf_graph *g = static_cast<HipGraph &>(gr).g;
    const int rc = !c.ok ? HSPF_E_HIP
                 : lans ? hspf_rlfa_lan_device(ctx_, g, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, rr.dist, pr.data(), ls.data(),
                                               o.n_protected, lfa_flags, alt, &out)
                 : srlgs ? hspf_rlfa_srlg_device(ctx_, g, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, rr.dist, pr.data(), ss.data(),
                                                 o.n_protected, lfa_flags, alt, &out)
                        : hspf_rlfa_device(ctx_, g, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, rr.dist, pr.data(), o.n_protected,
                                           lfa_flags, alt, &out);
    if (rc != HSPF_OK) fail(fn);
    c.fetch(o.pq_node, out.pq_node, ps); c.fetch(o.pq_via, out.pq_via, ps); c.fetch(o.pq_metric, out.pq_metric, ps); c.fetch(o.pq_counts, out.pq_counts, ps * nw);
    c.fetch(o.rl_node, out.rl_node, pn); c.fetch(o.rl_via, out.rl_via, pn); c.fetch(o.rl_coverage, out.rl_coverage, cb);
    if (with_spaces) { c.fetch(o.space_via, out.space_via, sp); c.fetch(o.space_flags, out.space_flags, sp); }
    if (!c.ok) fail(fn);
    return o;
  }
 public:
  // the hspf_srlg array of an SRLG call, its lengths held to the slot arrays
  static std::vector<hspf_srlg> srlg_raw(const std::string &who, const std::vector<LfaProtect> &protect, const std::vector<Srlg> &srlgs) {
    if (srlgs.size() != protect.size()) throw std::runtime_error(who + "one Srlg per protected root");
    std::vector<hspf_srlg> out;
    for (size_t i = 0; i < srlgs.size(); ++i) {
      const Srlg &m = srlgs[i];
      if (m.mem_ptr.size() != protect[i].nbr.size() + 1) throw std::runtime_error(who + "mem_ptr needs one entry per slot and one more");
      const size_t t = m.mem_ptr.back();
      if (m.tail.size() < t || m.pos.size() < t || m.head.size() < t || m.cost.size() < t || m.tail_row.size() < t || m.head_row.size() < t)
        throw std::runtime_error(who + "a member column is shorter than mem_ptr says");
      out.push_back(hspf_srlg{m.mem_ptr.data(), m.tail.data(), m.pos.data(), m.head.data(), m.cost.data(), m.tail_row.data(), m.head_row.data()});
    }
    return out;
  }
  // the frame of lfa() (lans == srlgs == nullptr: hspf_lfa_device), lfa_lan() (hspf_lfa_lan_device) and lfa_srlg() (hspf_lfa_srlg_device);
  // one pool request per array
  LfaOut lfa_with(DeviceRun &run, const std::vector<LfaProtect> &protect, const std::vector<LfaLan> *lans, const std::vector<Srlg> *srlgs,
                  uint32_t lfa_flags, bool with_masks) {
    auto &r = static_cast<HipDeviceRun &>(run);
    const uint32_t cw = lans ? HSPF_LFA_LAN_COVERAGE_WORDS : srlgs ? HSPF_LFA_SRLG_COVERAGE_WORDS : HSPF_LFA_COVERAGE_WORDS;
    const char *fn = lans ? "hspf_lfa_lan_device: " : srlgs ? "hspf_lfa_srlg_device: " : "hspf_lfa_device: ";
    LfaOut o = head<LfaOut>(protect, r);
    o.mask_words = r.mask_words;
    if (protect.empty()) return o;
    const std::vector<hspf_lfa_protect> ps = protect_raw("lfa: ", protect);
    std::vector<hspf_lfa_lan> ls;
    if (lans) ls = lan_raw("lfa_lan: ", protect, *lans);
    std::vector<hspf_srlg> ss;
    if (srlgs) ss = srlg_raw("lfa_srlg: ", protect, *srlgs);
    const size_t pn = (size_t)o.n_protected * o.n_vertices, pw = pn * o.mask_words, cb = (size_t)o.n_protected * cw;
    HipLease slot(*pool_, pn * 4), met(*pool_, pn * 4), cov(*pool_, cb * 4), fl(*pool_, pn), cm(*pool_, pw * 8, with_masks), nm(*pool_, pw * 8, with_masks);
    hspf_lfa_out out{slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cm.as<uint64_t>(), nm.as<uint64_t>(), cov.as<uint32_t>()};
    const int rc = lans ? hspf_lfa_lan_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, ps.data(), ls.data(), o.n_protected, lfa_flags, &out)
                 : srlgs ? hspf_lfa_srlg_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, ps.data(), ss.data(), o.n_protected, lfa_flags, &out)
                        : hspf_lfa_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, ps.data(), o.n_protected, lfa_flags, &out);
    if (rc != HSPF_OK) fail(fn);
    DevCursor c;
    c.fetch(o.alt_slot, out.alt_slot, pn); c.fetch(o.alt_metric, out.alt_metric, pn); c.fetch(o.alt_flags, out.alt_flags, pn); c.fetch(o.coverage, out.coverage, cb);
    if (with_masks) { c.fetch(o.cand_mask, out.cand_mask, pw); c.fetch(o.node_mask, out.node_mask, pw); }
    if (!c.ok) fail(fn);
    return o;
  }
  // the frame of backup_routes_ecmp() (srlgs nullptr) and backup_routes_ecmp_srlg().  Two calls: eb_ptr and the total, then the
  // entries into arrays of that size
  BackupEcmpOut backup_routes_ecmp_with(DeviceRun &run, DeviceRoutes &routes, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                                        const std::vector<uint32_t> &pfx_metric, uint32_t table_flags, const std::vector<LfaProtect> &protect,
                                        const std::vector<Srlg> *srlgs, uint32_t lfa_flags, const TilfaOut *tilfa) {
    auto &r = static_cast<HipDeviceRun &>(run);
    auto &rt = static_cast<HipDeviceRoutes &>(routes);
    BackupEcmpOut o = head<BackupEcmpOut>(protect, rt);
    if (protect.empty()) return o;
    routes_of_run("backup_routes_ecmp: ", r, rt, pfx_ptr, pfx_vertex, pfx_metric);
    const std::vector<hspf_lfa_protect> pr = protect_raw("backup_routes_ecmp: ", protect);
    std::vector<hspf_srlg> ss;
    if (srlgs) ss = srlg_raw("backup_routes_ecmp_srlg: ", protect, *srlgs);
    const size_t ps = (size_t)o.n_protected * 64u * r.mask_words;
    const bool with_links = srlgs != nullptr, with_ti = has_tilfa("backup_routes_ecmp: ", tilfa, ps, with_links);
    const size_t pb = (size_t)o.n_protected * o.n_prefixes + 1;
    const size_t cb = (size_t)o.n_protected * (srlgs ? HSPF_BK_ECMP_SRLG_COVERAGE_WORDS : HSPF_BK_ECMP_COVERAGE_WORDS);
    // one block: eb_ptr | eb_coverage | ti_via | ti_metric | (with groups: ti_p | ti_link |) ti_kind
    HipLease blk(*pool_, (pb + cb) * 4 + (with_ti ? ps * (with_links ? 17 : 9) : 0));
    DevCursor c(blk);
    hspf_backup_ecmp_out out{};
    out.eb_ptr = c.take<uint32_t>(pb);
    uint32_t *cov = c.take<uint32_t>(cb);
    hspf_tilfa_out ti{};
    if (with_ti) ti = put_tilfa(c, *tilfa, with_links);
    if (!c.ok) fail("hipMemcpy of the repairs: ");
    const char *what = srlgs ? "hspf_routes_backup_ecmp_srlg_device: " : "hspf_routes_backup_ecmp_device: ";
    const hspf_prefix_table tab = given_table(pfx_ptr, pfx_vertex, pfx_metric, table_flags);
    const hspf_routes ro = rt.raw();
    uint64_t total = 0;
    auto call = [&](uint64_t cap) {
      const int rc = srlgs ? hspf_routes_backup_ecmp_srlg_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), ss.data(), o.n_protected,
                                                                 lfa_flags, &tab, &ro, with_ti ? &ti : nullptr, cap, &out, &total)
                           : hspf_routes_backup_ecmp_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), o.n_protected, lfa_flags, &tab,
                                                            &ro, with_ti ? &ti : nullptr, cap, &out, &total);
      if (rc != HSPF_OK) fail(what);
    };
    call(0);
    const size_t t = (size_t)total;
    o.eb_coverage.assign(cb, 0u);
    if (t) {
      // the entries: eb_primary | eb_slot | eb_metric | eb_kind | eb_flags
      HipLease ent(*pool_, t * 14);
      DevCursor e(ent);
      out.eb_primary = e.take<uint32_t>(t); out.eb_slot = e.take<uint32_t>(t); out.eb_metric = e.take<uint32_t>(t); out.eb_kind = e.take<uint8_t>(t);
      out.eb_flags = e.take<uint8_t>(t); out.eb_coverage = cov;
      call(total);
      c.fetch(o.eb_primary, out.eb_primary, t); c.fetch(o.eb_slot, out.eb_slot, t); c.fetch(o.eb_metric, out.eb_metric, t); c.fetch(o.eb_kind, out.eb_kind, t);
      c.fetch(o.eb_flags, out.eb_flags, t); c.fetch(o.eb_coverage, out.eb_coverage, cb);
    }
    c.fetch(o.eb_ptr, out.eb_ptr, pb);
    if (!c.ok) fail(what);
    return o;
  }
  LfaOut lfa(DeviceRun &run, const std::vector<LfaProtect> &protect, uint32_t lfa_flags, bool with_masks) override {
    return lfa_with(run, protect, nullptr, nullptr, lfa_flags, with_masks);
  }
  // two calls: ea_ptr and the total, then the entries into arrays of that size; one pool request per array
  LfaEcmpOut lfa_ecmp(DeviceRun &run, const std::vector<LfaProtect> &protect, uint32_t lfa_flags) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    LfaEcmpOut o = head<LfaEcmpOut>(protect, r);
    if (protect.empty()) return o;
    const std::vector<hspf_lfa_protect> ps = protect_raw("lfa_ecmp: ", protect);
    const size_t pb = (size_t)o.n_protected * o.n_vertices + 1, cb = (size_t)o.n_protected * HSPF_LFA_ECMP_COVERAGE_WORDS;
    const char *what = "hspf_lfa_ecmp_device: ";
    HipLease ptr(*pool_, pb * 4);
    hspf_lfa_ecmp_out out{ptr.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t total = 0;
    if (hspf_lfa_ecmp_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, ps.data(), o.n_protected, lfa_flags, 0, &out, &total) != HSPF_OK) fail(what);
    const size_t t = (size_t)total;
    DevCursor c;
    o.ea_coverage.assign(cb, 0u);
    if (t) {
      HipLease pri(*pool_, t * 4), slot(*pool_, t * 4), met(*pool_, t * 4), cov(*pool_, cb * 4), fl(*pool_, t);
      out = hspf_lfa_ecmp_out{ptr.as<uint32_t>(), pri.as<uint32_t>(), slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cov.as<uint32_t>()};
      if (hspf_lfa_ecmp_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, ps.data(), o.n_protected, lfa_flags, total, &out, &total) != HSPF_OK)
        fail(what);
      c.fetch(o.ea_primary, out.ea_primary, t); c.fetch(o.ea_slot, out.ea_slot, t); c.fetch(o.ea_metric, out.ea_metric, t); c.fetch(o.ea_flags, out.ea_flags, t);
      c.fetch(o.ea_coverage, out.ea_coverage, cb);
    }
    c.fetch(o.ea_ptr, out.ea_ptr, pb);
    if (!c.ok) fail(what);
    return o;
  }
  // (backup_routes / backup_routes_lan stay the base's "not supported": a DeviceRoutes does not keep its prefix table, which
  // hspf_routes_backup_device needs; hspf::Engine::routes_backup_device / routes_backup_lan_device take it explicitly.)
  LfaOut lfa_lan(DeviceRun &run, const std::vector<LfaProtect> &protect, const std::vector<LfaLan> &lans, uint32_t lfa_flags, bool with_masks) override {
    if (lans.size() != protect.size()) throw std::runtime_error("lfa_lan: one LfaLan per protected root");
    return lfa_with(run, protect, &lans, nullptr, lfa_flags, with_masks);
  }
  LfaOut lfa_srlg(DeviceRun &run, const std::vector<LfaProtect> &protect, const std::vector<Srlg> &srlgs, uint32_t lfa_flags, bool with_masks) override {
    return lfa_with(run, protect, nullptr, &srlgs, lfa_flags, with_masks);
  }
  RlfaOut rlfa(Graph &gr, DeviceRun &run, DeviceRun &reverse_run, const std::vector<LfaProtect> &protect, uint32_t lfa_flags, const LfaOut *lfa,
               bool with_spaces) override {
    return rlfa_with(gr, run, reverse_run, protect, nullptr, nullptr, lfa_flags, lfa, with_spaces);
  }
  RlfaOut rlfa_lan(Graph &gr, DeviceRun &run, DeviceRun &reverse_run, const std::vector<LfaProtect> &protect, const std::vector<LfaLan> &lans,
                   uint32_t lfa_flags, const LfaOut *lfa, bool with_spaces) override {
    if (lans.size() != protect.size()) throw std::runtime_error("rlfa_lan: one LfaLan per protected root");
    return rlfa_with(gr, run, reverse_run, protect, &lans, nullptr, lfa_flags, lfa, with_spaces);
  }
  RlfaOut rlfa_srlg(Graph &gr, DeviceRun &run, DeviceRun &reverse_run, const std::vector<LfaProtect> &protect, const std::vector<Srlg> &srlgs,
                    uint32_t lfa_flags, const LfaOut *lfa, bool with_spaces) override {
    return rlfa_with(gr, run, reverse_run, protect, nullptr, &srlgs, lfa_flags, lfa, with_spaces);
  }
  TilfaOut tilfa(Graph &gr, DeviceRun &run, DeviceRun &reverse_run, const std::vector<LfaProtect> &protect, uint32_t lfa_flags, const LfaOut *lfa,
                 const RlfaOut &rl) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    auto &rr = static_cast<HipDeviceRun &>(reverse_run);
    same_shape("tilfa: ", r, rr);
    TilfaOut o = head<TilfaOut>(protect, r);
    o.slot_stride = 64u * r.mask_words;
    if (protect.empty()) return o;
    const size_t pn = (size_t)o.n_protected * o.n_vertices, ps = (size_t)o.n_protected * o.slot_stride, sp = ps * o.n_vertices;
    if (rl.space_flags.size() != sp || rl.space_via.size() != sp) throw std::runtime_error("tilfa: the RLFA result holds no space tables of this protect list");
    const std::vector<hspf_lfa_protect> pr = protect_raw("tilfa: ", protect);
    const size_t cb = (size_t)o.n_protected * HSPF_TILFA_COVERAGE_WORDS;
    // one block: ti_p | ti_q | ti_via | ti_link | ti_metric | ti_counts | td_coverage | space_via | ti_kind | td_kind | space_flags | alt_flags
    HipLease blk(*pool_, (ps * 5 + ps * HSPF_TILFA_COUNT_WORDS + cb + sp) * 4 + ps + pn + sp + (has_alt(lfa, pn) ? pn : 0));
    DevCursor c(blk);
    hspf_tilfa_out out{};
    out.ti_p = c.take<uint32_t>(ps); out.ti_q = c.take<uint32_t>(ps); out.ti_via = c.take<uint32_t>(ps); out.ti_link = c.take<uint32_t>(ps);
    out.ti_metric = c.take<uint32_t>(ps); out.ti_counts = c.take<uint32_t>(ps * HSPF_TILFA_COUNT_WORDS); out.td_coverage = c.take<uint32_t>(cb);
    const uint32_t *sv = c.put(rl.space_via);
    out.ti_kind = c.take<uint8_t>(ps); out.td_kind = c.take<uint8_t>(pn);
    const uint8_t *sf = c.put(rl.space_flags), *alt = put_alt(c, lfa, pn);
    const char *what = "hspf_tilfa_device: ";
    if (!c.ok || hspf_tilfa_device(ctx_, static_cast<HipGraph &>(gr).g, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, rr.dist, pr.data(), o.n_protected,
                                   lfa_flags, alt, sf, sv, &out) != HSPF_OK)
      fail(what);
    c.fetch(o.ti_kind, out.ti_kind, ps); c.fetch(o.ti_p, out.ti_p, ps); c.fetch(o.ti_q, out.ti_q, ps); c.fetch(o.ti_via, out.ti_via, ps);
    c.fetch(o.ti_link, out.ti_link, ps); c.fetch(o.ti_metric, out.ti_metric, ps); c.fetch(o.ti_counts, out.ti_counts, ps * HSPF_TILFA_COUNT_WORDS);
    c.fetch(o.td_kind, out.td_kind, pn); c.fetch(o.td_coverage, out.td_coverage, cb);
    if (!c.ok) fail(what);
    return o;
  }
  TilfaPcOut tilfa_pc(Graph &gr, DeviceRun &run, DeviceRun &reverse_run, const std::vector<LfaProtect> &protect, uint32_t lfa_flags, const LfaOut *lfa,
                      const RlfaOut &rl, const std::vector<uint32_t> &pc_dist, uint32_t n_pc_rows, const std::vector<uint32_t> &pc_row, uint32_t run_flags,
                      uint32_t max_walk) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    auto &rr = static_cast<HipDeviceRun &>(reverse_run);
    same_shape("tilfa_pc: ", r, rr);
    TilfaPcOut o = head<TilfaPcOut>(protect, r);
    if (protect.empty()) return o;
    const size_t pn = (size_t)o.n_protected * o.n_vertices, ps = (size_t)o.n_protected * 64u * r.mask_words, sp = ps * o.n_vertices, pcw = (size_t)n_pc_rows * o.n_vertices;
    if (rl.space_flags.size() != sp || rl.space_via.size() != sp) throw std::runtime_error("tilfa_pc: the RLFA result holds no space tables of this protect list");
    if (pc_row.size() != ps || pc_dist.size() != pcw) throw std::runtime_error("tilfa_pc: pc_row or pc_dist is not of this protect list");
    const std::vector<hspf_lfa_protect> pr = protect_raw("tilfa_pc: ", protect);
    const size_t cb = (size_t)o.n_protected * HSPF_TIPC_COVERAGE_WORDS, A = HSPF_TIPC_MAX_ADJ;
    // one block: tp_p | tp_via | tp_q | tp_metric | tp_hop_pos | tp_hop_head | tp_coverage | space_via | pc_dist | tp_kind | tp_n_adj | tp_flags | space_flags | alt_flags
    HipLease blk(*pool_, (pn * 4 + pn * A * 2 + cb + sp + std::max<size_t>(pcw, 1)) * 4 + pn * 3 + sp + (has_alt(lfa, pn) ? pn : 0));
    DevCursor c(blk);
    hspf_tilfa_pc_out out{};
    out.tp_p = c.take<uint32_t>(pn); out.tp_via = c.take<uint32_t>(pn); out.tp_q = c.take<uint32_t>(pn); out.tp_metric = c.take<uint32_t>(pn);
    out.tp_hop_pos = c.take<uint32_t>(pn * A); out.tp_hop_head = c.take<uint32_t>(pn * A); out.tp_coverage = c.take<uint32_t>(cb);
    const uint32_t *sv = c.put(rl.space_via);
    uint32_t *pcd = c.take<uint32_t>(std::max<size_t>(pcw, 1));
    c.upload(pcd, pc_dist);
    out.tp_kind = c.take<uint8_t>(pn); out.tp_n_adj = c.take<uint8_t>(pn); out.tp_flags = c.take<uint8_t>(pn);
    const uint8_t *sf = c.put(rl.space_flags), *alt = put_alt(c, lfa, pn);
    const char *what = "hspf_tilfa_pc_device: ";
    if (!c.ok || hspf_tilfa_pc_device(ctx_, static_cast<HipGraph &>(gr).g, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, rr.dist, pr.data(), o.n_protected,
                                      lfa_flags, alt, sf, sv, pcd, n_pc_rows, pc_row.data(), run_flags, max_walk, &out) != HSPF_OK)
      fail(what);
    c.fetch(o.tp_kind, out.tp_kind, pn); c.fetch(o.tp_n_adj, out.tp_n_adj, pn); c.fetch(o.tp_flags, out.tp_flags, pn); c.fetch(o.tp_p, out.tp_p, pn);
    c.fetch(o.tp_via, out.tp_via, pn); c.fetch(o.tp_q, out.tp_q, pn); c.fetch(o.tp_metric, out.tp_metric, pn); c.fetch(o.tp_hop_pos, out.tp_hop_pos, pn * A);
    c.fetch(o.tp_hop_head, out.tp_hop_head, pn * A); c.fetch(o.tp_coverage, out.tp_coverage, cb);
    if (!c.ok) fail(what);
    return o;
  }
  RlfaNodeOut rlfa_node(Graph &gr, DeviceRun &run, const std::vector<LfaProtect> &protect, uint32_t run_flags, uint32_t lfa_flags, const LfaOut *lfa,
                        const RlfaOut &rl, uint32_t max_pq) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    RlfaNodeOut o = head<RlfaNodeOut>(protect, r);
    o.slot_stride = 64u * r.mask_words; o.max_pq = max_pq;
    if (protect.empty()) return o;
    if (max_pq == 0 || max_pq > HSPF_RLFA_NODE_MAX_PQ) throw std::runtime_error("rlfa_node: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ");
    const size_t pn = (size_t)o.n_protected * o.n_vertices, ps = (size_t)o.n_protected * o.slot_stride, sp = ps * o.n_vertices, pm = ps * max_pq;
    if (rl.space_flags.size() != sp) throw std::runtime_error("rlfa_node: the RLFA result holds no space tables of this protect list");
    const std::vector<hspf_lfa_protect> pr = protect_raw("rlfa_node: ", protect);
    const size_t cb = (size_t)o.n_protected * HSPF_NP_COVERAGE_WORDS;
    // one block: nq_node | nq_via | nq_metric | nq_count | nd_node | nd_via | nd_metric | nd_set | nd_coverage | nd_kind | space_flags | alt_flags
    HipLease blk(*pool_, (pm * 3 + ps + pn * 4 + cb) * 4 + pn + sp + (has_alt(lfa, pn) ? pn : 0));
    DevCursor c(blk);
    hspf_rlfa_node_sel sel{};
    hspf_rlfa_node_out out{};
    sel.nq_node = c.take<uint32_t>(pm); sel.nq_via = c.take<uint32_t>(pm); sel.nq_metric = c.take<uint32_t>(pm); sel.nq_count = c.take<uint32_t>(ps);
    out.nd_node = c.take<uint32_t>(pn); out.nd_via = c.take<uint32_t>(pn); out.nd_metric = c.take<uint32_t>(pn); out.nd_set = c.take<uint32_t>(pn);
    out.nd_coverage = c.take<uint32_t>(cb);
    out.nd_kind = c.take<uint8_t>(pn);
    const uint8_t *sf = c.put(rl.space_flags), *alt = put_alt(c, lfa, pn);
    const char *what = "hspf_rlfa_node_select_device: ";
    if (!c.ok || hspf_rlfa_node_select_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), o.n_protected, lfa_flags, sf, max_pq,
                                              &sel) != HSPF_OK)
      fail(what);
    c.fetch(o.nq_node, sel.nq_node, pm); c.fetch(o.nq_via, sel.nq_via, pm); c.fetch(o.nq_metric, sel.nq_metric, pm); c.fetch(o.nq_count, sel.nq_count, ps);
    if (!c.ok) fail(what);
    const bool none = y_union(o.y_roots, &o.nq_node);
    HipLease ydist(*pool_, o.y_roots.size() * (size_t)o.n_vertices * 4);
    y_run(gr, o.y_roots, none, run_flags, ydist.as<uint32_t>(), "hspf_run_device (the PQ-node rows): ");
    what = "hspf_rlfa_node_device: ";
    if (hspf_rlfa_node_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), o.n_protected, ydist.as<uint32_t>(), o.y_roots.data(),
                              (uint32_t)o.y_roots.size(), &sel, max_pq, alt, &out) != HSPF_OK)
      fail(what);
    c.fetch(o.nd_kind, out.nd_kind, pn); c.fetch(o.nd_node, out.nd_node, pn); c.fetch(o.nd_via, out.nd_via, pn); c.fetch(o.nd_metric, out.nd_metric, pn);
    c.fetch(o.nd_set, out.nd_set, pn); c.fetch(o.nd_coverage, out.nd_coverage, cb);
    if (!c.ok) fail(what);
    return o;
  }
  TilfaNodeOut tilfa_node(Graph &gr, DeviceRun &run, const std::vector<LfaProtect> &protect, uint32_t run_flags, uint32_t lfa_flags, const LfaOut *lfa,
                          const RlfaOut &rl, const RlfaNodeOut *node, uint32_t max_pairs) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    TilfaNodeOut o = head<TilfaNodeOut>(protect, r);
    o.slot_stride = 64u * r.mask_words; o.max_pairs = max_pairs;
    if (protect.empty()) return o;
    if (max_pairs == 0 || max_pairs > HSPF_TILFA_NODE_MAX_PAIRS) throw std::runtime_error("tilfa_node: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS");
    const size_t pn = (size_t)o.n_protected * o.n_vertices, ps = (size_t)o.n_protected * o.slot_stride, sp = ps * o.n_vertices, pm = ps * max_pairs;
    if (rl.space_flags.size() != sp) throw std::runtime_error("tilfa_node: the RLFA result holds no space tables of this protect list");
    const std::vector<hspf_lfa_protect> pr = protect_raw("tilfa_node: ", protect);
    const size_t cb = (size_t)o.n_protected * HSPF_TN_COVERAGE_WORDS;
    const bool with_nd = node && node->supported && node->nd_kind.size() == pn;
    // one block: tq_q | tq_p | tq_link | tq_via | tq_metric | tq_count | tn_p | tn_q | tn_link | tn_via | tn_metric | tn_set | tn_coverage | tn_kind |
    // space_flags | alt_flags | nd_kind
    HipLease blk(*pool_, (pm * 5 + ps + pn * 6 + cb) * 4 + pn + sp + (has_alt(lfa, pn) ? pn : 0) + (with_nd ? pn : 0));
    DevCursor c(blk);
    hspf_tilfa_node_sel sel{};
    hspf_tilfa_node_out out{};
    sel.tq_q = c.take<uint32_t>(pm); sel.tq_p = c.take<uint32_t>(pm); sel.tq_link = c.take<uint32_t>(pm); sel.tq_via = c.take<uint32_t>(pm);
    sel.tq_metric = c.take<uint32_t>(pm); sel.tq_count = c.take<uint32_t>(ps);
    out.tn_p = c.take<uint32_t>(pn); out.tn_q = c.take<uint32_t>(pn); out.tn_link = c.take<uint32_t>(pn); out.tn_via = c.take<uint32_t>(pn);
    out.tn_metric = c.take<uint32_t>(pn); out.tn_set = c.take<uint32_t>(pn); out.tn_coverage = c.take<uint32_t>(cb);
    out.tn_kind = c.take<uint8_t>(pn);
    const uint8_t *sf = c.put(rl.space_flags), *alt = put_alt(c, lfa, pn), *ndk = with_nd ? c.put(node->nd_kind) : nullptr;
    const char *what = "hspf_tilfa_node_select_device: ";
    if (!c.ok || hspf_tilfa_node_select_device(ctx_, static_cast<HipGraph &>(gr).g, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(),
                                               o.n_protected, lfa_flags, sf, max_pairs, &sel) != HSPF_OK)
      fail(what);
    c.fetch(o.tq_q, sel.tq_q, pm); c.fetch(o.tq_p, sel.tq_p, pm); c.fetch(o.tq_link, sel.tq_link, pm); c.fetch(o.tq_via, sel.tq_via, pm);
    c.fetch(o.tq_metric, sel.tq_metric, pm); c.fetch(o.tq_count, sel.tq_count, ps);
    if (!c.ok) fail(what);
    const bool none = y_union(o.y_roots, &o.tq_q);
    HipLease ydist(*pool_, o.y_roots.size() * (size_t)o.n_vertices * 4);
    y_run(gr, o.y_roots, none, run_flags, ydist.as<uint32_t>(), "hspf_run_device (the q rows): ");
    what = "hspf_tilfa_node_device: ";
    if (hspf_tilfa_node_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), o.n_protected, ydist.as<uint32_t>(), o.y_roots.data(),
                               (uint32_t)o.y_roots.size(), &sel, max_pairs, alt, ndk, &out) != HSPF_OK)
      fail(what);
    c.fetch(o.tn_kind, out.tn_kind, pn); c.fetch(o.tn_p, out.tn_p, pn); c.fetch(o.tn_q, out.tn_q, pn); c.fetch(o.tn_link, out.tn_link, pn);
    c.fetch(o.tn_via, out.tn_via, pn); c.fetch(o.tn_metric, out.tn_metric, pn); c.fetch(o.tn_set, out.tn_set, pn); c.fetch(o.tn_coverage, out.tn_coverage, cb);
    if (!c.ok) fail(what);
    return o;
  }
  BackupOut backup_routes_srlg(DeviceRun &run, DeviceRoutes &routes, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                               const std::vector<uint32_t> &pfx_metric, uint32_t table_flags, const std::vector<LfaProtect> &protect,
                               const std::vector<Srlg> &srlgs, uint32_t lfa_flags, const TilfaOut *tilfa) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    auto &rt = static_cast<HipDeviceRoutes &>(routes);
    BackupOut o = head<BackupOut>(protect, rt);
    o.mask_words = r.mask_words;
    if (protect.empty()) return o;
    routes_of_run("backup_routes_srlg: ", r, rt, pfx_ptr, pfx_vertex, pfx_metric);
    const std::vector<hspf_lfa_protect> pr = protect_raw("backup_routes_srlg: ", protect);
    const std::vector<hspf_srlg> ss = srlg_raw("backup_routes_srlg: ", protect, srlgs);
    const size_t ps = (size_t)o.n_protected * 64u * r.mask_words, pp = (size_t)o.n_protected * o.n_prefixes, pw = pp * r.mask_words;
    const bool with_ti = has_tilfa("backup_routes_srlg: ", tilfa, ps, true);
    const size_t cb = (size_t)o.n_protected * HSPF_BK_SRLG_COVERAGE_WORDS;
    // one block: bk_cand_mask | bk_node_mask | bk_primary | bk_slot | bk_metric | bk_coverage | ti_via | ti_metric | ti_p | ti_link | ti_kind | bk_kind | bk_flags
    HipLease blk(*pool_, pw * 16 + pp * 12 + cb * 4 + (with_ti ? ps * 17 : 0) + pp * 2);
    DevCursor c(blk);
    hspf_backup_out out{};
    out.bk_cand_mask = c.take<uint64_t>(pw); out.bk_node_mask = c.take<uint64_t>(pw);
    out.bk_primary = c.take<uint32_t>(pp); out.bk_slot = c.take<uint32_t>(pp); out.bk_metric = c.take<uint32_t>(pp); out.bk_coverage = c.take<uint32_t>(cb);
    hspf_tilfa_out ti{};
    if (with_ti) ti = put_tilfa(c, *tilfa, true);
    out.bk_kind = c.take<uint8_t>(pp); out.bk_flags = c.take<uint8_t>(pp);
    if (!c.ok) fail("hipMemcpy of the repairs: ");
    const char *what = "hspf_routes_backup_srlg_device: ";
    const hspf_prefix_table tab = given_table(pfx_ptr, pfx_vertex, pfx_metric, table_flags);
    const hspf_routes ro = rt.raw();
    if (hspf_routes_backup_srlg_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), ss.data(), o.n_protected, lfa_flags, &tab, &ro,
                                       with_ti ? &ti : nullptr, &out) != HSPF_OK)
      fail(what);
    c.fetch(o.bk_kind, out.bk_kind, pp); c.fetch(o.bk_flags, out.bk_flags, pp); c.fetch(o.bk_primary, out.bk_primary, pp); c.fetch(o.bk_slot, out.bk_slot, pp);
    c.fetch(o.bk_metric, out.bk_metric, pp); c.fetch(o.bk_cand_mask, out.bk_cand_mask, pw); c.fetch(o.bk_node_mask, out.bk_node_mask, pw);
    c.fetch(o.bk_coverage, out.bk_coverage, cb);
    if (!c.ok) fail(what);
    return o;
  }
  BackupEcmpOut backup_routes_ecmp(DeviceRun &run, DeviceRoutes &routes, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                                   const std::vector<uint32_t> &pfx_metric, uint32_t table_flags, const std::vector<LfaProtect> &protect,
                                   uint32_t lfa_flags, const TilfaOut *tilfa) override {
    return backup_routes_ecmp_with(run, routes, pfx_ptr, pfx_vertex, pfx_metric, table_flags, protect, nullptr, lfa_flags, tilfa);
  }
  BackupEcmpOut backup_routes_ecmp_srlg(DeviceRun &run, DeviceRoutes &routes, const std::vector<uint32_t> &pfx_ptr, const std::vector<uint32_t> &pfx_vertex,
                                        const std::vector<uint32_t> &pfx_metric, uint32_t table_flags, const std::vector<LfaProtect> &protect,
                                        const std::vector<Srlg> &srlgs, uint32_t lfa_flags, const TilfaOut *tilfa) override {
    return backup_routes_ecmp_with(run, routes, pfx_ptr, pfx_vertex, pfx_metric, table_flags, protect, &srlgs, lfa_flags, tilfa);
  }
  BackupNodeOut backup_routes_node(Graph &gr, DeviceRun &run, DeviceRoutes &routes, const std::vector<uint32_t> &pfx_ptr,
                                   const std::vector<uint32_t> &pfx_vertex, const std::vector<uint32_t> &pfx_metric, uint32_t table_flags,
                                   const std::vector<LfaProtect> &protect, uint32_t run_flags, const RlfaNodeOut *node, const TilfaNodeOut *pairs,
                                   const BackupOut *backup) override {
    auto &r = static_cast<HipDeviceRun &>(run);
    auto &rt = static_cast<HipDeviceRoutes &>(routes);
    BackupNodeOut o = head<BackupNodeOut>(protect, rt);
    if (protect.empty()) return o;
    routes_of_run("backup_routes_node: ", r, rt, pfx_ptr, pfx_vertex, pfx_metric);
    const size_t ps = (size_t)o.n_protected * 64u * r.mask_words, pp = (size_t)o.n_protected * o.n_prefixes;
    const bool with_rn = node && node->supported, with_tn = pairs && pairs->supported, with_bk = backup && backup->supported;
    if (!with_rn && !with_tn) throw std::runtime_error("backup_routes_node: at least one of the two lists is required");
    const size_t pq = with_rn ? ps * node->max_pq : 0, pm = with_tn ? ps * pairs->max_pairs : 0;
    if (with_rn && (node->nq_count.size() != ps || node->nq_node.size() != pq || node->nq_via.size() != pq || node->nq_metric.size() != pq))
      throw std::runtime_error("backup_routes_node: the RLFA-node result is not of this protect list");
    if (with_tn && (pairs->tq_count.size() != ps || pairs->tq_q.size() != pm || pairs->tq_p.size() != pm || pairs->tq_link.size() != pm ||
                    pairs->tq_via.size() != pm || pairs->tq_metric.size() != pm))
      throw std::runtime_error("backup_routes_node: the TI-LFA-node result is not of this protect list");
    if (with_bk && (backup->bk_kind.size() != pp || backup->bk_flags.size() != pp))
      throw std::runtime_error("backup_routes_node: the backup result is not of this protect list and table");
    const std::vector<hspf_lfa_protect> pr = protect_raw("backup_routes_node: ", protect);
    const bool none = y_union(o.y_roots, with_rn ? &node->nq_node : nullptr, with_tn ? &pairs->tq_q : nullptr);
    const size_t cb = (size_t)o.n_protected * HSPF_BN_COVERAGE_WORDS, yw = o.y_roots.size() * (size_t)r.n_vertices;
    // one block: the lists (nq_node | nq_via | nq_metric | nq_count | tq_q | tq_p | tq_link | tq_via | tq_metric | tq_count) | bn_primary .. bn_set_pair |
    // bn_coverage | ydist | bn_kind | bk_kind | bk_flags
    HipLease blk(*pool_, (pq * 3 + (with_rn ? ps : 0) + pm * 5 + (with_tn ? ps : 0) + pp * 8 + cb + yw) * 4 + pp + (with_bk ? 2 * pp : 0));
    DevCursor c(blk);
    hspf_rlfa_node_sel rn{};
    hspf_tilfa_node_sel tn{};
    hspf_backup_node_out out{};
    if (with_rn) { rn.nq_node = c.put(node->nq_node); rn.nq_via = c.put(node->nq_via); rn.nq_metric = c.put(node->nq_metric); rn.nq_count = c.put(node->nq_count); }
    if (with_tn) {
      tn.tq_q = c.put(pairs->tq_q); tn.tq_p = c.put(pairs->tq_p); tn.tq_link = c.put(pairs->tq_link); tn.tq_via = c.put(pairs->tq_via);
      tn.tq_metric = c.put(pairs->tq_metric); tn.tq_count = c.put(pairs->tq_count);
    }
    out.bn_primary = c.take<uint32_t>(pp); out.bn_p = c.take<uint32_t>(pp); out.bn_q = c.take<uint32_t>(pp); out.bn_link = c.take<uint32_t>(pp);
    out.bn_via = c.take<uint32_t>(pp); out.bn_metric = c.take<uint32_t>(pp); out.bn_set_pq = c.take<uint32_t>(pp); out.bn_set_pair = c.take<uint32_t>(pp);
    out.bn_coverage = c.take<uint32_t>(cb);
    uint32_t *ydist = c.take<uint32_t>(yw);
    out.bn_kind = c.take<uint8_t>(pp);
    hspf_backup_out bk{};
    if (with_bk) { bk.bk_kind = c.put(backup->bk_kind); bk.bk_flags = c.put(backup->bk_flags); }
    if (!c.ok) fail("hipMemcpy of the lists: ");
    y_run(gr, o.y_roots, none, run_flags, ydist, "hspf_run_device (the rows of the listed nodes): ");
    const char *what = "hspf_routes_backup_node_device: ";
    const hspf_prefix_table tab = given_table(pfx_ptr, pfx_vertex, pfx_metric, table_flags);
    const hspf_routes ro = rt.raw();
    if (hspf_routes_backup_node_device(ctx_, r.n_vertices, r.n_roots, r.mask_words, r.dist, r.flags, r.mask, pr.data(), o.n_protected, &tab, &ro, ydist, o.y_roots.data(),
                                       (uint32_t)o.y_roots.size(), with_rn ? &rn : nullptr, with_rn ? node->max_pq : 0u, with_tn ? &tn : nullptr,
                                       with_tn ? pairs->max_pairs : 0u, with_bk ? &bk : nullptr, &out) != HSPF_OK)
      fail(what);
    c.fetch(o.bn_kind, out.bn_kind, pp); c.fetch(o.bn_primary, out.bn_primary, pp); c.fetch(o.bn_p, out.bn_p, pp); c.fetch(o.bn_q, out.bn_q, pp);
    c.fetch(o.bn_link, out.bn_link, pp); c.fetch(o.bn_via, out.bn_via, pp); c.fetch(o.bn_metric, out.bn_metric, pp); c.fetch(o.bn_set_pq, out.bn_set_pq, pp);
    c.fetch(o.bn_set_pair, out.bn_set_pair, pp); c.fetch(o.bn_coverage, out.bn_coverage, cb);
    if (!c.ok) fail(what);
    return o;
  }
  RouteEvents routes_events(DeviceRoutes &old_set, DeviceRoutes &new_set, bool with_silent) override {
    auto &a = static_cast<HipDeviceRoutes &>(old_set);
    auto &b = static_cast<HipDeviceRoutes &>(new_set);
    if (a.n_roots != b.n_roots || a.n_prefixes != b.n_prefixes || a.mask_words != b.mask_words) throw std::runtime_error("routes_events: the two sets differ in shape");
    RouteEvents out;
    out.supported = true;
    out.mask_words = b.mask_words;
    if ((size_t)b.n_roots * b.n_prefixes == 0) return out;
    const size_t stride = out.stride();
    auto grow = [&](size_t records) {                                // the page-locked record buffer: kept, grown on demand (contents carried over)
      void *p = nullptr;
      if (hspf_host_alloc(ctx_, records * stride * 4, &p) != HSPF_OK) throw std::runtime_error(std::string("hspf_host_alloc: ") + hspf_last_error(ctx_));
      if (ev_pin_) { memcpy(p, ev_pin_, std::min(ev_pin_bytes_, records * stride * 4)); hspf_host_free(ctx_, ev_pin_); }
      ev_pin_ = (uint32_t *)p; ev_pin_bytes_ = records * stride * 4;
    };
    if (ev_pin_bytes_ < 1024 * stride * 4) grow(1024);
    const uint32_t cap = (uint32_t)std::min<size_t>(ev_pin_bytes_ / (stride * 4), 0xFFFFFFFFu);
    hspf_routes ro = a.raw(), rn = b.raw();
    uint32_t total = 0;
    int rc = hspf_routes_events(ctx_, b.n_roots, b.n_prefixes, b.mask_words, &ro, &rn, with_silent ? HSPF_EV_SILENT : 0u, cap, ev_pin_, &total);
    if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_routes_events: ") + hspf_last_error(ctx_));
    if (total > cap) {
      grow((size_t)total + total / 4);
      rc = hspf_routes_events_rest(ctx_, cap, total - cap, ev_pin_ + (size_t)cap * stride);
      if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_routes_events_rest: ") + hspf_last_error(ctx_));
    }
    out.n = total; out.data = ev_pin_;
    return out;
  }
 private:
  uint32_t *ev_pin_ = nullptr;         // page-locked record buffer of routes_events
  size_t ev_pin_bytes_ = 0;
  void *diff_ = nullptr;
  size_t diff_cap_ = 0;
  template <typename WT>
  static void decode_row(const WT *w, const hspf_packed_layout &ly, uint16_t exact_flag, Tables &t, size_t o) {
    const WT nr = (WT)ly.not_reached, hm = (WT)ly.hops_mask, mm = (WT)((1ull << ly.mask_bits) - 1ull);
    const uint32_t ds = ly.dist_shift, hs = ly.hops_shift, n = t.n_vertices;
    uint32_t *d = t.dist.data() + o; uint16_t *h = t.hops.data() + o, *f = t.flags.data() + o; uint64_t *m = t.mask.data() + o;
    for (uint32_t v = 0; v < n; ++v) {
      const WT x = w[v];
      const bool in = x < nr;
      d[v] = in ? (uint32_t)(x >> ds) : 0xFFFFFFFFu;
      h[v] = in ? (uint16_t)((x >> hs) & hm) : (uint16_t)0;
      f[v] = in ? (uint16_t)(HSPF_RF_IN_SPT | exact_flag) : (uint16_t)0;
      m[v] = in ? (uint64_t)(x & mm) : 0ull;
    }
  }
  hspf_ctx *ctx_ = nullptr;
  void *pin_ = nullptr;
  size_t pin_cap_ = 0;
  std::shared_ptr<HipPool> pool_ = std::make_shared<HipPool>();      // (shared with the run / route objects: they may outlive the engine)
};

}  // namespace host
}  // namespace hspf
