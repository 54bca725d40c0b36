// holo_spf_hip.hpp — C++17 RAII convenience layer over the C ABI of include/holo_spf_hip.h.
//
// Header only, no dependency beyond the C header and the HIP runtime the caller already links for its
// device buffers.  It is the compiled-language twin of the safe Rust wrapper sketched in
// INTEGRATION.md §3 (Engine: Send, not Sync; Graph freed on drop; errors as codes, never exceptions
// across the boundary — this layer turns a non-zero code into hspf::Error for C++ callers).
#ifndef HOLO_SPF_HIP_HPP
#define HOLO_SPF_HIP_HPP

#include <cstdint>
#include <stdexcept>
#include <memory>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

#include "holo_spf_hip.h"

namespace hspf {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &what) : std::runtime_error(what + ": " + hspf_strerror(c)), code(c) {}
};

struct Tables {                       // row-major [root][vertex] host results of one run
  uint32_t n_roots = 0, n_vertices = 0, mask_words = 1;
  std::vector<uint32_t> dist, pop_rank;
  std::vector<uint16_t> hops, flags;
  std::vector<uint64_t> mask;
  hspf_stats stats{};
};

// Page-locked host memory from hspf_host_alloc (results cross the bus at full speed into it), freed with the object.
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  PinnedBuffer(hspf_ctx *ctx, size_t bytes) : ctx_(ctx), bytes_(bytes) {
    const int rc = hspf_host_alloc(ctx, bytes, &p_);
    if (rc != HSPF_OK) throw Error(rc, "hspf_host_alloc");
  }
  PinnedBuffer(PinnedBuffer &&o) noexcept : ctx_(o.ctx_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  PinnedBuffer &operator=(PinnedBuffer &&o) noexcept { if (this != &o) { reset(); ctx_ = o.ctx_; p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
  PinnedBuffer(const PinnedBuffer &) = delete;
  PinnedBuffer &operator=(const PinnedBuffer &) = delete;
  ~PinnedBuffer() { reset(); }
  void reset() { if (p_) hspf_host_free(ctx_, p_); p_ = nullptr; bytes_ = 0; }
  void *data() const { return p_; }
  size_t size() const { return bytes_; }
 private:
  hspf_ctx *ctx_ = nullptr;
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

// Packed results of one run (ABI 7): ONE word per (root, vertex) in a page-locked buffer + the run's field positions.
// A vertex is decoded where it is looked at (the rebuild of `Vertex{distance, hops, nexthops}` touches each once).
struct PackedTables {
  uint32_t n_roots = 0, n_vertices = 0;
  hspf_packed_layout layout{};
  PinnedBuffer words;
  std::vector<uint8_t> root_status;            // HSPF_ROOT_EXACT per root
  hspf_stats stats{};
  uint64_t word(uint32_t r, uint32_t v) const { return hspf_packed_word(&layout, words.data(), (size_t)r * n_vertices + v); }
  bool in_spt(uint32_t r, uint32_t v) const { return hspf_packed_in_spt(&layout, word(r, v)) != 0; }
  uint32_t dist(uint32_t r, uint32_t v) const { return hspf_packed_dist(&layout, word(r, v)); }
  uint16_t hops(uint32_t r, uint32_t v) const { return hspf_packed_hops(&layout, word(r, v)); }
  uint64_t mask(uint32_t r, uint32_t v) const { return hspf_packed_mask(&layout, word(r, v)); }
};

// Device memory from hspf_device_alloc (tables that stay in HBM between calls), freed with the object.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(hspf_ctx *ctx, size_t bytes) : ctx_(ctx), bytes_(bytes) {
    const int rc = hspf_device_alloc(ctx, bytes ? bytes : 8, &p_);
    if (rc != HSPF_OK) throw Error(rc, "hspf_device_alloc");
  }
  DeviceBuffer(DeviceBuffer &&o) noexcept : ctx_(o.ctx_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { if (this != &o) { reset(); ctx_ = o.ctx_; p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  ~DeviceBuffer() { reset(); }
  void reset() { if (p_) hspf_device_free(ctx_, p_); p_ = nullptr; bytes_ = 0; }
  template <typename T> T *as() const { return static_cast<T *>(p_); }
  size_t size() const { return bytes_; }
  template <typename T> std::vector<T> to_host(size_t count) const {
    std::vector<T> v(count);
    const int rc = count ? hspf_device_to_host(ctx_, v.data(), p_, count * sizeof(T)) : HSPF_OK;
    if (rc != HSPF_OK) throw Error(rc, "hspf_device_to_host");
    return v;
  }
 private:
  hspf_ctx *ctx_ = nullptr;
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

// Loop-free alternates (hspf_lfa_candidates / hspf_lfa_device): the candidate table of one root, one entry per first-hop
// slot, and the per-destination results of one protected root on the host.
struct LfaCandidates {
  uint32_t root = 0, total_slots = 0;
  std::vector<uint32_t> nbr, cost, root_link;
  std::vector<uint8_t> cflags;
};
struct Lfa {
  uint32_t n_vertices = 0, mask_words = 1;
  LfaCandidates candidates;
  std::vector<uint32_t> roots;                  // the SPF roots of the run behind it: [root] ++ its distinct neighbour routers
  std::vector<uint32_t> alt_slot, alt_metric;   // [n_vertices]
  std::vector<uint8_t> alt_flags;               // [n_vertices] HSPF_LFA_*
  std::vector<uint64_t> cand_mask, node_mask;   // [n_vertices][mask_words]
  uint32_t coverage[HSPF_LFA_COVERAGE_WORDS] = {};
};

// Per-primary alternates of the ECMP destinations (hspf_lfa_ecmp_device) of one protected root on the host: a stream in CSR form
// over the destinations, the entries of one destination in ascending primary slot order.
struct LfaEcmp {
  uint32_t n_vertices = 0;
  LfaCandidates candidates;
  std::vector<uint32_t> roots;                          // the SPF roots of the run behind it, as in Lfa
  std::vector<uint32_t> ea_ptr;                         // [n_vertices + 1]
  std::vector<uint32_t> ea_primary, ea_slot, ea_metric; // [ea_ptr.back()]
  std::vector<uint8_t> ea_flags;                        // HSPF_LFA_LINK_PROTECT | _NODE_PROTECT | _DOWNSTREAM | HSPF_LFA_EA_PRIMARY
  uint32_t ea_coverage[HSPF_LFA_ECMP_COVERAGE_WORDS] = {};
};

// Remote loop-free alternates (hspf_csr_transpose / hspf_rlfa_device) of one protected root on the host: the LFA result they
// complete, the PQ node of every slot, the remote alternate of every destination.
struct Rlfa {
  Lfa lfa;                                      // (cand_mask / node_mask are not fetched: empty)
  uint32_t slot_stride = 64;                    // 64 * mask_words
  std::vector<uint32_t> pq_node, pq_via, pq_metric;   // [slot_stride]
  std::vector<uint32_t> pq_counts;              // [slot_stride][HSPF_RLFA_COUNT_WORDS]
  std::vector<uint8_t> space_flags;             // [slot_stride][n_vertices] HSPF_RLFA_IN_* (empty unless asked for)
  std::vector<uint32_t> space_via;              // [slot_stride][n_vertices]
  std::vector<uint32_t> rl_node, rl_via;        // [n_vertices]
  uint32_t rl_coverage[HSPF_RLFA_COVERAGE_WORDS] = {};
};

// Two-segment repair paths (hspf_tilfa_device) of one protected root on the host: the RLFA result they complete (with its space
// tables), per slot the cheapest one- or two-segment repair, per destination its class.
struct Tilfa {
  Rlfa rlfa;
  std::vector<uint8_t> ti_kind;                 // [slot_stride] HSPF_TILFA_NONE / _NODE / _PAIR
  std::vector<uint32_t> ti_p, ti_q, ti_via, ti_link, ti_metric;   // [slot_stride]
  std::vector<uint32_t> ti_counts;              // [slot_stride][HSPF_TILFA_COUNT_WORDS]
  std::vector<uint8_t> td_kind;                 // [n_vertices] HSPF_TILFA_D_*
  uint32_t td_coverage[HSPF_TILFA_COVERAGE_WORDS] = {};
};

// Two-segment node-protecting repairs (hspf_tilfa_node_select_device / hspf_tilfa_node_device) of one protected root on the host:
// the RLFA result they complete (with its space tables), the node-protecting remote LFA in front of them (hspf_rlfa_node_*: its
// one-segment repairs stand), per slot the listed q's, per destination its class and repair.
struct TilfaNode {
  Rlfa rlfa;
  uint32_t max_pq = 0, max_pairs = 0;
  std::vector<uint32_t> nq_node, nq_via, nq_metric;       // [slot_stride][max_pq]
  std::vector<uint32_t> nq_count;                         // [slot_stride]
  std::vector<uint32_t> pq_roots;                         // the roots of the PQ-node rows: the ascending union of the nq lists
  std::vector<uint8_t> nd_kind;                           // [n_vertices] HSPF_NP_D_*
  std::vector<uint32_t> nd_node, nd_via, nd_metric;       // [n_vertices]
  uint32_t nd_coverage[HSPF_NP_COVERAGE_WORDS] = {};
  std::vector<uint32_t> tq_q, tq_p, tq_link, tq_via, tq_metric;   // [slot_stride][max_pairs]
  std::vector<uint32_t> tq_count;                         // [slot_stride]
  std::vector<uint32_t> y_roots;                          // the roots of the q rows: the ascending union of the tq lists
  std::vector<uint8_t> tn_kind;                           // [n_vertices] HSPF_TN_D_*
  std::vector<uint32_t> tn_p, tn_q, tn_link, tn_via, tn_metric, tn_set;   // [n_vertices]
  uint32_t tn_coverage[HSPF_TN_COVERAGE_WORDS] = {};
};

// Per-prefix backup routes (hspf_routes_device + hspf_routes_backup_device) of one protected root on the host: the route of every
// prefix, its backup (HSPF_BK_*), and the per-slot repairs bk_primary indexes (ti_* of `tilfa`: empty without `remote`).
struct BackupRoutes {
  Tilfa tilfa;                                  // (with remote; without it only tilfa.rlfa.lfa is filled)
  uint32_t n_prefixes = 0;
  std::vector<uint32_t> best_metric, best_entry;          // [n_prefixes]
  std::vector<uint64_t> nexthop_mask;                     // [n_prefixes][mask_words]
  std::vector<uint8_t> bk_kind, bk_flags;                 // [n_prefixes]
  std::vector<uint32_t> bk_primary, bk_slot, bk_metric;   // [n_prefixes]
  std::vector<uint64_t> bk_cand_mask, bk_node_mask;       // [n_prefixes][mask_words]
  uint32_t bk_coverage[HSPF_BK_COVERAGE_WORDS] = {};
  // backup_routes(..., ecmp = true): per primary of every HSPF_BK_ECMP prefix its backup (hspf_routes_backup_ecmp_device), a stream
  // in CSR form over the prefixes, the entries of one prefix in ascending primary slot order.  Empty otherwise.
  bool with_ecmp = false;
  std::vector<uint32_t> eb_ptr;                           // [n_prefixes + 1]
  std::vector<uint32_t> eb_primary, eb_slot, eb_metric;   // [eb_ptr.back()]
  std::vector<uint8_t> eb_kind, eb_flags;                 // HSPF_BK_LFA / _NODE / _PAIR / _NONE | HSPF_LFA_NODE_PROTECT | _DOWNSTREAM | HSPF_LFA_EA_PRIMARY
  uint32_t eb_coverage[HSPF_BK_ECMP_COVERAGE_WORDS] = {};
};

class Engine;

// The engine context, shared by the Engine and every Graph made from it: a Graph that outlives its Engine (members
// declared in the wrong order, a Graph moved out of the Engine's scope) keeps the context alive until it has freed its
// device arrays, instead of handing hspf_graph_free a dangling ctx.
struct CtxHolder {
  hspf_ctx *ctx = nullptr;
  CtxHolder() = default;
  CtxHolder(const CtxHolder &) = delete;
  CtxHolder &operator=(const CtxHolder &) = delete;
  ~CtxHolder() { if (ctx) hspf_shutdown(ctx); }
};

class Graph {
 public:
  Graph(Graph &&o) noexcept : holder_(std::move(o.holder_)), ctx_(o.ctx_), g_(o.g_) { o.g_ = nullptr; }
  Graph(const Graph &) = delete;
  Graph &operator=(const Graph &) = delete;
  ~Graph() { if (g_) hspf_graph_free(ctx_, g_); }
  uint32_t n_vertices() const { return hspf_graph_n_vertices(g_); }
  uint32_t n_links() const { return hspf_graph_n_edges(g_); }
  uint32_t n_links_kept() const { return hspf_graph_n_edges_kept(g_); }
  hspf_graph *raw() const { return g_; }

  // One re-originated / purged LSP or LSA = one replaced row (hspf_graph_patch).
  struct Row {
    uint32_t vertex;
    std::vector<uint32_t> col, metric;
    uint8_t vflags;
  };
  // Rows in any order; duplicates of a vertex are an error (HSPF_E_INVAL from the library).
  void patch(std::vector<Row> rows) {
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.vertex < b.vertex; });
    std::vector<uint32_t> vertex, row_ptr{0}, col, metric;
    std::vector<uint8_t> vflags;
    for (const Row &r : rows) {
      if (r.col.size() != r.metric.size()) throw Error(HSPF_E_INVAL, "Graph::patch: col/metric length mismatch");
      vertex.push_back(r.vertex);
      col.insert(col.end(), r.col.begin(), r.col.end());
      metric.insert(metric.end(), r.metric.begin(), r.metric.end());
      row_ptr.push_back((uint32_t)col.size());
      vflags.push_back(r.vflags);
    }
    if (col.empty()) { col.push_back(0); metric.push_back(0); }      // non-NULL pointers for an all-empty delta
    hspf_rows d{(uint32_t)vertex.size(), vertex.data(), row_ptr.data(), col.data(), metric.data(), vflags.data()};
    const int rc = hspf_graph_patch(ctx_, g_, &d);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_graph_patch (") + hspf_last_error(ctx_) + ")");
  }

 private:
  friend class Engine;
  Graph(std::shared_ptr<CtxHolder> h, hspf_graph *g) : holder_(std::move(h)), ctx_(holder_->ctx), g_(g) {}
  std::shared_ptr<CtxHolder> holder_;
  hspf_ctx *ctx_;
  hspf_graph *g_;
};

class Engine {
 public:
  explicit Engine(int device = 0) : holder_(std::make_shared<CtxHolder>()) {
    const int rc = hspf_init(device, &holder_->ctx);
    if (rc != HSPF_OK) throw Error(rc, "hspf_init");
    ctx_ = holder_->ctx;
  }
  Engine(const Engine &) = delete;
  Engine &operator=(const Engine &) = delete;
  ~Engine() = default;                               // the context goes with the last holder (this, or a surviving Graph)
  hspf_ctx *raw() const { return ctx_; }

  Graph upload(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col,
               const std::vector<uint32_t> &metric, const std::vector<uint8_t> &vflags, uint32_t max_path_metric) {
    hspf_csr csr{(uint32_t)vflags.size(), (uint32_t)col.size(), row_ptr.data(), col.data(), metric.data(), vflags.data(),
                 max_path_metric};
    hspf_graph *g = nullptr;
    const int rc = hspf_graph_upload(ctx_, &csr, &g);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_graph_upload (") + hspf_last_error(ctx_) + ")");
    return Graph(holder_, g);
  }

  uint32_t mask_words(const Graph &g, const std::vector<uint32_t> &roots) {
    uint32_t w = 1;
    const int rc = hspf_mask_words(ctx_, g.raw(), roots.data(), (uint32_t)roots.size(), &w);
    if (rc != HSPF_OK) throw Error(rc, "hspf_mask_words");
    return w;
  }

  // (H vertices, slot bases, total slots) of one root — see the header comment of hspf_result.
  std::pair<std::vector<uint32_t>, std::vector<uint32_t>> slot_table(const Graph &g, uint32_t root, uint32_t *total = nullptr) {
    uint32_t tot = 0;
    const int cnt = hspf_slot_table(ctx_, g.raw(), root, nullptr, nullptr, 0, &tot);
    if (cnt < 0) throw Error(cnt, "hspf_slot_table");
    std::vector<uint32_t> hv(cnt), hb(cnt);
    hspf_slot_table(ctx_, g.raw(), root, hv.data(), hb.data(), (uint32_t)cnt, &tot);
    if (total) *total = tot;
    return {hv, hb};
  }

  Tables run(const Graph &g, const std::vector<uint32_t> &roots, uint32_t run_flags = 0) {
    Tables t;
    t.n_roots = (uint32_t)roots.size();
    t.n_vertices = g.n_vertices();
    t.mask_words = mask_words(g, roots);
    const size_t rn = (size_t)t.n_roots * t.n_vertices;
    t.dist.resize(rn); t.hops.resize(rn); t.flags.resize(rn); t.mask.resize(rn * t.mask_words);
    if (run_flags & HSPF_RUN_POP_RANK) t.pop_rank.resize(rn);
    hspf_result out{t.dist.data(), t.hops.data(), t.flags.data(), t.mask.data(), t.mask_words,
                    t.pop_rank.empty() ? nullptr : t.pop_rank.data()};
    const int rc = hspf_run(ctx_, g.raw(), roots.data(), t.n_roots, run_flags, &out);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run (") + hspf_last_error(ctx_) + ")");
    hspf_get_stats(ctx_, &t.stats);
    return t;
  }

  // Failure scenarios: row r = the run of roots[r] with failures[r] applied (HSPF_FAIL_*), the graph untouched; everything else
  // as run().  run_failures_device writes to DEVICE pointers sized for roots.size() rows and returns the run's statistics.
  Tables run_failures(const Graph &g, const std::vector<uint32_t> &roots, const std::vector<hspf_failure> &failures, uint32_t run_flags = 0) {
    if (failures.size() != roots.size()) throw Error(HSPF_E_INVAL, "run_failures: one hspf_failure per root");
    Tables t;
    t.n_roots = (uint32_t)roots.size();
    t.n_vertices = g.n_vertices();
    t.mask_words = mask_words(g, roots);
    const size_t rn = (size_t)t.n_roots * t.n_vertices;
    t.dist.resize(rn); t.hops.resize(rn); t.flags.resize(rn); t.mask.resize(rn * t.mask_words);
    hspf_result out{t.dist.data(), t.hops.data(), t.flags.data(), t.mask.data(), t.mask_words, nullptr};
    const int rc = hspf_run_failures(ctx_, g.raw(), roots.data(), failures.data(), t.n_roots, run_flags, &out);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_failures (") + hspf_last_error(ctx_) + ")");
    hspf_get_stats(ctx_, &t.stats);
    return t;
  }
  hspf_stats run_failures_device(const Graph &g, const std::vector<uint32_t> &roots, const std::vector<hspf_failure> &failures, uint32_t run_flags,
                                 const hspf_result &out_device) {
    if (failures.size() != roots.size()) throw Error(HSPF_E_INVAL, "run_failures_device: one hspf_failure per root");
    hspf_result out = out_device;
    const int rc = hspf_run_failures_device(ctx_, g.raw(), roots.data(), failures.data(), (uint32_t)roots.size(), run_flags, &out);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_failures_device (") + hspf_last_error(ctx_) + ")");
    hspf_stats st{};
    hspf_get_stats(ctx_, &st);
    return st;
  }

  // ABI 7: packed results — a quarter of hspf_run's bytes over the bus.  `reuse`: a PackedTables of an earlier run whose
  // buffer is taken over when it is large enough.  Throws Error with code HSPF_E_NO_PACKED when the run's results do not
  // fit packed words (more than 24 first-hop slots): the caller then uses run().
  PackedTables run_packed(const Graph &g, const std::vector<uint32_t> &roots, uint32_t run_flags = 0, PackedTables *reuse = nullptr) {
    PackedTables t;
    t.n_roots = (uint32_t)roots.size();
    t.n_vertices = g.n_vertices();
    const size_t need = (size_t)8 * t.n_roots * t.n_vertices;
    if (reuse && reuse->words.size() >= need) t.words = std::move(reuse->words);
    else t.words = PinnedBuffer(ctx_, need);
    t.root_status.assign(t.n_roots, 0);
    const int rc = hspf_run_packed(ctx_, g.raw(), roots.data(), t.n_roots, run_flags, t.words.data(), t.words.size(), &t.layout, t.root_status.data());
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_packed (") + hspf_last_error(ctx_) + ")");
    hspf_get_stats(ctx_, &t.stats);
    return t;
  }

  // ABI 6: several runs in flight from one caller thread (one per area / level / neighbour set).  `out_device` holds
  // DEVICE pointers sized for roots.size() rows; they must stay valid, and unshared with other runs in flight, until
  // wait(ticket) has returned.  Results are bit-identical to hspf_run_device's.
  uint64_t run_device_async(const Graph &g, const std::vector<uint32_t> &roots, uint32_t run_flags, const hspf_result &out_device) {
    uint64_t ticket = 0;
    const int rc = hspf_run_device_async(ctx_, g.raw(), roots.data(), (uint32_t)roots.size(), run_flags, &out_device, &ticket);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_device_async (") + hspf_last_error(ctx_) + ")");
    return ticket;
  }
  hspf_stats wait(uint64_t ticket) {
    hspf_stats st{};
    const int rc = hspf_wait(ctx_, ticket, &st);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_wait (") + hspf_last_error(ctx_) + ")");
    return st;
  }
  // The route event stream (hspf_routes_events): every (root, prefix) pair of two DEVICE table sets whose action is not
  // SAME, SILENT pairs included when asked for, as paired old -> new records of HSPF_EVENT_REC_WORDS + 4 * n_mask_words words.
  // `records` is resized to the whole stream (a stream longer than its capacity on entry is completed with
  // hspf_routes_events_rest); pass the same vector again and the steady state is one device call.
  uint32_t routes_events(uint32_t n_roots, uint32_t n_prefixes, uint32_t n_mask_words, const hspf_routes &old_dev, const hspf_routes &new_dev,
                         bool with_silent, std::vector<uint32_t> &records) {
    const size_t stride = HSPF_EVENT_REC_WORDS + 4u * (size_t)n_mask_words;
    if (records.size() < 1024u * stride) records.resize(1024u * stride);
    const uint32_t cap = (uint32_t)std::min<size_t>(records.size() / stride, 0xFFFFFFFFu);
    uint32_t total = 0;
    int rc = hspf_routes_events(ctx_, n_roots, n_prefixes, n_mask_words, &old_dev, &new_dev, with_silent ? HSPF_EV_SILENT : 0u, cap, records.data(), &total);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_events (") + hspf_last_error(ctx_) + ")");
    records.resize((size_t)total * stride);
    if (total > cap && (rc = hspf_routes_events_rest(ctx_, cap, total - cap, records.data() + (size_t)cap * stride)) != HSPF_OK)
      throw Error(rc, std::string("hspf_routes_events_rest (") + hspf_last_error(ctx_) + ")");
    return total;
  }
  // Loop-free alternates (RFC 5286).  lfa_candidates: host arithmetic on the caller's CSR, no device.
  static LfaCandidates lfa_candidates(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                                      const std::vector<uint8_t> &vflags, uint32_t root) {
    hspf_csr csr{(uint32_t)vflags.size(), (uint32_t)col.size(), row_ptr.data(), col.data(), metric.data(), vflags.data(), 0xFFFFFFFFu};
    LfaCandidates c;
    c.root = root;
    const int k = hspf_lfa_candidates(&csr, root, 0, nullptr, nullptr, nullptr, nullptr, &c.total_slots);
    if (k < 0) throw Error(k, "hspf_lfa_candidates");
    c.nbr.resize(k); c.cost.resize(k); c.root_link.resize(k); c.cflags.resize(k);
    hspf_lfa_candidates(&csr, root, (uint32_t)k, c.nbr.data(), c.cost.data(), c.root_link.data(), c.cflags.data(), nullptr);
    return c;
  }
  // hspf_lfa_device on DEVICE tables of a previous run (several protected roots may share them).
  void lfa_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                  const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, hspf_lfa_out out_dev) {
    const int rc = hspf_lfa_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                   lfa_flags, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_lfa_device (") + hspf_last_error(ctx_) + ")");
  }
  // Broadcast-link protection (RFC 5286 section 3.3).  lfa_lan_candidates: per slot the LAN behind its first link (host arithmetic);
  // lfa_lan_device: lfa_device with loop-freeness towards those pseudonodes; `lans[i]` belongs to `protect[i]`, coverage has
  // HSPF_LFA_LAN_COVERAGE_WORDS words per root.  (No start-to-finish chain here yet: Python's SpfContext.lfa(lan_protect=True) has one.)
  static std::vector<uint32_t> lfa_lan_candidates(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                                                  const std::vector<uint8_t> &vflags, uint32_t root) {
    hspf_csr csr{(uint32_t)vflags.size(), (uint32_t)col.size(), row_ptr.data(), col.data(), metric.data(), vflags.data(), 0xFFFFFFFFu};
    const int k = hspf_lfa_lan_candidates(&csr, root, 0, nullptr, nullptr);
    if (k < 0) throw Error(k, "hspf_lfa_lan_candidates");
    std::vector<uint32_t> lan((size_t)k);
    hspf_lfa_lan_candidates(&csr, root, (uint32_t)k, lan.data(), nullptr);
    return lan;
  }
  void lfa_lan_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                      const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_lfa_lan> &lans, uint32_t lfa_flags,
                      hspf_lfa_out out_dev) {
    if (lans.size() != protect.size()) throw Error(HSPF_E_INVAL, "lfa_lan_device: one hspf_lfa_lan per protected root");
    const int rc = hspf_lfa_lan_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), lans.data(),
                                       (uint32_t)protect.size(), lfa_flags, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_lfa_lan_device (") + hspf_last_error(ctx_) + ")");
  }
  // One root start to finish: candidates, ONE run for [root] ++ its distinct neighbour routers with the tables left in HBM,
  // the alternates evaluated there, the five arrays and the coverage on the host.  The four vectors must be the CSR `g` was
  // uploaded from (and patched to): the candidate table comes from them, the SPTs from `g`.  Only the vertex count can be
  // checked here (HSPF_E_INVAL); rows that differ give alternates of a graph that does not exist.
  Lfa lfa(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
          const std::vector<uint8_t> &vflags, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0) {
    if (vflags.size() != g.n_vertices() || row_ptr.size() != vflags.size() + 1 || col.size() != g.n_links() || metric.size() != col.size())
      throw Error(HSPF_E_INVAL, "Engine::lfa: the CSR is not the one the graph was uploaded from");
    Lfa r;
    r.candidates = lfa_candidates(row_ptr, col, metric, vflags, root);
    const LfaCandidates &c = r.candidates;
    std::vector<uint32_t> nbrs;
    for (uint32_t v : c.nbr) if (v != HSPF_NO_ROOT) nbrs.push_back(v);
    std::sort(nbrs.begin(), nbrs.end());
    nbrs.erase(std::unique(nbrs.begin(), nbrs.end()), nbrs.end());
    r.roots.push_back(root);
    r.roots.insert(r.roots.end(), nbrs.begin(), nbrs.end());
    std::vector<uint32_t> nbr_row(c.nbr.size(), 0u);
    for (size_t k = 0; k < c.nbr.size(); ++k)
      if (c.nbr[k] != HSPF_NO_ROOT) nbr_row[k] = 1u + (uint32_t)(std::lower_bound(nbrs.begin(), nbrs.end(), c.nbr[k]) - nbrs.begin());
    const uint32_t n = g.n_vertices(), R = (uint32_t)r.roots.size();
    const uint32_t W = std::max(mask_words(g, r.roots), ((uint32_t)c.nbr.size() + 63u) / 64u);
    r.n_vertices = n; r.mask_words = W;
    const size_t rn = (size_t)R * n;
    DeviceBuffer dist(ctx_, rn * 4), flags(ctx_, rn * 2), mask(ctx_, rn * 8 * W);
    DeviceBuffer slot(ctx_, (size_t)n * 4), met(ctx_, (size_t)n * 4), fl(ctx_, n), cm(ctx_, (size_t)n * 8 * W), nm(ctx_, (size_t)n * 8 * W),
        cov(ctx_, HSPF_LFA_COVERAGE_WORDS * 4);
    hspf_result out{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), W, nullptr};
    const int rc = hspf_run_device(ctx_, g.raw(), r.roots.data(), R, run_flags, &out);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_device (") + hspf_last_error(ctx_) + ")");
    const hspf_lfa_protect p{root, 0u, (uint32_t)c.nbr.size(), c.nbr.data(), nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()};
    lfa_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags,
               hspf_lfa_out{slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cm.as<uint64_t>(), nm.as<uint64_t>(), cov.as<uint32_t>()});
    r.alt_slot = slot.to_host<uint32_t>(n); r.alt_metric = met.to_host<uint32_t>(n); r.alt_flags = fl.to_host<uint8_t>(n);
    r.cand_mask = cm.to_host<uint64_t>((size_t)n * W); r.node_mask = nm.to_host<uint64_t>((size_t)n * W);
    const std::vector<uint32_t> cv = cov.to_host<uint32_t>(HSPF_LFA_COVERAGE_WORDS);
    std::copy(cv.begin(), cv.end(), r.coverage);
    return r;
  }
  // hspf_lfa_ecmp_device on DEVICE tables: per-primary alternates of the destinations with two or more primary slots.  Returns the
  // total number of entries; when it exceeds cap_entries only ea_ptr was written (repeat with larger arrays).
  uint64_t lfa_ecmp_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                           const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, uint64_t cap_entries,
                           hspf_lfa_ecmp_out out_dev) {
    uint64_t total = 0;
    const int rc = hspf_lfa_ecmp_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                        lfa_flags, cap_entries, &out_dev, &total);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_lfa_ecmp_device (") + hspf_last_error(ctx_) + ")");
    return total;
  }
  // One root start to finish, as lfa(): the same run, then hspf_lfa_ecmp_device twice — for ea_ptr and the total, then with arrays of
  // that size.  The four vectors must be the CSR `g` was uploaded from.
  LfaEcmp lfa_ecmp(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                   const std::vector<uint8_t> &vflags, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0) {
    if (vflags.size() != g.n_vertices() || row_ptr.size() != vflags.size() + 1 || col.size() != g.n_links() || metric.size() != col.size())
      throw Error(HSPF_E_INVAL, "Engine::lfa_ecmp: the CSR is not the one the graph was uploaded from");
    LfaEcmp r;
    r.candidates = lfa_candidates(row_ptr, col, metric, vflags, root);
    const LfaCandidates &c = r.candidates;
    std::vector<uint32_t> nbrs;
    for (uint32_t v : c.nbr) if (v != HSPF_NO_ROOT) nbrs.push_back(v);
    std::sort(nbrs.begin(), nbrs.end());
    nbrs.erase(std::unique(nbrs.begin(), nbrs.end()), nbrs.end());
    r.roots.push_back(root);
    r.roots.insert(r.roots.end(), nbrs.begin(), nbrs.end());
    std::vector<uint32_t> nbr_row(c.nbr.size(), 0u);
    for (size_t k = 0; k < c.nbr.size(); ++k)
      if (c.nbr[k] != HSPF_NO_ROOT) nbr_row[k] = 1u + (uint32_t)(std::lower_bound(nbrs.begin(), nbrs.end(), c.nbr[k]) - nbrs.begin());
    const uint32_t n = g.n_vertices(), R = (uint32_t)r.roots.size();
    const uint32_t W = std::max(mask_words(g, r.roots), ((uint32_t)c.nbr.size() + 63u) / 64u);
    r.n_vertices = n;
    const size_t rn = (size_t)R * n;
    DeviceBuffer dist(ctx_, rn * 4), flags(ctx_, rn * 2), mask(ctx_, rn * 8 * W), ptr(ctx_, ((size_t)n + 1) * 4);
    hspf_result out{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), W, nullptr};
    const int rc = hspf_run_device(ctx_, g.raw(), r.roots.data(), R, run_flags, &out);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_device (") + hspf_last_error(ctx_) + ")");
    const hspf_lfa_protect p{root, 0u, (uint32_t)c.nbr.size(), c.nbr.data(), nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()};
    const uint64_t total = lfa_ecmp_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, 0,
                                           hspf_lfa_ecmp_out{ptr.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr});
    if (total) {
      const size_t t = (size_t)total;
      DeviceBuffer pri(ctx_, t * 4), slot(ctx_, t * 4), met(ctx_, t * 4), fl(ctx_, t), cov(ctx_, HSPF_LFA_ECMP_COVERAGE_WORDS * 4);
      lfa_ecmp_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, total,
                      hspf_lfa_ecmp_out{ptr.as<uint32_t>(), pri.as<uint32_t>(), slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cov.as<uint32_t>()});
      r.ea_primary = pri.to_host<uint32_t>(t); r.ea_slot = slot.to_host<uint32_t>(t); r.ea_metric = met.to_host<uint32_t>(t);
      r.ea_flags = fl.to_host<uint8_t>(t);
      const std::vector<uint32_t> cv = cov.to_host<uint32_t>(HSPF_LFA_ECMP_COVERAGE_WORDS);
      std::copy(cv.begin(), cv.end(), r.ea_coverage);
    }
    r.ea_ptr = ptr.to_host<uint32_t>((size_t)n + 1);
    return r;
  }
  // Remote loop-free alternates (RFC 7490).  csr_transpose: host arithmetic, no device; of a run on the result only `dist`
  // has a meaning (the distance TO the root).
  struct Transposed { std::vector<uint32_t> row_ptr, col, metric; };
  static Transposed csr_transpose(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                                  const std::vector<uint8_t> &vflags) {
    hspf_csr csr{(uint32_t)vflags.size(), (uint32_t)col.size(), row_ptr.data(), col.data(), metric.data(), vflags.data(), 0xFFFFFFFFu};
    Transposed t;
    t.row_ptr.resize(vflags.size() + 1); t.col.resize(col.size()); t.metric.resize(col.size());
    const int rc = hspf_csr_transpose(&csr, t.row_ptr.data(), t.col.data(), t.metric.data());
    if (rc != HSPF_OK) throw Error(rc, "hspf_csr_transpose");
    return t;
  }
  // hspf_rlfa_device on DEVICE tables: the forward set and rdist_dev, the dist of the same roots on the transposed graph.
  void rlfa_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                   const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                   hspf_rlfa_out out_dev) {
    const int rc = hspf_rlfa_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                                    (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_rlfa_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_rlfa_lan_device: rlfa_device with P, extended P and Q loop-free towards the pseudonode of every slot's LAN.  `lans[i]`
  // belongs to `protect[i]`; both table sets come from the run [S] ++ neighbour routers ++ LANs, rdist_dev ALWAYS from the transposed
  // graph; pq_counts has HSPF_RLFA_LAN_COUNT_WORDS words per slot, rl_coverage HSPF_RLFA_LAN_COVERAGE_WORDS per root.
  void rlfa_lan_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                       const uint64_t *mask_dev, const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect,
                       const std::vector<hspf_lfa_lan> &lans, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev, hspf_rlfa_out out_dev) {
    if (lans.size() != protect.size()) throw Error(HSPF_E_INVAL, "rlfa_lan_device: one hspf_lfa_lan per protected root");
    const int rc = hspf_rlfa_lan_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                                        lans.data(), (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_rlfa_lan_device (") + hspf_last_error(ctx_) + ")");
  }
  // Shared-risk link groups.  srlg_members: host arithmetic, no device (hspf_srlg_members): per first-hop slot of `root` the other
  // links that share a group id with the link of the root's row the slot stands behind; tail_row / head_row are the caller's to fill.
  struct SrlgMembers {
    std::vector<uint32_t> mem_ptr, tail, pos, head, cost, tail_row, head_row;
    hspf_srlg raw() const { return hspf_srlg{mem_ptr.data(), tail.data(), pos.data(), head.data(), cost.data(), tail_row.data(), head_row.data()}; }
  };
  static SrlgMembers srlg_members(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                                  const std::vector<uint8_t> &vflags, uint32_t root, const std::vector<uint32_t> &grp_ptr,
                                  const std::vector<uint32_t> &grp) {
    if (grp_ptr.size() != col.size() + 1) throw Error(HSPF_E_INVAL, "srlg_members: grp_ptr needs one entry per link and one more");
    hspf_csr csr{(uint32_t)vflags.size(), (uint32_t)col.size(), row_ptr.data(), col.data(), metric.data(), vflags.data(), 0xFFFFFFFFu};
    uint32_t slots = 0, total = 0;
    int k = hspf_srlg_members(&csr, root, grp_ptr.data(), grp.data(), 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &slots, &total);
    if (k < 0) throw Error(k, "hspf_srlg_members");
    SrlgMembers m;
    m.mem_ptr.resize((size_t)k + 1); m.tail.resize(total); m.pos.resize(total); m.head.resize(total); m.cost.resize(total);
    k = hspf_srlg_members(&csr, root, grp_ptr.data(), grp.data(), (uint32_t)k, total, m.mem_ptr.data(), m.tail.data(), m.pos.data(), m.head.data(),
                          m.cost.data(), &slots, &total);
    if (k < 0) throw Error(k, "hspf_srlg_members");
    return m;
  }
  // hspf_lfa_srlg_device: lfa_device whose alternates neither start on nor cross a member of a primary's group.  `srlgs[i]` belongs
  // to `protect[i]`; coverage has HSPF_LFA_SRLG_COVERAGE_WORDS words per root.
  void lfa_srlg_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                       const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_srlg> &srlgs,
                       uint32_t lfa_flags, hspf_lfa_out out_dev) {
    if (srlgs.size() != protect.size()) throw Error(HSPF_E_INVAL, "lfa_srlg_device: one hspf_srlg per protected root");
    const int rc = hspf_lfa_srlg_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), srlgs.data(),
                                        (uint32_t)protect.size(), lfa_flags, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_lfa_srlg_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_rlfa_srlg_device: rlfa_device with P, extended P and Q narrowed by the members of every slot's group; both table sets come
  // from the run [S] ++ neighbour routers ++ member endpoints; pq_counts has HSPF_RLFA_SRLG_COUNT_WORDS words per slot, rl_coverage
  // HSPF_RLFA_SRLG_COVERAGE_WORDS per root.  The space tables feed tilfa_device unchanged.
  void rlfa_srlg_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                        const uint64_t *mask_dev, const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect,
                        const std::vector<hspf_srlg> &srlgs, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev, hspf_rlfa_out out_dev) {
    if (srlgs.size() != protect.size()) throw Error(HSPF_E_INVAL, "rlfa_srlg_device: one hspf_srlg per protected root");
    const int rc = hspf_rlfa_srlg_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                                         srlgs.data(), (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_rlfa_srlg_device (") + hspf_last_error(ctx_) + ")");
  }
  // One root start to finish, as lfa(): ONE run of [root] ++ its neighbour routers on `g` and one on the upload of its transpose
  // (skipped when `symmetric` says every link has its reverse at the same cost), hspf_lfa_device, hspf_rlfa_device, results on
  // the host.  The four vectors must be the CSR `g` was uploaded from, max_path_metric the one it was uploaded with.
  Rlfa rlfa(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
            const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0,
            bool symmetric = false, bool with_spaces = false) {
    return rlfa_impl(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric, with_spaces, nullptr, nullptr, nullptr);
  }
  // hspf_tilfa_device on DEVICE tables: those of rlfa_device plus the space tables it wrote (required); `g` is the FORWARD graph.
  void tilfa_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                    const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                    const uint8_t *space_flags_dev, const uint32_t *space_via_dev, hspf_tilfa_out out_dev) {
    const int rc = hspf_tilfa_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                                     (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, space_flags_dev, space_via_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_tilfa_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_tilfa_pc_device on DEVICE tables: those of tilfa_device, and pc_dist_dev [n_pc_rows][n_vertices] — the dist of a
  // run_failures_device on `g` — with pc_row [protect.size()][64 * n_mask_words] (host) naming each slot's row (HSPF_NO_ROOT: none).
  void tilfa_pc_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                       const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                       const uint8_t *space_flags_dev, const uint32_t *space_via_dev, const uint32_t *pc_dist_dev, uint32_t n_pc_rows,
                       const std::vector<uint32_t> &pc_row, uint32_t run_flags, uint32_t max_walk, hspf_tilfa_pc_out out_dev) {
    if (pc_row.size() != protect.size() * 64u * n_mask_words) throw Error(HSPF_E_INVAL, "tilfa_pc_device: pc_row holds 64 * n_mask_words entries per protected root");
    const int rc = hspf_tilfa_pc_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                                        (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, space_flags_dev, space_via_dev, pc_dist_dev, n_pc_rows,
                                        pc_row.data(), run_flags, max_walk, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_tilfa_pc_device (") + hspf_last_error(ctx_) + ")");
  }
  // One root start to finish: rlfa() with the space tables, everything kept on the device, then hspf_tilfa_device on the same rows.
  Tilfa tilfa(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
              const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0,
              bool symmetric = false) {
    Tilfa t;
    t.rlfa = rlfa_impl(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric, true, &t, nullptr, nullptr);
    return t;
  }
  // hspf_rlfa_node_select_device on DEVICE tables: the table set and protect list of lfa_device and the space_flags rlfa_device
  // wrote for them; the lists are [protect.size()][64 * n_mask_words][max_pq].
  void rlfa_node_select_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                               const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags,
                               const uint8_t *space_flags_dev, uint32_t max_pq, hspf_rlfa_node_sel out_dev) {
    const int rc = hspf_rlfa_node_select_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                                (uint32_t)protect.size(), lfa_flags, space_flags_dev, max_pq, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_rlfa_node_select_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_rlfa_node_device on DEVICE tables: ydist_dev is the dist of a forward run of y_roots (host list: the caller's choice among
  // the listed nodes), sel_dev what rlfa_node_select_device wrote with the same max_pq.
  void rlfa_node_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                        const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const uint32_t *ydist_dev,
                        const std::vector<uint32_t> &y_roots, const hspf_rlfa_node_sel &sel_dev, uint32_t max_pq, const uint8_t *alt_flags_in_dev,
                        hspf_rlfa_node_out out_dev) {
    const int rc = hspf_rlfa_node_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                         ydist_dev, y_roots.data(), (uint32_t)y_roots.size(), &sel_dev, max_pq, alt_flags_in_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_rlfa_node_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_tilfa_node_select_device on DEVICE tables: the table set and protect list of lfa_device, the FORWARD graph and the
  // space_flags rlfa_device wrote for them; the lists are [protect.size()][64 * n_mask_words][max_pairs].
  void tilfa_node_select_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags,
                                const uint8_t *space_flags_dev, uint32_t max_pairs, hspf_tilfa_node_sel out_dev) {
    const int rc = hspf_tilfa_node_select_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                                 (uint32_t)protect.size(), lfa_flags, space_flags_dev, max_pairs, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_tilfa_node_select_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_tilfa_node_device on DEVICE tables: ydist_dev is the dist of a forward run of y_roots (host list: the caller's choice among
  // the listed q's), sel_dev what tilfa_node_select_device wrote with the same max_pairs; nd_kind_in_dev: the nd_kind of
  // rlfa_node_device for the same protect list, or nullptr.
  void tilfa_node_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                         const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const uint32_t *ydist_dev,
                         const std::vector<uint32_t> &y_roots, const hspf_tilfa_node_sel &sel_dev, uint32_t max_pairs, const uint8_t *alt_flags_in_dev,
                         const uint8_t *nd_kind_in_dev, hspf_tilfa_node_out out_dev) {
    const int rc = hspf_tilfa_node_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                          ydist_dev, y_roots.data(), (uint32_t)y_roots.size(), &sel_dev, max_pairs, alt_flags_in_dev, nd_kind_in_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_tilfa_node_device (") + hspf_last_error(ctx_) + ")");
  }
  // One root start to finish: rlfa() with the space tables, everything kept on the device, then the node-protecting remote LFA
  // (select, ONE run over the union of the listed PQ nodes, evaluate) and the two-segment node-protecting repairs (select, ONE run
  // over the union of the listed q's, evaluate with the alt_flags of hspf_lfa_device and the nd_kind of hspf_rlfa_node_device) on
  // the same rows.
  TilfaNode tilfa_node(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                       const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0,
                       bool symmetric = false, uint32_t max_pq = 16, uint32_t max_pairs = 16) {
    if (max_pq == 0 || max_pq > HSPF_RLFA_NODE_MAX_PQ) throw Error(HSPF_E_INVAL, "Engine::tilfa_node: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ");
    if (max_pairs == 0 || max_pairs > HSPF_TILFA_NODE_MAX_PAIRS) throw Error(HSPF_E_INVAL, "Engine::tilfa_node: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS");
    TilfaNode t;
    t.max_pq = max_pq; t.max_pairs = max_pairs;
    t.rlfa = rlfa_impl(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric, true, nullptr, nullptr, nullptr, &t);
    return t;
  }
  // hspf_routes_backup_device on DEVICE tables: the table set and protect list of lfa_device, the HOST prefix table and the routes
  // hspf_routes_device wrote for it, optionally the per-slot arrays of tilfa_device (nullptr: no remote fallback).
  void routes_backup_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                            const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const hspf_prefix_table &table,
                            const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev, hspf_backup_out out_dev) {
    const int rc = hspf_routes_backup_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                             lfa_flags, &table, &routes_dev, tilfa_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_backup_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_routes_backup_ecmp_device on the same inputs: per primary of every prefix with two or more primary slots, its backup.
  // Returns the total number of entries; when it exceeds cap_entries only eb_ptr was written (repeat with larger arrays).
  uint64_t routes_backup_ecmp_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                     const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags,
                                     const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev, uint64_t cap_entries,
                                     hspf_backup_ecmp_out out_dev) {
    uint64_t total = 0;
    const int rc = hspf_routes_backup_ecmp_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                                  (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, cap_entries, &out_dev, &total);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_backup_ecmp_device (") + hspf_last_error(ctx_) + ")");
    return total;
  }
  // hspf_routes_backup_ecmp_srlg_device: routes_backup_ecmp_device whose alternate for a primary h neither starts on nor crosses, on
  // its way to the prefix, a member of h's OWN shared-risk group (`srlgs` as for lfa_srlg_device; HSPF_LFA_SRLG_SAFE_REPAIRS in
  // lfa_flags vouches for tilfa_dev, whose ti_p / ti_link are read too; eb_coverage has HSPF_BK_ECMP_SRLG_COVERAGE_WORDS words per root).
  uint64_t routes_backup_ecmp_srlg_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                          const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_srlg> &srlgs,
                                          uint32_t lfa_flags, const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev,
                                          uint64_t cap_entries, hspf_backup_ecmp_out out_dev) {
    if (srlgs.size() != protect.size()) throw Error(HSPF_E_INVAL, "routes_backup_ecmp_srlg_device: one hspf_srlg per protected root");
    uint64_t total = 0;
    const int rc = hspf_routes_backup_ecmp_srlg_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), srlgs.data(),
                                                       (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, cap_entries, &out_dev, &total);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_backup_ecmp_srlg_device (") + hspf_last_error(ctx_) + ")");
    return total;
  }
  // hspf_routes_backup_lan_device: the same with loop-freeness towards the pseudonodes of the primaries' LANs (`lans` as for
  // lfa_lan_device; bk_coverage has HSPF_BK_LAN_COVERAGE_WORDS words per root).
  void routes_backup_lan_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_lfa_lan> &lans,
                                uint32_t lfa_flags, const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev,
                                hspf_backup_out out_dev) {
    if (lans.size() != protect.size()) throw Error(HSPF_E_INVAL, "routes_backup_lan_device: one hspf_lfa_lan per protected root");
    const int rc = hspf_routes_backup_lan_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), lans.data(),
                                                 (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_backup_lan_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_routes_backup_srlg_device: routes_backup_device whose alternates neither start on nor cross, on their way to the prefix, a
  // member of a primary's shared-risk group (`srlgs` as for lfa_srlg_device; HSPF_LFA_SRLG_SAFE_REPAIRS in lfa_flags vouches for
  // tilfa_dev, whose ti_p / ti_link are read too; bk_coverage has HSPF_BK_SRLG_COVERAGE_WORDS words per root).
  void routes_backup_srlg_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                 const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_srlg> &srlgs,
                                 uint32_t lfa_flags, const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev,
                                 hspf_backup_out out_dev) {
    if (srlgs.size() != protect.size()) throw Error(HSPF_E_INVAL, "routes_backup_srlg_device: one hspf_srlg per protected root");
    const int rc = hspf_routes_backup_srlg_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), srlgs.data(),
                                                  (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_backup_srlg_device (") + hspf_last_error(ctx_) + ")");
  }
  // hspf_routes_backup_node_device on DEVICE tables: the table set and protect list of lfa_device, the HOST prefix table and the
  // routes hspf_routes_device wrote for it, ydist_dev the dist of a forward run of y_roots (host list: the caller's choice among the
  // listed nodes), rn_sel_dev / tn_sel_dev what the two select calls wrote with max_pq / max_pairs (nullptr: no such entries; at
  // least one), bk_in_dev what routes_backup_device wrote (nullptr: node-protecting alternates are not looked at).
  void routes_backup_node_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                 const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const hspf_prefix_table &table,
                                 const hspf_routes &routes_dev, const uint32_t *ydist_dev, const std::vector<uint32_t> &y_roots,
                                 const hspf_rlfa_node_sel *rn_sel_dev, uint32_t max_pq, const hspf_tilfa_node_sel *tn_sel_dev, uint32_t max_pairs,
                                 const hspf_backup_out *bk_in_dev, hspf_backup_node_out out_dev) {
    const int rc = hspf_routes_backup_node_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                                  (uint32_t)protect.size(), &table, &routes_dev, ydist_dev, y_roots.data(), (uint32_t)y_roots.size(),
                                                  rn_sel_dev, max_pq, tn_sel_dev, max_pairs, bk_in_dev, &out_dev);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_backup_node_device (") + hspf_last_error(ctx_) + ")");
  }
  // One root start to finish: the chain of tilfa() (of lfa() alone without `remote`), hspf_routes_device for the root's row and
  // hspf_routes_backup_device, everything kept on the device in between.  table_flags: HSPF_PFX_SATURATING / HSPF_PFX_LAST_MIN.
  // ecmp: hspf_routes_backup_ecmp_device runs twice behind it on the same tables (the sizing call, the filling call): eb_* are filled.
  BackupRoutes backup_routes(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                             const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, const std::vector<uint32_t> &pfx_ptr,
                             const std::vector<uint32_t> &pfx_vertex, const std::vector<uint32_t> &pfx_metric, uint32_t table_flags = 0,
                             uint32_t run_flags = 0, uint32_t lfa_flags = 0, bool symmetric = false, bool remote = true, bool ecmp = false) {
    if (pfx_ptr.empty() || pfx_vertex.size() != pfx_metric.size()) throw Error(HSPF_E_INVAL, "Engine::backup_routes: malformed prefix table");
    BackupRoutes b;
    b.with_ecmp = ecmp;
    b.n_prefixes = (uint32_t)pfx_ptr.size() - 1u;
    const hspf_prefix_table t{b.n_prefixes, (uint32_t)pfx_vertex.size(), pfx_ptr.data(), pfx_vertex.data(), pfx_metric.data(), table_flags & ~HSPF_PFX_RESIDENT,
                              nullptr, nullptr, nullptr, nullptr};
    b.tilfa.rlfa = rlfa_impl(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric || !remote, remote,
                             remote ? &b.tilfa : nullptr, &b, &t);
    return b;
  }
  void wait_all() { (void)hspf_wait_all(ctx_); }
  uint32_t async_lanes() const { return hspf_async_lanes(ctx_); }
  // true: these runs are too small to pay for a launch — the caller keeps its own CPU loop (hspf_recommend_cpu)
  static bool recommend_cpu(uint32_t n_vertices, uint32_t n_edges, uint32_t n_roots) {
    return hspf_recommend_cpu(n_vertices, n_edges, n_roots) != 0;
  }

 private:
  // rlfa(); with `ti` the two-segment step runs on the same device tables before anything is freed; with `bk` the routes of `table`
  // and their backups are derived there too (without `ti` the remote-LFA call is skipped: nothing reads it); with `tn` (and the
  // space tables) the two node-protecting pairs of calls run there, each with its own run over the union of its lists
  Rlfa rlfa_impl(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                 const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags, uint32_t lfa_flags,
                 bool symmetric, bool with_spaces, Tilfa *ti, BackupRoutes *bk, const hspf_prefix_table *table, TilfaNode *tn = nullptr) {
    if (vflags.size() != g.n_vertices() || row_ptr.size() != vflags.size() + 1 || col.size() != g.n_links() || metric.size() != col.size())
      throw Error(HSPF_E_INVAL, "Engine::rlfa: the CSR is not the one the graph was uploaded from");
    Rlfa r;
    r.lfa.candidates = lfa_candidates(row_ptr, col, metric, vflags, root);
    const LfaCandidates &c = r.lfa.candidates;
    std::vector<uint32_t> nbrs;
    for (uint32_t v : c.nbr) if (v != HSPF_NO_ROOT) nbrs.push_back(v);
    std::sort(nbrs.begin(), nbrs.end());
    nbrs.erase(std::unique(nbrs.begin(), nbrs.end()), nbrs.end());
    r.lfa.roots.push_back(root);
    r.lfa.roots.insert(r.lfa.roots.end(), nbrs.begin(), nbrs.end());
    std::vector<uint32_t> nbr_row(c.nbr.size(), 0u);
    for (size_t k = 0; k < c.nbr.size(); ++k)
      if (c.nbr[k] != HSPF_NO_ROOT) nbr_row[k] = 1u + (uint32_t)(std::lower_bound(nbrs.begin(), nbrs.end(), c.nbr[k]) - nbrs.begin());
    const uint32_t n = g.n_vertices(), R = (uint32_t)r.lfa.roots.size();
    const uint32_t W = std::max(mask_words(g, r.lfa.roots), ((uint32_t)c.nbr.size() + 63u) / 64u), S = 64u * W;
    r.lfa.n_vertices = n; r.lfa.mask_words = W; r.slot_stride = S;
    const size_t rn = (size_t)R * n, sn = with_spaces ? (size_t)S * n : 0;
    DeviceBuffer dist(ctx_, rn * 4), flags(ctx_, rn * 2), mask(ctx_, rn * 8 * W), rdist(ctx_, symmetric ? 0 : rn * 4);
    DeviceBuffer slot(ctx_, (size_t)n * 4), met(ctx_, (size_t)n * 4), fl(ctx_, n), cov(ctx_, HSPF_LFA_COVERAGE_WORDS * 4);
    DeviceBuffer pq_node(ctx_, S * 4), pq_via(ctx_, S * 4), pq_metric(ctx_, S * 4), pq_counts(ctx_, (size_t)S * 4 * HSPF_RLFA_COUNT_WORDS),
        sp_flags(ctx_, sn), sp_via(ctx_, sn * 4), rl_node(ctx_, (size_t)n * 4), rl_via(ctx_, (size_t)n * 4), rl_cov(ctx_, HSPF_RLFA_COVERAGE_WORDS * 4);
    hspf_result out{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), W, nullptr};
    int rc = hspf_run_device(ctx_, g.raw(), r.lfa.roots.data(), R, run_flags, &out);
    if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_device (") + hspf_last_error(ctx_) + ")");
    if (!symmetric) {
      const Transposed t = csr_transpose(row_ptr, col, metric, vflags);
      Graph gt = upload(t.row_ptr, t.col, t.metric, vflags, max_path_metric);
      hspf_result rout{rdist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr};
      rc = hspf_run_device(ctx_, gt.raw(), r.lfa.roots.data(), R, run_flags, &rout);
      if (rc != HSPF_OK) throw Error(rc, std::string("hspf_run_device on the transposed graph (") + hspf_last_error(ctx_) + ")");
    }
    const hspf_lfa_protect p{root, 0u, (uint32_t)c.nbr.size(), c.nbr.data(), nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()};
    lfa_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags,
               hspf_lfa_out{slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), nullptr, nullptr, cov.as<uint32_t>()});
    const bool remote = !bk || ti;
    if (remote)
    rlfa_device(g, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), symmetric ? dist.as<uint32_t>() : rdist.as<uint32_t>(), {p},
                lfa_flags, fl.as<uint8_t>(),
                hspf_rlfa_out{pq_node.as<uint32_t>(), pq_via.as<uint32_t>(), pq_metric.as<uint32_t>(), pq_counts.as<uint32_t>(),
                              with_spaces ? sp_flags.as<uint8_t>() : nullptr, with_spaces ? sp_via.as<uint32_t>() : nullptr, rl_node.as<uint32_t>(),
                              rl_via.as<uint32_t>(), rl_cov.as<uint32_t>()});
    r.lfa.alt_slot = slot.to_host<uint32_t>(n); r.lfa.alt_metric = met.to_host<uint32_t>(n); r.lfa.alt_flags = fl.to_host<uint8_t>(n);
    const std::vector<uint32_t> cv = cov.to_host<uint32_t>(HSPF_LFA_COVERAGE_WORDS);
    std::copy(cv.begin(), cv.end(), r.lfa.coverage);
    if (remote) {
    r.pq_node = pq_node.to_host<uint32_t>(S); r.pq_via = pq_via.to_host<uint32_t>(S); r.pq_metric = pq_metric.to_host<uint32_t>(S);
    r.pq_counts = pq_counts.to_host<uint32_t>((size_t)S * HSPF_RLFA_COUNT_WORDS);
    if (with_spaces) { r.space_flags = sp_flags.to_host<uint8_t>(sn); r.space_via = sp_via.to_host<uint32_t>(sn); }
    r.rl_node = rl_node.to_host<uint32_t>(n); r.rl_via = rl_via.to_host<uint32_t>(n);
    const std::vector<uint32_t> rc4 = rl_cov.to_host<uint32_t>(HSPF_RLFA_COVERAGE_WORDS);
    std::copy(rc4.begin(), rc4.end(), r.rl_coverage);
    }
    DeviceBuffer kind(ctx_, ti ? S : 0), tv(ctx_, ti ? S * 4 : 0), tm(ctx_, ti ? S * 4 : 0);
    if (ti) {
      DeviceBuffer tp(ctx_, S * 4), tq(ctx_, S * 4), tl(ctx_, S * 4),
          tc(ctx_, (size_t)S * 4 * HSPF_TILFA_COUNT_WORDS), dk(ctx_, n), dc(ctx_, HSPF_TILFA_COVERAGE_WORDS * 4);
      tilfa_device(g, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), symmetric ? dist.as<uint32_t>() : rdist.as<uint32_t>(), {p},
                   lfa_flags, fl.as<uint8_t>(), sp_flags.as<uint8_t>(), sp_via.as<uint32_t>(),
                   hspf_tilfa_out{kind.as<uint8_t>(), tp.as<uint32_t>(), tq.as<uint32_t>(), tv.as<uint32_t>(), tl.as<uint32_t>(), tm.as<uint32_t>(),
                                  tc.as<uint32_t>(), dk.as<uint8_t>(), dc.as<uint32_t>()});
      ti->ti_kind = kind.to_host<uint8_t>(S); ti->ti_p = tp.to_host<uint32_t>(S); ti->ti_q = tq.to_host<uint32_t>(S);
      ti->ti_via = tv.to_host<uint32_t>(S); ti->ti_link = tl.to_host<uint32_t>(S); ti->ti_metric = tm.to_host<uint32_t>(S);
      ti->ti_counts = tc.to_host<uint32_t>((size_t)S * HSPF_TILFA_COUNT_WORDS); ti->td_kind = dk.to_host<uint8_t>(n);
      const std::vector<uint32_t> c5 = dc.to_host<uint32_t>(HSPF_TILFA_COVERAGE_WORDS);
      std::copy(c5.begin(), c5.end(), ti->td_coverage);
    }
    if (tn) {
      // the ascending union of the vertices a select call listed, its rows (dist only) on the forward graph; one padding row keeps the
      // arguments of the evaluate call valid where no list holds a vertex
      auto rows_of = [&](const std::vector<uint32_t> &listed, std::vector<uint32_t> &y, DeviceBuffer &ydist) {
        for (uint32_t v : listed) if (v != HSPF_NO_ROOT) y.push_back(v);
        std::sort(y.begin(), y.end());
        y.erase(std::unique(y.begin(), y.end()), y.end());
        const bool none = y.empty();
        if (none) y.push_back(HSPF_NO_ROOT);
        ydist = DeviceBuffer(ctx_, y.size() * (size_t)n * 4);
        if (none) return;
        hspf_result yout{ydist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr};
        const int yrc = hspf_run_device(ctx_, g.raw(), y.data(), (uint32_t)y.size(), run_flags, &yout);
        if (yrc != HSPF_OK) throw Error(yrc, std::string("hspf_run_device over the listed vertices (") + hspf_last_error(ctx_) + ")");
      };
      const size_t SQ = (size_t)S * tn->max_pq, SP = (size_t)S * tn->max_pairs;
      DeviceBuffer qn(ctx_, SQ * 4), qv(ctx_, SQ * 4), qm(ctx_, SQ * 4), qc(ctx_, S * 4), ydn(ctx_, 0);
      const hspf_rlfa_node_sel nsel{qn.as<uint32_t>(), qv.as<uint32_t>(), qm.as<uint32_t>(), qc.as<uint32_t>()};
      rlfa_node_select_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, sp_flags.as<uint8_t>(), tn->max_pq, nsel);
      tn->nq_node = qn.to_host<uint32_t>(SQ); tn->nq_via = qv.to_host<uint32_t>(SQ); tn->nq_metric = qm.to_host<uint32_t>(SQ);
      tn->nq_count = qc.to_host<uint32_t>(S);
      rows_of(tn->nq_node, tn->pq_roots, ydn);
      DeviceBuffer dk(ctx_, n), dn(ctx_, (size_t)n * 4), dv(ctx_, (size_t)n * 4), dm(ctx_, (size_t)n * 4), dc(ctx_, HSPF_NP_COVERAGE_WORDS * 4);
      rlfa_node_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, ydn.as<uint32_t>(), tn->pq_roots, nsel, tn->max_pq,
                       fl.as<uint8_t>(), hspf_rlfa_node_out{dk.as<uint8_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(), dm.as<uint32_t>(), nullptr, dc.as<uint32_t>()});
      tn->nd_kind = dk.to_host<uint8_t>(n); tn->nd_node = dn.to_host<uint32_t>(n); tn->nd_via = dv.to_host<uint32_t>(n); tn->nd_metric = dm.to_host<uint32_t>(n);
      const std::vector<uint32_t> c5 = dc.to_host<uint32_t>(HSPF_NP_COVERAGE_WORDS);
      std::copy(c5.begin(), c5.end(), tn->nd_coverage);
      DeviceBuffer tq(ctx_, SP * 4), tp(ctx_, SP * 4), tl(ctx_, SP * 4), tvi(ctx_, SP * 4), tme(ctx_, SP * 4), tc(ctx_, S * 4), ydq(ctx_, 0);
      const hspf_tilfa_node_sel tsel{tq.as<uint32_t>(), tp.as<uint32_t>(), tl.as<uint32_t>(), tvi.as<uint32_t>(), tme.as<uint32_t>(), tc.as<uint32_t>()};
      tilfa_node_select_device(g, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, sp_flags.as<uint8_t>(), tn->max_pairs, tsel);
      tn->tq_q = tq.to_host<uint32_t>(SP); tn->tq_p = tp.to_host<uint32_t>(SP); tn->tq_link = tl.to_host<uint32_t>(SP);
      tn->tq_via = tvi.to_host<uint32_t>(SP); tn->tq_metric = tme.to_host<uint32_t>(SP); tn->tq_count = tc.to_host<uint32_t>(S);
      rows_of(tn->tq_q, tn->y_roots, ydq);
      DeviceBuffer ek(ctx_, n), ep(ctx_, (size_t)n * 4), eq(ctx_, (size_t)n * 4), el(ctx_, (size_t)n * 4), ev(ctx_, (size_t)n * 4), em(ctx_, (size_t)n * 4),
          es(ctx_, (size_t)n * 4), ec(ctx_, HSPF_TN_COVERAGE_WORDS * 4);
      tilfa_node_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, ydq.as<uint32_t>(), tn->y_roots, tsel, tn->max_pairs,
                        fl.as<uint8_t>(), dk.as<uint8_t>(),
                        hspf_tilfa_node_out{ek.as<uint8_t>(), ep.as<uint32_t>(), eq.as<uint32_t>(), el.as<uint32_t>(), ev.as<uint32_t>(), em.as<uint32_t>(),
                                            es.as<uint32_t>(), ec.as<uint32_t>()});
      tn->tn_kind = ek.to_host<uint8_t>(n); tn->tn_p = ep.to_host<uint32_t>(n); tn->tn_q = eq.to_host<uint32_t>(n); tn->tn_link = el.to_host<uint32_t>(n);
      tn->tn_via = ev.to_host<uint32_t>(n); tn->tn_metric = em.to_host<uint32_t>(n); tn->tn_set = es.to_host<uint32_t>(n);
      const std::vector<uint32_t> c6 = ec.to_host<uint32_t>(HSPF_TN_COVERAGE_WORDS);
      std::copy(c6.begin(), c6.end(), tn->tn_coverage);
    }
    if (bk) {
      const size_t np = table->n_prefixes, nz = std::max<size_t>(np, 1);
      DeviceBuffer bm(ctx_, nz * 4), be(ctx_, nz * 4), nh(ctx_, nz * 8 * W), kk(ctx_, nz), pp(ctx_, nz * 4), ss(ctx_, nz * 4), mm(ctx_, nz * 4), ff(ctx_, nz),
          cmk(ctx_, nz * 8 * W), nmk(ctx_, nz * 8 * W), cv7(ctx_, HSPF_BK_COVERAGE_WORDS * 4);
      hspf_routes ro{bm.as<uint32_t>(), be.as<uint32_t>(), nh.as<uint64_t>()};
      rc = hspf_routes_device(ctx_, n, 1, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), table, &ro);
      if (rc != HSPF_OK) throw Error(rc, std::string("hspf_routes_device (") + hspf_last_error(ctx_) + ")");
      hspf_prefix_table tr = *table;
      tr.flags |= HSPF_PFX_RESIDENT;                      // the arrays hspf_routes_device has just staged
      const hspf_tilfa_out tio{kind.as<uint8_t>(), nullptr, nullptr, tv.as<uint32_t>(), nullptr, tm.as<uint32_t>(), nullptr, nullptr, nullptr};
      routes_backup_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, tr, ro, ti ? &tio : nullptr,
                           hspf_backup_out{kk.as<uint8_t>(), pp.as<uint32_t>(), ss.as<uint32_t>(), mm.as<uint32_t>(), ff.as<uint8_t>(), cmk.as<uint64_t>(),
                                           nmk.as<uint64_t>(), cv7.as<uint32_t>()});
      bk->best_metric = bm.to_host<uint32_t>(np); bk->best_entry = be.to_host<uint32_t>(np); bk->nexthop_mask = nh.to_host<uint64_t>(np * W);
      bk->bk_kind = kk.to_host<uint8_t>(np); bk->bk_primary = pp.to_host<uint32_t>(np); bk->bk_slot = ss.to_host<uint32_t>(np);
      bk->bk_metric = mm.to_host<uint32_t>(np); bk->bk_flags = ff.to_host<uint8_t>(np);
      bk->bk_cand_mask = cmk.to_host<uint64_t>(np * W); bk->bk_node_mask = nmk.to_host<uint64_t>(np * W);
      const std::vector<uint32_t> c7 = cv7.to_host<uint32_t>(HSPF_BK_COVERAGE_WORDS);
      std::copy(c7.begin(), c7.end(), bk->bk_coverage);
      if (bk->with_ecmp) {
        DeviceBuffer ptr(ctx_, (np + 1) * 4);
        const uint64_t total = routes_backup_ecmp_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, tr, ro,
                                                         ti ? &tio : nullptr, 0, hspf_backup_ecmp_out{ptr.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
        if (total) {
          const size_t t = (size_t)total;
          DeviceBuffer pri(ctx_, t * 4), knd(ctx_, t), slot(ctx_, t * 4), met(ctx_, t * 4), efl(ctx_, t), cov(ctx_, HSPF_BK_ECMP_COVERAGE_WORDS * 4);
          routes_backup_ecmp_device(n, R, W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), {p}, lfa_flags, tr, ro, ti ? &tio : nullptr, total,
                                    hspf_backup_ecmp_out{ptr.as<uint32_t>(), pri.as<uint32_t>(), knd.as<uint8_t>(), slot.as<uint32_t>(), met.as<uint32_t>(),
                                                         efl.as<uint8_t>(), cov.as<uint32_t>()});
          bk->eb_primary = pri.to_host<uint32_t>(t); bk->eb_kind = knd.to_host<uint8_t>(t); bk->eb_slot = slot.to_host<uint32_t>(t);
          bk->eb_metric = met.to_host<uint32_t>(t); bk->eb_flags = efl.to_host<uint8_t>(t);
          const std::vector<uint32_t> c8 = cov.to_host<uint32_t>(HSPF_BK_ECMP_COVERAGE_WORDS);
          std::copy(c8.begin(), c8.end(), bk->eb_coverage);
        }
        bk->eb_ptr = ptr.to_host<uint32_t>(np + 1);
      }
    }
    return r;
  }
  std::shared_ptr<CtxHolder> holder_;
  hspf_ctx *ctx_ = nullptr;
};

}  // namespace hspf
#endif
