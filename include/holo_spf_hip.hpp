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
    check(hspf_graph_upload(ctx_, &csr, &g), "hspf_graph_upload");
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
    check(hspf_run(ctx_, g.raw(), roots.data(), t.n_roots, run_flags, &out), "hspf_run");
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
    check(hspf_run_failures(ctx_, g.raw(), roots.data(), failures.data(), t.n_roots, run_flags, &out), "hspf_run_failures");
    hspf_get_stats(ctx_, &t.stats);
    return t;
  }
  hspf_stats run_failures_device(const Graph &g, const std::vector<uint32_t> &roots, const std::vector<hspf_failure> &failures, uint32_t run_flags,
                                 const hspf_result &out_device) {
    if (failures.size() != roots.size()) throw Error(HSPF_E_INVAL, "run_failures_device: one hspf_failure per root");
    hspf_result out = out_device;
    check(hspf_run_failures_device(ctx_, g.raw(), roots.data(), failures.data(), (uint32_t)roots.size(), run_flags, &out), "hspf_run_failures_device");
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
    check(hspf_run_packed(ctx_, g.raw(), roots.data(), t.n_roots, run_flags, t.words.data(), t.words.size(), &t.layout, t.root_status.data()), "hspf_run_packed");
    hspf_get_stats(ctx_, &t.stats);
    return t;
  }

  // ABI 6: several runs in flight from one caller thread (one per area / level / neighbour set).  `out_device` holds
  // DEVICE pointers sized for roots.size() rows; they must stay valid, and unshared with other runs in flight, until
  // wait(ticket) has returned.  Results are bit-identical to hspf_run_device's.
  uint64_t run_device_async(const Graph &g, const std::vector<uint32_t> &roots, uint32_t run_flags, const hspf_result &out_device) {
    uint64_t ticket = 0;
    check(hspf_run_device_async(ctx_, g.raw(), roots.data(), (uint32_t)roots.size(), run_flags, &out_device, &ticket), "hspf_run_device_async");
    return ticket;
  }
  hspf_stats wait(uint64_t ticket) {
    hspf_stats st{};
    check(hspf_wait(ctx_, ticket, &st), "hspf_wait");
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
    check(hspf_routes_events(ctx_, n_roots, n_prefixes, n_mask_words, &old_dev, &new_dev, with_silent ? HSPF_EV_SILENT : 0u, cap, records.data(), &total), "hspf_routes_events");
    records.resize((size_t)total * stride);
    if (total > cap) check(hspf_routes_events_rest(ctx_, cap, total - cap, records.data() + (size_t)cap * stride), "hspf_routes_events_rest");
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
    check(hspf_lfa_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                          lfa_flags, &out_dev), "hspf_lfa_device");
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
    check(hspf_lfa_lan_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), lans.data(),
                              (uint32_t)protect.size(), lfa_flags, &out_dev), "hspf_lfa_lan_device");
  }
  // One root start to finish: candidates, ONE run for [root] ++ its distinct neighbour routers with the tables left in HBM,
  // the alternates evaluated there, the five arrays and the coverage on the host.  The four vectors must be the CSR `g` was
  // uploaded from (and patched to): the candidate table comes from them, the SPTs from `g`.  Only the vertex count can be
  // checked here (HSPF_E_INVAL); rows that differ give alternates of a graph that does not exist.
  Lfa lfa(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
          const std::vector<uint8_t> &vflags, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0) {
    Lfa r;
    Chain c = chain_head("Engine::lfa", g, row_ptr, col, metric, vflags, root, run_flags, lfa_flags, r.candidates, r.roots);
    lfa_step(c, r, true);
    return r;
  }
  // hspf_lfa_ecmp_device on DEVICE tables: per-primary alternates of the destinations with two or more primary slots.  Returns the
  // total number of entries; when it exceeds cap_entries only ea_ptr was written (repeat with larger arrays).
  uint64_t lfa_ecmp_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                           const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, uint64_t cap_entries,
                           hspf_lfa_ecmp_out out_dev) {
    uint64_t total = 0;
    check(hspf_lfa_ecmp_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                               lfa_flags, cap_entries, &out_dev, &total), "hspf_lfa_ecmp_device");
    return total;
  }
  // One root start to finish, as lfa(): the same run, then hspf_lfa_ecmp_device twice — for ea_ptr and the total, then with arrays of
  // that size.  The four vectors must be the CSR `g` was uploaded from.
  LfaEcmp lfa_ecmp(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                   const std::vector<uint8_t> &vflags, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0) {
    LfaEcmp r;
    const Chain c = chain_head("Engine::lfa_ecmp", g, row_ptr, col, metric, vflags, root, run_flags, lfa_flags, r.candidates, r.roots);
    const size_t n = c.n;
    r.n_vertices = c.n;
    DeviceBuffer ptr(ctx_, (n + 1) * 4);
    const uint64_t total = lfa_ecmp_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), c.protect(), lfa_flags, 0,
                                           hspf_lfa_ecmp_out{ptr.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr});
    if (total) {
      const size_t t = (size_t)total;
      DeviceBuffer pri(ctx_, t * 4), slot(ctx_, t * 4), met(ctx_, t * 4), fl(ctx_, t), cov(ctx_, HSPF_LFA_ECMP_COVERAGE_WORDS * 4);
      lfa_ecmp_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), c.protect(), lfa_flags, total,
                      hspf_lfa_ecmp_out{ptr.as<uint32_t>(), pri.as<uint32_t>(), slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cov.as<uint32_t>()});
      r.ea_primary = pri.to_host<uint32_t>(t); r.ea_slot = slot.to_host<uint32_t>(t); r.ea_metric = met.to_host<uint32_t>(t);
      r.ea_flags = fl.to_host<uint8_t>(t);
      words_to_host(cov, r.ea_coverage);
    }
    r.ea_ptr = ptr.to_host<uint32_t>(n + 1);
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
    check(hspf_rlfa_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                           (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, &out_dev), "hspf_rlfa_device");
  }
  // hspf_rlfa_lan_device: rlfa_device with P, extended P and Q loop-free towards the pseudonode of every slot's LAN.  `lans[i]`
  // belongs to `protect[i]`; both table sets come from the run [S] ++ neighbour routers ++ LANs, rdist_dev ALWAYS from the transposed
  // graph; pq_counts has HSPF_RLFA_LAN_COUNT_WORDS words per slot, rl_coverage HSPF_RLFA_LAN_COVERAGE_WORDS per root.
  void rlfa_lan_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                       const uint64_t *mask_dev, const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect,
                       const std::vector<hspf_lfa_lan> &lans, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev, hspf_rlfa_out out_dev) {
    if (lans.size() != protect.size()) throw Error(HSPF_E_INVAL, "rlfa_lan_device: one hspf_lfa_lan per protected root");
    check(hspf_rlfa_lan_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                               lans.data(), (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, &out_dev), "hspf_rlfa_lan_device");
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
    check(hspf_lfa_srlg_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), srlgs.data(),
                               (uint32_t)protect.size(), lfa_flags, &out_dev), "hspf_lfa_srlg_device");
  }
  // hspf_rlfa_srlg_device: rlfa_device with P, extended P and Q narrowed by the members of every slot's group; both table sets come
  // from the run [S] ++ neighbour routers ++ member endpoints; pq_counts has HSPF_RLFA_SRLG_COUNT_WORDS words per slot, rl_coverage
  // HSPF_RLFA_SRLG_COVERAGE_WORDS per root.  The space tables feed tilfa_device unchanged.
  void rlfa_srlg_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                        const uint64_t *mask_dev, const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect,
                        const std::vector<hspf_srlg> &srlgs, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev, hspf_rlfa_out out_dev) {
    if (srlgs.size() != protect.size()) throw Error(HSPF_E_INVAL, "rlfa_srlg_device: one hspf_srlg per protected root");
    check(hspf_rlfa_srlg_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                                srlgs.data(), (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, &out_dev), "hspf_rlfa_srlg_device");
  }
  // One root start to finish, as lfa(): ONE run of [root] ++ its neighbour routers on `g` and one on the upload of its transpose
  // (skipped when `symmetric` says every link has its reverse at the same cost), hspf_lfa_device, hspf_rlfa_device, results on
  // the host.  The four vectors must be the CSR `g` was uploaded from, max_path_metric the one it was uploaded with.
  Rlfa rlfa(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
            const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0,
            bool symmetric = false, bool with_spaces = false) {
    Rlfa r;
    Chain c = rlfa_head(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric, r);
    remote_step(c, r, with_spaces);
    return r;
  }
  // hspf_tilfa_device on DEVICE tables: those of rlfa_device plus the space tables it wrote (required); `g` is the FORWARD graph.
  void tilfa_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                    const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                    const uint8_t *space_flags_dev, const uint32_t *space_via_dev, hspf_tilfa_out out_dev) {
    check(hspf_tilfa_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                            (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, space_flags_dev, space_via_dev, &out_dev), "hspf_tilfa_device");
  }
  // hspf_tilfa_pc_device on DEVICE tables: those of tilfa_device, and pc_dist_dev [n_pc_rows][n_vertices] — the dist of a
  // run_failures_device on `g` — with pc_row [protect.size()][64 * n_mask_words] (host) naming each slot's row (HSPF_NO_ROOT: none).
  void tilfa_pc_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                       const uint32_t *rdist_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                       const uint8_t *space_flags_dev, const uint32_t *space_via_dev, const uint32_t *pc_dist_dev, uint32_t n_pc_rows,
                       const std::vector<uint32_t> &pc_row, uint32_t run_flags, uint32_t max_walk, hspf_tilfa_pc_out out_dev) {
    if (pc_row.size() != protect.size() * 64u * n_mask_words) throw Error(HSPF_E_INVAL, "tilfa_pc_device: pc_row holds 64 * n_mask_words entries per protected root");
    check(hspf_tilfa_pc_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, protect.data(),
                               (uint32_t)protect.size(), lfa_flags, alt_flags_in_dev, space_flags_dev, space_via_dev, pc_dist_dev, n_pc_rows,
                               pc_row.data(), run_flags, max_walk, &out_dev), "hspf_tilfa_pc_device");
  }
  // One root start to finish: rlfa() with the space tables, everything kept on the device, then hspf_tilfa_device on the same rows.
  Tilfa tilfa(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
              const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags = 0, uint32_t lfa_flags = 0,
              bool symmetric = false) {
    Tilfa t;
    Chain c = rlfa_head(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric, t.rlfa);
    remote_step(c, t.rlfa, true);
    two_segment_step(c, t);
    return t;
  }
  // hspf_rlfa_node_select_device on DEVICE tables: the table set and protect list of lfa_device and the space_flags rlfa_device
  // wrote for them; the lists are [protect.size()][64 * n_mask_words][max_pq].
  void rlfa_node_select_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                               const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags,
                               const uint8_t *space_flags_dev, uint32_t max_pq, hspf_rlfa_node_sel out_dev) {
    check(hspf_rlfa_node_select_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                       (uint32_t)protect.size(), lfa_flags, space_flags_dev, max_pq, &out_dev), "hspf_rlfa_node_select_device");
  }
  // hspf_rlfa_node_device on DEVICE tables: ydist_dev is the dist of a forward run of y_roots (host list: the caller's choice among
  // the listed nodes), sel_dev what rlfa_node_select_device wrote with the same max_pq.
  void rlfa_node_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                        const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const uint32_t *ydist_dev,
                        const std::vector<uint32_t> &y_roots, const hspf_rlfa_node_sel &sel_dev, uint32_t max_pq, const uint8_t *alt_flags_in_dev,
                        hspf_rlfa_node_out out_dev) {
    check(hspf_rlfa_node_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                ydist_dev, y_roots.data(), (uint32_t)y_roots.size(), &sel_dev, max_pq, alt_flags_in_dev, &out_dev), "hspf_rlfa_node_device");
  }
  // hspf_tilfa_node_select_device on DEVICE tables: the table set and protect list of lfa_device, the FORWARD graph and the
  // space_flags rlfa_device wrote for them; the lists are [protect.size()][64 * n_mask_words][max_pairs].
  void tilfa_node_select_device(const Graph &g, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags,
                                const uint8_t *space_flags_dev, uint32_t max_pairs, hspf_tilfa_node_sel out_dev) {
    check(hspf_tilfa_node_select_device(ctx_, g.raw(), g.n_vertices(), n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                        (uint32_t)protect.size(), lfa_flags, space_flags_dev, max_pairs, &out_dev), "hspf_tilfa_node_select_device");
  }
  // hspf_tilfa_node_device on DEVICE tables: ydist_dev is the dist of a forward run of y_roots (host list: the caller's choice among
  // the listed q's), sel_dev what tilfa_node_select_device wrote with the same max_pairs; nd_kind_in_dev: the nd_kind of
  // rlfa_node_device for the same protect list, or nullptr.
  void tilfa_node_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                         const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const uint32_t *ydist_dev,
                         const std::vector<uint32_t> &y_roots, const hspf_tilfa_node_sel &sel_dev, uint32_t max_pairs, const uint8_t *alt_flags_in_dev,
                         const uint8_t *nd_kind_in_dev, hspf_tilfa_node_out out_dev) {
    check(hspf_tilfa_node_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                 ydist_dev, y_roots.data(), (uint32_t)y_roots.size(), &sel_dev, max_pairs, alt_flags_in_dev, nd_kind_in_dev, &out_dev), "hspf_tilfa_node_device");
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
    Chain c = rlfa_head(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric, t.rlfa);
    remote_step(c, t.rlfa, true);
    node_steps(c, t);
    return t;
  }
  // hspf_routes_backup_device on DEVICE tables: the table set and protect list of lfa_device, the HOST prefix table and the routes
  // hspf_routes_device wrote for it, optionally the per-slot arrays of tilfa_device (nullptr: no remote fallback).
  void routes_backup_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                            const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags, const hspf_prefix_table &table,
                            const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev, hspf_backup_out out_dev) {
    check(hspf_routes_backup_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), (uint32_t)protect.size(),
                                    lfa_flags, &table, &routes_dev, tilfa_dev, &out_dev), "hspf_routes_backup_device");
  }
  // hspf_routes_backup_ecmp_device on the same inputs: per primary of every prefix with two or more primary slots, its backup.
  // Returns the total number of entries; when it exceeds cap_entries only eb_ptr was written (repeat with larger arrays).
  uint64_t routes_backup_ecmp_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                     const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, uint32_t lfa_flags,
                                     const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev, uint64_t cap_entries,
                                     hspf_backup_ecmp_out out_dev) {
    uint64_t total = 0;
    check(hspf_routes_backup_ecmp_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                         (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, cap_entries, &out_dev, &total), "hspf_routes_backup_ecmp_device");
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
    check(hspf_routes_backup_ecmp_srlg_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), srlgs.data(),
                                              (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, cap_entries, &out_dev, &total), "hspf_routes_backup_ecmp_srlg_device");
    return total;
  }
  // hspf_routes_backup_lan_device: the same with loop-freeness towards the pseudonodes of the primaries' LANs (`lans` as for
  // lfa_lan_device; bk_coverage has HSPF_BK_LAN_COVERAGE_WORDS words per root).
  void routes_backup_lan_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_lfa_lan> &lans,
                                uint32_t lfa_flags, const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev,
                                hspf_backup_out out_dev) {
    if (lans.size() != protect.size()) throw Error(HSPF_E_INVAL, "routes_backup_lan_device: one hspf_lfa_lan per protected root");
    check(hspf_routes_backup_lan_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), lans.data(),
                                        (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, &out_dev), "hspf_routes_backup_lan_device");
  }
  // hspf_routes_backup_srlg_device: routes_backup_device whose alternates neither start on nor cross, on their way to the prefix, a
  // member of a primary's shared-risk group (`srlgs` as for lfa_srlg_device; HSPF_LFA_SRLG_SAFE_REPAIRS in lfa_flags vouches for
  // tilfa_dev, whose ti_p / ti_link are read too; bk_coverage has HSPF_BK_SRLG_COVERAGE_WORDS words per root).
  void routes_backup_srlg_device(uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev, const uint16_t *flags_dev,
                                 const uint64_t *mask_dev, const std::vector<hspf_lfa_protect> &protect, const std::vector<hspf_srlg> &srlgs,
                                 uint32_t lfa_flags, const hspf_prefix_table &table, const hspf_routes &routes_dev, const hspf_tilfa_out *tilfa_dev,
                                 hspf_backup_out out_dev) {
    if (srlgs.size() != protect.size()) throw Error(HSPF_E_INVAL, "routes_backup_srlg_device: one hspf_srlg per protected root");
    check(hspf_routes_backup_srlg_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(), srlgs.data(),
                                         (uint32_t)protect.size(), lfa_flags, &table, &routes_dev, tilfa_dev, &out_dev), "hspf_routes_backup_srlg_device");
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
    check(hspf_routes_backup_node_device(ctx_, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, protect.data(),
                                         (uint32_t)protect.size(), &table, &routes_dev, ydist_dev, y_roots.data(), (uint32_t)y_roots.size(),
                                         rn_sel_dev, max_pq, tn_sel_dev, max_pairs, bk_in_dev, &out_dev), "hspf_routes_backup_node_device");
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
    // without `remote` nothing reads the remote LFA or the reverse run: both are skipped
    Chain c = rlfa_head(g, row_ptr, col, metric, vflags, max_path_metric, root, run_flags, lfa_flags, symmetric || !remote, b.tilfa.rlfa);
    if (remote) {
      remote_step(c, b.tilfa.rlfa, true);
      two_segment_step(c, b.tilfa);
    }
    backup_step(c, b, t);
    return b;
  }
  void wait_all() { (void)hspf_wait_all(ctx_); }
  uint32_t async_lanes() const { return hspf_async_lanes(ctx_); }
  // true: these runs are too small to pay for a launch — the caller keeps its own CPU loop (hspf_recommend_cpu)
  static bool recommend_cpu(uint32_t n_vertices, uint32_t n_edges, uint32_t n_roots) {
    return hspf_recommend_cpu(n_vertices, n_edges, n_roots) != 0;
  }

 private:
  void check(int rc, const char *call) const {
    if (rc != HSPF_OK) throw Error(rc, std::string(call) + " (" + hspf_last_error(ctx_) + ")");
  }
  template <size_t N> static void words_to_host(const DeviceBuffer &b, uint32_t (&dst)[N]) {      // a coverage array
    const std::vector<uint32_t> v = b.to_host<uint32_t>(N);
    std::copy(v.begin(), v.end(), dst);
  }
  // The device tables the steps of a one-root chain share.  The head fills the first line — the forward run of [root] ++ its
  // distinct neighbour routers, left in HBM — and the one protected root over it; every step leaves what a later one reads.
  struct Chain {
    const Graph *g = nullptr;
    const LfaCandidates *cand = nullptr;
    uint32_t n = 0, R = 0, W = 1, S = 64, run_flags = 0, lfa_flags = 0;
    std::vector<uint32_t> nbr_row;
    DeviceBuffer dist, flags, mask;     // chain_head
    DeviceBuffer rdist;                 // rlfa_head: the dist of the same roots on the transposed graph (not read where the costs are symmetric)
    DeviceBuffer alt_flags;             // lfa_step
    DeviceBuffer sp_flags, sp_via;      // remote_step
    DeviceBuffer ti_kind, ti_via, ti_metric;   // two_segment_step
    bool repairs = false;               // ... has run
    bool symmetric = false;
    uint32_t *d() const { return dist.as<uint32_t>(); }
    uint16_t *f() const { return flags.as<uint16_t>(); }
    uint64_t *m() const { return mask.as<uint64_t>(); }
    const uint32_t *rd() const { return symmetric ? dist.as<uint32_t>() : rdist.as<uint32_t>(); }
    std::vector<hspf_lfa_protect> protect() const {
      return {hspf_lfa_protect{cand->root, 0u, (uint32_t)cand->nbr.size(), cand->nbr.data(), nbr_row.data(), cand->cost.data(), cand->root_link.data(),
                               cand->cflags.data()}};
    }
  };
  // The head of every chain: the CSR held against the graph (`who` names the caller in the message), the candidate table into `cand`,
  // [root] ++ its sorted distinct neighbour routers into `roots` with the row of every slot's neighbour, the mask width, the run.
  Chain chain_head(const char *who, const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                   const std::vector<uint8_t> &vflags, uint32_t root, uint32_t run_flags, uint32_t lfa_flags, LfaCandidates &cand, std::vector<uint32_t> &roots) {
    if (vflags.size() != g.n_vertices() || row_ptr.size() != vflags.size() + 1 || col.size() != g.n_links() || metric.size() != col.size())
      throw Error(HSPF_E_INVAL, std::string(who) + ": the CSR is not the one the graph was uploaded from");
    cand = lfa_candidates(row_ptr, col, metric, vflags, root);
    std::vector<uint32_t> nbrs;
    for (uint32_t v : cand.nbr) if (v != HSPF_NO_ROOT) nbrs.push_back(v);
    std::sort(nbrs.begin(), nbrs.end());
    nbrs.erase(std::unique(nbrs.begin(), nbrs.end()), nbrs.end());
    roots.push_back(root);
    roots.insert(roots.end(), nbrs.begin(), nbrs.end());
    Chain c;
    c.g = &g; c.cand = &cand; c.run_flags = run_flags; c.lfa_flags = lfa_flags;
    c.nbr_row.assign(cand.nbr.size(), 0u);
    for (size_t k = 0; k < cand.nbr.size(); ++k)
      if (cand.nbr[k] != HSPF_NO_ROOT) c.nbr_row[k] = 1u + (uint32_t)(std::lower_bound(nbrs.begin(), nbrs.end(), cand.nbr[k]) - nbrs.begin());
    c.n = g.n_vertices(); c.R = (uint32_t)roots.size();
    c.W = std::max(mask_words(g, roots), ((uint32_t)cand.nbr.size() + 63u) / 64u); c.S = 64u * c.W;
    const size_t rn = (size_t)c.R * c.n;
    c.dist = DeviceBuffer(ctx_, rn * 4); c.flags = DeviceBuffer(ctx_, rn * 2); c.mask = DeviceBuffer(ctx_, rn * 8 * c.W);
    hspf_result out{c.d(), nullptr, c.f(), c.m(), c.W, nullptr};
    check(hspf_run_device(ctx_, g.raw(), roots.data(), c.R, run_flags, &out), "hspf_run_device");
    return c;
  }
  // The LFA step: hspf_lfa_device over the head's run; the masks only for lfa() itself.  alt_flags stay for the steps behind it.
  void lfa_step(Chain &c, Lfa &r, bool with_masks) {
    const size_t n = c.n, nw = with_masks ? n * c.W : 0;
    r.n_vertices = c.n; r.mask_words = c.W;
    DeviceBuffer slot(ctx_, n * 4), met(ctx_, n * 4), cm, nm, cov(ctx_, HSPF_LFA_COVERAGE_WORDS * 4);
    c.alt_flags = DeviceBuffer(ctx_, n);
    if (with_masks) { cm = DeviceBuffer(ctx_, nw * 8); nm = DeviceBuffer(ctx_, nw * 8); }
    lfa_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), c.protect(), c.lfa_flags,
               hspf_lfa_out{slot.as<uint32_t>(), met.as<uint32_t>(), c.alt_flags.as<uint8_t>(), cm.as<uint64_t>(), nm.as<uint64_t>(), cov.as<uint32_t>()});
    r.alt_slot = slot.to_host<uint32_t>(n); r.alt_metric = met.to_host<uint32_t>(n); r.alt_flags = c.alt_flags.to_host<uint8_t>(n);
    if (with_masks) { r.cand_mask = cm.to_host<uint64_t>(nw); r.node_mask = nm.to_host<uint64_t>(nw); }
    words_to_host(cov, r.coverage);
  }
  // The head of the remote chains (all say Engine::rlfa): chain_head, the run of the same roots on the upload of the transposed CSR —
  // skipped when `symmetric` — and the LFA step.
  Chain rlfa_head(const Graph &g, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<uint32_t> &metric,
                  const std::vector<uint8_t> &vflags, uint32_t max_path_metric, uint32_t root, uint32_t run_flags, uint32_t lfa_flags, bool symmetric, Rlfa &r) {
    Chain c = chain_head("Engine::rlfa", g, row_ptr, col, metric, vflags, root, run_flags, lfa_flags, r.lfa.candidates, r.lfa.roots);
    r.slot_stride = c.S;
    c.symmetric = symmetric;
    c.rdist = DeviceBuffer(ctx_, symmetric ? 0 : (size_t)c.R * c.n * 4);
    if (!symmetric) {
      const Transposed t = csr_transpose(row_ptr, col, metric, vflags);
      Graph gt = upload(t.row_ptr, t.col, t.metric, vflags, max_path_metric);
      hspf_result rout{c.rdist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr};
      check(hspf_run_device(ctx_, gt.raw(), r.lfa.roots.data(), c.R, run_flags, &rout), "hspf_run_device on the transposed graph");
    }
    lfa_step(c, r.lfa, false);
    return c;
  }
  // The remote step: hspf_rlfa_device; the space tables, when asked for, stay for the steps behind it.
  void remote_step(Chain &c, Rlfa &r, bool with_spaces) {
    const size_t n = c.n, S = c.S, sn = with_spaces ? S * n : 0;
    DeviceBuffer pq_node(ctx_, S * 4), pq_via(ctx_, S * 4), pq_metric(ctx_, S * 4), pq_counts(ctx_, S * 4 * HSPF_RLFA_COUNT_WORDS), rl_node(ctx_, n * 4),
        rl_via(ctx_, n * 4), rl_cov(ctx_, HSPF_RLFA_COVERAGE_WORDS * 4);
    c.sp_flags = DeviceBuffer(ctx_, sn); c.sp_via = DeviceBuffer(ctx_, sn * 4);
    rlfa_device(*c.g, c.R, c.W, c.d(), c.f(), c.m(), c.rd(), c.protect(), c.lfa_flags, c.alt_flags.as<uint8_t>(),
                hspf_rlfa_out{pq_node.as<uint32_t>(), pq_via.as<uint32_t>(), pq_metric.as<uint32_t>(), pq_counts.as<uint32_t>(),
                              with_spaces ? c.sp_flags.as<uint8_t>() : nullptr, with_spaces ? c.sp_via.as<uint32_t>() : nullptr, rl_node.as<uint32_t>(),
                              rl_via.as<uint32_t>(), rl_cov.as<uint32_t>()});
    r.pq_node = pq_node.to_host<uint32_t>(S); r.pq_via = pq_via.to_host<uint32_t>(S); r.pq_metric = pq_metric.to_host<uint32_t>(S);
    r.pq_counts = pq_counts.to_host<uint32_t>(S * HSPF_RLFA_COUNT_WORDS);
    if (with_spaces) { r.space_flags = c.sp_flags.to_host<uint8_t>(sn); r.space_via = c.sp_via.to_host<uint32_t>(sn); }
    r.rl_node = rl_node.to_host<uint32_t>(n); r.rl_via = rl_via.to_host<uint32_t>(n);
    words_to_host(rl_cov, r.rl_coverage);
  }
  // The two-segment step: hspf_tilfa_device on the space tables; kind, via and metric of every slot stay for the backup step.
  void two_segment_step(Chain &c, Tilfa &t) {
    const size_t n = c.n, S = c.S;
    c.ti_kind = DeviceBuffer(ctx_, S); c.ti_via = DeviceBuffer(ctx_, S * 4); c.ti_metric = DeviceBuffer(ctx_, S * 4);
    c.repairs = true;
    DeviceBuffer tp(ctx_, S * 4), tq(ctx_, S * 4), tl(ctx_, S * 4), tc(ctx_, S * 4 * HSPF_TILFA_COUNT_WORDS), dk(ctx_, n), dc(ctx_, HSPF_TILFA_COVERAGE_WORDS * 4);
    tilfa_device(*c.g, c.R, c.W, c.d(), c.f(), c.m(), c.rd(), c.protect(), c.lfa_flags, c.alt_flags.as<uint8_t>(), c.sp_flags.as<uint8_t>(), c.sp_via.as<uint32_t>(),
                 hspf_tilfa_out{c.ti_kind.as<uint8_t>(), tp.as<uint32_t>(), tq.as<uint32_t>(), c.ti_via.as<uint32_t>(), tl.as<uint32_t>(), c.ti_metric.as<uint32_t>(),
                                tc.as<uint32_t>(), dk.as<uint8_t>(), dc.as<uint32_t>()});
    t.ti_kind = c.ti_kind.to_host<uint8_t>(S); t.ti_p = tp.to_host<uint32_t>(S); t.ti_q = tq.to_host<uint32_t>(S);
    t.ti_via = c.ti_via.to_host<uint32_t>(S); t.ti_link = tl.to_host<uint32_t>(S); t.ti_metric = c.ti_metric.to_host<uint32_t>(S);
    t.ti_counts = tc.to_host<uint32_t>(S * HSPF_TILFA_COUNT_WORDS); t.td_kind = dk.to_host<uint8_t>(n);
    words_to_host(dc, t.td_coverage);
  }
  // The ascending union of the vertices a select call listed into `y`, and their rows (dist only) on the forward graph; one padding
  // row keeps the arguments of the evaluate call valid where no list holds a vertex.
  DeviceBuffer rows_of(const Chain &c, const std::vector<uint32_t> &listed, std::vector<uint32_t> &y) {
    for (uint32_t v : listed) if (v != HSPF_NO_ROOT) y.push_back(v);
    std::sort(y.begin(), y.end());
    y.erase(std::unique(y.begin(), y.end()), y.end());
    const bool none = y.empty();
    if (none) y.push_back(HSPF_NO_ROOT);
    DeviceBuffer ydist(ctx_, y.size() * (size_t)c.n * 4);
    if (none) return ydist;
    hspf_result yout{ydist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr};
    check(hspf_run_device(ctx_, c.g->raw(), y.data(), (uint32_t)y.size(), c.run_flags, &yout), "hspf_run_device over the listed vertices");
    return ydist;
  }
  // The node-protecting pair: the remote LFA (select, the rows of the listed PQ nodes, evaluate), then the two-segment repairs
  // (select, the rows of the listed q's, evaluate with the nd_kind of the first); both read the space tables.
  void node_steps(Chain &c, TilfaNode &t) {
    const size_t n = c.n, S = c.S, SQ = S * t.max_pq, SP = S * t.max_pairs;
    const std::vector<hspf_lfa_protect> p = c.protect();
    DeviceBuffer qn(ctx_, SQ * 4), qv(ctx_, SQ * 4), qm(ctx_, SQ * 4), qc(ctx_, S * 4);
    const hspf_rlfa_node_sel nsel{qn.as<uint32_t>(), qv.as<uint32_t>(), qm.as<uint32_t>(), qc.as<uint32_t>()};
    rlfa_node_select_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), p, c.lfa_flags, c.sp_flags.as<uint8_t>(), t.max_pq, nsel);
    t.nq_node = qn.to_host<uint32_t>(SQ); t.nq_via = qv.to_host<uint32_t>(SQ); t.nq_metric = qm.to_host<uint32_t>(SQ); t.nq_count = qc.to_host<uint32_t>(S);
    const DeviceBuffer ydn = rows_of(c, t.nq_node, t.pq_roots);
    DeviceBuffer dk(ctx_, n), dn(ctx_, n * 4), dv(ctx_, n * 4), dm(ctx_, n * 4), dc(ctx_, HSPF_NP_COVERAGE_WORDS * 4);
    rlfa_node_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), p, ydn.as<uint32_t>(), t.pq_roots, nsel, t.max_pq, c.alt_flags.as<uint8_t>(),
                     hspf_rlfa_node_out{dk.as<uint8_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(), dm.as<uint32_t>(), nullptr, dc.as<uint32_t>()});
    t.nd_kind = dk.to_host<uint8_t>(n); t.nd_node = dn.to_host<uint32_t>(n); t.nd_via = dv.to_host<uint32_t>(n); t.nd_metric = dm.to_host<uint32_t>(n);
    words_to_host(dc, t.nd_coverage);
    DeviceBuffer tq(ctx_, SP * 4), tp(ctx_, SP * 4), tl(ctx_, SP * 4), tvi(ctx_, SP * 4), tme(ctx_, SP * 4), tc(ctx_, S * 4);
    const hspf_tilfa_node_sel tsel{tq.as<uint32_t>(), tp.as<uint32_t>(), tl.as<uint32_t>(), tvi.as<uint32_t>(), tme.as<uint32_t>(), tc.as<uint32_t>()};
    tilfa_node_select_device(*c.g, c.R, c.W, c.d(), c.f(), c.m(), p, c.lfa_flags, c.sp_flags.as<uint8_t>(), t.max_pairs, tsel);
    t.tq_q = tq.to_host<uint32_t>(SP); t.tq_p = tp.to_host<uint32_t>(SP); t.tq_link = tl.to_host<uint32_t>(SP);
    t.tq_via = tvi.to_host<uint32_t>(SP); t.tq_metric = tme.to_host<uint32_t>(SP); t.tq_count = tc.to_host<uint32_t>(S);
    const DeviceBuffer ydq = rows_of(c, t.tq_q, t.y_roots);
    DeviceBuffer ek(ctx_, n), ep(ctx_, n * 4), eq(ctx_, n * 4), el(ctx_, n * 4), ev(ctx_, n * 4), em(ctx_, n * 4), es(ctx_, n * 4), ec(ctx_, HSPF_TN_COVERAGE_WORDS * 4);
    tilfa_node_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), p, ydq.as<uint32_t>(), t.y_roots, tsel, t.max_pairs, c.alt_flags.as<uint8_t>(), dk.as<uint8_t>(),
                      hspf_tilfa_node_out{ek.as<uint8_t>(), ep.as<uint32_t>(), eq.as<uint32_t>(), el.as<uint32_t>(), ev.as<uint32_t>(), em.as<uint32_t>(),
                                          es.as<uint32_t>(), ec.as<uint32_t>()});
    t.tn_kind = ek.to_host<uint8_t>(n); t.tn_p = ep.to_host<uint32_t>(n); t.tn_q = eq.to_host<uint32_t>(n); t.tn_link = el.to_host<uint32_t>(n);
    t.tn_via = ev.to_host<uint32_t>(n); t.tn_metric = em.to_host<uint32_t>(n); t.tn_set = es.to_host<uint32_t>(n);
    words_to_host(ec, t.tn_coverage);
  }
  // The routes-and-backup step: hspf_routes_device for the root's row, hspf_routes_backup_device on it (with the repairs of the
  // two-segment step where it ran), and behind them — with_ecmp — hspf_routes_backup_ecmp_device twice: the sizing call, the filling call.
  void backup_step(Chain &c, BackupRoutes &b, const hspf_prefix_table &table) {
    const size_t np = table.n_prefixes, nz = std::max<size_t>(np, 1), W = c.W;
    const std::vector<hspf_lfa_protect> p = c.protect();
    DeviceBuffer bm(ctx_, nz * 4), be(ctx_, nz * 4), nh(ctx_, nz * 8 * W), kk(ctx_, nz), pp(ctx_, nz * 4), ss(ctx_, nz * 4), mm(ctx_, nz * 4), ff(ctx_, nz),
        cmk(ctx_, nz * 8 * W), nmk(ctx_, nz * 8 * W), cv(ctx_, HSPF_BK_COVERAGE_WORDS * 4);
    hspf_routes ro{bm.as<uint32_t>(), be.as<uint32_t>(), nh.as<uint64_t>()};
    check(hspf_routes_device(ctx_, c.n, 1, c.W, c.d(), c.f(), c.m(), &table, &ro), "hspf_routes_device");
    hspf_prefix_table tr = table;
    tr.flags |= HSPF_PFX_RESIDENT;                      // the arrays hspf_routes_device has just staged
    const hspf_tilfa_out tio{c.ti_kind.as<uint8_t>(), nullptr, nullptr, c.ti_via.as<uint32_t>(), nullptr, c.ti_metric.as<uint32_t>(), nullptr, nullptr, nullptr};
    const hspf_tilfa_out *ti = c.repairs ? &tio : nullptr;
    routes_backup_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), p, c.lfa_flags, tr, ro, ti,
                         hspf_backup_out{kk.as<uint8_t>(), pp.as<uint32_t>(), ss.as<uint32_t>(), mm.as<uint32_t>(), ff.as<uint8_t>(), cmk.as<uint64_t>(),
                                         nmk.as<uint64_t>(), cv.as<uint32_t>()});
    b.best_metric = bm.to_host<uint32_t>(np); b.best_entry = be.to_host<uint32_t>(np); b.nexthop_mask = nh.to_host<uint64_t>(np * W);
    b.bk_kind = kk.to_host<uint8_t>(np); b.bk_primary = pp.to_host<uint32_t>(np); b.bk_slot = ss.to_host<uint32_t>(np);
    b.bk_metric = mm.to_host<uint32_t>(np); b.bk_flags = ff.to_host<uint8_t>(np);
    b.bk_cand_mask = cmk.to_host<uint64_t>(np * W); b.bk_node_mask = nmk.to_host<uint64_t>(np * W);
    words_to_host(cv, b.bk_coverage);
    if (!b.with_ecmp) return;
    DeviceBuffer ptr(ctx_, (np + 1) * 4);
    const uint64_t total = routes_backup_ecmp_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), p, c.lfa_flags, tr, ro, ti, 0,
                                                     hspf_backup_ecmp_out{ptr.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
    if (total) {
      const size_t t = (size_t)total;
      DeviceBuffer pri(ctx_, t * 4), knd(ctx_, t), slot(ctx_, t * 4), met(ctx_, t * 4), efl(ctx_, t), cov(ctx_, HSPF_BK_ECMP_COVERAGE_WORDS * 4);
      routes_backup_ecmp_device(c.n, c.R, c.W, c.d(), c.f(), c.m(), p, c.lfa_flags, tr, ro, ti, total,
                                hspf_backup_ecmp_out{ptr.as<uint32_t>(), pri.as<uint32_t>(), knd.as<uint8_t>(), slot.as<uint32_t>(), met.as<uint32_t>(),
                                                     efl.as<uint8_t>(), cov.as<uint32_t>()});
      b.eb_primary = pri.to_host<uint32_t>(t); b.eb_kind = knd.to_host<uint8_t>(t); b.eb_slot = slot.to_host<uint32_t>(t);
      b.eb_metric = met.to_host<uint32_t>(t); b.eb_flags = efl.to_host<uint8_t>(t);
      words_to_host(cov, b.eb_coverage);
    }
    b.eb_ptr = ptr.to_host<uint32_t>(np + 1);
  }
  std::shared_ptr<CtxHolder> holder_;
  hspf_ctx *ctx_ = nullptr;
};

}  // namespace hspf
#endif
