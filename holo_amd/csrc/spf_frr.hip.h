// spf_frr.hip.h — host side of the fast-reroute calls of the C ABI (include/holo_spf_hip.h).  Included by spf_capi.hip (one TU).
//   host arithmetic:       hspf_lfa_candidates, hspf_lfa_lan_candidates, hspf_csr_transpose, hspf_srlg_members
//   alternates:            hspf_lfa_device, hspf_lfa_lan_device, hspf_lfa_srlg_device (lfa_call); hspf_lfa_ecmp_device (lfa_ecmp_call)
//   remote alternates:     hspf_rlfa_device, hspf_rlfa_lan_device, hspf_rlfa_srlg_device (rlfa_call)
//   two-segment repairs:   hspf_tilfa_device
//   post-convergence path: hspf_tilfa_pc_device
//   per-prefix backups:    hspf_routes_backup_device, hspf_routes_backup_lan_device, hspf_routes_backup_srlg_device (routes_backup);
//                          hspf_routes_backup_ecmp_device, hspf_routes_backup_ecmp_srlg_device (backup_ecmp_call)
//   node protection:       hspf_rlfa_node_select_device, hspf_rlfa_node_device, hspf_tilfa_node_select_device, hspf_tilfa_node_device,
//                          hspf_routes_backup_node_device
//
// The 19 device calls share one staged structure — the candidate tables of the protected roots (spf_frr_common.hip.h) — and one
// frame, FrrCall: its checks, stage(), the call's memsets, gather() where the kernels need the per-root scalars, the call's own
// kernels, finish().  A call that leaves any other way drains the stream in the frame's destructor.  `fn` names the calling entry
// point in hspf_last_error.
#pragma once

#include <unordered_map>

#include "spf_lfa.hip.h"
#include "spf_rlfa.hip.h"
#include "spf_tilfa.hip.h"
#include "spf_tilfa_pc.hip.h"
#include "spf_backup.hip.h"
#include "spf_rlfa_node.hip.h"
#include "spf_tilfa_node.hip.h"
#include "spf_backup_node.hip.h"
#include "spf_srlg.hip.h"
#include "spf_backup_srlg.hip.h"
#include "spf_backup_ecmp.hip.h"

namespace {

int frr_bad(hspf_ctx *ctx, const char *fn, const std::string &what) { ctx->last_error = std::string(fn) + ": " + what; return HSPF_E_INVAL; }

// The checks of the protected roots, and the staged block (its layout: spf_frr_common.hip.h) copied to ctx->lfa_tab on the context's
// stream, with ctx->lfa_scal sized for k_lfa_gather.  `tab` is the copy's source: the frame's (FrrCall), which outlives the copy.
int lfa_stage(hspf_ctx *ctx, const char *fn, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const hspf_lfa_protect *prot,
                     uint32_t n_prot, std::vector<uint32_t> &tab, uint32_t *out_max_k) {
  auto bad = [&](const std::string &what) { return frr_bad(ctx, fn, what); };
  size_t tab_words = (size_t)n_prot * LFA_HDR_WORDS, scal_words = 0;
  uint32_t max_k = 0;
  for (uint32_t i = 0; i < n_prot; ++i) {
    const hspf_lfa_protect &p = prot[i];
    const std::string who = "protected root " + std::to_string(i) + ": ";
    if (p.root_row >= n_rows) return bad(who + "root_row >= n_rows");
    if (p.root_vertex >= n_vertices) return bad(who + "root_vertex >= n_vertices");
    if (p.n_slots > 64ull * n_mask_words) return bad(who + "n_slots > 64 * n_mask_words");
    if (p.n_slots && (!p.nbr || !p.nbr_row || !p.cost || !p.root_link || !p.cflags)) return bad(who + "NULL slot array");
    for (uint32_t k = 0; k < p.n_slots; ++k) {
      if (p.nbr[k] == HSPF_NO_ROOT) continue;
      if (p.nbr[k] >= n_vertices) return bad(who + "nbr of slot " + std::to_string(k) + " >= n_vertices");
      if (p.nbr_row[k] >= n_rows) return bad(who + "nbr_row of slot " + std::to_string(k) + " >= n_rows");
    }
    tab_words += (size_t)FRR_COLS * p.n_slots;
    scal_words += (size_t)p.n_slots * ((size_t)p.n_slots + 1);
    max_k = std::max(max_k, p.n_slots);
  }
  if (tab_words > (1u << 28) || scal_words > (1u << 28)) { ctx->last_error = std::string(fn) + ": the slot tables of this call need more than 1 GiB of scratch"; return HSPF_E_NOMEM; }
  tab.assign(tab_words, 0u);
  size_t to = (size_t)n_prot * LFA_HDR_WORDS, so = 0;
  for (uint32_t i = 0; i < n_prot; ++i) {
    const hspf_lfa_protect &p = prot[i];
    const uint32_t K = p.n_slots;
    uint32_t *h = tab.data() + (size_t)i * LFA_HDR_WORDS, *t = tab.data() + to;
    uint32_t C = 0;
    for (uint32_t k = 0; k < K; ++k) {
      const bool c = p.nbr[k] != HSPF_NO_ROOT;
      t[k] = p.nbr[k]; t[K + k] = c ? p.nbr_row[k] : 0u; t[2 * K + k] = p.cost[k]; t[3 * K + k] = p.root_link[k];
      t[4 * K + k] = c ? p.cflags[k] : 0u;
      if (c) t[5 * K + C++] = k;
    }
    h[0] = p.root_vertex; h[1] = p.root_row; h[2] = K; h[3] = C; h[4] = (uint32_t)to; h[5] = (uint32_t)so;
    to += (size_t)FRR_COLS * K; so += (size_t)K * ((size_t)K + 1);
  }
  (void)hipSetDevice(ctx->device);
  int rc;
  if ((rc = ensure(ctx, ctx->lfa_tab, tab_words * 4, false))) return rc;
  if ((rc = ensure(ctx, ctx->lfa_scal, std::max<size_t>(scal_words, 1) * 4, false))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->lfa_tab.p, tab.data(), tab_words * 4, hipMemcpyHostToDevice, ctx->stream));
  *out_max_k = max_k;
  return HSPF_OK;
}

// The LAN columns of a LAN call, checked: before anything is staged or launched.
int lan_check(hspf_ctx *ctx, const char *fn, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const hspf_lfa_protect *prot,
              const hspf_lfa_lan *lan, uint32_t n_prot) {
  if (!lan) return frr_bad(ctx, fn, "NULL lan pointer");
  for (uint32_t i = 0; i < n_prot; ++i) {
    const std::string who = "protected root " + std::to_string(i) + ": ";
    if (prot[i].n_slots > 64ull * n_mask_words) return frr_bad(ctx, fn, who + "n_slots > 64 * n_mask_words");      // (before lan is read that far)
    if (prot[i].n_slots && (!lan[i].lan || !lan[i].lan_row)) return frr_bad(ctx, fn, who + "NULL lan / lan_row array");
    for (uint32_t k = 0; k < prot[i].n_slots; ++k) {
      if (lan[i].lan[k] == HSPF_NO_ROOT) continue;
      if (lan[i].lan[k] >= n_vertices) return frr_bad(ctx, fn, who + "lan of slot " + std::to_string(k) + " >= n_vertices");
      if (lan[i].lan_row[k] >= n_rows) return frr_bad(ctx, fn, who + "lan_row of slot " + std::to_string(k) + " >= n_rows");
    }
  }
  return HSPF_OK;
}

// The LAN block (its layout: spf_frr_common.hip.h) copied to ctx->lan_tab on the context's stream, with ctx->lan_scal sized for
// k_lfa_gather_lan.  After lan_check and lfa_stage.  `ltab` is the copy's source: the frame's.
int lan_stage(hspf_ctx *ctx, const char *fn, const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, std::vector<uint32_t> &ltab,
              LanArgs *out, size_t *out_max_gather) {
  ltab.assign((size_t)n_prot * LAN_HDR_WORDS, 0u);
  size_t so = 0, max_gather = 0;
  std::vector<uint32_t> lv;
  for (uint32_t i = 0; i < n_prot; ++i) {
    const uint32_t K = prot[i].n_slots;
    const size_t to = ltab.size();
    ltab.resize(to + 2 * (size_t)K, 0u);
    lv.clear();
    std::unordered_map<uint32_t, uint32_t> index;                   // LAN vertex -> its index, in order of first appearance
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t L = lan[i].lan[k];
      uint32_t j = LFA_NONE;
      if (L != HSPF_NO_ROOT) {
        auto it = index.find(L);
        if (it == index.end()) { it = index.emplace(L, (uint32_t)lv.size()).first; lv.push_back(L); }
        j = it->second;
      }
      ltab[to + k] = j; ltab[to + K + k] = j != LFA_NONE ? lan[i].lan_row[k] : 0u;
    }
    ltab.insert(ltab.end(), lv.begin(), lv.end());
    const size_t NL = lv.size();
    if (ltab.size() > (1u << 28) || so + (size_t)K * NL > (1u << 28)) { ctx->last_error = std::string(fn) + ": the LAN tables of this call need more than 1 GiB of scratch"; return HSPF_E_NOMEM; }
    uint32_t *h = ltab.data() + (size_t)i * LAN_HDR_WORDS;
    h[0] = (uint32_t)NL; h[1] = (uint32_t)to; h[2] = (uint32_t)so;
    so += (size_t)K * NL;
    max_gather = std::max(max_gather, (size_t)K * ((size_t)K + 1 + NL));
  }
  int rc;
  if ((rc = ensure(ctx, ctx->lan_tab, ltab.size() * 4, false))) return rc;
  if ((rc = ensure(ctx, ctx->lan_scal, std::max<size_t>(so, 1) * 4, false))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->lan_tab.p, ltab.data(), ltab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  out->ltab = (const uint32_t *)ctx->lan_tab.p; out->lscal = (uint32_t *)ctx->lan_scal.p;
  *out_max_gather = max_gather;
  return HSPF_OK;
}

static_assert(SRLG_MAXM == HSPF_SRLG_MAX_MEMBERS && RLFA_SRLG_CW == HSPF_RLFA_SRLG_COUNT_WORDS, "the kernels' member bound and count width are the header's");

// The member columns of an SRLG call, checked: before anything is staged or launched.  Every index a kernel dereferences is held
// to its bound here.
int srlg_check(hspf_ctx *ctx, const char *fn, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const hspf_lfa_protect *prot,
               const hspf_srlg *srlg, uint32_t n_prot) {
  if (!srlg) return frr_bad(ctx, fn, "NULL srlg pointer");
  for (uint32_t i = 0; i < n_prot; ++i) {
    const std::string who = "protected root " + std::to_string(i) + ": ";
    const uint32_t K = prot[i].n_slots;
    const hspf_srlg &g = srlg[i];
    if (K > 64ull * n_mask_words) return frr_bad(ctx, fn, who + "n_slots > 64 * n_mask_words");      // (before mem_ptr is read that far)
    if (!g.mem_ptr) return frr_bad(ctx, fn, who + "NULL mem_ptr");
    for (uint32_t k = 0; k < K; ++k) {
      if (g.mem_ptr[k + 1] < g.mem_ptr[k]) return frr_bad(ctx, fn, who + "mem_ptr is not monotone at slot " + std::to_string(k));
      if (g.mem_ptr[k + 1] - g.mem_ptr[k] > HSPF_SRLG_MAX_MEMBERS) return frr_bad(ctx, fn, who + "slot " + std::to_string(k) + " has more than HSPF_SRLG_MAX_MEMBERS members");
    }
    if (g.mem_ptr[K] > g.mem_ptr[0] && (!g.tail || !g.pos || !g.head || !g.cost || !g.tail_row || !g.head_row)) return frr_bad(ctx, fn, who + "NULL member column");
    for (uint32_t m = g.mem_ptr[0]; m < g.mem_ptr[K]; ++m) {
      const std::string mem = "member " + std::to_string(m);
      if (g.tail[m] >= n_vertices || g.head[m] >= n_vertices) return frr_bad(ctx, fn, who + "tail or head of " + mem + " >= n_vertices");
      if (g.tail_row[m] >= n_rows || g.head_row[m] >= n_rows) return frr_bad(ctx, fn, who + "tail_row or head_row of " + mem + " >= n_rows");
    }
  }
  return HSPF_OK;
}

// The member block (its layout: spf_srlg.hip.h; behind its six member columns a seventh, pos [NM], that only k_backup_srlg reads)
// copied to ctx->srlg_tab on the context's stream, with ctx->srlg_scal sized for k_srlg_gather.  After srlg_check and lfa_stage.  `stab` is the copy's source: the frame's.
int srlg_stage(hspf_ctx *ctx, const char *fn, const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, std::vector<uint32_t> &stab,
               SrlgArgs *out, size_t *out_max_gather, uint32_t *out_max_nms) {
  stab.assign((size_t)n_prot * SRLG_HDR_WORDS, 0u);
  size_t so = 0, max_gather = 0;
  uint32_t max_nms = 0;
  struct Mem { uint32_t tail, pos, head, cost, trow, hrow; };
  std::vector<Mem> dm;                                              // the distinct members, in order of first appearance
  std::vector<uint32_t> sidx;
  for (uint32_t i = 0; i < n_prot; ++i) {
    const uint32_t K = prot[i].n_slots, S = prot[i].root_vertex;
    const hspf_srlg &g = srlg[i];
    const size_t to = stab.size();
    dm.clear(); sidx.clear();
    std::unordered_map<uint64_t, std::vector<uint32_t>> index;      // (tail, pos) -> the distinct members that carry it
    stab.resize(to + 2 * (size_t)K + 1, 0u);
    uint32_t nms = 0;
    for (uint32_t k = 0; k < K; ++k) {
      stab[to + k] = (uint32_t)sidx.size();
      for (uint32_t m = g.mem_ptr[k]; m < g.mem_ptr[k + 1]; ++m) {
        const Mem x{g.tail[m], g.pos[m], g.head[m], g.cost[m], g.tail_row[m], g.head_row[m]};
        std::vector<uint32_t> &same = index[((uint64_t)x.tail << 32) | x.pos];
        uint32_t j = LFA_NONE;
        for (uint32_t c : same)
          if (dm[c].head == x.head && dm[c].cost == x.cost && dm[c].trow == x.trow && dm[c].hrow == x.hrow) j = c;
        if (j == LFA_NONE) { j = (uint32_t)dm.size(); dm.push_back(x); same.push_back(j); }
        sidx.push_back(j);
      }
      if (g.mem_ptr[k + 1] > g.mem_ptr[k] && prot[i].nbr[k] != HSPF_NO_ROOT) stab[to + K + 1 + nms++] = k;
    }
    stab[to + K] = (uint32_t)sidx.size();
    stab.insert(stab.end(), sidx.begin(), sidx.end());
    const size_t NM = dm.size(), mo = stab.size();
    stab.resize(mo + SRLG_STAGED_COLS * NM);
    for (size_t j = 0; j < NM; ++j) {
      stab[mo + j] = dm[j].tail; stab[mo + NM + j] = dm[j].head; stab[mo + 2 * NM + j] = dm[j].cost;
      stab[mo + 3 * NM + j] = dm[j].trow; stab[mo + 4 * NM + j] = dm[j].hrow; stab[mo + 5 * NM + j] = dm[j].tail == S ? dm[j].pos : LFA_NONE;
      stab[mo + SRLG_POS_COL * NM + j] = dm[j].pos;                      // (read through srlg_pos() in spf_backup_srlg.hip.h)
    }
    const size_t scal = NM * (1 + 2 * (size_t)K);
    if (stab.size() > (1u << 28) || so + scal > (1u << 28)) { ctx->last_error = std::string(fn) + ": the member tables of this call need more than 1 GiB of scratch"; return HSPF_E_NOMEM; }
    uint32_t *h = stab.data() + (size_t)i * SRLG_HDR_WORDS;
    h[0] = (uint32_t)NM; h[1] = (uint32_t)to; h[2] = (uint32_t)so; h[3] = (uint32_t)sidx.size(); h[4] = nms;
    so += scal;
    max_gather = std::max(max_gather, scal);
    max_nms = std::max(max_nms, nms);
  }
  int rc;
  if ((rc = ensure(ctx, ctx->srlg_tab, stab.size() * 4, false))) return rc;
  if ((rc = ensure(ctx, ctx->srlg_scal, std::max<size_t>(so, 1) * 4, false))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->srlg_tab.p, stab.data(), stab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  out->stab = (const uint32_t *)ctx->srlg_tab.p; out->sscal = (uint32_t *)ctx->srlg_scal.p;
  *out_max_gather = max_gather; *out_max_nms = max_nms;
  return HSPF_OK;
}

// The graph's two-way flags, one byte per link in the order of the device's raw CSR, copied to ctx->tilfa_tw on the context's stream
// (hspf_tilfa_device, hspf_tilfa_node_select_device).  The host mirror's pool is in that order unless a patch moved rows; then `tw`,
// the frame's, is the copy's source.
int tw_stage(hspf_ctx *ctx, const char *fn, const hspf_graph *g, std::vector<uint8_t> &tw) {
  auto bad = [&](const std::string &what) { return frr_bad(ctx, fn, what); };
  const uint32_t e = g->e;
  int rc;
  if ((rc = ensure(ctx, ctx->tilfa_tw, std::max<size_t>(e, 1), false))) return rc;
  const uint8_t *tw_src = g->twoway.data();
  if (!g->pool_compact()) {
    tw.resize(e);
    size_t o = 0;
    for (uint32_t v = 0; v < g->n; ++v) {
      if (o + g->rlen[v] > e) return bad("the graph's host mirror and its link count disagree");
      if (g->rlen[v]) memcpy(tw.data() + o, g->twoway.data() + g->rstart[v], g->rlen[v]);
      o += g->rlen[v];
    }
    if (o != e) return bad("the graph's host mirror and its link count disagree");
    tw_src = tw.data();
  } else if (g->twoway.size() < e) return bad("the graph's host mirror and its link count disagree");
  if (e) HIPCHK(ctx, hipMemcpyAsync(ctx->tilfa_tw.p, tw_src, e, hipMemcpyHostToDevice, ctx->stream));
  return HSPF_OK;
}

// The walk behind hspf_lfa_candidates and hspf_lfa_lan_candidates: slot(index, target, cost, first link, target is a network,
// two-way) for every first-hop slot of `root` in slot order.  Returns the number of slots as hspf_lfa_candidates does.
template <class F>
int lfa_walk(const hspf_csr *csr, uint32_t root, uint32_t *out_total_slots, F &&slot) {
  if (!csr || !csr->row_ptr || !csr->vflags || (csr->n_edges && (!csr->col || !csr->metric)) || root >= csr->n_vertices) return HSPF_E_INVAL;
  return guarded(nullptr, [&]() -> int {
    const uint32_t n = csr->n_vertices;
    const uint32_t *rp = csr->row_ptr, *col = csr->col, *met = csr->metric;
    auto row_ok = [&](uint32_t v) { return rp[v] <= rp[v + 1] && rp[v + 1] <= csr->n_edges; };
    auto links_back = [&](uint32_t t, uint32_t v) {                 // the two-way check: does t's row list v?  (cost not compared)
      if (!row_ok(t)) return false;
      for (uint32_t k = rp[t]; k < rp[t + 1]; ++k) if (col[k] == v) return true;
      return false;
    };
    // H = [root] ++ networks reached through networks only, breadth-first, links in row order, each once (hspf_slot_table);
    // per entry the cost of its discovery path and the link of the root's row that starts it
    struct HEnt { uint32_t v, path_cost, first_link; };
    std::vector<HEnt> H{{root, 0u, 0u}};
    std::vector<uint32_t> seen{root};                               // (sorted: H holds a handful of vertices)
    uint64_t total = 0;
    for (size_t qi = 0; qi < H.size(); ++qi) {
      const HEnt p = H[qi];
      if (!row_ok(p.v)) return HSPF_E_INVAL;
      for (uint32_t k = rp[p.v]; k < rp[p.v + 1]; ++k, ++total) {
        const uint32_t t = col[k], j = k - rp[p.v];
        if (t >= n) return HSPF_E_INVAL;
        if (total > 0xFFFFFFF0ull) return HSPF_E_INVAL;
        const uint64_t c64 = (uint64_t)p.path_cost + met[k];
        const uint32_t c = c64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c64;
        const uint32_t first = qi == 0 ? j : p.first_link;
        const bool net = (csr->vflags[t] & HSPF_VF_NETWORK) != 0;
        const bool two = (net || t != root) && links_back(t, p.v);
        slot(total, t, c, first, net, two);
        if (net && two) {
          auto it = std::lower_bound(seen.begin(), seen.end(), t);
          if (it == seen.end() || *it != t) { seen.insert(it, t); H.push_back({t, c, first}); }
        }
      }
    }
    if (out_total_slots) *out_total_slots = (uint32_t)total;
    return (int)std::min<uint64_t>(total, 0x7FFFFFFFull);
  });
}

static_assert(bk_cov_words(FrrProt::Plain) == HSPF_BK_COVERAGE_WORDS && bk_cov_words(FrrProt::Lan) == HSPF_BK_LAN_COVERAGE_WORDS &&
              bk_cov_words(FrrProt::Srlg) == HSPF_BK_SRLG_COVERAGE_WORDS, "the coverage kernel's widths are the header's");

// ---- the frame of a device call ----------------------------------------------------------------------------------------------
// One FrrCall per call, declared inside the guarded() lambda.  It holds the call's common arguments, the shared checks, and every
// host block whose copy to the device the call enqueues (the candidate tables, the LAN or member block, the two-way bytes) with
// what staging them yields for the launches.  A call reads top to bottom: checks -> stage -> memsets -> arguments -> launches ->
// finish().  Every other way out behind the first enqueue — a return, a HIPCHK, an exception on its way to guarded() — passes
// the destructor, which drains the stream: no copy is left reading a block of the frame, or of the caller, that is gone.
struct FrrCall {
  hspf_ctx *const ctx; const char *const fn;
  const uint32_t n, R, W;                               // n_vertices, n_rows, n_mask_words
  const uint32_t *const dist; const uint16_t *const flags; const uint64_t *const mask;
  const hspf_lfa_protect *const prot; const uint32_t n_prot;
  size_t stride = 0, n_slots = 0;                       // 64 * W, n_prot * stride (check_slots)
  std::vector<uint32_t> tab, mtab;                      // sources of the staged copies: the candidate tables; the LAN or member block (hspf_tilfa_pc_device: its row block)
  std::vector<uint8_t> tw;                              // the same: the two-way bytes where a patch moved rows
  uint32_t max_k = 0, max_nms = 0;
  size_t max_gather = 0;
  LanArgs la{};
  SrlgArgs sa{};
  uint32_t tiles_x = 0; size_t n_tiles = 0; uint32_t *d_total = nullptr;      // the CSR stream of the ECMP calls (stream_open)
  uint32_t *ymap = nullptr; uint32_t n_yrows = 0;       // the listed nodes' vertex -> row map (node_map)
  void *owned = nullptr;                                // device scratch of this call alone (scratch): released with the frame
  bool enqueued = false, finished = false;

  FrrCall(hspf_ctx *ctx, const char *fn, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words, const uint32_t *dist_dev,
          const uint16_t *flags_dev, const uint64_t *mask_dev, const hspf_lfa_protect *prot, uint32_t n_prot)
      : ctx(ctx), fn(fn), n(n_vertices), R(n_rows), W(n_mask_words), dist(dist_dev), flags(flags_dev), mask(mask_dev), prot(prot), n_prot(n_prot) {}
  FrrCall(const FrrCall &) = delete;
  ~FrrCall() {
    if (enqueued && !finished) (void)hipStreamSynchronize(ctx->stream);
    if (owned) (void)hipFree(owned);
  }

  // -- checks: nothing is staged, written or launched before the last of them
  int bad(const std::string &what) const { return frr_bad(ctx, fn, what); }
  // the tables, prot and out; `more`: the call's further pointers, which `what` names with them
  int check_ptrs(const void *out, bool more = true, const char *what = "NULL table, prot or out pointer") const {
    return (!more || !dist || !flags || !mask || !prot || !out) ? bad(what) : HSPF_OK;
  }
  int check_dims() const {
    if (n == 0 || R == 0 || W == 0 || n_prot == 0 || n_prot > 65535u || W > (1u << 20)) return bad("n_vertices, n_rows, n_mask_words or n_prot out of range");
    return HSPF_OK;
  }
  int check_graph(const hspf_graph *g) const {
    if (g->invalid) return bad("the graph is invalid after a failed hspf_graph_patch (free it and upload again)");
    return g->n != n ? bad("n_vertices is not the graph's") : HSPF_OK;
  }
  int check_twoway(const hspf_graph *g) const { return g->twoway.size() != g->col.size() ? bad("the graph holds no two-way flags") : HSPF_OK; }
  int check_slots() {                                   // after check_dims
    stride = (size_t)64 * W; n_slots = (size_t)n_prot * stride;
    return n_slots > (1u << 28) ? bad("n_prot * 64 * n_mask_words out of range") : HSPF_OK;
  }
  int check_routes(const hspf_routes *r) const {
    return (!r->best_metric || !r->best_entry || !r->nexthop_mask) ? bad("NULL best_metric / best_entry / nexthop_mask") : HSPF_OK;
  }
  int check_prefix_table(const hspf_prefix_table *t) const {      // (the entries: stage_prefix_table)
    if (!t->pfx_ptr || (t->n_entries && (!t->pfx_vertex || !t->pfx_metric))) return bad("NULL pfx_ptr / pfx_vertex / pfx_metric");
    return (t->flags & HSPF_PFX_ORDERED) ? bad("HSPF_PFX_ORDERED tables are out of scope") : HSPF_OK;
  }
  int check_tilfa(FrrProt mode, const hspf_tilfa_out *ti) const {
    const bool srlg = mode == FrrProt::Srlg;            // its repairs are walked: the forced adjacency is read too
    if (ti && (!ti->ti_kind || !ti->ti_via || !ti->ti_metric || (srlg && (!ti->ti_p || !ti->ti_link))))
      return bad(srlg ? "NULL ti_kind / ti_via / ti_metric / ti_p / ti_link in tilfa_dev" : "NULL ti_kind / ti_via / ti_metric in tilfa_dev");
    return HSPF_OK;
  }
  // a selection struct and its list length; `where`: "" for the call that writes it, " in sel_dev" ... for one that reads it
  int check_rn_sel(const hspf_rlfa_node_sel *q, uint32_t max_pq, const char *where) const {
    if (!q->nq_node || !q->nq_via || !q->nq_metric || !q->nq_count) return bad(std::string("NULL nq_node / nq_via / nq_metric / nq_count") + where);
    return (max_pq == 0 || max_pq > HSPF_RLFA_NODE_MAX_PQ) ? bad("max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ") : HSPF_OK;
  }
  int check_tn_sel(const hspf_tilfa_node_sel *q, uint32_t max_pairs, const char *where) const {
    if (!q->tq_q || !q->tq_p || !q->tq_link || !q->tq_via || !q->tq_metric || !q->tq_count)
      return bad(std::string("NULL tq_q / tq_p / tq_link / tq_via / tq_metric / tq_count") + where);
    return (max_pairs == 0 || max_pairs > HSPF_TILFA_NODE_MAX_PAIRS) ? bad("max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS") : HSPF_OK;
  }
  int check_y_roots(const uint32_t *y_roots, uint32_t n_y) const {      // after check_dims
    if (n_y == 0) return bad("n_yrows is 0");
    for (uint32_t i = 0; i < n_y; ++i)
      if (y_roots[i] != HSPF_NO_ROOT && y_roots[i] >= n) return bad("y_roots entry " + std::to_string(i) + " >= n_vertices");
    return HSPF_OK;
  }
  // the mode's columns (`lan` is read in the mode Lan alone, `srlg` in the mode Srlg alone; so in stage)
  int check_mode(FrrProt mode, const hspf_lfa_lan *lan, const hspf_srlg *srlg) const {
    if (mode == FrrProt::Lan) return lan_check(ctx, fn, n, R, W, prot, lan, n_prot);
    return mode == FrrProt::Srlg ? srlg_check(ctx, fn, n, R, W, prot, srlg, n_prot) : HSPF_OK;
  }
  // the entries an ECMP call can emit, bounded: its ptr array is u32, the scan's carry too (`items`: what n_items counts)
  int check_pairs(uint32_t n_items, const char *items) const {
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < n_prot; ++i) pairs += (uint64_t)n_items * std::max(prot[i].n_slots, 1u);
    return pairs >= (1ull << 32) ? bad(std::string(items) + " * max(n_slots, 1), summed over the protected roots, reaches 2^32: split the protect list") : HSPF_OK;
  }

  // -- staging: from here on the stream may hold copies out of this frame
  hipStream_t stream() { enqueued = true; return ctx->stream; }
  int stage_prefix_table(const hspf_prefix_table *t) { enqueued = true; return pfx_table_stage(ctx, fn, n, t); }
  // lfa_stage (with the checks of the protected roots), then the mode's block.  After check_mode.
  int stage(FrrProt mode, const hspf_lfa_lan *lan, const hspf_srlg *srlg) {
    enqueued = true;
    int rc;
    if ((rc = lfa_stage(ctx, fn, n, R, W, prot, n_prot, tab, &max_k))) return rc;
    if (mode == FrrProt::Lan) return lan_stage(ctx, fn, prot, lan, n_prot, mtab, &la, &max_gather);
    return mode == FrrProt::Srlg ? srlg_stage(ctx, fn, prot, srlg, n_prot, mtab, &sa, &max_gather, &max_nms) : HSPF_OK;
  }
  int stage_twoway(const hspf_graph *g) { enqueued = true; return tw_stage(ctx, fn, g, tw); }
  // Scratch that the call sizes and the frame releases (one per call): too large to stay with the context.  Nothing is enqueued
  // on it yet when this fails; the destructor frees it behind the drained stream.
  int scratch(size_t bytes, void **out) {
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMalloc(&owned, std::max<size_t>(bytes, 8)));
    *out = owned;
    return HSPF_OK;
  }
  // The vertex -> row map of the listed nodes (after check_y_roots): ctx->rnode_map sized and cleared, the list copied behind it
  // (the caller's: it lives through the call).  launch_node_map() fills the map; a frame's own memsets may stand between the two.
  int node_map(const uint32_t *y_roots, uint32_t n_y) {
    int rc;
    if ((rc = ensure(ctx, ctx->rnode_map, ((size_t)n + n_y) * 4, false))) return rc;
    hipStream_t s = stream();
    ymap = (uint32_t *)ctx->rnode_map.p; n_yrows = n_y;
    HIPCHK(ctx, hipMemsetAsync(ymap, 0xFF, (size_t)n * 4, s));
    HIPCHK(ctx, hipMemcpyAsync(ymap + n, y_roots, (size_t)n_y * 4, hipMemcpyHostToDevice, s));
    return HSPF_OK;
  }
  void launch_node_map() {
    RnodeDestArgs m{};                                  // k_rlfa_nmap reads n, the root list and the map
    m.n = n; m.yroots = ymap + n; m.n_yrows = n_yrows; m.ymap = ymap;
    hipLaunchKernelGGL(k_rlfa_nmap, dim3((n_yrows + 255) / 256), dim3(256), 0, ctx->stream, m);
  }

  // -- launches
  // The gather of the mode on the staged blocks: d(N_k, S) and d(N_k, N_p) of every protected root (k_lfa_gather), in the mode Lan
  // with d(N_k, L) (k_lfa_gather_lan), in the mode Srlg followed by the members' distances (k_srlg_gather).  Returns the arguments
  // it launched with (lfa_call goes on with them).
  LfaArgs gather(FrrProt mode, uint32_t lfa_flags) {
    LfaArgs a{};
    a.n = n; a.W = W; a.ignore_overload = (lfa_flags & HSPF_LFA_IGNORE_OVERLOAD) ? 1u : 0u;
    a.dist = dist; a.flags = flags; a.mask = mask;
    a.tab = (const uint32_t *)ctx->lfa_tab.p; a.scal = (uint32_t *)ctx->lfa_scal.p;
    auto grid = [&](size_t work) { return dim3((uint32_t)std::min<size_t>((work + 255) / 256, 1024), n_prot); };
    if (mode == FrrProt::Lan) {
      if (max_gather) hipLaunchKernelGGL(k_lfa_gather_lan, grid(max_gather), dim3(256), 0, ctx->stream, a, la);
    } else if (max_k) {
      hipLaunchKernelGGL(k_lfa_gather, grid((size_t)max_k * ((size_t)max_k + 1)), dim3(256), 0, ctx->stream, a);
    }
    if (mode == FrrProt::Srlg && max_gather) hipLaunchKernelGGL(k_srlg_gather, grid(max_gather), dim3(256), 0, ctx->stream, a, sa);
    return a;
  }
  // The CSR stream of the ECMP calls, before anything is staged: the tile scratch of n_items per protected root and the pinned word
  // the total arrives in (h_ev[1]: word 0 is the event stream's).  After check_pairs.
  int stream_open(uint32_t n_items) {
    (void)hipSetDevice(ctx->device);
    tiles_x = (n_items + LFA_TILE - 1) / LFA_TILE; n_tiles = (size_t)tiles_x * n_prot;
    int rc;
    if ((rc = ensure(ctx, ctx->ea_scr, (n_tiles + 4) * 4, false))) return rc;
    if (!ctx->h_ev) HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_ev, 64, hipHostMallocDefault));
    HIPCHK(ctx, hipHostGetDevicePointer((void **)&d_total, ctx->h_ev, 0));
    ++d_total;
    return HSPF_OK;
  }
  uint32_t *tile() const { return (uint32_t *)ctx->ea_scr.p; }
  // ... and its end: count(grid) -> k_events_scan -> fill(grid), ONE synchronisation, the total
  template <class Count, class Fill>
  int stream_close(Count &&count, Fill &&fill, const char *kernels, uint64_t *out_total) {
    const dim3 grid(tiles_x, n_prot);
    count(grid);
    hipLaunchKernelGGL(k_events_scan, dim3(1), dim3(1024), 0, ctx->stream, (uint32_t)n_tiles, tile(), tile() + n_tiles, d_total);
    fill(grid);
    int rc;
    if ((rc = finish(kernels))) return rc;
    *out_total = ctx->h_ev[1];
    return HSPF_OK;
  }
  // The end of a call: a launch error is reported under the name of its kernels (nullptr: nothing was launched); then the stream
  // is drained.
  int finish(const char *kernels) {
    const hipError_t le = kernels ? hipGetLastError() : hipSuccess;
    if (le != hipSuccess) { ctx->last_error = std::string(kernels) + ": " + hipGetErrorString(le); return HSPF_E_HIP; }
    finished = true;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return HSPF_OK;
  }
};

// What the per-prefix backup kernels of both families read: the table set, the staged tables and scalars, the staged prefix table,
// the routes, the repairs of tilfa_dev; in `b` what the mode Srlg adds (the member block, the forced adjacency, the repairs flag).
// The outputs are the caller's to fill in.
BackupArgs backup_args(const FrrCall &f, const LfaArgs &ga, uint32_t lfa_flags, const hspf_prefix_table *t, const hspf_routes *routes_dev,
                       const hspf_tilfa_out *tilfa_dev, BackupSrlgArgs *b) {
  BackupArgs a{};
  a.n = f.n; a.W = f.W; a.ignore_overload = ga.ignore_overload; a.stride = 64u * f.W;
  a.n_pfx = t->n_prefixes; a.sat = (t->flags & HSPF_PFX_SATURATING) ? 1u : 0u;
  a.dist = f.dist; a.flags = f.flags;
  a.tab = ga.tab; a.scal = ga.scal;
  a.pfx_ptr = (const uint32_t *)f.ctx->pf_ptr.p; a.pfx_vertex = (const uint32_t *)f.ctx->pf_vtx.p; a.pfx_metric = (const uint32_t *)f.ctx->pf_met.p;
  a.best_metric = routes_dev->best_metric; a.best_entry = routes_dev->best_entry; a.nh_mask = routes_dev->nexthop_mask;
  *b = BackupSrlgArgs{};
  b->sa = f.sa; b->repairs = (lfa_flags & HSPF_LFA_SRLG_SAFE_REPAIRS) ? 1u : 0u;
  if (tilfa_dev) {
    a.ti_kind = tilfa_dev->ti_kind; a.ti_via = tilfa_dev->ti_via; a.ti_metric = tilfa_dev->ti_metric;
    b->ti_p = tilfa_dev->ti_p; b->ti_link = tilfa_dev->ti_link;
  }
  return a;
}

// The one frame of hspf_routes_backup_device, hspf_routes_backup_lan_device and hspf_routes_backup_srlg_device: `lan` is read in
// the mode Lan alone, `srlg` in the mode Srlg alone.
int routes_backup(hspf_ctx *ctx, const char *fn, FrrProt mode, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                  const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                  const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                  const hspf_prefix_table *t, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev, hspf_backup_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, fn, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, t && routes_dev, "NULL table, prot, prefix table, routes or out pointer")) || (rc = f.check_routes(routes_dev))) return rc;
    if (!out_dev->bk_kind || !out_dev->bk_primary || !out_dev->bk_slot || !out_dev->bk_metric || !out_dev->bk_flags || !out_dev->bk_coverage)
      return f.bad("NULL bk_kind / bk_primary / bk_slot / bk_metric / bk_flags / bk_coverage");
    if ((rc = f.check_tilfa(mode, tilfa_dev)) || (rc = f.check_dims()) || (rc = f.check_prefix_table(t)) || (rc = f.check_slots()) ||
        (rc = f.check_mode(mode, lan, srlg)) || (rc = f.stage_prefix_table(t)) || (rc = f.stage(mode, lan, srlg))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(out_dev->bk_coverage, 0, (size_t)n_prot * bk_cov_words(mode) * 4, s));
    if (!t->n_prefixes) return f.finish(nullptr);       // nothing to launch
    const LfaArgs ga = f.gather(mode, lfa_flags);
    BackupSrlgArgs b;
    BackupArgs a = backup_args(f, ga, lfa_flags, t, routes_dev, tilfa_dev, &b);
    a.bk_kind = out_dev->bk_kind; a.bk_primary = out_dev->bk_primary; a.bk_slot = out_dev->bk_slot; a.bk_metric = out_dev->bk_metric;
    a.bk_flags = out_dev->bk_flags; a.cand_mask = out_dev->bk_cand_mask; a.node_mask = out_dev->bk_node_mask; a.coverage = out_dev->bk_coverage;
    const uint32_t n_tiles = (t->n_prefixes + LFA_TILE - 1) / LFA_TILE;
    const dim3 grid(n_tiles, n_prot), cgrid(std::min(n_tiles, 64u), n_prot);
    if (mode == FrrProt::Lan) {
      hipLaunchKernelGGL(k_backup_lan, grid, dim3(256), 0, s, a, BackupProt<FrrProt::Lan>{f.la, (lfa_flags & HSPF_LFA_LAN_SAFE_REPAIRS) ? 1u : 0u, 0u});
      hipLaunchKernelGGL(k_backup_cov_lan, cgrid, dim3(256), 0, s, a);
    } else if (mode == FrrProt::Srlg) {
      hipLaunchKernelGGL(k_backup_srlg, grid, dim3(256), 0, s, a, BackupProt<FrrProt::Srlg>{b});
      hipLaunchKernelGGL(k_backup_cov_srlg, cgrid, dim3(256), 0, s, a);
    } else {
      hipLaunchKernelGGL(k_backup, grid, dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_backup_cov, cgrid, dim3(256), 0, s, a);
    }
    return f.finish(mode == FrrProt::Lan ? "k_backup_lan" : mode == FrrProt::Srlg ? "k_backup_srlg" : "k_backup");
  });
}

// The one frame of hspf_lfa_device, hspf_lfa_lan_device and hspf_lfa_srlg_device (`lan`, `srlg`: as routes_backup)
int lfa_call(hspf_ctx *ctx, const char *fn, FrrProt mode, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
             const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
             const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags, hspf_lfa_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, fn, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev))) return rc;
    if (!out_dev->alt_slot || !out_dev->alt_metric || !out_dev->alt_flags || !out_dev->coverage) return f.bad("NULL alt_slot / alt_metric / alt_flags / coverage");
    if ((rc = f.check_dims()) || (rc = f.check_mode(mode, lan, srlg)) || (rc = f.stage(mode, lan, srlg))) return rc;
    hipStream_t s = f.stream();
    const uint32_t coverage_words = mode == FrrProt::Lan ? HSPF_LFA_LAN_COVERAGE_WORDS : mode == FrrProt::Srlg ? HSPF_LFA_SRLG_COVERAGE_WORDS : HSPF_LFA_COVERAGE_WORDS;
    HIPCHK(ctx, hipMemsetAsync(out_dev->coverage, 0, (size_t)n_prot * coverage_words * 4, s));
    LfaArgs a = f.gather(mode, lfa_flags);
    a.alt_slot = out_dev->alt_slot; a.alt_metric = out_dev->alt_metric; a.alt_flags = out_dev->alt_flags;
    a.cand_mask = out_dev->cand_mask; a.node_mask = out_dev->node_mask; a.coverage = out_dev->coverage;
    const dim3 grid((n_vertices + LFA_TILE - 1) / LFA_TILE, n_prot);
    const bool one = f.max_k <= 64;                     // every root's slots fit one mask word: the tables go to LDS
    if (mode == FrrProt::Lan) {
      if (one) hipLaunchKernelGGL(k_lfa_lan<true>, grid, dim3(256), 0, s, a, LfaProt<FrrProt::Lan>{f.la});
      else hipLaunchKernelGGL(k_lfa_lan<false>, grid, dim3(256), 0, s, a, LfaProt<FrrProt::Lan>{f.la});
    } else if (mode == FrrProt::Srlg) {
      if (one) hipLaunchKernelGGL(k_lfa_srlg<true>, grid, dim3(256), 0, s, a, LfaProt<FrrProt::Srlg>{f.sa});
      else hipLaunchKernelGGL(k_lfa_srlg<false>, grid, dim3(256), 0, s, a, LfaProt<FrrProt::Srlg>{f.sa});
    } else {
      if (one) hipLaunchKernelGGL(k_lfa<true>, grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL(k_lfa<false>, grid, dim3(256), 0, s, a);
    }
    return f.finish(mode == FrrProt::Lan ? "k_lfa_lan" : mode == FrrProt::Srlg ? "k_lfa_srlg" : "k_lfa");
  });
}

static_assert(EA_CW == HSPF_LFA_ECMP_COVERAGE_WORDS && HSPF_LFA_EA_PRIMARY == 0x20u, "the fill kernel's coverage width and primary bit are the header's");

// The frame of hspf_lfa_ecmp_device (kernels: spf_lfa_ecmp.hip.h): the checks and the staging of lfa_call, then the frame's CSR stream
int lfa_ecmp_call(hspf_ctx *ctx, const char *fn, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                  const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                  const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, uint64_t cap_entries, hspf_lfa_ecmp_out *out_dev,
                  uint64_t *out_total) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, fn, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev))) return rc;
    if (!out_dev->ea_ptr || !out_total) return f.bad("NULL ea_ptr or out_total");
    if (cap_entries && (!out_dev->ea_primary || !out_dev->ea_slot || !out_dev->ea_metric || !out_dev->ea_flags || !out_dev->ea_coverage))
      return f.bad("NULL ea_primary / ea_slot / ea_metric / ea_flags / ea_coverage with cap_entries > 0");
    if ((rc = f.check_dims()) || (rc = f.check_pairs(n_vertices, "n_vertices")) || (rc = f.stream_open(n_vertices)) ||
        (rc = f.stage(FrrProt::Plain, nullptr, nullptr))) return rc;
    hipStream_t s = f.stream();
    if (out_dev->ea_coverage) HIPCHK(ctx, hipMemsetAsync(out_dev->ea_coverage, 0, (size_t)n_prot * HSPF_LFA_ECMP_COVERAGE_WORDS * 4, s));
    LfaEcmpArgs a{};
    a.l = f.gather(FrrProt::Plain, lfa_flags);
    a.n_prot = n_prot; a.cap = cap_entries; a.tile = f.tile();
    a.ea_ptr = out_dev->ea_ptr; a.ea_primary = out_dev->ea_primary; a.ea_slot = out_dev->ea_slot; a.ea_metric = out_dev->ea_metric;
    a.ea_flags = out_dev->ea_flags; a.ea_coverage = out_dev->ea_coverage;
    return f.stream_close([&](dim3 grid) { hipLaunchKernelGGL(k_lfa_ecmp_count, grid, dim3(256), 0, s, a); },
                          [&](dim3 grid) {
                            if (f.max_k <= 64) hipLaunchKernelGGL(k_lfa_ecmp_fill<true>, grid, dim3(256), 0, s, a);
                            else hipLaunchKernelGGL(k_lfa_ecmp_fill<false>, grid, dim3(256), 0, s, a);
                          }, "k_lfa_ecmp", out_total);
  });
}

static_assert(be_cov_words(FrrProt::Plain) == HSPF_BK_ECMP_COVERAGE_WORDS && be_cov_words(FrrProt::Srlg) == HSPF_BK_ECMP_SRLG_COVERAGE_WORDS,
              "the fill kernel's coverage widths are the header's");

// The one frame of hspf_routes_backup_ecmp_device and hspf_routes_backup_ecmp_srlg_device (kernels: spf_backup_ecmp.hip.h; `srlg`
// is read in the mode Srlg alone): the checks, the staging and the arguments of routes_backup in the same mode, then the frame's
// CSR stream as lfa_ecmp_call (the same scratch and the same pinned word).
int backup_ecmp_call(hspf_ctx *ctx, const char *fn, FrrProt mode, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                     const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                     const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags, const hspf_prefix_table *t,
                     const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev, uint64_t cap_entries, hspf_backup_ecmp_out *out_dev,
                     uint64_t *out_total) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, fn, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, t && routes_dev, "NULL table, prot, prefix table, routes or out pointer")) || (rc = f.check_routes(routes_dev))) return rc;
    if (!out_dev->eb_ptr || !out_total) return f.bad("NULL eb_ptr or out_total");
    if (cap_entries && (!out_dev->eb_primary || !out_dev->eb_kind || !out_dev->eb_slot || !out_dev->eb_metric || !out_dev->eb_flags || !out_dev->eb_coverage))
      return f.bad("NULL eb_primary / eb_kind / eb_slot / eb_metric / eb_flags / eb_coverage with cap_entries > 0");
    if ((rc = f.check_tilfa(mode, tilfa_dev)) || (rc = f.check_dims()) || (rc = f.check_prefix_table(t)) || (rc = f.check_slots()) ||
        (rc = f.check_pairs(t->n_prefixes, "n_prefixes")) || (rc = f.check_mode(mode, nullptr, srlg)) || (rc = f.stage_prefix_table(t)) ||
        (rc = f.stream_open(t->n_prefixes)) || (rc = f.stage(mode, nullptr, srlg))) return rc;
    hipStream_t s = f.stream();
    if (out_dev->eb_coverage) HIPCHK(ctx, hipMemsetAsync(out_dev->eb_coverage, 0, (size_t)n_prot * be_cov_words(mode) * 4, s));
    if (!t->n_prefixes) {                               // nothing to launch: the one word of eb_ptr
      HIPCHK(ctx, hipMemsetAsync(out_dev->eb_ptr, 0, 4, s));
      if ((rc = f.finish(nullptr))) return rc;
      *out_total = 0;
      return HSPF_OK;
    }
    const LfaArgs ga = f.gather(mode, lfa_flags);
    BackupEcmpArgs a{};
    BackupEcmpProt<FrrProt::Srlg> pa{};
    a.b = backup_args(f, ga, lfa_flags, t, routes_dev, tilfa_dev, &pa.s);
    a.n_prot = n_prot; a.cap = cap_entries; a.tile = f.tile();
    a.eb_ptr = out_dev->eb_ptr; a.eb_primary = out_dev->eb_primary; a.eb_kind = out_dev->eb_kind; a.eb_slot = out_dev->eb_slot;
    a.eb_metric = out_dev->eb_metric; a.eb_flags = out_dev->eb_flags; a.eb_coverage = out_dev->eb_coverage;
    return f.stream_close([&](dim3 grid) { hipLaunchKernelGGL(k_backup_ecmp_count, grid, dim3(256), 0, s, a); },
                          [&](dim3 grid) {
                            if (mode == FrrProt::Srlg) hipLaunchKernelGGL(k_backup_ecmp_fill_srlg, grid, dim3(256), 0, s, a, pa);
                            else hipLaunchKernelGGL(k_backup_ecmp_fill, grid, dim3(256), 0, s, a);
                          }, mode == FrrProt::Srlg ? "k_backup_ecmp_srlg" : "k_backup_ecmp", out_total);
  });
}

static_assert(RLFA_CW == HSPF_RLFA_COUNT_WORDS && RLFA_LAN_CW == HSPF_RLFA_LAN_COUNT_WORDS, "the kernels' count widths are the header's");

// The one frame of hspf_rlfa_device, hspf_rlfa_lan_device and hspf_rlfa_srlg_device (`lan`, `srlg`: as routes_backup)
int rlfa_call(hspf_ctx *ctx, const char *fn, FrrProt mode, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
              const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
              const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
              const uint8_t *alt_flags_in_dev, hspf_rlfa_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, fn, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, g && rdist_dev, "NULL graph, table, prot or out pointer"))) return rc;
    if (!out_dev->pq_node || !out_dev->pq_via || !out_dev->pq_metric || !out_dev->pq_counts || !out_dev->rl_node || !out_dev->rl_via || !out_dev->rl_coverage)
      return f.bad("NULL pq_node / pq_via / pq_metric / pq_counts / rl_node / rl_via / rl_coverage");
    if ((rc = f.check_dims()) || (rc = f.check_graph(g)) || (rc = f.check_slots()) || (rc = f.check_mode(mode, lan, srlg)) ||
        (rc = f.stage(mode, lan, srlg)) || (rc = ensure(ctx, ctx->rlfa_key, f.n_slots * 8, false))) return rc;
    hipStream_t s = f.stream();
    const bool with_lan = mode == FrrProt::Lan, with_srlg = mode == FrrProt::Srlg;
    const uint32_t count_words = with_lan ? HSPF_RLFA_LAN_COUNT_WORDS : with_srlg ? HSPF_RLFA_SRLG_COUNT_WORDS : HSPF_RLFA_COUNT_WORDS;
    const uint32_t coverage_words = with_lan ? HSPF_RLFA_LAN_COVERAGE_WORDS : with_srlg ? HSPF_RLFA_SRLG_COVERAGE_WORDS : HSPF_RLFA_COVERAGE_WORDS;
    HIPCHK(ctx, hipMemsetAsync(ctx->rlfa_key.p, 0xFF, f.n_slots * 8, s));
    HIPCHK(ctx, hipMemsetAsync(out_dev->pq_counts, 0, f.n_slots * count_words * 4, s));
    HIPCHK(ctx, hipMemsetAsync(out_dev->rl_coverage, 0, (size_t)n_prot * coverage_words * 4, s));
    const LfaArgs ga = f.gather(mode, lfa_flags);
    RlfaArgs a{};
    a.n = n_vertices; a.W = n_mask_words; a.ignore_overload = ga.ignore_overload; a.stride = (uint32_t)f.stride;
    a.dist = dist_dev; a.rdist = rdist_dev; a.flags = flags_dev; a.mask = mask_dev; a.vf = (const uint8_t *)g->d_vflags;
    a.tab = ga.tab; a.scal = ga.scal;
    a.alt_in = alt_flags_in_dev; a.key = (unsigned long long *)ctx->rlfa_key.p;
    a.pq_node = out_dev->pq_node; a.pq_via = out_dev->pq_via; a.pq_metric = out_dev->pq_metric; a.pq_counts = out_dev->pq_counts;
    a.space_flags = out_dev->space_flags; a.space_via = out_dev->space_via;
    a.rl_node = out_dev->rl_node; a.rl_via = out_dev->rl_via; a.rl_cov = out_dev->rl_coverage;
    const uint32_t n_tiles = (n_vertices + LFA_TILE - 1) / LFA_TILE;
    const dim3 grid(n_tiles, n_prot), fgrid((uint32_t)((f.n_slots + 255) / 256));
    if (with_lan) {
      hipLaunchKernelGGL(k_rlfa_lan, grid, dim3(256), 0, s, a, RlfaLan<true>{f.la});
      hipLaunchKernelGGL(k_rlfa_final_lan, fgrid, dim3(256), 0, s, a, n_prot, RlfaLan<true>{f.la});
      hipLaunchKernelGGL(k_rlfa_dest_lan, grid, dim3(256), 0, s, a, RlfaLan<true>{f.la});
    } else if (with_srlg) {
      hipLaunchKernelGGL(k_rlfa_srlg, grid, dim3(256), 0, s, a, f.sa);
      if (f.max_nms) hipLaunchKernelGGL(k_rlfa_srlg_slot, dim3(n_tiles, std::min(f.max_nms, 65535u), n_prot), dim3(256), 0, s, a, f.sa);
      hipLaunchKernelGGL(k_rlfa_srlg_final, fgrid, dim3(256), 0, s, a, n_prot, f.sa);
      hipLaunchKernelGGL(k_rlfa_srlg_dest, grid, dim3(256), 0, s, a, f.sa);
    } else {
      hipLaunchKernelGGL(k_rlfa, grid, dim3(256), 0, s, a, RlfaLan<false>{});
      hipLaunchKernelGGL(k_rlfa_final, fgrid, dim3(256), 0, s, a, n_prot, RlfaLan<false>{});
      hipLaunchKernelGGL(k_rlfa_dest, grid, dim3(256), 0, s, a, RlfaLan<false>{});
    }
    return f.finish(with_lan ? "k_rlfa_lan" : with_srlg ? "k_rlfa_srlg" : "k_rlfa");
  });
}

}  // namespace

extern "C" {

// ---- loop-free alternates (include/holo_spf_hip.h "loop-free alternates on device"; kernels: spf_lfa.hip.h) ----------------
int hspf_lfa_candidates(const hspf_csr *csr, uint32_t root, uint32_t cap, uint32_t *nbr, uint32_t *cost, uint32_t *root_link,
                        uint8_t *cflags, uint32_t *out_total_slots) {
  return lfa_walk(csr, root, out_total_slots, [&](uint64_t k, uint32_t t, uint32_t c, uint32_t first, bool net, bool two) {
    if (k >= cap) return;
    const bool is_cand = !net && t != root && two;
    if (nbr) nbr[k] = is_cand ? t : HSPF_NO_ROOT;
    if (cost) cost[k] = c;
    if (root_link) root_link[k] = first;
    if (cflags) cflags[k] = (is_cand && (csr->vflags[t] & HSPF_VF_NO_TRANSIT)) ? (uint8_t)HSPF_LFA_C_NO_TRANSIT : (uint8_t)0;
  });
}

// The slots of the root's own row come first and in link order, so link `first` of a deeper slot has been seen when the slot is.
int hspf_lfa_lan_candidates(const hspf_csr *csr, uint32_t root, uint32_t cap, uint32_t *lan, uint32_t *out_total_slots) {
  std::vector<uint32_t> of_link;                                    // per link of the root's row: the LAN it leads to
  uint32_t own = 0;
  if (csr && csr->row_ptr && root < csr->n_vertices && csr->row_ptr[root] <= csr->row_ptr[root + 1]) own = csr->row_ptr[root + 1] - csr->row_ptr[root];
  return lfa_walk(csr, root, out_total_slots, [&](uint64_t k, uint32_t t, uint32_t, uint32_t first, bool net, bool two) {
    if (k < own) of_link.push_back(net && two ? t : HSPF_NO_ROOT);
    if (k < cap && lan) lan[k] = first < of_link.size() ? of_link[first] : HSPF_NO_ROOT;
  });
}

int hspf_lfa_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                    const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                    const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, hspf_lfa_out *out_dev) {
  return lfa_call(ctx, "hspf_lfa_device", FrrProt::Plain, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, nullptr, nullptr, n_prot,
                  lfa_flags, out_dev);
}

int hspf_lfa_lan_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                        const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                        const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, uint32_t lfa_flags, hspf_lfa_out *out_dev) {
  return lfa_call(ctx, "hspf_lfa_lan_device", FrrProt::Lan, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, lan, nullptr, n_prot,
                  lfa_flags, out_dev);
}

int hspf_lfa_ecmp_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                         const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, uint64_t cap_entries,
                         hspf_lfa_ecmp_out *out_dev, uint64_t *out_total) {
  return lfa_ecmp_call(ctx, "hspf_lfa_ecmp_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot, lfa_flags,
                       cap_entries, out_dev, out_total);
}

// ---- remote loop-free alternates (include/holo_spf_hip.h "remote loop-free alternates on device"; kernels: spf_rlfa.hip.h) ----
int hspf_csr_transpose(const hspf_csr *csr, uint32_t *row_ptr_out, uint32_t *col_out, uint32_t *metric_out) {
  if (!csr || !row_ptr_out) return HSPF_E_INVAL;
  const uint32_t n = csr->n_vertices, e = csr->n_edges;
  if (n == 0 || n > (1u << 24) || e > HSPF_MAX_LINKS || !csr->row_ptr || !csr->vflags || (e && (!csr->col || !csr->metric || !col_out || !metric_out))) return HSPF_E_INVAL;
  if (csr->row_ptr[0] != 0 || csr->row_ptr[n] != e) return HSPF_E_INVAL;
  for (uint32_t u = 0; u < n; ++u)
    if (csr->row_ptr[u + 1] < csr->row_ptr[u]) return HSPF_E_INVAL;
  for (uint32_t k = 0; k < e; ++k)
    if (csr->col[k] >= n) return HSPF_E_INVAL;
  // a stable counting sort by target: the links are visited by ascending source, then by position in the source's row
  for (uint32_t t = 0; t <= n; ++t) row_ptr_out[t] = 0;
  for (uint32_t k = 0; k < e; ++k) ++row_ptr_out[csr->col[k] + 1];
  for (uint32_t t = 0; t < n; ++t) row_ptr_out[t + 1] += row_ptr_out[t];
  for (uint32_t u = 0; u < n; ++u)
    for (uint32_t k = csr->row_ptr[u]; k < csr->row_ptr[u + 1]; ++k) {
      const uint32_t o = row_ptr_out[csr->col[k]]++;                 // (row_ptr_out[t] runs from the start of row t to its end ...)
      col_out[o] = u; metric_out[o] = csr->metric[k];
    }
  for (uint32_t t = n; t > 0; --t) row_ptr_out[t] = row_ptr_out[t - 1];      // (... which is the start of row t + 1: shift back)
  row_ptr_out[0] = 0;
  return HSPF_OK;
}

int hspf_rlfa_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                     const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                     const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                     hspf_rlfa_out *out_dev) {
  return rlfa_call(ctx, "hspf_rlfa_device", FrrProt::Plain, g, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, prot, nullptr,
                   nullptr, n_prot, lfa_flags, alt_flags_in_dev, out_dev);
}

int hspf_rlfa_lan_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                         const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, uint32_t lfa_flags,
                         const uint8_t *alt_flags_in_dev, hspf_rlfa_out *out_dev) {
  return rlfa_call(ctx, "hspf_rlfa_lan_device", FrrProt::Lan, g, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, prot, lan,
                   nullptr, n_prot, lfa_flags, alt_flags_in_dev, out_dev);
}

// ---- shared-risk link groups (include/holo_spf_hip.h "SRLG-safe alternates and remote-LFA spaces"; kernels: spf_srlg.hip.h) ----
int hspf_srlg_members(const hspf_csr *csr, uint32_t root, const uint32_t *grp_ptr, const uint32_t *grp, uint32_t cap_slots, uint32_t cap_members,
                      uint32_t *mem_ptr, uint32_t *tail, uint32_t *pos, uint32_t *head, uint32_t *cost, uint32_t *out_total_slots,
                      uint32_t *out_total_members) {
  if (!csr || !csr->row_ptr || !grp_ptr || root >= csr->n_vertices) return HSPF_E_INVAL;
  const uint32_t n = csr->n_vertices, e = csr->n_edges;
  if (csr->row_ptr[0] != 0 || csr->row_ptr[n] != e || (e && (!csr->col || !csr->metric))) return HSPF_E_INVAL;
  for (uint32_t u = 0; u < n; ++u)
    if (csr->row_ptr[u + 1] < csr->row_ptr[u]) return HSPF_E_INVAL;
  for (uint32_t l = 0; l < e; ++l)
    if (grp_ptr[l + 1] < grp_ptr[l]) return HSPF_E_INVAL;
  if (grp_ptr[e] > grp_ptr[0] && !grp) return HSPF_E_INVAL;
  std::vector<uint32_t> rl;                                         // root_link of every slot
  uint32_t total_slots = 0;
  const int K = lfa_walk(csr, root, &total_slots, [&](uint64_t, uint32_t, uint32_t, uint32_t first, bool, bool) { rl.push_back(first); });
  if (K < 0) return K;
  return guarded(nullptr, [&]() -> int {
    const uint32_t own = csr->row_ptr[root + 1] - csr->row_ptr[root];
    // per link of the root's row that some slot stands behind: the links that share a group with it, ascending, itself left out
    std::vector<std::vector<uint32_t>> of_link(own);
    std::vector<uint8_t> wanted(own, 0), done(own, 0);
    for (uint32_t f : rl) if (f < own) wanted[f] = 1;
    std::unordered_map<uint32_t, std::vector<uint32_t>> by_group;   // group id -> its links, ascending (filled on first need)
    bool filled = false;
    uint64_t total = 0;
    for (size_t k = 0; k < rl.size(); ++k) {
      if (k <= cap_slots && mem_ptr) mem_ptr[k] = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);      // (entry cap_slots closes slot cap_slots - 1)
      const uint32_t f = rl[k];
      if (f >= own) continue;
      const uint32_t prot_link = csr->row_ptr[root] + f;
      if (!done[f]) {
        done[f] = 1;
        if (grp_ptr[prot_link + 1] > grp_ptr[prot_link]) {
          if (!filled) {
            filled = true;
            for (uint32_t l = 0; l < e; ++l)
              for (uint32_t x = grp_ptr[l]; x < grp_ptr[l + 1]; ++x) {
                std::vector<uint32_t> &v = by_group[grp[x]];
                if (v.empty() || v.back() != l) v.push_back(l);
              }
          }
          std::vector<uint32_t> &m = of_link[f];
          for (uint32_t x = grp_ptr[prot_link]; x < grp_ptr[prot_link + 1]; ++x) {
            const std::vector<uint32_t> &v = by_group[grp[x]];
            m.insert(m.end(), v.begin(), v.end());
          }
          std::sort(m.begin(), m.end());
          m.erase(std::unique(m.begin(), m.end()), m.end());
          m.erase(std::remove(m.begin(), m.end(), prot_link), m.end());
        }
      }
      for (uint32_t l : of_link[f]) {
        if (csr->col[l] >= n) return HSPF_E_INVAL;
        if (total < cap_members) {
          const uint32_t a = (uint32_t)(std::upper_bound(csr->row_ptr, csr->row_ptr + n + 1, l) - csr->row_ptr) - 1u;      // the row that holds link l
          if (tail) tail[total] = a;
          if (pos) pos[total] = l - csr->row_ptr[a];
          if (head) head[total] = csr->col[l];
          if (cost) cost[total] = csr->metric[l];
        }
        ++total;
      }
    }
    if (total > 0xFFFFFFF0ull) return HSPF_E_INVAL;
    if (rl.size() <= cap_slots && mem_ptr) mem_ptr[rl.size()] = (uint32_t)total;
    if (out_total_slots) *out_total_slots = total_slots;
    if (out_total_members) *out_total_members = (uint32_t)total;
    return K;
  });
}

int hspf_lfa_srlg_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                         const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags, hspf_lfa_out *out_dev) {
  return lfa_call(ctx, "hspf_lfa_srlg_device", FrrProt::Srlg, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, nullptr, srlg, n_prot,
                  lfa_flags, out_dev);
}

int hspf_rlfa_srlg_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                          const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                          const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                          const uint8_t *alt_flags_in_dev, hspf_rlfa_out *out_dev) {
  return rlfa_call(ctx, "hspf_rlfa_srlg_device", FrrProt::Srlg, g, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, rdist_dev, prot, nullptr,
                   srlg, n_prot, lfa_flags, alt_flags_in_dev, out_dev);
}

// ---- per-prefix backups with shared-risk link groups (include/holo_spf_hip.h "per-prefix SRLG-safe backups"; kernels: spf_backup_srlg.hip.h) ----
int hspf_routes_backup_srlg_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                   const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                   const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                                   const hspf_prefix_table *table, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev,
                                   hspf_backup_out *out_dev) {
  return routes_backup(ctx, "hspf_routes_backup_srlg_device", FrrProt::Srlg, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, nullptr,
                       srlg, n_prot, lfa_flags, table, routes_dev, tilfa_dev, out_dev);
}

// ---- per-primary SRLG-safe backups of ECMP prefixes (include/holo_spf_hip.h "per-primary SRLG-safe backups for ECMP prefixes"; kernels: spf_backup_ecmp.hip.h) ----
int hspf_routes_backup_ecmp_srlg_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                        const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                        const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                                        const hspf_prefix_table *table, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev,
                                        uint64_t cap_entries, hspf_backup_ecmp_out *out_dev, uint64_t *out_total) {
  return backup_ecmp_call(ctx, "hspf_routes_backup_ecmp_srlg_device", FrrProt::Srlg, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, srlg,
                          n_prot, lfa_flags, table, routes_dev, tilfa_dev, cap_entries, out_dev, out_total);
}

// ---- two-segment repair paths (include/holo_spf_hip.h "two-segment repair paths on device"; kernels: spf_tilfa.hip.h) ----
int hspf_tilfa_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                      const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                      const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                      const uint8_t *space_flags_dev, const uint32_t *space_via_dev, hspf_tilfa_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  (void)lfa_flags;                                      // (eligibility and the overload rule are in the space tables)
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_tilfa_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, g && rdist_dev, "NULL graph, table, prot or out pointer"))) return rc;
    if (!space_flags_dev || !space_via_dev) return f.bad("NULL space_flags / space_via (the tables of hspf_rlfa_device are required)");
    if (!out_dev->ti_kind || !out_dev->ti_p || !out_dev->ti_q || !out_dev->ti_via || !out_dev->ti_link || !out_dev->ti_metric || !out_dev->ti_counts ||
        !out_dev->td_kind || !out_dev->td_coverage)
      return f.bad("NULL ti_kind / ti_p / ti_q / ti_via / ti_link / ti_metric / ti_counts / td_kind / td_coverage");
    if ((rc = f.check_dims()) || (rc = f.check_graph(g))) return rc;
    if (n_vertices > 0x7FFFFFFFu) return f.bad("n_vertices does not fit the selection key");
    if ((rc = f.check_slots()) || (rc = f.check_twoway(g)) || (rc = f.stage(FrrProt::Plain, nullptr, nullptr)) ||
        (rc = ensure(ctx, ctx->tilfa_key, f.n_slots * 8, false)) || (rc = f.stage_twoway(g))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(ctx->tilfa_key.p, 0xFF, f.n_slots * 8, s));
    HIPCHK(ctx, hipMemsetAsync(out_dev->ti_counts, 0, f.n_slots * HSPF_TILFA_COUNT_WORDS * 4, s));
    HIPCHK(ctx, hipMemsetAsync(out_dev->td_coverage, 0, (size_t)n_prot * HSPF_TILFA_COVERAGE_WORDS * 4, s));
    TilfaArgs a{};
    a.n = n_vertices; a.W = n_mask_words; a.stride = (uint32_t)f.stride;
    a.dist = dist_dev; a.rdist = rdist_dev; a.flags = flags_dev; a.mask = mask_dev;
    a.tab = (const uint32_t *)ctx->lfa_tab.p; a.alt_in = alt_flags_in_dev;
    a.sflags = space_flags_dev; a.svia = space_via_dev;
    a.row_ptr = g->d_row_ptr[g->cur]; a.col = g->d_col[g->cur]; a.metric = g->d_metric[g->cur]; a.tw = (const uint8_t *)ctx->tilfa_tw.p;
    a.key = (unsigned long long *)ctx->tilfa_key.p;
    a.ti_kind = out_dev->ti_kind; a.ti_p = out_dev->ti_p; a.ti_q = out_dev->ti_q; a.ti_via = out_dev->ti_via; a.ti_link = out_dev->ti_link;
    a.ti_metric = out_dev->ti_metric; a.ti_counts = out_dev->ti_counts; a.td_kind = out_dev->td_kind; a.td_cov = out_dev->td_coverage;
    const uint32_t n_tiles = (n_vertices + LFA_TILE - 1) / LFA_TILE;
    if (f.max_k) hipLaunchKernelGGL(k_tilfa, dim3(n_tiles, std::min(f.max_k, 65535u), n_prot), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_tilfa_final, dim3((uint32_t)((f.n_slots + 255) / 256)), dim3(256), 0, s, a, n_prot);
    hipLaunchKernelGGL(k_tilfa_dest, dim3(n_tiles, n_prot), dim3(256), 0, s, a);
    return f.finish("k_tilfa");
  });
}

// ---- TI-LFA along the post-convergence path (include/holo_spf_hip.h "repairs along the post-convergence path"; kernels: spf_tilfa_pc.hip.h) ----
static_assert(TIPC_MAX_ADJ == HSPF_TIPC_MAX_ADJ && TIPC_COV == HSPF_TIPC_COVERAGE_WORDS && TIPC_LFA == HSPF_TIPC_D_LFA && TIPC_REPAIR == HSPF_TIPC_D_REPAIR &&
              TIPC_NONE == HSPF_TIPC_D_NONE && TIPC_LONG == HSPF_TIPC_D_LONG && TIPC_LAN == HSPF_TIPC_D_LAN && TIPC_WALK == HSPF_TIPC_D_WALK &&
              TIPC_F_ON_PC == HSPF_TIPC_ON_PC && TIPC_F_P_IS_ROOT == HSPF_TIPC_P_IS_ROOT && TIPC_F_Q_IS_DEST == HSPF_TIPC_Q_IS_DEST &&
              TIPC_SRC_NT == hspf::SRC_NO_TRANSIT && TIPC_SRC_MASK == hspf::SRC_MASK, "the kernels' constants are the header's and the graph's");

int hspf_tilfa_pc_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                         const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                         const uint8_t *space_flags_dev, const uint32_t *space_via_dev, const uint32_t *pc_dist_dev, uint32_t n_pc_rows,
                         const uint32_t *pc_row, uint32_t run_flags, uint32_t max_walk, hspf_tilfa_pc_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  (void)lfa_flags;                                      // (eligibility and the overload rule of the spaces are in the space tables)
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_tilfa_pc_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, g && rdist_dev, "NULL graph, table, prot or out pointer"))) return rc;
    if (!space_flags_dev || !space_via_dev) return f.bad("NULL space_flags / space_via (the tables of hspf_rlfa_device are required)");
    if (!pc_dist_dev || !pc_row) return f.bad("NULL pc_dist / pc_row (the rows of hspf_run_failures_device are required)");
    if (!out_dev->tp_kind || !out_dev->tp_p || !out_dev->tp_via || !out_dev->tp_q || !out_dev->tp_n_adj || !out_dev->tp_hop_pos || !out_dev->tp_hop_head ||
        !out_dev->tp_metric || !out_dev->tp_flags || !out_dev->tp_coverage)
      return f.bad("NULL tp_kind / tp_p / tp_via / tp_q / tp_n_adj / tp_hop_pos / tp_hop_head / tp_metric / tp_flags / tp_coverage");
    if ((rc = f.check_dims()) || (rc = f.check_graph(g))) return rc;
    if (max_walk == 0 || max_walk > 65535u) return f.bad("max_walk outside 1 .. 65535");
    if ((rc = f.check_slots())) return rc;
    // the rows: given for candidate slots only, inside pc_dist; the staged block prow | pidx | plist
    std::vector<uint32_t> &pt = f.mtab;
    pt.assign(2 * f.n_slots, LFA_NONE);
    for (uint32_t i = 0; i < n_prot; ++i) {
      const hspf_lfa_protect &p = prot[i];
      const std::string who = "protected root " + std::to_string(i) + ": ";
      if (p.n_slots > f.stride) return f.bad(who + "n_slots > 64 * n_mask_words");      // (before nbr is read that far)
      if (p.n_slots && !p.nbr) return f.bad(who + "NULL slot array");
      for (uint32_t e = 0; e < f.stride; ++e) {
        const size_t s = (size_t)i * f.stride + e;
        const uint32_t r = pc_row[s];
        if (r == HSPF_NO_ROOT) continue;
        if (e >= p.n_slots || p.nbr[e] == HSPF_NO_ROOT) return f.bad(who + "pc_row given for slot " + std::to_string(e) + ", which is no candidate");
        if (r >= n_pc_rows) return f.bad(who + "pc_row of slot " + std::to_string(e) + " >= n_pc_rows");
        pt[s] = r; pt[f.n_slots + s] = (uint32_t)(pt.size() - 2 * f.n_slots); pt.push_back((uint32_t)s);
      }
    }
    const size_t n_pairs = pt.size() - 2 * f.n_slots;
    void *par = nullptr;
    if ((rc = f.stage(FrrProt::Plain, nullptr, nullptr)) || (rc = ensure(ctx, ctx->tipc_tab, pt.size() * 4, false)) ||
        (rc = f.scratch(n_pairs * n_vertices * sizeof(uint2), &par))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemcpyAsync(ctx->tipc_tab.p, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(out_dev->tp_coverage, 0, (size_t)n_prot * HSPF_TIPC_COVERAGE_WORDS * 4, s));
    TipcArgs a{};
    a.n = n_vertices; a.W = n_mask_words; a.stride = (uint32_t)f.stride; a.ignore_overload = (run_flags & HSPF_RUN_IGNORE_OVERLOAD) ? 1u : 0u;
    a.max_walk = max_walk; a.n_pairs = (uint32_t)n_pairs;
    a.dist = dist_dev; a.flags = flags_dev; a.mask = mask_dev;
    a.tab = (const uint32_t *)ctx->lfa_tab.p; a.alt_in = alt_flags_in_dev;
    a.sflags = space_flags_dev; a.svia = space_via_dev; a.pc_dist = pc_dist_dev;
    a.prow = (const uint32_t *)ctx->tipc_tab.p; a.pidx = a.prow + f.n_slots; a.plist = a.pidx + f.n_slots;
    a.in_ptr = g->d_in_ptr; a.in_src = g->d_in_src; a.in_w = g->d_in_w; a.in_fpos = g->d_in_fpos; a.vflags = g->d_vflags;
    a.par = (uint2 *)par;
    a.tp_kind = out_dev->tp_kind; a.tp_n_adj = out_dev->tp_n_adj; a.tp_flags = out_dev->tp_flags; a.tp_p = out_dev->tp_p; a.tp_via = out_dev->tp_via;
    a.tp_q = out_dev->tp_q; a.tp_hop_pos = out_dev->tp_hop_pos; a.tp_hop_head = out_dev->tp_hop_head; a.tp_metric = out_dev->tp_metric;
    a.tp_cov = out_dev->tp_coverage;
    const uint32_t n_tiles = (n_vertices + LFA_TILE - 1) / LFA_TILE;
    if (n_pairs) hipLaunchKernelGGL(k_tipc_parent, dim3(n_tiles, (uint32_t)std::min<size_t>(n_pairs, 65535)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_tipc_walk, dim3(n_tiles, n_prot), dim3(256), 0, s, a);
    return f.finish("k_tipc_walk");
  });
}

// ---- per-prefix backup routes (include/holo_spf_hip.h "per-prefix backup routes on device"; kernels: spf_backup.hip.h) ----
int hspf_routes_backup_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                              const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                              const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const hspf_prefix_table *t,
                              const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev, hspf_backup_out *out_dev) {
  return routes_backup(ctx, "hspf_routes_backup_device", FrrProt::Plain, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, nullptr,
                       nullptr, n_prot, lfa_flags, t, routes_dev, tilfa_dev, out_dev);
}

int hspf_routes_backup_ecmp_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                   const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                   const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const hspf_prefix_table *table,
                                   const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev, uint64_t cap_entries,
                                   hspf_backup_ecmp_out *out_dev, uint64_t *out_total) {
  return backup_ecmp_call(ctx, "hspf_routes_backup_ecmp_device", FrrProt::Plain, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, nullptr, n_prot,
                          lfa_flags, table, routes_dev, tilfa_dev, cap_entries, out_dev, out_total);
}

int hspf_routes_backup_lan_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                  const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                  const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, uint32_t lfa_flags,
                                  const hspf_prefix_table *t, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev,
                                  hspf_backup_out *out_dev) {
  return routes_backup(ctx, "hspf_routes_backup_lan_device", FrrProt::Lan, n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, lan,
                       nullptr, n_prot, lfa_flags, t, routes_dev, tilfa_dev, out_dev);
}

// ---- node-protecting remote LFA (include/holo_spf_hip.h "node-protecting remote loop-free alternates on device"; kernels:
// spf_rlfa_node.hip.h) ----
int hspf_rlfa_node_select_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                 const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                 const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *space_flags_dev,
                                 uint32_t max_pq, hspf_rlfa_node_sel *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_rlfa_node_select_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev))) return rc;
    if (!space_flags_dev) return f.bad("NULL space_flags (the table of hspf_rlfa_device is required)");
    if ((rc = f.check_rn_sel(out_dev, max_pq, "")) || (rc = f.check_dims()) || (rc = f.check_slots()) || (rc = f.stage(FrrProt::Plain, nullptr, nullptr))) return rc;
    const uint32_t n_tiles = (n_vertices + LFA_TILE - 1) / LFA_TILE, max_k = f.max_k;
    const size_t part_keys = (size_t)n_prot * max_k * n_tiles * max_pq;      // one list per workgroup
    if (part_keys > ((size_t)1 << 30)) { ctx->last_error = std::string(f.fn) + ": the partial lists of this call need more than 8 GiB of scratch"; return HSPF_E_NOMEM; }
    if ((rc = ensure(ctx, ctx->rnode_part, std::max<size_t>(part_keys, 1) * 8, false))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(out_dev->nq_count, 0, f.n_slots * 4, s));
    RnodeSelArgs a{};
    a.n = n_vertices; a.stride = (uint32_t)f.stride; a.ignore_overload = (lfa_flags & HSPF_LFA_IGNORE_OVERLOAD) ? 1u : 0u; a.max_pq = max_pq;
    a.max_k = max_k; a.n_tiles = n_tiles;
    a.dist = dist_dev; a.tab = (const uint32_t *)ctx->lfa_tab.p; a.sflags = space_flags_dev;
    a.part = (unsigned long long *)ctx->rnode_part.p;
    a.nq_node = out_dev->nq_node; a.nq_via = out_dev->nq_via; a.nq_metric = out_dev->nq_metric; a.nq_count = out_dev->nq_count;
    if (max_k) hipLaunchKernelGGL(k_rlfa_nsel, dim3(n_tiles, std::min(max_k, 65535u), n_prot), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_rlfa_nsel_final, dim3((uint32_t)f.stride, n_prot), dim3(64), 0, s, a);
    return f.finish("k_rlfa_nsel");
  });
}

int hspf_rlfa_node_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                          const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                          const hspf_lfa_protect *prot, uint32_t n_prot,
                          const uint32_t *ydist_dev, const uint32_t *y_roots, uint32_t n_yrows,
                          const hspf_rlfa_node_sel *sel_dev, uint32_t max_pq,
                          const uint8_t *alt_flags_in_dev, hspf_rlfa_node_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_rlfa_node_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev))) return rc;
    if (!ydist_dev || !y_roots || !sel_dev) return f.bad("NULL ydist, y_roots or sel pointer");
    if ((rc = f.check_rn_sel(sel_dev, max_pq, " in sel_dev"))) return rc;
    if (!out_dev->nd_kind || !out_dev->nd_node || !out_dev->nd_via || !out_dev->nd_metric || !out_dev->nd_coverage)
      return f.bad("NULL nd_kind / nd_node / nd_via / nd_metric / nd_coverage");
    if ((rc = f.check_dims()) || (rc = f.check_slots()) || (rc = f.check_y_roots(y_roots, n_yrows)) || (rc = f.stage(FrrProt::Plain, nullptr, nullptr)) ||
        (rc = f.node_map(y_roots, n_yrows))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(out_dev->nd_coverage, 0, (size_t)n_prot * HSPF_NP_COVERAGE_WORDS * 4, s));
    RnodeDestArgs a{};
    a.n = n_vertices; a.W = n_mask_words; a.stride = 64u * n_mask_words; a.max_pq = max_pq;
    a.dist = dist_dev; a.flags = flags_dev; a.mask = mask_dev; a.tab = (const uint32_t *)ctx->lfa_tab.p;
    a.ydist = ydist_dev; a.yroots = f.ymap + n_vertices; a.n_yrows = n_yrows; a.ymap = f.ymap;
    a.nq_node = sel_dev->nq_node; a.nq_via = sel_dev->nq_via; a.nq_metric = sel_dev->nq_metric; a.nq_count = sel_dev->nq_count;
    a.alt_in = alt_flags_in_dev;
    a.nd_kind = out_dev->nd_kind; a.nd_node = out_dev->nd_node; a.nd_via = out_dev->nd_via; a.nd_metric = out_dev->nd_metric;
    a.nd_set = out_dev->nd_set; a.nd_cov = out_dev->nd_coverage;
    f.launch_node_map();
    hipLaunchKernelGGL(k_rlfa_ndest, dim3((n_vertices + LFA_TILE - 1) / LFA_TILE, n_prot), dim3(256), 0, s, a);
    return f.finish("k_rlfa_ndest");
  });
}

// ---- two-segment node-protecting repairs (include/holo_spf_hip.h "two-segment node-protecting repairs on device"; kernels:
// spf_tilfa_node.hip.h) ----
static_assert(TNODE_MAX_PAIRS == HSPF_TILFA_NODE_MAX_PAIRS, "the kernels' list length is the header's");

int hspf_tilfa_node_select_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                  const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                  const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *space_flags_dev,
                                  uint32_t max_pairs, hspf_tilfa_node_sel *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_tilfa_node_select_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, g, "NULL graph, table, prot or out pointer"))) return rc;
    if (!space_flags_dev) return f.bad("NULL space_flags (the table of hspf_rlfa_device is required)");
    if ((rc = f.check_tn_sel(out_dev, max_pairs, "")) || (rc = f.check_dims()) || (rc = f.check_graph(g)) || (rc = f.check_slots()) ||
        (rc = f.check_twoway(g)) || (rc = f.stage(FrrProt::Plain, nullptr, nullptr))) return rc;
    const uint32_t n_tiles = (n_vertices + LFA_TILE - 1) / LFA_TILE, max_k = f.max_k;
    const size_t cells = (size_t)n_prot * max_k * n_vertices;                  // one per (root, candidate, vertex): not tiled
    const size_t part_keys = (size_t)n_prot * max_k * n_tiles * max_pairs;     // one list per workgroup
    if (cells > ((size_t)1 << 30)) {
      ctx->last_error = std::string(f.fn) + ": the cells of this call (8 bytes x slots x n_vertices per protected root) need more than 8 GiB of scratch: split prot";
      return HSPF_E_NOMEM;
    }
    if ((rc = ensure(ctx, ctx->tnode_cell, std::max<size_t>(cells, 1) * 8, false)) ||
        (rc = ensure(ctx, ctx->rnode_part, std::max<size_t>(part_keys, 1) * 8, false)) || (rc = f.stage_twoway(g))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(ctx->tnode_cell.p, 0xFF, std::max<size_t>(cells, 1) * 8, s));
    HIPCHK(ctx, hipMemsetAsync(out_dev->tq_count, 0, f.n_slots * 4, s));
    TnSelArgs a{};
    a.r.n = n_vertices; a.r.stride = (uint32_t)f.stride; a.r.ignore_overload = (lfa_flags & HSPF_LFA_IGNORE_OVERLOAD) ? 1u : 0u; a.r.max_pq = max_pairs;
    a.r.max_k = max_k; a.r.n_tiles = n_tiles;
    a.r.dist = dist_dev; a.r.tab = (const uint32_t *)ctx->lfa_tab.p; a.r.sflags = space_flags_dev;
    a.r.part = (unsigned long long *)ctx->rnode_part.p;
    a.row_ptr = g->d_row_ptr[g->cur]; a.col = g->d_col[g->cur]; a.metric = g->d_metric[g->cur]; a.tw = (const uint8_t *)ctx->tilfa_tw.p;
    a.cell = (unsigned long long *)ctx->tnode_cell.p;
    a.tq_q = out_dev->tq_q; a.tq_p = out_dev->tq_p; a.tq_link = out_dev->tq_link; a.tq_via = out_dev->tq_via; a.tq_metric = out_dev->tq_metric;
    a.tq_count = out_dev->tq_count;
    if (max_k) {
      const dim3 grid(n_tiles, std::min(max_k, 65535u), n_prot);
      hipLaunchKernelGGL(k_tn_link, grid, dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_tn_sel, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_tn_sel_final, dim3((uint32_t)f.stride, n_prot), dim3(64), 0, s, a);
    return f.finish("k_tn_link");
  });
}

int hspf_tilfa_node_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                           const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                           const hspf_lfa_protect *prot, uint32_t n_prot,
                           const uint32_t *ydist_dev, const uint32_t *y_roots, uint32_t n_yrows,
                           const hspf_tilfa_node_sel *sel_dev, uint32_t max_pairs,
                           const uint8_t *alt_flags_in_dev, const uint8_t *nd_kind_in_dev, hspf_tilfa_node_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_tilfa_node_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev))) return rc;
    if (!ydist_dev || !y_roots || !sel_dev) return f.bad("NULL ydist, y_roots or sel pointer");
    if ((rc = f.check_tn_sel(sel_dev, max_pairs, " in sel_dev"))) return rc;
    if (!out_dev->tn_kind || !out_dev->tn_p || !out_dev->tn_q || !out_dev->tn_link || !out_dev->tn_via || !out_dev->tn_metric || !out_dev->tn_coverage)
      return f.bad("NULL tn_kind / tn_p / tn_q / tn_link / tn_via / tn_metric / tn_coverage");
    if ((rc = f.check_dims()) || (rc = f.check_slots()) || (rc = f.check_y_roots(y_roots, n_yrows)) || (rc = f.stage(FrrProt::Plain, nullptr, nullptr)) ||
        (rc = f.node_map(y_roots, n_yrows))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(out_dev->tn_coverage, 0, (size_t)n_prot * HSPF_TN_COVERAGE_WORDS * 4, s));
    TnDestArgs a{};
    a.n = n_vertices; a.W = n_mask_words; a.stride = 64u * n_mask_words; a.max_pairs = max_pairs;
    a.dist = dist_dev; a.flags = flags_dev; a.mask = mask_dev; a.tab = (const uint32_t *)ctx->lfa_tab.p;
    a.ydist = ydist_dev; a.ymap = f.ymap;
    a.tq_q = sel_dev->tq_q; a.tq_p = sel_dev->tq_p; a.tq_link = sel_dev->tq_link; a.tq_via = sel_dev->tq_via; a.tq_metric = sel_dev->tq_metric;
    a.tq_count = sel_dev->tq_count;
    a.alt_in = alt_flags_in_dev; a.nd_in = nd_kind_in_dev;
    a.tn_kind = out_dev->tn_kind; a.tn_p = out_dev->tn_p; a.tn_q = out_dev->tn_q; a.tn_link = out_dev->tn_link; a.tn_via = out_dev->tn_via;
    a.tn_metric = out_dev->tn_metric; a.tn_set = out_dev->tn_set; a.tn_cov = out_dev->tn_coverage;
    f.launch_node_map();
    hipLaunchKernelGGL(k_tn_dest, dim3((n_vertices + LFA_TILE - 1) / LFA_TILE, n_prot), dim3(256), 0, s, a);
    return f.finish("k_tn_dest");
  });
}

// ---- per-prefix node-protecting backups (include/holo_spf_hip.h "per-prefix node-protecting backups on device"; kernel:
// spf_backup_node.hip.h) ----
static_assert(BN_CW == HSPF_BN_COVERAGE_WORDS, "the kernel's count width is the header's");
static_assert(BN_LFA == HSPF_BN_LFA && BN_PQ == HSPF_BN_PQ && BN_LAST_HOP == HSPF_BN_LAST_HOP && BN_NONE == HSPF_BN_NONE && BN_PAIR == HSPF_BN_PAIR &&
              BN_PAIR < BN_CW && BN_BK_LFA == HSPF_BK_LFA && BN_NODE_PROTECT == HSPF_LFA_NODE_PROTECT, "the kernel's kinds and bits are the header's");

int hspf_routes_backup_node_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                   const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                   const hspf_lfa_protect *prot, uint32_t n_prot,
                                   const hspf_prefix_table *t, const hspf_routes *routes_dev,
                                   const uint32_t *ydist_dev, const uint32_t *y_roots, uint32_t n_yrows,
                                   const hspf_rlfa_node_sel *rn_sel_dev, uint32_t max_pq,
                                   const hspf_tilfa_node_sel *tn_sel_dev, uint32_t max_pairs,
                                   const hspf_backup_out *bk_in_dev, hspf_backup_node_out *out_dev) {
  if (!ctx) return HSPF_E_INVAL;
  return guarded(ctx, [&]() -> int {
    FrrCall f(ctx, "hspf_routes_backup_node_device", n_vertices, n_rows, n_mask_words, dist_dev, flags_dev, mask_dev, prot, n_prot);
    int rc;
    if ((rc = f.check_ptrs(out_dev, t && routes_dev, "NULL table, prot, prefix table, routes or out pointer")) || (rc = f.check_routes(routes_dev))) return rc;
    if (!out_dev->bn_kind || !out_dev->bn_primary || !out_dev->bn_p || !out_dev->bn_q || !out_dev->bn_link || !out_dev->bn_via || !out_dev->bn_metric ||
        !out_dev->bn_coverage)
      return f.bad("NULL bn_kind / bn_primary / bn_p / bn_q / bn_link / bn_via / bn_metric / bn_coverage");
    if (!ydist_dev || !y_roots) return f.bad("NULL ydist or y_roots pointer");
    if (!rn_sel_dev && !tn_sel_dev) return f.bad("NULL rn_sel_dev and tn_sel_dev (at least one list is required)");
    if ((rn_sel_dev && (rc = f.check_rn_sel(rn_sel_dev, max_pq, " in rn_sel_dev"))) || (tn_sel_dev && (rc = f.check_tn_sel(tn_sel_dev, max_pairs, " in tn_sel_dev"))))
      return rc;
    if (bk_in_dev && (!bk_in_dev->bk_kind || !bk_in_dev->bk_flags)) return f.bad("NULL bk_kind / bk_flags in bk_in_dev");
    if ((rc = f.check_dims()) || (rc = f.check_prefix_table(t)) || (rc = f.check_slots()) || (rc = f.check_y_roots(y_roots, n_yrows)) ||
        (rc = f.stage_prefix_table(t)) || (rc = f.stage(FrrProt::Plain, nullptr, nullptr))) return rc;
    hipStream_t s = f.stream();
    HIPCHK(ctx, hipMemsetAsync(out_dev->bn_coverage, 0, (size_t)n_prot * HSPF_BN_COVERAGE_WORDS * 4, s));
    if (!t->n_prefixes) return f.finish(nullptr);       // nothing to launch
    if ((rc = f.node_map(y_roots, n_yrows))) return rc;
    BackupNodeArgs a{};
    a.n = n_vertices; a.W = n_mask_words; a.stride = 64u * n_mask_words; a.n_pfx = t->n_prefixes;
    a.sat = (t->flags & HSPF_PFX_SATURATING) ? 1u : 0u; a.max_pq = rn_sel_dev ? max_pq : 0u; a.max_pairs = tn_sel_dev ? max_pairs : 0u;
    a.dist = dist_dev; a.flags = flags_dev; a.tab = (const uint32_t *)ctx->lfa_tab.p;
    a.pfx_ptr = (const uint32_t *)ctx->pf_ptr.p; a.pfx_vertex = (const uint32_t *)ctx->pf_vtx.p; a.pfx_metric = (const uint32_t *)ctx->pf_met.p;
    a.best_entry = routes_dev->best_entry; a.nh_mask = routes_dev->nexthop_mask;
    a.ydist = ydist_dev; a.ymap = f.ymap;
    if (rn_sel_dev) { a.nq_node = rn_sel_dev->nq_node; a.nq_via = rn_sel_dev->nq_via; a.nq_metric = rn_sel_dev->nq_metric; a.nq_count = rn_sel_dev->nq_count; }
    if (tn_sel_dev) {
      a.tq_q = tn_sel_dev->tq_q; a.tq_p = tn_sel_dev->tq_p; a.tq_link = tn_sel_dev->tq_link; a.tq_via = tn_sel_dev->tq_via;
      a.tq_metric = tn_sel_dev->tq_metric; a.tq_count = tn_sel_dev->tq_count;
    }
    if (bk_in_dev) { a.bk_kind_in = bk_in_dev->bk_kind; a.bk_flags_in = bk_in_dev->bk_flags; }
    a.bn_kind = out_dev->bn_kind; a.bn_primary = out_dev->bn_primary; a.bn_p = out_dev->bn_p; a.bn_q = out_dev->bn_q; a.bn_link = out_dev->bn_link;
    a.bn_via = out_dev->bn_via; a.bn_metric = out_dev->bn_metric; a.bn_set_pq = out_dev->bn_set_pq; a.bn_set_pair = out_dev->bn_set_pair;
    a.bn_cov = out_dev->bn_coverage;
    f.launch_node_map();
    hipLaunchKernelGGL(k_backup_node, dim3((t->n_prefixes + LFA_TILE - 1) / LFA_TILE, n_prot), dim3(256), 0, s, a);
    return f.finish("k_backup_node");
  });
}

}  // extern "C"
