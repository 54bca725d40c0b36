// spf_backup_node.hip.h — per-prefix node-protecting backups: the listed PQ nodes of hspf_rlfa_node_select_device and the listed
// q's of hspf_tilfa_node_select_device tested against their distance to the PREFIX (the minimum over its advertisers), from the
// forward SPT rows rooted at them (hspf_routes_backup_node_device; the semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  That of k_backup: lane = prefix, 256 consecutive prefixes per workgroup, blockIdx.y = the protected root; the route is
// read and every output is written coalesced.  d_E(p) of the one primary is computed once, in front of the lists.  A list is walked
// in chunks of BN_CH entries: per chunk the lane keeps the rows and d_Y(p) of its BN_CH listed nodes in registers (the loops over
// a chunk are unrolled: no dynamically indexed private array, no scratch) and streams the prefix's entries ONCE — per entry (v, m)
// one gather ydist[row_j][v] per entry of the chunk.  Unlike k_backup the rows are NOT wave-uniform: the list belongs to the
// lane's own primary slot, so neighbouring lanes share a row only where they share the slot (prefixes behind one neighbour
// usually do, and then the gathers of a wave differ in v alone).
//   k_backup_node   everything: the two lists, the choice, the six counts (frr_cover: ballots, one LDS add per wave, one vector
//                   atomic add per workgroup and counter).
// The vertex -> row map of the listed nodes is k_rlfa_nmap's.  There is no wave-per-prefix path: a prefix with very many
// advertisers is walked by ONE lane and holds its wave back.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_backup.hip.h"
#include "spf_tilfa_node.hip.h"

namespace {

constexpr uint32_t BN_CH = BK_CH;                  // list entries per chunk
constexpr uint32_t BN_CW = 6;                      // HSPF_BN_COVERAGE_WORDS
// the header's numbers (spf_frr.hip.h holds each against its macro)
constexpr uint32_t BN_LFA = 1, BN_PQ = 2, BN_LAST_HOP = 3, BN_NONE = 4, BN_PAIR = 5;      // HSPF_BN_*
constexpr uint32_t BN_BK_LFA = 3;                  // HSPF_BK_LFA (bk_kind of hspf_routes_backup_device)
constexpr uint32_t BN_NODE_PROTECT = 0x08;         // HSPF_LFA_NODE_PROTECT (its bk_flags)

struct BackupNodeArgs {
  uint32_t n, W, stride, n_pfx;                                            // stride = 64 * W slots per protected root
  uint32_t sat, max_pq, max_pairs, pad0;
  const uint32_t *dist; const uint16_t *flags;                             // the forward table set
  const uint32_t *tab;                                                     // the staged candidate tables
  const uint32_t *pfx_ptr, *pfx_vertex, *pfx_metric;                       // the staged prefix table
  const uint32_t *best_entry; const uint64_t *nh_mask;                     // hspf_routes of the same table set
  const uint32_t *ydist, *ymap;                                            // [n_yrows][n] rows rooted at listed nodes; vertex -> row (k_rlfa_nmap)
  const uint32_t *nq_node, *nq_via, *nq_metric, *nq_count;                 // hspf_rlfa_node_sel, or all NULL
  const uint32_t *tq_q, *tq_p, *tq_link, *tq_via, *tq_metric, *tq_count;   // hspf_tilfa_node_sel, or all NULL
  const uint8_t *bk_kind_in, *bk_flags_in;                                 // [n_prot][n_pfx] of hspf_routes_backup_device, or both NULL
  uint8_t *bn_kind; uint32_t *bn_primary, *bn_p, *bn_q, *bn_link, *bn_via, *bn_metric, *bn_set_pq, *bn_set_pair, *bn_cov;
};

// One list (node[j], metric[j], j < L, at `lb`) against prefix entries lo .. hi: bit j of `set` = entry j protects; the smallest
// metric[j] + d_Y(p) among them, then the smaller j.  dEp is a number.
__device__ __forceinline__ void bn_walk(const BackupNodeArgs &a, const uint32_t *node, const uint32_t *metric, size_t lb, uint32_t L,
                                        uint32_t lo, uint32_t hi, uint32_t E, uint64_t dEp, uint32_t &set, uint64_t &best, uint32_t &bj) {
  const uint32_t n = a.n;
  set = 0; best = ~0ull; bj = 0;
  for (uint32_t c0 = 0; c0 < L; c0 += BN_CH) {
    uint32_t row[BN_CH];
    uint64_t dYp[BN_CH];
#pragma unroll
    for (uint32_t j = 0; j < BN_CH; ++j) {
      row[j] = LFA_NONE; dYp[j] = BK_NO_DIST;
      if (c0 + j < L) {
        const uint32_t Y = node[lb + c0 + j];
        if (Y < n) row[j] = a.ymap[Y];                                             // a listed node without a row is skipped
      }
    }
    for (uint32_t e = lo; e < hi; ++e) {
      const uint32_t v = a.pfx_vertex[e], met = a.pfx_metric[e];
#pragma unroll
      for (uint32_t j = 0; j < BN_CH; ++j) {
        if (row[j] == LFA_NONE) continue;
        const uint32_t d = a.ydist[(size_t)row[j] * n + v];
        if (d == LFA_NONE) continue;
        uint64_t t = (uint64_t)d + met;
        if (a.sat && t > 0xFFFFFFFFull) t = 0xFFFFFFFFull;
        dYp[j] = t < dYp[j] ? t : dYp[j];
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < BN_CH; ++j) {
      if (row[j] == LFA_NONE || dYp[j] == BK_NO_DIST) continue;
      const uint32_t dYE = a.ydist[(size_t)row[j] * n + E];
      if (dYE == LFA_NONE || !(dYp[j] < (uint64_t)dYE + dEp)) continue;
      set |= 1u << (c0 + j);
      const uint64_t tot = (uint64_t)metric[lb + c0 + j] + dYp[j];
      if (tot < best) { best = tot; bj = c0 + j; }                                  // ascending j: a tie keeps the smaller j
    }
  }
}

__global__ __launch_bounds__(256) void k_backup_node(BackupNodeArgs a) {
  __shared__ uint32_t s_cov[BN_CW];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  if (tid < BN_CW) s_cov[tid] = 0;
  __syncthreads();
  const uint32_t p = blockIdx.x * LFA_TILE + tid;
  const bool valid = p < a.n_pfx;
  const size_t oi = (size_t)tb.srow * a.n_pfx + (valid ? p : 0u), oo = (size_t)pi * a.n_pfx + p;
  uint32_t kind = 0, prim = LFA_NONE, bp = LFA_NONE, bq = LFA_NONE, link = LFA_NONE, via = LFA_NONE, met = 0, set_pq = 0, set_pair = 0;
  uint32_t np = 0, p0 = 0;
  if (valid && a.best_entry[oi] != LFA_NONE) frr_primaries(tb, a.nh_mask + oi * a.W, np, p0);
  if (np == 1) {
    prim = p0;
    const uint32_t E = tb.nbr[p0];
    if (a.bk_kind_in && a.bk_kind_in[oo] == BN_BK_LFA && (a.bk_flags_in[oo] & BN_NODE_PROTECT)) kind = BN_LFA;
    else if (E == LFA_NONE) kind = BN_NONE;
    else {
      const uint32_t lo = a.pfx_ptr[p], hi = a.pfx_ptr[p + 1];
      const size_t so = (size_t)pi * a.stride + p0;
      bool own;
      const uint64_t dEp = bk_dist_to_prefix(a, tb.row[p0], lo, hi, E, &own);        // (from the forward set; own: E's own entry attains it)
      if (dEp != BK_NO_DIST) {
        uint64_t best;
        uint32_t bj;
        if (a.nq_node) {
          const uint32_t cnt = a.nq_count[so], L = cnt < a.max_pq ? cnt : a.max_pq;
          bn_walk(a, a.nq_node, a.nq_metric, so * a.max_pq, L, lo, hi, E, dEp, set_pq, best, bj);
          if (set_pq) {
            const size_t ob = so * a.max_pq + bj;
            kind = BN_PQ; bp = bq = a.nq_node[ob]; via = a.nq_via[ob];
            met = (uint32_t)(best > RNODE_SAT ? RNODE_SAT : best);
          }
        }
        if (a.tq_q && (!set_pq || a.bn_set_pair)) {                                // a one-segment repair stands before any pair
          const uint32_t cnt = a.tq_count[so], L = cnt < a.max_pairs ? cnt : a.max_pairs;
          bn_walk(a, a.tq_q, a.tq_metric, so * a.max_pairs, L, lo, hi, E, dEp, set_pair, best, bj);
          if (set_pair && !set_pq) {
            const size_t ob = so * a.max_pairs + bj;
            kind = BN_PAIR; bp = a.tq_p[ob]; bq = a.tq_q[ob]; link = a.tq_link[ob]; via = a.tq_via[ob];
            met = (uint32_t)(best > RNODE_SAT ? RNODE_SAT : best);
          }
        }
      }
      if (!kind) kind = (dEp != BK_NO_DIST && own) ? BN_LAST_HOP : BN_NONE;                      // the entries are tested BEFORE the last-hop class
    }
  }
  if (valid) {
    a.bn_kind[oo] = (uint8_t)kind; a.bn_primary[oo] = prim; a.bn_p[oo] = bp; a.bn_q[oo] = bq; a.bn_link[oo] = link; a.bn_via[oo] = via;
    a.bn_metric[oo] = met;
    if (a.bn_set_pq) a.bn_set_pq[oo] = set_pq;
    if (a.bn_set_pair) a.bn_set_pair[oo] = set_pair;
  }
  frr_cover<BN_CW>(kind ? 1u | (1u << kind) : 0u, s_cov, a.bn_cov + (size_t)pi * BN_CW);   // counter 0: any class; counter j: class j (1 .. 5)
}

}  // namespace
