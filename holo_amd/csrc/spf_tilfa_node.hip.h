// spf_tilfa_node.hip.h — two-segment node-protecting repairs (TI-LFA node protection): per (protected root S, protected slot e)
// the cheapest few routers q of the Q-space that a forced adjacency p -> q enters from a node p of the extended P-space whose
// release path avoids the NODE E behind the slot (hspf_tilfa_node_select_device), and per destination the cheapest of them whose
// own shortest path to the destination avoids E too, from the forward SPT rows rooted at those q (hspf_tilfa_node_device; the
// semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  As k_tilfa / k_rlfa_nsel: lane = vertex, 256 consecutive vertices per workgroup; the candidate slots of a root are the
// grid's y axis, the protected roots its z axis.  The unit that is listed is q, but links are found from p:
//   k_tn_link       lane = p.  Per slot the lane loads space_flags[e][p] (coalesced); a lane outside the extended P-space is done
//                   (a wave without one does no row walk at all).  The others find their node-avoiding release point (rnode_release of
//                   spf_rlfa_node.hip.h) and walk p's row of the raw CSR as k_tilfa does; every qualifying link issues ONE vector
//                   64-bit atomicMin of (saturated relN(p) + w) << 32 | p into the call's cell of (S, candidate, q).  The cells are
//                   set to all-ones by the call; a minimum does not depend on the order of its operands.  The link position is not
//                   in the key: k_tn_sel_final finds it again in p's row.
//   k_tn_sel        lane = q.  The key (entry metric << 32 | q) is unique per q; the cheapest max_pairs of the workgroup and the
//                   count by k_rlfa_nsel's own extraction (rnode_block_top), into [root][candidate][tile][max_pairs], all-ones
//                   padded: every cell is written.
//   k_tn_sel_final  one wave per (S, slot): the tiles' lists merged as k_rlfa_nsel_final merges them (rnode_merge_tiles); lane
//                   j then reads p of the j-th q from its cell, recomputes p's release point and walks p's row for the first
//                   link into q at that metric; writes entry j.  Slots that are no candidates get the padding.
//   k_tn_dest       lane = destination over S's mask row (as k_rlfa_ndest): the six coverage counts.
// The vertex -> row map of the q rows is k_rlfa_nmap's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_rlfa_node.hip.h"

namespace {

constexpr uint32_t TNODE_MAX_PAIRS = 32;           // HSPF_TILFA_NODE_MAX_PAIRS
static_assert(TNODE_MAX_PAIRS == RNODE_MAX_PQ, "the shared top-M extraction keeps RNODE_MAX_PQ keys per wave");

struct TnSelArgs {
  RnodeSelArgs r;                                                          // n, stride, ignore_overload, max_pq = max_pairs, max_k, n_tiles, dist, tab, sflags, part
  const uint32_t *row_ptr, *col, *metric; const uint8_t *tw;               // the forward graph's raw CSR; two-way byte per link (staged)
  unsigned long long *cell;                                                // [n_prot][max_k][n] scratch, all-ones
  uint32_t *tq_q, *tq_p, *tq_link, *tq_via, *tq_metric, *tq_count;
};

__device__ __forceinline__ unsigned long long tn_entry(uint64_t rel, uint32_t w, uint32_t p) {
  const uint64_t t = rel + w;
  return ((t > RNODE_SAT ? RNODE_SAT : t) << 32) | p;
}

// is the link at k of p's row a usable forced adjacency into the Q-space of the slot whose space row starts at `so`?
__device__ __forceinline__ bool tn_link_ok(const TnSelArgs &a, size_t so, uint32_t k, uint32_t p, uint32_t E, uint32_t &q) {
  q = a.col[k];
  return q != p && q < a.r.n && q != E && a.tw[k] && (a.r.sflags[so + q] & 0x0Cu) == 0x0Cu;      // eligible and in Q
}

__global__ __launch_bounds__(256) void k_tn_link(TnSelArgs a) {
  const uint32_t tid = threadIdx.x, pi = blockIdx.z;
  const FrrTab tb = frr_tab(a.r.tab, pi);
  const uint32_t n = a.r.n;
  const uint32_t p = blockIdx.x * LFA_TILE + tid;
  const bool valid = p < n;
  const uint32_t pp = valid ? p : 0u;
  const uint32_t rb = valid ? a.row_ptr[pp] : 0u, re = valid ? a.row_ptr[pp + 1] : 0u;
  const size_t slot0 = (size_t)pi * a.r.stride;
  for (uint32_t ci = blockIdx.y; ci < tb.C; ci += gridDim.y) {
    const uint32_t e = tb.cl[ci], E = tb.nbr[e];
    const size_t so = (slot0 + e) * n;
    const uint32_t sf = valid ? a.r.sflags[so + pp] : 0u;
    const bool in_xp = (sf & 0x08u) && (sf & 0x03u) && pp != E;                    // eligible, in P or some XP
    if (!in_xp) continue;                                                          // (no barrier and no wave operation below: a lane may leave)
    uint64_t rel; uint32_t via;
    if (!rnode_release(a.r, tb, e, E, pp, a.r.dist[(size_t)tb.row[e] * n + pp], rel, via)) continue;
    unsigned long long *cells = a.cell + ((size_t)pi * a.r.max_k + ci) * n;
    for (uint32_t k = rb; k < re; ++k) {
      uint32_t q;
      if (tn_link_ok(a, so, k, pp, E, q)) atomicMin(cells + q, tn_entry(rel, a.metric[k], pp));
    }
  }
}

__global__ __launch_bounds__(256) void k_tn_sel(TnSelArgs a) {
  __shared__ unsigned long long s_list[4 * RNODE_MAX_PQ];
  __shared__ uint32_t s_cnt;
  const uint32_t tid = threadIdx.x, pi = blockIdx.z;
  const FrrTab tb = frr_tab(a.r.tab, pi);
  const uint32_t n = a.r.n, M = a.r.max_pq;
  const uint32_t q = blockIdx.x * LFA_TILE + tid;
  const bool valid = q < n;
  const size_t slot0 = (size_t)pi * a.r.stride;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (uint32_t ci = blockIdx.y; ci < tb.C; ci += gridDim.y) {
    const uint32_t e = tb.cl[ci];
    const unsigned long long c = valid ? a.cell[((size_t)pi * a.r.max_k + ci) * n + q] : RLFA_NO_KEY;
    const unsigned long long key = c == RLFA_NO_KEY ? RLFA_NO_KEY : ((c & 0xFFFFFFFF00000000ull) | q);
    rnode_block_top(key, M, s_list, &s_cnt, a.r.part + (((size_t)pi * a.r.max_k + ci) * a.r.n_tiles + blockIdx.x) * M, a.tq_count + slot0 + e);
  }
}

// one wave per (protected root, slot): the tiles' lists -> the slot's list; p from the cell, its via and the link again
__global__ __launch_bounds__(64) void k_tn_sel_final(TnSelArgs a) {
  const uint32_t lane = threadIdx.x, e = blockIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.r.tab, pi);
  const uint32_t n = a.r.n, M = a.r.max_pq;
  const size_t o = ((size_t)pi * a.r.stride + e) * M + lane;
  uint32_t q = LFA_NONE, p = LFA_NONE, link = LFA_NONE, via = LFA_NONE, met = 0;
  if (e < tb.K && tb.nbr[e] != LFA_NONE) {                                         // (block-uniform)
    uint32_t ci = 0;                                                               // e's place in the candidate list
    for (uint32_t k0 = 0; k0 < e; k0 += 64u) ci += (uint32_t)__popcll(__ballot(k0 + lane < e && tb.nbr[k0 + lane] != LFA_NONE));
    const unsigned long long *lists = a.r.part + ((size_t)pi * a.r.max_k + ci) * a.r.n_tiles * M;
    const unsigned long long mine = rnode_merge_tiles(lists, a.r.n_tiles, M, lane);
    const uint32_t qq = (uint32_t)mine, E = tb.nbr[e];
    // A key of k_tn_sel carries a q < n whose cell k_tn_link wrote: its low word is a p < n that HAD a release point and a
    // qualifying link into q at exactly this metric, and nothing has written the tables since.  So the release point is found
    // again and the row walk ends at a link; only the two bounds are checked, so that a broken invariant cannot read out of bounds
    // (it would show as padding in a list that tq_count says is longer: the tests compare both).
    const unsigned long long cellv = mine != RLFA_NO_KEY && qq < n ? a.cell[((size_t)pi * a.r.max_k + ci) * n + qq] : RLFA_NO_KEY;
    const uint32_t pv = (uint32_t)cellv;
    if (pv < n) {
      uint64_t rel;
      rnode_release(a.r, tb, e, E, pv, a.r.dist[(size_t)tb.row[e] * n + pv], rel, via);
      q = qq; p = pv; met = (uint32_t)(mine >> 32);
      const size_t so = ((size_t)pi * a.r.stride + e) * n;
      const uint32_t rb = a.row_ptr[pv], re = a.row_ptr[pv + 1];
      for (uint32_t k = rb; k < re; ++k) {                                         // ascending position: the first link at the entry metric
        uint32_t t;
        if (tn_link_ok(a, so, k, pv, E, t) && t == qq && tn_entry(rel, a.metric[k], pv) == cellv) { link = k - rb; break; }
      }
    }
  }
  if (lane < M) { a.tq_q[o] = q; a.tq_p[o] = p; a.tq_link[o] = link; a.tq_via[o] = via; a.tq_metric[o] = met; }
}

struct TnDestArgs {
  uint32_t n, W, stride, max_pairs;
  const uint32_t *dist; const uint16_t *flags; const uint64_t *mask;       // the forward table set
  const uint32_t *tab;                                                     // the staged candidate tables
  const uint32_t *ydist;                                                   // [n_yrows][n] rows rooted at listed q's
  const uint32_t *ymap;                                                    // [n] vertex -> row of ydist, all-ones: none (k_rlfa_nmap)
  const uint32_t *tq_q, *tq_p, *tq_link, *tq_via, *tq_metric, *tq_count;
  const uint8_t *alt_in;                                                   // [n_prot][n] alt_flags of hspf_lfa_device, or NULL
  const uint8_t *nd_in;                                                    // [n_prot][n] nd_kind of hspf_rlfa_node_device, or NULL
  uint8_t *tn_kind; uint32_t *tn_p, *tn_q, *tn_link, *tn_via, *tn_metric, *tn_set, *tn_cov;
};

// per destination D of S with exactly one primary slot: covered by a node-protecting LFA | no candidate | E itself | by the
// one-segment repair of hspf_rlfa_node_device | by a listed pair whose q reaches D without E | uncovered; the six counts
__global__ __launch_bounds__(256) void k_tn_dest(TnDestArgs a) {
  __shared__ uint32_t s_cov[6];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n, M = a.max_pairs;
  if (tid < 6) s_cov[tid] = 0;
  __syncthreads();
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  const size_t od = (size_t)pi * n + D;
  const bool in = valid && D != tb.S && (a.flags[sd] & 1u) && a.dist[sd] != LFA_NONE;
  uint32_t cls = 0, p = LFA_NONE, q = LFA_NONE, link = LFA_NONE, via = LFA_NONE, met = 0, set = 0;
  if (in) {
    uint32_t np, p0;
    frr_primaries(tb, a.mask + sd * a.W, np, p0);
    if (np == 1) {
      if (a.alt_in && (a.alt_in[od] & 0x08u)) cls = 1u;                            // HSPF_LFA_NODE_PROTECT: LFA covers it
      else if (tb.nbr[p0] == LFA_NONE) cls = 4u;
      else if (tb.nbr[p0] == D) cls = 3u;
      else if (a.nd_in && a.nd_in[od] == 2u) cls = 2u;                             // HSPF_NP_D_PQ: the one-segment repair stands
      else {
        const uint32_t E = tb.nbr[p0];
        const size_t so = (size_t)pi * a.stride + p0;
        const uint32_t cnt = a.tq_count[so], L = cnt < M ? cnt : M;
        const uint32_t dED = a.dist[(size_t)tb.row[p0] * n + D];
        uint64_t best = ~0ull;
        uint32_t bj = 0;
        for (uint32_t j = 0; j < L; ++j) {
          const uint32_t Y = a.tq_q[so * M + j];
          if (Y >= n) continue;
          const uint32_t r = a.ymap[Y];
          if (r == LFA_NONE) continue;                                             // a listed q without a row is skipped
          const uint32_t *dY = a.ydist + (size_t)r * n;
          const uint32_t dYD = dY[D];
          if (!lfa_less(dYD, dY[E], dED)) continue;
          set |= 1u << j;
          const uint64_t tot = (uint64_t)a.tq_metric[so * M + j] + dYD;
          if (tot < best) { best = tot; bj = j; }
        }
        if (set) {
          cls = 5u;
          const size_t ob = so * M + bj;
          p = a.tq_p[ob]; q = a.tq_q[ob]; link = a.tq_link[ob]; via = a.tq_via[ob];
          met = (uint32_t)(best > RNODE_SAT ? RNODE_SAT : best);
        } else cls = 4u;
      }
    }
  }
  if (valid) {
    a.tn_kind[od] = (uint8_t)cls; a.tn_p[od] = p; a.tn_q[od] = q; a.tn_link[od] = link; a.tn_via[od] = via; a.tn_metric[od] = met;
    if (a.tn_set) a.tn_set[od] = set;
  }
  frr_cover<6>(cls ? 1u | (1u << cls) : 0u, s_cov, a.tn_cov + (size_t)pi * 6);      // counter 0: any class; counter j: class j (1 .. 5)
}

}  // namespace
