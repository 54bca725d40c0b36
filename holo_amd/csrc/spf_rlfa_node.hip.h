// spf_rlfa_node.hip.h — node-protecting remote loop-free alternates (RFC 8102): per (protected root S, protected slot e) the
// cheapest few link-protecting PQ nodes whose release path avoids the NODE E behind the slot (hspf_rlfa_node_select_device), and
// per destination the cheapest of them whose own shortest path to the destination avoids E too, from the forward SPT rows
// rooted at those nodes (hspf_rlfa_node_device; the semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  As k_tilfa: lane = vertex, 256 consecutive v per workgroup; the candidate slots of a root are the grid's y axis, the
// protected roots its z axis.
//   k_rlfa_nsel        per slot the lane loads space_flags[e][v] (coalesced); a wave none of whose vertices is a link-protecting
//                      PQ node is done.  The others load d(S, v), d(E, v) and stream the via-slots k once: d(N_k, v) is judged
//                      against the wave-uniform d(N_k, E) and forgotten.  The key (saturated release metric << 32 | v) is
//                      unique per vertex, so the cheapest max_pq of a wave are taken by repeated extraction of "the smallest key
//                      not below the last one + 1" — a wave minimum each; lane j keeps the j-th.  The four waves' lists meet in
//                      LDS, wave 0 extracts the workgroup's list the same way and stores it (plain vector stores) into the
//                      call's scratch: [root][candidate][tile][max_pq] keys, all-ones padded — every cell is written, none is
//                      initialised.  The count is a ballot + popcount, one LDS add per wave, one vector atomic per workgroup.
//   k_rlfa_nsel_final  one wave per (S, slot): lane t holds the smallest unused key of the sorted lists of tiles t, t + 64, ...; a
//                      wave minimum per extraction, and only the winner's lane walks its lists again; lane j then recomputes the
//                      via of the j-th winner (as k_tilfa_final does for q) and writes entry j.  Slots that are no candidates
//                      get the padding.
//   k_rlfa_nmap        vertex -> row of the PQ-node table set, from the caller's root list.
//   k_rlfa_ndest       lane = destination over S's mask row (as k_rlfa_dest / k_tilfa_dest): the list of its one primary slot is
//                      walked, entry j's d(Y, D) is a load of consecutive D in one row wherever neighbouring lanes share the
//                      slot; the five coverage counts.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_rlfa.hip.h"

namespace {

constexpr uint32_t RNODE_MAX_PQ = 32;              // HSPF_RLFA_NODE_MAX_PQ
constexpr uint64_t RNODE_SAT = 0xFFFFFFFEull;

struct RnodeSelArgs {
  uint32_t n, stride, ignore_overload, max_pq;                             // stride = 64 * W slots per protected root
  uint32_t max_k, n_tiles;                                                 // the dimensions of `part`
  const uint32_t *dist;                                                    // the forward table set
  const uint32_t *tab;                                                     // the staged candidate tables
  const uint8_t *sflags;                                                   // [n_prot][stride][n] of hspf_rlfa_device
  unsigned long long *part;                                                // [n_prot][max_k][n_tiles][max_pq] scratch
  uint32_t *nq_node, *nq_via, *nq_metric, *nq_count;
};

// The release point of v under slot e when the NODE E is to be avoided: d(S, v) if S's own paths to v avoid E, cost[k] + d(N_k, v)
// over the via-slots k whose paths do; S first, then ascending k.  dEv = d(E, v).  false: v has none.
__device__ __forceinline__ bool rnode_release(const RnodeSelArgs &a, const FrrTab &tb, uint32_t e, uint32_t E, uint32_t v, uint32_t dEv,
                                              uint64_t &best, uint32_t &via) {
  const uint32_t n = a.n;
  const uint32_t *dS = a.dist + (size_t)tb.srow * n;
  best = ~0ull; via = LFA_NONE;
  if (dEv == LFA_NONE) return false;
  const uint32_t dSv = dS[v];
  if (lfa_less(dSv, dS[E], dEv)) { best = dSv; via = RLFA_VIA_SELF; }
  const uint32_t rle = tb.rl[e];
  for (uint32_t ci = 0; ci < tb.C; ++ci) {
    const uint32_t k = tb.cl[ci];
    if ((tb.cf[k] & 1u) && !a.ignore_overload) continue;                           // an overloaded neighbour carries no transit traffic
    if (tb.rl[k] == rle || tb.nbr[k] == E) continue;                               // the protected first link | a parallel link to E
    const uint32_t *dN = a.dist + (size_t)tb.row[k] * n;
    const uint32_t dNv = dN[v];
    if (!lfa_less(dNv, dN[E], dEv)) continue;
    const uint64_t rel = (uint64_t)tb.cost[k] + dNv;
    if (rel < best) { best = rel; via = k; }
  }
  return via != LFA_NONE;
}

// The top-M extraction the select kernels share (this file and spf_tilfa_node.hip.h).  Keys are unique or all-ones.
// the M smallest of the wave's 2 x 64 keys in ascending order, by repeated extraction of "the smallest key not below the last one + 1"
// (a wave minimum each): lane j returns the j-th
__device__ __forceinline__ unsigned long long rnode_wave_top(unsigned long long k0, unsigned long long k1, uint32_t M, uint32_t lane) {
  unsigned long long out = RLFA_NO_KEY, lo = 0;
  for (uint32_t j = 0; j < M; ++j) {
    const unsigned long long c0 = k0 >= lo ? k0 : RLFA_NO_KEY, c1 = k1 >= lo ? k1 : RLFA_NO_KEY;
    const unsigned long long m = rlfa_wave_min(c0 < c1 ? c0 : c1);
    if (m == RLFA_NO_KEY) break;
    if (lane == j) out = m;
    lo = m + 1;
  }
  return out;
}

// One key per thread of a 256-thread workgroup -> the workgroup's M smallest, stored (plain vector stores, all-ones padded) to
// part[0 .. M), and the number of keys added to *count.  Per wave into s_list[4 * RNODE_MAX_PQ], wave 0 merges the four lists the
// same way.  *s_cnt is the workgroup's, 0 on entry and on return; every thread comes here (two barriers inside).
__device__ __forceinline__ void rnode_block_top(unsigned long long key, uint32_t M, unsigned long long *s_list, uint32_t *s_cnt,
                                                unsigned long long *part, uint32_t *count) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long mine = RLFA_NO_KEY;
  const unsigned long long b = __ballot(key != RLFA_NO_KEY);
  if (b) {                                                                         // (wave-uniform)
    if (lane == 0) atomicAdd(s_cnt, (uint32_t)__popcll(b));
    mine = rnode_wave_top(key, RLFA_NO_KEY, M, lane);
  }
  if (lane < RNODE_MAX_PQ) s_list[wave * RNODE_MAX_PQ + lane] = mine;
  __syncthreads();
  if (wave == 0) {
    // the four sorted lists -> the workgroup's: two cells per lane, the same extraction
    const unsigned long long out = rnode_wave_top(s_list[lane], s_list[lane + 64], M, lane);
    if (lane < M) part[lane] = out;
    if (lane == 0 && *s_cnt) { atomicAdd(count, *s_cnt); *s_cnt = 0; }
  }
  __syncthreads();
}

// One wave: the n_tiles sorted, all-ones padded lists of M keys at `lists` -> their M smallest; lane j returns the j-th.  Lane t holds
// the smallest unused key of tiles t, t + 64, ...; a wave minimum per extraction, and only the winner's lane walks its lists again.
__device__ __forceinline__ unsigned long long rnode_merge_tiles(const unsigned long long *lists, uint32_t n_tiles, uint32_t M, uint32_t lane) {
  // the lane's candidate: the smallest key not below `lo` in its tiles' lists (sorted: the first one counts)
  auto scan = [&](unsigned long long lo) {
    unsigned long long c = RLFA_NO_KEY;
    for (uint32_t t = lane; t < n_tiles; t += 64u) {
      const unsigned long long *L = lists + (size_t)t * M;
      for (uint32_t i = 0; i < M; ++i) {
        const unsigned long long k = L[i];
        if (k >= lo) { c = k < c ? k : c; break; }
      }
    }
    return c;
  };
  unsigned long long mine = RLFA_NO_KEY, c = scan(0);
  for (uint32_t j = 0; j < M; ++j) {
    const unsigned long long m = rlfa_wave_min(c);
    if (m == RLFA_NO_KEY) break;
    if (lane == j) mine = m;
    if (c == m) c = scan(m + 1);                                                   // keys are unique: only the winner's lane looks again
  }
  return mine;
}

__global__ __launch_bounds__(256) void k_rlfa_nsel(RnodeSelArgs a) {
  __shared__ unsigned long long s_list[4 * RNODE_MAX_PQ];
  __shared__ uint32_t s_cnt;
  const uint32_t tid = threadIdx.x, pi = blockIdx.z;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n, M = a.max_pq;
  const uint32_t v = blockIdx.x * LFA_TILE + tid;
  const bool valid = v < n;
  const uint32_t vv = valid ? v : 0u;
  const size_t slot0 = (size_t)pi * a.stride;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (uint32_t ci = blockIdx.y; ci < tb.C; ci += gridDim.y) {
    const uint32_t e = tb.cl[ci], E = tb.nbr[e];
    const uint32_t sf = valid ? a.sflags[(slot0 + e) * n + vv] : 0u;
    const bool lpq = (sf & 0x0Cu) == 0x0Cu && (sf & 0x03u) && vv != E;             // eligible, in Q, in P or some XP: a link-protecting PQ node
    unsigned long long key = RLFA_NO_KEY;
    if (lpq) {                                                                     // (a wave without one loads nothing more)
      uint64_t best; uint32_t via;
      if (rnode_release(a, tb, e, E, vv, a.dist[(size_t)tb.row[e] * n + vv], best, via))
        key = ((best > RNODE_SAT ? RNODE_SAT : best) << 32) | vv;
    }
    rnode_block_top(key, M, s_list, &s_cnt, a.part + (((size_t)pi * a.max_k + ci) * a.n_tiles + blockIdx.x) * M, a.nq_count + slot0 + e);
  }
}

// one wave per (protected root, slot): the tiles' lists -> the slot's list; the via of each winner again
__global__ __launch_bounds__(64) void k_rlfa_nsel_final(RnodeSelArgs a) {
  const uint32_t lane = threadIdx.x, e = blockIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n, M = a.max_pq;
  const size_t o = ((size_t)pi * a.stride + e) * M + lane;
  uint32_t node = LFA_NONE, via = LFA_NONE, met = 0;
  if (e < tb.K && tb.nbr[e] != LFA_NONE) {                                         // (block-uniform)
    uint32_t ci = 0;                                                               // e's place in the candidate list
    for (uint32_t k0 = 0; k0 < e; k0 += 64u) ci += (uint32_t)__popcll(__ballot(k0 + lane < e && tb.nbr[k0 + lane] != LFA_NONE));
    const unsigned long long *lists = a.part + ((size_t)pi * a.max_k + ci) * a.n_tiles * M;
    const unsigned long long mine = rnode_merge_tiles(lists, a.n_tiles, M, lane);
    if (mine != RLFA_NO_KEY) {
      const uint32_t v = (uint32_t)mine, E = tb.nbr[e];
      uint64_t best;
      if (v < n && rnode_release(a, tb, e, E, v, a.dist[(size_t)tb.row[e] * n + v], best, via)) { node = v; met = (uint32_t)(mine >> 32); }
      else via = LFA_NONE;
    }
  }
  if (lane < M) { a.nq_node[o] = node; a.nq_via[o] = via; a.nq_metric[o] = met; }
}

struct RnodeDestArgs {
  uint32_t n, W, stride, max_pq;
  const uint32_t *dist; const uint16_t *flags; const uint64_t *mask;       // the forward table set
  const uint32_t *tab;                                                     // the staged candidate tables
  const uint32_t *ydist;                                                   // [n_yrows][n] rows rooted at the PQ nodes
  const uint32_t *yroots; uint32_t n_yrows;                                // the root list (staged)
  uint32_t *ymap;                                                          // [n] vertex -> row of ydist, all-ones: none
  const uint32_t *nq_node, *nq_via, *nq_metric, *nq_count;
  const uint8_t *alt_in;                                                   // [n_prot][n] alt_flags of hspf_lfa_device, or NULL
  uint8_t *nd_kind; uint32_t *nd_node, *nd_via, *nd_metric, *nd_set, *nd_cov;
};

// vertex -> row (a vertex listed twice keeps one of its rows: they are identical)
__global__ __launch_bounds__(256) void k_rlfa_nmap(RnodeDestArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_yrows) return;
  const uint32_t v = a.yroots[i];
  if (v < a.n) a.ymap[v] = i;
}

// per destination D of S with exactly one primary slot: covered by a node-protecting LFA | by a listed PQ node whose path to D
// avoids E | E itself | uncovered; the five counts
__global__ __launch_bounds__(256) void k_rlfa_ndest(RnodeDestArgs a) {
  __shared__ uint32_t s_cov[5];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n, M = a.max_pq;
  if (tid < 5) s_cov[tid] = 0;
  __syncthreads();
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  const size_t od = (size_t)pi * n + D;
  const bool in = valid && D != tb.S && (a.flags[sd] & 1u) && a.dist[sd] != LFA_NONE;
  uint32_t cls = 0, node = LFA_NONE, via = LFA_NONE, met = 0, set = 0;
  if (in) {
    uint32_t np, p0;
    frr_primaries(tb, a.mask + sd * a.W, np, p0);
    if (np == 1) {
      if (a.alt_in && (a.alt_in[od] & 0x08u)) cls = 1u;                            // HSPF_LFA_NODE_PROTECT: LFA covers it
      else if (tb.nbr[p0] == LFA_NONE) cls = 4u;
      else if (tb.nbr[p0] == D) cls = 3u;
      else {
        const uint32_t E = tb.nbr[p0];
        const size_t so = (size_t)pi * a.stride + p0;
        const uint32_t cnt = a.nq_count[so], L = cnt < M ? cnt : M;
        const uint32_t dED = a.dist[(size_t)tb.row[p0] * n + D];
        uint64_t best = ~0ull;
        uint32_t bj = 0;
        for (uint32_t j = 0; j < L; ++j) {
          const uint32_t Y = a.nq_node[so * M + j];
          if (Y >= n) continue;
          const uint32_t r = a.ymap[Y];
          if (r == LFA_NONE) continue;                                             // a listed node without a row is skipped
          const uint32_t *dY = a.ydist + (size_t)r * n;
          const uint32_t dYD = dY[D];
          if (!lfa_less(dYD, dY[E], dED)) continue;
          set |= 1u << j;
          const uint64_t tot = (uint64_t)a.nq_metric[so * M + j] + dYD;
          if (tot < best) { best = tot; bj = j; }
        }
        if (set) {
          cls = 2u;
          node = a.nq_node[so * M + bj]; via = a.nq_via[so * M + bj];
          met = (uint32_t)(best > RNODE_SAT ? RNODE_SAT : best);
        } else cls = 4u;
      }
    }
  }
  if (valid) {
    a.nd_kind[od] = (uint8_t)cls; a.nd_node[od] = node; a.nd_via[od] = via; a.nd_metric[od] = met;
    if (a.nd_set) a.nd_set[od] = set;
  }
  frr_cover<5>(cls ? 1u | (1u << cls) : 0u, s_cov, a.nd_cov + (size_t)pi * 5);      // counter 0: any class; counter j: class j (1 .. 4)
}

}  // namespace
