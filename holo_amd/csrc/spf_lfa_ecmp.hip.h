// spf_lfa_ecmp.hip.h — per-primary alternates of ECMP destinations (hspf_lfa_ecmp_device; the semantics are written down once, in
// include/holo_spf_hip.h).  For every (protected root S, destination D) with two or more primary slots and every one of those
// primaries h: the alternate of h and what it protects, as a compact stream in CSR form over (S, D).
//
// Three steps on the staged candidate tables of hspf_lfa_device (spf_frr_common.hip.h) and k_lfa_gather's scalars:
//   k_lfa_ecmp_count    lane = (S, D), 256 consecutive D per workgroup: popcount of the masked words of mask_S[D], the per-D
//                       count (0 below two primaries) into ea_ptr[(S, D)] and the tile's total into the scratch.  Reads S's row only.
//   k_events_scan       (spf_kernels.hip.h, as it is) the exclusive scan over the tile totals in place, the total behind them and
//                       into a pinned word.  One workgroup, 1024 tiles per pass.  The host-side bound of the call keeps the total
//                       below 2^32, so the scan's 32-bit carry is exact.
//   k_lfa_ecmp_fill<ONE> a workgroup per tile again.  The scan INSIDE the tile (gb_block_exclusive) turns the 256 counts into the
//                       tile's 257 ea_ptr values, kept in LDS and written out: ea_ptr is complete whatever the capacity.  Then,
//                       unless the total exceeds cap_entries, the tile's entries — one contiguous range of the stream — are dealt
//                       to the lanes with stride 256: a lane finds its D by binary search in LDS, its h as the r-th set bit of P,
//                       and runs the candidate loop of lfa_body for that one (D, h).  A fat-tree D with 50 primaries x 100
//                       candidates is 50 lanes x 100 row reads, not one lane x 5 000; the d(N_k, D) reads of a tile stay inside one
//                       1 KB segment per row.
//                       ONE = true (every root has at most 64 slots): the columns, d(N_k, S) and the K x K matrix in LDS exactly as
//                       in k_lfa<true>, next to the ea_ptr tile (21.3 KB in all); ONE = false: through the caches.
// Coverage: the five per-ENTRY counters are summed over a lane's entries with wave ballots into lane j's register, one LDS add per
// wave; the two per-DESTINATION counters are flag bits of lane = D; frr_cover adds those and issues the one atomic per workgroup
// and counter for all seven.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_lfa.hip.h"

namespace {

constexpr uint32_t EA_CW = 7;                // HSPF_LFA_ECMP_COVERAGE_WORDS
constexpr uint32_t EA_SCAN_PASS = 1024;      // tiles k_events_scan consumes per pass

struct LfaEcmpArgs {
  LfaArgs l;                                 // the table set, the staged tables and scalars (its outputs are not used)
  uint32_t n_prot, pad;
  unsigned long long cap;
  uint32_t *tile;                            // [n_prot * tiles_x] tile totals, then offsets | the total
  uint32_t *ea_ptr, *ea_primary, *ea_slot, *ea_metric; uint8_t *ea_flags; uint32_t *ea_coverage;
};

__global__ __launch_bounds__(256) void k_lfa_ecmp_count(LfaEcmpArgs a) {
  __shared__ uint32_t s_scan[GB_BLOCK];
  static_assert(GB_BLOCK == (int)LFA_TILE, "gb_block_exclusive scans one tile");
  const uint32_t tid = threadIdx.x, pi = blockIdx.y, n = a.l.n;
  const FrrTab tb = frr_tab(a.l.tab, pi);
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  uint32_t np = 0, p0;
  if (valid && D != tb.S && (a.l.flags[sd] & 1u) && a.l.dist[sd] != LFA_NONE) frr_primaries(tb, a.l.mask + sd * a.l.W, np, p0);
  const uint32_t cnt = np >= 2 ? np : 0u;
  if (valid) a.ea_ptr[(size_t)pi * n + D] = cnt;
  uint32_t total;
  (void)gb_block_exclusive(cnt, s_scan, total);
  if (tid == 0) a.tile[(size_t)pi * gridDim.x + blockIdx.x] = total;
}

template <bool ONE>
__global__ __launch_bounds__(256) void k_lfa_ecmp_fill(LfaEcmpArgs a) {
  __shared__ uint32_t s_cov[EA_CW];
  __shared__ uint32_t s_ptr[LFA_TILE + 1];                               // the tile's ea_ptr values, from 0
  __shared__ uint32_t s_scan[GB_BLOCK];
  __shared__ uint8_t s_miss[LFA_TILE];                                   // destination of the tile: some primary got no alternate
  __shared__ uint32_t s_tab[ONE ? (FRR_COLS + 1) * 64 : 1];              // the columns, then d(N_k, S)
  __shared__ uint32_t s_m[ONE ? 64 * 64 : 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.y;
  FrrTab tb = frr_tab(a.l.tab, a.l.scal, pi);
  const uint32_t K = tb.K, n = a.l.n, W = a.l.W;
  if (tid < EA_CW) s_cov[tid] = 0;
  s_miss[tid] = 0;
  if constexpr (ONE) {                                                   // the same view over a copy in LDS, as k_lfa<true>
    for (uint32_t i = tid; i < FRR_COLS * K; i += 256u) s_tab[i] = tb.cols[i];
    for (uint32_t i = tid; i < K; i += 256u) s_tab[FRR_COLS * K + i] = tb.dns[i];
    for (uint32_t i = tid; i < K * K; i += 256u) s_m[i] = tb.m[i];
    tb = frr_tab_over(tb.S, tb.srow, K, tb.C, s_tab, s_tab + FRR_COLS * K, s_m);
  }
  // the scan inside the tile: counts -> ea_ptr
  const uint32_t D0 = blockIdx.x * LFA_TILE;
  const bool valid = D0 + tid < n;
  const size_t od = (size_t)pi * n + D0 + tid;
  const uint32_t cnt = valid ? a.ea_ptr[od] : 0u;
  uint32_t ttot;
  const uint32_t loc = gb_block_exclusive(cnt, s_scan, ttot);
  const size_t ti = (size_t)pi * gridDim.x + blockIdx.x, n_tiles = (size_t)a.n_prot * gridDim.x;
  const uint32_t base = a.tile[ti];
  s_ptr[tid] = loc;
  if (tid == 0) s_ptr[LFA_TILE] = ttot;
  if (valid) a.ea_ptr[od] = base + loc;
  if (ti + 1 == n_tiles && tid == 0) a.ea_ptr[(size_t)a.n_prot * n] = base + ttot;
  __syncthreads();
  if ((unsigned long long)a.tile[n_tiles] > a.cap) return;               // the caller repeats the call with larger arrays

  uint32_t my_cov = 0;                                                   // lane j, 1 <= j <= 5, of a wave: its count of entry bit j
  for (uint32_t e0 = 0; e0 < ttot; e0 += 256u) {                         // (uniform: every lane comes to the ballots)
    const uint32_t e = e0 + tid;
    uint32_t cv = 0;
    if (e < ttot) {
      uint32_t lo = 0, hi = LFA_TILE;                                    // the largest dl with s_ptr[dl] <= e: its count is not 0
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_ptr[mid] <= e) lo = mid; else hi = mid;
      }
      const uint32_t D = D0 + lo;
      uint32_t r = e - s_ptr[lo];
      const size_t sd = (size_t)tb.srow * n + D;
      const uint64_t *pm = a.l.mask + sd * W;
      const uint32_t dSD = a.l.dist[sd];
      uint32_t h = 0;                                                    // the r-th primary
      for (uint32_t w = 0; w < tb.Wk; ++w) {
        uint64_t x = frr_word(tb, pm, w);
        const uint32_t c = (uint32_t)__popcll(x);
        if (r < c) {
          for (; r; --r) x &= x - 1;
          h = w * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
          break;
        }
        r -= c;
      }
      const uint32_t rlh = tb.rl[h], E = tb.nbr[h];
      const uint32_t dED = E != LFA_NONE ? a.l.dist[(size_t)tb.row[h] * n + D] : LFA_NONE;
      bool have = false, bnode = false, bprim = false, bdown = false;
      uint64_t bsum = 0;
      uint32_t bslot = LFA_NONE;
      for (uint32_t ci = 0; ci < tb.C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if (k == h) continue;
        const uint32_t dND = a.l.dist[(size_t)tb.row[k] * n + D];
        if (!lfa_less(dND, tb.dns[k], dSD)) continue;                    // loop-free: ONE rule, a primary or not
        if ((tb.cf[k] & 1u) && !a.l.ignore_overload && tb.nbr[k] != D) continue;
        if (tb.rl[k] == rlh) continue;                                   // shares the first link's fate
        const bool nd = E != LFA_NONE && lfa_less(dND, tb.m[k * K + h], dED);
        const bool pr = (pm[k >> 6] >> (k & 63u)) & 1ull;
        const uint64_t sum = (uint64_t)tb.cost[k] + dND;
        if (!have || (nd && !bnode) || (nd == bnode && ((pr && !bprim) || (pr == bprim && sum < bsum)))) {   // ascending slot order
          have = true; bnode = nd; bprim = pr; bsum = sum; bslot = k; bdown = dND < dSD;
        }
      }
      const uint32_t fl = have ? 0x04u | (bnode ? 0x08u : 0u) | (bdown ? 0x10u : 0u) | (bprim ? 0x20u : 0u) : 0u;
      const size_t g = (size_t)base + e;                                 // < total <= cap
      a.ea_primary[g] = h; a.ea_slot[g] = bslot;
      a.ea_metric[g] = !have ? 0u : bsum > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)bsum;
      a.ea_flags[g] = (uint8_t)fl;
      if (!have) s_miss[lo] = 1;
      cv = 0x02u | (fl & 0x04u) | (fl & 0x18u) | (fl & 0x20u);           // entry | with an alternate | node | downstream | a primary
    }
#pragma unroll
    for (uint32_t j = 1; j <= 5; ++j) {
      const uint32_t c = (uint32_t)__popcll(__ballot((cv >> j) & 1u));
      if (lane == j) my_cov += c;
    }
  }
  if (my_cov) atomicAdd(&s_cov[lane], my_cov);                           // (only lanes 1 .. 5 hold a count)
  __syncthreads();                                                       // s_miss is complete
  const uint32_t dfl = cnt >= 2 ? 0x01u | (s_miss[tid] ? 0u : 0x40u) : 0u;   // ECMP destination | every primary has an alternate
  frr_cover<EA_CW>(dfl, s_cov, a.ea_coverage + (size_t)pi * EA_CW);
}

}  // namespace
