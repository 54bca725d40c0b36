// spf_backup_ecmp.hip.h — per-primary backups of ECMP prefixes (hspf_routes_backup_ecmp_device; the semantics are written down once,
// in include/holo_spf_hip.h).  For every (protected root S, prefix p) whose route has two or more primary slots and every one of those
// primaries h: the backup of h and what it protects, as a compact stream in CSR form over (S, p).  The rule is that of
// hspf_lfa_ecmp_device (spf_lfa_ecmp.hip.h) with d_N(p), the minimum over p's advertisers, in place of d(N, D).
//
// Three steps on the staged candidate tables (spf_frr_common.hip.h), k_lfa_gather's scalars and the staged prefix table:
//   k_backup_ecmp_count   lane = (S, p), 256 consecutive prefixes per workgroup: popcount of the masked words of nexthop_mask[p], the
//                         per-p count (0 for an absent route and below two primaries) into eb_ptr[(S, p)], the tile's total into the
//                         scratch.  Reads S's route row only.
//   k_events_scan         (spf_kernels.hip.h, as it is) the exclusive scan over the tile totals in place, the total behind them and
//                         into a pinned word.  The host-side bound of the call keeps the total below 2^32.
//   k_backup_ecmp_fill    a workgroup per tile again.  Two scans INSIDE the tile (gb_block_exclusive): the counts give the tile's 257
//                         eb_ptr values, kept in LDS and written out whatever the capacity; the "is ECMP" bits give the list of the
//                         tile's ECMP prefixes.  Unless the total exceeds cap_entries that list is taken in BATCHES of
//                         B = max(1, BE_SLOTS / C) prefixes:
//                           fill   lanes take (prefix of the batch, candidate) pairs with stride 256, stream the prefix's entries
//                                  ONCE for that neighbour's row and leave d_N(p) — with the bit "N's own entry attains it" — in LDS:
//                                  C x entries row gathers per ECMP prefix, no factor of the number of primaries;
//                           walk   behind a barrier the batch's entries — one contiguous range of the stream — are dealt to the
//                                  lanes with stride 256: a lane finds its p by binary search in LDS, its h as the r-th set bit of
//                                  P, and walks the candidates of p FROM LDS under the one rule (order: node, primary, sum, slot).
//                                  d_E(p) of a router primary is the LDS value of slot h itself (h is a candidate: its place in
//                                  the ascending candidate list by binary search).
//                         A root with more candidates than BE_SLOTS (2 048) takes one prefix per batch and its candidates in chunks
//                         of BE_SLOTS: the lane keeps its choice across the chunks, d_E(p) is then streamed by the lane, and a
//                         prefix with more than 256 primaries refills the chunks per 256 entries.  Every loop bound in front of a
//                         barrier comes from LDS or the arguments: uniform across the workgroup; there is no return in front of one.
//                         ONE shape: the staged columns and scalars are read through the caches (the K <= 64 copy in LDS of
//                         k_lfa_ecmp_fill<true> was not built: the LDS goes to the d_N(p) batch).
// Modes (FrrProt, spf_frr_common.hip.h).  The fill step is ONE body, backup_ecmp_fill_body<P>, in two modes: Plain is
// k_backup_ecmp_fill as it was; Srlg (hspf_routes_backup_ecmp_srlg_device) is k_backup_ecmp_fill_srlg.  The batch and the walk are
// the same text; BackupEcmpLane<Srlg> adds what depends on the ENTRY (p, h) alone: the members of slot h — of h, not of all of P —
// and d_{b_i}(p) of those at most 16 members, computed ONCE per entry in front of the candidate chunks.  The lane is BkMembers
// (spf_backup_srlg.hip.h), the member lane of k_backup_srlg: its two streams of the prefix's entries (members 0 .. 7, 8 .. 15), its
// member test and its forced-adjacency test; the values are packed to 33 bits in registers.  A candidate reads
// loc, d(N_k, a_i) and w_i of k_srlg_gather's block only after it has passed every plain condition; an entry whose h has no
// members reads sptr[h], sptr[h + 1] and nothing else of the member block, and streams no advertiser row more than Plain does.
// Registers, not LDS: next to the d_N(p) batch 256 entries x 16 members x 33 bits would be 17 KB more (37 KB: four workgroups per
// CU where the registers allow more), the values are private to the lane that made them, and the resource report shows the
// register form without scratch (profiles/r28_notes.md).  Coverage has three more per-entry words in the mode Srlg.
// Coverage: the six per-ENTRY counters are summed over a lane's entries with wave ballots into lane j's register, one LDS add per
// wave; the two per-PREFIX counters are flag bits of lane = p; frr_cover adds those and issues the one atomic per workgroup and
// counter for all eight.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_backup.hip.h"
#include "spf_backup_srlg.hip.h"

namespace {

constexpr uint32_t EB_CW = 8;                // HSPF_BK_ECMP_COVERAGE_WORDS
constexpr uint32_t EBS_CW = 11;              // HSPF_BK_ECMP_SRLG_COVERAGE_WORDS
constexpr uint32_t be_cov_words(FrrProt P) { return P == FrrProt::Srlg ? EBS_CW : EB_CW; }
constexpr uint32_t BE_SLOTS = 2048;          // d_N(p) values of one batch in LDS (16 KB)
constexpr uint64_t BE_OWN = 1ull << 62;      // next to a d_N(p) (< 2^33) in LDS: N's own entry attains it
constexpr uint64_t BE_VAL = (1ull << 40) - 1ull;

struct BackupEcmpArgs {
  BackupArgs b;                              // the table set, the staged tables, the prefix table, the routes, the repairs (bk_* unused)
  uint32_t n_prot, pad;
  unsigned long long cap;
  uint32_t *tile;                            // [n_prot * tiles_x] tile totals, then offsets | the total
  uint32_t *eb_ptr, *eb_primary; uint8_t *eb_kind; uint32_t *eb_slot, *eb_metric; uint8_t *eb_flags; uint32_t *eb_coverage;
};

// the fill body's modes (spf_frr_common.hip.h: <Family>Prot<P>, <Family>Lane<P>)
template <FrrProt P> struct BackupEcmpProt {};
template <> struct BackupEcmpProt<FrrProt::Srlg> { BackupSrlgArgs s; };
template <FrrProt P> struct BackupEcmpLane {};
template <> struct BackupEcmpLane<FrrProt::Srlg> {
  BkMembers mb;                                                          // the members of the entry's h (spf_backup_srlg.hip.h)
  uint32_t sfl = 0;                                                      // HSPF_BK_SRLG_PRIMARY | _PAIR_REFUSED | HSPF_LFA_SRLG_REFUSED

  __device__ __forceinline__ void open(const BackupEcmpProt<FrrProt::Srlg> &pa, uint32_t pi, uint32_t K) { mb.st = srlg_tab(pa.s.sa, pi, K); }
  // a new entry (p, h)
  __device__ __forceinline__ void entry(const BackupArgs &a, bool live, uint32_t h, uint32_t lo, uint32_t hi) {
    if (live) mb.stream(a, h, lo, hi); else mb.clear();
    sfl = mb.nm ? 0x01u : 0u;
  }
};

__global__ __launch_bounds__(256) void k_backup_ecmp_count(BackupEcmpArgs a) {
  __shared__ uint32_t s_scan[GB_BLOCK];
  static_assert(GB_BLOCK == (int)LFA_TILE, "gb_block_exclusive scans one tile");
  const uint32_t tid = threadIdx.x, pi = blockIdx.y, n_pfx = a.b.n_pfx;
  const FrrTab tb = frr_tab(a.b.tab, pi);
  const uint32_t p = blockIdx.x * LFA_TILE + tid;
  const bool valid = p < n_pfx;
  const size_t oi = (size_t)tb.srow * n_pfx + (valid ? p : 0u);
  uint32_t np = 0, p0;
  if (valid && a.b.best_entry[oi] != LFA_NONE) frr_primaries(tb, a.b.nh_mask + oi * a.b.W, np, p0);
  const uint32_t cnt = np >= 2 ? np : 0u;
  if (valid) a.eb_ptr[(size_t)pi * n_pfx + p] = cnt;
  uint32_t total;
  (void)gb_block_exclusive(cnt, s_scan, total);
  if (tid == 0) a.tile[(size_t)pi * gridDim.x + blockIdx.x] = total;
}

template <FrrProt P>
__device__ __forceinline__ void backup_ecmp_fill_body(const BackupEcmpArgs &a, const BackupEcmpProt<P> &pa) {
  constexpr bool SRLG = P == FrrProt::Srlg;
  constexpr uint32_t CW = be_cov_words(P);
  __shared__ uint64_t s_d[BE_SLOTS];                                     // [prefix of the batch][candidate of the chunk]
  __shared__ uint32_t s_cov[CW];
  __shared__ uint32_t s_ptr[LFA_TILE + 1];                               // the tile's eb_ptr values, from 0
  __shared__ uint32_t s_scan[GB_BLOCK];
  __shared__ uint16_t s_rank[LFA_TILE];                                  // prefix of the tile -> its place among the tile's ECMP prefixes
  __shared__ uint16_t s_list[LFA_TILE];                                  // ... and back
  __shared__ uint8_t s_miss[LFA_TILE];                                   // prefix of the tile: some primary got no backup
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.b.tab, a.b.scal, pi);
  const uint32_t K = tb.K, C = tb.C, W = a.b.W, n_pfx = a.b.n_pfx;
  if (tid < CW) s_cov[tid] = 0;
  s_miss[tid] = 0;
  BackupEcmpLane<P> ln;
  if constexpr (SRLG) ln.open(pa, pi, K);
  // the scans inside the tile: counts -> eb_ptr, ECMP bits -> the list
  const uint32_t p_first = blockIdx.x * LFA_TILE;
  const bool valid = p_first + tid < n_pfx;
  const size_t od = (size_t)pi * n_pfx + p_first + tid;
  const uint32_t cnt = valid ? a.eb_ptr[od] : 0u;
  uint32_t ttot, n_ecmp;
  const uint32_t loc = gb_block_exclusive(cnt, s_scan, ttot);
  __syncthreads();                                                       // (every lane has read the total: s_scan is free)
  const uint32_t rank = gb_block_exclusive(cnt ? 1u : 0u, s_scan, n_ecmp);
  const size_t ti = (size_t)pi * gridDim.x + blockIdx.x, n_tiles = (size_t)a.n_prot * gridDim.x;
  const uint32_t base = a.tile[ti];
  s_ptr[tid] = loc;
  s_rank[tid] = (uint16_t)rank;
  if (cnt) s_list[rank] = (uint16_t)tid;
  if (tid == 0) s_ptr[LFA_TILE] = ttot;
  if (valid) a.eb_ptr[od] = base + loc;
  if (ti + 1 == n_tiles && tid == 0) a.eb_ptr[(size_t)a.n_prot * n_pfx] = base + ttot;
  __syncthreads();
  const bool fill = (unsigned long long)a.tile[n_tiles] <= a.cap;        // else: the caller repeats the call with larger arrays
  const uint32_t todo = fill ? n_ecmp : 0u;                              // (uniform: the whole grid reads one word)

  const uint32_t CC = C < BE_SLOTS ? C : BE_SLOTS;                       // candidates per chunk
  const uint32_t B = C ? (BE_SLOTS / CC) : LFA_TILE;                     // prefixes per batch (C == 0: nothing is kept in LDS)
  const bool one_chunk = C <= BE_SLOTS;
  uint32_t my_cov = 0;                                                   // lane j, 1 <= j <= 6 (Srlg: and 8 <= j <= 10), of a wave: its count of entry bit j
  for (uint32_t b0 = 0; b0 < todo; b0 += B) {
    const uint32_t nb = todo - b0 < B ? todo - b0 : B;
    const uint32_t e_lo = s_ptr[s_list[b0]], e_hi = s_ptr[s_list[b0 + nb - 1u] + 1u];   // the batch's entries: one range
    for (uint32_t e0 = e_lo; e0 < e_hi; e0 += 256u) {
      const uint32_t e = e0 + tid;
      const bool live = e < e_hi;
      // this lane's (p, h)
      uint32_t pl = 0, h = 0, bp = 0, lo = 0, hi = 0, rlh = LFA_NONE, E = LFA_NONE;
      uint64_t dSp = 0, dEp = BK_NO_DIST;
      const uint64_t *pm = a.b.nh_mask;
      if (live) {
        uint32_t l2 = 0, h2 = LFA_TILE;                                  // the largest pl with s_ptr[pl] <= e: its count is not 0
        while (h2 - l2 > 1) {
          const uint32_t mid = (l2 + h2) >> 1;
          if (s_ptr[mid] <= e) l2 = mid; else h2 = mid;
        }
        pl = l2; bp = (uint32_t)s_rank[pl] - b0;
        const uint32_t p = p_first + pl;
        uint32_t r = e - s_ptr[pl];
        const size_t oi = (size_t)tb.srow * n_pfx + p;
        pm = a.b.nh_mask + oi * W;
        dSp = a.b.best_metric[oi];
        lo = a.b.pfx_ptr[p]; hi = a.b.pfx_ptr[p + 1];
        for (uint32_t w = 0; w < tb.Wk; ++w) {                           // the r-th primary
          uint64_t x = frr_word(tb, pm, w);
          const uint32_t c = (uint32_t)__popcll(x);
          if (r < c) {
            for (; r; --r) x &= x - 1;
            h = w * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
            break;
          }
          r -= c;
        }
        rlh = tb.rl[h]; E = tb.nbr[h];
        if (E != LFA_NONE && !one_chunk) dEp = bk_dist_to_prefix(a.b, tb.row[h], lo, hi);
      }
      if constexpr (SRLG) ln.entry(a.b, live, h, lo, hi);                // (no barrier inside)
      bool have = false, bnode = false, bprim = false, bdown = false;
      uint64_t bsum = 0;
      uint32_t bslot = LFA_NONE;
      for (uint32_t c0 = 0; c0 < C; c0 += CC) {                          // (one trip unless C > BE_SLOTS)
        const uint32_t cc = C - c0 < CC ? C - c0 : CC;
        if (!one_chunk || e0 == e_lo) {                                  // d_N(p) of the batch: once per prefix
          __syncthreads();                                               // s_d is free
          for (uint32_t i = tid; i < nb * cc; i += 256u) {
            const uint32_t q = i / cc, k = tb.cl[c0 + i - q * cc];
            const uint32_t p = p_first + s_list[b0 + q];
            bool own = false;
            const uint64_t d = bk_dist_to_prefix(a.b, tb.row[k], a.b.pfx_ptr[p], a.b.pfx_ptr[p + 1], tb.nbr[k], &own);
            s_d[i] = d == BK_NO_DIST ? BK_NO_DIST : d | (own ? BE_OWN : 0ull);
          }
          __syncthreads();
        }
        if (!live) continue;
        const uint64_t *sd = s_d + (size_t)bp * cc;
        if (one_chunk && E != LFA_NONE) {                                // d_E(p): the value of slot h itself
          uint32_t l2 = 0, h2 = C;
          while (h2 - l2 > 1) {
            const uint32_t mid = (l2 + h2) >> 1;
            if (tb.cl[mid] <= h) l2 = mid; else h2 = mid;
          }
          dEp = sd[l2] == BK_NO_DIST ? BK_NO_DIST : sd[l2] & BE_VAL;
        }
        for (uint32_t ci = 0; ci < cc; ++ci) {
          const uint32_t k = tb.cl[c0 + ci];
          if (k == h) continue;
          const uint64_t raw = sd[ci];
          const uint64_t d = raw == BK_NO_DIST ? BK_NO_DIST : raw & BE_VAL;
          if (!bk_less(d, tb.dns[k], dSp)) continue;                     // loop-free towards the prefix: ONE rule, a primary or not
          if ((tb.cf[k] & 1u) && !a.b.ignore_overload && !(raw & BE_OWN)) continue;
          if (tb.rl[k] == rlh) continue;                                 // shares the first link's fate
          if constexpr (SRLG) {                                          // every plain condition holds: now the group of h
            if (ln.mb.nm && !ln.mb.safe(k, tb.rl[k], d)) { ln.sfl |= 0x80u; continue; }
          }
          const bool nd = dEp != BK_NO_DIST && bk_less(d, tb.m[k * K + h], dEp);
          const bool pr = (pm[k >> 6] >> (k & 63u)) & 1ull;
          const uint64_t sum = (uint64_t)tb.cost[k] + d;
          if (!have || (nd && !bnode) || (nd == bnode && ((pr && !bprim) || (pr == bprim && sum < bsum)))) {   // ascending slot order
            have = true; bnode = nd; bprim = pr; bsum = sum; bslot = k; bdown = d < dSp;
          }
        }
      }
      uint32_t cv = 0;
      if (live) {
        uint32_t kind = 6u, slot = LFA_NONE, met = 0, fl = 0;
        if (have) {
          kind = 3u; slot = bslot;
          met = bsum > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)bsum;
          fl = (bnode ? 0x08u : 0u) | (bdown ? 0x10u : 0u) | (bprim ? 0x20u : 0u);
        } else if (a.b.ti_kind) {
          const size_t o = (size_t)pi * a.b.stride + h;
          const uint32_t tk = a.b.ti_kind[o];
          bool take = tk != 0;
          if constexpr (SRLG) {
            if (ln.mb.nm) {                                              // h has members: only repairs the caller vouches for
              take = take && pa.s.repairs;
              if (take && tk == 2u && ln.mb.forced(pa.s.ti_p[o], pa.s.ti_link[o])) { take = false; ln.sfl |= 0x02u; }
            }
          }
          if (take) { kind = tk == 1u ? 4u : 5u; slot = a.b.ti_via[o]; met = a.b.ti_metric[o]; }
        }
        if constexpr (SRLG) fl |= ln.sfl;
        const size_t g = (size_t)base + e;                               // < total <= cap
        a.eb_primary[g] = h; a.eb_kind[g] = (uint8_t)kind; a.eb_slot[g] = slot; a.eb_metric[g] = met; a.eb_flags[g] = (uint8_t)fl;
        if (kind == 6u) s_miss[pl] = 1;
        // entry | _LFA | node | downstream | a primary | repaired
        cv = 0x02u | (kind == 3u ? 0x04u : 0u) | (fl & 0x08u) | (fl & 0x10u) | (fl & 0x20u) | ((kind == 4u || kind == 5u) ? 0x40u : 0u);
        // Srlg: the primary has members | a slot was refused for them | the pair was refused
        if constexpr (SRLG) cv |= ((fl & 0x01u) << 8) | ((fl & 0x80u) << 2) | ((fl & 0x02u) << 9);
      }
#pragma unroll
      for (uint32_t j = 1; j <= 6; ++j) {
        const uint32_t c = (uint32_t)__popcll(__ballot((cv >> j) & 1u));
        if (lane == j) my_cov += c;
      }
      if constexpr (SRLG) {
#pragma unroll
        for (uint32_t j = EB_CW; j < CW; ++j) {
          const uint32_t c = (uint32_t)__popcll(__ballot((cv >> j) & 1u));
          if (lane == j) my_cov += c;
        }
      }
    }
  }
  if (my_cov) atomicAdd(&s_cov[lane], my_cov);                           // (only lanes 1 .. 6, Srlg: and 8 .. 10, hold a count)
  __syncthreads();                                                       // s_miss is complete
  const uint32_t dfl = (fill && cnt) ? 0x01u | (s_miss[tid] ? 0u : 0x80u) : 0u;   // ECMP prefix | every primary has a backup
  frr_cover<CW>(dfl, s_cov, a.eb_coverage + (size_t)pi * CW);
}

__global__ __launch_bounds__(256) void k_backup_ecmp_fill(BackupEcmpArgs a) { backup_ecmp_fill_body<FrrProt::Plain>(a, BackupEcmpProt<FrrProt::Plain>{}); }
__global__ __launch_bounds__(256) void k_backup_ecmp_fill_srlg(BackupEcmpArgs a, BackupEcmpProt<FrrProt::Srlg> pa) { backup_ecmp_fill_body<FrrProt::Srlg>(a, pa); }

}  // namespace
