// spf_frr_common.hip.h — what the fast-reroute kernels share (spf_lfa / spf_rlfa / spf_tilfa / spf_backup .hip.h): the staged
// candidate table of a protected root as ONE view, the scan of a destination's primaries, and the coverage tail.
//
// The staged table (written by lfa_stage in spf_frr.hip.h, read here and nowhere else).  `tab` is one block of u32 words:
//   [n_prot][LFA_HDR_WORDS] headers, one per protected root:
//       word 0  S       the root's vertex
//       word 1  srow    the row of S's SPT in the table set
//       word 2  K       its first-hop slots
//       word 3  C       how many of them are candidates (nbr != LFA_NONE)
//       word 4  offset (in words, from `tab`) of the root's slot arrays
//       word 5  offset (in words, from `scal`) of the root's scalars
//       word 6, 7  0
//   then per root, at its offset, FRR_COLS columns of K words each, in this order:
//       nbr | row | cost | root_link | cflags | candidate list
//     nbr[k] the router behind slot k (LFA_NONE: no candidate), row[k] the row of its SPT, cost[k] the cost of the path the slot
//     stands for, root_link[k] the link of S's own row that starts it, cflags[k] HSPF_LFA_C_*; the candidate list holds the C
//     candidate slots in ascending order (its other K - C words are 0).
// `scal` is k_lfa_gather's block, per root at its offset:  d(N_k, S) [K] | d(N_k, N_p) [K][K]   (LFA_NONE where a slot is no
// candidate or the vertex is not reached).
//
// The LAN block of the calls that protect broadcast links (hspf_lfa_lan_device, hspf_routes_backup_lan_device) is a SECOND pair of
// blocks next to these, written by lan_stage in spf_frr.hip.h; the layout above does not change.  `ltab`:
//   [n_prot][LAN_HDR_WORDS] headers:  word 0  NL  the distinct LANs of the root's slots
//                                     word 1  offset (in words, from `ltab`) of the root's LAN columns
//                                     word 2  offset (in words, from `lscal`) of the root's LAN scalars;   word 3  0
//   then per root, at its offset:  li [K] | lrow [K] | lv [NL]
//     li[k] the index (< NL) of the LAN that slot k crosses, LFA_NONE for a point-to-point slot; lrow[k] the row of the SPT rooted
//     at that LAN's vertex; lv[j] the vertex of LAN j.
// `lscal` is the LAN part of k_lfa_gather_lan's output, per root at its offset:  d(N_k, lv[j]) [K][NL]  (LFA_NONE where slot k is no
// candidate).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t LFA_HDR_WORDS = 8;
constexpr uint32_t LFA_NONE = 0xFFFFFFFFu;
constexpr uint32_t LFA_TILE = 256;
constexpr uint32_t FRR_COLS = 6;           // columns of a root's table: what frr_tab_over names, lfa_stage writes and k_lfa<true> copies

constexpr uint32_t LAN_HDR_WORDS = 4;

// `a < b + c` in 64 bits; any term "not reached" makes it false
__device__ __forceinline__ bool lfa_less(uint32_t a, uint32_t b, uint32_t c) {
  return a != LFA_NONE && b != LFA_NONE && c != LFA_NONE && (uint64_t)a < (uint64_t)b + (uint64_t)c;
}

// the table of one protected root; dns / m are NULL in a view made without the scalars
struct FrrTab {
  uint32_t S, srow, K, C;
  uint32_t Wk;                                          // mask words that hold the K slots
  uint64_t last_word;                                   // the slots of word Wk - 1 that exist
  const uint32_t *cols;                                 // all FRR_COLS columns, contiguous: cols[0 .. FRR_COLS * K)
  const uint32_t *nbr, *row, *cost, *rl, *cf, *cl;      // each of them
  const uint32_t *dns, *m;                              // d(N_k, S) [K] | d(N_k, N_p) [K][K]
};

// a view over explicit bases: `cols` = the columns, wherever they sit (k_lfa<true>: its LDS copy)
__device__ __forceinline__ FrrTab frr_tab_over(uint32_t S, uint32_t srow, uint32_t K, uint32_t C, const uint32_t *cols, const uint32_t *dns,
                                               const uint32_t *m) {
  const uint64_t last_word = (K & 63u) ? ((1ull << (K & 63u)) - 1ull) : ~0ull;
  static_assert(FRR_COLS == 6, "a new column is named here, in FrrTab and in lfa_stage");
  return FrrTab{S, srow, K, C, (K + 63u) >> 6, last_word, cols, cols, cols + K, cols + 2 * K, cols + 3 * K, cols + 4 * K, cols + 5 * K, dns, m};
}

// where the scalars of protected root `pi` start in `scal` (k_lfa_gather writes there)
__device__ __forceinline__ uint32_t frr_scal_offset(const uint32_t *tab, uint32_t pi) { return tab[(size_t)pi * LFA_HDR_WORDS + 5]; }

// protected root `pi` of the staged block, without / with its scalars
__device__ __forceinline__ FrrTab frr_tab(const uint32_t *tab, uint32_t pi) {
  const uint32_t *hdr = tab + (size_t)pi * LFA_HDR_WORDS;
  return frr_tab_over(hdr[0], hdr[1], hdr[2], hdr[3], tab + hdr[4], nullptr, nullptr);
}
__device__ __forceinline__ FrrTab frr_tab(const uint32_t *tab, const uint32_t *scal, uint32_t pi) {
  FrrTab t = frr_tab(tab, pi);
  t.dns = scal + frr_scal_offset(tab, pi);
  t.m = t.dns + t.K;
  return t;
}

// word w of a next-hop mask, clipped to the K slots that exist
__device__ __forceinline__ uint64_t frr_word(const FrrTab &t, const uint64_t *pm, uint32_t w) {
  return pm[w] & (w + 1 == t.Wk ? t.last_word : ~0ull);
}

// the primaries of a destination: how many, and the first one
__device__ __forceinline__ void frr_primaries(const FrrTab &t, const uint64_t *pm, uint32_t &np, uint32_t &p0) {
  np = 0; p0 = 0;
  for (uint32_t w = 0; w < t.Wk; ++w) {
    const uint64_t x = frr_word(t, pm, w);
    if (x && !np) p0 = w * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
    np += (uint32_t)__popcll(x);
  }
}

// f(q) for the primaries q of a destination in ascending order, until one returns false: did every one return true?
template <class F>
__device__ __forceinline__ bool frr_all_primaries(const FrrTab &t, const uint64_t *pm, F &&f) {
  for (uint32_t w = 0; w < t.Wk; ++w) {
    uint64_t x = frr_word(t, pm, w);
    while (x) {
      const uint32_t q = w * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
      x &= x - 1;
      if (!f(q)) return false;
    }
  }
  return true;
}

// What a call protects against on top of the link itself: nothing more, the pseudonode of a primary's LAN (RFC 5286 section 3.3),
// or the shared-risk link group of a primary.  A kernel family has ONE body, a template over the mode; per family and mode
//   <Family>Prot<P>   the kernel arguments of the mode (empty for Plain), passed to the kernel next to the family's own;
//   <Family>Lane<P>   what a lane keeps for the mode next to the body's own state (empty for Plain), with the mode's conditions
//                     as members where they are more than a line;
// selected with `if constexpr`: an instantiation holds nothing of another mode.  The Srlg specialisations stand in spf_srlg.hip.h,
// next to the member block they read, and the Srlg kernels are instantiated there.  (Folded: lfa_body in spf_lfa.hip.h, backup_body and
// k_backup_cov_t in spf_backup.hip.h, backup_ecmp_fill_body in spf_backup_ecmp.hip.h.)
enum class FrrProt { Plain, Lan, Srlg };

// the LAN block of the call (both NULL in a call without one), and the view of one protected root over it
struct LanArgs { const uint32_t *ltab; uint32_t *lscal; };
struct LanTab {
  uint32_t NL;
  const uint32_t *li, *lrow, *lv;                       // [K] | [K] | [NL]
  const uint32_t *ml;                                   // d(N_k, lv[j]) [K][NL]
};
__device__ __forceinline__ LanTab lan_tab(const LanArgs &la, uint32_t pi, uint32_t K) {
  const uint32_t *hdr = la.ltab + (size_t)pi * LAN_HDR_WORDS;
  const uint32_t *c = la.ltab + hdr[1];
  return LanTab{hdr[0], c, c + K, c + 2 * K, la.lscal + hdr[2]};
}

// does any primary of the destination cross a LAN of S?
__device__ __forceinline__ bool lan_any_primary(const FrrTab &t, const LanTab &lt, const uint64_t *pm) {
  bool any = false;
  for (uint32_t w = 0; w < t.Wk; ++w) {
    uint64_t x = frr_word(t, pm, w);
    while (x) {
      const uint32_t p = w * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
      x &= x - 1;
      any = any || lt.li[p] != LFA_NONE;
    }
  }
  return any;
}

// The coverage tail of a lane-per-destination kernel: bit j of `fl` counts towards out[j], j < NC.  Wave ballots + popcounts, one
// LDS add per wave, one vector atomic add per workgroup and counter.  s_cov[NC] is the workgroup's, zeroed in front of an
// earlier barrier; every thread of the workgroup comes here (there is a barrier inside).
template <uint32_t NC>
__device__ __forceinline__ void frr_cover(uint32_t fl, uint32_t *s_cov, uint32_t *out) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  uint32_t my_cov = 0;                                  // lane j < NC of a wave: its count of flag bit j
#pragma unroll
  for (uint32_t j = 0; j < NC; ++j) {
    const uint32_t c = (uint32_t)__popcll(__ballot((fl >> j) & 1u));
    if (lane == j) my_cov = c;
  }
  if (lane < NC && my_cov) atomicAdd(&s_cov[lane], my_cov);
  __syncthreads();
  if (tid < NC && s_cov[tid]) atomicAdd(out + tid, s_cov[tid]);
}

}  // namespace
