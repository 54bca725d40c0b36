// spf_backup.hip.h — per-prefix backup routes: the loop-free alternates of RFC 5286 section 6.1 evaluated against the neighbours'
// distances to the PREFIX (the minimum over its advertisers), with the per-link repair of hspf_tilfa_device as the fallback
// (hspf_routes_backup_device; the semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  lane = prefix, 256 consecutive prefixes per workgroup, blockIdx.y = the protected root: the route (best_metric,
// best_entry, nexthop_mask) is read and every output is written coalesced.  The candidate slots are walked in chunks of BK_CH
// (as k_rlfa walks the protected slots): per chunk the lane keeps d_N(p) of its BK_CH neighbours in registers and streams the
// prefix's entries ONCE — per entry (v, m) one gather dist[nbr_row[k]][v] per slot of the chunk; slot, row and neighbour are
// wave-uniform (scalar registers), only v differs between lanes.  Nothing that scales with K or with the number of advertisers
// lives in registers.  d_E(p) of the one primary is computed once, in front of the chunks; an ECMP prefix (whose sets are
// written, no slot is chosen) streams its entries again per chunk and primary.
//   k_backup       everything but the counts.
//   k_backup_cov_t<P>   the coverage of every protection mode P (FrrProt, spf_frr_common.hip.h): a wave counts the kinds of its
//                  prefixes, and the mode's bits of bk_flags, with ballots (grid-stride over the tiles of one protected root),
//                  then one vector atomic add per wave and word.
// The LAN variant (hspf_routes_backup_lan_device) is k_backup_lan, a further instantiation of the same body: d_L(p) of the one
// primary's LAN is computed once next to d_E(p); a candidate that has passed every plain
// condition is then held against d(N, L) + d_L(p); the per-link repair is taken for a point-to-point primary, and for a LAN
// primary only under HSPF_LFA_LAN_SAFE_REPAIRS (the caller's word that the repairs come from hspf_rlfa_lan_device's tables).
// There is no wave-per-prefix path: a prefix with very many advertisers is walked by ONE lane and holds its wave back.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_frr_common.hip.h"

namespace {

constexpr uint32_t BK_CH = 8;                      // candidate slots per chunk
constexpr uint64_t BK_NO_DIST = ~0ull;             // d_X(p): no advertiser of p is reached from X
constexpr uint32_t BK_KINDS = 7;                   // HSPF_BK_*

struct BackupArgs {
  uint32_t n, W, ignore_overload, stride;                                  // stride = 64 * W slots per protected root
  uint32_t n_pfx, sat, lan_repairs, pad1;                                   // lan_repairs: HSPF_LFA_LAN_SAFE_REPAIRS (k_backup_lan)
  const uint32_t *dist; const uint16_t *flags;                             // the table set
  const uint32_t *tab, *scal;                                              // as LfaArgs (staged by the call, gathered by k_lfa_gather)
  const uint32_t *pfx_ptr, *pfx_vertex, *pfx_metric;                       // the staged prefix table
  const uint32_t *best_metric, *best_entry; const uint64_t *nh_mask;       // hspf_routes of the same table set
  const uint8_t *ti_kind; const uint32_t *ti_via, *ti_metric;              // hspf_tilfa_out's per-slot arrays, or NULL
  uint8_t *bk_kind; uint32_t *bk_primary, *bk_slot, *bk_metric; uint8_t *bk_flags;
  uint64_t *cand_mask, *node_mask; uint32_t *coverage;
};

// one term d(X, v) + m of d_X(p); BK_NO_DIST when v is not in X's SPT.  Args: BackupArgs, or BackupNodeArgs (spf_backup_node.hip.h)
template <class Args>
__device__ __forceinline__ uint64_t bk_term(const Args &a, size_t xv, uint32_t m) {
  const uint32_t d = a.dist[xv];
  if (!(a.flags[xv] & 1u) || d == LFA_NONE) return BK_NO_DIST;
  const uint64_t s = (uint64_t)d + m;
  return (a.sat && s > 0xFFFFFFFFull) ? 0xFFFFFFFFull : s;
}

// d_X(p) for the row of X: the entries lo .. hi streamed once.  With `own`: does the entry of X itself attain it?
template <class Args>
__device__ __forceinline__ uint64_t bk_dist_to_prefix(const Args &a, uint32_t row, uint32_t lo, uint32_t hi, uint32_t X = LFA_NONE, bool *own = nullptr) {
  uint64_t best = BK_NO_DIST;
  bool mine = false;
  const size_t base = (size_t)row * a.n;
  for (uint32_t e = lo; e < hi; ++e) {
    const uint32_t v = a.pfx_vertex[e];
    const uint64_t t = bk_term(a, base + v, a.pfx_metric[e]);
    if (t < best) { best = t; mine = v == X; }
    else if (t == best && v == X && t != BK_NO_DIST) mine = true;
  }
  if (own) *own = mine;
  return best;
}

// `x < b + c` in 64 bits; x == BK_NO_DIST or b "not reached" makes it false (c is a number: a route's metric or a d_E(p) that exists)
__device__ __forceinline__ bool bk_less(uint64_t x, uint32_t b, uint64_t c) {
  return x != BK_NO_DIST && b != LFA_NONE && x < (uint64_t)b + c;
}

template <bool LAN>
__device__ __forceinline__ void backup_body(const BackupArgs &a, const LanArgs &la) {
  const uint32_t pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const uint32_t K = tb.K, C = tb.C, n = a.n, W = a.W, Wk = tb.Wk;
  const uint32_t p = blockIdx.x * LFA_TILE + threadIdx.x;
  if (p >= a.n_pfx) return;                                                        // (no barrier below)
  const size_t oi = (size_t)tb.srow * a.n_pfx + p, oo = (size_t)pi * a.n_pfx + p;
  const uint32_t lo = a.pfx_ptr[p], hi = a.pfx_ptr[p + 1];
  const bool route = a.best_entry[oi] != LFA_NONE;
  const uint64_t dSp = a.best_metric[oi];
  const uint64_t *pm = a.nh_mask + oi * W;
  uint32_t np = 0, p0 = 0;
  if (route) frr_primaries(tb, pm, np, p0);
  uint32_t kind = !route ? 0u : np == 0 ? 1u : np >= 2 ? 2u : 6u;
  const bool sets = kind >= 2;                                                     // the two sets are evaluated and written
  uint32_t rl0 = LFA_NONE, E0 = LFA_NONE;
  uint64_t dE0p = BK_NO_DIST;
  if (np == 1) {
    rl0 = tb.rl[p0]; E0 = tb.nbr[p0];
    if (E0 != LFA_NONE) dE0p = bk_dist_to_prefix(a, tb.row[p0], lo, hi);
  }
  LanTab lt{};
  uint32_t li0 = LFA_NONE, lfl = 0;                                                // LAN: the one primary's LAN; the two LAN bits
  uint64_t dL0p = BK_NO_DIST;
  bool lanp = false;                                                               // LAN: some primary crosses a LAN of S
  if constexpr (LAN) {
    lt = lan_tab(la, pi, K);
    if (np == 1) {
      li0 = lt.li[p0];
      lanp = li0 != LFA_NONE;
      if (lanp) dL0p = bk_dist_to_prefix(a, lt.lrow[p0], lo, hi);
    } else if (np >= 2) lanp = lan_any_primary(tb, lt, pm);
    if (lanp) lfl |= 0x20u;
  }
  bool have = false, bnode = false, bdown = false;
  uint64_t bsum = 0, cw = 0, nw = 0;
  uint32_t aslot = LFA_NONE, wi = 0;                                               // wi: the word of the sets that cw / nw stand for
  for (uint32_t c0 = 0; c0 < C; c0 += BK_CH) {
    // d_N(p) of the chunk's neighbours: the entries streamed once; own bit j: N_j's own entry attains d_{N_j}(p)
    uint64_t dNp[BK_CH];
    uint32_t own = 0;
#pragma unroll
    for (uint32_t j = 0; j < BK_CH; ++j) dNp[j] = BK_NO_DIST;
    if (sets)
      for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t v = a.pfx_vertex[e], met = a.pfx_metric[e];
#pragma unroll
        for (uint32_t j = 0; j < BK_CH; ++j) {
          if (c0 + j >= C) break;
          const uint32_t k = tb.cl[c0 + j];
          const uint64_t t = bk_term(a, (size_t)tb.row[k] * n + v, met);
          const bool mine = v == tb.nbr[k];
          if (t < dNp[j]) { dNp[j] = t; own = (own & ~(1u << j)) | ((mine ? 1u : 0u) << j); }
          else if (t == dNp[j] && mine && t != BK_NO_DIST) own |= 1u << j;
        }
      }
#pragma unroll
    for (uint32_t j = 0; j < BK_CH; ++j) {
      if (c0 + j >= C) break;
      const uint32_t k = tb.cl[c0 + j];                                            // ascending, the same for every lane
      while (wi < (k >> 6)) {                                                      // the words in front of slot k are complete
        if (a.cand_mask) a.cand_mask[oo * W + wi] = cw;
        if (a.node_mask) a.node_mask[oo * W + wi] = nw;
        cw = 0; nw = 0; ++wi;
      }
      if (!sets) continue;
      const uint64_t d = dNp[j];
      if (!bk_less(d, tb.dns[k], dSp)) continue;                                   // loop-free with respect to the prefix
      if ((tb.cf[k] & 1u) && !a.ignore_overload && !((own >> j) & 1u)) continue;   // an overloaded neighbour carries no transit traffic
      bool ok, nd = false;
      if (np == 1) {
        ok = tb.rl[k] != rl0;                                                      // (k == p0 has p0's root_link)
        if constexpr (LAN) {                                                       // every plain condition holds: now the pseudonode
          if (ok && lanp && !(dL0p != BK_NO_DIST && bk_less(d, lt.ml[k * lt.NL + li0], dL0p))) { ok = false; lfl |= 0x40u; }
        }
        nd = ok && E0 != LFA_NONE && dE0p != BK_NO_DIST && bk_less(d, tb.m[k * K + p0], dE0p);
      } else {
        ok = !((pm[k >> 6] >> (k & 63u)) & 1ull);
        uint32_t n_router = 0;
        bool all = true, lanok = true;
        const uint32_t rlk = tb.rl[k];
        for (uint32_t w2 = 0; w2 < Wk && ok; ++w2) {
          uint64_t x = frr_word(tb, pm, w2);
          while (x) {
            const uint32_t q = w2 * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
            x &= x - 1;
            if (tb.rl[q] == rlk) { ok = false; break; }
            if (tb.nbr[q] != LFA_NONE) {
              ++n_router;
              if (all) {
                const uint64_t dEp = bk_dist_to_prefix(a, tb.row[q], lo, hi);
                all = dEp != BK_NO_DIST && bk_less(d, tb.m[k * K + q], dEp);
              }
            }
            if constexpr (LAN) {
              if (lanp && lanok) {
                const uint32_t j = lt.li[q];
                if (j != LFA_NONE) {
                  const uint64_t dLp = bk_dist_to_prefix(a, lt.lrow[q], lo, hi);
                  lanok = dLp != BK_NO_DIST && bk_less(d, lt.ml[k * lt.NL + j], dLp);
                }
              }
            }
          }
        }
        if constexpr (LAN) {
          if (ok && !lanok) { ok = false; lfl |= 0x40u; }
        }
        nd = ok && n_router && all;
      }
      if (!ok) continue;
      cw |= 1ull << (k & 63u);
      if (nd) nw |= 1ull << (k & 63u);
      if (np == 1) {
        const uint64_t sum = (uint64_t)tb.cost[k] + d;
        if (!have || (nd && !bnode) || (nd == bnode && sum < bsum)) {              // ascending slot order: a tie keeps the smaller slot
          have = true; bnode = nd; bsum = sum; aslot = k; bdown = d < dSp;
        }
      }
    }
  }
  for (; wi < W; ++wi) {                                                           // the last word with candidates, and what lies behind
    if (a.cand_mask) a.cand_mask[oo * W + wi] = cw;
    if (a.node_mask) a.node_mask[oo * W + wi] = nw;
    cw = 0; nw = 0;
  }
  uint32_t prim = LFA_NONE, slot = LFA_NONE, met = 0, fl = 0;
  if (np == 1) {
    prim = p0;
    if (have) {
      kind = 3u; slot = aslot;
      met = bsum > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)bsum;
      fl = (bnode ? 0x08u : 0u) | (bdown ? 0x10u : 0u);
    } else if (a.ti_kind && !(LAN && lanp && !a.lan_repairs)) {                             // (a LAN primary: only repairs the caller vouches for)
      const size_t o = (size_t)pi * a.stride + p0;
      const uint32_t tk = a.ti_kind[o];
      if (tk) { kind = tk == 1u ? 4u : 5u; slot = a.ti_via[o]; met = a.ti_metric[o]; }
    }
  }
  if constexpr (LAN) fl |= lfl;
  a.bk_kind[oo] = (uint8_t)kind; a.bk_primary[oo] = prim; a.bk_slot[oo] = slot; a.bk_metric[oo] = met; a.bk_flags[oo] = (uint8_t)fl;
}

__global__ __launch_bounds__(256) void k_backup(BackupArgs a) { backup_body<false>(a, LanArgs{}); }
__global__ __launch_bounds__(256) void k_backup_lan(BackupArgs a, LanArgs la) { backup_body<true>(a, la); }

// coverage[pi][]: the seven kinds, then the prefixes with one bit of bk_flags each:
//   Lan   HSPF_LFA_LAN_PRIMARY, HSPF_LFA_LAN_REFUSED;   Srlg   HSPF_BK_SRLG_PRIMARY, HSPF_LFA_SRLG_REFUSED, HSPF_BK_SRLG_PAIR_REFUSED
constexpr uint32_t bk_cov_words(FrrProt P) { return BK_KINDS + (P == FrrProt::Plain ? 0u : P == FrrProt::Lan ? 2u : 3u); }
constexpr uint32_t bk_cov_flag(FrrProt P, uint32_t j) { return P == FrrProt::Lan ? 0x20u << j : j == 0 ? 0x01u : j == 1 ? 0x80u : 0x02u; }

// ballots per tile, the counts kept in lanes 0 .. CW - 1, one vector atomic add per wave and word
template <FrrProt P>
__global__ __launch_bounds__(256) void k_backup_cov_t(BackupArgs a) {
  constexpr uint32_t CW = bk_cov_words(P);
  const uint32_t pi = blockIdx.y, lane = threadIdx.x & 63u;
  const uint8_t *kinds = a.bk_kind + (size_t)pi * a.n_pfx, *fls = a.bk_flags + (size_t)pi * a.n_pfx;
  uint32_t mine = 0;
  for (uint32_t t0 = blockIdx.x * 256u; t0 < a.n_pfx; t0 += gridDim.x * 256u) {    // t0 + 255 is the last prefix of the workgroup's tile
    const uint32_t p = t0 + threadIdx.x;
    const uint32_t kind = p < a.n_pfx ? kinds[p] : BK_KINDS;
    uint32_t fl = 0;
    if constexpr (P != FrrProt::Plain) fl = p < a.n_pfx ? fls[p] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < CW; ++j) {
      const bool hit = j < BK_KINDS ? kind == j : (fl & bk_cov_flag(P, j - BK_KINDS)) != 0;
      const uint32_t c = (uint32_t)__popcll(__ballot(hit));
      if (lane == j) mine += c;
    }
  }
  if (lane < CW && mine) atomicAdd(a.coverage + (size_t)pi * CW + lane, mine);
}
constexpr auto k_backup_cov = k_backup_cov_t<FrrProt::Plain>;
constexpr auto k_backup_cov_lan = k_backup_cov_t<FrrProt::Lan>;
constexpr auto k_backup_cov_srlg = k_backup_cov_t<FrrProt::Srlg>;

}  // namespace
