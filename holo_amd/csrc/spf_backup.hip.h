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
// ONE body, backup_body<FrrProt P> (the modes: spf_frr_common.hip.h): the route and primaries prologue, the chunked stream of d_N(p)
// with the own bits, the word flush of the two sets, the loop-free and the overload test, the walk over the primaries of an ECMP
// prefix, the pick rule and the epilogue that chooses between the alternate and the per-link repair stand here once.  A mode adds
// BackupProt<P>, its kernel arguments, and BackupLane<P>, its lane state with four hooks (below, in front of the body).
//   k_backup       Plain: everything but the counts.
//   k_backup_lan   Lan (hspf_routes_backup_lan_device): d_L(p) of the one primary's LAN is computed once next to d_E(p); a candidate
//                  that has passed every plain condition is then held against d(N, L) + d_L(p); the per-link repair is taken for a
//                  point-to-point primary, and for a LAN primary only under HSPF_LFA_LAN_SAFE_REPAIRS (the caller's word that the
//                  repairs come from hspf_rlfa_lan_device's tables).
//   k_backup_srlg  Srlg (hspf_routes_backup_srlg_device): spf_backup_srlg.hip.h.
//   k_backup_cov_t<P>   the coverage of every protection mode P: a wave counts the kinds of its
//                  prefixes, and the mode's bits of bk_flags, with ballots (grid-stride over the tiles of one protected root),
//                  then one vector atomic add per wave and word.
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
  uint32_t n_pfx, sat, pad0, pad1;
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

// The mode's kernel arguments and its lane state (FrrProt, spf_frr_common.hip.h).  A lane has four hooks into backup_body:
//   open        in front of the chunks: the mode's view of the root, what it keeps about the primaries of the prefix;
//   one         one primary, candidate k (root_link rlk, d_{N_k}(p) = d) has passed every plain condition: may it stay?
//   ecmp        the same behind the walk over two or more primaries;
//   may_repair / repair / flags   the epilogue: may the per-link repair be looked at, may the one found (kind tk, at o) be taken,
//               and the mode's bits of bk_flags.
// STREAMS_DE: open() computes d_E(p) of the one primary in a stream of its own (Srlg: next to the members' rows).
// The Srlg specialisations stand in spf_backup_srlg.hip.h, next to the member lane they use.
template <FrrProt P> struct BackupProt {};
template <> struct BackupProt<FrrProt::Lan> { LanArgs la; uint32_t lan_repairs, pad; };   // lan_repairs: HSPF_LFA_LAN_SAFE_REPAIRS
template <FrrProt P> struct BackupLane {
  static constexpr bool STREAMS_DE = false;
  __device__ __forceinline__ void open(const BackupArgs &, const BackupProt<P> &, const FrrTab &, uint32_t, const uint64_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t &) {}
  __device__ __forceinline__ bool one(uint32_t, uint32_t, uint64_t) { return true; }
  __device__ __forceinline__ bool ecmp(const BackupArgs &, const FrrTab &, const uint64_t *, uint32_t, uint32_t, uint64_t, uint32_t, uint32_t) { return true; }
  __device__ __forceinline__ bool may_repair(const BackupProt<P> &) const { return true; }
  __device__ __forceinline__ bool repair(const BackupProt<P> &, size_t, uint32_t) { return true; }
  __device__ __forceinline__ uint32_t flags() const { return 0u; }
};
// Lan: d_L(p) of the one primary's LAN is computed once, in front of the chunks; a candidate is held against d(N, L) + d_L(p)
template <> struct BackupLane<FrrProt::Lan> {
  static constexpr bool STREAMS_DE = false;
  LanTab lt;
  uint32_t li0 = LFA_NONE, lfl = 0;                                                // the one primary's LAN; HSPF_LFA_LAN_PRIMARY | _REFUSED
  uint64_t dL0p = BK_NO_DIST;
  bool lanp = false;                                                               // some primary crosses a LAN of S

  __device__ __forceinline__ void open(const BackupArgs &a, const BackupProt<FrrProt::Lan> &pa, const FrrTab &tb, uint32_t pi, const uint64_t *pm,
                                       uint32_t np, uint32_t p0, uint32_t lo, uint32_t hi, uint64_t &) {
    lt = lan_tab(pa.la, pi, tb.K);
    if (np == 1) {
      li0 = lt.li[p0];
      lanp = li0 != LFA_NONE;
      if (lanp) dL0p = bk_dist_to_prefix(a, lt.lrow[p0], lo, hi);
    } else if (np >= 2) lanp = lan_any_primary(tb, lt, pm);
    if (lanp) lfl |= 0x20u;
  }
  __device__ __forceinline__ bool one(uint32_t k, uint32_t, uint64_t d) {
    if (!lanp || (dL0p != BK_NO_DIST && bk_less(d, lt.ml[k * lt.NL + li0], dL0p))) return true;
    lfl |= 0x40u;
    return false;
  }
  __device__ __forceinline__ bool ecmp(const BackupArgs &a, const FrrTab &tb, const uint64_t *pm, uint32_t k, uint32_t, uint64_t d, uint32_t lo, uint32_t hi) {
    if (!lanp) return true;
    const bool ok = frr_all_primaries(tb, pm, [&](uint32_t q) {
      const uint32_t j = lt.li[q];
      if (j == LFA_NONE) return true;
      const uint64_t dLp = bk_dist_to_prefix(a, lt.lrow[q], lo, hi);
      return dLp != BK_NO_DIST && bk_less(d, lt.ml[k * lt.NL + j], dLp);
    });
    if (!ok) lfl |= 0x40u;
    return ok;
  }
  __device__ __forceinline__ bool may_repair(const BackupProt<FrrProt::Lan> &pa) const { return !lanp || pa.lan_repairs; }   // (a LAN primary: only repairs the caller vouches for)
  __device__ __forceinline__ bool repair(const BackupProt<FrrProt::Lan> &, size_t, uint32_t) { return true; }
  __device__ __forceinline__ uint32_t flags() const { return lfl; }
};

template <FrrProt P>
__device__ __forceinline__ void backup_body(const BackupArgs &a, const BackupProt<P> &pa) {
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
    if (!BackupLane<P>::STREAMS_DE && E0 != LFA_NONE) dE0p = bk_dist_to_prefix(a, tb.row[p0], lo, hi);
  }
  BackupLane<P> ln;
  ln.open(a, pa, tb, pi, pm, np, p0, lo, hi, dE0p);
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
      const uint32_t rlk = tb.rl[k];
      if (np == 1) {
        ok = rlk != rl0 && ln.one(k, rlk, d);                                      // (k == p0 has p0's root_link); then the mode
        nd = ok && E0 != LFA_NONE && dE0p != BK_NO_DIST && bk_less(d, tb.m[k * K + p0], dE0p);
      } else {
        ok = !((pm[k >> 6] >> (k & 63u)) & 1ull);
        uint32_t n_router = 0;
        bool all = true;
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
          }
        }
        ok = ok && ln.ecmp(a, tb, pm, k, rlk, d, lo, hi);
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
    } else if (a.ti_kind && ln.may_repair(pa)) {
      const size_t o = (size_t)pi * a.stride + p0;
      const uint32_t tk = a.ti_kind[o];
      if (tk && ln.repair(pa, o, tk)) { kind = tk == 1u ? 4u : 5u; slot = a.ti_via[o]; met = a.ti_metric[o]; }
    }
  }
  fl |= ln.flags();
  a.bk_kind[oo] = (uint8_t)kind; a.bk_primary[oo] = prim; a.bk_slot[oo] = slot; a.bk_metric[oo] = met; a.bk_flags[oo] = (uint8_t)fl;
}

__global__ __launch_bounds__(256) void k_backup(BackupArgs a) { backup_body(a, BackupProt<FrrProt::Plain>{}); }
__global__ __launch_bounds__(256) void k_backup_lan(BackupArgs a, BackupProt<FrrProt::Lan> pa) { backup_body(a, pa); }

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
