// spf_lfa.hip.h — loop-free alternates (RFC 5286) per (protected root, destination) from the SPT rows of the root and of its
// neighbour routers (hspf_lfa_device; the semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  The work per (S, D) is C loads d(N_k, D) — one per candidate, from C row-major rows — a few compares, two bit sets
// and one selection: a streaming kernel whose floor is the bytes of the rows it reads and of the outputs it writes.
//   k_lfa_gather   once per protected root: the scalars that do not depend on D — d(N_k, S) and the K x K matrix d(N_k, N_p) —
//                  gathered from the tables into a small scratch block (K + K*K words), so that the streaming kernel never
//                  issues a scattered load for them.
//   k_lfa<ONE>     lane = destination, 256 consecutive D per workgroup: every row load is coalesced (consecutive D of
//                  one row).  Nothing is held per candidate in registers (K reaches 128 and beyond): a candidate is loaded,
//                  judged, folded into the running best and into the current u64 word of the two sets, and forgotten.  The
//                  primaries' d(E, D) is kept when there is ONE primary (the only case that selects an alternate) and re-read
//                  — from L2: the row was just streamed — for ECMP destinations.
//                  ONE = true: every protected root of the call has at most 64 slots (one mask word): the slot tables and
//                  the K x K matrix sit in LDS (at most 18.3 KB), the sets are two registers.  ONE = false: any K, tables
//                  and matrix are read through the caches (K = 128: 64 KB of matrix, L2-resident), the sets are produced
//                  word by word.
// One source per kernel: lfa_body<ONE, P> is every streaming kernel, P the protection mode (FrrProt, spf_frr_common.hip.h);
// k_lfa<ONE>, k_lfa_lan<ONE> and k_lfa_srlg<ONE> (spf_srlg.hip.h, with the Srlg mode's conditions) are its instantiations.
// The LAN variants (hspf_lfa_lan_device: RFC 5286 section 3.3, loop-freeness with respect to the pseudonode of a primary's LAN)
// are k_lfa_gather_lan and k_lfa_lan<ONE>.  The gather adds d(N_k, L) for the
// distinct LANs L of S — a [K][NL] block indexed by a compact LAN index, not a second K x K matrix — and the streaming kernel
// reads it through the caches, only for a candidate that has passed every plain condition at a destination whose primary
// crosses a LAN: the LDS footprint of ONE = true is that of k_lfa<true> (plus two coverage words), and a table set without LANs
// never evaluates a LAN term.  d(L, D) of the one primary is one more coalesced row read, like d(E, D).
// Coverage: wave ballots + popcounts, one LDS add per wave and one vector atomic add per workgroup and counter.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_frr_common.hip.h"

namespace {

struct LfaArgs {
  uint32_t n, W, ignore_overload, pad;
  const uint32_t *dist; const uint16_t *flags; const uint64_t *mask;     // the table set
  const uint32_t *tab;                 // the staged candidate tables (spf_frr_common.hip.h)
  uint32_t *scal;                      // k_lfa_gather's block of scalars (the same)
  uint32_t *alt_slot, *alt_metric; uint8_t *alt_flags; uint64_t *cand_mask, *node_mask; uint32_t *coverage;
};

template <bool LAN>
__device__ __forceinline__ void lfa_gather_body(const LfaArgs &a, const LanArgs &la) {
  const FrrTab tb = frr_tab(a.tab, blockIdx.y);
  const uint32_t S = tb.S, K = tb.K;
  uint32_t *out = a.scal + frr_scal_offset(a.tab, blockIdx.y);
  const uint32_t total = K + K * K;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    uint32_t v = LFA_NONE;
    if (i < K) {
      if (tb.nbr[i] != LFA_NONE) v = a.dist[(size_t)tb.row[i] * a.n + S];
    } else {
      const uint32_t k = (i - K) / K, p = (i - K) - k * K;
      if (tb.nbr[k] != LFA_NONE && tb.nbr[p] != LFA_NONE) v = a.dist[(size_t)tb.row[k] * a.n + tb.nbr[p]];
    }
    out[i] = v;
  }
  if constexpr (LAN) {                                                             // d(N_k, L_j): [K][NL]
    const LanTab lt = lan_tab(la, blockIdx.y, K);
    uint32_t *lout = la.lscal + la.ltab[(size_t)blockIdx.y * LAN_HDR_WORDS + 2];
    const uint32_t ltotal = K * lt.NL;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < ltotal; i += gridDim.x * 256u) {
      const uint32_t k = i / lt.NL, j = i - k * lt.NL;
      lout[i] = tb.nbr[k] != LFA_NONE ? a.dist[(size_t)tb.row[k] * a.n + lt.lv[j]] : LFA_NONE;
    }
  }
}

__global__ __launch_bounds__(256) void k_lfa_gather(LfaArgs a) { lfa_gather_body<false>(a, LanArgs{}); }
__global__ __launch_bounds__(256) void k_lfa_gather_lan(LfaArgs a, LanArgs la) { lfa_gather_body<true>(a, la); }


// The mode's kernel arguments, and its lane state (FrrProt, spf_frr_common.hip.h).  applies: the mode has a say at this destination
// (some primary crosses a LAN of S / has members).
template <FrrProt P> struct LfaProt {};
template <> struct LfaProt<FrrProt::Lan> { LanArgs la; };
template <FrrProt P> struct LfaLane {};
template <> struct LfaLane<FrrProt::Lan> {
  LanTab lt;
  uint32_t li0 = LFA_NONE, dL0D = LFA_NONE;                                        // the one primary's LAN and d(L, D)
  bool applies = false;
};

template <bool ONE, FrrProt P>
__device__ __forceinline__ void lfa_body(const LfaArgs &a, const LfaProt<P> &pa) {
  constexpr bool LAN = P == FrrProt::Lan, SRLG = P == FrrProt::Srlg;
  constexpr uint32_t NC = P == FrrProt::Plain ? 5 : 7;                             // the five alt_flags bits, then the mode's two counts
  __shared__ uint32_t s_cov[NC];
  __shared__ uint32_t s_tab[ONE ? (FRR_COLS + 1) * 64 : 1];             // the columns, then d(N_k, S)
  __shared__ uint32_t s_m[ONE ? 64 * 64 : 1];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const uint32_t S = tb.S, K = tb.K, n = a.n, W = a.W, Wk = tb.Wk;
  if (tid < NC) s_cov[tid] = 0;
  if constexpr (ONE) {                                                             // the same view over a copy in LDS
    for (uint32_t i = tid; i < FRR_COLS * K; i += 256u) s_tab[i] = tb.cols[i];
    for (uint32_t i = tid; i < K; i += 256u) s_tab[FRR_COLS * K + i] = tb.dns[i];
    for (uint32_t i = tid; i < K * K; i += 256u) s_m[i] = tb.m[i];
    tb = frr_tab_over(S, tb.srow, K, tb.C, s_tab, s_tab + FRR_COLS * K, s_m);
  }
  __syncthreads();
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  const size_t od = (size_t)pi * n + D;
  const uint32_t dSD = a.dist[sd];
  const bool in = valid && D != S && (a.flags[sd] & 1u) && dSD != LFA_NONE;
  uint32_t fl = 0, aslot = LFA_NONE, amet = 0;
  uint64_t cw = 0, nw = 0;                                                         // ONE: the two sets
  LfaLane<P> ml;
  if constexpr (LAN) ml.lt = lan_tab(pa.la, pi, K);
  if constexpr (SRLG) ml.open(pa, pi, K);
  if (in) {
    const uint64_t *pm = a.mask + sd * W;
    uint32_t np, p0;
    frr_primaries(tb, pm, np, p0);
    fl = (np ? 0x01u : 0u) | (np >= 2 ? 0x02u : 0u);
    uint32_t rl0 = LFA_NONE, E0 = LFA_NONE, dE0D = LFA_NONE;
    if (np == 1) {
      rl0 = tb.rl[p0]; E0 = tb.nbr[p0];
      if (E0 != LFA_NONE) dE0D = a.dist[(size_t)tb.row[p0] * n + D];
      if constexpr (LAN) {
        ml.li0 = ml.lt.li[p0];
        ml.applies = ml.li0 != LFA_NONE;
        if (ml.applies) ml.dL0D = a.dist[(size_t)ml.lt.lrow[p0] * n + D];
      }
      if constexpr (SRLG) ml.one_primary(p0);
    } else if (np >= 2) {
      if constexpr (LAN) ml.applies = lan_any_primary(tb, ml.lt, pm);
      if constexpr (SRLG) ml.any_primary(tb, pm);
    }
    if constexpr (LAN) { if (ml.applies) fl |= 0x20u; }
    bool have = false, bnode = false, bdown = false;
    uint64_t bsum = 0;
    uint32_t ci = 0;
    for (uint32_t w = 0; w < Wk; ++w) {
      if constexpr (!ONE) { cw = 0; nw = 0; }
      for (; ci < tb.C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if ((k >> 6) != w) break;
        const uint32_t dND = a.dist[(size_t)tb.row[k] * n + D];
        if (!lfa_less(dND, tb.dns[k], dSD)) continue;                               // loop-free
        if ((tb.cf[k] & 1u) && !a.ignore_overload && tb.nbr[k] != D) continue;       // an overloaded neighbour carries no transit traffic
        bool ok = true, nd = false;
        const uint32_t rlk = tb.rl[k];
        if (np == 1) {
          ok = rlk != rl0;
          if constexpr (LAN) {                                                     // every plain condition holds: now the pseudonode
            if (ok && ml.applies && !lfa_less(dND, ml.lt.ml[k * ml.lt.NL + ml.li0], ml.dL0D)) { ok = false; fl |= 0x40u; }
          }
          if constexpr (SRLG) {                                                    // ... now the group
            if (ok && ml.applies && !ml.safe_one(a, k, rlk, p0, dND, D)) { ok = false; fl |= 0x80u; }
          }
          nd = ok && E0 != LFA_NONE && lfa_less(dND, tb.m[k * K + p0], dE0D);
        } else if (np >= 2) {
          uint32_t n_router = 0;
          bool all = true, lanok = true;
          for (uint32_t w2 = 0; w2 < Wk && ok; ++w2) {
            uint64_t x = frr_word(tb, pm, w2);
            while (x) {
              const uint32_t p = w2 * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
              x &= x - 1;
              if (tb.rl[p] == rlk) { ok = false; break; }
              if (tb.nbr[p] != LFA_NONE) {
                ++n_router;
                all = all && lfa_less(dND, tb.m[k * K + p], a.dist[(size_t)tb.row[p] * n + D]);
              }
              if constexpr (LAN) {
                if (ml.applies && lanok) {
                  const uint32_t j = ml.lt.li[p];
                  if (j != LFA_NONE) lanok = lfa_less(dND, ml.lt.ml[k * ml.lt.NL + j], a.dist[(size_t)ml.lt.lrow[p] * n + D]);
                }
              }
            }
          }
          if constexpr (LAN) {
            if (ok && !lanok) { ok = false; fl |= 0x40u; }
          }
          if constexpr (SRLG) {
            if (ok && ml.applies && !ml.safe_ecmp(a, tb, pm, k, rlk, dND, D)) { ok = false; fl |= 0x80u; }
          }
          nd = ok && n_router && all;
        }
        if (!ok) continue;
        cw |= 1ull << (k & 63u);
        if (nd) nw |= 1ull << (k & 63u);
        if (np == 1) {
          const uint64_t sum = (uint64_t)tb.cost[k] + dND;
          if (!have || (nd && !bnode) || (nd == bnode && sum < bsum)) {            // candidates come in ascending slot order
            have = true; bnode = nd; bsum = sum; aslot = k; bdown = dND < dSD;
          }
        }
      }
      if constexpr (!ONE) {
        if (a.cand_mask) a.cand_mask[od * W + w] = cw;
        if (a.node_mask) a.node_mask[od * W + w] = nw;
      }
    }
    if (have) {
      fl |= 0x04u | (bnode ? 0x08u : 0u) | (bdown ? 0x10u : 0u);
      amet = bsum > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)bsum;
    }
  }
  if (valid) {
    a.alt_slot[od] = aslot; a.alt_metric[od] = amet; a.alt_flags[od] = (uint8_t)fl;
    // the words of the sets that the loop above did not write
    const uint32_t w0 = ONE ? 0u : (in ? Wk : 0u);
    for (uint32_t w = w0; w < W; ++w) {
      if (a.cand_mask) a.cand_mask[od * W + w] = (ONE && w == 0) ? cw : 0ull;
      if (a.node_mask) a.node_mask[od * W + w] = (ONE && w == 0) ? nw : 0ull;
    }
  }
  // coverage: the counted bits of alt_flags as they lie (Lan's two are bits 5 and 6); Srlg: "a primary has members", which is no
  // bit of alt_flags, and HSPF_LFA_SRLG_REFUSED (bit 7) behind the five
  uint32_t cv = fl;
  if constexpr (SRLG) cv = (fl & 0x1Fu) | (ml.applies ? 0x20u : 0u) | ((fl & 0x80u) ? 0x40u : 0u);
  frr_cover<NC>(cv, s_cov, a.coverage + (size_t)pi * NC);
}

template <bool ONE>
__global__ __launch_bounds__(256) void k_lfa(LfaArgs a) { lfa_body<ONE>(a, LfaProt<FrrProt::Plain>{}); }
template <bool ONE>
__global__ __launch_bounds__(256) void k_lfa_lan(LfaArgs a, LfaProt<FrrProt::Lan> pa) { lfa_body<ONE>(a, pa); }

}  // namespace
