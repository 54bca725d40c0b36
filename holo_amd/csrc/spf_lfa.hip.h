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
// Coverage: wave ballots + popcounts, one LDS add per wave and one vector atomic add per workgroup and counter.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t LFA_HDR_WORDS = 8;      // per protected root: S, its row, K, C, offset of the slot arrays, offset of the scalars, 0, 0
constexpr uint32_t LFA_NONE = 0xFFFFFFFFu;
constexpr uint32_t LFA_TILE = 256;

struct LfaArgs {
  uint32_t n, W, ignore_overload, pad;
  const uint32_t *dist; const uint16_t *flags; const uint64_t *mask;     // the table set
  const uint32_t *tab;                 // [n_prot][LFA_HDR_WORDS] headers, then per root: nbr | row | cost | root_link | cflags | candidate list, K words each
  uint32_t *scal;                      // per root at its offset: d(N_k, S) [K] | d(N_k, N_p) [K][K]
  uint32_t *alt_slot, *alt_metric; uint8_t *alt_flags; uint64_t *cand_mask, *node_mask; uint32_t *coverage;
};

__global__ __launch_bounds__(256) void k_lfa_gather(LfaArgs a) {
  const uint32_t *hdr = a.tab + (size_t)blockIdx.y * LFA_HDR_WORDS;
  const uint32_t S = hdr[0], K = hdr[2];
  const uint32_t *nbr = a.tab + hdr[4], *row = nbr + K;
  uint32_t *out = a.scal + hdr[5];
  const uint32_t total = K + K * K;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    uint32_t v = LFA_NONE;
    if (i < K) {
      if (nbr[i] != LFA_NONE) v = a.dist[(size_t)row[i] * a.n + S];
    } else {
      const uint32_t k = (i - K) / K, p = (i - K) - k * K;
      if (nbr[k] != LFA_NONE && nbr[p] != LFA_NONE) v = a.dist[(size_t)row[k] * a.n + nbr[p]];
    }
    out[i] = v;
  }
}

// `a < b + c` in 64 bits; any term "not reached" makes it false
__device__ __forceinline__ bool lfa_less(uint32_t a, uint32_t b, uint32_t c) {
  return a != LFA_NONE && b != LFA_NONE && c != LFA_NONE && (uint64_t)a < (uint64_t)b + (uint64_t)c;
}

template <bool ONE>
__global__ __launch_bounds__(256) void k_lfa(LfaArgs a) {
  __shared__ uint32_t s_cov[5];
  __shared__ uint32_t s_tab[ONE ? 7 * 64 : 1];
  __shared__ uint32_t s_m[ONE ? 64 * 64 : 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.y;
  const uint32_t *hdr = a.tab + (size_t)pi * LFA_HDR_WORDS;
  const uint32_t S = hdr[0], srow = hdr[1], K = hdr[2], C = hdr[3];
  const uint32_t n = a.n, W = a.W, Wk = (K + 63u) >> 6;
  const uint32_t *nbr, *row, *cost, *rl, *cf, *cl, *dns, *m;
  if (tid < 5) s_cov[tid] = 0;
  if constexpr (ONE) {
    const uint32_t *g = a.tab + hdr[4], *gs = a.scal + hdr[5];
    for (uint32_t i = tid; i < 6 * K; i += 256u) s_tab[i] = g[i];
    for (uint32_t i = tid; i < K; i += 256u) s_tab[6 * K + i] = gs[i];
    for (uint32_t i = tid; i < K * K; i += 256u) s_m[i] = gs[K + i];
    nbr = s_tab; row = s_tab + K; cost = s_tab + 2 * K; rl = s_tab + 3 * K; cf = s_tab + 4 * K; cl = s_tab + 5 * K; dns = s_tab + 6 * K; m = s_m;
  } else {
    nbr = a.tab + hdr[4]; row = nbr + K; cost = nbr + 2 * K; rl = nbr + 3 * K; cf = nbr + 4 * K; cl = nbr + 5 * K;
    dns = a.scal + hdr[5]; m = dns + K;
  }
  __syncthreads();
  const uint64_t last_word = (K & 63u) ? ((1ull << (K & 63u)) - 1ull) : ~0ull;     // slots of the last word that exist
  uint32_t my_cov = 0;                                                             // lane j < 5 of a wave: its count of flag bit j
  {
    const uint32_t D = blockIdx.x * LFA_TILE + tid;
    const bool valid = D < n;
    const size_t sd = (size_t)srow * n + (valid ? D : 0u);
    const size_t od = (size_t)pi * n + D;
    const uint32_t dSD = a.dist[sd];
    const bool in = valid && D != S && (a.flags[sd] & 1u) && dSD != LFA_NONE;
    uint32_t fl = 0, aslot = LFA_NONE, amet = 0;
    uint64_t cw = 0, nw = 0;                                                       // ONE: the two sets
    if (in) {
      const uint64_t *pm = a.mask + sd * W;
      // the primaries: how many, and the first one
      uint32_t np = 0, p0 = 0;
      for (uint32_t w = 0; w < Wk; ++w) {
        const uint64_t x = pm[w] & (w + 1 == Wk ? last_word : ~0ull);
        if (x && !np) p0 = w * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
        np += (uint32_t)__popcll(x);
      }
      fl = (np ? 0x01u : 0u) | (np >= 2 ? 0x02u : 0u);
      uint32_t rl0 = LFA_NONE, E0 = LFA_NONE, dE0D = LFA_NONE;
      if (np == 1) {
        rl0 = rl[p0]; E0 = nbr[p0];
        if (E0 != LFA_NONE) dE0D = a.dist[(size_t)row[p0] * n + D];
      }
      bool have = false, bnode = false, bdown = false;
      uint64_t bsum = 0;
      uint32_t ci = 0;
      for (uint32_t w = 0; w < Wk; ++w) {
        if constexpr (!ONE) { cw = 0; nw = 0; }
        for (; ci < C; ++ci) {
          const uint32_t k = cl[ci];
          if ((k >> 6) != w) break;
          const uint32_t dND = a.dist[(size_t)row[k] * n + D];
          if (!lfa_less(dND, dns[k], dSD)) continue;                               // loop-free
          if ((cf[k] & 1u) && !a.ignore_overload && nbr[k] != D) continue;         // an overloaded neighbour carries no transit traffic
          bool ok = true, nd = false;
          if (np == 1) {
            ok = rl[k] != rl0;
            nd = ok && E0 != LFA_NONE && lfa_less(dND, m[k * K + p0], dE0D);
          } else if (np >= 2) {
            uint32_t n_router = 0;
            bool all = true;
            const uint32_t rlk = rl[k];
            for (uint32_t w2 = 0; w2 < Wk && ok; ++w2) {
              uint64_t x = pm[w2] & (w2 + 1 == Wk ? last_word : ~0ull);
              while (x) {
                const uint32_t p = w2 * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
                x &= x - 1;
                if (rl[p] == rlk) { ok = false; break; }
                if (nbr[p] != LFA_NONE) {
                  ++n_router;
                  all = all && lfa_less(dND, m[k * K + p], a.dist[(size_t)row[p] * n + D]);
                }
              }
            }
            nd = ok && n_router && all;
          }
          if (!ok) continue;
          cw |= 1ull << (k & 63u);
          if (nd) nw |= 1ull << (k & 63u);
          if (np == 1) {
            const uint64_t sum = (uint64_t)cost[k] + dND;
            if (!have || (nd && !bnode) || (nd == bnode && sum < bsum)) {          // candidates come in ascending slot order
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
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) {
      const uint32_t c = (uint32_t)__popcll(__ballot((fl >> j) & 1u));
      if (lane == j) my_cov += c;
    }
  }
  if (lane < 5 && my_cov) atomicAdd(&s_cov[lane], my_cov);
  __syncthreads();
  if (tid < 5 && s_cov[tid]) atomicAdd(a.coverage + (size_t)pi * 5 + tid, s_cov[tid]);
}

}  // namespace
