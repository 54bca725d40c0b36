// spf_tilfa.hip.h — two-segment repair paths (TI-LFA, link protection): per (protected root S, protected slot e) the cheapest
// repair that is either one node of extended-P ∩ Q or a node p of extended P plus one forced adjacency p -> q into Q, from the
// space tables hspf_rlfa_device wrote, the forward and reverse-distance rows, and the raw CSR of the forward graph
// (hspf_tilfa_device; the semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  As k_rlfa: lane = vertex p, 256 consecutive p per workgroup; the candidate slots of a root are the grid's y axis, the
// protected roots its z axis.
//   k_tilfa        per slot the lane loads space_flags[e][p], space_via[e][p] (coalesced) and the one distance its release metric
//                  needs (d(S, p) or d(N_via, p): consecutive p of one row per via), then walks p's own row of the raw CSR: per
//                  link the staged two-way byte, a 1-byte gather of space_flags[e][q] and a 4-byte gather of rdist[row of E][q].
//                  Selection: ONE 64-bit key per (S, e), (saturated total << 32 | kind bit << 31 | p) — the kind bit (0 = single
//                  node, 1 = pair) sits above p, so that at equal totals a single node wins before p is compared; q and the link
//                  position are not in the key: k_tilfa_final finds them again in the winner's row.  Wave minimum, one LDS min
//                  per wave, one vector 64-bit atomicMin per workgroup and slot into the key array the call sets to all-ones.
//                  Counts: a ballot + popcount for the single nodes, a wave sum for the pairs, one LDS add per wave and one
//                  vector atomic add per workgroup, slot and counter.
//   k_tilfa_final  one thread per (S, slot): key -> ti_kind / ti_p / ti_metric, ti_via from the table, and for a pair the
//                  winner's row once more for the smallest (total, q, position).
//   k_tilfa_dest   lane = destination over S's mask row (as k_rlfa_dest): the class of its one primary slot, five counts.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_rlfa.hip.h"

namespace {

constexpr uint64_t TILFA_SAT = 0xFFFFFFFEull;
constexpr unsigned long long TILFA_PAIR_BIT = 0x80000000ull;

struct TilfaArgs {
  uint32_t n, W, stride, pad;                                              // stride = 64 * W slots per protected root
  const uint32_t *dist, *rdist; const uint16_t *flags; const uint64_t *mask;   // the two table sets
  const uint32_t *tab;                                                     // as LfaArgs (staged by the call)
  const uint8_t *alt_in;                                                   // [n_prot][n] alt_flags of hspf_lfa_device, or NULL
  const uint8_t *sflags; const uint32_t *svia;                             // [n_prot][stride][n] of hspf_rlfa_device
  const uint32_t *row_ptr, *col, *metric; const uint8_t *tw;               // the forward graph's raw CSR; two-way byte per link (staged)
  unsigned long long *key;                                                 // [n_prot][stride] scratch, all-ones
  uint8_t *ti_kind; uint32_t *ti_p, *ti_q, *ti_via, *ti_link, *ti_metric, *ti_counts;
  uint8_t *td_kind; uint32_t *td_cov;
};

// the release metric of v under slot e from its via (64 bits); false: v has no release point (or the table holds no slot of S)
__device__ __forceinline__ bool tilfa_rel(const TilfaArgs &a, const FrrTab &tb, uint32_t via, uint32_t v, uint64_t &rel) {
  if (via == RLFA_VIA_SELF) { rel = a.dist[(size_t)tb.srow * a.n + v]; return true; }
  if (via >= tb.K) return false;
  rel = (uint64_t)tb.cost[via] + a.dist[(size_t)tb.row[via] * a.n + v];
  return true;
}

__global__ __launch_bounds__(256) void k_tilfa(TilfaArgs a) {
  __shared__ uint32_t s_cnt[2];
  __shared__ unsigned long long s_key;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.z;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n;
  const uint32_t p = blockIdx.x * LFA_TILE + tid;
  const bool valid = p < n;
  const uint32_t pp = valid ? p : 0u;
  const uint32_t rb = valid ? a.row_ptr[pp] : 0u, re = valid ? a.row_ptr[pp + 1] : 0u;
  const size_t slot0 = (size_t)pi * a.stride;
  if (tid < 2) s_cnt[tid] = 0;
  if (tid == 0) s_key = RLFA_NO_KEY;
  __syncthreads();
  for (uint32_t ci = blockIdx.y; ci < tb.C; ci += gridDim.y) {
    const uint32_t e = tb.cl[ci];
    const size_t so = (slot0 + e) * n;
    const uint32_t *rdE = a.rdist + (size_t)tb.row[e] * n;
    const uint32_t sf = valid ? a.sflags[so + pp] : 0u;
    uint64_t rel = 0;
    const bool in_xp = (sf & 0x08u) && (sf & 0x03u) && tilfa_rel(a, tb, a.svia[so + pp], pp, rel);   // eligible, in P or some XP
    const bool single = in_xp && (sf & 0x04u);
    unsigned long long key = RLFA_NO_KEY;
    if (single) {
      const uint64_t t = rel + rdE[pp];
      key = ((t > TILFA_SAT ? TILFA_SAT : t) << 32) | pp;
    }
    uint32_t n_pair = 0;
    if (in_xp) {
      uint64_t best = ~0ull;
      for (uint32_t k = rb; k < re; ++k) {
        const uint32_t q = a.col[k];
        if (q == pp || q >= n || !a.tw[k]) continue;
        if ((a.sflags[so + q] & 0x0Cu) != 0x0Cu) continue;                       // eligible and in Q
        const uint64_t t = rel + a.metric[k] + rdE[q];
        ++n_pair;
        best = t < best ? t : best;
      }
      if (n_pair) {
        const unsigned long long kp = ((best > TILFA_SAT ? TILFA_SAT : best) << 32) | TILFA_PAIR_BIT | pp;
        key = kp < key ? kp : key;
      }
    }
    const uint32_t c_single = (uint32_t)__popcll(__ballot(single));
    uint32_t c_pair = n_pair;
#pragma unroll
    for (int o = 32; o; o >>= 1) c_pair += __shfl_xor(c_pair, o);
    if (c_single || c_pair) {                                                    // (wave-uniform)
      key = rlfa_wave_min(key);
      if (lane == 0) {
        if (c_single) atomicAdd(&s_cnt[0], c_single);
        if (c_pair) atomicAdd(&s_cnt[1], c_pair);
        atomicMin(&s_key, key);
      }
    }
    __syncthreads();
    // one vector atomic per workgroup, slot and counter; the owner of an LDS cell resets it for the next slot
    if (tid < 2) {
      const uint32_t cnt = s_cnt[tid];
      if (cnt) { atomicAdd(a.ti_counts + (slot0 + e) * 2 + tid, cnt); s_cnt[tid] = 0; }
    }
    if (tid == 2) {
      const unsigned long long k2 = s_key;
      if (k2 != RLFA_NO_KEY) { atomicMin(a.key + slot0 + e, k2); s_key = RLFA_NO_KEY; }
    }
    __syncthreads();
  }
}

// one thread per (protected root, slot): key -> kind / p / metric; the via from the table; a pair's q and link from p's row
__global__ __launch_bounds__(256) void k_tilfa_final(TilfaArgs a, uint32_t n_prot) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_prot * a.stride) return;
  const uint32_t pi = i / a.stride, e = i - pi * a.stride;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n;
  uint32_t kind = 0, p = LFA_NONE, q = LFA_NONE, via = LFA_NONE, link = LFA_NONE, met = 0;
  const unsigned long long key = a.key[i];
  if (e < tb.K && tb.nbr[e] != LFA_NONE && key != RLFA_NO_KEY) {
    const size_t so = (size_t)i * n;
    met = (uint32_t)(key >> 32); p = (uint32_t)key & 0x7FFFFFFFu; kind = (key & TILFA_PAIR_BIT) ? 2u : 1u;
    via = a.svia[so + p];
    q = p;
    uint64_t rel = 0;
    if (kind == 2u && tilfa_rel(a, tb, via, p, rel)) {
      const uint32_t *rdE = a.rdist + (size_t)tb.row[e] * n;
      const uint32_t rb = a.row_ptr[p], re = a.row_ptr[p + 1];
      uint64_t bt = ~0ull;
      for (uint32_t k = rb; k < re; ++k) {
        const uint32_t t = a.col[k];
        if (t == p || t >= n || !a.tw[k] || (a.sflags[so + t] & 0x0Cu) != 0x0Cu) continue;
        uint64_t tot = rel + a.metric[k] + rdE[t];
        tot = tot > TILFA_SAT ? TILFA_SAT : tot;
        if (tot < bt || (tot == bt && t < q)) { bt = tot; q = t; link = k - rb; }      // ascending position: a tie keeps the earlier link
      }
    }
  }
  a.ti_kind[i] = (uint8_t)kind; a.ti_p[i] = p; a.ti_q[i] = q; a.ti_via[i] = via; a.ti_link[i] = link; a.ti_metric[i] = met;
}

// per destination D of S with exactly one primary slot: covered by LFA | by a single node | by a pair | uncovered; the five counts
__global__ __launch_bounds__(256) void k_tilfa_dest(TilfaArgs a) {
  __shared__ uint32_t s_cov[5];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n;
  if (tid < 5) s_cov[tid] = 0;
  __syncthreads();
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  const size_t od = (size_t)pi * n + D;
  const bool in = valid && D != tb.S && (a.flags[sd] & 1u) && a.dist[sd] != LFA_NONE;
  uint32_t cls = 0;
  if (in) {
    uint32_t np, p0;
    frr_primaries(tb, a.mask + sd * a.W, np, p0);
    if (np == 1) {
      if (a.alt_in && (a.alt_in[od] & 0x04u)) cls = 1u;                            // HSPF_LFA_LINK_PROTECT: LFA covers it
      else {
        const uint32_t kd = a.ti_kind[(size_t)pi * a.stride + p0];
        cls = kd ? kd + 1u : 4u;
      }
    }
  }
  if (valid) a.td_kind[od] = (uint8_t)cls;
  frr_cover<5>(cls ? 1u | (1u << cls) : 0u, s_cov, a.td_cov + (size_t)pi * 5);      // counter 0: any class; counter j: class j (1 .. 4)
}

}  // namespace
