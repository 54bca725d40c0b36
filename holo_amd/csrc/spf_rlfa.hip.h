// spf_rlfa.hip.h — remote loop-free alternates (RFC 7490): the PQ node of every (protected root S, protected slot e) from the
// forward SPT rows of S and its neighbour routers and the rows of the same roots on the transposed graph (hspf_rlfa_device; the
// semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  As k_lfa: lane = vertex, 256 consecutive v per workgroup, every row load coalesced; the per-root scalars d(N_k, S) come
// from k_lfa_gather's scratch block.  The second dimension — the protected slots — is walked in chunks of RLFA_CH candidates:
//   k_rlfa        per chunk the lane keeps c + d(E_e, v), the P / XP / Q bits and the running release point of its RLFA_CH slots
//                 in registers; the candidates k are streamed ONCE per chunk — d(N_k, v) is loaded, judged against every slot of
//                 the chunk and forgotten.  Nothing that scales with K lives in registers.  The counts are wave ballots +
//                 popcounts, one LDS add per wave and one vector atomic add per workgroup, slot and counter; the selection is a
//                 wave minimum of the 64-bit key (release metric << 32 | v), one LDS min per wave and one vector 64-bit atomicMin
//                 per workgroup and slot into a key array the call initialises to all-ones.
//   k_rlfa_final  one thread per (S, slot): the key becomes pq_node / pq_metric, and the via is recomputed for that one vertex —
//                 so the per-vertex via table (space_via) can stay optional.
//   k_rlfa_dest   lane = destination over S's mask row: the PQ node of the one primary slot, and the four coverage counts.
// The LAN variants (hspf_rlfa_lan_device: P, extended P and Q additionally loop-free towards the pseudonode L of the slot's LAN) are
// the `true` instantiations of the same three bodies; the kernels above are the `false` ones.  Per chunk the lane additionally keeps
// d(L_j, v) of its slots — loaded once per DISTINCT LAN of the chunk (the compact index li is wave-uniform: a later slot of the same
// LAN copies the register), with rdist[lr][v] next to it for the Q side; d(S, L_j) and d(L_j, E_j) are wave-uniform reads next to
// cost[e].  The via-slot stream reads d(N_k, L) as scalars from k_lfa_gather_lan's [K][NL] block and adds no per-lane load.  The
// plain sets are kept as three more bit masks, for the fifth count word only: selection, tables and release point see the
// LAN-safe sets.  A slot without a LAN evaluates no LAN term.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_frr_common.hip.h"

namespace {

constexpr uint32_t RLFA_CH = 8;                    // protected slots per chunk
constexpr uint32_t RLFA_VIA_SELF = 0xFFFFFFFEu;    // HSPF_RLFA_VIA_SELF
constexpr uint64_t RLFA_NO_KEY = ~0ull;
constexpr uint32_t RLFA_CW = 4, RLFA_LAN_CW = 5;   // count words per slot: HSPF_RLFA_COUNT_WORDS, HSPF_RLFA_LAN_COUNT_WORDS (held to them in spf_frr.hip.h)

struct RlfaArgs {
  uint32_t n, W, ignore_overload, stride;                                  // stride = 64 * W slots per protected root
  const uint32_t *dist, *rdist; const uint16_t *flags; const uint64_t *mask;   // the two table sets
  const uint8_t *vf;                                                       // the graph's resident vertex flags
  const uint32_t *tab, *scal;                                              // as LfaArgs (staged by the call, gathered by k_lfa_gather)
  const uint8_t *alt_in;                                                   // [n_prot][n] alt_flags of hspf_lfa_device, or NULL
  unsigned long long *key;                                                 // [n_prot][stride] scratch, all-ones
  uint32_t *pq_node, *pq_via, *pq_metric, *pq_counts;
  uint8_t *space_flags; uint32_t *space_via;
  uint32_t *rl_node, *rl_via, *rl_cov;
};

__device__ __forceinline__ unsigned long long rlfa_wave_min(unsigned long long x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned long long y = __shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}

// The LAN block as a kernel argument of an instantiation: nothing for LAN = false.  (The three kernels are instantiated as kernels,
// not inlined into wrappers: behind a wrapper the register allocation of the `false` instantiation moves — k_rlfa to 83 VGPRs and
// 54 SGPR spills against 91 and 18 — with not one line of the body changed.)
template <bool LAN> struct RlfaLan {};
template <> struct RlfaLan<true> { LanArgs la; };

// The LAN instantiation asks for five waves per SIMD, the occupancy the plain one reaches unasked: left alone the compiler settles
// on 101 VGPRs and four waves for it; asked, on 93.  The hint of the plain one (1) is no constraint: its code is the parent's.
template <bool LAN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LAN ? 5 : 1))) void k_rlfa_t(RlfaArgs a, RlfaLan<LAN> l) {
  constexpr uint32_t CW = LAN ? RLFA_LAN_CW : RLFA_CW;
  __shared__ uint32_t s_cnt[RLFA_CH * CW];
  __shared__ unsigned long long s_key[RLFA_CH];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const uint32_t S = tb.S, C = tb.C, n = a.n;
  const uint32_t v = blockIdx.x * LFA_TILE + tid;
  const bool valid = v < n;
  const uint32_t vv = valid ? v : 0u;
  const size_t sv = (size_t)tb.srow * n + vv;
  const uint32_t dSv = a.dist[sv], rSv = a.rdist[sv];
  const uint32_t f = a.vf[vv];
  const bool elig = valid && v != S && (a.flags[sv] & 1u) && dSv != LFA_NONE && !(f & 0x05u) &&      // a router, not NO_EXPAND
                    (!(f & 0x02u) || a.ignore_overload);
  const size_t slot0 = (size_t)pi * a.stride;
  LanTab lt{};
  if constexpr (LAN) lt = lan_tab(l.la, pi, tb.K);
  if (tid < RLFA_CH * CW) s_cnt[tid] = 0;
  if (tid < RLFA_CH) s_key[tid] = RLFA_NO_KEY;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < C; c0 += RLFA_CH) {
    // the chunk: its slots' c + d(E, v), the P and Q bits, the release point so far
    uint64_t t[RLFA_CH], best[RLFA_CH];
    uint32_t via[RLFA_CH], rle[RLFA_CH], es[RLFA_CH];
    uint32_t tm = 0, pm = 0, qm = 0, xm = 0;                                       // bit j: t[j] is finite | P | Q | some XP
    uint32_t lij[LAN ? RLFA_CH : 1], dLv[LAN ? RLFA_CH : 1], rLv[LAN ? RLFA_CH : 1];      // LAN: the slot's LAN index; d(L_j, v); d(v, L_j)
    uint32_t pp = 0, qp = 0, xp = 0;                                               // LAN: the plain P | Q | some XP (pm / qm / xm: LAN-safe)
#pragma unroll
    for (uint32_t j = 0; j < RLFA_CH; ++j) {
      const bool live = c0 + j < C;
      const uint32_t e = tb.cl[live ? c0 + j : c0];
      es[j] = e; rle[j] = tb.rl[e];
      const size_t ev = (size_t)tb.row[e] * n + vv;
      const uint32_t c = tb.cost[e], dEv = a.dist[ev], rEv = a.rdist[ev];
      t[j] = (uint64_t)c + dEv;
      const bool tok = live && elig && dEv != LFA_NONE;
      bool p = tok && (uint64_t)dSv < t[j];
      bool q = live && elig && lfa_less(rEv, rSv, c);
      if constexpr (LAN) {
        pp |= (p ? 1u : 0u) << j; qp |= (q ? 1u : 0u) << j;
        const uint32_t l = live ? lt.li[e] : LFA_NONE;                               // wave-uniform
        lij[j] = l; dLv[j] = LFA_NONE; rLv[j] = LFA_NONE;
        if (l != LFA_NONE) {
          bool first = true;                                                       // the rows of a LAN are loaded by its first slot of the chunk
#pragma unroll
          for (uint32_t jj = 0; jj < j; ++jj)
            if (first && lij[jj] == l) { dLv[j] = dLv[jj]; rLv[j] = rLv[jj]; first = false; }
          const size_t lrow = (size_t)lt.lrow[e] * n;
          if (first) { dLv[j] = a.dist[lrow + vv]; rLv[j] = a.rdist[lrow + vv]; }
          const uint32_t dSL = a.dist[(size_t)tb.srow * n + lt.lv[l]], dLE = a.dist[lrow + tb.nbr[e]];      // wave-uniform
          p = p && lfa_less(dSv, dSL, dLv[j]);
          q = q && lfa_less(rEv, rLv[j], dLE);
        }
      }
      tm |= (tok ? 1u : 0u) << j; pm |= (p ? 1u : 0u) << j; qm |= (q ? 1u : 0u) << j;
      best[j] = p ? (uint64_t)dSv : ~0ull;
      via[j] = p ? RLFA_VIA_SELF : LFA_NONE;
    }
    // the via-slots, once per chunk (ascending k: a tie keeps S, then the smaller slot)
    if (__ballot(tm != 0)) {
      for (uint32_t ci = 0; ci < C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if ((tb.cf[k] & 1u) && !a.ignore_overload) continue;                       // an overloaded neighbour carries no transit traffic
        const uint32_t dNS = tb.dns[k];
        if (dNS == LFA_NONE) continue;
        const uint32_t dNv = a.dist[(size_t)tb.row[k] * n + vv], rlk = tb.rl[k];
        const uint64_t rel = (uint64_t)tb.cost[k] + dNv;
        const uint32_t okm = dNv != LFA_NONE ? tm : 0u;
#pragma unroll
        for (uint32_t j = 0; j < RLFA_CH; ++j) {
          if (((okm >> j) & 1u) && rlk != rle[j] && (uint64_t)dNv < (uint64_t)dNS + t[j]) {
            if constexpr (LAN) {
              xp |= 1u << j;
              if (lij[j] != LFA_NONE && !lfa_less(dNv, lt.ml[k * lt.NL + lij[j]], dLv[j])) continue;      // d(N_k, L): a scalar
            }
            xm |= 1u << j;
            if (rel < best[j]) { best[j] = rel; via[j] = k; }
          }
        }
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < RLFA_CH; ++j) {
      if (c0 + j >= C) break;
      const bool p = (pm >> j) & 1u, x = (xm >> j) & 1u, q = (qm >> j) & 1u;
      const bool ext = p || x, pq = ext && q;
      const uint32_t c_p = (uint32_t)__popcll(__ballot(p)), c_x = (uint32_t)__popcll(__ballot(ext)), c_q = (uint32_t)__popcll(__ballot(q));
      const unsigned long long b_pq = __ballot(pq);
      if (lane == 0) {
        if (c_p) atomicAdd(&s_cnt[j * CW + 0], c_p);
        if (c_x) atomicAdd(&s_cnt[j * CW + 1], c_x);
        if (c_q) atomicAdd(&s_cnt[j * CW + 2], c_q);
        if (b_pq) atomicAdd(&s_cnt[j * CW + 3], (uint32_t)__popcll(b_pq));
      }
      if constexpr (LAN) {                                                         // in the plain (P or XP) and Q, not in the LAN-safe one
        const bool lost = ((((pp | xp) & qp) >> j) & 1u) && !pq;
        const unsigned long long b_lost = __ballot(lost);
        if (lane == 0 && b_lost) atomicAdd(&s_cnt[j * CW + 4], (uint32_t)__popcll(b_lost));
      }
      if (b_pq) {
        const uint64_t sat = best[j] > 0xFFFFFFFEull ? 0xFFFFFFFEull : best[j];
        const unsigned long long key = rlfa_wave_min(pq ? (unsigned long long)((sat << 32) | v) : RLFA_NO_KEY);
        if (lane == 0) atomicMin(&s_key[j], key);
      }
      if (valid) {
        const size_t o = (slot0 + es[j]) * n + v;
        if (a.space_flags) a.space_flags[o] = (uint8_t)((p ? 1u : 0u) | (x ? 2u : 0u) | (q ? 4u : 0u) | (elig ? 8u : 0u));
        if (a.space_via) a.space_via[o] = via[j];
      }
    }
    __syncthreads();
    // one vector atomic per workgroup, slot and counter; the owner of an LDS cell resets it for the next chunk
    if (tid < RLFA_CH * CW) {
      const uint32_t j = tid / CW, cnt = s_cnt[tid];
      if (cnt) { atomicAdd(a.pq_counts + (slot0 + tb.cl[c0 + j]) * CW + (tid - j * CW), cnt); s_cnt[tid] = 0; }      // cnt != 0: slot j of the chunk exists
    }
    if (tid < RLFA_CH) {
      const unsigned long long key = s_key[tid];
      if (key != RLFA_NO_KEY) { atomicMin(a.key + slot0 + tb.cl[c0 + tid], key); s_key[tid] = RLFA_NO_KEY; }
    }
    __syncthreads();
  }
  // the optional tables of the slots that are no candidates: "none"
  if (valid && (a.space_flags || a.space_via)) {
    for (uint32_t e = 0; e < a.stride; ++e) {
      if (e < tb.K && tb.nbr[e] != LFA_NONE) continue;
      const size_t o = (slot0 + e) * n + v;
      if (a.space_flags) a.space_flags[o] = 0;
      if (a.space_via) a.space_via[o] = LFA_NONE;
    }
  }
}

constexpr auto k_rlfa = k_rlfa_t<false>;
constexpr auto k_rlfa_lan = k_rlfa_t<true>;

// one thread per (protected root, slot): key -> pq_node / pq_metric, and the via of that one vertex again (LAN: under the same
// LAN conditions as the chunk loop)
template <bool LAN>
__global__ __launch_bounds__(256) void k_rlfa_final_t(RlfaArgs a, uint32_t n_prot, RlfaLan<LAN> l) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_prot * a.stride) return;
  const uint32_t pi = i / a.stride, e = i - pi * a.stride;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const uint32_t n = a.n;
  uint32_t node = LFA_NONE, via = LFA_NONE, met = 0;
  const unsigned long long key = a.key[i];
  if (e < tb.K && tb.nbr[e] != LFA_NONE && key != RLFA_NO_KEY) {
    node = (uint32_t)key; met = (uint32_t)(key >> 32);
    const uint32_t dSv = a.dist[(size_t)tb.srow * n + node], dEv = a.dist[(size_t)tb.row[e] * n + node];
    LanTab lt{};
    uint32_t li = LFA_NONE, dLv = LFA_NONE;                                           // LAN: the slot's LAN index and d(L, node)
    if constexpr (LAN) {
      lt = lan_tab(l.la, pi, tb.K);
      li = lt.li[e];
      if (li != LFA_NONE) dLv = a.dist[(size_t)lt.lrow[e] * n + node];
    }
    if (dEv != LFA_NONE) {                                                         // (a PQ node has a P or an XP: d(E, v) is finite)
      const uint64_t t = (uint64_t)tb.cost[e] + dEv;
      uint64_t best = ~0ull;
      bool lan_p = true;                                                           // LAN: S's own path to the node avoids L
      if constexpr (LAN) lan_p = li == LFA_NONE || lfa_less(dSv, a.dist[(size_t)tb.srow * n + lt.lv[li]], dLv);
      if (dSv != LFA_NONE && (uint64_t)dSv < t && lan_p) { best = dSv; via = RLFA_VIA_SELF; }
      for (uint32_t ci = 0; ci < tb.C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if ((tb.cf[k] & 1u) && !a.ignore_overload) continue;
        const uint32_t dNS = tb.dns[k], dNv = a.dist[(size_t)tb.row[k] * n + node];
        if (dNS == LFA_NONE || dNv == LFA_NONE || tb.rl[k] == tb.rl[e] || !((uint64_t)dNv < (uint64_t)dNS + t)) continue;
        if constexpr (LAN) {
          if (li != LFA_NONE && !lfa_less(dNv, lt.ml[k * lt.NL + li], dLv)) continue;
        }
        const uint64_t rel = (uint64_t)tb.cost[k] + dNv;
        if (rel < best) { best = rel; via = k; }
      }
    }
  }
  a.pq_node[i] = node; a.pq_via[i] = via; a.pq_metric[i] = met;
}

constexpr auto k_rlfa_final = k_rlfa_final_t<false>;
constexpr auto k_rlfa_final_lan = k_rlfa_final_t<true>;

// per destination D of S: the PQ node of its one primary slot, where LFA left it unprotected; the four coverage counts (LAN: and
// the one-primary destinations behind a LAN | of those, the uncovered ones whose slot had a plain PQ node)
template <bool LAN>
__global__ __launch_bounds__(256) void k_rlfa_dest_t(RlfaArgs a, RlfaLan<LAN> l) {
  constexpr uint32_t NC = LAN ? 6 : 4;
  __shared__ uint32_t s_cov[NC];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n;
  if (tid < NC) s_cov[tid] = 0;
  __syncthreads();
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  const size_t od = (size_t)pi * n + D;
  const bool in = valid && D != tb.S && (a.flags[sd] & 1u) && a.dist[sd] != LFA_NONE;
  uint32_t fl = 0, node = LFA_NONE, via = LFA_NONE;
  if (in) {
    uint32_t np, p0;
    frr_primaries(tb, a.mask + sd * a.W, np, p0);
    if (np == 1) {
      fl = 1u;
      if (a.alt_in && (a.alt_in[od] & 0x04u)) fl |= 2u;                            // HSPF_LFA_LINK_PROTECT: LFA covers it
      else {
        const size_t o = (size_t)pi * a.stride + p0;
        if (tb.nbr[p0] != LFA_NONE && a.pq_node[o] != LFA_NONE) { node = a.pq_node[o]; via = a.pq_via[o]; fl |= 4u; }
        else fl |= 8u;
      }
      if constexpr (LAN) {
        if (lan_tab(l.la, pi, tb.K).li[p0] != LFA_NONE) {
          fl |= 16u;
          const uint32_t *cnt = a.pq_counts + ((size_t)pi * a.stride + p0) * RLFA_LAN_CW;
          if ((fl & 8u) && cnt[3] + cnt[4] != 0) fl |= 32u;                        // the plain sets had a PQ node
        }
      }
    }
  }
  if (valid) { a.rl_node[od] = node; a.rl_via[od] = via; }
  frr_cover<NC>(fl, s_cov, a.rl_cov + (size_t)pi * NC);
}

constexpr auto k_rlfa_dest = k_rlfa_dest_t<false>;
constexpr auto k_rlfa_dest_lan = k_rlfa_dest_t<true>;

}  // namespace
