// spf_srlg.hip.h — loop-free alternates and remote-LFA spaces that avoid a shared-risk link group (hspf_lfa_srlg_device,
// hspf_rlfa_srlg_device; the semantics are written down once, in include/holo_spf_hip.h).  The local kernel is lfa_body
// (spf_lfa.hip.h) in the mode FrrProt::Srlg.  The remote kernels are their own: they split the slots differently from k_rlfa_t
// (spf_rlfa.hip.h), and use what they share with it (lfa_less, frr_tab, frr_primaries, frr_cover, rlfa_wave_min) from here.
//
// The member block (written by srlg_stage in spf_frr.hip.h, read here and nowhere else) is a THIRD pair of blocks next to the slot
// tables and the LAN block.  `stab`:
//   [n_prot][SRLG_HDR_WORDS] headers:  word 0  NM   the distinct members of the root's slots
//                                      word 1  offset (in words, from `stab`) of the root's columns
//                                      word 2  offset (in words, from `sscal`) of the root's scalars
//                                      word 3  T    the length of the index list
//                                      word 4  NMS  the candidate slots that have members;   words 5 .. 7  0
//   then per root, at its offset:  sptr [K + 1] | msl [K] | sidx [T] | tail | head | cost | trow | hrow | loc  (each [NM])
//     the members of slot k are sidx[sptr[k] .. sptr[k + 1]), indices into the NM distinct members (slots behind one link of S
//     share them); msl holds the NMS candidate slots with members in ascending order (its other words are 0); loc[i] is the
//     member's position in S's own row when its tail is S, LFA_NONE otherwise: member i is local to slot k iff loc[i] == root_link[k].
// `sscal` is k_srlg_gather's output, per root at its offset:  d(S, a_i) [NM] | d(N_k, a_i) [K][NM] | d(b_i, N_k) [K][NM]  (LFA_NONE
// where slot k is no candidate or the vertex is not reached): every term of a crossing that does not depend on the lane.
//
// Shape.  k_lfa_srlg<ONE> is lfa_body<ONE, Srlg>: the member conditions stand behind every plain one, so a candidate that passed them reads
// d(b_i, D) of the primary's members — rows the destination's neighbours in the wave read too — and the scalar next to it.
// A destination whose primaries have no member evaluates no member term.
// The remote call splits the candidate slots of a root in two:
//   k_rlfa_srlg       the slots WITHOUT members, in chunks of RLFA_CH exactly as k_rlfa (five count words per slot);
//   k_rlfa_srlg_slot  one workgroup per (256 vertices, slot WITH members): the lane keeps d(b_i, v) of the slot's at most
//                     HSPF_SRLG_MAX_MEMBERS members in registers — each loaded once, with d(v, a_i) next to it for the Q side — and
//                     streams the via-slots once; d(N_k, a_i), d(S, a_i), d(b_i, E) and the members' costs are wave-uniform reads,
//                     so the via-slot stream adds no per-lane load.  The plain sets are kept as three more bits, for the fifth
//                     count word only.
//   k_rlfa_srlg_final / k_rlfa_srlg_dest   as k_rlfa_final / k_rlfa_dest, under the same member conditions / with two more words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_lfa.hip.h"
#include "spf_rlfa.hip.h"

namespace {

constexpr uint32_t SRLG_HDR_WORDS = 8;
constexpr uint32_t SRLG_MAXM = 16;                 // HSPF_SRLG_MAX_MEMBERS (held to it in spf_frr.hip.h)
constexpr uint32_t RLFA_SRLG_CW = 5;               // HSPF_RLFA_SRLG_COUNT_WORDS (the same)

struct SrlgArgs { const uint32_t *stab; uint32_t *sscal; };
struct SrlgTab {
  uint32_t NM, T, NMS;
  const uint32_t *sptr, *msl, *sidx;                      // [K + 1] | [K] | [T]
  const uint32_t *tail, *head, *cost, *trow, *hrow, *loc; // [NM] each
  const uint32_t *dSa, *dNa, *dbN;                        // [NM] | [K][NM] | [K][NM]
};
__device__ __forceinline__ SrlgTab srlg_tab(const SrlgArgs &sa, uint32_t pi, uint32_t K) {
  const uint32_t *hdr = sa.stab + (size_t)pi * SRLG_HDR_WORDS;
  const uint32_t NM = hdr[0], T = hdr[3];
  const uint32_t *c = sa.stab + hdr[1], *m = c + 2 * K + 1 + T;
  const uint32_t *s = sa.sscal + hdr[2];
  return SrlgTab{NM, T, hdr[4], c, c + K + 1, c + 2 * K + 1, m, m + NM, m + 2 * NM, m + 3 * NM, m + 4 * NM, m + 5 * NM,
                 s, s + NM, s + NM + (size_t)K * NM};
}

// crosses(X -> v, i): d(X, a_i) and d(b_i, v) are both finite and d(X, v) >= d(X, a_i) + w_i + d(b_i, v), in 64 bits.  A member
// that X does not reach, or whose head does not reach v, is not crossed (unlike lfa_less, where an infinite term refuses).
__device__ __forceinline__ bool srlg_cross(uint32_t dxv, uint32_t dxa, uint32_t w, uint32_t dbv) {
  return dxa != LFA_NONE && dbv != LFA_NONE && (uint64_t)dxv >= (uint64_t)dxa + (uint64_t)w + (uint64_t)dbv;
}

// the per-root scalars of the member conditions
__global__ __launch_bounds__(256) void k_srlg_gather(LfaArgs a, SrlgArgs sa) {
  const FrrTab tb = frr_tab(a.tab, blockIdx.y);
  const uint32_t K = tb.K;
  const SrlgTab st = srlg_tab(sa, blockIdx.y, K);
  const uint32_t NM = st.NM, KN = K * NM, total = NM + 2 * KN;
  uint32_t *out = sa.sscal + sa.stab[(size_t)blockIdx.y * SRLG_HDR_WORDS + 2];
  for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < total; x += gridDim.x * 256u) {
    uint32_t v = LFA_NONE;
    if (x < NM) v = a.dist[(size_t)tb.srow * a.n + st.tail[x]];
    else if (x < NM + KN) {
      const uint32_t k = (x - NM) / NM, i = (x - NM) - k * NM;
      if (tb.nbr[k] != LFA_NONE) v = a.dist[(size_t)tb.row[k] * a.n + st.tail[i]];
    } else {
      const uint32_t k = (x - NM - KN) / NM, i = (x - NM - KN) - k * NM;
      if (tb.nbr[k] != LFA_NONE) v = a.dist[(size_t)st.hrow[i] * a.n + tb.nbr[k]];
    }
    out[x] = v;
  }
}

// candidate k (root_link rlk, d(N_k, D) = dND) against the members of primary p: no member is local to k, none is crossed
__device__ __forceinline__ bool srlg_lfa_safe(const LfaArgs &a, const SrlgTab &st, uint32_t k, uint32_t rlk, uint32_t p, uint32_t dND, uint32_t D) {
  const uint32_t x1 = st.sptr[p + 1];
  for (uint32_t x = st.sptr[p]; x < x1; ++x) {
    const uint32_t i = st.sidx[x];
    if (st.loc[i] == rlk) return false;
    if (srlg_cross(dND, st.dNa[(size_t)k * st.NM + i], st.cost[i], a.dist[(size_t)st.hrow[i] * a.n + D])) return false;
  }
  return true;
}

// lfa_body (spf_lfa.hip.h) in the mode FrrProt::Srlg: its arguments, its lane state and the member conditions the body calls
template <> struct LfaProt<FrrProt::Srlg> { SrlgArgs sa; };
template <> struct LfaLane<FrrProt::Srlg> {
  SrlgTab st;
  bool applies = false;                                                            // some primary has members

  __device__ __forceinline__ void open(const LfaProt<FrrProt::Srlg> &pa, uint32_t pi, uint32_t K) { st = srlg_tab(pa.sa, pi, K); }
  __device__ __forceinline__ void one_primary(uint32_t p0) { applies = st.sptr[p0 + 1] != st.sptr[p0]; }
  __device__ __forceinline__ void any_primary(const FrrTab &tb, const uint64_t *pm) {
    applies = st.T && !frr_all_primaries(tb, pm, [&](uint32_t p) { return st.sptr[p + 1] == st.sptr[p]; });
  }
  __device__ __forceinline__ bool safe_one(const LfaArgs &a, uint32_t k, uint32_t rlk, uint32_t p0, uint32_t dND, uint32_t D) const {
    return srlg_lfa_safe(a, st, k, rlk, p0, dND, D);
  }
  __device__ __forceinline__ bool safe_ecmp(const LfaArgs &a, const FrrTab &tb, const uint64_t *pm, uint32_t k, uint32_t rlk, uint32_t dND, uint32_t D) const {
    return frr_all_primaries(tb, pm, [&](uint32_t p) { return srlg_lfa_safe(a, st, k, rlk, p, dND, D); });
  }
};

template <bool ONE>
__global__ __launch_bounds__(256) void k_lfa_srlg(LfaArgs a, LfaProt<FrrProt::Srlg> pa) { lfa_body<ONE>(a, pa); }

// what every lane of the two remote kernels starts from
struct RlfaLane { uint32_t v, vv, dSv, rSv; bool valid, elig; };
__device__ __forceinline__ RlfaLane rlfa_lane(const RlfaArgs &a, const FrrTab &tb) {
  RlfaLane l;
  l.v = blockIdx.x * LFA_TILE + threadIdx.x;
  l.valid = l.v < a.n;
  l.vv = l.valid ? l.v : 0u;
  const size_t sv = (size_t)tb.srow * a.n + l.vv;
  l.dSv = a.dist[sv]; l.rSv = a.rdist[sv];
  const uint32_t f = a.vf[l.vv];
  l.elig = l.valid && l.v != tb.S && (a.flags[sv] & 1u) && l.dSv != LFA_NONE && !(f & 0x05u) && (!(f & 0x02u) || a.ignore_overload);
  return l;
}

// the candidate slots without members: k_rlfa (spf_rlfa.hip.h) with five count words; a slot with members is left to
// k_rlfa_srlg_slot (its place in the chunk stays empty)
__global__ __launch_bounds__(256) void k_rlfa_srlg(RlfaArgs a, SrlgArgs sa) {
  constexpr uint32_t CW = RLFA_SRLG_CW;
  __shared__ uint32_t s_cnt[RLFA_CH * CW];
  __shared__ unsigned long long s_key[RLFA_CH];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const SrlgTab st = srlg_tab(sa, pi, tb.K);
  const uint32_t C = tb.C, n = a.n;
  const RlfaLane L = rlfa_lane(a, tb);
  const uint32_t v = L.v, vv = L.vv, dSv = L.dSv, rSv = L.rSv;
  const bool valid = L.valid, elig = L.elig;
  const size_t slot0 = (size_t)pi * a.stride;
  if (tid < RLFA_CH * CW) s_cnt[tid] = 0;
  if (tid < RLFA_CH) s_key[tid] = RLFA_NO_KEY;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < C; c0 += RLFA_CH) {
    uint64_t t[RLFA_CH], best[RLFA_CH];
    uint32_t via[RLFA_CH], rle[RLFA_CH], es[RLFA_CH];
    uint32_t tm = 0, pm = 0, qm = 0, xm = 0, lm = 0;                               // bit j: t[j] is finite | P | Q | some XP | the slot is this kernel's
#pragma unroll
    for (uint32_t j = 0; j < RLFA_CH; ++j) {
      const uint32_t e = tb.cl[c0 + j < C ? c0 + j : c0];
      const bool live = c0 + j < C && st.sptr[e + 1] == st.sptr[e];                // wave-uniform
      es[j] = e; rle[j] = tb.rl[e];
      const size_t ev = (size_t)tb.row[e] * n + vv;
      const uint32_t c = tb.cost[e], dEv = a.dist[ev], rEv = a.rdist[ev];
      t[j] = (uint64_t)c + dEv;
      const bool tok = live && elig && dEv != LFA_NONE;
      const bool p = tok && (uint64_t)dSv < t[j];
      const bool q = live && elig && lfa_less(rEv, rSv, c);
      lm |= (live ? 1u : 0u) << j;
      tm |= (tok ? 1u : 0u) << j; pm |= (p ? 1u : 0u) << j; qm |= (q ? 1u : 0u) << j;
      best[j] = p ? (uint64_t)dSv : ~0ull;
      via[j] = p ? RLFA_VIA_SELF : LFA_NONE;
    }
    if (__ballot(tm != 0)) {                                                       // the via-slots, once per chunk
      for (uint32_t ci = 0; ci < C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if ((tb.cf[k] & 1u) && !a.ignore_overload) continue;
        const uint32_t dNS = tb.dns[k];
        if (dNS == LFA_NONE) continue;
        const uint32_t dNv = a.dist[(size_t)tb.row[k] * n + vv], rlk = tb.rl[k];
        const uint64_t rel = (uint64_t)tb.cost[k] + dNv;
        const uint32_t okm = dNv != LFA_NONE ? tm : 0u;
#pragma unroll
        for (uint32_t j = 0; j < RLFA_CH; ++j) {
          if (((okm >> j) & 1u) && rlk != rle[j] && (uint64_t)dNv < (uint64_t)dNS + t[j]) {
            xm |= 1u << j;
            if (rel < best[j]) { best[j] = rel; via[j] = k; }
          }
        }
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < RLFA_CH; ++j) {
      if (!((lm >> j) & 1u)) continue;                                             // (wave-uniform)
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
  if (valid && (a.space_flags || a.space_via)) {                                   // the optional tables of the slots that are no candidates: "none"
    for (uint32_t e = 0; e < a.stride; ++e) {
      if (e < tb.K && tb.nbr[e] != LFA_NONE) continue;
      const size_t o = (slot0 + e) * n + v;
      if (a.space_flags) a.space_flags[o] = 0;
      if (a.space_via) a.space_via[o] = LFA_NONE;
    }
  }
}

// one candidate slot with members per (workgroup, turn): blockIdx.y walks the root's list msl
__global__ __launch_bounds__(256) void k_rlfa_srlg_slot(RlfaArgs a, SrlgArgs sa) {
  constexpr uint32_t CW = RLFA_SRLG_CW;
  __shared__ uint32_t s_cnt[CW];
  __shared__ unsigned long long s_key;
  __shared__ uint32_t s_mi[SRLG_MAXM], s_w[SRLG_MAXM], s_loc[SRLG_MAXM], s_hrow[SRLG_MAXM], s_trow[SRLG_MAXM], s_dSa[SRLG_MAXM], s_dbE[SRLG_MAXM];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, pi = blockIdx.z;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const SrlgTab st = srlg_tab(sa, pi, tb.K);
  const uint32_t C = tb.C, n = a.n, NM = st.NM;
  const RlfaLane L = rlfa_lane(a, tb);
  const uint32_t v = L.v, vv = L.vv, dSv = L.dSv, rSv = L.rSv;
  const bool valid = L.valid, elig = L.elig;
  const size_t slot0 = (size_t)pi * a.stride;
  for (uint32_t ms = blockIdx.y; ms < st.NMS; ms += gridDim.y) {                   // (uniform over the workgroup)
    const uint32_t e = st.msl[ms], m0 = st.sptr[e];
    const uint32_t nm = min(st.sptr[e + 1] - m0, SRLG_MAXM);                       // (the call refuses more: the clamp keeps the registers' bound local)
    __syncthreads();                                                               // the turn before has read its members
    if (tid < SRLG_MAXM) {
      const uint32_t i = tid < nm ? st.sidx[m0 + tid] : 0u;
      s_mi[tid] = i; s_w[tid] = st.cost[i]; s_loc[tid] = st.loc[i]; s_hrow[tid] = st.hrow[i]; s_trow[tid] = st.trow[i];
      s_dSa[tid] = st.dSa[i]; s_dbE[tid] = st.dbN[(size_t)e * NM + i];
    }
    if (tid < CW) s_cnt[tid] = 0;
    if (tid == 0) s_key = RLFA_NO_KEY;
    __syncthreads();
    const uint32_t rle = tb.rl[e], c = tb.cost[e];
    const size_t ev = (size_t)tb.row[e] * n + vv;
    const uint32_t dEv = a.dist[ev], rEv = a.rdist[ev];
    const uint64_t t = (uint64_t)c + dEv;
    const bool tok = elig && dEv != LFA_NONE;
    const bool pp = tok && (uint64_t)dSv < t, qp = elig && lfa_less(rEv, rSv, c);  // the plain P and Q
    bool p = pp, q = qp, xp = false, x = false;
    uint32_t mb[SRLG_MAXM];                                                        // d(b_i, v)
#pragma unroll
    for (uint32_t i = 0; i < SRLG_MAXM; ++i) {
      mb[i] = LFA_NONE;
      if (i < nm) {
        mb[i] = a.dist[(size_t)s_hrow[i] * n + vv];
        const uint32_t rav = a.rdist[(size_t)s_trow[i] * n + vv];                  // d(v, a_i)
        if (srlg_cross(dSv, s_dSa[i], s_w[i], mb[i])) p = false;
        if (srlg_cross(rEv, rav, s_w[i], s_dbE[i])) q = false;
      }
    }
    uint64_t best = p ? (uint64_t)dSv : ~0ull;
    uint32_t via = p ? RLFA_VIA_SELF : LFA_NONE;
    if (__ballot(tok)) {
      for (uint32_t ci = 0; ci < C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if ((tb.cf[k] & 1u) && !a.ignore_overload) continue;
        const uint32_t dNS = tb.dns[k], rlk = tb.rl[k];
        if (dNS == LFA_NONE || rlk == rle) continue;
        const uint32_t dNv = a.dist[(size_t)tb.row[k] * n + vv];
        if (!(tok && dNv != LFA_NONE && (uint64_t)dNv < (uint64_t)dNS + t)) continue;
        xp = true;
        bool ok = true;
        const uint32_t *dNa = st.dNa + (size_t)k * NM;
#pragma unroll
        for (uint32_t i = 0; i < SRLG_MAXM; ++i)
          if (i < nm && (s_loc[i] == rlk || srlg_cross(dNv, dNa[s_mi[i]], s_w[i], mb[i]))) ok = false;
        if (!ok) continue;
        x = true;
        const uint64_t rel = (uint64_t)tb.cost[k] + dNv;
        if (rel < best) { best = rel; via = k; }
      }
    }
    const bool ext = p || x, pq = ext && q, lost = (pp || xp) && qp && !pq;
    const uint32_t c_p = (uint32_t)__popcll(__ballot(p)), c_x = (uint32_t)__popcll(__ballot(ext)), c_q = (uint32_t)__popcll(__ballot(q));
    const unsigned long long b_pq = __ballot(pq), b_lost = __ballot(lost);
    if (lane == 0) {
      if (c_p) atomicAdd(&s_cnt[0], c_p);
      if (c_x) atomicAdd(&s_cnt[1], c_x);
      if (c_q) atomicAdd(&s_cnt[2], c_q);
      if (b_pq) atomicAdd(&s_cnt[3], (uint32_t)__popcll(b_pq));
      if (b_lost) atomicAdd(&s_cnt[4], (uint32_t)__popcll(b_lost));
    }
    if (b_pq) {
      const uint64_t sat = best > 0xFFFFFFFEull ? 0xFFFFFFFEull : best;
      const unsigned long long key = rlfa_wave_min(pq ? (unsigned long long)((sat << 32) | v) : RLFA_NO_KEY);
      if (lane == 0) atomicMin(&s_key, key);
    }
    if (valid) {
      const size_t o = (slot0 + e) * n + v;
      if (a.space_flags) a.space_flags[o] = (uint8_t)((p ? 1u : 0u) | (x ? 2u : 0u) | (q ? 4u : 0u) | (elig ? 8u : 0u));
      if (a.space_via) a.space_via[o] = via;
    }
    __syncthreads();
    if (tid < CW && s_cnt[tid]) atomicAdd(a.pq_counts + (slot0 + e) * CW + tid, s_cnt[tid]);
    if (tid == 0 && s_key != RLFA_NO_KEY) atomicMin(a.key + slot0 + e, s_key);
  }
}

// one thread per (protected root, slot): key -> pq_node / pq_metric, and the via of that one vertex again, under the member
// conditions of the slot
__global__ __launch_bounds__(256) void k_rlfa_srlg_final(RlfaArgs a, uint32_t n_prot, SrlgArgs sa) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_prot * a.stride) return;
  const uint32_t pi = i / a.stride, e = i - pi * a.stride;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const uint32_t n = a.n;
  uint32_t node = LFA_NONE, via = LFA_NONE, met = 0;
  const unsigned long long key = a.key[i];
  if (e < tb.K && tb.nbr[e] != LFA_NONE && key != RLFA_NO_KEY) {
    node = (uint32_t)key; met = (uint32_t)(key >> 32);
    const SrlgTab st = srlg_tab(sa, pi, tb.K);
    const uint32_t m0 = st.sptr[e], m1 = st.sptr[e + 1];
    const uint32_t dSv = a.dist[(size_t)tb.srow * n + node], dEv = a.dist[(size_t)tb.row[e] * n + node];
    if (dEv != LFA_NONE) {                                                         // (a PQ node has a P or an XP: d(E, v) is finite)
      const uint64_t t = (uint64_t)tb.cost[e] + dEv;
      uint64_t best = ~0ull;
      bool safe = true;                                                            // S's own path to the node crosses no member
      for (uint32_t x = m0; x < m1 && safe; ++x) {
        const uint32_t m = st.sidx[x];
        safe = !srlg_cross(dSv, st.dSa[m], st.cost[m], a.dist[(size_t)st.hrow[m] * n + node]);
      }
      if (dSv != LFA_NONE && (uint64_t)dSv < t && safe) { best = dSv; via = RLFA_VIA_SELF; }
      for (uint32_t ci = 0; ci < tb.C; ++ci) {
        const uint32_t k = tb.cl[ci];
        if ((tb.cf[k] & 1u) && !a.ignore_overload) continue;
        const uint32_t dNS = tb.dns[k], dNv = a.dist[(size_t)tb.row[k] * n + node], rlk = tb.rl[k];
        if (dNS == LFA_NONE || dNv == LFA_NONE || rlk == tb.rl[e] || !((uint64_t)dNv < (uint64_t)dNS + t)) continue;
        bool ok = true;
        for (uint32_t x = m0; x < m1 && ok; ++x) {
          const uint32_t m = st.sidx[x];
          ok = st.loc[m] != rlk && !srlg_cross(dNv, st.dNa[(size_t)k * st.NM + m], st.cost[m], a.dist[(size_t)st.hrow[m] * n + node]);
        }
        if (!ok) continue;
        const uint64_t rel = (uint64_t)tb.cost[k] + dNv;
        if (rel < best) { best = rel; via = k; }
      }
    }
  }
  a.pq_node[i] = node; a.pq_via[i] = via; a.pq_metric[i] = met;
}

// k_rlfa_dest with two more words: the one-primary destinations whose primary has members | of those, the uncovered ones whose
// slot had a plain PQ node
__global__ __launch_bounds__(256) void k_rlfa_srlg_dest(RlfaArgs a, SrlgArgs sa) {
  constexpr uint32_t NC = 6;
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
      const SrlgTab st = srlg_tab(sa, pi, tb.K);
      if (st.sptr[p0 + 1] != st.sptr[p0]) {
        fl |= 16u;
        const uint32_t *cnt = a.pq_counts + ((size_t)pi * a.stride + p0) * RLFA_SRLG_CW;
        if ((fl & 8u) && cnt[3] + cnt[4] != 0) fl |= 32u;                          // the plain sets had a PQ node
      }
    }
  }
  if (valid) { a.rl_node[od] = node; a.rl_via[od] = via; }
  frr_cover<NC>(fl, s_cov, a.rl_cov + (size_t)pi * NC);
}

}  // namespace
