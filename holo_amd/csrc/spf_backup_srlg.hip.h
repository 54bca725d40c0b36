// spf_backup_srlg.hip.h — per-prefix backup routes that avoid the shared-risk link groups of the primaries
// (hspf_routes_backup_srlg_device; the semantics are written down once, in include/holo_spf_hip.h).  The kernels of
// spf_backup.hip.h and spf_srlg.hip.h are not instantiated again: their text is untouched, and what they share (BackupArgs,
// bk_term, bk_dist_to_prefix, bk_less, srlg_tab, frr_tab, frr_primaries) is used from here.  (k_backup_srlg is still a copy of
// backup_body with the member conditions in it: as an instantiation of one body over FrrProt it lost the registers of d_{b_i}(p)
// to scratch, profiles/r25_notes.md.)
//
// Staged blocks.  The slot tables and the prefix table are those of hspf_routes_backup_device; the member block is srlg_stage's
// (spf_srlg.hip.h), with ONE column appended behind `loc`:  pos [NM], the member's position within its tail's row.  No offset that
// srlg_tab reads moves; the column is reached through srlg_pos() below, which srlg_stage shares its two constants with.  d(N_k, a_i) and the members' costs come from the block that
// k_srlg_gather fills.
//
// Shape.  k_backup_srlg is k_backup — lane = prefix, 256 prefixes per workgroup, blockIdx.y = the protected root, candidate slots
// in chunks of BK_CH with d_N(p) in registers — with the member conditions behind every plain one.
//   one primary   d_{b_i}(p) of the primary's members is computed next to d_E(p), in front of the chunks, in ONE stream of the
//                 prefix's entries: per entry (v, m) one gather dist[head_row_i][v] per member; a primary with more than BKS_MCH
//                 members takes a second stream for members 8 .. 15.  All HSPF_SRLG_MAX_MEMBERS values stay in registers, packed
//                 to 33 bits (16 low words and one word of high bits; a sum is at most 0x1FFFFFFFD, so 0x1FFFFFFFF stands for
//                 "no advertiser reached").  As 16 x u64 next to 16 head rows the kernel took 147 VGPRs, in this form 131: one
//                 wave per SIMD fewer than k_backup.  With amdgpu_waves_per_eu(4) the compiler fits it into 104 VGPRs without
//                 scratch (profiles/r23_notes.md has the resource reports).  A candidate reads
//                 loc, d(N_k, a_i) and w_i only after it has passed every plain condition; a prefix whose primary has no member
//                 evaluates no member term and streams nothing more than k_backup does.
//   ECMP          sets only: a candidate that passed the plain conditions re-streams the entries per primary and member, as the
//                 plain kernel re-streams them per primary.
//   k_backup_cov_srlg   k_backup_cov_t<Srlg> (spf_backup.hip.h), ten words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_backup.hip.h"
#include "spf_srlg.hip.h"

namespace {

// The member columns of a root's block, each [NM], in the order srlg_stage writes them: the SRLG_TAB_COLS that srlg_tab names
// (tail | head | cost | trow | hrow | loc), then pos.  A further column that srlg_tab learns to read goes in FRONT of pos: raise
// SRLG_TAB_COLS, and the assertion keeps pos behind it.
constexpr uint32_t SRLG_TAB_COLS = 6, SRLG_POS_COL = 6, SRLG_STAGED_COLS = 7;
static_assert(SRLG_POS_COL >= SRLG_TAB_COLS && SRLG_POS_COL < SRLG_STAGED_COLS, "pos lies behind every column srlg_tab reads and inside the staged block");
__device__ __forceinline__ const uint32_t *srlg_pos(const SrlgTab &st) { return st.tail + (size_t)SRLG_POS_COL * st.NM; }      // (tail is column 0)

constexpr uint32_t BKS_MCH = 8;                    // member rows per stream of a prefix's entries

struct BackupSrlgArgs {
  SrlgArgs sa;
  const uint32_t *ti_p, *ti_link;                  // hspf_tilfa_out's forced adjacency, or NULL with ti_kind
  uint32_t repairs, pad;                           // HSPF_LFA_SRLG_SAFE_REPAIRS
};

// crosses_p(N_k, i): d(N_k, a_i) finite, d_{b_i}(p) exists (neither BK_NO_DIST nor its packed form), d_{N_k}(p) >= d(N_k, a_i) +
// w_i + d_{b_i}(p).  dbp < 2^33, so the sum stays far inside 64 bits.
constexpr uint64_t BKS_NO_DIST33 = 0x1FFFFFFFFull;
__device__ __forceinline__ bool bks_cross(uint64_t dNp, uint32_t dNa, uint32_t w, uint64_t dbp) {
  return dNa != LFA_NONE && dbp != BK_NO_DIST && dbp != BKS_NO_DIST33 && dNp >= (uint64_t)dNa + (uint64_t)w + dbp;
}

// d_{b_i}(p) in 33 bits: the low word, and bit j of `hi` for member j
__device__ __forceinline__ uint64_t bks_get(const uint32_t (&lo)[SRLG_MAXM], uint32_t hi, uint32_t j) { return (uint64_t)lo[j] | ((uint64_t)((hi >> j) & 1u) << 32); }
__device__ __forceinline__ void bks_set(uint32_t (&lo)[SRLG_MAXM], uint32_t &hi, uint32_t j, uint64_t x) {
  lo[j] = (uint32_t)x; hi = (hi & ~(1u << j)) | ((uint32_t)(x >> 32) << j);
}

// candidate k (root_link rlk, d_{N_k}(p) = d) against the members of primary q, their d_{b_i}(p) streamed here (the ECMP path)
__device__ __forceinline__ bool bks_safe_stream(const BackupArgs &a, const SrlgTab &st, uint32_t k, uint32_t rlk, uint32_t q, uint64_t d,
                                                uint32_t lo, uint32_t hi) {
  const uint32_t x1 = st.sptr[q + 1];
  for (uint32_t x = st.sptr[q]; x < x1; ++x) {
    const uint32_t i = st.sidx[x];
    if (st.loc[i] == rlk) return false;
    const uint32_t dNa = st.dNa[(size_t)k * st.NM + i];
    if (dNa == LFA_NONE) continue;
    if (bks_cross(d, dNa, st.cost[i], bk_dist_to_prefix(a, st.hrow[i], lo, hi))) return false;
  }
  return true;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_backup_srlg(BackupArgs a, BackupSrlgArgs b) {
  const uint32_t pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, a.scal, pi);
  const uint32_t K = tb.K, C = tb.C, n = a.n, W = a.W, Wk = tb.Wk;
  const uint32_t p = blockIdx.x * LFA_TILE + threadIdx.x;
  if (p >= a.n_pfx) return;                                                        // (no barrier below)
  const SrlgTab st = srlg_tab(b.sa, pi, K);
  const size_t oi = (size_t)tb.srow * a.n_pfx + p, oo = (size_t)pi * a.n_pfx + p;
  const uint32_t lo = a.pfx_ptr[p], hi = a.pfx_ptr[p + 1];
  const bool route = a.best_entry[oi] != LFA_NONE;
  const uint64_t dSp = a.best_metric[oi];
  const uint64_t *pm = a.nh_mask + oi * W;
  uint32_t np = 0, p0 = 0;
  if (route) frr_primaries(tb, pm, np, p0);
  uint32_t kind = !route ? 0u : np == 0 ? 1u : np >= 2 ? 2u : 6u;
  const bool sets = kind >= 2;                                                     // the two sets are evaluated and written
  uint32_t rl0 = LFA_NONE, E0 = LFA_NONE, s0 = 0, nm0 = 0;                         // s0, nm0: the one primary's members in sidx
  uint64_t dE0p = BK_NO_DIST;
  uint32_t dbl[SRLG_MAXM], dbh = 0xFFFFu;                                          // d_{b_i}(p) of the one primary's members (bks_get / bks_set)
  bool hasm = false;                                                               // some primary has members
  if (np == 1) {
    rl0 = tb.rl[p0]; E0 = tb.nbr[p0];
    s0 = st.sptr[p0]; nm0 = st.sptr[p0 + 1] - s0;
    nm0 = nm0 > SRLG_MAXM ? SRLG_MAXM : nm0;                                       // (the call checked it: the bound of the register array)
    hasm = nm0 != 0;
    // d_E(p) and the members' d_b(p): the entries streamed once
    const size_t ebase = (size_t)tb.row[p0] * n;
#pragma unroll
    for (uint32_t j = 0; j < SRLG_MAXM; ++j) dbl[j] = 0xFFFFFFFFu;
    if (E0 != LFA_NONE || hasm) {
#pragma unroll
      for (uint32_t m0 = 0; m0 < SRLG_MAXM; m0 += BKS_MCH) {                       // (one stream unless the primary has more than BKS_MCH members)
        if (m0 && m0 >= nm0) break;
        uint32_t hrow[BKS_MCH];
#pragma unroll
        for (uint32_t j = 0; j < BKS_MCH; ++j) hrow[j] = m0 + j < nm0 ? st.hrow[st.sidx[s0 + m0 + j]] : 0u;
        for (uint32_t e = lo; e < hi; ++e) {
          const uint32_t v = a.pfx_vertex[e], met = a.pfx_metric[e];
          if (!m0 && E0 != LFA_NONE) { const uint64_t t = bk_term(a, ebase + v, met); dE0p = t < dE0p ? t : dE0p; }
#pragma unroll
          for (uint32_t j = 0; j < BKS_MCH; ++j) {
            if (m0 + j >= nm0) break;
            const uint64_t t = bk_term(a, (size_t)hrow[j] * n + v, met);           // (BK_NO_DIST is above every packed value)
            if (t < bks_get(dbl, dbh, m0 + j)) bks_set(dbl, dbh, m0 + j, t);
          }
        }
      }
    }
  } else {
#pragma unroll
    for (uint32_t j = 0; j < SRLG_MAXM; ++j) dbl[j] = 0xFFFFFFFFu;
  }
  if (np >= 2 && st.T) {
    for (uint32_t w2 = 0; w2 < Wk; ++w2) {
      uint64_t x = frr_word(tb, pm, w2);
      while (x) {
        const uint32_t q = w2 * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
        x &= x - 1;
        hasm = hasm || st.sptr[q + 1] != st.sptr[q];
      }
    }
  }
  uint32_t sfl = (sets && hasm) ? 0x01u : 0u;                                      // HSPF_BK_SRLG_PRIMARY | _PAIR_REFUSED | HSPF_LFA_SRLG_REFUSED
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
        ok = rlk != rl0;                                                           // (k == p0 has p0's root_link)
        if (ok && hasm) {                                                          // every plain condition holds: now the group
          bool safe = true;
#pragma unroll
          for (uint32_t i2 = 0; i2 < SRLG_MAXM; ++i2) {
            if (i2 >= nm0) break;
            const uint32_t i = st.sidx[s0 + i2];
            safe = safe && st.loc[i] != rlk && !bks_cross(d, st.dNa[(size_t)k * st.NM + i], st.cost[i], bks_get(dbl, dbh, i2));
          }
          if (!safe) { ok = false; sfl |= 0x80u; }
        }
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
        if (ok && hasm) {
          bool safe = true;
          for (uint32_t w2 = 0; w2 < Wk && safe; ++w2) {
            uint64_t x = frr_word(tb, pm, w2);
            while (x && safe) {
              const uint32_t q = w2 * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u;
              x &= x - 1;
              safe = bks_safe_stream(a, st, k, rlk, q, d, lo, hi);
            }
          }
          if (!safe) { ok = false; sfl |= 0x80u; }
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
    } else if (a.ti_kind && !(hasm && !b.repairs)) {                               // (a primary with members: only repairs the caller vouches for)
      const size_t o = (size_t)pi * a.stride + p0;
      const uint32_t tk = a.ti_kind[o];
      bool forced = false;                                                         // the pair's forced adjacency is a member of the primary
      if (tk == 2u && hasm) {
        const uint32_t tp = b.ti_p[o], tl = b.ti_link[o];
        const uint32_t *pos = srlg_pos(st);
        for (uint32_t i2 = 0; i2 < nm0; ++i2) {
          const uint32_t i = st.sidx[s0 + i2];
          forced = forced || (st.tail[i] == tp && pos[i] == tl);
        }
      }
      if (forced) sfl |= 0x02u;
      else if (tk) { kind = tk == 1u ? 4u : 5u; slot = a.ti_via[o]; met = a.ti_metric[o]; }
    }
  }
  fl |= sfl;
  a.bk_kind[oo] = (uint8_t)kind; a.bk_primary[oo] = prim; a.bk_slot[oo] = slot; a.bk_metric[oo] = met; a.bk_flags[oo] = (uint8_t)fl;
}

}  // namespace
