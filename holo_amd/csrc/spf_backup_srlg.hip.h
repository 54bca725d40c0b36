// spf_backup_srlg.hip.h — per-prefix backup routes that avoid the shared-risk link groups of the primaries
// (hspf_routes_backup_srlg_device; the semantics are written down once, in include/holo_spf_hip.h).  k_backup_srlg is
// backup_body (spf_backup.hip.h) in the mode FrrProt::Srlg: this file holds the mode's arguments, its lane state with the four
// hooks the body calls, and BkMembers, the member lane that the per-primary ECMP fill (spf_backup_ecmp.hip.h) uses as well.
//
// Staged blocks.  The slot tables and the prefix table are those of hspf_routes_backup_device; the member block is srlg_stage's
// (spf_srlg.hip.h), with ONE column appended behind `loc`:  pos [NM], the member's position within its tail's row.  No offset that
// srlg_tab reads moves; the column is reached through srlg_pos() below, which srlg_stage shares its two constants with.
// d(N_k, a_i) and the members' costs come from the block that k_srlg_gather fills.
//
// BkMembers: what a lane keeps about the members of ONE primary h.
//   stream   d_{b_i}(p) of h's members in ONE stream of the prefix's entries: per entry (v, m) one gather dist[head_row_i][v] per
//            member; an h with more than BKS_MCH members takes a second stream for members 8 .. 15.  The per-prefix kernel folds
//            d_E(p) of a router primary into the first stream.  All HSPF_SRLG_MAX_MEMBERS values stay in registers, packed to 33
//            bits (16 low words in ONE 16-lane vector and one word of high bits; a sum is at most 0x1FFFFFFFD, so 0x1FFFFFFFF
//            stands for "no advertiser reached").  An h without members streams nothing (the kernel: nothing beyond d_E(p)).
//   safe     a candidate that has passed every plain condition against the members: none local to it, none crossed.  A loop to
//            the number of members: as a vector the values are indexed by a run-time count without leaving the registers (as an
//            array inside the lane's struct they went to scratch, and unrolled 16 times per slot of a chunk the kernel no longer
//            fitted four waves: profiles/r29_notes.md has both reports).  loc, d(N_k, a_i) and w_i are read only here.
//   forced   is the forced adjacency of a two-segment repair a member of h?
// The ECMP sets of the per-prefix kernel (two or more primaries, no slot is chosen) keep no values: bks_safe_stream re-streams
// the entries per primary and member, as the plain kernel re-streams them per primary; bks_member_ok is the one test of both.
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
typedef uint32_t bks_lo_t __attribute__((ext_vector_type(16)));
__device__ __forceinline__ uint64_t bks_get(const bks_lo_t &lo, uint32_t hi, uint32_t j) { return (uint64_t)lo[j] | ((uint64_t)((hi >> j) & 1u) << 32); }
__device__ __forceinline__ void bks_set(bks_lo_t &lo, uint32_t &hi, uint32_t j, uint64_t x) {
  lo[j] = (uint32_t)x; hi = (hi & ~(1u << j)) | ((uint32_t)(x >> 32) << j);
}

// member i against candidate k (root_link rlk, d_{N_k}(p) = d): it is not local to k and k's path to p does not cross it.
// dbp() yields d_{b_i}(p); it is asked only for a member that N_k reaches.
template <class F>
__device__ __forceinline__ bool bks_member_ok(const SrlgTab &st, uint32_t i, uint32_t k, uint32_t rlk, uint64_t d, F &&dbp) {
  if (st.loc[i] == rlk) return false;
  const uint32_t dNa = st.dNa[(size_t)k * st.NM + i];
  return dNa == LFA_NONE || !bks_cross(d, dNa, st.cost[i], dbp());
}

// candidate k against the members of primary q, their d_{b_i}(p) streamed here (the ECMP sets of the per-prefix kernel)
__device__ __forceinline__ bool bks_safe_stream(const BackupArgs &a, const SrlgTab &st, uint32_t k, uint32_t rlk, uint32_t q, uint64_t d,
                                                uint32_t lo, uint32_t hi) {
  const uint32_t x1 = st.sptr[q + 1];
  for (uint32_t x = st.sptr[q]; x < x1; ++x) {
    const uint32_t i = st.sidx[x];
    if (!bks_member_ok(st, i, k, rlk, d, [&] { return bk_dist_to_prefix(a, st.hrow[i], lo, hi); })) return false;
  }
  return true;
}

// What a lane keeps about the members of ONE primary h: where they stand in sidx, and their d_{b_i}(p), at most SRLG_MAXM values
// packed to 33 bits in registers.  Used by the one-primary path of k_backup_srlg and, per entry (p, h), by k_backup_ecmp_fill_srlg.
struct BkMembers {
  SrlgTab st;
  uint32_t s0 = 0, nm = 0;                                                         // the members of h: sidx[s0 .. s0 + nm)
  bks_lo_t dbl; uint32_t dbh = 0xFFFFu;                                            // their d_{b_i}(p) (bks_get / bks_set)

  __device__ __forceinline__ void clear() {
    s0 = 0; nm = 0; dbh = 0xFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < SRLG_MAXM; ++j) dbl[j] = 0xFFFFFFFFu;
  }
  // the members of h and their d_b(p): the prefix's entries lo .. hi streamed once per BKS_MCH member head rows.  With `extra` the
  // first stream also takes the minimum over row erow into dE (d_E(p) of a router primary).  Nothing is streamed for an h without
  // members unless `extra` asks for the row.
  template <class Args>
  __device__ __forceinline__ void stream(const Args &a, uint32_t h, uint32_t lo, uint32_t hi, bool extra = false, uint32_t erow = 0, uint64_t *dE = nullptr) {
    clear();
    s0 = st.sptr[h];
    nm = st.sptr[h + 1] - s0;
    nm = nm > SRLG_MAXM ? SRLG_MAXM : nm;                                          // (the call checked it: the bound of dbl)
    if (!nm && !extra) return;
    const size_t ebase = (size_t)erow * a.n;
#pragma unroll
    for (uint32_t m0 = 0; m0 < SRLG_MAXM; m0 += BKS_MCH) {                         // (one stream unless h has more than BKS_MCH members)
      if (m0 && m0 >= nm) break;
      uint32_t hrow[BKS_MCH];
#pragma unroll
      for (uint32_t j = 0; j < BKS_MCH; ++j) hrow[j] = m0 + j < nm ? st.hrow[st.sidx[s0 + m0 + j]] : 0u;
      for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t v = a.pfx_vertex[e], met = a.pfx_metric[e];
        if (!m0 && extra) { const uint64_t t = bk_term(a, ebase + v, met); *dE = t < *dE ? t : *dE; }
#pragma unroll
        for (uint32_t j = 0; j < BKS_MCH; ++j) {
          if (m0 + j >= nm) break;
          const uint64_t t = bk_term(a, (size_t)hrow[j] * a.n + v, met);           // (BK_NO_DIST is above every packed value)
          if (t < bks_get(dbl, dbh, m0 + j)) bks_set(dbl, dbh, m0 + j, t);
        }
      }
    }
  }
  // candidate k (root_link rlk, d_{N_k}(p) = d), which has passed every plain condition: no member of h is local to k, none is crossed
  __device__ __forceinline__ bool safe(uint32_t k, uint32_t rlk, uint64_t d) const {
    bool ok = true;
    // (a loop to nm, not an unrolled one: dbl is a vector, which the compiler indexes by a run-time count in registers.  The 128
    // unrolled tests of a chunk — as two loops of BKS_MCH — cost k_backup_srlg its fourth wave, profiles/r29_notes.md)
    for (uint32_t i2 = 0; i2 < nm && ok; ++i2) ok = bks_member_ok(st, st.sidx[s0 + i2], k, rlk, d, [&] { return bks_get(dbl, dbh, i2); });
    return ok;
  }
  // is the forced adjacency (tp, tl) of h's two-segment repair a member of h?
  __device__ __forceinline__ bool forced(uint32_t tp, uint32_t tl) const {
    const uint32_t *pos = srlg_pos(st);
    bool f = false;
    for (uint32_t i2 = 0; i2 < nm; ++i2) {
      const uint32_t i = st.sidx[s0 + i2];
      f = f || (st.tail[i] == tp && pos[i] == tl);
    }
    return f;
  }
};

// backup_body (spf_backup.hip.h) in the mode FrrProt::Srlg: its arguments, its lane state and the hooks the body calls
template <> struct BackupProt<FrrProt::Srlg> { BackupSrlgArgs s; };
template <> struct BackupLane<FrrProt::Srlg> {
  static constexpr bool STREAMS_DE = true;
  BkMembers mb;                                                                    // the one primary's
  uint32_t sfl = 0;                                                                // HSPF_BK_SRLG_PRIMARY | _PAIR_REFUSED | HSPF_LFA_SRLG_REFUSED
  bool hasm = false;                                                               // some primary has members

  __device__ __forceinline__ void open(const BackupArgs &a, const BackupProt<FrrProt::Srlg> &pa, const FrrTab &tb, uint32_t pi, const uint64_t *pm,
                                       uint32_t np, uint32_t p0, uint32_t lo, uint32_t hi, uint64_t &dE0p) {
    mb.st = srlg_tab(pa.s.sa, pi, tb.K);
    if (np == 1) {                                                                 // d_E(p) and the members' d_b(p): the entries streamed once
      mb.stream(a, p0, lo, hi, tb.nbr[p0] != LFA_NONE, tb.row[p0], &dE0p);
      hasm = mb.nm != 0;
    } else {
      mb.clear();
      if (np >= 2) hasm = mb.st.T && !frr_all_primaries(tb, pm, [&](uint32_t q) { return mb.st.sptr[q + 1] == mb.st.sptr[q]; });
    }
    if (hasm) sfl = 0x01u;
  }
  __device__ __forceinline__ bool one(uint32_t k, uint32_t rlk, uint64_t d) {
    if (!hasm || mb.safe(k, rlk, d)) return true;
    sfl |= 0x80u;
    return false;
  }
  __device__ __forceinline__ bool ecmp(const BackupArgs &a, const FrrTab &tb, const uint64_t *pm, uint32_t k, uint32_t rlk, uint64_t d, uint32_t lo, uint32_t hi) {
    if (!hasm || frr_all_primaries(tb, pm, [&](uint32_t q) { return bks_safe_stream(a, mb.st, k, rlk, q, d, lo, hi); })) return true;
    sfl |= 0x80u;
    return false;
  }
  __device__ __forceinline__ bool may_repair(const BackupProt<FrrProt::Srlg> &pa) const { return !hasm || pa.s.repairs; }   // (a primary with members: only repairs the caller vouches for)
  // a pair whose forced adjacency is a member of the primary is refused
  __device__ __forceinline__ bool repair(const BackupProt<FrrProt::Srlg> &pa, size_t o, uint32_t tk) {
    if (!(tk == 2u && hasm && mb.forced(pa.s.ti_p[o], pa.s.ti_link[o]))) return true;
    sfl |= 0x02u;
    return false;
  }
  __device__ __forceinline__ uint32_t flags() const { return sfl; }
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_backup_srlg(BackupArgs a, BackupProt<FrrProt::Srlg> pa) { backup_body(a, pa); }

}  // namespace
