// spf_tilfa_pc.hip.h — TI-LFA repairs along the post-convergence path (link protection): per (protected root S, destination D with
// one primary slot e) the segment list that follows D's path in the SPT S has AFTER link e failed — the row of
// hspf_run_failures_device for that link — from the space tables hspf_rlfa_device wrote and the device graph's in-link arrays
// (hspf_tilfa_pc_device; the semantics are written down once, in include/holo_spf_hip.h).
//
// Shape.  As spf_tilfa.hip.h: lane = vertex, 256 consecutive vertices per workgroup.
//   k_tipc_parent  grid y = the (protected root, slot) pairs that have a post-convergence row (the call's list), x = vertex tiles.
//                  The lane scans its vertex's in-links once — (source | overload bit, cost, position in the source's row), the
//                  links that survive the two-way check, what k_dag<.., FAIL = true> reads — and keeps the smallest (u, j) among the
//                  tight, usable ones: pc[u] + w == pc[v], u expandable under the run's overload rule, not the failed link.  It
//                  writes the pair into the call's scratch [pairs][n], 8 bytes per entry, coalesced; (NONE, NONE) for S, for a
//                  vertex the row does not reach and for a vertex without such a link.
//   k_tipc_walk    lane = destination over S's mask row (as k_tilfa_dest), frr_primaries for the one slot.  The walk reads one
//                  parent pair (8 bytes) and one flag byte per step, both gathers; the four recorded hops stay in registers.  The
//                  lanes of a wave walk paths of different lengths: the wave runs as long as its longest, capped by max_walk.
//                  Coverage through frr_cover<12>.
// The parent scan is a kernel of its own and not folded into the walk: the paths of the destinations of one slot share their
// upper parts, so a walk that scanned in-links itself would scan the rows near S once per destination below them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_tilfa.hip.h"

namespace {

constexpr uint32_t TIPC_MAX_ADJ = 4;       // HSPF_TIPC_MAX_ADJ
constexpr uint32_t TIPC_COV = 12;          // HSPF_TIPC_COVERAGE_WORDS
constexpr uint32_t TIPC_SRC_NT = 0x80000000u, TIPC_SRC_MASK = 0x3FFFFFFFu;      // GraphDev::in_src (spf_kernels.hip.h: SRC_NO_TRANSIT, SRC_MASK)
constexpr uint32_t TIPC_LFA = 1, TIPC_REPAIR = 2, TIPC_NONE = 3, TIPC_LONG = 4, TIPC_LAN = 5, TIPC_WALK = 6;      // HSPF_TIPC_D_*
constexpr uint32_t TIPC_F_ON_PC = 1, TIPC_F_P_IS_ROOT = 2, TIPC_F_Q_IS_DEST = 4;                                  // HSPF_TIPC_*

struct TipcArgs {
  uint32_t n, W, stride, ignore_overload, max_walk, n_pairs;
  const uint32_t *dist; const uint16_t *flags; const uint64_t *mask;       // the forward table set
  const uint32_t *tab;                                                     // as LfaArgs (staged by the call)
  const uint8_t *alt_in;                                                   // [n_prot][n] alt_flags of hspf_lfa_device, or NULL
  const uint8_t *sflags; const uint32_t *svia;                             // [n_prot][stride][n] of hspf_rlfa_device
  const uint32_t *pc_dist;                                                 // [n_pc_rows][n] dist of hspf_run_failures_device
  const uint32_t *prow, *pidx, *plist;                                     // staged: [n_prot][stride] row of pc_dist | index into `par` (LFA_NONE: no row); [n_pairs] the (root, slot) pairs
  const uint32_t *in_ptr, *in_src, *in_w, *in_fpos; const uint8_t *vflags; // the device graph: in-links after the two-way check, resident vertex flags
  uint2 *par;                                                              // [n_pairs][n] scratch: (parent, position in its row)
  uint8_t *tp_kind, *tp_n_adj, *tp_flags;
  uint32_t *tp_p, *tp_via, *tp_q, *tp_hop_pos, *tp_hop_head, *tp_metric, *tp_cov;
};

__global__ __launch_bounds__(256) void k_tipc_parent(TipcArgs a) {
  const uint32_t n = a.n;
  const uint32_t v = blockIdx.x * LFA_TILE + threadIdx.x;
  if (v >= n) return;
  const uint32_t e0 = a.in_ptr[v], e1 = a.in_ptr[v + 1];
  for (uint32_t it = blockIdx.y; it < a.n_pairs; it += gridDim.y) {
    const uint32_t i = a.plist[it], pi = i / a.stride, e = i - pi * a.stride;
    const FrrTab tb = frr_tab(a.tab, pi);
    const uint32_t S = tb.S, fpos = tb.rl[e];
    const uint32_t *pc = a.pc_dist + (size_t)a.prow[i] * n;
    const uint32_t dv = pc[v];
    uint32_t bu = LFA_NONE, bj = LFA_NONE;
    if (v != S && dv != LFA_NONE) {
      for (uint32_t k = e0; k < e1; ++k) {
        const uint32_t raw = a.in_src[k], u = raw & TIPC_SRC_MASK;
        if (u >= n) continue;
        if (!a.ignore_overload && (raw & TIPC_SRC_NT) && u != S) continue;           // not expanded unless root
        const uint32_t j = a.in_fpos[k];
        if (u == S && j == fpos) continue;                                           // the failed link
        const uint32_t du = pc[u];
        if (du == LFA_NONE || (uint64_t)du + a.in_w[k] != dv) continue;              // tight, in 64 bits
        if (u < bu || (u == bu && j < bj)) { bu = u; bj = j; }
      }
    }
    a.par[(size_t)it * n + v] = make_uint2(bu, bj);
  }
}

__global__ __launch_bounds__(256) void k_tipc_walk(TipcArgs a) {
  __shared__ uint32_t s_cov[TIPC_COV];
  const uint32_t tid = threadIdx.x, pi = blockIdx.y;
  const FrrTab tb = frr_tab(a.tab, pi);
  const uint32_t n = a.n, S = tb.S;
  if (tid < TIPC_COV) s_cov[tid] = 0;
  __syncthreads();
  const uint32_t D = blockIdx.x * LFA_TILE + tid;
  const bool valid = D < n;
  const size_t sd = (size_t)tb.srow * n + (valid ? D : 0u);
  const size_t od = (size_t)pi * n + D;
  const bool in = valid && D != S && (a.flags[sd] & 1u) && a.dist[sd] != LFA_NONE;
  uint32_t cls = 0, p = LFA_NONE, q = LFA_NONE, via = LFA_NONE, gap = 0, met = 0, fl = 0;
  uint32_t hpos[TIPC_MAX_ADJ], hhead[TIPC_MAX_ADJ];      // in the order of recording: q first, towards p
#pragma unroll
  for (uint32_t h = 0; h < TIPC_MAX_ADJ; ++h) { hpos[h] = LFA_NONE; hhead[h] = LFA_NONE; }
  if (in) {
    uint32_t np, e;
    frr_primaries(tb, a.mask + sd * a.W, np, e);
    if (np == 1) {
      const size_t i = (size_t)pi * a.stride + e;
      const uint32_t it = (e < tb.K && tb.nbr[e] != LFA_NONE) ? a.pidx[i] : LFA_NONE;
      if (a.alt_in && (a.alt_in[od] & 0x04u)) cls = TIPC_LFA;                      // HSPF_LFA_LINK_PROTECT: LFA covers it
      else if (it == LFA_NONE) cls = TIPC_NONE;
      else {
        const uint32_t *pc = a.pc_dist + (size_t)a.prow[i] * n;
        const uint2 *par = a.par + (size_t)it * n;
        const uint8_t *sf = a.sflags + i * n;
        const uint32_t *sv = a.svia + i * n;
        TilfaArgs ta{};                                                            // what tilfa_rel reads
        ta.n = n; ta.dist = a.dist;
        const uint32_t pcD = pc[D];
        cls = pcD == LFA_NONE ? TIPC_NONE : TIPC_WALK;
        uint32_t cur = D;
        bool lan = false;
        uint64_t rel = 0;
        q = D;
        for (uint32_t step = 0; cls == TIPC_WALK && step < a.max_walk; ++step) {
          const uint32_t f = sf[cur];
          if ((f & 0x0Cu) == 0x0Cu) { q = cur; gap = 0; lan = false; }             // eligible and in Q: the list starts again here
          if ((f & 0x08u) && (f & 0x03u) && tilfa_rel(ta, tb, sv[cur], cur, rel)) { p = cur; via = sv[cur]; cls = TIPC_REPAIR; break; }
          if (cur == S) { p = S; rel = 0; cls = TIPC_REPAIR; break; }
          const uint2 pr = par[cur];
          if (pr.x == LFA_NONE) { cls = TIPC_NONE; break; }                        // (no tight parent: not a row of this link)
          if (gap && (a.vflags[cur] & 1u)) lan = true;                             // HSPF_VF_NETWORK strictly between p and q
#pragma unroll
          for (uint32_t h = 0; h < TIPC_MAX_ADJ; ++h)
            if (gap == h) { hpos[h] = pr.y; hhead[h] = cur; }
          ++gap;
          cur = pr.x;
        }
        if (cls == TIPC_REPAIR) {
          if (gap > TIPC_MAX_ADJ) cls = TIPC_LONG;
          else if (lan) cls = TIPC_LAN;
        }
        if (cls == TIPC_REPAIR) {
          const uint32_t pcp = p == S ? 0u : pc[p];
          const uint64_t t = rel + pcD - pcp;
          met = (uint32_t)(t > TILFA_SAT ? TILFA_SAT : t);
          fl = (rel == pcp ? TIPC_F_ON_PC : 0u) | (p == S ? TIPC_F_P_IS_ROOT : 0u) | (q == D ? TIPC_F_Q_IS_DEST : 0u);
        } else { p = LFA_NONE; q = LFA_NONE; via = LFA_NONE; gap = 0; }
      }
    }
  }
  if (valid) {
    a.tp_kind[od] = (uint8_t)cls; a.tp_n_adj[od] = (uint8_t)gap; a.tp_flags[od] = (uint8_t)fl;
    a.tp_p[od] = p; a.tp_via[od] = via; a.tp_q[od] = q; a.tp_metric[od] = met;
#pragma unroll
    for (uint32_t h = 0; h < TIPC_MAX_ADJ; ++h) {                                  // the order p -> q: the last recorded hop first
      uint32_t hp = LFA_NONE, hh = LFA_NONE;
#pragma unroll
      for (uint32_t r = 0; r < TIPC_MAX_ADJ; ++r)
        if (cls == TIPC_REPAIR && h < gap && gap - 1u - h == r) { hp = hpos[r]; hh = hhead[r]; }
      a.tp_hop_pos[od * TIPC_MAX_ADJ + h] = hp; a.tp_hop_head[od * TIPC_MAX_ADJ + h] = hh;
    }
  }
  // counter 0: the population; 1 .. 6: the classes; 7 .. 11: the repairs by their number of adjacencies
  frr_cover<TIPC_COV>(cls ? 1u | (1u << cls) | (cls == TIPC_REPAIR ? 1u << (7u + gap) : 0u) : 0u, s_cov, a.tp_cov + (size_t)pi * TIPC_COV);
}

}  // namespace
