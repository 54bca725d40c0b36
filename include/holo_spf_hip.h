/*
 * holo_spf_hip.h — C ABI of libholo_spf_hip.so, the MI355X (gfx950) SPF engine.
 *
 * This is the drop-in boundary for the link-state SPF hot path of holo-routing/holo.
 * The reference has no FFI for this path; the boundary is drawn at
 * the two functions that do all shortest-path-tree work:
 *
 *   holo-ospf/src/spf.rs:587-729   run_area<V>()     one SPT per area, root = self
 *   holo-isis/src/spf.rs:527-709   compute_spt()     one SPT per (level, MT, arbitrary root)
 *   holo-isis/src/flooding/manet.rs:47-69            the batched-roots caller (one SPT per adjacency)
 *
 * What crosses the boundary is the *graph* those loops walk (CSR restatement of
 * `vertex_lsa_links` holo-ospf/src/ospfv2/spf.rs:389-460, ospfv3/spf.rs:348-419 and
 * `vertex_edges` holo-isis/src/spf.rs:1013-1128) and, per root, the per-vertex result the
 * loops produce (`Vertex{distance,hops,nexthops}` holo-ospf/src/spf.rs:38-46,
 * holo-isis/src/spf.rs:78-88).  Everything that needs Interface / Adjacency / LSA objects
 * (next-hop address resolution, prefix attachment) stays with the caller and consumes
 * dist / hops / first_hop_mask.  See INTEGRATION.md for the Rust-side binding.
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no C++ or torch types;
 *   - every entry point returns 0 (HSPF_OK) or a negative HSPF_E* code; nothing aborts or
 *     throws across the boundary (mirrors `Error::SpfRootNotFound(..).log(); return;`
 *     holo-ospf/src/spf.rs:605-610 — the caller logs and keeps its own loop as fallback);
 *   - a ctx is used by one thread at a time; distinct ctxs may run concurrently (one HIP
 *     stream each), matching the one-OS-thread-per-instance contract of
 *     holo-protocol/src/lib.rs:427-430;
 *   - there is NO CPU fallback inside the library: without a HIP device hspf_init fails.
 */
#ifndef HOLO_SPF_HIP_H
#define HOLO_SPF_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSPF_ABI_VERSION 8u   /* 8: hspf_stats + n_repaired_roots / repair_* (dynamic pop order resolved in parallel); HSPF_RF_EXACT = "the pop order is dynamic";
                                 7: + packed results (hspf_run_packed / _device / _async, hspf_wait_packed, hspf_packed_layout + decode helpers),
                                    hspf_host_alloc / hspf_host_free, hspf_device_alloc / _free / _to_host / hspf_host_to_device, hspf_rib_clear_device / hspf_rib_fold_device (several areas, one RIB, on the device), HSPF_E_NO_PACKED (additions only); the library no longer sets
                                    GPU_MAX_HW_QUEUES at load time;
                                 6: + hspf_run_device_async / hspf_wait / hspf_wait_all / hspf_async_lanes, hspf_multi_run_async / hspf_multi_run_wait, hspf_recommend_cpu (additions only);
                                 5: + hspf_routes_diff_count / hspf_routes_pack, hspf_multi_init_error, HSPF_PFX_RESIDENT, HSPF_GX_ELL_* / LEAF / SUMMARY */

/* ---- error codes ------------------------------------------------------------------- */
#define HSPF_OK                 0
#define HSPF_E_INVAL           -1   /* bad argument (NULL, out-of-range root, malformed CSR)   */
#define HSPF_E_NODEV           -2   /* no usable HIP device / device ordinal out of range     */
#define HSPF_E_HIP             -3   /* a HIP runtime call failed; see hspf_last_error(ctx)     */
#define HSPF_E_NOMEM           -4   /* host or device allocation failed                        */
#define HSPF_E_TOO_MANY_SLOTS  -5   /* a root has more first-hop slots than n_mask_words*64    */
#define HSPF_E_INTERNAL        -6   /* invariant violated (never expected)                     */
#define HSPF_E_NO_PACKED       -7   /* hspf_run_packed*: this run's results do not fit packed words
                                       (more than 24 first-hop slots, hop counts beyond the hop field);
                                       nothing was written, call hspf_run / hspf_run_device instead */

/* ---- vertex flags (hspf_csr.vflags) -------------------------------------------------- */
/* bit0: vertex is an OSPF network vertex / IS-IS pseudonode.  Reaching it does not
 *       increment `hops` (holo-ospf/src/spf.rs:675-678, holo-isis/src/spf.rs:650-653).      */
#define HSPF_VF_NETWORK    0x01u
/* bit1: IS-IS overload bit set for the topology of this run: the vertex stays in the SPT
 *       but its links are skipped unless it is the root (holo-isis/src/spf.rs:568-574).
 *       Routers only, as in the reference (`!vertex.id.is_pseudonode()`): ignored on a vertex
 *       that also has HSPF_VF_NETWORK.                                                          */
#define HSPF_VF_NO_TRANSIT 0x02u
/* bit2: never expanded, root included: zeroth LSP missing / seqno 0 / lifetime 0
 *       (holo-isis/src/spf.rs:558-561) or protocols-supported gate (:582-604).               */
#define HSPF_VF_NO_EXPAND  0x04u

/* ---- run flags (hspf_run*.run_flags) -------------------------------------------------- */
/* OSPF semantics for first hops: a network reached from a hops==0 parent gets its own
 * first-hop slot (holo-ospf/src/ospfv2/spf.rs:296-302).  Without it (IS-IS) a pseudonode
 * reached from a hops==0 parent gets no next hop (holo-isis/src/spf.rs:680-701).            */
#define HSPF_RUN_NET_NEXTHOPS     0x01u
/* IS-IS flooding-topology run (mt_id == None): overload bit is not applied
 * (holo-isis/src/spf.rs:566-574).                                                           */
#define HSPF_RUN_IGNORE_OVERLOAD  0x02u
/* Force the sequential exact kernel for every root (test hook).                             */
#define HSPF_RUN_FORCE_EXACT      0x04u
/* Also produce hspf_result.pop_rank.                                                        */
#define HSPF_RUN_POP_RANK         0x08u
/* Count the rows the fused fixed point evaluates (hspf_stats.rows_recomputed).  A diagnostic: the counting
 * instantiation of the kernel is a few per cent slower, the results are the same.                           */
#define HSPF_RUN_COUNT_ROWS       0x10u

/* ---- per-(root,vertex) result flags (hspf_result.vflags_out) --------------------------- */
#define HSPF_RF_IN_SPT   0x0001u    /* vertex was popped into the SPT                         */
#define HSPF_RF_EXACT    0x0002u    /* the root's pop order is NOT the static (distance, index) order (zero-cost links, saturation):
                                       rows from k_repair or the sequential kernel; ask for pop_rank when the order matters */

#define HSPF_DIST_INF    0xFFFFFFFFu /* dist of a vertex that is not in the SPT               */
#define HSPF_NO_ROOT     0xFFFFFFFFu /* padding entry in a roots[] array: produces an empty SPT */

typedef struct hspf_ctx   hspf_ctx;    /* one per protocol-instance thread: device, stream, scratch */
typedef struct hspf_graph hspf_graph;  /* device-resident graph of one LSDB generation              */

/*
 * The LSDB graph of one area (OSPF) or one level x topology (IS-IS), as forward CSR.
 *   - vertex index == rank in the reference's VertexId order, so that integer compare is
 *     the candidate-list tie-break (holo-ospf/src/ospfv2/spf.rs:41-45: networks before
 *     routers, then numeric; holo-isis/src/spf.rs:96-100: pseudonodes first, then the
 *     7-byte LAN id);
 *   - row u lists the links of u in LSA / LSP order exactly as the reference iterates them
 *     (incl. parallel links and the TLV2+TLV22 duplicates of metric-type "both"); links whose
 *     target LSA/LSP is absent are simply not listed;
 *   - the two-way connectivity check (holo-ospf/src/spf.rs:654-664,
 *     holo-isis/src/spf.rs:616-627) is applied by the library, not the caller;
 *   - arrays are caller-owned host memory, borrowed for the duration of the call only.
 */
typedef struct {
  uint32_t        n_vertices;       /* <= 2^24                                                */
  uint32_t        n_edges;
  const uint32_t *row_ptr;          /* [n_vertices+1], row_ptr[0]==0, non-decreasing          */
  const uint32_t *col;              /* [n_edges] target vertex index                          */
  const uint32_t *metric;           /* [n_edges] link cost (OSPF u16, IS-IS u8/u24, widened)  */
  const uint8_t  *vflags;           /* [n_vertices] HSPF_VF_*                                 */
  uint32_t        max_path_metric;  /* relaxations with dist > this are dropped: 0xFFFFFFFF
                                       for OSPF (saturating add, holo-ospf/src/spf.rs:672),
                                       1023 / 0xFE000000 for IS-IS (holo-isis/src/spf.rs:44-49,
                                       637-647)                                               */
} hspf_csr;

/*
 * Per-root results, row-major [n_roots][n_vertices].  With hspf_run() the pointers are
 * caller-owned HOST memory; with hspf_run_device() they are DEVICE (HBM) pointers and the
 * results never leave the GPU (for device-side consumers and the RCCL all-gather).
 * Any pointer may be NULL to skip that output (dist must not be NULL).
 *
 * first_hop_mask: bit k of word k/64 == first-hop slot k of that root is one of the vertex's
 * next hops.  Slots are numbered per root over the out-links of the vertices that can have
 * hops == 0:  H = [root] ++ (network vertices reachable from the root through network
 * vertices only, breadth-first, links in row order, each vertex once);
 * slot(p, j) = sum(deg(H[i]) for H[i] before p) + j   for the j-th link of row p
 * (positions count ALL links of the row as passed in hspf_csr).  hspf_slot_table() returns
 * H and the bases so the caller can map a slot back to (parent vertex, link) and call its
 * own `calc_nexthops` / `resolve_nexthop` on it.
 */
typedef struct {
  uint32_t *dist;            /* HSPF_DIST_INF when not in SPT                                 */
  uint16_t *hops;            /* holo `Vertex.hops` (first-discoverer rule)                    */
  uint16_t *vflags_out;      /* HSPF_RF_*                                                     */
  uint64_t *first_hop_mask;  /* [n_roots][n_vertices][n_mask_words]                           */
  uint32_t  n_mask_words;    /* capacity in u64 words per (root,vertex); >= hspf_mask_words() */
  uint32_t *pop_rank;        /* position in the reference's pop order (needs HSPF_RUN_POP_RANK),
                                0xFFFFFFFF when not in SPT                                     */
} hspf_result;

/* Timing / work counters of the last hspf_run*() on a ctx (HIP-event timed, on the ctx stream). */
typedef struct {
  uint32_t n_roots;
  uint32_t n_batches;          /* 64-root wavefront batches                                   */
  uint32_t n_relax_launches;   /* launches of the fused sweep / distance relaxation kernel    */
  uint32_t n_dag_launches;     /* launches of the SPT-DAG (hops / first-hop) kernel           */
  uint32_t n_exact_roots;      /* roots that needed the sequential exact kernel               */
  uint32_t n_mask_words;
  float    ms_total;           /* first launch -> results in place (device time)              */
  float    ms_relax;
  float    ms_dag;
  float    ms_finish;          /* transpose to row-major outputs (+ exact kernel)             */
  float    ms_d2h;             /* only for hspf_run(): device->host copies                    */
  uint32_t state_bytes;        /* per-(vertex,root) state of the fused path: 4 or 8; 0 = two-phase path */
  uint32_t narrow_overflow;    /* 1: the 4-byte state overflowed and the run was redone with 8 bytes   */
  uint64_t rows_recomputed;    /* HSPF_RUN_COUNT_ROWS: (vertex, 64-root batch) rows the fused fixed point evaluated, summed
                                  over its launches (0 without the flag); the reference settles each vertex once per root
                                  (holo-isis/src/spf.rs:552-556), i.e. n_batches * n_vertices rows would be 1x */
  uint32_t single_wg;          /* 1: small graph, the run took the one-workgroup-per-root kernel (one launch);
                                  2: one to eight roots on a mid-size graph, one XCD per root (k_xcd, one launch):
                                  dbg[1] then holds its sweeps (bits 0-15; bit 31: a workgroup ran on another XCD) */
  uint32_t lane_vertex;        /* 1: a few roots on a larger graph, the run took the lane = vertex kernel (k_lv)   */
  uint32_t dbg[4];             /* [0]: bit 0 = the run took the lean sweep (k_fused_lean), bit 1 = its instantiation for graphs with zero-cost rows
                                  (RF_ZERO rows, not hop-count-like); [1]: lean sweep: bits 0-7 = dense passes that did
                                  work, 8-15 = head sweeps that ran, 16-23 = dense passes planned, 24-30 = head sweeps planned
                                  (the plan is sized from the previous run, the launches decide on the device);
                                  bit 31 = a wide-mask run left the graph's leaves to the emit;
                                  [2], [3]: host microseconds from the entry of the (last) run to its first enqueue /
                                  to its return.  HSPF_RUN_COUNT_ROWS on the one-workgroup path instead: sweeps,
                                  shader cycles, 100 MHz wall ticks and set-up cycles of the first root's workgroup  */
  /* ABI 8: roots whose pop order is dynamic (zero-cost router links) — distances from the sweep kernels, hops and first-hop
     masks recomputed in the true pop order by k_repair, one workgroup per root (holo_amd/csrc/spf_repair.hip.h) */
  uint32_t n_repaired_roots;   /* roots k_repair put right (n_exact_roots counts only what still needed the sequential kernel) */
  uint32_t repair_sweeps;      /* worklist sweeps of the slowest of them                               */
  uint32_t repair_evals;       /* (root, vertex) evaluations in the true order, all of them together    */
  uint32_t repair_groups;      /* groups of vertices released by a higher-numbered one that were walked  */
  float    ms_repair;          /* host time of the repair step (enqueue to completion)                   */
} hspf_stats;

/* ---- lifecycle -------------------------------------------------------------------------- */
uint32_t    hspf_abi_version(void);
int         hspf_device_count(void);                       /* >=0, or HSPF_E_*                 */
int         hspf_init(int device_ordinal, hspf_ctx **out);
void        hspf_shutdown(hspf_ctx *ctx);
const char *hspf_strerror(int code);
const char *hspf_last_error(const hspf_ctx *ctx);          /* detail of the last failure       */
/* Where the GPU path pays (no GPU needed; pure arithmetic): 1 when the caller's own CPU loop is expected to finish
 * these runs sooner than the engine can, 0 otherwise.  One root on a small LSDB is the reference's everyday call
 * (run_area / compute_spt, one root per area / level: holo-ospf/src/spf.rs:540-542, holo-isis/src/spf.rs:746-761);
 * the engine's floor for any run is one launch + one stream synchronisation (measured wall on MI355X, one root on 4-neighbour
 * grids: 0.033 ms at 25-64 vertices, 0.036 at 100, 0.039 at 144-256, 0.046 at 400, 0.050 at 500: ~0.032 + 3.5e-5 n), the
 * reference-shaped loop (ordered map, linear candidate scan, per-edge two-way rescan) costs
 * ~(2.4e-4 n + 7e-7 n^2) ms per root on one host core (n = 100: 0.03, 196: 0.09, 484: 0.29 ms; tools/cpu_small_graph_table.py),
 * so: CPU iff n_roots * (2.4e-4 n + 7e-7 n^2) < 0.032 + 3.5e-5 n — one root below ~110 vertices, two below ~60, never from
 * 8 roots up.  n_edges is taken for callers whose links-per-router ratio is far from the grid-like 4-8 the table was measured on
 * (the per-root cost is scaled by max(1, n_edges / (8 n))).  INTEGRATION.md section 6 shows the call site. */
int hspf_recommend_cpu(uint32_t n_vertices, uint32_t n_edges, uint32_t n_roots);
/* Use an externally owned hipStream_t (e.g. torch's current stream) instead of the ctx's own. */
int         hspf_set_stream(hspf_ctx *ctx, void *hip_stream);
void       *hspf_get_stream(const hspf_ctx *ctx);

/* ---- graph ------------------------------------------------------------------------------ */
int      hspf_graph_upload(hspf_ctx *ctx, const hspf_csr *csr, hspf_graph **out);

/* The same from LSDB records (ABI 8; SURVEY.md §8f-1: "LSDB -> CSR extraction"): vertices by 64-bit KEY in any order, links as
 * (target key, cost) in LSA / LSP link order, targets unresolved.  Ascending key order must be the reference's VertexId order
 * (IS-IS: !pseudonode << 56 | the 7 LAN-id bytes, big-endian — holo-isis/src/spf.rs:96-100; OSPFv2: router << 32 | id —
 * holo-ospf/src/ospfv2/spf.rs:41-45).  The device ranks the keys, resolves every link's target, drops links whose target is
 * not a vertex of the LSDB (vertex_lsa_links / vertex_edges do not yield them) and builds the graph; what it built can be
 * read back with hspf_graph_export (ROW_PTR / COL / METRIC / VFLAGS: the caller's CSR as hspf_graph_upload would have got it).
 * rank_out (may be NULL): [n_vertices] index of input vertex i in the graph.  Duplicate keys: HSPF_E_INVAL. */
typedef struct {
  uint32_t n_vertices, n_links;
  const uint64_t *vertex_key;   /* [n_vertices]                                                   */
  const uint32_t *row_ptr;      /* [n_vertices+1] rows of the vertices in the order of vertex_key  */
  const uint64_t *target_key;   /* [n_links]                                                      */
  const uint32_t *metric;       /* [n_links]                                                      */
  const uint8_t  *vflags;       /* [n_vertices] HSPF_VF_*                                         */
  uint32_t max_path_metric;
} hspf_keyed_lsdb;
int      hspf_graph_upload_keyed(hspf_ctx *ctx, const hspf_keyed_lsdb *lsdb, hspf_graph **out, uint32_t *rank_out);
void     hspf_graph_free(hspf_ctx *ctx, hspf_graph *g);
uint32_t hspf_graph_n_vertices(const hspf_graph *g);
uint32_t hspf_graph_n_edges(const hspf_graph *g);          /* links of the caller's CSR (after patches) */
uint32_t hspf_graph_n_edges_kept(const hspf_graph *g);     /* links surviving the two-way check */

/*
 * Incremental update.  An LSP / LSA that is re-originated, purged or aged out changes
 * exactly the links OUT OF its own vertex and that vertex's gates — holo-isis keys a partial run by the
 * changed LSPs (`trigger_lsps`, holo-isis/src/spf.rs:144,735), holo-ospf by the changed LSAs
 * (`SpfTriggerLsa`, holo-ospf/src/spf.rs:120-139) — so the unit of change is "replace whole rows":
 * for each listed vertex the new row (links in LSA order, as in hspf_csr) and its new flags.  The vertex set
 * is fixed; a new or vanished vertex needs a fresh hspf_graph_upload.  After the call the graph is
 * indistinguishable from one uploaded from the patched CSR (two-way check, kept links and the whole device
 * layout are rebuilt on the device from the resident CSR; only the replaced rows cross the bus).
 * On HSPF_E_INVAL nothing has changed; after HSPF_E_HIP / HSPF_E_NOMEM the graph must be freed.
 */
typedef struct {
  uint32_t        n_changed;
  const uint32_t *vertex;     /* [n_changed]   strictly ascending vertex indices                   */
  const uint32_t *row_ptr;    /* [n_changed+1] bounds of the replacement rows inside col / metric  */
  const uint32_t *col;        /* [row_ptr[n_changed]]                                              */
  const uint32_t *metric;     /* [row_ptr[n_changed]]                                              */
  const uint8_t  *vflags;     /* [n_changed]   HSPF_VF_* of those vertices after the change        */
} hspf_rows;
int hspf_graph_patch(hspf_ctx *ctx, hspf_graph *g, const hspf_rows *rows);

/* Copies one array of the device-resident graph back to the host (inspection, tests, debugging).
 * dst == NULL: only *out_bytes is set.  The layout: kept links = two-way and source expandable; in-rows
 * (links INTO a vertex) ordered by (cost descending, source ascending, position in the source row
 * ascending), IN_SRC carries the source's HSPF_VF_NO_TRANSIT in bit 31 and whether it is a leaf (HSPF_GX_LEAF) in
 * bit 30; out-rows in the caller's order. */
#define HSPF_GX_ROW_PTR   0u   /* u32 [n+1]    caller's CSR as resident on the device             */
#define HSPF_GX_COL       1u   /* u32 [e]                                                         */
#define HSPF_GX_METRIC    2u   /* u32 [e]                                                         */
#define HSPF_GX_VFLAGS    3u   /* u8  [n]                                                         */
#define HSPF_GX_IN_PTR    4u   /* u32 [n+1]                                                       */
#define HSPF_GX_IN_SRC    5u   /* u32 [kept]                                                      */
#define HSPF_GX_IN_COST   6u   /* u32 [kept]                                                      */
#define HSPF_GX_IN_POS    7u   /* u32 [kept]   position of the link inside its source row         */
#define HSPF_GX_OUT_PTR   8u   /* u32 [n+1]                                                       */
#define HSPF_GX_OUT_DST   9u   /* u32 [kept]                                                      */
#define HSPF_GX_OUT_COST 10u   /* u32 [kept]                                                      */
#define HSPF_GX_OUT_POS  11u   /* u32 [kept]                                                      */
#define HSPF_GX_ROWFLAGS 12u   /* u8  [n]      internal per-row flags of the fused sweep          */
#define HSPF_GX_TWOWAY   13u   /* u8  [e]      1 = the target's row lists the source              */
#define HSPF_GX_UNITS    14u   /* u32 [...]    work units of the sweep kernels: empty when no 16-vertex chunk holds a row
                                  of more than 32 in-links; else [4 units per heavy chunk | 1 unit per other chunk],
                                  each class in vertex order, entry = first vertex (| 0x80000000: one row per wave) */
#define HSPF_GX_BUILD_MODE 15u /* u32 [1]      how the last upload / patch derived the layout: 0 = per-link row scans,
                                  1 = hub mode (a row of more than 512 links: two device-wide sorts, O(log degree) per
                                  link), 2 = the last patch changed costs only (same targets, order and flags in every
                                  replaced row): the affected rows were re-ranked in place, nothing was rebuilt;
                                  3 = the last patch was structural and only the affected rows (the replaced ones, their
                                  old and new targets) were re-derived, the compact arrays behind them shifted.  The
                                  layout itself does not depend on the mode                                          */
#define HSPF_GX_ELL_SRC  16u   /* u32 [16(n+1)] fixed-stride copy of the in-rows of at most 16 links: source << 8, the low
                                  byte of a row's first entry = in-degree (0x1F: more than 16) | more than 16 out-links
                                  << 5 | network << 7; unused entries name the pad row n                            */
#define HSPF_GX_ELL_COST 17u   /* u32 [16(n+1)] their costs (unused entries 0)                                       */
#define HSPF_GX_ELL_OUT  18u   /* u32 [16(n+1)] out-neighbour j << 2 (unused entries 0xFFFFFFFF)                     */
#define HSPF_GX_LEAF     20u   /* u8  [n]      1 = leaf: exactly one kept in-link, and the kept out-links (at most one) lead
                                  back to its source.  IN_SRC carries the source's leaf bit in bit 30                */
#define HSPF_GX_SUMMARY  19u   /* u32 [12]     what a build derives from the links and a patch must keep current:
                                  largest kept cost, hop-count shape (0/1), smallest-graph kernel allowed (0/1), OR of
                                  the row flags, rows with a zero-cost link from a higher-numbered source, rows off the
                                  hop-count shape, largest in-degree, kept links; of the caller's rows (a structural
                                  patch updates them from the replaced rows alone): longest row, network vertices,
                                  links in rows of more than 32, "a quarter of the links sit in such rows" (0/1)      */
#define HSPF_GX_HOST_ROW_PTR 21u /* u32 [n+1]  the HOST mirror of the caller's row bounds (slot tables are made from it; a
                                  structural patch splices it in place): equals ROW_PTR                              */
#define HSPF_GX_HOST_COL 22u   /* u32 [e]      ... and of the caller's targets: equals COL                           */
#define HSPF_GX_ZCYC     23u   /* u8  [n]      (ABI 8) 1 = the vertex may lie on a cycle of zero-cost kept links: what survives 8
                                  rounds of "keeps a zero-cost in-link from and a zero-cost out-link to a survivor".  0 bytes
                                  when no row has a zero-cost link from a higher- or equal-numbered source (array unused)  */
int hspf_graph_export(hspf_ctx *ctx, const hspf_graph *g, uint32_t which, void *dst, size_t cap_bytes,
                      size_t *out_bytes);

/* ---- first-hop slots -------------------------------------------------------------------- */
/* Number of u64 mask words needed for these roots on this graph (>= 1). */
int hspf_mask_words(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots,
                    uint32_t *out_words);
/* Slot table of one root: writes up to `cap` entries of H (vertex index) and its slot base;
 * returns the number of entries of H (may exceed cap), or HSPF_E_*. */
int hspf_slot_table(hspf_ctx *ctx, const hspf_graph *g, uint32_t root,
                    uint32_t *h_vertex, uint32_t *h_base, uint32_t cap, uint32_t *out_total_slots);

/* ---- run -------------------------------------------------------------------------------- */
/* Synchronous: on return the results are in the caller's host buffers. */
int hspf_run(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots,
             uint32_t run_flags, hspf_result *out);
/* Results are written to device buffers; returns after the work has been *enqueued and
 * completed* on the ctx stream (the call synchronises the stream once at the end so that
 * error flags can be read).  roots is a host array. */
int hspf_run_device(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots,
                    uint32_t run_flags, hspf_result *out_device);
int hspf_get_stats(const hspf_ctx *ctx, hspf_stats *out);

/* ---- failure scenarios: the SPT a root has AFTER a failure, one scenario per row ---------- */
/*
 * Row r is the run of roots[r] on the graph with fail[r] applied; the graph itself is not touched, so any number of
 * scenarios — every link of a router under link failure, every neighbour under node failure — are ONE batch of one run
 * ("lane = root": a scenario is a lane whose root happens to repeat).  This is the post-convergence tree: the yardstick of
 * the fast-reroute calls below (hspf_tilfa_device's "the best total is the SPF distance S -> E with the protected link
 * removed" is dist[E] of the HSPF_FAIL_ROOT_LINK row of that link) and the input of what they leave out of scope.
 *
 * Everything is as hspf_run_device defines it — distances, hop counts, HSPF_RF_*, the first-hop mask and its slot
 * numbering (positions count ALL links of the root's row as passed: no slot moves because a link failed), max_path_metric,
 * overload, HSPF_RUN_NET_NEXTHOPS, HSPF_RUN_IGNORE_OVERLOAD, n_mask_words as hspf_mask_words gives it for `roots` — except:
 *   HSPF_FAIL_NONE       nothing: the row equals hspf_run_device's row of that root.
 *   HSPF_FAIL_ROOT_LINK  arg = position j of a link in the ROOT's row of the caller's CSR: that link is not used in this row.
 *                        Only that direction matters for the root's own SPT (the root's distance is 0 and never improved);
 *                        parallel links to the same neighbour stay, and the two-way check of every other link is unaffected
 *                        (the neighbour still lists the root).  A link that did not survive the two-way check changes
 *                        nothing.  The slot bit of j is never set.  j >= the row's length: HSPF_E_INVAL.
 *   HSPF_FAIL_VERTEX     arg = a vertex X != root: X is not in this row's SPT (dist HSPF_DIST_INF, hops 0, flags 0, mask 0)
 *                        and no link out of X is used.  X may be a router or a network vertex (a LAN failure).  X == root
 *                        or X >= n: HSPF_E_INVAL.
 * roots[r] == HSPF_NO_ROOT gives an empty SPT as always; its failure is not looked at.  The same root may appear in any
 * number of rows.  Argument errors (also an unknown kind, HSPF_RUN_POP_RANK, HSPF_RUN_COUNT_ROWS) return HSPF_E_INVAL before
 * anything is launched — hspf_get_stats still shows the previous run — with a text in hspf_last_error that names the call.
 *
 * Engine path: scenario runs take ONE path, the two-phase fixed point (distances, then hops and masks over the tight-link
 * DAG) with the failure test on the rare side of its sweeps, whatever the number of slots; leaves take part in the fixed
 * point instead of being derived in the emit.  Roots whose pop order is dynamic under the failure (zero-cost plateaus) or
 * whose sums saturate u32 are redone by the sequential kernel with the same exclusion (HSPF_RF_EXACT in their rows): slow
 * and correct.  OUT OF SCOPE: packed words and the asynchronous / ticket forms; failures of links that are not the root's;
 * more than one failure per row.
 */
#define HSPF_FAIL_NONE      0u   /* the row is a plain run of its root                                   */
#define HSPF_FAIL_ROOT_LINK 1u   /* arg = position j of a link in the ROOT's row of the caller's CSR     */
#define HSPF_FAIL_VERTEX    2u   /* arg = a vertex index X != root                                        */
typedef struct {
  uint32_t kind;            /* HSPF_FAIL_*                                                 */
  uint32_t arg;             /* the link position or the vertex, as the kind says           */
} hspf_failure;
/* roots and fail are host arrays of n_rows entries; out_dev holds DEVICE pointers (n_rows rows), as for hspf_run_device. */
int hspf_run_failures_device(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, const hspf_failure *fail,
                             uint32_t n_rows, uint32_t run_flags, hspf_result *out_dev);
/* ... and with host buffers, as hspf_run. */
int hspf_run_failures(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, const hspf_failure *fail,
                      uint32_t n_rows, uint32_t run_flags, hspf_result *out_host);

/* ---- asynchronous runs (ABI 6) ----------------------------------------------------------- */
/*
 * The reference runs ONE SPF at a time per instance thread (holo-protocol/src/lib.rs:427-430), but an SPF event holds
 * several independent runs: one per area (holo-ospf/src/spf.rs:540-542), per level and topology
 * (holo-isis/src/spf.rs:746-761), per neighbour (holo-isis/src/flooding/manet.rs:59-69).  hspf_run_device_async
 * hands a run to one of the context's LANES — private engine contexts on the same device, each with its own stream,
 * scratch and host thread (HSPF_ASYNC_LANES, default 3) — and returns a ticket at once; hspf_wait blocks until that run
 * is over and returns its code (and statistics).  Lanes are taken in ticket order (ticket % lanes), each runs its tickets
 * one after the other from a short queue: the call blocks only while three tickets of that lane are already waiting.  The roots are copied; `out_device` buffers must stay
 * valid, and must not be shared between runs in flight, until the ticket has been waited for.  A run alone leaves most
 * of the chip idle during its sparse first and last sweeps (chains of small dependent launches); runs in flight on
 * several lanes move in lockstep and interleave those chains (isis-100k, 64-root runs: 150 k runs/s with three in flight
 * against 124 k one after the other).  Results are bit-identical to hspf_run_device's.  hspf_graph_patch /
 * hspf_graph_free on the context wait for its runs in flight first; results of a ticket are kept until eight later runs
 * of its lane have finished.  Same threading contract as every other call: one caller thread per context.
 * The lanes are also where a SYNCHRONOUS run of more than 64 roots goes when its roots fall into different state classes
 * (a few roots with many first-hop slots among many with few: each class is a run of its own): all classes but one are
 * handed to lanes and run side by side (fat-tree k=100, 51 switch roots + 50 host roots: 1.69 ms instead of 2.01).  The
 * lanes are created by the first call that needs them (~15 ms once per context).  In the same calls a LEAF root — a router
 * whose only two-way link leads to a router that is a root of the same call — is not run at all: its rows are its
 * neighbour's, one link further (distance + link cost up to the max-path metric, hops + 1, its one first-hop slot).
 */
int hspf_run_device_async(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots,
                          uint32_t run_flags, const hspf_result *out_device, uint64_t *ticket);
int hspf_wait(hspf_ctx *ctx, uint64_t ticket, hspf_stats *stats /* may be NULL */);
int hspf_wait_all(hspf_ctx *ctx);                  /* every run in flight is over (codes: hspf_wait)        */
uint32_t hspf_async_lanes(const hspf_ctx *ctx);    /* how many runs can be in flight                        */

/* ---- packed results (ABI 7) ---------------------------------------------------------------- */
/*
 * hspf_run delivers 16 bytes per (root, vertex) — 102 MB for 64 roots on a 100 000-vertex level, 1.8 ms over PCIe against
 * 0.45 ms of compute — although the engine holds the whole answer in ONE machine word per (root, vertex):
 * [distance | hop count | first-hop mask], 4 bytes when the fields fit (the usual case: checked on the device, never
 * assumed), else 8.  hspf_run_packed hands exactly those words over, row-major [n_roots][n_vertices], together with the
 * field positions of THIS run; the caller (whose next step looks at a vertex once: rebuilding `Vertex{distance, hops,
 * nexthops}`, holo-isis/src/spf.rs:78-88, holo-ospf/src/spf.rs:38-46) decodes a word where it needs it:
 *     in SPT     word <  not_reached                        (else: dist = HSPF_DIST_INF, hops = 0, mask = 0)
 *     distance   word >> dist_shift
 *     hops       (word >> hops_shift) & hops_mask
 *     mask       word & ((1 << mask_bits) - 1)              first-hop slots 0 .. mask_bits - 1, as hspf_result.first_hop_mask
 * (inline helpers below).  The values are bit for bit those of hspf_run.  What has no room in a word comes per root:
 * root_status[r] & HSPF_ROOT_EXACT = the root went through the sequential kernel (HSPF_RF_EXACT of hspf_run: its pop
 * order is not the static (distance, index) order; ask for pop_rank with hspf_run when the caller needs that order).
 * HSPF_RUN_POP_RANK is not accepted.  A run whose roots have more than 24 first-hop slots, or whose hop counts outgrow
 * the field, returns HSPF_E_NO_PACKED before / without writing anything: the caller then calls hspf_run.
 *
 * `words` must have room for 8 bytes per (root, vertex) — cap_bytes >= 8 * n_roots * n_vertices always suffices; only
 * layout->word_bytes * n_roots * n_vertices bytes are written (and cross the bus).  Host destinations: memory from
 * hspf_host_alloc (page-locked: the copy runs at bus speed) or any other host memory (the library then stages the copy
 * through its own page-locked blocks, chunk by chunk, at the speed of one host memcpy).
 */
typedef struct {
  uint32_t word_bytes;     /* 4 or 8                                                              */
  uint32_t dist_shift;
  uint32_t hops_shift;
  uint32_t hops_mask;
  uint32_t mask_bits;
  uint32_t reserved;       /* 0                                                                   */
  uint64_t not_reached;    /* word >= not_reached: the vertex is not in the SPT of that root      */
} hspf_packed_layout;
#define HSPF_ROOT_EXACT 0x01u

static inline uint64_t hspf_packed_word(const hspf_packed_layout *l, const void *words, size_t index) {
  return l->word_bytes == 4u ? (uint64_t)((const uint32_t *)words)[index] : ((const uint64_t *)words)[index];
}
static inline int      hspf_packed_in_spt(const hspf_packed_layout *l, uint64_t w) { return w < l->not_reached; }
static inline uint32_t hspf_packed_dist(const hspf_packed_layout *l, uint64_t w) { return w < l->not_reached ? (uint32_t)(w >> l->dist_shift) : HSPF_DIST_INF; }
static inline uint16_t hspf_packed_hops(const hspf_packed_layout *l, uint64_t w) { return w < l->not_reached ? (uint16_t)((w >> l->hops_shift) & l->hops_mask) : (uint16_t)0; }
static inline uint64_t hspf_packed_mask(const hspf_packed_layout *l, uint64_t w) { return w < l->not_reached ? (w & ((1ull << l->mask_bits) - 1ull)) : 0ull; }

/* Page-locked host memory for result buffers (hipHostMalloc / hipHostFree behind the boundary, so that the Rust side
 * needs no HIP binding of its own).  Valid on every context of the process. */
int  hspf_host_alloc(hspf_ctx *ctx, size_t bytes, void **out);
void hspf_host_free(hspf_ctx *ctx, void *p);

/* Device memory for callers that keep tables in HBM (hspf_run_device -> hspf_routes_device -> hspf_routes_diff_device)
 * without a HIP binding of their own (the Rust wrapper): hipMalloc / hipFree / a synchronous device-to-host copy on the
 * context's device. */
int  hspf_device_alloc(hspf_ctx *ctx, size_t bytes, void **out);
void hspf_device_free(hspf_ctx *ctx, void *p);
int  hspf_device_to_host(hspf_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int  hspf_host_to_device(hspf_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);

/* Synchronous, words in HOST memory (see above).  root_status: [n_roots] or NULL. */
int hspf_run_packed(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots, uint32_t run_flags,
                    void *words_host, size_t cap_bytes, hspf_packed_layout *layout, uint8_t *root_status);
/* The same with `words_dev` in DEVICE memory (a quarter of the bytes of hspf_run_device's tables for consumers that stay
 * on the GPU or send the rows on with hspf_multi_allgather_rows); root_status is a HOST array. */
int hspf_run_packed_device(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots, uint32_t run_flags,
                           void *words_dev, size_t cap_bytes, hspf_packed_layout *layout, uint8_t *root_status);
/* Asynchronous form of hspf_run_packed on the context's lanes (hspf_run_device_async): the run AND its copy to the host
 * belong to the ticket, so the copy of one batch crosses the bus while the next batch computes.  words_host /
 * root_status must stay valid, and must not be shared between tickets in flight, until hspf_wait_packed has returned
 * for the ticket; that call also fills `layout`.  hspf_wait works on such a ticket too (without the layout). */
int hspf_run_packed_async(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots, uint32_t run_flags,
                          void *words_host, size_t cap_bytes, uint8_t *root_status, uint64_t *ticket);
int hspf_wait_packed(hspf_ctx *ctx, uint64_t ticket, hspf_packed_layout *layout, hspf_stats *stats /* may be NULL */);

/* ---- route derivation on device (the step right after the SPT) ------------------- */
/*
 * Prefix attachment of holo-isis compute_routes (holo-isis/src/spf.rs:864-918) for every root of a
 * previous hspf_run_device(): for each IP prefix, over the vertices that advertise it (iterated in
 * VertexId order, i.e. ascending vertex index), route metric = dist[v] + prefix metric; the smallest
 * wins (`Ordering::Less` replaces the route, :902-905), equal metrics merge their next hops
 * (`merge_nexthops`, :906-909).  What needs addresses — building Nexthop objects, the max-paths
 * truncation by address order (:920-929) — stays with the caller and consumes best_metric /
 * best_entry / nexthop_mask.
 *
 * The prefix table is CSR by prefix: entries pfx_ptr[p] .. pfx_ptr[p+1] are the (vertex, metric)
 * advertisements of prefix p, sorted by vertex index.  All result / input table pointers are DEVICE
 * pointers; pfx_* are caller-owned HOST arrays (uploaded per call).
 *
 * holo-ospf's update_rib_intra_area (holo-ospf/src/route.rs:343-448) is the same reduction with two twists,
 * selected by `flags`:
 *   HSPF_PFX_SATURATING   route metric = dist[v].saturating_add(metric)  (route.rs:362-366); the reached / not
 *                         reached distinction is then carried by best_entry alone (0xFFFFFFFF = no route).
 *   HSPF_PFX_LAST_MIN     the transit-network rule (route.rs:388-400): among equal metrics the LATER entry —
 *                         the larger LS-ID, entries being in ascending vertex = LS-ID order — REPLACES the
 *                         route instead of merging into it: best_entry = last entry attaining the minimum,
 *                         nexthop_mask = that entry's mask only.
 * An OSPF caller evaluates one table of Network-LSA prefixes with both flags and one table of Router-LSA stub
 * prefixes with HSPF_PFX_SATURATING, and folds the two per-prefix results in that order (networks sort before
 * routers in VertexId order): holo_amd/routes.py ospf_intra_area_device_routes.
 */
#define HSPF_PFX_SATURATING 0x1u
#define HSPF_PFX_LAST_MIN   0x2u
/*
 *   HSPF_PFX_ORDERED      the literal, ORDER-DEPENDENT fold of update_rib_intra_area (route.rs:343-448) for tables
 *                         whose entries do not come in vertex order: OSPFv3 reads its stub networks off the
 *                         Intra-Area-Prefix-LSAs in LSDB order (holo-ospf/src/ospfv3/spf.rs:421-478), router and
 *                         network vertices interleaved.  The entries of a prefix are listed in the reference's
 *                         iteration order; bit 31 of pfx_vertex (HSPF_PFX_ENTRY_NETWORK) marks an entry whose vertex
 *                         is a network, pfx_origin[e] is the Link State ID of that vertex's LSA (`stub.vertex.lsa
 *                         .origin().lsa_id`); metrics add saturating.  Per entry, as the reference: worse than the
 *                         route so far -> skipped (:371-375); a network entry meeting a route replaces it when shorter
 *                         or equal with a GREATER origin and is skipped otherwise (:388-400); then route_update
 *                         (:918-965): better replaces, equal merges the next hops.  init_* (optional, [n_prefixes],
 *                         the same for every root): the route an earlier area left in the RIB for that prefix
 *                         (the RIB is shared by the areas, route.rs:146-160) — init_exists[p] != 0, its metric and
 *                         origin; best_entry == HSPF_PFX_KEPT_INIT then says that this route still owns the prefix
 *                         and nexthop_mask holds what the table's entries merged INTO it.
 */
#define HSPF_PFX_ORDERED    0x4u
/*
 *   HSPF_PFX_RESIDENT     the caller's word that pfx_ptr / pfx_vertex / pfx_metric are exactly what its previous
 *                         hspf_routes_device call on this context passed (same pointers, same sizes, contents
 *                         untouched since — a prefix table changes with the LSDB, not with every SPF run): the range
 *                         checks and the host-to-device copies are skipped.  A table that does not match what was
 *                         recorded then (or an ordered one) is uploaded as usual.
 */
#define HSPF_PFX_RESIDENT   0x8u
#define HSPF_PFX_ENTRY_NETWORK 0x80000000u
#define HSPF_PFX_KEPT_INIT  0xFFFFFFFEu
typedef struct {
  uint32_t        n_prefixes;
  uint32_t        n_entries;
  const uint32_t *pfx_ptr;      /* [n_prefixes+1]                                                */
  const uint32_t *pfx_vertex;   /* [n_entries] advertising vertex (| HSPF_PFX_ENTRY_NETWORK with HSPF_PFX_ORDERED) */
  const uint32_t *pfx_metric;   /* [n_entries] advertised metric                                 */
  uint32_t        flags;        /* HSPF_PFX_*; 0 = the IS-IS rule                                */
  /* HSPF_PFX_ORDERED only (ABI 4; NULL otherwise): */
  const uint32_t *pfx_origin;   /* [n_entries]  Link State ID of the entry's vertex LSA          */
  const uint8_t  *init_exists;  /* [n_prefixes] or NULL                                          */
  const uint32_t *init_metric;  /* [n_prefixes] or NULL                                          */
  const uint32_t *init_origin;  /* [n_prefixes] or NULL                                          */
} hspf_prefix_table;

typedef struct {
  uint32_t *best_metric;        /* [n_roots][n_prefixes]  HSPF_DIST_INF: no advertising vertex in the SPT */
  uint32_t *best_entry;         /* [n_roots][n_prefixes]  index of the FIRST entry attaining it (route
                                   attributes — level, external flag, CONNECTED — come from that vertex,
                                   holo-isis/src/route.rs:79-107); 0xFFFFFFFF when unreachable    */
  uint64_t *nexthop_mask;       /* [n_roots][n_prefixes][n_mask_words] union of the first-hop masks of
                                   every entry attaining it                                        */
} hspf_routes;

int hspf_routes_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_roots, uint32_t n_mask_words,
                       const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                       const hspf_prefix_table *table, hspf_routes *out_dev);

/* ---- several areas, ONE RIB: the fold on device (ABI 7) ---------------------------------------
 * An OSPF instance computes one SPT per area and folds the areas' stub networks into ONE routing table, area after area
 * (the per-area loop holo-ospf/src/spf.rs:540-542; `update_rib_intra_area`, holo-ospf/src/route.rs:343-448, works on the
 * RIB the earlier areas left: better replaces, equal merges, the transit-network rule on the larger LS-ID).  hspf_rib_device
 * is that table on the device, over the INSTANCE-wide prefix list and an instance-wide first-hop slot numbering (area a's
 * slots start at mask word `word_offset` of its fold call: word-aligned, so placing an area's mask is a word copy);
 * hspf_rib_fold_device runs the literal ordered fold (HSPF_PFX_ORDERED) of ONE area's table with the state the earlier
 * areas left as its initial state and writes the new state back — nothing crosses the bus between areas.  After the last
 * area (best_metric, best_entry, nexthop_mask) IS an hspf_routes of one root over n_prefixes prefixes and n_mask_words
 * words: hspf_routes_diff_device / hspf_routes_pack compare it with the tables of the previous SPF event as for one area.
 *   best_entry   0xFFFFFFFF: no route; else area_index << 24 | entry index in that area's table (the route's owner:
 *                attributes that need LSA objects come from it on the host)
 *   origin       LS-ID of the owner's vertex LSA (the transit-network rule of the NEXT area's fold needs it)
 * All hspf_rib_device pointers are DEVICE pointers; `table` and `prefix_map` (area prefix -> instance prefix index, every
 * index at most once) are caller-owned HOST arrays.  table->flags must carry HSPF_PFX_ORDERED; init_* are ignored. */
typedef struct {
  uint32_t  n_prefixes;
  uint32_t  n_mask_words;
  uint32_t *best_metric;     /* [n_prefixes] */
  uint32_t *best_entry;      /* [n_prefixes] */
  uint64_t *nexthop_mask;    /* [n_prefixes][n_mask_words] */
  uint32_t *origin;          /* [n_prefixes] */
} hspf_rib_device;
int hspf_rib_clear_device(hspf_ctx *ctx, const hspf_rib_device *rib);           /* the empty RIB in front of the first area */
int hspf_rib_fold_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t area_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,   /* one root's rows of the area's run */
                         const hspf_prefix_table *table, const uint32_t *prefix_map,
                         uint32_t area_index, uint32_t word_offset, const hspf_rib_device *rib);

/* ---- RIB diff on device (the first half of the wire step after the path) -------------------------
 * update_global_rib (holo-isis/src/route.rs:254-312, holo-ospf/src/route.rs:856-916) walks the new RIB, skips every route
 * whose metric and next hops are what the old RIB held, sends a RouteIpAdd for the rest and a RouteIpDel for what
 * vanished — per-route host work and messages that dominate once an LSDB carries 100 k+ prefixes.  On
 * the tables hspf_routes_device() writes, that comparison is "same best_metric and same nexthop_mask": this call does it
 * for every (root, prefix) of two such result sets in HBM and compacts the indices that need a message.
 * PRECONDITION (the caller's): both sets index the same prefix list, and a first-hop slot means the same next hop in both
 * runs (the rows of the root and of its hops-0 networks did not change) — otherwise compare on the host.
 *   action[r][p]   HSPF_DIFF_SAME      nothing to send (:268-277)
 *                  HSPF_DIFF_INSTALL   new or changed, and the new route has next hops: RouteIpAdd (:283-295)
 *                  HSPF_DIFF_WITHDRAW  the old route had next hops (was installed) and the prefix has no route any
 *                                      more: RouteIpDel (:303-310)
 *                  HSPF_DIFF_SILENT    changed, but nothing goes on the wire (a route without next hops: CONNECTED, or
 *                                      unresolved next hops)
 *   changed / changed_ptr   per root r the prefix indices with INSTALL or WITHDRAW, ascending (the reference's emission
 *                  order is the prefix order): changed[changed_ptr[r] .. changed_ptr[r+1]); changed has room for
 *                  n_roots * n_prefixes entries.  All pointers are DEVICE pointers.
 */
#define HSPF_DIFF_SAME     0u
#define HSPF_DIFF_INSTALL  1u
#define HSPF_DIFF_WITHDRAW 2u
#define HSPF_DIFF_SILENT   3u
int hspf_routes_diff_device(hspf_ctx *ctx, uint32_t n_roots, uint32_t n_prefixes, uint32_t n_mask_words,
                            const hspf_routes *old_dev, const hspf_routes *new_dev,
                            uint8_t *action_dev, uint32_t *changed_dev, uint32_t *changed_ptr_dev);

/* ---- the hand-off of the diff (second quarter) ----------------------------------------------------
 * route_install sends ONE message per route (holo-isis/src/ibus/tx.rs:35-110, holo-ospf/src/ibus/tx.rs:32-77 ->
 * holo-routing/src/rib.rs:92-135).  hspf_routes_pack turns the changed list of the last hspf_routes_diff_device into ONE
 * contiguous record stream in the reference's emission order and brings it to the host with ONE copy: what a single
 * batched RouteIpAdd / RouteIpDel message carries.  Record k (HSPF_ROUTE_REC_WORDS + 2 * n_mask_words u32 words):
 *     [0] root index   [1] prefix index   [2] action (HSPF_DIFF_INSTALL | HSPF_DIFF_WITHDRAW)   [3] metric of the NEW route
 *     [4] best_entry of the new route (0xFFFFFFFF: the prefix has no route any more)   [5] 0
 *     [6 ..] the new route's next-hop mask words, low half first
 * roots ascending, prefixes ascending inside a root.  The caller expands a record into its message: prefix text from its
 * own prefix list, next hops = the resolved first-hop slots of the mask (holo_amd.routes.expand_route_records is the twin
 * that reproduces the reference's recorded RouteIpAdd / RouteIpDel sequence from it).
 * hspf_routes_diff_count: number of records the last hspf_routes_diff_device left (it came back with that call's own
 * synchronisation), i.e. n_records and the size of records_host. */
#define HSPF_ROUTE_REC_WORDS 6u
uint32_t hspf_routes_diff_count(const hspf_ctx *ctx);
int hspf_routes_pack(hspf_ctx *ctx, uint32_t n_roots, uint32_t n_prefixes, uint32_t n_mask_words, const hspf_routes *new_dev,
                     const uint8_t *action_dev, const uint32_t *changed_dev, const uint32_t *changed_ptr_dev,
                     uint32_t n_records, uint32_t *records_host);

/* ---- the route event stream: old -> new pairs, SILENT changes included, one device call (same ABI: a new symbol) -------
 * hspf_routes_diff_device + hspf_routes_pack hand over the pairs that need a MESSAGE.  A caller that keeps its own RIB
 * needs more: what every changed route WAS (to withdraw or replace it) and the changes that put nothing on the wire
 * (HSPF_DIFF_SILENT: a route that turns into one without next hops, or one that had none and vanishes).
 * hspf_routes_events compares two table sets of hspf_routes_device (same PRECONDITION as hspf_routes_diff_device, same
 * action rule — one device function computes both) and brings every pair whose action is not HSPF_DIFF_SAME to the host as
 * ONE stream of paired records.  Record k, HSPF_EVENT_REC_WORDS + 4 * n_mask_words u32 words:
 *     [0] root index   [1] prefix index   [2] action (HSPF_DIFF_INSTALL | HSPF_DIFF_WITHDRAW | HSPF_DIFF_SILENT)
 *     [3] NEW best_metric   [4] NEW best_entry (0xFFFFFFFF: no route now)
 *     [5] OLD best_metric   [6] OLD best_entry (0xFFFFFFFF: no route before)   [7] 0
 *     [8 ..)                       NEW nexthop_mask words, low half first (2 * n_mask_words words)
 *     [8 + 2 * n_mask_words ..)    OLD nexthop_mask words, low half first
 * roots ascending, prefixes ascending inside a root (the reference's emission order).  Applying the new half of every
 * record of a HSPF_EV_SILENT stream to a copy of the old tables gives the new tables (holo_amd.routes.apply_route_events).
 *   flags            HSPF_EV_SILENT: SILENT pairs are part of the stream; without it INSTALL / WITHDRAW pairs only.
 *   *n_records       always the TOTAL number of events.  min(total, capacity_records) records are written to records_host
 *                    (what lies behind them in records_host is unspecified); a total above the capacity is not an error:
 *                    hspf_routes_events_rest(first, count) copies any range [first, first + count) of the same stream — no
 *                    second comparison, no lost event — until the next route call on the context (hspf_routes_device,
 *                    hspf_rib_fold_device, hspf_routes_diff_device, hspf_routes_pack, hspf_routes_events: each voids the
 *                    stream, a later _rest is HSPF_E_INVAL) and as long as neither table set was written to (a tail the
 *                    staging did not hold is written from the tables).  A range beyond the total is HSPF_E_INVAL.
 *                    capacity_records == 0 with records_host == NULL asks for the count alone.
 * Cost and staging policy: three kernels (classify + count per 1024-pair tile, one scan over the tile totals, the write
 * pass) and, in the steady state, ONE synchronisation and ONE device-to-host copy: the total comes back in a pinned word
 * the scan kernel stores itself, and the copy is issued BEFORE the total is known, for as many records as the SMALLER of the
 * last two calls on this context produced plus a quarter (at least 1024), within capacity_records — the smaller, so that the
 * call after one cold start does not copy megabytes for a handful of events, while streams that are large call after call
 * still arrive in one copy.  The device staging is sized the same
 * way — from what earlier calls needed, never for n_roots * n_prefixes records — and only grows; the write pass clips at its
 * capacity.  A call that produces more than predicted pays for it once: the staging grows to the whole stream, the write
 * pass alone runs again (the action bytes and ranks are kept), and a second copy fetches the tail.
 * The ONE synchronisation / ONE copy holds for a PAGE-LOCKED records_host (hspf_host_alloc): pageable memory is filled
 * through the context's two page-locked staging blocks, one event wait per 8 MB block, at the speed of a host memcpy.  The
 * early copy always moves the predicted number of records (48 KB at least with one mask word), also when fewer events exist:
 * what lies in records_host behind the stream is stale staging content.  n_mask_words is at most 2^20.
 * All table pointers are DEVICE pointers; argument errors are HSPF_E_INVAL with a text in hspf_last_error. */
#define HSPF_EV_SILENT       0x1u
#define HSPF_EVENT_REC_WORDS 8u
int hspf_routes_events(hspf_ctx *ctx, uint32_t n_roots, uint32_t n_prefixes, uint32_t n_mask_words,
                       const hspf_routes *old_dev, const hspf_routes *new_dev, uint32_t flags,
                       uint32_t capacity_records, uint32_t *records_host, uint32_t *n_records);
int hspf_routes_events_rest(hspf_ctx *ctx, uint32_t first, uint32_t count, uint32_t *records_host);

/* ---- ancestor sets on device (the queries of flooding::manet::reflood_list) ------------------------
 * For every root of a previous hspf_run_device() and a level L (1 = first hops / remote-neighbour list, 2 = second
 * hops): the root's level-L routers = router vertices of its SPT with hops == L, numbered in ascending vertex index
 * (level_rank, 0xFFFFFFFF elsewhere; level_count = how many), and anc[root][v] = the n_words x 64 bit set of the level-L
 * routers that are ancestors of v in the SPT's parent DAG, or v itself — holo-isis Spt::is_on_path(a, d)
 * (holo-isis/src/spf.rs:261-286) for a level-L router a is then bit level_rank[a] of anc[root][d].
 * roots / run_flags: as passed to the run.  dist / hops / flags / level_rank / level_count / anc are DEVICE pointers
 * ([n_roots][n_vertices] row-major, anc with n_words words per entry; level_rank may be NULL).
 * A root that needed the sequential exact kernel (dynamic pop order) gets level_count 0xFFFFFFFF and no sets: the
 * caller keeps its own walk for it.  Returns HSPF_E_TOO_MANY_SLOTS when a root has more than 64 x n_words level-L
 * routers (level_count is filled in either way: call again with enough words). */
int hspf_ancestors_device(hspf_ctx *ctx, const hspf_graph *g, const uint32_t *roots, uint32_t n_roots, uint32_t run_flags,
                          const uint32_t *dist_dev, const uint16_t *hops_dev, const uint16_t *flags_dev,
                          uint32_t level, uint32_t n_words, uint32_t *level_rank_dev, uint32_t *level_count_dev,
                          uint64_t *anc_dev);

/* ---- loop-free alternates on device (RFC 5286) from neighbour SPTs: new symbols, same ABI number -----------------------
 * The consumer the many-roots batch was built for: a run of [S] ++ (S's neighbour routers) leaves their SPTs in HBM as
 * rows of one table set, and the backup next hops of S are inequalities over those rows.  hspf_lfa_device evaluates them
 * per (protected root, destination) where the tables are; hspf_lfa_candidates (host arithmetic, no context) says which
 * first-hop slots of S are candidates at all.  The reference ships only the YANG for this (ietf-isis fast-reroute/lfa,
 * frr-protection-available-{link,node,downstream}-type), no code.
 *
 * Terms.  S = a protected root; its SPT is row `root_row` of a table set [n_rows][n_vertices] (dist, vflags_out,
 * first_hop_mask with W = n_mask_words words) exactly as hspf_run_device wrote it.  A slot k of S is a first-hop slot as
 * defined above (hspf_result / hspf_slot_table): slot(p, j) = link j of H-vertex p.  Per slot k the candidate table holds
 *   nbr[k]        the ROUTER the slot's link leads to, or HSPF_NO_ROOT when the slot is no candidate: its target is a network
 *                 vertex, or S itself, or the link fails the two-way check;
 *   nbr_row[k]    the table row that holds the SPT rooted at nbr[k] (the caller's: it made the run);
 *   cost[k]       sum of the link costs along the path the slot stands for, S -> (network vertices) -> target (saturating u32):
 *                 the path by which H reached p (its breadth-first discovery links) plus link j;
 *   root_link[k]  position in S's OWN row of the link that starts that path (p == S: j itself);
 *   cflags[k]     HSPF_LFA_C_NO_TRANSIT when the neighbour carries HSPF_VF_NO_TRANSIT.
 * cost and root_link are filled for EVERY slot (a primary slot need not be a candidate), nbr / cflags for candidates.
 *
 * For a destination D in S's SPT, D != S:  P = the primary slots = the bits of mask_S[D]; d(X, Y) = dist in the row rooted
 * at X.  All sums are evaluated in 64 bits (max_path_metric may be 0xFE000000: two terms overflow u32); a term that is
 * HSPF_DIST_INF makes its inequality false.  Candidate k with N = nbr[k] belongs to
 *   cand        (loop-free and link-protecting) iff  d(N, D) < d(N, S) + d(S, D),  and root_link[k] != root_link[p] for every p
 *               in P,  and k is not in P,  and (cflags[k] has no NO_TRANSIT, or N == D, or the call passes HSPF_LFA_IGNORE_OVERLOAD);
 *   node        (node-protecting) iff k is in cand, P has at least one slot whose nbr[p] is a router, and for every such p with
 *               E = nbr[p]:  d(N, D) < d(N, E) + d(E, D)   (a primary slot whose target is not a router protects no node;
 *               E == D makes the inequality false by itself);
 *   downstream  iff  d(N, D) < d(S, D).
 * Outputs per (S, D):
 *   alt_flags   HSPF_LFA_HAS_PRIMARY   P is not empty
 *               HSPF_LFA_ECMP          popcount(P) >= 2: no alternate is chosen by THIS call (per primary: hspf_lfa_ecmp_device,
 *                                      below); the two sets are still written
 *               HSPF_LFA_LINK_PROTECT  an alternate was chosen (alt_slot is a member of cand)
 *               HSPF_LFA_NODE_PROTECT  ... and it is a member of node
 *               HSPF_LFA_DOWNSTREAM    ... and it is a downstream neighbour
 *   alt_slot    HSPF_LFA_NO_SLOT for none.  Chosen only when popcount(P) == 1: a member of node before a member of cand only,
 *               then the smallest cost[k] + d(N, D) (64 bits), then the smallest slot index
 *   alt_metric  that sum, saturated at 0xFFFFFFFE (0 when there is no alternate)
 *   cand_mask / node_mask   u64[W] per (S, D), bit k = slot k (optional: NULL skips the table)
 * For D == S, or D not in S's SPT, every output is zero and alt_slot is HSPF_LFA_NO_SLOT.
 * coverage[5] per protected root, counted on the device: destinations with a primary | ECMP destinations | destinations with
 * an alternate | with a node-protecting alternate | with a downstream alternate (the five alt_flags bits, in that order).
 *
 * LAN pseudonodes are handled through root_link ALONE: a candidate reached over the same first link of S as a primary is never
 * offered.  Loop-freeness with respect to the pseudonode itself (RFC 5286 section 3.3) is not checked by THIS call: a candidate on
 * another link whose own shortest path to D crosses the primary's LAN is still offered as link-protecting.  hspf_lfa_lan_device
 * ("broadcast-link protection", below) adds that check.  Shared-risk link groups: hspf_lfa_srlg_device ("SRLG-safe alternates and
 * remote-LFA spaces", below). */
#define HSPF_LFA_C_NO_TRANSIT    0x01u   /* hspf_lfa_protect.cflags */
#define HSPF_LFA_IGNORE_OVERLOAD 0x01u   /* hspf_lfa_device lfa_flags */
#define HSPF_LFA_HAS_PRIMARY     0x01u   /* alt_flags */
#define HSPF_LFA_ECMP            0x02u
#define HSPF_LFA_LINK_PROTECT    0x04u
#define HSPF_LFA_NODE_PROTECT    0x08u
#define HSPF_LFA_DOWNSTREAM      0x10u
#define HSPF_LFA_NO_SLOT         0xFFFFFFFFu
#define HSPF_LFA_COVERAGE_WORDS  5u
/* Candidate table of one root from the caller's CSR: pure host arithmetic (no context, no device, like hspf_recommend_cpu).
 * Restates the slot numbering of hspf_slot_table and applies the two-way check to the rows it touches (S's and those of the
 * network vertices of H, and one scan of each target's row).  Writes up to `cap` entries of each array (any may be NULL);
 * returns the number of slots (may exceed cap; also in *out_total_slots when not NULL), or HSPF_E_INVAL. */
int hspf_lfa_candidates(const hspf_csr *csr, uint32_t root, uint32_t cap, uint32_t *nbr, uint32_t *cost, uint32_t *root_link,
                        uint8_t *cflags, uint32_t *out_total_slots);
typedef struct {
  uint32_t        root_vertex;   /* S                                                                         */
  uint32_t        root_row;      /* row of the table set that holds S's SPT                                    */
  uint32_t        n_slots;       /* entries of the five arrays below: <= 64 * n_mask_words                     */
  const uint32_t *nbr;           /* HOST arrays [n_slots] (hspf_lfa_candidates); nbr_row is read for candidates only */
  const uint32_t *nbr_row;
  const uint32_t *cost;
  const uint32_t *root_link;
  const uint8_t  *cflags;
} hspf_lfa_protect;
typedef struct {                 /* DEVICE pointers                                                            */
  uint32_t *alt_slot;            /* [n_prot][n_vertices]                                                       */
  uint32_t *alt_metric;          /* [n_prot][n_vertices]                                                       */
  uint8_t  *alt_flags;           /* [n_prot][n_vertices]                                                       */
  uint64_t *cand_mask;           /* [n_prot][n_vertices][n_mask_words] or NULL                                 */
  uint64_t *node_mask;           /* [n_prot][n_vertices][n_mask_words] or NULL                                 */
  uint32_t *coverage;            /* [n_prot][HSPF_LFA_COVERAGE_WORDS]                                          */
} hspf_lfa_out;
/* Several protected roots may share one table set (whole-network coverage: a 64-root batch in which every root's neighbours
 * are rows of the batch too).  The per-root tables are staged once, everything is enqueued on the context's stream, and the
 * call synchronises once at the end (as hspf_ancestors_device).  Argument errors — a NULL required pointer, root_row or a
 * candidate's nbr_row >= n_rows, root_vertex or a candidate's nbr >= n_vertices, n_slots > 64 * n_mask_words — return
 * HSPF_E_INVAL with a text in hspf_last_error before anything is launched. */
int hspf_lfa_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                    const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                    const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, hspf_lfa_out *out_dev);

/* ---- per-primary alternates for ECMP destinations (RFC 5286 sections 3.4, 3.6): new symbol, same ABI number ----------------------
 * hspf_lfa_device stops at a destination with two or more primary slots: it sets HSPF_LFA_ECMP and writes two sets that are safe
 * against ALL primaries at once.  That is not the answer a RIB needs.  Two primaries behind the same first link of S (two routers on
 * one LAN) share that link's fate and do not protect each other; two parallel links to one neighbour E protect each other's link
 * and not the node E; and protection is reported, and a backup installed, PER primary next hop
 * (frr-protection-available-{link,node,downstream}-type).  hspf_lfa_ecmp_device gives, for every destination with at least two
 * primary slots and for every one of those primaries, the alternate of that primary and what it protects.
 *
 * Inputs.  The forward table set, `prot`, n_prot and lfa_flags exactly as for hspf_lfa_device.  No graph.
 * Terms as there: S a protected root, D a vertex of S's SPT, D != S, P = the bits of mask_S[D] below n_slots.  The call speaks only
 * about D with popcount(P) >= 2.  For such a D and a protected primary h in P let E = nbr[h] (may be HSPF_NO_ROOT).  A slot k with
 * N = nbr[k] is judged by ONE rule whether or not k is itself a primary; every sum is evaluated in 64 bits and a term that is
 * HSPF_DIST_INF makes its inequality false:
 *   cand(h)     k != h,  and nbr[k] != HSPF_NO_ROOT,  and d(N, D) < d(N, S) + d(S, D),  and root_link[k] != root_link[h],  and
 *               (cflags[k] has no NO_TRANSIT, or N == D, or the call passes HSPF_LFA_IGNORE_OVERLOAD);
 *   node(h)     k is in cand(h), E != HSPF_NO_ROOT, and d(N, D) < d(N, E) + d(E, D)   (N == E makes this false by itself);
 *   downstream  d(N, D) < d(S, D);
 *   choice      (section 3.6 in spirit) a member of node(h) before a member of cand(h) only, then a slot that is in P before one
 *               that is not, then the smaller cost[k] + d(N, D) (64 bits), then the smaller slot index.
 * A primary with positive costs passes the loop-free inequality by itself; applying it to primaries anyway keeps one rule and is
 * safe with zero-cost router links.  A primary whose target is a network vertex (nbr == HSPF_NO_ROOT) can be protected; it can
 * never be an alternate.
 *
 * Output: a compact stream in CSR form over (protected root, destination).  DEVICE pointers:
 *   ea_ptr       u32 [n_prot * n_vertices + 1].  For i * n_vertices + D:  ea_ptr[. + 1] - ea_ptr[.] is popcount(P) when that is at
 *                least 2, and 0 otherwise (also for D == S and D outside the SPT).  ALWAYS written completely.
 *   the entries of one D are its primaries in ascending slot order; entry arrays of cap_entries elements each:
 *   ea_primary   u32  h
 *   ea_slot      u32  the chosen slot, or HSPF_LFA_NO_SLOT
 *   ea_metric    u32  cost[k] + d(N, D) saturated at 0xFFFFFFFE, 0 for none
 *   ea_flags     u8   HSPF_LFA_LINK_PROTECT | HSPF_LFA_NODE_PROTECT | HSPF_LFA_DOWNSTREAM with their alt_flags values, and
 *                     HSPF_LFA_EA_PRIMARY 0x20: the alternate is another primary of D.  (0x01 and 0x02 mean something else in
 *                     alt_flags; 0x20 is HSPF_LFA_LAN_PRIMARY only in the outputs of the LAN calls, which this call is not.)
 *   ea_coverage  u32 [n_prot][HSPF_LFA_ECMP_COVERAGE_WORDS], counted on the device: ECMP destinations | entries | entries with
 *                an alternate | with a node-protecting one | with a downstream one | whose alternate is a primary | ECMP
 *                destinations of which EVERY primary has an alternate.
 * *out_total (HOST): the total number of entries, = ea_ptr[n_prot * n_vertices].
 *
 * Capacity.  The caller passes cap_entries and entry arrays of that size.  When the total exceeds cap_entries the call still
 * returns 0 and writes ea_ptr and *out_total; the entry arrays and ea_coverage are then unspecified, and the caller repeats the
 * call with larger arrays (the convention of hspf_lfa_candidates and hspf_routes_events: an overflow is not an error).
 * cap_entries == 0 with NULL entry arrays and NULL ea_coverage asks for ea_ptr and the total alone.
 * Argument errors — everything hspf_lfa_device rejects; ea_ptr or out_total NULL; an entry array or ea_coverage NULL with
 * cap_entries > 0; and the host-side bound  sum over the protected roots of n_vertices * max(n_slots, 1) >= 2^32  (the stream is
 * indexed in 32 bits: split the protect list) — return HSPF_E_INVAL with a text in hspf_last_error that names
 * hspf_lfa_ecmp_device, before anything is launched.  The staged tables are those of hspf_lfa_device; everything is enqueued on
 * the context's stream and the call synchronises once at the end.
 *
 * From ea_* to a backup next hop per primary next hop: INTEGRATION.md §5s.
 *
 * OUT OF SCOPE: ECMP backups per prefix (hspf_routes_backup_ecmp_device, below: this call's rule with d_N(p) in place of d(N, D)); the LAN-safe and
 * SRLG-safe variants of this call; remote or TI-LFA repairs for an ECMP primary that has no alternate; entries for destinations
 * with a single primary (alt_slot of hspf_lfa_device is that answer). */
#define HSPF_LFA_EA_PRIMARY            0x20u   /* ea_flags: the alternate is another primary of the destination */
#define HSPF_LFA_ECMP_COVERAGE_WORDS   7u
typedef struct {                 /* DEVICE pointers                                                            */
  uint32_t *ea_ptr;              /* [n_prot * n_vertices + 1]                                                  */
  uint32_t *ea_primary;          /* [cap_entries]                                                              */
  uint32_t *ea_slot;             /* [cap_entries]                                                              */
  uint32_t *ea_metric;           /* [cap_entries]                                                              */
  uint8_t  *ea_flags;            /* [cap_entries]                                                              */
  uint32_t *ea_coverage;         /* [n_prot][HSPF_LFA_ECMP_COVERAGE_WORDS]                                     */
} hspf_lfa_ecmp_out;
int hspf_lfa_ecmp_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                         const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, uint64_t cap_entries,
                         hspf_lfa_ecmp_out *out_dev, uint64_t *out_total);

/* ---- broadcast-link protection (RFC 5286 section 3.3) for the alternates and the per-prefix backups: new symbols, same ABI number --
 * When S reaches D across a LAN, what S detects is the loss of its attachment to that LAN, and an alternate must not cross the LAN
 * either: it must be loop-free with respect to the pseudonode.  root_link alone refuses only candidates behind the same first link
 * of S; a neighbour on another link whose own shortest path to D crosses the LAN passes hspf_lfa_device.  The two calls below are
 * hspf_lfa_device and hspf_routes_backup_device with that one more condition.  It needs d(N, L), an entry of a row the caller
 * already has, and d(L, D): one more row of the same batch, rooted at the LAN's network vertex L — the run is
 * [S] ++ (S's neighbour routers) ++ (S's LANs), same run_flags.
 *
 * hspf_lfa_lan_candidates (host arithmetic, no context; slot numbering, row checks and return convention of hspf_lfa_candidates):
 *   lan[k]  the vertex that link root_link[k] of S's OWN row leads to, when that vertex carries HSPF_VF_NETWORK and the link passes
 *           the two-way check; HSPF_NO_ROOT otherwise (a point-to-point link).  Filled for EVERY slot, like cost / root_link: a
 *           slot's LAN is a function of its root_link alone, so all slots behind one link of S agree.
 * hspf_lfa_lan is parallel to hspf_lfa_protect: entry i belongs to prot[i], with the same n_slots.
 *
 * hspf_lfa_lan_device.  Everything of hspf_lfa_device, with one more condition on membership of `cand` (and through it on `node`,
 * the choice, alt_* and both masks): for every primary slot p in P with L = lan[p] != HSPF_NO_ROOT
 *     d(N, D) < d(N, L) + d(L, D)
 * d(N, L) is read from N's row at vertex L, d(L, D) from row lan_row[p]; the sum is evaluated in 64 bits and an HSPF_DIST_INF term
 * makes the inequality false.  D == L makes it false by itself: nothing protects the LAN's own vertex against the LAN's failure.
 * alt_flags gains
 *   HSPF_LFA_LAN_PRIMARY   some primary of D crosses a LAN of S
 *   HSPF_LFA_LAN_REFUSED   at least one slot met every condition of hspf_lfa_device's cand and failed only the LAN inequality
 * and coverage is [n_prot][HSPF_LFA_LAN_COVERAGE_WORDS]: the five words of hspf_lfa_device, then the destinations with each of the
 * two new bits.  With every lan[k] == HSPF_NO_ROOT the outputs are those of hspf_lfa_device (and coverage words 5, 6 are 0).
 * Argument errors — everything hspf_lfa_device rejects, lan == NULL, a NULL lan / lan_row array with n_slots > 0, lan[k] >=
 * n_vertices where it is not HSPF_NO_ROOT, lan_row[k] >= n_rows for such a k — return HSPF_E_INVAL with a text that names
 * hspf_lfa_lan_device, before anything is launched.
 *
 * hspf_routes_backup_lan_device.  Everything of hspf_routes_backup_device ("per-prefix backup routes on device", below), with
 * cand(p) additionally requiring, for every e in P with L = lan[e] != HSPF_NO_ROOT
 *     d_N(p) < d(N, L) + d_L(p)
 * where d_L(p) is d_X(p) of that section evaluated on row lan_row[e] (no advertiser reached from L: false; HSPF_PFX_SATURATING as
 * there).  The fallback to the per-link repair (HSPF_BK_NODE / _PAIR) is taken only when lan[e] == HSPF_NO_ROOT: the repairs of
 * hspf_tilfa_device are not known to avoid the LAN, so a LAN primary without an alternate is HSPF_BK_NONE — unless lfa_flags has
 * HSPF_LFA_LAN_SAFE_REPAIRS, the caller's word that tilfa_dev was computed from hspf_rlfa_lan_device's tables: then the fallback
 * is taken for a LAN primary too.  Every other call ignores that bit.  bk_flags gains the two
 * bits above with the same values (for HSPF_BK_ECMP .. HSPF_BK_NONE); bk_coverage is [n_prot][HSPF_BK_LAN_COVERAGE_WORDS]: the
 * seven kinds, then the prefixes with each of the two bits.  Argument errors name hspf_routes_backup_lan_device.
 *
 * LAN-aware P / extended-P / Q spaces are hspf_rlfa_lan_device ("remote loop-free alternates with LAN-safe spaces", below).
 * OUT OF SCOPE: LAN-safe hspf_rlfa_node_device repairs; alternates over the
 * protected LAN itself to another attached router (node-protecting but not link-protecting in RFC 5286 Figure 5: root_link keeps
 * refusing them); a pseudonode deeper on the path than S's own attachment; SRLGs. */
#define HSPF_LFA_LAN_PRIMARY         0x20u   /* alt_flags / bk_flags of the LAN calls */
#define HSPF_LFA_LAN_REFUSED         0x40u
#define HSPF_LFA_LAN_SAFE_REPAIRS    0x02u   /* lfa_flags of hspf_routes_backup_lan_device */
#define HSPF_LFA_LAN_COVERAGE_WORDS  7u
#define HSPF_BK_LAN_COVERAGE_WORDS   9u
int hspf_lfa_lan_candidates(const hspf_csr *csr, uint32_t root, uint32_t cap, uint32_t *lan, uint32_t *out_total_slots);
typedef struct {                 /* parallel to hspf_lfa_protect: entry i belongs to prot[i]                   */
  const uint32_t *lan;           /* HOST [n_slots]  hspf_lfa_lan_candidates                                    */
  const uint32_t *lan_row;       /* HOST [n_slots]  row of the table set holding the SPT ROOTED AT lan[k]; read only where
                                    lan[k] != HSPF_NO_ROOT                                                     */
} hspf_lfa_lan;
int hspf_lfa_lan_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                        const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                        const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, uint32_t lfa_flags,
                        hspf_lfa_out *out_dev);

/* ---- remote loop-free alternates on device (RFC 7490): PQ nodes per protected link: new symbols, same ABI number --------
 * hspf_lfa_device counts the destinations that get no alternate and leaves them unrepaired; on rings and sparse meshes that is
 * most of them.  Remote LFA tunnels to a PQ node: a router that S — or another neighbour of S — reaches without crossing the
 * protected link (P-space, extended P-space) and that reaches the link's far end E without crossing it either (Q-space).  P and
 * extended P are inequalities over the forward rows a caller already has for LFA; Q needs distances TO S and TO E: one more
 * run of the same root list on the transposed graph (hspf_csr_transpose).
 *
 * hspf_csr_transpose (host arithmetic, no context): row t of the result lists (source u, cost) of every link u -> t of `csr`,
 * ordered by ascending u, then by position in u's row (a stable counting sort).  Outputs are the caller's: row_ptr_out[n + 1],
 * col_out[e], metric_out[e].  vflags and max_path_metric are the caller's to reuse unchanged for the upload.  HSPF_E_INVAL on
 * what hspf_graph_upload rejects (and on a link target >= n_vertices).  Of a run on the transposed graph ONLY `dist` has a
 * meaning — dist[row of X][v] = d(v, X), the distance from v TO X: the two-way check, the overload rule ("not expanded unless
 * root") and prefix pruning are symmetric under reversal, hops and first-hop masks depend on row order and are not.  One
 * exception: a vertex with HSPF_VF_NO_EXPAND reaches nothing as a root but is reached as a target, so the row of such an X and
 * the entries of such a v are NOT reverse distances; hspf_rlfa_device excludes such vertices from every set.
 *
 * hspf_rlfa_device.  The forward table set (dist, vflags_out, first_hop_mask: [n_rows][n_vertices]), `prot` and lfa_flags are
 * exactly those of hspf_lfa_device; rdist_dev [n_rows][n_vertices] is `dist` of a run of the SAME root list on the transposed
 * graph, so root_row / nbr_row index both sets and rdist[row of X][v] = d(v, X).  On a graph whose costs are symmetric
 * (every link u -> v has its reverse at the same cost) d(v, X) = d(X, v) and the caller may pass the forward dist as rdist_dev;
 * on any other graph that gives a wrong Q-space.  `g` is the (forward or transposed) uploaded graph: its resident vertex
 * flags are read.  alt_flags_in_dev: NULL, or the alt_flags [n_prot][n_vertices] hspf_lfa_device wrote for the same `prot`.
 *
 * Per protected root S and per slot e with nbr[e] != HSPF_NO_ROOT (a candidate slot; E = nbr[e], c = cost[e]); N_k = nbr[k].
 * Every sum is evaluated in 64 bits; a term that is HSPF_DIST_INF makes its inequality false.
 *   eligible(v)   v is in S's SPT, v != S, v carries neither HSPF_VF_NETWORK nor HSPF_VF_NO_EXPAND, and no HSPF_VF_NO_TRANSIT
 *                 unless the call passes HSPF_LFA_IGNORE_OVERLOAD.  E itself may be eligible (parallel links).
 *                 Every set below holds eligible vertices only.
 *   P(e, v)       d(S, v) < c + d(E, v)
 *   XP(e, k, v)   d(N_k, v) < d(N_k, S) + c + d(E, v)   for a via-slot k: nbr[k] != HSPF_NO_ROOT, root_link[k] != root_link[e],
 *                 and cflags[k] has no HSPF_LFA_C_NO_TRANSIT unless the call passes HSPF_LFA_IGNORE_OVERLOAD
 *   Q(e, v)       d(v, E) < d(v, S) + c                 (rdist)
 *   release point of v: the smallest (64 bits) of d(S, v) if P holds (via = HSPF_RLFA_VIA_SELF) and cost[k] + d(N_k, v) over
 *                 the k with XP (via = k); on a tie S comes first, then the smaller k.  The release metric is that sum
 *                 saturated at 0xFFFFFFFE.
 *   PQ node of (S, e): among the v with (P or some XP) and Q, the smallest release metric, then the smallest vertex index.
 * Outputs (DEVICE pointers; slots are strided by 64 * n_mask_words per protected root):
 *   pq_node / pq_via / pq_metric [n_prot][stride]: the PQ node, the via of its release point, its release metric; HSPF_NO_ROOT /
 *                 HSPF_LFA_NO_SLOT / 0 for "none" — also for slots that are no candidates and for slots >= n_slots.
 *   pq_counts [n_prot][stride][4]: the number of v in P | in P or some XP | in Q | in (P or some XP) and Q.
 *   space_flags u8 / space_via u32 [n_prot][stride][n_vertices], optional (NULL skips the table): HSPF_RLFA_IN_P, _IN_XP (some
 *                 XP), _IN_Q, _ELIGIBLE; the via of v's release point (HSPF_LFA_NO_SLOT: v has none).  0 / HSPF_LFA_NO_SLOT for
 *                 slots that are no candidates.
 *   rl_node / rl_via [n_prot][n_vertices], per destination D of S (D != S, in S's SPT): filled for every D with exactly ONE
 *                 primary slot e — and, when alt_flags_in_dev is given, no HSPF_LFA_LINK_PROTECT — with the PQ node and via of
 *                 e; HSPF_NO_ROOT / HSPF_LFA_NO_SLOT everywhere else, also where that one slot is no candidate (its target
 *                 is a network vertex or S) or has no PQ node.
 *   rl_coverage [n_prot][4], counted on the device: destinations with exactly one primary | of those, the ones whose given
 *                 alt_flags have HSPF_LFA_LINK_PROTECT (0 when alt_flags_in_dev is NULL) | of the rest, the ones with a PQ
 *                 node | the ones still uncovered.
 * Argument errors — a NULL required pointer, n_vertices not the graph's, and everything hspf_lfa_device rejects in `prot` —
 * return HSPF_E_INVAL with a text in hspf_last_error that names hspf_rlfa_device, before anything is launched.  Everything is
 * enqueued on the context's stream; the call synchronises once at the end.
 *
 * Node-protecting remote LFA (RFC 8102: the PQ node's path to D may cross E) is hspf_rlfa_node_select_device /
 * hspf_rlfa_node_device, below.  OUT OF SCOPE: loop-freeness with respect to a
 * LAN pseudonode in THIS call (the same root_link rule and the same limitation as hspf_lfa_device: hspf_rlfa_lan_device, below,
 * adds it); segment lists beyond one tunnel
 * (hspf_tilfa_device, below, adds one forced adjacency).  Shared-risk link groups: hspf_rlfa_srlg_device ("SRLG-safe alternates
 * and remote-LFA spaces", below). */
#define HSPF_RLFA_VIA_SELF       0xFFFFFFFEu   /* pq_via / space_via / rl_via: released by S itself (P-space) */
#define HSPF_RLFA_IN_P           0x01u         /* space_flags */
#define HSPF_RLFA_IN_XP          0x02u
#define HSPF_RLFA_IN_Q           0x04u
#define HSPF_RLFA_ELIGIBLE       0x08u
#define HSPF_RLFA_COUNT_WORDS    4u
#define HSPF_RLFA_COVERAGE_WORDS 4u
int hspf_csr_transpose(const hspf_csr *csr, uint32_t *row_ptr_out, uint32_t *col_out, uint32_t *metric_out);
typedef struct {                 /* DEVICE pointers; stride = 64 * n_mask_words                               */
  uint32_t *pq_node;             /* [n_prot][stride]                                                           */
  uint32_t *pq_via;              /* [n_prot][stride]                                                           */
  uint32_t *pq_metric;           /* [n_prot][stride]                                                           */
  uint32_t *pq_counts;           /* [n_prot][stride][HSPF_RLFA_COUNT_WORDS]                                    */
  uint8_t  *space_flags;         /* [n_prot][stride][n_vertices] or NULL                                       */
  uint32_t *space_via;           /* [n_prot][stride][n_vertices] or NULL                                       */
  uint32_t *rl_node;             /* [n_prot][n_vertices]                                                       */
  uint32_t *rl_via;              /* [n_prot][n_vertices]                                                       */
  uint32_t *rl_coverage;         /* [n_prot][HSPF_RLFA_COVERAGE_WORDS]                                         */
} hspf_rlfa_out;
int hspf_rlfa_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                     const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                     const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                     hspf_rlfa_out *out_dev);

/* ---- remote loop-free alternates with LAN-safe spaces (RFC 7490 on broadcast links): new symbol, same ABI number --------------
 * hspf_rlfa_device builds P, extended P and Q against the far router E only.  When the protected slot crosses a LAN of S
 * (lan[e] of hspf_lfa_lan_candidates is a vertex L), what fails is S's attachment to L, and a tunnel to the PQ node — or the PQ
 * node's own path on to E — that crosses the pseudonode breaks on exactly the failure it repairs.  hspf_rlfa_lan_device is
 * hspf_rlfa_device with the hspf_lfa_lan columns of hspf_lfa_lan_device (`lan` parallel to `prot`) and one more condition per set.
 *
 * Both table sets come from the root list [S] ++ (S's neighbour routers) ++ (S's LANs) that hspf_lfa_lan_device asks for: `dist`
 * is the forward run, rdist_dev the `dist` of the SAME list on the transposed graph, so rdist[lan_row[e]][v] = d(v, L).  The
 * forward-dist-as-rdist shortcut of hspf_rlfa_device is NEVER valid here: a pseudonode's links cost 0 one way, so no graph with a
 * LAN has symmetric costs.
 *
 * For a candidate slot e with L = lan[e] != HSPF_NO_ROOT and lr = lan_row[e] (sums in 64 bits; an HSPF_DIST_INF term makes the
 * inequality false):
 *   P_lan(e, v)      P(e, v)      and  d(S, v)   < d(S, L)   + d(L, v)      S's row at v and at L; row lr at v
 *   XP_lan(e, k, v)  XP(e, k, v)  and  d(N_k, v) < d(N_k, L) + d(L, v)      N_k's row at v and at L; row lr at v
 *   Q_lan(e, v)      Q(e, v)      and  d(v, E)   < d(v, L)   + d(L, E)      rdist[rowE][v], rdist[lr][v]; dist[lr][E]
 * Each is the literal conjunction, so every LAN-safe set is a subset of hspf_rlfa_device's.  Eligibility, via-slot admission, the
 * tie order, the release point and its metric (now over P_lan / XP_lan), the PQ choice, rl_node / rl_via and the four bits of
 * space_flags are those of hspf_rlfa_device — the bits now mean the LAN-safe sets, so the tables can be fed to hspf_tilfa_device
 * as they are.  A slot with lan[e] == HSPF_NO_ROOT is computed exactly as by hspf_rlfa_device.
 * Outputs: hspf_rlfa_out with wider count arrays.
 *   pq_counts   [n_prot][stride][HSPF_RLFA_LAN_COUNT_WORDS]: the four words of hspf_rlfa_device over the LAN-safe sets, then the
 *               number of v in the plain (P or some XP) and Q that are not in the LAN-safe one (0 for a point-to-point slot).
 *   rl_coverage [n_prot][HSPF_RLFA_LAN_COVERAGE_WORDS]: the four words of hspf_rlfa_device, then the one-primary destinations
 *               whose primary crosses a LAN | of those, the ones left uncovered although the plain rule had a PQ node.
 * With every lan[k] == HSPF_NO_ROOT all shared outputs equal hspf_rlfa_device's and the new words are 0.  Argument errors —
 * everything hspf_rlfa_device rejects, everything hspf_lfa_lan_device rejects in `lan` — return HSPF_E_INVAL with a text that names
 * hspf_rlfa_lan_device, before anything is launched.  From rl_* / ti_* on a LAN primary to a tunnel: INTEGRATION.md 5n.
 *
 * OUT OF SCOPE: a forced adjacency across another LAN (p -> network vertex -> q is still not offered by hspf_tilfa_device, so
 * LAN-heavy graphs keep more HSPF_TILFA_NONE than necessary); hspf_rlfa_node_select_device on these tables (its NP / NXP release
 * paths are re-derived against E only: not LAN-safe); LAN pseudonodes as the protected node; per-prefix Q-spaces; SRLGs. */
#define HSPF_RLFA_LAN_COUNT_WORDS    5u
#define HSPF_RLFA_LAN_COVERAGE_WORDS 6u
int hspf_rlfa_lan_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                         const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, uint32_t lfa_flags,
                         const uint8_t *alt_flags_in_dev, hspf_rlfa_out *out_dev);

/* ---- SRLG-safe alternates and remote-LFA spaces on device: new symbols, same ABI number ----------------------------------------
 * A shared-risk link group (SRLG) is a set of links that fail together: one fibre, one conduit, one line card.  hspf_lfa_device
 * offers a neighbour whose own shortest path runs over a link in the same conduit as the primary; hspf_rlfa_device offers a PQ node
 * whose tunnel or onward path does.  The two calls below are those calls with one more inequality per set and per group member,
 * read from rows of the same batch: the SPTs rooted at the member links' endpoints.
 *
 * SRLG table.  The caller holds, per directed link of its CSR (a link is its position in `col`), a list of u32 group ids:
 * grp_ptr[n_edges + 1] and grp[].  For a protected root S and a first-hop slot k the PROTECTED LINK is the link at position
 * root_link[k] of S's own row; all slots behind one link of S agree, as lan[] does.  A MEMBER of slot k is any OTHER directed link
 * of the graph that shares at least one group id with the protected link, described by six fields:
 *   tail a | pos (its position within a's row) | head b | cost w | tail_row | head_row
 * ordered by ascending (tail, pos).  tail_row / head_row are the rows of the table set that hold the SPTs rooted at a and at b
 * (the caller's: it made the run).
 * Root list.  The batch is [S] ++ (S's neighbour routers) ++ (the distinct tails and heads of all members that are not already in
 * the list); the forward and the transposed run use the same list and the same run_flags.
 *
 * crosses(X -> v, i), for a source X, a target v and a member i, holds iff d(X, a_i) and d(b_i, v) are BOTH FINITE and
 *     d(X, v) >= d(X, a_i) + w_i + d(b_i, v)                                   (the sum in 64 bits)
 * A member that X does not reach, or whose head does not reach v, is not crossed.  This is NOT the LAN rule, where an
 * HSPF_DIST_INF term makes the inequality false and so refuses: a member may lie anywhere in the graph, and an unreachable one
 * must not refuse anything.  A head b_i that carries HSPF_VF_NO_TRANSIT is expanded as the root of its row, so d(b_i, v) may be
 * finite where no transit path through b_i exists: the test is conservative there — it may refuse, it never wrongly admits.
 * Member i is LOCAL to slot k when tail_i == S and pos_i == root_link[k]: slot k's own first link is in the group.
 *
 * hspf_srlg_members (host arithmetic, no context; slot numbering, row checks and return value of hspf_lfa_candidates): the members
 * of every slot of `root`.  mem_ptr[k] .. mem_ptr[k + 1] delimit slot k's members in the four columns; mem_ptr holds the true
 * offsets for k <= min(slots, cap_slots) (so it has cap_slots + 1 entries), the columns are written below cap_members (any
 * output may be NULL).  *out_total_slots / *out_total_members say what to size the arrays for when calling again.  HSPF_E_INVAL
 * on what hspf_lfa_candidates rejects, on a row_ptr that is not the one of a whole CSR (row_ptr[0] == 0, monotone,
 * row_ptr[n_vertices] == n_edges), on a member's head >= n_vertices and on a grp_ptr that is not monotone.
 *
 * hspf_srlg is parallel to hspf_lfa_protect (entry i belongs to prot[i], same n_slots): mem_ptr[n_slots + 1] and the six member
 * columns as HOST arrays.
 *
 * hspf_lfa_srlg_device.  Everything of hspf_lfa_device, with more conditions on membership of `cand` (and through it on `node`, the
 * choice, alt_* and both masks): for every primary slot p in P and every member i of p
 *     i is not local to k,   and   crosses(N_k -> D, i) is false
 * d(N_k, a_i) is read from N_k's row at a_i, d(b_i, D) from row head_row_i at D.  alt_flags gains
 *   HSPF_LFA_SRLG_REFUSED   at least one slot met every condition of hspf_lfa_device's cand and failed only an SRLG condition
 * (0x20 and 0x40 stay with the LAN calls, so a combined call has room).  coverage is [n_prot][HSPF_LFA_SRLG_COVERAGE_WORDS]: the
 * five words of hspf_lfa_device | destinations with a primary that has at least one member | destinations with
 * HSPF_LFA_SRLG_REFUSED.  With every mem_ptr all zero the outputs are those of hspf_lfa_device and words 5, 6 are 0.
 *
 * hspf_rlfa_srlg_device.  Everything of hspf_rlfa_device, with the three spaces of a candidate slot e narrowed by its members i:
 *   P_s(e, v)      P(e, v)      and for no i  crosses(S -> v, i)
 *   XP_s(e, k, v)  XP(e, k, v)  and no member of e is local to k  and for no i  crosses(N_k -> v, i)
 *   Q_s(e, v)      Q(e, v)      and for no i:  d(v, a_i) and d(b_i, E) both finite and d(v, E) >= d(v, a_i) + w_i + d(b_i, E)
 * with d(v, E) = rdist[row of E][v], d(v, a_i) = rdist[tail_row_i][v], d(b_i, E) = dist[head_row_i][E].  Eligibility, via-slot
 * admission, the tie order, the release point and its metric, the PQ choice, rl_* and the four space_flags bits are those of
 * hspf_rlfa_device evaluated over the safe sets: the bits mean the safe sets, so the tables feed hspf_tilfa_device unchanged.
 *   pq_counts   [n_prot][stride][HSPF_RLFA_SRLG_COUNT_WORDS]: the four words over the safe sets, then the number of v in the plain
 *               (P or some XP) and Q that are not in the safe one.
 *   rl_coverage [n_prot][HSPF_RLFA_SRLG_COVERAGE_WORDS]: the four plain words | one-primary destinations whose primary has
 *               members | of those, the ones left uncovered although the plain rule had a PQ node.
 * With no members all shared outputs equal hspf_rlfa_device's.  The forward-dist-as-rdist shortcut stays valid on graphs with
 * symmetric costs.
 *
 * Argument errors of both device calls — everything the plain call rejects, srlg == NULL, a NULL mem_ptr, a NULL column where
 * mem_ptr[n_slots] > mem_ptr[0], a mem_ptr that is not monotone, more than HSPF_SRLG_MAX_MEMBERS members on one slot, tail or head
 * >= n_vertices, tail_row or head_row >= n_rows — return HSPF_E_INVAL with a text that names the call, before anything is launched.
 *
 * OUT OF SCOPE: the forced adjacency of a TI-LFA pair — HSPF_TILFA_NODE repairs from the safe tables are SRLG-safe, and a
 * HSPF_TILFA_PAIR has its p in the safe P / XP set and its q in the safe Q set, but the forced link p -> q may itself be a member:
 * the consumer compares (ti_p, ti_link) with the slot's (tail, pos) list (hspf_routes_backup_srlg_device, below,
 * does it per prefix);
 * node-protecting calls with SRLGs; SRLGs combined with the LAN inequalities (a LAN slot is treated as by the plain calls);
 * the fuzz_frr run of tools/gpu_fuzz.py (the randomised differential run does not draw group tables). */
#define HSPF_SRLG_MAX_MEMBERS          16u
#define HSPF_LFA_SRLG_REFUSED          0x80u   /* alt_flags of hspf_lfa_srlg_device */
#define HSPF_LFA_SRLG_COVERAGE_WORDS   7u
#define HSPF_RLFA_SRLG_COUNT_WORDS     5u
#define HSPF_RLFA_SRLG_COVERAGE_WORDS  6u
int hspf_srlg_members(const hspf_csr *csr, uint32_t root, const uint32_t *grp_ptr, const uint32_t *grp, uint32_t cap_slots,
                      uint32_t cap_members, uint32_t *mem_ptr, uint32_t *tail, uint32_t *pos, uint32_t *head, uint32_t *cost,
                      uint32_t *out_total_slots, uint32_t *out_total_members);
typedef struct {                 /* parallel to hspf_lfa_protect: entry i belongs to prot[i]; HOST arrays       */
  const uint32_t *mem_ptr;       /* [n_slots + 1]                                                              */
  const uint32_t *tail;          /* [mem_ptr[n_slots]] each: hspf_srlg_members ...                             */
  const uint32_t *pos;
  const uint32_t *head;
  const uint32_t *cost;
  const uint32_t *tail_row;      /* ... and the rows of the SPTs rooted at tail / head                         */
  const uint32_t *head_row;
} hspf_srlg;
int hspf_lfa_srlg_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                         const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                         hspf_lfa_out *out_dev);
int hspf_rlfa_srlg_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                          const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                          const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                          const uint8_t *alt_flags_in_dev, hspf_rlfa_out *out_dev);

/* ---- two-segment repair paths on device (TI-LFA, link protection): new symbol, same ABI number ----------------------------
 * hspf_rlfa_device leaves rl_coverage[3]: destinations whose one primary link has no LFA and whose extended P-space and
 * Q-space do not intersect.  The segment-routing repair for them is two segments: tunnel to a node p of the extended P-space,
 * force ONE adjacency p -> q into the Q-space, and let q forward normally.  hspf_tilfa_device finds, per protected link, the
 * cheapest repair among the PQ nodes (one segment) and those (p, link) pairs (two segments).
 *
 * Inputs.  The forward table set, rdist_dev, `prot`, n_prot, lfa_flags and the optional alt_flags_in_dev are exactly those of
 * hspf_rlfa_device.  space_flags_dev / space_via_dev [n_prot][stride][n_vertices] are REQUIRED: the tables hspf_rlfa_device wrote
 * for the same `prot` and lfa_flags (eligibility and the overload rule are read from them, not evaluated again).  `g` must be
 * the FORWARD graph — its links are scanned — where hspf_rlfa_device takes either.
 * LAN-safe use: fed with the tables hspf_rlfa_lan_device wrote (same `prot`, same two table sets) and the alt_flags of
 * hspf_lfa_lan_device, every repair avoids the pseudonode of the slot's LAN by construction — p is in P_lan / XP_lan, q in Q_lan,
 * and the forced adjacency joins two routers; ti_counts[..][0] then equals pq_counts[..][3] of hspf_rlfa_lan_device.  The kernel
 * is the same (tests/test_gpu_rlfa_lan.py holds it to that contract).
 *
 * Per protected root S and candidate slot e (E = nbr[e], rowE = nbr_row[e]); every sum is evaluated in 64 bits.
 *   rel(v)        the release metric of v, rebuilt from via = space_via[e][v]: d(S, v) for HSPF_RLFA_VIA_SELF, cost[via] +
 *                 d(N_via, v) for a slot.
 *   single node   v with HSPF_RLFA_ELIGIBLE, (HSPF_RLFA_IN_P or _IN_XP) and _IN_Q:   total = rel(v) + rdist[rowE][v].
 *   pair          the link at position j of p's row in g, target q != p, cost w, where p has _ELIGIBLE and (_IN_P or _IN_XP),
 *                 q has _ELIGIBLE and _IN_Q, and the link passes the two-way check (q's row lists p; the cost is not compared:
 *                 the rule of hspf_slot_table / hspf_lfa_candidates):   total = rel(p) + w + rdist[rowE][q].
 *                 S is never eligible, so the protected link itself is never the forced adjacency.
 *   order         totals are saturated at 0xFFFFFFFE first and compared afterwards (as pq_metric); then: the smaller total, a
 *                 single node before a pair, the smaller p, the smaller q, the smaller position j.
 * On a graph of routers with symmetric costs >= 1 and no overload the best total is the SPF distance S -> E with the protected
 * link removed, and there is no repair exactly when E is unreachable there (tests/test_host_tilfa.py).
 * Outputs (DEVICE pointers; slots are strided by 64 * n_mask_words per protected root; "none" — also for slots that are no
 * candidates and for slots >= n_slots — is HSPF_NO_ROOT / HSPF_LFA_NO_SLOT / 0):
 *   ti_kind u8 [n_prot][stride]     HSPF_TILFA_NONE, HSPF_TILFA_NODE (one segment), HSPF_TILFA_PAIR (two)
 *   ti_p / ti_q                     the chosen nodes; ti_q == ti_p for HSPF_TILFA_NODE
 *   ti_via                          the via of p's release point (HSPF_RLFA_VIA_SELF or a slot of S)
 *   ti_link                         position of the chosen link within p's row of g; HSPF_LFA_NO_SLOT unless HSPF_TILFA_PAIR
 *   ti_metric                       the saturated total
 *   ti_counts [n_prot][stride][2]   the number of single nodes (= pq_counts[..][3] of hspf_rlfa_device) | of usable (p, link) pairs
 *   td_kind u8 [n_prot][n_vertices] per destination D of S with exactly one primary slot: HSPF_TILFA_D_LFA the given alt_flags
 *                                   have HSPF_LFA_LINK_PROTECT, _D_NODE / _D_PAIR that slot has a one- / two-segment repair,
 *                                   _D_NONE uncovered (also where the slot is no candidate); 0 everywhere else
 *   td_coverage [n_prot][5]         counted on the device: destinations with exactly one primary, then the four classes
 * Argument errors — what hspf_rlfa_device rejects, and NULL space tables — return HSPF_E_INVAL with a text in hspf_last_error
 * that names hspf_tilfa_device, before anything is launched.  The call sizes its own scratch (the selection keys and the
 * graph's two-way flags, staged from the host mirror: one byte per link), enqueues everything on the context's stream and
 * synchronises once at the end.
 *
 * From a result to a segment list: the first segment is the Node-SID of ti_p, sent out of the first hop
 * ti_via names (S's own primary next hops towards ti_p for HSPF_RLFA_VIA_SELF, else the neighbour of slot ti_via); for a pair
 * the second segment is the Adj-SID p advertises for the link at position ti_link of its row.
 *
 * OUT OF SCOPE: adjacencies across a LAN pseudonode (p -> network vertex -> q is not offered: q must be a router in p's own
 * row); node protection (one-segment node-protecting repairs: hspf_rlfa_node_device, below; two-segment ones:
 * hspf_tilfa_node_select_device / hspf_tilfa_node_device, below that); repairs that end at the destination instead of at E,
 * follow its post-convergence path, or need more than one adjacency (hspf_tilfa_pc_device, below: per destination, up to
 * HSPF_TIPC_MAX_ADJ adjacencies). */
#define HSPF_TILFA_NONE           0u            /* ti_kind */
#define HSPF_TILFA_NODE           1u
#define HSPF_TILFA_PAIR           2u
#define HSPF_TILFA_D_LFA          1u            /* td_kind */
#define HSPF_TILFA_D_NODE         2u
#define HSPF_TILFA_D_PAIR         3u
#define HSPF_TILFA_D_NONE         4u
#define HSPF_TILFA_COUNT_WORDS    2u
#define HSPF_TILFA_COVERAGE_WORDS 5u
typedef struct {                 /* DEVICE pointers; stride = 64 * n_mask_words                               */
  uint8_t  *ti_kind;             /* [n_prot][stride]                                                           */
  uint32_t *ti_p;                /* [n_prot][stride]                                                           */
  uint32_t *ti_q;                /* [n_prot][stride]                                                           */
  uint32_t *ti_via;              /* [n_prot][stride]                                                           */
  uint32_t *ti_link;             /* [n_prot][stride]                                                           */
  uint32_t *ti_metric;           /* [n_prot][stride]                                                           */
  uint32_t *ti_counts;           /* [n_prot][stride][HSPF_TILFA_COUNT_WORDS]                                   */
  uint8_t  *td_kind;             /* [n_prot][n_vertices]                                                       */
  uint32_t *td_coverage;         /* [n_prot][HSPF_TILFA_COVERAGE_WORDS]                                        */
} hspf_tilfa_out;
int hspf_tilfa_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                      const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                      const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                      const uint8_t *space_flags_dev, const uint32_t *space_via_dev, hspf_tilfa_out *out_dev);

/* ---- TI-LFA repairs along the post-convergence path (link protection): new symbol, same ABI number ---------------------------
 * hspf_tilfa_device repairs a LINK: its segment list ends at the far router E, whatever the destination, and it offers one
 * adjacency at most.  The TI-LFA draft asks for the repair of each DESTINATION to follow the path that destination has after
 * convergence.  hspf_tilfa_pc_device walks that path — the row hspf_run_failures_device gives for the failed link — from D up to
 * S and cuts it into: a Node-SID, up to HSPF_TIPC_MAX_ADJ Adj-SIDs, and D's own shortest path from there.
 *
 * Inputs.  Everything hspf_tilfa_device takes, with the same meaning (`g` the FORWARD graph; space_flags_dev / space_via_dev
 * REQUIRED), and
 *   pc_dist_dev [n_pc_rows][n_vertices]  DEVICE: the `dist` table of an hspf_run_failures_device call on `g`.
 *   pc_row [n_prot][stride]              HOST, u32: for slot e of protected root i the row of pc_dist_dev that holds
 *                                        {HSPF_FAIL_ROOT_LINK, root_link[e]} of that root; HSPF_NO_ROOT: no row.
 *   run_flags                            those the failure run was given; only HSPF_RUN_IGNORE_OVERLOAD is looked at.
 *   max_walk                             1 .. 65535: the vertices a walk may visit.
 *
 * Per protected root S and destination D != S in S's SPT with exactly ONE primary slot e (the population of td_kind);
 * c = cost[e], pc = row pc_row[e].  Every sum is evaluated in 64 bits; totals saturate at 0xFFFFFFFE as ti_metric.
 *   parent(v)   for v != S with pc[v] != HSPF_DIST_INF: among the links (u -> v, cost w, position j in u's row of the caller's
 *               CSR) the scenario run itself uses — they survive the two-way check and u has no HSPF_VF_NO_EXPAND (the device
 *               graph's in-link arrays hold exactly those, also after hspf_graph_patch); u is a network, or S, or has no
 *               HSPF_VF_NO_TRANSIT, or run_flags has HSPF_RUN_IGNORE_OVERLOAD; the link is not the failed one (u == S and
 *               j == root_link[e]); and it is tight, pc[u] + w == pc[v] — the one with the smallest (u, j).
 *   walk        cur = D, q = D, an empty gap list.  At each cur, in this order:
 *                 1. cur has HSPF_RLFA_ELIGIBLE and _IN_Q in space_flags[e]: q = cur, the gap list is emptied.
 *                 2. cur has _ELIGIBLE, _IN_P or _IN_XP, and a release point (space_via[e][cur] != HSPF_LFA_NO_SLOT): p = cur, stop.
 *                 3. cur == S: p = S, no node segment, stop.
 *                 4. the hop (position j of parent(cur)'s row, head cur) goes to the FRONT of the gap list; cur = parent(cur).
 *               A walk that has visited max_walk vertices without stopping is HSPF_TIPC_D_WALK: tight links of cost 0 that form a
 *               cycle are the one way to get there on a row of the failure run, and the cap makes that outcome deterministic.
 *   repair      the Node-SID of p sent out of via = space_via[e][p] exactly as ti_via is; the Adj-SIDs of the recorded links
 *               p -> ... -> q; from q the packet follows q's own shortest path to D.
 * Why the last part is safe: q is in Q(e) or q == D.  e is a primary of D, so d(S, D) = c + d(E, D).  A shortest path q -> D over
 * the failed link would cost d(q, S) + c + d(E, D); Q(e) says d(q, E) < d(q, S) + c, so that is more than d(q, E) + d(E, D),
 * which is at least d(q, D): no shortest path of q to D crosses the link.  (q == D: the path is empty.)  The first part is
 * hspf_rlfa_device's P / XP inequality, the middle part is forced link by link and never the failed link.
 *
 * Outputs (DEVICE pointers, [n_prot][n_vertices] unless stated; "none" is HSPF_NO_ROOT / HSPF_LFA_NO_SLOT / 0 as elsewhere):
 *   tp_kind u8    0 outside the population, else
 *                 HSPF_TIPC_D_LFA     the given alt_flags have HSPF_LFA_LINK_PROTECT; the vertex is not walked
 *                 HSPF_TIPC_D_REPAIR  a repair was found
 *                 HSPF_TIPC_D_NONE    the slot is no candidate, has no row, or pc[D] is HSPF_DIST_INF (also: a vertex on the walk
 *                                     has no parent, which a row of that link never shows)
 *                 HSPF_TIPC_D_LONG    the walk stopped with more than HSPF_TIPC_MAX_ADJ hops between p and q
 *                 HSPF_TIPC_D_LAN     not _D_LONG, and a vertex strictly between p and q carries HSPF_VF_NETWORK
 *                 HSPF_TIPC_D_WALK    see above
 *   for HSPF_TIPC_D_REPAIR, "none" otherwise:
 *   tp_p, tp_via, tp_q        tp_via is HSPF_LFA_NO_SLOT for p == S (no node segment)
 *   tp_n_adj u8               the recorded hops, 0 .. HSPF_TIPC_MAX_ADJ
 *   tp_hop_pos / tp_hop_head  [n_prot][n_vertices][HSPF_TIPC_MAX_ADJ], in the order p -> q: the position of the link in its
 *                             tail's row, and its head; the tail of hop 0 is p, of hop i the head of hop i - 1; the head of the
 *                             last hop is q.  Unused entries HSPF_LFA_NO_SLOT / HSPF_NO_ROOT.
 *   tp_metric                 rel(p) + pc[D] - pc[p], saturated; rel(p) rebuilt from the via as hspf_tilfa_device does, rel(S) = 0,
 *                             pc[S] = 0
 *   tp_flags u8               HSPF_TIPC_ON_PC rel(p) == pc[p]: the repair costs exactly the post-convergence distance |
 *                             HSPF_TIPC_P_IS_ROOT | HSPF_TIPC_Q_IS_DEST
 *   tp_coverage [n_prot][12]  counted on the device: the population | the six classes in the order of their values | the
 *                             _D_REPAIR destinations with tp_n_adj = 0, 1, 2, 3, 4
 * Argument errors — what hspf_tilfa_device rejects, NULL pc_dist_dev / pc_row, a pc_row entry given for a slot that is no
 * candidate (or >= n_slots), a row >= n_pc_rows, max_walk outside 1 .. 65535 — return HSPF_E_INVAL with a text in hspf_last_error
 * that names hspf_tilfa_pc_device, before anything is launched.  The call sizes its own scratch (8 bytes per vertex and slot
 * with a row, released before it returns), enqueues everything on the context's stream and synchronises once at the end.
 *
 * From a result to a label stack: INTEGRATION.md §5w.
 *
 * LAN PRIMARIES.  For a slot behind a pseudonode (root_link[e] leads to a network vertex) the failed link is S's link onto the
 * LAN, but the P / XP sets of hspf_rlfa_device are relative to E: the release path S -> p may run over that link to ANOTHER
 * router of the LAN (the limitation hspf_rlfa_device states; hspf_rlfa_lan_device removes it for its own outputs).  Such a
 * _D_REPAIR is safe against the failure of E's attachment, not of S's link onto the LAN; it shows as tp_metric < pc[D].  The
 * adjacencies and q's tail end are safe either way.  A caller that protects the LAN link itself must not install these
 * (INTEGRATION.md 5w).
 *
 * OUT OF SCOPE: node protection (HSPF_FAIL_VERTEX rows); SRLG- and LAN-safe tables (the call reads whatever space tables it is
 * given, but the walk knows of one failed link only); destinations with several primaries (ECMP); per-prefix mapping;
 * adjacencies across a pseudonode (_D_LAN, as hspf_tilfa_device); packed and asynchronous forms. */
#define HSPF_TIPC_MAX_ADJ        4u
#define HSPF_TIPC_D_LFA          1u            /* tp_kind */
#define HSPF_TIPC_D_REPAIR       2u
#define HSPF_TIPC_D_NONE         3u
#define HSPF_TIPC_D_LONG         4u
#define HSPF_TIPC_D_LAN          5u
#define HSPF_TIPC_D_WALK         6u
#define HSPF_TIPC_ON_PC          0x01u         /* tp_flags */
#define HSPF_TIPC_P_IS_ROOT      0x02u
#define HSPF_TIPC_Q_IS_DEST      0x04u
#define HSPF_TIPC_COVERAGE_WORDS 12u
typedef struct {                 /* DEVICE pointers                                                            */
  uint8_t  *tp_kind;             /* [n_prot][n_vertices]                                                       */
  uint32_t *tp_p;                /* [n_prot][n_vertices]                                                       */
  uint32_t *tp_via;              /* [n_prot][n_vertices]                                                       */
  uint32_t *tp_q;                /* [n_prot][n_vertices]                                                       */
  uint8_t  *tp_n_adj;            /* [n_prot][n_vertices]                                                       */
  uint32_t *tp_hop_pos;          /* [n_prot][n_vertices][HSPF_TIPC_MAX_ADJ]                                    */
  uint32_t *tp_hop_head;         /* [n_prot][n_vertices][HSPF_TIPC_MAX_ADJ]                                    */
  uint32_t *tp_metric;           /* [n_prot][n_vertices]                                                       */
  uint8_t  *tp_flags;            /* [n_prot][n_vertices]                                                       */
  uint32_t *tp_coverage;         /* [n_prot][HSPF_TIPC_COVERAGE_WORDS]                                         */
} hspf_tilfa_pc_out;
int hspf_tilfa_pc_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                         const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev, const uint32_t *rdist_dev,
                         const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const uint8_t *alt_flags_in_dev,
                         const uint8_t *space_flags_dev, const uint32_t *space_via_dev, const uint32_t *pc_dist_dev, uint32_t n_pc_rows,
                         const uint32_t *pc_row, uint32_t run_flags, uint32_t max_walk, hspf_tilfa_pc_out *out_dev);

/* ---- per-prefix backup routes on device (RFC 5286 section 6.1): new symbol, same ABI number --------------------------------
 * hspf_lfa_device, hspf_rlfa_device and hspf_tilfa_device protect VERTICES and LINKS; what a RIB installs, and what
 * hspf_routes_device delivers, is per PREFIX.  For a prefix with one advertiser the two agree; for a multi-homed prefix
 * (anycast loopbacks, redistributed prefixes, an OSPF stub network on two routers) they do not: the loop-free inequality is
 * evaluated against the neighbour's distance to the PREFIX, the minimum over all advertisers, not against its distance to the
 * vertex S happens to use — a neighbour can be an alternate for the prefix and none for S's attaining vertex.
 * hspf_routes_backup_device joins the tables: per (protected root, prefix) a backup next hop, or the per-link repair of the one
 * primary link.  It takes no graph.
 *
 * Inputs.  The forward table set, `prot`, n_prot and lfa_flags are exactly those of hspf_lfa_device.  `table` is the HOST prefix
 * table of hspf_routes_device: flags may be 0, HSPF_PFX_SATURATING, and HSPF_PFX_LAST_MIN together with either;
 * HSPF_PFX_RESIDENT is honoured under hspf_routes_device's contract (the two calls share one staged copy: a table this call
 * uploaded is resident for the next hspf_routes_device and the other way round).  routes_dev is what hspf_routes_device wrote for
 * the same table set and table: protected root i reads row prot[i].root_row of it.  tilfa_dev: NULL (no remote fallback), or
 * the hspf_tilfa_out hspf_tilfa_device wrote for the same `prot`; only ti_kind, ti_via and ti_metric are read.
 *
 * Per protected root S and prefix p; every sum is evaluated in 64 bits; a term that is HSPF_DIST_INF, or an advertiser whose
 * vertex is not HSPF_RF_IN_SPT in the row, contributes nothing.
 *   d_X(p)      for a row root X: the minimum over the entries (v, m) of p of d(X, v) + m.  With HSPF_PFX_SATURATING each
 *               d(X, v) + m is first saturated at 0xFFFFFFFF as u32, as hspf_routes_device does (the saturated value is a
 *               number, not "not reached").  HSPF_PFX_LAST_MIN changes nothing in d_X(p).
 *   d_S(p)      routes.best_metric: read, not recomputed (a number whenever the route exists).  P = the bits of
 *               routes.nexthop_mask[p] below n_slots, read as given (HSPF_PFX_LAST_MIN only changed which mask
 *               hspf_routes_device left).  The route is absent when best_entry == 0xFFFFFFFF.
 *   cand(p)     slot k with N = nbr[k] != HSPF_NO_ROOT iff  d_N(p) < d(N, S) + d_S(p),  and root_link[k] != root_link[e] for
 *               every e in P,  and k is not in P,  and (cflags[k] has no HSPF_LFA_C_NO_TRANSIT, or the call passes
 *               HSPF_LFA_IGNORE_OVERLOAD, or N's own entry (v == N) attains d_N(p): N delivers without transiting)
 *   node(p)     k in cand(p), P has at least one slot whose nbr is a router, and for every such slot with E its nbr:
 *               d_N(p) < d(N, E) + d_E(p)
 *   downstream  d_N(p) < d_S(p)
 *   choice      only when popcount(P) == 1: a member of node before a member of cand only, then the smallest cost[k] + d_N(p)
 *               (64 bits), then the smallest k — the rule of hspf_lfa_device with p in place of D
 *   fallback    popcount(P) == 1 with e the one primary slot, no slot chosen, tilfa_dev given and ti_kind[e] != HSPF_TILFA_NONE:
 *               the per-link repair of e backs up the prefix (it delivers to E = nbr[e], and E is S's next hop towards p)
 * Outputs (DEVICE pointers, [n_prot][n_prefixes] unless stated):
 *   bk_kind u8     HSPF_BK_NO_ROUTE no route | _LOCAL a route and P is empty | _ECMP popcount(P) >= 2 | _LFA an alternate slot
 *                  was chosen | _NODE / _PAIR the one- / two-segment repair of the primary link | _NONE one primary, nothing found
 *   bk_primary     the one primary slot e for HSPF_BK_LFA .. HSPF_BK_NONE (the consumer indexes ti_p / ti_q / ti_link with it),
 *                  HSPF_LFA_NO_SLOT otherwise
 *   bk_slot        _LFA: the chosen slot; _NODE / _PAIR: ti_via[e] (may be HSPF_RLFA_VIA_SELF); HSPF_LFA_NO_SLOT otherwise
 *   bk_metric      _LFA: cost[k] + d_N(p) saturated at 0xFFFFFFFE; _NODE / _PAIR: ti_metric[e] — the repair's cost to E, NOT a
 *                  cost to p; 0 otherwise
 *   bk_flags u8    _LFA: HSPF_LFA_NODE_PROTECT | HSPF_LFA_DOWNSTREAM with the bit values of alt_flags; 0 otherwise
 *   bk_cand_mask / bk_node_mask   u64 [n_prot][n_prefixes][n_mask_words], optional (NULL skips the table): the two sets for
 *                  HSPF_BK_ECMP .. HSPF_BK_NONE, zero elsewhere
 *   bk_coverage    u32 [n_prot][HSPF_BK_COVERAGE_WORDS], counted on the device: the number of prefixes of each kind, 0 .. 6
 * Argument errors — a NULL required pointer, everything hspf_lfa_device rejects in `prot`, HSPF_PFX_ORDERED, everything the
 * table checks of hspf_routes_device reject — return HSPF_E_INVAL with a text in hspf_last_error that names
 * hspf_routes_backup_device, before any kernel is launched.  Everything is enqueued on the context's stream; the call
 * synchronises once at the end.
 *
 * From bk_* to a next hop with a backup and its label stack: INTEGRATION.md §5k.
 *
 * OUT OF SCOPE: HSPF_PFX_ORDERED tables (OSPFv3's interleaved fold: HSPF_E_INVAL); backups for ECMP routes (per vertex:
 * hspf_lfa_ecmp_device, above; per prefix: hspf_routes_backup_ecmp_device, below; the two sets are still written); per-prefix Q-spaces (the remote repair is the primary LINK's, as in
 * td_kind; node-protecting remote repairs per prefix are hspf_routes_backup_node_device's, below).  Loop-freeness with respect to a LAN pseudonode is not checked by THIS
 * call: hspf_routes_backup_lan_device ("broadcast-link protection", above) adds it.  One lane walks one prefix: there is no wave-per-prefix path for prefixes with very many advertisers. */
#define HSPF_BK_NO_ROUTE       0u
#define HSPF_BK_LOCAL          1u
#define HSPF_BK_ECMP           2u
#define HSPF_BK_LFA            3u
#define HSPF_BK_NODE           4u
#define HSPF_BK_PAIR           5u
#define HSPF_BK_NONE           6u
#define HSPF_BK_COVERAGE_WORDS 7u
typedef struct {                 /* DEVICE pointers                                                            */
  uint8_t  *bk_kind;             /* [n_prot][n_prefixes]                                                       */
  uint32_t *bk_primary;          /* [n_prot][n_prefixes]                                                       */
  uint32_t *bk_slot;             /* [n_prot][n_prefixes]                                                       */
  uint32_t *bk_metric;           /* [n_prot][n_prefixes]                                                       */
  uint8_t  *bk_flags;            /* [n_prot][n_prefixes]                                                       */
  uint64_t *bk_cand_mask;        /* [n_prot][n_prefixes][n_mask_words] or NULL                                 */
  uint64_t *bk_node_mask;        /* [n_prot][n_prefixes][n_mask_words] or NULL                                 */
  uint32_t *bk_coverage;         /* [n_prot][HSPF_BK_COVERAGE_WORDS]                                           */
} hspf_backup_out;
int hspf_routes_backup_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                              const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                              const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const hspf_prefix_table *table,
                              const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev, hspf_backup_out *out_dev);
/* The same with loop-freeness towards the pseudonodes of the primaries' LANs ("broadcast-link protection", above). */
int hspf_routes_backup_lan_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                  const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                  const hspf_lfa_protect *prot, const hspf_lfa_lan *lan, uint32_t n_prot, uint32_t lfa_flags,
                                  const hspf_prefix_table *table, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev,
                                  hspf_backup_out *out_dev);

/* ---- per-primary backups for ECMP prefixes (RFC 5286 sections 3.4, 3.6, 6.1): new symbol, same ABI number -------------------------
 * The four per-prefix calls stop at a route with two or more primary next hops: HSPF_BK_ECMP, the two sets that are safe against
 * ALL primaries at once, no choice.  In a fat-tree or a meshed core that is most of the RIB.  The per-vertex stream of
 * hspf_lfa_ecmp_device cannot stand in: a multi-homed prefix can be ECMP through two advertisers whose vertices have one primary
 * each, and the loop-free inequality has to be held against the neighbour's distance to the PREFIX.  hspf_routes_backup_ecmp_device
 * gives, for every prefix whose route has at least two primary slots and for every one of those primaries, the backup of that
 * primary and what it protects: the rule of hspf_lfa_ecmp_device with d_N(p) in place of d(N, D), and the per-link repair of
 * hspf_routes_backup_device as the fallback.
 *
 * Inputs.  Exactly those of hspf_routes_backup_device: the forward table set, `prot`, n_prot, lfa_flags, the HOST prefix table
 * (HSPF_PFX_SATURATING, HSPF_PFX_LAST_MIN and HSPF_PFX_RESIDENT as there; HSPF_PFX_ORDERED: HSPF_E_INVAL), routes_dev, and
 * tilfa_dev (NULL: no fallback; only ti_kind, ti_via and ti_metric are read).  cap_entries and out_total follow the convention of
 * hspf_lfa_ecmp_device.  No graph.
 * Terms as for hspf_routes_backup_device: S a protected root, p a prefix whose route exists (best_entry != 0xFFFFFFFF), P = the bits
 * of nexthop_mask[p] below n_slots, d_X(p) the minimum over p's entries with the same saturation rule, d_S(p) = best_metric, read
 * and not recomputed.  The call speaks only about p with popcount(P) >= 2.  For such a p and a protected primary h in P let
 * E = nbr[h] (may be HSPF_NO_ROOT).  A slot k with N = nbr[k] is judged by ONE rule whether or not k is itself a primary; every sum
 * is evaluated in 64 bits and a term that is "not reached" makes its inequality false:
 *   cand(h)     k != h,  and nbr[k] != HSPF_NO_ROOT,  and d_N(p) < d(N, S) + d_S(p),  and root_link[k] != root_link[h],  and
 *               (cflags[k] has no HSPF_LFA_C_NO_TRANSIT, or the call passes HSPF_LFA_IGNORE_OVERLOAD, or N's own entry (v == N)
 *               attains d_N(p): N delivers without transiting, as in hspf_routes_backup_device);
 *   node(h)     k is in cand(h), E is a router (E != HSPF_NO_ROOT), d_E(p) exists, and d_N(p) < d(N, E) + d_E(p)   (N == E makes
 *               this false by itself);
 *   downstream  d_N(p) < d_S(p);
 *   choice      the rule of hspf_lfa_ecmp_device: a member of node(h) before a member of cand(h) only, then a slot that is in P
 *               before one that is not, then the smaller cost[k] + d_N(p) (64 bits), then the smaller slot index;
 *   fallback    no slot chosen for h, tilfa_dev given and ti_kind[h] != HSPF_TILFA_NONE: the per-link repair of h backs up this
 *               next hop (it delivers to E, and E is a next hop of S towards p: the argument of the one-primary fallback).
 *
 * Output: a compact stream in CSR form over (protected root, prefix).  DEVICE pointers:
 *   eb_ptr       u32 [n_prot * n_prefixes + 1].  For i * n_prefixes + p:  eb_ptr[. + 1] - eb_ptr[.] is popcount(P) when that is at
 *                least 2, and 0 otherwise (an absent route, a route with fewer than two primaries).  ALWAYS written completely.
 *   the entries of one p are its primaries in ascending slot order; entry arrays of cap_entries elements each:
 *   eb_primary   u32  h
 *   eb_kind      u8   HSPF_BK_LFA a slot was chosen | HSPF_BK_NODE / HSPF_BK_PAIR the one- / two-segment repair of h | HSPF_BK_NONE
 *   eb_slot      u32  _LFA: the chosen slot; _NODE / _PAIR: ti_via[h] (may be HSPF_RLFA_VIA_SELF); HSPF_LFA_NO_SLOT otherwise
 *   eb_metric    u32  _LFA: cost[k] + d_N(p) saturated at 0xFFFFFFFE; _NODE / _PAIR: ti_metric[h] — the cost to E, NOT to p; 0
 *                     otherwise
 *   eb_flags     u8   _LFA: HSPF_LFA_NODE_PROTECT | HSPF_LFA_DOWNSTREAM | HSPF_LFA_EA_PRIMARY (the backup is another primary of p)
 *                     with their existing bit values; 0 otherwise
 *   eb_coverage  u32 [n_prot][HSPF_BK_ECMP_COVERAGE_WORDS], counted on the device: ECMP prefixes | entries | entries of kind _LFA |
 *                node-protecting entries | downstream entries | entries whose alternate is a primary | repaired entries (_NODE or
 *                _PAIR) | ECMP prefixes of which EVERY primary has a backup of any kind.
 * *out_total (HOST): the total number of entries, = eb_ptr[n_prot * n_prefixes].
 *
 * Capacity.  When the total exceeds cap_entries the call still returns 0 and writes eb_ptr and *out_total; the entry arrays and
 * eb_coverage are then unspecified, and the caller repeats the call with larger arrays.  cap_entries == 0 with NULL entry arrays
 * and NULL eb_coverage asks for eb_ptr and the total alone.
 * Argument errors — everything hspf_routes_backup_device rejects; eb_ptr or out_total NULL; an entry array or eb_coverage NULL with
 * cap_entries > 0; and the host-side bound  sum over the protected roots of n_prefixes * max(n_slots, 1) >= 2^32  (the stream is
 * indexed in 32 bits: split the protect list) — return HSPF_E_INVAL with a text in hspf_last_error that names
 * hspf_routes_backup_ecmp_device, before anything is launched.  Everything is enqueued on the context's stream and the call
 * synchronises once at the end.
 *
 * From eb_* to a backup per next hop of a prefix: INTEGRATION.md §5t.
 *
 * OUT OF SCOPE: the LAN-safe and node-protecting-remote variants of this call (hspf_routes_backup_lan_device, _srlg_ and
 * _node_ still answer HSPF_BK_ECMP with the two sets; the SRLG-safe variant is hspf_routes_backup_ecmp_srlg_device, below);
 * per-prefix Q-spaces; HSPF_PFX_ORDERED tables. */
#define HSPF_BK_ECMP_COVERAGE_WORDS    8u
typedef struct {                 /* DEVICE pointers                                                            */
  uint32_t *eb_ptr;              /* [n_prot * n_prefixes + 1]                                                  */
  uint32_t *eb_primary;          /* [cap_entries]                                                              */
  uint8_t  *eb_kind;             /* [cap_entries]                                                              */
  uint32_t *eb_slot;             /* [cap_entries]                                                              */
  uint32_t *eb_metric;           /* [cap_entries]                                                              */
  uint8_t  *eb_flags;            /* [cap_entries]                                                              */
  uint32_t *eb_coverage;         /* [n_prot][HSPF_BK_ECMP_COVERAGE_WORDS]                                      */
} hspf_backup_ecmp_out;
int hspf_routes_backup_ecmp_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                   const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                   const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags, const hspf_prefix_table *table,
                                   const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev, uint64_t cap_entries,
                                   hspf_backup_ecmp_out *out_dev, uint64_t *out_total);

/* ---- node-protecting remote loop-free alternates on device (RFC 8102): new symbols, same ABI number -------------------------
 * hspf_rlfa_device protects LINKS: the tunnel to its PQ node, and that node's own path on to the destination, may run straight
 * through the router E behind the protected link.  RFC 8102 keeps the cheapest few link-protecting PQ nodes of every protected
 * link whose release path avoids the node E (the RFC's default limit is 16), runs a forward SPF rooted at each of them, and
 * tests per destination whether the node's own path avoids E.  "A forward SPF per PQ node" is one more hspf_run_device of a
 * many-roots batch on the same read-only graph; the two steps around it are the calls below.  Neither takes a graph.
 *
 * hspf_rlfa_node_select_device.  The forward table set, `prot` and lfa_flags are exactly those of hspf_lfa_device;
 * space_flags_dev [n_prot][stride][n_vertices] is what hspf_rlfa_device wrote for the same `prot` and lfa_flags (Q-space is read
 * from it: no reverse distances).  max_pq is 1 .. HSPF_RLFA_NODE_MAX_PQ.
 * Per protected root S and candidate slot e (E = nbr[e]); N_k = nbr[k]; every sum is evaluated in 64 bits; a term that is
 * HSPF_DIST_INF makes its inequality false.
 *   NP(e, v)      d(S, v) < d(S, E) + d(E, v): S's own shortest paths to v avoid the node E
 *   NXP(e, k, v)  d(N_k, v) < d(N_k, E) + d(E, v)   for a via-slot k of hspf_rlfa_device's XP rule (nbr[k] != HSPF_NO_ROOT,
 *                 root_link[k] != root_link[e], cflags[k] without HSPF_LFA_C_NO_TRANSIT unless the call passes
 *                 HSPF_LFA_IGNORE_OVERLOAD) with N_k != E (a parallel link to E is no way round E)
 *   v qualifies   iff space_flags[e][v] has HSPF_RLFA_ELIGIBLE and _IN_Q, and _IN_P or _IN_XP (so the list is a subset of the
 *                 link-protecting PQ set whatever the vertex flags of the graph), v != E, and NP or some NXP holds
 *   release point the smallest (64 bits) of d(S, v) if NP holds (via = HSPF_RLFA_VIA_SELF) and cost[k] + d(N_k, v) over the k
 *                 with NXP (via = k); on a tie S comes first, then the smaller k.  The release metric is that sum saturated
 *                 at 0xFFFFFFFE.
 * Outputs (DEVICE pointers; slots are strided by 64 * n_mask_words per protected root):
 *   nq_node / nq_via / nq_metric [n_prot][stride][max_pq]: the qualifying vertices in ascending order of (release metric, vertex
 *                 index), the first min(nq_count, max_pq) of them; the rest of a list, and the lists of slots that are no
 *                 candidates or >= n_slots, are HSPF_NO_ROOT / HSPF_LFA_NO_SLOT / 0.
 *   nq_count [n_prot][stride]: ALL qualifying vertices of the slot (may exceed max_pq); 0 for slots that are no candidates.
 *
 * hspf_rlfa_node_device.  ydist_dev [n_yrows][n_vertices] is `dist` of a FORWARD hspf_run_device whose root list was y_roots
 * (HOST array): the caller's choice — the union of the lists, or fewer.  HSPF_NO_ROOT entries are skipped; a vertex listed
 * twice may use either row; a listed node without a row is skipped.  The vertex -> row map is built on the device.  sel_dev
 * and max_pq are those of the select call; alt_flags_in_dev: NULL, or the alt_flags of hspf_lfa_device for the same `prot`.
 * Per S and destination D in S's SPT, D != S, with exactly ONE primary slot e (E = nbr[e]):
 *   entry j < min(nq_count[e], max_pq) with Y = nq_node[e][j] protects D iff  d(Y, D) < d(Y, E) + d(E, D)   (d(Y, .) from Y's
 *                 row, d(E, D) from row nbr_row[e] of the forward set)
 *   choice        among the protecting entries the smallest nq_metric[e][j] + d(Y, D) (64 bits), then the smaller j
 *   nd_kind u8    0 unless D has exactly one primary; else, in this order: HSPF_NP_D_LFA the given alt_flags have
 *                 HSPF_LFA_NODE_PROTECT | HSPF_NP_D_NONE the slot is no candidate | HSPF_NP_D_LAST_HOP D == E (node protection is
 *                 undefined: the link repair is all there is) | HSPF_NP_D_PQ an entry was chosen | HSPF_NP_D_NONE
 *   nd_node / nd_via / nd_metric   for HSPF_NP_D_PQ the chosen entry's node and via, and the sum saturated at 0xFFFFFFFE;
 *                 HSPF_NO_ROOT / HSPF_LFA_NO_SLOT / 0 otherwise
 *   nd_set u32    optional (NULL skips the table): bit j = entry j protects D, for the D that reach the test; 0 otherwise
 *   nd_coverage [n_prot][5], counted on the device: destinations with exactly one primary, then the four classes.
 * Argument errors of both — a NULL required pointer, everything hspf_lfa_device rejects in `prot`, max_pq outside
 * 1 .. HSPF_RLFA_NODE_MAX_PQ, n_yrows == 0, a y_roots entry >= n_vertices that is not HSPF_NO_ROOT — return HSPF_E_INVAL with a
 * text in hspf_last_error that names the function, before anything is launched.  Everything is enqueued on the context's
 * stream; each call synchronises once at the end.
 *
 * From nd_* to a tunnel that survives the neighbour's failure: INTEGRATION.md §5l.
 *
 * Where no listed PQ node protects a destination (HSPF_NP_D_NONE), a forced adjacency after the tunnel may: the two-segment
 * node-protecting repairs of hspf_tilfa_node_select_device / hspf_tilfa_node_device, below.
 * OUT OF SCOPE: LAN pseudonodes as the protected
 * node (the failure of every router behind the primary's LAN); SRLGs.  Per prefix: hspf_routes_backup_node_device, below. */
#define HSPF_RLFA_NODE_MAX_PQ   32u
#define HSPF_NP_D_LFA           1u             /* nd_kind */
#define HSPF_NP_D_PQ            2u
#define HSPF_NP_D_LAST_HOP      3u
#define HSPF_NP_D_NONE          4u
#define HSPF_NP_COVERAGE_WORDS  5u
typedef struct {                 /* DEVICE pointers; stride = 64 * n_mask_words                               */
  uint32_t *nq_node;             /* [n_prot][stride][max_pq]  HSPF_NO_ROOT-padded                              */
  uint32_t *nq_via;              /* [n_prot][stride][max_pq]  HSPF_RLFA_VIA_SELF or a slot; HSPF_LFA_NO_SLOT padding */
  uint32_t *nq_metric;           /* [n_prot][stride][max_pq]  release metric; 0 padding                        */
  uint32_t *nq_count;            /* [n_prot][stride]          ALL qualifying vertices (may exceed max_pq)      */
} hspf_rlfa_node_sel;
int hspf_rlfa_node_select_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                 const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                 const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags,
                                 const uint8_t *space_flags_dev, uint32_t max_pq, hspf_rlfa_node_sel *out_dev);
typedef struct {                 /* DEVICE pointers                                                            */
  uint8_t  *nd_kind;             /* [n_prot][n_vertices]                                                       */
  uint32_t *nd_node;             /* [n_prot][n_vertices]                                                       */
  uint32_t *nd_via;              /* [n_prot][n_vertices]                                                       */
  uint32_t *nd_metric;           /* [n_prot][n_vertices]                                                       */
  uint32_t *nd_set;              /* [n_prot][n_vertices] bit j = list entry j protects; or NULL                */
  uint32_t *nd_coverage;         /* [n_prot][HSPF_NP_COVERAGE_WORDS]                                           */
} hspf_rlfa_node_out;
int hspf_rlfa_node_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                          const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                          const hspf_lfa_protect *prot, uint32_t n_prot,
                          const uint32_t *ydist_dev, const uint32_t *y_roots /* HOST */, uint32_t n_yrows,
                          const hspf_rlfa_node_sel *sel_dev, uint32_t max_pq,
                          const uint8_t *alt_flags_in_dev, hspf_rlfa_node_out *out_dev);

/* ---- two-segment node-protecting repairs on device (TI-LFA node protection): new symbols, same ABI number -------------------
 * hspf_rlfa_node_device can only choose among the link-protecting PQ nodes: routers in both the extended P-space and the Q-space
 * of the protected link.  Where that set is empty — exactly where hspf_tilfa_device needs a pair — or where every PQ node's own
 * path to the destination crosses the neighbour, every destination ends as HSPF_NP_D_NONE.  The repair for them is the pair of
 * hspf_tilfa_device made node-protecting: a tunnel to a node p of the extended P-space whose release path avoids the NODE E, one
 * forced adjacency p -> q into the Q-space, and a q whose own path to the destination avoids E.  The destination test depends
 * on q alone, so the select call lists q's (each with the cheapest way into it), the caller runs ONE forward hspf_run_device
 * over the listed q's, and the second call tests per destination — the shape of the RLFA-node pair above.
 *
 * hspf_tilfa_node_select_device.  The forward table set, `prot`, n_prot and lfa_flags are exactly those of hspf_lfa_device; `g` is
 * the FORWARD graph (its links are scanned, as by hspf_tilfa_device); space_flags_dev [n_prot][stride][n_vertices] is what
 * hspf_rlfa_device wrote for the same `prot` and lfa_flags.  max_pairs is 1 .. HSPF_TILFA_NODE_MAX_PAIRS.
 * Per protected root S and candidate slot e (E = nbr[e]); every sum is evaluated in 64 bits; a term that is HSPF_DIST_INF makes
 * its inequality false.
 *   relN(p), via  the release point of p under hspf_rlfa_node_select_device's rule (NP: S itself, via = HSPF_RLFA_VIA_SELF; NXP
 *                 for a via-slot k with N_k != E; S first, then the smaller k), as the UNSATURATED 64-bit sum.  p has a
 *                 node-avoiding release point iff NP or some NXP holds.
 *   a link qualifies   the link at position j of p's row in g, target q, cost w, iff it is a usable pair of hspf_tilfa_device (p has
 *                 HSPF_RLFA_ELIGIBLE and _IN_P or _IN_XP; q != p; q has _ELIGIBLE and _IN_Q; the link passes the two-way check),
 *                 p != E, q != E, and p has a node-avoiding release point.
 *   entry of q    over the qualifying links into q the smallest relN(p) + w, saturated at 0xFFFFFFFE first and compared
 *                 afterwards (as ti_metric); then the smaller p, then the smaller j.  Only the cheapest way into a q matters.
 *   list          the q's with a qualifying link in ascending (saturated entry metric, q); the first min(tq_count, max_pairs).
 * Outputs (DEVICE pointers; slots are strided by 64 * n_mask_words per protected root):
 *   tq_q / tq_p / tq_link / tq_via / tq_metric [n_prot][stride][max_pairs]: per list entry q, the p of its entry, the position j
 *                 of the link in p's row of g, the via of p's release point, the saturated entry metric.  The rest of a list,
 *                 and the lists of slots that are no candidates or >= n_slots, are HSPF_NO_ROOT / HSPF_NO_ROOT /
 *                 HSPF_LFA_NO_SLOT / HSPF_LFA_NO_SLOT / 0.
 *   tq_count [n_prot][stride]: ALL distinct q with a qualifying link (may exceed max_pairs); 0 for slots that are no candidates.
 * Scratch.  The call keeps one 8-byte cell per (protected root, candidate slot, vertex): 8 bytes x (the largest n_slots of the
 * call) x n_vertices per protected root, next to the staged two-way bytes (one per link).  It does NOT tile: a call whose cells
 * exceed 2^30 (8 GiB) returns HSPF_E_NOMEM and the caller splits `prot`.  At 100 000 routers and 4 slots that is 3.2 MB per root.
 *
 * hspf_tilfa_node_device.  The inputs of hspf_rlfa_node_device with sel_dev / max_pairs of the select call above in place of
 * hspf_rlfa_node_sel / max_pq: ydist_dev [n_yrows][n_vertices] is `dist` of a FORWARD hspf_run_device whose root list was y_roots
 * (HOST array) — the caller's choice of listed q's; HSPF_NO_ROOT entries are skipped, a vertex listed twice may use either
 * row, a listed q without a row is skipped.  nd_kind_in_dev: NULL, or the nd_kind [n_prot][n_vertices] hspf_rlfa_node_device wrote
 * for the same `prot`.
 * Per S and destination D in S's SPT, D != S, with exactly ONE primary slot e (E = nbr[e]):
 *   entry j < min(tq_count[e], max_pairs) with q = tq_q[e][j] protects D iff  d(q, D) < d(q, E) + d(E, D)   (d(q, .) from q's row,
 *                 d(E, D) from row nbr_row[e] of the forward set)
 *   choice        among the protecting entries the smallest tq_metric[e][j] + d(q, D) (64 bits), then the smaller j
 *   tn_kind u8    0 unless D has exactly one primary; else, in this order: HSPF_TN_D_LFA the given alt_flags have
 *                 HSPF_LFA_NODE_PROTECT | HSPF_TN_D_NONE the slot is no candidate | HSPF_TN_D_LAST_HOP D == E | HSPF_TN_D_PQ
 *                 nd_kind_in is given and says HSPF_NP_D_PQ (the one-segment repair stands; nothing is chosen here) |
 *                 HSPF_TN_D_PAIR an entry was chosen | HSPF_TN_D_NONE
 *   tn_p / tn_q / tn_link / tn_via / tn_metric   for HSPF_TN_D_PAIR the chosen entry's fields and the sum saturated at 0xFFFFFFFE;
 *                 HSPF_NO_ROOT / HSPF_NO_ROOT / HSPF_LFA_NO_SLOT / HSPF_LFA_NO_SLOT / 0 otherwise
 *   tn_set u32    optional (NULL skips the table): bit j = entry j protects D, for the D that reach the test; 0 otherwise
 *   tn_coverage [n_prot][6], counted on the device: destinations with exactly one primary, then the five classes by their numbers.
 * Argument errors of both — everything the RLFA-node pair rejects, max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS, and for the
 * select call a NULL graph, n_vertices not the graph's, a NULL space table — return HSPF_E_INVAL with a text in hspf_last_error
 * that names the function, before anything is launched.  Each call stages once, enqueues everything on the context's stream and
 * synchronises once at the end.
 *
 * From tn_* to a label stack: INTEGRATION.md §5o.
 *
 * OUT OF SCOPE: LAN pseudonodes as the protected node; LAN-safe release paths (the NP / NXP release paths are derived against E
 * only — the limitation of hspf_rlfa_node_select_device — so on the tables of hspf_rlfa_lan_device the tunnel may still cross the
 * slot's pseudonode); forced adjacencies across a pseudonode (q must be a router in p's own row); segment
 * lists longer than two; SRLGs.  Per prefix: hspf_routes_backup_node_device, below. */
#define HSPF_TILFA_NODE_MAX_PAIRS 32u
#define HSPF_TN_D_LFA             1u           /* tn_kind */
#define HSPF_TN_D_PQ              2u
#define HSPF_TN_D_LAST_HOP        3u
#define HSPF_TN_D_NONE            4u
#define HSPF_TN_D_PAIR            5u
#define HSPF_TN_COVERAGE_WORDS    6u
typedef struct {                 /* DEVICE pointers; stride = 64 * n_mask_words                               */
  uint32_t *tq_q;                /* [n_prot][stride][max_pairs]  HSPF_NO_ROOT-padded                           */
  uint32_t *tq_p;                /* [n_prot][stride][max_pairs]  HSPF_NO_ROOT-padded                           */
  uint32_t *tq_link;             /* [n_prot][stride][max_pairs]  position in p's row; HSPF_LFA_NO_SLOT padding */
  uint32_t *tq_via;              /* [n_prot][stride][max_pairs]  HSPF_RLFA_VIA_SELF or a slot; HSPF_LFA_NO_SLOT padding */
  uint32_t *tq_metric;           /* [n_prot][stride][max_pairs]  entry metric; 0 padding                       */
  uint32_t *tq_count;            /* [n_prot][stride]             ALL q with a qualifying link (may exceed max_pairs) */
} hspf_tilfa_node_sel;
int hspf_tilfa_node_select_device(hspf_ctx *ctx, const hspf_graph *g, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                  const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                  const hspf_lfa_protect *prot, uint32_t n_prot, uint32_t lfa_flags,
                                  const uint8_t *space_flags_dev, uint32_t max_pairs, hspf_tilfa_node_sel *out_dev);
typedef struct {                 /* DEVICE pointers                                                            */
  uint8_t  *tn_kind;             /* [n_prot][n_vertices]                                                       */
  uint32_t *tn_p;                /* [n_prot][n_vertices]                                                       */
  uint32_t *tn_q;                /* [n_prot][n_vertices]                                                       */
  uint32_t *tn_link;             /* [n_prot][n_vertices]                                                       */
  uint32_t *tn_via;              /* [n_prot][n_vertices]                                                       */
  uint32_t *tn_metric;           /* [n_prot][n_vertices]                                                       */
  uint32_t *tn_set;              /* [n_prot][n_vertices] bit j = list entry j protects; or NULL                */
  uint32_t *tn_coverage;         /* [n_prot][HSPF_TN_COVERAGE_WORDS]                                           */
} hspf_tilfa_node_out;
int hspf_tilfa_node_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                           const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                           const hspf_lfa_protect *prot, uint32_t n_prot,
                           const uint32_t *ydist_dev, const uint32_t *y_roots /* HOST */, uint32_t n_yrows,
                           const hspf_tilfa_node_sel *sel_dev, uint32_t max_pairs,
                           const uint8_t *alt_flags_in_dev, const uint8_t *nd_kind_in_dev, hspf_tilfa_node_out *out_dev);

/* ---- per-prefix node-protecting backups on device: new symbol, same ABI number -------------------------------------------------
 * hspf_rlfa_node_device and hspf_tilfa_node_device protect destination VERTICES; what a RIB installs is per PREFIX, and
 * hspf_routes_backup_device gives node protection only through the HSPF_LFA_NODE_PROTECT bit of a directly connected alternate (its
 * remote fallback is the LINK repair of the primary, which need not survive the neighbour's failure).  For a prefix with one
 * advertiser the per-vertex answer at that advertiser is the prefix's; for a multi-homed prefix it is not: whether a listed node
 * Y reaches the prefix without the neighbour E is a question about Y's distance to the PREFIX, the minimum over all advertisers.
 * The sharpest case is an anycast prefix advertised by E itself and by a router behind it: per vertex the destination is E
 * (HSPF_NP_D_LAST_HOP, nothing to protect), per prefix a PQ node reaches the other advertiser without touching E.
 * hspf_routes_backup_node_device is that join, per (protected root, prefix).  It takes no graph.
 *
 * Inputs.  The forward table set and `prot` are exactly those of hspf_lfa_device.  `table` and routes_dev are those of
 * hspf_routes_backup_device, under the same flag rules (HSPF_PFX_ORDERED is rejected, HSPF_PFX_RESIDENT shares the one staged
 * copy, HSPF_PFX_LAST_MIN changes nothing here).  ydist_dev [n_yrows][n_vertices] is `dist` of ONE forward hspf_run_device whose
 * root list was y_roots (HOST array) — the caller's choice, usually the union of the listed PQ nodes and the listed q's;
 * HSPF_NO_ROOT entries are skipped, a vertex listed twice may use either row, a listed node without a row is skipped; the vertex
 * -> row map is built on the device.  rn_sel_dev / max_pq: NULL (no one-segment entries), or what hspf_rlfa_node_select_device
 * wrote for the same `prot`; tn_sel_dev / max_pairs: NULL (no two-segment entries), or what hspf_tilfa_node_select_device wrote;
 * at least one of the two.  bk_in_dev: NULL, or the hspf_backup_out hspf_routes_backup_device wrote for the same `prot` and
 * table; only bk_kind and bk_flags are read.
 *
 * Per protected root S and prefix p whose route exists (routes.best_entry != 0xFFFFFFFF) with exactly ONE primary slot e
 * (popcount of routes.nexthop_mask[p] below n_slots is 1), E = nbr[e]; every sum is evaluated in 64 bits.
 *   d_E(p)      as in hspf_routes_backup_device, from row nbr_row[e] of the forward set: the minimum over the entries (v, m) of p
 *               with v HSPF_RF_IN_SPT in that row and d(E, v) != HSPF_DIST_INF of d(E, v) + m, each sum first saturated at
 *               0xFFFFFFFF under HSPF_PFX_SATURATING
 *   d_Y(p)      for a listed node Y with a row: the minimum over the entries (v, m) of p of ydist[row(Y)][v] + m; an
 *               HSPF_DIST_INF entry contributes nothing (the rows are read as hspf_rlfa_node_device reads them: `dist` alone); each
 *               sum first saturated at 0xFFFFFFFF under HSPF_PFX_SATURATING
 *   entry j protects p   iff  d_Y(p) < d(Y, E) + d_E(p)  with d(Y, E) = ydist[row(Y)][E]; a missing d_Y(p), a missing d_E(p) or an
 *               HSPF_DIST_INF d(Y, E) makes it false.  One-segment entries: j < min(nq_count[e], max_pq), Y = nq_node[e][j];
 *               two-segment entries: j < min(tq_count[e], max_pairs), Y = tq_q[e][j] (the test depends on q alone)
 *   choice      among the protecting one-segment entries the smallest nq_metric[e][j] + d_Y(p), then the smaller j
 *               (HSPF_BN_PQ); ONLY when none protects, the same over the two-segment entries with tq_metric[e][j] + d_q(p)
 *               (HSPF_BN_PAIR): a one-segment repair stands before any pair whatever the cost, as in hspf_tilfa_node_device
 *   bn_kind u8  0 unless the route exists with exactly one primary; else, in this order: HSPF_BN_LFA bk_in_dev is given, its
 *               bk_kind is HSPF_BK_LFA and its bk_flags has HSPF_LFA_NODE_PROTECT | HSPF_BN_NONE the slot is no candidate
 *               (nbr[e] == HSPF_NO_ROOT) | HSPF_BN_PQ | HSPF_BN_PAIR | HSPF_BN_LAST_HOP nothing protects and E's own entry
 *               (v == E) attains d_E(p): the link repair is all there is | HSPF_BN_NONE.
 *               The entries are tested BEFORE the last-hop class — deliberately unlike the per-vertex calls: that is what lets an
 *               anycast prefix on E be protected.  The numbering follows HSPF_TN_D_*.
 * Outputs (DEVICE pointers, [n_prot][n_prefixes] unless stated; "none" is HSPF_NO_ROOT / HSPF_LFA_NO_SLOT / 0 as elsewhere):
 *   bn_primary  the one primary slot e for kinds 1 .. 5, HSPF_LFA_NO_SLOT otherwise
 *   bn_p / bn_q the chosen nodes: HSPF_BN_PQ bn_p == bn_q == the PQ node; HSPF_BN_PAIR tq_p / tq_q of the entry; HSPF_NO_ROOT
 *               otherwise
 *   bn_link     HSPF_BN_PAIR: the position of the forced link in p's row (tq_link); HSPF_LFA_NO_SLOT otherwise
 *   bn_via      nq_via / tq_via of the chosen entry (may be HSPF_RLFA_VIA_SELF); HSPF_LFA_NO_SLOT otherwise
 *   bn_metric   the chosen sum saturated at 0xFFFFFFFE — here a cost to the PREFIX (bk_metric of a remote repair is not); 0 otherwise
 *   bn_set_pq / bn_set_pair   u32, optional (NULL skips the table): bit j = entry j of the one- / two-segment list protects p,
 *               for the prefixes that reach the test (one primary, not HSPF_BN_LFA, the slot a candidate); 0 otherwise.  With
 *               bn_set_pair given the two-segment entries are tested even when a PQ entry was chosen.
 *   bn_coverage u32 [n_prot][HSPF_BN_COVERAGE_WORDS], counted on the device: prefixes with exactly one primary, then classes 1 .. 5.
 * Argument errors — everything hspf_routes_backup_device rejects (without its lfa_flags and tilfa_dev), everything
 * hspf_rlfa_node_device rejects about the y rows (NULL ydist_dev / y_roots, n_yrows == 0, a y_roots entry >= n_vertices that is not
 * HSPF_NO_ROOT), both sel pointers NULL, a NULL array in a given sel or in bk_in_dev (bk_kind, bk_flags), max_pq outside
 * 1 .. HSPF_RLFA_NODE_MAX_PQ with rn_sel_dev given, max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS with tn_sel_dev given (the limit of
 * a sel that is NULL is not read) — return HSPF_E_INVAL with a text in hspf_last_error that names
 * hspf_routes_backup_node_device, before anything is launched.  The call stages once, enqueues everything on the context's stream
 * and synchronises once at the end.
 *
 * From bn_* to a next hop with a label stack: INTEGRATION.md §5p.
 *
 * OUT OF SCOPE: LAN pseudonodes as the protected node; LAN-safe release paths (the limitation of the two select calls); ECMP routes
 * (bn_kind 0; per vertex: hspf_lfa_ecmp_device, per prefix: hspf_routes_backup_ecmp_device, plain mode only); a wave-per-prefix path for prefixes with very many advertisers (one lane walks
 * one prefix); SRLGs. */
#define HSPF_BN_LFA            1u             /* bn_kind */
#define HSPF_BN_PQ             2u
#define HSPF_BN_LAST_HOP       3u
#define HSPF_BN_NONE           4u
#define HSPF_BN_PAIR           5u
#define HSPF_BN_COVERAGE_WORDS 6u
typedef struct {                 /* DEVICE pointers                                                            */
  uint8_t  *bn_kind;             /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_primary;          /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_p;                /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_q;                /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_link;             /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_via;              /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_metric;           /* [n_prot][n_prefixes]                                                       */
  uint32_t *bn_set_pq;           /* [n_prot][n_prefixes] bit j = one-segment entry j protects; or NULL         */
  uint32_t *bn_set_pair;         /* [n_prot][n_prefixes] bit j = two-segment entry j protects; or NULL         */
  uint32_t *bn_coverage;         /* [n_prot][HSPF_BN_COVERAGE_WORDS]                                           */
} hspf_backup_node_out;
int hspf_routes_backup_node_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                   const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                   const hspf_lfa_protect *prot, uint32_t n_prot,
                                   const hspf_prefix_table *table, const hspf_routes *routes_dev,
                                   const uint32_t *ydist_dev, const uint32_t *y_roots /* HOST */, uint32_t n_yrows,
                                   const hspf_rlfa_node_sel *rn_sel_dev, uint32_t max_pq,
                                   const hspf_tilfa_node_sel *tn_sel_dev, uint32_t max_pairs,
                                   const hspf_backup_out *bk_in_dev, hspf_backup_node_out *out_dev);

/* ---- per-prefix SRLG-safe backups on device: new symbol, same ABI number ---------------------------------------------------------
 * hspf_lfa_srlg_device answers per VERTEX; what a RIB installs is per PREFIX, and for a multi-homed prefix the member inequality —
 * like the loop-free one ("per-prefix backup routes", above) — must be held against the distances to the PREFIX: a neighbour whose
 * shortest path to S's attaining vertex avoids the conduit may reach the prefix through another advertiser, over a member.
 * hspf_routes_backup_srlg_device is everything hspf_routes_backup_device is, with the following on top.
 *
 * Inputs.  `srlg` is parallel to `prot` (hspf_srlg, "SRLG-safe alternates", above); the batch and root list are those of
 * hspf_lfa_srlg_device: [S] ++ neighbour routers ++ member endpoints.  At most HSPF_SRLG_MAX_MEMBERS members per slot; the
 * argument checks on `srlg` are the same as there.  tilfa_dev: NULL, or the hspf_tilfa_out of hspf_tilfa_device for the same `prot`;
 * THIS call reads ti_kind, ti_via, ti_metric AND ti_p, ti_link (all five required when tilfa_dev is given; the plain call reads
 * neither of the last two).
 *   d_{b_i}(p)        d_X(p) of the per-prefix section evaluated on row head_row_i; HSPF_PFX_SATURATING is treated as there.
 *   crosses_p(N_k, i) d(N_k, a_i) is finite, d_{b_i}(p) exists, and  d_{N_k}(p) >= d(N_k, a_i) + w_i + d_{b_i}(p)  (64 bits).
 *                     An unreachable member refuses nothing: the SRLG rule, not the LAN rule.
 *   cand(p)           additionally, for every primary slot e in P and every member i of e: i is not local to k (not (tail_i == S and
 *                     pos_i == root_link[k])), and crosses_p(N_k, i) is false.
 *   node(p), downstream and the choice are unchanged, evaluated over the narrowed cand.
 *   fallback          one primary e, no slot chosen.  e without members: exactly the plain call's.  e with members: the per-link
 *                     repair is taken only under HSPF_LFA_SRLG_SAFE_REPAIRS in lfa_flags — the caller's word that tilfa_dev was
 *                     computed from hspf_rlfa_srlg_device's tables.  Then HSPF_TILFA_NODE gives HSPF_BK_NODE; HSPF_TILFA_PAIR gives
 *                     HSPF_BK_PAIR unless (ti_p[e], ti_link[e]) equals (tail_i, pos_i) of a member of e: the forced adjacency is
 *                     itself in the group, and the result is HSPF_BK_NONE with HSPF_BK_SRLG_PAIR_REFUSED.
 * bk_flags gains (next to HSPF_LFA_NODE_PROTECT | HSPF_LFA_DOWNSTREAM; 0x20 and 0x40 stay with the LAN call):
 *   HSPF_LFA_SRLG_REFUSED      some slot met every condition of the plain cand(p) and failed only a member condition
 *   HSPF_BK_SRLG_PRIMARY       some slot in P has at least one member (kinds HSPF_BK_ECMP .. HSPF_BK_NONE)
 *   HSPF_BK_SRLG_PAIR_REFUSED  as above
 * bk_coverage is [n_prot][HSPF_BK_SRLG_COVERAGE_WORDS]: the seven kinds | prefixes with HSPF_BK_SRLG_PRIMARY | with
 * HSPF_LFA_SRLG_REFUSED | with HSPF_BK_SRLG_PAIR_REFUSED.
 * With every mem_ptr all zero all shared outputs equal hspf_routes_backup_device's, words 7 .. 9 are 0, and
 * HSPF_LFA_SRLG_SAFE_REPAIRS has no effect.  No other call rejects or reads bit 0x04 of lfa_flags.
 * Argument errors — everything hspf_routes_backup_device rejects (with ti_p / ti_link among the required tilfa_dev arrays) and
 * everything hspf_lfa_srlg_device rejects in `srlg` — return HSPF_E_INVAL with a text that names hspf_routes_backup_srlg_device,
 * before any kernel is launched.
 *
 * From bk_* to a next hop when SRLGs are configured: INTEGRATION.md §5r.
 *
 * OUT OF SCOPE: a choice for ECMP routes (HSPF_BK_ECMP and the two sets here; per primary and against that primary's own group:
 * hspf_routes_backup_ecmp_srlg_device, below); SRLGs combined with the LAN inequalities (a LAN primary is treated as by hspf_routes_backup_device); SRLGs combined
 * with node-protecting backups (hspf_routes_backup_node_device); per-prefix Q-spaces (the remote repair is the primary LINK's);
 * HSPF_PFX_ORDERED tables (HSPF_E_INVAL); group tables in the fuzz_frr run of tools/gpu_fuzz.py (existing seeds keep their meaning).
 */
#define HSPF_LFA_SRLG_SAFE_REPAIRS   0x04u   /* lfa_flags of hspf_routes_backup_srlg_device; every other call ignores it */
#define HSPF_BK_SRLG_PRIMARY         0x01u   /* bk_flags: some primary slot of the prefix has members */
#define HSPF_BK_SRLG_PAIR_REFUSED    0x02u   /* bk_flags: the primary's two-segment repair forces a member link */
/* HSPF_LFA_SRLG_REFUSED 0x80u is reused in bk_flags */
#define HSPF_BK_SRLG_COVERAGE_WORDS  10u
int hspf_routes_backup_srlg_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                   const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                   const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                                   const hspf_prefix_table *table, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev,
                                   hspf_backup_out *out_dev);

/* ---- per-primary SRLG-safe backups for ECMP prefixes on device: new symbol, same ABI number ------------------------------------
 * hspf_routes_backup_srlg_device stops at a route with two or more primaries (HSPF_BK_ECMP, no choice);
 * hspf_routes_backup_ecmp_device chooses per primary but knows no groups, and its tie order prefers another primary: two
 * equal-cost uplinks in one conduit are handed to each other, and one cut takes both.  hspf_routes_backup_ecmp_srlg_device is
 * everything hspf_routes_backup_ecmp_device is ("per-primary backups for ECMP prefixes", above), with the following on top.
 *
 * Inputs.  Those of hspf_routes_backup_ecmp_device, plus `srlg` parallel to `prot` exactly as in hspf_routes_backup_srlg_device
 * (at most HSPF_SRLG_MAX_MEMBERS members per slot; batch and root list [S] ++ neighbour routers ++ member endpoints).  tilfa_dev:
 * NULL, or the hspf_tilfa_out for the same `prot`; ti_kind, ti_via, ti_metric AND ti_p, ti_link are required when it is given.
 * For a prefix p with popcount(P) >= 2 and a protected primary h in P let M(h) be the members of slot h.  The members of h ALONE
 * count: the entry protects h's link, and its risk group is h's; the members of the other primaries play no part.
 *   crosses_p(N_k, i) as for hspf_routes_backup_srlg_device: d(N_k, a_i) is finite, d_{b_i}(p) exists, and
 *                     d_{N_k}(p) >= d(N_k, a_i) + w_i + d_{b_i}(p)  (64 bits; HSPF_PFX_SATURATING as there).  An unreachable member
 *                     refuses nothing.
 *   cand(h)           additionally, for every member i in M(h): i is not local to k (not (tail_i == S and pos_i == root_link[k])),
 *                     and crosses_p(N_k, i) is false.  The rule is the same whether or not k is itself a primary: a primary whose
 *                     own first link is in h's group is refused as a backup of h.
 *   node(h), downstream and the choice (node, then primary, then sum, then slot) are unchanged, over the narrowed cand(h).
 *   fallback          no slot chosen for h.  h without members: the plain call's.  h with members: the per-link repair is taken
 *                     only under HSPF_LFA_SRLG_SAFE_REPAIRS; then HSPF_TILFA_NODE gives HSPF_BK_NODE, and HSPF_TILFA_PAIR gives
 *                     HSPF_BK_PAIR unless (ti_p[h], ti_link[h]) equals (tail_i, pos_i) of a member of h: then the entry is
 *                     HSPF_BK_NONE with HSPF_BK_SRLG_PAIR_REFUSED.
 * eb_flags gains three bits, on an entry of ANY kind (0x08 / 0x10 / 0x20 keep their meaning):
 *   HSPF_BK_SRLG_PRIMARY       (0x01) h has at least one member
 *   HSPF_LFA_SRLG_REFUSED      (0x80) some slot met every condition of the plain cand(h) and failed only a member condition
 *   HSPF_BK_SRLG_PAIR_REFUSED  (0x02) as above
 * eb_coverage is [n_prot][HSPF_BK_ECMP_SRLG_COVERAGE_WORDS]: the eight words of the plain call (word 7 still counts the prefixes
 * of which every primary has a backup of any kind) | entries with HSPF_BK_SRLG_PRIMARY | with HSPF_LFA_SRLG_REFUSED | with
 * HSPF_BK_SRLG_PAIR_REFUSED.  eb_ptr, *out_total and the capacity convention are exactly the plain call's: they depend on the
 * routes alone.
 * With every mem_ptr all zero every shared output equals hspf_routes_backup_ecmp_device's bit for bit, words 8 .. 10 are 0, and
 * HSPF_LFA_SRLG_SAFE_REPAIRS has no effect.
 * Argument errors — everything hspf_routes_backup_ecmp_device rejects, everything hspf_lfa_srlg_device rejects in `srlg` (17
 * members on a slot among them), ti_p or ti_link NULL when tilfa_dev is given, HSPF_PFX_ORDERED — return HSPF_E_INVAL with a text
 * that names hspf_routes_backup_ecmp_srlg_device, before anything is launched.
 *
 * From eb_* to a backup per next hop when SRLGs are configured: INTEGRATION.md §5u.
 *
 * OUT OF SCOPE: the per-vertex twin (hspf_lfa_ecmp_device with groups); LAN-safe and node-protecting-remote ECMP variants; SRLGs
 * combined with the LAN inequalities; group tables in the fuzz_frr run of tools/gpu_fuzz.py. */
#define HSPF_BK_ECMP_SRLG_COVERAGE_WORDS  11u
int hspf_routes_backup_ecmp_srlg_device(hspf_ctx *ctx, uint32_t n_vertices, uint32_t n_rows, uint32_t n_mask_words,
                                        const uint32_t *dist_dev, const uint16_t *flags_dev, const uint64_t *mask_dev,
                                        const hspf_lfa_protect *prot, const hspf_srlg *srlg, uint32_t n_prot, uint32_t lfa_flags,
                                        const hspf_prefix_table *table, const hspf_routes *routes_dev, const hspf_tilfa_out *tilfa_dev,
                                        uint64_t cap_entries, hspf_backup_ecmp_out *out_dev, uint64_t *out_total);

/* ---- several GPUs --------------------------------------------------------------------------
 * SPF roots are independent units over a read-only graph: the graph is replicated on every GPU, whole 64-root
 * wavefront batches are dealt to the ranks (hspf_shard_bounds), every rank runs its slice, and ONE all-gather per
 * table gives every rank the rows of all roots.  The reference has no analogue — its only multi-root caller is the
 * sequential loop of holo-isis/src/flooding/manet.rs:47-69; what this replaces on the holo side is that loop and the
 * per-area fan-out of holo-ospf/src/spf.rs:540-542.
 *
 * A rank is one engine context on one device.  Two job shapes:
 *   single process  hspf_multi_config.unique_id == NULL, world == n_local: the process drives every device (one host
 *                   thread per device inside hspf_multi_run); the gather is direct device-to-device copies over
 *                   xGMI (every device pushes its slice to every other one: the all-to-all pattern a fully
 *                   connected xGMI mesh is built for).  device_ordinals may repeat an ordinal — several contexts and
 *                   streams on one GPU — which is how the path is tested on a one-GPU box.
 *   one process per GPU  (n_local = 1, world = number of processes): rank 0 creates a communicator id with
 *                   hspf_multi_unique_id, the HOST transports its 128 bytes to the other processes (holo would use its
 *                   ibus; bench.py uses torch.distributed), every process calls hspf_multi_init with it; the gather is
 *                   ncclAllGather / ncclBroadcast of RCCL (librccl.so, loaded at run time) on the contexts' streams.
 * Every call is collective over the ranks of the job and synchronous. */
typedef struct hspf_multi hspf_multi;
typedef struct hspf_multi_graph hspf_multi_graph;
#define HSPF_COMM_ID_BYTES 128
typedef struct {
  uint32_t       n_local;          /* devices driven by this process                                              */
  const int     *device_ordinals;  /* [n_local]                                                                   */
  uint32_t       world;            /* ranks of the job                                                            */
  uint32_t       first_rank;       /* rank of local device 0 (local device i is rank first_rank + i)              */
  const uint8_t *unique_id;        /* NULL, or HSPF_COMM_ID_BYTES bytes from hspf_multi_unique_id                 */
} hspf_multi_config;

int         hspf_multi_unique_id(uint8_t id[HSPF_COMM_ID_BYTES]);      /* needs librccl.so                        */
int         hspf_multi_init(const hspf_multi_config *cfg, hspf_multi **out);
/* Detail of the last failed hspf_multi_init on the calling thread (e.g. RCCL's own message); "" if none. */
const char *hspf_multi_init_error(void);
void        hspf_multi_shutdown(hspf_multi *m);
const char *hspf_multi_last_error(const hspf_multi *m);
hspf_ctx   *hspf_multi_ctx(hspf_multi *m, uint32_t local_index);      /* the rank's context, for the one-device calls */
uint32_t    hspf_multi_n_local(const hspf_multi *m);

int  hspf_multi_graph_upload(hspf_multi *m, const hspf_csr *csr, hspf_multi_graph **out);   /* a replica per local device */
int  hspf_multi_graph_patch(hspf_multi *m, hspf_multi_graph *g, const hspf_rows *rows);
void hspf_multi_graph_free(hspf_multi *m, hspf_multi_graph *g);
hspf_graph *hspf_multi_graph_local(hspf_multi_graph *g, uint32_t local_index);

/* [begin, end) of rank `rank` in a list of n_roots roots: whole 64-root batches dealt as evenly as possible, the
 * first n_batches % world ranks take one more, the ragged tail goes to the last rank that has work. */
void hspf_shard_bounds(uint32_t n_roots, uint32_t world, uint32_t rank, uint32_t *begin, uint32_t *end);

/* Areas first, then roots (BASELINE configs[3]): every area is its own graph with its own root list;
 * the (area, 64-root batch) units, in area order, are cut into `world` contiguous runs of equal batch counts, so a
 * rank touches as few areas as possible (it uploads only those) and no batch is split.  Writes one slice per (rank,
 * area) pair that has work, rank-major; returns the number of slices (may exceed cap; nothing beyond cap is written). */
typedef struct { uint32_t rank, area, root_begin, root_end; } hspf_area_slice;
uint32_t hspf_plan_areas(uint32_t n_areas, const uint32_t *roots_per_area, uint32_t world,
                         hspf_area_slice *out, uint32_t cap);

/* Number of mask words the roots of the whole job need (every rank passes the same list). */
int hspf_multi_mask_words(hspf_multi *m, const hspf_multi_graph *g, const uint32_t *roots, uint32_t n_roots, uint32_t *out_words);

/* Sharded run.  `all[i]` (i < n_local) are DEVICE buffers on local device i sized for ALL n_roots roots, laid out as
 * for hspf_run_device ([n_roots][n_vertices] ...).  Rank r computes rows [begin_r, end_r) straight into its own
 * buffers; the tables selected in `gather` (present in `all`) are then all-gathered in place, so that on return every
 * local device holds those tables for every root.  gather = 0: no exchange (each device holds its own rows only). */
#define HSPF_GATHER_DIST   0x1u
#define HSPF_GATHER_HOPS   0x2u
#define HSPF_GATHER_FLAGS  0x4u
#define HSPF_GATHER_MASK   0x8u
/* The exchange is enqueued on the ranks' communication streams and the call returns when the ranks' OWN rows are
 * complete: the gather then overlaps whatever the caller does next — typically the next hspf_multi_run into a second
 * set of tables.  A later hspf_multi_run into the SAME tables first waits for their pending gather; hspf_multi_wait
 * waits for all of them (call it before reading gathered rows). */
#define HSPF_GATHER_ASYNC  0x100u
int hspf_multi_wait(hspf_multi *m);
int hspf_multi_run(hspf_multi *m, const hspf_multi_graph *g, const uint32_t *roots, uint32_t n_roots,
                   uint32_t run_flags, hspf_result *all, uint32_t gather);

/* hspf_multi_run in two halves (ABI 6): the first hands every local device's slice to a lane of its context
 * (hspf_run_device_async) and returns a ticket; the second waits for the slices and then does what hspf_multi_run does
 * with `gather` (the exchange, synchronous or HSPF_GATHER_ASYNC).  Several tickets may be in flight, into DIFFERENT
 * tables; wait for them in ticket order (every rank the same order: the exchange is a collective).  No host thread is
 * created per call: the lanes' threads live as long as the context (hspf_multi_run itself uses them when it drives
 * more than one local device). */
int hspf_multi_run_async(hspf_multi *m, const hspf_multi_graph *g, const uint32_t *roots, uint32_t n_roots,
                         uint32_t run_flags, const hspf_result *all, uint64_t *ticket);
int hspf_multi_run_wait(hspf_multi *m, uint64_t ticket, hspf_result *all, uint32_t gather);

/* The collective on its own, for any per-root table (route tables after hspf_routes_device: "a single all-gather of
 * per-root route tables", BASELINE north_star): tables[i] is a device buffer on local device i of n_roots rows of
 * row_bytes bytes whose rows [begin_r, end_r) are filled; on return all rows are, on every device. */
int hspf_multi_allgather_rows(hspf_multi *m, void *const *tables, size_t row_bytes, uint32_t n_roots);

/* Statistics of the last hspf_multi_run on local device i (as hspf_get_stats). */
int hspf_multi_get_stats(const hspf_multi *m, uint32_t local_index, hspf_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* HOLO_SPF_HIP_H */
