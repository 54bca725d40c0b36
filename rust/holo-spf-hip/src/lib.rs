//! Safe wrapper over the C ABI of libholo_spf_hip.so (`sys`, generated from include/holo_spf_hip.h).
//!
//! One `Engine` per protocol-instance thread (holo-protocol/src/lib.rs:427-430: an instance runs on its own OS thread
//! and processes its messages sequentially): `Send`, not `Sync`.  Every failure is an integer code turned into
//! `Error`; callers log it and keep their existing CPU loop — the convention of
//! `Error::SpfRootNotFound(area).log(); return;` (holo-ospf/src/spf.rs:605-610).  Nothing panics or aborts across the
//! boundary (the library catches C++ exceptions at every entry point).
//!
//! NOT compiled in the engine repository's image (no cargo / rustc there): kept mechanical, one C call per method.

pub mod sys;

use std::ffi::{CStr, c_void};
use std::fmt;
use std::marker::PhantomData;
use std::ptr;

/// An `HSPF_E_*` code with the library's detail text.
#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub detail: String,
}

impl fmt::Display for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        let what = unsafe { CStr::from_ptr(sys::hspf_strerror(self.code)) }.to_string_lossy();
        write!(f, "holo-spf-hip: {} ({}): {}", what, self.code, self.detail)
    }
}

impl std::error::Error for Error {}

impl Error {
    /// Logged, never fatal: the caller falls back to its own loop.
    pub fn log(&self) {
        tracing::warn!(code = self.code, detail = %self.detail, "SPF engine error, falling back to the CPU loop");
    }
}

/// The caller's CSR of one area / level x topology (include/holo_spf_hip.h `hspf_csr`): vertex index = rank in the
/// reference's VertexId order, links in LSA / LSP order, already filtered by the per-protocol rules.
#[derive(Debug, Default, Clone, PartialEq, Eq)]
pub struct Csr {
    pub row_ptr: Vec<u32>,
    pub col: Vec<u32>,
    pub metric: Vec<u32>,
    pub vflags: Vec<u8>,
    pub max_path_metric: u32,
}

impl Csr {
    pub fn n_vertices(&self) -> u32 {
        self.vflags.len() as u32
    }
    pub fn row(&self, v: u32) -> (&[u32], &[u32]) {
        let (a, b) = (self.row_ptr[v as usize] as usize, self.row_ptr[v as usize + 1] as usize);
        (&self.col[a..b], &self.metric[a..b])
    }
    /// Does vertex `t` list `v` (the two-way check of the reference loop, cost not compared)?
    pub fn links_back(&self, t: u32, v: u32) -> bool {
        self.row(t).0.contains(&v)
    }
}

/// The LSDB records of `Engine::upload_keyed` (include/holo_spf_hip.h `hspf_keyed_lsdb`).
#[derive(Debug, Default, Clone, PartialEq, Eq)]
pub struct KeyedLsdb {
    pub vertex_key: Vec<u64>,
    pub row_ptr: Vec<u32>,
    pub target_key: Vec<u64>,
    pub metric: Vec<u32>,
    pub vflags: Vec<u8>,
    pub max_path_metric: u32,
}

/// One replaced row of `Graph::patch`.
#[derive(Debug, Clone)]
pub struct RowPatch {
    pub vertex: u32,
    pub col: Vec<u32>,
    pub metric: Vec<u32>,
    pub vflags: u8,
}

/// Page-locked host memory from `hspf_host_alloc`: packed results cross the bus at full speed into it.
pub struct PinnedBuf<'e> {
    eng: &'e Engine,
    p: *mut c_void,
    bytes: usize,
}

impl PinnedBuf<'_> {
    pub fn len(&self) -> usize {
        self.bytes
    }
    pub fn is_empty(&self) -> bool {
        self.bytes == 0
    }
}

impl Drop for PinnedBuf<'_> {
    fn drop(&mut self) {
        unsafe { sys::hspf_host_free(self.eng.ctx, self.p) }
    }
}

/// Device memory from `hspf_device_alloc` (tables that stay in HBM between `run_device`, `routes_device` and
/// `routes_changed`).
pub struct DeviceBuf<'e> {
    eng: &'e Engine,
    p: *mut c_void,
    bytes: usize,
}

impl DeviceBuf<'_> {
    pub fn to_host<T: Copy + Default>(&self, count: usize) -> Result<Vec<T>, Error> {
        let mut v = vec![T::default(); count];
        let bytes = count * std::mem::size_of::<T>();
        // a real check: the pool hands out blocks by size class, a count beyond what was asked for would read a
        // neighbour's block — or past the allocation — in a release build
        if bytes > self.bytes {
            return Err(self.eng.err(sys::HSPF_E_INVAL));
        }
        let rc = unsafe { sys::hspf_device_to_host(self.eng.ctx, v.as_mut_ptr() as *mut c_void, self.p, bytes) };
        if rc != sys::HSPF_OK {
            return Err(self.eng.err(rc));
        }
        Ok(v)
    }
}

impl Drop for DeviceBuf<'_> {
    fn drop(&mut self) {
        // back to the engine's pool (freed with the engine)
        self.eng.pool.borrow_mut().entry(Engine::size_class(self.bytes)).or_default().push(self.p);
    }
}

/// Where the per-(root, vertex) values of a run live on the host.
enum Repr<'e> {
    /// `hspf_run`: four arrays, 8 + 8 `words` bytes per (root, vertex).
    Full { words: u32, dist: Vec<u32>, hops: Vec<u16>, flags: Vec<u16>, mask: Vec<u64> },
    /// `hspf_run_packed` (ABI 7): ONE 4- or 8-byte word per (root, vertex) in page-locked memory + the run's field
    /// positions; a vertex is decoded where it is looked at (include/holo_spf_hip.h "packed results").
    Packed { buf: PinnedBuf<'e>, layout: sys::hspf_packed_layout, root_status: Vec<u8> },
}

/// Per (root, vertex) results of a run, row-major `[root][vertex]`.
pub struct Tables<'e> {
    pub n_roots: u32,
    pub n_vertices: u32,
    repr: Repr<'e>,
}

impl<'e> Tables<'e> {
    #[inline]
    fn at(&self, root: u32, v: u32) -> usize {
        root as usize * self.n_vertices as usize + v as usize
    }
    #[inline]
    fn word(&self, buf: &PinnedBuf<'e>, layout: &sys::hspf_packed_layout, i: usize) -> u64 {
        // (hspf_packed_word of the header)
        unsafe {
            if layout.word_bytes == 4 {
                *(buf.p as *const u32).add(i) as u64
            } else {
                *(buf.p as *const u64).add(i)
            }
        }
    }
    pub fn in_spt(&self, root: u32, v: u32) -> bool {
        match &self.repr {
            Repr::Full { flags, .. } => flags[self.at(root, v)] & sys::HSPF_RF_IN_SPT as u16 != 0,
            Repr::Packed { buf, layout, .. } => self.word(buf, layout, self.at(root, v)) < layout.not_reached,
        }
    }
    /// The root went through the sequential kernel (its pop order is not the static one): `Engine::pop_ranks`.
    pub fn exact(&self, root: u32, v: u32) -> bool {
        match &self.repr {
            Repr::Full { flags, .. } => flags[self.at(root, v)] & sys::HSPF_RF_EXACT as u16 != 0,
            Repr::Packed { root_status, .. } => root_status[root as usize] & sys::HSPF_ROOT_EXACT as u8 != 0 && self.in_spt(root, v),
        }
    }
    pub fn dist(&self, root: u32, v: u32) -> u32 {
        match &self.repr {
            Repr::Full { dist, .. } => dist[self.at(root, v)],
            Repr::Packed { buf, layout, .. } => {
                let w = self.word(buf, layout, self.at(root, v));
                if w < layout.not_reached { (w >> layout.dist_shift) as u32 } else { sys::HSPF_DIST_INF }
            }
        }
    }
    pub fn hops(&self, root: u32, v: u32) -> u16 {
        match &self.repr {
            Repr::Full { hops, .. } => hops[self.at(root, v)],
            Repr::Packed { buf, layout, .. } => {
                let w = self.word(buf, layout, self.at(root, v));
                if w < layout.not_reached { ((w >> layout.hops_shift) & layout.hops_mask as u64) as u16 } else { 0 }
            }
        }
    }
    /// First-hop slots of (root, v), ascending.
    pub fn slots(&self, root: u32, v: u32) -> impl Iterator<Item = u32> + '_ {
        let (words, base) = match &self.repr {
            Repr::Full { words, .. } => (*words as usize, self.at(root, v) * *words as usize),
            Repr::Packed { .. } => (1usize, 0usize),
        };
        (0..words).flat_map(move |w| {
            let mut m = match &self.repr {
                Repr::Full { mask, .. } => mask[base + w],
                Repr::Packed { buf, layout, .. } => {
                    let x = self.word(buf, layout, self.at(root, v));
                    if x < layout.not_reached { x & ((1u64 << layout.mask_bits) - 1) } else { 0 }
                }
            };
            std::iter::from_fn(move || {
                if m == 0 {
                    return None;
                }
                let b = m.trailing_zeros();
                m &= m - 1;
                Some(w as u32 * 64 + b)
            })
        })
    }
    /// The page-locked buffer of a packed result, for the next run of the same size (`Engine::run_packed`).
    pub fn into_buffer(self) -> Option<PinnedBuf<'e>> {
        match self.repr {
            Repr::Packed { buf, .. } => Some(buf),
            Repr::Full { .. } => None,
        }
    }
}

/// The candidate table of one root (`hspf_lfa_candidates`): one entry per first-hop slot.
pub struct LfaCandidates {
    pub root: u32,
    pub nbr: Vec<u32>,
    pub cost: Vec<u32>,
    pub root_link: Vec<u32>,
    pub cflags: Vec<u8>,
}

/// The shared-risk members of every first-hop slot of one root (`hspf_srlg_members`): slot k's members are entries
/// `mem_ptr[k] .. mem_ptr[k + 1]` of the columns.  `tail_row` / `head_row` (the rows of the SPTs rooted at the members'
/// endpoints) are the caller's to fill: it makes the run.
pub struct SrlgMembers {
    pub mem_ptr: Vec<u32>,
    pub tail: Vec<u32>,
    pub pos: Vec<u32>,
    pub head: Vec<u32>,
    pub cost: Vec<u32>,
    pub tail_row: Vec<u32>,
    pub head_row: Vec<u32>,
}

/// Loop-free alternates of the protected roots of one `Engine::lfa_device` call, row-major `[protected root][vertex]`.
pub struct Lfa {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub words: u32,
    pub alt_slot: Vec<u32>,
    pub alt_metric: Vec<u32>,
    pub alt_flags: Vec<u8>,
    pub cand_mask: Vec<u64>,
    pub node_mask: Vec<u64>,
    pub coverage: Vec<u32>,
}

impl Lfa {
    /// The chosen alternate of (protected root `i`, destination `v`): (slot, metric), `None` when there is none.
    pub fn alternate(&self, i: usize, v: u32) -> Option<(u32, u32)> {
        let k = i * self.n_vertices as usize + v as usize;
        (self.alt_slot[k] != sys::HSPF_LFA_NO_SLOT).then(|| (self.alt_slot[k], self.alt_metric[k]))
    }
    pub fn node_protecting(&self, i: usize, v: u32) -> bool {
        self.alt_flags[i * self.n_vertices as usize + v as usize] as u32 & sys::HSPF_LFA_NODE_PROTECT != 0
    }
}

/// One entry of `LfaEcmp`: the alternate of one primary slot of an ECMP destination.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct EcmpAlternate {
    pub primary: u32,
    /// The chosen slot and `cost[slot] + d(N, D)`; `None`: this primary has no alternate.
    pub alternate: Option<(u32, u32)>,
    /// `HSPF_LFA_LINK_PROTECT | HSPF_LFA_NODE_PROTECT | HSPF_LFA_DOWNSTREAM | HSPF_LFA_EA_PRIMARY`
    pub flags: u8,
}

/// Per-primary alternates of the ECMP destinations of one `Engine::lfa_ecmp_device` call: a stream in CSR form over
/// (protected root, destination), the entries of one destination in ascending primary slot order.
pub struct LfaEcmp {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub ea_ptr: Vec<u32>,
    pub ea_primary: Vec<u32>,
    pub ea_slot: Vec<u32>,
    pub ea_metric: Vec<u32>,
    pub ea_flags: Vec<u8>,
    pub ea_coverage: Vec<u32>,
}

impl LfaEcmp {
    /// The entries of (protected root `i`, destination `d`): empty unless `d` has two or more primary slots.
    pub fn alternates(&self, i: usize, d: u32) -> Vec<EcmpAlternate> {
        let k = i * self.n_vertices as usize + d as usize;
        (self.ea_ptr[k] as usize..self.ea_ptr[k + 1] as usize)
            .map(|e| EcmpAlternate {
                primary: self.ea_primary[e],
                alternate: (self.ea_slot[e] != sys::HSPF_LFA_NO_SLOT).then(|| (self.ea_slot[e], self.ea_metric[e])),
                flags: self.ea_flags[e],
            })
            .collect()
    }
}

/// Remote loop-free alternates (RFC 7490) of the protected roots of one `Engine::rlfa_device` call.  Slots are strided by
/// `slot_stride` = 64 * mask words per protected root.
pub struct Rlfa {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub slot_stride: u32,
    pub pq_node: Vec<u32>,
    pub pq_via: Vec<u32>,
    pub pq_metric: Vec<u32>,
    pub pq_counts: Vec<u32>,
    pub space_flags: Vec<u8>,
    pub space_via: Vec<u32>,
    pub rl_node: Vec<u32>,
    pub rl_via: Vec<u32>,
    pub rl_coverage: Vec<u32>,
}

impl Rlfa {
    /// The PQ node of (protected root `i`, slot `e`): (node, via, release metric), `None` when there is none.  `via` is a slot
    /// of the root or `HSPF_RLFA_VIA_SELF`.
    pub fn pq_node(&self, i: usize, e: u32) -> Option<(u32, u32, u32)> {
        let k = i * self.slot_stride as usize + e as usize;
        (self.pq_node[k] != sys::HSPF_NO_ROOT).then(|| (self.pq_node[k], self.pq_via[k], self.pq_metric[k]))
    }
    /// The remote alternate of (protected root `i`, destination `v`): (PQ node, via), `None` when there is none.
    pub fn remote_alternate(&self, i: usize, v: u32) -> Option<(u32, u32)> {
        let k = i * self.n_vertices as usize + v as usize;
        (self.rl_node[k] != sys::HSPF_NO_ROOT).then(|| (self.rl_node[k], self.rl_via[k]))
    }
}

/// Two-segment repair paths (TI-LFA, link protection) of the protected roots of one `Engine::tilfa_device` call.  Slots are
/// strided by `slot_stride` = 64 * mask words per protected root.
pub struct Tilfa {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub slot_stride: u32,
    pub ti_kind: Vec<u8>,
    pub ti_p: Vec<u32>,
    pub ti_q: Vec<u32>,
    pub ti_via: Vec<u32>,
    pub ti_link: Vec<u32>,
    pub ti_metric: Vec<u32>,
    pub ti_counts: Vec<u32>,
    pub td_kind: Vec<u8>,
    pub td_coverage: Vec<u32>,
}

/// What `tilfa_pc_device` returns: per (protected root, destination) the repair along the post-convergence path
/// (`hspf_tilfa_pc_device`).  Arrays are `[n_protected][n_vertices]`, the hop arrays with
/// `HSPF_TIPC_MAX_ADJ` entries per destination.
#[derive(Debug, Clone)]
pub struct TilfaPc {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub tp_kind: Vec<u8>,
    pub tp_p: Vec<u32>,
    pub tp_via: Vec<u32>,
    pub tp_q: Vec<u32>,
    pub tp_n_adj: Vec<u8>,
    pub tp_hop_pos: Vec<u32>,
    pub tp_hop_head: Vec<u32>,
    pub tp_metric: Vec<u32>,
    pub tp_flags: Vec<u8>,
    pub tp_coverage: Vec<u32>,
}

impl TilfaPc {
    /// The repair of destination `d` of protected root `i`: `(via, p, [(tail, position, head)], q)` — the Node-SID of `p` out of
    /// `via` (`HSPF_LFA_NO_SLOT`: `p` is the root, no node segment), the Adj-SID of every listed link, then `q`'s own path.
    /// `None` unless `HSPF_TIPC_D_REPAIR`.
    pub fn segments(&self, i: usize, d: usize) -> Option<(u32, u32, Vec<(u32, u32, u32)>, u32)> {
        let c = i * self.n_vertices as usize + d;
        if i >= self.n_protected as usize || d >= self.n_vertices as usize || self.tp_kind[c] as u32 != sys::HSPF_TIPC_D_REPAIR {
            return None;
        }
        let a = sys::HSPF_TIPC_MAX_ADJ as usize;
        let mut tail = self.tp_p[c];
        let mut hops = Vec::with_capacity(self.tp_n_adj[c] as usize);
        for h in 0..(self.tp_n_adj[c] as usize).min(a) {
            let head = self.tp_hop_head[c * a + h];
            hops.push((tail, self.tp_hop_pos[c * a + h], head));
            tail = head;
        }
        Some((self.tp_via[c], self.tp_p[c], hops, self.tp_q[c]))
    }
}

impl Tilfa {
    /// The repair of (protected root `i`, slot `e`): (via, p, forced link of p's row or `None` for a single node, total),
    /// `None` when there is none.  The segment list is the Node-SID of p, then the Adj-SID of that link.
    pub fn repair(&self, i: usize, e: u32) -> Option<(u32, u32, Option<u32>, u32)> {
        let k = i * self.slot_stride as usize + e as usize;
        (self.ti_kind[k] as u32 != sys::HSPF_TILFA_NONE).then(|| {
            let link = (self.ti_kind[k] as u32 == sys::HSPF_TILFA_PAIR).then(|| self.ti_link[k]);
            (self.ti_via[k], self.ti_p[k], link, self.ti_metric[k])
        })
    }
}

/// Node-protecting remote loop-free alternates (RFC 8102) of the protected roots of one `Engine::rlfa_node_device` call.  Slots
/// are strided by `slot_stride` = 64 * mask words per protected root, lists by `max_pq` per slot.
pub struct RlfaNode {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub slot_stride: u32,
    pub max_pq: u32,
    pub nq_node: Vec<u32>,
    pub nq_via: Vec<u32>,
    pub nq_metric: Vec<u32>,
    pub nq_count: Vec<u32>,
    pub y_roots: Vec<u32>,
    pub nd_kind: Vec<u8>,
    pub nd_node: Vec<u32>,
    pub nd_via: Vec<u32>,
    pub nd_metric: Vec<u32>,
    pub nd_set: Vec<u32>,
    pub nd_coverage: Vec<u32>,
}

impl RlfaNode {
    /// The tunnel that protects destination `d` of protected root `i` against the failure of its primary neighbour:
    /// (PQ node, via, cost), `None` unless its class is `HSPF_NP_D_PQ`.
    pub fn repair(&self, i: usize, d: u32) -> Option<(u32, u32, u32)> {
        let k = i * self.n_vertices as usize + d as usize;
        (self.nd_kind[k] as u32 == sys::HSPF_NP_D_PQ).then(|| (self.nd_node[k], self.nd_via[k], self.nd_metric[k]))
    }
}

/// Two-segment node-protecting repairs of the protected roots of one `Engine::tilfa_node_device` call.  Slots are strided by
/// `slot_stride` = 64 * mask words per protected root, lists by `max_pairs` per slot.
pub struct TilfaNode {
    pub n_protected: u32,
    pub n_vertices: u32,
    pub slot_stride: u32,
    pub max_pairs: u32,
    pub tq_q: Vec<u32>,
    pub tq_p: Vec<u32>,
    pub tq_link: Vec<u32>,
    pub tq_via: Vec<u32>,
    pub tq_metric: Vec<u32>,
    pub tq_count: Vec<u32>,
    pub y_roots: Vec<u32>,
    pub tn_kind: Vec<u8>,
    pub tn_p: Vec<u32>,
    pub tn_q: Vec<u32>,
    pub tn_link: Vec<u32>,
    pub tn_via: Vec<u32>,
    pub tn_metric: Vec<u32>,
    pub tn_set: Vec<u32>,
    pub tn_coverage: Vec<u32>,
}

impl TilfaNode {
    /// The two-segment repair that protects destination `d` of protected root `i` against the failure of its primary neighbour:
    /// (p, via, position of the forced link in p's row, q, cost), `None` unless its class is `HSPF_TN_D_PAIR`.
    pub fn repair(&self, i: usize, d: u32) -> Option<(u32, u32, u32, u32, u32)> {
        let k = i * self.n_vertices as usize + d as usize;
        (self.tn_kind[k] as u32 == sys::HSPF_TN_D_PAIR).then(|| (self.tn_p[k], self.tn_via[k], self.tn_link[k], self.tn_q[k], self.tn_metric[k]))
    }
}

/// Per-prefix node-protecting backups of the protected roots of one `Engine::routes_backup_node_device` call, `n_prefixes` cells
/// per protected root.
pub struct BackupNode {
    pub n_protected: u32,
    pub n_prefixes: u32,
    pub y_roots: Vec<u32>,
    pub bn_kind: Vec<u8>,
    pub bn_primary: Vec<u32>,
    pub bn_p: Vec<u32>,
    pub bn_q: Vec<u32>,
    pub bn_link: Vec<u32>,
    pub bn_via: Vec<u32>,
    pub bn_metric: Vec<u32>,
    pub bn_set_pq: Vec<u32>,
    pub bn_set_pair: Vec<u32>,
    pub bn_coverage: Vec<u32>,
}

impl BackupNode {
    /// The repair that protects prefix `p` of protected root `i` against the failure of its primary neighbour: (tunnel end,
    /// via, position of the forced link in its row or `None` for a PQ node, q, cost to the prefix); `None` unless its kind is
    /// `HSPF_BN_PQ` or `HSPF_BN_PAIR`.
    pub fn repair(&self, i: usize, p: u32) -> Option<(u32, u32, Option<u32>, u32, u32)> {
        let k = i * self.n_prefixes as usize + p as usize;
        let kind = self.bn_kind[k] as u32;
        (kind == sys::HSPF_BN_PQ || kind == sys::HSPF_BN_PAIR)
            .then(|| (self.bn_p[k], self.bn_via[k], (kind == sys::HSPF_BN_PAIR).then(|| self.bn_link[k]), self.bn_q[k], self.bn_metric[k]))
    }
}

/// `hspf_run_device` results left in HBM: input of `routes_device` / `ancestors_device`.
pub struct DeviceTables<'e> {
    pub n_roots: u32,
    pub n_vertices: u32,
    pub words: u32,
    dist: DeviceBuf<'e>,
    hops: DeviceBuf<'e>,
    flags: DeviceBuf<'e>,
    mask: DeviceBuf<'e>,
}

impl<'e> DeviceTables<'e> {
    /// Distance, hops and flags only (the first-hop slot replay reads nothing else; half the bytes of `to_host`): the mask
    /// accessors of the returned tables see empty masks.
    pub fn to_host_without_masks(&self) -> Result<Tables<'e>, Error> {
        let cells = self.n_roots as usize * self.n_vertices as usize;
        Ok(Tables {
            n_roots: self.n_roots,
            n_vertices: self.n_vertices,
            repr: Repr::Full {
                words: self.words,
                dist: self.dist.to_host(cells)?,
                hops: self.hops.to_host(cells)?,
                flags: self.flags.to_host(cells)?,
                mask: vec![0u64; cells * self.words as usize],
            },
        })
    }

    /// The copy the host side still needs for next-hop resolution (one root: 1.6 MB at 100 000 vertices).
    pub fn to_host(&self) -> Result<Tables<'e>, Error> {
        let cells = self.n_roots as usize * self.n_vertices as usize;
        Ok(Tables {
            n_roots: self.n_roots,
            n_vertices: self.n_vertices,
            repr: Repr::Full {
                words: self.words,
                dist: self.dist.to_host(cells)?,
                hops: self.hops.to_host(cells)?,
                flags: self.flags.to_host(cells)?,
                mask: self.mask.to_host(cells * self.words as usize)?,
            },
        })
    }
}

/// The (vertex, prefix, metric) advertisements of one level / topology as CSR by prefix (`hspf_prefix_table`): entries of
/// a prefix in ascending vertex index = the reference's `Spt::iter` order.  Root independent: built once per LSDB
/// generation, kept on the device (`HSPF_PFX_RESIDENT`).
#[derive(Debug, Default, Clone)]
pub struct PrefixTable {
    pub pfx_ptr: Vec<u32>,
    pub pfx_vertex: Vec<u32>,
    pub pfx_metric: Vec<u32>,
    pub flags: u32,
}

impl PrefixTable {
    pub fn n_prefixes(&self) -> u32 {
        self.pfx_ptr.len().saturating_sub(1) as u32
    }
}

/// One entry of `BackupEcmp`: the backup of one primary slot of an ECMP prefix.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct EcmpBackup {
    pub primary: u32,
    /// `HSPF_BK_LFA`, `HSPF_BK_NODE`, `HSPF_BK_PAIR` or `HSPF_BK_NONE`
    pub kind: u8,
    /// `HSPF_BK_LFA`: the chosen slot and `cost[slot] + d_N(p)`; `HSPF_BK_NODE` / `HSPF_BK_PAIR`: `ti_via` of the primary and the
    /// repair's cost to the primary's neighbour; `None`: this primary has no backup.
    pub backup: Option<(u32, u32)>,
    /// `HSPF_LFA_NODE_PROTECT | HSPF_LFA_DOWNSTREAM | HSPF_LFA_EA_PRIMARY` for `HSPF_BK_LFA`
    pub flags: u8,
}

/// Per-primary backups of the ECMP prefixes of one `Engine::routes_backup_ecmp_device` call: a stream in CSR form over
/// (protected root, prefix), the entries of one prefix in ascending primary slot order.
pub struct BackupEcmp {
    pub n_protected: u32,
    pub n_prefixes: u32,
    pub eb_ptr: Vec<u32>,
    pub eb_primary: Vec<u32>,
    pub eb_kind: Vec<u8>,
    pub eb_slot: Vec<u32>,
    pub eb_metric: Vec<u32>,
    pub eb_flags: Vec<u8>,
    pub eb_coverage: Vec<u32>,
}

impl BackupEcmp {
    /// The entries of (protected root `i`, prefix `p`): empty unless the route of `p` has two or more primary slots.
    pub fn entries(&self, i: usize, p: u32) -> Vec<EcmpBackup> {
        let k = i * self.n_prefixes as usize + p as usize;
        (self.eb_ptr[k] as usize..self.eb_ptr[k + 1] as usize)
            .map(|e| EcmpBackup {
                primary: self.eb_primary[e],
                kind: self.eb_kind[e],
                backup: (self.eb_kind[e] as u32 != sys::HSPF_BK_NONE).then(|| (self.eb_slot[e], self.eb_metric[e])),
                flags: self.eb_flags[e],
            })
            .collect()
    }
}

/// Per-prefix backup routes of one `routes_backup_device` call, on the host: `[n_protected][n_prefixes]` (the masks with `words`
/// words per entry), `bk_coverage` `[n_protected][HSPF_BK_COVERAGE_WORDS]`; `bk_kind` holds `HSPF_BK_*`.
pub struct Backup {
    pub n_protected: u32,
    pub n_prefixes: u32,
    pub words: u32,
    pub bk_kind: Vec<u8>,
    pub bk_primary: Vec<u32>,
    pub bk_slot: Vec<u32>,
    pub bk_metric: Vec<u32>,
    pub bk_flags: Vec<u8>,
    pub bk_cand_mask: Vec<u64>,
    pub bk_node_mask: Vec<u64>,
    pub bk_coverage: Vec<u32>,
}

/// Route tables of one `routes_device` call (or an uploaded set) in HBM: `hspf_routes`.
pub struct DeviceRoutes<'e> {
    pub n_roots: u32,
    pub n_prefixes: u32,
    pub words: u32,
    best_metric: DeviceBuf<'e>,
    best_entry: DeviceBuf<'e>,
    nexthop_mask: DeviceBuf<'e>,
}

impl DeviceRoutes<'_> {
    /// Metric, owner entry (all ones: no route) and next-hop mask words of every (root, prefix), on the host: what a caller
    /// that keeps its own RIB needs when it has to drop these tables (changes that put nothing on the wire leave no record).
    pub fn to_host(&self) -> Result<(Vec<u32>, Vec<u32>, Vec<u64>), Error> {
        let rp = self.n_roots as usize * self.n_prefixes as usize;
        Ok((self.best_metric.to_host(rp)?, self.best_entry.to_host(rp)?, self.nexthop_mask.to_host(rp * self.words as usize)?))
    }
    fn raw(&self) -> sys::hspf_routes {
        sys::hspf_routes {
            best_metric: self.best_metric.p as *mut u32,
            best_entry: self.best_entry.p as *mut u32,
            nexthop_mask: self.nexthop_mask.p as *mut u64,
        }
    }
}

/// One changed (root, prefix) pair of `routes_changed`: what the route IS (`new_*`) and what it WAS (`old_*`).
#[derive(Debug, Clone)]
pub struct RouteRecord {
    pub root: u32,
    pub prefix: u32,
    pub action: u32, // sys::HSPF_DIFF_INSTALL | sys::HSPF_DIFF_WITHDRAW; from routes_events(.., true) also sys::HSPF_DIFF_SILENT
    pub new_metric: u32,
    pub new_entry: u32, // 0xFFFFFFFF: the prefix has no route any more
    pub new_mask: Vec<u64>,
    pub old_metric: u32,
    pub old_entry: u32, // 0xFFFFFFFF: there was no route
    pub old_mask: Vec<u64>,
}

impl RouteRecord {
    pub fn slots(mask: &[u64]) -> impl Iterator<Item = u32> + '_ {
        mask.iter().enumerate().flat_map(|(w, &m)| {
            let mut m = m;
            std::iter::from_fn(move || {
                if m == 0 {
                    return None;
                }
                let b = m.trailing_zeros();
                m &= m - 1;
                Some(w as u32 * 64 + b)
            })
        })
    }
}

/// A `run_packed_async` in flight: buffer and status array stay here until `wait_packed` turns them into `Tables`.
pub struct PackedTicket<'e> {
    eng: &'e Engine,
    ticket: u64,
    buf: Option<PinnedBuf<'e>>,
    root_status: Option<Box<[u8]>>,
    n_roots: u32,
    n_vertices: u32,
}

/// A ticket that is dropped without `wait_packed` (an early `?`, an unwinding panic) must not free its page-locked buffer
/// and status array under the lane thread and the copy stream that still write them (a use-after-free reachable
/// from safe code): the drop waits for the run first; the fields go afterwards.
impl Drop for PackedTicket<'_> {
    fn drop(&mut self) {
        if self.buf.is_some() {
            unsafe { sys::hspf_wait(self.eng.ctx, self.ticket, ptr::null_mut()) };
        }
    }
}

/// Level-L ancestor bit sets of every (root, vertex) of a hop-count run (`hspf_ancestors_device`).
#[derive(Debug, Default, Clone)]
pub struct AncestorSets {
    pub n_vertices: u32,
    pub words: u32,
    pub level_rank: Vec<u32>,  // [root][vertex]: rank among the root's level-L routers, u32::MAX elsewhere
    pub level_count: Vec<u32>, // [root]; u32::MAX: no sets for this root (sequential kernel)
    pub anc: Vec<u64>,         // [root][vertex][words]
}

impl AncestorSets {
    pub fn available(&self, root: u32) -> bool {
        self.level_count[root as usize] != u32::MAX
    }
    /// `Spt::is_on_path(ancestor, descendant)` for a level-L router `ancestor` of root row `root`.
    pub fn is_on_path(&self, root: u32, ancestor: u32, descendant: u32) -> Option<bool> {
        let rank = self.level_rank[root as usize * self.n_vertices as usize + ancestor as usize];
        if rank == u32::MAX || !self.available(root) {
            return None;
        }
        let base = (root as usize * self.n_vertices as usize + descendant as usize) * self.words as usize;
        Some(self.anc[base + (rank / 64) as usize] >> (rank % 64) & 1 != 0)
    }
}

pub struct Engine {
    ctx: *mut sys::hspf_ctx,
    /// Device blocks of dropped `DeviceBuf`s, by size class (64 KB steps), handed out again by `device_alloc`: a running
    /// instance makes the same few allocations every SPF event, and `hipMalloc` / `hipFree` cost 10-50 us each and
    /// synchronise the device (the compiled C++ twin's `HipPool`: LSP change -> messages 0.94 -> 0.81 ms).  Every engine call
    /// that touches a block is synchronous, so a returned block is idle.
    pool: std::cell::RefCell<std::collections::BTreeMap<usize, Vec<*mut c_void>>>,
    /// Records the previous `routes_events` produced: sizes the buffer of the next call.
    events_hint: std::cell::Cell<usize>,
}

// One OS thread per protocol instance; a context is used by exactly one thread at a time.
unsafe impl Send for Engine {}

pub struct Graph<'e> {
    eng: &'e Engine,
    g: *mut sys::hspf_graph,
    pub n: u32,
    _not_sync: PhantomData<*mut ()>,
}

impl Engine {
    fn err(&self, code: i32) -> Error {
        let detail = unsafe { CStr::from_ptr(sys::hspf_last_error(self.ctx)) }.to_string_lossy().into_owned();
        Error { code, detail }
    }

    pub fn new(device: i32) -> Result<Self, Error> {
        if unsafe { sys::hspf_abi_version() } != sys::HSPF_ABI_VERSION {
            return Err(Error { code: sys::HSPF_E_INTERNAL, detail: "libholo_spf_hip.so: ABI version mismatch".into() });
        }
        let mut ctx = ptr::null_mut();
        let rc = unsafe { sys::hspf_init(device, &mut ctx) };
        if rc != sys::HSPF_OK {
            return Err(Error { code: rc, detail: "hspf_init".into() });
        }
        Ok(Engine { ctx, pool: Default::default(), events_hint: Default::default() })
    }

    /// `HOLO_SPF_HIP_DEVICE=<ordinal>`; unset or unusable => `None` => today's code path, byte for byte.
    pub fn from_env() -> Option<Self> {
        let dev = std::env::var("HOLO_SPF_HIP_DEVICE").ok()?.parse::<i32>().ok()?;
        match Engine::new(dev) {
            Ok(e) => Some(e),
            Err(e) => {
                e.log();
                None
            }
        }
    }

    /// `hspf_lfa_candidates`: the candidate table of `root`, one entry per first-hop slot — pure host arithmetic on the CSR
    /// (no device).  `nbr[k] == HSPF_NO_ROOT`: slot k is no candidate (network target, the root itself, one-way link).
    pub fn lfa_candidates(csr: &Csr, root: u32) -> Result<LfaCandidates, Error> {
        let c = sys::hspf_csr {
            n_vertices: csr.n_vertices(),
            n_edges: csr.col.len() as u32,
            row_ptr: csr.row_ptr.as_ptr(),
            col: csr.col.as_ptr(),
            metric: csr.metric.as_ptr(),
            vflags: csr.vflags.as_ptr(),
            max_path_metric: csr.max_path_metric,
        };
        let mut total = 0u32;
        let k = unsafe { sys::hspf_lfa_candidates(&c, root, 0, ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), &mut total) };
        if k < 0 {
            return Err(Error { code: k, detail: "hspf_lfa_candidates".into() });
        }
        let k = k as usize;
        let mut out = LfaCandidates { root, nbr: vec![0; k], cost: vec![0; k], root_link: vec![0; k], cflags: vec![0; k] };
        let rc = unsafe {
            sys::hspf_lfa_candidates(&c, root, k as u32, out.nbr.as_mut_ptr(), out.cost.as_mut_ptr(), out.root_link.as_mut_ptr(), out.cflags.as_mut_ptr(), &mut total)
        };
        if rc < 0 {
            return Err(Error { code: rc, detail: "hspf_lfa_candidates".into() });
        }
        Ok(out)
    }

    /// `hspf_lfa_lan_candidates`: per first-hop slot of `root` the network vertex its `root_link` leads to over a two-way link,
    /// `HSPF_NO_ROOT` for a point-to-point link — pure host arithmetic on the CSR (no device).
    pub fn lfa_lan_candidates(csr: &Csr, root: u32) -> Result<Vec<u32>, Error> {
        let c = sys::hspf_csr {
            n_vertices: csr.n_vertices(),
            n_edges: csr.col.len() as u32,
            row_ptr: csr.row_ptr.as_ptr(),
            col: csr.col.as_ptr(),
            metric: csr.metric.as_ptr(),
            vflags: csr.vflags.as_ptr(),
            max_path_metric: csr.max_path_metric,
        };
        let mut total = 0u32;
        let k = unsafe { sys::hspf_lfa_lan_candidates(&c, root, 0, ptr::null_mut(), &mut total) };
        if k < 0 {
            return Err(Error { code: k, detail: "hspf_lfa_lan_candidates".into() });
        }
        let mut lan = vec![0u32; k as usize];
        let rc = unsafe { sys::hspf_lfa_lan_candidates(&c, root, k as u32, lan.as_mut_ptr(), &mut total) };
        if rc < 0 {
            return Err(Error { code: rc, detail: "hspf_lfa_lan_candidates".into() });
        }
        Ok(lan)
    }

    /// `hspf_srlg_members`: per first-hop slot of `root` the other links that share a group id with the link of the root's row
    /// the slot stands behind — pure host arithmetic on the CSR (no device).  `grp_ptr` has one entry per link and one more.
    pub fn srlg_members(csr: &Csr, root: u32, grp_ptr: &[u32], grp: &[u32]) -> Result<SrlgMembers, Error> {
        if grp_ptr.len() != csr.col.len() + 1 || grp_ptr.last().map_or(true, |e| *e as usize > grp.len()) {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "srlg_members: grp_ptr / grp do not match the links".into() });
        }
        let c = sys::hspf_csr {
            n_vertices: csr.n_vertices(),
            n_edges: csr.col.len() as u32,
            row_ptr: csr.row_ptr.as_ptr(),
            col: csr.col.as_ptr(),
            metric: csr.metric.as_ptr(),
            vflags: csr.vflags.as_ptr(),
            max_path_metric: csr.max_path_metric,
        };
        let (mut slots, mut total) = (0u32, 0u32);
        let k = unsafe {
            sys::hspf_srlg_members(&c, root, grp_ptr.as_ptr(), grp.as_ptr(), 0, 0, ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), &mut slots, &mut total)
        };
        if k < 0 {
            return Err(Error { code: k, detail: "hspf_srlg_members".into() });
        }
        let m = total as usize;
        let mut out = SrlgMembers { mem_ptr: vec![0; k as usize + 1], tail: vec![0; m], pos: vec![0; m], head: vec![0; m], cost: vec![0; m], tail_row: Vec::new(), head_row: Vec::new() };
        let rc = unsafe {
            sys::hspf_srlg_members(&c, root, grp_ptr.as_ptr(), grp.as_ptr(), k as u32, total, out.mem_ptr.as_mut_ptr(), out.tail.as_mut_ptr(), out.pos.as_mut_ptr(), out.head.as_mut_ptr(), out.cost.as_mut_ptr(), &mut slots, &mut total)
        };
        if rc < 0 {
            return Err(Error { code: rc, detail: "hspf_srlg_members".into() });
        }
        Ok(out)
    }

    /// The `hspf_srlg` array of an SRLG call: `srlgs[i]` belongs to `protect[i]`, with `tail_row` / `head_row` filled.
    fn srlg_raw(who: &str, protect: &[(u32, &LfaCandidates, &[u32])], srlgs: &[&SrlgMembers]) -> Result<Vec<sys::hspf_srlg>, Error> {
        let fits = |c: &LfaCandidates, m: &SrlgMembers| {
            let t = m.mem_ptr.last().map_or(0, |e| *e as usize);
            m.mem_ptr.len() == c.nbr.len() + 1 && [&m.tail, &m.pos, &m.head, &m.cost, &m.tail_row, &m.head_row].iter().all(|x| x.len() >= t)
        };
        if srlgs.len() != protect.len() || protect.iter().zip(srlgs).any(|((_, c, _), m)| !fits(c, m)) {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: format!("{who}: the member lists do not match the slot arrays of the protected roots") });
        }
        Ok(srlgs.iter().map(|m| sys::hspf_srlg {
            mem_ptr: m.mem_ptr.as_ptr(),
            tail: m.tail.as_ptr(),
            pos: m.pos.as_ptr(),
            head: m.head.as_ptr(),
            cost: m.cost.as_ptr(),
            tail_row: m.tail_row.as_ptr(),
            head_row: m.head_row.as_ptr(),
        }).collect())
    }

    /// `hspf_lfa_srlg_device`: `lfa_device` whose alternates neither start on nor cross a link that shares a risk group with a
    /// primary's first link.  `coverage` has `HSPF_LFA_SRLG_COVERAGE_WORDS` words per root; `alt_flags` may carry
    /// `HSPF_LFA_SRLG_REFUSED`.
    pub fn lfa_srlg_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], srlgs: &[&SrlgMembers],
                           ignore_overload: bool, with_masks: bool) -> Result<Lfa, Error> {
        self.lfa_device_with(tables, protect, None, Some(srlgs), ignore_overload, with_masks)
    }

    /// The `hspf_lfa_lan` array of a LAN call: `lans[i]` = (`lan`, `lan_row`) of `protect[i]`, one entry per slot each.
    fn lan_raw(who: &str, protect: &[(u32, &LfaCandidates, &[u32])], lans: &[(&[u32], &[u32])]) -> Result<Vec<sys::hspf_lfa_lan>, Error> {
        if lans.len() != protect.len() || protect.iter().zip(lans).any(|((_, c, _), (l, r))| l.len() != c.nbr.len() || r.len() != c.nbr.len()) {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: format!("{who}: lan / lan_row do not match the slot arrays of the protected roots") });
        }
        Ok(lans.iter().map(|(l, r)| sys::hspf_lfa_lan { lan: l.as_ptr(), lan_row: r.as_ptr() }).collect())
    }

    /// `hspf_lfa_lan_device`: `lfa_device` with loop-freeness towards the pseudonode of every primary's LAN (RFC 5286 section
    /// 3.3).  `lans[i]` = (`lfa_lan_candidates` of the root, per slot the row of the SPT rooted at that LAN).  `coverage` has
    /// `HSPF_LFA_LAN_COVERAGE_WORDS` words per root; `alt_flags` may carry `HSPF_LFA_LAN_PRIMARY` / `HSPF_LFA_LAN_REFUSED`.
    pub fn lfa_lan_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], lans: &[(&[u32], &[u32])],
                          ignore_overload: bool, with_masks: bool) -> Result<Lfa, Error> {
        self.lfa_device_with(tables, protect, Some(lans), None, ignore_overload, with_masks)
    }

    /// `hspf_lfa_device`: loop-free alternates (RFC 5286) of every protected root from the rows of `tables` (a previous
    /// `run_device` whose roots hold each protected root and its neighbour routers).  `protect[i]` = (row of the root's SPT,
    /// its candidate table, `nbr_row[k]` = row of the SPT rooted at `nbr[k]`).  The results come back on the host; the SPT
    /// tables never leave the device.
    pub fn lfa_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], ignore_overload: bool, with_masks: bool) -> Result<Lfa, Error> {
        self.lfa_device_with(tables, protect, None, None, ignore_overload, with_masks)
    }

    /// The frame of `lfa_device` (`lans` and `srlgs` None), `lfa_lan_device` and `lfa_srlg_device` (at most one of the two).
    fn lfa_device_with(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], lans: Option<&[(&[u32], &[u32])]>,
                       srlgs: Option<&[&SrlgMembers]>, ignore_overload: bool, with_masks: bool) -> Result<Lfa, Error> {
        let (n, w, np) = (tables.n_vertices as usize, tables.words as usize, protect.len());
        let lan_raw = match lans { Some(l) => Some(Self::lan_raw("lfa_lan_device", protect, l)?), None => None };
        let srlg_raw = match srlgs { Some(m) => Some(Self::srlg_raw("lfa_srlg_device", protect, m)?), None => None };
        let cov_words = if lans.is_some() { sys::HSPF_LFA_LAN_COVERAGE_WORDS } else if srlgs.is_some() { sys::HSPF_LFA_SRLG_COVERAGE_WORDS } else { sys::HSPF_LFA_COVERAGE_WORDS } as usize;
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "lfa_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let cells = np * n;
        let slot = self.device_alloc(cells * 4)?;
        let metric = self.device_alloc(cells * 4)?;
        let flags = self.device_alloc(cells)?;
        let cov = self.device_alloc(np * cov_words * 4)?;
        let masks = if with_masks { Some((self.device_alloc(cells * w * 8)?, self.device_alloc(cells * w * 8)?)) } else { None };
        let mut out = sys::hspf_lfa_out {
            alt_slot: slot.p as *mut u32,
            alt_metric: metric.p as *mut u32,
            alt_flags: flags.p as *mut u8,
            cand_mask: masks.as_ref().map_or(ptr::null_mut(), |m| m.0.p as *mut u64),
            node_mask: masks.as_ref().map_or(ptr::null_mut(), |m| m.1.p as *mut u64),
            coverage: cov.p as *mut u32,
        };
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 };
        let (dist, flags_in, mask) = (tables.dist.p as *const u32, tables.flags.p as *const u16, tables.mask.p as *const u64);
        let rc = unsafe {
            match (&lan_raw, &srlg_raw) {
                (Some(l), _) => {
                    sys::hspf_lfa_lan_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), l.as_ptr(), np as u32, lfa_flags, &mut out)
                }
                (None, Some(m)) => {
                    sys::hspf_lfa_srlg_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), m.as_ptr(), np as u32, lfa_flags, &mut out)
                }
                (None, None) => sys::hspf_lfa_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), np as u32, lfa_flags, &mut out),
            }
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Lfa {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            words: tables.words,
            alt_slot: slot.to_host(cells)?,
            alt_metric: metric.to_host(cells)?,
            alt_flags: flags.to_host(cells)?,
            cand_mask: match &masks { Some(m) => m.0.to_host(cells * w)?, None => Vec::new() },
            node_mask: match &masks { Some(m) => m.1.to_host(cells * w)?, None => Vec::new() },
            coverage: cov.to_host(np * cov_words)?,
        })
    }

    /// `hspf_lfa_ecmp_device`: for every destination with two or more primary slots and every one of those primaries, the
    /// alternate of that primary and what it protects (RFC 5286 sections 3.4, 3.6).  `tables` and `protect` as for
    /// `lfa_device`.  Two calls: the first sizes the stream (`ea_ptr` and the total), the second fills it.
    pub fn lfa_ecmp_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], ignore_overload: bool) -> Result<LfaEcmp, Error> {
        let (n, np) = (tables.n_vertices as usize, protect.len());
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "lfa_ecmp_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let cov_words = sys::HSPF_LFA_ECMP_COVERAGE_WORDS as usize;
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 };
        let (dist, flags_in, mask) = (tables.dist.p as *const u32, tables.flags.p as *const u16, tables.mask.p as *const u64);
        let ea_ptr = self.device_alloc((np * n + 1) * 4)?;
        let mut out = sys::hspf_lfa_ecmp_out {
            ea_ptr: ea_ptr.p as *mut u32,
            ea_primary: ptr::null_mut(),
            ea_slot: ptr::null_mut(),
            ea_metric: ptr::null_mut(),
            ea_flags: ptr::null_mut(),
            ea_coverage: ptr::null_mut(),
        };
        let mut total: u64 = 0;
        let rc = unsafe {
            sys::hspf_lfa_ecmp_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), np as u32, lfa_flags, 0, &mut out, &mut total)
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let cap = total as usize;
        let mut res = LfaEcmp {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            ea_ptr: Vec::new(),
            ea_primary: Vec::new(),
            ea_slot: Vec::new(),
            ea_metric: Vec::new(),
            ea_flags: Vec::new(),
            ea_coverage: vec![0; np * cov_words],
        };
        if cap == 0 {
            res.ea_ptr = ea_ptr.to_host(np * n + 1)?;
            return Ok(res);
        }
        let primary = self.device_alloc(cap * 4)?;
        let slot = self.device_alloc(cap * 4)?;
        let metric = self.device_alloc(cap * 4)?;
        let flags = self.device_alloc(cap)?;
        let cov = self.device_alloc(np * cov_words * 4)?;
        out.ea_primary = primary.p as *mut u32;
        out.ea_slot = slot.p as *mut u32;
        out.ea_metric = metric.p as *mut u32;
        out.ea_flags = flags.p as *mut u8;
        out.ea_coverage = cov.p as *mut u32;
        let rc = unsafe {
            sys::hspf_lfa_ecmp_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), np as u32, lfa_flags, total, &mut out, &mut total)
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        res.ea_ptr = ea_ptr.to_host(np * n + 1)?;
        res.ea_primary = primary.to_host(cap)?;
        res.ea_slot = slot.to_host(cap)?;
        res.ea_metric = metric.to_host(cap)?;
        res.ea_flags = flags.to_host(cap)?;
        res.ea_coverage = cov.to_host(np * cov_words)?;
        Ok(res)
    }

    /// `hspf_csr_transpose`: the reversed graph (row t lists the sources of t's incoming links by ascending source, then by
    /// position in the source's row) with `vflags` and `max_path_metric` reused — pure host arithmetic.  Of a run on it only
    /// `dist` has a meaning: the distance TO the root.
    pub fn csr_transpose(csr: &Csr) -> Result<Csr, Error> {
        let c = sys::hspf_csr {
            n_vertices: csr.n_vertices(),
            n_edges: csr.col.len() as u32,
            row_ptr: csr.row_ptr.as_ptr(),
            col: csr.col.as_ptr(),
            metric: csr.metric.as_ptr(),
            vflags: csr.vflags.as_ptr(),
            max_path_metric: csr.max_path_metric,
        };
        let mut out = Csr {
            row_ptr: vec![0; csr.row_ptr.len()],
            col: vec![0; csr.col.len()],
            metric: vec![0; csr.col.len()],
            vflags: csr.vflags.clone(),
            max_path_metric: csr.max_path_metric,
        };
        let rc = unsafe { sys::hspf_csr_transpose(&c, out.row_ptr.as_mut_ptr(), out.col.as_mut_ptr(), out.metric.as_mut_ptr()) };
        if rc != sys::HSPF_OK {
            return Err(Error { code: rc, detail: "hspf_csr_transpose".into() });
        }
        Ok(out)
    }

    /// `hspf_rlfa_device`: the PQ node of every (protected root, slot) and the remote alternate of every destination with one
    /// primary.  `tables`: the forward run; `reverse`: the run of the SAME roots on the upload of `csr_transpose` (pass
    /// `tables` again on a graph whose costs are symmetric); `protect` as for `lfa_device`; `lfa`: what `lfa_device` returned
    /// for the same `protect`, so that only the destinations it left unprotected get a remote alternate.
    pub fn rlfa_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, reverse: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])],
                       ignore_overload: bool, lfa: Option<&Lfa>, with_spaces: bool) -> Result<Rlfa, Error> {
        self.rlfa_device_with(g, tables, reverse, protect, None, None, ignore_overload, lfa, with_spaces)
    }

    /// `hspf_rlfa_lan_device`: `rlfa_device` with P, extended P and Q loop-free towards the pseudonode of every slot's LAN.
    /// `lans` as for `lfa_lan_device`; both table sets come from the run [root] + neighbour routers + LANs and `reverse` is
    /// ALWAYS the run on the upload of `csr_transpose`; `lfa`: what `lfa_lan_device` returned.  `pq_counts` has
    /// `HSPF_RLFA_LAN_COUNT_WORDS` words per slot, `rl_coverage` `HSPF_RLFA_LAN_COVERAGE_WORDS` per root; the result feeds
    /// `tilfa_device` unchanged.
    pub fn rlfa_lan_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, reverse: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])],
                           lans: &[(&[u32], &[u32])], ignore_overload: bool, lfa: Option<&Lfa>, with_spaces: bool) -> Result<Rlfa, Error> {
        self.rlfa_device_with(g, tables, reverse, protect, Some(lans), None, ignore_overload, lfa, with_spaces)
    }

    /// `hspf_rlfa_srlg_device`: `rlfa_device` with P, extended P and Q narrowed to the vertices whose paths cross no member of
    /// the slot's risk group.  `srlgs` as for `lfa_srlg_device`; both table sets come from the run [root] + neighbour routers +
    /// member endpoints; `lfa`: what `lfa_srlg_device` returned.  `pq_counts` has `HSPF_RLFA_SRLG_COUNT_WORDS` words per slot,
    /// `rl_coverage` `HSPF_RLFA_SRLG_COVERAGE_WORDS` per root; the result feeds `tilfa_device` unchanged (the forced link of a
    /// pair is not checked against the members).
    #[allow(clippy::too_many_arguments)]
    pub fn rlfa_srlg_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, reverse: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])],
                            srlgs: &[&SrlgMembers], ignore_overload: bool, lfa: Option<&Lfa>, with_spaces: bool) -> Result<Rlfa, Error> {
        self.rlfa_device_with(g, tables, reverse, protect, None, Some(srlgs), ignore_overload, lfa, with_spaces)
    }

    /// The frame of `rlfa_device` (`lans` and `srlgs` None), `rlfa_lan_device` and `rlfa_srlg_device` (at most one of the two).
    #[allow(clippy::too_many_arguments)]
    fn rlfa_device_with(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, reverse: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])],
                        lans: Option<&[(&[u32], &[u32])]>, srlgs: Option<&[&SrlgMembers]>, ignore_overload: bool, lfa: Option<&Lfa>,
                        with_spaces: bool) -> Result<Rlfa, Error> {
        let (n, np) = (tables.n_vertices as usize, protect.len());
        let who = if lans.is_some() { "rlfa_lan_device" } else if srlgs.is_some() { "rlfa_srlg_device" } else { "rlfa_device" };
        let lan_raw = match lans { Some(l) => Some(Self::lan_raw(who, protect, l)?), None => None };
        let srlg_raw = match srlgs { Some(m) => Some(Self::srlg_raw(who, protect, m)?), None => None };
        let count_words = if lans.is_some() { sys::HSPF_RLFA_LAN_COUNT_WORDS } else if srlgs.is_some() { sys::HSPF_RLFA_SRLG_COUNT_WORDS } else { sys::HSPF_RLFA_COUNT_WORDS } as usize;
        let cov_words = if lans.is_some() { sys::HSPF_RLFA_LAN_COVERAGE_WORDS } else if srlgs.is_some() { sys::HSPF_RLFA_SRLG_COVERAGE_WORDS } else { sys::HSPF_RLFA_COVERAGE_WORDS } as usize;
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 };
        if reverse.n_vertices != tables.n_vertices || reverse.n_roots != tables.n_roots {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: format!("{who}: the two table sets differ in shape") });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: format!("{who}: the slot arrays of a protected root differ in length") });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let stride = 64 * tables.words as usize;
        let (slots, cells) = (np * stride, np * n);
        let pq_node = self.device_alloc(slots * 4)?;
        let pq_via = self.device_alloc(slots * 4)?;
        let pq_metric = self.device_alloc(slots * 4)?;
        let pq_counts = self.device_alloc(slots * count_words * 4)?;
        let rl_node = self.device_alloc(cells * 4)?;
        let rl_via = self.device_alloc(cells * 4)?;
        let rl_cov = self.device_alloc(np * cov_words * 4)?;
        let spaces = if with_spaces { Some((self.device_alloc(slots * n)?, self.device_alloc(slots * n * 4)?)) } else { None };
        let alt = match lfa {
            Some(l) if l.alt_flags.len() == cells => Some(self.device_from(&l.alt_flags)?),
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: format!("{who}: the LFA result is not of this protect list") }),
            None => None,
        };
        let mut out = sys::hspf_rlfa_out {
            pq_node: pq_node.p as *mut u32,
            pq_via: pq_via.p as *mut u32,
            pq_metric: pq_metric.p as *mut u32,
            pq_counts: pq_counts.p as *mut u32,
            space_flags: spaces.as_ref().map_or(ptr::null_mut(), |s| s.0.p as *mut u8),
            space_via: spaces.as_ref().map_or(ptr::null_mut(), |s| s.1.p as *mut u32),
            rl_node: rl_node.p as *mut u32,
            rl_via: rl_via.p as *mut u32,
            rl_coverage: rl_cov.p as *mut u32,
        };
        let (dist, flags_in, mask, rdist) = (tables.dist.p as *const u32, tables.flags.p as *const u16, tables.mask.p as *const u64, reverse.dist.p as *const u32);
        let alt_p = alt.as_ref().map_or(ptr::null(), |a| a.p as *const u8);
        let rc = unsafe {
            match (&lan_raw, &srlg_raw) {
                (Some(l), _) => {
                    sys::hspf_rlfa_lan_device(self.ctx, g.g, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, rdist, raw.as_ptr(), l.as_ptr(), np as u32, lfa_flags, alt_p, &mut out)
                }
                (None, Some(m)) => {
                    sys::hspf_rlfa_srlg_device(self.ctx, g.g, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, rdist, raw.as_ptr(), m.as_ptr(), np as u32, lfa_flags, alt_p, &mut out)
                }
                (None, None) => sys::hspf_rlfa_device(self.ctx, g.g, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, rdist, raw.as_ptr(), np as u32, lfa_flags, alt_p, &mut out),
            }
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Rlfa {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            slot_stride: stride as u32,
            pq_node: pq_node.to_host(slots)?,
            pq_via: pq_via.to_host(slots)?,
            pq_metric: pq_metric.to_host(slots)?,
            pq_counts: pq_counts.to_host(slots * count_words)?,
            space_flags: match &spaces { Some(s) => s.0.to_host(slots * n)?, None => Vec::new() },
            space_via: match &spaces { Some(s) => s.1.to_host(slots * n)?, None => Vec::new() },
            rl_node: rl_node.to_host(cells)?,
            rl_via: rl_via.to_host(cells)?,
            rl_coverage: rl_cov.to_host(np * cov_words)?,
        })
    }

    /// `hspf_tilfa_device`: per (protected root, slot) the cheapest repair that is one PQ node or a node of the extended P-space
    /// plus one forced adjacency into the Q-space.  `g` is the FORWARD graph; `tables`, `reverse`, `protect`, `lfa` as for
    /// `rlfa_device`; `rlfa`: what `rlfa_device` returned for the same `protect` with `with_spaces`.
    pub fn tilfa_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, reverse: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])],
                        ignore_overload: bool, lfa: Option<&Lfa>, rlfa: &Rlfa) -> Result<Tilfa, Error> {
        let (n, np) = (tables.n_vertices as usize, protect.len());
        if reverse.n_vertices != tables.n_vertices || reverse.n_roots != tables.n_roots {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_device: the two table sets differ in shape".into() });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let stride = 64 * tables.words as usize;
        let (slots, cells) = (np * stride, np * n);
        if rlfa.space_flags.len() != slots * n || rlfa.space_via.len() != slots * n {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_device: the RLFA result holds no space tables of this protect list".into() });
        }
        let sp_flags = self.device_from(&rlfa.space_flags)?;
        let sp_via = self.device_from(&rlfa.space_via)?;
        let alt = match lfa {
            Some(l) if l.alt_flags.len() == cells => Some(self.device_from(&l.alt_flags)?),
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_device: the LFA result is not of this protect list".into() }),
            None => None,
        };
        let ti_kind = self.device_alloc(slots)?;
        let ti_p = self.device_alloc(slots * 4)?;
        let ti_q = self.device_alloc(slots * 4)?;
        let ti_via = self.device_alloc(slots * 4)?;
        let ti_link = self.device_alloc(slots * 4)?;
        let ti_metric = self.device_alloc(slots * 4)?;
        let ti_counts = self.device_alloc(slots * sys::HSPF_TILFA_COUNT_WORDS as usize * 4)?;
        let td_kind = self.device_alloc(cells)?;
        let td_cov = self.device_alloc(np * sys::HSPF_TILFA_COVERAGE_WORDS as usize * 4)?;
        let mut out = sys::hspf_tilfa_out {
            ti_kind: ti_kind.p as *mut u8,
            ti_p: ti_p.p as *mut u32,
            ti_q: ti_q.p as *mut u32,
            ti_via: ti_via.p as *mut u32,
            ti_link: ti_link.p as *mut u32,
            ti_metric: ti_metric.p as *mut u32,
            ti_counts: ti_counts.p as *mut u32,
            td_kind: td_kind.p as *mut u8,
            td_coverage: td_cov.p as *mut u32,
        };
        let rc = unsafe {
            sys::hspf_tilfa_device(
                self.ctx,
                g.g,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                reverse.dist.p as *const u32,
                raw.as_ptr(),
                np as u32,
                if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 },
                alt.as_ref().map_or(ptr::null(), |a| a.p as *const u8),
                sp_flags.p as *const u8,
                sp_via.p as *const u32,
                &mut out,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Tilfa {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            slot_stride: stride as u32,
            ti_kind: ti_kind.to_host(slots)?,
            ti_p: ti_p.to_host(slots)?,
            ti_q: ti_q.to_host(slots)?,
            ti_via: ti_via.to_host(slots)?,
            ti_link: ti_link.to_host(slots)?,
            ti_metric: ti_metric.to_host(slots)?,
            ti_counts: ti_counts.to_host(slots * sys::HSPF_TILFA_COUNT_WORDS as usize)?,
            td_kind: td_kind.to_host(cells)?,
            td_coverage: td_cov.to_host(np * sys::HSPF_TILFA_COVERAGE_WORDS as usize)?,
        })
    }

    /// `hspf_tilfa_pc_device`: per destination with one primary slot the repair that follows its post-convergence path.  `g`,
    /// `tables`, `reverse`, `protect`, `lfa`, `rlfa` as for `tilfa_device`; `pc`: the tables of a `run_failures_device` on `g`;
    /// `pc_row[i * 64 * words + e]`: the row of `pc` with `{HSPF_FAIL_ROOT_LINK, root_link[e]}` of protected root `i`, or
    /// `HSPF_NO_ROOT`; `run_flags`: those of that run; `max_walk`: 1 ..= 65535.
    #[allow(clippy::too_many_arguments)]
    pub fn tilfa_pc_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, reverse: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])],
                           ignore_overload: bool, lfa: Option<&Lfa>, rlfa: &Rlfa, pc: &DeviceTables<'_>, pc_row: &[u32], run_flags: u32,
                           max_walk: u32) -> Result<TilfaPc, Error> {
        let (n, np) = (tables.n_vertices as usize, protect.len());
        let stride = 64 * tables.words as usize;
        if reverse.n_vertices != tables.n_vertices || reverse.n_roots != tables.n_roots || pc.n_vertices != tables.n_vertices || pc_row.len() != np * stride {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_pc_device: the table sets or pc_row differ in shape".into() });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_pc_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let (slots, cells, adj) = (np * stride, np * n, sys::HSPF_TIPC_MAX_ADJ as usize);
        if rlfa.space_flags.len() != slots * n || rlfa.space_via.len() != slots * n {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_pc_device: the RLFA result holds no space tables of this protect list".into() });
        }
        let sp_flags = self.device_from(&rlfa.space_flags)?;
        let sp_via = self.device_from(&rlfa.space_via)?;
        let alt = match lfa {
            Some(l) if l.alt_flags.len() == cells => Some(self.device_from(&l.alt_flags)?),
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_pc_device: the LFA result is not of this protect list".into() }),
            None => None,
        };
        let tp_kind = self.device_alloc(cells)?;
        let tp_p = self.device_alloc(cells * 4)?;
        let tp_via = self.device_alloc(cells * 4)?;
        let tp_q = self.device_alloc(cells * 4)?;
        let tp_n_adj = self.device_alloc(cells)?;
        let tp_hop_pos = self.device_alloc(cells * adj * 4)?;
        let tp_hop_head = self.device_alloc(cells * adj * 4)?;
        let tp_metric = self.device_alloc(cells * 4)?;
        let tp_flags = self.device_alloc(cells)?;
        let tp_cov = self.device_alloc(np * sys::HSPF_TIPC_COVERAGE_WORDS as usize * 4)?;
        let mut out = sys::hspf_tilfa_pc_out {
            tp_kind: tp_kind.p as *mut u8,
            tp_p: tp_p.p as *mut u32,
            tp_via: tp_via.p as *mut u32,
            tp_q: tp_q.p as *mut u32,
            tp_n_adj: tp_n_adj.p as *mut u8,
            tp_hop_pos: tp_hop_pos.p as *mut u32,
            tp_hop_head: tp_hop_head.p as *mut u32,
            tp_metric: tp_metric.p as *mut u32,
            tp_flags: tp_flags.p as *mut u8,
            tp_coverage: tp_cov.p as *mut u32,
        };
        let rc = unsafe {
            sys::hspf_tilfa_pc_device(
                self.ctx,
                g.g,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                reverse.dist.p as *const u32,
                raw.as_ptr(),
                np as u32,
                if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 },
                alt.as_ref().map_or(ptr::null(), |a| a.p as *const u8),
                sp_flags.p as *const u8,
                sp_via.p as *const u32,
                pc.dist.p as *const u32,
                pc.n_roots,
                pc_row.as_ptr(),
                run_flags,
                max_walk,
                &mut out,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(TilfaPc {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            tp_kind: tp_kind.to_host(cells)?,
            tp_p: tp_p.to_host(cells)?,
            tp_via: tp_via.to_host(cells)?,
            tp_q: tp_q.to_host(cells)?,
            tp_n_adj: tp_n_adj.to_host(cells)?,
            tp_hop_pos: tp_hop_pos.to_host(cells * adj)?,
            tp_hop_head: tp_hop_head.to_host(cells * adj)?,
            tp_metric: tp_metric.to_host(cells)?,
            tp_flags: tp_flags.to_host(cells)?,
            tp_coverage: tp_cov.to_host(np * sys::HSPF_TIPC_COVERAGE_WORDS as usize)?,
        })
    }

    /// `hspf_rlfa_node_select_device`, one `hspf_run_device` over the ascending union of the listed nodes, then
    /// `hspf_rlfa_node_device`: per destination with one primary the cheapest of the `max_pq` listed PQ nodes whose release path
    /// and whose own path to the destination both avoid the primary's neighbour.  `g` is the FORWARD graph; `tables`, `protect`,
    /// `lfa` as for `rlfa_device`; `rlfa`: what `rlfa_device` returned for the same `protect` with `with_spaces`; `run_flags`: those
    /// `tables` were made with (the PQ-node rows come from a run of the same kind).
    pub fn rlfa_node_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, run_flags: u32, protect: &[(u32, &LfaCandidates, &[u32])],
                            ignore_overload: bool, lfa: Option<&Lfa>, rlfa: &Rlfa, max_pq: u32) -> Result<RlfaNode, Error> {
        let (n, np) = (tables.n_vertices as usize, protect.len());
        if max_pq == 0 || max_pq > sys::HSPF_RLFA_NODE_MAX_PQ {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "rlfa_node_device: max_pq outside 1 .. HSPF_RLFA_NODE_MAX_PQ".into() });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "rlfa_node_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let stride = 64 * tables.words as usize;
        let (slots, cells, m) = (np * stride, np * n, max_pq as usize);
        if rlfa.space_flags.len() != slots * n {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "rlfa_node_device: the RLFA result holds no space tables of this protect list".into() });
        }
        let sp_flags = self.device_from(&rlfa.space_flags)?;
        let alt = match lfa {
            Some(l) if l.alt_flags.len() == cells => Some(self.device_from(&l.alt_flags)?),
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "rlfa_node_device: the LFA result is not of this protect list".into() }),
            None => None,
        };
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 };
        let nq_node = self.device_alloc(slots * m * 4)?;
        let nq_via = self.device_alloc(slots * m * 4)?;
        let nq_metric = self.device_alloc(slots * m * 4)?;
        let nq_count = self.device_alloc(slots * 4)?;
        let mut sel = sys::hspf_rlfa_node_sel {
            nq_node: nq_node.p as *mut u32,
            nq_via: nq_via.p as *mut u32,
            nq_metric: nq_metric.p as *mut u32,
            nq_count: nq_count.p as *mut u32,
        };
        let rc = unsafe {
            sys::hspf_rlfa_node_select_device(
                self.ctx,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                raw.as_ptr(),
                np as u32,
                lfa_flags,
                sp_flags.p as *const u8,
                max_pq,
                &mut sel,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let nodes: Vec<u32> = nq_node.to_host(slots * m)?;
        let mut y_roots: Vec<u32> = nodes.iter().copied().filter(|&v| v != sys::HSPF_NO_ROOT).collect();
        y_roots.sort_unstable();
        y_roots.dedup();
        if y_roots.is_empty() {
            y_roots.push(sys::HSPF_NO_ROOT); // one padding row keeps the arguments of the second call valid
        }
        let y = self.run_device(g, &y_roots, run_flags)?;
        let nd_kind = self.device_alloc(cells)?;
        let nd_node = self.device_alloc(cells * 4)?;
        let nd_via = self.device_alloc(cells * 4)?;
        let nd_metric = self.device_alloc(cells * 4)?;
        let nd_set = self.device_alloc(cells * 4)?;
        let nd_cov = self.device_alloc(np * sys::HSPF_NP_COVERAGE_WORDS as usize * 4)?;
        let mut out = sys::hspf_rlfa_node_out {
            nd_kind: nd_kind.p as *mut u8,
            nd_node: nd_node.p as *mut u32,
            nd_via: nd_via.p as *mut u32,
            nd_metric: nd_metric.p as *mut u32,
            nd_set: nd_set.p as *mut u32,
            nd_coverage: nd_cov.p as *mut u32,
        };
        let rc = unsafe {
            sys::hspf_rlfa_node_device(
                self.ctx,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                raw.as_ptr(),
                np as u32,
                y.dist.p as *const u32,
                y_roots.as_ptr(),
                y_roots.len() as u32,
                &sel,
                max_pq,
                alt.as_ref().map_or(ptr::null(), |a| a.p as *const u8),
                &mut out,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(RlfaNode {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            slot_stride: stride as u32,
            max_pq,
            nq_node: nodes,
            nq_via: nq_via.to_host(slots * m)?,
            nq_metric: nq_metric.to_host(slots * m)?,
            nq_count: nq_count.to_host(slots)?,
            y_roots,
            nd_kind: nd_kind.to_host(cells)?,
            nd_node: nd_node.to_host(cells)?,
            nd_via: nd_via.to_host(cells)?,
            nd_metric: nd_metric.to_host(cells)?,
            nd_set: nd_set.to_host(cells)?,
            nd_coverage: nd_cov.to_host(np * sys::HSPF_NP_COVERAGE_WORDS as usize)?,
        })
    }

    /// `hspf_tilfa_node_select_device`, one `hspf_run_device` over the ascending union of the listed q's, then
    /// `hspf_tilfa_node_device`: per destination with one primary the cheapest of the `max_pairs` listed pairs — a tunnel to p that
    /// avoids the primary's neighbour, one forced adjacency p -> q — whose q reaches the destination without that neighbour.  `g`
    /// is the FORWARD graph; `tables`, `protect`, `lfa`, `rlfa`, `run_flags` as for `rlfa_node_device`; `node`: what
    /// `rlfa_node_device` returned for the same `protect` (its one-segment repairs stand), or `None`.
    pub fn tilfa_node_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, run_flags: u32, protect: &[(u32, &LfaCandidates, &[u32])],
                             ignore_overload: bool, lfa: Option<&Lfa>, rlfa: &Rlfa, node: Option<&RlfaNode>, max_pairs: u32) -> Result<TilfaNode, Error> {
        let (n, np) = (tables.n_vertices as usize, protect.len());
        if max_pairs == 0 || max_pairs > sys::HSPF_TILFA_NODE_MAX_PAIRS {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_node_device: max_pairs outside 1 .. HSPF_TILFA_NODE_MAX_PAIRS".into() });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_node_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let stride = 64 * tables.words as usize;
        let (slots, cells, m) = (np * stride, np * n, max_pairs as usize);
        if rlfa.space_flags.len() != slots * n {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_node_device: the RLFA result holds no space tables of this protect list".into() });
        }
        let sp_flags = self.device_from(&rlfa.space_flags)?;
        let alt = match lfa {
            Some(l) if l.alt_flags.len() == cells => Some(self.device_from(&l.alt_flags)?),
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_node_device: the LFA result is not of this protect list".into() }),
            None => None,
        };
        let nd = match node {
            Some(r) if r.nd_kind.len() == cells => Some(self.device_from(&r.nd_kind)?),
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "tilfa_node_device: the RLFA-node result is not of this protect list".into() }),
            None => None,
        };
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 };
        let tq_q = self.device_alloc(slots * m * 4)?;
        let tq_p = self.device_alloc(slots * m * 4)?;
        let tq_link = self.device_alloc(slots * m * 4)?;
        let tq_via = self.device_alloc(slots * m * 4)?;
        let tq_metric = self.device_alloc(slots * m * 4)?;
        let tq_count = self.device_alloc(slots * 4)?;
        let mut sel = sys::hspf_tilfa_node_sel {
            tq_q: tq_q.p as *mut u32,
            tq_p: tq_p.p as *mut u32,
            tq_link: tq_link.p as *mut u32,
            tq_via: tq_via.p as *mut u32,
            tq_metric: tq_metric.p as *mut u32,
            tq_count: tq_count.p as *mut u32,
        };
        let rc = unsafe {
            sys::hspf_tilfa_node_select_device(
                self.ctx,
                g.g,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                raw.as_ptr(),
                np as u32,
                lfa_flags,
                sp_flags.p as *const u8,
                max_pairs,
                &mut sel,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let qs: Vec<u32> = tq_q.to_host(slots * m)?;
        let mut y_roots: Vec<u32> = qs.iter().copied().filter(|&v| v != sys::HSPF_NO_ROOT).collect();
        y_roots.sort_unstable();
        y_roots.dedup();
        if y_roots.is_empty() {
            y_roots.push(sys::HSPF_NO_ROOT); // one padding row keeps the arguments of the second call valid
        }
        let y = self.run_device(g, &y_roots, run_flags)?;
        let tn_kind = self.device_alloc(cells)?;
        let tn_p = self.device_alloc(cells * 4)?;
        let tn_q = self.device_alloc(cells * 4)?;
        let tn_link = self.device_alloc(cells * 4)?;
        let tn_via = self.device_alloc(cells * 4)?;
        let tn_metric = self.device_alloc(cells * 4)?;
        let tn_set = self.device_alloc(cells * 4)?;
        let tn_cov = self.device_alloc(np * sys::HSPF_TN_COVERAGE_WORDS as usize * 4)?;
        let mut out = sys::hspf_tilfa_node_out {
            tn_kind: tn_kind.p as *mut u8,
            tn_p: tn_p.p as *mut u32,
            tn_q: tn_q.p as *mut u32,
            tn_link: tn_link.p as *mut u32,
            tn_via: tn_via.p as *mut u32,
            tn_metric: tn_metric.p as *mut u32,
            tn_set: tn_set.p as *mut u32,
            tn_coverage: tn_cov.p as *mut u32,
        };
        let rc = unsafe {
            sys::hspf_tilfa_node_device(
                self.ctx,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                raw.as_ptr(),
                np as u32,
                y.dist.p as *const u32,
                y_roots.as_ptr(),
                y_roots.len() as u32,
                &sel,
                max_pairs,
                alt.as_ref().map_or(ptr::null(), |a| a.p as *const u8),
                nd.as_ref().map_or(ptr::null(), |a| a.p as *const u8),
                &mut out,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(TilfaNode {
            n_protected: np as u32,
            n_vertices: tables.n_vertices,
            slot_stride: stride as u32,
            max_pairs,
            tq_q: qs,
            tq_p: tq_p.to_host(slots * m)?,
            tq_link: tq_link.to_host(slots * m)?,
            tq_via: tq_via.to_host(slots * m)?,
            tq_metric: tq_metric.to_host(slots * m)?,
            tq_count: tq_count.to_host(slots)?,
            y_roots,
            tn_kind: tn_kind.to_host(cells)?,
            tn_p: tn_p.to_host(cells)?,
            tn_q: tn_q.to_host(cells)?,
            tn_link: tn_link.to_host(cells)?,
            tn_via: tn_via.to_host(cells)?,
            tn_metric: tn_metric.to_host(cells)?,
            tn_set: tn_set.to_host(cells)?,
            tn_coverage: tn_cov.to_host(np * sys::HSPF_TN_COVERAGE_WORDS as usize)?,
        })
    }

    /// `hspf_routes_backup_device`: per (protected root, prefix) the backup of the route `routes_device` wrote for the same
    /// `tables` and `table` — an alternate slot that is loop-free with respect to the PREFIX, or the repair of the one primary
    /// link out of `tilfa` (what `tilfa_device` returned for the same `protect`; `None`: no remote fallback).  `resident`: the
    /// context still holds `table` from the `routes_device` call.
    pub fn routes_backup_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], ignore_overload: bool,
                                table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>, tilfa: Option<&Tilfa>) -> Result<Backup, Error> {
        self.routes_backup_device_with(tables, protect, None, None, ignore_overload, table, resident, routes, tilfa)
    }

    /// `hspf_routes_backup_ecmp_device`: for every prefix whose route has two or more primary slots and every one of those
    /// primaries, its backup — an alternate slot that is loop-free with respect to the PREFIX (the rule of `lfa_ecmp_device` with
    /// the neighbour's distance to the prefix), or the repair of that primary's link out of `tilfa`.  Inputs as for
    /// `routes_backup_device`.  Two calls: the first sizes the stream (`eb_ptr` and the total), the second fills it.
    #[allow(clippy::too_many_arguments)]
    pub fn routes_backup_ecmp_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], ignore_overload: bool,
                                     table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>, tilfa: Option<&Tilfa>) -> Result<BackupEcmp, Error> {
        self.routes_backup_ecmp_device_with(tables, protect, None, ignore_overload, table, resident, routes, tilfa)
    }

    /// `hspf_routes_backup_ecmp_srlg_device`: `routes_backup_ecmp_device` whose alternate for a primary h neither starts on nor
    /// crosses, on its way to the PREFIX, a member of h's own shared-risk group — the members of h alone count, and another primary
    /// in h's group is refused as h's backup.  `srlgs` as for `lfa_srlg_device` (the tables hold the member endpoints' rows);
    /// `safe_repairs` is `HSPF_LFA_SRLG_SAFE_REPAIRS`.  `eb_flags` carries `HSPF_BK_SRLG_PRIMARY`, `HSPF_LFA_SRLG_REFUSED` and
    /// `HSPF_BK_SRLG_PAIR_REFUSED` on an entry of any kind; `eb_coverage` has `HSPF_BK_ECMP_SRLG_COVERAGE_WORDS` words per root.
    #[allow(clippy::too_many_arguments)]
    pub fn routes_backup_ecmp_srlg_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], srlgs: &[&SrlgMembers],
                                          ignore_overload: bool, safe_repairs: bool, table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>,
                                          tilfa: Option<&Tilfa>) -> Result<BackupEcmp, Error> {
        self.routes_backup_ecmp_device_with(tables, protect, Some((srlgs, safe_repairs)), ignore_overload, table, resident, routes, tilfa)
    }

    /// The frame of `routes_backup_ecmp_device` (`srlg` None) and `routes_backup_ecmp_srlg_device`.
    #[allow(clippy::too_many_arguments)]
    fn routes_backup_ecmp_device_with(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], srlg: Option<(&[&SrlgMembers], bool)>,
                                      ignore_overload: bool, table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>,
                                      tilfa: Option<&Tilfa>) -> Result<BackupEcmp, Error> {
        let (np, pf, w) = (protect.len(), table.n_prefixes() as usize, tables.words as usize);
        let srlg_raw = match srlg { Some((m, _)) => Some(Self::srlg_raw("routes_backup_ecmp_srlg_device", protect, m)?), None => None };
        if routes.n_prefixes != table.n_prefixes() || routes.words != tables.words {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_ecmp_device: the routes are not of this table set and table".into() });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_ecmp_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let slots = np * 64 * w;
        let ti = match tilfa {
            Some(t) if t.ti_kind.len() == slots && t.ti_via.len() == slots && t.ti_metric.len() == slots => {
                Some((self.device_from(&t.ti_kind)?, self.device_from(&t.ti_via)?, self.device_from(&t.ti_metric)?))
            }
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_ecmp_device: the TI-LFA result is not of this protect list".into() }),
            None => None,
        };
        // the SRLG call also reads the forced adjacency of a pair
        let ti_pl = match (tilfa, srlg) {
            (Some(t), Some(_)) if t.ti_p.len() == slots && t.ti_link.len() == slots => Some((self.device_from(&t.ti_p)?, self.device_from(&t.ti_link)?)),
            (Some(_), Some(_)) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_ecmp_srlg_device: the TI-LFA result is not of this protect list".into() }),
            _ => None,
        };
        let ti_raw = ti.as_ref().map(|(k, v, m)| sys::hspf_tilfa_out {
            ti_kind: k.p as *mut u8,
            ti_p: ti_pl.as_ref().map_or(ptr::null_mut(), |x| x.0.p as *mut u32),
            ti_q: ptr::null_mut(),
            ti_via: v.p as *mut u32,
            ti_link: ti_pl.as_ref().map_or(ptr::null_mut(), |x| x.1.p as *mut u32),
            ti_metric: m.p as *mut u32,
            ti_counts: ptr::null_mut(),
            td_kind: ptr::null_mut(),
            td_coverage: ptr::null_mut(),
        });
        let mut t = sys::hspf_prefix_table {
            n_prefixes: table.n_prefixes(),
            n_entries: table.pfx_vertex.len() as u32,
            pfx_ptr: table.pfx_ptr.as_ptr(),
            pfx_vertex: table.pfx_vertex.as_ptr(),
            pfx_metric: table.pfx_metric.as_ptr(),
            flags: table.flags | if resident { sys::HSPF_PFX_RESIDENT } else { 0 },
            pfx_origin: ptr::null(),
            init_exists: ptr::null(),
            init_metric: ptr::null(),
            init_origin: ptr::null(),
        };
        let r = sys::hspf_routes {
            best_metric: routes.best_metric.p as *mut u32,
            best_entry: routes.best_entry.p as *mut u32,
            nexthop_mask: routes.nexthop_mask.p as *mut u64,
        };
        let cov_words = if srlg.is_some() { sys::HSPF_BK_ECMP_SRLG_COVERAGE_WORDS } else { sys::HSPF_BK_ECMP_COVERAGE_WORDS } as usize;
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 }
            | if matches!(srlg, Some((_, true))) { sys::HSPF_LFA_SRLG_SAFE_REPAIRS } else { 0 };
        let (dist, flags_in, mask) = (tables.dist.p as *const u32, tables.flags.p as *const u16, tables.mask.p as *const u64);
        let ti_ptr = ti_raw.as_ref().map_or(ptr::null(), |x| x as *const sys::hspf_tilfa_out);
        let eb_ptr = self.device_alloc((np * pf + 1) * 4)?;
        let mut out = sys::hspf_backup_ecmp_out {
            eb_ptr: eb_ptr.p as *mut u32,
            eb_primary: ptr::null_mut(),
            eb_kind: ptr::null_mut(),
            eb_slot: ptr::null_mut(),
            eb_metric: ptr::null_mut(),
            eb_flags: ptr::null_mut(),
            eb_coverage: ptr::null_mut(),
        };
        let mut total: u64 = 0;
        let rc = unsafe {
            match &srlg_raw {
                None => sys::hspf_routes_backup_ecmp_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, 0, &mut out, &mut total),
                Some(m) => sys::hspf_routes_backup_ecmp_srlg_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), m.as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, 0, &mut out, &mut total),
            }
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let cap = total as usize;
        let mut res = BackupEcmp {
            n_protected: np as u32,
            n_prefixes: table.n_prefixes(),
            eb_ptr: Vec::new(),
            eb_primary: Vec::new(),
            eb_kind: Vec::new(),
            eb_slot: Vec::new(),
            eb_metric: Vec::new(),
            eb_flags: Vec::new(),
            eb_coverage: vec![0; np * cov_words],
        };
        if cap == 0 {
            res.eb_ptr = eb_ptr.to_host(np * pf + 1)?;
            return Ok(res);
        }
        let primary = self.device_alloc(cap * 4)?;
        let kind = self.device_alloc(cap)?;
        let slot = self.device_alloc(cap * 4)?;
        let metric = self.device_alloc(cap * 4)?;
        let flags = self.device_alloc(cap)?;
        let cov = self.device_alloc(np * cov_words * 4)?;
        out.eb_primary = primary.p as *mut u32;
        out.eb_kind = kind.p as *mut u8;
        out.eb_slot = slot.p as *mut u32;
        out.eb_metric = metric.p as *mut u32;
        out.eb_flags = flags.p as *mut u8;
        out.eb_coverage = cov.p as *mut u32;
        t.flags |= sys::HSPF_PFX_RESIDENT; // the sizing call has just staged the table
        let rc = unsafe {
            match &srlg_raw {
                None => sys::hspf_routes_backup_ecmp_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, total, &mut out, &mut total),
                Some(m) => sys::hspf_routes_backup_ecmp_srlg_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), m.as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, total, &mut out, &mut total),
            }
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        res.eb_ptr = eb_ptr.to_host(np * pf + 1)?;
        res.eb_primary = primary.to_host(cap)?;
        res.eb_kind = kind.to_host(cap)?;
        res.eb_slot = slot.to_host(cap)?;
        res.eb_metric = metric.to_host(cap)?;
        res.eb_flags = flags.to_host(cap)?;
        res.eb_coverage = cov.to_host(np * cov_words)?;
        Ok(res)
    }

    /// `hspf_routes_backup_srlg_device`: `routes_backup_device` whose alternates neither start on nor cross, on their way to the
    /// PREFIX, a member of a primary's shared-risk group.  `srlgs` as for `lfa_srlg_device` (the tables hold the member endpoints'
    /// rows); `safe_repairs` is `HSPF_LFA_SRLG_SAFE_REPAIRS`: `tilfa` comes from `rlfa_srlg_device`'s tables, so a primary with
    /// members may take its repair — unless the repair's forced link is a member (`HSPF_BK_SRLG_PAIR_REFUSED`).  `bk_coverage` has
    /// `HSPF_BK_SRLG_COVERAGE_WORDS` words per root.
    #[allow(clippy::too_many_arguments)]
    pub fn routes_backup_srlg_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], srlgs: &[&SrlgMembers],
                                     ignore_overload: bool, safe_repairs: bool, table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>,
                                     tilfa: Option<&Tilfa>) -> Result<Backup, Error> {
        self.routes_backup_device_with(tables, protect, None, Some((srlgs, safe_repairs)), ignore_overload, table, resident, routes, tilfa)
    }

    /// `hspf_routes_backup_lan_device`: `routes_backup_device` with loop-freeness towards the pseudonode of every primary's LAN;
    /// a LAN primary never takes the per-link repair.  `lans` as for `lfa_lan_device`; `bk_coverage` has
    /// `HSPF_BK_LAN_COVERAGE_WORDS` words per root.
    #[allow(clippy::too_many_arguments)]
    pub fn routes_backup_lan_device(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], lans: &[(&[u32], &[u32])],
                                    ignore_overload: bool, table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>,
                                    tilfa: Option<&Tilfa>) -> Result<Backup, Error> {
        self.routes_backup_device_with(tables, protect, Some(lans), None, ignore_overload, table, resident, routes, tilfa)
    }

    /// The frame of `routes_backup_device` (`lans` and `srlg` None), `routes_backup_lan_device` and `routes_backup_srlg_device`.
    #[allow(clippy::too_many_arguments)]
    fn routes_backup_device_with(&self, tables: &DeviceTables<'_>, protect: &[(u32, &LfaCandidates, &[u32])], lans: Option<&[(&[u32], &[u32])]>,
                                 srlg: Option<(&[&SrlgMembers], bool)>, ignore_overload: bool, table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>,
                                 tilfa: Option<&Tilfa>) -> Result<Backup, Error> {
        let (np, pf, w) = (protect.len(), table.n_prefixes() as usize, tables.words as usize);
        let lan_raw = match lans { Some(l) => Some(Self::lan_raw("routes_backup_lan_device", protect, l)?), None => None };
        let srlg_raw = match srlg { Some((m, _)) => Some(Self::srlg_raw("routes_backup_srlg_device", protect, m)?), None => None };
        let cov_words = if srlg.is_some() { sys::HSPF_BK_SRLG_COVERAGE_WORDS } else if lans.is_some() { sys::HSPF_BK_LAN_COVERAGE_WORDS } else { sys::HSPF_BK_COVERAGE_WORDS } as usize;
        if routes.n_prefixes != table.n_prefixes() || routes.words != tables.words {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_device: the routes are not of this table set and table".into() });
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_device: the slot arrays of a protected root differ in length".into() });
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let slots = np * 64 * w;
        let ti = match tilfa {
            Some(t) if t.ti_kind.len() == slots && t.ti_via.len() == slots && t.ti_metric.len() == slots => {
                Some((self.device_from(&t.ti_kind)?, self.device_from(&t.ti_via)?, self.device_from(&t.ti_metric)?))
            }
            Some(_) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_device: the TI-LFA result is not of this protect list".into() }),
            None => None,
        };
        // the SRLG call also reads the forced adjacency of a pair
        let ti_pl = match (tilfa, srlg) {
            (Some(t), Some(_)) if t.ti_p.len() == slots && t.ti_link.len() == slots => Some((self.device_from(&t.ti_p)?, self.device_from(&t.ti_link)?)),
            (Some(_), Some(_)) => return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_backup_srlg_device: the TI-LFA result is not of this protect list".into() }),
            _ => None,
        };
        let ti_raw = ti.as_ref().map(|(k, v, m)| sys::hspf_tilfa_out {
            ti_kind: k.p as *mut u8,
            ti_p: ti_pl.as_ref().map_or(ptr::null_mut(), |x| x.0.p as *mut u32),
            ti_q: ptr::null_mut(),
            ti_via: v.p as *mut u32,
            ti_link: ti_pl.as_ref().map_or(ptr::null_mut(), |x| x.1.p as *mut u32),
            ti_metric: m.p as *mut u32,
            ti_counts: ptr::null_mut(),
            td_kind: ptr::null_mut(),
            td_coverage: ptr::null_mut(),
        });
        let cells = np * pf;
        let bk_kind = self.device_alloc(cells)?;
        let bk_primary = self.device_alloc(cells * 4)?;
        let bk_slot = self.device_alloc(cells * 4)?;
        let bk_metric = self.device_alloc(cells * 4)?;
        let bk_flags = self.device_alloc(cells)?;
        let bk_cand = self.device_alloc(cells * 8 * w)?;
        let bk_node = self.device_alloc(cells * 8 * w)?;
        let bk_cov = self.device_alloc(np * cov_words * 4)?;
        let mut out = sys::hspf_backup_out {
            bk_kind: bk_kind.p as *mut u8,
            bk_primary: bk_primary.p as *mut u32,
            bk_slot: bk_slot.p as *mut u32,
            bk_metric: bk_metric.p as *mut u32,
            bk_flags: bk_flags.p as *mut u8,
            bk_cand_mask: bk_cand.p as *mut u64,
            bk_node_mask: bk_node.p as *mut u64,
            bk_coverage: bk_cov.p as *mut u32,
        };
        let t = sys::hspf_prefix_table {
            n_prefixes: table.n_prefixes(),
            n_entries: table.pfx_vertex.len() as u32,
            pfx_ptr: table.pfx_ptr.as_ptr(),
            pfx_vertex: table.pfx_vertex.as_ptr(),
            pfx_metric: table.pfx_metric.as_ptr(),
            flags: table.flags | if resident { sys::HSPF_PFX_RESIDENT } else { 0 },
            pfx_origin: ptr::null(),
            init_exists: ptr::null(),
            init_metric: ptr::null(),
            init_origin: ptr::null(),
        };
        let r = sys::hspf_routes {
            best_metric: routes.best_metric.p as *mut u32,
            best_entry: routes.best_entry.p as *mut u32,
            nexthop_mask: routes.nexthop_mask.p as *mut u64,
        };
        let lfa_flags = if ignore_overload { sys::HSPF_LFA_IGNORE_OVERLOAD } else { 0 }
            | if matches!(srlg, Some((_, true))) { sys::HSPF_LFA_SRLG_SAFE_REPAIRS } else { 0 };
        let (dist, flags_in, mask) = (tables.dist.p as *const u32, tables.flags.p as *const u16, tables.mask.p as *const u64);
        let ti_ptr = ti_raw.as_ref().map_or(ptr::null(), |x| x as *const sys::hspf_tilfa_out);
        let rc = unsafe {
            match &lan_raw {
                None if srlg_raw.is_some() => sys::hspf_routes_backup_srlg_device(
                    self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), srlg_raw.as_ref().unwrap().as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, &mut out,
                ),
                None => sys::hspf_routes_backup_device(self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, &mut out),
                Some(l) => sys::hspf_routes_backup_lan_device(
                    self.ctx, tables.n_vertices, tables.n_roots, tables.words, dist, flags_in, mask, raw.as_ptr(), l.as_ptr(), np as u32, lfa_flags, &t, &r, ti_ptr, &mut out,
                ),
            }
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Backup {
            n_protected: np as u32,
            n_prefixes: table.n_prefixes(),
            words: tables.words,
            bk_kind: bk_kind.to_host(cells)?,
            bk_primary: bk_primary.to_host(cells)?,
            bk_slot: bk_slot.to_host(cells)?,
            bk_metric: bk_metric.to_host(cells)?,
            bk_flags: bk_flags.to_host(cells)?,
            bk_cand_mask: bk_cand.to_host(cells * w)?,
            bk_node_mask: bk_node.to_host(cells * w)?,
            bk_coverage: bk_cov.to_host(np * cov_words)?,
        })
    }

    /// `hspf_routes_backup_node_device`: per (protected root, prefix) with one primary the cheapest listed PQ node of `rlfa_node`
    /// — or, where none protects, the cheapest listed pair of `tilfa_node` — that reaches the PREFIX without the primary's
    /// neighbour; one `hspf_run_device` over the ascending union of the listed nodes on the way.  At least one of the two lists;
    /// `backup`: what `routes_backup_device` returned for the same `protect` and `table` (its node-protecting alternates stand),
    /// or `None`.  `resident`: the context still holds `table`.
    #[allow(clippy::too_many_arguments)]
    pub fn routes_backup_node_device(&self, g: &Graph<'_>, tables: &DeviceTables<'_>, run_flags: u32, protect: &[(u32, &LfaCandidates, &[u32])],
                                     table: &PrefixTable, resident: bool, routes: &DeviceRoutes<'_>, rlfa_node: Option<&RlfaNode>,
                                     tilfa_node: Option<&TilfaNode>, backup: Option<&Backup>) -> Result<BackupNode, Error> {
        let (np, pf, w) = (protect.len(), table.n_prefixes() as usize, tables.words as usize);
        let bad = |what: &str| Error { code: sys::HSPF_E_INVAL, detail: format!("routes_backup_node_device: {what}") };
        if routes.n_prefixes != table.n_prefixes() || routes.words != tables.words {
            return Err(bad("the routes are not of this table set and table"));
        }
        if rlfa_node.is_none() && tilfa_node.is_none() {
            return Err(bad("at least one of the two lists is required"));
        }
        let mut raw = Vec::with_capacity(np);
        for (root_row, c, nbr_row) in protect {
            let k = c.nbr.len();
            if nbr_row.len() != k || c.cost.len() != k || c.root_link.len() != k || c.cflags.len() != k {
                return Err(bad("the slot arrays of a protected root differ in length"));
            }
            raw.push(sys::hspf_lfa_protect {
                root_vertex: c.root,
                root_row: *root_row,
                n_slots: k as u32,
                nbr: c.nbr.as_ptr(),
                nbr_row: nbr_row.as_ptr(),
                cost: c.cost.as_ptr(),
                root_link: c.root_link.as_ptr(),
                cflags: c.cflags.as_ptr(),
            });
        }
        let slots = np * 64 * w;
        let cells = np * pf;
        let mut y_roots: Vec<u32> = Vec::new();
        let rn = match rlfa_node {
            Some(r) if r.nq_count.len() == slots && r.nq_node.len() == slots * r.max_pq as usize => {
                y_roots.extend(r.nq_node.iter().copied().filter(|&v| v != sys::HSPF_NO_ROOT));
                Some((self.device_from(&r.nq_node)?, self.device_from(&r.nq_via)?, self.device_from(&r.nq_metric)?, self.device_from(&r.nq_count)?, r.max_pq))
            }
            Some(_) => return Err(bad("the RLFA-node result is not of this protect list")),
            None => None,
        };
        let tn = match tilfa_node {
            Some(t) if t.tq_count.len() == slots && t.tq_q.len() == slots * t.max_pairs as usize => {
                y_roots.extend(t.tq_q.iter().copied().filter(|&v| v != sys::HSPF_NO_ROOT));
                Some((
                    self.device_from(&t.tq_q)?,
                    self.device_from(&t.tq_p)?,
                    self.device_from(&t.tq_link)?,
                    self.device_from(&t.tq_via)?,
                    self.device_from(&t.tq_metric)?,
                    self.device_from(&t.tq_count)?,
                    t.max_pairs,
                ))
            }
            Some(_) => return Err(bad("the TI-LFA-node result is not of this protect list")),
            None => None,
        };
        let bk = match backup {
            Some(b) if b.bk_kind.len() == cells && b.bk_flags.len() == cells => Some((self.device_from(&b.bk_kind)?, self.device_from(&b.bk_flags)?)),
            Some(_) => return Err(bad("the backup result is not of this protect list and table")),
            None => None,
        };
        y_roots.sort_unstable();
        y_roots.dedup();
        if y_roots.is_empty() {
            y_roots.push(sys::HSPF_NO_ROOT); // one padding row keeps the arguments of the call valid
        }
        let y = self.run_device(g, &y_roots, run_flags)?;
        let rn_raw = rn.as_ref().map(|(a, b, c, d, _)| sys::hspf_rlfa_node_sel { nq_node: a.p as *mut u32, nq_via: b.p as *mut u32, nq_metric: c.p as *mut u32, nq_count: d.p as *mut u32 });
        let tn_raw = tn.as_ref().map(|(a, b, c, d, e, f, _)| sys::hspf_tilfa_node_sel {
            tq_q: a.p as *mut u32,
            tq_p: b.p as *mut u32,
            tq_link: c.p as *mut u32,
            tq_via: d.p as *mut u32,
            tq_metric: e.p as *mut u32,
            tq_count: f.p as *mut u32,
        });
        let bk_raw = bk.as_ref().map(|(k, f)| sys::hspf_backup_out {
            bk_kind: k.p as *mut u8,
            bk_primary: ptr::null_mut(),
            bk_slot: ptr::null_mut(),
            bk_metric: ptr::null_mut(),
            bk_flags: f.p as *mut u8,
            bk_cand_mask: ptr::null_mut(),
            bk_node_mask: ptr::null_mut(),
            bk_coverage: ptr::null_mut(),
        });
        let bn_kind = self.device_alloc(cells)?;
        let bn_primary = self.device_alloc(cells * 4)?;
        let bn_p = self.device_alloc(cells * 4)?;
        let bn_q = self.device_alloc(cells * 4)?;
        let bn_link = self.device_alloc(cells * 4)?;
        let bn_via = self.device_alloc(cells * 4)?;
        let bn_metric = self.device_alloc(cells * 4)?;
        let bn_set_pq = self.device_alloc(cells * 4)?;
        let bn_set_pair = self.device_alloc(cells * 4)?;
        let bn_cov = self.device_alloc(np * sys::HSPF_BN_COVERAGE_WORDS as usize * 4)?;
        let mut out = sys::hspf_backup_node_out {
            bn_kind: bn_kind.p as *mut u8,
            bn_primary: bn_primary.p as *mut u32,
            bn_p: bn_p.p as *mut u32,
            bn_q: bn_q.p as *mut u32,
            bn_link: bn_link.p as *mut u32,
            bn_via: bn_via.p as *mut u32,
            bn_metric: bn_metric.p as *mut u32,
            bn_set_pq: bn_set_pq.p as *mut u32,
            bn_set_pair: bn_set_pair.p as *mut u32,
            bn_coverage: bn_cov.p as *mut u32,
        };
        let t = sys::hspf_prefix_table {
            n_prefixes: table.n_prefixes(),
            n_entries: table.pfx_vertex.len() as u32,
            pfx_ptr: table.pfx_ptr.as_ptr(),
            pfx_vertex: table.pfx_vertex.as_ptr(),
            pfx_metric: table.pfx_metric.as_ptr(),
            flags: table.flags | if resident { sys::HSPF_PFX_RESIDENT } else { 0 },
            pfx_origin: ptr::null(),
            init_exists: ptr::null(),
            init_metric: ptr::null(),
            init_origin: ptr::null(),
        };
        let r = sys::hspf_routes {
            best_metric: routes.best_metric.p as *mut u32,
            best_entry: routes.best_entry.p as *mut u32,
            nexthop_mask: routes.nexthop_mask.p as *mut u64,
        };
        let rc = unsafe {
            sys::hspf_routes_backup_node_device(
                self.ctx,
                tables.n_vertices,
                tables.n_roots,
                tables.words,
                tables.dist.p as *const u32,
                tables.flags.p as *const u16,
                tables.mask.p as *const u64,
                raw.as_ptr(),
                np as u32,
                &t,
                &r,
                y.dist.p as *const u32,
                y_roots.as_ptr(),
                y_roots.len() as u32,
                rn_raw.as_ref().map_or(ptr::null(), |x| x as *const sys::hspf_rlfa_node_sel),
                rn.as_ref().map_or(0, |x| x.4),
                tn_raw.as_ref().map_or(ptr::null(), |x| x as *const sys::hspf_tilfa_node_sel),
                tn.as_ref().map_or(0, |x| x.6),
                bk_raw.as_ref().map_or(ptr::null(), |x| x as *const sys::hspf_backup_out),
                &mut out,
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(BackupNode {
            n_protected: np as u32,
            n_prefixes: table.n_prefixes(),
            y_roots,
            bn_kind: bn_kind.to_host(cells)?,
            bn_primary: bn_primary.to_host(cells)?,
            bn_p: bn_p.to_host(cells)?,
            bn_q: bn_q.to_host(cells)?,
            bn_link: bn_link.to_host(cells)?,
            bn_via: bn_via.to_host(cells)?,
            bn_metric: bn_metric.to_host(cells)?,
            bn_set_pq: bn_set_pq.to_host(cells)?,
            bn_set_pair: bn_set_pair.to_host(cells)?,
            bn_coverage: bn_cov.to_host(np * sys::HSPF_BN_COVERAGE_WORDS as usize)?,
        })
    }

    /// `true`: these runs are too small to pay for a launch — keep the CPU loop (hspf_recommend_cpu).
    pub fn recommend_cpu(n_vertices: u32, n_edges: u32, n_roots: u32) -> bool {
        unsafe { sys::hspf_recommend_cpu(n_vertices, n_edges, n_roots) != 0 }
    }

    pub fn upload(&self, csr: &Csr) -> Result<Graph<'_>, Error> {
        let c = sys::hspf_csr {
            n_vertices: csr.n_vertices(),
            n_edges: csr.col.len() as u32,
            row_ptr: csr.row_ptr.as_ptr(),
            col: csr.col.as_ptr(),
            metric: csr.metric.as_ptr(),
            vflags: csr.vflags.as_ptr(),
            max_path_metric: csr.max_path_metric,
        };
        let mut g = ptr::null_mut();
        let rc = unsafe { sys::hspf_graph_upload(self.ctx, &c, &mut g) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Graph { eng: self, g, n: csr.n_vertices(), _not_sync: PhantomData })
    }

    /// `hspf_graph_upload_keyed` (ABI 8): the LSDB's records as they sit there — vertices by 64-bit key in any order, links
    /// by target key in LSP / LSA order, targets unresolved.  The device ranks the keys (ascending key order = the reference's
    /// `VertexId` order, holo-isis/src/spf.rs:96-100), resolves the targets and drops links to vertices the LSDB does not
    /// hold (`vertex_edges` does not yield them, holo-isis/src/spf.rs:1013-1128).  Returns the graph and, per input
    /// vertex, its index in it; `Graph::export_csr` reads the CSR it built back for the host mirrors.
    pub fn upload_keyed(&self, lsdb: &KeyedLsdb) -> Result<(Graph<'_>, Vec<u32>), Error> {
        let n = lsdb.vertex_key.len();
        if lsdb.row_ptr.len() != n + 1 || lsdb.vflags.len() != n || lsdb.metric.len() != lsdb.target_key.len()
            || lsdb.row_ptr.last().copied().unwrap_or(0) as usize != lsdb.target_key.len()
        {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "upload_keyed: array lengths disagree".into() });
        }
        let c = sys::hspf_keyed_lsdb {
            n_vertices: n as u32,
            n_links: lsdb.target_key.len() as u32,
            vertex_key: lsdb.vertex_key.as_ptr(),
            row_ptr: lsdb.row_ptr.as_ptr(),
            target_key: lsdb.target_key.as_ptr(),
            metric: lsdb.metric.as_ptr(),
            vflags: lsdb.vflags.as_ptr(),
            max_path_metric: lsdb.max_path_metric,
        };
        let mut g = ptr::null_mut();
        let mut rank = vec![0u32; n];
        let rc = unsafe { sys::hspf_graph_upload_keyed(self.ctx, &c, &mut g, rank.as_mut_ptr()) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok((Graph { eng: self, g, n: n as u32, _not_sync: PhantomData }, rank))
    }

    pub fn host_alloc(&self, bytes: usize) -> Result<PinnedBuf<'_>, Error> {
        let mut p = ptr::null_mut();
        let rc = unsafe { sys::hspf_host_alloc(self.ctx, bytes, &mut p) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(PinnedBuf { eng: self, p, bytes })
    }

    fn size_class(bytes: usize) -> usize {
        (bytes.max(1) + 65535) & !65535
    }

    pub fn device_alloc(&self, bytes: usize) -> Result<DeviceBuf<'_>, Error> {
        let class = Self::size_class(bytes);
        if let Some(p) = self.pool.borrow_mut().get_mut(&class).and_then(|free| free.pop()) {
            return Ok(DeviceBuf { eng: self, p, bytes });
        }
        let mut p = ptr::null_mut();
        let rc = unsafe { sys::hspf_device_alloc(self.ctx, class, &mut p) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(DeviceBuf { eng: self, p, bytes })
    }

    fn device_from<T: Copy>(&self, v: &[T]) -> Result<DeviceBuf<'_>, Error> {
        let bytes = std::mem::size_of_val(v);
        let d = self.device_alloc(bytes)?;
        let rc = unsafe { sys::hspf_host_to_device(self.ctx, d.p, v.as_ptr() as *const c_void, bytes) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(d)
    }

    /// Results on the host.  First the PACKED hand-off (`hspf_run_packed`: one word per (root, vertex) into page-locked
    /// memory, a quarter of `hspf_run`'s bytes over the bus; `reuse` = the buffer of an earlier result); runs whose
    /// results do not fit packed words (`HSPF_E_NO_PACKED`: more than 24 first-hop slots) take `hspf_run`.  `roots` may
    /// hold `HSPF_NO_ROOT` padding.
    pub fn run<'e>(&'e self, g: &Graph<'_>, roots: &[u32], run_flags: u32, reuse: Option<PinnedBuf<'e>>) -> Result<Tables<'e>, Error> {
        match self.run_packed(g, roots, run_flags, reuse) {
            Err(e) if e.code == sys::HSPF_E_NO_PACKED => self.run_full(g, roots, run_flags),
            other => other,
        }
    }

    /// `hspf_run_packed` (ABI 7).
    pub fn run_packed<'e>(&'e self, g: &Graph<'_>, roots: &[u32], run_flags: u32, reuse: Option<PinnedBuf<'e>>) -> Result<Tables<'e>, Error> {
        let need = 8 * roots.len() * g.n as usize;
        let buf = match reuse {
            Some(b) if b.len() >= need => b,
            _ => self.host_alloc(need)?,
        };
        let mut layout = std::mem::MaybeUninit::<sys::hspf_packed_layout>::zeroed();
        let mut root_status = vec![0u8; roots.len()];
        let rc = unsafe {
            sys::hspf_run_packed(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, run_flags, buf.p, buf.bytes, layout.as_mut_ptr(), root_status.as_mut_ptr())
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Tables { n_roots: roots.len() as u32, n_vertices: g.n, repr: Repr::Packed { buf, layout: unsafe { layout.assume_init() }, root_status } })
    }

    /// `hspf_run_packed_async`: the run AND its copy to the host belong to the ticket (the copy of one batch crosses the
    /// bus while the next computes).  `wait_packed` gives the tables.
    pub fn run_packed_async<'e>(&'e self, g: &Graph<'_>, roots: &[u32], run_flags: u32, reuse: Option<PinnedBuf<'e>>) -> Result<PackedTicket<'e>, Error> {
        let need = 8 * roots.len() * g.n as usize;
        let buf = match reuse {
            Some(b) if b.len() >= need => b,
            _ => self.host_alloc(need)?,
        };
        let mut root_status = vec![0u8; roots.len()].into_boxed_slice();
        let mut ticket = 0u64;
        let rc = unsafe {
            sys::hspf_run_packed_async(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, run_flags, buf.p, buf.bytes, root_status.as_mut_ptr(), &mut ticket)
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(PackedTicket { eng: self, ticket, buf: Some(buf), root_status: Some(root_status), n_roots: roots.len() as u32, n_vertices: g.n })
    }

    pub fn wait_packed<'e>(&'e self, mut t: PackedTicket<'e>) -> Result<Tables<'e>, Error> {
        let mut layout = std::mem::MaybeUninit::<sys::hspf_packed_layout>::zeroed();
        let rc = unsafe { sys::hspf_wait_packed(self.ctx, t.ticket, layout.as_mut_ptr(), ptr::null_mut()) };
        // (the run is over either way: the ticket's drop has nothing left to wait for)
        let (buf, root_status) = (t.buf.take().expect("a ticket is waited for once"), t.root_status.take().expect("a ticket is waited for once"));
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Tables {
            n_roots: t.n_roots,
            n_vertices: t.n_vertices,
            repr: Repr::Packed { buf, layout: unsafe { layout.assume_init() }, root_status: root_status.into_vec() },
        })
    }

    /// `hspf_mask_words` + `hspf_run`: four arrays in host vectors.
    pub fn run_full(&self, g: &Graph<'_>, roots: &[u32], run_flags: u32) -> Result<Tables<'_>, Error> {
        let mut words = 0u32;
        let rc = unsafe { sys::hspf_mask_words(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, &mut words) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let cells = roots.len() * g.n as usize;
        let (mut dist, mut hops, mut flags, mut mask) = (vec![0u32; cells], vec![0u16; cells], vec![0u16; cells], vec![0u64; cells * words as usize]);
        let mut out = sys::hspf_result {
            dist: dist.as_mut_ptr(),
            hops: hops.as_mut_ptr(),
            vflags_out: flags.as_mut_ptr(),
            first_hop_mask: mask.as_mut_ptr(),
            n_mask_words: words,
            pop_rank: ptr::null_mut(),
        };
        let rc = unsafe { sys::hspf_run(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, run_flags, &mut out) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Tables { n_roots: roots.len() as u32, n_vertices: g.n, repr: Repr::Full { words, dist, hops, flags, mask } })
    }

    /// `hspf_mask_words` + `hspf_run_failures`: `run_failures_device` with the four arrays in host vectors.
    pub fn run_failures(&self, g: &Graph<'_>, roots: &[u32], failures: &[sys::hspf_failure], run_flags: u32) -> Result<Tables<'_>, Error> {
        if failures.len() != roots.len() {
            return Err(self.err(sys::HSPF_E_INVAL));
        }
        let mut words = 0u32;
        let rc = unsafe { sys::hspf_mask_words(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, &mut words) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let cells = roots.len() * g.n as usize;
        let (mut dist, mut hops, mut flags, mut mask) = (vec![0u32; cells], vec![0u16; cells], vec![0u16; cells], vec![0u64; cells * words as usize]);
        let mut out = sys::hspf_result {
            dist: dist.as_mut_ptr(),
            hops: hops.as_mut_ptr(),
            vflags_out: flags.as_mut_ptr(),
            first_hop_mask: mask.as_mut_ptr(),
            n_mask_words: words,
            pop_rank: ptr::null_mut(),
        };
        let rc = unsafe { sys::hspf_run_failures(self.ctx, g.g, roots.as_ptr(), failures.as_ptr(), roots.len() as u32, run_flags, &mut out) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(Tables { n_roots: roots.len() as u32, n_vertices: g.n, repr: Repr::Full { words, dist, hops, flags, mask } })
    }

    /// `hspf_run_device`: the tables stay in HBM (input of `routes_device` / `ancestors_device`).
    pub fn run_device(&self, g: &Graph<'_>, roots: &[u32], run_flags: u32) -> Result<DeviceTables<'_>, Error> {
        let mut words = 0u32;
        let rc = unsafe { sys::hspf_mask_words(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, &mut words) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let cells = roots.len() * g.n as usize;
        let t = DeviceTables {
            n_roots: roots.len() as u32,
            n_vertices: g.n,
            words,
            dist: self.device_alloc(cells * 4)?,
            hops: self.device_alloc(cells * 2)?,
            flags: self.device_alloc(cells * 2)?,
            mask: self.device_alloc(cells * 8 * words as usize)?,
        };
        let mut out = sys::hspf_result {
            dist: t.dist.p as *mut u32,
            hops: t.hops.p as *mut u16,
            vflags_out: t.flags.p as *mut u16,
            first_hop_mask: t.mask.p as *mut u64,
            n_mask_words: words,
            pop_rank: ptr::null_mut(),
        };
        let rc = unsafe { sys::hspf_run_device(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, run_flags, &mut out) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(t)
    }

    /// `hspf_run_failures_device`: row r is the run of `roots[r]` with `failures[r]` applied (`HSPF_FAIL_ROOT_LINK`: a position in
    /// the root's own row; `HSPF_FAIL_VERTEX`: a vertex other than the root), the graph untouched — the post-convergence trees of
    /// a router's links and neighbours in one batch.  The tables stay in HBM like `run_device`'s.
    pub fn run_failures_device(&self, g: &Graph<'_>, roots: &[u32], failures: &[sys::hspf_failure], run_flags: u32) -> Result<DeviceTables<'_>, Error> {
        if failures.len() != roots.len() {
            return Err(self.err(sys::HSPF_E_INVAL));
        }
        let mut words = 0u32;
        let rc = unsafe { sys::hspf_mask_words(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, &mut words) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let cells = roots.len() * g.n as usize;
        let t = DeviceTables {
            n_roots: roots.len() as u32,
            n_vertices: g.n,
            words,
            dist: self.device_alloc(cells * 4)?,
            hops: self.device_alloc(cells * 2)?,
            flags: self.device_alloc(cells * 2)?,
            mask: self.device_alloc(cells * 8 * words as usize)?,
        };
        let mut out = sys::hspf_result {
            dist: t.dist.p as *mut u32,
            hops: t.hops.p as *mut u16,
            vflags_out: t.flags.p as *mut u16,
            first_hop_mask: t.mask.p as *mut u64,
            n_mask_words: words,
            pop_rank: ptr::null_mut(),
        };
        let rc = unsafe { sys::hspf_run_failures_device(self.ctx, g.g, roots.as_ptr(), failures.as_ptr(), roots.len() as u32, run_flags, &mut out) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(t)
    }

    /// `hspf_routes_device`: prefix attachment for every root of `run`, tables left in HBM.  `resident`: the table is the
    /// one the previous call on this engine passed (same vectors, untouched): nothing is uploaded again.
    pub fn routes_device(&self, run: &DeviceTables<'_>, table: &PrefixTable, resident: bool) -> Result<DeviceRoutes<'_>, Error> {
        let (r, p, w) = (run.n_roots as usize, table.n_prefixes() as usize, run.words as usize);
        let out = DeviceRoutes {
            n_roots: run.n_roots,
            n_prefixes: table.n_prefixes(),
            words: run.words,
            best_metric: self.device_alloc(r * p * 4)?,
            best_entry: self.device_alloc(r * p * 4)?,
            nexthop_mask: self.device_alloc(r * p * 8 * w)?,
        };
        if p == 0 {
            return Ok(out);
        }
        let t = sys::hspf_prefix_table {
            n_prefixes: table.n_prefixes(),
            n_entries: table.pfx_vertex.len() as u32,
            pfx_ptr: table.pfx_ptr.as_ptr(),
            pfx_vertex: table.pfx_vertex.as_ptr(),
            pfx_metric: table.pfx_metric.as_ptr(),
            flags: table.flags | if resident { sys::HSPF_PFX_RESIDENT } else { 0 },
            pfx_origin: ptr::null(),
            init_exists: ptr::null(),
            init_metric: ptr::null(),
            init_origin: ptr::null(),
        };
        let mut ro = out.raw();
        let rc = unsafe {
            sys::hspf_routes_device(self.ctx, run.n_vertices, run.n_roots, run.words, run.dist.p as *const u32, run.flags.p as *const u16, run.mask.p as *const u64, &t, &mut ro)
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(out)
    }

    /// A host table set brought to the device: the RIB held before, when no previous device set is comparable.
    pub fn routes_upload(&self, n_roots: u32, n_prefixes: u32, words: u32, best_metric: &[u32], best_entry: &[u32], nexthop_mask: &[u64]) -> Result<DeviceRoutes<'_>, Error> {
        Ok(DeviceRoutes {
            n_roots,
            n_prefixes,
            words,
            best_metric: self.device_from(best_metric)?,
            best_entry: self.device_from(best_entry)?,
            nexthop_mask: self.device_from(nexthop_mask)?,
        })
    }

    /// `hspf_routes_events` (+ `hspf_routes_events_rest` when the stream is longer than the first call took): every
    /// (root, prefix) pair whose action is not SAME — `HSPF_DIFF_SILENT` pairs included when `with_silent` — as paired
    /// old -> new records in the reference's emission order.  ONE comparison on the device, one synchronisation and one
    /// copy in the steady state; with `with_silent` a caller's own RIB follows every event of the engine.
    pub fn routes_events(&self, old: &DeviceRoutes<'_>, new: &DeviceRoutes<'_>, with_silent: bool) -> Result<Vec<RouteRecord>, Error> {
        if old.n_roots != new.n_roots || old.n_prefixes != new.n_prefixes || old.words != new.words {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_events: the two sets differ in shape".into() });
        }
        let w = new.words as usize;
        let stride = sys::HSPF_EVENT_REC_WORDS as usize + 4 * w;
        let hint = self.events_hint.get();
        let cap = (hint + hint / 4).max(1024);
        let mut rec = vec![0u32; cap * stride];
        let mut total = 0u32;
        let (ro, rn) = (old.raw(), new.raw());
        let flags = if with_silent { sys::HSPF_EV_SILENT } else { 0 };
        let rc = unsafe {
            sys::hspf_routes_events(self.ctx, new.n_roots, new.n_prefixes, new.words, &ro, &rn, flags, cap as u32, rec.as_mut_ptr(), &mut total)
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let k = total as usize;
        self.events_hint.set(k);
        rec.resize(k * stride, 0);
        if k > cap {
            let rc = unsafe { sys::hspf_routes_events_rest(self.ctx, cap as u32, (k - cap) as u32, rec[cap * stride..].as_mut_ptr()) };
            if rc != sys::HSPF_OK {
                return Err(self.err(rc));
            }
        }
        let words_of = |half: &[u32]| -> Vec<u64> { (0..w).map(|i| half[2 * i] as u64 | (half[2 * i + 1] as u64) << 32).collect() };
        Ok(rec
            .chunks_exact(stride)
            .map(|r| RouteRecord {
                root: r[0],
                prefix: r[1],
                action: r[2],
                new_metric: r[3],
                new_entry: r[4],
                new_mask: words_of(&r[8..8 + 2 * w]),
                old_metric: r[5],
                old_entry: r[6],
                old_mask: words_of(&r[8 + 2 * w..]),
            })
            .collect())
    }

    /// `hspf_routes_diff_device` + `hspf_routes_pack` (twice: the changed list packed from the new set and from the old
    /// one): the (root, prefix) pairs that need a RouteIpAdd / RouteIpDel, in the reference's emission order, with what the
    /// route is and what it was.  ONE comparison on the device, two small copies to the host.
    pub fn routes_changed(&self, old: &DeviceRoutes<'_>, new: &DeviceRoutes<'_>) -> Result<Vec<RouteRecord>, Error> {
        if old.n_roots != new.n_roots || old.n_prefixes != new.n_prefixes || old.words != new.words {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "routes_changed: the two sets differ in shape".into() });
        }
        let (r, p, w) = (new.n_roots as usize, new.n_prefixes as usize, new.words as usize);
        if r * p == 0 {
            return Ok(Vec::new());
        }
        let action = self.device_alloc(r * p)?;
        let changed = self.device_alloc(r * p * 4)?;
        let changed_ptr = self.device_alloc((r + 1) * 4)?;
        let (ro, rn) = (old.raw(), new.raw());
        let rc = unsafe {
            sys::hspf_routes_diff_device(self.ctx, new.n_roots, new.n_prefixes, new.words, &ro, &rn, action.p as *mut u8, changed.p as *mut u32, changed_ptr.p as *mut u32)
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        let k = unsafe { sys::hspf_routes_diff_count(self.ctx) } as usize;
        let stride = sys::HSPF_ROUTE_REC_WORDS as usize + 2 * w;
        let (mut rec_new, mut rec_old) = (vec![0u32; k * stride], vec![0u32; k * stride]);
        if k != 0 {
            for (set, rec) in [(&rn, &mut rec_new), (&ro, &mut rec_old)] {
                let rc = unsafe {
                    sys::hspf_routes_pack(self.ctx, new.n_roots, new.n_prefixes, new.words, set, action.p as *const u8, changed.p as *const u32, changed_ptr.p as *const u32, k as u32, rec.as_mut_ptr())
                };
                if rc != sys::HSPF_OK {
                    return Err(self.err(rc));
                }
            }
        }
        let words_of = |rec: &[u32]| -> Vec<u64> { (0..w).map(|i| rec[6 + 2 * i] as u64 | (rec[7 + 2 * i] as u64) << 32).collect() };
        Ok((0..k)
            .map(|i| {
                let (n, o) = (&rec_new[i * stride..(i + 1) * stride], &rec_old[i * stride..(i + 1) * stride]);
                RouteRecord {
                    root: n[0],
                    prefix: n[1],
                    action: n[2],
                    new_metric: n[3],
                    new_entry: n[4],
                    new_mask: words_of(n),
                    old_metric: o[3],
                    old_entry: o[4],
                    old_mask: words_of(o),
                }
            })
            .collect())
    }

    /// `hspf_ancestors_device`: for every root of a hop-count `run_device` and level L (1 = first hops, 2 = second hops) the
    /// bit sets that answer `Spt::is_on_path(a, d)` (holo-isis/src/spf.rs:261-286) for a level-L router `a` with one bit
    /// test: `AncestorSets::is_on_path`.  A root that needed the sequential kernel has no sets (`level_count` all ones):
    /// the caller keeps its own walk for it.
    pub fn ancestors_device(&self, g: &Graph<'_>, roots: &[u32], run_flags: u32, run: &DeviceTables<'_>, level: u32) -> Result<AncestorSets, Error> {
        let (r, n) = (roots.len(), g.n as usize);
        let level_rank = self.device_alloc(r * n * 4)?;
        let level_count = self.device_alloc(r * 4)?;
        let mut words = 1u32;
        loop {
            let anc = self.device_alloc(r * n * 8 * words as usize)?;
            let rc = unsafe {
                sys::hspf_ancestors_device(
                    self.ctx, g.g, roots.as_ptr(), r as u32, run_flags, run.dist.p as *const u32, run.hops.p as *const u16, run.flags.p as *const u16,
                    level, words, level_rank.p as *mut u32, level_count.p as *mut u32, anc.p as *mut u64,
                )
            };
            let count: Vec<u32> = level_count.to_host(r)?;
            if rc == sys::HSPF_E_TOO_MANY_SLOTS {
                let most = count.iter().copied().filter(|&c| c != u32::MAX).max().unwrap_or(0);
                words = most.div_ceil(64).max(words + 1);
                continue;
            }
            if rc != sys::HSPF_OK {
                return Err(self.err(rc));
            }
            return Ok(AncestorSets { n_vertices: g.n, words, level_rank: level_rank.to_host(r * n)?, level_count: count, anc: anc.to_host(r * n * words as usize)? });
        }
    }

    /// Pop ranks of roots whose pop order is dynamic (`HSPF_RF_EXACT`: zero-cost plateaus): `[root][vertex]`.
    pub fn pop_ranks(&self, g: &Graph<'_>, roots: &[u32], run_flags: u32) -> Result<Vec<u32>, Error> {
        let cells = roots.len() * g.n as usize;
        let (mut dist, mut rank) = (vec![0u32; cells], vec![0u32; cells]);
        let mut out = sys::hspf_result {
            dist: dist.as_mut_ptr(),
            hops: ptr::null_mut(),
            vflags_out: ptr::null_mut(),
            first_hop_mask: ptr::null_mut(),
            n_mask_words: 0,
            pop_rank: rank.as_mut_ptr(),
        };
        let flags = run_flags | sys::HSPF_RUN_POP_RANK;
        let rc = unsafe { sys::hspf_run(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, flags, &mut out) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(rank)
    }

    /// Several runs in flight from this one thread (one per area / level / neighbour set): device buffers, a ticket.
    ///
    /// # Safety
    /// `out_device` holds DEVICE pointers sized for `roots.len()` rows; they must stay valid, and unshared with other
    /// runs in flight, until `wait(ticket)` has returned.
    pub unsafe fn run_device_async(
        &self,
        g: &Graph<'_>,
        roots: &[u32],
        run_flags: u32,
        out_device: &sys::hspf_result,
    ) -> Result<u64, Error> {
        let mut ticket = 0u64;
        let rc = sys::hspf_run_device_async(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, run_flags, out_device, &mut ticket);
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(ticket)
    }

    pub fn wait(&self, ticket: u64) -> Result<sys::hspf_stats, Error> {
        let mut st = std::mem::MaybeUninit::<sys::hspf_stats>::zeroed();
        let rc = unsafe { sys::hspf_wait(self.ctx, ticket, st.as_mut_ptr()) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(unsafe { st.assume_init() })
    }

    // ---- several areas, ONE RIB, on the device (ABI 7: hspf_rib_clear_device / hspf_rib_fold_device) ---------------------

    /// The empty instance-wide RIB state in front of the first area (`hspf_rib_clear_device`).
    pub fn rib_new(&self, n_prefixes: u32, words: u32) -> Result<RibDevice<'_>, Error> {
        let (p, w) = (n_prefixes as usize, words as usize);
        let rib = RibDevice {
            n_prefixes,
            words,
            best_metric: self.device_alloc(p.max(1) * 4)?,
            best_entry: self.device_alloc(p.max(1) * 4)?,
            nexthop_mask: self.device_alloc((p * w).max(1) * 8)?,
            origin: self.device_alloc(p.max(1) * 4)?,
        };
        let rc = unsafe { sys::hspf_rib_clear_device(self.ctx, &rib.raw()) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(rib)
    }

    /// `hspf_rib_fold_device`: the literal ordered fold of ONE area's table (`HSPF_PFX_ORDERED`: entries in
    /// `V::intra_area_networks` order with their owners' LS-IDs) into the state the earlier areas left — `update_rib_intra_area`
    /// (holo-ospf/src/route.rs:343-448) for the whole area in one call.  `run` = the area's one-root `run_device`;
    /// `prefix_map[i]` = instance-wide index of the area's prefix i; `word_offset` = where the area's first-hop slots start
    /// in the instance-wide numbering.
    #[allow(clippy::too_many_arguments)]
    pub fn rib_fold(&self, rib: &RibDevice<'_>, run: &DeviceTables<'_>, table: &OrderedPrefixTable, prefix_map: &[u32], area_index: u32, word_offset: u32) -> Result<(), Error> {
        if run.n_roots != 1 || prefix_map.len() != table.n_prefixes() as usize || word_offset + run.words > rib.words {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "rib_fold: one root per area; one map entry per prefix; the area's mask words must fit".into() });
        }
        let t = sys::hspf_prefix_table {
            n_prefixes: table.n_prefixes(),
            n_entries: table.pfx_vertex.len() as u32,
            pfx_ptr: table.pfx_ptr.as_ptr(),
            pfx_vertex: table.pfx_vertex.as_ptr(),
            pfx_metric: table.pfx_metric.as_ptr(),
            flags: table.flags | sys::HSPF_PFX_ORDERED,
            pfx_origin: table.pfx_origin.as_ptr(),
            init_exists: ptr::null(),
            init_metric: ptr::null(),
            init_origin: ptr::null(),
        };
        let rc = unsafe {
            sys::hspf_rib_fold_device(
                self.ctx, run.n_vertices, run.words, run.dist.p as *const u32, run.flags.p as *const u16, run.mask.p as *const u64, &t, prefix_map.as_ptr(), area_index, word_offset, &rib.raw(),
            )
        };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(())
    }

    /// `hspf_run_packed_device`: the packed words of every (root, vertex) left in HBM (a quarter of `run_device`'s bytes, for
    /// consumers that stay on the GPU or send the rows on with `Multi::allgather_rows`); returns the buffer, the layout of the
    /// words and the per-root status (`sys::HSPF_ROOT_EXACT`: the root's pop order is dynamic).
    pub fn run_packed_device(&self, g: &Graph<'_>, roots: &[u32], run_flags: u32) -> Result<(DeviceBuf<'_>, sys::hspf_packed_layout, Vec<u8>), Error> {
        let cap = roots.len() * g.n as usize * 8;
        let buf = self.device_alloc(cap.max(8))?;
        let mut layout = std::mem::MaybeUninit::<sys::hspf_packed_layout>::zeroed();
        let mut status = vec![0u8; roots.len()];
        let rc = unsafe { sys::hspf_run_packed_device(self.ctx, g.g, roots.as_ptr(), roots.len() as u32, run_flags, buf.p, cap, layout.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok((buf, unsafe { layout.assume_init() }, status))
    }

    /// Statistics of the last run on this engine (`hspf_get_stats`): which kernels ran, `n_exact_roots`, `n_repaired_roots`.
    pub fn stats(&self) -> sys::hspf_stats {
        let mut st = std::mem::MaybeUninit::<sys::hspf_stats>::zeroed();
        unsafe {
            sys::hspf_get_stats(self.ctx, st.as_mut_ptr());
            st.assume_init()
        }
    }

    /// Every run handed to a lane is over (`hspf_wait_all`); the number of lanes (`hspf_async_lanes`).
    pub fn wait_all(&self) -> Result<(), Error> {
        let rc = unsafe { sys::hspf_wait_all(self.ctx) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(())
    }
    pub fn async_lanes(&self) -> u32 {
        unsafe { sys::hspf_async_lanes(self.ctx) }
    }
    pub fn device_count() -> i32 {
        unsafe { sys::hspf_device_count() }
    }
}

impl Drop for Engine {
    fn drop(&mut self) {
        for (_, free) in std::mem::take(&mut *self.pool.borrow_mut()) {
            for p in free {
                unsafe { sys::hspf_device_free(self.ctx, p) }
            }
        }
        unsafe { sys::hspf_shutdown(self.ctx) }
    }
}

impl Graph<'_> {
    /// The caller's CSR as it is resident on the device (`hspf_graph_export`: ROW_PTR / COL / METRIC / VFLAGS) — what
    /// `Engine::upload_keyed` built from the LSDB records, for `CsrCache`'s host mirror.
    pub fn export_csr(&self, max_path_metric: u32) -> Result<Csr, Error> {
        fn fetch<T: Clone + Default>(g: &Graph<'_>, which: u32) -> Result<Vec<T>, Error> {
            let mut bytes = 0usize;
            let rc = unsafe { sys::hspf_graph_export(g.eng.ctx, g.g, which, ptr::null_mut(), 0, &mut bytes) };
            if rc != sys::HSPF_OK && bytes == 0 {
                return Err(g.eng.err(rc));
            }
            let mut v = vec![T::default(); bytes / std::mem::size_of::<T>()];
            let rc = unsafe { sys::hspf_graph_export(g.eng.ctx, g.g, which, v.as_mut_ptr() as *mut _, bytes, &mut bytes) };
            if rc != sys::HSPF_OK {
                return Err(g.eng.err(rc));
            }
            Ok(v)
        }
        Ok(Csr {
            row_ptr: fetch::<u32>(self, sys::HSPF_GX_ROW_PTR)?,
            col: fetch::<u32>(self, sys::HSPF_GX_COL)?,
            metric: fetch::<u32>(self, sys::HSPF_GX_METRIC)?,
            vflags: fetch::<u8>(self, sys::HSPF_GX_VFLAGS)?,
            max_path_metric,
        })
    }

    /// Whole rows replaced (the rows of the LSPs / LSAs that triggered the run: `trigger_lsps`, `SpfTriggerLsa`).
    pub fn patch(&mut self, rows: &[RowPatch]) -> Result<(), Error> {
        let vertex: Vec<u32> = rows.iter().map(|r| r.vertex).collect();
        let vflags: Vec<u8> = rows.iter().map(|r| r.vflags).collect();
        let mut row_ptr = Vec::with_capacity(rows.len() + 1);
        let (mut col, mut metric) = (Vec::new(), Vec::new());
        row_ptr.push(0u32);
        for r in rows {
            col.extend_from_slice(&r.col);
            metric.extend_from_slice(&r.metric);
            row_ptr.push(col.len() as u32);
        }
        let p = sys::hspf_rows {
            n_changed: rows.len() as u32,
            vertex: vertex.as_ptr(),
            row_ptr: row_ptr.as_ptr(),
            col: col.as_ptr(),
            metric: metric.as_ptr(),
            vflags: vflags.as_ptr(),
        };
        let rc = unsafe { sys::hspf_graph_patch(self.eng.ctx, self.g, &p) };
        if rc != sys::HSPF_OK {
            return Err(self.eng.err(rc));
        }
        Ok(())
    }

    /// `(vertex, slot base)` of every vertex of H = {root, networks attached to it}: slot `base + j` is the j-th link
    /// of that vertex's row (include/holo_spf_hip.h "first-hop slots").
    pub fn slot_table(&self, root: u32) -> Result<Vec<(u32, u32)>, Error> {
        let mut total = 0u32;
        let cnt = unsafe { sys::hspf_slot_table(self.eng.ctx, self.g, root, ptr::null_mut(), ptr::null_mut(), 0, &mut total) };
        if cnt < 0 {
            return Err(self.eng.err(cnt));
        }
        let (mut hv, mut hb) = (vec![0u32; cnt as usize], vec![0u32; cnt as usize]);
        let rc = unsafe { sys::hspf_slot_table(self.eng.ctx, self.g, root, hv.as_mut_ptr(), hb.as_mut_ptr(), cnt as u32, &mut total) };
        if rc < 0 {
            return Err(self.eng.err(rc));
        }
        Ok(hv.into_iter().zip(hb).collect())
    }
}

impl Drop for Graph<'_> {
    fn drop(&mut self) {
        unsafe { sys::hspf_graph_free(self.eng.ctx, self.g) }
    }
}

/// The resident CSR of one (area | level x topology x metric mode) and what it was built from: `get_or_patch` turns
/// the rows derived from the CURRENT LSDB into either nothing (unchanged), a row patch (`hspf_graph_patch`: same
/// vertex set, some rows differ — what `trigger_lsps` / `SpfTriggerLsa` describe) or a fresh upload (a vertex appeared
/// or vanished).  `K` = the protocol's vertex id (`VertexId`), in the reference's order.
pub struct CsrCache<'e, K: Ord + Clone> {
    pub keys: Vec<K>,
    pub csr: Csr,
    pub graph: Option<Graph<'e>>,
}

impl<'e, K: Ord + Clone> Default for CsrCache<'e, K> {
    fn default() -> Self {
        CsrCache { keys: Vec::new(), csr: Csr::default(), graph: None }
    }
}

impl<'e, K: Ord + Clone> CsrCache<'e, K> {
    pub fn index_of(&self, key: &K) -> Option<u32> {
        self.keys.binary_search(key).ok().map(|i| i as u32)
    }

    /// `keys` ascending, `fresh` = the CSR derived from the LSDB as it is now.
    pub fn get_or_patch(&mut self, eng: &'e Engine, keys: Vec<K>, fresh: Csr) -> Result<&Graph<'e>, Error> {
        let same_shape = self.graph.is_some() && self.keys == keys && self.csr.max_path_metric == fresh.max_path_metric;
        if same_shape {
            let mut rows = Vec::new();
            for v in 0..fresh.n_vertices() {
                let (nc, nm) = fresh.row(v);
                let (oc, om) = self.csr.row(v);
                if nc != oc || nm != om || fresh.vflags[v as usize] != self.csr.vflags[v as usize] {
                    rows.push(RowPatch { vertex: v, col: nc.to_vec(), metric: nm.to_vec(), vflags: fresh.vflags[v as usize] });
                }
            }
            if !rows.is_empty() {
                if let Err(e) = self.graph.as_mut().unwrap().patch(&rows) {
                    // After a failed patch the library's graph is invalid (device arrays and host mirrors may be out of
                    // step; every later call on it returns HSPF_E_INVAL) and `self.csr` no longer describes it: drop the
                    // replica, so that the next call uploads afresh instead of diffing against a stale CSR.  The error
                    // still goes up: the caller falls back to its CPU loop for this run.
                    self.graph = None;
                    self.keys.clear();
                    self.csr = Csr::default();
                    return Err(e);
                }
                self.csr = fresh;
            }
        } else {
            self.graph = None; // frees the old replica first
            self.graph = Some(eng.upload(&fresh)?);
            self.keys = keys;
            self.csr = fresh;
        }
        Ok(self.graph.as_ref().unwrap())
    }
}

/// `hspf_prefix_table` of one OSPF area with `HSPF_PFX_ORDERED`: the entries of a prefix in the order
/// `V::intra_area_networks` yields them, `pfx_origin` = Link State ID of the entry's vertex LSA (the transit-network rule of
/// holo-ospf/src/route.rs:388-400 compares it); network-LSA entries carry `HSPF_PFX_ENTRY_NETWORK` in `pfx_vertex`.
#[derive(Debug, Default, Clone)]
pub struct OrderedPrefixTable {
    pub pfx_ptr: Vec<u32>,
    pub pfx_vertex: Vec<u32>,
    pub pfx_metric: Vec<u32>,
    pub pfx_origin: Vec<u32>,
    pub flags: u32, // HSPF_PFX_SATURATING for OSPF (u32 saturating add, spf.rs:672)
}

impl OrderedPrefixTable {
    pub fn n_prefixes(&self) -> u32 {
        self.pfx_ptr.len().saturating_sub(1) as u32
    }
}

/// The instance-wide RIB state of one OSPF Full computation on the device (`hspf_rib_device`): after the last area's fold
/// `(best_metric, best_entry, nexthop_mask)` IS an `hspf_routes` of one root — `into_routes` hands it to `routes_changed`.
pub struct RibDevice<'e> {
    pub n_prefixes: u32,
    pub words: u32,
    best_metric: DeviceBuf<'e>,
    best_entry: DeviceBuf<'e>,
    nexthop_mask: DeviceBuf<'e>,
    origin: DeviceBuf<'e>,
}

impl<'e> RibDevice<'e> {
    fn raw(&self) -> sys::hspf_rib_device {
        sys::hspf_rib_device {
            n_prefixes: self.n_prefixes,
            n_mask_words: self.words,
            best_metric: self.best_metric.p as *mut u32,
            best_entry: self.best_entry.p as *mut u32,
            nexthop_mask: self.nexthop_mask.p as *mut u64,
            origin: self.origin.p as *mut u32,
        }
    }
    /// Metric, owner (`area_index << 24 | entry`; all ones: no route) and next-hop mask of every prefix, on the host.
    pub fn to_host(&self) -> Result<(Vec<u32>, Vec<u32>, Vec<u64>), Error> {
        let (p, w) = (self.n_prefixes as usize, self.words as usize);
        Ok((self.best_metric.to_host(p)?, self.best_entry.to_host(p)?, self.nexthop_mask.to_host(p * w)?))
    }
    pub fn into_routes(self) -> DeviceRoutes<'e> {
        DeviceRoutes { n_roots: 1, n_prefixes: self.n_prefixes, words: self.words, best_metric: self.best_metric, best_entry: self.best_entry, nexthop_mask: self.nexthop_mask }
    }
}

// ---- several GPUs (include/holo_spf_hip.h "several GPUs") -----------------------------------------------------
// Roots are independent units over a replicated graph: a `Multi` drives the devices of this process (one engine context
// each) or is ONE rank of a job of processes (RCCL: `unique_id` from rank 0, carried by the host's own transport — holo's
// ibus).  Tables are DEVICE buffers the caller owns, one `hspf_result` per local device, sized for ALL roots.

pub struct Multi {
    m: *mut sys::hspf_multi,
}

pub struct MultiGraph<'m> {
    multi: &'m Multi,
    g: *mut sys::hspf_multi_graph,
    pub n: u32,
}

impl Multi {
    fn err(&self, code: i32) -> Error {
        let detail = unsafe { CStr::from_ptr(sys::hspf_multi_last_error(self.m)) }.to_string_lossy().into_owned();
        Error { code, detail }
    }

    /// Rank 0 of a job of processes: the communicator id every rank passes to `new` (`hspf_multi_unique_id`; needs librccl.so).
    pub fn unique_id() -> Result<[u8; sys::HSPF_COMM_ID_BYTES as usize], Error> {
        let mut id = [0u8; sys::HSPF_COMM_ID_BYTES as usize];
        let rc = unsafe { sys::hspf_multi_unique_id(id.as_mut_ptr()) };
        if rc != sys::HSPF_OK {
            return Err(Error { code: rc, detail: "hspf_multi_unique_id (librccl.so)".into() });
        }
        Ok(id)
    }

    /// `unique_id == None`: one process drives every device (`world == device_ordinals.len()`, peer copies over xGMI);
    /// `Some(id)`: this process is the ranks `first_rank ..` of a job of `world` ranks (RCCL).
    pub fn new(device_ordinals: &[i32], world: u32, first_rank: u32, unique_id: Option<&[u8; sys::HSPF_COMM_ID_BYTES as usize]>) -> Result<Self, Error> {
        let cfg = sys::hspf_multi_config {
            n_local: device_ordinals.len() as u32,
            device_ordinals: device_ordinals.as_ptr(),
            world,
            first_rank,
            unique_id: unique_id.map_or(ptr::null(), |id| id.as_ptr()),
        };
        let mut m = ptr::null_mut();
        let rc = unsafe { sys::hspf_multi_init(&cfg, &mut m) };
        if rc != sys::HSPF_OK {
            let detail = unsafe { CStr::from_ptr(sys::hspf_multi_init_error()) }.to_string_lossy().into_owned();
            return Err(Error { code: rc, detail });
        }
        Ok(Multi { m })
    }

    pub fn n_local(&self) -> u32 {
        unsafe { sys::hspf_multi_n_local(self.m) }
    }

    /// A replica of the graph on every local device.
    pub fn upload(&self, csr: &Csr) -> Result<MultiGraph<'_>, Error> {
        let c = sys::hspf_csr {
            n_vertices: csr.n_vertices(),
            n_edges: csr.col.len() as u32,
            row_ptr: csr.row_ptr.as_ptr(),
            col: csr.col.as_ptr(),
            metric: csr.metric.as_ptr(),
            vflags: csr.vflags.as_ptr(),
            max_path_metric: csr.max_path_metric,
        };
        let mut g = ptr::null_mut();
        let rc = unsafe { sys::hspf_multi_graph_upload(self.m, &c, &mut g) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(MultiGraph { multi: self, g, n: csr.n_vertices() })
    }

    /// `[begin, end)` of `rank` in a list of `n_roots` roots: whole 64-root batches (`hspf_shard_bounds`).
    pub fn shard_bounds(n_roots: u32, world: u32, rank: u32) -> (u32, u32) {
        let (mut b, mut e) = (0u32, 0u32);
        unsafe { sys::hspf_shard_bounds(n_roots, world, rank, &mut b, &mut e) };
        (b, e)
    }

    /// Areas first, then roots (multi-area OSPF, BASELINE configs[3]): the (rank, area, root range) slices of `hspf_plan_areas`.
    pub fn plan_areas(roots_per_area: &[u32], world: u32) -> Vec<sys::hspf_area_slice> {
        let cap = roots_per_area.len() as u32 + world;
        let mut out = vec![sys::hspf_area_slice { rank: 0, area: 0, root_begin: 0, root_end: 0 }; cap as usize];
        let k = unsafe { sys::hspf_plan_areas(roots_per_area.len() as u32, roots_per_area.as_ptr(), world, out.as_mut_ptr(), cap) };
        out.truncate(k.min(cap) as usize);
        out
    }

    pub fn mask_words(&self, g: &MultiGraph<'_>, roots: &[u32]) -> Result<u32, Error> {
        let mut w = 0u32;
        let rc = unsafe { sys::hspf_multi_mask_words(self.m, g.g, roots.as_ptr(), roots.len() as u32, &mut w) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(w)
    }

    /// Sharded run + the all-gather of the tables selected in `gather` (the `HSPF_GATHER_*` bits of `sys`).
    ///
    /// # Safety
    /// `all[i]` holds DEVICE pointers on local device i sized for ALL `roots.len()` rows; valid until the call (or, with
    /// `HSPF_GATHER_ASYNC`, `wait`) has returned.
    pub unsafe fn run(&self, g: &MultiGraph<'_>, roots: &[u32], run_flags: u32, all: &mut [sys::hspf_result], gather: u32) -> Result<(), Error> {
        if all.len() != self.n_local() as usize {
            return Err(Error { code: sys::HSPF_E_INVAL, detail: "Multi::run: one hspf_result per local device".into() });
        }
        let rc = sys::hspf_multi_run(self.m, g.g, roots.as_ptr(), roots.len() as u32, run_flags, all.as_mut_ptr(), gather);
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(())
    }

    /// The two halves of `run` (several steps in flight, into DIFFERENT tables; wait in ticket order on every rank).
    ///
    /// # Safety
    /// As `run`; the tables of a ticket must not be shared with another ticket in flight.
    pub unsafe fn run_async(&self, g: &MultiGraph<'_>, roots: &[u32], run_flags: u32, all: &[sys::hspf_result]) -> Result<u64, Error> {
        let mut ticket = 0u64;
        let rc = sys::hspf_multi_run_async(self.m, g.g, roots.as_ptr(), roots.len() as u32, run_flags, all.as_ptr(), &mut ticket);
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(ticket)
    }
    /// # Safety
    /// `all` = the tables the ticket was started with.
    pub unsafe fn run_wait(&self, ticket: u64, all: &mut [sys::hspf_result], gather: u32) -> Result<(), Error> {
        let rc = sys::hspf_multi_run_wait(self.m, ticket, all.as_mut_ptr(), gather);
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(())
    }

    /// Pending asynchronous gathers are over (`hspf_multi_wait`).
    pub fn wait(&self) -> Result<(), Error> {
        let rc = unsafe { sys::hspf_multi_wait(self.m) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(())
    }

    /// The collective on its own, for any per-root table (route tables after `routes_device`: "a single all-gather of
    /// per-root route tables").
    ///
    /// # Safety
    /// `tables[i]`: a device buffer on local device i of `n_roots` rows of `row_bytes` bytes whose own rows are filled.
    pub unsafe fn allgather_rows(&self, tables: &[*mut c_void], row_bytes: usize, n_roots: u32) -> Result<(), Error> {
        let rc = sys::hspf_multi_allgather_rows(self.m, tables.as_ptr(), row_bytes, n_roots);
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(())
    }

    pub fn stats(&self, local_index: u32) -> Result<sys::hspf_stats, Error> {
        let mut st = std::mem::MaybeUninit::<sys::hspf_stats>::zeroed();
        let rc = unsafe { sys::hspf_multi_get_stats(self.m, local_index, st.as_mut_ptr()) };
        if rc != sys::HSPF_OK {
            return Err(self.err(rc));
        }
        Ok(unsafe { st.assume_init() })
    }

    /// The context of local device `i`, for the one-device calls (`hspf_device_alloc`, `hspf_routes_device` ...) on that rank.
    pub fn ctx_raw(&self, local_index: u32) -> *mut sys::hspf_ctx {
        unsafe { sys::hspf_multi_ctx(self.m, local_index) }
    }
}

impl Drop for Multi {
    fn drop(&mut self) {
        unsafe { sys::hspf_multi_shutdown(self.m) }
    }
}

impl MultiGraph<'_> {
    /// Whole rows replaced on every replica (`hspf_multi_graph_patch`).
    pub fn patch(&mut self, rows: &[RowPatch]) -> Result<(), Error> {
        let vertex: Vec<u32> = rows.iter().map(|r| r.vertex).collect();
        let vflags: Vec<u8> = rows.iter().map(|r| r.vflags).collect();
        let mut row_ptr = vec![0u32];
        let (mut col, mut metric) = (Vec::new(), Vec::new());
        for r in rows {
            col.extend_from_slice(&r.col);
            metric.extend_from_slice(&r.metric);
            row_ptr.push(col.len() as u32);
        }
        let p = sys::hspf_rows { n_changed: rows.len() as u32, vertex: vertex.as_ptr(), row_ptr: row_ptr.as_ptr(), col: col.as_ptr(), metric: metric.as_ptr(), vflags: vflags.as_ptr() };
        let rc = unsafe { sys::hspf_multi_graph_patch(self.multi.m, self.g, &p) };
        if rc != sys::HSPF_OK {
            return Err(self.multi.err(rc));
        }
        Ok(())
    }
    /// The replica on local device `i` (`hspf_multi_graph_local`), for the one-device calls on that rank's context.
    pub fn local_raw(&self, local_index: u32) -> *mut sys::hspf_graph {
        unsafe { sys::hspf_multi_graph_local(self.g, local_index) }
    }
}

impl Drop for MultiGraph<'_> {
    fn drop(&mut self) {
        unsafe { sys::hspf_multi_graph_free(self.multi.m, self.g) }
    }
}
