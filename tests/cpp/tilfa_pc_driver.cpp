// tilfa_pc_driver.cpp — TI-LFA repairs along the post-convergence path through the compiled layers, against expected values the
// Python model wrote.
//   tilfa_pc_driver --engine host [--out-dir DIR] <case files...>
//                                                      the sequential host twin (hspf::host::tilfa_pc_sequential) on the tables of the
//                                                      file: no device; with --out-dir what it returned is written to DIR/<case>.out, one
//                                                      array per line in the order of the expected arrays
//   tilfa_pc_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                      the host interface's default on an engine without the call:
//                                                      TilfaPcOut::supported == false, nothing else filled in
//   tilfa_pc_driver --engine hip <case files...>       the RAII layer (hspf::Engine::tilfa_pc_device on the file's tables, copied to
//                                                      the device) AND the host interface (hspf::host::HipEngine: its own runs, lfa,
//                                                      rlfa with the space tables, run_failures, tilfa_pc), every array compared
// A case file is a list of decimal numbers (tests/test_cpp_tilfa_pc.py writes them from tests/_tilfa_pc_model.py):
//   n e max_path root run_flags lfa_flags max_walk | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | W dist[R n] flags[R n] mask[R n W] | has_alt alt_flags[n] | space_flags[S n] space_via[S n] |
//   n_pc pc_row[S] pc_dist[n_pc n] | tp_kind[n] tp_p[n] tp_via[n] tp_q[n] tp_n_adj[n] tp_hop_pos[4n] tp_hop_head[4n] tp_metric[n] tp_flags[n]
//   tp_coverage[12]                                                                                                   (S = 64 W)
// Built by build() and by tests/test_cpp_tilfa_pc.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, lfa_flags = 0, max_walk = 0, K = 0, R = 0, W = 0, has_alt = 0, n_pc = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row, dist, space_via, pc_row, pc_dist;
  std::vector<uint16_t> flags;
  std::vector<uint64_t> mask;
  std::vector<uint8_t> vflags, cflags, alt, space_flags;
  hspf::host::TilfaPcOut want;
};

template <typename T>
void take(std::istream &in, std::vector<T> &v, size_t count) {
  v.resize(count);
  for (size_t i = 0; i < count; ++i) { uint64_t x; in >> x; v[i] = (T)x; }
}

Case load(const char *path) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error(std::string("cannot open ") + path);
  Case c;
  in >> c.n >> c.e >> c.maxp >> c.root >> c.run_flags >> c.lfa_flags >> c.max_walk;
  take(in, c.row_ptr, (size_t)c.n + 1); take(in, c.col, c.e); take(in, c.metric, c.e); take(in, c.vflags, c.n);
  in >> c.K;
  take(in, c.nbr, c.K); take(in, c.cost, c.K); take(in, c.root_link, c.K); take(in, c.cflags, c.K);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.nbr_row, c.K);
  in >> c.W;
  const size_t n = c.n, S = 64u * (size_t)c.W, rn = (size_t)c.R * n;
  take(in, c.dist, rn); take(in, c.flags, rn); take(in, c.mask, rn * c.W);
  in >> c.has_alt;
  take(in, c.alt, n);
  take(in, c.space_flags, S * n); take(in, c.space_via, S * n);
  in >> c.n_pc;
  take(in, c.pc_row, S); take(in, c.pc_dist, (size_t)c.n_pc * n);
  hspf::host::TilfaPcOut &w = c.want;
  take(in, w.tp_kind, n); take(in, w.tp_p, n); take(in, w.tp_via, n); take(in, w.tp_q, n); take(in, w.tp_n_adj, n);
  take(in, w.tp_hop_pos, n * HSPF_TIPC_MAX_ADJ); take(in, w.tp_hop_head, n * HSPF_TIPC_MAX_ADJ); take(in, w.tp_metric, n); take(in, w.tp_flags, n);
  take(in, w.tp_coverage, HSPF_TIPC_COVERAGE_WORDS);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

template <typename A, typename B>
size_t differ(const char *who, const char *what, const A &got, const B &want, size_t count) {
  size_t bad = got.size() < count ? 1 : 0;
  if (bad) { printf("  %s %s: %zu entries, want %zu\n", who, what, got.size(), count); return bad; }
  for (size_t i = 0; i < count; ++i)
    if ((uint64_t)got[i] != (uint64_t)want[i]) {
      if (!bad) printf("  %s %s[%zu]: got %llu, want %llu\n", who, what, i, (unsigned long long)got[i], (unsigned long long)want[i]);
      ++bad;
    }
  return bad;
}

void dump(const std::string &path, const hspf::host::TilfaPcOut &o) {
  std::ofstream out(path);
  auto line = [&](const auto &v) { for (auto x : v) out << (uint64_t)x << ' '; out << '\n'; };
  line(o.tp_kind); line(o.tp_p); line(o.tp_via); line(o.tp_q); line(o.tp_n_adj); line(o.tp_hop_pos); line(o.tp_hop_head); line(o.tp_metric); line(o.tp_flags);
  line(o.tp_coverage);
  if (!out) throw std::runtime_error("cannot write " + path);
}

size_t differ_all(const char *who, const hspf::host::TilfaPcOut &o, const Case &c) {
  const hspf::host::TilfaPcOut &w = c.want;
  const size_t n = c.n, A = HSPF_TIPC_MAX_ADJ;
  if (!o.supported || o.n_protected != 1 || o.n_vertices != c.n) { printf("  %s: unsupported or shape differs\n", who); return 1; }
  size_t b = differ(who, "tp_kind", o.tp_kind, w.tp_kind, n) + differ(who, "tp_p", o.tp_p, w.tp_p, n) + differ(who, "tp_via", o.tp_via, w.tp_via, n) +
             differ(who, "tp_q", o.tp_q, w.tp_q, n) + differ(who, "tp_n_adj", o.tp_n_adj, w.tp_n_adj, n) + differ(who, "tp_hop_pos", o.tp_hop_pos, w.tp_hop_pos, n * A) +
             differ(who, "tp_hop_head", o.tp_hop_head, w.tp_hop_head, n * A) + differ(who, "tp_metric", o.tp_metric, w.tp_metric, n) +
             differ(who, "tp_flags", o.tp_flags, w.tp_flags, n) + differ(who, "tp_coverage", o.tp_coverage, w.tp_coverage, HSPF_TIPC_COVERAGE_WORDS);
  // segments(): the list of a repair chains from p to q over links of the CSR
  for (uint32_t d = 0; d < c.n && !b; ++d) {
    uint32_t via, p, q;
    std::vector<hspf::host::TilfaPcOut::Hop> hops;
    if (!o.segments(0, d, via, p, hops, q)) { b += w.tp_kind[d] == HSPF_TIPC_D_REPAIR; continue; }
    uint32_t tail = p;
    for (const auto &h : hops) {
      if (h.tail != tail || h.pos >= c.row_ptr[tail + 1] - c.row_ptr[tail] || c.col[c.row_ptr[tail] + h.pos] != h.head) { printf("  %s: segments(%u) is no path\n", who, d); ++b; break; }
      tail = h.head;
    }
    if (tail != q) { printf("  %s: segments(%u) does not end at q\n", who, d); ++b; }
  }
  return b;
}

struct DevCopy {                                                    // a host array on the device for the RAII leg
  void *p = nullptr;
  template <typename T> explicit DevCopy(const std::vector<T> &v) {
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 8);
    if (hipMalloc(&p, bytes) != hipSuccess) throw std::runtime_error("hipMalloc");
    if (!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy");
  }
  explicit DevCopy(size_t bytes) { if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) throw std::runtime_error("hipMalloc"); }
  DevCopy(const DevCopy &) = delete;
  ~DevCopy() { if (p) (void)hipFree(p); }
  template <typename T> T *as() const { return (T *)p; }
  template <typename T> std::vector<T> host(size_t count) const {
    std::vector<T> v(count);
    if (count && hipMemcpy(v.data(), p, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy");
    return v;
  }
};

}  // namespace

int main(int argc, char **argv) {
  std::string engine = "hip", oracle_so = "oracle/liboracle_spf.so", out_dir;
  std::vector<const char *> files;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--engine") && i + 1 < argc) engine = argv[++i];
    else if (!strcmp(argv[i], "--oracle-so") && i + 1 < argc) oracle_so = argv[++i];
    else if (!strcmp(argv[i], "--out-dir") && i + 1 < argc) out_dir = argv[++i];
    else files.push_back(argv[i]);
  }
  try {
    size_t cases = 0, compared = 0, bad = 0, unsupported = 0;
    for (const char *f : files) {
      const Case c = load(f);
      ++cases;
      const size_t n = c.n, A = HSPF_TIPC_MAX_ADJ;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      if (engine == "host") {
        hspf::host::Tables fwd;
        fwd.n_roots = c.R; fwd.n_vertices = c.n; fwd.mask_words = c.W; fwd.dist = c.dist; fwd.flags = c.flags; fwd.mask = c.mask;
        const hspf::host::TilfaPcOut o = hspf::host::tilfa_pc_sequential(c.row_ptr, c.col, c.metric, c.vflags, fwd, {hp}, c.space_flags, c.space_via,
                                                                          c.has_alt ? &c.alt : nullptr, c.pc_dist, c.n_pc, c.pc_row, c.run_flags, c.max_walk);
        if (!out_dir.empty()) {
          const std::string name(f);
          dump(out_dir + "/" + name.substr(name.find_last_of('/') + 1) + ".out", o);
        }
        const size_t b = differ_all("twin", o, c);
        if (b) printf("  %s\n", f);
        bad += b; compared += n;
        continue;
      }
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        const hspf::host::TilfaPcOut o = static_cast<hspf::host::Engine &>(eng).tilfa_pc(*g, *run, *run, {hp}, c.lfa_flags, nullptr, hspf::host::RlfaOut{}, c.pc_dist,
                                                                                         c.n_pc, c.pc_row, c.run_flags, c.max_walk);
        if (!o.supported && o.tp_kind.empty() && o.tp_p.empty() && o.tp_hop_pos.empty() && o.tp_coverage.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      {   // the RAII layer on the file's tables
        hspf::Engine eng(0);
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        DevCopy dist(c.dist), flags(c.flags), mask(c.mask), alt(c.alt), sf(c.space_flags), sv(c.space_via), pcd(c.pc_dist);
        DevCopy kind(n), p(n * 4), via(n * 4), q(n * 4), nadj(n), hpos(n * A * 4), hhead(n * A * 4), met(n * 4), fl(n), cov(HSPF_TIPC_COVERAGE_WORDS * 4);
        const hspf_lfa_protect pr{c.root, 0, c.K, c.nbr.data(), c.nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()};
        eng.tilfa_pc_device(g, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), dist.as<uint32_t>(), {pr}, c.lfa_flags,
                            c.has_alt ? alt.as<uint8_t>() : nullptr, sf.as<uint8_t>(), sv.as<uint32_t>(), pcd.as<uint32_t>(), c.n_pc, c.pc_row, c.run_flags, c.max_walk,
                            hspf_tilfa_pc_out{kind.as<uint8_t>(), p.as<uint32_t>(), via.as<uint32_t>(), q.as<uint32_t>(), nadj.as<uint8_t>(), hpos.as<uint32_t>(),
                                              hhead.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cov.as<uint32_t>()});
        hspf::host::TilfaPcOut o;
        o.supported = true; o.n_protected = 1; o.n_vertices = c.n;
        o.tp_kind = kind.host<uint8_t>(n); o.tp_p = p.host<uint32_t>(n); o.tp_via = via.host<uint32_t>(n); o.tp_q = q.host<uint32_t>(n);
        o.tp_n_adj = nadj.host<uint8_t>(n); o.tp_hop_pos = hpos.host<uint32_t>(n * A); o.tp_hop_head = hhead.host<uint32_t>(n * A);
        o.tp_metric = met.host<uint32_t>(n); o.tp_flags = fl.host<uint8_t>(n); o.tp_coverage = cov.host<uint32_t>(HSPF_TIPC_COVERAGE_WORDS);
        b += differ_all("raii", o, c);
      }
      {   // the host interface on the product engine: its own tables, space tables and failure rows
        hspf::host::HipEngine heng(0);
        auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        const hspf::Engine::Transposed t = hspf::Engine::csr_transpose(c.row_ptr, c.col, c.metric, c.vflags);
        auto hgt = heng.upload(t.row_ptr, t.col, t.metric, c.vflags, c.maxp);
        auto run = heng.run_device(*hg, c.roots, c.run_flags);
        auto rrun = heng.run_device(*hgt, c.roots, c.run_flags);
        const hspf::host::LfaOut lo = heng.lfa(*run, {hp}, c.lfa_flags, false);
        const hspf::host::RlfaOut ro = heng.rlfa(*hg, *run, *rrun, {hp}, c.lfa_flags, c.has_alt ? &lo : nullptr, true);
        // the rows in the file's order: pc_row names them
        std::vector<uint32_t> froots(c.n_pc, c.root);
        std::vector<hspf::host::Failure> fails(c.n_pc);
        for (size_t e = 0; e < c.pc_row.size(); ++e)
          if (c.pc_row[e] != HSPF_NO_ROOT) { fails[c.pc_row[e]].kind = HSPF_FAIL_ROOT_LINK; fails[c.pc_row[e]].arg = c.root_link[e]; }
        std::vector<uint32_t> pcd;
        if (c.n_pc) pcd = heng.run_failures(*hg, froots, fails, c.run_flags).dist;
        if (pcd != c.pc_dist) { printf("  %s: host interface: the failure rows differ from the model's\n", f); ++b; }
        // the engine's own run has the mask words ITS roots need (the file's W may be wider): pc_row at that run's slot stride
        std::vector<uint32_t> prow(c.pc_row.begin(), c.pc_row.begin() + std::min<size_t>(c.pc_row.size(), ro.slot_stride));
        prow.resize(ro.slot_stride, HSPF_NO_ROOT);
        const hspf::host::TilfaPcOut o = heng.tilfa_pc(*hg, *run, *rrun, {hp}, c.lfa_flags, c.has_alt ? &lo : nullptr, ro, pcd, c.n_pc, prow, c.run_flags, c.max_walk);
        b += differ_all("host interface", o, c);
      }
      if (b) printf("  %s\n", f);
      compared += 2 * n;
      bad += b;
    }
    printf("%zu cases, %zu destinations compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "tilfa_pc_driver: %s\n", e.what());
    return 2;
  }
}
