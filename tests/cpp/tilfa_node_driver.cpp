// tilfa_node_driver.cpp — two-segment node-protecting repairs through the compiled layers, against expected values the Python model
// wrote.
//   tilfa_node_driver --engine hip <case files...>               the RAII layer (hspf::Engine: lfa_device, rlfa_device with space_flags,
//                                                                tilfa_node_select_device, a run of the listed q's, tilfa_node_device,
//                                                                on DeviceBuffers), its one-root convenience (hspf::Engine::tilfa_node:
//                                                                the whole chain from a graph and a root) AND the host interface
//                                                                (hspf::host::HipEngine::tilfa_node on a DeviceRun, an RlfaOut and the
//                                                                RlfaNodeOut of rlfa_node), every array compared
//   tilfa_node_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                                the host interface's default on an engine without the call:
//                                                                TilfaNodeOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_tilfa_node.py writes them from tests/_tilfa_node_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | W M tq_q[SM] tq_p[SM] tq_link[SM] tq_via[SM] tq_metric[SM] tq_count[S] | Y y_roots[Y] | nd_kind_in[n] |
//   tn_kind[n] tn_p[n] tn_q[n] tn_link[n] tn_via[n] tn_metric[n] tn_set[n] tn_coverage[6]                  (S = 64 W, M = max_pairs)
// nd_kind_in is the RLFA-node model's nd_kind for max_pq = 16: the RAII leg uploads it, the convenience and the host leg compute
// their own with the RLFA-node calls.
// Built by build() (holo_amd/build.py: build_driver); tests/test_cpp_tilfa_node.py rebuilds it when it is older than its sources.
// TEST INFRASTRUCTURE.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, K = 0, R = 0, W = 0, M = 0, Y = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row;
  std::vector<uint32_t> tq_q, tq_p, tq_link, tq_via, tq_metric, tq_count, y_roots, tn_p, tn_q, tn_link, tn_via, tn_metric, tn_set, tn_coverage;
  std::vector<uint8_t> vflags, cflags, nd_kind_in, tn_kind;
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
  in >> c.n >> c.e >> c.maxp >> c.root >> c.run_flags;
  take(in, c.row_ptr, (size_t)c.n + 1); take(in, c.col, c.e); take(in, c.metric, c.e); take(in, c.vflags, c.n);
  in >> c.K;
  take(in, c.nbr, c.K); take(in, c.cost, c.K); take(in, c.root_link, c.K); take(in, c.cflags, c.K);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.nbr_row, c.K);
  in >> c.W >> c.M;
  const size_t S = 64u * (size_t)c.W, SM = S * c.M;
  take(in, c.tq_q, SM); take(in, c.tq_p, SM); take(in, c.tq_link, SM); take(in, c.tq_via, SM); take(in, c.tq_metric, SM); take(in, c.tq_count, S);
  in >> c.Y;
  take(in, c.y_roots, c.Y);
  take(in, c.nd_kind_in, c.n);
  take(in, c.tn_kind, c.n); take(in, c.tn_p, c.n); take(in, c.tn_q, c.n); take(in, c.tn_link, c.n); take(in, c.tn_via, c.n); take(in, c.tn_metric, c.n);
  take(in, c.tn_set, c.n);
  take(in, c.tn_coverage, HSPF_TN_COVERAGE_WORDS);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

template <typename A, typename B>
size_t differ(const char *what, const A &got, const B &want, size_t count) {
  if (got.size() < count) { printf("  %s: %zu entries, want %zu\n", what, (size_t)got.size(), count); return 1; }
  size_t bad = 0;
  for (size_t i = 0; i < count; ++i)
    if ((uint64_t)got[i] != (uint64_t)want[i]) {
      if (!bad) printf("  %s[%zu]: got %llu, want %llu\n", what, i, (unsigned long long)got[i], (unsigned long long)want[i]);
      ++bad;
    }
  return bad;
}

void run_rows(hspf_ctx *ctx, hspf_graph *g, const std::vector<uint32_t> &roots, uint32_t run_flags, hspf_result out) {
  const int rc = hspf_run_device(ctx, g, roots.data(), (uint32_t)roots.size(), run_flags, &out);
  if (rc != HSPF_OK) throw std::runtime_error(std::string("hspf_run_device: ") + hspf_last_error(ctx));
}

}  // namespace

int main(int argc, char **argv) {
  std::string engine = "hip", oracle_so = "oracle/liboracle_spf.so";
  std::vector<const char *> files;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--engine") && i + 1 < argc) engine = argv[++i];
    else if (!strcmp(argv[i], "--oracle-so") && i + 1 < argc) oracle_so = argv[++i];
    else files.push_back(argv[i]);
  }
  try {
    size_t cases = 0, compared = 0, bad = 0, unsupported = 0;
    for (const char *f : files) {
      const Case c = load(f);
      ++cases;
      const size_t S = 64u * (size_t)c.W, SM = S * c.M, n = c.n;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        const hspf::host::TilfaNodeOut o = static_cast<hspf::host::Engine &>(eng).tilfa_node(*g, *run, {hp}, c.run_flags, 0, nullptr, hspf::host::RlfaOut{}, nullptr, c.M);
        if (!o.supported && o.tq_q.empty() && o.tq_count.empty() && o.y_roots.empty() && o.tn_kind.empty() && o.tn_coverage.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      {
        // the RAII layer, on device buffers of its own
        hspf::Engine eng(0);
        hspf_ctx *ctx = eng.raw();
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        const hspf::Engine::Transposed t = hspf::Engine::csr_transpose(c.row_ptr, c.col, c.metric, c.vflags);
        hspf::Graph gt = eng.upload(t.row_ptr, t.col, t.metric, c.vflags, c.maxp);
        const size_t rn = (size_t)c.R * n;
        hspf::DeviceBuffer dist(ctx, rn * 4), flags(ctx, rn * 2), mask(ctx, rn * 8 * c.W), rdist(ctx, rn * 4);
        run_rows(ctx, g.raw(), c.roots, c.run_flags, hspf_result{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), c.W, nullptr});
        run_rows(ctx, gt.raw(), c.roots, c.run_flags, hspf_result{rdist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr});
        const std::vector<hspf_lfa_protect> p{{c.root, 0u, c.K, c.nbr.data(), c.nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()}};
        hspf::DeviceBuffer slot(ctx, n * 4), met(ctx, n * 4), fl(ctx, n), cov(ctx, HSPF_LFA_COVERAGE_WORDS * 4);
        eng.lfa_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, 0,
                       hspf_lfa_out{slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), nullptr, nullptr, cov.as<uint32_t>()});
        hspf::DeviceBuffer pn(ctx, S * 4), pv(ctx, S * 4), pm(ctx, S * 4), pc(ctx, S * 4 * HSPF_RLFA_COUNT_WORDS), sf(ctx, S * n), rln(ctx, n * 4), rlv(ctx, n * 4),
            rlc(ctx, HSPF_RLFA_COVERAGE_WORDS * 4);
        eng.rlfa_device(g, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), rdist.as<uint32_t>(), p, 0, fl.as<uint8_t>(),
                        hspf_rlfa_out{pn.as<uint32_t>(), pv.as<uint32_t>(), pm.as<uint32_t>(), pc.as<uint32_t>(), sf.as<uint8_t>(), nullptr, rln.as<uint32_t>(),
                                      rlv.as<uint32_t>(), rlc.as<uint32_t>()});
        hspf::DeviceBuffer qq(ctx, SM * 4), qp(ctx, SM * 4), ql(ctx, SM * 4), qv(ctx, SM * 4), qm(ctx, SM * 4), qc(ctx, S * 4);
        const hspf_tilfa_node_sel sel{qq.as<uint32_t>(), qp.as<uint32_t>(), ql.as<uint32_t>(), qv.as<uint32_t>(), qm.as<uint32_t>(), qc.as<uint32_t>()};
        eng.tilfa_node_select_device(g, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, 0, sf.as<uint8_t>(), c.M, sel);
        const std::vector<uint32_t> qs = qq.to_host<uint32_t>(SM);
        std::vector<uint32_t> y;
        for (uint32_t v : qs) if (v != HSPF_NO_ROOT) y.push_back(v);
        std::sort(y.begin(), y.end());
        y.erase(std::unique(y.begin(), y.end()), y.end());
        if (y.empty()) y.push_back(HSPF_NO_ROOT);
        hspf::DeviceBuffer ydist(ctx, y.size() * n * 4);
        run_rows(ctx, g.raw(), y, c.run_flags, hspf_result{ydist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr});
        hspf::DeviceBuffer ndk(ctx, n);
        if (hipMemcpy(ndk.as<uint8_t>(), c.nd_kind_in.data(), n, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy of nd_kind_in");
        hspf::DeviceBuffer dk(ctx, n), dp(ctx, n * 4), dq(ctx, n * 4), dl(ctx, n * 4), dv(ctx, n * 4), dm(ctx, n * 4), ds(ctx, n * 4), dc(ctx, HSPF_TN_COVERAGE_WORDS * 4);
        eng.tilfa_node_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, ydist.as<uint32_t>(), y, sel, c.M, fl.as<uint8_t>(),
                              ndk.as<uint8_t>(),
                              hspf_tilfa_node_out{dk.as<uint8_t>(), dp.as<uint32_t>(), dq.as<uint32_t>(), dl.as<uint32_t>(), dv.as<uint32_t>(), dm.as<uint32_t>(),
                                                  ds.as<uint32_t>(), dc.as<uint32_t>()});
        if (y != c.y_roots) { printf("  %s: the union of the lists differs\n", f); ++b; }
        b += differ("tq_q", qs, c.tq_q, SM) + differ("tq_p", qp.to_host<uint32_t>(SM), c.tq_p, SM) + differ("tq_link", ql.to_host<uint32_t>(SM), c.tq_link, SM);
        b += differ("tq_via", qv.to_host<uint32_t>(SM), c.tq_via, SM) + differ("tq_metric", qm.to_host<uint32_t>(SM), c.tq_metric, SM);
        b += differ("tq_count", qc.to_host<uint32_t>(S), c.tq_count, S) + differ("tn_kind", dk.to_host<uint8_t>(n), c.tn_kind, n) + differ("tn_p", dp.to_host<uint32_t>(n), c.tn_p, n);
        b += differ("tn_q", dq.to_host<uint32_t>(n), c.tn_q, n) + differ("tn_link", dl.to_host<uint32_t>(n), c.tn_link, n) + differ("tn_via", dv.to_host<uint32_t>(n), c.tn_via, n);
        b += differ("tn_metric", dm.to_host<uint32_t>(n), c.tn_metric, n) + differ("tn_set", ds.to_host<uint32_t>(n), c.tn_set, n);
        b += differ("tn_coverage", dc.to_host<uint32_t>(HSPF_TN_COVERAGE_WORDS), c.tn_coverage, HSPF_TN_COVERAGE_WORDS);
      }
      {
        // the one-root convenience of the RAII layer: the whole chain from the graph and the root
        hspf::Engine eng(0);
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        const hspf::TilfaNode t = eng.tilfa_node(g, c.row_ptr, c.col, c.metric, c.vflags, c.maxp, c.root, c.run_flags, 0, false, 16, c.M);
        if (t.rlfa.slot_stride != S || t.rlfa.lfa.roots != c.roots || t.max_pairs != c.M || t.y_roots != c.y_roots) { printf("  %s: convenience: shape, roots or y_roots differ\n", f); ++b; }
        else
          b += differ("conv nd_kind", t.nd_kind, c.nd_kind_in, n) + differ("conv tq_q", t.tq_q, c.tq_q, SM) + differ("conv tq_p", t.tq_p, c.tq_p, SM) +
               differ("conv tq_link", t.tq_link, c.tq_link, SM) + differ("conv tq_via", t.tq_via, c.tq_via, SM) + differ("conv tq_metric", t.tq_metric, c.tq_metric, SM) +
               differ("conv tq_count", t.tq_count, c.tq_count, S) + differ("conv tn_kind", t.tn_kind, c.tn_kind, n) + differ("conv tn_p", t.tn_p, c.tn_p, n) +
               differ("conv tn_q", t.tn_q, c.tn_q, n) + differ("conv tn_link", t.tn_link, c.tn_link, n) + differ("conv tn_via", t.tn_via, c.tn_via, n) +
               differ("conv tn_metric", t.tn_metric, c.tn_metric, n) + differ("conv tn_set", t.tn_set, c.tn_set, n) +
               differ("conv tn_coverage", std::vector<uint32_t>(t.tn_coverage, t.tn_coverage + HSPF_TN_COVERAGE_WORDS), c.tn_coverage, HSPF_TN_COVERAGE_WORDS);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::Engine::Transposed t = hspf::Engine::csr_transpose(c.row_ptr, c.col, c.metric, c.vflags);
      auto hgt = heng.upload(t.row_ptr, t.col, t.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      auto rrun = heng.run_device(*hgt, c.roots, c.run_flags);
      const hspf::host::LfaOut lo = heng.lfa(*run, {hp}, 0, false);
      const hspf::host::RlfaOut ro = heng.rlfa(*hg, *run, *rrun, {hp}, 0, &lo, true);
      const hspf::host::RlfaNodeOut no = heng.rlfa_node(*hg, *run, {hp}, c.run_flags, 0, &lo, ro, 16);
      b += differ("host nd_kind (the input)", no.nd_kind, c.nd_kind_in, n);
      const hspf::host::TilfaNodeOut o = heng.tilfa_node(*hg, *run, {hp}, c.run_flags, 0, &lo, ro, &no, c.M);
      if (!o.supported || o.slot_stride != S || o.n_vertices != c.n || o.max_pairs != c.M || o.y_roots != c.y_roots) { printf("  %s: host interface: unsupported, or shape or y_roots differ\n", f); ++b; }
      else
        b += differ("host tq_q", o.tq_q, c.tq_q, SM) + differ("host tq_p", o.tq_p, c.tq_p, SM) + differ("host tq_link", o.tq_link, c.tq_link, SM) +
             differ("host tq_via", o.tq_via, c.tq_via, SM) + differ("host tq_metric", o.tq_metric, c.tq_metric, SM) + differ("host tq_count", o.tq_count, c.tq_count, S) +
             differ("host tn_kind", o.tn_kind, c.tn_kind, n) + differ("host tn_p", o.tn_p, c.tn_p, n) + differ("host tn_q", o.tn_q, c.tn_q, n) +
             differ("host tn_link", o.tn_link, c.tn_link, n) + differ("host tn_via", o.tn_via, c.tn_via, n) + differ("host tn_metric", o.tn_metric, c.tn_metric, n) +
             differ("host tn_set", o.tn_set, c.tn_set, n) + differ("host tn_coverage", o.tn_coverage, c.tn_coverage, HSPF_TN_COVERAGE_WORDS);
      compared += 3 * (size_t)c.n;
      bad += b;
    }
    printf("%zu cases, %zu destinations compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "tilfa_node_driver: %s\n", e.what());
    return 2;
  }
}
