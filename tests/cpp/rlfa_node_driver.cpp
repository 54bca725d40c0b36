// rlfa_node_driver.cpp — node-protecting remote LFA through the compiled layers, against expected values the Python model wrote.
//   rlfa_node_driver --engine hip <case files...>                the RAII layer (hspf::Engine: lfa_device, rlfa_device with space_flags,
//                                                                rlfa_node_select_device, a run of the listed nodes, rlfa_node_device,
//                                                                on DeviceBuffers) AND the host interface
//                                                                (hspf::host::HipEngine::rlfa_node on a DeviceRun and an RlfaOut),
//                                                                every array compared
//   rlfa_node_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                                the host interface's default on an engine without the call:
//                                                                RlfaNodeOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_rlfa_node.py writes them from tests/_rlfa_node_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | W M nq_node[SM] nq_via[SM] nq_metric[SM] nq_count[S] | Y y_roots[Y] |
//   nd_kind[n] nd_node[n] nd_via[n] nd_metric[n] nd_set[n] nd_coverage[5]                                  (S = 64 W, M = max_pq)
// Built by tests/test_cpp_rlfa_node.py.  TEST INFRASTRUCTURE.
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
  std::vector<uint32_t> nq_node, nq_via, nq_metric, nq_count, y_roots, nd_node, nd_via, nd_metric, nd_set, nd_coverage;
  std::vector<uint8_t> vflags, cflags, nd_kind;
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
  take(in, c.nq_node, SM); take(in, c.nq_via, SM); take(in, c.nq_metric, SM); take(in, c.nq_count, S);
  in >> c.Y;
  take(in, c.y_roots, c.Y);
  take(in, c.nd_kind, c.n); take(in, c.nd_node, c.n); take(in, c.nd_via, c.n); take(in, c.nd_metric, c.n); take(in, c.nd_set, c.n);
  take(in, c.nd_coverage, HSPF_NP_COVERAGE_WORDS);
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
        const hspf::host::RlfaNodeOut o = static_cast<hspf::host::Engine &>(eng).rlfa_node(*g, *run, {hp}, c.run_flags, 0, nullptr, hspf::host::RlfaOut{}, c.M);
        if (!o.supported && o.nq_node.empty() && o.nq_count.empty() && o.y_roots.empty() && o.nd_kind.empty() && o.nd_coverage.empty()) ++unsupported;
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
        hspf::DeviceBuffer qn(ctx, SM * 4), qv(ctx, SM * 4), qm(ctx, SM * 4), qc(ctx, S * 4);
        const hspf_rlfa_node_sel sel{qn.as<uint32_t>(), qv.as<uint32_t>(), qm.as<uint32_t>(), qc.as<uint32_t>()};
        eng.rlfa_node_select_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, 0, sf.as<uint8_t>(), c.M, sel);
        const std::vector<uint32_t> nodes = qn.to_host<uint32_t>(SM);
        std::vector<uint32_t> y;
        for (uint32_t v : nodes) if (v != HSPF_NO_ROOT) y.push_back(v);
        std::sort(y.begin(), y.end());
        y.erase(std::unique(y.begin(), y.end()), y.end());
        if (y.empty()) y.push_back(HSPF_NO_ROOT);
        hspf::DeviceBuffer ydist(ctx, y.size() * n * 4);
        run_rows(ctx, g.raw(), y, c.run_flags, hspf_result{ydist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr});
        hspf::DeviceBuffer dk(ctx, n), dn(ctx, n * 4), dv(ctx, n * 4), dm(ctx, n * 4), ds(ctx, n * 4), dc(ctx, HSPF_NP_COVERAGE_WORDS * 4);
        eng.rlfa_node_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, ydist.as<uint32_t>(), y, sel, c.M, fl.as<uint8_t>(),
                             hspf_rlfa_node_out{dk.as<uint8_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(), dm.as<uint32_t>(), ds.as<uint32_t>(), dc.as<uint32_t>()});
        if (y != c.y_roots) { printf("  %s: the union of the lists differs\n", f); ++b; }
        b += differ("nq_node", nodes, c.nq_node, SM) + differ("nq_via", qv.to_host<uint32_t>(SM), c.nq_via, SM) + differ("nq_metric", qm.to_host<uint32_t>(SM), c.nq_metric, SM);
        b += differ("nq_count", qc.to_host<uint32_t>(S), c.nq_count, S) + differ("nd_kind", dk.to_host<uint8_t>(n), c.nd_kind, n) + differ("nd_node", dn.to_host<uint32_t>(n), c.nd_node, n);
        b += differ("nd_via", dv.to_host<uint32_t>(n), c.nd_via, n) + differ("nd_metric", dm.to_host<uint32_t>(n), c.nd_metric, n) + differ("nd_set", ds.to_host<uint32_t>(n), c.nd_set, n);
        b += differ("nd_coverage", dc.to_host<uint32_t>(HSPF_NP_COVERAGE_WORDS), c.nd_coverage, HSPF_NP_COVERAGE_WORDS);
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
      const hspf::host::RlfaNodeOut o = heng.rlfa_node(*hg, *run, {hp}, c.run_flags, 0, &lo, ro, c.M);
      if (!o.supported || o.slot_stride != S || o.n_vertices != c.n || o.max_pq != c.M || o.y_roots != c.y_roots) { printf("  %s: host interface: unsupported, or shape or y_roots differ\n", f); ++b; }
      else
        b += differ("host nq_node", o.nq_node, c.nq_node, SM) + differ("host nq_via", o.nq_via, c.nq_via, SM) + differ("host nq_metric", o.nq_metric, c.nq_metric, SM) +
             differ("host nq_count", o.nq_count, c.nq_count, S) + differ("host nd_kind", o.nd_kind, c.nd_kind, n) + differ("host nd_node", o.nd_node, c.nd_node, n) +
             differ("host nd_via", o.nd_via, c.nd_via, n) + differ("host nd_metric", o.nd_metric, c.nd_metric, n) + differ("host nd_set", o.nd_set, c.nd_set, n) +
             differ("host nd_coverage", o.nd_coverage, c.nd_coverage, HSPF_NP_COVERAGE_WORDS);
      compared += 2 * (size_t)c.n;
      bad += b;
    }
    printf("%zu cases, %zu destinations compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "rlfa_node_driver: %s\n", e.what());
    return 2;
  }
}
