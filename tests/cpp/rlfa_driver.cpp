// rlfa_driver.cpp — remote loop-free alternates through the compiled layers, against expected values the numpy model wrote.
//   rlfa_driver --engine hip <case files...>                     the RAII layer (hspf::Engine::rlfa: candidates, the forward and the
//                                                                transposed run with the tables left in HBM, hspf_lfa_device,
//                                                                hspf_rlfa_device) AND the host interface
//                                                                (hspf::host::HipEngine::rlfa on two DeviceRuns), every array compared
//   rlfa_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                                the host interface's default on an engine without the call:
//                                                                RlfaOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_rlfa.py writes them from tests/_rlfa_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | W pq_node[S] pq_via[S] pq_metric[S] pq_counts[4S] space_flags[S*n] space_via[S*n] rl_node[n] rl_via[n]
//   rl_coverage[4]                                                                                              (S = 64 W)
// Built by tests/test_cpp_rlfa.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, K = 0, R = 0, W = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row;
  std::vector<uint32_t> pq_node, pq_via, pq_metric, pq_counts, space_via, rl_node, rl_via, rl_coverage;
  std::vector<uint8_t> vflags, cflags, space_flags;
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
  in >> c.W;
  const size_t S = 64u * (size_t)c.W;
  take(in, c.pq_node, S); take(in, c.pq_via, S); take(in, c.pq_metric, S); take(in, c.pq_counts, S * HSPF_RLFA_COUNT_WORDS);
  take(in, c.space_flags, S * c.n); take(in, c.space_via, S * c.n); take(in, c.rl_node, c.n); take(in, c.rl_via, c.n);
  take(in, c.rl_coverage, HSPF_RLFA_COVERAGE_WORDS);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

template <typename A, typename B>
size_t differ(const char *what, const A &got, const B &want, size_t count) {
  size_t bad = 0;
  for (size_t i = 0; i < count; ++i)
    if ((uint64_t)got[i] != (uint64_t)want[i]) {
      if (!bad) printf("  %s[%zu]: got %llu, want %llu\n", what, i, (unsigned long long)got[i], (unsigned long long)want[i]);
      ++bad;
    }
  return bad;
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
      const size_t S = 64u * (size_t)c.W;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        const hspf::host::RlfaOut o = static_cast<hspf::host::Engine &>(eng).rlfa(*g, *run, *run, {hp}, 0, nullptr, true);
        if (!o.supported && o.pq_node.empty() && o.pq_counts.empty() && o.rl_node.empty() && o.rl_coverage.empty() && o.space_flags.empty()) ++unsupported;
        continue;
      }
      // the RAII layer
      hspf::Engine eng(0);
      hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::Rlfa r = eng.rlfa(g, c.row_ptr, c.col, c.metric, c.vflags, c.maxp, c.root, c.run_flags, 0, false, true);
      size_t b = 0;
      if (r.lfa.candidates.nbr.size() != c.K || r.lfa.roots != c.roots || r.lfa.mask_words != c.W || r.slot_stride != S) { printf("  %s: K / roots / W differ\n", f); ++b; }
      else {
        b += differ("pq_node", r.pq_node, c.pq_node, S) + differ("pq_via", r.pq_via, c.pq_via, S) + differ("pq_metric", r.pq_metric, c.pq_metric, S);
        b += differ("pq_counts", r.pq_counts, c.pq_counts, S * HSPF_RLFA_COUNT_WORDS);
        b += differ("space_flags", r.space_flags, c.space_flags, S * c.n) + differ("space_via", r.space_via, c.space_via, S * c.n);
        b += differ("rl_node", r.rl_node, c.rl_node, c.n) + differ("rl_via", r.rl_via, c.rl_via, c.n);
        b += differ("rl_coverage", r.rl_coverage, c.rl_coverage, HSPF_RLFA_COVERAGE_WORDS);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::Engine::Transposed t = hspf::Engine::csr_transpose(c.row_ptr, c.col, c.metric, c.vflags);
      auto hgt = heng.upload(t.row_ptr, t.col, t.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      auto rrun = heng.run_device(*hgt, c.roots, c.run_flags);
      const hspf::host::LfaOut lo = heng.lfa(*run, {hp}, 0, false);
      const hspf::host::RlfaOut o = heng.rlfa(*hg, *run, *rrun, {hp}, 0, &lo, true);
      if (!o.supported || o.slot_stride != S || o.n_vertices != c.n) { printf("  %s: host interface: unsupported or shape differs\n", f); ++b; }
      else
        b += differ("host pq_node", o.pq_node, c.pq_node, S) + differ("host pq_via", o.pq_via, c.pq_via, S) + differ("host pq_metric", o.pq_metric, c.pq_metric, S) +
             differ("host pq_counts", o.pq_counts, c.pq_counts, S * HSPF_RLFA_COUNT_WORDS) + differ("host space_flags", o.space_flags, c.space_flags, S * c.n) +
             differ("host space_via", o.space_via, c.space_via, S * c.n) + differ("host rl_node", o.rl_node, c.rl_node, c.n) +
             differ("host rl_via", o.rl_via, c.rl_via, c.n) + differ("host rl_coverage", o.rl_coverage, c.rl_coverage, HSPF_RLFA_COVERAGE_WORDS);
      compared += 2 * (size_t)c.n;
      bad += b;
    }
    printf("%zu cases, %zu destinations compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "rlfa_driver: %s\n", e.what());
    return 2;
  }
}
