// lfa_driver.cpp — loop-free alternates through the compiled layers, against expected values the numpy model wrote.
//   lfa_driver --engine hip <case files...>                      the RAII layer (hspf::Engine::lfa: candidates, one run with the
//                                                                tables left in HBM, hspf_lfa_device) AND the host interface
//                                                                (hspf::host::HipEngine::lfa on a DeviceRun), every array compared
//   lfa_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                                the host interface's default on an engine without the call:
//                                                                LfaOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_lfa.py writes them from tests/_lfa_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | W alt_slot[n] alt_metric[n] alt_flags[n] cand_mask[n*W] node_mask[n*W] coverage[5]
// Built by tests/test_cpp_lfa.py.  TEST INFRASTRUCTURE.
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
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row, alt_slot, alt_metric, coverage;
  std::vector<uint8_t> vflags, cflags, alt_flags;
  std::vector<uint64_t> cand_mask, node_mask;
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
  take(in, c.alt_slot, c.n); take(in, c.alt_metric, c.n); take(in, c.alt_flags, c.n);
  take(in, c.cand_mask, (size_t)c.n * c.W); take(in, c.node_mask, (size_t)c.n * c.W); take(in, c.coverage, HSPF_LFA_COVERAGE_WORDS);
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
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        const hspf::host::LfaOut o = static_cast<hspf::host::Engine &>(eng).lfa(*run, {hp}, 0, true);
        if (!o.supported && o.alt_slot.empty() && o.alt_flags.empty() && o.coverage.empty() && o.cand_mask.empty()) ++unsupported;
        continue;
      }
      // the RAII layer
      hspf::Engine eng(0);
      hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::Lfa r = eng.lfa(g, c.row_ptr, c.col, c.metric, c.vflags, c.root, c.run_flags);
      size_t b = 0;
      if (r.candidates.nbr.size() != c.K || r.roots != c.roots || r.mask_words != c.W) { printf("  %s: K / roots / W differ\n", f); ++b; }
      else {
        b += differ("nbr", r.candidates.nbr, c.nbr, c.K) + differ("cost", r.candidates.cost, c.cost, c.K) +
             differ("root_link", r.candidates.root_link, c.root_link, c.K) + differ("cflags", r.candidates.cflags, c.cflags, c.K);
        b += differ("alt_slot", r.alt_slot, c.alt_slot, c.n) + differ("alt_metric", r.alt_metric, c.alt_metric, c.n) + differ("alt_flags", r.alt_flags, c.alt_flags, c.n);
        b += differ("cand_mask", r.cand_mask, c.cand_mask, (size_t)c.n * c.W) + differ("node_mask", r.node_mask, c.node_mask, (size_t)c.n * c.W);
        b += differ("coverage", r.coverage, c.coverage, HSPF_LFA_COVERAGE_WORDS);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      const hspf::host::LfaOut o = heng.lfa(*run, {hp}, 0, true);
      if (!o.supported || o.mask_words != c.W || o.n_vertices != c.n) { printf("  %s: host interface: unsupported or shape differs\n", f); ++b; }
      else
        b += differ("host alt_slot", o.alt_slot, c.alt_slot, c.n) + differ("host alt_metric", o.alt_metric, c.alt_metric, c.n) +
             differ("host alt_flags", o.alt_flags, c.alt_flags, c.n) + differ("host cand_mask", o.cand_mask, c.cand_mask, (size_t)c.n * c.W) +
             differ("host node_mask", o.node_mask, c.node_mask, (size_t)c.n * c.W) + differ("host coverage", o.coverage, c.coverage, HSPF_LFA_COVERAGE_WORDS);
      compared += 2 * (size_t)c.n;
      bad += b;
    }
    printf("%zu cases, %zu destinations compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "lfa_driver: %s\n", e.what());
    return 2;
  }
}
