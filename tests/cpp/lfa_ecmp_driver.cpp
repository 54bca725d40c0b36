// lfa_ecmp_driver.cpp — per-primary alternates of ECMP destinations through the compiled layers, against expected values the Python
// model wrote.
//   lfa_ecmp_driver --engine hip <case files...>     the RAII layer (hspf::Engine::lfa_ecmp: candidates, run, both sizing calls) AND
//                                                    the host interface (hspf::host::HipEngine::run_device -> lfa_ecmp), every array
//   lfa_ecmp_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                    the host interface's default on an engine without the call:
//                                                    LfaEcmpOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_lfa_ecmp.py writes them from tests/_lfa_ecmp_model.py):
//   n e max_path root run_flags lfa_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | T ea_ptr[n+1] ea_primary[T] ea_slot[T] ea_metric[T] ea_flags[T] ea_coverage[7]
// Built by build() and by tests/test_cpp_lfa_ecmp.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, lfa_flags = 0, K = 0, R = 0, T = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row;
  std::vector<uint32_t> ea_ptr, ea_primary, ea_slot, ea_metric, ea_coverage;
  std::vector<uint8_t> vflags, cflags, ea_flags;
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
  in >> c.n >> c.e >> c.maxp >> c.root >> c.run_flags >> c.lfa_flags;
  take(in, c.row_ptr, (size_t)c.n + 1); take(in, c.col, c.e); take(in, c.metric, c.e); take(in, c.vflags, c.n);
  in >> c.K;
  take(in, c.nbr, c.K); take(in, c.cost, c.K); take(in, c.root_link, c.K); take(in, c.cflags, c.K);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.nbr_row, c.K);
  in >> c.T;
  take(in, c.ea_ptr, (size_t)c.n + 1); take(in, c.ea_primary, c.T); take(in, c.ea_slot, c.T); take(in, c.ea_metric, c.T); take(in, c.ea_flags, c.T);
  take(in, c.ea_coverage, HSPF_LFA_ECMP_COVERAGE_WORDS);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

size_t n_compared = 0;      // entries differ() has looked at

template <typename A, typename B>
size_t differ(const char *what, const A &got, const B &want, size_t count) {
  n_compared += count;
  if (got.size() != count) { printf("  %s: %zu entries, want %zu\n", what, (size_t)got.size(), count); return 1; }
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
    size_t cases = 0, bad = 0, unsupported = 0;
    for (const char *f : files) {
      const Case c = load(f);
      ++cases;
      const size_t T = c.T, CW = HSPF_LFA_ECMP_COVERAGE_WORDS;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        const hspf::host::LfaEcmpOut o = static_cast<hspf::host::Engine &>(eng).lfa_ecmp(*run, {hp}, c.lfa_flags);
        if (!o.supported && o.ea_ptr.empty() && o.ea_primary.empty() && o.ea_coverage.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      {
        // the RAII layer: candidates from the CSR, the run, the two calls
        hspf::Engine eng(0);
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        const hspf::LfaEcmp r = eng.lfa_ecmp(g, c.row_ptr, c.col, c.metric, c.vflags, c.root, c.run_flags, c.lfa_flags);
        b += differ("candidates.nbr", r.candidates.nbr, c.nbr, c.K) + differ("roots", r.roots, c.roots, c.R);
        b += differ("ea_ptr", r.ea_ptr, c.ea_ptr, (size_t)c.n + 1) + differ("ea_primary", r.ea_primary, c.ea_primary, T);
        b += differ("ea_slot", r.ea_slot, c.ea_slot, T) + differ("ea_metric", r.ea_metric, c.ea_metric, T) + differ("ea_flags", r.ea_flags, c.ea_flags, T);
        b += differ("ea_coverage", std::vector<uint32_t>(r.ea_coverage, r.ea_coverage + CW), c.ea_coverage, CW);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      const hspf::host::LfaEcmpOut o = heng.lfa_ecmp(*run, {hp}, c.lfa_flags);
      if (!o.supported || o.n_protected != 1 || o.n_vertices != c.n) { printf("  %s: host interface: unsupported, or shape differs\n", f); ++b; }
      else {
        b += differ("host ea_ptr", o.ea_ptr, c.ea_ptr, (size_t)c.n + 1) + differ("host ea_primary", o.ea_primary, c.ea_primary, T);
        b += differ("host ea_slot", o.ea_slot, c.ea_slot, T) + differ("host ea_metric", o.ea_metric, c.ea_metric, T);
        b += differ("host ea_flags", o.ea_flags, c.ea_flags, T) + differ("host ea_coverage", o.ea_coverage, c.ea_coverage, CW);
      }
      bad += b;
    }
    printf("%zu cases, %zu entries compared, %zu differ, %zu answered not supported\n", cases, n_compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "lfa_ecmp_driver: %s\n", e.what());
    return 2;
  }
}
