// backup_ecmp_driver.cpp — per-primary backups of ECMP prefixes through the compiled layers, against expected values the Python model
// wrote.
//   backup_ecmp_driver --engine hip <case files...>     the RAII layer (hspf::Engine::backup_routes(..., ecmp = true): the whole chain with
//                                                       the repairs, both calls) AND the host interface (hspf::host::HipEngine::run_device
//                                                       -> routes_device -> backup_routes_ecmp without repairs), every array
//   backup_ecmp_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                       the host interface's default on an engine without the call:
//                                                       BackupEcmpOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_backup_ecmp.py writes them from tests/_backup_ecmp_model.py):
//   n e max_path root run_flags lfa_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | NP NE table_flags pfx_ptr[NP+1] pfx_vertex[NE] pfx_metric[NE] | two expected blocks, with and without
//   the repairs, each  T eb_ptr[NP+1] eb_primary[T] eb_kind[T] eb_slot[T] eb_metric[T] eb_flags[T] eb_coverage[8]
// Built by build() and by tests/test_cpp_backup_ecmp.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Want {
  uint32_t T = 0;
  std::vector<uint32_t> eb_ptr, eb_primary, eb_slot, eb_metric, eb_coverage;
  std::vector<uint8_t> eb_kind, eb_flags;
};

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, lfa_flags = 0, K = 0, R = 0, NP = 0, NE = 0, tflags = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row, pfx_ptr, pfx_vertex, pfx_metric;
  std::vector<uint8_t> vflags, cflags;
  Want with, without;
};

template <typename T>
void take(std::istream &in, std::vector<T> &v, size_t count) {
  v.resize(count);
  for (size_t i = 0; i < count; ++i) { uint64_t x; in >> x; v[i] = (T)x; }
}

void take_want(std::istream &in, Want &w, uint32_t np) {
  in >> w.T;
  take(in, w.eb_ptr, (size_t)np + 1); take(in, w.eb_primary, w.T); take(in, w.eb_kind, w.T); take(in, w.eb_slot, w.T); take(in, w.eb_metric, w.T);
  take(in, w.eb_flags, w.T); take(in, w.eb_coverage, HSPF_BK_ECMP_COVERAGE_WORDS);
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
  in >> c.NP >> c.NE >> c.tflags;
  take(in, c.pfx_ptr, (size_t)c.NP + 1); take(in, c.pfx_vertex, c.NE); take(in, c.pfx_metric, c.NE);
  take_want(in, c.with, c.NP); take_want(in, c.without, c.NP);
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
      const size_t CW = HSPF_BK_ECMP_COVERAGE_WORDS, NP1 = (size_t)c.NP + 1;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        auto routes = eng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
        const hspf::host::BackupEcmpOut o = static_cast<hspf::host::Engine &>(eng).backup_routes_ecmp(*run, *routes, c.pfx_ptr, c.pfx_vertex, c.pfx_metric,
                                                                                                      c.tflags, {hp}, c.lfa_flags, nullptr);
        if (!o.supported && o.eb_ptr.empty() && o.eb_primary.empty() && o.eb_coverage.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      {
        // the RAII layer: candidates from the CSR, the runs, the repairs, the routes, the plain backups, then the two calls
        hspf::Engine eng(0);
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        const hspf::BackupRoutes r = eng.backup_routes(g, c.row_ptr, c.col, c.metric, c.vflags, c.maxp, c.root, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags,
                                                       c.run_flags, c.lfa_flags, false, true, true);
        const Want &w = c.with;
        b += differ("eb_ptr", r.eb_ptr, w.eb_ptr, NP1) + differ("eb_primary", r.eb_primary, w.eb_primary, w.T) + differ("eb_kind", r.eb_kind, w.eb_kind, w.T);
        b += differ("eb_slot", r.eb_slot, w.eb_slot, w.T) + differ("eb_metric", r.eb_metric, w.eb_metric, w.T) + differ("eb_flags", r.eb_flags, w.eb_flags, w.T);
        b += differ("eb_coverage", std::vector<uint32_t>(r.eb_coverage, r.eb_coverage + CW), w.eb_coverage, CW);
        size_t n_ecmp = 0;                                              // the stream speaks about exactly the HSPF_BK_ECMP prefixes
        for (uint8_t k : r.bk_kind) n_ecmp += k == HSPF_BK_ECMP;
        if (n_ecmp != w.eb_coverage[0]) { printf("  %s: %zu HSPF_BK_ECMP prefixes, %u in eb_coverage\n", f, n_ecmp, w.eb_coverage[0]); ++b; }
      }
      // the host interface on the product engine, without repairs
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      auto routes = heng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
      const hspf::host::BackupEcmpOut o = heng.backup_routes_ecmp(*run, *routes, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags, {hp}, c.lfa_flags, nullptr);
      const Want &w = c.without;
      if (!o.supported || o.n_protected != 1 || o.n_prefixes != c.NP) { printf("  %s: host interface: unsupported, or shape differs\n", f); ++b; }
      else {
        b += differ("host eb_ptr", o.eb_ptr, w.eb_ptr, NP1) + differ("host eb_primary", o.eb_primary, w.eb_primary, w.T) + differ("host eb_kind", o.eb_kind, w.eb_kind, w.T);
        b += differ("host eb_slot", o.eb_slot, w.eb_slot, w.T) + differ("host eb_metric", o.eb_metric, w.eb_metric, w.T);
        b += differ("host eb_flags", o.eb_flags, w.eb_flags, w.T) + differ("host eb_coverage", o.eb_coverage, w.eb_coverage, CW);
      }
      bad += b;
    }
    printf("%zu cases, %zu entries compared, %zu differ, %zu answered not supported\n", cases, n_compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "backup_ecmp_driver: %s\n", e.what());
    return 2;
  }
}
