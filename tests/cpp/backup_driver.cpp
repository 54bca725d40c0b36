// backup_driver.cpp — per-prefix backup routes through the compiled layers, against expected values the Python model wrote.
//   backup_driver --engine hip <case files...>                   the RAII layer (hspf::Engine::backup_routes: the chain of tilfa(),
//                                                                hspf_routes_device and hspf_routes_backup_device with everything
//                                                                kept in HBM); every output array is printed and compared
//   backup_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                                the host interface's default on an engine without the call:
//                                                                BackupOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_backup.py writes them from tests/_backup_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] | R roots[R] | W remote |
//   P E table_flags pfx_ptr[P+1] pfx_vertex[E] pfx_metric[E] | best_metric[P] best_entry[P] nexthop_mask[P W] bk_kind[P] bk_primary[P]
//   bk_slot[P] bk_metric[P] bk_flags[P] bk_cand_mask[P W] bk_node_mask[P W] bk_coverage[7]
// Built by holo_amd/build.py (build_driver).  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, K = 0, R = 0, W = 0, remote = 0, P = 0, E = 0, tflags = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, roots, pfx_ptr, pfx_vertex, pfx_metric;
  std::vector<uint32_t> best_metric, best_entry, bk_primary, bk_slot, bk_metric, bk_coverage;
  std::vector<uint64_t> nexthop_mask, bk_cand_mask, bk_node_mask;
  std::vector<uint8_t> vflags, bk_kind, bk_flags;
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
  take(in, c.nbr, c.K);
  in >> c.R;
  take(in, c.roots, c.R);
  in >> c.W >> c.remote >> c.P >> c.E >> c.tflags;
  take(in, c.pfx_ptr, (size_t)c.P + 1); take(in, c.pfx_vertex, c.E); take(in, c.pfx_metric, c.E);
  const size_t pw = (size_t)c.P * c.W;
  take(in, c.best_metric, c.P); take(in, c.best_entry, c.P); take(in, c.nexthop_mask, pw);
  take(in, c.bk_kind, c.P); take(in, c.bk_primary, c.P); take(in, c.bk_slot, c.P); take(in, c.bk_metric, c.P); take(in, c.bk_flags, c.P);
  take(in, c.bk_cand_mask, pw); take(in, c.bk_node_mask, pw); take(in, c.bk_coverage, HSPF_BK_COVERAGE_WORDS);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

template <typename A, typename B>
size_t differ(const char *what, const A &got, const B &want, size_t count) {
  size_t bad = 0;
  printf("  %s:", what);
  for (size_t i = 0; i < count; ++i) {
    printf(" %llu", (unsigned long long)got[i]);
    if ((uint64_t)got[i] != (uint64_t)want[i]) {
      if (!bad) printf(" <- [%zu] want %llu", i, (unsigned long long)want[i]);
      ++bad;
    }
  }
  printf("\n");
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
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        auto routes = eng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
        hspf::host::LfaProtect hp;
        hp.root_vertex = c.root;
        const hspf::host::BackupOut o = static_cast<hspf::host::Engine &>(eng).backup_routes(*run, *routes, {hp}, 0, nullptr);
        if (!o.supported && o.bk_kind.empty() && o.bk_primary.empty() && o.bk_slot.empty() && o.bk_metric.empty() && o.bk_coverage.empty()) ++unsupported;
        continue;
      }
      hspf::Engine eng(0);
      hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::BackupRoutes r = eng.backup_routes(g, c.row_ptr, c.col, c.metric, c.vflags, c.maxp, c.root, c.pfx_ptr, c.pfx_vertex, c.pfx_metric,
                                                     c.tflags, c.run_flags, 0, false, c.remote != 0);
      const hspf::Lfa &l = r.tilfa.rlfa.lfa;
      size_t b = 0;
      printf("%s\n", f);
      if (l.candidates.nbr != c.nbr || l.roots != c.roots || l.mask_words != c.W || r.n_prefixes != c.P) { printf("  K / roots / W / P differ\n"); ++b; }
      else {
        const size_t pw = (size_t)c.P * c.W;
        b += differ("best_metric", r.best_metric, c.best_metric, c.P) + differ("best_entry", r.best_entry, c.best_entry, c.P);
        b += differ("nexthop_mask", r.nexthop_mask, c.nexthop_mask, pw) + differ("bk_kind", r.bk_kind, c.bk_kind, c.P);
        b += differ("bk_primary", r.bk_primary, c.bk_primary, c.P) + differ("bk_slot", r.bk_slot, c.bk_slot, c.P);
        b += differ("bk_metric", r.bk_metric, c.bk_metric, c.P) + differ("bk_flags", r.bk_flags, c.bk_flags, c.P);
        b += differ("bk_cand_mask", r.bk_cand_mask, c.bk_cand_mask, pw) + differ("bk_node_mask", r.bk_node_mask, c.bk_node_mask, pw);
        b += differ("bk_coverage", r.bk_coverage, c.bk_coverage, HSPF_BK_COVERAGE_WORDS);
      }
      compared += c.P;
      bad += b;
    }
    printf("%zu cases, %zu prefixes compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "backup_driver: %s\n", e.what());
    return 2;
  }
}
