// tilfa_driver.cpp — two-segment repair paths through the compiled layers, against expected values the Python model wrote.
//   tilfa_driver --engine hip <case files...>                    the RAII layer (hspf::Engine::tilfa: rlfa() with the space tables kept
//                                                                in HBM, then hspf_tilfa_device) AND the host interface
//                                                                (hspf::host::HipEngine::tilfa on two DeviceRuns and an RlfaOut), every
//                                                                array compared
//   tilfa_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                                the host interface's default on an engine without the call:
//                                                                TilfaOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_tilfa.py writes them from tests/_tilfa_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   R roots[R] nbr_row[K] | W ti_kind[S] ti_p[S] ti_q[S] ti_via[S] ti_link[S] ti_metric[S] ti_counts[2S] td_kind[n] td_coverage[5]
//                                                                                                               (S = 64 W)
// Built by tests/test_cpp_tilfa.py.  TEST INFRASTRUCTURE.
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
  std::vector<uint32_t> ti_p, ti_q, ti_via, ti_link, ti_metric, ti_counts, td_coverage;
  std::vector<uint8_t> vflags, cflags, ti_kind, td_kind;
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
  take(in, c.ti_kind, S); take(in, c.ti_p, S); take(in, c.ti_q, S); take(in, c.ti_via, S); take(in, c.ti_link, S); take(in, c.ti_metric, S);
  take(in, c.ti_counts, S * HSPF_TILFA_COUNT_WORDS); take(in, c.td_kind, c.n); take(in, c.td_coverage, HSPF_TILFA_COVERAGE_WORDS);
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
        const hspf::host::TilfaOut o = static_cast<hspf::host::Engine &>(eng).tilfa(*g, *run, *run, {hp}, 0, nullptr, hspf::host::RlfaOut{});
        if (!o.supported && o.ti_kind.empty() && o.ti_p.empty() && o.ti_counts.empty() && o.td_kind.empty() && o.td_coverage.empty()) ++unsupported;
        continue;
      }
      // the RAII layer
      hspf::Engine eng(0);
      hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::Tilfa r = eng.tilfa(g, c.row_ptr, c.col, c.metric, c.vflags, c.maxp, c.root, c.run_flags, 0, false);
      size_t b = 0;
      if (r.rlfa.lfa.candidates.nbr.size() != c.K || r.rlfa.lfa.roots != c.roots || r.rlfa.lfa.mask_words != c.W || r.rlfa.slot_stride != S) { printf("  %s: K / roots / W differ\n", f); ++b; }
      else {
        b += differ("ti_kind", r.ti_kind, c.ti_kind, S) + differ("ti_p", r.ti_p, c.ti_p, S) + differ("ti_q", r.ti_q, c.ti_q, S) + differ("ti_via", r.ti_via, c.ti_via, S);
        b += differ("ti_link", r.ti_link, c.ti_link, S) + differ("ti_metric", r.ti_metric, c.ti_metric, S);
        b += differ("ti_counts", r.ti_counts, c.ti_counts, S * HSPF_TILFA_COUNT_WORDS) + differ("td_kind", r.td_kind, c.td_kind, c.n);
        b += differ("td_coverage", r.td_coverage, c.td_coverage, HSPF_TILFA_COVERAGE_WORDS);
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
      const hspf::host::TilfaOut o = heng.tilfa(*hg, *run, *rrun, {hp}, 0, &lo, ro);
      if (!o.supported || o.slot_stride != S || o.n_vertices != c.n) { printf("  %s: host interface: unsupported or shape differs\n", f); ++b; }
      else
        b += differ("host ti_kind", o.ti_kind, c.ti_kind, S) + differ("host ti_p", o.ti_p, c.ti_p, S) + differ("host ti_q", o.ti_q, c.ti_q, S) +
             differ("host ti_via", o.ti_via, c.ti_via, S) + differ("host ti_link", o.ti_link, c.ti_link, S) + differ("host ti_metric", o.ti_metric, c.ti_metric, S) +
             differ("host ti_counts", o.ti_counts, c.ti_counts, S * HSPF_TILFA_COUNT_WORDS) + differ("host td_kind", o.td_kind, c.td_kind, c.n) +
             differ("host td_coverage", o.td_coverage, c.td_coverage, HSPF_TILFA_COVERAGE_WORDS);
      compared += 2 * (size_t)c.n;
      bad += b;
    }
    printf("%zu cases, %zu destinations compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "tilfa_driver: %s\n", e.what());
    return 2;
  }
}
