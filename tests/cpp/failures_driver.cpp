// failures_driver.cpp — failure-scenario SPF rows through the compiled layers, against expected rows the CPU oracle wrote.
//   failures_driver --engine hip <case files...>      the RAII layer (hspf::Engine::run_failures AND run_failures_device with the
//                                                     tables left in HBM) and the host interface (hspf::host::HipEngine::run_failures)
//   failures_driver --engine host <case files...>     the host twin, hspf::host::run_failures_sequential, on the case's CSR (no GPU)
//   failures_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                     the oracle engine standing in for the GPU engine: run_failures() answered by
//                                                     plain runs on the CSR with the failed links retargeted to an extra vertex
// A case file is a list of decimal numbers (tests/_failure_cases.py writes them):
//   n e max_path run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | R roots[R] kind[R] arg[R] | W dist[R*n] hops[R*n] flags[R*n] mask[R*n*W]
// Distances, hop counts, HSPF_RF_IN_SPT and every mask word are compared.  Built by build().  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, run_flags = 0, R = 0, W = 0;
  std::vector<uint32_t> row_ptr, col, metric, roots, kind, arg, dist;
  std::vector<uint8_t> vflags;
  std::vector<uint16_t> hops, flags;
  std::vector<uint64_t> mask;
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
  in >> c.n >> c.e >> c.maxp >> c.run_flags;
  take(in, c.row_ptr, (size_t)c.n + 1); take(in, c.col, c.e); take(in, c.metric, c.e); take(in, c.vflags, c.n);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.kind, c.R); take(in, c.arg, c.R);
  in >> c.W;
  const size_t rn = (size_t)c.R * c.n;
  take(in, c.dist, rn); take(in, c.hops, rn); take(in, c.flags, rn); take(in, c.mask, rn * c.W);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

size_t compare(const char *who, const char *file, const Case &c, const hspf::host::Tables &t) {
  if (t.n_roots != c.R || t.n_vertices != c.n || t.mask_words != c.W) { printf("  %s %s: shape differs (W %u, want %u)\n", who, file, t.mask_words, c.W); return 1; }
  size_t bad = 0;
  for (size_t i = 0; i < (size_t)c.R * c.n; ++i) {
    bool ok = t.dist[i] == c.dist[i] && t.hops[i] == c.hops[i] && (t.flags[i] & HSPF_RF_IN_SPT) == (c.flags[i] & HSPF_RF_IN_SPT);
    for (uint32_t w = 0; w < c.W; ++w) ok = ok && t.mask[i * c.W + w] == c.mask[i * c.W + w];
    if (!ok) {
      if (!bad) printf("  %s %s: row %zu vertex %zu: dist %u (want %u) hops %u (want %u) flags %u (want %u) mask[0] %llx (want %llx)\n", who, file, i / c.n, i % c.n,
                       t.dist[i], c.dist[i], t.hops[i], c.hops[i], t.flags[i], c.flags[i], (unsigned long long)t.mask[i * c.W], (unsigned long long)c.mask[i * c.W]);
      ++bad;
    }
  }
  return bad;
}

hspf::host::Tables as_host(const hspf::Tables &r) {
  hspf::host::Tables t;
  t.n_roots = r.n_roots; t.n_vertices = r.n_vertices; t.mask_words = r.mask_words;
  t.dist = r.dist; t.hops = r.hops; t.flags = r.flags; t.mask = r.mask;
  return t;
}

// The oracle engine with run_failures(): every row is a plain run on the graph with one extra vertex n (an empty row) that the failed
// link, or every link of the excluded vertex's row, is retargeted to — such links fail the two-way check and no position moves.
class FailOracleEngine : public OracleEngine {
 public:
  using OracleEngine::OracleEngine;
  Tables run_failures(Graph &gr, const std::vector<uint32_t> &roots, const std::vector<Failure> &failures, uint32_t run_flags) override {
    auto &g = static_cast<OracleGraph &>(gr);
    const uint32_t n = (uint32_t)g.vflags.size();
    Tables t;
    t.n_roots = (uint32_t)roots.size(); t.n_vertices = n;
    for (uint32_t root : roots)
      if (root != HSPF_NO_ROOT) t.mask_words = std::max(t.mask_words, (slot_table(gr, root).total + 63u) / 64u);
    const size_t W = t.mask_words;
    t.dist.assign((size_t)t.n_roots * n, HSPF_DIST_INF); t.hops.assign((size_t)t.n_roots * n, 0); t.flags.assign((size_t)t.n_roots * n, 0);
    t.mask.assign((size_t)t.n_roots * n * W, 0);
    for (uint32_t r = 0; r < t.n_roots; ++r) {
      if (roots[r] == HSPF_NO_ROOT) continue;
      OracleGraph h;
      h.row_ptr = g.row_ptr; h.row_ptr.push_back(g.row_ptr.back());
      h.col = g.col; h.metric = g.metric; h.vflags = g.vflags; h.vflags.push_back(0); h.max_path = g.max_path;
      if (failures[r].kind == HSPF_FAIL_ROOT_LINK) h.col[g.row_ptr[roots[r]] + failures[r].arg] = n;
      if (failures[r].kind == HSPF_FAIL_VERTEX)
        for (uint32_t k = g.row_ptr[failures[r].arg]; k < g.row_ptr[failures[r].arg + 1]; ++k) h.col[k] = n;
      const Tables one = run(h, {roots[r]}, run_flags);
      if (one.mask_words > W) throw std::runtime_error("run_failures: a retargeted graph needs more mask words");
      // A retargeted link into a network vertex of the root's slot table takes that vertex out of the table ON THE RETARGETED GRAPH and
      // moves the bases of the networks behind it; the call keeps the intact graph's numbering, so the bits are carried over slot by
      // slot: (table vertex, position) names a slot in both numberings (tests/_failure_cases.py does the same).
      const SlotTable st1 = slot_table(gr, roots[r]), st2 = slot_table(h, roots[r]);
      const bool moved = st1.vertex != st2.vertex || st1.base != st2.base;
      for (uint32_t v = 0; v < n; ++v) {
        const size_t o = (size_t)r * n + v;
        t.dist[o] = one.dist[v]; t.hops[o] = one.hops[v]; t.flags[o] = one.flags[v];
        const uint64_t *src = one.mask.data() + (size_t)v * one.mask_words;
        if (!moved) { for (uint32_t w = 0; w < one.mask_words; ++w) t.mask[o * W + w] = src[w]; continue; }
        for (size_t i2 = 0; i2 < st2.vertex.size(); ++i2) {
          const uint32_t p = st2.vertex[i2];
          const size_t i1 = std::find(st1.vertex.begin(), st1.vertex.end(), p) - st1.vertex.begin();
          if (i1 == st1.vertex.size()) throw std::runtime_error("run_failures: the retargeted graph's slot table is no subset of the intact one");
          for (uint32_t j = 0; j < g.row_ptr[p + 1] - g.row_ptr[p]; ++j) {
            const uint32_t s2 = st2.base[i2] + j, s1 = st1.base[i1] + j;
            if (src[s2 / 64] >> (s2 % 64) & 1) t.mask[o * W + s1 / 64] |= 1ull << (s1 % 64);
          }
        }
      }
    }
    return t;
  }
};

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
    size_t cases = 0, rows = 0, bad = 0;
    for (const char *f : files) {
      const Case c = load(f);
      ++cases;
      std::vector<hspf::host::Failure> hf(c.R);
      std::vector<hspf_failure> cf(c.R);
      for (uint32_t r = 0; r < c.R; ++r) { hf[r].kind = c.kind[r]; hf[r].arg = c.arg[r]; cf[r] = hspf_failure{c.kind[r], c.arg[r]}; }
      if (engine == "host") {
        bad += compare("host twin", f, c, hspf::host::run_failures_sequential(c.row_ptr, c.col, c.metric, c.vflags, c.maxp, c.roots, hf, c.run_flags));
        rows += c.R;
        continue;
      }
      if (engine == "oracle") {
        FailOracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        bad += compare("oracle engine", f, c, static_cast<hspf::host::Engine &>(eng).run_failures(*g, c.roots, hf, c.run_flags));
        rows += c.R;
        continue;
      }
      // the RAII layer: host tables, then the device form copied back
      hspf::Engine eng(0);
      hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      const hspf::Tables r = eng.run_failures(g, c.roots, cf, c.run_flags);
      bad += compare("RAII", f, c, as_host(r));
      {
        const size_t rn = (size_t)c.R * c.n;
        hspf::host::Tables d;
        d.n_roots = c.R; d.n_vertices = c.n; d.mask_words = r.mask_words;
        d.dist.resize(rn); d.hops.resize(rn); d.flags.resize(rn); d.mask.resize(rn * d.mask_words);
        void *dd = nullptr, *dh = nullptr, *df = nullptr, *dm = nullptr;
        if (hipMalloc(&dd, rn * 4) != hipSuccess || hipMalloc(&dh, rn * 2) != hipSuccess || hipMalloc(&df, rn * 2) != hipSuccess ||
            hipMalloc(&dm, rn * 8 * d.mask_words) != hipSuccess) throw std::runtime_error("hipMalloc");
        eng.run_failures_device(g, c.roots, cf, c.run_flags, hspf_result{(uint32_t *)dd, (uint16_t *)dh, (uint16_t *)df, (uint64_t *)dm, d.mask_words, nullptr});
        if (hipMemcpy(d.dist.data(), dd, rn * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(d.hops.data(), dh, rn * 2, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(d.flags.data(), df, rn * 2, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(d.mask.data(), dm, rn * 8 * d.mask_words, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy");
        (void)hipFree(dd); (void)hipFree(dh); (void)hipFree(df); (void)hipFree(dm);
        bad += compare("RAII device", f, c, d);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      bad += compare("host interface", f, c, heng.run_failures(*hg, c.roots, hf, c.run_flags));
      rows += 3 * (size_t)c.R;
    }
    printf("%zu cases, %zu rows compared, %zu entries differ\n", cases, rows, bad);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "failures_driver: %s\n", e.what());
    return 2;
  }
}
