// lfa_lan_driver.cpp — broadcast-link protection through the compiled layers, against expected values the Python model wrote.
//   lfa_lan_driver --engine hip <case files...>      the RAII layer (hspf::Engine: lfa_lan_candidates, lfa_lan_device, hspf_routes_device,
//                                                    routes_backup_lan_device on DeviceBuffers) AND the host interface
//                                                    (hspf::host::HipEngine::lfa_lan on a DeviceRun), every array compared
//   lfa_lan_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                    the host interface's defaults on an engine without the calls:
//                                                    LfaOut / BackupOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_lfa_lan.py writes them from tests/_lfa_lan_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] lan[K] |
//   R roots[R] nbr_row[K] lan_row[K] | W alt_slot[n] alt_metric[n] alt_flags[n] cand_mask[nW] node_mask[nW] coverage[7] |
//   P E tflags pfx_ptr[P+1] pfx_vertex[E] pfx_metric[E] |
//   bk_kind[P] bk_primary[P] bk_slot[P] bk_metric[P] bk_flags[P] bk_cand_mask[PW] bk_node_mask[PW] bk_coverage[9]
// Built by tests/test_cpp_lfa_lan.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, K = 0, R = 0, W = 0, P = 0, E = 0, tflags = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, lan, roots, nbr_row, lan_row;
  std::vector<uint32_t> alt_slot, alt_metric, coverage, pfx_ptr, pfx_vertex, pfx_metric, bk_primary, bk_slot, bk_metric, bk_coverage;
  std::vector<uint64_t> cand_mask, node_mask, bk_cand_mask, bk_node_mask;
  std::vector<uint8_t> vflags, cflags, alt_flags, bk_kind, bk_flags;
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
  take(in, c.nbr, c.K); take(in, c.cost, c.K); take(in, c.root_link, c.K); take(in, c.cflags, c.K); take(in, c.lan, c.K);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.nbr_row, c.K); take(in, c.lan_row, c.K);
  in >> c.W;
  const size_t nw = (size_t)c.n * c.W;
  take(in, c.alt_slot, c.n); take(in, c.alt_metric, c.n); take(in, c.alt_flags, c.n); take(in, c.cand_mask, nw); take(in, c.node_mask, nw);
  take(in, c.coverage, HSPF_LFA_LAN_COVERAGE_WORDS);
  in >> c.P >> c.E >> c.tflags;
  take(in, c.pfx_ptr, (size_t)c.P + 1); take(in, c.pfx_vertex, c.E); take(in, c.pfx_metric, c.E);
  const size_t pw = (size_t)c.P * c.W;
  take(in, c.bk_kind, c.P); take(in, c.bk_primary, c.P); take(in, c.bk_slot, c.P); take(in, c.bk_metric, c.P); take(in, c.bk_flags, c.P);
  take(in, c.bk_cand_mask, pw); take(in, c.bk_node_mask, pw); take(in, c.bk_coverage, HSPF_BK_LAN_COVERAGE_WORDS);
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
      const size_t n = c.n, nw = n * c.W, P = c.P, pw = P * c.W;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      const hspf::host::LfaLan hl{c.lan, c.lan_row};
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        auto routes = eng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
        hspf::host::Engine &base = eng;
        const hspf::host::LfaOut o = base.lfa_lan(*run, {hp}, {hl}, 0, true);
        const hspf::host::BackupOut b = base.backup_routes_lan(*run, *routes, {hp}, {hl}, 0, nullptr);
        if (!o.supported && o.alt_slot.empty() && o.coverage.empty() && !b.supported && b.bk_kind.empty() && b.bk_coverage.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      {
        // the RAII layer, on device buffers of its own
        hspf::Engine eng(0);
        hspf_ctx *ctx = eng.raw();
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        b += differ("lan", hspf::Engine::lfa_lan_candidates(c.row_ptr, c.col, c.metric, c.vflags, c.root), c.lan, c.K);
        const size_t rn = (size_t)c.R * n;
        hspf::DeviceBuffer dist(ctx, rn * 4), flags(ctx, rn * 2), mask(ctx, rn * 8 * c.W);
        hspf_result res{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), c.W, nullptr};
        if (hspf_run_device(ctx, g.raw(), c.roots.data(), c.R, c.run_flags, &res) != HSPF_OK) throw std::runtime_error(std::string("hspf_run_device: ") + hspf_last_error(ctx));
        const std::vector<hspf_lfa_protect> p{{c.root, 0u, c.K, c.nbr.data(), c.nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()}};
        const std::vector<hspf_lfa_lan> l{{c.lan.data(), c.lan_row.data()}};
        hspf::DeviceBuffer slot(ctx, n * 4), met(ctx, n * 4), fl(ctx, n), cm(ctx, nw * 8), nm(ctx, nw * 8), cov(ctx, HSPF_LFA_LAN_COVERAGE_WORDS * 4);
        eng.lfa_lan_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, l, 0,
                           hspf_lfa_out{slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cm.as<uint64_t>(), nm.as<uint64_t>(), cov.as<uint32_t>()});
        b += differ("alt_slot", slot.to_host<uint32_t>(n), c.alt_slot, n) + differ("alt_metric", met.to_host<uint32_t>(n), c.alt_metric, n);
        b += differ("alt_flags", fl.to_host<uint8_t>(n), c.alt_flags, n) + differ("cand_mask", cm.to_host<uint64_t>(nw), c.cand_mask, nw);
        b += differ("node_mask", nm.to_host<uint64_t>(nw), c.node_mask, nw);
        b += differ("coverage", cov.to_host<uint32_t>(HSPF_LFA_LAN_COVERAGE_WORDS), c.coverage, HSPF_LFA_LAN_COVERAGE_WORDS);
        const size_t rp = (size_t)c.R * P;
        hspf::DeviceBuffer bm(ctx, rp * 4), be(ctx, rp * 4), nh(ctx, rp * 8 * c.W);
        const hspf_prefix_table tab{c.P, c.E, c.pfx_ptr.data(), c.pfx_vertex.data(), c.pfx_metric.data(), c.tflags};
        hspf_routes ro{bm.as<uint32_t>(), be.as<uint32_t>(), nh.as<uint64_t>()};
        if (hspf_routes_device(ctx, c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), &tab, &ro) != HSPF_OK)
          throw std::runtime_error(std::string("hspf_routes_device: ") + hspf_last_error(ctx));
        hspf::DeviceBuffer kk(ctx, P), kp(ctx, P * 4), ks(ctx, P * 4), km(ctx, P * 4), kf(ctx, P), kc(ctx, pw * 8), kn(ctx, pw * 8), kv(ctx, HSPF_BK_LAN_COVERAGE_WORDS * 4);
        eng.routes_backup_lan_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, l, 0, tab, ro, nullptr,
                                     hspf_backup_out{kk.as<uint8_t>(), kp.as<uint32_t>(), ks.as<uint32_t>(), km.as<uint32_t>(), kf.as<uint8_t>(), kc.as<uint64_t>(),
                                                     kn.as<uint64_t>(), kv.as<uint32_t>()});
        b += differ("bk_kind", kk.to_host<uint8_t>(P), c.bk_kind, P) + differ("bk_primary", kp.to_host<uint32_t>(P), c.bk_primary, P);
        b += differ("bk_slot", ks.to_host<uint32_t>(P), c.bk_slot, P) + differ("bk_metric", km.to_host<uint32_t>(P), c.bk_metric, P);
        b += differ("bk_flags", kf.to_host<uint8_t>(P), c.bk_flags, P) + differ("bk_cand_mask", kc.to_host<uint64_t>(pw), c.bk_cand_mask, pw);
        b += differ("bk_node_mask", kn.to_host<uint64_t>(pw), c.bk_node_mask, pw);
        b += differ("bk_coverage", kv.to_host<uint32_t>(HSPF_BK_LAN_COVERAGE_WORDS), c.bk_coverage, HSPF_BK_LAN_COVERAGE_WORDS);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      const hspf::host::LfaOut o = heng.lfa_lan(*run, {hp}, {hl}, 0, true);
      if (!o.supported || o.n_vertices != c.n || o.mask_words != c.W) { printf("  %s: host interface: unsupported, or shape differs\n", f); ++b; }
      else
        b += differ("host alt_slot", o.alt_slot, c.alt_slot, n) + differ("host alt_metric", o.alt_metric, c.alt_metric, n) + differ("host alt_flags", o.alt_flags, c.alt_flags, n) +
             differ("host cand_mask", o.cand_mask, c.cand_mask, nw) + differ("host node_mask", o.node_mask, c.node_mask, nw) +
             differ("host coverage", o.coverage, c.coverage, HSPF_LFA_LAN_COVERAGE_WORDS);
      compared += 2 * n + P;
      bad += b;
    }
    printf("%zu cases, %zu entries compared, %zu differ, %zu answered not supported\n", cases, compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "lfa_lan_driver: %s\n", e.what());
    return 2;
  }
}
