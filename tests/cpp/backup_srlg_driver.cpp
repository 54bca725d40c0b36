// backup_srlg_driver.cpp — per-prefix SRLG-safe backups through the compiled layers, against expected values the Python model wrote.
//   backup_srlg_driver --engine hip <case files...>     the RAII layer (hspf::Engine::routes_backup_srlg_device on DeviceBuffers after
//                                                       hspf_run_device and hspf_routes_device) AND the host interface
//                                                       (hspf::host::HipEngine::routes_device -> backup_routes_srlg), every array
//   backup_srlg_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                       the host interface's default on an engine without the call:
//                                                       BackupOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_backup_srlg.py writes them from tests/_backup_srlg_model.py):
//   n e max_path root run_flags lfa_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   M mem_ptr[K+1] tail[M] pos[M] head[M] cost[M] tail_row[M] head_row[M] | R roots[R] nbr_row[K] | W |
//   P E tflags pfx_ptr[P+1] pfx_vertex[E] pfx_metric[E] | ti_kind[S] ti_via[S] ti_metric[S] ti_p[S] ti_link[S]          (S = 64 W)
//   bk_kind[P] bk_primary[P] bk_slot[P] bk_metric[P] bk_flags[P] bk_cand_mask[PW] bk_node_mask[PW] bk_coverage[10]
// The per-slot repairs are the model's (tests/test_cpp_srlg.py takes the calls that write them through the same layers).
// Built by build() and by tests/test_cpp_backup_srlg.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, lfa_flags = 0, K = 0, M = 0, R = 0, W = 0, P = 0, E = 0, tflags = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row;
  std::vector<uint32_t> mem_ptr, m_tail, m_pos, m_head, m_cost, tail_row, head_row;
  std::vector<uint32_t> pfx_ptr, pfx_vertex, pfx_metric, ti_via, ti_metric, ti_p, ti_link;
  std::vector<uint32_t> bk_primary, bk_slot, bk_metric, bk_coverage;
  std::vector<uint64_t> bk_cand_mask, bk_node_mask;
  std::vector<uint8_t> vflags, cflags, ti_kind, bk_kind, bk_flags;
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
  in >> c.M;
  take(in, c.mem_ptr, (size_t)c.K + 1); take(in, c.m_tail, c.M); take(in, c.m_pos, c.M); take(in, c.m_head, c.M); take(in, c.m_cost, c.M);
  take(in, c.tail_row, c.M); take(in, c.head_row, c.M);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.nbr_row, c.K);
  in >> c.W >> c.P >> c.E >> c.tflags;
  take(in, c.pfx_ptr, (size_t)c.P + 1); take(in, c.pfx_vertex, c.E); take(in, c.pfx_metric, c.E);
  const size_t S = 64 * (size_t)c.W, pw = (size_t)c.P * c.W;
  take(in, c.ti_kind, S); take(in, c.ti_via, S); take(in, c.ti_metric, S); take(in, c.ti_p, S); take(in, c.ti_link, S);
  take(in, c.bk_kind, c.P); take(in, c.bk_primary, c.P); take(in, c.bk_slot, c.P); take(in, c.bk_metric, c.P); take(in, c.bk_flags, c.P);
  take(in, c.bk_cand_mask, pw); take(in, c.bk_node_mask, pw); take(in, c.bk_coverage, HSPF_BK_SRLG_COVERAGE_WORDS);
  if (!in) throw std::runtime_error(std::string("short case file ") + path);
  return c;
}

size_t n_compared = 0;      // entries differ() has looked at

template <typename A, typename B>
size_t differ(const char *what, const A &got, const B &want, size_t count) {
  n_compared += count;
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
    size_t cases = 0, bad = 0, unsupported = 0;
    for (const char *f : files) {
      const Case c = load(f);
      ++cases;
      const size_t n = c.n, S = 64 * (size_t)c.W, P = c.P, pw = P * c.W;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      const hspf::host::Srlg hs{c.mem_ptr, c.m_tail, c.m_pos, c.m_head, c.m_cost, c.tail_row, c.head_row};
      hspf::host::TilfaOut hti;
      hti.supported = true; hti.n_protected = 1; hti.n_vertices = c.n; hti.slot_stride = (uint32_t)S;
      hti.ti_kind = c.ti_kind; hti.ti_via = c.ti_via; hti.ti_metric = c.ti_metric; hti.ti_p = c.ti_p; hti.ti_link = c.ti_link;
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        auto routes = eng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
        const hspf::host::BackupOut o = static_cast<hspf::host::Engine &>(eng).backup_routes_srlg(*run, *routes, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags,
                                                                                                 {hp}, {hs}, c.lfa_flags, &hti);
        if (!o.supported && o.bk_kind.empty() && o.bk_coverage.empty() && o.bk_cand_mask.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      {
        // the RAII layer, on device buffers of its own
        hspf::Engine eng(0);
        hspf_ctx *ctx = eng.raw();
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        const size_t rn = (size_t)c.R * n;
        hspf::DeviceBuffer dist(ctx, rn * 4), flags(ctx, rn * 2), mask(ctx, rn * 8 * c.W);
        hspf_result res{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), c.W, nullptr};
        if (hspf_run_device(ctx, g.raw(), c.roots.data(), c.R, c.run_flags, &res) != HSPF_OK) throw std::runtime_error(std::string("hspf_run_device: ") + hspf_last_error(ctx));
        hspf::DeviceBuffer bm(ctx, P * 4 + 4), be(ctx, P * 4 + 4), nh(ctx, pw * 8 + 8);
        const hspf_prefix_table tab{c.P, c.E, c.pfx_ptr.data(), c.pfx_vertex.data(), c.pfx_metric.data(), c.tflags, nullptr, nullptr, nullptr, nullptr};
        hspf_routes ro{bm.as<uint32_t>(), be.as<uint32_t>(), nh.as<uint64_t>()};
        if (hspf_routes_device(ctx, c.n, 1, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), &tab, &ro) != HSPF_OK)
          throw std::runtime_error(std::string("hspf_routes_device: ") + hspf_last_error(ctx));
        hspf::DeviceBuffer tk(ctx, S), tv(ctx, S * 4), tm(ctx, S * 4), tp(ctx, S * 4), tl(ctx, S * 4);
        auto up = [&](hspf::DeviceBuffer &d, const void *src, size_t bytes) {
          if (hspf_host_to_device(ctx, d.as<void>(), src, bytes) != HSPF_OK) throw std::runtime_error(std::string("hspf_host_to_device: ") + hspf_last_error(ctx));
        };
        up(tk, c.ti_kind.data(), S); up(tv, c.ti_via.data(), S * 4); up(tm, c.ti_metric.data(), S * 4); up(tp, c.ti_p.data(), S * 4); up(tl, c.ti_link.data(), S * 4);
        const hspf_tilfa_out ti{tk.as<uint8_t>(), tp.as<uint32_t>(), nullptr, tv.as<uint32_t>(), tl.as<uint32_t>(), tm.as<uint32_t>(), nullptr, nullptr, nullptr};
        const std::vector<hspf_lfa_protect> p{{c.root, 0u, c.K, c.nbr.data(), c.nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()}};
        const std::vector<hspf_srlg> l{{c.mem_ptr.data(), c.m_tail.data(), c.m_pos.data(), c.m_head.data(), c.m_cost.data(), c.tail_row.data(), c.head_row.data()}};
        hspf::DeviceBuffer kind(ctx, P + 1), prim(ctx, P * 4 + 4), slot(ctx, P * 4 + 4), met(ctx, P * 4 + 4), fl(ctx, P + 1), cm(ctx, pw * 8 + 8), nm(ctx, pw * 8 + 8),
            cov(ctx, HSPF_BK_SRLG_COVERAGE_WORDS * 4);
        hspf_prefix_table tr = tab;
        tr.flags |= HSPF_PFX_RESIDENT;                    // the arrays hspf_routes_device has just staged
        eng.routes_backup_srlg_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, l, c.lfa_flags, tr, ro, &ti,
                                      hspf_backup_out{kind.as<uint8_t>(), prim.as<uint32_t>(), slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), cm.as<uint64_t>(),
                                                      nm.as<uint64_t>(), cov.as<uint32_t>()});
        b += differ("bk_kind", kind.to_host<uint8_t>(P), c.bk_kind, P) + differ("bk_primary", prim.to_host<uint32_t>(P), c.bk_primary, P);
        b += differ("bk_slot", slot.to_host<uint32_t>(P), c.bk_slot, P) + differ("bk_metric", met.to_host<uint32_t>(P), c.bk_metric, P);
        b += differ("bk_flags", fl.to_host<uint8_t>(P), c.bk_flags, P) + differ("bk_cand_mask", cm.to_host<uint64_t>(pw), c.bk_cand_mask, pw);
        b += differ("bk_node_mask", nm.to_host<uint64_t>(pw), c.bk_node_mask, pw);
        b += differ("bk_coverage", cov.to_host<uint32_t>(HSPF_BK_SRLG_COVERAGE_WORDS), c.bk_coverage, HSPF_BK_SRLG_COVERAGE_WORDS);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      auto routes = heng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
      const hspf::host::BackupOut o = heng.backup_routes_srlg(*run, *routes, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags, {hp}, {hs}, c.lfa_flags, &hti);
      if (!o.supported || o.n_prefixes != c.P || o.mask_words != c.W) { printf("  %s: host interface: unsupported, or shape differs\n", f); ++b; }
      else {
        b += differ("host bk_kind", o.bk_kind, c.bk_kind, P) + differ("host bk_primary", o.bk_primary, c.bk_primary, P) + differ("host bk_slot", o.bk_slot, c.bk_slot, P);
        b += differ("host bk_metric", o.bk_metric, c.bk_metric, P) + differ("host bk_flags", o.bk_flags, c.bk_flags, P);
        b += differ("host bk_cand_mask", o.bk_cand_mask, c.bk_cand_mask, pw) + differ("host bk_node_mask", o.bk_node_mask, c.bk_node_mask, pw);
        b += differ("host bk_coverage", o.bk_coverage, c.bk_coverage, HSPF_BK_SRLG_COVERAGE_WORDS);
      }
      bad += b;
    }
    printf("%zu cases, %zu entries compared, %zu differ, %zu answered not supported\n", cases, n_compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "backup_srlg_driver: %s\n", e.what());
    return 2;
  }
}
