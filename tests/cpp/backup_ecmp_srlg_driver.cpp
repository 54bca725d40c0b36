// backup_ecmp_srlg_driver.cpp — per-primary SRLG-safe backups of ECMP prefixes through the compiled layers, against expected values the
// Python model wrote.
//   backup_ecmp_srlg_driver --engine hip <case files...>   the RAII layer (hspf::Engine::routes_backup_ecmp_srlg_device on DeviceBuffers
//                                                          after hspf_run_device and hspf_routes_device: the sizing call, then the
//                                                          filling call) AND the host interface (hspf::host::HipEngine::routes_device
//                                                          -> backup_routes_ecmp_srlg), every array
//   backup_ecmp_srlg_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                          the host interface's default on an engine without the call:
//                                                          BackupEcmpOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_backup_ecmp_srlg.py writes them from tests/_backup_ecmp_srlg_model.py):
//   n e max_path root run_flags lfa_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   M mem_ptr[K+1] tail[M] pos[M] head[M] cost[M] tail_row[M] head_row[M] | R roots[R] nbr_row[K] | W |
//   P E tflags pfx_ptr[P+1] pfx_vertex[E] pfx_metric[E] | ti_kind[S] ti_via[S] ti_metric[S] ti_p[S] ti_link[S]          (S = 64 W)
//   T eb_ptr[P+1] eb_primary[T] eb_kind[T] eb_slot[T] eb_metric[T] eb_flags[T] eb_coverage[11]
// The per-slot repairs are the model's.  Built by build() and by tests/test_cpp_backup_ecmp_srlg.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, lfa_flags = 0, K = 0, M = 0, R = 0, W = 0, P = 0, E = 0, tflags = 0, T = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row;
  std::vector<uint32_t> mem_ptr, m_tail, m_pos, m_head, m_cost, tail_row, head_row;
  std::vector<uint32_t> pfx_ptr, pfx_vertex, pfx_metric, ti_via, ti_metric, ti_p, ti_link;
  std::vector<uint32_t> eb_ptr, eb_primary, eb_slot, eb_metric, eb_coverage;
  std::vector<uint8_t> vflags, cflags, ti_kind, eb_kind, eb_flags;
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
  const size_t S = 64 * (size_t)c.W;
  take(in, c.ti_kind, S); take(in, c.ti_via, S); take(in, c.ti_metric, S); take(in, c.ti_p, S); take(in, c.ti_link, S);
  in >> c.T;
  take(in, c.eb_ptr, (size_t)c.P + 1); take(in, c.eb_primary, c.T); take(in, c.eb_kind, c.T); take(in, c.eb_slot, c.T); take(in, c.eb_metric, c.T);
  take(in, c.eb_flags, c.T); take(in, c.eb_coverage, HSPF_BK_ECMP_SRLG_COVERAGE_WORDS);
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
      const size_t n = c.n, S = 64 * (size_t)c.W, P = c.P, pw = P * c.W, T = c.T, CW = HSPF_BK_ECMP_SRLG_COVERAGE_WORDS;
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
        const hspf::host::BackupEcmpOut o = static_cast<hspf::host::Engine &>(eng).backup_routes_ecmp_srlg(*run, *routes, c.pfx_ptr, c.pfx_vertex, c.pfx_metric,
                                                                                                           c.tflags, {hp}, {hs}, c.lfa_flags, &hti);
        if (!o.supported && o.eb_ptr.empty() && o.eb_primary.empty() && o.eb_coverage.empty()) ++unsupported;
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
        hspf_prefix_table tr = tab;
        tr.flags |= HSPF_PFX_RESIDENT;                    // the arrays hspf_routes_device has just staged
        hspf::DeviceBuffer ptr(ctx, P * 4 + 4);
        const uint64_t total = eng.routes_backup_ecmp_srlg_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, l, c.lfa_flags, tr, ro,
                                                                  &ti, 0, hspf_backup_ecmp_out{ptr.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
        if (total != T) { printf("  %s: the sizing call says %llu entries, want %zu\n", f, (unsigned long long)total, T); ++b; }
        else {
          hspf::DeviceBuffer prim(ctx, T * 4 + 4), kind(ctx, T + 1), slot(ctx, T * 4 + 4), met(ctx, T * 4 + 4), fl(ctx, T + 1), cov(ctx, CW * 4);
          eng.routes_backup_ecmp_srlg_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, l, c.lfa_flags, tr, ro, &ti, total,
                                             hspf_backup_ecmp_out{ptr.as<uint32_t>(), prim.as<uint32_t>(), kind.as<uint8_t>(), slot.as<uint32_t>(), met.as<uint32_t>(),
                                                                  fl.as<uint8_t>(), cov.as<uint32_t>()});
          b += differ("eb_ptr", ptr.to_host<uint32_t>(P + 1), c.eb_ptr, P + 1) + differ("eb_primary", prim.to_host<uint32_t>(T), c.eb_primary, T);
          b += differ("eb_kind", kind.to_host<uint8_t>(T), c.eb_kind, T) + differ("eb_slot", slot.to_host<uint32_t>(T), c.eb_slot, T);
          b += differ("eb_metric", met.to_host<uint32_t>(T), c.eb_metric, T) + differ("eb_flags", fl.to_host<uint8_t>(T), c.eb_flags, T);
          b += differ("eb_coverage", cov.to_host<uint32_t>(CW), c.eb_coverage, CW);
        }
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      auto routes = heng.routes_device(*run, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags);
      const hspf::host::BackupEcmpOut o = heng.backup_routes_ecmp_srlg(*run, *routes, c.pfx_ptr, c.pfx_vertex, c.pfx_metric, c.tflags, {hp}, {hs}, c.lfa_flags, &hti);
      if (!o.supported || o.n_protected != 1 || o.n_prefixes != c.P || o.eb_primary.size() != T) { printf("  %s: host interface: unsupported, or shape differs\n", f); ++b; }
      else {
        b += differ("host eb_ptr", o.eb_ptr, c.eb_ptr, P + 1) + differ("host eb_primary", o.eb_primary, c.eb_primary, T) + differ("host eb_kind", o.eb_kind, c.eb_kind, T);
        b += differ("host eb_slot", o.eb_slot, c.eb_slot, T) + differ("host eb_metric", o.eb_metric, c.eb_metric, T);
        b += differ("host eb_flags", o.eb_flags, c.eb_flags, T) + differ("host eb_coverage", o.eb_coverage, c.eb_coverage, CW);
      }
      bad += b;
    }
    printf("%zu cases, %zu entries compared, %zu differ, %zu answered not supported\n", cases, n_compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "backup_ecmp_srlg_driver: %s\n", e.what());
    return 2;
  }
}
