// srlg_driver.cpp — SRLG-safe alternates and remote-LFA spaces through the compiled layers, against expected values the Python model
// wrote.
//   srlg_driver --engine hip <case files...>     the RAII layer (hspf::Engine: srlg_members on the host, then lfa_srlg_device,
//                                                rlfa_srlg_device, tilfa_device on DeviceBuffers, nothing leaving the device in
//                                                between) AND the host interface (hspf::host::HipEngine::lfa_srlg -> rlfa_srlg ->
//                                                tilfa on two DeviceRuns), every array
//   srlg_driver --engine oracle --oracle-so oracle/liboracle_spf.so <case files...>
//                                                the host interface's default on an engine without the calls:
//                                                LfaOut / RlfaOut::supported == false, nothing else filled in
// A case file is a list of decimal numbers (tests/test_cpp_srlg.py writes them from tests/_srlg_model.py):
//   n e max_path root run_flags | row_ptr[n+1] col[e] metric[e] vflags[n] | K nbr[K] cost[K] root_link[K] cflags[K] |
//   grp_ptr[e+1] G grp[G] | M mem_ptr[K+1] tail[M] pos[M] head[M] cost[M] | R roots[R] nbr_row[K] tail_row[M] head_row[M] | W |
//   alt_slot[n] alt_metric[n] alt_flags[n] coverage[7] |
//   pq_node[S] pq_via[S] pq_metric[S] pq_counts[5S] space_flags[Sn] space_via[Sn] rl_node[n] rl_via[n] rl_coverage[6] |
//   ti_kind[S] ti_p[S] ti_q[S] ti_via[S] ti_link[S] ti_metric[S] ti_counts[2S] td_kind[n] td_coverage[5]            (S = 64 W)
// Built by build() and by tests/test_cpp_srlg.py.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "holo_spf_hip.hpp"
#include "holo_spf_host.hpp"
#include "oracle_engine.hpp"

namespace {

struct Case {
  uint32_t n = 0, e = 0, maxp = 0, root = 0, run_flags = 0, K = 0, R = 0, W = 0, G = 0, M = 0;
  std::vector<uint32_t> row_ptr, col, metric, nbr, cost, root_link, roots, nbr_row;
  std::vector<uint32_t> grp_ptr, grp, mem_ptr, m_tail, m_pos, m_head, m_cost, tail_row, head_row;
  std::vector<uint32_t> alt_slot, alt_metric, coverage;
  std::vector<uint8_t> alt_flags;
  std::vector<uint32_t> pq_node, pq_via, pq_metric, pq_counts, space_via, rl_node, rl_via, rl_coverage;
  std::vector<uint32_t> ti_p, ti_q, ti_via, ti_link, ti_metric, ti_counts, td_coverage;
  std::vector<uint8_t> vflags, cflags, space_flags, ti_kind, td_kind;
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
  take(in, c.grp_ptr, (size_t)c.e + 1);
  in >> c.G;
  take(in, c.grp, c.G);
  in >> c.M;
  take(in, c.mem_ptr, (size_t)c.K + 1); take(in, c.m_tail, c.M); take(in, c.m_pos, c.M); take(in, c.m_head, c.M); take(in, c.m_cost, c.M);
  in >> c.R;
  take(in, c.roots, c.R); take(in, c.nbr_row, c.K); take(in, c.tail_row, c.M); take(in, c.head_row, c.M);
  in >> c.W;
  take(in, c.alt_slot, c.n); take(in, c.alt_metric, c.n); take(in, c.alt_flags, c.n); take(in, c.coverage, HSPF_LFA_SRLG_COVERAGE_WORDS);
  const size_t S = 64 * (size_t)c.W, sn = S * c.n;
  take(in, c.pq_node, S); take(in, c.pq_via, S); take(in, c.pq_metric, S); take(in, c.pq_counts, S * HSPF_RLFA_SRLG_COUNT_WORDS);
  take(in, c.space_flags, sn); take(in, c.space_via, sn); take(in, c.rl_node, c.n); take(in, c.rl_via, c.n);
  take(in, c.rl_coverage, HSPF_RLFA_SRLG_COVERAGE_WORDS);
  take(in, c.ti_kind, S); take(in, c.ti_p, S); take(in, c.ti_q, S); take(in, c.ti_via, S); take(in, c.ti_link, S); take(in, c.ti_metric, S);
  take(in, c.ti_counts, S * HSPF_TILFA_COUNT_WORDS); take(in, c.td_kind, c.n); take(in, c.td_coverage, HSPF_TILFA_COVERAGE_WORDS);
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
      const size_t n = c.n, S = 64 * (size_t)c.W, sn = S * n;
      hspf::host::LfaProtect hp;
      hp.root_vertex = c.root; hp.root_row = 0; hp.nbr = c.nbr; hp.nbr_row = c.nbr_row; hp.cost = c.cost; hp.root_link = c.root_link; hp.cflags = c.cflags;
      const hspf::host::Srlg hs{c.mem_ptr, c.m_tail, c.m_pos, c.m_head, c.m_cost, c.tail_row, c.head_row};
      if (engine == "oracle") {
        OracleEngine eng(oracle_so);
        auto g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        auto run = eng.run_device(*g, c.roots, c.run_flags);
        const hspf::host::LfaOut a = static_cast<hspf::host::Engine &>(eng).lfa_srlg(*run, {hp}, {hs}, 0, false);
        const hspf::host::RlfaOut o = static_cast<hspf::host::Engine &>(eng).rlfa_srlg(*g, *run, *run, {hp}, {hs}, 0, nullptr, true);
        if (!a.supported && a.alt_slot.empty() && a.coverage.empty() && !o.supported && o.pq_node.empty() && o.pq_counts.empty() && o.rl_coverage.empty()) ++unsupported;
        continue;
      }
      size_t b = 0;
      const hspf::Engine::Transposed t = hspf::Engine::csr_transpose(c.row_ptr, c.col, c.metric, c.vflags);
      {
        // the member lists from the group table, through the RAII layer's host call
        hspf::Engine::SrlgMembers sm = hspf::Engine::srlg_members(c.row_ptr, c.col, c.metric, c.vflags, c.root, c.grp_ptr, c.grp);
        b += differ("mem_ptr", sm.mem_ptr, c.mem_ptr, (size_t)c.K + 1) + (sm.mem_ptr.size() != (size_t)c.K + 1) + (sm.tail.size() != c.M);
        b += differ("tail", sm.tail, c.m_tail, c.M) + differ("pos", sm.pos, c.m_pos, c.M) + differ("head", sm.head, c.m_head, c.M) + differ("cost", sm.cost, c.m_cost, c.M);
        sm.tail_row = c.tail_row; sm.head_row = c.head_row;
        // the RAII layer, on device buffers of its own
        hspf::Engine eng(0);
        hspf_ctx *ctx = eng.raw();
        hspf::Graph g = eng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
        hspf::Graph gt = eng.upload(t.row_ptr, t.col, t.metric, c.vflags, c.maxp);
        const size_t rn = (size_t)c.R * n;
        hspf::DeviceBuffer dist(ctx, rn * 4), flags(ctx, rn * 2), mask(ctx, rn * 8 * c.W), rdist(ctx, rn * 4);
        hspf_result res{dist.as<uint32_t>(), nullptr, flags.as<uint16_t>(), mask.as<uint64_t>(), c.W, nullptr};
        if (hspf_run_device(ctx, g.raw(), c.roots.data(), c.R, c.run_flags, &res) != HSPF_OK) throw std::runtime_error(std::string("hspf_run_device: ") + hspf_last_error(ctx));
        hspf_result rres{rdist.as<uint32_t>(), nullptr, nullptr, nullptr, 1, nullptr};
        if (hspf_run_device(ctx, gt.raw(), c.roots.data(), c.R, c.run_flags, &rres) != HSPF_OK) throw std::runtime_error(std::string("hspf_run_device (transposed): ") + hspf_last_error(ctx));
        const std::vector<hspf_lfa_protect> p{{c.root, 0u, c.K, c.nbr.data(), c.nbr_row.data(), c.cost.data(), c.root_link.data(), c.cflags.data()}};
        const std::vector<hspf_srlg> l{sm.raw()};
        hspf::DeviceBuffer slot(ctx, n * 4), met(ctx, n * 4), fl(ctx, n), cov(ctx, HSPF_LFA_SRLG_COVERAGE_WORDS * 4);
        eng.lfa_srlg_device(c.n, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), p, l, 0,
                            hspf_lfa_out{slot.as<uint32_t>(), met.as<uint32_t>(), fl.as<uint8_t>(), nullptr, nullptr, cov.as<uint32_t>()});
        b += differ("alt_slot", slot.to_host<uint32_t>(n), c.alt_slot, n) + differ("alt_metric", met.to_host<uint32_t>(n), c.alt_metric, n);
        b += differ("alt_flags", fl.to_host<uint8_t>(n), c.alt_flags, n);
        b += differ("coverage", cov.to_host<uint32_t>(HSPF_LFA_SRLG_COVERAGE_WORDS), c.coverage, HSPF_LFA_SRLG_COVERAGE_WORDS);
        hspf::DeviceBuffer qn(ctx, S * 4), qv(ctx, S * 4), qm(ctx, S * 4), qc(ctx, S * 4 * HSPF_RLFA_SRLG_COUNT_WORDS), sf(ctx, sn), sv(ctx, sn * 4), rn_(ctx, n * 4),
            rv(ctx, n * 4), rc(ctx, HSPF_RLFA_SRLG_COVERAGE_WORDS * 4);
        eng.rlfa_srlg_device(g, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), rdist.as<uint32_t>(), p, l, 0, fl.as<uint8_t>(),
                            hspf_rlfa_out{qn.as<uint32_t>(), qv.as<uint32_t>(), qm.as<uint32_t>(), qc.as<uint32_t>(), sf.as<uint8_t>(), sv.as<uint32_t>(), rn_.as<uint32_t>(),
                                          rv.as<uint32_t>(), rc.as<uint32_t>()});
        b += differ("pq_node", qn.to_host<uint32_t>(S), c.pq_node, S) + differ("pq_via", qv.to_host<uint32_t>(S), c.pq_via, S);
        b += differ("pq_metric", qm.to_host<uint32_t>(S), c.pq_metric, S);
        b += differ("pq_counts", qc.to_host<uint32_t>(S * HSPF_RLFA_SRLG_COUNT_WORDS), c.pq_counts, S * HSPF_RLFA_SRLG_COUNT_WORDS);
        b += differ("space_flags", sf.to_host<uint8_t>(sn), c.space_flags, sn) + differ("space_via", sv.to_host<uint32_t>(sn), c.space_via, sn);
        b += differ("rl_node", rn_.to_host<uint32_t>(n), c.rl_node, n) + differ("rl_via", rv.to_host<uint32_t>(n), c.rl_via, n);
        b += differ("rl_coverage", rc.to_host<uint32_t>(HSPF_RLFA_SRLG_COVERAGE_WORDS), c.rl_coverage, HSPF_RLFA_SRLG_COVERAGE_WORDS);
        hspf::DeviceBuffer tk(ctx, S), tp(ctx, S * 4), tq(ctx, S * 4), tv(ctx, S * 4), tl(ctx, S * 4), tm(ctx, S * 4), tc(ctx, S * 4 * HSPF_TILFA_COUNT_WORDS), dk(ctx, n),
            dc(ctx, HSPF_TILFA_COVERAGE_WORDS * 4);
        eng.tilfa_device(g, c.R, c.W, dist.as<uint32_t>(), flags.as<uint16_t>(), mask.as<uint64_t>(), rdist.as<uint32_t>(), p, 0, fl.as<uint8_t>(), sf.as<uint8_t>(),
                         sv.as<uint32_t>(),
                         hspf_tilfa_out{tk.as<uint8_t>(), tp.as<uint32_t>(), tq.as<uint32_t>(), tv.as<uint32_t>(), tl.as<uint32_t>(), tm.as<uint32_t>(), tc.as<uint32_t>(),
                                        dk.as<uint8_t>(), dc.as<uint32_t>()});
        b += differ("ti_kind", tk.to_host<uint8_t>(S), c.ti_kind, S) + differ("ti_p", tp.to_host<uint32_t>(S), c.ti_p, S) + differ("ti_q", tq.to_host<uint32_t>(S), c.ti_q, S);
        b += differ("ti_via", tv.to_host<uint32_t>(S), c.ti_via, S) + differ("ti_link", tl.to_host<uint32_t>(S), c.ti_link, S);
        b += differ("ti_metric", tm.to_host<uint32_t>(S), c.ti_metric, S);
        b += differ("ti_counts", tc.to_host<uint32_t>(S * HSPF_TILFA_COUNT_WORDS), c.ti_counts, S * HSPF_TILFA_COUNT_WORDS);
        b += differ("td_kind", dk.to_host<uint8_t>(n), c.td_kind, n);
        b += differ("td_coverage", dc.to_host<uint32_t>(HSPF_TILFA_COVERAGE_WORDS), c.td_coverage, HSPF_TILFA_COVERAGE_WORDS);
      }
      // the host interface on the product engine
      hspf::host::HipEngine heng(0);
      auto hg = heng.upload(c.row_ptr, c.col, c.metric, c.vflags, c.maxp);
      auto hgt = heng.upload(t.row_ptr, t.col, t.metric, c.vflags, c.maxp);
      auto run = heng.run_device(*hg, c.roots, c.run_flags);
      auto rrun = heng.run_device(*hgt, c.roots, c.run_flags);
      const hspf::host::LfaOut lo = heng.lfa_srlg(*run, {hp}, {hs}, 0, false);
      const hspf::host::RlfaOut o = heng.rlfa_srlg(*hg, *run, *rrun, {hp}, {hs}, 0, &lo, true);
      if (!lo.supported) { printf("  %s: host interface: lfa_srlg unsupported\n", f); ++b; }
      else
        b += differ("host alt_slot", lo.alt_slot, c.alt_slot, n) + differ("host alt_metric", lo.alt_metric, c.alt_metric, n) +
             differ("host alt_flags", lo.alt_flags, c.alt_flags, n) + differ("host coverage", lo.coverage, c.coverage, HSPF_LFA_SRLG_COVERAGE_WORDS);
      if (!o.supported || o.n_vertices != c.n || o.slot_stride != S) { printf("  %s: host interface: unsupported, or shape differs\n", f); ++b; }
      else {
        b += differ("host pq_node", o.pq_node, c.pq_node, S) + differ("host pq_via", o.pq_via, c.pq_via, S) + differ("host pq_metric", o.pq_metric, c.pq_metric, S);
        b += differ("host pq_counts", o.pq_counts, c.pq_counts, S * HSPF_RLFA_SRLG_COUNT_WORDS) + differ("host space_flags", o.space_flags, c.space_flags, sn);
        b += differ("host space_via", o.space_via, c.space_via, sn) + differ("host rl_node", o.rl_node, c.rl_node, n) + differ("host rl_via", o.rl_via, c.rl_via, n);
        b += differ("host rl_coverage", o.rl_coverage, c.rl_coverage, HSPF_RLFA_SRLG_COVERAGE_WORDS);
        const hspf::host::TilfaOut ti = heng.tilfa(*hg, *run, *rrun, {hp}, 0, &lo, o);
        if (!ti.supported) { printf("  %s: host interface: tilfa unsupported\n", f); ++b; }
        else
          b += differ("host ti_kind", ti.ti_kind, c.ti_kind, S) + differ("host ti_p", ti.ti_p, c.ti_p, S) + differ("host ti_q", ti.ti_q, c.ti_q, S) +
               differ("host ti_via", ti.ti_via, c.ti_via, S) + differ("host ti_link", ti.ti_link, c.ti_link, S) +
               differ("host ti_counts", ti.ti_counts, c.ti_counts, S * HSPF_TILFA_COUNT_WORDS) +
               differ("host ti_metric", ti.ti_metric, c.ti_metric, S) + differ("host td_kind", ti.td_kind, c.td_kind, n) +
               differ("host td_coverage", ti.td_coverage, c.td_coverage, HSPF_TILFA_COVERAGE_WORDS);
      }
      bad += b;
    }
    printf("%zu cases, %zu entries compared, %zu differ, %zu answered not supported\n", cases, n_compared, bad, unsupported);
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "srlg_driver: %s\n", e.what());
    return 2;
  }
}
