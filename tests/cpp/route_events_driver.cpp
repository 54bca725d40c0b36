// route_events_driver.cpp — RibPipeline on an engine WITH the route event stream (Engine::routes_events), step by step against the
// literal restatement: the messages of every step AND, after every step, the pipeline's whole RIB (RibPipeline::full_rib():
// prefix, metric, resolved next hops, routes without next hops included) equal to the RIB the restatement holds.
//   route_events_driver --engine oracle --oracle-so oracle/liboracle_spf.so --golden <dir> <step vectors...>
//   route_events_driver --engine hip --golden <dir> <step vectors...>
// Vectors: the layout tests/cpp/host_parity.cpp replays (a step vector whose `source` names its snapshot under <dir>/isis, optional
// `next`: further whole vectors on the same pipeline).  The CPU stand-in is OracleEngine plus a restatement of hspf_routes_events
// on host vectors.  Built by tests/test_cpp_route_events.py.  TEST INFRASTRUCTURE.
#define main host_parity_main
#include "host_parity.cpp"          // the JSON -> instance helpers of the existing driver (its main is not used)
#undef main

class EventsOracleEngine : public OracleEngine {
 public:
  using OracleEngine::OracleEngine;
  size_t calls = 0, silent = 0;
  RouteEvents routes_events(DeviceRoutes &old_set, DeviceRoutes &new_set, bool with_silent) override {
    const RoutesOut &a = static_cast<OracleRoutes &>(old_set).t, &b = static_cast<OracleRoutes &>(new_set).t;
    const uint32_t R = new_set.n_roots, P = new_set.n_prefixes, W = new_set.mask_words;
    RouteEvents out;
    out.supported = true;
    out.mask_words = W;
    ++calls;
    for (uint32_t r = 0; r < R; ++r)
      for (uint32_t p = 0; p < P; ++p) {
        const size_t i = (size_t)r * P + p;
        const bool had = a.best_entry[i] != 0xFFFFFFFFu, has = b.best_entry[i] != 0xFFFFFFFFu;
        bool same_nh = true, old_nh = false, new_nh = false;
        for (uint32_t w = 0; w < W; ++w) {
          same_nh = same_nh && a.nexthop_mask[i * W + w] == b.nexthop_mask[i * W + w];
          old_nh = old_nh || a.nexthop_mask[i * W + w] != 0; new_nh = new_nh || b.nexthop_mask[i * W + w] != 0;
        }
        uint32_t act;                                   // the rule of include/holo_spf_hip.h (HSPF_DIFF_*)
        if (has) act = (had && a.best_metric[i] == b.best_metric[i] && same_nh) ? HSPF_DIFF_SAME : (new_nh ? HSPF_DIFF_INSTALL : HSPF_DIFF_SILENT);
        else act = had ? (old_nh ? HSPF_DIFF_WITHDRAW : HSPF_DIFF_SILENT) : HSPF_DIFF_SAME;
        if (act == HSPF_DIFF_SAME || (act == HSPF_DIFF_SILENT && !with_silent)) continue;
        if (act == HSPF_DIFF_SILENT) ++silent;
        out.own.insert(out.own.end(), {r, p, act, b.best_metric[i], b.best_entry[i], a.best_metric[i], a.best_entry[i], 0u});
        for (const RoutesOut *t : {&b, &a})
          for (uint32_t w = 0; w < W; ++w) { out.own.push_back((uint32_t)t->nexthop_mask[i * W + w]); out.own.push_back((uint32_t)(t->nexthop_mask[i * W + w] >> 32)); }
        ++out.n;
      }
    out.data = out.own.data();
    return out;
  }
};

struct Counters { int pipelines = 0, steps = 0, bad = 0, lost_and_regained = 0; size_t rows = 0, rows_without_nexthops = 0; };

// the pipeline's RIB against the restatement's rows: same prefixes, metric, next hops (as sets of (address, interface))
static bool same_rib(const I::RibPipeline &pipe, const std::vector<I::RibRow> &want, Counters &c, const char *what) {
  if (!pipe.rib_is_current()) { std::fprintf(stderr, "  %s: the pipeline's RIB is not kept current (engine without events?)\n", what); return false; }
  const std::map<IpKey, I::RibRow> &held = pipe.full_rib();
  std::map<IpKey, const I::RibRow *> rows;
  for (auto &r : want) rows[parse_ip(r.prefix)] = &r;
  bool same = rows.size() == held.size();
  for (auto &kv : rows) {
    auto it = held.find(kv.first);
    if (it == held.end() || it->second.metric != kv.second->metric || !I::detail::same_nexthops(kv.second->nexthops, it->second.nexthops)) {
      same = false;
      std::fprintf(stderr, "  %s: %s metric %u (%zu next hops): the pipeline holds %s\n", what, kv.second->prefix.c_str(), kv.second->metric, kv.second->nexthops.size(),
                   it == held.end() ? "no such row" : ("metric " + std::to_string(it->second.metric) + ", " + std::to_string(it->second.nexthops.size()) + " next hops").c_str());
    }
    c.rows++; c.rows_without_nexthops += kv.second->nexthops.empty();
  }
  if (rows.size() != held.size()) std::fprintf(stderr, "  %s: %zu rows held, %zu in the RIB\n", what, held.size(), rows.size());
  // (the installed view is the rows with next hops)
  size_t installed = 0;
  for (auto &kv : rows) installed += !kv.second->nexthops.empty();
  if (pipe.rib().size() != installed) { std::fprintf(stderr, "  %s: installed view %zu rows, %zu expected\n", what, pipe.rib().size(), installed); same = false; }
  return same;
}

// 1 checked, 0 a difference, -1 not applicable (as check_isis_wire decides for its pipeline leg)
static int check_chain(const J &vec, const std::string &golden_dir, Engine &eng, Counters &c) {
  if (!vec.has("ibus_routes") || !vec.has("rib_before") || vec["proto"].s != "isis") return -1;
  if (vec["source"].s.find("nb-config-summary") != std::string::npos) return -1;
  std::map<std::string, int> ifindex;
  for (auto &kv : vec["ifindex"].obj) ifindex[kv.first] = (int)kv.second.i();
  const I::Instance inst = instance_from_vector(vec);
  std::vector<std::pair<int, int>> tabs;
  for (int lv : inst.config.levels()) for (int mt : {I::MT_STANDARD, I::MT_IPV6_UNICAST}) if (inst.config.is_topology_enabled(mt)) tabs.push_back({lv, mt});
  if (tabs.size() != 1) return -1;
  const std::string src = vec["source"].s;
  const size_t a = src.find("snapshot ");
  if (a == std::string::npos) return -1;
  const size_t sl = src.find('/', a), co = src.find(',', a);
  const J base = load_json(golden_dir + "/isis/" + src.substr(a + 9, sl - a - 9) + "_" + src.substr(sl + 1, co - sl - 1) + ".json");
  const I::Instance inst0 = instance_from_vector(base);
  if (inst0.interfaces.size() != inst.interfaces.size()) return -1;
  for (size_t i = 0; i < inst.interfaces.size(); ++i) {
    const I::Interface &x = inst0.interfaces[i], &y = inst.interfaces[i];
    if (x.name != y.name || x.interface_type != y.interface_type || x.metric != y.metric || x.adjacencies.size() != y.adjacencies.size()) return -1;
    for (size_t k = 0; k < x.adjacencies.size(); ++k)
      if (x.adjacencies[k].system_id != y.adjacencies[k].system_id || x.adjacencies[k].state != y.adjacencies[k].state || x.adjacencies[k].ipv4_addrs != y.adjacencies[k].ipv4_addrs ||
          x.adjacencies[k].ipv6_addrs != y.adjacencies[k].ipv6_addrs || x.adjacencies[k].level_usage != y.adjacencies[k].level_usage || x.adjacencies[k].topologies != y.adjacencies[k].topologies) return -1;
  }
  const I::InstanceCfg &c0 = inst0.config, &c1 = inst.config;
  if (!(c0.level_type == c1.level_type && c0.metric_type == c1.metric_type && c0.ipv4_enabled == c1.ipv4_enabled && c0.ipv6_enabled == c1.ipv6_enabled &&
        c0.mt_ipv6_unicast == c1.mt_ipv6_unicast && c0.att_ignore == c1.att_ignore && c0.max_paths == c1.max_paths && c0.area_addrs == c1.area_addrs)) return -1;
  const int level = tabs[0].first;
  static const I::Lsdb empty;
  I::RibPipeline pipe(inst0, eng, level, tabs[0].second, ifindex);
  // which prefixes lost all their next hops at some step while staying in the RIB, and got some back later
  std::map<std::string, int> nh_state;      // 1: in the RIB without next hops after having had some
  bool regained = false;
  auto track = [&](const std::vector<I::RibRow> &before, const std::vector<I::RibRow> &after) {
    std::map<std::string, bool> had;
    for (auto &r : before) had[r.prefix] = !r.nexthops.empty();
    for (auto &r : after) {
      auto h = had.find(r.prefix);
      if (h != had.end() && h->second && r.nexthops.empty()) nh_state[r.prefix] = 1;
      else if (!r.nexthops.empty() && nh_state.count(r.prefix) && nh_state[r.prefix] == 1) { nh_state[r.prefix] = 2; regained = true; }
    }
  };
  std::vector<I::RibRow> prev_rib = rib_rows(base["rib"]);
  bool ok = true;
  {
    const auto first = pipe.step(inst0, {});
    ++c.steps;
    if (!(first == I::update_global_rib(prev_rib, {}, ifindex))) { std::fprintf(stderr, "  first step: messages differ\n"); ok = false; }
    ok = same_rib(pipe, prev_rib, c, "first step") && ok;
  }
  I::Instance prev_inst = inst0;
  std::vector<const J *> chain{&vec};
  if (vec.has("next")) for (auto &nx : vec["next"].arr) chain.push_back(&nx);
  for (size_t s = 0; s < chain.size() && ok; ++s) {
    I::Instance cur = instance_from_vector(*chain[s]);
    auto p0 = prev_inst.lsdb.find(level), p1 = cur.lsdb.find(level);
    const auto tr = I::changed_lan_ids(p0 == prev_inst.lsdb.end() ? empty : p0->second, p1 == cur.lsdb.end() ? empty : p1->second);
    const auto got = pipe.step(cur, tr);
    ++c.steps;
    const std::vector<I::RibRow> cur_rib = rib_rows((*chain[s])["rib"]);
    const std::string what = "step " + std::to_string(s + 1);
    if (!(got == I::update_global_rib(cur_rib, prev_rib, ifindex))) { std::fprintf(stderr, "  %s: messages differ (%zu)\n", what.c_str(), got.size()); ok = false; }
    ok = same_rib(pipe, cur_rib, c, what.c_str()) && ok;
    track(prev_rib, cur_rib);
    prev_inst = std::move(cur);
    prev_rib = cur_rib;
  }
  if (regained) ++c.lost_and_regained;
  ++c.pipelines;
  return ok ? 1 : 0;
}

int main(int argc, char **argv) {
  std::string engine = "oracle", oracle_so = "oracle/liboracle_spf.so", golden_dir;
  std::vector<std::string> files;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--engine") && i + 1 < argc) engine = argv[++i];
    else if (!strcmp(argv[i], "--oracle-so") && i + 1 < argc) oracle_so = argv[++i];
    else if (!strcmp(argv[i], "--golden") && i + 1 < argc) golden_dir = argv[++i];
    else files.push_back(argv[i]);
  }
  std::unique_ptr<Engine> eng;
  EventsOracleEngine *stand_in = nullptr;
  try {
    if (engine == "hip") {
      if (hspf_device_count() <= 0) { std::printf("no HIP device: the product engine cannot run here\n"); return 77; }
      eng = std::make_unique<HipEngine>(0);
    } else { auto e = std::make_unique<EventsOracleEngine>(oracle_so); stand_in = e.get(); eng = std::move(e); }
  } catch (const std::exception &e) { std::fprintf(stderr, "engine: %s\n", e.what()); return 1; }
  Counters c;
  int skipped = 0;
  for (auto &path : files) {
    try {
      const int r = check_chain(load_json(path), golden_dir, *eng, c);
      if (r < 0) ++skipped;
      else if (r == 0) { ++c.bad; std::fprintf(stderr, "RIB / MESSAGE MISMATCH %s\n", path.c_str()); }
    } catch (const std::exception &e) { ++c.bad; std::fprintf(stderr, "EXCEPTION %s: %s\n", path.c_str(), e.what()); }
  }
  if (stand_in) std::printf("stand-in engine: %zu routes_events calls, %zu SILENT records\n", stand_in->calls, stand_in->silent);
  std::printf("%d pipelines (%d steps) followed through the event stream, %d differ, %d not applicable; %zu RIB rows compared, %zu of them without next hops; "
              "%d chains in which a route lost all its next hops and regained them\n", c.pipelines, c.steps, c.bad, skipped, c.rows, c.rows_without_nexthops, c.lost_and_regained);
  return c.bad ? 1 : 0;
}
