// Node-level A/B of the slot placement (not product code): one MultiNode of G
// groups x 3 (default 1,048,576) whose even group ids are led by this node and
// whose odd ids follow node 2, so that led and followed groups alternate slot by
// slot in arrival order; under HBN_PLACE_ARRIVAL or HBN_PLACE_ROLE
// (argv[1] = arrival | role) it times
//   tick cycles   hbn_tick + hbn_ready + storage append + hbn_advance (every
//                 leader beats: heartbeat_tick 1; election_tick is large)
//   mixed cycles  per led group a proposal and its two followers' MsgAppResp
//                 for the previous entry, per followed group its leader's MsgApp
//                 (one entry) and MsgHeartbeat, through hbn_step_many /
//                 hbn_propose_many, then Ready / append / Advance
// and prints one JSON line: wall ms per cycle (median of the timed cycles), the
// node's host phase seconds (hbn_profile) per cycle, and the placement
// statistics.  The device time of k_tick / k_route_fast comes from running it
// under `rocprofv3 --kernel-trace --stats` (the kernels of the timed cycles are
// the bulk of their calls).  Run the two modes alternately on one box.
// Build (one line): g++ -O2 -std=c++17 -o tools/microbench/place_ab tools/microbench/place_ab.cpp
//          -Iinclude -Letcd_amd -lhbnode -lhipbatch -Wl,-rpath,'$ORIGIN/../../etcd_amd'
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hbnode.h"

using clk = std::chrono::steady_clock;
static double ms(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
#define CK(x)                                                                      \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ != 0) {                                                                \
      std::fprintf(stderr, "%s failed: %d (%s)\n", #x, rc_, hbn_last_error());    \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "arrival";
  const uint32_t G = argc > 2 ? (uint32_t)std::atol(argv[2]) : (1u << 20);
  const int cycles = argc > 3 ? std::atoi(argv[3]) : 6;
  hbn_node* mn = nullptr;
  CK(hbn_start(0, 1, G, 3, 256, HB_NO_LIMIT, 4ull * G + 16, &mn));
  std::vector<hbn_storage*> st(G + 1, nullptr);
  std::vector<uint64_t> last(G + 1, 0), lterm(G + 1, 1), adv;
  const uint64_t peers[3] = {1, 2, 3};
  hbn_config cfg{60000, 1, 0};
  for (uint32_t g = 1; g <= G; ++g) {
    CK(hbn_storage_new(&st[g]));
    CK(hbn_create_group(mn, g, &cfg, st[g], peers, 3));
  }
  auto cycle = [&]() -> int {
    const hbn_group_ready* rds = nullptr;
    uint64_t cnt = 0;
    int r = hbn_ready(mn, &rds, &cnt);
    if (r == HBN_EAGAIN) return hbn_advance(mn, nullptr, 0);
    if (r) return r;
    adv.resize(cnt);
    for (uint64_t i = 0; i < cnt; ++i) {
      const hbn_group_ready& rd = rds[i];
      if (rd.fault) return -100;
      if (rd.n_entries) {
        if ((r = hbn_storage_append(st[rd.group], rd.entries, rd.n_entries))) return r;
        last[rd.group] = rd.entries[rd.n_entries - 1].index;
        lterm[rd.group] = rd.entries[rd.n_entries - 1].term;
      }
      adv[i] = rd.group;
    }
    return hbn_advance(mn, adv.data(), cnt);
  };
  CK(cycle());
  hbn_message m;
  std::memset(&m, 0, sizeof(m));
  for (uint32_t g = 2; g <= G; g += 2) {  // even ids: this node wins the election at term 2
    CK(hbn_campaign(mn, g));
    m.type = HB_MSG_VOTE_RESP;
    m.from = 2;
    m.term = 2;
    CK(hbn_step(mn, g, &m));
  }
  for (int k = 0; k < 3; ++k) CK(cycle());
  if (mode == "role") CK(hbn_set_placement(mn, HBN_PLACE_ROLE));
  std::fprintf(stderr, "place_ab: %u groups ready (%s)\n", G, mode.c_str());

  // the mixed cycle's input, in one interleaved arrival stream
  std::vector<uint64_t> bg, pg;
  std::vector<hbn_message> bm;
  std::vector<hbn_entry> ents(G + 1);
  static const uint8_t foo[3] = {'f', 'o', 'o'};
  std::vector<const uint8_t*> pdata;
  std::vector<uint64_t> plen;
  auto build_mixed = [&]() {
    bg.clear();
    bm.clear();
    pg.clear();
    for (uint32_t g = 1; g <= G; ++g) {
      hbn_message x;
      std::memset(&x, 0, sizeof(x));
      x.to = 1;
      x.term = 2;
      if (g % 2 == 0) {
        x.type = HB_MSG_APP_RESP;
        x.index = last[g];
        for (uint64_t f = 2; f <= 3; ++f) {
          x.from = f;
          bg.push_back(g);
          bm.push_back(x);
        }
        pg.push_back(g);
      } else {
        hbn_entry& e = ents[g];
        std::memset(&e, 0, sizeof(e));
        e.term = 2;
        e.index = last[g] + 1;
        e.has_data = 1;
        e.data = foo;
        e.data_len = 3;
        x.type = HB_MSG_APP;
        x.from = 2;
        x.index = last[g];
        x.log_term = lterm[g];
        x.commit = last[g];
        x.entries = &e;
        x.n_entries = 1;
        bg.push_back(g);
        bm.push_back(x);
        x.type = HB_MSG_HEARTBEAT;
        x.index = x.log_term = 0;
        x.entries = nullptr;
        x.n_entries = 0;
        bg.push_back(g);
        bm.push_back(x);
      }
    }
    pdata.assign(pg.size(), foo);
    plen.assign(pg.size(), 3);
  };
  auto median = [](std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  double p0[16] = {}, p1[16] = {}, p1m[16] = {}, p2[16] = {};
  uint32_t np = 0;
  std::vector<double> t_tick, t_mixed;
  for (int k = 0; k < 2; ++k) {  // warm-up: one of each
    CK(hbn_tick(mn));
    CK(cycle());
  }
  hbn_profile(mn, p0, 16, &np);
  for (int k = 0; k < cycles; ++k) {
    auto a = clk::now();
    CK(hbn_tick(mn));
    CK(cycle());
    t_tick.push_back(ms(a, clk::now()));
  }
  hbn_profile(mn, p1, 16, &np);
  for (int k = 0; k < cycles + 1; ++k) {
    build_mixed();
    uint64_t done = 0;
    auto a = clk::now();
    CK(hbn_step_many(mn, bg.size(), bg.data(), bm.data(), &done));
    CK(hbn_propose_many(mn, pg.size(), pg.data(), pdata.data(), plen.data(), &done));
    CK(cycle());
    if (k) t_mixed.push_back(ms(a, clk::now()));
    if (k == 0) hbn_profile(mn, p1m, 16, &np);  // (the first mixed cycle moves the followed groups to term 2: untimed)
  }
  hbn_profile(mn, p2, 16, &np);
  hbn_placement ps;
  CK(hbn_placement_stats(mn, &ps));
  static const char* names[] = {"sync_loads", "reserve", "hb_step", "fetch", "replay", "stepped", "build",
                                "merge", "advance", "bulk_lookup", "bulk_resp", "bulk_prop", "clear"};
  std::printf("{\"mode\": \"%s\", \"groups\": %u, \"cycles\": %d, \"tick_cycle_ms\": %.3f, \"mixed_cycle_ms\": %.3f, "
              "\"led\": %u, \"other\": %u, \"mixed_tiles\": %u, \"moves_total\": %llu, \"repacks\": %llu",
              mode.c_str(), G, cycles, median(t_tick), median(t_mixed), ps.led, ps.other, ps.mixed_tiles,
              (unsigned long long)ps.moves_total, (unsigned long long)ps.repacks);
  std::printf(", \"tick_phase_ms\": {");
  for (uint32_t i = 0; i < np && i < 13; ++i)
    std::printf("%s\"%s\": %.3f", i ? ", " : "", names[i], 1e3 * (p1[i] - p0[i]) / cycles);
  std::printf("}, \"mixed_phase_ms\": {");
  for (uint32_t i = 0; i < np && i < 13; ++i)
    std::printf("%s\"%s\": %.3f", i ? ", " : "", names[i], 1e3 * (p2[i] - p1m[i]) / cycles);
  std::printf("}}\n");
  hbn_stop(mn);
  for (auto* s : st)
    if (s) hbn_storage_free(s);
  return 0;
}
