// AddressSanitizer + UBSan harness for the role-ordered slot map of libhbnode
// (etcd_amd/csrc/hbslots.h; no GPU, no engine): randomised create / remove /
// role-flip sequences against a brute-force model that keeps, per slot, which
// group sits there.  After every re-pack plan the harness applies the move list
// to the model with read-before-write semantics and checks
//   - the list is well formed (distinct live sources, distinct destinations, no
//     live group overwritten without being moved itself),
//   - the layout invariant: led groups dense in [0, nl), the others dense in
//     [nl, nl + no), nothing above, at most one mixed 64-slot tile,
//   - the map's own view (role per slot, counts) equals the model's,
//   - moves <= 2 * (groups whose led / not-led role differs from the previous
//     re-pack + groups removed since), a new group counting as not led.
// Capacities include 1, 2, a full slot space (capacity == live count, so only
// swaps can fix it) and sizes that are no multiple of the tile.
// Built by tests/test_slotmap.py; prints "slots_asan ok" and exits 0 on success.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../etcd_amd/csrc/hbslots.h"

using hbslots::Move;
using hbslots::SlotMap;

static int g_fail = 0;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail = 1;                                                               \
    }                                                                           \
  } while (0)

struct Model {
  uint32_t cap = 0;
  std::vector<int64_t> at;      // slot -> group id, -1 empty
  std::map<int64_t, bool> led;  // live groups -> led
  std::map<int64_t, bool> led_prev;  // as of the previous re-pack (new groups: false)
  uint64_t removed = 0;
  int64_t next_id = 1;
};

static void check_layout(const Model& m, const SlotMap& sm) {
  uint32_t nl = 0, no = 0;
  for (const auto& kv : m.led) (kv.second ? nl : no)++;
  CHECK(sm.led() == nl && sm.other() == no);
  for (uint32_t s = 0; s < m.cap; ++s) {
    const int64_t id = m.at[s];
    if (s < nl) CHECK(id >= 0 && m.led.at(id));
    else if (s < nl + no) CHECK(id >= 0 && !m.led.at(id));
    else CHECK(id < 0);
    const uint8_t want = id < 0 ? hbslots::EMPTY : (m.led.at(id) ? hbslots::LED : hbslots::OTHER);
    CHECK(sm.role(s) == want);
  }
  CHECK(sm.mixed_tiles() <= 1);
  CHECK(sm.top() == nl + no);
}

// the re-pack: plan, validate, apply to the model (read before write), check
static size_t repack(Model& m, SlotMap& sm, bool bounded) {
  std::vector<Move> mv;
  sm.plan(mv);
  std::set<uint32_t> srcs, dsts;
  for (const Move& x : mv) {
    CHECK(x.src < m.cap && x.dst < m.cap && x.src != x.dst);
    CHECK(srcs.insert(x.src).second);
    CHECK(dsts.insert(x.dst).second);
    CHECK(x.src < m.cap && m.at[x.src] >= 0);
  }
  for (uint32_t d : dsts) CHECK(m.at[d] < 0 || srcs.count(d));  // no live group is lost
  std::vector<int64_t> stage;
  for (const Move& x : mv) stage.push_back(m.at[x.src]);
  for (const Move& x : mv) m.at[x.src] = -1;
  for (size_t i = 0; i < mv.size(); ++i) m.at[mv[i].dst] = stage[i];
  std::set<int64_t> seen;
  for (int64_t id : m.at)
    if (id >= 0) CHECK(seen.insert(id).second);
  CHECK(seen.size() == m.led.size());
  check_layout(m, sm);
  if (bounded) {
    uint64_t flips = 0;
    for (const auto& kv : m.led) {
      auto p = m.led_prev.find(kv.first);
      flips += (p == m.led_prev.end() ? false : p->second) != kv.second;
    }
    CHECK(mv.size() <= 2 * (flips + m.removed));
  }
  m.led_prev = m.led;
  m.removed = 0;
  return mv.size();
}

static int64_t pick(const Model& m, std::mt19937& rng) {
  if (m.led.empty()) return -1;
  auto it = m.led.begin();
  std::advance(it, rng() % m.led.size());
  return it->first;
}

static void create(Model& m, SlotMap& sm) {
  const uint32_t s = sm.alloc();
  if (m.led.size() == m.cap) {
    CHECK(s == hbslots::NONE);
    return;
  }
  CHECK(s != hbslots::NONE && s < m.cap && m.at[s] < 0);
  if (s == hbslots::NONE || s >= m.cap) return;
  m.at[s] = m.next_id;
  m.led[m.next_id++] = false;
}
static void remove(Model& m, SlotMap& sm, int64_t id) {
  for (uint32_t s = 0; s < m.cap; ++s)
    if (m.at[s] == id) {
      sm.release(s);
      m.at[s] = -1;
    }
  m.led.erase(id);
  m.led_prev.erase(id);
  ++m.removed;
}
static void flip(Model& m, SlotMap& sm, int64_t id) {
  m.led[id] = !m.led[id];
  for (uint32_t s = 0; s < m.cap; ++s)
    if (m.at[s] == id) sm.set_led(s, m.led[id]);
}

static void run(uint32_t cap, uint32_t rounds, unsigned seed, bool keep_full) {
  std::mt19937 rng(seed);
  Model m;
  m.cap = cap;
  m.at.assign(cap, -1);
  SlotMap sm;
  sm.init(cap);
  if (keep_full)
    for (uint32_t i = 0; i < cap; ++i) create(m, sm);
  uint64_t moves = 0;
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t ops = rng() % 8;
    for (uint32_t k = 0; k < ops; ++k) {
      const uint32_t what = rng() % 10;
      if (keep_full) {  // capacity == live count: flips, and a removal refilled at once
        const int64_t id = pick(m, rng);
        if (what < 8) flip(m, sm, id);
        else {
          remove(m, sm, id);
          create(m, sm);
        }
      } else if (what < 3 || m.led.empty()) {
        create(m, sm);
      } else if (what < 5) {
        remove(m, sm, pick(m, rng));
      } else {
        flip(m, sm, pick(m, rng));
        if (what == 9) flip(m, sm, pick(m, rng));  // (possibly the same one back)
      }
    }
    moves += repack(m, sm, true);
    CHECK(repack(m, sm, true) == 0);  // a second plan finds nothing to do
  }
  if (cap >= 8 && rounds >= 50) CHECK(moves > 0);
}

// adopt() an arrival-order occupancy (holes, interleaved roles), then the usual checks
static void run_adopt(uint32_t cap, unsigned seed) {
  std::mt19937 rng(seed);
  Model m;
  m.cap = cap;
  m.at.assign(cap, -1);
  std::vector<uint8_t> roles(cap, hbslots::EMPTY);
  for (uint32_t s = 0; s < cap; ++s) {
    if (rng() % 5 == 0) continue;
    const bool led = rng() % 2;
    roles[s] = led ? hbslots::LED : hbslots::OTHER;
    m.at[s] = m.next_id;
    m.led[m.next_id++] = led;
  }
  SlotMap sm;
  sm.adopt(roles);
  repack(m, sm, false);  // the first re-pack of an adopted layout may move every group
  for (int r = 0; r < 20; ++r) {
    if (!m.led.empty()) flip(m, sm, pick(m, rng));
    create(m, sm);
    if (!m.led.empty() && r % 3 == 0) remove(m, sm, pick(m, rng));
    repack(m, sm, true);
  }
}

int main() {
  for (unsigned seed = 1; seed <= 6; ++seed) {
    for (uint32_t cap : {1u, 2u, 3u, 7u, 64u, 65u, 130u, 200u}) {
      run(cap, cap <= 7 ? 200 : 120, seed * 7919u + cap, false);
      run(cap, cap <= 7 ? 200 : 120, seed * 104729u + cap, true);
    }
    for (uint32_t cap : {1u, 2u, 63u, 64u, 200u, 257u}) run_adopt(cap, seed * 31u + cap);
  }
  if (g_fail) return 1;
  std::printf("slots_asan ok\n");
  return 0;
}
