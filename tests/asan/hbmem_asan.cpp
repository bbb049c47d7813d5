// AddressSanitizer + UBSan harness for the engine's owning buffer type
// (etcd_amd/csrc/hbmem.h; no GPU, no HIP): DevBuf over malloc-backed traits
// that count live blocks and fail the k-th allocation on request.  After every
// reserve the harness writes cap() elements, so an undersized block is ASan's
// to catch; every scenario ends with no live block.
//   - reserve below, at and above the capacity,
//   - the four growth rules of the engine: exact, max(need, 2 cap),
//     need + need / 4, and a fixed size from the first use,
//   - a failed first allocation and a failed regrowth: the buffer is empty and
//     a later reserve succeeds,
//   - release twice, move-construct, move-assign onto a non-empty target,
//   - the hb_set_rand sequence: fresh buffer, copy the prefix, move-assign,
//   - the hook runs once per (re)allocation, never otherwise, and its error
//     leaves the buffer as it was.
// Built by tests/test_hbmem.py; prints "hbmem_asan ok" and exits 0 on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../../etcd_amd/csrc/hbmem.h"

static int g_fail = 0;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail = 1;                                                               \
    }                                                                           \
  } while (0)

struct CountingMem {
  static int live, allocs, fail_at;  // fail_at: the allocation (1-based, from reset()) that fails; 0 none
  static size_t last_bytes;
  static void reset() { allocs = fail_at = 0; }
  static void* alloc(size_t bytes) {
    if (++allocs == fail_at) return nullptr;
    last_bytes = bytes;
    void* p = std::malloc(bytes ? bytes : 1);
    if (p) ++live;
    return p;
  }
  static void free(void* p) {
    --live;
    std::free(p);
  }
};
int CountingMem::live = 0, CountingMem::allocs = 0, CountingMem::fail_at = 0;
size_t CountingMem::last_bytes = 0;
// a second traits type, as the pinned flavour is: same template, other calls
struct OtherMem {
  static int live;
  static void* alloc(size_t bytes) {
    ++live;
    return std::malloc(bytes);
  }
  static void free(void* p) {
    --live;
    std::free(p);
  }
};
int OtherMem::live = 0;

template <class T>
using Buf = hbmem::DevBuf<T, CountingMem>;

template <class B>
static void fill(B& b, int v) {
  if (b.cap()) std::memset(b.get(), v, b.cap() * sizeof(*b.get()));
}
// every scenario starts and ends with no live block
struct Scenario {
  Scenario() {
    CountingMem::reset();
    CHECK(CountingMem::live == 0);
  }
  ~Scenario() { CHECK(CountingMem::live == 0 && OtherMem::live == 0); }
};

static void reserve_around_cap() {
  Scenario sc;
  Buf<uint32_t> b;
  CHECK(!b && b.get() == nullptr && b.cap() == 0);
  CHECK(b.reserve(0) == HB_OK && !b && CountingMem::allocs == 0);  // nothing asked, nothing allocated
  CHECK(b.reserve(100) == HB_OK && b && b.cap() == 100 && CountingMem::last_bytes == 400);
  fill(b, 1);
  uint32_t* p = b.get();
  CHECK(b.reserve(99) == HB_OK && b.get() == p && b.cap() == 100);   // below
  CHECK(b.reserve(100) == HB_OK && b.get() == p && b.cap() == 100);  // at
  CHECK(CountingMem::allocs == 1);
  CHECK(b.reserve(101) == HB_OK && b.cap() == 101 && CountingMem::allocs == 2 && CountingMem::live == 1);  // above
  fill(b, 2);
  CHECK(b.reserve(7) == HB_OK && b.cap() == 101);  // never shrinks
}

static void growth_rules() {
  Scenario sc;
  {  // exact (dec_q, evw, s_edesc, s_eterm, lx_jobs, decf_*)
    Buf<uint64_t> b;
    for (uint64_t need : {16ull, 17ull, 4000ull, 64ull, 4001ull}) {
      const uint64_t before = b.cap();
      CHECK(b.reserve(need) == HB_OK && b.cap() == (need > before ? need : before));
      fill(b, 3);
    }
  }
  {  // max(need, 2 cap) (mv_*, rnd)
    Buf<uint64_t> b;
    const uint64_t needs[] = {10, 11, 15, 21, 1000, 1001}, caps[] = {10, 20, 20, 40, 1000, 2000};
    for (int i = 0; i < 6; ++i) {
      CHECK(b.reserve(needs[i], 2 * b.cap()) == HB_OK && b.cap() == caps[i]);
      fill(b, 4);
    }
  }
  {  // need + need / 4 (evx): only when it has to grow
    Buf<uint8_t> b;
    const uint64_t needs[] = {1000, 1250, 1251, 3}, caps[] = {1250, 1250, 1563, 1563};
    for (int i = 0; i < 4; ++i) {
      CHECK(b.reserve(needs[i], needs[i] + needs[i] / 4) == HB_OK && b.cap() == caps[i]);
      fill(b, 5);
    }
  }
  {  // a fixed size from the first use (hstage, dstage)
    const uint64_t STAGE = 1 << 16;
    Buf<uint8_t> b;
    hbmem::DevBuf<uint8_t, OtherMem> pinned;
    for (uint64_t need : {uint64_t(256), STAGE, uint64_t(512)}) {
      CHECK(b.reserve(need, STAGE) == HB_OK && b.cap() == STAGE);
      CHECK(pinned.reserve(need, STAGE) == HB_OK && pinned.cap() == STAGE);
      fill(b, 6);
      fill(pinned, 6);
    }
    CHECK(CountingMem::live == 1 && OtherMem::live == 1);
  }
}

static void allocation_failures() {
  Scenario sc;
  Buf<uint64_t> b;
  CountingMem::fail_at = 1;  // the first allocation
  CHECK(b.reserve(50) == HB_ENOMEM && !b && b.get() == nullptr && b.cap() == 0 && CountingMem::live == 0);
  CHECK(b.reserve(50) == HB_OK && b.cap() == 50);
  fill(b, 7);
  CountingMem::reset();
  CountingMem::fail_at = 1;  // a regrowth: the old block is gone too
  CHECK(b.reserve(60, 2 * b.cap()) == HB_ENOMEM && !b && b.cap() == 0 && CountingMem::live == 0);
  CHECK(b.reserve(10) == HB_OK && b.cap() == 10 && CountingMem::live == 1);
  fill(b, 8);
  CountingMem::reset();
  CountingMem::fail_at = 1;  // a reserve that needs no block cannot fail
  CHECK(b.reserve(10) == HB_OK && b.cap() == 10 && CountingMem::allocs == 0);
}

static void release_and_moves() {
  Scenario sc;
  Buf<uint32_t> a;
  a.release();  // empty: nothing to free
  CHECK(a.reserve(8) == HB_OK);
  a.release();
  CHECK(!a && a.cap() == 0 && CountingMem::live == 0);
  a.release();  // twice
  CHECK(CountingMem::live == 0);
  CHECK(a.reserve(8) == HB_OK);
  fill(a, 9);
  uint32_t* pa = a.get();
  Buf<uint32_t> b(std::move(a));  // move-construct: the source is empty
  CHECK(!a && a.cap() == 0 && b.get() == pa && b.cap() == 8 && CountingMem::live == 1);
  Buf<uint32_t> c;
  CHECK(c.reserve(32) == HB_OK && CountingMem::live == 2);
  c = std::move(b);  // onto a non-empty target: its block is freed
  CHECK(!b && c.get() == pa && c.cap() == 8 && CountingMem::live == 1);
  fill(c, 10);
  Buf<uint32_t>& self = c;
  c = std::move(self);  // self-assignment keeps the block
  CHECK(c.get() == pa && c.cap() == 8 && CountingMem::live == 1);
  c = Buf<uint32_t>();  // an empty source empties the target
  CHECK(!c && CountingMem::live == 0);
  CHECK(a.reserve(4) == HB_OK && a.cap() == 4);  // a moved-from buffer is an empty one
  fill(a, 11);
}

// hb_set_rand: the table grows and keeps the earlier draws
static bool set_rand(Buf<uint64_t>& rnd, uint64_t& nrnd, uint64_t first, uint64_t count, const uint64_t* draws) {
  const uint64_t need = first + count;
  if (need > rnd.cap()) {
    Buf<uint64_t> fresh;
    if (fresh.reserve(need, 2 * rnd.cap()) != HB_OK) return false;
    if (rnd && first) std::memcpy(fresh.get(), rnd.get(), first * 8);
    rnd = std::move(fresh);
  }
  if (count) std::memcpy(rnd.get() + first, draws, count * 8);
  if (need > nrnd) nrnd = need;
  return true;
}
static void rand_sequence() {
  Scenario sc;
  uint64_t draws[4008];
  for (uint64_t i = 0; i < 4008; ++i) draws[i] = i * 0x9E3779B97F4A7C15ull + 1;
  Buf<uint64_t> rnd;
  uint64_t nrnd = 0;
  CHECK(set_rand(rnd, nrnd, 0, 8, draws) && rnd.cap() == 8);
  CHECK(set_rand(rnd, nrnd, 8, 4000, draws + 8) && rnd.cap() == 4008 && CountingMem::live == 1);
  CHECK(set_rand(rnd, nrnd, 4, 2, draws + 4) && rnd.cap() == 4008);  // rewriting inside: no new block
  CHECK(nrnd == 4008 && std::memcmp(rnd.get(), draws, sizeof(draws)) == 0);
  CHECK(set_rand(rnd, nrnd, 4008, 1, draws) && rnd.cap() == 8016);  // doubles
  CHECK(std::memcmp(rnd.get(), draws, sizeof(draws)) == 0 && rnd.get()[4008] == draws[0]);
  fill(rnd, 12);
  CountingMem::reset();
  CountingMem::fail_at = 1;  // a failed growth keeps the table in force
  uint64_t* p = rnd.get();
  CHECK(!set_rand(rnd, nrnd, 8016, 1, draws) && rnd.get() == p && rnd.cap() == 8016 && CountingMem::live == 1);
}

static void hook_calls() {
  Scenario sc;
  int calls = 0;
  auto idle = [&calls]() -> int {
    ++calls;
    return HB_OK;
  };
  Buf<uint32_t> b;
  CHECK(b.reserve(0, 0, idle) == HB_OK && calls == 0);
  CHECK(b.reserve(16, 0, idle) == HB_OK && calls == 1);  // the first allocation counts
  CHECK(b.reserve(16, 0, idle) == HB_OK && b.reserve(3, 64, idle) == HB_OK && calls == 1);
  CHECK(b.reserve(17, 64, idle) == HB_OK && calls == 2 && b.cap() == 64);
  fill(b, 13);
  CHECK(b.reserve(64, 4096, idle) == HB_OK && calls == 2 && b.cap() == 64);  // grow_to alone never reallocates
  CountingMem::reset();
  CountingMem::fail_at = 1;
  CHECK(b.reserve(65, 0, idle) == HB_ENOMEM && calls == 3 && !b);  // the hook ran before the failed allocation
  CHECK(b.reserve(65, 0, idle) == HB_OK && calls == 4 && b.cap() == 65);
  fill(b, 14);
  // a hook that fails: its code comes back, the block stays, nothing is allocated
  uint32_t* p = b.get();
  CountingMem::reset();
  CHECK(b.reserve(66, 0, [] { return (int)HB_EDEVICE; }) == HB_EDEVICE && b.get() == p && b.cap() == 65);
  CHECK(CountingMem::allocs == 0 && CountingMem::live == 1);
}

int main() {
  reserve_around_cap();
  growth_rules();
  allocation_failures();
  release_and_moves();
  rand_sequence();
  hook_calls();
  if (g_fail || CountingMem::live != 0 || OtherMem::live != 0) return 1;
  std::puts("hbmem_asan ok");
  return 0;
}
