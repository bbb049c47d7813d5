// bin_asan.cpp — etcd_amd/csrc/hipbatch_bin.h on the host under
// AddressSanitizer + UBSan (tests/test_egress_bin_ref.py builds and runs it).
//
// Tables of 1, 2, 3, 254 and 255 node ids (the rule below; tests/egress_bin_util.py
// restates it as asan_table, and the GPU test sends the same table and probes
// through hb_egress_bin).  A table's sorted ids and bin bytes are copied into
// heap arrays of exactly n entries, so a lookup that reads one entry past the
// table aborts the run.  Probes: every id of the table, each id - 1 and + 1
// (wrapping), the id with its 32-bit halves swapped, and 0.  Each must give
// the caller's bin number (by a linear search over the caller's list), or n
// for "other".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../etcd_amd/csrc/hipbatch_bin.h"

namespace {

[[noreturn]] void die(const char* what, uint64_t a = 0, uint64_t b = 0) {
  std::fprintf(stderr, "bin_asan: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  std::exit(1);
}

// The caller's list: the edge ids first (1, 2^32, 2^63, 2^64 - 1; pairs that differ only in
// their high or only in their low 32 bits; a pair that is each other's halves swapped), then
// k x 0x9E3779B97F4A7C15 mod 2^64 for k = 1, 2, ...  The first n of them, in this order, which
// is not the sorted order.
std::vector<uint64_t> table(uint32_t n) {
  static const uint64_t edge[] = {1ull,
                                  1ull << 32,
                                  1ull << 63,
                                  ~0ull,
                                  (1ull << 32) | 1ull,
                                  (7ull << 32) | 5ull,
                                  (5ull << 32) | 7ull,
                                  (7ull << 32) | 6ull,
                                  (6ull << 32) | 5ull,
                                  0xFFFFFFFFull,
                                  0xFFFFFFFF00000000ull,
                                  (1ull << 63) | 1ull};
  std::vector<uint64_t> ids;
  for (uint64_t e : edge)
    if (ids.size() < n) ids.push_back(e);
  for (uint64_t k = 1; ids.size() < n; ++k) ids.push_back(k * 0x9E3779B97F4A7C15ull);
  return ids;
}

uint32_t linear(const std::vector<uint64_t>& ids, uint64_t to) {
  for (uint32_t b = 0; b < ids.size(); ++b)
    if (ids[b] == to) return b;
  return (uint32_t)ids.size();
}

uint64_t run_table(uint32_t n) {
  const std::vector<uint64_t> ids = table(n);
  hb::BinTable t;
  if (!hb::bin_build(ids.data(), n, &t)) die("bin_build refused a good table", n);
  for (uint32_t i = 1; i < n; ++i)
    if (t.id[i - 1] >= t.id[i]) die("table not strictly ascending", n, i);
  for (uint32_t i = 0; i < n; ++i)
    if (ids[t.bin[i]] != t.id[i]) die("bin byte does not name its id", n, i);
  const std::vector<uint64_t> sid(t.id, t.id + n);  // exactly n entries each
  const std::vector<uint8_t> sbin(t.bin, t.bin + n);
  uint64_t probes = 0;
  auto probe = [&](uint64_t to) {
    const uint32_t want = linear(ids, to), got = hb::bin_lookup(sid.data(), sbin.data(), n, to);
    if (got != want) die("bin_lookup", to, got);
    const uint32_t info_slot = 4u | (1u << 4), info_other = 4u | (hb::BIN_REF_OTHER << 4) | (1u << 8);
    if (hb::bin_of(sid.data(), sbin.data(), n, info_slot, to) != want) die("bin_of (slot)", to);
    if (hb::bin_of(sid.data(), sbin.data(), n, info_other, to) != n) die("bin_of (HB_REF_OTHER)", to);
    ++probes;
  };
  for (uint64_t id : ids) {
    probe(id);
    probe(id - 1);
    probe(id + 1);
    probe((id << 32) | (id >> 32));
  }
  probe(0);
  return probes;
}

}  // namespace

int main() {
  uint64_t probes = 0;
  for (uint32_t n : {1u, 2u, 3u, 254u, 255u}) probes += run_table(n);
  // what hb_set_egress_peers refuses
  hb::BinTable t;
  std::vector<uint64_t> ids = table(255);
  ids.push_back(12345);
  if (hb::bin_build(ids.data(), 256, &t)) die("256 ids accepted");
  ids = table(9);
  ids[4] = 0;
  if (hb::bin_build(ids.data(), 9, &t)) die("a zero id accepted");
  ids = table(9);
  ids[8] = ids[2];
  if (hb::bin_build(ids.data(), 9, &t)) die("a repeated id accepted");
  if (!hb::bin_build(nullptr, 0, &t)) die("the empty table refused");
  if (hb::bin_lookup(nullptr, nullptr, 0, 7) != 0) die("empty table: not other");
  std::printf("bin ok: %llu probes\n", (unsigned long long)probes);
  return 0;
}
