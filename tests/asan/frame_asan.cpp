// frame_asan.cpp — etcd_amd/csrc/hipbatch_frame.h on the host under
// AddressSanitizer + UBSan (tests/test_frame.py builds and runs it).
//
// Without arguments: fr_isize / fr_rows round trips and rejections, the
// validation table (every fstatus by a one-field change of a good frame), the
// directory's edge cases, and the hand frame of tests/test_frame.py built and
// read back in heap buffers of exactly the sizes in use, so a read or write one
// byte past a frame, a column or a table aborts the run.  It prints the hand
// frame as hex ("hand ...") and what unframing it gives ("rows ...").
// With "dir <cap> <id>...": gd_build of the ids in that order, printed as
// "key ..." / "slot ..." / "dups d full f" for the Python Directory to match.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../etcd_amd/csrc/hipbatch_frame.h"

namespace {

using namespace hb;

[[noreturn]] void die(const char* what, uint64_t a = 0, uint64_t b = 0) {
  std::fprintf(stderr, "frame_asan: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  std::exit(1);
}

void sizes() {
  for (uint64_t c = 0; c <= 300; ++c) {
    const uint64_t s = fr_isize(c);
    if (s % 8) die("frame size not a multiple of 8", c, s);
    if (c && s != 48 + 12 * c + 4 * (c & 1)) die("fr_isize", c, s);
    if (fr_rows(s) != c) die("fr_rows(fr_isize(c)) != c", c, fr_rows(s));
  }
  const uint64_t big = 0xFFFFFFFFull;
  if (fr_rows(fr_isize(big)) != big) die("round trip at 2^32 - 1");
  if (fr_rows(fr_isize(big) + 12) != FR_IMPOSSIBLE) die("a length past 2^32 - 1 rows accepted");
  std::vector<bool> made(4096, false);
  for (uint64_t c = 0; fr_isize(c) < 4096; ++c) made[fr_isize(c)] = true;
  uint64_t rejected = 0;
  for (uint64_t l = 0; l < 4096; ++l) {
    if (made[l]) continue;
    if (fr_rows(l) != FR_IMPOSSIBLE) die("a length no count gives was accepted", l, fr_rows(l));
    ++rejected;
  }
  std::printf("sizes ok: %llu lengths rejected\n", (unsigned long long)rejected);
}

// The hand frame of tests/test_frame.py: node 0x1111 to node 0x2222, seq 7,
// three records of 30, 0 and 45 bytes; the second is HB_WIRE_HOST (a hole).
struct Hand {
  std::vector<uint32_t> group{2, 0, 1};
  std::vector<uint64_t> off{100, 130, 130, 175};
  std::vector<uint8_t> status{0, 2, 0};
  std::vector<uint64_t> gid{0xA000000000000001ull, 0xB000000000000002ull, 0xC000000000000003ull};
};

std::vector<uint8_t> hand_frame(uint32_t* fstat) {
  const Hand h;
  std::vector<uint8_t> f(fr_isize(3));  // exactly the frame
  *fstat = fr_build_frame(f.data(), 3, h.group.data(), h.off.data(), h.status.data(), 0, h.gid.data(), 3, 0x1111,
                          0x2222, 7, 75);
  return f;
}

struct Rows {
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, group;
  uint64_t unknown = 0;
  uint32_t st = 0;
};
// frame copied into an exactly sized heap block first
Rows unframe(const std::vector<uint8_t>& frame, uint64_t self, uint64_t from, uint64_t boff, uint64_t blen,
             const std::vector<uint64_t>& key, const std::vector<uint32_t>& slot) {
  const uint64_t c = fr_rows(frame.size());
  if (c == FR_IMPOSSIBLE || c == 0) die("unframe: impossible length", frame.size());
  const std::vector<uint8_t> copy(frame);
  Rows r;
  r.off.assign(c, 99);
  r.len.assign(c, 99);
  r.group.assign(c, 99);
  r.st = fr_unframe_one(copy.data(), c, self, from, boff, blen, key.data(), slot.data(), key.size(), r.off.data(),
                        r.len.data(), r.group.data(), &r.unknown);
  return r;
}

void hand_and_validation() {
  uint32_t fstat = 0;
  const std::vector<uint8_t> f = hand_frame(&fstat);
  if (fstat != 1) die("hand frame: one hole expected", fstat);
  std::printf("hand ");
  for (uint8_t b : f) std::printf("%02x", b);
  std::printf("\n");
  const FrHeader h = fr_parse_header(f.data());
  if (h.magic != FR_MAGIC || h.flags || h.from != 0x1111 || h.to != 0x2222 || h.seq != 7 || h.bytes != 75 ||
      h.count != 3 || h.holes != 1)
    die("header round trip");
  // the receiver holds the third record's group at slot 1 and does not know the first record's
  const Hand hd;
  std::vector<uint64_t> ids{0xD00Dull, hd.gid[1], 0};
  std::vector<uint64_t> key(64);
  std::vector<uint32_t> slot(64);
  uint32_t dups = 9, full = 9;
  gd_build(ids.data(), 3, key.data(), slot.data(), 64, &dups, &full);
  if (dups || full) die("directory of the hand frame");
  const uint64_t boff = (1ull << 33) + 5;
  Rows r = unframe(f, 0x2222, 0x1111, boff, 75, key, slot);
  std::printf("rows %u %llu", r.st, (unsigned long long)r.unknown);
  for (int j = 0; j < 3; ++j)
    std::printf(" %llu:%u:%u", (unsigned long long)r.off[j], r.len[j], r.group[j]);
  std::printf("\n");
  if (r.st != FR_OK || r.unknown != 1) die("hand frame: status / unknown", r.st, r.unknown);
  if (r.off[0] != boff || r.off[1] != boff + 30 || r.off[2] != boff + 30) die("hand frame: offsets");
  if (r.len[0] != 0 || r.group[0] != FR_NO_SLOT) die("unknown gid not dropped");
  if (r.len[1] != 0 || r.group[1] != FR_NO_SLOT) die("hole not dropped");
  if (r.len[2] != 45 || r.group[2] != 1) die("delivered row");

  // every fstatus by a one-field change
  struct Case {
    const char* name;
    uint64_t at;     // byte to change in the frame, or ~0
    uint8_t xorv;
    uint64_t self, from, blen;
    uint32_t want;
  };
  const uint64_t len0 = fr_len_at(3, 0), len1 = fr_len_at(3, 1);
  const Case cases[] = {
      {"good", ~0ull, 0, 0x2222, 0x1111, 75, FR_OK},
      {"magic", 0, 1, 0x2222, 0x1111, 75, FR_BAD_MAGIC},
      {"flags", 4, 1, 0x2222, 0x1111, 75, FR_BAD_MAGIC},
      {"count", 40, 1, 0x2222, 0x1111, 75, FR_BAD_COUNT},
      {"to", 16, 1, 0x2222, 0x1111, 75, FR_BAD_ROUTE},
      {"self", ~0ull, 0, 0x2223, 0x1111, 75, FR_BAD_ROUTE},
      {"from", 8, 1, 0x2222, 0x1111, 75, FR_BAD_ROUTE},
      {"sender", ~0ull, 0, 0x2222, 0x1112, 75, FR_BAD_ROUTE},
      {"bytes field", 32, 1, 0x2222, 0x1111, 75, FR_BAD_LENGTH},
      {"bytes_len + 1", ~0ull, 0, 0x2222, 0x1111, 76, FR_BAD_LENGTH},
      {"sum + 1", len0, 1, 0x2222, 0x1111, 75, FR_BAD_LENGTH},  // 30 -> 31
      {"sum - 1", len0, 3, 0x2222, 0x1111, 75, FR_BAD_LENGTH},  // 30 -> 29
      {"hole length counts", len1, 1, 0x2222, 0x1111, 75, FR_BAD_LENGTH},  // the hole's 0 -> 1
      {"holes field is not checked", 44, 1, 0x2222, 0x1111, 75, FR_OK},
  };
  for (const Case& c : cases) {
    std::vector<uint8_t> g(f);
    if (c.at != ~0ull) g[c.at] ^= c.xorv;
    const Rows q = unframe(g, c.self, c.from, 0, c.blen, key, slot);
    if (q.st != c.want) die(c.name, q.st, c.want);
    if (q.st != FR_OK)
      for (int j = 0; j < 3; ++j)
        if (q.off[j] != 0 || q.len[j] != 0 || q.group[j] != FR_NO_SLOT) die("a bad frame's row survived", j);
  }
  // a hole with bytes: its length moves the rows behind it
  {
    Hand hh;
    hh.status[0] = 0x80 | 20;  // HB_WIRE_SPLICE | prefix_len
    std::vector<uint8_t> g(fr_isize(3));
    const uint32_t st = fr_build_frame(g.data(), 3, hh.group.data(), hh.off.data(), hh.status.data(), 0,
                                       hh.gid.data(), 3, 0x1111, 0x2222, 7, 75);
    if (st != 2) die("a split MsgApp is a hole", st);
    const Rows q = unframe(g, 0x2222, 0x1111, 1000, 75, key, slot);
    if (q.st != FR_OK || q.len[0] != 0 || q.off[1] != 1030 || q.off[2] != 1030 || q.len[2] != 45) die("hole with bytes");
  }
  // group past capacity, gid 0, oversize
  {
    Hand hh;
    hh.group[0] = 3;
    hh.gid[0] = 0;
    hh.status[1] = 0;
    hh.off = {0, 1ull << 31, (1ull << 31) + 1, (1ull << 31) + 2};
    std::vector<uint8_t> g(fr_isize(3));
    const uint32_t st = fr_build_frame(g.data(), 3, hh.group.data(), hh.off.data(), hh.status.data(), 0,
                                       hh.gid.data(), 3, 1, 2, 0, (1ull << 31) + 2);
    if (st != FR_OVERSIZE || fr_parse_header(g.data()).magic != 0) die("oversize bin", st);
    if (fr_get64(g.data() + fr_gid_at(0)) != 0 || !(fr_get32(g.data() + fr_len_at(3, 0)) & FR_HOLE))
      die("group past capacity");
    if (!(fr_get32(g.data() + fr_len_at(3, 1)) & FR_HOLE)) die("gid 0 is a hole");
    if (fr_get32(g.data() + fr_len_at(3, 2)) != 1) die("a plain row");
  }
  std::printf("validation ok: %zu cases\n", sizeof(cases) / sizeof(cases[0]));
}

struct Dir {
  std::vector<uint64_t> key;
  std::vector<uint32_t> slot;
  uint32_t dups = 0, full = 0;
  Dir(const std::vector<uint64_t>& ids, uint64_t cap) : key(cap), slot(cap) {  // exactly cap entries
    gd_build(ids.data(), (uint32_t)ids.size(), key.data(), slot.data(), cap, &dups, &full);
  }
  uint32_t find(uint64_t id) const { return gd_lookup(key.data(), slot.data(), key.size(), id); }
};
// the first `want` ids >= from whose first probe is `bucket`
std::vector<uint64_t> in_bucket(uint64_t cap, uint64_t bucket, uint32_t want, uint64_t from) {
  std::vector<uint64_t> v;
  for (uint64_t id = from; v.size() < want; ++id)
    if ((gd_mix(id) & (cap - 1)) == bucket) v.push_back(id);
  return v;
}

void directory() {
  if (gd_cap_ok(32, 1) || gd_cap_ok(96, 1) || gd_cap_ok(64, 33) || !gd_cap_ok(64, 32) || gd_cap_ok(0, 0) ||
      !gd_cap_ok(1ull << 40, 1u << 31))
    die("gd_cap_ok");
  {  // ids that differ only in bits 32..63
    std::vector<uint64_t> ids;
    for (uint64_t k = 0; k < 32; ++k) ids.push_back((k << 32) | 7);
    ids[0] = 7;
    const Dir d(ids, 64);  // load exactly 0.5
    if (d.dups || d.full) die("high-bit ids: dups");
    for (uint32_t i = 0; i < 32; ++i)
      if (d.find(ids[i]) != i) die("high-bit ids", i);
    if (d.find((32ull << 32) | 7) != FR_NO_SLOT || d.find(8) != FR_NO_SLOT) die("absent id found");
  }
  {  // one bucket, the last one: the run wraps from cap - 1 to 0
    const std::vector<uint64_t> ids = in_bucket(64, 63, 5, 1000);
    const Dir d(ids, 64);
    if (d.key[63] != ids[0] || d.key[0] != ids[1] || d.key[3] != ids[4] || d.key[4] != 0) die("wrapping run");
    for (uint32_t i = 0; i < 5; ++i)
      if (d.find(ids[i]) != i) die("colliding ids", i);
    const std::vector<uint64_t> more = in_bucket(64, 63, 6, 1000);
    if (d.find(more[5]) != FR_NO_SLOT) die("absent id of the same bucket");
  }
  {  // id 0 skipped, a duplicate counted and mapped to its first slot
    const std::vector<uint64_t> ids{5, 0, 9, 5, 0, 9, 11};
    const Dir d(ids, 64);
    if (d.dups != 2 || d.full) die("dups", d.dups);
    if (d.find(5) != 0 || d.find(9) != 2 || d.find(11) != 6) die("duplicate's slot");
    uint32_t used = 0;
    for (uint64_t k : d.key) used += k != 0;
    if (used != 3) die("id 0 was inserted", used);
  }
  {  // a full table (no caller may build one: gd_cap_ok): the lookup ends after cap probes
    std::vector<uint64_t> ids;
    for (uint64_t k = 1; k <= 66; ++k) ids.push_back(k * 0x9E3779B97F4A7C15ull);
    const Dir d(ids, 64);
    if (d.full != 2 || d.dups) die("full table", d.full);
    for (uint32_t i = 0; i < 64; ++i)
      if (d.find(ids[i]) != i) die("full table: present id", i);
    if (d.find(ids[64]) != FR_NO_SLOT || d.find(12345) != FR_NO_SLOT) die("full table: absent id");
  }
  std::printf("directory ok\n");
}

int dir_cmd(int argc, char** argv) {
  const uint64_t cap = std::strtoull(argv[2], nullptr, 0);
  std::vector<uint64_t> ids;
  for (int i = 3; i < argc; ++i) ids.push_back(std::strtoull(argv[i], nullptr, 0));
  const Dir d(ids, cap);
  std::printf("key");
  for (uint64_t k : d.key) std::printf(" %llu", (unsigned long long)k);
  std::printf("\nslot");
  for (uint64_t p = 0; p < cap; ++p) std::printf(" %u", d.key[p] ? d.slot[p] : 0u);
  std::printf("\ndups %u full %u\n", d.dups, d.full);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "dir")) return dir_cmd(argc, argv);
  sizes();
  hand_and_validation();
  directory();
  std::printf("frame ok\n");
  return 0;
}
