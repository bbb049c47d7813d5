// hipbatch_frame.h — the index frame of a peer stream and the group-id directory
// (hb_frame / hb_unframe / hb_gid_dir_build).
//
// A peer's byte span (hb_peer_spans) is a run of raftpb.Message records with no
// boundaries and no group ids in it.  The index frame beside it carries both,
// as two columns behind a fixed header, little-endian:
//
//    0 u32 magic "HBF1" |  4 u32 flags 0 |  8 u64 from | 16 u64 to | 24 u64 seq |
//   32 u64 bytes        | 40 u32 count c | 44 u32 holes |
//   48 u64 gid[c]       | 48 + 8c u32 len[c] (bit 31 = hole) | 4 zero bytes when c is odd
//
// so fr_isize(c) = 48 + 12c + 4(c & 1) for c > 0 and 0 for c = 0 (an empty bin
// makes no frame).  fr_isize is injective and fr_rows is its inverse: a receiver
// takes the row count from the frame's length, checks the frame's extent against
// its buffer with it, and only then reads a table word.
//
// The directory maps a 64-bit group id to the receiver's slot: open addressing
// over a power-of-two table, first probe splitmix64(id) & (cap - 1), linear
// probing, key 0 = empty, at most cap probes.  The device builds it with a
// 64-bit compare-and-swap (hipbatch.hip); gd_build here is the host's build and
// gd_lookup the one probe both sides use.
//
// Plain C++ with no HIP header and no intrinsic: the engine compiles it for the
// device and the host, tests/asan/frame_asan.cpp for the host under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FR_HD __host__ __device__
#else
#define FR_HD
#endif

namespace hb {

constexpr uint32_t FR_MAGIC = 0x31464248u;  // "HBF1"
constexpr uint64_t FR_HEADER = 48;
constexpr uint32_t FR_HOLE = 0x80000000u;   // bit 31 of a len word
constexpr uint32_t FR_LEN_MASK = 0x7FFFFFFFu;
constexpr uint64_t FR_IMPOSSIBLE = ~0ull;   // fr_rows: no count gives this length
constexpr uint64_t FR_MAX_ROWS = 0xFFFFFFFFull;  // count is a u32
constexpr uint32_t FR_MAX_FRAMES = 256;     // frames of one hb_unframe
constexpr uint32_t FR_OVERSIZE = 0xFFFFFFFFu;    // fstat of a bin with a record of 2^31 bytes or more
constexpr uint32_t FR_NO_SLOT = 0xFFFFFFFFu;     // absent from the directory; the group of a dropped row
// status of a wire record that is a message for the receiver (HB_WIRE_OK)
constexpr uint8_t FR_WIRE_OK = 0;

// fstatus of hb_unframe (HB_FRAME_*), in the order the checks are made
enum : uint32_t { FR_OK = 0, FR_BAD_MAGIC = 1, FR_BAD_COUNT = 2, FR_BAD_ROUTE = 3, FR_BAD_LENGTH = 4 };

// Bytes of a frame of c rows (c <= FR_MAX_ROWS: at most 12 * 2^32 + 52, no wrap).
FR_HD inline uint64_t fr_isize(uint64_t c) { return c ? FR_HEADER + 12 * c + 4 * (c & 1) : 0; }

// The c with fr_isize(c) == len, or FR_IMPOSSIBLE.  An even c gives 48 + 12c,
// an odd c 52 + 12c: the remainder of (len - 48) by 12 tells which.
FR_HD inline uint64_t fr_rows(uint64_t len) {
  if (len == 0) return 0;
  if (len < FR_HEADER + 16) return FR_IMPOSSIBLE;  // one row is 64 bytes
  const uint64_t body = len - FR_HEADER, r = body % 12;
  uint64_t c;
  if (r == 0) c = body / 12;
  else if (r == 4) c = (body - 4) / 12;
  else return FR_IMPOSSIBLE;
  if (c == 0 || c > FR_MAX_ROWS || ((c & 1) != 0) != (r == 4)) return FR_IMPOSSIBLE;
  return c;
}

// Offsets of the columns inside a frame of c rows.
FR_HD inline uint64_t fr_gid_at(uint64_t j) { return FR_HEADER + 8 * j; }
FR_HD inline uint64_t fr_len_at(uint64_t c, uint64_t j) { return FR_HEADER + 8 * c + 4 * j; }

FR_HD inline void fr_put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}
FR_HD inline void fr_put64(uint8_t* p, uint64_t v) {
  fr_put32(p, (uint32_t)v);
  fr_put32(p + 4, (uint32_t)(v >> 32));
}
FR_HD inline uint32_t fr_get32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
FR_HD inline uint64_t fr_get64(const uint8_t* p) { return (uint64_t)fr_get32(p) | (uint64_t)fr_get32(p + 4) << 32; }

struct FrHeader {
  uint32_t magic, flags;
  uint64_t from, to, seq, bytes;
  uint32_t count, holes;
};

// The 48 header bytes.  An oversize bin's header is written with magic 0.
FR_HD inline void fr_pack_header(uint8_t* p, const FrHeader& h) {
  fr_put32(p, h.magic);
  fr_put32(p + 4, h.flags);
  fr_put64(p + 8, h.from);
  fr_put64(p + 16, h.to);
  fr_put64(p + 24, h.seq);
  fr_put64(p + 32, h.bytes);
  fr_put32(p + 40, h.count);
  fr_put32(p + 44, h.holes);
}
FR_HD inline FrHeader fr_parse_header(const uint8_t* p) {
  FrHeader h;
  h.magic = fr_get32(p);
  h.flags = fr_get32(p + 4);
  h.from = fr_get64(p + 8);
  h.to = fr_get64(p + 16);
  h.seq = fr_get64(p + 24);
  h.bytes = fr_get64(p + 32);
  h.count = fr_get32(p + 40);
  h.holes = fr_get32(p + 44);
  return h;
}

// One row of a sender's frame.  The row's gid is the group's id (0 for a group
// past capacity: `gid_of_group` is then not read by the caller and passed as 0).
// It is a hole when the record is not HB_WIRE_OK (HB_WIRE_HOST with length 0, or
// HB_WIRE_SPLICE | k: a split MsgApp must never be decoded as one without
// entries), when the group lies past capacity or when its id is unset.
struct FrRow {
  uint64_t gid;
  uint32_t len;   // the len word, hole bit included
  bool oversize;  // byte_len >= 2^31: the bin cannot be framed
};
FR_HD inline FrRow fr_row(uint8_t status, bool group_ok, uint64_t gid_of_group, uint64_t byte_len) {
  FrRow r;
  r.gid = group_ok ? gid_of_group : 0;
  r.oversize = byte_len > FR_LEN_MASK;
  const bool hole = status != FR_WIRE_OK || !group_ok || r.gid == 0;
  r.len = ((uint32_t)byte_len & FR_LEN_MASK) | (hole ? FR_HOLE : 0u);
  return r;
}

// The checks of one received frame of `rows` rows (rows > 0; the extent was
// checked before the header was read), `sum` = the 64-bit sum of its rows'
// lengths (a hole's length counts: its bytes lie in the span).
FR_HD inline uint32_t fr_validate(const FrHeader& h, uint64_t rows, uint64_t self_id, uint64_t from,
                                  uint64_t bytes_len, uint64_t sum) {
  if (h.magic != FR_MAGIC || h.flags != 0) return FR_BAD_MAGIC;
  if ((uint64_t)h.count != rows) return FR_BAD_COUNT;
  if (h.to != self_id || h.from != from) return FR_BAD_ROUTE;
  if (h.bytes != bytes_len || sum != bytes_len) return FR_BAD_LENGTH;
  return FR_OK;
}

// ---- the group-id directory ---------------------------------------------------
FR_HD inline uint64_t gd_mix(uint64_t x) {  // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
FR_HD inline bool gd_cap_ok(uint64_t cap, uint64_t count) {
  return cap >= 64 && (cap & (cap - 1)) == 0 && count <= cap / 2;
}
// The slot of `id` (id != 0; cap a power of two), or FR_NO_SLOT: an empty key
// ends the probe run, and so does the cap-th probe of a table without one.
FR_HD inline uint32_t gd_lookup(const uint64_t* key, const uint32_t* slot, uint64_t cap, uint64_t id) {
  const uint64_t mask = cap - 1;
  uint64_t p = gd_mix(id) & mask;
  for (uint64_t k = 0; k < cap; ++k) {
    const uint64_t v = key[p];
    if (v == id) return slot[p];
    if (v == 0) return FR_NO_SLOT;
    p = (p + 1) & mask;
  }
  return FR_NO_SLOT;
}
// Host build: clears key[0, cap), inserts every non-zero gid[i] -> i in order.
// *dups = ids already present when inserted (the first slot stays), *full = ids
// that found no empty key in cap probes (never when gd_cap_ok).  cap must be a
// power of two.
inline void gd_build(const uint64_t* gid, uint32_t count, uint64_t* key, uint32_t* slot, uint64_t cap,
                     uint32_t* dups, uint32_t* full) {
  const uint64_t mask = cap - 1;
  uint32_t nd = 0, nf = 0;
  for (uint64_t p = 0; p < cap; ++p) key[p] = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const uint64_t id = gid[i];
    if (id == 0) continue;
    uint64_t p = gd_mix(id) & mask, k = 0;
    for (; k < cap; ++k) {
      if (key[p] == 0) {
        key[p] = id;
        slot[p] = i;
        break;
      }
      if (key[p] == id) {
        ++nd;
        break;
      }
      p = (p + 1) & mask;
    }
    if (k == cap) ++nf;
  }
  if (dups) *dups = nd;
  if (full) *full = nf;
}

// ---- host reference of both directions (the tests' C core) ----------------------
// One bin's frame into dst[0, fr_isize(c)): rows j = records first + j of a
// binned batch.  Returns the hole count, or FR_OVERSIZE (the header then has
// magic 0).  gid has `capacity` words.
inline uint32_t fr_build_frame(uint8_t* dst, uint64_t c, const uint32_t* group, const uint64_t* off,
                               const uint8_t* status, uint64_t first, const uint64_t* gid, uint32_t capacity,
                               uint64_t from, uint64_t to, uint64_t seq, uint64_t bytes) {
  if (c == 0) return 0;
  uint32_t holes = 0;
  bool over = false;
  for (uint64_t j = 0; j < c; ++j) {
    const uint64_t i = first + j;
    const bool ok = group[i] < capacity;
    const FrRow r = fr_row(status[i], ok, ok ? gid[group[i]] : 0, off[i + 1] - off[i]);
    fr_put64(dst + fr_gid_at(j), r.gid);
    fr_put32(dst + fr_len_at(c, j), r.len);
    holes += (r.len & FR_HOLE) != 0;
    over |= r.oversize;
  }
  if (c & 1) fr_put32(dst + fr_len_at(c, c), 0);
  FrHeader h;
  h.magic = over ? 0 : FR_MAGIC;
  h.flags = 0;
  h.from = from;
  h.to = to;
  h.seq = seq;
  h.bytes = bytes;
  h.count = (uint32_t)c;
  h.holes = holes;
  fr_pack_header(dst, h);
  return over ? FR_OVERSIZE : holes;
}

// One received frame (frame[0, len), fr_rows(len) = rows > 0 checked by the
// caller) into rows of off / len / group; returns its fstatus and adds the rows
// dropped for an absent gid to *n_unknown.
inline uint32_t fr_unframe_one(const uint8_t* frame, uint64_t rows, uint64_t self_id, uint64_t from,
                               uint64_t bytes_off, uint64_t bytes_len, const uint64_t* key, const uint32_t* slot,
                               uint64_t cap, uint64_t* off, uint32_t* len, uint32_t* group, uint64_t* n_unknown) {
  uint64_t sum = 0;
  for (uint64_t j = 0; j < rows; ++j) sum += fr_get32(frame + fr_len_at(rows, j)) & FR_LEN_MASK;
  const uint32_t st = fr_validate(fr_parse_header(frame), rows, self_id, from, bytes_len, sum);
  uint64_t run = 0;
  for (uint64_t j = 0; j < rows; ++j) {
    off[j] = 0;
    len[j] = 0;
    group[j] = FR_NO_SLOT;
    if (st != FR_OK) continue;
    const uint32_t w = fr_get32(frame + fr_len_at(rows, j));
    const uint64_t id = fr_get64(frame + fr_gid_at(j));
    off[j] = bytes_off + run;
    run += w & FR_LEN_MASK;
    if ((w & FR_HOLE) || id == 0) continue;
    const uint32_t s = gd_lookup(key, slot, cap, id);
    if (s == FR_NO_SLOT) {
      ++*n_unknown;
      continue;
    }
    len[j] = w & FR_LEN_MASK;
    group[j] = s;
  }
  return st;
}

}  // namespace hb
