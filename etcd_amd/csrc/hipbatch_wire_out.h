// hipbatch_wire_out.h — encoder of payload-free raftpb.Message records (wire egress).
//
// Restates Message.MarshalTo (raft/raftpb/raft.pb.go:1271-1330) for a message
// without entries and with the empty (non-nullable) Snapshot: every scalar
// field is written, in field order, as gogo does for required fields; varints
// follow encodeVarintRaft (:1446-1454).
//
//   08 type | 10 to | 18 from | 20 term | 28 logTerm | 30 index | 40 commit |
//   4a 08 12 06 0a 00 10 00 18 00 | 50 reject (00 / 01) | 58 rejectHint
//
// A MsgApp with entries is written in the split form (wo_prefix_len below): the
// same bytes, and the place where the host splices the entries.  hb_encode_ents
// writes such a MsgApp whole: the entry encoder, the coverage rule of its entry
// source and the plan of a payload copy are at the end of this file.
//
// Plain C++ with no HIP header and no intrinsic: the engine compiles it for
// the device (hb_encode, hb_encode_ents, hipbatch.hip) and tests/asan/wire_out_asan.cpp,
// wire_out_app_asan.cpp and wire_out_ents_asan.cpp for the host, under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WO_HD __host__ __device__
#else
#define WO_HD
#endif

namespace hb {

// Snapshot{Metadata{ConfState{}, Index 0, Term 0}} behind its key and length
constexpr uint32_t WO_SNAP_LEN = 10;
// keys: ten single bytes (fields 1-6, 8, 9, 10, 11); varint fields besides the
// type: to, from, term, logTerm, index, commit, rejectHint
constexpr uint32_t WO_KEYS = 10, WO_VARINTS = 7, WO_VARINT_MAX = 10;
// a MessageType (0..11) is one byte; so is the bool
constexpr uint32_t WO_MIN = WO_KEYS + 1 + WO_VARINTS * 1 + (WO_SNAP_LEN - 1) + 1;
constexpr uint32_t WO_MAX = WO_KEYS + 1 + WO_VARINTS * WO_VARINT_MAX + (WO_SNAP_LEN - 1) + 1;
static_assert(WO_MIN == 28 && WO_MAX == 91, "record bounds of a payload-free Message");

// sovRaft
WO_HD inline uint32_t wo_varint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    ++n;
  }
  return n;
}

// encodeVarintRaft; returns the position after the varint
WO_HD inline uint32_t wo_put_varint(uint8_t* dst, uint32_t i, uint64_t v) {
  while (v >= 0x80) {
    dst[i++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  dst[i++] = (uint8_t)v;
  return i;
}

// Message.Size() of the record (type < 128: every MessageType)
WO_HD inline uint32_t wo_size(uint32_t type, uint64_t to, uint64_t from, uint64_t term, uint64_t log_term,
                              uint64_t index, uint64_t commit, bool reject, uint64_t hint) {
  (void)reject;
  return WO_KEYS + (WO_SNAP_LEN - 1) + 1 + wo_varint_len(type) + wo_varint_len(to) + wo_varint_len(from) +
         wo_varint_len(term) + wo_varint_len(log_term) + wo_varint_len(index) + wo_varint_len(commit) +
         wo_varint_len(hint);
}

// The split form, for a MsgApp that carries entries.  MarshalTo writes the
// entries (field 7: 3a, varint(Entry.Size()), Entry, once per entry) as one
// contiguous run between field 6 (Index) and field 8 (Commit), and a MsgApp's
// Reject and RejectHint are 0.  So the record is written as prefix ‖ suffix, the
// bytes of the same message without entries, and the run goes in at the prefix's
// end: wo_prefix_len is fields 1-6, at most 6 keys + the type + 5 varints.
constexpr uint32_t WO_PREFIX_MAX = 6 + 1 + 5 * WO_VARINT_MAX;
static_assert(WO_PREFIX_MAX == 57 && WO_PREFIX_MAX < 0x80, "a prefix length fits the low 7 bits of a status byte");
WO_HD inline uint32_t wo_prefix_len(uint32_t type, uint64_t to, uint64_t from, uint64_t term, uint64_t log_term,
                                    uint64_t index) {
  return 6 + wo_varint_len(type) + wo_varint_len(to) + wo_varint_len(from) + wo_varint_len(term) +
         wo_varint_len(log_term) + wo_varint_len(index);
}

// Message.MarshalTo into dst[0, wo_size(...)); returns the bytes written
WO_HD inline uint32_t wo_write(uint8_t* dst, uint32_t type, uint64_t to, uint64_t from, uint64_t term,
                               uint64_t log_term, uint64_t index, uint64_t commit, bool reject, uint64_t hint) {
  uint32_t i = 0;
  dst[i++] = 0x08;
  i = wo_put_varint(dst, i, type);
  dst[i++] = 0x10;
  i = wo_put_varint(dst, i, to);
  dst[i++] = 0x18;
  i = wo_put_varint(dst, i, from);
  dst[i++] = 0x20;
  i = wo_put_varint(dst, i, term);
  dst[i++] = 0x28;
  i = wo_put_varint(dst, i, log_term);
  dst[i++] = 0x30;
  i = wo_put_varint(dst, i, index);
  dst[i++] = 0x40;
  i = wo_put_varint(dst, i, commit);
  const uint8_t snap[WO_SNAP_LEN] = {0x4a, 0x08, 0x12, 0x06, 0x0a, 0x00, 0x10, 0x00, 0x18, 0x00};
  for (uint32_t j = 0; j < WO_SNAP_LEN; ++j) dst[i++] = snap[j];
  dst[i++] = 0x50;
  dst[i++] = reject ? 1 : 0;
  dst[i++] = 0x58;
  i = wo_put_varint(dst, i, hint);
  return i;
}

// Size and bytes of the split record: those of the entry-free message with Reject = 0 and
// RejectHint = 0, whatever the record's hint column holds (there: the last entry's index).
WO_HD inline uint32_t wo_size_split(uint32_t type, uint64_t to, uint64_t from, uint64_t term, uint64_t log_term,
                                    uint64_t index, uint64_t commit) {
  return wo_size(type, to, from, term, log_term, index, commit, false, 0);
}
WO_HD inline uint32_t wo_write_split(uint8_t* dst, uint32_t type, uint64_t to, uint64_t from, uint64_t term,
                                     uint64_t log_term, uint64_t index, uint64_t commit) {
  return wo_write(dst, type, to, from, term, log_term, index, commit, false, 0);
}
// the split record is a payload-free record: the bounds and hb_encode's LDS window hold
static_assert(WO_PREFIX_MAX + 1 + WO_VARINT_MAX + WO_SNAP_LEN + 2 + 2 <= WO_MAX, "prefix + suffix within WO_MAX");

// ---- a MsgApp written whole: prefix ‖ entries ‖ suffix (hb_encode_ents) ---------------------
// The two halves of wo_write_split on their own: fields 1-6, and fields 8-11 of a MsgApp
// (Commit, the empty snapshot, Reject = 0, RejectHint = 0).  Each returns the bytes written.
WO_HD inline uint32_t wo_write_prefix(uint8_t* dst, uint32_t type, uint64_t to, uint64_t from, uint64_t term,
                                      uint64_t log_term, uint64_t index) {
  uint32_t i = 0;
  dst[i++] = 0x08;
  i = wo_put_varint(dst, i, type);
  dst[i++] = 0x10;
  i = wo_put_varint(dst, i, to);
  dst[i++] = 0x18;
  i = wo_put_varint(dst, i, from);
  dst[i++] = 0x20;
  i = wo_put_varint(dst, i, term);
  dst[i++] = 0x28;
  i = wo_put_varint(dst, i, log_term);
  dst[i++] = 0x30;
  i = wo_put_varint(dst, i, index);
  return i;
}
constexpr uint32_t WO_SUFFIX_MAX = 1 + WO_VARINT_MAX + WO_SNAP_LEN + 2 + 2;
WO_HD inline uint32_t wo_write_suffix(uint8_t* dst, uint64_t commit) {
  uint32_t i = 0;
  dst[i++] = 0x40;
  i = wo_put_varint(dst, i, commit);
  const uint8_t snap[WO_SNAP_LEN] = {0x4a, 0x08, 0x12, 0x06, 0x0a, 0x00, 0x10, 0x00, 0x18, 0x00};
  for (uint32_t j = 0; j < WO_SNAP_LEN; ++j) dst[i++] = snap[j];
  dst[i++] = 0x50;
  dst[i++] = 0;
  dst[i++] = 0x58;
  dst[i++] = 0;
  return i;
}

// An entry descriptor (HB_ENT_DESC of hipbatch.h): len(Data) | Type << 30 | (Data != nil) << 31
constexpr uint32_t WO_ENT_LEN_MASK = 0x3FFFFFFF;
WO_HD inline uint32_t wo_desc_len(uint32_t desc) { return desc & WO_ENT_LEN_MASK; }
WO_HD inline uint32_t wo_desc_type(uint32_t desc) { return (desc >> 30) & 1u; }
WO_HD inline bool wo_desc_has_data(uint32_t desc) { return (desc >> 31) != 0; }

// Entry.Size() (raft/raftpb/raft.pb.go:1030-1043): Type, Term and Index always, Data when not nil
WO_HD inline uint64_t wo_entry_size(uint32_t desc, uint64_t term, uint64_t index) {
  uint64_t n = 3 + wo_varint_len(wo_desc_type(desc)) + wo_varint_len(term) + wo_varint_len(index);
  if (wo_desc_has_data(desc)) n += 1 + wo_varint_len(wo_desc_len(desc)) + (uint64_t)wo_desc_len(desc);
  return n;
}
// Field 7's framing and the entry up to its Data bytes: 3a varint(Entry.Size()) 08 Type 10 Term
// 18 Index [22 varint(len)].  At most 1 + 5 + 2 + 11 + 11 + 6 bytes; returns the bytes written.
constexpr uint32_t WO_ENTRY_HEAD_MAX = 1 + 5 + 2 + 11 + 11 + 6;
WO_HD inline uint32_t wo_entry_head_len(uint32_t desc, uint64_t term, uint64_t index) {
  return 1 + wo_varint_len(wo_entry_size(desc, term, index)) + 3 + wo_varint_len(wo_desc_type(desc)) +
         wo_varint_len(term) + wo_varint_len(index) +
         (wo_desc_has_data(desc) ? 1 + wo_varint_len(wo_desc_len(desc)) : 0);
}
WO_HD inline uint32_t wo_entry_head(uint8_t* dst, uint32_t desc, uint64_t term, uint64_t index) {
  uint32_t i = 0;
  dst[i++] = 0x3a;
  i = wo_put_varint(dst, i, wo_entry_size(desc, term, index));
  dst[i++] = 0x08;
  i = wo_put_varint(dst, i, wo_desc_type(desc));
  dst[i++] = 0x10;
  i = wo_put_varint(dst, i, term);
  dst[i++] = 0x18;
  i = wo_put_varint(dst, i, index);
  if (wo_desc_has_data(desc)) {
    dst[i++] = 0x22;
    i = wo_put_varint(dst, i, wo_desc_len(desc));
  }
  return i;
}

// The coverage rule of hb_encode_ents.  A record of a group carries entries (index, hint]; the
// group's window holds `count` consecutive entries from index `first`, entry first + j at
// position start + j of the per-entry arrays (n_ent elements each).  The record is covered when
//   hint > index, count > 0, index + 1 >= first,
//   (index + 1 - first) + (hint - index) <= count, start + count <= n_ent,
// and every entry with Data has edata + len <= data_len.  No sum is formed that could wrap, and
// no element of a per-entry array is read before the window lies inside [0, n_ent).  On success
// *pos = the position of entry index + 1, *ne = hint - index and *run = the bytes of the field-7
// run (per entry 1 + len(varint(Entry.Size())) + Entry.Size()).
WO_HD inline bool wo_ents_window(uint64_t index, uint64_t hint, uint64_t first, uint32_t count, uint64_t start,
                                 uint64_t n_ent, uint64_t* pos, uint64_t* ne) {
  if (hint <= index || count == 0) return false;  // (index < 2^64 - 1 from here on: index + 1 does not wrap)
  if (index + 1 < first) return false;
  const uint64_t skip = index + 1 - first, want = hint - index;
  if (skip > count || want > count - skip) return false;
  if (start > n_ent || count > n_ent - start) return false;
  *pos = start + skip;
  *ne = want;
  return true;
}
WO_HD inline bool wo_ents_covered(uint64_t index, uint64_t hint, uint64_t first, uint32_t count, uint64_t start,
                                  uint64_t n_ent, const uint64_t* eterm, const uint32_t* edesc, const uint64_t* edata,
                                  uint64_t data_len, uint64_t* pos, uint64_t* ne, uint64_t* run) {
  if (!wo_ents_window(index, hint, first, count, start, n_ent, pos, ne)) return false;
  uint64_t bytes = 0;
  for (uint64_t k = 0; k < *ne; ++k) {
    const uint32_t desc = edesc[*pos + k];
    if (wo_desc_has_data(desc)) {
      const uint64_t at = edata[*pos + k];
      if (at > data_len || wo_desc_len(desc) > data_len - at) return false;
    }
    const uint64_t es = wo_entry_size(desc, eterm[*pos + k], index + 1 + k);
    bytes += 1 + wo_varint_len(es) + es;
  }
  *run = bytes;
  return true;
}

// The chunk plan of a payload copy: dst[0, len) = src[0, len) by `lanes` cooperating lanes.
// head = the bytes before the first destination address that is a multiple of 16, body = whole
// chunks of 16 bytes, tail = the rest.  Head and tail go byte by byte.  A body chunk is one
// aligned 16-byte store; its load is one aligned 16-byte load where source and destination
// share a 16-byte phase, else 16 bytes loaded at the alignment the source does have there:
// width = the largest power of two <= 16 that divides the distance between the two addresses
// (the narrower loads: the compiler may fuse them where the target loads unaligned).  Nothing
// outside [src, src + len) is read and nothing outside [dst, dst + len) is written.
constexpr uint32_t WO_CHUNK = 16;
struct wo_chunk_plan {
  uint32_t width;  // 1, 2, 4, 8 or 16: the source's alignment at a body chunk
  uint64_t head, body, tail;  // head + body * WO_CHUNK + tail == len
};
WO_HD inline wo_chunk_plan wo_plan_copy(uintptr_t src, uintptr_t dst, uint64_t len) {
  wo_chunk_plan p;
  const uintptr_t d = (src - dst) | WO_CHUNK;
  p.width = (uint32_t)(d & (~d + 1));  // lowest set bit
  const uint64_t to_align = (uint64_t)((WO_CHUNK - (dst & (WO_CHUNK - 1))) & (WO_CHUNK - 1));
  p.head = to_align < len ? to_align : len;
  p.body = (len - p.head) / WO_CHUNK;
  p.tail = len - p.head - p.body * WO_CHUNK;
  return p;
}
struct alignas(WO_CHUNK) wo_chunk {
  uint8_t b[WO_CHUNK];
};
// 16 bytes from a source aligned to W
template <uint32_t W>
WO_HD inline wo_chunk wo_load_chunk(const uint8_t* src) {
  wo_chunk c;
  __builtin_memcpy(&c, __builtin_assume_aligned(src, W), WO_CHUNK);
  return c;
}
WO_HD inline void wo_store_chunk(uint8_t* dst, const wo_chunk& c) {
  __builtin_memcpy(__builtin_assume_aligned(dst, WO_CHUNK), &c, WO_CHUNK);
}
// a lane's body chunks: four loads in flight, then their stores
template <uint32_t W>
WO_HD inline void wo_copy_body(const uint8_t* s, uint8_t* d, uint64_t body, uint32_t lane, uint32_t lanes) {
  uint64_t c = lane;
  const uint64_t L = lanes;
  for (; c + 3 * L < body; c += 4 * L) {
    const wo_chunk c0 = wo_load_chunk<W>(s + c * WO_CHUNK), c1 = wo_load_chunk<W>(s + (c + L) * WO_CHUNK),
                   c2 = wo_load_chunk<W>(s + (c + 2 * L) * WO_CHUNK), c3 = wo_load_chunk<W>(s + (c + 3 * L) * WO_CHUNK);
    wo_store_chunk(d + c * WO_CHUNK, c0);
    wo_store_chunk(d + (c + L) * WO_CHUNK, c1);
    wo_store_chunk(d + (c + 2 * L) * WO_CHUNK, c2);
    wo_store_chunk(d + (c + 3 * L) * WO_CHUNK, c3);
  }
  for (; c < body; c += L) wo_store_chunk(d + c * WO_CHUNK, wo_load_chunk<W>(s + c * WO_CHUNK));
}
// lane `lane` of `lanes` does its share of the plan
WO_HD inline void wo_copy_lane(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t lane, uint32_t lanes) {
  const wo_chunk_plan p = wo_plan_copy(reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst), len);
  for (uint64_t x = lane; x < p.head; x += lanes) dst[x] = src[x];
  const uint8_t* s = src + p.head;
  uint8_t* d = dst + p.head;
  switch (p.width) {
    case 16:
      wo_copy_body<16>(s, d, p.body, lane, lanes);
      break;
    case 8:
      wo_copy_body<8>(s, d, p.body, lane, lanes);
      break;
    case 4:
      wo_copy_body<4>(s, d, p.body, lane, lanes);
      break;
    case 2:
      wo_copy_body<2>(s, d, p.body, lane, lanes);
      break;
    default:
      wo_copy_body<1>(s, d, p.body, lane, lanes);
      break;
  }
  const uint64_t t0 = p.head + p.body * WO_CHUNK;
  for (uint64_t x = t0 + lane; x < len; x += lanes) dst[x] = src[x];
}

}  // namespace hb
