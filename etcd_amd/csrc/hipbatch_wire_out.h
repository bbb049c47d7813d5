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
// same bytes, and the place where the host splices the entries.
//
// Plain C++ with no HIP header and no intrinsic: the engine compiles it for
// the device (hb_encode, hipbatch.hip) and tests/asan/wire_out_asan.cpp for the
// host, under the sanitizers.
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

}  // namespace hb
