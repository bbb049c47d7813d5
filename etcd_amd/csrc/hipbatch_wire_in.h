// hipbatch_wire_in.h — canonical-shape parser of raftpb.Message records with entries
// (wire ingestion of the follower side, hb_decode_follow).
//
// The shape Message.MarshalTo writes (raft/raftpb/raft.pb.go:1271-1330), entries included:
//
//   08 type | 10 to | 18 from | 20 term | 28 logTerm | 30 index |
//   { 3a len(Entry) Entry }* |
//   40 commit | 4a 08 12 06 0a 00 10 00 18 00 | 50 reject | 58 rejectHint | end
//
// with an Entry as Entry.MarshalTo writes it for the entries a follower's device log takes:
//
//   08 Type (one byte, 00 or 01) | 10 Term | 18 Index | [ 22 len(Data) Data ] | end of its span
//
// and for a forwarded proposal (hb_set_wire_props bit HB_WIRE_PROPS_IN; a MsgProp whose header
// fields 4-6, Commit, Reject and RejectHint are all 0 and which carries at least one entry) as
// Propose makes them:
//
//   08 00 | 10 00 | 18 00 | [ 22 len(Data) Data ] | end of its span
//
// Every varint is at most 10 bytes (bits past 63 drop, as Go's shift does).  Entry k of a
// message carries Index == m.Index + 1 + k (mod 2^64) and at most WI_ENT_MAX_DATA bytes of
// Data.  On this shape Message.Unmarshal makes the same assignments in the same order and no
// Entry returns an error, so the values read here are the reference's; any other record is
// "not canonical" and the caller runs the general decoder (hipbatch_wire.h).
//
// Nothing outside d[0, l) is read.  Plain C++ with no HIP header and no intrinsic: the
// engine compiles it for the device (hipbatch.hip) and tests/asan/wire_in_asan.cpp and
// tests/asan/wire_props_asan.cpp for the host, under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WI_HD __host__ __device__
#define WI_ROLLED _Pragma("nounroll")  // a rolled loop holds one saved exec mask, not one per byte
#else
#define WI_HD
#define WI_ROLLED
#endif

namespace hb {

constexpr uint32_t WI_ENT_MAX_DATA = 0x3FFFFFFF;  // HB_ENT_MAX_DATA
constexpr uint32_t WI_MAX_ENTS = (1u << 23) - 1;  // entries of one canonical message (256 records' counts fit 32 bits)
constexpr uint32_t WI_ENT_MIN = 8;                // wire bytes of the shortest entry: 3a 06 08 T 10 t 18 i

struct WiHeader {
  uint32_t type;  // the low 32 bits of the varint: MessageType is int32
  uint64_t to, from, term, log_term, index;
  uint64_t ents;  // position of the first byte after field 6
};
struct WiTail {
  uint64_t commit, hint;
  bool reject;
};
struct WiEntry {
  uint64_t term;
  uint32_t desc;  // HB_ENT_DESC(len(Data), Type, field 4 present)
  uint64_t data;  // position in the record of the first Data byte, 0 when Data is absent
};

WI_HD inline bool wi_varint(const uint8_t* d, uint64_t l, uint64_t& i, uint64_t& v) {
  v = 0;
  WI_ROLLED
  for (int k = 0; k < 10; ++k) {
    if (i >= l) return false;
    const uint32_t b = d[i++];
    v |= (uint64_t)(b & 0x7F) << (7 * k);  // k = 9: bits past 63 drop
    if (b < 0x80) return true;
  }
  return false;
}

WI_HD inline bool wi_field(const uint8_t* d, uint64_t l, uint64_t& i, uint8_t key, uint64_t& v) {
  if (i >= l || d[i] != key) return false;
  ++i;
  return wi_varint(d, l, i, v);
}

// fields 1-6, once and in order
WI_HD inline bool wi_header(const uint8_t* d, uint64_t l, WiHeader* h) {
  uint64_t i = 0, t;
  if (!wi_field(d, l, i, 0x08, t) || !wi_field(d, l, i, 0x10, h->to) || !wi_field(d, l, i, 0x18, h->from) ||
      !wi_field(d, l, i, 0x20, h->term) || !wi_field(d, l, i, 0x28, h->log_term) ||
      !wi_field(d, l, i, 0x30, h->index))
    return false;
  h->type = (uint32_t)t;
  h->ents = i;
  return true;
}

// One entry of the field-7 run at d[i] (the caller saw 3a there), which must carry `index`;
// i moves past it.
WI_HD inline bool wi_entry(const uint8_t* d, uint64_t l, uint64_t& i, uint64_t index, WiEntry* e) {
  uint64_t span, v;
  if (!wi_field(d, l, i, 0x3a, span)) return false;
  if (span > l - i) return false;
  const uint64_t end = i + span;
  if (end - i < 2 || d[i] != 0x08 || d[i + 1] > 1) return false;
  const uint32_t type = d[i + 1];
  i += 2;
  if (!wi_field(d, end, i, 0x10, e->term)) return false;
  if (!wi_field(d, end, i, 0x18, v) || v != index) return false;
  if (i == end) {
    e->desc = type << 30;
    e->data = 0;
    return true;
  }
  if (!wi_field(d, end, i, 0x22, v)) return false;
  if (v > WI_ENT_MAX_DATA || v != end - i) return false;
  e->desc = (uint32_t)v | (type << 30) | (1u << 31);
  e->data = i;
  i = end;
  return true;
}

// field 8, the empty snapshot, fields 10 and 11, the end of the record
WI_HD inline bool wi_tail(const uint8_t* d, uint64_t l, uint64_t i, WiTail* t) {
  uint64_t r;
  if (!wi_field(d, l, i, 0x40, t->commit)) return false;
  // 4a 08 | 12 06 | 0a 00 | 10 00 | 18 00 : Snapshot{Metadata{ConfState{}, 0, 0}}
  const uint8_t snap[10] = {0x4a, 0x08, 0x12, 0x06, 0x0a, 0x00, 0x10, 0x00, 0x18, 0x00};
  if (l - i < 10) return false;
  bool same = true;
  for (int j = 0; j < 10; ++j) same &= d[i + j] == snap[j];
  if (!same) return false;
  i += 10;
  if (!wi_field(d, l, i, 0x50, r) || !wi_field(d, l, i, 0x58, t->hint)) return false;
  t->reject = r != 0;
  return i == l;
}

// One entry of a forwarded proposal's field-7 run at d[i] (the caller saw 3a there), as
// Propose makes it (pb.Entry{Data: data}, raft/node.go; stepFollower forwards it untouched):
//
//   08 00 | 10 00 | 18 00 | [ 22 len(Data) Data ] | end of its span
//
// Type, Term and Index are the single byte 00 each; e->term = 0.  i moves past it.
WI_HD inline bool wi_prop_entry(const uint8_t* d, uint64_t l, uint64_t& i, WiEntry* e) {
  uint64_t span, v;
  if (!wi_field(d, l, i, 0x3a, span)) return false;
  if (span > l - i) return false;
  const uint64_t end = i + span;
  if (end - i < 6) return false;
  const uint8_t head[6] = {0x08, 0x00, 0x10, 0x00, 0x18, 0x00};
  bool same = true;
  for (int j = 0; j < 6; ++j) same &= d[i + j] == head[j];
  if (!same) return false;
  i += 6;
  e->term = 0;
  if (i == end) {
    e->desc = 0;
    e->data = 0;
    return true;
  }
  if (!wi_field(d, end, i, 0x22, v)) return false;
  if (v > WI_ENT_MAX_DATA || v != end - i) return false;
  e->desc = (uint32_t)v | (1u << 31);
  e->data = i;
  i = end;
  return true;
}

constexpr uint32_t WI_MSG_PROP = 2;  // HB_MSG_PROP (raftpb.MsgProp)

// Whether a record of this header takes the proposal rule (hb_set_wire_props bit HB_WIRE_PROPS_IN).
WI_HD inline bool wi_is_prop(const WiHeader& h, bool props) { return props && h.type == WI_MSG_PROP; }

// The whole record: header, the entry run (counted and checked, *ne entries), tail.  The entry
// rule is the follower's (wi_entry), or with `props` for a record of type MsgProp the forwarded
// proposal's: wi_prop_entry for every entry, at least one of them, and the header r.send writes
// for a MsgProp (Term = LogTerm = Index = Commit = 0, no Reject, RejectHint = 0).
WI_HD inline bool wi_message(const uint8_t* d, uint64_t l, WiHeader* h, WiTail* t, uint32_t* ne, bool props = false) {
  if (!wi_header(d, l, h)) return false;
  const bool prop = wi_is_prop(*h, props);
  if (prop && (h->term | h->log_term | h->index) != 0) return false;
  uint64_t i = h->ents;
  uint32_t n = 0;
  while (i < l && d[i] == 0x3a) {
    WiEntry e;
    if (n == WI_MAX_ENTS) return false;
    if (!(prop ? wi_prop_entry(d, l, i, &e) : wi_entry(d, l, i, h->index + 1 + n, &e))) return false;
    ++n;
  }
  *ne = n;
  if (!wi_tail(d, l, i, t)) return false;
  return !prop || (n != 0 && t->commit == 0 && !t->reject && t->hint == 0);
}

}  // namespace hb
