// hipbatch_bin.h — the node table of hb_egress_bin.
//
// A record of an hb_out_batch goes to the bin of its destination node: the
// caller's position of m.To in the table given to hb_set_egress_peers, or
// "other" (bin n) for an id that is not in it and for a record whose to_ref is
// HB_REF_OTHER.  The table is kept sorted by id with the caller's bin number
// beside each id, so a lookup is a binary search of 8 steps over at most 255
// ids; all 64 bits of an id are compared.
//
// Plain C++ with no HIP header and no intrinsic: the engine compiles it for
// the device (the kernels keep the table in LDS) and for the host
// (hb_set_egress_peers builds the table), tests/asan/bin_asan.cpp for the host
// under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BN_HD __host__ __device__
#else
#define BN_HD
#endif

namespace hb {

constexpr uint32_t BIN_MAX_PEERS = 255;             // HB_EGRESS_MAX_PEERS
constexpr uint32_t BIN_SLOTS = BIN_MAX_PEERS + 1;   // bins of a full table: 255 nodes and "other"
constexpr uint32_t BIN_REF_OTHER = 0xD;             // HB_REF_OTHER

// The table as the device holds it: ids ascending, bin[i] = the caller's bin of id[i].
struct BinTable {
  uint64_t id[BIN_SLOTS];
  uint8_t bin[BIN_SLOTS];
};

// Sorts the caller's n ids into t.  false: n > 255, a zero id or a repeated id
// (t is then unspecified).  Entries at and past n are zeroed.
inline bool bin_build(const uint64_t* ids, uint32_t n, BinTable* t) {
  if (n > BIN_MAX_PEERS) return false;
  for (uint32_t i = 0; i < BIN_SLOTS; ++i) {
    t->id[i] = 0;
    t->bin[i] = 0;
  }
  for (uint32_t b = 0; b < n; ++b) {  // insertion sort: n <= 255, a configuration call
    const uint64_t v = ids[b];
    if (v == 0) return false;
    uint32_t p = b;
    while (p > 0 && t->id[p - 1] > v) {
      t->id[p] = t->id[p - 1];
      t->bin[p] = t->bin[p - 1];
      --p;
    }
    if (p > 0 && t->id[p - 1] == v) return false;
    t->id[p] = v;
    t->bin[p] = (uint8_t)b;
  }
  return true;
}

// The bin of node id `to` in a table of n sorted ids (n <= 255): the number of
// ids below `to` by a branch-light lower bound (steps 128 .. 1 sum to 255, so
// every position 0 .. n is reachable and no id at or past n is read), then one
// full 64-bit compare.  n = "other".
BN_HD inline uint32_t bin_lookup(const uint64_t* id, const uint8_t* bin, uint32_t n, uint64_t to) {
  uint32_t lo = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t step = 128; step >= 1; step >>= 1) {
    const uint32_t m = lo + step;
    if (m <= n && id[m - 1] < to) lo = m;
  }
  return (lo < n && id[lo] == to) ? (uint32_t)bin[lo] : n;
}

// The bin of a record (info = HB_INFO(type, to_ref, reject)).
BN_HD inline uint32_t bin_of(const uint64_t* id, const uint8_t* bin, uint32_t n, uint32_t info, uint64_t to) {
  if (((info >> 4) & 0xF) == BIN_REF_OTHER) return n;
  return bin_lookup(id, bin, n, to);
}

}  // namespace hb
