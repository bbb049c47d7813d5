// hipbatch.hip — MI355X (gfx950) batched Raft leader-bookkeeping engine.
//
// One hb_step() = three phases on the handle's stream:
//   1. partition  (k_radix_hist, k_scan_rows, k_radix_scatter x passes,
//      k_part_bounds): a stable LSD radix sort of the arrival-ordered batch by
//      partition = group >> PART_LOG, so every partition's segment keeps
//      arrival order.
//   2. apply      (k_apply<NMAX>): one 1024-lane workgroup per partition, one
//      lane per raft group.  The lane loads its group's SoA state into
//      registers once, steps the group's messages in arrival order (LDS
//      counting sort of the staged segment), emits events through a
//      wave-cooperative chunk allocator, and writes back only dirty fields.
//   3. finish     (k_finish): per-workgroup statistics are reduced to one
//      HB_STAT_COUNT vector (RCCL-reducible) and the event count is closed.
//
// The work is integer and HBM-bound; there is no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "hbmem.h"
#include "hipbatch_kernels.h"
#include "hipbatch_fast.h"
#include "hipbatch_elect.h"
#include "hipbatch_lead.h"
#include "hipbatch_wire.h"
#include "hipbatch_wire_in.h"
#include "hipbatch_wire_out.h"
#include "hipbatch_bin.h"
#include "hipbatch_frame.h"

using namespace hb;

#define HB_CHECK(expr)                                                       \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      if (getenv("HB_DEBUG"))                                                \
        fprintf(stderr, "hipbatch: %s failed: %s (%s:%d)\n", #expr,          \
                hipGetErrorString(_e), __FILE__, __LINE__);                  \
      return HB_EDEVICE;                                                     \
    }                                                                        \
  } while (0)

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= (uint32_t)d) v += t;
  }
  return v;
}

// Block-wide exclusive scan (blockDim.x = 1024); returns exclusive prefix, *total = block sum.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh16, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(v);
  if (lane == 63) sh16[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    const uint32_t nw = blockDim.x >> 6;
    uint32_t x = lane < nw ? sh16[lane] : 0;
    x = wave_incl_scan(x);
    if (lane < nw) sh16[lane] = x;
  }
  __syncthreads();
  const uint32_t before = wave == 0 ? 0 : sh16[wave - 1];
  *total = sh16[(blockDim.x >> 6) - 1];
  __syncthreads();
  return before + incl - v;
}

// ============================================================================
// Phase 1: partition the batch into buckets
//
// A bucket is 2^sis_log consecutive apply partitions (sis_log <= 4: up to
// 4096 groups, 7 at n = 3; hb_create picks the smallest that needs no extra pass, down to
// one k_route workgroup per bucket).  The batch is sorted by bucket id with a
// stable LSD radix sort, 8-bit digits: one pass up to 256 buckets, two up to
// 64K.  A 512-lane workgroup ranks a 2048-message tile stably (ballot
// matching inside a wave, per-wave counters across waves), stages it in LDS
// in digit order and writes each digit's run contiguously, so the global
// stores are coalesced runs (~8 records per digit per tile) instead of
// scattered single records.  Messages of groups >= capacity are dropped in
// the first pass.  Arrival order is preserved within every bucket.
//
// The final pass writes the apply input: one 16-byte MsgRec per message
// (info with the group's lane in bits 16-23 and its partition in the bucket
// in bits 24-27 (30-31 and 14 above 16 partitions: rec_sub), arrival index, Term and Index packed into one word, below).
// k_route reads the records and writes the partition once more as a key byte
// per message, contiguous, for the general kernel's bucket walk (a separate
// key array written here took 8-byte runs per digit per tile: partial lines).
//
// The 16-byte record: every pass over the messages (scatter write, route read
// and write, apply read) moves 16 instead of 24 bytes.  Term and Index share
// one u64 (Index in bits 0-39, Term in 40-63) when they fit, which is every
// message a raft cluster sends below 2^24 terms and 2^40 entries; otherwise
// the record is marked REC_LONG and the first pass keeps the full pair in
// the prep set's side table at the message's arrival index, where every
// reader takes it from (rec_unpack).  Bit-exact for every u64 value.
// ============================================================================
struct BatchDev {
  const uint32_t* group;
  const uint32_t* info;
  const uint64_t* term;
  const uint64_t* index;
  const uint64_t* hint;
  const uint32_t* props;
  uint64_t n;
};

// A bucket is 2^sis_log apply partitions (hb_handle::sis_log, chosen at
// hb_create: at most SIS_MAX, fewer when that costs no extra radix pass, so
// that one k_route workgroup owns a whole bucket and reads it once).
constexpr uint32_t SIS_LOG_MAX = 4;
// HB_SIS_LOG_MAX3 > 4: n = 3 handles take buckets of up to 2^7 partitions
// (32K groups) when that saves a radix pass (8M groups: 256 buckets, one pass
// instead of two); k_route_fast's 16 sisters then read their bucket from L2,
// 16 times over.  Measured (cfg5, same box): partition 433 -> 241 us but
// k_route_fast 485 -> 1032 us (0.92 -> 1.27 ms/step): off.
#ifndef HB_SIS_LOG_MAX3
#define HB_SIS_LOG_MAX3 4
#endif
constexpr uint32_t SIS_LOG_MAX3 = HB_SIS_LOG_MAX3;
static_assert(SIS_LOG_MAX3 <= 7, "a record carries its partition in the bucket in 7 bits (rec_sub)");
// a prep set's counters: k_apply's 8 work-list lengths, k_elect's 8, k_follow's, the finish ticket —
// each on a 128-byte line of its own (CTR_STRIDE words): the returning atomics of every partition
// on one line serialise at the memory side (~7 ns each; 16K partitions put 16K on a list)
enum : uint32_t { CTR_STRIDE = 32, CTR_AP = 0, CTR_EL = 8 * CTR_STRIDE, CTR_FL = 16 * CTR_STRIDE,
                  CTR_DONE = 17 * CTR_STRIDE, CTR_STEADY = 18 * CTR_STRIDE, CTR_WORDS = 19 * CTR_STRIDE };
// step statistics: NSH shards per value, each (value, shard) on a 128-byte line of its own
constexpr uint32_t NSH = 8;
constexpr uint64_t STAGE_MAX = 8ull << 20;  // host-pointer batches packed into one pinned copy up to this size  // (a shard per XCD slot; a finish lane per (value, shard))
__host__ __device__ constexpr uint32_t shard_at(uint32_t k, uint32_t sh) { return (k * NSH + sh) * 16; }
constexpr uint32_t RDX_BITS = 8;
constexpr uint32_t RDX_BINS = 1u << RDX_BITS;
#ifndef HB_RDX_THREADS  // measured (cfg2 / cfg5 A/B): 1024 x 2 beat 512 x 4 (-3 us / -46 us per step),
#define HB_RDX_THREADS 1024  // 256 x 4, 512 x 2, 512 x 8 and 1024 x 4
#endif
#ifndef HB_RDX_ROUNDS
#define HB_RDX_ROUNDS 2
#endif
constexpr uint32_t RDX_THREADS = HB_RDX_THREADS;
constexpr uint32_t RDX_WAVES = RDX_THREADS / 64;
constexpr uint32_t RDX_ROUNDS = HB_RDX_ROUNDS;
constexpr uint32_t RDX_TILE = RDX_THREADS * RDX_ROUNDS;  // 2048

struct MsgRec {      // apply input record (16 B)
  uint32_t info;     // type | from << 4 | reject << 8 | voted << 9 | lane << 16 | sub (rec_sub_bits) | long << 28
  uint32_t orig;     // arrival index in the batch
  uint64_t ti;       // Index | Term << 40 (REC_LONG: side[2 orig], side[2 orig + 1])
};
static_assert(sizeof(MsgRec) == 16, "one dwordx4 per record");
constexpr uint32_t REC_LONG = 1u << 28;
// Follower-side batches (hb_batch.commit present, "X mode"): every record also
// carries a 16-byte extension {hint (m.LogTerm / RejectHint), m.Commit} through
// the partition and the route (recx / slotx), and a MsgApp's info says how
// many entries it carries (bits 10-15) and REC_UNI when there are at most
// REC_UNI_MAX and every one has the message's Term — what the follower fast
// lane needs, with no gather by arrival index.
constexpr uint32_t REC_UNI = 1u << 29;
constexpr uint32_t REC_UNI_MAX = 8;
constexpr uint32_t REC_NE_SHIFT = 10;
__device__ __forceinline__ uint32_t rec_ne(uint32_t info) { return (info >> REC_NE_SHIFT) & 0xFu; }
// A final record's partition in its bucket (sub < 2^sis_log, at most 7 bits):
// bits 0-3 at 24-27, bits 4-5 at 30-31, bit 6 at 14 (the entry count above
// uses bits 10-13 only: REC_UNI_MAX = 8)
__device__ __forceinline__ uint32_t rec_sub_bits(uint32_t sub) {
  return ((sub & 0xFu) << 24) | (((sub >> 4) & 3u) << 30) | (((sub >> 6) & 1u) << 14);
}
__device__ __forceinline__ uint32_t rec_sub(uint32_t info) {
  return ((info >> 24) & 0xFu) | (((info >> 30) & 3u) << 4) | (((info >> 14) & 1u) << 6);
}
// the bits of a batch info word a record keeps (lane / partition bits are added by the final pass)
constexpr uint32_t REC_KEEP = 0x3FFFu | REC_LONG | REC_UNI;
constexpr uint32_t REC_IDX_BITS = 40;
constexpr uint64_t REC_IDX_MASK = (1ull << REC_IDX_BITS) - 1;
// pack (term, index) into ti; false: does not fit (REC_LONG)
__device__ __forceinline__ bool rec_pack(uint64_t term, uint64_t index, uint64_t* ti) {
  *ti = index | (term << REC_IDX_BITS);
  return index <= REC_IDX_MASK && term < (1ull << (64 - REC_IDX_BITS));
}
// a record's Term and Index (a long record's from the side table)
__device__ __forceinline__ void rec_unpack(uint32_t info, uint32_t orig, uint64_t ti, const uint64_t* side,
                                           uint64_t* term, uint64_t* index) {
  if (info & REC_LONG) {
    *term = side[2 * (size_t)orig];
    *index = side[2 * (size_t)orig + 1];
  } else {
    *term = ti >> REC_IDX_BITS;
    *index = ti & REC_IDX_MASK;
  }
}
// a route slot (lane-major [k][G], one dwordx4): info, arrival index, ti
__device__ __forceinline__ void slot_unpack(const uint4 r, const uint64_t* side, uint32_t* info, uint32_t* orig,
                                            uint64_t* term, uint64_t* index) {
  *info = r.x;
  *orig = r.y;
  rec_unpack(r.x, r.y, (uint64_t)r.z | ((uint64_t)r.w << 32), side, term, index);
}

struct RadixSrc {
  const uint32_t* group;
  const uint32_t* info;   // the batch's fields (first pass) ...
  const uint64_t* term;
  const uint64_t* index;
  const MsgRec* rec;      // ... or an intermediate pass's records (info without lane bits, arrival index)
  const uint32_t* n_dev;  // null: n
  uint64_t* side;         // first pass: the long records' (term, index) by arrival index
  uint32_t n;
  // X mode (hb_batch.commit present): the batch's hint / commit / entry arrays
  // (first pass) or the intermediate pass's extensions
  const uint64_t* hint;
  const uint64_t* mcommit;
  const uint64_t* eoff;
  const uint64_t* eterm;
  uint64_t n_ent;
  const uint4* recx;
};

// Intermediate pass output: the group ids (what the next pass's histogram
// reads) plus one 16-byte record per message, so that a digit's run of a tile
// is one contiguous store instead of several runs of 32-64 bytes (the SoA
// layout wrote 1.6x its bytes as partial lines on cfg4).
struct RadixDst {
  uint32_t* group;
  MsgRec* rec;
  uint4* recx;  // X mode
};

struct FinalDst {  // final pass output = apply input
  MsgRec* rec;
  uint4* recx;       // X mode: {hint, commit} beside each record
  uint32_t* bucket;  // bucket id per message (multi-pass only, for k_bucket_bounds)
  uint32_t* bk_off;  // [NBK + 1] written by the one-pass scatter
  uint32_t NBK;
  uint32_t sis_log;  // partitions per bucket (log2)
};

__device__ __forceinline__ uint32_t src_n(const RadixSrc& s) { return s.n_dev ? *s.n_dev : s.n; }
// shift = the bucket's log2 size + the pass's digit offset
// dbits = the pass's digit width (<= RDX_BITS; the first of two passes takes half the bits)
__device__ __forceinline__ uint32_t rdx_digit(uint32_t g, uint32_t shift, uint32_t dbits) {
  return (g >> shift) & ((1u << dbits) - 1u);
}

// Exclusive scan over the first 256 threads of the block (all threads call it).
__device__ __forceinline__ uint32_t excl_scan256(uint32_t v, uint32_t* sh4, uint32_t* total) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t incl = wave_incl_scan(v);
  if (tid < 256 && lane == 63) sh4[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) before += (w < wave) ? sh4[w] : 0u;
  *total = sh4[0] + sh4[1] + sh4[2] + sh4[3];
  __syncthreads();
  return before + incl - v;
}

// Per-tile digit counts, HIST_TPB tiles per workgroup: every group id of the
// workgroup's tiles is loaded at once (more loads in flight per lane than one
// 2048-message tile gives), then counted tile by tile in LDS.
#ifndef HB_HIST_TPB
#define HB_HIST_TPB 4
#endif
constexpr uint32_t HIST_TPB = HB_HIST_TPB;
// One-pass partitions take each tile's digit offsets without a scan launch:
// k_radix_hist also writes each workgroup's digit sums
// (DirectSums::agg) and adds them into its superblock's (SB_HW workgroups,
// agent-scope atomics), and the scatter sums the superblocks, aggregates and
// tiles before its own (k_radix_scatter_d).  The superblock sums rotate over
// three buffers: a step's hist clears the one the next step adds into (read
// by the scatter two steps ago), as far as that one was dirtied.
constexpr uint32_t SB_HW = 32;
constexpr uint32_t SUP_BUFS = 3;
struct DirectSums {
  uint32_t* agg = nullptr;    // [hist workgroups][RDX_BINS]; null: k_scan_rows scans the counts
  uint32_t* sup = nullptr;    // [superblocks][RDX_BINS] of this step (zero on entry)
  uint32_t* clear = nullptr;  // the next step's superblock buffer: n_clear words to zero
  uint32_t n_clear = 0;
  uint32_t* bk_fill = nullptr;  // (k_scan_rows' clears)
  uint32_t NBK = 0;
  uint32_t* ctr = nullptr;
};
__global__ void __launch_bounds__(RDX_THREADS) k_radix_hist(RadixSrc s, uint32_t G, uint32_t shift, uint32_t dbits,
                                                           uint32_t ntiles, uint32_t* hist, uint32_t dm,
                                                           DirectSums ds) {
  __shared__ uint32_t cnt[HIST_TPB][RDX_BINS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < HIST_TPB * RDX_BINS; i += RDX_THREADS) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const uint32_t n = src_n(s);
  const uint32_t t0 = blockIdx.x * HIST_TPB;
  uint32_t gv[HIST_TPB][RDX_ROUNDS];
#pragma unroll
  for (uint32_t t = 0; t < HIST_TPB; ++t)
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
      const uint32_t i = (t0 + t) * RDX_TILE + r * RDX_THREADS + tid;
      gv[t][r] = i < n ? s.group[i] : 0xFFFFFFFFu;
    }
#pragma unroll
  for (uint32_t t = 0; t < HIST_TPB; ++t)
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r)
      if (gv[t][r] < G) atomicAdd(&cnt[t][rdx_digit(gv[t][r], shift, dbits)], 1u);
  __syncthreads();
  for (uint32_t i = tid; i < (HIST_TPB << dbits); i += RDX_THREADS) {  // the pass's digits only
    if (dm) {  // [digit][tile]
      const uint32_t t = i % HIST_TPB, dg = i / HIST_TPB;
      if (t0 + t < ntiles) hist[(size_t)dg * ntiles + (t0 + t)] = cnt[t][dg];
    } else {  // [tile][digit]
      const uint32_t t = i >> dbits, dg = i & ((1u << dbits) - 1);
      if (t0 + t < ntiles) hist[((size_t)(t0 + t) << dbits) + dg] = cnt[t][dg];
    }
  }
  if (ds.agg) {  // uniform (one pass: dbits = RDX_BITS)
    if (tid < RDX_BINS) {
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t t = 0; t < HIST_TPB; ++t) sum += cnt[t][tid];
      ds.agg[(size_t)blockIdx.x * RDX_BINS + tid] = sum;
      if (sum)
        __hip_atomic_fetch_add(&ds.sup[(size_t)(blockIdx.x / SB_HW) * RDX_BINS + tid], sum, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t gi = blockIdx.x * RDX_THREADS + tid, gs = gridDim.x * RDX_THREADS;
    for (uint32_t i = gi; i < ds.n_clear; i += gs) ds.clear[i] = 0;
    for (uint32_t i = gi; i < ds.NBK; i += gs) ds.bk_fill[i * CTR_STRIDE] = 0;
    if (blockIdx.x == 0)
      for (uint32_t i = tid; i < CTR_WORDS; i += RDX_THREADS) ds.ctr[i] = 0;
  }
}

// Digit scan: workgroup d turns digit d's counts of every tile into exclusive
// per-tile prefixes and writes their total to totals[d].  Two-pass handles keep
// the counts digit-major ([nb][ntiles], dm: a streaming read per workgroup;
// tile-major rows made each workgroup read one word per row: cfg4 1.793 ->
// 1.765 ms, cfg5 0.982 -> 0.968 ms); a one-pass handle keeps them tile-major
// ([ntiles][nb]: the scatter reads its tile's row in one line; digit-major
// measured cfg2 +2 us), with the digits of one 128-byte line of every row
// scanned by workgroups of one XCD.  It also clears the per-bucket event-chunk
// cursors for the coming apply.
#ifndef HB_SCAN_PER
#define HB_SCAN_PER 16
#endif
constexpr uint32_t SCAN_PER = HB_SCAN_PER;
__global__ void __launch_bounds__(1024) k_scan_rows(uint32_t* hist, uint32_t ntiles, uint32_t dbits, uint32_t* totals,
                                                    uint32_t* bk_fill, uint32_t NBK, uint32_t* ctr, uint32_t dm) {
  __shared__ uint32_t sh16[16];
  const uint32_t nb = 1u << dbits;
  const uint32_t d = dm ? blockIdx.x : (nb >= 8 ? (blockIdx.x & 7) * (nb / 8) + (blockIdx.x >> 3) : blockIdx.x);
  uint32_t* col = dm ? hist + (size_t)d * ntiles : hist + d;
  const uint32_t CS = dm ? 0u : dbits;  // element i of the digit's counts at col[i << CS]
  for (uint32_t i = blockIdx.x * 1024 + threadIdx.x; i < NBK; i += gridDim.x * 1024) bk_fill[i * CTR_STRIDE] = 0;
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < CTR_WORDS; i += blockDim.x) ctr[i] = 0;
  // SCAN_PER consecutive tiles per lane, all loads of a chunk in flight at once
  uint32_t carry = 0;
  for (uint32_t base = 0; base < ntiles; base += 1024 * SCAN_PER) {
    const uint32_t i0 = base + threadIdx.x * SCAN_PER;
    uint32_t v[SCAN_PER], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; ++k) {
      v[k] = i0 + k < ntiles ? col[(size_t)(i0 + k) << CS] : 0u;
      sum += v[k];
    }
    uint32_t tot;
    uint32_t run = carry + block_excl_scan(sum, sh16, &tot);
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; ++k) {
      if (i0 + k < ntiles) col[(size_t)(i0 + k) << CS] = run;
      run += v[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) totals[d] = carry;
}

// Tile loads of k_radix_scatter (coalesced: round r, lane l -> element wave*256 + r*64 + l).
template <bool X>
struct ScatTile {
  uint32_t g[RDX_ROUNDS], i[RDX_ROUNDS], o[RDX_ROUNDS];
  uint64_t t[RDX_ROUNDS];  // packed ti
  bool v[RDX_ROUNDS];
};
template <bool X>
__device__ __forceinline__ void scat_load(const RadixSrc& s, uint32_t n, uint32_t G, uint32_t base, uint32_t wave,
                                          uint32_t lane, ScatTile<X>& T) {
#pragma unroll
  for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
    const uint32_t i = base + wave * (64 * RDX_ROUNDS) + r * 64 + lane;
    bool v = i < n;
    T.g[r] = v ? s.group[i] : 0u;
    v = v && T.g[r] < G;
    T.v[r] = v;
    if (s.rec) {
      MsgRec m{};
      if (v) m = s.rec[i];
      T.i[r] = m.info;
      T.o[r] = m.orig;
      T.t[r] = m.ti;
    } else {  // the batch: pack Term and Index (a long pair goes to the side table)
      const uint32_t inf = v ? s.info[i] : 0u;
      const uint64_t tm = v ? s.term[i] : 0ull, ix = v ? s.index[i] : 0ull;
      uint64_t ti;
      const bool fits = rec_pack(tm, ix, &ti);
      if (v && !fits) {
        s.side[2 * (size_t)i] = tm;
        s.side[2 * (size_t)i + 1] = ix;
      }
      uint32_t ie = (inf & 0x3FFu) | (fits ? 0u : REC_LONG);
      if constexpr (X) {
        // a MsgApp's entries: how many, and whether all carry m.Term (the
        // batch's entry arrays are in arrival order: near-contiguous per wave)
        if (v && (inf & 0xFu) == HB_MSG_APP && s.eoff && s.eterm) {
          const uint64_t e0 = s.eoff[i], e1 = i + 1 < n ? s.eoff[i + 1] : s.n_ent;
          const uint64_t ne = e1 - e0;
          bool uni = ne <= REC_UNI_MAX;
#pragma unroll
          for (uint32_t k = 0; k < REC_UNI_MAX; ++k)  // (bounded: the round loop stays unrolled)
            if (uni && k < ne) uni = s.eterm[e0 + k] == tm;
          if (uni) ie |= REC_UNI | ((uint32_t)ne << REC_NE_SHIFT);
        }
      }
      T.i[r] = ie;
      T.o[r] = v ? i : 0u;
      T.t[r] = ti;
    }
  }
}

// One workgroup scatters SCAT_TPW consecutive tiles; the next tile's loads
// are issued before the current tile is ranked, staged and written, so they
// are in flight during its LDS phases and stores.
#ifndef HB_SCAT_TPW
#define HB_SCAT_TPW 2
#endif
constexpr uint32_t SCAT_TPW = HB_SCAT_TPW;
// The scatter of TPW consecutive tiles from tile0 (`first`: the workgroup that
// writes n_valid and the one-pass bucket bounds); `off` / `totals` may be LDS.
// off[dg * ds + tile * ts]: a tile's exclusive prefix of digit dg.
// `pre` runs right after the first tile's loads are issued (k_radix_scatter_d
// sums its offsets there); off's tile index counts from tbase.
struct NoPre {
  __device__ void operator()() const {}
};
template <bool FINAL, bool X, uint32_t TPW, class Pre = NoPre>
__device__ __forceinline__ void scatter_tiles(const RadixSrc& s, const RadixDst& d, const FinalDst& f, uint32_t G,
                                              uint32_t shift, uint32_t dbits, uint32_t ntiles, uint32_t tile0,
                                              const uint32_t* off, uint32_t ds, uint32_t ts, const uint32_t* totals,
                                              uint32_t* n_valid, bool first, const Pre& pre = Pre{},
                                              uint32_t tbase = 0) {
  __shared__ uint32_t s_base[RDX_BINS];  // digit base in the pass output (exclusive scan of the totals)
  __shared__ uint32_t s_off[RDX_BINS];
  __shared__ uint32_t s_wcnt[RDX_WAVES][RDX_BINS];
  __shared__ uint32_t s_dstart[RDX_BINS + 1];
  __shared__ uint32_t sh4[4];
  // the tile staged in digit order: group / info / arrival (3 x 4 B) and ti (8 B)
  // per message; X mode then stages the extensions {hint, commit} (16 B) in the
  // same 40 KB once the records are written (two workgroups still fit a CU)
  __shared__ uint64_t st_buf[RDX_TILE * 5 / 2];
  uint32_t* const st_group = reinterpret_cast<uint32_t*>(st_buf);
  uint32_t* const st_info = st_group + RDX_TILE;
  uint32_t* const st_orig = st_info + RDX_TILE;
  uint64_t* const st_ti = st_buf + 3 * RDX_TILE / 2;
  uint4* const st_x = reinterpret_cast<uint4*>(st_buf);
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t nb = 1u << dbits;  // the pass's digits (totals / off rows hold nb)
  const uint32_t n = src_n(s);
  ScatTile<X> cur, nxt;
  scat_load(s, n, G, tile0 * RDX_TILE, wave, lane, cur);
  pre();
  {
    const uint32_t t = tid < nb ? totals[tid] : 0u;
    uint32_t all;
    const uint32_t excl = excl_scan256(t, sh4, &all);
    if (tid < RDX_BINS) s_base[tid] = excl;
    if (first) {
      if (FINAL && f.bk_off && tid <= f.NBK && tid < RDX_BINS) f.bk_off[tid] = excl;
      if (tid == 0) {
        *n_valid = all;
        if (FINAL && f.bk_off && f.NBK == RDX_BINS) f.bk_off[RDX_BINS] = all;
      }
    }
  }
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (uint32_t j = 0; j < TPW; ++j) {
    const uint32_t tile = tile0 + j;
    if (tile >= ntiles) break;  // uniform
    // this tile's digit starts in the output; per-wave digit counters cleared
    if (tid < nb) s_off[tid] = s_base[tid] + off[(size_t)tid * ds + (size_t)(tile - tbase) * ts];
#pragma unroll
    for (uint32_t k = 0; k < RDX_WAVES * RDX_BINS / RDX_THREADS; ++k) (&s_wcnt[0][0])[tid + k * RDX_THREADS] = 0;
    __syncthreads();
    uint32_t vd[RDX_ROUNDS], vr[RDX_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) vd[r] = rdx_digit(cur.g[r], shift, dbits);
    // the next tile's loads go out now
    if (j + 1 < TPW && tile + 1 < ntiles) scat_load(s, n, G, (tile + 1) * RDX_TILE, wave, lane, nxt);
    // stable rank inside the wave: rounds in order, lanes in order
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
      uint64_t peers = __ballot(cur.v[r]);
#pragma unroll
      for (uint32_t k = 0; k < RDX_BITS; ++k) {
        if (k >= dbits) break;
        const bool bit = (vd[r] >> k) & 1u;
        const uint64_t bk = __ballot(bit);
        peers &= bit ? bk : ~bk;
      }
      const uint32_t rank = (uint32_t)__popcll(peers & lt);
      const uint32_t before = cur.v[r] ? s_wcnt[wave][vd[r]] : 0u;
      vr[r] = before + rank;
      if (cur.v[r] && rank == 0) s_wcnt[wave][vd[r]] = before + (uint32_t)__popcll(peers);
    }
    __syncthreads();
    // per digit: prefix over waves, then digit starts inside the tile
    uint32_t run = 0;
    if (tid < RDX_BINS) {
#pragma unroll
      for (uint32_t w = 0; w < RDX_WAVES; ++w) {
        const uint32_t c = s_wcnt[w][tid];
        s_wcnt[w][tid] = run;
        run += c;
      }
    }
    {
      uint32_t all;
      const uint32_t excl = excl_scan256(tid < RDX_BINS ? run : 0u, sh4, &all);
      if (tid < RDX_BINS) s_dstart[tid] = excl;
      if (tid == 0) s_dstart[RDX_BINS] = all;
    }
    __syncthreads();
    uint32_t sp[RDX_ROUNDS];  // staging position of this thread's messages
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
      sp[r] = s_dstart[vd[r]] + s_wcnt[wave][vd[r]] + vr[r];
      if (cur.v[r]) {
        const uint32_t p = sp[r];
        st_group[p] = cur.g[r];
        st_info[p] = cur.i[r];
        st_orig[p] = cur.o[r];
        st_ti[p] = cur.t[r];
      }
    }
    // X mode: the extensions {m.LogTerm / RejectHint, m.Commit} are read now,
    // not with the tile (16 more VGPRs per tile in flight left one workgroup
    // per CU), and cross the records' output phase in flight
    uint4 xv[X ? RDX_ROUNDS : 1];
    if constexpr (X) {
#pragma unroll
      for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
        const uint32_t i = tile * RDX_TILE + wave * (64 * RDX_ROUNDS) + r * 64 + lane;
        xv[r] = make_uint4(0, 0, 0, 0);
        if (cur.v[r]) {
          if (s.rec) {
            xv[r] = s.recx[i];
          } else {
            const uint64_t h = s.hint ? s.hint[i] : 0ull, c = s.mcommit[i];
            xv[r] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)c, (uint32_t)(c >> 32));
          }
        }
      }
    }
    __syncthreads();
    const uint32_t valid = s_dstart[RDX_BINS];
    uint32_t wo[RDX_ROUNDS];  // output position of staging position r * RDX_THREADS + tid
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
      const uint32_t p = r * RDX_THREADS + tid;
      if (p < valid) {
        const uint32_t g = st_group[p];
        const uint32_t dg = rdx_digit(g, shift, dbits);
        const uint32_t o = s_off[dg] + (p - s_dstart[dg]);
        wo[r] = o;
        if (FINAL) {
          MsgRec m;
          m.info = (st_info[p] & REC_KEEP) | ((g & (PART - 1)) << 16) |
                   rec_sub_bits((g >> PART_LOG) & ((1u << f.sis_log) - 1));
          m.orig = st_orig[p];
          m.ti = st_ti[p];
          f.rec[o] = m;
          if (f.bucket) f.bucket[o] = g >> (PART_LOG + f.sis_log);
        } else {
          d.group[o] = g;
          MsgRec m;
          m.info = st_info[p];
          m.orig = st_orig[p];
          m.ti = st_ti[p];
          d.rec[o] = m;
        }
      }
    }
    if constexpr (X) {  // the extensions, through the same staging
      __syncthreads();
#pragma unroll
      for (uint32_t r = 0; r < RDX_ROUNDS; ++r)
        if (cur.v[r]) st_x[sp[r]] = xv[r];
      __syncthreads();
#pragma unroll
      for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
        const uint32_t p = r * RDX_THREADS + tid;
        if (p < valid) (FINAL ? f.recx : d.recx)[wo[r]] = st_x[p];
      }
    }
    __syncthreads();  // the next tile reuses s_off / s_wcnt / s_dstart / the staging
    cur = nxt;
  }
}
template <bool FINAL, bool X>
__global__ void __launch_bounds__(RDX_THREADS) __attribute__((amdgpu_waves_per_eu(8))) k_radix_scatter(RadixSrc s, RadixDst d, FinalDst f, uint32_t G,
                                                              uint32_t shift, uint32_t dbits, uint32_t ntiles, const uint32_t* off,
                                                              uint32_t ds, uint32_t ts, const uint32_t* totals, uint32_t* n_valid) {
  scatter_tiles<FINAL, X, SCAT_TPW>(s, d, f, G, shift, dbits, ntiles, blockIdx.x * SCAT_TPW, off, ds, ts, totals, n_valid,
                                    blockIdx.x == 0);
}

// One pass with direct offsets: each tile's exclusive digit
// prefix = the superblocks before its own + the hist workgroups before its own
// in the superblock + the tiles before it in its hist workgroup; the digit
// totals = every superblock.  Four lanes per digit split those loads, all
// issued at once, while the first tile's loads are in flight.
constexpr uint32_t DQ = RDX_THREADS / RDX_BINS;  // lanes per digit
#ifndef HB_DIRECT_PER
#define HB_DIRECT_PER 16  // items per lane in one round trip (more: further round trips)
#endif
constexpr uint32_t DIRECT_PER = HB_DIRECT_PER;
static_assert(DQ * RDX_BINS == RDX_THREADS && SCAT_TPW <= HIST_TPB && HIST_TPB % SCAT_TPW == 0,
              "a scatter workgroup's tiles sit in one hist workgroup");
struct DirectPre {
  const uint32_t* hist;  // raw tile counts [tile][RDX_BINS]
  const uint32_t* agg;
  const uint32_t* sup;
  uint32_t ntiles, tile0;
  uint32_t* l_pre;  // [DQ][RDX_BINS]
  uint32_t* l_tsum;  // [DQ][RDX_BINS]
  uint32_t* l_off;  // [SCAT_TPW][RDX_BINS]: exclusive prefixes of the workgroup's tiles
  uint32_t* l_tot;  // [RDX_BINS]
  __device__ __forceinline__ const uint32_t* item(uint32_t i, uint32_t nsb, uint32_t na, uint32_t sb,
                                                  uint32_t hb) const {
    return i < nsb ? sup + (size_t)i * RDX_BINS
                   : i < nsb + na ? agg + (size_t)(sb * SB_HW + (i - nsb)) * RDX_BINS
                                  : hist + (size_t)(hb * HIST_TPB + (i - nsb - na)) * RDX_BINS;
  }
  __device__ void operator()() const {
    const uint32_t tid = threadIdx.x, dg = tid % RDX_BINS, q = tid / RDX_BINS;
    const uint32_t hb = tile0 / HIST_TPB, sb = hb / SB_HW;
    const uint32_t nhw = (ntiles + HIST_TPB - 1) / HIST_TPB, nsb = (nhw + SB_HW - 1) / SB_HW;
    const uint32_t na = hb - sb * SB_HW, nt = tile0 - hb * HIST_TPB, ni = nsb + na + nt;
    // the workgroup's own tiles but its last: their counts (lanes of quarter 0)
    uint32_t own[SCAT_TPW > 1 ? SCAT_TPW - 1 : 1];
#pragma unroll
    for (uint32_t j = 0; j + 1 < SCAT_TPW; ++j)
      own[j] = (q == 0 && tile0 + j < ntiles) ? hist[(size_t)(tile0 + j) * RDX_BINS + dg] : 0u;
    uint32_t pre = 0, tot = 0;
    for (uint32_t i0 = 0; i0 < ni; i0 += DQ * DIRECT_PER) {  // (one turn up to 16 superblocks: 8M messages)
      uint32_t v[DIRECT_PER];
#pragma unroll
      for (uint32_t k = 0; k < DIRECT_PER; ++k) {
        const uint32_t i = i0 + k * DQ + q;
        v[k] = i < ni ? item(i, nsb, na, sb, hb)[dg] : 0u;
      }
#pragma unroll
      for (uint32_t k = 0; k < DIRECT_PER; ++k) {
        const uint32_t i = i0 + k * DQ + q;
        if (i < nsb) {
          tot += v[k];
          if (i < sb) pre += v[k];
        } else {
          pre += v[k];
        }
      }
    }
    l_pre[q * RDX_BINS + dg] = pre;
    l_tsum[q * RDX_BINS + dg] = tot;
    __syncthreads();
    if (q == 0) {
      uint32_t p = 0, t = 0;
#pragma unroll
      for (uint32_t k = 0; k < DQ; ++k) {
        p += l_pre[k * RDX_BINS + dg];
        t += l_tsum[k * RDX_BINS + dg];
      }
      l_tot[dg] = t;
#pragma unroll
      for (uint32_t j = 0; j < SCAT_TPW; ++j) {
        l_off[j * RDX_BINS + dg] = p;
        if (j + 1 < SCAT_TPW) p += own[j];
      }
    }
    __syncthreads();
  }
};
template <bool X>
__global__ void __launch_bounds__(RDX_THREADS) __attribute__((amdgpu_waves_per_eu(8))) k_radix_scatter_d(
    RadixSrc s, FinalDst f, uint32_t G, uint32_t shift, uint32_t ntiles, const uint32_t* hist, const uint32_t* agg,
    const uint32_t* sup, uint32_t* n_valid) {
  __shared__ uint32_t l_pre[DQ * RDX_BINS], l_tsum[DQ * RDX_BINS];
  __shared__ uint32_t l_off[SCAT_TPW * RDX_BINS], l_tot[RDX_BINS];
  const uint32_t tile0 = blockIdx.x * SCAT_TPW;
  const DirectPre pre{hist, agg, sup, ntiles, tile0, l_pre, l_tsum, l_off, l_tot};
  scatter_tiles<true, X, SCAT_TPW>(s, RadixDst{}, f, G, shift, RDX_BITS, ntiles, tile0, l_off, 1u, RDX_BINS, l_tot,
                                   n_valid, blockIdx.x == 0, pre, tile0);
}

// One bucket (a node of at most 4,096 groups): the partition is the identity
// on the kept messages, so the final records are the batch's in arrival order
// minus the messages beyond capacity — a stable compaction (ballot prefixes
// per wave, one block scan per tile), no ranking or staging.  Same output as
// k_radix_small / the tiled kernels.
template <bool X>
__global__ void __launch_bounds__(RDX_THREADS) k_pack_one(RadixSrc s, FinalDst f, uint32_t G, uint32_t ntiles,
                                                         uint32_t* bk_fill, uint32_t NBK, uint32_t* ctr,
                                                         uint32_t* n_valid) {
  __shared__ uint32_t s_w[RDX_WAVES];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (uint32_t i = tid; i < NBK; i += RDX_THREADS) bk_fill[i * CTR_STRIDE] = 0;  // (k_scan_rows' clears)
  for (uint32_t i = tid; i < CTR_WORDS; i += RDX_THREADS) ctr[i] = 0;
  const uint32_t n = src_n(s);
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  uint32_t base = 0;
  ScatTile<X> cur, nxt;
  scat_load(s, n, G, 0, wave, lane, cur);
  for (uint32_t tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) scat_load(s, n, G, (tile + 1) * RDX_TILE, wave, lane, nxt);
    // element wave * 64 R + r * 64 + lane: prefixes in (wave, r, lane) order = arrival order
    uint32_t rank[RDX_ROUNDS], wc = 0;
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
      const uint64_t b = __ballot(cur.v[r]);
      rank[r] = wc + (uint32_t)__popcll(b & lt);
      wc += (uint32_t)__popcll(b);
    }
    if (lane == 0) s_w[wave] = wc;
    __syncthreads();
    uint32_t before = base, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < RDX_WAVES; ++w) {
      const uint32_t c = s_w[w];
      before += w < wave ? c : 0u;
      all += c;
    }
    __syncthreads();  // (s_w is rewritten by the next tile)
#pragma unroll
    for (uint32_t r = 0; r < RDX_ROUNDS; ++r) {
      if (!cur.v[r]) continue;
      const uint32_t o = before + rank[r], g = cur.g[r];
      MsgRec m;
      m.info = (cur.i[r] & REC_KEEP) | ((g & (PART - 1)) << 16) | rec_sub_bits((g >> PART_LOG) & ((1u << f.sis_log) - 1));
      m.orig = cur.o[r];
      m.ti = cur.t[r];
      f.rec[o] = m;
      if constexpr (X) {
        const uint32_t i = cur.o[r];
        const uint64_t h = s.hint ? s.hint[i] : 0ull, c = s.mcommit[i];
        f.recx[o] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)c, (uint32_t)(c >> 32));
      }
    }
    base += all;
    cur = nxt;
  }
  if (tid == 0) {
    *n_valid = base;
    if (f.bk_off) {
      f.bk_off[0] = 0;
      f.bk_off[1] = base;
    }
  }
}

// A small one-pass batch (at most SMALL_TILES tiles: a MultiNode node's Ready
// cycle over a few thousand groups) in ONE workgroup: the tile histograms and
// their column scan in LDS, then the same scatter — k_radix_hist +
// k_scan_rows + k_radix_scatter in one launch, the same output.
constexpr uint32_t SMALL_TILES = 8;
template <bool X>
__global__ void __launch_bounds__(RDX_THREADS) k_radix_small(RadixSrc s, FinalDst f, uint32_t G, uint32_t shift,
                                                            uint32_t ntiles, uint32_t* bk_fill, uint32_t NBK,
                                                            uint32_t* ctr, uint32_t* n_valid) {
  __shared__ uint32_t s_hist[SMALL_TILES * RDX_BINS];  // [tile][digit]: counts, then exclusive prefixes
  __shared__ uint32_t s_tot[RDX_BINS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < SMALL_TILES * RDX_BINS; i += RDX_THREADS) s_hist[i] = 0;
  for (uint32_t i = tid; i < NBK; i += RDX_THREADS) bk_fill[i * CTR_STRIDE] = 0;  // (k_scan_rows' clears)
  for (uint32_t i = tid; i < CTR_WORDS; i += RDX_THREADS) ctr[i] = 0;
  __syncthreads();
  const uint32_t n = src_n(s);
  for (uint32_t i = tid; i < n; i += RDX_THREADS) {
    const uint32_t g = s.group[i];
    if (g < G) atomicAdd(&s_hist[(i / RDX_TILE) * RDX_BINS + rdx_digit(g, shift, RDX_BITS)], 1u);
  }
  __syncthreads();
  if (tid < RDX_BINS) {
    uint32_t run = 0;
    for (uint32_t t = 0; t < ntiles; ++t) {
      const uint32_t c = s_hist[t * RDX_BINS + tid];
      s_hist[t * RDX_BINS + tid] = run;
      run += c;
    }
    s_tot[tid] = run;
  }
  __syncthreads();
  scatter_tiles<true, X, SMALL_TILES>(s, RadixDst{}, f, G, shift, RDX_BITS, ntiles, 0, s_hist, 1u, RDX_BINS, s_tot,
                                      n_valid, true);
}

// bk_off[b] = first position of bucket b in the sorted batch (b <= NBK); the
// multi-pass case (the one-pass scatter writes bk_off itself).
__global__ void k_bucket_bounds(const uint32_t* bucket, const uint32_t* n_dev, uint32_t NBK, uint32_t* bk_off) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > NBK) return;
  uint32_t lo = 0, hi = *n_dev;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (bucket[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  bk_off[b] = lo;
}

// ============================================================================
// Phase 2: apply
// ============================================================================
#include "hipbatch_follow.h"  // (reads the record layout above)
struct ApplyArgs {
  DevState S;
  const MsgRec* rec;        // sorted batch: bucket order, arrival order inside a bucket
  uint8_t* key;             // partition-in-bucket of each record (k_route writes it for the walk)
  const uint32_t* bk_off;   // [NBK+1] bucket bounds in rec
  uint32_t* bk_fill;        // [NBK x CTR_STRIDE] event records reserved by the bucket's partitions (a line each)
  const uint64_t* hint;     // original-order RejectHint
  const uint32_t* props;    // dense proposals or null
  uint64_t* ev;             // event region base (compact words, hipbatch_kernels.h)
  uint32_t ev_per_msg;      // bound on event words per stepped message
  uint32_t props_on;        // 1 if props[] is present (one proposal slot per group)
  uint32_t NB;              // partitions
  uint32_t NBK;             // buckets
  uint32_t* ev_counts;      // [NB] records in each chunk
  uint64_t* ev_off;         // [NB] chunk offsets (records)
  uint64_t* stats_shard;    // step statistics, NSH shards per value (shard_at; atomic adds)
  uint32_t* pflag;          // [NB][PART/32] groups handed from k_apply_fast to k_apply
  uint32_t* ap_cnt;         // [8] k_apply's work lists: partitions k_apply_fast flagged, one list per
  uint32_t* ap_list;        // [8][NB]  XCD slot (blockIdx % 8) of the flagging workgroup
  uint32_t* fl_cnt;         // k_follow's work list: partitions with groups k_apply handed on
  uint32_t* fl_list;        // [NB]
  uint32_t* eflag;          // [NB][PART/32] (n >= 5) handed-over groups k_elect should try: not a
  uint32_t* el_cnt;         // [8]   leader, or a leader with a higher-term message in its slots;
  uint32_t* el_list;        // [8][NB]  k_elect's work lists (per XCD slot, as ap_list)
  uint32_t grid;            // apply_grid: virtual workgroups of the partition mapping (part_of)
  uint32_t sis_log;         // partitions per bucket (log2)
  uint32_t* done;           // k_apply workgroups finished (the last one runs the finish)
  uint64_t* stats;          // [HB_STAT_COUNT] this step's statistics (finish)
  uint64_t* accum;          // caller accumulator or null (finish)
  uint32_t* resume;         // [G] messages consumed by k_apply_fast | not loaded << 30 | prop pending << 31
  uint64_t* commit0;        // [G] committed at batch start (for HB_STAT_COMMITS)
  // k_route -> k_apply_fast / k_apply: each group's first kmax messages, lane-major
  uint32_t kmax;            // slots per group (= route_kmax(nmax))
  uint8_t* cnt;             // [G] messages of the group in this batch (saturated at 255)
  uint4* slot;              // [kmax][G] MsgRec {info, arrival index, ti} (slot_unpack)
  const uint64_t* side;     // [2 n] (term, index) of the REC_LONG records, by arrival index
  // X mode (follower-side batches): the records' extensions {hint, commit}
  const uint4* recx;        // beside rec (k_route input)
  uint4* slotx;             // [kmax][G] beside slot (null: no X mode this step)
  // storm hand-over (n >= 5): k_route closes a partition none of whose groups
  // k_apply_lead would load (handover_class), as k_apply_lead would (flags,
  // lists, event chunks), runs k_elect's lane over it, and k_apply_lead skips it
  uint32_t nmax;            // the handle's replica bound (5 or 7)
  uint32_t storm;           // 2: this step's route closes such partitions (lskip), 0: it does not
  uint8_t* lskip;           // [NB] 1: the route closed the partition
  // the n = 3 fast lane's wave-uniform steady path (SteadyLane, hipbatch_fast.h)
  uint32_t steady;          // 1: a wave of steady / idle lanes takes it (HB_FAST_STEADY=0 at hb_create: never)
  uint32_t* steady_cnt;     // tests (HB_FAST_STEADY_COUNT=1): group-waves that took it this step; else null
};

// Message slots k_route keeps per group: n - 1 (one MsgAppResp per follower,
// what k_apply_fast consumes), plus HB_KS_EXTRA for n >= 5 so that k_apply
// reads a handed-over group's messages from its slots (an election: MsgHup +
// n - 1 MsgVoteResp + a step-down) instead of walking the bucket.
#ifndef HB_KS_EXTRA
#define HB_KS_EXTRA 2
#endif
// n = 5 keeps 8 slots (4 acks + up to 4 heartbeat responses of a cfg3 step fit,
// so the general kernel's bucket walk is almost never needed)
#ifndef HB_KS5
#define HB_KS5 8
#endif
// n = 3 keeps up to 3: a leader's two MsgAppResp plus the MsgProp a MultiNode
// application proposes in the same Ready cycle stay on the fast lane when the
// batch says it carries MsgProp messages (HB_STEP_MSG_PROPS); otherwise 2 —
// the third slot costs cfg2 4 % (route at one workgroup per CU, one more slot
// per lane: 118.4-120.0 vs 123.5-124.6 us in two same-box pairs)
constexpr uint32_t route_kmax(int nmax) {
  return nmax <= 3 ? 3u : (nmax <= 5 ? (uint32_t)HB_KS5 : (uint32_t)(nmax - 1 + HB_KS_EXTRA));
}
// the slots a step uses (route_kmax is the most any step uses: the allocation)
inline uint32_t step_kmax(uint32_t nmax, uint32_t flags) {
  return nmax <= 3 ? ((flags & HB_STEP_MSG_PROPS) ? 3u : 2u) : route_kmax((int)nmax);
}
static_assert(route_kmax(3) <= 8 && route_kmax(5) <= 8 && route_kmax(7) <= 8,
              "the slot sorts carry slot numbers as 4-bit nibbles of one uint32_t");

// stats slots reduced per workgroup
enum { ST_MSGS, ST_APPRESP, ST_VOTERESP, ST_DROPPED, ST_COMMITS, ST_WON, ST_LOST, ST_FAULTS, ST_ENTRIES, ST_N };

#ifndef HB_FAST_WAVES
#define HB_FAST_WAVES 4
#endif
constexpr uint32_t FLAG_WORDS = PART / 32;  // per-partition bitmask of groups handed to k_apply
// Set (or clear) lane `lane`'s bit of a partition flag mask.  `lane & 63` must
// be the hardware lane and `lane >> 6` the wave's slot in the partition, so a
// wave owns words 2w and 2w + 1.  The wave ballots the predicate and its
// lowest active lane issues at most two LDS atomics, instead of one per
// flagged lane all landing on the same word (32-way serialised; per-lane
// atomics measured 0.4533 vs 0.4516 ms on cfg3).
template <bool SET>
__device__ __forceinline__ void flag_put(uint32_t* words, uint32_t lane, bool on) {
  const uint64_t act = __ballot(1);
  const uint64_t b = __ballot(on);
  if (b && (lane & 63) == (uint32_t)__ffsll((long long)act) - 1) {
    const uint32_t w = (lane >> 6) * 2, lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
    if (lo) SET ? atomicOr(&words[w], lo) : atomicAnd(&words[w], ~lo);
    if (hi) SET ? atomicOr(&words[w + 1], hi) : atomicAnd(&words[w + 1], ~hi);
  }
}
constexpr uint32_t KPL = 64;                // bucket key bytes scanned per lane per segment
constexpr uint32_t SEG = PART * KPL;        // positions per key-scan segment

// blockIdx -> partition.  The sister partitions of a bucket get block ids
// with equal blockIdx % 8, i.e. one XCD under the round-robin placement, so
// the bucket's keys and records are fetched into one L2 (speed only).
__device__ __forceinline__ uint32_t part_of(uint32_t x, uint32_t sl) {
  const uint32_t r = x & 7, q = x >> 3;
  return ((((q >> sl) << 3) | r) << sl) | (q & ((1u << sl) - 1));
}
__device__ __forceinline__ uint32_t block_part(uint32_t sl) { return part_of(blockIdx.x, sl); }

// LDS staging of one round (<= CH messages) of a partition's messages.
// w[j][i] = word j of the round's i-th MsgRec (info, orig, term lo/hi, index lo/hi).
// (Gathering the records by LDS-DMA, global_load_lds_dword x6, measured slower
// than register staging: 6 requests per record instead of 2-3.)
template <uint32_t CH>
struct Stage {
  static constexpr uint32_t CHUNK = CH;
  uint32_t rbuf[CH];      // bucket-relative positions, increasing (= arrival order)
  uint32_t w[6][CH];
  uint16_t perm[CH];
  uint32_t cnt[PART];
  uint32_t sh16[16];
  uint64_t bcast;
  __device__ __forceinline__ uint32_t info(uint32_t i) const { return w[0][i]; }
  __device__ __forceinline__ uint32_t orig(uint32_t i) const { return w[1][i]; }
  __device__ __forceinline__ uint64_t term(uint32_t i) const { return (uint64_t)w[2][i] | ((uint64_t)w[3][i] << 32); }
  __device__ __forceinline__ uint64_t index(uint32_t i) const { return (uint64_t)w[4][i] | ((uint64_t)w[5][i] << 32); }
};

// This lane's KPL key bytes of segment `seg` (positions seg + tid*KPL + k).
// load_keys only issues the loads, so the caller can overlap them with other
// work; eval_keys returns bit k set where the key equals `sub` and the
// position is in [lo, hi).  Four keys per dword: a SWAR zero-byte test, then
// the four byte flags are gathered into a nibble by one multiply.
struct Keys {
  uint4 q[KPL / 16];
  uint32_t base;
};
__device__ __forceinline__ Keys load_keys(const uint8_t* key, uint32_t seg, uint32_t lo, uint32_t hi) {
  Keys k;
  k.base = seg + threadIdx.x * KPL;
  const uint4* p = reinterpret_cast<const uint4*>(key + k.base);
#pragma unroll
  for (int q = 0; q < (int)(KPL / 16); ++q) k.q[q] = (k.base < hi && k.base + KPL > lo) ? p[q] : make_uint4(0, 0, 0, 0);
  return k;
}
__device__ __forceinline__ uint64_t eval_keys(const Keys& k, uint32_t lo, uint32_t hi, uint32_t sub) {
  const uint32_t base = k.base;
  if (base >= hi || base + KPL <= lo) return 0;
  const uint32_t rep = sub * 0x01010101u;
  uint64_t eq = 0;
#pragma unroll
  for (int q = 0; q < (int)(KPL / 16); ++q) {
    const uint32_t w[4] = {k.q[q].x, k.q[q].y, k.q[q].z, k.q[q].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t x = w[j] ^ rep;
      const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where byte == sub
      const uint32_t c = (((z >> 7) * 0x01020408u) >> 24) & 0xFu;                 // bytes 0..3 -> bits 0..3
      eq |= (uint64_t)c << (16 * q + 4 * j);
    }
  }
  const uint32_t a = lo > base ? lo - base : 0u;                // < KPL
  const uint32_t b = hi - base < KPL ? hi - base : KPL;          // > a
  const uint64_t vm = (b >= 64 ? ~0ull : ((1ull << b) - 1)) & (~0ull << a);
  return eq & vm;
}
__device__ __forceinline__ uint64_t scan_keys(const uint8_t* key, uint32_t seg, uint32_t lo, uint32_t hi,
                                              uint32_t sub) {
  return eval_keys(load_keys(key, seg, lo, hi), lo, hi, sub);
}

// Walk the partition's messages of bucket [lo, hi) in arrival order, in
// rounds of at most CHUNK.  on_total(total) runs once (all threads) before
// the first round with the partition's message count; round(fill) runs per
// round with sl.rbuf[0, fill) = the round's bucket-relative positions.
// `first`: the keys of segment 0, already loaded by the caller (or null).
template <class St, class OnTotal, class Round>
__device__ __forceinline__ void walk_partition(St& sl, const ApplyArgs& a, uint32_t lo, uint32_t hi, uint32_t sub,
                                               const Keys* first, OnTotal&& on_total, Round&& round) {
  constexpr uint32_t CHUNK = St::CHUNK;
  const uint32_t tid = threadIdx.x;
  const uint32_t seg0 = lo & ~15u;
  const uint32_t nseg = hi > lo ? (hi - seg0 + SEG - 1) / SEG : 0u;  // uniform
  if (nseg != 1) {
    uint32_t total = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
      uint32_t t;
      (void)block_excl_scan((uint32_t)__popcll(scan_keys(a.key, seg0 + s * SEG, lo, hi, sub)), sl.sh16, &t);
      total += t;
    }
    on_total(total);
  }
  uint32_t fill = 0;  // uniform
  for (uint32_t s = 0; s < nseg; ++s) {
    const uint32_t seg = seg0 + s * SEG;
    const uint64_t eq = (s == 0 && first) ? eval_keys(*first, lo, hi, sub) : scan_keys(a.key, seg, lo, hi, sub);
    uint32_t tot;
    const uint32_t pre = block_excl_scan((uint32_t)__popcll(eq), sl.sh16, &tot);
    if (nseg == 1) on_total(tot);
    const uint32_t base = seg + tid * KPL - lo;
    for (uint32_t done = 0; done < tot;) {
      const uint32_t take = (tot - done) < (CHUNK - fill) ? (tot - done) : (CHUNK - fill);
      uint64_t m = eq;
      uint32_t idx = pre;
      while (m) {
        const uint32_t k = (uint32_t)__ffsll((long long)m) - 1;
        m &= m - 1;
        if (idx >= done && idx < done + take) sl.rbuf[fill + idx - done] = base + k;
        ++idx;
      }
      fill += take;
      done += take;
      if (fill == CHUNK) {
        __syncthreads();
        round(fill);
        fill = 0;
      }
    }
  }
  if (fill) {
    __syncthreads();
    round(fill);
  }
}

// Gather the round's records into LDS and counting-sort them by lane: on
// return the lane's messages are perm[*start, *start + *cnt), in arrival order.
// `issued()` runs once the round's record loads are in flight.
template <class St, class Issued>
__device__ __forceinline__ void gather_round(St& sl, const ApplyArgs& a, uint32_t lo, uint32_t fill,
                                             uint32_t* start, uint32_t* cnt, Issued&& issued) {
  constexpr uint32_t PER = St::CHUNK / PART;
  const uint32_t tid = threadIdx.x;
  sl.cnt[tid] = 0;
  __syncthreads();
  MsgRec m[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; ++k) {
    const uint32_t i = tid + k * PART;
    if (i < fill) m[k] = a.rec[lo + sl.rbuf[i]];
  }
  issued();
#pragma unroll
  for (uint32_t k = 0; k < PER; ++k) {
    const uint32_t i = tid + k * PART;
    if (i < fill) {
      uint64_t tm, ix;
      rec_unpack(m[k].info, m[k].orig, m[k].ti, a.side, &tm, &ix);
      sl.w[0][i] = m[k].info;
      sl.w[1][i] = m[k].orig;
      sl.w[2][i] = (uint32_t)tm;
      sl.w[3][i] = (uint32_t)(tm >> 32);
      sl.w[4][i] = (uint32_t)ix;
      sl.w[5][i] = (uint32_t)(ix >> 32);
      atomicAdd(&sl.cnt[(m[k].info >> 16) & (PART - 1)], 1u);
    }
  }
  __syncthreads();
  const uint32_t my_cnt = sl.cnt[tid];
  uint32_t total;
  const uint32_t my_start = block_excl_scan(my_cnt, sl.sh16, &total);
  sl.cnt[tid] = my_start;  // becomes the fill cursor
  __syncthreads();
  for (uint32_t i = tid; i < fill; i += PART) {
    const uint32_t pos = atomicAdd(&sl.cnt[(sl.info(i) >> 16) & (PART - 1)], 1u);
    sl.perm[pos] = (uint16_t)i;
  }
  __syncthreads();
  for (uint32_t x = 1; x < my_cnt; ++x) {  // tiny insertion sort of the lane's run
    const uint16_t v = sl.perm[my_start + x];
    uint32_t y = x;
    while (y > 0 && sl.perm[my_start + y - 1] > v) {
      sl.perm[my_start + y] = sl.perm[my_start + y - 1];
      --y;
    }
    sl.perm[my_start + y] = v;
  }
  *start = my_start;
  *cnt = my_cnt;
}

// The arrival order of a lane's KS route slots as slot numbers in nibbles of
// one word (nibble x = the slot of the lane's x-th message): key[k] = slot k's
// arrival index (0xFFFFFFFF for an unused slot, which sorts last); an
// odd-even transposition network carries the nibbles through its exchanges.
// (Ranking each slot by counting — KS^2 compares, no exchanges — measured
// neutral on cfg3 / cfg4.)
template <uint32_t KS>
__device__ __forceinline__ uint32_t arrival_perm(uint32_t (&key)[KS]) {
  uint32_t perm = 0;
#pragma unroll
  for (uint32_t k = 0; k < KS; ++k) perm |= k << (4 * k);
#pragma unroll
  for (uint32_t r = 0; r < KS; ++r) {
#pragma unroll
    for (uint32_t k = (r & 1); k + 1 < KS; k += 2) {
      const uint32_t k0 = key[k], k1 = key[k + 1];
      const bool sw = k1 < k0;
      key[k] = sw ? k1 : k0;
      key[k + 1] = sw ? k0 : k1;
      const uint32_t p0 = (perm >> (4 * k)) & 0xF, p1 = (perm >> (4 * (k + 1))) & 0xF;
      const uint32_t swp = (perm & ~(0xFFu << (4 * k))) | (p1 << (4 * k)) | (p0 << (4 * (k + 1)));
      perm = sw ? swp : perm;
    }
  }
  return perm;
}

__device__ __forceinline__ bool is_response(uint32_t type) {  // raft/util.go:53-55
  return type == HB_MSG_APP_RESP || type == HB_MSG_VOTE_RESP || type == HB_MSG_HEARTBEAT_RESP ||
         type == HB_MSG_UNREACHABLE;
}

// Reduce the lane statistics of the workgroup and add them (plus the events
// it reserved) to this XCD slot's shard of the step statistics: one no-return
// atomic per value per workgroup, spread over 8 shards; k_finish sums them.
// vals[ST_N] = the lane's events (public count).
template <class T>
__device__ __forceinline__ void reduce_stats(const ApplyArgs& a, uint64_t* l_stats, const T (&vals)[ST_N + 1]) {
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k <= ST_N; ++k) {
    uint64_t v = vals[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0 && v) atomicAdd((unsigned long long*)&l_stats[k], (unsigned long long)v);
  }
  __syncthreads();
  const uint64_t v = tid <= ST_N ? l_stats[tid] : 0ull;
  if (tid <= ST_N && v)
    atomicAdd((unsigned long long*)&a.stats_shard[shard_at(tid, blockIdx.x & (NSH - 1))], (unsigned long long)v);
}

// The fast and leader kernels' lane statistics are small per-lane counts
// (messages, responses, drops: at most the route slots; commits, faults: 0 or
// 1): four 16-bit fields per word keep a wave's sums exact (< 2^16 while each
// lane's count is < 1024), so ten values take four wave reductions, not ten.
template <>
__device__ __forceinline__ void reduce_stats<uint32_t>(const ApplyArgs& a, uint64_t* l_stats,
                                                       const uint32_t (&vals)[ST_N + 1]) {
  const uint32_t tid = threadIdx.x;
  uint64_t w[4] = {(uint64_t)vals[ST_MSGS] | (uint64_t)vals[ST_APPRESP] << 16 | (uint64_t)vals[ST_DROPPED] << 32 |
                       (uint64_t)vals[ST_COMMITS] << 48,
                   (uint64_t)vals[ST_VOTERESP] | (uint64_t)vals[ST_WON] << 16 | (uint64_t)vals[ST_LOST] << 32 |
                       (uint64_t)vals[ST_FAULTS] << 48,
                   (uint64_t)vals[ST_ENTRIES], (uint64_t)vals[ST_N]};
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) w[k] += __shfl_xor(w[k], d);
  if ((tid & 63) == 0) {
    const uint64_t v[ST_N + 1] = {w[0] & 0xFFFF, (w[0] >> 16) & 0xFFFF, w[1] & 0xFFFF, (w[0] >> 32) & 0xFFFF,
                                  w[0] >> 48,    (w[1] >> 16) & 0xFFFF, (w[1] >> 32) & 0xFFFF, w[1] >> 48,
                                  w[2],          w[3]};
    static_assert(ST_MSGS == 0 && ST_APPRESP == 1 && ST_VOTERESP == 2 && ST_DROPPED == 3 && ST_COMMITS == 4 &&
                      ST_WON == 5 && ST_LOST == 6 && ST_FAULTS == 7 && ST_ENTRIES == 8 && ST_N == 9,
                  "the unpacking above follows the ST_ order");
#pragma unroll
    for (int k = 0; k <= ST_N; ++k)
      if (v[k]) atomicAdd((unsigned long long*)&l_stats[k], (unsigned long long)v[k]);
  }
  __syncthreads();
  const uint64_t v = tid <= ST_N ? l_stats[tid] : 0ull;
  if (tid <= ST_N && v)
    atomicAdd((unsigned long long*)&a.stats_shard[shard_at(tid, blockIdx.x & (NSH - 1))], (unsigned long long)v);
}

// ---------------------------------------------------------------------------
// k_route<KMAX>: W = BK / RG workgroups per bucket, each owning RG groups
// (RG x KMAX message slots fit in LDS: RG = 2048 / 1024 for KMAX = 2 / > 2,
// half that in X mode).  Each workgroup streams its bucket's records (coalesced; the W
// sisters of a bucket share one XCD's L2), ranks the messages of its groups
// with one LDS counter per group, stages each group's first KMAX messages in
// LDS and writes them out lane-major (slot k of group g at slots.*[k][g]) with
// coalesced stores, so k_apply_fast reads them in the same round trip as the
// group state.  Counter ranks follow LDS-atomic order, not arrival order:
// k_apply_fast sorts a group's slots by arrival index and hands a group with
// more than KMAX messages to k_apply whole.  cnt[g] = the group's message
// count (saturated at 255).  Each partition reserves its M event chunk in the
// bucket's region (one atomic per partition).  No raft logic runs here.
// ---------------------------------------------------------------------------
constexpr uint32_t ROUTE_THREADS = 1024;
// cnt[g]: the group's message count (saturated at 127) | CNT_HIGHER when some
// message of the group carries a Term above the group's (n >= 5 routes of
// leader-side batches without dense proposals: k_apply_lead then hands a busy leader — an
// election storm's — over without reading its slots or state; cfg4 1.914 ->
// 1.83 ms.  With dense proposals the check cost cfg3 1.3 % for nothing: a
// leader there proposes, and one without the flag is loaded and stepped up to
// the higher term, as before)
constexpr uint32_t CNT_MASK = 0x7F, CNT_HIGHER = 0x80;
// The storm hand-over rule: what k_apply_lead does with a group, in a step
// without dense proposals and without X, before it steps any of its messages.
// k_route closes a partition whose groups with messages are all HO_NONE,
// HO_ELECT or HO_APPLY, and k_apply_lead then skips it (lskip), so the two
// must agree group for group: both call this.
//   not live (removed or faulted)      HO_NONE   nothing to do
//   no leader                          HO_ELECT  handed over unloaded, k_elect's
//   leader, r.Commit unknown (M_NC)    HO_APPLY  handed over unloaded, not k_elect's
//   leader, c <= nmax - 1              HO_LOAD   loaded and stepped
//   leader, nmax - 1 < c <= cap        HO_ELECT  with `higher` (an election storm's leader),
//                                      HO_LOAD   without
//   leader, c > cap                    HO_OVER   handed over unloaded to k_apply (its bucket
//                                                walk); the route keeps such a partition open
// mlo: meta's low word; c: the group's messages in the batch; higher: one of
// its slotted messages carries a Term above the group's (the route's hib,
// CNT_HIGHER); cap: the slots a group keeps.
enum : uint32_t { HO_NONE, HO_LOAD, HO_ELECT, HO_APPLY, HO_OVER };
__device__ __forceinline__ uint32_t handover_class(uint32_t mlo, uint32_t c, bool higher, uint32_t nmax, uint32_t cap) {
  if (m_n(mlo) == 0 || m_fault(mlo) != 0) return HO_NONE;
  if (m_state(mlo) != HB_STATE_LEADER) return HO_ELECT;
  if (mlo & (uint32_t)M_NC) return HO_APPLY;
  if (c > cap) return HO_OVER;
  return (c > nmax - 1 && higher) ? HO_ELECT : HO_LOAD;
}
// (The route writes a group's slots in counter-rank order; sorting them by
// arrival in its write-out, so that k_apply_lead needs no LDS slot copy,
// measured cfg4 1.912 vs 1.871 ms for the sort.)
#ifndef HB_ROUTE_UNROLL
#define HB_ROUTE_UNROLL 4
#endif
constexpr uint32_t ROUTE_UNROLL = HB_ROUTE_UNROLL;  // records in flight per lane
// Route groups per workgroup (log2), measured on MI355X with 16-byte records
// (same-box A/B, r04): KMAX = 2 at 2048 (2 sisters per 4096-group bucket, 72 KB
// LDS) vs 1024: cfg2 119.2 vs 120.5 us, cfg5 0.995 vs 1.004 ms; KMAX = 6 / 8 at
// 1024 vs 512 (buckets of at least 1024 groups): cfg4 1.949 vs 2.020 ms, cfg3
// neutral.  X mode stages twice the bytes per slot, so it keeps half as many.
constexpr uint32_t route_rg_log(uint32_t kmax, bool x = false) {
  return (kmax <= 3 ? 11u : 10u) - (x ? 1u : 0u);
}
template <int KMAX, bool X> struct RouteGeom {
  static constexpr uint32_t RG_LOG = route_rg_log(KMAX, X);
  static constexpr uint32_t RG = 1u << RG_LOG;     // groups per workgroup
  // workgroups per bucket: 2^(PART_LOG + sis_log - RG_LOG) (sis_log >= RG_LOG - PART_LOG)
};

// EN > 0 (n = EN, a step with ApplyArgs::storm): the storm hand-over — the
// route closes the partitions k_apply_lead would only hand over
// (handover_class) and runs the election lane over them in its own
// workgroup, from the LDS slots (§3.2).  EN = 0 carries none of it.
template <int KMAX, bool X, int EN = 0>
__global__ void __launch_bounds__(ROUTE_THREADS) k_route(ApplyArgs a) {
  using RGm = RouteGeom<KMAX, X>;
  constexpr uint32_t RG = RGm::RG, NP = RG / PART;
  const uint32_t sl = a.sis_log, W = 1u << (PART_LOG + sl - RGm::RG_LOG);
  __shared__ uint32_t l_cnt[RG];
  __shared__ uint4 l_slot[KMAX][RG];  // the group's first KMAX records as they will be stored
  __shared__ uint4 l_slotx[X ? KMAX : 1][X ? RG : 1];  // X mode: their extensions
  __shared__ uint32_t l_ptot[NP];
  constexpr bool HI = KMAX >= 5;  // (CNT_HIGHER)
  constexpr bool EL = EN > 0;  // (the host launches it only without props and X)
  static_assert(!EL || (HI && !X && RG == ROUTE_THREADS), "EL: one group per lane");
  __shared__ uint32_t l_pf[EL ? RG / 32 : 1];  // EL: groups k_apply_lead would hand over unloaded (pflag words)
  __shared__ uint32_t l_ok[EL ? NP : 1];        // 1: the partition needs no k_apply_lead
  __shared__ uint64_t l_moff[EL ? NP : 1];      // the partitions' M chunks
  __shared__ uint32_t l_efill[EL ? NP : 1];     // ... and their fill
  __shared__ uint64_t l_stats[EL ? ST_N + 1 : 1];
  // blockIdx -> (bucket, w): the W sisters of a bucket share blockIdx % 8 (one XCD)
  const uint32_t x = blockIdx.x, q = x >> 3;
  const uint32_t bk = ((q / W) << 3) | (x & 7), w = q % W;
  if (bk >= a.NBK) return;  // uniform: grid padding
  const uint32_t tid = threadIdx.x;
  const uint32_t G = a.S.G;
  const uint32_t lg0 = w * RG;  // first group (in the bucket) of this workgroup
  // (uniform; a follower-side batch's route measured +12 us with it)
  const bool hi_on = HI && !X && !a.props_on;
  for (uint32_t i = tid; i < RG; i += ROUTE_THREADS) l_cnt[i] = 0;
  if (tid < NP) l_ptot[tid] = 0;
  if (EL && tid < NP) l_ok[tid] = 1;
  if (EL && tid < NP) l_efill[tid] = 0;
  if (EL && tid <= ST_N) l_stats[tid] = 0;
  __syncthreads();
  const uint32_t lo = a.bk_off[bk], hi = a.bk_off[bk + 1];
  const uint32_t sub_lo = lg0 >> PART_LOG, sub_hi = (lg0 + RG) >> PART_LOG;
  for (uint32_t base = lo; base < hi; base += ROUTE_THREADS * ROUTE_UNROLL) {
    MsgRec m[ROUTE_UNROLL];
    uint4 mx[X ? ROUTE_UNROLL : 1];
    uint32_t sub[ROUTE_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < ROUTE_UNROLL; ++u) {
      const uint32_t p = base + u * ROUTE_THREADS + tid;
      if (p < hi) m[u] = a.rec[p];
      if constexpr (X) mx[u] = p < hi ? a.recx[p] : make_uint4(0, 0, 0, 0);
      sub[u] = p < hi ? rec_sub(m[u].info) : 0xFFu;  // the partition in the bucket
    }
    if (w == 0) {  // the key bytes the general kernel's bucket walk scans (one coalesced store per lane)
#pragma unroll
      for (uint32_t u = 0; u < ROUTE_UNROLL; ++u) {
        const uint32_t p = base + u * ROUTE_THREADS + tid;
        if (p < hi) a.key[p] = (uint8_t)sub[u];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < ROUTE_UNROLL; ++u) {
      const uint32_t p = base + u * ROUTE_THREADS + tid;
      const bool own = p < hi && sub[u] >= sub_lo && sub[u] < sub_hi;
      const uint32_t l = own ? (((sub[u] - sub_lo) << PART_LOG) | ((m[u].info >> 16) & (PART - 1))) : RG;
      if (l < RG) {
        const uint32_t r = atomicAdd(&l_cnt[l], 1u);
        if (r < (uint32_t)KMAX) {
          l_slot[r][l] = make_uint4(m[u].info, m[u].orig, (uint32_t)m[u].ti, (uint32_t)(m[u].ti >> 32));
          if constexpr (X) l_slotx[r][l] = mx[X ? u : 0];
        }
      }
    }
  }
  __syncthreads();
  const uint32_t gbase = (bk << (PART_LOG + sl)) + lg0;
  uint32_t e_c = 0;  // (EL: the lane's group, i = tid)
  bool e_hand = false, e_elect = false;
  uint64_t e_meta = 0;
  for (uint32_t i = tid; i < RG; i += ROUTE_THREADS) {
    const uint32_t c = l_cnt[i], g = gbase + i;
    bool hand = false, elect = false, ok = true;  // (EL)
    if (g < G) {
      // a group whose messages all sit in its slots: any Term above its own?
      bool hib = false;
      uint64_t meta = 0;
      if (EL && c > 0) meta = a.S.meta[g];
      if (hi_on && c <= (uint32_t)KMAX) {
        const uint64_t t = a.S.term[g];
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)KMAX; ++k) {
          if (k < c) {
            const uint4 r = l_slot[k][i];
            uint64_t tm, ix;
            rec_unpack(r.x, r.y, (uint64_t)r.z | ((uint64_t)r.w << 32), a.side, &tm, &ix);
            hib |= tm > t;
          }
        }
      }
      a.cnt[g] = (uint8_t)((c < CNT_MASK ? c : CNT_MASK) | (hib ? CNT_HIGHER : 0u));
      if constexpr (EL) {  // (the slots are written after the election lane)
        if (c > 0) {  // (a group k_apply_lead would load, or hand to k_apply's bucket walk, keeps the partition open)
          const uint32_t cls = handover_class((uint32_t)meta, c, hib, a.nmax, (uint32_t)KMAX);
          elect = cls == HO_ELECT;
          hand = elect || cls == HO_APPLY;
          ok = hand || cls == HO_NONE;
          if (hand) a.resume[g] = 1u << 30;
        }
        e_c = c;
        e_hand = hand;
        e_elect = elect;
        e_meta = meta;
      } else {
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)KMAX; ++k) {
          if (k < c) {
            at32(a.slot, k * G + g) = l_slot[k][i];
            if constexpr (X) at32(a.slotx, k * G + g) = l_slotx[k][i];
          }
        }
      }
    }
    uint32_t s = c;  // the wave's 64 groups lie in one partition
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((tid & 63) == 0 && s) atomicAdd(&l_ptot[i >> PART_LOG], s);
    if constexpr (EL) {
      const uint64_t b = __ballot(hand), bad = __ballot(!ok);
      if ((tid & 63) == 0) {
        l_pf[i >> 5] = (uint32_t)b;
        l_pf[(i >> 5) + 1] = (uint32_t)(b >> 32);
        if (bad) atomicAnd(&l_ok[i >> PART_LOG], 0u);
      }
    }
  }
  __syncthreads();
  if (tid < NP) {
    const uint32_t part = (bk << sl) + w * NP + tid;
    if (part < a.NB) {
      const uint32_t r = atomicAdd(&a.bk_fill[bk * CTR_STRIDE], a.ev_per_msg * (l_ptot[tid] + PART * a.props_on));
      const uint64_t mo =
          (uint64_t)a.ev_per_msg * ((uint64_t)a.NB * PART + lo + ((uint64_t)bk * PART << sl) * a.props_on) + r;
      a.ev_off[2 * part + 1] = mo;
      if constexpr (EL) l_moff[tid] = mo;
    }
  }
  if constexpr (EL) {
    // ---- the election lane over the closed partitions (k_elect's work, slots from LDS)
    __syncthreads();  // l_moff
    const uint32_t p = __builtin_amdgcn_readfirstlane(tid >> PART_LOG);
    const uint32_t g = gbase + tid;
    const bool closed = l_ok[p] != 0;  // (uniform per wave)
    bool done = false;
    uint32_t st_msgs = 0, st_app = 0, st_vote = 0, st_drop = 0, st_commit = 0;
    ElectLane<EN> L;
    L.won = L.lost = L.nev = 0;
    L.committed = L.last = 0;
    uint64_t last0 = 0;
    if (closed) {
      L.S = a.S;
      L.E.chunk = a.ev + l_moff[p];
      L.E.fill = &l_efill[p];
      L.g = g;
      L.meta = e_meta;
      // k_elect's own groups: no leader, or a busy leader with a higher-term message (resume 0, not loaded)
      const bool mine = e_elect && e_c <= (uint32_t)KMAX && L.self() < L.n() && !(L.meta & M_NC);
      if (mine) {
        L.load();
        last0 = L.last;
        const uint64_t commit0 = L.committed;
        uint32_t key[KMAX];
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)KMAX; ++k) key[k] = k < e_c ? l_slot[k][tid].y : 0xFFFFFFFFu;
        const uint32_t perm = arrival_perm<(uint32_t)KMAX>(key);
        uint32_t x = 0;
#pragma nounroll
        for (; x < e_c; ++x) {
          uint32_t inf, org;
          uint64_t mterm, ix;
          slot_unpack(l_slot[(perm >> (4 * x)) & 0xF][tid], a.side, &inf, &org, &mterm, &ix);
          const uint32_t type = inf & 0xF, from = (inf >> 4) & 0xF;
          if (from >= L.n() && is_response(type)) {  // raft/multinode.go:235
            st_drop++;
            continue;
          }
          if (!L.takes(type, from, mterm)) break;
          L.step(type, from, mterm, (inf >> 8) & 1u);
          st_msgs++;
          st_app += type == HB_MSG_APP_RESP;
          st_vote += type == HB_MSG_VOTE_RESP;
        }
        if (x > 0) {
          L.store();
          if (x == e_c) {
            done = true;  // the group's batch ends here
          } else {        // k_apply resumes at message x, loading what was stored
            a.resume[g] = x;
            a.commit0[g] = commit0;
          }
        }
        st_commit = done && L.committed != commit0;
      }
      flag_put<false>(&l_pf[p * FLAG_WORDS], tid & (PART - 1), done);
    }
    // the slots k_apply (or k_apply_lead / k_elect of an open partition) reads
    if (g < G && e_c > 0 && (!closed || (e_hand && !done))) {
#pragma unroll
      for (uint32_t k = 0; k < (uint32_t)KMAX; ++k)
        if (k < e_c) at32(a.slot, k * G + g) = l_slot[k][tid];
    }
    const uint32_t vals[ST_N + 1] = {st_msgs, st_app, st_vote, st_drop, st_commit, L.won, L.lost, 0,
                                     (uint32_t)(L.last - last0), L.nev};
    reduce_stats(a, l_stats, vals);  // (ends with a barrier: l_pf and l_efill are final)
    // ---- close the partitions k_apply_lead would only hand over (its fast_close)
    if (tid < NP * FLAG_WORDS) {
      const uint32_t p = tid / FLAG_WORDS, j = tid % FLAG_WORDS, part = (bk << sl) + w * NP + p;
      if (part < a.NB && l_ok[p]) a.pflag[(size_t)part * FLAG_WORDS + j] = l_pf[p * FLAG_WORDS + j];
    }
    if (tid < NP) {
      const uint32_t part = (bk << sl) + w * NP + tid;
      if (part < a.NB) {
        a.lskip[part] = (uint8_t)l_ok[tid];
        if (l_ok[tid]) {
          a.ev_off[2 * part] = (uint64_t)part * PART * a.ev_per_msg;
          a.ev_counts[2 * part] = 0;
          a.ev_counts[2 * part + 1] = l_efill[tid];
          uint32_t any = 0;
#pragma unroll
          for (uint32_t j = 0; j < FLAG_WORDS; ++j) any |= l_pf[tid * FLAG_WORDS + j];
          const uint32_t xs = blockIdx.x & 7;  // (= the bucket's XCD slot, as k_apply_lead's)
          if (any) a.ap_list[(size_t)xs * a.NB + atomicAdd(&a.ap_cnt[xs * CTR_STRIDE], 1u)] = part;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// k_apply_fast: one workgroup per partition, one lane per group, steady-state
// leader operations only (FastLane).  Every load of the lane (state, its
// message count, its first KMAX messages) is issued at once; no LDS staging,
// no barrier until the statistics.  The first message a lane cannot take
// (and everything after it, and messages beyond KMAX) is handed to k_apply:
// the lane's bit is set in pflag[part] and resume[g] = messages already
// consumed | prop-pending bit.
// ---------------------------------------------------------------------------
// The fast lane's work on one group once its loads are in: the dense proposal into the
// partition's P chunk, then the slot messages in arrival order into its M
// chunk, as far as FastLane takes them.  Sets the group's hand-over bit in
// l_flag (and, n >= 5, its k_elect bit in l_eflag), resume / commit0, and
// returns the statistics of the lane.
// lead: a leader whose state is loaded (the fast path may step it); leader:
// the group is a leader (for k_elect's test) — a leader with more messages
// than slots and no proposal is handed over with its state unloaded.
// fol (X mode): a follower whose messages all sit in its slots, stepped by
// FollowLane as far as it takes them (s_h / s_c: m.LogTerm, m.Commit).
// STEADY (n = 3, two slots, not X mode): a wave whose lanes are all steady or
// idle runs SteadyLane instead (a.steady; `nsteady` counts those waves).
// The event words of a wave that took the steady path (evm: the lane's words,
// 0 for an idle lane).  A lane's words are known, so there is one LDS add per
// wave and chunk, the words of one kind side by side (a group's words keep
// their order).
__device__ __forceinline__ void steady_emit(const ApplyArgs& a, const SteadyLane& P, uint32_t evm, uint32_t lane,
                                            uint64_t poff, uint64_t moff, uint32_t* l_pfill, uint32_t* l_fill) {
  uint32_t tot = 0, base = 0;
#pragma unroll
  for (uint32_t j = 0; j < SteadyLane::EW_P; ++j) tot += (uint32_t)__popcll(__ballot((evm >> j) & 1u));
  if (tot && (lane & 63) == 0) base = atomicAdd(l_pfill, tot);
  base = __builtin_amdgcn_readfirstlane(base);
  uint64_t* chunk = a.ev + poff;
#pragma unroll
  for (uint32_t j = 0; j < SteadyLane::EW_P; ++j) {
    const uint64_t m = __ballot((evm >> j) & 1u);
    if ((evm >> j) & 1u) chunk[base + mbcnt64(m)] = P.word(j, lane);
    base += (uint32_t)__popcll(m);
  }
  tot = 0;
  base = 0;
#pragma unroll
  for (uint32_t j = SteadyLane::EW_P; j < SteadyLane::EW; ++j) tot += (uint32_t)__popcll(__ballot((evm >> j) & 1u));
  if (tot && (lane & 63) == 0) base = atomicAdd(l_fill, tot);
  base = __builtin_amdgcn_readfirstlane(base);
  chunk = a.ev + moff;
#pragma unroll
  for (uint32_t j = SteadyLane::EW_P; j < SteadyLane::EW; ++j) {
    const uint64_t m = __ballot((evm >> j) & 1u);
    if ((evm >> j) & 1u) chunk[base + mbcnt64(m)] = P.word(j, lane);
    base += (uint32_t)__popcll(m);
  }
}

// What the fast lane decides from a group's meta word, message count and
// dense proposal before it loads anything else (one definition for
// k_apply_fast and both passes of k_route_fast: they must agree).
//   live: the slot takes part (valid, n > 0, not faulted).
//   leader: only a leader has fast-path work; any other live group is handed
//     to k_apply whole, without loading its state here (resume bit 30:
//     commit0 = its committed as k_apply loads it).
//   nc: a group that has not stepped since an empty HardState (r.Commit = 0,
//     M_NC) is the general lane's: its first Step sets r.Commit.
//   lead: a leader whose state is loaded.  One the fast path cannot finish
//     (more messages than slots) and without a dense proposal is handed over
//     whole, its state unloaded (cfg4: every group; k_elect / k_apply load it).
struct FastRole {
  bool live, leader, nc, lead;
};
__device__ __forceinline__ FastRole fast_role(uint32_t mlo, bool valid, uint32_t cnt, uint32_t prop_raw,
                                              uint32_t kmax) {
  FastRole r;
  r.live = valid && ((mlo >> 2) & 7) != 0 && ((mlo >> 17) & 0xF) == 0;
  r.leader = r.live && (mlo & 3) == HB_STATE_LEADER;
  r.nc = (mlo & (uint32_t)M_NC) != 0;
  r.lead = r.leader && !r.nc && (cnt <= kmax || prop_raw != 0);
  return r;
}

template <int NMAX, uint32_t KS, bool STEADY = false>
__device__ __forceinline__ bool fast_step(const ApplyArgs& a, FollowLane<NMAX>& L, uint32_t part, uint32_t lane,
                                          bool live, bool lead, bool leader, bool fol, uint32_t prop_raw, uint32_t cnt,
                                          uint32_t (&s_info)[KS], uint32_t (&s_orig)[KS],
                                          uint64_t (&s_term)[KS], uint64_t (&s_index)[KS],
                                          uint64_t (&s_h)[KS], uint64_t (&s_c)[KS],
                                          uint64_t moff, uint32_t* l_pfill, uint32_t* l_fill, uint32_t* l_flag,
                                          uint32_t* l_eflag, uint32_t (&vals)[ST_N + 1], uint32_t& nsteady) {
  constexpr uint32_t KMAX = KS;
  const uint32_t g = part * PART + lane;
  const uint64_t last0 = L.last, commit0 = L.committed;

  bool flagged = false;
  uint32_t resume = 0;
  uint32_t st_msgs = 0, st_drop = 0, st_app = 0;

  // ---- the dense proposal: its events go to the partition's P chunk (fixed
  // slot of ev_per_msg x PART words), before any message event of the group.
  const uint64_t poff = (uint64_t)part * PART * a.ev_per_msg;
  if (lane == 0) a.ev_off[2 * part] = poff;
  const uint32_t prop_k = live ? prop_raw : 0u;
  if constexpr (STEADY) {
    static_assert(NMAX == 3 && KS == 2, "SteadyLane is the n = 3, two-slot lane");
    if (a.steady) {  // (uniform)
      // idle: nothing is stepped and nothing stored below (not live; or no
      // proposal and no message, and a loaded leader's load / store are
      // no-ops: M_RS clear, self a slot).  A live non-leader with work is
      // neither: it is handed over.
      const bool work = live && (prop_k != 0 || cnt != 0);
      const bool idle = !work && (!lead || (!(L.mlo & (uint32_t)M_RS) && L.self() < 3));
      SteadyLane P;
      P.ok = false;
      P.evm = 0;
      if (lead && work) P.plan(L, prop_k, cnt, s_info, s_orig, s_term, s_index);
      const bool steady = lead && work && P.ok;
      if (__ballot(!(steady || idle)) == 0) {
        steady_emit(a, P, steady ? P.evm : 0u, lane, poff, moff, l_pfill, l_fill);
        if (steady) P.commit(L);
        // (no lane is flagged: resume, commit0, cnt and the slots are not
        // written, and the partition's hand-over bits stay 0)
        vals[ST_MSGS] = steady ? cnt : 0u;
        vals[ST_APPRESP] = steady ? cnt : 0u;
        vals[ST_VOTERESP] = 0;
        vals[ST_DROPPED] = 0;
        vals[ST_COMMITS] = (uint32_t)(steady && P.committed != commit0);
        vals[ST_WON] = 0;
        vals[ST_LOST] = 0;
        vals[ST_FAULTS] = 0;
        vals[ST_ENTRIES] = steady ? (uint32_t)(P.last - last0) : 0u;
        vals[ST_N] = steady ? P.nev() : 0u;
        if (a.steady_cnt && __ballot(g < a.S.G) != 0) ++nsteady;  // (tests; a wave of grid padding is not counted)
        return false;
      }
    }
  }
  L.E.chunk = a.ev + poff;
  L.E.fill = l_pfill;
  if (prop_k) {
    if (lead && L.prop_ok(prop_k)) {
      L.arrival = 0xFFFFFFFFu;
      L.prop(prop_k);
    } else {
      flagged = true;
      resume = 1u << 31;  // the proposal itself is pending (stepped by k_apply into the M chunk)
    }
  }

  // ---- the lane's messages, arrival order (M chunk reserved by k_route).  The
  // slots arrive in k_route's counter order: sort them by arrival index
  // (odd-even transposition over KMAX registers; unused slots sort last).
#pragma unroll
  for (uint32_t k = 0; k < KMAX; ++k) s_orig[k] = k < cnt ? s_orig[k] : 0xFFFFFFFFu;
#pragma unroll
  for (uint32_t r = 0; r < KMAX; ++r) {
#pragma unroll
    for (uint32_t k = (r & 1); k + 1 < KMAX; k += 2) {
      const bool sw = s_orig[k + 1] < s_orig[k];
      const uint32_t i0 = s_info[k], o0 = s_orig[k];
      const uint64_t t0 = s_term[k], x0 = s_index[k], h0 = s_h[k], c0 = s_c[k];
      s_info[k] = sw ? s_info[k + 1] : i0;
      s_orig[k] = sw ? s_orig[k + 1] : o0;
      s_term[k] = sw ? s_term[k + 1] : t0;
      s_index[k] = sw ? s_index[k + 1] : x0;
      s_h[k] = sw ? s_h[k + 1] : h0;
      s_c[k] = sw ? s_c[k + 1] : c0;
      s_info[k + 1] = sw ? i0 : s_info[k + 1];
      s_orig[k + 1] = sw ? o0 : s_orig[k + 1];
      s_term[k + 1] = sw ? t0 : s_term[k + 1];
      s_index[k + 1] = sw ? x0 : s_index[k + 1];
      s_h[k + 1] = sw ? h0 : s_h[k + 1];
      s_c[k + 1] = sw ? c0 : s_c[k + 1];
    }
  }
  L.E.chunk = a.ev + moff;
  L.E.fill = l_fill;
  uint32_t j = 0;  // messages consumed
  if (live && !lead && !fol && cnt > 0 && !flagged) {
    flagged = true;
    resume = 0;
  }
  if (live && cnt > KMAX && !flagged && !L.faulted()) {  // the slots hold an arbitrary KMAX: all to k_apply
    flagged = true;
    resume = 0;
  }
  if (lead) {
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k) {
      if (k >= cnt || flagged || L.faulted()) break;
      const uint32_t inf = s_info[k];
      const uint32_t type = inf & 0xF, from = (inf >> 4) & 0xF;
      const bool reject = (inf >> 8) & 1u;
      if (from >= L.n() && is_response(type)) {  // raft/multinode.go:235
        st_drop++;
        j++;
        continue;
      }
      if (KMAX >= 3 && type == HB_MSG_PROP) {  // a local proposal (Term 0; Index = its entry count): stepLeader MsgProp
        if (s_term[k] != 0 || s_index[k] > 0xFFFFFFFFull || !L.prop_ok((uint32_t)s_index[k])) {
          flagged = true;
          resume = j;
          break;
        }
        L.arrival = s_orig[k];
        L.prop((uint32_t)s_index[k]);
        st_msgs++;
        j++;
        continue;
      }
      if (!L.accept_ok(type, from, s_term[k], reject)) {
        flagged = true;
        resume = j;
        break;
      }
      L.arrival = s_orig[k];
      L.accept(from, s_index[k]);
      st_msgs++;
      if (KMAX >= 3) st_app++;
      j++;
    }
  }
  bool fstepped = false;  // FollowLane stepped a message: its state is stored
  if (fol) {
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k) {
      if (k >= cnt || flagged || L.faulted()) break;
      const uint32_t inf = s_info[k];
      const uint32_t from = (inf >> 4) & 0xF;
      if (!L.takes_follow(inf, from, s_term[k], s_index[k], s_h[k], s_c[k])) {
        flagged = true;
        resume = j;
        break;
      }
      L.arrival = s_orig[k];
      L.step_follow(inf, from, s_term[k], s_index[k], s_h[k], s_c[k]);
      fstepped = true;
      st_msgs++;
      j++;
    }
  }

  if (lead) L.store();
  if (fstepped) L.store_follow();
  const bool stored = lead || fstepped;
  if constexpr (NMAX >= 5) {  // k_elect's candidates: an election (or a step-down) is likely
    bool higher = false;
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k) higher |= k < cnt && s_term[k] > L.term;
    flag_put<true>(l_eflag, lane, flagged && (!leader || higher));
  }
  flag_put<true>(l_flag, lane, flagged);
  if (flagged) {
    at32(a.resume, g) = resume | (stored ? 0u : 1u << 30);
    if (stored) at32(a.commit0, g) = commit0;
  }
  vals[ST_MSGS] = st_msgs;
  vals[ST_APPRESP] = KMAX >= 3 ? st_app : (lead ? st_msgs : 0u);  // (two slots: every leader message is a MsgAppResp)
  vals[ST_VOTERESP] = 0;
  vals[ST_DROPPED] = st_drop;
  vals[ST_COMMITS] = (uint32_t)(!flagged && L.committed != commit0);  // commitTo only raises
  vals[ST_WON] = 0;
  vals[ST_LOST] = 0;
  vals[ST_FAULTS] = (uint32_t)(L.faulted() != 0 && live);
  vals[ST_ENTRIES] = (uint32_t)(L.last - last0);  // (entries appended to one group in one step)
  vals[ST_N] = L.nev;
  return flagged;
}

// The partition's bookkeeping after its lanes (one lane: `lane == 0`'s thread):
// event fills, and the k_apply / k_elect work lists of this XCD slot.
__device__ __forceinline__ void fast_close(const ApplyArgs& a, uint32_t part, const uint32_t* l_flag,
                                           const uint32_t* l_eflag, uint32_t pfill, uint32_t fill) {
  a.ev_counts[2 * part] = pfill;
  a.ev_counts[2 * part + 1] = fill;
  uint32_t any = 0, eany = 0;
#pragma unroll
  for (uint32_t w = 0; w < FLAG_WORDS; ++w) {
    any |= l_flag[w];
    eany |= l_eflag ? l_eflag[w] : 0u;
  }
  const uint32_t xs = blockIdx.x & 7;
  if (any)  // the partition joins k_apply's list of its XCD slot
    a.ap_list[(size_t)xs * a.NB + atomicAdd(&a.ap_cnt[xs * CTR_STRIDE], 1u)] = part;
  if (eany)  // ... and k_elect's
    a.el_list[(size_t)xs * a.NB + atomicAdd(&a.el_cnt[xs * CTR_STRIDE], 1u)] = part;
}

// (n = 3 only: n >= 5 runs k_apply_lead)
template <int NMAX, bool X, uint32_t KMAX>  // KMAX: one MsgAppResp per follower per batch (+ a MsgProp)
__global__ void __launch_bounds__(PART, HB_FAST_WAVES) k_apply_fast(ApplyArgs a) {
  static_assert(NMAX <= 3, "n >= 5 leaders and followers step in k_apply_lead");
  __shared__ uint32_t l_fill, l_pfill;
  __shared__ uint32_t l_flag[FLAG_WORDS];
  __shared__ uint32_t l_eflag[FLAG_WORDS];
  __shared__ uint64_t l_stats[ST_N + 1];
  __shared__ uint32_t l_steady;

  const uint32_t part = block_part(a.sis_log);
  if (part >= a.NB) return;  // uniform: grid padding
  const uint32_t tid = threadIdx.x;
  const uint32_t g = part * PART + tid;
  const bool gvalid = g < a.S.G;
  if (tid == 0) l_fill = l_pfill = l_steady = 0;
  if (tid <= ST_N) l_stats[tid] = 0;
  if (tid < FLAG_WORDS) l_flag[tid] = l_eflag[tid] = 0;

  // ---- every load of the lane, one round trip
  FollowLane<NMAX> L;
  L.S = a.S;
  L.g = g;
  L.mlo = gvalid ? at32(reinterpret_cast<uint32_t*>(a.S.meta), 2 * g) : 0u;
  const uint32_t prop_raw = (a.props && gvalid) ? at32(a.props, g) : 0u;
  const uint32_t cnt = gvalid ? at32(a.cnt, g) & CNT_MASK : 0u;
  // The state that depends on nothing is loaded beside meta (one round trip
  // fewer for every leader; a group with no fast-path work wastes 52 bytes)
  if (gvalid) L.load_head();
  // A group takes part when its slot is live (n > 0) and not faulted.
  const FastRole role = fast_role(L.mlo, gvalid, cnt, prop_raw, KMAX);
  const bool live = role.live, leader = role.leader, nc = role.nc, lead = role.lead;
  // X mode: a follower whose messages all sit in its slots and that has no
  // dense proposal (stepFollower MsgProp forwards it: the general lane)
  const bool fol = X && live && !nc && L.state() == HB_STATE_FOLLOWER && cnt > 0 && cnt <= KMAX && prop_raw == 0;
  L.dirty = 0;
  L.nev = 0;
  if (lead) {
    L.load_rest();
  } else if (fol) {
    L.load_follow();
  } else {
    L.last = L.committed = 0;
    if (!(NMAX >= 5 && leader)) L.term = 0;
  }
  uint32_t s_info[KMAX], s_orig[KMAX];
  uint64_t s_term[KMAX], s_index[KMAX], s_h[KMAX], s_c[KMAX];
  // a leader's (follower's) used slots, in the state loads' round trip (both
  // wait for meta and the count); a group the fast path cannot finish reads none
  const bool slots = (lead || fol) && cnt <= KMAX;
  uint4 raw[KMAX];
#pragma unroll
  for (uint32_t k = 0; k < KMAX; ++k) {
    // (n >= 5: a busier leader's terms too, for k_elect's step-down test below)
    const bool u = NMAX >= 5 ? leader && k < cnt : slots && k < cnt;
    raw[k] = u ? at32(a.slot, k * a.S.G + g) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (uint32_t k = 0; k < KMAX; ++k) slot_unpack(raw[k], a.side, &s_info[k], &s_orig[k], &s_term[k], &s_index[k]);
#pragma unroll
  for (uint32_t k = 0; k < KMAX; ++k) {
    uint4 x = make_uint4(0, 0, 0, 0);
    if (X && fol && k < cnt) x = at32(a.slotx, k * a.S.G + g);
    s_h[k] = (uint64_t)x.x | ((uint64_t)x.y << 32);
    s_c[k] = (uint64_t)x.z | ((uint64_t)x.w << 32);
  }
  uint32_t vals[ST_N + 1];
  constexpr bool STEADY = NMAX == 3 && KMAX == 2 && !X;
  uint32_t nsteady = 0;
  (void)fast_step<NMAX, KMAX, STEADY>(a, L, part, tid, live, lead, leader, fol, prop_raw, cnt, s_info, s_orig, s_term,
                                      s_index, s_h, s_c, a.ev_off[2 * part + 1], &l_pfill, &l_fill, l_flag, l_eflag, vals,
                                      nsteady);
  if (STEADY && a.steady_cnt && nsteady && (tid & 63) == 0) atomicAdd(&l_steady, nsteady);
  reduce_stats(a, l_stats, vals);
  if (STEADY && a.steady_cnt && tid == 0 && l_steady) atomicAdd(a.steady_cnt, l_steady);
  if (tid < FLAG_WORDS) a.pflag[(size_t)part * FLAG_WORDS + tid] = l_flag[tid];
  if constexpr (NMAX >= 5) {
    if (tid < FLAG_WORDS) a.eflag[(size_t)part * FLAG_WORDS + tid] = l_eflag[tid];
  }
  if (tid == 0) fast_close(a, part, l_flag, NMAX >= 5 ? l_eflag : nullptr, l_pfill, l_fill);
}

// ---------------------------------------------------------------------------
// k_route_fast<KMAX, X, WIDE>: k_route<KMAX, X> and k_apply_fast<3, X, KMAX> in one
// workgroup (n = 3, prep and apply on one stream).  The route phase stages
// each of the workgroup's RG groups' first KMAX messages (and, X mode, their
// extensions) in LDS exactly as k_route does; the fast lane then reads them
// from there instead of from the slot arrays, so the slots are neither
// written nor read back (16 + 16 B per message in X mode, plus the count, each
// way).  Only a group the fast lane hands over gets its count and slots
// written to HBM, where k_apply reads them.  Narrow form: 512 lanes per
// workgroup and at most ~73 KB of LDS (RG = 2048 groups for two leader-side
// slots, fewer when a group keeps more bytes), two workgroups per CU; wide
// form (RouteFastGeom, below): twice the lanes, groups and LDS, one workgroup
// per CU.  Each lane steps RG / lanes groups in turn, with no barrier between
// them (the partitions' event cursors and hand-over masks stay in LDS until
// the end).  A workgroup that owns its whole bucket (W = 1) places its
// partitions' M event chunks by a prefix in LDS; sisters share the bucket's
// cursor in bk_fill.  Measured on
// cfg2 (same-box A/Bs) and not kept: 1024-group workgroups of 256 or 512
// lanes (+6-9 %), 8 or 16 records in flight per lane in the route phase
// (0 / +1.5 %), the slots staged as four 4-byte planes (neutral), the group
// loop not unrolled (neutral), the next group's first-round loads issued
// before this group's second round in that one loop (+8 %: it spills).  With
// two slots and not in X mode the lane's groups are stepped in two passes:
// the steady group-waves by steady_pass, which has that look-ahead, then the
// rest by the loop below.
// ---------------------------------------------------------------------------
#ifndef HB_RF_UNROLL
#define HB_RF_UNROLL 4  // records in flight per lane in the route phase
#endif
#ifndef HB_RF_WAVES
#define HB_RF_WAVES 4
#endif
constexpr uint32_t RF_UNROLL = HB_RF_UNROLL;
// The forms an eligible handle runs wide, bit (KMAX == 3) * 2 + X: <2, false>
// (the leader-side step, measured: DESIGN §3.3a).  The other three keep narrow
// until their own workloads are measured wide.
constexpr uint32_t RF_WIDE_FORMS = 3u;
// Two geometries, both compiled; the handle picks one at hb_create (rf_wide).
// Narrow: 512 lanes, two workgroups per CU.  Wide: 1024 lanes and twice the
// groups, one workgroup per CU with the same 16 waves and up to 148 KB of LDS:
// for handles whose buckets hold 4096 groups or more, where a narrow
// workgroup shares its bucket with a sister that streams the same records.
// A lane steps RG / THREADS groups in either form.
template <uint32_t KMAX, bool X, bool WIDE> struct RouteFastGeom {
  static constexpr uint32_t THREADS = WIDE ? 1024 : 512;
  // 16 B per slot, twice in X mode: 2 slots x 2048, 3 x 1024, X 2 x 1024, X 3 x 512 groups (wide: twice that)
  static constexpr uint32_t RG_LOG = (WIDE ? 12u : 11u) - (KMAX > 2 ? 1u : 0u) - (X ? 1u : 0u);
  static constexpr uint32_t RG = 1u << RG_LOG;  // groups per workgroup
  static constexpr uint32_t NP = RG / PART;     // partitions per workgroup
};
// Group i of the workgroup (0 <= i < RG) as the fast lane names it.
struct RouteFastGroup {
  uint32_t p, part, lane, g;
  bool valid;
  __device__ __forceinline__ RouteFastGroup(const ApplyArgs& a, uint32_t part0, uint32_t i) {
    // (a wave's 64 groups lie in one partition: kept as a scalar)
    p = (uint32_t)__builtin_amdgcn_readfirstlane(i >> PART_LOG);
    part = part0 + p;
    lane = i & (PART - 1);
    g = part * PART + lane;
    valid = part < a.NB && g < a.S.G;
  }
};

// Pass 1 of k_route_fast<2, false> over a lane's RG / THREADS groups: the
// group-waves whose lanes are all steady or idle are stepped here (what
// fast_step's steady branch does, on SteadyIn instead of a FastLane), with the
// next group's first round trip (SteadyHead) in flight under the current
// group's second round trip, plan, events and stores.  H holds group 0's, issued
// before the route phase.  A group-wave that is not steady is left untouched
// (nothing is written before the vote) and its bit is set in the returned
// mask; the wave owns its group-waves, so the mask is wave-uniform.  The
// statistics a steady step can make non-zero are added to acc.
template <uint32_t RG, uint32_t THREADS>
__device__ __forceinline__ uint32_t steady_pass(const ApplyArgs& a, SteadyHead H, uint32_t part0,
                                                const uint32_t* l_cnt, const uint4 (*l_slot)[RG],
                                                const uint64_t* l_moff, uint32_t* l_pfill, uint32_t* l_fill,
                                                uint32_t (&acc)[ST_N + 1], uint32_t& nsteady) {
  constexpr uint32_t NW = RG / THREADS;
  uint32_t pend = 0;
  uint32_t msgs = 0, commits = 0, entries = 0, nev = 0;
  // (unrolled: the `k + 1 < NW` below must fold, or the loads under it sit
  // behind a join like the one SteadyHead::load avoids)
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) {
    const uint32_t i = threadIdx.x + k * THREADS;
    const RouteFastGroup R(a, part0, i);
    SteadyIn L(a.S, R.g, H);
    const uint32_t prop_k = H.props;  // (0 unless the group is valid)
    const uint32_t c = R.valid ? l_cnt[i] : 0u;
    const uint32_t cnt = c < CNT_MASK ? c : CNT_MASK;
    const FastRole role = fast_role(L.mlo, R.valid, cnt, prop_k, 2);
    const bool live = role.live, lead = role.lead;
    if (lead) L.load_rest();
    uint32_t s_info[2], s_orig[2];
    uint64_t s_term[2], s_index[2];
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
      const bool u = lead && cnt <= 2 && j < cnt;
      slot_unpack(u ? l_slot[j][i] : make_uint4(0, 0, 0, 0), a.side, &s_info[j], &s_orig[j], &s_term[j], &s_index[j]);
    }
    uint64_t moff = l_moff[R.p];
    moff = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)moff) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(moff >> 32)) << 32;
    // ---- the look-ahead: the next group's first round trip leaves now
    if (k + 1 < NW) {  // (uniform)
      const RouteFastGroup N(a, part0, i + THREADS);
      H.load(a.S, a.props, N.g, N.valid);
    }
    // ---- fast_step's steady branch
    const bool work = live && (prop_k != 0 || cnt != 0);
    const bool idle = !work && (!lead || (!(L.mlo & (uint32_t)M_RS) && L.self() < 3));
    SteadyLane P;
    P.ok = false;
    P.evm = 0;
    if (lead && work) P.plan(L, prop_k, cnt, s_info, s_orig, s_term, s_index);
    const bool steady = lead && work && P.ok;
    if (__ballot(!(steady || idle)) != 0) {
      pend |= 1u << k;
      continue;
    }
    const uint64_t poff = (uint64_t)R.part * PART * a.ev_per_msg;
    if (R.lane == 0) a.ev_off[2 * R.part] = poff;
    steady_emit(a, P, steady ? P.evm : 0u, R.lane, poff, moff, &l_pfill[R.p], &l_fill[R.p]);
    if (steady) P.commit(L);
    msgs += steady ? cnt : 0u;
    commits += (uint32_t)(steady && P.committed != L.committed);
    entries += steady ? (uint32_t)(P.last - L.last) : 0u;
    nev += steady ? P.nev() : 0u;
    if (a.steady_cnt && __ballot(R.g < a.S.G) != 0) ++nsteady;  // (tests; a wave of grid padding is not counted)
  }
  acc[ST_MSGS] += msgs;
  acc[ST_COMMITS] += commits;
  acc[ST_ENTRIES] += entries;
  acc[ST_N] += nev;
  return (uint32_t)__builtin_amdgcn_readfirstlane(pend);
}

template <uint32_t KMAX, bool X, bool WIDE>
__global__ void __launch_bounds__((RouteFastGeom<KMAX, X, WIDE>::THREADS), HB_RF_WAVES) k_route_fast(ApplyArgs a) {
  constexpr int NMAX = 3;
  using GM = RouteFastGeom<KMAX, X, WIDE>;
  constexpr uint32_t RG = GM::RG, NP = GM::NP, RF_THREADS = GM::THREADS;
  const uint32_t sl = a.sis_log, W = 1u << (PART_LOG + sl - GM::RG_LOG);
  __shared__ uint32_t l_cnt[RG];
  __shared__ uint4 l_slot[KMAX][RG];
  __shared__ uint4 l_slotx[X ? KMAX : 1][X ? RG : 1];
  __shared__ uint32_t l_ptot[NP];
  __shared__ uint64_t l_moff[NP];
  __shared__ uint32_t l_fill[NP], l_pfill[NP];
  __shared__ uint32_t l_flag[NP][FLAG_WORDS];
  __shared__ uint64_t l_stats[ST_N + 1];
  const uint32_t x = blockIdx.x, q = x >> 3;
  const uint32_t bk = ((q / W) << 3) | (x & 7), w = q % W;
  if (bk >= a.NBK) return;  // uniform: grid padding
  const uint32_t tid = threadIdx.x;
  const uint32_t G = a.S.G;
  const uint32_t lg0 = w * RG;
  const uint32_t part0 = (bk << sl) + w * NP;
  constexpr bool STEADY = KMAX == 2 && !X;
  // (pass 1, below: its first group's first round trip crosses the route phase in flight)
  SteadyHead H0 = {};
  if constexpr (STEADY) {
    if (a.steady) {  // (uniform)
      const RouteFastGroup R(a, part0, tid);
      H0.load(a.S, a.props, R.g, R.valid);
    }
  }
  for (uint32_t i = tid; i < RG; i += RF_THREADS) l_cnt[i] = 0;
  if (tid < NP) {
    l_ptot[tid] = 0;
    l_fill[tid] = l_pfill[tid] = 0;
  }
  for (uint32_t i = tid; i < NP * FLAG_WORDS; i += RF_THREADS) (&l_flag[0][0])[i] = 0;
  if (tid <= ST_N) l_stats[tid] = 0;
  __syncthreads();
  // ---- route: the bucket's records, the workgroup's groups ranked into LDS (as k_route)
  const uint32_t lo = a.bk_off[bk], hi = a.bk_off[bk + 1];
  const uint32_t sub_lo = lg0 >> PART_LOG, sub_hi = (lg0 + RG) >> PART_LOG;
  for (uint32_t base = lo; base < hi; base += RF_THREADS * RF_UNROLL) {
    MsgRec m[RF_UNROLL];
    uint4 mx[X ? RF_UNROLL : 1];
    uint32_t sub[RF_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < RF_UNROLL; ++u) {
      const uint32_t p = base + u * RF_THREADS + tid;
      if (p < hi) m[u] = a.rec[p];
      if constexpr (X) mx[u] = p < hi ? a.recx[p] : make_uint4(0, 0, 0, 0);
      sub[u] = p < hi ? rec_sub(m[u].info) : 0xFFu;
    }
    if (w == 0) {  // the key bytes of the general kernel's bucket walk
#pragma unroll
      for (uint32_t u = 0; u < RF_UNROLL; ++u) {
        const uint32_t p = base + u * RF_THREADS + tid;
        if (p < hi) a.key[p] = (uint8_t)sub[u];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < RF_UNROLL; ++u) {
      const uint32_t p = base + u * RF_THREADS + tid;
      const bool own = p < hi && sub[u] >= sub_lo && sub[u] < sub_hi;
      const uint32_t l = own ? (((sub[u] - sub_lo) << PART_LOG) | ((m[u].info >> 16) & (PART - 1))) : RG;
      if (l < RG) {
        const uint32_t r = atomicAdd(&l_cnt[l], 1u);
        if (r < KMAX) {
          l_slot[r][l] = make_uint4(m[u].info, m[u].orig, (uint32_t)m[u].ti, (uint32_t)(m[u].ti >> 32));
          if constexpr (X) l_slotx[r][l] = mx[X ? u : 0];
        }
      }
    }
  }
  __syncthreads();
  // ---- each partition's M event chunk in its bucket's region (as k_route)
  for (uint32_t i = tid; i < RG; i += RF_THREADS) {
    uint32_t s = l_cnt[i];  // (a wave's 64 groups lie in one partition)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((tid & 63) == 0 && s) atomicAdd(&l_ptot[i >> PART_LOG], s);
  }
  __syncthreads();
  if (tid < NP) {
    const uint32_t part = part0 + tid;
    uint64_t mo = 0;
    if (part < a.NB) {
      uint32_t r = 0;
      if (W == 1) {  // (uniform) the bucket is this workgroup's: its partitions' chunks in order, no cursor
        for (uint32_t j = 0; j < NP; ++j) {
          const uint32_t n = a.ev_per_msg * (l_ptot[j] + PART * a.props_on);
          r += j < tid ? n : 0u;  // (a partition past NB has no lower sister inside NB)
        }
      } else {
        r = atomicAdd(&a.bk_fill[bk * CTR_STRIDE], a.ev_per_msg * (l_ptot[tid] + PART * a.props_on));
      }
      mo = (uint64_t)a.ev_per_msg * ((uint64_t)a.NB * PART + lo + ((uint64_t)bk * PART << sl) * a.props_on) + r;
      a.ev_off[2 * part + 1] = mo;
    }
    l_moff[tid] = mo;
    l_ptot[tid] = 0;  // (read above: word 0 now counts the steady group-waves, a.steady_cnt)
  }
  __syncthreads();
  // ---- the fast lane (as k_apply_fast) over the workgroup's groups, RG / RF_THREADS per lane
  uint32_t acc[ST_N + 1];
#pragma unroll
  for (int k = 0; k <= ST_N; ++k) acc[k] = 0;
  uint32_t nsteady = 0;
  // Two passes (two slots, not X mode): the steady group-waves first, on the
  // lean lane with its look-ahead; then the others, as k_apply_fast steps
  // them.  A lane's groups are distinct, so the order between them is free.
  // (HB_FAST_STEADY=0: every group-wave is pass 2's.)
  uint32_t pend = (1u << (RG / RF_THREADS)) - 1;
  if constexpr (STEADY) {
    if (a.steady)  // (uniform)
      pend = steady_pass<RG, RF_THREADS>(a, H0, part0, l_cnt, l_slot, l_moff, l_pfill, l_fill, acc, nsteady);
  }
  for (uint32_t i = tid, kw = 0; i < RG; i += RF_THREADS, ++kw) {
    if (STEADY && !((pend >> kw) & 1u)) continue;  // (uniform) stepped by pass 1
    // (a wave's 64 groups lie in one partition: with the steady path the
    // partition and its M chunk are kept as scalars, which frees the lane
    // registers the two paths need side by side)
    const uint32_t p = STEADY ? (uint32_t)__builtin_amdgcn_readfirstlane(i >> PART_LOG) : i >> PART_LOG;
    const uint32_t part = part0 + p, lane = i & (PART - 1);
    const uint32_t g = part * PART + lane;
    const bool gvalid = part < a.NB && g < G;
    uint64_t moff = l_moff[p];
    if constexpr (STEADY)
      moff = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)moff) |
             (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(moff >> 32)) << 32;
    FollowLane<NMAX> L;
    L.S = a.S;
    L.g = g;
    L.mlo = gvalid ? at32(reinterpret_cast<uint32_t*>(a.S.meta), 2 * g) : 0u;
    const uint32_t prop_raw = (a.props && gvalid) ? at32(a.props, g) : 0u;
    const uint32_t c = gvalid ? l_cnt[i] : 0u;
    const uint32_t cnt = c < CNT_MASK ? c : CNT_MASK;
    if (gvalid) L.load_head();
    const FastRole role = fast_role(L.mlo, gvalid, cnt, prop_raw, KMAX);
    const bool live = role.live, leader = role.leader, nc = role.nc, lead = role.lead;
    const bool fol = X && live && !nc && L.state() == HB_STATE_FOLLOWER && cnt > 0 && cnt <= KMAX && prop_raw == 0;
    L.dirty = 0;
    L.nev = 0;
    if (lead) {
      L.load_rest();
    } else if (fol) {
      L.load_follow();
    } else {
      L.last = L.committed = 0;
      L.term = 0;
    }
    uint32_t s_info[KMAX], s_orig[KMAX];
    uint64_t s_term[KMAX], s_index[KMAX], s_h[KMAX], s_c[KMAX];
    const bool slots = (lead || fol) && cnt <= KMAX;
#pragma unroll
    for (uint32_t k = 0; k < KMAX; ++k) {
      const bool u = slots && k < cnt;
      slot_unpack(u ? l_slot[k][i] : make_uint4(0, 0, 0, 0), a.side, &s_info[k], &s_orig[k], &s_term[k], &s_index[k]);
      uint4 xe = make_uint4(0, 0, 0, 0);
      if constexpr (X) {
        if (fol && k < cnt) xe = l_slotx[k][i];
      }
      s_h[k] = (uint64_t)xe.x | ((uint64_t)xe.y << 32);
      s_c[k] = (uint64_t)xe.z | ((uint64_t)xe.w << 32);
    }
    uint32_t vals[ST_N + 1];
    // (the steady branch off: pass 1 has taken this group-wave's vote)
    const bool flagged = fast_step<NMAX, KMAX, false>(a, L, part, lane, live, lead, leader, fol, prop_raw, cnt, s_info,
                                                      s_orig, s_term, s_index, s_h, s_c, moff, &l_pfill[p],
                                                      &l_fill[p], l_flag[p], nullptr, vals, nsteady);
    // (two slots, not X mode: only a leader's messages are stepped here and
    // each is a MsgAppResp, so that sum is the message sum: one register less)
#pragma unroll
    for (int k = 0; k <= ST_N; ++k)
      if (!(STEADY && k == ST_APPRESP)) acc[k] += vals[k];
    if (flagged) {  // what k_apply reads of a group it takes over: its count and slots
      a.cnt[g] = (uint8_t)cnt;
#pragma unroll
      for (uint32_t k = 0; k < KMAX; ++k) {
        if (k < c) {
          at32(a.slot, k * G + g) = l_slot[k][i];
          if constexpr (X) at32(a.slotx, k * G + g) = l_slotx[k][i];
        }
      }
    }
  }
  if constexpr (STEADY) acc[ST_APPRESP] = acc[ST_MSGS];
  if (STEADY && a.steady_cnt && nsteady && (tid & 63) == 0) atomicAdd(&l_ptot[0], nsteady);
  reduce_stats(a, l_stats, acc);  // (ends with a barrier: the partitions' fills and flags are final)
  if (STEADY && a.steady_cnt && tid == 0 && l_ptot[0]) atomicAdd(a.steady_cnt, l_ptot[0]);
  for (uint32_t j = tid; j < NP * FLAG_WORDS; j += RF_THREADS) {
    const uint32_t p = j / FLAG_WORDS, part = part0 + p;
    if (part < a.NB) a.pflag[(size_t)part * FLAG_WORDS + j % FLAG_WORDS] = l_flag[p][j % FLAG_WORDS];
  }
  if (tid < NP && part0 + tid < a.NB) fast_close(a, part0 + tid, l_flag[tid], nullptr, l_pfill[tid], l_fill[tid]);
}

// ---------------------------------------------------------------------------
// k_apply: the general state machine (Lane::step) for the groups
// k_apply_fast handed over, from their resume point: every leader / candidate
// message type; at a group's first follower-side message (MsgApp /
// MsgHeartbeat / MsgSnap / MsgVote) the group is handed on to a second pass
// over the same partition with the follower-capable lane (Lane<NMAX, true>).
// Only partitions k_apply_fast put on a work list are visited.  A group whose
// messages all sit in its k_route slots (count <= route_kmax) steps them from
// there, in arrival order; the bucket is walked (LDS rounds) only when some
// group of the partition has more messages than slots.
// ---------------------------------------------------------------------------
#ifndef HB_GEN_WAVES
#define HB_GEN_WAVES 2
#endif
struct GenShared {
  Stage<CHUNK> sl;
  uint32_t l_fill;
  uint32_t l_flag[FLAG_WORDS];
  uint32_t l_next[FLAG_WORDS];  // groups handed on to the follower-side pass
  uint64_t l_stats[ST_N + 1];
};

// One partition through the general lane.  FOLLOW = false: the groups
// k_apply_fast flagged (pflag); returns whether any was handed on at a
// follower-side message (sh.l_next).  FOLLOW = true, chained: those groups,
// right after, in the same workgroup (flags and the chunk fill from LDS).
template <int NMAX, bool FOLLOW>
__device__ __forceinline__ bool apply_part(const ApplyArgs& a, uint32_t part, GenShared& sh, bool chained) {
  const uint32_t tid = threadIdx.x;
  const uint32_t bk = part >> a.sis_log, sub = part & ((1u << a.sis_log) - 1);
  const uint32_t g = part * PART + tid;
  const uint32_t fill0 = chained ? sh.l_fill : a.ev_counts[2 * part + 1];
  if (tid < FLAG_WORDS) {
    sh.l_flag[tid] = chained ? sh.l_next[tid] : a.pflag[(size_t)part * FLAG_WORDS + tid];
    sh.l_next[tid] = 0;
  }
  __syncthreads();
  uint32_t any = 0;
#pragma unroll
  for (uint32_t w = 0; w < FLAG_WORDS; ++w) any |= sh.l_flag[w];
  if (!any) return false;  // uniform
  const bool flagged = (sh.l_flag[tid >> 5] >> (tid & 31)) & 1u;

  if (tid == 0) sh.l_fill = fill0;  // append to the M chunk after the previous kernels' events
  if (tid <= ST_N) sh.l_stats[tid] = 0;

  Lane<NMAX, FOLLOW> L;
  L.S = a.S;
  L.E.chunk = a.ev + a.ev_off[2 * part + 1];
  L.E.fill = &sh.l_fill;
  L.g = g;
  L.won = 0;
  L.lost = 0;
  L.nev = 0;
  L.dirty = 0;
  L.prog = false;
  L.voted = false;
  L.meta = 0;
  L.last = 0;
  L.committed = 0;
  uint32_t resume = 0;
  uint64_t commit0 = 0;
  if (flagged) {  // live and not faulted when it was handed over
    L.meta = a.S.meta[g];
    L.load_group();
    resume = a.resume[g];
    commit0 = ((resume >> 30) & 1u) ? L.committed : a.commit0[g];
  }
  const uint64_t last0 = L.last;
  uint32_t st_msgs = 0, st_app = 0, st_vote = 0, st_drop = 0;
  const uint32_t skip = resume & 0x3FFFFFFFu;
  uint32_t j = 0;
  bool handed = false;  // (!FOLLOW) a follower-side message: the group goes on to the follower pass
  uint32_t hand_at = 0;
  const uint32_t lo = a.bk_off[bk], hi = a.bk_off[bk + 1];

  constexpr uint32_t KS = route_kmax(NMAX);
  const uint32_t cnt = flagged ? a.cnt[g] & CNT_MASK : 0u;
  const bool by_slot = flagged && cnt <= a.kmax;  // (a.kmax <= KS: the step's slot count)
  const bool by_walk = flagged && !by_slot;
  __syncthreads();  // l_fill
  // one message through the lane; false: handed on (k_apply only)
  auto step_one = [&](uint32_t inf, uint32_t morig, uint64_t mterm, uint64_t mindex, uint32_t ordinal) -> bool {
    const uint32_t type = inf & 0xF, from = (inf >> 4) & 0xF;
    const bool reject = (inf >> 8) & 1u;
    if (!FOLLOW && is_follower_type(type)) {
      handed = true;
      hand_at = ordinal;
      return false;
    }
    if (from >= L.n() && is_response(type)) {  // raft/multinode.go:235
      st_drop++;
      return true;
    }
    L.arrival = morig;
    L.voted = (inf & HB_INFO_VOTED) != 0;
    // RejectHint of a rejected MsgAppResp; m.LogTerm / the snapshot term of the follower side
    const bool wants_hint = (reject && type == HB_MSG_APP_RESP) || (FOLLOW && is_follower_type(type));
    L.step(type, from, mterm, mindex, reject, (wants_hint && a.hint) ? a.hint[morig] : 0ull);
    st_msgs++;
    st_app += type == HB_MSG_APP_RESP;
    st_vote += type == HB_MSG_VOTE_RESP;
    return true;
  };
  if (by_slot) {
    if (resume >> 31) {
      L.arrival = 0xFFFFFFFFu;
      L.step(HB_MSG_PROP, L.self(), 0, a.props[g], false, 0);
    }
    // arrival order of the slots: odd-even transposition over the arrival
    // indices, the slot numbers riding along as nibbles of `perm`
    uint32_t key[KS];
    uint32_t perm = 0;
#pragma unroll
    for (uint32_t k = 0; k < KS; ++k) {
      key[k] = k < cnt ? at32(a.slot, k * a.S.G + g).y : 0xFFFFFFFFu;
      perm |= k << (4 * k);
    }
#pragma unroll
    for (uint32_t r = 0; r < KS; ++r) {
#pragma unroll
      for (uint32_t k = (r & 1); k + 1 < KS; k += 2) {
        const uint32_t k0 = key[k], k1 = key[k + 1];
        const bool sw = k1 < k0;
        key[k] = sw ? k1 : k0;
        key[k + 1] = sw ? k0 : k1;
        const uint32_t p0 = (perm >> (4 * k)) & 0xF, p1 = (perm >> (4 * (k + 1))) & 0xF;
        const uint32_t swp = (perm & ~(0xFFu << (4 * k))) | (p1 << (4 * k)) | (p0 << (4 * (k + 1)));
        perm = sw ? swp : perm;
      }
    }
    // the next message's loads are issued before this one is stepped (one
    // rolled loop: Lane::step is inlined once per call site)
    uint32_t inf_n = 0, orig_n = 0;
    uint64_t term_n = 0, index_n = 0;
    if (cnt > skip)
      slot_unpack(at32(a.slot, ((perm >> (4 * skip)) & 0xF) * a.S.G + g), a.side, &inf_n, &orig_n, &term_n, &index_n);
#pragma nounroll
    for (uint32_t x = skip; x < cnt; ++x) {
      if (L.faulted()) break;
      const uint32_t inf = inf_n, morig = orig_n;
      const uint64_t mterm = term_n, mindex = index_n;
      if (x + 1 < cnt)
        slot_unpack(at32(a.slot, ((perm >> (4 * (x + 1))) & 0xF) * a.S.G + g), a.side, &inf_n, &orig_n, &term_n,
                    &index_n);
      if (!step_one(inf, morig, mterm, mindex, x)) break;
    }
  }

  auto on_total = [&](uint32_t) {
    __syncthreads();  // l_fill
    if (by_walk && (resume >> 31)) {
      L.arrival = 0xFFFFFFFFu;
      L.step(HB_MSG_PROP, L.self(), 0, a.props[g], false, 0);
    }
  };
  auto round = [&](uint32_t fill) {
    uint32_t my_start, my_cnt;
    gather_round(sh.sl, a, lo, fill, &my_start, &my_cnt, []() {});
    if (by_walk) {
      for (uint32_t x = 0; x < my_cnt; ++x, ++j) {
        if (j < skip || handed) continue;
        if (L.faulted()) break;
        const uint32_t i = sh.sl.perm[my_start + x];
        (void)step_one(sh.sl.info(i), sh.sl.orig(i), sh.sl.term(i), sh.sl.index(i), j);
      }
    }
    __syncthreads();
  };
  if (__syncthreads_or(by_walk)) walk_partition(sh.sl, a, lo, hi, sub, nullptr, on_total, round);

  if (flagged) L.store();
  if (handed) {  // the follower-side pass resumes the group at its follower-side message
    atomicOr(&sh.l_next[tid >> 5], 1u << (tid & 31));
    a.resume[g] = hand_at;
    a.commit0[g] = commit0;
  }
  const bool done = flagged && !handed;  // the group's batch ends in this kernel
  const uint64_t vals[ST_N + 1] = {st_msgs,
                                   st_app,
                                   st_vote,
                                   st_drop,
                                   (uint64_t)(done && L.committed != commit0),
                                   L.won,
                                   L.lost,
                                   (uint64_t)(done && L.faulted() != 0),
                                   L.last - last0,
                                   L.nev};
  reduce_stats(a, sh.l_stats, vals);  // (ends with a barrier: l_next and l_fill are final)
  if (tid == 0) a.ev_counts[2 * part + 1] = sh.l_fill;
  uint32_t nx = 0;
  if constexpr (!FOLLOW) {
#pragma unroll
    for (uint32_t w = 0; w < FLAG_WORDS; ++w) nx |= sh.l_next[w];
  }
  return nx != 0;
}

// k_apply runs over k_apply_fast's work lists, on the apply grid: workgroup w
// takes entry w / 8 of the list of XCD slot w % 8 (the slot of the workgroup
// that flagged the partition, so a bucket's sisters stay on one XCD; a list
// holds at most grid / 8 entries).  Partitions it hands on at a follower-side
// message (MsgApp / MsgHeartbeat / MsgSnap / MsgVote) go to k_follow's list.
#ifndef HB_FOLLOW_GRID
#define HB_FOLLOW_GRID 128
#endif
constexpr uint32_t FOLLOW_GRID = HB_FOLLOW_GRID;
// k_apply's grid: 0 = one workgroup per partition (each takes at most one list
// entry); else a persistent grid of that many (a multiple of 8).  Measured on
// MI355X: 512 saves ~1.5 us on an empty cfg2 step but cost 5-7 % on cfg3 /
// cfg4 while every partition was on the lists.  Since the leader lane
// (k_apply_lead) the n >= 5 lists are short, and the per-partition grid of a
// 256-VGPR, 31 KB-LDS kernel is itself ~40 us of dispatch (cfg3).
#ifndef HB_GEN_GRID
#define HB_GEN_GRID 1024
#endif
constexpr uint32_t GEN_GRID = HB_GEN_GRID;
#ifndef HB_GEN_GRID3
#define HB_GEN_GRID3 512  // n = 3 (cfg2 / cfg5: few partitions handed over): persistent, 2 per CU
#endif
constexpr uint32_t GEN_GRID3 = HB_GEN_GRID3;
static_assert(GEN_GRID % 8 == 0, "k_apply strides its XCD-slot lists by gridDim.x / 8");

// The step's finish (as k_finish), run by the last k_follow workgroup: the
// statistics shards (agent-scope atomics of every apply kernel) summed into
// stats (+ accum), the shards and the work lists cleared for the next step.
static_assert((ST_N + 1) * NSH <= PART && (NSH & (NSH - 1)) == 0, "a finish lane per (value, shard)");
__device__ __forceinline__ void finish_step(const ApplyArgs& a) {
  const int map[ST_N + 1] = {HB_STAT_MSGS,  HB_STAT_APPRESP, HB_STAT_VOTERESP, HB_STAT_DROPPED, HB_STAT_COMMITS,
                             HB_STAT_WON,   HB_STAT_LOST,    HB_STAT_FAULTS,   HB_STAT_ENTRIES, HB_STAT_EVENTS};
  // one lane per (value, shard): one round trip; the NSH lanes of a value are adjacent in a wave
  const uint32_t t = threadIdx.x, k = t / NSH;
  uint64_t v = 0;
  if (k <= ST_N) {
    v = __hip_atomic_load(&a.stats_shard[shard_at(k, t % NSH)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.stats_shard[shard_at(k, t % NSH)], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (uint32_t d = 1; d < NSH; d <<= 1) v += __shfl_xor(v, d);
  if (k <= ST_N && t % NSH == 0) {
    a.stats[map[k]] = v;
    if (a.accum) a.accum[map[k]] += v;
  }
}

// The workgroups that finish the step take tickets; the step's finish runs
// in the last.  Only workgroups that had work take one (`working` of them, a
// count every workgroup derives from the work-list lengths): a ticket per
// workgroup of the grid serialises hundreds of atomics on one word (~11 ns
// each).  With no work anywhere, workgroup 0 finishes at once.  (The
// work-list counters and the ticket word belong to the prep set and are
// cleared by the next prep that reuses it, never by a workgroup still
// reading them.)
__device__ __forceinline__ void finish_by_ticket(const ApplyArgs& a, bool worked, uint32_t working,
                                                 uint32_t* l_last) {
  if (working == 0) {
    if (blockIdx.x == 0) finish_step(a);  // uniform
    return;
  }
  if (!worked) return;  // uniform
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this workgroup's stats atomics are performed
  __syncthreads();
  if (threadIdx.x == 0)
    *l_last = __hip_atomic_fetch_add(a.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == working - 1;
  __syncthreads();
  if (*l_last) finish_step(a);  // uniform
}

// CHAIN (n = 3): the follower-side pass runs chained in the same workgroup
// and k_apply's last workgroup runs the step's finish — no k_follow launch
// (n = 3's general kernel does not spill either way; at n >= 5 the follower
// lane's registers stay out of the hot general kernel).
template <int NMAX>
__global__ void __launch_bounds__(PART, HB_GEN_WAVES) k_apply(ApplyArgs a) {
  constexpr bool CHAIN = NMAX <= 3;
  __shared__ GenShared sh;
  __shared__ uint32_t l_last;
  // persistent over the list of its XCD slot when the grid is smaller than
  // the partitions (HB_GEN_GRID)
  const uint32_t xs = blockIdx.x & 7, stride = gridDim.x >> 3;
  uint32_t nl = 0, working = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    const uint32_t c = __hip_atomic_load(&a.ap_cnt[k * CTR_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nl = k == xs ? c : nl;
    working += c < stride ? c : stride;  // workgroups of slot k with at least one entry
  }
  for (uint32_t i = blockIdx.x >> 3; i < nl; i += stride) {  // uniform
    const uint32_t part = a.ap_list[(size_t)xs * a.NB + i];
    if (apply_part<NMAX, false>(a, part, sh, false)) {  // uniform: the partition goes on to the follower pass
      if constexpr (CHAIN) {
        __syncthreads();
        (void)apply_part<NMAX, true>(a, part, sh, true);
      } else {
        if (threadIdx.x < FLAG_WORDS) a.pflag[(size_t)part * FLAG_WORDS + threadIdx.x] = sh.l_next[threadIdx.x];
        if (threadIdx.x == 0) a.fl_list[atomicAdd(a.fl_cnt, 1u)] = part;
      }
    }
    __syncthreads();  // sh is reused by the next partition
  }
  if constexpr (CHAIN) finish_by_ticket(a, (blockIdx.x >> 3) < nl, working, &l_last);
}

// k_elect: the election lane (hipbatch_elect.h) over k_apply_fast's work
// lists, before k_apply (n >= 5, unsized logs): a handed-over group whose
// messages all sit in its route slots is stepped by ElectLane as far as it
// takes them; a group it finishes leaves the partition's flags, a group it
// hands over resumes in k_apply at the first message it did not take.
#ifndef HB_ELECT_WAVES
#define HB_ELECT_WAVES 4
#endif
#ifndef HB_ELECT_GRID  // persistent over the XCD-slot lists (cfg4 -9 to -11 us, cfg3 -3 to -6 us vs one
#define HB_ELECT_GRID 1024  // workgroup per partition: an empty or short list launched 16K workgroups)
#endif
constexpr uint32_t ELECT_GRID = HB_ELECT_GRID;
static_assert(ELECT_GRID % 8 == 0, "k_elect strides its XCD-slot lists by gridDim.x / 8");

template <int NMAX>
__global__ void __launch_bounds__(PART, HB_ELECT_WAVES) k_elect(ApplyArgs a) {
  constexpr uint32_t KS = route_kmax(NMAX);
  __shared__ uint32_t l_fill;
  __shared__ uint32_t l_flag[FLAG_WORDS];
  __shared__ uint32_t l_eflag[FLAG_WORDS];
  __shared__ uint64_t l_stats[ST_N + 1];
  // each lane's route slots, read once: the arrival keys come from them and the
  // messages are then read back in arrival order (reading the keys from HBM and
  // the slots again fetched every slot line twice: 16-byte slots, 4-byte keys)
  __shared__ uint4 l_slot[KS][PART];
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x & 7, stride = gridDim.x >> 3;
  const uint32_t nl = __hip_atomic_load(&a.el_cnt[xs * CTR_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the partition list two ahead and the next partition's flags and event fill
  // are fetched during this partition's work (two round trips off each turn:
  // cfg4 1.741-1.762 -> 1.734-1.742 ms)
  const uint32_t* list = a.el_list + (size_t)xs * a.NB;
  uint32_t i = blockIdx.x >> 3;
  uint32_t part = i < nl ? list[i] : 0u;
  uint32_t nxt = i + stride < nl ? list[i + stride] : 0u;
  uint32_t pf = 0, pe = 0, pfill = 0;
  if (i < nl) {
    if (tid < FLAG_WORDS) {
      pf = a.pflag[(size_t)part * FLAG_WORDS + tid];
      pe = a.eflag[(size_t)part * FLAG_WORDS + tid];
    }
    if (tid == 0) pfill = a.ev_counts[2 * part + 1];
  }
  for (; i < nl; i += stride) {  // uniform
    const uint32_t g = part * PART + tid;
    if (tid < FLAG_WORDS) {
      l_flag[tid] = pf;
      l_eflag[tid] = pe;
    }
    if (tid == 0) l_fill = pfill;  // after k_apply_fast's events
    if (tid <= ST_N) l_stats[tid] = 0;
    __syncthreads();
    const bool flagged = (l_eflag[tid >> 5] >> (tid & 31)) & 1u;  // (a subset of the k_apply flags)
    ElectLane<NMAX> L;
    L.S = a.S;
    L.E.chunk = a.ev + a.ev_off[2 * part + 1];
    L.E.fill = &l_fill;
    L.g = g;
    L.meta = flagged ? a.S.meta[g] : 0ull;
    const uint32_t cnt = flagged ? a.cnt[g] & CNT_MASK : 0u;
    const uint32_t resume = flagged ? a.resume[g] : 0u;
    // (flagged groups are live and not faulted; a pending dense proposal goes to k_apply)
    const bool mine = flagged && cnt <= KS && (resume >> 31) == 0 && L.self() < L.n() && !(L.meta & M_NC);
    uint32_t st_msgs = 0, st_app = 0, st_vote = 0, st_drop = 0;
    bool done = false;
    uint64_t last0 = 0, commit0 = 0;
    L.won = L.lost = L.nev = 0;
    L.committed = L.last = 0;
    uint32_t key[KS];  // the slots' arrival keys (0xFFFFFFFF past cnt)
    // every load of a flagged lane in the round trip of meta / cnt / resume: the
    // state, commit0 and all KS slots (those past cnt are masked here); loading
    // only a lane that is `mine`, after that test, measured cfg4 1.813-1.815 vs
    // 1.763-1.765 ms
    uint64_t c0 = 0;
    if (flagged) {
      L.load();
      c0 = a.commit0[g];
      uint4 sl[KS];
#pragma unroll
      for (uint32_t k = 0; k < KS; ++k) sl[k] = at32(a.slot, k * a.S.G + g);
#pragma unroll
      for (uint32_t k = 0; k < KS; ++k) {
        const uint4 r = k < cnt ? sl[k] : make_uint4(0, 0xFFFFFFFFu, 0, 0);
        l_slot[k][tid] = r;
        key[k] = r.y;
      }
    }
    const uint32_t nn = i + 2 * stride < nl ? list[i + 2 * stride] : 0u;
    if (i + stride < nl) {
      if (tid < FLAG_WORDS) {
        pf = a.pflag[(size_t)nxt * FLAG_WORDS + tid];
        pe = a.eflag[(size_t)nxt * FLAG_WORDS + tid];
      }
      if (tid == 0) pfill = a.ev_counts[2 * nxt + 1];
    }
    if (mine) {
      last0 = L.last;
      commit0 = ((resume >> 30) & 1u) ? L.committed : c0;
      // arrival order of the slots (odd-even transposition, slot numbers as nibbles)
      const uint32_t perm = arrival_perm<KS>(key);
      const uint32_t skip = resume & 0x3FFFFFFFu;
      uint32_t x = skip;
#pragma nounroll
      for (; x < cnt; ++x) {
        uint32_t inf, org;  // (from the lane's LDS copy)
        uint64_t mterm, ix;
        slot_unpack(l_slot[(perm >> (4 * x)) & 0xF][tid], a.side, &inf, &org, &mterm, &ix);
        const uint32_t type = inf & 0xF, from = (inf >> 4) & 0xF;
        if (from >= L.n() && is_response(type)) {  // raft/multinode.go:235
          st_drop++;
          continue;
        }
        if (!L.takes(type, from, mterm)) break;
        L.step(type, from, mterm, (inf >> 8) & 1u);
        st_msgs++;
        st_app += type == HB_MSG_APP_RESP;
        st_vote += type == HB_MSG_VOTE_RESP;
      }
      if (x > skip) {
        L.store();
        if (x == cnt) {
          done = true;  // the group's batch ends here
        } else {  // k_apply resumes at message x, loading what was stored
          a.resume[g] = x;
          a.commit0[g] = commit0;
        }
      }
    }
    flag_put<false>(l_flag, tid, done);
    const uint64_t vals[ST_N + 1] = {st_msgs,
                                     st_app,
                                     st_vote,
                                     st_drop,
                                     (uint64_t)(done && L.committed != commit0),
                                     L.won,
                                     L.lost,
                                     0,
                                     mine ? L.last - last0 : 0ull,
                                     L.nev};
    reduce_stats(a, l_stats, vals);  // (ends with a barrier: l_flag and l_fill are final)
    if (tid < FLAG_WORDS) a.pflag[(size_t)part * FLAG_WORDS + tid] = l_flag[tid];
    if (tid == 0) a.ev_counts[2 * part + 1] = l_fill;
    __syncthreads();  // the next partition reuses the LDS
    part = nxt;
    nxt = nn;
  }
}

#ifndef HB_LEAD_XWAVES  // k_apply_lead<5> in X mode (LDS: 4 staged slots + the lane rows = 36 KB)
#define HB_LEAD_XWAVES 4
#endif
#ifndef HB_LEAD_WAVES
#define HB_LEAD_WAVES 3  // (n = 5: 125 VGPRs, 53 KB of LDS: 3 workgroups per CU)
#endif

#ifndef HB_LEAD7_WAVES  // k_apply_lead<7> (measured on cfg4: 2 waves +3 %, 4 waves -0.6 % with 128 B/lane of scratch)
#define HB_LEAD7_WAVES 3
#endif
// ---------------------------------------------------------------------------
// k_apply_lead (n >= 5, replaces k_apply_fast there): one workgroup per
// partition, one lane per group, the leader lane (hipbatch_lead.h) for every
// leader whose messages all sit in its route slots: the dense proposal, then
// the slot messages in arrival order as far as LeadLane::takes allows — every
// response a leader steps at its own term.  One load and one store of the
// group's state for the whole batch.  What it cannot take is handed over as
// k_apply_fast does (resume word, pflag; eflag for k_elect: a group that is no
// leader, or a leader stopped by a higher-term message).  Which groups it loads
// and which it hands over unloaded is handover_class's rule.
// ---------------------------------------------------------------------------
// X mode (follower-side batches): a follower whose messages all sit in its
// first FOLLOW_SLOTS route slots is stepped by FollowLane in the same pass
// (the follower side of a node with n >= 5 replicas: about (n-1)/n of its
// groups), the slots' {m.LogTerm, m.Commit} extensions staged beside them.
constexpr uint32_t FOLLOW_SLOTS = 4;
// Leaders' Match / Next in LDS (LeadLaneL, n = 5) or in registers (LeadLane,
// n = 7: 28 KB of {Match, Next} leave 2 workgroups per CU, cfg4 2.018 vs 1.918 ms)
template <int NMAX> struct LeadOf {
  static constexpr bool LDS = NMAX <= 5;
  using T = typename std::conditional<LDS, LeadLaneL<NMAX>, LeadLane<NMAX>>::type;
};
template <int NMAX, bool X>
__global__ void __launch_bounds__(PART, NMAX <= 5 ? (X ? HB_LEAD_XWAVES : HB_LEAD_WAVES)
                                                 : HB_LEAD7_WAVES) k_apply_lead(ApplyArgs a) {
  constexpr uint32_t KS = route_kmax(NMAX);
  constexpr uint32_t FS = X ? FOLLOW_SLOTS : 1u;
  constexpr bool LDS = LeadOf<NMAX>::LDS;
  __shared__ uint32_t l_fill, l_pfill;
  __shared__ uint32_t l_flag[FLAG_WORDS];
  __shared__ uint32_t l_eflag[FLAG_WORDS];
  __shared__ uint64_t l_stats[ST_N + 1];
  // the lane's route slots, read once (as in k_elect).  X mode stages only the
  // first FS (a follower's; a leader reads the rest from HBM), so that the
  // kernel fits 4 workgroups per CU
  constexpr uint32_t SR = X ? FS : KS;
  __shared__ uint4 l_slot[SR][PART];
  // per lane, one 16-byte word per slot: a leader's {Match, Next} (LeadLaneL) or,
  // X mode, a follower's slot extensions {m.LogTerm, m.Commit} — a lane is one or the other
  constexpr uint32_t LW = LDS ? (NMAX > FS ? NMAX : FS) : (X ? FS : 1u);
  __shared__ uint4 l_lane[LW][(LDS || X) ? PART : 1];
  const uint32_t part = block_part(a.sis_log);
  if (part >= a.NB) return;  // uniform: grid padding
  if (!X && a.storm && a.lskip[part]) return;  // uniform: the route closed it (storm hand-over)
  const uint32_t tid = threadIdx.x;
  const uint32_t g = part * PART + tid;
  const bool gvalid = g < a.S.G;
  auto slot_at = [&](uint32_t k) -> uint4 {
    if constexpr (SR < KS) return k < SR ? l_slot[k < SR ? k : 0][threadIdx.x] : at32(a.slot, k * a.S.G + g);
    else return l_slot[k][threadIdx.x];
  };
  if (tid == 0) l_fill = l_pfill = 0;
  if (tid <= ST_N) l_stats[tid] = 0;
  if (tid < FLAG_WORDS) l_flag[tid] = l_eflag[tid] = 0;

  FollowLane<NMAX, typename LeadOf<NMAX>::T> L;
  L.S = a.S;
  L.g = g;
  if constexpr (LDS) L.lp = &l_lane[0][tid];
  L.mlo = gvalid ? reinterpret_cast<const uint32_t*>(a.S.meta)[2 * (size_t)g] : 0u;
  const uint32_t prop_raw = (a.props && gvalid) ? a.props[g] : 0u;
  const uint32_t craw = gvalid ? a.cnt[g] : 0u, cnt = craw & CNT_MASK;
  // X mode (a MultiNode node's batch: it leads some groups and follows most):
  // the per-group fields every role steps with come in meta's round trip
  L.last = L.committed = 0;
  L.term = 0;
  if (X && gvalid) L.load_state_head();
  const bool live = gvalid && L.n() != 0 && L.faulted() == 0;
  const bool leader = live && L.state() == HB_STATE_LEADER;
  const bool fits = cnt <= KS;  // every message of the group is in its slots
  // r.Commit = 0 (M_NC): the general lane steps the group's first message
  const bool nc = (L.mlo & (uint32_t)M_NC) != 0;
  // X mode: a follower whose messages all sit in its first FS slots, without a
  // dense proposal (stepFollower forwards it: the general lane)
  const bool fol = X && live && !nc && L.state() == HB_STATE_FOLLOWER && cnt > 0 && cnt <= FS && prop_raw == 0;
  L.dirty = 0;
  L.nev = 0;
  // (without X, loading the state beside meta, as k_apply_fast does, measured
  // neutral on cfg3 and +4.5 % on cfg4, whose lanes are mostly not leaders)
  // What to do with the group before its first message is handover_class, the
  // rule k_route closes partitions by (an election storm's leader is handed
  // over without reading its slots or its state).  This kernel's own cases,
  // which the route never closes: a follower of X mode (fol), and a leader
  // with a dense proposal, which is loaded whatever its messages.
  const uint32_t cls = handover_class(L.mlo, cnt, (craw & CNT_HIGHER) != 0, (uint32_t)NMAX, KS);
  const bool loaded = prop_raw != 0 ? (leader && !nc) : cls == HO_LOAD;
  const bool slots = (loaded && fits) || fol;
#pragma unroll
  for (uint32_t k = 0; k < SR; ++k)
    if (slots && k < cnt) l_slot[k][tid] = at32(a.slot, k * a.S.G + g);
  if constexpr (X) {
#pragma unroll
    for (uint32_t k = 0; k < FS; ++k)
      if (fol && k < cnt) l_lane[k][tid] = at32(a.slotx, k * a.S.G + g);
  }
  if (loaded) L.load(X);
  if (fol) L.load_follow();  // (a follower reads no Progress)
  // k_elect's, if handed over: no leader, or a leader a higher term steps down
  bool elect = prop_raw != 0 ? !leader : cls == HO_ELECT;
  // the slots' arrival indices, only for a group this kernel steps
  uint32_t key[KS];
#pragma unroll
  for (uint32_t k = 0; k < KS; ++k) key[k] = (slots && k < cnt) ? slot_at(k).y : 0xFFFFFFFFu;
  // arrival order of the slots (slot numbers as nibbles)
  const uint32_t perm = arrival_perm<KS>(key);
  const uint64_t last0 = L.last, commit0 = L.committed;
  bool flagged = false;
  uint32_t resume = 0;
  uint32_t st_msgs = 0, st_app = 0, st_vote = 0, st_drop = 0;

  // ---- the dense proposal: the partition's P chunk (fixed slot), before any message event
  const uint64_t poff = (uint64_t)part * PART * a.ev_per_msg;
  if (tid == 0) a.ev_off[2 * part] = poff;
  L.E.chunk = a.ev + poff;
  L.E.fill = &l_pfill;
  const uint32_t prop_k = live ? prop_raw : 0u;
  if (prop_k) {
    if (loaded && L.prop_ok(prop_k)) {
      L.arrival = 0xFFFFFFFFu;
      L.prop(prop_k);
    } else {
      flagged = true;
      resume = 1u << 31;  // the proposal itself is pending (stepped by k_apply into the M chunk)
    }
  }
  // ---- the slot messages in arrival order (M chunk reserved by k_route)
  L.E.chunk = a.ev + a.ev_off[2 * part + 1];
  L.E.fill = &l_fill;
  bool fstepped = false;  // FollowLane stepped a message: its state is stored
  if (X && fol) {
#pragma nounroll
    for (uint32_t x = 0; x < cnt; ++x) {
      if (L.faulted()) break;
      const uint32_t ks = (perm >> (4 * x)) & 0xF;
      uint32_t inf, morig;
      uint64_t mterm, mindex;
      slot_unpack(slot_at(ks), a.side, &inf, &morig, &mterm, &mindex);
      const uint4 ext = l_lane[ks < FS ? ks : 0][(LDS || X) ? tid : 0];
      const uint64_t lt = (uint64_t)ext.x | ((uint64_t)ext.y << 32), mc = (uint64_t)ext.z | ((uint64_t)ext.w << 32);
      const uint32_t from = (inf >> 4) & 0xF;
      if (!L.takes_follow(inf, from, mterm, mindex, lt, mc)) {
        flagged = true;
        resume = x;
        break;
      }
      L.arrival = morig;
      L.step_follow(inf, from, mterm, mindex, lt, mc);
      fstepped = true;
      st_msgs++;
    }
  } else if (live && cnt > 0 && !flagged && !L.faulted()) {
    if (!loaded || !fits) {  // all to k_apply (or k_elect)
      flagged = true;
      resume = 0;
    } else {
      uint32_t x = 0;
      uint4 nx = slot_at(perm & 0xF);  // (the next slot's load runs ahead of this step)
#pragma nounroll
      for (; x < cnt; ++x) {
        if (L.faulted()) break;
        uint32_t inf, morig;
        uint64_t mterm, mindex;
        const uint4 cur = nx;
        if (x + 1 < cnt) nx = slot_at((perm >> (4 * (x + 1))) & 0xF);
        slot_unpack(cur, a.side, &inf, &morig, &mterm, &mindex);
        const uint32_t type = inf & 0xF, from = (inf >> 4) & 0xF;
        const bool reject = (inf >> 8) & 1u;
        if (from >= L.n() && is_response(type)) {  // raft/multinode.go:235
          st_drop++;
          continue;
        }
        if (!L.takes(type, from, mterm)) {
          flagged = true;
          resume = x;
          elect = mterm > L.term;
          break;
        }
        L.arrival = morig;
        L.step(type, from, mterm, mindex, reject,
               (reject && type == HB_MSG_APP_RESP && a.hint) ? a.hint[morig] : 0ull);
        st_msgs++;
        st_app += type == HB_MSG_APP_RESP;
        st_vote += type == HB_MSG_VOTE_RESP;
      }
    }
  }
  if (loaded) L.store();
  if (fstepped) L.store_follow();
  const bool stored = loaded || fstepped;
  if constexpr (NMAX >= 5) flag_put<true>(l_eflag, tid, flagged && elect);  // k_elect's candidates
  flag_put<true>(l_flag, tid, flagged);
  if (flagged) {
    a.resume[g] = resume | (stored ? 0u : 1u << 30);
    if (stored) a.commit0[g] = commit0;
  }
  const uint32_t vals[ST_N + 1] = {st_msgs,
                                   st_app,
                                   st_vote,
                                   st_drop,
                                   (uint32_t)(!flagged && L.committed != commit0),
                                   0,
                                   0,
                                   (uint32_t)(L.faulted() != 0 && live),
                                   (uint32_t)(L.last - last0),
                                   L.nev};
  reduce_stats(a, l_stats, vals);
  if (tid < FLAG_WORDS) {
    a.pflag[(size_t)part * FLAG_WORDS + tid] = l_flag[tid];
    if (NMAX >= 5) a.eflag[(size_t)part * FLAG_WORDS + tid] = l_eflag[tid];
  }
  if (tid == 0) fast_close(a, part, l_flag, NMAX >= 5 ? l_eflag : nullptr, l_pfill, l_fill);
}

// k_follow: the follower-capable lane (Lane<NMAX, true>) for the groups
// k_apply handed on at a follower-side message, over k_apply's work list (its
// registers and code stay out of k_apply, the hot general kernel of cfg3 /
// cfg4).  Its last workgroup out runs the step's finish: the statistics are
// agent-scope atomics, performed at the memory side, so each workgroup waits
// for its own (vmcnt(0)) before taking a ticket, and the last reads the shards
// with agent-scope loads.
template <int NMAX>
__global__ void __launch_bounds__(PART, HB_GEN_WAVES) k_follow(ApplyArgs a) {
  __shared__ GenShared sh;
  __shared__ uint32_t l_last;
  const uint32_t nl = __hip_atomic_load(a.fl_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t i = blockIdx.x; i < nl; i += gridDim.x) {
    (void)apply_part<NMAX, true>(a, a.fl_list[i], sh, false);
    __syncthreads();
  }
  finish_by_ticket(a, blockIdx.x < nl, nl < gridDim.x ? nl : gridDim.x, &l_last);
}

// ---------------------------------------------------------------------------
// k_tick: one MultiNode.Tick (raft/multinode.go:264-275) — every live group
// runs tickHeartbeat (leader) or tickElection (raft/raft.go:362-382), the
// draw of isElectionTimeout (:765-771) read from the node's r.rand stream at
// the group's own position; a leader's due MsgBeat sends its heartbeats from
// Match / pm alone, a due MsgHup is stepped at once by the general state
// machine.  Events go to the partition's P chunk (at most one
// step per group, so the chunk's ev_per_msg x PART words bound them).
// ---------------------------------------------------------------------------
template <int NMAX>
__global__ void __launch_bounds__(PART, 2) k_tick(ApplyArgs a) {
  __shared__ uint32_t l_fill;
  __shared__ uint64_t l_stats[ST_N + 1];
  const uint32_t part = block_part(a.sis_log);
  if (part >= a.NB) return;  // uniform: grid padding
  const uint32_t tid = threadIdx.x;
  const uint32_t g = part * PART + tid;
  if (tid == 0) l_fill = 0;
  if (tid <= ST_N) l_stats[tid] = 0;
  __syncthreads();

  const uint64_t poff = (uint64_t)part * PART * a.ev_per_msg;
  Lane<NMAX> L;
  L.S = a.S;
  L.E.chunk = a.ev + poff;
  L.E.fill = &l_fill;
  L.g = g;
  L.won = 0;
  L.lost = 0;
  L.nev = 0;
  L.dirty = 0;
  L.meta = 0;
  L.last = 0;
  L.committed = 0;
  L.arrival = 0xFFFFFFFFu;
  uint32_t type = 0xFF;
  bool live = false;
  // meta's low word (state, n, self, flags) decides a tick; the high word (the
  // vote tally) is read only by a group that steps or faults (4 B per group)
  const uint32_t* meta32 = reinterpret_cast<const uint32_t*>(a.S.meta);
  auto meta_hi = [&]() { L.meta |= (uint64_t)at32(meta32, 2 * g + 1) << 32; };
  if (g < a.S.G) {
    L.meta = at32(meta32, 2 * g);
    live = L.n() != 0 && !L.faulted();
  }
  if (live) {
    const uint32_t cfg = a.S.tcfg[g];
    const uint32_t et = cfg & 0xFFFFu, ht = cfg >> 16;
    uint32_t el = a.S.elapsed[g];
    if (L.state() == HB_STATE_LEADER) {  // tickHeartbeat
      if (++el >= ht) {
        el = 0;
        type = HB_MSG_BEAT;
      }
    } else if (L.self() == HB_SLOT_NONE) {  // tickElection: !promotable()
      el = 0;
    } else if (++el >= et) {  // isElectionTimeout: d = elapsed - et >= 0 takes a draw
      const uint32_t pos = a.S.rpos[g];
      if (pos >= a.S.nrnd) {
        meta_hi();
        L.fault(HB_FAULT_RAND_EXHAUSTED);
        L.dirty |= D_META;
        L.ev(HB_EV_FAULT, 0, HB_FAULT_RAND_EXHAUSTED, HB_NO_INDEX);
      } else {
        a.S.rpos[g] = pos + 1;
        if ((uint64_t)(el - et) > a.S.rnd[pos] % et) {
          el = 0;
          type = HB_MSG_HUP;
        }
      }
    }
    a.S.elapsed[g] = el;
  }
  uint64_t last0 = 0, commit0 = 0;
  if (type == HB_MSG_BEAT && !(L.meta & (M_RS | M_NC))) {
    // stepLeader MsgBeat -> bcastHeartbeat (raft/raft.go:495-498, :290-300):
    // a MsgHeartbeat to every peer in slot order at min(Match, committed), each
    // Progress resumed.  Only those fields are read and only a cleared pause bit
    // is written (Lane::step would load the whole group, ring heads included,
    // and write every peer's Progress back unchanged).  The self slot, whose
    // arrays may be stale under M_SM, is skipped; Next, which may be stale under
    // M_NX, is not read.
    const uint64_t committed = a.S.commit[g];
    const uint32_t nn = L.n(), sf = L.self();
    uint64_t mt[NMAX];
    uint32_t pmv[NMAX];
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      const bool on = (uint32_t)s < nn && (uint32_t)s != sf;
      mt[s] = on ? a.S.match[(size_t)s * a.S.G + g] : 0ull;
      pmv[s] = on ? a.S.pm[(size_t)s * a.S.G + g] : 0u;
    }
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      if ((uint32_t)s >= nn || (uint32_t)s == sf) continue;
      L.ev(HB_EV_HEARTBEAT, s, 0, umin64(mt[s], committed));
      if (pmv[s] & PM_PAUSED) a.S.pm[(size_t)s * a.S.G + g] = pmv[s] & ~PM_PAUSED;
    }
  } else if (type == HB_MSG_HUP && !sz_on(a.S.max_msg_size) && !(L.meta & M_NC) && L.self() < L.n()) {
    // a non-leader's election timeout: campaign through the election lane
    // (hipbatch_elect.h, as k_elect steps it), which leaves the n Progress
    // entries in the reset form (M_RS) instead of writing them — ~4 % of the
    // groups campaign per tick, each writing n x 20 scattered bytes through
    // the general lane (the tick's 2.3 x traffic over its byte model, r05)
    meta_hi();
    ElectLane<NMAX> E;
    E.S = a.S;
    E.E = L.E;
    E.g = g;
    E.meta = L.meta;
    E.load();
    last0 = E.last;
    commit0 = E.committed;
    E.step(HB_MSG_HUP, L.self(), 0, false);
    E.store();
    L.meta = E.meta;
    L.last = E.last;
    L.committed = E.committed;
    L.won = E.won;
    L.lost = E.lost;
    L.nev = E.nev;
    L.dirty = 0;  // (stored)
  } else if (type != 0xFF) {  // MsgHup (or the MsgBeat of a reset-form / M_NC leader): the general state machine
    meta_hi();
    L.load_all();
    last0 = L.last;
    commit0 = L.committed;
    L.step(type, L.self(), 0, 0, false, 0);
  }
  if (live && L.dirty) {
    if (type == 0xFF) L.S.meta[g] = L.meta;  // the fault only
    else L.store();
  }
  const bool stepped = type != 0xFF;
  const uint64_t vals[ST_N + 1] = {(uint64_t)stepped,
                                   0,
                                   0,
                                   0,
                                   (uint64_t)(stepped && L.committed != commit0),
                                   L.won,
                                   L.lost,
                                   (uint64_t)(live && L.faulted() != 0),
                                   stepped ? L.last - last0 : 0ull,
                                   L.nev};
  reduce_stats(a, l_stats, vals);
  if (tid == 0) {
    a.ev_off[2 * part] = poff;
    a.ev_off[2 * part + 1] = poff;
    a.ev_counts[2 * part] = l_fill;
    a.ev_counts[2 * part + 1] = 0;
  }
}

// ---------------------------------------------------------------------------
// k_decode: wire ingestion (hb_decode).  One lane per record: Message.Unmarshal
// (hipbatch_wire.h), multiNode.Step's local-message filter (raft/multinode.go:
// 432-439), m.From -> slot through the group's peer ids, one batch record out.
// ---------------------------------------------------------------------------
struct DecodeArgs {
  const uint8_t* bytes;
  const uint64_t* off;
  const uint32_t* len;
  const uint32_t* group;
  uint64_t n;
  const uint64_t* meta;
  const uint4* peer;  // [G] rows of HB_PEER_ROW node ids (64 B), or null
  uint32_t G, nmax;
  uint32_t* o_group;
  uint32_t* o_info;
  uint64_t* o_term;
  uint64_t* o_index;
  uint64_t* o_hint;
  uint8_t* status;
};

constexpr uint32_t HB_PEER_ROW = 8;  // u64 per group peer row: node ids of slots 0..6, then n

// Outcome of one record -> batch record + status (shared by both passes).
__device__ __forceinline__ void dec_emit(const DecodeArgs& a, uint64_t k, int rc, const WireMsg& m, uint32_t g, bool gok,
                                         const uint64_t* ids) {
  uint32_t st;
  if (rc == W_ERR) st = HB_WIRE_ERROR;
  else if (rc == W_PANIC) st = HB_WIRE_PANIC;
  else if (rc == W_DEEP) st = HB_WIRE_HOST;
  else if (m.type == HB_MSG_HUP || m.type == HB_MSG_BEAT || m.type == HB_MSG_UNREACHABLE ||
           m.type == HB_MSG_SNAP_STATUS)
    st = HB_WIRE_LOCAL;  // IsLocalMsg raft/util.go:49-51
  else if (m.type != HB_MSG_APP_RESP && m.type != HB_MSG_VOTE_RESP && m.type != HB_MSG_HEARTBEAT_RESP)
    st = HB_WIRE_HOST;
  else if (!gok) st = HB_WIRE_BADGROUP;
  else st = HB_WIRE_OK;
  uint32_t slot = HB_SLOT_NONE;
  if (st == HB_WIRE_OK && a.peer && m.from != 0) {
    const uint32_t nn = (uint32_t)ids[HB_PEER_ROW - 1];
#pragma unroll
    for (uint32_t s = 0; s < HB_MAX_REPLICAS; ++s)
      if (s < nn && slot == HB_SLOT_NONE && ids[s] == m.from) slot = s;
  }
  const bool ok = st == HB_WIRE_OK;
  a.o_group[k] = ok ? g : 0xFFFFFFFFu;
  a.o_info[k] = ok ? ((uint32_t)m.type | (slot << 4) | ((uint32_t)m.reject << 8)) : 0u;
  a.o_term[k] = ok ? m.term : 0ull;
  a.o_index[k] = ok ? m.index : 0ull;
  a.o_hint[k] = ok ? m.hint : 0ull;
  a.status[k] = (uint8_t)st;
}

// Pass 1 (k_decode): a wave's 64 records are contiguous in the usual layout,
// so the wave copies their span into its own LDS window with coalesced
// 16-byte loads (bytes at the unaligned ends one by one, so nothing outside
// the span is read) and each lane runs the straight-line MarshalTo-shape
// parser (w_fast_message) from LDS.  A record of any other shape (or a wave
// whose span does not fit the window) is queued for pass 2, k_decode_general,
// which runs the full Message.Unmarshal restatement over the queue only: its
// register and scratch footprint never limits the occupancy of pass 1.
constexpr uint32_t DEC_THREADS = 256;
constexpr uint32_t DEC_WIN = 4096;  // bytes of records staged per wave
constexpr uint32_t DEC_GEN_BLOCKS = 128;  // pass 2 is the exception path; scratch-heavy waves are costly to launch
__global__ void __launch_bounds__(DEC_THREADS) k_decode(DecodeArgs a, uint32_t* q, uint32_t* qn) {
  __shared__ uint4 l_win[DEC_THREADS / 64][DEC_WIN / 16 + 2];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t k = (uint64_t)blockIdx.x * DEC_THREADS + threadIdx.x;
  const bool live = k < a.n;
  const uint64_t o = live ? a.off[k] : 0ull;
  const uint32_t len = live ? a.len[k] : 0u;
  uint64_t lo = live ? o : ~0ull, hi = live ? o + len : 0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const bool fits = hi > lo && hi - lo <= DEC_WIN;  // uniform in the wave
  uint8_t* win = reinterpret_cast<uint8_t*>(&l_win[wave][0]);
  const uintptr_t A = reinterpret_cast<uintptr_t>(a.bytes) + lo, B = reinterpret_cast<uintptr_t>(a.bytes) + hi;
  const uintptr_t base = A & ~(uintptr_t)15;
  if (fits) {
    const uintptr_t A16 = (A + 15) & ~(uintptr_t)15, B16 = B & ~(uintptr_t)15;
    if (A16 < B16) {
      const uint32_t nc = (uint32_t)((B16 - A16) >> 4), c0 = (uint32_t)((A16 - base) >> 4);
      for (uint32_t c = lane; c < nc; c += 64) l_win[wave][c0 + c] = reinterpret_cast<const uint4*>(A16)[c];
      for (uintptr_t x = A + lane; x < A16; x += 64) win[x - base] = *reinterpret_cast<const uint8_t*>(x);
      for (uintptr_t x = B16 + lane; x < B; x += 64) win[x - base] = *reinterpret_cast<const uint8_t*>(x);
    } else {
      for (uintptr_t x = A + lane; x < B; x += 64) win[x - base] = *reinterpret_cast<const uint8_t*>(x);
    }
  }
  __syncthreads();
  if (!live) return;
  // the group's peer row and meta are random gathers: issue them before the
  // parse so their latency hides behind it
  const uint32_t g = a.group[k];
  const bool gok = g < a.G;
  uint4 prow[4] = {};
  if (gok && a.peer) {
#pragma unroll
    for (int j = 0; j < 4; ++j) prow[j] = a.peer[(size_t)g * 4 + j];
  }
  WireMsg m;
  const bool fast = fits && w_fast_message(win + (reinterpret_cast<uintptr_t>(a.bytes) + o - base), (int64_t)len, &m);
  // wave-aggregated append of the other records to the pass-2 queue
  const uint64_t slow = __ballot(!fast);
  if (slow) {
    const uint32_t cnt = (uint32_t)__popcll(slow);
    const uint32_t leader = (uint32_t)__ffsll((long long)slow) - 1;
    uint32_t b0 = 0;
    if (lane == leader) b0 = atomicAdd(qn, cnt);
    b0 = __shfl(b0, (int)leader);
    if (!fast) q[b0 + (uint32_t)__popcll(slow & ((1ull << lane) - 1))] = (uint32_t)k;
  }
  if (!fast) return;
  dec_emit(a, k, W_OK, m, g, gok, reinterpret_cast<const uint64_t*>(prow));
}

// row[7] of a group's peer row = its replica count n (from meta), so the
// From -> slot lookup reads one 64-byte row and no meta.  Refreshed whenever
// either side (hb_load_groups / hb_load_peers) changes.
__global__ void k_peer_n(uint64_t* peer, const uint64_t* meta, uint32_t first, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) peer[(size_t)(first + i) * HB_PEER_ROW + HB_PEER_ROW - 1] = m_n(meta[first + i]);
}

// Pass 2: Message.Unmarshal (hipbatch_wire.h) for the queued records, read
// from global memory.  Grid-stride over the queue length written by pass 1;
// the last workgroup to finish clears the queue for the next hb_decode.
__global__ void __launch_bounds__(DEC_THREADS) k_decode_general(DecodeArgs a, const uint32_t* q, uint32_t* qn) {
  const uint32_t total = *(volatile uint32_t*)qn;
  for (uint32_t j = blockIdx.x * DEC_THREADS + threadIdx.x; j < total; j += gridDim.x * DEC_THREADS) {
    const uint64_t k = q[j];
    const uint32_t g = a.group[k];
    const bool gok = g < a.G;
    uint64_t ids[HB_PEER_ROW] = {};
    if (gok && a.peer) {
      const uint64_t* row = reinterpret_cast<const uint64_t*>(a.peer) + (size_t)g * HB_PEER_ROW;
#pragma unroll
      for (uint32_t s = 0; s < HB_PEER_ROW; ++s) ids[s] = row[s];
    }
    WireMsg m;
    const int rc = w_unmarshal_message(a.bytes + a.off[k], (int64_t)a.len[k], &m);
    dec_emit(a, k, rc, m, g, gok, ids);
  }
  // qn[1] counts finished workgroups; the last one resets both words
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(qn + 1, 1u) == gridDim.x - 1) {
      qn[0] = 0;
      qn[1] = 0;
      __threadfence();
    }
  }
}

// ---------------------------------------------------------------------------
// hb_decode_follow: hb_decode plus the follower side.  MsgApp
// (with its entries), MsgHeartbeat and MsgVote become batch records too; the
// entry run of record i goes to eterm / edesc / edata at eoff[i].
//   k_decf_parse    a lane per record: the canonical-shape parser
//                   (hipbatch_wire_in.h) from the wave's LDS window, or from
//                   global memory when the wave's span does not fit (one long
//                   payload is enough); batch record, status, the record's
//                   entry count scanned inside the workgroup (eoff[i] = the
//                   prefix in its workgroup, bsum = the workgroup's sum).  Any
//                   other shape is queued.
//   k_decf_general  Message.Unmarshal over the queue, as k_decode_general; a
//                   queued record never has an entry run.
//   k_decf_scan     one workgroup: the workgroups' bases, the total, eoff[n],
//                   the sentinel record n.
//   k_decf_write    a lane per record: eoff[i] += its workgroup's base, then the
//                   lanes with entries walk their record again (global memory)
//                   and write the run, unless the total exceeds ent_cap.
//   k_decf_small    scan + write in one workgroup (the small-step rule).
// ---------------------------------------------------------------------------
struct DecfArgs {
  DecodeArgs d;
  uint64_t* o_commit;
  uint64_t* eoff;
  uint64_t* eterm;
  uint32_t* edesc;
  uint64_t* edata;
  uint64_t ent_cap;
  uint64_t* n_ent;
  uint32_t* bsum;   // [workgroups of k_decf_parse] entries per workgroup
  uint64_t* bbase;  // [workgroups + 1] their exclusive scan, then the total
};
// PROPS (hb_set_wire_props bit HB_WIRE_PROPS_IN): a canonical forwarded MsgProp is
// a batch record too.  A template parameter of the kernels that parse, so that with the bit off
// the code that runs is the code a handle without the knob ran.
constexpr uint32_t DECF_WIN = 8192;  // bytes staged per wave: 128 a record (a MsgApp with one small entry is ~70)
constexpr uint32_t DECF_SMALL_MAX = 16384;  // the small-step rule: scan and write in one workgroup
static_assert(WI_ENT_MAX_DATA == HB_ENT_MAX_DATA && (uint64_t)DEC_THREADS * WI_MAX_ENTS < (1ull << 32),
              "descriptor layout; a workgroup's entry count fits 32 bits");
static_assert(DECF_SMALL_MAX <= DEC_THREADS * DEC_THREADS, "k_decf_small scans one workgroup sum per lane");
static_assert((DEC_THREADS / 64) * (DECF_WIN + 32) <= 40 * 1024, "four workgroups of k_decf_parse per CU (160 KiB LDS)");

// Outcome of one record -> batch record + status (both passes).  nent: the
// field-7 occurrences; canon: the record has the canonical shape and its
// entries pass the checks.  Returns whether the record keeps an entry run.
template <bool PROPS>
__device__ __forceinline__ bool decf_emit(const DecfArgs& a, uint64_t k, int rc, const WireMsgF& f, bool canon,
                                          uint32_t g, bool gok, const uint64_t* ids) {
  const WireMsg& m = f.m;
  const bool resp = m.type == HB_MSG_APP_RESP || m.type == HB_MSG_VOTE_RESP || m.type == HB_MSG_HEARTBEAT_RESP;
  const bool fol = m.type == HB_MSG_APP || m.type == HB_MSG_HEARTBEAT || m.type == HB_MSG_VOTE;
  // a forwarded proposal that passed wi_message's proposal rule (pass one only: canon)
  const bool prop = PROPS && canon && m.type == HB_MSG_PROP;
  uint32_t slot = HB_SLOT_NONE;
  if (rc == W_OK && (resp || fol || prop) && gok && a.d.peer && m.from != 0) {
    const uint32_t nn = (uint32_t)ids[HB_PEER_ROW - 1];
#pragma unroll
    for (uint32_t s = 0; s < HB_MAX_REPLICAS; ++s)
      if (s < nn && slot == HB_SLOT_NONE && ids[s] == m.from) slot = s;
  }
  uint32_t st;
  if (rc == W_ERR) st = HB_WIRE_ERROR;
  else if (rc == W_PANIC) st = HB_WIRE_PANIC;
  else if (rc == W_DEEP) st = HB_WIRE_HOST;
  else if (m.type == HB_MSG_HUP || m.type == HB_MSG_BEAT || m.type == HB_MSG_UNREACHABLE ||
           m.type == HB_MSG_SNAP_STATUS)
    st = HB_WIRE_LOCAL;  // IsLocalMsg raft/util.go:49-51
  else if (resp) st = gok ? HB_WIRE_OK : HB_WIRE_BADGROUP;
  else if (prop) st = gok ? HB_WIRE_OK : HB_WIRE_HOST;  // index = the entry count; a non-member's slot is HB_SLOT_NONE
  else if (!fol || !gok) st = HB_WIRE_HOST;  // (hb_decode's precedence: the type rule comes before the group's)
  else if (m.type == HB_MSG_VOTE) st = slot != HB_SLOT_NONE ? HB_WIRE_OK : HB_WIRE_HOST;  // HB_INFO_VOTED: the host's
  else if (m.type == HB_MSG_APP) st = (f.f.nentries == 0 || canon) ? HB_WIRE_OK : HB_WIRE_HOST;
  else st = HB_WIRE_OK;  // MsgHeartbeat
  const bool ok = st == HB_WIRE_OK;
  uint64_t hint = m.hint, commit = 0;
  if (fol) {
    hint = m.type == HB_MSG_HEARTBEAT ? 0ull : f.f.log_term;
    commit = m.type == HB_MSG_VOTE ? 0ull : f.f.commit;
  }
  a.d.o_group[k] = ok ? g : 0xFFFFFFFFu;
  a.d.o_info[k] = ok ? ((uint32_t)m.type | (slot << 4) | ((uint32_t)m.reject << 8)) : 0u;
  a.d.o_term[k] = ok ? m.term : 0ull;
  a.d.o_index[k] = ok ? (prop ? (uint64_t)f.f.nentries : m.index) : 0ull;
  a.d.o_hint[k] = ok ? hint : 0ull;  // (a proposal's header is all zero: wi_message)
  a.o_commit[k] = ok ? commit : 0ull;
  a.d.status[k] = (uint8_t)st;
  return ok && (m.type == HB_MSG_APP || prop) && f.f.nentries != 0;
}

template <bool PROPS>
__device__ __forceinline__ bool decf_canon(const uint8_t* p, uint32_t len, WireMsgF* f) {
  WiHeader h;
  WiTail t;
  uint32_t ne = 0;
  if (!wi_message(p, len, &h, &t, &ne, PROPS)) return false;
  f->m.type = (int32_t)h.type;
  f->m.from = h.from;
  f->m.term = h.term;
  f->m.index = h.index;
  f->m.hint = t.hint;
  f->m.reject = t.reject;
  f->f.log_term = h.log_term;
  f->f.commit = t.commit;
  f->f.nentries = ne;
  return true;
}

template <bool PROPS>
__global__ void __launch_bounds__(DEC_THREADS) k_decf_parse(DecfArgs a, uint32_t* q, uint32_t* qn) {
  __shared__ uint4 l_win[DEC_THREADS / 64][DECF_WIN / 16 + 2];
  __shared__ uint32_t sh16[16];
  const DecodeArgs& A_ = a.d;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t k = (uint64_t)blockIdx.x * DEC_THREADS + threadIdx.x;
  const bool live = k < A_.n;
  const uint64_t o = live ? A_.off[k] : 0ull;
  const uint32_t len = live ? A_.len[k] : 0u;
  uint64_t lo = live ? o : ~0ull, hi = live ? o + len : 0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const bool fits = hi > lo && hi - lo <= DECF_WIN;  // uniform in the wave
  uint8_t* win = reinterpret_cast<uint8_t*>(&l_win[wave][0]);
  const uintptr_t A = reinterpret_cast<uintptr_t>(A_.bytes) + lo, B = reinterpret_cast<uintptr_t>(A_.bytes) + hi;
  const uintptr_t base = A & ~(uintptr_t)15;
  if (fits) {
    const uintptr_t A16 = (A + 15) & ~(uintptr_t)15, B16 = B & ~(uintptr_t)15;
    if (A16 < B16) {
      const uint32_t nc = (uint32_t)((B16 - A16) >> 4), c0 = (uint32_t)((A16 - base) >> 4);
      for (uint32_t c = lane; c < nc; c += 64) l_win[wave][c0 + c] = reinterpret_cast<const uint4*>(A16)[c];
      for (uintptr_t x = A + lane; x < A16; x += 64) win[x - base] = *reinterpret_cast<const uint8_t*>(x);
      for (uintptr_t x = B16 + lane; x < B; x += 64) win[x - base] = *reinterpret_cast<const uint8_t*>(x);
    } else {
      for (uintptr_t x = A + lane; x < B; x += 64) win[x - base] = *reinterpret_cast<const uint8_t*>(x);
    }
  }
  __syncthreads();
  // (no early exit: every lane takes part in the workgroup's scan below)
  const uint32_t g = live ? A_.group[k] : 0u;
  const bool gok = live && g < A_.G;
  uint4 prow[4] = {};
  if (gok && A_.peer) {
#pragma unroll
    for (int j = 0; j < 4; ++j) prow[j] = A_.peer[(size_t)g * 4 + j];
  }
  WireMsgF f;
  bool canon = false;
  if (live) {
    // a wave whose span does not fit (a long payload among its records) parses from global memory:
    // one copy of the parser behind a flat pointer, chosen per wave
    const uint8_t* src = fits ? win + (reinterpret_cast<uintptr_t>(A_.bytes) + o - base) : A_.bytes + o;
    canon = decf_canon<PROPS>(src, len, &f);
  }
  // wave-aggregated append of the other records to the general pass's queue
  const bool slowl = live && !canon;
  const uint64_t slow = __ballot(slowl);
  if (slow) {
    const uint32_t cnt = (uint32_t)__popcll(slow);
    const uint32_t leader = (uint32_t)__ffsll((long long)slow) - 1;
    uint32_t b0 = 0;
    if (lane == leader) b0 = atomicAdd(qn, cnt);
    b0 = __shfl(b0, (int)leader);
    if (slowl) q[b0 + (uint32_t)__popcll(slow & ((1ull << lane) - 1))] = (uint32_t)k;
  }
  uint32_t ne = 0;
  if (canon && decf_emit<PROPS>(a, k, W_OK, f, true, g, gok, reinterpret_cast<const uint64_t*>(prow))) ne = f.f.nentries;
  uint32_t tot;
  const uint32_t ex = block_excl_scan(ne, sh16, &tot);
  if (live) a.eoff[k] = ex;
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(DEC_THREADS) k_decf_general(DecfArgs a, const uint32_t* q, uint32_t* qn) {
  const uint32_t total = *(volatile uint32_t*)qn;
  for (uint32_t j = blockIdx.x * DEC_THREADS + threadIdx.x; j < total; j += gridDim.x * DEC_THREADS) {
    const uint64_t k = q[j];
    const uint32_t g = a.d.group[k];
    const bool gok = g < a.d.G;
    uint64_t ids[HB_PEER_ROW] = {};
    if (gok && a.d.peer) {
      const uint64_t* row = reinterpret_cast<const uint64_t*>(a.d.peer) + (size_t)g * HB_PEER_ROW;
#pragma unroll
      for (uint32_t s = 0; s < HB_PEER_ROW; ++s) ids[s] = row[s];
    }
    WireMsgF f;
    const int rc = w_unmarshal_follow(a.d.bytes + a.d.off[k], (int64_t)a.d.len[k], &f);
    (void)decf_emit<false>(a, k, rc, f, false, g, gok, ids);  // (a queued record is no proposal record)
  }
  // qn[1] counts finished workgroups; the last one resets both words
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(qn + 1, 1u) == gridDim.x - 1) {
      qn[0] = 0;
      qn[1] = 0;
      __threadfence();
    }
  }
}

// Block-wide exclusive scan of 64-bit values (any blockDim.x that is a multiple of 64).
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, uint64_t* sh16, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(incl, d);
    if (lane >= (uint32_t)d) incl += t;
  }
  if (lane == 63) sh16[wave] = incl;
  __syncthreads();
  uint64_t before = 0, tot = 0;
  for (uint32_t w = 0; w < nw; ++w) {
    const uint64_t x = sh16[w];
    if (w < wave) before += x;
    tot += x;
  }
  *total = tot;
  __syncthreads();
  return before + incl - v;
}

// The total, eoff[n] and record n: a dropped record, so that a step over n + 1
// records with n_edesc = ent_cap reads the count nowhere (include/hipbatch.h).
__device__ __forceinline__ void decf_finish(const DecfArgs& a, uint64_t tot) {
  const uint64_t n = a.d.n;
  a.eoff[n] = tot;
  *a.n_ent = tot;
  a.d.o_group[n] = 0xFFFFFFFFu;
  a.d.o_info[n] = 0u;
  a.d.o_term[n] = 0ull;
  a.d.o_index[n] = 0ull;
  a.d.o_hint[n] = 0ull;
  a.o_commit[n] = 0ull;
}

// Workgroup `blk` of k_decf_parse, whose first entry is `base`: the final eoff,
// and the entry runs when `write` (uniform).  eoff is rewritten in place: every
// lane reads its own and its neighbour's local prefix before any lane writes.
template <bool PROPS>
__device__ __forceinline__ void decf_write_block(const DecfArgs& a, uint64_t blk, uint64_t base, bool write) {
  const uint64_t n = a.d.n, k = blk * DEC_THREADS + threadIdx.x;
  const bool live = k < n;
  uint64_t loc = 0, nxt = 0;
  if (live) {
    loc = a.eoff[k];
    nxt = (threadIdx.x == DEC_THREADS - 1 || k + 1 == n) ? (uint64_t)a.bsum[blk] : a.eoff[k + 1];
  }
  __syncthreads();
  if (!live) return;
  const uint64_t e0 = base + loc, ne = nxt - loc;
  a.eoff[k] = e0;
  if (!write || ne == 0) return;
  const uint64_t o = a.d.off[k];
  const uint8_t* p = a.d.bytes + o;
  const uint64_t l = a.d.len[k];
  WiHeader h;
  if (!wi_header(p, l, &h)) return;  // (pass one accepted it)
  uint64_t i = h.ents;
  for (uint64_t j = 0; j < ne; ++j) {
    WiEntry e;
    if constexpr (PROPS) {  // the entry rule pass one used
      if (!(wi_is_prop(h, true) ? wi_prop_entry(p, l, i, &e) : wi_entry(p, l, i, h.index + 1 + j, &e))) return;
    } else {
      if (!wi_entry(p, l, i, h.index + 1 + j, &e)) return;
    }
    a.eterm[e0 + j] = e.term;
    a.edesc[e0 + j] = e.desc;
    a.edata[e0 + j] = e.data ? o + e.data : 0ull;
  }
}

__global__ void __launch_bounds__(1024) k_decf_scan(DecfArgs a, uint32_t nblk) {
  __shared__ uint64_t sh16[16];
  const uint32_t per = (nblk + 1023) / 1024, b0 = threadIdx.x * per;
  uint64_t sum = 0;
  for (uint32_t i = b0; i < b0 + per && i < nblk; ++i) sum += a.bsum[i];
  uint64_t tot;
  uint64_t run = block_excl_scan64(sum, sh16, &tot);
  for (uint32_t i = b0; i < b0 + per && i < nblk; ++i) {
    a.bbase[i] = run;
    run += a.bsum[i];
  }
  if (threadIdx.x == 0) {
    a.bbase[nblk] = tot;
    decf_finish(a, tot);
  }
}
template <bool PROPS>
__global__ void __launch_bounds__(DEC_THREADS) k_decf_write(DecfArgs a, uint32_t nblk) {
  decf_write_block<PROPS>(a, blockIdx.x, a.bbase[blockIdx.x], a.bbase[nblk] <= a.ent_cap);
}
// At most DECF_SMALL_MAX records (at most DEC_THREADS workgroups of k_decf_parse): scan and write.
template <bool PROPS>
__global__ void __launch_bounds__(DEC_THREADS) k_decf_small(DecfArgs a, uint32_t nblk) {
  __shared__ uint64_t sh16[16];
  __shared__ uint64_t l_base[DEC_THREADS];
  uint64_t tot;
  l_base[threadIdx.x] = block_excl_scan64(threadIdx.x < nblk ? (uint64_t)a.bsum[threadIdx.x] : 0ull, sh16, &tot);
  __syncthreads();
  if (threadIdx.x == 0) decf_finish(a, tot);
  for (uint32_t b = 0; b < nblk; ++b) decf_write_block<PROPS>(a, b, l_base[b], tot <= a.ent_cap);
}

// ============================================================================
// Phase 3: finish
// ============================================================================
__global__ void __launch_bounds__(128) k_finish(uint64_t* shard, uint64_t* stats, uint64_t* accum) {
  const int map[ST_N + 1] = {HB_STAT_MSGS,  HB_STAT_APPRESP, HB_STAT_VOTERESP, HB_STAT_DROPPED, HB_STAT_COMMITS,
                             HB_STAT_WON,   HB_STAT_LOST,    HB_STAT_FAULTS,   HB_STAT_ENTRIES, HB_STAT_EVENTS};
  const uint32_t t = threadIdx.x, k = t / NSH;
  uint64_t v = 0;
  if (k <= ST_N) {
    v = shard[shard_at(k, t % NSH)];
    shard[shard_at(k, t % NSH)] = 0;  // ready for the next step
  }
#pragma unroll
  for (uint32_t d = 1; d < NSH; d <<= 1) v += __shfl_xor(v, d);
  if (k <= ST_N && t % NSH == 0) {
    stats[map[k]] = v;
    if (accum) accum[map[k]] += v;
  }
}

// ============================================================================
// group load / gather / inflights
// ============================================================================
__global__ void k_load(DevState S, uint32_t first, uint32_t count, const hb_group* src) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t g = first + i;
  const hb_group& r = src[i];
  S.term[g] = r.term;
  S.commit[g] = r.committed;
  S.first[g] = r.first_index;
  S.last[g] = r.last_index;
  S.tfirst[g] = r.term_first;
  S.tlast[g] = r.term_last;
  S.snap[g] = r.snap_index;
  uint64_t m = meta_make(r.state, r.n, r.self_slot, r.lead, r.vote, r.fault, r.votes_resp, r.votes_grant);
  if (r.term_last == r.last_index) m |= M_TL;
  if (r.self_slot < r.n && r.pr[r.self_slot].match == r.last_index && r.pr[r.self_slot].next == r.last_index + 1)
    m |= M_SM;
  if (r.commit_zero && r.committed != 0) m |= M_NC;  // r.Commit = 0 until the group's first Step
  bool nx = S.lazy_next != 0 && r.state == HB_STATE_LEADER && r.n != 0 && r.n <= S.nmax;
  for (uint32_t s = 0; s < S.nmax && s < r.n; ++s) nx = nx && r.pr[s].next == r.last_index + 1;
  if (nx) m |= M_NX;  // the next words are then not kept (nor written here)
  S.meta[g] = m;
  S.elapsed[g] = 0;  // newRaft: fresh r.rand, becomeFollower -> reset
  S.rpos[g] = 0;
  if (S.szx) {  // finite max_msg_size: no entry sizes yet (hb_load_entry_sizes)
    S.szlo[g] = r.last_index;
    *cum_at(S.szx[g], r.last_index) = 0;
  }
  S.trc[g] = 0;  // no older term runs yet (hb_load_term_runs)
  for (uint32_t s = 0; s < S.nmax; ++s) {
    const bool on = s < r.n;
    const size_t o = (size_t)s * S.G + g;
    S.match[o] = on ? r.pr[s].match : 0;
    if (!(nx && on)) S.next[o] = on ? r.pr[s].next : 0;
    S.pending[o] = on ? r.pr[s].pending_snapshot : 0;
    S.pm[o] = on ? pm_make(r.pr[s].state, r.pr[s].paused, r.pr[s].ins_start, r.pr[s].ins_count) : 0;
  }
}

__global__ void k_gather(DevState S, uint32_t first, uint32_t count, hb_group* dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t g = first + i;
  hb_group r;
  memset(&r, 0, sizeof(r));
  const uint64_t m = S.meta[g];
  r.term = S.term[g];
  r.committed = S.commit[g];
  r.first_index = S.first[g];
  r.last_index = S.last[g];
  r.term_first = S.tfirst[g];
  r.term_last = (m & M_TL) ? r.last_index : S.tlast[g];
  r.snap_index = S.snap[g];
  r.state = m_state(m);
  r.n = m_n(m);
  r.self_slot = m_self(m);
  r.lead = m_lead(m);
  r.vote = m_vote(m);
  r.fault = m_fault(m);
  r.votes_resp = m_resp(m);
  r.votes_grant = m_grant(m);
  r.commit_zero = (m & M_NC) ? 1u : 0u;
  for (uint32_t s = 0; s < S.nmax && s < r.n; ++s) {
    const size_t o = (size_t)s * S.G + g;
    uint32_t p = S.pm[o];
    const bool kept = !((m & M_SM) && s == r.self_slot);  // M_SM: materialized from last
    r.pr[s].match = kept ? S.match[o] : r.last_index;
    r.pr[s].next = (kept && !(m & M_NX)) ? S.next[o] : r.last_index + 1;  // M_NX: every slot's, likewise
    if (m & M_RS) rs_progress(m, s, r.last_index, r.term_first, &r.pr[s].match, &r.pr[s].next, &p);
    r.pr[s].state = pm_state(p);
    r.pr[s].paused = pm_paused(p);
    r.pr[s].ins_start = pm_start(p);
    r.pr[s].ins_count = pm_count(p);
    r.pr[s].pending_snapshot = pm_state(p) == HB_PR_SNAPSHOT ? S.pending[o] : 0;
  }
  // the record's run lies in [first_index - 1, last_index]: hb_set_log_bounds may have moved
  // firstIndex past the start the device keeps (which M_RS above still needs as it is)
  if (r.term_first != HB_NO_INDEX && r.term_first + 1 < r.first_index) r.term_first = r.first_index - 1;
  dst[i] = r;
}

// hb_lazy_next_groups (tests): the live groups whose next array is not kept (M_NX)
__global__ void k_count_lazy_next(DevState S, uint32_t* out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t m = g < S.G ? S.meta[g] : 0ull;
  const uint64_t b = __ballot(m_n(m) != 0 && (m & M_NX) != 0);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(out, (uint32_t)__popcll(b));
}

__global__ void k_set_bounds(DevState S, uint32_t count, const uint32_t* groups, const uint64_t* first,
                             const uint64_t* snap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t g = groups[i];
  S.first[g] = first[i];
  S.snap[g] = snap[i];
}

// hb_load_term_runs: group groups[i] takes runs (start, term) off[i] .. + n_i
__global__ void k_load_runs(DevState S, uint32_t count, const uint32_t* groups, const uint32_t* n_runs,
                            const uint64_t* off, const uint64_t* runs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t g = groups[i], k = n_runs[i];
  uint64_t* R = lx_base(S.trx[g]);  // the host reserved >= k runs
  for (uint32_t j = 0; j < k; ++j) {
    R[2 * j] = runs[2 * (off[i] + j)];
    R[2 * j + 1] = runs[2 * (off[i] + j) + 1];
  }
  S.trc[g] = k;  // count k, head 0
}

// hb_load_entry_sizes: group groups[i] takes the sizes of its entries
// (last - n_i, last], concatenated at sizes + off[i]
__global__ void k_load_sizes(DevState S, uint32_t count, const uint32_t* groups, const uint32_t* n_sizes,
                             const uint64_t* off, const uint32_t* sizes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t g = groups[i], k = n_sizes[i];
  const uint64_t last = S.last[g], lo = last - k, x = S.szx[g];  // the host reserved > k entries
  const uint32_t* z = sizes + off[i];
  uint64_t acc = 0;
  *cum_at(x, lo) = 0;
  for (uint32_t j = 1; j <= k; ++j) {
    acc += z[j - 1];
    *cum_at(x, lo + j) = acc;
  }
  S.szlo[g] = lo;
}

// hb_reserve_log: move job i's ring to a larger extent, keeping its content.
// A job is 4 words: group | kind << 32 (0 sizes, 1 runs), old extent word, new extent word, unused.
__global__ void k_regrow(DevState S, uint32_t count, const uint64_t* jobs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t* j = jobs + 4 * (size_t)i;
  const uint32_t g = (uint32_t)j[0], kind = (uint32_t)(j[0] >> 32);
  const uint64_t ox = j[1], nx = j[2];
  if (kind == 0) {  // cum(i) for i in [szlo, last]: same index, new mask
    const uint64_t lo = S.szlo[g], last = S.last[g];
    for (uint64_t k = lo; k <= last; ++k) *cum_at(nx, k) = *cum_at(ox, k);
    S.szx[g] = nx;
  } else {  // runs in ring order, to the front of the new ring (head 0)
    const uint64_t c = S.trc[g];
    const uint32_t n = (uint32_t)c, h = (uint32_t)(c >> 32);
    const uint64_t om = lx_cap(ox) - 1;
    const uint64_t* O = lx_base(ox);
    uint64_t* N = lx_base(nx);
    for (uint32_t k = 0; k < n; ++k) {
      const uint64_t o = 2 * ((h + k) & om);
      N[2 * k] = O[o];
      N[2 * k + 1] = O[o + 1];
    }
    S.trx[g] = nx;
    S.trc[g] = n;
  }
}

__global__ void k_remove(DevState S, uint32_t first, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) S.meta[first + i] = 0;
}

__global__ void k_set_ins(DevState S, uint32_t g, uint32_t s, uint32_t start, uint32_t count, const uint64_t* vals) {
  for (uint32_t i = threadIdx.x; i < count; i += blockDim.x) {
    uint32_t idx = start + i;
    if (idx >= S.W) idx -= S.W;
    S.ring[((size_t)s * S.W + idx) * S.G + g] = vals[i];
  }
  if (threadIdx.x == 0) {
    const uint64_t m = S.meta[g];
    if (m & M_RS) {  // the reset form written out first: this slot's window changes alone
      for (uint32_t k = 0; k < m_n(m); ++k) {
        const size_t ok = (size_t)k * S.G + g;
        uint64_t mt, nx;
        uint32_t pk;
        rs_progress(m, k, S.last[g], S.tfirst[g], &mt, &nx, &pk);
        if (!((m & M_SM) && k == m_self(m))) {
          S.match[ok] = mt;
          S.next[ok] = nx;
        }
        S.pm[ok] = pk;
      }
      S.meta[g] = m & ~M_RS;
    }
    // (M_NX stays as it is: a window is not Next, and the flag never comes with M_RS)
    const size_t o = (size_t)s * S.G + g;
    const uint32_t p = S.pm[o];
    S.pm[o] = pm_make(pm_state(p), pm_paused(p), start, count);
  }
}

__global__ void k_get_ins(DevState S, uint32_t g, uint32_t s, uint64_t* vals, uint32_t* sc) {
  const size_t o = (size_t)s * S.G + g;
  const uint32_t p = (S.meta[g] & M_RS) ? 0u : S.pm[o];  // the reset form: an empty window
  const uint32_t start = pm_start(p), count = pm_count(p);
  for (uint32_t i = threadIdx.x; i < count; i += blockDim.x) {
    uint32_t idx = start + i;
    if (idx >= S.W) idx -= S.W;
    vals[i] = S.ring[((size_t)s * S.W + idx) * S.G + g];
  }
  if (threadIdx.x == 0) {
    sc[0] = start;
    sc[1] = count;
  }
}

// ============================================================================
// hb_move_groups: slot dst[i] takes every device word of slot src[i].  All
// sources are read (k_move_gather, k_move_ring<false>) into a staging buffer
// before any destination is written (k_move_scatter, k_move_ring<true>), so
// swaps, cycles and chains need no ordering.  The raw words travel: the lazy
// forms of meta (M_RS / M_SM / M_TL / M_NC / M_NX) stay exactly as they are.
// ============================================================================
struct MoveArgs {
  uint32_t count, nvac;
  const uint32_t* src;      // [count]
  const uint32_t* dst;      // [count]
  const uint32_t* vac;      // [nvac] slots in src but not in dst: they end up empty ...
  const uint64_t* vac_szx;  // [nvac] ... and own the extents the overwritten slots held
  const uint64_t* vac_trx;  // [nvac]
  uint64_t* stage;          // [move_words()][count], word-major (a lane per move: coalesced)
  uint64_t* peer;           // the peer-id table or null
  uint64_t* jobs;           // [count x nmax] non-empty inflight windows: (move * 8 + slot) | ring-stage offset << 28
  unsigned long long* ctr;  // [0] jobs, [1] ring-stage words
  uint64_t* rstage;         // the windows' words, window after window
};
constexpr uint32_t MV_PM_WORD = 8 + 3;  // stage word of slot s's pm: MV_PM_WORD + 4 s
constexpr uint32_t MV_JOB_SHIFT = 28;   // a job's low bits: move (< 2^24 groups) * 8 + slot
__host__ __device__ inline uint32_t move_words(uint32_t nmax, bool sized, bool peers) {
  return 8 + 4 * nmax + 2 + 2 + (sized ? 2u : 0u) + (peers ? HB_PEER_ROW : 0u);
}
// the live window of a staged pm word (start, count), as k_get_ins reads it
__device__ __forceinline__ void move_window(const DevState& S, uint64_t meta, uint32_t pm, uint32_t* start,
                                            uint32_t* count) {
  const uint32_t c = (meta & M_RS) ? 0u : pm_count(pm);  // the reset form: an empty window
  *count = c < S.W ? c : S.W;
  *start = pm_start(pm) % S.W;
}

__global__ void __launch_bounds__(256) k_move_gather(DevState S, MoveArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  const uint32_t g = a.src[i];
  uint64_t* w = a.stage + i;
  auto put = [&](uint64_t x) {
    *w = x;
    w += a.count;
  };
  const uint64_t m = S.meta[g];
  put(S.term[g]);
  put(S.commit[g]);
  put(S.first[g]);
  put(S.last[g]);
  put(S.tfirst[g]);
  put(S.tlast[g]);
  put(S.snap[g]);
  put(m);
  for (uint32_t s = 0; s < S.nmax; ++s) {
    const size_t o = (size_t)s * S.G + g;
    const uint32_t p = S.pm[o];
    put(S.match[o]);
    put(S.next[o]);
    put(S.pending[o]);
    put(p);
    uint32_t start, cnt;
    move_window(S, m, p, &start, &cnt);
    if (cnt && g != a.dst[i]) {  // a window to carry: its place in the ring stage, and a wave's job
      const uint64_t off = atomicAdd(a.ctr + 1, (unsigned long long)cnt);
      const uint64_t j = atomicAdd(a.ctr, 1ull);
      a.jobs[j] = (uint64_t)(i * 8u + s) | (off << MV_JOB_SHIFT);
    }
  }
  put((uint64_t)S.elapsed[g] | ((uint64_t)S.rpos[g] << 32));
  put(S.tcfg[g]);
  put(S.trc[g]);
  put(S.trx[g]);
  if (S.szx) {
    put(S.szlo[g]);
    put(S.szx[g]);
  }
  if (a.peer)
    for (uint32_t k = 0; k < HB_PEER_ROW; ++k) put(a.peer[(size_t)g * HB_PEER_ROW + k]);
}

// lanes [0, count): move i's words into dst[i]; lanes [count, count + nvac): a vacated slot
__global__ void __launch_bounds__(256) k_move_scatter(DevState S, MoveArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) {
    const uint32_t v = i - a.count;
    if (v >= a.nvac) return;
    const uint32_t g = a.vac[v];
    S.meta[g] = 0;  // as hb_remove_groups leaves it; the rings start over in their new extents
    S.trc[g] = 0;
    S.trx[g] = a.vac_trx[v];
    if (S.szx) {
      S.szlo[g] = S.last[g];
      S.szx[g] = a.vac_szx[v];
    }
    return;
  }
  const uint32_t g = a.dst[i];
  const uint64_t* w = a.stage + i;
  auto get = [&]() {
    const uint64_t x = *w;
    w += a.count;
    return x;
  };
  S.term[g] = get();
  S.commit[g] = get();
  S.first[g] = get();
  S.last[g] = get();
  S.tfirst[g] = get();
  S.tlast[g] = get();
  S.snap[g] = get();
  S.meta[g] = get();
  for (uint32_t s = 0; s < S.nmax; ++s) {
    const size_t o = (size_t)s * S.G + g;
    S.match[o] = get();
    S.next[o] = get();
    S.pending[o] = get();
    S.pm[o] = (uint32_t)get();
  }
  const uint64_t t = get();
  S.elapsed[g] = (uint32_t)t;
  S.rpos[g] = (uint32_t)(t >> 32);
  S.tcfg[g] = (uint32_t)get();
  S.trc[g] = get();
  S.trx[g] = get();
  if (S.szx) {
    S.szlo[g] = get();
    S.szx[g] = get();
  }
  if (a.peer)
    for (uint32_t k = 0; k < HB_PEER_ROW; ++k) a.peer[(size_t)g * HB_PEER_ROW + k] = get();
}

// A wave per job (move, follower slot): the live window's words between the
// inflight ring and the ring stage, at the same ring positions (OUT: stage -> dst).
template <bool OUT>
__global__ void __launch_bounds__(256) k_move_ring(DevState S, MoveArgs a, uint32_t njobs) {
  const uint32_t j = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63u;
  if (j >= njobs) return;
  const uint64_t job = a.jobs[j];
  const uint32_t is = (uint32_t)(job & ((1ull << MV_JOB_SHIFT) - 1)), i = is >> 3, s = is & 7u;
  const uint64_t off = job >> MV_JOB_SHIFT;
  if (i >= a.count || s >= S.nmax) return;
  const uint32_t g = OUT ? a.dst[i] : a.src[i];
  const uint64_t m = a.stage[(size_t)7 * a.count + i];
  const uint32_t p = (uint32_t)a.stage[(size_t)(MV_PM_WORD + 4 * s) * a.count + i];
  uint32_t start, cnt;
  move_window(S, m, p, &start, &cnt);
  for (uint32_t k = lane; k < cnt; k += 64) {
    uint32_t idx = start + k;
    if (idx >= S.W) idx -= S.W;
    uint64_t* r = S.ring + ((size_t)s * S.W + idx) * S.G + g;
    if (OUT) *r = a.rstage[off + k];
    else a.rstage[off + k] = *r;
  }
}

// Dense gather of the chunked events: chunk c (counts[c] compact words at
// base + offs[c]; chunk 2p / 2p+1 = partition p's P / M chunk) is expanded
// into public hb_event records at out + dst[c], dst = exclusive scan of the
// per-chunk event counts.
__device__ __forceinline__ uint32_t evc_outputs(uint64_t w) {
  const uint32_t t = (uint32_t)w & 0xF;
  if (t == EVC_CONT) return 0;
  if (t == EVC_BCAST || t == EVC_VBCAST) return __popc((uint32_t)(w >> 4) & 0x7F);
  return 1;
}
__global__ void __launch_bounds__(256) k_chunk_events(const uint64_t* base, const uint32_t* counts,
                                                      const uint64_t* offs, uint32_t* out_counts) {
  __shared__ uint32_t sh16[16];
  const uint32_t c = blockIdx.x, n = counts[c];
  const uint64_t* src = base + offs[c];
  uint32_t k = 0;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) k += evc_outputs(src[i]);
  uint32_t tot;
  (void)block_excl_scan(k, sh16, &tot);
  if (threadIdx.x == 0) out_counts[c] = tot;
}
__global__ void __launch_bounds__(1024) k_scan_counts(const uint32_t* counts, uint32_t n, uint64_t* dst) {
  __shared__ uint32_t sh16[16];
  const uint32_t per = (n + 1023) / 1024, b0 = threadIdx.x * per;
  uint64_t sum = 0;
  for (uint32_t i = b0; i < b0 + per && i < n; ++i) sum += counts[i];
  uint32_t tot;
  uint64_t run = block_excl_scan((uint32_t)sum, sh16, &tot);  // total events < 2^32
  for (uint32_t i = b0; i < b0 + per && i < n; ++i) {
    dst[i] = run;
    run += counts[i];
  }
}
__global__ void __launch_bounds__(256) k_expand_events(const uint64_t* base, const uint32_t* counts,
                                                       const uint64_t* offs, const uint64_t* dst, hb_event* out) {
  __shared__ uint32_t sh16[16];
  const uint32_t c = blockIdx.x, n = counts[c], part = c >> 1;
  const uint64_t* src = base + offs[c];
  uint64_t run = dst[c];
  for (uint32_t t0 = 0; t0 < n; t0 += blockDim.x) {
    const uint32_t i = t0 + threadIdx.x;
    const uint64_t w = i < n ? src[i] : (uint64_t)EVC_CONT;
    const uint32_t k = evc_outputs(w);
    uint32_t tot;
    const uint32_t ex = block_excl_scan(k, sh16, &tot);
    if (k) {
      const uint32_t type = (uint32_t)w & 0xF, to = (uint32_t)(w >> 4) & 0x7F, aux = (uint32_t)(w >> 12) & 0xF;
      const uint32_t group = part * PART + ((uint32_t)(w >> 16) & 0xFF);
      uint64_t x = w >> 24;
      if ((w >> 11) & 1u) x |= (src[i + 1] >> 4) << 40;
      hb_event* o = out + run + ex;
      if (type == EVC_BCAST || type == EVC_VBCAST) {
        const uint8_t et = type == EVC_BCAST ? (uint8_t)HB_EV_APP : (uint8_t)HB_EV_VOTE;
        uint32_t m = to, r = 0;
        while (m) {
          const uint32_t s = __ffs(m) - 1;
          m &= m - 1;
          o[r++] = hb_event{x, group, et, (uint8_t)s, (uint16_t)aux};
        }
      } else {
        o[0] = hb_event{x, group, (uint8_t)type, (uint8_t)to, (uint16_t)aux};
      }
    }
    run += tot;
  }
}

// The compact delta to the host (hb_events_to_host): the words themselves,
// densely in chunk order, plus the words per chunk and their total.  Host
// destinations are pinned memory the kernels write through (posted PCIe writes,
// one coalesced 512-byte run per wave), so the copy is sized on the device.
__global__ void __launch_bounds__(1024) k_scan_words(const uint32_t* counts, uint32_t n, uint64_t* dst,
                                                     uint32_t* h_counts, uint64_t* h_total) {
  __shared__ uint32_t sh16[16];
  const uint32_t per = (n + 1023) / 1024, b0 = threadIdx.x * per;
  uint64_t sum = 0;
  for (uint32_t i = b0; i < b0 + per && i < n; ++i) sum += counts[i];
  uint32_t tot;
  uint64_t run = block_excl_scan((uint32_t)sum, sh16, &tot);  // total words < 2^32
  for (uint32_t i = b0; i < b0 + per && i < n; ++i) {
    dst[i] = run;
    run += counts[i];
  }
  for (uint32_t i = threadIdx.x; i < n; i += 1024) h_counts[i] = counts[i];
  if (threadIdx.x == 0) {
    dst[n] = tot;
    *h_total = tot;
  }
}
__global__ void __launch_bounds__(256) k_gather_words(const uint64_t* base, const uint32_t* counts,
                                                      const uint64_t* offs, const uint64_t* dst, uint64_t* out,
                                                      uint64_t cap) {
  const uint32_t c = blockIdx.x, n = counts[c];
  if (dst[gridDim.x] > cap) return;  // the caller's buffer is too small: counts and total only
  const uint64_t* src = base + offs[c];
  uint64_t* o = out + dst[c];
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) o[i] = src[i];
}

// Both in one workgroup when the chunks are few (a small node: 2 chunks per
// 256 groups): chunk offsets scanned in LDS, then a wave per chunk copies.
constexpr uint32_t WORDS_SMALL = 1024;
__global__ void __launch_bounds__(1024) k_words_small(const uint32_t* counts, uint32_t n, const uint64_t* base,
                                                      const uint64_t* offs, uint64_t* out, uint64_t cap,
                                                      uint32_t* h_counts, uint64_t* h_total) {
  __shared__ uint32_t sh16[16];
  __shared__ uint64_t s_dst[WORDS_SMALL];
  const uint32_t tid = threadIdx.x;
  const uint32_t c = tid < n ? counts[tid] : 0u;
  uint32_t tot;
  const uint32_t run = block_excl_scan(c, sh16, &tot);  // total words < 2^32
  if (tid < n) {
    s_dst[tid] = run;
    h_counts[tid] = c;
  }
  if (tid == 0) *h_total = tot;
  __syncthreads();
  if (tot > cap) return;  // the caller's buffer is too small: counts and total only
  const uint32_t wave = tid >> 6, lane = tid & 63;
  for (uint32_t k = wave; k < n; k += 16) {
    const uint32_t m = counts[k];
    const uint64_t* src = base + offs[k];
    uint64_t* o = out + s_dst[k];
    for (uint32_t i = lane; i < m; i += 64) o[i] = src[i];
  }
}

// ============================================================================
// Wire egress: hb_encode, hb_egress
// ============================================================================
// hb_encode: a device batch of payload-free outgoing messages -> the bytes
// Message.MarshalTo writes (hipbatch_wire_out.h), packed densely in record
// order.  Pass one sizes the records (block sums), one workgroup scans the
// sums, pass two writes: the mirror image of k_decode.  A wave's 64 records are
// one contiguous span of at most 64 x 91 bytes; each lane encodes into the
// wave's LDS window at its offset, then the wave stores the span with
// coalesced 16-byte stores and its unaligned head and tail byte by byte:
// neighbouring waves own neighbouring bytes, so nothing outside the span is
// read or written.
struct EncodeArgs {
  const uint32_t* info;
  const uint64_t *to, *term, *log_term, *index, *commit, *hint;
  uint64_t cap;
  const uint64_t* n_dev;  // null: cap
  uint64_t self_id;
  uint8_t* bytes;
  uint64_t bytes_cap;
  uint64_t* off;
  uint8_t* status;
  uint64_t* total;
  uint32_t* bsum;   // [blocks] bytes per pass-one workgroup
  uint64_t* bbase;  // [blocks + 1] their exclusive scan, then the total
};
constexpr uint32_t ENC_THREADS = 256;
constexpr uint32_t ENC_SMALL_THREADS = 512;
constexpr uint32_t ENC_SMALL_MAX = 16384;  // the small-step rule: one workgroup, one launch
constexpr uint32_t ENC_WIN = 64 * WO_MAX + 16;  // a wave's span plus the 16-byte phase of its first byte
static_assert(ENC_WIN % 16 == 0, "the window is read back as uint4");
static_assert(WO_PREFIX_MAX + 1 + WO_VARINT_MAX + WO_SNAP_LEN + 4 <= WO_MAX && WO_PREFIX_MAX < HB_WIRE_SPLICE,
              "a split record (HB_OUT_ENTS) is a payload-free record: WO_MAX and the window hold");

struct EncRec {
  uint32_t type;
  bool reject, host;
  bool ents;  // HB_OUT_ENTS: the split form (hint is the last entry's index, not a RejectHint)
  uint64_t to, term, log_term, index, commit, hint;
};
__device__ __forceinline__ uint64_t enc_n(const EncodeArgs& a) {
  const uint64_t n = a.n_dev ? *a.n_dev : a.cap;
  return n < a.cap ? n : a.cap;
}
// record i and its encoded length (0: past the end, HB_REF_OTHER: the host knows the id, or
// HB_OUT_HOST: a MsgVote or MsgApp the replay could not complete).  A record with HB_OUT_ENTS
// is the entry-free message (Reject = 0, RejectHint = 0): prefix ‖ suffix, wo_prefix_len.
__device__ __forceinline__ uint32_t enc_load(const EncodeArgs& a, uint64_t i, uint64_t n, EncRec* r) {
  r->host = false;
  r->ents = false;
  if (i >= n) return 0;
  const uint32_t info = a.info[i];
  r->type = info & 0xF;
  r->reject = (info >> 8) & 1u;
  r->host = ((info >> 4) & 0xF) == HB_REF_OTHER || (info & HB_OUT_HOST) != 0;
  if (r->host) return 0;
  r->to = a.to[i];
  r->term = a.term[i];
  r->log_term = a.log_term[i];
  r->index = a.index[i];
  r->commit = a.commit[i];
  r->hint = a.hint[i];
  r->ents = (info & HB_OUT_ENTS) != 0;
  if (r->ents) {
    r->reject = false;
    r->hint = 0;
  }
  return wo_size(r->type, r->to, a.self_id, r->term, r->log_term, r->index, r->commit, r->reject, r->hint);
}

// One tile of blockDim.x records from i0, whose first byte is `base`: off and
// status always, the bytes when `write` (uniform).  Returns the tile's bytes.
__device__ __forceinline__ uint32_t enc_tile(const EncodeArgs& a, uint64_t i0, uint64_t n, uint64_t base, bool write,
                                             uint4* l_win, uint32_t* sh16) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t i = i0 + threadIdx.x;
  EncRec r;
  const uint32_t sz = enc_load(a, i, n, &r);
  uint32_t tot;
  const uint32_t ex = block_excl_scan(sz, sh16, &tot);
  const uint64_t p = base + ex;
  if (i < n) {
    a.off[i] = p;
    uint8_t st = r.host ? (uint8_t)HB_WIRE_HOST : (uint8_t)HB_WIRE_OK;
    if (r.ents)
      st = (uint8_t)(HB_WIRE_SPLICE | wo_prefix_len(r.type, r.to, a.self_id, r.term, r.log_term, r.index));
    a.status[i] = st;
  }
  if (!write) return tot;
  const uint64_t lo = __shfl(p, 0), hi = __shfl(p + sz, 63);  // the wave's span
  uint4* wwin = l_win + (size_t)wave * (ENC_WIN / 16);
  uint8_t* win = reinterpret_cast<uint8_t*>(wwin);
  const uintptr_t A = reinterpret_cast<uintptr_t>(a.bytes) + lo, B = reinterpret_cast<uintptr_t>(a.bytes) + hi;
  const uintptr_t b16 = A & ~(uintptr_t)15;
  if (sz)
    wo_write(win + (A - b16) + (p - lo), r.type, r.to, a.self_id, r.term, r.log_term, r.index, r.commit, r.reject,
             r.hint);
  __syncthreads();
  if (hi > lo) {
    const uintptr_t A16 = (A + 15) & ~(uintptr_t)15, B16 = B & ~(uintptr_t)15;
    if (A16 < B16) {
      const uint32_t nc = (uint32_t)((B16 - A16) >> 4), c0 = (uint32_t)((A16 - b16) >> 4);
      for (uint32_t c = lane; c < nc; c += 64) reinterpret_cast<uint4*>(A16)[c] = wwin[c0 + c];
      for (uintptr_t x = A + lane; x < A16; x += 64) *reinterpret_cast<uint8_t*>(x) = win[x - b16];
      for (uintptr_t x = B16 + lane; x < B; x += 64) *reinterpret_cast<uint8_t*>(x) = win[x - b16];
    } else {
      for (uintptr_t x = A + lane; x < B; x += 64) *reinterpret_cast<uint8_t*>(x) = win[x - b16];
    }
  }
  __syncthreads();  // the window is free for the next tile
  return tot;
}

__global__ void __launch_bounds__(ENC_THREADS) k_enc_size(EncodeArgs a) {
  __shared__ uint32_t sh16[16];
  EncRec r;
  const uint32_t sz = enc_load(a, (uint64_t)blockIdx.x * ENC_THREADS + threadIdx.x, enc_n(a), &r);
  uint32_t tot;
  (void)block_excl_scan(sz, sh16, &tot);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(1024) k_enc_scan(EncodeArgs a, uint32_t nblk) {
  __shared__ uint32_t sh16[16];
  const uint32_t per = (nblk + 1023) / 1024, b0 = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t i = b0; i < b0 + per && i < nblk; ++i) sum += a.bsum[i];
  uint32_t tot;
  uint64_t run = block_excl_scan(sum, sh16, &tot);  // total bytes < 2^32 (hb_encode bounds cap)
  for (uint32_t i = b0; i < b0 + per && i < nblk; ++i) {
    a.bbase[i] = run;
    run += a.bsum[i];
  }
  if (threadIdx.x == 0) {
    a.bbase[nblk] = tot;
    a.off[enc_n(a)] = tot;
    *a.total = tot;
  }
}
__global__ void __launch_bounds__(ENC_THREADS) k_enc_write(EncodeArgs a, uint32_t nblk) {
  __shared__ uint32_t sh16[16];
  __shared__ uint4 l_win[(ENC_THREADS / 64) * (ENC_WIN / 16)];
  const bool write = a.bbase[nblk] <= a.bytes_cap;  // else off, status and total only
  (void)enc_tile(a, (uint64_t)blockIdx.x * ENC_THREADS, enc_n(a), a.bbase[blockIdx.x], write, l_win, sh16);
}
// A batch of at most ENC_SMALL_MAX records: all three in one workgroup.
__global__ void __launch_bounds__(ENC_SMALL_THREADS) k_enc_small(EncodeArgs a) {
  __shared__ uint32_t sh16[16];
  __shared__ uint4 l_win[(ENC_SMALL_THREADS / 64) * (ENC_WIN / 16)];
  const uint64_t n = enc_n(a);
  uint32_t sum = 0;
  for (uint64_t i = threadIdx.x; i < n; i += ENC_SMALL_THREADS) {
    EncRec r;
    sum += enc_load(a, i, n, &r);
  }
  uint32_t tot;
  (void)block_excl_scan(sum, sh16, &tot);
  if (threadIdx.x == 0) {
    a.off[n] = tot;
    *a.total = tot;
  }
  const bool write = tot <= a.bytes_cap;
  uint64_t base = 0;
  for (uint64_t i0 = 0; i0 < n; i0 += ENC_SMALL_THREADS) base += enc_tile(a, i0, n, base, write, l_win, sh16);
}

// hb_encode_ents: hb_encode with a covered MsgApp written whole, its entries
// gathered from the caller's window table.  The same three passes, sizes and offsets 64-bit.
// The write pass has two regimes, chosen per wave (uniformly): a wave whose 64 records span at
// most ENCE_WIN - 16 bytes composes them in its LDS window, payload bytes included, and stores
// the span as enc_tile does; a longer span is written in place, every lane its own prefix,
// entry heads, payloads below ENCE_COOP bytes and suffix, and then the wave copies the
// payloads of ENCE_COOP bytes and more together, record by record (wo_copy_lane).
struct EnceArgs {
  EncodeArgs e;  // bsum / bbase unused: the sums here are 64-bit
  const uint32_t* group;
  uint32_t capacity;
  const uint64_t* first;
  const uint32_t* count;
  const uint64_t* start;
  uint64_t n_ent;
  const uint64_t* eterm;
  const uint32_t* edesc;
  const uint64_t* edata;
  const uint8_t* data;
  uint64_t data_len;
  uint64_t* bsum;   // [blocks]
  uint64_t* bbase;  // [blocks + 1]
};
// 64 records of 96 bytes: a wave of cfg2's MsgApps with one 16-byte entry (68 bytes each, about
// 4.4 KB) fits, and so does any wave without a covered record (64 x WO_MAX).  4 waves x 6,160 B
// = 24,640 B a workgroup: 6 workgroups in a CU's 160 KB.
constexpr uint32_t ENCE_WIN = 64 * 96 + 16;
constexpr uint32_t ENCE_COOP = 256;  // a payload this long is copied by the whole wave
static_assert(ENCE_WIN % 16 == 0 && ENCE_WIN >= ENC_WIN, "read back as uint4; a payload-free wave always fits");
static_assert(ENC_SMALL_THREADS / 64 * ENCE_WIN <= 64 * 1024, "k_ence_small's windows fit static LDS");

struct EnceRec {
  EncRec r;
  bool cov;      // its entries are written here (else the split form, or no entries at all)
  uint64_t pos;  // place of entry index + 1 in the per-entry arrays
  uint64_t ne;   // entries carried
};
// record i, whether it is covered, and its encoded length
__device__ __forceinline__ uint64_t ence_load(const EnceArgs& a, uint64_t i, uint64_t n, EnceRec* x) {
  const uint32_t sz = enc_load(a.e, i, n, &x->r);
  x->cov = false;
  x->pos = x->ne = 0;
  // a MsgProp's (index, hint] is (0, arrival index], not an index range: never covered
  if (!x->r.ents || x->r.type == HB_MSG_PROP) return sz;
  const uint32_t g = a.group[i];
  if (g >= a.capacity) return sz;
  uint64_t run = 0;
  if (!wo_ents_covered(x->r.index, a.e.hint[i], a.first[g], a.count[g], a.start[g], a.n_ent, a.eterm, a.edesc, a.edata,
                       a.data_len, &x->pos, &x->ne, &run))
    return sz;
  x->cov = true;
  x->r.ents = false;  // (status HB_WIRE_OK)
  return sz + run;
}
// The record's bytes at dst: LDS in the short regime (coop = no limit: every payload is copied
// here), global memory in the long one (payloads of `coop` bytes and more are left to the wave).
// Returns whether a payload was left.
__device__ __forceinline__ bool ence_put(const EnceArgs& a, const EnceRec& x, uint8_t* dst, uint32_t coop) {
  const EncRec& r = x.r;
  if (!x.cov) {
    wo_write(dst, r.type, r.to, a.e.self_id, r.term, r.log_term, r.index, r.commit, r.reject, r.hint);
    return false;
  }
  bool left = false;
  dst += wo_write_prefix(dst, r.type, r.to, a.e.self_id, r.term, r.log_term, r.index);
  for (uint64_t k = 0; k < x.ne; ++k) {
    const uint32_t desc = a.edesc[x.pos + k];
    dst += wo_entry_head(dst, desc, a.eterm[x.pos + k], r.index + 1 + k);
    if (wo_desc_has_data(desc)) {
      const uint32_t len = wo_desc_len(desc);
      if (len >= coop) {
        left = true;
      } else {
        const uint8_t* s = a.data + a.edata[x.pos + k];
        for (uint32_t j = 0; j < len; ++j) dst[j] = s[j];
      }
      dst += len;
    }
  }
  wo_write_suffix(dst, r.commit);
  return left;
}
// One tile of blockDim.x records from i0, whose first byte is `base` (enc_tile's contract).
__device__ __forceinline__ uint64_t ence_tile(const EnceArgs& a, uint64_t i0, uint64_t n, uint64_t base, bool write,
                                              uint4* l_win, uint64_t* sh16) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t i = i0 + threadIdx.x;
  EnceRec x;
  const uint64_t sz = ence_load(a, i, n, &x);
  uint64_t tot;
  const uint64_t p = base + block_excl_scan64(sz, sh16, &tot);
  if (i < n) {
    a.e.off[i] = p;
    uint8_t st = x.r.host ? (uint8_t)HB_WIRE_HOST : (uint8_t)HB_WIRE_OK;
    if (x.r.ents)
      st = (uint8_t)(HB_WIRE_SPLICE | wo_prefix_len(x.r.type, x.r.to, a.e.self_id, x.r.term, x.r.log_term, x.r.index));
    a.e.status[i] = st;
  }
  if (!write) return tot;
  const uint64_t lo = __shfl(p, 0), hi = __shfl(p + sz, 63);  // the wave's span
  const bool fits = hi - lo <= ENCE_WIN - 16;  // short span: compose in LDS, store coalesced
  uint4* wwin = l_win + (size_t)wave * (ENCE_WIN / 16);
  uint8_t* win = reinterpret_cast<uint8_t*>(wwin);
  const uintptr_t A = reinterpret_cast<uintptr_t>(a.e.bytes) + lo, B = reinterpret_cast<uintptr_t>(a.e.bytes) + hi;
  const uintptr_t b16 = A & ~(uintptr_t)15;
  if (fits) {
    if (sz) (void)ence_put(a, x, win + (A - b16) + (p - lo), 0xFFFFFFFFu);
  } else {  // long span: in place, then the long payloads by the whole wave
    const bool left = sz ? ence_put(a, x, a.e.bytes + p, ENCE_COOP) : false;
    uint64_t todo = __ballot(left);
    while (todo) {
      const int l = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t pos = __shfl(x.pos, l), ne = __shfl(x.ne, l), index = __shfl(x.r.index, l);
      uint64_t cur = __shfl(p + wo_prefix_len(x.r.type, x.r.to, a.e.self_id, x.r.term, x.r.log_term, x.r.index), l);
      for (uint64_t k = 0; k < ne; ++k) {  // (uniform: every lane walks record l's entries)
        const uint32_t desc = a.edesc[pos + k];
        cur += wo_entry_head_len(desc, a.eterm[pos + k], index + 1 + k);
        if (wo_desc_has_data(desc)) {
          const uint32_t len = wo_desc_len(desc);
          if (len >= ENCE_COOP) wo_copy_lane(a.data + a.edata[pos + k], a.e.bytes + cur, len, lane, 64);
          cur += len;
        }
      }
    }
  }
  __syncthreads();
  if (fits && hi > lo) {
    const uintptr_t A16 = (A + 15) & ~(uintptr_t)15, B16 = B & ~(uintptr_t)15;
    if (A16 < B16) {
      const uint32_t nc = (uint32_t)((B16 - A16) >> 4), c0 = (uint32_t)((A16 - b16) >> 4);
      for (uint32_t c = lane; c < nc; c += 64) reinterpret_cast<uint4*>(A16)[c] = wwin[c0 + c];
      for (uintptr_t y = A + lane; y < A16; y += 64) *reinterpret_cast<uint8_t*>(y) = win[y - b16];
      for (uintptr_t y = B16 + lane; y < B; y += 64) *reinterpret_cast<uint8_t*>(y) = win[y - b16];
    } else {
      for (uintptr_t y = A + lane; y < B; y += 64) *reinterpret_cast<uint8_t*>(y) = win[y - b16];
    }
  }
  __syncthreads();  // the windows are free for the next tile
  return tot;
}

__global__ void __launch_bounds__(ENC_THREADS) k_ence_size(EnceArgs a) {
  __shared__ uint64_t sh16[16];
  EnceRec x;
  const uint64_t sz = ence_load(a, (uint64_t)blockIdx.x * ENC_THREADS + threadIdx.x, enc_n(a.e), &x);
  uint64_t tot;
  (void)block_excl_scan64(sz, sh16, &tot);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(1024) k_ence_scan(EnceArgs a, uint32_t nblk) {
  __shared__ uint64_t sh16[16];
  const uint32_t per = (nblk + 1023) / 1024, b0 = threadIdx.x * per;
  uint64_t sum = 0;
  for (uint32_t i = b0; i < b0 + per && i < nblk; ++i) sum += a.bsum[i];
  uint64_t tot;
  uint64_t run = block_excl_scan64(sum, sh16, &tot);
  for (uint32_t i = b0; i < b0 + per && i < nblk; ++i) {
    a.bbase[i] = run;
    run += a.bsum[i];
  }
  if (threadIdx.x == 0) {
    a.bbase[nblk] = tot;
    a.e.off[enc_n(a.e)] = tot;
    *a.e.total = tot;
  }
}
__global__ void __launch_bounds__(ENC_THREADS) k_ence_write(EnceArgs a, uint32_t nblk) {
  __shared__ uint64_t sh16[16];
  __shared__ uint4 l_win[(ENC_THREADS / 64) * (ENCE_WIN / 16)];
  const bool write = a.bbase[nblk] <= a.e.bytes_cap;  // else off, status and total only
  (void)ence_tile(a, (uint64_t)blockIdx.x * ENC_THREADS, enc_n(a.e), a.bbase[blockIdx.x], write, l_win, sh16);
}
// A batch of at most ENC_SMALL_MAX records: all three in one workgroup.
__global__ void __launch_bounds__(ENC_SMALL_THREADS) k_ence_small(EnceArgs a) {
  __shared__ uint64_t sh16[16];
  __shared__ uint4 l_win[(ENC_SMALL_THREADS / 64) * (ENCE_WIN / 16)];
  const uint64_t n = enc_n(a.e);
  uint64_t sum = 0;
  for (uint64_t i = threadIdx.x; i < n; i += ENC_SMALL_THREADS) {
    EnceRec x;
    sum += ence_load(a, i, n, &x);
  }
  uint64_t tot;
  (void)block_excl_scan64(sum, sh16, &tot);
  if (threadIdx.x == 0) {
    a.e.off[n] = tot;
    *a.e.total = tot;
  }
  const bool write = tot <= a.e.bytes_cap;
  uint64_t base = 0;
  for (uint64_t i0 = 0; i0 < n; i0 += ENC_SMALL_THREADS) base += ence_tile(a, i0, n, base, write, l_win, sh16);
}

// hb_egress: the last step's event words -> an hb_out_batch.  One workgroup
// per partition (its P chunk, then its M chunk), one lane per group.  The
// words of a chunk interleave the partition's groups in emission order, and a
// record's place in the output is fixed by its word's place in the chunk: a
// per-word record count (1 for a response or a heartbeat, in vote mode 1 for
// a vote and the mask's population for a vote broadcast, in append mode the
// same for HB_EV_APP and EVC_BCAST; the engine emits
// nothing for a group after its HB_EV_FAULT), a block scan per tile, a
// running base per chunk, chunk bases from a scan over the chunks.  A chunk
// goes through LDS in tiles of EG_TILE words; every lane then walks the tile's
// group bytes (16 per LDS broadcast read) and consumes its own group's words
// in order, carrying (term, last, pend) in registers across tiles and chunks
// (vote mode: lt too; append mode: lt, cm, bl, blt).
struct EgressArgs {
  const uint64_t* ev;
  const uint64_t* ev_off;
  const uint32_t* ev_counts;
  uint32_t nc, G;
  const uint64_t *term0, *last0, *peer;
  const uint64_t* lterm0;  // [G] vote / append mode: lastTerm before the step, or HB_LT_UNKNOWN (else null)
  // append mode (else null): committed before the step, and the boundary pair: the index just
  // below the current-term run and its term (HB_LT_UNKNOWN: not known to the device)
  const uint64_t *commit0, *bl0, *blt0;
  uint64_t max_msg_size;
  const uint64_t *szx, *szlo;  // CUT only (else null): the groups' size rings as they stand at hb_egress
  const uint64_t *trx, *trc;   // LT only (else null): the groups' older-runs rings as they stand at hb_egress
  uint32_t* ccnt;    // [nc] records per chunk
  uint64_t* cbase;   // [nc + 1] their exclusive scan, then the total
  uint64_t cap;
  uint64_t* count;
  uint32_t *o_group, *o_info;
  uint64_t *o_to, *o_term, *o_log_term, *o_index, *o_commit, *o_hint;
};
constexpr uint64_t HB_LT_UNKNOWN = ~0ull;  // lterm0 / the replay's lastTerm: not known to the device
constexpr uint32_t EG_TILE = 2048;  // words of a chunk in LDS at a time (8 per lane)
constexpr uint32_t EG_PER = EG_TILE / PART;
constexpr uint32_t EG_SMALL = 1024;  // chunks the one-workgroup count + scan takes
static_assert(EG_PER == 8, "a lane's group bytes of a tile are one 8-byte LDS store");

// The records a word makes.  VOTES (hb_set_egress bit HB_EGRESS_VOTES): campaign's MsgVotes too,
// one for an HB_EV_VOTE word and one per slot of an EVC_VBCAST word's mask.  APPS (bit
// HB_EGRESS_APPS): sendAppend's MsgApps too, one for an HB_EV_APP word and one per slot of an
// EVC_BCAST word's mask.  FWD (hb_set_wire_props bit HB_WIRE_PROPS_OUT): stepFollower's forwarded
// MsgProp too, one for an HB_EV_PROP_FWD word.
template <bool VOTES, bool APPS, bool FWD>
__device__ __forceinline__ uint32_t eg_record(uint64_t w) {
  const uint32_t t = (uint32_t)w & 0xF;
  if (FWD && t == HB_EV_PROP_FWD) return 1u;
  if (APPS) {
    if (t == EVC_BCAST) return (uint32_t)__popc((uint32_t)(w >> 4) & 0x7Fu);
    if (t == HB_EV_APP) return 1u;
  }
  if (VOTES) {
    if (t == EVC_VBCAST) return (uint32_t)__popc((uint32_t)(w >> 4) & 0x7Fu);
    if (t == HB_EV_VOTE) return 1u;
  }
  return (t == HB_EV_RESP || t == HB_EV_HEARTBEAT) ? 1u : 0u;
}
template <bool VOTES, bool APPS, bool FWD>
__global__ void __launch_bounds__(256) k_eg_count(EgressArgs a) {
  __shared__ uint32_t sh16[16];
  const uint32_t c = blockIdx.x, n = a.ev_counts[c];
  const uint64_t* src = a.ev + a.ev_off[c];
  uint32_t k = 0;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) k += eg_record<VOTES, APPS, FWD>(src[i]);
  uint32_t tot;
  (void)block_excl_scan(k, sh16, &tot);
  if (threadIdx.x == 0) a.ccnt[c] = tot;
}
__global__ void __launch_bounds__(1024) k_eg_scan(EgressArgs a) {
  __shared__ uint32_t sh16[16];
  const uint32_t n = a.nc, per = (n + 1023) / 1024, b0 = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t i = b0; i < b0 + per && i < n; ++i) sum += a.ccnt[i];
  uint32_t tot;
  uint64_t run = block_excl_scan(sum, sh16, &tot);  // total events < 2^32
  for (uint32_t i = b0; i < b0 + per && i < n; ++i) {
    a.cbase[i] = run;
    run += a.ccnt[i];
  }
  if (threadIdx.x == 0) {
    a.cbase[n] = tot;
    *a.count = tot;
  }
}
// Count and scan in one workgroup when the chunks are few: a wave per chunk counts.
template <bool VOTES, bool APPS, bool FWD>
__global__ void __launch_bounds__(1024) k_eg_small(EgressArgs a) {
  __shared__ uint32_t sh16[16];
  __shared__ uint32_t s_cnt[EG_SMALL];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (uint32_t c = wave; c < a.nc; c += 16) {
    const uint32_t n = a.ev_counts[c];
    const uint64_t* src = a.ev + a.ev_off[c];
    uint32_t k = 0;
    for (uint32_t i = lane; i < n; i += 64) k += eg_record<VOTES, APPS, FWD>(src[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) k += __shfl_xor(k, d);
    if (lane == 0) s_cnt[c] = k;
  }
  __syncthreads();
  const uint32_t c = tid < a.nc ? s_cnt[tid] : 0u;
  uint32_t tot;
  const uint32_t run = block_excl_scan(c, sh16, &tot);
  if (tid < a.nc) a.cbase[tid] = run;
  if (tid == 0) {
    a.cbase[a.nc] = tot;
    *a.count = tot;
  }
}

// CUT (hb_set_egress_limit on an append-mode handle with a finite max_msg_size):
// a MsgApp with entries takes limitSize's cut from the group's size ring instead of the flag,
// unless the ring no longer holds cum(x) or the group has a follower append / restore anywhere in
// the call's events.  The record count of a word does not depend on it, so the count kernels do
// not take the parameter.
// LT (hb_set_egress_logterm on an append-mode handle): an aux = 0 MsgApp that is
// not at the boundary takes its LogTerm from the group's older-runs ring instead of the flag,
// unless the ring no longer reaches down to its Index or the group has a follower append / restore
// anywhere in the call's events (the same look-ahead as CUT's, made once for both).
template <bool VOTES, bool APPS, bool CUT, bool FWD, bool LT>
__global__ void __launch_bounds__(PART) k_egress(EgressArgs a) {
  static_assert(APPS || !CUT, "the cut is a MsgApp's");
  static_assert(APPS || !LT, "the LogTerm lookup is a MsgApp's");
  __shared__ uint64_t s_w[EG_TILE];
  __shared__ uint32_t s_pos[EG_TILE];
  __shared__ uint4 s_key[EG_TILE / 16];
  __shared__ uint32_t sh16[16];
  const uint32_t tid = threadIdx.x, part = blockIdx.x, g = part * PART + tid;
  const bool live = g < a.G;
  // CUT: the group's size ring as it stands now (rule (i)), read once: the replay below visits a
  // wave's sends one lane at a time, and a load there would be waited for at every visit.  The
  // extent word is 0 where the ring cannot be trusted (rule (ii): the in-order replay has no
  // look-ahead, so the partition's words are read once before it; a plain same-value byte store)
  // LT: likewise the two words of the group's older-runs ring; the count word is 0 (no run: every
  // lookup fails, rule (i)) where rule (ii) holds.  Only the search itself, dependent loads from
  // the ring, stands in the send's rare sub-branch.
  uint64_t sx = 0, slo = 0, tx = 0, tc = 0;
  if (CUT || LT) {
    if (CUT && live) {
      sx = a.szx[g];
      slo = a.szlo[g];
    }
    if (LT && live) {
      tx = a.trx[g];
      tc = a.trc[g];
    }
    __shared__ uint8_t s_fol[256];  // by a word's group byte
    static_assert(PART <= 256, "a word's group byte names a lane of the partition");
    for (uint32_t i = tid; i < 256; i += PART) s_fol[i] = 0;
    __syncthreads();
    for (uint32_t c = 2 * part; c < 2 * part + 2; ++c) {
      const uint32_t n = a.ev_counts[c];
      const uint64_t* src = a.ev + a.ev_off[c];
      for (uint32_t i = tid; i < n; i += PART) {
        const uint64_t w = src[i];
        const uint32_t aux = (uint32_t)(w >> 12) & 0xF;
        // (an EVC_CONT word has another type: its bits 4.. are value bits, its group byte is 0)
        if (((uint32_t)w & 0xF) == HB_EV_FOLLOW && (aux == HB_FOLLOW_APPEND || aux == HB_FOLLOW_RESTORE))
          s_fol[(uint32_t)(w >> 16) & 0xFF] = 1;
      }
    }
    __syncthreads();
    if (s_fol[tid] != 0) {
      if (CUT) sx = 0;
      if (LT) tc = 0;
    }
  }
  uint64_t term = live ? a.term0[g] : 0ull, last = live ? a.last0[g] : 0ull;
  uint64_t lt = 0;  // VOTES: raftLog.lastTerm() at this point of the replay, or HB_LT_UNKNOWN
  if (VOTES || APPS) lt = live ? a.lterm0[g] : 0ull;
  // APPS: raftLog.committed, and the boundary pair (the index just below the current-term run,
  // HB_NO_INDEX: unknown; its term, or HB_LT_UNKNOWN) at this point of the replay
  uint64_t cm = 0, bl = HB_NO_INDEX, blt = HB_LT_UNKNOWN;
  if (APPS && live) {
    cm = a.commit0[g];
    bl = a.bl0[g];
    blt = a.blt0[g];
  }
  bool cm_known = true;
  bool pend = false, dead = false;
  const uint32_t pat = tid * 0x01010101u;
  for (uint32_t c = 2 * part; c < 2 * part + 2; ++c) {
    const uint32_t n = a.ev_counts[c];
    const uint64_t* src = a.ev + a.ev_off[c];
    uint64_t run = a.cbase[c];
    for (uint32_t t0 = 0; t0 < n; t0 += EG_TILE) {
      const uint32_t m = n - t0 < EG_TILE ? n - t0 : EG_TILE;
      // stage: a lane takes EG_PER consecutive words, so one block scan places the tile's records
      uint64_t w[EG_PER];
      uint32_t k = 0;
#pragma unroll
      for (uint32_t j = 0; j < EG_PER; ++j) {
        const uint32_t li = tid * EG_PER + j;
        w[j] = li < m ? src[t0 + li] : (uint64_t)EVC_CONT;
        k += eg_record<VOTES, APPS, FWD>(w[j]);
      }
      uint32_t tot;
      uint32_t pos = block_excl_scan(k, sh16, &tot);
      uint32_t klo = 0, khi = 0;
#pragma unroll
      for (uint32_t j = 0; j < EG_PER; ++j) {
        const uint32_t li = tid * EG_PER + j;
        s_w[li] = w[j];
        s_pos[li] = pos;
        pos += eg_record<VOTES, APPS, FWD>(w[j]);
        const uint32_t kb = (uint32_t)(w[j] >> 16) & 0xFF;
        if (j < 4) klo |= kb << (8 * j);
        else khi |= kb << (8 * (j - 4));
      }
      reinterpret_cast<uint2*>(s_key)[tid] = make_uint2(klo, khi);
      __syncthreads();
      // consume: this lane's words of the tile, in order
      const uint32_t nq = (m + 15) / 16;
      for (uint32_t q = 0; q < nq && !dead; ++q) {
        const uint4 kk = s_key[q];
        const uint32_t kd[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          const uint32_t x = kd[d] ^ pat;
          if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) continue;  // no byte of the four is this lane
          for (uint32_t b = 0; b < 4; ++b) {
            if (((x >> (8 * b)) & 0xFF) != 0 || dead) continue;
            const uint32_t li = q * 16 + d * 4 + b;
            if (li >= m) continue;
            const uint64_t ww = s_w[li];
            const uint32_t type = (uint32_t)ww & 0xF, to = (uint32_t)(ww >> 4) & 0x7F, aux = (uint32_t)(ww >> 12) & 0xF;
            if (type == EVC_CONT) continue;  // (its group byte is 0: lane 0 meets them)
            uint64_t xv = ww >> 24;
            if ((ww >> 11) & 1u) {  // the continuation word follows in the chunk
              const uint64_t cw = li + 1 < m ? s_w[li + 1] : (t0 + li + 1 < n ? src[t0 + li + 1] : 0ull);
              xv |= (cw >> 4) << 40;
            }
            if (type == HB_EV_TERM) {
              term = xv;
              if (APPS) {  // reset: the current-term run is empty, the log is unchanged
                bl = pend ? HB_NO_INDEX : last;
                blt = lt;
              }
            } else if (APPS && type == HB_EV_COMMIT) {
              cm = xv;
              cm_known = true;
            } else if (type == HB_EV_LAST) {
              last = xv;
              if (VOTES || APPS) lt = term;  // appendEntry: the group's own entries carry its Term
            } else if (type == HB_EV_FOLLOW) {
              const bool app = aux == HB_FOLLOW_APPEND || aux == HB_FOLLOW_RESTORE;
              pend |= app;
              if ((VOTES || APPS) && app) lt = HB_LT_UNKNOWN;  // the events hold no terms of a leader's entries
              if (APPS && app) {  // ... nor where the current-term run now starts
                bl = HB_NO_INDEX;
                blt = HB_LT_UNKNOWN;
                cm_known = false;  // until the next HB_EV_COMMIT
              }
            } else if (type == HB_EV_FAULT) dead = true;
            else if (FWD && type == HB_EV_PROP_FWD) {
              // stepFollower's forward (raft/raft.go:616-624): send leaves a MsgProp's Term at 0
              // (:226-236); the entries are the host's, named by the arrival index in hint
              const uint64_t o = run + s_pos[li];
              if (o < a.cap) {
                const bool slot = to <= HB_REF_SLOT_MAX;
                a.o_group[o] = g;
                a.o_info[o] = HB_INFO(HB_MSG_PROP, slot ? to : (uint32_t)HB_REF_OTHER, false) | (uint32_t)HB_OUT_ENTS;
                a.o_to[o] = slot ? a.peer[(size_t)g * HB_PEER_ROW + to] : 0ull;
                a.o_term[o] = 0;
                a.o_log_term[o] = 0;
                a.o_index[o] = 0;
                a.o_commit[o] = 0;
                a.o_hint[o] = xv;
              }
            } else if (APPS && (type == HB_EV_APP || type == EVC_BCAST)) {
              // sendAppend's MsgApp (raft/raft.go:261-281): one record per slot, in slot order.
              // LogTerm: the Term when the aux bit says so, the boundary's term for a send at the
              // boundary; anything the replay cannot prove leaves the record to the host.
              const bool at_bl = bl != HB_NO_INDEX && xv == bl && blt != HB_LT_UNKNOWN;
              bool lt_known = (aux & 1u) || at_bl;
              uint64_t lterm = (aux & 1u) ? term : blt;
              if (LT && !lt_known) {  // below the boundary: Runs::find over the ring as it stands now
                Runs r;
                r.R = lx_base(tx);
                r.mask = lx_cap(tx) - 1;
                r.n = (uint32_t)tc;
                r.h = (uint32_t)(tc >> 32);
                lt_known = true;
                lterm = r.find(xv, &lt_known);
              }
              bool host = !lt_known || !cm_known;
              const bool ents = xv < last;  // entries (x, L]
              uint64_t L = 0;
              if (ents) {
                if (CUT) {  // (launched only under a finite limit) limitSize's cut, from the ring
                  if (sx == 0 || xv < slo) host = true;
                  else if (xv + 1 == last) L = last;  // the first entry always goes: no sum is read
                  else if (!host) L = sz_cut(sx, a.max_msg_size, xv + 1, last);
                } else if (a.max_msg_size == HB_NO_LIMIT) L = last;
                else if (a.max_msg_size == 0) L = xv + 1;
                else host = true;  // limitSize's cut: no event carries it
              }
              const uint32_t flags = host ? (uint32_t)HB_OUT_HOST : (ents ? (uint32_t)HB_OUT_ENTS : 0u);
              uint32_t mask = type == EVC_BCAST ? to : 1u << (to <= HB_REF_SLOT_MAX ? to : 7u);
              for (uint64_t o = run + s_pos[li]; mask && o < a.cap; mask &= mask - 1, ++o) {
                const uint32_t s = (uint32_t)__ffs(mask) - 1;
                const bool slot = s <= HB_REF_SLOT_MAX;  // (no lane sends a MsgApp outside prs)
                a.o_group[o] = g;
                a.o_info[o] = HB_INFO(HB_MSG_APP, slot ? s : (uint32_t)HB_REF_OTHER, false) | flags;
                a.o_to[o] = slot ? a.peer[(size_t)g * HB_PEER_ROW + s] : 0ull;
                a.o_term[o] = term;
                a.o_log_term[o] = host ? 0ull : lterm;
                a.o_index[o] = xv;
                a.o_commit[o] = host ? 0ull : cm;
                a.o_hint[o] = host ? 0ull : L;
              }
            } else if (VOTES && (type == HB_EV_VOTE || type == EVC_VBCAST)) {
              // campaign's MsgVote (raft/raft.go:429-443): one record per slot, in slot order; a
              // LogTerm the replay cannot tell leaves the record to the host (HB_OUT_HOST)
              const bool known = lt != HB_LT_UNKNOWN;
              uint32_t mask = type == EVC_VBCAST ? to : 1u << (to <= HB_REF_SLOT_MAX ? to : 7u);
              for (uint64_t o = run + s_pos[li]; mask && o < a.cap; mask &= mask - 1, ++o) {
                const uint32_t s = (uint32_t)__ffs(mask) - 1;
                const bool slot = s <= HB_REF_SLOT_MAX;  // (no lane sends a MsgVote outside prs)
                a.o_group[o] = g;
                a.o_info[o] = HB_INFO(HB_MSG_VOTE, slot ? s : (uint32_t)HB_REF_OTHER, false) |
                              (known ? 0u : (uint32_t)HB_OUT_HOST);
                a.o_to[o] = slot ? a.peer[(size_t)g * HB_PEER_ROW + s] : 0ull;
                a.o_term[o] = term;
                a.o_log_term[o] = known ? lt : 0ull;
                a.o_index[o] = xv;
                a.o_commit[o] = 0;
                a.o_hint[o] = 0;
              }
            } else if (type == HB_EV_RESP || type == HB_EV_HEARTBEAT) {
              uint32_t mtype = HB_MSG_HEARTBEAT;
              uint64_t index = 0, commit = 0, hint = 0;
              bool reject = false;
              if (type == HB_EV_HEARTBEAT) {
                commit = xv;
              } else {
                const uint32_t kind = aux & 7u;
                reject = (aux & HB_RESP_REJECT) != 0;
                mtype = kind == HB_RESP_APP ? HB_MSG_APP_RESP
                                            : (kind == HB_RESP_HEARTBEAT ? HB_MSG_HEARTBEAT_RESP : HB_MSG_VOTE_RESP);
                if (kind == HB_RESP_APP) {
                  index = xv;
                  if (reject) {
                    hint = last;  // handleAppendEntries raft/raft.go:661-663
                  } else if (pend) {
                    last = xv;  // lastnewi of the append / the restored snapshot's index
                    pend = false;
                  }
                }
              }
              const uint64_t o = run + s_pos[li];
              if (o < a.cap) {
                const bool slot = to <= HB_REF_SLOT_MAX;
                a.o_group[o] = g;
                a.o_info[o] = HB_INFO(mtype, slot ? to : (uint32_t)HB_REF_OTHER, reject);
                a.o_to[o] = slot ? a.peer[(size_t)g * HB_PEER_ROW + to] : 0ull;
                a.o_term[o] = term;
                a.o_log_term[o] = 0;
                a.o_index[o] = index;
                a.o_commit[o] = commit;
                a.o_hint[o] = hint;
              }
            }
          }
        }
      }
      __syncthreads();  // the tile is consumed
      run += tot;
    }
  }
}

// The pre-step snapshot of the term and last columns (hb_set_egress).  VOTES: also
// lterm0 = raftLog.lastTerm() as Lane::fterm(last) gives it: Term inside the
// current-term run [tfirst, last], else the newest older run of the ring at or
// below last (only those groups read the ring), HB_LT_UNKNOWN when the ring
// does not reach (runs never loaded).
struct SnapArgs {
  const uint64_t *term, *last;
  uint64_t *term0, *last0;
  uint32_t G;
  const uint64_t *tfirst, *trx, *trc;  // VOTES / append mode only
  uint64_t* lterm0;
  const uint64_t *commit, *first;  // append mode only
  uint64_t *commit0, *bl0, *blt0;
};
__device__ __forceinline__ uint64_t eg_last_term(const SnapArgs& a, uint32_t g, uint64_t term, uint64_t last) {
  const uint64_t tf = a.tfirst[g];
  if (tf != HB_NO_INDEX && last >= tf) return term;
  const uint64_t x = a.trx[g], c = a.trc[g];
  Runs r;
  r.R = lx_base(x);
  r.mask = lx_cap(x) - 1;
  r.n = (uint32_t)c;
  r.h = (uint32_t)(c >> 32);
  bool ok = true;
  const uint64_t t = r.find(last, &ok);
  return ok ? t : HB_LT_UNKNOWN;
}
template <bool VOTES>
__global__ void __launch_bounds__(256) k_eg_snap(SnapArgs a) {
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
  const uint32_t G = a.G;
  if (!VOTES) {
    if (i + 1 < G) {
      *reinterpret_cast<uint4*>(a.term0 + i) = *reinterpret_cast<const uint4*>(a.term + i);
      *reinterpret_cast<uint4*>(a.last0 + i) = *reinterpret_cast<const uint4*>(a.last + i);
    } else if (i < G) {
      a.term0[i] = a.term[i];
      a.last0[i] = a.last[i];
    }
    return;
  }
  if (i + 1 < G) {
    const uint4 t = *reinterpret_cast<const uint4*>(a.term + i), l = *reinterpret_cast<const uint4*>(a.last + i);
    *reinterpret_cast<uint4*>(a.term0 + i) = t;
    *reinterpret_cast<uint4*>(a.last0 + i) = l;
    const uint64_t lt0 = eg_last_term(a, i, (uint64_t)t.x | ((uint64_t)t.y << 32), (uint64_t)l.x | ((uint64_t)l.y << 32));
    const uint64_t lt1 = eg_last_term(a, i + 1, (uint64_t)t.z | ((uint64_t)t.w << 32), (uint64_t)l.z | ((uint64_t)l.w << 32));
    *reinterpret_cast<uint4*>(a.lterm0 + i) =
        make_uint4((uint32_t)lt0, (uint32_t)(lt0 >> 32), (uint32_t)lt1, (uint32_t)(lt1 >> 32));
  } else if (i < G) {
    const uint64_t t = a.term[i], l = a.last[i];
    a.term0[i] = t;
    a.last0[i] = l;
    a.lterm0[i] = eg_last_term(a, i, t, l);
  }
}
// Append mode (hb_set_egress bit HB_EGRESS_APPS): term0, last0, lterm0 as above, commit0, and the
// boundary pair: bl0 = the index just below the current-term run (tfirst - 1; with no such run
// the log's last index, where a run would start) and blt0 = its term as Lane::fterm(bl0) gives
// it, HB_LT_UNKNOWN when the ring does not reach or bl0 lies below the log (first - 1 is the
// lowest index with a term).  One group per lane: a group with a current-term run reads its
// ring for blt0, one without reads it once (blt0 = lterm0).
__global__ void __launch_bounds__(256) k_eg_snap_app(SnapArgs a) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.G) return;
  const uint64_t t = a.term[g], l = a.last[g], tf = a.tfirst[g];
  a.term0[g] = t;
  a.last0[g] = l;
  a.commit0[g] = a.commit[g];
  const bool run = tf != HB_NO_INDEX;
  const uint64_t b = run ? tf - 1 : l;  // (tfirst = 0 gives HB_NO_INDEX: below the log)
  uint64_t lt = HB_LT_UNKNOWN, bt = HB_LT_UNKNOWN;
  if (run && l >= tf) lt = t;
  if (lt == HB_LT_UNKNOWN || b + 1 >= a.first[g]) {
    const uint64_t x = a.trx[g], c = a.trc[g];
    Runs r;
    r.R = lx_base(x);
    r.mask = lx_cap(x) - 1;
    r.n = (uint32_t)c;
    r.h = (uint32_t)(c >> 32);
    if (lt == HB_LT_UNKNOWN) {
      bool ok = true;
      const uint64_t v = r.find(l, &ok);
      if (ok) lt = v;
    }
    if (!run) {
      bt = lt;
    } else if (b + 1 >= a.first[g]) {
      bool ok = true;
      const uint64_t v = r.find(b, &ok);
      if (ok) bt = v;
    }
  }
  if (b + 1 < a.first[g]) bt = HB_LT_UNKNOWN;
  a.lterm0[g] = lt;
  a.bl0[g] = b;
  a.blt0[g] = bt;
}

// ============================================================================
// Per-peer egress: hb_egress_bin, hb_peer_spans
// ============================================================================
// A stable multi-split of an hb_out_batch by destination node: at most 256
// bins (the node table of hb_set_egress_peers and "other"), the records of a
// bin in the order they had in the input.  Tiles of BIN_TILE records: a
// histogram pass classifies every record (hipbatch_bin.h, the table in LDS),
// keeps its bin as a key byte and counts the tile's bins; a workgroup per bin
// scans the bin's counts over the tiles; the scatter ranks a tile stably from
// the key bytes (the partition's in-wave ranking: 8 ballots per 64-record
// round, per-wave counters across the waves), stages it in LDS in bin order and
// writes each bin's run of every array contiguously; its first workgroup writes
// bin_off.  A batch of at most ENC_SMALL_MAX records does all of it in one
// workgroup, its key bytes in LDS, and stores from registers.
struct BinArgs {
  const uint32_t *i_group, *i_info;
  const uint64_t *i_to, *i_term, *i_log_term, *i_index, *i_commit, *i_hint;
  uint32_t *o_group, *o_info;
  uint64_t *o_to, *o_term, *o_log_term, *o_index, *o_commit, *o_hint;
  uint32_t* src;          // null: not wanted
  uint64_t* bin_off;      // [np + 2]
  const BinTable* table;  // device copy, ids ascending
  uint32_t np;            // ids in the table; bin np = "other"
  uint32_t cap;
  const uint64_t* n_dev;  // null: cap
  uint8_t* key;           // [cap] the bin of every record (tiled path)
  uint32_t* hist;         // [np + 1][ntiles] counts, then each bin's exclusive scan (tiled path)
  uint32_t* tot;          // [np + 1] records per bin
  uint32_t ntiles;
};
constexpr uint32_t BIN_THREADS = 1024;
constexpr uint32_t BIN_WAVES = BIN_THREADS / 64;
constexpr uint32_t BIN_ROUNDS = 2;
constexpr uint32_t BIN_TILE = BIN_THREADS * BIN_ROUNDS;  // 2048, as the partition's
static_assert(BIN_SLOTS == 256 && BIN_WAVES * BIN_SLOTS % BIN_THREADS == 0, "a key is one byte");

__device__ __forceinline__ uint32_t bin_n(const BinArgs& a) {
  const uint64_t n = a.n_dev ? *a.n_dev : (uint64_t)a.cap;
  return n < a.cap ? (uint32_t)n : a.cap;
}
__device__ __forceinline__ void bin_table_load(const BinArgs& a, uint64_t* s_id, uint8_t* s_bin) {
  for (uint32_t i = threadIdx.x; i < a.np; i += blockDim.x) {
    s_id[i] = a.table->id[i];
    s_bin[i] = a.table->bin[i];
  }
}
// Stable destinations of one tile.  Record (wave, r, lane) of the tile is its
// record wave * 128 + r * 64 + lane, so (wave, round, lane) order is input order.
// s_off[b] = the first output record of the tile's bin b on entry, the one
// after its last on return; s_cnt[b] (optional) = the tile's records of bin b.
// All threads call it; it ends on a barrier.
__device__ __forceinline__ void bin_rank_tile(const uint32_t (&key)[BIN_ROUNDS], const bool (&valid)[BIN_ROUNDS],
                                              uint32_t (*s_wcnt)[BIN_SLOTS], uint32_t* s_off,
                                              uint32_t (&dest)[BIN_ROUNDS], uint32_t* s_cnt = nullptr) {
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (uint32_t k = 0; k < BIN_WAVES * BIN_SLOTS / BIN_THREADS; ++k) (&s_wcnt[0][0])[tid + k * BIN_THREADS] = 0;
  __syncthreads();
  uint32_t vr[BIN_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
    uint64_t peers = __ballot(valid[r]);
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const bool bit = (key[r] >> k) & 1u;
      const uint64_t bk = __ballot(bit);
      peers &= bit ? bk : ~bk;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & lt);
    const uint32_t before = valid[r] ? s_wcnt[wave][key[r]] : 0u;
    vr[r] = before + rank;
    if (valid[r] && rank == 0) s_wcnt[wave][key[r]] = before + (uint32_t)__popcll(peers);
  }
  __syncthreads();
  if (tid < BIN_SLOTS) {  // per bin: prefix over the waves from the bin's start
    uint32_t run = s_off[tid];
#pragma unroll
    for (uint32_t w = 0; w < BIN_WAVES; ++w) {
      const uint32_t c = s_wcnt[w][tid];
      s_wcnt[w][tid] = run;
      run += c;
    }
    if (s_cnt) s_cnt[tid] = run - s_off[tid];
    s_off[tid] = run;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r) dest[r] = valid[r] ? s_wcnt[wave][key[r]] + vr[r] : 0u;
  __syncthreads();  // the counters are free for the next tile
}
struct BinRec {
  uint32_t group, info;
  uint64_t to, term, log_term, index, commit, hint;
};
__device__ __forceinline__ void bin_rec_load(const BinArgs& a, uint32_t i, BinRec* r) {
  r->group = a.i_group[i];
  r->info = a.i_info[i];
  r->to = a.i_to[i];
  r->term = a.i_term[i];
  r->log_term = a.i_log_term[i];
  r->index = a.i_index[i];
  r->commit = a.i_commit[i];
  r->hint = a.i_hint[i];
}
// record i of the input becomes record d of the output (d < n: the scan of n records' counts)
__device__ __forceinline__ void bin_rec_store(const BinArgs& a, uint32_t d, uint32_t i, uint32_t n, const BinRec& r) {
  if (d >= n) return;
  a.o_group[d] = r.group;
  a.o_info[d] = r.info;
  a.o_to[d] = r.to;
  a.o_term[d] = r.term;
  a.o_log_term[d] = r.log_term;
  a.o_index[d] = r.index;
  a.o_commit[d] = r.commit;
  a.o_hint[d] = r.hint;
  if (a.src) a.src[d] = i;
}

__global__ void __launch_bounds__(BIN_THREADS) k_bin_hist(BinArgs a) {
  __shared__ uint64_t s_id[BIN_SLOTS];
  __shared__ uint8_t s_bin[BIN_SLOTS];
  __shared__ uint32_t s_cnt[BIN_SLOTS];
  const uint32_t tid = threadIdx.x, n = bin_n(a), i0 = blockIdx.x * BIN_TILE;
  uint32_t info[BIN_ROUNDS];
  uint64_t to[BIN_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
    const uint32_t i = i0 + r * BIN_THREADS + tid;
    info[r] = i < n ? a.i_info[i] : 0u;
    to[r] = i < n ? a.i_to[i] : 0ull;
  }
  bin_table_load(a, s_id, s_bin);
  if (tid < BIN_SLOTS) s_cnt[tid] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
    const uint32_t i = i0 + r * BIN_THREADS + tid;
    if (i < n) {
      const uint32_t b = bin_of(s_id, s_bin, a.np, info[r], to[r]);
      a.key[i] = (uint8_t)b;
      atomicAdd(&s_cnt[b], 1u);
    }
  }
  __syncthreads();
  if (tid <= a.np) a.hist[(size_t)tid * a.ntiles + blockIdx.x] = s_cnt[tid];
}
// Workgroup b turns bin b's counts of every tile into exclusive per-tile prefixes
// (SCAN_PER tiles per lane per chunk) and writes their total to tot[b], as k_scan_rows.
__global__ void __launch_bounds__(1024) k_bin_scan(BinArgs a) {
  __shared__ uint32_t sh16[16];
  uint32_t* row = a.hist + (size_t)blockIdx.x * a.ntiles;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < a.ntiles; base += 1024 * SCAN_PER) {
    const uint32_t i0 = base + threadIdx.x * SCAN_PER;
    uint32_t v[SCAN_PER], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; ++k) {
      v[k] = i0 + k < a.ntiles ? row[i0 + k] : 0u;
      sum += v[k];
    }
    uint32_t tot;
    uint32_t run = carry + block_excl_scan(sum, sh16, &tot);
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; ++k) {
      if (i0 + k < a.ntiles) row[i0 + k] = run;
      run += v[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) a.tot[blockIdx.x] = carry;
}
// Two u64 columns of the tile through LDS: in at the records' places in bin
// order (p), out at this thread's output places j = r * BIN_THREADS + tid.
__device__ __forceinline__ void bin_stage_swap(uint64_t* st0, uint64_t* st1, const uint32_t (&p)[BIN_ROUNDS],
                                               const bool (&valid)[BIN_ROUNDS], const bool (&ov)[BIN_ROUNDS],
                                               uint64_t (&x)[BIN_ROUNDS], uint64_t (&y)[BIN_ROUNDS]) {
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r)
    if (valid[r]) {
      st0[p[r]] = x[r];
      st1[p[r]] = y[r];
    }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r)
    if (ov[r]) {
      x[r] = st0[r * BIN_THREADS + threadIdx.x];
      y[r] = st1[r * BIN_THREADS + threadIdx.x];
    }
  __syncthreads();
}
// block_excl_scan of two values at once (one set of barriers): v0's exclusive
// prefix is returned with its total, v1's goes to *e1 with its total.
__device__ __forceinline__ uint32_t block_excl_scan2(uint32_t v0, uint32_t v1, uint32_t (*sh)[16], uint32_t* t0,
                                                     uint32_t* e1, uint32_t* t1) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t i0 = wave_incl_scan(v0), i1 = wave_incl_scan(v1);
  if (lane == 63) {
    sh[0][wave] = i0;
    sh[1][wave] = i1;
  }
  __syncthreads();
  if (wave == 0) {
    uint32_t x0 = lane < nw ? sh[0][lane] : 0, x1 = lane < nw ? sh[1][lane] : 0;
    x0 = wave_incl_scan(x0);
    x1 = wave_incl_scan(x1);
    if (lane < nw) {
      sh[0][lane] = x0;
      sh[1][lane] = x1;
    }
  }
  __syncthreads();
  const uint32_t b0 = wave == 0 ? 0 : sh[0][wave - 1], b1 = wave == 0 ? 0 : sh[1][wave - 1];
  *t0 = sh[0][nw - 1];
  *t1 = sh[1][nw - 1];
  __syncthreads();
  *e1 = b1 + i1 - v1;
  return b0 + i0 - v0;
}
// A bin's base is the scan of the bins' totals: every workgroup scans the 256
// words itself, as the radix scatter does, in the barriers of the scan of its
// own tile's counts, and the first one writes bin_off.  The tile goes through
// LDS in bin order, two u64 columns at a time, so that a bin's records of the
// tile leave as one contiguous run per array: storing each record from the
// registers that loaded it cost 1.9 x the kernel at 65 bins and the same at 4
// (DESIGN.md §3.16).
__global__ void __launch_bounds__(BIN_THREADS) k_bin_scatter(BinArgs a) {
  __shared__ uint32_t s_wcnt[BIN_WAVES][BIN_SLOTS];
  __shared__ uint32_t s_off[BIN_SLOTS], s_cnt[BIN_SLOTS], s_dstart[BIN_SLOTS], s_gstart[BIN_SLOTS], sh32[2][16];
  __shared__ uint8_t s_skey[BIN_TILE];
  __shared__ uint64_t st0[BIN_TILE], st1[BIN_TILE];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = bin_n(a);
  uint32_t key[BIN_ROUNDS], dest[BIN_ROUNDS], idx[BIN_ROUNDS];
  bool valid[BIN_ROUNDS];
  BinRec rec[BIN_ROUNDS] = {};
#pragma unroll
  for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
    idx[r] = blockIdx.x * BIN_TILE + wave * (64 * BIN_ROUNDS) + r * 64 + lane;
    valid[r] = idx[r] < n;
    key[r] = valid[r] ? (uint32_t)a.key[idx[r]] : 0u;
    if (valid[r]) bin_rec_load(a, idx[r], &rec[r]);
  }
  const uint32_t btot = tid <= a.np ? a.tot[tid] : 0u;  // (crosses the ranking in flight)
  // s_off: the tile's place inside each bin; dest then counts from the bin's first record
  if (tid < BIN_SLOTS) s_off[tid] = tid <= a.np ? a.hist[(size_t)tid * a.ntiles + blockIdx.x] : 0u;
  bin_rank_tile(key, valid, s_wcnt, s_off, dest, s_cnt);  // (its first barrier orders s_off)
  {
    uint32_t m, base, all;  // the tile's records; this lane's bin's base; the batch's records
    const uint32_t excl = block_excl_scan2(tid < BIN_SLOTS ? s_cnt[tid] : 0u, btot, sh32, &m, &base, &all);
    if (tid < BIN_SLOTS) {
      s_dstart[tid] = excl;                               // the bin's first place in the staged tile
      s_gstart[tid] = base + (s_off[tid] - s_cnt[tid]);   // ... and in the output
    }
    if (blockIdx.x == 0) {
      if (tid <= a.np) a.bin_off[tid] = base;
      if (tid == 0) a.bin_off[a.np + 1] = all;
    }
    __syncthreads();
    uint32_t p[BIN_ROUNDS], od[BIN_ROUNDS];
    bool ov[BIN_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      p[r] = 0;
      if (valid[r]) {  // (s_off[b] is now the end of the tile's run inside bin b)
        p[r] = s_dstart[key[r]] + (dest[r] - (s_off[key[r]] - s_cnt[key[r]]));
        s_skey[p[r]] = (uint8_t)key[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      const uint32_t j = r * BIN_THREADS + tid;
      ov[r] = j < m;
      const uint32_t b = ov[r] ? (uint32_t)s_skey[j] : 0u;
      od[r] = s_gstart[b] + (j - s_dstart[b]);
    }
    uint64_t x[BIN_ROUNDS], y[BIN_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      x[r] = (uint64_t)rec[r].group | ((uint64_t)rec[r].info << 32);
      y[r] = idx[r];
    }
    bin_stage_swap(st0, st1, p, valid, ov, x, y);
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      rec[r].group = (uint32_t)x[r];
      rec[r].info = (uint32_t)(x[r] >> 32);
      idx[r] = (uint32_t)y[r];
      x[r] = rec[r].to;
      y[r] = rec[r].term;
    }
    bin_stage_swap(st0, st1, p, valid, ov, x, y);
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      rec[r].to = x[r];
      rec[r].term = y[r];
      x[r] = rec[r].log_term;
      y[r] = rec[r].index;
    }
    bin_stage_swap(st0, st1, p, valid, ov, x, y);
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      rec[r].log_term = x[r];
      rec[r].index = y[r];
      x[r] = rec[r].commit;
      y[r] = rec[r].hint;
    }
    bin_stage_swap(st0, st1, p, valid, ov, x, y);
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      rec[r].commit = x[r];
      rec[r].hint = y[r];
      if (ov[r]) bin_rec_store(a, od[r], idx[r], n, rec[r]);
    }
  }
}
// A batch of at most ENC_SMALL_MAX records: classify, scan and scatter in one workgroup.
__global__ void __launch_bounds__(BIN_THREADS) k_bin_small(BinArgs a) {
  __shared__ uint64_t s_id[BIN_SLOTS];
  __shared__ uint8_t s_bin[BIN_SLOTS];
  __shared__ uint32_t s_wcnt[BIN_WAVES][BIN_SLOTS];
  __shared__ uint32_t s_off[BIN_SLOTS];
  __shared__ uint8_t s_key[ENC_SMALL_MAX];
  __shared__ uint32_t sh16[16];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t n = min(bin_n(a), ENC_SMALL_MAX);  // (hb_egress_bin sends no larger cap here)
  bin_table_load(a, s_id, s_bin);
  if (tid < BIN_SLOTS) s_off[tid] = 0;
  __syncthreads();
  for (uint32_t i = tid; i < n; i += BIN_THREADS) {
    const uint32_t b = bin_of(s_id, s_bin, a.np, a.i_info[i], a.i_to[i]);
    s_key[i] = (uint8_t)b;
    atomicAdd(&s_off[b], 1u);
  }
  __syncthreads();
  {
    const uint32_t c = tid < BIN_SLOTS ? s_off[tid] : 0u;
    uint32_t tot;
    const uint32_t excl = block_excl_scan(c, sh16, &tot);  // (ends on a barrier: every count is read)
    if (tid < BIN_SLOTS) s_off[tid] = excl;
    if (tid <= a.np) a.bin_off[tid] = excl;
    if (tid == 0) a.bin_off[a.np + 1] = tot;
  }
  for (uint32_t t0 = 0; t0 < n; t0 += BIN_TILE) {
    uint32_t key[BIN_ROUNDS], dest[BIN_ROUNDS], idx[BIN_ROUNDS];
    bool valid[BIN_ROUNDS];
    BinRec rec[BIN_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r) {
      idx[r] = t0 + wave * (64 * BIN_ROUNDS) + r * 64 + lane;
      valid[r] = idx[r] < n;
      key[r] = valid[r] ? (uint32_t)s_key[idx[r]] : 0u;
      if (valid[r]) bin_rec_load(a, idx[r], &rec[r]);
    }
    bin_rank_tile(key, valid, s_wcnt, s_off, dest);
#pragma unroll
    for (uint32_t r = 0; r < BIN_ROUNDS; ++r)
      if (valid[r]) bin_rec_store(a, dest[r], idx[r], n, rec[r]);
  }
}
// span[b] = off[bin_off[b]], b in [0, np + 1]
__global__ void __launch_bounds__(BIN_SLOTS + 64) k_peer_spans(const uint64_t* off, const uint64_t* bin_off,
                                                               uint64_t* span, uint32_t np) {
  const uint32_t b = threadIdx.x;
  if (b <= np + 1) span[b] = off[bin_off[b]];
}

// ============================================================================
// framed peer streams (hb_gid_dir_build / hb_frame / hb_unframe)
// ============================================================================
constexpr uint32_t FRM_THREADS = 256;            // a tile: one row per lane
constexpr uint32_t FRM_WORDS = BIN_SLOTS + 1;    // bin_off / ispan words (n_peers + 2 <= 257); frame bases
constexpr uint32_t FRM_GRID_MAX = 2048;          // workgroups of a grid-stride launch: what 256 CUs hold at once
static_assert(FRM_THREADS == BIN_SLOTS && FR_MAX_FRAMES == BIN_SLOTS, "a lane per bin and per frame");
static_assert(ENC_SMALL_MAX % FRM_THREADS == 0 && ENC_SMALL_MAX / FRM_THREADS <= 64, "the small paths' tiles fit one wave's scan");

// A launch's device counter to the caller's word (device or pinned memory), in
// a launch of its own: a ticket in the counting launch would be one same-address
// atomic per workgroup, and 16,384 of those take longer than the rows do.
__global__ void k_count_out(const uint32_t* ctr, uint32_t* out32, uint64_t* out64) {
  if (out32) *out32 = *ctr;
  if (out64) *out64 = (uint64_t)*ctr;
}

// ---- the directory ---------------------------------------------------------------
__global__ void __launch_bounds__(FRM_THREADS) k_gid_clear(uint64_t* key, uint64_t cap, uint32_t* ctr) {
  for (uint64_t p = (uint64_t)blockIdx.x * FRM_THREADS + threadIdx.x; p < cap; p += (uint64_t)gridDim.x * FRM_THREADS)
    key[p] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) *ctr = 0u;
}
// gid[i] -> i for every non-zero id: the first probe that finds the key empty
// claims it (a 64-bit compare-and-swap) and writes the slot; one that finds the
// id itself is a duplicate and leaves the first claim.
__global__ void __launch_bounds__(FRM_THREADS) k_gid_insert(const uint64_t* gid, uint32_t count, uint64_t* key,
                                                            uint32_t* slot, uint64_t cap, uint32_t* ctr) {
  const uint64_t mask = cap - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * FRM_THREADS + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * FRM_THREADS) {
    const uint64_t id = gid[i];
    if (id == 0) continue;
    uint64_t p = gd_mix(id) & mask;
    for (uint64_t k = 0; k < cap; ++k) {
      const uint64_t was = atomicCAS(reinterpret_cast<unsigned long long*>(key + p), 0ull, (unsigned long long)id);
      if (was == 0) {
        slot[p] = (uint32_t)i;
        break;
      }
      if (was == id) {
        atomicAdd(ctr, 1u);
        break;
      }
      p = (p + 1) & mask;
    }
  }
}

// ---- hb_frame ----------------------------------------------------------------------
struct FrameArgs {
  const uint32_t* group;
  const uint64_t* to;
  const uint64_t* off;
  const uint8_t* status;
  const uint64_t* bin_off;  // [np + 2]
  const uint64_t* span;     // [np + 2]
  const uint64_t* gid;      // [capacity]
  uint32_t capacity, np;
  uint64_t max_rows;        // the handle's largest record batch: a larger bin_off is not believed
  uint64_t self_id, seq;
  uint8_t* index;
  uint64_t index_cap;
  uint64_t* ispan;          // [np + 2]
  uint32_t* fstat;          // [np + 1]
  uint32_t* cnt;            // tiled path: [BIN_SLOTS] holes per bin, then [BIN_SLOTS] oversize flags
};
// bin_off and the frames' places into LDS (all threads; ends on a barrier).
// s_boff[b], b in [0, np + 1]; s_isp[b] = the bytes of the frames before bin b,
// s_isp[np] = s_isp[np + 1] = the total.  A bin_off that does not ascend, or
// ends past max_rows, is read as an empty batch: no row, no frame.
__device__ __forceinline__ void frame_plan(const FrameArgs& a, uint64_t* s_boff, uint64_t* s_isp, uint64_t* sh16) {
  const uint32_t t = threadIdx.x;
  for (uint32_t b = t; b <= a.np + 1; b += FRM_THREADS) s_boff[b] = a.bin_off[b];
  __syncthreads();
  const bool bad = (t <= a.np && s_boff[t] > s_boff[t + 1]) || (t == 0 && s_boff[a.np + 1] > a.max_rows);
  const bool any_bad = __syncthreads_or(bad) != 0;
  if (any_bad)
    for (uint32_t b = t; b <= a.np + 1; b += FRM_THREADS) s_boff[b] = 0;
  __syncthreads();
  uint64_t tot;
  const uint64_t sz = t < a.np ? fr_isize(s_boff[t + 1] - s_boff[t]) : 0ull;
  s_isp[t] = block_excl_scan64(sz, sh16, &tot);  // (t >= np: the total)
  if (t == 0) s_isp[FRM_THREADS] = tot;
  __syncthreads();
}
// Records [i0, i0 + FRM_THREADS) of the binned batch: a lane per record writes
// its row's two words (rows of a bin are consecutive lanes: both stores coalesce)
// and each wave adds its holes to cnt[bin] with one atomic per bin it touches.
__device__ __forceinline__ void frame_tile(const FrameArgs& a, const uint64_t* s_boff, const uint64_t* s_isp,
                                           uint64_t i0, uint64_t n, bool write, uint32_t* cnt) {
  const uint64_t i = i0 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t b = 0;
#pragma unroll
  for (uint32_t step = 128; step >= 1; step >>= 1) {  // bins that end at or before i (bin_lookup's search)
    const uint32_t m = b + step;
    if (m <= a.np && s_boff[m] <= i) b = m;
  }
  const bool live = i < n && b < a.np;  // ("other" gets no frame)
  bool hole = false, over = false;
  if (live) {
    const uint32_t g = a.group[i];
    const bool ok = g < a.capacity;
    const FrRow r = fr_row(a.status[i], ok, ok ? a.gid[g] : 0ull, a.off[i + 1] - a.off[i]);
    hole = (r.len & FR_HOLE) != 0;
    over = r.oversize;
    if (write) {
      const uint64_t c = s_boff[b + 1] - s_boff[b], j = i - s_boff[b];
      uint8_t* f = a.index + s_isp[b];
      *reinterpret_cast<uint64_t*>(f + fr_gid_at(j)) = r.gid;
      *reinterpret_cast<uint32_t*>(f + fr_len_at(c, j)) = r.len;
      if (j + 1 == c && (c & 1)) *reinterpret_cast<uint32_t*>(f + fr_len_at(c, c)) = 0u;
    }
  }
  // the wave's runs of equal bins: the first lane of a run counts it
  const uint32_t key = live ? b : 0xFFFFFFFFu;
  const uint32_t prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const uint64_t hm = __ballot(hole), om = __ballot(over), sm = __ballot(head);
  if (head && live) {
    const uint64_t above = lane == 63 ? 0ull : (sm >> (lane + 1)) << (lane + 1);
    const uint64_t upto = above ? (above & (0ull - above)) - 1 : ~0ull;  // lanes below the next run
    const uint64_t run = upto & ~((1ull << lane) - 1);
    const uint32_t nh = (uint32_t)__popcll(hm & run);
    if (nh) atomicAdd(cnt + b, nh);
    if (om & run) atomicOr(cnt + BIN_SLOTS + b, 1u);
  }
}
// ispan, fstat and the headers: lane b is bin b (one workgroup, after every row).
__device__ __forceinline__ void frame_heads(const FrameArgs& a, const uint64_t* s_boff, const uint64_t* s_isp,
                                            bool write, const uint32_t* cnt) {
  const uint32_t b = threadIdx.x;
  if (b <= a.np + 1) a.ispan[b] = s_isp[b <= a.np ? b : a.np];
  if (b + FRM_THREADS <= a.np + 1) a.ispan[b + FRM_THREADS] = s_isp[a.np];  // (np = 255: word 256)
  if (b == a.np) a.fstat[b] = 0u;
  if (b >= a.np) return;
  const uint64_t c = s_boff[b + 1] - s_boff[b];
  const bool over = cnt[BIN_SLOTS + b] != 0;
  a.fstat[b] = over ? FR_OVERSIZE : cnt[b];
  if (!write || c == 0) return;
  FrHeader h;
  h.magic = over ? 0u : FR_MAGIC;
  h.flags = 0;
  h.from = a.self_id;
  h.to = a.to[s_boff[b]];  // (the bin holds the records whose `to` is ids[b])
  h.seq = a.seq;
  h.bytes = a.span[b + 1] - a.span[b];
  h.count = (uint32_t)c;
  h.holes = cnt[b];
  fr_pack_header(a.index + s_isp[b], h);
}
__global__ void __launch_bounds__(FRM_THREADS) k_frame(FrameArgs a) {
  __shared__ uint64_t s_boff[FRM_WORDS], s_isp[FRM_WORDS], sh16[16];
  frame_plan(a, s_boff, s_isp, sh16);
  const uint64_t n = s_boff[a.np + 1];
  const bool write = s_isp[a.np] <= a.index_cap;
  for (uint64_t i0 = (uint64_t)blockIdx.x * FRM_THREADS; i0 < n; i0 += (uint64_t)gridDim.x * FRM_THREADS)
    frame_tile(a, s_boff, s_isp, i0, n, write, a.cnt);
}
__global__ void __launch_bounds__(FRM_THREADS) k_frame_heads(FrameArgs a) {
  __shared__ uint64_t s_boff[FRM_WORDS], s_isp[FRM_WORDS], sh16[16];
  frame_plan(a, s_boff, s_isp, sh16);
  frame_heads(a, s_boff, s_isp, s_isp[a.np] <= a.index_cap, a.cnt);
}
// A handle whose largest record batch is at most ENC_SMALL_MAX: one workgroup, the counts in LDS.
__global__ void __launch_bounds__(FRM_THREADS) k_frame_small(FrameArgs a) {
  __shared__ uint64_t s_boff[FRM_WORDS], s_isp[FRM_WORDS], sh16[16];
  __shared__ uint32_t s_cnt[2 * BIN_SLOTS];
  s_cnt[threadIdx.x] = 0u;
  s_cnt[threadIdx.x + BIN_SLOTS] = 0u;
  frame_plan(a, s_boff, s_isp, sh16);
  const uint64_t n = s_boff[a.np + 1];
  const bool write = s_isp[a.np] <= a.index_cap;
  for (uint64_t i0 = 0; i0 < n; i0 += FRM_THREADS) frame_tile(a, s_boff, s_isp, i0, n, write, s_cnt);
  __syncthreads();
  frame_heads(a, s_boff, s_isp, write, s_cnt);
}

// ---- hb_unframe --------------------------------------------------------------------
// The frame table the host validated and copied: u64 words, FRM_WORDS bases
// (base[k] = the first output row of frame k, base[nf] = n), then FR_MAX_FRAMES
// words each of index_off, bytes_off, bytes_len and from.
constexpr uint32_t UNF_IOFF = FRM_WORDS, UNF_BOFF = UNF_IOFF + FR_MAX_FRAMES, UNF_BLEN = UNF_BOFF + FR_MAX_FRAMES,
                   UNF_FROM = UNF_BLEN + FR_MAX_FRAMES, UNF_WORDS = UNF_FROM + FR_MAX_FRAMES;
struct UnfArgs {
  const uint8_t* index;
  const uint64_t* ft;  // [UNF_WORDS]
  uint32_t nf;
  uint64_t n, self_id;
  const uint64_t* key;
  const uint32_t* slot;
  uint64_t cap;
  uint64_t* off;
  uint32_t* len;
  uint32_t* group;
  uint32_t* fstatus;    // [nf]
  uint64_t* n_unknown;
  uint64_t* tsum;       // tiled path: [tiles] bytes per tile
  uint64_t* tbase;      // [tiles + 1] their scan
  uint64_t* pbase;      // [nf + 1] bytes before each frame's first row
  uint32_t* fst;        // [nf] fstatus for the write pass
  uint32_t* ctr;        // [1] unknown rows
};
__device__ __forceinline__ void unf_tables(const UnfArgs& a, uint64_t* s_base, uint64_t* s_ioff) {
  for (uint32_t k = threadIdx.x; k <= a.nf; k += blockDim.x) s_base[k] = a.ft[k];
  for (uint32_t k = threadIdx.x; k < a.nf; k += blockDim.x) s_ioff[k] = a.ft[UNF_IOFF + k];
  __syncthreads();
}
// The frame of output row r < n: the bases at or below r, less one (bin_lookup's search).
__device__ __forceinline__ uint32_t unf_frame_of(const uint64_t* s_base, uint32_t nf, uint64_t r) {
  uint32_t k = 0;
#pragma unroll
  for (uint32_t step = 128; step >= 1; step >>= 1) {
    const uint32_t m = k + step;
    if (m < nf && s_base[m] <= r) k = m;
  }
  return k;
}
// Row r's len word (the host checked the frame's extent against the buffer).
__device__ __forceinline__ uint32_t unf_len_word(const UnfArgs& a, const uint64_t* s_base, const uint64_t* s_ioff,
                                                 uint32_t k, uint64_t r) {
  const uint64_t c = s_base[k + 1] - s_base[k];
  return *reinterpret_cast<const uint32_t*>(a.index + s_ioff[k] + fr_len_at(c, r - s_base[k]));
}
__device__ __forceinline__ uint64_t unf_row_bytes(const UnfArgs& a, const uint64_t* s_base, const uint64_t* s_ioff,
                                                  uint64_t r) {
  return unf_len_word(a, s_base, s_ioff, unf_frame_of(s_base, a.nf, r), r) & FR_LEN_MASK;
}
// The bytes of tile t's rows (all threads; the value is the workgroup's).
__device__ __forceinline__ uint64_t unf_tile_sum(const UnfArgs& a, const uint64_t* s_base, const uint64_t* s_ioff,
                                                 uint64_t t, uint64_t* sh16) {
  const uint64_t r = t * FRM_THREADS + threadIdx.x;
  uint64_t tot;
  (void)block_excl_scan64(r < a.n ? unf_row_bytes(a, s_base, s_ioff, r) : 0ull, sh16, &tot);
  return tot;
}
// After the tiles' scan (tbase[0, nt], visible to the workgroup): the bytes
// before every frame's first row, a wave per boundary, then a lane per frame
// checks its header once.  All threads; ends on a barrier.
__device__ __forceinline__ void unf_frames(const UnfArgs& a, const uint64_t* s_base, const uint64_t* s_ioff,
                                           const uint64_t* tbase, uint64_t nt, uint64_t* s_pb, uint32_t* fst) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (uint32_t k = wave; k <= a.nf; k += nw) {
    const uint64_t rb = s_base[k];
    uint64_t p;
    if (rb >= a.n) {
      p = tbase[nt];
    } else {
      const uint64_t t = rb / FRM_THREADS;
      uint64_t s = 0;
      for (uint64_t r = t * FRM_THREADS + lane; r < rb; r += 64) s += unf_row_bytes(a, s_base, s_ioff, r);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
      p = tbase[t] + s;
    }
    if (lane == 0) s_pb[k] = p;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < a.nf; k += blockDim.x) {
    const uint64_t rows = s_base[k + 1] - s_base[k], blen = a.ft[UNF_BLEN + k];
    uint32_t st;
    if (rows == 0) st = blen == 0 ? FR_OK : FR_BAD_LENGTH;  // (no frame: no bytes)
    else st = fr_validate(fr_parse_header(a.index + s_ioff[k]), rows, a.self_id, a.ft[UNF_FROM + k], blen,
                          s_pb[k + 1] - s_pb[k]);
    a.fstatus[k] = st;
    fst[k] = st;
  }
  __syncthreads();
}
// Tile t, whose first row has `before` bytes of all frames in front of it: the
// three output words of every row; cnt takes the rows of an unknown gid.
__device__ __forceinline__ void unf_tile_write(const UnfArgs& a, const uint64_t* s_base, const uint64_t* s_ioff,
                                               const uint64_t* s_pb, const uint32_t* fst, uint64_t t, uint64_t before,
                                               uint64_t* sh16, uint32_t* cnt) {
  const uint64_t r = t * FRM_THREADS + threadIdx.x;
  const bool live = r < a.n;
  uint32_t k = 0, w = 0;
  if (live) {
    k = unf_frame_of(s_base, a.nf, r);
    w = unf_len_word(a, s_base, s_ioff, k, r);
  }
  uint64_t tot;
  const uint64_t p = before + block_excl_scan64(live ? (uint64_t)(w & FR_LEN_MASK) : 0ull, sh16, &tot);
  bool unknown = false;
  if (live) {
    uint64_t o = 0;
    uint32_t l = 0, g = FR_NO_SLOT;
    if (fst[k] == FR_OK) {
      o = a.ft[UNF_BOFF + k] + (p - s_pb[k]);
      const uint64_t id = *reinterpret_cast<const uint64_t*>(a.index + s_ioff[k] + fr_gid_at(r - s_base[k]));
      if (!(w & FR_HOLE) && id != 0) {
        g = gd_lookup(a.key, a.slot, a.cap, id);
        unknown = g == FR_NO_SLOT;
        if (!unknown) l = w & FR_LEN_MASK;
      }
    }
    a.off[r] = o;
    a.len[r] = l;
    a.group[r] = g;
  }
  const uint64_t um = __ballot(unknown);
  if ((threadIdx.x & 63) == 0 && um) atomicAdd(cnt, (uint32_t)__popcll(um));
}
__global__ void __launch_bounds__(FRM_THREADS) k_unf_sum(UnfArgs a) {
  __shared__ uint64_t s_base[FRM_WORDS], s_ioff[FR_MAX_FRAMES], sh16[16];
  unf_tables(a, s_base, s_ioff);
  const uint64_t tot = unf_tile_sum(a, s_base, s_ioff, blockIdx.x, sh16);
  if (threadIdx.x == 0) a.tsum[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(1024) k_unf_scan(UnfArgs a, uint32_t nt) {
  __shared__ uint64_t s_base[FRM_WORDS], s_ioff[FR_MAX_FRAMES], s_pb[FRM_WORDS], sh16[16];
  unf_tables(a, s_base, s_ioff);
  const uint32_t per = (nt + 1023) / 1024, t0 = threadIdx.x * per;
  uint64_t sum = 0;
  for (uint32_t i = t0; i < t0 + per && i < nt; ++i) sum += a.tsum[i];
  uint64_t tot;
  uint64_t run = block_excl_scan64(sum, sh16, &tot);
  for (uint32_t i = t0; i < t0 + per && i < nt; ++i) {
    a.tbase[i] = run;
    run += a.tsum[i];
  }
  if (threadIdx.x == 0) {
    a.tbase[nt] = tot;
    a.ctr[0] = 0u;
  }
  __syncthreads();
  unf_frames(a, s_base, s_ioff, a.tbase, nt, s_pb, a.fst);
  for (uint32_t k = threadIdx.x; k <= a.nf; k += 1024) a.pbase[k] = s_pb[k];
}
__global__ void __launch_bounds__(FRM_THREADS) k_unf_write(UnfArgs a) {
  __shared__ uint64_t s_base[FRM_WORDS], s_ioff[FR_MAX_FRAMES], s_pb[FRM_WORDS], sh16[16];
  __shared__ uint32_t s_fst[FR_MAX_FRAMES];
  unf_tables(a, s_base, s_ioff);
  for (uint32_t k = threadIdx.x; k <= a.nf; k += FRM_THREADS) s_pb[k] = a.pbase[k];
  for (uint32_t k = threadIdx.x; k < a.nf; k += FRM_THREADS) s_fst[k] = a.fst[k];
  __syncthreads();
  unf_tile_write(a, s_base, s_ioff, s_pb, s_fst, blockIdx.x, a.tbase[blockIdx.x], sh16, a.ctr);
}
// At most ENC_SMALL_MAX rows (at most 64 tiles): the three passes in one workgroup.
__global__ void __launch_bounds__(FRM_THREADS) k_unf_small(UnfArgs a, uint32_t nt) {
  __shared__ uint64_t s_base[FRM_WORDS], s_ioff[FR_MAX_FRAMES], s_pb[FRM_WORDS], sh16[16];
  __shared__ uint64_t s_tsum[64], s_tbase[65];
  __shared__ uint32_t s_fst[FR_MAX_FRAMES], s_cnt;
  unf_tables(a, s_base, s_ioff);
  if (threadIdx.x == 0) s_cnt = 0u;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint64_t tot = unf_tile_sum(a, s_base, s_ioff, t, sh16);
    if (threadIdx.x == 0) s_tsum[t] = tot;
  }
  __syncthreads();
  uint64_t tot;
  const uint64_t ex = block_excl_scan64(threadIdx.x < nt ? s_tsum[threadIdx.x] : 0ull, sh16, &tot);
  if (threadIdx.x < nt) s_tbase[threadIdx.x] = ex;
  if (threadIdx.x == 0) s_tbase[nt] = tot;
  __syncthreads();
  unf_frames(a, s_base, s_ioff, s_tbase, nt, s_pb, s_fst);
  for (uint32_t t = 0; t < nt; ++t) unf_tile_write(a, s_base, s_ioff, s_pb, s_fst, t, s_tbase[t], sh16, &s_cnt);
  __syncthreads();
  if (threadIdx.x == 0) *a.n_unknown = (uint64_t)s_cnt;
}

// ============================================================================
// host side
// ============================================================================
// Scratch that is allocated lazily or grown on demand is a DevBuf (hbmem.h):
// it frees itself with its owner, and a failed allocation is HB_ENOMEM.
struct HipDevice {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipFree(p); }
};
struct HipPinned {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipHostFree(p); }
};
template <class T>
using Dev = hbmem::DevBuf<T, HipDevice>;
template <class T>
using Pinned = hbmem::DevBuf<T, HipPinned>;
// reserve() hook: the old block's last reader is a kernel or a copy on `s`
inline auto stream_idle(hipStream_t s) {
  return [s]() -> int {
    HB_CHECK(hipStreamSynchronize(s));
    return HB_OK;
  };
}
// two buffers that exist together: both reserved, or both empty
template <class A, class B>
int reserve_pair(A& a, uint64_t na, B& b, uint64_t nb) {
  if (a.reserve(na) == HB_OK && b.reserve(nb) == HB_OK) return HB_OK;
  a.release();
  b.release();
  return HB_ENOMEM;
}

// What one step's prep (partition + route) hands to its apply.  Two sets, so
// the prep of batch k+1 (on the prep stream) can run while batch k applies.
struct PrepSet {
  MsgRec* rec = nullptr;          // final pass = apply input
  uint8_t* key = nullptr;         // partition-in-bucket per record (+ SEG bytes of padding)
  uint32_t* bucket = nullptr;     // bucket id per record (multi-pass only)
  uint32_t* bk_off = nullptr;     // [NBK + 1]
  uint32_t* bk_fill = nullptr;    // [NBK] event words reserved in each bucket's region (k_route)
  uint32_t* ctr = nullptr;        // [CTR_WORDS] work-list counters + finish ticket (cleared by this set's prep)
  uint8_t* cnt = nullptr;         // [G]
  Dev<uint8_t> dstage;            // device copy of the packed host batch
  uint4* slot = nullptr;          // [route_kmax][G]
  uint64_t* side = nullptr;       // [2 max_batch] long records' (term, index)
  uint4* recx = nullptr;          // X mode: [max_batch] beside rec
  uint4* slotx = nullptr;         // X mode: [route_kmax][G] beside slot
  uint64_t* ev_off = nullptr;     // [2 NB] event chunk offsets (route writes the M chunks)
  uint32_t* ev_counts = nullptr;  // [2 NB]
  hipEvent_t prepped = nullptr;   // prep stream: this set is ready
  hipEvent_t applied = nullptr;   // apply stream: the last apply reading this set is done
  bool used = false;
};

// The log pool: extents of the per-group log index rings (DevState szx / trx),
// power-of-two sizes carved from device slabs, recycled through per-size free
// lists.  Only the host allocates (hb_reserve_log, hb_load_*): the device never
// grows a ring, it relies on the capacity reserved before the step.
struct LogPool {
  std::vector<void*> slabs;
  char* cur = nullptr;
  size_t left = 0;
  std::vector<uint64_t> free_[48];  // by log2(bytes)
  uint64_t bytes_live = 0;
  // an extent of 2^lb bytes (lb >= 7: 128-byte aligned, the extent word's tag bits stay free)
  uint64_t get(uint32_t lb) {
    if (!free_[lb].empty()) {
      const uint64_t a = free_[lb].back();
      free_[lb].pop_back();
      bytes_live += 1ull << lb;
      return a;
    }
    const size_t bytes = 1ull << lb;
    const size_t align = bytes < 4096 ? bytes : 4096;
    size_t pad = (align - (reinterpret_cast<uintptr_t>(cur) & (align - 1))) & (align - 1);
    if (!cur || left < pad + bytes) {
      const size_t slab = std::max<size_t>(bytes, 256ull << 20);
      void* p = nullptr;
      if (hipMalloc(&p, slab) != hipSuccess) return 0;
      slabs.push_back(p);
      cur = static_cast<char*>(p);
      left = slab;
      pad = 0;
    }
    const uint64_t a = reinterpret_cast<uint64_t>(cur + pad);
    cur += pad + bytes;
    left -= pad + bytes;
    bytes_live += bytes;
    return a;
  }
  void put(uint64_t a, uint32_t lb) {
    free_[lb].push_back(a);
    bytes_live -= 1ull << lb;
  }
  void release() {
    for (void* p : slabs) (void)hipFree(p);
    slabs.clear();
  }
};
constexpr uint32_t SZ_LOG_MIN = 4;  // a size ring starts at 16 entries (128 B)
constexpr uint32_t TR_LOG_MIN = 3;  // a run ring at 8 runs (128 B)

struct hb_handle {
  int device = 0;
  hipStream_t stream = nullptr;   // apply stream (hb_set_stream)
  hipStream_t prep = nullptr;     // partition + route (library-owned)
  hipStream_t in_stream = nullptr;  // where the batch inputs are produced (hb_set_input_stream)
  bool in_stream_set = false;
  hipEvent_t in_ready = nullptr;
  uint32_t G = 0, nmax = 0, W = 0, NB = 0;
  uint64_t max_msg_size = 0, max_batch = 0;
  DevState st{};
  std::vector<void*> allocs;
  // the log index (host mirror of DevState szx / trx: extent address | log2 capacity)
  LogPool pool;
  std::vector<uint64_t> h_szx, h_trx;
  Dev<uint64_t> lx_jobs;          // hb_reserve_log's regrow jobs
  // partition scratch
  uint32_t* hist = nullptr;       // [tiles][RDX_BINS]
  uint32_t* n_valid = nullptr;    // messages kept after pass 1 (device)
  uint32_t* totals = nullptr;     // [RDX_BINS] digit totals of the current pass
  // one-pass direct offsets: hist workgroup sums, rotating superblock sums
  uint32_t* hagg = nullptr;       // [hist workgroups][RDX_BINS]
  uint32_t* hsup = nullptr;       // [SUP_BUFS][sup_max][RDX_BINS]
  uint32_t sup_max = 0, sup_k = 0;
  uint32_t sup_used[SUP_BUFS] = {};  // superblocks each buffer holds non-zero (cleared by a later hist)
  RadixDst tmp[2] = {};           // intermediate passes (ping-pong)
  PrepSet set[2];
  uint32_t next_set = 0, cur = 0;  // set of the next / the last step
  uint32_t NBK = 0;               // buckets
  uint32_t sis_log = SIS_LOG_MAX;  // partitions per bucket (log2)
  uint32_t rf_wide = 0;            // the forms of k_route_fast this handle runs wide (route_fast_form bits)
  uint32_t passes = 1;
  // small steps (a few thousand messages, hb_step / hb_events_to_host): one
  // launch for the partition and one for the event words; HB_SMALL_STEP=0
  // turns that off (same output: the A/B and the parity tests compare both)
  bool no_small = false;
  uint32_t kern = 0;  // hb_step_kernels of the last step
  uint32_t fuse = 2;  // k_route_fast: 0 never, 1 one-pass handles, 2 every geometry (HB_ROUTE_FUSE at hb_create)
  uint32_t storm = 2;  // n >= 5: 2: the route's storm hand-over, 0: off (HB_STORM=0 at hb_create)
  bool steady = true;        // n = 3 fast lane: the wave-uniform steady path (HB_FAST_STEADY=0 at hb_create: off)
  bool steady_count = false;  // tests: count the group-waves that take it (HB_FAST_STEADY_COUNT=1 at hb_create)
  uint32_t agrid = 0;  // the apply kernels' grid (apply_grid_for)
  uint32_t bk_bits = 1;            // bits of a bucket id
  // host-pointer staging
  uint32_t* s_group = nullptr;
  uint32_t* s_info = nullptr;
  uint32_t* s_props = nullptr;
  uint64_t* s_term = nullptr;
  uint64_t* s_index = nullptr;
  uint64_t* s_hint = nullptr;
  uint64_t* s_eoff = nullptr;     // [max_batch]
  uint64_t* s_commit = nullptr;   // [max_batch]
  uint64_t* s_peoff = nullptr;    // [G] (finite max_msg_size)
  Dev<uint32_t> s_edesc;          // [n_edesc]
  Dev<uint64_t> s_eterm;          // [n_edesc]
  // events
  uint64_t* ev = nullptr;   // compact event words
  uint64_t ev_region = 0;  // records
  uint32_t ev_per_msg = 0;
  uint64_t* stats_shard = nullptr;  // shard_at(value, shard)
  uint64_t* stats_accum = nullptr;  // optional caller buffer (hb_set_stats_accum)
  Pinned<uint64_t> stats_pin;       // [HB_STAT_COUNT] readback (hb_copy_events' count)
  // host-pointer batches up to STAGE_MAX bytes: packed into one pinned block, one H2D copy
  Pinned<uint8_t> hstage;
  hipEvent_t hstage_done = nullptr; // the last copy out of hstage has completed
  uint64_t* stats = nullptr;
  // fast -> general hand-over
  uint32_t* pflag = nullptr;      // [NB][PART/32]
  uint32_t* ap_list = nullptr;    // [8][NB]
  uint32_t* fl_list = nullptr;    // [NB]
  uint32_t* eflag = nullptr;      // [NB][PART/32] k_elect's groups (n >= 5)
  uint8_t* lskip = nullptr;       // [NB] partitions the route closed (n >= 5 storm hand-over)
  uint32_t* el_list = nullptr;    // [8][NB]
  uint32_t* done = nullptr;       // k_apply workgroups finished this step
  uint32_t* resume = nullptr;     // [G]
  uint64_t* commit0 = nullptr;    // [G]
  Dev<uint64_t> peer;             // [G][HB_PEER_ROW] node ids (hb_load_peers)
  Dev<uint32_t> dec_q;            // hb_decode pass-2 queue (record indices)
  Dev<uint32_t> dec_qn;           // [queue length, finished pass-2 workgroups]
  Dev<uint32_t> decf_sum;         // hb_decode_follow: [workgroups] entries per k_decf_parse workgroup
  Dev<uint64_t> decf_base;        // [workgroups + 1] their scan (grown with decf_sum)
  Dev<uint8_t> evx;               // hb_copy_events expansion scratch (bytes)
  Dev<uint64_t> evw;              // hb_events_to_host: per-chunk word offsets + total
  // wire egress (hb_set_egress / hb_egress / hb_encode): nothing of it exists while egress is off
  bool egress = false;
  bool eg_stepped = false;        // a step or tick has run since hb_set_egress(on)
  bool eg_limit = false;          // hb_set_egress_limit: limitSize's cut at hb_egress (§3.23)
  bool eg_logterm = false;        // hb_set_egress_logterm: a resend's LogTerm from the run ring (§3.25)
  int wire_props = 0;             // hb_set_wire_props: HB_WIRE_PROPS_IN | HB_WIRE_PROPS_OUT (§3.24)
  bool eg_votes = false;          // HB_EGRESS_VOTES: MsgVote records, the lterm0 column
  Dev<uint64_t> lterm0;           // [G] raftLog.lastTerm() before the last step / tick, or HB_LT_UNKNOWN
  bool eg_apps = false;           // HB_EGRESS_APPS: MsgApp records; lterm0 and the three columns below
  Dev<uint64_t> eg_commit0;       // [G] raftLog.committed before it (commit0 above is the step's own)
  Dev<uint64_t> bl0;              // [G] the index just below the current-term run before it
  Dev<uint64_t> blt0;             // [G] that index's term, or HB_LT_UNKNOWN
  Dev<uint64_t> term0;            // [G] the term column before the last step / tick
  Dev<uint64_t> last0;            // [G] the last column before it
  Dev<uint32_t> eg_cnt;           // [2 NB] records per chunk
  Dev<uint64_t> eg_base;          // [2 NB + 1] their scan
  // per-peer egress (hb_set_egress_peers / hb_egress_bin): nothing of it exists before the first table
  Dev<BinTable> bin_table;        // device copy of the node table
  uint32_t bin_np = 0;            // its ids (the table is set while bin_table is)
  Dev<uint8_t> bin_key;           // [largest batch] key bytes of the tiled path
  Dev<uint32_t> bin_hist;         // [256] bin totals, then [256][its tiles] tile histograms
  Dev<uint32_t> enc_sum;          // hb_encode: [blocks] bytes per pass-one workgroup
  Dev<uint64_t> enc_base;         // [blocks + 1]
  Dev<uint64_t> ence_sum;         // hb_encode_ents: [blocks] bytes per pass-one workgroup
  Dev<uint64_t> ence_base;        // [blocks + 1]
  // framed peer streams (hb_frame / hb_unframe / hb_gid_dir_build): nothing of it exists before the first call
  Dev<uint32_t> frm_cnt;          // hb_frame, tiled path: [256] holes per bin, [256] oversize flags
  Dev<uint32_t> gd_ctr;           // hb_gid_dir_build: [1] duplicates
  Pinned<uint64_t> unf_pin;       // hb_unframe: host image of the frame table (UNF_WORDS)
  Dev<uint64_t> unf_ft;           // its device copy
  hipEvent_t unf_done = nullptr;  // the last copy out of unf_pin has completed
  Dev<uint64_t> unf_sum;          // [tiles] bytes per tile, [tiles + 1] their scan, [257] bytes before each frame
  Dev<uint32_t> unf_st;           // [256] fstatus for the write pass, [1] unknown rows
  Dev<uint64_t> rnd;              // the r.rand stream (hb_set_rand)
  // hb_move_groups scratch, reused (u64 words)
  Dev<uint64_t> mv_in;            // the call's slot lists and vacated slots' extents (one H2D copy)
  Dev<uint64_t> mv_stage;         // [move_words][count]
  Dev<uint64_t> mv_jobs;          // [count x nmax]
  Dev<uint64_t> mv_rstage;        // the carried inflight windows
  Dev<unsigned long long> mv_ctr;  // [2] jobs, ring-stage words
  std::vector<uint64_t> mv_host;  // host image of mv_in
  std::vector<uint8_t> mv_mark;   // [G] validation marks: 1 in src, 2 in dst (all zero between calls)
  static constexpr uint32_t PROF_RING = 256;
  // per profiled step: prep start, prep end (prep stream), apply start, fast end,
  // general end, finish end (apply stream)
  static constexpr uint32_t PH_EVENTS = 6;
  hipEvent_t ph[PROF_RING][PH_EVENTS] = {};
  bool prof_full[PROF_RING] = {};  // all phases recorded (else only HB_PHASE_APPLY)
  uint32_t prof_n = 0;  // profiled steps since hb_phase_reset
  bool stepped = false;
};

namespace {

int dalloc(hb_handle* h, void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (hipMalloc(p, bytes) != hipSuccess) return HB_ENOMEM;
  h->allocs.push_back(*p);
  return HB_OK;
}

template <class T>
int dalloc_t(hb_handle* h, T** p, size_t count) {
  return dalloc(h, reinterpret_cast<void**>(p), count * sizeof(T));
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

uint32_t ceil_log2(uint32_t x) {
  uint32_t b = 0;
  while ((1u << b) < x) ++b;
  return b;
}
uint32_t ceil_log2_64(uint64_t x) {
  uint32_t b = 0;
  while (b < 63 && (1ull << b) < x) ++b;
  return b;
}

// Grow the log-index rings of groups[i] to hold at least szcap[i] entry sizes
// and trcap[i] term runs (null array or 0: unchanged); the content moves
// along (k_regrow).  Never shrinks.
int reserve_log(hb_handle* h, uint32_t count, const uint32_t* groups, const uint64_t* szcap, const uint64_t* trcap) {
  struct Need {
    uint32_t g;
    uint64_t sz, tr;
  };
  std::vector<Need> need;
  need.reserve(count);
  for (uint32_t i = 0; i < count; ++i) {
    if (groups[i] >= h->G) return HB_EINVAL;
    const uint64_t sz = (szcap && h->st.szx) ? szcap[i] : 0, tr = trcap ? trcap[i] : 0;
    const bool grow_sz = sz > (1ull << (h->h_szx.empty() ? 0 : (h->h_szx[groups[i]] & LX_TAG)));
    const bool grow_tr = tr > (1ull << (h->h_trx[groups[i]] & LX_TAG));
    if ((sz && grow_sz) || (tr && grow_tr)) need.push_back({groups[i], sz, tr});
  }
  if (need.empty()) return HB_OK;
  // one job per (group, ring): duplicates of a group merge to their largest need
  std::sort(need.begin(), need.end(), [](const Need& a, const Need& b) { return a.g < b.g; });
  std::vector<uint64_t> jobs;
  std::vector<std::pair<uint64_t, uint32_t>> old;  // extents to recycle once the copies ran
  for (size_t i = 0; i < need.size();) {
    Need m = need[i++];
    while (i < need.size() && need[i].g == m.g) {
      m.sz = std::max(m.sz, need[i].sz);
      m.tr = std::max(m.tr, need[i].tr);
      ++i;
    }
    for (uint32_t kind = 0; kind < 2; ++kind) {
      const uint64_t want = kind ? m.tr : m.sz;
      uint64_t& hx = kind ? h->h_trx[m.g] : h->h_szx[m.g];
      const uint32_t lc = (uint32_t)(hx & LX_TAG);
      if (!want || want <= (1ull << lc)) continue;
      const uint32_t l = ceil_log2_64(want), rec = kind ? 4 : 3;  // 16-byte runs, 8-byte sizes
      const uint64_t a = h->pool.get(l + rec);
      if (!a) return HB_ENOMEM;
      const uint64_t nx = lx_word(a, l);
      jobs.insert(jobs.end(), {(uint64_t)m.g | ((uint64_t)kind << 32), hx, nx, 0});
      old.emplace_back(hx & ~LX_TAG, lc + rec);
      hx = nx;
    }
  }
  const uint32_t nj = (uint32_t)(jobs.size() / 4);
  if (const int rc = h->lx_jobs.reserve(jobs.size())) return rc;
  HB_CHECK(hipMemcpyAsync(h->lx_jobs.get(), jobs.data(), jobs.size() * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_regrow, dim3((nj + 255) / 256), dim3(256), 0, h->stream, h->st, nj,
                     (const uint64_t*)h->lx_jobs.get());
  HB_CHECK(hipStreamSynchronize(h->stream));
  for (auto& o : old) h->pool.put(o.first, o.second);
  return HB_OK;
}

template <int KMAX>
uint32_t route_grid(const hb_handle* h, bool x) {
  return ((h->NBK + 7) & ~7u) << (PART_LOG + h->sis_log - (x ? RouteGeom<KMAX, true>::RG_LOG : RouteGeom<KMAX, false>::RG_LOG));
}
template <int KMAX>
void launch_route(hb_handle* h, const ApplyArgs& a, hipStream_t st) {
  if constexpr (KMAX >= 5) {
    if (a.storm) {  // the storm hand-over (never an X step's: hb_step)
      if (h->nmax <= 5)
        hipLaunchKernelGGL((k_route<KMAX, false, 5>), dim3(route_grid<KMAX>(h, false)), dim3(ROUTE_THREADS), 0, st, a);
      else
        hipLaunchKernelGGL((k_route<KMAX, false, 7>), dim3(route_grid<KMAX>(h, false)), dim3(ROUTE_THREADS), 0, st, a);
      return;
    }
  }
  if (a.slotx) hipLaunchKernelGGL((k_route<KMAX, true>), dim3(route_grid<KMAX>(h, true)), dim3(ROUTE_THREADS), 0, st, a);
  else hipLaunchKernelGGL((k_route<KMAX, false>), dim3(route_grid<KMAX>(h, false)), dim3(ROUTE_THREADS), 0, st, a);
}

// XCD-aware grid (see block_part()): whole groups of 8 buckets x 2^sis_log
// partitions, cut after the last block that maps to a real partition (a small
// handle's 4 partitions sit at blocks 0, 8, 16, 24 of a 128-block grid).
uint32_t apply_grid_for(uint32_t NBK, uint32_t sl, uint32_t NB) {
  const uint32_t full = ((NBK + 7) & ~7u) << sl;
  uint32_t need = 0;
  for (uint32_t x = 0; x < full; ++x) {
    const uint32_t r = x & 7, q = x >> 3;  // part_of() on the host
    if ((((((q >> sl) << 3) | r) << sl) | (q & ((1u << sl) - 1))) < NB) need = x + 1;
  }
  return (need + 7) & ~7u;
}
uint32_t apply_grid(const hb_handle* h) { return h->agrid; }

// hb_set_egress: the group's Term and lastIndex before the step (one launch, 32 B per group moved;
// vote mode: lastTerm too, 16 B per group more and a ring lookup for a last index below the current-term run;
// append mode: committed and the boundary pair as well, k_eg_snap_app)
void egress_snapshot(hb_handle* h, hipStream_t st) {
  SnapArgs a;
  a.term = h->st.term;
  a.last = h->st.last;
  a.term0 = h->term0.get();
  a.last0 = h->last0.get();
  a.G = h->G;
  a.tfirst = h->st.tfirst;
  a.trx = h->st.trx;
  a.trc = h->st.trc;
  a.lterm0 = h->lterm0.get();
  a.commit = h->st.commit;
  a.first = h->st.first;
  a.commit0 = h->eg_commit0.get();
  a.bl0 = h->bl0.get();
  a.blt0 = h->blt0.get();
  if (h->eg_apps) hipLaunchKernelGGL(k_eg_snap_app, dim3((h->G + 255) / 256), dim3(256), 0, st, a);
  else if (h->eg_votes) hipLaunchKernelGGL(k_eg_snap<true>, dim3((h->G + 511) / 512), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_eg_snap<false>, dim3((h->G + 511) / 512), dim3(256), 0, st, a);
  h->eg_stepped = true;
}
// A device-readable word the caller names: pinned host memory (hb_alloc_pinned) or device memory.
template <class T>
T* dev_view(T* p) {
  void* d = nullptr;
  if (p && hipHostGetDevicePointer(&d, const_cast<void*>(static_cast<const void*>(p)), 0) == hipSuccess && d)
    return static_cast<T*>(d);
  (void)hipGetLastError();  // not host memory: a device pointer as it is
  return p;
}

// The apply kernels; ev = this step's phase events (HB_STEP_PROFILE) or null.
template <uint32_t KMAX, bool X, bool WIDE>
void launch_route_fast_t(hb_handle* h, const ApplyArgs& a) {
  using GM = RouteFastGeom<KMAX, X, WIDE>;
  hipLaunchKernelGGL((k_route_fast<KMAX, X, WIDE>), dim3(((h->NBK + 7) & ~7u) << (PART_LOG + h->sis_log - GM::RG_LOG)),
                     dim3(GM::THREADS), 0, h->stream, a);
}
template <bool WIDE>
void launch_route_fast_w(hb_handle* h, const ApplyArgs& a) {
  if (a.kmax == 3) {
    if (a.slotx) launch_route_fast_t<3, true, WIDE>(h, a);
    else launch_route_fast_t<3, false, WIDE>(h, a);
  } else {
    if (a.slotx) launch_route_fast_t<2, true, WIDE>(h, a);
    else launch_route_fast_t<2, false, WIDE>(h, a);
  }
}
// One bit of hb_handle::rf_wide per form of k_route_fast.
inline uint32_t route_fast_form(uint32_t kmax, bool x) { return 1u << ((kmax == 3 ? 2u : 0u) + (x ? 1u : 0u)); }
inline bool route_fast_wide(const hb_handle* h, uint32_t kmax, bool x) { return h->rf_wide & route_fast_form(kmax, x); }
void launch_route_fast(hb_handle* h, const ApplyArgs& a) {
  if (route_fast_wide(h, a.kmax, a.slotx != nullptr)) launch_route_fast_w<true>(h, a);
  else launch_route_fast_w<false>(h, a);
}
// the route-fast workgroup (groups, log2) of a step: the wide form's is one more
template <bool WIDE>
constexpr uint32_t route_fast_rg_log_w(uint32_t kmax, bool x) {
  return kmax == 3 ? (x ? RouteFastGeom<3, true, WIDE>::RG_LOG : RouteFastGeom<3, false, WIDE>::RG_LOG)
                   : (x ? RouteFastGeom<2, true, WIDE>::RG_LOG : RouteFastGeom<2, false, WIDE>::RG_LOG);
}
inline uint32_t route_fast_rg_log(const hb_handle* h, uint32_t kmax, bool x) {
  return route_fast_wide(h, kmax, x) ? route_fast_rg_log_w<true>(kmax, x) : route_fast_rg_log_w<false>(kmax, x);
}
// fused: k_route_fast stood in for k_route + k_apply_fast (launched by hb_step)
template <int NMAX>
void launch_apply(hb_handle* h, const ApplyArgs& a, hipEvent_t* ev, bool full, bool fused = false) {
  const uint32_t grid = apply_grid(h);
  if (ev) (void)hipEventRecord(ev[2], h->stream);
  if (fused) {
    if constexpr (NMAX <= 3) launch_route_fast(h, a);
  } else if constexpr (NMAX >= 5) {
    if (a.slotx) hipLaunchKernelGGL((k_apply_lead<NMAX, true>), dim3(grid), dim3(PART), 0, h->stream, a);
    else hipLaunchKernelGGL((k_apply_lead<NMAX, false>), dim3(grid), dim3(PART), 0, h->stream, a);
  }
  else if (a.kmax == 3) {
    if (a.slotx) hipLaunchKernelGGL((k_apply_fast<NMAX, true, 3>), dim3(grid), dim3(PART), 0, h->stream, a);
    else hipLaunchKernelGGL((k_apply_fast<NMAX, false, 3>), dim3(grid), dim3(PART), 0, h->stream, a);
  } else {
    if (a.slotx) hipLaunchKernelGGL((k_apply_fast<NMAX, true, 2>), dim3(grid), dim3(PART), 0, h->stream, a);
    else hipLaunchKernelGGL((k_apply_fast<NMAX, false, 2>), dim3(grid), dim3(PART), 0, h->stream, a);
  }
  if (ev) (void)hipEventRecord(ev[3], h->stream);
  // the list kernels loop over their XCD slot's list, so a small handle (a
  // MultiNode node of a few thousand groups: 4 partitions under a 128-entry
  // virtual grid) launches one workgroup per list entry it can have, at least 8
  const uint32_t lists = std::max(8u, (h->NB + 7) & ~7u);
  if constexpr (NMAX >= 5) {  // the general kernel spills at n >= 5: elections go first
    if (!sz_on(h->max_msg_size))
      hipLaunchKernelGGL(k_elect<NMAX>, dim3(std::min(lists, ELECT_GRID ? std::min(grid, ELECT_GRID) : grid)),
                         dim3(PART), 0, h->stream, a);
  }
  if constexpr (NMAX <= 3) {  // chained follower pass; the last workgroup runs the finish
    const uint32_t gg = std::min(lists, GEN_GRID3 ? std::min(grid, GEN_GRID3) : grid);
    hipLaunchKernelGGL(k_apply<NMAX>, dim3(gg), dim3(PART), 0, h->stream, a);
  } else {
    hipLaunchKernelGGL(k_apply<NMAX>, dim3(std::min(lists, GEN_GRID ? std::min(grid, GEN_GRID) : grid)), dim3(PART), 0,
                       h->stream, a);
    // k_follow's last workgroup also runs the step's finish (k_finish)
    hipLaunchKernelGGL(k_follow<NMAX>, dim3(FOLLOW_GRID), dim3(PART), 0, h->stream, a);
  }
  if (ev && full) (void)hipEventRecord(ev[4], h->stream);
}

}  // namespace

extern "C" {

int hb_abi_version(void) { return HB_ABI_VERSION; }

const char* hb_strerror(int code) {
  switch (code) {
    case HB_OK: return "ok";
    case HB_EINVAL: return "invalid argument";
    case HB_ENOMEM: return "out of memory";
    case HB_EDEVICE: return "device error";
    case HB_EINVARIANT: return "device invariant violated";
    default: return "unknown error";
  }
}

int hb_create(int device, uint32_t capacity, uint32_t max_replicas, uint32_t max_inflight,
              uint64_t max_msg_size, uint64_t max_batch, hb_handle** out) {
  if (!out || capacity == 0 || max_replicas < 1 || max_replicas > HB_MAX_REPLICAS || max_inflight < 1 ||
      max_inflight > HB_MAX_INFLIGHT || max_batch >= (1ull << 31) || capacity > (1u << 24))
    return HB_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return HB_EDEVICE;
  DeviceGuard guard(device);
  hb_handle* h = new hb_handle();
  h->device = device;
  h->G = capacity;
  h->nmax = max_replicas <= 3 ? 3 : (max_replicas <= 5 ? 5 : 7);
  h->W = max_inflight;
  h->max_msg_size = max_msg_size;
  h->max_batch = max_batch;
  h->NB = (capacity + PART - 1) / PART;
  if (const char* e = getenv("HB_SMALL_STEP")) h->no_small = e[0] == '0';
  if (const char* e = getenv("HB_ROUTE_FUSE")) h->fuse = (uint32_t)atoi(e);
  if (const char* e = getenv("HB_STORM")) h->storm = atoi(e) == 0 ? 0u : 2u;
  if (const char* e = getenv("HB_FAST_STEADY")) h->steady = atoi(e) != 0;
  if (const char* e = getenv("HB_FAST_STEADY_COUNT")) h->steady_count = atoi(e) != 0;
  const size_t G = capacity, R = h->nmax;
  DevState& s = h->st;
  s.G = capacity;
  s.W = max_inflight;
  s.nmax = h->nmax;
  s.lazy_next = h->nmax <= 3 ? 1u : 0u;  // M_NX (hipbatch_kernels.h); HB_LAZY_NEXT=0: never set (same output)
  if (const char* e = getenv("HB_LAZY_NEXT")) s.lazy_next = (h->nmax <= 3 && atoi(e) != 0) ? 1u : 0u;
  s.max_msg_size = max_msg_size;
  int rc = HB_OK;
#define ALLOC(ptr, count) \
  if (rc == HB_OK) rc = dalloc_t(h, &(ptr), (count))
  ALLOC(s.term, G);
  ALLOC(s.commit, G);
  ALLOC(s.first, G);
  ALLOC(s.last, G);
  ALLOC(s.tfirst, G);
  ALLOC(s.tlast, G);
  ALLOC(s.snap, G);
  ALLOC(s.meta, G);
  ALLOC(s.match, R * G);
  ALLOC(s.next, R * G);
  ALLOC(s.pending, R * G);
  ALLOC(s.pm, R * G);
  ALLOC(s.ring, R * (size_t)max_inflight * G);
  ALLOC(s.elapsed, G);
  ALLOC(s.rpos, G);
  ALLOC(s.tcfg, G);
  ALLOC(s.trx, G);  // the log index (DevState): older term runs (follower side) ...
  ALLOC(s.trc, G);
  if (sz_on(max_msg_size)) {  // ... and, for limitSize, the entries' cumulative sizes
    ALLOC(s.szx, G);
    ALLOC(s.szlo, G);
  }
  // partition scratch
  const size_t mb = max_batch ? max_batch : 1;
  // buckets: SIS_MAX partitions each, or fewer — down to one k_route
  // workgroup per bucket — while that needs no extra radix pass
  auto nbk_for = [&](uint32_t sl) { return (capacity + (PART << sl) - 1) / (PART << sl); };
  auto passes_for = [&](uint32_t sl) {
    return (std::max<uint32_t>(ceil_log2(nbk_for(sl)), 1) + RDX_BITS - 1) / RDX_BITS;
  };
  const uint32_t sl_max = h->nmax <= 3 ? SIS_LOG_MAX3 : SIS_LOG_MAX;
  h->sis_log = sl_max;
  const uint32_t sl_min = route_rg_log(route_kmax(h->nmax)) - PART_LOG;
  while (h->sis_log > sl_min && passes_for(h->sis_log - 1) == passes_for(sl_max)) --h->sis_log;
  if (const char* e = getenv("HB_SIS_LOG")) {  // (A/B knob: a fixed bucket size, within the allowed range)
    const int v = atoi(e);
    if (v >= (int)sl_min && v <= (int)sl_max) h->sis_log = (uint32_t)v;
  }
  // k_route_fast's geometry: wide where a narrow <2, false> workgroup would
  // have a sister (n = 3, buckets of 4096 groups or more), in the forms that
  // measured no slower wide (RF_WIDE_FORMS); HB_RF_WIDE=1: every form, 0: none
  // (A/B knob, within that range).
  if (h->nmax == 3 && PART_LOG + h->sis_log >= RouteFastGeom<2, false, true>::RG_LOG) {
    h->rf_wide = RF_WIDE_FORMS;
    if (const char* e = getenv("HB_RF_WIDE")) h->rf_wide = atoi(e) ? 0xFu : 0u;
  }
  h->NBK = nbk_for(h->sis_log);
  h->passes = passes_for(h->sis_log);
  h->bk_bits = std::max<uint32_t>(ceil_log2(h->NBK), 1);
  h->agrid = apply_grid_for(h->NBK, h->sis_log, h->NB);
  const size_t tiles_max = (mb + RDX_TILE - 1) / RDX_TILE;
  ALLOC(h->hist, (size_t)RDX_BINS * tiles_max);
  ALLOC(h->n_valid, 4);
  ALLOC(h->totals, RDX_BINS);
  if (h->passes == 1) {
    const size_t nhw = (tiles_max + HIST_TPB - 1) / HIST_TPB;
    h->sup_max = (uint32_t)((nhw + SB_HW - 1) / SB_HW);
    ALLOC(h->hagg, nhw * RDX_BINS);
    ALLOC(h->hsup, (size_t)SUP_BUFS * h->sup_max * RDX_BINS);
    if (rc == HB_OK && hipMemset(h->hsup, 0, (size_t)SUP_BUFS * h->sup_max * RDX_BINS * 4) != hipSuccess)
      rc = HB_EDEVICE;
  }
  for (uint32_t k = 0; k + 1 < h->passes && k < 2; ++k) {  // ping-pong buffers of intermediate passes
    RadixDst& d = h->tmp[k];
    ALLOC(d.group, mb);
    ALLOC(d.rec, mb);
    ALLOC(d.recx, mb);
  }
  for (PrepSet& ps : h->set) {
    ALLOC(ps.rec, mb);
    ALLOC(ps.key, mb + SEG);
    if (h->passes > 1) ALLOC(ps.bucket, mb);
    ALLOC(ps.bk_off, h->NBK + 1);
    ALLOC(ps.bk_fill, (size_t)h->NBK * CTR_STRIDE);
    ALLOC(ps.ctr, CTR_WORDS);
    ALLOC(ps.cnt, G);
    ALLOC(ps.slot, route_kmax(R) * G);
    ALLOC(ps.side, 2 * mb);
    ALLOC(ps.recx, mb);
    ALLOC(ps.slotx, route_kmax(R) * G);
    ALLOC(ps.ev_counts, 2ull * h->NB);
    ALLOC(ps.ev_off, 2ull * h->NB);
  }
  ALLOC(h->s_group, mb);
  ALLOC(h->s_info, mb);
  ALLOC(h->s_term, mb);
  ALLOC(h->s_index, mb);
  ALLOC(h->s_hint, mb);
  ALLOC(h->s_props, G);
  ALLOC(h->s_eoff, mb);
  ALLOC(h->s_commit, mb);
  if (sz_on(max_msg_size)) ALLOC(h->s_peoff, G);
  // events: (batch + one proposal slot per group) x EV_MAX (exact bound)
  h->ev_per_msg = EVC_WORDS_MAX * (h->nmax + 4);  // events per message <= nmax + 4, <= 2 words each
  // P chunks (one per partition, dense proposals) then the bucket regions of M chunks
  h->ev_region = ((uint64_t)h->NB * PART + mb + ((uint64_t)h->NBK * PART << h->sis_log)) * h->ev_per_msg;
  ALLOC(h->ev, h->ev_region);
  ALLOC(h->stats_shard, shard_at(ST_N + 1, 0));
  ALLOC(h->pflag, (size_t)h->NB * FLAG_WORDS);
  ALLOC(h->ap_list, 8ull * h->NB);
  ALLOC(h->fl_list, h->NB);
  if (h->nmax >= 5) {
    ALLOC(h->eflag, (size_t)h->NB * FLAG_WORDS);
    ALLOC(h->lskip, (size_t)h->NB);
    ALLOC(h->el_list, 8ull * h->NB);
  }
  ALLOC(h->resume, G);
  ALLOC(h->commit0, G);
  ALLOC(h->stats, HB_STAT_COUNT);
#undef ALLOC
  if (rc == HB_OK) rc = h->stats_pin.reserve(HB_STAT_COUNT);
  if (rc != HB_OK) {
    hb_destroy(h);
    return rc;
  }
  // the prep stream runs at the lowest priority: its kernels fill what the
  // apply stage leaves idle instead of competing with it
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  bool ok = hipStreamCreateWithPriority(&h->prep, hipStreamNonBlocking, prio_least) == hipSuccess &&
            hipEventCreateWithFlags(&h->in_ready, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&h->hstage_done, hipEventDisableTiming) == hipSuccess;
  for (PrepSet& ps : h->set)
    ok = ok && hipEventCreateWithFlags(&ps.prepped, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&ps.applied, hipEventDisableTiming) == hipSuccess;
  for (auto& row : h->ph)
    for (auto& e : row) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok) {
    hb_destroy(h);
    return HB_EDEVICE;
  }
  // empty slots (n = 0), zeroed progress
  if (hipMemset(s.meta, 0, G * 8) != hipSuccess || hipMemset(s.pm, 0, R * G * 4) != hipSuccess ||
      hipMemset(s.elapsed, 0, G * 4) != hipSuccess || hipMemset(s.rpos, 0, G * 4) != hipSuccess ||
      hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(s.tcfg), 10u | (1u << 16), G) != hipSuccess ||
      hipMemset(h->stats, 0, HB_STAT_COUNT * 8) != hipSuccess || hipMemset(h->stats_shard, 0, shard_at(ST_N + 1, 0) * 8ull) != hipSuccess ||
      hipMemset(h->set[0].ctr, 0, CTR_WORDS * 4) != hipSuccess || hipMemset(h->set[1].ctr, 0, CTR_WORDS * 4) != hipSuccess ||
      hipMemset(h->set[0].ev_counts, 0, h->NB * 8ull) != hipSuccess ||
      hipMemset(h->set[0].ev_off, 0, h->NB * 16ull) != hipSuccess ||
      hipMemset(s.trc, 0, G * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    hb_destroy(h);
    return HB_EDEVICE;
  }
  // the log index: every group starts with a 128-byte extent per ring, carved
  // from one slab each (hb_reserve_log moves a group to a larger one)
  auto init_rings = [&](std::vector<uint64_t>& hx, uint64_t* dx, uint32_t log2cap) {
    void* slab = nullptr;
    if (hipMalloc(&slab, G * 128) != hipSuccess) return false;
    h->pool.slabs.push_back(slab);
    hx.resize(G);
    const uint64_t base = reinterpret_cast<uint64_t>(slab);
    for (size_t g = 0; g < G; ++g) hx[g] = lx_word(base + 128 * g, log2cap);
    return hipMemcpy(dx, hx.data(), G * 8, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!init_rings(h->h_trx, s.trx, TR_LOG_MIN) || (s.szx && !init_rings(h->h_szx, s.szx, SZ_LOG_MIN))) {
    hb_destroy(h);
    return HB_ENOMEM;
  }
  *out = h;
  return HB_OK;
}

int hb_destroy(hb_handle* h) {
  if (!h) return HB_EINVAL;
  DeviceGuard guard(h->device);
  (void)hipDeviceSynchronize();
  for (auto& row : h->ph)
    for (auto& e : row)
      if (e) (void)hipEventDestroy(e);
  for (PrepSet& ps : h->set) {
    if (ps.prepped) (void)hipEventDestroy(ps.prepped);
    if (ps.applied) (void)hipEventDestroy(ps.applied);
  }
  if (h->hstage_done) (void)hipEventDestroy(h->hstage_done);
  if (h->unf_done) (void)hipEventDestroy(h->unf_done);
  if (h->in_ready) (void)hipEventDestroy(h->in_ready);
  if (h->prep) (void)hipStreamDestroy(h->prep);
  h->pool.release();
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;  // every DevBuf member frees itself, on h->device still
  return HB_OK;
}

int hb_set_stream(hb_handle* h, void* stream) {
  if (!h) return HB_EINVAL;
  h->stream = reinterpret_cast<hipStream_t>(stream);
  return HB_OK;
}

int hb_sync(hb_handle* h) {
  if (!h) return HB_EINVAL;
  DeviceGuard guard(h->device);
  HB_CHECK(hipStreamSynchronize(h->prep));
  HB_CHECK(hipStreamSynchronize(h->stream));
  return HB_OK;
}

static bool valid_ref(uint32_t r, uint32_t n) {
  return r < n || r == HB_REF_OTHER || r == HB_REF_SELF || r == HB_REF_NONE;
}

int hb_load_groups(hb_handle* h, uint32_t first, uint32_t count, const hb_group* groups) {
  if (!h || !groups || (uint64_t)first + count > h->G) return HB_EINVAL;
  if (count == 0) return HB_OK;
  for (uint32_t i = 0; i < count; ++i) {
    const hb_group& r = groups[i];
    if (r.n < 1 || r.n > h->nmax || r.state > 2 || r.fault > 15) return HB_EINVAL;
    if (!(r.self_slot < r.n || r.self_slot == HB_SLOT_NONE)) return HB_EINVAL;
    if (!valid_ref(r.lead, r.n) || !valid_ref(r.vote, r.n)) return HB_EINVAL;
    if (r.first_index == 0 || r.last_index + 1 < r.first_index) return HB_EINVAL;
    if (r.term_first != HB_NO_INDEX &&
        (r.term_first > r.term_last || r.term_first + 1 < r.first_index || r.term_last > r.last_index))
      return HB_EINVAL;
    if ((r.votes_resp | r.votes_grant) > 0xFF || (r.votes_grant & ~r.votes_resp)) return HB_EINVAL;
    for (uint32_t s = 0; s < r.n; ++s) {
      const hb_progress& p = r.pr[s];
      if (p.state > 2 || p.paused > 1 || p.ins_start >= h->W || p.ins_count > h->W) return HB_EINVAL;
    }
  }
  DeviceGuard guard(h->device);
  Dev<hb_group> d;
  if (const int rc = d.reserve(count)) return rc;
  hipError_t e = hipMemcpyAsync(d.get(), groups, sizeof(hb_group) * count, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_load, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->st, first, count, d.get());
    if (h->peer)
      hipLaunchKernelGGL(k_peer_n, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->peer.get(), h->st.meta, first,
                         count);
    e = hipStreamSynchronize(h->stream);
  }
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_get_groups(hb_handle* h, uint32_t first, uint32_t count, hb_group* out) {
  if (!h || !out || (uint64_t)first + count > h->G) return HB_EINVAL;
  if (count == 0) return HB_OK;
  DeviceGuard guard(h->device);
  Dev<hb_group> d;
  if (const int rc = d.reserve(count)) return rc;
  hipLaunchKernelGGL(k_gather, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->st, first, count, d.get());
  hipError_t e = hipMemcpyAsync(out, d.get(), sizeof(hb_group) * count, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_remove_groups(hb_handle* h, uint32_t first, uint32_t count) {
  if (!h || (uint64_t)first + count > h->G) return HB_EINVAL;
  if (count == 0) return HB_OK;
  DeviceGuard guard(h->device);
  hipLaunchKernelGGL(k_remove, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->st, first, count);
  HB_CHECK(hipStreamSynchronize(h->stream));
  return HB_OK;
}

int hb_move_groups(hb_handle* h, uint32_t count, const uint32_t* src, const uint32_t* dst) {
  if (!h || (count && (!src || !dst))) return HB_EINVAL;
  if (count == 0) return HB_OK;
  if (count > h->G) return HB_EINVAL;  // more pairs than slots: a duplicate
  // validation: every slot in range, src distinct, dst distinct (marks: 1 in src, 2 in dst)
  if (h->mv_mark.size() != h->G) h->mv_mark.assign(h->G, 0);
  std::vector<uint8_t>& mark = h->mv_mark;
  uint32_t seen = 0;
  bool ok = true;
  for (; seen < count; ++seen) {
    const uint32_t s = src[seen], d = dst[seen];
    if (s >= h->G || d >= h->G || (mark[s] & 1) || (mark[d] & 2)) {
      ok = false;
      break;
    }
    mark[s] |= 1;
    mark[d] |= 2;
  }
  // vacated slots (in src, not in dst) take over the log extents of the
  // overwritten ones (in dst, not in src): equally many, every slot keeps one of each kind
  std::vector<uint32_t> vac, over;
  if (ok)
    for (uint32_t i = 0; i < count; ++i) {
      if (!(mark[src[i]] & 2)) vac.push_back(src[i]);
      if (!(mark[dst[i]] & 1)) over.push_back(dst[i]);
    }
  for (uint32_t i = 0; i < seen; ++i) mark[src[i]] = mark[dst[i]] = 0;
  if (!ok || vac.size() != over.size()) return HB_EINVAL;
  const uint32_t nvac = (uint32_t)vac.size();
  const bool sized = h->st.szx != nullptr;

  DeviceGuard guard(h->device);
  const uint32_t NW = move_words(h->nmax, sized, bool(h->peer));
  const uint64_t in_words = 2ull * nvac + (2ull * count + nvac + 1) / 2;
  // the scratch at least doubles (the old blocks are idle: every call that uses them synchronizes)
  int rc = h->mv_in.reserve(in_words, 2 * h->mv_in.cap());
  if (rc == HB_OK) rc = h->mv_stage.reserve((uint64_t)NW * count, 2 * h->mv_stage.cap());
  if (rc == HB_OK) rc = h->mv_jobs.reserve((uint64_t)h->nmax * count, 2 * h->mv_jobs.cap());
  if (rc == HB_OK) rc = h->mv_ctr.reserve(2);
  if (rc != HB_OK) return rc;
  // one upload: the vacated slots' new extent words (u64), then src, dst, vac (u32)
  h->mv_host.assign(in_words, 0);
  uint32_t* hsrc = reinterpret_cast<uint32_t*>(h->mv_host.data() + 2ull * nvac);
  for (uint32_t v = 0; v < nvac; ++v) {
    h->mv_host[v] = sized ? h->h_szx[over[v]] : 0;
    h->mv_host[nvac + v] = h->h_trx[over[v]];
  }
  std::memcpy(hsrc, src, 4ull * count);
  std::memcpy(hsrc + count, dst, 4ull * count);
  if (nvac) std::memcpy(hsrc + 2ull * count, vac.data(), 4ull * nvac);
  MoveArgs a{};
  a.count = count;
  a.nvac = nvac;
  a.vac_szx = h->mv_in.get();
  a.vac_trx = h->mv_in.get() + nvac;
  a.src = reinterpret_cast<const uint32_t*>(h->mv_in.get() + 2ull * nvac);
  a.dst = a.src + count;
  a.vac = a.dst + count;
  a.stage = h->mv_stage.get();
  a.peer = h->peer.get();
  a.jobs = h->mv_jobs.get();
  a.ctr = h->mv_ctr.get();
  a.rstage = h->mv_rstage.get();
  hipStream_t st = h->stream;
  HB_CHECK(hipMemcpyAsync(h->mv_in.get(), h->mv_host.data(), in_words * 8, hipMemcpyHostToDevice, st));
  HB_CHECK(hipMemsetAsync(h->mv_ctr.get(), 0, 16, st));
  hipLaunchKernelGGL(k_move_gather, dim3((count + 255) / 256), dim3(256), 0, st, h->st, a);
  HB_CHECK(hipGetLastError());
  // how many windows travel (none after a reset, the usual case: no ring kernels then)
  unsigned long long ctr[2] = {0, 0};
  HB_CHECK(hipMemcpyAsync(ctr, h->mv_ctr.get(), 16, hipMemcpyDeviceToHost, st));
  HB_CHECK(hipStreamSynchronize(st));
  const uint32_t njobs = (uint32_t)ctr[0];
  if (njobs) {
    if (ctr[0] > (uint64_t)h->nmax * count || ctr[1] > ctr[0] * h->W) return HB_EINVARIANT;
    rc = h->mv_rstage.reserve(ctr[1], 2 * h->mv_rstage.cap());
    if (rc != HB_OK) return rc;
    a.rstage = h->mv_rstage.get();
    hipLaunchKernelGGL(k_move_ring<false>, dim3((njobs + 3) / 4), dim3(256), 0, st, h->st, a, njobs);
    HB_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_move_scatter, dim3((count + nvac + 255) / 256), dim3(256), 0, st, h->st, a);
  HB_CHECK(hipGetLastError());
  if (njobs) {
    hipLaunchKernelGGL(k_move_ring<true>, dim3((njobs + 3) / 4), dim3(256), 0, st, h->st, a, njobs);
    HB_CHECK(hipGetLastError());
  }
  HB_CHECK(hipStreamSynchronize(st));
  // the host mirrors of the extent words follow
  for (int kind = 0; kind < (sized ? 2 : 1); ++kind) {
    std::vector<uint64_t>& hx = kind ? h->h_szx : h->h_trx;
    std::vector<uint64_t> moved(count);
    for (uint32_t i = 0; i < count; ++i) moved[i] = hx[src[i]];
    for (uint32_t v = 0; v < nvac; ++v) hx[vac[v]] = h->mv_host[(kind ? 0 : nvac) + v];
    for (uint32_t i = 0; i < count; ++i) hx[dst[i]] = moved[i];
  }
  return HB_OK;
}

int hb_set_log_bounds(hb_handle* h, uint32_t count, const uint32_t* groups, const uint64_t* first_index,
                      const uint64_t* snap_index) {
  if (!h || (count && (!groups || !first_index || !snap_index))) return HB_EINVAL;
  if (count == 0) return HB_OK;
  for (uint32_t i = 0; i < count; ++i)
    if (groups[i] >= h->G || first_index[i] == 0) return HB_EINVAL;
  DeviceGuard guard(h->device);
  Dev<char> d;
  if (const int rc = d.reserve((uint64_t)count * (4 + 8 + 8))) return rc;
  uint64_t* dfirst = reinterpret_cast<uint64_t*>(d.get());
  uint64_t* dsnap = dfirst + count;
  uint32_t* dgroup = reinterpret_cast<uint32_t*>(dsnap + count);
  hipError_t e = hipMemcpyAsync(dfirst, first_index, count * 8ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dsnap, snap_index, count * 8ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dgroup, groups, count * 4ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_set_bounds, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->st, count,
                       (const uint32_t*)dgroup, (const uint64_t*)dfirst, (const uint64_t*)dsnap);
    e = hipStreamSynchronize(h->stream);
  }
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_load_term_runs(hb_handle* h, uint32_t count, const uint32_t* groups, const uint32_t* n_runs,
                      const uint64_t* runs) {
  if (!h || (count && (!groups || !n_runs))) return HB_EINVAL;
  if (count == 0) return HB_OK;
  std::vector<uint64_t> off(count), cap(count);
  uint64_t tot = 0;
  for (uint32_t i = 0; i < count; ++i) {
    if (groups[i] >= h->G) return HB_EINVAL;
    off[i] = tot;
    tot += n_runs[i];
    cap[i] = (uint64_t)n_runs[i] + 1;  // room for the reset that pushes the current-term run
  }
  if (tot && !runs) return HB_EINVAL;
  DeviceGuard guard(h->device);
  if (const int rc = reserve_log(h, count, groups, nullptr, cap.data())) return rc;
  Dev<char> d;
  if (const int rc = d.reserve(count * (8ull + 4 + 4) + tot * 16 + 16)) return rc;
  uint64_t* doff = reinterpret_cast<uint64_t*>(d.get());
  uint64_t* druns = doff + count;
  uint32_t* dgrp = reinterpret_cast<uint32_t*>(druns + 2 * tot);
  uint32_t* dn = dgrp + count;
  hipError_t e = hipMemcpyAsync(doff, off.data(), count * 8ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess && tot) e = hipMemcpyAsync(druns, runs, tot * 16ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dgrp, groups, count * 4ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dn, n_runs, count * 4ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_load_runs, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->st, count,
                       (const uint32_t*)dgrp, (const uint32_t*)dn, (const uint64_t*)doff, (const uint64_t*)druns);
    e = hipStreamSynchronize(h->stream);
  }
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_load_entry_sizes(hb_handle* h, uint32_t count, const uint32_t* groups, const uint32_t* n_sizes,
                        const uint32_t* sizes) {
  if (!h || (count && (!groups || !n_sizes))) return HB_EINVAL;
  if (!sz_on(h->max_msg_size)) return HB_EINVAL;
  if (count == 0) return HB_OK;
  std::vector<uint64_t> off(count), cap(count);
  uint64_t tot = 0;
  for (uint32_t i = 0; i < count; ++i) {
    if (groups[i] >= h->G) return HB_EINVAL;
    off[i] = tot;
    tot += n_sizes[i];
    cap[i] = (uint64_t)n_sizes[i] + 1;  // the base entry plus n sizes
  }
  if (tot && !sizes) return HB_EINVAL;
  DeviceGuard guard(h->device);
  if (const int rc = reserve_log(h, count, groups, cap.data(), nullptr)) return rc;
  Dev<char> d;
  if (const int rc = d.reserve(count * (4ull + 4 + 8) + tot * 4 + 16)) return rc;
  uint64_t* doff = reinterpret_cast<uint64_t*>(d.get());
  uint32_t* dgrp = reinterpret_cast<uint32_t*>(doff + count);
  uint32_t* dn = dgrp + count;
  uint32_t* dsz = dn + count;
  hipError_t e = hipMemcpyAsync(doff, off.data(), count * 8ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dgrp, groups, count * 4ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dn, n_sizes, count * 4ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess && tot) e = hipMemcpyAsync(dsz, sizes, tot * 4ull, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_load_sizes, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->st, count,
                       (const uint32_t*)dgrp, (const uint32_t*)dn, (const uint64_t*)doff, (const uint32_t*)dsz);
    e = hipStreamSynchronize(h->stream);
  }
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_reserve_log(hb_handle* h, uint32_t count, const uint32_t* groups, const uint64_t* size_cap,
                   const uint64_t* run_cap) {
  if (!h || (count && !groups)) return HB_EINVAL;
  if (count == 0 || (!size_cap && !run_cap)) return HB_OK;
  DeviceGuard guard(h->device);
  return reserve_log(h, count, groups, size_cap, run_cap);
}

int hb_log_capacity(hb_handle* h, uint32_t group, uint64_t* size_cap, uint64_t* run_cap) {
  if (!h || group >= h->G) return HB_EINVAL;
  if (size_cap) *size_cap = h->h_szx.empty() ? 0 : 1ull << (h->h_szx[group] & LX_TAG);
  if (run_cap) *run_cap = 1ull << (h->h_trx[group] & LX_TAG);
  return HB_OK;
}

int hb_set_inflights(hb_handle* h, uint32_t group, uint32_t slot, uint32_t start, uint32_t count,
                     const uint64_t* vals) {
  if (!h || group >= h->G || slot >= h->nmax || start >= h->W || count > h->W || (count && !vals))
    return HB_EINVAL;
  DeviceGuard guard(h->device);
  Dev<uint64_t> d;
  if (const int rc = d.reserve(count ? count : 1)) return rc;
  hipError_t e = hipSuccess;
  if (count) e = hipMemcpyAsync(d.get(), vals, 8ull * count, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_set_ins, dim3(1), dim3(256), 0, h->stream, h->st, group, slot, start, count, d.get());
    e = hipStreamSynchronize(h->stream);
  }
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_load_timers(hb_handle* h, uint32_t first, uint32_t count, const hb_timer* timers) {
  if (!h || !timers || (uint64_t)first + count > h->G) return HB_EINVAL;
  if (count == 0) return HB_OK;
  std::vector<uint32_t> el(count), pos(count), cfg(count);
  for (uint32_t i = 0; i < count; ++i) {
    if (timers[i].election_tick == 0) return HB_EINVAL;  // r.rand.Int() % 0
    el[i] = timers[i].elapsed;
    pos[i] = timers[i].rand_pos;
    cfg[i] = timers[i].election_tick | ((uint32_t)timers[i].heartbeat_tick << 16);
  }
  DeviceGuard guard(h->device);
  HB_CHECK(hipMemcpyAsync(h->st.elapsed + first, el.data(), count * 4ull, hipMemcpyHostToDevice, h->stream));
  HB_CHECK(hipMemcpyAsync(h->st.rpos + first, pos.data(), count * 4ull, hipMemcpyHostToDevice, h->stream));
  HB_CHECK(hipMemcpyAsync(h->st.tcfg + first, cfg.data(), count * 4ull, hipMemcpyHostToDevice, h->stream));
  HB_CHECK(hipStreamSynchronize(h->stream));
  return HB_OK;
}

int hb_get_timers(hb_handle* h, uint32_t first, uint32_t count, hb_timer* out) {
  if (!h || !out || (uint64_t)first + count > h->G) return HB_EINVAL;
  if (count == 0) return HB_OK;
  std::vector<uint32_t> el(count), pos(count), cfg(count);
  DeviceGuard guard(h->device);
  HB_CHECK(hipMemcpyAsync(el.data(), h->st.elapsed + first, count * 4ull, hipMemcpyDeviceToHost, h->stream));
  HB_CHECK(hipMemcpyAsync(pos.data(), h->st.rpos + first, count * 4ull, hipMemcpyDeviceToHost, h->stream));
  HB_CHECK(hipMemcpyAsync(cfg.data(), h->st.tcfg + first, count * 4ull, hipMemcpyDeviceToHost, h->stream));
  HB_CHECK(hipStreamSynchronize(h->stream));
  for (uint32_t i = 0; i < count; ++i) {
    out[i] = hb_timer{};
    out[i].elapsed = el[i];
    out[i].rand_pos = pos[i];
    out[i].election_tick = (uint16_t)(cfg[i] & 0xFFFFu);
    out[i].heartbeat_tick = (uint16_t)(cfg[i] >> 16);
  }
  return HB_OK;
}

int hb_set_rand(hb_handle* h, uint64_t first, uint64_t count, const uint64_t* draws) {
  if (!h || (count && !draws) || first > h->st.nrnd) return HB_EINVAL;  // no holes
  const uint64_t need = first + count;
  DeviceGuard guard(h->device);
  if (need > h->rnd.cap()) {  // the table at least doubles; the earlier draws move along
    Dev<uint64_t> fresh;
    if (const int rc = fresh.reserve(need, 2 * h->rnd.cap())) return rc;
    hipError_t e = hipSuccess;
    if (h->rnd && first) e = hipMemcpyAsync(fresh.get(), h->rnd.get(), first * 8, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // no kernel reads the old table any more
    if (e != hipSuccess) return HB_EDEVICE;
    h->rnd = std::move(fresh);
  }
  if (count) {
    HB_CHECK(hipMemcpyAsync(h->rnd.get() + first, draws, count * 8, hipMemcpyHostToDevice, h->stream));
    HB_CHECK(hipStreamSynchronize(h->stream));
  }
  h->st.rnd = h->rnd.get();
  if (need > h->st.nrnd) h->st.nrnd = need;
  return HB_OK;
}

int hb_load_peers(hb_handle* h, uint32_t first, uint32_t count, const uint64_t* ids) {
  if (!h || (count && !ids) || (uint64_t)first + count > h->G) return HB_EINVAL;
  if (count == 0) return HB_OK;
  DeviceGuard guard(h->device);
  const size_t G = h->G;
  if (!h->peer) {
    if (const int rc = h->peer.reserve(G * HB_PEER_ROW)) return rc;
    HB_CHECK(hipMemsetAsync(h->peer.get(), 0, G * HB_PEER_ROW * 8, h->stream));
  }
  // one 64-byte row per group (k_decode reads it with one gather): slots
  // 0..nmax-1, zeros, then n (k_peer_n)
  std::vector<uint64_t> rows((size_t)count * HB_PEER_ROW, 0);
  for (uint32_t i = 0; i < count; ++i)
    for (uint32_t s = 0; s < h->nmax; ++s) rows[(size_t)i * HB_PEER_ROW + s] = ids[(size_t)i * HB_MAX_REPLICAS + s];
  HB_CHECK(hipMemcpyAsync(h->peer.get() + (size_t)first * HB_PEER_ROW, rows.data(), rows.size() * 8,
                          hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_peer_n, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->peer.get(), h->st.meta, first,
                     count);
  HB_CHECK(hipGetLastError());
  HB_CHECK(hipStreamSynchronize(h->stream));  // rows is freed on return
  return HB_OK;
}

// what hb_decode and hb_decode_follow hand their kernels alike
static DecodeArgs decode_args(const hb_handle* h, const uint8_t* bytes, const uint64_t* off, const uint32_t* len,
                              const uint32_t* group, uint64_t n, const hb_batch* out, uint8_t* status) {
  DecodeArgs da;
  da.bytes = bytes;
  da.off = off;
  da.len = len;
  da.group = group;
  da.n = n;
  da.meta = h->st.meta;
  da.peer = reinterpret_cast<const uint4*>(h->peer.get());
  da.G = h->G;
  da.nmax = h->nmax;
  da.o_group = const_cast<uint32_t*>(out->group);
  da.o_info = const_cast<uint32_t*>(out->info);
  da.o_term = const_cast<uint64_t*>(out->term);
  da.o_index = const_cast<uint64_t*>(out->index);
  da.o_hint = const_cast<uint64_t*>(out->hint);
  da.status = status;
  return da;
}
// The pass-2 queue of both: room for n record indices, and its two counters
// (zeroed on `ds` when they are allocated).  sync_first: wait for `ds` before
// a queue that is too small is replaced.
static int decode_queue(hb_handle* h, uint64_t n, hipStream_t ds, bool sync_first) {
  if (n > h->dec_q.cap()) {
    if (sync_first) HB_CHECK(hipStreamSynchronize(ds));
    if (const int rc = h->dec_q.reserve(n)) return rc;
  }
  if (!h->dec_qn) {
    if (const int rc = h->dec_qn.reserve(2)) return rc;
    HB_CHECK(hipMemsetAsync(h->dec_qn.get(), 0, 2 * sizeof(uint32_t), ds));
  }
  return HB_OK;
}

int hb_decode(hb_handle* h, const uint8_t* bytes, const uint64_t* off, const uint32_t* len, const uint32_t* group,
              uint64_t n, const hb_batch* out, uint8_t* status) {
  if (!h || !out) return HB_EINVAL;
  if (n == 0) return HB_OK;
  if (n >= (1ull << 32)) return HB_EINVAL;  // record indices are 32-bit in the pass-2 queue
  if (!bytes || !off || !len || !group || !status || !out->group || !out->info || !out->term || !out->index ||
      !out->hint)
    return HB_EINVAL;
  DeviceGuard guard(h->device);
  const DecodeArgs da = decode_args(h, bytes, off, len, group, n, out, status);
  // on the stream the batches come from, so hb_step's prep orders after it
  hipStream_t ds = h->in_stream_set ? h->in_stream : h->stream;
  if (const int rc = decode_queue(h, n, ds, false)) return rc;
  hipLaunchKernelGGL(k_decode, dim3((unsigned)((n + DEC_THREADS - 1) / DEC_THREADS)), dim3(DEC_THREADS), 0, ds, da,
                     h->dec_q.get(), h->dec_qn.get());
  HB_CHECK(hipGetLastError());
  const uint64_t gb = (n + DEC_THREADS - 1) / DEC_THREADS;
  hipLaunchKernelGGL(k_decode_general, dim3((unsigned)(gb < DEC_GEN_BLOCKS ? gb : DEC_GEN_BLOCKS)), dim3(DEC_THREADS), 0,
                     ds, da, h->dec_q.get(), h->dec_qn.get());
  HB_CHECK(hipGetLastError());
  return HB_OK;
}

int hb_decode_caps(void) { return HB_DECODE_FOLLOW; }

int hb_decode_follow(hb_handle* h, const uint8_t* bytes, const uint64_t* off, const uint32_t* len, const uint32_t* group,
                     uint64_t n, const hb_batch* out, uint8_t* status, uint64_t ent_cap, uint64_t* edata,
                     uint64_t* n_ent) {
  if (!h || !out || !n_ent) return HB_EINVAL;
  if (n >= (1ull << 32) || n + 1 > h->max_batch) return HB_EINVAL;  // record n is the sentinel
  if (!out->group || !out->info || !out->term || !out->index || !out->hint || !out->commit || !out->eoff)
    return HB_EINVAL;
  if (n && (!bytes || !off || !len || !group || !status)) return HB_EINVAL;
  if (ent_cap && (!out->eterm || !out->edesc || !edata)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  DecfArgs fa;
  fa.d = decode_args(h, bytes, off, len, group, n, out, status);
  fa.o_commit = const_cast<uint64_t*>(out->commit);
  fa.eoff = const_cast<uint64_t*>(out->eoff);
  fa.eterm = const_cast<uint64_t*>(out->eterm);
  fa.edesc = const_cast<uint32_t*>(out->edesc);
  fa.edata = edata;
  fa.ent_cap = ent_cap;
  fa.n_ent = dev_view(n_ent);
  const bool props = (h->wire_props & HB_WIRE_PROPS_IN) != 0;
  // on the stream the batches come from, as hb_decode
  hipStream_t ds = h->in_stream_set ? h->in_stream : h->stream;
  const uint64_t nblk = (n + DEC_THREADS - 1) / DEC_THREADS;
  if (const int rc = decode_queue(h, n, ds, true)) return rc;  // (shared with hb_decode)
  if (nblk + 1 > h->decf_sum.cap()) {
    HB_CHECK(hipStreamSynchronize(ds));
    if (const int rc = reserve_pair(h->decf_sum, nblk + 1, h->decf_base, nblk + 2)) return rc;
  }
  fa.bsum = h->decf_sum.get();
  fa.bbase = h->decf_base.get();
  if (nblk) {
    if (props)
      hipLaunchKernelGGL(k_decf_parse<true>, dim3((unsigned)nblk), dim3(DEC_THREADS), 0, ds, fa, h->dec_q.get(),
                         h->dec_qn.get());
    else
      hipLaunchKernelGGL(k_decf_parse<false>, dim3((unsigned)nblk), dim3(DEC_THREADS), 0, ds, fa, h->dec_q.get(),
                         h->dec_qn.get());
    HB_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_decf_general, dim3((unsigned)(nblk < DEC_GEN_BLOCKS ? nblk : DEC_GEN_BLOCKS)), dim3(DEC_THREADS),
                       0, ds, fa, h->dec_q.get(), h->dec_qn.get());
    HB_CHECK(hipGetLastError());
  }
  if (n <= DECF_SMALL_MAX && !h->no_small) {
    if (props) hipLaunchKernelGGL(k_decf_small<true>, dim3(1), dim3(DEC_THREADS), 0, ds, fa, (uint32_t)nblk);
    else hipLaunchKernelGGL(k_decf_small<false>, dim3(1), dim3(DEC_THREADS), 0, ds, fa, (uint32_t)nblk);
  } else {
    hipLaunchKernelGGL(k_decf_scan, dim3(1), dim3(1024), 0, ds, fa, (uint32_t)nblk);
    if (nblk && props)
      hipLaunchKernelGGL(k_decf_write<true>, dim3((unsigned)nblk), dim3(DEC_THREADS), 0, ds, fa, (uint32_t)nblk);
    else if (nblk)
      hipLaunchKernelGGL(k_decf_write<false>, dim3((unsigned)nblk), dim3(DEC_THREADS), 0, ds, fa, (uint32_t)nblk);
  }
  HB_CHECK(hipGetLastError());
  return HB_OK;
}

int hb_tick(hb_handle* h, uint32_t flags) {
  if (!h || flags) return HB_EINVAL;
  DeviceGuard guard(h->device);
  hipStream_t st = h->stream;
  const bool two = h->in_stream_set && h->in_stream != h->stream;
  PrepSet& ps = h->set[h->next_set];
  ApplyArgs aa{};
  aa.S = h->st;
  aa.ev = h->ev;
  aa.ev_per_msg = h->ev_per_msg;
  aa.NB = h->NB;
  aa.NBK = h->NBK;
  aa.sis_log = h->sis_log;
  aa.ev_counts = ps.ev_counts;
  aa.ev_off = ps.ev_off;
  aa.stats_shard = h->stats_shard;
  const uint32_t grid = apply_grid(h);
  if (h->egress) egress_snapshot(h, st);
  switch (h->nmax) {
    case 3: hipLaunchKernelGGL(k_tick<3>, dim3(grid), dim3(PART), 0, st, aa); break;
    case 5: hipLaunchKernelGGL(k_tick<5>, dim3(grid), dim3(PART), 0, st, aa); break;
    default: hipLaunchKernelGGL(k_tick<7>, dim3(grid), dim3(PART), 0, st, aa); break;
  }
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(128), 0, st, h->stats_shard, h->stats, h->stats_accum);
  if (two) HB_CHECK(hipEventRecord(ps.applied, st));  // a later prep reusing this set waits for it
  HB_CHECK(hipGetLastError());
  ps.used = true;
  h->cur = h->next_set;
  h->next_set ^= 1;
  h->stepped = true;
  h->kern = 0;
  return HB_OK;
}

int hb_get_inflights(hb_handle* h, uint32_t group, uint32_t slot, uint32_t* start, uint32_t* count,
                     uint64_t* vals) {
  if (!h || group >= h->G || slot >= h->nmax || !start || !count || !vals) return HB_EINVAL;
  DeviceGuard guard(h->device);
  Dev<uint64_t> d;
  Dev<uint32_t> sc;
  if (reserve_pair(d, h->W, sc, 2) != HB_OK) return HB_ENOMEM;
  hipLaunchKernelGGL(k_get_ins, dim3(1), dim3(256), 0, h->stream, h->st, group, slot, d.get(), sc.get());
  uint32_t hsc[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(hsc, sc.get(), 8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess && hsc[1]) e = hipMemcpy(vals, d.get(), 8ull * hsc[1], hipMemcpyDeviceToHost);
  *start = hsc[0];
  *count = hsc[1];
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_step(hb_handle* h, const hb_batch* b, uint32_t flags) {
  if (!h || !b || b->n > h->max_batch) return HB_EINVAL;
  if (b->n && (!b->group || !b->info || !b->term || !b->index)) return HB_EINVAL;
  const bool sized = sz_on(h->max_msg_size);  // appended entries carry descriptors
  if (sized && ((b->n && !b->eoff) || (b->props && !b->peoff) || (b->n_edesc && !b->edesc))) return HB_EINVAL;
  // MsgApp entry terms need their per-message offsets, and described entries
  // need terms or descriptors (else a MsgApp's entries would silently vanish)
  if ((b->eterm && b->n && !b->eoff) || (b->n_edesc && !b->eterm && !b->edesc)) return HB_EINVAL;
  if ((flags & HB_STEP_HOST_PTRS) && b->eoff) {  // offsets non-decreasing and within the entries
    uint64_t prev = 0;
    for (uint64_t i = 0; i < b->n; ++i) {
      if (b->eoff[i] < prev || b->eoff[i] > b->n_edesc) return HB_EINVAL;
      prev = b->eoff[i];
    }
  }
  DeviceGuard guard(h->device);
  hipStream_t st = h->stream;  // apply stream
  // prep stream (partition + route): the library's own stream when the caller
  // named a separate input stream, else the apply stream itself (no hops)
  const bool two = h->in_stream_set && h->in_stream != h->stream;
  hipStream_t ps_st = two ? h->prep : st;
  const bool prof = (flags & HB_STEP_PROFILE) != 0;
  const bool prof_apply = prof || (flags & HB_STEP_PROFILE_APPLY) != 0;
  PrepSet& ps = h->set[h->next_set];
  hipEvent_t* ev = h->ph[h->prof_n % hb_handle::PROF_RING];

  // ---- prep inputs.  The prep stream waits for (a) the inputs: the input
  // stream's work so far (default: the apply stream, i.e. no overlap), (b) the
  // last apply that read this prep set (two steps ago).
  BatchDev bd{b->group, b->info, b->term, b->index, b->hint, b->props, b->n};
  const uint32_t* bd_edesc = b->edesc;
  const uint64_t* bd_eoff = b->eoff;
  const uint64_t* bd_peoff = b->peoff;
  const uint64_t* bd_commit = b->commit;
  const uint64_t* bd_eterm = b->eterm;
  if (two) {
    HB_CHECK(hipEventRecord(h->in_ready, h->in_stream));
    HB_CHECK(hipStreamWaitEvent(ps_st, h->in_ready, 0));
    if (ps.used) HB_CHECK(hipStreamWaitEvent(ps_st, ps.applied, 0));
  }
  // Host-pointer batches.  Small ones (the host MultiNode's Ready cycles) are
  // packed into one pinned block and sent with ONE copy; larger ones go
  // array by array into the handle's staging buffers.
  bool packed = false;
  if (flags & HB_STEP_HOST_PTRS) {
    const size_t n = b->n;
    struct Part {
      const void* src;
      size_t bytes;
      size_t off;
    };
    Part parts[11] = {{b->group, n * 4, 0},
                      {b->info, n * 4, 0},
                      {b->term, n * 8, 0},
                      {b->index, n * 8, 0},
                      {b->hint, b->hint ? n * 8 : 0, 0},
                      {b->props, b->props ? (size_t)h->G * 4 : 0, 0},
                      {b->edesc, (sized && b->edesc) ? b->n_edesc * 4 : 0, 0},
                      {b->eterm, b->eterm ? b->n_edesc * 8 : 0, 0},
                      {b->eoff, b->eoff ? n * 8 : 0, 0},
                      {b->commit, b->commit ? n * 8 : 0, 0},
                      {b->peoff, (sized && b->props) ? (size_t)h->G * 8 : 0, 0}};
    size_t total = 0;
    for (Part& q : parts) {
      q.off = total;
      total += (q.src && q.bytes) ? (q.bytes + 255) & ~(size_t)255 : 0;
    }
    if (total > 0 && total <= STAGE_MAX) {
      packed = true;
      // both blocks are STAGE_MAX bytes from their first use
      int rc = h->hstage.reserve(total, STAGE_MAX, [h]() -> int {
        HB_CHECK(hipEventSynchronize(h->hstage_done));
        return HB_OK;
      });
      // (this set's last reader is done: the prep stream waited for it)
      if (rc == HB_OK) rc = ps.dstage.reserve(total, STAGE_MAX, stream_idle(st));
      if (rc != HB_OK) return rc;
      HB_CHECK(hipEventSynchronize(h->hstage_done));  // the previous step's copy has left the block
      for (const Part& q : parts)
        if (q.src && q.bytes) std::memcpy(h->hstage.get() + q.off, q.src, q.bytes);
      HB_CHECK(hipMemcpyAsync(ps.dstage.get(), h->hstage.get(), total, hipMemcpyHostToDevice, ps_st));
      HB_CHECK(hipEventRecord(h->hstage_done, ps_st));
      auto at = [&](int k) { return parts[k].src && parts[k].bytes ? ps.dstage.get() + parts[k].off : nullptr; };
      bd.group = reinterpret_cast<const uint32_t*>(at(0));
      bd.info = reinterpret_cast<const uint32_t*>(at(1));
      bd.term = reinterpret_cast<const uint64_t*>(at(2));
      bd.index = reinterpret_cast<const uint64_t*>(at(3));
      bd.hint = reinterpret_cast<const uint64_t*>(at(4));
      bd.props = reinterpret_cast<const uint32_t*>(at(5));
      bd_edesc = reinterpret_cast<const uint32_t*>(at(6));
      bd_eterm = reinterpret_cast<const uint64_t*>(at(7));
      bd_eoff = reinterpret_cast<const uint64_t*>(at(8));
      bd_commit = reinterpret_cast<const uint64_t*>(at(9));
      bd_peoff = reinterpret_cast<const uint64_t*>(at(10));
    }
  }
  if ((flags & HB_STEP_HOST_PTRS) && !packed) {
    // partition inputs on the prep stream (staging is reused in prep-stream
    // order); props / hint are read by apply, so they go on the apply stream.
    const size_t n = b->n;
    if (n) {
      HB_CHECK(hipMemcpyAsync(h->s_group, b->group, n * 4, hipMemcpyHostToDevice, ps_st));
      HB_CHECK(hipMemcpyAsync(h->s_info, b->info, n * 4, hipMemcpyHostToDevice, ps_st));
      HB_CHECK(hipMemcpyAsync(h->s_term, b->term, n * 8, hipMemcpyHostToDevice, ps_st));
      HB_CHECK(hipMemcpyAsync(h->s_index, b->index, n * 8, hipMemcpyHostToDevice, ps_st));
      if (b->hint) HB_CHECK(hipMemcpyAsync(h->s_hint, b->hint, n * 8, hipMemcpyHostToDevice, st));
    }
    if (b->props) HB_CHECK(hipMemcpyAsync(h->s_props, b->props, (size_t)h->G * 4, hipMemcpyHostToDevice, st));
    bd.group = h->s_group;
    bd.info = h->s_info;
    bd.term = h->s_term;
    bd.index = h->s_index;
    bd.hint = b->hint ? h->s_hint : nullptr;
    bd.props = b->props ? h->s_props : nullptr;
    // entry descriptors / terms, m.Commit: read by apply, so on the apply stream
    // (the old staging may still be read: the apply stream goes idle before it is replaced)
    if (sized && b->edesc && b->n_edesc) {
      if (const int rc = h->s_edesc.reserve(b->n_edesc, 0, stream_idle(st))) return rc;
      HB_CHECK(hipMemcpyAsync(h->s_edesc.get(), b->edesc, b->n_edesc * 4, hipMemcpyHostToDevice, st));
    }
    if (b->eterm && b->n_edesc) {
      if (const int rc = h->s_eterm.reserve(b->n_edesc, 0, stream_idle(st))) return rc;
      HB_CHECK(hipMemcpyAsync(h->s_eterm.get(), b->eterm, b->n_edesc * 8, hipMemcpyHostToDevice, st));
    }
    if (b->eoff && n) HB_CHECK(hipMemcpyAsync(h->s_eoff, b->eoff, n * 8, hipMemcpyHostToDevice, st));
    if (b->commit && n) HB_CHECK(hipMemcpyAsync(h->s_commit, b->commit, n * 8, hipMemcpyHostToDevice, st));
    if (sized && b->props) HB_CHECK(hipMemcpyAsync(h->s_peoff, b->peoff, (size_t)h->G * 8, hipMemcpyHostToDevice, st));
    bd_edesc = (sized && b->edesc) ? h->s_edesc.get() : nullptr;
    bd_eterm = b->eterm ? h->s_eterm.get() : nullptr;
    bd_eoff = b->eoff ? h->s_eoff : nullptr;
    bd_commit = b->commit ? h->s_commit : nullptr;
    bd_peoff = (sized && b->props) ? h->s_peoff : nullptr;
  }
  if (prof) HB_CHECK(hipEventRecord(ev[0], ps_st));

  // ---- phase 1: partition (prep stream) ---------------------------------------
  const uint32_t NB = h->NB;
  // X mode: a follower-side batch (m.Commit given) carries {hint, commit} with every record
  const bool xmode = bd_commit != nullptr && b->n > 0;
  if (b->n == 0) {
    HB_CHECK(hipMemsetAsync(ps.bk_off, 0, (h->NBK + 1) * 4ull, ps_st));
    HB_CHECK(hipMemsetAsync(ps.bk_fill, 0, h->NBK * 4ull * CTR_STRIDE, ps_st));
    HB_CHECK(hipMemsetAsync(ps.ctr, 0, CTR_WORDS * 4ull, ps_st));
  } else {
    const uint32_t ntiles = (uint32_t)((b->n + RDX_TILE - 1) / RDX_TILE);
    RadixSrc src{bd.group, bd.info, bd.term, bd.index, nullptr, nullptr, ps.side, (uint32_t)b->n,
                 bd.hint, bd_commit, bd_eoff, bd_eterm, b->n_edesc, nullptr};
    const FinalDst fin{ps.rec, ps.recx, ps.bucket, h->passes == 1 ? ps.bk_off : nullptr, h->NBK, h->sis_log};
    uint32_t shift = PART_LOG + h->sis_log;
    if (h->passes == 1 && h->NBK == 1 && ntiles <= SMALL_TILES && !h->no_small) {  // one bucket: a compaction
      if (xmode)
        hipLaunchKernelGGL(k_pack_one<true>, dim3(1), dim3(RDX_THREADS), 0, ps_st, src, fin, h->G, ntiles, ps.bk_fill,
                           h->NBK, ps.ctr, h->n_valid);
      else
        hipLaunchKernelGGL(k_pack_one<false>, dim3(1), dim3(RDX_THREADS), 0, ps_st, src, fin, h->G, ntiles, ps.bk_fill,
                           h->NBK, ps.ctr, h->n_valid);
    } else if (h->passes == 1 && ntiles <= SMALL_TILES && !h->no_small) {  // one launch for the whole partition
      if (xmode)
        hipLaunchKernelGGL(k_radix_small<true>, dim3(1), dim3(RDX_THREADS), 0, ps_st, src, fin, h->G, shift, ntiles,
                           ps.bk_fill, h->NBK, ps.ctr, h->n_valid);
      else
        hipLaunchKernelGGL(k_radix_small<false>, dim3(1), dim3(RDX_THREADS), 0, ps_st, src, fin, h->G, shift, ntiles,
                           ps.bk_fill, h->NBK, ps.ctr, h->n_valid);
    }
    for (uint32_t p = 0; p < h->passes && !(h->passes == 1 && ntiles <= SMALL_TILES && !h->no_small); ++p) {
      const bool last_pass = p + 1 == h->passes;
      const RadixDst& dst = h->tmp[p & 1];
      // two passes split the bucket id's bits evenly (the first takes the low
      // half): 5 + 5 bits for 1,024 buckets write 64-message digit runs in both
      // passes, where 8 + 2 wrote 8-message runs (partial lines) in the first
      const uint32_t b0 = h->bk_bits / 2;
      const uint32_t dbits = h->passes == 1 ? RDX_BITS : p == 0 ? b0 : h->bk_bits - b0;
      const uint32_t dm = h->passes > 1;  // digit-major tile counts (k_scan_rows)
      const uint32_t nhw = (ntiles + HIST_TPB - 1) / HIST_TPB;
      const dim3 sg((ntiles + SCAT_TPW - 1) / SCAT_TPW);
      if (h->passes == 1) {  // hist + direct scatter: no scan launch
        const uint32_t k = h->sup_k, kn = (k + 1) % SUP_BUFS;
        const size_t bw = (size_t)h->sup_max * RDX_BINS;
        DirectSums dsum{h->hagg, h->hsup + k * bw, h->hsup + kn * bw, h->sup_used[kn] * RDX_BINS,
                        ps.bk_fill, h->NBK, ps.ctr};
        h->sup_used[kn] = 0;
        h->sup_used[k] = (nhw + SB_HW - 1) / SB_HW;
        h->sup_k = kn;
        hipLaunchKernelGGL(k_radix_hist, dim3(nhw), dim3(RDX_THREADS), 0, ps_st, src, h->G, shift, dbits, ntiles, h->hist,
                           0u, dsum);
        if (xmode)
          hipLaunchKernelGGL(k_radix_scatter_d<true>, sg, dim3(RDX_THREADS), 0, ps_st, src, fin, h->G, shift, ntiles,
                             (const uint32_t*)h->hist, (const uint32_t*)h->hagg, (const uint32_t*)dsum.sup, h->n_valid);
        else
          hipLaunchKernelGGL(k_radix_scatter_d<false>, sg, dim3(RDX_THREADS), 0, ps_st, src, fin, h->G, shift, ntiles,
                             (const uint32_t*)h->hist, (const uint32_t*)h->hagg, (const uint32_t*)dsum.sup, h->n_valid);
        break;  // (one pass)
      }
      hipLaunchKernelGGL(k_radix_hist, dim3(nhw), dim3(RDX_THREADS), 0, ps_st, src, h->G, shift, dbits, ntiles, h->hist,
                         dm, DirectSums{});
      hipLaunchKernelGGL(k_scan_rows, dim3(1u << dbits), dim3(1024), 0, ps_st, h->hist, ntiles, dbits, h->totals, ps.bk_fill,
                         h->NBK, ps.ctr, dm);
#define HB_SCATTER(F, X)                                                                                             \
  hipLaunchKernelGGL((k_radix_scatter<F, X>), sg, dim3(RDX_THREADS), 0, ps_st, src, dst, fin, h->G, shift, dbits, ntiles, \
                     (const uint32_t*)h->hist, dm ? ntiles : 1u, dm ? 1u : (1u << dbits), (const uint32_t*)h->totals,    \
                     h->n_valid)
      if (last_pass) {
        if (xmode) HB_SCATTER(true, true);
        else HB_SCATTER(true, false);
      } else {
        if (xmode) HB_SCATTER(false, true);
        else HB_SCATTER(false, false);
      }
#undef HB_SCATTER
      src = RadixSrc{dst.group, nullptr, nullptr, nullptr, dst.rec, h->n_valid, nullptr, (uint32_t)b->n,
                     nullptr, nullptr, nullptr, nullptr, 0, dst.recx};
      shift += dbits;
    }
    if (h->passes > 1)
      hipLaunchKernelGGL(k_bucket_bounds, dim3((h->NBK + 1 + 255) / 256), dim3(256), 0, ps_st,
                         (const uint32_t*)ps.bucket, (const uint32_t*)h->n_valid, h->NBK, ps.bk_off);
  }

  // ---- phase 2: route each partition's messages to its lanes (prep stream) ----
  ApplyArgs aa{};
  aa.S = h->st;
  aa.S.edesc = bd_edesc;
  aa.S.eoff = bd_eoff;
  aa.S.peoff = bd_peoff;
  aa.S.bcommit = bd_commit;
  aa.S.eterm = bd_eterm;
  aa.S.n_ent = b->n_edesc;
  aa.S.bn = b->n;
  aa.ap_cnt = ps.ctr + CTR_AP;
  aa.ap_list = h->ap_list;
  aa.fl_cnt = ps.ctr + CTR_FL;
  aa.fl_list = h->fl_list;
  aa.eflag = h->eflag;
  aa.el_cnt = ps.ctr + CTR_EL;
  aa.el_list = h->el_list;
  aa.grid = apply_grid(h);
  aa.sis_log = h->sis_log;
  aa.done = ps.ctr + CTR_DONE;
  aa.stats = h->stats;
  aa.accum = h->stats_accum;
  aa.rec = ps.rec;
  aa.key = ps.key;
  aa.bk_off = ps.bk_off;
  aa.bk_fill = ps.bk_fill;
  aa.hint = bd.hint;
  aa.props = bd.props;
  aa.ev = h->ev;
  aa.ev_per_msg = h->ev_per_msg;
  aa.props_on = bd.props ? 1u : 0u;
  aa.NB = NB;
  aa.NBK = h->NBK;
  aa.ev_counts = ps.ev_counts;
  aa.ev_off = ps.ev_off;
  aa.stats_shard = h->stats_shard;
  aa.pflag = h->pflag;
  aa.resume = h->resume;
  aa.commit0 = h->commit0;
  aa.kmax = step_kmax(h->nmax, flags);
  aa.cnt = ps.cnt;
  aa.slot = ps.slot;
  aa.side = ps.side;
  aa.recx = ps.recx;
  aa.slotx = xmode ? ps.slotx : nullptr;
  aa.nmax = h->nmax;
  aa.lskip = h->lskip;
  aa.steady = h->steady ? 1u : 0u;
  aa.steady_cnt = h->steady_count ? ps.ctr + CTR_STEADY : nullptr;
  // the route's storm hand-over writes the handle's flags and lists: only when
  // the apply of the previous step is not running beside it (one stream)
  aa.storm = (h->nmax >= 5 && !two && !xmode && !bd.props) ? h->storm : 0u;
  // n = 3, prep and apply on one stream: the route runs inside the fast
  // kernel's workgroups (k_route_fast; two-pass handles too: cfg5 0.998 ->
  // 0.931 ms/step same box)
  const bool fused = h->nmax == 3 && !two && (h->fuse >= 2 || (h->fuse == 1 && h->passes == 1)) &&
                     PART_LOG + h->sis_log >= route_fast_rg_log(h, aa.kmax, xmode);
  // Egress: the term and last columns as they are before this step, on the
  // apply stream.  One stream: the route below is the first kernel that can
  // write them (its storm hand-over runs the election lane).  Two stages: the
  // route runs on the prep stream without the hand-over (aa.storm = 0) and
  // writes no group state, so the copy is ordered after the previous step's
  // apply and before this step's, the only writers.
  if (h->egress) egress_snapshot(h, st);
  switch (h->nmax) {
    case 3:
      if (fused) break;
      if (aa.kmax == 3) launch_route<3>(h, aa, ps_st);
      else launch_route<2>(h, aa, ps_st);
      break;
    case 5: launch_route<route_kmax(5)>(h, aa, ps_st); break;
    default: launch_route<route_kmax(7)>(h, aa, ps_st); break;
  }
  if (prof) HB_CHECK(hipEventRecord(ev[1], ps_st));
  if (two) {
    HB_CHECK(hipEventRecord(ps.prepped, ps_st));
    // ---- phase 3: apply (apply stream, after the previous step's apply) ------
    HB_CHECK(hipStreamWaitEvent(st, ps.prepped, 0));
  }
  switch (h->nmax) {
    case 3: launch_apply<3>(h, aa, prof_apply ? ev : nullptr, prof, fused); break;
    case 5: launch_apply<5>(h, aa, prof_apply ? ev : nullptr, prof); break;
    default: launch_apply<7>(h, aa, prof_apply ? ev : nullptr, prof); break;
  }
  if (prof) HB_CHECK(hipEventRecord(ev[5], st));  // (the finish runs inside k_follow)
  if (two) HB_CHECK(hipEventRecord(ps.applied, st));
  HB_CHECK(hipGetLastError());
  ps.used = true;
  h->cur = h->next_set;
  h->next_set ^= 1;
  if (prof_apply) {
    h->prof_full[h->prof_n % hb_handle::PROF_RING] = prof;
    h->prof_n++;
  }
  h->stepped = true;
  h->kern = (fused ? HB_KERN_ROUTE_FAST : 0u) | (aa.storm ? HB_KERN_ROUTE_ELECT : 0u) |
            (fused && route_fast_wide(h, aa.kmax, xmode) ? HB_KERN_ROUTE_FAST_WIDE : 0u);
  return HB_OK;
}

int hb_events_device(hb_handle* h, const uint64_t** base, const uint64_t** chunk_off, const uint32_t** counts,
                     uint32_t* n_chunks) {
  if (!h || !base || !chunk_off || !counts || !n_chunks) return HB_EINVAL;
  *base = h->ev;
  *chunk_off = h->set[h->cur].ev_off;
  *counts = h->set[h->cur].ev_counts;
  *n_chunks = 2 * h->NB;
  return HB_OK;
}

int hb_copy_events(hb_handle* h, hb_event* out, uint64_t cap, uint64_t* n) {
  if (!h || !n) return HB_EINVAL;
  DeviceGuard guard(h->device);
  HB_CHECK(hipMemcpyAsync(h->stats_pin.get(), h->stats, HB_STAT_COUNT * 8, hipMemcpyDeviceToHost, h->stream));
  HB_CHECK(hipStreamSynchronize(h->stream));
  const uint64_t total = h->stepped ? h->stats_pin.get()[HB_STAT_EVENTS] : 0;
  *n = total;
  if (total == 0) return HB_OK;
  if (!out || cap < total) return HB_EINVAL;
  // expansion scratch (records + per-chunk scan), kept across calls; it grows with a quarter to spare
  const uint64_t need = total * sizeof(hb_event) + 24ull * h->NB;
  if (const int rc = h->evx.reserve(need, need + need / 4)) return rc;
  hb_event* d = reinterpret_cast<hb_event*>(h->evx.get());
  uint64_t* dst = reinterpret_cast<uint64_t*>(d + total);
  uint32_t* per_chunk = reinterpret_cast<uint32_t*>(dst + 2 * h->NB);
  hipLaunchKernelGGL(k_chunk_events, dim3(2 * h->NB), dim3(256), 0, h->stream, (const uint64_t*)h->ev,
                     (const uint32_t*)h->set[h->cur].ev_counts, (const uint64_t*)h->set[h->cur].ev_off, per_chunk);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, h->stream, (const uint32_t*)per_chunk, 2 * h->NB, dst);
  hipLaunchKernelGGL(k_expand_events, dim3(2 * h->NB), dim3(256), 0, h->stream, (const uint64_t*)h->ev,
                     (const uint32_t*)h->set[h->cur].ev_counts, (const uint64_t*)h->set[h->cur].ev_off, (const uint64_t*)dst, d);
  hipError_t e = hipMemcpyAsync(out, d, total * sizeof(hb_event), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  return e == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_events_to_host(hb_handle* h, uint64_t* words, uint64_t cap, uint32_t* counts, uint64_t* total) {
  if (!h || !counts || !total || (cap && !words)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  void *dw = nullptr, *dc = nullptr, *dt = nullptr;
  if (hipHostGetDevicePointer(&dc, counts, 0) != hipSuccess || hipHostGetDevicePointer(&dt, total, 0) != hipSuccess ||
      (cap && hipHostGetDevicePointer(&dw, words, 0) != hipSuccess))
    return HB_EINVAL;  // not memory from hb_alloc_pinned
  const uint32_t nc = 2 * h->NB;
  if (!h->stepped) {  // no step yet: no events
    HB_CHECK(hipMemsetAsync(dc, 0, nc * 4ull, h->stream));
    HB_CHECK(hipMemsetAsync(dt, 0, 8, h->stream));
    return HB_OK;
  }
  if (const int rc = h->evw.reserve(nc + 1ull)) return rc;
  const PrepSet& ps = h->set[h->cur];
  if (nc <= WORDS_SMALL && !h->no_small) {
    hipLaunchKernelGGL(k_words_small, dim3(1), dim3(1024), 0, h->stream, (const uint32_t*)ps.ev_counts, nc,
                       (const uint64_t*)h->ev, (const uint64_t*)ps.ev_off, static_cast<uint64_t*>(dw), cap,
                       static_cast<uint32_t*>(dc), static_cast<uint64_t*>(dt));
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  hipLaunchKernelGGL(k_scan_words, dim3(1), dim3(1024), 0, h->stream, (const uint32_t*)ps.ev_counts, nc, h->evw.get(),
                     static_cast<uint32_t*>(dc), static_cast<uint64_t*>(dt));
  hipLaunchKernelGGL(k_gather_words, dim3(nc), dim3(256), 0, h->stream, (const uint64_t*)h->ev,
                     (const uint32_t*)ps.ev_counts, (const uint64_t*)ps.ev_off, (const uint64_t*)h->evw.get(),
                     static_cast<uint64_t*>(dw), cap);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

// ---- wire egress ---------------------------------------------------------------
// the snapshot columns of a mode: lterm0 in vote and append mode, commit0 / bl0 / blt0 in append mode
static int egress_reserve_cols(hb_handle* h, bool lt, bool apps) {
  const uint64_t G = h->G;
  int rc = lt ? h->lterm0.reserve(G) : HB_OK;
  for (Dev<uint64_t>* c : {&h->eg_commit0, &h->bl0, &h->blt0})
    if (apps && rc == HB_OK) rc = c->reserve(G);
  return rc;
}
// only a mode's own columns stay
static void egress_keep_cols(hb_handle* h, bool lt, bool apps) {
  if (!lt) h->lterm0.release();
  if (apps) return;
  h->eg_commit0.release();
  h->bl0.release();
  h->blt0.release();
}
int hb_set_egress(hb_handle* h, int on) {
  if (!h) return HB_EINVAL;
  DeviceGuard guard(h->device);
  const bool votes = on && (on & HB_EGRESS_VOTES), apps = on && (on & HB_EGRESS_APPS);
  if (h->egress && (!on || votes != h->eg_votes || apps != h->eg_apps))
    HB_CHECK(hipStreamSynchronize(h->stream));  // an hb_egress may still read the columns
  auto drop_all = [h] {
    h->term0.release();
    h->last0.release();
    h->eg_cnt.release();
    h->eg_base.release();
    egress_keep_cols(h, false, false);
  };
  if (!on) {
    if (!h->egress) return HB_OK;
    drop_all();
    h->egress = h->eg_votes = h->eg_apps = false;
    return HB_OK;
  }
  const uint64_t G = h->G, nc = 2 * (uint64_t)h->NB;
  if (h->egress) {
    if (votes == h->eg_votes && apps == h->eg_apps) return HB_OK;
    // the mode changes: the step before this call has no matching snapshot
    h->eg_stepped = false;
    if (const int rc = egress_reserve_cols(h, votes || apps, apps)) {  // (the mode in force stays; nothing new is kept)
      egress_keep_cols(h, h->eg_votes || h->eg_apps, h->eg_apps);
      return rc;
    }
    egress_keep_cols(h, votes || apps, apps);  // (the new columns exist: the old mode's others go)
    h->eg_votes = votes;
    h->eg_apps = apps;
    return HB_OK;
  }
  int rc = h->term0.reserve(G);
  if (rc == HB_OK) rc = h->last0.reserve(G);
  if (rc == HB_OK) rc = h->eg_cnt.reserve(nc);
  if (rc == HB_OK) rc = h->eg_base.reserve(nc + 1);
  if (rc == HB_OK) rc = egress_reserve_cols(h, votes || apps, apps);
  if (rc != HB_OK) {
    drop_all();
    return rc;
  }
  h->egress = true;
  h->eg_votes = votes;
  h->eg_apps = apps;
  h->eg_stepped = false;  // the step before this call has no snapshot: its events are not replayed
  return HB_OK;
}

int hb_egress_mode(hb_handle* h) {
  if (!h) return HB_EINVAL;
  return h->egress ? (HB_EGRESS_ON | (h->eg_votes ? HB_EGRESS_VOTES : 0) | (h->eg_apps ? HB_EGRESS_APPS : 0)) : 0;
}

int hb_egress_caps(void) { return HB_EGRESS_ON | HB_EGRESS_VOTES | HB_EGRESS_APPS; }

int hb_set_egress_limit(hb_handle* h, int on) {
  if (!h) return HB_EINVAL;
  const bool want = on != 0;
  if (want == h->eg_limit) return HB_OK;
  if (h->egress) {  // as a mode change: an hb_egress may be in flight, and the step before has no say
    DeviceGuard guard(h->device);
    HB_CHECK(hipStreamSynchronize(h->stream));
    h->eg_stepped = false;
  }
  h->eg_limit = want;
  return HB_OK;
}

int hb_egress_limit(hb_handle* h) { return h ? (h->eg_limit ? 1 : 0) : HB_EINVAL; }

int hb_egress_limit_caps(void) { return HB_EGRESS_LIMIT_V1; }

int hb_set_egress_logterm(hb_handle* h, int on) {
  if (!h) return HB_EINVAL;
  const bool want = on != 0;
  if (want == h->eg_logterm) return HB_OK;
  if (h->egress) {  // as hb_set_egress_limit: a mode change
    DeviceGuard guard(h->device);
    HB_CHECK(hipStreamSynchronize(h->stream));
    h->eg_stepped = false;
  }
  h->eg_logterm = want;
  return HB_OK;
}

int hb_egress_logterm(hb_handle* h) { return h ? (h->eg_logterm ? 1 : 0) : HB_EINVAL; }

int hb_egress_logterm_caps(void) { return HB_EGRESS_LOGTERM_V1; }

int hb_set_wire_props(hb_handle* h, int bits) {
  if (!h || (bits & ~(HB_WIRE_PROPS_IN | HB_WIRE_PROPS_OUT)) != 0) return HB_EINVAL;
  if (bits == h->wire_props) return HB_OK;
  // a configuration call: an hb_egress or hb_decode_follow may be in flight (the forward record
  // reads no pre-step column, so the events of the step before stay good)
  DeviceGuard guard(h->device);
  HB_CHECK(hipStreamSynchronize(h->stream));
  if (h->in_stream_set) HB_CHECK(hipStreamSynchronize(h->in_stream));
  h->wire_props = bits;
  return HB_OK;
}

int hb_wire_props(hb_handle* h) { return h ? h->wire_props : HB_EINVAL; }

int hb_wire_props_caps(void) { return HB_WIRE_PROPS_IN | HB_WIRE_PROPS_OUT; }

int hb_egress(hb_handle* h, uint64_t self_id, const hb_out_batch* out, uint64_t cap, uint64_t* count) {
  (void)self_id;  // m.From: hb_encode writes it; the batch holds no sender
  if (!h || !out || !count) return HB_EINVAL;
  if (!out->group || !out->info || !out->to || !out->term || !out->log_term || !out->index || !out->commit ||
      !out->hint)
    return HB_EINVAL;
  if (!h->egress || !h->peer) return HB_EINVAL;
  DeviceGuard guard(h->device);
  uint64_t* dcount = dev_view(count);
  if (!h->eg_stepped) {  // no step since hb_set_egress: no events
    HB_CHECK(hipMemsetAsync(dcount, 0, 8, h->stream));
    return HB_OK;
  }
  const PrepSet& ps = h->set[h->cur];
  EgressArgs ea;
  ea.ev = h->ev;
  ea.ev_off = ps.ev_off;
  ea.ev_counts = ps.ev_counts;
  ea.nc = 2 * h->NB;
  ea.G = h->G;
  ea.term0 = h->term0.get();
  ea.last0 = h->last0.get();
  ea.peer = h->peer.get();
  ea.lterm0 = h->lterm0.get();
  ea.commit0 = h->eg_commit0.get();
  ea.bl0 = h->bl0.get();
  ea.blt0 = h->blt0.get();
  ea.max_msg_size = h->max_msg_size;
  const bool cut = h->eg_limit && h->eg_apps && sz_on(h->max_msg_size);
  ea.szx = cut ? h->st.szx : nullptr;
  ea.szlo = cut ? h->st.szlo : nullptr;
  const bool lt = h->eg_logterm && h->eg_apps;
  ea.trx = lt ? h->st.trx : nullptr;
  ea.trc = lt ? h->st.trc : nullptr;
  ea.ccnt = h->eg_cnt.get();
  ea.cbase = h->eg_base.get();
  ea.cap = cap;
  ea.count = dcount;
  ea.o_group = out->group;
  ea.o_info = out->info;
  ea.o_to = out->to;
  ea.o_term = out->term;
  ea.o_log_term = out->log_term;
  ea.o_index = out->index;
  ea.o_commit = out->commit;
  ea.o_hint = out->hint;
  const bool small = ea.nc <= EG_SMALL && !h->no_small;
  // (the instantiations without APPS are the ones a handle without the bit always ran)
  // (a word's record count does not depend on the cut: the count kernels are append mode's)
  // (with HB_WIRE_PROPS_OUT off the instantiations are the ones a handle without the knob ran)
  const bool fwd = (h->wire_props & HB_WIRE_PROPS_OUT) != 0;
#define EG_LAUNCH_F(V, A, C, F, L)                                                                    \
  do {                                                                                               \
    if (small) hipLaunchKernelGGL((k_eg_small<V, A, F>), dim3(1), dim3(1024), 0, h->stream, ea);    \
    else {                                                                                           \
      hipLaunchKernelGGL((k_eg_count<V, A, F>), dim3(ea.nc), dim3(256), 0, h->stream, ea);          \
      hipLaunchKernelGGL(k_eg_scan, dim3(1), dim3(1024), 0, h->stream, ea);                         \
    }                                                                                                \
    hipLaunchKernelGGL((k_egress<V, A, C, F, L>), dim3(h->NB), dim3(PART), 0, h->stream, ea);       \
  } while (0)
#define EG_LAUNCH(V, A, C)                        \
  do {                                            \
    if (fwd) EG_LAUNCH_F(V, A, C, true, false);   \
    else EG_LAUNCH_F(V, A, C, false, false);      \
  } while (0)
  // (the lookup's instantiations exist for append mode only; with the knob off the ones above run)
#define EG_LAUNCH_LT(V, C)                          \
  do {                                              \
    if (fwd) EG_LAUNCH_F(V, true, C, true, true);   \
    else EG_LAUNCH_F(V, true, C, false, true);      \
  } while (0)
  if (lt) {
    if (cut) {
      if (h->eg_votes) EG_LAUNCH_LT(true, true);
      else EG_LAUNCH_LT(false, true);
    } else if (h->eg_votes) EG_LAUNCH_LT(true, false);
    else EG_LAUNCH_LT(false, false);
  } else if (cut) {
    if (h->eg_votes) EG_LAUNCH(true, true, true);
    else EG_LAUNCH(false, true, true);
  } else if (h->eg_apps) {
    if (h->eg_votes) EG_LAUNCH(true, true, false);
    else EG_LAUNCH(false, true, false);
  } else if (h->eg_votes) EG_LAUNCH(true, false, false);
  else EG_LAUNCH(false, false, false);
#undef EG_LAUNCH_LT
#undef EG_LAUNCH
#undef EG_LAUNCH_F
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_encode(hb_handle* h, const hb_out_batch* in, uint64_t cap, const uint64_t* n_dev, uint64_t self_id,
              uint8_t* bytes, uint64_t bytes_cap, uint64_t* off, uint8_t* status, uint64_t* total) {
  if (!h || !in || !off || !status || !total || (bytes_cap && !bytes)) return HB_EINVAL;
  if (!in->group || !in->info || !in->to || !in->term || !in->log_term || !in->index || !in->commit || !in->hint)
    return HB_EINVAL;
  const uint64_t cap_max = h->max_batch * (h->nmax + 4ull);
  // (byte offsets inside the kernels' scans are 32-bit: 91 bytes a record at most)
  if (cap > cap_max || cap * WO_MAX >= (1ull << 32)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  EncodeArgs ea;
  ea.info = in->info;
  ea.to = in->to;
  ea.term = in->term;
  ea.log_term = in->log_term;
  ea.index = in->index;
  ea.commit = in->commit;
  ea.hint = in->hint;
  ea.cap = cap;
  ea.n_dev = dev_view(n_dev);
  ea.self_id = self_id;
  ea.bytes = bytes;
  ea.bytes_cap = bytes_cap;
  ea.off = off;
  ea.status = status;
  ea.total = dev_view(total);
  ea.bsum = nullptr;
  ea.bbase = nullptr;
  if (cap <= ENC_SMALL_MAX && !h->no_small) {
    hipLaunchKernelGGL(k_enc_small, dim3(1), dim3(ENC_SMALL_THREADS), 0, h->stream, ea);
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  if (!h->enc_sum) {  // once, for the largest batch the handle takes
    const uint64_t cm = cap_max * WO_MAX >= (1ull << 32) ? ((1ull << 32) - 1) / WO_MAX : cap_max;
    const uint64_t nb = (cm + ENC_THREADS - 1) / ENC_THREADS + 1;
    if (const int rc = reserve_pair(h->enc_sum, nb, h->enc_base, nb + 1)) return rc;
  }
  ea.bsum = h->enc_sum.get();
  ea.bbase = h->enc_base.get();
  const uint32_t nblk = (uint32_t)((cap + ENC_THREADS - 1) / ENC_THREADS);
  if (nblk == 0) {  // (cap 0 with the small path off)
    hipLaunchKernelGGL(k_enc_small, dim3(1), dim3(ENC_SMALL_THREADS), 0, h->stream, ea);
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  hipLaunchKernelGGL(k_enc_size, dim3(nblk), dim3(ENC_THREADS), 0, h->stream, ea);
  hipLaunchKernelGGL(k_enc_scan, dim3(1), dim3(1024), 0, h->stream, ea, nblk);
  hipLaunchKernelGGL(k_enc_write, dim3(nblk), dim3(ENC_THREADS), 0, h->stream, ea, nblk);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_encode_caps(void) { return HB_ENCODE_ENTS; }

int hb_encode_ents(hb_handle* h, const hb_out_batch* in, uint64_t cap, const uint64_t* n_dev, uint64_t self_id,
                   const hb_ent_source* src, uint8_t* bytes, uint64_t bytes_cap, uint64_t* off, uint8_t* status,
                   uint64_t* total) {
  if (!h || !in || !src || !off || !status || !total || (bytes_cap && !bytes)) return HB_EINVAL;
  if (!in->group || !in->info || !in->to || !in->term || !in->log_term || !in->index || !in->commit || !in->hint)
    return HB_EINVAL;
  if (!src->first || !src->count || !src->start) return HB_EINVAL;
  if (src->n_ent && (!src->eterm || !src->edesc || !src->edata)) return HB_EINVAL;
  if (src->data_len && !src->data) return HB_EINVAL;
  const uint64_t cap_max = h->max_batch * (h->nmax + 4ull);
  if (cap > cap_max || cap >= (1ull << 32)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  EnceArgs ea;
  ea.e.info = in->info;
  ea.e.to = in->to;
  ea.e.term = in->term;
  ea.e.log_term = in->log_term;
  ea.e.index = in->index;
  ea.e.commit = in->commit;
  ea.e.hint = in->hint;
  ea.e.cap = cap;
  ea.e.n_dev = dev_view(n_dev);
  ea.e.self_id = self_id;
  ea.e.bytes = bytes;
  ea.e.bytes_cap = bytes_cap;
  ea.e.off = off;
  ea.e.status = status;
  ea.e.total = dev_view(total);
  ea.e.bsum = nullptr;
  ea.e.bbase = nullptr;
  ea.group = in->group;
  ea.capacity = h->G;
  ea.first = src->first;
  ea.count = src->count;
  ea.start = src->start;
  ea.n_ent = src->n_ent;
  ea.eterm = src->eterm;
  ea.edesc = src->edesc;
  ea.edata = src->edata;
  ea.data = src->data;
  ea.data_len = src->data_len;
  ea.bsum = nullptr;
  ea.bbase = nullptr;
  const uint32_t nblk = (uint32_t)((cap + ENC_THREADS - 1) / ENC_THREADS);
  if (nblk == 0 || (cap <= ENC_SMALL_MAX && !h->no_small)) {
    hipLaunchKernelGGL(k_ence_small, dim3(1), dim3(ENC_SMALL_THREADS), 0, h->stream, ea);
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  if (!h->ence_sum) {  // once, for the largest batch the handle takes
    const uint64_t cm = cap_max >= (1ull << 32) ? (1ull << 32) - 1 : cap_max;
    const uint64_t nb = (cm + ENC_THREADS - 1) / ENC_THREADS + 1;
    if (const int rc = reserve_pair(h->ence_sum, nb, h->ence_base, nb + 1)) return rc;
  }
  ea.bsum = h->ence_sum.get();
  ea.bbase = h->ence_base.get();
  hipLaunchKernelGGL(k_ence_size, dim3(nblk), dim3(ENC_THREADS), 0, h->stream, ea);
  hipLaunchKernelGGL(k_ence_scan, dim3(1), dim3(1024), 0, h->stream, ea, nblk);
  hipLaunchKernelGGL(k_ence_write, dim3(nblk), dim3(ENC_THREADS), 0, h->stream, ea, nblk);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

// ---- per-peer egress -------------------------------------------------------------
int hb_set_egress_peers(hb_handle* h, const uint64_t* ids, uint32_t n) {
  if (!h || n > HB_EGRESS_MAX_PEERS || (n && !ids)) return HB_EINVAL;
  BinTable t;
  if (!bin_build(ids, n, &t)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  if (n == 0) {
    if (!h->bin_table) return HB_OK;
    HB_CHECK(hipStreamSynchronize(h->stream));  // an hb_egress_bin may still read them
    h->bin_table.release();
    h->bin_key.release();
    h->bin_hist.release();
    h->bin_np = 0;
    return HB_OK;
  }
  if (const int rc = h->bin_table.reserve(1)) return rc;
  // on the stream, after the hb_egress_bin calls made so far; `t` lives on this stack
  HB_CHECK(hipMemcpyAsync(h->bin_table.get(), &t, sizeof(BinTable), hipMemcpyHostToDevice, h->stream));
  HB_CHECK(hipStreamSynchronize(h->stream));
  h->bin_np = n;
  return HB_OK;
}

int hb_egress_bin(hb_handle* h, const hb_out_batch* in, uint64_t cap, const uint64_t* n_dev, const hb_out_batch* out,
                  uint32_t* src, uint64_t* bin_off) {
  if (!h || !in || !out || !bin_off) return HB_EINVAL;
  if (!in->group || !in->info || !in->to || !in->term || !in->log_term || !in->index || !in->commit || !in->hint)
    return HB_EINVAL;
  if (!out->group || !out->info || !out->to || !out->term || !out->log_term || !out->index || !out->commit ||
      !out->hint)
    return HB_EINVAL;
  if (out->group == in->group || out->info == in->info || out->to == in->to || out->term == in->term ||
      out->log_term == in->log_term || out->index == in->index || out->commit == in->commit ||
      out->hint == in->hint)
    return HB_EINVAL;
  if (!h->bin_table) return HB_EINVAL;
  // (record numbers, src among them, are 32-bit)
  if (cap > h->max_batch * (h->nmax + 4ull) || cap >= (1ull << 32)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  BinArgs a;
  a.i_group = in->group;
  a.i_info = in->info;
  a.i_to = in->to;
  a.i_term = in->term;
  a.i_log_term = in->log_term;
  a.i_index = in->index;
  a.i_commit = in->commit;
  a.i_hint = in->hint;
  a.o_group = out->group;
  a.o_info = out->info;
  a.o_to = out->to;
  a.o_term = out->term;
  a.o_log_term = out->log_term;
  a.o_index = out->index;
  a.o_commit = out->commit;
  a.o_hint = out->hint;
  a.src = src;
  a.bin_off = dev_view(bin_off);
  a.table = h->bin_table.get();
  a.np = h->bin_np;
  a.cap = (uint32_t)cap;
  a.n_dev = dev_view(n_dev);
  a.key = nullptr;
  a.hist = nullptr;
  a.tot = nullptr;
  a.ntiles = 0;
  if (cap == 0 || (cap <= ENC_SMALL_MAX && !h->no_small)) {
    hipLaunchKernelGGL(k_bin_small, dim3(1), dim3(BIN_THREADS), 0, h->stream, a);
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  if (!h->bin_key) {  // once, for the largest batch the handle takes
    const uint64_t cm = std::min<uint64_t>(h->max_batch * (h->nmax + 4ull), (1ull << 32) - 1);
    const uint64_t nt = (cm + BIN_TILE - 1) / BIN_TILE;
    // (the bins' totals, then their rows)
    if (const int rc = reserve_pair(h->bin_key, cm, h->bin_hist, (nt + 1) * BIN_SLOTS)) return rc;
  }
  a.key = h->bin_key.get();
  a.tot = h->bin_hist.get();
  a.hist = h->bin_hist.get() + BIN_SLOTS;
  a.ntiles = (uint32_t)((cap + BIN_TILE - 1) / BIN_TILE);
  hipLaunchKernelGGL(k_bin_hist, dim3(a.ntiles), dim3(BIN_THREADS), 0, h->stream, a);
  hipLaunchKernelGGL(k_bin_scan, dim3(a.np + 1), dim3(1024), 0, h->stream, a);
  hipLaunchKernelGGL(k_bin_scatter, dim3(a.ntiles), dim3(BIN_THREADS), 0, h->stream, a);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_peer_spans(hb_handle* h, const uint64_t* off, const uint64_t* bin_off, uint64_t* span) {
  if (!h || !off || !bin_off || !span) return HB_EINVAL;
  if (!h->bin_table) return HB_EINVAL;
  DeviceGuard guard(h->device);
  hipLaunchKernelGGL(k_peer_spans, dim3(1), dim3(BIN_SLOTS + 64), 0, h->stream, off, dev_view(bin_off), dev_view(span),
                     h->bin_np);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

// ---- framed peer streams ---------------------------------------------------------
int hb_frame_caps(void) { return HB_FRAME_V1; }
uint64_t hb_frame_size(uint64_t rows) { return rows > FR_MAX_ROWS ? UINT64_MAX : fr_isize(rows); }
uint64_t hb_frame_rows(uint64_t index_len) { return fr_rows(index_len); }

int hb_gid_dir_build(hb_handle* h, const uint64_t* gid, uint32_t count, uint64_t* key, uint32_t* slot, uint64_t cap,
                     uint32_t* dups) {
  if (!h || !key || !slot || !dups || (count && !gid)) return HB_EINVAL;
  if (!gd_cap_ok(cap, count)) return HB_EINVAL;
  DeviceGuard guard(h->device);
  hipStream_t ds = h->in_stream_set ? h->in_stream : h->stream;  // as hb_decode
  if (const int rc = h->gd_ctr.reserve(1)) return rc;
  const uint64_t cb = (cap + FRM_THREADS - 1) / FRM_THREADS, ib = ((uint64_t)count + FRM_THREADS - 1) / FRM_THREADS;
  hipLaunchKernelGGL(k_gid_clear, dim3((unsigned)std::min<uint64_t>(cb, FRM_GRID_MAX)), dim3(FRM_THREADS), 0, ds, key,
                     cap, h->gd_ctr.get());
  hipLaunchKernelGGL(k_gid_insert, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(ib, 1), FRM_GRID_MAX)),
                     dim3(FRM_THREADS), 0, ds, gid, count, key, slot, cap, h->gd_ctr.get());
  hipLaunchKernelGGL(k_count_out, dim3(1), dim3(1), 0, ds, h->gd_ctr.get(), dev_view(dups), (uint64_t*)nullptr);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_frame(hb_handle* h, const hb_out_batch* binned, const uint64_t* off, const uint8_t* status,
             const uint64_t* bin_off, const uint64_t* span, const uint64_t* gid, uint64_t self_id, uint64_t seq,
             uint8_t* index, uint64_t index_cap, uint64_t* ispan, uint32_t* fstat) {
  if (!h || !binned || !off || !status || !bin_off || !span || !gid || !ispan || !fstat) return HB_EINVAL;
  if (!binned->group || !binned->to || (index_cap && !index)) return HB_EINVAL;
  if (reinterpret_cast<uintptr_t>(index) % 8) return HB_EINVAL;  // the columns are stored as words
  if (!h->bin_table) return HB_EINVAL;
  DeviceGuard guard(h->device);
  FrameArgs a;
  a.group = binned->group;
  a.to = binned->to;
  a.off = off;
  a.status = status;
  a.bin_off = dev_view(bin_off);
  a.span = dev_view(span);
  a.gid = gid;
  a.capacity = h->G;
  a.np = h->bin_np;
  a.max_rows = std::min<uint64_t>(h->max_batch * (h->nmax + 4ull), (1ull << 32) - 1);  // hb_egress_bin's bound
  a.self_id = self_id;
  a.seq = seq;
  a.index = index;
  a.index_cap = index_cap;
  a.ispan = dev_view(ispan);
  a.fstat = dev_view(fstat);
  a.cnt = nullptr;
  // the batch's size is bin_off's last word, on the device: the small-step rule goes by the handle's bound
  if (a.max_rows <= ENC_SMALL_MAX && !h->no_small) {
    hipLaunchKernelGGL(k_frame_small, dim3(1), dim3(FRM_THREADS), 0, h->stream, a);
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  if (const int rc = h->frm_cnt.reserve(2 * BIN_SLOTS)) return rc;
  a.cnt = h->frm_cnt.get();
  HB_CHECK(hipMemsetAsync(a.cnt, 0, 2 * BIN_SLOTS * sizeof(uint32_t), h->stream));
  const uint64_t nb = (a.max_rows + FRM_THREADS - 1) / FRM_THREADS;
  hipLaunchKernelGGL(k_frame, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(nb, 1), FRM_GRID_MAX)),
                     dim3(FRM_THREADS), 0, h->stream, a);
  hipLaunchKernelGGL(k_frame_heads, dim3(1), dim3(FRM_THREADS), 0, h->stream, a);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_unframe(hb_handle* h, const uint8_t* index, uint64_t index_size, const hb_frame_in* frames, uint32_t n_frames,
               uint64_t self_id, const hb_gid_dir* dir, uint64_t bytes_size, uint64_t* off, uint32_t* len,
               uint32_t* group, uint64_t n, uint32_t* fstatus, uint64_t* n_unknown) {
  if (!h || !dir || !n_unknown || (n_frames && (!frames || !fstatus))) return HB_EINVAL;
  if (!dir->key || !dir->slot || dir->cap == 0 || (dir->cap & (dir->cap - 1))) return HB_EINVAL;
  if (n && (!index || !off || !len || !group)) return HB_EINVAL;
  if (n_frames > FR_MAX_FRAMES || n > h->max_batch) return HB_EINVAL;
  if (reinterpret_cast<uintptr_t>(index) % 8) return HB_EINVAL;
  uint64_t base[FRM_WORDS];
  uint64_t rows_all = 0;
  for (uint32_t k = 0; k < n_frames; ++k) {
    const hb_frame_in& f = frames[k];
    if (f.index_off % 8) return HB_EINVAL;
    if (f.index_off > index_size || f.index_len > index_size - f.index_off) return HB_EINVAL;
    if (f.bytes_off > bytes_size || f.bytes_len > bytes_size - f.bytes_off) return HB_EINVAL;
    const uint64_t rows = fr_rows(f.index_len);
    if (rows == FR_IMPOSSIBLE) return HB_EINVAL;
    base[k] = rows_all;
    rows_all += rows;  // (at most 256 x 2^32)
  }
  base[n_frames] = rows_all;
  if (rows_all != n) return HB_EINVAL;
  DeviceGuard guard(h->device);
  hipStream_t ds = h->in_stream_set ? h->in_stream : h->stream;  // as hb_decode
  if (!h->unf_ft) {  // once, for the largest batch the handle takes
    const uint64_t nt = (h->max_batch + FRM_THREADS - 1) / FRM_THREADS;
    if (h->unf_pin.reserve(UNF_WORDS) != HB_OK || h->unf_sum.reserve(2 * nt + 1 + FRM_WORDS) != HB_OK ||
        h->unf_st.reserve(FR_MAX_FRAMES + 1) != HB_OK || h->unf_ft.reserve(UNF_WORDS) != HB_OK ||
        (!h->unf_done && hipEventCreateWithFlags(&h->unf_done, hipEventDisableTiming) != hipSuccess)) {
      h->unf_ft.release();
      return HB_ENOMEM;
    }
  }
  HB_CHECK(hipEventSynchronize(h->unf_done));  // the previous call's copy has left the block
  uint64_t* ft = h->unf_pin.get();
  std::memset(ft, 0, UNF_WORDS * sizeof(uint64_t));
  for (uint32_t k = 0; k <= n_frames; ++k) ft[k] = base[k];
  for (uint32_t k = 0; k < n_frames; ++k) {
    ft[UNF_IOFF + k] = frames[k].index_off;
    ft[UNF_BOFF + k] = frames[k].bytes_off;
    ft[UNF_BLEN + k] = frames[k].bytes_len;
    ft[UNF_FROM + k] = frames[k].from;
  }
  HB_CHECK(hipMemcpyAsync(h->unf_ft.get(), ft, UNF_WORDS * sizeof(uint64_t), hipMemcpyHostToDevice, ds));
  HB_CHECK(hipEventRecord(h->unf_done, ds));
  const uint64_t nt_max = (h->max_batch + FRM_THREADS - 1) / FRM_THREADS;
  UnfArgs a;
  a.index = index;
  a.ft = h->unf_ft.get();
  a.nf = n_frames;
  a.n = n;
  a.self_id = self_id;
  a.key = dir->key;
  a.slot = dir->slot;
  a.cap = dir->cap;
  a.off = off;
  a.len = len;
  a.group = group;
  a.fstatus = dev_view(fstatus);
  a.n_unknown = dev_view(n_unknown);
  a.tsum = h->unf_sum.get();
  a.tbase = a.tsum + nt_max;
  a.pbase = a.tbase + nt_max + 1;
  a.fst = h->unf_st.get();
  a.ctr = a.fst + FR_MAX_FRAMES;
  const uint32_t nt = (uint32_t)((n + FRM_THREADS - 1) / FRM_THREADS);
  if (n <= ENC_SMALL_MAX && !h->no_small) {
    hipLaunchKernelGGL(k_unf_small, dim3(1), dim3(FRM_THREADS), 0, ds, a, nt);
    return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
  }
  if (nt) hipLaunchKernelGGL(k_unf_sum, dim3(nt), dim3(FRM_THREADS), 0, ds, a);
  hipLaunchKernelGGL(k_unf_scan, dim3(1), dim3(1024), 0, ds, a, nt);
  if (nt) hipLaunchKernelGGL(k_unf_write, dim3(nt), dim3(FRM_THREADS), 0, ds, a);
  hipLaunchKernelGGL(k_count_out, dim3(1), dim3(1), 0, ds, a.ctr, (uint32_t*)nullptr, a.n_unknown);
  return hipGetLastError() == hipSuccess ? HB_OK : HB_EDEVICE;
}

int hb_event_words_chunks(hb_handle* h, uint32_t* n_chunks, uint32_t* groups_per_chunk) {
  if (!h || !n_chunks) return HB_EINVAL;
  *n_chunks = 2 * h->NB;
  if (groups_per_chunk) *groups_per_chunk = PART;
  return HB_OK;
}

int hb_expand_event_words(const uint64_t* words, uint64_t n_words, const uint32_t* counts, uint32_t n_chunks,
                          hb_event* out, uint64_t cap, uint64_t* n_out) {
  if (!n_out || (n_words && (!words || !counts))) return HB_EINVAL;
  uint64_t k = 0, w = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint64_t end = w + counts[c];
    if (end > n_words) return HB_EINVAL;
    for (; w < end; ++w) {
      const uint64_t x0 = words[w];
      const uint32_t type = (uint32_t)x0 & 0xF;
      if (type == EVC_CONT) continue;
      const uint32_t to = (uint32_t)(x0 >> 4) & 0x7F, aux = (uint32_t)(x0 >> 12) & 0xF;
      const uint32_t group = (c >> 1) * PART + ((uint32_t)(x0 >> 16) & 0xFF);
      uint64_t x = x0 >> 24;
      if (((x0 >> 11) & 1u) && w + 1 < end) x |= (words[w + 1] >> 4) << 40;
      if (type == EVC_BCAST || type == EVC_VBCAST) {
        const uint8_t et = type == EVC_BCAST ? (uint8_t)HB_EV_APP : (uint8_t)HB_EV_VOTE;
        for (uint32_t s = 0; s < 7; ++s)
          if ((to >> s) & 1u) {
            if (out && k < cap) out[k] = hb_event{x, group, et, (uint8_t)s, (uint16_t)aux};
            ++k;
          }
      } else {
        if (out && k < cap) out[k] = hb_event{x, group, (uint8_t)type, (uint8_t)to, (uint16_t)aux};
        ++k;
      }
    }
  }
  *n_out = k;
  return (out && k > cap) ? HB_EINVAL : HB_OK;
}

int hb_stats_device(hb_handle* h, uint64_t** dev_stats) {
  if (!h || !dev_stats) return HB_EINVAL;
  *dev_stats = h->stats;
  return HB_OK;
}

int hb_stats(hb_handle* h, uint64_t* out) {
  if (!h || !out) return HB_EINVAL;
  DeviceGuard guard(h->device);
  HB_CHECK(hipMemcpyAsync(out, h->stats, HB_STAT_COUNT * 8, hipMemcpyDeviceToHost, h->stream));
  HB_CHECK(hipStreamSynchronize(h->stream));
  return HB_OK;
}

int hb_phase_ms(hb_handle* h, float* out, uint32_t* steps) {
  if (!h || !out) return HB_EINVAL;
  DeviceGuard guard(h->device);
  const uint32_t n = std::min<uint32_t>(h->prof_n, hb_handle::PROF_RING);
  if (steps) *steps = n;
  for (int i = 0; i < HB_PHASE_COUNT; ++i) out[i] = 0.f;
  if (n == 0) return HB_EINVAL;
  HB_CHECK(hipStreamSynchronize(h->prep));
  HB_CHECK(hipStreamSynchronize(h->stream));
  // (start, end) event of each phase in h->ph[k]
  static const int span[HB_PHASE_COUNT][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}};
  uint32_t nfull = 0;
  for (uint32_t k = 0; k < n; ++k) nfull += h->prof_full[k] ? 1u : 0u;
  for (uint32_t k = 0; k < n; ++k) {
    for (int i = 0; i < HB_PHASE_COUNT; ++i) {
      if (i != HB_PHASE_APPLY && !h->prof_full[k]) continue;
      float ms = 0.f;
      HB_CHECK(hipEventElapsedTime(&ms, h->ph[k][span[i][0]], h->ph[k][span[i][1]]));
      out[i] += ms / (float)(i == HB_PHASE_APPLY ? n : nfull);
    }
  }
  return HB_OK;
}

int hb_step_kernels(hb_handle* h, uint32_t* mask) {
  if (!h || !mask) return HB_EINVAL;
  *mask = h->kern;
  return HB_OK;
}

int hb_steady_waves(hb_handle* h, uint32_t* n) {
  if (!h || !n) return HB_EINVAL;
  *n = 0;
  if (!h->stepped || !h->steady_count) return HB_OK;
  DeviceGuard guard(h->device);
  HB_CHECK(hipStreamSynchronize(h->stream));
  HB_CHECK(hipMemcpy(n, h->set[h->cur].ctr + CTR_STEADY, 4, hipMemcpyDeviceToHost));
  return HB_OK;
}

int hb_lazy_next_groups(hb_handle* h, uint32_t* n) {
  if (!h || !n) return HB_EINVAL;
  *n = 0;
  DeviceGuard guard(h->device);
  Dev<uint32_t> d;
  if (const int rc = d.reserve(1)) return rc;
  HB_CHECK(hipMemsetAsync(d.get(), 0, 4, h->stream));
  hipLaunchKernelGGL(k_count_lazy_next, dim3((h->G + 255) / 256), dim3(256), 0, h->stream, h->st, d.get());
  HB_CHECK(hipMemcpyAsync(n, d.get(), 4, hipMemcpyDeviceToHost, h->stream));
  HB_CHECK(hipStreamSynchronize(h->stream));
  return HB_OK;
}

int hb_phase_reset(hb_handle* h) {
  if (!h) return HB_EINVAL;
  h->prof_n = 0;
  return HB_OK;
}

int hb_set_stats_accum(hb_handle* h, uint64_t* dev_accum) {
  if (!h) return HB_EINVAL;
  h->stats_accum = dev_accum;
  return HB_OK;
}

int hb_set_input_stream(hb_handle* h, void* stream) {
  if (!h) return HB_EINVAL;
  h->in_stream = reinterpret_cast<hipStream_t>(stream);
  h->in_stream_set = true;
  return HB_OK;
}

int hb_stats_to(hb_handle* h, uint64_t* dev_dst) {
  if (!h || !dev_dst) return HB_EINVAL;
  DeviceGuard guard(h->device);
  HB_CHECK(hipMemcpyAsync(dev_dst, h->stats, HB_STAT_COUNT * 8, hipMemcpyDeviceToDevice, h->stream));
  return HB_OK;
}

int hb_alloc_pinned(size_t bytes, void** out) {
  if (!out) return HB_EINVAL;
  return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? HB_OK : HB_ENOMEM;
}

int hb_free_pinned(void* p) { return hipHostFree(p) == hipSuccess ? HB_OK : HB_EDEVICE; }

}  // extern "C"
