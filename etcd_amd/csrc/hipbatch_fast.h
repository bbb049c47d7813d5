// hipbatch_fast.h — the steady-state leader fast path of the apply phase.
//
// k_apply_fast steps, per group (one lane), exactly the two operations that
// make up steady-state replication (BASELINE.json cfg2):
//
//   * MsgProp on a leader whose own id is in prs
//       stepLeader raft/raft.go:500-513 -> appendEntry :351-360 ->
//       maybeCommit :323-332 -> bcastAppend :303-310
//   * MsgAppResp, Reject = false, from a member whose Progress is Replicate,
//     on a leader, m.Term == 0 or == Term (the Step gate raft/raft.go:462-490
//     passes without a transition)
//       stepLeader raft/raft.go:514-546 (maybeUpdate, freeTo, maybeCommit,
//       bcastAppend / sendAppend)
//
// Every other message (and everything after it for that group) is handed to
// k_apply<NMAX> (the general state machine in hipbatch_kernels.h) through a
// per-group resume word, so the two kernels together step every group's
// messages once, in arrival order.  FastLane is the specialization of
// Lane::step for these preconditions; the parity tests run both paths
// against the oracle.
//
// Why a separate lane type: the general pipeline is ~4k instructions of
// mostly-skipped branches and register-indexed slot access.  Here every slot
// access uses a compile-time slot index (runtime slots become predicated
// unrolled loops), so the hot lane is a few hundred instructions and needs
// few registers.
#pragma once

#include "hipbatch_kernels.h"

namespace hb {

template <int NMAX>
struct FastLane {
  DevState S;
  EvSink E;
  uint32_t g;
  uint32_t arrival;  // batch position of the message; 0xFFFFFFFF: props[] proposal
  uint64_t term, committed, first, last, tfirst, tlast;
  uint32_t mlo;      // meta bits [0, 32): state, n, self, lead, vote, fault
  uint64_t match[NMAX], next[NMAX], head[NMAX];
  uint32_t pm[NMAX];
  uint32_t dirty;
  uint32_t hv;       // bit s: head[s] holds inflights.buffer[start] of slot s (read lazily)
  // n = 7 keeps no head copies: the leader lane's 7 x 3 Progress words plus its
  // 8 route slots otherwise spill (132 B/lane); a head is then read when needed
  static constexpr bool HEADS = NMAX <= 5;
  uint32_t nev;      // public events emitted (an EVC_BCAST word counts once per slot)

  __device__ __forceinline__ uint32_t n() const { return (mlo >> 2) & 7; }
  __device__ __forceinline__ uint32_t state() const { return mlo & 3; }
  __device__ __forceinline__ uint32_t self() const { return (mlo >> 5) & 0xF; }
  __device__ __forceinline__ uint32_t faulted() const { return (mlo >> 17) & 0xF; }
  __device__ __forceinline__ uint64_t arrival_x() const {
    return arrival == 0xFFFFFFFFu ? HB_NO_INDEX : (uint64_t)arrival;
  }
  __device__ __forceinline__ void ev(uint32_t type, uint32_t to, uint32_t aux, uint64_t x) {
    emit_ev(E, g & (PART - 1), type, to, aux, x);
    nev++;
  }
  __device__ __forceinline__ void fault(uint32_t code) {
    if (faulted()) return;
    mlo = (mlo & ~(0xFu << 17)) | (code << 17);
    dirty |= D_META;
  }
  __device__ __forceinline__ uint64_t* ring_at(uint32_t s, uint32_t idx) const {
    return S.ring + ((size_t)s * S.W + idx) * S.G + g;
  }

  // All state loads of the lane are independent, so they are in flight together.
  __device__ __forceinline__ void load() {
    load_head();
    load_rest();
  }
  // The loads that depend on nothing the lane reads (k_apply_fast issues them
  // with meta itself, in its first round trip) ...
  __device__ __forceinline__ void load_head() {
    load_state_head();
    load_pm();
  }
  // (the per-group fields, which every role steps with, and the packed
  // Progress states, which only a leader reads)
  __device__ __forceinline__ void load_state_head() {
    term = at32(S.term, g);
    committed = at32(S.commit, g);
    first = at32(S.first, g);
    last = at32(S.last, g);
    tfirst = at32(S.tfirst, g);
  }
  __device__ __forceinline__ void load_pm() {
#pragma unroll
    for (int s = 0; s < NMAX; ++s) pm[s] = at32(S.pm, s * S.G + g);
  }
  // ... and those that wait for meta (which arrays are kept) and pm (the ring
  // heads): the second round trip.
  __device__ __forceinline__ void load_rest() {
    // arrays the meta flags mark as not kept are not read (M_TL / M_SM / M_NX,
    // hipbatch_kernels.h); these loads issue once meta is in, beside the
    // ring heads, which wait for pm anyway
    tlast = (mlo & (uint32_t)M_TL) ? last : at32(S.tlast, g);
    const uint32_t sf = (mlo & (uint32_t)M_SM) ? self() : 0xFFu;
    const bool nxl = NMAX <= 3 && (mlo & (uint32_t)M_NX) != 0;  // (slots >= n are never read)
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      match[s] = ((uint32_t)s == sf) ? last : at32(S.match, s * S.G + g);
      next[s] = ((uint32_t)s == sf || nxl) ? last + 1 : at32(S.next, s * S.G + g);
    }
    if (mlo & (uint32_t)M_RS) {  // a group k_elect left in the reset form: every slot written back
      const uint32_t nn = n();
#pragma unroll
      for (int s = 0; s < NMAX; ++s) {
        if ((uint32_t)s < nn) {
          uint64_t mt, nx;
          uint32_t p;
          rs_progress(mlo, (uint32_t)s, last, tfirst, &mt, &nx, &p);
          match[s] = mt;
          next[s] = nx;
          pm[s] = p;
        }
      }
    }
    // The ring heads are loaded with the state (one more round trip, beside
    // nothing else); free_to reads one lazily if a lane has none.  (Loading
    // them only on demand — an ack at or past Next - 1 frees the whole window
    // unread — measured 1-3 % slower on cfg2 / cfg3 / cfg5.)
#pragma unroll
    for (int s = 0; s < NMAX; ++s) head[s] = (HEADS && pm_count(pm[s])) ? *ring_at(s, pm_start(pm[s])) : 0;
    hv = HEADS ? (1u << NMAX) - 1 : 0u;
    dirty = 0;
    if (mlo & (uint32_t)M_RS) {
      mlo &= ~(uint32_t)M_RS;
      dirty |= D_META;
#pragma unroll
      for (int s = 0; s < NMAX; ++s)
        if ((uint32_t)s < n()) dirty |= (1u << (D_SLOT0 + s)) | (1u << (D_PM0 + s));
    }
  }
  // Dirty bits (hipbatch_kernels.h) plus, lane-local to the fast path:
  // D_TFIRST (tfirst alone; D_TRUN then means tlast) and per-slot D_PM0 + s
  // (pm alone; D_SLOT0 + s then means match / next).
  static constexpr uint32_t D_TFIRST = 1u << 5;
  static constexpr uint32_t D_PM0 = 16;
  __device__ __forceinline__ void store() {
    // keep M_TL / M_SM only while they still hold; a cleared flag makes its
    // array live again, so it is written
    const bool tl = (mlo & (uint32_t)M_TL) && tlast == last;
    if ((mlo & (uint32_t)M_TL) && !tl) {
      mlo &= ~(uint32_t)M_TL;
      dirty |= D_META | D_TRUN;
    }
    uint32_t sf = 0xFFu;
    if (mlo & (uint32_t)M_SM) {
      const uint32_t s0 = self();
      bool ok = false;
#pragma unroll
      for (int s = 0; s < NMAX; ++s)
        if ((uint32_t)s == s0) ok = match[s] == last && next[s] == last + 1;
      if (ok) {
        sf = s0;
      } else {
        mlo &= ~(uint32_t)M_SM;
        dirty |= D_META | (1u << (D_SLOT0 + s0));
      }
    }
    // M_NX is derived again (the lane is a Leader past the M_RS form, and stays
    // one): set while every slot's Next == last + 1, and the next array is then
    // not written; a flag that falls makes the array live, so every slot's is
    bool nx = false;
    if constexpr (NMAX <= 3) {
      const uint32_t nn = n();
      nx = S.lazy_next != 0 && state() == HB_STATE_LEADER && nn != 0;
#pragma unroll
      for (int s = 0; s < NMAX; ++s)
        if ((uint32_t)s < nn) nx = nx && next[s] == last + 1;
      if (nx != ((mlo & (uint32_t)M_NX) != 0)) {
        if (!nx) {
#pragma unroll
          for (int s = 0; s < NMAX; ++s)
            if ((uint32_t)s < nn) dirty |= 1u << (D_SLOT0 + s);
        }
        mlo ^= (uint32_t)M_NX;
        dirty |= D_META;
      }
    }
    if (dirty & D_META) at32(reinterpret_cast<uint32_t*>(S.meta), 2 * g) = mlo;  // little-endian low word
    if (dirty & D_COMMIT) at32(S.commit, g) = committed;
    if (dirty & D_LAST) at32(S.last, g) = last;
    if (dirty & D_TFIRST) at32(S.tfirst, g) = tfirst;
    if ((dirty & D_TRUN) && !tl) at32(S.tlast, g) = tlast;
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      if ((dirty & (1u << (D_SLOT0 + s))) && (uint32_t)s != sf) {
        at32(S.match, s * S.G + g) = match[s];
        if (!nx) at32(S.next, s * S.G + g) = next[s];
      }
      if (dirty & (1u << (D_PM0 + s))) at32(S.pm, s * S.G + g) = pm[s];
    }
  }
  __device__ __forceinline__ void set_pm(int s, uint32_t v) {
    if (v != pm[s]) dirty |= 1u << (D_PM0 + s);
    pm[s] = v;
  }

  // isPaused raft/progress.go:147-158
  __device__ __forceinline__ bool is_paused(uint32_t p) const {
    const uint32_t st = pm_state(p);
    if (st == HB_PR_PROBE) return pm_paused(p) != 0;
    if (st == HB_PR_REPLICATE) return pm_count(p) == S.W;
    return true;
  }
  // inflights.freeTo raft/progress.go:204-224 (s is a compile-time constant
  // after the callers' unrolled slot loops).  nx0 = Next before the ack: in
  // Replicate every entry is below Next (inflights.add of the last index sent,
  // then Next = that + 1, raft/raft.go:270-273; Next only grows until the
  // window is reset), so to >= nx0 - 1 pops the whole window without reading
  // it; otherwise the head entry comes from the register copy, read once.
  __device__ __forceinline__ void free_to(int s, uint64_t to, uint64_t nx0) {
    const uint32_t p = pm[s];
    const uint32_t cnt = pm_count(p);
    if (cnt == 0) return;
    uint32_t idx = pm_start(p);
    const uint32_t W = S.W;
    if (nx0 != 0 && to >= nx0 - 1) {
      idx += cnt;
      if (idx >= W) idx -= W;
      set_pm(s, pm_make(pm_state(p), pm_paused(p), idx, 0));
      return;
    }
    if (!((hv >> s) & 1u)) {
      head[s] = *ring_at(s, idx);
      hv |= 1u << s;
    }
    uint64_t v = head[s];
    if (to < v) return;
    uint32_t i = 0;
    while (true) {
      ++i;
      if (++idx >= W) idx -= W;
      if (i == cnt) break;
      v = *ring_at(s, idx);
      if (to < v) break;
    }
    set_pm(s, pm_make(pm_state(p), pm_paused(p), idx, cnt - i));
    head[s] = v;
  }
  // an HB_EV_APP's aux: the entry at x (the MsgApp's Index) has the current Term
  // (m.LogTerm == m.Term), so the host need not look it up
  __device__ __forceinline__ uint32_t lt_cur(uint64_t x) const { return (tfirst <= x && x <= tlast) ? 1u : 0u; }
  // raftLog.term(i) == Term over the current-term run (raft/log.go:198-217)
  __device__ __forceinline__ bool term_eq(uint64_t i) const {
    if (i + 1 < first || i > last) return term == 0;
    return tfirst <= i && i <= tlast;
  }
  // maybeCommit raft/raft.go:323-332 + raftLog.maybeCommit raft/log.go:241-247 +
  // commitTo :172-180.  The q-th largest Match by an odd-even transposition
  // network over the NMAX registers (absent slots read as 0).
  __device__ __forceinline__ bool maybe_commit() {
    uint64_t v[NMAX];
    const uint32_t nn = n();
#pragma unroll
    for (int s = 0; s < NMAX; ++s) v[s] = ((uint32_t)s < nn) ? match[s] : 0;
#pragma unroll
    for (int r = 0; r < NMAX; ++r) {
#pragma unroll
      for (int j = (r & 1); j + 1 < NMAX; j += 2) {
        const uint64_t a = v[j], b = v[j + 1];
        v[j] = a > b ? a : b;
        v[j + 1] = a > b ? b : a;
      }
    }
    uint64_t mci = v[0];
#pragma unroll
    for (int s = 1; s < NMAX; ++s) mci = ((uint32_t)s == nn / 2) ? v[s] : mci;  // q-1, q = n/2+1
    if (mci > committed && term_eq(mci)) {
      if (last < mci) {
        fault(HB_FAULT_COMMIT_RANGE);
        return false;
      }
      committed = mci;
      dirty |= D_COMMIT;
      ev(HB_EV_COMMIT, 0, 0, mci);
      return true;
    }
    return false;
  }
  // sendAppend raft/raft.go:239-282 to slot s: the progress side effects;
  // returns the message it sends (SEND_NONE / SEND_APP / SEND_SNAP, index *x)
  // for the caller to emit.
  enum : uint32_t { SEND_NONE = 0, SEND_APP = 1, SEND_SNAP = 2 };
  __device__ __forceinline__ uint32_t send_decide(int s, uint64_t* xo) {
    const uint32_t p = pm[s];
    if (is_paused(p)) return SEND_NONE;
    if (next[s] < first) {  // needSnapshot raft/raft.go:715-717
      const uint64_t snapi = S.snap[g];
      if (snapi == 0) {
        fault(HB_FAULT_EMPTY_SNAPSHOT);
        return SEND_NONE;
      }
      set_pm(s, pm_make(HB_PR_SNAPSHOT, 0, 0, 0));  // becomeSnapshot
      S.pending[(size_t)s * S.G + g] = snapi;
      *xo = snapi;
      return SEND_SNAP;
    }
    const uint64_t x = next[s] - 1;
    if (next[s] <= last) {
      bool ok = true;
      const uint64_t lastsent = sz_limit(S, g, next[s], last, &ok);
      if (!ok) {
        fault(HB_FAULT_SIZE_WINDOW);
        return SEND_NONE;
      }
      const uint32_t st = pm_state(p);
      if (st == HB_PR_REPLICATE) {
        const uint32_t cnt = pm_count(p), start = pm_start(p);
        if (cnt == S.W) {
          fault(HB_FAULT_INFLIGHTS_FULL);
          return SEND_NONE;
        }
        uint32_t idx = start + cnt;
        if (idx >= S.W) idx -= S.W;
        *ring_at(s, idx) = lastsent;              // inflights.add
        if (cnt == 0) {
          head[s] = lastsent;
          hv |= 1u << s;
        }
        next[s] = lastsent + 1;                   // optimisticUpdate
        dirty |= 1u << (D_SLOT0 + s);
        set_pm(s, pm_make(HB_PR_REPLICATE, pm_paused(p), start, cnt + 1));
      } else if (st == HB_PR_PROBE) {
        set_pm(s, p | PM_PAUSED);                 // pause
      }
    }
    *xo = x;
    return SEND_APP;
  }
  __device__ __forceinline__ void send_append(int s) {
    uint64_t x = 0;
    const uint32_t k = send_decide(s, &x);
    if (k != SEND_NONE) ev(k == SEND_APP ? HB_EV_APP : HB_EV_SNAP, s, k == SEND_APP ? lt_cur(x) : 0u, x);
  }
  // bcastAppend raft/raft.go:303-310 (slot order, self skipped).  When every
  // message it sends is a MsgApp with the same Index (steady state), the sends
  // are recorded as one EVC_BCAST word; otherwise one event per send, in slot
  // order.  Nothing else is emitted between the sends, so the order holds.
  __device__ __forceinline__ void bcast_append() {
    const uint32_t nn = n(), sf = self();
    uint32_t kind[NMAX];
    uint64_t xs[NMAX];
    uint32_t mask = 0;
    uint64_t x0 = 0;
    bool same = true;
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      kind[s] = SEND_NONE;
      xs[s] = 0;
      if ((uint32_t)s < nn && (uint32_t)s != sf && !faulted()) kind[s] = send_decide(s, &xs[s]);
      if (kind[s] != SEND_NONE) {
        if (mask == 0) x0 = xs[s];
        same = same && kind[s] == SEND_APP && xs[s] == x0;
        mask |= 1u << s;
      }
    }
    if (mask == 0) return;
    if (same && (mask & (mask - 1))) {
      emit_ev(E, g & (PART - 1), EVC_BCAST, mask, lt_cur(x0), x0);
      nev += __popc(mask);
      return;
    }
#pragma unroll
    for (int s = 0; s < NMAX; ++s)
      if (kind[s] != SEND_NONE)
        ev(kind[s] == SEND_APP ? HB_EV_APP : HB_EV_SNAP, s, kind[s] == SEND_APP ? lt_cur(xs[s]) : 0u, xs[s]);
  }

  // ---- preconditions (checked per message by the kernel)
  __device__ __forceinline__ bool prop_ok(uint32_t k) const {
    return k != 0 && state() == HB_STATE_LEADER && self() != HB_SLOT_NONE;
  }
  __device__ __forceinline__ bool accept_ok(uint32_t type, uint32_t from, uint64_t mterm, bool reject) const {
    bool rep = false;
#pragma unroll
    for (int s = 0; s < NMAX; ++s) rep = ((uint32_t)s == from) ? (pm_state(pm[s]) == HB_PR_REPLICATE) : rep;
    return type == HB_MSG_APP_RESP && !reject && state() == HB_STATE_LEADER && (mterm == 0 || mterm == term) &&
           from < n() && rep;
  }

  // ---- MsgProp with k entries on a leader (prop_ok)
  __device__ __forceinline__ void prop(uint32_t k) {
    const uint64_t old = last;
    if (sz_on(S.max_msg_size))  // the entries' descriptors: the dense proposal's, or the MsgProp message's
      sz_append(S, g, old, k, term, S.edesc + (arrival == 0xFFFFFFFFu ? S.peoff[g] : S.eoff[arrival]));
    last += k;
    if (tfirst == HB_NO_INDEX) {
      tfirst = old + 1;
      dirty |= D_TFIRST;
    }
    tlast = last;
    dirty |= D_LAST | D_TRUN;
    ev(HB_EV_LAST, 0, 0, last);
    const uint32_t sf = self();
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      if ((uint32_t)s == sf) {  // self maybeUpdate(lastIndex) raft/raft.go:358
        if (match[s] < last) {
          match[s] = last;
          set_pm(s, pm[s] & ~PM_PAUSED);
        }
        if (next[s] < last + 1) next[s] = last + 1;
        dirty |= 1u << (D_SLOT0 + s);
      }
    }
    maybe_commit();
    bcast_append();
    if (faulted()) ev(HB_EV_FAULT, 0, faulted(), arrival_x());
  }

  // ---- accepted MsgAppResp from a Replicate member (accept_ok)
  __device__ __forceinline__ void accept(uint32_t from, uint64_t index) {
    bool updated = false, old_paused = false;
#pragma unroll
    for (int s = 0; s < NMAX; ++s) {
      if ((uint32_t)s == from) {
        old_paused = pm_count(pm[s]) == S.W;      // isPaused() in Replicate, before maybeUpdate
        const uint64_t nx0 = next[s];
        if (next[s] < index + 1) next[s] = index + 1;
        if (match[s] < index) {                   // maybeUpdate raft/progress.go:102-113
          match[s] = index;
          set_pm(s, pm[s] & ~PM_PAUSED);
          updated = true;
          free_to(s, index, nx0);                 // Replicate: ins.freeTo(m.Index)
        }
        dirty |= 1u << (D_SLOT0 + s);
      }
    }
    if (!updated) return;
    if (maybe_commit()) {
      bcast_append();
    } else if (old_paused && !faulted()) {
#pragma unroll
      for (int s = 0; s < NMAX; ++s)
        if ((uint32_t)s == from) send_append(s);
    }
    if (faulted()) ev(HB_EV_FAULT, 0, faulted(), arrival_x());
  }
};

// ---------------------------------------------------------------------------
// SteadyLane: FastLane<3>::prop + accept + maybe_commit + bcast_append + store
// for a leader in steady replication, as straight-line code.
// fast_step runs it for a whole wave when every lane of the wave is steady or
// has nothing to step; otherwise the wave runs the general FastLane body.
//
// plan() steps a copy of the lane's state in registers and clears `ok` at the
// first thing the specialisation does not cover; nothing is written until
// the wave has voted, so a lane that turns out not to be steady costs nothing
// but the vote.  A lane is steady when all of these hold:
//   * it is a loaded leader (`lead`: live, not M_NC, cnt <= 2 or a proposal)
//     with n == 3, self < 3, M_RS clear, no size limit (max_msg_size =
//     HB_NO_LIMIT: a MsgApp carries every entry up to last), cnt <= 2;
//   * both followers (the two slots that are not self) are Replicate;
//   * every message passes accept_ok (MsgAppResp, not a reject, Term 0 or the
//     group's) and comes from a follower, two messages from different ones;
//   * each ack advances Match and stays inside the log (match < index <=
//     last) and covers everything sent (Next != 0, index >= Next - 1: free_to
//     pops the whole window without a ring read);
//   * no window is full whenever isPaused is asked (each bcastAppend, each
//     ack), and no follower needs a snapshot (Next >= first);
//   * a bcastAppend sends both followers the same Index (one EVC_BCAST word)
//     and leaves both at Next = last + 1, so a later one of the step sends
//     Index = last and appends nothing to a window;
//   * maybeCommit advances at most once in the step, inside the log;
//   * every event's x is below 2^40 (one word per event).
// The events of such a step are then named by a few values (last, committed,
// the first bcastAppend's Index) and a mask of which are present, so the lane
// carries no event words through the vote.  With self known the followers are
// two values (a < b, slot order), so there is no runtime slot index, no
// per-message loop, no head copy and no fault, drop or hand-over test.  The
// events are the words FastLane emits, in the same order per group; commit()
// writes what FastLane::store would.
// ---------------------------------------------------------------------------
struct SteadyFol {
  uint64_t match, next;
  uint32_t pm;
};

struct SteadyLane {
  // event words: P chunk 0 LAST, 1 COMMIT, 2 EVC_BCAST; M chunk, message t:
  // 3 + 2t COMMIT, 4 + 2t EVC_BCAST
  static constexpr uint32_t EW_P = 3, EW = 7;
  static constexpr uint32_t EVM_BCAST = 0x54, EVM_COMMIT = 0x2A;
  uint64_t last, committed, tfirst, tlast;
  uint64_t smatch, snext;  // the self slot
  uint32_t spm;
  SteadyFol fa, fb;        // the other two slots, slot order
  uint32_t spm0, pa0, pb0;  // the three pm words as loaded
  uint32_t sf, sa, sb;
  uint32_t evm;            // bit j: event word j is emitted
  uint32_t ltm;            // bit j (an EVC_BCAST word): its aux, lt_cur of its Index
  uint32_t jfirst;         // the word of the step's first bcastAppend (0: none yet)
  uint64_t xfirst;         // its Index (a later one sends last)
  uint32_t ring_a, ring_b;  // inflights.add's ring position (valid with add_a / add_b)
  bool add_a, add_b, touch_a, touch_b;  // touch: match / next are written (the slot's dirty bit)
  bool prop, d_tfirst;
  bool ok;

  __device__ __forceinline__ uint32_t lt_cur(uint64_t x) const { return (tfirst <= x && x <= tlast) ? 1u : 0u; }

  // send_decide to a Replicate follower; returns the MsgApp's Index
  __device__ __forceinline__ uint64_t send(SteadyFol& f, uint32_t& ring, bool& add, bool& touch, uint32_t W,
                                           uint64_t first) {
    const uint32_t c = pm_count(f.pm);
    ok = ok && c != W && f.next >= first;
    const uint64_t x = f.next - 1;
    if (f.next <= last) {
      uint32_t idx = pm_start(f.pm) + c;
      if (idx >= W) idx -= W;
      ring = idx;  // inflights.add(last)
      add = true;
      f.next = last + 1;  // optimisticUpdate
      touch = true;
      f.pm = pm_make(HB_PR_REPLICATE, pm_paused(f.pm), pm_start(f.pm), c + 1);
    }
    ok = ok && f.next == last + 1;
    return x;
  }
  // bcast_append: both followers are sent to, the same Index; word j
  __device__ __forceinline__ void bcast(uint32_t W, uint64_t first, uint32_t j) {
    const uint64_t xa = send(fa, ring_a, add_a, touch_a, W, first);
    const uint64_t xb = send(fb, ring_b, add_b, touch_b, W, first);
    ok = ok && xa == xb;
    if (jfirst == 0) {
      jfirst = j;
      xfirst = xa;
    }  // (else xa == last: both were left at Next = last + 1, and an ack inside the log keeps that)
    evm |= 1u << j;
    ltm |= lt_cur(xa) << j;
  }
  // maybe_commit over {self, a, b}: the median is the quorum's Match; word j
  __device__ __forceinline__ bool maybe_commit(uint64_t term, uint64_t first, uint32_t j) {
    const uint64_t mx = umax64(smatch, fa.match), mn = umin64(smatch, fa.match);
    const uint64_t mci = umax64(mn, umin64(mx, fb.match));
    const bool teq = (mci + 1 < first || mci > last) ? term == 0 : (tfirst <= mci && mci <= tlast);
    const bool up = mci > committed && teq;
    ok = ok && !(up && (last < mci || (evm & EVM_COMMIT) != 0));
    if (up) {
      committed = mci;
      evm |= 1u << j;
    }
    return up;
  }
  // accept (after accept_ok) of message t
  __device__ __forceinline__ void ack(uint32_t info, uint64_t mterm, uint64_t index, uint64_t term, uint32_t W,
                                      uint64_t first, uint32_t t) {
    const uint32_t type = info & 0xF, from = (info >> 4) & 0xF;
    const bool reject = (info >> 8) & 1u;
    ok = ok && type == HB_MSG_APP_RESP && !reject && (mterm == 0 || mterm == term) && (from == sa || from == sb);
    const bool isa = from == sa;
    const uint64_t am = fa.match, an = fa.next, bm = fb.match, bn = fb.next;
    const uint32_t ap = fa.pm, bp = fb.pm;
    const uint64_t m0 = isa ? am : bm, nx0 = isa ? an : bn;
    const uint32_t p0 = isa ? ap : bp;
    const uint32_t c = pm_count(p0);
    ok = ok && c != W && m0 < index && index <= last && nx0 != 0 && index >= nx0 - 1;
    const uint64_t nx = umax64(nx0, index + 1);
    uint32_t idx = pm_start(p0) + c;  // freeTo: the whole window
    if (c != 0 && idx >= W) idx -= W;
    const uint32_t p = pm_make(HB_PR_REPLICATE, 0, idx, 0);
    fa.match = isa ? index : am;  // maybeUpdate
    fa.next = isa ? nx : an;
    fa.pm = isa ? p : ap;
    touch_a = touch_a || isa;
    fb.match = isa ? bm : index;
    fb.next = isa ? bn : nx;
    fb.pm = isa ? bp : p;
    touch_b = touch_b || !isa;
    // the window this ack leaves is empty, so an inflights.add made earlier in
    // the step for this follower lies outside it: nothing reads that ring word
    // (only [start, start + count) is ever read), and it is not stored.  A later
    // send of the step sets add / ring afresh.
    add_a = add_a && !isa;
    add_b = add_b && isa;
    if (maybe_commit(term, first, EW_P + 2 * t)) bcast(W, first, EW_P + 2 * t + 1);
  }

  // Steps the lane's proposal and its (at most two) messages on a copy of L
  // (a FastLane<3>, or the lean SteadyIn below).
  template <class LT>
  __device__ __forceinline__ void plan(const LT& L, uint32_t prop_k, uint32_t cnt,
                                       const uint32_t (&s_info)[2], const uint32_t (&s_orig)[2],
                                       const uint64_t (&s_term)[2], const uint64_t (&s_index)[2]) {
    const uint32_t W = L.S.W;
    last = L.last;
    committed = L.committed;
    tfirst = L.tfirst;
    tlast = L.tlast;
    sf = L.self();
    sa = sf == 0 ? 1u : 0u;
    sb = sf == 2 ? 1u : 2u;
    // (selects on values: a conditional on the array elements themselves is a
    // runtime address, and the lane's registers become scratch)
    const uint64_t m0 = L.match[0], m1 = L.match[1], m2 = L.match[2];
    const uint64_t n0 = L.next[0], n1 = L.next[1], n2 = L.next[2];
    const uint32_t p0 = L.pm[0], p1 = L.pm[1], p2 = L.pm[2];
    smatch = sf == 0 ? m0 : (sf == 1 ? m1 : m2);
    snext = sf == 0 ? n0 : (sf == 1 ? n1 : n2);
    spm = spm0 = sf == 0 ? p0 : (sf == 1 ? p1 : p2);
    fa.match = sf == 0 ? m1 : m0;
    fa.next = sf == 0 ? n1 : n0;
    fa.pm = pa0 = sf == 0 ? p1 : p0;
    fb.match = sf == 2 ? m1 : m2;
    fb.next = sf == 2 ? n1 : n2;
    fb.pm = pb0 = sf == 2 ? p1 : p2;
    add_a = add_b = touch_a = touch_b = false;
    ring_a = ring_b = 0;
    evm = ltm = jfirst = 0;
    xfirst = 0;
    prop = d_tfirst = false;
    ok = L.n() == 3 && sf < 3 && !(L.mlo & (uint32_t)M_RS) && L.S.max_msg_size == HB_NO_LIMIT && cnt <= 2 &&
         pm_state(fa.pm) == HB_PR_REPLICATE && pm_state(fb.pm) == HB_PR_REPLICATE;
    if (prop_k) {  // FastLane::prop
      prop = true;
      const uint64_t old = last;
      last += prop_k;
      if (tfirst == HB_NO_INDEX) {
        tfirst = old + 1;
        d_tfirst = true;
      }
      tlast = last;
      evm |= 1u;
      if (smatch < last) {
        smatch = last;
        spm &= ~PM_PAUSED;
      }
      if (snext < last + 1) snext = last + 1;
      maybe_commit(L.term, L.first, 1);
      bcast(W, L.first, 2);
    }
    // arrival order
    const uint32_t ia = s_info[0], ib = s_info[1], oa = s_orig[0], ob = s_orig[1];
    const uint64_t ta = s_term[0], tb = s_term[1], xa = s_index[0], xb = s_index[1];
    const bool sw = cnt == 2 && ob < oa;
    const uint32_t i0 = sw ? ib : ia, i1 = sw ? ia : ib;
    const uint64_t t0 = sw ? tb : ta, t1 = sw ? ta : tb;
    const uint64_t x0 = sw ? xb : xa, x1 = sw ? xa : xb;
    if (cnt == 2) ok = ok && ((i0 ^ i1) & 0xF0u) != 0;  // two followers
    if (cnt >= 1) ack(i0, t0, x0, L.term, W, L.first, 0);
    if (cnt >= 2) ack(i1, t1, x1, L.term, W, L.first, 1);
    ok = ok && ((last | xfirst) >> 40) == 0;  // (committed <= last)
  }
  // public events (an EVC_BCAST word counts once per follower)
  __device__ __forceinline__ uint32_t nev() const { return __popc(evm) + __popc(evm & EVM_BCAST); }
  // event word j (bit j of evm)
  __device__ __forceinline__ uint64_t word(uint32_t j, uint32_t lane) const {
    if (j == 0) return evc_word(HB_EV_LAST, 0, 0, lane, last, false);
    if ((EVM_COMMIT >> j) & 1u) return evc_word(HB_EV_COMMIT, 0, 0, lane, committed, false);
    return evc_word(EVC_BCAST, (1u << sa) | (1u << sb), (ltm >> j) & 1u, lane, j == jfirst ? xfirst : last, false);
  }

  // FastLane::store for what plan() changed.  M_TL and M_SM, where set, still
  // hold, so their arrays stay unwritten and those bits never change.  M_NX is
  // derived as FastLane::store does (a steady step nearly always ends with
  // every Next at last + 1): while it holds no Next is written; the one meta
  // store is for a group that gains it (or, a follower left behind without a
  // bcastAppend, loses it: then all three Next words are written).
  template <class LT>
  __device__ __forceinline__ void commit(const LT& L) const {
    const DevState& S = L.S;
    const uint32_t g = L.g;
    const bool nx0 = (L.mlo & (uint32_t)M_NX) != 0;
    const bool nx = S.lazy_next != 0 && snext == last + 1 && fa.next == last + 1 && fb.next == last + 1;
    const bool all = nx0 && !nx;  // the next array is live again
    if (nx != nx0) at32(reinterpret_cast<uint32_t*>(S.meta), 2 * g) = L.mlo ^ (uint32_t)M_NX;
    if (committed != L.committed) at32(S.commit, g) = committed;
    if (prop) {
      at32(S.last, g) = last;
      if (d_tfirst) at32(S.tfirst, g) = tfirst;
      if (!(L.mlo & (uint32_t)M_TL)) at32(S.tlast, g) = tlast;
      if (!(L.mlo & (uint32_t)M_SM)) at32(S.match, sf * S.G + g) = smatch;
    }
    if (!(L.mlo & (uint32_t)M_SM) && !nx && (prop || all)) at32(S.next, sf * S.G + g) = snext;
    if (spm != spm0) at32(S.pm, sf * S.G + g) = spm;
    if (touch_a) at32(S.match, sa * S.G + g) = fa.match;
    if (!nx && (touch_a || all)) at32(S.next, sa * S.G + g) = fa.next;
    if (fa.pm != pa0) at32(S.pm, sa * S.G + g) = fa.pm;
    if (add_a) *L.ring_at(sa, ring_a) = last;
    if (touch_b) at32(S.match, sb * S.G + g) = fb.match;
    if (!nx && (touch_b || all)) at32(S.next, sb * S.G + g) = fb.next;
    if (fb.pm != pb0) at32(S.pm, sb * S.G + g) = fb.pm;
    if (add_b) *L.ring_at(sb, ring_b) = last;
  }
};

// ---------------------------------------------------------------------------
// The steady step's own view of a group (k_route_fast's pass 1):
// only what SteadyLane::plan and commit read, so a loop over it carries none
// of FastLane's heads, dirty bits, arrival or event sink.
//
// SteadyHead is the first round trip (what depends on nothing the lane reads):
// 15 registers, loaded one group ahead.  The loads sit in straight-line code:
// a lane without a valid group reads group 0's words (inside every array) and
// drops them.  An exec-masked block would be a join in the control flow, and
// at a join the wait-count pass assumes the shorter path, so the wait for the
// current group's second round would become a wait for these loads too.  For
// the same reason an absent props array is read as pm.
// ---------------------------------------------------------------------------
struct SteadyHead {
  uint32_t mlo, props;
  uint64_t term, committed, first, last, tfirst;
  uint32_t pm[3];

  __device__ __forceinline__ void load(const DevState& S, const uint32_t* props_in, uint32_t g, bool valid) {
    const uint32_t gl = valid ? g : 0u;
    const uint32_t* pr = props_in ? props_in : S.pm;  // (uniform select, no branch)
    const uint32_t m = at32(reinterpret_cast<const uint32_t*>(S.meta), 2 * gl);  // little-endian low word
    const uint32_t k = at32(pr, gl);
    const uint64_t t = at32(S.term, gl), c = at32(S.commit, gl), f = at32(S.first, gl), l = at32(S.last, gl),
                   tf = at32(S.tfirst, gl);
    uint32_t p[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) p[s] = at32(S.pm, s * S.G + gl);
    mlo = valid ? m : 0u;
    props = (valid && props_in) ? k : 0u;
    term = valid ? t : 0ull;
    committed = valid ? c : 0ull;
    first = valid ? f : 0ull;
    last = valid ? l : 0ull;
    tfirst = valid ? tf : 0ull;
#pragma unroll
    for (int s = 0; s < 3; ++s) pm[s] = valid ? p[s] : 0u;
  }
};

struct SteadyIn {
  const DevState& S;
  uint32_t g;
  uint32_t mlo;
  uint64_t term, committed, first, last, tfirst, tlast;
  uint64_t match[3], next[3];
  uint32_t pm[3];

  __device__ __forceinline__ SteadyIn(const DevState& S_, uint32_t g_, const SteadyHead& H)
      : S(S_), g(g_), mlo(H.mlo), term(H.term), committed(H.committed), first(H.first), last(H.last),
        tfirst(H.tfirst), tlast(0), match{0, 0, 0}, next{0, 0, 0}, pm{H.pm[0], H.pm[1], H.pm[2]} {}
  __device__ __forceinline__ uint32_t n() const { return (mlo >> 2) & 7; }
  __device__ __forceinline__ uint32_t state() const { return mlo & 3; }
  __device__ __forceinline__ uint32_t self() const { return (mlo >> 5) & 0xF; }
  __device__ __forceinline__ uint32_t faulted() const { return (mlo >> 17) & 0xF; }
  __device__ __forceinline__ uint64_t* ring_at(uint32_t s, uint32_t idx) const {
    return S.ring + ((size_t)s * S.W + idx) * S.G + g;
  }
  // The second round trip: FastLane<3>::load_rest without the M_RS form (plan
  // turns such a group down before it reads a Progress word) and without the
  // ring heads (a steady ack frees its whole window unread).
  __device__ __forceinline__ void load_rest() {
    tlast = (mlo & (uint32_t)M_TL) ? last : at32(S.tlast, g);
    const uint32_t sf = (mlo & (uint32_t)M_SM) ? self() : 0xFFu;
    const bool nxl = (mlo & (uint32_t)M_NX) != 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      match[s] = ((uint32_t)s == sf) ? last : at32(S.match, s * S.G + g);
      next[s] = ((uint32_t)s == sf || nxl) ? last + 1 : at32(S.next, s * S.G + g);
    }
  }
};

}  // namespace hb
