/*
 * hipbatch.h — C ABI of the MI355X batched Raft leader-bookkeeping engine.
 *
 * This is the drop-in boundary that a Go `raft/hipbatch` package binds through
 * cgo.  It replaces the per-group CPU loop that
 * `raft.MultiNode` runs in its single `run` goroutine
 * (reference: raft/multinode.go:166-322) for the leader-side bookkeeping:
 *
 *   - MsgAppResp progress updates    raft/raft.go:514-546, raft/progress.go:100-166
 *   - inflight flow control          raft/progress.go:172-237
 *   - quorum commit                  raft/raft.go:323-332, raft/log.go:241-247
 *   - vote tally / campaign          raft/raft.go:429-460, 585-614
 *   - the Step term gate             raft/raft.go:462-490
 *   - MultiNode dispatch filters     raft/multinode.go:233-237, raft/util.go:49-55
 *
 * Design rules:
 *   - Group state lives on the device as structure-of-arrays in HBM; one
 *     handle owns one GPU's shard of groups.  A handle is single-owner and not
 *     thread-safe, mirroring the single `run` goroutine that owns all group
 *     state in the reference (raft/multinode.go:166-168).
 *   - Every export returns an int: 0 = OK, negative = HB_E*.  Invariant
 *     violations that make the reference panic are reported per group as an
 *     HB_EV_FAULT event (the host then panics with the reference message); they
 *     never unwind across this ABI.
 *   - No torch types, no C++ types: plain pointers and sizes only.
 */
#ifndef HIPBATCH_H_
#define HIPBATCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_ABI_VERSION 8

/* ---- error codes -------------------------------------------------------- */
#define HB_OK          0
#define HB_EINVAL     -1   /* bad argument (range, size, unsupported config)   */
#define HB_ENOMEM     -2   /* device or pinned allocation failed               */
#define HB_EDEVICE    -3   /* HIP runtime error / no device                    */
#define HB_EINVARIANT -4   /* a device-side capacity invariant was violated    */

/* ---- limits -------------------------------------------------------------- */
#define HB_MAX_REPLICAS   7      /* n = len(r.prs) per group, 1..7 (north star: 3/5/7) */
#define HB_MAX_INFLIGHT   1024   /* Config.MaxInflightMsgs upper bound on device       */
#define HB_NO_LIMIT       UINT64_MAX  /* raft noLimit (raft/raft.go:30)                */
#define HB_NO_INDEX       UINT64_MAX
/* The log index (hb_reserve_log): per group, the cumulative Entry.Size() of
 * its log (finite MaxSizePerMsg) and its older term runs (follower side), in
 * rings of any power-of-two capacity; these are the capacities hb_create
 * starts every group with (128 bytes per ring). */
#define HB_SIZE_RING_MIN  16
#define HB_TERM_RING_MIN  8

/* ---- raft enums (values equal the reference's) --------------------------- */
/* StateType raft/raft.go:35-39 */
#define HB_STATE_FOLLOWER  0
#define HB_STATE_CANDIDATE 1
#define HB_STATE_LEADER    2
/* ProgressStateType raft/progress.go:19-23 */
#define HB_PR_PROBE     0
#define HB_PR_REPLICATE 1
#define HB_PR_SNAPSHOT  2
/* MessageType raft/raftpb/raft.proto:34-47 */
#define HB_MSG_HUP            0
#define HB_MSG_BEAT           1
#define HB_MSG_PROP           2
#define HB_MSG_APP            3
#define HB_MSG_APP_RESP       4
#define HB_MSG_VOTE           5
#define HB_MSG_VOTE_RESP      6
#define HB_MSG_SNAP           7
#define HB_MSG_HEARTBEAT      8
#define HB_MSG_HEARTBEAT_RESP 9
#define HB_MSG_UNREACHABLE    10
#define HB_MSG_SNAP_STATUS    11

/* ---- node references ------------------------------------------------------
 * Peers of a group are addressed by their slot in the group's peer list
 * (the host keeps slot -> node id).  lead / vote are encoded as:           */
#define HB_REF_SLOT_MAX   6      /* 0..6 = slot in the peer list              */
#define HB_REF_OTHER      0xD    /* an id that is not in prs (host keeps it)   */
#define HB_REF_SELF       0xE    /* r.id while r.id is not in prs              */
#define HB_REF_NONE       0xF    /* raft.None (raft/raft.go:29)                */
#define HB_SLOT_NONE      0xF    /* from_slot of a non-member / self not in prs*/

/* ---- messages (structure-of-arrays batch) --------------------------------
 * One batch = messages in arrival order, as the `run` goroutine would receive
 * them on recvc/propc.  Only the relative order of messages of the same group
 * is significant (groups are independent, raft/multinode.go:125-131).
 *
 * info[i] = type | from_slot << 4 | reject << 8 | voted << 9
 *   type      : HB_MSG_* of m.Type.  Device types: HUP, BEAT, PROP, APP_RESP,
 *               VOTE_RESP, HEARTBEAT_RESP, UNREACHABLE, SNAP_STATUS and the
 *               follower side: APP, HEARTBEAT, SNAP, VOTE.
 *   from_slot : slot of m.From in the group's prs, HB_SLOT_NONE if absent.
 *   reject    : m.Reject.
 *   voted     : only for from_slot == HB_SLOT_NONE: m.From is the node the
 *               group voted for (its Vote is HB_REF_OTHER), read by MsgVote's
 *               `r.Vote == m.From` (raft/raft.go:641).
 * term[i]  = m.Term (0 = local message, no term gate, raft/raft.go:471-472)
 * index[i] = m.Index; for HB_MSG_PROP the number of entries (>0); for
 *            HB_MSG_SNAP the snapshot's Metadata.Index.
 * hint[i]  = m.RejectHint of a rejected MsgAppResp; m.LogTerm of MsgApp /
 *            MsgVote; the snapshot's Metadata.Term of MsgSnap (may be NULL
 *            when the batch holds none of these).
 * commit[i]= m.Commit of MsgApp / MsgHeartbeat (may be NULL when it holds none).
 * MsgApp entries: message i's entries are k = eoff[i]..eoff[i+1] (the last
 *            message's run ends at n_edesc); eterm[k] = their terms (Index =
 *            m.Index + 1 + position), edesc[k] their descriptors (finite
 *            max_msg_size).
 * props    = optional dense [capacity] entry counts: group g first steps one
 *            MsgProp carrying props[g] entries (if > 0), before its messages
 *            in this batch.  NULL = none.
 *
 * Entry descriptors — read only when the handle's max_msg_size is finite
 * (neither HB_NO_LIMIT nor 0): sendAppend then sends entries(Next,
 * maxMsgSize) cut by limitSize (raft/raft.go:265, raft/util.go:97-110), which
 * needs every appended entry's protobuf size (raft/raftpb/raft.pb.go:1030-
 * 1043).  The device computes Entry.Size() from the descriptor plus the Term
 * and Index it assigns (appendEntry, raft/raft.go:351-360):
 *   edesc[k] = HB_ENT_DESC(len(Data), Type, Data != nil)
 *   eoff[i]  = first descriptor of MsgProp message i (its index[i] entries)
 *   peoff[g] = first descriptor of the dense proposal props[g]
 * n_edesc = number of descriptors (bytes copied with HB_STEP_HOST_PTRS).
 */
#define HB_INFO(type, from_slot, reject) \
  ((uint32_t)(type) | ((uint32_t)(from_slot) << 4) | ((uint32_t)((reject) ? 1 : 0) << 8))
#define HB_INFO_VOTED     0x200u
#define HB_ENT_MAX_DATA   0x3FFFFFFF
#define HB_ENT_DESC(data_len, type, has_data) \
  ((uint32_t)(data_len) | ((uint32_t)(type) << 30) | ((uint32_t)((has_data) ? 1 : 0) << 31))

typedef struct hb_batch {
  uint64_t        n;
  const uint32_t* group;
  const uint32_t* info;
  const uint64_t* term;
  const uint64_t* index;
  const uint64_t* hint;
  const uint32_t* props;
  uint64_t        n_edesc;   /* entries described by edesc / eterm */
  const uint32_t* edesc;
  const uint64_t* eoff;
  const uint64_t* peoff;
  const uint64_t* commit;
  const uint64_t* eterm;
} hb_batch;

/* hb_step flags */
#define HB_STEP_HOST_PTRS 0x1u   /* batch arrays are host pointers (copied H2D; up to 8 MiB in all
                                    they are packed into one pinned block during the call and sent
                                    with one copy, so the arrays may be reused once hb_step returns) */
#define HB_STEP_PROFILE   0x2u   /* record per-phase HIP events (hb_phase_ms)   */
#define HB_STEP_PROFILE_APPLY 0x4u  /* only the HB_PHASE_APPLY events (two, on the apply stream) */
#define HB_STEP_MSG_PROPS 0x8u   /* the batch carries MsgProp messages (no dense props): groups of
                                    3 keep a third route slot, so a leader's two MsgAppResp and its
                                    proposal stay on the fast path (a hint: results are the same) */

/* ---- per-group state (host view, array-of-structures) --------------------
 * Device keeps this as SoA.  Field meanings follow the reference:
 *   term/vote/commit : pb.HardState (raft/raft.go:126; vote is a node ref)
 *   lead, state      : SoftState (raft/node.go:40-43)
 *   committed        : raftLog.committed
 *   first_index      : raftLog.firstIndex()   (raft/log.go:150-159)
 *   last_index       : raftLog.lastIndex()    (raft/log.go:161-170)
 *   term_first..term_last : the maximal run of indices i in
 *        [first_index-1, last_index] with raftLog.term(i) == term.  Exact
 *        because log terms never decrease with the index and never exceed the
 *        current Term.  Empty run: term_first = HB_NO_INDEX, term_last = 0.
 *   snap_index       : raftLog.snapshot().Metadata.Index (0 = empty snapshot)
 *   votes_resp/grant : r.votes (raft/raft.go:139) as slot bitmasks; bit 7 =
 *                      r.id when r.id is not in prs.
 *   fault            : non-zero once the group hit a reference panic; the
 *                      device ignores the group until it is reloaded.
 *   commit_zero      : r.Commit (= HardState.Commit) is 0 although committed
 *                      is not.  The reference sets r.Commit = raftLog.committed
 *                      only in loadState and at the end of every Step that
 *                      passes the term gate (raft/raft.go:466,488,759), so a
 *                      group created with an empty HardState keeps r.Commit = 0
 *                      until its first Step: a bootstrapped MultiNode group
 *                      (committed = len(peers), raft/multinode.go:197-211) or
 *                      one restored from a snapshot (committed = firstIndex - 1,
 *                      raft/log.go:60).  handleAppendEntries tests m.Index <
 *                      r.Commit (raft/raft.go:652), not committed.  These are
 *                      the only values r.Commit takes (r.Commit == committed,
 *                      or 0 before the first Step); 0 = r.Commit == committed.
 *                      The device clears it when the group steps a message
 *                      past the term gate.
 */
typedef struct hb_progress {
  uint64_t match;
  uint64_t next;
  uint64_t pending_snapshot;  /* valid in HB_PR_SNAPSHOT, else 0 */
  uint32_t state;             /* HB_PR_* */
  uint32_t paused;
  uint32_t ins_start;         /* inflights.start */
  uint32_t ins_count;         /* inflights.count */
} hb_progress;

typedef struct hb_group {
  uint64_t term;
  uint64_t committed;
  uint64_t first_index;
  uint64_t last_index;
  uint64_t term_first;
  uint64_t term_last;
  uint64_t snap_index;
  uint32_t state;
  uint32_t n;
  uint32_t self_slot;         /* slot of r.id or HB_SLOT_NONE */
  uint32_t lead;              /* node ref */
  uint32_t vote;              /* node ref */
  uint32_t votes_resp;
  uint32_t votes_grant;
  uint32_t fault;             /* HB_FAULT_* */
  uint32_t commit_zero;       /* r.Commit == 0 != committed (no Step since an empty HardState) */
  uint32_t pad;
  hb_progress pr[HB_MAX_REPLICAS];
} hb_group;

/* fault codes: the reference panic each one stands for */
#define HB_FAULT_NONE            0
#define HB_FAULT_LEADER_CAMPAIGN 1  /* "invalid transition [leader -> candidate]" raft/raft.go:396 */
#define HB_FAULT_EMPTY_PROP      2  /* "%x stepped empty MsgProp" raft/raft.go:502               */
#define HB_FAULT_EMPTY_SNAPSHOT  3  /* "need non-empty snapshot" raft/raft.go:252-254            */
#define HB_FAULT_INFLIGHTS_FULL  4  /* "cannot add into a full inflights" raft/progress.go:192  */
#define HB_FAULT_NIL_PROGRESS    5  /* nil *Progress dereference (local msg from non-member)    */
#define HB_FAULT_COMMIT_RANGE    6  /* "tocommit(%d) is out of range" raft/log.go:175-177       */
#define HB_FAULT_NO_SELF         7  /* appendEntry with r.id not in prs (nil deref raft.go:358) */
#define HB_FAULT_FOLLOWER_LEADER 8  /* "invalid transition [follower -> leader]" raft/raft.go:409 (oracle KATs only) */
#define HB_FAULT_RAND_EXHAUSTED  9  /* engine-defined, no reference panic: hb_tick needed draw
                                       rand_pos of the group but hb_set_rand supplied fewer */
#define HB_FAULT_SIZE_WINDOW    10  /* engine precondition, no reference panic: with a finite
                                       max_msg_size, sendAppend needed the size of an entry the
                                       caller never loaded into the log index
                                       (hb_load_entry_sizes), or one a ring smaller than the
                                       log dropped (hb_reserve_log).  libhbnode loads and
                                       reserves both, so it never sees this code. */
#define HB_FAULT_TERM_WINDOW    11  /* engine precondition, no reference panic: the follower side
                                       needed the term of an entry the caller never loaded
                                       (hb_load_term_runs) or a too-small ring dropped; as above,
                                       unreachable through libhbnode */
#define HB_FAULT_CONFLICT_COMMITTED 12  /* "entry %d conflict with committed entry" raft/log.go:79 */

/* ---- events (the sparse delta list) ---------------------------------------
 * One ordered stream of 16-byte records per group describes everything the
 * host needs to build `Ready` (raft/node.go:447-463) for the groups that
 * changed: HardState/SoftState marks and the messages raft.send appended to
 * r.msgs (raft/raft.go:227-236), in the order the reference produced them.
 * Groups with no event did not change.  Marks are emitted eagerly at the
 * point the reference changes the value.
 *
 *   HB_EV_TERM      x = new Term                   (raft.reset, raft/raft.go:334-338)
 *   HB_EV_STATE     x = state | lead<<8 | vote<<16 (becomeFollower/Candidate/Leader,
 *                   and the follower side's r.lead / r.Vote = m.From); aux =
 *                   HB_STATE_OTH_LEAD / _VOTE when that lead / vote was just
 *                   set to the sender of the message being stepped and the
 *                   sender is outside prs (ref HB_REF_OTHER: its id is that
 *                   message's m.From); such an event is emitted even when the
 *                   packed refs did not change
 *   HB_EV_COMMIT    x = new committed              (raftLog.commitTo, raft/log.go:172-180)
 *   HB_EV_LAST      x = new lastIndex, aux = 1 for the becomeLeader noop entry,
 *                   0 for proposal entries        (raft.appendEntry, raft/raft.go:351-360)
 *   HB_EV_APP       to, x = m.Index (= Next-1).  Entries are (x, L] where L is
 *                   the current lastIndex (max_msg_size noLimit), x+1
 *                   (max_msg_size 0), or limitSize's cut of (x, lastIndex]
 *                   (finite max_msg_size); none if x+1 > lastIndex.  m.Commit =
 *                   current committed, m.Term = current term, m.LogTerm = term(x);
 *                   aux = 1 when term(x) == m.Term (the host then needs no log
 *                   lookup for LogTerm), else 0.
 *                   (raft.sendAppend, raft/raft.go:261-281)
 *   HB_EV_SNAP      to, x = snapshot index         (raft/raft.go:246-260)
 *   HB_EV_HEARTBEAT to, x = m.Commit              (raft.sendHeartbeat, raft/raft.go:285-299)
 *   HB_EV_VOTE      to, x = m.Index (lastIndex); m.LogTerm = lastTerm (raft/raft.go:435-442)
 *   HB_EV_PROP_FWD  to = lead ref, x = arrival index of the MsgProp (HB_NO_INDEX
 *                   for a dense props[] proposal)  (stepFollower, raft/raft.go:618-624)
 *   HB_EV_PROP_DROP x = arrival index (HB_NO_INDEX for props[]): proposal dropped
 *                   (raft/raft.go:587-589, 619-621)
 *   HB_EV_FAULT     aux = HB_FAULT_*, x = arrival index of the message
 *   HB_EV_RESP      a response the follower side sends to `to` (m.From of the
 *                   message being stepped: slot, or HB_REF_OTHER for a sender
 *                   outside prs): aux = HB_RESP_APP (MsgAppResp, x = m.Index),
 *                   HB_RESP_HEARTBEAT (MsgHeartbeatResp), HB_RESP_VOTE
 *                   (MsgVoteResp), | HB_RESP_REJECT; a rejecting MsgAppResp's
 *                   RejectHint is lastIndex at that point (raft/raft.go:651-682)
 *   HB_EV_FOLLOW    aux = HB_FOLLOW_STEP: the follower-side message at arrival
 *                   x (MsgApp / MsgHeartbeat / MsgSnap / MsgVote) is stepped
 *                   (it is not of a lower term; emitted before the term gate's
 *                   becomeFollower): the events up to the next one belong to it.
 *                   aux = HB_FOLLOW_APPEND: raftLog.maybeAppend appended that
 *                   MsgApp's entries from its first conflict (raft/log.go:72-88).
 *                   aux = HB_FOLLOW_RESTORE: that MsgSnap's snapshot was
 *                   restored (raft/raft.go:684-707): log = the snapshot, every
 *                   peer slot's Progress reset; a caller whose snapshot
 *                   ConfState differs from the group's peers reloads the group.
 */
#define HB_EV_TERM      1
#define HB_EV_STATE     2
#define HB_EV_COMMIT    3
#define HB_STATE_OTH_LEAD  1
#define HB_STATE_OTH_VOTE  2
#define HB_EV_LAST      4
#define HB_EV_APP       5
#define HB_EV_SNAP      6
#define HB_EV_HEARTBEAT 7
#define HB_EV_VOTE      8
#define HB_EV_PROP_FWD  9
#define HB_EV_PROP_DROP 10
#define HB_EV_FAULT     11
#define HB_EV_RESP      13
#define HB_EV_FOLLOW    14
#define HB_RESP_APP        0
#define HB_RESP_HEARTBEAT  1
#define HB_RESP_VOTE       2
#define HB_RESP_REJECT     8
#define HB_FOLLOW_STEP     0
#define HB_FOLLOW_APPEND   1
#define HB_FOLLOW_RESTORE  2

typedef struct hb_event {
  uint64_t x;
  uint32_t group;
  uint8_t  type;
  uint8_t  to;
  uint16_t aux;
} hb_event;

/* ---- step statistics (reduced over the batch; RCCL-reducible u64s) ------- */
#define HB_STAT_MSGS       0  /* messages stepped (after the membership filter)     */
#define HB_STAT_APPRESP    1  /* MsgAppResp stepped (incl. stale / ignored ones)     */
#define HB_STAT_VOTERESP   2  /* MsgVoteResp stepped                                 */
#define HB_STAT_DROPPED    3  /* responses from non-members (raft/multinode.go:235)  */
#define HB_STAT_COMMITS    4  /* groups whose committed advanced in this batch       */
#define HB_STAT_WON        5  /* elections won (candidate -> leader)                 */
#define HB_STAT_LOST       6  /* elections lost by poll (candidate -> follower)      */
#define HB_STAT_EVENTS     7  /* events emitted                                      */
#define HB_STAT_FAULTS     8  /* groups that faulted in this batch                   */
#define HB_STAT_ENTRIES    9  /* log entries appended (proposals + noops)            */
#define HB_STAT_COUNT      10

/* ---- phases (HB_STEP_PROFILE) -------------------------------------------- */
#define HB_PHASE_PARTITION 0  /* bucket radix sort + per-partition routing to lanes */
#define HB_PHASE_APPLY     1  /* steady-state fast path (the dominant kernel)      */
#define HB_PHASE_GENERAL   2  /* general state machine for handed-over groups      */
#define HB_PHASE_FINISH    3  /* statistics reduction                              */
#define HB_PHASE_COUNT     4

typedef struct hb_handle hb_handle;

/* ---- lifecycle ------------------------------------------------------------ */
/* Create a handle on `device` holding up to `capacity` groups of at most
 * `max_replicas` peers, MaxInflightMsgs = max_inflight (Config.MaxInflightMsgs,
 * raft/raft.go:98) and MaxSizePerMsg = max_msg_size (raft/raft.go:93; any
 * value: HB_NO_LIMIT, 0, or a finite size, for which the device keeps the
 * cumulative sizes of each group's log, see hb_load_entry_sizes /
 * hb_reserve_log).  `max_batch` bounds hb_step's n.
 * Device memory: per group ~100 B + nmax x (28 + 8 max_inflight) B of state,
 * 16 B + a 128-byte term-run ring, and for a finite max_msg_size 16 B + a
 * 128-byte size ring (rings grow with hb_reserve_log: 8 B per log entry,
 * 16 B per term run).
 * A step of at most 16,384 messages on a handle of at most 1M groups
 * partitions in one workgroup (one launch), and hb_events_to_host compacts at
 * most 1,024 chunks in one; HB_SMALL_STEP=0 in the environment at hb_create
 * keeps the tiled kernels for such steps (the same results). */
int  hb_create(int device, uint32_t capacity, uint32_t max_replicas,
               uint32_t max_inflight, uint64_t max_msg_size, uint64_t max_batch,
               hb_handle** out);
int  hb_destroy(hb_handle* h);
/* Launch on this HIP stream (hipStream_t as void*); NULL = the null stream.
 * This is the apply stream: the group state, the events and the statistics
 * are produced on it, in hb_step order. */
int  hb_set_stream(hb_handle* h, void* hip_stream);
/* Each hb_step runs in two stages: prep (sort the batch by bucket and route
 * every group's messages to it; a library-owned stream, double-buffered) and
 * apply (the raft bookkeeping; the apply stream).  Prep only reads the batch,
 * so the prep of step k+1 may run while step k applies.  Prep waits for the
 * work enqueued so far on the INPUT stream, the one that produces the batch
 * arrays: by default the apply stream (prep k+1 then starts after apply k);
 * a caller whose batches are ready earlier, or produced on a stream of their
 * own, names that stream here to let the two stages overlap.  NULL stream
 * pointer = the null stream.  The caller must keep a batch's arrays intact
 * until hb_step for it has been followed by hb_sync or by the next hb_step
 * returning. */
int  hb_set_input_stream(hb_handle* h, void* hip_stream);
int  hb_sync(hb_handle* h);   /* waits for both stages of every step so far */
int  hb_abi_version(void);
const char* hb_strerror(int code);

/* ---- group state (CreateGroup / RemoveGroup / Status) ---------------------
 * Load `count` groups into slots [first, first+count) from host records
 * (CreateGroup, raft/multinode.go:181-217; inflight windows start empty
 * unless set with hb_set_inflights).  Gather them back for Status
 * (raft/status.go:34-49). */
int  hb_load_groups(hb_handle* h, uint32_t first, uint32_t count, const hb_group* groups);
int  hb_get_groups(hb_handle* h, uint32_t first, uint32_t count, hb_group* out);
/* RemoveGroup (raft/multinode.go:219-222): mark slots empty (all messages to
 * them are ignored until reloaded). */
int  hb_remove_groups(hb_handle* h, uint32_t first, uint32_t count);
/* Relocate groups on the device (compacting, defragmenting or re-ordering the
 * slot space; libhbnode's role-ordered placement, hbn_set_placement).
 * Slot dst[i] takes everything the handle keeps for slot src[i], as it was before the call.
 * src[] are distinct; dst[] are distinct; src[i] == dst[i] is a no-op pair.
 * A swap is {a,b} -> {b,a}; cycles and chains are allowed.
 * Slots in src but not in dst end up empty, as after hb_remove_groups.
 * A dst slot that is not in src loses what it held.
 * src and dst are host arrays.
 * Ordered on the apply stream like hb_load_groups (synchronous).
 * Events already produced keep the old slot numbers.
 * "Everything" is the raw device state, not an hb_group round trip: the group
 * record and every Progress in whatever lazy form the device keeps them, the
 * timers (elapsed, rand_pos, election / heartbeat ticks), the peer ids of
 * hb_load_peers, each follower's live inflight window at its ring positions,
 * and both log-index rings with their content: hb_log_capacity(dst[i])
 * afterwards is what hb_log_capacity(src[i]) was.  The ring extents of the
 * overwritten slots pass to the vacated ones, so every slot still owns one of
 * each kind and repeated moves do not grow the log pool.  All sources are read
 * before any destination is written (staging buffers grown on demand and
 * reused: no device allocation per call in steady state).
 * HB_EINVAL, before any device work: a NULL handle, count > 0 with a NULL
 * array, a slot >= capacity, a duplicate in src, a duplicate in dst. */
int  hb_move_groups(hb_handle* h, uint32_t count, const uint32_t* src, const uint32_t* dst);
/* The application changed a group's Storage (MemoryStorage.Compact /
 * CreateSnapshot / ApplySnapshot, raft/storage.go:150-214): refresh the
 * device copies of raftLog.firstIndex() and raftLog.snapshot().Metadata.Index
 * that sendAppend reads (needSnapshot, raft/raft.go:246-260, 715-717) for
 * `count` group slots (host arrays). */
int  hb_set_log_bounds(hb_handle* h, uint32_t count, const uint32_t* groups,
                       const uint64_t* first_index, const uint64_t* snap_index);
/* ---- the log index ---------------------------------------------------------
 * What the device needs of a group's log besides its current-term run: the
 * entries' protobuf sizes (a finite MaxSizePerMsg: sendAppend cuts
 * entries(Next, maxMsgSize) with limitSize, raft/raft.go:265,
 * raft/log.go:219-224, raft/util.go:97-110, for ANY Next in the log) and the
 * terms below the current-term run (follower side: raftLog.term(i) for any i,
 * raft/log.go:198-217).  The host owns the log (it holds the payloads and
 * Storage) and loads both once per group; the device keeps them up to date as
 * it appends, truncates and restores.  Each lives in a per-group ring whose
 * capacity the host reserves: the ring drops its oldest element only when it
 * is full, so a capacity covering [firstIndex - 1, lastIndex] plus what the
 * next step can append (entries of MsgProp / props / MsgApp, one noop per
 * election) means nothing the reference can read is ever missing.
 *
 * Finite max_msg_size only: the Entry.Size() of the entries (last_index -
 * n_sizes[i], last_index] of group groups[i] (any n_sizes[i] <= last_index;
 * normally the whole log from first_index), in index order, concatenated over
 * i in `sizes` (host arrays); the ring grows to hold them.  hb_load_groups
 * leaves a group with none (only a follower at Next = last_index + 1 can be
 * served); a send that needs an entry never loaded faults HB_FAULT_SIZE_WINDOW. */
int  hb_load_entry_sizes(hb_handle* h, uint32_t count, const uint32_t* groups,
                         const uint32_t* n_sizes, const uint32_t* sizes);
/* Follower side: the terms of a loaded group's log below its current-term run
 * (term_first), which raftLog.term() lookups of MsgApp / MsgVote / MsgSnap
 * need (matchTerm, findConflict, isUpToDate; raft/log.go:72-123, 249-251).
 * groups[i] takes n_runs[i] runs (start index, term), oldest first, the pairs
 * of all groups concatenated in `runs` (host arrays): run k covers [start_k,
 * start_k+1) and the last one reaches term_first - 1 (or last_index when
 * term_first = HB_NO_INDEX); normally every run down to first_index - 1.  The
 * ring grows to hold them plus one.  hb_load_groups leaves a group with none:
 * a lookup below term_first then faults HB_FAULT_TERM_WINDOW. */
int  hb_load_term_runs(hb_handle* h, uint32_t count, const uint32_t* groups,
                       const uint32_t* n_runs, const uint64_t* runs);
/* Grow the rings of groups[i] to hold at least size_cap[i] cumulative sizes
 * (the span [oldest needed index, lastIndex] including firstIndex - 1; ignored
 * unless max_msg_size is finite) and run_cap[i] term runs (every run of the log
 * plus the runs the next step can start); a NULL array or 0 leaves that ring
 * as is.  Capacities round up to a power of two and never shrink; the content
 * is kept.  Synchronous (one copy kernel for the groups that grow).  Call it
 * before an hb_step / hb_tick that could outgrow a ring. */
int  hb_reserve_log(hb_handle* h, uint32_t count, const uint32_t* groups,
                    const uint64_t* size_cap, const uint64_t* run_cap);
/* The current ring capacities of one group (0 sizes: max_msg_size not finite). */
int  hb_log_capacity(hb_handle* h, uint32_t group, uint64_t* size_cap, uint64_t* run_cap);
/* Inflight window of (group, slot): buffer[(start + i) % max_inflight] = vals[i]. */
int  hb_set_inflights(hb_handle* h, uint32_t group, uint32_t slot,
                      uint32_t start, uint32_t count, const uint64_t* vals);
int  hb_get_inflights(hb_handle* h, uint32_t group, uint32_t slot,
                      uint32_t* start, uint32_t* count, uint64_t* vals /* [max_inflight] */);

/* ---- timers (MultiNode.Tick) ---------------------------------------------
 * Per group: r.elapsed, Config.ElectionTick / HeartbeatTick, and how many
 * values the group's r.rand has produced.  Every group of a MultiNode owns a
 * rand.Rand seeded with the same node id (raft/raft.go:189 with
 * config.ID = mn.id, raft/multinode.go:182), so all groups read one stream,
 * each at its own position.  The host supplies that stream (the outputs of
 * rand.New(rand.NewSource(id)).Int(), in order) with hb_set_rand and keeps it
 * longer than any group's rand_pos + 1 (one draw per group per tick at most).
 * hb_create sets election_tick 10, heartbeat_tick 1 (the reference tests'
 * defaults, raft/raft_test.go:1884-1894); hb_load_groups zeroes elapsed and
 * rand_pos of the loaded groups (newRaft: fresh rand, becomeFollower -> reset).
 * Follower-side receipts that reset r.elapsed (MsgApp / MsgHeartbeat /
 * MsgSnap / granted MsgVote, raft/raft.go:625-640) are handled by the host;
 * it reports them with hb_load_timers. */
typedef struct hb_timer {
  uint32_t elapsed;          /* r.elapsed */
  uint32_t rand_pos;         /* r.rand.Int() values taken so far */
  uint16_t election_tick;    /* r.electionTimeout (>= 1) */
  uint16_t heartbeat_tick;   /* r.heartbeatTimeout */
  uint32_t pad;
} hb_timer;
int  hb_load_timers(hb_handle* h, uint32_t first, uint32_t count, const hb_timer* timers);
int  hb_get_timers(hb_handle* h, uint32_t first, uint32_t count, hb_timer* out);
/* draws[i] = the (first + i)-th r.rand.Int() value (0 <= v < 2^63); the table
 * grows to first + count, earlier entries are kept.  Host memory. */
int  hb_set_rand(hb_handle* h, uint64_t first, uint64_t count, const uint64_t* draws);
/* One MultiNode.Tick (raft/multinode.go:264-275): every live group ticks
 * once, tickHeartbeat for leaders, tickElection otherwise (raft/raft.go:
 * 362-382, isElectionTimeout :765-771); a due MsgBeat / MsgHup is stepped at
 * once.  Events and statistics as for hb_step (the stepped MsgBeat / MsgHup
 * count in HB_STAT_MSGS).  flags: 0. */
int  hb_tick(hb_handle* h, uint32_t flags);

/* ---- wire ingestion ------------------------------------------------------
 * Decode raftpb.Message records (protobuf, raft/raftpb/raft.pb.go:549-799
 * Message.Unmarshal with its Entry / Snapshot / SnapshotMetadata / ConfState
 * sub-messages and gogo proto.Skip) straight into a device batch, as
 * multiNode.Step receives them (raft/multinode.go:432-439).  Record i is
 * bytes[off[i], off[i] + len[i]) for group slot group[i]; m.From becomes the
 * group's slot through the node ids set with hb_load_peers (HB_SLOT_NONE when
 * absent, so hb_step's membership filter applies).  bytes / off / len / group
 * and every array of `out` are device memory; out->props is ignored.  Record
 * i of `out` is the batch record (group = 0xFFFFFFFF unless HB_WIRE_OK, so
 * hb_step drops it); status[i] says what became of it:                      */
#define HB_WIRE_OK       0  /* MsgAppResp / MsgVoteResp / MsgHeartbeatResp: in the batch      */
#define HB_WIRE_LOCAL    1  /* local type from the network, dropped by Step (IsLocalMsg)      */
#define HB_WIRE_HOST     2  /* well-formed, not for the device batch (other types, or unknown
                               fields nesting groups deeper than 16): the host steps it        */
#define HB_WIRE_ERROR    3  /* Unmarshal returns an error (truncated, wrong / illegal wire type) */
#define HB_WIRE_PANIC    4  /* the reference would panic or never return (negative lengths)  */
#define HB_WIRE_BADGROUP 5  /* group[i] >= capacity                                          */
/* ids[i * HB_MAX_REPLICAS + s] = node id of slot s of group first + i (host memory). */
int  hb_load_peers(hb_handle* h, uint32_t first, uint32_t count, const uint64_t* ids);
int  hb_decode(hb_handle* h, const uint8_t* bytes, const uint64_t* off, const uint32_t* len,
               const uint32_t* group, uint64_t n, const hb_batch* out, uint8_t* status);

/* hb_decode plus the follower side: the bytes one engine's hb_encode (and the
 * host's splice of the entry payloads) writes, another engine steps.  Same
 * inputs; status[i] is hb_decode's, except that these HB_WIRE_HOST records
 * become HB_WIRE_OK batch records (the group being < capacity):
 *   MsgHeartbeat             always: term, index, commit = m.Commit, hint = 0
 *   MsgVote                  when m.From is a member of the group (a slot is
 *                            found; HB_INFO_VOTED needs the host otherwise):
 *                            term, index, hint = m.LogTerm
 *   MsgApp without entries   always: term, index, hint = m.LogTerm, commit
 *   MsgApp with entries      when the record has the shape Message.MarshalTo
 *                            writes (fields 1-6 once and in order, the field-7
 *                            run, field 8, the empty snapshot, fields 10 and
 *                            11, the end; varints of at most 10 bytes) and
 *                            every entry is 08 Type 10 Term 18 Index [22 len
 *                            Data] ending at its span, with Type the one byte
 *                            00 or 01, Index == m.Index + 1 + k and len(Data)
 *                            <= HB_ENT_MAX_DATA: as above, plus its entry run
 * Any other record Unmarshal accepts stays HB_WIRE_HOST (MsgSnap, MsgProp unless
 * hb_set_wire_props has HB_WIRE_PROPS_IN on, a
 * MsgApp whose entries have another shape or whose Entry error the reference
 * drops).  The three response types give hb_decode's record with commit = 0.
 * info = type | slot << 4 | reject << 8; a MsgApp or MsgHeartbeat from a
 * non-member has slot HB_SLOT_NONE.
 *
 * Entries: out->eoff[i], i in [0, n], is the first entry of record i and
 * eoff[n] = *n_ent the total (only HB_WIRE_OK MsgApp records have a run).  For
 * entry k: out->eterm[k], out->edesc[k] = HB_ENT_DESC(len(Data), Type, field 4
 * present), edata[k] = the offset in `bytes` of its first Data byte (0 when
 * Data is absent): the host keeps its payloads from there.  eterm / edesc /
 * edata hold ent_cap entries; when *n_ent > ent_cap none of their words is
 * written (eoff, status, the batch and *n_ent are) and the caller calls again.
 * The total of len[] / 8 always suffices: an entry is at least 8 wire bytes.
 *
 * The sentinel: the batch arrays of `out` (group, info, term, index, hint,
 * commit) and eoff have n + 1 elements, and record n is written as a dropped
 * record (group = 0xFFFFFFFF, the rest 0).  hb_step reads n_edesc only as the
 * end of the LAST record's run, and only when that record is a valid MsgApp;
 * so a caller steps b.n = n + 1 with b.n_edesc = ent_cap straight from these
 * arrays, and decode -> step needs no host read of the count (it must still
 * be <= ent_cap for the run to have been written).
 *
 * All arrays are device memory (bytes / off / len / group / status may be NULL
 * when n = 0, eterm / edesc / edata when ent_cap = 0); n_ent is device or
 * hb_alloc_pinned memory.  Asynchronous, on the stream hb_decode uses.
 * HB_EINVAL before any device work: a NULL handle or array, n + 1 >
 * max_batch, n >= 2^32.  n = 0 writes the sentinel, eoff[0] = 0, *n_ent = 0. */
#define HB_DECODE_FOLLOW 1
int  hb_decode_caps(void);   /* the decode features this library knows: HB_DECODE_FOLLOW */
int  hb_decode_follow(hb_handle* h, const uint8_t* bytes, const uint64_t* off, const uint32_t* len,
                      const uint32_t* group, uint64_t n, const hb_batch* out, uint8_t* status,
                      uint64_t ent_cap, uint64_t* edata, uint64_t* n_ent);

/* ---- wire egress ---------------------------------------------------------
 * The send path's counterpart of hb_decode: the payload-free messages a step
 * or tick produces (MsgAppResp, MsgHeartbeatResp, MsgVoteResp, MsgHeartbeat
 * and, in vote mode, campaign's MsgVote: no entries, the empty snapshot) leave
 * the device as the bytes
 * (in append mode a leader's MsgApp too: all of it but the entry payloads, which
 * the host splices in at a place the device names)
 * Message.MarshalTo writes (raft/raftpb/raft.pb.go:1271-1330), ready for the
 * transport, without the host replaying an event.  Two calls, both
 * asynchronous on the handle's stream:
 *   hb_egress  the last step's events -> a batch of outgoing messages
 *   hb_encode  such a batch -> wire bytes
 * A batch is a structure of arrays in device memory, capacity `cap` records: */
typedef struct hb_out_batch {
  uint32_t* group;    /* group slot                                                   */
  uint32_t* info;     /* HB_INFO(type, to_ref, reject) [| HB_OUT_HOST | HB_OUT_ENTS]; to_ref = slot or HB_REF_OTHER */
  uint64_t* to;       /* m.To as a node id (0 when to_ref == HB_REF_OTHER)            */
  uint64_t* term;     /* m.Term */
  uint64_t* log_term; /* m.LogTerm */
  uint64_t* index;    /* m.Index */
  uint64_t* commit;   /* m.Commit */
  uint64_t* hint;     /* m.RejectHint; with HB_OUT_ENTS the index of the last entry carried */
} hb_out_batch;
/* Egress on (any non-zero `on`): every later hb_step / hb_tick first copies the
 * groups' Term and lastIndex columns (16 B per group, allocated here) so that
 * hb_egress can give each message the Term and each rejection the RejectHint
 * of the point of its send: the events are a delta, the state after the step
 * holds only the final values.  Off (the default): nothing is allocated,
 * copied or launched, and hb_egress returns HB_EINVAL.
 * Bit HB_EGRESS_VOTES of `on` adds vote mode: a third column, the log's
 * lastTerm before the step (8 B per group more; a group whose last index lies
 * below its current-term run reads its term-run ring), and hb_egress also
 * makes campaign's MsgVote records.  Without the bit the snapshot and
 * hb_egress's output are what they were before the bit existed.  A call that
 * changes the mode while egress is on waits for the stream, allocates or frees
 * the column, and hb_egress gives count 0 until the next step or tick (the
 * step before the call has no matching snapshot).
 * Bit HB_EGRESS_APPS adds append mode: the lastTerm column as in vote mode,
 * the committed column and the boundary pair (the index just below the
 * current-term run and its term; 32 B per group more than plain egress, and a
 * group with a current-term run reads its term-run ring), and hb_egress also
 * makes sendAppend's MsgApp records.  The bits combine: the modes are 0, 1, 3,
 * 5 and 7.  Without the bit the kernels launched, the bytes the snapshot moves
 * and every output are what they were before the bit existed; a change of this
 * bit while egress is on behaves like a change of the vote bit. */
#define HB_EGRESS_ON    1
#define HB_EGRESS_VOTES 2
#define HB_EGRESS_APPS  4
int  hb_set_egress(hb_handle* h, int on);
/* The mode in force: 0 (off), or HB_EGRESS_ON | any of HB_EGRESS_VOTES and
 * HB_EGRESS_APPS (0, 1, 3, 5, 7); HB_EINVAL for a NULL handle.  Vote mode is an addition inside ABI 8 (every
 * value of `on` used before keeps its meaning), so the version number does not
 * tell whether a library knows the bit: one that lacks this function does not
 * (it takes any non-zero `on` as HB_EGRESS_ON and makes no vote record). */
int  hb_egress_mode(hb_handle* h);
/* The mode bits this library knows (HB_EGRESS_ON | HB_EGRESS_VOTES | HB_EGRESS_APPS): append
 * mode is an addition inside ABI 8 too, and a library that lacks this function lacks it. */
int  hb_egress_caps(void);
/* limitSize's cut in append mode (inside ABI 8, a knob of
 * its own so that hb_egress_mode / hb_egress_caps keep their values).  Off (the
 * default): under a finite non-zero max_msg_size every MsgApp record with
 * entries is HB_OUT_HOST, and every output of every call is what it was before
 * the knob existed.  On, on a handle in append mode whose max_msg_size is
 * finite and non-zero: such a record is an HB_OUT_ENTS record with hint = L,
 * the last entry limitSize lets through (raft/util.go:97-110: the first entry
 * of (index, last] always, every further one while the sum of Entry.Size()
 * stays <= max_msg_size), read at hb_egress from the group's ring of
 * cumulative sizes.  The record stays HB_OUT_HOST where that read cannot be
 * proven to be the send's: (i) the ring no longer holds the sum at `index`
 * (later appends or hb_set_log_bounds moved its oldest index past it, or the
 * group's sizes were never loaded); (ii) the group has a follower append or
 * restore (HB_EV_FOLLOW with aux APPEND / RESTORE) anywhere in the same call,
 * before or after the send, which may have rewritten the ring.  The other
 * reasons to flag a record, and every other column, are unchanged; with
 * max_msg_size 0 or HB_NO_LIMIT, or without append mode, the knob changes
 * nothing.  Precondition while on: hb_egress runs before any call that rewrites
 * a group's size ring (hb_load_entry_sizes, hb_load_groups, hb_remove_groups,
 * hb_move_groups), as it already runs before the next step; hb_reserve_log
 * keeps the contents and may come first.  A change of the knob while egress is
 * on waits for the stream, and hb_egress gives count 0 until the next step or
 * tick, as a mode change does.  hb_egress_limit returns 0 or 1, HB_EINVAL for a
 * NULL handle; a library that lacks hb_egress_limit_caps lacks the knob. */
#define HB_EGRESS_LIMIT_V1 1
int  hb_set_egress_limit(hb_handle* h, int on);
int  hb_egress_limit(hb_handle* h);
int  hb_egress_limit_caps(void);         /* the cut features this library knows: HB_EGRESS_LIMIT_V1 */
/* A probe resend's LogTerm in append mode (inside ABI 8,
 * a knob of its own like hb_set_egress_limit).  Off (the default): a MsgApp
 * record whose send lies below the index just under the leader's current-term
 * run is HB_OUT_HOST, and every output of every call is what it was before the
 * knob existed.  On, on a handle in append mode: such a record carries
 * log_term = the term of `index`, read at hb_egress from the group's ring of
 * older term runs (hb_load_term_runs and what the engine pushed since), as
 * raftLog.term gives it (raft/raft.go:261-281).  The record stays HB_OUT_HOST
 * where that read cannot be proven to be the send's: (i) the ring's oldest run
 * starts above `index` (the runs were never loaded that far, or Term changes
 * later in the call pushed that run out of a full ring); (ii) the group has a
 * follower append or restore (HB_EV_FOLLOW with aux APPEND / RESTORE) anywhere
 * in the same call, before or after the send, which may have cut the ring.
 * The other reasons to flag a record (Commit unknown, the limit without
 * hb_set_egress_limit) and every other column are unchanged, and a send at the
 * boundary keeps the boundary's term without a read; without append mode the
 * knob changes nothing.  Precondition while on: hb_egress runs before any call
 * that rewrites a group's run ring (hb_load_term_runs, hb_load_groups,
 * hb_remove_groups, hb_move_groups), as it already runs before the next step;
 * hb_reserve_log keeps the runs in order and hb_set_log_bounds does not touch
 * them, so both may come first.  A change of the knob while egress is on waits
 * for the stream, and hb_egress gives count 0 until the next step or tick, as
 * a mode change does.  hb_egress_logterm returns 0 or 1, HB_EINVAL for a NULL
 * handle; a library that lacks hb_egress_logterm_caps lacks the knob. */
#define HB_EGRESS_LOGTERM_V1 1
int  hb_set_egress_logterm(hb_handle* h, int on);
int  hb_egress_logterm(hb_handle* h);
int  hb_egress_logterm_caps(void);       /* the lookup features this library knows: HB_EGRESS_LOGTERM_V1 */
/* Forwarded proposals on the wire path (inside ABI 8, a
 * knob of its own so that hb_decode_caps, hb_egress_caps and hb_egress_limit_caps
 * keep their values).  With the bits at 0 (the default) every output of every
 * call is what it was before the knob existed.
 * HB_WIRE_PROPS_IN: hb_decode_follow makes an HB_WIRE_OK batch record of a
 * MsgProp that is the message r.send forwards (raft/raft.go:616-624, :226-236)
 * and nothing else:
 *   - the canonical shape (as for a MsgApp with entries, above), Type MsgProp;
 *   - Term == LogTerm == Index == Commit == 0, Reject false, RejectHint == 0;
 *   - at least one entry (an empty MsgProp panics a leader: the host reports
 *     it) and at most 2^23 - 1;
 *   - every entry is 08 00 | 10 00 | 18 00 | [22 len Data] ending at its span:
 *     Type, Term and Index the single byte 00 (what Propose makes; an
 *     EntryConfChange goes to the host, which holds pendingConf), len(Data) <=
 *     HB_ENT_MAX_DATA;
 *   - group[i] < capacity.  m.From may be a non-member (slot HB_SLOT_NONE).
 * Any other MsgProp stays HB_WIRE_HOST.  The batch record: info =
 * HB_INFO(HB_MSG_PROP, slot, 0), term = 0, index = the entry count, hint =
 * commit = 0; its entry run lies at eoff[i] like a MsgApp's, with eterm[k] = 0,
 * edesc[k] = HB_ENT_DESC(len, 0, field 4 present), edata[k] = the offset of the
 * first Data byte or 0.  eoff is one prefix sum over MsgApp and MsgProp runs;
 * the entry total, the ent_cap rule and the sentinel are unchanged.  The fate
 * of proposal i is in the step's events (HB_EV_LAST, HB_EV_PROP_FWD or
 * HB_EV_PROP_DROP with x = i).
 * HB_WIRE_PROPS_OUT: hb_egress makes one record per HB_EV_PROP_FWD event,
 * placed by the event's position like every other record: info =
 * HB_INFO(HB_MSG_PROP, to_ref, 0) | HB_OUT_ENTS with to_ref the event's lead ref
 * (a slot, or HB_REF_OTHER), to = the slot's node id (0 for HB_REF_OTHER), term
 * = log_term = index = commit = 0 (send leaves a MsgProp's Term at 0), hint =
 * the event's x: the arrival index of the proposal in the stepped batch, or
 * HB_NO_INDEX for a dense props[] proposal.  hb_encode writes it in the split
 * form (status HB_WIRE_SPLICE | prefix_len) and the host completes it with the
 * entries it holds for that arrival; hb_encode_ents never covers it.  No
 * pre-step column is read and nothing is allocated: the next hb_egress or
 * hb_decode_follow honours the bits.  The bit without egress on is legal and
 * inert.  hb_set_wire_props waits for the handle's streams; HB_EINVAL for a NULL
 * handle or any bit outside hb_wire_props_caps().  hb_wire_props returns the
 * bits in force, HB_EINVAL for a NULL handle; a library that lacks
 * hb_wire_props_caps lacks the knob. */
#define HB_WIRE_PROPS_IN   1   /* hb_decode_follow: a canonical MsgProp becomes a batch record   */
#define HB_WIRE_PROPS_OUT  2   /* hb_egress: HB_EV_PROP_FWD makes a MsgProp record               */
int  hb_set_wire_props(hb_handle* h, int bits);
int  hb_wire_props(hb_handle* h);
int  hb_wire_props_caps(void);           /* HB_WIRE_PROPS_IN | HB_WIRE_PROPS_OUT */
/* A vote record whose LogTerm the device cannot tell: info carries this flag
 * and log_term = 0; the host builds the message from its event as before.
 * Likewise a MsgApp record of append mode whose LogTerm, Commit or entry range
 * the device cannot tell: log_term = commit = hint = 0, only to, term and index
 * are the message's. */
#define HB_OUT_HOST     0x400u
/* A MsgApp record that carries entries (index, hint]: the hint column holds the
 * index of the last entry, not a RejectHint (a MsgApp's RejectHint is 0).  No
 * other consumer of info gives bit 11 a meaning: hb_encode reads bits 0-3, 4-7,
 * 8 and HB_OUT_HOST, hb_egress_bin bits 4-7. */
#define HB_OUT_ENTS     0x800u
/* One record per HB_EV_RESP / HB_EV_HEARTBEAT event of the last step or tick
 * (since hb_set_egress), in chunk order then word order of hb_events_device:
 * a group's records are in the order the reference appended the messages to
 * r.msgs.  m.Term = the group's Term at the send; a rejecting MsgAppResp's
 * RejectHint = its lastIndex at the send; `to` = the node id hb_load_peers
 * gave the slot (HB_EINVAL if no peer row was ever loaded), or to_ref =
 * HB_REF_OTHER and to = 0 for a sender outside prs (the host knows its id).
 * Vote mode: also one MsgVote record per HB_EV_VOTE event (one per slot of a
 * broadcast word's mask, in slot order): m.Term = the Term after
 * becomeCandidate, m.Index = the event's x, m.LogTerm = raftLog.lastTerm() at
 * the send, replayed from the pre-step column: the group's own appends
 * (HB_EV_LAST) set it to the Term of that point.  It is unknown, and the record
 * flagged HB_OUT_HOST, only when the group appended a leader's entries or
 * restored a snapshot earlier in the same call (the events carry no entry
 * terms), or when its last index lay below the current-term run and its term
 * runs were never loaded (hb_load_term_runs); a campaign from hb_tick never is.
 * Append mode: also one MsgApp record per HB_EV_APP event (one per slot of a
 * broadcast word's mask, in slot order, at consecutive output positions):
 * info = HB_INFO(HB_MSG_APP, slot, 0), m.Term = the Term at the send, m.Index =
 * the event's x, m.Commit = raftLog.committed at the send (the pre-step column,
 * then each HB_EV_COMMIT), m.LogTerm = the Term when the event's aux bit is set,
 * else the term of the index just below the current-term run when x is that
 * index (a new leader's first bcastAppend) and the device knows it.  With no
 * entries to send (x >= lastIndex at the send) hint = 0 and the record is an
 * ordinary payload-free one.  With entries info carries HB_OUT_ENTS and hint =
 * L, the last entry's index: lastIndex at the send under max_msg_size
 * HB_NO_LIMIT, x + 1 under max_msg_size 0.  The record is flagged HB_OUT_HOST
 * instead (log_term = commit = hint = 0) when the device cannot prove a value:
 * entries under a finite non-zero max_msg_size (limitSize's cut is in no
 * event), an aux = 0 send anywhere but at a known boundary, or any send after
 * the group appended a leader's entries or restored a snapshot earlier in the
 * same call until an HB_EV_COMMIT (Commit) and an HB_EV_TERM with a known
 * lastTerm (LogTerm) re-establish them.
 * Messages with a snapshot (HB_EV_SNAP), HB_EV_PROP_FWD unless hb_set_wire_props
 * has HB_WIRE_PROPS_OUT on (then one MsgProp record each, see above), without append mode
 * HB_EV_APP and without vote mode HB_EV_VOTE, make no record: the host builds
 * them as before.  self_id is this node's id; a record holds no sender (hb_encode
 * writes m.From), so hb_egress only takes it for symmetry with hb_encode.
 * *count (device-readable: device memory or hb_alloc_pinned memory) = the
 * number of records; when it exceeds cap only the first cap are written (a cut
 * may fall between two records of one broadcast word) and the caller calls
 * again (the events stay valid until the next step).  hb_egress itself puts no
 * bound on cap; hb_encode's and hb_egress_bin's (max_batch x (max_replicas + 4))
 * holds a MsgApp to every peer for every stepped message, so it is wide enough
 * for append mode whenever the step's dense proposals are no more than
 * 4 max_batch / (max_replicas - 1): a 1M x 3 step of one proposal and two acks
 * per group (max_batch >= 2M) makes 4M records against a bound of 14M. */
int  hb_egress(hb_handle* h, uint64_t self_id, const hb_out_batch* out, uint64_t cap, uint64_t* count);
/* Record i (m.From = self_id) becomes bytes[off[i], off[i+1]), packed densely
 * in record order, 28 to 91 bytes each; off[n] and *total = the byte count.
 * n = *n_dev (device-readable like *total, e.g. hb_egress's count, clamped to
 * cap; NULL = cap).  status[i] = HB_WIRE_OK, or HB_WIRE_HOST with length 0 for
 * a record whose to_ref is HB_REF_OTHER or whose info carries HB_OUT_HOST.
 * A record with HB_OUT_ENTS (and without HB_OUT_HOST) is written as prefix ||
 * suffix, the bytes of the same message without entries (fields 1-6, then
 * fields 8-11: Commit, the empty snapshot, Reject = 0, RejectHint = 0; still
 * 28 to 91 bytes), and status[i] = HB_WIRE_SPLICE | prefix_len (at most 57).
 * The full message is bytes[off[i], off[i] + prefix_len), then for each entry
 * of (index, hint] the bytes 0x3a, varint(Entry.Size()), Entry, then the rest of
 * the record: a three-part gather write.
 * When *total > bytes_cap no byte is
 * written (off, status and total are): call again with a larger buffer, 91 x n
 * always suffices.  HB_EINVAL before any device work: a NULL handle or array,
 * cap > max_batch x (max_replicas + 4), cap x 91 >= 2^32. */
#define HB_WIRE_SPLICE 0x80  /* hb_encode status bit: low 7 bits = where the entries go */
int  hb_encode(hb_handle* h, const hb_out_batch* in, uint64_t cap, const uint64_t* n_dev, uint64_t self_id,
               uint8_t* bytes, uint64_t bytes_cap, uint64_t* off /* [cap + 1] */, uint8_t* status /* [cap] */,
               uint64_t* total);

/* hb_encode with the entries written by the device: a leader's MsgApp leaves as
 * the whole message, no host splice.  Everything hb_encode says about n_dev,
 * off, status, total and dense packing in record order holds; off[n] and *total
 * = the byte count.  The entries come from a dense window table, one window per
 * group (the three per-entry words are those hb_decode_follow writes): */
#define HB_ENCODE_ENTS 1
int  hb_encode_caps(void);            /* the encode features this library knows: HB_ENCODE_ENTS */
typedef struct hb_ent_source {       /* every pointer is device memory */
  const uint64_t* first;    /* [capacity] index of the first entry held for group g            */
  const uint32_t* count;    /* [capacity] how many consecutive entries from first[g]; 0 = none */
  const uint64_t* start;    /* [capacity] place of entry first[g] in the three per-entry arrays */
  uint64_t        n_ent;    /* length of eterm / edesc / edata                                  */
  const uint64_t* eterm;    /* Entry.Term                                                       */
  const uint32_t* edesc;    /* HB_ENT_DESC(len(Data), Type, Data != nil)                        */
  const uint64_t* edata;    /* offset in `data` of the first Data byte (ignored without Data)   */
  const uint8_t*  data;
  uint64_t        data_len;
} hb_ent_source;
/* Entry first[g] + j of group g lies at position start[g] + j of eterm / edesc /
 * edata.  Windows may share positions and payload bytes.
 * - A record without HB_OUT_ENTS, or an HB_WIRE_HOST record (HB_REF_OTHER,
 *   HB_OUT_HOST), gets exactly the bytes and status hb_encode gives it.
 * - A record with HB_OUT_ENTS and without HB_OUT_HOST, of group g =
 *   in->group[i], carries entries (index, hint].  It is covered when
 *     g < capacity, hint > index, count[g] > 0, index + 1 >= first[g],
 *     (index + 1 - first[g]) + (hint - index) <= count[g],
 *     start[g] + count[g] <= n_ent,
 *     and for each of its entries with Data, edata + len <= data_len.
 *   The rule is evaluated without wrap-around, and no element of a per-entry
 *   array is read before the bounds that guard it have passed.
 * - A covered record is written whole, status = HB_WIRE_OK: the prefix (fields
 *   1-6), then per entry 0x3a, varint(Entry.Size()), 08 Type 10 varint(Term) 18
 *   varint(Index) [22 varint(len) Data] with Index = index + 1 + k (what
 *   Entry.MarshalTo writes, and the canonical shape hb_decode_follow accepts),
 *   then the suffix (fields 8-11).
 * - A record that is not covered is written as hb_encode writes it: prefix ||
 *   suffix, status = HB_WIRE_SPLICE | prefix_len; the host completes that one.
 *   Coverage is decided per record: covered and uncovered records mix freely.
 * - A record whose type is HB_MSG_PROP (hb_set_wire_props) is never covered: its
 *   (index, hint] is (0, arrival index], not an index range of the group's log.
 * Sizes and offsets are 64-bit throughout: a record can be many megabytes and
 * the total can pass 2^32; there is no cap x 91 bound.  When *total > bytes_cap
 * no byte of `bytes` is written (off, status and total are): call again.
 * Nothing outside data[0, data_len), the first n_ent elements of the per-entry
 * arrays and bytes[0, total) is touched.  `bytes` must not overlap src->data.
 * HB_EINVAL before any device work: a NULL handle, batch, batch array, src, off,
 * status or total; bytes NULL with bytes_cap > 0; first, count or start NULL; a
 * per-entry array NULL with n_ent > 0; data NULL with data_len > 0; cap >
 * max_batch x (max_replicas + 4) or cap >= 2^32.  Asynchronous on the handle's
 * stream; the struct itself is read during the call only. */
int  hb_encode_ents(hb_handle* h, const hb_out_batch* in, uint64_t cap, const uint64_t* n_dev, uint64_t self_id,
                    const hb_ent_source* src,
                    uint8_t* bytes, uint64_t bytes_cap, uint64_t* off /* [cap + 1] */, uint8_t* status /* [cap] */,
                    uint64_t* total);

/* ---- per-peer egress -----------------------------------------------------
 * A transport has one stream per remote node: it needs one contiguous byte
 * span per destination, each group's messages still in r.msgs order inside
 * it.  hb_egress_bin is a stable split of a record batch by destination node,
 * between hb_egress and hb_encode; the per-peer byte spans then fall out of
 * hb_encode's off[].  The chain hb_egress -> hb_egress_bin -> hb_encode (on
 * `out`) -> hb_peer_spans runs on the handle's stream and is fed by hb_egress's
 * device count: no host round trip.  Without a node table nothing is
 * allocated or launched. */
#define HB_EGRESS_MAX_PEERS 255
/* The node table of hb_egress_bin: n distinct non-zero node ids (host memory), n <= 255.
 * Bin b is ids[b] (the caller's order); bin n is "other".  n = 0 frees the table.
 * HB_EINVAL before any device work: NULL handle, n > 255, ids NULL with n > 0,
 * a zero or repeated id.  Stream-ordered against earlier hb_egress_bin calls
 * (it waits for the handle's stream: a configuration call). */
int  hb_set_egress_peers(hb_handle* h, const uint64_t* ids, uint32_t n);
/* Stable split of the first n records of `in` by destination:
 * n = *n_dev clamped to cap, or cap when n_dev is NULL (as hb_encode).
 * out = the same records, bin-major, and inside a bin in the order they had in `in`.
 * bin_off[b], b in [0, n_peers + 1]: first output record of bin b;
 * bin_off[n_peers + 1] = n.  So (n_peers + 2) u64 words of device or pinned memory.
 * src[j] (optional, may be NULL) = the index in `in` of output record j.
 * Bin of a record: to_ref == HB_REF_OTHER -> "other"; else the b with ids[b] == to
 * (all 64 bits); no such b -> "other".
 * A record flagged HB_OUT_HOST or HB_OUT_ENTS moves like any other: binned by its `to`,
 * info and hint unchanged, so append mode needs nothing from hb_egress_bin or hb_peer_spans.
 * Records of `out` (and src) at and past n are not written; `in` is not written.
 * n = 0 and cap = 0 are legal: bin_off is then all zeros.
 * HB_EINVAL before any device work: NULL handle / batch / array / bin_off, no table set,
 * cap > max_batch x (max_replicas + 4) or cap >= 2^32, any array of `out` equal to
 * the same array of `in`.  Asynchronous on the handle's stream. */
int  hb_egress_bin(hb_handle* h, const hb_out_batch* in, uint64_t cap, const uint64_t* n_dev,
                   const hb_out_batch* out, uint32_t* src, uint64_t* bin_off);
/* span[b] = off[bin_off[b]] for b in [0, n_peers + 1]: with `off` from an hb_encode of the
 * binned batch, peer b's bytes are bytes[span[b], span[b+1]).  One small launch, so that a
 * transport reads n_peers + 2 words instead of two per-record arrays.  span: device or
 * pinned memory.  HB_EINVAL: a NULL argument, no table set. */
int  hb_peer_spans(hb_handle* h, const uint64_t* off, const uint64_t* bin_off, uint64_t* span);

/* ---- framed peer streams -------------------------------------------------
 * A peer's byte span is a run of raftpb.Message records: it holds neither
 * their boundaries nor their groups (a Message carries no group id,
 * raft/multinode.go:432-439), and group[i] of a record batch is the sender's
 * slot, which means nothing on another node.  What two nodes share is the
 * 64-bit MultiNode group id.  hb_frame writes one index frame per non-empty
 * peer bin beside the bytes: the group id and the length of every record, so a
 * transport ships two spans per peer (index[ispan[b], ispan[b+1]) and
 * bytes[span[b], span[b+1])) and nothing per record.  hb_unframe turns the
 * frames of several peers into the off / len / group arrays hb_decode_follow
 * takes, through a device directory from group id to the receiver's slot; no
 * host read lies between.  An addition inside ABI 8: a library that lacks
 * hb_frame_caps lacks all of it.
 *
 * The index frame, little-endian, every frame at a multiple of 8 bytes:
 *    0 u32 magic 0x31464248 ("HBF1")    4 u32 flags  0
 *    8 u64 from  the sender's node id  16 u64 to     the destination's (ids[b])
 *   24 u64 seq   the caller's number   32 u64 bytes  span[b+1] - span[b]
 *   40 u32 count rows c                44 u32 holes  rows with the hole bit
 *   48 u64 gid[c]
 *   48 + 8c  u32 len[c]   bits 0..30 the record's byte length, bit 31 = hole
 *            (4 zero bytes when c is odd)
 * hb_frame_size(c) = 48 + 12c + 4(c & 1) for c > 0 and 0 for c = 0 (an empty
 * bin makes no frame; UINT64_MAX for c >= 2^32); it is injective, and
 * hb_frame_rows is its inverse (UINT64_MAX for a length no count gives): a
 * receiver takes c from the frame's length.  Row j is the bin's j-th record;
 * the records' bytes are the peer's span as it is.  A hole is a row whose
 * bytes, if any, lie in the span but are no message for the receiver: status[i]
 * != HB_WIRE_OK (HB_WIRE_HOST with length 0, or HB_WIRE_SPLICE | k: a split
 * MsgApp must not be decoded as one without entries), group[i] >= capacity (its
 * gid word is 0), or a group whose id is 0 (unset). */
#define HB_FRAME_V1 1
int  hb_frame_caps(void);                       /* the frame features this library knows: HB_FRAME_V1 */
uint64_t hb_frame_size(uint64_t rows);
uint64_t hb_frame_rows(uint64_t index_len);

/* The directory, group id -> slot: open addressing over cap keys (a power of
 * two), first probe splitmix64(id) & (cap - 1), linear probing, key 0 = empty,
 * at most cap probes, then "absent".  key / slot are caller-owned device memory
 * that the engine reads during a call only (as hb_ent_source): after
 * hb_move_groups the caller permutes its id column and builds again. */
typedef struct hb_gid_dir { const uint64_t* key; const uint32_t* slot; uint64_t cap; } hb_gid_dir;
/* Clears key[0, cap), then inserts every non-zero gid[i] -> i (gid: device,
 * [count]: the id of slot i, 0 = none).  *dups (device or pinned) = the ids
 * that were present already when inserted: such an id maps to one of its slots,
 * and the caller treats *dups > 0 as an error.  The table's layout depends on
 * the order of the inserts and is unspecified; lookups are not.  HB_EINVAL
 * before any device work: a NULL handle or array, cap not a power of two, cap <
 * 64 or cap < 2 x count.  Three launches (clear, insert, the count), asynchronous on
 * the stream hb_decode uses. */
int  hb_gid_dir_build(hb_handle* h, const uint64_t* gid, uint32_t count, uint64_t* key, uint32_t* slot,
                      uint64_t cap, uint32_t* dups);

/* The index frames of a binned batch: `binned`, bin_off from hb_egress_bin, off
 * and status from hb_encode / hb_encode_ents of it, span from hb_peer_spans,
 * gid = device [capacity] (the id of every slot, 0 = unset).  Reads group and
 * to of the batch, off, status, bin_off, span and gid, and no message byte; the
 * record count is bin_off[n_peers + 1].  ispan[b], b in [0, n_peers + 1] = the
 * bytes of the frames of the bins before b (ispan[n_peers] = ispan[n_peers + 1]
 * = the total: bin n_peers, "other", never gets a frame).  When the total
 * exceeds index_cap no byte of `index` is written (ispan and fstat are): call
 * again.  fstat[b], b in [0, n_peers) = the bin's hole count, or 0xFFFFFFFF for
 * a bin with a record of 2^31 bytes or more, which no len word holds: its
 * header is written with magic 0 (a receiver rejects it) and its rows are
 * unspecified; fstat[n_peers] = 0.  seq is copied into every header.  index:
 * device memory at a multiple of 8; ispan / fstat: device or pinned.  A bin_off
 * that does not ascend or ends past max_batch x (max_replicas + 4) is read as
 * an empty batch.  HB_EINVAL before any device work: a NULL argument (index
 * with index_cap > 0), a misaligned index, no node table set.  Asynchronous on
 * the handle's stream. */
int  hb_frame(hb_handle* h, const hb_out_batch* binned, const uint64_t* off, const uint8_t* status,
              const uint64_t* bin_off, const uint64_t* span, const uint64_t* gid /* device [capacity] */,
              uint64_t self_id, uint64_t seq, uint8_t* index, uint64_t index_cap,
              uint64_t* ispan /* [n_peers + 2] */, uint32_t* fstat /* [n_peers + 1] */);

/* n_frames received frames -> the record arrays of hb_decode_follow.  Frame k
 * is index[index_off, index_off + index_len) with its bytes at [bytes_off,
 * bytes_off + bytes_len) of the buffer the caller will decode, and came from
 * node `from`; `frames` is host memory, read during the call.  rows_k =
 * hb_frame_rows(index_len); its rows take output positions [base_k, base_k +
 * rows_k) in the caller's frame order, n = the sum.  fstatus[k] (device or
 * pinned): */
#define HB_FRAME_OK         0  /* the frame passed every check                                    */
#define HB_FRAME_BAD_MAGIC  1  /* the magic or the flags are wrong                                */
#define HB_FRAME_BAD_COUNT  2  /* the header's count differs from rows_k                          */
#define HB_FRAME_BAD_ROUTE  3  /* to != self_id, or from != frames[k].from                        */
#define HB_FRAME_BAD_LENGTH 4  /* the header's bytes, or the 64-bit sum of the rows' lengths (holes
                                  included), differ from bytes_len                                */
/* (the first that applies, in this order; a frame of no rows is OK when
 * bytes_len is 0 and BAD_LENGTH otherwise).  Every row of a bad frame becomes
 * off = 0, len = 0, group = 0xFFFFFFFF.  In a good frame off = bytes_off + the
 * sum of the lengths of the rows before it, so every offset lies inside the
 * frame's byte range; a delivered row has len = its length and group = the
 * directory's slot; a dropped row has len = 0 and group = 0xFFFFFFFF, which
 * hb_decode_follow drops: a hole, a gid of 0, or a gid absent from the directory
 * (the reference's "no such group: ignore", raft/multinode.go:233-237).
 * *n_unknown (device or pinned) = the rows dropped for an absent gid.  No
 * payload byte is read: malformed payload is hb_decode_follow's business.
 * off / len / group: device memory, n elements; index: device memory at a
 * multiple of 8.  bytes_size bounds the byte ranges only, so offsets past 2^32
 * are fine.  HB_EINVAL before any device work: a NULL handle or array (index /
 * off / len / group may be NULL when n = 0), index_off not a multiple of 8, a
 * range outside index_size or bytes_size, an index_len no row count gives, n !=
 * the sum of rows_k, n > max_batch, n_frames > 256, a directory whose cap is no
 * power of two.  n = 0 and n_frames = 0 are legal.  Asynchronous on the stream
 * hb_decode uses; hb_decode_follow(h, bytes, off, len, group, n, ...) and
 * hb_step follow unchanged. */
typedef struct hb_frame_in { uint64_t index_off, index_len, bytes_off, bytes_len, from; } hb_frame_in;
int  hb_unframe(hb_handle* h, const uint8_t* index, uint64_t index_size, const hb_frame_in* frames /* host */,
                uint32_t n_frames, uint64_t self_id, const hb_gid_dir* dir, uint64_t bytes_size,
                uint64_t* off, uint32_t* len, uint32_t* group, uint64_t n,
                uint32_t* fstatus /* [n_frames] */, uint64_t* n_unknown);

/* ---- the hot path ----------------------------------------------------------
 * Step one batch (all messages of the batch, per group in arrival order).
 * Asynchronous on the handle's stream.  Events and statistics of the step
 * are read with the functions below. */
int  hb_step(hb_handle* h, const hb_batch* b, uint32_t flags);

/* Events of the last step, as written by the device (zero-copy access for a
 * consumer on the GPU): `n_chunks` chunks, two per 256-group partition p
 * (chunk 2p: the events of the dense props[] proposals, chunk 2p+1: the
 * events of the partition's messages); chunk c holds counts[c] 8-byte words
 * at base + chunk_off[c].  A group's events are its words in chunk 2p, then
 * in chunk 2p+1, each in order.  Word format (bit ranges):
 *   [0:4)   type: HB_EV_*; 12 = an HB_EV_APP to every slot of the mask in
 *           `to` (same x and aux), in slot order; 0 = an HB_EV_VOTE to every
 *           slot of the mask (same x, aux 0: campaign's MsgVotes), in slot
 *           order; 15 = continuation word
 *   [4:11)  to (slot / node ref), or the slot mask of types 12 and 0
 *   [11]    x needs 64 bits: the next word is a continuation holding
 *           x bits 40..63 in its bits [4:28)
 *   [12:16) aux
 *   [16:24) group - 256 p
 *   [24:64) x bits 0..39
 * hb_copy_events expands them into hb_event records.  Device pointers; valid
 * until the next hb_step. */
#define HB_EVW_BCAST 12
#define HB_EVW_VBCAST 0
#define HB_EVW_CONT  15
int  hb_events_device(hb_handle* h, const uint64_t** base, const uint64_t** chunk_off,
                      const uint32_t** counts, uint32_t* n_chunks);
/* Gather the last step's events densely into host memory (synchronizes).
 * *n = number of events; returns HB_EINVAL if cap is too small. */
int  hb_copy_events(hb_handle* h, hb_event* out, uint64_t cap, uint64_t* n);
/* The compact delta list for a host consumer: the last
 * step's event words exactly as the device wrote them (format above), densely
 * in chunk order, written by the device into pinned host memory from
 * hb_alloc_pinned: words[0 .. *total) when *total <= cap (else only counts and
 * total are written: call again with a larger buffer, the step's events stay
 * valid until the next hb_step / hb_tick), counts[c] = the words of chunk c for
 * every chunk (hb_event_words_chunks).  Asynchronous on the handle's stream
 * (8 bytes per word over PCIe instead of hb_copy_events' 16 per event, one
 * word per bcastAppend): the host reads the buffers after hb_sync.  A group's
 * events are its words in chunk 2p, then chunk 2p + 1, in order, p = group /
 * groups_per_chunk; hb_expand_event_words turns them into hb_event records. */
int  hb_events_to_host(hb_handle* h, uint64_t* words, uint64_t cap, uint32_t* counts, uint64_t* total);
int  hb_event_words_chunks(hb_handle* h, uint32_t* n_chunks, uint32_t* groups_per_chunk);
/* Host-side expansion of hb_events_to_host's output into hb_event records
 * (*n_out = the number of records; HB_EINVAL if cap is too small; out NULL
 * only counts).  Pure CPU, no handle. */
int  hb_expand_event_words(const uint64_t* words, uint64_t n_words, const uint32_t* counts, uint32_t n_chunks,
                           hb_event* out, uint64_t cap, uint64_t* n_out);
/* Statistics of the last step: device pointer to HB_STAT_COUNT u64 (for an
 * RCCL all-reduce on the same stream) or a synchronous host copy. */
int  hb_stats_device(hb_handle* h, uint64_t** dev_stats);
int  hb_stats(hb_handle* h, uint64_t* out);
/* Asynchronous device-to-device copy of the last step's statistics (on the
 * handle's stream), e.g. into a buffer that an RCCL all-reduce then sums. */
int  hb_stats_to(hb_handle* h, uint64_t* dev_dst /* [HB_STAT_COUNT] */);
/* Optional device accumulator: every later hb_step also adds its statistics
 * into dev_accum[HB_STAT_COUNT] in its finish phase (no extra launch).
 * NULL turns it off.  The buffer must outlive its use. */
int  hb_set_stats_accum(hb_handle* h, uint64_t* dev_accum);
/* Per-phase device time (ms) averaged over the HB_STEP_PROFILE steps since
 * hb_phase_reset (the last 256 of them); *steps = how many (synchronizes). */
int  hb_phase_ms(hb_handle* h, float* out /* [HB_PHASE_COUNT] */, uint32_t* steps);
int  hb_phase_reset(hb_handle* h);
/* Which apply kernels the last hb_step launched (for profiles and rooflines):
 * HB_KERN_ROUTE_FAST = the route and the n = 3 fast lane ran as one kernel
 * (k_route_fast; HB_PHASE_APPLY then brackets it), else k_route and
 * k_apply_fast / k_apply_lead separately.  HB_KERN_ROUTE_ELECT = (n >= 5,
 * batches without dense proposals) the route closed the partitions whose
 * groups k_apply_lead would only hand over and ran the election lane there
 * (k_route<8, false, n>; HB_STORM=0 at hb_create turns it off).
 * HB_KERN_ROUTE_FAST_WIDE = (with HB_KERN_ROUTE_FAST) k_route_fast ran in its
 * wide form, 1,024 lanes and twice the groups per workgroup: the choice of an
 * n = 3 handle whose buckets hold 4,096 groups or more (HB_RF_WIDE=0 / 1 at
 * hb_create overrides it there). */
#define HB_KERN_ROUTE_FAST 1u
#define HB_KERN_ROUTE_ELECT 2u
#define HB_KERN_ROUTE_FAST_WIDE 4u
int  hb_step_kernels(hb_handle* h, uint32_t* mask);
/* The n = 3 fast lane steps a wave whose 64 groups are all in steady
 * replication (or have nothing to step) by a straight-line path; HB_FAST_STEADY=0
 * at hb_create turns that off (same output).  For tests: with
 * HB_FAST_STEADY_COUNT=1 at hb_create the last hb_step counted the waves of
 * groups that took the path (waves of grid padding excluded); *n = that
 * count, 0 when the knob was not set (synchronizes). */
int  hb_steady_waves(hb_handle* h, uint32_t* n);

/* On handles with max_replicas <= 3 the engine does not keep the per-slot Next
 * of a leader whose every slot has Next == lastIndex + 1 (what bcastAppend's
 * optimistic update leaves a healthy leader with at every step boundary): the
 * steady step neither reads nor writes those words, and hb_get_groups derives
 * them.  HB_LAZY_NEXT=0 at hb_create turns that off (same output).  For
 * tests: *n = the live groups currently held in that form (synchronizes);
 * always 0 with HB_LAZY_NEXT=0 or max_replicas > 3. */
int  hb_lazy_next_groups(hb_handle* h, uint32_t* n);

/* ---- pinned host memory for cgo callers (Go must not hand Go memory to C
 * that C retains; raft/hipbatch packs batches into these buffers). -------- */
int  hb_alloc_pinned(size_t bytes, void** out);
int  hb_free_pinned(void* p);

#ifdef __cplusplus
}
#endif
#endif /* HIPBATCH_H_ */
