"""Hand-built leader scenarios of wire egress with limitSize's cut, on top
of tests/egress_app_cases.py: that set, which runs unchanged under any finite
max_msg_size, and the cases that are about the cut.

Every entry here is pb.Entry{Term, Index} without Data, so Entry.Size() is 4 + sov(Term) +
sov(Index): 6 bytes while both are below 128.  Under the limits below, entries (5, 8] of
"prop-k" (18 bytes) are

  LIMITS   13  cut after two: (5, 7]         1   every entry exceeds it: (5, 6]
           18  the sum exactly: (5, 8]       17  one byte less: (5, 7]
         1000  "probe-behind": 200 entries behind, a long binary search

Every case states how many of its records stay HB_OUT_HOST, as egress_app_cases does;
FLAGGED names the reasons.  The wide cases (wide_scenarios) stand at an index base of their
own, each with the two limits that cut one entry apart.
"""
import numpy as np

from etcd_amd import abi, synth
from oracle.pyoracle import Raft

from . import egress_app_cases as AC
from .egress_app_cases import _acks, _case
from .egress_cases import _m
from .lift_util import base

A = abi
SIZES = AC.SIZES
LIMITS = (13, 1, 18, 17, 1000)
BEHIND = 200  # entries "probe-behind"'s leader appends before the batch
FLAGGED = dict(AC.FLAGGED)
FLAGGED["send-then-truncate"] = "a follower append after the send: the ring may not be the one the send read"


def entry_size(term, index):
    """Entry.Size() of pb.Entry{Term, Index} (raft/raftpb/raft.pb.go:1030-1043)."""
    sov = lambda v: max(1, (v.bit_length() + 6) // 7)  # noqa: E731
    return 4 + sov(term) + sov(index)


def scenarios(sizes=SIZES):
    out = AC.scenarios(sizes)
    for n in sizes:
        T = 4 + n
        cur = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        hard = (T, 0, 2)
        fol = list(range(2, n + 1))
        prop = lambda k=1: _m(A.HB_MSG_PROP, 1, nents=k)  # noqa: E731
        # a Probe follower 200 entries behind: the proposal's broadcast goes to Probe followers at
        # Next 5 and pauses them; follower 2's progress is set anew (Probe, Next 5, not paused), so
        # its MsgHeartbeatResp sends (4, L]; its ack of L makes it Replicate at Next L + 1 and the
        # resend starts there
        L = probe_cut(T + 1, 1000)
        out.append(_case("probe-behind", n, "leader", cur, hard,
                         [_m(A.HB_MSG_HEARTBEAT_RESP, 2, T + 1), _m(A.HB_MSG_APP_RESP, 2, T + 1, L)],
                         setup=[("step", prop(BEHIND)), ("progress", 2, 0, 5)]))
        # a send, then a step-down and a truncating append in the same call: fresh Probe followers
        # get (4, 6]; the new leader's MsgApp at 4 conflicts with the noop at 5 and replaces (4, 6]
        out.append(_case("send-then-truncate", n, "leader", cur, hard,
                         [prop(), _m(A.HB_MSG_APP, 2, T + 3, 4, T, 3, ents=[T + 3])], flagged=n - 1))
        # the proposals of 2 and 3 entries that the acks chase under a small limit
        out.append(_case("prop-then-acks", n, "leader", cur, hard,
                         [prop(3)] + _acks(fol, T + 1, 6) + _acks(fol, T + 1, 7),
                         setup=[("step", m) for m in _acks(fol, T + 1, 5)]))
    return out


def probe_cut(term, limit, x=4, last=5 + BEHIND):
    """The last entry of (x, last] that `limit` lets through."""
    total, i = entry_size(term, x + 1), x + 1
    while i < last and total + entry_size(term, i + 1) <= limit:
        i += 1
        total += entry_size(term, i)
    return i


WIDE = ("P35", "W32", "W40", "W62")


def wide_base(name):
    """(B, Tb): entries B + 6, B + 7, B + 8 are the proposal's.  P35: B + 7 = 2^35, where
    sov(Index) grows from 5 to 6; the others are tests/lift_util.py's bases."""
    return ((1 << 35) - 7, 0) if name == "P35" else base(name, delta=7, eps=3)


def wide_limits(name, n):
    """The two limits one entry's last byte apart: entries B + 6 and B + 7 exactly, and one less."""
    B, Tb = wide_base(name)
    t = Tb + 4 + n + 1
    both = entry_size(t, B + 6) + entry_size(t, B + 7)
    return both, both - 1


def wide_scenarios(name, sizes=SIZES):
    """"prop-k" and "cfg2" on a log that starts at a snapshot at B + 2: (B+3, T-1) (B+4, T), the
    leader's noop at B + 5."""
    B, Tb = wide_base(name)
    out = []
    for n in sizes:
        T = Tb + 4 + n
        ents = [(B + 3, T - 1), (B + 4, T)]
        fol = list(range(2, n + 1))
        repl = [("step", m) for m in _acks(fol, T + 1, B + 5)]
        for cname, msgs in (("prop-k", [_m(A.HB_MSG_PROP, 1, nents=3)]),
                            ("cfg2", [_m(A.HB_MSG_PROP, 1, nents=1)] + _acks(fol, T + 1, B + 6))):
            out.append(_case(f"{cname}-{name}", n, "leader", ents, (T, 0, B + 2), msgs, setup=repl,
                             snapshot=(B + 2, T - 1)))
    return out


def log_sizes(r):
    """Entry.Size() of every entry the raft's log holds, firstIndex first (all without Data)."""
    return [entry_size(r.term(i), i) for i in range(r.firstIndex, r.lastIndex + 1)]


def build(c, max_msg_size):
    """egress_app_cases.build on a raft with a finite max_msg_size: the sizes of the log it
    starts with are loaded before it takes its role (hb_load_entry_sizes); what it appends
    itself it sizes itself."""
    r = Raft(1, c["peers"], ents=c["ents"], snapshot=c["snapshot"], hard=c["hard"], max_msg_size=max_msg_size)
    r.load_sizes(log_sizes(r))
    if c["role"] != "follower":
        r.becomeCandidate()
        if c["role"] == "leader":
            r.becomeLeader()
    for op in c["setup"]:
        if op[0] == "step":
            r.Step(AC.oracle_msg(op[1]))
        else:
            r.setProgress(*op[1:])
    assert not r.fault, c["name"]
    r.readMessages()
    return r


def cfg2_sized_inputs(G=300, n=3):
    """The cfg2 step of test_egress_app_gpu.test_max_msg_size for a finite limit: (groups, runs,
    loaded sizes, batch).  Every leader's whole log has its size loaded; group g proposes
    1 + g % 3 entries with random descriptors of up to 100 payload bytes."""
    g, runs = synth.steady_groups(G, n, seed=911, last_hi=1 << 12)
    loaded = synth.window_sizes(g, runs, seed=912, frac_full=1.0)
    b = synth.cfg2_batch(g, 0, seed=913)
    b["props"] = (1 + np.arange(G) % 3).astype(np.uint32)
    b["index"] = (g["last_index"][b["group"]] + b["props"][b["group"]]).astype(np.uint64)
    return g, runs, loaded, synth.attach_entry_descs(b, G, seed=914, max_len=100)


RING_PROPS, RING_K = 4, 6


def ring_scenario(G=40, n=3, limit=150):
    """Rule (i): leaders whose size ring stays at HB_SIZE_RING_MIN = 16 (the last 8 sizes loaded,
    nothing reserved) take four MsgProp messages of six entries each in one call, 24 entries
    against a ring of 16.  The first three carry entries without Data (about 8 bytes each: the six
    go whole, so every Replicate follower's Next keeps up and no send reaches below the ring), the
    last one entries of 60 to 100 payload bytes, which the limit cuts.  After the call the ring
    holds [last0 + 9, last0 + 24]: the sends at last0 and last0 + 6 are flagged, those at
    last0 + 12 and last0 + 18 carry their cut.  (groups, runs, loaded, batch, limit)."""
    g, runs = synth.steady_groups(G, n, seed=921, last_hi=1 << 10)
    whole = synth.window_sizes(g, runs, seed=922, frac_full=1.0)
    loaded = {gi: z[-8:] for gi, z in whole.items()}
    rng = np.random.default_rng(923)
    N = RING_PROPS * G
    zero = np.zeros(N, np.uint64)
    batch = dict(group=np.tile(np.arange(G, dtype=np.uint32), RING_PROPS),
                 info=np.full(N, A.hb_info(A.HB_MSG_PROP, 0), np.uint32), term=zero,
                 index=np.full(N, RING_K, np.uint64), hint=zero, props=None, msg_props=True,
                 eoff=np.arange(N, dtype=np.uint64) * np.uint64(RING_K))
    desc = np.zeros((RING_PROPS, G, RING_K), np.uint32)
    desc[-1] = rng.integers(60, 101, (G, RING_K)).astype(np.uint32) | np.uint32(1 << 31)
    batch["edesc"] = desc.reshape(-1)
    return g, runs, loaded, batch, limit
