"""Hand-built leader scenarios of wire egress in append mode, on
top of tests/egress_cases.py (whose _m / runs_of / export they go through): one
group and one list of messages each, at n = 3, 5 and 7, and one n = 1 leader that
sends nothing.

T = the group's Term before the batch; the log is (1,1) (2,1) (3,T-1) (4,T)
("cur": it ends in the current-term run) or (1,1) (2,1) (3,T-2) ("old").  A
leader has won at T + 1 and holds its noop at 5, so the index just below its
current-term run is 4 and that index's term is T.  "fresh": every follower is
in Probe at Next = 5 (reset's value).  "repl": every follower has acked the
noop (Replicate, Match 5, Next 6, empty window, committed 5).

Every case states how many of its records are flagged HB_OUT_HOST.  That is 0
except where the name says why: FLAGGED below.
"""
from etcd_amd import abi
from oracle.pyoracle import Msg, Raft

from . import egress_cases as EC
from .egress_cases import _m

A = abi
SIZES = (3, 5, 7)
# the cases whose MsgApp records stay with the host, and why
FLAGGED = {
    "reject-below-boundary": "an aux = 0 send below the boundary: its LogTerm is in no event",
    "append-then-win": "a follower append earlier in the call: lastTerm, hence the boundary's term, is unknown",
}


def _rej(frm, term, index, hint):
    """A rejecting MsgAppResp (RejectHint travels in the batch's hint column)."""
    return dict(_m(A.HB_MSG_APP_RESP, frm, term, index, log_term=hint), reject=True)


def _acks(ids, term, index):
    return [_m(A.HB_MSG_APP_RESP, f, term, index) for f in ids]


def _case(name, n, role, ents, hard, msgs, setup=(), snapshot=None, flagged=0):
    return dict(name=f"{name}/{n}", role=role, peers=list(range(1, n + 1)), ents=ents, hard=hard, msgs=msgs,
                setup=tuple(setup), snapshot=snapshot, flagged=flagged)


def scenarios(sizes=SIZES):
    out = []
    for n in sizes:
        T = 4 + n
        cur = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        old = [(1, 1), (2, 1), (3, T - 2)]
        hard = (T, 0, 2)
        fol = list(range(2, n + 1))
        q = n // 2  # acks that, with the leader's own Match, make a quorum
        repl = [("step", m) for m in _acks(fol, T + 1, 5)]
        prop = lambda k=1: _m(A.HB_MSG_PROP, 1, nents=k)  # noqa: E731
        grants = [_m(A.HB_MSG_VOTE_RESP, f, T + 1) for f in fol[:q]]
        hup = _m(A.HB_MSG_HUP, 1)

        def add(name, role, ents, msgs, **kw):
            out.append(_case(name, n, role, ents, hard, msgs, **kw))
        # 1. the cfg2 step: a proposal, then every follower acks it.  The first broadcast carries
        #    entry 6; the ack that makes the quorum moves Commit and the second carries none
        add("cfg2", "leader", cur, [prop()] + _acks(fol, T + 1, 6), setup=repl)
        # 2. two proposals, a quorum acks 6, the other followers ack 7: Commit is 6 in the first
        #    broadcast after the acks and 7 in the second
        add("commit-moves", "leader", cur, [prop(), prop()] + _acks(fol[:q], T + 1, 6) + _acks(fol[q:2 * q], T + 1, 7),
            setup=repl)
        # 3. one MsgProp of three entries: entries (5, 8]
        add("prop-k", "leader", cur, [prop(3)], setup=repl)
        # 4. a rejection.  aux = 1: a Replicate follower rejects 6 (maybeDecrTo: Next = Match + 1 = 6,
        #    becomeProbe), the resend is at Index 5, the noop.  aux = 0 at the boundary: a Probe
        #    follower at Next 6 rejects 5 with hint 4 (Next = 5), the resend is at Index 4, whose
        #    term T is the boundary's.  Below the boundary (hint 2: Index 2, term 1): flagged
        add("reject-aux1", "leader", cur, [prop(), _rej(2, T + 1, 6, 5)], setup=repl)
        add("reject-at-boundary", "leader", cur, [_rej(2, T + 1, 5, 4)], setup=[("progress", 2, 0, 6)])
        add("reject-below-boundary", "leader", cur, [_rej(2, T + 1, 4, 2)], flagged=1)
        # 5. MsgHeartbeatResp from a follower behind the log: sendAppend.  Replicate: Next is past
        #    the log, an empty MsgApp at Index 6.  6. Probe: Index 4 with entry 5, which pauses the
        #    follower; its second MsgHeartbeatResp sends nothing
        add("heartbeat-resp", "leader", cur, [prop(), _m(A.HB_MSG_HEARTBEAT_RESP, 2, T + 1)], setup=repl)
        add("heartbeat-resp-paused", "leader", cur,
            [_m(A.HB_MSG_HEARTBEAT_RESP, 2, T + 1), _m(A.HB_MSG_HEARTBEAT_RESP, 2, T + 1)])
        # 7. a follower below firstIndex gets the snapshot (HB_EV_SNAP, no record); the next one a MsgApp
        add("needs-snapshot", "leader", [(3, T - 1), (4, T)],
            [_m(A.HB_MSG_HEARTBEAT_RESP, 2, T + 1), _m(A.HB_MSG_HEARTBEAT_RESP, 3, T + 1)],
            setup=[("progress", 2, 0, 1)], snapshot=(2, 1))
        # 8. an election won inside the call: the first bcastAppend is at the pre-noop last index,
        #    aux = 0, LogTerm from the boundary that HB_EV_TERM set (T, or T - 2 from the ring)
        add("win-cur", "follower", cur, [hup] + grants)
        add("win-old", "follower", old, [hup] + grants)
        # 11. a follower append, then Hup and the grants in one call
        add("append-then-win", "follower", cur, [_m(A.HB_MSG_APP, 2, T, 4, T, 3, ents=[T]), hup] + grants,
            flagged=n - 1)
        # 12. a leader stepped down by a higher term in mid-batch: its first broadcast, then the
        #     rejection of the MsgApp; the proposal and the acks after it send nothing
        add("stepdown", "leader", cur,
            [prop(), _m(A.HB_MSG_APP, 2, T + 3, 99, T + 3, 2), prop()] + _acks(fol, T + 1, 6), setup=repl)
        # 13. MsgHup to a leader faults the group: the broadcast before it, nothing after
        add("fault", "leader", cur, [prop(), hup, prop()], setup=repl)
    # n = 1: a leader alone commits at once and sends nothing
    out.append(_case("single-leader", 1, "leader", [(1, 1), (2, 3)], (3, 0, 2), [_m(A.HB_MSG_PROP, 1, nents=2)]))
    return out


def election_cases(sizes=SIZES):
    """Scenarios 8 / 9 / 10 alone: the two logs, Hup and the grants."""
    return [c for c in scenarios(sizes) if c["name"].split("/")[0] in ("win-cur", "win-old")]


def size_cases(sizes=SIZES):
    """Scenario 14: the cases that send both entry-carrying and empty MsgApps, for a handle
    with max_msg_size 0 or finite."""
    return [c for c in scenarios(sizes) if c["name"].split("/")[0] in ("cfg2", "prop-k", "commit-moves")]


def as_tuple(c):
    """The case in the format of tests/egress_cases.py."""
    return (c["name"], c["role"], c["peers"], c["ents"], c["hard"], c["msgs"])


def oracle_msg(m):
    if m.get("reject"):
        return Msg(m["type"], From=m["frm"], To=1, Term=m["term"], Index=m["index"], Reject=True,
                   RejectHint=m["log_term"])
    return EC.oracle_msg(m)


def build(c, max_msg_size=A.HB_NO_LIMIT):
    kw = {} if max_msg_size == A.HB_NO_LIMIT else dict(max_msg_size=max_msg_size)
    r = Raft(1, c["peers"], ents=c["ents"], snapshot=c["snapshot"], hard=c["hard"], **kw)
    if c["role"] != "follower":
        r.becomeCandidate()
        if c["role"] == "leader":
            r.becomeLeader()
    for op in c["setup"]:
        if op[0] == "step":
            r.Step(oracle_msg(op[1]))
        else:
            r.setProgress(*op[1:])
    assert not r.fault, c["name"]
    r.readMessages()
    return r


def export(rafts, cases):
    """EC.export plus the reject bit of the rejecting MsgAppResps (same round-robin order)."""
    groups, runs, peers, batch = EC.export(rafts, [as_tuple(c) for c in cases])
    i = 0
    for k in range(max(len(c["msgs"]) for c in cases)):
        for c in cases:
            if k >= len(c["msgs"]):
                continue
            if c["msgs"][k].get("reject"):
                batch["info"][i] |= 1 << 8
            i += 1
    assert i == len(batch["group"])
    return groups, runs, peers, batch
