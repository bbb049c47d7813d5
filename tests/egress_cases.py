"""Hand-built scenarios of wire egress, one batch per group, for both the CPU
pin of the replay rules (tests/test_egress_replay.py: the oracle's own r.msgs)
and the device (tests/test_egress_gpu.py).  Together they cover every row of
the replay table in DESIGN.md §3.15.

A scenario is a role (follower, candidate, leader), a log of several terms and
a list of messages; build() makes the oracle.pyoracle.Raft of each, and
export() turns those into the group records, log term runs and one batch in
the engine's format (the rafts' ids are slot + 1, the oracle's)."""
import numpy as np

from etcd_amd import abi
from oracle.pyoracle import Msg, Raft

A = abi


def _m(type, frm, term=0, index=0, log_term=0, commit=0, ents=(), snap=None, nents=0):
    return dict(type=type, frm=frm, term=term, index=index, log_term=log_term, commit=commit, ents=tuple(ents),
                snap=snap, nents=nents)


def scenarios():
    """[(name, role, peers, ents, hard, messages)]; T = the group's Term before the batch."""
    out = []
    for v in range(3):
        T = 3 + 2 * v
        peers = [1, 2, 3] if v != 1 else [1, 2, 3, 4, 5]
        ents = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        hard = (T, 0, 2)
        F = lambda name, msgs: out.append((f"{name}/{v}", "follower", peers, ents, hard, msgs))  # noqa: E731
        # MsgApp at T, then MsgVote at T + 1: the two responses carry different Terms
        F("app-then-vote", [_m(A.HB_MSG_APP, 2, T, 4, T, 3, ents=[T]), _m(A.HB_MSG_VOTE, 3, T + 1, 5, T)])
        # an appending MsgApp, then a rejected one: RejectHint is the new last
        F("append-then-reject", [_m(A.HB_MSG_APP, 2, T, 4, T, 2, ents=[T, T]), _m(A.HB_MSG_APP, 2, T, 9, T, 2)])
        # an append that truncates a conflicting suffix, then a reject
        F("conflict-then-reject", [_m(A.HB_MSG_APP, 2, T + 1, 3, T - 1, 2, ents=[T + 1]),
                                   _m(A.HB_MSG_APP, 2, T + 1, 9, T, 2)])
        # a rejected MsgApp alone: RejectHint = the lastIndex before the step
        F("reject-alone", [_m(A.HB_MSG_APP, 3, T, 9, T, 2)])
        # MsgSnap that restores, then a reject: RejectHint = the snapshot's index
        F("restore-then-reject", [_m(A.HB_MSG_SNAP, 2, T, snap=(10 + v, T)), _m(A.HB_MSG_APP, 2, T, 20, T, 2)])
        # a MsgSnap the log already covers (no restore: the response names committed)
        F("snap-ignored", [_m(A.HB_MSG_SNAP, 2, T, snap=(2, 1)), _m(A.HB_MSG_APP, 2, T, 9, T, 2)])
        # MsgVote from a sender outside prs between two heartbeats: HB_REF_OTHER
        F("vote-outsider", [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=3), _m(A.HB_MSG_VOTE, 9, T + 1, 4, T),
                            _m(A.HB_MSG_HEARTBEAT, 2, T + 1, commit=4)])
        # a group that faults mid-batch (commitTo past lastIndex, raft/log.go:175-177)
        F("fault-mid-batch", [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=3), _m(A.HB_MSG_HEARTBEAT, 2, T, commit=100),
                              _m(A.HB_MSG_HEARTBEAT, 2, T, commit=4)])
        # votes: granted, then refused (already voted), a stale one ignored
        F("votes", [_m(A.HB_MSG_VOTE, 2, T + 1, 4, T), _m(A.HB_MSG_VOTE, 3, T + 1, 4, T),
                    _m(A.HB_MSG_VOTE, 3, T - 1, 4, T), _m(A.HB_MSG_VOTE, 3, T + 2, 1, 1)])
        # heartbeat and a MsgApp that only moves the commit
        F("heartbeat-and-commit", [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=4), _m(A.HB_MSG_APP, 2, T, 4, T, 4)])
        # a candidate (Term T + 1): a vote request refused, then the leader's heartbeat
        out.append((f"candidate/{v}", "candidate", peers, ents, hard,
                    [_m(A.HB_MSG_VOTE, 2, T + 1, 4, T), _m(A.HB_MSG_HEARTBEAT, 3, T + 1, commit=2),
                     _m(A.HB_MSG_APP, 3, T + 1, 4, T, 3, ents=[T + 1])]))
        # a leader (Term T + 1, noop at 5) appends a proposal (HB_EV_LAST), steps down on a
        # higher-term MsgApp and rejects it: RejectHint = the last it appended itself
        out.append((f"leader-steps-down/{v}", "leader", peers, ents, hard,
                    [_m(A.HB_MSG_PROP, 1, nents=2), _m(A.HB_MSG_APP, 2, T + 2, 99, T + 1, 2)]))
        # a leader beats (MsgBeat through hb_step): MsgHeartbeat to every peer
        out.append((f"leader-beats/{v}", "leader", peers, ents, hard,
                    [_m(A.HB_MSG_BEAT, 1), _m(A.HB_MSG_PROP, 1, nents=1), _m(A.HB_MSG_BEAT, 1)]))
    return out


def build(sc):
    name, role, peers, ents, hard, msgs = sc
    r = Raft(1, peers, ents=ents, hard=hard)
    if role != "follower":
        r.becomeCandidate()
        if role == "leader":
            r.becomeLeader()
        r.readMessages()
    return r


def oracle_msg(m):
    if m["type"] == A.HB_MSG_PROP:
        return Msg(A.HB_MSG_PROP, From=m["frm"], To=1, Entries=m["nents"])
    if m["type"] == A.HB_MSG_SNAP:
        return Msg(A.HB_MSG_SNAP, From=m["frm"], To=1, Term=m["term"], Snapshot=m["snap"])
    return Msg(m["type"], From=m["frm"], To=1, Term=m["term"], Index=m["index"], LogTerm=m["log_term"],
               Commit=m["commit"], Entries=[(m["index"] + 1 + k, t) for k, t in enumerate(m["ents"])]
               if m["type"] == A.HB_MSG_APP else 0)


def runs_of(r):
    """The log's term runs [(start index, term)] from firstIndex - 1."""
    out, prev = [], None
    for i in range(r.firstIndex - 1, r.lastIndex + 1):
        t = r.term(i)
        if t != prev:
            out.append((i, t))
            prev = t
    return out


def export(rafts, scs):
    """(groups GROUP_DTYPE, runs, peers [G, 7], batch) of the scenarios' rafts."""
    G = len(rafts)
    groups = np.zeros(G, dtype=A.GROUP_DTYPE)
    runs = []
    peers = np.zeros((G, A.HB_MAX_REPLICAS), np.uint64)
    for g, r in enumerate(rafts):
        groups[g] = np.frombuffer(bytes(r.to_group()), dtype=A.GROUP_DTYPE)[0]
        runs.append(runs_of(r))
        ids = [r.r.ids[i] for i in range(r.r.n)]
        assert ids == list(range(1, len(ids) + 1))
        peers[g, :len(ids)] = ids
    grp, info, term, index, hint, commit, eoff, eterm = [], [], [], [], [], [], [], []
    # round-robin over the groups: the batch interleaves them, each group's messages in order
    depth = max(len(sc[5]) for sc in scs)
    for k in range(depth):
        for g, sc in enumerate(scs):
            if k >= len(sc[5]):
                continue
            m = sc[5][k]
            n = int(groups[g]["n"])
            slot = m["frm"] - 1 if 1 <= m["frm"] <= n else A.HB_SLOT_NONE
            grp.append(g)
            info.append(A.hb_info(m["type"], slot))
            term.append(m["term"])
            eoff.append(len(eterm))
            commit.append(m["commit"])
            if m["type"] == A.HB_MSG_PROP:
                index.append(m["nents"])
                hint.append(0)
            elif m["type"] == A.HB_MSG_SNAP:
                index.append(m["snap"][0])
                hint.append(m["snap"][1])
            else:
                index.append(m["index"])
                hint.append(m["log_term"])
                eterm.extend(m["ents"])
    batch = dict(group=np.array(grp, np.uint32), info=np.array(info, np.uint32), term=np.array(term, np.uint64),
                 index=np.array(index, np.uint64), hint=np.array(hint, np.uint64), commit=np.array(commit, np.uint64),
                 eoff=np.array(eoff, np.uint64), eterm=np.array(eterm, np.uint64), props=None, msg_props=True)
    return groups, runs, peers, batch
