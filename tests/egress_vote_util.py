"""The replay rules of wire egress in vote mode, restated in Python.

replay_votes() is egress_util.replay plus campaign's MsgVote: every HB_EV_VOTE
event becomes a record whose LogTerm is raftLog.lastTerm() at the send, carried
forward from last_term() of the group's record before the step:

  HB_EV_LAST                        lt = the Term of that point (the group's own entries)
  HB_EV_FOLLOW, APPEND / RESTORE    lt = unknown until the next HB_EV_LAST
  HB_EV_VOTE                        MsgVote{Term, Index = x, LogTerm = lt}

A vote whose lt is unknown is still a record: flagged (HB_OUT_HOST, the last
field of the tuple), log_term 0, no bytes.  tests/test_egress_vote_replay.py
pins these rules to the oracle's own r.msgs; tests/test_egress_vote_gpu.py uses
them as the reference of hb_egress in vote mode.
"""
import numpy as np

from etcd_amd import abi

from .egress_util import FIELDS, replay

UNKNOWN = None  # the device's HB_LT_UNKNOWN
VOTE_FIELDS = FIELDS + ("host",)


def last_term(group_record, runs):
    """The snapshot value of a group: Term when last_index lies in the current-term run,
    else the term of the newest of `runs` (the older runs the device holds, [(start, term)]
    oldest first; None or empty: never loaded) starting at or below it, else UNKNOWN."""
    last, tf = int(group_record["last_index"]), int(group_record["term_first"])
    if tf != abi.HB_NO_INDEX and last >= tf:
        return int(group_record["term"])
    lt = UNKNOWN
    for start, t in (runs or ()):
        if int(start) <= last:
            lt = int(t)
    return lt


def oracle_older_runs(og):
    """{group: the older runs the device's ring holds at this point}, from the oracle: the runs
    of its log below the current-term run, from the oldest start the engine's log index knows
    (tw_lo, which the oracle keeps for HB_FAULT_TERM_WINDOW; HB_NO_INDEX: none was loaded)."""
    groups = og.groups()
    out = {}
    for g in range(len(groups)):
        r = og.raft(g)
        tf, lo = int(groups[g]["term_first"]), int(r.tw_lo)
        out[g] = [(int(r.log.runs[k].index), int(r.log.runs[k].term)) for k in range(r.log.nruns)
                  if (tf == abi.HB_NO_INDEX or int(r.log.runs[k].index) < tf) and lo != abi.HB_NO_INDEX
                  and int(r.log.runs[k].index) >= lo]
    return out


def replay_votes(events, groups0, runs, peers, self_id):
    """events, groups0, peers, self_id as egress_util.replay; runs[g] = group g's older runs
    (last_term).  Returns tuples of VOTE_FIELDS in event order."""
    state = {}
    out = []
    for x, g, t, to, aux in np.asarray(events).tolist():  # (abi.EVENT_DTYPE's field order)
        s = state.get(g)
        if s is None:
            rr = runs.get(g) if isinstance(runs, dict) else runs[g]
            s = state[g] = [int(groups0[g]["term"]), int(groups0[g]["last_index"]), False, False,
                            last_term(groups0[g], rr)]
        if s[3]:  # faulted: the replay ended
            continue
        if t == abi.HB_EV_TERM:
            s[0] = x
        elif t == abi.HB_EV_LAST:
            s[1] = x
            s[4] = s[0]
        elif t == abi.HB_EV_FOLLOW:
            if aux in (abi.HB_FOLLOW_APPEND, abi.HB_FOLLOW_RESTORE):
                s[2] = True
                s[4] = UNKNOWN
        elif t == abi.HB_EV_FAULT:
            s[3] = True
        elif t == abi.HB_EV_VOTE:
            assert to <= abi.HB_REF_SLOT_MAX
            host = s[4] is UNKNOWN
            out.append((g, abi.HB_MSG_VOTE, to, int(peers[g][to]), self_id, s[0], 0 if host else s[4], x, 0, False, 0,
                        host))
        elif t in (abi.HB_EV_RESP, abi.HB_EV_HEARTBEAT):
            slot = to <= abi.HB_REF_SLOT_MAX
            to_ref = to if slot else abi.HB_REF_OTHER
            to_id = int(peers[g][to]) if slot else 0
            mtype, index, commit, reject, hint = abi.HB_MSG_HEARTBEAT, 0, 0, False, 0
            if t == abi.HB_EV_HEARTBEAT:
                commit = x
            else:
                kind = aux & 7
                reject = bool(aux & abi.HB_RESP_REJECT)
                mtype = {abi.HB_RESP_APP: abi.HB_MSG_APP_RESP, abi.HB_RESP_HEARTBEAT: abi.HB_MSG_HEARTBEAT_RESP,
                         abi.HB_RESP_VOTE: abi.HB_MSG_VOTE_RESP}[kind]
                if kind == abi.HB_RESP_APP:
                    index = x
                    if reject:
                        hint = s[1]
                    elif s[2]:
                        s[1], s[2] = x, False
            out.append((g, mtype, to_ref, to_id, self_id, s[0], 0, index, commit, reject, hint, False))
    # without the votes these are the rules of egress_util.replay, record for record
    assert [r[:-1] for r in out if r[1] != abi.HB_MSG_VOTE] == replay(events, groups0, peers, self_id)
    assert not any(r[-1] for r in out if r[1] != abi.HB_MSG_VOTE)
    return out


def is_vote(rec):
    return rec[1] == abi.HB_MSG_VOTE


def marshal(rec):
    """The wire bytes of one record (b'' for HB_REF_OTHER and for a flagged vote: the host sends it)."""
    from .wire_util import gogo_marshal
    g, mtype, to_ref, to, frm, term, log_term, index, commit, reject, hint, host = rec
    if to_ref == abi.HB_REF_OTHER or host:
        return b""
    return gogo_marshal(mtype, to=to, frm=frm, term=term, log_term=log_term, index=index, commit=commit,
                        reject=reject, hint=hint)


def out_arrays(records):
    """The hb_out_batch arrays of a list of records (numpy, abi.OUT_BATCH_FIELDS)."""
    n = len(records)
    a = {name: np.zeros(n, dtype=dt) for name, dt in abi.OUT_BATCH_FIELDS}
    for i, (g, mtype, to_ref, to, frm, term, log_term, index, commit, reject, hint, host) in enumerate(records):
        a["group"][i] = g
        a["info"][i] = abi.hb_info(mtype, to_ref, reject) | (abi.HB_OUT_HOST if host else 0)
        a["to"][i], a["term"][i], a["log_term"][i] = to, term, log_term
        a["index"][i], a["commit"][i], a["hint"][i] = index, commit, hint
    return a
