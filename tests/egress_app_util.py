"""The replay rules of wire egress in append mode, restated in Python.

replay_apps() is egress_vote_util.replay_votes plus sendAppend's MsgApp: every
HB_EV_APP event becomes a record.  Next to (term, last, pend, lt) a group carries

  cm        raftLog.committed        the pre-step column, then each HB_EV_COMMIT;
                                     unknown from a follower append / restore
                                     until the next HB_EV_COMMIT
  bl, blt   the index just below the current-term run and its term
                                     the pre-step pair (boundary()); HB_EV_TERM
                                     sets them to (last, lt); a follower append /
                                     restore makes them unknown

  HB_EV_APP (to, x, aux)   MsgApp{Term, Index = x, Commit = cm, LogTerm}
      aux = 1: LogTerm = Term;  aux = 0, x == bl, blt known: LogTerm = blt;
      entries (x, L] when x < last: L = last (max_msg_size HB_NO_LIMIT), x + 1
      (max_msg_size 0); the record then carries HB_OUT_ENTS and hint = L.

Anything the replay cannot prove (the LogTerm otherwise, cm unknown, entries
under a finite max_msg_size) flags the record: HB_OUT_HOST, log_term = commit =
hint = 0, no bytes.  tests/test_egress_app_replay.py pins these rules to the
oracle's own r.msgs; tests/test_egress_app_gpu.py uses them as the reference of
hb_egress in append mode.
"""
import numpy as np

from etcd_amd import abi

from .egress_util import replay
from .egress_vote_util import UNKNOWN, VOTE_FIELDS, last_term, replay_votes

APP_FIELDS = VOTE_FIELDS + ("ents",)


def boundary(group_record, runs):
    """The snapshot's boundary pair of a group: (bl, blt).  bl = term_first - 1, or
    last_index when the current-term run is empty; blt = its term from `runs` (the older
    runs the device holds), UNKNOWN when they do not reach or bl lies below the log."""
    last, tf = int(group_record["last_index"]), int(group_record["term_first"])
    if tf == abi.HB_NO_INDEX:
        return last, last_term(group_record, runs)
    bl = tf - 1
    blt = UNKNOWN
    if bl >= 0 and bl + 1 >= int(group_record["first_index"]):
        for start, t in (runs or ()):
            if int(start) <= bl:
                blt = int(t)
    return (bl if bl >= 0 else UNKNOWN), blt


def replay_apps(events, groups0, runs, peers, self_id, max_msg_size=abi.HB_NO_LIMIT, votes=True):
    """events, groups0, runs, peers, self_id as egress_vote_util.replay_votes.  Returns
    tuples of APP_FIELDS in event order; votes=False leaves the MsgVote records out (mode 5)."""
    state = {}
    out = []
    for x, g, t, to, aux in np.asarray(events).tolist():  # (abi.EVENT_DTYPE's field order)
        s = state.get(g)
        if s is None:
            rr = runs.get(g) if isinstance(runs, dict) else runs[g]
            bl, blt = boundary(groups0[g], rr)
            s = state[g] = dict(term=int(groups0[g]["term"]), last=int(groups0[g]["last_index"]), pend=False,
                                dead=False, lt=last_term(groups0[g], rr), cm=int(groups0[g]["committed"]), bl=bl,
                                blt=blt)
        if s["dead"]:  # faulted: the replay ended
            continue
        if t == abi.HB_EV_TERM:
            s["term"] = x
            s["bl"], s["blt"] = (UNKNOWN if s["pend"] else s["last"]), s["lt"]
        elif t == abi.HB_EV_COMMIT:
            s["cm"] = x
        elif t == abi.HB_EV_LAST:
            s["last"] = x
            s["lt"] = s["term"]
        elif t == abi.HB_EV_FOLLOW:
            if aux in (abi.HB_FOLLOW_APPEND, abi.HB_FOLLOW_RESTORE):
                s["pend"] = True
                s["lt"] = s["cm"] = s["bl"] = s["blt"] = UNKNOWN
        elif t == abi.HB_EV_FAULT:
            s["dead"] = True
        elif t == abi.HB_EV_APP:
            assert to <= abi.HB_REF_SLOT_MAX
            at_bl = s["bl"] is not UNKNOWN and x == s["bl"] and s["blt"] is not UNKNOWN
            host = not ((aux & 1) or at_bl) or s["cm"] is UNKNOWN
            lterm = s["term"] if aux & 1 else s["blt"]
            ents = x < s["last"]
            L = 0
            if ents:
                if max_msg_size == abi.HB_NO_LIMIT:
                    L = s["last"]
                elif max_msg_size == 0:
                    L = x + 1
                else:
                    host = True
            if host:
                out.append((g, abi.HB_MSG_APP, to, int(peers[g][to]), self_id, s["term"], 0, x, 0, False, 0, True, False))
            else:
                out.append((g, abi.HB_MSG_APP, to, int(peers[g][to]), self_id, s["term"], lterm, x, s["cm"], False, L,
                            False, ents))
        elif t == abi.HB_EV_VOTE:
            if votes:
                host = s["lt"] is UNKNOWN
                out.append((g, abi.HB_MSG_VOTE, to, int(peers[g][to]), self_id, s["term"], 0 if host else s["lt"], x, 0,
                            False, 0, host, False))
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
                        hint = s["last"]
                    elif s["pend"]:
                        s["last"], s["pend"] = x, False
            out.append((g, mtype, to_ref, to_id, self_id, s["term"], 0, index, commit, reject, hint, False, False))
    # without the append records these are the rules of replay_votes (mode 3) / replay (mode 1)
    rest = [r[:-1] for r in out if not is_app(r)]
    assert not any(r[-1] for r in out if not is_app(r))
    if votes:
        assert rest == replay_votes(events, groups0, runs, peers, self_id)
    else:
        assert [r[:-1] for r in rest] == replay(events, groups0, peers, self_id) and not any(r[-1] for r in rest)
    return out


def is_app(rec):
    return rec[1] == abi.HB_MSG_APP


def entry_tuple(group, index, term):
    """The entry the tests splice in for entry `index` of `group`, as wire_util.gogo_marshal
    takes it: (type, term, index, data), the payload a function of group and index, 0 to 4
    bytes long (Data = nil for a length of 0)."""
    n = (group + index) % 5
    return (0, term, index, bytes((group + index + k) & 0xFF for k in range(n)) if n else None)


def entry_bytes(group, index, term):
    """That entry marshalled (Entry.MarshalTo)."""
    from .wire_util import _entry
    return _entry(entry_tuple(group, index, term))


def marshal(rec):
    """The bytes hb_encode writes for one record: b'' for HB_REF_OTHER and a flagged record;
    the entry-free message (Reject = 0, RejectHint = 0) for one with entries."""
    from .wire_util import gogo_marshal
    g, mtype, to_ref, to, frm, term, log_term, index, commit, reject, hint, host, ents = rec
    if to_ref == abi.HB_REF_OTHER or host:
        return b""
    return gogo_marshal(mtype, to=to, frm=frm, term=term, log_term=log_term, index=index, commit=commit,
                        reject=reject, hint=0 if ents else hint)


def prefix_len(rec):
    """Fields 1-6 of the record's message."""
    from etcd_amd.splice import varint
    g, mtype, to_ref, to, frm, term, log_term, index = rec[:8]
    return 6 + sum(len(varint(v)) for v in (mtype, to, frm, term, log_term, index))


def status_of(rec):
    if rec[2] == abi.HB_REF_OTHER or rec[11]:
        return abi.HB_WIRE_HOST
    return (abi.HB_WIRE_SPLICE | prefix_len(rec)) if rec[12] else abi.HB_WIRE_OK


def out_arrays(records):
    """The hb_out_batch arrays of a list of records (numpy, abi.OUT_BATCH_FIELDS)."""
    n = len(records)
    a = {name: np.zeros(n, dtype=dt) for name, dt in abi.OUT_BATCH_FIELDS}
    for i, (g, mtype, to_ref, to, frm, term, log_term, index, commit, reject, hint, host, ents) in enumerate(records):
        a["group"][i] = g
        a["info"][i] = (abi.hb_info(mtype, to_ref, reject) | (abi.HB_OUT_HOST if host else 0) |
                        (abi.HB_OUT_ENTS if ents else 0))
        a["to"][i], a["term"][i], a["log_term"][i] = to, term, log_term
        a["index"][i], a["commit"][i], a["hint"][i] = index, commit, hint
    return a
