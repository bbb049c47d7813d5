"""Hand-built campaign scenarios of wire egress in vote mode,
in the format of tests/egress_cases.py (whose _m / build / export / oracle_msg
they go through): one group and one list of messages each, at n = 2 (the
single HB_EV_VOTE word), 3, 5 and 7 (the EVC_VBCAST word), and one n = 1 group
that wins at once and sends nothing.

T = the group's Term before the batch.  "cur" logs end in the current-term run
(lastTerm = T); "old" logs end two terms below it, so the LogTerm comes from
the term-run ring and differs from the vote's Term - 1.
"""
from etcd_amd import abi

from .egress_cases import _m

A = abi
FLAGGED = ("append-then-hup", "restore-then-hup")  # the scenarios whose votes stay with the host
SIZES = (2, 3, 5, 7)


def _hup():
    return _m(A.HB_MSG_HUP, 1)


def scenarios(sizes=SIZES):
    """[(name, role, peers, ents, hard, messages)]"""
    out = []
    for n in sizes:
        T = 4 + n
        peers = list(range(1, n + 1))
        cur = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        old = [(1, 1), (2, 1), (3, T - 2)]
        hard = (T, 0, 2)
        grants = [_m(A.HB_MSG_VOTE_RESP, 2 + k, T + 1) for k in range(n // 2)]  # with its own vote: a quorum

        def add(name, role, ents, msgs):
            out.append((f"{name}/{n}", role, peers, ents, hard, msgs))
        # the last index lies in an older run: LogTerm T - 2 from the ring, Term T + 1
        add("hup-old-run", "follower", old, [_hup()])
        # the last index lies in the current-term run: LogTerm T
        add("hup-cur-run", "follower", cur, [_hup()])
        # a candidate (Term T + 1) campaigns again; a follower campaigns twice in one batch
        add("candidate-hup", "candidate", cur, [_hup()])
        add("hup-twice", "follower", old, [_hup(), _hup()])
        # MsgHup, then a higher-term MsgApp that truncates below the voted index 4 and appends
        # 3 and 4 at T + 2: the vote carries T, the log after the step says T + 2
        add("hup-then-truncate", "follower", cur, [_hup(), _m(A.HB_MSG_APP, 2, T + 2, 2, 1, 2, ents=[T + 2, T + 2])])
        # Hup, win (noop at 5, Term T + 1), step down on a rejected MsgApp of Term T + 3, Hup
        # again: the second votes' LogTerm is the noop's T + 1, their Term T + 4
        add("win-stepdown-hup", "follower", cur,
            [_hup()] + grants + [_m(A.HB_MSG_APP, 2, T + 3, 99, T + 3, 2), _hup()])
        # an appending MsgApp, then MsgHup: the appended entry's term is not in the events
        add("append-then-hup", "follower", cur, [_m(A.HB_MSG_APP, 2, T, 4, T, 3, ents=[T]), _hup()])
        # a restoring MsgSnap, then MsgHup
        add("restore-then-hup", "follower", cur, [_m(A.HB_MSG_SNAP, 2, T, snap=(10 + n, T)), _hup()])
        # a leader that gets MsgHup faults: its heartbeats before it, nothing after
        add("leader-hup", "leader", cur, [_m(A.HB_MSG_BEAT, 1), _hup(), _m(A.HB_MSG_BEAT, 1)])
        # a heartbeat, a MsgVote from outside prs (HB_REF_OTHER response), then MsgHup
        add("outsider-then-hup", "follower", cur,
            [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=3), _m(A.HB_MSG_VOTE, 9, T + 1, 4, T), _hup()])
    # n = 1: the campaign wins at once, no MsgVote
    out.append(("single/1", "follower", [1], [(1, 1), (2, 3)], (3, 0, 2), [_hup()]))
    return out
