"""Hand-built scenarios of forwarded proposals, in the format of
tests/egress_cases.py (whose build / export / oracle_msg turn them into oracle.pyoracle.Raft
objects, group records and one batch): followers with a lead inside and outside prs, followers
without a lead, candidates and leaders, each stepped with MsgProp messages."""
from etcd_amd import abi

from .egress_cases import _m

A = abi


def scenarios():
    """[(name, role, peers, ents, hard, messages)]; T = the group's Term before the batch."""
    out = []
    for v in range(3):
        T = 3 + 2 * v
        peers = [1, 2, 3] if v != 1 else [1, 2, 3, 4, 5]
        ents = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        hard = (T, 0, 2)
        F = lambda name, msgs: out.append((f"{name}/{v}", "follower", peers, ents, hard, msgs))  # noqa: E731
        P = lambda n, frm=1: _m(A.HB_MSG_PROP, frm, nents=n)  # noqa: E731
        # a heartbeat names the lead, then two proposals (one from another node): two forwards
        F("lead-then-forwards", [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=3), P(2), P(1, 3)])
        # no lead yet: dropped; then the lead is known: forwarded
        F("drop-then-forward", [P(1), _m(A.HB_MSG_HEARTBEAT, 3, T, commit=2), P(3)])
        # a lead outside prs: HB_REF_OTHER
        F("outsider-lead", [_m(A.HB_MSG_HEARTBEAT, 9, T, commit=2), P(1), P(2)])
        # the lead changes with the term between two forwards; a response lies between them
        F("two-leads", [_m(A.HB_MSG_APP, 2, T, 4, T, 3, ents=[T]), P(1), _m(A.HB_MSG_HEARTBEAT, 3, T + 1, commit=3),
                        P(2), _m(A.HB_MSG_APP, 3, T + 1, 9, T, 2)])
        # a vote granted at a higher term clears the lead: the proposal after it is dropped
        F("vote-clears-lead", [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=3), P(1), _m(A.HB_MSG_VOTE, 3, T + 1, 4, T), P(1)])
        # a group that faults mid-batch forwards nothing after it
        F("fault-then-prop", [_m(A.HB_MSG_HEARTBEAT, 2, T, commit=3), P(1), _m(A.HB_MSG_HEARTBEAT, 2, T, commit=100),
                              P(1)])
        # without a lead at all
        F("no-lead", [P(1), P(2)])
        # a candidate drops proposals; the leader's heartbeat makes it a follower that forwards
        out.append((f"candidate/{v}", "candidate", peers, ents, hard,
                    [P(1), _m(A.HB_MSG_HEARTBEAT, 3, T + 1, commit=2), P(2)]))
        # a leader appends its own, steps down on a higher-term heartbeat and forwards the next
        out.append((f"leader-steps-down/{v}", "leader", peers, ents, hard,
                    [P(2), _m(A.HB_MSG_HEARTBEAT, 2, T + 2, commit=2), P(1)]))
    return out
