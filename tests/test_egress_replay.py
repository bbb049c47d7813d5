"""The replay rules of wire egress pinned to the oracle's own r.msgs (CPU).

tests/egress_util.replay restates the rules of DESIGN.md §3.15 over a step's
events.  Here a few dozen oracle.pyoracle.Raft objects (followers with logs of
several terms, candidates, leaders: tests/egress_cases.py) are stepped twice
with the same messages: as Raft objects, whose readMessages() gives the full
messages the reference appended to r.msgs, and exported with to_group() into
an OracleGroups, whose step / tick gives the events.  The replay of the events
must equal the messages of the four payload-free types field for field: To,
From, Term, LogTerm, Index, Commit, Reject, RejectHint.
"""
import numpy as np

from etcd_amd import abi, synth
from oracle.pyoracle import OracleGroups

from . import egress_cases as EC
from .egress_util import EGRESS_TYPES, by_group, replay

DRAWS = np.arange(1, 64, dtype=np.uint64) * np.uint64(7919)


def _expected(g, r, n):
    """r.msgs of raft g, the four types, as egress_util records."""
    out = []
    for m in r.readMessages():
        if m.Type not in EGRESS_TYPES:
            continue
        slot = 1 <= m.To <= n
        out.append((g, m.Type, m.To - 1 if slot else abi.HB_REF_OTHER, m.To if slot else 0, m.From, m.Term, m.LogTerm,
                    m.Index, m.Commit, bool(m.Reject), m.RejectHint))
    return out


def _oracle_groups(rafts, scs):
    groups, runs, peers, batch = EC.export(rafts, scs)
    og = OracleGroups(groups, runs, 256)
    og.load_term_runs(synth.older_runs(og.groups(), runs))
    return og, peers, batch


def test_replay_of_step_events_equals_read_messages():
    scs = EC.scenarios()
    assert len(scs) >= 36
    rafts = [EC.build(sc) for sc in scs]
    og, peers, batch = _oracle_groups(rafts, scs)
    before = og.groups()
    ev, _ = og.step(batch)
    got = by_group(replay(ev, before, peers, 1))
    want = []
    for g, (r, sc) in enumerate(zip(rafts, scs)):
        for m in sc[5]:
            if r.fault:  # the reference panicked: nothing is stepped after it
                break
            r.Step(EC.oracle_msg(m))
        want += _expected(g, r, len(sc[2]))
    assert got == want
    # the scenarios reach every row of the table
    types = {(r[1], r[9]) for r in got}
    assert types >= {(abi.HB_MSG_APP_RESP, False), (abi.HB_MSG_APP_RESP, True), (abi.HB_MSG_HEARTBEAT_RESP, False),
                     (abi.HB_MSG_VOTE_RESP, False), (abi.HB_MSG_VOTE_RESP, True), (abi.HB_MSG_HEARTBEAT, False)}
    assert any(r[2] == abi.HB_REF_OTHER for r in got)
    assert {int(e["type"]) for e in ev} >= {abi.HB_EV_TERM, abi.HB_EV_LAST, abi.HB_EV_FOLLOW, abi.HB_EV_FAULT,
                                           abi.HB_EV_RESP, abi.HB_EV_HEARTBEAT, abi.HB_EV_APP}
    assert {int(e["aux"]) for e in ev if e["type"] == abi.HB_EV_FOLLOW} == \
        {abi.HB_FOLLOW_STEP, abi.HB_FOLLOW_APPEND, abi.HB_FOLLOW_RESTORE}
    # a response's Term differs from the Term before the step, and from the one after it
    after = og.groups()
    assert any(r[5] != int(before[r[0]]["term"]) for r in got)
    assert any(r[5] != int(after[r[0]]["term"]) for r in got)
    assert any(r[9] and r[10] != int(before[r[0]]["last_index"]) for r in got)


def test_replay_of_tick_events_equals_read_messages():
    scs = EC.scenarios()
    rafts = []
    for sc in scs:
        r = EC.build(sc)
        r.draws = DRAWS
        rafts.append(r)
    og, peers, _ = _oracle_groups(rafts, scs)
    timers = np.zeros(len(scs), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"] = 10, 1
    og.load_timers(timers)
    before = og.groups()
    ev, _ = og.tick(DRAWS)
    got = by_group(replay(ev, before, peers, 1))
    want = []
    for g, (r, sc) in enumerate(zip(rafts, scs)):
        r.tick()
        want += _expected(g, r, len(sc[2]))
    assert got == want
    leaders = sum(sc[1] == "leader" for sc in scs)
    assert leaders and len(got) == sum((len(sc[2]) - 1) for sc in scs if sc[1] == "leader")
    assert all(r[1] == abi.HB_MSG_HEARTBEAT for r in got)
