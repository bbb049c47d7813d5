"""The replay rule of the forward record pinned to the oracle's own r.msgs (CPU).

tests/props_util.replay_forwards restates what hb_egress makes of an HB_EV_PROP_FWD event with
HB_WIRE_PROPS_OUT on.  As tests/test_egress_replay.py does, the scenarios of
tests/wire_props_cases.py (followers with a lead inside and outside prs, without a lead,
candidates, leaders) are stepped twice with the same messages: as oracle.pyoracle.Raft
objects, whose readMessages() gives the messages the reference appended to r.msgs, and as an
OracleGroups, whose step gives the events.  The replay must equal the messages of type MsgProp
field for field (To = the lead, From, Term 0 and the rest 0), and the proposal its hint names
must carry the message's entry count.
"""
from etcd_amd import abi
from oracle.pyoracle import OracleGroups

from . import egress_cases as EC
from . import wire_props_cases as PC
from .egress_util import by_group, replay
from .props_util import merge_forwards, replay_forwards


def _expected(g, r, n):
    """r.msgs of raft g, type MsgProp, as egress_util records with the entry count in place of the hint."""
    out = []
    for m in r.readMessages():
        if m.Type != abi.HB_MSG_PROP:
            continue
        slot = 1 <= m.To <= n
        assert m.RejectHint == 0
        out.append((g, m.Type, m.To - 1 if slot else abi.HB_REF_OTHER, m.To if slot else 0, m.From, m.Term, m.LogTerm,
                    m.Index, m.Commit, bool(m.Reject), int(m.nents)))
    return out


def test_replay_of_forward_events_equals_read_messages():
    scs = PC.scenarios()
    rafts = [EC.build(sc) for sc in scs]
    groups, runs, peers, batch = EC.export(rafts, scs)
    og = OracleGroups(groups, runs, 256)
    before = og.groups()
    ev, _ = og.step(batch)
    fwd = replay_forwards(ev, peers, 1)
    got = by_group([r for _, r in fwd])
    want = []
    for g, (r, sc) in enumerate(zip(rafts, scs)):
        for m in sc[5]:
            if r.fault:  # the reference panicked: nothing is stepped after it
                break
            r.Step(EC.oracle_msg(m))
        want += _expected(g, r, len(sc[2]))
    # hint = the arrival index of the proposal in the stepped batch: that record's entry count
    assert all(int(batch["group"][r[10]]) == r[0] and (int(batch["info"][r[10]]) & 0xF) == abi.HB_MSG_PROP for r in got)
    assert [r[:10] + (int(batch["index"][r[10]]),) for r in got] == want
    assert all(r[5:10] == (0, 0, 0, 0, False) and r[4] == 1 for r in got)
    # the scenarios reach the rule's rows: a lead inside and outside prs, two leads in one step, the
    # drops (no lead, candidate), nothing after a fault, a leader that appends instead
    assert any(r[2] == abi.HB_REF_OTHER and r[3] == 0 for r in got)
    assert {r[3] for r in got} >= {0, 2, 3}
    per = {g: [r[3] for r in got if r[0] == g] for g in range(len(scs))}
    name = [sc[0] for sc in scs]
    assert per[name.index("two-leads/0")] == [2, 3] and per[name.index("no-lead/1")] == []
    assert len(per[name.index("fault-then-prop/2")]) == 1 and len(per[name.index("candidate/0")]) == 1
    assert len(per[name.index("vote-clears-lead/0")]) == 1 and len(per[name.index("leader-steps-down/1")]) == 1
    types = {int(e["type"]) for e in ev}
    assert types >= {abi.HB_EV_PROP_FWD, abi.HB_EV_PROP_DROP, abi.HB_EV_LAST, abi.HB_EV_FAULT, abi.HB_EV_RESP}
    # merged with the payload-free records, a group's records keep the order of r.msgs
    plain = lambda e: [r + (False, False) for r in replay(e, before, peers, 1)]  # noqa: E731
    merged = merge_forwards(ev, plain, peers, 1)
    assert [r for r in merged if r[1] != abi.HB_MSG_PROP] == by_group(plain(ev))
    assert [r[:11] for r in merged if r[1] == abi.HB_MSG_PROP] == got
    g = name.index("two-leads/0")
    assert [r[1] for r in merged if r[0] == g] == [abi.HB_MSG_APP_RESP, abi.HB_MSG_PROP, abi.HB_MSG_HEARTBEAT_RESP,
                                                   abi.HB_MSG_PROP, abi.HB_MSG_APP_RESP]
