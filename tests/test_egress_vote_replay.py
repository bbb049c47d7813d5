"""The vote-mode replay rules pinned to the oracle's own r.msgs (CPU).

As tests/test_egress_replay.py, with campaign's MsgVote: the scenarios of
tests/egress_vote_cases.py and tests/egress_cases.py are stepped (and ticked,
every non-leader's election timeout firing) twice, as oracle.pyoracle.Raft
objects, whose readMessages() gives the messages the reference appended to
r.msgs, and as an OracleGroups, whose events tests/egress_vote_util.replay_votes
replays.  Every record, MsgVote included, must equal the oracle's message field
for field (To, From, Term, LogTerm, Index, Commit, Reject, RejectHint); a
flagged vote (LogTerm left to the host) must still match in To, Term and Index.
"""
import numpy as np

from etcd_amd import abi, synth
from oracle.pyoracle import OracleGroups

from . import egress_cases as EC
from . import egress_vote_cases as VC
from .egress_util import EGRESS_TYPES, by_group
from .egress_vote_util import is_vote, last_term, oracle_older_runs, replay_votes

DRAWS = np.arange(1, 64, dtype=np.uint64) * np.uint64(7919)
TYPES = EGRESS_TYPES + (abi.HB_MSG_VOTE,)


def _expected(g, r, n):
    out = []
    for m in r.readMessages():
        if m.Type not in TYPES:
            continue
        slot = 1 <= m.To <= n
        out.append((g, m.Type, m.To - 1 if slot else abi.HB_REF_OTHER, m.To if slot else 0, m.From, m.Term, m.LogTerm,
                    m.Index, m.Commit, bool(m.Reject), m.RejectHint))
    return out


def _all_scenarios():
    return VC.scenarios() + EC.scenarios()


def _oracle_groups(rafts, scs):
    groups, runs, peers, batch = EC.export(rafts, scs)
    og = OracleGroups(groups, runs, 256)
    older = synth.older_runs(og.groups(), runs)
    og.load_term_runs(older)
    return og, older, peers, batch


def _compare(got, want):
    """got: replay_votes records; want: the oracle's.  Returns the flagged votes."""
    assert len(got) == len(want)
    flagged = []
    for a, b in zip(got, want):
        if a[-1]:
            assert is_vote(a) and a[6] == 0
            assert (a[0], a[1], a[2], a[3], a[4], a[5], a[7]) == (b[0], b[1], b[2], b[3], b[4], b[5], b[7]), (a, b)
            flagged.append(a)
        else:
            assert a[:-1] == b, (a, b)
    return flagged


def test_last_term_is_the_oracles_last_term():
    scs = _all_scenarios()
    rafts = [EC.build(sc) for sc in scs]
    og, older, _, _ = _oracle_groups(rafts, scs)
    before = og.groups()
    assert older == oracle_older_runs(og)
    for g, r in enumerate(rafts):
        assert last_term(before[g], older[g]) == r.term(r.lastIndex), scs[g][0]
        in_run = before[g]["term_first"] != abi.HB_NO_INDEX and before[g]["last_index"] >= before[g]["term_first"]
        assert in_run or last_term(before[g], None) is None  # below the run and never loaded: unknown
    assert any(last_term(before[g], older[g]) != int(before[g]["term"]) for g in range(len(scs)))


def test_replay_of_step_events_equals_read_messages():
    scs = _all_scenarios()
    rafts = [EC.build(sc) for sc in scs]
    og, older, peers, batch = _oracle_groups(rafts, scs)
    before = og.groups()
    ev, _ = og.step(batch)
    got = by_group(replay_votes(ev, before, older, peers, 1))
    want = []
    for g, (r, sc) in enumerate(zip(rafts, scs)):
        for m in sc[5]:
            if r.fault:  # the reference panicked: nothing is stepped after it
                break
            r.Step(EC.oracle_msg(m))
        want += _expected(g, r, len(sc[2]))
    flagged = _compare(got, want)
    name = [sc[0] for sc in scs]
    # the flagged votes are exactly those of the two scenarios built for it
    assert {name[r[0]] for r in flagged} == {f"{s}/{n}" for s in VC.FLAGGED for n in VC.SIZES}
    votes = [r for r in got if is_vote(r)]
    for g, sc in enumerate(scs):
        mine = [r for r in votes if r[0] == g]
        if sc[0].split("/")[0] in VC.FLAGGED:
            assert len(mine) == len(sc[2]) - 1 and all(r[-1] for r in mine)
    clear = [r for r in votes if not r[-1]]
    assert any(r[6] != r[5] - 1 for r in clear)  # a LogTerm that is not Term - 1
    # a LogTerm that the log after the step no longer holds at that index (truncated and re-appended)
    moved = [r for r in clear if og.term(r[0], r[7]) != r[6]]
    assert moved and {name[r[0]].split("/")[0] for r in moved} == {"hup-then-truncate"}
    # the shapes: the single vote (n = 2), the broadcasts, the immediate win, the fault
    per = lambda s: [r for r in votes if name[r[0]] == s]  # noqa: E731
    assert len(per("hup-cur-run/2")) == 1 and len(per("hup-cur-run/7")) == 6 and not per("single/1")
    assert len(per("hup-twice/5")) == 8 and len({r[5] for r in per("hup-twice/5")}) == 2
    assert not per("leader-hup/3") and og.groups()[name.index("leader-hup/3")]["fault"] == abi.HB_FAULT_LEADER_CAMPAIGN
    second = per("win-stepdown-hup/3")[-1]
    T = scs[name.index("win-stepdown-hup/3")][4][0]
    assert (second[5], second[6], second[7]) == (T + 4, T + 1, 5)
    g = name.index("outsider-then-hup/3")
    assert any(r[0] == g and r[2] == abi.HB_REF_OTHER for r in got) and len(per("outsider-then-hup/3")) == 2
    assert any(r[2] == abi.HB_REF_OTHER and r[0] >= len(VC.scenarios()) for r in got)  # the other types' rows stay


def test_replay_of_tick_events_equals_read_messages():
    scs = _all_scenarios()
    rafts = []
    for sc in scs:
        r = EC.build(sc)
        r.draws = DRAWS
        r.r.elapsed = 20  # past every randomized election timeout
        rafts.append(r)
    og, older, peers, _ = _oracle_groups(rafts, scs)
    timers = np.zeros(len(scs), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
    og.load_timers(timers)
    before = og.groups()
    ev, _ = og.tick(DRAWS)
    got = by_group(replay_votes(ev, before, older, peers, 1))
    want = []
    for g, (r, sc) in enumerate(zip(rafts, scs)):
        r.tick()
        want += _expected(g, r, len(sc[2]))
    assert not _compare(got, want)  # no tick vote is flagged
    votes = [r for r in got if is_vote(r)]
    campaigners = [sc for sc in scs if sc[1] != "leader" and len(sc[2]) > 1]
    assert len(votes) == sum(len(sc[2]) - 1 for sc in campaigners) and len(campaigners) > 30
    assert any(r[6] != r[5] - 1 for r in votes)
    beats = [r for r in got if r[1] == abi.HB_MSG_HEARTBEAT]
    assert len(beats) == sum(len(sc[2]) - 1 for sc in scs if sc[1] == "leader") and len(beats) + len(votes) == len(got)
