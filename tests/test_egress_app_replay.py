"""The append-mode replay rules pinned to the oracle's own r.msgs (CPU).

As tests/test_egress_vote_replay.py, with sendAppend's MsgApp: the scenarios of
tests/egress_app_cases.py (and, for the other record types, those of
tests/egress_vote_cases.py and tests/egress_cases.py) are stepped and ticked
twice, as oracle.pyoracle.Raft objects, whose readMessages() gives the messages
the reference appended to r.msgs, and as an OracleGroups, whose events
tests/egress_app_util.replay_apps replays.  Every MsgApp record must equal the
oracle's message in To, From, Term, LogTerm, Index, Commit and the first and
last entry index; a flagged record must still match in To, From, Term and Index,
and every case states how many of its records are flagged.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth
from oracle.pyoracle import OracleGroups

from . import egress_app_cases as AC
from . import egress_cases as EC
from . import egress_vote_cases as VC
from .egress_app_util import boundary, is_app, replay_apps
from .egress_util import EGRESS_TYPES, by_group
from .egress_vote_util import oracle_older_runs
from .lift_util import base, lift

DRAWS = np.arange(1, 64, dtype=np.uint64) * np.uint64(7919)
TYPES = EGRESS_TYPES + (abi.HB_MSG_VOTE, abi.HB_MSG_APP)


def _expected(g, r, n):
    """The oracle's messages of TYPES as replay_apps tuples without the two flags, then the
    entry range (first, last) or (0, 0)."""
    out = []
    for m in r.readMessages():
        if m.Type not in TYPES:
            continue
        slot = 1 <= m.To <= n
        rng = (m.ent_lo, m.ent_lo + m.nents - 1) if m.Type == abi.HB_MSG_APP and m.nents else (0, 0)
        out.append((g, m.Type, m.To - 1 if slot else abi.HB_REF_OTHER, m.To if slot else 0, m.From, m.Term, m.LogTerm,
                    m.Index, m.Commit, bool(m.Reject), m.RejectHint) + rng)
    return out


def _compare(got, want):
    """got: replay_apps records; want: _expected's.  Returns the flagged records."""
    assert len(got) == len(want), (len(got), len(want))
    flagged = []
    for a, b in zip(got, want):
        host, ents = a[11], a[12]
        if host:
            assert (a[6], a[8], a[10], ents) == (0, 0, 0, False), a
            assert (a[:6], a[7]) == (b[:6], b[7]), (a, b)
            flagged.append(a)
        elif is_app(a):
            assert a[:10] == b[:10] and b[10] == 0, (a, b)
            assert ((a[7] + 1, a[10]) if ents else (0, 0)) == b[11:], (a, b)
            assert ents or a[10] == 0
        else:
            assert a[:11] == b[:11] and not ents, (a, b)
    return flagged


def _oracle_groups(rafts, cases, load_runs=True, max_msg_size=abi.HB_NO_LIMIT, lifted=None):
    groups, runs, peers, batch = AC.export(rafts, cases)
    if lifted:
        groups, runs, _ = lift(groups, runs, None, *lifted)
        batch = _lift_batch(batch, *lifted)
    og = OracleGroups(groups, runs, 256, max_msg_size)
    if load_runs:
        og.load_term_runs(synth.older_runs(og.groups(), runs))
    return og, peers, batch


def _lift_batch(batch, B, T):
    """The hand-built batch at index base B and term base T: every Term but a local message's 0,
    every Index, Commit, LogTerm and entry term of the message types that carry one."""
    b = dict(batch)
    t = b["info"] & 0xF
    b["term"] = np.where(b["term"] != 0, b["term"] + np.uint64(T), 0).astype(np.uint64)
    idx = np.isin(t, (abi.HB_MSG_APP_RESP, abi.HB_MSG_APP, abi.HB_MSG_VOTE, abi.HB_MSG_SNAP))
    b["index"] = np.where(idx, b["index"] + np.uint64(B), b["index"]).astype(np.uint64)
    rej = (t == abi.HB_MSG_APP_RESP) & ((b["info"] >> 8) & 1 == 1)
    lt = np.isin(t, (abi.HB_MSG_APP, abi.HB_MSG_VOTE, abi.HB_MSG_SNAP))
    b["hint"] = np.where(rej, b["hint"] + np.uint64(B), np.where(lt, b["hint"] + np.uint64(T), b["hint"])).astype(np.uint64)
    com = np.isin(t, (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT))
    b["commit"] = np.where(com, b["commit"] + np.uint64(B), b["commit"]).astype(np.uint64)
    b["eterm"] = (b["eterm"] + np.uint64(T)).astype(np.uint64)
    return b


def _lift_expected(want, B, T):
    out = []
    for r in want:
        g, mtype, to_ref, to, frm, term, lt, index, commit, reject, hint, lo, hi = r
        app_resp = mtype == abi.HB_MSG_APP_RESP
        out.append((g, mtype, to_ref, to, frm, term + T, lt + T if mtype in (abi.HB_MSG_APP, abi.HB_MSG_VOTE) else lt,
                    index + B if mtype in (abi.HB_MSG_APP, abi.HB_MSG_VOTE, abi.HB_MSG_APP_RESP) else index,
                    commit + B if mtype in (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT) else commit, reject,
                    hint + B if app_resp and reject else hint, lo + B if hi else 0, hi + B if hi else 0))
    return out


def _step_all(rafts, cases):
    want = []
    for g, (r, c) in enumerate(zip(rafts, cases)):
        for m in c["msgs"]:
            if r.fault:  # the reference panicked: nothing is stepped after it
                break
            r.Step(AC.oracle_msg(m))
        want += _expected(g, r, len(c["peers"]))
    return want


def _flag_counts(cases, flagged):
    """Flagged MsgApp records per case; any other flagged record is a vote of append-then-win
    (its LogTerm is unknown for the same reason, tests/egress_vote_cases.py)."""
    assert all(is_app(r) or cases[r[0]]["name"].startswith("append-then-win") for r in flagged)
    return {c["name"]: sum(1 for r in flagged if r[0] == g and is_app(r)) for g, c in enumerate(cases)}


def test_boundary_is_the_oracles_term_below_the_run():
    cases = AC.scenarios()
    rafts = [AC.build(c) for c in cases]
    og, _, _ = _oracle_groups(rafts, cases)
    before, older = og.groups(), oracle_older_runs(og)
    for g, (r, c) in enumerate(zip(rafts, cases)):
        bl, blt = boundary(before[g], older[g])
        assert blt == r.term(bl), c["name"]
        if c["role"] == "leader" and len(c["peers"]) > 1:
            assert (bl, blt) == (4, c["hard"][0]), c["name"]  # just below the noop, the Term before the election
        assert boundary(before[g], None)[1] is None or before[g]["term_first"] == abi.HB_NO_INDEX


def test_replay_of_step_events_equals_read_messages():
    cases = AC.scenarios()
    rafts = [AC.build(c) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    flagged = _compare(got, _step_all(rafts, cases))
    assert _flag_counts(cases, flagged) == {c["name"]: c["flagged"] for c in cases}
    assert {c["name"].split("/")[0] for c in cases if c["flagged"]} == set(AC.FLAGGED)
    name = [c["name"] for c in cases]
    per = lambda s: [r for r in got if is_app(r) and name[r[0]] == s]  # noqa: E731
    for n in AC.SIZES:
        T = 4 + n
        a = per(f"cfg2/{n}")  # one entry and the old Commit, then none and the new one
        assert [(r[7], r[10], r[8], r[12]) for r in a] == [(5, 6, 5, True)] * (n - 1) + [(6, 0, 6, False)] * (n - 1)
        assert [r[2] for r in a] == list(range(1, n)) * 2 and all(r[6] == r[5] == T + 1 for r in a)
        a = per(f"commit-moves/{n}")
        assert [r[8] for r in a] == [5] * (2 * (n - 1)) + [6] * (n - 1) + [7] * (n - 1)
        assert [(r[7], r[10]) for r in per(f"prop-k/{n}")] == [(5, 8)] * (n - 1)
        assert [(r[7], r[6], r[10]) for r in per(f"reject-aux1/{n}")][-1] == (5, T + 1, 6)
        assert [(r[2], r[7], r[6], r[10]) for r in per(f"reject-at-boundary/{n}")] == [(1, 4, T, 5)]
        assert [(r[7], r[11]) for r in per(f"reject-below-boundary/{n}")] == [(2, True)]
        assert [(r[7], r[12]) for r in per(f"heartbeat-resp/{n}")][-1] == (6, False)
        assert [(r[7], r[6], r[10]) for r in per(f"heartbeat-resp-paused/{n}")] == [(4, T, 5)]  # the second sends nothing
        assert [(r[2], r[7]) for r in per(f"needs-snapshot/{n}")] == [(2, 4)]
        assert (ev[(ev["group"] == name.index(f"needs-snapshot/{n}"))]["type"] == abi.HB_EV_SNAP).sum() == 1
        assert [(r[7], r[6], r[8], r[10]) for r in per(f"win-cur/{n}")] == [(4, T, 2, 5)] * (n - 1)
        assert [(r[7], r[6], r[8], r[10]) for r in per(f"win-old/{n}")] == [(3, T - 2, 2, 4)] * (n - 1)
        assert len(per(f"append-then-win/{n}")) == n - 1
        assert len(per(f"stepdown/{n}")) == n - 1 == len(per(f"fault/{n}"))
        assert og.groups()[name.index(f"fault/{n}")]["fault"] == abi.HB_FAULT_LEADER_CAMPAIGN
    assert not per("single-leader/1") and og.groups()[name.index("single-leader/1")]["committed"] == 5


def test_the_other_scenario_sets_make_the_same_records_plus_apps():
    """The vote and plain scenario sets through replay_apps (whose own assertion reduces it to
    replay_votes): their leaders' MsgApps against the oracle too."""
    scs = VC.scenarios() + EC.scenarios()
    cases = [dict(name=s[0], role=s[1], peers=s[2], ents=s[3], hard=s[4], msgs=s[5], setup=(), snapshot=None) for s in scs]
    rafts = [AC.build(c) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    flagged = _compare(got, _step_all(rafts, cases))
    assert sum(is_app(r) for r in got) > 20
    # flagged: the votes tests/egress_vote_cases.py names, and no MsgApp but a winner's whose log a
    # leader wrote earlier in the call
    assert {cases[r[0]]["name"].split("/")[0] for r in flagged if not is_app(r)} == set(VC.FLAGGED)
    assert not [r for r in flagged if is_app(r)]


def test_replay_of_tick_events_equals_read_messages():
    cases = AC.scenarios()
    rafts = []
    for c in cases:
        r = AC.build(c)
        r.draws = DRAWS
        r.r.elapsed = 20  # past every timeout
        rafts.append(r)
    og, peers, _ = _oracle_groups(rafts, cases)
    timers = np.zeros(len(cases), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
    og.load_timers(timers)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.tick(DRAWS)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    want = []
    for g, (r, c) in enumerate(zip(rafts, cases)):
        r.tick()
        want += _expected(g, r, len(c["peers"]))
    assert not _compare(got, want)
    assert not any(is_app(r) for r in got)  # a tick sends heartbeats and votes; its winners (n = 1) send nothing


def test_election_split_over_two_calls():
    """Scenario 9: Hup by a tick, the grants by a step.  The boundary comes from the snapshot of the
    second call: the candidate's current-term run is empty, so bl0 = last and blt0 = lastTerm."""
    cases = AC.election_cases()
    rafts = []
    for c in cases:
        r = AC.build(c)
        r.draws = DRAWS
        r.r.elapsed = 20
        rafts.append(r)
    og, peers, _ = _oracle_groups(rafts, cases)
    timers = np.zeros(len(cases), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
    og.load_timers(timers)
    og.tick(DRAWS)
    for r in rafts:
        r.tick()
        r.readMessages()
    grants = [dict(c, msgs=c["msgs"][1:]) for c in cases]
    _, _, _, batch = AC.export(rafts, grants)
    before, older = og.groups(), oracle_older_runs(og)
    assert (before["term_first"] == abi.HB_NO_INDEX).all() and (before["state"] == abi.HB_STATE_CANDIDATE).all()
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    assert not _compare(got, _step_all(rafts, grants))
    for g, c in enumerate(cases):
        T, old = c["hard"][0], c["name"].startswith("win-old")
        mine = [r for r in got if r[0] == g and is_app(r)]
        assert [(r[7], r[6]) for r in mine] == [((3, T - 2) if old else (4, T))] * (len(c["peers"]) - 1)


def test_never_loaded_runs_flag_the_first_broadcast():
    """Scenario 10: the election cases on groups whose term runs were never loaded.  A log that ends
    in the current-term run still knows its lastTerm; one that ends below it does not."""
    cases = AC.election_cases()
    rafts = [AC.build(c) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases, load_runs=False)
    before, older = og.groups(), oracle_older_runs(og)
    assert not any(older.values())
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    flagged = _compare(got, _step_all(rafts, cases))
    want = {c["name"]: (len(c["peers"]) - 1 if c["name"].startswith("win-old") else 0) for c in cases}
    apps = [r for r in flagged if is_app(r)]
    assert _flag_counts(cases, apps) == want and sum(want.values()) > 0


@pytest.mark.parametrize("max_msg_size", [0, 13])
def test_max_msg_size_zero_and_finite(max_msg_size):
    """Scenario 14.  0: every entry-carrying MsgApp holds exactly entry x + 1.  13 (two entries of
    6 bytes): limitSize's cut is in no event, so a record with entries is flagged, an empty one not."""
    cases = AC.size_cases()
    rafts = []
    for c in cases:
        if max_msg_size:
            c = dict(c, setup=(("sizes", [6] * len(c["ents"])),) + c["setup"])
        rafts.append(_build_sized(c, max_msg_size))
    og, peers, batch = _oracle_groups(rafts, cases, max_msg_size=max_msg_size)
    if max_msg_size:
        g0 = og.groups()
        og.load_sizes({g: [6] * int(g0[g]["last_index"]) for g in range(len(cases))})
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1, max_msg_size=max_msg_size))
    want = _step_all(rafts, cases)
    flagged = _compare(got, want)
    apps = [r for r in got if is_app(r)]
    with_ents = [b for b in want if b[1] == abi.HB_MSG_APP and b[12]]
    assert len(with_ents) > 10 and len(with_ents) < len(apps)
    if max_msg_size == 0:
        assert not flagged and all(r[10] == r[7] + 1 for r in apps if r[12])
        assert any(b[12] < 8 for b in with_ents if b[7] == 5)  # prop-k: (5, 6], not (5, 8]
    else:
        assert len(flagged) == len(with_ents) and not any(r[12] for r in apps)
        assert any(b[12] == 7 for b in with_ents)  # the cut the flag leaves to the host: (5, 7] of (5, 8]


def _build_sized(c, max_msg_size):
    from oracle.pyoracle import Raft
    r = Raft(1, c["peers"], ents=c["ents"], hard=c["hard"], max_msg_size=max_msg_size)
    for op in c["setup"]:
        if op[0] == "sizes":
            r.load_sizes(op[1])
    r.becomeCandidate()
    r.becomeLeader()
    for op in c["setup"]:
        if op[0] == "step":
            r.Step(AC.oracle_msg(op[1]))
    assert not r.fault
    r.readMessages()
    return r


@pytest.mark.parametrize("name", ["W32", "W40", "W62"])
def test_wide_values(name):
    """Scenario 15: the scenario set lifted to 2^32, to 2^40 / 2^24 and to 2^61 / 2^50.  The oracle
    groups run at the lifted values; the Raft objects run as they are and their messages are
    lifted (every rule of the reference is translation-invariant in index and term)."""
    B, T = base(name, delta=5, eps=3)
    cases = [c for c in AC.scenarios() if not c["snapshot"] and len(c["peers"]) > 1]
    rafts = [AC.build(c) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases, lifted=(B, T))
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    flagged = _compare(got, _lift_expected(_step_all(rafts, cases), B, T))
    assert _flag_counts(cases, flagged) == {c["name"]: c["flagged"] for c in cases}
    x = [r[7] for r in got if is_app(r)]
    if name == "W40":
        assert min(x) < 1 << 40 <= max(x)
