"""The replay rules of the LogTerm lookup pinned to the oracle's own r.msgs (CPU).

As tests/test_egress_app_replay.py: the scenarios of tests/egress_logterm_cases.py are stepped
twice, as oracle.pyoracle.Raft objects, whose readMessages() gives every MsgApp with the
LogTerm the reference computed (raftLog.term of its Index), and as an OracleGroups, whose
events tests/egress_logterm_util.replay_apps_logterm replays.  Every unflagged MsgApp record
must carry the oracle's LogTerm; every case states its number of flagged records.
"""
import numpy as np
import pytest

from etcd_amd import abi
from oracle.pyoracle import OracleGroups

from . import egress_app_cases as AC
from . import egress_limit_cases as LC
from . import egress_logterm_cases as GC
from .compact_util import pow2ceil
from .egress_app_util import is_app, replay_apps
from .egress_limit_util import follower_rewrites, replay_apps_limit, sized, size_table
from .egress_logterm_util import lookup_sends, replay_apps_logterm, ring_oldest
from .egress_util import by_group
from .egress_vote_util import oracle_older_runs
from .lift_util import base, lift
from .test_egress_app_replay import _compare, _flag_counts, _lift_batch, _lift_expected, _step_all


def setup(cases, max_msg_size=abi.HB_NO_LIMIT, lifted=None):
    """(rafts, og, peers, batch, loaded runs, loaded sizes): the oracle side of a case set."""
    rafts = [LC.build(c, max_msg_size) if sized(max_msg_size) else AC.build(c) for c in cases]
    groups, runs, peers, batch = AC.export(rafts, cases)
    if lifted:
        groups, runs, _ = lift(groups, runs, None, *lifted)
        batch = _lift_batch(batch, *lifted)
    og = OracleGroups(groups, runs, 256, max_msg_size)
    loaded = GC.loaded_runs(og.groups(), runs, cases)
    og.load_term_runs(loaded)
    sizes = None
    if sized(max_msg_size):
        sizes = {g: LC.log_sizes(r) for g, r in enumerate(rafts)}
        og.load_sizes(sizes)
    return rafts, og, peers, batch, loaded, sizes


def run_caps(loaded):
    """The run ring's capacity after hb_load_term_runs (n runs plus one) when nobody reserves more."""
    return {g: max(abi.HB_TERM_RING_MIN, int(pow2ceil(len(rr) + 1))) for g, rr in loaded.items()}


def run(cases, max_msg_size=abi.HB_NO_LIMIT, cut=False, lifted=None):
    """(records by group, flagged records, the ring's final oldest starts, the events)."""
    B, T = lifted or (0, 0)
    rafts, og, peers, batch, loaded, sizes = setup(cases, max_msg_size, lifted)
    before, older = og.groups(), oracle_older_runs(og)
    assert {g: [tuple(r) for r in rr] for g, rr in older.items()} == loaded  # the ring is what was loaded
    ev, _ = og.step(batch)
    want = _step_all(rafts, cases)
    if lifted:
        want = _lift_expected(want, B, T)
    oldest = ring_oldest(ev, before, older, run_caps(loaded))
    limit = None
    if cut:
        szlo = {g: int(before[g]["last_index"]) - len(z) for g, z in sizes.items()}
        limit = (size_table(ev, before, sizes, batch), szlo)
    term_of = lambda g, i: rafts[g].term(i - B) + T  # noqa: E731
    got = by_group(replay_apps_logterm(ev, before, older, peers, 1, term_of, oldest, max_msg_size=max_msg_size,
                                       limit=limit))
    return got, _compare(got, want), oldest, ev, (before, older, peers)


def test_replay_with_the_lookup_equals_read_messages():
    cases = GC.scenarios()
    got, flagged, oldest, ev, _ = run(cases)
    assert _flag_counts(cases, flagged) == {c["name"]: c["flagged"] for c in cases}
    assert {c["name"].split("/")[0] for c in cases if c["flagged"]} == set(GC.FLAGGED)
    name = [c["name"] for c in cases]
    per = lambda s: [r for r in got if is_app(r) and name[r[0]] == s]  # noqa: E731
    for n in GC.SIZES:
        T = 4 + n
        # (Index, LogTerm, flagged, last entry)
        assert [(r[7], r[6], r[11], r[10]) for r in per(f"reject-below-boundary/{n}")] == [(2, 1, False, 5)]
        assert [(r[7], r[6], r[11]) for r in per(f"walk-down/{n}")] == [(3, 3, False), (2, 2, False), (1, 1, False)]
        assert [(r[7], r[6], r[11]) for r in per(f"at-snapshot/{n}")] == [(2, 1, False)]
        assert [(r[7], r[6], r[11]) for r in per(f"at-snapshot-unloaded/{n}")] == [(2, 0, True)]
        assert oldest[name.index(f"at-snapshot-unloaded/{n}")] == 3 and oldest[name.index(f"at-snapshot/{n}")] == 2
        assert [(r[7], r[6], r[11]) for r in per(f"send-then-truncate/{n}")] == [(2, 0, True)]
        assert [(r[7], r[6], r[11]) for r in per(f"send-then-heartbeat/{n}")] == [(2, 1, False)]
        assert [r[11] for r in per(f"append-then-win/{n}")] == [True] * (n - 1)
        # the existing rules stay first: at the boundary, and inside the current-term run
        assert [(r[7], r[6]) for r in per(f"reject-at-boundary/{n}")] == [(4, T)]
        assert [(r[7], r[6]) for r in per(f"reject-aux1/{n}")][-1] == (5, T + 1)
        g = name.index(f"send-then-heartbeat/{n}")
        mine = ev[ev["group"] == g]
        assert (mine["type"] == abi.HB_EV_TERM).sum() == 1 and g not in follower_rewrites(ev)
        g = name.index(f"send-then-truncate/{n}")
        mine = ev[(ev["group"] == g) & (ev["type"] == abi.HB_EV_FOLLOW)]
        assert (mine["aux"] == abi.HB_FOLLOW_APPEND).sum() == 1


def test_the_knob_changes_only_the_lookup_records():
    """Against the parent rule on the same events: the records that differ are exactly the sends
    lookup_sends names that neither rule flags."""
    cases = GC.scenarios()
    got, _, _, ev, (before, older, peers) = run(cases)
    parent = by_group(replay_apps(ev, before, older, peers, 1))
    diff = [(a, b) for a, b in zip(got, parent) if a != b]
    names = {cases[a[0]]["name"].split("/")[0] for a, _ in diff}
    assert names == {"reject-below-boundary", "walk-down", "at-snapshot", "send-then-heartbeat"}
    assert all(b[11] and not a[11] and a[:6] == b[:6] and a[7] == b[7] for a, b in diff)
    # (every flagged record of the set is such a send: append-then-win's too, whose boundary is unknown)
    assert len(diff) == sum(lookup_sends(ev, before, older)) - sum(c["flagged"] for c in cases) == 18
    assert all(c["flagged"] == 0 or c["name"].split("/")[0] in GC.FLAGGED for c in cases)


def test_ring_of_8_drops_the_run_of_the_early_send():
    """Rule (i) by a drop: the model really drops the run (the final oldest start lies above the
    early send's Index), and the sibling one run higher keeps its LogTerm."""
    cases = GC.ring_drop_cases()
    got, flagged, oldest, ev, (before, older, _) = run(cases)
    assert _flag_counts(cases, flagged) == {c["name"]: c["flagged"] for c in cases}
    for g, c in enumerate(cases):
        assert len(older[g]) == 7 and older[g][0] == (2, 1) and older[g][1] == (3, 2), c["name"]
        assert (ev[ev["group"] == g]["type"] == abi.HB_EV_TERM).sum() == 3  # step-down, campaign, step-down
        assert oldest[g] == 3, c["name"]  # two pushes into a ring of 8 that held 7: (2, 1) left
        first = [r for r in got if r[0] == g and is_app(r)][0]
        early = c["name"].startswith("drop-early")
        assert c["x"] == first[7] == (2 if early else 3) and (oldest[g] > first[7]) == early
        assert (first[6], first[11]) == ((0, True) if early else (2, False)), c["name"]
        # the new leader's broadcast in between is at its boundary: no lookup
        n = len(c["peers"])
        assert [(r[7], r[6], r[11]) for r in got if r[0] == g and is_app(r)][1:] == [(9, c["hard"][0] + 1, False)] * (n - 1)
    # with one slot more the run stays: nothing is flagged (the rule is the ring's, not the case's)
    rafts, og, peers, batch, loaded, _ = setup(cases)
    before, older = og.groups(), oracle_older_runs(og)
    ev2, _ = og.step(batch)
    assert set(ring_oldest(ev2, before, older, 16).values()) == {2}


@pytest.mark.parametrize("limit", [13, 1000])
def test_below_the_boundary_under_a_limit(limit):
    cases = GC.limit_cases()
    # both knobs: the cut and the LogTerm
    got, flagged, _, ev, (before, older, peers) = run(cases, max_msg_size=limit, cut=True)
    assert not flagged
    for g, c in enumerate(cases):
        T = c["hard"][0]
        (r,) = [r for r in got if r[0] == g and is_app(r)]
        # (every Term here is below 128: Entry.Size() is the same 6 or 7 bytes at T - 1, T and T + 1)
        assert (r[7], r[6], r[12], r[10]) == (2, 1, True, LC.probe_cut(T + 1, limit, x=2)), c["name"]
    assert all(r[10] == 4 for r in got if is_app(r)) if limit == 13 else all(r[10] > 100 for r in got if is_app(r))
    # this knob alone: flagged for the cut
    got1, flagged1, _, _, _ = run(cases, max_msg_size=limit, cut=False)
    assert _flag_counts(cases, flagged1) == {c["name"]: c["flagged_one_knob"] for c in cases}
    # the limit knob alone: flagged for the LogTerm
    rafts, og, peers, batch, loaded, sizes = setup(cases, limit)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    szlo = {g: int(before[g]["last_index"]) - len(z) for g, z in sizes.items()}
    only = by_group(replay_apps_limit(ev, before, older, peers, 1, limit, size_table(ev, before, sizes, batch), szlo))
    assert _flag_counts(cases, _compare(only, _step_all(rafts, cases))) == {c["name"]: 1 for c in cases}
    assert only == got1


@pytest.mark.parametrize("name", GC.WIDE)
def test_wide_values(name):
    """One resend below the boundary (and the walk-down) at 2^32, at 2^40 / 2^24 and at 2^61 /
    2^50: the oracle groups run at the lifted values, the Raft objects' messages are lifted."""
    B, T = base(name, delta=3, eps=2)
    cases = GC.below_cases()
    got, flagged, oldest, _, _ = run(cases, lifted=(B, T))
    assert not flagged
    apps = [r for r in got if is_app(r)]
    assert len(apps) == 4 * len(GC.SIZES) and all(r[6] == r[7] - B + T or r[7] - B == 2 for r in apps)
    assert sorted({r[7] - B for r in apps}) == [1, 2, 3] and all(T < r[6] <= T + 3 for r in apps)
    if name == "W40":
        x = [r[7] for r in apps]
        assert min(x) < 1 << 40 <= max(x)
