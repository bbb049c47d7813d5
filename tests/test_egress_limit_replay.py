"""The replay rules of limitSize's cut pinned to the oracle's own r.msgs (CPU).

As tests/test_egress_app_replay.py on rafts with a finite max_msg_size: the scenarios of
tests/egress_limit_cases.py are stepped twice, as oracle.pyoracle.Raft objects, whose
readMessages() gives every MsgApp with the entry range limitSize left it (ent_lo, nents),
and as an OracleGroups, whose events tests/egress_limit_util.replay_apps_limit replays.
Every unflagged MsgApp record must name the oracle's range; every case states its number
of flagged records.
"""
import numpy as np
import pytest

from etcd_amd import abi

from . import egress_limit_cases as LC
from .compact_util import OracleCompactPair
from .egress_app_util import is_app, replay_apps
from .egress_limit_util import replay_apps_limit, size_table, szlo_final
from .egress_util import by_group
from .egress_vote_util import oracle_older_runs
from .test_egress_app_replay import _compare, _flag_counts, _oracle_groups, _step_all


def run(cases, limit):
    """(records by group, the oracle's messages, flagged records, case names)."""
    rafts = [LC.build(c, limit) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases, max_msg_size=limit)
    loaded = {g: LC.log_sizes(r) for g, r in enumerate(rafts)}
    og.load_sizes(loaded)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    assert not (og.groups()["fault"] == abi.HB_FAULT_SIZE_WINDOW).any()
    # the oracle keeps every size it was given: the ring's oldest index is the loaded window's
    szlo = {g: int(before[g]["last_index"]) - len(z) for g, z in loaded.items()}
    got = by_group(replay_apps_limit(ev, before, older, peers, 1, limit, size_table(ev, before, loaded, batch), szlo))
    want = _step_all(rafts, cases)
    return got, want, _compare(got, want), [c["name"] for c in cases]


@pytest.mark.parametrize("limit", LC.LIMITS)
def test_replay_with_the_cut_equals_read_messages(limit):
    cases = LC.scenarios()
    got, want, flagged, name = run(cases, limit)
    assert _flag_counts(cases, flagged) == {c["name"]: c["flagged"] for c in cases}
    assert {c["name"].split("/")[0] for c in cases if c["flagged"]} == set(LC.FLAGGED)
    per = lambda s: [r for r in got if is_app(r) and name[r[0]] == s]  # noqa: E731
    apps = [r for r in got if is_app(r)]
    with_ents = [b for b in want if b[1] == abi.HB_MSG_APP and b[12]]
    # every record with entries that is not flagged for one of FLAGGED's reasons carries its cut
    assert len(with_ents) > 40 and sum(r[12] for r in apps) + sum(c["flagged"] for c in cases) >= len(with_ents)
    for n in LC.SIZES:
        T = 4 + n
        k = {13: 2, 1: 1, 18: 3, 17: 2, 1000: 3}[limit]  # entries of (5, 8] in one message
        assert [(r[7], r[10]) for r in per(f"prop-k/{n}")] == [(5, 5 + k)] * (n - 1)
        # the new leader's noop: one entry, whatever the limit
        assert [(r[7], r[6], r[10]) for r in per(f"win-cur/{n}")] == [(4, T, 5)] * (n - 1)
        assert [(r[7], r[6], r[10]) for r in per(f"win-old/{n}")] == [(3, T - 2, 4)] * (n - 1)
        # a send, then the truncating append: every record with entries stays with the host
        assert [(r[7], r[11], r[12]) for r in per(f"send-then-truncate/{n}")] == [(4, True, False)] * (n - 1)
        assert [r[11] for r in per(f"append-then-win/{n}")] == [True] * (n - 1)
        # the rejected MsgApp of "stepdown" appends nothing: its first broadcast keeps the cut
        assert [(r[7], r[10], r[11]) for r in per(f"stepdown/{n}")] == [(5, 6, False)] * (n - 1)
        a = per(f"probe-behind/{n}")
        L = LC.probe_cut(T + 1, limit)
        assert a[0][7] == 4 and a[0][10] == L and a[0][2] == 1
        if limit == 1000:
            assert L == 164 and [(r[7], r[10], r[6]) for r in a] == [(4, 164, T), (164, 205, T + 1)]
        else:
            assert L < 8 and a[1][7] == LC.probe_cut(T + 1, 1000)  # (the ack names 164: Next = 165)
        if limit in (13, 17):  # (5, 7], then the acks of 6 move Commit and the rest follows: (7, 8]
            assert {(r[7], r[10]) for r in per(f"prop-then-acks/{n}")} >= {(5, 7), (7, 8)}
    assert not per("single-leader/1")
    if limit == 1:
        assert all(r[10] == r[7] + 1 for r in apps if r[12])
    else:
        assert any(r[10] > r[7] + 1 for r in apps if r[12])


@pytest.mark.parametrize("name", LC.WIDE)
def test_the_cut_where_entry_sizes_change(name):
    """A cut at wide values: the rafts stand at the base themselves (a snapshot at B + 2), since
    Entry.Size() is not translation-invariant.  P35: entry 2^35 is a byte longer than 2^35 - 1."""
    B, _ = LC.wide_base(name)
    cases = LC.wide_scenarios(name)
    for which in (0, 1):
        for n in LC.SIZES:  # the limit depends on the Term, hence on n
            mine = [c for c in cases if len(c["peers"]) == n]
            limit = LC.wide_limits(name, n)[which]
            got, want, flagged, names = run(mine, limit)
            assert not flagged
            pk = [r for r in got if is_app(r) and names[r[0]].startswith("prop-k")]
            assert [(r[7], r[10]) for r in pk] == [(B + 5, B + 7 - which)] * (n - 1)
            assert sum(r[12] for r in got if is_app(r)) == 2 * (n - 1)
    if name == "P35":
        assert LC.entry_size(1, B + 7) == LC.entry_size(1, B + 6) + 1 == 11
        # two entries of the shorter size would fit the lower limit: the cut is the longer entry's
        assert 2 * LC.entry_size(12, B + 6) == LC.wide_limits(name, 7)[1]


def test_forcing_every_cut_to_the_host_is_the_parent_rule():
    """replay_apps_limit asserts that it reduces to replay_apps(max_msg_size = finite); here the
    other direction: with rule (i) covering every send (no size kept) nothing is cut."""
    cases = LC.scenarios((3,))
    rafts = [LC.build(c, 13) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases, max_msg_size=13)
    loaded = {g: LC.log_sizes(r) for g, r in enumerate(rafts)}
    og.load_sizes(loaded)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    none = {g: 1 << 62 for g in loaded}
    got = replay_apps_limit(ev, before, older, peers, 1, 13, None, none)
    assert got == replay_apps(ev, before, older, peers, 1, max_msg_size=13) and any(r[11] for r in got)


def _oracle_expect(pair, ev, before, older, szlo0, peers, limit, loaded, batch):
    """replay_apps_limit over an oracle-only pair (compact_util.OracleCompactPair): the ring's
    capacity is the one the pair predicts for the device (cap_sz)."""
    now = pair.og.groups()
    szlo = [szlo_final(szlo0[g], now["last_index"][g], pair.cap_sz[g]) for g in range(len(now))]
    return by_group(replay_apps_limit(ev, before, older, peers, 1, limit, size_table(ev, before, loaded, batch), szlo,
                                      votes=False))


def _steady_peers(G, n):
    p = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    p[:, :n] = np.arange(1, n + 1, dtype=np.uint64)
    return p


def test_cfg2_step_under_limit_150_reference():
    """The inputs of the device test: at 150 the step makes cut records, whole ones of two and
    three entries and records without entries, no fault and nothing flagged (at 256 no cut)."""
    counts = {}
    for limit in (150, 256):
        g, runs, loaded, b = LC.cfg2_sized_inputs()
        pair = OracleCompactPair(g, runs, 3, 256, max_msg_size=limit, sizes=loaded, term_runs=True)
        peers = _steady_peers(len(g), 3)
        before, older, szlo0 = pair.og.groups(), oracle_older_runs(pair.og), pair.og.log_info()[:, 1]
        ev, _, now = pair.step(b)
        assert not now["fault"].any()
        want = _oracle_expect(pair, ev, before, older, szlo0, peers, limit, loaded, b)
        last = [r[10] for r in by_group(replay_apps(ev, before, older, peers, 1, votes=False))]
        cut = sum(1 for r, l in zip(want, last) if r[12] and r[10] < l)
        whole = [r for r, l in zip(want, last) if r[12] and r[10] == l]
        counts[limit] = (cut, len(whole), sum(r[10] - r[7] >= 2 for r in whole), sum(not r[12] for r in want),
                         sum(r[11] for r in want))
    print("cut, whole, whole of two or more entries, without entries, flagged:", counts)
    assert counts[150] == (124, 537, 286, 539, 0) and counts[256][0] == 0


def test_ring_of_16_reference():
    """Rule (i) on the CPU: the state the device test reaches.  24 entries appended in one call
    against a ring of 16 (nothing reserved), no HB_FAULT_SIZE_WINDOW; the sends at last0 and
    last0 + 6 lie below the final ring and are flagged, the later ones carry their cut."""
    g, runs, loaded, batch, limit = LC.ring_scenario()
    G, n = len(g), int(g["n"][0])
    pair = OracleCompactPair(g, runs, n, 256, hold=True, max_msg_size=limit, sizes=loaded, term_runs=True)
    assert (pair.cap_sz == abi.HB_SIZE_RING_MIN).all()
    before, older, szlo0 = pair.og.groups(), oracle_older_runs(pair.og), pair.og.log_info()[:, 1]
    ev, _, now = pair.step(batch)
    assert not now["fault"].any() and (now["last_index"] == g["last_index"] + 24).all()
    assert (pair.cap_sz == abi.HB_SIZE_RING_MIN).all()
    want = _oracle_expect(pair, ev, before, older, szlo0, _steady_peers(G, n), limit, loaded, batch)
    for gi in range(G):
        last0 = int(g["last_index"][gi])
        mine = [r for r in want if r[0] == gi]
        assert [(r[7] - last0, r[11]) for r in mine] == [(x, x < 9) for x in (0, 6, 12, 18) for _ in range(n - 1)]
        # every send stayed inside the ring as it stood at that send (no HB_FAULT_SIZE_WINDOW on the device)
        assert all(r[7] >= max(int(szlo0[gi]), r[7] + 6 - 15) for r in mine)
        assert all(r[10] == last0 + 18 for r in mine if r[7] == last0 + 12)
        assert all(last0 + 18 < r[10] < last0 + 24 for r in mine if r[7] == last0 + 18)
