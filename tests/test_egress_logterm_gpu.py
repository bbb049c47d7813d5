"""GPU parity of the LogTerm lookup in wire egress: hb_set_egress_logterm on
a handle in append mode, hb_egress + hb_encode (+ hb_egress_bin, hb_encode_ents, hb_peer_spans,
hb_frame, hb_unframe, hb_decode_follow) against tests/egress_logterm_util.py, which
tests/test_egress_logterm_replay.py pins to the oracle's own r.msgs.

Every scenario goes through parity_util.Pair, so the engine's events and groups are already
compared with the oracle's; the expected records are replay_apps_logterm of the oracle's
events, the runs the ring held before the call, and the ring's final oldest start as
hb_log_capacity and egress_logterm_util.ring_oldest give it.  Every array, off, status, total
and the bytes are compared exactly (test_egress_app_gpu._check).
"""
import numpy as np
import pytest

from etcd_amd import abi, synth

from . import egress_app_cases as AC
from . import egress_limit_cases as LC
from . import egress_logterm_cases as GC
from . import props_util as PU
from .compact_util import CompactPair
from .egress_app_util import is_app, replay_apps
from .egress_bin_util import bin_reference
from .egress_limit_util import replay_apps_limit, size_table, with_descs
from .egress_logterm_util import replay_apps_logterm, ring_oldest
from .egress_util import by_group, replay
from .egress_vote_util import oracle_older_runs, replay_votes
from .lift_util import base, lift
from .parity_util import Pair
from .test_egress_app_gpu import _check, _oracle_bytes, _spliced
from .test_egress_app_replay import _lift_batch, _lift_expected, _step_all
from .test_egress_gpu import _check as _check_plain, _egress, _peers, _tap
from .test_egress_vote_gpu import _check as _check_votes

pytestmark = pytest.mark.gpu

SELF = 1
FIELDS = abi.OUT_BATCH_FIELDS
NO_LIMIT = abi.HB_NO_LIMIT


def _before(pair):
    """What the expectation needs from before a call: the groups, the ring's older term runs, the
    oldest index of every size ring."""
    return pair.og.groups(), oracle_older_runs(pair.og), pair.og.log_info()[:, 1].astype(np.int64)


def _run_caps(pair):
    return {g: pair.eng.log_capacity(g)[1] for g in range(pair.og.G)}


def _expect(pair, snap, peers, rafts, caps=None, votes=True, limit=NO_LIMIT, cut=None, lifted=(0, 0), grouped=True):
    """replay_apps_logterm of the oracle's events.  caps: the run rings' capacities during the call
    (default: hb_log_capacity now); cut = (loaded sizes, batch): the limit knob is on too."""
    B, T = lifted
    ev = pair.ora_ev
    oldest = ring_oldest(ev, snap[0], snap[1], _run_caps(pair) if caps is None else caps)
    lim = None
    if cut is not None:
        szlo = {g: int(snap[2][g]) for g in range(len(snap[0]))}  # (no case here appends past its size ring)
        lim = (size_table(ev, snap[0], cut[0], cut[1]), szlo)
    term_of = lambda g, i: rafts[g].term(i - B) + T  # noqa: E731
    recs = replay_apps_logterm(ev, snap[0], snap[1], peers, SELF, term_of, oldest, max_msg_size=limit, limit=lim,
                               votes=votes)
    return by_group(recs) if grouped else recs


def _pair(nmax, cases, knob=True, lifted=None, compact=False, hold=False, **mode):
    cases = [c for c in cases if len(c["peers"]) <= nmax]
    rafts = [AC.build(c) for c in cases]
    groups, runs, peers, batch = AC.export(rafts, cases)
    if lifted:
        groups, runs, _ = lift(groups, runs, None, *lifted)
        batch = _lift_batch(batch, *lifted)
    tr = GC.loaded_runs(groups, runs, cases)
    if compact:
        pair = _tap(CompactPair(groups, runs, nmax, 256, hold=hold, max_batch=4096, term_runs=tr))
    else:
        pair = _tap(Pair(groups, runs, nmax, 256, max_batch=4096, term_runs=tr))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, **mode)
    pair.eng.set_egress_logterm(knob)
    assert pair.eng.egress_logterm() == knob
    return pair, cases, rafts, peers, batch


def _flag_map(want, cases):
    out = {}
    for r in want:
        if is_app(r) and r[11]:
            out[cases[r[0]]["name"]] = out.get(cases[r[0]]["name"], 0) + 1
    return out


# ---- 1. the case set in one step: knob off is the parent, knob on, the spliced bytes ------------
@pytest.mark.parametrize("votes", [True, False], ids=["mode7", "mode5"])
@pytest.mark.parametrize("nmax", [3, 5, 7])
def test_scenario_step(nmax, votes):
    # the knob off: the parent's flags
    pair, cases, rafts, peers, batch = _pair(nmax, GC.scenarios(), knob=False, votes=votes, apps=True)
    snap = _before(pair)
    pair.step(batch, ctx=f"logterm off nmax={nmax}")
    off = by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF, votes=votes))
    _check(_egress(pair.eng, 4096), off, f"logterm off nmax={nmax}")
    assert _flag_map(off, cases)[f"reject-below-boundary/{nmax}"] == 1 and _flag_map(off, cases)[f"walk-down/{nmax}"] == 3
    pair.eng.close()
    # a fresh handle with it on, the same step
    pair, cases, rafts, peers, batch = _pair(nmax, GC.scenarios(), votes=votes, apps=True)
    assert pair.eng.egress_mode() == (7 if votes else 5)
    snap = _before(pair)
    pair.step(batch, ctx=f"logterm nmax={nmax}")
    want = _expect(pair, snap, peers, rafts, votes=votes)
    res = _egress(pair.eng, 4096)
    _check(res, want, f"logterm nmax={nmax}")
    assert _flag_map(want, cases) == {c["name"]: c["flagged"] for c in cases if c["flagged"]}
    assert {k.split("/")[0] for k in _flag_map(want, cases)} == set(GC.FLAGGED)
    name = [c["name"] for c in cases]
    per = lambda s: [(r[7], r[6]) for r in want if is_app(r) and name[r[0]] == s]  # noqa: E731
    assert per(f"reject-below-boundary/{nmax}") == [(2, 1)] and per(f"walk-down/{nmax}") == [(3, 3), (2, 2), (1, 1)]
    assert per(f"at-snapshot/{nmax}") == [(2, 1)] and per(f"send-then-heartbeat/{nmax}") == [(2, 1)]
    assert len(want) - len(off) == 0 and sum(a != b for a, b in zip(want, off)) == 6 * sum(
        1 for c in cases if c["name"].startswith("walk-down"))
    # the complete messages: record + entries against the oracle's own r.msgs, per group in order
    oracle = [m for m in _step_all(rafts, cases) if votes or m[1] != abi.HB_MSG_VOTE]
    term_of = lambda g, i: rafts[g].term(i)  # noqa: E731
    got, exp = _spliced(res, term_of), _oracle_bytes(oracle, term_of)
    assert set(got) == set(exp)
    k = 0
    for g in exp:
        assert len(got[g]) == len(exp[g]), name[g]
        for a, b in zip(got[g], exp[g]):
            if a is not None:
                assert a == b, (name[g], a.hex(), b.hex())
                k += 1
    assert k == sum(1 for r in want if not r[11] and r[2] != abi.HB_REF_OTHER)


# ---- 2. rule (i) by a drop ------------------------------------------------------------------------
def test_ring_of_8_drops_the_run_of_the_early_send():
    pair, cases, rafts, peers, batch = _pair(7, GC.ring_drop_cases(), compact=True, hold=True, votes=True, apps=True)
    G = len(cases)
    assert all(pair.eng.log_capacity(g)[1] == abi.HB_TERM_RING_MIN for g in range(G))
    snap = _before(pair)
    assert all(len(snap[1][g]) == 7 for g in range(G))
    pair.step(batch, ctx="logterm ring drop")
    pair.check_capacity("logterm ring drop")
    assert all(pair.eng.log_capacity(g)[1] == abi.HB_TERM_RING_MIN for g in range(G))
    assert not pair.og.groups()["fault"].any()
    want = _expect(pair, snap, peers, rafts)
    for g, c in enumerate(cases):
        first = [r for r in want if r[0] == g and is_app(r)][0]
        assert (first[7], first[6], first[11]) == ((2, 0, True) if c["name"].startswith("drop-early") else (3, 2, False))
    assert _flag_map(want, cases) == {c["name"]: 1 for c in cases if c["flagged"]}
    _check(_egress(pair.eng, 1024), want, "logterm ring drop")


# ---- 3. hb_reserve_log and hb_set_log_bounds between the step and hb_egress ----------------------
def test_reserve_log_and_set_log_bounds_before_egress_change_nothing():
    pair, cases, rafts, peers, batch = _pair(7, GC.scenarios(), compact=True, votes=True, apps=True)
    G = len(cases)
    snap = _before(pair)
    pair.step(batch, ctx="logterm regrow")
    caps = _run_caps(pair)
    want = _expect(pair, snap, peers, rafts, caps=caps)
    assert sum(1 for r in want if is_app(r) and not r[11] and r[7] <= 3) >= 6 * len(GC.SIZES)
    # a regrow of every run ring (k_regrow copies the runs in ring order) ...
    pair.raise_capacity(np.arange(G), 0, np.full(G, 4 * max(caps.values())))
    assert all(pair.eng.log_capacity(g)[1] == 4 * max(caps.values()) for g in range(G))
    # ... and a compaction of every live group at its commit index (k_set_bounds: first and snap only)
    now = pair.og.groups()
    live = np.nonzero((now["fault"] == 0) & (now["committed"] >= now["first_index"]))[0]
    rc, after = pair.compact(live, now["committed"][live], ctx="logterm compact")
    assert (rc == 0).all() and (after["first_index"][live] == now["committed"][live] + 1).all() and len(live) > G // 2
    _check(_egress(pair.eng, 4096), want, "logterm regrow + bounds")


# ---- 4. the cfg2 step: no send is below the boundary, the knob changes nothing -------------------
def test_cfg2_step_with_the_knob_on_is_the_knob_off_output(monkeypatch):
    G, n = 512, 3
    got = []
    for small, knob in (("1", False), ("1", True), ("0", True)):
        monkeypatch.setenv("HB_SMALL_STEP", small)
        g, runs = synth.steady_groups(G, n, seed=523, last_hi=1 << 14)
        pair = _tap(Pair(g, runs, n, 256, max_batch=8 * G, term_runs=True))
        peers = _peers(G, n)
        pair.eng.load_peers(peers)
        pair.eng.set_egress(True, apps=True)
        pair.eng.set_egress_logterm(knob)
        snap = _before(pair)
        pair.step(synth.cfg2_batch(g, 0, seed=521), ctx=f"logterm cfg2 small={small} knob={knob}")
        want = by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF, votes=False))
        assert len(want) == 4 * G and not any(r[11] for r in want)
        res = _egress(pair.eng, len(want) + 3, enc_cap=20000 if small == "0" else None)
        _check(res, want, f"logterm cfg2 small={small} knob={knob}")
        got.append(res)
        pair.eng.close()
    a, cnt = got[0], got[0]["count"]
    oa = np.argsort(a["group"][:cnt], kind="stable")
    for b in got[1:]:
        ob = np.argsort(b["group"][:cnt], kind="stable")
        assert b["count"] == cnt and b["total"] == a["total"]
        for name, _ in FIELDS:
            assert np.array_equal(a[name][:cnt][oa], b[name][:cnt][ob]), name
        assert np.array_equal(a["status"][:cnt][oa], b["status"][:cnt][ob])


# ---- 5. cap inside a broadcast word, and the per-peer chain --------------------------------------
def test_cap_cuts_inside_a_broadcast_word_and_the_per_peer_chain():
    from .test_egress_bin_gpu import _chain
    pair, cases, rafts, peers, batch = _pair(7, GC.scenarios(), votes=True, apps=True)
    snap = _before(pair)
    pair.step(batch, ctx="logterm cap")
    want = _expect(pair, snap, peers, rafts)
    full = _egress(pair.eng, len(want))
    _check(full, want, "logterm cap full")
    n = full["count"]
    grp, idx, typ = full["group"][:n], full["index"][:n], full["info"][:n] & 0xF
    same = (grp[1:] == grp[:-1]) & (idx[1:] == idx[:-1]) & (typ[1:] == abi.HB_MSG_APP) & (typ[:-1] == abi.HB_MSG_APP)
    inner = np.nonzero(same[1:] & same[:-1])[0] + 1
    looked = np.nonzero((typ == abi.HB_MSG_APP) & (idx <= 3) & (full["info"][:n] & abi.HB_OUT_HOST == 0))[0]
    assert len(inner) > 10 and len(looked) >= 6
    for cap in (int(inner[0]), int(inner[len(inner) // 2]), int(looked[0]), int(looked[-1]) + 1, 0):
        part = _egress(pair.eng, cap)
        assert part["count"] == n, cap
        for name, dt in FIELDS:
            assert np.array_equal(part[name][:cap], full[name][:cap]), (cap, name)
            assert (part[name][cap:].view(np.int64 if dt == "<u8" else np.int32) == -1).all(), (cap, name)
        assert part["total"] == int(full["off"][cap]) and np.array_equal(part["off"][:cap + 1], full["off"][:cap + 1])
        assert np.array_equal(part["status"][:cap], full["status"][:cap])
    pool = np.arange(2, 8, dtype=np.uint64)
    pair.eng.set_egress_peers(pool)
    res = _chain(pair.eng, SELF, 2048, len(pool))
    cnt = res["n"]
    assert cnt == n
    order, boff = bin_reference(res["raw"]["to"][:cnt], res["raw"]["info"][:cnt], pool)
    assert np.array_equal(res["bin_off"], boff) and np.array_equal(res["src"][:cnt], order.astype(np.uint32))
    for name, _ in FIELDS:
        assert np.array_equal(res["raw"][name][:cnt], full[name][:cnt]), name
        assert np.array_equal(res["out"][name][:cnt], res["raw"][name][:cnt][order]), name
    assert np.array_equal(res["status"][:cnt], full["status"][:cnt][order])


# ---- 6. both knobs under a finite limit ----------------------------------------------------------
def _limit_pair(nmax, cases, limit, logterm, cut, fwd=False, **mode):
    cases = [c for c in cases if len(c["peers"]) <= nmax]
    rafts = [LC.build(c, limit) for c in cases]
    groups, runs, peers, batch = AC.export(rafts, cases)
    loaded = {g: LC.log_sizes(r) for g, r in enumerate(rafts)}
    pair = _tap(Pair(groups, runs, nmax, 256, max_msg_size=limit, max_batch=4096,
                     term_runs=GC.loaded_runs(groups, runs, cases), sizes=loaded))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, **mode)
    pair.eng.set_egress_limit(cut)
    pair.eng.set_egress_logterm(logterm)
    if fwd:
        pair.eng.set_wire_props(egress=True)
    return pair, cases, rafts, peers, with_descs(batch), loaded


@pytest.mark.parametrize("limit", [13, 1000])
def test_both_knobs_under_a_limit(limit):
    cases = GC.limit_cases() + [dict(c, unloaded=0) for c in LC.scenarios()] + GC.scenarios()[len(AC.scenarios()):]
    pair, cases, rafts, peers, batch, loaded = _limit_pair(7, cases, limit, True, True, votes=True, apps=True)
    assert pair.eng.egress_limit() and pair.eng.egress_logterm() and pair.eng.egress_mode() == 7
    snap = _before(pair)
    pair.step(batch, ctx=f"logterm + limit {limit}")
    want = _expect(pair, snap, peers, rafts, limit=limit, cut=(loaded, batch))
    name = [c["name"] for c in cases]
    for n in GC.SIZES:
        (r,) = [r for r in want if is_app(r) and name[r[0]] == f"probe-below/{n}"]
        assert (r[7], r[6], r[11], r[12], r[10]) == (2, 1, False, True, LC.probe_cut(5 + n, limit, x=2))
        assert [(r[7], r[6], r[11]) for r in want if is_app(r) and name[r[0]] == f"walk-down/{n}"] == \
            [(3, 3, False), (2, 2, False), (1, 1, False)]
    res = _egress(pair.eng, 4096)
    _check(res, want, f"logterm + limit {limit}")
    # the complete messages of the looked-up records against the oracle's
    oracle = _step_all(rafts, cases)
    term_of = lambda g, i: rafts[g].term(i)  # noqa: E731
    got, exp = _spliced(res, term_of), _oracle_bytes(oracle, term_of)
    for n in GC.SIZES:
        for s in (f"probe-below/{n}", f"walk-down/{n}", f"at-snapshot/{n}"):
            g = name.index(s)
            assert got[g] == exp[g] and None not in got[g], s
    pair.eng.close()
    # each knob alone leaves the Probe follower's record to the host
    for logterm, cut in ((True, False), (False, True)):
        pair, cs, rafts, peers, batch, loaded = _limit_pair(7, GC.limit_cases(), limit, logterm, cut, apps=True)
        snap = _before(pair)
        pair.step(batch, ctx=f"logterm={logterm} cut={cut} {limit}")
        if logterm:
            want = _expect(pair, snap, peers, rafts, votes=False, limit=limit)
        else:
            szlo = {g: int(snap[2][g]) for g in range(len(cs))}
            want = by_group(replay_apps_limit(pair.ora_ev, snap[0], snap[1], peers, SELF, limit,
                                              size_table(pair.ora_ev, snap[0], loaded, batch), szlo, votes=False))
        assert [(r[7], r[11]) for r in want if is_app(r)] == [(2, True)] * len(cs)
        _check(_egress(pair.eng, 256), want, f"logterm={logterm} cut={cut} {limit}")
        pair.eng.close()


# ---- 7. with hb_set_wire_props out on: the FWD instantiations -------------------------------------
def _forward_cases():
    """A follower that knows its leader forwards a proposal (HB_EV_PROP_FWD) between two responses."""
    out = []
    for n in GC.SIZES:
        T = 4 + n
        out.append(dict(AC._case("forward", n, "follower", [(1, 1), (2, 1), (3, T - 1), (4, T)], (T, 0, 2),
                                 [AC._m(abi.HB_MSG_HEARTBEAT, 2, T, commit=3), AC._m(abi.HB_MSG_PROP, 1, nents=2),
                                  AC._m(abi.HB_MSG_HEARTBEAT, 2, T, commit=4)]), unloaded=0))
    return out


@pytest.mark.parametrize("mode,limit", [(7, NO_LIMIT), (5, NO_LIMIT), (7, 13), (5, 13)])
def test_forward_records_beside_looked_up_ones(mode, limit):
    votes = bool(mode & 2)
    cases = GC.scenarios() + _forward_cases()
    if limit == NO_LIMIT:
        pair, cases, rafts, peers, batch = _pair(7, cases, votes=votes, apps=True)
        pair.eng.set_wire_props(egress=True)
        cut = None
    else:
        pair, cases, rafts, peers, batch, loaded = _limit_pair(7, cases, limit, True, True, fwd=True, votes=votes,
                                                               apps=True)
        cut = (loaded, batch)
    assert pair.eng.wire_props() == abi.HB_WIRE_PROPS_OUT and pair.eng.egress_mode() == mode
    snap = _before(pair)
    pair.step(batch, ctx=f"logterm forwards mode {mode} limit {limit}")
    caps = _run_caps(pair)
    oldest = ring_oldest(pair.ora_ev, snap[0], snap[1], caps)
    lim = None if cut is None else (size_table(pair.ora_ev, snap[0], cut[0], cut[1]),
                                    {g: int(snap[2][g]) for g in range(len(cases))})
    term_of = lambda g, i: rafts[g].term(i)  # noqa: E731
    whole = by_group(replay_apps_logterm(pair.ora_ev, snap[0], snap[1], peers, SELF, term_of, oldest,
                                         max_msg_size=limit, limit=lim, votes=votes))

    def recs(ev):  # merge_forwards asks for a group's records and for the count of a prefix's
        if not len(ev):
            return []
        g = int(ev["group"][0])
        mine = [r for r in whole if r[0] == g]
        if len(ev) == (pair.ora_ev["group"] == g).sum():
            return mine
        return mine[:len(replay_apps(ev, snap[0], snap[1], peers, SELF, votes=votes))]
    want = PU.merge_forwards(pair.ora_ev, recs, peers, SELF)
    fwd = [r for r in want if r[1] == abi.HB_MSG_PROP]
    # (the stepped-down leader of "stepdown" forwards its later proposal too)
    assert len(fwd) >= len(GC.SIZES) and len(want) == len(whole) + len(fwd)
    assert {cases[r[0]]["name"].split("/")[0] for r in fwd} >= {"forward"}
    assert sum(1 for r in want if is_app(r) and not r[11] and r[7] <= 3 and r[6] in (1, 2, 3)) >= 6 * len(GC.SIZES)
    _check(_egress(pair.eng, 4096), want, f"logterm forwards mode {mode} limit {limit}")


# ---- 8. the knob itself ---------------------------------------------------------------------------
def test_toggling_the_knob_drops_the_step():
    """One handle: the first rejection of the walk-down with the knob off (flagged, as the parent),
    the knob on (count 0 until the next step), the second rejection (LogTerm 2), the knob off
    again, the third (flagged)."""
    cases = [c for c in GC.scenarios() if c["name"].startswith("walk-down")]
    steps = [[dict(c, msgs=c["msgs"][k:k + 1]) for c in cases] for k in range(3)]
    pair, _, rafts, peers, batch = _pair(7, steps[0], knob=False, votes=True, apps=True)
    eng = pair.eng
    for k, knob in enumerate((False, True, False)):
        if k:
            eng.set_egress_logterm(knob)
            assert eng.egress_logterm() == knob and eng.egress_mode() == 7
            res = _egress(eng, 64)
            assert (res["count"], res["total"], int(res["off"][0])) == (0, 0, 0)
            assert (res["group"].view(np.int32) == -1).all()
            _, _, _, batch = AC.export(rafts, steps[k])
        snap = _before(pair)
        pair.step(batch, ctx=f"logterm toggle step {k}")
        for r, c in zip(rafts, steps[k]):
            r.Step(AC.oracle_msg(c["msgs"][0]))
            r.readMessages()
        if knob:
            want = _expect(pair, snap, peers, rafts)
        else:
            want = by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF))
        assert [(r[7], r[6], r[11]) for r in want if is_app(r)] == [(3 - k, 2 if knob else 0, not knob)] * len(cases)
        _check(_egress(eng, 64), want, f"logterm toggle step {k}")
        eng.set_egress_logterm(knob)  # the same value: nothing changes
        assert _egress(eng, 64)["count"] == len(want)
    # with egress off the knob is only remembered
    eng.set_egress(False)
    eng.set_egress_logterm(True)
    assert eng.egress_logterm() and eng.egress_mode() == 0 and not eng.egress_limit()
    eng.set_egress_logterm(False)
    assert not eng.egress_logterm()


@pytest.mark.parametrize("mode", [1, 3])
def test_knob_on_without_append_mode_changes_nothing(mode):
    pair, cases, rafts, peers, batch = _pair(5, GC.scenarios(), votes=mode == 3)
    assert pair.eng.egress_mode() == mode and pair.eng.egress_logterm()
    snap = _before(pair)
    ev, _, _ = pair.step(batch, ctx=f"logterm mode {mode}")
    assert (ev["type"] == abi.HB_EV_APP).sum() > 50
    res = _egress(pair.eng, 2048)
    if mode == 1:
        _check_plain(res, by_group(replay(pair.ora_ev, snap[0], peers, SELF)), "logterm mode 1")
    else:
        _check_votes(res, by_group(replay_votes(pair.ora_ev, snap[0], snap[1], peers, SELF)), "logterm mode 3")
    assert not ((res["info"][:res["count"]] & 0xF) == abi.HB_MSG_APP).any()


def test_election_over_a_tick_and_a_step():
    from .test_egress_gpu import DRAWS
    cases = [dict(c, unloaded=0) for c in AC.election_cases()]
    pair, cases, rafts, peers, _ = _pair(7, cases, votes=True, apps=True)
    timers = np.zeros(len(cases), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
    pair.set_timers(timers, DRAWS)
    snap = _before(pair)
    pair.tick(ctx="logterm election tick")
    want = _expect(pair, snap, peers, rafts)
    assert want and not any(is_app(r) or r[11] for r in want)
    _check(_egress(pair.eng, 256), want, "logterm election tick")
    grants = [dict(c, msgs=c["msgs"][1:]) for c in cases]
    for r in rafts:
        r.draws = DRAWS
        r.r.elapsed = 20
        r.tick()
        r.readMessages()
    _, _, _, batch = AC.export(rafts, grants)
    snap = _before(pair)
    pair.step(batch, ctx="logterm election grants")
    want = _expect(pair, snap, peers, rafts)
    apps = [r for r in want if is_app(r)]
    assert len(apps) == sum(len(c["peers"]) - 1 for c in cases) and not any(r[11] for r in apps)
    assert want == by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF))  # every send is at the boundary
    _check(_egress(pair.eng, 256), want, "logterm election grants")


# ---- 9. wide values -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.WIDE)
def test_wide_values(name):
    B, T = base(name, delta=3, eps=2)
    pair, cases, rafts, peers, batch = _pair(7, GC.below_cases(), lifted=(B, T), votes=True, apps=True)
    snap = _before(pair)
    pair.step(batch, ctx=f"logterm wide {name}")
    want = _expect(pair, snap, peers, rafts, lifted=(B, T))
    apps = [r for r in want if is_app(r)]
    assert len(apps) == 4 * len(GC.SIZES) and not any(r[11] for r in apps)
    assert sorted({r[7] - B for r in apps}) == [1, 2, 3] and all(T < r[6] <= T + 3 for r in apps)
    oracle = _lift_expected(_step_all(rafts, cases), B, T)
    assert [(r[7], r[6]) for r in apps] == [(m[7], m[6]) for m in oracle if m[1] == abi.HB_MSG_APP]
    _check(_egress(pair.eng, 256), want, f"logterm wide {name}")


# ---- 10. the loopback: a catch-up that never touches the host -------------------------------------
def test_loopback_catch_up_below_the_boundary(monkeypatch):
    """A leader whose follower 2 rejected the probe at the boundary (4) with its last index as the
    hint, and a follower engine holding that follower: its log ends at 2 (one run below the
    boundary's) or at 1 (two runs below).  The leader steps the rejection; the resend travels
    hb_egress -> hb_egress_bin -> hb_encode_ents -> hb_peer_spans -> hb_frame -> hb_unframe ->
    hb_decode_follow -> hb_step without a record for the host, and the follower equals its
    oracle, caught up to the leader's last index."""
    from . import wire_util as W
    from .encode_ents_util import encode_ents_reference, log_source, records_of
    from .ingest_util import follow_reference
    from .parity_util import assert_events_equal, assert_groups_equal
    from .test_encode_ents_gpu import _source
    from .cluster_util import receive as _receive, send_chain as _send_chain
    from .test_frame_gpu import _build_dir, _dev, _host, _ids
    from .test_ingest_gpu import _with_sentinel
    monkeypatch.delenv("HB_SMALL_STEP", raising=False)
    n, K = 3, 20
    T = 4 + n
    log = [(1, 1), (2, 2), (3, 3), (4, T)]
    hints = [2 if k % 2 == 0 else 1 for k in range(K)]
    lcases = [dict(AC._case(f"lead{k}", n, "leader", log, (T, 0, 1), [AC._rej(2, T + 1, 4, h)]), unloaded=0)
              for k, h in enumerate(hints)]
    lead, lcases, lrafts, lpeers, lbatch = _pair(n, lcases, apps=True)
    G = len(lcases)
    lead.eng.set_egress_peers(np.array([2, 3], dtype=np.uint64))
    fcases = [dict(AC._case(f"fol{k}", n, "follower", log[:h], (T + 1, 0, 1), []), unloaded=0) for k, h in enumerate(hints)]
    frafts = [AC.build(c) for c in fcases]
    fgroups, fruns, _, _ = AC.export(frafts, [dict(c, msgs=[AC._m(abi.HB_MSG_BEAT, 1)]) for c in fcases])  # (the batch is unused)
    fol = _tap(Pair(fgroups, fruns, n, 256, max_batch=8 * G, term_runs=True))
    fpeers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    fpeers[:, :3] = (2, 1, 3)
    fol.eng.load_peers(fpeers)
    rng = np.random.default_rng(20251)
    gid = _ids(rng, G)
    ldir, ldups = _build_dir(lead.eng, gid)
    fdir, fdups = _build_dir(fol.eng, gid)
    assert ldups == 0 and fdups == 0
    src = log_source(lrafts)  # every leader's whole log, the noop at 5 included
    snap = _before(lead)
    lead.step(lbatch, ctx="logterm loopback rejection")
    want = _expect(lead, snap, lpeers, lrafts, votes=False)
    assert [(r[0], r[3], r[7], r[6], r[10], r[11]) for r in want] == [(g, 2, h, h, 5, False) for g, h in enumerate(hints)]

    ch = _send_chain(lead.eng, 1, 77, 4 * G, 2, _dev(gid), dsrc=_source(src), bytes_per=91 + 4 * 40)
    lead.eng.sync()
    nrec = G
    assert int(ch["count"].item()) == nrec
    bo = _host(ch["bin_off"], np.uint64)
    lo, hi = int(bo[0]), int(bo[1])
    assert (lo, hi) == (0, nrec) and int(bo[2]) == nrec  # everything goes to node 2
    info = ch["out"]["info"][:nrec].cpu().numpy().view(np.uint32)
    st = ch["status"].cpu().numpy()[:nrec]
    assert not (info & abi.HB_OUT_HOST).any() and (info & abi.HB_OUT_ENTS).all()
    assert (st == abi.HB_WIRE_OK).all() and not (st & abi.HB_WIRE_SPLICE).any()
    assert _host(ch["fstat"], np.uint32).tolist() == [0, 0, 0]
    # the follower's oracle steps the reference encoder's bytes of the same records
    recs_np = {name: ch["out"][name][lo:hi].cpu().numpy().view(dt) for name, dt in FIELDS}
    recs = records_of(recs_np, nrec, SELF)
    assert sorted(recs) == sorted(want)
    ref = encode_ents_reference(recs, src)
    assert (ref[2] == abi.HB_WIRE_OK).all()
    rdata, roff, rln = W.pack(ref[0])
    fref = follow_reference(rdata, roff, rln, recs_np["group"], G, np.full(G, n, np.uint32), fpeers)
    ent_cap = sum(5 - h for h in hints)
    assert (fref["status"] == abi.HB_WIRE_OK).all() and fref["n_ent"] == ent_cap
    ob = _with_sentinel(None, fref)
    fol.reserve(ob)
    rx = _receive(fol, 2, ch, 0, 1, fdir, nrec, ent_cap)
    dev_ev, dev_st = fol.eng.events(), fol.eng.stats()
    ora_ev, ora_st = fol.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, "logterm loopback follower")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_ENTRIES] == ent_cap
    fnow = fol.og.groups()
    assert_groups_equal(fol.eng.get_groups(), fnow, "logterm loopback follower")
    assert (fnow["last_index"] == 5).all() and not fnow["fault"].any()
    assert int(_host(rx["fst"], np.uint32)[0]) == abi.HB_FRAME_OK and int(rx["unk"].item()) == 0
    assert (rx["dstatus"].cpu().numpy() == abi.HB_WIRE_OK).all() and int(rx["n_ent"].item()) == ent_cap
    hoff = _host(ch["off"], np.uint64)
    assert ch["data"].cpu().numpy()[int(hoff[lo]):int(hoff[hi])].tobytes() == b"".join(ref[0])
    for g in range(G):  # the follower's log is the leader's
        assert [fol.og.term(g, i) for i in range(1, 6)] == [lrafts[g].term(i) for i in range(1, 6)]
    lead.eng.close()
    fol.eng.close()
