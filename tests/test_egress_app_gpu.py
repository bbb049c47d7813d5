"""GPU parity of wire egress in append mode: hb_set_egress with
HB_EGRESS_APPS, hb_egress + hb_encode (+ hb_egress_bin, hb_peer_spans) against
the append replay rules (tests/egress_app_util.py, pinned to the oracle's r.msgs
by tests/test_egress_app_replay.py), and the bytes, with the entries spliced in
by etcd_amd.splice, against the reference encoder's restatement
(tests/wire_util.gogo_marshal) of the oracle's own messages.

Every scenario goes through parity_util.Pair, so the engine's events are
already compared with the oracle's; the expected records are replay_apps of
the oracle's events from the oracle's groups (and the older term runs the
device's ring holds) before the step.  The record count, every array of the out
batch, status, off, total and the bytes are compared exactly, records matched
after a stable sort by group as in tests/test_egress_gpu.py.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth
from etcd_amd.splice import splice

from . import egress_app_cases as AC
from . import egress_cases as EC
from . import egress_vote_cases as VC
from .egress_app_util import entry_bytes, entry_tuple, is_app, marshal, out_arrays, replay_apps, status_of
from .egress_bin_util import bin_reference
from .egress_util import by_group, replay
from .egress_vote_util import oracle_older_runs, replay_votes
from .lift_util import lift, lifted
from .parity_util import Pair
from .test_egress_app_replay import _step_all
from .test_egress_gpu import _check as _check_plain, _egress, _peers, _tap
from .test_egress_vote_gpu import _check as _check_votes

pytestmark = pytest.mark.gpu

SELF = 1
FIELDS = abi.OUT_BATCH_FIELDS


def _snap(pair):
    """What the expectation needs from before a step: the groups and the ring's older runs."""
    return pair.og.groups(), oracle_older_runs(pair.og)


def _expect(pair, snap, peers, self_id=SELF, **kw):
    return by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, self_id, **kw))


def _check(res, want, ctx=""):
    """test_egress_gpu._check for append-mode records: HB_OUT_ENTS / HB_OUT_HOST in info, the last
    entry's index in hint, HB_WIRE_SPLICE | prefix_len in status."""
    n = len(want)
    assert res["count"] == n, f"{ctx}: count {res['count']} expected {n}"
    assert n <= res["cap"] and n <= res["enc_cap"]
    order = np.argsort(res["group"][:n], kind="stable")
    exp = out_arrays(want)
    for name, _ in FIELDS:
        d = res[name][:n][order]
        bad = np.nonzero(d != exp[name])[0]
        assert len(bad) == 0, f"{ctx}: {name} differs at sorted {bad[:5]}: dev {d[bad[:5]]} expected {exp[name][bad[:5]]}"
    recs, st = [None] * n, np.zeros(n, np.uint8)
    for j, i in enumerate(order):
        recs[int(i)] = marshal(want[j])
        st[int(i)] = status_of(want[j])
    lens = np.array([len(r) for r in recs], dtype=np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    assert res["total"] == int(off[n]), f"{ctx}: total"
    assert np.array_equal(res["off"][:n + 1], off), f"{ctx}: off"
    bad = np.nonzero(res["status"][:n] != st)[0]
    assert len(bad) == 0, f"{ctx}: status at {bad[:5]}: dev {res['status'][bad[:5]]} expected {st[bad[:5]]}"
    assert (res["status"][n:] == 0xEE).all() and (res["group"][n:].view(np.int32) == -1).all(), f"{ctx}: past n"
    assert ((lens == 0) == (st == abi.HB_WIRE_HOST)).all()
    blob = b"".join(recs)
    assert res["bytes_cap"] >= len(blob)
    got = res["data"][:len(blob)].tobytes()
    if got != blob:
        i = next(k for k in range(n) if got[int(off[k]):int(off[k + 1])] != recs[k])
        raise AssertionError(f"{ctx}: bytes of record {i} (group {res['group'][i]}): "
                             f"{got[int(off[i]):int(off[i + 1])].hex()} expected {recs[i].hex()}")
    assert (res["data"][len(blob):] == 0xAA).all(), f"{ctx}: bytes written past total"


def _spliced(res, term_of):
    """Per group, the complete wire bytes of every unflagged device record in the device's order:
    the record, its entries (egress_app_util.entry_bytes; term_of(g, i) = the entry's term)
    spliced in where the status byte says."""
    n = res["count"]
    raw = res["data"].tobytes()
    out = {}
    for i in range(n):
        info, st = int(res["info"][i]), int(res["status"][i])
        if st == abi.HB_WIRE_HOST:
            assert info & abi.HB_OUT_HOST or (info >> 4) & 0xF == abi.HB_REF_OTHER
            msg = None
        else:
            g = int(res["group"][i])
            ents = []
            if info & abi.HB_OUT_ENTS:
                assert st & abi.HB_WIRE_SPLICE and info & 0xF == abi.HB_MSG_APP
                ents = [entry_bytes(g, j, term_of(g, j)) for j in range(int(res["index"][i]) + 1, int(res["hint"][i]) + 1)]
                assert ents
            else:
                assert st == abi.HB_WIRE_OK
            msg = splice(raw[int(res["off"][i]):int(res["off"][i + 1])], st, ents)
        out.setdefault(int(res["group"][i]), []).append(msg)
    return out


def _oracle_bytes(want, term_of):
    """Per group, gogo_marshal of the oracle's own messages (test_egress_app_replay._expected
    tuples), the entries of a MsgApp being egress_app_util.entry_tuple of its range."""
    from .wire_util import gogo_marshal
    out = {}
    for g, mtype, to_ref, to, frm, term, lt, index, commit, reject, hint, lo, hi in want:
        ents = [entry_tuple(g, j, term_of(g, j)) for j in range(lo, hi + 1)] if hi else []
        out.setdefault(g, []).append(gogo_marshal(mtype, to=to, frm=frm, term=term, log_term=lt, index=index,
                                                  entries=ents, commit=commit, reject=reject, hint=hint))
    return out


def _all_cases(nmax):
    other = [dict(name=s[0], role=s[1], peers=s[2], ents=s[3], hard=s[4], msgs=s[5], setup=(), snapshot=None, flagged=0)
             for s in VC.scenarios() + EC.scenarios()]
    return [c for c in AC.scenarios() + other if len(c["peers"]) <= nmax]


def _scenario_pair(nmax, cases=None, term_runs=True, **mode):
    cases = _all_cases(nmax) if cases is None else cases
    rafts = [AC.build(c) for c in cases]
    groups, runs, peers, batch = AC.export(rafts, cases)
    pair = _tap(Pair(groups, runs, nmax, 256, max_batch=4096, term_runs=term_runs))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, **mode)
    return pair, cases, rafts, peers, batch


# ---- 1. the scenario set in one step, and the spliced bytes ---------------------------------
@pytest.mark.parametrize("nmax", [3, 5, 7])
def test_scenario_step(nmax):
    pair, cases, rafts, peers, batch = _scenario_pair(nmax, votes=True, apps=True)
    assert pair.eng.egress_mode() == 7
    snap = _snap(pair)
    pair.step(batch, ctx=f"app scenarios nmax={nmax}")
    want = _expect(pair, snap, peers)
    res = _egress(pair.eng, 4096)
    _check(res, want, f"app scenarios nmax={nmax}")
    words, _ = pair.eng.event_words()
    types = set((words & np.uint64(0xF)).tolist())
    print("event word types:", sorted(types))
    assert abi.HB_EVW_BCAST in types and abi.HB_EV_APP in types
    apps = [r for r in want if is_app(r)]
    name = [c["name"] for c in cases]
    flagged = {}
    for r in apps:
        if r[11]:
            flagged[name[r[0]]] = flagged.get(name[r[0]], 0) + 1
    assert flagged == {c["name"]: c["flagged"] for c in cases if c["flagged"]}
    assert {k.split("/")[0] for k in flagged} == set(AC.FLAGGED)
    assert sum(r[12] for r in apps) > 10 and sum(not r[12] and not r[11] for r in apps) >= 7  # (n = 3: cfg2 2, commit-moves 4, heartbeat-resp 1)
    # the complete messages: record + entries against the oracle's own r.msgs, per group in order
    oracle = _step_all(rafts, cases)
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


# ---- 2. the election cases: split over two calls, runs never loaded -------------------------
def test_election_split_over_a_tick_and_a_step():
    cases = AC.election_cases()
    from .test_egress_gpu import DRAWS
    pair, cases, rafts, peers, _ = _scenario_pair(7, cases=cases, votes=True, apps=True)
    timers = np.zeros(len(cases), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
    pair.set_timers(timers, DRAWS)
    snap = _snap(pair)
    pair.tick(ctx="app election tick")
    want = _expect(pair, snap, peers)
    assert want and not any(is_app(r) or r[11] for r in want)
    _check(_egress(pair.eng, 256), want, "app election tick")
    grants = [dict(c, msgs=c["msgs"][1:]) for c in cases]
    for r in rafts:
        r.draws = DRAWS
        r.r.elapsed = 20
        r.tick()
        r.readMessages()
    _, _, _, batch = AC.export(rafts, grants)
    snap = _snap(pair)
    assert (snap[0]["term_first"] == abi.HB_NO_INDEX).all()
    pair.step(batch, ctx="app election grants")
    want = _expect(pair, snap, peers)
    apps = [r for r in want if is_app(r)]
    assert len(apps) == sum(len(c["peers"]) - 1 for c in cases) and not any(r[11] for r in apps)
    assert {r[6] for r in apps} == {c["hard"][0] - (2 if c["name"].startswith("win-old") else 0) for c in cases}
    _check(_egress(pair.eng, 256), want, "app election grants")


def test_never_loaded_runs_are_flagged():
    pair, cases, rafts, peers, batch = _scenario_pair(7, cases=AC.election_cases(), term_runs=None, votes=True, apps=True)
    snap = _snap(pair)
    assert not any(snap[1].values())
    pair.step(batch, ctx="app never loaded")
    want = _expect(pair, snap, peers)
    _check(_egress(pair.eng, 256), want, "app never loaded")
    for r in want:
        assert r[11] == cases[r[0]]["name"].startswith("win-old"), r
    assert sum(is_app(r) for r in want) == sum(len(c["peers"]) - 1 for c in cases)


# ---- 3. max_msg_size 0 and finite -----------------------------------------------------------
@pytest.mark.parametrize("max_msg_size", [0, 256])
def test_max_msg_size(max_msg_size):
    G, n = 300, 3
    g, runs = synth.steady_groups(G, n, seed=911, last_hi=1 << 12)
    kw = dict(sizes=synth.window_sizes(g, runs, seed=912, frac_full=1.0)) if max_msg_size else {}
    pair = _tap(Pair(g, runs, n, 256, max_msg_size=max_msg_size, max_batch=4 * G, term_runs=True, **kw))
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    b = synth.cfg2_batch(g, 0, seed=913)
    b["props"] = (1 + np.arange(G) % 3).astype(np.uint32)  # 1 to 3 entries a proposal
    b["index"] = (g["last_index"][b["group"]] + b["props"][b["group"]]).astype(np.uint64)
    if max_msg_size:
        b = synth.attach_entry_descs(b, G, seed=914, max_len=100)
    snap = _snap(pair)
    pair.step(b, ctx=f"app max_msg_size {max_msg_size}", check_inflights=False)
    want = _expect(pair, snap, peers, max_msg_size=max_msg_size, votes=False)
    apps = [r for r in want if is_app(r)]
    assert len(apps) == len(want) >= 4 * G
    if max_msg_size == 0:
        assert not any(r[11] for r in apps) and all(r[10] == r[7] + 1 for r in apps if r[12])
        assert sum(r[12] for r in apps) > 2 * G  # one entry a message: the proposals of 2 and 3 take more sends
    else:
        sent = pair.ora_ev[pair.ora_ev["type"] == abi.HB_EV_APP]
        assert sum(r[11] for r in apps) > G and not any(r[12] for r in apps)
        assert sum(not r[11] for r in apps) > G and len(sent) == len(apps)
    _check(_egress(pair.eng, len(want) + 5), want, f"app max_msg_size {max_msg_size}")


# ---- 4. one cfg2 step through both count paths and both fast-lane paths ---------------------
def _cfg2(monkeypatch, small, steady, n=3, G=512):
    monkeypatch.setenv("HB_SMALL_STEP", small)
    monkeypatch.setenv("HB_FAST_STEADY", steady)
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    g, runs = synth.steady_groups(G, n, seed=520 + n, last_hi=1 << 14)
    pair = _tap(Pair(g, runs, n, 256, max_batch=8 * G, term_runs=True))
    # (hb_encode's cap bound is max_batch x (nmax + 4): 28,672 here, above the 20,000 of the tiled path)
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    assert pair.eng.egress_mode() == 5
    snap = _snap(pair)
    pair.step(synth.cfg2_batch(g, 0, seed=521), ctx=f"app cfg2 small={small} steady={steady}")
    if n == 3:
        assert (pair.eng.steady_waves() > 0) == (steady == "1")
    want = _expect(pair, snap, peers, votes=False)
    assert len(want) == 2 * (n - 1) * G and all(is_app(r) and not r[11] for r in want)
    assert sum(r[12] for r in want) == (n - 1) * G  # half carry the entry, half only the new Commit
    for r in want:
        last0 = int(snap[0]["last_index"][r[0]])
        assert (r[7], r[10], r[8]) in ((last0, last0 + 1, last0), (last0 + 1, 0, last0 + 1))
    res = _egress(pair.eng, len(want) + 3, enc_cap=20000 if small == "0" else None)
    _check(res, want, f"app cfg2 small={small} steady={steady}")
    return res, pair


def test_cfg2_step_both_count_paths_both_lanes(monkeypatch):
    """512 groups x 3, the flagship step: through k_eg_small and, with HB_SMALL_STEP=0, through
    k_eg_count + k_eg_scan; through the steady wave path and, with HB_FAST_STEADY=0, through
    FastLane.  The same records every time."""
    runs = [_cfg2(monkeypatch, s, f)[0] for s in ("1", "0") for f in ("1", "0")]
    a = runs[0]
    n = a["count"]
    oa = np.argsort(a["group"][:n], kind="stable")
    for b in runs[1:]:
        assert b["count"] == n and b["total"] == a["total"]
        ob = np.argsort(b["group"][:n], kind="stable")
        for name, _ in FIELDS:
            assert np.array_equal(a[name][:n][oa], b[name][:n][ob]), name
        assert np.array_equal(a["status"][:n][oa], b["status"][:n][ob])


# ---- 5. cap cuts inside one word's records --------------------------------------------------
def test_cap_cuts_inside_a_broadcast_word(monkeypatch):
    full, pair = _cfg2(monkeypatch, "1", "1", n=7, G=120)
    n = full["count"]
    assert n == 12 * 120
    grp, idx = full["group"][:n], full["index"][:n]
    same = (grp[1:] == grp[:-1]) & (idx[1:] == idx[:-1])
    inner = np.nonzero(same[1:] & same[:-1])[0] + 1  # records with a neighbour of their word on both sides
    assert len(inner) > 10
    for cap in (int(inner[0]), int(inner[len(inner) // 2]), int(inner[-1]), 0):
        part = _egress(pair.eng, cap)
        assert part["count"] == n, cap  # the full number
        for name, dt in FIELDS:
            assert np.array_equal(part[name][:cap], full[name][:cap]), (cap, name)
            assert (part[name][cap:].view(np.int64 if dt == "<u8" else np.int32) == -1).all(), (cap, name)
        assert part["total"] == int(full["off"][cap]) and np.array_equal(part["off"][:cap + 1], full["off"][:cap + 1])
        assert np.array_equal(part["status"][:cap], full["status"][:cap])
        assert part["data"][:part["total"]].tobytes() == full["data"][:part["total"]].tobytes()
        assert (part["data"][part["total"]:] == 0xAA).all()


# ---- 6. wide values -------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("W32", 3), ("W40", 5), ("W62", 7), ("T61", 3)])
def test_wide_values(name, n):
    """The cfg2 step lifted: W40 puts the sends' Index on both sides of 2^40 (a continuation word
    after a broadcast word), W62 and T61 (Index and Term at 2^61) give 9-byte varints."""
    G = 300
    g, runs = synth.steady_groups(G, n, seed=700 + n, last_hi=1 << 12)
    if name == "T61":
        g, runs, _ = lift(g, runs, None, 1 << 61, (1 << 61) - 500)
    else:
        g, runs, _ = lifted(name, g, runs, None, delta=2048, eps=500)
    pair = _tap(Pair(g, runs, n, 256, max_batch=(n - 1) * G, term_runs=True))
    peers = _peers(G, n)
    peers[:, 1:n] |= np.uint64(1 << 63)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    snap = _snap(pair)
    pair.step(synth.cfg2_batch(g, 0, seed=701), ctx=f"app wide {name}")
    want = _expect(pair, snap, peers, votes=False)
    assert len(want) == 2 * (n - 1) * G and all(is_app(r) and not r[11] for r in want)
    res = _egress(pair.eng, len(want))
    _check(res, want, f"app wide {name}")
    words, _ = pair.eng.event_words()
    wt = words & np.uint64(0xF)
    x = np.array([r[7] for r in want], dtype=np.uint64)
    assert (wt == abi.HB_EVW_BCAST).any()
    if name == "W40":
        assert ((x >> np.uint64(40)) != 0).any() and ((x >> np.uint64(40)) == 0).any() and (wt == abi.HB_EVW_CONT).any()
        long_b = (wt[:-1] == abi.HB_EVW_BCAST) & (((words[:-1] >> np.uint64(11)) & np.uint64(1)) == 1)
        assert long_b.any() and (wt[1:][long_b] == abi.HB_EVW_CONT).all()  # EVC_CONT on a broadcast word
    if name in ("W62", "T61"):
        assert (x >> np.uint64(61)).all() and min(r[5] for r in want) >= 1 << 50
        longest = int(np.diff(res["off"][:res["count"] + 1].astype(np.int64)).max())
        # to: 10 bytes; index, commit (2^61): 9; term, logTerm: 8 (2^50) or 9 (just below 2^61)
        assert longest == 28 + 9 + 2 * 8 + 2 * (8 if name == "T61" else 7)
    term_of = lambda gi, i: int(snap[0]["term"][gi])  # noqa: E731  (the proposal's entries carry the Term)
    msgs = _spliced(res, term_of)
    from .wire_util import pb_classes
    M = pb_classes()["Message"]
    seen = 0
    for gi in range(0, G, 37):
        for raw in msgs[gi]:
            p = M.FromString(raw)
            assert p.type == abi.HB_MSG_APP and p.term == int(snap[0]["term"][gi]) and getattr(p, "from") == SELF
            assert [e.Index for e in p.entries] in ([], [p.index + 1])
            seen += len(p.entries)
    assert seen > 0


# ---- 7. modes -------------------------------------------------------------------------------
def test_modes_1_and_3_are_unchanged_and_a_mode_change_drops_the_step():
    got = {}
    for mode, kw in ((1, {}), (3, dict(votes=True)), (7, dict(votes=True, apps=True))):
        pair, cases, rafts, peers, batch = _scenario_pair(5, **kw)
        assert pair.eng.egress_mode() == mode
        snap = _snap(pair)
        ev, _, _ = pair.step(batch, ctx=f"app modes {mode}")
        assert (ev["type"] == abi.HB_EV_APP).sum() > 50
        res = _egress(pair.eng, 2048)
        if mode == 1:    # what hb_set_egress(1) made before the bit existed: tests/egress_util.replay
            _check_plain(res, by_group(replay(pair.ora_ev, snap[0], peers, SELF)), "mode 1")
        elif mode == 3:  # and vote mode: tests/egress_vote_util.replay_votes
            _check_votes(res, by_group(replay_votes(pair.ora_ev, snap[0], snap[1], peers, SELF)), "mode 3")
        n = res["count"]
        info = res["info"][:n]
        if mode != 7:
            assert not ((info & 0xF) == abi.HB_MSG_APP).any() and not (info & abi.HB_OUT_ENTS).any()
            assert not (res["status"][:n] & abi.HB_WIRE_SPLICE).any()
        order = np.argsort(res["group"][:n], kind="stable")
        got[mode] = {name: res[name][:n][order] for name, _ in FIELDS}
    keep = (got[7]["info"] & 0xF) != abi.HB_MSG_APP
    assert 0 < keep.sum() < len(keep)
    for name, _ in FIELDS:  # mode 7 without its MsgApps is mode 3, per group and in order
        assert np.array_equal(got[7][name][keep], got[3][name]), name
    # a mode change on a handle with egress on: the step before it has no matching snapshot
    eng = pair.eng
    for kw, mode in ((dict(votes=True), 3), (dict(apps=True), 5), ({}, 1), (dict(votes=True, apps=True), 7)):
        eng.set_egress(True, **kw)
        assert eng.egress_mode() == mode
        res = _egress(eng, 64)
        assert (res["count"], res["total"], int(res["off"][0])) == (0, 0, 0)
        assert (res["group"].view(np.int32) == -1).all()
    eng.set_egress(True, votes=True, apps=True)  # the same mode again: nothing changes
    # the next step is replayed as usual (every leader takes one more proposal)
    G = len(cases)
    z = np.zeros(G, np.uint64)
    b = dict(group=np.arange(G, dtype=np.uint32), info=np.full(G, abi.hb_info(abi.HB_MSG_PROP, 0), np.uint32), term=z,
             index=np.ones(G, np.uint64), hint=z, props=None, msg_props=True)
    snap = _snap(pair)
    pair.step(b, ctx="app modes second step", check_inflights=False)
    want = _expect(pair, snap, peers)
    assert sum(is_app(r) for r in want) > 20
    _check(_egress(eng, 2048), want, "after a mode change")
    eng.set_egress(False)
    assert eng.egress_mode() == 0
    eng.set_egress(True, apps=True)
    assert _egress(eng, 64)["count"] == 0


# ---- 8. the per-peer chain ------------------------------------------------------------------
def test_per_peer_chain_keeps_the_entries_flag():
    """hb_egress -> hb_egress_bin -> hb_encode -> hb_peer_spans on a cfg2 step, peer rows drawn from a
    pool of 3 node ids: a record moves with its info (HB_OUT_ENTS) and hint, and each peer's span
    with the entries spliced in is that peer's stream of whole messages."""
    from .test_egress_bin_gpu import _chain
    from .wire_util import gogo_marshal
    G, n, self_id = 300, 3, 77
    pool = np.array([21, (1 << 40) | 5, (1 << 63) | 9], dtype=np.uint64)
    rng = np.random.default_rng(909)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    for i in range(G):
        peers[i, :n] = pool[rng.permutation(3)]
    g, runs = synth.steady_groups(G, n, seed=910, last_hi=1 << 14)
    pair = _tap(Pair(g, runs, n, 256, max_batch=4 * G, term_runs=True))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    pair.eng.set_egress_peers(pool)
    snap = _snap(pair)
    pair.step(synth.cfg2_batch(g, 0, seed=911), ctx="app chain")
    want = replay_apps(pair.ora_ev, snap[0], snap[1], peers, self_id, votes=False)
    res = _chain(pair.eng, self_id, 2048, 3)
    cnt, nb = res["n"], 3
    assert cnt == len(want) == 4 * G
    order, boff = bin_reference(res["raw"]["to"][:cnt], res["raw"]["info"][:cnt], pool)
    assert np.array_equal(res["bin_off"], boff) and np.array_equal(res["src"][:cnt], order.astype(np.uint32))
    for name, dt in FIELDS:
        assert np.array_equal(res["out"][name][:cnt], res["raw"][name][:cnt][order]), name  # info and hint unchanged
    assert (res["out"]["info"][:cnt] & abi.HB_OUT_ENTS != 0).sum() == 2 * G
    idl = pool.tolist()
    term_of = lambda gi, i: int(snap[0]["term"][gi])  # noqa: E731
    raw = res["data"].tobytes()
    for b in range(nb):
        lo, hi = int(boff[b]), int(boff[b + 1])
        s0, s1 = int(res["span"][b]), int(res["span"][b + 1])
        assert s0 == int(res["off"][lo]) and s1 == int(res["off"][hi])
        # the peer's stream: every record of its span, completed
        stream = []
        for i in range(lo, hi):
            gi, st = int(res["out"]["group"][i]), int(res["status"][i])
            ents = [entry_bytes(gi, j, term_of(gi, j))
                    for j in range(int(res["out"]["index"][i]) + 1, int(res["out"]["hint"][i]) + 1)] \
                if res["out"]["info"][i] & abi.HB_OUT_ENTS else []
            assert bool(ents) == bool(st & abi.HB_WIRE_SPLICE)
            stream.append((gi, splice(raw[int(res["off"][i]):int(res["off"][i + 1])], st, ents)))
        exp = [(r[0], gogo_marshal(abi.HB_MSG_APP, to=r[3], frm=self_id, term=r[5], log_term=r[6], index=r[7],
                                   entries=[entry_tuple(r[0], j, term_of(r[0], j)) for j in range(r[7] + 1, r[10] + 1)]
                                   if r[12] else [], commit=r[8]))
               for r in want if idl.index(r[3]) == b]
        assert sorted(stream, key=lambda t: t[0]) == sorted(exp, key=lambda t: t[0]), f"bin {b}"  # stable: a group's in order
        assert hi > lo
    assert int(boff[nb]) == cnt and int(res["span"][nb + 1]) == res["total"]
    assert (res["data"][res["total"]:] == 0xAA).all()
