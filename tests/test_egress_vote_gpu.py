"""GPU parity of wire egress in vote mode: hb_set_egress with
HB_EGRESS_VOTES, hb_egress + hb_encode (+ hb_egress_bin, hb_peer_spans) against
the vote replay rules (tests/egress_vote_util.py, pinned to the oracle's r.msgs
by tests/test_egress_vote_replay.py) and the reference encoder's restatement
(tests/wire_util.gogo_marshal).

Every scenario goes through parity_util.Pair, so the engine's events are
already compared with the oracle's; the expected records are replay_votes of
the oracle's events from the oracle's groups (and the older term runs the
device's ring holds) before the step.  The record count, every array of the out
batch, status, off, total and the bytes are compared exactly, records matched
after a stable sort by group as in tests/test_egress_gpu.py.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth

from . import egress_cases as EC
from . import egress_vote_cases as VC
from .egress_bin_util import bin_reference
from .egress_util import by_group, replay
from .egress_vote_util import is_vote, marshal, oracle_older_runs, out_arrays, replay_votes
from .lift_util import lift, lifted
from .parity_util import Pair
from .test_egress_gpu import DRAWS, _check as _check_plain, _egress, _peers, _tap

pytestmark = pytest.mark.gpu

SELF = 1
FIELDS = abi.OUT_BATCH_FIELDS


def _snap(pair):
    """What the expectation needs from before a step: the groups and the ring's older runs."""
    return pair.og.groups(), oracle_older_runs(pair.og)


def _expect(pair, snap, peers, self_id=SELF):
    return by_group(replay_votes(pair.ora_ev, snap[0], snap[1], peers, self_id))


def _check(res, want, ctx=""):
    """test_egress_gpu._check for vote-mode records (a flagged vote: HB_OUT_HOST in info, no bytes)."""
    n = len(want)
    assert res["count"] == n, f"{ctx}: count {res['count']} expected {n}"
    assert n <= res["cap"] and n <= res["enc_cap"]
    order = np.argsort(res["group"][:n], kind="stable")
    exp = out_arrays(want)
    for name, _ in FIELDS:
        d = res[name][:n][order]
        bad = np.nonzero(d != exp[name])[0]
        assert len(bad) == 0, f"{ctx}: {name} differs at sorted {bad[:5]}: dev {d[bad[:5]]} expected {exp[name][bad[:5]]}"
    recs = [None] * n
    for j, i in enumerate(order):
        recs[int(i)] = marshal(want[j])
    lens = np.array([len(r) for r in recs], dtype=np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    assert res["total"] == int(off[n]), f"{ctx}: total"
    assert np.array_equal(res["off"][:n + 1], off), f"{ctx}: off"
    st = np.where(lens == 0, abi.HB_WIRE_HOST, abi.HB_WIRE_OK).astype(np.uint8)
    assert np.array_equal(res["status"][:n], st), f"{ctx}: status"
    assert (res["status"][n:] == 0xEE).all() and (res["group"][n:].view(np.int32) == -1).all(), f"{ctx}: past n"
    blob = b"".join(recs)
    assert res["bytes_cap"] >= len(blob)
    got = res["data"][:len(blob)].tobytes()
    if got != blob:
        i = next(k for k in range(n) if got[int(off[k]):int(off[k + 1])] != recs[k])
        raise AssertionError(f"{ctx}: bytes of record {i} (group {res['group'][i]}): "
                             f"{got[int(off[i]):int(off[i + 1])].hex()} expected {recs[i].hex()}")
    assert (res["data"][len(blob):] == 0xAA).all(), f"{ctx}: bytes written past total"


def _round_trip(res, self_id=SELF):
    """Every unflagged vote's bytes through the protobuf library: the fields it was built from."""
    from .wire_util import pb_classes
    M = pb_classes()["Message"]
    n, k = res["count"], 0
    raw = res["data"].tobytes()
    for i in range(n):
        info = int(res["info"][i])
        if info & 0xF != abi.HB_MSG_VOTE or info & abi.HB_OUT_HOST:
            continue
        p = M.FromString(raw[int(res["off"][i]):int(res["off"][i + 1])])
        assert (p.type, p.to, getattr(p, "from"), p.term, p.logTerm, p.index, p.commit, p.reject, p.rejectHint,
                len(p.entries)) == (abi.HB_MSG_VOTE, int(res["to"][i]), self_id, int(res["term"][i]),
                                    int(res["log_term"][i]), int(res["index"][i]), 0, False, 0, 0), i
        k += 1
    return k


def _word_types(eng):
    words, _ = eng.event_words()
    return set((words & np.uint64(0xF)).tolist())


def _scenarios(nmax):
    return [sc for sc in VC.scenarios() + EC.scenarios() if len(sc[2]) <= nmax]


def _scenario_pair(nmax, votes):
    scs = _scenarios(nmax)
    rafts = [EC.build(sc) for sc in scs]
    groups, runs, peers, batch = EC.export(rafts, scs)
    pair = _tap(Pair(groups, runs, nmax, 256, max_batch=4096, term_runs=True))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, votes=votes)
    return pair, scs, peers, batch


def _old_run(g, sel):
    """The groups `sel` of synth.follow_groups three terms on with no entry of their own Term: the
    last index lies in an older run, the current-term run is empty."""
    g["term"][sel] += np.uint64(3)
    g["term_first"][sel], g["term_last"][sel] = abi.HB_NO_INDEX, 0
    return g


def _hup_batch(G):
    z = np.zeros(G, np.uint64)
    return dict(group=np.arange(G, dtype=np.uint32), info=np.full(G, abi.hb_info(abi.HB_MSG_HUP, 0), np.uint32),
                term=z, index=z, hint=z, props=None)


def _tick_pair(n, G=300, term_runs=True, peers=None):
    """Even groups lead, odd groups follow and are past every election timeout; every third
    follower's last index lies in an older run."""
    g, runs = synth.steady_groups(G, n, seed=300 + n, last_hi=1 << 16)
    f, _ = synth.follow_groups(G, n, seed=300 + n, last_hi=1 << 16, with_runs=True)
    g[1::2] = f[1::2]
    old = np.arange(1, G, 6)
    g = _old_run(g, old)
    if term_runs is not True:
        term_runs = term_runs(g, runs, old)
    pair = _tap(Pair(g, runs, n, 256, max_batch=4096, term_runs=term_runs))
    peers = _peers(G, n) if peers is None else peers
    pair.eng.load_peers(peers)
    timers = np.zeros(G, dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"] = 10, 1
    timers["elapsed"][1::2] = 20
    pair.set_timers(timers, DRAWS)
    return pair, peers, old


# ---- 1. the scenario set in one step --------------------------------------------------------
@pytest.mark.parametrize("nmax", [3, 5, 7])
def test_scenario_step(nmax):
    pair, scs, peers, batch = _scenario_pair(nmax, votes=True)
    snap = _snap(pair)
    _, _, after = pair.step(batch, ctx=f"vote scenarios nmax={nmax}")
    want = _expect(pair, snap, peers)
    res = _egress(pair.eng, 2048)
    _check(res, want, f"vote scenarios nmax={nmax}")
    types = _word_types(pair.eng)
    print("event word types:", sorted(types))
    assert abi.HB_EV_VOTE in types  # the plain vote word (n = 2 at the least)
    name = [sc[0] for sc in scs]
    votes = [r for r in want if is_vote(r)]
    assert {name[r[0]] for r in votes if r[-1]} == {f"{s}/{n}" for s in VC.FLAGGED for n in VC.SIZES if n <= nmax}
    clear = [r for r in votes if not r[-1]]
    assert any(r[6] != r[5] - 1 for r in clear)
    assert any(pair.og.term(r[0], r[7]) != r[6] for r in clear)  # the final log no longer says so
    assert not [r for r in votes if name[r[0]].startswith(("leader-hup", "single"))]
    assert after[name.index("leader-hup/3")]["fault"] == abi.HB_FAULT_LEADER_CAMPAIGN
    assert any(r[2] == abi.HB_REF_OTHER for r in want)
    assert _round_trip(res) == len(clear)


# ---- 2. runs that were never loaded ---------------------------------------------------------
def test_never_loaded_runs_are_flagged():
    scs = [sc for sc in VC.scenarios() if sc[0].split("/")[0] in ("hup-old-run", "hup-cur-run")]
    rafts = [EC.build(sc) for sc in scs]
    groups, runs, peers, batch = EC.export(rafts, scs)
    pair = _tap(Pair(groups, runs, 7, 256, max_batch=4096))  # no hb_load_term_runs
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, votes=True)
    snap = _snap(pair)
    assert not any(snap[1].values())
    pair.step(batch, ctx="never loaded")
    want = _expect(pair, snap, peers)
    _check(_egress(pair.eng, 256), want, "never loaded")
    for r in want:
        assert is_vote(r) and r[-1] == scs[r[0]][0].startswith("hup-old-run")
    assert len(want) == 2 * sum(n - 1 for n in VC.SIZES)


# ---- 3. a tick's campaigns beside the leaders' heartbeats -----------------------------------
@pytest.mark.parametrize("n", [3, 5, 7])
def test_tick_campaigns(n):
    pair, peers, old = _tick_pair(n)
    G = len(peers)
    pair.eng.set_egress(True, votes=True)
    snap = _snap(pair)
    pair.tick(ctx=f"vote tick n={n}")
    want = _expect(pair, snap, peers)
    votes = [r for r in want if is_vote(r)]
    assert len(votes) == (n - 1) * (G // 2) and not any(r[-1] for r in votes)
    assert sum(r[1] == abi.HB_MSG_HEARTBEAT for r in want) == (n - 1) * (G // 2) == len(want) - len(votes)
    assert {r[0] for r in votes if r[6] != r[5] - 1} == set(old.tolist())  # LogTerm from the ring
    words, counts = pair.eng.event_words()
    assert counts[0::2].sum() > 0 and counts[1::2].sum() == 0  # a tick's events sit in the P chunks
    wt = words & np.uint64(0xF)
    assert (wt == abi.HB_EVW_VBCAST).sum() == G // 2 and not (wt == abi.HB_EV_VOTE).any()  # one broadcast word each
    res = _egress(pair.eng, 2048)
    _check(res, want, f"vote tick n={n}")
    assert _round_trip(res) == len(votes)


# ---- 4. a small storm: chunks longer than a tile, both count paths --------------------------
def _storm(small, monkeypatch):
    monkeypatch.setenv("HB_SMALL_STEP", small)
    G, n, K = 512, 7, 4
    g, runs = synth.follow_groups(G, n, seed=441, last_hi=1 << 14, with_runs=True)
    g = _old_run(g, np.arange(0, G, 5))
    pair = _tap(Pair(g, runs, n, 256, max_batch=1 << 13, term_runs=True))
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, votes=True)
    g0 = pair.og.groups()
    # per group: K MsgHeartbeat of its leader and one MsgHup after the first g % (K + 1) of them;
    # the heartbeats after it carry the candidate's Term, so every one of them is answered
    grp, info, term, commit = [], [], [], []
    for k in range(K + 1):
        for i in range(G):
            hup = k == i % (K + 1)
            grp.append(i)
            info.append(abi.hb_info(abi.HB_MSG_HUP, 0) if hup else abi.hb_info(abi.HB_MSG_HEARTBEAT, 1))
            term.append(0 if hup else int(g0["term"][i]) + (1 if k > i % (K + 1) else 0))
            commit.append(0 if hup else int(g0["committed"][i]))
    m = len(grp)
    z = np.zeros(m, np.uint64)
    b = dict(group=np.array(grp, np.uint32), info=np.array(info, np.uint32), term=np.array(term, np.uint64), index=z,
             hint=z, commit=np.array(commit, np.uint64), eoff=z, eterm=np.zeros(0, np.uint64), props=None)
    snap = _snap(pair)
    pair.step(b, ctx=f"vote storm small={small}", check_inflights=False)
    _, counts = pair.eng.event_words()
    assert len(counts) == 4 and (counts[1::2] > 2048).all(), counts
    want = _expect(pair, snap, peers)
    assert sum(is_vote(r) for r in want) == 6 * G and len(want) == (6 + K) * G
    assert not any(r[-1] for r in want)
    res = _egress(pair.eng, len(want) + 3, enc_cap=20000 if small == "0" else None)
    _check(res, want, f"vote storm small={small}")
    return res


def test_small_storm_both_count_paths(monkeypatch):
    """512 groups x 7: a partition's M chunk exceeds the 2,048 words of a tile and the broadcast
    words lie on both sides of the tile boundaries.  Once through k_eg_small and once, with
    HB_SMALL_STEP=0, through k_eg_count + k_eg_scan: the same records."""
    a, b = _storm("1", monkeypatch), _storm("0", monkeypatch)
    n = a["count"]
    assert n == b["count"] and a["total"] == b["total"]
    oa, ob = np.argsort(a["group"][:n], kind="stable"), np.argsort(b["group"][:n], kind="stable")
    for name, _ in FIELDS:
        assert np.array_equal(a[name][:n][oa], b[name][:n][ob]), name


# ---- 5. cap cuts inside one word's records --------------------------------------------------
def test_cap_cuts_inside_a_broadcast_word():
    pair, peers, _ = _tick_pair(7, G=120)
    pair.eng.set_egress(True, votes=True)
    snap = _snap(pair)
    pair.tick(ctx="vote cap")
    want = _expect(pair, snap, peers)
    n = len(want)
    full = _egress(pair.eng, n)
    _check(full, want, "vote cap full")
    vote = (full["info"][:n] & 0xF) == abi.HB_MSG_VOTE
    same = vote[1:] & vote[:-1] & (full["group"][1:n] == full["group"][:n - 1])
    inner = np.nonzero(same[1:] & same[:-1])[0] + 1  # records with a neighbour of their word on both sides
    assert len(inner) > 10
    for cap in (int(inner[0]), int(inner[len(inner) // 2]), int(inner[-1]), 0):
        part = _egress(pair.eng, cap)
        assert part["count"] == n, cap  # the full number
        for name, dt in FIELDS:
            assert np.array_equal(part[name][:cap], full[name][:cap]), (cap, name)
            assert (part[name][cap:].view(np.int64 if dt == "<u8" else np.int32) == -1).all(), (cap, name)
        assert part["total"] == int(full["off"][cap]) and np.array_equal(part["off"][:cap + 1], full["off"][:cap + 1])
        assert part["data"][:part["total"]].tobytes() == full["data"][:part["total"]].tobytes()
        assert (part["data"][part["total"]:] == 0xAA).all()


# ---- 6. wide values -------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,via", [("W32", 3, "step"), ("W40", 2, "step"), ("W40", 5, "tick"), ("W62", 7, "tick"),
                                        ("T61", 3, "step")])
def test_wide_values(name, n, via):
    """Every group of a lifted scenario campaigns (MsgHup in a step, or a tick past its timeout:
    one broadcast word per group): W40 puts the voted Index on both sides of 2^40 (a
    continuation word after the vote word), W62 and T61 (Index and Term at 2^61) give 9-byte
    varints, node ids past 2^63 10-byte ones."""
    G = 300
    g, runs = synth.follow_groups(G, n, seed=600 + n, last_hi=1 << 12, with_runs=True)
    g = _old_run(g, np.arange(0, G, 4))
    if name == "T61":
        g, runs, _ = lift(g, runs, None, 1 << 61, (1 << 61) - 500)
    else:
        g, runs, _ = lifted(name, g, runs, None, delta=2048, eps=500)
    pair = _tap(Pair(g, runs, n, 256, max_batch=4096, term_runs=True))
    peers = _peers(G, n)
    peers[:, 1:n] |= np.uint64(1 << 63)
    pair.eng.load_peers(peers)
    if via == "tick":
        timers = np.zeros(G, dtype=abi.TIMER_DTYPE)
        timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
        pair.set_timers(timers, DRAWS)
    pair.eng.set_egress(True, votes=True)
    snap = _snap(pair)
    if via == "tick":
        pair.tick(ctx=f"vote wide {name}")
    else:
        pair.step(_hup_batch(G), ctx=f"vote wide {name}")
    want = _expect(pair, snap, peers)
    assert len(want) == (n - 1) * G and all(is_vote(r) and not r[-1] for r in want)
    assert any(r[6] != r[5] - 1 for r in want)
    res = _egress(pair.eng, len(want))
    _check(res, want, f"vote wide {name}")
    x = pair.ora_ev["x"][pair.ora_ev["type"] == abi.HB_EV_VOTE]
    types = _word_types(pair.eng)
    print("event word types:", sorted(types))
    # (a tick sends one broadcast word per group; a step's lane may send a word per vote)
    assert abi.HB_EVW_VBCAST in types if via == "tick" else types & {abi.HB_EV_VOTE, abi.HB_EVW_VBCAST}
    if name == "W40":
        assert ((x >> np.uint64(40)) != 0).any() and ((x >> np.uint64(40)) == 0).any() and abi.HB_EVW_CONT in types
    longest = int(np.diff(res["off"][:res["count"] + 1].astype(np.int64)).max())
    if name in ("W62", "T61"):
        assert (x >> np.uint64(61)).all() and abi.HB_EVW_CONT in types
        assert min(r[5] for r in want) >= 1 << 50 and min(r[6] for r in want) >= 1 << 50
        assert longest >= 28 + 9 + 8 + 7 + 7  # to: 10 bytes; index: 9; term, logTerm: 8 at the least
    if name == "T61":
        assert min(r[6] for r in want) >= 1 << 60 and longest == 28 + 9 + 3 * 8
    assert _round_trip(res) == len(want)


# ---- 7. modes -------------------------------------------------------------------------------
def test_mode_1_makes_no_vote_record():
    """hb_set_egress(1) on the vote scenarios: what it made before vote mode existed."""
    pair, scs, peers, batch = _scenario_pair(5, votes=False)
    before = pair.og.groups()
    ev, _, _ = pair.step(batch, ctx="vote scenarios mode 1")
    assert (ev["type"] == abi.HB_EV_VOTE).sum() > 30
    want = by_group(replay(pair.ora_ev, before, peers, SELF))
    res = _egress(pair.eng, 1024)
    _check_plain(res, want, "mode 1")
    assert not ((res["info"][:res["count"]] & 0xF) == abi.HB_MSG_VOTE).any()
    assert not (res["info"][:res["count"]] & abi.HB_OUT_HOST).any()


def test_modes_agree_and_a_mode_change_drops_the_step():
    got = {}
    for votes in (False, True):
        pair, scs, peers, batch = _scenario_pair(5, votes=votes)
        pair.step(batch, ctx=f"vote modes votes={votes}")
        res = _egress(pair.eng, 1024)
        n = res["count"]
        order = np.argsort(res["group"][:n], kind="stable")
        got[votes] = {name: res[name][:n][order] for name, _ in FIELDS}
    keep = (got[True]["info"] & 0xF) != abi.HB_MSG_VOTE
    assert 0 < keep.sum() < len(keep)
    for name, _ in FIELDS:  # mode 3 without its votes is mode 1, per group and in order
        assert np.array_equal(got[True][name][keep], got[False][name]), name
    # a mode change on a handle with egress on: the step before it has no matching snapshot
    eng = pair.eng
    assert eng.egress_mode() == abi.HB_EGRESS_ON | abi.HB_EGRESS_VOTES
    for votes in (False, True):
        eng.set_egress(True, votes=votes)
        assert eng.egress_mode() == abi.HB_EGRESS_ON | (abi.HB_EGRESS_VOTES if votes else 0)
        res = _egress(eng, 64)
        assert (res["count"], res["total"], int(res["off"][0])) == (0, 0, 0)
        assert (res["group"].view(np.int32) == -1).all()
    eng.set_egress(True, votes=True)  # the same mode again: nothing changes
    # the next step is replayed as usual (every group gets MsgHup once more)
    snap = _snap(pair)
    pair.step(_hup_batch(len(scs)), ctx="vote modes second step")
    want = _expect(pair, snap, peers)
    assert sum(is_vote(r) for r in want) > 100
    _check(_egress(eng, 1024), want, "after a mode change")
    eng.set_egress(True, votes=False)
    eng.set_egress(False)
    assert eng.egress_mode() == 0
    eng.set_egress(True, votes=True)
    assert _egress(eng, 64)["count"] == 0


# ---- 8. the per-peer chain ------------------------------------------------------------------
def _tuples(a, n, self_id):
    info = a["info"][:n]
    return [(int(a["group"][i]), int(info[i] & 0xF), int((info[i] >> 4) & 0xF), int(a["to"][i]), self_id,
             int(a["term"][i]), int(a["log_term"][i]), int(a["index"][i]), int(a["commit"][i]),
             bool((info[i] >> 8) & 1), int(a["hint"][i]), bool(info[i] & abi.HB_OUT_HOST)) for i in range(n)]


def test_per_peer_chain_of_a_tick():
    """hb_egress -> hb_egress_bin -> hb_encode -> hb_peer_spans on the tick case, peer rows drawn
    from a pool of 3 node ids; the runs of a few old-run followers are never loaded, so their
    votes are flagged: they land in their peer's bin with length 0."""
    from .test_egress_bin_gpu import _chain
    G, n, self_id = 300, 3, 77
    pool = np.array([21, (1 << 40) | 5, (1 << 63) | 9], dtype=np.uint64)
    rng = np.random.default_rng(808)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    for i in range(G):
        peers[i, :n] = pool[rng.permutation(3)]

    def some_runs(g, runs, old):
        older = synth.older_runs(g, runs)
        return {i: rr for i, rr in older.items() if i not in set(old[::3].tolist())}
    pair, peers, old = _tick_pair(n, G=G, term_runs=some_runs, peers=peers)
    pair.eng.set_egress(True, votes=True)
    pair.eng.set_egress_peers(pool)
    snap = _snap(pair)
    pair.tick(ctx="vote chain tick")
    want = replay_votes(pair.ora_ev, snap[0], snap[1], peers, self_id)
    flagged = {r[0] for r in want if r[-1]}
    assert flagged == set(old[::3].tolist())
    res = _chain(pair.eng, self_id, 1024, 3)
    cnt, nb = res["n"], 3
    assert cnt == len(want) == 2 * G
    order, boff = bin_reference(res["raw"]["to"][:cnt], res["raw"]["info"][:cnt], pool)
    assert np.array_equal(res["bin_off"], boff) and np.array_equal(res["src"][:cnt], order.astype(np.uint32))
    for name, dt in FIELDS:
        assert np.array_equal(res["out"][name][:cnt], res["raw"][name][:cnt][order]), name  # info unchanged
        assert (res["out"][name][cnt:].view(np.int64 if dt == "<u8" else np.int32) == -1).all()
    assert int(boff[nb]) == cnt  # "other" is empty: a flagged record is binned by its `to`
    got = _tuples(res["out"], cnt, self_id)
    idl = pool.tolist()
    ln = np.diff(res["off"][:cnt + 1].astype(np.int64))
    host = np.array([r[-1] for r in got])
    for b in range(nb):
        lo, hi = int(boff[b]), int(boff[b + 1])
        exp = sorted((r for r in want if idl.index(r[3]) == b), key=lambda r: r[0])  # stable: a group's in order
        assert sorted(got[lo:hi], key=lambda r: r[0]) == exp, f"bin {b}"
        blob = b"".join(marshal(r) for r in got[lo:hi])
        s0, s1 = int(res["span"][b]), int(res["span"][b + 1])
        assert res["data"][s0:s1].tobytes() == blob and s1 - s0 == len(blob), f"bin {b}: bytes"
        assert host[lo:hi].any(), f"bin {b} holds a flagged record"
    assert (ln[host] == 0).all() and (res["status"][:cnt][host] == abi.HB_WIRE_HOST).all()
    assert (ln[~host] >= 28).all() and (res["status"][:cnt][~host] == abi.HB_WIRE_OK).all()
    assert int(res["span"][nb + 1]) == res["total"] == int(ln.sum())
    assert (res["data"][res["total"]:] == 0xAA).all()
