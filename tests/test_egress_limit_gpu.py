"""GPU parity of limitSize's cut in wire egress: hb_set_egress_limit on a
handle in append mode with a finite max_msg_size, hb_egress + hb_encode (+ hb_egress_bin,
hb_peer_spans, hb_encode_ents, hb_decode_follow) against tests/egress_limit_util.py, which
tests/test_egress_limit_replay.py pins to the oracle's own r.msgs.

Every scenario goes through parity_util.Pair, so the engine's events and groups are already
compared with the oracle's; the expected records are replay_apps_limit of the oracle's
events, the sizes the test loaded and the batch's descriptors, and the ring's oldest index
as hb_log_capacity and the final last index give it.  Every array, off, status, total and
the bytes are compared exactly (test_egress_app_gpu._check).
"""
import numpy as np
import pytest

from etcd_amd import abi, synth

from . import egress_app_cases as AC
from . import egress_limit_cases as LC
from .egress_limit_cases import cfg2_sized_inputs, ring_scenario
from .compact_util import CompactPair
from .egress_app_util import is_app, replay_apps
from .egress_bin_util import bin_reference
from .egress_limit_util import replay_apps_limit, size_table, szlo_final, with_descs
from .egress_util import by_group
from .egress_vote_util import oracle_older_runs
from .parity_util import Pair
from .test_egress_app_gpu import _check, _oracle_bytes, _spliced
from .test_egress_app_replay import _step_all
from .test_egress_gpu import _egress, _peers, _tap

pytestmark = pytest.mark.gpu

SELF = 1
FIELDS = abi.OUT_BATCH_FIELDS
LIMIT = 150


def _before(pair):
    """What the expectation needs from before a call: the groups, the ring's older term runs and
    the oldest index of every size ring."""
    return pair.og.groups(), oracle_older_runs(pair.og), pair.og.log_info()[:, 1].astype(np.int64)


def _expect(pair, snap, peers, limit, loaded, batch=None, self_id=SELF, votes=True, grouped=True):
    now = pair.og.groups()
    szlo = [szlo_final(snap[2][g], now["last_index"][g], pair.eng.log_capacity(g)[0]) for g in range(len(now))]
    size_of = size_table(pair.ora_ev, snap[0], loaded, batch)
    recs = replay_apps_limit(pair.ora_ev, snap[0], snap[1], peers, self_id, limit, size_of, szlo, votes=votes)
    return by_group(recs) if grouped else recs


def _cfg2_sized(monkeypatch, small, steady, knob, limit=LIMIT, G=300, n=3):
    """The cfg2 step of test_egress_app_gpu.test_max_msg_size under a finite limit."""
    monkeypatch.setenv("HB_SMALL_STEP", small)
    monkeypatch.setenv("HB_FAST_STEADY", steady)
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    g, runs, loaded, b = cfg2_sized_inputs(G, n)
    # (hb_encode's cap bound is max_batch x (nmax + 4): above the 20,000 of the tiled path)
    pair = _tap(Pair(g, runs, n, 256, max_msg_size=limit, max_batch=4096, term_runs=True, sizes=loaded))
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    if knob:
        pair.eng.set_egress_limit(True)
    assert pair.eng.egress_limit() == knob and pair.eng.egress_mode() == 5
    snap = _before(pair)
    pair.step(b, ctx=f"limit cfg2 small={small} steady={steady} knob={knob}", check_inflights=False)
    assert not pair.og.groups()["fault"].any()
    return pair, snap, peers, loaded, b, g


def _last_at_send(pair, snap, peers, votes=False):
    """Per record of the unlimited replay, in the order of by_group: the last index at the send."""
    return [r[10] for r in by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF, votes=votes))]


# ---- 3. the cfg2 step at max_msg_size = 150 -------------------------------------------------
def test_cfg2_step_under_limit_150(monkeypatch):
    got = []
    for small in ("1", "0"):
        for steady in ("1", "0"):
            pair, snap, peers, loaded, b, g = _cfg2_sized(monkeypatch, small, steady, True)
            want = _expect(pair, snap, peers, LIMIT, loaded, b, votes=False)
            # from the reference alone: cut records, whole ones of two or more entries, none flagged
            last = _last_at_send(pair, snap, peers)
            assert len(last) == len(want) and all(is_app(r) for r in want)
            cut = sum(1 for r, l in zip(want, last) if r[12] and r[10] < l)
            whole = [r for r, l in zip(want, last) if r[12] and r[10] == l]
            print(f"limit {LIMIT}: cut {cut}, whole {len(whole)} ({sum(r[10] - r[7] >= 2 for r in whole)} of two or "
                  f"more entries), without entries {sum(not r[12] for r in want)}, flagged {sum(r[11] for r in want)}")
            assert cut >= 100 and sum(r[10] - r[7] >= 2 for r in whole) >= 250 and not any(r[11] for r in want)
            res = _egress(pair.eng, len(want) + 5, enc_cap=20000 if small == "0" else None)
            _check(res, want, f"limit cfg2 small={small} steady={steady}")
            got.append(res)
    a, n = got[0], got[0]["count"]
    oa = np.argsort(a["group"][:n], kind="stable")
    for b_ in got[1:]:
        ob = np.argsort(b_["group"][:n], kind="stable")
        for name, _ in FIELDS:
            assert np.array_equal(a[name][:n][oa], b_[name][:n][ob]), name


def test_cfg2_step_with_the_knob_off_is_the_parent(monkeypatch):
    pair, snap, peers, loaded, b, g = _cfg2_sized(monkeypatch, "1", "1", False)
    want = by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF, max_msg_size=LIMIT, votes=False))
    ents = sum(r[10] > 0 for r in by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF, votes=False)))
    assert sum(r[11] for r in want) == ents > 300 and not any(r[12] for r in want)
    _check(_egress(pair.eng, len(want) + 5), want, "limit cfg2 knob off")
    # the same handle with the knob on, the next step: the cut
    pair.eng.set_egress_limit(True)
    assert pair.eng.egress_limit() and _egress(pair.eng, 64)["count"] == 0
    now = pair.og.groups()
    b2 = synth.cfg2_batch(now, 0, seed=915)
    b2 = synth.attach_entry_descs(b2, len(now), seed=916, max_len=100)
    # (the sizes of what the first step appended: the reference computes them as the device did)
    first = size_table(pair.ora_ev, snap[0], loaded, b)
    loaded2 = {gi: [first(gi, i) for i in range(max(1, int(now["last_index"][gi]) - 3), int(now["last_index"][gi]) + 1)]
               for gi in range(len(now))}
    snap = _before(pair)
    pair.step(b2, ctx="limit cfg2 second step", check_inflights=False)
    want = _expect(pair, snap, peers, LIMIT, loaded2, b2, votes=False)
    assert sum(r[12] for r in want) >= len(now) and not any(r[11] for r in want)
    _check(_egress(pair.eng, len(want) + 5), want, "limit cfg2 knob on, second step")


# ---- 4. the scenario set in one step, and the spliced bytes ---------------------------------
def _scenario_pair(nmax, limit, cases=None, knob=True, **mode):
    cases = [c for c in (LC.scenarios() if cases is None else cases) if len(c["peers"]) <= nmax]
    rafts = [LC.build(c, limit) for c in cases]
    groups, runs, peers, batch = AC.export(rafts, cases)
    loaded = {g: LC.log_sizes(r) for g, r in enumerate(rafts)}
    pair = _tap(Pair(groups, runs, nmax, 256, max_msg_size=limit, max_batch=4096, term_runs=True, sizes=loaded))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, **mode)
    pair.eng.set_egress_limit(knob)
    return pair, cases, rafts, peers, with_descs(batch), loaded


@pytest.mark.parametrize("limit", LC.LIMITS)
@pytest.mark.parametrize("nmax", [3, 5, 7])
def test_scenario_step(nmax, limit):
    pair, cases, rafts, peers, batch, loaded = _scenario_pair(nmax, limit, votes=True, apps=True)
    assert pair.eng.egress_mode() == 7 and pair.eng.egress_limit()
    snap = _before(pair)
    pair.step(batch, ctx=f"limit scenarios nmax={nmax} limit={limit}")
    want = _expect(pair, snap, peers, limit, loaded, batch)
    res = _egress(pair.eng, 4096)
    _check(res, want, f"limit scenarios nmax={nmax} limit={limit}")
    name = [c["name"] for c in cases]
    flagged = {}
    for r in want:
        if is_app(r) and r[11]:
            flagged[name[r[0]]] = flagged.get(name[r[0]], 0) + 1
    assert flagged == {c["name"]: c["flagged"] for c in cases if c["flagged"]}
    assert {k.split("/")[0] for k in flagged} == set(LC.FLAGGED)
    assert sum(r[12] for r in want if is_app(r)) > 15
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


@pytest.mark.parametrize("name", LC.WIDE)
def test_wide_values(name):
    B, _ = LC.wide_base(name)
    for which in (0, 1):
        cases = [c for c in LC.wide_scenarios(name) if len(c["peers"]) == 5]
        limit = LC.wide_limits(name, 5)[which]
        pair, cases, rafts, peers, batch, loaded = _scenario_pair(5, limit, cases=cases, apps=True)
        snap = _before(pair)
        pair.step(batch, ctx=f"limit wide {name} {limit}")
        want = _expect(pair, snap, peers, limit, loaded, batch, votes=False)
        assert [(r[7], r[10]) for r in want if r[0] == 0] == [(B + 5, B + 7 - which)] * 4
        _check(_egress(pair.eng, 256), want, f"limit wide {name} {limit}")


# ---- 5. rule (i): the ring no longer holds cum(x) -------------------------------------------
def test_ring_of_16_drops_the_early_sends():
    g, runs, loaded, batch, limit = ring_scenario()
    G, n = len(g), int(g["n"][0])
    pair = _tap(CompactPair(g, runs, n, 256, hold=True, max_msg_size=limit, max_batch=4096, term_runs=True, sizes=loaded))
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    pair.eng.set_egress_limit(True)
    snap = _before(pair)
    pair.step(batch, ctx="limit ring of 16", check_inflights=False)
    pair.check_capacity("limit ring of 16")
    assert all(pair.eng.log_capacity(gi)[0] == abi.HB_SIZE_RING_MIN for gi in range(G))
    assert not pair.og.groups()["fault"].any()
    want = _expect(pair, snap, peers, limit, loaded, batch, votes=False)
    for gi in range(G):
        mine = [r for r in want if r[0] == gi]
        last0 = int(g["last_index"][gi])
        assert [(r[7] - last0, r[11]) for r in mine] == [(x, x < 9) for x in (0, 6, 12, 18) for _ in range(n - 1)]
    assert any(r[12] and r[10] < r[7] + 6 for r in want)  # late ones are cut
    _check(_egress(pair.eng, len(want) + 3), want, "limit ring of 16")


def test_set_log_bounds_between_the_step_and_egress(monkeypatch):
    """The application compacts after the step and before hb_egress: hb_set_log_bounds moves
    firstIndex and leaves the size ring alone, so the records are the step's."""
    G, n = 200, 3
    g, runs = synth.steady_groups(G, n, seed=931, last_hi=1 << 10)
    loaded = synth.window_sizes(g, runs, seed=932, frac_full=1.0)
    pair = _tap(CompactPair(g, runs, n, 256, max_msg_size=LIMIT, max_batch=4 * G, term_runs=True, sizes=loaded))
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    pair.eng.set_egress_limit(True)
    b = synth.cfg2_batch(g, 0, seed=933)
    b["props"] = np.full(G, 3, np.uint32)
    b["index"] = (g["last_index"][b["group"]] + np.uint64(3)).astype(np.uint64)
    b = synth.attach_entry_descs(b, G, seed=934, max_len=100)
    snap = _before(pair)
    pair.step(b, ctx="limit bounds", check_inflights=False)
    now = pair.og.groups()
    rc, after = pair.compact(np.arange(G), now["committed"], ctx="limit bounds compact")
    assert (rc == 0).all() and (after["first_index"] == now["committed"] + 1).all()
    want = _expect(pair, snap, peers, LIMIT, loaded, b, votes=False)
    assert not any(r[11] for r in want) and sum(r[12] for r in want) >= 2 * G
    _check(_egress(pair.eng, len(want) + 3), want, "limit bounds")


# ---- 6. cap inside a broadcast word, and the per-peer chain ---------------------------------
def test_cap_cuts_inside_a_broadcast_word_and_the_per_peer_chain(monkeypatch):
    from .test_egress_bin_gpu import _chain
    pair, snap, peers, loaded, b, g = _cfg2_sized(monkeypatch, "1", "1", True, G=120, n=7)
    want = _expect(pair, snap, peers, LIMIT, loaded, b, votes=False)
    full = _egress(pair.eng, len(want))
    _check(full, want, "limit cap full")
    n = full["count"]
    grp, idx = full["group"][:n], full["index"][:n]
    same = (grp[1:] == grp[:-1]) & (idx[1:] == idx[:-1])
    inner = np.nonzero(same[1:] & same[:-1])[0] + 1
    cutrec = np.nonzero((full["info"][:n] & abi.HB_OUT_ENTS != 0))[0]
    assert len(inner) > 10 and len(cutrec) > 100
    for cap in (int(inner[0]), int(inner[len(inner) // 2]), int(inner[-1]), 0):
        part = _egress(pair.eng, cap)
        assert part["count"] == n, cap
        for name, dt in FIELDS:
            assert np.array_equal(part[name][:cap], full[name][:cap]), (cap, name)
            assert (part[name][cap:].view(np.int64 if dt == "<u8" else np.int32) == -1).all(), (cap, name)
        assert part["total"] == int(full["off"][cap]) and np.array_equal(part["off"][:cap + 1], full["off"][:cap + 1])
        assert np.array_equal(part["status"][:cap], full["status"][:cap])
    # the per-peer chain: a record moves with its info and hint
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
    for bi in range(len(pool)):
        lo, hi = int(boff[bi]), int(boff[bi + 1])
        assert hi > lo and int(res["span"][bi]) == int(res["off"][lo]) and int(res["span"][bi + 1]) == int(res["off"][hi])
        assert (res["out"]["to"][lo:hi] == pool[bi]).all()


# ---- 7. loopback under limit 150 ------------------------------------------------------------
def test_loopback_under_limit_150(monkeypatch):
    import torch
    from . import wire_util as W
    from .encode_ents_util import build_source, encode_ents_reference, records_of
    from .ingest_util import follow_reference
    from .parity_util import assert_events_equal, assert_groups_equal
    from .test_encode_ents_gpu import _source
    from .test_ingest_gpu import _with_sentinel
    G, n = 300, 3
    lead, snap, peers, loaded, b, g = _cfg2_sized(monkeypatch, "1", "1", True)
    want = _expect(lead, snap, peers, LIMIT, loaded, b, votes=False, grouped=False)
    last = [r[10] for r in replay_apps(lead.ora_ev, snap[0], snap[1], peers, SELF, votes=False)]
    to2 = [(r, l) for r, l in zip(want, last) if r[3] == 2]
    assert sum(1 for r, l in to2 if r[12] and r[10] < l) >= 40 and not any(r[11] for r, _ in to2)
    lead.eng.set_egress_peers(np.array([2, 3], dtype=np.uint64))
    # every log covered: the entries the step proposed, as the batch's descriptors describe them
    rng = np.random.default_rng(917)
    win = {}
    for gi in range(G):
        d = b["edesc"][int(b["peoff"][gi]):int(b["peoff"][gi]) + int(b["props"][gi])]
        win[gi] = (int(g["last_index"][gi]) + 1,
                   [(int(x >> 30) & 1, int(g["term"][gi]),
                     bytes(rng.integers(0, 256, int(x) & abi.HB_ENT_MAX_DATA, dtype=np.uint8)) if x >> 31 else None)
                    for x in d.tolist()])
    src = build_source(win, G)
    assert np.array_equal(src["edesc"], b["edesc"])
    dsrc = _source(src)
    fg, fruns = synth.follow_groups(G, n, seed=911, last_hi=1 << 12, with_runs=True)
    assert np.array_equal(fg["last_index"], g["last_index"]) and np.array_equal(fg["term"], g["term"])
    fol = _tap(Pair(fg, fruns, n, 256, max_batch=8 * G, term_runs=True))
    fpeers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    fpeers[:, :3] = (2, 1, 3)
    fol.eng.load_peers(fpeers)
    cap = 8 * G
    t = lambda dt, fill, k=cap: torch.full((max(k, 1),), fill, dtype=dt, device="cuda")  # noqa: E731
    tdt = {"<u4": torch.int32, "<u8": torch.int64}
    raw = {name: t(tdt[dt], -1) for name, dt in FIELDS}
    out = {name: t(tdt[dt], -1) for name, dt in FIELDS}
    count, total = t(torch.int64, -1, 1), t(torch.int64, -1, 1)
    bin_off, span = t(torch.int64, -1, 4), t(torch.int64, -1, 4)
    bytes_cap = cap * (91 + 3 * 140)
    data, off, status = t(torch.uint8, 0xAA, bytes_cap), t(torch.int64, -1, cap + 1), t(torch.uint8, 0xEE)
    lead.eng.egress(SELF, raw, cap, count)
    lead.eng.egress_bin(raw, cap, out, bin_off, n_dev=count)
    lead.eng.encode_ents(SELF, out, cap, dsrc, data, off, status, total, n_dev=count)
    lead.eng.peer_spans(off, bin_off, span)
    lead.eng.sync()
    cnt = int(count.item())
    assert cnt == len(want)
    st = status.cpu().numpy()[:cnt]
    assert (st == abi.HB_WIRE_OK).all() and not (st & abi.HB_WIRE_SPLICE).any()
    lo, hi = (int(v) for v in bin_off[:2].cpu().numpy())  # bin 0: node 2
    nrec = hi - lo
    assert nrec == len(to2)
    f_off = off[lo:hi]
    f_len = (off[lo + 1:hi + 1] - off[lo:hi]).to(torch.int32)
    f_grp = out["group"][lo:hi].contiguous()
    # (a follower whose ack names the whole proposal is not sent the rest of a cut one: fewer
    # entries travel than were proposed)
    ent_cap = sum(r[10] - r[7] for r, _ in to2 if r[12])
    assert 0 < ent_cap < int(b["props"].sum())
    fill = lambda k, dt: torch.full((max(k, 1),), -0x11111112, dtype=dt, device="cuda")  # noqa: E731
    fout = {k: fill(nrec + 1, torch.int32 if k in ("group", "info") else torch.int64)
            for k in ("group", "info", "term", "index", "hint", "commit", "eoff")}
    fout["eterm"], fout["edesc"] = fill(ent_cap, torch.int64), fill(ent_cap, torch.int32)
    edata, n_ent = fill(ent_cap, torch.int64), fill(1, torch.int64)
    fstatus = torch.full((nrec,), 0xEE, dtype=torch.uint8, device="cuda")
    # what the follower's oracle steps: the reference encoder's bytes of the same records
    recs_np = {name: out[name][lo:hi].cpu().numpy().view(dt) for name, dt in FIELDS}
    recs = records_of(recs_np, nrec, SELF)
    assert sorted(recs) == sorted(r for r, _ in to2)
    ref = encode_ents_reference(recs, src)
    assert (ref[2] == abi.HB_WIRE_OK).all()
    rdata, roff, rln = W.pack(ref[0])
    fref = follow_reference(rdata, roff, rln, recs_np["group"], G, np.full(G, n, np.uint32), fpeers)
    assert (fref["status"] == abi.HB_WIRE_OK).all() and fref["n_ent"] == ent_cap
    ob = _with_sentinel(None, fref)
    fol.reserve(ob)
    fol.eng.decode_follow(data, f_off, f_len, f_grp, fout, fstatus, ent_cap, edata, n_ent)
    fol.eng.step_decoded(fout, ent_cap)
    dev_ev, dev_st = fol.eng.events(), fol.eng.stats()
    ora_ev, ora_st = fol.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, "limit loopback follower")
    assert np.array_equal(dev_st, ora_st) and 0 < dev_st[abi.HB_STAT_ENTRIES] <= ent_cap
    fnow = fol.og.groups()
    assert_groups_equal(fol.eng.get_groups(), fnow, "limit loopback follower")
    assert (fnow["last_index"] > fg["last_index"]).sum() > G // 2 and not fnow["fault"].any()
    assert (fstatus.cpu().numpy() == abi.HB_WIRE_OK).all() and int(n_ent.item()) == ent_cap
    hoff = off.cpu().numpy().view(np.uint64)
    assert data.cpu().numpy()[int(hoff[lo]):int(hoff[hi])].tobytes() == b"".join(ref[0])


# ---- 8. the knob itself ---------------------------------------------------------------------
@pytest.mark.parametrize("max_msg_size", [abi.HB_NO_LIMIT, 0])
def test_knob_on_without_a_finite_limit_changes_nothing(max_msg_size):
    G, n = 300, 3
    g, runs = synth.steady_groups(G, n, seed=941, last_hi=1 << 12)
    pair = _tap(Pair(g, runs, n, 256, max_msg_size=max_msg_size, max_batch=4 * G, term_runs=True))
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, apps=True)
    pair.eng.set_egress_limit(True)
    assert pair.eng.egress_limit() and pair.eng.egress_mode() == 5
    b = synth.cfg2_batch(g, 0, seed=942)
    b["props"] = (1 + np.arange(G) % 3).astype(np.uint32)
    b["index"] = (g["last_index"][b["group"]] + b["props"][b["group"]]).astype(np.uint64)
    snap = _before(pair)
    pair.step(b, ctx=f"limit knob max_msg_size={max_msg_size}", check_inflights=False)
    want = by_group(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF, max_msg_size=max_msg_size, votes=False))
    assert sum(r[12] for r in want) >= 2 * G and not any(r[11] for r in want)
    _check(_egress(pair.eng, len(want) + 5), want, f"limit knob max_msg_size={max_msg_size}")
    # without append mode the knob changes nothing either (mode 1: tests/egress_util.replay)
    from .egress_util import replay
    from .test_egress_gpu import _check as _check_plain
    pair.eng.set_egress(True)
    assert pair.eng.egress_mode() == 1 and pair.eng.egress_limit()
    snap = _before(pair)
    pair.step(synth.cfg2_batch(pair.og.groups(), 0, seed=943), ctx="limit knob mode 1", check_inflights=False)
    res = _egress(pair.eng, 64)
    _check_plain(res, by_group(replay(pair.ora_ev, snap[0], peers, SELF)), "limit knob mode 1")


def test_toggling_the_knob_drops_the_step(monkeypatch):
    pair, snap, peers, loaded, b, g = _cfg2_sized(monkeypatch, "1", "1", True, G=64)
    want = _expect(pair, snap, peers, LIMIT, loaded, b, votes=False)
    _check(_egress(pair.eng, len(want)), want, "limit toggle before")
    eng = pair.eng
    eng.set_egress_limit(True)  # the same value: nothing changes
    assert _egress(eng, len(want))["count"] == len(want)
    for on in (False, True):
        eng.set_egress_limit(on)
        assert eng.egress_limit() == on and eng.egress_mode() == 5
        res = _egress(eng, 64)
        assert (res["count"], res["total"], int(res["off"][0])) == (0, 0, 0)
        assert (res["group"].view(np.int32) == -1).all()
    # with egress off the knob is only remembered
    eng.set_egress(False)
    eng.set_egress_limit(False)
    eng.set_egress_limit(True)
    assert eng.egress_limit() and eng.egress_mode() == 0


def test_election_over_a_tick_and_a_step_under_a_limit():
    """A campaign by hb_tick, the grants and the win by hb_step, on a handle with a finite limit:
    the new leader's first broadcast carries its noop, one entry whatever the limit."""
    from .test_egress_gpu import DRAWS
    limit = 13
    pair, cases, rafts, peers, _, loaded = _scenario_pair(7, limit, cases=AC.election_cases(), votes=True, apps=True)
    timers = np.zeros(len(cases), dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"], timers["elapsed"] = 10, 1, 20
    pair.set_timers(timers, DRAWS)
    snap = _before(pair)
    pair.tick(ctx="limit election tick")
    want = _expect(pair, snap, peers, limit, loaded)
    assert want and not any(is_app(r) or r[11] for r in want)
    _check(_egress(pair.eng, 256), want, "limit election tick")
    grants = [dict(c, msgs=c["msgs"][1:]) for c in cases]
    for r in rafts:
        r.draws = DRAWS
        r.r.elapsed = 20
        r.tick()
        r.readMessages()
    _, _, _, batch = AC.export(rafts, grants)
    batch = with_descs(batch)
    snap = _before(pair)
    pair.step(batch, ctx="limit election grants")
    want = _expect(pair, snap, peers, limit, loaded, batch)
    apps = [r for r in want if is_app(r)]
    assert len(apps) == sum(len(c["peers"]) - 1 for c in cases) and not any(r[11] for r in apps)
    assert all(r[12] and r[10] == r[7] + 1 for r in apps)
    _check(_egress(pair.eng, 256), want, "limit election grants")
