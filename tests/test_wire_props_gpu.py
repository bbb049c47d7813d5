"""GPU parity of forwarded proposals on the wire path (hb_set_wire_props).

Receive side: hb_decode_follow with HB_WIRE_PROPS_IN against tests/props_util.props_reference
(bit-exact), then decode -> step against the oracle.  Send side: hb_egress with
HB_WIRE_PROPS_OUT against tests/props_util.merge_forwards (pinned to the oracle's r.msgs by
tests/test_wire_props_replay.py), through hb_egress_bin, hb_encode, hb_encode_ents and the host
splice.  Then the two together: a follower engine's forwards stepped by a leader engine.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth
from etcd_amd.splice import source_covers, splice

from . import props_util as PU
from . import wire_util as W
from .egress_app_util import marshal, replay_apps, status_of
from .egress_util import replay
from .egress_vote_util import oracle_older_runs
from .ingest_util import follow_reference
from .parity_util import Pair, assert_events_equal, assert_groups_equal
from .test_egress_app_gpu import _check as _check_egress
from .test_egress_gpu import _check as _check_plain, _egress, _tap
from .test_ingest_gpu import BATCH, FILL, _check as _check_decode, _decode, _engine, _mix, _payload, _peers

pytestmark = pytest.mark.gpu

SELF = 1
DATA = (None, 0, 1, 16, 100)
MIX = (0.3, 0.2, 0.5)  # synth.random_groups: leaders, candidates, followers (with a lead inside or outside prs, or none)


def _run(eng, torch, recs, grp, G, peers, ent_cap=None, ctx="", lead=0, props=True, group_n=None):
    """Decode `recs` (after `lead` bytes of junk, so offsets are unaligned) and compare with props_reference."""
    data, off, ln = W.pack(recs)
    if lead:
        data = np.concatenate([np.full(lead, 0x3a, np.uint8), data])
        off = off + np.uint64(lead)
    ent_cap = int(ln.astype(np.uint64).sum()) // 8 if ent_cap is None else ent_cap
    group_n = np.full(G, 3, np.uint32) if group_n is None else group_n
    ref = PU.props_reference(data, off, ln, grp, G, group_n, peers, props=props)
    out, host = _decode(eng, torch, data, off, ln, grp, ent_cap)
    _check_decode(host, ref, len(recs), ent_cap, ctx)
    return out, host, ref, (data, off, ln)


def _prop_mix(n, salt=0):
    """n records cycling through MsgProp (1-3 entries; Data nil, empty, 1, 16, 100 bytes), MsgApp
    with entries, MsgHeartbeat and MsgAppResp."""
    recs = []
    for i in range(n):
        k = i + salt
        kind = k % 5
        if kind in (0, 2):
            ne = 1 + (k // 5) % 3
            recs.append(PU.prop([_payload(DATA[(k + j) % len(DATA)], k + j) for j in range(ne)], to=1, frm=1 + k % 4))
            continue
        t = (None, abi.HB_MSG_APP, None, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_APP_RESP)[kind]
        ne = (k // 5) % 3 if t == abi.HB_MSG_APP else 0
        idx = 1000 + 7 * k
        recs.append(W.gogo_marshal(t, to=1, frm=1 + k % 4, term=5 + k % 3, log_term=4, index=idx, commit=idx - 1,
                                   entries=[(j & 1, 5, idx + 1 + j, _payload(DATA[(k + j) % len(DATA)], k + j))
                                            for j in range(ne)]))
    return recs


# ---- 5. knob off is today -------------------------------------------------------------------
def test_knob_off_decode_is_follow_reference():
    import torch
    G = 8
    eng, _, peers = _engine(G, max_batch=1 << 10)
    assert eng.wire_props() == 0
    recs = [c[0] for c in PU.rule_cases().values()] + _prop_mix(200, salt=1)
    grp = (np.arange(len(recs)) % (G + 1)).astype(np.uint32)
    data, off, ln = W.pack(recs)
    ent_cap = int(ln.astype(np.uint64).sum()) // 8
    ref = follow_reference(data, off, ln, grp, G, np.full(G, 3, np.uint32), peers)
    ok_props = [i for i, r in enumerate(recs) if PU.prop_entries(r) is not None]
    assert len(ok_props) > 80 and (ref["status"][ok_props] == abi.HB_WIRE_HOST).all()
    for bits in (None, dict(egress=True)):  # the default, then the other bit alone
        if bits is not None:
            eng.set_wire_props(**bits)
            assert eng.wire_props() == abi.HB_WIRE_PROPS_OUT
        _, host = _decode(eng, torch, data, off, ln, grp, ent_cap)
        _check_decode(host, ref, len(recs), ent_cap, f"knob off {bits}")
    eng.set_wire_props(decode=True, egress=True)
    assert eng.wire_props() == 3
    eng.set_wire_props()
    assert eng.wire_props() == 0
    _, host = _decode(eng, torch, data, off, ln, grp, ent_cap)
    _check_decode(host, ref, len(recs), ent_cap, "knob back to 0")


@pytest.mark.parametrize("mode", [1, 7])
def test_knob_off_egress_is_the_replay(mode):
    G, nmax = 64, 3
    g, runs, ins = synth.random_groups(G, nmax, seed=401, W=8, state_mix=MIX)
    pair = _tap(Pair(g, runs, nmax, 8, ins=ins, max_batch=1 << 12, term_runs=True))
    peers = _peers(G, nmax)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, votes=bool(mode & 2), apps=bool(mode & 4))
    pair.eng.set_wire_props(decode=True)  # the other bit alone
    snap = (pair.og.groups(), oracle_older_runs(pair.og))
    pair.step(synth.random_batch(g, 600, seed=402), ctx="knob off")
    assert (pair.ora_ev["type"] == abi.HB_EV_PROP_FWD).sum() > 5
    res = _egress(pair.eng, 4096)
    if mode == 1:
        _check_plain(res, sorted(replay(pair.ora_ev, snap[0], peers, SELF), key=lambda r: r[0]), "knob off mode 1")
    else:
        _check_egress(res, sorted(replay_apps(pair.ora_ev, snap[0], snap[1], peers, SELF), key=lambda r: r[0]),
                      "knob off mode 7")
    assert not ((res["info"][:res["count"]] & 0xF) == abi.HB_MSG_PROP).any()


# ---- 6. the rule table on the device --------------------------------------------------------
def test_rule_table_among_ok_neighbours():
    import torch
    from .ingest_util import rule_cases as follow_cases
    G = 4
    eng, _, peers = _engine(G, max_batch=1 << 11)
    eng.set_wire_props(decode=True)
    cases = PU.rule_cases()
    recs, where, grp = [], {}, []
    for i, (name, (rec, _, _)) in enumerate(cases.items()):
        recs += _mix(3, salt=5 * i)[:1 + i % 3]  # MsgApp, MsgHeartbeat, MsgApp: HB_WIRE_OK from any sender
        where[name] = len(recs)
        recs.append(rec)
        grp += [0] * (len(recs) - len(grp))
    where["group past the capacity"] = len(recs)
    recs.append(cases["one entry"][0])
    grp.append(G)
    recs += [c[0] for c in follow_cases().values()] + _mix(5, salt=40)  # the follower rules beside them, unchanged
    grp += [0] * (len(recs) - len(grp))
    grp = np.array(grp, np.uint32)
    _, host, ref, _ = _run(eng, torch, recs, grp, G, peers, ctx="rules", lead=2)
    d0, o0, l0 = W.pack(recs)
    base = follow_reference(d0, o0, l0, grp, G, np.full(G, 3, np.uint32), peers)
    for name, (_, ok, ne) in cases.items():
        k = where[name]
        assert (host["status"][k] == abi.HB_WIRE_OK) == ok, name
        assert ok or host["status"][k] == base["status"][k], name  # exactly as without the bit
        assert int(host["eoff"][k + 1] - host["eoff"][k]) == ne, name
        assert host["status"][k - 1] == abi.HB_WIRE_OK, name
        assert (host["group"][k] == 0xFFFFFFFF) == (not ok), name
        if ok:
            assert host["index"][k] == ne and host["info"][k] & 0xF == abi.HB_MSG_PROP, name
            assert not (host["term"][k] or host["hint"][k] or host["commit"][k]), name
    k = where["group past the capacity"]
    assert host["status"][k] == abi.HB_WIRE_HOST and host["eoff"][k + 1] == host["eoff"][k]
    k = where["from a non-member"]
    assert (host["info"][k] >> 4) & 0xF == abi.HB_SLOT_NONE


# ---- 7. edges of the decode kernels ---------------------------------------------------------
@pytest.mark.parametrize("small", ["1", "0"])
def test_shapes_at_the_edges(monkeypatch, small):
    """tests/test_ingest_gpu.test_shapes_at_the_edges with proposals among the records: one eoff scan
    carries both kinds of run through every n at which the code takes another path, a wave wider than
    its LDS window, one 64 KiB payload among small records, a proposal of 300 entries, and ent_cap
    one short then exact."""
    import torch
    monkeypatch.setenv("HB_SMALL_STEP", small)
    G = 64
    eng, _, peers = _engine(G, max_batch=1 << 15)
    eng.set_wire_props(decode=True)
    for n in (1, 64, 65, 257, 16385):
        recs = _prop_mix(n, salt=n)
        grp = (np.arange(n) % (G + 1)).astype(np.uint32)
        _, host, ref, _ = _run(eng, torch, recs, grp, G, peers, ctx=f"n={n}", lead=n % 16)
        t = ref["info"][:-1] & 0xF
        assert n < 64 or {abi.HB_MSG_PROP, abi.HB_MSG_APP} <= set(t[np.diff(ref["eoff"]) > 0].tolist())
    grp = np.zeros(130, np.uint32)
    # 64 proposals of ~230 bytes: the wave's span is nearly twice its window
    wide = [PU.prop([_payload(200, i)], frm=1 + i % 3) for i in range(130)]
    _, _, ref, _ = _run(eng, torch, wide, grp, G, peers, ctx="wide wave", lead=1)
    assert ref["n_ent"] == 130 and (ref["status"] == abi.HB_WIRE_OK).all()
    # one 64 KiB payload among small records; a proposal of 300 entries
    big = _prop_mix(130, salt=3)
    big[70] = PU.prop([_payload(1, 1), _payload(65536, 2), None])
    big[71] = PU.prop([_payload((None, 0, 3)[j % 3], j) for j in range(300)], frm=3)
    _, _, ref, _ = _run(eng, torch, big, grp, G, peers, ctx="64 KiB payload", lead=3)
    assert (ref["status"][70:72] == abi.HB_WIRE_OK).all() and int(ref["eoff"][72] - ref["eoff"][71]) == 300
    assert ref["index"][71] == 300 and 65536 in (ref["edesc"] & np.uint32(abi.HB_ENT_MAX_DATA)).tolist()
    # ent_cap one short (no per-entry word written; eoff / n_ent written), then exact
    recs = _prop_mix(700, salt=2)
    grp = (np.arange(700) % G).astype(np.uint32)
    data, off, ln = W.pack(recs)
    ref = PU.props_reference(data, off, ln, grp, G, np.full(G, 3, np.uint32), peers)
    ne = ref["n_ent"]
    assert ne > follow_reference(data, off, ln, grp, G, np.full(G, 3, np.uint32), peers)["n_ent"] > 50
    _, host = _decode(eng, torch, data, off, ln, grp, ne - 1)
    _check_decode(host, ref, 700, ne - 1, "one short")
    assert (host["edesc"].view(np.uint8) == FILL).all() and (host["edata"].view(np.uint8) == FILL).all()
    _, host = _decode(eng, torch, data, off, ln, grp, ne)
    _check_decode(host, ref, 700, ne, "exact")


# ---- 8. decode then step, against the oracle ------------------------------------------------
def _roles(now):
    st, lead = now["state"], now["lead"]
    fol = st == abi.HB_STATE_FOLLOWER
    return dict(leader=int((st == abi.HB_STATE_LEADER).sum()), candidate=int((st == abi.HB_STATE_CANDIDATE).sum()),
                led=int((fol & (lead != abi.HB_REF_NONE)).sum()), leaderless=int((fol & (lead == abi.HB_REF_NONE)).sum()))


def _proposals(now, per_group, lens, salt=0):
    """per_group proposals for every group, round-robin: [(group, m.From, [Data, ...])].  The sender
    is a member (this node or another) or, now and then, node 1000."""
    G, out = len(now), []
    for r in range(per_group):
        for g in range(G):
            k = r * G + g + salt
            frm = 1000 if k % 11 == 0 else 1 + k % int(now["n"][g])
            out.append((g, frm, [_payload(lens[(k + j) % len(lens)], k + j) for j in range(1 + k % 3)]))
    return out


def _prop_batch(props, now, sentinel=True):
    """The same proposals as HB_MSG_PROP batch records (what a host packs by hand), plus the sentinel."""
    n = len(props)
    b = dict(group=np.full(n + 1, 0xFFFFFFFF, np.uint32), info=np.zeros(n + 1, np.uint32))
    for k in ("term", "index", "hint", "commit", "eoff"):
        b[k] = np.zeros(n + 1, np.uint64)
    edesc = []
    for i, (g, frm, ents) in enumerate(props):
        slot = frm - 1 if 1 <= frm <= int(now["n"][g]) else abi.HB_SLOT_NONE
        b["group"][i], b["info"][i], b["index"][i], b["eoff"][i] = g, abi.hb_info(abi.HB_MSG_PROP, slot), len(ents), len(edesc)
        edesc += [abi.hb_ent_desc(0 if d is None else len(d), 0, d is not None) for d in ents]
    b["eoff"][n] = len(edesc)
    b["edesc"] = np.array(edesc, np.uint32)
    b["eterm"] = np.zeros(len(edesc), np.uint64)
    b["props"] = None
    return b


@pytest.mark.parametrize("nmax,seed,limit", [(3, 411, abi.HB_NO_LIMIT), (5, 412, abi.HB_NO_LIMIT), (3, 413, 256),
                                              (5, 414, 256)])
def test_decode_then_step(nmax, seed, limit):
    """G = 64 random groups (leaders, followers with and without a lead, candidates) take two
    gogo-marshalled proposals each through hb_decode_follow (sentinel, n_edesc = ent_cap) and
    hb_step: events, stats and every group record are the oracle's, stepped with the same proposals
    as HB_MSG_PROP records.  limit = 256: the leaders' sends are cut by the descriptors the decoder
    wrote (payloads of 0 to 200 bytes)."""
    import torch
    G = 64
    g, runs, ins = synth.random_groups(G, nmax, seed=seed, W=8, state_mix=MIX)
    kw = {} if limit == abi.HB_NO_LIMIT else dict(max_msg_size=limit,
                                                  sizes=synth.window_sizes(g, runs, seed=seed + 1, frac_full=1.0))
    pair = Pair(g, runs, nmax, 8, ins=ins, max_batch=1 << 10, term_runs=True, **kw)
    peers = _peers(G, nmax)
    pair.eng.load_peers(peers)
    pair.eng.set_wire_props(decode=True)
    now = pair.og.groups()
    roles = _roles(now)
    assert min(roles.values()) >= 3, roles
    seen = set()
    for step in range(2):
        props = _proposals(now, 2, (None, 0, 1, 16, 100, 200), salt=step)
        recs = [PU.prop(ents, to=SELF, frm=frm) for _, frm, ents in props]
        grp = np.array([p[0] for p in props], np.uint32)
        ctx = f"props n={nmax} limit={limit} step {step}"
        out, host, ref, _ = _run(pair.eng, torch, recs, grp, G, peers, ctx=ctx, lead=step, group_n=now["n"])
        ob = _prop_batch(props, now)
        assert (ref["status"] == abi.HB_WIRE_OK).all()
        for k in BATCH + ("eoff", "edesc", "eterm"):
            assert np.array_equal(ref[k], ob[k]), k
        ent_cap = len(host["edesc"])
        pair.reserve(ob)
        pair.eng.step_decoded(out, ent_cap)  # b.n = n + 1, n_edesc = ent_cap: no host read of the count
        dev_ev, dev_st = pair.eng.events(), pair.eng.stats()
        ora_ev, ora_st = pair.og.step(ob)
        assert_events_equal(dev_ev, ora_ev, ctx)
        assert np.array_equal(dev_st, ora_st), f"{ctx}: stats dev {dev_st.tolist()} ora {ora_st.tolist()}"
        now = pair.og.groups()
        assert_groups_equal(pair.eng.get_groups(), now, ctx)
        seen |= {int(t) for t in ora_ev["type"]}
        # the fate of proposal i is in the events: x = i
        fate = ora_ev[np.isin(ora_ev["type"], (abi.HB_EV_PROP_FWD, abi.HB_EV_PROP_DROP))]
        assert (fate["x"] < len(props)).all() and (grp[fate["x"].astype(np.int64)] == fate["group"]).all()
    assert seen >= {abi.HB_EV_LAST, abi.HB_EV_PROP_FWD, abi.HB_EV_PROP_DROP, abi.HB_EV_APP}


# ---- 9. egress records ----------------------------------------------------------------------
def _forward_setup(nmax, mode, seed):
    G = 64
    g, runs, ins = synth.random_groups(G, nmax, seed=seed, W=8, state_mix=MIX)
    pair = _tap(Pair(g, runs, nmax, 8, ins=ins, max_batch=1 << 12, term_runs=True))
    peers = _peers(G, nmax)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True, votes=bool(mode & 2), apps=bool(mode & 4))
    pair.eng.set_wire_props(egress=True)
    assert pair.eng.egress_mode() == mode and pair.eng.wire_props() == abi.HB_WIRE_PROPS_OUT
    snap = (pair.og.groups(), oracle_older_runs(pair.og))
    # every device type, dense proposals, and the follower side's messages (their responses lie between the forwards)
    f = synth.follower_messages(snap[0], pair.og.term, 300, seed=seed + 2)
    b = synth.merge_batches(synth.random_batch(g, 600, seed=seed + 1), f, seed=seed + 3)
    pair.step(b, ctx=f"forwards n={nmax} mode {mode}")
    if mode == 1:
        base = lambda e: [r + (False, False) for r in replay(e, snap[0], peers, SELF)]  # noqa: E731
    else:
        base = lambda e: replay_apps(e, snap[0], snap[1], peers, SELF, votes=bool(mode & 2))  # noqa: E731
    return pair, b, peers, PU.merge_forwards(pair.ora_ev, base, peers, SELF)


def _entries_of(b, g, hint):
    """The entries the host holds for a forward: those of the stepped record at arrival `hint`, or
    of the group's dense proposal; Data a function of the place."""
    ne = int(b["props"][g]) if hint == abi.HB_NO_INDEX else int(b["index"][hint])
    salt = g if hint == abi.HB_NO_INDEX else 64 + hint
    return [(0, 0, 0, _payload(DATA[(salt + k) % len(DATA)], salt + k)) for k in range(ne)]


@pytest.mark.parametrize("nmax,mode", [(3, 1), (5, 1), (3, 5), (5, 5), (3, 7), (5, 7)])
def test_forward_records(nmax, mode):
    from .egress_bin_util import bin_reference
    from .test_egress_bin_gpu import _chain
    pair, b, peers, want = _forward_setup(nmax, mode, 420 + 10 * nmax + mode)
    fwd = [r for r in want if r[1] == abi.HB_MSG_PROP]
    assert len(fwd) > 10 and len(want) > len(fwd) + 50
    assert any(r[10] == abi.HB_NO_INDEX for r in fwd) and any(r[10] != abi.HB_NO_INDEX for r in fwd)
    assert any(r[2] == abi.HB_REF_OTHER and r[3] == 0 for r in fwd) and any(r[2] <= abi.HB_REF_SLOT_MAX for r in fwd)
    t = b["info"] & 0xF
    assert all(r[10] == abi.HB_NO_INDEX or (t[r[10]] == abi.HB_MSG_PROP and b["group"][r[10]] == r[0]) for r in fwd)
    res = _egress(pair.eng, 4096)
    _check_egress(res, want, f"forwards n={nmax} mode {mode}")  # columns, count, status, the split bytes
    n = res["count"]
    isf = (res["info"][:n] & 0xF) == abi.HB_MSG_PROP
    assert (res["info"][:n][isf] & abi.HB_OUT_ENTS).all() and not (res["info"][:n][isf] & abi.HB_OUT_HOST).any()
    other = ((res["info"][:n] >> 4) & 0xF) == abi.HB_REF_OTHER
    assert (res["status"][:n][isf & other] == abi.HB_WIRE_HOST).all()
    assert (res["off"][1:n + 1][isf & other] == res["off"][:n][isf & other]).all()
    # the host's splice: the whole MsgProp, byte for byte, and the leader's decoder would take it
    raw, done = res["data"].tobytes(), 0
    for i in np.nonzero(isf & ~other)[0]:
        g, st, hint = int(res["group"][i]), int(res["status"][i]), int(res["hint"][i])
        ents = _entries_of(b, g, hint)
        assert st & abi.HB_WIRE_SPLICE
        msg = splice(raw[int(res["off"][i]):int(res["off"][i + 1])], st, [W._entry(e) for e in ents])
        assert msg == W.gogo_marshal(abi.HB_MSG_PROP, to=int(res["to"][i]), frm=SELF, entries=ents), (i, g)
        assert int(res["to"][i]) == int(peers[g][(int(res["info"][i]) >> 4) & 0xF])
        # (a follower forwards an empty MsgProp too; the leader's host reports that one)
        assert len(PU.prop_entries(msg)) == len(ents) if ents else PU.prop_entries(msg) is None
        done += 1
    assert done > 5
    # a cap that cuts just before and just after a forward record
    p = int(np.nonzero(isf)[0][1])
    for cap in (p, p + 1):
        cut = _egress(pair.eng, cap)
        assert cut["count"] == n
        for name, _ in abi.OUT_BATCH_FIELDS:
            assert np.array_equal(cut[name][:cap], res[name][:cap]), (cap, name)
        assert np.array_equal(cut["off"][:cap + 1], res["off"][:cap + 1])
        assert np.array_equal(cut["status"][:cap], res["status"][:cap])
    # hb_egress_bin moves the record with info and hint intact
    ids = np.arange(1, nmax + 1, dtype=np.uint64)
    pair.eng.set_egress_peers(ids)
    ch = _chain(pair.eng, SELF, 4096, nmax)
    assert ch["n"] == n
    order, boff = bin_reference(ch["raw"]["to"][:n], ch["raw"]["info"][:n], ids)
    assert np.array_equal(ch["bin_off"], boff) and np.array_equal(ch["src"][:n], order.astype(np.uint32))
    for name, _ in abi.OUT_BATCH_FIELDS:
        assert np.array_equal(ch["raw"][name][:n], res[name][:n]), name
        assert np.array_equal(ch["out"][name][:n], res[name][:n][order]), name
    bf = (ch["out"]["info"][:n] & 0xF) == abi.HB_MSG_PROP
    assert bf.sum() == isf.sum() and np.array_equal(ch["status"][:n], res["status"][:n][order])
    for bi in range(nmax):
        sl = slice(int(boff[bi]), int(boff[bi + 1]))
        assert (ch["out"]["to"][sl] == ids[bi]).all()


# ---- 10. hb_encode_ents never covers a proposal ---------------------------------------------
def test_encode_ents_never_covers_a_proposal():
    from .encode_ents_util import build_source, encode_ents_reference
    from .test_encode_ents_gpu import _app, _arrays, _check, _engine as _bare_engine, _run as _encode
    fwd = lambda g, hint, to_ref=1: (g, abi.HB_MSG_PROP, to_ref, 2 if to_ref == 1 else 0, SELF, 0, 0, 0, 0, False,  # noqa: E731
                                     hint, False, True)
    records = [fwd(0, 3), _app(1, 4, 6), fwd(2, abi.HB_NO_INDEX), _app(3, 0, 2), fwd(3, 1), fwd(4, 2, abi.HB_REF_OTHER)]
    ent = lambda g, k: (0, 7, _payload((3, None, 0, 20)[(g + k) % 4], g + k))  # noqa: E731
    # group 0 holds entries 1 .. hint + 1: the coverage rule would pass if the type were ignored
    windows = {0: (1, [ent(0, k) for k in range(4)]), 1: (5, [ent(1, k) for k in range(2)]),
               2: (1, [ent(2, k) for k in range(3)]), 3: (1, [ent(3, k) for k in range(2)]), 4: (1, [ent(4, k) for k in range(3)])}
    src = build_source(windows, 8)
    assert source_covers(0, 3, src["first"][0], src["count"][0], src["start"][0], len(src["edesc"]), src["edesc"],
                         src["edata"], len(src["data"])) is not None
    assert source_covers(0, 1, src["first"][3], src["count"][3], src["start"][3], len(src["edesc"]), src["edesc"],
                         src["edata"], len(src["data"])) is not None
    # the reference: a proposal keeps the split form, everything else is hb_encode_ents' own rule
    recs, st = [], []
    for r in records:
        if r[1] == abi.HB_MSG_PROP:
            recs.append(marshal(r))
            st.append(status_of(r))
        else:
            one = encode_ents_reference([r], src)
            recs.append(one[0][0])
            st.append(int(one[2][0]))
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    st = np.array(st, np.uint8)
    assert st[1] == abi.HB_WIRE_OK and st[3] == abi.HB_WIRE_OK and len(recs[1]) > len(marshal(records[1]))  # the MsgApps are covered
    assert all(st[i] & abi.HB_WIRE_SPLICE for i in (0, 2, 4)) and st[5] == abi.HB_WIRE_HOST
    eng = _bare_engine(8)
    batch = _arrays(records)
    res = _encode(eng, batch, len(records), src, 4096)
    _check(res, (recs, off, st), "encode_ents with proposals")
    plain = _encode(eng, batch, len(records), src, 4096, plain=True)
    for i in (0, 2, 4, 5):  # the bytes and status of hb_encode
        assert plain["status"][i] == st[i]
        assert plain["data"][int(plain["off"][i]):int(plain["off"][i + 1])].tobytes() == recs[i]
    # the split record completes to the whole message
    assert splice(recs[0], st[0], [W._entry((0, 0, 0, b"x"))]) == W.gogo_marshal(abi.HB_MSG_PROP, to=2, frm=SELF,
                                                                               entries=[(0, 0, 0, b"x")])


# ---- 11. loopback: the capability itself ----------------------------------------------------
def test_loopback_follower_to_leader():
    """Two engines hold the same 64 groups at different slots: node 1 leads them, node 2 follows
    with that lead.  The follower steps one proposal per group; its forwards leave through hb_egress
    -> hb_egress_bin -> hb_encode -> hb_peer_spans and the host splice; the leader takes node 1's
    span through hb_decode_follow (the group column from the slot map) and hb_step.  The leader's
    events and groups are those of an oracle leader stepped with the same proposals directly, and
    every decoded descriptor names the payload bytes the follower's host spliced in."""
    import torch
    from .test_egress_bin_gpu import _chain
    G, n = 64, 3
    g, runs = synth.steady_groups(G, n, seed=431, last_hi=1 << 14)
    lead = Pair(g, runs, n, 256, max_batch=8 * G, term_runs=True)
    lpeers = _peers(G, n)  # the leader is node 1 at slot 0; node 2 is its slot 1
    lead.eng.load_peers(lpeers)
    lead.eng.set_wire_props(decode=True)
    # node 2's view: itself at slot 0, the leader (node 1) at slot 1; its slot s holds the leader's group perm[s]
    fg, fruns = synth.follow_groups(G, n, seed=431, last_hi=1 << 14, with_runs=True)
    perm = np.random.default_rng(432).permutation(G)
    fol = _tap(Pair(fg[perm], [fruns[i] for i in perm], n, 256, max_batch=8 * G, term_runs=True))
    fpeers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    fpeers[:, :3] = (2, 1, 3)
    fol.eng.load_peers(fpeers)
    fol.eng.set_egress(True)
    fol.eng.set_wire_props(egress=True)
    fol.eng.set_egress_peers(np.array([1, 3], dtype=np.uint64))
    # the follower steps one proposal per group (from its own clients: m.From = node 2, its slot 0)
    order = np.random.default_rng(433).permutation(G)
    ne = (1 + order % 3).astype(np.uint64)
    data_of = lambda i, k: _payload(DATA[(i + k) % len(DATA)], 7 * i + k)  # noqa: E731
    fb = dict(group=order.astype(np.uint32), info=np.full(G, abi.hb_info(abi.HB_MSG_PROP, 0), np.uint32),
              term=np.zeros(G, np.uint64), index=ne, hint=np.zeros(G, np.uint64), props=None, msg_props=True)
    ev, st, _ = fol.step(fb, ctx="loopback follower")
    assert (ev["type"] == abi.HB_EV_PROP_FWD).sum() == G and st[abi.HB_STAT_ENTRIES] == 0
    res = _chain(fol.eng, 2, 4 * G, 2)
    lo, hi = int(res["bin_off"][0]), int(res["bin_off"][1])  # bin 0: node 1
    assert res["n"] == G and (lo, hi) == (0, G) and int(res["span"][1]) == int(res["off"][G])
    raw = res["data"].tobytes()
    msgs, grp, arrival = [], [], []
    for i in range(lo, hi):
        s, stt, x = int(res["out"]["group"][i]), int(res["status"][i]), int(res["out"]["hint"][i])
        assert res["out"]["info"][i] == (abi.hb_info(abi.HB_MSG_PROP, 1) | abi.HB_OUT_ENTS) and int(fb["group"][x]) == s
        ents = [W._entry((0, 0, 0, data_of(x, k))) for k in range(int(ne[x]))]
        msgs.append(splice(raw[int(res["off"][i]):int(res["off"][i + 1])], stt, ents))
        grp.append(int(perm[s]))  # the slot map: the follower's slot -> the leader's
        arrival.append(x)
    grp = np.array(grp, np.uint32)
    assert sorted(arrival) == list(range(G)) and sorted(grp.tolist()) == list(range(G))
    # the leader decodes the span and steps it
    out, host, ref, (data, off, ln) = _run(lead.eng, torch, msgs, grp, G, lpeers, ctx="loopback decode")
    assert (ref["status"] == abi.HB_WIRE_OK).all() and ref["n_ent"] == int(ne.sum())
    props = [(int(grp[j]), 2, [data_of(x, k) for k in range(int(ne[x]))]) for j, x in enumerate(arrival)]
    ob = _prop_batch(props, lead.og.groups())
    for k in BATCH + ("eoff", "edesc"):
        assert np.array_equal(ref[k], ob[k]), k
    ent_cap = len(host["edesc"])
    lead.reserve(ob)
    lead.eng.step_decoded(out, ent_cap)
    dev_ev, dev_st = lead.eng.events(), lead.eng.stats()
    ora_ev, ora_st = lead.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, "loopback leader")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_ENTRIES] == int(ne.sum())
    now = lead.og.groups()
    assert_groups_equal(lead.eng.get_groups(), now, "loopback leader")
    want_last = g["last_index"].copy()
    want_last[grp] += ne[np.array(arrival)]
    assert np.array_equal(now["last_index"], want_last)
    # every decoded edata / edesc names the payload bytes the follower's host spliced in
    blob = data.tobytes()
    for j, x in enumerate(arrival):
        for k in range(int(ne[x])):
            e = int(host["eoff"][j]) + k
            d, at, pay = int(host["edesc"][e]), int(host["edata"][e]), data_of(x, k)
            assert d == abi.hb_ent_desc(0 if pay is None else len(pay), 0, pay is not None), (j, k)
            assert (at == 0) if pay is None else (at > 0 and blob[at:at + len(pay)] == pay), (j, k)
