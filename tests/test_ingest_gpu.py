"""GPU parity of hb_decode_follow: MsgApp with its entries,
MsgHeartbeat and MsgVote from wire bytes into a device batch, against the CPU
reference (tests/ingest_util.follow_reference: the oracle's Message.Unmarshal,
the contract's rule table, a Python canonical-shape parser), bit-exact; then
decode -> step against the oracle, and two engines talking through their bytes."""
import numpy as np
import pytest

from etcd_amd import abi, synth
from oracle.pyoracle import decode_batch

from . import wire_util as W
from .ingest_util import follow_reference, records_of, rule_cases
from .parity_util import Pair, assert_events_equal, assert_groups_equal

pytestmark = pytest.mark.gpu

BATCH = ("group", "info", "term", "index", "hint", "commit")
DT = dict(group=np.uint32, info=np.uint32, term=np.uint64, index=np.uint64, hint=np.uint64, commit=np.uint64,
          eoff=np.uint64, eterm=np.uint64, edesc=np.uint32)
DATA_LENS = (None, 0, 1, 15, 16, 17, 100, 5000)
EDGES = sorted({v for k in range(1, 10) for v in ((1 << 7 * k) - 1, 1 << 7 * k)} | {1 << 63, (1 << 64) - 1})
FILL = 0xEE


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[a.dtype]
    return torch.from_numpy(a.view(view)).cuda()


def _peers(G, n):
    p = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    p[:, :n] = np.arange(1, n + 1, dtype=np.uint64)  # the oracle's ids: slot + 1
    return p


def _payload(ln, salt):
    return None if ln is None else bytes((salt + 3 * j) & 0xFF for j in range(ln))


def _decode(eng, torch, data, off, ln, grp, ent_cap):
    """decode_follow into arrays pre-filled with 0xEE; returns (device out dict, host view)."""
    n = len(off)
    tdt = {np.uint32: torch.int32, np.uint64: torch.int64}
    full = lambda k, dt: torch.full((max(k, 1),), -0x1111111111111112 if dt is torch.int64 else -0x11111112,  # noqa: E731
                                    dtype=dt, device="cuda")
    out = {k: full(n + 1, tdt[DT[k]]) for k in BATCH + ("eoff",)}
    out["eterm"], out["edesc"] = full(ent_cap, torch.int64), full(ent_cap, torch.int32)
    edata, n_ent = full(ent_cap, torch.int64), full(1, torch.int64)
    status = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    eng.decode_follow(_dev(torch, data), _dev(torch, off), _dev(torch, ln), _dev(torch, grp), out, status, ent_cap,
                      edata, n_ent)
    torch.cuda.synchronize()
    host = {k: out[k].cpu().numpy().view(DT[k]) for k in out}
    host.update(status=status.cpu().numpy(), edata=edata.cpu().numpy().view(np.uint64),
                n_ent=int(n_ent.cpu().numpy().view(np.uint64)[0]))
    return out, host


def _check(host, ref, n, ent_cap, ctx=""):
    assert host["n_ent"] == ref["n_ent"], f"{ctx}: n_ent {host['n_ent']} expected {ref['n_ent']}"
    bad = np.nonzero(host["status"][:n] != ref["status"])[0]
    assert len(bad) == 0, f"{ctx}: status at {bad[:5]}: dev {host['status'][bad[:5]]} ref {ref['status'][bad[:5]]}"
    for k in BATCH + ("eoff",):
        bad = np.nonzero(host[k][:n + 1] != ref[k])[0]
        assert len(bad) == 0, f"{ctx}: {k} at {bad[:5]}: dev {host[k][bad[:5]]} ref {ref[k][bad[:5]]}"
    ne = ref["n_ent"]
    kept = ne if ne <= ent_cap else 0  # past the capacity no entry word is written
    for k in ("eterm", "edesc", "edata"):
        bad = np.nonzero(host[k][:kept] != ref[k][:kept])[0]
        assert len(bad) == 0, f"{ctx}: {k} at {bad[:5]}: dev {host[k][bad[:5]]} ref {ref[k][bad[:5]]}"
        assert (host[k][kept:ent_cap].view(np.uint8) == FILL).all(), f"{ctx}: {k} written past the count"


def _engine(G, n=3, max_batch=1 << 16, seed=3, peers=None):
    from etcd_amd.hipbatch import Engine
    g, _ = synth.steady_groups(G, n, seed=seed, with_runs=False)
    eng = Engine(G, max_replicas=n, max_inflight=8, max_batch=max_batch)
    eng.load_groups(g)
    peers = _peers(G, n) if peers is None else peers
    eng.load_peers(peers)
    return eng, g, peers


def _run(eng, torch, recs, grp, G, peers, ent_cap=None, ctx="", lead=0):
    """Decode `recs` (after `lead` bytes of junk, so offsets are unaligned) and compare with the reference."""
    data, off, ln = W.pack(recs)
    if lead:
        data = np.concatenate([np.full(lead, 0x3a, np.uint8), data])
        off = off + np.uint64(lead)
    ent_cap = int(ln.astype(np.uint64).sum()) // 8 if ent_cap is None else ent_cap
    ref = follow_reference(data, off, ln, grp, G, np.full(G, 3, np.uint32), peers)
    out, host = _decode(eng, torch, data, off, ln, grp, ent_cap)
    _check(host, ref, len(recs), ent_cap, ctx)
    return out, host, ref, (data, off, ln)


# ---- 1. the corpus ------------------------------------------------------------------------------
def test_corpus_bit_exact():
    import torch
    G = 3000
    rng = np.random.default_rng(21)
    peers = _peers(G, 3)
    peers[::7, 1] = 99  # some groups do not know node 2
    eng, now, _ = _engine(G, peers=peers)
    fb = synth.follower_messages(now, lambda g, i: int(now["term"][g]), 9000, seed=22)
    lens = rng.integers(0, len(DATA_LENS), len(fb["eterm"]) + 1)
    eo = np.append(fb["eoff"], len(fb["eterm"])).astype(np.int64)
    good = records_of(fb, peers, lambda i, k: _payload(DATA_LENS[lens[eo[i] + k]], i + k))
    resp, rgrp = W.response_records(G, 1, peers, rng)
    recs = good + list(resp)
    grp = np.concatenate([fb["group"], rgrp])
    pick = rng.permutation(len(recs))[:6000]
    recs += [W.mutate(recs[i], rng)[0] for i in pick]
    grp = np.concatenate([grp, rng.integers(0, G + 50, 6000).astype(np.uint32)])
    order = rng.permutation(len(recs))
    recs, grp = [recs[i] for i in order], grp[order]
    _, host, ref, (data, off, ln) = _run(eng, torch, recs, grp, G, peers, ctx="corpus", lead=5)
    counts = np.bincount(ref["status"], minlength=6)
    assert all(counts[s] > 0 for s in (abi.HB_WIRE_OK, abi.HB_WIRE_HOST, abi.HB_WIRE_ERROR, abi.HB_WIRE_PANIC))
    assert ref["n_ent"] > 5000 and len({int(d) & abi.HB_ENT_MAX_DATA for d in ref["edesc"]}) >= 7
    t = ref["info"][:-1] & 0xF
    ok = ref["status"] == abi.HB_WIRE_OK
    for mt in (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_VOTE) + W.RESP_TYPES:
        assert (ok & (t == mt)).sum() > 100, mt
    assert (ok & (((ref["info"][:-1] >> 4) & 0xF) == abi.HB_SLOT_NONE)).any()
    # hb_decode on the same bytes: still the oracle's, and the two agree wherever it keeps a record from the host
    n = len(recs)
    out = {k: torch.empty(n, dtype=torch.int32 if DT[k] == np.uint32 else torch.int64, device="cuda") for k in BATCH[:5]}
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    eng.decode(_dev(torch, data), _dev(torch, off), _dev(torch, ln), _dev(torch, grp), out, status)
    torch.cuda.synchronize()
    ora = decode_batch(data, off, ln, grp, G, np.full(G, 3, np.uint32), peers)
    st = status.cpu().numpy()
    assert np.array_equal(st, ora["status"])
    for k in BATCH[:5]:
        assert np.array_equal(out[k].cpu().numpy().view(DT[k]), ora[k]), k
    same = st != abi.HB_WIRE_HOST
    assert np.array_equal(host["status"][:n][same], st[same])
    assert set(np.unique(host["status"][:n][~same]).tolist()) == {abi.HB_WIRE_OK, abi.HB_WIRE_HOST}


# ---- 2. shapes at the edges ---------------------------------------------------------------------
def _mix(n, salt=0, ents=(0, 1, 2, 0, 3), lens=(None, 0, 1, 16, 100)):
    """n records cycling through MsgApp (0-3 entries), MsgHeartbeat, MsgVote and MsgAppResp."""
    recs = []
    for i in range(n):
        k = i + salt
        t = (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_APP, abi.HB_MSG_VOTE, abi.HB_MSG_APP_RESP)[k % 5]
        ne = ents[(k // 5) % len(ents)] if t == abi.HB_MSG_APP else 0
        idx = 1000 + 7 * k
        recs.append(W.gogo_marshal(t, to=1, frm=1 + k % 4, term=5 + k % 3, log_term=4, index=idx, commit=idx - 1,
                                   entries=[(j & 1, 5, idx + 1 + j, _payload(lens[(k + j) % len(lens)], k + j))
                                            for j in range(ne)]))
    return recs


@pytest.mark.parametrize("small", ["1", "0"])
def test_shapes_at_the_edges(monkeypatch, small):
    """Every n at which the code takes another path (the empty call, one lane, a full wave, one more,
    a workgroup and one more, the first n past the one-workgroup scan; with HB_SMALL_STEP=0 all of
    them through k_decf_scan + k_decf_write), a wave wider than its LDS window, one 64 KiB payload
    among small records, a record of 300 entries, unaligned offsets."""
    import torch
    monkeypatch.setenv("HB_SMALL_STEP", small)
    G = 64
    eng, _, peers = _engine(G, max_batch=1 << 15)
    for n in (0, 1, 64, 65, 257, 16385):
        recs = _mix(n, salt=n)
        grp = (np.arange(n) % (G + 1)).astype(np.uint32)
        _, host, ref, _ = _run(eng, torch, recs, grp, G, peers, ctx=f"n={n}", lead=n % 16)
        assert n < 64 or ref["n_ent"] > 0
    grp = np.zeros(130, np.uint32)
    # 64 records of ~250 bytes: the wave's span is twice its window
    wide = [W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=2, term=5, log_term=5, index=10 * i, commit=3,
                           entries=[(0, 5, 10 * i + 1, _payload(200, i))]) for i in range(130)]
    _, _, ref, _ = _run(eng, torch, wide, grp, G, peers, ctx="wide wave", lead=1)
    assert ref["n_ent"] == 130 and (ref["status"] == abi.HB_WIRE_OK).all()
    # one 64 KiB payload among small records; a record of 300 entries
    big = _mix(130, salt=3)
    big[70] = W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=2, term=5, log_term=5, index=77, commit=3,
                             entries=[(0, 5, 78, _payload(1, 1)), (1, 5, 79, _payload(65536, 2)), (0, 5, 80, None)])
    big[71] = W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=3, term=5, log_term=5, index=500, commit=3,
                             entries=[(0, 5, 501 + j, _payload((None, 0, 3)[j % 3], j)) for j in range(300)])
    _, _, ref, _ = _run(eng, torch, big, grp, G, peers, ctx="64 KiB payload", lead=3)
    assert (ref["status"][70:72] == abi.HB_WIRE_OK).all() and int(ref["eoff"][72] - ref["eoff"][71]) == 300
    assert 65536 in (ref["edesc"] & np.uint32(abi.HB_ENT_MAX_DATA)).tolist()


def test_past_one_scan_block():
    """More than 1024 workgroups of k_decf_parse, so that k_decf_scan's lanes sum two of them each:
    255 copies of 1031 records, the reference computed for one copy and shifted."""
    import torch
    G, B, K = 64, 1031, 255
    eng, _, peers = _engine(G, max_batch=1 << 19)
    base = _mix(B, salt=1)
    data1, off1, ln1 = W.pack(base)
    grp1 = (np.arange(B) % G).astype(np.uint32)
    r1 = follow_reference(data1, off1, ln1, grp1, G, np.full(G, 3, np.uint32), peers)
    nb, ne1, n = len(data1), r1["n_ent"], B * K
    assert (n + 255) // 256 > 1024 and ne1 > 0
    shift = np.repeat(np.arange(K, dtype=np.uint64), B)
    ref = {k: np.append(np.tile(r1[k][:-1], K), r1[k][-1:]) for k in BATCH}
    ref["status"] = np.tile(r1["status"], K)
    ref["eoff"] = np.append(np.tile(r1["eoff"][:-1], K) + shift * np.uint64(ne1), np.uint64(ne1 * K))
    es = np.repeat(np.arange(K, dtype=np.uint64), ne1) * np.uint64(nb)
    ref["eterm"], ref["edesc"] = np.tile(r1["eterm"], K), np.tile(r1["edesc"], K)
    ref["edata"] = np.where(np.tile(r1["edata"], K) != 0, np.tile(r1["edata"], K) + es, 0).astype(np.uint64)
    ref["n_ent"] = ne1 * K
    data, ln, grp = np.tile(data1, K), np.tile(ln1, K), np.tile(grp1, K)
    off = np.tile(off1, K) + shift * np.uint64(nb)
    ent_cap = ne1 * K + 7
    _, host = _decode(eng, torch, data, off, ln, grp, ent_cap)
    _check(host, ref, n, ent_cap, "past one scan block")


def test_full_width_varints():
    """Term, Index, LogTerm, Commit and the entry Terms take every varint-length edge of a u64 (the
    entries numbered from the Index, mod 2^64) in MsgApp, MsgHeartbeat and MsgVote records; the
    decoded values are the encoded ones."""
    import torch
    G = 64
    eng, _, peers = _engine(G, max_batch=1 << 12)
    E = len(EDGES)
    fields = ("term", "index", "log_term", "commit", "eterm")
    recs, want = [], []
    for t in (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_VOTE):
        for fi, f in enumerate(fields):
            for k, v in enumerate(EDGES):
                kw = {o: EDGES[(k + 3 + 4 * ((fi + j) % 5)) % E] for j, o in enumerate(fields)}
                kw[f] = v
                et = kw.pop("eterm")
                ne = (1, 3, 2)[k % 3] if t == abi.HB_MSG_APP else 0
                ents = [(0, et, (kw["index"] + 1 + j) & ((1 << 64) - 1), _payload((None, 2)[j & 1], j)) for j in range(ne)]
                recs.append(W.gogo_marshal(t, to=1, frm=1 + (k + fi) % 3, entries=ents, **kw))
                want.append((kw["term"], kw["index"], 0 if t == abi.HB_MSG_HEARTBEAT else kw["log_term"],
                             0 if t == abi.HB_MSG_VOTE else kw["commit"], et, ne))
    assert {len(W.varint(v)) for v in EDGES} == set(range(1, 11))
    grp = (np.arange(len(recs)) % G).astype(np.uint32)
    _, host, ref, _ = _run(eng, torch, recs, grp, G, peers, ctx="edges", lead=9)
    assert (ref["status"] == abi.HB_WIRE_OK).all()
    w = np.array([x[:4] for x in want], dtype=np.uint64)
    for j, k in enumerate(("term", "index", "hint", "commit")):
        assert np.array_equal(host[k][:-1], w[:, j]), k
    assert np.array_equal(host["eterm"][:ref["n_ent"]], np.repeat(np.array([x[4] for x in want], np.uint64),
                                                                  [x[5] for x in want]))


# ---- 3. ent_cap one short of the count ----------------------------------------------------------
def test_ent_cap_one_short_then_exact():
    import torch
    G = 64
    eng, _, peers = _engine(G, max_batch=1 << 12)
    recs = _mix(700, salt=2)
    grp = (np.arange(700) % G).astype(np.uint32)
    data, off, ln = W.pack(recs)
    ref = follow_reference(data, off, ln, grp, G, np.full(G, 3, np.uint32), peers)
    ne = ref["n_ent"]
    assert ne > 100
    _, host = _decode(eng, torch, data, off, ln, grp, ne - 1)
    _check(host, ref, 700, ne - 1, "one short")  # count, eoff, status and the batch right; no entry word written
    assert (host["eterm"].view(np.uint8) == FILL).all() and (host["edata"].view(np.uint8) == FILL).all()
    _, host = _decode(eng, torch, data, off, ln, grp, ne)
    _check(host, ref, 700, ne, "exact")
    assert np.array_equal(host["eterm"][:ne], ref["eterm"])
    _, host = _decode(eng, torch, data, off, ln, grp, 0)  # no entry arrays at all
    assert host["n_ent"] == ne and np.array_equal(host["eoff"], ref["eoff"])


def test_argument_checks():
    import torch
    from etcd_amd.hipbatch import HipBatchError
    eng, _, peers = _engine(8, max_batch=64)
    data, off, ln = W.pack(_mix(64))
    with pytest.raises(HipBatchError):  # n + 1 > max_batch: the sentinel needs a record
        _decode(eng, torch, data, off, ln, np.zeros(64, np.uint32), 64)
    out, host = _decode(eng, torch, data[:1], off[:0], ln[:0], np.zeros(0, np.uint32), 0)
    assert host["n_ent"] == 0 and host["eoff"][0] == 0 and host["group"][0] == 0xFFFFFFFF and host["info"][0] == 0
    # ent_cap = 0: eterm / edesc / edata may be NULL (count, eoff, status and the batch are still written);
    # with ent_cap > 0 a NULL entry array is HB_EINVAL, as a NULL batch array or count always is
    recs = _mix(40, salt=1)
    data, off, ln = W.pack(recs)
    grp = np.zeros(40, np.uint32)
    ref = follow_reference(data, off, ln, grp, 8, np.full(8, 3, np.uint32), peers)
    full, _ = _decode(eng, torch, data, off, ln, grp, 64)
    d = [_dev(torch, x) for x in (data, off, ln, grp)]
    bare = {k: torch.zeros(41, dtype=full[k].dtype, device="cuda") for k in BATCH + ("eoff",)}
    status, n_ent = torch.zeros(40, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.decode_follow(d[0], d[1], d[2], d[3], bare, status, 0, None, n_ent)
    torch.cuda.synchronize()
    assert int(n_ent.item()) == ref["n_ent"] > 0 and np.array_equal(status.cpu().numpy(), ref["status"])
    for k in BATCH + ("eoff",):
        assert np.array_equal(bare[k].cpu().numpy().view(DT[k]), ref[k]), k
    ed = torch.zeros(64, dtype=torch.int64, device="cuda")
    for broken in (dict(full, eterm=None), dict(full, edesc=None), dict(full, commit=None), dict(full, eoff=None)):
        with pytest.raises(HipBatchError):
            eng.decode_follow(d[0], d[1], d[2], d[3], broken, status, 64, ed, n_ent)
    with pytest.raises(HipBatchError):
        eng.decode_follow(d[0], d[1], d[2], d[3], full, status, 64, None, n_ent)  # edata NULL
    with pytest.raises(HipBatchError):
        eng.decode_follow(d[0], d[1], d[2], d[3], full, status, 64, torch.zeros(64, dtype=torch.int64, device="cuda"), None)


# ---- 4. the HOST rules, one record each, among OK neighbours ------------------------------------
def test_host_rules_among_ok_neighbours():
    import torch
    G = 4
    eng, _, peers = _engine(G, max_batch=1 << 10)
    cases = rule_cases()
    recs, where = [], {}
    for i, (name, (rec, _, _)) in enumerate(cases.items()):
        recs += _mix(3, salt=5 * i)[:1 + i % 3]  # MsgApp, MsgHeartbeat, MsgApp: HB_WIRE_OK from any sender
        where[name] = len(recs)
        recs.append(rec)
    recs += _mix(5, salt=40)
    grp = np.zeros(len(recs), np.uint32)
    _, host, ref, _ = _run(eng, torch, recs, grp, G, peers, ctx="rules", lead=2)
    for name, (_, st, ne) in cases.items():
        k = where[name]
        assert host["status"][k] == st, name
        assert int(host["eoff"][k + 1] - host["eoff"][k]) == ne, name
        assert host["status"][k - 1] == abi.HB_WIRE_OK, name
        assert (host["group"][k] == 0xFFFFFFFF) == (st != abi.HB_WIRE_OK), name
    for name in ("gap", "type 2", "reordered entry fields", "unknown field in an entry", "unknown field between entries",
                 "dropped Entry error", "vote of a non-member", "snap", "prop"):
        assert cases[name][1] == abi.HB_WIRE_HOST


# ---- 5. decode -> step --------------------------------------------------------------------------
def _with_sentinel(b, ref):
    """The oracle's batch: what the decode keeps of the generating batch, plus the sentinel record."""
    ob = {k: ref[k] for k in BATCH}
    ob.update(eoff=ref["eoff"], eterm=ref["eterm"], edesc=ref["edesc"], props=None)
    return ob


def _decode_step(pair, torch, b, peers, G, n, data_of, ctx, expect_all=True):
    recs = records_of(b, peers, data_of)
    data, off, ln = W.pack(recs)
    ent_cap = int(ln.astype(np.uint64).sum()) // 8
    ref = follow_reference(data, off, ln, b["group"], G, np.full(G, n, np.uint32), peers)
    # the reference's record is the generating one wherever the device keeps it
    ok = ref["status"] == abi.HB_WIRE_OK
    for k in BATCH:
        gen = b[k] & np.uint32(0x1FF) if k == "info" else b[k]  # (HB_INFO_VOTED is the host's)
        assert np.array_equal(ref[k][:-1][ok], gen[ok]), k
    t = b["info"] & 0xF
    host_only = (t == abi.HB_MSG_SNAP) | ((t == abi.HB_MSG_VOTE) & (((b["info"] >> 4) & 0xF) == abi.HB_SLOT_NONE))
    assert np.array_equal(ok, ~host_only) and (not expect_all or ok.all())
    assert np.array_equal(ref["eterm"], np.asarray(b["eterm"], np.uint64)[_kept_entries(b, ok)])
    out, host = _decode(pair.eng, torch, data, off, ln, b["group"], ent_cap)
    _check(host, ref, len(recs), ent_cap, ctx)
    ob = _with_sentinel(b, ref)
    pair.reserve(ob)
    pair.eng.step_decoded(out, ent_cap)  # b.n = n + 1, n_edesc = ent_cap: no host read of the count
    dev_ev, dev_st = pair.eng.events(), pair.eng.stats()
    ora_ev, ora_st = pair.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, ctx)
    assert np.array_equal(dev_st, ora_st), f"{ctx}: stats dev {dev_st.tolist()} ora {ora_st.tolist()}"
    now = pair.og.groups()
    assert_groups_equal(pair.eng.get_groups(), now, ctx)
    return dev_st, now


def _kept_entries(b, ok):
    eo = np.append(np.asarray(b["eoff"], np.int64), len(b["eterm"]))
    keep = np.zeros(len(b["eterm"]), bool)
    for i in np.nonzero(ok)[0]:
        keep[eo[i]:eo[i + 1]] = True
    return keep


@pytest.mark.parametrize("ents", [1, 3])
def test_decode_then_step_follow(ents):
    import torch
    G, n = 4000, 3
    g, runs = synth.follow_groups(G, n, seed=201, last_hi=1 << 14, with_runs=True)
    pair = Pair(g, runs, n, 256, max_batch=2 * G + 16, term_runs=True)
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    for step in range(3):
        b = synth.follow_batch(g, step, seed=202, ents=ents)
        st, now = _decode_step(pair, torch, b, peers, G, n, lambda i, k: _payload(16, i + k), f"follow {ents} step {step}")
        assert st[abi.HB_STAT_COMMITS] == G and st[abi.HB_STAT_ENTRIES] == ents * G and st[abi.HB_STAT_FAULTS] == 0
        assert np.array_equal(now["last_index"], g["last_index"] + np.uint64((step + 1) * ents))


@pytest.mark.parametrize("nmax,seed", [(3, 211), (5, 212)])
def test_decode_then_step_follower_mix(nmax, seed):
    import torch
    G = 1500
    g, runs, ins = synth.random_groups(G, nmax, seed=seed, W=8)
    pair = Pair(g, runs, nmax, 8, ins=ins, max_batch=1 << 13, term_runs=True)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    peers[:, :nmax] = np.arange(1, nmax + 1, dtype=np.uint64)
    pair.eng.load_peers(peers)
    now = pair.og.groups()
    nn = now["n"].astype(np.uint32)
    for k in range(3):
        b = synth.follower_messages(now, pair.og.term, 3000, seed=seed + 10 * k)
        recs = records_of(b, peers, lambda i, j: _payload(DATA_LENS[(i + j) % len(DATA_LENS)], i))
        data, off, ln = W.pack(recs)
        ent_cap = int(ln.astype(np.uint64).sum()) // 8
        ref = follow_reference(data, off, ln, b["group"], G, nn, peers)
        ok = ref["status"] == abi.HB_WIRE_OK
        t = b["info"] & 0xF
        host_only = (t == abi.HB_MSG_SNAP) | ((t == abi.HB_MSG_VOTE) & (((b["info"] >> 4) & 0xF) == abi.HB_SLOT_NONE))
        assert np.array_equal(ok, ~host_only)
        for key in BATCH:
            gen = b[key] & np.uint32(0x1FF) if key == "info" else b[key]
            assert np.array_equal(ref[key][:-1][ok], gen[ok]), key
        out, host = _decode(pair.eng, torch, data, off, ln, b["group"], ent_cap)
        _check(host, ref, len(recs), ent_cap, f"mix {nmax} step {k}")
        ob = _with_sentinel(b, ref)
        pair.reserve(ob)
        pair.eng.step_decoded(out, ent_cap)
        dev_ev, dev_st = pair.eng.events(), pair.eng.stats()
        ora_ev, ora_st = pair.og.step(ob)
        assert_events_equal(dev_ev, ora_ev, f"mix {nmax} step {k}")
        assert np.array_equal(dev_st, ora_st)
        now = pair.og.groups()
        assert_groups_equal(pair.eng.get_groups(), now, f"mix {nmax} step {k}")


def test_decode_then_step_finite_max_msg_size():
    """A handle with a finite max_msg_size reads the decoded edesc: the appended entries' sizes."""
    import torch
    G, n = 1000, 3
    g, runs = synth.follow_groups(G, n, seed=221, last_hi=1 << 10, with_runs=True)
    sizes = synth.window_sizes(g, runs, seed=222, frac_full=1.0)
    pair = Pair(g, runs, n, 256, max_msg_size=4096, sizes=sizes, max_batch=2 * G + 16, term_runs=True)
    peers = _peers(G, n)
    pair.eng.load_peers(peers)
    for step in range(2):
        b = synth.follow_batch(g, step, seed=223, ents=2)
        st, _ = _decode_step(pair, torch, b, peers, G, n, lambda i, k: _payload(DATA_LENS[(i + k) % len(DATA_LENS)], i),
                             f"finite step {step}")
        assert st[abi.HB_STAT_ENTRIES] == 2 * G and st[abi.HB_STAT_FAULTS] == 0


# ---- 6. loopback: two engines, their own bytes --------------------------------------------------
def test_loopback_leader_to_follower_and_back():
    """A leader engine (node 1) steps one proposal per group with append-mode egress; its records for
    node 2 are binned, encoded and spliced.  A follower engine (node 2: its peer rows in its own slot
    order, itself at slot 0) takes them through decode_follow -> step; its MsgAppResp bytes come back
    through the existing hb_decode -> step.  Both engines equal their oracles after each hop."""
    import torch
    from etcd_amd.splice import splice
    from .egress_app_util import entry_bytes
    from .test_egress_bin_gpu import _chain
    from .test_egress_gpu import _tap
    G, n = 512, 3
    g, runs = synth.steady_groups(G, n, seed=231, last_hi=1 << 14)
    lead = _tap(Pair(g, runs, n, 256, max_batch=8 * G, term_runs=True))
    lpeers = _peers(G, n)  # the leader is node 1 at slot 0
    lead.eng.load_peers(lpeers)
    lead.eng.set_egress(True, apps=True)
    lead.eng.set_egress_peers(np.array([2, 3], dtype=np.uint64))
    # node 2's view of the same groups: itself at slot 0, the leader (node 1) at slot 1, node 3 at slot 2
    fg, fruns = synth.follow_groups(G, n, seed=231, last_hi=1 << 14, with_runs=True)
    fol = _tap(Pair(fg, fruns, n, 256, max_batch=8 * G, term_runs=True))
    fpeers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    fpeers[:, :3] = (2, 1, 3)
    fol.eng.load_peers(fpeers)
    fol.eng.set_egress(True)
    assert np.array_equal(fg["last_index"], g["last_index"]) and np.array_equal(fg["term"], g["term"])
    # hop 1: the leader proposes (the cfg2 step: the proposal, both acks, so the entry and then the new Commit go out)
    lead.step(synth.cfg2_batch(g, 0, seed=232), ctx="loopback propose")
    res = _chain(lead.eng, 1, 8 * G, 2)
    lo, hi = int(res["bin_off"][0]), int(res["bin_off"][1])  # bin 0: node 2
    assert hi - lo == 2 * G
    raw = res["data"].tobytes()
    term_of = lambda gi, i: int(g["term"][gi])  # noqa: E731
    msgs, grp = [], []
    for i in range(lo, hi):
        gi, st = int(res["out"]["group"][i]), int(res["status"][i])
        ents = [entry_bytes(gi, j, term_of(gi, j)) for j in range(int(res["out"]["index"][i]) + 1, int(res["out"]["hint"][i]) + 1)] \
            if res["out"]["info"][i] & abi.HB_OUT_ENTS else []
        assert bool(ents) == bool(st & abi.HB_WIRE_SPLICE)
        msgs.append(splice(raw[int(res["off"][i]):int(res["off"][i + 1])], st, ents))
        grp.append(gi)
    grp = np.array(grp, np.uint32)
    # hop 2: the follower decodes and steps them
    data, off, ln = W.pack(msgs)
    ent_cap = int(ln.astype(np.uint64).sum()) // 8
    ref = follow_reference(data, off, ln, grp, G, np.full(G, n, np.uint32), fpeers)
    assert (ref["status"] == abi.HB_WIRE_OK).all() and ref["n_ent"] == G
    assert (ref["info"][:-1] == abi.hb_info(abi.HB_MSG_APP, 1, False)).all()
    out, host = _decode(fol.eng, torch, data, off, ln, grp, ent_cap)
    _check(host, ref, 2 * G, ent_cap, "loopback decode")
    ob = _with_sentinel(None, ref)
    fol.reserve(ob)
    fol.eng.step_decoded(out, ent_cap)
    dev_ev, dev_st = fol.eng.events(), fol.eng.stats()
    ora_ev, ora_st = fol.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, "loopback follower")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_ENTRIES] == G
    fnow = fol.og.groups()
    assert_groups_equal(fol.eng.get_groups(), fnow, "loopback follower")
    assert np.array_equal(fnow["last_index"], g["last_index"] + np.uint64(1))
    # hop 3: the follower's MsgAppResp bytes back to the leader through hb_decode
    back = _chain_plain(fol.eng, torch, 2, 2 * G)
    keep = [i for i in range(back["n"]) if int(back["to"][i]) == 1]
    assert len(keep) == 2 * G and all(int(back["info"][i]) & 0xF == abi.HB_MSG_APP_RESP for i in keep)
    braw = back["data"].tobytes()
    rmsgs = [braw[int(back["off"][i]):int(back["off"][i + 1])] for i in keep]
    rgrp = back["group"][keep].astype(np.uint32)
    rdata, roff, rln = W.pack(rmsgs)
    rout = {k: torch.empty(2 * G, dtype=torch.int32 if DT[k] == np.uint32 else torch.int64, device="cuda") for k in BATCH[:5]}
    rstatus = torch.empty(2 * G, dtype=torch.uint8, device="cuda")
    lead.eng.decode(_dev(torch, rdata), _dev(torch, roff), _dev(torch, rln), _dev(torch, rgrp), rout, rstatus)
    torch.cuda.synchronize()
    assert (rstatus.cpu().numpy() == abi.HB_WIRE_OK).all()
    ora = decode_batch(rdata, roff, rln, rgrp, G, np.full(G, n, np.uint32), lpeers)
    assert (ora["info"] == abi.hb_info(abi.HB_MSG_APP_RESP, 1, False)).all()
    lead.eng.step(rout["group"], rout["info"], rout["term"], rout["index"], rout["hint"], None, host=False)
    dev_ev, dev_st = lead.eng.events(), lead.eng.stats()
    ora_ev, ora_st = lead.og.step(dict(group=ora["group"], info=ora["info"], term=ora["term"], index=ora["index"],
                                       hint=ora["hint"], props=None))
    assert_events_equal(dev_ev, ora_ev, "loopback leader ack")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_APPRESP] == 2 * G
    assert_groups_equal(lead.eng.get_groups(), lead.og.groups(), "loopback leader ack")


def _chain_plain(eng, torch, self_id, cap):
    """hb_egress -> hb_encode of the last step (no binning); host arrays."""
    t = lambda dt, fill, k=cap: torch.full((max(k, 1),), fill, dtype=dt, device="cuda")  # noqa: E731
    tdt = {"<u4": torch.int32, "<u8": torch.int64}
    raw = {name: t(tdt[np.dtype(dt).str], -1) for name, dt in abi.OUT_BATCH_FIELDS}
    count, total = t(torch.int64, -1, 1), t(torch.int64, -1, 1)
    data, off, status = t(torch.uint8, 0xAA, 91 * cap), t(torch.int64, -1, cap + 1), t(torch.uint8, 0xEE)
    eng.egress(self_id, raw, cap, count)
    eng.encode(self_id, raw, cap, data, off, status, total, n_dev=count)
    eng.sync()
    res = {name: raw[name].cpu().numpy().view(np.dtype(dt)) for name, dt in abi.OUT_BATCH_FIELDS}
    res.update(n=int(count.item()), data=data.cpu().numpy(), off=off.cpu().numpy().view(np.uint64),
               status=status.cpu().numpy())
    return res
