"""CPU tests of the reference of hb_decode_follow (tests/ingest_util.py) and of the
ABI additions (no GPU calls).

- follow_reference returns the generating values for records of every follower type
  from both encoders (wire_util.gogo_marshal, the protobuf library), 0-4 entries,
  Data None / b"" / non-empty.
- on wire_util.mutate'd records its status equals the oracle's hb_decode contract
  (decode_batch) wherever that is not HB_WIRE_HOST.
- wherever the canonical parser accepts a record, its entries are the protobuf
  library's parse of the same bytes.
"""
import os
import re

import numpy as np

from etcd_amd import abi
from oracle.pyoracle import decode_batch

from . import wire_util as W
from .ingest_util import canonical_entries, follow_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATAS = (None, b"", b"x", b"0123456789abcdef", bytes(range(200)))


def _peers(G, n):
    p = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    p[:, :n] = np.arange(1, n + 1, dtype=np.uint64)
    return p


def _records(rng, count=600):
    """(record, generating values) of the follower types and the responses."""
    out = []
    types = (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_VOTE) + W.RESP_TYPES
    for k in range(count):
        t = types[k % len(types)]
        term, lt, idx, com = (int(rng.integers(0, 1 << s)) for s in (20, 20, 40, 40))
        frm = int(rng.integers(1, 5))  # 4 is no member
        ne = (k // len(types)) % 5 if t == abi.HB_MSG_APP else 0
        ents = [(int(rng.integers(0, 2)), int(rng.integers(1, 1 << 20)), idx + 1 + j, DATAS[(k + j) % len(DATAS)])
                for j in range(ne)]
        rej = t in W.RESP_TYPES and k % 4 == 0
        hint = int(rng.integers(0, 1 << 30)) if rej else 0
        kw = dict(to=1, frm=frm, term=term, log_term=lt, index=idx, commit=com, reject=rej, hint=hint, entries=ents)
        rec = W.gogo_marshal(t, **kw) if k % 2 == 0 else W.pb_message(t, **kw)
        if k % 2:
            assert rec == W.gogo_marshal(t, **kw)  # the two encoders agree on this schema
        out.append((rec, t, frm, term, lt, idx, com, rej, hint, ents))
    return out


def test_reference_returns_the_generating_values():
    rng = np.random.default_rng(11)
    G = 8
    rows = _records(rng)
    recs = [r[0] for r in rows]
    data, off, ln = W.pack(recs)
    grp = (np.arange(len(recs)) % (G + 1)).astype(np.uint32)  # group G is out of range
    ref = follow_reference(data, off, ln, grp, G, np.full(G, 3, np.uint32), _peers(G, 3))
    seen = set()
    e = 0
    for k, (rec, t, frm, term, lt, idx, com, rej, hint, ents) in enumerate(rows):
        gok = grp[k] < G
        slot = frm - 1 if frm <= 3 else abi.HB_SLOT_NONE
        if t in W.RESP_TYPES:
            want = abi.HB_WIRE_OK if gok else abi.HB_WIRE_BADGROUP
        else:
            want = abi.HB_WIRE_OK if gok and not (t == abi.HB_MSG_VOTE and frm > 3) else abi.HB_WIRE_HOST
        assert ref["status"][k] == want, k
        assert ref["eoff"][k] == e
        if want != abi.HB_WIRE_OK:
            assert (ref["group"][k], ref["info"][k], ref["term"][k], ref["index"][k], ref["hint"][k],
                    ref["commit"][k]) == (0xFFFFFFFF, 0, 0, 0, 0, 0)
            continue
        seen.add((t, len(ents)))
        whint = hint if t in W.RESP_TYPES else (0 if t == abi.HB_MSG_HEARTBEAT else lt)
        wcom = com if t in (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT) else 0
        assert (ref["group"][k], ref["info"][k], ref["term"][k], ref["index"][k], ref["hint"][k], ref["commit"][k]) == \
            (grp[k], abi.hb_info(t, slot, rej), term, idx, whint, wcom), k
        for ty, et, _, d in ents:
            assert ref["eterm"][e] == et
            assert ref["edesc"][e] == abi.hb_ent_desc(0 if d is None else len(d), ty, d is not None)
            if d is None:
                assert ref["edata"][e] == 0
            else:
                p = int(ref["edata"][e])
                assert p > int(off[k]) and bytes(data[p:p + len(d)]) == d
            e += 1
    assert e == ref["n_ent"] == ref["eoff"][-1] == len(ref["eterm"]) == len(ref["edesc"]) == len(ref["edata"])
    assert ref["group"][-1] == 0xFFFFFFFF and ref["info"][-1] == 0 and ref["term"][-1] == 0  # the sentinel
    assert {(abi.HB_MSG_APP, j) for j in range(5)} <= seen
    assert {(abi.HB_MSG_HEARTBEAT, 0), (abi.HB_MSG_VOTE, 0)} <= seen and {(t, 0) for t in W.RESP_TYPES} <= seen


def test_mutated_records_keep_the_decoders_status_and_entries_match_protobuf():
    from google.protobuf.message import DecodeError
    rng = np.random.default_rng(12)
    G = 8
    good = [r[0] for r in _records(rng, 400)]
    recs = list(good)
    for r in good * 4:
        recs.append(W.mutate(r, rng)[0])
    data, off, ln = W.pack(recs)
    grp = rng.integers(0, G + 2, len(recs)).astype(np.uint32)
    nn, peers = np.full(G, 3, np.uint32), _peers(G, 3)
    ref = follow_reference(data, off, ln, grp, G, nn, peers)
    dec = decode_batch(data, off, ln, grp, G, nn, peers)
    same = dec["status"] != abi.HB_WIRE_HOST
    assert np.array_equal(ref["status"][same], dec["status"][same])
    assert set(np.unique(ref["status"][~same]).tolist()) == {abi.HB_WIRE_OK, abi.HB_WIRE_HOST}
    for k in ("group", "info", "term", "index", "hint"):  # the responses' records are hb_decode's
        assert np.array_equal(ref[k][:-1][same], dec[k][same]), k
    assert not ref["commit"][:-1][same].any()
    counts = np.bincount(ref["status"], minlength=6)
    assert all(counts[s] > 0 for s in (abi.HB_WIRE_OK, abi.HB_WIRE_HOST, abi.HB_WIRE_ERROR, abi.HB_WIRE_PANIC))
    M = W.pb_classes()["Message"]
    accepted = with_ents = 0
    for rec in recs:
        ents = canonical_entries(rec)
        if ents is None:
            continue
        accepted += 1
        with_ents += bool(ents)
        try:
            p = M.FromString(rec)
        except DecodeError:
            raise AssertionError(f"canonical but not protobuf: {rec.hex()}")
        assert len(p.entries) == len(ents)
        for j, (e, (term, desc, pos)) in enumerate(zip(p.entries, ents)):
            assert e.Term == term and e.Index == (p.index + 1 + j) & ((1 << 64) - 1)
            assert desc == abi.hb_ent_desc(len(e.Data), e.Type, e.HasField("Data"))
            assert (pos == 0) == (not e.HasField("Data")) and rec[pos:pos + len(e.Data)] == e.Data
    assert accepted >= 400 and with_ents > 40


def test_the_rules_one_record_each():
    """The HB_WIRE_HOST rules of the contract, and the shapes that stay HB_WIRE_OK."""
    from .ingest_util import rule_cases
    G = 2
    nn, peers = np.full(G, 3, np.uint32), _peers(G, 3)
    cases = rule_cases()
    assert {"gap", "type 2", "reordered entry fields", "unknown field in an entry", "unknown field between entries",
            "dropped Entry error", "vote of a non-member", "snap", "prop"} <= set(cases)
    recs = [c[0] for c in cases.values()]
    data, off, ln = W.pack(recs)
    ref = follow_reference(data, off, ln, np.zeros(len(recs), np.uint32), G, nn, peers)
    for k, (name, (_, st, ne)) in enumerate(cases.items()):
        assert ref["status"][k] == st, name
        assert int(ref["eoff"][k + 1]) - int(ref["eoff"][k]) == ne, name
    assert (ref["info"][list(cases).index("app of a non-member")] >> 4) & 0xF == abi.HB_SLOT_NONE


def test_decode_follow_abi():
    assert abi.HB_DECODE_FOLLOW == 1
    txt = open(os.path.join(ROOT, "include", "hipbatch.h")).read()
    assert re.search(r"^#define\s+HB_DECODE_FOLLOW\s+1\b", txt, re.M)
    assert re.search(r"^#define\s+HB_ABI_VERSION\s+8\b", txt, re.M)
    from etcd_amd import hipbatch
    L = hipbatch.lib()  # loads without touching the GPU
    assert L.hb_abi_version() == abi.HB_ABI_VERSION == 8
    assert L.hb_decode_caps() == abi.HB_DECODE_FOLLOW
    # argument checks come before any device work: a NULL handle
    assert L.hb_decode_follow(None, None, None, None, None, 0, None, None, 0, None, None) == abi.HB_EINVAL
