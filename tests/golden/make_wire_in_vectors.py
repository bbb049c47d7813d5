"""Generate tests/golden/wire_in/wire_in_vectors.npz: vectors of the canonical-shape parser.

Test infrastructure only, built from tests/wire_util alone.  Messages as
Message.MarshalTo writes them (wire_util.gogo_marshal, entries included) for
etcd_amd/csrc/hipbatch_wire_in.h, which tests/asan/wire_in_asan.cpp runs over them
under the sanitizers:

- every varint-length edge of a u64 (EDGES) in Term, LogTerm, Index (the entries
  numbered from it, mod 2^64), Commit and the entry Term, the others holding edges
  of other lengths;
- 0, 1, 3 and 300 entries; Data absent, empty and of 1, 127, 128 and 70,000 bytes;
  both entry types; MsgHeartbeat and MsgVote beside MsgApp;
- records the parser must call "not canonical" (canon = 0): an index gap, Type 2,
  a non-minimal Type, reordered entry fields, an unknown field inside an entry and
  between entries, a malformed entry, an over-long Data length, reordered message
  fields, a non-empty snapshot, trailing bytes.

  fields [N, 10] u64: type, to, from, term, log_term, index, commit, hint, entries, canon
  off    [N + 1] u64, data u8: message i = data[off[i], off[i + 1])
  eoff   [N + 1] u64: the entries of message i are eoff[i] .. eoff[i + 1] of
  eterm  [E] u64, edesc [E] u32 (HB_ENT_DESC), epos [E] u64 (position of the first
         Data byte inside the message, 0 when Data is absent)

  python tests/golden/make_wire_in_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from etcd_amd import abi  # noqa: E402
from tests.wire_util import _entry, gogo_marshal, key, varint  # noqa: E402

EDGES = sorted({v for k in range(1, 10) for v in ((1 << 7 * k) - 1, 1 << 7 * k)} | {1 << 63, (1 << 64) - 1})
FIELDS = ("term", "log_term", "index", "commit", "eterm")
DATA_LENS = (None, 0, 1, 127, 128, 70000)
NAME = "wire_in_vectors.npz"
MASK = (1 << 64) - 1


def _data(ln, salt):
    return None if ln is None else bytes((salt + 7 * j) & 0xFF for j in range(ln))


def _ents(index, eterm, n, salt, lens=(None, 0, 1, 5, 16)):
    return [(int((salt + k) % 3 == 0), eterm, (index + 1 + k) & MASK, _data(lens[(salt + k) % len(lens)], salt + k))
            for k in range(n)]


def vectors():
    """[(type, kw of gogo_marshal (entries as (type, term, index, data)), canonical)]"""
    E = len(EDGES)
    rows = []
    for fi, f in enumerate(FIELDS):
        for k, v in enumerate(EDGES):
            kw = {o: EDGES[(k + 3 + 4 * ((fi + j) % len(FIELDS))) % E] for j, o in enumerate(FIELDS)}
            kw[f] = v
            n = (1, 3)[k % 2] if f == "eterm" else (0, 1, 3)[(k + fi) % 3]
            eterm = kw.pop("eterm")
            rows.append((abi.HB_MSG_APP, dict(to=1 + k % 3, frm=1 + (k + fi) % 3, entries=_ents(kw["index"], eterm, n, k + fi),
                                              **kw), 1))
    base = dict(to=1, frm=2, term=7, log_term=6, index=1000, commit=999)
    for n in (0, 1, 3, 300):
        rows.append((abi.HB_MSG_APP, dict(base, entries=_ents(1000, 7, n, n)), 1))
    for i, ln in enumerate(DATA_LENS):
        rows.append((abi.HB_MSG_APP, dict(base, entries=[(i & 1, 7, 1001, _data(ln, i))]), 1))
    rows.append((abi.HB_MSG_APP, dict(base, entries=[(0, 7, 1001, None), (1, 7, 1002, _data(128, 9)), (0, 8, 1003, b"")]), 1))
    rows.append((abi.HB_MSG_HEARTBEAT, dict(to=1, frm=2, term=7, commit=55), 1))
    rows.append((abi.HB_MSG_VOTE, dict(to=1, frm=3, term=8, log_term=7, index=1000), 1))
    rows.append((abi.HB_MSG_APP_RESP, dict(to=1, frm=3, term=8, index=1000, reject=True, hint=77), 1))
    rows.append((abi.HB_MSG_APP, dict(to=0, frm=0), 1))
    return rows


def not_canonical():
    """Records Unmarshal accepts (or not) that the parser must refuse."""
    base = dict(to=1, frm=2, term=7, log_term=6, index=1000, commit=999)
    e = lambda i, t=0, d=b"ab": (t, 7, i, d)  # noqa: E731
    ent7 = lambda body: key(7, 2) + varint(len(body)) + body  # noqa: E731
    head = gogo_marshal(abi.HB_MSG_APP, **base)
    cut = head.index(key(8, 0) + varint(999) + key(9, 2))
    pre, post = head[:cut], head[cut:]
    good, bare = _entry(e(1001)), _entry(e(1001, 0, None))
    return [
        gogo_marshal(abi.HB_MSG_APP, entries=[e(1001), e(1003)], **base),                       # an index gap
        gogo_marshal(abi.HB_MSG_APP, entries=[e(1002)], **base),                                # not m.Index + 1
        gogo_marshal(abi.HB_MSG_APP, entries=[e(1001, 2)], **base),                             # Type 2
        pre + ent7(b"\x08\x80\x00" + good[2:]) + post,                                          # non-minimal Type
        pre + ent7(key(2, 0) + varint(7) + key(1, 0) + varint(0) + key(3, 0) + varint(1001)) + post,  # reordered
        pre + ent7(good + key(9, 0) + varint(1)) + post,                                        # unknown field inside
        pre + ent7(good) + key(20, 0) + varint(1) + ent7(_entry(e(1002))) + post,               # unknown field between
        pre + ent7(key(4, 2) + varint(50) + b"\x01") + post,                                    # a dropped Entry error
        pre + ent7(bare + key(4, 2) + varint(3) + b"a") + post,                            # Data past its span
        pre + ent7(good + b"\x00") + post,                                                      # bytes after Data
        pre + key(7, 2) + varint(200) + good + post,                                            # a span past the record
        pre + ent7(bare + key(4, 2) + varint((1 << 64) - 20)) + post,                       # a negative length
        pre + ent7(bare + key(4, 2) + b"\xff" * 10 + b"\x01") + post,                       # an 11-byte varint
        post + pre,                                                                             # message fields reordered
        gogo_marshal(abi.HB_MSG_APP, snapshot=(None, (1,), 5, 5), **base),                      # a snapshot
        head + key(20, 0) + varint(1),                                                          # trailing field
        head[:-1],                                                                              # truncated
        b"",
    ]


def build():
    """The arrays of the fixture."""
    recs, fields, eterm, edesc, epos, eoff = [], [], [], [], [], [0]
    for t, kw, canon in vectors():
        rec = gogo_marshal(t, **kw)
        ents = kw.get("entries", ())
        for ty, et, _, d in ents:
            eterm.append(et)
            edesc.append(abi.hb_ent_desc(0 if d is None else len(d), int(ty), d is not None))
        pos = 0  # where each Data lies: found from the encoder's own lengths
        for ent in ents:
            eb = _entry(ent)
            at = rec.index(key(7, 2) + varint(len(eb)) + eb, pos)
            pos = at + len(key(7, 2) + varint(len(eb)) + eb)
            epos.append(0 if ent[3] is None else pos - len(ent[3]))
        eoff.append(len(eterm))
        recs.append(rec)
        fields.append((t, kw.get("to", 0), kw.get("frm", 0), kw.get("term", 0), kw.get("log_term", 0), kw.get("index", 0),
                       kw.get("commit", 0), kw.get("hint", 0), len(ents), canon))
    for rec in not_canonical():
        recs.append(rec)
        eoff.append(len(eterm))
        fields.append((0,) * 10)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return dict(fields=np.array(fields, dtype=np.uint64), off=off, data=np.frombuffer(b"".join(recs), dtype=np.uint8),
                eoff=np.array(eoff, np.uint64), eterm=np.array(eterm, np.uint64), edesc=np.array(edesc, np.uint32),
                epos=np.array(epos, np.uint64))


def main():
    z = build()
    os.makedirs(os.path.join(HERE, "wire_in"), exist_ok=True)
    np.savez(os.path.join(HERE, "wire_in", NAME), **z)
    print(f"{NAME}: {len(z['fields'])} vectors, {int(z['off'][-1])} bytes, {len(z['eterm'])} entries")


if __name__ == "__main__":
    main()
