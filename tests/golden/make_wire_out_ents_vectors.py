"""Generate tests/golden/wire_out/wire_out_ents_vectors.npz: entry and whole-MsgApp encoder vectors.

Test infrastructure only.  What hb_encode_ents writes for a covered record: the
entries of a MsgApp as Entry.MarshalTo and Message.MarshalTo frame them.  The
bytes are those of tests/wire_util._entry and gogo_marshal (the restatement of
the reference's generated encoder); tests/asan/wire_out_ents_asan.cpp checks
wo_entry_size, wo_entry_head and the whole message (wo_write_prefix, the
entries, wo_write_suffix) of etcd_amd/csrc/hipbatch_wire_out.h against them
under the sanitizers.

Entries: every varint-length edge of a u64 (the EDGES of make_wire_out_vectors.py)
in Term and in Index; Data absent, empty, and of the lengths 1, 15-17, 117-130
(both sides of the 1 / 2-byte edge of Entry.Size()), 16,383, 16,384 and 70,000;
Type 0 and 1.  Messages: 0, 1, 3 and 300 entries, and one with the three long
payloads; a message's entries are consecutive rows of the entry table and their
Index is m.Index + 1 + k.  Every payload is a slice of one pattern blob.

  ents  [E, 4] u64: desc = HB_ENT_DESC(len, Type, Data != nil), Term, Index, the payload's offset in pdata
  esize [E] u64:    Entry.Size()
  hoff  [E + 1] u64, hdata u8: the entry's framing and head = 3a varint(Size) 08 Type 10 Term 18 Index [22 varint(len)]
  pdata u8:         the payload blob
  msgs  [M, 8] u64: to, from, term, log_term, index, commit, first entry row, end entry row
  moff  [M + 1] u64, mdata u8: the whole message

  python tests/golden/make_wire_out_ents_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from etcd_amd import abi  # noqa: E402
from tests.golden.make_wire_out_vectors import EDGES  # noqa: E402
from tests.wire_util import _entry, gogo_marshal, key, varint  # noqa: E402

NAME = "wire_out_ents_vectors.npz"
MASK = (1 << 64) - 1
# None = Data absent (nil); 0 = present and empty
DATA_LENS = [None, 0, 1, 15, 16, 17] + list(range(117, 131)) + [16383, 16384, 70000]
LONG = (16383, 16384, 70000)
BLOB = 70000 + 64


def blob():
    i = np.arange(BLOB, dtype=np.uint64)
    return ((i * np.uint64(37) + (i >> np.uint64(8)) * np.uint64(11) + np.uint64(5)) & np.uint64(0xFF)).astype(np.uint8)


def payload(pd, ln, poff):
    return None if ln is None else pd[poff:poff + ln].tobytes()


def entry_rows():
    """[(type, term, index, data length or None, payload offset)]: the stand-alone entries."""
    rows = []
    E = len(EDGES)
    for k, v in enumerate(EDGES):  # the edge in Term, then in Index, the other at an edge of another length
        rows.append((k & 1, v, EDGES[(k + 5) % E], DATA_LENS[k % 6], k % 16))
        rows.append(((k + 1) & 1, EDGES[(k + 9) % E], v, DATA_LENS[(k + 3) % 6], (k + 7) % 16))
    for j, ln in enumerate(DATA_LENS):  # every length, both types, small and wide Term / Index
        rows.append((0, 1 + j, 2 + j, ln, j % 16))
        rows.append((1, EDGES[(3 * j) % E], EDGES[(3 * j + 1) % E], ln, (j + 3) % 16))
    rows.append((0, 0, 0, None, 0))
    rows.append((1, MASK, MASK, 70000, 15))
    return rows


def message_rows():
    """[(to, frm, term, log_term, index, commit, [(type, eterm, data length or None, payload offset)])]"""
    short = [ln for ln in DATA_LENS if ln not in LONG]
    out = []
    for n in (0, 1, 3, 300):
        for w, (to, frm, term, lt, idx, com) in enumerate(((2, 1, 7, 7, 40, 39),
                                                            (1 << 63, MASK, 1 << 50, (1 << 50) - 1, (1 << 61) - 2, 1 << 61),
                                                            (3, 1, 1 << 14, 127, (1 << 7 * (n % 9 + 1)) - 2, 128))):
            ents = [((k + w) % 5 == 0 and 1 or 0, term - (k % 3 == 2), short[(k + 2 * w + n) % len(short)], (k * 5 + w) % 32)
                    for k in range(n)]
            out.append((to, frm, term, lt, idx, com, ents))
    out.append((9, 1, 300, 300, 16383, 16000, [(0, 300, ln, 1 + j) for j, ln in enumerate(LONG)]))
    out.append((0, 0, 0, 0, 0, 0, [(0, 0, None, 0)]))
    return out


def table():
    """(entry table rows [(type, term, index, ln, poff)], message rows [(to, frm, term, lt, idx, com, e0, e1)])"""
    ents = entry_rows()
    msgs = []
    for to, frm, term, lt, idx, com, es in message_rows():
        e0 = len(ents)
        for k, (t, et, ln, poff) in enumerate(es):
            ents.append((t, et & MASK, (idx + 1 + k) & MASK, ln, poff))
        msgs.append((to, frm, term, lt, idx, com, e0, len(ents)))
    return ents, msgs


def desc_of(t, ln):
    return abi.hb_ent_desc(ln or 0, t, ln is not None)


def build():
    pd = blob()
    ents, msgs = table()
    tup = [(t, term, index, payload(pd, ln, poff)) for t, term, index, ln, poff in ents]
    raw = [_entry(e) for e in tup]
    heads = [key(7, 2) + varint(len(r)) + (r if e[3] is None else r[:len(r) - len(e[3])]) for r, e in zip(raw, tup)]
    whole = [gogo_marshal(abi.HB_MSG_APP, to=to, frm=frm, term=term, log_term=lt, index=idx, entries=tup[e0:e1], commit=com)
             for to, frm, term, lt, idx, com, e0, e1 in msgs]
    return pd, ents, msgs, raw, heads, whole


def arrays():
    pd, ents, msgs, raw, heads, whole = build()
    hoff = np.zeros(len(ents) + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in heads])
    moff = np.zeros(len(msgs) + 1, np.uint64)
    moff[1:] = np.cumsum([len(m) for m in whole])
    return dict(ents=np.array([(desc_of(t, ln), term, index, poff) for t, term, index, ln, poff in ents], dtype=np.uint64),
                esize=np.array([len(r) for r in raw], dtype=np.uint64), hoff=hoff,
                hdata=np.frombuffer(b"".join(heads), dtype=np.uint8), pdata=pd,
                msgs=np.array(msgs, dtype=np.uint64), moff=moff, mdata=np.frombuffer(b"".join(whole), dtype=np.uint8))


def main():
    a = arrays()
    np.savez(os.path.join(HERE, "wire_out", NAME), **a)
    print(f"{NAME}: {len(a['ents'])} entries, {len(a['msgs'])} messages, {int(a['moff'][-1])} message bytes")


if __name__ == "__main__":
    main()
