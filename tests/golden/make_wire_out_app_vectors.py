"""Generate tests/golden/wire_out/wire_out_app_vectors.npz: MsgApp encoder vectors.

Test infrastructure only.  sendAppend's MsgApp (raft/raft.go:261-281) as wire
egress encodes it in append mode: Reject false, RejectHint 0, the empty snapshot,
and 0, 1 or 3 entries.  Every varint-length edge of a u64 (the EDGES of
make_wire_out_vectors.py) in each of to / from / term / logTerm / index / commit
while the other five hold edges of other lengths; the smallest record and the
one with all six at the maximum.  The bytes are those of
tests/wire_util.gogo_marshal with the entries (the restatement of the
reference's Message.MarshalTo); tests/asan/wire_out_app_asan.cpp checks the
split form of etcd_amd/csrc/hipbatch_wire_out.h against them under the
sanitizers: prefix ‖ entries ‖ suffix.

  fields [N, 8] u64: to, from, term, log_term, index, commit, number of entries,
                     the expected prefix length (fields 1-6)
  off    [N + 1] u64, data u8:   the whole message i = data[off[i], off[i + 1])
  eoff   [N + 1] u64, edata u8:  its entries as MarshalTo writes them (per entry
                     0x3a, varint(Entry.Size()), Entry) = edata[eoff[i], eoff[i + 1])

  python tests/golden/make_wire_out_app_vectors.py
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

FIELDS = ("to", "frm", "term", "log_term", "index", "commit")
NAME = "wire_out_app_vectors.npz"
MASK = (1 << 64) - 1


def entries_of(term, index, n, salt):
    """n entries after `index` (mod 2^64) at `term`: (type, term, index, data) with payloads of
    0 to 6 bytes, nil for some, one of them an EntryConfChange."""
    out = []
    for k in range(n):
        ln = (salt + 3 * k) % 7
        data = None if (salt + k) % 4 == 0 else bytes((salt + k + j) & 0xFF for j in range(ln))
        out.append((1 if (salt + k) % 5 == 0 else 0, term, (index + 1 + k) & MASK, data))
    return out


def vectors():
    """[(to, frm, term, log_term, index, commit, nents)]"""
    E = len(EDGES)
    rows = []
    for fi, f in enumerate(FIELDS):
        for k, v in enumerate(EDGES):
            kw = {o: EDGES[(k + 3 + 4 * ((fi + j) % len(FIELDS))) % E] for j, o in enumerate(FIELDS)}
            kw[f] = v
            if (k + fi) % 4 == 0:  # and small values, zero included
                kw[FIELDS[(fi + 1) % len(FIELDS)]] = k % 3
            rows.append(tuple(kw[o] for o in FIELDS) + ((0, 1, 3)[(k + fi) % 3],))
    for n in (0, 1, 3):
        rows.append((0, 0, 0, 0, 0, 0, n))   # 28 bytes without the entries
        rows.append((MASK,) * 6 + (n,))      # 82: the longest record
    return rows


def build(row, salt):
    """(whole message, entry run, prefix length) of one vector."""
    to, frm, term, lt, idx, com, n = row
    ents = entries_of(term, idx, n, salt)
    full = gogo_marshal(abi.HB_MSG_APP, to=to, frm=frm, term=term, log_term=lt, index=idx, entries=ents, commit=com)
    run = b"".join(key(7, 2) + varint(len(_entry(e))) + _entry(e) for e in ents)
    prefix = 6 + 1 + sum(len(varint(v)) for v in (to, frm, term, lt, idx))
    return full, run, prefix


def main():
    rows = vectors()
    built = [build(r, i) for i, r in enumerate(rows)]
    bare = [len(f) - len(r) for f, r, _ in built]
    assert min(bare) == 28 and max(bare) == 82
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f, _, _ in built])
    eoff = np.zeros(len(rows) + 1, np.uint64)
    eoff[1:] = np.cumsum([len(r) for _, r, _ in built])
    fields = np.array([r + (p,) for r, (_, _, p) in zip(rows, built)], dtype=np.uint64)
    np.savez(os.path.join(HERE, "wire_out", NAME), fields=fields, off=off,
             data=np.frombuffer(b"".join(f for f, _, _ in built), dtype=np.uint8), eoff=eoff,
             edata=np.frombuffer(b"".join(r for _, r, _ in built), dtype=np.uint8))
    print(f"{NAME}: {len(rows)} vectors, {int(off[-1])} bytes, {int(eoff[-1])} of entries")


if __name__ == "__main__":
    main()
