"""Generate tests/golden/wire_out/wire_out_vectors.npz: encoder vectors of wire egress.

Test infrastructure only.  Payload-free raftpb.Message records of the four
types wire egress encodes, with the bytes tests/wire_util.gogo_marshal (the
restatement of the reference's Message.MarshalTo) writes for them: every
varint-length edge of a u64 in every field (the EDGES list of
tests/test_wire_gpu.py) while the other fields hold edges of other lengths,
the smallest record, and the all-maximum 91-byte one.
tests/asan/wire_out_asan.cpp checks etcd_amd/csrc/hipbatch_wire_out.h against
them under the sanitizers.

  fields [N, 9] u64: type, to, from, term, log_term, index, commit, reject, hint
  off    [N + 1] u64, data u8: record i = data[off[i], off[i + 1])

  python tests/golden/make_wire_out_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from etcd_amd import abi  # noqa: E402
from tests.wire_util import gogo_marshal  # noqa: E402

EDGES = sorted({v for k in range(1, 10) for v in ((1 << 7 * k) - 1, 1 << 7 * k)} | {1 << 63, (1 << 64) - 1})
TYPES = (abi.HB_MSG_APP_RESP, abi.HB_MSG_HEARTBEAT_RESP, abi.HB_MSG_VOTE_RESP, abi.HB_MSG_HEARTBEAT)
FIELDS = ("to", "frm", "term", "log_term", "index", "commit", "hint")


def vectors():
    E = len(EDGES)
    rows = []
    for ti, t in enumerate(TYPES):
        for fi, f in enumerate(FIELDS):
            for k, v in enumerate(EDGES):
                # the swept field takes v, the others edges 3, 7, 11, ... places further on
                kw = {o: EDGES[(k + 3 + 4 * ((fi + j) % len(FIELDS))) % E] for j, o in enumerate(FIELDS)}
                kw[f] = v
                if (k + fi + ti) % 4 == 0:  # and small values, zero included
                    kw[FIELDS[(fi + 1) % len(FIELDS)]] = k % 3
                rows.append((t, kw["to"], kw["frm"], kw["term"], kw["log_term"], kw["index"], kw["commit"],
                             (k + fi) & 1, kw["hint"]))
    top = (1 << 64) - 1
    for t in TYPES:
        rows.append((t, 0, 0, 0, 0, 0, 0, 0, 0))               # 28 bytes
        rows.append((t, top, top, top, top, top, top, 1, top))  # 91 bytes
    return rows


def main():
    rows = vectors()
    recs = [gogo_marshal(t, to=to, frm=frm, term=term, log_term=lt, index=idx, commit=com, reject=bool(rej), hint=hint)
            for t, to, frm, term, lt, idx, com, rej, hint in rows]
    assert min(map(len, recs)) == 28 and max(map(len, recs)) == 91
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    np.savez(os.path.join(HERE, "wire_out", "wire_out_vectors.npz"), fields=np.array(rows, dtype=np.uint64), off=off,
             data=np.frombuffer(b"".join(recs), dtype=np.uint8))
    print(f"wire_out_vectors.npz: {len(recs)} records, {int(off[-1])} bytes")


if __name__ == "__main__":
    main()
