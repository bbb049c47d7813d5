"""Generate tests/golden/wire_out/wire_out_vote_vectors.npz: MsgVote encoder vectors.

Test infrastructure only.  campaign's MsgVote (raft/raft.go:429-443) as wire
egress encodes it in vote mode: Commit 0, Reject false, RejectHint 0, and every
varint-length edge of a u64 (the EDGES of make_wire_out_vectors.py) in each of
to / from / term / logTerm / index while the other four hold edges of other
lengths; the smallest record and the one with all five at the maximum.  The
bytes are those of tests/wire_util.gogo_marshal (the restatement of the
reference's Message.MarshalTo); tests/asan/wire_out_vote_asan.cpp checks
etcd_amd/csrc/hipbatch_wire_out.h against them under the sanitizers.

  fields [N, 9] u64: type, to, from, term, log_term, index, commit, reject, hint
  off    [N + 1] u64, data u8: record i = data[off[i], off[i + 1])

  python tests/golden/make_wire_out_vote_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from etcd_amd import abi  # noqa: E402
from tests.golden.make_wire_out_vectors import EDGES  # noqa: E402
from tests.wire_util import gogo_marshal  # noqa: E402

FIELDS = ("to", "frm", "term", "log_term", "index")
NAME = "wire_out_vote_vectors.npz"


def vectors():
    E = len(EDGES)
    rows = []
    for fi, f in enumerate(FIELDS):
        for k, v in enumerate(EDGES):
            # the swept field takes v, the others edges 3, 7, 11, ... places further on
            kw = {o: EDGES[(k + 3 + 4 * ((fi + j) % len(FIELDS))) % E] for j, o in enumerate(FIELDS)}
            kw[f] = v
            if (k + fi) % 4 == 0:  # and small values, zero included
                kw[FIELDS[(fi + 1) % len(FIELDS)]] = k % 3
            rows.append((abi.HB_MSG_VOTE, kw["to"], kw["frm"], kw["term"], kw["log_term"], kw["index"], 0, 0, 0))
    top = (1 << 64) - 1
    rows.append((abi.HB_MSG_VOTE, 0, 0, 0, 0, 0, 0, 0, 0))            # 28 bytes
    rows.append((abi.HB_MSG_VOTE, top, top, top, top, top, 0, 0, 0))  # 73 bytes
    return rows


def main():
    rows = vectors()
    recs = [gogo_marshal(t, to=to, frm=frm, term=term, log_term=lt, index=idx, commit=com, reject=bool(rej), hint=hint)
            for t, to, frm, term, lt, idx, com, rej, hint in rows]
    assert min(map(len, recs)) == 28 and max(map(len, recs)) == 73
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    np.savez(os.path.join(HERE, "wire_out", NAME), fields=np.array(rows, dtype=np.uint64), off=off,
             data=np.frombuffer(b"".join(recs), dtype=np.uint8))
    print(f"{NAME}: {len(recs)} records, {int(off[-1])} bytes")


if __name__ == "__main__":
    main()
