"""Generate tests/golden/wire_in/wire_props_vectors.npz: vectors of the forwarded-proposal rule.

Test infrastructure only, built from tests/props_util.rule_cases (the bytes of
tests/wire_util.gogo_marshal): one MsgProp per rule of hb_decode_follow's HB_WIRE_PROPS_IN
contract, on both sides of each, for etcd_amd/csrc/hipbatch_wire_in.h, which
tests/asan/wire_props_asan.cpp runs over them under the sanitizers.

  accept [N] u8: the parser takes the record under the proposal rule
  frm    [N] u64: m.From of an accepted record
  off    [N + 1] u64, data u8: message i = data[off[i], off[i + 1])
  eoff   [N + 1] u64: the entries of message i are eoff[i] .. eoff[i + 1] of
  edesc  [E] u32 (HB_ENT_DESC), epos [E] u64 (position of the first Data byte inside the
         message, 0 when Data is absent)

  python tests/golden/make_wire_props_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.props_util import prop_entries, rule_cases  # noqa: E402

NAME = "wire_props_vectors.npz"


def build():
    """The arrays of the fixture."""
    recs, accept, frm, edesc, epos, eoff = [], [], [], [], [], [0]
    for name, (rec, ok, ne) in rule_cases().items():
        ents = prop_entries(rec)
        assert (ents is not None) == ok and len(ents or ()) == ne, name
        for _, desc, pos in ents or ():
            edesc.append(desc)
            epos.append(pos)
        eoff.append(len(edesc))
        recs.append(rec)
        accept.append(int(ok))
        frm.append({"from a non-member": 9, "from node 0": 0}.get(name, 2) if ok else 0)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return dict(accept=np.array(accept, np.uint8), frm=np.array(frm, np.uint64), off=off,
                data=np.frombuffer(b"".join(recs), dtype=np.uint8), eoff=np.array(eoff, np.uint64),
                edesc=np.array(edesc, np.uint32), epos=np.array(epos, np.uint64))


def main():
    z = build()
    os.makedirs(os.path.join(HERE, "wire_in"), exist_ok=True)
    np.savez(os.path.join(HERE, "wire_in", NAME), **z)
    print(f"{NAME}: {len(z['accept'])} vectors, {int(z['off'][-1])} bytes, {len(z['edesc'])} entries")


if __name__ == "__main__":
    main()
