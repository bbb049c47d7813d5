"""Reference of hb_decode_follow on the CPU (include/hipbatch.h).

Status and header come from the oracle's Message.Unmarshal
(oracle.pyoracle.unmarshal_message) and the rule table of the contract; the
entries from canonical_entries, a small parser of the one shape whose entries
the device keeps, which returns None for any other shape.
"""
import numpy as np

from etcd_amd import abi
from oracle.pyoracle import unmarshal_message

U64 = (1 << 64) - 1
SNAP = bytes([0x4a, 0x08, 0x12, 0x06, 0x0a, 0x00, 0x10, 0x00, 0x18, 0x00])
LOCAL = (abi.HB_MSG_HUP, abi.HB_MSG_BEAT, abi.HB_MSG_UNREACHABLE, abi.HB_MSG_SNAP_STATUS)
RESP = (abi.HB_MSG_APP_RESP, abi.HB_MSG_VOTE_RESP, abi.HB_MSG_HEARTBEAT_RESP)
FOLLOW = (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_VOTE)
MAX_ENTS = (1 << 23) - 1


def _varint(d, i, end):
    """A varint of at most 10 bytes at d[i:end] -> (value mod 2^64, next) or None."""
    v = 0
    for k in range(10):
        if i >= end:
            return None
        b = d[i]
        i += 1
        v |= (b & 0x7F) << (7 * k)
        if b < 0x80:
            return v & U64, i
    return None


def _field(d, i, end, key):
    if i >= end or d[i] != key:
        return None
    return _varint(d, i + 1, end)


def canonical_entries(rec):
    """The entries of a record of the canonical MarshalTo shape, each as
    (term, HB_ENT_DESC, position of the first Data byte in rec or 0), or None
    when the record has any other shape or an entry misses a check."""
    d, l = bytes(rec), len(rec)
    i, head = 0, []
    for key in (0x08, 0x10, 0x18, 0x20, 0x28, 0x30):
        r = _field(d, i, l, key)
        if r is None:
            return None
        head.append(r[0])
        i = r[1]
    index = head[5]
    ents = []
    while i < l and d[i] == 0x3a:
        if len(ents) == MAX_ENTS:
            return None
        r = _varint(d, i + 1, l)
        if r is None or r[0] > l - r[1]:
            return None
        i, end = r[1], r[1] + r[0]
        if end - i < 2 or d[i] != 0x08 or d[i + 1] > 1:
            return None
        etype = d[i + 1]
        r = _field(d, i + 2, end, 0x10)
        if r is None:
            return None
        term, i = r
        r = _field(d, i, end, 0x18)
        if r is None or r[0] != (index + 1 + len(ents)) & U64:
            return None
        i = r[1]
        if i == end:
            ents.append((term, abi.hb_ent_desc(0, etype, False), 0))
            continue
        r = _field(d, i, end, 0x22)
        if r is None or r[0] > abi.HB_ENT_MAX_DATA or r[0] != end - r[1]:
            return None
        ents.append((term, abi.hb_ent_desc(r[0], etype, True), r[1]))
        i = end
    r = _field(d, i, l, 0x40)
    if r is None or d[r[1]:r[1] + 10] != SNAP:
        return None
    r = _field(d, r[1] + 10, l, 0x50)
    if r is None:
        return None
    r = _field(d, r[1], l, 0x58)
    if r is None or r[1] != l:
        return None
    return ents


def follow_reference(data, off, length, group, capacity, group_n, peers):
    """hb_decode_follow's contract: dict of status [n], the six batch arrays and
    eoff [n + 1] (record n the sentinel), n_ent, eterm / edesc / edata [n_ent]."""
    n = len(off)
    raw = bytes(np.ascontiguousarray(data, dtype=np.uint8))
    out = dict(status=np.zeros(n, np.uint8), group=np.full(n + 1, 0xFFFFFFFF, np.uint32),
               info=np.zeros(n + 1, np.uint32), term=np.zeros(n + 1, np.uint64), index=np.zeros(n + 1, np.uint64),
               hint=np.zeros(n + 1, np.uint64), commit=np.zeros(n + 1, np.uint64), eoff=np.zeros(n + 1, np.uint64))
    eterm, edesc, edata = [], [], []
    for k in range(n):
        o, g = int(off[k]), int(group[k])
        rec = raw[o:o + int(length[k])]
        out["eoff"][k] = len(eterm)
        rc, m = unmarshal_message(rec)
        gok = g < capacity
        slot = abi.HB_SLOT_NONE
        if rc == 0 and gok and m.from_ != 0:
            for s in range(min(int(group_n[g]), abi.HB_MAX_REPLICAS)):
                if int(peers[g][s]) == m.from_:
                    slot = s
                    break
        ents = None
        if rc == 1:
            st = abi.HB_WIRE_ERROR
        elif rc == 2:
            st = abi.HB_WIRE_PANIC
        elif rc == 3:
            st = abi.HB_WIRE_HOST
        elif m.type in LOCAL:
            st = abi.HB_WIRE_LOCAL
        elif m.type in RESP:
            st = abi.HB_WIRE_OK if gok else abi.HB_WIRE_BADGROUP
        elif m.type not in FOLLOW or not gok:
            st = abi.HB_WIRE_HOST
        elif m.type == abi.HB_MSG_VOTE:
            st = abi.HB_WIRE_OK if slot != abi.HB_SLOT_NONE else abi.HB_WIRE_HOST
        elif m.type == abi.HB_MSG_APP and m.nentries:
            ents = canonical_entries(rec)
            st = abi.HB_WIRE_OK if ents is not None else abi.HB_WIRE_HOST
        else:
            st = abi.HB_WIRE_OK
        out["status"][k] = st
        if st != abi.HB_WIRE_OK:
            continue
        out["group"][k] = g
        out["info"][k] = abi.hb_info(m.type, slot, bool(m.reject))
        out["term"][k], out["index"][k] = m.term, m.index
        if m.type in RESP:
            out["hint"][k] = m.reject_hint
        else:
            out["hint"][k] = 0 if m.type == abi.HB_MSG_HEARTBEAT else m.log_term
            out["commit"][k] = 0 if m.type == abi.HB_MSG_VOTE else m.commit
        for t, desc, pos in ents or ():
            eterm.append(t)
            edesc.append(desc)
            edata.append(o + pos if pos else 0)
    out["eoff"][n] = out["n_ent"] = len(eterm)
    out["eterm"] = np.array(eterm, np.uint64).reshape(-1)
    out["edesc"] = np.array(edesc, np.uint32).reshape(-1)
    out["edata"] = np.array(edata, np.uint64).reshape(-1)
    return out


def rule_cases():
    """One record per rule of the contract, for a group whose members are nodes 1-3:
    {name: (record, expected status, entries kept)}."""
    from . import wire_util as W
    e = lambda i, ty=0, d=b"ab": (ty, 7, i, d)  # noqa: E731
    app = lambda ents: W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=2, term=7, log_term=7, index=10, commit=9,  # noqa: E731
                                      entries=ents)
    ent7 = lambda body: W.key(7, 2) + W.varint(len(body)) + body  # noqa: E731
    head = W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=2, term=7, log_term=7, index=10)
    cut = head.index(W.key(8, 0) + W.varint(0) + W.key(9, 2))
    pre, post = head[:cut], head[cut:]
    good = W._entry(e(11))
    OK, HOST = abi.HB_WIRE_OK, abi.HB_WIRE_HOST
    return {
        "ok": (app([e(11), e(12, 1, None), e(13, 0, b"")]), OK, 3),
        "no entries, reordered": (post + pre, OK, 0),
        "gap": (app([e(11), e(13)]), HOST, 0),
        "type 2": (app([e(11, 2)]), HOST, 0),
        "reordered entry fields": (pre + ent7(W.key(2, 0) + W.varint(7) + W.key(1, 0) + W.varint(0) + W.key(3, 0) +
                                              W.varint(11)) + post, HOST, 0),
        "unknown field in an entry": (pre + ent7(good + W.key(9, 0) + W.varint(1)) + post, HOST, 0),
        "unknown field between entries": (pre + ent7(good) + W.key(20, 0) + W.varint(1) + ent7(W._entry(e(12))) + post,
                                          HOST, 0),
        "dropped Entry error": (pre + ent7(W.key(4, 2) + W.varint(50) + b"\x01") + post, HOST, 0),
        "non-minimal entry type": (pre + ent7(b"\x08\x80\x00" + good[2:]) + post, HOST, 0),
        "vote of a member": (W.gogo_marshal(abi.HB_MSG_VOTE, to=1, frm=3, term=8, log_term=7, index=10), OK, 0),
        "vote of a non-member": (W.gogo_marshal(abi.HB_MSG_VOTE, to=1, frm=9, term=8, log_term=7, index=10), HOST, 0),
        "app of a non-member": (W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=9, term=8, log_term=7, index=10), OK, 0),
        "heartbeat with an entry": (W.gogo_marshal(abi.HB_MSG_HEARTBEAT, to=1, frm=2, term=7, commit=5, entries=[e(1)]),
                                    OK, 0),
        "snap": (W.gogo_marshal(abi.HB_MSG_SNAP, to=1, frm=2, term=7, snapshot=(b"s", (1, 2, 3), 5, 6)), HOST, 0),
        "prop": (W.gogo_marshal(abi.HB_MSG_PROP, to=1, frm=2, entries=[(0, 0, 0, b"p")]), HOST, 0),
    }


def records_of(batch, peers, data_of, outsider=1000):
    """A follower-side batch (etcd_amd.synth: group / info / term / index / hint / commit /
    eoff / eterm) as gogo-marshalled records.  m.From = the id of the sender's slot in the
    group's peer row (`outsider` for HB_SLOT_NONE); entry k of message i carries Data
    data_of(i, k) (None, b"" or bytes).  A MsgSnap carries a snapshot of its index / term."""
    from . import wire_util as W
    n = len(batch["group"])
    eoff = np.append(np.asarray(batch["eoff"], np.int64), len(batch["eterm"])) if batch.get("eoff") is not None \
        else np.zeros(n + 1, np.int64)
    recs = []
    for i in range(n):
        info, g = int(batch["info"][i]), int(batch["group"][i])
        t, slot = info & 0xF, (info >> 4) & 0xF
        frm = outsider if slot == abi.HB_SLOT_NONE else int(peers[g][slot])
        idx, hint = int(batch["index"][i]), int(batch["hint"][i]) if batch.get("hint") is not None else 0
        com = int(batch["commit"][i]) if batch.get("commit") is not None else 0
        kw = dict(to=int(peers[g][0]), frm=frm, term=int(batch["term"][i]))
        if t == abi.HB_MSG_SNAP:
            recs.append(W.gogo_marshal(t, snapshot=(b"snap", (1, 2, 3), idx, hint), **kw))
            continue
        if t in (abi.HB_MSG_APP, abi.HB_MSG_VOTE):
            kw.update(log_term=hint, index=idx)
        elif t != abi.HB_MSG_HEARTBEAT:
            kw.update(index=idx, hint=hint, reject=bool((info >> 8) & 1))
        if t in (abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT):
            kw.update(commit=com)
        ents = [(0, int(batch["eterm"][e]), idx + 1 + k, data_of(i, k)) for k, e in enumerate(range(eoff[i], eoff[i + 1]))]
        recs.append(W.gogo_marshal(t, entries=ents, **kw))
    return recs
