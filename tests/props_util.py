"""References of forwarded proposals on the wire path (include/hipbatch.h).

Receive side: prop_entries is a small parser of the one MsgProp hb_decode_follow takes with
HB_WIRE_PROPS_IN on (the message r.send forwards), None for any other record;
props_reference is tests/ingest_util.follow_reference plus that rule.  rule_cases holds one
record per rule of the contract, on both sides of each.

Send side: replay_forwards turns a step's events into the MsgProp records hb_egress makes with
HB_WIRE_PROPS_OUT on; tests/test_wire_props_replay.py pins it to the oracle's own r.msgs.
"""
import numpy as np

from etcd_amd import abi

from .ingest_util import MAX_ENTS, SNAP, _field, _varint, follow_reference

PROP_HEAD = bytes([0x08, 0x00, 0x10, 0x00, 0x18, 0x00])  # Type 0, Term 0, Index 0: pb.Entry{Data: data}


def prop_entries(rec):
    """The entries of a forwarded MsgProp of the canonical shape, each as (0, HB_ENT_DESC,
    position of the first Data byte in rec or 0); None when any rule of the contract fails
    (all but the group's)."""
    d, l = bytes(rec), len(rec)
    i, head = 0, []
    for key in (0x08, 0x10, 0x18, 0x20, 0x28, 0x30):
        r = _field(d, i, l, key)
        if r is None:
            return None
        head.append(r[0])
        i = r[1]
    if head[0] & 0xFFFFFFFF != abi.HB_MSG_PROP or head[3] or head[4] or head[5]:
        return None
    ents = []
    while i < l and d[i] == 0x3a:
        if len(ents) == MAX_ENTS:
            return None
        r = _varint(d, i + 1, l)
        if r is None or r[0] > l - r[1]:
            return None
        i, end = r[1], r[1] + r[0]
        if d[i:min(i + 6, end)] != PROP_HEAD:
            return None
        i += 6
        if i == end:
            ents.append((0, abi.hb_ent_desc(0, 0, False), 0))
            continue
        r = _field(d, i, end, 0x22)
        if r is None or r[0] > abi.HB_ENT_MAX_DATA or r[0] != end - r[1]:
            return None
        ents.append((0, abi.hb_ent_desc(r[0], 0, True), r[1]))
        i = end
    r = _field(d, i, l, 0x40)
    if r is None or r[0] != 0 or d[r[1]:r[1] + 10] != SNAP:
        return None
    r = _field(d, r[1] + 10, l, 0x50)
    if r is None or r[0] != 0:
        return None
    r = _field(d, r[1], l, 0x58)
    if r is None or r[1] != l or r[0] != 0:
        return None
    return ents if ents else None


def props_reference(data, off, length, group, capacity, group_n, peers, props=True):
    """hb_decode_follow's contract with HB_WIRE_PROPS_IN on (props=False: follow_reference)."""
    base = follow_reference(data, off, length, group, capacity, group_n, peers)
    if not props:
        return base
    n = len(off)
    raw = bytes(np.ascontiguousarray(data, dtype=np.uint8))
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    eterm, edesc, edata = [], [], []
    for k in range(n):
        o, g = int(off[k]), int(group[k])
        out["eoff"][k] = len(eterm)
        b0, b1 = int(base["eoff"][k]), int(base["eoff"][k + 1])
        eterm += base["eterm"][b0:b1].tolist()
        edesc += base["edesc"][b0:b1].tolist()
        edata += base["edata"][b0:b1].tolist()
        if base["status"][k] != abi.HB_WIRE_HOST or g >= capacity:
            continue
        rec = raw[o:o + int(length[k])]
        ents = prop_entries(rec)
        if ents is None:
            continue
        frm = _field(rec, _field(rec, _field(rec, 0, len(rec), 0x08)[1], len(rec), 0x10)[1], len(rec), 0x18)[0]
        slot = abi.HB_SLOT_NONE
        if frm != 0:
            for s in range(min(int(group_n[g]), abi.HB_MAX_REPLICAS)):
                if int(peers[g][s]) == frm:
                    slot = s
                    break
        out["status"][k] = abi.HB_WIRE_OK
        out["group"][k] = g
        out["info"][k] = abi.hb_info(abi.HB_MSG_PROP, slot, False)
        out["term"][k] = out["hint"][k] = out["commit"][k] = 0
        out["index"][k] = len(ents)
        for t, desc, pos in ents:
            eterm.append(t)
            edesc.append(desc)
            edata.append(o + pos if pos else 0)
    out["eoff"][n] = out["n_ent"] = len(eterm)
    out["eterm"] = np.array(eterm, np.uint64).reshape(-1)
    out["edesc"] = np.array(edesc, np.uint32).reshape(-1)
    out["edata"] = np.array(edata, np.uint64).reshape(-1)
    return out


def prop(entries, to=1, frm=2, **kw):
    """gogo_marshal of a MsgProp whose entries carry the given Data (None, b"" or bytes)."""
    from . import wire_util as W
    return W.gogo_marshal(abi.HB_MSG_PROP, to=to, frm=frm, entries=[(0, 0, 0, d) for d in entries], **kw)


def rule_cases():
    """One record per rule of §2, on both sides of each, for a group whose members are
    nodes 1-3: {name: (record, accepted, entries kept)}."""
    from . import wire_util as W
    ent7 = lambda body: W.key(7, 2) + W.varint(len(body)) + body  # noqa: E731
    head = prop([])
    cut = head.index(W.key(8, 0) + W.varint(0) + W.key(9, 2))
    pre, post = head[:cut], head[cut:]
    good = W._entry((0, 0, 0, b"ab"))
    bare = W._entry((0, 0, 0, None))
    raw = lambda ents, **kw: W.gogo_marshal(abi.HB_MSG_PROP, to=1, frm=2, entries=ents, **kw)  # noqa: E731
    return {
        "one entry": (prop([b"ab"]), True, 1),
        "Data nil, empty, one byte": (prop([None, b"", b"x"]), True, 3),
        "128-byte Data (two-byte length)": (prop([bytes(range(128))]), True, 1),
        "from a non-member": (prop([b"ab"], frm=9), True, 1),
        "from node 0": (prop([b"ab"], frm=0), True, 1),
        "three hundred entries": (prop([bytes([k & 0xFF]) * (k % 5) for k in range(300)]), True, 300),
        "no entries": (prop([]), False, 0),
        "Term": (prop([b"ab"], term=7), False, 0),
        "LogTerm": (prop([b"ab"], log_term=1), False, 0),
        "Index": (prop([b"ab"], index=1), False, 0),
        "Commit": (prop([b"ab"], commit=1), False, 0),
        "Reject": (prop([b"ab"], reject=True), False, 0),
        "RejectHint": (prop([b"ab"], hint=1), False, 0),
        "EntryConfChange": (raw([(1, 0, 0, b"cc")]), False, 0),
        "entry Term": (raw([(0, 7, 0, b"ab")]), False, 0),
        "entry Index": (raw([(0, 0, 1, b"ab")]), False, 0),
        "second entry numbered like a MsgApp's": (raw([(0, 0, 0, b"a"), (0, 0, 1, b"b")]), False, 0),
        "non-minimal entry Type": (pre + ent7(b"\x08\x80\x00" + good[2:]) + post, False, 0),
        "non-minimal entry Term": (pre + ent7(b"\x08\x00\x10\x80\x00" + good[4:]) + post, False, 0),
        "reordered entry fields": (pre + ent7(W.key(2, 0) + W.varint(0) + W.key(1, 0) + W.varint(0) + W.key(3, 0) +
                                              W.varint(0)) + post, False, 0),
        "unknown field in an entry": (pre + ent7(good + W.key(9, 0) + W.varint(1)) + post, False, 0),
        "unknown field between entries": (pre + ent7(good) + W.key(20, 0) + W.varint(1) + ent7(good) + post, False, 0),
        "Data past its span": (pre + ent7(bare + W.key(4, 2) + W.varint(3) + b"a") + post, False, 0),
        "bytes after Data": (pre + ent7(good + b"\x00") + post, False, 0),
        "a span past the record": (pre + W.key(7, 2) + W.varint(200) + good + post, False, 0),
        "a five-byte entry": (pre + ent7(bare[:5]) + post, False, 0),
        "a negative Data length": (pre + ent7(bare + W.key(4, 2) + W.varint((1 << 64) - 20)) + post, False, 0),
        "an 11-byte varint": (pre + ent7(bare + W.key(4, 2) + b"\xff" * 10 + b"\x01") + post, False, 0),
        "message fields reordered": (post + pre + ent7(good), False, 0),
        "a snapshot": (raw([(0, 0, 0, b"ab")], snapshot=(None, (1,), 5, 5)), False, 0),
        "trailing field": (prop([b"ab"]) + W.key(20, 0) + W.varint(1), False, 0),
        "truncated": (prop([b"ab"])[:-1], False, 0),
        "a MsgApp with a proposal's entry": (W.gogo_marshal(abi.HB_MSG_APP, to=1, frm=2, entries=[(0, 0, 0, b"ab")]),
                                             False, 0),
    }




def replay_forwards(events, peers, self_id):
    """The MsgProp records of a step's HB_EV_PROP_FWD events, as tuples of
    tests/egress_util.FIELDS with hint = the proposal's arrival index (HB_NO_INDEX for a
    dense props[] proposal), each with its position among the events: [(position, record)].
    A group makes none after its HB_EV_FAULT."""
    dead, out = set(), []
    for pos, e in enumerate(events):
        g, t = int(e["group"]), int(e["type"])
        if g in dead:
            continue
        if t == abi.HB_EV_FAULT:
            dead.add(g)
        elif t == abi.HB_EV_PROP_FWD:
            to = int(e["to"])
            slot = to <= abi.HB_REF_SLOT_MAX
            out.append((pos, (g, abi.HB_MSG_PROP, to if slot else abi.HB_REF_OTHER, int(peers[g][to]) if slot else 0,
                              self_id, 0, 0, 0, 0, False, int(e["x"]))))
    return out


def merge_forwards(events, base, peers, self_id):
    """The records of hb_egress with HB_WIRE_PROPS_OUT on, by group (the only order the engine
    promises across groups): base(events) -> the records of the mode without the bit, as
    tuples of tests/egress_app_util.APP_FIELDS in event order (a replay is independent per
    group); every forward record (host False, ents True) goes where its event stands among
    its group's events."""
    events = np.asarray(events)
    out = []
    for g in sorted({int(x) for x in events["group"]}):
        ev = events[events["group"] == g]
        recs = list(base(ev))
        assert all(r[0] == g for r in recs)
        fwd = replay_forwards(ev, peers, self_id)
        for k, (pos, rec) in enumerate(fwd):
            recs.insert(len(base(ev[:pos])) + k, rec + (False, True))
        out += recs
    return out
