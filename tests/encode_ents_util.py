"""The CPU reference of hb_encode_ents and the entry sources the tests use.

encode_ents_reference(records, src) restates the call: a record is hb_encode's
(tests/egress_app_util.marshal / status_of, i.e. wire_util.gogo_marshal), and one
that carries entries and that the source covers (etcd_amd.splice.source_covers)
is completed with etcd_amd.splice.splice from the entries the source names
(etcd_amd.splice.entry_bytes) and gets HB_WIRE_OK.  tests/test_wire_out_ents.py
pins it to oracle.pyoracle.Raft.readMessages() through tests/egress_app_cases.py.

A source is a dict of numpy arrays: first, start (u64 [capacity]), count (u32
[capacity]), eterm, edata (u64 [n_ent]), edesc (u32 [n_ent]), data (u8); n_ent
and data_len may be given to state less than the arrays hold.
"""
import numpy as np

from etcd_amd import abi
from etcd_amd.splice import entry_bytes, source_covers, splice

from .egress_app_util import entry_tuple, marshal, status_of

SRC_ARRAYS = (("first", np.uint64), ("count", np.uint32), ("start", np.uint64), ("eterm", np.uint64),
              ("edesc", np.uint32), ("edata", np.uint64), ("data", np.uint8))


def n_ent_of(src):
    return int(src.get("n_ent", len(src["edesc"])))


def data_len_of(src):
    return int(src.get("data_len", len(src["data"])))


def record_entries(rec, src):
    """The marshalled entries the device writes for one record, or None when the record is not
    a covered one (no entries, flagged, or outside its group's window)."""
    g, index, hint, host, ents = rec[0], rec[7], rec[10], rec[11], rec[12]
    if not ents or host or rec[2] == abi.HB_REF_OTHER or g >= len(src["first"]):
        return None
    pos = source_covers(index, hint, src["first"][g], src["count"][g], src["start"][g], n_ent_of(src), src["edesc"],
                        src["edata"], data_len_of(src))
    if pos is None:
        return None
    out = []
    for k in range(hint - index):
        d, at = int(src["edesc"][pos + k]), int(src["edata"][pos + k])
        ln = d & abi.HB_ENT_MAX_DATA if d >> 31 else 0
        out.append(entry_bytes(d, int(src["eterm"][pos + k]), index + 1 + k, src["data"][at:at + ln].tobytes() if ln else b""))
    return out


def encode_ents_reference(records, src):
    """records: tuples of egress_app_util.APP_FIELDS in batch order.  Returns (the bytes of
    every record, off u64 [n + 1], status u8 [n])."""
    recs, st = [], np.zeros(len(records), np.uint8)
    for i, rec in enumerate(records):
        raw, s = marshal(rec), status_of(rec)
        ents = record_entries(rec, src)
        if ents is not None:
            assert s & abi.HB_WIRE_SPLICE
            raw, s = splice(raw, s, ents), abi.HB_WIRE_OK
        recs.append(raw)
        st[i] = s
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    return recs, off, st


def records_of(batch, n, self_id):
    """The record tuples of the first n records of hb_out_batch arrays (numpy)."""
    out = []
    for i in range(n):
        info = int(batch["info"][i])
        out.append((int(batch["group"][i]), info & 0xF, (info >> 4) & 0xF, int(batch["to"][i]), self_id,
                    int(batch["term"][i]), int(batch["log_term"][i]), int(batch["index"][i]), int(batch["commit"][i]),
                    bool((info >> 8) & 1), int(batch["hint"][i]), bool(info & abi.HB_OUT_HOST),
                    bool(info & abi.HB_OUT_ENTS)))
    return out


def build_source(windows, capacity):
    """windows: {group: (first index, [(type, term, data or None)])}; the entries of the groups in
    ascending group order, their payloads back to back.  Groups without a window have count 0."""
    src = dict(first=np.zeros(capacity, np.uint64), count=np.zeros(capacity, np.uint32),
               start=np.zeros(capacity, np.uint64))
    eterm, edesc, edata, blob = [], [], [], bytearray()
    for g in sorted(windows):
        first, ents = windows[g]
        src["first"][g], src["count"][g], src["start"][g] = first, len(ents), len(eterm)
        for t, term, data in ents:
            eterm.append(term)
            edesc.append(abi.hb_ent_desc(len(data) if data is not None else 0, t, data is not None))
            edata.append(len(blob))
            if data:
                blob += data
    src["eterm"] = np.array(eterm, dtype=np.uint64)
    src["edesc"] = np.array(edesc, dtype=np.uint32)
    src["edata"] = np.array(edata, dtype=np.uint64)
    src["data"] = np.frombuffer(bytes(blob), dtype=np.uint8).copy()
    return src


def log_source(rafts, capacity=None):
    """A source that covers every log: group g's window is the whole log of rafts[g], entry i
    being egress_app_util.entry_tuple(g, i, its term)."""
    win = {}
    for g, r in enumerate(rafts):
        ents = r.entries()
        if ents:
            win[g] = (ents[0][0], [(0, t, entry_tuple(g, i, t)[3]) for i, t in ents])
    return build_source(win, len(rafts) if capacity is None else capacity)
