"""Completing a MsgApp record of wire egress in append mode.

hb_encode writes a record that carries entries (HB_OUT_ENTS) as prefix ‖ suffix
and sets status = HB_WIRE_SPLICE | prefix_len.  Message.MarshalTo writes the
entries as one contiguous run of field 7 between Index and Commit, so the full
message is the prefix, that run, the suffix: a transport sends the three parts
with one gather write (INTEGRATION.md shows it with an iovec).

hb_encode_ents writes the run on the device for every record its
entry source covers; entry_bytes and source_covers restate its entry encoding and
its coverage rule for the host.
"""
from . import abi


def varint(v):
    """encodeVarintRaft."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def entries_run(entries):
    """The bytes Message.MarshalTo writes for m.Entries: per marshalled entry
    0x3a, varint(Entry.Size()), the entry."""
    return b"".join(b"\x3a" + varint(len(e)) + bytes(e) for e in entries)


def splice(record, status, entries=()):
    """record: the bytes hb_encode wrote for one record; status: its status byte;
    entries: the marshalled raftpb.Entry of each entry it carries, in index order.
    Returns the message's wire bytes: the record itself unless status carries
    HB_WIRE_SPLICE, else prefix ‖ entries ‖ suffix."""
    record = bytes(record)
    status = int(status)
    if not status & abi.HB_WIRE_SPLICE:
        if entries:
            raise ValueError("a record without HB_WIRE_SPLICE carries no entries")
        return record
    k = status & 0x7F
    if k > len(record):
        raise ValueError("prefix length past the record")
    return record[:k] + entries_run(entries) + record[k:]


def entry_bytes(desc, term, index, data=b""):
    """The marshalled raftpb.Entry (Entry.MarshalTo) of a descriptor: desc = abi.hb_ent_desc(len(Data),
    Type, Data != nil); `data` holds at least len(Data) bytes when the descriptor has Data."""
    desc = int(desc)
    out = b"\x08" + varint((desc >> 30) & 1) + b"\x10" + varint(int(term)) + b"\x18" + varint(int(index))
    if desc >> 31:
        ln = desc & abi.HB_ENT_MAX_DATA
        if len(data) < ln:
            raise ValueError("fewer Data bytes than the descriptor states")
        out += b"\x22" + varint(ln) + bytes(data[:ln])
    return out


def source_covers(index, hint, first, count, start, n_ent, edesc=(), edata=(), data_len=0):
    """hb_encode_ents' coverage rule for a record that carries entries (index, hint] of a group
    whose window holds `count` entries from index `first` at position `start` of the per-entry
    arrays (n_ent elements; edesc / edata are read only inside the window).  Returns the
    position of entry index + 1, or None when the record is not covered."""
    index, hint, first, count, start, n_ent = (int(v) for v in (index, hint, first, count, start, n_ent))
    if hint <= index or count == 0 or index + 1 < first:
        return None
    if (index + 1 - first) + (hint - index) > count or start + count > n_ent:
        return None
    pos = start + index + 1 - first
    for k in range(pos, pos + hint - index):
        d = int(edesc[k])
        if d >> 31 and int(edata[k]) + (d & abi.HB_ENT_MAX_DATA) > int(data_len):
            return None
    return pos
