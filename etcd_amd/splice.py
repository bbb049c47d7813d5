"""Completing a MsgApp record of wire egress in append mode.

hb_encode writes a record that carries entries (HB_OUT_ENTS) as prefix ‖ suffix
and sets status = HB_WIRE_SPLICE | prefix_len.  Message.MarshalTo writes the
entries as one contiguous run of field 7 between Index and Commit, so the full
message is the prefix, that run, the suffix: a transport sends the three parts
with one gather write (INTEGRATION.md shows it with an iovec).
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
