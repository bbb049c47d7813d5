"""The index frame of a peer stream and the group-id directory on the host.

hb_frame writes one index frame per peer beside the peer's byte span: the group id and
the length of every record, so a transport ships two spans per peer and nothing per
record.  This module restates the format, the hole rule, the receiver's checks and the
directory's probe (etcd_amd/csrc/hipbatch_frame.h) for a host that receives frames
without a GPU; the tests compare hb_frame / hb_unframe / hb_gid_dir_build with it bit
for bit.

    0 u32 magic "HBF1" | 4 u32 flags 0 | 8 u64 from | 16 u64 to | 24 u64 seq |
    32 u64 bytes | 40 u32 count c | 44 u32 holes | 48 u64 gid[c] |
    48 + 8c u32 len[c] (bit 31 = hole) | 4 zero bytes when c is odd
"""
import struct

import numpy as np

from . import abi

MAGIC = 0x31464248
HEADER = 48
HOLE = 0x80000000
LEN_MASK = 0x7FFFFFFF
IMPOSSIBLE = (1 << 64) - 1
NO_SLOT = 0xFFFFFFFF
OVERSIZE = 0xFFFFFFFF
MAX_FRAMES = 256
_M64 = (1 << 64) - 1
_HDR = struct.Struct("<IIQQQQII")


def isize(c):
    """Bytes of a frame of c rows; 0 for no rows (an empty bin makes no frame)."""
    return HEADER + 12 * c + 4 * (c & 1) if c else 0


def rows(length):
    """The c with isize(c) == length, or IMPOSSIBLE."""
    if length == 0:
        return 0
    if length < HEADER + 16:
        return IMPOSSIBLE
    body = length - HEADER
    r = body % 12
    if r not in (0, 4):
        return IMPOSSIBLE
    c = (body - r) // 12
    if c == 0 or c > 0xFFFFFFFF or (c & 1) != (r == 4):
        return IMPOSSIBLE
    return c


def row(status, group, capacity, gid, byte_len):
    """(gid word, len word, oversize) of one record: the hole rule."""
    ok = group < capacity
    g = int(gid[group]) if ok else 0
    hole = status != abi.HB_WIRE_OK or not ok or g == 0
    return g, (byte_len & LEN_MASK) | (HOLE if hole else 0), byte_len > LEN_MASK


def build_frame(group, off, status, first, c, gid, capacity, from_id, to_id, seq, nbytes):
    """One bin's frame: records first .. first + c - 1 of a binned batch.  Returns (bytes, fstat):
    fstat = the hole count, or OVERSIZE (the header then has magic 0)."""
    if c == 0:
        return b"", 0
    gids, lens, over = [], [], False
    for i in range(first, first + c):
        g, w, o = row(int(status[i]), int(group[i]), capacity, gid, (int(off[i + 1]) - int(off[i])) & _M64)
        gids.append(g)
        lens.append(w)
        over |= o
    holes = sum(1 for w in lens if w & HOLE)
    out = _HDR.pack(0 if over else MAGIC, 0, from_id, to_id, seq, nbytes, c, holes)
    out += struct.pack("<%dQ" % c, *gids) + struct.pack("<%dI" % c, *lens) + (b"\0\0\0\0" if c & 1 else b"")
    return out, (OVERSIZE if over else holes)


def build_index(group, to, off, status, bin_off, span, gid, capacity, self_id, seq):
    """hb_frame on the host: (index bytes, ispan [peers + 2], fstat [peers + 1]) of a binned batch;
    bin_off / span have peers + 2 words."""
    npeers = len(bin_off) - 2
    index, ispan, fstat = b"", [], []
    for b in range(npeers):
        ispan.append(len(index))
        first, c = int(bin_off[b]), int(bin_off[b + 1]) - int(bin_off[b])
        f, st = build_frame(group, off, status, first, c, gid, capacity, self_id, int(to[first]) if c else 0, seq,
                            (int(span[b + 1]) - int(span[b])) & _M64)
        index += f
        fstat.append(st)
    ispan += [len(index), len(index)]
    fstat.append(0)
    return index, np.asarray(ispan, np.uint64), np.asarray(fstat, np.uint32)


def parse_index(frame):
    """A frame's header fields and columns: dict(magic, flags, from_id, to, seq, bytes, count, holes,
    gid [c], len [c], hole [c]); c comes from the frame's length (ValueError if no count gives it)."""
    frame = bytes(frame)
    c = rows(len(frame))
    if c == IMPOSSIBLE or c == 0:
        raise ValueError("no row count gives a frame of %d bytes" % len(frame))
    magic, flags, from_id, to, seq, nbytes, count, holes = _HDR.unpack_from(frame, 0)
    gid = np.frombuffer(frame, "<u8", c, HEADER)
    w = np.frombuffer(frame, "<u4", c, HEADER + 8 * c)
    return dict(magic=magic, flags=flags, from_id=from_id, to=to, seq=seq, bytes=nbytes, count=count, holes=holes,
                gid=gid, len=w & np.uint32(LEN_MASK), hole=(w & np.uint32(HOLE)) != 0)


def validate(frame, c, self_id, from_id, bytes_len):
    """fstatus of one received frame of c rows (the first check that fails, in HB_FRAME_* order)."""
    if c == 0:
        return abi.HB_FRAME_OK if bytes_len == 0 else abi.HB_FRAME_BAD_LENGTH
    p = parse_index(frame)
    if p["magic"] != MAGIC or p["flags"] != 0:
        return abi.HB_FRAME_BAD_MAGIC
    if p["count"] != c:
        return abi.HB_FRAME_BAD_COUNT
    if p["to"] != self_id or p["from_id"] != from_id:
        return abi.HB_FRAME_BAD_ROUTE
    if p["bytes"] != bytes_len or int(p["len"].astype(np.uint64).sum()) != bytes_len:
        return abi.HB_FRAME_BAD_LENGTH
    return abi.HB_FRAME_OK


# ---- the directory ----------------------------------------------------------------------
def mix(x):
    """splitmix64."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def dir_cap(count):
    """The smallest legal cap for `count` ids: a power of two, >= 64 and >= 2 x count."""
    cap = 64
    while cap < 2 * count:
        cap *= 2
    return cap


class Directory:
    """gd_build / gd_lookup: ids -> slots by open addressing (key 0 = empty)."""

    def __init__(self, gid, cap=None):
        self.cap = dir_cap(len(gid)) if cap is None else cap
        if self.cap & (self.cap - 1) or self.cap == 0:
            raise ValueError("cap must be a power of two")
        self.key = [0] * self.cap
        self.slot = [0] * self.cap
        self.dups = 0
        for i, g in enumerate(gid):
            g = int(g)
            if g == 0:
                continue
            p = mix(g) & (self.cap - 1)
            for _ in range(self.cap):
                if self.key[p] == 0:
                    self.key[p], self.slot[p] = g, i
                    break
                if self.key[p] == g:
                    self.dups += 1
                    break
                p = (p + 1) & (self.cap - 1)

    def lookup(self, g):
        p = mix(g) & (self.cap - 1)
        for _ in range(self.cap):
            if self.key[p] == g:
                return self.slot[p]
            if self.key[p] == 0:
                return NO_SLOT
            p = (p + 1) & (self.cap - 1)
        return NO_SLOT


def unframe(index, frames, self_id, lookup):
    """hb_unframe on the host.  index: the index buffer; frames: [(index_off, index_len, bytes_off,
    bytes_len, from), ...]; lookup: gid -> slot or NO_SLOT (Directory.lookup, or a dict's get with
    NO_SLOT).  Returns (off u64 [n], len u32 [n], group u32 [n], fstatus u32 [frames], n_unknown)."""
    index = bytes(index)
    off, ln, grp, fstatus, unknown = [], [], [], [], 0
    if len(frames) > MAX_FRAMES:
        raise ValueError("more than %d frames" % MAX_FRAMES)
    for ioff, ilen, boff, blen, from_id in frames:
        c = rows(ilen)
        if c == IMPOSSIBLE or ioff % 8 or ioff + ilen > len(index):
            raise ValueError("bad frame extent")
        fr = index[ioff:ioff + ilen]
        st = validate(fr, c, self_id, from_id, blen)
        fstatus.append(st)
        if st != abi.HB_FRAME_OK or c == 0:
            off += [0] * c
            ln += [0] * c
            grp += [NO_SLOT] * c
            continue
        p = parse_index(fr)
        run = 0
        for j in range(c):
            off.append(boff + run)
            run += int(p["len"][j])
            g = int(p["gid"][j])
            s = NO_SLOT
            if not p["hole"][j] and g != 0:
                s = lookup(g)
                unknown += s == NO_SLOT
            ln.append(int(p["len"][j]) if s != NO_SLOT else 0)
            grp.append(s)
    return (np.asarray(off, np.uint64), np.asarray(ln, np.uint32), np.asarray(grp, np.uint32),
            np.asarray(fstatus, np.uint32), unknown)
