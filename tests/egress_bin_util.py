"""The reference of hb_egress_bin, from numpy alone.

bin_reference() is the contract restated: a record's bin is the caller's
position of its destination id in the node table, or "other" (bin len(ids))
for an unknown id and for a record whose to_ref is HB_REF_OTHER; the output
is the stable sort of the records by bin.  Stability makes the result a pure
function of the input, so every GPU test compares exactly.
"""
import numpy as np

from etcd_amd import abi

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
# tests/asan/bin_asan.cpp table(): the edge ids, then k x GOLD mod 2^64
ASAN_EDGE = (1, 1 << 32, 1 << 63, M64, (1 << 32) | 1, (7 << 32) | 5, (5 << 32) | 7, (7 << 32) | 6, (6 << 32) | 5,
             0xFFFFFFFF, 0xFFFFFFFF00000000, (1 << 63) | 1)
ASAN_SIZES = (1, 2, 3, 254, 255)


def bins_of(to, info, ids):
    """The bin of every record (int64 array)."""
    to = np.asarray(to, dtype=np.uint64)
    info = np.asarray(info, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.uint64)
    n = len(ids)
    b = np.full(len(to), n, dtype=np.int64)
    for k in range(n):  # the caller's order; ids are distinct
        b[to == ids[k]] = k
    b[((info >> np.uint32(4)) & np.uint32(0xF)) == abi.HB_REF_OTHER] = n
    return b


def bin_reference(to, info, ids):
    """(order, bin_off): output record j is input record order[j]; bin b is
    output records bin_off[b] .. bin_off[b + 1], b in [0, len(ids)]; bin_off has
    len(ids) + 2 entries and ends with the record count."""
    b = bins_of(to, info, ids)
    order = np.argsort(b, kind="stable")
    counts = np.bincount(b, minlength=len(ids) + 1)
    bin_off = np.zeros(len(ids) + 2, dtype=np.uint64)
    bin_off[1:] = np.cumsum(counts)
    return order, bin_off


def asan_table(n):
    """The node table of n ids that tests/asan/bin_asan.cpp builds, in the caller's order."""
    ids = list(ASAN_EDGE[:n])
    k = 1
    while len(ids) < n:
        ids.append((k * GOLD) & M64)
        k += 1
    return np.array(ids, dtype=np.uint64)


def asan_probes(ids):
    """Its probes: every id, each id - 1 and + 1 (wrapping), halves swapped, and 0."""
    out = []
    for v in (int(x) for x in ids):
        out += [v, (v - 1) & M64, (v + 1) & M64, ((v << 32) | (v >> 32)) & M64]
    out.append(0)
    return np.array(out, dtype=np.uint64)
