"""Translate a synthetic scenario to a large log index and Term.

The engine keeps three width boundaries ("The 16-byte record"): a
batch record packs Index in 40 and Term in 24 bits (wider: REC_LONG, the pair
in the side table), a device event word carries 40 bits of x (wider: a second
EVC_CONT word), and the group arrays are addressed with 32-bit offsets while
their values are 64-bit.  lift() moves a whole scenario (group records, log
term runs, inflight windows) up by an index base B and a term base T, so the
scenarios of the suite run unchanged in shape at and across those boundaries.
Batches need no lifting: every generator in etcd_amd/synth.py reads the Term
and the last index from the groups it is given.

The oracle (raft_oracle.c) works on full uint64 values throughout, so a lifted
scenario stepped through it is the reference for the engine's wide paths.
"""
import numpy as np

from etcd_amd import abi

IDX_BITS, TERM_BITS = 40, 24  # a short record's Index and Term (MsgRec.ti); an event word's x


def lift(groups, runs, ins, index_base, term_base):
    """Copies of (groups, runs, ins) at index_base / term_base.

    committed, first_index, last_index += B; term += T (term_first / term_last
    travel with the log; the oracle derives them from the runs anyway); every
    run (start, term) -> (start + B, term + T); every inflight value += B; per
    slot < n: next += B, match and pending_snapshot += B only where non-zero (a
    follower at Match 0 stays there: the huge-lag case); slots >= n stay zero.
    For B > 0 a log that starts at B + 1 has its snapshot at B: snap_index =
    first_index - 1 (a leader whose follower falls below firstIndex sends it;
    with no snapshot the reference panics, HB_FAULT_EMPTY_SNAPSHOT)."""
    B, T = np.uint64(index_base), np.uint64(term_base)
    assert index_base < 1 << 62 and term_base < 1 << 62  # Pair.reserve sums in int64
    g = np.array(groups, dtype=abi.GROUP_DTYPE, copy=True)
    for f in ("committed", "first_index", "last_index"):
        g[f] += B
    g["term"] += T
    has_run = g["term_first"] != np.uint64(abi.HB_NO_INDEX)
    g["term_first"][has_run] += B
    g["term_last"][has_run] += B
    if index_base > 0:
        g["snap_index"] = g["first_index"] - np.uint64(1)
    pr = g["pr"]
    live = np.arange(pr.shape[1])[None, :] < g["n"][:, None]
    pr["next"][live] += B
    for f in ("match", "pending_snapshot"):
        nz = live & (pr[f] != 0)
        pr[f][nz] += B
    if runs is None:
        lruns = None
    elif isinstance(runs, tuple):  # flat [R, 2] (index, term) rows plus offsets
        flat = np.array(runs[0], dtype=np.uint64, copy=True)
        flat[:, 0] += B
        flat[:, 1] += T
        lruns = (flat, runs[1])
    else:
        lruns = [[(int(i) + index_base, int(t) + term_base) for i, t in rr] for rr in runs]
    lins = None if ins is None else {k: np.asarray(v, dtype=np.uint64) + B for k, v in ins.items()}
    return g, lruns, lins


# The named bases.  delta / eps are a scenario's own offsets, chosen so that its
# index and term spread straddles the boundary.
BASES = ("W32", "W40", "T40", "W62")


def base(name, delta=0, eps=0):
    """(B, T) of a named base:
    W32  B = 2^32 - delta             32-bit truncation with no format change
    W40  B = 2^40 - delta, T = 2^24 - eps   both record bounds and the event bound,
                                      short and long mixed, values crossing mid-run
    T40  T = 2^40 - eps               short index, long term: REC_LONG by term only;
                                      vote and term events with a continuation word
    W62  B = 2^61, T = 2^50           everything long, high continuation bits"""
    return {"W32": ((1 << 32) - delta, 0),
            "W40": ((1 << IDX_BITS) - delta, (1 << TERM_BITS) - eps),
            "T40": (0, (1 << 40) - eps),
            "W62": (1 << 61, 1 << 50)}[name]


def lifted(name, groups, runs, ins=None, delta=0, eps=0):
    """lift() to a named base; name None: the scenario as it is (the same objects)."""
    if name is None:
        return groups, runs, ins
    B, T = base(name, delta, eps)
    return lift(groups, runs, ins, B, T)


def long_records(batch):
    """Which messages of a batch make REC_LONG records: Index >= 2^40 or Term >= 2^24."""
    return (np.asarray(batch["index"], dtype=np.uint64) >> np.uint64(IDX_BITS) != 0) | \
           (np.asarray(batch["term"], dtype=np.uint64) >> np.uint64(TERM_BITS) != 0)
