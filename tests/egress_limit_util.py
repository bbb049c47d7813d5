"""The replay rules of wire egress in append mode with limitSize's cut,
restated in Python.

replay_apps_limit() is egress_app_util.replay_apps on a handle with a finite max_msg_size
and hb_set_egress_limit on: a MsgApp with entries (x, last] that replay_apps would flag
for the limit alone is an HB_OUT_ENTS record with hint = L, limitSize's cut of that range
(oracle orc_limit_size over Entry.Size() of the entries), unless

  (i)   x < szlo_final[g]: the group's size ring, as it stands when hb_egress runs, no
        longer holds the cumulative size at x;
  (ii)  the group has an HB_EV_FOLLOW event with aux APPEND or RESTORE anywhere in the
        call's events, before or after the send.

Every other reason to flag a record, and every other column, is replay_apps'.  With every
record that has entries forced to HB_OUT_HOST the result is replay_apps(...,
max_msg_size=finite); the function asserts that.

size_table() gives size_of(g, i) = Entry.Size() of entry i: the loaded sizes for the
entries the log held before the call, orc_entry_size(desc, term, index) for those a leader
appended in it.  tests/test_egress_limit_replay.py pins the rules to the oracle's own
r.msgs; tests/test_egress_limit_gpu.py uses them as the device's reference.
"""
import numpy as np

from etcd_amd import abi
from oracle import pyoracle

from .egress_app_util import is_app, replay_apps


def sized(max_msg_size):
    return max_msg_size not in (0, abi.HB_NO_LIMIT)


def limit_cut(sizes, max_msg_size):
    """limitSize (raft/util.go:97-110) over the sizes of entries x + 1 ..: how many go."""
    a = np.ascontiguousarray(sizes, dtype=np.uint64)
    return int(pyoracle.lib().orc_limit_size(a.ctypes.data_as(pyoracle.C.POINTER(pyoracle.C.c_uint64)), len(a),
                                             max_msg_size))


def follower_rewrites(events):
    """The groups of rule (ii)."""
    f = events[(events["type"] == abi.HB_EV_FOLLOW) &
               ((events["aux"] == abi.HB_FOLLOW_APPEND) | (events["aux"] == abi.HB_FOLLOW_RESTORE))]
    return set(int(g) for g in f["group"])


def szlo_final(szlo0, last_final, size_cap):
    """The oldest index the size ring keeps after a call in which only a leader appended (sz_keep
    in hipbatch_kernels.h): a ring of capacity `size_cap` (hb_log_capacity) that holds
    cum(last_final) holds nothing below last_final - (size_cap - 1)."""
    lo, last, cap = int(szlo0), int(last_final), int(size_cap)
    return max(lo, last - (cap - 1)) if last >= cap else lo


def replay_apps_limit(events, groups0, runs, peers, self_id, max_msg_size, size_of, szlo_final, votes=True):
    """events, groups0, runs, peers, self_id, votes as replay_apps; max_msg_size finite and
    non-zero; size_of(g, i) = Entry.Size() of entry i of group g; szlo_final[g] = the ring's
    oldest index when hb_egress runs.  Returns tuples of egress_app_util.APP_FIELDS."""
    assert sized(max_msg_size)
    # without a limit the replay names the whole range (x, last]: hint = last at the send
    whole = replay_apps(events, groups0, runs, peers, self_id, max_msg_size=abi.HB_NO_LIMIT, votes=votes)
    rewritten = follower_rewrites(events)
    out, forced = [], []
    for r in whole:
        g, x, last, host, ents = r[0], r[7], r[10], r[11], r[12]
        flagged = r[:6] + (0, x, 0, False, 0, True, False)
        if not (is_app(r) and ents):
            out.append(r)
            forced.append(r)
            continue
        assert not host and x < last
        forced.append(flagged)
        if g in rewritten or x < int(szlo_final[g]):
            out.append(flagged)
            continue
        k = limit_cut([size_of(g, i) for i in range(x + 1, last + 1)], max_msg_size)
        assert 1 <= k <= last - x
        out.append(r[:10] + (x + k,) + r[11:])
    assert forced == replay_apps(events, groups0, runs, peers, self_id, max_msg_size=max_msg_size, votes=votes)
    return out


def size_table(events, groups0, loaded, batch=None):
    """size_of(g, i) for replay_apps_limit.  loaded = {g: Entry.Size() of the group's last
    len entries before the call} (hb_load_entry_sizes); a leader's appends of the call are
    read off its HB_EV_LAST events (aux = 1: becomeLeader's empty entry) and take their
    descriptors from the batch in order: the dense proposal (props / peoff) first, then
    every MsgProp message (index entries at eoff); a batch without edesc describes every
    entry as pb.Entry{} with the Term and Index only.  A group of rule (ii) has no sizes
    after its follower append."""
    z = {}
    for g, s in loaded.items():
        last = int(groups0[g]["last_index"])
        for k, v in enumerate(s):
            z[(g, last - len(s) + 1 + k)] = int(v)
    src = {}
    edesc = None if batch is None else batch.get("edesc")
    if batch is not None:
        if batch.get("props") is not None:
            for g, k in enumerate(np.asarray(batch["props"]).tolist()):
                if k:
                    e0 = int(batch["peoff"][g]) if edesc is not None else 0
                    src.setdefault(g, []).append((k, e0))
        t = np.asarray(batch["info"]) & 0xF
        for i in np.nonzero(t == abi.HB_MSG_PROP)[0].tolist():
            k = int(batch["index"][i])
            if k:
                src.setdefault(int(batch["group"][i]), []).append((k, int(batch["eoff"][i]) if edesc is not None else 0))
    esz = pyoracle.lib().orc_entry_size
    state, dead = {}, follower_rewrites(events)
    for e in events:
        g = int(e["group"])
        if g in dead:
            continue
        s = state.setdefault(g, [int(groups0[g]["term"]), int(groups0[g]["last_index"])])
        t, x = int(e["type"]), int(e["x"])
        if t == abi.HB_EV_TERM:
            s[0] = x
        elif t == abi.HB_EV_FAULT:
            dead.add(g)
        elif t == abi.HB_EV_LAST:
            k = x - s[1]
            descs = [0] * k
            if not int(e["aux"]) & 1:
                q = src.get(g, [])
                while q and q[0][0] != k:
                    assert edesc is None, "a dropped proposal among described ones"
                    q.pop(0)
                assert q, f"group {g}: an append of {k} entries without a proposal"
                _, e0 = q.pop(0)
                if edesc is not None:
                    descs = [int(d) for d in edesc[e0:e0 + k]]
            for j in range(k):
                z[(g, s[1] + 1 + j)] = int(esz(descs[j], s[0], s[1] + 1 + j))
            s[1] = x

    def size_of(g, i):
        return z[(g, i)]
    return size_of


def with_descs(batch):
    """A hand-built scenario batch (egress_cases.export: MsgApp entry terms at eoff) for a handle
    with a finite max_msg_size: MsgApp and MsgProp entries share one entry array (a MsgProp's
    index[i] entries follow eoff[i] too), every descriptor pb.Entry{}'s (no Data, EntryNormal)."""
    t = np.asarray(batch["info"]) & 0xF
    bounds = np.append(np.asarray(batch["eoff"], dtype=np.int64), len(batch["eterm"]))
    eoff, eterm = [], []
    for i in range(len(t)):
        eoff.append(len(eterm))
        eterm.extend(batch["eterm"][bounds[i]:bounds[i + 1]].tolist())
        if t[i] == abi.HB_MSG_PROP:
            eterm.extend([0] * int(batch["index"][i]))
    return dict(batch, eoff=np.array(eoff, np.uint64), eterm=np.array(eterm, np.uint64).reshape(-1),
                edesc=np.zeros(len(eterm), np.uint32))
