"""The replay rules of wire egress in append mode with the LogTerm lookup,
restated in Python.

replay_apps_logterm() is egress_app_util.replay_apps (or, with `limit`, egress_limit_util.
replay_apps_limit) on a handle with hb_set_egress_logterm on: a MsgApp record that those flag
only for its LogTerm (an aux = 0 send that is not at the known boundary) carries log_term =
the term of its Index x, unless

  (i)   the group's older-runs ring, as it stands when hb_egress runs, holds no run starting
        at or below x (oldest_final[g] is None or > x);
  (ii)  the group has an HB_EV_FOLLOW event with aux APPEND or RESTORE anywhere in the call's
        events, before or after the send.

Every other reason to flag the record (Commit unknown, the limit), and every other column,
is the base replay's.  With every looked-up record forced back to HB_OUT_HOST the result is
the base replay's; the function asserts that.

ring_oldest() is the small model of the ring that rule (i) needs: capacity run_cap
(hb_log_capacity), the runs the ring held before the call, one push per Term change whose
current-term run was non-empty (Lane::reset -> tr_push), drop-oldest when full.  It follows a
group up to its first follower append / restore, where rule (ii) takes over.
tests/test_egress_logterm_replay.py pins the rules to the oracle's own r.msgs;
tests/test_egress_logterm_gpu.py uses them as the device's reference.
"""
import numpy as np

from etcd_amd import abi

from .egress_app_util import boundary, is_app, replay_apps
from .egress_limit_util import follower_rewrites, replay_apps_limit
from .egress_vote_util import UNKNOWN, last_term


def ring_oldest(events, groups0, runs, run_cap):
    """{group: the start of the oldest run the ring holds when hb_egress runs, None: no run}.
    runs[g] = the ring's runs before the call [(start, term)], oldest first; run_cap[g] (or one
    int) its capacity."""
    out = {}
    state = {}
    for g in range(len(groups0)):
        rr = runs.get(g) if isinstance(runs, dict) else runs[g]
        tf = int(groups0[g]["term_first"])
        cap = int(run_cap if isinstance(run_cap, int) else run_cap[g])
        ring = [(int(s), int(t)) for s, t in (rr or ())]
        assert len(ring) <= cap
        state[g] = dict(ring=ring, cap=cap, term=int(groups0[g]["term"]), last=int(groups0[g]["last_index"]),
                        tf=None if tf == abi.HB_NO_INDEX else tf, stop=False)
    for e in events:
        s = state[int(e["group"])]
        if s["stop"]:
            continue
        t, aux, x = int(e["type"]), int(e["aux"]), int(e["x"])
        if t == abi.HB_EV_TERM:
            if s["tf"] is not None:  # Runs::push
                ring = s["ring"]
                if not (ring and ring[-1][1] == s["term"]):
                    if len(ring) == s["cap"]:
                        ring.pop(0)
                    ring.append((s["tf"], s["term"]))
            s["term"], s["tf"] = x, None
        elif t == abi.HB_EV_LAST:  # appendEntry: the group's own entries carry its Term
            if s["tf"] is None:
                s["tf"] = s["last"] + 1
            s["last"] = x
        elif t == abi.HB_EV_FAULT or (t == abi.HB_EV_FOLLOW and aux in (abi.HB_FOLLOW_APPEND, abi.HB_FOLLOW_RESTORE)):
            s["stop"] = True
    for g, s in state.items():
        out[g] = s["ring"][0][0] if s["ring"] else None
    return out


def lookup_sends(events, groups0, runs):
    """Per HB_EV_APP event, in event order: whether the send is one the lookup is for (aux = 0 and
    not at the known boundary), by the boundary rules of egress_app_util.replay_apps."""
    state, out = {}, []
    for x, g, t, _, aux in np.asarray(events).tolist():  # (abi.EVENT_DTYPE's field order)
        s = state.get(g)
        if s is None:
            rr = runs.get(g) if isinstance(runs, dict) else runs[g]
            bl, blt = boundary(groups0[g], rr)
            s = state[g] = dict(last=int(groups0[g]["last_index"]), pend=False, dead=False, term=int(groups0[g]["term"]),
                                lt=last_term(groups0[g], rr), bl=bl, blt=blt)
        if s["dead"]:
            continue
        if t == abi.HB_EV_TERM:
            s["term"] = x
            s["bl"], s["blt"] = (UNKNOWN if s["pend"] else s["last"]), s["lt"]
        elif t == abi.HB_EV_LAST:
            s["last"], s["lt"] = x, s["term"]
        elif t == abi.HB_EV_FOLLOW:
            if aux in (abi.HB_FOLLOW_APPEND, abi.HB_FOLLOW_RESTORE):
                s["pend"] = True
                s["lt"] = s["bl"] = s["blt"] = UNKNOWN
        elif t == abi.HB_EV_FAULT:
            s["dead"] = True
        elif t == abi.HB_EV_APP:
            at_bl = s["bl"] is not UNKNOWN and x == s["bl"] and s["blt"] is not UNKNOWN
            out.append(not (aux & 1) and not at_bl)
        elif t == abi.HB_EV_RESP and (aux & 7) == abi.HB_RESP_APP and not aux & abi.HB_RESP_REJECT and s["pend"]:
            s["last"], s["pend"] = x, False
    return out


def replay_apps_logterm(events, groups0, runs, peers, self_id, term_of, oldest_final,
                        max_msg_size=abi.HB_NO_LIMIT, limit=None, votes=True):
    """events, groups0, runs, peers, self_id, votes as replay_apps; term_of(g, i) = the term of
    entry i of group g's log; oldest_final = ring_oldest(...).  limit = None: the limit knob is
    off (replay_apps under max_msg_size); limit = (size_of, szlo_final): it is on
    (replay_apps_limit).  Returns tuples of egress_app_util.APP_FIELDS."""
    def base(ev):
        if limit is None:
            return replay_apps(ev, groups0, runs, peers, self_id, max_msg_size=max_msg_size, votes=votes)
        return replay_apps_limit(ev, groups0, runs, peers, self_id, max_msg_size, limit[0], limit[1], votes=votes)

    parent = base(events)
    looked = lookup_sends(events, groups0, runs)
    # the same events with every such send marked as its LogTerm known: what else flags the
    # record, and every other column, come out of the base replay itself
    marked = events.copy()
    k = 0
    for i in range(len(marked)):
        if int(marked[i]["type"]) == abi.HB_EV_APP:
            if k < len(looked) and looked[k]:
                marked[i]["aux"] = int(marked[i]["aux"]) | 1
            k += 1
    lifted = base(marked)
    assert len(lifted) == len(parent) and sum(is_app(r) for r in parent) == len(looked)
    rewritten = follower_rewrites(events)
    out, forced = [], []
    k = 0
    for r, p in zip(lifted, parent):
        if not is_app(r):
            assert r == p
            out.append(r)
            forced.append(r)
            continue
        mine = looked[k]
        k += 1
        if not mine:
            assert r == p
            out.append(r)
            forced.append(r)
            continue
        g, x = r[0], r[7]
        assert p[11] and (p[6], p[8], p[10], p[12]) == (0, 0, 0, False)  # the parent flags it whatever else holds
        forced.append(p)
        lo = oldest_final[g]
        if r[11] or g in rewritten or lo is None or x < int(lo):
            out.append(p)
            continue
        out.append(r[:6] + (int(term_of(g, x)),) + r[7:])
    assert forced == parent
    return out
