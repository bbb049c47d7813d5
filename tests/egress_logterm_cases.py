"""Hand-built leader scenarios of wire egress with the LogTerm lookup, on top
of tests/egress_app_cases.py: that set unchanged, with the flagged counts the knob leaves, and
the cases that are about a resend below the boundary.

T = the group's Term before the batch, as in egress_app_cases; a leader has won at T + 1.
Every case states how many of its MsgApp records stay HB_OUT_HOST with the knob on
("flagged"); FLAGGED names the reasons.  A case with "unloaded" = k has its k oldest term
runs left out of hb_load_term_runs.

  walk-down             the log (1,1) (2,2) (3,3) (4,T), noop at 5: a Probe follower rejects 4,
                        3 and 2 in one batch (hints 3, 2, 1); the resends at 3, 2 and 1 carry
                        the terms 3, 2 and 1, each from its own run
  at-snapshot           a compacted log (snapshot (2,1), entries (3,T-1) (4,T)): the resend at
                        2 = firstIndex - 1 carries the snapshot's term
  at-snapshot-unloaded  the same with the run (2,1) never loaded: rule (i)
  send-then-truncate    a resend at 2, then a step-down and a truncating MsgApp: rule (ii)
  send-then-heartbeat   a resend at 2, then a step-down on a higher-term MsgHeartbeat: the
                        ring only gains a run, the LogTerm is the ring's

ring_drop_cases(): rule (i) by a drop, on run rings of HB_TERM_RING_MIN = 8 that nobody
reserves.  The log is snapshot (2,1), (3,2) (4,3) (5,4) (6,5) (7,6) (8,T), noop at 9: seven
older runs.  The batch is a rejection (resend at x), a step-down (push: 8 runs, full), MsgHup
and the grants (leader at T + 4, noop at 10), a second step-down (push: the run (2,1) leaves).
"drop-early" resends at 2, in the run that left: flagged.  "drop-sibling" resends at 3, one
run higher: LogTerm 2.

limit_cases(): "probe-behind" of egress_limit_cases with the Probe follower's Next moved to 3:
its MsgHeartbeatResp sends (2, L], below the boundary and cut by the limit.
"""
from etcd_amd import abi

from . import egress_app_cases as AC
from . import egress_limit_cases as LC
from .egress_app_cases import _case, _rej
from .egress_cases import _m

A = abi
SIZES = AC.SIZES
RUN_CAP = abi.HB_TERM_RING_MIN
FLAGGED = {
    "append-then-win": AC.FLAGGED["append-then-win"],
    "at-snapshot-unloaded": "rule (i): the run that holds the Index was never loaded",
    "send-then-truncate": "rule (ii): a follower append after the send may have cut the ring",
}
WIDE = ("W32", "W40", "W62")


def scenarios(sizes=SIZES):
    out = []
    for c in AC.scenarios(sizes):
        if c["name"].startswith("reject-below-boundary"):
            c = dict(c, flagged=0)
        out.append(dict(c, unloaded=0))
    for n in sizes:
        T = 4 + n
        cur = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        hard = (T, 0, 2)

        def add(name, ents, msgs, unloaded=0, **kw):
            out.append(dict(_case(name, n, "leader", ents, hard, msgs, **kw), unloaded=unloaded))
        add("walk-down", [(1, 1), (2, 2), (3, 3), (4, T)],
            [_rej(2, T + 1, 4, 3), _rej(2, T + 1, 3, 2), _rej(2, T + 1, 2, 1)])
        add("at-snapshot", [(3, T - 1), (4, T)], [_rej(2, T + 1, 4, 2)], snapshot=(2, 1))
        add("at-snapshot-unloaded", [(3, T - 1), (4, T)], [_rej(2, T + 1, 4, 2)], snapshot=(2, 1), unloaded=1, flagged=1)
        add("send-then-truncate", cur, [_rej(2, T + 1, 4, 2), _m(A.HB_MSG_APP, 3, T + 3, 4, T, 3, ents=[T + 3])],
            flagged=1)
        add("send-then-heartbeat", cur, [_rej(2, T + 1, 4, 2), _m(A.HB_MSG_HEARTBEAT, 3, T + 3, commit=2)])
    return out


def below_cases(sizes=SIZES):
    """The cases without a snapshot whose records the knob lifts, for the wide bases."""
    return [c for c in scenarios(sizes) if c["name"].split("/")[0] in ("reject-below-boundary", "walk-down")]


def ring_drop_cases(sizes=SIZES):
    out = []
    for n in sizes:
        T = 4 + n
        ents = [(3, 2), (4, 3), (5, 4), (6, 5), (7, 6), (8, T)]
        fol = list(range(2, n + 1))
        grants = [_m(A.HB_MSG_VOTE_RESP, f, T + 4) for f in fol[:n // 2]]
        for name, hint, flagged in (("drop-early", 2, 1), ("drop-sibling", 3, 0)):
            msgs = ([_rej(2, T + 1, 8, hint), _m(A.HB_MSG_HEARTBEAT, 3, T + 3, commit=2), _m(A.HB_MSG_HUP, 1)] + grants +
                    [_m(A.HB_MSG_HEARTBEAT, 3, T + 6, commit=2)])
            out.append(dict(_case(name, n, "leader", ents, (T, 0, 2), msgs, snapshot=(2, 1), flagged=flagged),
                            unloaded=0, x=hint))
    return out


def limit_cases(sizes=SIZES):
    """flagged: with both knobs on; each knob alone leaves the one record to the host."""
    out = []
    for n in sizes:
        T = 4 + n
        cur = [(1, 1), (2, 1), (3, T - 1), (4, T)]
        out.append(dict(_case("probe-below", n, "leader", cur, (T, 0, 2), [_m(A.HB_MSG_HEARTBEAT_RESP, 2, T + 1)],
                              setup=[("step", _m(A.HB_MSG_PROP, 1, nents=LC.BEHIND)), ("progress", 2, 0, 3)]),
                        unloaded=0, flagged_one_knob=1))
    return out


def loaded_runs(groups, runs, cases):
    """{g: the older runs hb_load_term_runs gives group g}: synth.older_runs without the case's
    `unloaded` oldest ones."""
    from etcd_amd import synth
    older = synth.older_runs(groups, runs)
    return {g: list(older[g])[cases[g].get("unloaded", 0):] for g in range(len(cases))}
