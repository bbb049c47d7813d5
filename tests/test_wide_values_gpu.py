"""GPU parity at wide values: the scenarios of test_parity_gpu.py lifted to the
engine's width boundaries (tests/lift_util.py: 2^32, 2^40 / 2^24, 2^61 / 2^50).

Every case steps the same body as its unlifted test through Pair: events,
compact words, statistics, every group record, inflight windows and timers
bit-exact against the oracle.  What that reaches that the unlifted suite does
not: REC_LONG records (the side table through rec_unpack) on every lane and in
the LDS route slots and the storm hand-over, batches mixing both record
formats, EVC_CONT continuation words on every event type, sz_limit and the
size / term-run rings at large indices, and 32-bit truncation of 64-bit
values (W32: no format change at all).  tests/test_lift.py proves on the
oracle alone that each (case, base) really holds both formats.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth

from . import wide_cases
from .lift_util import lift, long_records
from .parity_util import Pair
from .test_parity_gpu import DRAWS
from .test_wire_gpu import run_decode_then_step_cfg2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,base", wide_cases.PLAIN)
def test_wide(case, base):
    wide_cases.run(case, base, Pair)


@pytest.mark.parametrize("storm", [None, "0"])
@pytest.mark.parametrize("case,base", wide_cases.STORM)
def test_wide_storm(case, base, storm, monkeypatch):
    wide_cases.run(case, base, Pair, storm=storm, monkeypatch=monkeypatch)


@pytest.mark.parametrize("base", wide_cases.WIDE)
def test_wide_decode_then_step_cfg2(base):
    """Device-resident decoded arrays (9- and 10-byte varints off the wire) into hb_step."""
    run_decode_then_step_cfg2(lift=base)


@pytest.mark.parametrize("n", [3, 5])
def test_commit_and_term_cross_the_record_bounds(n):
    """Values that pass a boundary between two steps of one handle.  cfg2
    steady: every group's last index is 2^40 - 2 and its Term 2^24 - 1 (the
    largest short Term), so step 0 acks and commits 2^40 - 1 in short records
    and one-word events and steps 1-3 take REC_LONG records and a continuation
    word for the same groups.  Then an election by ticks from Term 2^24 - 1:
    the campaign takes every group to 2^24, the votes that answer it are long
    records by Term alone."""
    G = 2000
    g, runs = synth.steady_groups(G, n, seed=7, last_hi=1, term_hi=1)
    g, runs, _ = lift(g, runs, None, (1 << 40) - 3, (1 << 24) - 2)
    assert (g["last_index"] == (1 << 40) - 2).all() and (g["term"] == (1 << 24) - 1).all()
    pair = Pair(g, runs, n, 256, max_batch=G * n + 16)
    short = wide = 0
    for step in range(4):
        b = synth.cfg2_batch(g, step, seed=70 + step)
        assert long_records(b).all() == long_records(b).any() == (step >= 1)
        ev, st, now = pair.step(b, ctx=f"crossing n={n} step {step}")  # (ev equals the oracle's stream)
        assert st[abi.HB_STAT_COMMITS] == G
        x = ev["x"][ev["type"] == abi.HB_EV_COMMIT]
        assert (x == (1 << 40) - 1 + step).all()
        short += int((x >> np.uint64(40) == 0).sum())
        wide += int((x >> np.uint64(40) != 0).sum())
    assert short == G and wide == 3 * G  # both one-word and two-word HB_EV_COMMIT occurred

    e, eruns = synth.election_groups(G, n, seed=8, term_hi=1)
    e, eruns, _ = lift(e, eruns, None, (1 << 40) - (1 << 15), (1 << 24) - 2)
    assert (e["term"] == (1 << 24) - 1).all()
    pair = Pair(e, eruns, n, 64, max_batch=1 << 16)
    t = np.zeros(G, abi.TIMER_DTYPE)
    t["election_tick"], t["heartbeat_tick"] = 4, 2
    pair.set_timers(t, DRAWS)
    terms = []
    for k in range(10):
        ev, _, now = pair.tick(ctx=f"crossing n={n} tick {k}")
        terms.append(ev["x"][ev["type"] == abi.HB_EV_TERM])
    terms = np.concatenate(terms)
    assert (terms == 1 << 24).sum() == G and (now["term"] >= 1 << 24).all()
    cand = np.nonzero(now["state"] == abi.HB_STATE_CANDIDATE)[0].astype(np.uint32)
    assert len(cand) > G // 2
    vg = np.repeat(cand, n - 1)
    vs = np.tile(np.arange(1, n, dtype=np.uint32), len(cand))
    b = dict(group=vg, info=(abi.HB_MSG_VOTE_RESP | (vs << 4)).astype(np.uint32),
             term=now["term"][vg].astype(np.uint64), index=np.zeros(len(vg), np.uint64), hint=None, props=None)
    assert long_records(b).all()
    _, st, _ = pair.step(b, ctx=f"crossing n={n} votes")
    assert st[abi.HB_STAT_WON] == len(cand)
