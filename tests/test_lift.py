"""The wide-value suite's generator conditions, on the oracle alone (no GPU).

tests/test_wide_values_gpu.py runs the scenarios of tests/wide_cases.py lifted
to the bases of tests/lift_util.py.  A lifted scenario proves something only
if its values really sit where the engine changes format, and if lifting did
not push its groups into faults (a faulted group's record is not compared).
For every (case, base) the GPU file uses, the same body runs here through
OraclePair and must satisfy:

  - the share of faulted groups at the end is at most the unlifted
    scenario's + 0.02;
  - W40: in every batch both REC_LONG and short records are >= 0.10 of the
    batch, and over the run events with x >= 2^40 and with x < 2^40 both occur;
  - W62: every record with a non-zero Term or Index is long (a MsgProp's
    index field is its entry count, not an Index: those stay short).

Measured, W40 long share per batch / faulted share at the end (lifted equals
unlifted within 0.02 everywhere; `pytest -s` prints every row): fuzz 0.58-0.61
/ 0.25-0.29 (mostly HB_FAULT_LEADER_CAMPAIGN, a property of
synth.random_batch), follower fuzz 0.63-0.67 / 0.24-0.27, ticks 0.59-0.61 /
0.15-0.19, finite max size 0.58-0.61 / 0.28-0.30, deep lag 0.58-0.61 / 0,
cfg2 0.75-0.77 / 0, MsgProp lane 0.50-0.60 / 0.11, closed-loop cfg3 0.73-0.75
/ 0, storm 0.43-0.46 / 0, hand-over classes 0.48-0.49 / 0, tick elections
0.52 / 0, commit_zero hand-over 0.63-0.76 / 0.
"""
import functools

import numpy as np
import pytest

from etcd_amd import abi, synth

from . import wide_cases
from .lift_util import BASES, base, lift, lifted, long_records
from .parity_util import OraclePair


def _run(case, b, monkeypatch):
    pairs = []

    def make(*a, **kw):
        pairs.append(OraclePair(*a, **kw))
        return pairs[-1]
    wide_cases.run(case, b, make, storm=None, monkeypatch=monkeypatch)
    return pairs


@functools.lru_cache(maxsize=None)
def _unlifted_faulted(case):
    mp = pytest.MonkeyPatch()
    try:
        return [p.faulted_share() for p in _run(case, None, mp)]
    finally:
        mp.undo()


@pytest.mark.parametrize("case,b", wide_cases.PLAIN + wide_cases.STORM)
def test_lifted_scenario_conditions(case, b, monkeypatch):
    pairs = _run(case, b, monkeypatch)
    plain = _unlifted_faulted(case)
    assert len(pairs) == len(plain)
    shares = [s for p in pairs for s in p.long_share]
    print(f"\n{case}/{b}: long share per batch {min(shares, default=0):.2f}-{max(shares, default=0):.2f}, "
          f"faulted {[round(p.faulted_share(), 3) for p in pairs]} (unlifted {[round(x, 3) for x in plain]}), "
          f"events wide/narrow {sum(p.ev_wide for p in pairs)}/{sum(p.ev_narrow for p in pairs)}")
    for p, f0 in zip(pairs, plain):
        assert p.faulted_share() <= f0 + 0.02
    if b == "W40":
        assert shares and min(shares) >= 0.10 and max(shares) <= 0.90, shares
        assert sum(p.ev_wide for p in pairs) > 0 and sum(p.ev_narrow for p in pairs) > 0
    if b == "W62":
        assert all(all(p.all_long) for p in pairs)


def test_lift_rules():
    """lift() itself, on a fuzzed state: every rule of its docstring, and the
    oracle's canonical record of the lifted state is the lifted canonical record."""
    from oracle.pyoracle import OracleGroups
    g, runs, ins = synth.random_groups(400, 5, seed=3, W=8)
    B, T = base("W40", 24, 20)
    lg, lruns, lins = lift(g, runs, ins, B, T)
    assert np.array_equal(lg["last_index"], g["last_index"] + np.uint64(B))
    assert np.array_equal(lg["term"], g["term"] + np.uint64(T))
    assert np.array_equal(lg["snap_index"], lg["first_index"] - np.uint64(1))
    for s in range(abi.HB_MAX_REPLICAS):
        live = s < g["n"]
        m, lm = g["pr"][:, s]["match"], lg["pr"][:, s]["match"]
        assert np.array_equal(lm, np.where(live & (m != 0), m + np.uint64(B), 0))
        assert np.array_equal(lg["pr"][:, s]["next"], np.where(live, g["pr"][:, s]["next"] + np.uint64(B), 0))
    assert all(np.array_equal(lins[k], ins[k] + np.uint64(B)) for k in ins)
    assert lruns[7] == [(i + B, t + T) for i, t in runs[7]]
    assert g["term"].max() < 40  # the input is a copy's source, unchanged
    a = OracleGroups(g, runs, 8, inflights=ins).groups()
    b = OracleGroups(lg, lruns, 8, inflights=lins).groups()
    has = a["term_first"] != np.uint64(abi.HB_NO_INDEX)
    assert np.array_equal(b["term_first"][has], a["term_first"][has] + np.uint64(B))
    assert np.array_equal(b["term_last"][has], a["term_last"][has] + np.uint64(B))
    assert np.array_equal(b["term_first"][~has], a["term_first"][~has])
    assert lifted(None, g, runs, ins)[0] is g
    assert [base(n)[0] < 1 << 62 and base(n)[1] < 1 << 62 for n in BASES] == [True] * 4


def test_long_records_bounds():
    b = dict(index=np.array([0, (1 << 40) - 1, 1 << 40, 5, 5], np.uint64),
             term=np.array([0, (1 << 24) - 1, 0, 1 << 24, (1 << 24) - 1], np.uint64))
    assert long_records(b).tolist() == [False, False, True, True, False]


@pytest.mark.parametrize("b", wide_cases.WIDE)
def test_decode_then_step_batches(b):
    """test_wire_gpu.run_decode_then_step_cfg2 decodes on the device, so it cannot
    run here; its batches (the same groups, offsets and seeds) hold both record
    formats under W40 and only long records under W62."""
    g, runs = synth.steady_groups(4000, 3, seed=5)
    g, runs, _ = lifted(b, g, runs, delta=1 << 19, eps=500)
    for step in range(3):
        share = long_records(synth.cfg2_batch(g, step, seed=50 + step)).mean()
        assert 0.10 <= share <= 0.90 if b == "W40" else share == 1.0, share
