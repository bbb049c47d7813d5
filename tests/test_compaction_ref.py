"""The compaction scenarios of tests/test_compaction_gpu.py on the oracle alone
(OracleCompactPair, no GPU): what each stream has to reach for its GPU run to
mean something.  These are conditions on the streams, not measurements: the
rings must stay at their minimum capacity while the logs advance several
capacities, every event kind must occur, and no group may run into the
engine's window preconditions."""
import functools

import numpy as np
import pytest

from etcd_amd import abi

from . import test_compaction_gpu as S
from .compact_util import OracleCompactPair

WINDOW = (abi.HB_FAULT_SIZE_WINDOW, abi.HB_FAULT_TERM_WINDOW)


@functools.lru_cache(maxsize=None)
def leader(n, size, lift=None):
    return S.run_leader_stream(n, size, make=OracleCompactPair, lift=lift)


@functools.lru_cache(maxsize=None)
def follow(n, size, lift=None):
    return S.run_follow_stream(n, size, make=OracleCompactPair, lift=lift)


def wrapped(pair, runs):
    """Scenarios 1, 2, 7: the rings stayed small and the logs went round them."""
    G = pair.G
    if pair.sized:
        assert (pair.appended >= 4 * pair.cap_sz).mean() >= 0.75
        assert np.median(pair.cap_sz) == abi.HB_SIZE_RING_MIN
    else:
        assert (pair.appended >= 4 * abi.HB_SIZE_RING_MIN).mean() >= 0.75
    if runs:
        assert (pair.runs_started >= 4 * pair.cap_tr).mean() >= 0.75
    assert np.median(pair.cap_tr) == abi.HB_TERM_RING_MIN
    assert pair.fault_count[:, list(WINDOW)].sum() == 0
    assert not np.isin(pair.og.groups()["fault"], WINDOW).any()
    return G


@pytest.mark.parametrize("n,size,lift", [(3, None, None), (3, 150, None), (5, 150, None), (7, 40, None), (3, 150, "W40")])
def test_leader_stream_reach(n, size, lift):
    pair = leader(n, size, lift)
    G = wrapped(pair, runs=False)
    now = pair.og.groups()
    assert (pair.ev_count[:, abi.HB_EV_SNAP] > 0).mean() >= 0.05
    assert (now["fault"][list(S.NOSNAP)] == abi.HB_FAULT_EMPTY_SNAPSHOT).all()
    other = np.ones(G, bool)
    other[list(S.NOSNAP)] = False
    assert (now["fault"][other] != 0).mean() <= 0.02
    if lift:  # indices either side of 2^40 at the end (the ring masks see both)
        below = (now["last_index"] >> np.uint64(40)) == 0
        assert 0.2 <= below.mean() <= 0.8


@pytest.mark.parametrize("n,size,lift", [(3, 150, None), (5, None, None), (3, 150, "W40")])
def test_follow_stream_reach(n, size, lift):
    pair = follow(n, size, lift)
    wrapped(pair, runs=True)
    now = pair.og.groups()
    assert (now["fault"] != 0).mean() <= 0.02
    assert pair.follow_count[:, abi.HB_FOLLOW_APPEND].sum() > 0 and pair.follow_count[:, abi.HB_FOLLOW_RESTORE].sum() > 0
    assert pair.resp_count[:, abi.HB_RESP_APP | abi.HB_RESP_REJECT].sum() > 0  # a rejected MsgApp
    assert pair.resp_count[:, abi.HB_RESP_VOTE].sum() > 0                      # a granted vote
    assert (pair.cycles >= 1).sum() >= 100  # follower -> candidate -> leader -> follower, all of it
    assert pair.ev_count[:, abi.HB_EV_SNAP].sum() > 0 and pair.ev_count[:, abi.HB_EV_APP].sum() > 0  # the leader stage served and sent snapshots
    if lift:
        below = (now["last_index"] >> np.uint64(40)) == 0
        assert 0.2 <= below.mean() <= 0.8


def test_wrapped_rings_moved_reach():
    pair, seen = S.run_wrapped_rings_moved(make=OracleCompactPair)
    # at the regrow and the move every group's rings had wrapped: the run ring's head is not 0
    assert (seen["runs_started"] > seen["cap_tr"]).all() and (seen["appended"] > seen["cap_sz"]).all()
    # and the ungrown groups went round twice more afterwards
    un = np.ones(pair.G, bool)
    un[1::3] = False
    un[list(S.RELOADED)] = False
    assert (pair.appended[un] - seen["appended"][un] >= 2 * abi.HB_SIZE_RING_MIN).mean() >= 0.75
    assert (pair.runs_started[un] - seen["runs_started"][un] >= 2 * abi.HB_TERM_RING_MIN).mean() >= 0.75
    assert pair.fault_count[:, list(WINDOW)].sum() == 0 and (pair.og.groups()["fault"] == 0).all()


@pytest.mark.parametrize("n", [3, 5])
def test_boundaries_on_the_oracle(n):
    S.check_boundaries(n, *S.run_boundaries(n, make=OracleCompactPair))


def test_steady_compaction_on_the_oracle():
    S.check_steady_compaction(*S.run_steady_compaction(make=OracleCompactPair))


def test_drop_rule_reach():
    """The sz_lo - 1 probes fault and the sz_lo probes do not, on the oracle."""
    pair, ev, now, szlo = S.run_drop_rule(make=OracleCompactPair)
    S.check_drop_rule(pair, ev, now, szlo)
    assert (pair.appended >= 3 * abi.HB_SIZE_RING_MIN).all()  # past the capacity, the MsgProp of 40 alone twice over
    assert (pair.fault_count[1::2, abi.HB_FAULT_SIZE_WINDOW] == 1).all() and pair.fault_count[0::2].sum() == 0
