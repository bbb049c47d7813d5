"""The n = 3 fast lane's wave-uniform steady path (SteadyLane):
parity against the oracle with the path taken, not taken and mixed, and the
count of group-waves that took it (HB_FAST_STEADY_COUNT=1 at create).

G = 4096 + 17 at n = 3, W = 8: two buckets, three k_route_fast workgroups of
2048 groups (eight partitions of 256, four waves each), a ragged last wave
and partition."""
import numpy as np
import pytest

from etcd_amd import abi, synth
from tests.parity_util import Pair, sort_events

pytestmark = pytest.mark.gpu

G, N, W = 4096 + 17, 3, 8
WAVES = (G + 63) // 64  # group-waves that hold a valid group (the last one: 17 groups and padding)
# the changed groups: lane 0 of a workgroup's first partition, lane 63 of its
# last partition, a middle lane of the next workgroup's first partition, and
# a lane of the ragged wave -- four different waves
ODD = (0, 2047, 2048 + 64 + 31, 4096 + 5)


def _state():
    return synth.steady_groups(G, N, seed=701, last_hi=1 << 16)


def _pair(monkeypatch, g, runs, ins=None, **kw):
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    return Pair(g, runs, N, W, ins=ins, max_batch=4 * G, **kw)


def test_all_steady(monkeypatch):
    g, runs = _state()
    pair = _pair(monkeypatch, g, runs)
    for step in range(3):
        _, st, _ = pair.step(synth.cfg2_batch(g, step, seed=702), ctx=f"all steady {step}")
        assert st[abi.HB_STAT_COMMITS] == G and st[abi.HB_STAT_APPRESP] == 2 * G
        assert bool(pair.eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        assert pair.eng.steady_waves() == WAVES


# ---- one odd lane per wave: each case changes group i of (g, b, ins) and
# returns whether its wave stays on the steady path
def _msgs(b, i):
    return np.nonzero(b["group"] == i)[0]


def _append(b, i, info, term, index):
    for k, v in (("group", i), ("info", info), ("term", term), ("index", index), ("hint", 0)):
        b[k] = np.append(b[k], np.array([v], dtype=b[k].dtype))


def _window(g, ins, i, s, match, sent):
    """Follower s of group i: Match, and a window holding `sent` (Next = last sent + 1)."""
    p = g["pr"][i][s]
    p["match"], p["next"], p["ins_start"], p["ins_count"] = match, sent[-1] + 1, 3, len(sent)
    ins[(i, s)] = np.array(sent, dtype=np.uint64)


def c_follower_state(g, runs, b, ins, i):
    g["state"][i], g["lead"][i] = abi.HB_STATE_FOLLOWER, 1
    return False


def c_probe_follower(g, runs, b, ins, i):
    g["pr"][i][1]["state"] = abi.HB_PR_PROBE
    return False


def c_rejected_ack(g, runs, b, ins, i):
    b["info"][_msgs(b, i)[0]] |= 1 << 8
    return False


def c_stale_ack(g, runs, b, ins, i):
    b["index"][_msgs(b, i)[0]] = g["last_index"][i]  # = Match
    return False


def c_same_follower(g, runs, b, ins, i):
    m = _msgs(b, i)
    b["info"][m] = abi.HB_MSG_APP_RESP | (1 << 4)
    return False


def c_third_message(g, runs, b, ins, i):
    _append(b, i, abi.HB_MSG_APP_RESP | (1 << 4), g["term"][i], g["last_index"][i] + 1)
    return False


def c_wrong_term(g, runs, b, ins, i):
    b["term"][_msgs(b, i)[1]] += 1
    return False


def c_from_not_member(g, runs, b, ins, i):
    b["info"][_msgs(b, i)[0]] = abi.HB_MSG_APP_RESP | (3 << 4)
    return False


def c_faulted(g, runs, b, ins, i):
    g["fault"][i] = abi.HB_FAULT_EMPTY_PROP
    return True  # (not live: nothing is stepped)


def c_commit_zero(g, runs, b, ins, i):
    g["commit_zero"][i] = 1
    return False


def _self_slot(s):
    def case(g, runs, b, ins, i):
        pr = g["pr"][i]
        pr[0]["state"], pr[s]["state"] = abi.HB_PR_REPLICATE, abi.HB_PR_PROBE
        g["self_slot"][i] = g["lead"][i] = g["vote"][i] = s
        m = _msgs(b, i)
        b["info"][m] = np.where((b["info"][m] >> 4) & 0xF == s, abi.HB_MSG_APP_RESP, b["info"][m])
        return True
    case.__name__ = f"c_self_slot_{s}"
    return case


def _small_n(n):
    def case(g, runs, b, ins, i):
        g["n"][i] = n
        g["pr"][i][n:] = 0
        return False
    case.__name__ = f"c_n_{n}"
    return case


def c_removed(g, runs, b, ins, i):
    return True  # (removed after the load, see _run_case: n = 0, nothing is stepped)


def c_last_index_2_40(g, runs, b, ins, i):
    last, term = (1 << 40) + 11, int(g["term"][i])
    g["last_index"][i] = g["committed"][i] = g["term_last"][i] = last
    g["term_first"][i] = last - 5
    g["pr"][i]["match"][:N] = last
    g["pr"][i]["next"][:N] = last + 1
    runs[i] = synth._runs_for(1, last - 5, last, term)
    b["index"][_msgs(b, i)] = last + 1
    return False


def c_lagging_ack(g, runs, b, ins, i):
    last = int(g["last_index"][i])
    _window(g, ins, i, 1, last - 3, [last - 1, last])
    m = [k for k in _msgs(b, i) if (b["info"][k] >> 4) & 0xF == 1][0]
    b["index"][m] = last - 1  # > Match, < Next - 1: the window's head stays
    return False


def c_full_window(g, runs, b, ins, i):
    last = int(g["last_index"][i])
    _window(g, ins, i, 1, last - W, list(range(last - W + 1, last + 1)))
    return False


def c_no_proposal(g, runs, b, ins, i):
    last = int(g["last_index"][i])
    g["committed"][i] = last - 1
    for s in (1, 2):
        _window(g, ins, i, s, last - 1, [last])
    b["props"][i] = 0
    b["index"][_msgs(b, i)] = last
    return True  # (both acks advance Match to last and empty the windows: steady without a proposal)


def c_idle(g, runs, b, ins, i):
    keep = b["group"] != i
    for k in ("group", "info", "term", "index", "hint"):
        b[k] = b[k][keep]
    b["props"][i] = 0
    return True


CASES = [c_follower_state, c_probe_follower, c_rejected_ack, c_stale_ack, c_same_follower, c_third_message,
         c_wrong_term, c_from_not_member, c_faulted, c_commit_zero, _self_slot(1), _self_slot(2), _small_n(1),
         _small_n(2), c_removed, c_last_index_2_40, c_lagging_ack, c_full_window, c_no_proposal, c_idle]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[2:])
def test_one_odd_lane_per_wave(case, monkeypatch):
    g, runs = _state()
    g["last_index"][list(ODD)] += 64  # (room below lastIndex for the lagging windows)
    for i in ODD:
        last = int(g["last_index"][i])
        g["committed"][i] = g["term_last"][i] = last
        g["pr"][i]["match"][:N] = last
        g["pr"][i]["next"][:N] = last + 1
        runs[i] = synth._runs_for(1, int(g["term_first"][i]), last, int(g["term"][i]))
    b = synth.cfg2_batch(g, 0, seed=703)
    b["hint"] = np.zeros(len(b["group"]), dtype=np.uint64)
    ins = {}
    steady = [case(g, runs, b, ins, i) for i in ODD]
    assert len(set(steady)) == 1
    pair = _pair(monkeypatch, g, runs, ins=ins)
    if case is c_removed:
        removed = np.array(ODD)
        for i in ODD:
            pair.eng.remove_groups(i, 1)
            pair.og.raft(i).n = 0
        dev_groups = pair.eng.get_groups

        def groups_but_removed():  # (a removed group's record is unspecified beyond n = 0)
            d = dev_groups()
            assert (d["n"][removed] == 0).all()
            d[removed] = pair.og.groups()[removed]
            return d
        pair.eng.get_groups = groups_but_removed
    pair.step(b, ctx=case.__name__)
    assert bool(pair.eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
    assert pair.eng.steady_waves() == (WAVES if steady[0] else WAVES - len(ODD))


def test_size_limit_on(monkeypatch):
    g, runs = synth.steady_groups(G, N, seed=711, last_hi=1 << 12)
    sizes = synth.window_sizes(g, runs, seed=712, frac_full=1.0)
    pair = _pair(monkeypatch, g, runs, max_msg_size=256, sizes=sizes)
    for step in range(2):
        b = synth.attach_entry_descs(synth.cfg2_batch(g, step, seed=713), G, seed=714 + step, max_len=100)
        _, st, _ = pair.step(b, ctx=f"size limit {step}")
        assert st[abi.HB_STAT_FAULTS] == 0
        assert pair.eng.steady_waves() == 0


def _stream(monkeypatch, env):
    """Events (per group), statistics and groups of a seeded 3-step stream
    with half of the waves steady, under the given create-time knobs."""
    from etcd_amd.hipbatch import Engine
    for k in ("HB_FAST_STEADY", "HB_ROUTE_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, _ = _state()
    rng = np.random.default_rng(721)
    g["pr"]["state"][rng.random(G) < 0.01, 1] = abi.HB_PR_PROBE  # (a Probe follower: its wave is not steady)
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=4 * G)
    eng.load_groups(g)
    eng.reserve_log(np.arange(G, dtype=np.uint32), None, np.full(G, 8, dtype=np.int64))
    out = []
    for step in range(3):
        eng.step_batch(synth.cfg2_batch(g, step, seed=722), host=True)
        fast = bool(eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        out.append((sort_events(eng.events()), eng.stats(), eng.get_groups(), fast))
    return out


@pytest.mark.parametrize("fuse", [None, "0"])
def test_switch_off_vs_on(fuse, monkeypatch):
    env = {} if fuse is None else {"HB_ROUTE_FUSE": fuse}
    on = _stream(monkeypatch, env)
    off = _stream(monkeypatch, dict(env, HB_FAST_STEADY="0"))
    for step, (a, b) in enumerate(zip(on, off)):
        assert a[3] == b[3] == (fuse is None)
        assert np.array_equal(a[0], b[0]), f"step {step}: events differ"
        assert np.array_equal(a[1], b[1]), f"step {step}: statistics differ"
        assert np.array_equal(a[2], b[2]), f"step {step}: groups differ"
        assert a[1][abi.HB_STAT_COMMITS] > G // 4


def test_mixed_stream(monkeypatch):
    g, runs, ins = synth.random_groups(G, N, seed=731, W=W)
    pair = _pair(monkeypatch, g, runs, ins=ins)
    rng = np.random.default_rng(732)
    now = pair.og.groups()
    for step in range(2):
        _, _, now = pair.step(synth.cfg3_open_batch(now, rng), ctx=f"mixed stream {step}")
