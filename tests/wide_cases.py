"""The scenarios of the wide-value suite: the bodies of tests/test_parity_gpu.py
run at the bases of tests/lift_util.py.  tests/test_wide_values_gpu.py runs
every (case, base) against the engine; tests/test_lift.py runs the same list
through the oracle alone and asserts the generator's conditions (both record
formats in play, faulted share), so a GPU case cannot pass by hiding its
values."""
from . import test_parity_gpu as P
from .lift_util import BASES

WIDE = ("W40", "W62")

# name -> (body, arguments, bases, takes (storm, monkeypatch))
CASES = {
    # random states and every message type: the general k_apply, k_apply_lead<5|7>, k_elect
    "fuzz-n3": (P.run_fuzz_all_message_types, (1, 3, 8), BASES, False),
    "fuzz-n5": (P.run_fuzz_all_message_types, (2, 5, 8), BASES, False),
    "fuzz-n7": (P.run_fuzz_all_message_types, (3, 7, 4), BASES, False),
    # follower side with term runs and timers: k_follow<5|7>
    "follower-n3": (P.run_fuzz_follower_side, (71, 3, 8), BASES, False),
    "follower-n5": (P.run_fuzz_follower_side, (72, 5, 16), BASES, False),
    "follower-n7": (P.run_fuzz_follower_side, (73, 7, 8), BASES, False),
    # k_tick
    "tick-n3": (P.run_tick_random_states, (31, 3, 8), BASES, False),
    "tick-n5": (P.run_tick_random_states, (32, 5, 8), BASES, False),
    "tick-n7": (P.run_tick_random_states, (33, 7, 16), BASES, False),
    # sz_limit and the size ring
    "finite-n3": (P.run_fuzz_finite_max_msg_size, (61, 3, 8, 40), WIDE, False),
    "finite-n5": (P.run_fuzz_finite_max_msg_size, (62, 5, 16, 150), WIDE, False),
    "finite-n7": (P.run_fuzz_finite_max_msg_size, (63, 7, 8, 1000), WIDE, False),
    "deep-lag": (P.run_deep_lag_finite_max_msg_size, (), WIDE, False),
    # the lead lanes and the n = 3 fast lane
    "cfg2-n5": (P.run_cfg2_steady_replication, (2500, 5), WIDE, False),
    "cfg2-n7": (P.run_cfg2_steady_replication, (1500, 7), WIDE, False),
    "msgprop": (P.run_msgprop_messages_on_fast_lane, (False,), WIDE, False),
    "msgprop-sized": (P.run_msgprop_messages_on_fast_lane, (True,), WIDE, False),
    "cfg3": (P.run_cfg3_lagging_followers_closed_loop, (), WIDE, False),
    # the LDS route slots and the storm hand-over
    "storm-n5": (P.run_cfg4_storm_repeatable_stream, (5,), WIDE, True),
    "storm-n7": (P.run_cfg4_storm_repeatable_stream, (7,), WIDE, True),
    "handover-n5": (P.run_storm_handover_class_boundaries, (5,), WIDE, True),
    "handover-n7": (P.run_storm_handover_class_boundaries, (7,), WIDE, True),
    "tick-elect": (P.run_tick_elections_and_heartbeats, (), WIDE, False),
    "commit-zero": (P.run_fast_lanes_hand_over_commit_zero_groups, (), WIDE, False),
}

PLAIN = [(c, b) for c, (_, _, bases, storm) in CASES.items() if not storm for b in bases]
STORM = [(c, b) for c, (_, _, bases, storm) in CASES.items() if storm for b in bases]


def run(case, base, make, storm=None, monkeypatch=None):
    fn, args, _, takes_storm = CASES[case]
    if takes_storm:
        return fn(*args, storm, monkeypatch, lift=base, make=make)
    return fn(*args, lift=base, make=make)
