"""GPU tests of libhbnode's role-ordered slot placement (HBN_PLACE_ROLE).

The layout is read back from the device (hb_get_groups over the whole capacity
through hbn_engine) and checked against the invariant of include/hbnode.h: the
led groups dense in [0, led), the others dense in [led, led + other), at most
one mixed 64-slot tile; hbn_placement_stats must say the same.  Everything the
MultiNode API shows must be the same as under HBN_PLACE_ARRIVAL.
"""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import abi, hipbatch
from etcd_amd.multinode import (HBN_PLACE_ARRIVAL, HBN_PLACE_ROLE, Config, ConfChangeAddNode, ConfChangeRemoveNode, Entry,
                                MemoryStorage, Message, StartMultiNode, lib)

from .multinode_scenario import CAPACITY, run_random_scenario

pytestmark = pytest.mark.gpu

TILE = 64


def device_roles(mn, capacity):
    """(live, led) masks by slot from the device's own group records."""
    h = lib().hbn_engine(mn.p)
    out = np.zeros(capacity, dtype=abi.GROUP_DTYPE)
    assert hipbatch.lib().hb_get_groups(C.c_void_p(h), 0, capacity, out.ctypes.data) == abi.HB_OK
    live = out["n"] > 0
    return live, live & (out["state"] == abi.HB_STATE_LEADER)


def mixed_tiles(live, led):
    k = 0
    for t in range(0, len(live), TILE):
        a, b = led[t:t + TILE], (live & ~led)[t:t + TILE]
        k += bool(a.any() and b.any())
    return k


def check_role_layout(mn, capacity, ctx=""):
    """The invariant, from the device records, and PlacementStats agreeing with it."""
    live, led = device_roles(mn, capacity)
    T, L = int(live.sum()), int(led.sum())
    assert live[:T].all() and not live[T:].any(), f"{ctx}: live groups are not dense in [0, {T})"
    assert led[:L].all() and not led[L:].any(), f"{ctx}: led groups are not dense in [0, {L})"
    mixed = mixed_tiles(live, led)
    assert mixed <= 1, ctx
    st = mn.PlacementStats()
    assert (st["mode"], st["led"], st["other"], st["mixed_tiles"]) == (HBN_PLACE_ROLE, L, T - L, mixed), f"{ctx}: {st}"
    return st


@pytest.mark.parametrize("seed,n", [(1, 3), (2, 5), (3, 3)])
def test_random_multinode_role_placement_vs_oracle(seed, n):
    """The scenario of test_random_multinode_vs_oracle (96 groups, capacity 128,
    60 rounds, max_inflight 8) under HBN_PLACE_ROLE, with the same per-round
    Ready assertions; after every Advance the layout invariant, the statistics
    and the move bound: groups moved <= 2 x groups whose led / not-led role
    (the oracle's state) differs from the previous Advance.  A group whose
    oracle faulted in the round counts as one possible change (its state at the
    panic point is not specified); no group is removed here."""
    track = dict(prev_led={}, prev_dead=set(), moves=0, to_led=0, from_led=0)

    def after_advance(mn, st, gids, rnd):
        s = check_role_layout(mn, CAPACITY, f"seed {seed} round {rnd}")
        flips = 0
        for gid in gids:
            dead = bool(st[gid].get("dead"))
            if dead:
                flips += gid not in track["prev_dead"]
                track["prev_dead"].add(gid)
                continue
            led = st[gid]["o"].state == abi.HB_STATE_LEADER
            was = track["prev_led"].get(gid, False)
            flips += led != was
            track["to_led"] += led and not was
            track["from_led"] += was and not led
            track["prev_led"][gid] = led
        moved = s["moves_total"] - track["moves"]
        track["moves"] = s["moves_total"]
        assert moved <= 2 * flips, f"seed {seed} round {rnd}: {moved} moves for {flips} role changes"
        assert s["repacks"] == rnd + 2  # SetPlacement's and one per Advance

    mn, st, gids, _ = run_random_scenario(seed, n, setup=lambda m: m.SetPlacement(HBN_PLACE_ROLE),
                                          after_advance=after_advance)
    assert track["moves"] > 0 and track["to_led"] > 0 and track["from_led"] > 0, track
    mn.Stop()


def _status(mn, gid):
    s = mn.Status(gid)
    if s is None:
        return None
    prog = {k: (p.match, p.next, p.pending_snapshot, p.state, p.paused, p.ins_start, p.ins_count)
            for k, p in s.Progress.items()}
    return (s.ID, s.HardState, s.SoftState, s.Applied, prog)


class _Twin:
    """Two nodes fed the same input; every Ready must be the same by group id."""

    def __init__(self, capacity, n_groups, max_replicas=5):
        self.nodes = [StartMultiNode(1, capacity=capacity, max_replicas=max_replicas, max_inflight=8) for _ in range(2)]
        draws = np.random.default_rng(5).integers(0, 1 << 62, 1 << 12, dtype=np.uint64)
        self.stor = [{}, {}]
        for mn in self.nodes:
            mn.SetRand(draws)
        self.gids = []
        for gid in range(1, n_groups + 1):
            self.create(gid)

    def create(self, gid):
        for mn, st in zip(self.nodes, self.stor):
            st[gid] = MemoryStorage()
            mn.CreateGroup(gid, Config(election=10, heartbeat=1), st[gid], peers=[1, 2, 3])
        self.gids.append(gid)

    def remove(self, gid):
        for mn, st in zip(self.nodes, self.stor):
            mn.RemoveGroup(gid)
            del st[gid]
        self.gids.remove(gid)

    def both(self, fn):
        return [fn(mn) for mn in self.nodes]

    def step(self, gid, m):
        self.both(lambda mn: mn.Step(gid, m))

    def cycle(self, ctx):
        """Ready on both, equal by group id; storage append; Advance.  Returns the Ready."""
        ra, rb = self.both(lambda mn: mn.Ready())
        assert sorted(ra) == sorted(rb), f"{ctx}: groups {sorted(set(ra) ^ set(rb))[:5]}"
        for gid in ra:
            assert ra[gid] == rb[gid], f"{ctx}: group {gid}\n arrival {ra[gid]}\n role    {rb[gid]}"
        for rds, mn, st in zip((ra, rb), self.nodes, self.stor):
            for gid, rd in rds.items():
                assert rd.fault == 0, f"{ctx}: group {gid} faulted"
                st[gid].Append(rd.Entries)
            mn.Advance(rds)
        return ra

    def drain(self, ctx):
        out = self.cycle(ctx)
        for k in range(4):
            if not self.cycle(f"{ctx} +{k + 1}"):
                break
        return out

    def statuses_equal(self, ctx):
        for gid in self.gids:
            a, b = self.both(lambda mn: _status(mn, gid))
            assert a == b, f"{ctx}: Status of group {gid}\n arrival {a}\n role    {b}"

    def elect(self, gids, term=2):
        for gid in gids:
            self.both(lambda mn: mn.Campaign(gid))
            self.step(gid, Message(Type=abi.HB_MSG_VOTE_RESP, From=2, To=1, Term=term))

    def stop(self):
        self.both(lambda mn: mn.Stop())


def test_placement_is_unobservable():
    """130 groups of n = 3 in capacity 256 (max_inflight 8), every even group
    led: interleaved under arrival order (>= 2 mixed tiles).  SetPlacement(ROLE)
    on one of two identically fed nodes leaves <= 1 mixed tile and every Status
    as it was; then proposals and MsgAppResp to the leaders, MsgApp and
    MsgHeartbeat to the followers, leaders deposed by a higher term,
    RemoveGroup of a moved leader and a moved follower, ApplyConfChange add and
    remove on moved leaders, two new groups, a Tick: after each cycle the two
    nodes' Ready dictionaries are equal by group id, and the role node keeps its
    layout."""
    CAP, NG = 256, 130
    tw = _Twin(CAP, NG)
    arrival, role = tw.nodes
    tw.drain("bootstrap")
    leaders = [g for g in tw.gids if g % 2 == 0]
    followers = [g for g in tw.gids if g % 2 == 1]
    tw.elect(leaders)
    tw.drain("elect")
    live, led = device_roles(arrival, CAP)
    assert int(led.sum()) == len(leaders) and mixed_tiles(live, led) >= 2
    assert arrival.PlacementStats()["mixed_tiles"] == mixed_tiles(live, led)

    before = {g: _status(role, g) for g in tw.gids}
    role.SetPlacement(HBN_PLACE_ROLE)
    st = check_role_layout(role, CAP, "SetPlacement")
    assert st["moves_total"] > 0 and st["led"] == len(leaders) and st["other"] == len(followers)
    assert {g: _status(role, g) for g in tw.gids} == before, "SetPlacement changed a Status"
    assert arrival.PlacementStats()["mode"] == HBN_PLACE_ARRIVAL and arrival.PlacementStats()["moves_total"] == 0

    def traffic(ctx, k):
        for g in leaders:
            if g in tw.gids:
                tw.both(lambda mn: mn.Propose(g, f"{g}-{k}".encode()))
        tw.drain(f"{ctx} propose")
        for g in leaders:
            if g in tw.gids:
                last = tw.stor[0][g].LastIndex()
                tw.step(g, Message(Type=abi.HB_MSG_APP_RESP, From=2, To=1, Term=lead_term[g], Index=last))
        for g in followers:
            if g in tw.gids:
                last = tw.stor[0][g].LastIndex()
                tw.step(g, Message(Type=abi.HB_MSG_APP, From=2, To=1, Term=2, LogTerm=tw.stor[0][g].Term(last)[0],
                                   Index=last, Entries=[Entry(Term=2, Index=last + 1, Data=b"f%d" % k)], Commit=last))
                tw.step(g, Message(Type=abi.HB_MSG_HEARTBEAT, From=2, To=1, Term=2, Commit=last))
        tw.drain(f"{ctx} traffic")
        check_role_layout(role, CAP, ctx)
        tw.statuses_equal(ctx)

    lead_term = {g: 2 for g in leaders}
    traffic("round 0", 0)
    # some leaders step down on a higher-term message; they are followers from here on
    for g in leaders[::7]:
        tw.step(g, Message(Type=abi.HB_MSG_HEARTBEAT, From=3, To=1, Term=5, Commit=0))
    tw.drain("depose")
    s = check_role_layout(role, CAP, "depose")
    assert s["led"] == len(leaders) - len(leaders[::7])
    deposed = set(leaders[::7])
    leaders = [g for g in leaders if g not in deposed]
    # (the deposed groups stay out of both lists: they follow node 3 at term 5 and get no more traffic)
    tw.statuses_equal("depose")
    # groups that SetPlacement moved: led groups from slots >= 65 (ids >= 66), followers from slots < 65
    moved_leader, moved_follower, cc_add, cc_rm = 96, 3, 102, 104
    assert {moved_leader, cc_add, cc_rm} <= set(leaders) and moved_follower in followers
    tw.remove(moved_leader)
    tw.remove(moved_follower)
    leaders.remove(moved_leader)
    followers.remove(moved_follower)
    assert tw.both(lambda mn: mn.ApplyConfChange(cc_add, ConfChangeAddNode, 4)) == [[1, 2, 3, 4]] * 2
    assert tw.both(lambda mn: mn.ApplyConfChange(cc_rm, ConfChangeRemoveNode, 3)) == [[1, 2]] * 2
    tw.create(201)
    tw.create(202)
    followers += [201, 202]
    tw.drain("membership")
    check_role_layout(role, CAP, "membership")
    traffic("round 1", 1)
    tw.elect([201], term=3)  # a group created under ROLE becomes led (its follower traffic was at term 2)
    tw.drain("elect new")
    followers.remove(201)
    leaders.append(201)
    lead_term[201] = 3
    tw.both(lambda mn: mn.Tick())
    tw.drain("tick")
    traffic("round 2", 2)
    s = check_role_layout(role, CAP, "end")
    assert s["led"] == len(leaders) and s["led"] + s["other"] == len(tw.gids)
    tw.stop()


def test_placement_with_no_free_slot():
    """8 groups of n = 3 in capacity 8 under HBN_PLACE_ROLE from the start: with
    no free slot every re-pack is made of swaps and cycles.  Leaders are elected
    and deposed in turns; Ready equals the arrival-order node's every cycle."""
    tw = _Twin(8, 0)
    arrival, role = tw.nodes
    role.SetPlacement(HBN_PLACE_ROLE)
    for gid in range(1, 9):
        tw.create(gid)
    tw.drain("bootstrap")
    check_role_layout(role, 8, "bootstrap")
    term = {g: 1 for g in tw.gids}
    plan = [("up", [2, 4, 6, 8]), ("down", [4, 8]), ("up", [1, 3]), ("down", [2, 1]), ("up", [4, 5, 7, 8, 2, 1]),
            ("down", [3, 6]), ("up", [3, 6])]  # the last round: all 8 led
    for k, (what, gs) in enumerate(plan):
        for g in gs:
            if what == "up":
                term[g] += 1
                tw.both(lambda mn: mn.Campaign(g))
                tw.step(g, Message(Type=abi.HB_MSG_VOTE_RESP, From=2, To=1, Term=term[g]))
            else:
                term[g] += 3
                tw.step(g, Message(Type=abi.HB_MSG_HEARTBEAT, From=3, To=1, Term=term[g], Commit=0))
        tw.drain(f"plan {k}")
        check_role_layout(role, 8, f"plan {k}")
        tw.statuses_equal(f"plan {k}")
    s = role.PlacementStats()
    assert s["led"] == 8 and s["other"] == 0 and s["moves_total"] > 0
    tw.stop()
