"""Cluster parity: three engines that each lead some groups and follow others
exchange nothing but the frames and byte spans they wrote, for 52 rounds, with every knob of the
wire path on: egress mode 7, hb_set_egress_logterm, hb_set_wire_props in and out,
hb_set_egress_limit under the finite limit, framed peer streams, per-node slot placements.

tests/cluster_util.py holds the harness; tests/test_cluster_ref.py runs the same scenarios on the
CPU and asserts what they reach.  Here every round compares, for every node and phase:
hb_unframe's rows, hb_decode_follow's batch and entry columns, the step's and the tick's events,
stats, group records, inflight windows and timers, hb_egress' records, hb_egress_bin's offsets and
order, hb_encode_ents' bytes, off and status, hb_peer_spans and hb_frame's index, each with its CPU
reference; and, independently, the per-peer byte stream with the messages the reference cluster of
Raft objects sent to that peer.  The engines step what the other engines wrote, and a new leader
re-sends entries from a store filled from hb_decode_follow's outputs alone.

test_compacting / test_compacting_moving: the same under log compaction.  hb_set_log_bounds after
every second round, hb_reserve_log by need before every call with hb_log_capacity compared with the
prediction, HB_EV_SNAP against the reference's MsgSnap, the MsgSnap and MsgSnapStatus rows decoded
as HB_WIRE_HOST / HB_WIRE_LOCAL and then written by the host into the decoded device batch, the
restore in k_follow, and replication resumed from a source window that starts at firstIndex.
"""
import pytest

from .cluster_util import NODES, Cluster, GpuNode, scenario

pytestmark = pytest.mark.gpu


def _run(name, monkeypatch, small=True):
    if small:
        monkeypatch.delenv("HB_SMALL_STEP", raising=False)
    else:
        monkeypatch.setenv("HB_SMALL_STEP", "0")  # read at hb_create: the tiled launches
    c = Cluster(scenario(name), device=GpuNode)
    try:
        c.run().check_end()
        for v in NODES:
            c.dev[v].check_end(c.B[v])
    finally:
        for v in NODES:
            c.dev[v].close()


@pytest.mark.parametrize("small", [True, False], ids=["default", "HB_SMALL_STEP=0"])
def test_elections(monkeypatch, small):
    _run("elections", monkeypatch, small)


def test_limited(monkeypatch):
    _run("limited", monkeypatch)


def test_moving(monkeypatch):
    _run("moving", monkeypatch)


def test_compacting(monkeypatch):
    _run("compacting", monkeypatch)


def test_compacting_moving(monkeypatch):
    _run("compacting_moving", monkeypatch)
