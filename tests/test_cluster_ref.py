"""The CPU twin of tests/test_cluster_gpu.py: the same scenarios with the
references of tests/cluster_util.py standing in for the engines, in the manner of
parity_util.OraclePair.  It proves that the references agree with each other and that the
scenarios reach what they claim.

In every round, for every node and phase: the batch oracle's group records equal the Raft
objects' field for field; the replayed records, encoded, binned and framed by the CPU
references, are (A)'s messages per peer and group, byte for byte and in r.msgs order (a record
handed to the host is completed from (A) and counted); a frame is read back by frame.unframe and
the decode reference into the batch the next oracle steps.  At the end the three log stores
agree with the registry on every committed entry, committed never went back, and no two nodes
led a group in one term.  Then the conditions of cluster_util.check_conditions hold.

The compacting scenarios add: every HB_EV_SNAP event is a MsgSnap of the Raft objects and the
message the host builds of it is theirs byte for byte; a MsgSnap row and a MsgSnapStatus row
decode as left to the host before the host writes their records; the three layers agree after
every compaction; the stores start at firstIndex; cluster_util.compacting_conditions hold.
"""
import pytest

from .cluster_util import Cluster, check_conditions, scenario


@pytest.mark.parametrize("name", ["elections", "limited", "moving", "compacting", "compacting_moving"])
def test_cluster_twin(name):
    c = Cluster(scenario(name)).run().check_end()
    print(name, check_conditions(c))
