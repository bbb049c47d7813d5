"""A round-based cluster of three nodes that exchange only wire frames.

Three layers, each an independent reference of the next:

  (A) RefCluster   G groups x 3 oracle.pyoracle.Raft objects that exchange the messages
                   readMessages() returns; entry payloads live in a registry keyed by
                   (group, index, term), which names an entry by Log Matching.
  (B) NodeRef      per node an OracleGroups over its replica of every group, stepped in the
                   engine's batch format, with the CPU references of the wire path around it:
                   frame.unframe + frame.Directory, props_reference, the event replays,
                   bin_reference, encode_ents_reference, frame.build_index.
  (C) a device     per node an Engine behind move_util.SlotView (tests/test_cluster_gpu.py);
                   tests/test_cluster_ref.py runs the same rounds with (B) in its place.

One round of a node: phase 1 steps one batch (the frames the other nodes sent it in the
previous round, ascending sender, each sender's phase-1 frame before its phase-2 frame, rows
in frame order; then its clients' proposals as MsgProp records from itself) and runs the send
chain; phase 2 ticks and runs the send chain.  What a node emits in round r arrives in round
r + 1, unless the fault schedule drops the whole frame.

The nodes form a closed loop: a node steps the bytes the other nodes wrote.  Where the device
hands a record to the host (a hole in the frame) the harness plays the host: a forwarded
MsgProp (HB_WIRE_SPLICE, by design) is completed with etcd_amd.splice from the entries of the
proposal's arrival, an HB_OUT_HOST record from (A)'s message; the completed bytes travel beside
the frame and take the hole's row at the receiver.

The `compacting` scenarios add log compaction: every node's application compacts at committed -
keep on every k-th round (Raft.compact / OracleGroups.compact / hb_set_log_bounds), the rings are
reserved by compact_util's rule before every call, and a follower that fell below a leader's
firstIndex is caught up with a MsgSnap.  HB_EV_SNAP makes no record, so the harness plays the host
once more: it builds the message from the event, ships it beside the frame, gives it a row of its
own at the receiver (after the rows its sender's frame holds for the group from before the event),
and writes the HB_MSG_SNAP record into that row of the decoded batch, which hb_decode_follow left
to the host.  The transport's ReportSnapshot comes back a round later as a local MsgSnapStatus row.
"""
import numpy as np

from etcd_amd import abi, frame
from etcd_amd.splice import splice
from oracle import pyoracle
from oracle.pyoracle import Msg, OracleGroups, Raft

from . import props_util as PU
from . import wire_util as W
from .compact_util import _Compacting
from .egress_app_util import is_app, marshal, status_of
from .egress_bin_util import bin_reference
from .egress_limit_util import follower_rewrites, szlo_final
from .egress_logterm_util import lookup_sends, replay_apps_logterm, ring_oldest
from .egress_vote_util import oracle_older_runs
from .encode_ents_util import build_source, encode_ents_reference, records_of

NODES = (1, 2, 3)
NO_LIMIT = abi.HB_NO_LIMIT
RUN_CAP = 64      # term-run ring capacity reserved for every group: no run is ever dropped
SIZE_CAP = 1024   # size ring capacity: no cumulative size is ever dropped
M32 = 0xFFFFFFFF
OK, HOST, SPLICE, LOCAL = abi.HB_WIRE_OK, abi.HB_WIRE_HOST, abi.HB_WIRE_SPLICE, abi.HB_WIRE_LOCAL
RECORD_EVENTS = (abi.HB_EV_APP, abi.HB_EV_VOTE, abi.HB_EV_RESP, abi.HB_EV_HEARTBEAT)
BATCH = ("group", "info", "term", "index", "hint", "commit")
SNAP_DATA = b"app state"  # Snapshot.Data of every MsgSnap (its ConfState names the three nodes)


def others(v):
    return [u for u in NODES if u != v]


def desc_of(p):
    return abi.hb_ent_desc(0 if p is None else len(p), 0, p is not None)


class Scenario:
    """Everything a run is a function of: sizes, timers, placements, proposals and faults."""

    def __init__(self, name, limit=NO_LIMIT, moving=False, G=96, capacity=128, rounds=52, W=8, seed=11,
                 partition=(1, 8, 22), drop=0.01, election=(8, 4, 6), favour=(0.4, 0.3, 0.3), lens=(None, 0, 1, 5, 16, 40),
                 rate=0.5, compact=None):
        self.name, self.limit, self.moving, self.G, self.capacity = name, limit, moving, G, capacity
        self.compact = compact  # (k, keep): on every k-th round the application compacts at committed - keep
        self.rounds, self.W, self.seed, self.partition, self.election, self.lens = rounds, W, seed, partition, election, lens
        rng = np.random.default_rng(seed)
        ids = set()
        while len(ids) < G:
            ids.update(int(x) | (1 << 63) for x in rng.integers(1, 1 << 62, G - len(ids), dtype=np.uint64))
        self.gid = np.array(sorted(ids), np.uint64)[rng.permutation(G)]
        self.draws = {v: rng.integers(0, 1 << 32, 4096, dtype=np.uint64) for v in NODES}
        # staggered elections: every group has a favourite node whose timer is about to fire
        fav = rng.choice(NODES, G, p=favour)
        self.elapsed0 = {v: np.where(fav == v, rng.integers(election[v - 1], 2 * election[v - 1], G),
                                     rng.integers(0, election[v - 1] // 2, G)).astype(np.uint32) for v in NODES}
        self.rand_pos0 = {v: rng.integers(0, 1024, G).astype(np.uint32) for v in NODES}
        self.perm = {v: rng.permutation(capacity)[:G].astype(np.int64) for v in NODES}
        self.lost = rng.random((rounds, 2, 4, 4)) < drop
        self.props = []
        for r in range(rounds):
            per = {v: [] for v in NODES}
            go = rng.random((G, 4)) < rate
            cnt = rng.integers(1, 4, (G, 4))
            for g in range(G):
                for v in NODES:
                    if go[g, v]:
                        per[v].append((g, [self.payload(g, v, r, k) for k in range(int(cnt[g, v]))]))
            self.props.append(per)
        self.move_rng = {v: np.random.default_rng(seed * 1000 + v) for v in NODES}

    def payload(self, g, v, r, k):
        h = (g * 7919 + v * 104729 + r * 1299709 + k * 15485863 + self.seed) & M32
        ln = self.lens[h % len(self.lens)]
        return None if ln is None else bytes(((h >> 8) + 5 * j) & 0xFF for j in range(ln))

    def dropped(self, r, phase, s, d):
        p, lo, hi = self.partition
        return bool((lo <= r < hi and p in (s, d)) or self.lost[r, phase, s, d])

    @property
    def compacting(self):
        return self.compact is not None

    @property
    def sized(self):
        return self.limit not in (0, NO_LIMIT)


def msg_bytes(d):
    snap = d.get("snap")
    return W.gogo_marshal(d["type"], to=d["to"], frm=d["frm"], term=d["term"], log_term=d["log_term"], index=d["index"],
                          entries=d["ents"], commit=d["commit"], reject=d["reject"], hint=d["hint"],
                          snapshot=None if snap is None else (SNAP_DATA, NODES) + snap)


def is_snap(d):
    return d["type"] == abi.HB_MSG_SNAP


def slot_of(node):
    return NODES.index(node)


class Log:
    """One group's entries in a node's store, from index `first` on: [(term, desc, Data, Entry.Size())]."""

    def __init__(self):
        self.first, self.ents = 1, []

    @property
    def next(self):
        return self.first + len(self.ents)

    def __getitem__(self, i):
        assert self.first <= i < self.next, f"entry {i} of a store that holds [{self.first}, {self.next})"
        return self.ents[i - self.first]

    def cut(self, lo):
        """Everything from index lo on leaves (a conflicting append)."""
        del self.ents[max(lo, self.first) - self.first:]

    def drop_below(self, first):
        """The application compacted: the store starts at `first`."""
        assert self.first <= first <= self.next
        del self.ents[:first - self.first]
        self.first = first

    def restart(self, first):
        """A restore: nothing but the snapshot below `first`."""
        self.first, self.ents = first, []


class Rings(_Compacting):
    """compact_util's reserve rule and capacity prediction for one node's groups (`eng`: the node's
    SlotView on the device, None in the twin)."""

    def __init__(self, og, sized):
        self.og, self.sized, self.eng, self.gpu = og, sized, None, False
        self._start(None, None)
        self.pushed = np.zeros(self.G, np.int64)  # entries appended since the group's last restore

    def attach(self, eng):
        self.eng, self.gpu = eng, True
        self.check_capacity("load")

    def before(self, batch=None, extra=0):
        """Before a step or a tick: hb_reserve_log by the rule."""
        self.reserve(batch, extra)
        self.b4 = self._before()

    def after(self, ev):
        """After it: the counters, and every 8th call hb_log_capacity against the prediction."""
        appended = self.appended.copy()
        self._after(self.b4, ev)
        self.pushed += self.appended - appended
        f = ev[(ev["type"] == abi.HB_EV_FOLLOW) & (ev["aux"] == abi.HB_FOLLOW_RESTORE)]
        self.pushed[f["group"].astype(np.int64)] = 0

    def wrapped(self):
        """The groups whose size ring has dropped an element since it last restarted."""
        return self.pushed >= self.cap_sz


# ---- (A) the reference cluster ----------------------------------------------------------------
class RefCluster:
    def __init__(self, sc):
        self.sc, self.registry, self.count = sc, {}, {}
        self.rafts = {}
        for v in NODES:
            self.rafts[v] = []
            for g in range(sc.G):
                r = Raft(v, list(NODES), max_inflight=sc.W, max_msg_size=sc.limit, election=sc.election[v - 1],
                         heartbeat=1, draws=sc.draws[v])
                r.r.elapsed, r.r.rand_pos = int(sc.elapsed0[v][g]), int(sc.rand_pos0[v][g])
                self.rafts[v].append(r)
        self.led = {}  # (group, term) -> node
        self.snap_groups, self.restored, self.restored_led = set(), set(), set()

    def _bump(self, k, n=1):
        self.count[k] = self.count.get(k, 0) + n

    def _drain(self, v, g, last0, payloads):
        r = self.rafts[v][g]
        if r.state == abi.HB_STATE_LEADER:
            who = self.led.setdefault((g, r.Term), v)
            assert who == v, f"group {g}: nodes {who} and {v} both led term {r.Term}"
            grown = r.lastIndex - last0
            if grown:
                pl = payloads if payloads is not None else [None]  # becomeLeader's empty entry
                assert grown == len(pl)
                for k, p in enumerate(pl):
                    self.registry[(g, last0 + 1 + k, r.Term)] = p
        out = []
        for m in r.readMessages():
            d = dict(g=g, type=m.Type, to=m.To, frm=m.From, term=m.Term, log_term=m.LogTerm, index=m.Index,
                     commit=m.Commit, reject=bool(m.Reject), hint=m.RejectHint, ents=[])
            if m.Type == abi.HB_MSG_APP:
                for i in range(m.Index + 1, m.Index + 1 + m.nents):
                    t = r.term(i)
                    d["ents"].append((0, t, i, self.registry[(g, i, t)]))
                self._bump("app")
                if m.nents:
                    self._bump("app_ents")
                    if m.Index + m.nents < r.lastIndex:
                        self._bump("app_cut")
                    if m.Index == r.firstIndex - 1 and r.firstIndex > 1:
                        self._bump("app_at_boundary")  # LogTerm is the dummy entry's
                    if (v, g) in self.restored:
                        self.restored_led.add(g)       # a node that restored the group sends from its store
                if m.LogTerm < m.Term:
                    self._bump("app_below_term")
            elif m.Type == abi.HB_MSG_PROP:
                d["ents"] = [(0, 0, 0, p) for p in payloads]
                self._bump("prop_fwd")
            elif m.Type == abi.HB_MSG_APP_RESP and m.Reject:
                self._bump("app_resp_reject")
            elif m.Type == abi.HB_MSG_VOTE_RESP and m.Reject:
                self._bump("vote_resp_reject")
            elif m.Type == abi.HB_MSG_SNAP:
                assert self.sc.compacting and m.snap_index == r.firstIndex - 1
                d["snap"] = (m.snap_index, m.snap_term or r.term(m.snap_index))
                self._bump("snap_sent")
                self.snap_groups.add((g, m.To))
            d["bytes"] = msg_bytes(d)
            out.append(d)
        if r.state == abi.HB_STATE_LEADER and payloads is not None:
            for u in others(v):  # a send the full window refused
                p = r.pr(u)
                if p.State == abi.HB_PR_REPLICATE and p.ins.count == p.ins.size and p.Next <= r.lastIndex:
                    self._bump("window_full")
        return out

    @staticmethod
    def _orc(d):
        if d["type"] == abi.HB_MSG_PROP:
            return Msg(d["type"], From=d["frm"], To=d["to"], Entries=len(d["ents"]), edesc=[desc_of(e[3]) for e in d["ents"]])
        return Msg(d["type"], From=d["frm"], To=d["to"], Term=d["term"], Index=d["index"], LogTerm=d["log_term"],
                   Commit=d["commit"], Reject=d["reject"], RejectHint=d["hint"], Entries=[(e[2], e[1]) for e in d["ents"]],
                   edesc=[desc_of(e[3]) for e in d["ents"]], Snapshot=d.get("snap"))

    def phase1(self, v, inbox, props, reports=()):
        """The frames' messages, the transport's ReportSnapshot calls [(group, to, reject)] as local
        MsgSnapStatus, the clients' proposals."""
        out = []
        for d in inbox:
            r = self.rafts[v][d["g"]]
            last0, first0 = r.lastIndex, r.firstIndex
            r.Step(self._orc(d))
            if is_snap(d):
                if r.firstIndex != first0:
                    assert (r.firstIndex, r.lastIndex, r.committed) == (d["snap"][0] + 1,) + (d["snap"][0],) * 2
                    self._bump("snap_restored")
                    self.restored.add((v, d["g"]))
                else:
                    self._bump("snap_ignored")
                last0 = r.lastIndex
            out += self._drain(v, d["g"], last0, [e[3] for e in d["ents"]] if d["type"] == abi.HB_MSG_PROP else None)
        for g, to, reject in reports:
            r = self.rafts[v][g]
            last0 = r.lastIndex
            r.Step(Msg(abi.HB_MSG_SNAP_STATUS, From=to, To=v, Reject=reject))
            out += self._drain(v, g, last0, None)
            self._bump("snap_status_reject" if reject else "snap_status_ok")
        for g, pl in props:
            r = self.rafts[v][g]
            last0 = r.lastIndex
            r.Step(Msg(abi.HB_MSG_PROP, From=v, To=v, Entries=len(pl), edesc=[desc_of(p) for p in pl]))
            out += self._drain(v, g, last0, pl)
        return out

    def phase2(self, v):
        out = []
        for g, r in enumerate(self.rafts[v]):
            last0 = r.lastIndex
            r.tick()
            out += self._drain(v, g, last0, None)
        return out

    def compact(self, v):
        """Node v's application compacts every group whose committed - keep lies above its firstIndex,
        there, with a snapshot: (groups, indices)."""
        gs, at = [], []
        for g, r in enumerate(self.rafts[v]):
            i = r.committed - self.sc.compact[1]
            if i > r.firstIndex:
                assert r.compact(i, snapshot=True) == 0
                gs.append(g)
                at.append(i)
        self._bump("compactions", len(gs))
        return gs, at

    def groups(self, v):
        return np.array([np.frombuffer(bytes(r.to_group()), dtype=abi.GROUP_DTYPE)[0] for r in self.rafts[v]],
                        dtype=abi.GROUP_DTYPE)

    def leaders(self):
        """Per group the node that leads it at the highest term, 0 for none."""
        out = np.zeros(self.sc.G, np.int64)
        for g in range(self.sc.G):
            best = -1
            for v in NODES:
                r = self.rafts[v][g]
                if r.state == abi.HB_STATE_LEADER and r.Term > best:
                    best, out[g] = r.Term, v
        return out

    def committed(self):
        return np.array([[self.rafts[v][g].committed for g in range(self.sc.G)] for v in NODES], np.int64)


# ---- (B) one node's references ------------------------------------------------------------------
class Snap:
    pass


class NodeRef:
    def __init__(self, sc, v, groups0):
        G = sc.G
        self.sc, self.v, self.G, self.C = sc, v, G, sc.capacity
        self.og = OracleGroups(groups0, [[(0, 0)]] * G, sc.W, sc.limit)
        t = np.zeros(G, abi.TIMER_DTYPE)
        t["election_tick"], t["heartbeat_tick"] = sc.election[v - 1], 1
        t["elapsed"], t["rand_pos"] = sc.elapsed0[v], sc.rand_pos0[v]
        self.timers0 = t
        self.og.load_timers(t)
        self.draws = sc.draws[v]
        self.peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
        self.peers[:, :3] = NODES
        self.slot = sc.perm[v].copy()
        self.store = {}   # (group, index, term) -> (desc, Data or None): what this node's host saw on the wire
        self.log = [Log() for _ in range(G)]  # per group the entries from the first held index on
        self.rings = Rings(self.og, sc.sized) if sc.compacting else None
        self.count = {}
        self.arrivals = {}
        self.commit_seen = np.zeros(G, np.int64)

    def _bump(self, k, n=1):
        self.count[k] = self.count.get(k, 0) + n

    # -- placement ------------------------------------------------------------------------------
    def inverse(self):
        inv = np.full(self.C, -1, np.int64)
        inv[self.slot] = np.arange(self.G)
        return inv

    def gid_col(self):
        col = np.zeros(self.C, np.uint64)
        col[self.slot] = self.sc.gid
        return col

    def directory(self):
        return frame.Directory(self.gid_col())

    def peers_cap(self):
        p = np.zeros((self.C, abi.HB_MAX_REPLICAS), np.uint64)
        p[self.slot, :3] = NODES
        n = np.zeros(self.C, np.uint32)
        n[self.slot] = 3
        return p, n

    # -- receive ---------------------------------------------------------------------------------
    def assemble(self, emissions, props, reports=()):
        """The transport: emissions = [(sender, frame bytes or None, span bytes, [(row, bytes)], [MsgSnap])]
        in delivery order, props = [(group, [Data])] of this node's clients, reports = [(group, to,
        reject)] of its own ReportSnapshot calls.  One index buffer, one byte buffer, the frame list
        of hb_unframe, the host's rows (frame row -> bytes), the MsgSnap rows (each where its sender's
        events put it among the frame's rows of its group) and the extra records."""
        index, data, frames, fills, snaps, base = b"", b"", [], [], [], 0
        for s, fr, sp, fl, sn in emissions:
            gids = frame.parse_index(fr)["gid"] if fr is not None else np.zeros(0, np.uint64)
            for d in sn:  # after the `before` rows the frame has for its group, before the next one
                mine = np.nonzero(gids == self.sc.gid[d["g"]])[0]
                snaps.append((base + (int(mine[d["before"]]) if d["before"] < len(mine) else len(gids)), d))
            if fr is None:
                continue
            assert len(index) % 8 == 0
            frames.append((len(index), len(fr), len(data), len(sp), s))
            index += fr
            data += sp
            fills += [(base + j, fr, j, b) for j, b in fl]
            base += frame.rows(len(fr))
        extra = []
        for g, to, reject in reports:
            extra.append((g, W.gogo_marshal(abi.HB_MSG_SNAP_STATUS, to=self.v, frm=to, reject=reject),
                          dict(info=abi.hb_info(abi.HB_MSG_SNAP_STATUS, slot_of(to), reject), term=0, index=0, hint=0)))
        for g, pl in props:
            extra.append((g, PU.prop(pl, to=self.v, frm=self.v), None))
        return dict(index=index, data=data, frames=frames, fills=fills, snaps=snaps, extra=extra, nf=base)

    def rows(self, asm, uf, d):
        """hb_unframe's rows, the holes the host fills patched in, the MsgSnap rows inserted where
        assemble placed them, the ReportSnapshot rows and the clients' proposals behind.  Leaves
        self.host_rows = [(row, the status the decoder must give it, the record the host writes)]."""
        off, ln, grp = (a.copy() for a in uf[:3])
        blob = bytearray(asm["data"])
        for row, fr, j, b in asm["fills"]:
            gid = int(frame.parse_index(fr)["gid"][j])
            assert grp[row] == frame.NO_SLOT and ln[row] == 0
            off[row], ln[row], grp[row] = len(blob), len(b), d.lookup(gid) if gid else frame.NO_SLOT
            blob += b
        self.host_rows = []
        if asm["snaps"]:
            at, so, sl, sg = [], [], [], []
            final = np.zeros(len(asm["snaps"]), np.int64)  # (np.insert: ascending position, stable)
            order = np.argsort([row for row, _ in asm["snaps"]], kind="stable")
            final[order] = np.array([asm["snaps"][j][0] for j in order], np.int64) + np.arange(len(order))
            for k, (row, m) in enumerate(asm["snaps"]):
                slot = d.lookup(int(self.sc.gid[m["g"]]))  # (the host's directory)
                assert slot == self.slot[m["g"]]
                at.append(row)
                so.append(len(blob))
                sl.append(len(m["bytes"]))
                sg.append(slot)
                blob += m["bytes"]
                self.host_rows.append((int(final[k]), HOST, dict(
                    group=slot, info=abi.hb_info(abi.HB_MSG_SNAP, slot_of(m["frm"]), False), term=m["term"],
                    index=m["snap"][0], hint=m["snap"][1])))
            off = np.insert(off, at, np.array(so, np.uint64))
            ln = np.insert(ln, at, np.array(sl, np.uint32))
            grp = np.insert(grp, at, np.array(sg, np.uint32))
        xo, xl, xg = [], [], []
        for g, b, rec in asm["extra"]:
            if rec is not None:
                self.host_rows.append((len(off) + len(xo), LOCAL, dict(rec, group=int(self.slot[g]))))
            xo.append(len(blob))
            xl.append(len(b))
            xg.append(int(self.slot[g]))
            blob += b
        blob += b"\0" * 8
        return (np.concatenate([off, np.array(xo, np.uint64)]), np.concatenate([ln, np.array(xl, np.uint32)]),
                np.concatenate([grp, np.array(xg, np.uint32)]), np.frombuffer(bytes(blob), np.uint8))

    def decode_ref(self, data, off, ln, grp):
        p, n = self.peers_cap()
        return PU.props_reference(data, off, ln, grp, self.C, n, p)

    def host_write(self, dec, ctx):
        """The host's records (MsgSnap, MsgSnapStatus) in their rows of a decoded batch.  The decoder
        must have left each to the host: its status is asserted, and group 0xFFFFFFFF."""
        if not self.host_rows:
            return dec
        out = dict(dec, **{k: dec[k].copy() for k in BATCH})
        for row, st, rec in self.host_rows:
            assert dec["status"][row] == st and dec["group"][row] == M32, \
                f"{ctx}: row {row} for the host decodes with status {dec['status'][row]} group {dec['group'][row]}"
            for k, x in rec.items():
                out[k][row] = x
        return out

    def batch_of(self, dec):
        """The decoded batch in oracle group numbers, sentinel included."""
        inv = self.inverse()
        s = dec["group"].astype(np.int64)
        okslot = s < self.C
        g = np.where(okslot, inv[np.where(okslot, s, 0)], -1)
        b = {k: dec[k] for k in BATCH}
        b["group"] = np.where(g >= 0, g, M32).astype(np.uint32)
        b.update(eoff=dec["eoff"], eterm=dec["eterm"], edesc=dec["edesc"], props=None)
        return b

    # -- the calls -------------------------------------------------------------------------------
    def before(self):
        s = Snap()
        s.groups, s.runs = self.og.groups(), oracle_older_runs(self.og)
        return s

    def step(self, batch, dec, data):
        snap = self.before()
        ev, st = self.og.step(batch)
        self._absorb(snap, ev, batch, dec, data)
        return snap, ev, st

    def tick(self):
        snap = self.before()
        ev, st = self.og.tick(self.draws)
        self.arrivals = {}
        self._absorb(snap, ev, None, None, None)
        return snap, ev, st

    def _absorb(self, snap, ev, batch, dec, data):
        """The host's log store: every entry a decoded MsgApp carried, and this node's own appends
        (a proposal's entries from the decoder's edesc / edata, the empty entry of becomeLeader)."""
        touched, queue = {}, {}
        if batch is not None:
            self.arrivals = {}
            n = len(batch["group"]) - 1
            typ = batch["info"][:n] & 0xF
            gone = set(int(x) for x in ev["x"][(ev["type"] == abi.HB_EV_PROP_FWD) | (ev["type"] == abi.HB_EV_PROP_DROP)])
            raw = data.tobytes()
            eoff, eterm, edesc, edata = dec["eoff"], dec["eterm"], dec["edesc"], dec["edata"]
            for i in np.nonzero((dec["status"] == OK) & (batch["group"][:n] != M32) &
                                ((typ == abi.HB_MSG_APP) | (typ == abi.HB_MSG_PROP)))[0].tolist():
                g = int(batch["group"][i])
                ents = []
                for k in range(int(eoff[i]), int(eoff[i + 1])):
                    d, at = int(edesc[k]), int(edata[k])
                    ents.append((int(eterm[k]), d, raw[at:at + (d & abi.HB_ENT_MAX_DATA)] if d >> 31 else None))
                if typ[i] == abi.HB_MSG_APP:
                    x = int(batch["index"][i])
                    for k, (t, d, p) in enumerate(ents):
                        self.store[(g, x + 1 + k, t)] = (d, p)
                    if ents:
                        touched[g] = min(touched.get(g, x + 1), x + 1)
                else:
                    self.arrivals[i] = ents
                    if i not in gone:
                        queue.setdefault(g, []).append(ents)
        term = {}
        for e in ev[(ev["type"] == abi.HB_EV_TERM) | (ev["type"] == abi.HB_EV_LAST)]:
            g, x = int(e["group"]), int(e["x"])
            if e["type"] == abi.HB_EV_TERM:
                term[g] = x
                continue
            t = term.get(g, int(snap.groups[g]["term"]))
            ents = [(0, 0, None)] if int(e["aux"]) & 1 else queue[g].pop(0)
            lo = x - len(ents) + 1
            for k, (_, d, p) in enumerate(ents):
                self.store[(g, lo + k, t)] = (d, p)
            touched[g] = min(touched.get(g, lo), lo)
        assert not any(queue.values()), "a proposal neither appended, forwarded nor dropped"
        now = self.og.groups()
        assert not now["fault"].any(), f"node {self.v}: oracle fault"
        esz = pyoracle.lib().orc_entry_size
        for g in ev["group"][(ev["type"] == abi.HB_EV_FOLLOW) & (ev["aux"] == abi.HB_FOLLOW_RESTORE)].tolist():
            self.log[g].restart(int(now[g]["first_index"]))  # nothing but the snapshot, then what followed it
            touched[g] = self.log[g].first
            self._bump("restores")
        for g, lo in touched.items():
            log = self.log[g]
            log.cut(lo)
            for i in range(log.next, int(now[g]["last_index"]) + 1):
                t = self.og.term(g, i)
                d, p = self.store[(g, i, t)]
                log.ents.append((t, d, p, int(esz(d, t, i))))
        self.now, self.touched = now, touched
        assert (now["committed"].astype(np.int64) >= self.commit_seen).all(), f"node {self.v}: committed went back"
        self.commit_seen = now["committed"].astype(np.int64)

    def size_of(self, g, i):
        return self.log[g][i][3]

    def compact(self, groups, index):
        """The application compacted `groups` at `index` (with a snapshot): the batch oracle follows,
        and the store drops what lies below the new firstIndex."""
        rc = self.og.compact(np.array(groups, np.uint32), np.array(index, np.uint64), True)
        assert not rc.any(), f"node {self.v}: compaction refused: {rc}"
        self.now = self.og.groups()
        for g, i in zip(groups, index):
            assert (int(self.now[g]["first_index"]), int(self.now[g]["snap_index"])) == (i + 1, i)
            self.log[g].drop_below(i + 1)

    def want(self, snap, ev):
        """The records hb_egress makes of the call (mode 7, both knobs, forwards), by group; the
        flagged ones counted by reason."""
        sc, v = self.sc, self.v
        info = self.og.log_info()
        # (the replays read five fields of every group's record before the call: as plain dicts)
        names = ("term", "last_index", "term_first", "first_index", "committed")
        g0 = [dict(zip(names, row)) for row in zip(*(snap.groups[k].tolist() for k in names))]
        if self.rings is None:
            oldest = ring_oldest(ev, g0, snap.runs, RUN_CAP)
            szlo = {g: int(info[g, 1]) for g in range(self.G)}
        else:  # the rings at the capacities the reserve rule gave them
            oldest = ring_oldest(ev, g0, snap.runs, self.rings.cap_tr)
            szlo = {g: szlo_final(info[g, 1], info[g, 3], self.rings.cap_sz[g]) for g in range(self.G)}
        lim = (self.size_of, szlo) if sc.sized else None
        whole_ev = replay_apps_logterm(ev, g0, snap.runs, self.peers, v, self.og.term, oldest,
                                       max_msg_size=sc.limit, limit=lim, votes=True)
        looked = lookup_sends(ev, g0, snap.runs)
        rewritten = follower_rewrites(ev)
        k = 0
        for r in whole_ev:
            if r[1] not in (abi.HB_MSG_APP, abi.HB_MSG_VOTE):
                continue
            kind = "app" if is_app(r) else "vote"
            self._bump(kind)
            mine = False
            if is_app(r):
                mine = looked[k]
                k += 1
                if mine and not r[11]:
                    self._bump("app_looked_up")
                    if r[12]:
                        self._bump("app_looked_up_ents")
            if r[11]:
                g, x = r[0], r[7]
                if g in rewritten:
                    why = "follower_append"
                elif is_app(r) and mine and (oldest[g] is None or x < oldest[g]):
                    why = "logterm_rule_i"
                elif is_app(r) and sc.sized and x < szlo[g]:
                    why = "limit_rule_i"
                else:
                    raise AssertionError(f"node {v}: record {r} flagged for no documented reason")
                self._bump(f"{kind}_host")
                self._bump(f"{kind}_host_{why}")
        whole = {}
        for r in whole_ev:
            whole.setdefault(r[0], []).append(r)
        per = np.bincount(ev["group"], minlength=self.G) if len(ev) else np.zeros(self.G, np.int64)

        def recs(e):
            if not len(e):
                return []
            g = int(e["group"][0])
            mine = whole.get(g, [])
            if len(e) == per[g]:
                return mine
            return mine[:int(np.isin(e["type"], RECORD_EVENTS).sum())]  # (mode 7: one record per such event)
        return PU.merge_forwards(ev, recs, self.peers, v)

    def snaps_of(self, snap, ev):
        """The HB_EV_SNAP events of a call as [group, to, x, the Term at the send, the records the
        group's earlier events of the call made for that peer], in event order."""
        term, made, out = {}, {}, []
        kinds = RECORD_EVENTS + (abi.HB_EV_PROP_FWD, abi.HB_EV_TERM, abi.HB_EV_SNAP)
        for x, g, t, to, _ in ev[np.isin(ev["type"], kinds)].tolist():
            if t == abi.HB_EV_TERM:
                term[g] = x
            elif t == abi.HB_EV_SNAP:
                out.append([g, int(self.peers[g][to]), x, term.get(g, int(snap.groups[g]["term"])), made.get((g, to), 0)])
            else:
                made[(g, to)] = made.get((g, to), 0) + 1
        return out

    def source(self, snap):
        """hb_ent_source from the store: every entry it holds (from firstIndex on) of every group this
        node led before the call or leads after it, by slot."""
        lead = (snap.groups["state"] == abi.HB_STATE_LEADER) | (self.now["state"] == abi.HB_STATE_LEADER)
        win = {int(self.slot[g]): (self.log[g].first, [((d >> 30) & 1, t, p) for t, d, p, _ in self.log[g].ents])
               for g in np.nonzero(lead)[0].tolist() if self.log[g].ents}
        return build_source(win, self.C)

    # -- send ------------------------------------------------------------------------------------
    def to_slots(self, recs):
        return [(int(self.slot[r[0]]),) + tuple(r[1:]) for r in recs]

    def emit_ref(self, raw, src, seq):
        """hb_egress_bin -> hb_encode_ents -> hb_peer_spans -> hb_frame of the records `raw` (by slot,
        in the device's order), on the CPU."""
        ids = np.array(others(self.v), np.uint64)
        to = np.array([r[3] for r in raw], np.uint64)
        info = np.array([abi.hb_info(r[1], r[2], r[9]) for r in raw], np.uint32)
        order, bin_off = bin_reference(to, info, ids)
        out = [raw[int(j)] for j in order]
        msgs, _, status = encode_ents_reference(out, src)
        for i, r in enumerate(out):
            if r[1] == abi.HB_MSG_PROP:  # hb_encode_ents never covers a proposal
                msgs[i], status[i] = marshal(r), status_of(r)
        off = np.zeros(len(out) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        span = off[bin_off.astype(np.int64)]
        group = np.array([r[0] for r in out], np.uint32)
        index, ispan, fstat = frame.build_index(group, to[order], off, status, bin_off, span, self.gid_col(), self.C,
                                                self.v, seq)
        return dict(order=order, bin_off=bin_off, out=out, msgs=msgs, status=status, off=off, span=span, index=index,
                    ispan=ispan, fstat=fstat, data=b"".join(msgs))

    def reconcile(self, em, a_out, ctx):
        """The independent check: per peer and group, the stream's messages are (A)'s, in r.msgs
        order.  Returns per peer (frame bytes, span bytes, [(row, completed bytes)])."""
        inv = self.inverse()
        bo = em["bin_off"].astype(np.int64)
        assert bo[2] == bo[3], f"{ctx}: a record for no peer"
        res = {}
        for b, peer in enumerate(others(self.v)):
            mine = {}
            for d in a_out:
                if d["to"] == peer:
                    mine.setdefault(d["g"], []).append(d)
            seen, fills = {}, []
            for i in range(bo[b], bo[b + 1]):
                r, st = em["out"][i], int(em["status"][i])
                g = int(inv[r[0]])
                k = seen.get(g, 0)
                seen[g] = k + 1
                assert k < len(mine.get(g, ())), f"{ctx}: to {peer} group {g}: record {k} {r} beyond the reference's messages"
                a = mine[g][k]
                raw = em["data"][int(em["off"][i]):int(em["off"][i + 1])]
                assert (r[1], r[3]) == (a["type"], a["to"]), f"{ctx}: to {peer} group {g} message {k}: {r} for {a}"
                if st == OK:
                    assert raw == a["bytes"], f"{ctx}: to {peer} group {g} message {k}: {raw.hex()} for {a['bytes'].hex()} ({a})"
                    continue
                if st & SPLICE:
                    assert r[1] == abi.HB_MSG_PROP, f"{ctx}: group {g}: a MsgApp the source does not cover: {r}"
                    full = splice(raw, st, [W._entry((0, 0, 0, p)) for _, _, p in self.arrivals[r[10]]])
                    assert full == a["bytes"], f"{ctx}: to {peer} group {g} forward {k}: {full.hex()} for {a['bytes'].hex()}"
                    self._bump("splice_prop")
                else:
                    assert st == HOST and r[11] and raw == b"" and (r[5], r[7]) == (a["term"], a["index"]), \
                        f"{ctx}: to {peer} group {g} message {k}: {r} status {st} for {a}"
                    full = a["bytes"]
                fills.append((i - int(bo[b]), full))
            assert {g: len(m) for g, m in mine.items()} == seen, f"{ctx}: to {peer}: messages missing from the stream"
            isp, sp = em["ispan"].astype(np.int64), em["span"].astype(np.int64)
            res[peer] = (em["index"][isp[b]:isp[b + 1]], em["data"][sp[b]:sp[b + 1]], fills)
        return res

    def random_move(self):
        """move_util.SlotView.random_move on the placement alone: (src, dst)."""
        rng = self.sc.move_rng[self.v]
        k = max(1, self.G // 3)
        who = rng.choice(self.G, k, replace=False)
        src = self.slot[who]
        pool = np.concatenate([src, np.nonzero(self.inverse() < 0)[0]])
        dst = rng.choice(pool, k, replace=False)
        self.slot[who] = dst
        self._bump("moves", int((src != dst).sum()))
        return src, dst


# ---- the rounds -----------------------------------------------------------------------------------
class Cluster:
    """(A) and (B) in lockstep; `device` = a factory (scenario, node, NodeRef) -> GpuNode puts (C)
    in the loop, None runs (B) in its place.  `tamper(what, round, node, phase, obj)` may corrupt the
    device-role output of a decode ("decode"), of a send chain ("send"; in the twin also its "records"),
    the HB_EV_SNAP events the host reads ("snaps") or the entry source it builds ("source"): the
    sensitivity experiment."""

    def __init__(self, sc, device=None, tamper=None):
        self.sc, self.tamper = sc, tamper
        self.A = RefCluster(sc)
        self.B = {v: NodeRef(sc, v, self.A.groups(v)) for v in NODES}
        self.dev = {v: device(sc, v, self.B[v]) for v in NODES} if device is not None else None
        for v in NODES:
            assert np.array_equal(self.B[v].og.groups(), self.A.groups(v)), "the oracle's record of a new group"
        self.flight = {v: [] for v in NODES}    # (sender, phase, frame, span, fills, MsgSnap) on their way to v
        self.a_flight = {v: [] for v in NODES}  # (A)'s messages on their way to v
        self.reports = {v: [] for v in NODES}   # (group, to, lost) of the MsgSnap v handed to its transport
        self.lead_hist, self.commit_hist = [], []
        self.moved_wrapped = 0
        self.round = 0

    def _send(self, v, phase, snap, ev, a_out, ctx):
        b, sc = self.B[v], self.sc
        want = b.want(snap, ev)
        src = b.source(snap)
        seq = 2 * self.round + phase
        if self.tamper is not None:
            self.tamper("source", self.round, v, phase, src)
        if self.dev is None:
            if self.tamper is not None:
                self.tamper("records", self.round, v, phase, want)
            raw = b.to_slots(want)
            em = b.emit_ref(raw, src, seq)
        else:
            em = self.dev[v].send(b, want, src, seq, ctx)
        if self.tamper is not None:
            self.tamper("send", self.round, v, phase, em)
        self._check_snaps(v, phase, snap, ev, a_out, ctx)
        res = b.reconcile(em, [d for d in a_out if not is_snap(d)], ctx)
        for u in others(v):
            snaps = [d for d in a_out if d["to"] == u and is_snap(d)]
            lost = sc.dropped(self.round, phase, v, u)
            self.reports[v] += [(d["g"], u, lost) for d in snaps]  # the transport's ReportSnapshot, a round later
            if lost:
                if snaps:
                    self.A._bump("snap_lost", len(snaps))
                continue
            fr, sp, fills = res[u]
            if len(fr) or snaps:
                self.next_flight[u].append((v, phase, fr if len(fr) else None, sp, fills, snaps))
            self.next_a[u] += [(v, phase, d) for d in a_out if d["to"] == u]

    def _check_snaps(self, v, phase, snap, ev, a_out, ctx):
        """HB_EV_SNAP makes no record: the events (group, to, x) are (A)'s MsgSnap of the call, in
        order per group, and the message the host builds of each (Term of the send, the snapshot's
        term from the log) is (A)'s, byte for byte.  The events also place the MsgSnap in its peer's
        stream: after as many records of the group as (A) sent that peer messages before it."""
        b = self.B[v]
        got = b.snaps_of(snap, ev)
        if self.tamper is not None:
            self.tamper("snaps", self.round, v, phase, got)
        assert self.sc.compacting or not got
        mine, seen = {}, {}
        for i, d in enumerate(a_out):
            if is_snap(d):
                mine.setdefault(d["g"], []).append(d)
                d["before"] = sum(e["g"] == d["g"] and e["to"] == d["to"] and not is_snap(e) for e in a_out[:i])
                if d["before"]:
                    self.A._bump("snap_after_records")
        for g, to, x, term, before in got:
            k = seen.get(g, 0)
            seen[g] = k + 1
            assert k < len(mine.get(g, ())), f"{ctx}: group {g}: HB_EV_SNAP to {to} at {x} beyond the reference's MsgSnap"
            a = mine[g][k]
            assert (to, x, before) == (a["to"], a["snap"][0], a["before"]), \
                f"{ctx}: group {g}: HB_EV_SNAP ({to}, {x}) after {before} records for {a}"
            full = W.gogo_marshal(abi.HB_MSG_SNAP, to=to, frm=v, term=term, snapshot=(SNAP_DATA, NODES, x, b.og.term(g, x)))
            assert full == a["bytes"], f"{ctx}: group {g}: the host's MsgSnap {full.hex()} for {a['bytes'].hex()}"
        assert {g: len(m) for g, m in mine.items()} == seen, f"{ctx}: a MsgSnap of the reference without its HB_EV_SNAP"

    def _compact(self, v, ctx):
        """The application of node v compacts on all three layers."""
        gs, at = self.A.compact(v)
        b = self.B[v]
        b.compact(gs, at)
        if self.dev is not None:
            self.dev[v].compact(b, gs, ctx)
        self._check_state(v, ctx)

    def _check_store(self, v, ctx):
        """Every entry the call put into the node's log store is the registry's: descriptor and bytes."""
        b = self.B[v]
        for g, lo in b.touched.items():
            for i in range(max(lo, b.log[g].first), b.log[g].next):
                t, d, p, _ = b.log[g][i]
                q = self.A.registry.get((g, i, t), b)
                assert q is not b and (d, p) == (desc_of(q), q), f"{ctx}: group {g} entry {i} term {t}: stored {(d, p)}, proposed {q}"

    def _check_state(self, v, ctx):
        a, now = self.A.groups(v), self.B[v].now
        if not np.array_equal(a, now):
            g = int(np.nonzero(a != now)[0][0])
            diff = [(f, a[g][f], now[g][f]) for f in abi.GROUP_DTYPE.names if not np.array_equal(a[g][f], now[g][f])]
            raise AssertionError(f"{ctx}: group {g}: the Raft objects and the batch oracle disagree: {diff}")

    def run_round(self):
        sc, r = self.sc, self.round
        self.next_flight = {v: [] for v in NODES}
        self.next_a = {v: [] for v in NODES}
        for v in NODES:
            b, ctx = self.B[v], f"{sc.name} round {r} node {v} step"
            key = lambda e: (e[0], e[1])  # noqa: E731  (ascending sender, phase 1 before phase 2)
            ems = [(s, fr, sp, fl, sn) for s, _, fr, sp, fl, sn in sorted(self.flight[v], key=key)]
            inbox = [d for _, _, d in sorted(self.a_flight[v], key=key)]
            props = sc.props[r][v]
            reports, self.reports[v] = self.reports[v], []
            a_out = self.A.phase1(v, inbox, props, reports)
            asm = b.assemble(ems, props, reports)
            d = b.directory()
            uf = frame.unframe(asm["index"], asm["frames"], v, d.lookup)
            assert not uf[3].any() and uf[4] == 0, f"{ctx}: fstatus {uf[3]} unknown {uf[4]}"
            if self.dev is not None:
                self.dev[v].unframe(b, asm, uf, ctx)
            off, ln, grp, data = b.rows(asm, uf, d)
            dec = b.decode_ref(data, off, ln, grp)
            mine = np.ones(len(off), bool)
            mine[[row for row, _, _ in b.host_rows]] = False  # (host_write asserts what those decode to)
            bad = np.nonzero((dec["status"] != OK) & (grp != frame.NO_SLOT) & mine)[0]
            assert len(bad) == 0, f"{ctx}: rows {bad[:5]} decode with status {dec['status'][bad[:5]]}"
            patched = b.host_write(dec, ctx)
            batch = b.batch_of(patched)
            if b.rings is not None:
                b.rings.before(batch)
            if self.dev is not None:
                patched = self.dev[v].decode_step(b, data, off, ln, grp, dec, ctx)
            if self.tamper is not None:
                self.tamper("decode", r, v, 0, patched)
            snap, ev, st = b.step(batch, patched, data)
            self._check_store(v, ctx)
            if self.dev is not None:
                self.dev[v].check(b, ev, st, ctx)
            if b.rings is not None:
                b.rings.after(ev)
            self._check_state(v, ctx)
            self._send(v, 0, snap, ev, a_out, ctx)
        for v in NODES:
            b, ctx = self.B[v], f"{sc.name} round {r} node {v} tick"
            a_out = self.A.phase2(v)
            if b.rings is not None:
                b.rings.before(extra=1)
            snap, ev, st = b.tick()
            if self.dev is not None:
                self.dev[v].tick()
                self.dev[v].check(b, ev, st, ctx, stepped=False)
            if b.rings is not None:
                b.rings.after(ev)
            self._check_state(v, ctx)
            self._send(v, 1, snap, ev, a_out, ctx)
        if sc.compacting and r % sc.compact[0] == sc.compact[0] - 1:
            for v in NODES:
                self._compact(v, f"{sc.name} round {r} node {v} compact")
        if sc.moving:
            for v in NODES:
                src, dst = self.B[v].random_move()
                if self.B[v].rings is not None:
                    inv = self.B[v].inverse()
                    self.moved_wrapped += int(self.B[v].rings.wrapped()[inv[dst[src != dst]]].sum())
                if self.dev is not None:
                    self.dev[v].move(src, dst, self.B[v])
        self.flight, self.a_flight = self.next_flight, self.next_a
        self.lead_hist.append(self.A.leaders())
        self.commit_hist.append(self.A.committed())
        self.round += 1

    def run(self):
        for _ in range(self.sc.rounds):
            self.run_round()
        return self

    # -- the end ---------------------------------------------------------------------------------
    def check_end(self):
        sc = self.sc
        for v in NODES:
            b = self.B[v]
            assert not b.now["fault"].any()
            for g in range(sc.G):
                c, first = int(b.now[g]["committed"]), int(b.now[g]["first_index"])
                assert int(b.now[g]["snap_index"]) <= c and b.log[g].first == first
                for i in range(first, c + 1):
                    t, d, p, _ = b.log[g][i]
                    assert (g, i, t) in self.A.registry, f"node {v} group {g}: entry {i} of term {t} is nobody's"
                    q = self.A.registry[(g, i, t)]
                    assert (d, p) == (desc_of(q), q), f"node {v} group {g} entry {i}: {(d, p)} for {q}"
        return self

    def counts(self):
        out = dict(self.A.count)
        for v in NODES:
            for k, n in self.B[v].count.items():
                out["B_" + k] = out.get("B_" + k, 0) + n
        return out


# ---- the scenarios and what they must reach ---------------------------------------------------------
LIMIT = 150
COMPACTING = dict(compact=(2, 4), partition=(1, 7, 22))  # every 2nd round at committed - 4; node 1 cut off a round earlier


def scenario(name, **over):
    """elections: no limit; limited: MaxSizePerMsg 150 with payloads of 0 to 64 bytes, so that limitSize
    cuts and the windows of 8 fill; moving: every node moves a third of its groups after every round.
    All three: 52 rounds, node 1 is cut off for rounds 8 to 21, every frame is lost with probability 0.01, every
    node proposes 1 to 3 entries to half of its groups in every round (followers forward them).
    compacting: limited, and every node compacts every group at committed - 4 after every second round, the
    rings reserved by need before every call; node 1 is cut off from round 7, so that enough probes still go
    below the leaders' boundaries.  compacting_moving: compacting with moving's moves."""
    limited = dict(limit=LIMIT, lens=(None, 0, 1, 7, 16, 33, 64))
    kw = dict(elections={}, limited=limited, moving=dict(moving=True),
              compacting=dict(limited, **COMPACTING), compacting_moving=dict(limited, moving=True, **COMPACTING))[name]
    return Scenario(name, **dict(kw, **over))


def compacting_conditions(c, L, cm, n):
    """What the compacting scenarios must reach beyond the others: the figures first,
    then the conditions on them."""
    sc = c.sc
    p, lo, hi = sc.partition
    followed = np.nonzero((L[lo - 1] != p) & (L[lo - 1] != 0))[0]
    caught = [g for g in followed.tolist() if (g, p) in c.A.snap_groups]
    # a group that got a snapshot has caught up: by the last round every node has passed the highest
    # `committed` any node held at the heal (on top of least_advance, which check_conditions asserts)
    got = sorted({g for g, _ in c.A.snap_groups})
    past = cm[-1][:, got].min(axis=0) - cm[hi - 1][:, got].max(axis=0)
    caps, once, twice, runs = {}, [], [], []
    for v in NODES:
        rg = c.B[v].rings
        last = c.B[v].og.log_info().astype(np.int64)[:, 3]
        once.append(int((last - 1 >= rg.cap_sz).sum()))
        twice.append(int((last - 1 >= 2 * rg.cap_sz).sum()))
        runs.append(int(rg.runs_started.max()))
        for k in zip(rg.cap_sz.tolist(), rg.cap_tr.tolist()):
            caps[k] = caps.get(k, 0) + 1
    f = dict(snap_groups_of_cut_node=len(caught), followed_by_cut_node=len(followed), snap_groups=len(got),
             least_past_the_heal=int(past.min()) if len(got) else 0,
             final_spread=int((cm[-1][:, got].max(axis=0) - cm[-1][:, got].min(axis=0)).max()) if len(got) else 0,
             restored_led=len(c.A.restored_led), capacities=dict(sorted(caps.items())), size_ring_wrapped=once,
             size_ring_wrapped_twice=twice, most_runs_started=runs, moved_wrapped=c.moved_wrapped)
    assert len(caught) >= len(followed) / 2 and len(followed) >= sc.G // 4, f
    assert f["least_past_the_heal"] >= 10, f
    assert n.get("snap_restored", 0) >= 1 and n.get("snap_ignored", 0) >= 1, n
    assert n.get("snap_lost", 0) >= 1 and n.get("snap_status_reject", 0) >= 1, n
    assert n.get("app_at_boundary", 0) >= 1, n
    assert f["restored_led"] >= 1, f
    # The rings wrap, on every node: the size ring of at least half of the groups has passed its
    # capacity, that of a few groups two capacities.  The capacity is each group's own under the
    # reserve rule: the rule adds a call's messages and entries to the span, which keeps every group
    # here above HB_SIZE_RING_MIN / HB_TERM_RING_MIN, and 52 rounds start at most 2 term runs in a
    # group, so no run ring wraps (DESIGN.md §4.1 has the figures).
    assert min(once) >= sc.G / 2 and min(twice) >= 4, f
    if sc.moving:
        assert c.moved_wrapped >= 1, f
    return f


def check_conditions(c):
    """The conditions on a scenario, on the reference alone: liveness, the classes
    of messages reached, the share of records handed to the host.  Returns the figures."""
    sc, n = c.sc, c.counts()
    L, cm = np.array(c.lead_hist), np.array(c.commit_hist)
    p, lo, hi = sc.partition
    assert (L[14] != 0).all(), f"groups without a leader at round 15: {np.nonzero(L[14] == 0)[0]}"
    orphan = L[lo - 1] == p
    again = ((L[lo:hi] != 0) & (L[lo:hi] != p)).any(axis=0)
    assert orphan.sum() >= sc.G // 4 and (again & orphan).sum() >= 0.9 * orphan.sum(), (orphan.sum(), (again & orphan).sum())
    adv = cm[-1] - cm[hi - 1]
    assert (adv >= 10).all(), f"committed after the heal: least advance {adv.min(axis=1)}"
    share = [max(float((L[r] == v).mean()) for r in range(len(L))) for v in NODES]
    assert min(share) >= 0.2, share
    assert n.get("app_resp_reject", 0) >= 30 and n.get("vote_resp_reject", 0) >= 50 and n.get("prop_fwd", 0) >= 1000, n
    assert n.get("B_app_looked_up_ents", 0) >= 100, n
    if sc.sized:
        assert n.get("app_cut", 0) >= 200 and n.get("window_full", 0) >= 1, n
    if sc.moving:
        for v in NODES:
            b = c.B[v]
            assert b.count["moves"] > sc.G and not np.array_equal(b.slot, np.arange(sc.G)) and \
                not np.array_equal(b.slot, sc.perm[v])
    assert n["B_splice_prop"] == n["prop_fwd"] and n["B_app"] == n["app"]
    handed = n.get("B_app_host", 0) + n.get("B_vote_host", 0)
    assert handed <= 0.01 * (n["B_app"] + n["B_vote"]), n
    if sc.compacting:
        n.update(compacting_conditions(c, L, cm, n))
    return dict(n, orphans=int(orphan.sum()), reelected=int((again & orphan).sum()), least_advance=int(adv.min()),
                best_share=[round(x, 2) for x in share], handed_to_host=handed)


# ---- the device chain (GPU tests only; torch is imported where it is used) -----------------------
FILL = 0xAA
_TV = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a.view(_TV[a.dtype])).cuda()


def host(t, dt):
    return t.cpu().numpy().view(dt)


def send_chain(eng, self_id, seq, cap, npeers, gid_col, dsrc=None, bytes_per=91):
    """hb_egress -> hb_egress_bin -> hb_encode[_ents] -> hb_peer_spans -> hb_frame on the engine's
    stream: six calls, no host read between them.  Device tensors."""
    import torch
    t = lambda dt, fill, k=cap: torch.full((max(k, 1),), fill, dtype=dt, device="cuda")  # noqa: E731
    tdt = {"<u4": torch.int32, "<u8": torch.int64}
    raw = {name: t(tdt[dt], -1) for name, dt in abi.OUT_BATCH_FIELDS}
    out = {name: t(tdt[dt], -1) for name, dt in abi.OUT_BATCH_FIELDS}
    count, total = t(torch.int64, -1, 1), t(torch.int64, -1, 1)
    bin_off, span, ispan = t(torch.int64, -1, npeers + 2), t(torch.int64, -1, npeers + 2), t(torch.int64, -1, npeers + 2)
    fstat = t(torch.int32, -1, npeers + 1)
    data, off, status = t(torch.uint8, FILL, cap * bytes_per), t(torch.int64, -1, cap + 1), t(torch.uint8, 0xEE)
    index = t(torch.uint8, FILL, frame.isize(cap) + 64 * npeers)
    eng.egress(self_id, raw, cap, count)
    eng.egress_bin(raw, cap, out, bin_off, n_dev=count)
    if dsrc is None:
        eng.encode(self_id, out, cap, data, off, status, total, n_dev=count)
    else:
        eng.encode_ents(self_id, out, cap, dsrc, data, off, status, total, n_dev=count)
    eng.peer_spans(off, bin_off, span)
    eng.frame(self_id, seq, out, off, status, bin_off, span, gid_col, index, ispan, fstat)
    return dict(raw=raw, out=out, count=count, total=total, bin_off=bin_off, span=span, ispan=ispan, fstat=fstat,
                data=data, off=off, status=status, index=index)


def receive(pair, self_id, ch, peer_bin, sender, d, nrec, ent_cap):
    """One peer's two spans into hb_unframe -> hb_decode_follow -> step_decoded.  The only host reads
    are the four span words a transport needs to ship them."""
    import torch
    sp, isp = host(ch["span"], np.uint64), host(ch["ispan"], np.uint64)
    fr = [(int(isp[peer_bin]), int(isp[peer_bin + 1] - isp[peer_bin]), int(sp[peer_bin]),
           int(sp[peer_bin + 1] - sp[peer_bin]), sender)]
    assert frame.rows(fr[0][1]) == nrec
    full = lambda k, dt: torch.full((max(k, 1),), -0x11111112, dtype=dt, device="cuda")  # noqa: E731
    off, ln, grp = full(nrec, torch.int64), full(nrec, torch.int32), full(nrec, torch.int32)
    fst, unk = full(1, torch.int32), full(1, torch.int64)
    fout = {k: full(nrec + 1, torch.int32 if k in ("group", "info") else torch.int64)
            for k in ("group", "info", "term", "index", "hint", "commit", "eoff")}
    fout["eterm"], fout["edesc"] = full(ent_cap, torch.int64), full(ent_cap, torch.int32)
    edata, n_ent = full(ent_cap, torch.int64), full(1, torch.int64)
    dstatus = torch.full((nrec,), 0xEE, dtype=torch.uint8, device="cuda")
    pair.eng.unframe(self_id, ch["index"], fr, d, len(ch["data"]), off, ln, grp, fst, unk)
    pair.eng.decode_follow(ch["data"], off, ln, grp, fout, dstatus, ent_cap, edata, n_ent)
    pair.eng.step_decoded(fout, ent_cap)
    return dict(off=off, ln=ln, grp=grp, fst=fst, unk=unk, dstatus=dstatus, n_ent=n_ent, frames=fr)


def _same(got, want, what, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{ctx}: {what}: {got.shape} for {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{ctx}: {what} at {bad[:5]}: dev {got[bad[:5]]} expected {want[bad[:5]]}"


class GpuNode:
    """(C): one node's Engine, every group at the node's own slot in a capacity larger than G, with
    every knob of the wire path on.  Each method runs the device's side of one step of a round and
    compares every output with (B)'s."""
    CAP_RECORDS = 4096
    BYTES_PER = 512

    def __init__(self, sc, v, b):
        from etcd_amd.hipbatch import Engine, GidDir
        from .move_util import SlotView
        from .parity_util import assert_groups_equal
        self.sc, self.v, self.GidDir = sc, v, GidDir
        init = b.og.groups()
        self.real = Engine(sc.capacity, max_replicas=3, max_inflight=sc.W, max_msg_size=sc.limit, max_batch=1 << 13)
        self.real.load_groups(init)
        self.view = SlotView(self.real, sc.G)
        self.view.move_slots(np.arange(sc.G), sc.perm[v])  # the node's own placement
        assert np.array_equal(self.view.slot, b.slot)
        peers = np.zeros((sc.capacity, abi.HB_MAX_REPLICAS), np.uint64)
        peers[:, :3] = NODES
        self.real.load_peers(peers)
        self.view.load_timers(b.timers0)
        self.real.set_rand(b.draws)
        if not sc.compacting:
            self.view.reserve_log(np.arange(sc.G), SIZE_CAP if sc.sized else None, RUN_CAP)
        self.real.set_egress(True, votes=True, apps=True)
        self.real.set_egress_logterm(True)
        self.real.set_wire_props(decode=True, egress=True)
        if sc.sized:
            self.real.set_egress_limit(True)
        self.real.set_egress_peers(np.array(others(v), np.uint64))
        assert self.real.egress_mode() == 7 and self.real.wire_props() == 3 and self.real.egress_logterm()
        assert self.real.egress_limit() == sc.sized
        assert_groups_equal(self.view.get_groups(), init, f"node {v} load")
        if sc.compacting:  # the rings are reserved by need before every call: (B) predicts, the engine follows
            b.rings.attach(self.view)
        else:
            self.caps = [self.view.log_capacity(g) for g in range(sc.G)]
            assert all(c[1] >= RUN_CAP for c in self.caps)
        self._dir_for = None

    def close(self):
        self.real.close()

    def directory(self, b):
        """hb_gid_dir_build of the node's id column (again after every move)."""
        import torch
        key = b.slot.tobytes()
        if self._dir_for != key:
            cap = frame.dir_cap(self.sc.capacity)
            d = self.GidDir(torch.full((cap,), -1, dtype=torch.int64, device="cuda"),
                            torch.full((cap,), -1, dtype=torch.int32, device="cuda"), cap)
            dups = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            self.gid_dev = dev(b.gid_col())
            self.real.gid_dir_build(self.gid_dev, d, dups)
            self.real.sync()
            assert int(host(dups, np.uint32)[0]) == 0
            self.dir, self._dir_for = d, key
        return self.dir

    def unframe(self, b, asm, uf, ctx):
        import torch
        n, nfr = asm["nf"], len(asm["frames"])
        d = self.directory(b)
        full = lambda k, dt: torch.full((k,), -7, dtype=dt, device="cuda")  # noqa: E731
        off, ln, grp = full(n + 8, torch.int64), full(n + 8, torch.int32), full(n + 8, torch.int32)
        fst, unk = full(nfr + 1, torch.int32), full(1, torch.int64)
        pad = np.frombuffer(asm["index"] + b"\0" * 8, np.uint8)
        self.real.unframe(self.v, dev(pad), asm["frames"], d, len(asm["data"]), off if n else None, ln if n else None,
                          grp if n else None, fst, unk, n=n, index_size=len(asm["index"]))
        self.real.sync()
        got = (host(off, np.uint64), host(ln, np.uint32), host(grp, np.uint32))
        for a, r, name in zip(got, uf[:3], ("off", "len", "group")):
            _same(a[:n], r, f"hb_unframe {name}", ctx)
            assert (a[n:] == a.dtype.type((1 << 8 * a.itemsize) - 7)).all(), f"{ctx}: hb_unframe {name} past row n"
        _same(host(fst, np.uint32)[:nfr], uf[3], "hb_unframe fstatus", ctx)
        assert int(host(unk, np.uint64)[0]) == uf[4], f"{ctx}: n_unknown"

    def decode_step(self, b, data, off, ln, grp, ref, ctx):
        """hb_decode_follow of the patched rows, compared with the reference, then step_decoded.
        Returns the device's decode on the host: the harness's log store reads it."""
        import torch
        n, ne = len(off), int(ref["n_ent"])
        ent_cap = ne + 8
        fill = lambda k, dt: torch.full((max(k, 1),), -0x1111111111111112 if dt is torch.int64 else -0x11111112,  # noqa: E731
                                        dtype=dt, device="cuda")
        out = {k: fill(n + 1, torch.int32 if k in ("group", "info") else torch.int64) for k in BATCH + ("eoff",)}
        out["eterm"], out["edesc"] = fill(ent_cap, torch.int64), fill(ent_cap, torch.int32)
        edata, n_ent = fill(ent_cap, torch.int64), fill(1, torch.int64)
        status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        self.real.decode_follow(dev(data), dev(off), dev(ln), dev(grp), out, status, ent_cap, edata, n_ent)
        dt = dict(group=np.uint32, info=np.uint32, edesc=np.uint32)
        if b.host_rows:  # the host reads what the decoder left to it and writes its records into those rows
            self.real.sync()
            got = {k: host(out[k], dt.get(k, np.uint64)) for k in out}
            for row, _, rec in b.host_rows:
                for k, x in rec.items():
                    out[k][row:row + 1].copy_(dev(np.array([x], got[k].dtype)))
            torch.cuda.synchronize()  # (the writes are torch's, the step the engine's stream)
        self.real.step_decoded(out, ent_cap)
        self.real.sync()
        if not b.host_rows:
            got = {k: host(out[k], dt.get(k, np.uint64)) for k in out}
        got.update(status=status.cpu().numpy(), edata=host(edata, np.uint64), n_ent=int(host(n_ent, np.uint64)[0]))
        assert got["n_ent"] == ne, f"{ctx}: n_ent {got['n_ent']} expected {ne}"
        _same(got["status"], ref["status"], "hb_decode_follow status", ctx)
        for k in BATCH + ("eoff",):
            _same(got[k][:n + 1], ref[k], f"hb_decode_follow {k}", ctx)
        for k in ("eterm", "edesc", "edata"):
            _same(got[k][:ne], ref[k], f"hb_decode_follow {k}", ctx)
            assert (got[k][ne:].view(np.uint8) == 0xEE).all(), f"{ctx}: {k} written past the entry count"
            got[k] = got[k][:ne]
        return b.host_write(got, ctx)  # (what the device decoded, compared above; then what it stepped)

    def check(self, b, ev, st, ctx, stepped=True):
        """After the step or the tick: events, stats, every group record and timers, and after the step
        the compact words' expansion and the inflight windows, as parity_util.Pair.step / .tick
        compare them."""
        from .parity_util import assert_events_equal, assert_groups_equal, assert_inflights_equal
        dev_ev, dev_st = self.view.events(), self.view.stats()
        if stepped:
            w, counts = self.view.event_words()
            assert np.array_equal(self.view.expand_words(w, counts), dev_ev), f"{ctx}: compact words differ"
        assert_events_equal(dev_ev, ev, ctx)
        assert np.array_equal(dev_st, st), \
            f"{ctx}: stats dev {dict(zip(abi.STAT_NAMES, dev_st.tolist()))} ora {dict(zip(abi.STAT_NAMES, st.tolist()))}"
        assert_groups_equal(self.view.get_groups(), b.now, ctx)
        if stepped:
            assert_inflights_equal(self.view, b.og, b.now, ctx)
        dt, ot = self.view.get_timers(), b.og.timers()
        bad = np.nonzero(dt != ot)[0]
        assert len(bad) == 0, f"{ctx}: timers differ at {bad[:5]}: dev {dt[bad[:3]]} ora {ot[bad[:3]]}"

    def tick(self):
        self.view.tick()

    def send(self, b, want, src, seq, ctx):
        """The send chain against (B): the records by group, then bin offsets, bytes, off, status,
        spans and index frames against the references of the device's own record order."""
        from etcd_amd.hipbatch import EntSource
        from .egress_app_util import out_arrays
        t = {k: dev(src[k] if len(src[k]) else np.zeros(1, src[k].dtype)) for k in
             ("first", "count", "start", "eterm", "edesc", "edata", "data")}
        dsrc = EntSource(t["first"], t["count"], t["start"], t["eterm"], t["edesc"], t["edata"], t["data"],
                         n_ent=len(src["edesc"]), data_len=len(src["data"]))
        self.directory(b)
        cap = self.CAP_RECORDS
        ch = send_chain(self.real, self.v, seq, cap, 2, self.gid_dev, dsrc=dsrc, bytes_per=self.BYTES_PER)
        self.real.sync()
        n, total = int(ch["count"].item()), int(ch["total"].item())
        assert n == len(want), f"{ctx}: {n} records, expected {len(want)}"
        assert n <= cap and total <= cap * self.BYTES_PER, f"{ctx}: the chain's buffers are too small ({n}, {total})"
        raw = {name: host(ch["raw"][name], dt) for name, dt in abi.OUT_BATCH_FIELDS}
        inv = b.inverse()
        grp = inv[np.minimum(raw["group"][:n].astype(np.int64), b.C - 1)]
        assert (raw["group"][:n] < b.C).all() and (grp >= 0).all(), f"{ctx}: a record of an empty slot"
        order = np.argsort(grp, kind="stable")
        exp = out_arrays(want)
        _same(grp[order], exp["group"], "hb_egress group", ctx)
        for name, _ in abi.OUT_BATCH_FIELDS[1:]:
            _same(raw[name][:n][order], exp[name], f"hb_egress {name}", ctx)
        for name, _ in abi.OUT_BATCH_FIELDS:
            assert (raw[name][n:].view(np.int64 if raw[name].itemsize == 8 else np.int32) == -1).all(), f"{ctx}: {name} past n"
        ref = b.emit_ref(records_of(raw, n, self.v), src, seq)
        _same(host(ch["bin_off"], np.uint64)[:4], ref["bin_off"], "hb_egress_bin bin_off", ctx)
        binned = {name: host(ch["out"][name], dt) for name, dt in abi.OUT_BATCH_FIELDS}
        for name, _ in abi.OUT_BATCH_FIELDS:
            _same(binned[name][:n], raw[name][:n][ref["order"]], f"hb_egress_bin {name}", ctx)
        off, status = host(ch["off"], np.uint64), ch["status"].cpu().numpy()
        _same(off[:n + 1], ref["off"], "hb_encode_ents off", ctx)
        _same(status[:n], ref["status"], "hb_encode_ents status", ctx)
        assert total == len(ref["data"]), f"{ctx}: total {total} expected {len(ref['data'])}"
        data = ch["data"].cpu().numpy()
        if data[:total].tobytes() != ref["data"]:
            i = next(k for k in range(n) if data[int(off[k]):int(off[k + 1])].tobytes() != ref["msgs"][k])
            raise AssertionError(f"{ctx}: bytes of binned record {i} {ref['out'][i]}: "
                                 f"{data[int(off[i]):int(off[i + 1])].tobytes().hex()} expected {ref['msgs'][i].hex()}")
        assert (data[total:] == FILL).all(), f"{ctx}: bytes written past total"
        _same(host(ch["span"], np.uint64)[:4], ref["span"], "hb_peer_spans", ctx)
        _same(host(ch["ispan"], np.uint64)[:4], ref["ispan"], "hb_frame ispan", ctx)
        _same(host(ch["fstat"], np.uint32)[:3], ref["fstat"], "hb_frame fstat", ctx)
        index = ch["index"].cpu().numpy()
        ni = len(ref["index"])
        assert index[:ni].tobytes() == ref["index"], f"{ctx}: index frames differ"
        assert (index[ni:] == FILL).all(), f"{ctx}: index bytes written past the frames"
        # what travels on is the device's own output
        return dict(order=ref["order"], bin_off=host(ch["bin_off"], np.uint64)[:4].copy(),
                    out=records_of(binned, n, self.v), msgs=ref["msgs"], status=status[:n].copy(), off=off[:n + 1].copy(),
                    span=host(ch["span"], np.uint64)[:4].copy(), index=index[:ni].tobytes(),
                    ispan=host(ch["ispan"], np.uint64)[:4].copy(), fstat=ref["fstat"], data=data[:total].tobytes())

    def move(self, src, dst, b):
        self.view.move_slots(src, dst)
        assert np.array_equal(self.view.slot, b.slot)

    def compact(self, b, groups, ctx):
        """hb_set_log_bounds of the groups (B) just compacted, from its records."""
        from .parity_util import assert_groups_equal
        if len(groups):
            gs = np.array(groups, np.uint32)
            self.view.set_log_bounds(gs, b.now["first_index"][gs], b.now["snap_index"][gs])
        assert_groups_equal(self.view.get_groups(), b.now, ctx)

    def check_end(self, b):
        if self.sc.compacting:
            b.rings.check_capacity(f"node {self.v} end")
            return
        for g in range(self.sc.G):
            assert self.view.log_capacity(g) == self.caps[g], f"group {g}: a ring was regrown"
