"""Parity under log compaction: Pair / OraclePair variants whose application
compacts its Storage (MemoryStorage.CreateSnapshot + Compact, raft/storage.go:
172-214 -> hb_set_log_bounds) and which reserve the two log-index rings by
libhbnode's rule (want_log() in hbnode.cpp) without its doubling: the span
[firstIndex - 1, max(lastIndex, top)] plus what the batch adds, and the runs of
that span.  A group that compacts as it appends therefore stays on rings of
fixed capacity that wrap and drop what lies below firstIndex - 1, and every
lookup the reference can make is still answered."""
import numpy as np

from etcd_amd import abi, synth

from .move_util import MovedPair
from .parity_util import OraclePair, Pair, assert_groups_equal


def pow2ceil(x):
    x = np.maximum(np.asarray(x, dtype=np.int64), 1)
    return (1 << np.ceil(np.log2(x)).astype(np.int64)).astype(np.int64)


def trim_runs(runs, lo):
    """A group's log term runs [(index, term), ...] with everything below index
    `lo` cut off: `lo` becomes the dummy entry and keeps its term."""
    k = max(i for i, r in enumerate(runs) if int(r[0]) <= lo)
    return [(lo, int(runs[k][1]))] + [(int(i), int(t)) for i, t in runs[k + 1:]]


def batch_adds(batch, G, extra=0):
    """Per group, what a step can append (`add`: the entries of its MsgProps /
    props / MsgApps and one noop or new term run per message) and the highest
    index a MsgApp of it reaches (`top`, 0 where none) -- Pair.reserve's sums."""
    add = np.full(G, extra, dtype=np.int64)
    top = np.zeros(G, dtype=np.int64)
    if batch is not None and len(batch["group"]):
        grp = np.asarray(batch["group"], dtype=np.int64)
        ok = grp < G
        add += np.bincount(grp[ok], minlength=G)[:G]
        t = np.asarray(batch["info"]) & 0xF
        idx = np.asarray(batch["index"], dtype=np.int64)
        prop = ok & (t == abi.HB_MSG_PROP)
        add += np.bincount(grp[prop], weights=idx[prop], minlength=G)[:G].astype(np.int64)
        if batch.get("eterm") is not None and batch.get("eoff") is not None:
            eoff = np.asarray(batch["eoff"], dtype=np.int64)
            ne = np.diff(np.append(eoff, len(batch["eterm"])))
            app = ok & (t == abi.HB_MSG_APP)
            add += np.bincount(grp[app], weights=ne[app], minlength=G)[:G].astype(np.int64)
            np.maximum.at(top, grp[app], idx[app] + ne[app])
    if batch is not None and batch.get("props") is not None:
        add += np.asarray(batch["props"], dtype=np.int64)[:G]
    return add, top


class _Compacting:
    """The bookkeeping both variants share (self.og, self.sized, self.gpu)."""

    def _start(self, sizes, term_runs, hold=False):
        G = self.G = self.og.G
        self.hold = hold  # scenario 6: a caller that never reserves
        self.cap_sz = np.full(G, abi.HB_SIZE_RING_MIN if self.sized else 0, dtype=np.int64)
        self.cap_tr = np.full(G, abi.HB_TERM_RING_MIN, dtype=np.int64)
        for g, z in (sizes or {}).items():  # hb_load_entry_sizes: the base entry plus n sizes
            self.cap_sz[g] = max(self.cap_sz[g], int(pow2ceil(len(z) + 1)))
        for g, rr in (term_runs or {}).items():  # hb_load_term_runs: n runs plus one
            self.cap_tr[g] = max(self.cap_tr[g], int(pow2ceil(len(rr) + 1)))
        self.appended = np.zeros(G, dtype=np.int64)       # entries appended since load
        self.runs_started = np.zeros(G, dtype=np.int64)   # term runs started since load
        self.ev_count = np.zeros((G, 16), dtype=np.int64)     # events by type
        self.fault_count = np.zeros((G, 16), dtype=np.int64)  # faults by code
        self.follow_count = np.zeros((G, 16), dtype=np.int64)  # HB_EV_FOLLOW by aux
        self.resp_count = np.zeros((G, 16), dtype=np.int64)    # HB_EV_RESP by aux
        self.steps = 0

    def needs(self, batch=None, extra=0):
        info = self.og.log_info().astype(np.int64)  # runs, sz_lo, first, last
        add, top = batch_adds(batch, self.G, extra)
        need_sz = np.maximum(info[:, 3], top) + add - (info[:, 2] - 1) + 1
        need_tr = info[:, 0] + add + 1
        return need_sz, need_tr

    def reserve(self, batch=None, extra=0):
        if self.hold:
            return
        need_sz, need_tr = self.needs(batch, extra)
        grow = need_tr > self.cap_tr
        if self.sized:
            grow |= need_sz > self.cap_sz
        if grow.any():
            gs = np.nonzero(grow)[0]
            if self.sized:
                self.cap_sz[gs] = np.maximum(self.cap_sz[gs], pow2ceil(need_sz[gs]))
            self.cap_tr[gs] = np.maximum(self.cap_tr[gs], pow2ceil(need_tr[gs]))
            if self.gpu:
                self.eng.reserve_log(gs.astype(np.uint32), need_sz[gs] if self.sized else None, need_tr[gs])

    def _before(self):
        info = self.og.log_info().astype(np.int64)
        return info[:, 0].copy(), info[:, 3].copy()

    def _after(self, before, ev):
        runs0, last0 = before
        info = self.og.log_info().astype(np.int64)
        self.appended += np.maximum(info[:, 3] - last0, 0)
        self.runs_started += np.maximum(info[:, 0] - runs0, 0)
        np.add.at(self.ev_count, (ev["group"].astype(np.int64), ev["type"].astype(np.int64) & 15), 1)
        f = ev[ev["type"] == abi.HB_EV_FAULT]
        np.add.at(self.fault_count, (f["group"].astype(np.int64), f["aux"].astype(np.int64) & 15), 1)
        f = ev[ev["type"] == abi.HB_EV_FOLLOW]
        np.add.at(self.follow_count, (f["group"].astype(np.int64), f["aux"].astype(np.int64) & 15), 1)
        f = ev[ev["type"] == abi.HB_EV_RESP]
        np.add.at(self.resp_count, (f["group"].astype(np.int64), f["aux"].astype(np.int64) & 15), 1)
        self.steps += 1
        if self.steps % 8 == 0:
            self.check_capacity(f"step {self.steps}")

    def check_capacity(self, ctx=""):
        """hb_log_capacity is what the host predicts: max(HB_*_RING_MIN, pow2ceil(max need so far))."""
        if not self.gpu:
            return
        for g in range(self.G):
            want = (int(self.cap_sz[g]), int(self.cap_tr[g]))
            got = self.eng.log_capacity(g)
            assert got == want, f"{ctx}: g{g} log capacity {got}, predicted {want}"

    def raise_capacity(self, groups, size_cap, run_cap):
        """hb_reserve_log beyond the need (the prediction follows)."""
        groups = np.asarray(groups, dtype=np.int64)
        if self.sized:
            self.cap_sz[groups] = np.maximum(self.cap_sz[groups], pow2ceil(size_cap))
        self.cap_tr[groups] = np.maximum(self.cap_tr[groups], pow2ceil(run_cap))
        if self.gpu:
            self.eng.reserve_log(groups.astype(np.uint32), size_cap if self.sized else None, run_cap)

    def reload(self, g, record, runs, sizes, term_runs):
        """Group g's slot is removed and takes a fresh group: its log index restarts
        (szlo, trc) in the extents the slot already owns."""
        self.og.reload(g, record, runs)
        if sizes:
            self.og.load_sizes({g: sizes})
        self.og.load_term_runs({g: term_runs})
        if self.gpu:
            real = getattr(self.eng, "real", self.eng)
            slot = int(self.eng.slot[g]) if hasattr(self.eng, "slot") else g
            real.remove_groups(slot, 1)
            real.load_groups(self.og.groups()[g:g + 1], first=slot)
            if sizes:
                real.load_entry_sizes({slot: sizes})
            real.load_term_runs({slot: term_runs})
        if sizes:
            self.cap_sz[g] = max(self.cap_sz[g], int(pow2ceil(len(sizes) + 1)))
        self.cap_tr[g] = max(self.cap_tr[g], int(pow2ceil(len(term_runs) + 1)))
        self.appended[g] = self.runs_started[g] = 0

    def swap(self, a, b):
        """Groups a[i] and b[i] trade slots (hb_move_groups); a no-op without an engine."""
        if self.gpu:
            sa, sb = self.eng.slot[np.asarray(a)].copy(), self.eng.slot[np.asarray(b)].copy()
            self.eng.move_slots(np.concatenate([sa, sb]), np.concatenate([sb, sa]))

    def compact(self, groups, index, snap=True, ctx="compact"):
        """The application compacts groups[k] at index[k] on both sides."""
        groups = np.asarray(groups, dtype=np.uint32)
        rc = self.og.compact(groups, index, snap)
        now = self.og.groups()
        if self.gpu and len(groups):
            self.eng.set_log_bounds(groups, now["first_index"][groups], now["snap_index"][groups])
            assert_groups_equal(self.eng.get_groups(), now, ctx)
        return rc, now


class CompactPair(_Compacting, Pair):
    def __init__(self, groups, runs, nmax, W, hold=False, **kw):
        Pair.__init__(self, groups, runs, nmax, W, **kw)
        tr = kw.get("term_runs")
        if tr is True:
            tr = synth.older_runs(self.og.groups(), runs)
        self._start(kw.get("sizes"), tr, hold)
        self.check_capacity("load")

    def step(self, batch, ctx="", check_inflights=True):
        b4 = self._before()
        out = Pair.step(self, batch, ctx, check_inflights)
        self._after(b4, out[0])
        return out


class MovedCompactPair(_Compacting, MovedPair):
    """CompactPair over an engine with spare slots whose groups can be moved
    (tests/move_util.py): capacities are kept per group, so a check after a move
    says that hb_log_capacity followed the groups."""

    def __init__(self, groups, runs, nmax, W, hold=False, spare=40, **kw):
        MovedPair.__init__(self, groups, runs, nmax, W, len(groups) + spare, **kw)
        tr = kw.get("term_runs")
        if tr is True:
            tr = synth.older_runs(self.og.groups(), runs)
        self._start(kw.get("sizes"), tr, hold)
        self.check_capacity("load")

    def step(self, batch, ctx="", check_inflights=True):
        b4 = self._before()
        out = Pair.step(self, batch, ctx, check_inflights)
        self._after(b4, out[0])
        return out


class OracleCompactPair(_Compacting, OraclePair):
    def __init__(self, groups, runs, nmax, W, hold=False, **kw):
        OraclePair.__init__(self, groups, runs, nmax, W, **kw)
        self.sized = kw.get("max_msg_size", abi.HB_NO_LIMIT) not in (0, abi.HB_NO_LIMIT)
        tr = kw.get("term_runs")
        if tr is True:
            tr = synth.older_runs(self.og.groups(), runs)
        self._start(kw.get("sizes"), tr, hold)

    def step(self, batch, ctx="", check_inflights=True):
        self.reserve(batch)
        b4 = self._before()
        ev, st = self.og.step(batch)
        self._after(b4, ev)
        return ev, st, self.og.groups()
