"""Parity harness for hb_move_groups: the oracle cannot move groups, so the
harness keeps the permutation (oracle group -> engine slot) and shows the
engine to parity_util.Pair through a view that speaks oracle group numbers.

SlotView translates on the way in (batch["group"], the dense props / peoff
arrays laid out by slot, timers, hb_reserve_log's group list) and on the way
out (events, group records, timers, inflight windows), so Pair.step / Pair.tick
and their assert helpers compare against the unmodified oracle as they are.
"""
import numpy as np

from etcd_amd import abi
from oracle.pyoracle import OracleGroups
from tests.parity_util import Pair, assert_groups_equal


class SlotView:
    """An Engine of `capacity` slots seen as the G oracle groups (slot[g] = the
    slot of oracle group g)."""

    def __init__(self, eng, G):
        self.real = eng
        self.G = G
        self.C = eng.capacity
        self.slot = np.arange(G, dtype=np.int64)  # groups are loaded at their own number

    # ---- the permutation ------------------------------------------------------
    def inverse(self):
        inv = np.full(self.C, -1, dtype=np.int64)
        inv[self.slot] = np.arange(self.G)
        return inv

    def free_slots(self):
        return np.nonzero(self.inverse() < 0)[0]

    def move_slots(self, src, dst):
        """hb_move_groups(src, dst) and the same on the permutation (a live dst
        outside src is lost: the parity tests never do that)."""
        src = np.asarray(src, dtype=np.int64)
        dst = np.asarray(dst, dtype=np.int64)
        inv = self.inverse()
        who = inv[src]
        lost = np.setdiff1d(dst, src)
        assert (inv[lost] < 0).all(), "move_slots would overwrite a live group"
        self.real.move_groups(src.astype(np.uint32), dst.astype(np.uint32))
        live = who >= 0
        self.slot[who[live]] = dst[live]

    def random_move(self, rng, frac=1 / 3):
        """Move a random `frac` of the groups to a random arrangement of their
        own slots and the free ones: swaps, cycles, chains into empty slots and
        identity pairs all occur."""
        k = max(1, int(self.G * frac))
        who = rng.choice(self.G, k, replace=False)
        src = self.slot[who]
        pool = np.concatenate([src, self.free_slots()])
        dst = rng.choice(pool, k, replace=False)
        self.move_slots(src, dst)
        return src, dst

    # ---- in -------------------------------------------------------------------
    def _by_slot(self, a, dtype):
        out = np.zeros(self.C, dtype=dtype)
        out[self.slot] = np.asarray(a)[: self.G]
        return out

    def xlate(self, batch):
        b = dict(batch)
        grp = np.asarray(batch["group"], dtype=np.int64)
        ok = grp < self.G
        out = np.where(ok, self.slot[np.where(ok, grp, 0)], grp - self.G + self.C)  # out of range stays so
        b["group"] = np.minimum(out, 0xFFFFFFFF).astype(np.uint32)
        if batch.get("props") is not None:
            b["props"] = self._by_slot(batch["props"], np.uint32)
        if batch.get("peoff") is not None:
            b["peoff"] = self._by_slot(batch["peoff"], np.uint64)
        return b

    def step_batch(self, batch, **kw):
        return self.real.step_batch(self.xlate(batch), **kw)

    def reserve_log(self, groups, size_cap=None, run_cap=None):
        return self.real.reserve_log(self.slot[np.asarray(groups, dtype=np.int64)].astype(np.uint32), size_cap, run_cap)

    def set_log_bounds(self, groups, first_index, snap_index):
        return self.real.set_log_bounds(self.slot[np.asarray(groups, dtype=np.int64)].astype(np.uint32), first_index,
                                        snap_index)

    def log_capacity(self, g):
        return self.real.log_capacity(int(self.slot[g]))

    def load_timers(self, timers):
        t = self.real.get_timers()
        t[self.slot] = timers
        self.real.load_timers(t)

    def set_rand(self, draws, first=0):
        return self.real.set_rand(draws, first)

    def tick(self):
        return self.real.tick()

    # ---- out ------------------------------------------------------------------
    def _events_back(self, ev):
        ev = ev.copy()
        g = self.inverse()[ev["group"]]
        assert (g >= 0).all(), "an event names a slot that holds no group"
        ev["group"] = g.astype(np.uint32)
        return ev

    def events(self):
        return self._events_back(self.real.events())

    def event_words(self):
        return self.real.event_words()

    def expand_words(self, words, counts):
        return self._events_back(self.real.expand_words(words, counts))

    def stats(self):
        return self.real.stats()

    def get_groups(self):
        """The groups in oracle order; every other slot must be empty (n = 0)."""
        allg = self.real.get_groups()
        rest = np.ones(self.C, dtype=bool)
        rest[self.slot] = False
        assert (allg["n"][rest] == 0).all(), f"slots {np.nonzero(rest & (allg['n'] != 0))[0][:5]} should be empty"
        return allg[self.slot]

    def get_timers(self):
        return self.real.get_timers()[self.slot]

    def get_inflights(self, g, s):
        return self.real.get_inflights(int(self.slot[g]), s)


class MovedPair(Pair):
    """parity_util.Pair over an engine of `capacity` >= len(groups) slots whose
    groups can be moved (self.eng is a SlotView; self.view.random_move / move_slots)."""

    def __init__(self, groups, runs, nmax, W, capacity, ins=None, max_msg_size=abi.HB_NO_LIMIT, max_batch=1 << 16,
                 sizes=None, term_runs=None):
        from etcd_amd.hipbatch import Engine
        G = len(groups)
        assert capacity >= G
        self.og = OracleGroups(groups, runs, W, max_msg_size, ins)
        init = self.og.groups()
        real = Engine(capacity, max_replicas=nmax, max_inflight=W, max_msg_size=max_msg_size, max_batch=max_batch)
        real.load_groups(init)  # slots 0 .. G-1: the permutation starts as the identity
        for (g, s), vals in (ins or {}).items():
            real.set_inflights(g, s, int(init[g]["pr"][s]["ins_start"]), vals)
        self.sized = max_msg_size not in (0, abi.HB_NO_LIMIT)
        if sizes:
            self.og.load_sizes(sizes)
            real.load_entry_sizes(sizes)
        if term_runs:
            if term_runs is True:
                from etcd_amd import synth
                term_runs = synth.older_runs(init, runs)
            self.og.load_term_runs(term_runs)
            real.load_term_runs(term_runs)
        self.view = self.eng = SlotView(real, G)
        assert_groups_equal(self.eng.get_groups(), init, "load")
