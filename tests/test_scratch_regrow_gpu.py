"""GPU tests of the engine's on-demand scratch (host memory): every
buffer a call allocates lazily or grows is taken through small -> large ->
small on one handle, and every result is compared element-wise with a fresh
handle that makes only that call.  A buffer that came back too small, kept a
stale pointer or lost its contents (hb_set_rand keeps the earlier draws) shows
as a difference; the last test watches free device memory over 32 handles.

G = 600 (three partitions: two full, one ragged), three replicas.  The batch
limit is 4,096 except for the two decode tests: hb_decode_follow takes
n + 1 <= max_batch records and the regrowth there has to pass DECF_SMALL_MAX
(16,384), the size at which it leaves the one-workgroup path, so those handles
take 32,768.  Steps of one handle touch disjoint groups (or every handle replays
the same deterministic steps), so a fresh handle sees the state the veteran saw.
Host-pointer batches of these sizes travel packed through the pinned block
(hstage / dstage); the per-array staging of s_edesc / s_eterm starts at 8 MiB a
batch and is not reached here.  All inputs are valid.
"""
import functools

import numpy as np
import pytest

from etcd_amd import abi, synth

from . import wire_util as W
from .parity_util import sort_events

pytestmark = pytest.mark.gpu

G, N, W8, MB = 600, 3, 8, 4096
DECF_SMALL_MAX = ENC_SMALL_MAX = 16384
ALL = np.arange(G, dtype=np.uint32)


def _peers():
    p = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    p[:, :N] = np.arange(1, N + 1, dtype=np.uint64)
    return p


def _engine(groups, max_batch=MB):
    """A handle with `groups` loaded, peer rows 1..3 and room in every log-index ring for
    what these tests append (hb_reserve_log: the device never grows a ring)."""
    from etcd_amd.hipbatch import Engine
    eng = Engine(G, max_replicas=N, max_inflight=W8, max_batch=max_batch)
    eng.load_groups(groups)
    eng.load_peers(_peers())
    eng.reserve_log(ALL, None, 128)
    return eng


def _events_both_ways(eng, ctx):
    """events() and events_to_host of the last step: the same stream; returned sorted by group."""
    ev = eng.events()
    words, counts = eng.event_words()
    assert np.array_equal(eng.expand_words(words, counts), ev), f"{ctx}: compact words differ from events()"
    return sort_events(ev)


# ---- decode / decode_follow: dec_q, dec_qn, decf_sum, decf_base ----------------------------------
@functools.lru_cache(maxsize=None)
def _corpus(n):
    from .test_ingest_gpu import _mix
    data, off, ln = W.pack(_mix(n, salt=n))
    return data, off, ln, (np.arange(n) % (G + 1)).astype(np.uint32)  # (one group past the capacity too)


DEC_SIZES = (64, DECF_SMALL_MAX + 1, 64)


@functools.lru_cache(maxsize=None)
def _steady():
    return synth.steady_groups(G, N, seed=3, with_runs=False)[0]


def _same(a, b, ctx):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{ctx}: {k} differs from the fresh handle's"


def test_decode_follow_regrows():
    """n = 64 (one-workgroup path), 16,385 (tiled path; dec_q and decf_* regrow), 64 again."""
    import torch
    from .test_ingest_gpu import _decode
    vet = _engine(_steady(), 1 << 15)
    for k, n in enumerate(DEC_SIZES):
        data, off, ln, grp = _corpus(n)
        cap = int(ln.astype(np.uint64).sum()) // 8
        fresh = _engine(_steady(), 1 << 15)
        _, want = _decode(fresh, torch, data, off, ln, grp, cap)
        fresh.close()
        _, got = _decode(vet, torch, data, off, ln, grp, cap)
        assert want["n_ent"] > 0 and (want["status"][:n] == abi.HB_WIRE_OK).sum() > n // 2
        _same(got, want, f"decode_follow call {k} n={n}")
    vet.close()


def _decode_plain(eng, torch, data, off, ln, grp):
    from .test_ingest_gpu import _dev
    n = len(off)
    out = {k: torch.full((n,), -0x11111112, dtype=torch.int32 if k in ("group", "info") else torch.int64, device="cuda")
           for k in ("group", "info", "term", "index", "hint")}
    status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.decode(_dev(torch, data), _dev(torch, off), _dev(torch, ln), _dev(torch, grp), out, status)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host["status"] = status.cpu().numpy()
    return host


def test_decode_regrows():
    import torch
    vet = _engine(_steady(), 1 << 15)
    for k, n in enumerate(DEC_SIZES):
        data, off, ln, grp = _corpus(n)
        fresh = _engine(_steady(), 1 << 15)
        want = _decode_plain(fresh, torch, data, off, ln, grp)
        fresh.close()
        assert (want["status"] == abi.HB_WIRE_OK).sum() > n // 8
        _same(_decode_plain(vet, torch, data, off, ln, grp), want, f"decode call {k} n={n}")
    vet.close()


# ---- step with host pointers and entry columns; events() and events_to_host after each ---------
@functools.lru_cache(maxsize=None)
def _followers():
    return synth.follow_groups(G, N, seed=11, last_hi=1 << 16, with_runs=False)[0]


def _follow_slice(lo, hi, ents):
    """The leader's MsgApp (`ents` entries) and MsgHeartbeat for the groups lo .. hi - 1."""
    b = synth.follow_batch(_followers()[lo:hi], 0, seed=lo, ents=ents)
    b["group"] = (b["group"] + np.uint32(lo)).astype(np.uint32)
    return b


def test_host_step_and_events_regrow():
    """n_edesc 16, 3,408 and 16 on disjoint groups: the packed staging, then the expansion
    scratch of events() (evx) and the word scan of events_to_host (evw) after each step."""
    vet = _engine(_followers())
    for k, (lo, hi, ents) in enumerate([(0, 16, 1), (16, 584, 6), (584, 600, 1)]):
        b = _follow_slice(lo, hi, ents)
        assert len(b["eterm"]) == (hi - lo) * ents
        fresh = _engine(_followers())
        fresh.step_batch(b, host=True)
        want_ev, want_g = _events_both_ways(fresh, f"fresh {k}"), fresh.get_groups()
        fresh.close()
        vet.step_batch(b, host=True)
        got_ev = _events_both_ways(vet, f"veteran {k}")
        assert len(want_ev) >= 2 * (hi - lo)
        assert np.array_equal(got_ev, want_ev), f"step {k}: events differ from the fresh handle's"
        assert vet.get_groups()[lo:hi].tobytes() == want_g[lo:hi].tobytes(), f"step {k}: groups differ"
        assert (want_g["last_index"][lo:hi] == _followers()["last_index"][lo:hi] + np.uint64(ents)).all()
    vet.close()


# ---- set_rand: the table grows and keeps the earlier draws --------------------------------------
def test_set_rand_keeps_earlier_draws():
    draws = np.random.default_rng(5).integers(0, 1 << 63, 4008, dtype=np.uint64)
    timers = synth.random_timers(G, seed=6, et_hi=4, pos_hi=4000)  # rand positions all over the table,
    timers["rand_pos"][::2] = np.arange(0, G, 2) % 8               # half of them in the part that was copied
    res = []
    for pieces in ([(0, 8), (8, 4008)], [(0, 4008)]):
        eng = _engine(_followers())
        eng.load_timers(timers)
        for lo, hi in pieces:
            eng.set_rand(draws[lo:hi], first=lo)
        eng.tick()
        res.append((sort_events(eng.events()), eng.get_groups(), eng.get_timers()))
        eng.close()
    (ev_a, g_a, t_a), (ev_b, g_b, t_b) = res
    assert (g_b["state"] == abi.HB_STATE_CANDIDATE).sum() > G // 8  # campaigns drew new timeouts
    assert (t_b["rand_pos"] != timers["rand_pos"]).sum() > G // 8
    assert np.array_equal(ev_a, ev_b) and g_a.tobytes() == g_b.tobytes() and t_a.tobytes() == t_b.tobytes()


# ---- move_groups: mv_in, mv_stage, mv_jobs, mv_rstage ------------------------------------------
def _move_engine():
    from oracle.pyoracle import OracleGroups
    g, runs, ins = synth.random_groups(G, N, seed=17, W=W8)
    g = OracleGroups(g, runs, W8, abi.HB_NO_LIMIT, ins).groups()
    eng = _engine(g)
    for (gi, s), vals in ins.items():
        eng.set_inflights(gi, s, int(g[gi]["pr"][s]["ins_start"]), vals)
    eng.load_term_runs(synth.older_runs(g, runs))
    eng.load_timers(synth.random_timers(G, seed=18))
    return eng, len(ins)


def _slots_state(eng, slots):
    g, t = eng.get_groups(), eng.get_timers()
    ins = [eng.get_inflights(int(s), k) for s in slots[::3] for k in range(N)]  # (every third slot's windows)
    return (g[slots].tobytes(), t[slots].tobytes(), [eng.log_capacity(int(s)) for s in slots],
            [(a, b.tolist()) for a, b in ins])


def test_move_groups_regrows():
    """4, 300 and 4 slots, each set permuted among itself (a rotation by one: one cycle)."""
    vet, n_ins = _move_engine()
    assert n_ins > 50  # inflight windows travel: mv_rstage is used
    for k, (lo, hi) in enumerate([(0, 4), (100, 400), (500, 504)]):
        src = np.arange(lo, hi, dtype=np.uint32)
        dst = np.roll(src, 1)
        fresh, _ = _move_engine()
        before = _slots_state(fresh, src)
        fresh.move_groups(src, dst)
        want = _slots_state(fresh, dst)
        fresh.close()
        assert want == before and _slots_state(vet, src) == before
        vet.move_groups(src, dst)
        assert _slots_state(vet, dst) == want, f"move {k}: slots differ from the fresh handle's"
    vet.close()


# ---- set_egress: the snapshot columns of each mode come and go ----------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    return synth.mixed_groups(G, N, seed=0x5EED0007, last_hi=1 << 12, with_runs=False)[0]


MODES = [None, (), ("votes",), ("apps",), ("votes",), None, ("apps",)]  # off, on, votes, apps, votes, off, apps


def _set_mode(eng, mode):
    if mode is None:
        eng.set_egress(False)
    else:
        eng.set_egress(True, **{m: True for m in mode})


def _egress_sorted(eng):
    from .test_egress_gpu import _egress
    res = _egress(eng, MB * (N + 4))
    n = res["count"]
    order = np.argsort(res["group"][:n], kind="stable")
    out = {name: res[name][:n][order] for name, _ in abi.OUT_BATCH_FIELDS}
    lens = np.diff(res["off"][:n + 1])[order]
    out.update(status=res["status"][:n][order], lens=lens)
    return n, res["total"], out


def test_set_egress_mode_changes():
    """A step and an hb_egress after every mode change; the fresh handle replays the earlier
    steps with egress off and goes straight into the mode.  The step before a change is not
    replayed: hb_egress right after it returns no record."""
    steps = [synth.mixed_batch(_mixed(), k)[0] for k in range(len(MODES))]
    vet = _engine(_mixed())
    seen = 0
    for k, mode in enumerate(MODES):
        fresh = _engine(_mixed())
        for b in steps[:k]:
            fresh.step_batch(b, host=True)
        _set_mode(fresh, mode)
        _set_mode(vet, mode)
        assert vet.egress_mode() == fresh.egress_mode()
        if mode is not None:
            assert _egress_sorted(vet)[0] == 0, f"stage {k}: the step before the change was replayed"
        fresh.step_batch(steps[k], host=True)
        vet.step_batch(steps[k], host=True)
        assert np.array_equal(_events_both_ways(vet, f"stage {k}"), _events_both_ways(fresh, f"fresh {k}"))
        if mode is not None:
            (n, total, got), (wn, wtotal, want) = _egress_sorted(vet), _egress_sorted(fresh)
            assert n == wn and total == wtotal and n > G, f"stage {k}: {n} records, fresh {wn}"
            _same(got, want, f"stage {k} mode {mode}")
            types = set((want["info"] & 0xF).tolist())
            assert abi.HB_MSG_APP_RESP in types and ((abi.HB_MSG_APP in types) == ("apps" in mode))
            seen += n
        fresh.close()
    assert vet.get_groups().tobytes() == _engine_final_groups(steps).tobytes()
    vet.close()
    assert seen > 5 * G


def _engine_final_groups(steps):
    eng = _engine(_mixed())
    for b in steps:
        eng.step_batch(b, host=True)
    g = eng.get_groups()
    eng.close()
    return g


# ---- set_egress_peers: bin_table, bin_key, bin_hist ---------------------------------------------
def test_set_egress_peers_set_clear_set():
    """egress_bin at 20,000 records (above ENC_SMALL_MAX: the tiled kernels with bin_key / bin_hist)
    after a table, refused after the table is cleared, and again after another table."""
    from etcd_amd.hipbatch import HipBatchError
    from .test_egress_bin_gpu import _bin, _check_bin, _records, _table
    n = ENC_SMALL_MAX + 3616
    vet = _engine(_steady())
    for k, ids in enumerate([_table(3, 1), None, _table(64, 2)]):
        if ids is None:
            vet.set_egress_peers([])
            rec = _records(n, _table(3, 1), "uniform", 40)
            with pytest.raises(HipBatchError):
                _bin(vet, rec, n, n)
            continue
        rec = _records(n, ids, "uniform", 40 + k)
        fresh = _engine(_steady())
        fresh.set_egress_peers(ids)
        want = _bin(fresh, rec, n, n)
        fresh.close()
        _check_bin(want, rec, n, ids, f"fresh table {k}")
        vet.set_egress_peers(ids)
        got = _bin(vet, rec, n, n)
        for name in want:
            assert np.array_equal(got[name], want[name]), f"table {k}: {name} differs from the fresh handle's"
    vet.close()


# ---- 32 handles: what a handle allocated is back when it is closed ------------------------------
def test_closed_handles_give_their_memory_back():
    """Each handle turns egress on (append mode: every column), sets a peer table, decodes and makes
    a packed host step (8 MiB of device staging).  After 32 of them free device memory is back
    within one handle's footprint, the margin because the allocator may keep that much cached."""
    import torch
    from .test_ingest_gpu import _dev
    data, off, ln, grp = _corpus(64)
    dev = [_dev(torch, a) for a in (data, off, ln, grp)]
    out = {k: torch.zeros(64, dtype=torch.int32 if k in ("group", "info") else torch.int64, device="cuda")
           for k in ("group", "info", "term", "index", "hint")}
    status = torch.zeros(64, dtype=torch.uint8, device="cuda")
    batch = synth.mixed_batch(_mixed(), 0)[0]
    ids = np.arange(1, 4, dtype=np.uint64)

    def one_handle():
        eng = _engine(_mixed())
        eng.set_egress(True, votes=True, apps=True)
        eng.set_egress_peers(ids)
        eng.decode(*dev, out, status)
        eng.step_batch(batch, host=True)
        eng.sync()
        used = torch.cuda.mem_get_info()[0]
        eng.close()
        return used

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    footprint = free0 - one_handle()
    assert footprint > (8 << 20)  # the staging block alone
    for _ in range(32):
        one_handle()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 >= free0 - footprint, f"{(free0 - free1) >> 10} KiB gone after 32 handles (one takes {footprint >> 10} KiB)"
