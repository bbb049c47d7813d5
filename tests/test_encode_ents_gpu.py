"""GPU parity of hb_encode_ents: a leader's MsgApp with its entries as device
wire bytes, compared bit for bit (bytes[0, total), off, status, total) with the CPU reference
of tests/encode_ents_util.py, which tests/test_wire_out_ents.py pins to the oracle's messages.
"""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import abi, hipbatch, synth
from etcd_amd.splice import varint

from . import egress_app_cases as AC
from .egress_app_util import is_app
from .encode_ents_util import build_source, encode_ents_reference, log_source, records_of
from .golden.make_wire_out_ents_vectors import DATA_LENS

pytestmark = pytest.mark.gpu

SELF = 1
FILL = 0xAA
GUARD = 64
_TV = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_TV[a.dtype])).cuda()


def _source(src):
    """An EntSource on the device from a numpy source dict (n_ent / data_len may understate)."""
    t = {k: _dev(src[k]) for k in ("first", "count", "start", "eterm", "edesc", "edata", "data")}
    return hipbatch.EntSource(t["first"], t["count"], t["start"], t["eterm"], t["edesc"], t["edata"], t["data"],
                              n_ent=src.get("n_ent"), data_len=src.get("data_len"))


def _batch(batch, n):
    return {name: _dev(np.ascontiguousarray(batch[name][:n]) if n else np.zeros(1, dt)) for name, dt in abi.OUT_BATCH_FIELDS}


def _run(eng, batch, n, src, bytes_cap, self_id=SELF, plain=False, dsrc=None, dbatch=None):
    """hb_encode_ents (plain: hb_encode) of the first n records into a buffer of bytes_cap bytes
    that is pre-filled and followed by GUARD bytes; host arrays."""
    import torch
    dbatch = _batch(batch, n) if dbatch is None else dbatch
    data = torch.full((bytes_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    buf = data[:bytes_cap] if bytes_cap else None
    if plain:
        eng.encode(self_id, dbatch, n, buf, off, status, total)
    else:
        eng.encode_ents(self_id, dbatch, n, _source(src) if dsrc is None else dsrc, buf, off, status, total)
    eng.sync()
    return dict(data=data.cpu().numpy(), off=off.cpu().numpy().view(np.uint64), status=status.cpu().numpy()[:n],
                total=int(total.item()), bytes_cap=bytes_cap)


def _check(res, ref, ctx="", n=None):
    """res against the reference (recs, off, st), or against its first n records."""
    recs, off, st = ref
    n = len(recs) if n is None else n
    tot = int(off[n])
    assert res["total"] == tot, f"{ctx}: total {res['total']} expected {tot}"
    assert np.array_equal(res["off"], off[:n + 1]), f"{ctx}: off"
    bad = np.nonzero(res["status"] != st[:n])[0]
    assert len(bad) == 0, f"{ctx}: status at {bad[:5]}: dev {res['status'][bad[:5]]} expected {st[bad[:5]]}"
    if tot > res["bytes_cap"]:
        assert (res["data"] == FILL).all(), f"{ctx}: bytes written although total > bytes_cap"
        return
    blob = b"".join(recs[:n])
    got = res["data"][:tot].tobytes()
    if got != blob:
        i = next(k for k in range(n) if got[int(off[k]):int(off[k + 1])] != recs[k])
        a, b = got[int(off[i]):int(off[i + 1])], recs[i]
        j = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
        raise AssertionError(f"{ctx}: bytes of record {i} differ at byte {j} of {len(b)}: "
                             f"{a[max(j - 8, 0):j + 24].hex()} expected {b[max(j - 8, 0):j + 24].hex()}")
    assert (res["data"][tot:] == FILL).all(), f"{ctx}: bytes written past total"


def _app(g, index, hint, term=7, to=2, commit=None, log_term=None, host=False, to_ref=1):
    """One MsgApp record tuple (egress_app_util.APP_FIELDS) that carries entries (index, hint]."""
    return (g, abi.HB_MSG_APP, to_ref, to, SELF, term, term if log_term is None else log_term, index,
            index if commit is None else commit, False, 0 if host else hint, host, not host)


def _plain(g, mtype=abi.HB_MSG_HEARTBEAT, term=7, to=3, commit=5):
    return (g, mtype, 2, to, SELF, term, 0, 0, commit, False, 0, False, False)


def _arrays(records):
    from .egress_app_util import out_arrays
    return out_arrays(records)


def _payload(ln, salt):
    return None if ln is None else bytes((salt * 29 + 3 * j + (j >> 8)) & 0xFF for j in range(ln))


def _engine(capacity, max_batch=4096, n=3):
    return hipbatch.Engine(capacity, max_replicas=n, max_batch=max_batch)


# ---- 1. the scenario step, every log covered ------------------------------------------------
@pytest.mark.parametrize("nmax", [3, 5, 7])
def test_scenario_step_leaves_whole_messages(nmax):
    from .test_egress_app_gpu import _all_cases, _egress, _oracle_bytes, _scenario_pair
    from .test_egress_app_replay import _step_all
    pair, cases, rafts, peers, batch = _scenario_pair(nmax, votes=True, apps=True)
    assert pair.eng.egress_mode() == 7 and len(cases) == len(_all_cases(nmax))
    pair.step(batch, ctx=f"ents scenarios nmax={nmax}")
    plain = _egress(pair.eng, 4096)  # hb_egress + hb_encode: the records, and what hb_encode makes of them
    n = plain["count"]
    oracle = _step_all(rafts, cases)  # (steps the Raft objects: their logs are the source)
    src = log_source(rafts, capacity=len(cases))
    records = records_of(plain, n, SELF)
    ref = encode_ents_reference(records, src)
    res = _run(pair.eng, plain, n, src, int(ref[1][n]))
    _check(res, ref, f"ents scenarios nmax={nmax}")
    st = res["status"]
    assert not (st & abi.HB_WIRE_SPLICE).any() and (plain["status"][:n] & abi.HB_WIRE_SPLICE).sum() > 10
    host = plain["status"][:n] == abi.HB_WIRE_HOST  # HB_OUT_HOST / HB_REF_OTHER records are unchanged
    assert host.any() and np.array_equal(st == abi.HB_WIRE_HOST, host)
    assert (np.diff(res["off"].astype(np.int64))[host] == 0).all()
    same = ~((plain["info"][:n] & abi.HB_OUT_ENTS) != 0)  # and so is every record without entries
    po, ro = plain["off"].astype(np.int64), res["off"].astype(np.int64)
    for i in np.nonzero(same)[0]:
        assert res["data"][ro[i]:ro[i + 1]].tobytes() == plain["data"][po[i]:po[i + 1]].tobytes()
    # the complete messages against gogo_marshal of the oracle's own r.msgs, per group in order
    term_of = lambda g, i: rafts[g].term(i)  # noqa: E731
    exp = _oracle_bytes(oracle, term_of)
    got = {}
    raw = res["data"].tobytes()
    for i, rec in enumerate(records):
        got.setdefault(rec[0], []).append(None if st[i] == abi.HB_WIRE_HOST else raw[int(ro[i]):int(ro[i + 1])])
    assert set(got) == set(exp)
    k = 0
    for g in exp:
        assert len(got[g]) == len(exp[g]), cases[g]["name"]
        for a, b in zip(got[g], exp[g]):
            if a is not None:
                assert a == b, (cases[g]["name"], a.hex(), b.hex())
                k += 1
    assert k == int((~host).sum()) and sum(is_app(r) and r[12] for r in records) > 10
    assert {c["name"].split("/")[0] for c in cases if c["flagged"]} == set(AC.FLAGGED)


# ---- 2. both launch paths -------------------------------------------------------------------
def test_cfg2_step_through_both_launch_paths(monkeypatch):
    """One 512 x 3 cfg2 step with 16-byte payloads (2,048 records) through k_ence_small and, with
    HB_SMALL_STEP=0, through k_ence_size / k_ence_scan / k_ence_write; n = 0 and the record counts
    around a wave, a workgroup and the small-step bound (the step's records repeated)."""
    from .test_egress_app_gpu import _cfg2
    G, n = 512, 3
    g, _ = synth.steady_groups(G, n, seed=520 + n, last_hi=1 << 14)  # the groups _cfg2 steps
    src = synth.cfg2_entry_source(g, 0, 16)
    out, ref, big = {}, None, None  # (the first engine's records feed both engines)
    for small in ("1", "0"):
        step, pair = _cfg2(monkeypatch, small, "1")
        cnt = step["count"]
        assert cnt == 2048 and (step["status"][:cnt] & abi.HB_WIRE_SPLICE != 0).sum() == 1024
        if ref is None:
            reps = 16385 // cnt + 1
            big = {name: np.tile(step[name][:cnt], reps) for name, _ in abi.OUT_BATCH_FIELDS}
            ref = encode_ents_reference(records_of(big, 16385, SELF), src)
            assert (ref[2][:cnt] == abi.HB_WIRE_OK).all()
        dsrc = _source(src)
        for cap in (0, 1, 255, 256, 257, 2048, 16384, 16385):
            res = _run(pair.eng, big, cap, src, int(ref[1][cap]), dsrc=dsrc)
            _check(res, ref, f"small={small} cap={cap}", n=cap)
            out[small, cap] = res
    for cap in (0, 1, 255, 256, 257, 2048, 16384, 16385):
        a, b = out["1", cap], out["0", cap]
        assert a["total"] == b["total"] and np.array_equal(a["off"], b["off"]) and np.array_equal(a["status"], b["status"])
        assert np.array_equal(a["data"], b["data"]), cap


# ---- 3. coverage boundaries -----------------------------------------------------------------
def _boundary_setup():
    """192 records of 192 groups (one each), every one carrying entries (10, 12] at Term 7 from a
    window of 2 entries with 16-byte payloads; group 100's entries hold the last two positions
    and its second payload the last bytes.  The cases change one group's window or record."""
    N = 192
    recs = [_app(g, 10, 12) for g in range(N)]
    src = dict(first=np.full(N, 11, np.uint64), count=np.full(N, 2, np.uint32),
               start=2 * np.arange(N, dtype=np.uint64))
    src["start"][100], src["start"][N - 1] = 2 * (N - 1), 2 * 100
    src["eterm"] = np.full(2 * N, 7, np.uint64)
    src["edesc"] = np.full(2 * N, abi.hb_ent_desc(16, 0, True), np.uint32)
    src["edata"] = 16 * np.arange(2 * N, dtype=np.uint64)
    src["data"] = (np.arange(32 * N) * 13 % 251).astype(np.uint8)
    return recs, src


def test_coverage_boundaries():
    recs, src = _boundary_setup()
    top = (1 << 64) - 1
    window = {  # group: (first, count, start) of a changed window, and whether it covers (10, 12]
        70: ((11, 0, 140), False),         # count = 0
        75: ((12, 2, 150), False),         # the window starts at index + 2
        80: ((11, 1, 160), False),         # it ends at hint - 1
        90: ((9, 4, 178), True),           # a longer window (over group 89's entries too) that ends at hint
        95: ((9, 3, 188), False),          # a longer window that ends at hint - 1
        125: ((11, 2, top), False),        # start + count would wrap
    }
    cases = {85: True, 100: True}          # exact fit (as every neighbour); start + count = n_ent, edata + len = data_len
    for g, ((first, count, start), cov) in window.items():
        src["first"][g], src["count"][g], src["start"][g] = first, count, start
        cases[g] = cov
    src["edata"][2 * 130 + 1] = top - 7    # edata + len would wrap
    cases[130] = False
    for g, hint in ((110, 10), (115, 9), (120, 13)):  # hint == index, hint < index, one entry past the window
        recs[g] = _app(g, 10, hint)
        cases[g] = False
    recs[135] = _app(135, 10, 12, host=True)  # HB_OUT_HOST: no bytes
    recs[140] = _plain(140)                    # no entries at all
    cases[135] = cases[140] = None
    eng = _engine(192)
    batch = _arrays(recs)
    plain = _run(eng, batch, len(recs), src, 91 * len(recs), plain=True)
    for name, kw, last in (("all", {}, True), ("n_ent + 1", dict(n_ent=2 * 192 - 1), False),
                           ("data_len + 1", dict(data_len=32 * 192 - 1), False)):
        s = dict(src, **kw)
        ref = encode_ents_reference(recs, s)
        res = _run(eng, batch, len(recs), s, int(ref[1][-1]))
        _check(res, ref, f"boundaries {name}")
        want = dict(cases)
        want[100] = last
        for g in range(192):
            cov = want.get(g, True)
            lo, hi = int(res["off"][g]), int(res["off"][g + 1])
            if cov:
                plen = int(plain["off"][g + 1]) - int(plain["off"][g])
                assert res["status"][g] == abi.HB_WIRE_OK and hi - lo == plen + 2 * (2 + 8 + 16), (name, g)
            else:  # as hb_encode writes it
                plo, phi = int(plain["off"][g]), int(plain["off"][g + 1])
                assert res["status"][g] == plain["status"][g], (name, g)
                assert res["data"][lo:hi].tobytes() == plain["data"][plo:phi].tobytes(), (name, g)
                if cov is False:
                    assert res["status"][g] & abi.HB_WIRE_SPLICE, (name, g)
    # (a record whose hint is not above its index carries HB_OUT_ENTS all the same: the split form)
    assert plain["status"][110] & abi.HB_WIRE_SPLICE and plain["status"][135] == abi.HB_WIRE_HOST
    # a group past the capacity is not covered either
    recs2 = list(recs)
    recs2[60] = _app(500, 10, 12)
    ref = encode_ents_reference(recs2, src)
    assert ref[2][60] & abi.HB_WIRE_SPLICE
    _check(_run(eng, _arrays(recs2), len(recs2), src, int(ref[1][-1])), ref, "group past capacity")


# ---- 4. payload shapes ----------------------------------------------------------------------
def _shape_setup():
    """128 records: one per Data length of the CPU fixture (Type 1 on every other one), one
    message of 300 entries, two groups whose windows share their payload bytes, short covered
    records in between."""
    win, recs = {}, []
    g = 0
    for j in range(128):
        if j % 5 == 2 and j // 5 < len(DATA_LENS):
            ln = DATA_LENS[j // 5]
            win[g] = (21, [((j // 5) & 1, 9, _payload(ln, j))])
            recs.append(_app(g, 20, 21, term=9))
        elif j == 8:
            win[g] = (5, [((k % 7 == 0) & 1, 9 - (k < 100), _payload((None, 0, 3, 40, 130)[k % 5], k)) for k in range(300)])
            recs.append(_app(g, 4, 304, term=9))
        else:
            win[g] = (101, [(0, 3, _payload(16, j)), (0, 3, _payload(5, j + 1))])
            recs.append(_app(g, 100, 101 + (j & 1), term=3))
        g += 1
    src = build_source(win, g + 2)
    # groups g and g + 1: windows over other positions, the same payload bytes as group 0's
    for k, gg in enumerate((g, g + 1)):
        src["first"][gg], src["count"][gg], src["start"][gg] = 101, 2, len(src["eterm"])
        for name, v in (("eterm", [3, 3 + k]), ("edesc", src["edesc"][:2]), ("edata", src["edata"][:2])):
            src[name] = np.concatenate([src[name], np.array(v, dtype=src[name].dtype)])
        recs[60 + k] = _app(gg, 100, 102, term=3 + k)
    return recs, src


def test_payload_shapes():
    recs, src = _shape_setup()
    assert {d & abi.HB_ENT_MAX_DATA for d in src["edesc"].tolist()} >= {ln or 0 for ln in DATA_LENS}
    ref = encode_ents_reference(recs, src)
    assert (ref[2] == abi.HB_WIRE_OK).all() and max(len(r) for r in ref[0]) > 70000
    eng = _engine(len(src["first"]))
    _check(_run(eng, _arrays(recs), len(recs), src, int(ref[1][-1])), ref, "payload shapes")


def _regime_setup():
    win, recs = {}, []
    long = np.frombuffer(_payload(65536, 77), np.uint8)
    for w, lane in enumerate((0, 31, 63, None)):
        for k in range(64):
            g = len(recs)
            if k == lane:
                win[g] = (8, [(0, 2, long.tobytes())])
                recs.append(_app(g, 7, 8, term=2))
            else:
                win[g] = (8, [(0, 2, _payload(16 + (k % 3), g))])
                recs.append(_app(g, 7, 8, term=2))
    src = build_source(win, 256 + 1024)
    # the phase records: payload i is blob[at_i, at_i + len_i), at_i % 16 = (i // 16) % 16
    blob = np.frombuffer(_payload(4096, 5), np.uint8)
    base, n0 = len(src["data"]), len(src["eterm"])
    base += (-base) % 16
    src["data"] = np.concatenate([src["data"], np.zeros(base - len(src["data"]), np.uint8), blob])
    lens = [256 + (i * 7) % 41 for i in range(1024)]
    for i, ln in enumerate(lens):
        g = 256 + i
        src["first"][g], src["count"][g], src["start"][g] = 8, 1, n0 + i
        recs.append(_app(g, 7, 8, term=2))
    src["eterm"] = np.concatenate([src["eterm"], np.full(1024, 2, np.uint64)])
    src["edesc"] = np.concatenate([src["edesc"], np.array([abi.hb_ent_desc(ln, 0, True) for ln in lens], np.uint32)])
    src["edata"] = np.concatenate([src["edata"], np.array([base + 16 * (i % 50) + (i // 16) % 16 for i in range(1024)], np.uint64)])
    return recs, src, lens, n0


def test_regime_switch_and_phases():
    """Waves of 63 short records and one 64 KiB payload at lane 0, 31 and 63 (the long regime, the
    payload copied by the wave), a wave of short records only (the LDS regime), then records with
    payloads of 256 to 296 bytes whose sources lie in all 16 phases against all 16 destination phases."""
    recs, src, lens, n0 = _regime_setup()
    ref = encode_ents_reference(recs, src)
    assert (ref[2] == abi.HB_WIRE_OK).all()
    # the payload of phase record i starts at off + prefix + head; the buffer itself is 16-byte aligned
    pairs = set()
    for i, ln in enumerate(lens):
        r = 256 + i
        pairs.add(((i // 16) % 16, (int(ref[1][r + 1]) - 16 - ln) % 16))  # the suffix of these records is 16 bytes
        assert ref[0][r][-16 - ln:-16] == src["data"][int(src["edata"][n0 + i]):][:ln].tobytes()
    assert len(pairs) == 256
    eng = _engine(len(src["first"]))
    import torch
    res = _run(eng, _arrays(recs), len(recs), src, int(ref[1][-1]))
    assert torch.empty(1, device="cuda").data_ptr() % 16 == 0
    _check(res, ref, "regimes and phases")


# ---- 5. bytes_cap ---------------------------------------------------------------------------
def test_bytes_cap_one_short_and_exact():
    recs, src = _shape_setup()
    ref = encode_ents_reference(recs, src)
    total = int(ref[1][-1])
    eng = _engine(len(src["first"]))
    batch = _arrays(recs)
    res = _run(eng, batch, len(recs), src, total - 1)
    assert res["total"] == total and (res["data"] == FILL).all()  # off, status, total written; the buffer untouched
    _check(res, ref, "bytes_cap one short")
    res = _run(eng, batch, len(recs), src, total)
    _check(res, ref, "bytes_cap exact")
    assert (res["data"][total:] == FILL).all() and len(res["data"]) == total + GUARD
    res = _run(eng, batch, len(recs), src, 0)  # no buffer at all
    _check(res, ref, "bytes_cap 0")


# ---- 6. totals past 2^32 --------------------------------------------------------------------
def test_totals_past_2_32():
    import torch
    N, NG, LEN = 70000, 64, 65536
    payload = _payload(LEN, 3)
    # 64 groups, one entry each at its own index and Term, all of them the same 64 KiB
    src = build_source({0: (1, [(0, 1, payload)])}, NG)
    src["first"] = (1000 + 300 * np.arange(NG)).astype(np.uint64)
    src["count"][:] = 1
    src["start"] = np.arange(NG, dtype=np.uint64)
    src["eterm"] = (5 + np.arange(NG)).astype(np.uint64)
    src["edesc"] = np.full(NG, abi.hb_ent_desc(LEN, 0, True), np.uint32)
    src["edata"] = np.zeros(NG, np.uint64)
    per = [_app(g, int(src["first"][g]) - 1, int(src["first"][g]), term=5 + g, to=2 + (g & 1)) for g in range(NG)]
    one = encode_ents_reference(per, src)  # the 64 distinct records
    assert (one[2] == abi.HB_WIRE_OK).all()
    sizes = np.array([len(r) for r in one[0]], dtype=np.uint64)
    recs = [per[i % NG] for i in range(N)]
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(np.tile(sizes, N // NG + 1)[:N], dtype=np.uint64)
    total = int(off[N])
    assert total > 1 << 32
    eng = _engine(NG, max_batch=16384)
    batch = _arrays(recs)
    dbatch, dsrc = _batch(batch, N), _source(src)
    res = _run(eng, batch, N, src, 0, dbatch=dbatch, dsrc=dsrc)
    assert res["total"] == total and np.array_equal(res["off"], off) and (res["status"] == abi.HB_WIRE_OK).all()
    data = torch.empty(total, dtype=torch.uint8, device="cuda")
    doff = torch.full((N + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((N,), 0xEE, dtype=torch.uint8, device="cuda")
    dtotal = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    eng.encode_ents(SELF, dbatch, N, dsrc, data, doff, status, dtotal)
    eng.sync()
    assert int(dtotal.item()) == total and np.array_equal(doff.cpu().numpy().view(np.uint64), off)
    assert (status.cpu().numpy() == abi.HB_WIRE_OK).all()
    straddle = int(np.searchsorted(off, 1 << 32, side="right")) - 1
    assert off[straddle] < 1 << 32 < off[straddle + 1]
    for i in (0, straddle, N - 1):  # only these spans are copied back
        lo, hi = int(off[i]), int(off[i + 1])
        assert data[lo:hi].cpu().numpy().tobytes() == one[0][i % NG], i
    del data


# ---- 7. wide values -------------------------------------------------------------------------
def test_wide_values_in_the_entries():
    """Term near 2^50 and Index near 2^61 (8- and 9-byte varints) through a lifted cfg2 step; Term
    at and above 2^63 (the 10-byte form) through a hand-made batch."""
    from .lift_util import lift
    from .parity_util import Pair
    from .test_egress_app_gpu import _egress
    from .test_egress_gpu import _peers, _tap
    G, n = 128, 3
    g, runs = synth.steady_groups(G, n, seed=703, last_hi=1 << 12)
    g, runs, _ = lift(g, runs, None, 1 << 61, (1 << 50) + 5)
    pair = _tap(Pair(g, runs, n, 256, max_batch=2 * G, term_runs=True))
    pair.eng.load_peers(_peers(G, n))
    pair.eng.set_egress(True, apps=True)
    pair.step(synth.cfg2_batch(g, 0, seed=704), ctx="ents wide")
    plain = _egress(pair.eng, 4 * G)
    cnt = plain["count"]
    assert cnt == 4 * G
    src = synth.cfg2_entry_source(g, 0, 16)
    records = records_of(plain, cnt, SELF)
    ref = encode_ents_reference(records, src)
    assert (ref[2] == abi.HB_WIRE_OK).all()
    assert min(r[5] for r in records) >= 1 << 50 and min(r[7] for r in records) >= 1 << 61
    assert all(len(varint(int(t))) == 8 for t in src["eterm"]) and all(len(varint(int(i))) == 9 for i in src["first"])
    _check(_run(pair.eng, plain, cnt, src, int(ref[1][-1])), ref, "ents wide, lifted")
    # hand-made: Term 2^63 .. 2^64 - 1 in the message and in the entries, Index up to 2^64 - 1
    top = (1 << 64) - 1
    win, recs = {}, []
    for k in range(70):
        term = top - k if k & 1 else (1 << 63) + k
        index = top - 3 - (k % 5) if k % 3 == 0 else (1 << 63) - 2 + k
        cnt = min(2, top - index)
        win[k] = (index + 1, [(k & 1, term - j, _payload(3 * k, k)) for j in range(cnt)])
        recs.append(_app(k, index, index + cnt, term=term, to=top - k, commit=index, log_term=term - 1))
    src = build_source(win, 70)
    ref = encode_ents_reference(recs, src)
    assert (ref[2] == abi.HB_WIRE_OK).all()
    _check(_run(pair.eng, _arrays(recs), len(recs), src, int(ref[1][-1])), ref, "ents wide, hand-made")


# ---- 8. device-to-device loopback -----------------------------------------------------------
def test_loopback_device_to_device():
    """tests/test_ingest_gpu.py::test_loopback_leader_to_follower_and_back's first two hops with no
    host in between: the leader's hb_egress -> hb_egress_bin -> hb_encode_ents -> hb_peer_spans,
    then node 2's span straight into the follower engine's hb_decode_follow (off, len and group
    derived on the device) and step_decoded."""
    import torch
    from .ingest_util import follow_reference
    from .parity_util import Pair, assert_events_equal, assert_groups_equal
    from .test_egress_gpu import _peers, _tap
    from .test_ingest_gpu import _with_sentinel
    G, n, PL = 512, 3, 16
    g, runs = synth.steady_groups(G, n, seed=231, last_hi=1 << 14)
    lead = _tap(Pair(g, runs, n, 256, max_batch=8 * G, term_runs=True))
    lead.eng.load_peers(_peers(G, n))
    lead.eng.set_egress(True, apps=True)
    lead.eng.set_egress_peers(np.array([2, 3], dtype=np.uint64))
    fg, fruns = synth.follow_groups(G, n, seed=231, last_hi=1 << 14, with_runs=True)
    fol = _tap(Pair(fg, fruns, n, 256, max_batch=8 * G, term_runs=True))
    fpeers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    fpeers[:, :3] = (2, 1, 3)
    fol.eng.load_peers(fpeers)
    assert np.array_equal(fg["last_index"], g["last_index"]) and np.array_equal(fg["term"], g["term"])
    src = synth.cfg2_entry_source(g, 0, PL)
    dsrc = _source(src)
    lead.step(synth.cfg2_batch(g, 0, seed=232), ctx="d2d propose")
    # the leader's chain, on its stream
    cap = 8 * G
    t = lambda dt, fill, k=cap: torch.full((max(k, 1),), fill, dtype=dt, device="cuda")  # noqa: E731
    tdt = {"<u4": torch.int32, "<u8": torch.int64}
    raw = {name: t(tdt[dt], -1) for name, dt in abi.OUT_BATCH_FIELDS}
    out = {name: t(tdt[dt], -1) for name, dt in abi.OUT_BATCH_FIELDS}
    count, total = t(torch.int64, -1, 1), t(torch.int64, -1, 1)
    bin_off, span = t(torch.int64, -1, 4), t(torch.int64, -1, 4)
    bytes_cap = cap * (91 + 40 + PL)
    data, off, status = t(torch.uint8, FILL, bytes_cap), t(torch.int64, -1, cap + 1), t(torch.uint8, 0xEE)
    lead.eng.egress(1, raw, cap, count)
    lead.eng.egress_bin(raw, cap, out, bin_off, n_dev=count)
    lead.eng.encode_ents(1, out, cap, dsrc, data, off, status, total, n_dev=count)
    lead.eng.peer_spans(off, bin_off, span)
    lead.eng.sync()
    lo, hi = (int(v) for v in bin_off[:2].cpu().numpy())  # bin 0: node 2 (two words, no message byte)
    nrec = hi - lo
    assert nrec == 2 * G and int(count.item()) == 4 * G
    # the follower's input, derived on the device
    f_off = off[lo:hi]
    f_len = (off[lo + 1:hi + 1] - off[lo:hi]).to(torch.int32)
    f_grp = out["group"][lo:hi].contiguous()
    ent_cap = 2 * G
    full = lambda k, dt: torch.full((max(k, 1),), -0x11111112, dtype=dt, device="cuda")  # noqa: E731
    fout = {k: full(nrec + 1, torch.int32 if k in ("group", "info") else torch.int64)
            for k in ("group", "info", "term", "index", "hint", "commit", "eoff")}
    fout["eterm"], fout["edesc"] = full(ent_cap, torch.int64), full(ent_cap, torch.int32)
    edata, n_ent = full(ent_cap, torch.int64), full(1, torch.int64)
    fstatus = torch.full((nrec,), 0xEE, dtype=torch.uint8, device="cuda")
    # what the follower's oracle steps: the reference encoder's bytes of the same records (the
    # record columns are read here, no message byte of the device is)
    recs_np = {name: out[name][lo:hi].cpu().numpy().view(dt) for name, dt in abi.OUT_BATCH_FIELDS}
    ref = encode_ents_reference(records_of(recs_np, nrec, 1), src)
    assert (ref[2] == abi.HB_WIRE_OK).all()
    from . import wire_util as W
    rdata, roff, rln = W.pack(ref[0])
    fref = follow_reference(rdata, roff, rln, recs_np["group"], G, np.full(G, n, np.uint32), fpeers)
    assert (fref["status"] == abi.HB_WIRE_OK).all() and fref["n_ent"] == G
    ob = _with_sentinel(None, fref)
    fol.reserve(ob)
    fol.eng.decode_follow(data, f_off, f_len, f_grp, fout, fstatus, ent_cap, edata, n_ent)
    fol.eng.step_decoded(fout, ent_cap)
    dev_ev, dev_st = fol.eng.events(), fol.eng.stats()
    ora_ev, ora_st = fol.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, "d2d follower")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_ENTRIES] == G
    fnow = fol.og.groups()
    assert_groups_equal(fol.eng.get_groups(), fnow, "d2d follower")
    assert np.array_equal(fnow["last_index"], g["last_index"] + np.uint64(1))
    # afterwards: the statuses, the entry count, the bytes, and where the decode found the payloads
    assert (fstatus.cpu().numpy() == abi.HB_WIRE_OK).all() and int(n_ent.item()) == G
    st = status.cpu().numpy()[:4 * G]
    assert (st == abi.HB_WIRE_OK).all()
    hoff = off.cpu().numpy().view(np.uint64)
    hdata = data.cpu().numpy()
    base = int(hoff[lo])
    assert hdata[base:int(hoff[hi])].tobytes() == b"".join(ref[0])
    sp = span.cpu().numpy().view(np.uint64)
    assert int(sp[0]) == base and int(sp[1]) == int(hoff[hi]) and int(sp[3]) == int(total.item())
    eoff = fout["eoff"].cpu().numpy().view(np.uint64)
    ed = edata.cpu().numpy().view(np.uint64)
    desc = fout["edesc"].cpu().numpy().view(np.uint32)
    seen = 0
    for i in range(nrec):
        for k in range(int(eoff[i]), int(eoff[i + 1])):
            gi = int(recs_np["group"][i])
            assert int(desc[k]) == abi.hb_ent_desc(PL, 0, True)
            assert hdata[int(ed[k]):int(ed[k]) + PL].tobytes() == src["data"][gi * PL:(gi + 1) * PL].tobytes()
            seen += 1
    assert seen == G


# ---- 9. the argument checks that need a handle ----------------------------------------------
def test_invalid_arguments_with_a_handle():
    eng = _engine(8, max_batch=16)
    L = hipbatch.lib()
    zin, zout = _dev(np.zeros(4096, np.uint64)), _dev(np.zeros(4096, np.uint64))  # inputs (all zero) and outputs
    p, q = zin.data_ptr(), zout.data_ptr()

    def call(cap=1, batch=True, src=True, off=q, status=q + 8192, total=q + 16384, data=None, bytes_cap=0, drop=None, **s):
        b = abi.hb_out_batch()
        for name, _ in abi.OUT_BATCH_FIELDS:
            setattr(b, name, None if drop == name else p)
        e = abi.hb_ent_source()
        for name in ("first", "count", "start", "eterm", "edesc", "edata", "data"):
            setattr(e, name, None if drop == name else p)
        e.n_ent, e.data_len = s.get("n_ent", 4), s.get("data_len", 4)
        return L.hb_encode_ents(eng.h, C.byref(b) if batch else None, cap, None, 1, C.byref(e) if src else None, data,
                                bytes_cap, off, status, total)

    assert call() == abi.HB_OK
    assert call(batch=False) == call(src=False) == call(off=None) == call(status=None) == call(total=None) == abi.HB_EINVAL
    for name, _ in abi.OUT_BATCH_FIELDS:
        assert call(drop=name) == abi.HB_EINVAL, name
    for name in ("first", "count", "start", "eterm", "edesc", "edata", "data"):
        assert call(drop=name) == abi.HB_EINVAL, name
    for name in ("eterm", "edesc", "edata"):
        assert call(drop=name, n_ent=0) == abi.HB_OK, name  # a per-entry array may be NULL with n_ent = 0
    assert call(drop="data", data_len=0) == abi.HB_OK
    assert call(bytes_cap=1) == abi.HB_EINVAL and call(data=q + 20000, bytes_cap=8) == abi.HB_OK
    assert call(cap=16 * 7) == abi.HB_OK and call(cap=16 * 7 + 1) == abi.HB_EINVAL  # max_batch x (max_replicas + 4)
    assert call(cap=1 << 32) == abi.HB_EINVAL
    eng.sync()
