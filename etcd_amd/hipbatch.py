"""Python binding of the engine's C ABI (include/hipbatch.h -> libhipbatch.so).

This is the product path: every call goes to the HIP library.  There is no CPU
fallback — if the library is missing or the device is unusable, construction
fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HB_LIB", os.path.join(_HERE, "libhipbatch.so"))
_lib = None


class HipBatchError(RuntimeError):
    def __init__(self, fn, code):
        self.code = code
        super().__init__(f"{fn} failed: {code} ({_strerror(code)})")


def _strerror(code):
    try:
        return lib().hb_strerror(code).decode()
    except Exception:
        return "?"


class HipRuntimeConflict(RuntimeError):
    """Two HIP runtimes (libamdhip64) are or would be mapped in this process:
    the engine's handle would live in one and the caller's streams and tensors
    in the other (hb_create then fails with HB_EDEVICE)."""


def _mapped_hip_runtimes():
    """The distinct libamdhip64 files mapped into this process (real paths)."""
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split()[-1]
                if "libamdhip64" in os.path.basename(p):
                    out.add(os.path.realpath(p))
    except OSError:
        pass
    return out


def _bind_one_hip_runtime():
    """Make the engine bind to the HIP runtime torch uses, whatever the import order.

    libhipbatch.so needs `libamdhip64.so.7` (RUNPATH /opt/rocm).  PyTorch-ROCm
    ships its own copy, which its libraries load as `libamdhip64.so` from their
    own directory.  Loaded after torch, the engine binds to torch's copy by
    soname; loaded first, it would map /opt/rocm's and torch would later map a
    second runtime beside it (r05: `hb_create failed: -3` in a process that
    imported the router before torch).  So when no runtime is mapped yet and
    torch's copy exists, that file is preloaded (RTLD_GLOBAL): the engine binds
    to it by soname and torch's later load finds the same file already mapped.
    A process that already holds two runtimes cannot be fixed here: a named
    error instead of HB_EDEVICE at the first call."""
    have = _mapped_hip_runtimes()
    if len(have) > 1:
        raise HipRuntimeConflict(f"two HIP runtimes already mapped: {sorted(have)}")
    if have:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for d in (spec.submodule_search_locations or []) if spec else []:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)
            return


def lib():
    """Load libhipbatch.so (built by `make -C etcd_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C etcd_amd/csrc` "
                          "(there is no CPU fallback)")
    _bind_one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    have = _mapped_hip_runtimes()
    if len(have) > 1:
        raise HipRuntimeConflict(f"loading {LIB_PATH} mapped a second HIP runtime: {sorted(have)}")
    P = C.POINTER
    H = C.c_void_p
    sig = {
        "hb_abi_version": (C.c_int, []),
        "hb_strerror": (C.c_char_p, [C.c_int]),
        "hb_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, P(H)]),
        "hb_destroy": (C.c_int, [H]),
        "hb_set_stream": (C.c_int, [H, C.c_void_p]),
        "hb_set_input_stream": (C.c_int, [H, C.c_void_p]),
        "hb_sync": (C.c_int, [H]),
        "hb_load_groups": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_void_p]),
        "hb_get_groups": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_void_p]),
        "hb_remove_groups": (C.c_int, [H, C.c_uint32, C.c_uint32]),
        "hb_move_groups": (C.c_int, [H, C.c_uint32, C.c_void_p, C.c_void_p]),
        "hb_set_inflights": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
        "hb_set_log_bounds": (C.c_int, [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_load_entry_sizes": (C.c_int, [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_load_term_runs": (C.c_int, [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_reserve_log": (C.c_int, [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_log_capacity": (C.c_int, [H, C.c_uint32, P(C.c_uint64), P(C.c_uint64)]),
        "hb_get_inflights": (C.c_int, [H, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32), C.c_void_p]),
        "hb_step": (C.c_int, [H, P(abi.hb_batch), C.c_uint32]),
        "hb_load_timers": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_void_p]),
        "hb_get_timers": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_void_p]),
        "hb_set_rand": (C.c_int, [H, C.c_uint64, C.c_uint64, C.c_void_p]),
        "hb_tick": (C.c_int, [H, C.c_uint32]),
        "hb_load_peers": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_void_p]),
        "hb_decode": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(abi.hb_batch),
                                C.c_void_p]),
        "hb_decode_caps": (C.c_int, []),
        "hb_decode_follow": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(abi.hb_batch),
                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
        "hb_set_egress": (C.c_int, [H, C.c_int]),
        "hb_egress_mode": (C.c_int, [H]),
        "hb_egress_caps": (C.c_int, []),
        "hb_set_egress_limit": (C.c_int, [H, C.c_int]),
        "hb_egress_limit": (C.c_int, [H]),
        "hb_egress_limit_caps": (C.c_int, []),
        "hb_set_egress_logterm": (C.c_int, [H, C.c_int]),
        "hb_egress_logterm": (C.c_int, [H]),
        "hb_egress_logterm_caps": (C.c_int, []),
        "hb_set_wire_props": (C.c_int, [H, C.c_int]),
        "hb_wire_props": (C.c_int, [H]),
        "hb_wire_props_caps": (C.c_int, []),
        "hb_egress": (C.c_int, [H, C.c_uint64, P(abi.hb_out_batch), C.c_uint64, C.c_void_p]),
        "hb_encode": (C.c_int, [H, P(abi.hb_out_batch), C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_encode_caps": (C.c_int, []),
        "hb_encode_ents": (C.c_int, [H, P(abi.hb_out_batch), C.c_uint64, C.c_void_p, C.c_uint64, P(abi.hb_ent_source),
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_set_egress_peers": (C.c_int, [H, C.c_void_p, C.c_uint32]),
        "hb_egress_bin": (C.c_int, [H, P(abi.hb_out_batch), C.c_uint64, C.c_void_p, P(abi.hb_out_batch), C.c_void_p,
                                    C.c_void_p]),
        "hb_peer_spans": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p]),
        "hb_frame_caps": (C.c_int, []),
        "hb_frame_size": (C.c_uint64, [C.c_uint64]),
        "hb_frame_rows": (C.c_uint64, [C.c_uint64]),
        "hb_gid_dir_build": (C.c_int, [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
        "hb_frame": (C.c_int, [H, P(abi.hb_out_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
        "hb_unframe": (C.c_int, [H, C.c_void_p, C.c_uint64, P(abi.hb_frame_in), C.c_uint32, C.c_uint64,
                                 P(abi.hb_gid_dir), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                 C.c_void_p, C.c_void_p]),
        "hb_events_device": (C.c_int, [H, P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_uint32)]),
        "hb_copy_events": (C.c_int, [H, C.c_void_p, C.c_uint64, P(C.c_uint64)]),
        "hb_events_to_host": (C.c_int, [H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
        "hb_event_words_chunks": (C.c_int, [H, P(C.c_uint32), P(C.c_uint32)]),
        "hb_expand_event_words": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                            P(C.c_uint64)]),
        "hb_stats_device": (C.c_int, [H, P(C.c_void_p)]),
        "hb_stats": (C.c_int, [H, C.c_void_p]),
        "hb_phase_ms": (C.c_int, [H, C.c_void_p, P(C.c_uint32)]),
        "hb_phase_reset": (C.c_int, [H]),
        "hb_step_kernels": (C.c_int, [H, P(C.c_uint32)]),
        "hb_stats_to": (C.c_int, [H, C.c_void_p]),
        "hb_set_stats_accum": (C.c_int, [H, C.c_void_p]),
        "hb_alloc_pinned": (C.c_int, [C.c_size_t, P(C.c_void_p)]),
        "hb_free_pinned": (C.c_int, [C.c_void_p]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.hb_abi_version() != abi.HB_ABI_VERSION:
        raise ImportError("libhipbatch ABI version mismatch")
    _lib = L
    return L


def _check(fn, rc):
    if rc != abi.HB_OK:
        raise HipBatchError(fn, rc)


def _ptr(a):
    """Address of a numpy array or a torch tensor (host or device)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


class EntSource:
    """The entry source of Engine.encode_ents (hb_ent_source): keeps the device tensors alive
    and builds the struct.  first / start u64 [capacity], count u32 [capacity]; eterm / edata
    u64 and edesc u32 of one length (None for no entries); data u8 (None for no payload)."""

    def __init__(self, first, count, start, eterm=None, edesc=None, edata=None, data=None, n_ent=None,
                 data_len=None):
        self.first, self.count, self.start = first, count, start
        self.eterm, self.edesc, self.edata, self.data = eterm, edesc, edata, data
        self.n_ent = (0 if edesc is None else len(edesc)) if n_ent is None else int(n_ent)
        self.data_len = (0 if data is None else len(data)) if data_len is None else int(data_len)

    def struct(self):
        s = abi.hb_ent_source()
        for name in ("first", "count", "start", "eterm", "edesc", "edata", "data"):
            setattr(s, name, _ptr(getattr(self, name)))
        s.n_ent, s.data_len = self.n_ent, self.data_len
        return s


class GidDir:
    """The group-id directory of Engine.unframe (hb_gid_dir): keeps the device tensors alive and
    builds the struct.  key u64 [cap], slot u32 [cap]; cap a power of two, at least 64 and at
    least twice the ids it holds."""

    def __init__(self, key, slot, cap=None):
        self.key, self.slot = key, slot
        self.cap = len(key) if cap is None else int(cap)

    def struct(self):
        d = abi.hb_gid_dir()
        d.key, d.slot, d.cap = _ptr(self.key), _ptr(self.slot), self.cap
        return d


class Engine:
    """One device-resident shard of raft groups (one hb_handle)."""

    def __init__(self, capacity, max_replicas=3, max_inflight=256, max_msg_size=abi.HB_NO_LIMIT,
                 max_batch=1 << 20, device=0, stream=None):
        L = lib()
        h = C.c_void_p()
        _check("hb_create", L.hb_create(device, capacity, max_replicas, max_inflight, max_msg_size,
                                        max_batch, C.byref(h)))
        self.h = h
        self.capacity = capacity
        self.max_inflight = max_inflight
        self.max_batch = max_batch
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "h", None):
            lib().hb_destroy(self.h)
            self.h = None
        for p, _ in getattr(self, "_pins", {}).values():
            lib().hb_free_pinned(p)
        self._pins = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream, a raw hipStream_t int, or None."""
        raw = getattr(stream, "cuda_stream", stream)
        _check("hb_set_stream", lib().hb_set_stream(self.h, C.c_void_p(raw or 0)))

    def set_input_stream(self, stream):
        """The stream that produces batch arrays (torch.cuda.Stream / raw hipStream_t / None
        for the null stream): the prep stage of a step waits only for it, so it can overlap
        the previous step's apply."""
        raw = getattr(stream, "cuda_stream", stream)
        _check("hb_set_input_stream", lib().hb_set_input_stream(self.h, C.c_void_p(raw or 0)))

    def sync(self):
        _check("hb_sync", lib().hb_sync(self.h))

    # ---- group state ---------------------------------------------------------
    def load_groups(self, groups, first=0):
        g = np.ascontiguousarray(groups, dtype=abi.GROUP_DTYPE)
        _check("hb_load_groups", lib().hb_load_groups(self.h, first, len(g), g.ctypes.data))

    def get_groups(self, first=0, count=None):
        count = self.capacity - first if count is None else count
        out = np.zeros(count, dtype=abi.GROUP_DTYPE)
        _check("hb_get_groups", lib().hb_get_groups(self.h, first, count, out.ctypes.data))
        return out

    def remove_groups(self, first, count):
        _check("hb_remove_groups", lib().hb_remove_groups(self.h, first, count))

    def move_groups(self, src, dst):
        """hb_move_groups: slot dst[i] takes every device word of slot src[i] (all sources
        are read first: swaps, cycles and chains are fine); vacated slots end up empty."""
        s = np.ascontiguousarray(src, dtype=np.uint32)
        d = np.ascontiguousarray(dst, dtype=np.uint32)
        assert s.shape == d.shape and s.ndim == 1
        _check("hb_move_groups", lib().hb_move_groups(self.h, len(s), s.ctypes.data if len(s) else None,
                                                      d.ctypes.data if len(d) else None))

    def set_inflights(self, group, slot, start, vals):
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        _check("hb_set_inflights", lib().hb_set_inflights(self.h, group, slot, start, len(v),
                                                          v.ctypes.data if len(v) else None))

    def set_log_bounds(self, groups, first_index, snap_index):
        """Refresh firstIndex / snapshot index of the given group slots after
        the application compacted or snapshotted their storage."""
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        f = np.ascontiguousarray(first_index, dtype=np.uint64)
        s = np.ascontiguousarray(snap_index, dtype=np.uint64)
        assert len(g) == len(f) == len(s)
        _check("hb_set_log_bounds", lib().hb_set_log_bounds(self.h, len(g), g.ctypes.data, f.ctypes.data,
                                                            s.ctypes.data))

    def load_entry_sizes(self, sizes):
        """Finite max_msg_size: {group slot: Entry.Size() of its last n entries, oldest first}
        (normally the whole log from firstIndex; the ring grows to hold them)."""
        gs = np.ascontiguousarray(sorted(sizes), dtype=np.uint32)
        ns = np.ascontiguousarray([len(sizes[int(g)]) for g in gs], dtype=np.uint32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(sizes[int(g)], dtype=np.uint32) for g in gs])
                                    if len(gs) else np.zeros(1, np.uint32), dtype=np.uint32)
        _check("hb_load_entry_sizes", lib().hb_load_entry_sizes(self.h, len(gs), gs.ctypes.data, ns.ctypes.data,
                                                                flat.ctypes.data))

    def load_term_runs(self, runs):
        """Follower side: {group slot: [(start index, term), ...] older term runs, oldest first}
        (normally every run down to firstIndex - 1; the ring grows to hold them)."""
        gs = np.ascontiguousarray(sorted(runs), dtype=np.uint32)
        ns = np.ascontiguousarray([len(runs[int(g)]) for g in gs], dtype=np.uint32)
        flat = np.ascontiguousarray([x for g in gs for r in runs[int(g)] for x in r] or [0], dtype=np.uint64)
        _check("hb_load_term_runs", lib().hb_load_term_runs(self.h, len(gs), gs.ctypes.data, ns.ctypes.data,
                                                            flat.ctypes.data))

    def reserve_log(self, groups, size_cap=None, run_cap=None):
        """Grow the log-index rings of the given group slots to hold at least
        size_cap entry sizes / run_cap term runs (hb_reserve_log; None = unchanged)."""
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        if not len(g):
            return
        sc = None if size_cap is None else np.ascontiguousarray(np.broadcast_to(size_cap, g.shape), dtype=np.uint64)
        rc = None if run_cap is None else np.ascontiguousarray(np.broadcast_to(run_cap, g.shape), dtype=np.uint64)
        _check("hb_reserve_log", lib().hb_reserve_log(self.h, len(g), g.ctypes.data,
                                                      None if sc is None else sc.ctypes.data,
                                                      None if rc is None else rc.ctypes.data))

    def log_capacity(self, group):
        """(size ring capacity, term-run ring capacity) of one group slot."""
        a, b = C.c_uint64(), C.c_uint64()
        _check("hb_log_capacity", lib().hb_log_capacity(self.h, group, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get_inflights(self, group, slot):
        out = np.zeros(self.max_inflight, dtype=np.uint64)
        s, c = C.c_uint32(), C.c_uint32()
        _check("hb_get_inflights", lib().hb_get_inflights(self.h, group, slot, C.byref(s), C.byref(c),
                                                          out.ctypes.data))
        return s.value, out[: c.value].copy()

    # ---- hot path --------------------------------------------------------------
    def step(self, group, info, term, index, hint=None, props=None, host=None, profile=False, edesc=None,
             eoff=None, peoff=None, commit=None, eterm=None, msg_props=False):
        """Step one batch.  Arrays are numpy (host) or torch tensors (host or cuda).
        profile: False, True (every phase) or "apply" (only HB_PHASE_APPLY).
        edesc / eoff / peoff: entry descriptors (finite max_msg_size, include/hipbatch.h).
        msg_props: the batch carries MsgProp messages (HB_STEP_MSG_PROPS)."""
        b = abi.hb_batch()
        b.n = len(group)
        b.group, b.info, b.term, b.index = _ptr(group), _ptr(info), _ptr(term), _ptr(index)
        b.hint, b.props = _ptr(hint), _ptr(props)
        b.n_edesc = len(edesc) if edesc is not None else (len(eterm) if eterm is not None else 0)
        b.edesc, b.eoff, b.peoff = _ptr(edesc), _ptr(eoff), _ptr(peoff)
        b.commit, b.eterm = _ptr(commit), _ptr(eterm)
        if host is None:
            host = not (hasattr(group, "is_cuda") and group.is_cuda)
        prof = {True: abi.HB_STEP_PROFILE, "apply": abi.HB_STEP_PROFILE_APPLY}.get(profile, 0)
        flags = (abi.HB_STEP_HOST_PTRS if host else 0) | prof | (abi.HB_STEP_MSG_PROPS if msg_props else 0)
        self._keep = (group, info, term, index, hint, props, edesc, eoff, peoff, commit, eterm)
        _check("hb_step", lib().hb_step(self.h, C.byref(b), flags))

    # ---- timers (MultiNode.Tick) ----------------------------------------------
    def load_timers(self, timers, first=0):
        t = np.ascontiguousarray(timers, dtype=abi.TIMER_DTYPE)
        _check("hb_load_timers", lib().hb_load_timers(self.h, first, len(t), t.ctypes.data))

    def get_timers(self, first=0, count=None):
        count = self.capacity - first if count is None else count
        out = np.zeros(count, dtype=abi.TIMER_DTYPE)
        _check("hb_get_timers", lib().hb_get_timers(self.h, first, count, out.ctypes.data))
        return out

    def set_rand(self, draws, first=0):
        """The node's r.rand.Int() stream (rand.New(rand.NewSource(id)))."""
        d = np.ascontiguousarray(draws, dtype=np.uint64)
        _check("hb_set_rand", lib().hb_set_rand(self.h, first, len(d), d.ctypes.data if len(d) else None))

    def tick(self):
        """One MultiNode.Tick over every group (asynchronous; events/stats as step)."""
        _check("hb_tick", lib().hb_tick(self.h, 0))

    # ---- wire ingestion ----------------------------------------------------------
    def load_peers(self, ids, first=0):
        """ids: [count, HB_MAX_REPLICAS] node ids per slot (0 = none)."""
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1, abi.HB_MAX_REPLICAS)
        _check("hb_load_peers", lib().hb_load_peers(self.h, first, len(a), a.ctypes.data))

    def decode(self, data, off, length, group, out, status):
        """Decode raftpb.Message records (device tensors) into the batch arrays
        out = {group, info, term, index, hint} (device tensors) + status (u8)."""
        b = abi.hb_batch()
        b.n = len(off)
        b.group, b.info, b.term, b.index = _ptr(out["group"]), _ptr(out["info"]), _ptr(out["term"]), _ptr(out["index"])
        b.hint, b.props = _ptr(out["hint"]), None
        self._keep_dec = (data, off, length, group, out, status)
        _check("hb_decode", lib().hb_decode(self.h, _ptr(data), _ptr(off), _ptr(length), _ptr(group), len(off),
                                            C.byref(b), _ptr(status)))

    def decode_follow(self, data, off, length, group, out, status, ent_cap, edata, n_ent):
        """hb_decode_follow: decode() plus the follower side (MsgApp with its entries, MsgHeartbeat,
        MsgVote).  out = {group, info, term, index, hint, commit, eoff} of len(off) + 1 elements
        (record n is the sentinel, eoff[n] the entry count) and {eterm, edesc} of ent_cap
        entries; edata = device u64 [ent_cap] (where each entry's Data lies in `data`);
        n_ent = a device (or pinned) u64 that takes the entry count.  When it exceeds ent_cap
        no entry word is written.  Step the result with step_decoded()."""
        b = abi.hb_batch()
        b.n = len(off)
        b.group, b.info, b.term, b.index = _ptr(out["group"]), _ptr(out["info"]), _ptr(out["term"]), _ptr(out["index"])
        b.hint, b.props, b.commit = _ptr(out["hint"]), None, _ptr(out["commit"])
        b.eoff, b.eterm, b.edesc = _ptr(out["eoff"]), _ptr(out.get("eterm")), _ptr(out.get("edesc"))
        b.n_edesc = ent_cap
        self._keep_decf = (data, off, length, group, out, status, edata, n_ent)
        _check("hb_decode_follow", lib().hb_decode_follow(self.h, _ptr(data), _ptr(off), _ptr(length), _ptr(group),
                                                          len(off), C.byref(b), _ptr(status), ent_cap, _ptr(edata),
                                                          _ptr(n_ent)))

    def step_decoded(self, out, ent_cap, props=None):
        """Step what decode_follow() wrote, sentinel included (b.n = n + 1, n_edesc = ent_cap):
        no host read of the entry count lies between the two calls."""
        self.step(out["group"], out["info"], out["term"], out["index"], out["hint"], props, host=False,
                  edesc=out.get("edesc") if ent_cap else None, eoff=out["eoff"], commit=out["commit"],
                  eterm=out.get("eterm") if ent_cap else None)

    # ---- wire egress ---------------------------------------------------------------
    def set_egress(self, on=True, votes=False, apps=False):
        """hb_set_egress: every later step / tick keeps the groups' Term and lastIndex
        from before it, which egress() needs; off frees them.  votes: vote mode
        (HB_EGRESS_VOTES), the lastTerm column too and campaign's MsgVote records.
        apps: append mode (HB_EGRESS_APPS), the committed column and the boundary pair
        too and sendAppend's MsgApp records (etcd_amd.splice completes those with entries)."""
        mode = (abi.HB_EGRESS_ON | (abi.HB_EGRESS_VOTES if votes else 0) | (abi.HB_EGRESS_APPS if apps else 0)) \
            if on else 0
        _check("hb_set_egress", lib().hb_set_egress(self.h, mode))

    def egress_mode(self):
        """hb_egress_mode: 0, or HB_EGRESS_ON | any of HB_EGRESS_VOTES and HB_EGRESS_APPS."""
        m = lib().hb_egress_mode(self.h)
        if m < 0:
            raise HipBatchError("hb_egress_mode", m)
        return m

    def set_egress_limit(self, on=True):
        """hb_set_egress_limit: in append mode under a finite max_msg_size, a MsgApp record
        with entries carries limitSize's cut (HB_OUT_ENTS, hint = the last entry sent) where
        the device can prove it, instead of HB_OUT_HOST.  egress() then runs before any call
        that rewrites a group's size ring (load_entry_sizes, load / remove / move groups)."""
        _check("hb_set_egress_limit", lib().hb_set_egress_limit(self.h, 1 if on else 0))

    def egress_limit(self):
        """hb_egress_limit: whether the knob is on."""
        v = lib().hb_egress_limit(self.h)
        if v < 0:
            raise HipBatchError("hb_egress_limit", v)
        return bool(v)

    def set_egress_logterm(self, on=True):
        """hb_set_egress_logterm: in append mode, a MsgApp record whose send lies below the
        leader's boundary carries the term of its Index, read from the group's older-runs ring
        where the device can prove it, instead of HB_OUT_HOST.  egress() then runs before any
        call that rewrites a group's run ring (load_term_runs, load / remove / move groups)."""
        _check("hb_set_egress_logterm", lib().hb_set_egress_logterm(self.h, 1 if on else 0))

    def egress_logterm(self):
        """hb_egress_logterm: whether the knob is on."""
        v = lib().hb_egress_logterm(self.h)
        if v < 0:
            raise HipBatchError("hb_egress_logterm", v)
        return bool(v)

    def set_wire_props(self, decode=False, egress=False):
        """hb_set_wire_props: forwarded proposals on the wire path.  decode
        (HB_WIRE_PROPS_IN): decode_follow() makes a batch record of a canonical forwarded
        MsgProp, its entry run at eoff like a MsgApp's.  egress (HB_WIRE_PROPS_OUT): egress()
        makes a split MsgProp record of every HB_EV_PROP_FWD event, hint = the proposal's
        arrival index (etcd_amd.splice completes it with the entries the host holds)."""
        bits = (abi.HB_WIRE_PROPS_IN if decode else 0) | (abi.HB_WIRE_PROPS_OUT if egress else 0)
        _check("hb_set_wire_props", lib().hb_set_wire_props(self.h, bits))

    def wire_props(self):
        """hb_wire_props: the bits in force (HB_WIRE_PROPS_IN | HB_WIRE_PROPS_OUT)."""
        v = lib().hb_wire_props(self.h)
        if v < 0:
            raise HipBatchError("hb_wire_props", v)
        return v

    @staticmethod
    def _out_batch(out):
        b = abi.hb_out_batch()
        for name, _ in abi.OUT_BATCH_FIELDS:
            setattr(b, name, _ptr(out[name]))
        return b

    def egress(self, self_id, out, cap, count):
        """hb_egress: the last step's payload-free outgoing messages into the device
        tensors out = {group, info, to, term, log_term, index, commit, hint} of `cap`
        records; count = a device (or pinned) u64 that takes the record count."""
        b = self._out_batch(out)
        self._keep_eg = (out, count)
        _check("hb_egress", lib().hb_egress(self.h, self_id, C.byref(b), cap, _ptr(count)))

    def encode(self, self_id, batch, cap, data, off, status, total, n_dev=None):
        """hb_encode: the records of `batch` (an egress() out dict) as raftpb.Message bytes
        into the device tensor `data` (u8), off [cap + 1] (u64), status [cap] (u8); total and
        n_dev = device (or pinned) u64 words (n_dev None: cap records)."""
        b = self._out_batch(batch)
        self._keep_enc = (batch, data, off, status, total, n_dev)
        _check("hb_encode", lib().hb_encode(self.h, C.byref(b), cap, _ptr(n_dev), self_id, _ptr(data),
                                            0 if data is None else len(data), _ptr(off), _ptr(status), _ptr(total)))

    def encode_ents(self, self_id, batch, cap, src, data, off, status, total, n_dev=None):
        """hb_encode_ents: encode() with the entries of every covered MsgApp written by the device
        from `src` (an EntSource): such a record comes out whole with status HB_WIRE_OK; one
        that `src` does not cover keeps HB_WIRE_SPLICE | prefix_len.  `data` must not overlap
        the source's payload bytes."""
        b = self._out_batch(batch)
        s = src.struct()
        self._keep_ence = (batch, src, data, off, status, total, n_dev)
        _check("hb_encode_ents", lib().hb_encode_ents(self.h, C.byref(b), cap, _ptr(n_dev), self_id, C.byref(s),
                                                      _ptr(data), 0 if data is None else len(data), _ptr(off),
                                                      _ptr(status), _ptr(total)))

    def set_egress_peers(self, ids):
        """hb_set_egress_peers: the node table of egress_bin(); bin b is ids[b], bin len(ids)
        is "other".  At most HB_EGRESS_MAX_PEERS distinct non-zero ids; an empty list frees it."""
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        _check("hb_set_egress_peers", lib().hb_set_egress_peers(self.h, a.ctypes.data if len(a) else None, len(a)))

    def egress_bin(self, batch, cap, out, bin_off, src=None, n_dev=None):
        """hb_egress_bin: the records of `batch` (an egress() out dict) split stably by destination
        node into the device tensors of `out` (the same eight arrays, none shared with `batch`);
        bin_off = device (or pinned) u64 [len(ids) + 2], src = optional device u32 [cap] (the input
        index of every output record), n_dev = a device (or pinned) u64 (None: cap records)."""
        bi, bo = self._out_batch(batch), self._out_batch(out)
        self._keep_bin = (batch, out, bin_off, src, n_dev)
        _check("hb_egress_bin", lib().hb_egress_bin(self.h, C.byref(bi), cap, _ptr(n_dev), C.byref(bo), _ptr(src),
                                                    _ptr(bin_off)))

    def peer_spans(self, off, bin_off, span):
        """hb_peer_spans: span[b] = off[bin_off[b]] (device or pinned u64 [len(ids) + 2]); with `off`
        from an encode() of the binned batch, peer b's bytes are data[span[b]:span[b + 1]]."""
        self._keep_span = (off, bin_off, span)
        _check("hb_peer_spans", lib().hb_peer_spans(self.h, _ptr(off), _ptr(bin_off), _ptr(span)))

    # ---- framed peer streams -----------------------------------------------------
    def gid_dir_build(self, gid, dir, dups, count=None):
        """hb_gid_dir_build: `dir` (a GidDir) cleared, then gid[i] -> i for every non-zero id of the
        device u64 tensor `gid`; dups = a device (or pinned) u32 that takes the repeated ids."""
        self._keep_gd = (gid, dir, dups)
        _check("hb_gid_dir_build", lib().hb_gid_dir_build(self.h, _ptr(gid), len(gid) if count is None else count,
                                                          _ptr(dir.key), _ptr(dir.slot), dir.cap, _ptr(dups)))

    def frame(self, self_id, seq, binned, off, status, bin_off, span, gid, index, ispan, fstat, index_cap=None):
        """hb_frame: the index frames of a binned batch (egress_bin's out and bin_off, encode's off and
        status of it, peer_spans' span; gid = device u64 [capacity], the id of every slot) into the
        device u8 tensor `index`; ispan u64 [peers + 2] and fstat u32 [peers + 1], device or pinned."""
        b = self._out_batch(binned)
        self._keep_fr = (binned, off, status, bin_off, span, gid, index, ispan, fstat)
        cap = (0 if index is None else len(index)) if index_cap is None else index_cap
        _check("hb_frame", lib().hb_frame(self.h, C.byref(b), _ptr(off), _ptr(status), _ptr(bin_off), _ptr(span),
                                          _ptr(gid), self_id, seq, _ptr(index), cap, _ptr(ispan), _ptr(fstat)))

    def unframe(self, self_id, index, frames, dir, bytes_size, off, length, group, fstatus, n_unknown, n=None,
                index_size=None):
        """hb_unframe: received frames -> decode_follow's off / length / group (device tensors of n
        rows).  frames = [(index_off, index_len, bytes_off, bytes_len, from), ...] in the order their
        rows take; dir = a GidDir; fstatus u32 [len(frames)] and n_unknown u64, device or pinned."""
        fr = (abi.hb_frame_in * max(len(frames), 1))()
        for k, f in enumerate(frames):
            fr[k].index_off, fr[k].index_len, fr[k].bytes_off, fr[k].bytes_len, fr[k].from_ = (int(v) for v in f)
        d = dir.struct()
        self._keep_unf = (index, dir, off, length, group, fstatus, n_unknown)
        isz = (0 if index is None else len(index)) if index_size is None else index_size
        _check("hb_unframe", lib().hb_unframe(self.h, _ptr(index), isz, fr, len(frames), self_id, C.byref(d),
                                              bytes_size, _ptr(off), _ptr(length), _ptr(group),
                                              (0 if off is None else len(off)) if n is None else n, _ptr(fstatus),
                                              _ptr(n_unknown)))

    def step_batch(self, batch, **kw):
        return self.step(batch["group"], batch["info"], batch["term"], batch["index"],
                         batch.get("hint"), batch.get("props"), edesc=batch.get("edesc"), eoff=batch.get("eoff"),
                         peoff=batch.get("peoff"), commit=batch.get("commit"), eterm=batch.get("eterm"),
                         msg_props=bool(batch.get("msg_props", False)), **kw)

    def events(self):
        """Dense events of the last step (host copy, synchronizes)."""
        n = C.c_uint64()
        L = lib()
        rc = L.hb_copy_events(self.h, None, 0, C.byref(n))
        if rc not in (abi.HB_OK, abi.HB_EINVAL):
            _check("hb_copy_events", rc)
        out = np.zeros(max(n.value, 1), dtype=abi.EVENT_DTYPE)
        _check("hb_copy_events", L.hb_copy_events(self.h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value]

    def events_into(self, host_ptr, cap):
        """Dense events of the last step into caller memory (e.g. pinned) of
        `cap` hb_event records; returns the count (synchronizes)."""
        n = C.c_uint64()
        _check("hb_copy_events", lib().hb_copy_events(self.h, C.c_void_p(host_ptr), cap, C.byref(n)))
        return n.value

    def n_chunks(self):
        n, per = C.c_uint32(), C.c_uint32()
        _check("hb_event_words_chunks", lib().hb_event_words_chunks(self.h, C.byref(n), C.byref(per)))
        return n.value, per.value

    def events_to_host(self, words_ptr, cap, counts_ptr, total_ptr):
        """Asynchronous compact delta (hb_events_to_host) into pinned buffers
        (hb_alloc_pinned / torch pin_memory): read them after sync()."""
        _check("hb_events_to_host", lib().hb_events_to_host(self.h, C.c_void_p(words_ptr), cap,
                                                            C.c_void_p(counts_ptr), C.c_void_p(total_ptr)))

    def event_words(self):
        """The last step's compact event words and per-chunk counts (host copies;
        synchronizes), via hb_events_to_host into pinned buffers."""
        nc, _ = self.n_chunks()
        L = lib()
        pins = getattr(self, "_pins", None)
        if pins is None:
            pins = self._pins = {}

        def pinned(name, nbytes):
            p, cap = pins.get(name, (None, 0))
            if cap < nbytes:
                if p:
                    L.hb_free_pinned(p)
                q = C.c_void_p()
                _check("hb_alloc_pinned", L.hb_alloc_pinned(max(nbytes, 64), C.byref(q)))
                pins[name] = (q.value, max(nbytes, 64))
            return pins[name][0]
        cnt = pinned("counts", 4 * nc)
        tot = pinned("total", 8)
        cap = pins.get("words", (None, 0))[1] // 8
        for _ in range(2):
            w = pinned("words", 8 * max(cap, 1))
            self.events_to_host(w, cap, cnt, tot)
            self.sync()
            total = C.c_uint64.from_address(tot).value
            if total <= cap:
                break
            cap = total
        words = np.ctypeslib.as_array((C.c_uint64 * max(total, 1)).from_address(w))[:total].copy()
        counts = np.ctypeslib.as_array((C.c_uint32 * nc).from_address(cnt)).copy()
        return words, counts

    @staticmethod
    def expand_words(words, counts):
        """hb_expand_event_words: compact words -> hb_event records (CPU)."""
        L = lib()
        w = np.ascontiguousarray(words, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        n = C.c_uint64()
        _check("hb_expand_event_words", L.hb_expand_event_words(w.ctypes.data, len(w), c.ctypes.data, len(c), None,
                                                                0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=abi.EVENT_DTYPE)
        _check("hb_expand_event_words", L.hb_expand_event_words(w.ctypes.data, len(w), c.ctypes.data, len(c),
                                                                out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value]

    def stats(self):
        out = np.zeros(abi.HB_STAT_COUNT, dtype=np.uint64)
        _check("hb_stats", lib().hb_stats(self.h, out.ctypes.data))
        return out

    def stats_device_ptr(self):
        p = C.c_void_p()
        _check("hb_stats_device", lib().hb_stats_device(self.h, C.byref(p)))
        return p.value

    def stats_to(self, dev_ptr):
        """Async D2D copy of the last step's stats to a device buffer (torch tensor or int)."""
        _check("hb_stats_to", lib().hb_stats_to(self.h, C.c_void_p(_ptr(dev_ptr) if not isinstance(dev_ptr, int)
                                                                   else dev_ptr)))

    def set_stats_accum(self, dev_ptr):
        """Accumulate every later step's statistics into a device buffer of
        HB_STAT_COUNT u64 (torch tensor or raw pointer) inside the finish
        phase; None turns it off."""
        p = None if dev_ptr is None else (dev_ptr if isinstance(dev_ptr, int) else _ptr(dev_ptr))
        _check("hb_set_stats_accum", lib().hb_set_stats_accum(self.h, C.c_void_p(p)))

    def phase_reset(self):
        _check("hb_phase_reset", lib().hb_phase_reset(self.h))

    def step_kernels(self):
        """hb_step_kernels: HB_KERN_* bits of the kernels the last step launched."""
        m = C.c_uint32()
        _check("hb_step_kernels", lib().hb_step_kernels(self.h, C.byref(m)))
        return int(m.value)

    def steady_waves(self):
        """hb_steady_waves: group-waves of the last step that took the fast lane's
        steady path (counted only when HB_FAST_STEADY_COUNT=1 was set at create)."""
        f = lib().hb_steady_waves  # (bound here: an A/B build from before the path has no such symbol)
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]
        n = C.c_uint32()
        _check("hb_steady_waves", f(self.h, C.byref(n)))
        return int(n.value)

    def lazy_next_groups(self):
        """hb_lazy_next_groups: live groups whose Next array is not kept (every
        slot's Next == lastIndex + 1; never with HB_LAZY_NEXT=0 at create)."""
        f = lib().hb_lazy_next_groups  # (bound here: an A/B build from before the form has no such symbol)
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]
        n = C.c_uint32()
        _check("hb_lazy_next_groups", f(self.h, C.byref(n)))
        return int(n.value)

    def phase_ms(self):
        """(per-phase average ms, number of profiled steps) since phase_reset()."""
        out = np.zeros(abi.HB_PHASE_COUNT, dtype=np.float32)
        n = C.c_uint32()
        _check("hb_phase_ms", lib().hb_phase_ms(self.h, out.ctypes.data, C.byref(n)))
        return out, n.value
