"""The contract of hb_set_egress_logterm (CPU): the three symbols, the constant
in the header and in abi.py, HB_EINVAL without a handle, and the values that must not move
(the library loads without touching the GPU)."""
import os
import re

from etcd_amd import abi, hipbatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "hipbatch.h")


def test_symbols_constants_and_null_handle():
    L = hipbatch.lib()
    for sym in ("hb_set_egress_logterm", "hb_egress_logterm", "hb_egress_logterm_caps"):
        assert hasattr(L, sym), sym
    assert abi.HB_EGRESS_LOGTERM_V1 == 1 and L.hb_egress_logterm_caps() == abi.HB_EGRESS_LOGTERM_V1
    assert L.hb_set_egress_logterm(None, 1) == abi.HB_EINVAL
    assert L.hb_set_egress_logterm(None, 0) == abi.HB_EINVAL
    assert L.hb_egress_logterm(None) == abi.HB_EINVAL
    # a knob of its own: the mode bits, the other knobs' bits and the version are what they were
    assert L.hb_egress_caps() == 7 == abi.HB_EGRESS_ON | abi.HB_EGRESS_VOTES | abi.HB_EGRESS_APPS
    assert L.hb_egress_limit_caps() == abi.HB_EGRESS_LIMIT_V1 == 1
    assert L.hb_wire_props_caps() == abi.HB_WIRE_PROPS_IN | abi.HB_WIRE_PROPS_OUT
    assert L.hb_encode_caps() == abi.HB_ENCODE_ENTS and L.hb_frame_caps() == abi.HB_FRAME_V1
    assert L.hb_decode_caps() & abi.HB_DECODE_FOLLOW
    assert L.hb_abi_version() == abi.HB_ABI_VERSION == 8
    assert L.hb_egress_mode(None) == abi.HB_EINVAL and L.hb_egress_limit(None) == abi.HB_EINVAL


def test_header_and_abi_agree():
    txt = open(HDR).read()
    for name, val in (("HB_EGRESS_LOGTERM_V1", abi.HB_EGRESS_LOGTERM_V1), ("HB_EGRESS_LIMIT_V1", abi.HB_EGRESS_LIMIT_V1),
                      ("HB_ABI_VERSION", abi.HB_ABI_VERSION), ("HB_EGRESS_APPS", abi.HB_EGRESS_APPS)):
        assert re.search(rf"^#define\s+{name}\s+{val}\b", txt, re.M), name
    for proto in (r"int\s+hb_set_egress_logterm\(hb_handle\* h, int on\);", r"int\s+hb_egress_logterm\(hb_handle\* h\);",
                  r"int\s+hb_egress_logterm_caps\(void\);"):
        assert re.search(proto, txt), proto
    assert hasattr(hipbatch.Engine, "set_egress_logterm") and hasattr(hipbatch.Engine, "egress_logterm")
    assert hasattr(hipbatch.Engine, "set_egress_limit") and hasattr(hipbatch.Engine, "set_egress")
