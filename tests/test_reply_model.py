"""layout.reply_plan (the host model of wsg_reply_messages' sizes and
offsets) against the frames the oracle's sessions send, and the ABI surface of
the two reply calls.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cppserver_amd as ca
import oracle
from cppserver_amd import layout
from tests import messages_cases as mc
from tests import reply_cases as rc


@pytest.mark.parametrize("rule", sorted(rc.RULES))
@pytest.mark.parametrize("mask", [0, 1])
def test_quirk_streams(rule, mask):
    q = mc.quirk_streams()
    streams = [q[name] for name in sorted(q)]
    keys = np.arange(len(streams), dtype=np.uint32) * 0x01010101 + rc.KEY4
    for batch in [mc.Batch(streams)] + [mc.Batch([s]) for s in streams]:
        rc.check_plan(batch, rc.RULES[rule], mask, keys[: batch.n_streams])


def test_quirk_replies_literal():
    """What the echo rule and the close rule answer to the named quirks."""
    q = mc.quirk_streams()
    one = lambda name, rule: rc.oracle_replies(mc.Batch([q[name]]), rule, 0)[0]  # noqa: E731
    assert one("continuation_after_fin", rc.ECHO) == [b"\x82\x0bhello world", b"\x82\x05again"]
    assert one("close_status_split", rc.ECHO) == [b""]
    assert one("close_status_split", rc.SAME_CLOSE_PONG) == [b"\x88\x02\x03\xe9"]
    assert one("close_one_byte", rc.SAME_CLOSE_PONG) == [b"\x88\x02\x03\xe8"]   # 1000: fewer than two bytes
    assert one("close_empty", rc.SAME_CLOSE_PONG) == [b"\x88\x02\x03\xe8"]
    # status bytes 00 00: PrepareSendFrame(op, mask, NULL, 0, 0) has no prefix
    zero = mc.Batch([[mc.raw_frame(0x88, b"\x00\x00why", key=3)]])
    assert rc.oracle_replies(zero, rc.SAME_CLOSE_PONG, 0)[0] == [b"\x88\x00"]
    msgs, *_ = rc.check_plan(zero, rc.SAME_CLOSE_PONG, 0)
    assert int(msgs["status"][0]) == 0 and int(msgs["len"][0]) == 3


def test_q2_pong_to_a_ping_carries_two_zero_bytes():
    """(WS_PONG & WS_CLOSE) == WS_CLOSE, so the pong to ping "ab"
    carries a zero status ahead of its data."""
    batch = mc.Batch([[mc.raw_frame(0x89, b"ab", key=0x11223344)]])
    assert rc.oracle_replies(batch, rc.ECHO, 0)[0] == [bytes.fromhex("8A0400006162")]
    *_, reply_off, stream_reply, rcount, wire = rc.check_plan(batch, rc.ECHO, 0)
    assert wire == bytes.fromhex("8A0400006162")
    assert list(reply_off) == [0, 6] and list(stream_reply) == [0, 6] and list(rcount) == [6, 1]
    # keyed: the prefix takes key bytes 0 and 1, the data starts at key byte 2
    keyed = rc.oracle_replies(batch, rc.ECHO, 1, [rc.KEY4])[0][0]
    k = rc.KEY4.to_bytes(4, "little")
    assert keyed == bytes([0x8A, 0x84]) + k + bytes([k[0], k[1], 0x61 ^ k[2], 0x62 ^ k[3]])


@pytest.mark.parametrize("group", range(20))
def test_random_frames(group):
    """200 seeds: up to 8 streams of up to 12 random frames (the opcodes of
    tests/test_gpu_rx_batch.py, status prefixes included), every rule."""
    for seed in range(10 * group, 10 * group + 10):
        rng = np.random.default_rng(12000 + seed)
        ns = int(rng.integers(1, 9))
        streams = [mc.random_frames(rng, int(rng.integers(0, 13)), int(rng.choice([40, 600, 70000])))
                   for _ in range(ns)]
        keys = rng.integers(0, 2**32, ns).astype(np.uint32)
        rule = rc.RULES[sorted(rc.RULES)[seed % len(rc.RULES)]]
        rc.check_plan(mc.Batch(streams), rule, seed & 1, keys)


def test_header_forms_and_seeded_state():
    rng = np.random.default_rng(1)
    batch = mc.Batch([rc.header_form_stream(rng)])
    for mask in (0, 1):
        *_, rcount, wire = rc.check_plan(batch, rc.ECHO, mask, [rc.KEY4])
        assert int(rcount[1]) == 14
    # a continuation that ends a message begun in an earlier call
    st = np.zeros(2, dtype=layout.STREAM_STATE)
    st["opcode"] = [9, 1]
    cont = mc.Batch([[mc.raw_frame(0x80, b"pinged", key=5)], [mc.raw_frame(0x80, b"text", key=6)]])
    *_, wire = rc.check_plan(cont, rc.SAME_CLOSE_PONG, 0, None, st)
    assert wire == b"\x8a\x08\x00\x00pinged" + b"\x81\x04text"


def test_reply_plan_without_messages():
    off, sr, count = layout.reply_plan(np.zeros(0, dtype=layout.MSG), rc.ECHO, 0, n_streams=3)
    assert list(off) == [0] and list(sr) == [0, 0, 0, 0] and list(count) == [0, 0]
    off, sr, count = layout.reply_plan(np.zeros(0, dtype=layout.MSG), rc.ECHO, 0)
    assert list(off) == [0] and list(sr) == [0] and list(count) == [0, 0]


def test_symbols_exported_and_declared():
    L = ca.lib()
    for name in ("wsg_reply_messages", "wsg_reply_streams"):
        assert hasattr(L, name), name
        assert getattr(L, name).restype is ctypes.c_int
    assert len(L.wsg_reply_messages.argtypes) == 19 and len(L.wsg_reply_streams.argtypes) == 21
    assert L.wsg_abi_version() == 3
    text = open(os.path.join(ca.ROOT, "include", "wsg_capi.h")).read()
    assert re.search(r"#define\s+WSG_REPLY_SAME\s+0xFF\b", text)
    assert re.search(r"#define\s+WSG_ABI_VERSION\s+3\b", text)
    for name, nargs in (("wsg_reply_messages", 19), ("wsg_reply_streams", 21)):
        (decl,) = re.findall(r"\bint %s\(([^;]*)\);" % name, text)
        assert len(decl.split(",")) == nargs
    assert ca.REPLY_SAME == 0xFF and tuple(ca.ECHO_REPLY) == (0, 0x82, 0, 0x8A, 0)


def test_null_arguments_are_refused_on_the_host():
    """The argument checks come before any device call: without a context
    the struct-free signature still loads and answers WSG_EINVAL."""
    L = ca.lib()
    n = ctypes.c_uint32(7)
    rule = bytes(ca.ECHO_REPLY)
    assert L.wsg_reply_messages(None, None, 0, None, 0, None, 0, None, rule, 0, None, None, 0, None, None, None, None,
                                None, None) == ca.WSG_EINVAL
    assert L.wsg_reply_streams(None, None, 0, None, 0, None, None, 0, None, rule, 0, None, None, 0, None, None, None,
                               None, None, ctypes.byref(n), None) == ca.WSG_EINVAL
