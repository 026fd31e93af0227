"""wsg_decode_messages without a GPU: the record layouts against the header,
the exported symbol, and layout.message_plan (the plan pass restated in numpy)
against the oracle's sessions — every stream's records that fire a callback,
read out of the oracle-unmasked bytes at the planned offsets, must be exactly
what one PrepareReceiveFrame session delivers (kind, data, status, in order)."""
import ctypes
import os
import re

import numpy as np
import pytest

import cppserver_amd as ca
from cppserver_amd import layout
from tests import messages_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32,
          "uint8_t": ctypes.c_uint8}


def header_struct(name):
    """typedef struct <name> of include/wsg_capi.h as a ctypes.Structure."""
    text = open(os.path.join(ROOT, "include", "wsg_capi.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, field, dim in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body):
        fields.append((field, CTYPES[ctype] * int(dim) if dim else CTYPES[ctype]))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("name,dtype,size", [("wsg_msg", layout.MSG, 40),
                                             ("wsg_stream_state", layout.STREAM_STATE, 8)])
def test_struct_layout_matches_header(name, dtype, size):
    st = header_struct(name)
    assert ctypes.sizeof(st) == dtype.itemsize == size
    assert [f for f, _ in st._fields_] == list(dtype.names)
    for field, _ in st._fields_:
        assert getattr(st, field).offset == dtype.fields[field][1], field


def test_symbol_exported_and_abi_stays_3():
    L = ctypes.CDLL(ca.LIB_PATH)
    assert hasattr(L, "wsg_decode_messages")
    assert ca.lib().wsg_abi_version() == 3


@pytest.mark.parametrize("name", ["rfc_fragmented_hello", "q5_continuation_concat"])
def test_kat_vectors(name):
    frames, events = mc.kat_stream(name)
    msgs, count, state, buf, _, _ = mc.check_model(mc.Batch([frames]))
    assert mc.records_events(msgs, buf, 0) == events
    assert int(msgs[0]["nframes"]) == 2 and int(state["consumed"][0]) == 2


@pytest.mark.parametrize("name", sorted(mc.quirk_streams()))
def test_quirk_stream_alone(name):
    mc.check_model(mc.Batch([mc.quirk_streams()[name]]))


def test_quirk_expectations():
    """What the reference does with the quirk streams, spelled out."""
    q = mc.quirk_streams()
    names = ["continuation_after_fin", "ping_inside_text", "close_one_byte", "close_status_split",
             "unknown_opcode_3", "tail_only", "empty", "close_empty"]
    msgs, count, state, buf, _, _ = mc.check_model(mc.Batch([q[k] for k in names]))
    ev = [mc.records_events(msgs, buf, j) for j in range(len(names))]
    assert ev[0] == [(1, b"hello world", 0), (1, b"again", 0)]
    # "ab" + the ping's (status-prefixed) payload go to onWSPing; the 0x80 frame is another ping
    assert [e[0] for e in ev[1]] == [3, 3, 1] and ev[1][0][1].startswith(b"ab") and ev[1][1][1] == b"cd"
    assert ev[2] == [(2, b"\x03", 1000)]
    assert ev[3] == [(2, b"gone", 0x03E9)]
    assert ev[4] == [(1, b"ok", 0)]
    unknown = msgs[msgs["stream"] == 4]
    assert list(unknown["kind"]) == [0, 0, 1] and list(unknown["opcode"]) == [3, 3, 1]
    assert [int(x) for x in unknown["len"]] == [3, 1, 2]          # the record and its bytes are still produced
    assert ev[5] == [] and int(state["consumed"][5]) == 0 and int(state["opcode"][5]) == 0
    assert ev[6] == [] and int(state["consumed"][6]) == 0
    assert ev[7] == [(2, b"", 1000)]
    assert list(state["consumed"][:5]) == [4, 4, 1, 4, 3]
    assert list(state["opcode"][:5]) == [1, 1, 8, 8, 1]


def test_all_quirks_with_empty_streams_between():
    q = mc.quirk_streams()
    streams = []
    for k in sorted(q):
        streams += [q[k], []]
    msgs, count, state, _, _, _ = mc.check_model(mc.Batch([[]] + streams))
    assert np.array_equal(msgs["first_frame"] + msgs["nframes"] - 1,
                          np.flatnonzero(mc.Batch([[]] + streams).oracle_decode()[1]["fin"]))


@pytest.mark.parametrize("seed", range(20))
def test_random_streams(seed):
    rng = np.random.default_rng(7000 + seed)
    streams = [mc.random_frames(rng, int(rng.integers(0, 12)), 300) for _ in range(int(rng.integers(1, 10)))]
    mc.check_model(mc.Batch(streams))


@pytest.mark.parametrize("seed", range(20))
def test_carry_over(seed):
    """Each stream cut at a random frame into two calls: the second takes the
    first's tail, the rest and the returned state; together they deliver what
    one session fed the whole stream delivers."""
    rng = np.random.default_rng(7100 + seed)
    streams = [mc.random_frames(rng, int(rng.integers(0, 14)), 200) for _ in range(int(rng.integers(1, 8)))]
    cuts = [int(rng.integers(0, len(s) + 1)) for s in streams]
    first = mc.Batch([s[:c] for s, c in zip(streams, cuts)])
    m1, _, st1, buf1, _, _ = mc.check_model(first)
    second = mc.Batch([s[int(st1["consumed"][j]):] for j, s in enumerate(streams)])
    m2, _, st2, buf2, _, _ = mc.check_model(second, st1)
    for j, s in enumerate(streams):
        got = mc.records_events(m1, buf1, j) + mc.records_events(m2, buf2, j)
        assert got == mc.session_events(s), "stream %d" % j
        whole = mc.check_model(mc.Batch([s]))[2]
        assert int(st1["consumed"][j]) + int(st2["consumed"][j]) == int(whole["consumed"][0])
        assert int(st2["opcode"][j]) == int(whole["opcode"][0]) or int(whole["consumed"][0]) == 0
