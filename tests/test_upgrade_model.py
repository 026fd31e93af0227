"""The upgrade handshake's rule on the CPU: layout.upgrade_judge (plain Python,
hashlib, base64) against the C++ classes it restates, against fixed answers,
and wsg_upgrade_judge (the rule the kernels run) against it, on every case of
tests/upgrade_cases.py."""
import base64
import collections
import ctypes
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import cppserver_amd as ca
from cppserver_amd import layout
from tests import upgrade_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = os.path.join(ROOT, "tests", "cpp", "_build", "upgrade_classes")


def read_frames(rest):
    """The messages and the partial tail WSSession's frame reader makes of
    whole-header FIN frames with key 0 or none: (messages, partial) in the
    form tests/cpp/upgrade_classes.cpp reports."""
    msgs, at = b"", 0
    while len(rest) - at >= 2:
        b0, b1 = rest[at], rest[at + 1]
        n, hdr = b1 & 0x7F, 2
        if n == 126:
            n, hdr = struct.unpack_from(">H", rest, at + 2)[0], 4
        assert n != 127
        if b1 & 0x80:
            assert len(rest) - at >= hdr + 4 and rest[at + hdr:at + hdr + 4] == bytes(4)
            hdr += 4
        if len(rest) - at < hdr + n:
            break
        assert b0 & 0x80
        msgs += bytes([b0 & 0x0F]) + struct.pack("<I", n) + rest[at + hdr:at + hdr + n]
        at += hdr + n
    return msgs, rest[at:]


@pytest.fixture(scope="module")
def classes(tmp_path_factory):
    """What the classes did with every case: (handshaked, response, messages, partial)."""
    d = tmp_path_factory.mktemp("upgrade")
    src, dst = str(d / "cases.bin"), str(d / "classes.bin")
    with open(src, "wb") as f:
        f.write(uc.pack_cases(uc.all_cases()))
    subprocess.run([CLASSES, src, dst], check=True, timeout=120)
    with open(dst, "rb") as f:
        out = f.read()
    res, at = [], 0
    for _ in uc.all_cases():
        hs = out[at]
        at += 1
        fields = []
        for _ in range(3):
            n, = struct.unpack_from("<I", out, at)
            fields.append(out[at + 4:at + 4 + n])
            at += 4 + n
        res.append((bool(hs), *fields))
    assert at == len(out)
    return res


def test_model_equals_the_classes(classes):
    """Bytes sent and the handshaked flag on every case, the fuzz included;
    the bytes handed on as frames wherever the frame reader can be observed
    without a device."""
    exp = uc.expected()
    names = [n for n, _, _ in uc.hand_cases()]
    for i, (data, e, (hs, resp, msgs, partial)) in enumerate(zip(uc.all_cases(), exp, classes)):
        what = names[i] if i < len(names) else "fuzz %d" % (i - len(names))
        assert resp == e["resp"], what
        assert hs == (e["code"] == layout.UP_ACCEPTED), what
    checked = 0
    for (name, data, frames), e, (hs, resp, msgs, partial) in zip(uc.hand_cases(), exp, classes):
        if not frames:
            continue
        assert e["code"] == layout.UP_ACCEPTED, name
        assert read_frames(data[e["consumed"]:]) == (msgs, partial), name
        assert msgs or partial, name
        checked += 1
    assert checked >= 4
    # a rejected or unfinished request hands nothing on
    for data, e, (hs, resp, msgs, partial) in zip(uc.all_cases(), exp, classes):
        if e["code"] != layout.UP_ACCEPTED:
            assert not msgs and not partial


def test_every_code_and_the_named_cases():
    exp = dict(zip((n for n, _, _ in uc.hand_cases()), uc.expected()))
    codes = {e["code"] for e in exp.values()}
    assert codes == set(range(layout.UP_TOO_LONG)), codes   # TOO_LONG needs max_request: below
    want = {
        "rfc": layout.UP_ACCEPTED, "browser": layout.UP_ACCEPTED, "empty": layout.UP_INCOMPLETE,
        "line_no_space": layout.UP_BAD_HTTP, "line_one_space": layout.UP_BAD_HTTP,
        "header_no_colon": layout.UP_BAD_HTTP, "header_colon_first": layout.UP_BAD_HTTP,
        "clen_not_digit": layout.UP_BAD_HTTP, "clen_not_digit_short_body": layout.UP_BAD_HTTP,
        "clen_body": layout.UP_ACCEPTED, "clen_short": layout.UP_INCOMPLETE, "clen_21_digits": layout.UP_ACCEPTED,
        "clen_huge": layout.UP_INCOMPLETE, "method_lower": layout.UP_NOT_GET, "method_post": layout.UP_NOT_GET,
        "plain_get": layout.UP_NOT_WEBSOCKET, "no_headers": layout.UP_NOT_WEBSOCKET,
        "bad_connection": layout.UP_BAD_CONNECTION, "bad_upgrade": layout.UP_BAD_UPGRADE,
        "empty_key": layout.UP_EMPTY_KEY, "bad_version": layout.UP_BAD_VERSION,
        "missing_key": layout.UP_MISSING, "only_key": layout.UP_MISSING, "blank_key": layout.UP_EMPTY_KEY,
        "empty_key_first": layout.UP_NOT_WEBSOCKET, "bad_upgrade_first": layout.UP_NOT_WEBSOCKET,
        "bad_version_last": layout.UP_ACCEPTED, "two_bad_upgrade_first": layout.UP_NOT_WEBSOCKET,
        "bad_in_front_of_missing": layout.UP_NOT_WEBSOCKET, "good_headers_behind_bad": layout.UP_NOT_WEBSOCKET,
        "two_keys_then_bad": layout.UP_BAD_UPGRADE, "key_behind_bad": layout.UP_NOT_WEBSOCKET,
        "duplicate_upgrade_second_bad": layout.UP_ACCEPTED, "keep_alive_short": layout.UP_BAD_CONNECTION,
        "keep_alive_upgrade_more": layout.UP_BAD_CONNECTION, "upgrade_cr": layout.UP_BAD_CONNECTION,
        "keep_alive_inner_vt_ff": layout.UP_ACCEPTED, "nul_in_value": layout.UP_BAD_UPGRADE,
        "nul_in_name": layout.UP_MISSING, "high_case_not_folded": layout.UP_BAD_UPGRADE,
        "name_with_inner_blank": layout.UP_MISSING, "name_prefix": layout.UP_MISSING,
        "version_13_padded": layout.UP_ACCEPTED, "version_013": layout.UP_BAD_VERSION,
        "lone_lf_in_value": layout.UP_ACCEPTED, "lone_cr_in_value": layout.UP_ACCEPTED,
        "lf_only_request": layout.UP_INCOMPLETE, "crcrlf_lines": layout.UP_BAD_UPGRADE,
        "bad_then_frames": layout.UP_BAD_UPGRADE, "only_crlfcrlf": layout.UP_BAD_HTTP,
        "line_empty": layout.UP_BAD_HTTP, "url_spaces": layout.UP_ACCEPTED, "method_gets": layout.UP_NOT_GET,
        "method_empty": layout.UP_NOT_GET, "clen_last_wins": layout.UP_ACCEPTED,
        "clen_last_wins_short": layout.UP_INCOMPLETE, "clen_empty": layout.UP_ACCEPTED,
        "clen_malformed_and_bad_header": layout.UP_BAD_HTTP, "header_no_colon_before_bad": layout.UP_BAD_HTTP,
        "two_bad_connection_first": layout.UP_NOT_WEBSOCKET,       # nothing seen in front of the failure
        "bad_version_then_empty_key": layout.UP_BAD_VERSION, "bad_behind_missing": layout.UP_BAD_UPGRADE,
        "key_then_empty_key": layout.UP_ACCEPTED,                  # all four in front of the failure
        "keep_alive_upgrade": layout.UP_ACCEPTED, "keep_alive_blanks": layout.UP_ACCEPTED,
        "keep_alive_cr": layout.UP_ACCEPTED, "upgrade_keep_alive": layout.UP_BAD_CONNECTION,
        "name_case": layout.UP_ACCEPTED, "blanks_around_colon": layout.UP_ACCEPTED,
        "then_frames": layout.UP_ACCEPTED, "then_second_request": layout.UP_ACCEPTED,
        "long_request": layout.UP_ACCEPTED,
    }
    for name, code in want.items():
        assert exp[name]["code"] == code, name
    cases = dict((n, d) for n, d, _ in uc.hand_cases())
    assert exp["clen_21_digits"]["consumed"] == len(cases["clen_21_digits"])   # 2^64 * 10 + 3 wraps to 3
    assert exp["clen_huge"]["need"] == layout.U64_MAX
    assert (exp["clen_short"]["consumed"], exp["clen_short"]["need"]) == (0, len(cases["clen_short"]) + 1)
    # duplicate keys: the last in front of the failure
    for name, key in (("two_keys", b"second"), ("two_keys_then_bad", b"second"), ("key_inner_blanks", b"a b\tc")):
        off, n = exp[name]["key"]
        assert cases[name][off:off + n] == key, name
    assert exp["two_keys"]["resp"] == layout.upgrade_response(layout.UP_ACCEPTED, b"second")
    # every prefix of the request is incomplete, the whole accepted
    for n in range(len(uc.RFC_REQUEST)):
        assert exp["prefix_%d" % n]["code"] == layout.UP_INCOMPLETE and exp["prefix_%d" % n]["consumed"] == 0
    assert exp["prefix_%d" % len(uc.RFC_REQUEST)]["code"] == layout.UP_ACCEPTED


def test_fixed_answers():
    """RFC 6455 1.3, OpenSSL (wsg_ws_accept), hashlib at the SHA-1 padding edges."""
    e = layout.upgrade_judge(uc.RFC_REQUEST)
    assert b"Sec-WebSocket-Accept: " + uc.ACCEPT + b"\r\n" in e["resp"] and len(e["resp"]) == 148
    assert layout.ws_accept(uc.KEY) == uc.ACCEPT
    for n in uc.KEY_LENGTHS:
        key = uc.key_of_length(n)
        want = base64.b64encode(hashlib.sha1(key + b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11").digest())
        out = ctypes.create_string_buffer(64)
        assert ca.lib().wsg_ws_accept(key, len(key), out, 64) == 0 and out.value == want
        req = uc.request(uc.four(key=b"Sec-WebSocket-Key: " + key))
        for resp in (layout.upgrade_judge(req)["resp"], ca.upgrade_judge(req)[2]):
            assert resp[97:125] == want and len(resp) == 148, n


def test_response_sizes():
    sizes = {code: len(layout.upgrade_response(code)) for code in range(layout.UP_TOO_LONG + 1)}
    assert sizes[layout.UP_ACCEPTED] == 148 and max(sizes.values()) == 196 == layout.UPGRADE_RESP_MAX
    assert [c for c, n in sizes.items() if n == 0] == [layout.UP_INCOMPLETE, layout.UP_NOT_GET,
                                                       layout.UP_NOT_WEBSOCKET, layout.UP_TOO_LONG]


def check_judge(data, e, max_request=0):
    rc, rec, resp, consumed, need = ca.upgrade_judge(data, max_request)
    assert rc == 0
    assert (int(rec["code"]), int(rec["status"]), int(rec["resp_len"]), int(rec["_pad"])) == (
        e["code"], e["status"], len(e["resp"]), 0)
    assert resp == e["resp"] and consumed == e["consumed"] and need == e["need"]
    assert (int(rec["key_off"]), int(rec["key_len"])) == e["key"]
    whole = e["code"] not in (layout.UP_INCOMPLETE, layout.UP_TOO_LONG, layout.UP_BAD_HTTP)
    assert (int(rec["url_off"]), int(rec["url_len"])) == (e["url"] if whole else (0, 0))


def test_judge_equals_the_model():
    for data, e in zip(uc.all_cases(), uc.expected()):
        check_judge(data, e)


def test_judge_max_request():
    short = uc.RFC_REQUEST[:100]
    body = uc.request(uc.four() + [b"Content-Length: 50"], body=b"abc")
    for data in (short, body, b""):
        for limit in (len(data) - 1, len(data), len(data) + 1):
            if limit < 0:
                continue
            e = layout.upgrade_judge(data, limit)
            assert e["code"] == (layout.UP_TOO_LONG if 0 < limit <= len(data) else layout.UP_INCOMPLETE)
            check_judge(data, e, limit)
    e = layout.upgrade_judge(uc.RFC_REQUEST, 10)   # a whole request is judged whatever the limit
    assert e["code"] == layout.UP_ACCEPTED
    check_judge(uc.RFC_REQUEST, e, 10)


def test_judge_capacity_and_arguments():
    rc, rec, resp, consumed, need = ca.upgrade_judge(uc.RFC_REQUEST, resp_cap=147)
    assert rc == ca.WSG_ENOMEM and int(rec["resp_len"]) == 148 and consumed == len(uc.RFC_REQUEST)
    assert ca.upgrade_judge(uc.RFC_REQUEST, resp_cap=148)[0] == 0
    assert ca.upgrade_judge(b"GET", resp_cap=0)[0] == 0
    rec = np.zeros(1, dtype=layout.UPGRADE_DTYPE)
    assert ca.lib().wsg_upgrade_judge(None, 4, 0, ca._np_ptr(rec), None, 0, None, None) == ca.WSG_EINVAL
    assert ca.lib().wsg_upgrade_judge(b"GET", 3, 0, None, None, 0, None, None) == ca.WSG_EINVAL
    assert ca.lib().wsg_upgrade_judge(b"GET", 3, 0, ca._np_ptr(rec), None, 8, None, None) == ca.WSG_EINVAL


def test_fuzz_mix():
    """A condition on the fuzz: at most a quarter of it incomplete or
    malformed HTTP, at least six distinct codes."""
    codes = collections.Counter(e["code"] for e in uc.expected()[len(uc.hand_cases()):])
    assert sum(codes.values()) == uc.N_FUZZ == 2000
    print(sorted(codes.items()))
    assert codes[layout.UP_INCOMPLETE] + codes[layout.UP_BAD_HTTP] <= uc.N_FUZZ // 4
    assert len(codes) >= 6


def test_upgrade_plan_tables():
    """The batch form: offsets, counts, a bad span among good ones."""
    cases = [uc.RFC_REQUEST, b"", uc.request(uc.four(upgrade=b"Upgrade: nope")), uc.RFC_REQUEST[:50],
             uc.request(uc.four()) + b"tail"]
    wire, spans = uc.batch(cases, gap=3)
    spans["off"][3] = len(wire) - 10   # runs past the wire
    spans["len"][3] = 50
    up, consumed, need, resp_off, resp, count, bad = layout.upgrade_plan(wire, spans)
    assert list(bad) == [False, False, False, True, False]
    assert list(up["code"]) == [1, 0, layout.UP_BAD_UPGRADE, 0, 1]
    assert list(resp_off) == [0, 148, 148, 148 + 169, 148 + 169, 2 * 148 + 169] and len(resp) == 2 * 148 + 169
    assert list(count) == [2, 1, 2, 2 * 148 + 169]
    assert int(up["key_off"][4]) == int(spans["off"][4]) + cases[4].find(uc.KEY)
    assert list(consumed) == [len(cases[0]), 0, len(cases[2]), 0, len(cases[4]) - 4]
