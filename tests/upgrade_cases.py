"""Upgrade requests for wsg_upgrade_streams, wsg_upgrade_judge and the model
(layout.upgrade_judge): hand-written cases for every outcome and every rule of
the header walk, every prefix of one request, and seeded mutations of the
RFC 6455 1.3 request.  No native code is loaded here."""
import functools
import struct

import numpy as np

from cppserver_amd import layout

KEY = b"dGhlIHNhbXBsZSBub25jZQ=="
ACCEPT = b"s3pPLMBiTxaQ9kYGzzhZRbK+xOo="          # RFC 6455 1.3
KEY_LENGTHS = (1, 19, 20, 83, 84, 147, 148, 1000)   # len + 36 around the SHA-1 padding edges
N_FUZZ = 2000
FUZZ_SEED = 6455


def request(lines, start=b"GET /chat HTTP/1.1", body=b""):
    return b"\r\n".join([start] + list(lines)) + b"\r\n\r\n" + body


RFC_LINES = (b"Host: server.example.com", b"Upgrade: websocket", b"Connection: Upgrade",
             b"Sec-WebSocket-Key: " + KEY, b"Origin: http://example.com",
             b"Sec-WebSocket-Protocol: chat, superchat", b"Sec-WebSocket-Version: 13")
RFC_REQUEST = request(RFC_LINES)


def four(connection=b"Connection: Upgrade", upgrade=b"Upgrade: websocket", key=b"Sec-WebSocket-Key: " + KEY,
         version=b"Sec-WebSocket-Version: 13"):
    # (the key first: a failing header counts only with one of the four in front of it)
    return [b"Host: h", key, upgrade, connection, version]


def browser_request():
    """About 500 bytes with a dozen headers, as a browser sends it."""
    return request([
        b"Host: chat.example.com:8443", b"Connection: Upgrade", b"Pragma: no-cache", b"Cache-Control: no-cache",
        b"User-Agent: Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36 (KHTML, like Gecko) Chrome/126.0.0.0 "
        b"Safari/537.36", b"Upgrade: websocket", b"Origin: https://chat.example.com", b"Sec-WebSocket-Version: 13",
        b"Accept-Encoding: gzip, deflate, br, zstd", b"Accept-Language: en-GB,en-US;q=0.9,en;q=0.8",
        b"Sec-WebSocket-Key: x3JJHMbDL1EzLkh9GBhXDw==",
        b"Sec-WebSocket-Extensions: permessage-deflate; client_max_window_bits"],
        start=b"GET /rooms/lobby?session=8d1f0c2e HTTP/1.1")


def text_frame(payload, key=0):
    """One masked FIN text frame; key 0 leaves the payload as it is."""
    k = struct.pack("<I", key)
    n = len(payload)
    head = bytes([0x81, 0x80 | n]) if n < 126 else bytes([0x81, 0xFE]) + struct.pack(">H", n)
    return head + k + bytes(b ^ k[i & 3] for i, b in enumerate(payload))


def key_of_length(n, salt=0):
    return bytes(33 + (i * 7 + salt * 13 + 5) % 94 for i in range(n))   # printable, no blank, no ':'


def padded_to(length, lines=None):
    """A valid request whose header block ends at exactly ``length`` bytes
    (``\\r\\n\\r\\n`` at length - 4), by padding its first header's value."""
    lines = list(lines if lines is not None else four())
    base = len(request(lines))
    assert length >= base
    lines[0] = lines[0] + b"x" * (length - base)
    out = request(lines)
    assert len(out) == length and out.find(b"\r\n\r\n") == length - 4
    return out


@functools.lru_cache(maxsize=None)
def hand_cases():
    """(name, bytes, frames) — frames: the bytes behind the request are key-0
    text frames (or a short tail) that the classes' frame reader can be
    observed on without a GPU."""
    frames = text_frame(b"hello") + text_frame(b"") + text_frame(b"x" * 200) + text_frame(b"partial")[:8]
    c = []

    def add(name, data, has_frames=False):
        c.append((name, bytes(data), has_frames))

    add("rfc", RFC_REQUEST)
    add("browser", browser_request())
    add("four", request(four()))
    add("empty", b"")
    add("no_header_end", RFC_REQUEST[:-1])
    add("only_crlfcrlf", b"\r\n\r\n")
    # malformed HTTP
    add("line_no_space", request(four(), start=b"GET"))
    add("line_one_space", request(four(), start=b"GET /chat"))
    add("line_empty", request(four(), start=b""))
    add("header_no_colon", request(four() + [b"novalue"]))
    add("header_colon_first", request(four() + [b": value"]))
    add("header_no_colon_before_bad", request([b"Upgrade: nope", b"junk"]))
    add("clen_not_digit", request(four() + [b"Content-Length: 1x"]))
    add("clen_negative", request(four() + [b"Content-Length: -1"]))
    add("clen_not_digit_short_body", request(four() + [b"Content-Length: 5 5"], body=b"a"))
    # Content-Length
    add("clen_body", request(four() + [b"Content-Length: 5"], body=b"abcde") + frames, True)
    add("clen_short", request(four() + [b"Content-Length: 5"], body=b"abcd"))
    add("clen_empty", request(four() + [b"Content-Length:"]))
    add("clen_last_wins", request([b"Content-Length: 99"] + four() + [b"content-LENGTH:  3 "], body=b"abc"))
    add("clen_last_wins_short", request([b"Content-Length: 1"] + four() + [b"Content-Length: 4"], body=b"abc"))
    add("clen_21_digits", request(four() + [b"Content-Length: 184467440737095516163"], body=b"abc"))   # 2^64 * 10 + 3
    add("clen_huge", request(four() + [b"Content-Length: 18446744073709551615"], body=b"abc"))
    add("clen_malformed_and_bad_header", request([b"Upgrade: nope", b"Content-Length: z"]))
    # methods
    add("method_lower", request(four(), start=b"get /chat HTTP/1.1"))
    add("method_post", request(four(), start=b"POST /chat HTTP/1.1"))
    add("method_gets", request(four(), start=b"GETS /chat HTTP/1.1"))
    add("method_empty", request(four(), start=b" /chat HTTP/1.1"))
    add("url_spaces", request(four(), start=b"GET /a b c HTTP/1.1"))
    add("url_empty", request(four(), start=b"GET  HTTP/1.1"))
    # not WebSocket
    add("plain_get", request([b"Host: example.com", b"Accept: */*"], start=b"GET /index.html HTTP/1.1"))
    add("no_headers", b"GET / HTTP/1.1\r\n\r\n")
    add("no_headers_then_frames", b"GET / HTTP/1.1\r\n\r\n" + frames)
    # each header failing, missing
    add("bad_connection", request(four(connection=b"Connection: close")))
    add("bad_upgrade", request(four(upgrade=b"Upgrade: h2c")))
    add("empty_key", request([b"Upgrade: websocket", b"Sec-WebSocket-Key:", b"Connection: Upgrade",
                              b"Sec-WebSocket-Version: 13"]))
    add("blank_key", request([b"Upgrade: websocket", b"Sec-WebSocket-Key: \t ", b"Connection: Upgrade",
                              b"Sec-WebSocket-Version: 13"]))
    add("empty_key_first", request(four(key=b"Sec-WebSocket-Key:")))          # none of the four in front of it
    add("bad_upgrade_first", request([b"Upgrade: h2c"] + four()))
    add("bad_version_last", request(four() + [b"Sec-WebSocket-Version: 12"]))   # all four in front of it
    add("bad_version", request(four(version=b"Sec-WebSocket-Version: 12")))
    add("version_13_padded", request(four(version=b"Sec-WebSocket-Version: 13 \t")))
    add("version_013", request(four(version=b"Sec-WebSocket-Version: 013")))
    for i, name in enumerate(("key", "upgrade", "connection", "version")):
        lines = four()
        del lines[1 + i]
        add("missing_" + name, request(lines))
    add("only_key", request([b"Sec-WebSocket-Key: " + KEY]))
    # two failing headers, both orders; a failing one in front of and behind a missing one
    add("two_bad_upgrade_first", request([b"Upgrade: nope", b"Connection: close", b"Sec-WebSocket-Key: k",
                                          b"Sec-WebSocket-Version: 13"]))
    add("two_bad_connection_first", request([b"Connection: close", b"Upgrade: nope", b"Sec-WebSocket-Key: k",
                                             b"Sec-WebSocket-Version: 13"]))
    add("bad_version_then_empty_key", request([b"Upgrade: websocket", b"Connection: Upgrade",
                                               b"Sec-WebSocket-Version: 8", b"Sec-WebSocket-Key:"]))
    add("bad_in_front_of_missing", request([b"Upgrade: nope", b"Connection: Upgrade", b"Sec-WebSocket-Version: 13"]))
    add("bad_behind_missing", request([b"Connection: Upgrade", b"Sec-WebSocket-Version: 13", b"Upgrade: nope"]))
    add("good_headers_behind_bad", request([b"Upgrade: nope"] + four()))
    # duplicate keys: the last in front of the failure is hashed
    add("two_keys", request(four() + [b"Sec-WebSocket-Key: second"]))
    add("two_keys_then_bad", request([b"Sec-WebSocket-Key: first", b"Sec-WebSocket-Key: second", b"Upgrade: nope",
                                      b"Sec-WebSocket-Key: third"]))
    add("key_behind_bad", request([b"Upgrade: nope", b"Sec-WebSocket-Key: late"]))
    add("key_then_empty_key", request(four() + [b"Sec-WebSocket-Key:"]))
    add("duplicate_upgrade_second_bad", request(four() + [b"Upgrade: nope"]))
    # name case, blanks around ':'
    add("name_case", request([b"UPGRADE: WebSocket", b"cOnNeCtIoN: uPgRaDe", b"sec-websocket-KEY: " + KEY,
                              b"SEC-WEBSOCKET-VERSION: 13"]))
    add("blanks_around_colon", request([b"Upgrade \t:\t websocket \t", b" Connection : Upgrade", b"\tSec-WebSocket-Key\t:\t" + KEY
                                        + b" ", b"Sec-WebSocket-Version:13"]))
    add("value_with_colons", request(four(key=b"Sec-WebSocket-Key: a:b::c")))
    add("key_inner_blanks", request(four(key=b"Sec-WebSocket-Key:  a b\tc  ")))
    add("name_with_inner_blank", request(four(upgrade=b"Up grade: websocket")))
    add("name_prefix", request(four(upgrade=b"Upgrades: websocket")))
    add("blank_name", request(four() + [b" : x"]))
    # Connection values
    add("keep_alive_upgrade", request(four(connection=b"Connection: keep-alive, Upgrade")))
    add("keep_alive_blanks", request(four(connection=b"Connection: Keep-Alive ,\tupgrade")))
    add("keep_alive_cr", request(four(connection=b"Connection: keep-alive,Upgrade\r")))
    add("keep_alive_inner_vt_ff", request(four(connection=b"Connection: keep\v-alive,\fUp\ngrade")))
    add("upgrade_keep_alive", request(four(connection=b"Connection: Upgrade, keep-alive")))
    add("keep_alive_upgrade_more", request(four(connection=b"Connection: keep-alive, Upgrade, x")))
    add("keep_alive_short", request(four(connection=b"Connection: keep-alive, Upgrad")))
    add("upgrade_cr", request(four(connection=b"Connection: Upgrade\r")))
    add("connection_blank", request(four(connection=b"Connection:")))
    # bytes 0x00 and 0x80-0xFF, lone CR and LF
    add("nul_in_value", request(four(upgrade=b"Upgrade: web\x00socket")))
    add("nul_in_name", request(four(upgrade=b"Upg\x00rade: websocket")))
    add("high_in_name", request(four() + [b"X-\x80\xff\xc3\xa9: \xfe\xff\x80"]))
    add("high_case_not_folded", request(four(upgrade=b"Upgrade: websocke\xd4")))   # 0xD4 is not 't' | 0x80 folded
    add("high_key", request(four(key=b"Sec-WebSocket-Key: \x00\x80\xff\x01")))
    add("lone_lf_in_value", request(four(key=b"Sec-WebSocket-Key: ab\ncd")))
    add("lone_cr_in_value", request(four(key=b"Sec-WebSocket-Key: ab\rcd")))
    add("lone_lf_line", request([b"Upgrade: websocket\nConnection: Upgrade", b"Sec-WebSocket-Key: k",
                                 b"Sec-WebSocket-Version: 13"]))
    add("lf_only_request", RFC_REQUEST.replace(b"\r\n", b"\n"))
    add("cr_before_crlfcrlf", request(four()[:-1] + [b"Sec-WebSocket-Version: 13\r"]))
    add("crcrlf_lines", request([ln + b"\r" for ln in four()]))
    # what follows
    add("then_frames", request(four()) + frames, True)
    add("rfc_then_frames", RFC_REQUEST + frames, True)
    add("then_second_request", request(four()) + b"GET / HTTP/1.1\r\n\r\n", True)
    add("bad_then_frames", request(four(upgrade=b"Upgrade: nope")) + frames)
    add("then_masked_frames", request(four()) + text_frame(b"masked text", 0x1A2B3C4D) + text_frame(b"y" * 130, 0xDEADBEEF))
    # key lengths
    for n in KEY_LENGTHS:
        add("key_len_%d" % n, request(four(key=b"Sec-WebSocket-Key: " + key_of_length(n))))
    add("long_request", padded_to(5000))
    for n in range(len(RFC_REQUEST) + 1):
        add("prefix_%d" % n, RFC_REQUEST[:n])
    return tuple(c)


def mutate(rng, data):
    """One to three edits of ``data``: byte flips, inserts from the separator
    set and 0x00 / 0xFF, deletions, dropped or duplicated lines, truncation."""
    inserts = b" \t\r\n:,\x00\xff"
    data = bytearray(data)
    for _ in range(int(rng.integers(1, 4))):
        kind = int(rng.integers(0, 100))
        at = int(rng.integers(0, max(len(data), 1)))
        if kind < 25 and data:
            data[at] ^= 1 << int(rng.integers(0, 8))
        elif kind < 50:
            data[at:at] = bytes([inserts[int(rng.integers(0, len(inserts)))]])
        elif kind < 65 and data:
            del data[at:at + int(rng.integers(1, 4))]
        elif kind < 95:
            lines = bytes(data).split(b"\r\n")
            if len(lines) < 4:
                continue
            k = int(rng.integers(1, len(lines) - 2))   # a header line: not the request line, not the end
            if kind < 80:
                del lines[k]
            else:
                lines.insert(k, lines[k])
            data = bytearray(b"\r\n".join(lines))
        else:
            del data[at:]
    return bytes(data)


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)
    return tuple(mutate(rng, RFC_REQUEST) for _ in range(N_FUZZ))


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case's bytes: the hand cases, then the fuzz."""
    return tuple(data for _, data, _ in hand_cases()) + fuzz_cases()


@functools.lru_cache(maxsize=None)
def expected():
    """The model's outcome of every case of all_cases(), computed once."""
    return tuple(layout.upgrade_judge(data) for data in all_cases())


def pack_cases(cases):
    """The case file the C++ programs read: count, then length and bytes."""
    return struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", len(c)) + c for c in cases)


def batch(cases, align=None, gap=0):
    """The cases laid out as one wire: (wire, spans).  ``align``: every span
    starts at that offset mod 16 (None: back to back, plus ``gap`` bytes)."""
    spans = np.zeros(len(cases), dtype=layout.STREAM_SPAN)
    parts, at = [], 0
    for j, c in enumerate(cases):
        pad = gap if align is None else (align - at) % 16
        parts.append(b"\xa5" * pad)
        at += pad
        spans["off"][j], spans["len"][j] = at, len(c)
        parts.append(c)
        at += len(c)
    wire = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return wire, spans
