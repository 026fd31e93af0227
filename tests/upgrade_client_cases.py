"""Upgrade responses for wsg_upgrade_client_streams, wsg_upgrade_client_judge
and the model (layout.upgrade_client_judge): hand-written cases for every
outcome and every clause of the rule, every prefix of one response, and seeded
mutations of the RFC 6455 1.3 response.  Every case is (name, bytes, nonce).
No native code is loaded here."""
import base64
import functools
import struct

import numpy as np

from cppserver_amd import layout
from tests.upgrade_cases import mutate as mutate_bytes

NONCE = b"the sample nonce"
KEY = b"dGhlIHNhbXBsZSBub25jZQ=="
ACCEPT = b"s3pPLMBiTxaQ9kYGzzhZRbK+xOo="          # RFC 6455 1.3
N_FUZZ = 2000
FUZZ_SEED = 6455
NUL_TRIES = 20000   # a digest starts with NUL once in 256 nonces


def response(lines, start=b"HTTP/1.1 101 Switching Protocols", body=b""):
    return b"\r\n".join([start] + list(lines)) + b"\r\n\r\n" + body


RFC_LINES = (b"Upgrade: websocket", b"Connection: Upgrade", b"Sec-WebSocket-Accept: " + ACCEPT,
             b"Sec-WebSocket-Protocol: chat")
RFC_RESPONSE = response(RFC_LINES)


def digest(nonce):
    return layout.upgrade_expect(nonce)


def accept_of(nonce):
    return base64.b64encode(digest(nonce))


def server_response(nonce):
    """The 148 bytes wsg_upgrade_streams answers that nonce's request with."""
    return layout.upgrade_response(layout.UP_ACCEPTED, base64.b64encode(nonce))


def three(connection=b"Connection: Upgrade", upgrade=b"Upgrade: websocket", accept=b"Sec-WebSocket-Accept: " + ACCEPT):
    return [b"Server: s", connection, upgrade, accept]


def unmasked_text(payload):
    n = len(payload)
    head = bytes([0x81, n]) if n < 126 else bytes([0x81, 126]) + struct.pack(">H", n)
    return head + payload


def padded_to(length, lines=None):
    """A valid response whose header block ends at exactly ``length`` bytes,
    by padding its first header's value."""
    lines = list(lines if lines is not None else three())
    base = len(response(lines))
    assert length >= base
    lines[0] = lines[0] + b"x" * (length - base)
    out = response(lines)
    assert len(out) == length and out.find(b"\r\n\r\n") == length - 4
    return out


def _find_nonce(rng, want):
    for _ in range(NUL_TRIES):
        nonce = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        if want(digest(nonce)):
            return nonce
    raise AssertionError("no nonce found in %d tries" % NUL_TRIES)


@functools.lru_cache(maxsize=None)
def nul_nonces():
    """(inner, k, first): a nonce whose digest's first NUL is at k in 1..18,
    and one whose digest starts with NUL."""
    rng = np.random.default_rng(1303)
    inner = _find_nonce(rng, lambda d: 1 <= d.find(b"\x00") <= 18)
    first = _find_nonce(rng, lambda d: d[0] == 0)
    return inner, digest(inner).find(b"\x00"), first


def _flip(d, at):
    return d[:at] + bytes([d[at] ^ 0x55]) + d[at + 1:]


@functools.lru_cache(maxsize=None)
def hand_cases():
    frames = unmasked_text(b"hello") + unmasked_text(b"") + unmasked_text(b"x" * 200) + unmasked_text(b"partial")[:4]
    c = []

    def add(name, data, nonce=NONCE):
        c.append((name, bytes(data), bytes(nonce)))

    D = digest(NONCE)
    assert b"\x00" not in D   # the wrong-byte cases below are judged at their byte

    def acc(raw):
        return b"Sec-WebSocket-Accept: " + raw

    def b64(raw):
        return base64.b64encode(raw)

    add("rfc", RFC_RESPONSE)
    add("server_101", server_response(NONCE))
    add("three", response(three()))
    add("empty", b"")
    add("no_header_end", RFC_RESPONSE[:-1])
    add("only_crlfcrlf", b"\r\n\r\n")
    add("other_nonce", RFC_RESPONSE, b"another nonce 16")
    # the status line
    add("status_no_reason", response(three(), start=b"HTTP/1.1 101"))
    add("status_empty_reason", response(three(), start=b"HTTP/1.1 101 "))
    add("status_two_spaces", response(three(), start=b"HTTP/1.1  101 Switching"))
    add("status_no_digits", response(three(), start=b"HTTP/1.1 abc Switching"))
    add("status_four_digits", response(three(), start=b"HTTP/1.1 1010 Switching"))
    add("status_two_digits", response(three(), start=b"HTTP/1.1 10 Switching"))
    add("status_ten_digits", response(three(), start=b"HTTP/1.1 4294967397 x"))    # 101 mod 2^32
    add("status_twenty_digits", response(three(), start=b"HTTP/1.1 99999999999999999999 x"))
    add("status_leading_space", response(three(), start=b" HTTP/1.1 101 Switching"))
    add("status_line_empty", response(three(), start=b""))
    add("status_no_space", response(three(), start=b"HTTP/1.1"))
    add("status_digit_then_letter", response(three(), start=b"HTTP/1.1 10x OK"))
    add("status_plus", response(three(), start=b"HTTP/1.1 +01 OK"))
    add("status_tab", response(three(), start=b"HTTP/1.1\t101 OK"))
    add("status_000", response(three(), start=b"HTTP/1.1 000 OK"))
    add("status_any_protocol", response(three(), start=b"x 101"))
    add("status_200_body", response([b"Content-Length: 5"], start=b"HTTP/1.1 200 OK", body=b"hello"))
    add("status_400_body", layout.upgrade_response(layout.UP_BAD_UPGRADE))
    add("status_400_short_body", layout.upgrade_response(layout.UP_BAD_UPGRADE)[:-1])
    add("status_200_with_three", response(three(), start=b"HTTP/1.1 200 OK"))
    add("status_100", response(three(), start=b"HTTP/1.1 100 Continue"))
    # malformed header lines
    add("header_no_colon", response(three() + [b"novalue"]))
    add("header_colon_first", response(three() + [b": value"]))
    add("header_no_colon_before_bad", response([b"Upgrade: nope", b"junk"]))
    add("bad_status_and_bad_header", response([b"junk"], start=b"HTTP/1.1 1x1 OK"))
    # Content-Length
    add("clen_body_then_frames", response(three() + [b"Content-Length: 5"], body=b"abcde") + frames)
    add("clen_short", response(three() + [b"Content-Length: 5"], body=b"abcd"))
    add("clen_empty", response(three() + [b"Content-Length:"]))
    add("clen_not_digit", response(three() + [b"Content-Length: 1x"]))
    add("clen_not_digit_short_body", response(three() + [b"Content-Length: 5 5"], body=b"a"))
    add("clen_last_wins", response([b"Content-Length: 99"] + three() + [b"content-LENGTH:  3 "], body=b"abc"))
    add("clen_last_wins_short", response([b"Content-Length: 1"] + three() + [b"Content-Length: 4"], body=b"abc"))
    add("clen_21_digits", response(three() + [b"Content-Length: 184467440737095516163"], body=b"abc"))
    add("clen_huge", response(three() + [b"Content-Length: 18446744073709551615"], body=b"abc"))
    add("clen_not_101_short", response([b"Content-Length: 9"], start=b"HTTP/1.1 404 Not Found", body=b"12345678"))
    # each header wrong, missing, duplicated, wrong behind a complete set
    add("bad_connection", response(three(connection=b"Connection: close")))
    add("bad_upgrade", response(three(upgrade=b"Upgrade: h2c")))
    add("bad_accept", response(three(accept=acc(b64(_flip(D, 3))))))
    for i, name in enumerate(("connection", "upgrade", "accept")):
        lines = three()
        del lines[1 + i]
        add("missing_" + name, response(lines))
    add("no_headers", b"HTTP/1.1 101 Switching Protocols\r\n\r\n")
    add("only_accept", response([acc(ACCEPT)]))
    add("duplicate_connection", response(three() + [b"Connection: Upgrade"]))
    add("duplicate_upgrade_second_bad", response(three() + [b"Upgrade: nope"]))
    add("duplicate_connection_second_bad", response(three() + [b"Connection: close"]))
    add("duplicate_accept_second_bad", response(three() + [acc(b64(_flip(D, 0)))]))
    add("duplicate_accept_first_bad", response([acc(b64(_flip(D, 0)))] + three()))
    add("two_accepts_both_good", response(three() + [acc(ACCEPT + b" ")]))
    add("bad_upgrade_first", response([b"Upgrade: h2c"] + three()))
    add("two_bad_upgrade_first", response([b"Upgrade: nope", b"Connection: close", acc(ACCEPT)]))
    add("two_bad_connection_first", response([b"Connection: close", b"Upgrade: nope", acc(ACCEPT)]))
    add("bad_accept_then_bad_upgrade", response([b"Connection: Upgrade", acc(b"AAAA"), b"Upgrade: nope"]))
    add("bad_in_front_of_missing", response([b"Upgrade: nope", b"Connection: Upgrade"]))
    add("bad_behind_missing", response([b"Connection: Upgrade", b"Upgrade: nope"]))
    add("accept_behind_bad", response([b"Connection: Upgrade", b"Upgrade: nope", acc(ACCEPT)]))
    # name case, blanks
    add("name_case", response([b"UPGRADE: WebSocket", b"cOnNeCtIoN: uPgRaDe", b"sec-websocket-ACCEPT: " + ACCEPT]))
    add("blanks_around_colon", response([b"Upgrade \t:\t websocket \t", b" Connection : Upgrade",
                                         b"\tSec-WebSocket-Accept\t:\t" + ACCEPT + b" "]))
    add("name_with_inner_blank", response(three(accept=b"Sec-WebSocket -Accept: " + ACCEPT)))
    add("name_prefix", response(three(accept=b"Sec-WebSocket-Accepted: " + ACCEPT)))
    add("name_short", response(three(accept=b"Sec-WebSocket-Accep: " + ACCEPT)))
    add("name_key", response(three() + [b"Sec-WebSocket-Key:", b"Sec-WebSocket-Version: 12"]))   # the server's names: nothing here
    add("value_with_colons", response(three(accept=acc(ACCEPT[:10] + b":::" + ACCEPT[10:]))))
    # Connection values
    add("keep_alive_upgrade", response(three(connection=b"Connection: keep-alive, Upgrade")))
    add("keep_alive_squeezed", response(three(connection=b"Connection: keep-alive,Upgrade")))
    add("upgrade_cr", response(three(connection=b"Connection: Upgrade\r")))
    add("connection_blank", response(three(connection=b"Connection:")))
    add("upgrade_upper", response(three(upgrade=b"Upgrade: WEBSOCKET")))
    # bytes 0x00 and 0x80-0xFF, lone CR and LF
    add("nul_in_value", response(three(upgrade=b"Upgrade: web\x00socket")))
    add("nul_in_name", response(three(upgrade=b"Upg\x00rade: websocket")))
    add("high_in_name", response(three() + [b"X-\x80\xff\xc3\xa9: \xfe\xff\x80"]))
    add("high_case_not_folded", response(three(upgrade=b"Upgrade: websocke\xd4")))
    add("high_in_accept", response(three(accept=acc(ACCEPT[:5] + b"\x80\xff\x00\xc1" + ACCEPT[5:]))))
    add("lone_lf_in_accept", response(three(accept=acc(ACCEPT[:7] + b"\n" + ACCEPT[7:]))))
    add("lone_cr_in_accept", response(three(accept=acc(ACCEPT[:7] + b"\r" + ACCEPT[7:]))))
    add("lone_lf_line", response([b"Upgrade: websocket\nConnection: Upgrade", acc(ACCEPT)]))
    add("lf_only_response", RFC_RESPONSE.replace(b"\r\n", b"\n"))
    add("crcrlf_lines", response([ln + b"\r" for ln in three()]))
    # what follows
    add("then_frames", response(three()) + frames)
    add("rfc_then_frames", RFC_RESPONSE + frames)
    add("server_101_then_frames", server_response(NONCE) + frames)
    add("bad_then_frames", response(three(upgrade=b"Upgrade: nope")) + frames)
    add("not_101_then_frames", response(three(), start=b"HTTP/1.1 200 OK") + frames)
    # accept values
    add("accept_empty", response(three(accept=acc(b""))))
    add("accept_blank", response(three(accept=acc(b" \t "))))
    add("accept_only_foreign", response(three(accept=acc(b"==-_.."))))
    add("accept_one_letter", response(three(accept=acc(b"Z"))))   # six bits: no byte
    for n in (1, 19, 20):
        add("accept_prefix_%d" % n, response(three(accept=acc(b64(D[:n])))))
    add("accept_21", response(three(accept=acc(b64(D + b"\x9c")))))
    add("accept_40", response(three(accept=acc(b64(D + bytes(range(200, 220)))))))
    for at in (0, 10, 19):
        add("accept_wrong_at_%d" % at, response(three(accept=acc(b64(_flip(D, at))))))
        add("accept_wrong_at_%d_short" % at, response(three(accept=acc(b64(_flip(D, at)[:at + 1])))))
    add("accept_wrong_at_20", response(three(accept=acc(b64(_flip(D + b"\x07", 20))))))
    add("accept_scattered", response(three(accept=acc(b"= ".join(ACCEPT[i:i + 3] for i in range(0, 27, 3)) + b"-_="))))
    add("accept_27_letters", response(three(accept=acc(ACCEPT[:27]))))
    add("accept_26_letters", response(three(accept=acc(ACCEPT[:26]))))   # 19 bytes
    add("accept_padding_first", response(three(accept=acc(b"====" + ACCEPT))))
    add("accept_lower", response(three(accept=acc(ACCEPT.lower()))))
    add("accept_urlsafe", response(three(accept=acc(ACCEPT.replace(b"+", b"-")))))   # '-' is skipped: the bits shift
    # NUL bytes in the digest
    inner, k, first = nul_nonces()
    Di, Df = digest(inner), digest(first)
    add("nul_inner_right", response(three(accept=acc(b64(Di)))), inner)
    add("nul_inner_differs_behind", response(three(accept=acc(b64(Di[:k + 1] + bytes(b ^ 0xFF for b in Di[k + 1:]))))), inner)
    add("nul_inner_differs_in_front", response(three(accept=acc(b64(_flip(Di, k - 1))))), inner)
    add("nul_inner_differs_at", response(three(accept=acc(b64(_flip(Di, k))))), inner)
    add("nul_first_right", response(three(accept=acc(b64(Df)))), first)
    add("nul_first_anything_behind", response(three(accept=acc(b"AAAA////"))), first)
    add("nul_first_differs", response(three(accept=acc(b64(_flip(Df, 0))))), first)
    add("long_response", padded_to(5000))
    for n in range(len(RFC_RESPONSE) + 1):
        add("prefix_%d" % n, RFC_RESPONSE[:n])
    return tuple(c)


def mutate(rng, data):
    """tests/upgrade_cases.mutate, and one time in four an edit aimed at the
    client's rule first: another status, a letter of the accept value, a
    header's value."""
    if int(rng.integers(0, 4)) == 0:
        kind = int(rng.integers(0, 3))
        if kind == 0:
            data = data.replace(b" 101 ", b" %d " % int(rng.integers(95, 1005)), 1)
        elif kind == 1:
            at = data.find(b"Accept: ") + 8 + int(rng.integers(0, 28))
            data = data[:at] + bytes([b"AZaz09+/=- "[int(rng.integers(0, 11))]]) + data[at + 1:]
        else:
            old, new = ((b"websocket", b"websocked"), (b": Upgrade", b": upgrade,"))[int(rng.integers(0, 2))]
            data = data.replace(old, new, 1)
        if int(rng.integers(0, 2)):
            return data
    return mutate_bytes(rng, data)


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)
    return tuple(("fuzz_%d" % i, mutate(rng, RFC_RESPONSE), NONCE) for i in range(N_FUZZ))


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case as (bytes, nonce): the hand cases, then the fuzz."""
    return tuple((data, nonce) for _, data, nonce in hand_cases() + fuzz_cases())


@functools.lru_cache(maxsize=None)
def expected():
    """The model's outcome of every case of all_cases(), computed once."""
    return tuple(layout.upgrade_client_judge(data, nonce) for data, nonce in all_cases())


def pack_cases(cases):
    """The case file the C++ programs read: count, then per case the 16 nonce
    bytes, the length and the bytes."""
    return struct.pack("<I", len(cases)) + b"".join(n + struct.pack("<I", len(d)) + d for d, n in cases)


def batch(cases, align=None, gap=0):
    """(bytes, nonce) cases laid out as one wire: (wire, spans, nonces).
    ``align``: every span starts at that offset mod 16 (None: back to back,
    plus ``gap`` bytes)."""
    spans = np.zeros(len(cases), dtype=layout.STREAM_SPAN)
    parts, at = [], 0
    for j, (c, _) in enumerate(cases):
        pad = gap if align is None else (align - at) % 16
        parts.append(b"\xa5" * pad)
        at += pad
        spans["off"][j], spans["len"][j] = at, len(c)
        parts.append(c)
        at += len(c)
    wire = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    nonces = np.frombuffer(b"".join(n for _, n in cases), dtype=np.uint8).copy()
    return wire, spans, nonces
