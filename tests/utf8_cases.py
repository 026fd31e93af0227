"""Shared by tests/test_utf8_model.py, tests/test_utf8_host.py (CPU) and
tests/test_gpu_utf8.py: byte strings for the UTF-8 rule (csrc/wsg_utf8.h) and
text generators, all from seeds or written out by hand.  The expected value of
a string is Python's strict decoder's alone (want).  No test lives here."""
import itertools

import numpy as np

# The 25 boundary byte values of the rule: the ends of every class of byte.
BOUNDARY = bytes([0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED,
                  0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF])

EURO = b"\xe2\x82\xac"          # U+20AC
GRIN = b"\xf0\x9f\x98\x80"      # U+1F600


def want(data):
    """valid_up_to by Python's decoder: len, or UnicodeDecodeError.start."""
    data = bytes(data)
    try:
        data.decode("utf-8")
        return len(data)
    except UnicodeDecodeError as e:
        return e.start


def exhaustive(max_len=4):
    """Every string of length 0..max_len over BOUNDARY (406 901 at 4)."""
    for n in range(max_len + 1):
        for t in itertools.product(BOUNDARY, repeat=n):
            yield bytes(t)


def random_strings(seed, count, lo=5, hi=12):
    rng = np.random.default_rng(seed)
    table = np.frombuffer(BOUNDARY, dtype=np.uint8)
    return [table[rng.integers(0, len(table), int(rng.integers(lo, hi + 1)))].tobytes() for _ in range(count)]


def kat():
    """name -> bytes: the known answers (RFC 3629, Autobahn 6.x)."""
    k = {
        "empty": b"",
        "ascii": b"Hello, WebSocket!",
        "first_1": b"\x00", "last_1": b"\x7f",
        "first_2": b"\xc2\x80", "last_2": b"\xdf\xbf",
        "first_3": b"\xe0\xa0\x80", "last_3": b"\xef\xbf\xbf",
        "first_4": b"\xf0\x90\x80\x80", "last_4": b"\xf4\x8f\xbf\xbf",
        "before_surrogates": b"\xed\x9f\xbf", "after_surrogates": b"\xee\x80\x80",
        "overlong_2a": b"\xc0\x80", "overlong_2b": b"\xc1\xbf",
        "overlong_3": b"\xe0\x9f\xbf", "overlong_4": b"\xf0\x8f\xbf\xbf",
        "surrogate_lo": b"\xed\xa0\x80", "surrogate_hi": b"\xed\xbf\xbf",
        "above_10ffff": b"\xf4\x90\x80\x80", "f5": b"\xf5\x80\x80\x80", "ff": b"\xff", "stray_80": b"\x80",
        "stray_after_text": b"abc\x80def", "stray_after_seq": b"\xc2\x80\x80",
        "lead2_ascii": b"\xc2A", "lead3_ascii": b"\xe2A\xac", "lead3_ascii_3rd": b"\xe2\x82A",
        "lead4_ascii": b"\xf0A\x98\x80", "lead4_ascii_4th": b"\xf0\x9f\x98A",
        "mixed": "κόσμε € 😀 end".encode("utf-8"),
    }
    for name, seq in (("c2", b"\xc2\x80"), ("euro", EURO), ("grin", GRIN)):
        for cut in range(1, len(seq)):     # every truncation at the string's end, bare and behind text
            k["trunc_%s_%d" % (name, cut)] = seq[:cut]
            k["text_trunc_%s_%d" % (name, cut)] = b"text " + seq + seq[:cut]
    return k


def mixed_text(rng, nbytes):
    """Valid text of exactly nbytes bytes, whole code points, sequences of
    1..4 bytes in about equal byte shares (ASCII fills the last bytes)."""
    count = nbytes                                      # code points drawn: at least one byte each
    size = rng.choice(4, size=count, p=np.array([12, 6, 4, 3]) / 25.0) + 1   # P(k bytes) ~ 1 / k: equal byte shares
    lo = np.array([0x20, 0x80, 0x800, 0x10000])[size - 1]
    hi = np.array([0x7F, 0x800, 0x10000, 0x110000])[size - 1]
    cps = lo + (rng.random(count) * (hi - lo)).astype(np.int64)
    cps[(cps >= 0xD800) & (cps < 0xE000)] = 0xE000      # no surrogate
    whole = int(np.searchsorted(np.cumsum(size), nbytes, side="right"))      # the code points that fit
    out = "".join(map(chr, cps[:whole].tolist())).encode("utf-8")
    out += bytes(rng.integers(0x20, 0x7F, nbytes - len(out), dtype=np.uint8))
    assert len(out) == nbytes
    return out


def corrupt(rng, text):
    """text with one byte replaced so that it is not valid UTF-8 any more."""
    assert len(text) > 0
    b = bytearray(text)
    while True:
        i = int(rng.integers(0, len(b)))
        old = b[i]
        b[i] = int(rng.choice([0x80, 0xBF, 0xC0, 0xF5, 0xFF, 0xE0, 0xF4]))
        if want(b) < len(b):
            return bytes(b)
        b[i] = old
