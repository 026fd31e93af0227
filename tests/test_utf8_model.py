"""The UTF-8 rule on the host: layout.utf8_valid_up_to / layout.utf8_plan (the
numpy restatement) and wsg_utf8_valid_up_to (the ABI's host helper, built from
csrc/wsg_utf8.h, the rule the kernel runs) against Python's strict decoder."""
import numpy as np
import pytest

import cppserver_amd as ca
from cppserver_amd import layout
from cppserver_amd.layout import MSG
from tests import utf8_cases as uc


def test_constants_match_the_header():
    text = open(ca.HEADERS[0]).read()
    for name, value in (("WSG_UTF8_TEXT", ca.UTF8_TEXT), ("WSG_UTF8_CLOSE", ca.UTF8_CLOSE),
                        ("WSG_UTF8_EVERY", ca.UTF8_EVERY)):
        assert "#define %s" % name in text
        assert int(text.split("#define %s" % name)[1].split()[0].rstrip("u")) == value


def test_exhaustive_short_strings():
    """Every string of length 0..4 over the 25 boundary bytes."""
    n = 0
    for b in uc.exhaustive(4):
        w = uc.want(b)
        assert ca.utf8_valid_up_to(b) == w, b.hex()
        assert layout.utf8_valid_up_to(b) == w, b.hex()
        n += 1
    assert n == sum(25 ** k for k in range(5))


def test_random_strings():
    for b in uc.random_strings(seed=11, count=20000):
        w = uc.want(b)
        assert ca.utf8_valid_up_to(b) == w, b.hex()
        assert layout.utf8_valid_up_to(b) == w, b.hex()


def test_kat():
    k = uc.kat()
    for name, b in k.items():
        w = uc.want(b)
        assert ca.utf8_valid_up_to(b) == w, name
        assert layout.utf8_valid_up_to(b) == w, name
    # the answers themselves, written out: the decoder is the reference, these pin it
    assert uc.want(k["overlong_3"]) == 0 and uc.want(k["surrogate_hi"]) == 0 and uc.want(k["above_10ffff"]) == 0
    assert uc.want(k["text_trunc_grin_3"]) == 9 and uc.want(k["stray_after_seq"]) == 2
    assert uc.want(k["last_4"]) == 4 and uc.want(k["mixed"]) == len(k["mixed"])


def test_truncations_and_corruptions_of_text():
    rng = np.random.default_rng(12)
    for _ in range(300):
        text = uc.mixed_text(rng, int(rng.integers(1, 80)))
        assert ca.utf8_valid_up_to(text) == len(text) == uc.want(text)
        cut = text[: int(rng.integers(0, len(text) + 1))]
        bad = uc.corrupt(rng, text)
        for b in (cut, bad):
            assert ca.utf8_valid_up_to(b) == uc.want(b) == layout.utf8_valid_up_to(b), b.hex()
        assert uc.want(bad) < len(bad)


def test_host_helper_reads_a_view_of_its_length_only():
    """The same bytes behind a longer buffer: the helper stops at len."""
    buf = uc.EURO + uc.GRIN
    for n in range(len(buf) + 1):
        assert ca.utf8_valid_up_to(buf[:n]) == uc.want(buf[:n])
        assert int(ca.lib().wsg_utf8_valid_up_to(buf, n)) == uc.want(buf[:n])


def _table(items):
    """[(kind, opcode, data, gap)] -> (MSG table, dense bytes); gap: bytes in
    front of the data that belong to no message (a close status)."""
    msgs = np.zeros(len(items), dtype=MSG)
    buf = b""
    for m, (kind, opcode, data, gap) in enumerate(items):
        buf += b"\x03\xe8"[:gap]
        msgs[m]["off"], msgs[m]["len"], msgs[m]["kind"], msgs[m]["opcode"] = len(buf), len(data), kind, opcode
        buf += data
    return msgs, np.frombuffer(buf, dtype=np.uint8)


def test_utf8_plan_selection_and_results():
    items = [
        (ca.CB_RECEIVED, ca.WS_TEXT, b"ok " + uc.EURO, 0),          # 0 text, valid
        (ca.CB_RECEIVED, ca.WS_BINARY, b"\xff\xfe", 0),             # 1 binary
        (ca.CB_RECEIVED, ca.WS_TEXT, b"ab" + uc.GRIN[:3], 0),       # 2 text, cut: invalid at 2
        (ca.CB_CLOSE, ca.WS_CLOSE, b"bye \xc0", 2),                 # 3 close, invalid at 4
        (ca.CB_PING, ca.WS_PING, b"\x80", 0),                       # 4 ping
        (ca.CB_RECEIVED, ca.WS_TEXT, b"", 0),                       # 5 empty text
        (0, 3, b"\xff", 0),                                         # 6 no callback
    ]
    msgs, buf = _table(items)
    lens = [len(i[2]) for i in items]
    u64max = 2 ** 64 - 1

    valid, result = layout.utf8_plan(msgs, buf, ca.UTF8_TEXT | ca.UTF8_CLOSE)
    assert list(valid) == [6, 2, 2, 4, 1, 0, 1] and list(result) == [2, 2, 4, 6 + 5 + 5 + 0]
    valid, result = layout.utf8_plan(msgs, buf, ca.UTF8_TEXT)
    assert list(valid) == [6, 2, 2, 5, 1, 0, 1] and list(result) == [1, 2, 3, 11]
    valid, result = layout.utf8_plan(msgs, buf, ca.UTF8_CLOSE)
    assert list(valid) == [6, 2, 5, 4, 1, 0, 1] and list(result) == [1, 3, 1, 5]
    valid, result = layout.utf8_plan(msgs, buf, ca.UTF8_EVERY)
    assert list(valid) == [6, 0, 2, 4, 0, 0, 0] and list(result) == [5, 1, 7, sum(lens)]
    valid, result = layout.utf8_plan(msgs, buf, 0)
    assert list(valid) == lens and list(result) == [0, u64max, 0, 0]
    # msg_cap: a message that ends past it is not checked (nor read)
    cap = int(msgs[2]["off"]) + 4
    valid, result = layout.utf8_plan(msgs, buf, ca.UTF8_EVERY, msg_cap=cap)
    assert list(valid) == [6, 0, 5, 5, 1, 0, 1] and list(result) == [1, 1, 2, 8]
    # no records
    valid, result = layout.utf8_plan(msgs[:0], buf[:0], ca.UTF8_EVERY)
    assert len(valid) == 0 and list(result) == [0, u64max, 0, 0]


@pytest.mark.parametrize("seed", range(3))
def test_utf8_plan_against_the_decoder(seed):
    rng = np.random.default_rng(40 + seed)
    items = []
    for _ in range(200):
        text = uc.mixed_text(rng, int(rng.integers(0, 40)))
        if text and rng.random() < 0.3:
            text = uc.corrupt(rng, text)
        kind, opcode = [(1, 1), (1, 2), (2, 8), (3, 9)][int(rng.integers(0, 4))]
        items.append((kind, opcode, text, 2 if kind == 2 else 0))
    msgs, buf = _table(items)
    valid, result = layout.utf8_plan(msgs, buf, ca.UTF8_TEXT | ca.UTF8_CLOSE)
    sel = [i for i, it in enumerate(items) if it[:2] in ((1, 1), (2, 8))]
    expect = [uc.want(it[2]) if i in sel else len(it[2]) for i, it in enumerate(items)]
    assert list(valid) == expect
    bad = [i for i in sel if expect[i] < len(items[i][2])]
    assert list(result) == [len(bad), bad[0], len(sel), sum(len(items[i][2]) for i in sel)]
