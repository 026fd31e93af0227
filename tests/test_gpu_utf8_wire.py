"""wsg_check_utf8_wire on the GPU: the UTF-8 check read from the masked wire.

Every call goes through run(): every output starts as a sentinel, and what
the call writes is held against three things: layout.utf8_wire_plan (the
model), Python's strict decoder over what the oracle's sessions deliver
(tests/utf8_wire_cases.py::check_case), and the existing device chain
wsg_decode_messages + wsg_check_utf8 on the same batch.  d_state must come
back bit for bit.  All comparisons are exact."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_STATE  # noqa: E402
from tests import big_cases as bc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import utf8_cases as uc  # noqa: E402
from tests import utf8_wire_cases as wc  # noqa: E402
from tests.test_gpu_reply import SENT64, SENTINEL, dev, sent  # noqa: E402

EXTRA = 3
U64_MAX = 2**64 - 1
CASES = wc.small_cases()


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def _on(stream):
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())


def d_wire_of(wire, behind=None):
    """The wire on the device; `behind`: the byte that fills the rest of its last 16-byte block."""
    n = len(wire)
    buf = torch.full(((n + 15) // 16 * 16 + 16,), 0xFF if behind is None else behind, dtype=torch.uint8, device="cuda")
    buf[:n] = torch.from_numpy(np.ascontiguousarray(wire))
    return buf[:n]


class Out:
    """Sentinel-filled outputs of one call over n frames in ns streams."""

    def __init__(self, n, ns, opcodes=None):
        self.n, self.ns = n, ns
        st = np.full((max(ns, 1) + EXTRA) * STREAM_STATE.itemsize, SENTINEL, dtype=np.uint8).view(STREAM_STATE)
        st["opcode"][:ns] = 0 if opcodes is None else opcodes
        self.state_in = st.view(np.uint8).copy()
        self.state = dev(self.state_in)
        self.msgs = sent((max(n, 1) + EXTRA) * MSG.itemsize)
        self.info = sent((max(n, 1) + EXTRA) * RECV_INFO.itemsize)
        self.count = sent((2 + EXTRA) * 8).view(torch.int64)
        self.valid = sent((max(n, 1) + EXTRA) * 8).view(torch.int64)
        self.result = sent((4 + EXTRA) * 8).view(torch.int64)

    def launch(self, codec, wire, fs, sf, which, stream=None):
        codec.check_utf8_wire(wire, fs, sf, state=self.state, which=which, msgs=self.msgs, count=self.count,
                              info=self.info, valid=self.valid, result=self.result, stream=stream)

    def refill(self):
        for t in (self.msgs, self.info, self.count, self.valid, self.result):
            t.view(torch.uint8).fill_(SENTINEL)

    def check(self, info, msgs, count, valid, result):
        """Everything the call writes against the expected tables; the rest still the sentinel."""
        n, nm = self.n, len(msgs)
        got_count = self.count.cpu().numpy().view(np.uint64)
        assert [int(x) for x in got_count[:2]] == [int(x) for x in count] and (got_count[2:] == SENT64).all()
        v = self.valid.cpu().numpy().view(np.uint64)
        got = [int(x) for x in v[:nm]]
        want = [int(x) for x in valid]
        assert got == want, [(m, g, w) for m, (g, w) in enumerate(zip(got, want)) if g != w][:10]
        assert (v[nm:] == SENT64).all()
        r = self.result.cpu().numpy().view(np.uint64)
        assert [int(x) for x in r[:4]] == [int(x) for x in result] and (r[4:] == SENT64).all()
        m = self.msgs.cpu().numpy()
        mc.same_fields(m[: nm * MSG.itemsize].view(MSG), msgs, mc.MSG_FIELDS)
        assert (m[nm * MSG.itemsize:] == SENTINEL).all() or n == 0
        i = self.info.cpu().numpy()
        mc.same_fields(i[: n * RECV_INFO.itemsize].view(RECV_INFO), info, mc.INFO_FIELDS)
        assert (i[max(n, 1) * RECV_INFO.itemsize:] == SENTINEL).all()
        assert np.array_equal(self.state.cpu().numpy(), self.state_in), "d_state was written"


def chain(codec, d_wire, fs, sf, out, which, stream=None):
    """wsg_decode_messages + wsg_check_utf8 on the same batch (on a copy of
    the state); returns (valid, result, msgs, count, info) on the host."""
    n = out.n
    with _on(stream):
        msg, msgs, count, _, info = codec.decode_messages(d_wire, fs, sf, state=out.state.clone())
        valid, result = codec.check_utf8(msg, msgs, count, which, msg_room=n)
    return valid, result, msgs, count, info


def run(codec, case, which=wc.DEFAULT, stream=None, wire=None, behind=None, with_chain=True, decoder=True):
    """One call on sentinel outputs and every comparison; returns (valid, result)."""
    b = case.batch
    n, ns = b.n, b.n_streams
    if decoder and wire is None:
        want = wc.check_case(case, which)
    else:
        want = wc.model(case, which, wire)
    code, info, msgs, count, valid, result = want
    out = Out(n, ns, None if case.state is None else case.state["opcode"])
    the_wire = b.wire if wire is None else wire
    d_wire = d_wire_of(the_wire, behind)
    fs, sf = dev(b.fs.view(np.int64)), dev(b.stream_first)
    if stream is not None:
        torch.cuda.synchronize()   # the buffers are ready before the side stream starts
    with _on(stream):
        out.launch(codec, d_wire, fs, sf, which)
    assert codec.sync_status(stream) == code
    assert codec.sync_status(stream) == 0   # reported once
    out.check(info, msgs, count, valid, result)
    if with_chain and code == 0:
        cv, cr, cm, ccount, ci = chain(codec, d_wire, fs, sf, out, which, stream)
        assert codec.sync_status(stream) == 0
        nm = len(msgs)
        assert torch.equal(cv[:nm], out.valid[:nm]) and torch.equal(cr, out.result[:4])
        assert torch.equal(cm[: nm * MSG.itemsize], out.msgs[: nm * MSG.itemsize])
        assert torch.equal(ccount, out.count[:2])
        assert torch.equal(ci[: n * RECV_INFO.itemsize], out.info[: n * RECV_INFO.itemsize])
    return [int(x) for x in valid], [int(x) for x in result]


# ------------------------------------------------- cuts, keys, edges, boundaries
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(codec, name):
    """tests/utf8_wire_cases.py: every KAT string at every payload alignment;
    payload lengths 0..20 at every alignment, masked and not; every sequence
    cut over two, three and four fragments with their own keys, with empty
    fragments and with a ping between; sequences on chunk, row and piece
    edges; message boundaries; close reasons; selection; tails."""
    results = [run(codec, CASES[name], which) for which in wc.WHICH]
    if name not in ("tails", "random_fragments"):
        assert any(r[1][0] > 0 for r in results) or name.endswith("_0")   # something in it is invalid


def test_selection_every_which(codec):
    for which in wc.ALL_WHICH:
        valid, result = run(codec, CASES["selection"], which)
        if which == 0:
            assert result == [0, U64_MAX, 0, 0]
    assert run(codec, CASES["selection"], layout.UTF8_EVERY)[0][0] == 0
    assert run(codec, CASES["selection"], wc.DEFAULT)[0][0] == 40   # unselected: its len


def test_carry_over_in_two_calls(codec):
    first, second = wc.carry_over()
    c1 = wc.Case(first)
    run(codec, c1)
    state = layout.message_plan(wc.model(c1, 0)[1], c1.batch.stream_first)[2]   # what a decode hands on
    assert int(state["consumed"][0]) == 1
    valid, result = run(codec, wc.Case(second, state["opcode"]))
    assert valid == [10, 0] and result == [1, 1, 2, 11]


# ------------------------------------------------------- wire end and errors
@pytest.mark.parametrize("behind", [0xFF, 0xAC, 0x80])
def test_bytes_behind_the_wire_end(codec, behind):
    """wire_len is no multiple of 16 and the rest of the last block holds
    bytes that would complete (AC, 80) or spoil (FF) the last message if they
    were taken for its own."""
    for pad in range(1, 16):
        frames = [wc.frame(wc.FIN | wc.BINARY, b"p" * pad), wc.frame(wc.FIN | wc.TEXT, b"end \xe2\x82")]
        case = wc.Case([frames])
        if len(case.batch.wire) % 16 == 0:
            continue
        valid, _ = run(codec, case, behind=behind)
        assert valid == [pad, 4]
    case = wc.Case([[wc.frame(wc.FIN | wc.TEXT, b"fine " + uc.EURO)]])
    assert run(codec, case, behind=behind)[0] == [8]


def test_frames_with_an_error(codec):
    """A wire cut short inside its last text frame, and a fragment whose
    length byte claims more than its frame holds: the frame error is latched,
    the frame is empty (as in the plan), the result is the model's."""
    key = 0x0BADF00D
    frames = [wc.frame(wc.FIN | wc.TEXT, b"one " + uc.EURO[:2], key=key), wc.frame(wc.TEXT, b"two \xe2", key=key + 1),
              wc.frame(wc.CONT, b"\x82", key=key + 2), wc.frame(wc.FIN | wc.CONT, b"\xac three " + uc.GRIN, key=key + 3)]
    c = wc.Case([frames])
    for cut in (1, 5, 12):
        wire = c.batch.wire[: len(c.batch.wire) - cut]
        assert wc.model(c, wc.DEFAULT, wire)[0] == ca.WSG_ETRUNC
        valid, result = run(codec, c, wire=wire, with_chain=False)
        assert valid == [4] and result == [1, 0, 1, 6]     # the open message lies in the tail
    wire = c.batch.wire.copy()
    at = int(c.batch.fs[2]) + 1
    wire[at] += 3                                           # the middle fragment runs into the next frame
    assert wc.model(c, wc.DEFAULT, wire)[0] == ca.WSG_EINVAL
    valid, result = run(codec, c, wire=wire, with_chain=False)
    assert valid == [4, 4] and result[0] == 2              # "two E2" + "AC three ...": the 82 is gone


# ----------------------------------------------------------------------- scale
def test_many_messages(codec):
    """More than 64 * 64 one-frame text messages: three rounds of the 64-probe
    search, the per-record kernels past one block; a handful invalid, the
    first and the last among them."""
    case, bad = wc.many_messages()
    valid, result = run(codec, case)
    assert result[0] == len(bad) and result[1] == 0 and result[2] == case.batch.n


def test_large_message_later_passes():
    """One message of several MiB on a grid of one block per CU
    ($WSG_UTF8_WIRE_BLOCKS_PER_CU=1), so that every wave takes several pieces; one
    bad byte at a time."""
    os.environ["WSG_UTF8_WIRE_BLOCKS_PER_CU"] = "1"
    try:
        c = ca.Codec(0)
    finally:
        del os.environ["WSG_UTF8_WIRE_BLOCKS_PER_CU"]
    try:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        per_pass = cus * 4 * 4096                  # one block per CU, four waves, a 4 KiB piece each
        n = 2 * per_pass + 3 * 4096 + 5
        rng = np.random.default_rng(7)
        spots = [0, 4095 - 14, 4096 - 14, per_pass - 14, per_pass - 13, 2 * per_pass, n - 1]
        edges = sorted(set(spots + [s + 1 for s in spots] + [n]))
        text = bytearray()
        for lo, hi in zip([0] + edges, edges):     # a code point begins at every spot and behind it
            text += uc.mixed_text(rng, hi - lo)
        assert len(text) == n and uc.want(text) == n
        key = 0xC3A5F00D
        out = Out(1, 1)
        fs, sf = dev(np.zeros(1, dtype=np.int64)), dev(np.array([0, 1], dtype=np.int32))
        for s in [None] + spots:
            data = bytearray(text)
            if s is not None:
                data[s] = 0xFF
            d_wire = d_wire_of(np.frombuffer(wc.frame(wc.FIN | wc.TEXT, bytes(data), key=key), dtype=np.uint8))
            out.refill()
            out.launch(c, d_wire, fs, sf, ca.UTF8_TEXT)
            assert c.sync_status() == 0
            v = out.valid.cpu().numpy().view(np.uint64)
            r = [int(x) for x in out.result.cpu().numpy().view(np.uint64)[:4]]
            assert int(v[0]) == (n if s is None else s) and (v[1:] == SENT64).all(), s
            assert r == ([0, U64_MAX, 1, n] if s is None else [1, 0, 1, n]), s
    finally:
        c.close()


# --------------------------------------------------------- runtime and arguments
def test_side_stream_no_synchronisation(codec):
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert run(codec, CASES["split_sequences"], stream=st)[1][0] > 0


def test_graph_replay_follows_new_bytes():
    """The call captured after one plain run and replayed on a wire whose
    bytes were changed in place (the same frame table)."""
    c = ca.Codec(0)   # a context of its own: the graph names its scratch
    try:
        rng = np.random.default_rng(102)
        sizes = [int(rng.integers(1, 200)) for _ in range(64)] + [5000]
        texts = [uc.mixed_text(rng, s) for s in sizes]

        def case_of(texts, seed):
            key = wc._keys(seed)
            frames = [wc.frame(wc.FIN | (wc.TEXT if i % 4 else wc.BINARY), t, key=key()) for i, t in enumerate(texts)]
            return wc.Case([frames[:30], frames[30:]])

        first = case_of(texts, 0)
        b = first.batch
        d_wire = d_wire_of(b.wire)
        fs, sf = dev(b.fs.view(np.int64)), dev(b.stream_first)
        out = Out(b.n, 2)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            out.launch(c, d_wire, fs, sf, wc.DEFAULT)
        assert c.sync_status(st) == 0
        out.check(*wc.check_case(first, wc.DEFAULT)[1:])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            out.launch(c, d_wire, fs, sf, wc.DEFAULT)
        for replay in range(3):
            changed = [uc.corrupt(rng, t) if rng.random() < 0.4 else uc.mixed_text(rng, len(t)) for t in texts]
            case = case_of(changed, replay + 1)
            assert np.array_equal(case.batch.fs, b.fs)
            d_wire.copy_(torch.from_numpy(case.batch.wire))
            out.refill()
            torch.cuda.synchronize()
            g.replay()
            assert c.sync_status(st) == 0
            want = wc.check_case(case, wc.DEFAULT)
            assert int(want[5][0]) > 0
            out.check(*want[1:])
    finally:
        c.close()


def test_null_and_misaligned_operands(codec):
    case = CASES["message_boundaries"]
    b = case.batch
    out = Out(b.n, b.n_streams)
    d_wire, fs, sf = d_wire_of(b.wire), dev(b.fs.view(np.int64)), dev(b.stream_first)
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    good = [d_wire.data_ptr(), len(b.wire), fs.data_ptr(), b.n, sf.data_ptr(), b.n_streams, out.state.data_ptr(),
            wc.DEFAULT, out.msgs.data_ptr(), out.count.data_ptr(), out.info.data_ptr(), out.valid.data_ptr(),
            out.result.data_ptr()]
    ptrs = (0, 2, 4, 6, 8, 9, 10, 11, 12)

    def call(ctx=codec._ctx, **change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        a = [vp(x) if i in ptrs else x for i, x in enumerate(a)]
        return codec._L.wsg_check_utf8_wire(ctx, *a, None)

    assert call(ctx=None) == ca.WSG_EINVAL
    for i in ptrs:
        assert call(**{"a%d" % i: None}) == ca.WSG_EINVAL, i
    for i, step in ((0, 8), (0, 1), (2, 4), (4, 2), (6, 4), (8, 4), (9, 4), (10, 4), (11, 2), (12, 1)):
        assert call(**{"a%d" % i: good[i] + step}) == ca.WSG_EINVAL, (i, step)
    assert call(a3=0xFFFFFFFF) == ca.WSG_EINVAL and call(a5=0) == ca.WSG_EINVAL
    torch.cuda.synchronize()
    for t in (out.msgs, out.count, out.info, out.valid, out.result):
        assert (t.view(torch.uint8) == SENTINEL).all()
    # NULL buffers are fine where nothing can be read or written through them; empty shapes are valid
    assert call(a0=None, a1=0, a2=None, a3=0, a8=None, a10=None, a11=None) == 0
    assert codec.sync_status() == 0
    assert [int(x) for x in out.result.cpu().numpy().view(np.uint64)[:4]] == [0, U64_MAX, 0, 0]
    assert [int(x) for x in out.count.cpu().numpy()[:2]] == [0, 0]
    assert call(a3=0, a5=0, a6=None) == 0 and call(a7=0) == 0 and call() == 0
    assert codec.sync_status() == 0
    out.check(*wc.model(case, wc.DEFAULT)[1:])
    empty = wc.Case([[], [wc.frame(wc.FIN | wc.TEXT, b"\xff")], []])
    assert run(codec, empty)[0] == [0]


def test_checked_launch_refuses_short_valid_block():
    """$WSG_CHECK=1 (read at wsg_create): a d_valid block one word short of n
    words is WSG_EINVAL and nothing is launched; a block of n words runs.  The
    blocks are exact device allocations."""
    os.environ["WSG_CHECK"] = "1"
    try:
        c = ca.Codec(0)
    finally:
        del os.environ["WSG_CHECK"]
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    vp = ctypes.c_void_p
    blocks = []

    def hip_block(nbytes):
        p = vp()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        assert hip.hipMemset(p, SENTINEL, ctypes.c_size_t(nbytes)) == 0
        blocks.append(p)
        return p.value

    def read_block(ptr, nbytes):
        host = np.empty(nbytes, dtype=np.uint8)
        assert hip.hipMemcpy(vp(host.ctypes.data), vp(ptr), ctypes.c_size_t(nbytes), 2) == 0   # device to host
        return host

    try:
        n = (2 << 20) // 8 + 1                   # n words end 8 bytes past 2 MiB, n - 1 end at it
        frames = [wc.frame(wc.FIN | wc.TEXT, b"\xc3" if i == 1 else b"", key=None) for i in range(n)]
        wire = np.frombuffer(b"".join(frames), dtype=np.uint8)
        starts = np.cumsum([0] + [len(f) for f in frames[:-1]]).astype(np.int64)
        out = Out(n, 1)
        d_wire, fs, sf = d_wire_of(wire), dev(starts), dev(np.array([0, n], dtype=np.int32))
        torch.cuda.synchronize()

        def call(valid_ptr):
            rc = c._L.wsg_check_utf8_wire(c._ctx, vp(d_wire.data_ptr()), len(wire), vp(fs.data_ptr()), n,
                                          vp(sf.data_ptr()), 1, vp(out.state.data_ptr()), ca.UTF8_TEXT,
                                          vp(out.msgs.data_ptr()), vp(out.count.data_ptr()), vp(out.info.data_ptr()),
                                          vp(valid_ptr), vp(out.result.data_ptr()), None)
            torch.cuda.synchronize()
            return rc

        short = hip_block((n - 1) * 8)
        assert call(short) == ca.WSG_EINVAL
        assert (read_block(short, (n - 1) * 8) == SENTINEL).all()
        assert (out.result.view(torch.uint8) == SENTINEL).all() and (out.count.view(torch.uint8) == SENTINEL).all()
        full = hip_block(n * 8)
        assert call(full) == 0
        got = read_block(full, n * 8).view(np.uint64)
        assert int(got[1]) == 0 and int(got.sum()) == 0
        assert [int(x) for x in out.result.cpu().numpy().view(np.uint64)[:4]] == [1, 1, n, 1]
        assert c.sync_status() == 0
    finally:
        c.close()
        for p in blocks:
            hip.hipFree(p)


# ------------------------------------------------------------------ above 4 GiB
def test_above_4gib(codec):
    """A masked binary filler frame of almost 4 GiB (unselected), then text
    messages whose wire offsets and dense offsets lie past 2^32: the dense
    offset 2^32 falls inside a sequence that is also split over two fragments
    there.  A piece position or an atomicMin operand cut to one word lands in
    the wrong message or on the wrong side of a message's start."""
    key = wc._keys(40)
    rest = wc.Case([[wc.frame(wc.FIN | wc.TEXT, b"ab" + uc.GRIN[:1], key=key()),     # bad at 2
                     wc.frame(wc.TEXT, b"split " + uc.GRIN[:2], key=key()),
                     wc.frame(wc.FIN | wc.CONT, uc.GRIN[2:] + b" whole", key=key()),
                     wc.frame(wc.FIN | wc.TEXT, b"bad \xed\xa0\x80", key=key())],
                    [wc.frame(wc.TEXT, uc.mixed_text(np.random.default_rng(41), 5000), key=key()),
                     wc.frame(wc.FIN | wc.CONT, b"\xbf", key=key())]])
    _, info, msgs, count, valid, result = wc.check_case(rest, wc.DEFAULT)
    target = 3 + 6 + 1                              # 2^32: between the first two bytes of the split sequence
    L0 = bc.MARK32 - target
    at = 14 + L0
    total = at + len(rest.batch.wire)
    wire = torch.zeros((total + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
    hdr = ca.header_pack(0x82, True, L0, 0, bc.FILLER_KEY)
    assert len(hdr) == 14
    wire[:14] = torch.from_numpy(np.frombuffer(hdr, dtype=np.uint8).copy())
    wire[at:total] = torch.from_numpy(rest.batch.wire)
    n, ns = rest.batch.n + 1, rest.batch.n_streams + 1
    fs = dev(np.concatenate([[0], rest.batch.fs + np.uint64(at)]).astype(np.uint64).view(np.int64))
    sf = dev(np.concatenate([[0], rest.batch.stream_first + 1]).astype(np.int32))
    want_msgs, want_count = bc.prepend_filler(msgs, count, L0)
    assert int(want_msgs["off"][2]) < bc.MARK32 < int(want_msgs["off"][2]) + int(want_msgs["len"][2])
    moved = bc.batch_spans(rest.batch)
    moved["off"] += np.uint64(at)
    want_info = bc.shift_info(info, rest.batch.stream_first, bc.batch_spans(rest.batch), moved)
    out = Out(n, ns)
    out.launch(codec, wire[:total], fs, sf, wc.DEFAULT)
    assert codec.sync_status() == 0
    got_info = out.info.cpu().numpy()[: n * RECV_INFO.itemsize].view(RECV_INFO)
    assert (int(got_info["payload_off"][0]), int(got_info["len"][0])) == (14, L0)
    mc.same_fields(got_info[1:], want_info, mc.INFO_FIELDS)
    want_valid = [L0] + [int(x) for x in valid]
    assert want_valid[1:] == [2, 16, 4, 5000]
    v = out.valid.cpu().numpy().view(np.uint64)
    assert [int(x) for x in v[: len(want_valid)]] == want_valid and (v[len(want_valid):] == SENT64).all()
    assert [int(x) for x in out.result.cpu().numpy().view(np.uint64)[:4]] == \
        [int(result[0]), int(result[1]) + 1, int(result[2]), int(result[3])]
    m = out.msgs.cpu().numpy()[: len(want_msgs) * MSG.itemsize].view(MSG)
    mc.same_fields(m, want_msgs, mc.MSG_FIELDS)
    assert [int(x) for x in out.count.cpu().numpy().view(np.uint64)[:2]] == [int(x) for x in want_count]
    assert np.array_equal(out.state.cpu().numpy(), out.state_in)


# ------------------------------------------------------------------------ fuzz
@pytest.mark.parametrize("group", range(4))
def test_fuzz(codec, group):
    """100 seeds of checked_reply_cases.fuzz_batch with text payloads."""
    invalid = 0
    for seed in range(25 * group, 25 * group + 25):
        case, _, _, _ = wc.fuzz(seed)
        invalid += run(codec, case, wc.WHICH[seed & 1], decoder=seed % 5 == 0)[1][0]
    assert invalid > 0
