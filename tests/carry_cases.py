"""Shared by tests/test_carry_model.py (CPU), tests/test_gpu_carry.py and
tests/test_gpu_carry_loop.py: batches for wsg_carry_streams (a wire with spans
as a round's calls leave them, the bytes just read, drops), and the echo
server's loop of tests/server_loop_cases.py with the carry in it.

In that loop stream j is connection j in every round: a connection that was
dropped, or that has delivered everything, stays in the table as a stream
without new bytes.  The driver never joins a wire: a round hands ``carry`` the
last round's wire, spans and close offsets and the bytes just read, and
``step`` what ``carry`` returned.  No test lives here."""
import numpy as np

from cppserver_amd import layout
from cppserver_amd.layout import STREAM_READ, STREAM_SPAN
from tests import server_loop_cases as sl

U64_MAX = 2 ** 64 - 1
SIZES = (0, 1, 15, 16, 17, 31, 32, 33)   # around one and two 16-byte chunks


class Case:
    """One call's inputs on the host.  ``wire_raw`` / ``new_raw``: the bytes of
    the device buffers, which run on behind wire / new to the end of the last
    16-byte block and one block more, all of it random."""

    def __init__(self, wire_raw, wire_len, spans, new_raw, new_len, reads, close_off):
        self.wire_raw, self.new_raw = wire_raw, new_raw
        self.wire, self.new = wire_raw[:wire_len], new_raw[:new_len]
        self.spans, self.reads, self.close_off = spans, reads, close_off
        self.ns = len(spans)

    def plan(self, next_cap=None):
        return layout.carry_plan(self.wire, self.spans, self.new, self.reads, self.close_off, next_cap)


def _place(at, mod):
    """The first position >= at that is `mod` modulo 16 (None: at)."""
    return at if mod is None else at + (mod - at) % 16


def make(rng, tails, news, tail_mod=None, new_mod=None, drop=None, consumed=None, reads=True, close=True):
    """A batch whose stream j has a tail of tails[j] bytes at a source offset of
    tail_mod[j] modulo 16 and a read of news[j] bytes at new_mod[j] modulo 16
    (None: wherever a random gap leaves them), behind consumed[j] bytes that
    the round before used up.  Random bytes lie everywhere: in the consumed
    prefixes, in the gaps between spans and between reads, and behind the end
    of both sources.  drop: the streams whose close offset is set; reads /
    close False: no d_read / no d_close_off at all."""
    ns = len(tails)
    spans = np.zeros(ns, dtype=STREAM_SPAN)
    rd = np.zeros(ns, dtype=STREAM_READ)
    at = nat = 0
    for j in range(ns):
        used = int(rng.integers(0, 40)) if consumed is None else int(consumed[j])
        start = _place(at + int(rng.integers(0, 20)) + used, None if tail_mod is None else int(tail_mod[j]))
        spans[j] = (start - used, used + int(tails[j]), used, int(rng.integers(0, 2 ** 32)))
        at = start + int(tails[j])
        rstart = _place(nat + int(rng.integers(0, 20)), None if new_mod is None else int(new_mod[j]))
        rd[j] = (rstart, int(news[j]))
        nat = rstart + int(news[j])
    wire_len, new_len = at + int(rng.integers(0, 20)), nat + int(rng.integers(0, 20))
    raw = [rng.integers(0, 256, (n + 15) // 16 * 16 + 16, dtype=np.uint8) for n in (wire_len, new_len)]
    close_off = None
    if close:
        close_off = np.full(ns, U64_MAX, dtype=np.uint64)
        if drop is not None:
            close_off[np.asarray(drop, dtype=bool)] = rng.integers(0, 2 ** 40, int(np.sum(drop)), dtype=np.uint64)
    return Case(raw[0], wire_len, spans, raw[1], new_len, rd if reads else None, close_off)


def alignments(rng):
    """Every tail length of SIZES with every read length of SIZES, at every
    tail source offset modulo 16 and four read source offsets: 4096 streams."""
    t, n, tm, nm = np.meshgrid(SIZES, SIZES, np.arange(16), (0, 1, 7, 15), indexing="ij")
    order = rng.permutation(t.size)
    return make(rng, t.ravel()[order], n.ravel()[order], tm.ravel()[order], nm.ravel()[order])


def piece_edges(rng):
    """Tails and reads around one 4 KiB piece and over three, and one stream of
    3 MiB + 7 bytes with a read of 1 MiB + 3."""
    edge = (4095, 4096, 4097, 3 * 4096 + 5)
    tails = [a for a in edge for _ in edge] + [0, 5, (3 << 20) + 7, 9]
    news = [b for _ in edge for b in edge] + [4096, 0, (1 << 20) + 3, 4097]
    return make(rng, tails, news)


def fuzz(seed):
    """1-3000 streams with lengths of 0, a few bytes, hundreds or (rarely) tens
    of KiB, random drops, random source alignments."""
    rng = np.random.default_rng([4117, seed])
    ns = int(rng.integers(1, 3001))

    def lengths():
        kind = rng.choice(4, ns, p=[0.25, 0.35, 0.4 - 20.0 / (ns + 2000), 20.0 / (ns + 2000)])
        return np.choose(kind, [np.zeros(ns, dtype=np.int64), rng.integers(1, 20, ns), rng.integers(100, 1000, ns),
                                rng.integers(10 << 10, 50 << 10, ns)])

    return make(rng, lengths(), lengths(), drop=rng.random(ns) < 0.1, reads=seed % 7 != 3, close=seed % 5 != 2)


# ------------------------------------------------------------------ the loop with the carry in it
def model_carry(wire, spans, close_off, new, reads):
    """The carry of a round on the host: layout.carry_plan."""
    nxt, out, count, key = layout.carry_plan(wire, spans, new, reads, close_off)
    assert key is None
    return nxt, out


def drive(step, carry, seed, keys=None, cases=sl, carries="opcode"):
    """server_loop_cases.drive with every connection a stream of its own for
    good.  ``carry(wire, spans, close_off, new, reads)`` gets the last round's
    wire, its spans with ``consumed`` as the round's call left it and its
    close offsets (in the first round no wire, a zeroed table and None) and the bytes just
    read (numpy uint8, STREAM_READ), and returns (wire, spans) for
    ``step(wire, spans, state, proto, keys, frame_cap)``, model_step's
    signature.  What ``step`` returns may carry ``spans_left`` and
    ``close_left``, the span table and close offsets to hand to the next carry
    as they are; without them they are made from bytes_consumed and close_off.
    ``cases``: server_loop_cases, or rfc_assembly_cases with ``carries``
    "ahead".  ``step.final()``, when there is one, returns the (state, proto)
    lists the run ends with (a step that keeps them to itself).

    Fills a Run that cases.check_run accepts, and: rounds, read_bytes (the
    bytes handed to carry) and, while the tables are numpy arrays, wire_bytes
    (the sum of the rounds' wire sizes, what a loop that uploads each round's
    wire sends), both (in the round with the most bytes, the streams with a
    tail and a read that are not empty) and a frame_cap for the step (None
    for tables on the device)."""
    conns, reads = cases.connections(), cases.schedule(seed)
    n = len(conns)
    run = sl.Run()
    run.out, run.verdict = [bytearray() for _ in range(n)], [sl.NONE] * n
    run.proto, run.left, run.rounds = [(0, 0)] * n, [b""] * n, 0
    state = [0] * n
    run.read_bytes = run.wire_bytes = run.both = 0
    fullest = -1
    pos, frames_done, rounds_of, gone = [0] * n, [0] * n, [0] * n, [False] * n
    frames_left = [len(c.frames) for c in conns]
    wire, spans, close_off = np.zeros(0, dtype=np.uint8), np.zeros(n, dtype=STREAM_SPAN), None   # the first round

    def read_round():
        chunks, rd, at = [], np.zeros(n, dtype=STREAM_READ), 0
        for j in range(n):
            new = b""
            if not gone[j] and pos[j] < len(conns[j].data):
                size = reads[j][rounds_of[j]]
                rounds_of[j] += 1
                new = conns[j].data[pos[j]:] if size == sl.REST else conns[j].data[pos[j]: pos[j] + size]
                pos[j] += len(new)
            chunks.append(new)   # back to back: what is handed over is what was read
            rd[j] = (at, len(new))
            at += len(new)
        return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy(), rd

    while any(not gone[j] and pos[j] < len(conns[j].data) for j in range(n)):
        assert run.rounds < sl.MAX_ROUNDS, "the loop does not end"
        new, rd = read_round()
        tails = _tails(spans, close_off) if isinstance(spans, np.ndarray) else None
        wire, spans = carry(wire, spans, close_off, new, rd)
        run.read_bytes += int(rd["len"].sum())
        frame_cap = None
        if tails is not None:   # (tables on the device stay there: the step sizes its own outputs)
            total = int(rd["len"].sum()) + int(tails.sum())
            run.wire_bytes += len(wire)
            if total > fullest:
                fullest, run.both = total, int(((tails > 0) & (rd["len"] > 0)).sum())
            frame_cap = min(total // 2, sum(frames_left[j] for j in range(n) if not gone[j])) + 1
        r = step(wire, spans, np.array(state), list(run.proto), keys, frame_cap)
        run.rounds += 1
        for j in range(n):
            run.out[j] += bytes(r.reply[int(r.stream_reply[j]): int(r.stream_reply[j + 1])])
            v = r.verdict[j]
            assert (v != sl.NONE) == (int(r.close_off[j]) != U64_MAX), "connection %d: a verdict without a close frame" % j
            if v != sl.NONE:   # disconnected: the next carry drops it, its later bytes are never read
                assert not gone[j], "connection %d: a dropped stream that is not empty" % j
                gone[j] = True
                run.verdict[j] = (v[0], v[1], v[2] - int(r.stream_first[j]) + frames_done[j])
                continue
            frames_done[j] += int(r.frames_consumed[j])
            frames_left[j] -= int(r.frames_consumed[j])
            if getattr(r, carries, None) is not None:
                state[j], run.proto[j] = int(getattr(r, carries)[j]), (int(r.proto[j][0]), int(r.proto[j][1]))
        if getattr(r, "spans_left", None) is not None:
            spans, close_off = r.spans_left, r.close_left
        else:
            spans = np.array(spans, dtype=STREAM_SPAN, copy=True)
            spans["consumed"] = r.bytes_consumed
            close_off = np.array([int(x) for x in r.close_off[:n]], dtype=np.uint64)
    # what is left of every connection: one more carry, without new bytes
    wire, spans = carry(wire, spans, close_off, np.zeros(0, dtype=np.uint8), np.zeros(n, dtype=STREAM_READ))
    wire, spans = _host(wire), _host(spans).view(STREAM_SPAN)
    for j in range(n):
        run.left[j] = wire[int(spans["off"][j]):][: int(spans["len"][j])].tobytes()
        assert not (gone[j] and run.left[j]), "connection %d: dropped and not empty" % j
    if hasattr(step, "final"):
        state, run.proto = step.final()
    setattr(run, carries, [int(x) for x in state])
    run.out = [bytes(o) for o in run.out]
    return run


def _host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _tails(spans, close_off):
    """The bytes each stream carries."""
    t = (spans["len"] - spans["consumed"]).astype(np.int64)
    if close_off is not None:
        t[close_off[: len(spans)] != U64_MAX] = 0
    return t
