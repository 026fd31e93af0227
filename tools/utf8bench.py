"""wsg_check_utf8 against wsg_decode_messages on the same batch, kernel times
from the wsg_timing hook (k_utf8_scan / k_msg_gather), the two calls
interleaved in one process.  k_msg_gather is the yardstick: the scan reads each
payload byte once and writes almost nothing, half the gather's algorithmic
bytes.

Shapes (tools/msgbench.py's, every message text):
  c2        4096 x 64 KiB masked frames, one frame per message, one stream per
            frame
  c3_frag   65536 ragged frames (uniform in [128, 65536]) in 4096 streams of 16
            frames, messages of 1-8 fragments, cut anywhere (inside a sequence
            too)

Corpora, from a seed, whole code points per message:
  ascii     bytes 20-7E
  mixed     valid text, sequences of 1-4 bytes in equal byte shares
  corrupt   the mixed text with one byte of every message FF (at the start of
            a code point, so that valid_up_to is known)

Before timing, d_valid and d_result are compared with what the corpus was
built to give; with --small (toy sizes) d_valid is also compared with Python's
decoder over the message bytes read back.  Per shape and corpus: median / min
/ max kernel microseconds of k_utf8_scan and of k_msg_gather over the
repetitions, `spread` = (max - min) / median, the scan's algorithmic bytes
(payload read once + records read by the three kernels + d_valid and d_result
written), its fraction of 8 TB/s, and time_ratio = scan / gather.  Prints one
JSON line.

usage: python tools/utf8bench.py [--reps 40] [--warmup 10] [--small]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cppserver_amd as ca  # noqa: E402
from cppserver_amd import workloads as wl  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_STATE  # noqa: E402

PEAK = 8e12   # HBM bytes/s
U64_MAX = 2 ** 64 - 1


def text_pool(rng, nbytes):
    """(pool bytes, bounds): valid text of about nbytes bytes, sequences of 1-4
    bytes in equal byte shares; bounds[i] is the offset of code point i
    (bounds[-1] = len(pool))."""
    size = rng.choice(4, size=nbytes // 2, p=np.array([12, 6, 4, 3]) / 25.0) + 1   # P(k bytes) ~ 1 / k
    lo = np.array([0x20, 0x80, 0x800, 0x10000])[size - 1]
    hi = np.array([0x7F, 0x800, 0x10000, 0x110000])[size - 1]
    cps = lo + (rng.random(len(size)) * (hi - lo)).astype(np.int64)
    cps[(cps >= 0xD800) & (cps < 0xE000)] = 0xE000
    pool = np.frombuffer("".join(map(chr, cps.tolist())).encode("utf-8"), dtype=np.uint8)
    bounds = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    assert bounds[-1] == len(pool)
    return pool, bounds


def fragment_opcodes(rng, n, per_stream):
    """tools/msgbench.py's messages of 1-8 fragments, as text."""
    op = np.zeros(n, dtype=np.uint8)
    first = []
    i = 0
    while i < n:
        left = per_stream - i % per_stream
        k = min(int(rng.integers(1, 9)), left)
        op[i] = 0x01
        op[i + k - 1] |= 0x80
        first.append(i)
        i += k
    return op, np.array(first + [n], dtype=np.int64)


class Shape:
    """The frames of a shape (descriptors over one payload arena in message
    order) and its messages' offsets in that arena."""

    def __init__(self, name, small):
        rng = np.random.default_rng(3)
        if name == "c2":
            n, size = (64, 4096) if small else (4096, 65536)
            self.desc, self.total = wl.ragged_desc(rng, np.full(n, size), opcode=0x81)
            self.first = np.arange(n + 1, dtype=np.int64)
            self.stream_first = np.arange(n + 1, dtype=np.int32)
        else:
            n, per_stream, hi = (1024, 16, 4096) if small else (65536, 16, 65536)
            self.desc, self.total = wl.ragged_desc(rng, rng.integers(128, hi + 1, n))
            self.desc["opcode"], self.first = fragment_opcodes(rng, n, per_stream)
            self.stream_first = np.arange(0, n + 1, per_stream, dtype=np.int32)
        self.n = n
        ends = np.concatenate([self.desc["src_off"].astype(np.int64), [self.total]])
        self.msg_off = ends[self.first]                 # len(messages) + 1 offsets into the arena
        self.msg_len = np.diff(self.msg_off)


def fill(shape, corpus, rng, pool, bounds, d_pool, d_ascii):
    """The payload arena on the device and the valid_up_to every message was built to have."""
    total, nmsg = shape.total, len(shape.msg_len)
    payload = torch.empty(total, dtype=torch.uint8, device="cuda")
    for at in range(0, total, int(d_ascii.numel())):    # ASCII everywhere first
        k = min(int(d_ascii.numel()), total - at)
        payload[at: at + k] = d_ascii[:k]
    want = shape.msg_len.copy()
    if corpus == "ascii":
        return payload, want
    # message m: the code points [b, e) of the pool, the most that fit; its last bytes (< 4) stay ASCII
    b = rng.integers(0, len(bounds) // 2, nmsg)
    e = np.searchsorted(bounds, bounds[b] + shape.msg_len, side="right") - 1
    assert (e < len(bounds)).all() and (bounds[e] - bounds[b] <= shape.msg_len).all()
    for m in range(nmsg):
        lo, hi = int(bounds[b[m]]), int(bounds[e[m]])
        payload[int(shape.msg_off[m]): int(shape.msg_off[m]) + hi - lo] = d_pool[lo:hi]
    if corpus == "corrupt":     # FF where a code point begins: everything before it stays valid
        pick = b + (rng.random(nmsg) * np.maximum(e - b, 1)).astype(np.int64)
        pos = np.minimum(bounds[pick] - bounds[b], shape.msg_len - 1)   # (a message of ASCII only: its last byte)
        want = np.where(shape.msg_len > 0, pos, 0)
        at = torch.from_numpy((shape.msg_off[:-1] + pos)[shape.msg_len > 0]).cuda()
        payload[at] = 0xFF
    return payload, want


def stats(us):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "spread": round((max(us) - min(us)) / med, 4)}


def measure(codec, shape, corpus, payload, want, reps, warmup, small):
    n, ns, nmsg = shape.n, len(shape.stream_first) - 1, len(shape.msg_len)
    cap = int(ca.frame_sizes(shape.desc).sum())
    wire = torch.empty(cap, dtype=torch.uint8, device="cuda")
    woff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode_batch(payload, ca.desc_to_tensor(shape.desc, "cuda"), wire=wire, wire_cap=cap, wire_off=woff)
    codec.sync()
    fs, sf = woff[:n].contiguous(), torch.from_numpy(shape.stream_first).cuda()
    info = torch.empty(n * RECV_INFO.itemsize, dtype=torch.uint8, device="cuda")
    msg = torch.empty(cap, dtype=torch.uint8, device="cuda")
    msgs = torch.empty(n * MSG.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
    valid = torch.empty(n, dtype=torch.int64, device="cuda")
    result = torch.empty(4, dtype=torch.int64, device="cuda")

    def messages():
        state.zero_()
        codec.decode_messages(wire, fs, sf, state=state, msg=msg, msgs=msgs, count=count, info=info)

    def check():
        codec.check_utf8(msg, msgs, count, which=ca.UTF8_TEXT, msg_cap=cap, msg_room=n, valid=valid, result=result)

    # once untimed, checked: the timed calls below do this work and nothing fails silently
    messages()
    check()
    codec.sync()
    cnt = [int(x) for x in count.cpu()]
    if cnt != [nmsg, shape.total] or not torch.equal(msg[: shape.total], payload):
        raise SystemExit("%s/%s: the decode did not give the payload back" % (shape.name, corpus))
    got = valid[:nmsg].cpu().numpy()
    if not np.array_equal(got, want):
        raise SystemExit("%s/%s: d_valid differs from the corpus in %d messages" % (shape.name, corpus,
                                                                                    int((got != want).sum())))
    bad = np.flatnonzero(want < shape.msg_len)
    res = [int(x) for x in result.cpu().numpy().view(np.uint64)]
    if res != [len(bad), int(bad[0]) if len(bad) else U64_MAX, nmsg, shape.total]:
        raise SystemExit("%s/%s: d_result %r" % (shape.name, corpus, res))
    if small:   # ... and against Python's decoder over the bytes read back
        host = msg[: shape.total].cpu().numpy().tobytes()
        for m in range(nmsg):
            data = host[int(shape.msg_off[m]): int(shape.msg_off[m + 1])]
            try:
                data.decode("utf-8")
                ref = len(data)
            except UnicodeDecodeError as e:
                ref = e.start
            if ref != int(got[m]):
                raise SystemExit("%s/%s: message %d: d_valid %d, the decoder %d" % (shape.name, corpus, m, got[m], ref))
    for _ in range(warmup):
        messages()
        check()
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    t_msg, t_utf8 = [], []
    for _ in range(reps):   # interleaved: both calls see the same machine state
        messages()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_msg.append(ms * 1e3)
        check()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_utf8.append(ms * 1e3)
    codec.timing(False)
    codec.sync()
    g, u = stats(t_msg), stats(t_utf8)
    bytes_utf8 = shape.total + 3 * MSG.itemsize * nmsg + 2 * 8 * nmsg + 4 * 8
    u.update(bytes=bytes_utf8, frac_of_8TBps=round(bytes_utf8 / (u["median_us"] * 1e-6) / PEAK, 4))
    return {"messages": nmsg, "frames": n, "payload_bytes": shape.total, "invalid": len(bad),
            "k_utf8_scan": u, "k_msg_gather": g, "time_ratio": round(u["median_us"] / g["median_us"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "utf8bench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    rng = np.random.default_rng(17)
    pool, bounds = text_pool(rng, (1 << 16) if a.small else (4 << 20))
    d_pool = torch.from_numpy(pool.copy()).cuda()
    d_ascii = torch.from_numpy(rng.integers(0x20, 0x7F, 1 << 24, dtype=np.uint8)).cuda()
    for name in ("c2", "c3_frag"):
        shape = Shape(name, a.small)
        shape.name = name
        res["shapes"][name] = {}
        for corpus in ("ascii", "mixed", "corrupt"):
            payload, want = fill(shape, corpus, np.random.default_rng(18), pool, bounds, d_pool, d_ascii)
            res["shapes"][name][corpus] = measure(codec, shape, corpus, payload, want, a.reps, a.warmup, a.small)
            del payload
            torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
