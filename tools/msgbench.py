"""wsg_decode_messages against wsg_decode_batch on the same wire, kernel times
from the wsg_timing hook (k_msg_gather / k_decode), the two calls interleaved
in one process.  k_decode is the yardstick: the gather's algorithmic bytes are
k_decode's minus the header bytes, so parity of the byte rates is the aim.

Shapes:
  c2        the C2 wire, 4096 x 64 KiB masked frames, one frame per message,
            one stream per frame
  c2_aligned (--diag) the C2 frames spaced so that every payload is 16-byte
            aligned in the wire: the gather without its source shift
  c3_frag   65536 ragged frames (C3's lengths, uniform in [128, 65536]) in 4096
            streams of 16 frames, messages of 1-8 fragments

Per shape and call: median / min / max kernel microseconds over the
repetitions, the algorithmic bytes (decode_batch: wire read + wire written +
frame table and info; decode_messages: payload read + message bytes written +
frame table, info, stream table, state and message records), the fraction of
8 TB/s, and the ratio of decode_messages' byte rate to k_decode's.  `spread`
is (max - min) / median of that call's own repetitions.  Prints one JSON line.

usage: python tools/msgbench.py [--reps 40] [--warmup 10] [--small]
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


def fragment_opcodes(rng, n, per_stream):
    """First-byte values for n frames in streams of per_stream frames: messages
    of 1-8 fragments (binary, continuations, FIN on the last), cut at the end of
    every stream."""
    op = np.zeros(n, dtype=np.uint8)
    i = 0
    while i < n:
        left = per_stream - i % per_stream
        k = min(int(rng.integers(1, 9)), left)
        op[i] = 0x02
        op[i + k - 1] |= 0x80
        i += k
    return op


def shape_c2(small):
    n, size = (64, 4096) if small else (4096, 65536)
    wire, fs, _ = wl.c2_wire(n, size, seed=2)
    return (torch.from_numpy(wire).cuda(), torch.from_numpy(fs.view(np.int64)).cuda(),
            torch.arange(n + 1, dtype=torch.int32, device="cuda"), n * size, None)


def shape_c2_aligned(small):
    """Diagnostic: the C2 frames two bytes apart, so that every payload starts
    16 bytes past a 16-byte boundary of the wire (source shift 0 in the gather)."""
    n, size = (64, 4096) if small else (4096, 65536)
    wire, fs, _ = wl.c2_wire(n, size, seed=2)
    fsz = len(wire) // n
    stride = (fsz + 15) // 16 * 16
    lead = (16 - (fsz - size) % 16) % 16
    spaced = np.zeros(n * stride + 16, dtype=np.uint8)
    starts = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(lead)
    idx = (starts[:, None] + np.arange(fsz, dtype=np.uint64)[None, :]).reshape(-1)
    spaced[idx] = wire
    return (torch.from_numpy(spaced).cuda(), torch.from_numpy(starts.view(np.int64)).cuda(),
            torch.arange(n + 1, dtype=torch.int32, device="cuda"), n * size, None)


def shape_c3_frag(codec, small):
    n, per_stream, hi = (1024, 16, 4096) if small else (65536, 16, 65536)
    rng = np.random.default_rng(3)
    desc, total = wl.ragged_desc(rng, rng.integers(128, hi + 1, n))
    desc["opcode"] = fragment_opcodes(rng, n, per_stream)
    payload = torch.from_numpy(wl.random_bytes(rng, total)).cuda()
    cap = int(ca.frame_sizes(desc).sum())
    wire = torch.empty(cap, dtype=torch.uint8, device="cuda")
    woff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode_batch(payload, ca.desc_to_tensor(desc, "cuda"), wire=wire, wire_cap=cap, wire_off=woff)
    codec.sync()
    sf = torch.arange(0, n + 1, per_stream, dtype=torch.int32, device="cuda")
    return wire, woff[:n].contiguous(), sf, total, payload


def stats(us):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "spread": round((max(us) - min(us)) / med, 4)}


def measure(codec, name, wire, fs, sf, payload_bytes, payload, reps, warmup):
    n, ns = int(fs.numel()), int(sf.numel()) - 1
    out = torch.empty_like(wire)
    info = torch.empty(n * RECV_INFO.itemsize, dtype=torch.uint8, device="cuda")
    msg = torch.empty(int(wire.numel()), dtype=torch.uint8, device="cuda")
    msgs = torch.empty(n * MSG.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")

    def batch():
        codec.decode_batch(wire, fs, out=out, info=info)

    def messages():
        state.zero_()
        codec.decode_messages(wire, fs, sf, state=state, msg=msg, msgs=msgs, count=count, info=info)

    # once untimed, checked: the timed calls below do this work and nothing fails silently
    messages()
    codec.sync()
    cnt = [int(x) for x in count.cpu()]
    if cnt[1] != payload_bytes:
        raise SystemExit("%s: %d message bytes, expected %d" % (name, cnt[1], payload_bytes))
    if payload is not None and not torch.equal(msg[:payload_bytes], payload[:payload_bytes]):
        raise SystemExit("%s: the message bytes are not the payloads the wire was encoded from" % name)
    for _ in range(warmup):
        batch()
        messages()
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    t_batch, t_msg = [], []
    for _ in range(reps):   # interleaved: both calls see the same machine state
        batch()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_batch.append(ms * 1e3)
        messages()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_msg.append(ms * 1e3)
    codec.timing(False)
    codec.sync()
    wire_len = int(wire.numel())
    bytes_batch = 2 * wire_len + (8 + RECV_INFO.itemsize) * n
    bytes_msg = (2 * payload_bytes + (8 + RECV_INFO.itemsize) * n + 4 * (ns + 1) + 2 * STREAM_STATE.itemsize * ns
                 + MSG.itemsize * cnt[0])
    b, m = stats(t_batch), stats(t_msg)
    rate_b = bytes_batch / (b["median_us"] * 1e-6)
    rate_m = bytes_msg / (m["median_us"] * 1e-6)
    b.update(bytes=bytes_batch, frac_of_8TBps=round(rate_b / PEAK, 4))
    m.update(bytes=bytes_msg, frac_of_8TBps=round(rate_m / PEAK, 4))
    return {"frames": n, "streams": ns, "messages": cnt[0], "wire_bytes": wire_len, "payload_bytes": payload_bytes,
            "decode_batch": b, "decode_messages": m, "byte_rate_ratio": round(rate_m / rate_b, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--diag", action="store_true", help="also c2_aligned: the C2 frames with 16-byte-aligned payloads")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "msgbench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    wire, fs, sf, total, payload = shape_c2(a.small)
    res["shapes"]["c2"] = measure(codec, "c2", wire, fs, sf, total, payload, a.reps, a.warmup)
    del wire, fs, sf, payload
    torch.cuda.empty_cache()
    if a.diag:
        wire, fs, sf, total, payload = shape_c2_aligned(a.small)
        res["shapes"]["c2_aligned"] = measure(codec, "c2_aligned", wire, fs, sf, total, payload, a.reps, a.warmup)
        del wire, fs, sf, payload
        torch.cuda.empty_cache()
    wire, fs, sf, total, payload = shape_c3_frag(codec, a.small)
    res["shapes"]["c3_frag"] = measure(codec, "c3_frag", wire, fs, sf, total, payload, a.reps, a.warmup)
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
