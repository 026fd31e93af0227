"""wsg_frame_streams against wsg_decode_batch on the same wire, kernel times
from the wsg_timing hook (the framer's two walks and the scan between them /
k_decode), the two calls interleaved in one process.  k_decode is the
yardstick: it is what runs next on the table the framer makes, so the ratio
says what the framer adds to a receive pass.

Shapes:
  c2            the C2 wire, 4096 x 64 KiB masked frames, one stream per frame
  c3            65536 ragged frames (C3's lengths, uniform in [128, 65536]) as
                4096 streams of 16 frames
  echo_100      the C1 echo shape: 100 streams of 1000 x 38-byte frames
  echo_10000    ... 10 000 streams
  serial        one stream of 1 Mi 38-byte frames: the serial worst case

Per shape: median / min / max kernel microseconds of either call over the
repetitions, `spread` = (max - min) / median of that call's own repetitions,
and ratio = framer median / k_decode median.  The framer's table is checked
against the wire's own once, untimed.  Prints one JSON line.

usage: python tools/framebench.py [--reps 40] [--warmup 10] [--small]
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
from cppserver_amd.layout import RECV_INFO, STREAM_SPAN  # noqa: E402


def spans_of(fs, wire_len, per_stream):
    """Streams of per_stream consecutive frames of the table fs (host uint64)."""
    edges = np.concatenate([fs[::per_stream], [np.uint64(wire_len)]]).astype(np.uint64)
    spans = np.zeros(len(edges) - 1, dtype=STREAM_SPAN)
    spans["off"] = edges[:-1]
    spans["len"] = edges[1:] - edges[:-1]
    return spans


def shape_c2(small):
    n, size = (64, 4096) if small else (4096, 65536)
    wire, fs, _ = wl.c2_wire(n, size, seed=2)
    return torch.from_numpy(wire).cuda(), fs, spans_of(fs, len(wire), 1)


def shape_c3(codec, small):
    n, per_stream, hi = (1024, 16, 4096) if small else (65536, 16, 65536)
    rng = np.random.default_rng(3)
    desc, total = wl.ragged_desc(rng, rng.integers(128, hi + 1, n))
    payload = torch.from_numpy(wl.random_bytes(rng, total)).cuda()
    cap = int(ca.frame_sizes(desc).sum())
    wire = torch.empty(cap, dtype=torch.uint8, device="cuda")
    woff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode_batch(payload, ca.desc_to_tensor(desc, "cuda"), wire=wire, wire_cap=cap, wire_off=woff)
    codec.sync()
    fs = woff[:n].cpu().numpy().view(np.uint64)
    return wire, fs, spans_of(fs, cap, per_stream)


def shape_echo(streams, per_stream):
    """streams x per_stream masked binary frames of 32 payload bytes (38 bytes each)."""
    rng = np.random.default_rng(1)
    frame = np.frombuffer(ca.header_pack(0x82, True, 32, key=0x1A2B3C4D), dtype=np.uint8)
    frame = np.concatenate([frame, rng.integers(0, 256, 32, dtype=np.uint8)])
    assert len(frame) == 38
    n = streams * per_stream
    wire = torch.from_numpy(frame).cuda().repeat(n)
    fs = np.arange(n, dtype=np.uint64) * np.uint64(38)
    return wire, fs, spans_of(fs, 38 * n, per_stream)


def stats(us):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "spread": round((max(us) - min(us)) / med, 4)}


def measure(codec, name, wire, fs, spans, reps, warmup):
    n, ns = len(fs), len(spans)
    d_fs = torch.from_numpy(fs.view(np.int64)).cuda()
    d_spans = torch.from_numpy(spans.view(np.uint8)).cuda()
    out = torch.empty_like(wire)
    info = torch.empty(n * RECV_INFO.itemsize, dtype=torch.uint8, device="cuda")
    table = torch.empty(n, dtype=torch.int64, device="cuda")
    sf = torch.empty(ns + 1, dtype=torch.int32, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")

    def batch():
        codec.decode_batch(wire, d_fs, out=out, info=info)

    def framer():
        codec.frame_streams(wire, d_spans, frame_start=table, frame_cap=n, stream_first=sf, count=count)

    # once untimed, checked: the timed calls below do this work and nothing fails silently
    framer()
    codec.sync()
    cnt = [int(x) for x in count.cpu()]
    if cnt != [n, int(wire.numel())] or not torch.equal(table, d_fs):
        raise SystemExit("%s: the framer's table is not the wire's (%r frames, bytes)" % (name, cnt))
    for _ in range(warmup):
        batch()
        framer()
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    t_batch, t_frame = [], []
    for _ in range(reps):   # interleaved: both calls see the same machine state
        batch()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_batch.append(ms * 1e3)
        framer()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_frame.append(ms * 1e3)
    codec.timing(False)
    codec.sync()
    b, f = stats(t_batch), stats(t_frame)
    return {"frames": n, "streams": ns, "wire_bytes": int(wire.numel()), "decode_batch": b, "frame_streams": f,
            "ratio": round(f["median_us"] / b["median_us"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "framebench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    per = 50 if a.small else 1000
    shapes = [("c2", lambda: shape_c2(a.small)), ("c3", lambda: shape_c3(codec, a.small)),
              ("echo_100", lambda: shape_echo(100, per)),
              ("echo_10000", lambda: shape_echo(200 if a.small else 10000, per)),
              ("serial", lambda: shape_echo(1, 4096 if a.small else 1 << 20))]
    for name, make in shapes:
        wire, fs, spans = make()
        res["shapes"][name] = measure(codec, name, wire, fs, spans, a.reps, a.warmup)
        del wire, fs, spans
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
