"""wsg_carry_streams on an echo server's two regimes, against the copies it is
held against and the PCIe traffic it removes.

Shapes:
  small   65536 streams, tails of 0-13 bytes, reads of 32-700 bytes
  large   4096 streams, each a 48 KiB tail and a 16 KiB read (a 64 KiB frame
          that completes)
  large_aligned   the large shape with every tail and read on a 128-byte line
          (no source shift: what the sources' phase costs the copy kernel)
Before any timing every output of the call is compared with layout.carry_plan.

Times, median / min / max over the repetitions (`spread` = (max - min) /
median), microseconds, device events around each:
  call        the whole wsg_carry_streams call (four kernels)
  copy        k_carry_copy alone, through wsg_timing (mean of the repetitions)
  membench    tools/_build/membench's best out-of-place copy of the next wire's
              size (the ceiling the copy kernel is held against)
  d2d         hipMemcpyAsync, device to device, of the next wire's bytes
  h2d_wire    hipMemcpyAsync from page-locked memory of the whole next wire
              (what a loop that uploads every round's wire sends)
  h2d_new     ... of the new bytes alone (what the loop with the carry sends)
`bytes` are the call's algorithmic bytes: the next wire written, the tails and
reads read, 32 + 16 + 8 per stream of tables read, 32 written.
Prints one JSON line.

usage: python tools/carrybench.py [--reps 40] [--warmup 10] [--small] [--no-membench]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from tests import carry_cases as kc  # noqa: E402

PEAK = 8e12   # HBM bytes/s


def stats(xs):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2),
            "spread": round((max(xs) - min(xs)) / med, 4)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return stats(t)


def membench_us(nbytes):
    mib = max(1, round(nbytes / (1 << 20)))
    r = subprocess.run([os.path.join(ROOT, "tools", "_build", "membench"), str(mib)], capture_output=True, text=True,
                       check=True, timeout=300)
    times = [float(m.group(1)) for m in re.finditer(r"^oop .*?([0-9.]+) us", r.stdout, re.M)]   # its out-of-place copies
    if not times:
        raise SystemExit("membench printed no copy line:\n" + r.stdout[-2000:])
    return mib, min(times)


def aligned(rng, n, tail, new):
    """n streams of `tail` + `new` bytes whose runs all start on a 128-byte line, nothing consumed."""
    spans = np.zeros(n, dtype=layout.STREAM_SPAN)
    reads = np.zeros(n, dtype=layout.STREAM_READ)
    spans["off"], spans["len"] = np.arange(n, dtype=np.uint64) * np.uint64(tail + 128), tail
    reads["off"], reads["len"] = np.arange(n, dtype=np.uint64) * np.uint64(new + 128), new
    wire_len, new_len = n * (tail + 128), n * (new + 128)
    raw = [rng.integers(0, 256, size + 16, dtype=np.uint8) for size in (wire_len, new_len)]
    return kc.Case(raw[0], wire_len, spans, raw[1], new_len, reads, np.full(n, kc.U64_MAX, dtype=np.uint64))


def measure(codec, hip, name, case, reps, warmup, membench):
    want = case.plan()
    total, ns = int(want[2][0]), case.ns
    d_wire = torch.from_numpy(case.wire_raw).cuda()[: len(case.wire)]
    d_new = torch.from_numpy(case.new_raw).cuda()[: len(case.new)]
    d_spans = torch.from_numpy(case.spans.view(np.uint8)).cuda()
    d_reads = torch.from_numpy(case.reads.view(np.uint8)).cuda()
    d_close = torch.from_numpy(case.close_off.view(np.int64)).cuda()
    nxt, spans, count = codec.carry_streams(d_wire, d_spans, d_new, d_reads, close_off=d_close, next_cap=total)
    codec.sync()
    # once untimed, verified against the numpy restatement: nothing below fails silently
    if not np.array_equal(count.cpu().numpy().view(np.uint64), want[2]):
        raise SystemExit("%s: d_count differs from layout.carry_plan" % name)
    if spans.cpu().numpy()[: ns * 32].tobytes() != want[1].tobytes():
        raise SystemExit("%s: d_next_span differs from layout.carry_plan" % name)
    if not np.array_equal(nxt.cpu().numpy()[:total], want[0]):
        raise SystemExit("%s: d_next differs from layout.carry_plan" % name)

    def call():
        codec.carry_streams(d_wire, d_spans, d_new, d_reads, close_off=d_close, next=nxt, next_cap=total,
                            next_spans=spans, count=count)

    c = timed(call, reps, warmup)
    codec.timing(True)
    for _ in range(reps):
        call()
    codec.sync()
    ms, launches = codec.timing_read()
    codec.timing(False)
    tails, news = int(want[2][1]), int(want[2][2])
    nbytes = total + tails + news + (32 + 16 + 8 + 32) * ns
    c.update(bytes=nbytes, frac_of_8TBps=round(nbytes / (c["median_us"] * 1e-6) / PEAK, 5))
    copy_us = ms * 1e3 / max(launches, 1)
    out = {"streams": ns, "next_bytes": total, "tail_bytes": tails, "new_bytes": news, "call": c,
           "copy": {"mean_us": round(copy_us, 2), "launches": int(launches),
                    "GBps_read_plus_written": round((total + tails + news) / (copy_us * 1e-6) / 1e9, 1)}}
    # the runtime's copies of the same bytes
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    other = torch.empty(total, dtype=torch.uint8, device="cuda")
    pinned = ca.pinned_empty(total)
    pinned[:] = want[0]

    def copy(dst, src, n, kind):
        if hip.hipMemcpyAsync(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(n), kind, st) != 0:
            raise SystemExit("hipMemcpyAsync failed")

    out["d2d"] = timed(lambda: copy(other.data_ptr(), nxt.data_ptr(), total, 3), reps, warmup)
    out["h2d_wire"] = timed(lambda: copy(other.data_ptr(), pinned.ctypes.data, total, 1), reps, warmup)
    out["h2d_new"] = timed(lambda: copy(other.data_ptr(), pinned.ctypes.data, news, 1), reps, warmup)
    out["copy_over_d2d"] = round(copy_us / out["d2d"]["median_us"], 3)
    out["h2d_new_over_h2d_wire"] = round(out["h2d_new"]["median_us"] / out["h2d_wire"]["median_us"], 3)
    if membench:
        del other
        mib, us = membench_us(total)
        out["membench"] = {"copy_mib": mib, "best_copy_us": us, "copy_frac_of_membench": round(us / copy_us, 4),
                           "call_frac_of_membench": round(us / c["median_us"], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--no-membench", action="store_true", help="leave tools/_build/membench out")
    a = ap.parse_args()
    codec = ca.Codec(0)
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    rng = np.random.default_rng(19)
    n_small, n_large = (1024, 64) if a.small else (65536, 4096)
    shapes = {"small": kc.make(rng, rng.integers(0, 14, n_small), rng.integers(32, 701, n_small)),
              "large": kc.make(rng, [48 << 10] * n_large, [16 << 10] * n_large),
              "large_aligned": aligned(rng, n_large, 48 << 10, 16 << 10)}
    res = {"tool": "carrybench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, case in shapes.items():
        res["shapes"][name] = measure(codec, hip, name, case, a.reps, a.warmup,
                                      not a.no_membench and name != "large_aligned")
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
