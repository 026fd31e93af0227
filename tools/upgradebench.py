"""wsg_upgrade_streams on a reconnect storm: 65536 connections' upgrade requests
judged in one call, against the same requests on one host core.

Shapes (65536 streams each, every stream with a key of its own):
  rfc       the RFC 6455 1.3 request (230 bytes, seven headers)
  browser   a browser-sized request of about 500 bytes with a dozen headers
One stream in 64 carries a wrong Sec-WebSocket-Version, so that 400 responses
are produced and checked.  Before any timing every output of the call is
compared with layout.upgrade_plan.

Times, median / min / max over the repetitions (`spread` = (max - min) /
median):
  call          the whole wsg_upgrade_streams call (five kernels), device events
                around it, microseconds
  host_judge    wsg_upgrade_judge over the same requests on one host core,
                nanoseconds per request (tools/bench_upgrade.cpp)
  host_classes  a fresh WSSession::onReceived per request in the same loop
                (HTTPRequest::Parse, PerformServerUpgrade with OpenSSL's SHA-1,
                HTTPResponse), nanoseconds per request
`bytes` are the call's algorithmic bytes: the request bytes up to the header
end read once, 32 per span read and 16 written, 32 per record written, the
responses written, 8 per response offset; frac_of_8TBps is taken on the call.
--membench: tools/_build/membench copies bytes / 2 (it reads and writes that
many), and `frac_of_membench` is its best copy's time over the call's.
Prints one JSON line.

usage: python tools/upgradebench.py [--reps 40] [--warmup 10] [--small] [--membench]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from tests import upgrade_cases as uc  # noqa: E402

PEAK = 8e12   # HBM bytes/s


def requests(name, n):
    base = uc.RFC_REQUEST if name == "rfc" else uc.browser_request()
    old = uc.KEY if name == "rfc" else b"x3JJHMbDL1EzLkh9GBhXDw=="
    out = []
    for j in range(n):
        r = base.replace(old, uc.key_of_length(24, j))
        if j % 64 == 63:
            r = r.replace(b"Sec-WebSocket-Version: 13", b"Sec-WebSocket-Version: 12")
        out.append(r)
    return out


def stats(xs, unit):
    med = statistics.median(xs)
    return {"median_" + unit: round(med, 2), "min_" + unit: round(min(xs), 2), "max_" + unit: round(max(xs), 2),
            "spread": round((max(xs) - min(xs)) / med, 4)}


def host_side(reqs, reps):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        with open(path, "wb") as f:
            f.write(uc.pack_cases(reqs))
        r = subprocess.run([os.path.join(ROOT, "tools", "_build", "bench_upgrade"), path, str(reps)],
                           capture_output=True, text=True, check=True)
    judge = [float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("judge ")]
    classes = [float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("classes ")]
    return stats(judge, "ns"), stats(classes, "ns")


def membench_us(nbytes):
    mib = max(1, round(nbytes / 2 / (1 << 20)))
    r = subprocess.run([os.path.join(ROOT, "tools", "_build", "membench"), str(mib)], capture_output=True, text=True,
                       check=True, timeout=300)
    times = [float(m.group(1)) for m in re.finditer(r"^oop .*?([0-9.]+) us", r.stdout, re.M)]   # its out-of-place copies
    if not times:
        raise SystemExit("membench printed no copy line:\n" + r.stdout[-2000:])
    best = min(times)
    return mib, best


def measure(codec, name, n, reps, warmup, membench):
    reqs = requests(name, n)
    wire, spans = uc.batch(reqs)
    want = layout.upgrade_plan(wire, spans)
    total = int(want[3][-1])
    d_wire = torch.zeros(len(wire) + 32, dtype=torch.uint8, device="cuda")[: len(wire)]
    d_wire.copy_(torch.from_numpy(wire))
    d_spans = torch.from_numpy(spans.view(np.uint8)).cuda()
    up, resp, resp_off, count = codec.upgrade_streams(d_wire, d_spans, resp_cap=total)
    codec.sync()
    # once untimed, verified against the numpy restatement: nothing below fails silently
    sp = d_spans.cpu().numpy().view(layout.STREAM_SPAN)
    if up.cpu().numpy()[: n * 32].tobytes() != want[0].tobytes():
        raise SystemExit("%s: d_up differs from layout.upgrade_plan" % name)
    if not (np.array_equal(sp["consumed"], want[1]) and np.array_equal(sp["need"], want[2])):
        raise SystemExit("%s: the spans differ from layout.upgrade_plan" % name)
    if not np.array_equal(resp_off.cpu().numpy().view(np.uint64), want[3]):
        raise SystemExit("%s: d_resp_off differs from layout.upgrade_plan" % name)
    if not np.array_equal(resp.cpu().numpy()[:total], want[4]):
        raise SystemExit("%s: d_resp differs from layout.upgrade_plan" % name)
    if not np.array_equal(count.cpu().numpy().view(np.uint64), want[5]):
        raise SystemExit("%s: d_count differs from layout.upgrade_plan" % name)

    def call():
        codec.upgrade_streams(d_wire, d_spans, resp_cap=total, up=up, resp=resp, resp_off=resp_off, count=count)

    for _ in range(warmup):
        call()
    codec.sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        a.record()
        call()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    nbytes = int(want[1].sum()) + (32 + 16) * n + 32 * n + total + 8 * (n + 1) + 32
    c = stats(t, "us")
    c.update(bytes=nbytes, frac_of_8TBps=round(nbytes / (c["median_us"] * 1e-6) / PEAK, 5),
             ns_per_request=round(c["median_us"] * 1e3 / n, 3))
    judge, classes = host_side(reqs, max(3, min(reps, 9)))
    out = {"streams": n, "request_bytes": len(reqs[0]), "accepted": int(want[5][0]), "rejected": int(want[5][1]),
           "response_bytes": total, "call": c, "host_judge": judge, "host_classes": classes,
           "judge_over_call": round(judge["median_ns"] / c["ns_per_request"], 1),
           "classes_over_call": round(classes["median_ns"] / c["ns_per_request"], 1)}
    if membench:
        mib, us = membench_us(nbytes)
        out["membench"] = {"copy_mib": mib, "best_copy_us": us, "frac_of_membench": round(us / c["median_us"], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--membench", action="store_true", help="also run tools/_build/membench on the same bytes")
    a = ap.parse_args()
    codec = ca.Codec(0)
    n = 1024 if a.small else 65536
    res = {"tool": "upgradebench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in ("rfc", "browser"):
        res["shapes"][name] = measure(codec, name, n, a.reps, a.warmup, a.membench)
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
