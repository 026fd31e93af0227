"""wsg_upgrade_client_streams on a connect storm: 65536 client connections'
upgrade responses judged in one call, against wsg_upgrade_streams on as many
requests in the same process (the yardstick: same walk, same stream count) and
against the same responses on one host core; and wsg_upgrade_requests for the
same connections against the runtime's device-to-device copy of as many bytes.

Workload: 65536 streams, each the 148-byte 101 response wsg_upgrade_streams
answers a nonce of its own with, followed by one unmasked text frame; one
stream in 64 is tampered with (an accept letter changed, or another status).
Before any timing every output of the call is compared with
layout.upgrade_client_plan, and every request with layout.upgrade_request.

Times, median / min / max over the repetitions (`spread` = (max - min) /
median), device events around the whole call, microseconds; the two _streams
calls are interleaved, one of each a repetition:
  client        wsg_upgrade_client_streams (four kernels)
  server        wsg_upgrade_streams over 65536 RFC 6455 1.3 requests (five kernels)
  requests      wsg_upgrade_requests, 65536 x 230 bytes
  copy          hipMemcpyAsync device to device of the same 65536 x 230 bytes
  host_judge    wsg_upgrade_client_judge over the responses on one host core,
                nanoseconds per response (tools/bench_upgrade_client.cpp)
  host_classes  a fresh WSClient::onReceived per response in the same loop
`bytes` of the client call: the response bytes up to the header end read once,
16 per nonce, 32 per span read and 16 written, 32 per record written, 32 per
digest written and read.
Prints one JSON line.

usage: python tools/upgradeclientbench.py [--reps 40] [--warmup 10] [--small] [--no-host]
"""
import argparse
import json
import os
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
from tests import upgrade_cases as us  # noqa: E402
from tests import upgrade_client_cases as uc  # noqa: E402

PEAK = 8e12   # HBM bytes/s
TPL_LEN, KEY_AT = 230, 150


def stats(xs, unit):
    med = statistics.median(xs)
    return {"median_" + unit: round(med, 2), "min_" + unit: round(min(xs), 2), "max_" + unit: round(max(xs), 2),
            "spread": round((max(xs) - min(xs)) / med, 4)}


def padded(a):
    d = torch.zeros(len(a) + 32, dtype=torch.uint8, device="cuda")[: len(a)]
    d.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return d


def client_cases(n):
    rng = np.random.default_rng(26)
    nonces = rng.integers(0, 256, 16 * n, dtype=np.uint8)
    frame = uc.unmasked_text(b"welcome")
    cases = []
    for j in range(n):
        nonce = nonces[16 * j:16 * j + 16].tobytes()
        r = uc.server_response(nonce)
        if j % 128 == 63:
            r = r[:110] + (b"A" if r[110:111] != b"A" else b"B") + r[111:]
        elif j % 128 == 127:
            r = r.replace(b" 101 ", b" 503 ", 1)
        cases.append((r + frame, nonce))
    return cases


def server_requests(n):
    return [us.RFC_REQUEST.replace(us.KEY, us.key_of_length(24, j)) for j in range(n)]


def host_side(cases, reps):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        with open(path, "wb") as f:
            f.write(uc.pack_cases([(data[:148], nonce) for data, nonce in cases]))
        r = subprocess.run([os.path.join(ROOT, "tools", "_build", "bench_upgrade_client"), path, str(reps)],
                           capture_output=True, text=True, check=True)
    judge = [float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("judge ")]
    classes = [float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("classes ")]
    return stats(judge, "ns"), stats(classes, "ns")


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--no-host", action="store_true", help="skip the host-core loops")
    a = ap.parse_args()
    codec = ca.Codec(0)
    n = 1024 if a.small else 65536

    # the client's call, verified against the model
    cases = client_cases(n)
    wire, spans, nonces = uc.batch(cases)
    want = layout.upgrade_client_plan(wire, spans, nonces)
    d_wire, d_spans, d_nonces = padded(wire), torch.from_numpy(spans.view(np.uint8)).cuda(), torch.from_numpy(nonces).cuda()
    up, count = codec.upgrade_client_streams(d_wire, d_spans, d_nonces)
    codec.sync()
    sp = d_spans.cpu().numpy().view(layout.STREAM_SPAN)
    if up.cpu().numpy()[: n * 32].tobytes() != want[0].tobytes():
        raise SystemExit("d_up differs from layout.upgrade_client_plan")
    if not (np.array_equal(sp["consumed"], want[1]) and np.array_equal(sp["need"], want[2])):
        raise SystemExit("the spans differ from layout.upgrade_client_plan")
    if not np.array_equal(count.cpu().numpy().view(np.uint64), want[3]):
        raise SystemExit("d_count differs from layout.upgrade_client_plan")

    # the yardstick: the server's call on as many requests
    swire, sspans = us.batch(server_requests(n))
    swant = layout.upgrade_plan(swire, sspans) if a.small else None
    s_wire, s_spans = padded(swire), torch.from_numpy(sspans.view(np.uint8)).cuda()
    cap = n * 148
    sup, sresp, soff, scount = codec.upgrade_streams(s_wire, s_spans, resp_cap=cap)
    codec.sync()
    if int(scount.cpu()[0]) != n or (swant is not None and sup.cpu().numpy()[: n * 32].tobytes() != swant[0].tobytes()):
        raise SystemExit("wsg_upgrade_streams did not accept every request")

    def client():
        codec.upgrade_client_streams(d_wire, d_spans, d_nonces, up=up, count=count)

    def server():
        codec.upgrade_streams(s_wire, s_spans, resp_cap=cap, up=sup, resp=sresp, resp_off=soff, count=scount)

    for _ in range(a.warmup):
        client()
        server()
    codec.sync()
    tc, ts = [], []
    for _ in range(a.reps):   # interleaved: one of each a repetition
        tc += timed(client, 1)
        ts += timed(server, 1)
    nbytes = int(want[1].sum()) + 16 * n + (32 + 16) * n + 32 * n + 2 * 32 * n + 24
    c, s = stats(tc, "us"), stats(ts, "us")
    c.update(bytes=nbytes, frac_of_8TBps=round(nbytes / (c["median_us"] * 1e-6) / PEAK, 5),
             ns_per_response=round(c["median_us"] * 1e3 / n, 3))
    s.update(ns_per_request=round(s["median_us"] * 1e3 / n, 3))

    # the requests against a copy of as many bytes
    tpl = bytearray(np.random.default_rng(1).integers(32, 127, TPL_LEN, dtype=np.uint8).tobytes())
    tpl[KEY_AT:KEY_AT + 24] = b"=" * 24
    tpl = bytes(tpl)
    d_tpl = padded(np.frombuffer(tpl, dtype=np.uint8))
    total = n * TPL_LEN
    req = torch.empty(total, dtype=torch.uint8, device="cuda")
    codec.upgrade_requests(d_tpl, KEY_AT, d_nonces, req=req, req_cap=total)
    codec.sync()
    got = req.cpu().numpy().reshape(n, TPL_LEN)
    for j in list(range(0, n, max(1, n // 257))) + [n - 1]:
        if got[j].tobytes() != layout.upgrade_request(tpl, KEY_AT, nonces[16 * j:16 * j + 16].tobytes()):
            raise SystemExit("request %d differs from layout.upgrade_request" % j)
    if not (got[:, :KEY_AT] == np.frombuffer(tpl[:KEY_AT], dtype=np.uint8)).all() or not (
            got[:, KEY_AT + 24:] == np.frombuffer(tpl[KEY_AT + 24:], dtype=np.uint8)).all():
        raise SystemExit("a request's template bytes differ")
    src = torch.empty(total, dtype=torch.uint8, device="cuda")

    def requests():
        codec.upgrade_requests(d_tpl, KEY_AT, d_nonces, req=req, req_cap=total)

    def copy():
        src.copy_(req)

    for _ in range(a.warmup):
        requests()
        copy()
    codec.sync()
    tr, tk = [], []
    for _ in range(a.reps):
        tr += timed(requests, 1)
        tk += timed(copy, 1)
    r, k = stats(tr, "us"), stats(tk, "us")
    r.update(bytes=total, frac_of_8TBps=round(total / (r["median_us"] * 1e-6) / PEAK, 5))
    res = {"tool": "upgradeclientbench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "streams": n, "response_bytes": 148,
           "accepted": int(want[3][0]), "rejected": int(want[3][1]), "client": c, "server": s,
           "client_over_server": round(c["median_us"] / s["median_us"], 3),
           "requests": r, "copy": k, "requests_over_copy": round(r["median_us"] / k["median_us"], 3)}
    if not a.no_host:
        judge, classes = host_side(cases, max(3, min(a.reps, 9)))
        res.update(host_judge=judge, host_classes=classes,
                   judge_over_call=round(judge["median_ns"] / c["ns_per_response"], 1),
                   classes_over_call=round(classes["median_ns"] / c["ns_per_response"], 1))
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
