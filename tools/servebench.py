"""wsg_reply_checked against wsg_reply_messages followed by wsg_check_protocol
on the same wire, the three calls interleaved in one process.  The fused call
launches the kernels of the other two (the checked instantiations of the
three reply kernels in the place of the plain ones) and three
one-lane-per-stream kernels more; in both forms the protocol check reads the
d_info that the reply's header pass wrote, so the fused call saves no pass over
the wire, only the host's second call.

Shapes: tools/protobench.py's (c2, c3_frag, small), every frame masked, the
role WSG_PROTO_SERVER, one stream in 64 with a reserved opcode somewhere.

Before any timing the fused call's d_verdict, d_proto and d_result are
compared with layout.protocol_plan over the d_info read back, its
d_reply_off, d_stream_reply, d_close_off and d_count with
layout.checked_reply_plan over the message table read back, every close frame
with the four bytes 88 02 03 EA, and the reply range of every stream without
a verdict with the same stream's range of wsg_reply_messages' output.

Times, median / min / max microseconds over the repetitions, device events
around each call (`spread` = (max - min) / median):
  reply_call     wsg_reply_messages
  check_call     wsg_check_protocol behind it
  two_calls      their sum, repetition by repetition
  checked_call   wsg_reply_checked
excess_us = checked_call's median - two_calls' median; within_spread says
whether that is at most checked_call's own max - min.  Prints one JSON line.

usage: python tools/servebench.py [--reps 40] [--warmup 10] [--small] [--shapes c2,c3_frag,small]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd import workloads as wl  # noqa: E402
from cppserver_amd.layout import MSG, PROTO_STATE, PROTO_VERDICT, RECV_INFO, STREAM_STATE  # noqa: E402
from tools.protobench import LIMIT, shape, stats  # noqa: E402

U64_MAX = np.uint64(2**64 - 1)


class Outputs:
    def __init__(self, n, ns, cap):
        u8 = lambda k: torch.empty(max(k, 16), dtype=torch.uint8, device="cuda")  # noqa: E731
        i64 = lambda k: torch.empty(k, dtype=torch.int64, device="cuda")  # noqa: E731
        self.reply, self.reply_off, self.stream_reply, self.close_off = u8(cap), i64(n + 1), i64(ns + 1), i64(ns)
        self.msgs, self.info, self.count = u8(n * MSG.itemsize), u8(n * RECV_INFO.itemsize), i64(5)
        self.state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.proto = torch.zeros(ns * PROTO_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.verdict, self.result = u8(ns * PROTO_VERDICT.itemsize), i64(3)


def verify(name, n, ns, stream_first, wire, two, one):
    """The fused call's outputs (one) against the models and the two-call form (two)."""
    def fail(what):
        raise SystemExit("%s: %s" % (name, what))

    info = one.info.cpu().numpy().view(RECV_INFO)[:n]
    consumed = one.state.cpu().numpy().view(STREAM_STATE)["consumed"]
    closes = int((info["opcode"] == 8).sum())
    want_v, want_p, want_r = layout.protocol_plan(info, stream_first, None, ca.PROTO_SERVER, LIMIT,
                                                  wire.cpu().numpy() if closes else np.zeros(0, dtype=np.uint8),
                                                  consumed)
    verdict = one.verdict.cpu().numpy()[: ns * 8].view(np.uint64)
    for got, want, what in ((verdict, want_v.view(np.uint64), "d_verdict"),
                            (one.proto.cpu().numpy().view(np.uint64), want_p.view(np.uint64), "d_proto"),
                            (one.result.cpu().numpy().view(np.uint64), want_r, "d_result"),
                            (verdict, two.verdict.cpu().numpy()[: ns * 8].view(np.uint64), "the two calls' d_verdict")):
        if not np.array_equal(got, want):
            fail("%s differs" % what)
    if int(want_r[0]) != len(range(0, ns, 64)):
        fail("%d violating streams, built for %d" % (int(want_r[0]), len(range(0, ns, 64))))
    count = one.count.cpu().numpy().view(np.uint64)
    nm = int(count[0])
    msgs = one.msgs.cpu().numpy().view(MSG)[:nm]
    if not np.array_equal(one.msgs.cpu().numpy()[: nm * MSG.itemsize], two.msgs.cpu().numpy()[: nm * MSG.itemsize]):
        fail("d_msgs differs from wsg_reply_messages'")
    reply_off, stream_reply, close_off, rcount = layout.checked_reply_plan(msgs, want_v, layout.ECHO_REPLY, 0, None, ns)
    for got, want, what in ((one.reply_off.cpu().numpy().view(np.uint64)[: nm + 1], reply_off, "d_reply_off"),
                            (one.stream_reply.cpu().numpy().view(np.uint64), stream_reply, "d_stream_reply"),
                            (one.close_off.cpu().numpy().view(np.uint64), close_off, "d_close_off"),
                            (count[2:5], rcount, "d_count[2..5)")):
        if not np.array_equal(got, want):
            fail("%s differs from layout.checked_reply_plan" % what)
    a, b = one.reply.cpu().numpy(), two.reply.cpu().numpy()
    sr2 = two.stream_reply.cpu().numpy().view(np.uint64)
    for j in range(ns):
        lo, hi = int(stream_reply[j]), int(stream_reply[j + 1])
        if close_off[j] != U64_MAX:
            if a[hi - 4: hi].tobytes() != b"\x88\x02\x03\xea" or int(close_off[j]) != hi - 4:
                fail("stream %d: not closed with 1002 at the end of its range" % j)
        elif not np.array_equal(a[lo:hi], b[int(sr2[j]): int(sr2[j + 1])]):
            fail("stream %d: replies differ from wsg_reply_messages'" % j)
    return int(want_r[0]), int(rcount[0])


def measure(codec, name, desc, total, stream_first, reps, warmup):
    n, ns = len(desc), len(stream_first) - 1
    rng = np.random.default_rng(5)
    payload = torch.from_numpy(wl.random_bytes(rng, min(total, 1 << 24))).cuda().repeat(-(-total // (1 << 24)))[:total]
    cap = int(ca.frame_sizes(desc).sum())
    wire = torch.empty(cap, dtype=torch.uint8, device="cuda")
    woff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode_batch(payload, ca.desc_to_tensor(desc, "cuda"), wire=wire, wire_cap=cap, wire_off=woff)
    codec.sync()
    del payload
    fs, sf = woff[:n].contiguous(), torch.from_numpy(stream_first).cuda()
    rcap = cap + 14 * n
    two, one = Outputs(n, ns, rcap), Outputs(n, ns, rcap)

    def reply():
        two.state.zero_()
        codec.reply_messages(wire, fs, sf, state=two.state, reply=two.reply, reply_cap=rcap, reply_off=two.reply_off,
                             stream_reply=two.stream_reply, msgs=two.msgs, count=two.count[:4], info=two.info)

    def check():
        two.proto.zero_()
        codec.check_protocol(wire, two.info, n, sf, proto=two.proto, role=ca.PROTO_SERVER, max_message=LIMIT,
                             state=two.state, verdict=two.verdict, result=two.result)

    def checked():
        one.state.zero_()
        one.proto.zero_()
        codec.reply_checked(wire, fs, sf, proto=one.proto, role=ca.PROTO_SERVER, max_message=LIMIT, state=one.state,
                            reply=one.reply, reply_cap=rcap, reply_off=one.reply_off, stream_reply=one.stream_reply,
                            close_off=one.close_off, verdict=one.verdict, result=one.result, msgs=one.msgs,
                            count=one.count, info=one.info)

    # once untimed, verified: nothing below fails silently
    reply()
    check()
    checked()
    if codec.sync_status() != 0:
        raise SystemExit("%s: an error was latched" % name)
    violating, reply_bytes = verify(name, n, ns, stream_first, wire, two, one)
    for _ in range(warmup):
        reply()
        check()
        checked()
    codec.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    t_reply, t_check, t_checked = [], [], []
    for _ in range(reps):   # interleaved: the calls see the same machine state
        two.state.zero_()
        two.proto.zero_()
        one.state.zero_()
        one.proto.zero_()
        ev[0].record()
        codec.reply_messages(wire, fs, sf, state=two.state, reply=two.reply, reply_cap=rcap, reply_off=two.reply_off,
                             stream_reply=two.stream_reply, msgs=two.msgs, count=two.count[:4], info=two.info)
        ev[1].record()
        ev[2].record()
        codec.check_protocol(wire, two.info, n, sf, proto=two.proto, role=ca.PROTO_SERVER, max_message=LIMIT,
                             state=two.state, verdict=two.verdict, result=two.result)
        ev[3].record()
        ev[4].record()
        codec.reply_checked(wire, fs, sf, proto=one.proto, role=ca.PROTO_SERVER, max_message=LIMIT, state=one.state,
                            reply=one.reply, reply_cap=rcap, reply_off=one.reply_off, stream_reply=one.stream_reply,
                            close_off=one.close_off, verdict=one.verdict, result=one.result, msgs=one.msgs,
                            count=one.count, info=one.info)
        ev[5].record()
        ev[5].synchronize()
        t_reply.append(ev[0].elapsed_time(ev[1]) * 1e3)
        t_check.append(ev[2].elapsed_time(ev[3]) * 1e3)
        t_checked.append(ev[4].elapsed_time(ev[5]) * 1e3)
    codec.sync()
    both = stats([a + b for a, b in zip(t_reply, t_check)])
    fused = stats(t_checked)
    excess = round(fused["median_us"] - both["median_us"], 2)
    return {"frames": n, "streams": ns, "violating_streams": violating, "reply_bytes": reply_bytes,
            "reply_call": stats(t_reply), "check_call": stats(t_check), "two_calls": both, "checked_call": fused,
            "excess_us": excess, "within_spread": bool(excess <= fused["max_us"] - fused["min_us"]),
            "time_ratio": round(fused["median_us"] / both["median_us"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--shapes", default="c2,c3_frag,small", help="which shapes, comma-separated")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "servebench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.shapes.split(","):
        desc, total, sf = shape(name, a.small)
        res["shapes"][name] = measure(codec, name, desc, total, sf, a.reps, a.warmup)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
