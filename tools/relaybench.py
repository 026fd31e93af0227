"""wsg_relay_validated (a chat server's round) against wsg_reply_validated (an
echo server's) on the same wire in one process, the calls interleaved:
  echo        wsg_reply_validated, reply_op ECHO_REPLY, mask 0, no keys: every
              data message back to its sender as one unmasked binary frame.
              It moves the same bytes into frames of the same sizes as the
              relay does, so it is the yardstick
  relay_1     wsg_relay_validated, reply_op CHAT_REPLY, relay_op CHAT_RELAY,
              one room (NULL tables)
  relay_1024  the same in 1024 rooms (fewer when there are fewer streams), a
              random d_order
with device events around each call, and the gathers of each through the
wsg_timing hook (the relay call has two: the reply's, which moves the pongs,
and the relay's).

Shapes: tools/servebench.py's (c2, c3_frag, small), every frame masked, the
role WSG_PROTO_SERVER, one stream in 64 with a reserved opcode somewhere.

Before any timing the relay calls' d_relay_off, d_group_relay and d_count[5..8)
are compared with layout.relay_plan over the message table and verdicts read
back, every reply-side table with the same call's under relay_op all zero, and
a sample of the relay frames (all of them in a small batch) byte for byte with
the echo's frame of the same message, whose first byte alone differs.

Times, median / min / max microseconds over the repetitions (`spread` = (max -
min) / median).  ratio = relay's median / echo's; gather_ratio the same for
the gathers; gather_within_spread says whether the relay's gathers are slower
than the echo's by no more than the echo's own max - min.  Prints one JSON line.

usage: python tools/relaybench.py [--reps 40] [--warmup 10] [--small] [--shapes c2,c3_frag,small]
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

WHICH = ca.UTF8_TEXT | ca.UTF8_CLOSE
NONE = (0, 0, 0, 0, 0)
U64_MAX = 2 ** 64 - 1


class Outputs:
    def __init__(self, n, ns, cap, ng):
        u8 = lambda k: torch.empty(max(k, 16), dtype=torch.uint8, device="cuda")  # noqa: E731
        i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device="cuda")  # noqa: E731
        self.reply, self.reply_off, self.stream_reply, self.close_off = u8(cap), i64(n + 1), i64(ns + 1), i64(ns)
        self.relay, self.relay_off, self.group_relay = u8(cap), i64(n), i64(ng + 1)
        self.msgs, self.info, self.count = u8(n * MSG.itemsize), u8(n * RECV_INFO.itemsize), i64(8)
        self.state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.proto = torch.zeros(ns * PROTO_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.verdict, self.result = u8(ns * PROTO_VERDICT.itemsize), i64(3)
        self.valid, self.utf8_result = i64(n), i64(4)

    def reset(self):
        self.state.zero_()
        self.proto.zero_()


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
    ng = min(1024, ns)
    order = np.random.default_rng(6).permutation(ns).astype(np.uint32)
    gf = (np.arange(ng + 1, dtype=np.uint64) * ns // ng).astype(np.uint32)
    d_order, d_gf = torch.from_numpy(order.view(np.int32)).cuda(), torch.from_numpy(gf.view(np.int32)).cuda()
    echo, one, many, zero = (Outputs(n, ns, rcap, g) for g in (1, 1, ng, ng))

    def run_echo():
        o = echo
        codec.reply_validated(wire, fs, sf, proto=o.proto, role=ca.PROTO_SERVER, max_message=LIMIT, which=WHICH,
                              reply_op=ca.ECHO_REPLY, mask=False, state=o.state, reply=o.reply, reply_cap=rcap,
                              reply_off=o.reply_off, stream_reply=o.stream_reply, close_off=o.close_off,
                              verdict=o.verdict, result=o.result, valid=o.valid, utf8_result=o.utf8_result,
                              msgs=o.msgs, count=o.count, info=o.info)

    def run_relay(o, rooms, reply_op=ca.CHAT_REPLY, relay_op=ca.CHAT_RELAY):
        codec.relay_validated(wire, fs, sf, proto=o.proto, role=ca.PROTO_SERVER, max_message=LIMIT, which=WHICH,
                              reply_op=reply_op, mask=False, relay_op=relay_op, order=d_order if rooms else None,
                              group_first=d_gf if rooms else None, state=o.state, reply=o.reply, reply_cap=rcap,
                              relay=o.relay, relay_cap=rcap, reply_off=o.reply_off, stream_reply=o.stream_reply,
                              close_off=o.close_off, relay_off=o.relay_off, group_relay=o.group_relay,
                              verdict=o.verdict, result=o.result, valid=o.valid, utf8_result=o.utf8_result,
                              msgs=o.msgs, count=o.count, info=o.info)

    def fail(what):
        raise SystemExit("%s: %s" % (name, what))

    # once untimed, verified: nothing below fails silently
    for o in (echo, one, many, zero):
        o.reset()
    run_echo()
    run_relay(one, False)
    run_relay(many, True)
    run_relay(zero, True, ca.CHAT_REPLY, NONE)
    if codec.sync_status() != 0:
        fail("an error was latched")
    nm = int(one.count[0].item())
    msgs = one.msgs.cpu().numpy()[: nm * MSG.itemsize].view(MSG)
    verdict = one.verdict.cpu().numpy()[: ns * 8].view(PROTO_VERDICT)
    h_echo_off = echo.reply_off.cpu().numpy().view(np.uint64)
    h_echo, sample = echo.reply.cpu().numpy(), np.random.default_rng(7).permutation(nm)[:4096]
    for o, order_, gf_ in ((one, None, None), (many, order, gf)):
        want_off, want_group, want_count = layout.relay_plan(msgs, verdict, ca.CHAT_RELAY, order_, gf_)
        if not np.array_equal(o.relay_off.cpu().numpy().view(np.uint64)[:nm], want_off):
            fail("d_relay_off differs from layout.relay_plan")
        if not np.array_equal(o.group_relay.cpu().numpy().view(np.uint64)[: len(want_group)], want_group):
            fail("d_group_relay differs from layout.relay_plan")
        if [int(x) for x in o.count.cpu().numpy().view(np.uint64)[5:8]] != [int(x) for x in want_count]:
            fail("d_count[5..8) differs from layout.relay_plan")
        if int(want_count[0]) != int(echo.count[2].item()) - 4 * int(echo.count[4].item()):
            fail("the relay's bytes are not the echo's without its close frames")
        for name_, k in (("reply", int(zero.count[2].item())), ("reply_off", nm + 1), ("stream_reply", ns + 1),
                         ("close_off", ns), ("verdict", ns * 8), ("proto", ns * PROTO_STATE.itemsize), ("result", 3),
                         ("msgs", nm * MSG.itemsize), ("info", n * RECV_INFO.itemsize),
                         ("state", ns * STREAM_STATE.itemsize), ("valid", nm), ("utf8_result", 4)):
            if not torch.equal(getattr(o, name_)[:k], getattr(zero, name_)[:k]):
                fail("d_%s differs from the call's under relay_op all zero" % name_)
        h_relay = o.relay.cpu().numpy()
        for q in sample:
            at = int(want_off[q])
            if at == U64_MAX:
                continue
            size = layout.frame_size(0x81, False, int(msgs["len"][q]))
            e = int(h_echo_off[q])
            if h_relay[at] != 0x81 or not np.array_equal(h_relay[at + 1: at + size], h_echo[e + 1: e + size]):
                fail("a relay frame differs from the echo's")
    relay_bytes, relay_frames = int(one.count[5].item()), int(one.count[6].item())
    calls = (run_echo, lambda: run_relay(one, False), lambda: run_relay(many, True))
    outs = (echo, one, many)
    for _ in range(warmup):
        for o, f in zip(outs, calls):
            o.reset()
            f()
    codec.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    times = [[], [], []]
    for _ in range(reps):   # interleaved: the calls see the same machine state
        for o in outs:
            o.reset()
        for k, f in enumerate(calls):
            ev[2 * k].record()
            f()
            ev[2 * k + 1].record()
        ev[5].synchronize()
        for k in range(3):
            times[k].append(ev[2 * k].elapsed_time(ev[2 * k + 1]) * 1e3)
    codec.sync()
    # the gathers through the timing hook
    codec.timing(True)
    codec.timing_read(reset=True)
    gathers = [[], [], []]
    for _ in range(reps):
        for k, (o, f) in enumerate(zip(outs, calls)):
            o.reset()
            f()
            ms, launches = codec.timing_read(reset=True)
            assert launches == (1 if k == 0 else 2)
            gathers[k].append(ms * 1e3)
    codec.timing(False)
    codec.sync()
    t, g = [stats(x) for x in times], [stats(x) for x in gathers]
    res = {"frames": n, "streams": ns, "rooms": ng, "messages": nm, "relay_bytes": relay_bytes,
           "relay_frames": relay_frames, "closed_streams": int(echo.count[4].item()),
           "echo": {"call": t[0], "gather": g[0]}}
    for k, key in ((1, "relay_1"), (2, "relay_%d" % ng)):
        slower = g[k]["median_us"] - g[0]["median_us"]
        res[key] = {"call": t[k], "gathers": g[k], "ratio": round(t[k]["median_us"] / t[0]["median_us"], 4),
                    "plan_excess_us": round((t[k]["median_us"] - g[k]["median_us"]) -
                                            (t[0]["median_us"] - g[0]["median_us"]), 2),
                    "gather_ratio": round(g[k]["median_us"] / g[0]["median_us"], 4),
                    "gather_within_spread": bool(slower <= g[0]["max_us"] - g[0]["min_us"])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--shapes", default="c2,c3_frag,small", help="which shapes, comma-separated")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "relaybench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.shapes.split(","):
        desc, total, sf = shape(name, a.small)
        res["shapes"][name] = measure(codec, name, desc, total, sf, a.reps, a.warmup)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
