"""wsg_reply_messages against the two calls it replaces, wsg_decode_messages
then wsg_encode_batch over d_msg, on the same wire: kernel times from the
wsg_timing hook (k_msg_gather with the reply wire as destination; k_msg_gather
into d_msg plus the encode's payload kernel), the calls interleaved in one
process.  The echo rule (layout.ECHO_REPLY), mask = 0, send keys 0.

Shapes (tools/msgbench.py's):
  c2        the C2 wire, 4096 x 64 KiB masked frames, one frame per message,
            one stream per frame
  c3_frag   65536 ragged frames (C3's lengths, uniform in [128, 65536]) in 4096
            streams of 16 frames, messages of 1-8 fragments

The two-call route's descriptors (one binary frame per message over d_msg)
are built once from the message table, outside the timing; the host round
trip it needs between its calls is not in its figure either.  Per shape and
leg: median / min / max kernel microseconds and spread = (max - min) / median
over the repetitions; `reply_over_two_calls` and `reply_over_gather` are
ratios of medians (the second against k_msg_gather's own time in the
decode_messages leg).  Once, before the timing, the reply wire is compared
with the two-call route's.  Prints one JSON line.

usage: python tools/replybench.py [--reps 40] [--warmup 10] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cppserver_amd as ca  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, SEND_DESC, STREAM_STATE  # noqa: E402
from tools.msgbench import shape_c2, shape_c3_frag, stats  # noqa: E402


def measure(codec, name, wire, fs, sf, payload_bytes, reps, warmup):
    n, ns = int(fs.numel()), int(sf.numel()) - 1
    wire_len = int(wire.numel())
    info = torch.empty(n * RECV_INFO.itemsize, dtype=torch.uint8, device="cuda")
    msg = torch.empty(wire_len, dtype=torch.uint8, device="cuda")
    msgs = torch.empty(n * MSG.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(4, dtype=torch.int64, device="cuda")
    state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
    cap = wire_len + 14 * n
    reply = torch.empty(cap, dtype=torch.uint8, device="cuda")
    reply_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    stream_reply = torch.empty(ns + 1, dtype=torch.int64, device="cuda")
    wire2 = torch.empty(cap, dtype=torch.uint8, device="cuda")

    def replies():
        state.zero_()
        codec.reply_messages(wire, fs, sf, reply_op=ca.ECHO_REPLY, mask=False, state=state, reply=reply,
                             reply_cap=cap, reply_off=reply_off, stream_reply=stream_reply, msgs=msgs, count=count,
                             info=info)

    def messages():
        state.zero_()
        codec.decode_messages(wire, fs, sf, state=state, msg=msg, msgs=msgs, count=count[:2], info=info)

    # once untimed, checked: the route that exists without the call, its descriptors from the table
    messages()
    codec.sync()
    nm, used = int(count[0]), int(count[1])
    if used != payload_bytes:
        raise SystemExit("%s: %d message bytes, expected %d" % (name, used, payload_bytes))
    table = msgs.cpu().numpy().view(MSG)[:nm]
    if not (table["kind"] == ca.CB_RECEIVED).all():
        raise SystemExit("%s: a message that is not data" % name)
    desc = np.zeros(nm, dtype=SEND_DESC)
    desc["src_off"], desc["len"], desc["opcode"] = table["off"], table["len"], ca.WS_FIN | ca.WS_BINARY
    d_desc = ca.desc_to_tensor(desc, "cuda")
    woff = torch.empty(nm + 1, dtype=torch.int64, device="cuda")

    def encode():
        codec.encode_batch(msg, d_desc, wire=wire2, wire_cap=cap, wire_off=woff)

    encode()
    replies()
    codec.sync()
    cnt = [int(x) for x in count.cpu()]
    total = int(woff[nm])
    if cnt[:2] != [nm, used] or cnt[2] != total or cnt[3] != nm:
        raise SystemExit("%s: counts %r, the two calls give %r" % (name, cnt, [nm, used, total, nm]))
    if not torch.equal(reply[:total], wire2[:total]) or not torch.equal(reply_off[: nm + 1], woff):
        raise SystemExit("%s: the reply wire is not the two calls' wire" % name)
    for _ in range(warmup):
        replies()
        messages()
        encode()
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    t = {"reply_messages": [], "decode_messages": [], "encode_batch": []}
    for _ in range(reps):   # interleaved: every call sees the same machine state
        for leg, call in (("reply_messages", replies), ("decode_messages", messages), ("encode_batch", encode)):
            call()
            ms, k = codec.timing_read(reset=True)
            assert k >= 1
            t[leg].append(ms * 1e3)
    codec.timing(False)
    codec.sync()
    res = {leg: stats(us) for leg, us in t.items()}
    two = [a + b for a, b in zip(t["decode_messages"], t["encode_batch"])]
    res["two_calls"] = stats(two)
    # algorithmic bytes of the payload kernels: the payload read and written once, or twice
    res["reply_messages"]["payload_traffic_bytes"] = 2 * payload_bytes
    res["two_calls"]["payload_traffic_bytes"] = 4 * payload_bytes
    r = res["reply_messages"]["median_us"]
    return dict(frames=n, streams=ns, messages=nm, wire_bytes=wire_len, payload_bytes=payload_bytes,
                reply_bytes=total, **res,
                reply_over_two_calls=round(r / res["two_calls"]["median_us"], 4),
                reply_over_gather=round(r / res["decode_messages"]["median_us"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "replybench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    wire, fs, sf, total, _ = shape_c2(a.small)
    res["shapes"]["c2"] = measure(codec, "c2", wire, fs, sf, total, a.reps, a.warmup)
    del wire, fs, sf
    torch.cuda.empty_cache()
    wire, fs, sf, total, _ = shape_c3_frag(codec, a.small)
    res["shapes"]["c3_frag"] = measure(codec, "c3_frag", wire, fs, sf, total, a.reps, a.warmup)
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
