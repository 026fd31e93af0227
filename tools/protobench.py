"""wsg_check_protocol against wsg_decode_messages' plan on the same batch, the
two calls interleaved in one process.  The plan kernels are the yardstick:
they do the same kind of work, one lane per frame over d_info with block scans
and one block over the partials in between.

Shapes:
  c2        4096 x 64 KiB masked frames, one frame per message, one stream per
            frame
  c3_frag   tools/msgbench.py's: 65536 ragged frames (uniform in [128, 65536])
            in 4096 streams of 16 frames, messages of 1-8 fragments
  small     1 Mi x 32-byte masked frames in 1024 streams of 1024 frames,
            messages of 1-8 fragments

Every frame is masked and the role is WSG_PROTO_SERVER; one stream in 64 gets
a frame with a reserved opcode, so that verdicts other than "none" are
produced and checked.  Before any timing d_verdict, d_proto and d_result are
compared with layout.protocol_plan over the d_info read back.

Times, median / min / max microseconds over the repetitions (`spread` = (max -
min) / median):
  k_proto_judge       the per-frame judging kernel, from the wsg_timing hook
  check_call          the whole wsg_check_protocol call (four kernels), device
                      events around it
  k_msg_gather        wsg_decode_messages' payload kernel, from the hook
  decode_call         the whole wsg_decode_messages call, device events
  msg_plan            decode_call - k_msg_gather of the same repetition: the six
                      plan kernels (and the gaps between the launches)
`bytes` are the check's algorithmic bytes: 32 per frame, the stream table,
d_proto read and written, d_verdict, d_result and 2 per close frame;
frac_of_8TBps is taken on check_call.  time_ratio = check_call / msg_plan.
Prints one JSON line.

usage: python tools/protobench.py [--reps 40] [--warmup 10] [--small] [--shapes c2,c3_frag,small]
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
from cppserver_amd import layout  # noqa: E402
from cppserver_amd import workloads as wl  # noqa: E402
from cppserver_amd.layout import MSG, PROTO_STATE, PROTO_VERDICT, RECV_INFO, STREAM_STATE  # noqa: E402
from tools.msgbench import fragment_opcodes  # noqa: E402

PEAK = 8e12   # HBM bytes/s
LIMIT = 1 << 20


def shape(name, small):
    """(descriptors, payload bytes, stream_first) of a shape."""
    rng = np.random.default_rng(3)
    if name == "c2":
        n, size = (64, 4096) if small else (4096, 65536)
        desc, total = wl.ragged_desc(rng, np.full(n, size))
        sf = np.arange(n + 1, dtype=np.int32)
    elif name == "c3_frag":
        n, per_stream, hi = (1024, 16, 4096) if small else (65536, 16, 65536)
        desc, total = wl.ragged_desc(rng, rng.integers(128, hi + 1, n))
        desc["opcode"] = fragment_opcodes(rng, n, per_stream)
        sf = np.arange(0, n + 1, per_stream, dtype=np.int32)
    else:
        n, per_stream = (4096, 256) if small else (1 << 20, 1024)
        desc, total = wl.ragged_desc(rng, np.full(n, 32))
        desc["opcode"] = fragment_opcodes(rng, n, per_stream)
        sf = np.arange(0, n + 1, per_stream, dtype=np.int32)
    ns = len(sf) - 1
    for j in range(0, ns, 64):   # a reserved opcode somewhere in one stream of 64
        lo, hi = int(sf[j]), int(sf[j + 1])
        desc["opcode"][lo + int(rng.integers(0, hi - lo))] = 0x83
    return desc, total, sf


def stats(us):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "spread": round((max(us) - min(us)) / med, 4)}


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
    info = torch.empty(n * RECV_INFO.itemsize, dtype=torch.uint8, device="cuda")
    msg = torch.empty(cap, dtype=torch.uint8, device="cuda")
    msgs = torch.empty(n * MSG.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
    proto = torch.zeros(ns * PROTO_STATE.itemsize, dtype=torch.uint8, device="cuda")
    verdict = torch.empty(ns * PROTO_VERDICT.itemsize, dtype=torch.uint8, device="cuda")
    result = torch.empty(3, dtype=torch.int64, device="cuda")

    def messages():
        state.zero_()
        codec.decode_messages(wire, fs, sf, state=state, msg=msg, msgs=msgs, count=count, info=info)

    def check():
        proto.zero_()
        codec.check_protocol(wire, info, n, sf, proto=proto, role=ca.PROTO_SERVER, max_message=LIMIT, state=state,
                             verdict=verdict, result=result)

    # once untimed, verified against the numpy restatement: nothing below fails silently
    messages()
    check()
    codec.sync()
    h_info = info.cpu().numpy().view(RECV_INFO)
    consumed = state.cpu().numpy().view(STREAM_STATE)["consumed"]
    closes = int((h_info["opcode"] == 8).sum())
    want_v, want_p, want_r = layout.protocol_plan(h_info, stream_first, None, ca.PROTO_SERVER, LIMIT,
                                                  wire.cpu().numpy() if closes else np.zeros(0, dtype=np.uint8), consumed)
    if not np.array_equal(verdict.cpu().numpy().view(np.uint64), want_v.view(np.uint64)):
        raise SystemExit("%s: d_verdict differs from layout.protocol_plan" % name)
    if not np.array_equal(proto.cpu().numpy().view(np.uint64), want_p.view(np.uint64)):
        raise SystemExit("%s: d_proto differs from layout.protocol_plan" % name)
    if not np.array_equal(result.cpu().numpy().view(np.uint64), want_r):
        raise SystemExit("%s: d_result %r, expected %r" % (name, result.cpu().tolist(), want_r.tolist()))
    if int(want_r[0]) != len(range(0, ns, 64)):
        raise SystemExit("%s: %d violating streams, built for %d" % (name, int(want_r[0]), len(range(0, ns, 64))))
    for _ in range(warmup):
        messages()
        check()
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_gather, t_decode, t_judge, t_check = [], [], [], []
    for _ in range(reps):   # interleaved: both calls see the same machine state
        state.zero_()
        ev[0].record()
        codec.decode_messages(wire, fs, sf, state=state, msg=msg, msgs=msgs, count=count, info=info)
        ev[1].record()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_gather.append(ms * 1e3)
        proto.zero_()
        ev[2].record()
        codec.check_protocol(wire, info, n, sf, proto=proto, role=ca.PROTO_SERVER, max_message=LIMIT, state=state,
                             verdict=verdict, result=result)
        ev[3].record()
        ev[3].synchronize()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_judge.append(ms * 1e3)
        t_decode.append(ev[0].elapsed_time(ev[1]) * 1e3)
        t_check.append(ev[2].elapsed_time(ev[3]) * 1e3)
    codec.timing(False)
    codec.sync()
    t_plan = [d - g for d, g in zip(t_decode, t_gather)]
    nbytes = RECV_INFO.itemsize * n + 4 * (ns + 1) + 2 * PROTO_STATE.itemsize * ns + PROTO_VERDICT.itemsize * ns + \
        STREAM_STATE.itemsize * ns + 3 * 8 + 2 * closes
    c, p = stats(t_check), stats(t_plan)
    c.update(bytes=nbytes, frac_of_8TBps=round(nbytes / (c["median_us"] * 1e-6) / PEAK, 5))
    return {"frames": n, "streams": ns, "violating_streams": int(want_r[0]), "k_proto_judge": stats(t_judge),
            "check_call": c, "k_msg_gather": stats(t_gather), "decode_call": stats(t_decode), "msg_plan": p,
            "time_ratio": round(c["median_us"] / p["median_us"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    ap.add_argument("--shapes", default="c2,c3_frag,small", help="which shapes, comma-separated (one alone for a trace)")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "protobench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.shapes.split(","):
        desc, total, sf = shape(name, a.small)
        res["shapes"][name] = measure(codec, name, desc, total, sf, a.reps, a.warmup)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
