"""wsg_reply_validated against the chain of calls it replaces, on the same wire
in one process, the two interleaved:
  chain   wsg_decode_messages -> wsg_check_utf8 -> wsg_utf8_verdicts ->
          wsg_reply_checked(d_also): the payload read three times and written
          twice, the plan pass run twice
  fused   wsg_reply_validated: the payload read twice and written once, one
          plan pass
with device events around each; and k_utf8_wire (wsg_check_utf8_wire) against
k_utf8_scan (wsg_check_utf8) on the same text through the wsg_timing hook.

Shapes and corpora: tools/utf8bench.py's (c2, c3_frag; ascii, mixed, corrupt),
every message text, every frame masked, the role WSG_PROTO_SERVER.

Before any timing every output of the fused call is compared with the
chain's (d_reply, d_reply_off, d_stream_reply, d_close_off, d_verdict,
d_proto, d_result, d_msgs, d_count, d_info, d_state, d_valid, the UTF-8
result), d_valid with what the corpus was built to give, and
wsg_check_utf8_wire's d_valid and d_result with wsg_check_utf8's.

Times, median / min / max microseconds over the repetitions (`spread` = (max -
min) / median).  saved_us = chain's median - fused's; not_slower says whether
the fused call's median is at most the chain's, or above it by no more than
the fused call's own max - min.  kernel_ratio = k_utf8_wire / k_utf8_scan.
Prints one JSON line.

usage: python tools/validbench.py [--reps 40] [--warmup 10] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cppserver_amd as ca  # noqa: E402
from cppserver_amd.layout import MSG, PROTO_STATE, PROTO_VERDICT, RECV_INFO, STREAM_STATE  # noqa: E402
from tools.utf8bench import Shape, fill, stats, text_pool  # noqa: E402

WHICH = ca.UTF8_TEXT | ca.UTF8_CLOSE


class Outputs:
    def __init__(self, n, ns, cap):
        u8 = lambda k: torch.empty(max(k, 16), dtype=torch.uint8, device="cuda")  # noqa: E731
        i64 = lambda k: torch.empty(k, dtype=torch.int64, device="cuda")  # noqa: E731
        self.reply, self.reply_off, self.stream_reply, self.close_off = u8(cap), i64(n + 1), i64(ns + 1), i64(ns)
        self.msgs, self.info, self.count = u8(n * MSG.itemsize), u8(n * RECV_INFO.itemsize), i64(5)
        self.state = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.proto = torch.zeros(ns * PROTO_STATE.itemsize, dtype=torch.uint8, device="cuda")
        self.verdict, self.result = u8(ns * PROTO_VERDICT.itemsize), i64(3)
        self.valid, self.utf8_result = i64(n), i64(4)

    def reset(self):
        self.state.zero_()
        self.proto.zero_()


def measure(codec, shape, corpus, payload, want, reps, warmup):
    n, ns, nmsg = shape.n, len(shape.stream_first) - 1, len(shape.msg_len)
    cap = int(ca.frame_sizes(shape.desc).sum())
    wire = torch.empty(cap, dtype=torch.uint8, device="cuda")
    woff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode_batch(payload, ca.desc_to_tensor(shape.desc, "cuda"), wire=wire, wire_cap=cap, wire_off=woff)
    codec.sync()
    fs, sf = woff[:n].contiguous(), torch.from_numpy(shape.stream_first).cuda()
    rcap = cap + 14 * n
    two, one = Outputs(n, ns, rcap), Outputs(n, ns, rcap)
    msg = torch.empty(cap, dtype=torch.uint8, device="cuda")
    dstate = torch.zeros(ns * STREAM_STATE.itemsize, dtype=torch.uint8, device="cuda")
    dmsgs, dinfo = torch.empty_like(two.msgs), torch.empty_like(two.info)
    dcount = torch.zeros(2, dtype=torch.int64, device="cuda")
    also = torch.empty(ns * PROTO_VERDICT.itemsize, dtype=torch.uint8, device="cuda")
    wvalid, wresult = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")

    def decode():
        dstate.zero_()
        codec.decode_messages(wire, fs, sf, state=dstate, msg=msg, msgs=dmsgs, count=dcount, info=dinfo)

    def scan():
        codec.check_utf8(msg, dmsgs, dcount, which=WHICH, msg_cap=cap, msg_room=n, valid=two.valid,
                         result=two.utf8_result)

    def chain():
        decode()
        scan()
        codec.utf8_verdicts(dmsgs, dcount, two.valid, ns, WHICH, msg_room=n, also=also)
        codec.reply_checked(wire, fs, sf, proto=two.proto, role=ca.PROTO_SERVER, also=also, state=two.state,
                            reply=two.reply, reply_cap=rcap, reply_off=two.reply_off, stream_reply=two.stream_reply,
                            close_off=two.close_off, verdict=two.verdict, result=two.result, msgs=two.msgs,
                            count=two.count, info=two.info)

    def fused():
        codec.reply_validated(wire, fs, sf, proto=one.proto, role=ca.PROTO_SERVER, which=WHICH, state=one.state,
                              reply=one.reply, reply_cap=rcap, reply_off=one.reply_off, stream_reply=one.stream_reply,
                              close_off=one.close_off, verdict=one.verdict, result=one.result, valid=one.valid,
                              utf8_result=one.utf8_result, msgs=one.msgs, count=one.count, info=one.info)

    def from_wire():
        codec.check_utf8_wire(wire, fs, sf, state=dstate, which=WHICH, msgs=dmsgs, count=dcount, info=dinfo,
                              valid=wvalid, result=wresult)

    def fail(what):
        raise SystemExit("%s/%s: %s" % (shape.name, corpus, what))

    # once untimed, verified: nothing below fails silently
    two.reset()
    one.reset()
    chain()
    fused()
    from_wire()
    if codec.sync_status() != 0:
        fail("an error was latched")
    nm = int(one.count[0].item())
    if nm != nmsg or not np.array_equal(one.valid[:nm].cpu().numpy(), want):
        fail("d_valid differs from the corpus")
    total = int(one.count[2].item())
    for name, k in (("reply", total), ("reply_off", nm + 1), ("stream_reply", ns + 1), ("close_off", ns),
                    ("verdict", ns * 8), ("proto", ns * PROTO_STATE.itemsize), ("result", 3),
                    ("msgs", nm * MSG.itemsize), ("count", 5), ("info", n * RECV_INFO.itemsize),
                    ("state", ns * STREAM_STATE.itemsize), ("valid", nm), ("utf8_result", 4)):
        if not torch.equal(getattr(one, name)[:k], getattr(two, name)[:k]):
            fail("d_%s differs from the chain's" % name)
    if not torch.equal(wvalid[:nm], two.valid[:nm]) or not torch.equal(wresult, two.utf8_result):
        fail("wsg_check_utf8_wire differs from wsg_check_utf8")
    closed = int(one.count[4].item())
    for _ in range(warmup):
        two.reset()
        one.reset()
        chain()
        fused()
    codec.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_chain, t_fused = [], []
    for _ in range(reps):   # interleaved: the calls see the same machine state
        two.reset()
        one.reset()
        ev[0].record()
        chain()
        ev[1].record()
        ev[2].record()
        fused()
        ev[3].record()
        ev[3].synchronize()
        t_chain.append(ev[0].elapsed_time(ev[1]) * 1e3)
        t_fused.append(ev[2].elapsed_time(ev[3]) * 1e3)
    codec.sync()
    # the two payload kernels through the timing hook
    decode()
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    t_scan, t_wire = [], []
    for _ in range(reps):
        scan()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_scan.append(ms * 1e3)
        from_wire()
        ms, k = codec.timing_read(reset=True)
        assert k == 1
        t_wire.append(ms * 1e3)
    codec.timing(False)
    codec.sync()
    c, f, s, w = stats(t_chain), stats(t_fused), stats(t_scan), stats(t_wire)
    saved = round(c["median_us"] - f["median_us"], 2)
    return {"messages": nmsg, "frames": n, "payload_bytes": shape.total, "closed_streams": closed, "reply_bytes": total,
            "chain": c, "fused": f, "saved_us": saved, "time_ratio": round(f["median_us"] / c["median_us"], 4),
            "not_slower": bool(saved >= -(f["max_us"] - f["min_us"])),
            "k_utf8_scan": s, "k_utf8_wire": w, "kernel_ratio": round(w["median_us"] / s["median_us"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "validbench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
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
            res["shapes"][name][corpus] = measure(codec, shape, corpus, payload, want, a.reps, a.warmup)
            del payload
            torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
