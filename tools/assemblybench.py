"""wsg_reply_validated under WSG_ASSEMBLY_REFERENCE and under WSG_ASSEMBLY_RFC
on the same wire in one process, the two interleaved, with device events
around each call; and the gather's time through the wsg_timing hook (the
call's dominant kernel: what is left of the call is its plan kernels and the
UTF-8 check).

Shapes and corpora: tools/validbench.py's (c2, c3_frag; ascii, mixed,
corrupt): no control frame lies between fragments, so both rules assemble the
same messages.  Before any timing every output of the RFC call is compared
with the reference call's (d_reply, d_reply_off, d_stream_reply, d_close_off,
d_verdict, d_proto, d_result, d_msgs, d_count, d_info, d_valid, the UTF-8
result and d_state's consumed; the state's opcode is the reference's alone).

Times, median / min / max microseconds over the repetitions.  extra_us = RFC's
median - the reference's; gather_ratio = the gather under RFC over the gather
under the reference (1.0 when the piece records are equally good).
Prints one JSON line.

usage: python tools/assemblybench.py [--reps 40] [--warmup 10] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cppserver_amd as ca  # noqa: E402
from cppserver_amd.layout import MSG, PROTO_STATE, RECV_INFO, STREAM_STATE  # noqa: E402
from tools.utf8bench import Shape, fill, stats, text_pool  # noqa: E402
from tools.validbench import WHICH, Outputs  # noqa: E402

MODES = (("reference", ca.ASSEMBLY_REFERENCE), ("rfc", ca.ASSEMBLY_RFC))


def measure(codec, shape, corpus, payload, want, reps, warmup):
    n, ns, nmsg = shape.n, len(shape.stream_first) - 1, len(shape.msg_len)
    cap = int(ca.frame_sizes(shape.desc).sum())
    wire = torch.empty(cap, dtype=torch.uint8, device="cuda")
    woff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode_batch(payload, ca.desc_to_tensor(shape.desc, "cuda"), wire=wire, wire_cap=cap, wire_off=woff)
    codec.sync()
    fs, sf = woff[:n].contiguous(), torch.from_numpy(shape.stream_first).cuda()
    rcap = cap + 14 * n
    outs = {name: Outputs(n, ns, rcap) for name, _ in MODES}

    def call(name, mode):
        o = outs[name]
        o.reset()
        codec.set_assembly(mode)
        codec.reply_validated(wire, fs, sf, proto=o.proto, role=ca.PROTO_SERVER, which=WHICH, state=o.state,
                              reply=o.reply, reply_cap=rcap, reply_off=o.reply_off, stream_reply=o.stream_reply,
                              close_off=o.close_off, verdict=o.verdict, result=o.result, valid=o.valid,
                              utf8_result=o.utf8_result, msgs=o.msgs, count=o.count, info=o.info)

    def fail(what):
        raise SystemExit("%s/%s: %s" % (shape.name, corpus, what))

    for name, mode in MODES:
        call(name, mode)
    if codec.sync_status() != 0:
        fail("an error was latched")
    ref, rfc = outs["reference"], outs["rfc"]
    nm, total = int(ref.count[0].item()), int(ref.count[2].item())
    if nm != nmsg or not np.array_equal(ref.valid[:nm].cpu().numpy(), want):
        fail("d_valid differs from the corpus")
    for name, k in (("reply", total), ("reply_off", nm + 1), ("stream_reply", ns + 1), ("close_off", ns),
                    ("verdict", ns * 8), ("proto", ns * PROTO_STATE.itemsize), ("result", 3),
                    ("msgs", nm * MSG.itemsize), ("count", 5), ("info", n * RECV_INFO.itemsize), ("valid", nm),
                    ("utf8_result", 4)):
        if not torch.equal(getattr(rfc, name)[:k], getattr(ref, name)[:k]):
            fail("d_%s differs between the modes" % name)
    st = [o.state.cpu().numpy().view(STREAM_STATE) for o in (ref, rfc)]
    if not np.array_equal(st[0]["consumed"], st[1]["consumed"]) or st[1]["opcode"].any() or st[1]["ahead"].any():
        fail("d_state differs between the modes")
    for _ in range(warmup):
        for name, mode in MODES:
            call(name, mode)
    codec.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    times = {name: [] for name, _ in MODES}
    for _ in range(reps):   # interleaved: the calls see the same machine state
        for k, (name, mode) in enumerate(MODES):
            outs[name].reset()
        for k, (name, mode) in enumerate(MODES):
            codec.set_assembly(mode)
            o = outs[name]
            ev[2 * k].record()
            codec.reply_validated(wire, fs, sf, proto=o.proto, role=ca.PROTO_SERVER, which=WHICH, state=o.state,
                                  reply=o.reply, reply_cap=rcap, reply_off=o.reply_off, stream_reply=o.stream_reply,
                                  close_off=o.close_off, verdict=o.verdict, result=o.result, valid=o.valid,
                                  utf8_result=o.utf8_result, msgs=o.msgs, count=o.count, info=o.info)
            ev[2 * k + 1].record()
        ev[3].synchronize()
        for k, (name, _) in enumerate(MODES):
            times[name].append(ev[2 * k].elapsed_time(ev[2 * k + 1]) * 1e3)
    codec.sync()
    codec.timing(True)
    codec.timing_read(reset=True)
    gather = {name: [] for name, _ in MODES}
    for _ in range(reps):
        for name, mode in MODES:
            call(name, mode)
            ms, k = codec.timing_read(reset=True)
            assert k == 1
            gather[name].append(ms * 1e3)
    codec.timing(False)
    codec.set_assembly(ca.ASSEMBLY_REFERENCE)
    codec.sync()
    t = {name: stats(times[name]) for name, _ in MODES}
    g = {name: stats(gather[name]) for name, _ in MODES}
    return {"messages": nmsg, "frames": n, "payload_bytes": shape.total, "reply_bytes": total,
            "reference": t["reference"], "rfc": t["rfc"],
            "extra_us": round(t["rfc"]["median_us"] - t["reference"]["median_us"], 2),
            "time_ratio": round(t["rfc"]["median_us"] / t["reference"]["median_us"], 4),
            "gather_reference": g["reference"], "gather_rfc": g["rfc"],
            "gather_ratio": round(g["rfc"]["median_us"] / g["reference"]["median_us"], 4),
            "rest_reference_us": round(t["reference"]["median_us"] - g["reference"]["median_us"], 2),
            "rest_rfc_us": round(t["rfc"]["median_us"] - g["rfc"]["median_us"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="toy sizes (a check of the tool, not a measurement)")
    a = ap.parse_args()
    codec = ca.Codec(0)
    res = {"tool": "assemblybench", "reps": a.reps, "warmup": a.warmup, "small": a.small,
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
