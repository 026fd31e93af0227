"""Register/occupancy report for k_decode and source variants with paths cut
out (which path sets the kernel's VGPR count), for the encode, lane, fan-out
and XOR kernels, and for k_msg_gather
(wsg_decode_messages; wsg_reply_messages runs it too), the reply plan, the
framer, the UTF-8 check (dense and from the wire), the protocol check,
the checked reply (wsg_reply_checked), the upgrade handshake (wsg_upgrade_streams), its client half
(wsg_upgrade_client_streams, wsg_upgrade_requests), the carry
(wsg_carry_streams) and the relay plan (wsg_relay_validated).  Compiles for gfx950 only (no GPU needed).

usage: python tools/regs.py
"""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name):
    with open(os.path.join(ROOT, "cppserver_amd", "csrc", name)) as f:
        return f.read()


def report(text, tag, kernel="_ZN3wsg8k_decode"):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "k.hip")
        with open(path, "w") as f:
            f.write(text)
        r = subprocess.run(
            ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
             "-I" + os.path.join(ROOT, "cppserver_amd", "csrc"), "--cuda-device-only", "-S", "-o",
             os.path.join(d, "k.s"), path, "-Rpass-analysis=kernel-resource-usage"],
            capture_output=True, text=True)
    out = r.stderr
    i = out.find("Function Name: " + kernel)
    block = out[i:i + 2500] if i >= 0 else ""

    def g(k):
        m = re.search(k + r": (\d+)", block)
        return m.group(1) if m else "?"
    print("%-28s VGPR %s SGPR %s sspill %s vspill %s scratch %s occ %s" % (
        tag, g(" VGPRs"), g("TotalSGPRs"), g("SGPRs Spill"), g("VGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
        g(r"Occupancy \[waves/SIMD\]")))


def cut(text, marker):
    assert marker in text, marker
    return text.replace(marker, "return;\n" + marker, 1)   # inside process_tile


if __name__ == "__main__":
    src = source("wsg_decode.hip")
    staged = "    // staged: payload segments in LDS"
    boundary = "        // boundary: per chunk"
    report(src, "full")
    report(cut(src, staged), "no-staged")
    report(cut(src, boundary), "no-boundary")
    report(cut(cut(src, staged), boundary), "no-staged-no-boundary")
    for name, kernels in (("wsg_encode.hip", ("k_encode_mask", "k_encode_small", "k_encode_finalize")),
                          ("wsg_lane_device.hip", ("k_lane",)),
                          ("wsg_fanout.hip", ("k_fanout_flat", "k_fanout_period<1>", "k_fanout_period<2>",
                                              "k_fanout_period<4>")),
                          ("wsg_misc.hip", ("k_xor",)),
                          ("wsg_messages.hip", ("k_msg_gather", "k_msg_finalize", "k_reply_local<0>", "k_reply_blocks<0>",
                                                "k_reply_finalize<0>", "k_msg_consumed", "k_reply_local<1>",
                                                "k_reply_blocks<1>", "k_reply_finalize<1>")),
                          ("wsg_assembly.hip", ("k_rfc_scan_local", "k_rfc_scan_blocks", "k_rfc_bytes_local",
                                                "k_rfc_bytes_blocks", "k_rfc_finalize", "k_rfc_state<0>", "k_rfc_state<1>",
                                                "k_rfc_reply_local<0>", "k_rfc_reply_local<1>",
                                                "k_rfc_reply_finalize<0>", "k_rfc_reply_finalize<1>")),
                          ("wsg_frames.hip", ("k_frame_count", "k_frame_write")),
                          ("wsg_utf8.hip", ("k_utf8_init", "k_utf8_scan", "k_utf8_count", "k_utf8_verdict_seed", "k_utf8_verdicts",
                                            "k_utf8_wire", "k_utf8_also_seed")),
                          ("wsg_proto.hip", ("k_proto_local", "k_proto_blocks", "k_proto_judge", "k_proto_finish",
                                             "k_proto_merge")),
                          ("wsg_upgrade.hip", ("k_upgrade_parse", "k_upgrade_scan_local", "k_upgrade_scan_blocks",
                                               "k_upgrade_accept", "k_upgrade_respond")),
                          ("wsg_upgrade_client.hip", ("k_upclient_expect", "k_upclient_parse", "k_upclient_count_local",
                                                      "k_upclient_count_blocks", "k_upgrade_requests")),
                          ("wsg_carry.hip", ("k_carry_sizes", "k_carry_scan_blocks", "k_carry_spans", "k_carry_copy")),
                          ("wsg_relay.hip", ("k_relay_local", "k_relay_frames<0>", "k_relay_frames<1>", "k_relay_blocks",
                                             "k_relay_streams_local", "k_relay_streams_blocks", "k_relay_finalize"))):
        src = source(name)
        for k in kernels:
            base, _, flag = k.partition("<")   # name<0|1>: an instantiation of a template on one bool (the fan-out's: one int)
            kind = "i" if base == "k_fanout_period" else "b"
            report(src, k, kernel="_ZN3wsg%d%s" % (len(base), base) + ("IL%s%sEE" % (kind, flag[0]) if flag else ""))
